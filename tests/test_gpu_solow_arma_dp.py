"""GPU: the ARMA-state optimal-savings yardstick of the Solow env (grl_solow_arma_* of include/goldsrl_solowarmadp.h;
csrc/solow_arma_dp.hip) and the baseline class that chooses between it and the (k, z, e) solver.

The solve is held to the float64 numpy restatement of the recurrence (tests/_solow_arma_dp_oracle.py); the play to the per-step
path, as tests/test_gpu_solow_dp.py holds the first solver's: grl_step with the traced actions runs the same float32 operations in
the same order, so rewards, capital and their sequential sums must be the per-step path's bits."""
import ctypes as C

import numpy as np
import pytest

import _solow_arma_dp_oracle as AO
from test_gpu_solow_sweep import PAIR_KEYS, _snapshot_engine, _twin_stats

pytestmark = pytest.mark.gpu

ORDERS = [(1, 0), (1, 1), (1, 2), (3, 1), (2, 2), (3, 3)]
# Largest |value - oracle| / max(1, |oracle|) of stage 0 measured over the eight cases of test_solve_against_the_oracle: see that
# test's docstring.  The bound is ten times the measurement.
VALUE_MEASURED = 1.998e-15
VALUE_TOL = 10 * VALUE_MEASURED
# nk, nx (cut to the order's m), ns, horizon: unequal axes with 70 rates (the lanes wrap, no multiple of 64) over 24 stages, enough
# for saving to pay, so that the arg-max is interior (43 to 50 distinct rates in the oracle's tables, 15 to 31 in stage 0); the
# last stage alone on 33 k nodes; 300 k nodes, more than the 256 lanes that fill the slab
SOLVES = [(p, q, 5, (4, 3, 2, 3), 70, 24) for p, q in ORDERS] + [(2, 2, 33, (4, 3, 2), 4, 1), (1, 1, 300, (3, 2), 5, 12)]


def _m(p, q):
    return max(p, max(q, 1) + 1)


def _small_grid(p, q, **kw):
    from goldsrl._ffi_solowarmadp import solow_arma_dp_grid
    g = dict(nk=7, nx=(4, 3, 2, 3)[:_m(p, q)], nq=3, ns=8, k_lo=30.0, k_hi=120.0, sigma=0.1)
    g.update(kw)
    return solow_arma_dp_grid(p, q, **g)


# ------------------------------------------------------------------------------------------ 1. the solve and the model
@pytest.mark.parametrize("p,q,nk,nx,ns,horizon", SOLVES)
def test_solve_against_the_oracle(p, q, nk, nx, ns, horizon):
    """Measured: the largest |value - oracle| / max(1, |oracle|) of stage 0 over the eight cases is 1.998e-15, at 300 k nodes over
    12 stages; the 24-stage cases give 0 to 5.7e-16, the single stage 3.3e-16 (exp, log and pow of the device against numpy's); the
    bound is ten times the largest.  The oracle's smallest gap between the best and the second-best Q on these grids is 3.8e-7
    ((3,3), 24 stages; asserted above 1e-8), so every stage's policy must be the oracle's exactly."""
    from goldsrl import _ffi
    from goldsrl._ffi_solowarmadp import solow_arma_dp_grid, solow_arma_dp_solve
    grid = solow_arma_dp_grid(p, q, nk=nk, nx=nx[:_m(p, q)], nq=3, ns=ns, sigma=0.1)
    policy, value, gap = AO.solve(grid, horizon, grid["model"]["A"], grid["model"]["b"], 0.02)
    assert gap > 1e-8, gap
    eng = _ffi.Engine(_ffi.ENV_SOLOW, 3, solow_p=p, solow_q=q)
    got = solow_arma_dp_solve(eng, grid, horizon)
    assert got["policy"].shape == policy.shape and got["value"].shape == value.shape
    dev = float((np.abs(got["value"] - value) / np.maximum(1.0, np.abs(value))).max())
    print("solow_arma_dp value deviation order %s grid %s: %.3e (oracle gap %.3e)" % ((p, q), (nk, nx, ns, horizon), dev, gap))
    assert got["policy"].tobytes() == policy.tobytes()
    assert dev <= VALUE_TOL, dev
    eng.close()


@pytest.mark.parametrize("p,q", ORDERS)
def test_model_is_the_numpy_derivation(p, q):
    from goldsrl import _ffi
    from goldsrl._ffi_solowarmadp import handle_rhos, solow_arma_model_device
    eng = _ffi.Engine(_ffi.ENV_SOLOW, 1, solow_p=p, solow_q=q)
    got = solow_arma_model_device(eng)
    A, b, Mz, Me = AO.model(*handle_rhos(p, q))
    assert (got["m"], got["p"], got["q"]) == (_m(p, q), p, max(q, 1))
    for name, want in (("A", A), ("b", b), ("Mz", Mz), ("Me", Me), ("f_std", AO.f_std(A, b, eng.cfg.solow_sigma))):
        assert got[name].tobytes() == want.tobytes(), name             # the operation order is kept
    eng.close()


# ------------------------------------------------------------------------------------------ 2. the play is the per-step path
@pytest.mark.parametrize("p,q", [(2, 2), (3, 3)])
@pytest.mark.parametrize("E", [1, 64, 65, 130])
def test_play_is_the_per_step_path_bit_for_bit(E, p, q):
    from goldsrl._ffi_solowarmadp import solow_arma_dp_play, solow_arma_dp_policy_actions, solow_arma_dp_set_policy, table_shape
    n = 40
    eng = _snapshot_engine(E, p, q, seed=E + q)
    grid = _small_grid(p, q, x_max=(0.25, 0.2, 0.15, 0.1)[:_m(p, q)])    # tight: some states leave the box and take the edge
    tables = np.random.RandomState(E).uniform(size=table_shape(grid, 3)).astype(np.float32)
    solow_arma_dp_set_policy(eng, grid, tables)
    eng.reset()
    got = solow_arma_dp_play(eng, n, trace_steps=n)
    assert got["actions"].shape == (n, E) and got["actions"].dtype == np.float32
    eng.reset()
    rewards, ks = np.zeros((n, E), np.float32), np.zeros((n, E), np.float32)
    for t in range(n):
        want = solow_arma_dp_policy_actions(grid, tables[0], eng.get_state("SOLOW_K"), eng.get_state("SOLOW_Z"), eng.get_state("SOLOW_E"))
        ulps = np.abs(got["actions"][t].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (t, ulps.max())                          # no TimeLimit: stage 0 throughout
        eng.step(got["actions"][t][:, None])
        rewards[t], ks[t] = eng.read("reward"), eng.get_state("SOLOW_K")
    assert got["rewards"].tobytes() == rewards.tobytes() and got["k"].tobytes() == ks.tobytes()
    if E > 1:
        assert len(np.unique(got["actions"][5])) > E // 2                # the envs really differ
    want = _twin_stats(rewards, np.full(E, n, np.int32), np.zeros(E, np.uint8), n)
    for key in PAIR_KEYS:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
    eng.close()


# ------------------------------------------------------------------------------------------ 3. stages and refusals
def test_stage_follows_the_steps_left():
    """stage = max(0, H - remaining): with TimeLimit 12 and H = 5 steps 0..7 use stage 0, steps 8..11 stages 1..4; elapsed 0 and 5
    inside one wave."""
    from goldsrl._ffi_solowarmadp import solow_arma_dp_play, solow_arma_dp_set_policy, table_shape
    E, cap, H = 70, 12, 5
    eng = _snapshot_engine(E, 2, 2, cap=cap, seed=5)
    grid = _small_grid(2, 2)
    level = (0.1 * (1 + np.arange(H, dtype=np.float64))).astype(np.float32)
    solow_arma_dp_set_policy(eng, grid, np.zeros(table_shape(grid, H), np.float32) + level[:, None, None, None, None])
    rng = np.random.RandomState(1)
    for _ in range(5):
        eng.step(rng.uniform(0.05, 0.95, size=(E, 1)).astype(np.float32))
    eng.reset(np.arange(0, E, 3))
    elapsed = eng.get_state("ELAPSED")
    assert set(elapsed) == {0, 5}
    got = solow_arma_dp_play(eng, 20, trace_steps=20)
    assert np.array_equal(got["length"], cap - elapsed) and (got["finished"] == 1).all()
    for env in (0, 1, 64, 66, 69):
        left = cap - elapsed[env]
        stage = np.maximum(0, H - (left - np.arange(left)))
        assert np.array_equal(got["actions"][:left, env], level[stage]), env
        assert (got["actions"][left:, env] == 0).all()
    eng.close()


def test_refusals():
    from goldsrl import _ffi, _ffi_solowarmadp as F
    lib = _ffi.load_library(extra_signatures=F.SOLOW_ARMA_DP_SIGNATURES)
    grid = _small_grid(2, 2)
    g = F._grid_struct(grid)
    pol = np.zeros(F.table_shape(grid, 2), np.float32)
    eng = _snapshot_engine(4, 2, 2)
    assert lib.grl_solow_arma_dp_play(eng.h, 4, 0) == _ffi.E_STATE and b"grl_solow_arma_dp_solve" in lib.grl_last_error(eng.h)   # no table yet
    assert lib.grl_solow_arma_dp_read(eng.h, b"policy", _ffi._ptr(pol), pol.nbytes) == _ffi.E_STATE
    for field, bad in (("nk", 1), ("nk", 4097), ("ns", 1), ("nq", 16), ("k_lo", 0.0), ("s_hi", 1.5), ("nx", (4, 1, 2, 0)), ("x_max", (0.3, 0.0, 0.1, 0.0))):
        b = F._grid_struct(grid)
        setattr(b, field, type(getattr(b, field))(*bad) if isinstance(bad, tuple) else bad)
        assert lib.grl_solow_arma_dp_solve(eng.h, C.byref(b), 2) == _ffi.E_INVALID, field
        assert lib.grl_solow_arma_dp_set_policy(eng.h, C.byref(b), 2, _ffi._ptr(pol)) == _ffi.E_INVALID, field
    assert lib.grl_solow_arma_dp_solve(eng.h, C.byref(g), 0) == _ffi.E_INVALID
    big = F._grid_struct(_small_grid(2, 2, nk=4096, nx=(64, 64, 64)))
    assert lib.grl_solow_arma_dp_solve(eng.h, C.byref(big), 2) == _ffi.E_SIZE and b"exceed" in lib.grl_last_error(eng.h)      # over the 1 GiB cap
    F.solow_arma_dp_set_policy(eng, grid, pol)
    value = np.zeros(pol.shape[1:], np.float64)
    assert lib.grl_solow_arma_dp_read(eng.h, b"value", _ffi._ptr(value), value.nbytes) == _ffi.E_STATE                      # set, not solved
    assert lib.grl_solow_arma_dp_read(eng.h, b"policy", _ffi._ptr(pol), pol.nbytes - 4) == _ffi.E_SIZE
    eng.close()
    wide = _ffi.Engine(_ffi.ENV_SOLOW, 4, solow_p=5, solow_q=1)
    model = F.SolowArmaCoef()
    for rc in (lib.grl_solow_arma_model(wide.h, C.byref(model)), lib.grl_solow_arma_dp_solve(wide.h, C.byref(g), 2)):
        assert rc == _ffi.E_INVALID and b"m = max(p, q + 1) = 5" in lib.grl_last_error(wide.h)
    wide.close()
    trade = _ffi.Engine(_ffi.ENV_TRADE, 4, n_assets=2)
    assert lib.grl_solow_arma_dp_solve(trade.h, C.byref(g), 2) == _ffi.E_INVALID
    assert lib.grl_solow_arma_dp_play(trade.h, 4, 0) == _ffi.E_INVALID
    with pytest.raises(ValueError):
        F.solow_arma_dp_solve(trade, grid, 2)
    trade.close()


# ------------------------------------------------------------------------------------------ 4. the baseline class
def test_baseline_class_takes_the_solver_of_the_order():
    from goldsrl import _ffi_solowarmadp, _ffi_solowdp
    from goldsrl.agents.a3c.policy_monitor import make_eval_engine
    from goldsrl.baselines import OptimalSavingsBaseline
    eng = make_eval_engine("Solow-2-2-finite-eval-v0", 3, max_episode_steps=64)
    b = OptimalSavingsBaseline(engine=eng, grid=_ffi_solowarmadp.engine_grid(eng, nk=12, nx=5, ns=16, k_lo=20.0, k_hi=200.0), horizon=8, max_episode_steps=64)
    ceiling = b.total()
    assert b.stats["total"].shape == (3,) and (b.stats["length"] == 64).all() and (b.stats["finished"] == 1).all()
    assert np.isfinite(ceiling) and ceiling == b.stats["total"].mean()
    assert OptimalSavingsBaseline(engine=eng).horizon == _ffi_solowarmadp.DEFAULT_HORIZON
    eng.close()
    # (1,1) stays on the (k, z, e) solver: the class's statistics are that path's bytes
    eng, twin = (make_eval_engine("Solow-1-1-finite-eval-v0", 3, max_episode_steps=64) for _ in range(2))
    grid = _ffi_solowdp.solow_dp_grid(nk=12, nz=7, nq=3, ns=16, k_lo=20.0, k_hi=200.0, z_max=0.8)
    got = OptimalSavingsBaseline(engine=eng, grid=grid, horizon=8, max_episode_steps=64).run(trace_steps=4)
    _ffi_solowdp.solow_dp_solve(twin, grid, 8, read=False)
    twin.reset()
    want = _ffi_solowdp.solow_dp_play(twin, 64, trace_steps=4)
    assert set(got) == set(want)
    for key in want:
        assert got[key].tobytes() == want[key].tobytes(), key
    eng.close(); twin.close()
