"""GPU: the perfect-foresight ceiling of the Solow env (grl_solow_foresight of include/goldsrl_solowforesight.h;
csrc/solow_foresight.hip) and the class that carries it.

The induction is held to the float64 numpy restatement of the recurrence (tests/_solow_foresight_oracle.py) run on the device's own
path; the play to the per-step path, as tests/test_gpu_solow_dp.py holds the inductions' plays: grl_step with the traced actions
runs the same float32 operations in the same order, so rewards and capital must be the per-step path's bits."""
import ctypes as C

import numpy as np
import pytest

import _solow_foresight_oracle as FO
from test_gpu_solow_sweep import OUTPUTS, PAIR_KEYS, STATE_FIELDS, _snapshot_engine, _twin_stats

pytestmark = pytest.mark.gpu

# Capital from below the grid (env 0: clamped > 0) to the reset value: at the low nodes saving pays, so the decisions are interior
# (16 to 170 distinct rates in the oracle's tables), not the all-consume plan a 40-step episode has at k_ss.
K0 = np.array([0.02, 0.3, 2.0, 20.0, 65.0], np.float32)
# p, q, E, steps, nk, ns: nk 23 is no multiple of the four waves, 64 is; ns 24 is below a wave, 70 a ragged second pass, 256 the most.
# 256 rates lie 0.004 apart, so near a flat top two of them can be closer in Q than the oracle can tell apart: that case has one
# env (920 arg-maxes; the oracle's smallest gap on its injected path, restated on the CPU, is 2.0e-7), the five-env cases fewer rates.
CASES = [(1, 0, 1, 24, 23, 24), (1, 1, 5, 32, 64, 70), (3, 2, 1, 40, 23, 256), (3, 2, 5, 24, 64, 24)]
# The played total of the float64 oracle moves by 0.1060 (tape seed 192) and 0.1026 (seed 7) from 48 x 48 to 96 x 96 nodes on the
# default k range of (1,1), 1 024 steps, tapes drawn in numpy the way _reset draws them: the largest is the bound below.
PLAYED_MOVEMENT_48_TO_96 = 0.1060


def _grid(nk, ns):
    return {"nk": nk, "ns": ns, "k_lo": 0.05, "k_hi": 150.0, "s_lo": 0.001, "s_hi": 0.999}


def _engine(p, q, E, steps):
    """With E > 1 a TimeLimit of steps + 3 and envs that enter with elapsed 0 and 5: L_e is steps (max_steps is shorter than what is
    left) and steps - 2 (the TimeLimit ends the episode) inside one launch."""
    eng = _snapshot_engine(E, p, q, cap=steps + 3 if E > 1 else 0, seed=E + q)
    if E > 1:
        rng = np.random.RandomState(1)
        for _ in range(5):
            eng.step(rng.uniform(0.05, 0.95, size=(E, 1)).astype(np.float32))
        eng.reset(np.arange(0, E, 2))
    eng.set_state("SOLOW_K", K0[:E])
    return eng


def _everything(eng):
    d = {f: eng.get_state(f) for f in STATE_FIELDS}
    d.update({o: eng.read(o) for o in OUTPUTS})
    return d


@pytest.mark.parametrize("p,q,E,steps,nk,ns", CASES)
def test_foresight_against_the_oracle_and_the_per_step_path(p, q, E, steps, nk, ns, monkeypatch):
    from goldsrl import _ffi
    from goldsrl._ffi_solowforesight import SOLOW_FORESIGHT_SIGNATURES, solow_foresight, solow_foresight_actions
    grid, delta = _grid(nk, ns), 0.02
    eng = _engine(p, q, E, steps)
    assert eng.cfg.solow_delta == delta
    elapsed, before = eng.get_state("ELAPSED"), _everything(eng)
    got = solow_foresight(eng, steps, trace_steps=steps, grid=grid, decisions=True)
    after = _everything(eng)
    for key in before:
        assert before[key].tobytes() == after[key].tobytes(), key          # the handle is read only
    want_len = np.where(elapsed > 0, steps + 3 - elapsed, steps) if E > 1 else np.full(E, steps)
    assert np.array_equal(got["length"], want_len) and np.array_equal(got["finished"], (elapsed > 0).astype(np.uint8))
    if E > 1:
        assert len(set(want_len)) == 2
    assert got["clamped"][0] > 0 and (got["clamped"][1:] == 0).all()
    # the induction: the oracle on the device's own path
    worst = 0.0
    for e in range(E):
        L = int(got["length"][e])
        dec, V, gap = FO.solve(got["ez"][:L, e].astype(np.float64), grid, delta)
        assert gap > 1e-9, gap                                             # the reference alone passes: no decision is left out
        assert got["decisions"][e, :L].tobytes() == dec.tobytes(), e
        assert not got["decisions"][e, L:].any() and not got["ez"][L:, e].any()
        want = FO.value_at(V, K0[e], grid)
        worst = max(worst, abs(got["value"][e] - want) / (L * max(1.0, abs(want))))
        assert abs(got["value"][e] - want) <= L * 2.0 ** -50 * max(1.0, abs(want)), (e, got["value"][e], want)
    print("solow_foresight value residual / L, order %s grid %s: %.3e (bound %.3e)" % ((p, q), (nk, ns, steps), worst, 2.0 ** -50))
    # the play: the look-up at the traced capital, then the per-step path with the traced actions
    rewards, live = np.zeros((steps, E), np.float32), np.arange(steps)[:, None] < got["length"][None]
    k = eng.get_state("SOLOW_K")
    for t in range(steps):
        want = solow_foresight_actions(got["decisions"], grid, t, k)
        ulps = np.abs(got["actions"][t].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps[live[t]].max(initial=0) <= 1, (t, ulps)
        eng.step(got["actions"][t][:, None])
        rewards[t], k = eng.read("reward"), eng.get_state("SOLOW_K")
        same_k = live[t] & ~((t == got["length"] - 1) & (got["finished"] == 1))     # a capped episode's last step auto-resets k
        assert got["k"][t][same_k].tobytes() == k[same_k].tobytes(), t
        k = np.where(same_k, k, np.float32(1.0))
    assert np.where(live, got["rewards"], 0).tobytes() == np.where(live, rewards, 0).tobytes()
    for name in ("actions", "rewards", "k"):
        assert not got[name][~live].any(), name
    twin = _twin_stats(rewards, got["length"], got["finished"], steps)
    for key in PAIR_KEYS:
        assert got[key].dtype == twin[key].dtype and got[key].tobytes() == twin[key].tobytes(), key
    eng.close()
    if E > 1:                                                              # the table capped at one env's: E launches, the same bytes
        eng = _engine(p, q, E, steps)
        monkeypatch.setenv("GRL_SOLOW_FORESIGHT_TABLE_BYTES", str(steps * nk))
        capped = solow_foresight(eng, steps, trace_steps=steps, grid=grid)
        for key in capped:
            if key != "grid":
                assert capped[key].tobytes() == got[key].tobytes(), key
        lib = _ffi.load_library(extra_signatures=SOLOW_FORESIGHT_SIGNATURES)
        table = np.zeros((E, steps, nk), np.uint8)
        assert lib.grl_solow_foresight_read(eng.h, b"decisions", _ffi._ptr(table), table.nbytes) == _ffi.E_STATE
        assert b"several launches" in lib.grl_last_error(eng.h)
        eng.close()


def test_refusals_and_the_end_of_the_tape():
    from goldsrl import _ffi, _ffi_solowforesight as F
    lib = _ffi.load_library(extra_signatures=F.SOLOW_FORESIGHT_SIGNATURES)
    grid = _grid(8, 8)
    g = F._grid_struct(grid)
    eng = _snapshot_engine(4, 5, 5, tape=16)                                   # m = 6: no induction solver takes this order
    buf = np.zeros(4, np.float64)
    assert lib.grl_solow_foresight_read(eng.h, b"total", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE
    for field, bad in (("nk", 1), ("nk", 1025), ("ns", 1), ("ns", 257), ("k_lo", 0.0), ("k_hi", 0.01), ("s_lo", -0.1), ("s_hi", 1.5)):
        b = F._grid_struct(dict(grid, **{field: bad}))
        assert lib.grl_solow_foresight(eng.h, C.byref(b), 4, 0) == _ffi.E_INVALID, field
    for max_steps, trace_steps in ((0, 0), (4, -1), (4, 5)):
        assert lib.grl_solow_foresight(eng.h, C.byref(g), max_steps, trace_steps) == _ffi.E_INVALID
    assert lib.grl_solow_foresight(eng.h, None, 4, 0) == _ffi.E_INVALID
    eng.step_async(np.full((4, 1), 0.3, np.float32))
    assert lib.grl_solow_foresight(eng.h, C.byref(g), 4, 0) == _ffi.E_INVALID and b"in flight" in lib.grl_last_error(eng.h)
    eng.wait()
    ok = F.solow_foresight(eng, 15, grid=grid)                                 # the whole tape left and no more
    assert (ok["length"] == 15).all() and not ok["finished"].any()
    assert lib.grl_solow_foresight_read(eng.h, b"actions", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE      # no trace was kept
    assert lib.grl_solow_foresight_read(eng.h, b"total", _ffi._ptr(buf), buf.nbytes - 8) == _ffi.E_SIZE
    with pytest.raises(_ffi.GrlError) as ei:
        F.solow_foresight(eng, 16, grid=grid)
    assert ei.value.code == _ffi.E_STATE and "4 env(s) popped from an empty shock tape" in str(ei.value)
    eng.close()
    trade = _ffi.Engine(_ffi.ENV_TRADE, 4, n_assets=2)
    assert lib.grl_solow_foresight(trade.h, C.byref(g), 4, 0) == _ffi.E_INVALID
    with pytest.raises(ValueError):
        F.solow_foresight(trade, 4, grid=grid)
    trade.close()


@pytest.mark.parametrize("env", ["Solow-1-1-finite-eval-v0", "Solow-2-2-finite-eval-v0"])
def test_ceiling_on_the_scale_of_the_seeded_eval_episodes(env):
    """Floor, induction and ceiling on the same seeded eval episodes, default grids: the plan that knows the shocks beats the best
    constant rate, stays inside its default k range, and is not below the induction's played total by more than the played total's
    own movement between 48 and 96 nodes."""
    from goldsrl.agents.a3c.policy_monitor import make_eval_engine
    from goldsrl.baselines import ConstantSavingsBaseline, OptimalSavingsBaseline, SolowForesightCeiling
    eng = make_eval_engine(env, 2)
    floor = ConstantSavingsBaseline(engine=eng).run()["total"].max(axis=0)
    top = SolowForesightCeiling(engine=eng)
    stats = top.run()
    optimal = OptimalSavingsBaseline(engine=eng).run()["total"]
    print("%s: floor %s induction %s ceiling %s value %s" % (env, floor, optimal, stats["total"], stats["value"]))
    assert (stats["length"] == 1024).all() and (stats["clamped"] == 0).all()
    assert (stats["total"] > floor).all()
    assert (stats["total"] >= optimal - PLAYED_MOVEMENT_48_TO_96).all()
    assert top.ceiling() == stats["total"].mean()
    eng.close()
