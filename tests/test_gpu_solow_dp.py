"""GPU: the optimal-savings yardstick of the Solow env (grl_solow_dp_* of include/goldsrl_solowdp.h; csrc/solow_dp.hip), the
baseline class, the monitors' optimal() and the script.

The solve is held to the float64 numpy restatement of the recurrence (tests/_solow_dp_oracle.py); the play to the per-step path,
as the constant-savings sweep is (tests/test_gpu_solow_sweep.py): grl_step with the traced actions runs the same float32
operations in the same order, so rewards, capital and their sequential sums must be the per-step path's bits."""
import ctypes as C

import numpy as np
import pytest

import _solow_dp_cases as DC
import _solow_dp_oracle as DO
from test_gpu_solow_sweep import OUTPUTS, PAIR_KEYS, RATES7, STATE_FIELDS, _snapshot_engine, _twin_stats, _Writer

pytestmark = pytest.mark.gpu

# Largest |value - oracle| / max(1, |oracle|) of stage 0 measured over the six cases of test_solve_against_the_oracle: see that
# test's docstring.  The bound is ten times the measurement.
VALUE_MEASURED = 1.56e-15
VALUE_TOL = 10 * VALUE_MEASURED


def _small_grid(**kw):
    from goldsrl._ffi_solowdp import solow_dp_grid
    g = dict(nk=7, nz=5, nq=3, ns=8, k_lo=30.0, k_hi=120.0, z_max=0.4, sigma=DC.SIGMA)
    g.update(kw)
    return solow_dp_grid(**g)


def _tables(eng, grid, horizon, seed):
    from goldsrl._ffi_solowdp import table_shape
    return np.random.RandomState(seed).uniform(size=table_shape(eng, grid, horizon)).astype(np.float32)


# ------------------------------------------------------------------------------------------ 1. the solve
@pytest.mark.parametrize("q", [1, 0])
@pytest.mark.parametrize("nk,nz,nq,ns,horizon", [(5, 3, 1, 4, 1), (16, 7, 3, 16, 6), (33, 5, 5, 65, 3)])
def test_solve_against_the_oracle(nk, nz, nq, ns, horizon, q):
    """Measured: the largest |value - oracle| / max(1, |oracle|) of stage 0 over the six cases is 1.554e-15, at 16 x 7 x 3 with
    q = 0 (2.2e-16 at one stage, 1.3e-15 to 1.6e-15 at three and six: exp, log and pow of the device against numpy's); the bound
    is ten times that.  The oracle's smallest gap between the best and the
    second-best Q on these grids is 3.3e-6 (16 x 7 x 3, q = 1), so every stage's policy must be the oracle's exactly."""
    from goldsrl import _ffi
    from goldsrl._ffi_solowdp import solow_dp_grid, solow_dp_solve
    grid = solow_dp_grid(nk=nk, nz=nz, nq=nq, ns=ns, sigma=DC.SIGMA)
    ne = nq if q else 1
    policy, value, gap = DO.solve(grid, horizon, DC.RHO, DC.THETA if q else 0.0, DC.DELTA, ne)
    assert gap > 1e-8, gap
    eng = _ffi.Engine(_ffi.ENV_SOLOW, 3, solow_p=1, solow_q=q)
    got = solow_dp_solve(eng, grid, horizon)
    assert got["policy"].shape == (horizon, nk, nz, ne) and got["value"].shape == (nk, nz, ne)
    dev = float((np.abs(got["value"] - value) / np.maximum(1.0, np.abs(value))).max())
    print("solow_dp value deviation grid %s q %d: %.3e (oracle gap %.3e)" % ((nk, nz, nq, ns, horizon), q, dev, gap))
    assert got["policy"].tobytes() == policy.tobytes()
    assert dev <= VALUE_TOL, dev
    eng.close()


# ------------------------------------------------------------------------------------------ 2. the play is the per-step path
@pytest.mark.parametrize("E,q", [(1, 1), (63, 1), (64, 1), (65, 1), (130, 1), (65, 0)])
def test_play_is_the_per_step_path_bit_for_bit(E, q):
    from goldsrl._ffi_solowdp import solow_dp_play, solow_dp_policy_actions, solow_dp_set_policy
    n = 40
    eng = _snapshot_engine(E, 1, q, seed=E + q)
    grid = _small_grid()
    tables = _tables(eng, grid, 3, E)
    solow_dp_set_policy(eng, grid, tables)
    eng.reset()
    got = solow_dp_play(eng, n, trace_steps=n)
    assert got["actions"].shape == (n, E) and got["actions"].dtype == np.float32
    eng.reset()
    rewards, ks = np.zeros((n, E), np.float32), np.zeros((n, E), np.float32)
    for t in range(n):
        k, z, e = eng.get_state("SOLOW_K"), eng.get_state("SOLOW_Z")[:, -1], eng.get_state("SOLOW_E")[:, -1]
        want = solow_dp_policy_actions(grid, tables[0], k, z, e)        # no TimeLimit: stage 0 throughout
        ulps = np.abs(got["actions"][t].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (t, ulps.max())
        eng.step(got["actions"][t][:, None])
        rewards[t], ks[t] = eng.read("reward"), eng.get_state("SOLOW_K")
    assert got["rewards"].tobytes() == rewards.tobytes() and got["k"].tobytes() == ks.tobytes()
    if E > 1:
        assert len(np.unique(got["actions"][5])) > E // 2                # the envs really differ
    want = _twin_stats(rewards, np.full(E, n, np.int32), np.zeros(E, np.uint8), n)
    for key in PAIR_KEYS:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key
    eng.reset()
    short = solow_dp_play(eng, 7, trace_steps=2)                         # fewer steps, a shorter trace, the same buffers
    want = _twin_stats(rewards, np.full(E, n, np.int32), np.zeros(E, np.uint8), 7)
    for key in PAIR_KEYS:
        assert short[key].tobytes() == want[key].tobytes(), key
    assert short["rewards"].tobytes() == rewards[:2].tobytes()
    eng.close()


# ------------------------------------------------------------------------------------------ 3. stages and clamps
def _stage_tables(eng, grid, horizon):
    from goldsrl._ffi_solowdp import table_shape
    t = np.zeros(table_shape(eng, grid, horizon), np.float32)
    t += (0.1 * (1 + np.arange(horizon, dtype=np.float64))).astype(np.float32)[:, None, None, None]
    return t


def test_stage_follows_the_steps_left():
    """stage = max(0, H - remaining): with TimeLimit 12 and H = 5 the seven steps beyond the horizon and the horizon's first step
    use stage 0 (steps 0..7), steps 8..11 stages 1..4."""
    from goldsrl._ffi_solowdp import solow_dp_play, solow_dp_set_policy
    E, cap, H = 70, 12, 5
    eng = _snapshot_engine(E, 1, 1, cap=cap, seed=5)
    grid = _small_grid()
    tables = _stage_tables(eng, grid, H)
    solow_dp_set_policy(eng, grid, tables)
    got = solow_dp_play(eng, 20, trace_steps=20)
    stage = np.maximum(0, H - (cap - np.arange(cap)))
    assert list(stage) == [0] * 8 + [1, 2, 3, 4]
    assert np.array_equal(got["actions"][:cap], np.repeat(tables[stage, 0, 0, 0][:, None], E, axis=1))
    assert (got["actions"][cap:] == 0).all() and (got["length"] == cap).all() and (got["finished"] == 1).all()
    # mid-episode, elapsed 0 and 5 inside one wave
    rng = np.random.RandomState(1)
    for _ in range(5):
        eng.step(rng.uniform(0.05, 0.95, size=(E, 1)).astype(np.float32))
    eng.reset(np.arange(0, E, 3))
    elapsed = eng.get_state("ELAPSED")
    assert set(elapsed) == {0, 5}
    got = solow_dp_play(eng, 20, trace_steps=20)
    assert np.array_equal(got["length"], cap - elapsed) and (got["finished"] == 1).all()
    for env in (0, 1, 64, 66, 69):
        left = cap - elapsed[env]
        stage = np.maximum(0, H - (left - np.arange(left)))
        assert np.array_equal(got["actions"][:left, env], tables[stage, 0, 0, 0]), env
        assert (got["actions"][left:, env] == 0).all()
    cut = solow_dp_play(eng, 9, trace_steps=0)
    assert np.array_equal(cut["length"], np.minimum(9, cap - elapsed)) and np.array_equal(cut["finished"], (elapsed == 5).astype(np.uint8))
    assert "actions" not in cut
    eng.close()


def test_no_time_limit_uses_stage_zero():
    from goldsrl._ffi_solowdp import solow_dp_play, solow_dp_set_policy
    eng = _snapshot_engine(5, 1, 1, cap=0, seed=2)
    grid = _small_grid()
    tables = _stage_tables(eng, grid, 4)
    solow_dp_set_policy(eng, grid, tables)
    got = solow_dp_play(eng, 30, trace_steps=30)
    assert (got["actions"] == tables[0, 0, 0, 0]).all() and (got["length"] == 30).all() and not got["finished"].any()
    eng.close()


def test_states_outside_the_grid_take_the_edge():
    from goldsrl._ffi_solowdp import solow_dp_play, solow_dp_set_policy
    E = 6
    eng = _snapshot_engine(E, 1, 1, seed=3)
    grid = _small_grid()
    tables = _tables(eng, grid, 1, 11)
    solow_dp_set_policy(eng, grid, tables)
    lo, hi = np.float32(grid["e_nodes"][0]), np.float32(grid["e_nodes"][2])
    # env:              0: low corner  1: high corner  2: low e   3: high e    4: k low only  5: z high only
    eng.set_state("SOLOW_K", np.array([1.0, 5000.0, 30.0, 30.0, 2.0, 30.0], np.float32))
    eng.set_state("SOLOW_Z", np.array([-3.0, 3.0, -0.4, -0.4, 0.4, 0.9], np.float32)[:, None])
    eng.set_state("SOLOW_E", np.array([0.0, 0.0, -1.0, 1.0, 0.0, 0.0], np.float32)[:, None])
    got = solow_dp_play(eng, 1, trace_steps=1)["actions"][0]
    tab = tables[0]
    assert lo < 0 < hi
    want = np.array([tab[0, 0, 1], tab[-1, -1, 1], tab[0, 0, 0], tab[0, 0, 2], tab[0, -1, 1], tab[0, -1, 1]], np.float32)
    assert got.tobytes() == want.tobytes(), (got, want)                  # the weights are 0 or 1 (or 1e-16 off): the edge's value itself
    eng.close()


# ------------------------------------------------------------------------------------------ 4. read only
def test_solve_and_play_leave_the_handle_untouched():
    from goldsrl import _ffi, _ffi_sweep
    from goldsrl._ffi_solowdp import solow_dp_play, solow_dp_solve

    def make():
        eng = _ffi.Engine(_ffi.ENV_SOLOW, 65, seed=7, solow_p=1, solow_q=1, solow_tape_len=64, max_episode_steps=24)
        eng.reset()
        eng.episodes_enable()
        rng = np.random.RandomState(2)
        for _ in range(3):
            eng.step(rng.uniform(0.05, 0.95, size=(65, 1)).astype(np.float32))
        return eng

    def everything(eng):
        d = {f: eng.get_state(f) for f in STATE_FIELDS}
        d.update({o: eng.read(o) for o in OUTPUTS})
        d["ep_total"], d["ep_len"] = eng.episodes_running()
        return d

    def same(a, b):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k

    eng, twin = make(), make()
    before = everything(eng)
    sweep = _ffi_sweep.solow_sweep(eng, RATES7[:3], 30)
    solved = solow_dp_solve(eng, _small_grid(), 4)
    same(before, everything(eng))
    first = solow_dp_play(eng, 30, trace_steps=5)
    same(before, everything(eng))
    assert (first["length"] == 21).all() and (first["finished"] == 1).all()
    bigger = solow_dp_solve(eng, _small_grid(nk=9, ns=70), 6)            # every table grows
    second = solow_dp_play(eng, 30, trace_steps=30)                      # the trace grows
    same(before, everything(eng))
    assert bigger["policy"].shape == (6, 9, 5, 3) and second["rewards"].shape == (30, 65) and (second["rewards"][21:] == 0).all()
    again = solow_dp_solve(eng, _small_grid(), 4)                        # the smaller one in the grown buffers
    assert again["policy"].tobytes() == solved["policy"].tobytes() and again["value"].tobytes() == solved["value"].tobytes()
    replay = solow_dp_play(eng, 30, trace_steps=5)
    for k in first:
        assert replay[k].tobytes() == first[k].tobytes(), k
    after = _ffi_sweep.solow_sweep(eng, RATES7[:3], 30)
    for k in PAIR_KEYS:
        assert after[k].tobytes() == sweep[k].tobytes(), k
    act = np.full((65, 1), 0.4, np.float32)
    eng.step(act); twin.step(act)
    same(everything(twin), everything(eng))
    eng.close(); twin.close()


# ------------------------------------------------------------------------------------------ 5. refusals
def test_refusals():
    from goldsrl import _ffi, _ffi_solowdp
    lib = _ffi.load_library(extra_signatures=_ffi_solowdp.SOLOW_DP_SIGNATURES)
    grid = _small_grid()
    g = _ffi_solowdp._grid_struct(grid)
    eng = _snapshot_engine(4)
    buf = np.zeros(4, np.float64)
    pol = np.zeros((2, 7, 5, 3), np.float32)
    assert lib.grl_solow_dp_play(eng.h, 4, 0) == _ffi.E_STATE and b"grl_solow_dp_solve" in lib.grl_last_error(eng.h)   # no table yet
    assert lib.grl_solow_dp_read(eng.h, b"policy", _ffi._ptr(pol), pol.nbytes) == _ffi.E_STATE
    assert lib.grl_solow_dp_play_read(eng.h, b"total", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE
    for field, bad in (("nk", 1), ("nz", 1), ("ns", 1), ("nq", 0), ("nq", 16), ("k_lo", 0.0), ("k_hi", 30.0), ("z_max", 0.0), ("s_hi", 1.5)):
        b = _ffi_solowdp._grid_struct(grid)
        setattr(b, field, bad)
        assert lib.grl_solow_dp_solve(eng.h, C.byref(b), 2) == _ffi.E_INVALID, field
        assert lib.grl_solow_dp_set_policy(eng.h, C.byref(b), 2, _ffi._ptr(pol)) == _ffi.E_INVALID, field
    for horizon in (0, -1):
        assert lib.grl_solow_dp_solve(eng.h, C.byref(g), horizon) == _ffi.E_INVALID
    assert lib.grl_solow_dp_solve(eng.h, None, 2) == _ffi.E_INVALID
    assert lib.grl_solow_dp_set_policy(eng.h, C.byref(g), 2, None) == _ffi.E_INVALID
    big = _ffi_solowdp._grid_struct(_small_grid(nk=1024, nz=1024, nq=1))
    assert lib.grl_solow_dp_solve(eng.h, C.byref(big), 257) == _ffi.E_SIZE and b"exceed" in lib.grl_last_error(eng.h)   # over the 1 GiB cap
    eng.step_async(np.full((4, 1), 0.3, np.float32))
    assert lib.grl_solow_dp_solve(eng.h, C.byref(g), 2) == _ffi.E_INVALID and b"in flight" in lib.grl_last_error(eng.h)
    eng.wait()
    _ffi_solowdp.solow_dp_set_policy(eng, grid, pol)
    eng.step_async(np.full((4, 1), 0.3, np.float32))
    assert lib.grl_solow_dp_play(eng.h, 4, 0) == _ffi.E_INVALID and b"in flight" in lib.grl_last_error(eng.h)
    eng.wait()
    assert lib.grl_solow_dp_read(eng.h, b"value", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE      # set, not solved
    assert lib.grl_solow_dp_read(eng.h, b"policy", _ffi._ptr(pol), pol.nbytes - 4) == _ffi.E_SIZE
    assert lib.grl_solow_dp_read(eng.h, b"nothing", _ffi._ptr(pol), pol.nbytes) == _ffi.E_INVALID
    for max_steps, trace_steps in ((0, 0), (4, -1), (4, 5)):
        assert lib.grl_solow_dp_play(eng.h, max_steps, trace_steps) == _ffi.E_INVALID
    _ffi_solowdp.solow_dp_play(eng, 4)
    assert lib.grl_solow_dp_play_read(eng.h, b"total", _ffi._ptr(buf), buf.nbytes - 8) == _ffi.E_SIZE
    assert lib.grl_solow_dp_play_read(eng.h, b"actions", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE      # no trace was kept
    assert lib.grl_solow_dp_play_read(eng.h, b"nothing", _ffi._ptr(buf), buf.nbytes) == _ffi.E_INVALID
    _ffi_solowdp.solow_dp_solve(eng, grid, 2)
    value = np.zeros((7, 5, 3), np.float64)
    assert lib.grl_solow_dp_read(eng.h, b"value", _ffi._ptr(value), value.nbytes + 8) == _ffi.E_SIZE
    eng.close()
    for p, q in ((2, 1), (1, 2)):
        other = _ffi.Engine(_ffi.ENV_SOLOW, 4, solow_p=p, solow_q=q)
        assert lib.grl_solow_dp_solve(other.h, C.byref(g), 2) == _ffi.E_INVALID and b"one dimension per lag" in lib.grl_last_error(other.h)
        assert lib.grl_solow_dp_set_policy(other.h, C.byref(g), 2, _ffi._ptr(pol)) == _ffi.E_INVALID
        other.close()
    trade = _ffi.Engine(_ffi.ENV_TRADE, 4, n_assets=2)
    assert lib.grl_solow_dp_solve(trade.h, C.byref(g), 2) == _ffi.E_INVALID
    assert lib.grl_solow_dp_play(trade.h, 4, 0) == _ffi.E_INVALID
    with pytest.raises(ValueError):
        _ffi_solowdp.solow_dp_solve(trade, grid, 2)
    trade.close()


def test_tape_exhausted_is_the_step_paths_error():
    from goldsrl import _ffi
    from goldsrl._ffi_solowdp import solow_dp_play, solow_dp_set_policy
    eng = _snapshot_engine(66, tape=8, cap=0)
    grid = _small_grid()
    solow_dp_set_policy(eng, grid, _tables(eng, grid, 1, 0))
    with pytest.raises(_ffi.GrlError) as ei:
        solow_dp_play(eng, 10)
    assert ei.value.code == _ffi.E_STATE and "66 env(s) popped from an empty shock tape" in str(ei.value)
    ok = solow_dp_play(eng, 8)                                           # the whole tape and no more
    assert (ok["length"] == 8).all() and not ok["finished"].any()
    eng.close()


# ------------------------------------------------------------------------------------------ 6. end to end
def test_ceiling_stands_above_the_floor_on_the_seeded_episode():
    """The seeded eval episode of the CPU test on the float32 env: the induction on 32 x 9 x 3, 32 actions, 128 stages against
    the best of the reference's 20 constant rates from grl_solow_sweep on the same engine."""
    from goldsrl import _ffi, _ffi_sweep
    from goldsrl._ffi_solowdp import solow_dp_grid
    from goldsrl.baselines import REFERENCE_RATES, OptimalSavingsBaseline
    z0, es = DC.seeded_shocks(2048)
    eng = _ffi.Engine(_ffi.ENV_SOLOW, 1, solow_p=1, solow_q=1, solow_tape_len=2048, max_episode_steps=DC.STEPS, flags=_ffi.F_RESET_FROM_SNAPSHOT)
    eng.set_state("SOLOW_Z0", np.array([[z0]], np.float32))
    eng.set_state("SOLOW_TAPE", es[None].astype(np.float32))
    eng.reset()
    floor = float(_ffi_sweep.solow_sweep(eng, REFERENCE_RATES, DC.STEPS)["total"].mean(axis=1).max())
    b = OptimalSavingsBaseline(engine=eng, grid=solow_dp_grid(sigma=DC.SIGMA, **DC.FLOOR_GRID), horizon=DC.FLOOR_HORIZON, max_episode_steps=DC.STEPS)
    st = b.run()
    ceiling = b.total()
    print("solow_dp seeded episode: floor %.4f ceiling %.4f" % (floor, ceiling))
    assert st["length"][0] == DC.STEPS and st["finished"][0] == 1
    assert ceiling >= floor + DC.MARGIN, (floor, ceiling)
    b.close()
    assert eng.h is not None                                             # a given engine stays the caller's
    eng.close()


def test_monitor_optimal_and_the_scalars():
    from goldsrl import _ffi_gauss
    from goldsrl.agents.a3c.policy_monitor import PolicyMonitor
    w = _Writer()
    mon = PolicyMonitor("Solow-1-1-finite-eval-v0", summary_writer=w, n_envs=3, max_episode_steps=32)
    grid = _small_grid(nk=12, nz=7, ns=16, k_lo=20.0, k_hi=200.0, z_max=0.8)
    ceiling = mon.optimal(grid=grid, horizon=8)
    assert ceiling == mon.optimal_total_reward == mon.optimal_stats["total"].mean() and np.isfinite(ceiling)
    assert mon.optimal_stats["total"].shape == (3,) and (mon.optimal_stats["length"] == 32).all()
    assert (mon.net.eng.get_state("ELAPSED") == 0).all() and (mon.net.eng.get_state("SOLOW_TAPE_POS") == 2047).all()
    mon.eval_once(_ffi_gauss.default_init_gauss(3, **_ffi_gauss.SOLOW_SIZES))
    mean = mon.log["mean_total_reward"][-1]
    mon.write_baseline_scalars(17)
    assert w.rows == [("eval/optimal_total_reward", ceiling, 17)]         # no floor yet: no share
    rate, floor = mon.baseline()
    del w.rows[:]
    mon.write_baseline_scalars(18)
    assert w.rows == [("eval/baseline_total_reward", floor, 18), ("eval/mean_total_reward_minus_baseline", mean - floor, 18),
                      ("eval/optimal_total_reward", ceiling, 18), ("eval/mean_total_reward_share_of_gap", (mean - floor) / (ceiling - floor), 18)]
    mon.close()
    trade = PolicyMonitor("TradeAR1-v0", n_envs=2, max_episode_steps=8)
    with pytest.raises(ValueError):
        trade.optimal()
    trade.close()


def test_optimal_solow_script(capsys):
    from goldsrl.scripts import optimal_solow
    rec = optimal_solow.main(["--envs", "2", "--grid", "16", "7", "3", "16", "--horizon", "16"])
    assert rec["n_envs"] == 2 and np.isfinite(rec["floor"]) and np.isfinite(rec["ceiling"]) and rec["gap"] == rec["ceiling"] - rec["floor"]
    assert "floor" in capsys.readouterr().out


def test_train_solow_grid_optimal_flag(tmp_path):
    import glob
    import os
    from goldsrl import utils_tfevents
    from goldsrl.scripts import train_solow_grid
    out = tmp_path / "run"
    train_solow_grid.main(["--eval-envs", "4", "--envs", "64", "--updates", "2", "--eval-every", "1", "--model_dir", str(out), "--baseline", "--optimal"])
    (events,) = glob.glob(os.path.join(str(out), "events.out.tfevents.*"))
    scalars = {}
    for tag, value, step, _ in utils_tfevents.read_scalars(events):
        scalars.setdefault(tag, []).append((step, value))
    for tag in ("eval/optimal_total_reward", "eval/mean_total_reward_share_of_gap", "eval/baseline_total_reward"):
        assert [s for s, _ in scalars[tag]] == [s for s, _ in scalars["eval/mean_total_reward"]] and len(scalars[tag]) == 2, tag
    floor, ceiling = scalars["eval/baseline_total_reward"][0][1], scalars["eval/optimal_total_reward"][0][1]
    assert ceiling > floor and scalars["eval/optimal_total_reward"][1][1] == ceiling      # the default grid stands above the agent's 51 rates
    for (_, m), (_, share) in zip(scalars["eval/mean_total_reward"], scalars["eval/mean_total_reward_share_of_gap"]):
        assert abs(share - (m - floor) / (ceiling - floor)) <= 1e-5 * max(1.0, abs(share))   # scalars are stored as float32
