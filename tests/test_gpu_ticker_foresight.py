"""GPU: the foresight ceiling of the Ticker env (grl_ticker_foresight / grl_ticker_foresight_read of
include/goldsrl_tickerforesight.h; csrc/ticker_foresight.hip), TickerForesightCeiling, the monitor's ticker_ceiling() and
train_ticker --ceiling.

The yardstick of the one-launch form is the per-step path, as in tests/test_gpu_ticker_sweep.py: grl_step with the recurrence's
actions computed on the host (_ffi_tickerforesight.ticker_foresight_actions) from the read-back TICKER_IDX / TICKER_START runs the
same float64 operations in the same order, so a pair's actions, account and rewards -- and their sequential float64 sums -- must be
the per-step path's bits.  The per-step twin of a case is played once.  The recurrence itself is held to a brute force and to the
reference env on the CPU (tests/test_ticker_foresight_oracle.py)."""
import glob
import os

import numpy as np
import pytest

import _ticker_foresight_oracle as FO

pytestmark = pytest.mark.gpu

HORIZONS = (0, 1, 2, 4, 16, 64)
PAIR_KEYS = ("total", "sum_sq", "min", "max", "length", "trades", "finished", "depleted")
TRACE_KEYS = ("trace_rewards", "trace_assets", "trace_actions")
STATE_FIELDS = ("TICKER_CASH", "TICKER_ASSETS", "TICKER_QUANTITY", "TICKER_IDX", "TICKER_START", "TICKER_START0", "ELAPSED", "EPISODE", "NHIST")
OUTPUTS = ("reward", "reward_f64", "done", "elapsed", "obs", "obs_raw", "done_count")


@pytest.fixture(scope="module")
def fix(golden):
    g = golden("ticker_rules")
    return {k: g[k] for k in g.files}


def _engine(E, matrix, starts=None, cap=1023, seed=0):
    from goldsrl import _ffi
    eng = _ffi.Engine(_ffi.ENV_TICKER, E, seed=seed, max_episode_steps=cap, flags=_ffi.F_RESET_FROM_SNAPSHOT if starts is not None else 0)
    eng.ticker_set_table(matrix)
    if starts is not None:
        eng.set_state("TICKER_START0", np.asarray(starts, np.int32))
    eng.reset()
    return eng


def _starts(E, matrix, seed=0):
    s = np.random.RandomState(seed).randint(0, matrix.shape[0] - 1024 + 1, size=E)
    s[0] = matrix.shape[0] - 1024                                          # the last window of the table
    return s


def _random_steps(eng, k, seed):
    rng = np.random.RandomState(seed)
    for _ in range(k):
        eng.step(np.concatenate([rng.randint(0, 3, size=(eng.E, 2)), rng.uniform(0, 1, size=(eng.E, 2))], axis=1).astype(np.float32))


def _play(eng, horizon, max_steps, matrix, cap=0):
    """The per-step path from the engine's current state: the pairs' n steps (the same n for every env of a case) of step(the
    recurrence's actions on the read-back state).  Returns actions (n,E,4) and rewards (n,E) float32, dones (n,E) bool, the assets
    after every step (n,E) float64 (the reset value where the step ended an episode) and the elapsed counters at the start."""
    from goldsrl._ffi_tickerforesight import ticker_foresight_actions, ticker_foresight_last
    E = eng.E
    el0, idx0 = eng.get_state("ELAPSED").copy(), eng.get_state("TICKER_IDX").copy()
    last = ticker_foresight_last(max_steps, cap, el0, idx0)
    n = last - idx0 + 1
    assert (n == n[0]).all() and n[0] >= 1
    steps = int(n[0])
    actions, rewards = np.zeros((steps, E, 4), np.float32), np.zeros((steps, E), np.float32)
    dones, assets = np.zeros((steps, E), bool), np.zeros((steps, E))
    for t in range(steps):
        cash, qty = eng.get_state("TICKER_CASH"), eng.get_state("TICKER_QUANTITY")
        idx, start = eng.get_state("TICKER_IDX"), eng.get_state("TICKER_START")
        assert (idx == idx0 + t).all()
        actions[t] = ticker_foresight_actions(horizon, cash, qty, matrix, start, idx, last)
        eng.step(actions[t])
        rewards[t], dones[t], assets[t] = eng.read("reward"), eng.read("done") > 0, eng.get_state("TICKER_ASSETS")
    return actions, rewards, dones, assets, el0


def _twin_stats(twin, cap=0):
    """What the call keeps, from the per-step path up to each env's first done: sequential float64 sums (np.cumsum adds in order),
    float32 min / max, the trades, and final_assets where the pair did not end (an ended env's assets are already the reset value)."""
    actions, rewards, dones, assets, el0 = twin
    steps, E = rewards.shape
    ended = dones.any(axis=0)
    n = np.where(ended, dones.argmax(axis=0) + 1, steps)
    at_limit = (el0 + n >= cap) if cap > 0 else np.zeros(E, bool)
    r64 = rewards.astype(np.float64)
    c1, c2 = np.cumsum(r64, axis=0), np.cumsum(r64 * r64, axis=0)
    env = np.arange(E)
    live = np.arange(steps)[:, None] < n[None]
    traded = (actions[:, :, :2] != 0).any(axis=2) & live
    return {"total": c1[n - 1, env], "sum_sq": c2[n - 1, env],
            "min": np.where(live, rewards, np.inf).min(axis=0).astype(np.float32),
            "max": np.where(live, rewards, -np.inf).max(axis=0).astype(np.float32),
            "length": n.astype(np.int32), "trades": traded.sum(axis=0).astype(np.int32), "finished": ended.astype(np.uint8),
            "depleted": (ended & ~at_limit).astype(np.uint8), "final_assets": assets[n - 1, env], "open": ~ended}


def _assert_bits(got, want, r, msg):
    for k in PAIR_KEYS:
        assert got[k][r].dtype == want[k].dtype, (k, got[k].dtype, want[k].dtype)
        assert got[k][r].tobytes() == want[k].tobytes(), "%s: %s of horizon column %d differs" % (msg, k, r)
    o = want["open"]
    assert got["final_assets"][r][o].tobytes() == want["final_assets"][o].tobytes(), "%s: final_assets of horizon column %d differs" % (msg, r)


def _assert_trace(got, twin, want, r, env, msg):
    actions, rewards, _, assets, _ = twin
    n = int(want["length"][env])
    assert got["trace_actions"][r, :n].tobytes() == actions[:n, env].tobytes(), "%s: trace_actions of horizon column %d" % (msg, r)
    assert got["trace_rewards"][r, :n].tobytes() == rewards[:n, env].tobytes(), "%s: trace_rewards of horizon column %d" % (msg, r)
    k = n if want["open"][env] else n - 1                                  # the step that ends an episode auto-resets the account
    assert got["trace_assets"][r, :k].tobytes() == assets[:k, env].tobytes(), "%s: trace_assets of horizon column %d" % (msg, r)
    assert got["trace_assets"][r, n - 1] == got["final_assets"][r, env]
    assert not got["trace_rewards"][r, n:].any() and not got["trace_assets"][r, n:].any() and not got["trace_actions"][r, n:].any()


def _check_against_the_step_path(matrix, E, starts, horizons, max_steps, cap=1023, prepare=None):
    """One call with every horizon against one per-step twin per horizon, each from the same prepared state."""
    from goldsrl import _ffi_tickerforesight
    eng = _engine(E, matrix, starts, cap=cap)
    if prepare:
        prepare(eng)
    env = E - 1
    got = _ffi_tickerforesight.ticker_foresight(eng, horizons, max_steps, trace_env=env)
    assert got["total"].shape == (len(horizons), E) and got["trace_actions"].shape == (len(horizons), max_steps, 4)
    twins = []
    for r, H in enumerate(horizons):
        eng.reset()
        if prepare:
            prepare(eng)
        twin = _play(eng, H, max_steps, matrix, cap)
        want = _twin_stats(twin, cap)
        _assert_bits(got, want, r, "E %d horizon %d" % (E, H))
        _assert_trace(got, twin, want, r, env, "E %d horizon %d" % (E, H))
        assert np.isnan(got["bound"][r]).all() == (H != 0) and np.isnan(got["bound"][r]).any() == (H != 0)
        twins.append(twin)
    eng.close()
    return got, twins


# ------------------------------------------------------------------------------------------ 1. bit for bit from a reset
@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
def test_foresight_is_the_per_step_path_bit_for_bit(E, fix):
    m = fix["matrix"]
    got, twins = _check_against_the_step_path(m, E, _starts(E, m, E), HORIZONS, 48)
    assert (got["length"] == 48).all() and not got["finished"].any()
    a0, a1 = twins[0][0], twins[1][0]
    assert (a0[:, :, :2] == 1).any() and (a0[:, :, :2] == 2).any() and not np.array_equal(a0, a1)      # buys, sales; the horizons differ
    assert (got["total"][0] >= got["total"][1:] - 48 * 2e-7).all()         # knowing everything is worth no less (float32 step rewards)
    if E > 1:
        assert len(np.unique(got["total"][0])) > 1                         # the envs really differ


# ------------------------------------------------------------------------------------------ 2. the two code paths
def test_a_horizon_past_the_episode_equals_the_whole_episode(fix):
    """horizon 64 runs the per-step backward loop, horizon 0 the one-pass plan with its decision bytes; over 48 steps both know
    every row.  Every output but `bound`, which is the whole-episode column's alone."""
    from goldsrl import _ffi_tickerforesight
    m, E = fix["matrix"], 130
    eng = _engine(E, m, _starts(E, m, 3))
    _random_steps(eng, 3, 8)
    got = _ffi_tickerforesight.ticker_foresight(eng, (64, 0, 47), 48, trace_env=77)
    for k in PAIR_KEYS + ("final_assets",) + TRACE_KEYS:
        assert got[k][0].tobytes() == got[k][1].tobytes() == got[k][2].tobytes(), k
    assert (got["length"] == 48).all() and (got["trades"] > 0).any() and got["trace_actions"][1].any()
    assert np.isnan(got["bound"][[0, 2]]).all() and np.isfinite(got["bound"][1]).all()
    eng.close()


# ------------------------------------------------------------------------------------------ 3. mid-episode start, the bound
def test_bound_from_a_mid_episode_state(fix):
    """After 7 random-action steps the account holds cash and both assets.  The device's bound is the host form's up to the two
    logarithms (each library's within 1 ulp of log(10) = 2.3: 4 x 2.2e-16 x 2.3 = 2e-15), the plain-loop oracle's likewise, and the
    played episode earns it: log(final + 1e-4) - log(before + 1e-4) within 1e-12."""
    from goldsrl import _ffi_tickerforesight
    from goldsrl._ffi_tickerforesight import ticker_foresight_bound, ticker_foresight_last
    m, E = fix["matrix"], 70
    prepare = lambda eng: _random_steps(eng, 7, 1)                         # noqa: E731
    got, _ = _check_against_the_step_path(m, E, _starts(E, m, 5), (0, 4), 48, prepare=prepare)
    eng = _engine(E, m, _starts(E, m, 5))
    prepare(eng)
    st = {f: eng.get_state(f) for f in STATE_FIELDS}
    cash, qty, before = st["TICKER_CASH"], st["TICKER_QUANTITY"], st["TICKER_ASSETS"]
    assert (st["TICKER_IDX"] == 7).all() and ((cash > 0) & (qty > 0).all(axis=1)).sum() > E // 4
    last = ticker_foresight_last(48, 1023, st["ELAPSED"], st["TICKER_IDX"])
    want = ticker_foresight_bound(cash, qty, before, m, st["TICKER_START"], st["TICKER_IDX"], last)
    assert np.abs(got["bound"][0] - want).max() <= 2e-15
    for e in (0, 1, 33, 69):
        one = {"cash": cash[e:e + 1], "assets": before[e:e + 1], "qty": qty[e:e + 1], "idx": st["TICKER_IDX"][e:e + 1].astype(np.int64),
               "start": st["TICKER_START"][e:e + 1].astype(np.int64)}
        assert abs(FO.play(m, None, 0, 48, state=one)[3] - got["bound"][0, e]) <= 2e-15
    earned = np.log(got["final_assets"][0] + 1e-4) - np.log(before + 1e-4)
    assert np.abs(earned - got["bound"][0]).max() <= 1e-12
    assert (got["bound"][0] > 0).all() and (got["total"][0] > got["total"][1]).any()
    eng.close()


# ------------------------------------------------------------------------------------------ 4. the ends
def test_timelimit_and_window_end(fix):
    m, E = fix["matrix"], 66
    got, _ = _check_against_the_step_path(m, E, _starts(E, m, 2), (0, 2, 64), 64, cap=20)
    assert (got["length"] == 20).all() and (got["finished"] == 1).all() and not got["depleted"].any()
    assert not got["trace_rewards"][:, 20:].any() and not got["trace_actions"][:, 20:].any() and not got["trace_assets"][:, 20:].any()
    at_1014 = lambda eng: eng.set_state("TICKER_IDX", np.full(E, 1014, np.int32))                        # noqa: E731
    got, _ = _check_against_the_step_path(m, E, _starts(E, m, 2), (0, 2, 64), 64, cap=0, prepare=at_1014)
    assert (got["length"] == 9).all() and not got["finished"].any() and not got["depleted"].any()        # rows 1014 .. 1022 are traded at
    assert not got["trace_rewards"][:, 9:].any() and not got["trace_actions"][:, 9:].any()
    from goldsrl import _ffi_tickerforesight
    eng = _engine(3, m, _starts(3, m, 2), cap=0)
    eng.set_state("TICKER_IDX", np.full(3, 1023, np.int32))                # nothing left to play
    none = _ffi_tickerforesight.ticker_foresight(eng, (0, 5), 5, trace_env=0)
    assert (none["length"] == 0).all() and (none["total"] == 0).all() and not none["finished"].any() and (none["bound"][0] == 0).all()
    assert not none["trace_rewards"].any()
    eng.close()


# ------------------------------------------------------------------------------------------ 5. a table that moves
def _moving_table(rows=1400, seed=6, sigma=0.02):
    rng = np.random.RandomState(seed)
    ret = rng.normal(0, sigma, size=rows)
    ret[0] = 0
    m = np.zeros((rows, 4))
    m[:, 0], m[:, 1] = 100.0 * np.exp(np.cumsum(ret)), 100.0 * np.exp(np.cumsum(-ret))
    return m


def test_a_table_that_moves_two_percent_a_row():
    """With 2 % moves against a 1.2 % round trip the trader switches between the asset and its inverse through cash: a sale, then a
    buy at the next step (a buy spends the cash the step began with); and where cash should go into asset 0 while asset 1 should be
    sold, the action is (1, 2).  Both are asserted on the plain-loop oracle before the device is held to the step path."""
    m, E = _moving_table(), 65
    starts = _starts(E, m, 9)
    acts = FO.plan(0, m[starts[1]:starts[1] + 1024], 0, 47)
    assert ((acts[:, 0] == 1) & (acts[:, 1] == 2)).any(), "no (buy 0, sell 1) action"
    sells = (acts[:-1, :2] == 2).any(axis=1) & ~(acts[:-1, :2] == 1).any(axis=1)
    assert (sells & (acts[1:, :2] == 1).any(axis=1)).any(), "no sale followed by a buy"
    got, twins = _check_against_the_step_path(m, E, starts, HORIZONS, 48)
    assert np.array_equal(got["trace_actions"][0], twins[0][0][:, E - 1]) and np.array_equal(twins[0][0][:, 1], acts)
    assert (got["trades"][0] > 10).all() and (got["total"][0] > 0.2).all()


# ------------------------------------------------------------------------------------------ 6. the handle is untouched
def test_call_leaves_the_handle_untouched_and_grows_its_buffers(fix):
    from goldsrl import _ffi_tickerforesight
    m = fix["matrix"]

    def make():
        eng = _engine(65, m, cap=24, seed=7)                               # window starts drawn on the device
        eng.episodes_enable()
        _random_steps(eng, 3, 2)
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
    assert before["reward"].any() and (before["NHIST"] > 0).all()
    second = _ffi_tickerforesight.ticker_foresight(eng, HORIZONS, 40, trace_env=64)
    same(before, everything(eng))
    assert (second["length"] == 21).all() and (second["finished"] == 1).all() and not second["depleted"].any()
    assert second["trace_rewards"].shape == (6, 40) and not second["trace_rewards"][:, 21:].any()
    first = _ffi_tickerforesight.ticker_foresight(eng, HORIZONS[:3], 30)   # a smaller one in the grown buffers
    same(before, everything(eng))
    for k in PAIR_KEYS + ("final_assets", "bound"):
        assert second[k][:3].tobytes() == first[k].tobytes(), k
    third = _ffi_tickerforesight.ticker_foresight(eng, HORIZONS + HORIZONS, 50, trace_env=0)              # every buffer grows
    same(before, everything(eng))
    again = _ffi_tickerforesight.ticker_foresight(eng, HORIZONS, 40, trace_env=64)
    for k in PAIR_KEYS + ("final_assets", "bound") + TRACE_KEYS:
        assert again[k].tobytes() == second[k].tobytes(), k
        assert third[k][6:].tobytes() == third[k][:6].tobytes(), k
    act = np.tile(np.array([1, 2, 0.4, 0.7], np.float32), (65, 1))
    eng.step(act); twin.step(act)                                          # a step after the call gives the bits it gives without it
    same(everything(twin), everything(eng))
    eng.close(); twin.close()


# ------------------------------------------------------------------------------------------ 7. refusals
def test_call_refuses_bad_arguments(fix):
    from goldsrl import _ffi, _ffi_tickerforesight
    lib = _ffi.load_library(extra_signatures=_ffi_tickerforesight.TICKER_FORESIGHT_SIGNATURES)
    m, P = fix["matrix"], _ffi._ptr
    eng = _engine(4, m)
    buf = np.zeros((2, 4), np.float64)
    assert lib.grl_ticker_foresight_read(eng.h, b"total", P(buf), buf.nbytes) == _ffi.E_STATE     # before the first call
    good = np.arange(65, dtype=np.int32)
    for n_h, max_steps, trace_env in ((0, 4, -1), (65, 4, -1), (-1, 4, -1), (2, 0, -1), (2, 4, 4), (2, 4, -2)):
        assert lib.grl_ticker_foresight(eng.h, P(good), n_h, max_steps, trace_env) == _ffi.E_INVALID
    assert lib.grl_ticker_foresight(eng.h, P(good), 0, 4, -1) == _ffi.E_INVALID and b"n_horizons" in lib.grl_last_error(eng.h)
    assert lib.grl_ticker_foresight(eng.h, None, 2, 4, -1) == _ffi.E_INVALID and b"null" in lib.grl_last_error(eng.h)
    for v in (-1, 1024):
        x = np.array([0, 3, v], np.int32)
        assert lib.grl_ticker_foresight(eng.h, P(x), 3, 4, -1) == _ffi.E_INVALID
        assert b"horizon 2 is not" in lib.grl_last_error(eng.h), lib.grl_last_error(eng.h)
        with pytest.raises(ValueError, match="horizon 2"):
            _ffi_tickerforesight.ticker_foresight(eng, x, 4)
    edge = np.array([1023, 0], np.int32)                                   # the edges of the range play
    assert lib.grl_ticker_foresight(eng.h, P(edge), 2, 4, 3) == _ffi.OK
    assert lib.grl_ticker_foresight(eng.h, P(good), 64, 4, -1) == _ffi.OK
    eng.step_async(np.zeros((4, 4), np.float32))
    assert lib.grl_ticker_foresight(eng.h, P(good), 2, 4, -1) == _ffi.E_INVALID and b"in flight" in lib.grl_last_error(eng.h)
    eng.wait()
    bare = _ffi.Engine(_ffi.ENV_TICKER, 4)                                 # no price table yet
    assert lib.grl_ticker_foresight(bare.h, P(good), 2, 4, -1) == _ffi.E_INVALID and b"table" in lib.grl_last_error(bare.h)
    assert lib.grl_ticker_foresight_read(bare.h, b"total", P(buf), buf.nbytes) == _ffi.E_STATE
    _ffi_tickerforesight.ticker_foresight(eng, [0, 4], 4)
    for name in (b"total", b"bound", b"sum_sq", b"final_assets"):
        assert lib.grl_ticker_foresight_read(eng.h, name, P(buf), buf.nbytes) == _ffi.OK
    assert lib.grl_ticker_foresight_read(eng.h, b"total", P(buf), buf.nbytes - 8) == _ffi.E_SIZE
    assert lib.grl_ticker_foresight_read(eng.h, b"trades", P(buf), buf.nbytes) == _ffi.E_SIZE
    assert lib.grl_ticker_foresight_read(eng.h, b"finished", P(buf), buf.nbytes) == _ffi.E_SIZE
    assert lib.grl_ticker_foresight_read(eng.h, b"nothing", P(buf), buf.nbytes) == _ffi.E_INVALID
    assert lib.grl_ticker_foresight_read(eng.h, None, P(buf), buf.nbytes) == _ffi.E_INVALID
    assert lib.grl_ticker_foresight_read(eng.h, b"total", None, buf.nbytes) == _ffi.E_INVALID
    for name in TRACE_KEYS:                                                # the last call traced no env
        assert lib.grl_ticker_foresight_read(eng.h, name.encode(), P(buf), buf.nbytes) == _ffi.E_STATE
    trade = _ffi.Engine(_ffi.ENV_TRADE, 4, n_assets=2)
    assert lib.grl_ticker_foresight(trade.h, P(good), 2, 4, -1) == _ffi.E_INVALID
    assert lib.grl_ticker_foresight_read(trade.h, b"total", P(buf), buf.nbytes) == _ffi.E_INVALID
    with pytest.raises(ValueError):
        _ffi_tickerforesight.ticker_foresight(trade, [0], 4)
    uncapped = _engine(2, m, cap=0)
    with pytest.raises(ValueError):
        _ffi_tickerforesight.ticker_foresight(uncapped, [0])               # no TimeLimit, no default
    trade.close(); bare.close(); uncapped.close(); eng.close()


# ------------------------------------------------------------------------------------------ 8. the ceiling is one
def test_whole_episode_foresight_dominates_every_default_rule(fix):
    from goldsrl import _ffi_tickerforesight, _ffi_tickersweep
    from goldsrl.baselines import DEFAULT_TICKER_RULES
    m, E = fix["matrix"], 64
    eng = _engine(E, m, _starts(E, m, 4))
    top = _ffi_tickerforesight.ticker_foresight(eng, [0], 256)
    rules = _ffi_tickersweep.ticker_sweep(eng, DEFAULT_TICKER_RULES, 256)
    assert (top["length"] == 256).all() and not top["depleted"].any()
    assert (top["final_assets"][0][None] >= rules["final_assets"] * (1 - 1e-12)).all()
    assert (top["final_assets"][0] > rules["final_assets"].max(axis=0)).any()
    assert np.abs(np.log(top["final_assets"][0] + 1e-4) - np.log(10.0 + 1e-4) - top["bound"][0]).max() <= 1e-12
    eng.close()


# ------------------------------------------------------------------------------------------ 9. monitor and script
class _Writer(object):
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def flush(self):
        pass


def test_ticker_ceiling_of_the_monitor(fix):
    from goldsrl import _ffi_gated
    from goldsrl.agents.a3c.policy_monitor import GatedPolicyMonitor, make_ticker_eval_engine
    from goldsrl.baselines import TickerForesightCeiling
    m, w = fix["matrix"], _Writer()
    mon = GatedPolicyMonitor(m, summary_writer=w, n_envs=5, max_episode_steps=48)
    total = mon.ticker_ceiling()
    eng = make_ticker_eval_engine(m, 5, max_episode_steps=48)             # a direct call on the same seeded windows
    eng.reset()
    direct = TickerForesightCeiling(eng)
    st = direct.run()
    assert np.array_equal(eng.get_state("TICKER_START"), mon.net.eng.get_state("TICKER_START"))
    for k in PAIR_KEYS + ("final_assets",):
        assert st[k].tobytes() == mon.ceiling_stats[k].tobytes(), k
    assert total == mon.ceiling_total_reward == direct.ceiling() == st["total"][5].mean() and total > 0
    assert [r[0] for r in mon.ceiling_table] == [1, 2, 4, 16, 64, 0] and mon.ceiling_table == direct.table()
    assert (mon.net.eng.get_state("ELAPSED") == 0).all() and (mon.net.eng.get_state("TICKER_IDX") == 0).all()
    mon.write_ceiling_scalars(3)
    assert w.rows == [("eval/ceiling_total_reward", total, 3)]             # no floor and no evaluation yet
    _, _, floor = mon.ticker_baseline()
    assert total >= floor
    mon.eval_once(_ffi_gated.default_init_gated(3))
    del w.rows[:]
    mon.write_ceiling_scalars(4)
    mean = mon.log["mean_total_reward"][-1]
    assert w.rows == [("eval/ceiling_total_reward", total, 4), ("eval/mean_total_reward_share_of_gap", (mean - floor) / (total - floor), 4)]
    mon.log["mean_total_reward"].append(floor)                             # a trader at the floor has covered none of the gap
    del w.rows[:]
    mon.write_ceiling_scalars(5)
    assert w.rows[1] == ("eval/mean_total_reward_share_of_gap", 0.0, 5)
    mon.log["mean_total_reward"].append(total)
    del w.rows[:]
    mon.write_ceiling_scalars(6)
    assert w.rows[1] == ("eval/mean_total_reward_share_of_gap", 1.0, 6)
    assert mon.ticker_ceiling([0, 3]) == total and len(mon.ceiling_table) == 2
    eng.close(); mon.close()


def _price_file(tmp_path):
    rng = np.random.RandomState(4)
    days = 600
    closes = 100.0 * np.exp(np.cumsum(rng.normal(3e-4, 0.008, size=days)))
    opens = closes * np.exp(rng.normal(0, 0.003, size=days))
    table = tmp_path / "table.npz"
    np.savez(table, Open=opens, Close=closes, Volume=rng.uniform(1e5, 5e5, size=days).round())
    return table


def test_train_ticker_ceiling_flag(tmp_path):
    from goldsrl import utils_tfevents
    from goldsrl.scripts import train_ticker
    table = _price_file(tmp_path)
    out = tmp_path / "run"
    train_ticker.main(["--table", str(table), "--envs", "64", "--steps", "4", "--updates", "2", "--eval-envs", "8", "--eval-every", "1",
                       "--baseline", "--ceiling", "--out", str(out)])
    (events,) = glob.glob(os.path.join(str(out), "events.out.tfevents.*"))
    scalars = {}
    for tag, value, step, _ in utils_tfevents.read_scalars(events):
        scalars.setdefault(tag, []).append((step, value))
    steps = [s for s, _ in scalars["eval/mean_total_reward"]]
    for tag in ("eval/baseline_total_reward", "eval/ceiling_total_reward", "eval/mean_total_reward_share_of_gap"):
        assert [s for s, _ in scalars[tag]] == steps and len(steps) == 2, tag
    c = [v for _, v in scalars["eval/ceiling_total_reward"]]
    b = [v for _, v in scalars["eval/baseline_total_reward"]]
    assert c[0] == c[1] and c[0] > b[0] >= 0                               # one run serves every evaluation
    for (_, mean), (_, share) in zip(scalars["eval/mean_total_reward"], scalars["eval/mean_total_reward_share_of_gap"]):
        want = (mean - b[0]) / (c[0] - b[0])
        assert abs(share - want) <= 1e-5 * max(1.0, abs(want))              # scalars are stored as float32
        assert share <= 1 + 1e-5


def test_ticker_foresight_script(tmp_path, capsys):
    from goldsrl.scripts import ticker_foresight
    table = _price_file(tmp_path)
    rec = ticker_foresight.main(["--table", str(table), "--envs", "8", "--steps", "64", "--json", str(tmp_path / "f.json")])
    text = capsys.readouterr().out
    assert "whole episode" in text and "ceiling" in text
    tot = {r["horizon"]: r["total"] for r in rec["horizons"]}
    assert list(tot) == [1, 2, 4, 16, 64, 0] and rec["ceiling"] == tot[0] == tot[64] and rec["gap"] == rec["ceiling"] - rec["floor"] >= 0
    assert tot[0] >= max(tot.values()) - 64 * 2e-7 and os.path.exists(str(tmp_path / "f.json"))
