"""GPU: the scripted rule baseline sweep of the Ticker env (grl_ticker_sweep / grl_ticker_sweep_read of
include/goldsrl_tickersweep.h; csrc/ticker_sweep.hip), the baseline class, the monitor's ticker_baseline() and
train_ticker --baseline.

The yardstick of the one-launch sweep is the per-step path: grl_step with the rule's actions computed on the host
(_ffi_tickersweep.ticker_rule_actions) from the read-back TICKER_CASH / TICKER_QUANTITY / TICKER_IDX / TICKER_START runs the same
float64 operations in the same order, so a pair's actions, account and rewards -- and their sequential float64 sums -- must be the
per-step path's bits.  The per-step twin of a case is played once and shared by every sweep of that case.  The reference env pins
the values through tests/golden/ticker_rules.npz (the unmodified TickerEnv)."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASH, HOLD0, HOLD1 = (0, 0, 0, 0, 1, 0), (1, 0, 1, 0, 0.5, 0), (0, 1, 0, 1, 0.5, 0)
SWITCH2 = (1, 0, 0, 1, 0.5, 2)
# hold cash; the equal mix with no band (trades at every step; buys both assets whenever both shares are below a half); the L = 2
# switch (full sells and full buys, two steps per switch); the cash switch; the inverse asset bought and held; a switch between two uneven mixes with a
# narrow band (partial buys and sells); the asset bought and held under a lookback longer than the test
RULES7 = np.array([CASH, (0.5, 0.5, 0.5, 0.5, 0, 0), SWITCH2, (1, 0, 0, 0, 0.5, 8), HOLD1, (0.3, 0.6, 0.6, 0.3, 0.02, 5), (1, 0, 1, 0, 0.5, 100)],
                  np.float32)
PAIR_KEYS = ("total", "sum_sq", "min", "max", "length", "trades", "finished", "depleted")
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


def _play(eng, rule, steps, matrix, reset=True):
    """The per-step path: `steps` calls of step(the rule's actions on the read-back state).  Returns actions (steps,E,4) and rewards
    (steps,E) float32, dones (steps,E) bool, the assets after every step (steps,E) float64 (the reset value where the step ended an
    episode) and the elapsed counters at the start."""
    from goldsrl._ffi_tickersweep import ticker_rule_actions, ticker_rule_back
    E = eng.E
    if reset:
        eng.reset()
    el0 = eng.get_state("ELAPSED").copy()
    actions, rewards = np.zeros((steps, E, 4), np.float32), np.zeros((steps, E), np.float32)
    dones, assets = np.zeros((steps, E), bool), np.zeros((steps, E))
    for t in range(steps):
        cash, qty = eng.get_state("TICKER_CASH"), eng.get_state("TICKER_QUANTITY")
        idx, start = eng.get_state("TICKER_IDX"), eng.get_state("TICKER_START")
        actions[t] = ticker_rule_actions(rule, cash, qty, matrix[start + idx][:, :2], ticker_rule_back(rule, matrix, start, idx))
        eng.step(actions[t])
        rewards[t], dones[t], assets[t] = eng.read("reward"), eng.read("done") > 0, eng.get_state("TICKER_ASSETS")
    return actions, rewards, dones, assets, el0


def _twin_stats(twin, max_steps, cap=0):
    """What the sweep keeps, from the per-step path up to each env's first done: sequential float64 sums (np.cumsum adds in order),
    float32 min / max, the trades, and final_assets where the pair did not end (an ended env's assets are already the reset value)."""
    actions, rewards, dones, assets, el0 = twin
    steps, E = rewards.shape
    ended = dones.any(axis=0)
    first = np.where(ended, dones.argmax(axis=0) + 1, steps)
    n = np.minimum(first, max_steps)
    finished = ended & (first <= max_steps)
    at_limit = (el0 + n >= cap) if cap > 0 else np.zeros(E, bool)
    r64 = rewards.astype(np.float64)
    c1, c2 = np.cumsum(r64, axis=0), np.cumsum(r64 * r64, axis=0)
    env = np.arange(E)
    live = np.arange(steps)[:, None] < n[None]
    traded = (actions[:, :, :2] != 0).any(axis=2) & live
    return {"total": c1[n - 1, env], "sum_sq": c2[n - 1, env],
            "min": np.where(live, rewards, np.inf).min(axis=0).astype(np.float32),
            "max": np.where(live, rewards, -np.inf).max(axis=0).astype(np.float32),
            "length": n.astype(np.int32), "trades": traded.sum(axis=0).astype(np.int32), "finished": finished.astype(np.uint8),
            "depleted": (finished & ~at_limit).astype(np.uint8), "final_assets": assets[n - 1, env], "open": ~finished}


def _assert_bits(got, want, r, msg):
    for k in PAIR_KEYS:
        assert got[k][r].dtype == want[k].dtype, (k, got[k].dtype, want[k].dtype)
        assert got[k][r].tobytes() == want[k].tobytes(), "%s: %s of rule %d differs" % (msg, k, r)
    o = want["open"]
    assert got["final_assets"][r][o].tobytes() == want["final_assets"][o].tobytes(), "%s: final_assets of rule %d differs" % (msg, r)


def _assert_trace(got, twin, want, r, env, max_steps, msg):
    actions, rewards, _, assets, _ = twin
    n = int(want["length"][env])
    assert got["trace_actions"][r, :n].tobytes() == actions[:n, env].tobytes(), "%s: trace_actions of rule %d" % (msg, r)
    assert got["trace_rewards"][r, :n].tobytes() == rewards[:n, env].tobytes(), "%s: trace_rewards of rule %d" % (msg, r)
    k = n if want["open"][env] else n - 1                                  # the step that ends an episode auto-resets the account
    assert got["trace_assets"][r, :k].tobytes() == assets[:k, env].tobytes(), "%s: trace_assets of rule %d" % (msg, r)
    assert got["trace_assets"][r, n - 1] == got["final_assets"][r, env]
    assert not got["trace_rewards"][r, n:].any() and not got["trace_assets"][r, n:].any() and not got["trace_actions"][r, n:].any()


# ------------------------------------------------------------------------------------------ 1. bit for bit from a reset
@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
def test_sweep_is_the_per_step_path_bit_for_bit(E, fix):
    from goldsrl import _ffi_tickersweep
    m = fix["matrix"]
    eng = _engine(E, m, _starts(E, m, E))
    twin = [_play(eng, rule, 64, m) for rule in RULES7]                    # played once, shared by the sweeps below
    a = twin[1][0]
    assert (a[0, :, :2] == 1).all() and (a[1:, :, :2] != 0).any(axis=2).mean() > 0.9             # both bought; then a trade at (nearly) every step
    assert (twin[2][0][:, :, :2] == 2).any() and (twin[5][0][:, :, 2:] % 1 != 0).any()           # full sells; partial trades
    assert not twin[0][0].any() and not twin[0][1].any()                                          # hold cash
    if E > 1:
        assert len(np.unique(twin[4][1][5])) > 1                           # the envs really differ
    env = E - 1
    for n_rules in (1, 2, 5, 7):
        for max_steps in (48, 64):
            eng.reset()
            got = _ffi_tickersweep.ticker_sweep(eng, RULES7[:n_rules], max_steps, trace_env=env)
            assert got["total"].shape == (n_rules, E) and got["trace_actions"].shape == (n_rules, max_steps, 4)
            for r in range(n_rules):
                want = _twin_stats(twin[r], max_steps)
                _assert_bits(got, want, r, "n_rules %d max_steps %d" % (n_rules, max_steps))
                _assert_trace(got, twin[r], want, r, env, max_steps, "n_rules %d max_steps %d" % (n_rules, max_steps))
            assert (got["length"] == max_steps).all() and not got["finished"].any()
    eng.close()


def test_three_rules_over_the_whole_window(fix):
    from goldsrl import _ffi_tickersweep
    m, starts = fix["matrix"], fix["starts"]
    rules = np.array([HOLD0, (0.5, 0.5, 0.5, 0.5, 0.01, 0), (1, 0, 0, 1, 0.5, 32)], np.float32)
    eng = _engine(3, m, starts)
    got = _ffi_tickersweep.ticker_sweep(eng, rules, trace_env=1)           # max_steps: the engine's 1 023
    assert (got["length"] == 1023).all() and (got["finished"] == 1).all() and not got["depleted"].any()
    assert (got["trades"][0] == 1).all() and (got["trades"][2] > 10).all()
    for r, rule in enumerate(rules):
        twin = _play(eng, rule, 1023, m)
        want = _twin_stats(twin, 1023, 1023)
        _assert_bits(got, want, r, "1023 steps")
        _assert_trace(got, twin, want, r, 1, 1023, "1023 steps")
    eng.close()


# ------------------------------------------------------------------------------------------ 2. mid-episode start
def test_sweep_from_a_mid_episode_state(fix):
    """After 10 random-action steps idx = elapsed = 10 and q is nonzero; lookbacks 2, 5 and 8 reach back inside the episode, 100
    reaches past its first row.  Every third env then holds a dust position, which the last rule (all cash, no band) sells: the
    env's sale of next to nothing.  (An exactly empty position has share 0, never above a band's upper edge: no rule sells it.)"""
    from goldsrl import _ffi_tickersweep
    m, E, cap = fix["matrix"], 70, 40
    rules = np.concatenate([RULES7, np.array([(0, 0, 0, 0, 0, 0)], np.float32)])

    def prefix():
        eng = _engine(E, m, _starts(E, m, 5), cap=cap)
        rng = np.random.RandomState(1)
        for _ in range(10):
            a = np.concatenate([rng.randint(0, 3, size=(E, 2)), rng.uniform(0, 1, size=(E, 2))], axis=1).astype(np.float32)
            eng.step(a)
        q, c = eng.get_state("TICKER_QUANTITY"), eng.get_state("TICKER_CASH")
        q[::3], c[::3] = [1e-300, 0.0], 10.0
        eng.set_state("TICKER_QUANTITY", q)
        eng.set_state("TICKER_CASH", c)
        eng.set_state("TICKER_ASSETS", np.where(np.arange(E) % 3 == 0, 10.0, eng.get_state("TICKER_ASSETS")))
        return eng

    eng = prefix()
    assert (eng.get_state("TICKER_IDX") == 10).all() and (eng.get_state("ELAPSED") == 10).all() and (eng.get_state("TICKER_QUANTITY") > 0).any()
    full = _ffi_tickersweep.ticker_sweep(eng, rules, 64, trace_env=3)
    cut = _ffi_tickersweep.ticker_sweep(eng, rules, 9, trace_env=69)
    for r, rule in enumerate(rules):
        t = prefix()
        twin = _play(t, rule, cap - 10, m, reset=False)
        t.close()
        assert twin[2][-1].all() and not twin[2][:-1].any()               # the TimeLimit, 30 steps on
        if r == 1:
            # The targets sum to at most 1, so a rule never asks for more than the cash: the fractions of a double buy sum to 1 up to
            # rounding, and above 1 only by the float32 rounding of the two.  That is the case the env rescales.
            a = twin[0]
            assert ((a[:, :, :2] == 1).all(axis=2) & (a[:, :, 2:].astype(np.float64).sum(axis=2) > 1)).any()
        for got, k, env in ((full, 64, 3), (cut, 9, 69)):
            want = _twin_stats(twin, k, cap)
            _assert_bits(got, want, r, "max_steps %d" % k)
            _assert_trace(got, twin, want, r, env, k, "max_steps %d" % k)
    assert (full["length"] == 30).all() and (full["finished"] == 1).all() and not full["depleted"].any()
    assert (cut["length"] == 9).all() and not cut["finished"].any()
    assert full["trace_actions"][7, 0].tolist() == [2, 0, 1, 0] and (full["trades"][7, ::3] == 1).all()   # the dust of env 3 is sold, once
    eng.close()


# ------------------------------------------------------------------------------------------ 3. the ends
def test_depletion_ends_a_pair_as_the_step_path_does(fix):
    from goldsrl import _ffi_tickersweep
    m, starts = fix["matrix"], fix["starts"]
    rules = np.array([SWITCH2, CASH], np.float32)
    eng = _engine(3, m, starts)
    got = _ffi_tickersweep.ticker_sweep(eng, rules, 1023, trace_env=2)
    assert np.array_equal(got["length"][0], fix["dep_length"]) and (got["depleted"][0] == 1).all() and (got["finished"][0] == 1).all()
    assert (got["final_assets"][0] < 1).all() and np.array_equal(got["trades"][0], fix["dep_trades"])
    assert (got["length"][1] == 1023).all() and (got["finished"][1] == 1).all() and not got["depleted"][1].any() and (got["total"][1] == 0).all()
    steps = int(fix["dep_length"].max())
    twin = _play(eng, rules[0], steps, m)
    want = _twin_stats(twin, 1023, 1023)
    _assert_bits(got, want, 0, "depletion")
    _assert_trace(got, twin, want, 0, 2, 1023, "depletion")
    eng.reset()                                                            # the twin has played on
    short = _ffi_tickersweep.ticker_sweep(eng, rules, 100)               # max_steps shorter than the depletion
    _assert_bits(short, _twin_stats(twin, 100, 1023), 0, "max_steps 100")
    assert (short["length"] == 100).all() and not short["finished"].any() and not short["depleted"].any()
    eng.close()


def test_window_end_stops_a_pair_without_the_window_error(fix):
    from goldsrl import _ffi_tickersweep
    m, E = fix["matrix"], 5
    eng = _engine(E, m, _starts(E, m, 2), cap=0)                           # no TimeLimit
    eng.set_state("TICKER_IDX", np.full(E, 1000, np.int32))
    rules = RULES7[[2, 4, 6]]
    got = _ffi_tickersweep.ticker_sweep(eng, rules, 64, trace_env=0)
    assert (got["length"] == 23).all() and not got["finished"].any() and not got["depleted"].any()       # rows 1000 .. 1022 are traded at
    cut = _ffi_tickersweep.ticker_sweep(eng, rules, 7)
    assert (cut["length"] == 7).all() and not cut["finished"].any()
    eng.step(np.zeros((E, 4), np.float32))                                 # err_flag is still 0: wait() raises nothing
    assert (eng.get_state("TICKER_IDX") == 1001).all()
    for r, rule in enumerate(rules):
        eng.reset()
        eng.set_state("TICKER_IDX", np.full(E, 1000, np.int32))
        twin = _play(eng, rule, 23, m, reset=False)                        # the 24th step is the one the step path refuses
        for g, k in ((got, 64), (cut, 7)):
            _assert_bits(g, _twin_stats(twin, k), r, "window end, max_steps %d" % k)
        _assert_trace(got, twin, _twin_stats(twin, 64), r, 0, 64, "window end")
    eng.set_state("TICKER_IDX", np.full(E, 1023, np.int32))                # nothing left to play
    none = _ffi_tickersweep.ticker_sweep(eng, rules, 5)
    assert (none["length"] == 0).all() and (none["total"] == 0).all() and not none["finished"].any() and np.isnan(none["mean"]).all()
    eng.close()


# ------------------------------------------------------------------------------------------ 4. the handle is untouched
def test_sweep_leaves_the_handle_untouched_and_grows_its_buffers(fix):
    from goldsrl import _ffi_tickersweep
    m = fix["matrix"]

    def make():
        eng = _engine(65, m, cap=24, seed=7)                               # window starts drawn on the device
        eng.episodes_enable()
        rng = np.random.RandomState(2)
        for _ in range(3):
            a = np.concatenate([rng.randint(0, 3, size=(65, 2)), rng.uniform(0, 1, size=(65, 2))], axis=1).astype(np.float32)
            eng.step(a)
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
    second = _ffi_tickersweep.ticker_sweep(eng, RULES7, 40, trace_env=64)  # the larger one first, with a trace
    same(before, everything(eng))
    assert (second["length"] == 21).all() and (second["finished"] == 1).all() and not second["depleted"].any()
    assert second["trace_rewards"].shape == (7, 40) and not second["trace_rewards"][:, 21:].any() and not second["trace_actions"][:, 21:].any()
    first = _ffi_tickersweep.ticker_sweep(eng, RULES7[:3], 30)             # a smaller one in the grown buffers
    same(before, everything(eng))
    for k in PAIR_KEYS + ("final_assets",):
        assert second[k][:3].tobytes() == first[k].tobytes(), k
    third = _ffi_tickersweep.ticker_sweep(eng, np.concatenate([RULES7, RULES7]), 50, trace_env=0)       # every buffer grows
    same(before, everything(eng))
    assert third["trace_assets"].shape == (14, 50) and (third["length"] == 21).all()
    again = _ffi_tickersweep.ticker_sweep(eng, RULES7, 40, trace_env=64)
    for k in PAIR_KEYS + ("final_assets", "trace_rewards", "trace_assets", "trace_actions"):
        assert again[k].tobytes() == second[k].tobytes(), k
        assert third[k][7:].tobytes() == third[k][:7].tobytes(), k
    act = np.tile(np.array([1, 2, 0.4, 0.7], np.float32), (65, 1))
    eng.step(act); twin.step(act)                                          # a step after the sweep gives the bits it gives without it
    same(everything(twin), everything(eng))
    eng.close(); twin.close()


# ------------------------------------------------------------------------------------------ 5. pinned to the reference
def test_sweep_against_the_reference_env(fix):
    """tests/golden/ticker_rules.npz: the unmodified TickerEnv under the twelve default rules.  Actions and assets bit for bit; step
    rewards within 2e-7 (the float32 reward tolerance of tests/test_gpu_ticker.py:55), totals within length x 2e-7.  The fixture's
    best and second-best mean totals are further apart than twice that, so the arg-max cannot flip."""
    from goldsrl.baselines import DEFAULT_TICKER_RULES, TickerRuleBaseline
    m, starts = fix["matrix"], fix["starts"]
    eng = _engine(3, m, starts)
    b = TickerRuleBaseline(eng, max_episode_steps=256)
    assert b.rules.tobytes() == DEFAULT_TICKER_RULES.tobytes() == fix["rules"].tobytes()
    worst_r = worst_t = 0.0
    for env in range(3):
        st = b.run(trace_env=env)
        assert (st["length"] == 256).all() and not st["finished"].any()
        assert np.array_equal(st["trace_actions"], fix["actions"][env]) and np.array_equal(st["trace_assets"], fix["assets"][env])
        worst_r = max(worst_r, float(np.abs(st["trace_rewards"] - fix["rewards"][env]).max()) / 2e-7)
    worst_t = float(np.abs(st["total"] - fix["total"].T).max()) / (256 * 2e-7)
    assert (st["total"][0] == 0).all() and (st["trades"][1] == 1).all()
    i, rule, total = b.best_total()
    # the two long cases and the depletion case
    long_rules = np.concatenate([DEFAULT_TICKER_RULES[fix["full_rules"]], DEFAULT_TICKER_RULES[[int(fix["dep_rule"])]]])
    for env in range(3):
        lg = TickerRuleBaseline(eng, long_rules).run(trace_env=env)
        assert np.array_equal(lg["trace_actions"][:2], fix["full_actions"][env]) and np.array_equal(lg["trace_assets"][:2], fix["full_assets"][env])
        n = fix["dep_actions"].shape[1]
        assert np.array_equal(lg["trace_actions"][2, :n], fix["dep_actions"][env]) and np.array_equal(lg["trace_assets"][2, :n], fix["dep_assets"][env])
        worst_r = max(worst_r, float(np.abs(lg["trace_rewards"][:2] - fix["full_rewards"][env]).max()) / 2e-7,
                      float(np.abs(lg["trace_rewards"][2, :n] - fix["dep_rewards"][env]).max()) / 2e-7)
    assert np.array_equal(lg["length"][2], fix["dep_length"]) and (lg["depleted"][2] == 1).all() and (lg["length"][:2] == 1023).all()
    worst_t = max(worst_t, float(np.abs(lg["total"][:2] - fix["full_total"].T).max()) / (1023 * 2e-7),
                  float((np.abs(lg["total"][2] - fix["dep_total"]) / (fix["dep_length"] * 2e-7)).max()))
    print("ticker_rules worst differences in units of the bound: step rewards %.3g, totals %.3g; best rule %d %r mean total %r"
          % (worst_r, worst_t, i, rule, total))
    assert worst_r <= 1.0 and worst_t <= 1.0
    assert i == int(fix["best_index"]) and rule == tuple(float(v) for v in DEFAULT_TICKER_RULES[i])
    assert abs(total - fix["total"].mean(axis=0)[i]) <= 256 * 2e-7
    eng.close()


# ------------------------------------------------------------------------------------------ 6. refusals
def test_sweep_refuses_bad_arguments(fix):
    from goldsrl import _ffi, _ffi_tickersweep
    lib = _ffi.load_library(extra_signatures=_ffi_tickersweep.TICKER_SWEEP_SIGNATURES)
    m, P = fix["matrix"], _ffi._ptr
    eng = _engine(4, m)
    buf = np.zeros((2, 4), np.float64)
    assert lib.grl_ticker_sweep_read(eng.h, b"total", P(buf), buf.nbytes) == _ffi.E_STATE          # before the first sweep
    good = np.tile(np.array([0.5, 0.5, 0.5, 0.5, 0.1, 4], np.float32), (4097, 1))
    for n_rules, max_steps, trace_env in ((0, 4, -1), (4097, 4, -1), (-1, 4, -1), (2, 0, -1), (2, 4, 4), (2, 4, -2)):
        assert lib.grl_ticker_sweep(eng.h, P(good), n_rules, max_steps, trace_env) == _ffi.E_INVALID
    assert lib.grl_ticker_sweep(eng.h, None, 2, 4, -1) == _ffi.E_INVALID and b"null" in lib.grl_last_error(eng.h)
    cases = [(k, v, b"rule 1: " + name + b" is not finite") for k, name in enumerate((b"up0", b"up1", b"dn0", b"dn1", b"band", b"lookback"))
             for v in (np.nan, np.inf, -np.inf)]
    cases += [(k, v, b"rule 1: " + name + b" is a weight outside") for k, name in enumerate((b"up0", b"up1", b"dn0", b"dn1")) for v in (-0.25, 1.5)]
    cases += [(0, 0.75, b"rule 1: up0 + up1 is above 1"), (3, 0.75, b"rule 1: dn0 + dn1 is above 1"), (4, -0.5, b"rule 1: band is negative")]
    cases += [(5, v, b"rule 1: lookback is not an integer in 0..1023") for v in (-1, 0.5, 1024, 3.25)]
    for k, v, msg in cases:
        x = good[:2].copy()
        x[1, k] = v
        assert lib.grl_ticker_sweep(eng.h, P(x), 2, 4, -1) == _ffi.E_INVALID, (k, v)
        assert msg in lib.grl_last_error(eng.h), (k, v, lib.grl_last_error(eng.h))
        with pytest.raises(ValueError):
            _ffi_tickersweep.ticker_sweep(eng, x, 4)
    edge = np.array([(1, 0, 0, 1, 0, 1023), (0, 0, 0, 0, 0, 0)], np.float32)                       # the edges of the ranges play
    assert lib.grl_ticker_sweep(eng.h, P(edge), 2, 4, 3) == _ffi.OK
    eng.step_async(np.zeros((4, 4), np.float32))
    assert lib.grl_ticker_sweep(eng.h, P(good), 2, 4, -1) == _ffi.E_INVALID and b"in flight" in lib.grl_last_error(eng.h)
    eng.wait()
    bare = _ffi.Engine(_ffi.ENV_TICKER, 4)                                 # no price table yet
    assert lib.grl_ticker_sweep(bare.h, P(good), 2, 4, -1) == _ffi.E_INVALID and b"table" in lib.grl_last_error(bare.h)
    _ffi_tickersweep.ticker_sweep(eng, good[:2], 4)
    assert lib.grl_ticker_sweep_read(eng.h, b"total", P(buf), buf.nbytes) == _ffi.OK
    assert lib.grl_ticker_sweep_read(eng.h, b"total", P(buf), buf.nbytes - 8) == _ffi.E_SIZE
    assert lib.grl_ticker_sweep_read(eng.h, b"trades", P(buf), buf.nbytes) == _ffi.E_SIZE
    assert lib.grl_ticker_sweep_read(eng.h, b"nothing", P(buf), buf.nbytes) == _ffi.E_INVALID
    assert lib.grl_ticker_sweep_read(eng.h, None, P(buf), buf.nbytes) == _ffi.E_INVALID
    assert lib.grl_ticker_sweep_read(eng.h, b"total", None, buf.nbytes) == _ffi.E_INVALID
    for name in (b"trace_rewards", b"trace_assets", b"trace_actions"):                             # the last sweep traced no env
        assert lib.grl_ticker_sweep_read(eng.h, name, P(buf), buf.nbytes) == _ffi.E_STATE
    trade = _ffi.Engine(_ffi.ENV_TRADE, 4, n_assets=2)
    assert lib.grl_ticker_sweep(trade.h, P(good), 2, 4, -1) == _ffi.E_INVALID
    assert lib.grl_ticker_sweep_read(trade.h, b"total", P(buf), buf.nbytes) == _ffi.E_INVALID
    with pytest.raises(ValueError):
        _ffi_tickersweep.ticker_sweep(trade, good[:2], 4)
    uncapped = _engine(2, m, cap=0)
    with pytest.raises(ValueError):
        _ffi_tickersweep.ticker_sweep(uncapped, good[:2])                  # no TimeLimit, no default
    trade.close(); bare.close(); uncapped.close(); eng.close()


# ------------------------------------------------------------------------------------------ 7. monitor and script
class _Writer(object):
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def flush(self):
        pass


def test_ticker_baseline_leaves_the_evaluation_alone(fix):
    from goldsrl import _ffi_gated
    from goldsrl.agents.a3c.policy_monitor import GatedPolicyMonitor
    from goldsrl.baselines import DEFAULT_TICKER_RULES
    m, w = fix["matrix"], _Writer()
    mon = GatedPolicyMonitor(m, summary_writer=w, n_envs=5, max_episode_steps=48)
    twin = GatedPolicyMonitor(m, n_envs=5, max_episode_steps=48)
    params = _ffi_gated.default_init_gated(3)
    i, rule, total = mon.ticker_baseline()
    assert (i, rule) == mon.baseline_rule and total == mon.baseline_total_reward and np.isfinite(total)
    assert rule == tuple(float(v) for v in DEFAULT_TICKER_RULES[i])
    st = mon.baseline_stats
    assert st["total"].shape == (12, 5) and (st["length"] == 48).all() and (st["finished"] == 1).all()
    assert (st["total"][0] == 0).all() and (st["trades"][0] == 0).all()    # hold cash totals exactly 0
    assert total == st["total"].mean(axis=1).max() and total >= 0
    starts = mon.net.eng.get_state("TICKER_START")
    assert len(np.unique(starts)) > 1 and (mon.net.eng.get_state("ELAPSED") == 0).all() and (mon.net.eng.get_state("TICKER_IDX") == 0).all()
    for _ in range(2):                                                     # every evaluation plays the windows the baseline played
        got, want = mon.eval_once(params), twin.eval_once(params)
        assert got == want and mon.total_rewards.tobytes() == twin.total_rewards.tobytes()
        assert np.array_equal(mon.net.eng.get_state("TICKER_START"), starts) and np.array_equal(twin.net.eng.get_state("TICKER_START"), starts)
    n = len(w.rows)
    mon.write_baseline_scalars(17)
    assert w.rows[n:] == [("eval/baseline_total_reward", total, 17),
                          ("eval/mean_total_reward_minus_baseline", mon.log["mean_total_reward"][-1] - total, 17)]
    assert mon.ticker_baseline([CASH, HOLD0])[0] in (0, 1)
    with pytest.raises(ValueError, match="TradeAR1 env only"):
        mon.rule_baseline()                                                # the trading-rule baseline stays TradeAR1's
    with pytest.raises(ValueError, match="Solow env only"):
        mon.baseline()
    twin.write_baseline_scalars(17)                                        # no baseline yet, no writer: nothing to write
    mon.close(); twin.close()


def test_train_ticker_baseline_flag(tmp_path):
    from goldsrl import utils_tfevents
    from goldsrl.scripts import train_ticker
    rng = np.random.RandomState(4)
    days = 600
    closes = 100.0 * np.exp(np.cumsum(rng.normal(3e-4, 0.008, size=days)))
    opens = closes * np.exp(rng.normal(0, 0.003, size=days))
    table = tmp_path / "table.npz"
    np.savez(table, Open=opens, Close=closes, Volume=rng.uniform(1e5, 5e5, size=days).round())

    def run(name, extra):
        out = tmp_path / name
        train_ticker.main(["--table", str(table), "--envs", "64", "--steps", "4", "--updates", "2", "--eval-envs", "3", "--eval-every", "1",
                           "--out", str(out)] + extra)
        (events,) = glob.glob(os.path.join(str(out), "events.out.tfevents.*"))
        scalars = {}
        for tag, value, step, _ in utils_tfevents.read_scalars(events):
            scalars.setdefault(tag, []).append((step, value))
        return scalars

    plain, base = run("plain", []), run("baseline", ["--baseline"])
    new = {"eval/baseline_total_reward", "eval/mean_total_reward_minus_baseline"}
    assert not new & set(plain) and set(base) == set(plain) | new
    for tag in new:
        assert [s for s, _ in base[tag]] == [s for s, _ in base["eval/mean_total_reward"]] and len(base[tag]) == 2
    b = [v for _, v in base["eval/baseline_total_reward"]]
    assert b[0] == b[1] and np.isfinite(b[0]) and b[0] >= 0                # one run serves every evaluation; hold cash is rule 0
    for (_, mean), (_, d), bv in zip(base["eval/mean_total_reward"], base["eval/mean_total_reward_minus_baseline"], b):
        assert abs(d - (mean - bv)) <= 1e-6 * max(1.0, abs(mean), abs(bv))  # scalars are stored as float32
    for tag in plain:
        assert [s for s, _ in base[tag]] == [s for s, _ in plain[tag]], tag
