"""CPU: the host form of the Ticker rule (goldsrl/_ffi_tickersweep.py:ticker_rule_actions) played on the float64 restatement of the
env (oracle/ticker.py) against the fixture of the unmodified reference env (tests/golden/gen_golden_ticker_rules.py), the default
rules, the selection rule, and what TickerRuleBaseline and train_ticker --baseline refuse without a device."""
import numpy as np
import pytest

from oracle import ticker as TK


def _play(matrix, starts, rule, steps):
    """`rule` on oracle/ticker.py from a reset at `starts`, every env until its own done.  Returns actions (E,steps,4) float32,
    rewards and assets (E,steps) float64, zero past the length, and the lengths."""
    from goldsrl._ffi_tickersweep import ticker_rule_actions, ticker_rule_back
    st, obs = TK.ticker_reset(matrix, starts)
    E = len(starts)
    actions, rewards, assets = np.zeros((E, steps, 4), np.float32), np.zeros((E, steps)), np.zeros((E, steps))
    length, live = np.zeros(E, np.int32), np.ones(E, bool)
    for t in range(steps):
        back = ticker_rule_back(rule, matrix, st["start"], st["idx"])
        a = ticker_rule_actions(rule, st["cash"], st["qty"], matrix[st["start"] + st["idx"]][:, :2], back)
        _, r, done = TK.ticker_step(matrix, st, a[:, :2].astype(np.int64), a[:, 2:].astype(np.float64))
        actions[live, t], rewards[live, t], assets[live, t] = a[live], r[live], st["assets"][live]
        length[live] = t + 1
        live &= ~done
        if not live.any():
            break
    return actions, rewards, assets, length


def test_default_rules_shape_and_order():
    from goldsrl.baselines import DEFAULT_TICKER_RULES
    r = DEFAULT_TICKER_RULES
    assert r.shape == (12, 6) and r.dtype == np.float32
    assert r[0].tolist() == [0, 0, 0, 0, 1, 0] and r[1].tolist() == [1, 0, 1, 0, 0.5, 0] and r[2].tolist() == [0, 1, 0, 1, 0.5, 0]
    assert (r[3:6, :4] == 0.5).all() and r[3:6, 4].tolist() == [np.float32(0.25), np.float32(0.05), np.float32(0.01)] and (r[3:6, 5] == 0).all()
    assert (r[6:10, :5] == [1, 0, 0, 1, 0.5]).all() and r[6:10, 5].tolist() == [2, 8, 32, 128]
    assert (r[10:, :5] == [1, 0, 0, 0, 0.5]).all() and r[10:, 5].tolist() == [8, 32]


def test_host_rule_on_the_oracle_reproduces_the_reference_fixture(golden):
    """actions and assets bit for bit, rewards within 1e-13 (the float64 reward tolerance of tests/test_gpu_ticker.py:76)"""
    from goldsrl.baselines import DEFAULT_TICKER_RULES
    g = golden("ticker_rules")
    matrix, starts, rules = g["matrix"], g["starts"], g["rules"]
    assert rules.tobytes() == DEFAULT_TICKER_RULES.tobytes()
    for r, rule in enumerate(rules):
        a, rew, ast, n = _play(matrix, starts, rule, 256)
        assert np.array_equal(a, g["actions"][:, r]) and np.array_equal(ast, g["assets"][:, r]) and np.array_equal(n, g["length"][:, r]), r
        assert np.abs(rew - g["rewards"][:, r]).max() <= 1e-13, r
    for k, r in enumerate(g["full_rules"]):
        a, rew, ast, n = _play(matrix, starts, rules[r], 1023)
        assert np.array_equal(a, g["full_actions"][:, k]) and np.array_equal(ast, g["full_assets"][:, k]) and (n == 1023).all()
        assert np.abs(rew - g["full_rewards"][:, k]).max() <= 1e-13
    a, rew, ast, n = _play(matrix, starts, rules[int(g["dep_rule"])], 1023)
    m = int(g["dep_length"].max())
    assert np.array_equal(n, g["dep_length"]) and (n < 1023).all()
    assert np.array_equal(a[:, :m], g["dep_actions"]) and np.array_equal(ast[:, :m], g["dep_assets"])
    assert np.abs(rew[:, :m] - g["dep_rewards"]).max() <= 1e-13


def test_what_the_fixture_says_about_the_family(golden):
    g = golden("ticker_rules")
    assert (g["rewards"][:, 0] == 0).all() and (g["total"][:, 0] == 0).all()                      # hold cash totals exactly 0
    bh = g["full_actions"][:, 0]
    assert ((bh[:, :, :2] != 0).any(axis=2).sum(axis=1) == 1).all() and (bh[:, 0, :2] == [1, 0]).all()   # buy and hold trades once, at step 0
    assert (g["dep_length"] < 1023).all() and (g["dep_trades"] > 300).all()                        # the L = 2 switch pays the spread
    mean = g["total"].mean(axis=0)
    order = np.argsort(-mean, kind="stable")
    assert int(g["best_index"]) == order[0] and mean[order[0]] - mean[order[1]] > 2 * 256 * 2e-7


def test_host_rule_by_hand():
    from goldsrl._ffi_tickersweep import ticker_rule_actions, ticker_rule_back
    cash, qty, p = np.array([10.0, 0.0, 5.0]), np.array([[0, 0], [0.1, 0], [0.05, 0]], np.float64), np.array([[100.0, 50.0]] * 3)
    # buy and hold: all cash -> buy everything; fully invested -> hold; half invested -> buy with f = (1 - .5) * 10 / 5 = 1
    a = ticker_rule_actions((1, 0, 1, 0, 0.5, 0), cash, qty, p, p[:, 0])
    assert a.dtype == np.float32 and a.tolist() == [[1, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0]]      # s = .5 is inside [.5, 1.5]: hold
    a = ticker_rule_actions((1, 0, 1, 0, 0.25, 0), cash, qty, p, p[:, 0])
    assert a.tolist() == [[1, 0, 1, 0], [0, 0, 0, 0], [1, 0, 1, 0]]
    # hold cash sells what it finds: s = 1 > 0 + band only when band < 1
    assert ticker_rule_actions((0, 0, 0, 0, 1, 0), cash, qty, p, p[:, 0]).tolist() == [[0, 0, 0, 0]] * 3
    assert ticker_rule_actions((0, 0, 0, 0, 0.5, 0), cash, qty, p, p[:, 0])[1].tolist() == [2, 0, 1, 0]
    # the switch: p0 below its lookback price -> the down weights; equal -> up
    rule = (1, 0, 0, 1, 0.5, 3)
    assert ticker_rule_actions(rule, cash[:1], qty[:1], p[:1], np.array([100.5])).tolist() == [[0, 1, 0, 1]]
    assert ticker_rule_actions(rule, cash[:1], qty[:1], p[:1], np.array([100.0])).tolist() == [[1, 0, 1, 0]]
    # both buys with fractions summing above 1 (the env rescales them), float32 rounding of the fraction
    a = ticker_rule_actions((0.5, 0.5, 0.5, 0.5, 0.01, 0), np.array([3.0]), np.array([[0.04, 0.06]]), p[:1], p[:1, 0])
    assert a[0, :2].tolist() == [1, 1] and a[0, 2] == np.float32(0.1 * 10.0 / 3.0) and a[0, 3] == np.float32((0.5 - 3.0 / 10.0) * 10.0 / 3.0)
    # cash a hair below zero after a full buy: fmax keeps the divisor positive, fmin caps the fraction
    a = ticker_rule_actions((0.5, 0.5, 0.5, 0.5, 0.01, 0), np.array([-1e-16]), np.array([[0.1, 0.0]]), p[:1], p[:1, 0])
    assert a[0].tolist() == [2, 1, 0.5, 1]
    # many rules at once, and the lookback row clamped at the window's first row
    table = np.arange(40, dtype=np.float64).reshape(10, 4) + 1
    rules = np.array([(1, 0, 0, 1, 0.5, 2), (1, 0, 0, 1, 0.5, 0), (0, 0, 0, 0, 1, 9)], np.float32)
    back = ticker_rule_back(rules, table, np.array([1, 1]), np.array([0, 5]))
    assert back.tolist() == [[5, 17], [5, 25], [5, 5]]
    many = ticker_rule_actions(rules, cash[:2], qty[:2], p[:2], back)
    assert many.shape == (3, 2, 4) and many[2].tolist() == [[0, 0, 0, 0]] * 2


def test_selection_takes_the_first_on_a_tie():
    from goldsrl.baselines import TickerRuleBaseline, select_best_ticker_rule, select_best_rule
    rules = np.array([(0, 0, 0, 0, 1, 0), (1, 0, 1, 0, 0.5, 0), (0, 1, 0, 1, 0.5, 0), (1, 0, 0, 1, 0.5, 8)], np.float32)
    total = np.array([[0.0, 0.0], [1.0, 3.0], [4.0, 0.0], [0.5, 0.5]])
    assert select_best_ticker_rule(rules, total) == (1, (1.0, 0.0, 1.0, 0.0, 0.5, 0.0), 2.0)      # rules 1 and 2 tie at 2.0
    total[2, 1] = 0.25
    assert select_best_ticker_rule(rules, total) == (2, (0.0, 1.0, 0.0, 1.0, 0.5, 0.0), 2.125)
    assert select_best_ticker_rule(rules, -total)[0] == 0                                           # hold cash beats every loss
    assert select_best_rule(rules, total) == (2, (0.0, 1.0), 2.125)                                 # TradeAR1's keeps its return value
    b = TickerRuleBaseline.__new__(TickerRuleBaseline)
    b.rules, b.stats = rules, {"total": total}
    assert b.best_total() == (2, (0.0, 1.0, 0.0, 1.0, 0.5, 0.0), 2.125)


class _Engine(object):
    """what TickerRuleBaseline asks of an engine before it touches the device"""

    def __init__(self, kind, cap=1023):
        self.kind = kind
        self.cfg = type("cfg", (), {"max_episode_steps": cap})()


def test_baseline_refuses_other_envs_and_malformed_rules_without_a_device():
    from goldsrl import _ffi
    from goldsrl._ffi_tickersweep import ticker_sweep
    from goldsrl.baselines import DEFAULT_TICKER_RULES, TickerRuleBaseline
    for kind in (_ffi.ENV_SWARM, _ffi.ENV_SOLOW, _ffi.ENV_TRADE):
        with pytest.raises(ValueError, match="Ticker env only"):
            TickerRuleBaseline(_Engine(kind))
        with pytest.raises(ValueError, match="not a Ticker engine"):
            ticker_sweep(_Engine(kind), DEFAULT_TICKER_RULES)
    eng = _Engine(_ffi.ENV_TICKER)
    b = TickerRuleBaseline(eng)
    assert b.rules.tobytes() == DEFAULT_TICKER_RULES.tobytes() and b.max_episode_steps == 1023
    good = [0.5, 0.5, 0.5, 0.5, 0.1, 4]
    for shape in ((2, 5), (6,), (0, 6)):
        with pytest.raises(ValueError, match="rules must be"):
            TickerRuleBaseline(eng, np.zeros(shape))
    bad = {}
    for k, (v, word) in enumerate(((np.nan, "up0 is not finite"), (1.5, "up1 is a weight"), (-0.1, "dn0 is a weight"), (np.inf, "dn1 is not finite"),
                                   (-0.01, "band is negative"), (2.5, "lookback is not an integer"))):
        row = list(good)
        row[k] = v
        bad[word] = [good, row]
    bad["up0 \\+ up1 is above 1"] = [[0.75, 0.5, 0, 0, 0.1, 0]]
    bad["dn0 \\+ dn1 is above 1"] = [[0, 0, 0.5, 0.75, 0.1, 0]]
    bad["rule 0: lookback"] = [[0, 0, 0, 0, 0.1, 1024]]
    bad["rule 1: lookback"] = [good, [0, 0, 0, 0, 0.1, -1]]
    for word, rules in bad.items():
        with pytest.raises(ValueError, match=word):
            TickerRuleBaseline(eng, rules)
    with pytest.raises(ValueError, match="rule 1: up1"):
        TickerRuleBaseline(eng, [good, [0, 1.5, 0, 0, 0, 0]])
    with pytest.raises(ValueError, match="max_episode_steps"):
        TickerRuleBaseline(_Engine(_ffi.ENV_TICKER, cap=0))
    assert TickerRuleBaseline(_Engine(_ffi.ENV_TICKER, cap=0), max_episode_steps=40).max_episode_steps == 40


def test_baseline_flag_needs_the_device_monitor(capsys):
    from goldsrl.scripts import train_ticker
    with pytest.raises(SystemExit) as e:
        train_ticker.parse_args(["--table", "t.npz", "--baseline"])
    assert e.value.code == 2 and "--eval-envs" in capsys.readouterr().err
    assert train_ticker.parse_args(["--table", "t.npz", "--baseline", "--eval-envs", "4"]).baseline is True
    assert train_ticker.parse_args(["--table", "t.npz"]).baseline is False
