"""CPU: the selection rule, the default rules and the host form of the rule of the scripted trading-rule baseline
(goldsrl/baselines.py:TradingRuleBaseline, goldsrl/_ffi_tradesweep.py:rule_actions), the fixture of the unmodified reference env
(tests/golden/gen_golden_trade_rules.py), and the --baseline flag's parser check."""
import numpy as np
import pytest


def test_default_rules_shape_and_order():
    from goldsrl.baselines import DEFAULT_TRADE_RULES
    assert DEFAULT_TRADE_RULES.shape == (9, 2) and DEFAULT_TRADE_RULES.dtype == np.float32
    assert list(DEFAULT_TRADE_RULES[:8, 0]) == [0, 1, 2, 5, 10, 20, 50, 100] and (DEFAULT_TRADE_RULES[:8, 1] == 0).all()
    assert tuple(DEFAULT_TRADE_RULES[8]) == (0, 1)


def test_best_total_on_canned_arrays_and_a_tie():
    from goldsrl.baselines import TradingRuleBaseline, select_best_rule
    rules = np.array([(0, 0), (1, 0), (2, 0.5), (0, 1)], np.float32)
    total = np.array([[0.0, 0.0], [1.0, 3.0], [4.0, 0.0], [0.5, 0.5]])
    assert select_best_rule(rules, total) == (1, (1.0, 0.0), 2.0)        # rules 1 and 2 tie at 2.0: the first wins
    total[2, 1] = 0.25
    assert select_best_rule(rules, total) == (2, (2.0, 0.5), 2.125)
    # best_total() is a pure function of the statistics: a baseline object holding them needs no engine
    b = TradingRuleBaseline.__new__(TradingRuleBaseline)
    b.rules, b.stats = rules, {"total": total}
    assert b.best_total() == (2, (2.0, 0.5), 2.125)
    assert select_best_rule(rules, -total)[0] == 0                       # hold cash, total 0, beats every loss


def test_host_rule_at_the_clamp_edges():
    """clip(bias - gain * (p - 1), -1, 1) by hand: p = 1 gives the bias; x = +-1 exactly stays; beyond is clamped."""
    from goldsrl._ffi_tradesweep import rule_actions
    a = rule_actions((4.0, 0.0), np.array([1.0, 0.75, 1.25, 0.5, 1.5, 0.875]))
    assert a.dtype == np.float32 and list(a) == [0.0, 1.0, -1.0, 1.0, -1.0, 0.5]
    assert list(rule_actions((0.0, 0.25), np.array([0.1, 1.0, 7.0]))) == [0.25, 0.25, 0.25]         # gain 0: the constant action
    assert list(rule_actions((1000.0, 0.3), np.array([1.0, 0.9993, 1.0013]))) == [np.float32(0.3), 1.0, -1.0]
    assert list(rule_actions((0.0, 0.0), np.array([0.5, 2.0]))) == [0.0, 0.0]
    # float32 rules are widened, not the other way round: gain 0.1f is 0.100000001490116...
    x = rule_actions(np.array((0.1, 0.0), np.float32), np.array([0.0]))
    assert x[0] == np.float32(np.float64(np.float32(0.1)))
    # many rules at once: (n_rules,) + the prices' shape
    many = rule_actions(np.array([(4, 0), (0, 1)], np.float32), np.array([[1.0, 0.875], [1.25, 1.0]]))
    assert many.shape == (2, 2, 2) and many[0].tolist() == [[0.0, 0.5], [-1.0, 0.0]] and (many[1] == 1.0).all()


def test_fixture_shapes_and_the_rules_it_was_played_with(golden):
    from goldsrl.baselines import DEFAULT_TRADE_RULES
    g = golden("trade_rules")
    assert g["rules"].tobytes() == DEFAULT_TRADE_RULES.tobytes()
    assert g["dep_rules"].tolist() == [[0, 1], [0, 0.5], [5, 0], [0, 0]]
    for n in (2, 3, 16):
        pre = "n%d_" % n
        assert g[pre + "normals"].shape == (256, n) and g[pre + "normals"].dtype == np.float32
        assert g[pre + "rewards"].shape == (9, 256) and g[pre + "assets"].shape == (9, 256)
        assert np.array_equal(g[pre + "total"], g[pre + "rewards"].sum(axis=1))
        assert (g[pre + "rewards"][0] == 0).all() and int(g[pre + "best_index"]) == int(np.argmax(g[pre + "total"]))
    assert g["dep_n2_length"].tolist() == [3, 8, 8, 16] and g["dep_n3_length"].tolist() == [5, 7, 7, 16]


def test_baseline_flag_needs_the_device_monitor(capsys):
    from goldsrl.scripts import train_trade
    with pytest.raises(SystemExit) as e:
        train_trade.parse_args(["--baseline"])
    assert e.value.code == 2 and "--eval-every" in capsys.readouterr().err
    assert train_trade.parse_args(["--baseline", "--eval-every", "1", "--eval-envs", "4"]).baseline is True
    assert train_trade.parse_args([]).baseline is False
