"""CPU: the selection rules and the moments of the constant-savings baseline (goldsrl/baselines.py, goldsrl/_ffi_sweep.py) on the
fixture of the unmodified reference script (tests/golden/gen_golden_constant_solow.py), and the --baseline flag's parser check."""
import numpy as np
import pytest

ORDERS = (1, 2, 3)
# scripts/constant_solow.py as printed by the unmodified reference: the best rate is index 6 of the 20 for all three orders
PRINTED_S_MAX = 0.33421052631578946
PRINTED_MEAN = {1: 0.8584489383443, 2: 0.8209713522371522, 3: 0.8049613896384379}


def test_fixture_is_the_printed_lines(golden):
    g = golden("constant_solow")
    assert np.array_equal(g["rates"], np.linspace(0.05, 0.95, 20)) and list(g["traced"]) == [0, 6, 19]
    for p in ORDERS:
        pre = "p%d_" % p
        assert g[pre + "printed"][0] == PRINTED_S_MAX and g[pre + "printed"][1] == PRINTED_MEAN[p]
        assert int(g[pre + "best_index"]) == 6
        assert g[pre + "z0"].shape == (p,) and g[pre + "tape_tail"].shape == (1024,) and g[pre + "rewards"].shape == (3, 1024)


@pytest.mark.parametrize("p", ORDERS)
def test_best_gives_the_scripts_line(golden, p):
    from goldsrl.baselines import select_best
    g, pre = golden("constant_solow"), "p%d_" % p
    s_max, max_mean, stats = select_best(g["rates"], g[pre + "mean"], g[pre + "max"], g[pre + "min"], g[pre + "std"])
    assert [s_max, max_mean] + list(stats) == list(g[pre + "printed"])
    assert s_max == g["rates"][6]


def test_best_through_the_class_without_a_device(golden):
    """best() and best_total() are pure functions of the statistics: a baseline object holding them needs no engine."""
    from goldsrl.baselines import ConstantSavingsBaseline
    g = golden("constant_solow")
    b = ConstantSavingsBaseline.__new__(ConstantSavingsBaseline)
    b.rates = g["rates"]
    b.stats = {k: g["p1_" + k][:, None] for k in ("mean", "max", "min", "std", "total")}
    s_max, max_mean, stats = b.best(0)
    assert [s_max, max_mean] + list(stats) == list(g["p1_printed"])
    rate, total = b.best_total()
    assert rate == g["rates"][6] and total == g["p1_total"][6] and total == g["p1_total"].max()


def test_strictly_greater_rule_on_a_tie():
    from goldsrl.baselines import select_best, select_best_total
    rates = np.array([0.1, 0.2, 0.3, 0.4])
    mean = np.array([0.5, 0.7, 0.7, 0.6])
    mx, mn, std = np.arange(4.0), -np.arange(4.0), 10 + np.arange(4.0)
    assert select_best(rates, mean, mx, mn, std) == (0.2, 0.7, (1.0, -1.0, 11.0))
    # the reference starts from max_mean = 0: no rate with a positive mean, no winner
    assert select_best(rates, -mean, mx, mn, std) == (0, 0, None)
    total = np.array([[1.0, 3.0], [2.0, 4.0], [4.0, 2.0], [0.0, 0.0]])
    assert select_best_total(rates, total) == (0.2, 3.0)


@pytest.mark.parametrize("p", ORDERS)
def test_std_from_the_two_sums(golden, p):
    """std = sqrt(sum_sq / n - mean^2) from sequential float64 sums against np.std of the reward sequences.  rtol 1e-9: float64
    rounding of a two-term difference of O(1) values with a variance >= 0.1 over 1 024 terms, expected error about 1e-13."""
    from goldsrl._ffi_sweep import reward_moments
    g = golden("constant_solow")
    for row, i in enumerate(g["traced"]):
        r = g["p%d_rewards" % p][row]
        total, sum_sq = np.cumsum(r)[-1], np.cumsum(r * r)[-1]
        mean, std = reward_moments(total, sum_sq, r.size)
        assert np.var(r) >= 0.1
        np.testing.assert_allclose(std, np.std(r), rtol=1e-9, atol=0)
        np.testing.assert_allclose(std, g["p%d_std" % p][i], rtol=1e-9, atol=0)
        np.testing.assert_allclose(mean, g["p%d_mean" % p][i], rtol=1e-12, atol=0)


@pytest.mark.parametrize("script", ["train_solow", "train_solow_grid", "train_paac_solow"])
def test_baseline_flag_needs_eval_envs(script, capsys):
    import importlib
    mod = importlib.import_module("goldsrl.scripts." + script)
    with pytest.raises(SystemExit) as e:
        mod.parse_args(["--baseline"])
    assert e.value.code == 2 and "--eval-envs" in capsys.readouterr().err
    assert mod.parse_args(["--baseline", "--eval-envs", "4"]).baseline is True
    assert mod.parse_args([]).baseline is False
