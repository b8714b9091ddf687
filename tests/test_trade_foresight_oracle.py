"""CPU: the foresight recurrence of include/goldsrl_tradeforesight.h.  The plain-loop oracle (tests/_trade_foresight_oracle.py, played
through oracle/oracle.py:trade_step) against a brute force over every action sequence; the fixture of the unmodified reference env
(tests/golden/gen_golden_trade_foresight.py) and the rule fixture against the bound; the numpy form of goldsrl/_ffi_tradeforesight.py
against the loop, bit for bit; and what the Python layers refuse without a device.

The allowance of every bound check is the device test's: length * 2**-24 * max(|min|, |max|) + 1e-10.  The first term is what
float32 step rewards may add (each within half an ulp of its float64 value); the float64 recurrence's own rounding is orders below
the second."""
import numpy as np
import pytest

import _trade_foresight_oracle as FO
from oracle import oracle as O

HORIZONS = (1, 2, 4, 16, 64, 0)


def _allowance(rewards):
    return len(rewards) * 2.0 ** -24 * np.abs(rewards).max() + 1e-10


@pytest.mark.parametrize("n,seed", [(1, 21), (1, 22), (2, 23), (2, 24)])
def test_recurrence_is_the_best_of_all_sequences(n, seed):
    """4 steps, normals scaled by 3 so the decisions are not all holds.  The plan's own sequence is one of the (5 ** n) ** 4, so the
    brute force cannot end below it; it ends above it by rounding at most: 4 steps of a few float64 roundings per asset, 1e-13
    relative with room."""
    normals = 3.0 * np.random.RandomState(seed).normal(size=(4, n))
    path = FO.price_path(normals, O.trade_std_e())[:4]
    acts = FO.plan(0, path, 3)
    assert (acts != 0).any(), "the path of seed %d trades nowhere" % seed
    rewards, assets = FO.play(path, acts[None])
    best, seq = FO.brute_force(path, 4)
    assert best >= assets[0, -1]
    assert best <= assets[0, -1] * (1 + 1e-13), (best, assets[0, -1], seq, acts)
    bound = FO.bound(path, 3, 10.0, np.zeros(n), 10.0)
    assert abs(rewards[0].sum() - bound) <= 1e-13
    assert abs(np.log(best + 1e-4) - np.log(10.0 + 1e-4) - bound) <= 1e-13


def test_a_horizon_past_the_episode_is_the_whole_episode(golden):
    path = golden("trade_foresight")["n3_path"]
    whole = FO.plan(0, path, 63)
    assert np.array_equal(FO.plan(1023, path, 63), whole) and np.array_equal(FO.plan(63, path, 63), whole)
    assert not np.array_equal(FO.plan(2, path, 63), whole)
    assert np.array_equal(whole[0], FO.action(0, path, 0, 63)) and not whole[63].any()       # the last step has nothing to gain


@pytest.mark.parametrize("n", [2, 3, 16])
def test_fixture_of_the_reference_env(golden, n):
    f, g, pre = golden("trade_foresight"), golden("trade_rules"), "n%d_" % n
    assert f["horizons"].tolist() == list(HORIZONS)
    path, bound = f[pre + "path"], float(f[pre + "bound"])
    assert path.shape == (256, n) and (path[0] == 1.0).all()
    assert np.allclose(path, FO.price_path(g[pre + "normals"], O.trade_std_e())[:256], rtol=1e-12, atol=0)
    whole = HORIZONS.index(0)
    for k, H in enumerate(HORIZONS):
        acts, rewards = f[pre + "actions"][k], f[pre + "rewards"][k]
        assert acts.dtype == np.float32 and np.array_equal(acts, FO.plan(H, path, 255))
        played, assets = FO.play(path, acts[None])
        assert np.abs(played[0] - rewards).max() <= 1e-12 and np.abs(assets[0] - f[pre + "assets"][k]).max() <= 1e-11
        assert f[pre + "total"][k] == rewards.sum()
        assert f[pre + "total"][k] <= bound + _allowance(rewards), (H, f[pre + "total"][k], bound)
    assert abs(f[pre + "total"][whole] - bound) <= _allowance(f[pre + "rewards"][whole])
    assert bound == FO.bound(path, 255, 10.0, np.zeros(n), 10.0)
    tot = f[pre + "total"]
    assert tot[0] < tot[1] < tot[2] < tot[3] <= tot[5] + 1e-12 and tot[4] <= tot[5] + 1e-12       # more rows known, no less earned
    # the nine default rules were played on the same normals: none is above the ceiling, the best is far below
    for r in range(9):
        assert g[pre + "total"][r] <= bound + _allowance(g[pre + "rewards"][r]), r
    assert g[pre + "total"].max() < 0.5 * bound


def test_numpy_form_is_the_loop_exactly(golden):
    from goldsrl._ffi_tradeforesight import (trade_foresight_actions, trade_foresight_bound, trade_foresight_coefficients,
                                             trade_foresight_last)
    f = golden("trade_foresight")
    assert trade_foresight_last(48, 0, np.array([0, 5, 90])).tolist() == [47, 47, 47]
    assert trade_foresight_last(48, 20, np.array([0, 5, 19, 20, 25])).tolist() == [19, 14, 0, 0, 0]
    for n in (2, 3, 16):
        path = f["n%d_path" % n]
        # three envs on one fixture path: from row 0, from row 100 and from row 200, with different last steps
        rows = 48
        prices = np.stack([path[0:rows], path[100:100 + rows], path[200:200 + rows]], axis=2)      # (rows, n, 3)
        last = np.array([47, 30, 11])
        for e, l in enumerate(last):
            prices[l + 1:, :, e] = 0.0                                     # as the device writes the rows past an env's m
        for H in HORIZONS + (1023,):
            for t in (0, 1, 7, 11, 12, 30, 31, 47):
                acts = trade_foresight_actions(H, prices, t, last)
                assert acts.dtype == np.float32 and acts.shape == (3, n)
                A, B, dec = trade_foresight_coefficients(H, prices, t, last)
                for e, l in enumerate(last):
                    one = prices[:, :, e]
                    if l < t:
                        assert not acts[e].any() and A[e] == 1.0
                        continue
                    end = l if H == 0 else min(t + H, l)
                    wA, wB, wdec = FO.coefficients(one, t, int(end))
                    assert A[e] == wA and B[:, e].tolist() == wB and dec[:, e].tolist() == wdec, (n, H, t, e)
                    assert np.array_equal(acts[e], FO.action(H, one, t, int(l)))
        assert np.array_equal(trade_foresight_actions(0, prices, 3, 47)[0], trade_foresight_actions(0, prices, 3, last)[0])    # a scalar last
        cash, qty = np.array([10.0, 3.5, 0.0]), np.arange(3 * n, dtype=np.float64).reshape(3, n) / 7
        assets = cash + (qty * prices[0].T).sum(axis=1)
        got = trade_foresight_bound(cash, qty, assets, prices, last)
        for e, l in enumerate(last):
            assert got[e] == FO.bound(prices[:, :, e], int(l), cash[e], qty[e], assets[e])


class _Engine(object):
    """what TradeForesightCeiling asks of an engine before it touches the device"""

    def __init__(self, kind, cap=1024):
        self.kind = kind
        self.cfg = type("cfg", (), {"max_episode_steps": cap, "n_assets": 2})()


def test_layers_refuse_without_a_device(capsys):
    from goldsrl import _ffi
    from goldsrl._ffi_tradeforesight import check_trade_horizons, trade_foresight
    from goldsrl.baselines import DEFAULT_TRADE_HORIZONS, TradeForesightCeiling
    from goldsrl.scripts import train_trade
    assert DEFAULT_TRADE_HORIZONS == (1, 2, 4, 16, 64, 0)
    assert check_trade_horizons(DEFAULT_TRADE_HORIZONS).dtype == np.int32
    for bad, word in (([], "horizons must be"), (list(range(65)), "horizons must be"), ([[1, 2]], "horizons must be"),
                      ([1, -1], "horizon 1 is not"), ([1024], "horizon 0 is not"), ([0, 2, 1.5], "horizon 2 is not")):
        with pytest.raises(ValueError, match=word):
            check_trade_horizons(bad)
    for kind in (_ffi.ENV_SWARM, _ffi.ENV_SOLOW, _ffi.ENV_TICKER):
        with pytest.raises(ValueError, match="TradeAR1 env only"):
            TradeForesightCeiling(_Engine(kind))
        with pytest.raises(ValueError, match="not a TradeAR1 engine"):
            trade_foresight(_Engine(kind), [0])
    c = TradeForesightCeiling(_Engine(_ffi.ENV_TRADE))
    assert c.horizons.tolist() == [1, 2, 4, 16, 64, 0] and c.max_episode_steps == 1024
    with pytest.raises(ValueError, match="max_episode_steps"):
        TradeForesightCeiling(_Engine(_ffi.ENV_TRADE, cap=0))
    with pytest.raises(ValueError, match="horizon 0"):
        TradeForesightCeiling(_Engine(_ffi.ENV_TRADE), [1, 2]).ceiling()          # no whole-episode column, no ceiling
    with pytest.raises(SystemExit) as e:
        train_trade.parse_args(["--ceiling"])
    assert e.value.code == 2 and "--eval-every" in capsys.readouterr().err
    assert train_trade.parse_args(["--ceiling", "--eval-every", "1", "--eval-envs", "4"]).ceiling is True
    assert train_trade.parse_args([]).ceiling is False
