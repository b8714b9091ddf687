"""CPU: the foresight recurrence of include/goldsrl_tickerforesight.h.  The plain-loop oracle (tests/_ticker_foresight_oracle.py, played
through oracle/ticker.py) against a brute force over every action sequence, against the twelve golden rules, and against the fixture
of the unmodified reference env (tests/golden/gen_golden_ticker_foresight.py); the numpy form of goldsrl/_ffi_tickerforesight.py
against the loop; and what the Python layers refuse without a device."""
import numpy as np
import pytest

import _ticker_foresight_oracle as FO
from oracle import ticker as TK

HORIZONS = (0, 1, 2, 4, 16, 64)


def _four_row_table(seed):
    """4 rows traded at, 2 % moves of two independent prices, and the row the env shows after the last step"""
    rng = np.random.RandomState(seed)
    p = 100.0 * np.exp(np.cumsum(rng.normal(0, 0.02, size=(4, 2)), axis=0))
    m = np.zeros((5, 4))
    m[:4, :2] = p
    m[4, :2] = p[3]
    return m


@pytest.mark.parametrize("seed", [11, 12])
def test_recurrence_is_the_best_of_all_sequences(seed):
    """The oracle's own sequence is one of the 65 536 (a buy or a sale of everything, or hold, per asset), so the brute force cannot end
    below it; it ends above it by rounding at most: 4 steps of about ten float64 roundings each, 1e-13 relative with room."""
    m = _four_row_table(seed)
    acts, _, assets, bound = FO.play(m, 0, 0, 4)
    best, seq = FO.brute_force(m, 4)
    assert (acts[:, :2] != 0).any(), "the table of seed %d trades nowhere" % seed
    assert not ((acts[:, 0] == 1) & (acts[:, 2] == 0)).any()
    assert best >= assets[-1]
    assert best <= assets[-1] * (1 + 1e-13), (best, assets[-1], seq, acts)
    assert abs(np.log(assets[-1] + 1e-4) - np.log(10.0 + 1e-4) - bound) <= 1e-13
    for c0, c1 in acts[:, :2]:                                             # never a buy and a sale of the same asset: one choice each
        assert c0 in (0, 1, 2) and c1 in (0, 1, 2) and not (c0 == 1 and c1 == 1)


def test_a_horizon_past_the_episode_is_the_whole_episode(golden):
    m = golden("ticker_rules")["matrix"]
    win = m[123:123 + 1024]
    whole = FO.plan(0, win, 5, 68)
    assert np.array_equal(FO.plan(1023, win, 5, 68), whole) and np.array_equal(FO.plan(63, win, 5, 68), whole)
    assert not np.array_equal(FO.plan(4, win, 5, 68), whole)
    assert np.array_equal(FO.plan(0, win, 5, 68)[0], FO.action(0, win, 5, 68))


def test_whole_episode_foresight_beats_every_golden_rule(golden):
    g = golden("ticker_rules")
    m, starts = g["matrix"], g["starts"]
    assert g["assets"].shape == (3, 12, 256)
    for s, st in enumerate(starts):
        _, rewards, assets, bound = FO.play(m, int(st), 0, 256)
        assert (assets[-1] >= g["assets"][s, :, -1] * (1 - 1e-12)).all(), (s, assets[-1], g["assets"][s, :, -1])
        assert bound >= g["total"][s].max() and abs(rewards.sum() - bound) <= 1e-12


def test_oracle_on_the_oracle_env_reproduces_the_reference_fixture(golden):
    g, f = golden("ticker_rules"), golden("ticker_foresight")
    m = g["matrix"]
    assert np.array_equal(f["starts"], g["starts"]) and f["horizons"].tolist() == [0, 4]
    for s, st in enumerate(f["starts"]):
        for k, H in enumerate(f["horizons"]):
            acts, rewards, assets, bound = FO.play(m, int(st), int(H), 256)
            assert np.array_equal(acts, f["actions"][s, k])
            assert np.abs(rewards - f["rewards"][s, k]).max() <= 1e-12 and np.abs(assets - f["assets"][s, k]).max() <= 1e-12
        assert abs(bound - f["bound"][s]) <= 1e-12
    tot = f["rewards"].sum(axis=2)
    assert (tot[:, 0] > tot[:, 1]).all() and (np.abs(tot[:, 0] - f["bound"]) <= 1e-12).all()


def test_numpy_form_is_the_loop_exactly(golden):
    from goldsrl._ffi_tickerforesight import (ticker_foresight_actions, ticker_foresight_bound, ticker_foresight_coefficients,
                                              ticker_foresight_last)
    m = golden("ticker_rules")["matrix"]
    start = np.array([0, 123, 376, 200, 376, 50, 7])
    idx = np.array([0, 10, 1000, 1022, 1023, 300, 990])
    last = ticker_foresight_last(48, 0, np.zeros(7, np.int64), idx)
    assert last.tolist() == [47, 57, 1022, 1022, 1022, 347, 1022]
    assert ticker_foresight_last(48, 20, np.array([0, 5, 19, 20, 25, 0, 0]), idx).tolist() == [19, 24, 1000, 1022, 1022, 319, 1009]
    cash, qty = np.linspace(1, 7, 7), np.arange(14, dtype=np.float64).reshape(7, 2) / 100
    for H in HORIZONS + (1023,):
        A, B0, B1, code = ticker_foresight_coefficients(H, m, start, idx, last)
        acts = ticker_foresight_actions(H, cash, qty, m, start, idx, last)
        assert acts.dtype == np.float32 and acts.shape == (7, 4)
        for i in range(7):
            win = m[start[i]:start[i] + 1024]
            if last[i] < idx[i]:
                assert acts[i].tolist() == [0, 0, 0, 0] and (A[i], B0[i], B1[i]) == (1.0, win[idx[i]][0], win[idx[i]][1])
                continue
            e = last[i] if H == 0 else min(idx[i] + H, last[i])
            want = FO.coefficients(win, int(idx[i]), int(e))
            assert (A[i], B0[i], B1[i], code[i] & 3, code[i] >> 2) == want, (H, i)
            assert np.array_equal(acts[i], FO.action(H, win, int(idx[i]), int(last[i])))
    assets = cash + (qty * m[start + idx][:, :2]).sum(axis=1)
    bound = ticker_foresight_bound(cash, qty, assets, m, start, idx, last)
    for i in (0, 1, 5):
        st = {"cash": cash[i:i + 1], "assets": assets[i:i + 1], "qty": qty[i:i + 1], "idx": idx[i:i + 1], "start": start[i:i + 1]}
        assert FO.play(m, None, 0, 48, state=st)[3] == bound[i]
    assert bound[4] == np.log(assets[4] + 1e-4) - np.log(assets[4] + 1e-4) == 0      # no step left: marked where it stands
    with pytest.raises(ValueError):
        ticker_foresight_actions(0, cash[:3], qty, m, start, idx, last)


class _Engine(object):
    """what TickerForesightCeiling asks of an engine before it touches the device"""

    def __init__(self, kind, cap=1023):
        self.kind = kind
        self.cfg = type("cfg", (), {"max_episode_steps": cap})()


def test_layers_refuse_without_a_device(capsys):
    from goldsrl import _ffi
    from goldsrl._ffi_tickerforesight import check_ticker_horizons, ticker_foresight
    from goldsrl.baselines import DEFAULT_TICKER_HORIZONS, TickerForesightCeiling
    from goldsrl.scripts import train_ticker
    assert DEFAULT_TICKER_HORIZONS == (1, 2, 4, 16, 64, 0)
    assert check_ticker_horizons(DEFAULT_TICKER_HORIZONS).dtype == np.int32
    for bad, word in (([], "horizons must be"), (list(range(65)), "horizons must be"), ([[1, 2]], "horizons must be"),
                      ([1, -1], "horizon 1 is not"), ([1024], "horizon 0 is not"), ([0, 2, 1.5], "horizon 2 is not")):
        with pytest.raises(ValueError, match=word):
            check_ticker_horizons(bad)
    for kind in (_ffi.ENV_SWARM, _ffi.ENV_SOLOW, _ffi.ENV_TRADE):
        with pytest.raises(ValueError, match="Ticker env only"):
            TickerForesightCeiling(_Engine(kind))
        with pytest.raises(ValueError, match="not a Ticker engine"):
            ticker_foresight(_Engine(kind), [0])
    c = TickerForesightCeiling(_Engine(_ffi.ENV_TICKER))
    assert c.horizons.tolist() == [1, 2, 4, 16, 64, 0] and c.max_episode_steps == 1023
    with pytest.raises(ValueError, match="max_episode_steps"):
        TickerForesightCeiling(_Engine(_ffi.ENV_TICKER, cap=0))
    with pytest.raises(ValueError, match="horizon 0"):
        TickerForesightCeiling(_Engine(_ffi.ENV_TICKER), [1, 2]).ceiling()          # no whole-episode column, no ceiling
    with pytest.raises(SystemExit) as e:
        train_ticker.parse_args(["--table", "t.npz", "--ceiling"])
    assert e.value.code == 2 and "--eval-envs" in capsys.readouterr().err
    assert train_ticker.parse_args(["--table", "t.npz", "--ceiling", "--eval-envs", "4"]).ceiling is True
    assert train_ticker.parse_args(["--table", "t.npz"]).ceiling is False
