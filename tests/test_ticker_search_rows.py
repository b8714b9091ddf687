"""CPU: the numpy statements of the Ticker rule search (goldsrl/_ffi_tickersearch.py; the scheme: include/goldsrl_tickersearch.h),
device-free.  Statement 3 must turn any six numbers inside the box into a row grl_ticker_sweep accepts -- the sweep's own check,
check_ticker_rules, is the judge --, return a row that already is one bit for bit, and use the second correction exactly where the
first does not suffice; the refit of equal rows returns them; the rank puts a tie to the smaller index."""
import numpy as np
import pytest

HAND = np.float32(0.0027385002)           # (float)(1 - f_a) + f_a is above 1 in float64: the pair needs the step down


def _valid(rows):
    """the sweep's rule check, vectorised: what check_ticker_rules refuses row by row"""
    r = np.asarray(rows)
    assert r.dtype == np.float32
    r64 = r.astype(np.float64)
    ok = np.isfinite(r).all(axis=-1) & (r[..., :4] >= 0).all(axis=-1) & (r[..., :4] <= 1).all(axis=-1)
    ok &= (r64[..., 0] + r64[..., 1] <= 1.0) & (r64[..., 2] + r64[..., 3] <= 1.0) & (r[..., 4] >= 0)
    ok &= (r[..., 5] >= 0) & (r[..., 5] <= 1023) & (r[..., 5] == np.floor(r[..., 5]))
    return ok


def test_every_row_is_a_rule_of_the_sweep():
    from goldsrl._ffi_tickersearch import ticker_search_rows
    from goldsrl._ffi_tickersweep import check_ticker_rules
    rng = np.random.default_rng(0)
    n = 200000
    v = np.concatenate([rng.uniform(0, 1, (n, 4)), rng.uniform(0, 0.5, (n, 1)), rng.uniform(0, 1023, (n, 1))], axis=1)
    v[: n // 4, 1] = 1.0 - v[: n // 4, 0]                                   # float64 sums at 1: the casts decide
    v[n // 4: n // 2, 3] = 1.0 - v[n // 4: n // 2, 2]
    v[n // 2: n // 2 + 1000, :4] = rng.integers(0, 2, (1000, 4))            # the corners
    hand = np.array([[HAND, 1.0, 1.0, HAND, 0.0, 0.5], [HAND, 1.0 - np.float64(HAND), 0.0, 0.0, 0.5, 1022.5]])
    v = np.concatenate([v, hand])
    rows, corrected = ticker_search_rows(v, return_corrected=True)
    assert rows.dtype == np.float32 and rows.shape == v.shape
    bad = np.flatnonzero(~_valid(rows))
    assert len(bad) == 0, (v[bad[:3]], rows[bad[:3]])
    check_ticker_rules(rows[:2000])                                         # the vectorised check above is the sweep's own
    check_ticker_rules(rows[-2:])
    assert (corrected == 1).any() and (corrected == 2).any() and (corrected == 0).any()
    # untouched numbers are the casts
    assert rows[:, 0].tobytes() == v[:, 0].astype(np.float32).tobytes() and rows[:, 2].tobytes() == v[:, 2].astype(np.float32).tobytes()
    assert rows[:, 4].tobytes() == v[:, 4].astype(np.float32).tobytes()
    assert rows[:, 5].tobytes() == np.rint(v[:, 5]).astype(np.float32).tobytes()
    assert rows[-2, 5] == 0.0 and rows[-1, 5] == 1022.0                     # ties to even
    same = corrected == 0
    assert rows[:, 1][same[:, 0]].tobytes() == v[:, 1].astype(np.float32)[same[:, 0]].tobytes()
    assert rows[:, 3][same[:, 1]].tobytes() == v[:, 3].astype(np.float32)[same[:, 1]].tobytes()


def test_the_vectorised_check_is_the_sweeps():
    from goldsrl._ffi_tickersweep import check_ticker_rules
    bad = np.array([(0.6, 0.5, 0, 0, 0, 0), (0, 0, 0.5, 0.6, 0, 0), (1.5, 0, 0, 0, 0, 0), (0, 0, 0, 0, -1, 0), (0, 0, 0, 0, 0, 1.5),
                    (0, 0, 0, 0, 0, 1024), (np.float32(HAND), np.float32(1.0), 0, 0, 0, 0)], np.float32)
    assert not _valid(bad).any()
    for row in bad:
        with pytest.raises(ValueError):
            check_ticker_rules(row[None])


def test_a_valid_row_is_returned_bit_for_bit():
    from goldsrl._ffi_tickersearch import ticker_search_rows
    from goldsrl.baselines import DEFAULT_TICKER_RULES
    rng = np.random.default_rng(1)
    n = 50000
    r = np.concatenate([rng.uniform(0, 1, (n, 4)), rng.uniform(0, 0.5, (n, 1)), rng.integers(0, 1024, (n, 1))], axis=1).astype(np.float32)
    r = np.concatenate([r[_valid(r)], DEFAULT_TICKER_RULES, np.array([(0.5, 0.5, 1, 0, 0, 1023), (HAND, np.nextafter(np.float32(1.0 - np.float64(HAND)), np.float32(0)), 0, 1, 0, 0)], np.float32)])
    assert _valid(r).all() and len(r) > 10000
    rows, corrected = ticker_search_rows(r.astype(np.float64), return_corrected=True)
    assert rows.tobytes() == r.tobytes() and not corrected.any()


def test_the_second_correction_ends_one_float32_below_the_cast():
    from goldsrl._ffi_tickersearch import ticker_search_rows
    rng = np.random.default_rng(2)
    fa = np.concatenate([rng.uniform(0, 1, 100000).astype(np.float32), [HAND]]).astype(np.float32)
    v = np.zeros((len(fa), 6))
    v[:, 0], v[:, 1] = fa, 1.0                                              # the sum is above 1 wherever f_a > 0
    v[:, 2], v[:, 3] = 1.0, fa                                              # f_a = 1: f_b becomes exactly 0
    rows, corrected = ticker_search_rows(v, return_corrected=True)
    cast = (1.0 - fa.astype(np.float64)).astype(np.float32)
    twice = corrected[:, 0] == 2
    assert twice[-1] and 0.1 < twice.mean() < 0.25                          # about one in six
    assert rows[twice, 1].tobytes() == np.nextafter(cast[twice], np.float32(0)).tobytes()
    assert (rows[twice, 1].view(np.uint32) == cast[twice].view(np.uint32) - 1).all()
    once = corrected[:, 0] == 1
    assert rows[once, 1].tobytes() == cast[once].tobytes() and (once | twice | (fa == 0)).all()
    # the step down was needed, and was enough
    assert (fa[twice].astype(np.float64) + cast[twice].astype(np.float64) > 1.0).all()
    assert (rows[:, 0].astype(np.float64) + rows[:, 1].astype(np.float64) <= 1.0).all()
    assert (rows[fa > 0, 3] == 0).all() and (corrected[fa > 0, 1] == 1).all()


def test_candidates_clamp_and_keep_the_incumbent():
    from goldsrl import _ffi_tickersearch as S
    lo, hi = np.array(S.DEFAULT_LO), np.array(S.DEFAULT_HI)
    start = np.array((1, 0, 0, 1, 0.5, 8), np.float32)
    mean = S.ticker_search_start(start, lo, hi)
    assert mean.tolist() == [1, 0, 0, 1, 0.5, 8]
    assert S.ticker_search_start((1, 0, 0, 1, 0.75, 0), lo, hi).tolist() == [1, 0, 0, 1, 0.5, 1]          # clamped into the box
    z = np.random.default_rng(3).standard_normal((64, 6))
    rows = S.ticker_search_candidates(mean, np.array(S.DEFAULT_SPREAD), z, lo, hi)
    assert rows[0].tobytes() == start.tobytes() and _valid(rows).all() and len(np.unique(rows[:, 5])) > 3
    inc = np.array((0.25, 0.5, 0.125, 0.5, 0.0625, 3), np.float32)
    again = S.ticker_search_candidates(mean, np.array(S.DEFAULT_SPREAD), z, lo, hi, inc)
    assert again[0].tobytes() == inc.tobytes() and again[1:].tobytes() == rows[1:].tobytes()
    spread, floor, lo0, hi0 = S.ticker_search_defaults((1, 0, 1, 0, 0.5, 0))                               # L = 0 stays L = 0
    assert spread[5] == floor[5] == lo0[5] == hi0[5] == 0
    assert (S.ticker_search_candidates(S.ticker_search_start((1, 0, 1, 0, 0.5, 0), lo0, hi0), spread, z, lo0, hi0)[:, 5] == 0).all()
    assert S.ticker_search_defaults((1, 0, 0, 1, 0.5, 128))[0][5] == 32 and S.ticker_search_defaults((1, 0, 0, 1, 0.5, 2))[2][5] == 1


def test_the_refit_of_equal_rows_returns_them():
    from goldsrl._ffi_tickersearch import ticker_search_refit
    floor = np.array((0.01, 0.01, 0.01, 0.01, 0.005, 0.5))
    for row in ((0.3, 0.6, 0.6, 0.3, 0.02, 5), (HAND, 0.7, 0.1, 0.9, 0.05, 1023), (1, 0, 0, 1, 0.5, 8)):
        rows = np.tile(np.array(row, np.float32), (7, 1))
        for K in (1, 2, 4, 7):                                              # a float32 widened has 29 spare bits: its K-fold sum is exact
            order, mean, std = ticker_search_refit(np.zeros(7), rows, K, floor)
            assert order.tolist() == list(range(7)) and order.dtype == np.int32
            assert mean.tobytes() == rows[0].astype(np.float64).tobytes() and std.tobytes() == floor.tobytes()
            assert not ticker_search_refit(np.zeros(7), rows, K, np.zeros(6))[2].any()
    # two different elites: the chains in rank order
    rows = np.array([(0, 0, 0, 0, 0, 2), (0.5, 0, 0, 0, 0.25, 4), (1, 0, 0, 0, 0.5, 9)], np.float32)
    order, mean, std = ticker_search_refit(np.array([1.0, 3.0, 2.0]), rows, 2, np.zeros(6))
    assert order.tolist() == [1, 2, 0] and mean.tolist() == [0.75, 0, 0, 0, 0.375, 6.5] and std.tolist() == [0.25, 0, 0, 0, 0.125, 2.5]


def test_the_rank_puts_a_tie_to_the_smaller_index():
    from goldsrl._ffi_tickersearch import ticker_search_rank
    assert ticker_search_rank([1.0, 2.0, 2.0, 0.5, 2.0, 1.0]).tolist() == [1, 2, 4, 0, 5, 3]
    assert ticker_search_rank(np.zeros(5)).tolist() == [0, 1, 2, 3, 4]
    assert ticker_search_rank([0.0, -0.0, 0.0]).tolist() == [0, 1, 2]       # signed zeros tie
    fit = np.random.default_rng(4).integers(0, 4, 200).astype(np.float64)
    order = ticker_search_rank(fit)
    assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(200))
    for a, b in zip(order[:-1], order[1:]):
        assert fit[a] > fit[b] or (fit[a] == fit[b] and a < b)
