"""CPU: the numpy statements of the TradeAR1 rule search (goldsrl/_ffi_tradesearch.py; the scheme: include/goldsrl_tradesearch.h),
device-free.  The four-number rule must be the sweep's (gain, bias) rule bit for bit on the sub-family gain_buy == gain_sell,
ref == 1, take gain_sell at p == ref and clip at +-1; a row is the float32 cast and nothing more; candidate 0 is the clamped start,
then the incumbent's bits; a parameter with zero spread and zero floor never moves."""
import numpy as np
import pytest


def test_the_symmetric_sub_family_is_the_sweeps_rule_bit_for_bit():
    from goldsrl._ffi_tradesearch import trade_rule4_actions
    from goldsrl._ffi_tradesweep import rule_actions
    from goldsrl.baselines import DEFAULT_TRADE_RULES
    rng = np.random.default_rng(0)
    two = np.concatenate([DEFAULT_TRADE_RULES, np.stack([rng.uniform(0, 300, 500), rng.uniform(-1, 1, 500)], axis=1).astype(np.float32),
                          np.array([(1000, 0.3), (5000, 0), (-3, 0.5)], np.float32)])
    four = np.stack([two[:, 0], two[:, 0], two[:, 1], np.ones(len(two), np.float32)], axis=1)
    prices = np.concatenate([np.exp(rng.normal(0, 0.05, (40, 16))).ravel(), [1.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2), 0.5, 2.0]])
    got, want = trade_rule4_actions(four, prices), rule_actions(two, prices)
    assert got.dtype == np.float32 and got.shape == (len(two), len(prices)) and got.tobytes() == want.tobytes()
    assert len(np.unique(got)) > 1000 and (got == 1).any() and (got == -1).any()
    assert trade_rule4_actions(four[7], prices.reshape(5, -1)).tobytes() == rule_actions(two[7], prices.reshape(5, -1)).tobytes()   # one rule


def test_the_side_is_chosen_by_the_sign_of_p_minus_ref_and_zero_sells():
    from goldsrl._ffi_tradesearch import trade_rule4_actions
    ref = np.float32(0.987)
    rule = np.array((220, 8.5, -0.25, ref), np.float32)
    below, above = np.nextafter(np.float64(ref), 0), np.nextafter(np.float64(ref), 2)
    a = trade_rule4_actions(rule, np.array([0.985, below, np.float64(ref), above, 1.0]))
    assert a[0] == np.float32(-0.25 - 220.0 * (0.985 - np.float64(ref))) and a[4] == np.float32(-0.25 - 8.5 * (1.0 - np.float64(ref)))
    assert a[1] == np.float32(-0.25 - 220.0 * (below - np.float64(ref))) and a[3] == np.float32(-0.25 - 8.5 * (above - np.float64(ref)))
    assert a[2] == np.float32(-0.25)
    # at d == 0 the product is a zero whose sign is the gain's: bias -0.0 minus +0.0 (gain_sell > 0) stays -0.0, minus -0.0 would be +0.0
    z = trade_rule4_actions(np.array((-1, 1, -0.0, 1), np.float32), np.array([1.0]))
    assert z[0] == 0 and np.signbit(z[0])
    z = trade_rule4_actions(np.array((1, -1, -0.0, 1), np.float32), np.array([1.0]))
    assert z[0] == 0 and not np.signbit(z[0])


def test_the_clip_edges():
    from goldsrl._ffi_tradesearch import trade_rule4_actions
    rule = np.array((64, 8, 0, 1), np.float32)                              # the products at 1 - 1/64 and 1 + 1/8 are exactly -1 and 1
    p = np.array([0.984375, np.nextafter(0.984375, 0), 0.99, 1.125, np.nextafter(1.125, 2), 1.0625, 0.5, 3.0])
    a = trade_rule4_actions(rule, p)
    want = np.clip(-np.where(p < 1, 64.0, 8.0) * (p - 1.0), -1, 1).astype(np.float32)
    assert a.tobytes() == want.tobytes()
    assert a[0] == 1 and a[1] == 1 and a[6] == 1 and a[3] == -1 and a[4] == -1 and a[7] == -1 and a[5] == -0.5 and 0 < a[2] < 1
    assert (np.abs(trade_rule4_actions(np.array((3e38, 3e38, 1, 1), np.float32), p)) <= 1).all()        # float32's largest gains stay actions
    for bad in ((1, 2, 3), np.zeros((2, 3)), np.zeros((1, 2, 4))):
        with pytest.raises(ValueError):
            trade_rule4_actions(bad, p)


def test_rows_candidates_and_the_incumbent():
    from goldsrl import _ffi_tradesearch as S
    start = np.array((100, 100, 0, 1), np.float32)
    spread, floor, lo, hi = S.trade_search_defaults(start)
    mean = S.trade_search_start(start, lo, hi)
    assert mean.tolist() == [100, 100, 0, 1] and mean.dtype == np.float64
    assert S.trade_search_start((-5, 20000, 2, 0.5), lo, hi).tolist() == [0, 10000, 1, 0.8]             # clamped into the box
    z = np.random.default_rng(3).standard_normal((64, 4))
    z[5] = (1000, -1000, 1000, -1000)                                           # far outside: the box's corners
    rows = S.trade_search_candidates(mean, spread, z, lo, hi)
    assert rows.dtype == np.float32 and rows.shape == (64, 4) and rows[0].tobytes() == start.tobytes()
    v = np.minimum(np.maximum(mean[None] + spread[None] * z, lo[None]), hi[None])
    assert rows[1:].tobytes() == v[1:].astype(np.float32).tobytes()         # statement 3 is the cast, nothing more
    assert rows[5].tolist() == [10000, 0, 1, np.float32(0.8)] and len(np.unique(rows[:, 3])) > 50
    assert S.trade_search_rows(np.array([0.1, 1e-50, -0.3, 1 + 2.0 ** -30])).tobytes() == np.array([0.1, 0, -0.3, 1], np.float32).tobytes()
    inc = np.array((220, 8.5, -0.87, 0.987), np.float32)
    again = S.trade_search_candidates(mean, spread, z, lo, hi, inc)
    assert again[0].tobytes() == inc.tobytes() and again[1:].tobytes() == rows[1:].tobytes()
    off = S.trade_search_candidates(S.trade_search_start((100, 100, 0, 2), lo, hi), spread, z, lo, hi)  # a start outside the box: clamped
    assert off[0].tolist() == [100, 100, 0, 1.25]


def test_a_parameter_with_zero_spread_and_floor_never_moves():
    from goldsrl import _ffi_tradesearch as S
    start = np.array((100, 100, 0.1, 0.987), np.float32)
    spread, floor, lo, hi = S.trade_search_defaults(start)
    spread[3] = floor[3] = 0.0
    spread[2] = floor[2] = 0.0
    rng = np.random.default_rng(5)
    mean, std, incumbent = S.trade_search_start(start, lo, hi), spread, None
    for g in range(6):
        rows = S.trade_search_candidates(mean, std, rng.standard_normal((9, 4)), lo, hi, incumbent)
        assert (rows[:, 3] == start[3]).all() and (rows[:, 2] == start[2]).all() and len(np.unique(rows[:, 0])) >= 8
        order, mean, std = S.trade_search_refit(rng.standard_normal(9), rows, 4, floor)
        assert mean[3] == np.float64(start[3]) and std[3] == 0 and mean[2] == np.float64(start[2]) and std[2] == 0
        assert (std[:2] >= floor[:2]).all() and (std[:2] > 0).all()
        incumbent = rows[order[0]].copy()
    # the refit's chains in rank order, and the floor
    rows = np.array([(0, 1, 0, 1), (2, 1, 0.5, 1), (4, 1, 1, 1)], np.float32)
    order, mean, std = S.trade_search_refit(np.array([1.0, 3.0, 2.0]), rows, 2, np.array([0, 0.5, 0, 0]))
    assert order.tolist() == [1, 2, 0] and order.dtype == np.int32 and mean.tolist() == [3, 1, 0.75, 1] and std.tolist() == [1, 0.5, 0.25, 0]
    assert S.trade_search_rank([1.0, 2.0, 2.0, 0.5]).tolist() == [1, 2, 0, 3]


def test_the_defaults():
    from goldsrl import _ffi_tradesearch as S
    spread, floor, lo, hi = S.trade_search_defaults((100, 100, 0, 1))
    assert spread.tolist() == [50, 50, 0.25, 0.02] and floor.tolist() == (spread / 20).tolist()
    assert lo.tolist() == [0, 0, -1, 0.8] and hi.tolist() == [10000, 10000, 1, 1.25]
    assert S.trade_search_defaults((0, 1, 0, 1))[0].tolist() == [1, 1, 0.25, 0.02]                      # a gain's spread is at least 1
    assert S.trade_search_defaults((220, 8.5, -0.87, 0.987))[0][:2].tolist() == [110, 4.25]
    for v in S.trade_search_defaults((5, 5, 1, 1)):
        assert v.dtype == np.float64 and v.shape == (4,)
    assert S.RULE4_FIELDS == ("gain_buy", "gain_sell", "bias", "ref") and S.OUTPUTS == ("candidates", "scores", "fit", "order", "mean", "std")


def test_argument_errors():
    from goldsrl import _ffi, _ffi_tradesearch as S

    class Cfg(object):
        max_episode_steps, n_assets, flags = 0, 2, 0

    class Trade(object):                              # as far as the checks look: they come before the library is loaded
        kind, E, cfg = _ffi.ENV_TRADE, 3, Cfg()
    eng, ok = Trade(), dict(generations=2, candidates=4, elites=2, max_steps=4)
    for start in ((1, 2, 3), (1, 2, 3, np.nan), (np.inf, 1, 0, 1), np.zeros((2, 4))):
        with pytest.raises(ValueError, match="4 finite numbers"):
            S.trade_search(eng, start, **ok)
    for counts in (dict(generations=0), dict(candidates=1), dict(candidates=1025), dict(elites=0), dict(elites=5)):
        with pytest.raises(ValueError, match="generations >= 1"):
            S.trade_search(eng, (100, 100, 0, 1), **dict(ok, **counts))
    for box in (dict(spread=(1, 1, 1)), dict(floor=(0, 0, 0, np.nan)), dict(lo=np.zeros((2, 4)))):
        with pytest.raises(ValueError, match="4 finite numbers over"):
            S.trade_search(eng, (100, 100, 0, 1), **dict(ok, **box))
    for box in (dict(spread=(1, 1, -1, 1)), dict(floor=(0, -1, 0, 0)), dict(lo=(0, 0, 0, 2), hi=(1, 1, 1, 1))):
        with pytest.raises(ValueError, match="spread >= 0, floor >= 0 and lo <= hi"):
            S.trade_search(eng, (100, 100, 0, 1), **dict(ok, **box))
    with pytest.raises(ValueError, match="finite as float32"):
        S.trade_search(eng, (100, 100, 0, 1), hi=(1e39, 1e4, 1, 1.25), **ok)
    with pytest.raises(ValueError, match="finite as float32"):
        S.trade_search(eng, (100, 100, 0, 1), lo=(-1e39, 0, -1, 0.8), **ok)
    with pytest.raises(ValueError, match="normals must be"):
        S.trade_search(eng, (100, 100, 0, 1), normals=np.zeros((2, 4, 3)), **ok)
    with pytest.raises(ValueError, match="max_steps must be at least 1"):
        S.trade_search(eng, (100, 100, 0, 1), generations=2, candidates=4, elites=2)                    # no TimeLimit, no default
    with pytest.raises(ValueError, match=r"tape must be \(max_steps, E, n_assets\)"):
        S.trade_search(eng, (100, 100, 0, 1), tape=np.zeros((4, 2, 3)), **ok)
    with pytest.raises(ValueError, match="F_INJECT_NOISE and a tape"):
        S.trade_search_host(eng, (100, 100, 0, 1), **ok)
    with pytest.raises(ValueError, match="4 finite numbers"):
        S.trade_search_play(eng, (1, 2, 3), 4)


@pytest.mark.parametrize("n", [2, 16])
def test_the_fixtures_leading_fits_lie_further_apart_than_twice_the_bound(golden, n):
    """tests/golden/trade_search.npz: what the GPU test's exact comparison of tables and elite orders rests on, re-asserted on the
    committed file (the generator asserts it where the reference env is at hand): in every generation any two fits among ranks
    0..K differ by more than twice 1e-5 * max(1, |fit|) + steps * 1e-9; and the recorded tables, orders, means and stds are the
    numpy statements applied to the recorded fits."""
    from goldsrl import _ffi_tradesearch as S
    g, pre = golden("trade_search"), "n%d_" % n
    G, C, K = (int(v) for v in g["shape"])
    T = int(g["steps"])
    fit, order, cand, z = g[pre + "fit"], g[pre + "order"], g[pre + "candidates"], g[pre + "normals"]
    assert fit.shape == (G, C) and cand.shape == (G, C, 4) and g[pre + "tape"].shape == (T, 3, n) and g[pre + "tape"].dtype == np.float32
    spread, floor, lo, hi = (g[pre + k] for k in ("spread", "floor", "lo", "hi"))
    for v, want in zip((spread, floor, lo, hi), S.trade_search_defaults(g["start"])):
        assert v.tobytes() == want.tobytes()
    assert g[pre + "mean"][0].tobytes() == S.trade_search_start(g["start"], lo, hi).tobytes() and g[pre + "std"][0].tobytes() == spread.tobytes()
    incumbent = None
    for gen in range(G):
        lead = fit[gen][order[gen][:K + 1]]
        assert (np.diff(lead) < 0).all()
        for i in range(K + 1):
            for j in range(i + 1, K + 1):
                bound = max(1e-5 * max(1.0, abs(lead[i])) + T * 1e-9, 1e-5 * max(1.0, abs(lead[j])) + T * 1e-9)
                assert abs(lead[i] - lead[j]) > 2 * bound, (gen, i, j, lead[i], lead[j])
        assert S.trade_search_candidates(g[pre + "mean"][gen], g[pre + "std"][gen], z[gen], lo, hi, incumbent).tobytes() == cand[gen].tobytes()
        o, mean, std = S.trade_search_refit(fit[gen], cand[gen], K, floor)
        assert o.tobytes() == order[gen].tobytes() and mean.tobytes() == g[pre + "mean"][gen + 1].tobytes()
        assert std.tobytes() == g[pre + "std"][gen + 1].tobytes()
        incumbent = cand[gen][order[gen][0]].copy()
