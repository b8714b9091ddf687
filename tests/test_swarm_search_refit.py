"""CPU: the numpy statements of the Swarm rule search's scheme (goldsrl/_ffi_swarmsearch.py:swarm_search_candidates,
swarm_search_refit; include/goldsrl_swarmsearch.h), device-free: the refit against np.mean / np.std, the order against np.lexsort
on ties, the offsets against swarm_rule_offsets, and the fixture of the unmodified reference env (tests/golden/swarm_search.npz)
reproduced byte for byte from its own fit and candidates."""
import numpy as np


def _box():
    from goldsrl import _ffi_swarmsearch as S
    return (np.array(v, np.float64) for v in (S.DEFAULT_SPREAD, S.DEFAULT_FLOOR, S.DEFAULT_LO, S.DEFAULT_HI))


def test_refit_is_mean_and_std_of_the_elites():
    from goldsrl import _ffi_swarmsearch as S
    rng = np.random.default_rng(3)
    for C, K in ((2, 1), (5, 2), (5, 5), (70, 8), (1024, 8)):
        # numbers of one sign and a spread of their own size: neither the mean nor the deviations from it cancel, so 1e-15
        # relative (4.5 ulp) covers the at most K - 1 = 7 roundings of half an ulp by which two orders of summation can differ
        cand = rng.random((C, 6)) * 2
        fit = -rng.random(C) * 100
        order, mean, std = S.swarm_search_refit(fit, cand, K, np.zeros(5))
        assert order.dtype == np.int32 and sorted(order.tolist()) == list(range(C)) and (np.diff(fit[order]) <= 0).all()
        el = cand[order[:K]][:, list(S.SEARCH_COLS)]
        np.testing.assert_allclose(mean, el.mean(0), rtol=1e-15, atol=0)
        np.testing.assert_allclose(std, el.std(0), rtol=1e-15, atol=0)
        # the floor holds a parameter's spread up, and a zero floor with equal elites leaves zero
        floor = np.array([0, 100.0, 0, 0, 1e-3])
        _, _, floored = S.swarm_search_refit(fit, cand, K, floor)
        assert floored[1] == 100.0 and np.array_equal(floored[[0, 2, 3]], std[[0, 2, 3]]) and floored[4] == max(std[4], 1e-3)
    # equal elites of few bits (their K-fold sums are exact) are their own mean; 0.7 is not such a number: 3 * 0.7 rounds
    same = np.tile(np.array([(1.0, 5.0, 0.0, -1.5, 1.5, 0.75)]), (6, 1))
    for K in (1, 2, 3, 6):
        order, mean, std = S.swarm_search_refit(np.zeros(6), same, K, np.zeros(5))
        assert order.tolist() == list(range(6)) and mean.tobytes() == same[0, list(S.SEARCH_COLS)].tobytes() and not std.any()
    same[:, 5] = 0.7
    for K, kept in ((1, True), (2, True), (3, False)):
        _, mean, std = S.swarm_search_refit(np.zeros(6), same, K, np.zeros(5))
        assert (mean[4] == 0.7) == kept and (std[4] == 0.0) == kept and abs(mean[4] - 0.7) < 2e-16 and std[4] < 2e-16


def test_order_on_ties_is_lexsort():
    from goldsrl import _ffi_swarmsearch as S
    rng = np.random.default_rng(5)
    for C in (2, 7, 64, 200):
        fit = -np.round(rng.random(C) * 4)                                   # five distinct values: many ties
        order, _, _ = S.swarm_search_refit(fit, np.zeros((C, 6)), 1, np.zeros(5))
        assert np.array_equal(order, np.lexsort((np.arange(C), -fit)))
    order, _, _ = S.swarm_search_refit(np.array([-3.0, -1.0, -3.0, -1.0, -2.0]), np.zeros((5, 6)), 2, np.zeros(5))
    assert order.tolist() == [1, 3, 4, 0, 2]


def test_candidates_rows_clamp_and_offsets():
    from goldsrl import _ffi_swarmsearch as S, _ffi_swarmrules as R
    spread, floor, lo, hi = _box()
    rng = np.random.default_rng(9)
    z = rng.standard_normal((40, 5)) * 4                                     # wide: some candidates leave the box
    mean = np.array([1.0, 5.0, -1.5, 1.5, 0.7])
    inc = np.array([1.0, 7.0, 1.0, -1.0, 1.0, 0.3])
    for anchor in (0.0, 1.0):
        inc[2] = anchor
        cand, off = S.swarm_search_candidates(mean, spread, z, lo, hi, anchor, inc)
        assert cand.shape == (40, 6) and off.shape == (40, 10, 2) and cand.dtype == off.dtype == np.float64
        assert cand[0].tobytes() == inc.tobytes() and (cand[:, 2] == anchor).all() and (cand[:, 0] == 1.0).all()
        five = cand[:, list(S.SEARCH_COLS)]
        assert (five >= lo).all() and (five <= hi).all() and (five[1:] == lo).any() and (five[1:] == hi).any()
        inside = np.abs(z[1:, 1]) < 2
        assert np.array_equal(five[1:, 1][inside], (mean[1] + spread[1] * z[1:, 1])[inside])
        assert off.tobytes() == R.swarm_rule_offsets(cand).tobytes()
    assert S.swarm_search_start([2.0, -1.0, 5.0, 0.5, 9.0], lo, hi).tolist() == [1.0, 0.0, 4.0, 0.5, 3.0]


def test_the_fixture_is_reproduced_byte_for_byte(golden):
    """numpy against numpy: fed the fixture's fit and candidates, the two functions give the fixture's order, mean, std and the
    next generation's candidates.  It pins the scheme without a device."""
    from goldsrl import _ffi_swarmsearch as S
    g = golden("swarm_search")
    spread, floor, lo, hi = _box()
    Gn, C, K = (int(v) for v in g["shape"])
    assert g["normals"].tobytes() == np.random.default_rng(0).standard_normal((Gn, C, 5)).tobytes()
    start = g["start"]
    assert g["mean"][0].tobytes() == S.swarm_search_start(start[list(S.SEARCH_COLS)], lo, hi).tobytes() and g["std"][0].tobytes() == spread.tobytes()
    incumbent = start.copy()
    for gen in range(Gn):
        cand, _ = S.swarm_search_candidates(g["mean"][gen], g["std"][gen], g["normals"][gen], lo, hi, start[2], incumbent)
        assert cand.tobytes() == g["candidates"][gen].tobytes(), gen
        order, mean, std = S.swarm_search_refit(g["fit"][gen], g["candidates"][gen], K, floor)
        assert order.tobytes() == g["order"][gen].tobytes() and mean.tobytes() == g["mean"][gen + 1].tobytes(), gen
        assert std.tobytes() == g["std"][gen + 1].tobytes(), gen
        incumbent = cand[order[0]]
    assert (g["gaps"] >= 1e-6).all()
    assert g["fit"][Gn - 1, g["order"][Gn - 1, 0]] - float(g["best_fixed_total"]) > 3
