"""CPU: the one copy of the cross-entropy searches' numpy statements and argument checks (goldsrl/_search.py), held to numpy and to
both searches' wrappers of it: the rank against np.lexsort on ties, the refit against np.mean / np.std and byte for byte against
swarm_search_refit and ticker_search_refit, the first-operand-wins clamp on signed zeros and on the box's bounds, and every
ValueError text of the three _check_* functions, written out here as the searches raised them before the copy was shared."""
import types

import numpy as np
import pytest

SWARM_FIELDS = "(('cancel', 'gain', 'off_x', 'off_y', 'radius'),)"
TICKER_FIELDS = "(('up0', 'up1', 'dn0', 'dn1', 'band', 'lookback'),)"


def test_rank_on_ties_is_lexsort():
    from goldsrl import _search as S
    rng = np.random.default_rng(5)
    for C in (2, 7, 64, 200):
        fit = -np.round(rng.random(C) * 4)                                   # five distinct values: many ties
        order = S.search_rank(fit)
        assert order.dtype == np.int32 and np.array_equal(order, np.lexsort((np.arange(C), -fit)))
    assert S.search_rank([0.0, -0.0, 0.0]).tolist() == [0, 1, 2]             # signed zeros tie


def test_refit_is_mean_and_std_of_the_elites_and_both_wrappers_bits():
    from goldsrl import _ffi_swarmsearch as W, _ffi_tickersearch as T, _search as S
    rng = np.random.default_rng(3)
    cols = list(W.SEARCH_COLS)
    for C, K in ((2, 1), (5, 2), (5, 5), (70, 8), (1024, 8)):
        # the inputs and the bound of tests/test_swarm_search_refit.py: numbers of one sign and a spread of their own size, so
        # neither the mean nor the deviations cancel, and 1e-15 relative (4.5 ulp) covers the at most K - 1 = 7 roundings of half an
        # ulp by which two orders of summation differ.  A float32 row widened is such a float64 number too.
        cand = rng.random((C, 6)) * 2
        fit = -rng.random(C) * 100
        rows32 = cand.astype(np.float32)
        floor5, floor6 = np.array([0, 100.0, 0, 0, 1e-3]), np.array([0, 100.0, 0, 0, 1e-3, 0])
        for columns, floor, wrapped in ((cand[:, cols], floor5, W.swarm_search_refit(fit, cand, K, floor5)),
                                        (rows32.astype(np.float64), floor6, T.ticker_search_refit(fit, rows32, K, floor6))):
            order, mean, std = S.search_refit(fit, columns, K, np.zeros(columns.shape[1]))
            assert np.array_equal(order, np.lexsort((np.arange(C), -fit)))
            el = columns[order[:K]]
            np.testing.assert_allclose(mean, el.mean(0), rtol=1e-15, atol=0)
            np.testing.assert_allclose(std, el.std(0, ddof=0), rtol=1e-15, atol=0)
            floored = S.search_refit(fit, columns, K, floor)
            assert floored[2][1] == 100.0 and floored[2][4] == max(std[4], 1e-3) and floored[2][0] == std[0]
            for mine, theirs in zip(floored, wrapped):
                assert mine.dtype == theirs.dtype and mine.tobytes() == theirs.tobytes(), (C, K)


def _bits(v):
    return np.asarray(v, np.float64).tobytes()


def test_the_first_operand_wins_a_tie():
    from goldsrl import _search as S
    assert _bits(S.first_max(-0.0, 0.0)) == _bits(-0.0) and _bits(S.first_max(0.0, -0.0)) == _bits(0.0)
    assert _bits(S.first_min(0.0, -0.0)) == _bits(0.0) and _bits(S.first_min(-0.0, 0.0)) == _bits(-0.0)
    assert _bits(S.search_clamp(0.0, -0.0, 1.0)) == _bits(0.0) and _bits(S.search_clamp(-0.0, -1.0, 0.0)) == _bits(-0.0)


def test_a_draw_on_a_bound_is_that_bound():
    from goldsrl import _search as S
    lo, hi = np.array([0.25, -4.0]), np.array([3.0, -0.5])
    mean, std = np.array([1.25, -1.5]), np.array([0.5, 0.25])
    z = np.array([(-2.0, 4.0),                                              # exactly lo[0], exactly hi[1]: every operation is exact
                  (3.5, -10.0),                                             # exactly hi[0], exactly lo[1]
                  (-9.0, 9.0), (9.0, -11.0),                                # past them
                  (1.0, 1.0)])                                              # inside
    v = S.search_draw(mean, std, z, lo, hi)
    assert v.dtype == np.float64 and v.shape == (5, 2)
    assert v[0].tobytes() == np.array([lo[0], hi[1]]).tobytes() and v[1].tobytes() == np.array([hi[0], lo[1]]).tobytes()
    assert v[2].tobytes() == v[0].tobytes() and v[3].tobytes() == v[1].tobytes()
    assert v[4].tolist() == [1.75, -1.25]
    # the shared draw is what both searches' candidates are made of
    from goldsrl import _ffi_swarmsearch as W, _ffi_tickersearch as T
    rng = np.random.default_rng(9)
    z5, z6 = rng.standard_normal((40, 5)) * 4, rng.standard_normal((40, 6)) * 4
    box5 = [np.array(b, np.float64) for b in (W.DEFAULT_SPREAD, W.DEFAULT_LO, W.DEFAULT_HI)]
    m5 = np.array([1.0, 5.0, -1.5, 1.5, 0.7])
    cand, _ = W.swarm_search_candidates(m5, box5[0], z5, box5[1], box5[2], 1.0, np.zeros(6))
    assert cand[1:, list(W.SEARCH_COLS)].tobytes() == S.search_draw(m5, box5[0], z5, box5[1], box5[2])[1:].tobytes()
    box6 = [np.array(b, np.float64) for b in (T.DEFAULT_SPREAD, T.DEFAULT_LO, T.DEFAULT_HI)]
    m6 = np.array([0.5, 0.25, 0.25, 0.5, 0.125, 8.0])
    rows = T.ticker_search_candidates(m6, box6[0], z6, box6[1], box6[2])
    assert rows[1:].tobytes() == T.ticker_search_rows(S.search_draw(m6, box6[0], z6, box6[1], box6[2]))[1:].tobytes()


def _raises(text, fn, *args):
    with pytest.raises(ValueError) as err:
        fn(*args)
    assert str(err.value) == text


def test_the_checks_raise_the_searches_texts():
    from goldsrl import _search as S
    for G, C, K in ((0, 4, 2), (1, 1, 1), (1, 1025, 2), (2, 4, 0), (2, 4, 5)):
        _raises("f: generations >= 1, 2 <= candidates <= 1024 and 1 <= elites <= candidates are required, got %d, %d, %d" % (G, C, K),
                S.check_counts, "f", G, C, K)
    assert S.check_counts("f", 1.0, np.int64(1024), "3") == (1, 1024, 3)
    names = ("spread", "floor", "lo", "hi")
    for fields, text in ((("cancel", "gain", "off_x", "off_y", "radius"), "5 finite numbers over " + SWARM_FIELDS),
                         (("up0", "up1", "dn0", "dn1", "band", "lookback"), "6 finite numbers over " + TICKER_FIELDS)):
        P = len(fields)
        good = [np.zeros(P), np.zeros(P), -np.ones(P), np.ones(P)]
        out = S.check_vectors("f", names, [list(g) for g in good], None, fields)
        assert all(o.dtype == np.float64 and o.flags.c_contiguous and np.array_equal(o, g) for o, g in zip(out, good))
        for i, name in enumerate(names):
            for bad in (np.zeros(P + 1), np.zeros(P - 1), np.where(np.arange(P) == P - 1, np.nan, 0.0), np.where(np.arange(P) == 0, np.inf, 0.0)):
                _raises("f: %s must be %s" % (name, text), S.check_vectors, "f", names, good[:i] + [bad] + good[i + 1:], None, fields)
        defaults = tuple(np.full(P, float(i)) for i in range(4))
        out = S.check_vectors("f", names, [None, good[1], None, good[3]], defaults, fields)
        assert out[0] is defaults[0] and out[2] is defaults[2] and np.array_equal(out[1], good[1])
        for G, C in ((1, 2), (3, 7)):
            wording = "(generations, candidates, %d) finite numbers" % P
            z = S.check_normals("f", None, 7, (G, C, P), wording)
            assert z.tobytes() == np.random.default_rng(7).standard_normal((G, C, P)).tobytes()
            assert S.check_normals("f", z.tolist(), 0, (G, C, P), wording).tobytes() == z.tobytes()
            _raises("f: normals must be (generations, candidates, %d) finite numbers, got shape (%d, %d)" % (P, G, C * P),
                    S.check_normals, "f", z.reshape(G, C * P), 0, (G, C, P), wording)
            z[0, 1, 0] = np.nan
            _raises("f: normals must be (generations, candidates, %d) finite numbers, got shape (%d, %d, %d)" % (P, G, C, P),
                    S.check_normals, "f", z, 0, (G, C, P), wording)
    _raises("f: normals must be (decisions, generations, candidates, 5) finite numbers with decisions = ceil(max_steps / replan) = 3, "
            "got shape (2, 1, 2, 5)", S.check_normals, "f", np.zeros((2, 1, 2, 5)), 0, (3, 1, 2, 5),
            "(decisions, generations, candidates, 5) finite numbers with decisions = ceil(max_steps / replan) = 3")


def test_the_three_wrappers_raise_them():
    """The _check_* functions of the three bindings, up to where they first ask the engine for anything but its kind."""
    from goldsrl import _ffi, _ffi_swarmcemplan as CP, _ffi_swarmsearch as W, _ffi_tickersearch as T
    swarm, ticker = types.SimpleNamespace(kind=_ffi.ENV_SWARM), types.SimpleNamespace(kind=_ffi.ENV_TICKER)
    start5, start6 = (1.0, 5.0, 0.0, -1.5, 1.5, 0.75), (1, 0, 0, 1, 0.5, 8)
    box5 = (W.DEFAULT_SPREAD, W.DEFAULT_FLOOR, W.DEFAULT_LO, W.DEFAULT_HI)

    def search(fn, engine, start, box, G=2, C=4, K=2, normals=None):
        return lambda: fn(engine, "f", start, box[0], box[1], box[2], box[3], G, C, K, 0, normals, None)

    def cemplan(box, G=2, C=4, M=2):
        return lambda: CP._check_cemplan(swarm, "f", None, start5, 4, 2, G, C, M, box[0], box[1], box[2], box[3], 0, None, None, None)

    counts = "f: generations >= 1, 2 <= candidates <= 1024 and 1 <= elites <= candidates are required, got %d, %d, %d"
    signs = "f: spread >= 0, floor >= 0 and lo <= hi are required"
    _raises("f: the engine is not a Swarm engine", search(W._check_search, ticker, start5, box5))
    _raises("f: the engine is not a Ticker engine", search(T._check_search, swarm, start6, (None,) * 4))
    for make, P, fields in ((lambda **kw: search(W._check_search, swarm, start5, **kw), 5, SWARM_FIELDS),
                            (lambda **kw: search(T._check_search, ticker, start6, **kw), 6, TICKER_FIELDS)):
        box = box5 if P == 5 else T.ticker_search_defaults(start6)
        _raises(counts % (0, 4, 2), make(box=box, G=0))
        _raises(counts % (2, 1025, 2), make(box=box, C=1025))
        _raises(counts % (2, 4, 5), make(box=box, K=5))
        for i, name in enumerate(("spread", "floor", "lo", "hi")):
            _raises("f: %s must be %d finite numbers over %s" % (name, P, fields), make(box=box[:i] + (np.zeros(P + 1),) + box[i + 1:]))
        _raises(signs, make(box=(-np.ones(P),) + tuple(box[1:])))
        _raises(signs, make(box=tuple(box[:2]) + (box[3], box[2])))
        _raises("f: normals must be (generations, candidates, %d) finite numbers, got shape (2, 4)" % P, make(box=box, normals=np.zeros((2, 4))))
    _raises(counts % (2, 4, 0), cemplan(box5, M=0))
    _raises("f: lo must be 5 finite numbers over " + SWARM_FIELDS, cemplan(box5[:2] + ((np.nan,) * 5, box5[3])))
    _raises(signs, cemplan(box5[:1] + ((-1.0,) * 5,) + box5[2:]))
