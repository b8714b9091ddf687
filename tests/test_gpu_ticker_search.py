"""GPU: the cross-entropy search over the six numbers of a Ticker rule, every generation in one call
(include/goldsrl_tickersearch.h, csrc/ticker_search.hip).  The oracle is the same search composed on the host from tested pieces
(goldsrl/_ffi_tickersearch.py:ticker_search_host: grl_ticker_sweep for the episodes, float64 adds in env order, a sort, the numpy
statements of the scheme); every comparison with it is of bytes, over all six outputs and the three summaries.  Only the case that
holds the search to the unmodified reference's fixture has a tolerance, the project's own for a mean total: steps x 2e-7."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("TICKER_CASH", "TICKER_ASSETS", "TICKER_QUANTITY", "TICKER_IDX", "TICKER_START", "TICKER_START0", "ELAPSED", "EPISODE", "NHIST")
OUTPUTS = ("reward", "reward_f64", "done", "elapsed", "obs", "obs_raw", "done_count")
SIX = ("candidates", "scores", "fit", "order", "mean", "std")
SWITCH8, MIXED = (1, 0, 0, 1, 0.5, 8), (0.3, 0.6, 0.6, 0.3, 0.02, 5)
SPREAD = (0.2, 0.2, 0.2, 0.2, 0.1, 3.0)
FLOOR = (0.01, 0.01, 0.01, 0.01, 0.005, 0.5)
LO, HI = (0, 0, 0, 0, 0, 0), (1, 1, 1, 1, 0.5, 64)


@pytest.fixture(scope="module")
def fix(golden):
    g = golden("ticker_rules")
    return {k: g[k] for k in g.files}


def _engine(E, matrix, starts=None, cap=1023, seed=0):
    """as tests/test_gpu_ticker_sweep.py builds its engines"""
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


def _state(eng):
    return {f: eng.get_state(f).tobytes() for f in STATE_FIELDS}


def _same(got, want):
    for k in SIX:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    assert got["best_rule"] == want["best_rule"] and got["best_fit"] == want["best_fit"]
    assert got["best_per_generation"].tobytes() == want["best_per_generation"].tobytes()


def _search_then_host(eng, start, **kw):
    """the one call, then the host composition on the same engine; neither advances it"""
    from goldsrl import _ffi_tickersearch as S
    before = _state(eng)
    got = S.ticker_search(eng, start, **kw)
    assert _state(eng) == before
    want = S.ticker_search_host(eng, start, **kw)
    assert _state(eng) == before
    _same(got, want)
    return got


def _shapes(got, G, C, E):
    assert got["candidates"].shape == (G, C, 6) and got["candidates"].dtype == np.float32 and got["scores"].shape == (G, C, E)
    assert got["fit"].shape == (G, C) and got["order"].shape == (G, C) and got["order"].dtype == np.int32
    assert got["mean"].shape == got["std"].shape == (G + 1, 6)
    assert (np.sort(got["order"], axis=1) == np.arange(C)).all()


# ------------------------------------------------------------------------------------------ 1. the one call is the host composition
@pytest.mark.parametrize("C,K", [(2, 1), (5, 2), (5, 5), (70, 8)])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
def test_the_one_call_is_the_host_composition(E, C, K, fix):
    from goldsrl._ffi_tickersweep import check_ticker_rules
    G, T, m = 3, 48, fix["matrix"]
    eng = _engine(E, m, _starts(E, m, E))
    for start in (SWITCH8, MIXED):
        got = _search_then_host(eng, start, spread=SPREAD, floor=FLOOR, lo=LO, hi=HI, generations=G, candidates=C, elites=K,
                                seed=E * 100 + C, max_steps=T)
        _shapes(got, G, C, E)
        check_ticker_rules(got["candidates"].reshape(-1, 6))
        assert got["candidates"][0, 0].tobytes() == np.array(start, np.float32).tobytes()          # the start lies in the box
        assert np.isfinite(got["scores"]).all() and got["scores"].any()
        if C >= 5:
            assert len(np.unique(got["candidates"][:, :, 5])) > 1                                  # the lookback moves
    eng.close()


# ------------------------------------------------------------------------------------------ 2. the candidate cap
def test_the_cap_of_candidates(fix):
    m = fix["matrix"]
    eng = _engine(1, m, _starts(1, m))
    got = _search_then_host(eng, SWITCH8, spread=SPREAD, floor=FLOOR, lo=LO, hi=HI, generations=2, candidates=1024, elites=64, seed=3,
                            max_steps=4)
    _shapes(got, 2, 1024, 1)
    eng.close()


# ------------------------------------------------------------------------------------------ 3. the incumbent
def test_the_incumbent_is_kept(fix):
    from goldsrl import _ffi_tickersearch as S
    m, G = fix["matrix"], 5
    eng = _engine(3, m, fix["starts"])
    out = S.ticker_search(eng, MIXED, spread=SPREAD, floor=FLOOR, lo=LO, hi=HI, generations=G, candidates=8, elites=3, seed=11, max_steps=64)
    for g in range(G - 1):
        first = out["order"][g, 0]
        assert out["candidates"][g + 1, 0].tobytes() == out["candidates"][g, first].tobytes(), g
        assert out["fit"][g + 1, 0].tobytes() == out["fit"][g, first].tobytes(), g
        assert out["scores"][g + 1, 0].tobytes() == out["scores"][g, first].tobytes(), g
    assert (np.diff(out["best_per_generation"]) >= 0).all()
    assert out["candidates"][0, 0].tobytes() == np.array(MIXED, np.float32).tobytes()                 # generation 0's is the start
    assert out["best_rule"] == tuple(float(v) for v in out["candidates"][G - 1, out["order"][G - 1, 0]]) and out["best_fit"] == out["fit"][G - 1].max()
    assert out["best_fit"] >= out["fit"][0, 0]                                                         # never below the start
    eng.close()


# ------------------------------------------------------------------------------------------ 4. ties and fixed parameters
def test_ties_and_fixed_parameters(fix):
    from goldsrl import _ffi_tickersearch as S
    m, G, C = fix["matrix"], 3, 12
    eng = _engine(3, m, fix["starts"])
    # buy and hold: a candidate whose up0 clamps to 1 gets up1 = 0 from the row statement, and under a wide band it trades once,
    # as the start does: exact twins, ranked by index
    hold = (1, 0, 1, 0, 0.5, 0)
    got = _search_then_host(eng, hold, generations=G, candidates=C, elites=4, seed=0, max_steps=256)
    assert (got["candidates"][:, :, 5] == 0).all() and (got["mean"][:, 5] == 0).all() and (got["std"][:, 5] == 0).all()     # L = 0 stays
    ties = 0
    for g in range(G):
        f = got["fit"][g, got["order"][g]]
        assert (np.diff(f) <= 0).all()
        for a, b, fa, fb in zip(got["order"][g, :-1], got["order"][g, 1:], f[:-1], f[1:]):
            if fa == fb:
                ties += 1
                assert a < b, (g, a, b)
    top = got["fit"][0, got["order"][0, :5]]
    print("ties in all generations: %d; generation 0's top five fits %s" % (ties, top))
    assert ties >= 2 and (got["fit"][:, 1:] == got["fit"][:, :1]).any()                               # twins of the incumbent itself

    # hold cash with no spread and no floor: every row is the start, every fit exactly 0
    cash, zero = (0, 0, 0, 0, 1, 0), np.zeros(6)
    got = _search_then_host(eng, cash, spread=zero, floor=zero, lo=zero, hi=(1, 1, 1, 1, 1, 0), generations=G, candidates=C, elites=3,
                            seed=1, max_steps=64)
    assert got["candidates"].tobytes() == np.tile(np.array(cash, np.float32), (G, C, 1)).tobytes()
    assert (got["order"] == np.arange(C)).all() and not got["fit"].any() and not got["scores"].any() and not got["std"].any()
    assert got["mean"].tobytes() == np.tile(np.array(cash, np.float64), (G + 1, 1)).tobytes()

    # lo = hi pins a parameter whatever the normals; a start outside the box is clamped in mean[0]
    lo, hi = np.array(LO, np.float64), np.array(HI, np.float64)
    lo[4] = hi[4] = 0.25
    got = _search_then_host(eng, (1, 0, 0, 1, 0.5, 100), spread=SPREAD, floor=FLOOR, lo=lo, hi=hi, generations=G, candidates=C, elites=3,
                            seed=4, max_steps=32)
    assert (got["candidates"][:, :, 4] == 0.25).all() and (got["mean"][:, 4] == 0.25).all()
    assert got["mean"][0].tolist() == [1, 0, 0, 1, 0.25, 64] and got["candidates"][0, 0].tolist() == [1, 0, 0, 1, 0.25, 64]
    eng.close()


# ------------------------------------------------------------------------------------------ 5. the simplex edge
def test_the_simplex_edge(fix):
    from goldsrl import _ffi_tickersearch as S
    m, G, C = fix["matrix"], 3, 16
    eng = _engine(5, m, _starts(5, m, 9))
    spread = (0.3, 0.3, 0.3, 0.3, 0.02, 1.0)
    kw = dict(spread=spread, floor=FLOOR, lo=LO, hi=HI, generations=G, candidates=C, elites=4, seed=5, max_steps=48)
    got = _search_then_host(eng, (0.9, 0.1, 0.1, 0.9, 0.05, 3), **kw)           # the host composition sweeps every table: a bad row fails it
    z = np.random.default_rng(5).standard_normal((G, C, 6))
    for g in range(G):
        incumbent = None if g == 0 else got["candidates"][g - 1, got["order"][g - 1, 0]]
        rows, corrected = S.ticker_search_candidates(got["mean"][g], got["std"][g], z[g], LO, HI, incumbent, return_corrected=True)
        assert rows.tobytes() == got["candidates"][g].tobytes()
        assert corrected[1:].any(), g                                          # statement 3 had work to do: the case is not vacuous
        pair = got["candidates"][g].astype(np.float64)
        assert (pair[:, 0] + pair[:, 1] <= 1.0).all() and (pair[:, 2] + pair[:, 3] <= 1.0).all()
    eng.close()


# ------------------------------------------------------------------------------------------ 6. the stops
def test_the_stops_are_the_sweeps(fix):
    from goldsrl import _ffi_tickersweep
    m = fix["matrix"]
    # a TimeLimit shorter than max_steps, three steps into the episode
    E = 5
    eng = _engine(E, m, _starts(E, m, 3), cap=20)
    rng = np.random.RandomState(1)
    for _ in range(3):
        eng.step(np.concatenate([rng.randint(0, 3, size=(E, 2)), rng.uniform(0, 1, size=(E, 2))], axis=1).astype(np.float32))
    assert (eng.get_state("ELAPSED") == 3).all()
    got = _search_then_host(eng, MIXED, spread=SPREAD, floor=FLOOR, lo=LO, hi=HI, generations=2, candidates=6, elites=2, seed=6, max_steps=48)
    for g in range(2):
        played = _ffi_tickersweep.ticker_sweep(eng, got["candidates"][g], 48)
        assert (played["length"] == 17).all() and (played["finished"] == 1).all()
        assert got["scores"][g].tobytes() == played["total"].tobytes(), g
    eng.close()

    # a depleting candidate among the rows: the L = 2 switch over the whole window
    eng = _engine(3, m, fix["starts"])
    switch2 = (1, 0, 0, 1, 0.5, 2)
    got = _search_then_host(eng, switch2, spread=SPREAD, floor=FLOOR, lo=LO, hi=HI, generations=2, candidates=4, elites=2, seed=7, max_steps=1023)
    played = _ffi_tickersweep.ticker_sweep(eng, got["candidates"][0], 1023)
    assert got["candidates"][0, 0].tobytes() == np.array(switch2, np.float32).tobytes()
    assert np.array_equal(played["length"][0], fix["dep_length"]) and (played["depleted"][0] == 1).all()
    assert len(np.unique(played["length"])) > 1                             # the pairs of one launch end at different steps
    assert got["scores"][0].tobytes() == played["total"].tobytes()

    # the end of the window: 23 steps are left
    eng.set_state("TICKER_IDX", np.full(3, 1000, np.int32))
    got = _search_then_host(eng, SWITCH8, spread=SPREAD, floor=FLOOR, lo=LO, hi=HI, generations=2, candidates=4, elites=2, seed=8, max_steps=64)
    played = _ffi_tickersweep.ticker_sweep(eng, got["candidates"][1], 64)
    assert (played["length"] == 23).all() and not played["finished"].any() and got["scores"][1].tobytes() == played["total"].tobytes()
    eng.close()


def test_the_handle_and_the_sweeps_results_are_untouched(fix):
    from goldsrl import _ffi, _ffi_tickersearch as S, _ffi_tickersweep as W
    from goldsrl._ffi_episode import read_outputs
    m, E = fix["matrix"], 65
    lib = _ffi.load_library(extra_signatures=W.TICKER_SWEEP_SIGNATURES)

    def make():
        eng = _engine(E, m, cap=24, seed=7)                                # window starts drawn on the device
        eng.episodes_enable()
        rng = np.random.RandomState(2)
        for _ in range(3):
            eng.step(np.concatenate([rng.randint(0, 3, size=(E, 2)), rng.uniform(0, 1, size=(E, 2))], axis=1).astype(np.float32))
        return eng

    def everything(eng):
        d = {f: eng.get_state(f) for f in STATE_FIELDS}
        d.update({o: eng.read(o) for o in OUTPUTS})
        d["ep_total"], d["ep_len"] = eng.episodes_running()
        return {k: v.tobytes() for k, v in d.items()}

    eng, twin = make(), make()
    before = everything(eng)
    swept = W.ticker_sweep(eng, np.array([SWITCH8, MIXED], np.float32), 30, trace_env=4)
    S.ticker_search(eng, SWITCH8, generations=3, candidates=6, elites=2, max_steps=40)
    S.ticker_search(eng, MIXED, generations=1, candidates=2, elites=1, max_steps=3)             # a smaller one in the grown buffers
    big = S.ticker_search(eng, MIXED, generations=4, candidates=9, elites=3, max_steps=40)      # every buffer grows
    assert everything(eng) == before
    again = read_outputs(eng, lib.grl_ticker_sweep_read, (("total", np.float64, ()), ("length", np.int32, ()), ("trades", np.int32, ()),
                                                          ("final_assets", np.float64, ())), (2, E))
    again.update(read_outputs(eng, lib.grl_ticker_sweep_read, (("trace_rewards", np.float32, ()),), (2, 30)))
    for k, v in again.items():
        assert v.tobytes() == swept[k].tobytes(), k
    _same(big, S.ticker_search(eng, MIXED, generations=4, candidates=9, elites=3, max_steps=40))
    act = np.tile(np.array([1, 2, 0.4, 0.7], np.float32), (E, 1))
    eng.step(act); twin.step(act)                                          # a step after the searches gives the bits it gives without them
    assert everything(eng) == everything(twin)
    eng.close(); twin.close()


# ------------------------------------------------------------------------------------------ 7. validation
def test_error_paths(fix):
    from goldsrl import _ffi, _ffi_tickersearch as S
    lib = _ffi.load_library(extra_signatures=S.TICKERSEARCH_SIGNATURES)
    m = fix["matrix"]
    G, C, K, T = 2, 4, 2, 3
    good = dict(start=np.array(SWITCH8, np.float32), std0=np.array(SPREAD), floor=np.array(FLOOR), lo=np.array(LO, np.float64),
                hi=np.array(HI, np.float64), normals=np.random.default_rng(0).standard_normal((G, C, 6)))
    names = ("start", "std0", "floor", "lo", "hi", "normals")

    def call(h, G=G, C=C, K=K, steps=T, **arrays):
        a = dict(good, **arrays)
        ptrs = [None if a[n] is None else _ffi._ptr(a[n]) for n in names]
        return lib.grl_ticker_search(h, *(ptrs + [G, C, K, steps]))

    def refused(h, word, **kw):
        rc, msg = call(h, **kw), lib.grl_last_error(h)
        assert rc == _ffi.E_INVALID and word in msg and b"grl_ticker_search" in msg, (rc, word, msg)
        return True

    trade = _ffi.Engine(_ffi.ENV_TRADE, 2, n_assets=2)
    with pytest.raises(ValueError):
        S.ticker_search(trade, SWITCH8, generations=G, candidates=C, elites=K, max_steps=T)
    assert refused(trade.h, b"not a Ticker handle")
    fit = np.zeros((G, C))
    assert lib.grl_ticker_search_read(trade.h, b"fit", _ffi._ptr(fit), fit.nbytes) == _ffi.E_INVALID
    trade.close()
    bare = _ffi.Engine(_ffi.ENV_TICKER, 2)                                  # no price table yet
    assert refused(bare.h, b"table")
    bare.close()

    eng = _engine(2, m)
    assert lib.grl_ticker_search_read(eng.h, b"fit", _ffi._ptr(fit), fit.nbytes) == _ffi.E_STATE             # before any run
    for n in names:
        assert refused(eng.h, b"null argument", **{n: None}), n
    # a start the sweep's rule check refuses
    for k, v, word in ((0, 1.5, b"start: up0 is a weight outside"), (1, 0.5, b"start: up0 + up1 is above 1"), (2, 0.5, b"start: dn0 + dn1 is above 1"),
                       (4, -0.5, b"start: band is negative"), (5, 8.5, b"start: lookback is not an integer"), (5, 1024, b"start: lookback"),
                       (3, np.nan, b"start: dn1 is not finite")):
        bad = good["start"].copy()
        bad[k] = v
        assert refused(eng.h, word, start=bad), (k, v)
    for n in names[1:]:                                                     # any number that is not finite, the argument and index named
        for v in (np.nan, np.inf, -np.inf):
            bad = good[n].copy()
            bad.reshape(-1)[-1] = v
            word = b"normals[%d] is not finite" % (G * C * 6 - 1) if n == "normals" else n.encode() + b"[5] (lookback) is not finite"
            assert refused(eng.h, word, **{n: bad}), (n, v)
    bad = good["std0"].copy(); bad[1] = -1e-300
    assert refused(eng.h, b"std0[1] (up1) is negative", std0=bad)
    bad = good["floor"].copy(); bad[4] = -1.0
    assert refused(eng.h, b"floor[4] (band) is negative", floor=bad)
    bad = good["lo"].copy(); bad[2] = 1.5
    assert refused(eng.h, b"lo[2] is above hi[2]", lo=bad)
    bad = good["lo"].copy(); bad[0] = -0.25                                 # a weight's box outside [0, 1]
    assert refused(eng.h, b"lo[0] (up0): a weight's box", lo=bad)
    bad = good["hi"].copy(); bad[3] = 1.25
    assert refused(eng.h, b"hi[3] (dn1): a weight's box", hi=bad)
    bad = good["lo"].copy(); bad[4] = -0.125                                # a band's box below 0
    assert refused(eng.h, b"lo[4] (band): the band's box", lo=bad)
    bad = good["lo"].copy(); bad[5] = -1.0                                  # a lookback's box outside 0..1023
    assert refused(eng.h, b"lo[5] (lookback): the lookback's box", lo=bad)
    bad = good["hi"].copy(); bad[5] = 1023.5
    assert refused(eng.h, b"hi[5] (lookback): the lookback's box", hi=bad)
    assert refused(eng.h, b"G must", G=0) and refused(eng.h, b"G must", G=-3)
    assert refused(eng.h, b"C must", C=1) and refused(eng.h, b"C must", C=1025)
    assert refused(eng.h, b"K must", K=0) and refused(eng.h, b"K must", K=C + 1)
    assert refused(eng.h, b"max_steps", steps=0)
    # an output past 2^31 - 1 elements: 2^20 generations of 1 024 candidates on 2 envs are 2^31 scores.  The call is refused on its
    # sizes, before it looks at the normals, which are therefore the small array of the other cases
    assert refused(eng.h, b"does not fit in int32", G=1 << 20, C=1024)
    assert lib.grl_ticker_search_read(eng.h, b"fit", _ffi._ptr(fit), fit.nbytes) == _ffi.E_STATE             # a refused call is no run
    for kw in (dict(generations=0), dict(candidates=1), dict(candidates=1025), dict(elites=0), dict(elites=C + 1), dict(spread=(0, -1, 0, 0, 0, 0)),
               dict(floor=(0, 0, 0, 0, 0, -1)), dict(lo=(0, 0, 1.5, 0, 0, 0)), dict(normals=np.zeros((G, C, 5))), dict(max_steps=0),
               dict(hi=(1, np.inf, 1, 1, 1, 8)), dict(hi=(1, 1, 1, 1.5, 1, 8)), dict(lo=(0, 0, 0, 0, -1, 0)), dict(hi=(1, 1, 1, 1, 1, 1024)),
               dict(spread=(0, 0, 0, 0, 0))):
        with pytest.raises(ValueError):                                         # the host checks, before the C ABI
            S.ticker_search(eng, SWITCH8, **dict(dict(generations=G, candidates=C, elites=K, max_steps=T), **kw))
    with pytest.raises(ValueError):
        S.ticker_search(eng, (0.6, 0.5, 0, 0, 0.1, 0), generations=G, candidates=C, elites=K, max_steps=T)    # no rule
    assert call(eng.h) == _ffi.OK
    shapes = {"candidates": (np.float32, (G, C, 6)), "scores": (np.float64, (G, C, 2)), "fit": (np.float64, (G, C)),
              "order": (np.int32, (G, C)), "mean": (np.float64, (G + 1, 6)), "std": (np.float64, (G + 1, 6))}
    for name, (dt, shape) in shapes.items():
        a = np.zeros(shape, dt)
        assert lib.grl_ticker_search_read(eng.h, name.encode(), _ffi._ptr(a), a.nbytes - a.itemsize) == _ffi.E_SIZE, name
        assert lib.grl_ticker_search_read(eng.h, name.encode(), _ffi._ptr(a), a.nbytes + a.itemsize) == _ffi.E_SIZE, name
        assert lib.grl_ticker_search_read(eng.h, name.encode(), _ffi._ptr(a), a.nbytes) == _ffi.OK and a.any(), name
    assert lib.grl_ticker_search_read(eng.h, b"nothing", _ffi._ptr(fit), fit.nbytes) == _ffi.E_INVALID
    assert lib.grl_ticker_search_read(eng.h, b"offsets", _ffi._ptr(fit), fit.nbytes) == _ffi.E_INVALID       # the Swarm search's, not this one's
    assert lib.grl_ticker_search_read(eng.h, None, _ffi._ptr(fit), fit.nbytes) == _ffi.E_INVALID
    assert lib.grl_ticker_search_read(eng.h, b"fit", None, fit.nbytes) == _ffi.E_INVALID
    eng.step_async(np.zeros((2, 4), np.float32))                                # a step in flight
    assert refused(eng.h, b"in flight")
    eng.wait()
    assert call(eng.h) == _ffi.OK
    uncapped = _engine(2, m, cap=0)
    with pytest.raises(ValueError):
        S.ticker_search(uncapped, SWITCH8, generations=G, candidates=C, elites=K)                           # no TimeLimit, no default
    uncapped.close(); eng.close()


# ------------------------------------------------------------------------------------------ 8. pinned to the reference
def test_the_reference_fixture(fix, golden):
    """The search from (1, 0, 0, 1, 0.5, 8) on the three windows of ticker_rules.npz, 256 steps, 4 generations of 12 candidates, 4
    elites, against what the same statements gave on the unmodified reference TickerEnv (tests/golden/ticker_search.npz), with the
    normals stored there.  The generator asserts that any two fits among ranks 0..K are bit-equal twins or further apart than twice
    the bound on a mean total, 256 x 2e-7, so order[:, :K] and with it every generation's table are compared exactly; the fits
    within the bound."""
    from goldsrl.baselines import TickerRuleSearch
    g = golden("ticker_search")
    Gn, C, K = (int(v) for v in g["shape"])
    steps = int(g["steps"])
    assert np.array_equal(g["starts"], fix["starts"]) and steps == 256
    eng = _engine(3, fix["matrix"], fix["starts"])
    b = TickerRuleSearch(eng, g["start"], generations=Gn, candidates=C, elites=K, normals=g["normals"], spread=g["spread"], floor=g["floor"],
                         lo=g["lo"], hi=g["hi"], max_episode_steps=steps)
    out = b.run()
    bound = steps * 2e-7
    worst = np.abs(out["fit"] - g["fit"]).max(axis=1)
    print("largest deviation of a fit from the fixture, per generation, in units of the bound: %s; smallest gaps %s; best per generation %s"
          % (", ".join("%.3g" % (v / bound) for v in worst), g["min_gap"], out["best_per_generation"]))
    assert out["candidates"].tobytes() == g["candidates"].tobytes()
    assert np.array_equal(out["order"][:, :K], g["order"][:, :K])
    assert out["mean"].tobytes() == g["mean"].tobytes() and out["std"].tobytes() == g["std"].tobytes()
    assert (np.abs(out["fit"] - g["fit"]) <= bound).all()
    rule, total = b.best()
    assert rule == tuple(float(v) for v in g["candidates"][Gn - 1, g["order"][Gn - 1, 0]]) and total == out["best_fit"]
    assert b.results == [(tuple(float(v) for v in g["start"]), rule, total)]
    assert b.play_on(eng) == total                                             # the found rule through grl_ticker_sweep: the episode scored
    assert total > out["fit"][0, 0] + 0.03                                     # from -0.123 to -0.071 in the fixture
    eng.close()


# ------------------------------------------------------------------------------------------ 9. the monitor
class _Writer(object):
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def flush(self):
        pass


def test_monitor_search_baseline(fix):
    from goldsrl import _ffi_gated, _ffi_tickersweep
    from goldsrl.agents.a3c.policy_monitor import GatedPolicyMonitor
    from goldsrl.baselines import TickerRuleBaseline, TickerRuleSearch
    m, w = fix["matrix"], _Writer()
    mon = GatedPolicyMonitor(m, summary_writer=w, n_envs=3, max_episode_steps=40)
    eng = mon.net.eng
    eng.reset()
    fresh = {f: eng.get_state(f) for f in STATE_FIELDS}
    rule, total = mon.ticker_search_baseline(2, 4, 2)
    after = {f: eng.get_state(f) for f in STATE_FIELDS}
    for f in STATE_FIELDS:
        if f != "EPISODE":                                                     # every reset starts a new episode
            assert after[f].tobytes() == fresh[f].tobytes(), f
    b = TickerRuleSearch(eng, generations=2, candidates=4, elites=2, max_episode_steps=40)          # the engine is reset: the same windows
    assert b.best() == (rule, total) and b.results == mon.search_baseline_results
    assert (rule, total, total) == (mon.search_baseline_rule, mon.search_baseline_total_reward, mon.search_baseline_in_sample_total_reward)
    assert b.start_total == TickerRuleBaseline(eng, max_episode_steps=40).best_total()[2] and total >= b.start_total - 40 * 2.0 ** -50
    assert not hasattr(mon, "baseline_total_reward") and not hasattr(mon, "ceiling_total_reward")   # the other flags' scalars are theirs
    # two starts: one call each, the better found rule kept
    two = TickerRuleSearch(eng, starts=[SWITCH8, MIXED], generations=2, candidates=4, elites=2, max_episode_steps=40)
    two.run()
    assert [r[0] for r in two.results] == [tuple(float(v) for v in np.array(s, np.float32)) for s in (SWITCH8, MIXED)]
    assert two.best()[1] == max(r[2] for r in two.results) and two.best()[0] in [r[1] for r in two.results]

    # tuned on a second table, played on the monitor's.  From buy-and-hold of the inverse asset, so that the found rule trades
    # (from the best default rule of 40 steps, hold cash, both totals would be exactly 0)
    other = np.ascontiguousarray(m[::-1])                                      # the same prices backwards: a falling market
    rule2, total2 = mon.ticker_search_baseline(2, 4, 2, starts=[(0, 1, 0, 1, 0.5, 0)], tune_table=other)
    assert len(mon.search_baseline_results) == 1 and mon.search_baseline_results[0][0] == (0, 1, 0, 1, 0.5, 0)
    eng.reset()
    direct = _ffi_tickersweep.ticker_sweep(eng, np.array([rule2], np.float32), 40)["total"][0]
    s = np.float64(0.0)
    for v in direct:
        s = s + v
    assert total2 == float(s / np.float64(3)) == mon.search_baseline_total_reward
    assert mon.search_baseline_in_sample_total_reward != total2 and np.isfinite(mon.search_baseline_in_sample_total_reward)
    assert (eng.get_state("ELAPSED") == 0).all() and (eng.get_state("TICKER_IDX") == 0).all()
    mon.eval_once(_ffi_gated.default_init_gated(3))
    n = len(w.rows)
    mon.write_search_baseline_scalars(9)
    assert w.rows[n:] == [("eval/search_baseline_total_reward", total2, 9),
                          ("eval/mean_total_reward_minus_search_baseline", mon.log["mean_total_reward"][-1] - total2, 9),
                          ("eval/search_baseline_in_sample_total_reward", mon.search_baseline_in_sample_total_reward, 9)]
    mon.close()


def _tables(tmp_path):
    """a training table and a held-out one, as tests/test_gpu_ticker_sweep.py makes its own"""
    paths = []
    for name, seed, drift in (("train.npz", 4, 3e-4), ("held.npz", 5, -1e-4)):
        rng = np.random.RandomState(seed)
        days = 600
        closes = 100.0 * np.exp(np.cumsum(rng.normal(drift, 0.008, size=days)))
        opens = closes * np.exp(rng.normal(0, 0.003, size=days))
        np.savez(tmp_path / name, Open=opens, Close=closes, Volume=rng.uniform(1e5, 5e5, size=days).round())
        paths.append(str(tmp_path / name))
    return paths


def test_train_ticker_search_baseline_flag(tmp_path):
    import glob
    import os

    from goldsrl import utils_tfevents
    from goldsrl.scripts import train_ticker
    train, held = _tables(tmp_path)

    def run(name, extra):
        out = tmp_path / name
        train_ticker.main(["--table", train, "--envs", "64", "--steps", "4", "--updates", "2", "--eval-envs", "3", "--eval-every", "1",
                           "--out", str(out)] + extra)
        (events,) = glob.glob(os.path.join(str(out), "events.out.tfevents.*"))
        scalars = {}
        for tag, value, step, _ in utils_tfevents.read_scalars(events):
            scalars.setdefault(tag, []).append((step, value))
        return scalars

    plain = run("plain", ["--baseline"])
    same = run("same", ["--baseline", "--search-baseline", "2:4:2"])
    other = run("other", ["--baseline", "--search-baseline", "2:4:2", "--eval-table", held])
    new = {"eval/search_baseline_total_reward", "eval/mean_total_reward_minus_search_baseline"}
    assert not new & set(plain) and set(same) == set(plain) | new
    assert set(other) == set(same) | {"eval/search_baseline_in_sample_total_reward"}
    for tag in plain:                                                       # the other flags' scalars are left alone
        assert [s for s, _ in same[tag]] == [s for s, _ in plain[tag]], tag
    assert same["eval/baseline_total_reward"] == plain["eval/baseline_total_reward"]
    for scalars in (same, other):
        for tag in set(scalars) - set(plain):
            assert [s for s, _ in scalars[tag]] == [s for s, _ in scalars["eval/mean_total_reward"]] and len(scalars[tag]) == 2
        b = [v for _, v in scalars["eval/search_baseline_total_reward"]]
        assert b[0] == b[1] and np.isfinite(b[0])                           # one search serves every evaluation
        for (_, mean), (_, d), bv in zip(scalars["eval/mean_total_reward"], scalars["eval/mean_total_reward_minus_search_baseline"], b):
            assert abs(d - (mean - bv)) <= 1e-6 * max(1.0, abs(mean), abs(bv))      # scalars are stored as float32
    assert same["eval/search_baseline_total_reward"][0][1] >= same["eval/baseline_total_reward"][0][1] - 1e-6   # never below its start


def test_the_script_reports_every_start(tmp_path, capsys):
    import json

    from goldsrl.scripts import ticker_search
    train, held = _tables(tmp_path)
    path = str(tmp_path / "found.json")
    rec = ticker_search.main(["--table", train, "--eval-table", held, "--envs", "3", "--steps", "64", "--search", "2:4:2",
                              "--starts", "1,0,0,1,0.5,8", "0.3,0.6,0.6,0.3,0.02,5", "--json", path])
    printed = capsys.readouterr().out
    assert printed.count("in-sample") == 2 and printed.count("held-out") == 3 and "best default rule" in printed
    kept = json.load(open(path))
    assert kept["best_in_sample"] == rec["best_in_sample"] == max(r["in_sample"] for r in rec["starts"]) and len(kept["starts"]) == 2
    assert [r["start"] for r in rec["starts"]] == [(1.0, 0.0, 0.0, 1.0, 0.5, 8.0), tuple(float(v) for v in np.array(MIXED, np.float32))]
    assert all(np.isfinite(r["held_out"]) and r["held_out"] != r["in_sample"] for r in rec["starts"])
    assert rec["best_held_out"] in [r["held_out"] for r in rec["starts"]]
