"""ctypes binding of the cross-entropy search over the six numbers of a Ticker rule (C ABI and the scheme, statement by statement:
include/goldsrl_tickersearch.h): every generation of every candidate on every env of the engine enqueued in one call.
ticker_search_start, ticker_search_rows, ticker_search_candidates and ticker_search_refit are the numpy statements of the scheme,
device-free (the clamp, the draw, the rank and the refit chains are _search.py's, shared with the Swarm searches);
ticker_search_host is the same search composed on the host from them and grl_ticker_sweep: the documented slow path,
and the oracle the device is held to.

The defaults (ticker_search_defaults): a spread of 0.2 on the four weights, 0.1 on the band and max(3, lookback / 4) on the lookback,
floors of a twentieth of that (0.5 on the lookback), the box [0, 1]^4 x [0, 0.5] x [1, 1023].  A start whose lookback is 0 gets a
zero spread and floor there and the box [0, 0]: L = 0 (no trend switch) is a different rule, not a neighbour of L = 1, so the search
neither leaves it nor enters it."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, steps_and_trace
from ._search import (BOX_NAMES, MAX_CANDIDATES, check_box, check_counts, check_normals, check_vectors, search_clamp, search_draw,  # noqa: F401
                      search_rank as ticker_search_rank, search_refit, search_summary)
from ._ffi_tickersweep import RULE_FIELDS, WINDOW, check_ticker_rules, ticker_sweep

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_tickersearch.h: a dict of its own, as the header is a file of its own (tests/test_ticker_search_header.py pins both)
TICKERSEARCH_SIGNATURES = {
    "grl_ticker_search": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "grl_ticker_search_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

DEFAULT_SPREAD = (0.2, 0.2, 0.2, 0.2, 0.1, 3.0)       # the lookback's grows with the start's: ticker_search_defaults
DEFAULT_FLOOR = (0.01, 0.01, 0.01, 0.01, 0.005, 0.5)
DEFAULT_LO = (0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
DEFAULT_HI = (1.0, 1.0, 1.0, 1.0, 0.5, float(WINDOW - 1))
OUTPUTS = ("candidates", "scores", "fit", "order", "mean", "std")


def ticker_search_defaults(start):
    """(spread, floor, lo, hi), float64 (6,) each, for a start rule: the module's defaults, the lookback's spread max(3, L / 4), and
    with L = 0 the lookback pinned (spread, floor, lo, hi all 0 there)."""
    L = float(np.asarray(start, np.float32).reshape(-1)[5])
    spread, floor, lo, hi = (np.array(v, np.float64) for v in (DEFAULT_SPREAD, DEFAULT_FLOOR, DEFAULT_LO, DEFAULT_HI))
    if L == 0:
        spread[5] = floor[5] = lo[5] = hi[5] = 0.0
    else:
        spread[5] = max(spread[5], L / 4.0)
    return spread, floor, lo, hi


def ticker_search_start(start, lo, hi):
    """Statement 1: the float32 start widened and clamped into the box."""
    return search_clamp(np.asarray(start, np.float32).astype(np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64))


def ticker_search_rows(v, return_corrected=False):
    """Statement 3: (..., 6) float64 numbers inside the box as the float32 rows that are played.  With return_corrected also a
    (..., 2) int array: per pair 0 (the casts gave a rule), 1 (f_b = (float)(1 - f_a)) or 2 (and one float32 down)."""
    v = np.asarray(v, np.float64)
    f = np.empty(v.shape, np.float32)
    f[..., :5] = v[..., :5].astype(np.float32)
    f[..., 5] = np.rint(v[..., 5]).astype(np.float32)
    corrected = np.zeros(v.shape[:-1] + (2,), np.int64)
    for pair, (a, b) in enumerate(((0, 1), (2, 3))):
        fa = f[..., a].astype(np.float64)
        s = fa + f[..., b].astype(np.float64)
        over = s > 1.0
        t = 1.0 - fa
        fb = np.where(over, t.astype(np.float32), f[..., b]).astype(np.float32)
        s = fa + fb.astype(np.float64)
        again = over & (s > 1.0)
        fb = np.where(again, np.nextafter(fb, np.float32(0)), fb).astype(np.float32)
        f[..., b] = fb
        corrected[..., pair] = over.astype(np.int64) + again.astype(np.int64)
    return (f, corrected) if return_corrected else f


def ticker_search_candidates(mean, std, z, lo, hi, incumbent=None, return_corrected=False):
    """Statements 2 to 4 for one generation.  mean, std, lo, hi: (6,); z: (C, 6) normals, row 0 ignored; incumbent: the float32 row
    that is candidate 0, or None in generation 0 (statement 3 of the mean).  Returns the (C, 6) float32 table."""
    v = search_draw(mean, std, z, lo, hi)
    if incumbent is None:
        v[0] = mean
    rows, corrected = ticker_search_rows(v, True)
    if incumbent is not None:
        rows[0] = np.asarray(incumbent, np.float32)
        corrected[0] = 0
    return (rows, corrected) if return_corrected else rows


def ticker_search_refit(fit, rows, elites, floor):
    """Statements 7 and 8.  fit (C,), rows (C, 6) float32.  Returns (order (C,) int32, mean (6,), std (6,)), the two sequential
    chains over the K elites in rank order."""
    return search_refit(fit, np.asarray(rows, np.float32).astype(np.float64), int(elites), floor)


def _check_search(engine, fn_name, start, spread, floor, lo, hi, generations, candidates, elites, seed, normals, max_steps):
    if engine.kind != _ffi.ENV_TICKER:
        raise ValueError("%s: the engine is not a Ticker engine" % fn_name)
    start = check_ticker_rules(np.asarray(start, np.float32).reshape(1, -1))[0]
    G, Cn, K = check_counts(fn_name, generations, candidates, elites)
    spread, floor, lo, hi = check_vectors(fn_name, BOX_NAMES, (spread, floor, lo, hi), ticker_search_defaults(start), RULE_FIELDS)
    check_box(fn_name, spread, floor, lo, hi)
    if (lo < 0).any() or (hi[:4] > 1).any() or hi[5] > WINDOW - 1:
        raise ValueError("%s: the box must hold rules only: weights in [0, 1], a band >= 0, a lookback in 0..%d" % (fn_name, WINDOW - 1))
    z = check_normals(fn_name, normals, seed, (G, Cn, 6), "(generations, candidates, 6) finite numbers")
    T, _ = steps_and_trace(engine, fn_name, max_steps)
    return start, spread, floor, lo, hi, G, Cn, K, z, T


def ticker_search(engine, start, spread=None, floor=None, lo=None, hi=None, generations=8, candidates=32, elites=8, seed=0, normals=None,
                  max_steps=None):
    """Search the six numbers of a rule from `start` (up0, up1, dn0, dn1, band, lookback) on every env of the engine from its
    CURRENT state (reset it first) over episodes of up to max_steps steps (default: the engine's max_episode_steps); the engine's
    state is left as it was.  spread, floor, lo, hi: 6 numbers each (default: ticker_search_defaults(start)); normals:
    (generations, candidates, 6), default np.random.default_rng(seed).standard_normal.  One call.

    Returns candidates (G, C, 6) float32, scores (G, C, E), fit (G, C), order (G, C) int32, mean and std (G + 1, 6), and best_rule
    (the last generation's candidates[order[0]]), best_fit and best_per_generation (G,)."""
    start, spread, floor, lo, hi, G, Cn, K, z, T = _check_search(engine, "ticker_search", start, spread, floor, lo, hi, generations,
                                                                 candidates, elites, seed, normals, max_steps)
    lib = _ffi.load_library(extra_signatures=TICKERSEARCH_SIGNATURES)
    engine._check(lib.grl_ticker_search(engine.h, _ffi._ptr(start), _ffi._ptr(spread), _ffi._ptr(floor), _ffi._ptr(lo), _ffi._ptr(hi),
                                        _ffi._ptr(z), G, Cn, K, T))
    out = read_outputs(engine, lib.grl_ticker_search_read,
                       (("candidates", np.float32, (6,)), ("scores", np.float64, (engine.E,)), ("fit", np.float64, ()), ("order", np.int32, ())),
                       (G, Cn))
    out.update(read_outputs(engine, lib.grl_ticker_search_read, (("mean", np.float64, (6,)), ("std", np.float64, (6,))), (G + 1,)))
    return search_summary(out)


def ticker_search_host(engine, start, spread=None, floor=None, lo=None, hi=None, generations=8, candidates=32, elites=8, seed=0,
                       normals=None, max_steps=None):
    """ticker_search composed on the host, a round trip per generation: ticker_sweep(engine, table, max_steps) for the scores (its
    "total"; it refuses a table with a row that is no rule), the fits as float64 adds over the envs in index order, a
    sorted(key=(-fit, index)) and the numpy statements above.  Same arguments and outputs as ticker_search.  ticker_sweep does not
    advance the engine, so neither does this."""
    start, spread, floor, lo, hi, G, Cn, K, z, T = _check_search(engine, "ticker_search_host", start, spread, floor, lo, hi, generations,
                                                                 candidates, elites, seed, normals, max_steps)
    E = engine.E
    out = {"candidates": np.zeros((G, Cn, 6), np.float32), "scores": np.zeros((G, Cn, E)), "fit": np.zeros((G, Cn)),
           "order": np.zeros((G, Cn), np.int32), "mean": np.zeros((G + 1, 6)), "std": np.zeros((G + 1, 6))}
    out["mean"][0] = ticker_search_start(start, lo, hi)
    out["std"][0] = spread
    incumbent = None
    for g in range(G):
        rows = ticker_search_candidates(out["mean"][g], out["std"][g], z[g], lo, hi, incumbent)
        played = ticker_sweep(engine, rows, T)
        assert played["rules"].tobytes() == rows.tobytes()
        s = np.zeros(Cn, np.float64)
        for e in range(E):                                                  # one add per candidate and env, in env order
            s = s + played["total"][:, e]
        out["scores"][g] = played["total"]
        out["fit"][g] = s / np.float64(E)
        out["candidates"][g] = rows
        out["order"][g], out["mean"][g + 1], out["std"][g + 1] = ticker_search_refit(out["fit"][g], rows, K, floor)
        incumbent = rows[out["order"][g, 0]].copy()
    return search_summary(out)
