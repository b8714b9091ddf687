"""ctypes binding of the cross-entropy search over the five real numbers of a Swarm feedback rule (C ABI and the scheme, statement
by statement: include/goldsrl_swarmsearch.h): every generation of every candidate on every env of the engine enqueued in one call.
swarm_search_candidates and swarm_search_refit are the numpy statements of the scheme, device-free (what of them knows nothing of
Swarm is _search.py's, shared with the Ticker search); swarm_search_host is the same search composed on the host from them and
grl_swarm_rules: the documented slow path, and the oracle the device is held to."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, steps_and_trace
from ._search import (BOX_NAMES, MAX_CANDIDATES, check_box, check_counts, check_normals, check_vectors, search_clamp, search_draw, search_refit,  # noqa: F401
                      search_summary)
from ._ffi_swarmrules import N_AGENTS, check_swarm_rules, swarm_rule_offsets, swarm_rules

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_swarmsearch.h: a dict of its own, as the header is a file of its own (tests/test_swarm_search_header.py pins both)
SWARMSEARCH_SIGNATURES = {
    "grl_swarm_search": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "grl_swarm_search_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

SEARCH_FIELDS = ("cancel", "gain", "off_x", "off_y", "radius")
SEARCH_COLS = (0, 1, 3, 4, 5)                       # where they stand in a six-number row (cancel, gain, anchor, off_x, off_y, radius)
DEFAULT_SPREAD = (0.0, 2.0, 0.5, 0.5, 0.3)
DEFAULT_FLOOR = (0.0, 0.05, 0.01, 0.01, 0.01)
DEFAULT_LO = (0.0, 0.0, -4.0, -4.0, 0.0)
DEFAULT_HI = (1.0, 40.0, 4.0, 4.0, 3.0)
OUTPUTS = ("candidates", "offsets", "scores", "fit", "order", "mean", "std")


def swarm_search_ring():
    """(10, 2): (cos, sin)(2 pi a / 10), exactly the expression of swarm_rule_offsets."""
    ang = 2.0 * np.pi * np.arange(N_AGENTS, dtype=np.float64) / N_AGENTS
    return np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=-1))


def swarm_search_start(mean0, lo, hi):
    """Step 1 of the scheme: the start clamped into the box."""
    return search_clamp(*(np.asarray(v, np.float64) for v in (mean0, lo, hi)))


def swarm_search_candidates(mean, std, z, lo, hi, anchor, incumbent):
    """Steps 2 to 4 of the scheme for one generation.  mean, std, lo, hi: (5,); z: (C, 5) normals, row 0 ignored; incumbent: the
    six-number row that is candidate 0.  Returns (candidates (C, 6), offsets (C, 10, 2)) float64."""
    z = np.asarray(z, np.float64)
    cand = np.empty((z.shape[0], 6), np.float64)
    cand[:, SEARCH_COLS] = search_draw(mean, std, z, lo, hi)
    cand[:, 2] = np.float64(anchor)
    cand[0] = np.asarray(incumbent, np.float64)
    ring = swarm_search_ring()
    off = np.empty((z.shape[0], N_AGENTS, 2), np.float64)
    tx = cand[:, 5:6] * ring[None, :, 0]
    off[:, :, 0] = cand[:, 3:4] + tx
    ty = cand[:, 5:6] * ring[None, :, 1]
    off[:, :, 1] = cand[:, 4:5] + ty
    return cand, off


def swarm_search_refit(fit, candidates, elites, floor):
    """Steps 7 and 8 of the scheme.  fit (C,), candidates (C, 6).  Returns (order (C,) int32: by fit descending, a tie to the smaller
    index; mean (5,); std (5,)), the two sequential chains over the K elites in rank order."""
    return search_refit(fit, np.asarray(candidates, np.float64)[:, SEARCH_COLS], int(elites), floor)


def _check_search(engine, fn_name, start, spread, floor, lo, hi, generations, candidates, elites, seed, normals, max_steps):
    if engine.kind != _ffi.ENV_SWARM:
        raise ValueError("%s: the engine is not a Swarm engine" % fn_name)
    start = check_swarm_rules(np.asarray(start, np.float64).reshape(1, -1))[0]
    G, Cn, K = check_counts(fn_name, generations, candidates, elites)
    spread, floor, lo, hi = check_vectors(fn_name, BOX_NAMES, (spread, floor, lo, hi), None, SEARCH_FIELDS)
    check_box(fn_name, spread, floor, lo, hi)
    z = check_normals(fn_name, normals, seed, (G, Cn, 5), "(generations, candidates, 5) finite numbers")
    T, _ = steps_and_trace(engine, fn_name, max_steps)
    return start, spread, floor, lo, hi, G, Cn, K, z, T


def swarm_search(engine, start, spread=DEFAULT_SPREAD, floor=DEFAULT_FLOOR, lo=DEFAULT_LO, hi=DEFAULT_HI, generations=8, candidates=32,
                 elites=8, seed=0, normals=None, max_steps=None):
    """Search the five real numbers of a rule from `start`, a six-number row (cancel, gain, anchor, off_x, off_y, radius) whose anchor
    is kept, on every env of the engine from its CURRENT state (reset it first) over episodes of up to max_steps steps (default: the
    engine's max_episode_steps); the engine's state is left as it was.  spread, floor, lo, hi: 5 numbers each over (cancel, gain,
    off_x, off_y, radius); normals: (generations, candidates, 5), default np.random.default_rng(seed).standard_normal.  One call.

    Returns candidates (G, C, 6), offsets (G, C, 10, 2), scores (E, G, C), fit (G, C), order (G, C) int32, mean and std (G + 1, 5),
    and best_rule (the last generation's candidates[order[0]]), best_fit and best_per_generation (G,)."""
    start, spread, floor, lo, hi, G, Cn, K, z, T = _check_search(engine, "swarm_search", start, spread, floor, lo, hi, generations,
                                                                 candidates, elites, seed, normals, max_steps)
    mean0 = np.ascontiguousarray(start[list(SEARCH_COLS)])
    ring = swarm_search_ring()
    lib = _ffi.load_library(extra_signatures=SWARMSEARCH_SIGNATURES)
    engine._check(lib.grl_swarm_search(engine.h, int(start[2]), _ffi._ptr(mean0), _ffi._ptr(spread), _ffi._ptr(floor), _ffi._ptr(lo),
                                       _ffi._ptr(hi), _ffi._ptr(ring), _ffi._ptr(z), G, Cn, K, T))
    out = read_outputs(engine, lib.grl_swarm_search_read,
                       (("candidates", np.float64, (6,)), ("offsets", np.float64, (N_AGENTS, 2)), ("fit", np.float64, ()), ("order", np.int32, ())),
                       (G, Cn))
    out.update(read_outputs(engine, lib.grl_swarm_search_read, (("scores", np.float64, (G, Cn)),), (engine.E,)))
    out.update(read_outputs(engine, lib.grl_swarm_search_read, (("mean", np.float64, (5,)), ("std", np.float64, (5,))), (G + 1,)))
    return search_summary(out)


def swarm_search_host(engine, start, spread=DEFAULT_SPREAD, floor=DEFAULT_FLOOR, lo=DEFAULT_LO, hi=DEFAULT_HI, generations=8, candidates=32,
                      elites=8, seed=0, normals=None, max_steps=None):
    """swarm_search composed on the host, a round trip per generation: swarm_rules(engine, candidates, max_steps), the scores and
    the fits as Python loops of float64 adds (over t < length, then over the envs), a sorted(key=(-fit, index)) and the two numpy
    functions above.  Same arguments and outputs as swarm_search.  swarm_rules does not advance the engine, so neither does this."""
    start, spread, floor, lo, hi, G, Cn, K, z, T = _check_search(engine, "swarm_search_host", start, spread, floor, lo, hi, generations,
                                                                 candidates, elites, seed, normals, max_steps)
    E = engine.E
    out = {"candidates": np.zeros((G, Cn, 6)), "offsets": np.zeros((G, Cn, N_AGENTS, 2)), "scores": np.zeros((E, G, Cn)),
           "fit": np.zeros((G, Cn)), "order": np.zeros((G, Cn), np.int32), "mean": np.zeros((G + 1, 5)), "std": np.zeros((G + 1, 5))}
    out["mean"][0] = swarm_search_start(start[list(SEARCH_COLS)], lo, hi)
    out["std"][0] = spread
    incumbent = start.copy()
    incumbent[list(SEARCH_COLS)] = out["mean"][0]
    for g in range(G):
        cand, off = swarm_search_candidates(out["mean"][g], out["std"][g], z[g], lo, hi, start[2], incumbent)
        played = swarm_rules(engine, cand, T)
        assert played["offsets"].tobytes() == off.tobytes()                 # step 4 gives the table's own bytes
        for c in range(Cn):
            f = np.float64(0.0)
            for e in range(E):
                s = np.float64(0.0)
                for t in range(int(played["length"][e, c])):
                    s = s + played["rewards"][e, c, t]
                out["scores"][e, g, c] = s
                f = f + s
            out["fit"][g, c] = f / np.float64(E)
        out["candidates"][g], out["offsets"][g] = cand, off
        out["order"][g], out["mean"][g + 1], out["std"][g + 1] = swarm_search_refit(out["fit"][g], cand, K, floor)
        incumbent = cand[out["order"][g, 0]].copy()
    return search_summary(out)
