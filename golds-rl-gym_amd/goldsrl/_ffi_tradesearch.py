"""ctypes binding of the cross-entropy search over the four numbers of a TradeAR1 rule (C ABI and the scheme, statement by statement:
include/goldsrl_tradesearch.h): every generation of every candidate on every env of the engine enqueued in one call.
trade_rule4_actions is the rule on the host, trade_search_start, trade_search_rows, trade_search_candidates and trade_search_refit
the numpy statements of the scheme, device-free (the clamp, the draw, the rank and the refit chains are _search.py's, shared with
the Swarm and Ticker searches); trade_search_host is the same search composed on the host from them and the per-step path: the
documented slow path, and the oracle the device is held to.  trade_search_play plays ONE rule on every env through the same call.

The defaults (trade_search_defaults).  The measured scale of the totals at 16 assets runs from 1.13 (best default rule) to 2.75 (the
foresight ceiling) over 1 024 steps: a rule's numbers matter in the first digit.  Prices are exp of an AR(1) with a stationary
standard deviation of 0.05, so `ref` gets a spread of 0.02 (two fifths of that) in the box [0.8, 1.25], four deviations either
side; `bias` is an action, spread 0.25 in [-1, 1].  The gains run over decades (the default table's go from 1 to 100, and a gain
above 1 / 0.05 = 20 already saturates the clip at one deviation), so a fixed linear spread cannot serve them: theirs is half the
start's gain (at least 1), which lets generation 0 reach a factor of three either way, and the refit (statement 8) rescales it
from there on -- a linear draw around a mean that moves, not a log-normal one, which would need a statement of its own in the
scheme.  Their box is [0, 10 000]: a negative gain buys what rises, which is a different rule.  Floors are a twentieth of the
spreads.  A caller who wants `ref` (or any number) fixed gives it spread 0 and floor 0."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, steps_and_trace
from ._search import (BOX_NAMES, MAX_CANDIDATES, check_box, check_counts, check_normals, check_vectors, search_clamp, search_draw,  # noqa: F401
                      search_rank as trade_search_rank, search_refit, search_summary)

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_tradesearch.h: a dict of its own, as the header is a file of its own (tests/test_trade_search_header.py pins both)
TRADESEARCH_SIGNATURES = {
    "grl_trade_search": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "grl_trade_search_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

RULE4_FIELDS = ("gain_buy", "gain_sell", "bias", "ref")
DEFAULT_SPREAD = (1.0, 1.0, 0.25, 0.02)               # the gains' grow with the start's: trade_search_defaults
DEFAULT_LO = (0.0, 0.0, -1.0, 0.8)
DEFAULT_HI = (10000.0, 10000.0, 1.0, 1.25)
OUTPUTS = ("candidates", "scores", "fit", "order", "mean", "std")


def trade_rule4_actions(rules, prices):
    """The host form of the rule: d = p - ref; g = gain_buy where d < 0 else gain_sell; clip(bias - g * d, -1, 1) rounded to
    float32, one IEEE float64 operation after the other -- the device's bits.  rules: (gain_buy, gain_sell, bias, ref) or
    (n_rules, 4), played as float32; prices: float64, any shape.  Returns float32 of prices' shape, or (n_rules,) + that shape."""
    r = np.asarray(rules, np.float32).astype(np.float64)
    p = np.asarray(prices, np.float64)
    if r.shape[-1:] != (4,) or r.ndim > 2:
        raise ValueError("trade_rule4_actions: rules must be (4,) or (n_rules, 4) of %s, got shape %s" % ((RULE4_FIELDS,), r.shape))
    if r.ndim == 1:
        gb, gs, b, ref = r
    else:
        gb, gs, b, ref = (r[:, k].reshape((-1,) + (1,) * p.ndim) for k in range(4))
    d = p - ref
    g = np.where(d < 0.0, gb, gs)
    m = g * d
    x = b - m
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def check_trade_rule4(fn_name, rule):
    """One rule as 4 finite float32."""
    r = np.ascontiguousarray(np.asarray(rule, np.float32).reshape(-1))
    if r.shape != (4,) or not np.isfinite(r).all():
        raise ValueError("%s: a rule is 4 finite numbers %s" % (fn_name, (RULE4_FIELDS,)))
    return r


def trade_search_defaults(start):
    """(spread, floor, lo, hi), float64 (4,) each, for a start rule: the module's defaults with each gain's spread
    max(1, |gain| / 2), floors a twentieth of the spreads."""
    s = np.asarray(start, np.float32).reshape(-1).astype(np.float64)
    spread, lo, hi = (np.array(v, np.float64) for v in (DEFAULT_SPREAD, DEFAULT_LO, DEFAULT_HI))
    for k in (0, 1):
        spread[k] = max(spread[k], abs(s[k]) / 2.0)
    return spread, spread / 20.0, lo, hi


def trade_search_start(start, lo, hi):
    """Statement 1: the float32 start widened and clamped into the box."""
    return search_clamp(np.asarray(start, np.float32).astype(np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64))


def trade_search_rows(v):
    """Statement 3: (..., 4) float64 numbers inside the box as the float32 rows that are played -- the cast, nothing more."""
    return np.asarray(v, np.float64).astype(np.float32)


def trade_search_candidates(mean, std, z, lo, hi, incumbent=None):
    """Statements 2 to 4 for one generation.  mean, std, lo, hi: (4,); z: (C, 4) normals, row 0 ignored; incumbent: the float32 row
    that is candidate 0, or None in generation 0 (statement 3 of the mean).  Returns the (C, 4) float32 table."""
    v = search_draw(mean, std, z, lo, hi)
    v[0] = mean
    rows = trade_search_rows(v)
    if incumbent is not None:
        rows[0] = np.asarray(incumbent, np.float32)
    return rows


def trade_search_refit(fit, rows, elites, floor):
    """Statements 7 and 8.  fit (C,), rows (C, 4) float32.  Returns (order (C,) int32, mean (4,), std (4,)), the two sequential
    chains over the K elites in rank order."""
    return search_refit(fit, np.asarray(rows, np.float32).astype(np.float64), int(elites), floor)


def _check_tape(engine, fn_name, normals, T):
    """The tape as the C side takes it, (T, n_assets, E) float32, or None."""
    if normals is None:
        return None
    tape = np.asarray(normals, np.float32)
    if tape.shape != (T, engine.E, engine.cfg.n_assets):
        raise ValueError("%s: tape must be (max_steps, E, n_assets) = %s, got %s" % (fn_name, (T, engine.E, engine.cfg.n_assets), tape.shape))
    return np.ascontiguousarray(tape.transpose(0, 2, 1))                    # the device layout: a * E + env per step


def _check_search(engine, fn_name, start, spread, floor, lo, hi, generations, candidates, elites, seed, normals, max_steps):
    if engine.kind != _ffi.ENV_TRADE:
        raise ValueError("%s: the engine is not a TradeAR1 engine" % fn_name)
    start = check_trade_rule4(fn_name, start)
    G, Cn, K = check_counts(fn_name, generations, candidates, elites)
    spread, floor, lo, hi = check_vectors(fn_name, BOX_NAMES, (spread, floor, lo, hi), trade_search_defaults(start), RULE4_FIELDS)
    check_box(fn_name, spread, floor, lo, hi)
    with np.errstate(over="ignore"):
        if not (np.isfinite(lo.astype(np.float32)).all() and np.isfinite(hi.astype(np.float32)).all()):
            raise ValueError("%s: every bound of the box must be finite as float32" % fn_name)
    z = check_normals(fn_name, normals, seed, (G, Cn, 4), "(generations, candidates, 4) finite numbers")
    T, _ = steps_and_trace(engine, fn_name, max_steps)
    return start, spread, floor, lo, hi, G, Cn, K, z, T


def trade_search(engine, start, spread=None, floor=None, lo=None, hi=None, generations=8, candidates=32, elites=8, seed=0, normals=None,
                 max_steps=None, tape=None):
    """Search the four numbers of a rule from `start` (gain_buy, gain_sell, bias, ref) on every env of the engine from its CURRENT
    state (reset it first) over episodes of up to max_steps steps (default: the engine's max_episode_steps); the engine's state,
    its generator's counters included, is left as it was.  spread, floor, lo, hi: 4 numbers each (default:
    trade_search_defaults(start)); normals: the search's, (generations, candidates, 4), default
    np.random.default_rng(seed).standard_normal.  tape: None (the engine's own price generator, at the counters its next steps
    would use) or the price normals (max_steps, E, n_assets) whose row t moves the prices after step t, as trade_sweep's `normals`.
    One call.

    Returns candidates (G, C, 4) float32, scores (G, C, E), fit (G, C), order (G, C) int32, mean and std (G + 1, 4), and best_rule
    (the last generation's candidates[order[0]]), best_fit and best_per_generation (G,)."""
    start, spread, floor, lo, hi, G, Cn, K, z, T = _check_search(engine, "trade_search", start, spread, floor, lo, hi, generations,
                                                                 candidates, elites, seed, normals, max_steps)
    tp = _check_tape(engine, "trade_search", tape, T)
    lib = _ffi.load_library(extra_signatures=TRADESEARCH_SIGNATURES)
    engine._check(lib.grl_trade_search(engine.h, _ffi._ptr(start), _ffi._ptr(spread), _ffi._ptr(floor), _ffi._ptr(lo), _ffi._ptr(hi),
                                       _ffi._ptr(z), None if tp is None else _ffi._ptr(tp), G, Cn, K, T))
    out = read_outputs(engine, lib.grl_trade_search_read,
                       (("candidates", np.float32, (4,)), ("scores", np.float64, (engine.E,)), ("fit", np.float64, ()), ("order", np.int32, ())),
                       (G, Cn))
    out.update(read_outputs(engine, lib.grl_trade_search_read, (("mean", np.float64, (4,)), ("std", np.float64, (4,))), (G + 1,)))
    return search_summary(out)


def trade_search_play(engine, rule, max_steps=None, tape=None):
    """The totals (E,) float64 of ONE rule (gain_buy, gain_sell, bias, ref) on every env from the engine's CURRENT state: a
    one-generation call with zero spread and floor in the box [rule, rule], whose every candidate is the rule; scores[0, 0].  The
    search takes no fewer than 2 candidates, so the rule is played twice and one update launch runs: with 2 or 4 candidates per lane
    (GRL_TRADE_SEARCH_RPL) both copies share a lane and its price path and the second costs the account steps only; with 1 the
    call costs two episodes per env.  The engine's state is left as it was."""
    r = check_trade_rule4("trade_search_play", rule).astype(np.float64)
    zero = np.zeros(4)
    out = trade_search(engine, r, zero, zero, r, r, generations=1, candidates=2, elites=1, normals=np.zeros((1, 2, 4)), max_steps=max_steps,
                       tape=tape)
    assert out["candidates"][0, 0].tobytes() == r.astype(np.float32).tobytes()
    return out["scores"][0, 0].copy()


def fit_mean(totals):
    """Statement 6 on one candidate's (E,) totals: adds in env order, one division."""
    s = np.float64(0.0)
    for v in np.asarray(totals, np.float64):
        s = s + v
    return float(s / np.float64(len(totals)))


def _play_per_step(engine, rows, tape, T):
    """scores (C, E) of the rows on the per-step path: for every row the engine is reset and stepped with the host-computed
    trade_rule4_actions on TRADE_PRICES, tape[t] set as TRADE_NORMALS before step t; an env's rewards are added, float64 in step
    order, until its first done."""
    E = engine.E
    scores = np.zeros((len(rows), E), np.float64)
    for c, row in enumerate(rows):
        engine.reset()
        s, alive = np.zeros(E, np.float64), np.ones(E, bool)
        for t in range(T):
            engine.set_state("TRADE_NORMALS", tape[t])
            engine.step(trade_rule4_actions(row, engine.get_state("TRADE_PRICES")))
            s = np.where(alive, s + engine.read("reward").astype(np.float64), s)
            alive &= ~(engine.read("done") > 0)
            if not alive.any():
                break
        scores[c] = s
    engine.reset()
    return scores


def trade_search_host(engine, start, spread=None, floor=None, lo=None, hi=None, generations=8, candidates=32, elites=8, seed=0,
                      normals=None, max_steps=None, tape=None):
    """trade_search composed on the host: per generation the table by the numpy statements above, every candidate scored through
    the per-step path (grl_step with trade_rule4_actions computed here from the engine's prices), the fits as float64 adds over the
    envs in index order, a sorted(key=(-fit, index)) and the refit.  The per-step path cannot rewind the engine's price generator,
    so this form needs an engine with F_INJECT_NOISE and a tape, plays every candidate from the RESET state and leaves the engine
    reset; trade_search on the reset engine with the same tape gives the same bytes.  Same outputs as trade_search."""
    start, spread, floor, lo, hi, G, Cn, K, z, T = _check_search(engine, "trade_search_host", start, spread, floor, lo, hi, generations,
                                                                 candidates, elites, seed, normals, max_steps)
    if tape is None or not engine.cfg.flags & _ffi.F_INJECT_NOISE:
        raise ValueError("trade_search_host: the per-step path needs an engine with F_INJECT_NOISE and a tape")
    _check_tape(engine, "trade_search_host", tape, T)
    tape = np.asarray(tape, np.float32)
    E = engine.E
    out = {"candidates": np.zeros((G, Cn, 4), np.float32), "scores": np.zeros((G, Cn, E)), "fit": np.zeros((G, Cn)),
           "order": np.zeros((G, Cn), np.int32), "mean": np.zeros((G + 1, 4)), "std": np.zeros((G + 1, 4))}
    out["mean"][0] = trade_search_start(start, lo, hi)
    out["std"][0] = spread
    incumbent = None
    for g in range(G):
        rows = trade_search_candidates(out["mean"][g], out["std"][g], z[g], lo, hi, incumbent)
        scores = _play_per_step(engine, rows, tape, T)
        s = np.zeros(Cn, np.float64)
        for e in range(E):                                                  # one add per candidate and env, in env order
            s = s + scores[:, e]
        out["scores"][g] = scores
        out["fit"][g] = s / np.float64(E)
        out["candidates"][g] = rows
        out["order"][g], out["mean"][g + 1], out["std"][g + 1] = trade_search_refit(out["fit"][g], rows, K, floor)
        incumbent = rows[out["order"][g, 0]].copy()
    return search_summary(out)
