"""ctypes binding of the scripted rule baseline sweep of the Ticker env (C ABI: include/goldsrl_tickersweep.h): every (env, rule)
pair plays a whole episode in one kernel launch.  ticker_rule_actions is the host form of the rule, device-free."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, reward_moments, steps_and_trace

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_tickersweep.h: a dict of its own, as the header is a file of its own (tests/test_ticker_sweep_header.py pins both)
TICKER_SWEEP_SIGNATURES = {
    "grl_ticker_sweep": (C.c_int, [_P, _P, _I, _I, _I]),
    "grl_ticker_sweep_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

RULE_FIELDS = ("up0", "up1", "dn0", "dn1", "band", "lookback")
WINDOW = 1024

_PAIR_DTYPES = (("total", np.float64, ()), ("sum_sq", np.float64, ()), ("final_assets", np.float64, ()), ("min", np.float32, ()),
                ("max", np.float32, ()), ("length", np.int32, ()), ("trades", np.int32, ()), ("finished", np.uint8, ()),
                ("depleted", np.uint8, ()))
_TRACE_DTYPES = (("trace_rewards", np.float32, ()), ("trace_assets", np.float64, ()), ("trace_actions", np.float32, (4,)))


def check_ticker_rules(rules):
    """rules as the (n_rules, 6) float32 array the device plays, or ValueError naming the offending rule and field: the checks of
    grl_ticker_sweep, device-free."""
    r = np.asarray(rules, np.float32)
    if r.ndim != 2 or r.shape[1] != 6 or r.shape[0] < 1:
        raise ValueError("rules must be (n_rules, 6) of (up0, up1, dn0, dn1, band, lookback), got shape %s" % (r.shape,))
    for i, u in enumerate(r):
        for k, name in enumerate(RULE_FIELDS):
            if not np.isfinite(u[k]):
                raise ValueError("rule %d: %s is not finite" % (i, name))
        for k in range(4):
            if u[k] < 0 or u[k] > 1:
                raise ValueError("rule %d: %s is a weight outside [0, 1]" % (i, RULE_FIELDS[k]))
        if float(u[0]) + float(u[1]) > 1.0:
            raise ValueError("rule %d: up0 + up1 is above 1" % i)
        if float(u[2]) + float(u[3]) > 1.0:
            raise ValueError("rule %d: dn0 + dn1 is above 1" % i)
        if u[4] < 0:
            raise ValueError("rule %d: band is negative" % i)
        if u[5] < 0 or u[5] > WINDOW - 1 or u[5] != np.floor(u[5]):
            raise ValueError("rule %d: lookback is not an integer in 0..1023" % i)
    return np.ascontiguousarray(r)


def _rule_columns(rules, ndim):
    """The six parameters widened to float64: scalars for one rule, (n_rules, 1, ...) columns for many."""
    r = np.asarray(rules, np.float32).astype(np.float64)
    if r.ndim == 1:
        return tuple(r)
    return tuple(r[:, k].reshape((-1,) + (1,) * ndim) for k in range(6))


def ticker_rule_back(rules, table, start, idx):
    """The lookback price the rule compares p0 with: table[start + max(idx - L, 0)][0], L = (int)lookback.  start, idx: (E,).
    Returns (E,), or (n_rules, E) for (n_rules, 6) rules."""
    start, idx = np.asarray(start, np.int64), np.asarray(idx, np.int64)
    L = np.asarray(_rule_columns(rules, idx.ndim)[5]).astype(np.int64)
    return np.asarray(table, np.float64)[start + np.maximum(idx - L, 0), 0]


def ticker_rule_actions(rules, cash, qty, prices, back):
    """The host form of the rule (include/goldsrl_tickersweep.h), one IEEE float64 operation after the other -- the device's bits.
    rules: one rule (6,) or (n_rules, 6), played as float32 widened to float64; cash (...,), qty (..., 2), prices (..., 2): what the
    observation shows, float64; back (...,) or (n_rules, ...): ticker_rule_back.  Returns the env's action rows
    (choice0, choice1, fraction0, fraction1), float32 (..., 4), or (n_rules, ..., 4)."""
    cash, qty, prices = np.asarray(cash, np.float64), np.asarray(qty, np.float64), np.asarray(prices, np.float64)
    up0, up1, dn0, dn1, band, lb = _rule_columns(rules, cash.ndim)
    L = np.asarray(lb).astype(np.int64)
    p0, p1 = prices[..., 0], prices[..., 1]
    up = (L == 0) | (p0 >= np.asarray(back, np.float64))
    targets = (np.where(up, up0, dn0), np.where(up, up1, dn1))
    v0 = qty[..., 0] * p0
    v1 = qty[..., 1] * p1
    hold = v0 + v1
    total = cash + hold
    choices, fractions = [], []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for t, v in zip(targets, (v0, v1)):
            s = v / total
            lo = t - band
            hi = t + band
            buy = s < lo
            sell = ~buy & (s > hi)
            w = (t - s) * total
            fb = np.fmin(w / np.fmax(cash, 1e-12), 1.0)
            fs = np.fmin((s - t) / s, 1.0)
            choices.append(np.where(buy, 1.0, np.where(sell, 2.0, 0.0)))
            fractions.append(np.where(buy, fb, np.where(sell, fs, 0.0)))
    shape = np.broadcast(*(choices + fractions)).shape
    return np.stack([np.broadcast_to(a, shape) for a in choices + fractions], axis=-1).astype(np.float32)


def ticker_sweep(engine, rules, max_steps=None, trace_env=None):
    """Play every (env, rule) pair from the engine's CURRENT state for up to max_steps steps (default: the engine's
    max_episode_steps); the engine's state is left as it was.  rules: (n_rules, 6) of (up0, up1, dn0, dn1, band, lookback), played
    as float32.  Returns rules (float32, as played), total, sum_sq, final_assets (float64), min, max (float32), length, trades
    (int32), finished, depleted (uint8), each (n_rules, E), mean and std of the step rewards (float64), and with trace_env the
    steps of that env: trace_rewards (float32), trace_assets (float64), (n_rules, max_steps), and trace_actions (float32,
    (n_rules, max_steps, 4)), zero past the pair's length."""
    if engine.kind != _ffi.ENV_TICKER:
        raise ValueError("ticker_sweep: the engine is not a Ticker engine")
    lib = _ffi.load_library(extra_signatures=TICKER_SWEEP_SIGNATURES)
    r = check_ticker_rules(rules)
    max_steps, t_env = steps_and_trace(engine, "ticker_sweep", max_steps, trace_env)
    n_rules = r.shape[0]
    engine._check(lib.grl_ticker_sweep(engine.h, _ffi._ptr(r), n_rules, max_steps, t_env))
    out = {"rules": r}
    out.update(read_outputs(engine, lib.grl_ticker_sweep_read, _PAIR_DTYPES, (n_rules, engine.E)))
    if t_env >= 0:
        out.update(read_outputs(engine, lib.grl_ticker_sweep_read, _TRACE_DTYPES, (n_rules, max_steps)))
    with np.errstate(divide="ignore", invalid="ignore"):       # a pair at the end of its window plays no step: its moments are NaN
        out["mean"], out["std"] = reward_moments(out["total"], out["sum_sq"], out["length"])
    return out
