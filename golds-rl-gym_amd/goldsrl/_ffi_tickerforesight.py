"""ctypes binding of the Ticker env's foresight ceiling (C ABI: include/goldsrl_tickerforesight.h): every (env, horizon) pair plays a
whole episode in one kernel launch.  ticker_foresight_actions is the host form of the recurrence, device-free."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, reward_moments, steps_and_trace
from ._ffi_tickersweep import _PAIR_DTYPES, _TRACE_DTYPES, WINDOW

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_tickerforesight.h: a dict of its own, as the header is a file of its own (tests/test_ticker_foresight_header.py
# pins both)
TICKER_FORESIGHT_SIGNATURES = {
    "grl_ticker_foresight": (C.c_int, [_P, _P, _I, _I, _I]),
    "grl_ticker_foresight_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

MAX_HORIZONS = 64
SPREAD = 0.006
UP, DN = 1.0 + SPREAD, 1.0 - SPREAD       # as the env forms them (csrc/ticker_dev.h:ticker_account_step)


def check_ticker_horizons(horizons):
    """horizons as the (n_horizons,) int32 array the device plays, or ValueError naming the offending index: the checks of
    grl_ticker_foresight, device-free."""
    raw = np.asarray(horizons)
    if raw.ndim != 1 or raw.shape[0] < 1 or raw.shape[0] > MAX_HORIZONS:
        raise ValueError("horizons must be 1..%d values, got shape %s" % (MAX_HORIZONS, raw.shape))
    for i, v in enumerate(raw):
        if not np.isfinite(v) or v != np.floor(v) or v < 0 or v > WINDOW - 1:
            raise ValueError("horizon %d is not 0 (the whole episode) or in 1..1023" % i)
    return np.ascontiguousarray(raw.astype(np.int32))


def ticker_foresight_last(max_steps, cap, elapsed, idx):
    """The row of a pair's last step, depletion aside: idx + n - 1 with n = min(max_steps, cap - elapsed (at least 1) if cap > 0,
    1023 - idx).  elapsed, idx: (E,).  last < idx: the pair plays no step."""
    idx, elapsed = np.asarray(idx, np.int64), np.asarray(elapsed, np.int64)
    n = np.minimum(int(max_steps), WINDOW - 1 - idx)
    if cap > 0:
        n = np.minimum(n, np.maximum(int(cap) - elapsed, 1))
    return idx + n - 1


def ticker_foresight_coefficients(horizon, table, start, idx, last):
    """The recurrence of include/goldsrl_tickerforesight.h over the known rows of the step at row idx, vectorised over envs, one IEEE
    float64 operation after the other -- the device's bits.  horizon: 0 (rows idx..last) or H (rows idx..min(idx + H, last));
    start, idx, last: (E,).  Returns A, B0, B1 (E,) float64 before the trade of row idx and the row's decision code
    choice0 | choice1 << 2 (E,) int64.  An env with last < idx gets A = 1, B = the prices of row idx and code 0."""
    table = np.asarray(table, np.float64)
    start, idx, last = np.asarray(start, np.int64), np.asarray(idx, np.int64), np.asarray(last, np.int64)
    H = int(horizon)
    e = last if H == 0 else np.minimum(idx + H, last)
    span = e - idx
    top = table[start + np.maximum(e, idx)]
    A, B0, B1 = np.ones(len(idx)), top[:, 0].copy(), top[:, 1].copy()
    code = np.zeros(len(idx), np.int64)
    for s in range(int(max(span.max(), -1)), -1, -1):
        on = s <= span
        row = table[start + idx + np.where(on, s, 0)]
        p0, p1 = row[:, 0], row[:, 1]
        a0 = p0 * UP
        a1 = p1 * UP
        x0 = B0 / a0
        x1 = B1 / a1
        b0 = p0 * DN
        b1 = p1 * DN
        y0 = b0 * A
        y1 = b1 * A
        An = A
        buy0 = x0 > An
        An = np.where(buy0, x0, An)
        buy1 = x1 > An
        An = np.where(buy1, x1, An)
        sell0 = y0 > B0
        sell1 = y1 > B1
        c0 = np.where(buy0 & ~buy1, 1, np.where(sell0, 2, 0))
        c1 = np.where(buy1, 1, np.where(sell1, 2, 0))
        A = np.where(on, An, A)
        B0 = np.where(on & sell0, y0, B0)
        B1 = np.where(on & sell1, y1, B1)
        code = np.where(on, c0 | (c1 << 2), code)
    return A, B0, B1, code


def ticker_foresight_actions(horizon, cash, qty, table, start, idx, last):
    """The host form of the device's decision at the step of row idx: the env's action rows (choice0, choice1, fraction0,
    fraction1), float32 (E, 4) -- a buy or a sale is always of everything, fraction 1.  cash (E,) and qty (E, 2) are what the
    observation shows; the account arithmetic is linear in them, so the decision does not depend on them, and they are only checked
    for their shapes.  An env with last < idx holds."""
    cash, qty = np.asarray(cash, np.float64), np.asarray(qty, np.float64)
    if cash.shape != np.shape(idx) or qty.shape != cash.shape + (2,):
        raise ValueError("cash must be (E,) and qty (E, 2) for idx (E,)")
    code = ticker_foresight_coefficients(horizon, table, start, idx, last)[3]
    c0, c1 = code & 3, code >> 2
    return np.stack([c0, c1, c0 != 0, c1 != 0], axis=-1).astype(np.float32)


def ticker_foresight_bound(cash, qty, assets, table, start, idx, last):
    """The "bound" output of a horizon-0 column on the host, in the device's operation order."""
    A, B0, B1, _ = ticker_foresight_coefficients(0, table, start, idx, last)
    cash, qty = np.asarray(cash, np.float64), np.asarray(qty, np.float64)
    vc = cash * A
    v0 = qty[:, 0] * B0
    v1 = qty[:, 1] * B1
    vs = vc + v0
    v = vs + v1
    return np.log(v + 1e-4) - np.log(np.asarray(assets, np.float64) + 1e-4)


def ticker_foresight(engine, horizons, max_steps=None, trace_env=None):
    """Play every (env, horizon) pair from the engine's CURRENT state for up to max_steps steps (default: the engine's
    max_episode_steps); the engine's state is left as it was.  horizons: 0 (the whole episode is known) or 1..1023 rows known
    beyond the current one.  Returns horizons (int32, as played), total, sum_sq, final_assets, bound (float64), min, max (float32),
    length, trades (int32), finished, depleted (uint8), each (n_horizons, E), mean and std of the step rewards (float64), and with
    trace_env the steps of that env: trace_rewards (float32), trace_assets (float64), (n_horizons, max_steps), and trace_actions
    (float32, (n_horizons, max_steps, 4)), zero past the pair's length.  bound is the ceiling of total in a horizon-0 row, NaN in
    the others."""
    if engine.kind != _ffi.ENV_TICKER:
        raise ValueError("ticker_foresight: the engine is not a Ticker engine")
    lib = _ffi.load_library(extra_signatures=TICKER_FORESIGHT_SIGNATURES)
    hz = check_ticker_horizons(horizons)
    max_steps, t_env = steps_and_trace(engine, "ticker_foresight", max_steps, trace_env)
    n = hz.shape[0]
    engine._check(lib.grl_ticker_foresight(engine.h, _ffi._ptr(hz), n, max_steps, t_env))
    out = {"horizons": hz}
    out.update(read_outputs(engine, lib.grl_ticker_foresight_read, _PAIR_DTYPES + (("bound", np.float64, ()),), (n, engine.E)))
    if t_env >= 0:
        out.update(read_outputs(engine, lib.grl_ticker_foresight_read, _TRACE_DTYPES, (n, max_steps)))
    with np.errstate(divide="ignore", invalid="ignore"):       # a pair at the end of its window plays no step: its moments are NaN
        out["mean"], out["std"] = reward_moments(out["total"], out["sum_sq"], out["length"])
    return out
