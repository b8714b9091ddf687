"""ctypes binding of the TradeAR1 env's foresight ceiling (C ABI: include/goldsrl_tradeforesight.h): every (env, horizon) pair plays a
whole episode in one call.  trade_foresight_actions is the host form of the recurrence, device-free."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, reward_moments, steps_and_trace

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_tradeforesight.h: a dict of its own, as the header is a file of its own (tests/test_trade_foresight_header.py pins
# both)
TRADE_FORESIGHT_SIGNATURES = {
    "grl_trade_foresight": (C.c_int, [_P, _P, _I, _P, _I, _I]),
    "grl_trade_foresight_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

MAX_HORIZONS = 64
MAX_HORIZON = 1023
MAX_PATH_CELLS = 1 << 28                    # max_steps * n_assets * E

_PAIR_DTYPES = (("total", np.float64, ()), ("sum_sq", np.float64, ()), ("final_assets", np.float64, ()), ("bound", np.float64, ()),
                ("min", np.float32, ()), ("max", np.float32, ()), ("length", np.int32, ()), ("trades", np.int32, ()),
                ("finished", np.uint8, ()), ("depleted", np.uint8, ()))


def check_trade_horizons(horizons):
    """horizons as the (n_horizons,) int32 array the device plays, or ValueError naming the offending index: the checks of
    grl_trade_foresight, device-free."""
    raw = np.asarray(horizons)
    if raw.ndim != 1 or raw.shape[0] < 1 or raw.shape[0] > MAX_HORIZONS:
        raise ValueError("horizons must be 1..%d values, got shape %s" % (MAX_HORIZONS, raw.shape))
    for i, v in enumerate(raw):
        if not np.isfinite(v) or v != np.floor(v) or v < 0 or v > MAX_HORIZON:
            raise ValueError("horizon %d is not 0 (the whole episode) or in 1..%d" % (i, MAX_HORIZON))
    return np.ascontiguousarray(raw.astype(np.int32))


def trade_foresight_last(max_steps, cap, elapsed):
    """The index of a pair's last step, depletion aside: m - 1 with m = min(max_steps, cap - elapsed (at least 1) if cap > 0).
    elapsed: (E,)."""
    elapsed = np.asarray(elapsed, np.int64)
    m = np.full(elapsed.shape, int(max_steps), np.int64)
    if cap > 0:
        m = np.minimum(m, np.maximum(int(cap) - elapsed, 1))
    return m - 1


def trade_foresight_coefficients(horizon, prices, t, last):
    """The recurrence of include/goldsrl_tradeforesight.h over the known rows of step t, vectorised over envs, one IEEE float64
    operation after the other -- the device's bits when prices is the device's path.  horizon: 0 (rows t..last) or H (rows
    t..min(t + H, last)); prices: (rows, n_assets, E) float64, the "prices" output; t: the step; last: (E,) or a number.  Returns
    A (E,) and B (n_assets, E) float64 before the trade of step t and the step's decisions (n_assets, E) int64: 0 hold, 1 buy,
    2 sell.  An env with last < t gets A = 1, B = its row t and holds."""
    p = np.asarray(prices, np.float64)
    n, E = p.shape[1], p.shape[2]
    t, H = int(t), int(horizon)
    last = np.broadcast_to(np.asarray(last, np.int64), (E,))
    e = last if H == 0 else np.minimum(t + H, last)
    span = e - t
    env = np.arange(E)
    A, B = np.ones(E), p[np.maximum(e, t), :, env].T.copy()
    dec = np.zeros((n, E), np.int64)
    nd = np.float64(n)
    with np.errstate(divide="ignore", invalid="ignore"):       # rows past an env's last step are zero and masked out
        for s in range(int(max(span.max(), -1)), -1, -1):
            on = s <= span
            row = p[t + np.where(on, s, 0), :, env].T          # (n, E)
            g = np.zeros(E)
            for a in range(n):
                x = B[a] / row[a]
                y = row[a] * A
                buy = x > A
                d = x - A
                g = np.where(buy, g + d, g)
                sell = y > B[a]
                B[a] = np.where(on & sell, y, B[a])
                dec[a] = np.where(on, np.where(sell, 2, np.where(buy, 1, 0)), dec[a])
            sh = g / nd
            A = np.where(on, A + sh, A)
    return A, B, dec


def trade_foresight_actions(horizon, prices, t, last):
    """The host form of the device's decision at step t: the env's action rows, float32 (E, n_assets) -- +1 buys asset a with
    cash / n of the cash the step begins with, -1 sells the whole holding, 0 holds.  The account is linear in (cash, q), so the
    decision depends on the prices alone.  An env with last < t holds."""
    dec = trade_foresight_coefficients(horizon, prices, t, last)[2]
    return np.where(dec == 1, 1.0, np.where(dec == 2, -1.0, 0.0)).T.astype(np.float32)


def trade_foresight_bound(cash, qty, assets, prices, last):
    """The "bound" output of a horizon-0 column on the host, in the device's operation order.  cash, assets: (E,); qty: (E, n)."""
    A, B, _ = trade_foresight_coefficients(0, prices, 0, last)
    qty = np.asarray(qty, np.float64)
    v = np.asarray(cash, np.float64) * A
    for a in range(B.shape[0]):
        w = qty[:, a] * B[a]
        v = v + w
    return np.log(v + 1e-4) - np.log(np.asarray(assets, np.float64) + 1e-4)


def trade_foresight(engine, horizons, max_steps=None, trace_env=None, normals=None):
    """Play every (env, horizon) pair from the engine's CURRENT state for up to max_steps steps (default: the engine's
    max_episode_steps); the engine's state is left as it was.  horizons: 0 (the whole episode is known) or 1..1023 rows known
    beyond the current one.  normals: None (the engine's own generator, at the counters its next steps would use) or a tape
    (max_steps, E, n_assets) whose row t moves the prices after step t.  Returns horizons (int32, as played), total, sum_sq,
    final_assets, bound (float64), min, max (float32), length, trades (int32), finished, depleted (uint8), each (n_horizons, E),
    mean and std of the step rewards (float64), prices (max_steps, n_assets, E) float64 -- the path every pair traded on, zero
    past an env's last step --, and with trace_env the steps of that env: trace_rewards (float32), trace_assets (float64),
    (n_horizons, max_steps), and trace_actions (float32, (n_horizons, max_steps, n_assets)), zero past the pair's length.  bound
    is the ceiling of total in a horizon-0 row, NaN in the others."""
    if engine.kind != _ffi.ENV_TRADE:
        raise ValueError("trade_foresight: the engine is not a TradeAR1 engine")
    lib = _ffi.load_library(extra_signatures=TRADE_FORESIGHT_SIGNATURES)
    hz = check_trade_horizons(horizons)
    max_steps, t_env = steps_and_trace(engine, "trade_foresight", max_steps, trace_env)
    n_assets = int(engine.cfg.n_assets)
    if max_steps * n_assets * engine.E > MAX_PATH_CELLS:
        raise ValueError("trade_foresight: max_steps * n_assets * E = %d is over the limit of %d (2^28) path cells"
                         % (max_steps * n_assets * engine.E, MAX_PATH_CELLS))
    tape = None
    if normals is not None:
        tape = np.asarray(normals, np.float32)
        if tape.shape != (max_steps, engine.E, n_assets):
            raise ValueError("trade_foresight: normals must be (max_steps, E, n_assets) = %s, got %s"
                             % ((max_steps, engine.E, n_assets), tape.shape))
        tape = np.ascontiguousarray(tape.transpose(0, 2, 1))        # the device layout: a * E + env per step
    n = hz.shape[0]
    engine._check(lib.grl_trade_foresight(engine.h, _ffi._ptr(hz), n, None if tape is None else _ffi._ptr(tape), max_steps, t_env))
    out = {"horizons": hz}
    out.update(read_outputs(engine, lib.grl_trade_foresight_read, _PAIR_DTYPES, (n, engine.E)))
    out.update(read_outputs(engine, lib.grl_trade_foresight_read, (("prices", np.float64, ()),), (max_steps, n_assets, engine.E)))
    if t_env >= 0:
        out.update(read_outputs(engine, lib.grl_trade_foresight_read,
                                (("trace_rewards", np.float32, ()), ("trace_assets", np.float64, ()), ("trace_actions", np.float32, (n_assets,))),
                                (n, max_steps)))
    out["mean"], out["std"] = reward_moments(out["total"], out["sum_sq"], out["length"])
    return out
