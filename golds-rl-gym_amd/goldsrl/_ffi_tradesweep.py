"""ctypes binding of the scripted trading-rule baseline sweep of the TradeAR1 env (C ABI: include/goldsrl_tradesweep.h): every
(env, rule) pair plays a whole episode in one kernel launch."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, reward_moments, steps_and_trace

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_tradesweep.h: a dict of its own, as the header is a file of its own (tests/test_trade_sweep_header.py pins both)
TRADE_SWEEP_SIGNATURES = {
    "grl_trade_sweep": (C.c_int, [_P, _P, _P, _I, _P, _I, _I]),
    "grl_trade_sweep_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

_PAIR_DTYPES = (("total", np.float64, ()), ("sum_sq", np.float64, ()), ("final_assets", np.float64, ()), ("min", np.float32, ()),
                ("max", np.float32, ()), ("length", np.int32, ()), ("finished", np.uint8, ()), ("depleted", np.uint8, ()))
_TRACE_DTYPES = (("trace_rewards", np.float32, ()), ("trace_assets", np.float64, ()))


def rule_actions(rules, prices):
    """The host form of the rule: clip(float64(bias) - float64(gain) * (p - 1.0), -1, 1) rounded to float32, one IEEE float64
    operation after the other -- the device's bits.  rules: (gain, bias) or (n_rules, 2); prices: float64, any shape.  Returns
    float32 of prices' shape, or (n_rules,) + that shape."""
    r = np.asarray(rules, np.float32).astype(np.float64)
    p = np.asarray(prices, np.float64)
    if r.ndim == 1:
        g, b = r
    else:
        g, b = r[:, 0].reshape((-1,) + (1,) * p.ndim), r[:, 1].reshape((-1,) + (1,) * p.ndim)
    return np.clip(b - g * (p - 1.0), -1.0, 1.0).astype(np.float32)


def trade_sweep(engine, rules, max_steps=None, trace_env=None, normals=None):
    """Play every (env, rule) pair from the engine's CURRENT state for up to max_steps steps (default: the engine's
    max_episode_steps); the engine's state is left as it was.  rules: (n_rules, 2) of (gain, bias), played as float32.  normals:
    None (the engine's own generator, at the counters its next steps would use) or a tape (max_steps, E, n_assets) whose row t
    moves the prices after step t.  Returns rules (float32, as played), total, sum_sq, final_assets (float64), min, max (float32),
    length (int32), finished, depleted (uint8), each (n_rules, E), mean and std of the step rewards (float64), and with trace_env
    the step rewards and the assets after every step of that env: trace_rewards (float32), trace_assets (float64),
    (n_rules, max_steps), zero past the pair's length."""
    if engine.kind != _ffi.ENV_TRADE:
        raise ValueError("trade_sweep: the engine is not a TradeAR1 engine")
    lib = _ffi.load_library(extra_signatures=TRADE_SWEEP_SIGNATURES)
    r = np.asarray(rules, np.float32)
    if r.ndim != 2 or r.shape[1] != 2 or r.shape[0] < 1:
        raise ValueError("trade_sweep: rules must be (n_rules, 2) of (gain, bias), got shape %s" % (r.shape,))
    if not np.isfinite(r).all():
        raise ValueError("trade_sweep: every gain and bias must be finite")
    gains, biases = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
    max_steps, t_env = steps_and_trace(engine, "trade_sweep", max_steps, trace_env)
    tape = None
    if normals is not None:
        tape = np.asarray(normals, np.float32)
        if tape.shape != (max_steps, engine.E, engine.cfg.n_assets):
            raise ValueError("trade_sweep: normals must be (max_steps, E, n_assets) = %s, got %s"
                             % ((max_steps, engine.E, engine.cfg.n_assets), tape.shape))
        tape = np.ascontiguousarray(tape.transpose(0, 2, 1))        # the device layout: a * E + env per step
    n_rules = r.shape[0]
    engine._check(lib.grl_trade_sweep(engine.h, _ffi._ptr(gains), _ffi._ptr(biases), n_rules, None if tape is None else _ffi._ptr(tape),
                                      max_steps, t_env))
    out = {"rules": np.stack([gains, biases], axis=1)}
    out.update(read_outputs(engine, lib.grl_trade_sweep_read, _PAIR_DTYPES, (n_rules, engine.E)))
    if t_env >= 0:
        out.update(read_outputs(engine, lib.grl_trade_sweep_read, _TRACE_DTYPES, (n_rules, max_steps)))
    out["mean"], out["std"] = reward_moments(out["total"], out["sum_sq"], out["length"])
    return out
