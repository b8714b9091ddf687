"""ctypes binding of the constant-savings baseline sweep of the Solow env (C ABI: include/goldsrl_sweep.h): every (env, rate) pair
plays a whole episode in one kernel launch."""
import ctypes as C

import numpy as np

from . import _ffi

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_sweep.h: a dict of its own, as the header is a file of its own (tests/test_sweep_header.py pins both)
SWEEP_SIGNATURES = {
    "grl_solow_sweep": (C.c_int, [_P, _P, _I, _I, _I]),
    "grl_solow_sweep_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

_PAIR_DTYPES = (("total", np.float64), ("sum_sq", np.float64), ("min", np.float32), ("max", np.float32), ("length", np.int32),
                ("finished", np.uint8))


def reward_moments(total, sum_sq, length):
    """mean = total / length and std = sqrt(max(sum_sq / length - mean**2, 0)) of the step rewards (np.std's population form)."""
    n = np.asarray(length, np.float64)
    mean = np.asarray(total, np.float64) / n
    std = np.sqrt(np.maximum(np.asarray(sum_sq, np.float64) / n - mean ** 2, 0.0))
    return mean, std


def solow_sweep(engine, rates, max_steps=None, trace_env=None):
    """Play every (env, rate) pair from the engine's CURRENT state (reset it first) for up to max_steps steps (default: the
    engine's max_episode_steps); the engine's state is left as it was.  Returns rates (float32, as played), total, sum_sq (float64),
    min, max (float32), length (int32), finished (uint8), each (n_rates, E), mean and std of the step rewards (float64), and with
    trace_env the step rewards and the capital after every step of that env: trace_rewards, trace_k (n_rates, max_steps)."""
    if engine.kind != _ffi.ENV_SOLOW:
        raise ValueError("solow_sweep: the engine is not a Solow engine")
    lib = _ffi.load_library(extra_signatures=SWEEP_SIGNATURES)
    r = np.ascontiguousarray(np.asarray(rates, np.float64).reshape(-1), np.float32)
    if max_steps is None:
        max_steps = int(engine.cfg.max_episode_steps)
    if max_steps < 1:
        raise ValueError("solow_sweep: max_steps must be at least 1 (an engine without a TimeLimit has no default)")
    t_env = -1 if trace_env is None else int(trace_env)
    engine._check(lib.grl_solow_sweep(engine.h, _ffi._ptr(r), r.size, int(max_steps), t_env))
    out = {"rates": r}
    for name, dt in _PAIR_DTYPES:
        a = np.empty((r.size, engine.E), dt)
        engine._check(lib.grl_solow_sweep_read(engine.h, name.encode(), _ffi._ptr(a), a.nbytes))
        out[name] = a
    if t_env >= 0:
        for name in ("trace_rewards", "trace_k"):
            a = np.empty((r.size, int(max_steps)), np.float32)
            engine._check(lib.grl_solow_sweep_read(engine.h, name.encode(), _ffi._ptr(a), a.nbytes))
            out[name] = a
    out["mean"], out["std"] = reward_moments(out["total"], out["sum_sq"], out["length"])
    return out
