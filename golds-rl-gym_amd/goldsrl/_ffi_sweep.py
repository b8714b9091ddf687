"""ctypes binding of the constant-savings baseline sweep of the Solow env (C ABI: include/goldsrl_sweep.h): every (env, rate) pair
plays a whole episode in one kernel launch."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, reward_moments, steps_and_trace      # reward_moments: imported from here by name

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_sweep.h: a dict of its own, as the header is a file of its own (tests/test_sweep_header.py pins both)
SWEEP_SIGNATURES = {
    "grl_solow_sweep": (C.c_int, [_P, _P, _I, _I, _I]),
    "grl_solow_sweep_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

_PAIR_DTYPES = (("total", np.float64, ()), ("sum_sq", np.float64, ()), ("min", np.float32, ()), ("max", np.float32, ()),
                ("length", np.int32, ()), ("finished", np.uint8, ()))
_TRACE_DTYPES = (("trace_rewards", np.float32, ()), ("trace_k", np.float32, ()))


def solow_sweep(engine, rates, max_steps=None, trace_env=None):
    """Play every (env, rate) pair from the engine's CURRENT state (reset it first) for up to max_steps steps (default: the
    engine's max_episode_steps); the engine's state is left as it was.  Returns rates (float32, as played), total, sum_sq (float64),
    min, max (float32), length (int32), finished (uint8), each (n_rates, E), mean and std of the step rewards (float64), and with
    trace_env the step rewards and the capital after every step of that env: trace_rewards, trace_k (n_rates, max_steps)."""
    if engine.kind != _ffi.ENV_SOLOW:
        raise ValueError("solow_sweep: the engine is not a Solow engine")
    lib = _ffi.load_library(extra_signatures=SWEEP_SIGNATURES)
    r = np.ascontiguousarray(np.asarray(rates, np.float64).reshape(-1), np.float32)
    max_steps, t_env = steps_and_trace(engine, "solow_sweep", max_steps, trace_env)
    engine._check(lib.grl_solow_sweep(engine.h, _ffi._ptr(r), r.size, max_steps, t_env))
    out = {"rates": r}
    out.update(read_outputs(engine, lib.grl_solow_sweep_read, _PAIR_DTYPES, (r.size, engine.E)))
    if t_env >= 0:
        out.update(read_outputs(engine, lib.grl_solow_sweep_read, _TRACE_DTYPES, (r.size, max_steps)))
    out["mean"], out["std"] = reward_moments(out["total"], out["sum_sq"], out["length"])
    return out
