"""What the bindings of the whole-episode launches (_ffi_sweep, _ffi_tradesweep, _ffi_tradeforesight, _ffi_tickersweep,
_ffi_tickerforesight, _ffi_solowdp, _ffi_replay, _ffi_swarmrules, _ffi_swarmplan, _ffi_swarmsearch, _ffi_swarmcemplan, _ffi_tickersearch, _ffi_tradesearch) do alike: the max_steps default and its refusal, trace_env as the C side takes it, the read-back
of a table of outputs, and the moments of the step rewards.  Nothing here loads the library."""
import numpy as np

from . import _ffi


def steps_and_trace(engine, fn_name, max_steps, trace_env=None):
    """(max_steps, t_env) as the C call takes them: max_steps defaults to the engine's max_episode_steps and is refused below 1,
    trace_env None becomes -1."""
    if max_steps is None:
        max_steps = int(engine.cfg.max_episode_steps)
    if max_steps < 1:
        raise ValueError("%s: max_steps must be at least 1 (an engine without a TimeLimit has no default)" % fn_name)
    return int(max_steps), -1 if trace_env is None else int(trace_env)


def read_outputs(engine, read_fn, specs, lead_shape):
    """{name: array} of the outputs in specs, rows of (name, dtype, inner_shape): each an np.empty of lead_shape + inner_shape
    filled by one read_fn(handle, name, pointer, nbytes) call (a grl_*_read)."""
    out = {}
    for name, dt, inner in specs:
        a = np.empty(tuple(lead_shape) + tuple(inner), dt)
        engine._check(read_fn(engine.h, name.encode(), _ffi._ptr(a), a.nbytes))
        out[name] = a
    return out


def reward_moments(total, sum_sq, length):
    """mean = total / length and std = sqrt(max(sum_sq / length - mean**2, 0)) of the step rewards (np.std's population form)."""
    n = np.asarray(length, np.float64)
    mean = np.asarray(total, np.float64) / n
    std = np.sqrt(np.maximum(np.asarray(sum_sq, np.float64) / n - mean ** 2, 0.0))
    return mean, std
