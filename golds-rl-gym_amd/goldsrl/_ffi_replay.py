"""ctypes binding of the scripted-episode replay of the Swarm env (C ABI: include/goldsrl_replay.h): every (env, action sequence)
pair plays its whole script in one kernel launch."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_replay.h: a dict of its own, as the header is a file of its own (tests/test_replay_header.py pins both)
REPLAY_SIGNATURES = {
    "grl_swarm_replay": (C.c_int, [_P, _P, _I, _I, _I, _P, _I, _I]),
    "grl_swarm_replay_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}


def swarm_replay(eng, actions, seq_len=None, trace_env=-1):
    """Play every (env, sequence) pair from the engine's CURRENT state (reset it first); the engine's state is left as it was.

    actions: (n_seq, T, 10, 2) rows shared by every env, or (E, n_seq, T, 10, 2) rows of each env's own.  float64 rows are
    stepped as SwarmEnv.step steps a direct caller's, float32 rows with the worker's float32 wind / dt arithmetic (quirk Q7);
    any other dtype raises.  seq_len: n_seq lengths in 1..T (default: all T).  A pair ends after the step whose reward is >= 0
    or that reaches the engine's TimeLimit (finished = 1), or when its script runs out.

    Returns rewards (E, n_seq, T) float64, zero past the pair's length, length (E, n_seq) int32, finished (E, n_seq) uint8 and,
    with trace_env >= 0, the positions after every step of that env: trace_x (n_seq, T, 80, 2), trace_xa (n_seq, T, 10, 2)."""
    if eng.kind != _ffi.ENV_SWARM:
        raise ValueError("swarm_replay: the engine is not a Swarm engine")
    a = np.asarray(actions)
    if a.dtype not in (np.float32, np.float64):
        raise TypeError("swarm_replay: actions must be float32 or float64 (the dtype selects the step's arithmetic), got %s" % a.dtype)
    if a.ndim not in (4, 5) or a.shape[-2:] != (10, 2) or (a.ndim == 5 and a.shape[0] != eng.E):
        raise ValueError("swarm_replay: actions must be (n_seq, T, 10, 2) or (%d, n_seq, T, 10, 2), got %s" % (eng.E, a.shape))
    a = np.ascontiguousarray(a)
    per_env = a.ndim == 5
    n_seq, T = (int(v) for v in a.shape[-4:-2])
    lens = None
    if seq_len is not None:
        lens = np.ascontiguousarray(seq_len, np.int32).reshape(-1)
        if lens.size != n_seq:
            raise ValueError("swarm_replay: seq_len needs %d values, got %d" % (n_seq, lens.size))
    t_env = -1 if trace_env is None else int(trace_env)
    lib = _ffi.load_library(extra_signatures=REPLAY_SIGNATURES)
    eng._check(lib.grl_swarm_replay(eng.h, _ffi._ptr(a), 1 if a.dtype == np.float64 else 0, n_seq, T,
                                    None if lens is None else _ffi._ptr(lens), 1 if per_env else 0, t_env))
    out = read_outputs(eng, lib.grl_swarm_replay_read, (("rewards", np.float64, (T,)), ("length", np.int32, ()), ("finished", np.uint8, ())),
                       (eng.E, n_seq))
    if t_env >= 0:
        out.update(read_outputs(eng, lib.grl_swarm_replay_read, (("trace_x", np.float64, (80, 2)), ("trace_xa", np.float64, (10, 2))), (n_seq, T)))
    return out
