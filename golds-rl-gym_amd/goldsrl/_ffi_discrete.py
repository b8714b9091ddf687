"""ctypes binding of the A3C discrete savings-grid agent on the device (GridSolowWorker on DiscretePolicyEstimator; C ABI:
include/goldsrl_discretenet.h, greedy acting and evaluation: include/goldsrl_discreteeval.h)."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_a3c import STAT_NAMES, A3cNet  # noqa: F401

_P, _I, _F, _SZ = C.c_void_p, C.c_int32, C.c_float, C.c_size_t

SOLOW_SIZES = dict(static_size=2, temporal_size=2, num_outputs=1)


class GrlDnetConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rnn_length", C.c_int32), ("max_samples", C.c_int32), ("lr_decay_steps", C.c_int32),
                ("always_bootstrap", C.c_int32), ("num_choices", C.c_int32), ("scale", C.c_float), ("gamma", C.c_float),
                ("gae_lambda", C.c_float), ("clip_norm", C.c_float), ("rms_decay", C.c_float), ("rms_epsilon", C.c_float),
                ("lr_decay_rate", C.c_float), ("grid_lb", C.c_double), ("grid_ub", C.c_double)]


DNET_SIGNATURES = {
    "grl_dnet_config_default": (C.c_int, [C.POINTER(GrlDnetConfig)]),
    "grl_dnet_create": (C.c_int, [_P, C.POINTER(GrlDnetConfig), C.POINTER(_P)]),
    "grl_dnet_destroy": (C.c_int, [_P]),
    "grl_dnet_last_error": (C.c_char_p, [_P]),
    "grl_dnet_num_params": (C.c_int64, [_P]),
    "grl_dnet_set_params": (C.c_int, [_P, _P, C.c_int64]),
    "grl_dnet_get_params": (C.c_int, [_P, _P, C.c_int64]),
    "grl_dnet_get_grads": (C.c_int, [_P, _I, _P, C.c_int64]),
    "grl_dnet_get_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "grl_dnet_set_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64]),
    "grl_dnet_get_action_counter": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "grl_dnet_set_action_counter": (C.c_int, [_P, C.c_uint64]),
    "grl_dnet_predict": (C.c_int, [_P, _I, _P, _P, _P, _P]),
    "grl_dnet_train": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _F, _F, _I, _P]),
    "grl_dnet_rollout": (C.c_int, [_P, _I]),
    "grl_dnet_train_rollout": (C.c_int, [_P, _F, _P]),
    "grl_dnet_read_rollout": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}
# include/goldsrl_discreteeval.h: a dict of its own, as the header is a file of its own (tests/test_discrete_header.py pins both)
DNET_EVAL_SIGNATURES = {
    "grl_dnet_set_greedy": (C.c_int, [_P, _I]),
    "grl_dnet_eval": (C.c_int, [_P, _I, _I]),
    "grl_dnet_read_eval": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}


def discrete_param_shapes(K=51, static_size=2, temporal_size=2, H=32, S=128):
    """tf.trainable_variables() order: the trunk (the Gaussian net's first ten blocks), the probs tower, the value head."""
    X = 3 * H
    return [
        ("gru_gates_w", (temporal_size + H, 2 * H)), ("gru_gates_b", (2 * H,)), ("gru_cand_w", (temporal_size + H, H)), ("gru_cand_b", (H,)),
        ("temporal_w", (H, 2 * H)), ("temporal_b", (2 * H,)), ("static1_w", (static_size, 2 * H)), ("static1_b", (2 * H,)),
        ("static2_w", (2 * H, H)), ("static2_b", (H,)),
        ("probs1_w", (X, 2 * S)), ("probs1_b", (2 * S,)), ("probs2_w", (2 * S, S)), ("probs2_b", (S,)), ("probs3_w", (S, K)), ("probs3_b", (K,)),
        ("value1_w", (X, 2 * S)), ("value1_b", (2 * S,)), ("value2_w", (2 * S, 1)), ("value2_b", (1,)),
    ]


def default_init_discrete(seed=3, K=51):
    """TF's defaults: glorot-uniform kernels, zero biases; the GRU as default_init_gated does it (gate bias 1)."""
    rng = np.random.RandomState(seed)
    parts = []
    for name, shape in discrete_param_shapes(K):
        if name.endswith("_w"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            parts.append(rng.uniform(-lim, lim, size=shape).reshape(-1))
        elif name == "gru_gates_b":
            parts.append(np.ones(shape))
        else:
            parts.append(np.zeros(shape))
    return np.concatenate(parts).astype(np.float32)


class DiscreteNet(A3cNet):
    """The savings-grid agent on a Solow Engine: predict / train on host samples, device-resident rollout + update.  A choice is
    an index into grid = np.linspace(grid_lb, grid_ub, num_choices); the env is stepped with the grid value.  Greedy: the first
    index of the largest probability (GridSolowWorker.get_greedy_action's arg-max)."""
    PREFIX = "grl_dnet_"

    def __init__(self, engine, **kw):
        self._create(engine, dict(DNET_SIGNATURES, **DNET_EVAL_SIGNATURES), GrlDnetConfig(), kw)
        self.sizes = dict(SOLOW_SIZES)
        self.S0, self.D, self.K = 2, 2, int(self.cfg.num_choices)
        self.grid = np.linspace(self.cfg.grid_lb, self.cfg.grid_ub, self.K)

    def predict(self, states, windows):
        s = np.ascontiguousarray(states, np.float32)
        w = np.ascontiguousarray(windows, np.float32)
        n = s.shape[0]
        assert s.shape == (n, self.S0) and w.shape == (n, self.R, self.D), (s.shape, w.shape)
        probs, vals = np.empty((n, self.K), np.float32), np.empty(n, np.float32)
        self._check(self.lib.grl_dnet_predict(self.n, n, _ffi._ptr(s), _ffi._ptr(w), _ffi._ptr(probs), _ffi._ptr(vals)))
        return {"probs": probs, "values": vals}

    def train(self, states, windows, choices, adv, targets, weights=None, grad_mult=1.0, lr=1e-4, apply_update=True):
        s = np.ascontiguousarray(states, np.float32)
        n = s.shape[0]
        w = np.ascontiguousarray(windows, np.float32)
        ch = np.ascontiguousarray(np.asarray(choices).reshape(-1), np.int32)
        arrs = [np.ascontiguousarray(a, np.float32) for a in (adv, targets)]
        assert s.shape == (n, self.S0) and w.shape == (n, self.R, self.D) and ch.shape == (n,)
        assert arrs[0].shape == (n,) and arrs[1].shape == (n,)
        wt = None if weights is None else np.ascontiguousarray(weights, np.float32)
        return self._train(n, _ffi._ptr(s), _ffi._ptr(w), _ffi._ptr(ch), *[_ffi._ptr(a) for a in arrs], None if wt is None else _ffi._ptr(wt),
                           float(grad_mult), float(lr), 1 if apply_update else 0)

    def read_rollout(self, which):
        T, E, R, D = self.T, self.eng.E, self.R, self.D
        shapes = {"states": (T, E, self.S0), "windows": (T, E, R, D), "probs": (T, E, self.K), "choices": (T, E), "actions": (T, E),
                  "values": (T, E), "rewards": (T, E), "dones": (T, E), "weights": (T, E), "adv": (T, E), "targets": (T, E),
                  "term_values": (T, E), "term_states": (T, E, self.S0), "term_windows": (T, E, R, D), "boot": (E,)}
        return self._read("read_rollout", which, shapes[which])

    EVAL_TRACE = ("states", "choices", "actions", "rewards", "dones")

    def eval(self, max_steps, trace_steps=0, trace_fields=EVAL_TRACE):
        """Greedy episodes of every env from the engine's current state (reset it first), one kernel launch; the engine is reset
        afterwards.  Returns total_reward (E) float64, length (E) int32, finished (E) uint8 and, with trace_steps > 0, states
        (S,E,2), choices (S,E) int32, actions, rewards, dones (S,E) of the first S = min(trace_steps, steps played) steps, each
        defined up to its env's own end (trace_fields: the ones to read back)."""
        tails = {"states": (self.S0,), "choices": (), "actions": (), "rewards": (), "dones": ()}
        return self._eval(max_steps, trace_steps, trace_fields, tails)
