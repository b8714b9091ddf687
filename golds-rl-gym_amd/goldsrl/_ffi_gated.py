"""ctypes binding of the Ticker gated trader on the device (C ABI: include/goldsrl_gatednet.h)."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_a3c import STAT_NAMES, A3cNet, signatures  # noqa: F401

N_ASSETS, N_CHOICES, STATIC_SIZE, TEMPORAL_SIZE = 2, 3, 7, 4


class GrlGnetConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rnn_length", C.c_int32), ("max_samples", C.c_int32), ("lr_decay_steps", C.c_int32),
                ("scale", C.c_float), ("gamma", C.c_float), ("gae_lambda", C.c_float), ("clip_norm", C.c_float),
                ("rms_decay", C.c_float), ("rms_epsilon", C.c_float), ("lr_decay_rate", C.c_float)]


# include/goldsrl_gatednet.h's 17 training functions and include/goldsrl_gatedeval.h's three: a dict per header (pinned by
# tests/test_gated_eval_header.py)
GNET_SIGNATURES, GNET_EVAL_SIGNATURES = signatures("grl_gnet_", GrlGnetConfig, predict=("probs", "mu", "sigma", "values"),
                                                   train=("choices", "raw", "adv", "targets"))


def gated_param_shapes(static_size=STATIC_SIZE, temporal_size=TEMPORAL_SIZE, H=32, S=128):
    """tf.trainable_variables() order: the trunk (the flat net's first ten blocks), the class tower, the normal tower, the value head."""
    X = 3 * H
    return [
        ("gru_gates_w", (temporal_size + H, 2 * H)), ("gru_gates_b", (2 * H,)), ("gru_cand_w", (temporal_size + H, H)), ("gru_cand_b", (H,)),
        ("temporal_w", (H, 2 * H)), ("temporal_b", (2 * H,)), ("static1_w", (static_size, 2 * H)), ("static1_b", (2 * H,)),
        ("static2_w", (2 * H, H)), ("static2_b", (H,)),
        ("class1_w", (X, 2 * S)), ("class1_b", (2 * S,)), ("class2_w", (2 * S, S)), ("class2_b", (S,)),
        ("class3_w", (S, N_ASSETS * N_CHOICES)), ("class3_b", (N_ASSETS * N_CHOICES,)),
        ("normal1_w", (X, 2 * S)), ("normal1_b", (2 * S,)), ("normal2_w", (2 * S, S)), ("normal2_b", (S,)),
        ("normal3_w", (S, N_ASSETS * N_CHOICES * 2)), ("normal3_b", (N_ASSETS * N_CHOICES * 2,)),
        ("value1_w", (X, 2 * S)), ("value1_b", (2 * S,)), ("value2_w", (2 * S, 1)), ("value2_b", (1,)),
    ]


def default_init_gated(seed=3):
    """flat_init's rule: glorot-uniform kernels, zero biases, GRU gate bias 1."""
    rng = np.random.RandomState(seed)
    parts = []
    for name, shape in gated_param_shapes():
        if name.endswith("_w"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            parts.append(rng.uniform(-lim, lim, size=shape).reshape(-1))
        elif name == "gru_gates_b":
            parts.append(np.ones(shape))
        else:
            parts.append(np.zeros(shape))
    return np.concatenate(parts).astype(np.float32)


class GatedNet(A3cNet):
    """The gated trader on a Ticker Engine: predict / train on host samples, device-resident rollout + update.  Greedy: per asset the
    choice is the first argmax of the float32 probs, raw = mu[choice]."""
    PREFIX = "grl_gnet_"

    S0, D = STATIC_SIZE, TEMPORAL_SIZE

    def __init__(self, engine, **kw):
        self._create(engine, dict(GNET_SIGNATURES, **GNET_EVAL_SIGNATURES), GrlGnetConfig(), kw)

    def predict(self, states, windows):
        return self._predict(states, windows, tuple((k, (N_ASSETS, N_CHOICES)) for k in ("probs", "mu", "sigma")))

    def train(self, states, windows, choices, raw, adv, targets, weights=None, grad_mult=1.0, lr=1e-4, apply_update=True):
        heads = [(choices, np.int32, (N_ASSETS,)), (raw, np.float32, (N_ASSETS,))]
        return self._train(states, windows, heads, adv, targets, weights, grad_mult, lr, apply_update)

    def read_rollout(self, which):
        T, E, R = self.T, self.eng.E, self.R
        shapes = {"states": (T, E, STATIC_SIZE), "windows": (T, E, R, TEMPORAL_SIZE), "choices": (T, E, N_ASSETS), "raw": (T, E, N_ASSETS),
                  "probs": (T, E, N_ASSETS, N_CHOICES), "mu": (T, E, N_ASSETS, N_CHOICES), "sigma": (T, E, N_ASSETS, N_CHOICES),
                  "values": (T, E), "rewards": (T, E), "dones": (T, E), "weights": (T, E), "adv": (T, E), "targets": (T, E),
                  "actions": (T, E, 2 * N_ASSETS), "boot": (E,)}
        return self._read("read_rollout", which, shapes[which])

    EVAL_TRACE = ("states", "probs", "mu", "choices", "actions", "rewards", "dones")

    def eval(self, max_steps, trace_steps=0, trace_fields=EVAL_TRACE):
        """Greedy episodes of every env from the engine's current state (reset it first), one kernel launch; the engine is reset
        afterwards.  Returns total_reward (E) float64, length (E) int32, finished (E) uint8 and, with trace_steps > 0, states (S,E,7),
        probs, mu (S,E,2,3), choices (S,E,2) int32, actions (S,E,4), rewards, dones (S,E) of the first S = min(trace_steps, steps
        played) steps, each defined up to its env's own end (trace_fields: the ones to read back)."""
        tails = {"states": (STATIC_SIZE,), "probs": (N_ASSETS, N_CHOICES), "mu": (N_ASSETS, N_CHOICES), "choices": (N_ASSETS,),
                 "actions": (2 * N_ASSETS,), "rewards": (), "dones": ()}
        return self._eval(max_steps, trace_steps, trace_fields, tails)
