"""ctypes binding of the A3C discrete savings-grid agent on the device (GridSolowWorker on DiscretePolicyEstimator; C ABI:
include/goldsrl_discretenet.h, greedy acting and evaluation: include/goldsrl_discreteeval.h)."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_a3c import STAT_NAMES, A3cNet, signatures  # noqa: F401

SOLOW_SIZES = dict(static_size=2, temporal_size=2, num_outputs=1)


class GrlDnetConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rnn_length", C.c_int32), ("max_samples", C.c_int32), ("lr_decay_steps", C.c_int32),
                ("always_bootstrap", C.c_int32), ("num_choices", C.c_int32), ("scale", C.c_float), ("gamma", C.c_float),
                ("gae_lambda", C.c_float), ("clip_norm", C.c_float), ("rms_decay", C.c_float), ("rms_epsilon", C.c_float),
                ("lr_decay_rate", C.c_float), ("grid_lb", C.c_double), ("grid_ub", C.c_double)]


# include/goldsrl_discretenet.h's 17 training functions and include/goldsrl_discreteeval.h's three: a dict per header
# (tests/test_discrete_header.py pins both)
DNET_SIGNATURES, DNET_EVAL_SIGNATURES = signatures("grl_dnet_", GrlDnetConfig, predict=("probs", "values"),
                                                   train=("choices", "adv", "targets"))


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
        return self._predict(states, windows, (("probs", (self.K,)),))

    def train(self, states, windows, choices, adv, targets, weights=None, grad_mult=1.0, lr=1e-4, apply_update=True):
        heads = [(np.asarray(choices).reshape(-1), np.int32, ())]
        return self._train(states, windows, heads, adv, targets, weights, grad_mult, lr, apply_update)

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
