"""ctypes binding of the A3C grid trader on the device (DiscretePolicyEstimator with num_outputs = 2 on a 2-asset TradeAR1 engine;
C ABI, greedy acting and evaluation: include/goldsrl_gridtradenet.h)."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_a3c import STAT_NAMES, A3cNet, signatures  # noqa: F401

TRADE_SIZES = dict(static_size=5, temporal_size=5, num_outputs=2)       # 2 assets
K_MAX = 48


class GrlGtnetConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rnn_length", C.c_int32), ("max_samples", C.c_int32), ("lr_decay_steps", C.c_int32),
                ("always_bootstrap", C.c_int32), ("num_choices", C.c_int32), ("num_outputs", C.c_int32), ("scale", C.c_float),
                ("gamma", C.c_float), ("gae_lambda", C.c_float), ("clip_norm", C.c_float), ("rms_decay", C.c_float),
                ("rms_epsilon", C.c_float), ("lr_decay_rate", C.c_float), ("grid_lb", C.c_double), ("grid_ub", C.c_double)]


# include/goldsrl_gridtradenet.h's 17 training functions and its three of the evaluation
GTNET_SIGNATURES, GTNET_EVAL_SIGNATURES = signatures("grl_gtnet_", GrlGtnetConfig, predict=("probs", "values"),
                                                     train=("choices", "adv", "targets"))


def gridtrade_param_shapes(K=17, static_size=5, temporal_size=5, num_outputs=2, H=32, S=128):
    """tf.trainable_variables() order: the trunk (the Gaussian net's first ten blocks), the probs tower whose last layer has
    num_outputs * K columns (column o * K + j: output o, choice j), the value head."""
    X = 3 * H
    return [
        ("gru_gates_w", (temporal_size + H, 2 * H)), ("gru_gates_b", (2 * H,)), ("gru_cand_w", (temporal_size + H, H)), ("gru_cand_b", (H,)),
        ("temporal_w", (H, 2 * H)), ("temporal_b", (2 * H,)), ("static1_w", (static_size, 2 * H)), ("static1_b", (2 * H,)),
        ("static2_w", (2 * H, H)), ("static2_b", (H,)),
        ("probs1_w", (X, 2 * S)), ("probs1_b", (2 * S,)), ("probs2_w", (2 * S, S)), ("probs2_b", (S,)),
        ("probs3_w", (S, num_outputs * K)), ("probs3_b", (num_outputs * K,)),
        ("value1_w", (X, 2 * S)), ("value1_b", (2 * S,)), ("value2_w", (2 * S, 1)), ("value2_b", (1,)),
    ]


def default_init_gridtrade(seed=3, K=17):
    """TF's defaults: glorot-uniform kernels, zero biases; the GRU as default_init_gated does it (gate bias 1)."""
    rng = np.random.RandomState(seed)
    parts = []
    for name, shape in gridtrade_param_shapes(K):
        if name.endswith("_w"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            parts.append(rng.uniform(-lim, lim, size=shape).reshape(-1))
        elif name == "gru_gates_b":
            parts.append(np.ones(shape))
        else:
            parts.append(np.zeros(shape))
    return np.concatenate(parts).astype(np.float32)


class GridTradeNet(A3cNet):
    """The grid trader on a 2-asset TradeAR1 Engine: predict / train on host samples, device-resident rollout + update, one-launch
    greedy evaluation.  A choice is, per asset, an index into grid = np.linspace(grid_lb, grid_ub, num_choices) (default 17 points
    on [-1, 1]); the env is stepped with the two grid values.  Greedy: per asset the first index of the largest probability."""
    PREFIX = "grl_gtnet_"

    def __init__(self, engine, **kw):
        self._create(engine, dict(GTNET_SIGNATURES, **GTNET_EVAL_SIGNATURES), GrlGtnetConfig(), kw)
        self.sizes = dict(TRADE_SIZES)
        self.S0, self.D, self.O, self.K = 5, 5, int(self.cfg.num_outputs), int(self.cfg.num_choices)
        self.grid = np.linspace(self.cfg.grid_lb, self.cfg.grid_ub, self.K)

    def predict(self, states, windows):
        return self._predict(states, windows, (("probs", (self.O, self.K)),))

    def train(self, states, windows, choices, adv, targets, weights=None, grad_mult=1.0, lr=1e-4, apply_update=True):
        return self._train(states, windows, [(choices, np.int32, (self.O,))], adv, targets, weights, grad_mult, lr, apply_update)

    def read_rollout(self, which):
        T, E, R, D, O = self.T, self.eng.E, self.R, self.D, self.O
        shapes = {"states": (T, E, self.S0), "windows": (T, E, R, D), "probs": (T, E, O, self.K), "choices": (T, E, O), "actions": (T, E, O),
                  "values": (T, E), "rewards": (T, E), "dones": (T, E), "weights": (T, E), "adv": (T, E), "targets": (T, E), "boot": (E,)}
        return self._read("read_rollout", which, shapes[which])

    EVAL_TRACE = ("states", "choices", "actions", "rewards", "dones")

    def eval(self, max_steps, trace_steps=0, trace_fields=EVAL_TRACE):
        """Greedy episodes of every env from the engine's current state (reset it first), one kernel launch; the engine is reset
        afterwards.  Returns total_reward (E) float64, length (E) int32, finished (E) uint8 and, with trace_steps > 0, states
        (S,E,5), choices (S,E,O) int32, actions (S,E,O), rewards, dones (S,E) of the first S = min(trace_steps, steps played) steps,
        each defined up to its env's own end (trace_fields: the ones to read back)."""
        tails = {"states": (self.S0,), "choices": (self.O,), "actions": (self.O,), "rewards": (), "dones": ()}
        return self._eval(max_steps, trace_steps, trace_fields, tails)
