"""ctypes binding of the A3C Gaussian agent on the device (SolowWorker / TradeWorker; C ABI: include/goldsrl_gaussnet.h)."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_a3c import STAT_NAMES, A3cNet, signatures  # noqa: F401

SOLOW_SIZES = dict(static_size=2, temporal_size=2, num_actions=1)       # scripts/train_solow.py:40-42
TRADE_SIZES = dict(static_size=5, temporal_size=5, num_actions=2)       # scripts/train_trade.py (2 assets)


class GrlAnetConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rnn_length", C.c_int32), ("max_samples", C.c_int32), ("lr_decay_steps", C.c_int32),
                ("always_bootstrap", C.c_int32), ("scale", C.c_float), ("gamma", C.c_float), ("gae_lambda", C.c_float),
                ("clip_norm", C.c_float), ("rms_decay", C.c_float), ("rms_epsilon", C.c_float), ("lr_decay_rate", C.c_float)]


# include/goldsrl_gaussnet.h's 17 training functions and include/goldsrl_gausseval.h's three: a dict per header (pinned by
# tests/test_gauss_eval_header.py)
ANET_SIGNATURES, ANET_EVAL_SIGNATURES = signatures("grl_anet_", GrlAnetConfig, predict=("mu", "sigma", "values"),
                                                   train=("raw", "adv", "targets"))


def gauss_param_shapes(static_size=2, temporal_size=2, num_actions=1, H=32, S=128):
    """tf.trainable_variables() order of scripts/train_solow.py:63-73: the trunk (the flat net's first ten blocks), the mu tower, the
    sigma tower, the value head."""
    X = 3 * H
    return [
        ("gru_gates_w", (temporal_size + H, 2 * H)), ("gru_gates_b", (2 * H,)), ("gru_cand_w", (temporal_size + H, H)), ("gru_cand_b", (H,)),
        ("temporal_w", (H, 2 * H)), ("temporal_b", (2 * H,)), ("static1_w", (static_size, 2 * H)), ("static1_b", (2 * H,)),
        ("static2_w", (2 * H, H)), ("static2_b", (H,)),
        ("mu1_w", (X, 2 * S)), ("mu1_b", (2 * S,)), ("mu2_w", (2 * S, S)), ("mu2_b", (S,)), ("mu3_w", (S, num_actions)), ("mu3_b", (num_actions,)),
        ("sigma1_w", (X, 2 * S)), ("sigma1_b", (2 * S,)), ("sigma2_w", (2 * S, S)), ("sigma2_b", (S,)),
        ("sigma3_w", (S, num_actions)), ("sigma3_b", (num_actions,)),
        ("value1_w", (X, 2 * S)), ("value1_b", (2 * S,)), ("value2_w", (2 * S, 1)), ("value2_b", (1,)),
    ]


def default_init_gauss(seed=3, static_size=2, temporal_size=2, num_actions=1):
    """TF's defaults: glorot-uniform kernels, zero biases; the sigma3 bias at -1 (a3c/estimators.py:289); the GRU as
    default_init_gated does it (gate bias 1)."""
    rng = np.random.RandomState(seed)
    parts = []
    for name, shape in gauss_param_shapes(static_size, temporal_size, num_actions):
        if name.endswith("_w"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            parts.append(rng.uniform(-lim, lim, size=shape).reshape(-1))
        elif name == "gru_gates_b":
            parts.append(np.ones(shape))
        elif name == "sigma3_b":
            parts.append(-np.ones(shape))
        else:
            parts.append(np.zeros(shape))
    return np.concatenate(parts).astype(np.float32)


class GaussNet(A3cNet):
    """The Gaussian agent on a Solow or 2-asset TradeAR1 Engine: predict / train on host samples, device-resident rollout + update.
    always_bootstrap defaults to what the engine's env takes (Solow 1, TradeAR1 0).  Greedy: raw = mu
    (run_n_steps(stochastic=False), a3c/worker.py:180-230)."""
    PREFIX = "grl_anet_"

    def __init__(self, engine, **kw):
        kw.setdefault("always_bootstrap", 1 if engine.kind == _ffi.ENV_SOLOW else 0)
        self._create(engine, dict(ANET_SIGNATURES, **ANET_EVAL_SIGNATURES), GrlAnetConfig(), kw)
        self.sizes = dict(SOLOW_SIZES if engine.kind == _ffi.ENV_SOLOW else TRADE_SIZES)
        self.S0, self.D, self.A = self.sizes["static_size"], self.sizes["temporal_size"], self.sizes["num_actions"]

    def predict(self, states, windows):
        return self._predict(states, windows, (("mu", (self.A,)), ("sigma", (self.A,))))

    def train(self, states, windows, raw, adv, targets, weights=None, grad_mult=1.0, lr=1e-4, apply_update=True):
        return self._train(states, windows, [(raw, np.float32, (self.A,))], adv, targets, weights, grad_mult, lr, apply_update)

    def read_rollout(self, which):
        T, E, R, D, A = self.T, self.eng.E, self.R, self.D, self.A
        shapes = {"states": (T, E, self.S0), "windows": (T, E, R, D), "raw": (T, E, A), "mu": (T, E, A), "sigma": (T, E, A), "actions": (T, E, A),
                  "values": (T, E), "rewards": (T, E), "dones": (T, E), "weights": (T, E), "adv": (T, E), "targets": (T, E),
                  "term_values": (T, E), "term_states": (T, E, self.S0), "term_windows": (T, E, R, D), "boot": (E,)}
        return self._read("read_rollout", which, shapes[which])

    EVAL_TRACE = ("states", "mu", "actions", "rewards", "dones")

    def eval(self, max_steps, trace_steps=0, trace_fields=EVAL_TRACE):
        """Greedy episodes of every env from the engine's current state (reset it first), one kernel launch; the engine is reset
        afterwards.  Returns total_reward (E) float64, length (E) int32, finished (E) uint8 and, with trace_steps > 0, states
        (S,E,S0), mu, actions (S,E,A), rewards, dones (S,E) of the first S = min(trace_steps, steps played) steps, each defined up to
        its env's own end (trace_fields: the ones to read back)."""
        tails = {"states": (self.S0,), "mu": (self.A,), "actions": (self.A,), "rewards": (), "dones": ()}
        return self._eval(max_steps, trace_steps, trace_fields, tails)
