"""ctypes binding of the A3C grid trader on the device (DiscretePolicyEstimator with num_outputs = 2 on a 2-asset TradeAR1 engine;
C ABI, greedy acting and evaluation: include/goldsrl_gridtradenet.h; learning from the attainable optimum's table:
include/goldsrl_gridtradeteach.h)."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_a3c import STAT_NAMES, signatures  # noqa: F401
from ._ffi_grid import GridNet, default_init_grid, grid_param_shapes

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

# include/goldsrl_gridtradeteach.h: a dict of its own, as the header is a file of its own
_P, _I, _F = C.c_void_p, C.c_int32, C.c_float
GTNET_TEACH_SIGNATURES = {
    "grl_gtnet_teach_rollout": (C.c_int, [_P, _I, C.c_double]),
    "grl_gtnet_train_teach_rollout": (C.c_int, [_P, _F, _P]),
    "grl_gtnet_teach": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _F, _F, _I, _P]),
}
TEACH_STAT_NAMES = ("cross_entropy",) + STAT_NAMES[1:] + ("agreement",)


def trade_grid_labels(actions, K, lb=-1.0, ub=1.0):
    """The soft label of float32 actions on np.linspace(lb, ub, K), as the teach rollout states it (float64, one operation per
    statement): (label_lo int32, label_w float32), mass 1 - w on point lo and w on lo + 1."""
    a = np.asarray(actions, np.float32).astype(np.float64)
    step = (float(ub) - float(lb)) / float(K - 1)
    pos = (a - float(lb)) / step
    lo = np.clip(np.floor(pos).astype(np.int64), 0, K - 2)
    return lo.astype(np.int32), np.clip(pos - lo, 0.0, 1.0).astype(np.float32)


def gridtrade_param_shapes(K=17, static_size=5, temporal_size=5, num_outputs=2, H=32, S=128):
    return grid_param_shapes(K, static_size, temporal_size, num_outputs, H, S)


def default_init_gridtrade(seed=3, K=17):
    return default_init_grid(seed, K, **TRADE_SIZES)


class GridTradeNet(GridNet):
    """The grid trader on a 2-asset TradeAR1 Engine (GridNet with one output per asset; default 17 points on [-1, 1]): choices and
    actions are (.., O), probabilities (.., O, K).  Trade episodes end terminally: the rollout has no term_* buffers."""
    PREFIX, CONFIG, SIZES, TERM = "grl_gtnet_", GrlGtnetConfig, TRADE_SIZES, False
    SIGNATURES = dict(GTNET_SIGNATURES, **GTNET_EVAL_SIGNATURES, **GTNET_TEACH_SIGNATURES)
    taught = False      # the last rollout was a teach rollout

    def rollout(self, T):
        super().rollout(T)
        self.taught = False

    def teach_rollout(self, T, agent_share=0.0):
        """rollout with the teacher: the table on the engine (trade_dp_solve / trade_dp_set_policy) labels every step, and each env
        is stepped with the agent's action with probability agent_share, else with the teacher's.  read_rollout then also serves
        "teacher_actions" (T,E,O) float32, "label_lo" (T,E,O) int32 and "label_w" (T,E,O) float32."""
        self._check(self._fn("teach_rollout")(self.n, int(T), float(agent_share)))
        self.T, self.taught = int(T), True

    def train_teach_rollout(self, lr=1e-4):
        """The supervised update on the last teach rollout; the seven stats by name (TEACH_STAT_NAMES)."""
        stats = np.zeros(7, np.float32)
        self._check(self._fn("train_teach_rollout")(self.n, float(lr), _ffi._ptr(stats)))
        return dict(zip(TEACH_STAT_NAMES, stats.tolist()))

    def teach(self, states, windows, label_lo, label_w, targets, weights=None, grad_mult=1.0, lr=1e-4, apply_update=True):
        """The supervised update on host samples: label_lo (n,O) int32 and label_w (n,O) as trade_grid_labels gives them."""
        n, s, w = self._stage(states, windows)
        lo, lw, tg = np.ascontiguousarray(label_lo, np.int32), np.ascontiguousarray(label_w, np.float32), np.ascontiguousarray(targets, np.float32)
        assert lo.shape == lw.shape == (n, self.O) and tg.shape == (n,), (lo.shape, lw.shape, tg.shape)
        wt = None if weights is None else np.ascontiguousarray(weights, np.float32)
        stats = np.zeros(7, np.float32)
        self._check(self._fn("teach")(self.n, n, _ffi._ptr(s), _ffi._ptr(w), _ffi._ptr(lo), _ffi._ptr(lw), _ffi._ptr(tg),
                                      None if wt is None else _ffi._ptr(wt), float(grad_mult), float(lr), 1 if apply_update else 0, _ffi._ptr(stats)))
        return dict(zip(TEACH_STAT_NAMES, stats.tolist()))

    def read_rollout(self, which):
        if which in ("teacher_actions", "label_lo", "label_w"):
            a = np.empty((self.T, self.eng.E, self.O), np.int32 if which == "label_lo" else np.float32)
            self._check(self._fn("read_rollout")(self.n, which.encode(), _ffi._ptr(a), a.nbytes))
            return a
        return super().read_rollout(which)
