"""ctypes binding of the A3C grid trader on the device (DiscretePolicyEstimator with num_outputs = 2 on a 2-asset TradeAR1 engine;
C ABI, greedy acting and evaluation: include/goldsrl_gridtradenet.h)."""
import ctypes as C

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


def gridtrade_param_shapes(K=17, static_size=5, temporal_size=5, num_outputs=2, H=32, S=128):
    return grid_param_shapes(K, static_size, temporal_size, num_outputs, H, S)


def default_init_gridtrade(seed=3, K=17):
    return default_init_grid(seed, K, **TRADE_SIZES)


class GridTradeNet(GridNet):
    """The grid trader on a 2-asset TradeAR1 Engine (GridNet with one output per asset; default 17 points on [-1, 1]): choices and
    actions are (.., O), probabilities (.., O, K).  Trade episodes end terminally: the rollout has no term_* buffers."""
    PREFIX, CONFIG, SIZES, TERM = "grl_gtnet_", GrlGtnetConfig, TRADE_SIZES, False
    SIGNATURES = dict(GTNET_SIGNATURES, **GTNET_EVAL_SIGNATURES)
