"""ctypes binding of the A3C discrete savings-grid agent on the device (GridSolowWorker on DiscretePolicyEstimator; C ABI:
include/goldsrl_discretenet.h, greedy acting and evaluation: include/goldsrl_discreteeval.h)."""
import ctypes as C

from . import _ffi
from ._ffi_a3c import STAT_NAMES, signatures  # noqa: F401
from ._ffi_grid import GridNet, default_init_grid, grid_param_shapes

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
    """grid_param_shapes with one output: probs3 has K columns."""
    return grid_param_shapes(K, static_size, temporal_size, 1, H, S)


def default_init_discrete(seed=3, K=51):
    return default_init_grid(seed, K, **SOLOW_SIZES)


class DiscreteNet(GridNet):
    """The savings-grid agent on a Solow Engine (GridNet with one output): the choices, actions and probabilities carry no output
    axis.  Greedy is GridSolowWorker.get_greedy_action's arg-max.  The rollout keeps term_values / term_states / term_windows."""
    PREFIX, CONFIG, SIZES, TERM = "grl_dnet_", GrlDnetConfig, SOLOW_SIZES, True
    SIGNATURES = dict(DNET_SIGNATURES, **DNET_EVAL_SIGNATURES)
