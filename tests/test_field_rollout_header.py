"""CPU: include/goldsrl_fieldrollout.h (ConvPolicyVFieldNetwork acting and learning on a Swarm handle) -- every function it declares
is exported by libgoldsrl.so and bound in goldsrl/_ffi_field.py's FIELD_ROLLOUT_SIGNATURES, none of them in FIELD_SIGNATURES,
goldsrl_fieldnet.h brings the header along, a NULL net is refused by every call, and the training script knows the net's geometry."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = {"grl_fieldnet_rollout_bind", "grl_fieldnet_predict_swarm", "grl_fieldnet_debug_grid", "grl_fieldnet_rollout",
             "grl_fieldnet_train_rollout", "grl_fieldnet_train_rollout_grads", "grl_fieldnet_read_rollout",
             "grl_fieldnet_get_optimizer_state", "grl_fieldnet_set_optimizer_state", "grl_fieldnet_get_action_counter",
             "grl_fieldnet_set_action_counter"}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_rollout_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_field
    declared = _declared("goldsrl_fieldrollout.h")
    assert declared == FUNCTIONS
    assert set(_ffi_field.FIELD_ROLLOUT_SIGNATURES) == declared and not declared & set(_ffi_field.FIELD_SIGNATURES)
    lib = _ffi.load_library(extra_signatures=_ffi_field.FIELD_ROLLOUT_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert '#include "goldsrl_fieldrollout.h"' in _header("goldsrl_fieldnet.h")
    # the net's header still declares none of them in its own text (tests/test_cabi_symbols.py reads it against FIELD_SIGNATURES)
    assert not FUNCTIONS & _declared("goldsrl_fieldnet.h")
    for method in ("rollout_bind", "predict_swarm", "debug_grid", "rollout", "train_rollout", "train_rollout_grads", "read_rollout",
                   "get_optimizer_state", "set_optimizer_state", "get_action_counter", "set_action_counter", "save_checkpoint"):
        assert callable(getattr(_ffi_field.FieldNet, method)), method


def test_null_net_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_field
    lib = _ffi.load_library(extra_signatures=_ffi_field.FIELD_ROLLOUT_SIGNATURES)
    step, counter = ctypes.c_int64(0), ctypes.c_uint64(0)
    calls = {
        "grl_fieldnet_rollout_bind": (None, 0.99),
        "grl_fieldnet_predict_swarm": (None, None, None, None),
        "grl_fieldnet_debug_grid": (None, 1, None, None, None, 0),
        "grl_fieldnet_rollout": (None, 4, 0),
        "grl_fieldnet_train_rollout": (None, 1e-3, None),
        "grl_fieldnet_train_rollout_grads": (None, None),
        "grl_fieldnet_read_rollout": (None, b"values", None, 0),
        "grl_fieldnet_get_optimizer_state": (None, None, None, 0, ctypes.byref(step)),
        "grl_fieldnet_set_optimizer_state": (None, None, None, 0, 0),
        "grl_fieldnet_get_action_counter": (None, ctypes.byref(counter)),
        "grl_fieldnet_set_action_counter": (None, 0),
    }
    assert set(calls) == FUNCTIONS
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == _ffi.E_INVALID, name


def test_the_learner_the_monitor_and_the_script_know_the_field_policy():
    from goldsrl.agents.paac import policy_monitor
    from goldsrl.agents.paac.policy_v_network import ConvPolicyVFieldNetwork
    from goldsrl.scripts import train_paac_conv, train_paac_field
    assert callable(policy_monitor.FieldSwarmPolicyMonitor.eval_once)
    args = train_paac_field.get_arg_parser().parse_args([])
    assert (args.height, args.filters, args.conv_layers) == (20, 5, 2)
    args = train_paac_field.get_arg_parser().parse_args(["--height", "12", "--filters", "4", "--conv_layers", "1", "-ec", "8"])
    assert (args.height, args.filters, args.conv_layers, args.emulator_counts) == (12, 4, 1, 8)
    # every argument of train_paac_conv is there, and the conv script's own defaults did not move
    conv = vars(train_paac_conv.get_arg_parser().parse_args([]))
    assert set(conv) <= set(vars(args)) and (conv["height"], conv["filters"]) == (84, 32)
    creator, _ = train_paac_field.get_network_and_environment_creator(args)
    net = creator()
    assert isinstance(net, ConvPolicyVFieldNetwork) and (net.height, net.width, net.channels, net.num_actions) == (12, 12, 2, 2)
    assert (net.filters, net.conv_layers) == (4, 1)
