"""CPU: include/goldsrl_fieldeval.h (the field policy's whole-episode evaluation) -- it declares exactly its two functions, both are
exported by libgoldsrl.so and bound in goldsrl/_ffi_field.py's FIELD_EVAL_SIGNATURES and in no other dict, goldsrl_fieldnet.h brings
the header along, a NULL net is refused without a device, and the training script knows --eval-envs."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = {"grl_fieldnet_eval", "grl_fieldnet_read_eval"}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_eval_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_field
    assert _declared("goldsrl_fieldeval.h") == FUNCTIONS
    assert set(_ffi_field.FIELD_EVAL_SIGNATURES) == FUNCTIONS
    assert not FUNCTIONS & set(_ffi_field.FIELD_SIGNATURES) and not FUNCTIONS & set(_ffi_field.FIELD_ROLLOUT_SIGNATURES)
    assert not FUNCTIONS & _declared("goldsrl_fieldnet.h") and not FUNCTIONS & _declared("goldsrl_fieldrollout.h")
    assert '#include "goldsrl_fieldeval.h"' in _header("goldsrl_fieldnet.h")
    lib = _ffi.load_library(extra_signatures=_ffi_field.FIELD_EVAL_SIGNATURES)
    for name in FUNCTIONS:
        assert hasattr(lib, name), name
    for method in ("eval", "read_eval"):
        assert callable(getattr(_ffi_field.FieldNet, method)), method


def test_null_net_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_field
    lib = _ffi.load_library(extra_signatures=_ffi_field.FIELD_EVAL_SIGNATURES)
    assert lib.grl_fieldnet_eval(None, 8, 1, 0, 0, -1) == _ffi.E_INVALID
    assert lib.grl_fieldnet_read_eval(None, b"rewards", None, 0) == _ffi.E_INVALID


def test_the_script_and_the_monitor_know_eval_envs():
    import inspect

    from goldsrl.agents.paac import policy_monitor
    from goldsrl.scripts import train_paac_field
    p = train_paac_field.get_arg_parser()
    assert p.parse_args([]).eval_envs == 1 and p.parse_args(["--eval-envs", "16"]).eval_envs == 16
    args = inspect.signature(policy_monitor.FieldSwarmPolicyMonitor.__init__).parameters
    assert args["n_envs"].default == 1 and isinstance(args["device_episode"].default, bool)
