"""CPU: include/goldsrl_neteval.h (the conv policy's evaluation episodes on the device) -- it declares exactly its two functions, both
are exported by libgoldsrl.so and bound in goldsrl/_ffi_net.py's NET_EVAL_SIGNATURES and in no other dict, goldsrl_net.h brings the
header along without declaring them itself, a NULL net is refused without a device, the Python surface exists, and --eval-envs is
train_paac_conv's own (default 0: the host-loop monitor) while train_paac_field keeps its default of 1."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = {"grl_net_eval", "grl_net_read_eval"}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_eval_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_net
    assert _declared("goldsrl_neteval.h") == FUNCTIONS
    assert set(_ffi_net.NET_EVAL_SIGNATURES) == FUNCTIONS
    assert not FUNCTIONS & set(_ffi_net.NET_SIGNATURES) and not FUNCTIONS & set(_ffi.SIGNATURES)
    assert not FUNCTIONS & _declared("goldsrl_net.h")
    assert '#include "goldsrl_neteval.h"' in _header("goldsrl_net.h")
    lib = _ffi.load_library(extra_signatures=_ffi_net.NET_EVAL_SIGNATURES)
    for name in FUNCTIONS:
        assert hasattr(lib, name), name


def test_null_net_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_net
    lib = _ffi.load_library(extra_signatures=_ffi_net.NET_EVAL_SIGNATURES)
    assert lib.grl_net_eval(None, 8, 0, None, 0, -1) == _ffi.E_INVALID
    assert lib.grl_net_read_eval(None, b"rewards", None, 0) == _ffi.E_INVALID


def test_the_python_surface_exists():
    import inspect

    from goldsrl import _ffi_net
    from goldsrl.agents.paac import policy_monitor
    for method in ("eval", "read_eval"):
        assert callable(getattr(_ffi_net.ConvNet, method)), method
    args = inspect.signature(_ffi_net.ConvNet.eval).parameters
    assert list(args) == ["self", "max_steps", "greedy", "normals", "keep_actions", "trace_env"]
    assert (args["greedy"].default, args["normals"].default, args["keep_actions"].default, args["trace_env"].default) == (False, None, False, -1)
    mon = policy_monitor.DeviceSwarmPolicyMonitor
    assert issubclass(mon, policy_monitor.SwarmPolicyMonitor)
    args = inspect.signature(mon.__init__).parameters
    assert args["env"].default == "Swarm-eval-v0" and args["n_envs"].default == 1 and args["greedy"].default is False


def test_the_scripts_know_eval_envs():
    from goldsrl.scripts import train_paac_conv, train_paac_field
    p = train_paac_conv.get_arg_parser()
    assert p.parse_args([]).eval_envs == 0 and p.parse_args(["--eval-envs", "16"]).eval_envs == 16
    assert train_paac_field.get_arg_parser().parse_args([]).eval_envs == 1
