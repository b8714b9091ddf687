"""CPU: include/goldsrl_gatedeval.h (greedy acting and greedy evaluation of the Ticker gated trader) -- every function it declares
is exported by libgoldsrl.so and bound in goldsrl/_ffi_gated.py, and goldsrl_gatednet.h brings it along."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_eval_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_gated
    text = re.sub(r"/\*.*?\*/", "", _header("goldsrl_gatedeval.h"), flags=re.S)
    declared = set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))
    assert declared == {"grl_gnet_set_greedy", "grl_gnet_eval", "grl_gnet_read_eval"}
    assert set(_ffi_gated.GNET_EVAL_SIGNATURES) == declared and not declared & set(_ffi_gated.GNET_SIGNATURES)
    lib = _ffi.load_library(extra_signatures=_ffi_gated.GNET_EVAL_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert '#include "goldsrl_gatedeval.h"' in _header("goldsrl_gatednet.h")
    for method in ("set_greedy", "eval"):
        assert callable(getattr(_ffi_gated.GatedNet, method))


def test_null_net_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_gated
    lib = _ffi.load_library(extra_signatures=_ffi_gated.GNET_EVAL_SIGNATURES)
    assert lib.grl_gnet_set_greedy(None, 1) == _ffi.E_INVALID
    assert lib.grl_gnet_eval(None, 8, 0) == _ffi.E_INVALID
    assert lib.grl_gnet_read_eval(None, b"length", None, 0) == _ffi.E_INVALID


def test_monitor_and_script_expose_the_evaluation():
    from goldsrl.agents.a3c import policy_monitor as pm
    from goldsrl.scripts import train_ticker
    for method in ("eval_once", "write_scalars", "write_log", "continuous_eval", "close"):
        assert getattr(pm.GatedPolicyMonitor, method) is getattr(pm.PolicyMonitor, method)      # shared, not copied
    args = train_ticker.get_arg_parser().parse_args(["--table", "t.npz"])
    assert args.eval_envs == 0 and args.eval_csv is None and args.eval_table is None
    args = train_ticker.get_arg_parser().parse_args(["--table", "t.npz", "--eval-envs", "64", "--eval-every", "3", "--eval-table", "h.npz"])
    assert (args.eval_envs, args.eval_every, args.eval_table) == (64, 3, "h.npz")
