"""CPU: include/goldsrl_flatwindow.h (the flat PAAC policy under the true history window) -- every function it declares is exported
by libgoldsrl.so and bound in goldsrl/_ffi_flat.py, and goldsrl_flatnet.h brings it along."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = {"grl_fnet_set_true_window", "grl_fnet_read_windows"}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_window_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_flat
    text = re.sub(r"/\*.*?\*/", "", _header("goldsrl_flatwindow.h"), flags=re.S)
    declared = set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))
    assert declared == FUNCTIONS
    assert set(_ffi_flat.FNET_WINDOW_SIGNATURES) == declared
    assert not declared & (set(_ffi_flat.FNET_SIGNATURES) | set(_ffi_flat.FNET_EVAL_SIGNATURES))
    lib = _ffi.load_library(extra_signatures=_ffi_flat.FNET_WINDOW_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert '#include "goldsrl_flatwindow.h"' in _header("goldsrl_flatnet.h")
    # the new header alone declares them: not the training header's own text (tests/test_cabi_symbols.py reads it against
    # FNET_SIGNATURES), not the evaluation's
    for other in ("goldsrl_flatnet.h", "goldsrl_flateval.h"):
        body = re.sub(r"/\*.*?\*/", "", _header(other), flags=re.S)
        assert not FUNCTIONS & set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", body)), other
    for method in ("set_true_window", "read_windows"):
        assert callable(getattr(_ffi_flat.FlatNet, method))


def test_null_net_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_flat
    lib = _ffi.load_library(extra_signatures=_ffi_flat.FNET_WINDOW_SIGNATURES)
    assert lib.grl_fnet_set_true_window(None, 1) == _ffi.E_INVALID
    assert lib.grl_fnet_read_windows(None, 0, 0, None, 0) == _ffi.E_INVALID


def test_the_estimator_the_monitor_and_the_script_know_the_switch():
    import inspect
    from goldsrl.agents.paac import policy_monitor, policy_v_network
    from goldsrl.scripts import train_paac_solow
    assert inspect.signature(policy_v_network.FlatPolicyVNetwork.bind).parameters["true_window"].default is False
    assert inspect.signature(policy_monitor.DeviceSolowPolicyMonitor.__init__).parameters["true_window"].default is False
    assert train_paac_solow.get_arg_parser().parse_args([]).true_history is False
    assert train_paac_solow.get_arg_parser().parse_args(["--true-history"]).true_history is True
