"""CPU: include/goldsrl_gausseval.h (greedy acting and greedy evaluation of the A3C Gaussian agent) -- every function it declares
is exported by libgoldsrl.so and bound in goldsrl/_ffi_gauss.py, and goldsrl_gaussnet.h brings it along."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_eval_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_gauss
    text = re.sub(r"/\*.*?\*/", "", _header("goldsrl_gausseval.h"), flags=re.S)
    declared = set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))
    assert declared == {"grl_anet_set_greedy", "grl_anet_eval", "grl_anet_read_eval"}
    assert set(_ffi_gauss.ANET_EVAL_SIGNATURES) == declared and not declared & set(_ffi_gauss.ANET_SIGNATURES)
    lib = _ffi.load_library(extra_signatures=_ffi_gauss.ANET_EVAL_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert '#include "goldsrl_gausseval.h"' in _header("goldsrl_gaussnet.h")
    for method in ("set_greedy", "eval"):
        assert callable(getattr(_ffi_gauss.GaussNet, method))


def test_null_net_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_gauss
    lib = _ffi.load_library(extra_signatures=_ffi_gauss.ANET_EVAL_SIGNATURES)
    assert lib.grl_anet_set_greedy(None, 1) == _ffi.E_INVALID
    assert lib.grl_anet_eval(None, 8, 0) == _ffi.E_INVALID
    assert lib.grl_anet_read_eval(None, b"length", None, 0) == _ffi.E_INVALID
