"""CPU: include/goldsrl_tradesweep.h (the scripted trading-rule baseline sweep of TradeAR1) -- the two functions it declares are
exported by libgoldsrl.so and bound in goldsrl/_ffi_tradesweep.py, the signature dict names exactly the declared set and shares
nothing with the pinned goldsrl.h or with goldsrl_sweep.h, and a null handle is refused without a device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_sweep, _ffi_tradesweep
    declared = _declared("goldsrl_tradesweep.h")
    assert declared == {"grl_trade_sweep", "grl_trade_sweep_read"}
    assert set(_ffi_tradesweep.TRADE_SWEEP_SIGNATURES) == declared
    assert not declared & set(_ffi.SIGNATURES) and not declared & _declared("goldsrl.h")
    assert not declared & set(_ffi_sweep.SWEEP_SIGNATURES) and not declared & _declared("goldsrl_sweep.h")
    lib = _ffi.load_library(extra_signatures=_ffi_tradesweep.TRADE_SWEEP_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), "include/goldsrl_tradesweep.h declares %s but libgoldsrl.so does not export it" % name
    assert '#include "goldsrl.h"' in _header("goldsrl_tradesweep.h")
    assert "Replaces nothing in the reference" in _header("goldsrl_tradesweep.h")
    assert callable(_ffi_tradesweep.trade_sweep)


def test_null_handle_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_tradesweep
    lib = _ffi.load_library(extra_signatures=_ffi_tradesweep.TRADE_SWEEP_SIGNATURES)
    assert lib.grl_trade_sweep(None, None, None, 1, None, 1, -1) == _ffi.E_INVALID
    assert lib.grl_trade_sweep_read(None, b"total", None, 0) == _ffi.E_INVALID
