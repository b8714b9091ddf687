"""CPU: include/goldsrl_tradeforesight.h (the foresight ceiling of the TradeAR1 env) -- the two functions it declares are exported by
libgoldsrl.so and bound in goldsrl/_ffi_tradeforesight.py, the signature dict names exactly the declared set and shares nothing
with the pinned goldsrl.h, with the trade sweep's header or with the Ticker foresight's, and a null handle is refused without a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_tradeforesight, _ffi_tradesweep
    declared = _declared("goldsrl_tradeforesight.h")
    assert declared == {"grl_trade_foresight", "grl_trade_foresight_read"}
    assert set(_ffi_tradeforesight.TRADE_FORESIGHT_SIGNATURES) == declared
    assert not declared & set(_ffi.SIGNATURES) and not declared & _declared("goldsrl.h")
    assert not declared & set(_ffi_tradesweep.TRADE_SWEEP_SIGNATURES) and not declared & _declared("goldsrl_tradesweep.h")
    assert not declared & _declared("goldsrl_tickerforesight.h")
    lib = _ffi.load_library(extra_signatures=_ffi_tradeforesight.TRADE_FORESIGHT_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), "include/goldsrl_tradeforesight.h declares %s but libgoldsrl.so does not export it" % name
    assert '#include "goldsrl.h"' in _header("goldsrl_tradeforesight.h")
    assert "Replaces nothing in the reference" in _header("goldsrl_tradeforesight.h")
    assert callable(_ffi_tradeforesight.trade_foresight) and callable(_ffi_tradeforesight.trade_foresight_actions)


def test_signatures_match_the_declarations():
    """argument counts and kinds of the two prototypes, read from the header's text"""
    from goldsrl import _ffi_tradeforesight
    text = re.sub(r"/\*.*?\*/", "", _header("goldsrl_tradeforesight.h"), flags=re.S)
    kinds = {"int32_t": C.c_int32, "size_t": C.c_size_t}
    for name, (restype, argtypes) in _ffi_tradeforesight.TRADE_FORESIGHT_SIGNATURES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            arg = arg.strip()
            if "*" in arg:
                want.append(C.c_char_p if arg.startswith("const char") else C.c_void_p)
            else:
                want.append(kinds[arg.split()[0]])
        assert restype is C.c_int and list(argtypes) == want, (name, argtypes, want)


def test_null_handle_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_tradeforesight
    lib = _ffi.load_library(extra_signatures=_ffi_tradeforesight.TRADE_FORESIGHT_SIGNATURES)
    assert lib.grl_trade_foresight(None, None, 1, None, 1, -1) == _ffi.E_INVALID
    assert lib.grl_trade_foresight_read(None, b"total", None, 0) == _ffi.E_INVALID
