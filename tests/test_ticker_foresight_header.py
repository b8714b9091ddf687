"""CPU: include/goldsrl_tickerforesight.h (the foresight ceiling of the Ticker env) -- the two functions it declares are exported by
libgoldsrl.so and bound in goldsrl/_ffi_tickerforesight.py, the signature dict names exactly the declared set and shares nothing
with the pinned goldsrl.h or with the sweep headers, and a null handle is refused without a device."""
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
    from goldsrl import _ffi, _ffi_tickerforesight, _ffi_tickersweep
    declared = _declared("goldsrl_tickerforesight.h")
    assert declared == {"grl_ticker_foresight", "grl_ticker_foresight_read"}
    assert set(_ffi_tickerforesight.TICKER_FORESIGHT_SIGNATURES) == declared
    assert not declared & set(_ffi.SIGNATURES) and not declared & _declared("goldsrl.h")
    assert not declared & set(_ffi_tickersweep.TICKER_SWEEP_SIGNATURES) and not declared & _declared("goldsrl_tickersweep.h")
    lib = _ffi.load_library(extra_signatures=_ffi_tickerforesight.TICKER_FORESIGHT_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), "include/goldsrl_tickerforesight.h declares %s but libgoldsrl.so does not export it" % name
    assert '#include "goldsrl.h"' in _header("goldsrl_tickerforesight.h")
    assert "Replaces nothing in the reference" in _header("goldsrl_tickerforesight.h")
    assert callable(_ffi_tickerforesight.ticker_foresight) and callable(_ffi_tickerforesight.ticker_foresight_actions)


def test_signatures_match_the_declarations():
    """argument counts and kinds of the two prototypes, read from the header's text"""
    from goldsrl import _ffi_tickerforesight
    text = re.sub(r"/\*.*?\*/", "", _header("goldsrl_tickerforesight.h"), flags=re.S)
    kinds = {"int32_t": C.c_int32, "size_t": C.c_size_t}
    for name, (restype, argtypes) in _ffi_tickerforesight.TICKER_FORESIGHT_SIGNATURES.items():
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
    from goldsrl import _ffi, _ffi_tickerforesight
    lib = _ffi.load_library(extra_signatures=_ffi_tickerforesight.TICKER_FORESIGHT_SIGNATURES)
    assert lib.grl_ticker_foresight(None, None, 1, 1, -1) == _ffi.E_INVALID
    assert lib.grl_ticker_foresight_read(None, b"total", None, 0) == _ffi.E_INVALID
