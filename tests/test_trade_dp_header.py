"""CPU: include/goldsrl_tradedp.h (the attainable optimum of the TradeAR1 env) -- the five functions it declares are exported by
libgoldsrl.so and bound in goldsrl/_ffi_tradedp.py, the signature dict names exactly the declared set and shares nothing with the
pinned goldsrl.h, the struct has the header's layout, and a null handle is refused without a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = {"grl_trade_dp_solve", "grl_trade_dp_set_policy", "grl_trade_dp_read", "grl_trade_dp_play", "grl_trade_dp_play_read"}


def _code(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_tradedp
    text = _code("goldsrl_tradedp.h")
    declared = set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))
    assert declared == FUNCTIONS == set(_ffi_tradedp.TRADE_DP_SIGNATURES)
    assert not declared & set(_ffi.SIGNATURES) and not declared & set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", _code("goldsrl.h")))
    lib = _ffi.load_library(extra_signatures=_ffi_tradedp.TRADE_DP_SIGNATURES)
    kinds = {"int32_t": C.c_int32, "size_t": C.c_size_t}
    for name, (restype, argtypes) in _ffi_tradedp.TRADE_DP_SIGNATURES.items():
        assert hasattr(lib, name), "include/goldsrl_tradedp.h declares %s but libgoldsrl.so does not export it" % name
        args = [a.strip() for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text).group(1).split(",")]
        want = [(C.c_char_p if a.startswith("const char") else C.c_void_p) if "*" in a else kinds[a.split()[0]] for a in args]
        assert restype is C.c_int and list(argtypes) == want, (name, argtypes, want)


def test_grid_struct_has_the_headers_layout():
    from goldsrl import _ffi_tradedp
    text = _code("goldsrl_tradedp.h")
    n = int(re.search(r"#define\s+GRL_TRADE_DP_MAX_NODES\s+(\d+)", text).group(1))
    assert n == _ffi_tradedp.MAX_NODES
    body = re.search(r"typedef struct grl_trade_dp_grid \{(.*?)\} grl_trade_dp_grid;", text, flags=re.S).group(1)
    want = []
    for line in filter(None, (l.strip() for l in body.split(";"))):
        ctype = {"double": C.c_double, "int32_t": C.c_int32}[line.split()[0]]
        for member in line.split(None, 1)[1].split(","):
            m = re.match(r"(\w+)(\[GRL_TRADE_DP_MAX_NODES\])?$", member.strip())
            want.append((m.group(1), C.sizeof(ctype) * (n if m.group(2) else 1)))
    assert [(f[0], C.sizeof(f[1])) for f in _ffi_tradedp.TradeDpGrid._fields_] == want
    assert C.sizeof(_ffi_tradedp.TradeDpGrid) == 8 * (1 + 2 * n) + 16


def test_null_handle_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_tradedp
    lib = _ffi.load_library(extra_signatures=_ffi_tradedp.TRADE_DP_SIGNATURES)
    g = _ffi_tradedp._grid_struct(_ffi_tradedp.trade_dp_grid())
    assert lib.grl_trade_dp_solve(None, C.byref(g), 4) == _ffi.E_INVALID
    assert lib.grl_trade_dp_set_policy(None, C.byref(g), 4, None) == _ffi.E_INVALID
    assert lib.grl_trade_dp_read(None, b"policy", None, 0) == _ffi.E_INVALID
    assert lib.grl_trade_dp_play(None, None, 4, 0) == _ffi.E_INVALID
    assert lib.grl_trade_dp_play_read(None, b"total", None, 0) == _ffi.E_INVALID
