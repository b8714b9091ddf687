"""CPU: include/goldsrl_solowarmadp.h (the ARMA-state optimal-savings yardstick of the Solow env) -- the six functions it declares
are exported by libgoldsrl.so and bound in goldsrl/_ffi_solowarmadp.py with the declared argument kinds, the signature dict names
exactly the declared set and shares nothing with goldsrl.h or goldsrl_solowdp.h, the two structs have the header's layout, and a
null handle is refused without a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = {"grl_solow_arma_model", "grl_solow_arma_dp_solve", "grl_solow_arma_dp_set_policy", "grl_solow_arma_dp_read",
             "grl_solow_arma_dp_play", "grl_solow_arma_dp_play_read"}


def _code(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_solowarmadp, _ffi_solowdp
    text = _code("goldsrl_solowarmadp.h")
    declared = set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))
    assert declared == FUNCTIONS == set(_ffi_solowarmadp.SOLOW_ARMA_DP_SIGNATURES)
    assert not declared & (set(_ffi.SIGNATURES) | set(_ffi_solowdp.SOLOW_DP_SIGNATURES))
    assert not declared & set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", _code("goldsrl.h") + _code("goldsrl_solowdp.h")))
    lib = _ffi.load_library(extra_signatures=_ffi_solowarmadp.SOLOW_ARMA_DP_SIGNATURES)
    kinds = {"int32_t": C.c_int32, "size_t": C.c_size_t}
    for name, (restype, argtypes) in _ffi_solowarmadp.SOLOW_ARMA_DP_SIGNATURES.items():
        assert hasattr(lib, name), "include/goldsrl_solowarmadp.h declares %s but libgoldsrl.so does not export it" % name
        args = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text).group(1).split(",")
        want = [(C.c_char_p if a.strip().startswith("const char") else C.c_void_p) if "*" in a else kinds[a.split()[0]] for a in args]
        assert restype is C.c_int and list(argtypes) == want, (name, argtypes, want)


@pytest.mark.parametrize("struct,cls", [("grl_solow_arma_coef", "SolowArmaCoef"), ("grl_solow_arma_dp_grid", "SolowArmaDpGrid")])
def test_structs_have_the_headers_layout(struct, cls):
    """the members, in order, with their array lengths, read from the header's text"""
    from goldsrl import _ffi_solowarmadp
    text = _code("goldsrl_solowarmadp.h")
    size = {k: int(v) for k, v in re.findall(r"#define\s+GRL_SOLOW_ARMA_DP_(MAX_DIM|MAX_LAGS|MAX_NODES)\s+(\d+)", text)}
    assert (size["MAX_DIM"], size["MAX_LAGS"], size["MAX_NODES"]) == (_ffi_solowarmadp.MAX_DIM, _ffi_solowarmadp.MAX_LAGS, _ffi_solowarmadp.MAX_NODES)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
    want = []
    for line in filter(None, (part.strip() for part in body.split(";"))):
        width = {"double": 8, "int32_t": 4}[line.split()[0]]
        for member in line.split(None, 1)[1].split(","):
            m = re.match(r"(\w+)(?:\[([^\]]+)\])?$", member.strip())
            count = eval(m.group(2).replace("GRL_SOLOW_ARMA_DP_", ""), {}, size) if m.group(2) else 1
            want.append((m.group(1), width * count))
    assert [(f[0], C.sizeof(f[1])) for f in getattr(_ffi_solowarmadp, cls)._fields_] == want


def test_null_handle_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_solowarmadp
    lib = _ffi.load_library(extra_signatures=_ffi_solowarmadp.SOLOW_ARMA_DP_SIGNATURES)
    g = _ffi_solowarmadp._grid_struct(_ffi_solowarmadp.solow_arma_dp_grid(2, 2))
    assert lib.grl_solow_arma_model(None, None) == _ffi.E_INVALID
    assert lib.grl_solow_arma_dp_solve(None, C.byref(g), 4) == _ffi.E_INVALID
    assert lib.grl_solow_arma_dp_set_policy(None, C.byref(g), 4, None) == _ffi.E_INVALID
    assert lib.grl_solow_arma_dp_read(None, b"policy", None, 0) == _ffi.E_INVALID
    assert lib.grl_solow_arma_dp_play(None, 4, 0) == _ffi.E_INVALID
    assert lib.grl_solow_arma_dp_play_read(None, b"total", None, 0) == _ffi.E_INVALID
