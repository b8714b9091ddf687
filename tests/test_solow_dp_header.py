"""CPU: include/goldsrl_solowdp.h (the optimal-savings yardstick of the Solow env) -- the five functions it declares are exported by
libgoldsrl.so and bound in goldsrl/_ffi_solowdp.py, the signature dict names exactly the declared set and shares nothing with the
pinned goldsrl.h or with the sweep headers, the struct has the header's layout, and a null handle is refused without a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = {"grl_solow_dp_solve", "grl_solow_dp_set_policy", "grl_solow_dp_read", "grl_solow_dp_play", "grl_solow_dp_play_read"}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", _header(name), flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_solowdp, _ffi_sweep, _ffi_tickersweep, _ffi_tradesweep
    declared = _declared("goldsrl_solowdp.h")
    assert declared == FUNCTIONS
    assert set(_ffi_solowdp.SOLOW_DP_SIGNATURES) == declared
    assert not declared & set(_ffi.SIGNATURES) and not declared & _declared("goldsrl.h")
    assert not declared & set(_ffi_sweep.SWEEP_SIGNATURES) and not declared & _declared("goldsrl_sweep.h")
    assert not declared & set(_ffi_tradesweep.TRADE_SWEEP_SIGNATURES) and not declared & _declared("goldsrl_tradesweep.h")
    assert not declared & set(_ffi_tickersweep.TICKER_SWEEP_SIGNATURES) and not declared & _declared("goldsrl_tickersweep.h")
    lib = _ffi.load_library(extra_signatures=_ffi_solowdp.SOLOW_DP_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), "include/goldsrl_solowdp.h declares %s but libgoldsrl.so does not export it" % name
    assert '#include "goldsrl.h"' in _header("goldsrl_solowdp.h")
    assert "Replaces nothing in the reference" in _header("goldsrl_solowdp.h")
    for f in (_ffi_solowdp.solow_dp_grid, _ffi_solowdp.solow_dp_solve, _ffi_solowdp.solow_dp_play, _ffi_solowdp.solow_dp_policy_actions):
        assert callable(f)


def test_signatures_match_the_declarations():
    """argument counts and kinds of the five prototypes, read from the header's text"""
    from goldsrl import _ffi_solowdp
    text = re.sub(r"/\*.*?\*/", "", _header("goldsrl_solowdp.h"), flags=re.S)
    kinds = {"int32_t": C.c_int32, "size_t": C.c_size_t}
    for name, (restype, argtypes) in _ffi_solowdp.SOLOW_DP_SIGNATURES.items():
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


def test_grid_struct_has_the_headers_layout():
    """the members of grl_solow_dp_grid, in order, read from the header's text"""
    from goldsrl import _ffi_solowdp
    text = re.sub(r"/\*.*?\*/", "", _header("goldsrl_solowdp.h"), flags=re.S)
    n = int(re.search(r"#define\s+GRL_SOLOW_DP_MAX_NODES\s+(\d+)", text).group(1))
    assert n == _ffi_solowdp.MAX_NODES == 15
    body = re.search(r"typedef struct grl_solow_dp_grid \{(.*?)\} grl_solow_dp_grid;", text, flags=re.S).group(1)
    want = []
    for line in body.split(";"):
        line = line.strip()
        if not line:
            continue
        ctype = {"double": C.c_double, "int32_t": C.c_int32}[line.split()[0]]
        for member in line.split(None, 1)[1].split(","):
            m = re.match(r"(\w+)(\[GRL_SOLOW_DP_MAX_NODES\])?$", member.strip())
            want.append((m.group(1), ctype * n if m.group(2) else ctype))
    got = _ffi_solowdp.SolowDpGrid._fields_
    assert [f[0] for f in got] == [w[0] for w in want]
    assert all(C.sizeof(a[1]) == C.sizeof(b[1]) for a, b in zip(got, want))
    assert C.sizeof(_ffi_solowdp.SolowDpGrid) == 8 * (5 + 2 * n) + 16


def test_null_handle_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_solowdp
    lib = _ffi.load_library(extra_signatures=_ffi_solowdp.SOLOW_DP_SIGNATURES)
    g = _ffi_solowdp._grid_struct(_ffi_solowdp.solow_dp_grid())
    assert lib.grl_solow_dp_solve(None, C.byref(g), 4) == _ffi.E_INVALID
    assert lib.grl_solow_dp_set_policy(None, C.byref(g), 4, None) == _ffi.E_INVALID
    assert lib.grl_solow_dp_read(None, b"policy", None, 0) == _ffi.E_INVALID
    assert lib.grl_solow_dp_play(None, 4, 0) == _ffi.E_INVALID
    assert lib.grl_solow_dp_play_read(None, b"total", None, 0) == _ffi.E_INVALID
