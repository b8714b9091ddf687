"""CPU: include/goldsrl_solowforesight.h (the perfect-foresight ceiling of the Solow env) -- the two functions it declares are
exported by libgoldsrl.so and bound in goldsrl/_ffi_solowforesight.py with the declared argument kinds, the signature dict names
exactly the declared set and shares nothing with the other headers, the struct has the header's layout, and a null handle is
refused without a device.  The numpy restatement of the recurrence (tests/_solow_foresight_oracle.py) is held to an enumeration."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import _solow_foresight_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FUNCTIONS = {"grl_solow_foresight", "grl_solow_foresight_read"}
DECLARATION = r"\b(grl_[a-z0-9_]+)\s*\("


def _code(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, name)).read(), flags=re.S)


def test_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_solowforesight as F
    text = _code("goldsrl_solowforesight.h")
    declared = set(re.findall(DECLARATION, text))
    assert declared == FUNCTIONS == set(F.SOLOW_FORESIGHT_SIGNATURES)
    lib = _ffi.load_library(extra_signatures=F.SOLOW_FORESIGHT_SIGNATURES)
    kinds = {"int32_t": C.c_int32, "size_t": C.c_size_t}
    for name, (restype, argtypes) in F.SOLOW_FORESIGHT_SIGNATURES.items():
        assert hasattr(lib, name), "include/goldsrl_solowforesight.h declares %s but libgoldsrl.so does not export it" % name
        args = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text).group(1).split(",")
        want = [(C.c_char_p if a.strip().startswith("const char") else C.c_void_p) if "*" in a else kinds[a.split()[0]] for a in args]
        assert restype is C.c_int and list(argtypes) == want, (name, argtypes, want)


@pytest.mark.parametrize("other", sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h") and f != "goldsrl_solowforesight.h"))
def test_names_are_shared_with_no_other_header(other):
    assert not FUNCTIONS & set(re.findall(DECLARATION, _code(other)))


def test_struct_has_the_headers_layout():
    """the members, in order, read from the header's text; the two size limits are the binding's"""
    from goldsrl import _ffi_solowforesight as F
    text = _code("goldsrl_solowforesight.h")
    size = {k: int(v) for k, v in re.findall(r"#define\s+GRL_SOLOW_FORESIGHT_(MAX_NK|MAX_NS)\s+(\d+)", text)}
    assert (size["MAX_NK"], size["MAX_NS"]) == (F.MAX_NK, F.MAX_NS)
    body = re.search(r"typedef struct grl_solow_foresight_grid \{(.*?)\} grl_solow_foresight_grid;", text, flags=re.S).group(1)
    want = []
    for line in filter(None, (part.strip() for part in body.split(";"))):
        width = {"double": 8, "int32_t": 4}[line.split()[0]]
        want += [(member.strip(), width) for member in line.split(None, 1)[1].split(",")]
    assert [(f[0], C.sizeof(f[1])) for f in F.SolowForesightGrid._fields_] == want


def test_null_handle_is_refused_without_a_device():
    from goldsrl import _ffi, _ffi_solowforesight as F
    lib = _ffi.load_library(extra_signatures=F.SOLOW_FORESIGHT_SIGNATURES)
    g = F._grid_struct({"nk": 8, "ns": 8, "k_lo": 1.0, "k_hi": 100.0, "s_lo": 0.001, "s_hi": 0.999})
    assert lib.grl_solow_foresight(None, C.byref(g), 4, 0) == _ffi.E_INVALID
    assert lib.grl_solow_foresight_read(None, b"total", None, 0) == _ffi.E_INVALID


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_brackets_the_enumeration(seed):
    """3 steps, 4 rates, nk = 1024, capital low enough that saving pays (the plan is rate 1, 1, 0): the best of the 4^3 rate
    sequences played exactly from k_0 must lie between the oracle's played total and its V_0(k_0).  Measured on seeds 1 to 5: the
    played total IS the enumeration's best, to the bit (the plan's blends are of equal rates), and V_0(k_0) is 3.5e-7 to 4.1e-7
    above it (the interpolation in k').  So the bracket is asserted with no slack at all, and its width below 4e-6, ten times the
    largest measured."""
    delta, k0 = 0.02, 0.05
    z = np.log([1.0, 3.0, 9.0]) + np.random.RandomState(seed).normal(scale=0.3, size=3)
    ez = np.exp(z.astype(np.float32)).astype(np.float64)
    grid = {"nk": 1024, "ns": 4, "k_lo": 0.01, "k_hi": 10.0, "s_lo": 0.05, "s_hi": 0.8}
    dec, V, _ = FO.solve(ez, grid, delta)
    assert len(np.unique(dec)) > 1
    played, _ = FO.play(dec, ez, k0, grid, delta)
    rates = FO.axes(grid)[2]
    best = -np.inf
    for seq in itertools.product(rates, repeat=3):
        k, total = k0, 0.0
        for t, s in enumerate(seq):
            y = ez[t] * k ** 0.33
            total += float(np.log((1.0 - s) * y + 1e-4))
            k = (1.0 - delta) * k + s * y
        best = max(best, total)
    v0 = FO.value_at(V, k0, grid)
    print("foresight oracle seed %d: played %.12f best %.12f V0 %.12f" % (seed, played, best, v0))
    assert played <= best <= v0
    assert v0 - played < 4e-6
