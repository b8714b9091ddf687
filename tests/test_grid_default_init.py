"""CPU: the two softmax-grid nets' parameter layouts and default initialisations, now one grid_param_shapes / default_init_grid
(goldsrl/_ffi_grid.py), give what default_init_discrete / default_init_gridtrade gave before they were joined: the same shapes and,
for the same seed, the same bytes.  tests/golden/grid_default_init.json holds, per (seed, K), the size, the shape list and the
SHA-256 of the float32 array as the separate functions computed them."""
import hashlib
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "grid_default_init.json")) as f:
    RECORDED = json.load(f)


def _functions(kind):
    from goldsrl import _ffi_discrete, _ffi_gridtrade
    return {"discrete": (_ffi_discrete.default_init_discrete, _ffi_discrete.discrete_param_shapes, _ffi_discrete.SOLOW_SIZES),
            "gridtrade": (_ffi_gridtrade.default_init_gridtrade, _ffi_gridtrade.gridtrade_param_shapes, _ffi_gridtrade.TRADE_SIZES)}[kind]


@pytest.mark.parametrize("kind,case", [(k, c) for k in sorted(RECORDED) for c in RECORDED[k]],
                         ids=lambda v: v if isinstance(v, str) else "seed%d-K%d" % (v["seed"], v["K"]))
def test_default_init_bytes_and_shapes_as_recorded(kind, case):
    from goldsrl import _ffi_grid
    init, shapes, sizes = _functions(kind)
    a = init(case["seed"], case["K"])
    assert a.dtype.name == "float32" and a.size == case["size"]
    assert hashlib.sha256(a.tobytes()).hexdigest() == case["sha256"]
    assert [[n, list(s)] for n, s in shapes(case["K"])] == case["shapes"]
    # the named functions are the shared ones at the net's sizes
    assert shapes(case["K"]) == _ffi_grid.grid_param_shapes(case["K"], **sizes)
    assert a.tobytes() == _ffi_grid.default_init_grid(case["seed"], case["K"], **sizes).tobytes()


def test_defaults_kept():
    for kind in RECORDED:
        init, shapes, _ = _functions(kind)
        first = RECORDED[kind][0]      # the recorded first case is the functions' defaults: seed 3, K = 51 / 17
        assert hashlib.sha256(init().tobytes()).hexdigest() == first["sha256"]
        assert [[n, list(s)] for n, s in shapes()] == first["shapes"]
