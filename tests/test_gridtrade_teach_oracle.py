"""CPU: tests/_gridtrade_teach_oracle.py, the float64 yardstick of the grid trader's supervised update -- its analytic gradient is the
central difference of its own cross-entropy; goldsrl._ffi_gridtrade.trade_grid_labels at the grid's ends, a point and a midpoint;
include/goldsrl_gridtradeteach.h declares what libgoldsrl.so exports and _ffi_gridtrade binds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _gridtrade_oracle as GT
import _gridtrade_teach_oracle as TT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K", [2, 17])
def test_gradient_is_the_central_difference_of_the_cross_entropy(K):
    """h = 1e-6 and the bound 1e-8 + 1e-6 |gradient| of tests/test_gridtrade_oracle.py, for its reasons: rounding 2e-10 per
    evaluation, truncation 1e-12.  Labels with w = 0, 0.3 and 1, differing between the outputs; the largest and two more entries of
    every block of the policy gradient."""
    n, R, h = 6, 3, 1e-6
    p = GT.init(6, K)
    rng = np.random.RandomState(K)
    for k in p:
        if k.endswith("_b"):
            p[k] = p[k] + 0.05 * rng.normal(size=p[k].shape)
    p["probs3_w"] = p["probs3_w"] * 4.0
    win = rng.normal(size=(n, R, 5))
    for i in range(n):
        win[i, (i + 1) % (R + 1):] = 0.0
    lo = rng.randint(0, K - 1, size=(n, 2))
    lo[0] = [0, K - 2]
    w = np.array([[0.0, 0.3], [0.3, 1.0], [1.0, 0.0], [0.3, 0.3], [0.0, 1.0], [1.0, 0.3]], np.float32)
    wt = np.array([1.0, 0.7, 0.0, 1.3, 1.0, 0.5])
    args = (rng.normal(size=(n, 5)), win, lo, w, rng.normal(size=n), wt, 0.7, 2.0)
    (ce, _, _, agree), gp, gv = TT.grads(p, *args)
    assert ce > 0 and 0.0 <= agree <= 1.0 and not any(gp[k].any() for k in p if k.startswith("value"))
    for k in (k for k in p if not k.startswith("value")):
        flat = gp[k].reshape(-1)
        assert np.abs(flat).max() > 1e-4, k
        for i in {int(np.abs(flat).argmax()), int(rng.randint(flat.size)), int(rng.randint(flat.size))}:
            q = {m: v.copy() for m, v in p.items()}
            q[k].reshape(-1)[i] += h
            up = TT.losses(q, *args)[0]
            q[k].reshape(-1)[i] -= 2 * h
            fd = (up - TT.losses(q, *args)[0]) / (2 * h)
            assert abs(fd - flat[i]) <= 1e-8 + 1e-6 * abs(flat[i]), (k, i, fd, flat[i])
    # w = 0 everywhere: the A3C gradient with advantage 1 and choice = lo
    _, g0, _ = TT.grads(p, args[0], win, lo, np.zeros((n, 2), np.float32), *args[4:])
    _, ga, _ = GT.grads(p, args[0], win, lo, np.ones(n), *args[4:])
    assert all(np.allclose(g0[k], ga[k], rtol=1e-12, atol=1e-15) for k in p)


def test_labels_at_the_ends_a_point_and_a_midpoint():
    from goldsrl._ffi_gridtrade import trade_grid_labels
    K = 17                                                     # step 0.125 on [-1, 1]: every case below is exact
    lo, w = trade_grid_labels(np.float32([-1.0, 1.0, 0.25, 0.3125, -2.0, 2.0]), K)
    assert lo.dtype == np.int32 and w.dtype == np.float32
    assert lo.tolist() == [0, K - 2, 10, 10, 0, K - 2] and w.tolist() == [0.0, 1.0, 0.0, 0.5, 0.0, 1.0]
    lo, w = trade_grid_labels(np.float32([[-1.0, 0.5]]), 2)
    assert lo.tolist() == [[0, 0]] and w.tolist() == [[0.0, 0.75]]
    grid = np.linspace(-1.0, 1.0, K)
    a = np.random.RandomState(0).uniform(-1, 1, 50).astype(np.float32)
    lo, w = trade_grid_labels(a, K)
    np.testing.assert_allclose((1 - w) * grid[lo] + w * grid[lo + 1], a, atol=1e-7)      # the label's mean is the action


def test_header_declared_exported_and_bound():
    from goldsrl import _ffi, _ffi_gridtrade
    raw = open(os.path.join(ROOT, "include", "goldsrl_gridtradeteach.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))
    sig = _ffi_gridtrade.GTNET_TEACH_SIGNATURES
    assert declared == set(sig) == {"grl_gtnet_teach_rollout", "grl_gtnet_train_teach_rollout", "grl_gtnet_teach"}
    assert not declared & (set(_ffi_gridtrade.GTNET_SIGNATURES) | set(_ffi_gridtrade.GTNET_EVAL_SIGNATURES))
    assert '#include "goldsrl_gridtradenet.h"' in text and "NO counterpart" in raw
    lib = _ffi.load_library(extra_signatures=sig)
    kinds = {"int32_t": C.c_int32, "float": C.c_float, "double": C.c_double}
    for name, (restype, argtypes) in sig.items():
        assert hasattr(lib, name), "include/goldsrl_gridtradeteach.h declares %s but libgoldsrl.so does not export it" % name
        args = [a.strip() for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text).group(1).split(",")]
        assert restype is C.c_int and list(argtypes) == [C.c_void_p if "*" in a else kinds[a.split()[0]] for a in args], name
    assert lib.grl_gtnet_teach_rollout(None, 4, 0.0) == _ffi.E_INVALID and lib.grl_gtnet_train_teach_rollout(None, 1e-4, None) == _ffi.E_INVALID
    assert all(hasattr(_ffi_gridtrade.GridTradeNet, m) for m in ("teach_rollout", "train_teach_rollout", "teach"))
