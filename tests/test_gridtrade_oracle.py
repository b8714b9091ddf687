"""CPU: tests/_gridtrade_oracle.py, the float64 yardstick of the grid trader's GPU tests -- at D = 2, O = 1 it is
tests/_grid_oracle.py exactly, and at D = 5, O = 2 its analytic gradients are the central differences of its own losses."""
import numpy as np

import _grid_oracle as D1
import _gridtrade_oracle as GT


def _samples(n, R, D, O, K, seed):
    rng = np.random.RandomState(seed)
    win = rng.normal(size=(n, R, D))
    for i in range(n):
        win[i, (i + 1) % (R + 1):] = 0.0                 # true lengths 1, 2, .., R, 0, ..
    wt = np.where(np.arange(n) % 4 == 2, 0.0, rng.uniform(0.5, 1.5, size=n))
    return rng.normal(size=(n, D)), win, rng.randint(0, K, size=(n, O)), rng.normal(size=n), rng.normal(size=n), wt


def test_one_output_on_solow_sizes_is_the_grid_oracle_exactly():
    K = 7
    p = D1.init(4, K)
    assert [n for n, _ in GT.param_shapes(K, 2, 1)] == D1.names(K) and GT.num_params(K, 2, 1) == D1.num_params(K)
    assert GT.num_params(17) == 95427 and GT.num_params(3) == 91041 + 258 * 3
    s, w, ch, adv, tgt, wt = _samples(9, 4, 2, 1, K, 1)
    ref, got = D1.grads(p, s, w, ch[:, 0], adv, tgt, wt, 0.3, 2.0), GT.grads(p, s, w, ch, adv, tgt, wt, 0.3, 2.0, O=1)
    assert got[0] == ref[0]
    for a, b in zip(got[1:], ref[1:]):
        assert all(np.array_equal(a[k], b[k]) for k in p)
    assert np.array_equal(GT.forward(p, s, w, 2.0, O=1)[0][:, 0], D1.forward(p, s, w, 2.0)[0])


def test_two_output_gradients_are_the_central_differences_of_the_losses():
    """Step h = 1e-6 on parameters of size 0.1 .. 1 and losses of size 1: the truncation error is h^2 f''' / 6 ~ 1e-12, the rounding
    error eps |loss| / h ~ 2e-16 / 1e-6 = 2e-10 per evaluation.  Bound: 1e-8 + 1e-6 |gradient|, fifty times the rounding error and
    far below a missing term (the smallest block's largest entry is above 1e-3).  Three entries of every block are tried, among
    them the largest of the analytic gradient."""
    K, D, O, h = 3, 5, 2, 1e-6
    p = GT.init(6, K, D, O)
    rng = np.random.RandomState(6)
    for k in p:                          # no bias at exactly 0: an empty window would put dense_temporal on the ReLU's kink
        if k.endswith("_b"):
            p[k] = p[k] + 0.05 * rng.normal(size=p[k].shape)
    p["probs3_w"] = p["probs3_w"] * 4.0
    s, w, ch, adv, tgt, wt = _samples(10, 3, D, O, K, 2)
    assert (ch[:, 0] != ch[:, 1]).any() and (wt == 0).any()
    args = (s, w, ch, adv, tgt, wt, 0.7, 2.0, O)
    _, gp, gv = GT.grads(p, *args)
    rng = np.random.RandomState(0)
    for which, g in ((0, gp), (1, gv)):
        for k in p:
            flat = g[k].reshape(-1)
            for i in {int(np.abs(flat).argmax()), int(rng.randint(flat.size)), int(rng.randint(flat.size))}:
                q = {n: v.copy() for n, v in p.items()}
                q[k].reshape(-1)[i] += h
                up = GT.losses(q, *args)[which]
                q[k].reshape(-1)[i] -= 2 * h
                fd = (up - GT.losses(q, *args)[which]) / (2 * h)
                assert abs(fd - flat[i]) <= 1e-8 + 1e-6 * abs(flat[i]), (which, k, i, fd, flat[i])
    assert all(np.abs(gp[k]).max() > 1e-3 for k in p if not k.startswith("value")) and not any(gp[k].any() for k in p if k.startswith("value"))
    assert not any(gv[k].any() for k in p if k.startswith("probs"))
