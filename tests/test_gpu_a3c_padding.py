"""GPU: the lanes a 64-sample workgroup of the three A3C nets has past the last sample are inert (csrc/net_a3c_core.inc: the shared trunk
reads a real sample's rows for them, the kernels give them weight 0).  70 samples are one full group and a group of 6; the same 70
followed by 58 OTHER samples of weight 0 fill both groups.  Both runs are two workgroups with the same slab order, padded and
weight-0 lanes only ever add +-0 to a sum, so everything the 70 produce is equal bit for bit -- no tolerance."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, FULL, R, K = 70, 128, 5, 64


def _make(kind):
    from goldsrl import _ffi, _ffi_discrete, _ffi_gated, _ffi_gauss
    if kind == "discrete":
        eng = _ffi.Engine(_ffi.ENV_SOLOW, 4, seed=7)
        net = _ffi_discrete.DiscreteNet(eng, rnn_length=R, max_samples=FULL, num_choices=K)
        net.set_params(_ffi_discrete.default_init_discrete(5, K))
        return eng, net, 2, 2, 1
    if kind == "gated":
        eng = _ffi.Engine(_ffi.ENV_TICKER, 4, seed=7)
        eng.ticker_set_table(np.load(os.path.join(ROOT, "tests", "golden", "ticker.npz"))["matrix"])
        net = _ffi_gated.GatedNet(eng, rnn_length=R, max_samples=FULL)
        net.set_params(_ffi_gated.default_init_gated(5))
        return eng, net, 7, 4, 2
    sizes = _ffi_gauss.SOLOW_SIZES if kind == "solow" else _ffi_gauss.TRADE_SIZES
    eng = _ffi.Engine(_ffi.ENV_SOLOW, 4, seed=7) if kind == "solow" else _ffi.Engine(_ffi.ENV_TRADE, 4, seed=7, n_assets=2)
    net = _ffi_gauss.GaussNet(eng, rnn_length=R, max_samples=FULL)
    net.set_params(_ffi_gauss.default_init_gauss(5, **sizes))
    return eng, net, sizes["static_size"], sizes["temporal_size"], sizes["num_actions"]


@pytest.mark.parametrize("kind", ["gated", "solow", "trade", "discrete"])
def test_lanes_past_the_last_sample_are_inert(kind):
    eng, net, S0, D, A = _make(kind)
    rng = np.random.RandomState(11)
    states = rng.normal(size=(FULL, S0)).astype(np.float32)
    win = rng.normal(size=(FULL, R, D)).astype(np.float32)
    for i, n in enumerate(rng.randint(1, R + 1, size=FULL)):      # every window length, zero rows behind it
        win[i, n:] = 0.0
    raw = rng.normal(size=(FULL, A)).astype(np.float32)
    adv, tgt = rng.normal(size=FULL).astype(np.float32), rng.normal(size=FULL).astype(np.float32)
    wt = (rng.uniform(size=FULL) > 0.25).astype(np.float32)
    wt[N - 1] = 1.0
    wt[N:] = 0.0
    extra = (rng.randint(0, 3, size=(FULL, 2)).astype(np.int32),) if kind == "gated" else ()
    heads = extra + (raw,)
    if kind == "discrete":      # its only head input is the choice
        heads = (rng.randint(0, K, size=FULL).astype(np.int32),)

    few, full = net.predict(states[:N], win[:N]), net.predict(states, win)
    assert sorted(few) == sorted(full)
    for k in few:
        assert np.array_equal(few[k], full[k][:N]), k

    def train(n):
        st = net.train(states[:n], win[:n], *[a[:n] for a in heads + (adv, tgt)], weights=wt[:n], apply_update=False)
        return st, net.get_grads("policy"), net.get_grads("value")

    (st_few, gp_few, gv_few), (st_full, gp_full, gv_full) = train(N), train(FULL)
    net.close(); eng.close()
    assert np.abs(gp_few).max() > 0 and np.abs(gv_few).max() > 0
    assert np.array_equal(gp_few, gp_full) and np.array_equal(gv_few, gv_full)
    assert st_few["policy_loss"] == st_full["policy_loss"] and st_few["value_loss"] == st_full["value_loss"]
