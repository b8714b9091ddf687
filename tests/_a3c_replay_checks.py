"""What a recorded rollout of an A3C net says about its acting, as the test_rollout_replay tests of test_gpu_gaussnet.py,
test_gpu_gatednet.py and test_gpu_discretenet.py state it: the recorded draws, choices and env actions are what the oracle's
act / choose give from the device's OWN recorded float32 heads and the oracle's Philox draws.  r: dict of read_rollout arrays."""
import numpy as np

import _gated_oracle as G
import _gauss_oracle as A
import _grid_oracle as D


def gauss_acting(r, seed, env_ids, counter0, tanh_action, stride=37):
    """raw rebuilt from the recorded mu / sigma, bit-equal; the env action is the worker's sigmoid / tanh of it, to float32"""
    T, E, Aa = r["raw"].shape
    acts = r["actions"]                   # what the envs were stepped with, as the device computed it
    for t in range(T):
        nz = A.draws(seed, env_ids, counter0 + t, Aa)
        raw = (r["mu"][t].astype(np.float64) + r["sigma"][t].astype(np.float64) * nz).astype(np.float32)
        assert np.array_equal(raw, r["raw"][t]), t
        for e in range(0, E, stride):
            raw1, ea = A.act(r["mu"][t, e], r["sigma"][t, e], nz[e], tanh_action=tanh_action)
            assert np.array_equal(raw1, r["raw"][t, e]), (t, e)
            np.testing.assert_allclose(acts[t, e], ea, rtol=1e-6, atol=0)      # the worker's sigmoid / tanh of the raw draw, to float32
    assert (np.abs(acts) <= 1).all() and (tanh_action or (acts >= 0).all())


def gated_acting(r, seed, env_ids, counter0, stride=37):
    """choices and raw rebuilt from the recorded probs / mu / sigma"""
    T, E = r["choices"].shape[:2]
    for t in range(T):
        u, nz = G.draws(seed, env_ids, counter0 + t)
        for e in range(0, E, stride):
            ch, raw, _ = G.act(r["probs"][t, e], r["mu"][t, e], r["sigma"][t, e], u[e], nz[e])
            assert np.array_equal(ch, r["choices"][t, e]), (t, e)
            assert np.array_equal(raw, r["raw"][t, e]), (t, e)


def discrete_acting(r, seed, env_ids, counter0, K):
    """the sampler on the device's OWN float32 probabilities and the oracle's u: exact.  (On the oracle's probabilities a u within
    1e-7 of a cumulative sum would make a correct kernel fail.)"""
    T, E = r["choices"].shape
    for t in range(T):
        u = D.draws(seed, env_ids, counter0 + t)
        want = np.array([D.choose(r["probs"][t, e], u[e]) for e in range(E)])
        assert np.array_equal(r["choices"][t], want), t
    assert np.array_equal(r["actions"], D.grid(K)[r["choices"]].astype(np.float32))
