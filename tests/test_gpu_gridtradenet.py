"""GPU: the A3C grid trader (csrc/net_gridtrade.hip through include/goldsrl_gridtradenet.h) against the float64 restatement
tests/_gridtrade_oracle.py -- predict, the host-sample update, the rollout's replay (both draws, the grid, the env, the GAE), the
rollout update against the host update, the one-launch evaluation against the greedy per-step rollout, the refusals.

Bounds: the project's forward bounds (rtol 5e-5, atol 5e-6) and GRAD_REL_BOUND of tests/test_gpu_discretenet.py (1e-6 policy, 3e-7
value, of the block's largest oracle entry plus the gradient's largest).  Measured on the MI355X against the float64 oracle
(n = 130, R = 5, _samples(K, 130, 5, 11)), worst block:
  K = 2   1.41e-7 (policy, static1_w)  / 1.88e-7 (value, static2_b)
  K = 17  1.25e-7 (policy, temporal_b) / 5.86e-8 (value, value2_w)
  K = 48  1.13e-7 (policy, temporal_b) / 5.64e-8 (value, value2_b)
The two-output head sums twice the terms of the savings-grid net's and stays inside its bounds, so they are unchanged.
"""
import numpy as np
import pytest

import _gridtrade_oracle as GT
from test_gpu_discretenet import FWD_ATOL, FWD_RTOL, GRAD_REL_BOUND

pytestmark = pytest.mark.gpu
KS = (2, 17, 48)
NEAR_DEPLETION = dict(trade_starting_balance=1.02, trade_std_p=0.3)      # episodes end terminally within a few steps


def _engine(E, n_assets=2, **kw):
    from goldsrl import _ffi
    eng = _ffi.Engine(_ffi.ENV_TRADE, E, n_assets=n_assets, **dict(dict(seed=7), **kw))
    eng.reset()
    return eng


def _net(eng, **kw):
    from goldsrl import _ffi_gridtrade
    return _ffi_gridtrade.GridTradeNet(eng, **dict(dict(max_samples=256), **kw))


def _params(K, seed=5):
    p = GT.init(seed, K)
    rng = np.random.RandomState(seed)
    for k in p:
        if k.endswith("_b"):
            p[k] = p[k] + 0.05 * rng.normal(size=p[k].shape)
    p["probs3_w"] = p["probs3_w"] * 4.0          # logits a few units apart: not a near-uniform row
    return GT.flatten(p).astype(np.float32)


def _samples(K, n, R, seed=0):
    """windows of every true length 0..R, weights with zeros, advantages of both signs; the choices hit 0 and K - 1 in both
    outputs and differ between the outputs"""
    rng = np.random.RandomState(seed)
    win = rng.normal(size=(n, R, 5)).astype(np.float32)
    for i in range(n):
        win[i, (i + seed) % (R + 1):] = 0.0
    ch = rng.randint(0, K, size=(n, 2)).astype(np.int32)
    ch[:2] = [[0, K - 1], [K - 1, 0]]
    w = np.where(rng.uniform(size=n) > 0.25, rng.uniform(0.5, 1.5, size=n), 0.0).astype(np.float32)
    w[:2] = 1.0
    return rng.normal(size=(n, 5)).astype(np.float32), win, ch, rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32), w


def _as64(K, flat):
    return GT.unflatten(np.asarray(flat, np.float32).astype(np.float64), K)


@pytest.fixture(scope="module")
def eng():
    e = _engine(65)
    yield e
    e.close()


@pytest.mark.parametrize("R", [1, 20])
@pytest.mark.parametrize("K", KS)
def test_predict_matches_oracle(eng, K, R):
    net = _net(eng, rnn_length=R, scale=3.0, num_choices=K)
    assert net.num_params == GT.num_params(K) == 91041 + 258 * K
    flat = _params(K)
    net.set_params(flat)
    s, w = _samples(K, 130, R, seed=3)[:2]
    empty = (np.arange(130) + 3) % (R + 1) == 0
    assert empty.any() and not w[empty].any()                             # windows of zero rows are among them
    got = net.predict(s, w)
    probs, values = GT.forward(_as64(K, flat), s, w, 3.0)
    assert got["probs"].shape == (130, 2, K) and got["probs"].dtype == np.float32
    np.testing.assert_allclose(got["probs"], probs, rtol=FWD_RTOL, atol=FWD_ATOL)
    np.testing.assert_allclose(got["values"], values, rtol=FWD_RTOL, atol=FWD_ATOL)
    assert np.abs(got["probs"].astype(np.float64).sum(2) - 1.0).max() < 1e-6
    net.close()


def _block_err(K, got, ref):
    gmax = np.abs(ref).max()
    errs = {b: np.abs(got[lo:hi] - ref[lo:hi]).max() / (np.abs(ref[lo:hi]).max() + gmax) for b, (lo, hi) in GT.block_ranges(K).items()}
    worst = max(errs, key=errs.get)
    return errs[worst], worst


@pytest.mark.parametrize("K", KS)
def test_host_train_gradients_and_update(eng, K):
    n, R, mult = 130, 5, 0.3
    P = GT.num_params(K)
    net = _net(eng, rnn_length=R, clip_norm=0.5, num_choices=K)
    flat = _params(K)
    net.set_params(flat)
    net.set_optimizer_state(np.ones(P, np.float32), np.ones(P, np.float32), 200000)
    s, w, ch, adv, tgt, wt = _samples(K, n, R, seed=11)
    assert (wt == 0).any() and (ch[:, 0] != ch[:, 1]).any() and {0, K - 1} <= set(ch[:, 0]) and {0, K - 1} <= set(ch[:, 1])
    stats = net.train(s, w, ch, adv, tgt, wt, grad_mult=mult, lr=1e-3, apply_update=False)
    gp, gv = net.get_grads("policy"), net.get_grads("value")
    (pl, vl, ent), rp, rv = GT.grads(_as64(K, flat), s, w, ch, adv, tgt, wt, mult)
    rp, rv = GT.flatten(rp), GT.flatten(rv)
    (ep, bp), (ev, bv) = _block_err(K, gp, rp), _block_err(K, gv, rv)
    print("K=%d worst block error: policy %.3g (%s), value %.3g (%s)" % (K, ep, bp, ev, bv))
    assert ep < GRAD_REL_BOUND["policy"] and ev < GRAD_REL_BOUND["value"], (ep, bp, ev, bv)
    np.testing.assert_allclose([stats["policy_loss"], stats["value_loss"], stats["entropy_mean"]], [pl, vl, ent], rtol=1e-4)
    # a head that reads output 0's choice for both outputs is outside the bound
    _, mp, _ = GT.grads(_as64(K, flat), s, w, ch[:, [0, 0]], adv, tgt, wt, mult)
    assert _block_err(K, GT.flatten(mp), rp)[0] > GRAD_REL_BOUND["policy"]
    # clip (0.5 on each gradient) + both RMSProp steps + the lr decay, on the device's own gradient
    net.train(s, w, ch, adv, tgt, wt, grad_mult=mult, lr=1e-3, apply_update=True)
    st = net.get_optimizer_state()
    w_ref, msp, msv = GT.apply_update(flat.astype(np.float64), gp.astype(np.float64), gv.astype(np.float64), np.ones(P), np.ones(P), 200000,
                                      1e-3, K, clip=0.5)[:3]
    assert st["global_step"] == 200002
    np.testing.assert_allclose(net.get_params(), w_ref, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(st["ms_policy"], msp, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(st["ms_value"], msv, rtol=1e-6, atol=1e-12)
    net.close()


def test_rollout_replay_and_rollout_update():
    from goldsrl import _ffi
    E, T, R, K, scale = 65, 6, 3, 17, 2.0
    kw = dict(seed=21, max_episode_steps=4, env_id_offset=1000)           # episodes end inside the rollout
    P = GT.num_params(K)
    flat = _params(K, 4)

    def run():
        eng = _engine(E, **kw)
        net = _net(eng, rnn_length=R, scale=scale, num_choices=K, max_samples=T * E)
        net.set_params(flat)
        net.set_action_counter(1000)
        net.rollout(T)
        return eng, net
    eng, net = run()
    r = {k: net.read_rollout(k) for k in ("states", "windows", "probs", "choices", "actions", "values", "rewards", "dones", "weights", "adv",
                                          "targets", "boot")}
    assert net.get_action_counter() == 1000 + T and r["choices"].dtype == np.int32 and r["choices"].shape == (T, E, 2)
    # both draws on the device's OWN float32 probabilities and the oracle's uniforms: integer equality; the grid's float32 values
    for t in range(T):
        u = GT.draws(eng.cfg.seed, np.arange(E) + 1000, 1000 + t)
        want = [[GT.choose(r["probs"][t, e, o], u[o][e]) for o in range(2)] for e in range(E)]
        assert np.array_equal(r["choices"][t], want), t
    assert np.array_equal(r["actions"].view(np.uint32), GT.grid(K)[r["choices"]].astype(np.float32).view(np.uint32))
    assert (r["choices"][..., 0] != r["choices"][..., 1]).any() and net.grid[K // 2] == 0.0
    # rewards and dones: the per-step grl_step path on a second handle fed the same actions
    twin = _engine(E, **kw)
    for t in range(T):
        twin.step(r["actions"][t])
        assert np.array_equal(twin.read("reward"), r["rewards"][t]) and np.array_equal(twin.read("done"), r["dones"][t] > 0), t
    twin.close()
    assert r["dones"][3].all()
    probs, values = GT.forward(_as64(K, flat), r["states"].reshape(-1, 5), r["windows"].reshape(-1, R, 5), scale)
    np.testing.assert_allclose(r["probs"].reshape(-1, 2, K), probs, rtol=FWD_RTOL, atol=FWD_ATOL)
    win, wts = GT.replay_windows(r["states"], r["dones"], R)
    assert np.array_equal(r["windows"], win) and np.array_equal(r["weights"], wts)
    adv, tgt = GT.gae_segments(r["rewards"], r["values"], r["boot"], r["dones"], None, False, 0.99, 0.96, scale)
    np.testing.assert_allclose(r["adv"], adv, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["targets"], tgt, rtol=1e-5, atol=1e-6 * scale)
    # train_rollout is train on the read-back rollout with grad_mult = 1 / E, bit for bit; two identical runs give identical bytes
    net.train_rollout(lr=1e-3)
    g_ro, p_ro = (net.get_grads("policy"), net.get_grads("value")), net.get_params()
    net.set_params(flat)
    net.set_optimizer_state(np.ones(P, np.float32), np.ones(P, np.float32), 0)
    net.train(r["states"].reshape(-1, 5), r["windows"].reshape(-1, R, 5), r["choices"].reshape(-1, 2), r["adv"].reshape(-1),
              r["targets"].reshape(-1), r["weights"].reshape(-1), grad_mult=1.0 / E, lr=1e-3)
    assert np.array_equal(net.get_grads("policy"), g_ro[0]) and np.array_equal(net.get_grads("value"), g_ro[1]) and g_ro[0].any()
    assert np.array_equal(net.get_params(), p_ro) and not np.array_equal(p_ro, flat)
    eng2, net2 = run()
    net2.train_rollout(lr=1e-3)
    assert np.array_equal(net2.get_params(), p_ro)
    # a choice outside the grid is refused, not clamped
    bad = r["choices"].reshape(-1, 2).copy(); bad[5, 1] = K
    with pytest.raises(_ffi.GrlError, match="a choice outside") as ei:
        net.train(r["states"].reshape(-1, 5), r["windows"].reshape(-1, R, 5), bad, r["adv"].reshape(-1), r["targets"].reshape(-1))
    assert ei.value.code == _ffi.E_INVALID
    net.close(); eng.close(); net2.close(); eng2.close()


def test_eval_is_the_greedy_rollout_bit_for_bit():
    E, CAP, R, K = 65, 16, 5, 17
    trace = ("states", "choices", "actions", "rewards", "dones")
    flat = _params(K, 7)

    def pair():
        eng = _engine(E, seed=1692, max_episode_steps=CAP, **NEAR_DEPLETION)
        eng.set_state("ELAPSED", ((np.arange(E) * 7) % CAP).astype(np.int32))      # the step cap ends a wave's episodes on different steps
        net = _net(eng, rnn_length=R, num_choices=K, max_samples=1)
        net.set_params(flat)
        return eng, net
    eng, net = pair()
    ev = net.eval(2 * CAP, trace_steps=2 * CAP)
    assert (eng.get_state("ELAPSED") == 0).all() and net.get_action_counter() == 0 and np.array_equal(net.get_params(), flat)
    eng2, twin = pair()
    twin.set_greedy(True)
    twin.rollout(CAP)
    ro = {k: twin.read_rollout(k) for k in trace}
    d = ro["dones"] > 0
    n = d.argmax(axis=0) + 1
    assert d.any(axis=0).all() and np.array_equal(ev["length"], n) and (ev["finished"] == 1).all() and len(np.unique(n)) >= 4
    for e in range(E):
        total = 0.0
        for v in ro["rewards"][:n[e], e]:
            total += float(v)                                              # total_reward += reward, float64
        assert ev["total_reward"][e] == total, e
        for k in trace:
            np.testing.assert_array_equal(ev[k][:n[e], e], ro[k][:n[e], e], err_msg="%s env %d" % (k, e))
    assert len(np.unique(ev["choices"])) >= 2
    for p in ((eng, net), (eng2, twin)):
        p[1].close(); p[0].close()


def test_refusals(eng):
    from goldsrl import _ffi, _ffi_gridtrade
    solow, three = _ffi.Engine(_ffi.ENV_SOLOW, 4), _ffi.Engine(_ffi.ENV_TRADE, 4, n_assets=3)
    for e, kw, msg in ((solow, {}, "needs a TradeAR1 handle"), (three, {}, "num_outputs 2 and the handle's 3 assets"),
                       (eng, dict(num_outputs=3), "num_outputs 3 and the handle's 2 assets"), (eng, dict(num_choices=49), r"2\.\.48"),
                       (eng, dict(num_choices=1), r"2\.\.48"), (eng, dict(always_bootstrap=1), "always_bootstrap = 0")):
        with pytest.raises(_ffi.GrlError, match=msg) as ei:
            _ffi_gridtrade.GridTradeNet(e, **kw)
        assert ei.value.code == _ffi.E_INVALID
    solow.close(); three.close()
    # the estimator facade binds two outputs to this net and one output to the savings-grid net only
    from goldsrl.agents.a3c import estimators as est
    net = _net(eng, rnn_length=5)
    s, w = _samples(17, 4, 5)[:2]
    pol = est.DiscretePolicyEstimator(2, 17, static_size=5, temporal_size=5, net=net)
    assert np.array_equal(pol.predict(s, w, batch=True)["probs"], net.predict(s, w)["probs"])
    assert est.ValueEstimator(static_size=5, temporal_size=5, net=net).predict(s, w, batch=True)["logits"].shape == (4,)
    with pytest.raises(ValueError):
        est.DiscretePolicyEstimator(1, 17, static_size=5, temporal_size=5, net=net)
    net.close()
