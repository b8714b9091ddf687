"""GPU: the A3C Gaussian agent (csrc/net_gauss.hip through include/goldsrl_gaussnet.h) against the float64 restatement
tests/_gauss_oracle.py, on both size sets (Solow, TradeAR1 with 2 assets) -- predict, the host-sample update, the device-resident
rollout + update against the single-worker update, the terminal bootstrap, the rollout's replay against oracle/oracle.py's env
steps and the Philox draws, consistency (host vs rollout path, bitwise reproducibility, checkpoints), the direction of one update,
the bench-size update, both training scripts and the estimator facades."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _a3c_replay_checks as RC
import _gauss_oracle as A
from oracle import oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS = ("solow", "trade")
SIZES = {"solow": A.SOLOW, "trade": A.TRADE}

# Per-block bound of |device - oracle| on the gradients, relative to the block's largest oracle entry plus the largest entry of the
# whole gradient (blocks that are nearly zero carry only rounding).  The starting point is the gated trader's bounds
# (test_gpu_gatednet.py: 1e-6 on host samples, 2e-4 at bench size, forward rtol 2e-4 / atol 2e-5), whose arithmetic this net
# shares; each bound here is at most 10x the figure measured on the MI355X against the float64 oracle and never looser than those:
#   host samples (n = 1 000, R = 5, _samples(kind, 1000, 5, 11)):
#     solow  worst block 1.68e-7 (policy, sigma3_b) / 3.98e-8 (value, temporal_b)
#     trade  worst block 5.00e-7 (policy, mu3_b)    / 5.31e-8 (value, static2_b)
#   bench size (8 192 envs x 20 steps, one rollout) -- sums of 163 840 terms that largely cancel, accumulated in fp32 over 256 slabs:
#     solow  worst block 3.40e-6 (policy, sigma1_b) / 5.72e-8 (value, value2_b)
#     trade  worst block 7.03e-5 (policy, mu1_b)    / 3.10e-8 (value, value2_w)
#   forward (predict at n = 1 .. 1 000, R = 5 and 20, scale 3), worst |device - oracle| / (2e-5 + 2e-4 |oracle|):
#     solow  0.0060 (mu) 0.0008 (sigma) 0.017 (values);  trade  0.037 (mu) 0.0011 (sigma) 0.019 (values)
#     so a quarter of the gated bound (rtol 5e-5, atol 5e-6) is 6.8x the worst measured figure
GRAD_REL_BOUND = {"policy": 1e-6, "value": 3e-7}
BENCH_REL_BOUND = {"solow": {"policy": 3e-5, "value": 3e-7}, "trade": {"policy": 2e-4, "value": 3e-7}}
FWD_RTOL, FWD_ATOL = 5e-5, 5e-6


def _engine(kind, E, seed=7, **kw):
    from goldsrl import _ffi
    if kind == "solow":
        eng = _ffi.Engine(_ffi.ENV_SOLOW, E, seed=seed, **kw)
    else:
        eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=seed, n_assets=2, **kw)
    eng.reset()
    return eng


def _net(eng, **kw):
    from goldsrl import _ffi_gauss
    kw.setdefault("max_samples", 8192)
    return _ffi_gauss.GaussNet(eng, **kw)


def _params(kind, seed=5):
    p = A.init(seed, **SIZES[kind])
    rng = np.random.RandomState(seed)
    for k in p:
        if k.endswith("_b"):
            p[k] = p[k] + 0.05 * rng.normal(size=p[k].shape)
    return A.flatten(p).astype(np.float32)


def _samples(kind, n, R, seed=0):
    D, Aa = SIZES[kind]["static_size"], SIZES[kind]["num_actions"]
    rng = np.random.RandomState(seed)
    states = rng.normal(size=(n, D)).astype(np.float32)
    win = rng.normal(size=(n, R, D)).astype(np.float32)
    lens = rng.randint(1, R + 1, size=n)
    for i in range(n):
        win[i, lens[i]:] = 0.0
    raw = rng.normal(size=(n, Aa)).astype(np.float32)
    adv = rng.normal(size=n).astype(np.float32)
    tgt = rng.normal(size=n).astype(np.float32)
    w = (rng.uniform(size=n) > 0.25).astype(np.float32)
    return states, win, raw, adv, tgt, w


def _as64(kind, flat):
    return A.unflatten(np.asarray(flat, np.float32).astype(np.float64), **SIZES[kind])


@pytest.fixture(scope="module")
def engs():
    e = {k: _engine(k, 64) for k in KINDS}
    yield e
    for v in e.values():
        v.close()


@pytest.mark.parametrize("R", [5, 20])
@pytest.mark.parametrize("kind", KINDS)
def test_predict_matches_oracle(engs, kind, R):
    net = _net(engs[kind], rnn_length=R, scale=3.0)
    flat = _params(kind)
    net.set_params(flat)
    p = _as64(kind, flat)
    worst = {}
    for n in (1, 63, 64, 65, 1000):
        s, w = _samples(kind, n, R, seed=n)[:2]
        got = net.predict(s, w)
        ref = A.forward(p, s.astype(np.float64), w.astype(np.float64), 3.0)
        for k, r in zip(("mu", "sigma", "values"), ref):
            assert got[k].shape == r.shape
            # |device - oracle| over the bound atol + rtol |oracle| of assert_allclose
            worst[k] = max(worst.get(k, 0.0), float((np.abs(got[k] - r) / (FWD_ATOL + FWD_RTOL * np.abs(r))).max()))
    print("predict %s R=%d: worst error / bound %s" % (kind, R, {k: "%.3g" % v for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), worst
    net.close()


def _block_err(kind, got, ref):
    """max over blocks of |got - ref|_inf / bound_scale, and the worst block's name"""
    gmax = np.abs(ref).max()
    worst, name = 0.0, None
    for b, (lo, hi) in A.block_ranges(**SIZES[kind]).items():
        scale = np.abs(ref[lo:hi]).max() + gmax
        e = np.abs(got[lo:hi] - ref[lo:hi]).max() / scale
        if e > worst:
            worst, name = e, b
    return worst, name


@pytest.mark.parametrize("kind", KINDS)
def test_host_train_gradients_clip_and_rmsprop(engs, kind):
    n, R = 1000, 5
    sizes = SIZES[kind]
    P = A.num_params(**sizes)
    net = _net(engs[kind], rnn_length=R, clip_norm=0.5)
    assert net.num_params == P
    flat = _params(kind)
    net.set_params(flat)
    net.set_optimizer_state(np.ones(P, np.float32), np.ones(P, np.float32), 200000)
    s, w, raw, adv, tgt, wt = _samples(kind, n, R, seed=11)
    mult = 0.3
    stats = net.train(s, w, raw, adv, tgt, wt, grad_mult=mult, lr=1e-3, apply_update=False)
    gp, gv = net.get_grads("policy"), net.get_grads("value")
    args64 = [a.astype(np.float64) for a in (s, w)]
    (pl, vl, ent), rp, rv = A.grads(_as64(kind, flat), *args64, raw, adv, tgt, wt, mult)
    rp, rv = A.flatten(rp), A.flatten(rv)
    ep, bp = _block_err(kind, gp, rp)
    ev, bv = _block_err(kind, gv, rv)
    print("%s worst block error: policy %.3g (%s), value %.3g (%s)" % (kind, ep, bp, ev, bv))
    assert ep < GRAD_REL_BOUND["policy"] and ev < GRAD_REL_BOUND["value"], (ep, bp, ev, bv)
    assert not gp[~A.policy_mask(**sizes)].any() and not gv[~A.value_mask(**sizes)].any()
    np.testing.assert_allclose([stats["policy_loss"], stats["value_loss"], stats["entropy_mean"]], [pl, vl, ent], rtol=1e-4)
    np.testing.assert_allclose([stats["policy_norm"], stats["value_norm"]], [np.linalg.norm(rp), np.linalg.norm(rv)], rtol=1e-4)
    # the bound is tight enough to see one 64-sample group go missing
    keep = np.ones(n, bool); keep[64:128] = False
    _, mp, mv = A.grads(_as64(kind, flat), *[a[keep] for a in args64], raw[keep], adv[keep], tgt[keep], wt[keep], mult)
    assert _block_err(kind, A.flatten(mp), rp)[0] > GRAD_REL_BOUND["policy"] and _block_err(kind, A.flatten(mv), rv)[0] > GRAD_REL_BOUND["value"]
    # clip (0.5 on each gradient) + both RMSProp steps on the device's own gradient
    stats = net.train(s, w, raw, adv, tgt, wt, grad_mult=mult, lr=1e-3, apply_update=True)
    st = net.get_optimizer_state()
    assert st["global_step"] == 200002
    lr = A.lr_at(1e-3, 200000)
    assert abs(stats["lr"] - lr) <= 1e-7 * lr
    w_ref, msp, msv, step, _, _, _ = A.apply_update(flat.astype(np.float64), gp.astype(np.float64), gv.astype(np.float64), np.ones(P), np.ones(P),
                                                     200000, 1e-3, sizes, clip=0.5)
    np.testing.assert_allclose(net.get_params(), w_ref, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(st["ms_policy"], msp, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(st["ms_value"], msv, rtol=1e-6, atol=1e-12)
    net.close()


REC = ("states", "windows", "raw", "mu", "sigma", "actions", "values", "rewards", "dones", "weights", "adv", "targets", "boot", "term_values")
TERM_IN = ("term_states", "term_windows")       # the terminal value pass's inputs: with always_bootstrap only, defined where dones != 0


def _read(net):
    return {k: net.read_rollout(k) for k in REC + (TERM_IN if net.cfg.always_bootstrap else ())}


def test_single_env_rollout_is_the_reference_worker_update():
    # from a fresh reset, with the 1 024-step cap, no episode can end inside 64 steps
    R, T, scale = 5, 64, 100.0
    sizes = A.SOLOW
    P = A.num_params(**sizes)
    e1 = _engine("solow", 1, seed=3)
    assert e1.cfg.max_episode_steps == 1024
    net = _net(e1, rnn_length=R, scale=scale)
    assert net.cfg.always_bootstrap == 1
    flat = _params("solow", 9)
    net.set_params(flat)
    net.rollout(T)
    rec = _read(net)
    stats = net.train_rollout(lr=1e-3)
    after = net.get_params()
    st = net.get_optimizer_state()
    net.close(); e1.close()
    assert not rec["dones"].any() and not rec["term_values"].any()
    keep = rec["weights"][:, 0] > 0
    assert keep.sum() == T - (R - 1) and not keep[:R - 1].any()
    boot = float(rec["boot"][0])
    (w_ref, msp, msv, step, lr, normp, normv), gp, gv, losses = A.worker_update(
        flat.astype(np.float64), sizes, np.ones(P), np.ones(P), 0, rec["states"][keep, 0].astype(np.float64),
        rec["windows"][keep, 0].astype(np.float64), rec["raw"][keep, 0], rec["rewards"][keep, 0].astype(np.float64), boot, 1e-3, scale=scale)
    assert st["global_step"] == 2
    np.testing.assert_allclose([stats["policy_norm"], stats["value_norm"]], [normp, normv], rtol=2e-3)
    np.testing.assert_allclose(after, w_ref, rtol=1e-5, atol=2e-8)
    np.testing.assert_allclose(st["ms_policy"], msp, rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(st["ms_value"], msv, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("kind", KINDS)
def test_single_env_rollout_with_episode_ends_bootstraps_as_the_worker(kind):
    """max_episode_steps below T: the rollout holds three worker rollouts (the worker's ends where its episode ends).  Solow
    (always_bootstrap on) bootstraps each finished one from the value net's prediction for the terminal observation, TradeAR1
    (off) from done_penalty = 0; one update sums their gradients."""
    R, T, cap = 5, 64, 24
    sizes = SIZES[kind]
    scale = 100.0 if kind == "solow" else 1.0
    P = A.num_params(**sizes)
    e1 = _engine(kind, 1, seed=3, max_episode_steps=cap)
    net = _net(e1, rnn_length=R, scale=scale)
    ab = kind == "solow"
    assert net.cfg.always_bootstrap == int(ab)
    flat = _params(kind, 9)
    net.set_params(flat)
    net.rollout(T)
    rec = _read(net)
    d = rec["dones"][:, 0] > 0
    assert np.flatnonzero(d).tolist() == [cap - 1, 2 * cap - 1]
    if ab:
        # the terminal value is predict on the recorded terminal observation and the window that ends in it
        got = net.predict(rec["term_states"][d, 0], rec["term_windows"][d, 0])["values"]
        assert np.array_equal(got, rec["term_values"][d, 0]) and np.all(got != 0)
        win, wts, twin = A.replay_windows(rec["states"], rec["dones"], R, rec["term_states"])
        np.testing.assert_array_equal(rec["term_windows"][d], twin[d])
        assert np.all(rec["term_states"][d, 0, 0] > 0)                      # k / 100 of a live economy, not a cleared row
    else:
        win, wts = A.replay_windows(rec["states"], rec["dones"], R)
        assert not rec["term_values"].any()
        from goldsrl import _ffi
        with pytest.raises(_ffi.GrlError):
            net.read_rollout("term_states")
    assert not rec["term_values"][~d].any()
    np.testing.assert_array_equal(rec["windows"], win)
    np.testing.assert_array_equal(rec["weights"], wts)
    stats = net.train_rollout(lr=1e-3)
    after = net.get_params()
    st = net.get_optimizer_state()
    net.close(); e1.close()
    # the three worker rollouts, each bootstrapped as GaussianWorker.update does, at the same parameters
    p = _as64(kind, flat)
    gp, gv = np.zeros(P), np.zeros(P)
    for lo, hi in ((0, cap), (cap, 2 * cap), (2 * cap, T)):
        keep = np.zeros(T, bool); keep[lo + R - 1:hi] = True
        assert np.array_equal(rec["weights"][lo:hi, 0] > 0, keep[lo:hi])
        boot = float(rec["term_values"][hi - 1, 0]) if hi < T else float(rec["boot"][0])
        s64, w64 = rec["states"][keep, 0].astype(np.float64), rec["windows"][keep, 0].astype(np.float64)
        V = A.forward(p, s64, w64, scale)[2]
        feed = A.update_feed(s64, w64, rec["raw"][keep, 0], rec["rewards"][keep, 0], V, boot, 0.99, 0.96, scale)
        _, a, b = A.grads(p, feed["states"], feed["history"], feed["actions"], feed["advantages"], feed["targets"], None, 1.0, scale)
        gp += A.flatten(a); gv += A.flatten(b)
    w_ref, msp, msv, step, lr, normp, normv = A.apply_update(flat.astype(np.float64), gp, gv, np.ones(P), np.ones(P), 0, 1e-3, sizes)
    assert st["global_step"] == 2
    np.testing.assert_allclose([stats["policy_norm"], stats["value_norm"]], [normp, normv], rtol=2e-3)
    np.testing.assert_allclose(after, w_ref, rtol=1e-5, atol=2e-8)
    np.testing.assert_allclose(st["ms_policy"], msp, rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(st["ms_value"], msv, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("kind", KINDS)
def test_rollout_replay(kind):
    from goldsrl import _ffi
    E, T, R, cap = 4100, 20, 5, 7
    sizes = SIZES[kind]
    D, Aa = sizes["static_size"], sizes["num_actions"]
    scale = 100.0 if kind == "solow" else 1.0
    ab = kind == "solow"
    rng = np.random.RandomState(3)
    if kind == "solow":
        eng = _engine(kind, E, seed=21, max_episode_steps=cap)
        k0, z0, e0 = eng.get_state("SOLOW_K"), eng.get_state("SOLOW_Z"), eng.get_state("SOLOW_E")
        tape = eng.get_state("SOLOW_TAPE")
    else:
        eng = _engine(kind, E, seed=21, max_episode_steps=cap, flags=_ffi.F_INJECT_NOISE)
        nrm = rng.normal(size=(E, 2)).astype(np.float32)
        eng.set_state("TRADE_NORMALS", nrm)                    # every step of an env draws these two normals
    eng.episodes_enable()
    net = _net(eng, rnn_length=R, scale=scale)
    flat = _params(kind, 4)
    net.set_params(flat)
    net.set_action_counter(1000)
    net.rollout(T)
    r = _read(net)
    eps = eng.episodes_read()
    assert net.get_action_counter() == 1000 + T
    assert r["dones"][cap - 1].all() and r["dones"].sum() >= 2 * E
    # draws: rebuilt from the recorded mu / sigma, bit-equal; the env actions from them (tests/_a3c_replay_checks.py)
    acts = r["actions"]                   # what the envs were stepped with, as the device computed it
    assert r["raw"].shape == (T, E, Aa)
    RC.gauss_acting(r, eng.cfg.seed, np.arange(E), 1000, tanh_action=(kind == "trade"), stride=37)
    # windows and weights follow from the recorded states and dones (fresh episodes at the first step: the engine was just reset)
    if ab:
        win, wts, twin = A.replay_windows(r["states"], r["dones"], R, r["term_states"])
        dd = r["dones"] > 0
        np.testing.assert_array_equal(r["term_windows"][dd], twin[dd])
    else:
        win, wts = A.replay_windows(r["states"], r["dones"], R)
        assert not r["term_values"].any()
    np.testing.assert_array_equal(r["windows"], win)
    np.testing.assert_array_equal(r["weights"], wts)
    # the env, fed the recorded actions (oracle/oracle.py), reproduces rewards, dones and the next observation up to each env's
    # first done; tolerances of test_gpu_envs.py
    alive = np.ones(E, bool)
    if kind == "solow":
        rho_z, rho_e = O.solow_rhos(1, 1)
        ok, oz, oe = k0.astype(np.float64), z0.astype(np.float64), e0.astype(np.float64)
        TT = tape.shape[1]
        for t in range(cap):
            ok, oz, oe, oobs, orew = O.solow_step(ok, oz, oe, tape[:, TT - 1 - t].astype(np.float64), acts[t, :, 0].astype(np.float64), rho_z, rho_e)
            np.testing.assert_allclose(r["rewards"][t], orew, rtol=1e-5, atol=5e-6)
            done = np.full(E, t + 1 >= cap)
            np.testing.assert_array_equal(r["dones"][t], done.astype(np.float32))
            nxt = r["term_states"][t] if done.all() else r["states"][t + 1]
            np.testing.assert_allclose(nxt, O.solow_process_state(oobs), rtol=1e-5, atol=1e-6)
    else:
        cash, assets = np.full(E, 10.0), np.full(E, 10.0); q, pr = np.zeros((E, 2)), np.ones((E, 2))
        for t in range(T):
            cash, assets, q, pr, obs, rew, done = O.trade_step(cash, assets, q, pr, acts[t].astype(np.float64), nrm.astype(np.float64), O.trade_std_e())
            done = done | (t + 1 >= cap)
            np.testing.assert_allclose(r["rewards"][t][alive], rew[alive], rtol=1e-5, atol=1e-9)
            np.testing.assert_array_equal(r["dones"][t][alive], done.astype(np.float32)[alive])
            live = alive & ~done
            if t + 1 < T:
                np.testing.assert_allclose(r["states"][t + 1][live], O.trade_process_state(obs)[live], rtol=1e-5, atol=1e-6)
            alive = live
    # mu, sigma, values equal predict on the recorded inputs; the terminal values likewise
    flat_s = r["states"].reshape(-1, D); flat_w = r["windows"].reshape(-1, R, D)
    for lo in range(0, T * E, 8192):
        got = net.predict(flat_s[lo:lo + 8192], flat_w[lo:lo + 8192])
        for k in ("mu", "sigma", "values"):
            np.testing.assert_array_equal(got[k], r[k].reshape((-1,) + r[k].shape[2:])[lo:lo + 8192], err_msg=k)
    if ab:
        d = r["dones"].reshape(-1) > 0
        ts, tw, tv = r["term_states"].reshape(-1, D)[d], r["term_windows"].reshape(-1, R, D)[d], r["term_values"].reshape(-1)[d]
        for lo in range(0, len(ts), 8192):
            np.testing.assert_array_equal(net.predict(ts[lo:lo + 8192], tw[lo:lo + 8192])["values"], tv[lo:lo + 8192])
        assert not r["term_values"].reshape(-1)[~d].any()
    # adv / targets: the worker's GAE cut at episode ends (oracle.gae where no episode ends inside the rollout)
    adv, tgt = A.gae_segments(r["rewards"], r["values"], r["boot"], r["dones"], r["term_values"], ab, 0.99, 0.96, scale)
    np.testing.assert_allclose(r["adv"], adv, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["targets"], tgt, rtol=1e-5, atol=1e-6 * scale)
    last = r["dones"][-1] > 0
    assert np.array_equal(r["boot"][last], r["term_values"][-1][last])          # 0 with always_bootstrap off
    assert len(eps) == int(r["dones"].sum())
    net.close(); eng.close()


def test_gae_without_dones_is_oracle_gae():
    E, T, R = 512, 12, 3
    eng = _engine("solow", E, seed=2)
    net = _net(eng, rnn_length=R, scale=100.0)
    net.set_params(_params("solow", 4))
    net.rollout(T)
    r = {k: net.read_rollout(k) for k in ("rewards", "values", "boot", "dones", "adv", "targets")}
    net.close(); eng.close()
    assert not r["dones"].any()
    a2, t2 = O.gae(r["rewards"].astype(np.float64), r["values"].astype(np.float64), r["boot"].astype(np.float64), 0.99, 0.96)
    np.testing.assert_allclose(r["adv"], a2 / 100.0, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["targets"], t2, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("kind", KINDS)
def test_train_rollout_equals_host_train_reproducible_and_checkpoint(tmp_path, kind):
    E, T, R = 300, 6, 3
    sizes = SIZES[kind]
    D, Aa, P = sizes["static_size"], sizes["num_actions"], A.num_params(**sizes)
    kw = dict(max_episode_steps=4)                      # episodes end inside the rollout
    eng = _engine(kind, E, seed=5, **kw)
    net = _net(eng, rnn_length=R)
    flat = _params(kind, 6)
    net.set_params(flat)
    net.rollout(T)
    r = {k: net.read_rollout(k) for k in ("states", "windows", "raw", "adv", "targets", "weights")}
    s1 = net.train_rollout(lr=1e-3)
    g_ro = net.get_grads("policy"), net.get_grads("value")
    p_ro = net.get_params()
    net.set_params(flat)
    net.set_optimizer_state(np.ones(P, np.float32), np.ones(P, np.float32), 0)
    s2 = net.train(r["states"].reshape(-1, D), r["windows"].reshape(-1, R, D), r["raw"].reshape(-1, Aa), r["adv"].reshape(-1),
                   r["targets"].reshape(-1), r["weights"].reshape(-1), grad_mult=1.0 / E, lr=1e-3)
    assert np.array_equal(net.get_grads("policy"), g_ro[0]) and np.array_equal(net.get_grads("value"), g_ro[1])
    assert np.array_equal(net.get_params(), p_ro)
    assert s1["policy_norm"] == s2["policy_norm"] and s1["value_norm"] == s2["value_norm"]
    net.close(); eng.close()

    def run(n_upd):
        e = _engine(kind, E, seed=5, **kw)
        nt = _net(e, rnn_length=R)
        nt.set_params(flat)
        for _ in range(n_upd):
            nt.rollout(T)
            nt.train_rollout(lr=1e-3)
        res = (nt.get_params(), nt.get_optimizer_state(), nt.get_action_counter(), nt.get_grads("policy"), nt.get_grads("value"))
        nt.close(); e.close()
        return res
    a, b = run(3), run(3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1]["ms_policy"], b[1]["ms_policy"]) and a[1]["global_step"] == 6
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    # checkpoint after update 1, restored into a fresh net on an engine that carries on from the same env state: same bits
    ck = str(tmp_path / "gauss.npz")
    e = _engine(kind, E, seed=5, **kw)
    nt = _net(e, rnn_length=R)
    nt.set_params(flat)
    nt.rollout(T); nt.train_rollout(lr=1e-3)
    nt.save_checkpoint(ck)
    nt.close()
    nt2 = _net(e, rnn_length=R)
    nt2.load_checkpoint(ck)
    ck_state = np.load(ck)
    assert int(ck_state["global_step"]) == 2 and int(ck_state["action_counter"]) == T
    for _ in range(2):
        nt2.rollout(T); nt2.train_rollout(lr=1e-3)
    got = nt2.get_params(), nt2.get_optimizer_state()
    nt2.close(); e.close()
    assert got[1]["global_step"] == 6
    # the reloaded net restarts its windows from the engine's current observations; the uninterrupted run kept them, so the
    # comparison is against an uninterrupted run whose net is also re-created (windows restarted) after update 1
    e = _engine(kind, E, seed=5, **kw)
    nt = _net(e, rnn_length=R)
    nt.set_params(flat)
    nt.rollout(T); nt.train_rollout(lr=1e-3)
    keep = (nt.get_params(), nt.get_optimizer_state(), nt.get_action_counter())
    nt.close()
    nt3 = _net(e, rnn_length=R)
    nt3.set_params(keep[0]); nt3.set_optimizer_state(keep[1]["ms_policy"], keep[1]["ms_value"], keep[1]["global_step"])
    nt3.set_action_counter(keep[2])
    for _ in range(2):
        nt3.rollout(T); nt3.train_rollout(lr=1e-3)
    want = nt3.get_params(), nt3.get_optimizer_state()
    nt3.close(); e.close()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1]["ms_value"], want[1]["ms_value"])


@pytest.mark.parametrize("kind", KINDS)
def test_direction_of_one_update(engs, kind):
    n, R = 512, 5
    net = _net(engs[kind], rnn_length=R)
    flat = _params(kind, 8)
    net.set_params(flat)
    s, w = _samples(kind, n, R, seed=3)[:2]
    before = net.predict(s, w)
    raw = before["mu"] + 0.5 * before["sigma"]                     # drawn above the mean, and it paid off: mu moves towards it
    adv = np.ones(n, np.float32)
    stats = net.train(s, w, raw, adv, before["values"], None, grad_mult=1.0 / n, lr=1e-3)
    assert stats["value_norm"] == 0.0
    after = net.predict(s, w)
    assert after["mu"].mean() > before["mu"].mean() + 1e-4
    net.close()


@pytest.mark.parametrize("kind", KINDS)
def test_bench_size_update_against_oracle(kind):
    E, T, R = 8192, 20, 5
    sizes = SIZES[kind]
    D, Aa, P = sizes["static_size"], sizes["num_actions"], A.num_params(**sizes)
    scale = 100.0 if kind == "solow" else 1.0
    eng = _engine(kind, E, seed=13)
    net = _net(eng, rnn_length=R, scale=scale)
    flat = _params(kind, 10)
    net.set_params(flat)
    net.rollout(T)
    r = {k: net.read_rollout(k) for k in ("states", "windows", "raw", "adv", "targets", "weights")}
    net.train_rollout(lr=1e-4)
    gp, gv = net.get_grads("policy"), net.get_grads("value")
    net.close(); eng.close()
    p = _as64(kind, flat)
    sp = np.zeros(P); sv = np.zeros(P)
    S = r["states"].reshape(-1, D).astype(np.float64); W = r["windows"].reshape(-1, R, D).astype(np.float64)
    RW, AD, TG, WT = r["raw"].reshape(-1, Aa), r["adv"].reshape(-1), r["targets"].reshape(-1), r["weights"].reshape(-1)
    for lo in range(0, T * E, 16384):       # chunks, as _flat_oracle.py
        sl = slice(lo, lo + 16384)
        _, a, b = A.grads(p, S[sl], W[sl], RW[sl], AD[sl], TG[sl], WT[sl], 1.0 / E, scale)
        sp += A.flatten(a); sv += A.flatten(b)
    ep, bp = _block_err(kind, gp, sp)
    ev, bv = _block_err(kind, gv, sv)
    print("%s bench size: worst block error policy %.3g (%s), value %.3g (%s)" % (kind, ep, bp, ev, bv))
    assert ep < BENCH_REL_BOUND[kind]["policy"] and ev < BENCH_REL_BOUND[kind]["value"], (ep, bp, ev, bv)


def _run_script(module, out, extra):
    cmd = [sys.executable, "-m", "goldsrl.scripts." + module, "--envs", "256", "--t_max", "20", "--updates", "3", "--model_dir", str(out)] + extra
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "golds-rl-gym_amd"), os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    files = os.listdir(out)
    assert any(f.startswith("events.out.tfevents") for f in files), files
    assert "checkpoint.npz" in files
    return np.load(out / "checkpoint.npz"), files


def test_train_solow_script(tmp_path):
    out = tmp_path / "run"
    z, files = _run_script("train_solow", out, ["--eval-every", "2"])
    assert int(z["global_step"]) == 6 and z["params"].size == A.num_params(**A.SOLOW) and int(z["action_counter"]) == 60
    assert "Solow-1-1.json" in files
    log = json.load(open(out / "Solow-1-1.json"))
    assert set(log) == {"total_reward", "episode_length"}
    assert log["episode_length"] == [1024, 1024] and len(log["total_reward"]) == 2          # after updates 2 and 3
    assert all(np.isfinite(v) for v in log["total_reward"])


def test_train_trade_script(tmp_path):
    out = tmp_path / "run"
    z, files = _run_script("train_trade", out, [])
    assert int(z["global_step"]) == 6 and z["params"].size == A.num_params(**A.TRADE) and int(z["action_counter"]) == 60


def test_estimator_facades(engs):
    from goldsrl import _ffi, _ffi_gauss
    from goldsrl.agents.a3c import estimators as est
    for kind in KINDS:
        sizes = SIZES[kind]
        D, Aa = sizes["static_size"], sizes["num_actions"]
        net = _net(engs[kind], rnn_length=5, scale=2.0)
        flat = _params(kind, 12)
        net.set_params(flat)
        pol = est.GaussianPolicyEstimator(Aa, static_size=D, temporal_size=D, net=net)
        val = est.ValueEstimator(static_size=D, temporal_size=D, net=net, scale=2.0)
        with pytest.raises(ValueError):
            est.GaussianPolicyEstimator(Aa + 1, static_size=D, temporal_size=D, net=net)
        with pytest.raises(ValueError):
            est.ValueEstimator(static_size=7, temporal_size=4, net=net, scale=2.0)          # the gated trader's sizes
        with pytest.raises(ValueError):
            est.ValueEstimator(static_size=D, temporal_size=D, net=net, scale=1.0)
        with pytest.raises(ValueError):
            est.GaussianPolicyEstimator(Aa, static_size=D, temporal_size=D, net=None)
        s, w = _samples(kind, 5, 5, seed=2)[:2]
        hist = w[:, :3]                                     # three rows: padded post to R = 5 inside predict
        p1 = pol.predict(s, hist, batch=True)
        assert set(p1) == {"mu", "sigma"} and all(v.shape == (5, Aa) for v in p1.values())
        v1 = val.predict(s, hist, batch=True)
        assert set(v1) == {"logits"} and v1["logits"].shape == (5,)
        ref = A.forward(_as64(kind, flat), s.astype(np.float64), np.concatenate([hist, np.zeros((5, 2, D), np.float32)], 1).astype(np.float64), 2.0)
        np.testing.assert_allclose(p1["mu"], ref[0], rtol=FWD_RTOL, atol=FWD_ATOL)
        np.testing.assert_allclose(p1["sigma"], ref[1], rtol=FWD_RTOL, atol=FWD_ATOL)
        np.testing.assert_allclose(v1["logits"], ref[2], rtol=FWD_RTOL, atol=FWD_ATOL)
        one = pol.predict(s[0], hist[0])                    # a single state, as the worker calls it
        assert one["mu"].shape == (1, Aa)
        net.close()
    # the net exists for these two size sets only, and each env takes one always_bootstrap
    with pytest.raises(_ffi.GrlError):
        _ffi_gauss.GaussNet(engs["solow"], always_bootstrap=0)
    with pytest.raises(_ffi.GrlError):
        _ffi_gauss.GaussNet(engs["trade"], always_bootstrap=1)
    e3 = _ffi.Engine(_ffi.ENV_TRADE, 4, n_assets=3)
    with pytest.raises(_ffi.GrlError):
        _ffi_gauss.GaussNet(e3)
    e3.close()
