"""GPU: the Ticker gated trader (csrc/net_gated.hip through include/goldsrl_gatednet.h) against the float64 restatement
tests/_gated_oracle.py -- predict, the host-sample update, the device-resident rollout + update, its replay against oracle/ticker.py
and the Philox draws, consistency (host vs rollout path, bitwise reproducibility, checkpoints), the direction of one update, the
bench-size update and the training script."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _a3c_replay_checks as RC
import _gated_oracle as G
from oracle import ticker as TK

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "ticker.npz")

# Per-block bound of |device - oracle| on the gradients, relative to the block's largest oracle entry plus the largest entry of the
# whole gradient (blocks that are nearly zero carry only rounding).  Measured on the MI355X:
#   host samples (n = 1 000, R = 5, _samples(1000, 5, 11)): worst block 9.6e-8 (policy, normal3_w) / 3.8e-8 (value, value2_b)
#   bench size (8 192 envs x 20 steps, one rollout):     worst block 7.0e-5 (policy, class2_b) / 2.1e-7 (value, value2_b) -- sums
#   of 163 840 terms that largely cancel, accumulated in fp32 over 256 slabs, plus ReLU inputs within rounding of 0
GRAD_REL_BOUND = 1e-6
BENCH_REL_BOUND = 2e-4


def _matrix():
    return np.load(GOLD)["matrix"]


def _engine(E, seed=7, **kw):
    from goldsrl import _ffi
    eng = _ffi.Engine(_ffi.ENV_TICKER, E, seed=seed, **kw)
    eng.ticker_set_table(_matrix())
    eng.reset()
    return eng


def _net(eng, **kw):
    from goldsrl import _ffi_gated
    kw.setdefault("max_samples", 8192)
    net = _ffi_gated.GatedNet(eng, **kw)
    return net


def _params(seed=5):
    p = G.init(seed)
    rng = np.random.RandomState(seed)
    for k in p:
        if k.endswith("_b"):
            p[k] = p[k] + 0.05 * rng.normal(size=p[k].shape)
    return G.flatten(p).astype(np.float32)


def _samples(n, R, seed=0):
    rng = np.random.RandomState(seed)
    states = rng.normal(size=(n, 7)).astype(np.float32)
    win = rng.normal(size=(n, R, 4)).astype(np.float32)
    lens = rng.randint(1, R + 1, size=n)
    for i in range(n):
        win[i, lens[i]:] = 0.0
    choices = rng.randint(0, 3, size=(n, 2)).astype(np.int32)
    raw = rng.normal(size=(n, 2)).astype(np.float32)
    adv = rng.normal(size=n).astype(np.float32)
    tgt = rng.normal(size=n).astype(np.float32)
    w = (rng.uniform(size=n) > 0.25).astype(np.float32)
    return states, win, choices, raw, adv, tgt, w


def _as64(flat):
    return G.unflatten(np.asarray(flat, np.float32).astype(np.float64))


@pytest.fixture(scope="module")
def eng():
    e = _engine(64)
    yield e
    e.close()


@pytest.mark.parametrize("R", [5, 20])
def test_predict_matches_oracle(eng, R):
    net = _net(eng, rnn_length=R)
    flat = _params()
    net.set_params(flat)
    p = _as64(flat)
    for n in (1, 63, 64, 65, 1000):
        s, w = _samples(n, R, seed=n)[:2]
        got = net.predict(s, w)
        ref = G.forward(p, s.astype(np.float64), w.astype(np.float64))
        for k, r in zip(("probs", "mu", "sigma", "values"), ref):
            np.testing.assert_allclose(got[k], r, rtol=2e-4, atol=2e-5, err_msg="%s n=%d R=%d" % (k, n, R))
    net.close()


def _block_err(got, ref):
    """max over blocks of |got - ref|_inf / bound_scale, and the worst block's name"""
    rng_ = G.block_ranges()
    gmax = np.abs(ref).max()
    worst, name = 0.0, None
    for b, (lo, hi) in rng_.items():
        scale = np.abs(ref[lo:hi]).max() + gmax
        e = np.abs(got[lo:hi] - ref[lo:hi]).max() / scale
        if e > worst:
            worst, name = e, b
    return worst, name


def test_host_train_gradients_clip_and_rmsprop(eng):
    n, R = 1000, 5
    net = _net(eng, rnn_length=R, clip_norm=0.5)
    flat = _params()
    net.set_params(flat)
    net.set_optimizer_state(np.ones(G.NUM_PARAMS, np.float32), np.ones(G.NUM_PARAMS, np.float32), 200000)
    s, w, ch, raw, adv, tgt, wt = _samples(n, R, seed=11)
    mult = 0.3
    stats = net.train(s, w, ch, raw, adv, tgt, wt, grad_mult=mult, lr=1e-3, apply_update=False)
    gp, gv = net.get_grads("policy"), net.get_grads("value")
    args64 = [a.astype(np.float64) for a in (s, w)]
    (pl, vl, ent), rp, rv = G.grads(_as64(flat), *args64, ch, raw, adv, tgt, wt, mult)
    rp, rv = G.flatten(rp), G.flatten(rv)
    ep, bp = _block_err(gp, rp)
    ev, bv = _block_err(gv, rv)
    print("worst block error: policy %.3g (%s), value %.3g (%s)" % (ep, bp, ev, bv))
    assert ep < GRAD_REL_BOUND and ev < GRAD_REL_BOUND, (ep, bp, ev, bv)
    assert not gp[~G.policy_mask()].any() and not gv[~G.value_mask()].any()
    np.testing.assert_allclose([stats["policy_loss"], stats["value_loss"], stats["entropy_mean"]], [pl, vl, ent], rtol=1e-4)
    np.testing.assert_allclose([stats["policy_norm"], stats["value_norm"]], [np.linalg.norm(rp), np.linalg.norm(rv)], rtol=1e-4)
    # the bound is tight enough to see one 64-sample group go missing
    keep = np.ones(n, bool); keep[64:128] = False
    (_, _, _), mp, mv = G.grads(_as64(flat), *[a[keep] for a in args64], ch[keep], raw[keep], adv[keep], tgt[keep], wt[keep], mult)
    assert _block_err(G.flatten(mp), rp)[0] > GRAD_REL_BOUND and _block_err(G.flatten(mv), rv)[0] > GRAD_REL_BOUND
    # clip (0.5 on each gradient) + both RMSProp steps on the device's own gradient
    stats = net.train(s, w, ch, raw, adv, tgt, wt, grad_mult=mult, lr=1e-3, apply_update=True)
    st = net.get_optimizer_state()
    assert st["global_step"] == 200002
    lr = G.lr_at(1e-3, 200000)
    assert abs(stats["lr"] - lr) <= 1e-7 * lr
    w_ref, msp, msv, step, _, _, _ = G.apply_update(flat.astype(np.float64), gp.astype(np.float64), gv.astype(np.float64),
                                                     np.ones(G.NUM_PARAMS), np.ones(G.NUM_PARAMS), 200000, 1e-3, clip=0.5)
    np.testing.assert_allclose(net.get_params(), w_ref, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(st["ms_policy"], msp, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(st["ms_value"], msv, rtol=1e-6, atol=1e-12)
    net.close()


def test_single_env_rollout_is_the_reference_worker_update():
    R, T = 5, 64
    e1 = _engine(1, seed=3)
    net = _net(e1, rnn_length=R)
    flat = _params(9)
    net.set_params(flat)
    net.rollout(T)
    rec = {k: net.read_rollout(k) for k in ("states", "windows", "choices", "raw", "rewards", "dones", "weights", "boot", "values")}
    stats = net.train_rollout(lr=1e-3)
    after = net.get_params()
    st = net.get_optimizer_state()
    net.close(); e1.close()
    d = rec["dones"][:, 0]
    assert not d[:R - 1].any()
    keep = rec["weights"][:, 0] > 0
    assert keep.sum() == T - (R - 1) and not keep[:R - 1].any()
    if d.any():
        pytest.skip("an episode ended inside the rollout: the single-worker restatement needs one episode")
    boot = float(rec["boot"][0])
    (w_ref, msp, msv, step, lr, normp, normv), gp, gv, losses = G.worker_update(
        flat.astype(np.float64), np.ones(G.NUM_PARAMS), np.ones(G.NUM_PARAMS), 0,
        rec["states"][keep, 0].astype(np.float64), rec["windows"][keep, 0].astype(np.float64), rec["choices"][keep, 0], rec["raw"][keep, 0],
        rec["rewards"][keep, 0].astype(np.float64), boot, 1e-3)
    assert st["global_step"] == 2
    np.testing.assert_allclose([stats["policy_norm"], stats["value_norm"]], [normp, normv], rtol=2e-3)
    np.testing.assert_allclose(after, w_ref, rtol=1e-5, atol=2e-8)
    np.testing.assert_allclose(st["ms_policy"], msp, rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(st["ms_value"], msv, rtol=1e-5, atol=1e-9)


def test_rollout_replay():
    E, T, R = 4100, 20, 5
    eng = _engine(E, seed=21, max_episode_steps=7)
    eng.episodes_enable()
    net = _net(eng, rnn_length=R)
    flat = _params(4)
    net.set_params(flat)
    net.set_action_counter(1000)
    start = {"start": eng.get_state("TICKER_START")}
    assert not eng.get_state("TICKER_IDX").any()
    net.rollout(T)
    r = {k: net.read_rollout(k) for k in ("states", "windows", "choices", "raw", "probs", "mu", "sigma", "values", "rewards", "dones",
                                           "weights", "adv", "targets", "boot")}
    eps = eng.episodes_read()
    assert net.get_action_counter() == 1000 + T
    # draws: rebuilt from the recorded probs / mu / sigma (tests/_a3c_replay_checks.py)
    assert r["choices"].shape == (T, E, 2)
    RC.gated_acting(r, eng.cfg.seed, np.arange(E), 1000, stride=37)
    # windows and weights follow from the recorded states and dones (fresh episodes at the first step: the engine was just reset)
    win, wts = G.replay_windows(r["states"], r["dones"], R)
    np.testing.assert_array_equal(r["windows"], win)
    np.testing.assert_array_equal(r["weights"], wts)
    # the env, fed the recorded actions (oracle/ticker.py), reproduces rewards and dones up to each env's first done
    m = _matrix()
    frac = (1.0 / (1.0 + np.exp(-r["raw"].astype(np.float64)))).astype(np.float32)
    st, _ = TK.ticker_reset(m, start["start"])
    alive = np.ones(E, bool)
    for t in range(T):
        _, rew, done = TK.ticker_step(m, st, r["choices"][t], frac[t].astype(np.float64))
        done = done | (t + 1 >= 7)
        np.testing.assert_array_equal(rew.astype(np.float32)[alive], r["rewards"][t][alive])
        np.testing.assert_array_equal(done.astype(np.float32)[alive], r["dones"][t][alive])
        alive &= ~done
    # values, probs, mu, sigma equal predict on the recorded inputs
    flat_s = r["states"].reshape(-1, 7); flat_w = r["windows"].reshape(-1, R, 4)
    for lo in range(0, T * E, 8192):
        got = net.predict(flat_s[lo:lo + 8192], flat_w[lo:lo + 8192])
        for k, rk in (("probs", "probs"), ("mu", "mu"), ("sigma", "sigma"), ("values", "values")):
            np.testing.assert_array_equal(got[k], r[rk].reshape((-1,) + r[rk].shape[2:])[lo:lo + 8192], err_msg=k)
    # adv / targets: the worker's GAE with a done mask (oracle.gae where no episode ends inside the rollout)
    adv, tgt = G.gae_masked(r["rewards"], r["values"], r["boot"], r["dones"], 0.99, 0.96, 1.0)
    np.testing.assert_allclose(r["adv"], adv, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r["targets"], tgt, rtol=1e-5, atol=1e-6)
    clean = ~r["dones"].any(0)
    a2, t2 = G.O.gae(r["rewards"][:, clean].astype(np.float64), r["values"][:, clean].astype(np.float64), r["boot"][clean].astype(np.float64), 0.99, 0.96)
    np.testing.assert_allclose(r["adv"][:, clean], a2, rtol=1e-5, atol=1e-6)
    assert (r["boot"][r["dones"][-1] > 0] == 0).all()
    assert len(eps) == int(r["dones"].sum())
    net.close(); eng.close()


def test_train_rollout_equals_host_train_reproducible_and_checkpoint(tmp_path):
    E, T, R = 300, 6, 3
    eng = _engine(E, seed=5)
    net = _net(eng, rnn_length=R)
    flat = _params(6)
    net.set_params(flat)
    net.rollout(T)
    r = {k: net.read_rollout(k) for k in ("states", "windows", "choices", "raw", "adv", "targets", "weights")}
    s1 = net.train_rollout(lr=1e-3)
    g_ro = net.get_grads("policy"), net.get_grads("value")
    p_ro = net.get_params()
    net.set_params(flat)
    net.set_optimizer_state(np.ones(G.NUM_PARAMS, np.float32), np.ones(G.NUM_PARAMS, np.float32), 0)
    s2 = net.train(r["states"].reshape(-1, 7), r["windows"].reshape(-1, R, 4), r["choices"].reshape(-1, 2), r["raw"].reshape(-1, 2),
                   r["adv"].reshape(-1), r["targets"].reshape(-1), r["weights"].reshape(-1), grad_mult=1.0 / E, lr=1e-3)
    assert np.array_equal(net.get_grads("policy"), g_ro[0]) and np.array_equal(net.get_grads("value"), g_ro[1])
    assert np.array_equal(net.get_params(), p_ro)
    assert s1["policy_norm"] == s2["policy_norm"] and s1["value_norm"] == s2["value_norm"]
    net.close(); eng.close()

    def run(n_upd):
        e = _engine(E, seed=5)
        nt = _net(e, rnn_length=R)
        nt.set_params(flat)
        for _ in range(n_upd):
            nt.rollout(T)
            nt.train_rollout(lr=1e-3)
        res = (nt.get_params(), nt.get_optimizer_state(), nt.get_action_counter())
        nt.close(); e.close()
        return res
    a, b = run(3), run(3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1]["ms_policy"], b[1]["ms_policy"]) and a[1]["global_step"] == 6
    # checkpoint after update 1, restored into a fresh net on an engine that carries on from the same env state: same bits
    ck = str(tmp_path / "gated.npz")
    e = _engine(E, seed=5)
    nt = _net(e, rnn_length=R)
    nt.set_params(flat)
    nt.rollout(T); nt.train_rollout(lr=1e-3)
    nt.save_checkpoint(ck)
    nt.close()
    nt2 = _net(e, rnn_length=R)
    nt2.load_checkpoint(ck)
    ck_state = np.load(ck)
    assert int(ck_state["global_step"]) == 2 and int(ck_state["action_counter"]) == T
    nt2.rollout(T)
    nt2.train_rollout(lr=1e-3)
    nt2.rollout(T)
    nt2.train_rollout(lr=1e-3)
    got = nt2.get_params(), nt2.get_optimizer_state()
    nt2.close(); e.close()
    assert got[1]["global_step"] == 6
    # the reloaded net restarts its windows from the engine's current observations; the uninterrupted run kept them, so the
    # comparison is against an uninterrupted run whose net is also re-created (windows restarted) after update 1
    e = _engine(E, seed=5)
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


def test_direction_of_one_update(eng):
    n, R = 512, 5
    net = _net(eng, rnn_length=R)
    flat = _params(8)
    net.set_params(flat)
    s, w = _samples(n, R, seed=3)[:2]
    before = net.predict(s, w)
    ch = np.zeros((n, 2), np.int32); ch[:, 0] = 1                  # buy asset 0, hold asset 1
    raw = before["mu"][:, :, 1].copy()                             # at the mean: the normal term pushes no direction on mu
    adv = np.ones(n, np.float32)
    stats = net.train(s, w, ch, raw, adv, before["values"], None, grad_mult=1.0 / n, lr=1e-3)
    assert stats["value_norm"] == 0.0
    after = net.predict(s, w)
    assert after["probs"][:, 0, 1].mean() > before["probs"][:, 0, 1].mean() + 1e-4
    net.close()


def test_bench_size_update_against_oracle():
    E, T, R = 8192, 20, 5
    eng = _engine(E, seed=13)
    net = _net(eng, rnn_length=R)
    flat = _params(10)
    net.set_params(flat)
    net.rollout(T)
    r = {k: net.read_rollout(k) for k in ("states", "windows", "choices", "raw", "adv", "targets", "weights")}
    net.train_rollout(lr=1e-4)
    gp, gv = net.get_grads("policy"), net.get_grads("value")
    net.close(); eng.close()
    p = _as64(flat)
    sp = np.zeros(G.NUM_PARAMS); sv = np.zeros(G.NUM_PARAMS)
    S = r["states"].reshape(-1, 7).astype(np.float64); W = r["windows"].reshape(-1, R, 4).astype(np.float64)
    C, RW = r["choices"].reshape(-1, 2), r["raw"].reshape(-1, 2)
    A, TG, WT = r["adv"].reshape(-1), r["targets"].reshape(-1), r["weights"].reshape(-1)
    for lo in range(0, T * E, 16384):       # chunks, as _flat_oracle.py
        sl = slice(lo, lo + 16384)
        _, a, b = G.grads(p, S[sl], W[sl], C[sl], RW[sl], A[sl], TG[sl], WT[sl], 1.0 / E)
        sp += G.flatten(a); sv += G.flatten(b)
    ep, bp = _block_err(gp, sp)
    ev, bv = _block_err(gv, sv)
    print("bench size: worst block error policy %.3g (%s), value %.3g (%s)" % (ep, bp, ev, bv))
    assert ep < BENCH_REL_BOUND and ev < BENCH_REL_BOUND, (ep, bp, ev, bv)


def test_train_ticker_script(tmp_path):
    out = tmp_path / "run"
    cmd = [sys.executable, "-m", "goldsrl.scripts.train_ticker", "--table", GOLD, "--envs", "256", "--steps", "20", "--updates", "3",
           "--out", str(out)]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "golds-rl-gym_amd"), os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    files = os.listdir(out)
    assert any(f.startswith("events.out.tfevents") for f in files), files
    assert "checkpoint.npz" in files
    z = np.load(out / "checkpoint.npz")
    assert int(z["global_step"]) == 6 and z["params"].size == G.NUM_PARAMS


def test_estimator_facades(eng):
    from goldsrl.agents.a3c import estimators as est
    net = _net(eng, rnn_length=5, scale=2.0)
    flat = _params(12)
    net.set_params(flat)
    pol = est.DiscreteAndContPolicyEstimator(2, static_size=7, temporal_size=4, net=net)
    val = est.ValueEstimator(static_size=7, temporal_size=4, net=net, scale=2.0)
    with pytest.raises(ValueError):
        est.DiscreteAndContPolicyEstimator(3, static_size=7, temporal_size=4, net=net)
    s, w = _samples(5, 5, seed=2)[:2]
    hist = w[:, :3]                                     # three rows: padded post to R = 5 inside predict
    p1 = pol.predict(s, hist, batch=True)
    assert set(p1) == {"mu", "sigma", "probs"} and all(v.shape == (5, 2, 3) for v in p1.values())
    v1 = val.predict(s, hist, batch=True)
    assert set(v1) == {"logits"} and v1["logits"].shape == (5,)
    ref = G.forward(_as64(flat), s.astype(np.float64), np.concatenate([hist, np.zeros((5, 2, 4), np.float32)], 1).astype(np.float64), 2.0)
    np.testing.assert_allclose(p1["probs"], ref[0], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(v1["logits"], ref[3], rtol=2e-4, atol=2e-5)
    one = pol.predict(s[0], hist[0])                    # a single state, as the worker calls it
    assert one["probs"].shape == (1, 2, 3)
    net.close()
