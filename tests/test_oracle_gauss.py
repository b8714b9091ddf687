"""CPU: the float64 restatement of the A3C Gaussian agent (tests/_gauss_oracle.py) against finite differences, an independent
torch autograd version, a hand-computed RMSProp example and the reference's own acting / window / update rules
(tests/golden/gauss_worker.npz); the C header of the Gaussian net against the library and its binding."""
import ctypes
import os
import re

import numpy as np
import pytest

import _gauss_oracle as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gauss_worker.npz")
SIZES = {"solow": A.SOLOW, "trade": A.TRADE}
CASES = ("on", "off", "short_on", "short_off")


def _batch(sizes, n=6, R=5, seed=0):
    rng = np.random.RandomState(seed)
    D, Aa = sizes["static_size"], sizes["num_actions"]
    states = rng.normal(size=(n, D))
    win = rng.normal(size=(n, R, D))
    for i in range(n):                      # ragged windows, zero rows after
        win[i, 1 + i % R:] = 0.0
    raw = rng.normal(size=(n, Aa))
    adv = rng.normal(size=n)
    tgt = rng.normal(size=n)
    w = (rng.uniform(size=n) > 0.3).astype(float)
    return states, win, raw, adv, tgt, w


def _params(sizes, seed=1):
    p = A.init(seed, **sizes)
    rng = np.random.RandomState(seed + 7)
    for k in p:                             # non-zero biases so that every block is exercised
        if k.endswith("_b"):
            p[k] = p[k] + 0.1 * rng.normal(size=p[k].shape)
    return p


def test_num_params_and_block_order():
    assert A.num_params(**A.SOLOW) == 148547 and A.num_params(**A.TRADE) == 149285
    want = ["gru_gates_w", "gru_gates_b", "gru_cand_w", "gru_cand_b", "temporal_w", "temporal_b", "static1_w", "static1_b", "static2_w",
            "static2_b", "mu1_w", "mu1_b", "mu2_w", "mu2_b", "mu3_w", "mu3_b", "sigma1_w", "sigma1_b", "sigma2_w", "sigma2_b", "sigma3_w",
            "sigma3_b", "value1_w", "value1_b", "value2_w", "value2_b"]
    for sizes, trunk in ((A.SOLOW, 7744), (A.TRADE, 8224)):
        assert A.names(**sizes) == want
        r = A.block_ranges(**sizes)
        tower = 96 * 256 + 256 + 256 * 128 + 128 + 128 * sizes["num_actions"] + sizes["num_actions"]
        assert r["mu1_w"][0] == trunk and r["sigma1_w"][0] == trunk + tower and r["value1_w"][0] == trunk + 2 * tower
        shapes = dict(A.param_shapes(**sizes))
        assert shapes["gru_gates_w"] == (sizes["temporal_size"] + 32, 64) and shapes["static1_w"] == (sizes["static_size"], 64)
        assert shapes["mu3_w"] == (128, sizes["num_actions"]) and shapes["value2_w"] == (256, 1)
        p = _params(sizes)
        assert A.sizes_of(p) == sizes
        assert np.array_equal(A.unflatten(A.flatten(p), **sizes)["sigma3_b"], p["sigma3_b"])
    assert (A.init(3, **A.SOLOW)["sigma3_b"] == -1).all() and (A.init(3, **A.SOLOW)["gru_gates_b"] == 1).all()


def test_forward_heads_are_bounded_as_the_reference_builds_them():
    sizes = A.TRADE
    states, win = _batch(sizes, n=40, seed=2)[:2]
    p = _params(sizes)
    p["mu3_w"] *= 50.0; p["sigma3_w"] *= 50.0          # saturate the heads
    mu, sigma, v = A.forward(p, states, win, scale=3.0)
    assert mu.shape == (40, 2) and sigma.shape == (40, 2) and v.shape == (40,)
    assert (np.abs(mu) <= 5.0).all() and np.abs(mu).max() > 4.9
    assert (sigma >= 1e-3).all() and (sigma <= 1.0 + 1e-3).all()
    np.testing.assert_allclose(A.forward(p, states, win, scale=1.0)[2] * 3.0, v, rtol=1e-14)


@pytest.mark.parametrize("env", ["solow", "trade"])
@pytest.mark.parametrize("which", ["policy", "value"])
def test_gradients_against_finite_differences(env, which):
    sizes = SIZES[env]
    states, win, raw, adv, tgt, w = _batch(sizes)
    p = _params(sizes)
    scale = 2.0
    _, gp, gv = A.grads(p, states, win, raw, adv, tgt, w, 0.5, scale)
    g = gp if which == "policy" else gv
    k = 0 if which == "policy" else 1

    def f(q):
        return A.losses(q, states, win, raw, adv, tgt, w, 0.5, scale)[k]
    num = A.NN.numeric_grad(f, p, A.names(**sizes), eps=1e-6, max_per=3, seed=3)
    for name, vals in num.items():
        for idx, v in vals:
            assert abs(g[name][idx] - v) <= 1e-6 + 1e-5 * abs(v), (name, idx, g[name][idx], v)
    blocks = A.POLICY_BLOCKS if which == "policy" else A.VALUE_BLOCKS
    for name in A.names(**sizes):
        if name not in blocks:
            assert not np.any(g[name]), name
        elif name != "gru_gates_b":
            assert np.any(g[name]), name


@pytest.mark.parametrize("env", ["solow", "trade"])
def test_losses_and_gradients_against_torch_autograd(env):
    import torch
    sizes = SIZES[env]
    n, R = 9, 5
    states, win, raw, adv, tgt, w = _batch(sizes, n=n, R=R, seed=4)
    p = _params(sizes, 2)
    scale, mult = 3.0, 0.25
    (pl, vl, ent), gp, gv = A.grads(p, states, win, raw, adv, tgt, w, mult, scale)
    T = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    s = torch.tensor(states); x_t = torch.tensor(win)
    length = (x_t.abs().amax(2) > 0).sum(1)
    h = torch.zeros(n, 32, dtype=torch.float64)
    for t in range(R):
        x = x_t[:, t]
        gates = torch.sigmoid(torch.cat([x, h], 1) @ T["gru_gates_w"] + T["gru_gates_b"])
        r, u = gates[:, :32], gates[:, 32:]
        c = torch.tanh(torch.cat([x, r * h], 1) @ T["gru_cand_w"] + T["gru_cand_b"])
        h = torch.where((t < length)[:, None], u * h + (1 - u) * c, h)
    relu = torch.relu
    xx = torch.cat([relu(h @ T["temporal_w"] + T["temporal_b"]),
                    relu(relu(s @ T["static1_w"] + T["static1_b"]) @ T["static2_w"] + T["static2_b"])], 1)

    def tower(name):
        return torch.tanh(relu(xx @ T[name + "1_w"] + T[name + "1_b"]) @ T[name + "2_w"] + T[name + "2_b"]) @ T[name + "3_w"] + T[name + "3_b"]
    mu = 5.0 * torch.tanh(tower("mu"))
    sig = torch.sigmoid(tower("sigma")) + 1e-3
    dist = torch.distributions.Normal(mu, sig)
    cp = mult * torch.tensor(w) * torch.tensor(adv)
    loss_p = (-dist.log_prob(torch.tensor(raw)) * cp[:, None]).sum()
    v = scale * (torch.tanh(xx @ T["value1_w"] + T["value1_b"]) @ T["value2_w"] + T["value2_b"])[:, 0]
    loss_v = (mult * torch.tensor(w) * 0.5 * (v - torch.tensor(tgt)) ** 2 / scale).sum()
    ent_t = (torch.tensor(w)[:, None] * dist.entropy()).sum() / (sizes["num_actions"] * torch.tensor(w).sum())
    assert abs(loss_p.item() - pl) <= 1e-10 * max(1.0, abs(pl))
    assert abs(loss_v.item() - vl) <= 1e-10 * max(1.0, abs(vl))
    assert abs(ent_t.item() - ent) <= 1e-10
    for loss, g, blocks in ((loss_p, gp, A.POLICY_BLOCKS), (loss_v, gv, A.VALUE_BLOCKS)):
        nm = [k for k in A.names(**sizes) if k in blocks]
        tg = torch.autograd.grad(loss, [T[k] for k in nm], allow_unused=True, retain_graph=True)
        for k, t_ in zip(nm, tg):
            ref = np.zeros_like(g[k]) if t_ is None else t_.numpy()
            assert np.abs(g[k] - ref).max() <= 1e-8, k                    # the bound of test_oracle_nets_torch.py
            np.testing.assert_allclose(g[k], ref, rtol=1e-8, atol=1e-10, err_msg=k)


def test_rmsprop_and_lr_decay_hand_computed():
    sizes = A.SOLOW
    P = A.num_params(**sizes)
    # three steps on one weight; ms starts at 1
    w = np.array([1.0, 2.0]); ms = np.ones(2)
    g = [np.array([0.5, -1.0]), np.array([2.0, 0.0]), np.array([-0.1, 0.3])]
    lr = 1e-2
    m, x = 1.0, 1.0
    for gi in g:
        m = 0.99 * m + 0.01 * gi[0] ** 2
        x = x - lr * gi[0] / np.sqrt(m + 0.1)
        w, ms = A.rmsprop(w, gi, ms, lr)
        assert abs(ms[0] - m) < 1e-15 and abs(w[0] - x) < 1e-15
    # lr = lr0 * 0.96^(step / 1e5), not staircase; the global step advances by 2 per update
    assert A.lr_at(1e-4, 0) == 1e-4
    assert abs(A.lr_at(1e-4, 50000) - 1e-4 * 0.96 ** 0.5) < 1e-20
    assert abs(A.lr_at(1e-4, 100000) - 0.96e-4) < 1e-20
    r = A.block_ranges(**sizes)
    params = np.zeros(P); gp = np.zeros(P); gv = np.zeros(P)
    gp[0] = 3.0; gv[0] = 4.0; gv[-1] = 1.0; gp[r["mu1_w"][0]] = 1.0
    w2, msp, msv, step, lr_used, normp, normv = A.apply_update(params, gp, gv, np.ones(P), np.ones(P), 4, 1e-3, sizes, clip=2.0)
    assert step == 6 and lr_used == A.lr_at(1e-3, 4)
    assert abs(normp - np.sqrt(10.0)) < 1e-12 and abs(normv - np.sqrt(17.0)) < 1e-12
    gp0, gv0 = 3.0 * 2.0 / np.sqrt(10.0), 4.0 * 2.0 / np.sqrt(17.0)
    mp, mv = 0.99 + 0.01 * gp0 ** 2, 0.99 + 0.01 * gv0 ** 2
    assert abs(w2[0] - ((0.0 - lr_used * gp0 / np.sqrt(mp + 0.1)) - lr_used * gv0 / np.sqrt(mv + 0.1))) < 1e-15
    gm = 1.0 * 2.0 / np.sqrt(10.0)
    assert abs(w2[r["mu1_w"][0]] + lr_used * gm / np.sqrt(0.99 + 0.01 * gm ** 2 + 0.1)) < 1e-15
    assert msp[-1] == 1.0 and msv[r["mu1_w"][0]] == 1.0 and msv[r["sigma3_b"][0]] == 1.0     # slots a gradient never reaches stay at 1
    assert A.policy_mask(**sizes).sum() == r["value1_w"][0] and A.value_mask(**sizes).sum() == 7744 + 25089


@pytest.mark.parametrize("case", CASES)
def test_window_weight_and_draw_rules_against_the_reference(case):
    g = np.load(GOLD)
    R, T_MAX = int(g["max_seq_length"]), int(g["t_max"])
    k_ = case + "_"
    steps, n_tr = int(g[k_ + "steps"]), int(g[k_ + "n_transitions"])
    states = g[k_ + "step_states"]                                    # the processed state of every step taken, (steps, 2)
    # the window the policy saw at step k: the last min(k + 1, R) processed states, padded post
    for k in range(steps):
        np.testing.assert_array_equal(A.window(states[:k + 1], R), g[k_ + "step_hist"][k])
    dones = np.zeros((steps, 1)); dones[-1, 0] = float(g[k_ + "done"])
    term = np.zeros((steps, 1, 2)); term[-1, 0] = g[k_ + "history"][-1]
    win, wts, twin = A.replay_windows(states[:, None].astype(np.float32), dones, R, term.astype(np.float32))
    np.testing.assert_array_equal(win[:, 0], g[k_ + "step_hist"].astype(np.float32))
    # a transition is recorded iff the step index in the episode is >= R - 1 (worker.py:201)
    assert wts[:, 0].tolist() == [0.0] * (R - 1) + [1.0] * (steps - R + 1) and n_tr == steps - (R - 1)
    assert n_tr == (T_MAX if not g[k_ + "done"] else 9 - (R - 1))
    keep = wts[:, 0] > 0
    np.testing.assert_array_equal(states[keep], g[k_ + "tr_state"])
    assert g[k_ + "tr_done"].tolist() == [False] * (n_tr - 1) + [bool(g[k_ + "done"])]
    # the draw: raw = mu + sigma * n; the device keeps it as float32, the env gets the worker's sigmoid of it
    for k in range(steps):
        raw, ea = A.act(g[k_ + "step_mu"][k], g[k_ + "step_sigma"][k], g[k_ + "normals"][k])
        j = k - (R - 1)
        if j >= 0:
            assert raw[0] == np.float32(g[k_ + "tr_raw"][j])
            np.testing.assert_allclose(ea[0], g[k_ + "env_action"][j], rtol=1e-6)
    # the terminal window (the worker's history[-R:] once the next state is appended) where the episode ended
    if g[k_ + "done"]:
        np.testing.assert_array_equal(twin[-1, 0], g[k_ + "history"][-R:].astype(np.float32))
        np.testing.assert_array_equal(g[k_ + "tr_next"][-1], g[k_ + "history"][-1])


@pytest.mark.parametrize("case", CASES)
def test_update_feed_against_the_reference(case):
    g = np.load(GOLD)
    R, scale = int(g["max_seq_length"]), float(g["scale"])
    k_ = case + "_"
    ab, done = case.endswith("on"), bool(g[k_ + "done"])
    steps = int(g[k_ + "steps"])
    states = g[k_ + "step_states"]
    win, wts = A.replay_windows(states[:, None], np.zeros((steps, 1)), R)
    keep = wts[:, 0] > 0
    # the bootstrap: V(next state | window ending in it) unless the episode is over and always_bootstrap is off (worker.py:251-257)
    assert bool(g[k_ + "boot_called"]) == (ab or not done)
    if g[k_ + "boot_called"]:
        np.testing.assert_array_equal(g[k_ + "boot_state"], g[k_ + "tr_next"][-1])
        np.testing.assert_array_equal(g[k_ + "boot_hist"], g[k_ + "history"][-R:])
    else:
        assert float(g[k_ + "boot_value"]) == 0.0
    values = g[k_ + "values"].astype(np.float64)
    feed = A.update_feed(states[keep], win[keep, 0], g[k_ + "tr_raw"][:, None], g[k_ + "tr_reward"], values, float(g[k_ + "boot_value"]),
                         0.99, 0.96, scale)
    np.testing.assert_array_equal(feed["states"], g[k_ + "feed_states"])
    np.testing.assert_array_equal(feed["history"], g[k_ + "feed_history"])            # flipped in time with everything else
    np.testing.assert_array_equal(feed["actions"], g[k_ + "feed_actions"])
    # The value net's answers are float32.  Under the numpy the fixture was captured with (NEP 50), the worker's product
    # discount_factor * V_st[t + 1] of a Python float and a float32 scalar is rounded to float32; numpy 1.13, which the reference
    # pins, and this restatement keep it in float64.  So each delta may differ by one float32 rounding of 0.99 |V| <= max|V| 2^-24,
    # and the discounted sum of deltas by at most 1 / (1 - gamma lambda) times that.
    tol = np.abs(np.concatenate([values, [float(g[k_ + "boot_value"])]])).max() * 2.0 ** -24 / (1.0 - 0.99 * 0.96)
    np.testing.assert_allclose(feed["advantages"], g[k_ + "feed_adv"], rtol=1e-12, atol=tol / scale)
    np.testing.assert_allclose(feed["targets"], g[k_ + "feed_targets"], rtol=1e-12, atol=tol)
    # the batched form: the same numbers from gae_segments on the whole rollout column, weight-0 steps included
    v_all = np.zeros((steps, 1)); v_all[keep, 0] = values
    r_all = np.zeros((steps, 1)); r_all[keep, 0] = g[k_ + "tr_reward"]
    dn = np.zeros((steps, 1)); dn[-1, 0] = float(done)
    tv = np.zeros((steps, 1)); tv[-1, 0] = float(g[k_ + "boot_value"]) if done else 0.0
    boot = np.array([0.0 if done else float(g[k_ + "boot_value"])])
    adv, tgt = A.gae_segments(r_all, v_all, boot, dn, tv, ab, 0.99, 0.96, scale)
    np.testing.assert_allclose(adv[keep, 0][::-1], g[k_ + "feed_adv"], rtol=1e-12, atol=tol / scale)
    np.testing.assert_allclose(tgt[keep, 0][::-1], g[k_ + "feed_targets"], rtol=1e-12, atol=tol)
    np.testing.assert_allclose(adv[keep, 0][::-1], feed["advantages"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(tgt[keep, 0][::-1], feed["targets"], rtol=1e-12, atol=1e-12)


def test_gae_segments_matches_oracle_gae_without_dones_and_cuts_at_dones():
    rng = np.random.RandomState(1)
    r, v, b = rng.normal(size=(6, 3)), rng.normal(size=(6, 3)), rng.normal(size=3)
    for ab in (False, True):
        adv, tgt = A.gae_segments(r, v, b, np.zeros((6, 3)), rng.normal(size=(6, 3)), ab, 0.99, 0.96, 2.0)
        a2, t2 = A.O.gae(r, v, b, 0.99, 0.96)
        np.testing.assert_allclose(adv * 2.0, a2, rtol=1e-12)
        np.testing.assert_allclose(tgt, t2, rtol=1e-12)
    # a done at t = 2 of column 1: steps 0..2 are their own segment whose bootstrap is the terminal value (or 0)
    dn = np.zeros((6, 3)); dn[2, 1] = 1
    tv = np.zeros((6, 3)); tv[2, 1] = 0.7
    for ab, behind in ((True, 0.7), (False, 0.0)):
        adv, tgt = A.gae_segments(r, v, b, dn, tv, ab, 0.99, 0.96, 1.0)
        a_head, _ = A.O.gae(r[:3, 1:2], v[:3, 1:2], np.array([behind]), 0.99, 0.96)
        a_tail, _ = A.O.gae(r[3:, 1:2], v[3:, 1:2], b[1:2], 0.99, 0.96)
        np.testing.assert_allclose(adv[:3, 1], a_head[:, 0], rtol=1e-12)
        np.testing.assert_allclose(adv[3:, 1], a_tail[:, 0], rtol=1e-12)
    # with no term_values and always_bootstrap off it is the gated trader's masked GAE
    import _gated_oracle as G
    adv, tgt = A.gae_segments(r, v, b * (1 - dn[-1]), dn, None, False, 0.99, 0.96, 1.5)
    a3, t3 = G.gae_masked(r, v, b * (1 - dn[-1]), dn, 0.99, 0.96, 1.5)
    np.testing.assert_allclose(adv, a3, rtol=1e-12); np.testing.assert_allclose(tgt, t3, rtol=1e-12)


def test_worker_update_is_grads_on_the_feed_plus_both_rmsprop_steps():
    sizes = A.SOLOW
    g = np.load(GOLD)
    R = int(g["max_seq_length"])
    states = g["on_step_states"]
    win, wts = A.replay_windows(states[:, None], np.zeros((len(states), 1)), R)
    keep = wts[:, 0] > 0
    flat = A.flatten(_params(sizes, 5))
    P = flat.size
    raw = g["on_tr_raw"][:, None]
    (w2, msp, msv, step, lr, normp, normv), gp, gv, (pl, vl, ent) = A.worker_update(
        flat, sizes, np.ones(P), np.ones(P), 0, states[keep], win[keep, 0], raw, g["on_tr_reward"], 1.25, 1e-3, scale=100.0)
    p = A.unflatten(flat, **sizes)
    V = A.forward(p, states[keep], win[keep, 0], 100.0)[2]
    adv, tgt = A.O.gae(g["on_tr_reward"][:, None], V[:, None], np.array([1.25]), 0.99, 0.96)
    (pl2, vl2, _), gp2, gv2 = A.grads(p, states[keep], win[keep, 0], raw, adv[:, 0] / 100.0, tgt[:, 0], None, 1.0, 100.0)
    np.testing.assert_allclose(gp, A.flatten(gp2), rtol=1e-9, atol=1e-12)       # the order of the samples does not matter
    np.testing.assert_allclose(gv, A.flatten(gv2), rtol=1e-9, atol=1e-12)
    assert step == 2 and abs(pl - pl2) <= 1e-9 * abs(pl2) and abs(vl - vl2) <= 1e-9 * abs(vl2)
    assert abs(normp - np.linalg.norm(gp)) < 1e-9 and np.any(w2 != flat)


def _declared():
    text = open(os.path.join(ROOT, "include", "goldsrl_gaussnet.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_gauss_header_declared_exported_bound_and_defaults():
    from goldsrl import _ffi, _ffi_gauss
    lib = _ffi.load_library(extra_signatures=_ffi_gauss.ANET_SIGNATURES)
    declared = _declared()
    assert len(declared) == 17 and all(n.startswith("grl_anet_") for n in declared)
    for name in declared:
        assert hasattr(lib, name), name
    assert set(_ffi_gauss.ANET_SIGNATURES) == declared
    cfg = _ffi_gauss.GrlAnetConfig()
    assert lib.grl_anet_config_default(ctypes.byref(cfg)) == 0
    assert cfg.struct_size == ctypes.sizeof(_ffi_gauss.GrlAnetConfig)
    assert (cfg.rnn_length, cfg.lr_decay_steps, cfg.always_bootstrap) == (5, 100000, 0)
    for k, v in (("scale", 1.0), ("gamma", 0.99), ("gae_lambda", 0.96), ("clip_norm", 40.0), ("rms_decay", 0.99), ("rms_epsilon", 0.1),
                 ("lr_decay_rate", 0.96)):
        assert abs(getattr(cfg, k) - v) < 1e-7, k
    assert cfg.max_samples >= 1
    header = open(os.path.join(ROOT, "include", "goldsrl_gaussnet.h")).read()
    assert "148 547" in header and "149 285" in header
    for sizes in (A.SOLOW, A.TRADE):
        init = _ffi_gauss.default_init_gauss(3, **sizes)
        assert init.size == A.num_params(**sizes)
        assert [n for n, _ in _ffi_gauss.gauss_param_shapes(**sizes)] == A.names(**sizes)
        assert [s for _, s in _ffi_gauss.gauss_param_shapes(**sizes)] == [s for _, s in A.param_shapes(**sizes)]
        r = A.block_ranges(**sizes)
        assert (init[slice(*r["sigma3_b"])] == -1).all() and (init[slice(*r["gru_gates_b"])] == 1).all() and not init[slice(*r["mu3_b"])].any()
    # the stream id of the draw sits next to the gated trader's in the device source
    src = open(os.path.join(ROOT, "golds-rl-gym_amd", "csrc", "net_gauss.hip")).read()
    assert re.search(r"RS_GAUSS_ACTION\s*=\s*19\b", src) and A.RS_GAUSS_ACTION == 19
