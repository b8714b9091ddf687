"""CPU: the float64 restatement of the A3C discrete savings-grid agent (tests/_grid_oracle.py) against the reference's own acting,
window and update rules (tests/golden/grid_worker.npz, captured from GridSolowWorker), finite differences, an independent torch
autograd version and the zero-parameter case."""
import os

import numpy as np
import pytest

import _grid_oracle as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "grid_worker.npz")
CASES = [("k%d_%s_" % (K, c), K) for K in (51, 3) for c in ("on", "off", "short_on", "short_off")]


def _batch(K, n=6, R=5, seed=0):
    rng = np.random.RandomState(seed)
    states = rng.normal(size=(n, 2))
    win = rng.normal(size=(n, R, 2))
    for i in range(n):                      # ragged windows, zero rows after
        win[i, 1 + i % R:] = 0.0
    ch = rng.randint(0, K, size=n)
    adv = rng.normal(size=n)
    tgt = rng.normal(size=n)
    w = (rng.uniform(size=n) > 0.3).astype(float)
    return states, win, ch, adv, tgt, w


def _params(K, seed=1):
    p = D.init(seed, K)
    rng = np.random.RandomState(seed + 7)
    for k in p:                             # non-zero biases so that every block is exercised
        if k.endswith("_b"):
            p[k] = p[k] + 0.1 * rng.normal(size=p[k].shape)
    return p


def test_num_params_and_block_order():
    assert D.num_params(51) == 97140 and D.num_params(3) == 90948 and D.num_params(64) == 90561 + 129 * 64
    want = ["gru_gates_w", "gru_gates_b", "gru_cand_w", "gru_cand_b", "temporal_w", "temporal_b", "static1_w", "static1_b", "static2_w",
            "static2_b", "probs1_w", "probs1_b", "probs2_w", "probs2_b", "probs3_w", "probs3_b", "value1_w", "value1_b", "value2_w", "value2_b"]
    import _gauss_oracle as A
    for K in (3, 51):
        assert D.names(K) == want
        assert D.param_shapes(K)[:10] == A.param_shapes(**A.SOLOW)[:10]             # the ten trunk blocks of the Gaussian net
        r = D.block_ranges(K)
        assert r["probs1_w"][0] == 7744 and r["value1_w"][0] == 7744 + 96 * 256 + 256 + 256 * 128 + 128 + 129 * K
        p = _params(K)
        assert D.K_of(p) == K and np.array_equal(D.unflatten(D.flatten(p), K)["probs3_b"], p["probs3_b"])
        assert D.policy_mask(K).sum() == r["value1_w"][0] and D.value_mask(K).sum() == 7744 + 25089
    from goldsrl import _ffi_discrete
    for K in (3, 51):
        assert _ffi_discrete.discrete_param_shapes(K) == D.param_shapes(K)
        init = _ffi_discrete.default_init_discrete(3, K)
        r = D.block_ranges(K)
        assert init.size == D.num_params(K) and (init[slice(*r["gru_gates_b"])] == 1).all() and not init[slice(*r["probs3_b"])].any()


@pytest.mark.parametrize("K", [3, 51])
def test_zero_parameters_are_uniform_greedy_0_and_the_lower_bound(K):
    p = {n: np.zeros(s) for n, s in D.param_shapes(K)}
    states, win = _batch(K, n=9)[:2]
    probs, values = D.forward(p, states, win, scale=3.0)
    assert probs.shape == (9, K) and (probs == 1.0 / K).all() and not values.any()
    assert D.greedy(probs[0].astype(np.float32)) == 0 and D.grid(K)[0] == D.LB == 0.01
    g = D.grid(K)
    assert g[-1] == D.UB and g.dtype == np.float64 and (np.diff(g) > 0).all()
    # the sampler on the uniform float32 row: the cumulative sum's first crossing, and 0 where u is above the whole sum
    p32 = probs[0].astype(np.float32)
    cum = np.cumsum(p32, dtype=np.float32)
    assert D.choose(p32, 0.0) == 0 and D.choose(p32, float(cum[0])) == 1 and D.choose(p32, np.nextafter(float(cum[0]), 0)) == 0
    assert D.choose(p32, 2.0) == 0 and D.choose(p32, np.nextafter(float(cum[-1]), 0)) <= K - 1
    # an exact tie takes the first index
    assert D.greedy(np.array([0.2, 0.3, 0.3, 0.2], np.float32)) == 1


@pytest.mark.parametrize("K", [3, 51])
@pytest.mark.parametrize("which", ["policy", "value"])
def test_gradients_against_finite_differences(K, which):
    states, win, ch, adv, tgt, w = _batch(K)
    p = _params(K)
    scale = 2.0
    _, gp, gv = D.grads(p, states, win, ch, adv, tgt, w, 0.5, scale)
    g = gp if which == "policy" else gv
    k = 0 if which == "policy" else 1

    def f(q):
        return D.losses(q, states, win, ch, adv, tgt, w, 0.5, scale)[k]
    num = D.NN.numeric_grad(f, p, D.names(K), eps=1e-6, max_per=3, seed=3)
    for name, vals in num.items():
        for idx, v in vals:
            assert abs(g[name][idx] - v) <= 1e-6 + 1e-5 * abs(v), (name, idx, g[name][idx], v)
    blocks = D.POLICY_BLOCKS if which == "policy" else D.VALUE_BLOCKS
    for name in D.names(K):
        if name not in blocks:
            assert not np.any(g[name]), name
        elif name != "gru_gates_b":
            assert np.any(g[name]), name


def test_the_gradient_carries_the_epsilon():
    """With a chosen probability near 1e-7 the factor p / (p + 1e-7) is far from 1: finite differences see it."""
    K = 3
    states, win, ch, adv, tgt, w = _batch(K, n=4)
    p = _params(K)
    p["probs3_b"] = np.array([0.0, 16.0, -2.0])          # p_0 ~ 1e-7
    ch[:] = 0
    probs = D.forward(p, states, win)[0]
    assert 1e-8 < probs[:, 0].max() < 1e-6
    _, gp, _ = D.grads(p, states, win, ch, adv, tgt, None)

    def f(q):
        return D.losses(q, states, win, ch, adv, tgt, None)[0]
    num = D.NN.numeric_grad(f, p, ["probs3_b"], eps=1e-6, max_per=3, seed=1)
    for idx, v in num["probs3_b"]:
        assert abs(gp["probs3_b"][idx] - v) <= 1e-6 + 1e-5 * abs(v)
    plain = (adv[:, None] * (probs - np.eye(K)[ch])).sum(0)                  # the gradient without the factor
    assert np.abs(plain - gp["probs3_b"]).max() > 0.1 * np.abs(plain).max()


def test_losses_and_gradients_against_torch_autograd():
    import torch
    K, n, R = 51, 9, 5
    states, win, ch, adv, tgt, w = _batch(K, n=n, R=R, seed=4)
    p = _params(K, 2)
    scale, mult = 3.0, 0.25
    (pl, vl, ent), gp, gv = D.grads(p, states, win, ch, adv, tgt, w, mult, scale)
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
    logits = relu(relu(xx @ T["probs1_w"] + T["probs1_b"]) @ T["probs2_w"] + T["probs2_b"]) @ T["probs3_w"] + T["probs3_b"]
    probs = torch.softmax(logits, -1)
    pc = (torch.nn.functional.one_hot(torch.tensor(ch), K) * probs).sum(-1)
    wt = torch.tensor(w)
    loss_p = (mult * wt * torch.tensor(adv) * -torch.log(pc + 1e-7)).sum()
    v = scale * (torch.tanh(xx @ T["value1_w"] + T["value1_b"]) @ T["value2_w"] + T["value2_b"])[:, 0]
    loss_v = (mult * wt * 0.5 * (v - torch.tensor(tgt)) ** 2 / scale).sum()
    ent_t = (wt * -(probs * torch.log(probs + 1e-7)).sum(-1)).sum() / wt.sum()
    assert abs(loss_p.item() - pl) <= 1e-10 * max(1.0, abs(pl))
    assert abs(loss_v.item() - vl) <= 1e-10 * max(1.0, abs(vl))
    assert abs(ent_t.item() - ent) <= 1e-10
    for loss, g, blocks in ((loss_p, gp, D.POLICY_BLOCKS), (loss_v, gv, D.VALUE_BLOCKS)):
        nm = [k for k in D.names(K) if k in blocks]
        tg = torch.autograd.grad(loss, [T[k] for k in nm], allow_unused=True, retain_graph=True)
        for k, t_ in zip(nm, tg):
            ref = np.zeros_like(g[k]) if t_ is None else t_.numpy()
            assert np.abs(g[k] - ref).max() <= 1e-8, k


@pytest.mark.parametrize("pre,K", CASES)
def test_window_choice_and_grid_rules_against_the_reference(pre, K):
    g = np.load(GOLD)
    R, T_MAX = int(g["max_seq_length"]), int(g["t_max"])
    steps, n_tr = int(g[pre + "steps"]), int(g[pre + "n_transitions"])
    states = g[pre + "step_states"]
    dones = np.zeros((steps, 1)); dones[-1, 0] = float(g[pre + "done"])
    term = np.zeros((steps, 1, 2)); term[-1, 0] = g[pre + "history"][-1]
    win, wts, twin = D.replay_windows(states[:, None].astype(np.float32), dones, R, term.astype(np.float32))
    np.testing.assert_array_equal(win[:, 0], g[pre + "step_hist"].astype(np.float32))
    assert wts[:, 0].tolist() == [0.0] * (R - 1) + [1.0] * (steps - R + 1) and n_tr == steps - (R - 1)
    assert n_tr == (T_MAX if not g[pre + "done"] else 9 - (R - 1))
    keep = wts[:, 0] > 0
    np.testing.assert_array_equal(states[keep], g[pre + "tr_state"])
    # the draw and the grid: choices exact, the values the env was stepped with exact, at every step (recorded or not)
    grid = D.grid(K, float(g["lb"]), float(g["ub"]))
    probs = g[pre + "step_probs"]
    assert probs.dtype == np.float32 and probs.shape == (steps, K)
    choices = np.array([D.choose(probs[k], g[pre + "uniforms"][k]) for k in range(steps)])
    assert np.array_equal(choices[keep], g[pre + "tr_choice"])
    assert np.array_equal(grid[choices], g[pre + "step_env_action"])
    assert len(np.unique(choices)) >= 2
    if g[pre + "done"]:
        np.testing.assert_array_equal(twin[-1, 0], g[pre + "history"][-R:].astype(np.float32))


@pytest.mark.parametrize("pre,K", CASES)
def test_update_feed_against_the_reference(pre, K):
    g = np.load(GOLD)
    R, scale = int(g["max_seq_length"]), float(g["scale"])
    ab, done = pre.endswith("on_"), bool(g[pre + "done"])
    steps = int(g[pre + "steps"])
    states = g[pre + "step_states"]
    win, wts = D.replay_windows(states[:, None], np.zeros((steps, 1)), R)
    keep = wts[:, 0] > 0
    assert bool(g[pre + "boot_called"]) == (ab or not done)
    if g[pre + "boot_called"]:
        np.testing.assert_array_equal(g[pre + "boot_state"], g[pre + "tr_next"][-1])
        np.testing.assert_array_equal(g[pre + "boot_hist"], g[pre + "history"][-R:])
    else:
        assert float(g[pre + "boot_value"]) == 0.0
    values = g[pre + "values"].astype(np.float64)
    feed = D.update_feed(states[keep], win[keep, 0], g[pre + "tr_choice"], g[pre + "tr_reward"], values, float(g[pre + "boot_value"]),
                         0.99, 0.96, scale)
    np.testing.assert_array_equal(feed["states"], g[pre + "feed_states"])
    np.testing.assert_array_equal(feed["history"], g[pre + "feed_history"])
    assert g[pre + "feed_actions"].shape == (keep.sum(), 1) and np.issubdtype(g[pre + "feed_actions"].dtype, np.integer)
    np.testing.assert_array_equal(feed["actions"], g[pre + "feed_actions"])
    # one float32 rounding of 0.99 |V| per delta, as tests/test_oracle_gauss.py describes (the capture's numpy rounds the product of a
    # Python float and a float32 scalar to float32; numpy 1.13 and this restatement keep float64)
    tol = np.abs(np.concatenate([values, [float(g[pre + "boot_value"])]])).max() * 2.0 ** -24 / (1.0 - 0.99 * 0.96)
    np.testing.assert_allclose(feed["advantages"], g[pre + "feed_adv"], rtol=1e-12, atol=tol / scale)
    np.testing.assert_allclose(feed["targets"], g[pre + "feed_targets"], rtol=1e-12, atol=tol)
    # the batched form: gae_segments on the whole rollout column, weight-0 steps included
    v_all = np.zeros((steps, 1)); v_all[keep, 0] = values
    r_all = np.zeros((steps, 1)); r_all[keep, 0] = g[pre + "tr_reward"]
    dn = np.zeros((steps, 1)); dn[-1, 0] = float(done)
    tv = np.zeros((steps, 1)); tv[-1, 0] = float(g[pre + "boot_value"]) if done else 0.0
    boot = np.array([0.0 if done else float(g[pre + "boot_value"])])
    adv, tgt = D.gae_segments(r_all, v_all, boot, dn, tv, ab, 0.99, 0.96, scale)
    np.testing.assert_allclose(adv[keep, 0][::-1], g[pre + "feed_adv"], rtol=1e-12, atol=tol / scale)
    np.testing.assert_allclose(tgt[keep, 0][::-1], g[pre + "feed_targets"], rtol=1e-12, atol=tol)


def test_worker_update_is_grads_on_the_feed_plus_both_rmsprop_steps():
    K = 3
    g = np.load(GOLD)
    pre = "k3_on_"
    R = int(g["max_seq_length"])
    states = g[pre + "step_states"]
    win, wts = D.replay_windows(states[:, None], np.zeros((len(states), 1)), R)
    keep = wts[:, 0] > 0
    flat = D.flatten(_params(K, 5))
    P = flat.size
    (w2, msp, msv, step, lr, normp, normv), gp, gv, (pl, vl, ent) = D.worker_update(
        flat, K, np.ones(P), np.ones(P), 0, states[keep], win[keep, 0], g[pre + "tr_choice"], g[pre + "tr_reward"], 1.25, 1e-3)
    p = D.unflatten(flat, K)
    V = D.forward(p, states[keep], win[keep, 0])[1]
    adv, tgt = D.O.gae(g[pre + "tr_reward"][:, None], V[:, None], np.array([1.25]), 0.99, 0.96)
    _, gp2, gv2 = D.grads(p, states[keep], win[keep, 0], g[pre + "tr_choice"], adv[:, 0], tgt[:, 0])
    np.testing.assert_allclose(gp, D.flatten(gp2), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(gv, D.flatten(gv2), rtol=1e-9, atol=1e-12)
    assert step == 2 and abs(normp - np.linalg.norm(gp)) < 1e-9 and np.any(w2 != flat)
    # slots a gradient never reaches keep their ms at 1
    r = D.block_ranges(K)
    assert (msp[r["value1_w"][0]:] == 1).all() and (msv[slice(*r["probs1_w"])] == 1).all() and (msp[slice(*r["probs3_b"])] != 1).any()
