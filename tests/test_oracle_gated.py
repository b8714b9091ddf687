"""CPU: the float64 restatement of the Ticker gated trader (tests/_gated_oracle.py) against finite differences, an independent
torch autograd version, a hand-computed RMSProp example and the reference's own acting / window rules
(tests/golden/gated_worker.npz); the C header of the gated net against the library and its binding."""
import ctypes
import os
import re

import numpy as np
import pytest

import _gated_oracle as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gated_worker.npz")


def _batch(n=6, R=5, seed=0):
    rng = np.random.RandomState(seed)
    states = rng.normal(size=(n, 7))
    win = rng.normal(size=(n, R, 4))
    for i in range(n):                      # ragged windows, zero rows after
        win[i, 1 + i % R:] = 0.0
    choices = rng.randint(0, 3, size=(n, 2))
    raw = rng.normal(size=(n, 2))
    adv = rng.normal(size=n)
    tgt = rng.normal(size=n)
    w = (rng.uniform(size=n) > 0.3).astype(float)
    return states, win, choices, raw, adv, tgt, w


def _params(seed=1):
    p = G.init(seed)
    rng = np.random.RandomState(seed + 7)
    for k in p:                             # non-zero biases so that every block is exercised
        if k.endswith("_b"):
            p[k] = p[k] + 0.1 * rng.normal(size=p[k].shape)
    return p


def test_num_params_and_block_order():
    assert G.NUM_PARAMS == 151123
    r = G.block_ranges()
    assert r["class1_w"][0] == 8256 and r["value1_w"][0] == 8256 + 117778
    p = _params()
    assert np.array_equal(G.unflatten(G.flatten(p))["normal3_b"], p["normal3_b"])


@pytest.mark.parametrize("which", ["policy", "value"])
def test_gradients_against_finite_differences(which):
    states, win, ch, raw, adv, tgt, w = _batch()
    p = _params()
    scale = 2.0
    _, gp, gv = G.grads(p, states, win, ch, raw, adv, tgt, w, 0.5, scale)
    g = gp if which == "policy" else gv
    k = 0 if which == "policy" else 1

    def f(q):
        return G.losses(q, states, win, ch, raw, adv, tgt, w, 0.5, scale)[k]
    num = G.NN.numeric_grad(f, p, [n for n, _ in G.SHAPES], eps=1e-6, max_per=3, seed=3)
    for name, vals in num.items():
        for idx, v in vals:
            assert abs(g[name][idx] - v) <= 1e-6 + 1e-5 * abs(v), (name, idx, g[name][idx], v)
    blocks = G.POLICY_BLOCKS if which == "policy" else G.VALUE_BLOCKS
    for name, _ in G.SHAPES:
        if name not in blocks:
            assert not np.any(g[name]), name
        elif name != "gru_gates_b":
            assert np.any(g[name]), name


def test_losses_and_gradients_against_torch_autograd():
    torch = pytest.importorskip("torch")
    states, win, ch, raw, adv, tgt, w = _batch(n=9, R=5, seed=4)
    p = _params(2)
    scale, mult = 3.0, 0.25
    (pl, vl, _), gp, gv = G.grads(p, states, win, ch, raw, adv, tgt, w, mult, scale)
    T = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    s = torch.tensor(states); x_t = torch.tensor(win)
    length = (x_t.abs().amax(2) > 0).sum(1)
    h = torch.zeros(9, 32, dtype=torch.float64)
    for t in range(5):
        x = x_t[:, t]
        gates = torch.sigmoid(torch.cat([x, h], 1) @ T["gru_gates_w"] + T["gru_gates_b"])
        r, u = gates[:, :32], gates[:, 32:]
        c = torch.tanh(torch.cat([x, r * h], 1) @ T["gru_cand_w"] + T["gru_cand_b"])
        h = torch.where((t < length)[:, None], u * h + (1 - u) * c, h)
    relu = torch.relu
    xx = torch.cat([relu(h @ T["temporal_w"] + T["temporal_b"]),
                    relu(relu(s @ T["static1_w"] + T["static1_b"]) @ T["static2_w"] + T["static2_b"])], 1)
    logits = (relu(relu(xx @ T["class1_w"] + T["class1_b"]) @ T["class2_w"] + T["class2_b"]) @ T["class3_w"] + T["class3_b"]).reshape(9, 2, 3)
    logp = torch.log_softmax(logits, -1)
    nrm = (relu(relu(xx @ T["normal1_w"] + T["normal1_b"]) @ T["normal2_w"] + T["normal2_b"]) @ T["normal3_w"] + T["normal3_b"]).reshape(9, 2, 3, 2)
    mu, sig = nrm[..., 0], torch.nn.functional.softplus(nrm[..., 1]) + 1e-7
    chi = torch.tensor(ch)
    lp = logp.gather(2, chi[..., None])[..., 0]
    mc, sc = mu.gather(2, chi[..., None])[..., 0], sig.gather(2, chi[..., None])[..., 0]
    dist = torch.distributions.Normal(mc, sc)
    cp = mult * torch.tensor(w) * torch.tensor(adv)
    loss_p = ((-lp - dist.log_prob(torch.tensor(raw))) * cp[:, None]).sum()
    v = scale * (torch.tanh(xx @ T["value1_w"] + T["value1_b"]) @ T["value2_w"] + T["value2_b"])[:, 0]
    loss_v = (mult * torch.tensor(w) * 0.5 * (v - torch.tensor(tgt)) ** 2 / scale).sum()
    assert abs(loss_p.item() - pl) <= 1e-10 * max(1.0, abs(pl))
    assert abs(loss_v.item() - vl) <= 1e-10 * max(1.0, abs(vl))
    for loss, g, blocks in ((loss_p, gp, G.POLICY_BLOCKS), (loss_v, gv, G.VALUE_BLOCKS)):
        names = [n for n, _ in G.SHAPES if n in blocks]
        tg = torch.autograd.grad(loss, [T[n] for n in names], allow_unused=True, retain_graph=True)
        for n, t_ in zip(names, tg):
            ref = np.zeros_like(g[n]) if t_ is None else t_.numpy()
            np.testing.assert_allclose(g[n], ref, rtol=1e-10, atol=1e-10, err_msg=n)


def test_rmsprop_and_lr_decay_hand_computed():
    # three steps on one weight that both gradients reach and one only the policy reaches; ms starts at 1
    w = np.array([1.0, 2.0]); ms = np.ones(2)
    g = [np.array([0.5, -1.0]), np.array([2.0, 0.0]), np.array([-0.1, 0.3])]
    lr = 1e-2
    expect_ms, expect_w = [], []
    m, x = 1.0, 1.0
    for gi in g:
        m = 0.99 * m + 0.01 * gi[0] ** 2
        x = x - lr * gi[0] / np.sqrt(m + 0.1)
        expect_ms.append(m); expect_w.append(x)
    for k, gi in enumerate(g):
        w, ms = G.rmsprop(w, gi, ms, lr)
        assert abs(ms[0] - expect_ms[k]) < 1e-15 and abs(w[0] - expect_w[k]) < 1e-15
    assert abs(ms[0] - 0.99 * (0.99 * (0.99 + 0.01 * 0.25) + 0.01 * 4.0) - 0.01 * 0.01) < 1e-15
    # lr = lr0 * 0.96^(step / 1e5), not staircase; the global step advances by 2 per update
    assert G.lr_at(1e-4, 0) == 1e-4
    assert abs(G.lr_at(1e-4, 50000) - 1e-4 * 0.96 ** 0.5) < 1e-20
    assert abs(G.lr_at(1e-4, 100000) - 0.96e-4) < 1e-20
    params = np.zeros(G.NUM_PARAMS)
    gp = np.zeros(G.NUM_PARAMS); gv = np.zeros(G.NUM_PARAMS)
    gp[0] = 3.0; gv[0] = 4.0; gv[-1] = 1.0; gp[G.block_ranges()["class1_w"][0]] = 1.0
    w2, msp, msv, step, lr_used, normp, normv = G.apply_update(params, gp, gv, np.ones(G.NUM_PARAMS), np.ones(G.NUM_PARAMS), 4, 1e-3, clip=2.0)
    assert step == 6 and lr_used == G.lr_at(1e-3, 4)
    assert abs(normp - np.sqrt(10.0)) < 1e-12 and abs(normv - np.sqrt(17.0)) < 1e-12
    gp0, gv0 = 3.0 * 2.0 / np.sqrt(10.0), 4.0 * 2.0 / np.sqrt(17.0)
    mp, mv = 0.99 + 0.01 * gp0 ** 2, 0.99 + 0.01 * gv0 ** 2
    assert abs(w2[0] - ((0.0 - lr_used * gp0 / np.sqrt(mp + 0.1)) - lr_used * gv0 / np.sqrt(mv + 0.1))) < 1e-15
    assert msp[-1] == 1.0 and msv[G.block_ranges()["class1_w"][0]] == 1.0     # slots a gradient never reaches stay at 1


def test_draw_and_window_rules_against_the_reference():
    g = np.load(GOLD)
    probs, u = g["probs"], g["u"]
    got = np.array([G.discrete_choice(probs[k], u[k]) for k in range(len(u))])
    assert np.array_equal(got, g["choices"])
    assert got[1] == 0 and got[2] == 0           # u at or above the last cumsum value: the reference's argmax of an all-False row
    for k in range(0, len(u), 2):
        ch = got[k:k + 2]
        env_probs = probs[k:k + 2]; mu = g["mu"][k:k + 2]; sg = g["sigma"][k:k + 2]
        c2, raw, frac = G.act(env_probs, mu, sg, u[k:k + 2], g["normals"][k:k + 2])
        assert np.array_equal(c2, ch)
        np.testing.assert_array_equal(raw, g["raw"][k:k + 2].astype(np.float32))
        np.testing.assert_allclose(frac, g["frac"][k:k + 2], rtol=1e-6)
    assert np.array_equal(g["disc"], g["choices"])
    # process_temporal_states: the last 4 columns; the window pads them post to R
    hist = g["history"]
    np.testing.assert_array_equal(hist[:, 3:], g["temporal"])
    w = G.window(hist[:3, 3:], 5)
    assert np.array_equal(w[:3], g["temporal"][:3]) and not w[3:].any()
    assert np.array_equal(G.window(hist[:, 3:], 5), g["temporal"][-5:])


def test_replay_windows_and_weights():
    T, E, R = 7, 2, 3
    rng = np.random.RandomState(0)
    states = rng.normal(size=(T, E, 7))
    dones = np.zeros((T, E)); dones[3, 1] = 1
    win, wts = G.replay_windows(states, dones, R)
    assert wts[:, 0].tolist() == [0, 0, 1, 1, 1, 1, 1]
    assert wts[:, 1].tolist() == [0, 0, 1, 1, 0, 0, 1]         # restarts after the done at t = 3
    np.testing.assert_array_equal(win[5, 1, :2], states[4:6, 1, 3:].astype(np.float32))
    assert not win[5, 1, 2:].any()


def test_masked_gae_matches_oracle_gae_without_dones():
    rng = np.random.RandomState(1)
    r, v, b = rng.normal(size=(6, 3)), rng.normal(size=(6, 3)), rng.normal(size=3)
    adv, tgt = G.gae_masked(r, v, b, np.zeros((6, 3)), 0.99, 0.96, 2.0)
    a2, t2 = G.O.gae(r, v, b, 0.99, 0.96)
    np.testing.assert_allclose(adv * 2.0, a2, rtol=1e-12)
    np.testing.assert_allclose(tgt, t2, rtol=1e-12)


def _declared_gated():
    text = open(os.path.join(ROOT, "include", "goldsrl_gatednet.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(grl_[a-z0-9_]+)\s*\(", text))


def test_gated_header_declared_exported_bound_and_defaults():
    from goldsrl import _ffi, _ffi_gated
    lib = _ffi.load_library(extra_signatures=_ffi_gated.GNET_SIGNATURES)
    declared = _declared_gated()
    assert len(declared) == 17
    for name in declared:
        assert hasattr(lib, name), name
    assert set(_ffi_gated.GNET_SIGNATURES) == declared
    cfg = _ffi_gated.GrlGnetConfig()
    assert lib.grl_gnet_config_default(ctypes.byref(cfg)) == 0
    assert cfg.struct_size == ctypes.sizeof(_ffi_gated.GrlGnetConfig)
    assert (cfg.rnn_length, cfg.lr_decay_steps) == (5, 100000)
    for k, v in (("scale", 1.0), ("gamma", 0.99), ("gae_lambda", 0.96), ("clip_norm", 40.0), ("rms_decay", 0.99), ("rms_epsilon", 0.1),
                 ("lr_decay_rate", 0.96)):
        assert abs(getattr(cfg, k) - v) < 1e-7, k
    assert cfg.max_samples >= 1
    assert _ffi_gated.default_init_gated().size == G.NUM_PARAMS
    assert [n for n, _ in _ffi_gated.gated_param_shapes()] == [n for n, _ in G.SHAPES]
