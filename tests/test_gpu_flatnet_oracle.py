"""The flat nets' training path at the sizes bench.py times, held to the float64 oracle (oracle/nets.py through _flat_oracle.py).

Solow (4 096 envs) and TradeAR1-16 (8 192 envs) train on one path: the persistent rollout keeps its activations (16 envs per
workgroup up to 4 096 envs, 32 up to 8 192), flat_backward_fast_kernel starts from that resident workspace on at most 256
workgroups -- each loops over 5 (Solow) or 10 (TradeAR1-16) groups of 64 samples and carries its LDS accumulators from one group to
the next -- then the slab reduction, the global norm, clip and Adam.  One warm-up update first (Adam has moved the parameters, the
TradeAR1 windows are full), then one measured rollout and update against the oracle: values and actions per sample, every gradient
block, the loss terms, the norm, the parameters and Adam's moments.  The size edges of the fast backward's group loop take the same
checks.  The oracle's own chunking is checked on the CPU."""
import time

import numpy as np
import pytest

import _adam_oracle as AO
import _flat_oracle as FO
from oracle import nets as NN
from oracle import oracle as O

# Per-block gradient bound (FO.block_errors) of the rollout path, from float32 measurements on the MI355X.  Largest block error
# measured: Solow 3.7e-4 (sig1_w, 4 096 envs) and 2.5e-4 (mu1_w, 4 100); TradeAR1-16 8.7e-5 (mu2_w, 8 192), 6.9e-5 (820), 6.1e-5
# (819) -- far above the explicit-history cases of test_gpu_flatnet.py (< 1e-6, random actions independent of the net's output).
# One 64-sample group left out or counted twice moved some block by 1.0e-2 or more in every case; the test asserts that it exceeds
# the bound.
GRAD_TOL = {"solow": 1e-3, "trade": 3e-4}


def _random_batch(n, S0, D, R, A, seed):
    rng = np.random.RandomState(seed)
    states = rng.normal(size=(n, S0)) * 0.3
    hist = rng.normal(size=(n, R, D)) * 0.3
    for i in range(n):
        hist[i, 1 + i % R:] = 0          # ragged lengths 1..R (zero rows end the sequence)
    return states, hist, rng.normal(size=(n, A)) * 2, rng.normal(size=n) * 0.3, rng.normal(size=n) * 40


@pytest.mark.parametrize("S0,D,R,A", [(2, 2, 5, 1), (33, 33, 20, 16)])     # Solow; TradeAR1-16
def test_the_chunked_oracle_equals_one_oracle_call(S0, D, R, A):
    """Chunks of 37 samples (307 = 8 x 37 + 11) and the five 64-sample groups (the last of 51) against one call over all samples."""
    n = 307
    p = NN.flat_init(seed=2, static_size=S0, temporal_size=D, num_actions=A)
    states, hist, act, adv, y = _random_batch(n, S0, D, R, A, seed=S0)
    loss, pl, cl, g, out = NN.flat_loss_and_grads(p, states, hist, act, adv, y, 100.0)
    win = FO.dense_windows(hist)
    c_loss, c_pl, c_cl, c_g, c_out = FO.loss_and_grads(p, states, win, act, adv, y, chunk=37)
    np.testing.assert_allclose([c_loss, c_pl, c_cl], [loss, pl, cl], rtol=1e-12, atol=0)
    parts = [FO.group_contribution(p, states, win, act, adv, y, k) for k in range(5)]
    for k in g:
        scale = np.abs(g[k]).max()
        np.testing.assert_allclose(c_g[k], g[k], rtol=1e-12, atol=1e-12 * scale)
        np.testing.assert_allclose(sum(q[k] for q in parts), g[k], rtol=1e-12, atol=1e-12 * scale)
    for a, b in zip(c_out, out):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * np.abs(b).max())
    # the TradeAR1 window: the state in rows < max(nhist, 1), capped at rnn
    nh = np.random.RandomState(1).randint(0, R + 3, size=n)
    dense = np.zeros((n, R, S0))
    for i in range(n):
        dense[i, :min(max(nh[i], 1), R)] = states[i]
    assert np.array_equal(FO.repeated_state_windows(states, nh, R)(5, 300), dense[5:300])
    # an altered gradient is as far from the true one as the group it changes
    alt = FO.altered(g, {"group 4 left out": (-1.0, parts[4])})
    e, k = FO.sensitivity(g, alt)["group 4 left out"]
    np.testing.assert_allclose(e, np.abs(parts[4][k]).max() / np.abs(g[k]).max(), rtol=1e-9)
    assert e == max(FO.block_errors(alt["group 4 left out"], g).values()) > 0.01


def _action_noise(seed, env_off, E, T, A, counter0):
    """eps of flat_sample_kernel (net_flat.hip:186-196): normal_pair(rng_block(seed, env + env_off, counter0 + t, 17, k >> 1))[k & 1]."""
    env = np.arange(E, dtype=np.uint64)[:, None] + np.uint64(env_off)
    pair = np.arange((A + 1) // 2, dtype=np.uint64)[None, :]
    eps = np.empty((T, E, A))
    for t in range(T):
        e0, e1 = O.normal_pair(O.rng_block(seed, env, counter0 + t, 17, pair))
        eps[t] = np.stack([e0, e1], axis=-1).reshape(E, -1)[:, :A]
    return eps


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind,E,cap", [
    ("solow", 4096, 8),       # bench: 81 920 samples; 16 envs per rollout workgroup; 1 280 groups, 5 per backward workgroup
    ("trade", 8192, 30),      # bench: 163 840 samples; 32 envs per rollout workgroup; 2 560 groups, 10 per backward workgroup
    ("trade", 820, 30),       # 257 groups: workgroup 0 loops twice, its second group is the partial one (16 samples)
    ("trade", 819, 30),       # 256 groups, the last partial (60 samples), no workgroup loops
    ("solow", 4100, 8),       # 32 envs per rollout workgroup, the last of 129 holds 4; 1 282 groups, the last partial; E % 64 != 0
])
def test_the_keeping_rollout_and_its_update_match_the_oracle(kind, E, cap, monkeypatch):
    from goldsrl import _ffi
    from goldsrl import rollout as RO
    T, lr, seed, tol = 20, 1e-3, 11, GRAD_TOL[kind]
    for v in ("GRL_FLAT_KEEP", "GRL_FLAT_GROUP", "GRL_FLAT_ROLLOUT", "GRL_FLAT_FORWARD"):
        monkeypatch.delenv(v, raising=False)
    if kind == "solow":
        eng = _ffi.Engine(_ffi.ENV_SOLOW, E, seed=seed, rnn_length=5, max_episode_steps=cap)
    else:
        eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=seed, n_assets=16, rnn_length=20, max_episode_steps=cap)
    eng.reset()
    roll = RO.FlatPolicyRollout(eng, T, train=True, lr=lr)
    net, cfg = roll.net, roll.net.cfg
    assert roll.keep_activations
    S0, R, A, N, scale, clip_norm = cfg.static_size, cfg.rnn_length, cfg.num_actions, T * E, cfg.scale, cfg.clip_norm
    env_off = int(eng.cfg.env_id_offset)
    roll.run(); eng.wait()      # warm-up update: Adam moves the parameters off their init, the TradeAR1 windows fill up
    assert np.isfinite(roll.last_stats["loss"])
    params = net.get_params()
    counter0 = net.get_action_counter()
    net.set_keep_activations(True)
    net.rollout(T); eng.wait()

    def rd(k, *shape):
        return net.read_rollout(k, (T, E) + shape)
    states, acts, vals = rd("states", S0).reshape(N, S0), rd("actions", A).reshape(N, A), rd("values").reshape(N)
    adv, y, masks, nh = rd("adv").reshape(N), rd("y").reshape(N), rd("masks"), rd("nhist").view(np.int32)
    hist = rd("histories", R, 2).reshape(N, R, 2) if kind == "solow" else None
    stats = net.train_rollout_grads()      # from the resident workspace, as the bench's update
    grads = net.get_grads()
    opt = net.get_optimizer_state()
    applied = net.apply_grads(lr)
    params1, opt1 = net.get_params(), net.get_optimizer_state()
    net.close(); eng.close()

    # the measured rollout holds full windows, rows right after a TimeLimit reset, and partial windows
    after_reset = np.zeros((T, E), bool)
    after_reset[1:] = masks[:-1] == 0
    assert after_reset.any() and (nh[after_reset] == 1).all()
    assert (nh >= R).any() and ((nh > 1) & (nh < R)).any()

    shapes = NN.flat_param_shapes(S0, S0, 32, 32, A)
    p = NN.unflatten_params(params.astype(np.float64), shapes)
    win = FO.dense_windows(hist) if kind == "solow" else FO.repeated_state_windows(states, nh, R)
    t0 = time.time()
    loss, pl, cl, g, (mu, sigma, vs) = FO.loss_and_grads(p, states, win, acts, adv, y, scale)
    groups = (N + 63) // 64
    drop = 256 if groups > 256 else groups - 1      # the first group workgroup 0 carries its accumulators into; else the partial one

    def part(k):
        return FO.group_contribution(p, states, win, acts, adv, y, k, scale)
    sens = FO.sensitivity(g, FO.altered(g, {"group %d left out" % drop: (-1.0, part(drop)), "group 0 twice": (1.0, part(0))}))
    oracle_s = time.time() - t0
    err = FO.block_errors(NN.unflatten_params(grads.astype(np.float64), shapes), g)
    eps = _action_noise(seed, env_off, E, T, A, counter0).reshape(N, A)
    act_err = np.abs(acts - (mu + sigma * eps))
    worst = max(err, key=err.get)
    print("\n[flat oracle] %s E=%d: block error %.3g (%s), tolerance %.3g, altered %s, margin %.1fx; |dvalue| %.3g, |daction| %.3g; "
          "oracle %.1f s" % (kind, E, err[worst], worst, tol, {k: "%.3g (%s)" % v for k, v in sens.items()},
                             min(e for e, _ in sens.values()) / tol, np.abs(vals - vs).max(), act_err.max(), oracle_s))

    # a. forward, per sample: stored values; stored raw actions = mu + sigma * eps with the sample kernel's draws
    np.testing.assert_allclose(vals, vs, rtol=2e-5, atol=2e-4)
    assert (act_err <= 2e-5 * (1 + np.abs(mu)) + np.abs(eps) * (2e-6 + 2e-5 * sigma)).all(), act_err.max()
    # b. gradient: every block and the loss terms
    np.testing.assert_allclose([stats["loss"], stats["policy_loss"], stats["critic_loss_mean"]], [loss, pl, cl], rtol=1e-4, atol=1e-6)
    # c. the bound would see one group left out or counted twice; the device gradient lies within it
    for label, (e, k) in sens.items():
        assert e > tol, (label, e, k)
    for k, e in err.items():
        assert e < tol, (k, e)
    # d. global norm against the oracle's; clip + Adam on the device's own gradient (float32 rounding of each operation)
    np.testing.assert_allclose(applied["global_norm"], np.sqrt(sum((v ** 2).sum() for v in g.values())), rtol=1e-4)
    step = opt["adam_step"]
    assert step == 1 and opt1["adam_step"] == step + 1
    AO.assert_within(AO.reference(grads, opt["adam_m"], opt["adam_v"], params, step + 1, lr, clip_norm), params1, opt1["adam_m"], opt1["adam_v"])
    assert not np.array_equal(params1, params)
