"""GPU: the grid trader learning from the attainable optimum's table (include/goldsrl_gridtradeteach.h; csrc/net_gridtrade.hip:
gt_teach_forward_kernel, gt_teach_backward_kernel) -- the teacher against the play of the same table, the coin against the oracle's
uniforms, the supervised update against tests/_gridtrade_teach_oracle.py, the rollout update against the host update, the refusals.

Bounds: GRAD_REL_BOUND and the stat tolerances of tests/test_gpu_gridtradenet.py.  The numpy look-up trade_dp_actions is held to 2^-23
as in tests/test_gpu_trade_dp.py (numpy's log and the device's differ in the last place); the device's two readers byte for byte."""
import numpy as np
import pytest

import _gridtrade_oracle as GT
import _gridtrade_teach_oracle as TT
from test_gpu_discretenet import GRAD_REL_BOUND
from test_gpu_gridtradenet import KS, _as64, _block_err, _engine, _net, _params, _samples

pytestmark = pytest.mark.gpu
E, HORIZON = 130, 3                                          # two full groups of 64 envs and a ragged one
READ = ("teacher_actions", "label_lo", "label_w", "choices", "actions", "rewards")


def _taught(K, cap, **kw):
    """an engine with a small solved table and a TimeLimit `cap`, its net, the table"""
    from goldsrl._ffi_tradedp import trade_dp_grid, trade_dp_solve
    eng = _engine(E, seed=7, max_episode_steps=cap, env_id_offset=300)
    grid = trade_dp_grid(nu=5, nx=5, na=5, nq=3, std_p=eng.cfg.trade_std_p)
    sol = trade_dp_solve(eng, grid, HORIZON)
    net = _net(eng, **dict(dict(rnn_length=5, num_choices=K, max_samples=6 * E), **kw))
    net.set_params(_params(K))
    net.set_action_counter(50)
    return eng, net, grid, sol["policy"]


@pytest.mark.parametrize("K", KS)
def test_teacher_is_the_play_bit_for_bit(K):
    """TimeLimit T + 2: moves left 6 .. 2 against a horizon of 3, so the row is capped on the first steps and not on the last."""
    from goldsrl._ffi_gridtrade import trade_grid_labels
    from goldsrl._ffi_tradedp import trade_dp_play
    T = 5
    eng, net, _, _ = _taught(K, T + 2)
    play = trade_dp_play(eng, T, T)                           # leaves the handle untouched
    net.teach_rollout(T, agent_share=0.0)
    r = {k: net.read_rollout(k) for k in READ}
    assert r["teacher_actions"].shape == (T, E, 2) and len(np.unique(play["actions"])) > 2 and (play["length"] == T).all()
    assert r["teacher_actions"].tobytes() == play["actions"].tobytes() and r["actions"].tobytes() == play["actions"].tobytes()
    assert r["rewards"].tobytes() == play["rewards"].tobytes()
    lo, w = trade_grid_labels(play["actions"], K)
    assert r["label_lo"].dtype == np.int32 and np.array_equal(r["label_lo"], lo) and r["label_w"].tobytes() == w.tobytes()
    assert net.get_action_counter() == 50 + T
    net.close(); eng.close()


@pytest.mark.parametrize("K", KS)
def test_agent_share_one_is_the_plain_rollout_with_labels(K):
    from goldsrl._ffi_tradedp import trade_dp_actions
    eng, net, grid, policy = _taught(K, 4)
    eng2, plain, _, _ = _taught(K, 4)
    for t in range(2):                                        # T = 2 as two single-step calls: the raw account is read between them
        cash, q, p = (eng.get_state(k) for k in ("TRADE_CASH", "TRADE_QUANTITY", "TRADE_PRICES"))
        want = trade_dp_actions(policy, grid, HORIZON, cash, q.reshape(E, 2), p.reshape(E, 2), 4 - eng.get_state("ELAPSED"))
        net.teach_rollout(1, agent_share=1.0)
        plain.rollout(1)
        for k in ("choices", "actions", "rewards"):
            assert net.read_rollout(k).tobytes() == plain.read_rollout(k).tobytes(), (k, t)
        assert np.abs(net.read_rollout("teacher_actions")[0] - want).max() <= 2.0 ** -23, t
    assert np.abs(want).max() > 0
    net.close(); eng.close(); plain.close(); eng2.close()


def test_the_coin_is_the_oracles_uniform():
    K, T = 17, 3
    eng, net, _, _ = _taught(K, 0)
    net.teach_rollout(T, agent_share=0.5)
    r = {k: net.read_rollout(k) for k in READ}
    own = GT.grid(K)[r["choices"]].astype(np.float32)
    for t in range(T):
        agent = TT.coin(eng.cfg.seed, np.arange(E) + 300, 50 + t) < 0.5
        assert agent.any() and not agent.all()
        assert r["actions"][t].tobytes() == np.where(agent[:, None], own[t], r["teacher_actions"][t]).tobytes(), t
    net.close(); eng.close()


def _labelled(K, n, R, seed):
    """_samples with labels: w = 0, w inside (0, 1), lo = K - 2 with w = 1, labels that differ between the outputs"""
    s, win, _, _, tgt, wt = _samples(K, n, R, seed)
    rng = np.random.RandomState(seed + 1)
    lo = rng.randint(0, K - 1, size=(n, 2)).astype(np.int32)
    w = rng.uniform(0.05, 0.95, size=(n, 2)).astype(np.float32)
    w[::3, 0] = 0.0
    w[1::4, 1] = 0.5
    lo[:2], w[:2] = [[K - 2, 0], [0, K - 2]], [[1.0, 0.0], [0.25, 1.0]]
    return s, win, lo, w, tgt, wt


@pytest.mark.parametrize("K", KS)
def test_host_teach_gradients_stats_and_update(K):
    n, R, mult = 130, 5, 0.3
    P = GT.num_params(K)
    eng = _engine(65)
    net = _net(eng, rnn_length=R, clip_norm=0.5, num_choices=K)
    flat = _params(K)
    net.set_params(flat)
    net.set_optimizer_state(np.ones(P, np.float32), np.ones(P, np.float32), 200000)
    s, win, lo, w, tgt, wt = _labelled(K, n, R, 11)
    assert (wt == 0).any() and (w == 0).any() and (w == 1).any() and ((lo != lo[:, ::-1]).any() or K == 2)
    stats = net.teach(s, win, lo, w, tgt, wt, grad_mult=mult, lr=1e-3, apply_update=False)
    gp, gv = net.get_grads("policy"), net.get_grads("value")
    (ce, vl, ent, agree), rp, rv = TT.grads(_as64(K, flat), s, win, lo, w, tgt, wt, mult)
    rp, rv = GT.flatten(rp), GT.flatten(rv)
    (ep, bp), (ev, bv) = _block_err(K, gp, rp), _block_err(K, gv, rv)
    print("K=%d worst block error: policy %.3g (%s), value %.3g (%s)" % (K, ep, bp, ev, bv))
    assert ep < GRAD_REL_BOUND["policy"] and ev < GRAD_REL_BOUND["value"], (ep, bp, ev, bv)
    np.testing.assert_allclose([stats["cross_entropy"], stats["value_loss"], stats["entropy_mean"], stats["agreement"]], [ce, vl, ent, agree], rtol=1e-4)
    net.teach(s, win, lo, w, tgt, wt, grad_mult=mult, lr=1e-3, apply_update=True)
    st = net.get_optimizer_state()
    w_ref, msp, msv = GT.apply_update(flat.astype(np.float64), gp.astype(np.float64), gv.astype(np.float64), np.ones(P), np.ones(P), 200000,
                                      1e-3, K, clip=0.5)[:3]
    assert st["global_step"] == 200002
    np.testing.assert_allclose(net.get_params(), w_ref, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(st["ms_policy"], msp, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(st["ms_value"], msv, rtol=1e-6, atol=1e-12)
    net.close(); eng.close()


def test_rollout_update_is_the_host_update():
    K, T, R = 17, 6, 3                                        # the sizes of test_rollout_replay_and_rollout_update: windows fill
    eng, net, _, _ = _taught(K, 4, rnn_length=R)              # TimeLimit 4: episodes end inside the rollout
    flat, P = _params(K), GT.num_params(K)
    net.teach_rollout(T, agent_share=0.0)
    r = {k: net.read_rollout(k) for k in ("states", "windows", "label_lo", "label_w", "targets", "weights", "dones")}
    assert r["dones"][3].all() and r["weights"].any() and (r["label_w"] > 0).any()
    st_ro = net.train_teach_rollout(lr=1e-3)
    g_ro, p_ro = (net.get_grads("policy"), net.get_grads("value")), net.get_params()
    net.set_params(flat)
    net.set_optimizer_state(np.ones(P, np.float32), np.ones(P, np.float32), 0)
    st = net.teach(r["states"].reshape(-1, 5), r["windows"].reshape(-1, R, 5), r["label_lo"].reshape(-1, 2), r["label_w"].reshape(-1, 2),
                   r["targets"].reshape(-1), r["weights"].reshape(-1), grad_mult=1.0 / E, lr=1e-3)
    assert np.array_equal(net.get_grads("policy"), g_ro[0]) and np.array_equal(net.get_grads("value"), g_ro[1]) and g_ro[0].any()
    assert np.array_equal(net.get_params(), p_ro) and not np.array_equal(p_ro, flat)
    assert st == pytest.approx(st_ro, rel=1e-6)      # the loss sums are atomic: their order is free
    net.close(); eng.close()


def test_refusals():
    from goldsrl import _ffi
    K = 17
    eng = _engine(65)
    net = _net(eng, rnn_length=5, num_choices=K)
    net.set_params(_params(K))

    def refused(code, msg, call, *a, **kw):
        with pytest.raises(_ffi.GrlError, match=msg) as ei:
            call(*a, **kw)
        assert ei.value.code == code

    refused(_ffi.E_STATE, "holds no table", net.teach_rollout, 2)
    eng2, taught, _, _ = _taught(K, 0)
    refused(_ffi.E_INVALID, "-0.1", taught.teach_rollout, 2, agent_share=-0.1)
    refused(_ffi.E_INVALID, "1.5", taught.teach_rollout, 2, agent_share=1.5)
    taught.rollout(2)
    refused(_ffi.E_STATE, "plain", taught.train_teach_rollout)
    for k in ("teacher_actions", "label_lo", "label_w"):
        refused(_ffi.E_STATE, k, taught.read_rollout, k)
    s, win, lo, w, tgt, wt = _labelled(K, 4, 5, 0)
    bad = lo.copy(); bad[3, 1] = K - 1
    refused(_ffi.E_INVALID, "label_lo %d" % (K - 1), net.teach, s, win, bad, w, tgt)
    bad = w.copy(); bad[2, 0] = 1.5
    refused(_ffi.E_INVALID, "label_w 1.5", net.teach, s, win, lo, bad, tgt)
    net.close(); eng.close(); taught.close(); eng2.close()
