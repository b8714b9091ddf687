"""GPU: greedy evaluation of the A3C discrete savings-grid agent (grl_dnet_eval / grl_dnet_read_eval of
include/goldsrl_discreteeval.h; csrc/net_discrete_eval.inc).

The yardstick of the one-launch evaluation is the per-step path with greedy on: both call the same device functions, so a twin
handle's greedy rollout must give the evaluation's bits up to every env's first done.  max_episode_steps 24 and max_steps 32: every
episode ends inside the launch; the envs start at staggered elapsed counts, so the episodes of a wave end on different steps."""
import numpy as np
import pytest

import _grid_oracle as D
from test_gpu_discretenet import _params

pytestmark = pytest.mark.gpu
CAP, MAX_STEPS, R, K = 24, 32, 5, 51
TRACE = ("states", "choices", "actions", "rewards", "dones")


def _elapsed(E):
    return ((np.arange(E) * 7) % CAP).astype(np.int32)          # lengths CAP - elapsed: 1 .. CAP, mixed inside a wave


def _pair(E, stagger=True, **kw):
    from goldsrl import _ffi, _ffi_discrete
    eng = _ffi.Engine(_ffi.ENV_SOLOW, E, seed=1692, flags=_ffi.F_RESEED_EACH_RESET, max_episode_steps=CAP, **kw)
    eng.reset()
    if stagger:
        eng.set_state("ELAPSED", _elapsed(E))
    net = _ffi_discrete.DiscreteNet(eng, rnn_length=R, num_choices=K, max_samples=1)
    net.set_params(_params(K, 5))
    return eng, net


def _close(*pairs):
    for eng, net in pairs:
        net.close(); eng.close()


@pytest.mark.parametrize("E", [1, 65, 130])
def test_eval_is_the_greedy_rollout_bit_for_bit(E):
    pair = _pair(E)
    ev = pair[1].eval(MAX_STEPS, trace_steps=MAX_STEPS)
    assert (pair[0].get_state("ELAPSED") == 0).all()               # the engine is reset afterwards
    assert pair[1].get_action_counter() == 0
    twin = _pair(E)
    twin[1].set_greedy(True)
    twin[1].rollout(CAP)
    ro = {k: twin[1].read_rollout(k) for k in TRACE}
    _close(pair, twin)
    d = ro["dones"] > 0
    assert d.any(axis=0).all()
    n = d.argmax(axis=0) + 1
    assert np.array_equal(n, CAP - _elapsed(E)) and np.array_equal(ev["length"], n) and (ev["finished"] == 1).all()
    S = ev["rewards"].shape[0]
    assert S == int(n.max()) and ev["choices"].dtype == np.int32
    for e in range(E):
        ne = int(n[e])
        total = 0.0
        for v in ro["rewards"][:ne, e]:
            total += float(v)                                          # total_reward += reward, float64
        assert ev["total_reward"][e] == total, e
        for k in TRACE:
            np.testing.assert_array_equal(ev[k][:ne, e], ro[k][:ne, e], err_msg="%s env %d" % (k, e))
    if E > 1:
        assert len(np.unique(ev["choices"])) >= 2
    live = np.arange(S)[:, None] < n[None]                         # past an env's end the trace is undefined
    assert np.array_equal(ev["actions"][live], D.grid(K)[ev["choices"][live]].astype(np.float32))


def test_eval_max_steps_and_errors():
    from goldsrl import _ffi
    eng, net = _pair(70, stagger=False)
    buf = np.zeros(70, np.float64)
    assert net.lib.grl_dnet_read_eval(net.n, b"total_reward", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE
    ev = net.eval(7, trace_steps=20)                                   # max_steps cuts the episodes; the trace is cut to the steps played
    assert (ev["length"] == 7).all() and (ev["finished"] == 0).all() and ev["rewards"].shape == (7, 70) and not ev["dones"].any()
    total = np.zeros(70)
    for t in range(7):
        total += ev["rewards"][t].astype(np.float64)
    assert np.array_equal(ev["total_reward"], total)
    for bad in (0, -3):
        with pytest.raises(_ffi.GrlError) as ei:
            net.eval(bad)
        assert ei.value.code == _ffi.E_INVALID
    _close((eng, net))


def test_grid_policy_monitor_returns_the_evaluations_totals():
    from goldsrl.agents.a3c.policy_monitor import GridPolicyMonitor
    E = 65
    params = _params(K, 5)
    pair = _pair(E, stagger=False)
    ev = pair[1].eval(MAX_STEPS, trace_steps=MAX_STEPS)
    _close(pair)
    mon = GridPolicyMonitor("Solow-1-1-finite-eval-v0", n_envs=E, n_grid=K, max_seq_length=R, max_episode_steps=CAP)
    total, length, rewards = mon.eval_once(params, max_sequence_length=R)
    assert np.array_equal(mon.total_rewards, ev["total_reward"]) and np.array_equal(mon.episode_lengths, ev["length"])
    assert total == ev["total_reward"][0] and length == CAP and rewards == [float(v) for v in ev["rewards"][:, 0]]
    assert mon.log["n_envs"] == E and mon.log["mean_total_reward"] == [float(ev["total_reward"].mean())]
    with pytest.raises(ValueError):
        mon.eval_once(params, max_sequence_length=R + 1)
    mon.close()
    with pytest.raises(ValueError):
        GridPolicyMonitor("TradeAR1-v0", n_envs=2)
