"""GPU: the flat PAAC policy under the TRUE history window (grl_fnet_set_true_window / grl_fnet_read_windows of
include/goldsrl_flatwindow.h; csrc/net_flat_window.inc).

The window of every sample is held to tests/_flat_windows.replay (the numpy restatement, itself held to the A3C oracle and to
SolowPolicyMonitor's window list by tests/test_flat_windows.py) bit for bit; the forward to the explicit-window path
(grl_fnet_predict) and to the float64 oracle; the two forms of the rollout to each other bit for bit at every group size; the
gradient to grl_fnet_train on the dense windows and to the float64 oracle; the evaluation to a twin handle's rollout bit for bit
up to each env's first done.  Scenarios (tests/_flat_windows.SCENARIOS, shapes of tests/_async_scenarios.py: E = 200, three waves
and a partial one): every window length occurs, windows slide, rows cross rollout boundaries, episodes end on a rollout's last
step (the conditions are asserted on the CPU by tests/test_flat_windows.py)."""

import numpy as np
import pytest

import _async_scenarios as SC
import _flat_oracle as FO
import _flat_windows as FW
from oracle import nets as NN
from oracle import oracle as O

pytestmark = pytest.mark.gpu
SEED, OFF = SC.GEN_SEED, SC.GEN_OFFSET
E = SC.E
C0 = 1000
CASES = FW.SCENARIOS
PSEED = {"solow": 3, "trade3": 4, "trade16": 3, "solow_short": 3}      # default_init_flat seeds, as tests/test_gpu_flat_eval.py
GROUPS = (16, 32, 64)
RO_FIELDS = ("states", "actions", "values", "rewards", "masks", "nhist", "y", "adv", "boot")
# per-block gradient bound against the float64 oracle: GRAD_TOL of tests/test_gpu_flatnet_oracle.py, per env kind
GRAD_TOL = {"solow": 1e-3, "trade": 3e-4}


def _sizes(case):
    c = CASES[case]
    if c["kind"] == "solow":
        return dict(static_size=2, temporal_size=2, num_actions=1)
    S = 1 + 2 * c["n"]
    return dict(static_size=S, temporal_size=S, num_actions=c["n"])


def _flat_params(case):
    from goldsrl import _ffi_flat
    return _ffi_flat.default_init_flat(PSEED[case], **_sizes(case))


def _pair(case, monkeypatch, true_window=True, group=None, mode="persistent", n_env=E, max_samples=None, cap=None):
    """A reset engine of the scenario with its net: Solow with the staggered TimeLimit, TradeAR1 close to depletion."""
    from goldsrl import _ffi, _ffi_flat
    c = CASES[case]
    cap = c["cap"] if cap is None else cap
    if mode == "graph":
        monkeypatch.setenv("GRL_FLAT_ROLLOUT", "graph")
    else:
        monkeypatch.delenv("GRL_FLAT_ROLLOUT", raising=False)
    if group is None:
        monkeypatch.delenv("GRL_FLAT_GROUP", raising=False)
    else:
        monkeypatch.setenv("GRL_FLAT_GROUP", str(group))
    if c["kind"] == "solow":
        eng = _ffi.Engine(_ffi.ENV_SOLOW, n_env, seed=SEED, env_id_offset=OFF, rnn_length=c["R"], max_episode_steps=cap, solow_tape_len=64)
    else:
        eng = _ffi.Engine(_ffi.ENV_TRADE, n_env, seed=SEED, env_id_offset=OFF, n_assets=c["n"], rnn_length=c["R"], max_episode_steps=cap,
                          **SC.TRADE_POLICY_DEPLETION[c["n"]])
    eng.reset()
    if c["kind"] == "solow":
        eng.set_state("ELAPSED", SC.staggered_elapsed(E, cap)[:n_env])
    net = _ffi_flat.FlatNet(eng, rnn_length=c["R"], scale=100.0, max_samples=max_samples or max(c["T"], 1) * n_env, **_sizes(case))
    net.set_params(_flat_params(case))
    net.set_action_counter(C0)
    if true_window:
        net.set_true_window(True)
    return eng, net


def _close(*pairs):
    for eng, net in pairs:
        net.close(); eng.close()


def _read_rollout(net, steps):
    n_env, A, S0 = net.eng.E, net.cfg.num_actions, net.cfg.static_size
    shapes = {"states": (steps, n_env, S0), "actions": (steps, n_env, A), "boot": (n_env,)}
    out = {k: net.read_rollout(k, shapes.get(k, (steps, n_env))) for k in RO_FIELDS}
    out["nhist"] = out["nhist"].view(np.int32)
    return out


def _env_state(eng, case):
    fields = ("SOLOW_K", "SOLOW_Z", "SOLOW_E", "ELAPSED", "EPISODE", "NHIST") if CASES[case]["kind"] == "solow" else \
        ("TRADE_CASH", "TRADE_ASSETS", "TRADE_QUANTITY", "TRADE_PRICES", "ELAPSED", "EPISODE", "NHIST")
    out = {k: eng.get_state(k) for k in fields}
    out["obs"] = eng.read("obs")
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def _run_chain(case, monkeypatch, reset_idx=SC.RESET_IDX, predict=False, **kw):
    """The scenario's rollouts in a row on one handle (the host resets reset_idx between the first two): per rollout the buffers,
    the windows of every sample and (predict) grl_fnet_predict of the recorded states on those windows; the env state at the end."""
    c = CASES[case]
    eng, net = _pair(case, monkeypatch, **kw)
    T, parts = c["T"], []
    for i in range(c["rollouts"]):
        if i == 1 and reset_idx is not None:
            eng.reset(reset_idx)
        net.rollout(T); eng.wait()
        ro = _read_rollout(net, T)
        ro["windows"] = net.read_windows().reshape(T, E, c["R"], net.cfg.temporal_size)
        if predict:
            ro["predict"] = net.predict(ro["states"].reshape(T * E, -1), ro["windows"].reshape(T * E, c["R"], -1))
        parts.append(ro)
    state = _env_state(eng, case)
    counter = net.get_action_counter()
    _close((eng, net))
    return dict(parts=parts, state=state, counter=counter)


_chains = {}


def _chain(case, monkeypatch):
    """The chain at the default group in the persistent form, computed once per scenario and left unchanged."""
    if case not in _chains:
        _chains[case] = _run_chain(case, monkeypatch, predict=True)
    return _chains[case]


def _expected_windows(case, parts, reset_idx=SC.RESET_IDX):
    return FW.replay_chain([p["states"] for p in parts], [p["masks"] == 0 for p in parts], CASES[case]["R"],
                           reset_between=[reset_idx] if reset_idx is not None else ())


def _assert_windows(case, parts, reset_idx=SC.RESET_IDX, label=""):
    for i, (p, (win, length)) in enumerate(zip(parts, _expected_windows(case, parts, reset_idx))):
        assert np.array_equal(p["nhist"], length), (case, label, i)
        assert np.array_equal(_bits(p["windows"]), _bits(win)), (case, label, i)


def _action_noise(steps, A, counter0):
    k = np.arange(A)
    env = (np.arange(E) + OFF)[None, :, None]
    e0, e1 = O.normal_pair(O.rng_block(SEED, env, (counter0 + np.arange(steps))[:, None, None], 17, (k // 2)[None, None, :]))
    return np.where((k % 2 == 0)[None, None, :], e0, e1)


# ------------------------------------------------------------------------------------------ 1. the windows
@pytest.mark.parametrize("case", sorted(CASES))
def test_windows_are_the_true_last_states_of_the_episode(case, monkeypatch):
    c = CASES[case]
    parts = _chain(case, monkeypatch)["parts"]
    _assert_windows(case, parts)
    lengths = np.concatenate([p["nhist"] for p in parts])
    assert set(np.unique(lengths).tolist()) == set(range(1, min(c["R"], c["cap"]) + 1))      # every length occurs
    assert (parts[0]["nhist"][0] == 1).all()                                        # first call after the switch
    assert (parts[1]["nhist"][0, SC.RESET_IDX] == 1).all()                          # envs the host reset in between
    assert (parts[1]["nhist"][0] > 1).any()                                         # rows carried over the boundary
    assert any((p["masks"][-1] == 0).any() for p in parts)                          # a done on the last step of a rollout
    # the rows are states of the same env's same episode, oldest first, the current state last
    for p in parts:
        L = p["nhist"]
        t, e = np.nonzero(L > 0)
        assert np.array_equal(p["windows"][t, e, L[t, e] - 1], p["states"][t, e])


def test_read_windows_ranges_and_errors(monkeypatch):
    from goldsrl import _ffi
    eng, net = _pair("solow", monkeypatch)
    buf = np.empty((4, 5, 2), np.float32)
    assert net.lib.grl_fnet_read_windows(net.n, 0, 4, _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE      # before a rollout
    T = CASES["solow"]["T"]
    net.rollout(T); eng.wait()
    whole = net.read_windows()
    assert whole.shape == (T * E, 5, 2)
    assert np.array_equal(net.read_windows(E + 7, 300), whole[E + 7:E + 307])
    assert net.lib.grl_fnet_read_windows(net.n, T * E - 3, 4, _ffi._ptr(buf), buf.nbytes) == _ffi.E_SIZE
    assert net.lib.grl_fnet_read_windows(net.n, 0, 4, _ffi._ptr(buf), buf.nbytes - 4) == _ffi.E_SIZE
    assert net.lib.grl_fnet_read_windows(net.n, -1, 4, _ffi._ptr(buf), buf.nbytes) == _ffi.E_SIZE
    # Solow's "histories" are the same dense windows
    assert np.array_equal(net.read_rollout("histories", (T, E, 5, 2)).reshape(T * E, 5, 2), whole)
    # the window the next rollout's first step would see
    pred = net.predict_env()
    net.rollout(T); eng.wait()
    assert np.array_equal(_bits(net.read_rollout("values", (T, E))[0]), _bits(pred["vs"]))
    _close((eng, net))


# ------------------------------------------------------------------------------------------ 2. the forward, teacher-forced
@pytest.mark.parametrize("case", sorted(CASES))
def test_forward_over_the_true_windows(case, monkeypatch):
    c = CASES[case]
    sz = _sizes(case)
    S0, A, T = sz["static_size"], sz["num_actions"], c["T"]
    p = NN.unflatten_params(_flat_params(case).astype(np.float64), NN.flat_param_shapes(S0, S0, 32, 32, A))
    for i, ro in enumerate(_chain(case, monkeypatch)["parts"]):
        N = T * E
        pred = ro["predict"]
        err_v = np.abs(pred["vs"] - ro["values"].reshape(N)).max()
        # a. the explicit-window path on the recorded (state, window) pairs gives the rollout's values: the bound
        #    test_trade_paac_rollout_gru_policy holds the same comparison to
        np.testing.assert_allclose(pred["vs"], ro["values"].reshape(N), rtol=1e-6, atol=1e-5)
        # b. the float64 oracle on the same pairs, the suite's forward tolerances
        mu, sigma, vs = NN.flat_forward(p, ro["states"].reshape(N, S0).astype(np.float64),
                                        ro["windows"].reshape(N, c["R"], S0).astype(np.float64), 100.0)
        np.testing.assert_allclose(ro["values"].reshape(N), vs, rtol=2e-5, atol=2e-4)
        np.testing.assert_allclose(pred["mu"], mu, rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(pred["sigma"], sigma, rtol=2e-5, atol=2e-6)
        # c. the recorded raw actions are mu + sigma * eps with the rollout's stream: counters C0 + (steps so far) + t
        eps = _action_noise(T, A, C0 + i * T).reshape(N, A)
        want = (pred["mu"].astype(np.float64) + pred["sigma"].astype(np.float64) * eps).astype(np.float32)
        err_a = np.abs(ro["actions"].reshape(N, A) - want).max()
        print("%s rollout %d: max |dvalue| %.3g, max |daction| %.3g" % (case, i, err_v, err_a))
        np.testing.assert_allclose(ro["actions"].reshape(N, A), want, rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------ 3. persistent == graph
@pytest.mark.parametrize("case", sorted(CASES))
def test_persistent_and_graph_forms_give_the_same_bits(case, monkeypatch):
    ref = _chain(case, monkeypatch)
    runs = [("graph", None, _run_chain(case, monkeypatch, mode="graph"))]
    runs += [("persistent", g, _run_chain(case, monkeypatch, group=g)) for g in GROUPS]
    for mode, g, got in runs:
        assert got["counter"] == ref["counter"] == C0 + CASES[case]["T"] * CASES[case]["rollouts"]
        for i, (a, b) in enumerate(zip(got["parts"], ref["parts"])):
            for k in RO_FIELDS + ("windows",):
                assert np.array_equal(_bits(a[k]), _bits(b[k])), (case, mode, g, i, k)
        for k, v in ref["state"].items():
            assert np.array_equal(_bits(got["state"][k]), _bits(v)), (case, mode, g, k)


# ------------------------------------------------------------------------------------------ 4. the gradient
@pytest.mark.parametrize("case", ["solow", "trade3", "trade16"])
def test_gradient_over_the_strided_windows(case, monkeypatch):
    """grl_fnet_train_rollout_grads in true mode: the general forward and backward over the strided views of the state slab.
    Largest block error against the float64 oracle measured on the MI355X (E = 200, T = 20, the second rollout): solow 2.7e-4
    (sig2_b; bound 1e-3), trade3 5.2e-6 (sig1_b; bound 3e-4), trade16 4.9e-6 (mu1_w; bound 3e-4).  One 64-sample group left out
    or counted twice moved some block by 3.7e-2 or more in every scenario."""
    c = CASES[case]
    sz = _sizes(case)
    S0, A, T, R = sz["static_size"], sz["num_actions"], c["T"], c["R"]
    N = T * E
    eng, net = _pair(case, monkeypatch)
    net.rollout(T); eng.wait()      # the second rollout is the one trained on: windows carried over the boundary
    net.rollout(T); eng.wait()
    ro = _read_rollout(net, T)
    win = net.read_windows()
    stats = net.train_rollout_grads()
    grads = net.get_grads()
    f = lambda k, *s: ro[k].reshape((N,) + s)      # noqa: E731
    # a. grl_fnet_train on the dense host windows of the same samples: the bound of
    #    test_fast_forward_form_equals_the_layer_by_layer_form
    twin = _pair(case, monkeypatch, true_window=False)
    dense = twin[1].train(f("states", S0), win, f("actions", A), f("adv"), f("y"), 0.0, apply_update=False)
    gd = twin[1].get_grads()
    _close(twin)
    np.testing.assert_allclose(grads, gd, rtol=1e-4, atol=1e-6 * np.abs(gd).max())
    for k in ("loss", "policy_loss", "critic_loss_mean"):
        np.testing.assert_allclose(stats[k], dense[k], rtol=1e-5, atol=1e-7)
    # b. the float64 oracle on the dense windows; one 64-sample group left out or counted twice must exceed the bound
    shapes = NN.flat_param_shapes(S0, S0, 32, 32, A)
    p = NN.unflatten_params(_flat_params(case).astype(np.float64), shapes)
    w = FO.dense_windows(win)
    args = (p, f("states", S0), w, f("actions", A), f("adv"), f("y"))
    loss, pl, cl, g, _ = FO.loss_and_grads(*args, 100.0)
    groups = (N + 63) // 64
    sens = FO.sensitivity(g, FO.altered(g, {"last group left out": (-1.0, FO.group_contribution(*args, groups - 1, 100.0)),
                                            "group 0 twice": (1.0, FO.group_contribution(*args, 0, 100.0))}))
    err = FO.block_errors(NN.unflatten_params(grads.astype(np.float64), shapes), g)
    worst = max(err, key=err.get)
    tol = GRAD_TOL[c["kind"]]
    print("%s: largest block error %.3g (%s), tolerance %.3g, altered %s" % (case, err[worst], worst, tol, sens))
    np.testing.assert_allclose([stats["loss"], stats["policy_loss"], stats["critic_loss_mean"]], [loss, pl, cl], rtol=1e-4, atol=1e-6)
    for label, (e, k) in sens.items():
        assert e > tol, (label, e, k)
    for k in g:                                                                     # no block is left out
        assert err[k] < tol, (k, err[k])
    # c. one update with Adam, then another rollout: the parameters moved and the windows are still right
    before = net.get_params()
    net.train_rollout(1e-3)
    assert np.abs(net.get_params() - before).max() > 0
    net.rollout(T); eng.wait()
    nxt = _read_rollout(net, T)
    nxt["windows"] = net.read_windows().reshape(T, E, R, S0)
    ro["windows"] = win.reshape(T, E, R, S0)
    _close((eng, net))
    got = FW.replay_chain([ro["states"], nxt["states"]], [ro["masks"] == 0, nxt["masks"] == 0], R)
    # the trained-on rollout began with carried rows the replay of two rollouts does not know: compare the later one where its
    # windows lie inside what was replayed -- every window whose episode began in the trained-on rollout, and all lengths
    assert (ro["nhist"][0] > 1).any()
    started = np.cumsum(ro["masks"] == 0, axis=0)[-1] > 0                           # the env was reset during the trained-on rollout
    assert started.any()
    assert np.array_equal(_bits(nxt["windows"][:, started]), _bits(got[1][0][:, started]))
    assert np.array_equal(nxt["nhist"][:, started], got[1][1][:, started])


# ------------------------------------------------------------------------------------------ 5. the evaluation
SAME = (("states", "states"), ("raw", "actions"), ("values", "values"), ("rewards", "rewards"), ("nhist", "nhist"))


def _assert_asynchronous(case, ro):
    """The conditions of tests/test_gpu_async_dones.py on the rollout yardstick, as tests/test_gpu_flat_eval.py holds them."""
    c = CASES[case]
    dones = ro["masks"] == 0
    share = SC.mixed_share(dones)
    print("%s: rollout mixed share %.2f, dones %d" % (case, share, int(dones.sum())))
    assert share >= 0.25
    if c["kind"] == "trade":
        el = np.zeros(dones.shape[1], np.int64)
        dep = 0
        for t in range(dones.shape[0]):
            el += 1
            dep += int((dones[t] & (el < c["cap"])).sum())
            el[dones[t]] = 0
        print("%s: depletion dones %d" % (case, dep))
        assert dep >= E // 4


def _assert_eval_is_rollout(ev, ro, steps, label):
    dones = (ro["masks"][:steps] == 0)
    assert dones.any(axis=0).all()
    n = dones.argmax(axis=0) + 1
    assert np.array_equal(ev["length"], n), label
    assert (ev["finished"] == 1).all(), label
    S = ev["rewards"].shape[0]
    assert S == int(n.max()) <= steps
    live = np.arange(S)[:, None] < n[None]
    for k, rk in SAME:
        assert np.array_equal(_bits(ev[k])[live], _bits(ro[rk][:S])[live]), (label, k)
    assert np.array_equal(ev["dones"][live] > 0, dones[:S][live]), label
    total = np.zeros(E)
    for t in range(S):
        total = np.where(live[t], total + ro["rewards"][t].astype(np.float64), total)
    assert np.array_equal(ev["total_reward"], total), label
    return live


@pytest.mark.parametrize("greedy", [False, True])
@pytest.mark.parametrize("case", ["solow", "trade3", "trade16"])
def test_eval_is_the_rollout_up_to_each_first_done(case, greedy, monkeypatch):
    c = CASES[case]
    steps = c["cap"] + 2
    a = _pair(case, monkeypatch, max_samples=steps * E)
    a[1].set_greedy(greedy)
    a[1].rollout(steps); a[0].wait()
    ro = _read_rollout(a[1], steps)
    _close(a)
    _assert_asynchronous(case, ro)
    for group in (None,) + GROUPS:
        b = _pair(case, monkeypatch, max_samples=E * c["T"], group=group)
        ev = b[1].eval(steps, trace_steps=steps, greedy=greedy)
        assert b[1].get_action_counter() == (C0 if greedy else C0 + steps)
        if group is None:
            # the evaluation reset the handle: the next rollout's first windows are the reset observation alone
            b[1].rollout(2); b[0].wait()
            nh = b[1].read_rollout("nhist", (2, E)).view(np.int32)
            assert (nh[0] == 1).all() and nh[1].max() == min(2, c["R"])
        _close(b)
        live = _assert_eval_is_rollout(ev, ro, steps, "%s G=%s greedy=%s" % (case, group, greedy))
        assert np.array_equal(_bits(ev["raw"])[live], _bits(ev["mu"])[live]) == bool(greedy)


def test_device_monitor_under_the_true_window(monkeypatch):
    """DeviceSolowPolicyMonitor(true_window=True), greedy: the mu it traces for env 0 against grl_fnet_predict over the true windows
    of its own traced states, at the tolerance of the teacher-forced forward."""
    from goldsrl import _ffi
    from goldsrl.agents.paac.policy_monitor import DeviceSolowPolicyMonitor
    for v in ("GRL_FLAT_ROLLOUT", "GRL_FLAT_GROUP"):
        monkeypatch.delenv(v, raising=False)
    conf = dict(num_actions=1, clip_norm=40.0, clip_norm_type="global", device="cuda:0", scale=100.0, static_size=2, temporal_size=2,
                entropy_regularisation_strength=0.0, static_hidden_size=32, rnn_hidden_size=32)

    class Learner(object):
        def get_flat_params(self):
            return _flat_params("solow")
    steps, R = 12, 5
    mon = DeviceSolowPolicyMonitor("Solow-1-1-finite-eval-v0", Learner(), network_conf=conf, n_envs=3, rnn_length=R, max_episode_steps=steps,
                                   true_window=True)
    total, length, rewards = mon.eval_once(greedy=True)
    assert length == steps and len(rewards) == steps
    net = mon.net

    def trace(k, tail, dtype=np.float32):
        a = np.empty((steps, 3) + tail, dtype)
        net._check(net.lib.grl_fnet_read_eval(net.n, k.encode(), _ffi._ptr(a), a.nbytes))
        return a
    states, mu, nh = trace("states", (2,)), trace("mu", (1,)), trace("nhist", (), np.int32)
    assert nh[:, 0].tolist() == [min(t + 1, R) for t in range(steps)]
    win, wl, _ = FW.replay(states[:, :1], np.arange(steps)[:, None] == steps - 1, R)
    # the monitor's net takes n_envs samples per call
    pred = np.concatenate([net.predict(states[i:i + 3, 0], win[i:i + 3, 0])["mu"] for i in range(0, steps, 3)])
    mon.close()
    np.testing.assert_allclose(mu[:, 0], pred, rtol=1e-6, atol=1e-5)


# ------------------------------------------------------------------------------------------ 6. the switch is inert when off
@pytest.mark.parametrize("case", ["solow", "trade16"])
def test_the_switch_is_inert_when_off(case, monkeypatch):
    c = CASES[case]
    T = c["T"]
    out = []
    for toggled in (False, True):
        eng, net = _pair(case, monkeypatch, true_window=False)
        if toggled:
            net.set_true_window(True); net.set_true_window(False)
        net.rollout(T); eng.wait()
        ro = _read_rollout(net, T)
        net.train_rollout_grads()
        ro["grads"] = net.get_grads()
        eng.reset()
        if c["kind"] == "solow":
            eng.set_state("ELAPSED", SC.staggered_elapsed(E, c["cap"]))
        ev = net.eval(c["cap"] + 2, trace_steps=c["cap"] + 2)
        ro.update({"ev_" + k: v for k, v in ev.items()})
        _close((eng, net))
        out.append(ro)
    for k in out[0]:
        assert np.array_equal(_bits(out[0][k]), _bits(out[1][k])), (case, k)
    # the quirk windows: min(max(nhist, 1), rnn) copies of the state -- not what the true mode records
    assert not np.array_equal(out[0]["nhist"], _chain(case, monkeypatch)["parts"][0]["nhist"])


def test_static_and_temporal_sizes_must_agree(monkeypatch):
    from goldsrl import _ffi, _ffi_flat
    eng = _ffi.Engine(_ffi.ENV_SOLOW, 8, seed=1)
    eng.reset()
    net = _ffi_flat.FlatNet(eng, static_size=3, temporal_size=2, rnn_length=5, max_samples=64)
    assert net.lib.grl_fnet_set_true_window(net.n, 1) == _ffi.E_INVALID
    assert net.lib.grl_fnet_set_true_window(net.n, 0) == _ffi.E_INVALID
    _close((eng, net))


@pytest.mark.parametrize("case", ["solow", "trade16"])
def test_keep_activations_is_accepted_and_ignored(case, monkeypatch):
    T = CASES[case]["T"]
    out = []
    for keep in (False, True):
        eng, net = _pair(case, monkeypatch)
        net.set_keep_activations(keep)
        for _ in range(2):
            net.rollout(T); eng.wait()
            stats = net.train_rollout(1e-3)
        out.append((net.get_params(), net.get_grads(), _read_rollout(net, T), stats))
        _close((eng, net))
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(_bits(out[0][1]), _bits(out[1][1]))
    for k in RO_FIELDS:
        assert np.array_equal(_bits(out[0][2][k]), _bits(out[1][2][k])), (case, k)
    assert out[0][3]["global_norm"] == out[1][3]["global_norm"]
