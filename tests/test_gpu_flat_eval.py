"""GPU: greedy acting and the one-launch evaluation of the flat PAAC policy (grl_fnet_set_greedy, grl_fnet_eval / grl_fnet_read_eval
of include/goldsrl_flateval.h; csrc/net_flat_eval.inc).

The yardstick of the evaluation is the per-step rollout on a twin handle (same seed, offset, parameters and action counter): both
call the same device functions, so the rollout must give the evaluation's bits up to every env's first done.  The scenarios end
their episodes on steps that differ from env to env inside a wave (tests/_async_scenarios.py): a staggered TimeLimit for Solow,
depletion for TradeAR1 with 3 assets (an odd count: one price wave has a lone asset) and 16 (all eight price waves).  Against the
float64 oracles the evaluation is held teacher-forced with the suite's tolerances (2e-5 relative for the forward, 1e-5 for the env
steps)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import _async_scenarios as SC
import _flat_cases as FC
import _flat_oracle as FO
from _flat_cases import C0, CASES, E, LOSS_SUMS, OFF, RO_FIELDS, SEED, T
from oracle import nets as NN
from oracle import oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GROUPS = (16, 32, 64)
# evaluation trace field -> rollout buffer it must equal bit for bit (dones against 1 - masks)
SAME = (("states", "states"), ("raw", "actions"), ("values", "values"), ("rewards", "rewards"), ("nhist", "nhist"))
# the scenarios' engines, nets and parameter seeds live in tests/_flat_cases.py (shared with tests/test_gpu_flat_fallbacks.py)
_sizes, _flat_params, _pair, _close, _read_rollout, _bits = FC.sizes, FC.flat_params, FC.pair, FC.close, FC.read_rollout, FC.bits


def _first_done(dones):
    """n (E,): index of each env's first done + 1; every env must have one"""
    d = dones > 0
    assert d.any(axis=0).all()
    return d.argmax(axis=0) + 1


def _assert_asynchronous(case, ro, steps=T):
    """The conditions of tests/test_gpu_async_dones.py, on the rollout yardstick alone."""
    dones = (1.0 - ro["masks"][:steps]) > 0
    share = SC.mixed_share(dones)
    print("%s: rollout mixed share %.2f, dones %d" % (case, share, int(dones.sum())))
    assert share >= 0.25
    c = CASES[case]
    if c["kind"] == "trade":
        kw = SC.TRADE_POLICY_DEPLETION[c["n"]]
        # a done before the TimeLimit counter (started at 0 after reset(), restarted behind every done) reaches the cap is a depletion
        el = np.zeros(dones.shape[1], np.int64)
        dep = 0
        for t in range(steps):
            el += 1
            dep += int((dones[t] & (el < c["cap"])).sum())
            el[dones[t]] = 0
        print("%s: depletion dones %d (start %.2f)" % (case, dep, kw["trade_starting_balance"]))
        assert dep >= E // 4


def _assert_eval_is_rollout(ev, ro, steps, label=""):
    """For every env, up to and including its first done: the traced fields equal the rollout's as bits; length, total, finished."""
    dones = 1.0 - ro["masks"][:steps]
    n = _first_done(dones)
    assert np.array_equal(ev["length"], n), label
    assert (ev["finished"] == 1).all(), label
    S = ev["rewards"].shape[0]
    assert S == int(n.max()) <= steps
    live = np.arange(S)[:, None] < n[None]
    for k, rk in SAME:
        assert np.array_equal(_bits(ev[k])[live], _bits(ro[rk][:S])[live]), (label, k)
    assert np.array_equal(_bits(ev["dones"])[live], _bits(dones[:S].astype(np.float32))[live]), label
    total = np.zeros(ev["length"].shape[0])
    for t in range(S):
        total = np.where(live[t], total + ro["rewards"][t].astype(np.float64), total)      # total += reward, float64, step order
    assert np.array_equal(ev["total_reward"], total), label
    return live


_yardsticks = {}


def _yardstick(case, monkeypatch):
    """The stochastic rollout(T) of the scenario from counter C0, computed once per case and left unchanged."""
    if case not in _yardsticks:
        pair = _pair(case, monkeypatch)
        pair[1].rollout(T); pair[0].wait()
        ro = _read_rollout(pair[1], T)
        assert pair[1].get_action_counter() == C0 + T
        _close(pair)
        _assert_asynchronous(case, ro)
        _yardsticks[case] = ro
    return _yardsticks[case]


_evals = {}


def _eval(case, monkeypatch):
    """eval(T, T, greedy=0) of the scenario at the default group with everything the oracle test needs, computed once per case."""
    if case not in _evals:
        eng, net = _pair(case, monkeypatch)
        start = {}
        if CASES[case]["kind"] == "solow":
            start = {k: eng.get_state(k) for k in ("SOLOW_K", "SOLOW_Z", "SOLOW_E", "SOLOW_TAPE")}
        ev = net.eval(T, trace_steps=T)
        assert net.get_action_counter() == C0 + T
        _close((eng, net))
        _evals[case] = dict(ev=ev, start=start)
    return _evals[case]


# ------------------------------------------------------------------------------------------ 1. stochastic eval == the rollout
@pytest.mark.parametrize("case", sorted(CASES))
def test_stochastic_eval_is_the_rollout_bit_for_bit(case, monkeypatch):
    ro = _yardstick(case, monkeypatch)
    ref = _eval(case, monkeypatch)["ev"]
    live = _assert_eval_is_rollout(ref, ro, T, case)
    assert not np.array_equal(_bits(ref["raw"])[live], _bits(ref["mu"])[live])      # noise was drawn
    for group in GROUPS:                                                            # E = 200: the last group is partial at 32 and 64
        pair = _pair(case, monkeypatch, group=group)
        ev = pair[1].eval(T, trace_steps=T)
        _close(pair)
        _assert_eval_is_rollout(ev, ro, T, "%s G=%d" % (case, group))
        for k in ref:                                                               # 4: G = 16, 32 and 64 give equal bits
            a, b = _bits(ev[k]), _bits(ref[k])
            assert np.array_equal(a[live] if a.ndim >= 2 else a, b[live] if b.ndim >= 2 else b), (case, group, k)


@pytest.mark.parametrize("case", sorted(CASES))
def test_eval_over_two_chained_rollouts_the_counter_runs_on(case, monkeypatch):
    cap = 32
    a, b = _pair(case, monkeypatch, cap=cap), _pair(case, monkeypatch, cap=cap, max_samples=E)
    parts = []
    for _ in range(2):
        a[1].rollout(T); a[0].wait()
        parts.append(_read_rollout(a[1], T))
    ro = {k: np.concatenate([p[k] for p in parts]) for k in RO_FIELDS}
    ev = b[1].eval(2 * T, trace_steps=2 * T)
    assert a[1].get_action_counter() == b[1].get_action_counter() == C0 + 2 * T
    _close(a, b)
    _assert_eval_is_rollout(ev, ro, 2 * T, case)
    assert ev["length"].max() > T                                                   # some episodes reach into the second rollout


# ------------------------------------------------------------------------------------------ 2. greedy
@pytest.mark.parametrize("case", sorted(CASES))
def test_greedy_rollout_and_greedy_eval(case, monkeypatch):
    a, g = _pair(case, monkeypatch), _pair(case, monkeypatch, mode="graph")
    for _, net in (a, g):
        net.set_greedy(True)
        net.rollout(T); net.eng.wait()
        assert net.get_action_counter() == C0                                       # nothing was drawn
    ra, rg = _read_rollout(a[1], T), _read_rollout(g[1], T)
    extra = {k: (a[1].read_rollout(k, s), g[1].read_rollout(k, s)) for k, s in (("y", (T, E)), ("adv", (T, E)), ("boot", (E,)))}
    # greedy off again: the stochastic rollout of a handle that saw the switch equals one that never did
    sw = _pair(case, monkeypatch)
    sw[1].set_greedy(True); sw[1].set_greedy(False)
    sw[1].rollout(T); sw[0].wait()
    back = _read_rollout(sw[1], T)
    assert sw[1].get_action_counter() == C0 + T
    _close(sw)
    _close(a, g)
    for k in RO_FIELDS:
        assert np.array_equal(_bits(ra[k]), _bits(rg[k])), (case, k)
    for k, (x, y) in extra.items():
        assert np.array_equal(_bits(x), _bits(y)), (case, k)
    ro = _yardstick(case, monkeypatch)
    for k in RO_FIELDS:
        assert np.array_equal(_bits(back[k]), _bits(ro[k])), (case, k)
    assert not np.array_equal(ra["actions"], ro["actions"])
    _assert_asynchronous(case, ra)
    e = _pair(case, monkeypatch, max_samples=E)
    ev = e[1].eval(T, trace_steps=T, greedy=True)
    assert e[1].get_action_counter() == C0
    _close(e)
    live = _assert_eval_is_rollout(ev, ra, T, case)
    assert np.array_equal(_bits(ev["raw"])[live], _bits(ev["mu"])[live])
    S = ev["mu"].shape[0]
    assert np.array_equal(_bits(ra["actions"][:S])[live], _bits(ev["mu"])[live])    # "actions" reads back equal to mu


# ------------------------------------------------------------------------------------------ 3. against the float64 oracles
@pytest.mark.parametrize("case", sorted(CASES))
def test_eval_against_the_oracles_teacher_forced(case, monkeypatch):
    c = CASES[case]
    job = _eval(case, monkeypatch)
    ev = job["ev"]
    n = ev["length"]
    S = ev["rewards"].shape[0]
    live = np.arange(S)[:, None] < n[None]                                          # (S,E): the step was played
    sz = _sizes(case)
    S0, A = sz["static_size"], sz["num_actions"]
    p = NN.unflatten_params(_flat_params(case).astype(np.float64), NN.flat_param_shapes(S0, S0, 32, 32, A))
    states, nhist = ev["states"][live], ev["nhist"][live]
    win = FO.repeated_state_windows(states, nhist, c["R"])
    mu, sigma, vs = NN.flat_forward(p, states.astype(np.float64), win(0, len(states)), 100.0)
    assert len(states) == int(n.sum())                                              # no sample is left out
    np.testing.assert_allclose(ev["mu"][live], mu, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(ev["sigma"][live], sigma, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(ev["values"][live], vs, rtol=2e-5, atol=2e-4)
    # the draw and the transform: raw = mu + sigma * e in double from the action stream, then the stable sigmoid / tanh
    k = np.arange(A)
    env = (np.arange(E) + OFF)[None, :, None]
    e0, e1 = O.normal_pair(O.rng_block(SEED, env, (C0 + np.arange(S))[:, None, None], 17, (k // 2)[None, None, :]))
    eps = np.where((k % 2 == 0)[None, None, :], e0, e1)
    raw = (ev["mu"].astype(np.float64) + ev["sigma"].astype(np.float64) * eps).astype(np.float32)
    np.testing.assert_allclose(ev["raw"][live], raw[live], rtol=1e-6, atol=1e-6)
    acts = ev["actions"]
    if c["kind"] == "solow":
        np.testing.assert_allclose(acts[live], 1.0 / (1.0 + np.exp(-ev["raw"][live].astype(np.float64))), rtol=1e-6, atol=0)
        st = job["start"]
        rho_z, rho_e = O.solow_rhos(1, 1)
        kk, z, e_ = (st[f].astype(np.float64) for f in ("SOLOW_K", "SOLOW_Z", "SOLOW_E"))
        tape = st["SOLOW_TAPE"].astype(np.float64)
        TT = tape.shape[1]
        assert np.array_equal(n, c["cap"] - SC.staggered_elapsed(E))
        for t in range(S):
            a = np.where(live[t], acts[t, :, 0], 0.5).astype(np.float64)
            kk, z, e_, obs, rew = O.solow_step(kk, z, e_, tape[:, TT - 1 - t], a, rho_z, rho_e)
            np.testing.assert_allclose(ev["rewards"][t][live[t]], rew[live[t]], rtol=1e-5, atol=5e-6)
            assert np.array_equal(ev["dones"][t][live[t]] > 0, (n == t + 1)[live[t]])
            if t + 1 < S:
                nx = live[t + 1]
                np.testing.assert_allclose(ev["states"][t + 1][nx], O.solow_process_state(obs)[nx], rtol=1e-5, atol=1e-6)
    else:
        np.testing.assert_allclose(acts[live], np.tanh(ev["raw"][live].astype(np.float64)), rtol=1e-6, atol=1e-7)
        nn = c["n"]
        kw = SC.TRADE_POLICY_DEPLETION[nn]
        nrm = SC.trade_generator_normals(SEED, OFF, E, S, nn)
        start = kw["trade_starting_balance"]
        cash, assets = np.full(E, start), np.full(E, start)
        q, pr = np.zeros((E, nn)), np.ones((E, nn))
        first = O.trade_process_state(SC.trade_reset_obs(E, nn, start))
        np.testing.assert_allclose(ev["states"][0], first, rtol=1e-5, atol=1e-6)
        nh = np.zeros(E, np.int64)                                                  # the worker's window: empty after reset(), +1 per step
        for t in range(S):
            assert np.array_equal(ev["nhist"][t][live[t]], nh[live[t]])
            nh = np.minimum(nh + 1, c["R"] + 1)
            a = np.where(live[t][:, None], acts[t], 0.0).astype(np.float64)
            cash, assets, q, pr, obs, rew, done = O.trade_step(cash, assets, q, pr, a, nrm[t], O.trade_std_e(kw["trade_std_p"]))
            done = done | (t + 1 >= c["cap"])
            np.testing.assert_allclose(ev["rewards"][t][live[t]], rew[live[t]], rtol=1e-5, atol=1e-9)
            assert np.array_equal(ev["dones"][t][live[t]] > 0, done[live[t]])
            if t + 1 < S:
                nx = live[t + 1]
                np.testing.assert_allclose(ev["states"][t + 1][nx], O.trade_process_state(obs)[nx], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------ 4. the env count
@pytest.mark.parametrize("case", sorted(CASES))
def test_eval_does_not_depend_on_the_env_count(case, monkeypatch):
    ref = _eval(case, monkeypatch)["ev"]
    pair = _pair(case, monkeypatch, n_env=64)
    got = pair[1].eval(T, trace_steps=T)
    _close(pair)
    for k in ("total_reward", "length", "finished"):
        assert np.array_equal(got[k], ref[k][:64]), (case, k)
    S = got["rewards"].shape[0]
    live = np.arange(S)[:, None] < got["length"][None]
    for k in ("states", "nhist", "mu", "sigma", "raw", "actions", "values", "rewards", "dones"):
        assert np.array_equal(_bits(got[k])[live], _bits(ref[k][:S, :64])[live]), (case, k)


# ------------------------------------------------------------------------------------------ 5. max_steps
def test_eval_max_steps(monkeypatch):
    from goldsrl import _ffi
    n_env = 70
    eng, net = _pair("solow", monkeypatch, n_env=n_env, cap=0, stagger=False, solow_tape_len=2048)
    buf = np.zeros(n_env, np.float64)
    assert net.lib.grl_fnet_read_eval(net.n, b"total_reward", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE      # before any eval
    ev = net.eval(7, trace_steps=20)                                                # the trace is capped at max_steps
    assert (ev["length"] == 7).all() and (ev["finished"] == 0).all() and ev["rewards"].shape == (7, n_env)
    assert not ev["dones"].any()
    total = np.zeros(n_env)
    for t in range(7):
        total += ev["rewards"][t].astype(np.float64)
    assert np.array_equal(ev["total_reward"], total)
    assert net.lib.grl_fnet_read_eval(net.n, b"total_reward", _ffi._ptr(buf), buf.nbytes - 8) == _ffi.E_SIZE
    assert net.lib.grl_fnet_read_eval(net.n, b"windows", _ffi._ptr(buf), buf.nbytes) == _ffi.E_INVALID
    for bad in ((0, 0), (-3, 0), (5, -1)):
        with pytest.raises(_ffi.GrlError) as ei:
            net.eval(bad[0], trace_steps=bad[1])
        assert ei.value.code == _ffi.E_INVALID
    _close((eng, net))


# ------------------------------------------------------------------------------------------ 6. eval leaves the rest alone
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("case", ["solow", "trade3"])
def test_eval_leaves_training_and_the_handle_alone(case, keep, monkeypatch):
    from goldsrl import _ffi
    cap = CASES[case]["cap"]
    # Solow: reseeded at every reset, so that the reset the evaluation ends with and the twin's reset() give the same episodes
    kw = dict(flags=_ffi.F_RESEED_EACH_RESET) if case == "solow" else {}
    a, b = _pair(case, monkeypatch, **kw), _pair(case, monkeypatch, **kw)
    g = _pair(case, monkeypatch, mode="graph", **kw)
    for eng, net in (a, b, g):
        eng.episodes_enable(capacity=8 * E)
        net.rollout_stage_times()                                                   # attaches the stage clock
        net.set_keep_activations(keep)
        net.rollout(T); eng.wait()
    ev = a[1].eval(cap, trace_steps=cap)                                            # between the rollout and its update
    assert (ev["finished"] == 1).all()
    assert a[1].get_action_counter() == C0 + T + cap and b[1].get_action_counter() == C0 + T
    for k in RO_FIELDS:                                                             # the last rollout's buffers
        assert np.array_equal(_bits(_read_rollout(a[1], T)[k]), _bits(_read_rollout(b[1], T)[k])), k
    ra, rb = a[0].episodes_read(), b[0].episodes_read()
    assert len(ra) > 0 and np.array_equal(ra, rb)
    for x, y in zip(a[0].episodes_running(), b[0].episodes_running()):
        assert np.array_equal(x, y)
    sa, sb = a[1].train_rollout(1e-3), b[1].train_rollout(1e-3)
    # the statistics: global_norm comes out of a fixed-order reduction and is held bit for bit; the loss sums are float64 atomicAdds
    # over the backward's workgroups in whatever order they finish (net_flat_bwd_fast.inc), so twins differ in the last bits with
    # or without an evaluation between them -- the bound tests/test_gpu_flatnet.py holds them to
    assert sa["global_norm"] == sb["global_norm"]
    for k in LOSS_SUMS:
        np.testing.assert_allclose(sa[k], sb[k], rtol=1e-6, atol=0, err_msg=k)
    assert np.array_equal(_bits(a[1].get_params()), _bits(b[1].get_params()))
    assert np.array_equal(_bits(a[1].get_grads()), _bits(b[1].get_grads()))
    oa, ob = a[1].get_optimizer_state(), b[1].get_optimizer_state()
    assert np.array_equal(oa["adam_m"], ob["adam_m"]) and np.array_equal(oa["adam_v"], ob["adam_v"]) and oa["adam_step"] == ob["adam_step"] == 1
    # afterwards the handle reads as after reset(): a plain rollout equals the twin's that was reset() instead of evaluated, and it
    # still takes the persistent form (the stage clock of the persistent kernel, not the graph's launches)
    assert (a[0].get_state("ELAPSED") == 0).all()
    b[0].reset()
    b[1].set_action_counter(a[1].get_action_counter())
    g[1].train_rollout(1e-3)
    for eng, net in (a, b, g):
        net.rollout(T); eng.wait()
    ra, rb = _read_rollout(a[1], T), _read_rollout(b[1], T)
    for k in RO_FIELDS:
        assert np.array_equal(_bits(ra[k]), _bits(rb[k])), k
    ta, tb, tg = (len(net.rollout_stage_times()) for _, net in (a, b, g))
    assert ta == tb > 0 and ta != tg
    _close(a, b, g)


# ------------------------------------------------------------------------------------------ 7. full length
def _registration(kind, n_env, cap=1024):
    from goldsrl import _ffi, _ffi_flat
    if kind == "solow":
        eng = _ffi.Engine(_ffi.ENV_SOLOW, n_env, seed=1692, flags=_ffi.F_RESEED_EACH_RESET, rnn_length=5, max_episode_steps=cap)
        sizes, R = dict(static_size=2, temporal_size=2, num_actions=1), 5
    else:
        eng = _ffi.Engine(_ffi.ENV_TRADE, n_env, seed=1692, n_assets=16, rnn_length=20, max_episode_steps=cap)
        sizes, R = dict(static_size=33, temporal_size=33, num_actions=16), 20
    net = _ffi_flat.FlatNet(eng, rnn_length=R, scale=100.0, max_samples=n_env, **sizes)
    net.set_params(_ffi_flat.default_init_flat(3, **sizes))
    return eng, net


@pytest.mark.parametrize("kind", ["solow", "trade16"])
def test_full_length_episodes_of_the_eval_registration(kind):
    pair = _registration(kind, 64)
    runs = []
    for _ in range(2):
        pair[1].set_action_counter(0)
        pair[0].reset()
        runs.append(pair[1].eval(1024))
    _close(pair)
    a, b = runs
    assert set(a) == {"total_reward", "length", "finished"}
    assert np.array_equal(a["total_reward"], b["total_reward"]) and np.array_equal(a["length"], b["length"])
    assert np.isfinite(a["total_reward"]).all() and (a["finished"] == 1).all()
    if kind == "solow":
        assert (a["length"] == 1024).all()
    else:
        assert (a["length"] >= 1).all() and (a["length"] <= 1024).all()
    assert len(np.unique(a["total_reward"])) == 64                                  # 64 different seeded episodes


# ------------------------------------------------------------------------------------------ 8. host layer
class _Global(object):
    """What the monitor needs of the learner's estimator: its conf and its flat parameters."""

    def __init__(self):
        from goldsrl import _ffi_flat
        self.conf = {'num_actions': 1, 'entropy_regularisation_strength': 0.02, 'device': '/gpu:0', 'scale': 100.0, 'clip_norm': 40.0,
                     'clip_norm_type': 'global', 'static_size': 2, 'temporal_size': 2, 'static_hidden_size': 32, 'rnn_hidden_size': 32}
        self.flat = _ffi_flat.default_init_flat(5)

    def get_flat_params(self):
        return self.flat


class _Writer(object):
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def flush(self):
        pass


def test_env_0_of_the_device_monitor_is_the_same_episode_at_any_env_count():
    from goldsrl.agents.paac.policy_monitor import DeviceSolowPolicyMonitor
    cap = 40
    out = {}
    for n_envs in (1, 200):
        w = _Writer()
        mon = DeviceSolowPolicyMonitor("Solow-1-1-finite-eval-v0", _Global(), summary_writer=w, n_envs=n_envs, rnn_length=5,
                                       max_episode_steps=cap)
        first = mon.eval_once()
        again = mon.eval_once()                                                     # same seeded episodes, same noise
        assert first == again and mon.net.get_action_counter() == cap
        greedy = mon.eval_once(greedy=True)
        assert greedy[1] == cap and greedy[0] != first[0]
        assert mon.total_rewards.shape == (n_envs,) and (mon.episode_lengths == cap).all()
        assert [r[0] for r in w.rows[:3]] == ["eval/total_reward", "eval/episode_length", "eval/mean_total_reward"] and len(w.rows) == 9
        assert w.rows[0][1] == first[0] and w.rows[1][1] == cap
        out[n_envs] = first
        mon.close()
    total, length, rewards = out[1]
    assert length == cap and len(rewards) == cap and out[200] == out[1]
    s = 0.0
    for r in rewards:
        s += r
    assert total == s


def _run(out, extra):
    from goldsrl import utils_tfevents
    cmd = [sys.executable, "-m", "goldsrl.scripts.train_paac_solow", "-ec", "128", "--max_local_steps", "8", "--max_global_steps",
           str(3 * 8 * 128), "--max_episode_steps", "24", "-df", str(out)] + extra
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "golds-rl-gym_amd"), os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    (events,) = glob.glob(os.path.join(str(out), "events.out.tfevents.*"))
    scalars = {}
    for tag, value, step, _ in utils_tfevents.read_scalars(events):
        scalars.setdefault(tag, []).append((step, value))
    return scalars


def test_train_paac_solow_evaluates_on_the_device_only_when_asked(tmp_path):
    plain = _run(tmp_path / "plain", [])
    assert set(plain) == {"global_norm", "loss/total", "loss/policy", "loss/critic_mean", "rl/reward"}      # what it wrote before
    assert [s for s, _ in plain["global_norm"]] == [1024, 2048, 3072]
    with_eval = _run(tmp_path / "eval", ["--eval-envs", "64", "--eval-updates", "1"])
    for tag in ("eval/total_reward", "eval/episode_length", "eval/mean_total_reward"):
        assert [s for s, _ in with_eval[tag]] == [1024, 2048, 3072], tag
        assert all(np.isfinite(v) for _, v in with_eval[tag])
    assert [v for _, v in with_eval["eval/episode_length"]] == [24, 24, 24]
    # the evaluation runs on a handle and a net of its own: the training scalars are the plain run's -- tags and steps exactly,
    # values bit for bit except the loss sums (float64 atomics in completion order: rtol 1e-6, as tests/test_gpu_flatnet.py)
    rest = {k: v for k, v in with_eval.items() if not k.startswith("eval/")}
    assert set(rest) == set(plain)
    for tag in plain:
        assert [st for st, _ in rest[tag]] == [st for st, _ in plain[tag]], tag
        got, want = [v for _, v in rest[tag]], [v for _, v in plain[tag]]
        if tag.startswith("loss/"):
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=tag)
        else:
            assert got == want, tag
