"""GPU: greedy acting and greedy evaluation of the Ticker gated trader (grl_gnet_set_greedy, grl_gnet_eval / grl_gnet_read_eval of
include/goldsrl_gatedeval.h; csrc/net_gated_eval.inc, csrc/ticker_dev.h).

The yardstick of the one-launch evaluation is the per-step path with greedy on: both call the same device functions, so a twin
handle's greedy rollout must give the evaluation's bits up to every env's first done.  The scenario (tests/_gated_eval_cases.py)
ends its episodes on steps that differ from env to env inside a wave: a staggered TimeLimit, and in one test depletion.  Against
the float64 oracle the evaluation is held teacher-forced, with the tolerances of test_gpu_gatednet.py."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _async_scenarios as SC
import _gated_eval_cases as GC
import _gated_oracle as G
from oracle import ticker as TK
from test_gpu_gatednet import _params

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
E, R, CAP = GC.E, GC.R, GC.CAP
FWD_RTOL, FWD_ATOL = 2e-4, 2e-5          # test_gpu_gatednet.test_predict_matches_oracle
TRACE = ("states", "probs", "mu", "choices", "actions", "rewards", "dones")
ROLLOUT = ("states", "windows", "choices", "raw", "probs", "mu", "sigma", "values", "actions", "rewards", "dones", "weights", "adv",
           "targets", "boot")
DEPLETION_PSEED = 15                     # a policy that holds, buys and sells on both assets (the oracle gap plays no part there)


def _pair(n_env=E, cap=CAP, flags=0, stagger=True, pseed=GC.PSEED):
    """A reset engine of the scenario with its net."""
    from goldsrl import _ffi, _ffi_gated
    eng = _ffi.Engine(_ffi.ENV_TICKER, n_env, seed=GC.SEED, env_id_offset=GC.OFF, max_episode_steps=cap, flags=flags)
    eng.ticker_set_table(GC.matrix())
    eng.reset()
    if stagger:
        eng.set_state("ELAPSED", SC.staggered_elapsed(E)[:n_env])
    net = _ffi_gated.GatedNet(eng, rnn_length=R, max_samples=8192)
    net.set_params(_params(pseed))
    return eng, net


def _close(*pairs):
    for eng, net in pairs:
        net.close(); eng.close()


def _first_done(dones):
    """n (E,): index of each env's first done + 1; every env must have one"""
    d = dones > 0
    assert d.any(axis=0).all()
    return d.argmax(axis=0) + 1


def _sigmoid32(raw32):
    return (1.0 / (1.0 + np.exp(-np.asarray(raw32, np.float32).astype(np.float64)))).astype(np.float32)


def _assert_eval_is_the_rollout(ev, ro, cap):
    """the evaluation's bits are the twin's greedy rollout's up to every env's first done; returns those lengths"""
    n = _first_done(ro["dones"])
    assert np.array_equal(ev["length"], n) and (ev["finished"] == 1).all()
    assert ev["rewards"].shape[0] == min(cap, int(ev["length"].max()))
    for e in range(ev["length"].shape[0]):
        ne = int(n[e])
        assert ev["total_reward"][e] == GC.running_total(ro["rewards"][:ne, e]), e
        for k in TRACE:
            np.testing.assert_array_equal(ev[k][:ne, e], ro[k][:ne, e], err_msg="%s env %d" % (k, e))
    return n


@pytest.fixture(scope="module")
def case():
    """The evaluation of the scenario with a full trace, and the twin handle's greedy rollout over the cap."""
    eng, net = _pair()
    start = eng.get_state("TICKER_START")
    ev = net.eval(CAP, trace_steps=CAP)
    elapsed_after = eng.get_state("ELAPSED")
    twin = _pair()
    twin[1].set_greedy(True)
    twin[1].rollout(CAP)
    ro = {k: twin[1].read_rollout(k) for k in ROLLOUT}
    _close((eng, net), twin)
    return dict(ev=ev, ro=ro, start=start, elapsed_after=elapsed_after)


# ------------------------------------------------------------------------------------------ 1. greedy rollout
def test_greedy_rollout():
    T = 12
    eng, net = _pair()
    net.set_action_counter(1000)
    net.set_greedy(True)
    net.rollout(T)
    r = {k: net.read_rollout(k) for k in ROLLOUT}
    assert net.get_action_counter() == 1000                       # nothing was drawn
    assert (r["dones"] > 0).any()                                 # windows restart inside the rollout
    ch, raw, frac = GC.greedy_pick(r["probs"], r["mu"])
    assert np.array_equal(r["choices"], ch)                       # first index of the largest float32 probability
    assert np.array_equal(r["raw"].view(np.uint32), raw.view(np.uint32))
    assert np.array_equal(r["actions"][..., :2], ch.astype(np.float32))
    assert np.array_equal(r["actions"][..., 2:], _sigmoid32(r["raw"])) and np.array_equal(frac, r["actions"][..., 2:])
    got = net.predict(r["states"].reshape(-1, 7), r["windows"].reshape(-1, R, 4))
    for k in ("probs", "mu", "sigma", "values"):
        np.testing.assert_array_equal(got[k], r[k].reshape(got[k].shape), err_msg=k)
    # greedy off again: the stochastic rollout of a handle that saw the switch equals one that never did
    a, b = _pair(), _pair()
    a[1].set_greedy(True); a[1].set_greedy(False)
    for _, nt in (a, b):
        nt.rollout(T)
    for k in ROLLOUT:
        np.testing.assert_array_equal(a[1].read_rollout(k), b[1].read_rollout(k), err_msg=k)
    assert a[1].get_action_counter() == b[1].get_action_counter() == T
    assert not np.array_equal(a[1].read_rollout("raw"), GC.greedy_pick(a[1].read_rollout("probs"), a[1].read_rollout("mu"))[1])
    _close((eng, net), a, b)


# ------------------------------------------------------------------------------------------ 2. eval == the per-step path
def test_eval_is_the_greedy_rollout_bit_for_bit(case):
    ev, ro = case["ev"], case["ro"]
    n = _assert_eval_is_the_rollout(ev, ro, CAP)
    assert np.array_equal(ev["length"], CAP - SC.staggered_elapsed(E)) and ev["length"].min() == 1 and ev["length"].max() == CAP
    first = (ro["dones"] > 0) & (np.arange(CAP)[:, None] < n[None])      # the twin's dones truncated at each env's first done
    share = SC.mixed_share(first)
    print("eval: lengths %s, mixed share %.2f" % (np.unique(ev["length"]).tolist(), share))
    assert share >= 0.25
    assert (case["elapsed_after"] == 0).all()


# ------------------------------------------------------------------------------------------ 3. depletion ends
def test_eval_depletion_ends():
    sel = np.arange(E) % 5 == 2

    def deplete(pair):
        for f in ("TICKER_CASH", "TICKER_ASSETS"):
            v = pair[0].get_state(f)
            v[sel] = 0.5                                                 # below MIN_CASH with no holdings: the first step ends the env
            pair[0].set_state(f, v)
        pair[0].observe()
        return pair
    a = deplete(_pair(stagger=False, pseed=DEPLETION_PSEED))
    start = a[0].get_state("TICKER_START")
    ev = a[1].eval(CAP, trace_steps=CAP)
    twin = deplete(_pair(stagger=False, pseed=DEPLETION_PSEED))
    twin[1].set_greedy(True)
    twin[1].rollout(CAP)
    ro = {k: twin[1].read_rollout(k) for k in TRACE}
    _close(a, twin)
    assert np.array_equal(ev["length"], np.where(sel, 1, CAP))
    m = GC.matrix()
    st, _ = TK.ticker_reset(m, start)
    st["cash"][sel] = 0.5; st["assets"][sel] = 0.5
    _, rew, done = TK.ticker_step(m, st, ev["choices"][0], ev["actions"][0, :, 2:].astype(np.float64))
    assert done[sel].all() and not done[~sel].any()
    assert np.array_equal(rew.astype(np.float32)[sel], ev["rewards"][0][sel])
    assert (ev["dones"][0][sel] == 1).all()
    _assert_eval_is_the_rollout(ev, ro, CAP)


# ------------------------------------------------------------------------------------------ 4. against the oracle
def test_eval_against_the_oracle_teacher_forced(case):
    ev = case["ev"]
    n = ev["length"]
    S = ev["rewards"].shape[0]
    live = np.arange(S)[:, None] < n[None]                               # (S,E): the step was played
    dones = ev["dones"].copy(); dones[~live] = 0
    win, _ = G.replay_windows(np.where(live[..., None], ev["states"], 0).astype(np.float32), dones, R)
    p = G.unflatten(_params(GC.PSEED).astype(np.float64))
    probs, mu = G.forward(p, ev["states"][live].astype(np.float64), win[live].astype(np.float64))[:2]
    np.testing.assert_allclose(ev["probs"][live], probs, rtol=FWD_RTOL, atol=FWD_ATOL)
    np.testing.assert_allclose(ev["mu"][live], mu, rtol=FWD_RTOL, atol=FWD_ATOL)
    # the choice: the oracle's argmax wherever the oracle's top two are further apart than the margin -- here everywhere
    clear = GC.top_two_gap(probs) > GC.MARGIN
    left_out = 1.0 - clear.mean()
    print("smallest oracle top-two gap %.4g, share left out %.3g" % (GC.top_two_gap(probs).min(), left_out))
    assert left_out == 0
    assert np.array_equal(ev["choices"][live][clear], np.argmax(probs, axis=-1)[clear])
    # the env, fed the traced choices and fractions
    m = GC.matrix()
    st, obs = TK.ticker_reset(m, case["start"])
    np.testing.assert_allclose(ev["states"][0], TK.ticker_process_state(obs), rtol=3e-7, atol=1e-7)
    el0 = SC.staggered_elapsed(E)
    for t in range(S):
        ch = np.where(live[t][:, None], ev["choices"][t], 0)
        fr = np.where(live[t][:, None], ev["actions"][t, :, 2:], 0.5).astype(np.float64)
        assert np.array_equal(ev["actions"][t, :, :2][live[t]], ev["choices"][t][live[t]].astype(np.float32))
        _, rew, done = TK.ticker_step(m, st, ch, fr)
        done = done | (el0 + t + 1 >= CAP)
        np.testing.assert_array_equal(rew.astype(np.float32)[live[t]], ev["rewards"][t][live[t]])
        np.testing.assert_array_equal(done.astype(np.float32)[live[t]], ev["dones"][t][live[t]])


# ------------------------------------------------------------------------------------------ 5. group edges
def test_eval_does_not_depend_on_the_env_count(case):
    ev = case["ev"]
    for n_env in (1, 63, 64, 65):
        pair = _pair(n_env)
        got = pair[1].eval(CAP)
        _close(pair)
        assert set(got) == {"total_reward", "length", "finished"}
        assert np.array_equal(got["total_reward"], ev["total_reward"][:n_env]), n_env
        assert np.array_equal(got["length"], ev["length"][:n_env]) and (got["finished"] == 1).all()


# ------------------------------------------------------------------------------------------ 6. max_steps, errors
def test_eval_max_steps_and_errors():
    from goldsrl import _ffi
    n_env = 70
    eng, net = _pair(n_env, cap=1023, stagger=False)
    buf = np.zeros(n_env, np.float64)
    assert net.lib.grl_gnet_read_eval(net.n, b"total_reward", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE      # no evaluation yet
    ev = net.eval(7, trace_steps=20)                                     # the trace is cut to the steps played
    assert (ev["length"] == 7).all() and (ev["finished"] == 0).all() and ev["rewards"].shape == (7, n_env)
    assert not ev["dones"].any()
    total = np.zeros(n_env)
    for t in range(7):
        total += ev["rewards"][t].astype(np.float64)
    assert np.array_equal(ev["total_reward"], total)
    for bad in (0, -3):
        with pytest.raises(_ffi.GrlError) as ei:
            net.eval(bad)
        assert ei.value.code == _ffi.E_INVALID
    with pytest.raises(_ffi.GrlError) as ei:
        net.eval(7, trace_steps=-1)
    assert ei.value.code == _ffi.E_INVALID
    _close((eng, net))
    uncapped = _pair(3, cap=0, stagger=False)                            # no TimeLimit: an env could run past its price window
    with pytest.raises(_ffi.GrlError) as ei:
        uncapped[1].eval(7)
    assert ei.value.code == _ffi.E_STATE
    _close(uncapped)


# ------------------------------------------------------------------------------------------ 7. eval leaves the rest alone
def test_eval_leaves_training_and_the_handle_alone():
    from goldsrl import _ffi
    n_env = 100
    a = _pair(n_env, flags=_ffi.F_RESEED_EACH_RESET, stagger=False)
    b = _pair(n_env, flags=_ffi.F_RESEED_EACH_RESET, stagger=False)
    a[1].rollout(4); b[1].rollout(4)
    a[1].eval(CAP, trace_steps=CAP)                                      # between the rollout and its update
    assert a[1].get_action_counter() == 4
    assert (a[0].get_state("ELAPSED") == 0).all()
    sa, sb = a[1].train_rollout(lr=1e-3), b[1].train_rollout(lr=1e-3)
    assert sa == sb
    assert np.array_equal(a[1].get_params(), b[1].get_params())
    for which in ("policy", "value"):
        assert np.array_equal(a[1].get_grads(which), b[1].get_grads(which))
    oa, ob = a[1].get_optimizer_state(), b[1].get_optimizer_state()
    assert np.array_equal(oa["ms_policy"], ob["ms_policy"]) and np.array_equal(oa["ms_value"], ob["ms_value"]) and oa["global_step"] == 2
    # afterwards the handle is a reset one: a plain rollout equals the twin's that was reset() instead of evaluated
    b[0].reset()
    a[1].rollout(3); b[1].rollout(3)
    for k in ROLLOUT:
        np.testing.assert_array_equal(a[1].read_rollout(k), b[1].read_rollout(k), err_msg=k)
    assert a[1].get_action_counter() == b[1].get_action_counter() == 7
    # reset() + eval repeats: the eval registration's episodes are the same ones every time
    params = _params(GC.PSEED)
    runs = []
    for _ in range(2):
        a[1].set_params(params)
        a[0].reset()
        runs.append(a[1].eval(CAP, trace_steps=CAP))
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)
    _close(a, b)


# ------------------------------------------------------------------------------------------ 8. the eval registration
def test_env_0_of_the_eval_registration_is_the_single_episode():
    from goldsrl import _ffi_gated
    from goldsrl.agents.a3c.policy_monitor import make_ticker_eval_engine
    m, cap = GC.matrix(), 40
    got = []
    for n_env in (65, 1):
        eng = make_ticker_eval_engine(m, n_env, max_episode_steps=cap)
        eng.reset()
        assert np.array_equal(eng.get_state("TICKER_START"), SC.ticker_reset_start(1692, np.arange(n_env), np.zeros(n_env, np.int64), m.shape[0]))
        net = _ffi_gated.GatedNet(eng, rnn_length=R, max_samples=1)
        net.set_params(_params(GC.PSEED))
        got.append(net.eval(cap, trace_steps=cap))
        _close((eng, net))
    big, one = got
    assert (big["length"] == cap).all() and (big["finished"] == 1).all() and np.isfinite(big["total_reward"]).all()
    assert one["total_reward"][0] == big["total_reward"][0] and one["length"][0] == cap
    for k in TRACE:
        np.testing.assert_array_equal(one[k][:, 0], big[k][:, 0], err_msg=k)


# ------------------------------------------------------------------------------------------ 9. scripts
def _run(out, extra):
    from goldsrl import utils_tfevents
    cmd = [sys.executable, "-m", "goldsrl.scripts.train_ticker", "--table", GC.GOLD, "--envs", "128", "--steps", "8", "--updates", "2",
           "--out", str(out)] + extra
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "golds-rl-gym_amd"), os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    (events,) = glob.glob(os.path.join(str(out), "events.out.tfevents.*"))
    scalars = {}
    for tag, value, step, _ in utils_tfevents.read_scalars(events):
        scalars.setdefault(tag, []).append((step, value))
    return scalars


def test_train_ticker_evaluates_on_the_device(tmp_path):
    out = tmp_path / "run"
    scalars = _run(out, ["--eval-envs", "64", "--eval-every", "1"])
    log = json.load(open(out / "Ticker.json"))
    assert set(log) == {"total_reward", "episode_length", "mean_total_reward", "std_total_reward", "n_envs"}
    assert log["n_envs"] == 64
    for k in ("total_reward", "episode_length", "mean_total_reward", "std_total_reward"):
        assert len(log[k]) == 2 and all(np.isfinite(v) for v in log[k]), k
    assert all(1 <= v <= 1023 for v in log["episode_length"])
    assert all(v > 0 for v in log["std_total_reward"])
    for tag, key in (("eval/total_reward", "total_reward"), ("eval/episode_length", "episode_length"), ("eval/mean_total_reward", "mean_total_reward")):
        assert [s for s, _ in scalars[tag]] == [2, 4]
        np.testing.assert_allclose([v for _, v in scalars[tag]], log[key], rtol=1e-6)


def test_train_ticker_without_eval_envs_writes_what_it_wrote(tmp_path):
    out = tmp_path / "run"
    scalars = _run(out, [])
    assert not [t for t in scalars if t.startswith("eval/")]
    assert not os.path.exists(out / "Ticker.json")
    assert "train/policy_loss" in scalars and os.path.exists(out / "checkpoint.npz")
