"""GPU: greedy acting and greedy evaluation of the A3C Gaussian agent (grl_anet_set_greedy, grl_anet_eval / grl_anet_read_eval of
include/goldsrl_gaussnet.h; csrc/net_gauss_eval.inc).

The yardstick of the one-launch evaluation is the per-step path with greedy on: both call the same device functions, so a twin
handle's greedy rollout must give the evaluation's bits up to every env's first done.  The scenarios end their episodes on steps
that differ from env to env inside a wave (tests/_async_scenarios.py): a staggered TimeLimit for Solow, depletion for TradeAR1.
Against the float64 oracle the evaluation is held teacher-forced, with the tolerances of test_gpu_gaussnet.py."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _async_scenarios as SC
import _gauss_oracle as A
from oracle import oracle as O
from test_gpu_gaussnet import FWD_ATOL, FWD_RTOL, _params

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS = ("solow", "trade")
SIZES = {"solow": A.SOLOW, "trade": A.TRADE}
SEED, OFF = SC.GEN_SEED, SC.GEN_OFFSET
E, R = SC.E, 5
CAP = {"solow": SC.CAP, "trade": 16}
PSEED = {"solow": 5, "trade": 7}
TRADE_KW = dict(trade_starting_balance=1.02, trade_std_p=0.3)
TRACE = ("states", "mu", "actions", "rewards", "dones")


def _pair(kind, n_env=E, cap=None, flags=0, seed=SEED, off=OFF, stagger=True, pseed=None, **kw):
    """A reset engine of the scenario with its net: Solow with the staggered TimeLimit, TradeAR1 close to depletion."""
    from goldsrl import _ffi, _ffi_gauss
    cap = CAP[kind] if cap is None else cap
    if kind == "solow":
        kw.setdefault("solow_tape_len", 64)
        eng = _ffi.Engine(_ffi.ENV_SOLOW, n_env, seed=seed, env_id_offset=off, max_episode_steps=cap, flags=flags, **kw)
    else:
        eng = _ffi.Engine(_ffi.ENV_TRADE, n_env, seed=seed, env_id_offset=off, n_assets=2, max_episode_steps=cap, flags=flags,
                          **dict(TRADE_KW, **kw))
    eng.reset()
    if kind == "solow" and stagger:
        eng.set_state("ELAPSED", SC.staggered_elapsed(E)[:n_env])
    net = _ffi_gauss.GaussNet(eng, rnn_length=R, scale=100.0 if kind == "solow" else 1.0, max_samples=8192)
    net.set_params(_params(kind, PSEED[kind] if pseed is None else pseed))
    return eng, net


def _close(*pairs):
    for eng, net in pairs:
        net.close(); eng.close()


def _first_done(dones):
    """n (E,): index of each env's first done + 1; every env must have one"""
    d = dones > 0
    assert d.any(axis=0).all()
    return d.argmax(axis=0) + 1


@pytest.fixture(scope="module", params=KINDS)
def case(request):
    """The evaluation of the scenario with a full trace, and the twin handle's greedy rollout over the cap."""
    kind = request.param
    cap = CAP[kind]
    eng, net = _pair(kind)
    start = {}
    if kind == "solow":
        start = {k: eng.get_state(k) for k in ("SOLOW_K", "SOLOW_Z", "SOLOW_E", "SOLOW_TAPE")}
    ev = net.eval(cap, trace_steps=cap)
    elapsed_after = eng.get_state("ELAPSED")
    twin = _pair(kind)
    twin[1].set_greedy(True)
    twin[1].rollout(cap)
    ro = {k: twin[1].read_rollout(k) for k in ("states", "windows", "raw", "mu", "sigma", "actions", "rewards", "dones")}
    _close((eng, net), twin)
    return dict(kind=kind, cap=cap, ev=ev, ro=ro, start=start, elapsed_after=elapsed_after)


# ------------------------------------------------------------------------------------------ 1. greedy rollout
@pytest.mark.parametrize("kind", KINDS)
def test_greedy_rollout(kind):
    T = 12
    D, Aa = SIZES[kind]["static_size"], SIZES[kind]["num_actions"]
    eng, net = _pair(kind)
    net.set_action_counter(1000)
    net.set_greedy(True)
    net.rollout(T)
    r = {k: net.read_rollout(k) for k in ("states", "windows", "raw", "mu", "sigma", "values", "actions", "dones")}
    assert net.get_action_counter() == 1000                       # nothing was drawn
    assert np.array_equal(r["raw"], r["mu"])
    assert (r["dones"] > 0).any()                                 # windows restart inside the rollout
    for t in range(T):
        for e in range(E):
            raw1, ea = A.act(r["mu"][t, e], r["sigma"][t, e], np.zeros(Aa), tanh_action=(kind == "trade"))
            assert np.array_equal(raw1, r["mu"][t, e])
            np.testing.assert_allclose(r["actions"][t, e], ea, rtol=1e-6, atol=0)
    got = net.predict(r["states"].reshape(-1, D), r["windows"].reshape(-1, R, D))
    for k in ("mu", "sigma", "values"):
        np.testing.assert_array_equal(got[k], r[k].reshape(got[k].shape), err_msg=k)
    # greedy off again: the stochastic rollout of a handle that saw the switch equals one that never did
    a, b = _pair(kind), _pair(kind)
    a[1].set_greedy(True); a[1].set_greedy(False)
    for _, nt in (a, b):
        nt.rollout(T)
    for k in ("states", "windows", "raw", "mu", "sigma", "values", "actions", "rewards", "dones", "adv", "targets", "boot"):
        np.testing.assert_array_equal(a[1].read_rollout(k), b[1].read_rollout(k), err_msg=k)
    assert a[1].get_action_counter() == b[1].get_action_counter() == T
    assert not np.array_equal(a[1].read_rollout("raw"), a[1].read_rollout("mu"))
    _close((eng, net), a, b)


# ------------------------------------------------------------------------------------------ 2. eval == the per-step path
def test_eval_is_the_greedy_rollout_bit_for_bit(case):
    kind, cap, ev, ro = case["kind"], case["cap"], case["ev"], case["ro"]
    n = _first_done(ro["dones"])
    lengths = np.unique(ev["length"])
    print("eval %s: lengths %s, mixed share %.2f" % (kind, lengths.tolist(), SC.mixed_share(
        (ro["dones"] > 0) & (np.arange(cap)[:, None] < n[None]))))
    if kind == "solow":
        assert np.array_equal(ev["length"], cap - SC.staggered_elapsed(E)) and ev["length"].min() == 1 and ev["length"].max() == cap
    else:
        depleted = ev["length"] < cap
        assert depleted.sum() >= E // 4 and len(lengths) >= 8
    first = (ro["dones"] > 0) & (np.arange(cap)[:, None] < n[None])      # the twin's dones truncated at each env's first done
    assert SC.mixed_share(first) >= 0.25
    assert np.array_equal(ev["length"], n) and (ev["finished"] == 1).all()
    S = ev["rewards"].shape[0]
    assert S == min(cap, int(ev["length"].max()))
    for e in range(E):
        ne = int(n[e])
        total = 0.0
        for v in ro["rewards"][:ne, e]:
            total += float(v)                                            # total_reward += reward, float64
        assert ev["total_reward"][e] == total, e
        for k in TRACE:
            np.testing.assert_array_equal(ev[k][:ne, e], ro[k][:ne, e], err_msg="%s env %d" % (k, e))
    assert (case["elapsed_after"] == 0).all()


# ------------------------------------------------------------------------------------------ 3. against the oracle
def test_eval_against_the_oracle_teacher_forced(case):
    kind, cap, ev = case["kind"], case["cap"], case["ev"]
    n = ev["length"]
    S = ev["rewards"].shape[0]
    live = np.arange(S)[:, None] < n[None]                               # (S,E): the step was played
    # the traced states are each env's episode from its start: the windows follow from them
    dones = ev["dones"].copy(); dones[~live] = 0
    win, _ = A.replay_windows(np.where(live[..., None], ev["states"], 0).astype(np.float32), dones, R)
    p = A.unflatten(_params(kind, PSEED[kind]).astype(np.float64), **SIZES[kind])
    mu = A.forward(p, ev["states"][live].astype(np.float64), win[live].astype(np.float64), 100.0 if kind == "solow" else 1.0)[0]
    np.testing.assert_allclose(ev["mu"][live], mu, rtol=FWD_RTOL, atol=FWD_ATOL)
    acts = ev["actions"]
    if kind == "solow":
        st = case["start"]
        rho_z, rho_e = O.solow_rhos(1, 1)
        k, z, e_ = (st[f].astype(np.float64) for f in ("SOLOW_K", "SOLOW_Z", "SOLOW_E"))
        tape = st["SOLOW_TAPE"].astype(np.float64)
        TT = tape.shape[1]
        for t in range(S):
            a = np.where(live[t], acts[t, :, 0], 0.5).astype(np.float64)
            k, z, e_, obs, rew = O.solow_step(k, z, e_, tape[:, TT - 1 - t], a, rho_z, rho_e)
            np.testing.assert_allclose(ev["rewards"][t][live[t]], rew[live[t]], rtol=1e-5, atol=5e-6)
            assert np.array_equal(ev["dones"][t][live[t]] > 0, (n == t + 1)[live[t]])
            if t + 1 < S:
                nx = live[t + 1]
                np.testing.assert_allclose(ev["states"][t + 1][nx], O.solow_process_state(obs)[nx], rtol=1e-5, atol=1e-6)
    else:
        nrm = SC.trade_generator_normals(SEED, OFF, E, S, 2)
        start = TRADE_KW["trade_starting_balance"]
        cash, assets = np.full(E, start), np.full(E, start)
        q, pr = np.zeros((E, 2)), np.ones((E, 2))
        for t in range(S):
            a = np.where(live[t][:, None], acts[t], 0.0).astype(np.float64)
            cash, assets, q, pr, obs, rew, done = O.trade_step(cash, assets, q, pr, a, nrm[t], O.trade_std_e(TRADE_KW["trade_std_p"]))
            done = done | (t + 1 >= cap)
            np.testing.assert_allclose(ev["rewards"][t][live[t]], rew[live[t]], rtol=1e-5, atol=1e-9)
            assert np.array_equal(ev["dones"][t][live[t]] > 0, done[live[t]])
            if t + 1 < S:
                nx = live[t + 1]
                np.testing.assert_allclose(ev["states"][t + 1][nx], O.trade_process_state(obs)[nx], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------ 4. group edges
def test_eval_does_not_depend_on_the_env_count(case):
    kind, cap, ev = case["kind"], case["cap"], case["ev"]
    for n_env in (1, 63, 64, 65):
        pair = _pair(kind, n_env)
        got = pair[1].eval(cap)
        _close(pair)
        assert set(got) == {"total_reward", "length", "finished"}
        assert np.array_equal(got["total_reward"], ev["total_reward"][:n_env]), n_env
        assert np.array_equal(got["length"], ev["length"][:n_env]) and (got["finished"] == 1).all()


# ------------------------------------------------------------------------------------------ 5. max_steps
def test_eval_max_steps():
    from goldsrl import _ffi
    n_env = 70
    eng, net = _pair("solow", n_env, cap=0, stagger=False, solow_tape_len=2048)
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
    _close((eng, net))


def test_read_eval_before_any_evaluation_is_an_error():
    from goldsrl import _ffi
    eng, net = _pair("solow", 3)
    buf = np.zeros(3, np.float64)
    rc = net.lib.grl_anet_read_eval(net.n, b"total_reward", _ffi._ptr(buf), buf.nbytes)
    assert rc == _ffi.E_STATE
    _close((eng, net))


# ------------------------------------------------------------------------------------------ 6. eval leaves the rest alone
def test_eval_leaves_training_and_the_handle_alone():
    from goldsrl import _ffi
    n_env, cap = 100, 9
    a = _pair("solow", n_env, cap=cap, flags=_ffi.F_RESEED_EACH_RESET, stagger=False)
    b = _pair("solow", n_env, cap=cap, flags=_ffi.F_RESEED_EACH_RESET, stagger=False)
    a[1].rollout(4); b[1].rollout(4)
    a[1].eval(cap, trace_steps=cap)                                      # between the rollout and its update
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
    for k in ("states", "windows", "raw", "mu", "sigma", "values", "actions", "rewards", "dones", "weights", "adv", "targets", "boot"):
        np.testing.assert_array_equal(a[1].read_rollout(k), b[1].read_rollout(k), err_msg=k)
    assert a[1].get_action_counter() == b[1].get_action_counter() == 7
    # reset() + eval repeats: the eval registration's episodes are the same ones every time
    params = _params("solow", PSEED["solow"])
    runs = []
    for _ in range(2):
        a[1].set_params(params)
        a[0].reset()
        runs.append(a[1].eval(cap, trace_steps=cap))
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)
    _close(a, b)


def test_eval_from_a_running_handle_differs_from_a_reset_one():
    """eval starts from the handle's CURRENT state: 4 steps into their episodes the envs have 5 steps left of the 9."""
    a = _pair("solow", 70)
    fresh = a[1].eval(SC.CAP)
    a[1].rollout(4)
    later = a[1].eval(SC.CAP)
    assert np.array_equal(fresh["length"], SC.CAP - SC.staggered_elapsed(70)) and (later["length"] == SC.CAP - 4).all()
    assert not np.array_equal(fresh["total_reward"], later["total_reward"])
    _close(a)


# ------------------------------------------------------------------------------------------ 7. full length, and the host monitor
def _eval_registration(n_env, cap):
    from goldsrl import _ffi, _ffi_gauss
    eng = _ffi.Engine(_ffi.ENV_SOLOW, n_env, seed=1692, flags=_ffi.F_RESEED_EACH_RESET, max_episode_steps=cap)
    eng.reset()
    net = _ffi_gauss.GaussNet(eng, rnn_length=R, scale=100.0, max_samples=1)
    net.set_params(_params("solow", 5))
    return eng, net


def test_full_length_episodes_of_the_eval_registration():
    big, one = _eval_registration(65, 1024), _eval_registration(1, 1024)
    eb, e1 = big[1].eval(1024), one[1].eval(1024)
    _close(big, one)
    assert (eb["length"] == 1024).all() and (eb["finished"] == 1).all() and np.isfinite(eb["total_reward"]).all()
    assert e1["total_reward"][0] == eb["total_reward"][0] and e1["length"][0] == 1024
    assert len(np.unique(eb["total_reward"])) == 65                      # 65 different seeded episodes


def test_env_0_is_the_host_monitors_episode(tmp_path, monkeypatch):
    """GreedyMonitor.eval_once of scripts/train_solow.py on the same registration with a 40-step cap: same episode, the float64
    sigmoid of the host path against the device's float32 one.  Bound: the per-step reward tolerance of test_rollout_replay, summed."""
    from goldsrl.envs import fed_env
    from goldsrl.scripts import train_solow
    cap = 40

    def register(p, q):
        fed_env.registry["Solow-%d-%d-finite-eval-v0" % (p, q)] = (fed_env.SolowEnv, cap, dict(p=p, q=q, seed=1692))
    monkeypatch.setattr(fed_env, "register_solow_env", register)
    mon = train_solow.GreedyMonitor(0, str(tmp_path / "host.json"))
    params = _params("solow", 5)
    host_total, host_len = mon.eval_once(params)
    mon.close()
    pair = _eval_registration(3, cap)
    ev = pair[1].eval(cap, trace_steps=cap)
    _close(pair)
    assert host_len == cap and ev["length"][0] == cap
    bound = cap * (5e-6 + 1e-5 * float(np.abs(ev["rewards"][:, 0]).max()))
    print("env 0: device %.9g host %.9g bound %.3g" % (ev["total_reward"][0], host_total, bound))
    assert abs(ev["total_reward"][0] - host_total) <= bound


# ------------------------------------------------------------------------------------------ 8. scripts
def _run(module, out, extra):
    from goldsrl import utils_tfevents
    cmd = [sys.executable, "-m", "goldsrl.scripts." + module, "--envs", "128", "--t_max", "8", "--updates", "2", "--model_dir", str(out)] + extra
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "golds-rl-gym_amd"), os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    (events,) = glob.glob(os.path.join(str(out), "events.out.tfevents.*"))
    scalars = {}
    for tag, value, step, _ in utils_tfevents.read_scalars(events):
        scalars.setdefault(tag, []).append((step, value))
    return scalars


@pytest.mark.parametrize("module,log_name", [("train_solow", "Solow-1-1.json"), ("train_trade", "TradeAR1.json")])
def test_scripts_evaluate_on_the_device(tmp_path, module, log_name):
    out = tmp_path / "run"
    scalars = _run(module, out, ["--eval-envs", "64", "--eval-every", "1"])
    log = json.load(open(out / log_name))
    assert set(log) == {"total_reward", "episode_length", "mean_total_reward", "std_total_reward", "n_envs"}
    assert log["n_envs"] == 64
    for k in ("total_reward", "episode_length", "mean_total_reward", "std_total_reward"):
        assert len(log[k]) == 2 and all(np.isfinite(v) for v in log[k]), k
    assert all(1 <= v <= 1024 for v in log["episode_length"]) and (module != "train_solow" or log["episode_length"] == [1024, 1024])
    assert all(v > 0 for v in log["std_total_reward"])
    for tag, key in (("eval/total_reward", "total_reward"), ("eval/episode_length", "episode_length"), ("eval/mean_total_reward", "mean_total_reward")):
        assert [s for s, _ in scalars[tag]] == [2, 4]
        np.testing.assert_allclose([v for _, v in scalars[tag]], log[key], rtol=1e-6)


def test_train_solow_without_eval_envs_writes_what_it_wrote(tmp_path):
    out = tmp_path / "run"
    scalars = _run("train_solow", out, ["--eval-every", "2"])
    log = json.load(open(out / "Solow-1-1.json"))
    assert set(log) == {"total_reward", "episode_length"} and log["episode_length"] == [1024]
    assert "eval/mean_total_reward" not in scalars and len(scalars["eval/total_reward"]) == 1
    assert not os.path.exists(out / "TradeAR1.json")
