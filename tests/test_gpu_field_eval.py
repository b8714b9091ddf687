"""GPU: grl_fieldnet_eval (include/goldsrl_fieldeval.h) -- the field policy's whole episode in one launch -- against the two paths it
restates nothing of: the host loop predict_swarm -> transform_actions -> float64 step (greedy, float64 rows) and the training
rollout (drawn, float32 rows), byte for byte; that it writes nothing it reads; its refusals; and the monitor built on it.
Tiny shapes: TimeLimit 3 with staggered counters, at most 8 steps; the monitor test alone plays the registered 128."""
import json

import numpy as np
import pytest

import _async_scenarios as SC
import _field_rollout_cases as FC

pytestmark = pytest.mark.gpu

GEOMS = sorted(FC.GEOMS)
TRACE_NET = (("trace_mu", "mu"), ("trace_sigma", "sigma"))
TRACE_OBS = (("trace_locust_bins", "locust_bins"), ("trace_agent_bins", "agent_bins"), ("trace_positions", "positions"))


def _swarm_engine(geom, n_envs, flags=0, elapsed=None):
    from goldsrl import _ffi
    eng = _ffi.Engine(_ffi.ENV_SWARM, n_envs, seed=FC.SEED, env_id_offset=FC.OFFSET, max_episode_steps=FC.CAP, grid_size=FC.GEOMS[geom]["height"],
                      flags=flags)
    eng.reset()
    if elapsed is not None:
        eng.set_state("ELAPSED", elapsed)
    eng.episodes_enable()
    return eng


def _host_loop(twin, tnet, max_steps):
    """The episode of every env of `twin` as FieldSwarmPolicyMonitor's host loop plays it: per step and env the observation acted on,
    mu / sigma / value, the float64 action, the reward and the positions after the step; length and finished by the end rule."""
    n, cap = twin.E, FC.CAP
    t_limit = np.maximum(cap - twin.get_state("ELAPSED").astype(np.int64), 1)
    steps = []
    for t in range(max_steps):
        obs = {name: twin.read(name) for _, name in TRACE_OBS}
        pred = tnet.predict_swarm()
        act = twin.transform_actions(pred["mu"]).astype(np.float64).reshape(n, 10, 2)
        twin.swarm_step_f64(act)
        # the step resets an env that is done (emulator_runner.py:128-132): behind such a step x / xa are the next episode's
        steps.append(dict(obs, mu=pred["mu"].reshape(n, 10, 2), sigma=pred["sigma"].reshape(n, 10, 2), value=pred["vs"].reshape(n, 10), actions=act,
                          reward=twin.read("reward_f64"), done=twin.read("done"), x=twin.get_state("SWARM_X"), xa=twin.get_state("SWARM_XA")))
    length, finished = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for e in range(n):
        for t in range(max_steps):
            fin = steps[t]["reward"][e] >= 0 or t + 1 >= t_limit[e]
            if fin or t + 1 == max_steps:
                length[e], finished[e] = t + 1, fin
                break
    return steps, length, finished


def _compare_greedy(geom, n_envs, max_steps, flags=0):
    from goldsrl import _ffi_replay
    el = SC.staggered_elapsed(n_envs, FC.CAP)
    eng, twin = _swarm_engine(geom, n_envs, flags, el), _swarm_engine(geom, n_envs, flags, el)
    FC.share_cells(eng); FC.share_cells(twin)
    net, tnet = FC.net(eng, geom), FC.net(twin, geom)
    steps, length, finished = _host_loop(twin, tnet, max_steps)
    for trace_env in range(n_envs):
        r = net.eval(max_steps, greedy=True, rows32=False, keep_actions=True, trace_env=trace_env)
        assert np.array_equal(r["length"], length) and np.array_equal(r["finished"], finished)
        for e in range(n_envs):
            n = length[e]
            assert np.array_equal(r["rewards"][e, :n], np.array([s["reward"][e] for s in steps[:n]])) and not r["rewards"][e, n:].any()
            assert np.array_equal(r["actions"][e, :n], np.stack([s["actions"][e] for s in steps[:n]])) and not r["actions"][e, n:].any()
            assert r["total_reward"][e] == sum(float(s["reward"][e]) for s in steps[:n])
        n = length[trace_env]
        for k, name in TRACE_NET + TRACE_OBS:
            want = np.stack([s[name][trace_env] for s in steps[:n]])
            assert np.array_equal(r[k][:n], want), (k, trace_env)
            assert not r[k][n:].any(), (k, trace_env)
        # positions: the twin's state reads wherever the twin still holds the episode (its step resets a done env at once), and at
        # every step the replay kernel's trace of the kept actions from the same start state
        rep = _ffi_replay.swarm_replay(eng, r["actions"][trace_env][None, :n], trace_env=trace_env)
        assert np.array_equal(rep["rewards"][trace_env, 0], r["rewards"][trace_env, :n]) and rep["length"][trace_env, 0] == n
        for k, name in (("trace_x", "x"), ("trace_xa", "xa")):
            held = [t for t in range(n) if not steps[t]["done"][trace_env]]
            assert len(held) >= n - 1 and all(np.array_equal(r[k][t], steps[t][name][trace_env]) for t in held), (k, trace_env)
            assert np.array_equal(r[k][:n], rep[k][0]) and not r[k][n:].any(), (k, trace_env)
        assert np.array_equal(r["trace_value"][:n], np.array([s["value"][trace_env, 0] for s in steps[:n]]))
        assert np.array_equal(r["trace_raw"][:n], r["trace_mu"][:n])      # greedy: the raw action is mu
    bins = np.concatenate([np.stack([s[k] for s in steps]).reshape(-1) for k in ("locust_bins", "agent_bins")])      # every bin byte the twin observed
    for x in (net, tnet, eng, twin):
        x.close()
    return length, finished, bins


@pytest.mark.parametrize("geom", GEOMS)
def test_greedy_f64_rows_one_env_is_the_host_loop(geom):
    """1. E = 1: the TimeLimit (3, counter 0) ends the episode before max_steps = 8 does."""
    length, finished, _ = _compare_greedy(geom, 1, 8)
    assert length.tolist() == [3] and finished.tolist() == [1]


@pytest.mark.parametrize("max_steps", [2, 8])
@pytest.mark.parametrize("geom", GEOMS)
def test_greedy_f64_rows_five_envs_are_the_host_loop(geom, max_steps):
    """1. E = 5, agents sharing a cell, an agent and a locust outside the box; with max_steps = 2 both endings occur."""
    length, finished, bins = _compare_greedy(geom, 5, max_steps)
    assert (bins == 255).any()      # the point outside the box was observed as such
    if max_steps == 2:
        assert (finished == 1).any() and (finished == 0).any() and length.tolist() == [2, 2, 1, 2, 2]
    else:
        assert finished.all() and length.tolist() == [3, 2, 1, 3, 2]


@pytest.mark.parametrize("geom", GEOMS)
def test_drawn_f32_rows_are_the_training_rollout(geom, monkeypatch):
    """2. greedy = 0, rows32 = 1 against rollout(T) of a twin net and engine (fused path, reward layout 0), up to each env's first done."""
    sc = FC.scenario(geom, True, 0, monkeypatch)
    ro, E, T = sc["ro"], FC.E, FC.T
    eng = FC.engine(geom, elapsed=SC.staggered_elapsed(E, FC.CAP))
    FC.share_cells(eng)
    net = FC.net(eng, geom, counter=FC.COUNTER0)
    first = np.array([int(np.argmax(ro["dones"][:, e])) for e in range(E)])
    assert ro["dones"].any(axis=0).all()
    per_agent = lambda a: a.reshape((T, E, 10) + a.shape[2:])
    for trace_env in range(E):
        r = net.eval(T, greedy=False, rows32=True, keep_actions=True, trace_env=trace_env)
        assert np.array_equal(r["length"], first + 1) and r["finished"].all()
        n = first[trace_env] + 1
        for k, name in (("trace_raw", "actions"), ("trace_mu", "mu"), ("trace_sigma", "sigma")):
            assert np.array_equal(r[k][:n], per_agent(ro[name])[:n, trace_env]), (k, trace_env)
        assert np.array_equal(r["trace_value"][:n], per_agent(ro["values"])[:n, trace_env, 0])
        for k, name in (("trace_locust_bins", "lb"), ("trace_agent_bins", "ab"), ("trace_positions", "ps")):
            assert np.array_equal(r[k][:n], ro[name][:n, trace_env]), (k, trace_env)
        for e in range(E):
            m = first[e] + 1
            assert np.array_equal(r["rewards"][e, :m].astype(np.float32), per_agent(ro["rewards"])[:m, e, 0])
            assert np.array_equal(r["actions"][e, :m].astype(np.float32), per_agent(ro["env_actions"])[:m, e])
            assert np.array_equal(r["actions"][e, :m].astype(np.float32).astype(np.float64), r["actions"][e, :m])
    assert net.get_action_counter() == FC.COUNTER0
    net.close(); eng.close()


def _everything(eng, net, T):
    out = {k: eng.get_state(k) for k in ("SWARM_X", "SWARM_XA", "SWARM_PNOISE", "SWARM_ANOISE", "ELAPSED", "EPISODE")}
    out.update({k: eng.read(k) for k in ("locust_bins", "agent_bins", "positions", "reward", "reward_f64", "done", "done_count")})
    out["ep_total"], out["ep_len"] = eng.episodes_running()
    out["params"] = net.get_params()
    st = net.get_optimizer_state()
    out.update(adam_m=st["adam_m"], adam_v=st["adam_v"], adam_step=np.array(st["adam_step"]), counter=np.array(net.get_action_counter()))
    out.update({"ro_" + k: v for k, v in FC.read_rollout(net, T).items()})
    return out


def test_eval_reads_only():
    """3. After an eval of each kind the env state, the observation, the episode records, the parameters, the optimizer state, the action
    counter and every buffer of the rollout made before read back as they were."""
    geom, E, T = "G12_L1_F4", 5, 2
    eng = FC.engine(geom, elapsed=SC.staggered_elapsed(E, FC.CAP))
    FC.share_cells(eng)
    net = FC.net(eng, geom, counter=FC.COUNTER0)
    net.rollout(T, 0)
    net.train_rollout(1e-3)      # non-zero Adam moments
    eng.wait()
    before = _everything(eng, net, T)
    assert before["adam_m"].any() and before["counter"] == FC.COUNTER0 + T
    for kw in (dict(greedy=True, rows32=False, keep_actions=True, trace_env=0), dict(greedy=False, rows32=True, keep_actions=False, trace_env=E - 1)):
        r = net.eval(8, **kw)
        assert (r["length"] >= 1).all()
        after = _everything(eng, net, T)
        assert sorted(after) == sorted(before)
        for k in before:
            assert np.array_equal(before[k], after[k]), (k, kw)
    net.close(); eng.close()


def test_fast_math_handle_is_its_own_host_loop():
    """4. Case 1 at E = 1 on a handle with the fast-math flag; the twin has the flag too."""
    from goldsrl import _ffi
    length, finished, _ = _compare_greedy("G8_L2_F3", 1, 8, flags=_ffi.F_SWARM_FAST_MATH)
    assert length.tolist() == [3] and finished.tolist() == [1]


def test_refusals():
    """5. Past the LDS budget, outputs the last call did not keep, a wrong byte count, a read before the first eval, a step in flight."""
    from goldsrl import _ffi, _ffi_field
    big = dict(height=32, width=32, channels=2, filters=32, conv_layers=1, num_actions=2)      # image 8 KB + pooled map 32 KB + p2 16 KB + the env
    eng = _ffi.Engine(_ffi.ENV_SWARM, 1, seed=FC.SEED, max_episode_steps=FC.CAP, grid_size=32)
    eng.reset()
    net = _ffi_field.FieldNet(eng, max_samples=1, scale=FC.SCALE, **big)
    with pytest.raises(_ffi.GrlError) as ei:      # not bound
        net.eval(2)
    assert ei.value.code == _ffi.E_INVALID and "grl_fieldnet_eval" in str(ei.value)
    net.rollout_bind(FC.GAMMA)
    with pytest.raises(_ffi.GrlError) as ei:
        net.eval(2)
    assert ei.value.code == _ffi.E_STATE and "grl_fieldnet_eval" in str(ei.value) and "LDS" in str(ei.value)
    net.close(); eng.close()

    geom = "G8_L2_F3"
    eng = FC.engine(geom, n_envs=2)
    net = FC.net(eng, geom)
    with pytest.raises(_ffi.GrlError) as ei:
        net.read_eval("rewards", 2)
    assert ei.value.code == _ffi.E_STATE
    for bad in (dict(max_steps=0), dict(max_steps=2, trace_env=2), dict(max_steps=2, trace_env=-2)):
        with pytest.raises(_ffi.GrlError) as ei:
            net.eval(**bad)
        assert ei.value.code == _ffi.E_INVALID and "grl_fieldnet_eval" in str(ei.value)
    net.eval(2)
    for which in ("actions", "trace_mu", "trace_x"):
        with pytest.raises(_ffi.GrlError) as ei:
            net.read_eval(which, 2)
        assert ei.value.code == _ffi.E_STATE, which
    with pytest.raises(_ffi.GrlError) as ei:
        net.read_eval("rewards", 3)
    assert ei.value.code == _ffi.E_SIZE
    with pytest.raises(_ffi.GrlError) as ei:
        net.read_eval("reward", 2)
    assert ei.value.code == _ffi.E_INVALID
    eng.step_async(np.zeros((2, 10, 2), np.float32))
    with pytest.raises(_ffi.GrlError) as ei:
        net.eval(2)
    assert ei.value.code == _ffi.E_INVALID and "in flight" in str(ei.value)
    eng.wait()
    assert net.eval(2)["length"].tolist() == [2, 2]
    net.close(); eng.close()


def _monitor(tmp_path, name, geom, **kw):
    from goldsrl import _ffi
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import ConvPolicyVFieldNetwork
    conf = dict(FC.GEOMS[geom], entropy_regularisation_strength=FC.BETA, device="/gpu:0", scale=FC.SCALE, clip_norm=40.0, clip_norm_type="global")
    eng = _ffi.Engine(_ffi.ENV_SWARM, 1, grid_size=conf["height"], seed=1692, max_episode_steps=128)
    eng.reset()
    glob = ConvPolicyVFieldNetwork(conf).bind(eng, gamma=FC.GAMMA)
    glob.set_flat_params(FC.params(geom)[2])
    mon = PM.FieldSwarmPolicyMonitor(global_policy_net=glob, summary_writer=PM.ScalarWriter(str(tmp_path / name), tfevents=False), **kw)
    mon.actions_path = str(tmp_path / (name + ".json"))
    return mon, glob, eng


def _close(mon, glob, eng):
    mon.policy_net.net.close(); mon.env._eng.close(); glob.net.close(); eng.close()


def test_monitor_plays_the_host_loops_episode(tmp_path):
    """6. eval_once through the kernel returns what the host loop returns, keeps the same swarm-eval.json, which replays to its rewards;
    with three envs env 0 is that episode."""
    from goldsrl import _ffi_replay
    geom = "G8_L2_F3"
    dev, host, three = (_monitor(tmp_path, n, geom, **kw) for n, kw in (("dev", dict(device_episode=True)), ("host", dict(device_episode=False)),
                                                                       ("three", dict(device_episode=True, n_envs=3))))
    got, want = dev[0].eval_once(), host[0].eval_once()
    assert dev[0].device_episode and not host[0].device_episode
    assert got[1] == want[1] == 128 and got[0] == want[0] and got[2] == want[2] and all(isinstance(v, float) for v in got[2])
    kept, kept_host = json.load(open(dev[0].actions_path)), json.load(open(host[0].actions_path))
    assert kept == kept_host and kept["score"] == got[0]
    env = dev[0].env
    env.reset()
    rep = _ffi_replay.swarm_replay(env._eng, np.asarray(kept["actions"], np.float64)[None])
    assert rep["length"][0, 0] == 128 and rep["rewards"][0, 0].tolist() == got[2]
    tags = lambda name: [json.loads(l)["tag"] for l in open(tmp_path / name / "scalars.jsonl")]
    assert tags("dev") == tags("host") == ["eval/total_reward", "eval/episode_length"]
    got3 = three[0].eval_once()
    assert got3 == got and json.load(open(three[0].actions_path)) == kept
    assert three[0].total_rewards.shape == (3,) and three[0].total_rewards[0] == got[0] and three[0].episode_lengths.tolist() == [128] * 3
    assert len(set(three[0].total_rewards.tolist())) == 3      # three different seeded episodes
    assert tags("three") == ["eval/total_reward", "eval/episode_length", "eval/mean_total_reward"]
    for m in (dev, host, three):
        _close(*m)
