"""GPU: grl_net_eval / grl_net_read_eval (include/goldsrl_neteval.h) -- the conv policy's evaluation episodes played on the device --
against the per-step paths whose code it shares and does not restate: the host loop predict -> (mu + sigma z).astype(float32) ->
transform_actions -> step -> read (host normals, greedy) and the training rollout (device noise), byte for byte; that the net's
training state is left alone; the range fallback; the refusals; the eval set's reset; and the monitor built on it.

Tiny shapes: at most 5 envs and 5 steps; the monitor test alone plays the registered 128-step episode (one pair).  The handles are
reseeded at every reset (F_RESEED_EACH_RESET), so a reset puts a handle back to the same start state and the host loop runs on the
same engine and net as the evaluation it is compared with."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 29
TRACE = ("trace_mu", "trace_sigma", "trace_raw", "trace_value")


def _named(flat):
    """Views into a flat parameter vector by name."""
    from goldsrl import _ffi_net
    out, at = {}, 0
    for name, shape in _ffi_net.CONV_PARAM_SHAPES:
        n = int(np.prod(shape))
        out[name] = flat[at:at + n].reshape(shape)
        at += n
    assert at == flat.size
    return out


def _params(seed=5):
    """Glorot kernels with small non-zero biases (with b1 = 0 the trunk's background terms vanish)."""
    from goldsrl import _ffi_net
    flat = _ffi_net.glorot_uniform_flat(seed=seed).copy()
    rng = np.random.RandomState(seed)
    for name, view in _named(flat).items():
        if name.endswith("_b"):
            view[...] = (rng.normal(size=view.shape) * 0.05).astype(np.float32)
    return flat


def _rig(E, chunk, cap=128, params=None, seed=SEED, **netkw):
    from goldsrl import _ffi, _ffi_net
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=seed, flags=_ffi.F_RESEED_EACH_RESET, max_episode_steps=cap)
    eng.reset()
    net = _ffi_net.ConvNet(eng, max_chunk_samples=chunk, **netkw)
    net.set_params(_params() if params is None else params)
    return eng, net


def _normals(E, S, seed=77):
    return np.random.RandomState(seed).normal(size=(E, S, 10, 2))


def _host_loop(eng, net, S, z=None):
    """The parent's per-step path on the handle from its reset state: z None acts greedily.  Per step mu / sigma / value, the raw and
    the env action, the float64 reward and done of every env; length = steps up to and with the env's first done."""
    E = eng.E
    eng.reset()
    steps = []
    for t in range(S):
        pred = net.predict()
        mu, sigma = pred["mu"].reshape(E, 10, 2), pred["sigma"].reshape(E, 10, 2)
        raw = mu if z is None else (mu + sigma * z[:, t]).astype(np.float32)
        act = eng.transform_actions(raw)
        eng.step(act)
        steps.append(dict(mu=mu, sigma=sigma, value=pred["vs"].reshape(E, 10), raw=raw, act=act, reward=eng.read("reward_f64"), done=eng.read("done")))
    done = np.stack([s["done"] for s in steps]).astype(bool)      # (S, E)
    length = np.where(done.any(axis=0), done.argmax(axis=0) + 1, S).astype(np.int32)
    return steps, length, done.any(axis=0).astype(np.uint8)


def _same_episodes(r, host, S, trace_env=-1):
    steps, length, finished = host
    E = len(length)
    assert np.array_equal(r["length"], length) and np.array_equal(r["finished"], finished)
    assert r["rewards"].shape == (E, S) and r["rewards"].dtype == np.float64
    for e in range(E):
        n = length[e]
        assert np.array_equal(r["rewards"][e, :n], np.array([s["reward"][e] for s in steps[:n]])), e
        assert not r["rewards"][e, n:].any(), e
        if "actions" in r:
            assert r["actions"].dtype == np.float32
            assert np.array_equal(r["actions"][e, :n], np.stack([s["act"][e] for s in steps[:n]])), e
            assert not r["actions"][e, n:].any(), e
        assert r["total_reward"][e] == sum(float(s["reward"][e]) for s in steps[:n])
    if trace_env >= 0:
        n = length[trace_env]
        for k in TRACE:
            want = np.stack([s[k[6:]][trace_env] for s in steps[:n]])
            assert r[k].dtype == np.float32 and np.array_equal(r[k][:n], want), k
            assert not r[k][n:].any(), k


def test_drawn_with_host_normals_one_env_is_the_host_loop():
    """1. E = 1, S = 4: rewards, length, kept actions and the trace of every step."""
    E, S = 1, 4
    eng, net = _rig(E, 10)
    z = _normals(E, S)
    host = _host_loop(eng, net, S, z)
    eng.reset()
    r = net.eval(S, normals=z, keep_actions=True, trace_env=0)
    _same_episodes(r, host, S, trace_env=0)
    assert host[1].tolist() == [S] and r["rewards"].all() and not np.array_equal(r["trace_raw"], r["trace_mu"])
    net.close(); eng.close()


def test_chunks_and_lanes(monkeypatch):
    """2. E = 5 in chunks of 2 envs (three chunks, the last ragged, on the lanes the rollout deals them to), S = 3, drawn and greedy;
    one lane gives the same bytes as the default."""
    E, S = 5, 3
    z = _normals(E, S)
    got = {}
    for lanes in (None, 1):
        if lanes is None:
            monkeypatch.delenv("GRL_NET_LANES", raising=False)
        else:
            monkeypatch.setenv("GRL_NET_LANES", str(lanes))      # read when a net is created
        eng, net = _rig(E, 20)
        for name, normals in (("drawn", z), ("greedy", None)):
            host = _host_loop(eng, net, S, normals)
            eng.reset()
            r = net.eval(S, greedy=normals is None, normals=normals, keep_actions=True, trace_env=E - 1)
            _same_episodes(r, host, S, trace_env=E - 1)
            if normals is None:
                assert np.array_equal(r["trace_raw"], r["trace_mu"])      # greedy: the raw action is mu
            got[(lanes, name)] = r
        net.close(); eng.close()
    for name in ("drawn", "greedy"):
        a, b = got[(None, name)], got[(1, name)]
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
    assert not np.array_equal(got[(None, "drawn")]["actions"], got[(None, "greedy")]["actions"])


def test_an_episode_that_ends_inside_the_call():
    """3. TimeLimit 3, S = 5: the episode ends at step 3, the auto-reset state goes on being stepped and nothing of it is kept;
    with S = 2 nothing ends."""
    E = 3
    eng, net = _rig(E, 20, cap=3)
    z = _normals(E, 5)
    host = _host_loop(eng, net, 5, z)
    assert host[1].tolist() == [3] * E and host[2].all()
    eng.reset()
    r = net.eval(5, normals=z, keep_actions=True, trace_env=1)
    _same_episodes(r, host, 5, trace_env=1)
    assert r["length"].tolist() == [3] * E and r["finished"].tolist() == [1] * E
    assert r["rewards"][:, :3].all() and not r["rewards"][:, 3:].any() and not r["actions"][:, 3:].any()
    eng.reset()
    r = net.eval(2, normals=z[:, :2], keep_actions=True)
    assert r["length"].tolist() == [2] * E and r["finished"].tolist() == [0] * E
    assert np.array_equal(r["rewards"], np.stack([s["reward"] for s in host[0][:2]], axis=1))
    net.close(); eng.close()


def test_device_noise_is_the_rollouts():
    """4. normals = None, greedy = False at action counter 7: the raw actions of every env are the training rollout's on a twin engine
    and net, the env actions their norm clip; the counter stays."""
    E, S, B = 4, 2, 40
    twin, tnet = _rig(E, 20)
    tnet.set_action_counter(7)
    tnet.rollout(S, 0)
    twin.wait()
    raw = tnet.read_rollout("actions", (S, B, 2)).reshape(S, E, 10, 2)
    assert tnet.get_action_counter() == 7 + S
    clipped = twin.transform_actions(raw)
    tnet.close(); twin.close()
    eng, net = _rig(E, 20)
    net.set_action_counter(7)
    for trace_env in range(E):
        eng.reset()
        r = net.eval(S, keep_actions=True, trace_env=trace_env)
        assert np.array_equal(r["trace_raw"], raw[:, trace_env]), trace_env
        assert np.array_equal(r["actions"], clipped.transpose(1, 0, 2, 3))
        assert net.get_action_counter() == 7
    net.close(); eng.close()


def test_the_training_state_is_left_alone():
    """5. rollout, eval with a read, train_rollout against rollout, train_rollout on a twin: parameters, Adam moments, step count and
    the returned statistics."""
    E, T = 4, 2
    out = []
    for with_eval in (True, False):
        eng, net = _rig(E, 20)
        net.set_action_counter(3)
        net.rollout(T, 0)
        eng.wait()
        if with_eval:
            r = net.eval(3, normals=_normals(E, 3), keep_actions=True, trace_env=0)
            assert r["length"].tolist() == [3] * E
        stats = net.train_rollout(1e-3)
        st = net.get_optimizer_state()
        out.append(dict(params=net.get_params(), m=st["adam_m"], v=st["adam_v"], step=st["adam_step"], stats=stats, counter=net.get_action_counter(),
                        keep=net.keep_info()["resident"]))
        net.close(); eng.close()
    a, b = out
    assert a["step"] == b["step"] == 1 and a["counter"] == b["counter"] == 3 + T and a["keep"] == b["keep"]
    assert a["m"].any() and a["stats"] == b["stats"] and all(np.isfinite(list(a["stats"].values())))
    for k in ("params", "m", "v"):
        assert np.array_equal(a[k], b[k]), k


def _overflowing_params():
    """The parameters of test_a_range_violation_moves_the_net_to_fp32_gemms_and_the_call_proceeds: relu(conv2) = 3e5 everywhere."""
    from goldsrl import _ffi_net
    flat = _ffi_net.glorot_uniform_flat(seed=3).copy()
    p = _named(flat)
    p["conv2_b"][...] = p["conv2_b"] + np.float32(3.0e5)
    p["conv3_w"][...] = (p["conv3_w"].astype(np.float64) * 1e-5).astype(np.float32)
    return flat


def test_a_range_violation_inside_an_evaluation(monkeypatch):
    """6. The first read raises E_RANGE and the net is on the fp32 form; after a reset the evaluation reads clean and is the host loop
    of a net forced onto that form.  With the fallback off the read fails alike and the net stays."""
    from goldsrl import _ffi
    E, S = 2, 2
    flat, z = _overflowing_params(), _normals(E, S)
    monkeypatch.delenv("GRL_NET_RANGE_FALLBACK", raising=False)
    eng, net = _rig(E, 20, params=flat)
    with pytest.raises(_ffi.GrlError) as ei:
        net.eval(S, normals=z, keep_actions=True)
    assert ei.value.code == _ffi.E_RANGE and "65504" in str(ei.value)
    assert net.range_info() == {"gemm_f32": True, "fallbacks": 1, "update_skipped": False}
    with pytest.raises(_ffi.GrlError) as ei:      # nothing of the invalid evaluation is handed out
        net.read_eval("rewards", S)
    assert ei.value.code == _ffi.E_STATE
    eng.reset()
    r = net.eval(S, normals=z, keep_actions=True, trace_env=1)
    assert net.range_info()["fallbacks"] == 1 and np.isfinite(r["rewards"]).all() and np.isfinite(r["trace_value"]).all()
    twin, tnet = _rig(E, 20, params=flat)
    tnet.predict()      # the upload's background pass ran on the fp16 form: this call takes its flag (and the fallback) ...
    tnet.set_gemm_f32(True)      # ... and the net is pinned to the fp32 form
    assert tnet.range_info()["gemm_f32"]
    _same_episodes(r, _host_loop(twin, tnet, S, z), S, trace_env=1)
    for x in (net, tnet, eng, twin):
        x.close()
    monkeypatch.setenv("GRL_NET_RANGE_FALLBACK", "off")      # read when the net is created
    eng, net = _rig(E, 20, params=flat)
    with pytest.raises(_ffi.GrlError) as ei:
        net.eval(S, normals=z)
    assert ei.value.code == _ffi.E_RANGE
    assert net.range_info() == {"gemm_f32": False, "fallbacks": 0, "update_skipped": False}
    net.close(); eng.close()


def test_refusals():
    """7. Every GRL_E_INVALID, GRL_E_STATE and GRL_E_SIZE case of the header."""
    from goldsrl import _ffi, _ffi_net

    def refused(code, call, *a, **kw):
        with pytest.raises(_ffi.GrlError) as ei:
            call(*a, **kw)
        assert ei.value.code == code, (a, kw, str(ei.value))
        return str(ei.value)

    E = 2
    eng, net = _rig(E, 20)
    assert net.lib.grl_net_eval(None, 2, 0, None, 0, -1) == _ffi.E_INVALID
    assert net.lib.grl_net_read_eval(None, b"rewards", None, 0) == _ffi.E_INVALID
    refused(_ffi.E_STATE, net.read_eval, "rewards", 2)      # before the first evaluation
    for bad in (dict(max_steps=0), dict(max_steps=1025), dict(max_steps=2, trace_env=E), dict(max_steps=2, trace_env=-2),
                dict(max_steps=2, greedy=True, normals=_normals(E, 2))):
        assert "grl_net_eval" in refused(_ffi.E_INVALID, net.eval, **bad)
    eng.step_async(np.zeros((E, 10, 2), np.float32))
    assert "in flight" in refused(_ffi.E_INVALID, net.eval, 2)
    eng.wait()
    assert net.eval(2)["length"].tolist() == [2, 2]
    for which in ("actions",) + TRACE:      # what the last evaluation did not keep
        refused(_ffi.E_STATE, net.read_eval, which, 2)
    refused(_ffi.E_SIZE, net.read_eval, "rewards", 3)
    refused(_ffi.E_INVALID, net.read_eval, "reward", 2)
    net.lib.grl_net_eval(net.n, 2, 0, None, 0, -1)      # asynchronous: a second call before anything joined
    assert "in flight" in refused(_ffi.E_INVALID, net.eval, 2)
    eng.wait()
    eng.step_async(np.zeros((E, 10, 2), np.float32))      # a read joins nothing but the streams: this step is still in flight behind it
    assert net.read_eval("length", 2).tolist() == [2, 2]
    assert "in flight" in refused(_ffi.E_INVALID, net.eval, 2)
    eng.wait()
    net.close()
    net3 = _ffi_net.ConvNet(eng, max_chunk_samples=20, num_actions=3)
    net3.set_params(_ffi_net.glorot_uniform_flat(seed=3, num_actions=3))
    assert "num_actions" in refused(_ffi.E_INVALID, net3.eval, 2)
    net3.close(); eng.close()
    # an output past int32: 104 858 envs x 1 024 steps x 20 kept floats; refused before anything is allocated or launched
    big = _ffi.Engine(_ffi.ENV_SWARM, 104858, seed=SEED)
    bnet = _ffi_net.ConvNet(big, max_chunk_samples=10)
    assert "int32" in refused(_ffi.E_INVALID, bnet.eval, 1024, keep_actions=True)
    bnet.close(); big.close()


def test_the_eval_sets_reset_side():
    """8. Env k of a seeded three-env SwarmEnv is the one-env SwarmEnv of seed + k: the state the reset leaves and the generator
    behind it, whose one (S, 10, 2) block is the host loop's S draws of (10, 2)."""
    from goldsrl.envs.multiagent import SwarmEnv
    three = SwarmEnv(seed=192, n_envs=3, max_episode_steps=128)
    three.reset()
    assert three.np_random is three.np_randoms[0] and len(three.np_randoms) == 3
    x, xa = three._eng.get_state("SWARM_X"), three._eng.get_state("SWARM_XA")
    for k in (1, 2):
        one = SwarmEnv(seed=192 + k, max_episode_steps=128)
        one.reset()
        assert np.array_equal(one._eng.get_state("SWARM_X")[0], x[k]) and np.array_equal(one._eng.get_state("SWARM_XA")[0], xa[k])
        block = three.np_randoms[k].normal(size=(2, 10, 2))
        assert np.array_equal(block, np.stack([one.np_random.normal(size=(10, 2)) for _ in range(2)]))
        one._eng.close()
    three._eng.close()


def _monitor(tmp_path, name, glob, cls, **kw):
    from goldsrl.agents.paac import policy_monitor as PM
    mon = cls(global_policy_net=glob, summary_writer=PM.ScalarWriter(str(tmp_path / name), tfevents=False), network_conf=glob.conf, **kw)
    mon.actions_path = str(tmp_path / (name + ".json"))
    return mon


def test_monitor_plays_the_host_loops_episode(tmp_path):
    """9. Swarm-eval-v0, 128 steps: the device monitor returns what SwarmPolicyMonitor.eval_once returns for the same global net, keeps
    the same swarm-eval.json and writes the same scalar tags; with three envs env 0 is that episode and the mean is written too."""
    from goldsrl import _ffi
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import ConvSingleAgentPolicyNetwork
    from goldsrl.envs import make
    conf = dict(num_actions=2, entropy_regularisation_strength=0.02, device="/gpu:0", height=84, width=84, channels=3, scale=1000.0, clip_norm=40.0,
                clip_norm_type="global")
    eng = _ffi.Engine(_ffi.ENV_SWARM, 1, seed=1692, max_episode_steps=128)
    eng.reset()
    glob = ConvSingleAgentPolicyNetwork(conf).bind(eng)
    glob.set_flat_params(_params())
    dev = _monitor(tmp_path, "dev", glob, PM.DeviceSwarmPolicyMonitor, n_envs=1)
    host = _monitor(tmp_path, "host", glob, PM.SwarmPolicyMonitor, env=make("Swarm-eval-v0"), state_processor=None)
    three = _monitor(tmp_path, "three", glob, PM.DeviceSwarmPolicyMonitor, n_envs=3)
    got, want = dev.eval_once(), host.eval_once()
    print("device monitor: total %.17g length %d; host loop: total %.17g length %d" % (got[0], got[1], want[0], want[1]))
    assert got[1] == want[1] == 128 and got[0] == want[0] and got[2] == want[2] and all(isinstance(v, float) for v in got[2])
    kept, kept_host = json.load(open(dev.actions_path)), json.load(open(host.actions_path))
    assert kept == kept_host and kept["score"] == got[0] and np.asarray(kept["actions"]).shape == (128, 10, 2)
    tags = lambda name: [json.loads(l)["tag"] for l in open(tmp_path / name / "scalars.jsonl")]
    assert tags("dev") == tags("host") == ["eval/total_reward", "eval/episode_length"]
    assert dev.total_rewards.tolist() == [got[0]] and dev.episode_lengths.tolist() == [128]
    got3 = three.eval_once()
    print("three envs: totals %s" % (three.total_rewards.tolist(),))
    assert three.total_rewards.shape == (3,) and three.total_rewards[0] == got[0] and three.episode_lengths.tolist() == [128] * 3
    assert got3 == got and json.load(open(three.actions_path)) == kept
    assert len(set(three.total_rewards.tolist())) == 3      # three different seeded episodes
    assert tags("three") == ["eval/total_reward", "eval/episode_length", "eval/mean_total_reward"]
    # the inherited baseline plays env 0's episode and leaves its handle reset (envs 1.. are reset by every eval_once)
    name, total = three.rule_baseline()
    left = [three.env._eng.get_state(f) for f in ("SWARM_X", "SWARM_XA", "ELAPSED")]
    three.env.reset()
    assert np.isfinite(total) and all(np.array_equal(a, three.env._eng.get_state(f)) for a, f in zip(left, ("SWARM_X", "SWARM_XA", "ELAPSED")))
    assert three.rest_env.n_envs == 2 and dev.rest_env is None      # env 0 alone on the registration's handle, envs 1.. beside it
    host.policy_net.net.close(); host.env._eng.close()
    dev.close(); three.close()
    glob.net.close(); eng.close()


def test_the_learner_builds_the_device_monitor(tmp_path):
    """10. --eval-envs 3 of train_paac_conv: GridPAACLearner evaluates on the device between updates, with the rule baseline's scalars."""
    from goldsrl.agents.paac.emulator_runner import SwarmRunner
    from goldsrl.agents.paac.paac import GridPAACLearner
    from goldsrl.scripts import train_paac_conv as S
    args = S.get_arg_parser().parse_args(["-ec", "4", "--max_local_steps", "2", "--max_global_steps", "16", "--eval-every", "1e-9", "--eval-envs", "3",
                                          "--rule-baseline", "-df", str(tmp_path / "logs")])
    nc, ec = S.get_network_and_environment_creator(args)
    learner = GridPAACLearner(nc, ec, args, SwarmRunner, state_processor=None)
    stats = learner.train()
    assert learner.global_step == 16 and np.isfinite(stats["loss"]) and learner.network.net.get_action_counter() == 4
    tags = [json.loads(l)["tag"] for l in open(tmp_path / "logs" / "scalars.jsonl")]
    for tag in ("eval/total_reward", "eval/episode_length", "eval/mean_total_reward", "eval/baseline_total_reward", "eval/total_reward_minus_baseline"):
        assert tags.count(tag) == 2, tag
    assert learner.policy_monitor.rest_env.n_envs == 2
    learner.cleanup()      # closes the monitor's two engines and nets, then the learner's own
    assert learner.policy_monitor is None


def test_the_monitor_rides_out_a_range_violation_on_both_nets(tmp_path, monkeypatch):
    """11. n_envs = 2 with the overflowing parameters in the global net: the monitor's two policy copies are two nets, each leaves the
    fp16 range in its own evaluation, each moves to the fp32 form and plays its episodes once more; eval_once returns, and so does
    the next one (whose parameter upload raises the flag again)."""
    from goldsrl import _ffi
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import ConvSingleAgentPolicyNetwork
    monkeypatch.delenv("GRL_NET_RANGE_FALLBACK", raising=False)
    conf = dict(num_actions=2, entropy_regularisation_strength=0.02, device="/gpu:0", height=84, width=84, channels=3, scale=1000.0, clip_norm=40.0,
                clip_norm_type="global")
    eng = _ffi.Engine(_ffi.ENV_SWARM, 1, seed=1692, max_episode_steps=128)
    eng.reset()
    glob = ConvSingleAgentPolicyNetwork(conf).bind(eng)
    glob.set_flat_params(_overflowing_params())
    mon = _monitor(tmp_path, "range", glob, PM.DeviceSwarmPolicyMonitor, n_envs=2)
    mon.max_episode_steps = 4      # the registration's env, four steps of it: the range, not the episode, is what this is about
    first = mon.eval_once()
    infos = [n.net.range_info() for n in (mon.policy_net, mon.rest_net)]
    assert all(i["gemm_f32"] and i["fallbacks"] == 1 for i in infos), infos
    assert first[1] == 4 and np.isfinite(first[2]).all() and np.isfinite(mon.total_rewards).all() and mon.episode_lengths.tolist() == [4, 4]
    again = mon.eval_once()
    assert again == first and [n.net.range_info()["fallbacks"] for n in (mon.policy_net, mon.rest_net)] == [1, 1]
    mon.close()
    glob.net.close(); eng.close()
