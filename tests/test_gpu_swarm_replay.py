"""GPU: scripted Swarm episodes in one launch (include/goldsrl_replay.h, csrc/swarm_replay.hip) against the per-step path on a
twin handle.  Both run block_step of csrc/swarm_dev.h, so rewards and positions are compared as bytes; only the case that holds the
replay to the unmodified reference's fixture has tolerances (those of test_swarm_eval_env_plays_the_references_seed_192_episode)."""
import json
import os
import queue

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("SWARM_X", "SWARM_XA", "SWARM_PNOISE", "SWARM_ANOISE", "ELAPSED", "EPISODE")
OUTPUTS = ("reward", "reward_f64", "done", "elapsed", "locust_bins", "agent_bins", "positions", "done_count")


def _engine(E, seed=7, **kw):
    from goldsrl import _ffi
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=seed, **kw)
    eng.reset()
    return eng


def _clip(a):
    """transform_actions_for_env (emulator_runner.py:113-118): rows with norm >= 1 are normalised"""
    n = np.sqrt((a ** 2).sum(axis=-1, keepdims=True))
    return np.where(n >= 1, a / np.maximum(n, 1e-30), a)


def _actions(shape, dtype, seed=0):
    return np.ascontiguousarray(_clip(np.random.RandomState(seed).normal(size=shape + (10, 2)) * 0.8).astype(dtype))


def _state(eng):
    return {f: eng.get_state(f) for f in FIELDS}


def _per_step(state, actions, flags=0):
    """The yardstick: a twin handle without a TimeLimit set to `state`, stepped through actions (E, T, 10, 2) one launch per step --
    swarm_step_f64 for float64 rows, step for float32 rows.  Returns rewards (E, T), x (E, T, 80, 2), xa (E, T, 10, 2)."""
    from goldsrl import _ffi
    E, T = actions.shape[:2]
    twin = _ffi.Engine(_ffi.ENV_SWARM, E, seed=99, max_episode_steps=0, flags=flags | _ffi.F_SWARM_NO_OBSERVE)
    twin.reset()
    for f in ("SWARM_X", "SWARM_XA", "SWARM_PNOISE", "SWARM_ANOISE"):
        twin.set_state(f, state[f])
    rew, xs, xas = np.zeros((E, T)), np.zeros((E, T, 80, 2)), np.zeros((E, T, 10, 2))
    for t in range(T):
        row = np.ascontiguousarray(actions[:, t])
        if row.dtype == np.float64:
            twin.swarm_step_f64(row)
        else:
            twin.step(row)
        rew[:, t], xs[:, t], xas[:, t] = twin.read("reward_f64"), twin.get_state("SWARM_X"), twin.get_state("SWARM_XA")
        assert not twin.read("done").any()          # no auto-reset inside the twin's episode
    twin.close()
    return rew, xs, xas


def _twin_for(state, acts, E, flags=0):
    """per-step results for shared rows (n_seq, T, 10, 2) or per-env rows (E, n_seq, T, 10, 2): lists over the sequences"""
    n_seq = acts.shape[-4]
    out = []
    for s in range(n_seq):
        rows = acts[:, s] if acts.ndim == 5 else np.broadcast_to(acts[s], (E,) + acts[s].shape)
        out.append(_per_step(state, np.ascontiguousarray(rows), flags))
    return out


def _assert_bits(out, twin, length, trace_env=None):
    E, n_seq, T = out["rewards"].shape
    for s in range(n_seq):
        rew, xs, xas = twin[s]
        for e in range(E):
            n = int(length[e, s])
            assert out["length"][e, s] == n
            assert out["rewards"][e, s, :n].tobytes() == rew[e, :n].tobytes(), (e, s)
            assert not out["rewards"][e, s, n:].any()
        if trace_env is not None:
            n = int(length[trace_env, s])
            assert out["trace_x"][s, :n].tobytes() == xs[trace_env, :n].tobytes(), s
            assert out["trace_xa"][s, :n].tobytes() == xas[trace_env, :n].tobytes(), s
            assert not out["trace_x"][s, n:].any() and not out["trace_xa"][s, n:].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_seq", [1, 3])
@pytest.mark.parametrize("E", [1, 3, 4, 5, 9])
def test_bits_against_the_per_step_path(E, n_seq, dtype):
    from goldsrl import _ffi_replay
    T = 6
    eng = _engine(E, max_episode_steps=128)
    acts = _actions((n_seq, T), dtype, seed=E * 10 + n_seq)
    mid = E // 2
    out = _ffi_replay.swarm_replay(eng, acts, trace_env=mid)
    assert out["rewards"].shape == (E, n_seq, T) and out["trace_x"].shape == (n_seq, T, 80, 2) and out["trace_xa"].shape == (n_seq, T, 10, 2)
    assert (out["length"] == T).all() and not out["finished"].any()
    _assert_bits(out, _twin_for(_state(eng), acts, E), np.full((E, n_seq), T), trace_env=mid)
    eng.close()


def test_ragged_script_lengths_inside_one_workgroup():
    from goldsrl import _ffi_replay
    E, T, lens = 3, 6, [1, 6, 3]
    eng = _engine(E, max_episode_steps=128)
    acts = _actions((3, T), np.float64, seed=5)
    out = _ffi_replay.swarm_replay(eng, acts, seq_len=lens, trace_env=1)
    want = np.tile(np.array(lens, np.int32), (E, 1))
    assert np.array_equal(out["length"], want) and not out["finished"].any()
    _assert_bits(out, _twin_for(_state(eng), acts, E), want, trace_env=1)
    eng.close()


@pytest.mark.parametrize("E,n_seq,lens,elapsed,length,finished", [
    # one workgroup, the TimeLimit of 8 ends its pairs after 2, 5, 8 and 6 steps
    (4, 1, None, [6, 3, 0, 2], [[2], [5], [8], [6]], [[1], [1], [1], [1]]),
    # scripts of 8 and 4 rows: the second one runs out before the TimeLimit wherever more than 4 steps are left
    (3, 2, [8, 4], [6, 3, 0], [[2, 2], [5, 4], [8, 4]], [[1, 1], [1, 0], [1, 0]]),
])
def test_time_limit_ends_differ_inside_one_workgroup(E, n_seq, lens, elapsed, length, finished):
    from goldsrl import _ffi_replay
    T = 8
    eng = _engine(E, max_episode_steps=8)
    eng.set_state("ELAPSED", np.array(elapsed, np.int32))
    acts = _actions((n_seq, T), np.float64, seed=11)
    out = _ffi_replay.swarm_replay(eng, acts, seq_len=lens, trace_env=1)
    assert out["length"].tolist() == length and out["finished"].tolist() == finished
    _assert_bits(out, _twin_for(_state(eng), acts, E), np.array(length), trace_env=1)
    eng.close()


def test_per_env_actions_equal_separate_replays():
    from goldsrl import _ffi, _ffi_replay
    E, n_seq, T = 5, 2, 4
    eng = _engine(E, max_episode_steps=128)
    st = _state(eng)
    acts = _actions((E, n_seq, T), np.float64, seed=3)
    out = _ffi_replay.swarm_replay(eng, acts, trace_env=3)
    for e in range(E):
        one = _ffi.Engine(_ffi.ENV_SWARM, 1, seed=1, max_episode_steps=128)
        one.reset()
        for f in ("SWARM_X", "SWARM_XA", "SWARM_PNOISE", "SWARM_ANOISE"):
            one.set_state(f, st[f][e:e + 1])
        ref = _ffi_replay.swarm_replay(one, acts[e], trace_env=0)
        assert ref["rewards"][0].tobytes() == out["rewards"][e].tobytes()
        assert np.array_equal(ref["length"][0], out["length"][e])
        if e == 3:
            assert ref["trace_x"].tobytes() == out["trace_x"].tobytes() and ref["trace_xa"].tobytes() == out["trace_xa"].tobytes()
        one.close()
    # and the per-env rows against the per-step path
    _assert_bits(out, _twin_for(st, acts, E), np.full((E, n_seq), T), trace_env=3)
    eng.close()


def test_the_handle_is_read_only():
    from goldsrl import _ffi_replay
    E = 5
    eng, other = _engine(E, max_episode_steps=128), _engine(E, max_episode_steps=128)
    first = _actions((E,), np.float32, seed=1)
    eng.step(first); other.step(first)          # so that the outputs hold something
    before = {f: eng.get_state(f).tobytes() for f in FIELDS}
    outs = {o: eng.read(o).tobytes() for o in OUTPUTS}
    _ffi_replay.swarm_replay(eng, _actions((2, 5), np.float64, seed=2), trace_env=2)
    _ffi_replay.swarm_replay(eng, _actions((E, 1, 3), np.float32, seed=3), seq_len=[2])
    assert {f: eng.get_state(f).tobytes() for f in FIELDS} == before
    assert {o: eng.read(o).tobytes() for o in OUTPUTS} == outs
    nxt = _actions((E,), np.float32, seed=4)
    eng.step(nxt); other.step(nxt)              # `other` never replayed
    for f in FIELDS:
        assert eng.get_state(f).tobytes() == other.get_state(f).tobytes(), f
    for o in OUTPUTS:
        assert eng.read(o).tobytes() == other.read(o).tobytes(), o
    eng.close(); other.close()


def test_the_references_seed_192_episode(golden):
    from goldsrl import envs
    from goldsrl.replay import SwarmReplay
    g = golden("swarm_traj")
    env = envs.make("Swarm-eval-v0")
    env.reset()
    out = SwarmReplay(env).play(g["actions"], trace_env=0)           # all 130 float64 rows
    assert out["rewards"].shape == (1, 1, 130)
    assert out["length"][0, 0] == 128 and out["finished"][0, 0] == 1
    np.testing.assert_allclose(out["rewards"][0, 0, :128], g["rewards"][:128], rtol=1e-9)
    assert not out["rewards"][0, 0, 128:].any()
    np.testing.assert_allclose(out["totals"][0, 0], np.sum(g["rewards"][:128]), rtol=1e-10)
    for i, step in enumerate(g["snap_steps"]):
        if step >= 127:
            break                                                    # at 127 the fixture holds the reset state (worker rule)
        np.testing.assert_allclose(out["xa_traj"][0, int(step)], g["xa_snap"][i], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(out["x_traj"][0, int(step)], g["x_snap"][i], rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("kind", ["fast", "refdiv"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_arithmetic_variants_against_a_twin_of_the_same_kind(kind, dtype, monkeypatch):
    from goldsrl import _ffi, _ffi_replay
    if kind == "refdiv":
        monkeypatch.setenv("GRL_SWARM_DIV", "ref")                   # read at grl_create, by the handle and by its twin
    flags = _ffi.F_SWARM_FAST_MATH if kind == "fast" else 0
    E, T = 5, 4
    eng = _engine(E, max_episode_steps=128, flags=flags)
    acts = _actions((2, T), dtype, seed=8)
    out = _ffi_replay.swarm_replay(eng, acts, trace_env=4)
    _assert_bits(out, _twin_for(_state(eng), acts, E, flags), np.full((E, 2), T), trace_env=4)
    eng.close()


@pytest.fixture(scope="module")
def monitor(tmp_path_factory):
    from goldsrl import envs, _ffi
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import ConvSingleAgentPolicyNetwork
    from goldsrl.agents.state_processors import SwarmStateProcessor
    conf = dict(name='local_learning', num_actions=2, clip_norm=40.0, clip_norm_type='global', device='/gpu:0',
                entropy_regularisation_strength=0.02, scale=1000.0, height=84, width=84, channels=3)
    d = tmp_path_factory.mktemp("replay")
    learner_eng = _ffi.Engine(_ffi.ENV_SWARM, 2, seed=5)
    learner_eng.reset()
    global_net = ConvSingleAgentPolicyNetwork(conf).bind(learner_eng, seed=11)
    mon = PM.SwarmPolicyMonitor(envs.make("Swarm-eval-v0"), global_net, SwarmStateProcessor(grid_size=84), PM.ScalarWriter(str(d / "eval")),
                                network_conf=conf)
    mon.actions_path = str(d / "swarm-eval.json")
    mon.tmp = d
    return mon


def test_make_swarm_gif_reproduces_the_monitors_score(monitor, capsys):
    from goldsrl.scripts import make_swarm_gif
    q = queue.Queue()
    for a in _actions((128,), np.float64, seed=21):
        q.put(a)
    total, length, rewards = monitor.eval_once(actions=q)
    assert length == 128 and json.load(open(monitor.actions_path))["score"] == total
    npy = str(monitor.tmp / "frames.npy")
    got, score = make_swarm_gif.main(["--actions", monitor.actions_path, "--no-gif", "--frames-npy", npy])
    printed = capsys.readouterr().out
    assert "score reproduced" in printed and "score differs" not in printed
    assert got == total == score                                     # the monitor's np.sum of the per-step path's rewards
    f = np.load(npy, mmap_mode="r")
    assert f.shape == (128, 320, 720, 3) and f.dtype == np.uint8
    # the same file replayed in the worker's float32 arithmetic is another episode (quirk Q7), and the script says so
    make_swarm_gif.main(["--actions", monitor.actions_path, "--no-gif", "--dtype", "float32"])
    assert "score differs" in capsys.readouterr().out


def test_scripted_baseline_totals_and_monitor_baseline(monitor):
    from goldsrl.baselines import ScriptedSwarmBaseline
    E, T = 3, 12
    eng = _engine(E, max_episode_steps=T)
    b = ScriptedSwarmBaseline(eng)
    assert b.scripts.shape == (2, T, 10, 2) and not b.scripts[0].any() and (b.scripts[1] == [-1.0, 0.0]).all()
    st = b.run()
    assert (st["length"] == T).all() and st["finished"].all()
    twin = _twin_for(_state(eng), b.scripts, E)
    for s in range(2):
        for e in range(E):
            assert st["totals"][e, s] == np.sum(twin[s][0][e])
    for e in range(E):
        name, total = b.best(e)
        assert total == st["totals"][e].max() and name == ("drift", "hold")[int(np.argmax(st["totals"][e]))]
    eng.close()
    # the monitor plays it on its own eval env and leaves that env as a reset leaves it
    monitor.env.reset()
    fresh = _state(monitor.env._eng)
    name, total = monitor.baseline()
    assert name in ("drift", "hold") and total == monitor.baseline_total_reward == monitor.baseline_stats["totals"][0].max()
    assert (monitor.baseline_stats["length"] == 128).all()
    after = _state(monitor.env._eng)
    for f in FIELDS:
        if f != "EPISODE":                                           # every reset starts a new episode
            assert after[f].tobytes() == fresh[f].tobytes(), f
    # the drift script through the monitor's per-step episode is the baseline's drift total, and the evaluation logs both scalars
    q = queue.Queue()
    for _ in range(128):
        q.put(np.zeros((10, 2)))
    drift, length, _ = monitor.eval_once(actions=q)
    assert length == 128 and drift == monitor.baseline_stats["totals"][0, 0]
    lines = [json.loads(ln) for ln in open(os.path.join(monitor.summary_writer.get_logdir(), "scalars.jsonl"))]
    logged = {ln["tag"]: ln["value"] for ln in lines}
    assert logged["eval/baseline_total_reward"] == total and logged["eval/total_reward_minus_baseline"] == drift - total


def test_error_paths():
    from goldsrl import _ffi, _ffi_replay
    solow = _ffi.Engine(_ffi.ENV_SOLOW, 2, seed=1)
    solow.reset()
    with pytest.raises(ValueError):
        _ffi_replay.swarm_replay(solow, _actions((1, 2), np.float64))
    lib = _ffi.load_library(extra_signatures=_ffi_replay.REPLAY_SIGNATURES)
    a = _actions((1, 2), np.float64)
    assert lib.grl_swarm_replay(solow.h, _ffi._ptr(a), 1, 1, 2, None, 0, -1) == _ffi.E_INVALID      # the C ABI refuses it too
    assert b"not a Swarm handle" in lib.grl_last_error(solow.h)
    solow.close()

    eng = _engine(2, max_episode_steps=128)
    buf = np.zeros(2 * 2 * 3)
    assert lib.grl_swarm_replay_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE      # before any replay
    acts = _actions((2, 3), np.float64)
    for bad in ([0, 3], [1, 4]):
        with pytest.raises(_ffi.GrlError) as ei:
            _ffi_replay.swarm_replay(eng, acts, seq_len=bad)
        assert ei.value.code == _ffi.E_INVALID
    with pytest.raises(ValueError):
        _ffi_replay.swarm_replay(eng, acts, seq_len=[1])
    with pytest.raises(TypeError):
        _ffi_replay.swarm_replay(eng, acts.astype(np.float16))
    for bad_env in (2, -2):
        with pytest.raises(_ffi.GrlError):
            _ffi_replay.swarm_replay(eng, acts, trace_env=bad_env)
    _ffi_replay.swarm_replay(eng, acts)                              # no trace
    tx = np.zeros((2, 3, 80, 2))
    assert lib.grl_swarm_replay_read(eng.h, b"trace_x", _ffi._ptr(tx), tx.nbytes) == _ffi.E_STATE
    assert lib.grl_swarm_replay_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes - 8) == _ffi.E_SIZE
    assert lib.grl_swarm_replay_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes) == _ffi.OK
    assert lib.grl_swarm_replay_read(eng.h, b"nothing", _ffi._ptr(buf), buf.nbytes) == _ffi.E_INVALID
    eng.step_async(_actions((2,), np.float32))                       # a step in flight
    assert lib.grl_swarm_replay(eng.h, _ffi._ptr(acts), 1, 2, 3, None, 0, -1) == _ffi.E_INVALID
    eng.wait()
    eng.close()
