"""GPU: the receding-horizon rule planner of the Swarm env, a planned episode in one call (include/goldsrl_swarmplan.h,
csrc/swarm_plan.hip).  The oracle is the same computation composed on the host from tested pieces
(goldsrl/_ffi_swarmplan.py:swarm_plan_host: grl_swarm_rules for the lookahead, a Python loop of float64 adds, np.argmax,
grl_swarm_step_f64 for the commit); every comparison with it is of bytes.  Only the case that holds the planner to the unmodified
reference's fixture has tolerances (those of tests/test_gpu_swarm_rules.py's fixture case)."""
import json
import queue

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("SWARM_X", "SWARM_XA", "SWARM_PNOISE", "SWARM_ANOISE", "ELAPSED", "EPISODE")
OUTPUTS = ("reward", "reward_f64", "done", "elapsed", "locust_bins", "agent_bins", "positions", "done_count")
SAME = ("rewards", "choices", "scores", "actions", "length", "finished")

# (cancel, gain, anchor, off_x, off_y, radius): tests/test_gpu_swarm_rules.py's three -- a centroid ring that clips some agents, a
# nearest-locust rule that saturates, a nearest-locust ring with half the wind cancelled
RULES = np.array([(0, 1.5, 0, 0.1, 0.2, 0.5), (1, 5, 1, 0.3, -0.3, 0), (0.5, 2, 1, 0, 0, 0.2)], np.float64)
# (horizon, replan, steps): a last commit shorter than replan; horizon > replan; horizon = replan
HKS = ((1, 1, 5), (3, 2, 5), (4, 4, 6))


def _engine(E, seed=7, **kw):
    from goldsrl import _ffi
    kw.setdefault("max_episode_steps", 128)
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=seed, **kw)
    eng.reset()
    return eng


def _state(eng):
    return {f: eng.get_state(f) for f in FIELDS}


def _same(got, want, keys=SAME, upto=None):
    """bytes; upto: per-env lengths -- the step rows are then compared up to each env's end only"""
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if upto is not None and k in ("rewards", "actions"):
            for e, n in enumerate(upto):
                assert got[k][e, :n].tobytes() == want[k][e, :n].tobytes(), (k, e)
        else:
            assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])


def _plan_then_host(eng, rules, H, K, S, trace_env=None):
    """the one call first -- it leaves the handle as it was --, then the host composition on the same engine, which advances it"""
    from goldsrl import _ffi_swarmplan as P
    before = {f: eng.get_state(f).tobytes() for f in FIELDS}
    got = P.swarm_plan(eng, rules, H, K, S, keep_actions=True, trace_env=trace_env)
    assert {f: eng.get_state(f).tobytes() for f in FIELDS} == before
    want = P.swarm_plan_host(eng, rules, H, K, S, keep_actions=True, trace_env=trace_env)
    return got, want


@pytest.mark.parametrize("n_rules", [1, 3])
@pytest.mark.parametrize("E", [1, 3, 4, 5, 9])
def test_the_one_call_is_the_host_composition(E, n_rules):
    for H, K, S in HKS:
        eng = _engine(E)
        got, want = _plan_then_host(eng, RULES[:n_rules], H, K, S, trace_env=E // 2)
        D = (S + K - 1) // K
        assert got["rewards"].shape == (E, S) and got["choices"].shape == (E, D) and got["scores"].shape == (E, D, n_rules)
        assert got["actions"].shape == (E, S, 10, 2) and got["trace_x"].shape == (S, 80, 2) and got["trace_xa"].shape == (S, 10, 2)
        assert (got["length"] == S).all() and not got["finished"].any() and (got["rewards"] < 0).all() and (got["choices"] >= 0).all()
        assert np.array_equal(got["totals"], got["rewards"].sum(-1))
        _same(got, want, SAME + ("trace_x", "trace_xa"))
        eng.close()


def _fixture_engine(golden):
    g = golden("swarm_rules")
    eng = _engine(1, seed=1)
    for f, k in (("SWARM_X", "x"), ("SWARM_XA", "xa"), ("SWARM_PNOISE", "particle_noise_row"), ("SWARM_ANOISE", "agent_noise_row")):
        eng.set_state(f, np.ascontiguousarray(g[k][None]))
    return eng, g


@pytest.mark.parametrize("H,K,S,distinct", [(1, 1, 12, 3), (4, 1, 6, 2), (8, 4, 8, 2)])
def test_switching_is_exercised(golden, H, K, S, distinct):
    from goldsrl.baselines import DEFAULT_SWARM_RULES
    eng, _ = _fixture_engine(golden)
    got, want = _plan_then_host(eng, DEFAULT_SWARM_RULES, H, K, S)
    print("(H, K, S) = (%d, %d, %d): choices %s" % (H, K, S, got["choices"][0].tolist()))
    assert len(set(got["choices"][0].tolist())) >= distinct
    _same(got, want)
    eng.close()


def test_ties_go_to_the_first_index():
    from goldsrl import _ffi_swarmplan as P, _ffi_swarmrules as R
    E, S = 5, 6
    eng = _engine(E)
    table = RULES[[0, 1, 0]]                                              # rule 2 is a copy of rule 0
    out = P.swarm_plan(eng, table, 2, 1, S)
    assert out["scores"][:, :, 2].tobytes() == out["scores"][:, :, 0].tobytes()
    assert not (out["choices"] == 2).any() and (out["choices"] == 0).any()
    # the same table with the better of the two first: the copy that wins is again the first
    out = P.swarm_plan(eng, RULES[[0, 0, 1]], 2, 1, S)
    assert not (out["choices"] == 1).any()
    # one rule: every choice is 0 and the run is grl_swarm_rules of that rule over S steps
    for H, K in ((1, 1), (3, 2), (6, 6)):
        one = P.swarm_plan(eng, RULES[1:2], H, K, S, keep_actions=True)
        ref = R.swarm_rules(eng, RULES[1:2], S, keep_actions=True)
        assert not one["choices"].any()
        for k in ("rewards", "actions", "length", "finished"):
            assert one[k].tobytes() == ref[k].tobytes(), (H, K, k)       # (E, 1, ...) against (E, ...): the same bytes
    eng.close()


def test_ends_by_the_time_limit():
    from goldsrl import _ffi_swarmplan as P, _ffi_swarmrules as R
    eng = _engine(4, max_episode_steps=6)
    out = P.swarm_plan(eng, RULES, 4, 4, 10)
    assert (out["length"] == 6).all() and (out["finished"] == 1).all()
    assert (out["rewards"][:, :6] < 0).all() and not out["rewards"][:, 6:].any()
    assert out["choices"].shape == (4, 3) and (out["choices"][:, :2] >= 0).all() and (out["choices"][:, 2] == -1).all()
    assert out["scores"][:, :2].all() and not out["scores"][:, 2].any()
    # the second lookahead starts at step 4 and is cut to the 2 steps the TimeLimit leaves
    got, want = _plan_then_host(eng, RULES, 4, 4, 10)
    _same(got, want, upto=[6] * 4)
    eng.close()

    # ends that differ inside a workgroup and across two: env e has e steps behind it
    E = 5
    eng = _engine(E, max_episode_steps=8)
    eng.set_state("ELAPSED", np.arange(E, dtype=np.int32))
    got, want = _plan_then_host(eng, RULES, 3, 2, 10, trace_env=3)
    assert got["length"].tolist() == [8 - e for e in range(E)] and (got["finished"] == 1).all()
    _same(got, want, upto=got["length"])
    for e in range(E):
        n, d = 8 - e, (8 - e + 1) // 2
        assert not got["rewards"][e, n:].any() and not got["actions"][e, n:].any()
        assert (got["choices"][e, :d] >= 0).all() and (got["choices"][e, d:] == -1).all() and not got["scores"][e, d:].any()
    # env 3 plays 5 steps; the host composition cannot trace the step that ends an episode (the engine has reset the env by then)
    assert got["trace_x"][:4].tobytes() == want["trace_x"][:4].tobytes() and got["trace_xa"][:4].tobytes() == want["trace_xa"][:4].tobytes()
    assert got["trace_x"][4].any() and got["trace_xa"][4].any() and not got["trace_x"][5:].any() and not got["trace_xa"][5:].any()
    eng.close()

    # the lookahead is cut by the TimeLimit, not by max_steps: one step is played, three are looked ahead
    eng = _engine(3)
    out = P.swarm_plan(eng, RULES, 3, 1, 1)
    look = R.swarm_rules(eng, RULES, 3)
    want = np.zeros((3, 3))
    for t in range(3):
        want = want + look["rewards"][:, :, t]
    assert out["scores"][:, 0].tobytes() == want.tobytes() and (out["length"] == 1).all() and not out["finished"].any()
    eng.close()


def test_dynamics_are_the_replay_of_the_kept_actions():
    from goldsrl import _ffi_replay, _ffi_swarmplan as P
    E, S = 5, 7
    eng = _engine(E)
    out = P.swarm_plan(eng, RULES, 3, 2, S, keep_actions=True, trace_env=4)
    rep = _ffi_replay.swarm_replay(eng, out["actions"].reshape(E, 1, S, 10, 2), trace_env=4)
    for k in ("rewards", "length", "finished", "trace_x", "trace_xa"):
        assert rep[k].dtype == out[k].dtype and rep[k].tobytes() == out[k].tobytes(), k
    eng.close()


def test_the_handle_is_read_only():
    from goldsrl import _ffi_swarmplan as P
    E = 5
    eng, other = _engine(E), _engine(E)
    first = np.ascontiguousarray(np.random.RandomState(1).normal(size=(E, 10, 2)).astype(np.float32) * 0.5)
    eng.step(first); other.step(first)          # so that the outputs hold something
    before = {f: eng.get_state(f).tobytes() for f in FIELDS}
    outs = {o: eng.read(o).tobytes() for o in OUTPUTS}
    P.swarm_plan(eng, RULES, 3, 2, 5, keep_actions=True, trace_env=2)
    P.swarm_plan(eng, RULES[:1], 1, 1, 3)
    assert {f: eng.get_state(f).tobytes() for f in FIELDS} == before
    assert {o: eng.read(o).tobytes() for o in OUTPUTS} == outs
    nxt = np.ascontiguousarray(np.random.RandomState(4).normal(size=(E, 10, 2)).astype(np.float32) * 0.5)
    eng.step(nxt); other.step(nxt)              # `other` never planned
    for f in FIELDS:
        assert eng.get_state(f).tobytes() == other.get_state(f).tobytes(), f
    for o in OUTPUTS:
        assert eng.read(o).tobytes() == other.read(o).tobytes(), o
    eng.close(); other.close()


@pytest.mark.parametrize("kind", ["fast", "refdiv"])
def test_the_math_mode_selects_the_step_only(kind, monkeypatch):
    from goldsrl import _ffi, _ffi_replay
    if kind == "refdiv":
        monkeypatch.setenv("GRL_SWARM_DIV", "ref")                   # read at grl_create
    E, S = 5, 6
    eng = _engine(E, flags=_ffi.F_SWARM_FAST_MATH if kind == "fast" else 0)
    got, want = _plan_then_host(eng, RULES, 3, 2, S, trace_env=4)
    _same(got, want, SAME + ("trace_x", "trace_xa"))
    eng.reset()
    from goldsrl import _ffi_swarmplan as P
    out = P.swarm_plan(eng, RULES, 3, 2, S, keep_actions=True, trace_env=4)
    rep = _ffi_replay.swarm_replay(eng, out["actions"].reshape(E, 1, S, 10, 2), trace_env=4)
    for k in ("rewards", "length", "finished", "trace_x", "trace_xa"):
        assert rep[k].tobytes() == out[k].tobytes(), k
    eng.close()


def test_error_paths():
    from goldsrl import _ffi, _ffi_swarmplan as P, _ffi_swarmrules as R
    lib = _ffi.load_library(extra_signatures=P.SWARMPLAN_SIGNATURES)
    head, off = np.ascontiguousarray(RULES[:, :3]), np.ascontiguousarray(R.swarm_rule_offsets(RULES))
    S = 6

    def call(h, head=head, off=off, n=3, H=3, K=2, steps=S, keep=0, trace=-1):
        return lib.grl_swarm_plan(h, _ffi._ptr(head), _ffi._ptr(off), n, H, K, steps, keep, trace)

    solow = _ffi.Engine(_ffi.ENV_SOLOW, 2, seed=1)
    solow.reset()
    with pytest.raises(ValueError):
        P.swarm_plan(solow, RULES, 3, 2, S)
    assert call(solow.h) == _ffi.E_INVALID and b"not a Swarm handle" in lib.grl_last_error(solow.h)
    solow.close()

    eng = _engine(2)
    buf = np.zeros((2, S))
    assert lib.grl_swarm_plan_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE        # before any run
    assert call(eng.h, K=4) == _ffi.E_INVALID and b"replan" in lib.grl_last_error(eng.h)                 # replan > horizon
    assert call(eng.h, K=0) == _ffi.E_INVALID and b"replan" in lib.grl_last_error(eng.h)
    assert call(eng.h, H=0, K=0) == _ffi.E_INVALID and call(eng.h, steps=0) == _ffi.E_INVALID
    assert call(eng.h, n=0) == _ffi.E_INVALID
    assert call(eng.h, np.zeros((4097, 3)), np.zeros((4097, 10, 2)), n=4097) == _ffi.E_INVALID
    assert call(eng.h, trace=2) == _ffi.E_INVALID and call(eng.h, trace=-2) == _ffi.E_INVALID
    bad = head.copy(); bad[1, 2] = 2.0
    assert call(eng.h, bad) == _ffi.E_INVALID and b"anchor" in lib.grl_last_error(eng.h)
    bad = head.copy(); bad[2, 1] = np.inf
    assert call(eng.h, bad) == _ffi.E_INVALID
    bad = off.copy(); bad[2, 9, 1] = np.nan
    assert call(eng.h, off=bad) == _ffi.E_INVALID and b"offset" in lib.grl_last_error(eng.h)
    assert lib.grl_swarm_plan(eng.h, None, _ffi._ptr(off), 3, 3, 2, S, 0, -1) == _ffi.E_INVALID
    assert lib.grl_swarm_plan(eng.h, _ffi._ptr(head), None, 3, 3, 2, S, 0, -1) == _ffi.E_INVALID
    assert lib.grl_swarm_plan_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE        # a refused call is no run
    for H, K in ((2, 3), (3, 0)):
        with pytest.raises(ValueError):
            P.swarm_plan(eng, RULES, H, K, S)                                # the host check, before the C ABI
    assert call(eng.h) == _ffi.OK                                            # no actions kept, no trace
    act, tx, txa = np.zeros((2, S, 10, 2)), np.zeros((S, 80, 2)), np.zeros((S, 10, 2))
    ch, sc = np.zeros((2, 3), np.int32), np.zeros((2, 3, 3))
    assert lib.grl_swarm_plan_read(eng.h, b"actions", _ffi._ptr(act), act.nbytes) == _ffi.E_STATE
    assert lib.grl_swarm_plan_read(eng.h, b"trace_x", _ffi._ptr(tx), tx.nbytes) == _ffi.E_STATE
    assert lib.grl_swarm_plan_read(eng.h, b"trace_xa", _ffi._ptr(txa), txa.nbytes) == _ffi.E_STATE
    assert lib.grl_swarm_plan_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes - 8) == _ffi.E_SIZE
    assert lib.grl_swarm_plan_read(eng.h, b"choices", _ffi._ptr(ch), ch.nbytes + 4) == _ffi.E_SIZE
    assert lib.grl_swarm_plan_read(eng.h, b"scores", _ffi._ptr(sc), sc.nbytes - 8) == _ffi.E_SIZE
    assert lib.grl_swarm_plan_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes) == _ffi.OK and (buf < 0).all()
    assert lib.grl_swarm_plan_read(eng.h, b"choices", _ffi._ptr(ch), ch.nbytes) == _ffi.OK and (ch >= 0).all()
    assert lib.grl_swarm_plan_read(eng.h, b"nothing", _ffi._ptr(buf), buf.nbytes) == _ffi.E_INVALID
    assert call(eng.h, keep=1, trace=1) == _ffi.OK
    assert lib.grl_swarm_plan_read(eng.h, b"actions", _ffi._ptr(act), act.nbytes) == _ffi.OK
    assert lib.grl_swarm_plan_read(eng.h, b"trace_x", _ffi._ptr(tx), tx.nbytes) == _ffi.OK
    eng.step_async(np.zeros((2, 10, 2), np.float32))                         # a step in flight
    assert call(eng.h) == _ffi.E_INVALID and b"in flight" in lib.grl_last_error(eng.h)
    eng.wait()
    eng.close()


def test_the_reference_fixture(golden):
    """The planner over the default rules on the reset state of the reference's SwarmEnv(seed=192), 128 steps, against what the same
    scheme gave on the unmodified reference env in numpy (tests/golden/swarm_plan.npz).  The generator asserts every gap between the
    best and the second score to be at least 1e-6 relative, so the choices are compared exactly.  Bounds: those of
    test_gpu_swarm_rules.py:test_the_reference_fixture -- rewards rtol 1e-9, totals rtol 1e-10."""
    from goldsrl.baselines import SwarmRulePlanner
    eng, rules_fixture = _fixture_engine(golden)
    g = golden("swarm_plan")
    best_fixed = rules_fixture["total"].max()
    assert best_fixed == float(g["best_fixed_total"])
    for H, K in g["cases"].tolist():
        b = SwarmRulePlanner(eng, g["rules"], H, K)
        out = b.run()
        key = lambda name: g["%s_%d_%d" % (name, H, K)]
        rel = np.abs(out["rewards"][0] - key("rewards")) / np.abs(key("rewards"))
        print("(H, K) = (%d, %d): total %.12f against %.12f, relative %.3g; largest relative reward error %.3g; %d switches; smallest gap %.3g"
              % (H, K, out["totals"][0], float(key("total")), abs(out["totals"][0] - key("total")) / abs(key("total")), rel.max(),
                 b.switches(), key("gaps").min()))
        assert out["length"][0] == int(key("length")) == 128 and out["finished"][0] == 1
        assert np.array_equal(out["choices"][0], key("choices"))
        np.testing.assert_allclose(out["rewards"][0], key("rewards"), rtol=1e-9)
        np.testing.assert_allclose(out["totals"][0], key("total"), rtol=1e-10)
        assert b.total() == out["totals"][0] and b.total() - best_fixed > 10
    eng.close()


@pytest.fixture(scope="module")
def monitor(tmp_path_factory):
    from goldsrl import envs, _ffi
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import ConvSingleAgentPolicyNetwork
    from goldsrl.agents.state_processors import SwarmStateProcessor
    conf = dict(name='local_learning', num_actions=2, clip_norm=40.0, clip_norm_type='global', device='/gpu:0',
                entropy_regularisation_strength=0.02, scale=1000.0, height=84, width=84, channels=3)
    d = tmp_path_factory.mktemp("plan")
    learner_eng = _ffi.Engine(_ffi.ENV_SWARM, 2, seed=5)
    learner_eng.reset()
    global_net = ConvSingleAgentPolicyNetwork(conf).bind(learner_eng, seed=11)
    mon = PM.SwarmPolicyMonitor(envs.make("Swarm-eval-v0"), global_net, SwarmStateProcessor(grid_size=84), PM.ScalarWriter(str(d / "eval")),
                                network_conf=conf)
    mon.actions_path = str(d / "swarm-eval.json")
    mon.tmp = d
    return mon


def test_monitor_plan_baseline(monitor, capsys):
    from goldsrl.baselines import SwarmRulePlanner
    from goldsrl.scripts import make_swarm_gif
    monitor.env.reset()
    fresh = _state(monitor.env._eng)
    _, rule_total = monitor.rule_baseline()
    name, total = monitor.plan_baseline()                                    # after the rule baseline: the plan is the one kept
    after = _state(monitor.env._eng)
    for f in FIELDS:
        if f != "EPISODE":                                                   # every reset starts a new episode
            assert after[f].tobytes() == fresh[f].tobytes(), f
    st = monitor.baseline_stats
    assert st["rewards"].shape == (1, 128) and st["choices"].shape == (1, 32) and st["length"][0] == 128
    assert total == monitor.baseline_total_reward == st["totals"][0] and name == monitor.baseline_name and name.startswith("plan (horizon 8, replan 4")
    assert total > rule_total
    b = SwarmRulePlanner(monitor.env._eng)                                   # the env is reset: the same episode
    assert b.total() == total and b.switches() >= 1
    # the planned episode played by the monitor, step by step: the same score, the scalars beside it, and a file that replays
    q = queue.Queue()
    for a in st["actions"][0]:
        q.put(a)
    played, length, _ = monitor.eval_once(actions=q)
    assert length == 128 and played == total
    rows = [json.loads(line) for line in open(monitor.summary_writer.get_logdir() + "/scalars.jsonl")]
    last = {r["tag"]: r["value"] for r in rows}
    assert last["eval/baseline_total_reward"] == total and last["eval/total_reward_minus_baseline"] == 0.0
    assert json.load(open(monitor.actions_path))["score"] == total
    got, score = make_swarm_gif.main(["--actions", monitor.actions_path, "--no-gif"])
    printed = capsys.readouterr().out
    assert "score reproduced" in printed and "score differs" not in printed and got == score == total


def test_the_script_keeps_the_planned_episode(tmp_path, capsys):
    from goldsrl.scripts import make_swarm_gif, swarm_rules
    path = str(tmp_path / "plan.json")
    best, six, score = swarm_rules.main(["--plan", "8:4", "--json", path])
    printed = capsys.readouterr().out
    assert "plan: horizon 8, replan 4" in printed
    kept = json.load(open(path))
    assert kept["score"] == score and len(kept["actions"]) == 128
    make_swarm_gif.main(["--actions", path, "--no-gif"])
    printed = capsys.readouterr().out
    assert "score reproduced" in printed and "score differs" not in printed
