"""GPU: feedback rules on the Swarm env, whole episodes in one launch (include/goldsrl_swarmrules.h, csrc/swarm_rules.hip).  The
rule's arithmetic is held to its numpy restatement (goldsrl/_ffi_swarmrules.py:swarm_rule_actions) as bits, the dynamics to the
replay of the kept actions on the same handle (both run block_step of csrc/swarm_dev.h) as bytes; only the case that holds the
kernel to the unmodified reference's fixture has tolerances (those of tests/test_gpu_swarm_replay.py's fixture case)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("SWARM_X", "SWARM_XA", "SWARM_PNOISE", "SWARM_ANOISE", "ELAPSED", "EPISODE")
OUTPUTS = ("reward", "reward_f64", "done", "elapsed", "locust_bins", "agent_bins", "positions", "done_count")
T = 6

# (cancel, gain, anchor, off_x, off_y, radius): a centroid rule with a ring whose raw action is longer than 1 for the agents far from
# their place and shorter for the near ones; a nearest-locust rule that saturates; a nearest-locust rule with a ring and half the
# wind cancelled
RULES = np.array([(0, 1.5, 0, 0.1, 0.2, 0.5), (1, 5, 1, 0.3, -0.3, 0), (0.5, 2, 1, 0, 0, 0.2)], np.float64)


def _engine(E, seed=7, **kw):
    from goldsrl import _ffi
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=seed, **kw)
    eng.reset()
    return eng


def _state(eng):
    return {f: eng.get_state(f) for f in FIELDS}


@pytest.fixture(scope="module")
def runs():
    """(E, n_rules) -> (engine, its state before the run, the run's outputs with the actions kept and the middle env traced); one
    launch per key, shared by the arithmetic and the dynamics tests"""
    from goldsrl import _ffi_swarmrules as R
    made = {}

    def get(E, n):
        if (E, n) not in made:
            eng = _engine(E, max_episode_steps=128)
            st = _state(eng)
            made[(E, n)] = (eng, st, R.swarm_rules(eng, RULES[:n], T, keep_actions=True, trace_env=E // 2))
        return made[(E, n)]
    yield get
    for eng, _, _ in made.values():
        eng.close()


@pytest.mark.parametrize("n_rules", [1, 3])
@pytest.mark.parametrize("E", [1, 3, 4, 5, 9])
def test_rule_arithmetic_is_the_numpy_statements(runs, E, n_rules):
    from goldsrl import _ffi_swarmrules as R
    eng, st, out = runs(E, n_rules)
    mid = E // 2
    assert out["rewards"].shape == (E, n_rules, T) and out["actions"].shape == (E, n_rules, T, 10, 2)
    assert out["trace_x"].shape == (n_rules, T, 80, 2) and out["trace_xa"].shape == (n_rules, T, 10, 2)
    assert (out["length"] == T).all() and not out["finished"].any()
    assert np.array_equal(out["totals"], out["rewards"].sum(-1)) and np.isfinite(out["rewards"]).all() and (out["rewards"] < 0).all()
    for r in range(n_rules):
        for t in range(T):
            x = st["SWARM_X"][mid] if t == 0 else out["trace_x"][r, t - 1]
            xa = st["SWARM_XA"][mid] if t == 0 else out["trace_xa"][r, t - 1]
            want = R.swarm_rule_actions(x, xa, RULES[r], out["offsets"][r])
            assert out["actions"][mid, r, t].tobytes() == want.tobytes(), (r, t)
    # every env's first action, not only the traced one's
    for e in range(E):
        for r in range(n_rules):
            want = R.swarm_rule_actions(st["SWARM_X"][e], st["SWARM_XA"][e], RULES[r], out["offsets"][r])
            assert out["actions"][e, r, 0].tobytes() == want.tobytes(), (e, r)
    # rule 0 clips some agents and leaves others: both branches of the clip ran
    norms = np.sqrt((out["actions"][mid, 0] ** 2).sum(-1))
    assert (norms < 0.99).any() and (np.abs(norms - 1.0) < 1e-12).any(), norms


@pytest.mark.parametrize("n_rules", [1, 3])
@pytest.mark.parametrize("E", [1, 3, 4, 5, 9])
def test_dynamics_are_the_replay_of_the_kept_actions(runs, E, n_rules):
    from goldsrl import _ffi_replay
    eng, st, out = runs(E, n_rules)
    rep = _ffi_replay.swarm_replay(eng, out["actions"], trace_env=E // 2)          # per-env rows (E, n_rules, T, 10, 2)
    for k in ("rewards", "length", "finished", "trace_x", "trace_xa"):
        assert rep[k].dtype == out[k].dtype and rep[k].tobytes() == out[k].tobytes(), k


@pytest.mark.parametrize("kind", ["fast", "refdiv"])
def test_the_math_mode_selects_the_step_only(kind, monkeypatch):
    from goldsrl import _ffi, _ffi_replay, _ffi_swarmrules as R
    if kind == "refdiv":
        monkeypatch.setenv("GRL_SWARM_DIV", "ref")                   # read at grl_create
    E = 5
    eng = _engine(E, max_episode_steps=128, flags=_ffi.F_SWARM_FAST_MATH if kind == "fast" else 0)
    st = _state(eng)
    out = R.swarm_rules(eng, RULES, T, keep_actions=True, trace_env=4)
    for r in range(len(RULES)):
        for t in range(T):
            x = st["SWARM_X"][4] if t == 0 else out["trace_x"][r, t - 1]
            xa = st["SWARM_XA"][4] if t == 0 else out["trace_xa"][r, t - 1]
            assert out["actions"][4, r, t].tobytes() == R.swarm_rule_actions(x, xa, RULES[r], out["offsets"][r]).tobytes(), (r, t)
    rep = _ffi_replay.swarm_replay(eng, out["actions"], trace_env=4)
    for k in ("rewards", "length", "finished", "trace_x", "trace_xa"):
        assert rep[k].tobytes() == out[k].tobytes(), k
    eng.close()


def test_drift_and_hold_are_the_scripted_baseline():
    from goldsrl.baselines import DEFAULT_SWARM_RULES, ScriptedSwarmBaseline, SwarmRuleBaseline
    E = 3
    eng = _engine(E, max_episode_steps=T)
    old = ScriptedSwarmBaseline(eng).run()
    b = SwarmRuleBaseline(eng, DEFAULT_SWARM_RULES[:4])
    new = b.run(keep_actions=True)
    assert new["rewards"][:, :2].tobytes() == old["rewards"].tobytes()
    assert np.array_equal(new["length"][:, :2], old["length"]) and np.array_equal(new["finished"][:, :2], old["finished"])
    assert (new["length"] == T).all() and new["finished"].all()             # the engine's TimeLimit is T
    assert not new["actions"][:, 0].any() and (new["actions"][:, 1] == [-1.0, 0.0]).all()
    i, six, total = b.best_total()
    assert total == new["totals"].mean(axis=0).max() and six == tuple(DEFAULT_SWARM_RULES[i])
    eng.close()


def test_time_limit_ends_differ_inside_one_workgroup():
    from goldsrl import _ffi_replay, _ffi_swarmrules as R
    eng = _engine(4, max_episode_steps=4)
    out = R.swarm_rules(eng, RULES[:1], T)                                  # elapsed 0 everywhere
    assert (out["length"] == 4).all() and (out["finished"] == 1).all() and not out["rewards"][:, :, 4:].any()
    assert (out["rewards"][:, :, :4] < 0).all()
    eng.set_state("ELAPSED", np.array([0, 2, 3, 1], np.int32))
    out = R.swarm_rules(eng, RULES[:1], T, keep_actions=True, trace_env=1)
    assert out["length"].tolist() == [[4], [2], [1], [3]] and (out["finished"] == 1).all()
    for e, n in enumerate((4, 2, 1, 3)):
        assert (out["rewards"][e, 0, :n] < 0).all() and not out["rewards"][e, 0, n:].any() and not out["actions"][e, 0, n:].any()
    assert not out["trace_x"][0, 2:].any() and not out["trace_xa"][0, 2:].any() and out["trace_x"][0, :2].any()
    rep = _ffi_replay.swarm_replay(eng, out["actions"], trace_env=1)         # the replay ends its pairs by the same TimeLimit
    for k in ("rewards", "length", "finished", "trace_x", "trace_xa"):
        assert rep[k].tobytes() == out[k].tobytes(), k
    # two rules per env: an env's pairs straddle workgroups, the ends follow the env
    out = R.swarm_rules(eng, RULES[:2], T)
    assert out["length"].tolist() == [[4, 4], [2, 2], [1, 1], [3, 3]] and (out["finished"] == 1).all()
    eng.close()


def test_the_handle_is_read_only():
    from goldsrl import _ffi_swarmrules as R
    E = 5
    eng, other = _engine(E, max_episode_steps=128), _engine(E, max_episode_steps=128)
    first = np.ascontiguousarray(np.random.RandomState(1).normal(size=(E, 10, 2)).astype(np.float32) * 0.5)
    eng.step(first); other.step(first)          # so that the outputs hold something
    before = {f: eng.get_state(f).tobytes() for f in FIELDS}
    outs = {o: eng.read(o).tobytes() for o in OUTPUTS}
    R.swarm_rules(eng, RULES, 5, keep_actions=True, trace_env=2)
    R.swarm_rules(eng, RULES[:1], 3)
    assert {f: eng.get_state(f).tobytes() for f in FIELDS} == before
    assert {o: eng.read(o).tobytes() for o in OUTPUTS} == outs
    nxt = np.ascontiguousarray(np.random.RandomState(4).normal(size=(E, 10, 2)).astype(np.float32) * 0.5)
    eng.step(nxt); other.step(nxt)              # `other` never played a rule
    for f in FIELDS:
        assert eng.get_state(f).tobytes() == other.get_state(f).tobytes(), f
    for o in OUTPUTS:
        assert eng.read(o).tobytes() == other.read(o).tobytes(), o
    eng.close(); other.close()


def test_error_paths():
    from goldsrl import _ffi, _ffi_swarmrules as R
    lib = _ffi.load_library(extra_signatures=R.SWARMRULES_SIGNATURES)
    head, off = np.ascontiguousarray(RULES[:, :3]), np.ascontiguousarray(R.swarm_rule_offsets(RULES))

    def call(h, head=head, off=off, n=3, steps=T, keep=0, trace=-1):
        return lib.grl_swarm_rules(h, _ffi._ptr(head), _ffi._ptr(off), n, steps, keep, trace)

    solow = _ffi.Engine(_ffi.ENV_SOLOW, 2, seed=1)
    solow.reset()
    with pytest.raises(ValueError):
        R.swarm_rules(solow, RULES, T)
    assert call(solow.h) == _ffi.E_INVALID and b"not a Swarm handle" in lib.grl_last_error(solow.h)
    solow.close()

    eng = _engine(2, max_episode_steps=128)
    buf = np.zeros((2, 3, T))
    assert lib.grl_swarm_rules_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE       # before any run
    big_head, big_off = np.zeros((4097, 3)), np.zeros((4097, 10, 2))
    assert call(eng.h, n=0) == _ffi.E_INVALID
    assert call(eng.h, big_head, big_off, n=4097) == _ffi.E_INVALID
    assert call(eng.h, steps=0) == _ffi.E_INVALID
    assert call(eng.h, trace=2) == _ffi.E_INVALID and call(eng.h, trace=-2) == _ffi.E_INVALID
    bad = head.copy(); bad[1, 2] = 2.0
    assert call(eng.h, bad) == _ffi.E_INVALID and b"anchor" in lib.grl_last_error(eng.h)
    bad = head.copy(); bad[2, 1] = np.inf
    assert call(eng.h, bad) == _ffi.E_INVALID
    bad = off.copy(); bad[2, 9, 1] = np.nan
    assert call(eng.h, off=bad) == _ffi.E_INVALID and b"offset" in lib.grl_last_error(eng.h)
    assert lib.grl_swarm_rules(eng.h, None, _ffi._ptr(off), 3, T, 0, -1) == _ffi.E_INVALID
    assert lib.grl_swarm_rules(eng.h, _ffi._ptr(head), None, 3, T, 0, -1) == _ffi.E_INVALID
    assert lib.grl_swarm_rules_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE       # a refused call is no run
    with pytest.raises(ValueError):
        R.swarm_rules(eng, [(1, 5, 2, 0, 0, 0)], T)                        # the host check, before the C ABI
    assert call(eng.h) == _ffi.OK                                          # no actions kept, no trace
    act, tx = np.zeros((2, 3, T, 10, 2)), np.zeros((3, T, 80, 2))
    assert lib.grl_swarm_rules_read(eng.h, b"actions", _ffi._ptr(act), act.nbytes) == _ffi.E_STATE
    assert lib.grl_swarm_rules_read(eng.h, b"trace_x", _ffi._ptr(tx), tx.nbytes) == _ffi.E_STATE
    assert lib.grl_swarm_rules_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes - 8) == _ffi.E_SIZE
    assert lib.grl_swarm_rules_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes) == _ffi.OK and (buf < 0).all()
    assert lib.grl_swarm_rules_read(eng.h, b"nothing", _ffi._ptr(buf), buf.nbytes) == _ffi.E_INVALID
    assert call(eng.h, keep=1, trace=1) == _ffi.OK
    assert lib.grl_swarm_rules_read(eng.h, b"actions", _ffi._ptr(act), act.nbytes) == _ffi.OK
    assert lib.grl_swarm_rules_read(eng.h, b"trace_x", _ffi._ptr(tx), tx.nbytes) == _ffi.OK
    eng.step_async(np.zeros((2, 10, 2), np.float32))                       # a step in flight
    assert call(eng.h) == _ffi.E_INVALID and b"in flight" in lib.grl_last_error(eng.h)
    eng.wait()
    eng.close()


def test_the_reference_fixture(golden):
    """The default rules on the reset state of the reference's SwarmEnv(seed=192), 128 steps, against the rewards the unmodified
    reference gave under the same rule in numpy (tests/golden/swarm_rules.npz).  Bounds: those of
    test_gpu_swarm_replay.py:test_the_references_seed_192_episode -- rewards rtol 1e-9, totals rtol 1e-10."""
    from goldsrl import _ffi
    from goldsrl.baselines import SwarmRuleBaseline
    g = golden("swarm_rules")
    eng = _ffi.Engine(_ffi.ENV_SWARM, 1, seed=1, max_episode_steps=128)
    eng.reset()
    for f, k in (("SWARM_X", "x"), ("SWARM_XA", "xa"), ("SWARM_PNOISE", "particle_noise_row"), ("SWARM_ANOISE", "agent_noise_row")):
        eng.set_state(f, np.ascontiguousarray(g[k][None]))
    b = SwarmRuleBaseline(eng, g["rules"])
    out = b.run(keep_actions=True)
    assert out["rewards"].shape == (1, len(g["rules"]), 128)
    assert np.array_equal(out["length"][0], g["length"]) and (out["finished"] == 1).all()
    assert np.array_equal(out["offsets"], g["offsets"])
    rel = np.abs(out["rewards"][0] - g["rewards"]) / np.abs(g["rewards"])
    trel = np.abs(out["totals"][0] - g["total"]) / np.abs(g["total"])
    for r in range(len(g["rules"])):
        print("rule %2d: largest relative reward error %.3g (step %d), total %.12f against %.12f, relative %.3g, largest action difference %.3g"
              % (r, rel[r].max(), int(rel[r].argmax()), out["totals"][0, r], g["total"][r], trel[r],
                 np.abs(out["actions"][0, r] - g["actions"][r]).max()))
    np.testing.assert_allclose(out["rewards"][0], g["rewards"], rtol=1e-9)
    np.testing.assert_allclose(out["totals"][0], g["total"], rtol=1e-10)
    i, six, total = b.best_total()
    assert i == int(g["best_index"]) and six == tuple(g["rules"][i]) and total == out["totals"][0, i]
    assert total - out["totals"][0, 1] > 100                                 # far above hold
    eng.close()


@pytest.fixture(scope="module")
def monitor(tmp_path_factory):
    from goldsrl import envs, _ffi
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import ConvSingleAgentPolicyNetwork
    from goldsrl.agents.state_processors import SwarmStateProcessor
    conf = dict(name='local_learning', num_actions=2, clip_norm=40.0, clip_norm_type='global', device='/gpu:0',
                entropy_regularisation_strength=0.02, scale=1000.0, height=84, width=84, channels=3)
    d = tmp_path_factory.mktemp("rules")
    learner_eng = _ffi.Engine(_ffi.ENV_SWARM, 2, seed=5)
    learner_eng.reset()
    global_net = ConvSingleAgentPolicyNetwork(conf).bind(learner_eng, seed=11)
    mon = PM.SwarmPolicyMonitor(envs.make("Swarm-eval-v0"), global_net, SwarmStateProcessor(grid_size=84), PM.ScalarWriter(str(d / "eval")),
                                network_conf=conf)
    mon.actions_path = str(d / "swarm-eval.json")
    return mon


def test_monitor_rule_baseline(monitor):
    from goldsrl.baselines import DEFAULT_SWARM_RULES
    monitor.env.reset()
    fresh = _state(monitor.env._eng)
    old_name, old_total = monitor.baseline()
    name, total = monitor.rule_baseline()
    after = _state(monitor.env._eng)
    for f in FIELDS:
        if f != "EPISODE":                                                   # every reset starts a new episode
            assert after[f].tobytes() == fresh[f].tobytes(), f
    st = monitor.baseline_stats
    assert st["rewards"].shape == (1, len(DEFAULT_SWARM_RULES), 128) and (st["length"] == 128).all()
    i, six = monitor.baseline_rule
    assert total == monitor.baseline_total_reward == st["totals"][0].max() == st["totals"][0, i]
    assert six == tuple(DEFAULT_SWARM_RULES[i]) and name == monitor.baseline_name and name.startswith("rule %d " % i)
    assert total >= old_total                                                # drift and hold are rows 0 and 1 of the set
    assert max(st["totals"][0, 0], st["totals"][0, 1]) == old_total and old_name in ("drift", "hold")
