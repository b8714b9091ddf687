"""GPU: the cross-entropy search over a Swarm rule's five real numbers, every generation in one call
(include/goldsrl_swarmsearch.h, csrc/swarm_search.hip).  The oracle is the same search composed on the host from tested pieces
(goldsrl/_ffi_swarmsearch.py:swarm_search_host: grl_swarm_rules for the episodes, Python loops of float64 adds, a sort, the two
numpy functions of the scheme); every comparison with it is of bytes, over all seven outputs.  Only the case that holds the search
to the unmodified reference's fixture has tolerances."""
import json
import queue

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("SWARM_X", "SWARM_XA", "SWARM_PNOISE", "SWARM_ANOISE", "ELAPSED", "EPISODE")
OUTPUTS = ("reward", "reward_f64", "done", "elapsed", "locust_bins", "agent_bins", "positions", "done_count")
SEVEN = ("candidates", "offsets", "scores", "fit", "order", "mean", "std")
START = (1.0, 5.0, 0.0, -1.5, 1.5, 0.7)                 # the best default rule
# tests/test_gpu_swarm_plan.py's three rules, for the plan that a search must leave alone
RULES = np.array([(0, 1.5, 0, 0.1, 0.2, 0.5), (1, 5, 1, 0.3, -0.3, 0), (0.5, 2, 1, 0, 0, 0.2)], np.float64)
# the fixture's later generations: ten times the largest relative deviation of a fit measured on the device, 2.03e-13 in
# generation 2 (LABNOTES.md); the cap on it is 1e-8, two orders under the 1e-6 gaps the generator asserts
LATER_FIT_RTOL = 2.03e-12


def _engine(E, seed=7, **kw):
    from goldsrl import _ffi
    kw.setdefault("max_episode_steps", 128)
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=seed, **kw)
    eng.reset()
    return eng


def _start(anchor=0.0):
    return START[:2] + (float(anchor),) + START[3:]


def _same(got, want, keys=SEVEN):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    assert got["best_rule"] == want["best_rule"] and got["best_fit"] == want["best_fit"]
    assert got["best_per_generation"].tobytes() == want["best_per_generation"].tobytes()


def _search_then_host(eng, start, **kw):
    """the one call, then the host composition on the same engine; neither advances it"""
    from goldsrl import _ffi_swarmsearch as S
    before = {f: eng.get_state(f).tobytes() for f in FIELDS}
    got = S.swarm_search(eng, start, **kw)
    assert {f: eng.get_state(f).tobytes() for f in FIELDS} == before
    want = S.swarm_search_host(eng, start, **kw)
    assert {f: eng.get_state(f).tobytes() for f in FIELDS} == before
    return got, want


@pytest.mark.parametrize("C,K", [(2, 1), (5, 2), (5, 5), (70, 8)])
@pytest.mark.parametrize("E", [1, 3, 4, 5, 9])
def test_the_one_call_is_the_host_composition(E, C, K):
    G, S = 3, 5
    eng = _engine(E)
    for anchor in (0, 1):
        got, want = _search_then_host(eng, _start(anchor), generations=G, candidates=C, elites=K, seed=E * 100 + C, max_steps=S)
        assert got["candidates"].shape == (G, C, 6) and got["offsets"].shape == (G, C, 10, 2) and got["scores"].shape == (E, G, C)
        assert got["fit"].shape == (G, C) and got["order"].shape == (G, C) and got["order"].dtype == np.int32
        assert got["mean"].shape == got["std"].shape == (G + 1, 5)
        assert (got["candidates"][:, :, 2] == anchor).all() and (got["candidates"][:, :, 0] == 1.0).all() and (got["scores"] < 0).all()
        assert (np.sort(got["order"], axis=1) == np.arange(C)).all()
        _same(got, want)
    eng.close()


def test_the_cap_of_candidates():
    eng = _engine(1)
    got, want = _search_then_host(eng, _start(), generations=2, candidates=1024, elites=64, seed=3, max_steps=2)
    assert (np.sort(got["order"], axis=1) == np.arange(1024)).all()
    _same(got, want)
    eng.close()


def test_the_incumbent_is_kept():
    from goldsrl import _ffi_swarmsearch as S
    eng = _engine(3)
    G = 5
    out = S.swarm_search(eng, _start(), generations=G, candidates=8, elites=3, seed=11, max_steps=6)
    for g in range(G - 1):
        first = out["order"][g, 0]
        assert out["candidates"][g + 1, 0].tobytes() == out["candidates"][g, first].tobytes(), g
        assert out["offsets"][g + 1, 0].tobytes() == out["offsets"][g, first].tobytes(), g
        assert out["fit"][g + 1, 0].tobytes() == out["fit"][g, first].tobytes(), g
        assert out["scores"][:, g + 1, 0].tobytes() == out["scores"][:, g, first].tobytes(), g
    assert (np.diff(out["best_per_generation"]) >= 0).all()
    assert out["candidates"][0, 0].tobytes() == np.array(START).tobytes()              # generation 0's is the start
    assert out["best_rule"] == tuple(out["candidates"][G - 1, out["order"][G - 1, 0]]) and out["best_fit"] == out["fit"][G - 1].max()
    eng.close()


def test_ties_and_fixed_parameters():
    from goldsrl import _ffi_swarmsearch as S
    E, G, C = 5, 3, 6
    eng = _engine(E)
    # two equal rows of normals: equal candidates, equal fits, and the smaller index ranks first
    z = np.random.default_rng(2).standard_normal((G, C, 5))
    z[:, 4] = z[:, 2]
    out = S.swarm_search(eng, _start(), generations=G, candidates=C, elites=2, normals=z, max_steps=5)
    assert out["candidates"][:, 4].tobytes() == out["candidates"][:, 2].tobytes()
    assert out["fit"][:, 4].tobytes() == out["fit"][:, 2].tobytes() and out["scores"][:, :, 4].tobytes() == out["scores"][:, :, 2].tobytes()
    for g in range(G):
        order = out["order"][g].tolist()
        assert order.index(2) + 1 == order.index(4), order
    _same(out, S.swarm_search_host(eng, _start(), generations=G, candidates=C, elites=2, normals=z, max_steps=5))

    # no spread and no floor: every candidate is the start.  Numbers of few bits, whose K-fold sums are exact (goldsrl_swarmsearch.h)
    few_bits = (1.0, 5.0, 1.0, -1.5, 1.5, 0.75)
    zero = np.zeros(5)
    out = S.swarm_search(eng, few_bits, spread=zero, floor=zero, generations=G, candidates=C, elites=3, seed=1, max_steps=5)
    assert out["candidates"].tobytes() == np.tile(np.array(few_bits), (G, C, 1)).tobytes()
    assert (out["order"] == np.arange(C)).all() and not out["std"].any()
    assert out["mean"].tobytes() == np.tile(np.array(few_bits)[[0, 1, 3, 4, 5]], (G + 1, 1)).tobytes()
    assert (out["fit"] == out["fit"][0, 0]).all()
    # the best default rule's 0.7 with two elites: 0.7 + 0.7 is exact as well
    out = S.swarm_search(eng, START, spread=zero, floor=zero, generations=G, candidates=C, elites=2, seed=1, max_steps=5)
    assert (out["order"] == np.arange(C)).all() and not out["std"].any() and out["mean"].tobytes() == np.tile(np.array(START)[[0, 1, 3, 4, 5]], (G + 1, 1)).tobytes()

    # lo = hi pins a parameter whatever the normals; a start outside the box is clamped in mean[0]
    lo, hi = np.array(S.DEFAULT_LO), np.array(S.DEFAULT_HI)
    lo[1] = hi[1] = 6.5
    out = S.swarm_search(eng, (1.0, 50.0, 0.0, -9.0, 1.5, 5.0), lo=lo, hi=hi, generations=G, candidates=C, elites=2, seed=4, max_steps=5)
    assert (out["candidates"][:, :, 1] == 6.5).all() and (out["mean"][:, 1] == 6.5).all()
    assert out["mean"][0].tolist() == [1.0, 6.5, -4.0, 1.5, 3.0] and out["candidates"][0, 0].tolist() == [1.0, 6.5, 0.0, -4.0, 1.5, 3.0]
    five = out["candidates"][:, :, [0, 1, 3, 4, 5]]
    assert (five >= lo).all() and (five <= hi).all()
    _same(out, S.swarm_search_host(eng, (1.0, 50.0, 0.0, -9.0, 1.5, 5.0), lo=lo, hi=hi, generations=G, candidates=C, elites=2, seed=4, max_steps=5))
    eng.close()


def test_episode_ends():
    from goldsrl import _ffi_swarmrules as R
    # every pair ends by the TimeLimit before max_steps
    eng = _engine(4, max_episode_steps=6)
    got, want = _search_then_host(eng, _start(1), generations=2, candidates=5, elites=2, seed=5, max_steps=10)
    _same(got, want)
    played = R.swarm_rules(eng, got["candidates"][1], 10)
    assert (played["length"] == 6).all() and (played["finished"] == 1).all()
    eng.close()

    # ends that differ inside a workgroup and across two: env e has e steps behind it
    E = 5
    eng = _engine(E, max_episode_steps=8)
    eng.set_state("ELAPSED", np.arange(E, dtype=np.int32))
    got, want = _search_then_host(eng, _start(), generations=3, candidates=5, elites=2, seed=6, max_steps=10)
    _same(got, want)
    played = R.swarm_rules(eng, got["candidates"][2], 10)
    assert played["length"].tolist() == [[8 - e] * 5 for e in range(E)]
    sums = np.zeros((E, 5))
    for t in range(10):
        sums = sums + played["rewards"][:, :, t]
    assert got["scores"][:, 2].tobytes() == sums.tobytes()
    eng.close()


def test_scores_are_the_rules_bits():
    from goldsrl import _ffi_swarmrules as R, _ffi_swarmsearch as S
    E, G, C, T = 5, 3, 7, 6
    eng = _engine(E)
    out = S.swarm_search(eng, _start(), generations=G, candidates=C, elites=3, seed=8, max_steps=T)
    for g in range(G):
        played = R.swarm_rules(eng, out["candidates"][g], T)
        assert played["offsets"].tobytes() == out["offsets"][g].tobytes()
        sums = np.zeros((E, C))
        for t in range(T):
            sums = sums + played["rewards"][:, :, t]
        assert out["scores"][:, g].tobytes() == sums.tobytes(), g
    eng.close()


def test_the_handle_is_read_only():
    from goldsrl import _ffi, _ffi_swarmplan as P, _ffi_swarmsearch as S
    from goldsrl._ffi_episode import read_outputs
    E = 5
    eng, other = _engine(E), _engine(E)
    first = np.ascontiguousarray(np.random.RandomState(1).normal(size=(E, 10, 2)).astype(np.float32) * 0.5)
    eng.step(first); other.step(first)          # so that the outputs hold something
    before = {f: eng.get_state(f).tobytes() for f in FIELDS}
    outs = {o: eng.read(o).tobytes() for o in OUTPUTS}
    plan = P.swarm_plan(eng, RULES, 3, 2, 5)
    S.swarm_search(eng, _start(), generations=3, candidates=6, elites=2, max_steps=5)
    S.swarm_search(eng, _start(1), generations=1, candidates=2, elites=1, max_steps=3)
    assert {f: eng.get_state(f).tobytes() for f in FIELDS} == before
    assert {o: eng.read(o).tobytes() for o in OUTPUTS} == outs
    # the plan's result, read again after the searches
    lib = _ffi.load_library(extra_signatures=P.SWARMPLAN_SIGNATURES)
    again = read_outputs(eng, lib.grl_swarm_plan_read, (("rewards", np.float64, (5,)), ("length", np.int32, ()), ("finished", np.uint8, ()),
                                                       ("choices", np.int32, (3,)), ("scores", np.float64, (3, 3))), (E,))
    for k, v in again.items():
        assert v.tobytes() == plan[k].tobytes(), k
    nxt = np.ascontiguousarray(np.random.RandomState(4).normal(size=(E, 10, 2)).astype(np.float32) * 0.5)
    eng.step(nxt); other.step(nxt)              # `other` never searched
    for f in FIELDS:
        assert eng.get_state(f).tobytes() == other.get_state(f).tobytes(), f
    for o in OUTPUTS:
        assert eng.read(o).tobytes() == other.read(o).tobytes(), o
    eng.close(); other.close()


@pytest.mark.parametrize("kind", ["fast", "refdiv"])
def test_the_math_mode_selects_the_step_only(kind, monkeypatch):
    from goldsrl import _ffi
    if kind == "refdiv":
        monkeypatch.setenv("GRL_SWARM_DIV", "ref")                   # read at grl_create
    eng = _engine(5, flags=_ffi.F_SWARM_FAST_MATH if kind == "fast" else 0)
    got, want = _search_then_host(eng, _start(1), generations=3, candidates=6, elites=2, seed=9, max_steps=6)
    _same(got, want)
    eng.close()


def test_error_paths():
    from goldsrl import _ffi, _ffi_swarmsearch as S
    lib = _ffi.load_library(extra_signatures=S.SWARMSEARCH_SIGNATURES)
    G, C, K, T = 2, 4, 2, 3
    good = dict(mean0=np.array([1.0, 5.0, -1.5, 1.5, 0.7]), std0=np.array(S.DEFAULT_SPREAD), floor=np.array(S.DEFAULT_FLOOR),
                lo=np.array(S.DEFAULT_LO), hi=np.array(S.DEFAULT_HI), ring=S.swarm_search_ring(),
                normals=np.random.default_rng(0).standard_normal((G, C, 5)))
    names = ("mean0", "std0", "floor", "lo", "hi", "ring", "normals")

    def call(h, anchor=0, G=G, C=C, K=K, steps=T, **arrays):
        a = dict(good, **arrays)
        ptrs = [None if a[n] is None else _ffi._ptr(a[n]) for n in names]
        return lib.grl_swarm_search(h, anchor, *(ptrs + [G, C, K, steps]))

    def refused(h, word, **kw):
        return call(h, **kw) == _ffi.E_INVALID and word in lib.grl_last_error(h)

    solow = _ffi.Engine(_ffi.ENV_SOLOW, 2, seed=1)
    solow.reset()
    with pytest.raises(ValueError):
        S.swarm_search(solow, START, generations=G, candidates=C, elites=K, max_steps=T)
    assert refused(solow.h, b"not a Swarm handle")
    solow.close()

    eng = _engine(2)
    fit = np.zeros((G, C))
    assert lib.grl_swarm_search_read(eng.h, b"fit", _ffi._ptr(fit), fit.nbytes) == _ffi.E_STATE           # before any run
    for n in names:
        assert refused(eng.h, b"null argument", **{n: None}), n
    assert refused(eng.h, b"anchor", anchor=2) and refused(eng.h, b"anchor", anchor=-1)
    for n in names:                                                                                      # any number that is not finite
        for v in (np.nan, np.inf, -np.inf):
            bad = good[n].copy()
            bad.reshape(-1)[-1] = v
            assert refused(eng.h, n.encode(), **{n: bad}), (n, v)
    bad = good["std0"].copy(); bad[1] = -1e-300
    assert refused(eng.h, b"std0[1] is negative", std0=bad)
    bad = good["floor"].copy(); bad[4] = -1.0
    assert refused(eng.h, b"floor[4] is negative", floor=bad)
    bad = good["lo"].copy(); bad[2] = 4.5
    assert refused(eng.h, b"lo[2] is above hi[2]", lo=bad)
    assert refused(eng.h, b"G must", G=0) and refused(eng.h, b"G must", G=-3)
    assert refused(eng.h, b"C must", C=1) and refused(eng.h, b"C must", C=1025)
    assert refused(eng.h, b"K must", K=0) and refused(eng.h, b"K must", K=C + 1)
    assert refused(eng.h, b"max_steps", steps=0)
    # an output past 2^31 - 1 elements: 2^17 generations of 1 024 candidates are 2^27 offset tables of 20 numbers.  The call is
    # refused on its sizes, before it looks at the normals, which are therefore the small array of the other cases
    assert refused(eng.h, b"does not fit in int32", G=1 << 17, C=1024)
    assert lib.grl_swarm_search_read(eng.h, b"fit", _ffi._ptr(fit), fit.nbytes) == _ffi.E_STATE           # a refused call is no run
    for kw in (dict(generations=0), dict(candidates=1), dict(candidates=1025), dict(elites=0), dict(elites=C + 1), dict(spread=(0, -1, 0, 0, 0)),
               dict(floor=(0, 0, 0, 0, -1)), dict(lo=(0, 0, 5, -4, 0)), dict(normals=np.zeros((G, C, 4))), dict(max_steps=0),
               dict(hi=(1, np.inf, 4, 4, 3))):
        with pytest.raises(ValueError):                                          # the host checks, before the C ABI
            S.swarm_search(eng, START, **dict(dict(generations=G, candidates=C, elites=K, max_steps=T), **kw))
    with pytest.raises(ValueError):
        S.swarm_search(eng, (1, 5, 2, 0, 0, 1), generations=G, candidates=C, elites=K, max_steps=T)       # the anchor
    assert call(eng.h) == _ffi.OK
    shapes = {"candidates": (np.float64, (G, C, 6)), "offsets": (np.float64, (G, C, 10, 2)), "scores": (np.float64, (2, G, C)),
              "fit": (np.float64, (G, C)), "order": (np.int32, (G, C)), "mean": (np.float64, (G + 1, 5)), "std": (np.float64, (G + 1, 5))}
    for name, (dt, shape) in shapes.items():
        a = np.zeros(shape, dt)
        assert lib.grl_swarm_search_read(eng.h, name.encode(), _ffi._ptr(a), a.nbytes - a.itemsize) == _ffi.E_SIZE, name
        assert lib.grl_swarm_search_read(eng.h, name.encode(), _ffi._ptr(a), a.nbytes + a.itemsize) == _ffi.E_SIZE, name
        assert lib.grl_swarm_search_read(eng.h, name.encode(), _ffi._ptr(a), a.nbytes) == _ffi.OK and a.any(), name
    assert lib.grl_swarm_search_read(eng.h, b"nothing", _ffi._ptr(fit), fit.nbytes) == _ffi.E_INVALID
    assert lib.grl_swarm_search_read(eng.h, None, _ffi._ptr(fit), fit.nbytes) == _ffi.E_INVALID
    assert lib.grl_swarm_search_read(eng.h, b"fit", None, fit.nbytes) == _ffi.E_INVALID
    eng.step_async(np.zeros((2, 10, 2), np.float32))                             # a step in flight
    assert refused(eng.h, b"in flight")
    eng.wait()
    assert call(eng.h) == _ffi.OK
    eng.close()


def _fixture_engine(golden):
    g = golden("swarm_rules")
    eng = _engine(1, seed=1)
    for f, k in (("SWARM_X", "x"), ("SWARM_XA", "xa"), ("SWARM_PNOISE", "particle_noise_row"), ("SWARM_ANOISE", "agent_noise_row")):
        eng.set_state(f, np.ascontiguousarray(g[k][None]))
    return eng, g


def test_the_reference_fixture(golden):
    """The search from the best default rule on the reset state of the reference's SwarmEnv(seed=192), 128 steps, 4 generations of 12
    candidates, 4 elites, against what the same scheme gave on the unmodified reference env in numpy (tests/golden/swarm_search.npz),
    with the normals stored there.  Generation 0's candidates are a function of the inputs alone: bytes.  Its fit: rtol 1e-10, the
    bound the rules' and the replay's fixture cases put on a total.  The generator asserts every best-to-second gap and every gap
    across the elite boundary to be at least 1e-6 relative (found: 1.2e-3 and 1.6e-3), so every generation's order[0] and elite set
    are compared exactly.  Later generations' fit: LATER_FIT_RTOL."""
    from goldsrl.baselines import SwarmRuleSearch
    eng, rules_fixture = _fixture_engine(golden)
    g = golden("swarm_search")
    Gn, C, K = (int(v) for v in g["shape"])
    assert g["start"].tobytes() == rules_fixture["rules"][int(rules_fixture["best_index"])].tobytes()
    b = SwarmRuleSearch(eng, g["start"], Gn, C, K, normals=g["normals"])
    out = b.run()
    rel = np.abs(out["fit"] - g["fit"]) / np.abs(g["fit"])
    print("largest relative deviation of a fit from the fixture, per generation: %s; smallest gaps %s"
          % (", ".join("%.3g" % v for v in rel.max(axis=1)), g["gaps"].min(axis=0)))
    print("found %.12f against %.12f; best fixed rule %.12f" % (out["best_fit"], g["fit"][Gn - 1, g["order"][Gn - 1, 0]], float(g["best_fixed_total"])))
    assert out["candidates"][0].tobytes() == g["candidates"][0].tobytes()
    assert out["mean"][0].tobytes() == g["mean"][0].tobytes() and out["std"][0].tobytes() == g["std"][0].tobytes()
    np.testing.assert_allclose(out["fit"][0], g["fit"][0], rtol=1e-10, atol=0)
    for gen in range(Gn):
        assert out["order"][gen, 0] == g["order"][gen, 0], gen
        assert set(out["order"][gen, :K].tolist()) == set(g["order"][gen, :K].tolist()), gen
    np.testing.assert_allclose(out["fit"][1:], g["fit"][1:], rtol=LATER_FIT_RTOL, atol=0)
    six, total = b.best()
    assert total == out["best_fit"] and total - float(g["best_fixed_total"]) > 3
    # the found rule played through swarm_rules is the episode the search scored
    played = b.play_best(keep_actions=True)
    s = np.float64(0.0)
    for t in range(int(played["length"][0, 0])):
        s = s + played["rewards"][0, 0, t]
    assert s == total and played["actions"].shape == (1, 1, 128, 10, 2)
    eng.close()


@pytest.fixture(scope="module")
def monitor(tmp_path_factory):
    from goldsrl import envs, _ffi
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import ConvSingleAgentPolicyNetwork
    from goldsrl.agents.state_processors import SwarmStateProcessor
    conf = dict(name='local_learning', num_actions=2, clip_norm=40.0, clip_norm_type='global', device='/gpu:0',
                entropy_regularisation_strength=0.02, scale=1000.0, height=84, width=84, channels=3)
    d = tmp_path_factory.mktemp("search")
    learner_eng = _ffi.Engine(_ffi.ENV_SWARM, 2, seed=5)
    learner_eng.reset()
    global_net = ConvSingleAgentPolicyNetwork(conf).bind(learner_eng, seed=11)
    mon = PM.SwarmPolicyMonitor(envs.make("Swarm-eval-v0"), global_net, SwarmStateProcessor(grid_size=84), PM.ScalarWriter(str(d / "eval")),
                                network_conf=conf)
    mon.actions_path = str(d / "swarm-eval.json")
    return mon


def test_monitor_search_baseline(monitor):
    from goldsrl.baselines import SwarmRuleBaseline, SwarmRuleSearch
    monitor.env.reset()
    fresh = {f: monitor.env._eng.get_state(f) for f in FIELDS}
    name, total = monitor.search_baseline(3, 8, 3)
    after = {f: monitor.env._eng.get_state(f) for f in FIELDS}
    for f in FIELDS:
        if f != "EPISODE":                                                   # every reset starts a new episode
            assert after[f].tobytes() == fresh[f].tobytes(), f
    b = SwarmRuleSearch(monitor.env._eng, None, 3, 8, 3)                     # the env is reset: the same episode
    six, value = b.best()
    assert total == value == monitor.search_baseline_total_reward and six == monitor.search_baseline_rule and name.startswith("tuned rule")
    # never below the start (the start's fit is a sequential sum, the table's total numpy's: equal to rounding)
    assert b.start_total == SwarmRuleBaseline(monitor.env._eng).best_total()[2] and value > b.start_total - 1e-9
    # alone, it is also the baseline; after another baseline it leaves that one's name and total alone
    assert monitor.baseline_total_reward == total and monitor.baseline_name == name
    rule_name, rule_total = monitor.rule_baseline()
    monitor.search_baseline(3, 8, 3)
    assert monitor.baseline_total_reward == rule_total and monitor.baseline_name == rule_name and monitor.search_baseline_total_reward == total
    q = queue.Queue()                                                        # the found rule's episode played by the monitor, step by step
    kept = b.play_best(keep_actions=True)
    for a in kept["actions"][0, 0]:
        q.put(a)
    played, length, _ = monitor.eval_once(actions=q)
    # the monitor's total is np.sum of the step rewards, the search's their sequential sum: the same rewards, equal to rounding
    assert length == 128 and played == float(np.sum(kept["rewards"][0, 0])) and abs(played - total) <= 128 * 2.0 ** -53 * abs(total)
    rows = [json.loads(line) for line in open(monitor.summary_writer.get_logdir() + "/scalars.jsonl")]
    last = {r["tag"]: r["value"] for r in rows}
    assert last["eval/search_baseline_total_reward"] == total and last["eval/total_reward_minus_search_baseline"] == played - total
    assert last["eval/baseline_total_reward"] == rule_total and last["eval/total_reward_minus_baseline"] == played - rule_total


def test_the_script_keeps_the_found_rules_episode(tmp_path, capsys):
    from goldsrl.scripts import make_swarm_gif, swarm_rules
    path = str(tmp_path / "search.json")
    best, six, score = swarm_rules.main(["--search", "2:4:2", "--json", path])
    printed = capsys.readouterr().out
    assert "search: generation 0 best" in printed and "search: generation 1 best" in printed and "search: 2 generations of 4 candidates, 2 elites" in printed
    kept = json.load(open(path))
    assert kept["score"] == score and len(kept["actions"]) == 128
    got, replayed = make_swarm_gif.main(["--actions", path, "--no-gif"])
    printed = capsys.readouterr().out
    assert "score reproduced" in printed and "score differs" not in printed and got == replayed == score
