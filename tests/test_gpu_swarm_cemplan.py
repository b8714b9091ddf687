"""GPU: the search planner of the Swarm env, a planned episode of every env in one call (include/goldsrl_swarmcemplan.h,
csrc/swarm_cemplan.hip).  The oracle is the same computation composed on the host from tested pieces
(goldsrl/_ffi_swarmcemplan.py:swarm_cemplan_host: grl_swarm_rules of the union table for the lookaheads, the search's numpy
statements, a Python > scan, grl_swarm_step_f64 for the commit); every comparison with it is of bytes.  Degenerate forms pin the call
to grl_swarm_rules and grl_swarm_plan.  Only the case that holds the planner to the unmodified reference's fixture has tolerances
(those of tests/test_gpu_swarm_plan.py's fixture case)."""
import json
import queue

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("SWARM_X", "SWARM_XA", "SWARM_PNOISE", "SWARM_ANOISE", "ELAPSED", "EPISODE")
OUTPUTS = ("reward", "reward_f64", "done", "elapsed", "locust_bins", "agent_bins", "positions", "done_count")
SAME = ("rewards", "length", "finished", "choices", "chosen_rules", "chosen_offsets", "lib_scores", "candidates", "scores", "order", "mean",
        "std", "actions")

# tests/test_gpu_swarm_plan.py's three rules and its (horizon, replan, steps)
RULES = np.array([(0, 1.5, 0, 0.1, 0.2, 0.5), (1, 5, 1, 0.3, -0.3, 0), (0.5, 2, 1, 0, 0, 0.2)], np.float64)
HKS = ((1, 1, 5), (3, 2, 5), (4, 4, 6))
# (generations, candidates, elites): the smallest; two generations; every candidate an elite; more candidates than a wave has lanes
GCM = ((1, 2, 1), (2, 5, 2), (2, 5, 5), (2, 70, 8))
STARTS = np.array([(1, 5, 0, -1.5, 1.5, 0.7), (0.5, 2, 1, 0.1, -0.2, 0.3)], np.float64)        # a centroid start, a nearest-locust start
WIDE = dict(lo=(-8.0, -8.0, -8.0, -8.0, -8.0), hi=(64.0, 64.0, 8.0, 8.0, 8.0))
PINNED = dict(spread=(0.0,) * 5, floor=(0.0,) * 5, **WIDE)


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
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, want[k].dtype, got[k].shape, want[k].shape)
        if upto is not None and k in ("rewards", "actions"):
            for e, n in enumerate(upto):
                assert got[k][e, :n].tobytes() == want[k][e, :n].tobytes(), (k, e)
        else:
            assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])


def _call_then_host(eng, rules, start, H, K, S, G, C, M, trace_env=None, **box):
    """the one call first -- it leaves the handle as it was --, then the host composition on the same engine, which advances it"""
    from goldsrl import _ffi_swarmcemplan as P
    before = {f: eng.get_state(f).tobytes() for f in FIELDS}
    got = P.swarm_cemplan(eng, rules, start, H, K, G, C, M, seed=3, max_steps=S, keep_actions=True, trace_env=trace_env, **box)
    assert {f: eng.get_state(f).tobytes() for f in FIELDS} == before
    want = P.swarm_cemplan_host(eng, rules, start, H, K, G, C, M, seed=3, max_steps=S, keep_actions=True, trace_env=trace_env, **box)
    return got, want


@pytest.mark.parametrize("n_rules", [0, 1, 3])
@pytest.mark.parametrize("E", [1, 3, 4, 5, 9])
def test_the_one_call_is_the_host_composition(E, n_rules):
    searched = 0
    for i, (G, C, M) in enumerate(GCM):
        if C == 70 and E > 5:                                               # the host's union table holds E * C <= 4096 rows
            continue
        for H, K, S in HKS:
            eng = _engine(E)
            got, want = _call_then_host(eng, RULES[:n_rules], STARTS[i % 2], H, K, S, G, C, M, trace_env=E // 2)
            D = (S + K - 1) // K
            assert got["rewards"].shape == (E, S) and got["choices"].shape == (E, D) and got["lib_scores"].shape == (E, D, n_rules)
            assert got["candidates"].shape == (E, D, G, C, 6) and got["order"].shape == (E, D, G, C) and got["mean"].shape == (E, D, G + 1, 5)
            assert got["actions"].shape == (E, S, 10, 2) and got["trace_x"].shape == (S, 80, 2) and got["trace_xa"].shape == (S, 10, 2)
            assert (got["length"] == S).all() and not got["finished"].any() and (got["rewards"] < 0).all()
            assert (got["choices"] >= 0).all() and (got["choices"] <= n_rules).all() and (got["scores"] < 0).all()
            assert (np.sort(got["order"], axis=-1) == np.arange(C)).all()                        # every rank list is a permutation
            assert np.array_equal(got["totals"], got["rewards"].sum(-1)) and got["searched"] == int((got["choices"] == n_rules).sum())
            _same(got, want, SAME + ("trace_x", "trace_xa"))
            searched += got["searched"]
            eng.close()
    assert searched > 0                                                     # the searched rule is committed somewhere


def test_no_library_and_no_spread_is_the_start_rule():
    """R = 0 with std0 = floor = 0: every candidate is the start rule, every choice is R = 0 (searched), the mean never moves, and the
    episode is grl_swarm_rules of that one rule.  Two elites: the refit's sums p + p are exact, so the mean keeps its bits."""
    from goldsrl import _ffi_swarmcemplan as P, _ffi_swarmrules as R
    E, S = 5, 6
    eng = _engine(E)
    for start in (RULES[0], RULES[1]):
        ref = R.swarm_rules(eng, start[None], S, keep_actions=True)
        for (H, K), (G, C, M) in zip(((1, 1), (3, 2), (6, 6)), ((1, 2, 1), (2, 5, 2), (3, 4, 2))):
            out = P.swarm_cemplan(eng, None, start, H, K, G, C, M, max_steps=S, keep_actions=True, **PINNED)
            D = (S + K - 1) // K
            assert not out["choices"].any() and out["searched"] == E * D and out["lib_scores"].shape == (E, D, 0)
            assert out["candidates"].tobytes() == np.broadcast_to(start, (E, D, G, C, 6)).tobytes()
            assert out["mean"].tobytes() == np.broadcast_to(start[[0, 1, 3, 4, 5]], (E, D, G + 1, 5)).tobytes() and not out["std"].any()
            assert (out["order"] == np.arange(C)).all()                      # all scores tie: index order
            for k in ("rewards", "actions", "length", "finished"):
                assert out[k].tobytes() == ref[k].tobytes(), (H, K, k)       # (E, ...) against (E, 1, ...): the same bytes
    eng.close()


def test_pinned_to_a_library_rule_is_the_rule_planner():
    """Candidates pinned to a copy of one library rule: the searched score ties that rule's, the tie goes to the library, no choice
    is R, and rewards, choices and library scores are grl_swarm_plan's bytes."""
    from goldsrl import _ffi_swarmcemplan as P, _ffi_swarmplan as PL
    E = 5
    eng = _engine(E)
    for i, (H, K, S) in enumerate(HKS):
        G, C, M = ((1, 2, 1), (2, 5, 2), (2, 3, 1))[i]
        plan = PL.swarm_plan(eng, RULES, H, K, S, keep_actions=True)
        for start in RULES:
            out = P.swarm_cemplan(eng, RULES, start, H, K, G, C, M, max_steps=S, keep_actions=True, **PINNED)
            assert not (out["choices"] == len(RULES)).any() and out["searched"] == 0
            for k in ("rewards", "actions", "choices", "length", "finished"):
                assert out[k].tobytes() == plan[k].tobytes(), (H, K, k)
            assert out["lib_scores"].tobytes() == plan["scores"].tobytes()
            which = int(np.flatnonzero((RULES == start).all(1))[0])
            assert out["scores"][:, :, 0, 0].tobytes() == out["lib_scores"][:, :, which].tobytes()      # the tie is one of bits
    eng.close()


def test_invariants():
    from goldsrl import _ffi_swarmcemplan as P
    from goldsrl._ffi_swarmsearch import DEFAULT_SPREAD
    E, R = 5, 3
    eng = _engine(E)
    out = P.swarm_cemplan(eng, RULES, STARTS[0], 3, 2, 3, 6, 3, seed=5, max_steps=9)
    D, G = 5, 3
    assert out["choices"].shape == (E, D) and (out["choices"] >= 0).all()
    first = out["order"][..., 0]                                            # (E, D, G)
    for e in range(E):
        for d in range(D):
            for g in range(1, G):                                           # the incumbent is replayed from the same state: the same score
                assert out["scores"][e, d, g, 0].tobytes() == out["scores"][e, d, g - 1, first[e, d, g - 1]].tobytes()
                assert out["candidates"][e, d, g, 0].tobytes() == out["candidates"][e, d, g - 1, first[e, d, g - 1]].tobytes()
            assert out["std"][e, d, 0].tobytes() == np.asarray(DEFAULT_SPREAD, np.float64).tobytes()
            found = out["candidates"][e, d, G - 1, first[e, d, G - 1]]
            if out["choices"][e, d] == R:
                assert out["chosen_rules"][e, d].tobytes() == found[:3].tobytes()
            else:
                assert out["chosen_rules"][e, d].tobytes() == RULES[out["choices"][e, d], :3].tobytes()
            if d + 1 < D:
                want = found[[0, 1, 3, 4, 5]] if out["choices"][e, d] == R else out["mean"][e, d, 0]
                assert out["mean"][e, d + 1, 0].tobytes() == want.tobytes(), (e, d)
    assert 0 < out["searched"] <= E * D
    eng.close()


def test_ends_by_the_time_limit():
    from goldsrl import _ffi_swarmcemplan as P, _ffi_swarmrules as R
    # ends that differ inside a workgroup and across two, at different decisions and inside a commit: env e has e steps behind it
    E = 5
    eng = _engine(E, max_episode_steps=8)
    eng.set_state("ELAPSED", np.arange(E, dtype=np.int32))
    got, want = _call_then_host(eng, RULES, STARTS[0], 3, 2, 10, 2, 5, 2, trace_env=3)
    assert got["length"].tolist() == [8 - e for e in range(E)] and (got["finished"] == 1).all()
    _same(got, want, upto=got["length"])
    for e in range(E):
        n, d = 8 - e, (8 - e + 1) // 2
        assert not got["rewards"][e, n:].any() and not got["actions"][e, n:].any()
        assert (got["choices"][e, :d] >= 0).all() and (got["choices"][e, d:] == -1).all()
        for k in ("chosen_rules", "chosen_offsets", "lib_scores", "candidates", "scores", "order", "mean", "std"):
            assert got[k][e, :d].any() and not got[k][e, d:].any(), (k, e)
    # env 3 plays 5 steps; the host composition cannot trace the step that ends an episode (the engine has reset the env by then)
    assert got["trace_x"][:4].tobytes() == want["trace_x"][:4].tobytes() and got["trace_xa"][:4].tobytes() == want["trace_xa"][:4].tobytes()
    assert got["trace_x"][4].any() and got["trace_xa"][4].any() and not got["trace_x"][5:].any() and not got["trace_xa"][5:].any()
    eng.close()

    # the lookahead is cut by the TimeLimit, not by max_steps: one step is played, three are looked ahead
    eng = _engine(3)
    out = P.swarm_cemplan(eng, RULES, STARTS[0], 3, 1, 1, 4, 2, max_steps=1)
    look = R.swarm_rules(eng, np.concatenate([RULES, out["candidates"][0, 0, 0]]), 3)
    want = np.zeros((3, 7))
    for t in range(3):
        want = want + look["rewards"][:, :, t]
    assert out["lib_scores"][:, 0].tobytes() == want[:, :3].tobytes() and (out["length"] == 1).all() and not out["finished"].any()
    assert out["scores"][:, 0, 0].tobytes() == want[:, 3:].tobytes()         # generation 0's candidates are the same rows for every env
    eng.close()


def test_dynamics_are_the_replay_of_the_kept_actions():
    from goldsrl import _ffi_replay, _ffi_swarmcemplan as P
    E, S = 5, 7
    eng = _engine(E)
    out = P.swarm_cemplan(eng, RULES, STARTS[1], 3, 2, 2, 5, 2, max_steps=S, keep_actions=True, trace_env=4)
    rep = _ffi_replay.swarm_replay(eng, out["actions"].reshape(E, 1, S, 10, 2), trace_env=4)
    for k in ("rewards", "length", "finished", "trace_x", "trace_xa"):
        assert rep[k].dtype == out[k].dtype and rep[k].tobytes() == out[k].tobytes(), k
    eng.close()


def test_the_handle_is_read_only():
    from goldsrl import _ffi_swarmcemplan as P
    E = 5
    eng, other = _engine(E), _engine(E)
    first = np.ascontiguousarray(np.random.RandomState(1).normal(size=(E, 10, 2)).astype(np.float32) * 0.5)
    eng.step(first); other.step(first)          # so that the outputs hold something
    before = {f: eng.get_state(f).tobytes() for f in FIELDS}
    outs = {o: eng.read(o).tobytes() for o in OUTPUTS}
    P.swarm_cemplan(eng, RULES, STARTS[0], 3, 2, 2, 5, 2, max_steps=5, keep_actions=True, trace_env=2)
    P.swarm_cemplan(eng, None, STARTS[1], 1, 1, 1, 2, 1, max_steps=3)
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
    from goldsrl import _ffi
    if kind == "refdiv":
        monkeypatch.setenv("GRL_SWARM_DIV", "ref")                   # read at grl_create
    E, S = 5, 6
    eng = _engine(E, flags=_ffi.F_SWARM_FAST_MATH if kind == "fast" else 0)
    got, want = _call_then_host(eng, RULES, STARTS[0], 3, 2, S, 2, 5, 2, trace_env=4)
    _same(got, want, SAME + ("trace_x", "trace_xa"))
    eng.close()


def test_error_paths():
    from goldsrl import _ffi, _ffi_swarmcemplan as P, _ffi_swarmrules as R
    from goldsrl._ffi_swarmsearch import DEFAULT_FLOOR, DEFAULT_HI, DEFAULT_LO, DEFAULT_SPREAD, swarm_search_ring
    lib = _ffi.load_library(extra_signatures=P.SWARMCEMPLAN_SIGNATURES)
    head, off = np.ascontiguousarray(RULES[:, :3]), np.ascontiguousarray(R.swarm_rule_offsets(RULES))
    S, D, G, C = 6, 3, 2, 5
    good = dict(head=head, off=off, n=3, anchor=0, mean0=np.array(STARTS[0][[0, 1, 3, 4, 5]]), std0=np.array(DEFAULT_SPREAD), floor=np.array(DEFAULT_FLOOR),
                lo=np.array(DEFAULT_LO), hi=np.array(DEFAULT_HI), ring=swarm_search_ring(), z=np.random.default_rng(0).standard_normal((D, G, C, 5)),
                H=3, K=2, G=G, C=C, M=2, steps=S, keep=0, trace=-1)

    def call(h, **kw):
        a = dict(good, **kw)
        p = lambda v: None if v is None else _ffi._ptr(np.ascontiguousarray(v, np.float64))
        return lib.grl_swarm_cemplan(h, p(a["head"]), p(a["off"]), a["n"], a["anchor"], p(a["mean0"]), p(a["std0"]), p(a["floor"]), p(a["lo"]),
                                     p(a["hi"]), p(a["ring"]), p(a["z"]), a["H"], a["K"], a["G"], a["C"], a["M"], a["steps"], a["keep"], a["trace"])

    def refused(h, word, **kw):
        assert call(h, **kw) == _ffi.E_INVALID, kw
        assert word.encode() in lib.grl_last_error(h), (kw, lib.grl_last_error(h))

    solow = _ffi.Engine(_ffi.ENV_SOLOW, 2, seed=1)
    solow.reset()
    with pytest.raises(ValueError):
        P.swarm_cemplan(solow, RULES, STARTS[0], max_steps=S)
    refused(solow.h, "not a Swarm handle")
    solow.close()

    eng = _engine(2)
    buf = np.zeros((2, S))
    assert lib.grl_swarm_cemplan_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE       # before any run
    for name in ("mean0", "std0", "floor", "lo", "hi", "ring", "z"):
        refused(eng.h, "null argument", **{name: None})
    refused(eng.h, "null argument", head=None)
    refused(eng.h, "null argument", off=None)
    refused(eng.h, "n_rules", n=-1)
    refused(eng.h, "n_rules", n=4097, head=np.zeros((4097, 3)), off=np.zeros((4097, 10, 2)))
    refused(eng.h, "anchor", anchor=2)
    refused(eng.h, "G must", G=0)
    refused(eng.h, "C must", C=1)
    refused(eng.h, "C must", C=1025)
    refused(eng.h, "K must", M=0)
    refused(eng.h, "K must", M=C + 1)
    refused(eng.h, "max_steps", steps=0)
    refused(eng.h, "horizon", H=0, K=0)
    refused(eng.h, "replan", K=4)                                            # replan > horizon
    refused(eng.h, "replan", K=0)
    bad = head.copy(); bad[1, 2] = 2.0
    refused(eng.h, "anchor", head=bad)
    bad = head.copy(); bad[2, 1] = np.inf
    refused(eng.h, "not finite", head=bad)
    bad = off.copy(); bad[2, 9, 1] = np.nan
    refused(eng.h, "offset", off=bad)
    for name in ("mean0", "std0", "floor", "lo", "hi"):
        bad = good[name].copy(); bad[3] = np.nan
        refused(eng.h, name + "[3] is not finite", **{name: bad})
    for name in ("std0", "floor"):
        bad = good[name].copy(); bad[1] = -1e-9
        refused(eng.h, name + "[1] is negative", **{name: bad})
    bad = good["lo"].copy(); bad[2] = 5.0
    refused(eng.h, "lo[2] is above hi[2]", lo=bad)
    bad = good["ring"].copy(); bad[4, 1] = np.inf
    refused(eng.h, "ring[4]", ring=bad)
    bad = good["z"].copy(); bad[2, 1, 4, 4] = np.nan
    refused(eng.h, "normals[%d] is not finite" % (bad.size - 1), z=bad)
    refused(eng.h, "trace_env", trace=2)
    refused(eng.h, "trace_env", trace=-2)
    # an output past 2^31 - 1 elements is refused before the normals are read or anything is allocated (the pointer is never followed)
    refused(eng.h, "does not fit in int32", steps=2 ** 24, H=1, K=1, G=64, C=1024, M=1)
    assert lib.grl_swarm_cemplan_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE       # a refused call is no run
    for kw in (dict(horizon=2, replan=3), dict(replan=0), dict(generations=0), dict(candidates=1), dict(elites=6, candidates=5),
               dict(spread=(0, -1, 0, 0, 0)), dict(lo=(0, 0, 5, 0, 0), hi=(1, 1, 1, 1, 1)), dict(normals=np.zeros((2, 2, 5, 5)))):
        with pytest.raises(ValueError):
            P.swarm_cemplan(eng, RULES, STARTS[0], **dict(dict(max_steps=S), **kw))            # the host check, before the C ABI
    assert call(eng.h) == _ffi.OK                                            # no actions kept, no trace
    act, tx, ch = np.zeros((2, S, 10, 2)), np.zeros((S, 80, 2)), np.zeros((2, D), np.int32)
    assert lib.grl_swarm_cemplan_read(eng.h, b"actions", _ffi._ptr(act), act.nbytes) == _ffi.E_STATE
    assert lib.grl_swarm_cemplan_read(eng.h, b"trace_x", _ffi._ptr(tx), tx.nbytes) == _ffi.E_STATE
    assert lib.grl_swarm_cemplan_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes - 8) == _ffi.E_SIZE
    assert lib.grl_swarm_cemplan_read(eng.h, b"choices", _ffi._ptr(ch), ch.nbytes + 4) == _ffi.E_SIZE
    assert lib.grl_swarm_cemplan_read(eng.h, b"rewards", _ffi._ptr(buf), buf.nbytes) == _ffi.OK and (buf < 0).all()
    assert lib.grl_swarm_cemplan_read(eng.h, b"choices", _ffi._ptr(ch), ch.nbytes) == _ffi.OK and (ch >= 0).all()
    assert lib.grl_swarm_cemplan_read(eng.h, b"nothing", _ffi._ptr(buf), buf.nbytes) == _ffi.E_INVALID
    assert call(eng.h, keep=1, trace=1) == _ffi.OK
    assert lib.grl_swarm_cemplan_read(eng.h, b"actions", _ffi._ptr(act), act.nbytes) == _ffi.OK
    assert lib.grl_swarm_cemplan_read(eng.h, b"trace_x", _ffi._ptr(tx), tx.nbytes) == _ffi.OK
    assert call(eng.h, n=0, head=None, off=None) == _ffi.OK                  # no library
    sc = np.zeros((2, D, 0))
    assert lib.grl_swarm_cemplan_read(eng.h, b"lib_scores", _ffi._ptr(np.zeros(1)), sc.nbytes) == _ffi.E_STATE
    eng.step_async(np.zeros((2, 10, 2), np.float32))                         # a step in flight
    refused(eng.h, "in flight")
    eng.wait()
    eng.close()


def _fixture_engine(golden):
    g = golden("swarm_rules")
    eng = _engine(1, seed=1)
    for f, k in (("SWARM_X", "x"), ("SWARM_XA", "xa"), ("SWARM_PNOISE", "particle_noise_row"), ("SWARM_ANOISE", "agent_noise_row")):
        eng.set_state(f, np.ascontiguousarray(g[k][None]))
    return eng, g


def test_the_reference_fixture(golden):
    """The search planner over the default rules on the reset state of the reference's SwarmEnv(seed=192), 128 steps, (H, K, G, C, M) =
    (8, 4, 2, 12, 4), against what the same scheme gave on the unmodified reference env in numpy (tests/golden/swarm_cemplan.npz),
    with the normals stored there.  The generator asserts at every decision the best-to-second gap and the gap across the elite
    boundary of every generation and the gap between the library's best and the searched score to be at least 1e-6 relative, or an
    exact tie of two rules that act alike (gain 0 and the same cancel: the same episode, the same bits on both sides, the tie broken
    by the index on both; the generator's docstring says why these are structural), so the choices, every order[0] and every elite
    set are compared exactly.  Bounds: those of
    test_gpu_swarm_plan.py:test_the_reference_fixture -- rewards rtol 1e-9, total rtol 1e-10."""
    from goldsrl.baselines import SwarmSearchPlanner
    eng, rules_fixture = _fixture_engine(golden)
    g = golden("swarm_cemplan")
    H, K, G, C, M = (int(v) for v in g["shape"])
    assert g["start"].tobytes() == rules_fixture["rules"][int(rules_fixture["best_index"])].tobytes()
    assert float(g["plan_total"]) == float(golden("swarm_plan")["total_8_4"])
    b = SwarmSearchPlanner(eng, g["rules"], g["start"], H, K, G, C, M, normals=g["normals"])
    out = b.run()
    rel = np.abs(out["rewards"][0] - g["rewards"]) / np.abs(g["rewards"])
    print("total %.12f against %.12f, relative %.3g; largest relative reward error %.3g; %d of %d decisions searched; smallest gaps that are no admitted tie %.3g "
          "(first rank) %.3g (elite boundary) %.3g (choice); whole orders equal: %s; rule planner (8, 4) %.12f"
          % (out["totals"][0], float(g["total"]), abs(out["totals"][0] - g["total"]) / abs(g["total"]), rel.max(), b.searched(),
             int((out["choices"] >= 0).sum()), g["gaps"][..., 0][~g["tied"][..., 0]].min(), g["gaps"][..., 1][~g["tied"][..., 1]].min(),
             g["choice_gaps"][~g["choice_tied"]].min(),
             np.array_equal(out["order"][0], g["order"]), float(g["plan_total"])))
    assert out["length"][0] == int(g["length"]) == 128 and out["finished"][0] == 1
    assert out["candidates"][0, 0, 0].tobytes() == g["candidates"][0, 0].tobytes()               # a function of the inputs alone
    assert np.array_equal(out["choices"][0], g["choices"])
    assert np.array_equal(out["order"][0, :, :, 0], g["order"][:, :, 0])
    for d in range(out["choices"].shape[1]):
        for gen in range(G):
            assert set(out["order"][0, d, gen, :M].tolist()) == set(g["order"][d, gen, :M].tolist()), (d, gen)
    np.testing.assert_allclose(out["rewards"][0], g["rewards"], rtol=1e-9)
    np.testing.assert_allclose(out["totals"][0], g["total"], rtol=1e-10)
    assert b.total() == out["totals"][0] and b.total() - float(g["plan_total"]) > 5 and b.searched() == int((g["choices"] == len(g["rules"])).sum())
    eng.close()


@pytest.fixture(scope="module")
def monitor(tmp_path_factory):
    from goldsrl import envs, _ffi
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import ConvSingleAgentPolicyNetwork
    from goldsrl.agents.state_processors import SwarmStateProcessor
    conf = dict(name='local_learning', num_actions=2, clip_norm=40.0, clip_norm_type='global', device='/gpu:0',
                entropy_regularisation_strength=0.02, scale=1000.0, height=84, width=84, channels=3)
    d = tmp_path_factory.mktemp("cemplan")
    learner_eng = _ffi.Engine(_ffi.ENV_SWARM, 2, seed=5)
    learner_eng.reset()
    global_net = ConvSingleAgentPolicyNetwork(conf).bind(learner_eng, seed=11)
    mon = PM.SwarmPolicyMonitor(envs.make("Swarm-eval-v0"), global_net, SwarmStateProcessor(grid_size=84), PM.ScalarWriter(str(d / "eval")),
                                network_conf=conf)
    mon.actions_path = str(d / "swarm-eval.json")
    return mon


def test_monitor_cem_plan_baseline(monitor, capsys):
    from goldsrl.baselines import DEFAULT_SWARM_RULES, SwarmSearchPlanner
    from goldsrl.scripts import make_swarm_gif
    monitor.env.reset()
    fresh = _state(monitor.env._eng)
    name, total = monitor.cem_plan_baseline()                               # no other baseline has run: it supplies the common pair too
    setting = (32, 8, 2, 16, 4)                                             # the monitor's default: the better one over other seeds (LABNOTES.md)
    after = _state(monitor.env._eng)
    for f in FIELDS:
        if f != "EPISODE":                                                   # every reset starts a new episode
            assert after[f].tobytes() == fresh[f].tobytes(), f
    st = monitor.cem_plan_stats
    assert st["rewards"].shape == (1, 128) and st["choices"].shape == (1, 16) and st["length"][0] == 128
    assert total == monitor.cem_plan_baseline_total_reward == st["totals"][0] and name == monitor.cem_plan_baseline_name
    assert name.startswith("search plan (horizon 32, replan 8, 2 generations of 16, 4 elites, 20 rules")
    assert monitor.baseline_name == name and monitor.baseline_total_reward == total
    _, plan_total = monitor.plan_baseline()                                 # the plan takes the common pair; the search plan keeps its own
    assert monitor.baseline_total_reward == plan_total and monitor.cem_plan_baseline_total_reward == total and total > plan_total
    name2, total2 = monitor.cem_plan_baseline()                             # again: the common pair stays the plan's
    assert (name2, total2) == (name, total) and monitor.baseline_total_reward == plan_total
    b = SwarmSearchPlanner(monitor.env._eng, DEFAULT_SWARM_RULES, None, *setting)          # the env is reset: the same episode
    assert b.total() == total and b.searched() >= 1
    # the planned episode played by the monitor, step by step: the same score, the scalars beside it, and a file that replays
    q = queue.Queue()
    for a in st["actions"][0]:
        q.put(a)
    played, length, _ = monitor.eval_once(actions=q)
    assert length == 128 and played == total
    rows = [json.loads(line) for line in open(monitor.summary_writer.get_logdir() + "/scalars.jsonl")]
    last = {r["tag"]: r["value"] for r in rows}
    assert last["eval/cem_plan_baseline_total_reward"] == total and last["eval/total_reward_minus_cem_plan_baseline"] == 0.0
    assert last["eval/baseline_total_reward"] == plan_total
    assert json.load(open(monitor.actions_path))["score"] == total
    got, score = make_swarm_gif.main(["--actions", monitor.actions_path, "--no-gif"])
    printed = capsys.readouterr().out
    assert "score reproduced" in printed and "score differs" not in printed and got == score == total


def test_the_script_keeps_the_planned_episode(tmp_path, capsys):
    from goldsrl.scripts import make_swarm_gif, swarm_rules
    path = str(tmp_path / "cemplan.json")
    best, six, score = swarm_rules.main(["--cem-plan", "8:4", "--json", path])
    printed = capsys.readouterr().out
    assert "cem-plan: horizon 8, replan 4, 2 generations of 12, 4 elites" in printed
    kept = json.load(open(path))
    assert kept["score"] == score and len(kept["actions"]) == 128
    make_swarm_gif.main(["--actions", path, "--no-gif"])
    printed = capsys.readouterr().out
    assert "score reproduced" in printed and "score differs" not in printed
