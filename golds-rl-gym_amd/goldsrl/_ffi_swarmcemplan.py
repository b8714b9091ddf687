"""ctypes binding of the search planner of the Swarm env (C ABI and the scheme, statement by statement:
include/goldsrl_swarmcemplan.h): at every decision each env tunes the rule's five real numbers by a short cross-entropy search over
lookaheads from where it stands, compares the result with a library of rules, commits the better for `replan` steps and plans
again, the whole planned episode of every env enqueued in one call.  swarm_cemplan_host is the same computation composed on the host
from tested pieces (grl_swarm_rules for the lookaheads, the search's numpy statements, a Python scan, grl_swarm_step_f64 for the
commit): the documented slow path, and the oracle the device is held to."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, steps_and_trace
from ._ffi_swarmrules import MAX_RULES, N_AGENTS, N_LOCUSTS, check_swarm_rules, swarm_rule_offsets, swarm_rules
from ._ffi_swarmsearch import (DEFAULT_FLOOR, DEFAULT_HI, DEFAULT_LO, DEFAULT_SPREAD, SEARCH_COLS, SEARCH_FIELDS,
                               swarm_search_candidates, swarm_search_refit, swarm_search_ring, swarm_search_start)
from ._search import BOX_NAMES, check_box, check_counts, check_normals, check_vectors

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_swarmcemplan.h: a dict of its own, as the header is a file of its own (tests/test_swarm_cemplan_header.py pins both)
SWARMCEMPLAN_SIGNATURES = {
    "grl_swarm_cemplan": (C.c_int, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I]),
    "grl_swarm_cemplan_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}


def _check_cemplan(engine, fn_name, rules, start, horizon, replan, generations, candidates, elites, spread, floor, lo, hi, seed, normals,
                   max_steps, trace_env):
    if engine.kind != _ffi.ENV_SWARM:
        raise ValueError("%s: the engine is not a Swarm engine" % fn_name)
    if rules is None or len(rules) == 0:
        r = np.zeros((0, 6), np.float64)                                    # no library: every choice is the searched rule
    else:
        r = check_swarm_rules(rules)
    start = check_swarm_rules(np.asarray(start, np.float64).reshape(1, -1))[0]
    H, K = int(horizon), int(replan)
    if H < 1 or K < 1 or K > H:
        raise ValueError("%s: 1 <= replan <= horizon is required, got horizon %d, replan %d" % (fn_name, H, K))
    G, Cn, M = check_counts(fn_name, generations, candidates, elites)
    spread, floor, lo, hi = check_vectors(fn_name, BOX_NAMES, (spread, floor, lo, hi), None, SEARCH_FIELDS)
    check_box(fn_name, spread, floor, lo, hi)
    T, t_env = steps_and_trace(engine, fn_name, max_steps, trace_env)
    D = (T + K - 1) // K
    z = check_normals(fn_name, normals, seed, (D, G, Cn, 5),
                      "(decisions, generations, candidates, 5) finite numbers with decisions = ceil(max_steps / replan) = %d" % D)
    return r, start, spread, floor, lo, hi, H, K, G, Cn, M, z, T, t_env, D


def _summary(out, R):
    out["totals"] = out["rewards"].sum(-1)
    out["searched"] = int((out["choices"] == R).sum())                      # decisions, over all envs, that committed a searched rule
    return out


def swarm_cemplan(engine, rules, start, horizon=8, replan=4, generations=2, candidates=12, elites=4, spread=DEFAULT_SPREAD,
                  floor=DEFAULT_FLOOR, lo=DEFAULT_LO, hi=DEFAULT_HI, seed=0, normals=None, max_steps=None, keep_actions=False, trace_env=None):
    """Plan every env from the engine's CURRENT state (reset it first) for up to max_steps steps (default: the engine's
    max_episode_steps); the engine's state is left as it was.  rules: the library, (n_rules, 6) rows (cancel, gain, anchor, off_x,
    off_y, radius), or None / empty for none.  start: the six-number row the search's mean starts from at the first decision; its
    anchor is the searched rules'.  At each of the D = ceil(max_steps / replan) decisions every env runs `generations` generations
    of `candidates` candidates refitted over `elites` elites around its own mean (the spread is reset to `spread` at every decision),
    each candidate and each library rule played min(horizon, steps to the TimeLimit) steps ahead; the searched rule is committed
    for replan steps if it beats the library's best strictly, else that library rule.  normals: (D, generations, candidates, 5),
    shared by all envs, default np.random.default_rng(seed).standard_normal.  One call.

    Returns rules, rewards (E, T), totals (E,), length (E,) int32, finished (E,) uint8, choices (E, D) int32 (the library index,
    n_rules for the searched rule, -1 past the env's last decision), chosen_rules (E, D, 3), chosen_offsets (E, D, 10, 2), lib_scores
    (E, D, n_rules), candidates (E, D, G, C, 6), scores and order (E, D, G, C), mean and std (E, D, G + 1, 5), searched (how many
    decisions committed a searched rule); with keep_actions actions (E, T, 10, 2); with trace_env trace_x (T, 80, 2) and trace_xa
    (T, 10, 2).  Everything is zero past the env's end."""
    r, start, spread, floor, lo, hi, H, K, G, Cn, M, z, T, t_env, D = _check_cemplan(
        engine, "swarm_cemplan", rules, start, horizon, replan, generations, candidates, elites, spread, floor, lo, hi, seed, normals,
        max_steps, trace_env)
    R = r.shape[0]
    off = np.ascontiguousarray(swarm_rule_offsets(r)) if R else np.zeros((0, N_AGENTS, 2), np.float64)
    head = np.ascontiguousarray(r[:, :3])
    mean0 = np.ascontiguousarray(start[list(SEARCH_COLS)])
    ring = swarm_search_ring()
    lib = _ffi.load_library(extra_signatures=SWARMCEMPLAN_SIGNATURES)
    engine._check(lib.grl_swarm_cemplan(engine.h, _ffi._ptr(head) if R else None, _ffi._ptr(off) if R else None, R, int(start[2]),
                                        _ffi._ptr(mean0), _ffi._ptr(spread), _ffi._ptr(floor), _ffi._ptr(lo), _ffi._ptr(hi), _ffi._ptr(ring),
                                        _ffi._ptr(z), H, K, G, Cn, M, T, 1 if keep_actions else 0, t_env))
    per_env = [("rewards", np.float64, (T,)), ("length", np.int32, ()), ("finished", np.uint8, ()), ("choices", np.int32, (D,)),
               ("chosen_rules", np.float64, (D, 3)), ("chosen_offsets", np.float64, (D, N_AGENTS, 2)),
               ("candidates", np.float64, (D, G, Cn, 6)), ("scores", np.float64, (D, G, Cn)), ("order", np.int32, (D, G, Cn)),
               ("mean", np.float64, (D, G + 1, 5)), ("std", np.float64, (D, G + 1, 5))]
    if R:
        per_env += [("lib_scores", np.float64, (D, R))]
    if keep_actions:
        per_env += [("actions", np.float64, (T, N_AGENTS, 2))]
    out = {"rules": r}
    out.update(read_outputs(engine, lib.grl_swarm_cemplan_read, per_env, (engine.E,)))
    if not R:
        out["lib_scores"] = np.zeros((engine.E, D, 0), np.float64)
    if t_env >= 0:
        out.update(read_outputs(engine, lib.grl_swarm_cemplan_read,
                                (("trace_x", np.float64, (N_LOCUSTS, 2)), ("trace_xa", np.float64, (N_AGENTS, 2))), (T,)))
    return _summary(out, R)


def _sum_in_order(rewards, length):
    s = np.float64(0.0)
    for t in range(int(length)):
        s = s + rewards[t]
    return s


def swarm_cemplan_host(engine, rules, start, horizon=8, replan=4, generations=2, candidates=12, elites=4, spread=DEFAULT_SPREAD,
                       floor=DEFAULT_FLOOR, lo=DEFAULT_LO, hi=DEFAULT_HI, seed=0, normals=None, max_steps=None, keep_actions=False,
                       trace_env=None):
    """swarm_cemplan composed on the host, several round trips per generation.  Per decision: one grl_swarm_rules(max_steps=horizon)
    of the library; per generation swarm_search_candidates per env, one grl_swarm_rules(max_steps=horizon) of the union table (the E
    envs' C rows, env e reading its own block: E * C <= 4096 is required), the scores as Python loops of float64 adds over
    t < length, swarm_search_refit per env; a Python > scan over the library's scores; one more grl_swarm_rules(max_steps=replan) of
    the E chosen rules with the action rows kept (env e reading pair (e, e)), and replan calls of grl_swarm_step_f64 with them.  Same arguments and outputs as swarm_cemplan.  It ADVANCES the engine as swarm_plan_host does
    (an env whose episode ends is auto-reset by the engine, takes no further part here and is stepped with zero actions; the trace
    row of the step that ends the traced env's episode stays zero)."""
    r, start, spread, floor, lo, hi, H, K, G, Cn, M, z, T, t_env, D = _check_cemplan(
        engine, "swarm_cemplan_host", rules, start, horizon, replan, generations, candidates, elites, spread, floor, lo, hi, seed, normals,
        max_steps, trace_env)
    E, R = engine.E, r.shape[0]
    if E * Cn > MAX_RULES:
        raise ValueError("swarm_cemplan_host: the union table of %d envs x %d candidates has more than %d rows" % (E, Cn, MAX_RULES))
    lib_off = swarm_rule_offsets(r) if R else np.zeros((0, N_AGENTS, 2), np.float64)
    out = {"rules": r, "rewards": np.zeros((E, T)), "length": np.zeros(E, np.int32), "finished": np.zeros(E, np.uint8),
           "choices": np.full((E, D), -1, np.int32), "chosen_rules": np.zeros((E, D, 3)), "chosen_offsets": np.zeros((E, D, N_AGENTS, 2)),
           "lib_scores": np.zeros((E, D, R)), "candidates": np.zeros((E, D, G, Cn, 6)), "scores": np.zeros((E, D, G, Cn)),
           "order": np.zeros((E, D, G, Cn), np.int32), "mean": np.zeros((E, D, G + 1, 5)), "std": np.zeros((E, D, G + 1, 5))}
    if keep_actions:
        out["actions"] = np.zeros((E, T, N_AGENTS, 2), np.float64)
    if t_env >= 0:
        out["trace_x"] = np.zeros((T, N_LOCUSTS, 2), np.float64)
        out["trace_xa"] = np.zeros((T, N_AGENTS, 2), np.float64)
    cols = list(SEARCH_COLS)
    mean_e = np.tile(swarm_search_start(start[cols], lo, hi), (E, 1))       # 1 start
    alive = np.ones(E, bool)
    t = 0
    for d in range(D):
        if not alive.any():
            break
        live = np.flatnonzero(alive)
        chosen = np.zeros((E, 6), np.float64)                               # the chosen rule of every env (an ended env: the zero row)
        if R:
            look = swarm_rules(engine, r, H)
            for e in live:
                for i in range(R):
                    out["lib_scores"][e, d, i] = _sum_in_order(look["rewards"][e, i], look["length"][e, i])
        incumbent = np.zeros((E, 6), np.float64)
        for e in live:
            out["mean"][e, d, 0], out["std"][e, d, 0] = mean_e[e], spread
            incumbent[e] = start
            incumbent[e, cols] = mean_e[e]
        for g in range(G):
            union = np.zeros((E * Cn, 6), np.float64)                       # an ended env's block: zero rows, never read
            offs = {}
            for e in live:
                cand, offs[e] = swarm_search_candidates(out["mean"][e, d, g], out["std"][e, d, g], z[d, g], lo, hi, start[2], incumbent[e])
                union[e * Cn:(e + 1) * Cn] = cand
            played = swarm_rules(engine, union, H)
            for e in live:
                cand = union[e * Cn:(e + 1) * Cn]
                assert played["offsets"][e * Cn:(e + 1) * Cn].tobytes() == offs[e].tobytes()       # step 4 gives the table's own bytes
                for c in range(Cn):
                    out["scores"][e, d, g, c] = _sum_in_order(played["rewards"][e, e * Cn + c], played["length"][e, e * Cn + c])
                out["candidates"][e, d, g] = cand
                out["order"][e, d, g], out["mean"][e, d, g + 1], out["std"][e, d, g + 1] = swarm_search_refit(out["scores"][e, d, g], cand, M, floor)
                incumbent[e] = cand[out["order"][e, d, g, 0]]
        for e in live:                                                      # 5 choose
            best = -1
            for i in range(R):
                if best < 0 or out["lib_scores"][e, d, i] > out["lib_scores"][e, d, best]:
                    best = i
            c0 = int(out["order"][e, d, G - 1, 0])
            if best < 0 or out["scores"][e, d, G - 1, c0] > out["lib_scores"][e, d, best]:
                out["choices"][e, d] = R
                out["chosen_rules"][e, d], out["chosen_offsets"][e, d] = incumbent[e, :3], offs[e][c0]
                chosen[e] = incumbent[e]
                mean_e[e] = incumbent[e, cols]
            else:
                out["choices"][e, d] = best
                out["chosen_rules"][e, d], out["chosen_offsets"][e, d] = r[best, :3], lib_off[best]
                chosen[e] = r[best]
        commit = swarm_rules(engine, chosen, K, keep_actions=True)["actions"]       # (E, E, K, 10, 2)
        for k in range(min(K, T - t)):                                      # 6 commit
            act = np.zeros((E, N_AGENTS, 2), np.float64)
            act[live] = commit[live, live, k]
            act[~alive] = 0.0
            engine.swarm_step_f64(act)
            rew, done = engine.read("reward_f64"), engine.read("done")
            if t_env >= 0 and alive[t_env] and not done[t_env]:
                # the env's positions after the step: its own unless the step ended the episode and the engine reset it
                out["trace_x"][t] = engine.get_state("SWARM_X")[t_env]
                out["trace_xa"][t] = engine.get_state("SWARM_XA")[t_env]
            for e in np.flatnonzero(alive):
                out["rewards"][e, t] = rew[e]
                if keep_actions:
                    out["actions"][e, t] = act[e]
                out["length"][e] = t + 1
                if done[e]:
                    out["finished"][e] = 1
                    alive[e] = False
            t += 1
    return _summary(out, R)
