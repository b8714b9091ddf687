#!/usr/bin/env python3
"""Golden fixture for the search planner of the Swarm env (goldsrl/baselines.py:SwarmSearchPlanner), made as
gen_golden_swarm_plan.py makes its own: the UNMODIFIED reference SwarmEnv (fed_gym/envs/multiagent.py) under the stand-ins of
_ref_stubs.py.  Build container only:
    python tests/golden/gen_golden_swarm_cemplan.py

The reference has no planner and no search; what it pins here is the env the plan is played on.  The scheme
(include/goldsrl_swarmcemplan.h) is written out below in numpy float64, one operation per statement: at every decision G generations
of C candidates around the env's mean (the spread reset to the default, candidate 0 the incumbent), every candidate and every
default rule played min(H, 128 - t) steps ahead from the env's state (SwarmEnv.t stays at 10 after the burn-in, so the env is
deterministic from a state and the lookahead restores it afterwards), score = a sequential float64 sum, rank and refit over M
elites; the searched rule is committed for K steps if its score is strictly above the library's best, else the first library rule
with the largest score.  The rule, its offsets and the default table are gen_golden_swarm_rules.py's; candidates and refit are
gen_golden_swarm_search.py's.

Played on SwarmEnv(seed=192) -- the episode of Swarm-eval-v0 --, 128 steps: the 20 default rules, start at the best default rule of
swarm_rules.npz, the default spreads and box, (H, K, G, C, M) = (8, 4, 2, 12, 4), normals
np.random.default_rng(0).standard_normal((32, 2, 12, 5)), stored.  Recorded per decision: the choice, the library scores, candidates,
scores, order, mean, std and the three gaps; per step the reward; the total.  Asserted: at every decision and in every generation the
best-to-second gap and the gap across the elite boundary, and at every decision the gap between the best library score and the
searched score, are at least 1e-6 relative OR AN EXACT TIE OF TWO RULES THAT ACT ALIKE -- the condition under which the device's
choices, first ranks and elite sets may be compared exactly -- and the total exceeds swarm_plan.npz's total_8_4 by more than 5.

Why the exact ties are admitted, and why no other seed of the normals is taken: they are structural.  Once the swarm is in place
the best the family has is `hold`, gain 0; the search finds it, the env's mean gain becomes 0, the spread is reset to 2 at the next
decision, and about half of the candidates are clamped to gain = lo = 0.  A rule with gain 0 acts by a = 0 * e - (cancel, 0): its
action is (-cancel, +-0) whatever its anchor, offsets and radius, so all such candidates and the library's `hold` play the same
episode and score the same bits, here and on the device alike, and both sides break the tie by the smaller index (the library on a
tie with the searched rule).  Every seed gives such decisions.  What could make the device differ is a NEAR tie, and those stay
excluded: a gap of zero is admitted only between two rows whose gain is 0 and whose cancel is equal (`acts_alike`), every other gap
must be at least 1e-6.  `tied` records which gaps were admitted that way."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_swarm_rules as G  # noqa: E402  (installs the stand-ins and imports the reference env)
import gen_golden_swarm_search as S  # noqa: E402

STEPS = G.STEPS
H, K, GENERATIONS, CANDIDATES, ELITES = 8, 4, 2, 12, 4
NORMALS_SEED = 0
MIN_GAP = 1e-6
MIN_GAIN = 5.0


def lookahead(env, x0, xa0, rule, off, n):
    """s = 0.0; s = s + r_t over up to n steps of the rule from (x0, xa0), ended by done"""
    env.states = [x0.copy(), xa0.copy()]
    s = np.float64(0.0)
    for _ in range(n):
        _, rew, done, _ = env.step(G.rule_action(rule, off, env.states[0], env.states[1]))
        s = s + rew
        if done:
            break
    return s


def acts_alike(a, b):
    """two six-number rows whose actions are the same whatever the state: equal rows, or gain 0 on both and the same cancel"""
    return bool(np.array_equal(a, b) or (a[1] == 0.0 and b[1] == 0.0 and a[0] == b[0]))


def main():
    fixed = np.load(os.path.join(HERE, "swarm_rules.npz"))
    start = fixed["rules"][int(fixed["best_index"])].copy()
    rules = G.default_rules()
    offsets = np.array([G.rule_offsets(r) for r in rules])
    plan_total = float(np.load(os.path.join(HERE, "swarm_plan.npz"))["total_8_4"])
    R, Gn, C, M = len(rules), GENERATIONS, CANDIDATES, ELITES
    D = (STEPS + K - 1) // K
    z = np.random.default_rng(NORMALS_SEED).standard_normal((D, Gn, C, 5))
    out = {"rules": rules, "start": start, "normals": z, "shape": np.array((H, K, Gn, C, M), np.int32), "plan_total": np.array(plan_total),
           "choices": np.full(D, -1, np.int32), "lib_scores": np.zeros((D, R)), "candidates": np.zeros((D, Gn, C, 6)),
           "scores": np.zeros((D, Gn, C)), "order": np.zeros((D, Gn, C), np.int32), "mean": np.zeros((D, Gn + 1, 5)),
           "std": np.zeros((D, Gn + 1, 5)), "gaps": np.zeros((D, Gn, 2)), "choice_gaps": np.zeros(D), "tied": np.zeros((D, Gn, 2), bool), "choice_tied": np.zeros(D, bool),
           "rewards": np.zeros(STEPS)}
    env = G.multiagent.SwarmEnv(seed=G.SEED)
    env.reset()
    mean_e = S.first_min(S.first_max(start[S.COLS], S.LO), S.HI)
    t, over = 0, False
    for d in range(D):
        if over:
            break
        x0, xa0 = env.states[0].copy(), env.states[1].copy()
        n = min(H, STEPS - t)
        for i in range(R):
            out["lib_scores"][d, i] = lookahead(env, x0, xa0, rules[i], offsets[i], n)
        out["mean"][d, 0], out["std"][d, 0] = mean_e, S.SPREAD
        incumbent = start.copy()
        incumbent[S.COLS] = mean_e
        for g in range(Gn):
            cand = S.candidates(out["mean"][d, g], out["std"][d, g], z[d, g], start[2], incumbent)
            sc = np.array([lookahead(env, x0, xa0, c, G.rule_offsets(c), n) for c in cand])
            order, mean, std = S.refit(sc, cand, M)
            srt = sc[order]
            out["gaps"][d, g] = ((srt[0] - srt[1]) / abs(srt[0]), (srt[M - 1] - srt[M]) / abs(srt[M - 1]))
            out["tied"][d, g] = (srt[0] == srt[1] and acts_alike(cand[order[0]], cand[order[1]]),
                                 srt[M - 1] == srt[M] and acts_alike(cand[order[M - 1]], cand[order[M]]))
            out["candidates"][d, g], out["scores"][d, g], out["order"][d, g], out["mean"][d, g + 1], out["std"][d, g + 1] = cand, sc, order, mean, std
            incumbent = cand[order[0]].copy()
        env.states = [x0.copy(), xa0.copy()]
        best = 0
        for i in range(1, R):
            if out["lib_scores"][d, i] > out["lib_scores"][d, best]:
                best = i
        s_lib, s_found = out["lib_scores"][d, best], out["scores"][d, Gn - 1, out["order"][d, Gn - 1, 0]]
        out["choice_gaps"][d] = abs(s_found - s_lib) / abs(s_lib)
        out["choice_tied"][d] = s_found == s_lib and acts_alike(incumbent, rules[best])
        if s_found > s_lib:
            out["choices"][d] = R
            rule, off = incumbent, G.rule_offsets(incumbent)
            mean_e = incumbent[S.COLS].copy()
        else:
            out["choices"][d] = best
            rule, off = rules[best], offsets[best]
        for k in range(min(K, STEPS - t)):
            _, rew, done, _ = env.step(G.rule_action(rule, off, env.states[0], env.states[1]))
            out["rewards"][t] = rew
            t += 1
            if done or t >= STEPS:
                over = True
                break
        print("decision %2d: choice %2d, searched %.6f against library %.6f, gaps %.3g %.3g %.3g" % (
            d, out["choices"][d], s_found, s_lib, out["gaps"][d, :, 0].min(), out["gaps"][d, :, 1].min(), out["choice_gaps"][d]), flush=True)
    n_dec = int((out["choices"] >= 0).sum())
    assert np.isfinite(out["rewards"]).all() and np.isfinite(out["scores"]).all() and np.isfinite(out["lib_scores"]).all()
    assert ((out["gaps"][:n_dec] >= MIN_GAP) | out["tied"][:n_dec]).all(), out["gaps"][:n_dec][~out["tied"][:n_dec]].min()
    assert ((out["choice_gaps"][:n_dec] >= MIN_GAP) | out["choice_tied"][:n_dec]).all(), out["choice_gaps"][:n_dec][~out["choice_tied"][:n_dec]].min()
    out["length"] = np.array(t, np.int32)
    out["total"] = np.sum(out["rewards"][:t])
    gp, tg = out["gaps"][:n_dec], out["tied"][:n_dec]
    print("length %d, total %.6f, rule planner (8, 4) %.6f: %+.6f; %d of %d decisions searched; smallest gaps that are no admitted tie "
          "%.3g (first rank) %.3g (elite boundary) %.3g (choice); admitted ties %d, %d, %d"
          % (t, out["total"], plan_total, out["total"] - plan_total, int((out["choices"] == R).sum()), n_dec,
             gp[:, :, 0][~tg[:, :, 0]].min(), gp[:, :, 1][~tg[:, :, 1]].min(), out["choice_gaps"][:n_dec][~out["choice_tied"][:n_dec]].min(),
             tg[:, :, 0].sum(), tg[:, :, 1].sum(), out["choice_tied"][:n_dec].sum()))
    assert out["total"] - plan_total > MIN_GAIN, (out["total"], plan_total)
    path = os.path.join(HERE, "swarm_cemplan.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
