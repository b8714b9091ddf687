#!/usr/bin/env python3
"""Golden fixture for the receding-horizon rule planner of the Swarm env (goldsrl/baselines.py:SwarmRulePlanner), made as
gen_golden_swarm_rules.py makes its own: the UNMODIFIED reference SwarmEnv (fed_gym/envs/multiagent.py) under the stand-ins of
_ref_stubs.py.  Build container only:
    python tests/golden/gen_golden_swarm_plan.py

The reference has no planner; what it pins here is the env the plan is played on.  The scheme (include/goldsrl_swarmplan.h) is
written out below: at every decision each default rule plays min(H, 128 - t) steps ahead from the env's state (SwarmEnv.t stays at
10 after the burn-in, so the env is deterministic from a state and the lookahead restores it afterwards), score = a sequential
float64 sum, the first rule with the largest score is committed for K steps.  The rule and the default table are
gen_golden_swarm_rules.py's.

Recorded for SwarmEnv(seed=192) -- the episode of Swarm-eval-v0 --, 128 steps, (H, K) = (4, 1) and (8, 4): per decision the choice,
the scores and the relative gap between the best and the second score, per step the reward, and the total.  Asserted: every gap is
at least 1e-6 -- the condition under which the device's choices may be compared exactly: three orders above the 1e-9 its rewards
are held to on this episode -- and both totals exceed the best fixed rule's (swarm_rules.npz) by more than 10."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_swarm_rules as G  # noqa: E402  (installs the stand-ins and imports the reference env)

STEPS = G.STEPS
CASES = ((4, 1), (8, 4))
MIN_GAP = 1e-6


def plan(H, K, rules, offsets):
    env = G.multiagent.SwarmEnv(seed=G.SEED)
    env.reset()
    D = (STEPS + K - 1) // K
    choices, scores, gaps = np.full(D, -1, np.int32), np.zeros((D, len(rules))), np.zeros(D)
    rewards, t, over = np.zeros(STEPS), 0, False
    for d in range(D):
        if over:
            break
        x0, xa0 = env.states[0].copy(), env.states[1].copy()
        for i, (r, o) in enumerate(zip(rules, offsets)):
            env.states = [x0.copy(), xa0.copy()]
            s = np.float64(0.0)
            for k in range(min(H, STEPS - t)):
                _, rew, done, _ = env.step(G.rule_action(r, o, env.states[0], env.states[1]))
                s = s + rew
                if done:
                    break
            scores[d, i] = s
        env.states = [x0.copy(), xa0.copy()]
        c = int(np.argmax(scores[d]))                           # the first index of the largest
        choices[d] = c
        top = np.sort(scores[d])[::-1]
        gaps[d] = (top[0] - top[1]) / abs(top[0])
        for k in range(min(K, STEPS - t)):
            _, rew, done, _ = env.step(G.rule_action(rules[c], offsets[c], env.states[0], env.states[1]))
            rewards[t] = rew
            t += 1
            if done or t >= STEPS:
                over = True
                break
    assert np.isfinite(rewards).all() and np.isfinite(scores).all()
    return dict(choices=choices, scores=scores, gaps=gaps, rewards=rewards, length=np.array(t, np.int32), total=np.sum(rewards[:t]))


def main():
    rules = G.default_rules()
    offsets = np.array([G.rule_offsets(r) for r in rules])
    best_fixed = np.load(os.path.join(HERE, "swarm_rules.npz"))["total"].max()
    out = {"rules": rules, "cases": np.array(CASES, np.int32), "best_fixed_total": np.array(best_fixed)}
    for H, K in CASES:
        p = plan(H, K, rules, offsets)
        n = int((p["choices"] >= 0).sum())
        print("(H, K) = (%d, %d): length %d, total %.6f (%+.6f on the best fixed rule %.6f), %d decisions, rules chosen %s, smallest gap %.3g"
              % (H, K, int(p["length"]), p["total"], p["total"] - best_fixed, best_fixed, n, sorted(set(p["choices"][:n].tolist())),
                 p["gaps"][:n].min()))
        assert (p["gaps"][:n] >= MIN_GAP).all(), p["gaps"][:n].min()
        assert p["total"] - best_fixed > 10, (p["total"], best_fixed)
        for k, v in p.items():
            out["%s_%d_%d" % (k, H, K)] = v
    path = os.path.join(HERE, "swarm_plan.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
