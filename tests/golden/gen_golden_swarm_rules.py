#!/usr/bin/env python3
"""Golden fixture for the feedback-rule baseline of the Swarm env (goldsrl/baselines.py:SwarmRuleBaseline), made as
gen_golden_ticker_rules.py makes its own: the UNMODIFIED reference SwarmEnv (fed_gym/envs/multiagent.py) under the stand-ins of
_ref_stubs.py.  Build container only:
    python tests/golden/gen_golden_swarm_rules.py

The reference has no feedback rule; what it pins here is the env the rules are played on.  The rule (include/goldsrl_swarmrules.h)
is written out below in numpy float64, one operation per line, on the positions the env holds before the step; the clip is the
float64 form of SwarmRunner.transform_actions_for_env (agents/paac/emulator_runner.py:113-118).

Recorded for SwarmEnv(seed=192) -- the episode of Swarm-eval-v0 -- and the default rules, 128 steps each: the state after the reset
(x, xa, the agent and particle noise rows in use), the rules and their offset tables, per rule the actions, the rewards, the length
and the total.  Asserted: drift and hold total what the all-zero and the (-1, 0) scripts total, the best rule's total exceeds
hold's by more than 100, and the best and second-best totals are further apart than twice the device test's bound (rtol 1e-10 of
the total, tests/test_gpu_swarm_replay.py's fixture case) -- else the runner-up leaves the recorded set."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_stubs  # noqa: E402

_ref_stubs.install()

from fed_gym.envs import multiagent  # noqa: E402

SEED, STEPS = 192, 128
TOTAL_RTOL = 1e-10        # the device test's bound on a total


def default_rules():
    rows = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0)]
    rows += [(1, g, 0, ox, oy, r) for g in (5, 20) for (ox, oy) in ((0, 0), (-0.5, 0.5), (-1, 1), (-1.5, 1.5)) for r in (0.7, 1.0)]
    rows += [(1, 5, 1, 0, 0, 0), (1, 5, 1, 0.3, -0.3, 0)]
    return np.array(rows, np.float64)


def rule_offsets(rule):
    off = np.zeros((10, 2))
    for a in range(10):
        ang = 2.0 * np.pi * a / 10
        off[a, 0] = rule[3] + rule[5] * np.cos(ang)
        off[a, 1] = rule[4] + rule[5] * np.sin(ang)
    return off


def rule_action(rule, off, x, xa):
    """(10, 2) float64 action rows of `rule` on locusts x (80, 2) and agents xa (10, 2)"""
    cancel, gain, anchor = np.float64(rule[0]), np.float64(rule[1]), int(rule[2])
    out = np.zeros((10, 2))
    for a in range(10):
        if anchor == 0:
            cx = np.float64(0.0)
            cy = np.float64(0.0)
            for j in range(80):
                cx = cx + x[j, 0]
                cy = cy + x[j, 1]
            cx = cx / 80.0
            cy = cy / 80.0
        else:
            best = None
            for j in range(80):
                dx = x[j, 0] - xa[a, 0]
                dy = x[j, 1] - xa[a, 1]
                sx = dx * dx
                sy = dy * dy
                d2 = sx + sy
                if best is None or d2 < best:
                    best, cx, cy = d2, x[j, 0], x[j, 1]
        tx = cx + off[a, 0]
        ty = cy + off[a, 1]
        ex = tx - xa[a, 0]
        ey = ty - xa[a, 1]
        gx = gain * ex
        ax = gx - cancel
        ay = gain * ey
        qx = ax * ax
        qy = ay * ay
        s = qx + qy
        d = np.sqrt(s)
        if d >= 1.0:
            ax = ax / d
            ay = ay / d
        out[a, 0], out[a, 1] = ax, ay
    return out


def play(choose, steps=STEPS):
    """One episode of the reference env from its seeded reset: choose(x, xa) -> (10, 2).  Returns the reset state, the actions, the
    rewards (zero past the length) and the length."""
    env = multiagent.SwarmEnv(seed=SEED)
    env.reset()
    start = dict(x=env.states[0].copy(), xa=env.states[1].copy(), agent_noise_row=env.agent_noise[env.t].copy(),
                 particle_noise_row=env.particle_noise[env.t].copy())
    actions, rewards, length = np.zeros((steps, 10, 2)), np.zeros(steps), 0
    for t in range(steps):
        act = np.array(choose(env.states[0], env.states[1]), np.float64)
        actions[t] = act
        _, r, done, _ = env.step(act.copy())
        rewards[t] = r
        length = t + 1
        if done:
            break
    assert np.isfinite(rewards).all() and np.isfinite(actions).all()
    return start, actions, rewards, length


def main():
    rules = default_rules()
    offsets = np.array([rule_offsets(r) for r in rules])
    res = [play(lambda x, xa, r=r, o=o: rule_action(r, o, x, xa)) for r, o in zip(rules, offsets)]
    start = res[0][0]
    for s, _, _, _ in res:
        for k in start:
            assert np.array_equal(s[k], start[k]), k
    totals = np.array([np.sum(r[2][:r[3]]) for r in res])
    # drift and hold are the two scripts of ScriptedSwarmBaseline
    for i, row in ((0, (0.0, 0.0)), (1, (-1.0, 0.0))):
        _, acts, rew, n = play(lambda x, xa, row=row: np.tile(np.array(row), (10, 1)))
        assert n == res[i][3] and np.array_equal(rew, res[i][2]), i
        assert np.array_equal(res[i][1], acts)                  # == : a drift row may hold -0.0
    for i, t in enumerate(totals):
        print("rule %2d %-34s length %3d total %.6f" % (i, tuple(float(v) for v in rules[i]), res[i][3], t))
    keep = list(range(len(rules)))
    order = sorted(keep, key=lambda i: -totals[i])
    while abs(totals[order[0]] - totals[order[1]]) <= 2 * TOTAL_RTOL * abs(totals[order[0]]):
        print("dropping the runner-up, rule", order[1])
        keep.remove(order[1])
        order = sorted(keep, key=lambda i: -totals[i])
    assert 0 in keep and 1 in keep
    assert totals[order[0]] - totals[1] > 100, (totals[order[0]], totals[1])
    out = dict(start)
    out["rules"], out["offsets"] = rules[keep], offsets[keep]
    out["actions"] = np.array([res[i][1] for i in keep])
    out["rewards"] = np.array([res[i][2] for i in keep])
    out["length"] = np.array([res[i][3] for i in keep], np.int32)
    out["total"] = totals[keep]
    out["best_index"] = np.array(int(np.argmax(out["total"])))
    print("best rule", int(out["best_index"]), tuple(float(v) for v in out["rules"][int(out["best_index"])]), "total", out["total"].max(), "hold", totals[1])
    path = os.path.join(HERE, "swarm_rules.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
