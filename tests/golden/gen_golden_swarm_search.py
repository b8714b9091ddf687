#!/usr/bin/env python3
"""Golden fixture for the cross-entropy search over a Swarm rule's five real numbers (goldsrl/baselines.py:SwarmRuleSearch), made
as gen_golden_swarm_plan.py makes its own: the UNMODIFIED reference SwarmEnv (fed_gym/envs/multiagent.py) under the stand-ins of
_ref_stubs.py.  Build container only:
    python tests/golden/gen_golden_swarm_search.py

The reference has no search; what it pins here is the env the candidates are played on.  The scheme (include/goldsrl_swarmsearch.h)
is written out below in numpy float64, one operation per statement; the rule and its offsets are gen_golden_swarm_rules.py's.

Played on SwarmEnv(seed=192) -- the episode of Swarm-eval-v0 --, 128 steps: start at the best default rule of swarm_rules.npz, the
default spreads, G = 4 generations of C = 12 candidates, K = 4 elites, normals of np.random.default_rng(0), stored.  Recorded:
candidates, fit, order, mean, std.  Asserted: in every generation the best-to-second gap and the gap across the elite boundary
(ranks K and K + 1) are at least 1e-6 relative -- the condition under which the device's first rank and elite set may be compared
exactly -- and the last generation's best exceeds the best fixed rule of swarm_rules.npz by more than 3."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_swarm_rules as G  # noqa: E402  (installs the stand-ins and imports the reference env)

STEPS = G.STEPS
GENERATIONS, CANDIDATES, ELITES = 4, 12, 4
SPREAD = np.array([0.0, 2.0, 0.5, 0.5, 0.3])
FLOOR = np.array([0.0, 0.05, 0.01, 0.01, 0.01])
LO = np.array([0.0, 0.0, -4.0, -4.0, 0.0])
HI = np.array([1.0, 40.0, 4.0, 4.0, 3.0])
COLS = [0, 1, 3, 4, 5]                     # (cancel, gain, off_x, off_y, radius) in a six-number row
MIN_GAP = 1e-6
MIN_GAIN = 3.0


def first_max(a, b):
    return np.where(a >= b, a, b)


def first_min(a, b):
    return np.where(a <= b, a, b)


def candidates(mean, std, z, anchor, incumbent):
    v = std[None] * z
    v = mean[None] + v
    v = first_max(v, LO[None])
    v = first_min(v, HI[None])
    cand = np.empty((z.shape[0], 6))
    cand[:, COLS] = v
    cand[:, 2] = anchor
    cand[0] = incumbent
    return cand


def refit(fit, cand, K):
    order = np.array(sorted(range(len(fit)), key=lambda c: (-fit[c], c)), np.int32)
    p = cand[order[:K]][:, COLS]
    kk = np.float64(K)
    m = np.zeros(5)
    for i in range(K):
        m = m + p[i]
    mean = m / kk
    s = np.zeros(5)
    for i in range(K):
        d = p[i] - mean
        q = d * d
        s = s + q
    v = s / kk
    sd = np.sqrt(v)
    return order, mean, first_max(sd, FLOOR)


def total(rule):
    off = G.rule_offsets(rule)
    _, _, rewards, n = G.play(lambda x, xa: G.rule_action(rule, off, x, xa))
    s = np.float64(0.0)
    for t in range(n):
        s = s + rewards[t]
    return s


def main():
    fixed = np.load(os.path.join(HERE, "swarm_rules.npz"))
    start = fixed["rules"][int(fixed["best_index"])].copy()
    best_fixed = fixed["total"].max()
    Gn, C, K = GENERATIONS, CANDIDATES, ELITES
    z = np.random.default_rng(0).standard_normal((Gn, C, 5))
    out = {"start": start, "normals": z, "shape": np.array((Gn, C, K), np.int32), "best_fixed_total": np.array(best_fixed),
           "candidates": np.zeros((Gn, C, 6)), "fit": np.zeros((Gn, C)), "order": np.zeros((Gn, C), np.int32),
           "mean": np.zeros((Gn + 1, 5)), "std": np.zeros((Gn + 1, 5)), "gaps": np.zeros((Gn, 2))}
    out["mean"][0] = first_min(first_max(start[COLS], LO), HI)
    out["std"][0] = SPREAD
    incumbent = start.copy()
    incumbent[COLS] = out["mean"][0]
    for g in range(Gn):
        cand = candidates(out["mean"][g], out["std"][g], z[g], start[2], incumbent)
        fit = np.array([total(c) for c in cand])          # one env: the fit is the score (s = 0.0 + score; s / 1.0)
        order, mean, std = refit(fit, cand, K)
        srt = fit[order]
        out["gaps"][g] = ((srt[0] - srt[1]) / abs(srt[0]), (srt[K - 1] - srt[K]) / abs(srt[K - 1]))
        out["candidates"][g], out["fit"][g], out["order"][g], out["mean"][g + 1], out["std"][g + 1] = cand, fit, order, mean, std
        incumbent = cand[order[0]].copy()
        print("generation %d: best %.6f at %s, gap to the second %.3g, across the elite boundary %.3g"
              % (g, srt[0], np.round(incumbent, 4).tolist(), out["gaps"][g, 0], out["gaps"][g, 1]), flush=True)
        assert (out["gaps"][g] >= MIN_GAP).all(), out["gaps"][g]
    assert np.isfinite(out["fit"]).all()
    last = out["fit"][Gn - 1, out["order"][Gn - 1, 0]]
    print("found %.6f, best fixed rule %.6f: %+.6f" % (last, best_fixed, last - best_fixed))
    assert last - best_fixed > MIN_GAIN, (last, best_fixed)
    path = os.path.join(HERE, "swarm_search.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
