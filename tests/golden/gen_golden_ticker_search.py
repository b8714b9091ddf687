#!/usr/bin/env python3
"""Golden fixture for the cross-entropy search over the six numbers of a Ticker rule (goldsrl/baselines.py:TickerRuleSearch), made
as gen_golden_ticker_rules.py makes its own: the UNMODIFIED reference TickerEnv under the stand-ins of _ref_stubs.py, through that
generator's make_env / play.  Build container only:
    python tests/golden/gen_golden_ticker_search.py

The reference has no search; what it pins here is the env the candidates are played on.  The scheme's statements
(include/goldsrl_tickersearch.h) are the numpy functions of goldsrl/_ffi_tickersearch.py, imported, not copied; the rule is
gen_golden_ticker_rules.py's rule_action.

Played on the table and the window starts (0, 123, 376) of ticker_rules.npz, 256 steps: start (1, 0, 0, 1, 0.5, 8), G = 4 generations
of C = 12 candidates, K = 4 elites, spread (0.2, 0.2, 0.2, 0.2, 0.1, 3), floor (0.01, 0.01, 0.01, 0.01, 0.005, 0.5), box
[0, 1]^4 x [0, 0.5] x [0, 64], normals of np.random.default_rng(SEED), stored.  A fit is the mean over the three starts (adds in
order, one division) of the sequential float64 sum of the reference's float64 step rewards.  Recorded: candidates, fit, order,
mean, std.  Asserted: in every generation any two fits among ranks 0..K are either bit-equal with identical recorded actions or
further apart than twice the device test's bound on a mean total (256 steps x 2e-7) -- the condition under which the device's
order[:, :K] and with it every later table may be compared exactly.  If a seed fails it, take another one."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "golds-rl-gym_amd"))
import gen_golden_ticker_rules as R  # noqa: E402  (installs the stand-ins and imports the reference env)
from goldsrl import _ffi_tickersearch as S  # noqa: E402  (the numpy statements; no library is loaded)

STEPS = R.STEPS
SEED = 0
GENERATIONS, CANDIDATES, ELITES = 4, 12, 4
START = np.array((1, 0, 0, 1, 0.5, 8), np.float32)
SPREAD = np.array([0.2, 0.2, 0.2, 0.2, 0.1, 3.0])
FLOOR = np.array([0.01, 0.01, 0.01, 0.01, 0.005, 0.5])
LO = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
HI = np.array([1.0, 1.0, 1.0, 1.0, 0.5, 64.0])
BOUND = STEPS * 2e-7


def main():
    fixed = np.load(os.path.join(HERE, "ticker_rules.npz"))
    matrix, starts = fixed["matrix"], fixed["starts"]
    Gn, C, K = GENERATIONS, CANDIDATES, ELITES
    z = np.random.default_rng(SEED).standard_normal((Gn, C, 6))
    out = {"start": START, "normals": z, "shape": np.array((Gn, C, K), np.int32), "steps": np.array(STEPS, np.int32), "starts": starts,
           "spread": SPREAD, "floor": FLOOR, "lo": LO, "hi": HI,
           "candidates": np.zeros((Gn, C, 6), np.float32), "fit": np.zeros((Gn, C)), "order": np.zeros((Gn, C), np.int32),
           "mean": np.zeros((Gn + 1, 6)), "std": np.zeros((Gn + 1, 6)), "min_gap": np.zeros(Gn)}
    out["mean"][0] = S.ticker_search_start(START, LO, HI)
    out["std"][0] = SPREAD
    played = {}

    def episode(row):
        """(fit, actions (3, STEPS, 4)) of a float32 row, played once"""
        key = row.tobytes()
        if key not in played:
            f, acts = np.float64(0.0), []
            for st in starts:
                a, rewards, _, n = R.play(matrix, int(st), row, STEPS)
                s = np.float64(0.0)
                for t in range(n):
                    s = s + rewards[t]
                f = f + s
                acts.append(a)
            played[key] = (f / np.float64(len(starts)), np.stack(acts))
        return played[key]

    incumbent = None
    for g in range(Gn):
        rows = S.ticker_search_candidates(out["mean"][g], out["std"][g], z[g], LO, HI, incumbent)
        S.check_ticker_rules(rows)
        fit = np.array([episode(r)[0] for r in rows])
        order, mean, std = S.ticker_search_refit(fit, rows, K, FLOOR)
        gaps = []
        for i in range(K + 1):
            for j in range(i + 1, K + 1):
                a, b = order[i], order[j]
                if fit[a] == fit[b]:
                    assert episode(rows[a])[1].tobytes() == episode(rows[b])[1].tobytes(), (g, a, b)
                else:
                    gaps.append(abs(fit[a] - fit[b]))
                    assert gaps[-1] > 2 * BOUND, (g, a, b, fit[a], fit[b])
        out["min_gap"][g] = min(gaps) if gaps else np.inf
        out["candidates"][g], out["fit"][g], out["order"][g], out["mean"][g + 1], out["std"][g + 1] = rows, fit, order, mean, std
        incumbent = rows[order[0]].copy()
        print("generation %d: best %.6f at %s, smallest gap among ranks 0..K %.3g against %.3g"
              % (g, fit[order[0]], np.round(incumbent.astype(np.float64), 4).tolist(), out["min_gap"][g], 2 * BOUND), flush=True)
    assert np.isfinite(out["fit"]).all() and (np.diff(out["fit"][np.arange(Gn), out["order"][:, 0]]) >= 0).all()
    path = os.path.join(HERE, "ticker_search.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
