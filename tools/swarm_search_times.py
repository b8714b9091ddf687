"""The cross-entropy search over a Swarm rule's five real numbers in one call (include/goldsrl_swarmsearch.h) next to the host
composition it replaces, measured in the same run.  The search starts from the best default rule of the handle's envs
(goldsrl.baselines.DEFAULT_SWARM_RULES), default spreads, 8 elites, 128 steps, (E, G, C) in (1, 8, 32), (16, 8, 64), (64, 8, 64):

  (a) grl_swarm_search, one call: G evaluations and G + 1 updates on the handle's stream, nothing read back between them; ms by HIP
      events on the stream around the call (the upload of the normals and the memsets included, reads not), median and spread (min,
      max) of the runs after the warm-up, every run from a reset handle (GRL_F_RESEED_EACH_RESET: the same state every time);
  (b) swarm_search_host on the same handle: per generation one grl_swarm_rules over 128 steps, the read of its E * C * 128 rewards,
      as many Python adds, a sort and the refit in numpy.  WALL CLOCK, ONE RUN; its seven outputs are compared with (a)'s as bytes;
  (c) grl_swarm_rules of C rules over 128 steps on the same handle, HIP events: what one generation's evaluation should cost;
  (d) beside the times the totals (means over the handle's envs): the best default rule's, the found rule's, and the planner's
      (horizon 32, replan 8) over the default rules;
  (e) the fixture (tests/golden/swarm_search.npz): per generation the largest relative deviation of the device's fit from it.

    python tools/swarm_search_times.py [--runs 5] [--warmup 1] [--json OUT]

Default output: profiles/swarm_search_times.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_swarmplan as P, _ffi_swarmrules as R, _ffi_swarmsearch as S  # noqa: E402
from goldsrl.baselines import DEFAULT_SWARM_RULES, select_best_swarm_rule  # noqa: E402

STEPS = 128
CASES = ((1, 8, 32), (16, 8, 64), (64, 8, 64))
ELITES = 8
PLAN = (32, 8)
# hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -Rpass-analysis=kernel-resource-usage csrc/swarm_search.hip
RESOURCES = {"swarm_search_update_kernel": {"vgprs": 54, "sgprs": 68, "scratch_bytes": 0, "lds_bytes": 12376, "lanes": 1024},
             "swarm_plan_kernel<MATH_EXACT, lookahead>": {"vgprs": 118, "scratch_bytes": 0, "lds_bytes": 8912, "waves_per_simd": 4},
             "swarm_plan_kernel<MATH_FAST, lookahead>": {"vgprs": 122, "scratch_bytes": 0, "lds_bytes": 8912, "waves_per_simd": 4},
             "swarm_plan_kernel<MATH_REFDIV, lookahead>": {"vgprs": 118, "scratch_bytes": 0, "lds_bytes": 8912, "waves_per_simd": 4}}


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def repeat(eng, fn, runs, warmup):
    ms = []
    for i in range(warmup + runs):
        eng.reset()
        t = timed(eng, fn)
        eng.wait()
        if i >= warmup:
            ms.append(t)
    return dict(stat(ms), clock="HIP events")


def case(E, G, C, runs, warmup):
    lib = _ffi.load_library(extra_signatures=dict(S.SWARMSEARCH_SIGNATURES, **R.SWARMRULES_SIGNATURES))
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=1692, flags=_ffi.F_SWARM_NO_OBSERVE | _ffi.F_RESEED_EACH_RESET, max_episode_steps=STEPS)
    rules = R.check_swarm_rules(DEFAULT_SWARM_RULES)
    eng.reset()
    best, six, best_total = select_best_swarm_rule(rules, R.swarm_rules(eng, rules, STEPS)["totals"])
    r = {"case": "the search in one call", "envs": E, "generations": G, "candidates": C, "elites": ELITES, "steps": STEPS, "runs": runs,
         "warmup": warmup, "kernels": 2 * G + 1, "start": {"rule": best, "six": six, "mean_total": best_total}}
    start = np.array(six)
    z = np.ascontiguousarray(np.random.default_rng(0).standard_normal((G, C, 5)))
    five = [np.ascontiguousarray(np.array(v, np.float64)) for v in (start[list(S.SEARCH_COLS)], S.DEFAULT_SPREAD, S.DEFAULT_FLOOR, S.DEFAULT_LO, S.DEFAULT_HI)]
    ring = S.swarm_search_ring()

    def one_call():
        eng._check(lib.grl_swarm_search(eng.h, int(start[2]), *([_ffi._ptr(v) for v in five] + [_ffi._ptr(ring), _ffi._ptr(z), G, C, ELITES, STEPS])))
    r["ms_one_call"] = repeat(eng, one_call, runs, warmup)
    eng.reset()
    out = S.swarm_search(eng, start, generations=G, candidates=C, elites=ELITES, normals=z, max_steps=STEPS)
    table = R.check_swarm_rules(out["candidates"][G - 1])
    head, off = np.ascontiguousarray(table[:, :3]), np.ascontiguousarray(out["offsets"][G - 1])
    r["ms_swarm_rules_of_C_rules"] = repeat(eng, lambda: eng._check(lib.grl_swarm_rules(eng.h, _ffi._ptr(head), _ffi._ptr(off), C, STEPS, 0, -1)),
                                            runs, warmup)
    r["one_call_over_G_rules_sweeps"] = r["ms_one_call"]["median"] / (G * r["ms_swarm_rules_of_C_rules"]["median"])
    r["found"] = {"six": out["best_rule"], "mean_total": out["best_fit"], "minus_start": out["best_fit"] - best_total,
                  "best_per_generation": out["best_per_generation"].tolist()}
    eng.reset()
    t0 = time.perf_counter()
    host = S.swarm_search_host(eng, start, generations=G, candidates=C, elites=ELITES, normals=z, max_steps=STEPS)
    sec = time.perf_counter() - t0
    r["host_composition"] = {"clock": "wall clock, ONE run", "ms": sec * 1e3,
                             "bits_equal_to_the_one_call": bool(all(host[k].tobytes() == out[k].tobytes() for k in S.OUTPUTS))}
    r["host_composition_over_one_call"] = sec * 1e3 / r["ms_one_call"]["median"]
    eng.reset()
    plan_total = float(P.swarm_plan(eng, rules, PLAN[0], PLAN[1], STEPS)["totals"].mean())
    r["planner"] = {"horizon": PLAN[0], "replan": PLAN[1], "mean_total": plan_total, "minus_found": plan_total - out["best_fit"]}
    eng.close()
    return r


def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "swarm_search.npz"))
    s = np.load(os.path.join(ROOT, "tests", "golden", "swarm_rules.npz"))
    eng = _ffi.Engine(_ffi.ENV_SWARM, 1, seed=1, max_episode_steps=STEPS)
    eng.reset()
    for f, k in (("SWARM_X", "x"), ("SWARM_XA", "xa"), ("SWARM_PNOISE", "particle_noise_row"), ("SWARM_ANOISE", "agent_noise_row")):
        eng.set_state(f, np.ascontiguousarray(s[k][None]))
    Gn, C, K = (int(v) for v in g["shape"])
    out = S.swarm_search(eng, g["start"], generations=Gn, candidates=C, elites=K, normals=g["normals"], max_steps=STEPS)
    eng.close()
    rel = np.abs(out["fit"] - g["fit"]) / np.abs(g["fit"])
    return {"case": "the fixture of the reference env (seed 192)", "generations": Gn, "candidates": C, "elites": K,
            "largest_relative_deviation_of_a_fit_per_generation": rel.max(axis=1).tolist(),
            "candidates_of_generation_0_equal_bytes": bool(out["candidates"][0].tobytes() == g["candidates"][0].tobytes()),
            "orders_equal": bool(np.array_equal(out["order"], g["order"])),
            "best_per_generation": out["best_per_generation"].tolist(), "fixture_best_per_generation": g["fit"][np.arange(Gn), g["order"][:, 0]].tolist(),
            "best_fixed_rule_total": float(g["best_fixed_total"]), "smallest_gaps_of_the_fixture": g["gaps"].min(axis=0).tolist()}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "swarm_search_times.json"))
    a = p.parse_args()
    out = {"times": [], "resources": RESOURCES}
    for E, G, C in CASES:
        out["times"].append(case(E, G, C, a.runs, a.warmup))
        print(json.dumps(out["times"][-1]), flush=True)
    out["fixture"] = fixture()
    print(json.dumps(out["fixture"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
