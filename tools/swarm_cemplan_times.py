"""The search planner of the Swarm env in one call (include/goldsrl_swarmcemplan.h) next to the host composition it replaces and
the rule planner it is built on, measured in the same run.  20 default rules, start at the best default rule of the handle's envs,
default spreads and box, 128 steps, (H, K, G, C, M) = (8, 4, 2, 12, 4) and (32, 8, 2, 16, 4), at 1 and 64 envs:

  (a) grl_swarm_cemplan, one call: per decision 2 G + 2 kernels on the handle's stream, nothing read back between them; ms by HIP
      events on the stream around the call (uploads and memsets included, reads not), median and spread (min, max) of the runs after
      the warm-up, every run from a reset handle (GRL_F_RESEED_EACH_RESET: the same state every time);
  (b) swarm_cemplan_host on the same handle.  WALL CLOCK, ONE RUN; its outputs are compared with (a)'s as bytes;
  (c) grl_swarm_plan at the same (H, K) over the same rules on the same handle, HIP events as (a): the parent's code, unchanged.
      The code predicts (a) / (c) = (G H + K) / (H + K), the ratio of the two chains of dependent steps;
  (d) beside the times the totals (means over the handle's envs): the best default rule's, the rule planner's at (H, K), the search
      planner's, and how many decisions committed a searched rule;
  (e) the fixture (tests/golden/swarm_cemplan.npz): the device's total and choices on the reference's seed-192 episode beside it.
The 64 envs of seed 1692 are the 64 other seeds of profiles/swarm_search_times.json (best default rule -95.14, tuned rule -89.22,
rule planner (32, 8) -83.28 there).

    python tools/swarm_cemplan_times.py [--runs 5] [--warmup 1] [--json OUT]

Default output: profiles/swarm_cemplan_times.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_swarmcemplan as CP, _ffi_swarmplan as P, _ffi_swarmrules as R  # noqa: E402
from goldsrl.baselines import DEFAULT_SWARM_RULES, select_best_swarm_rule  # noqa: E402

STEPS = 128
ENVS = (1, 64)
SETTINGS = ((8, 4, 2, 12, 4), (32, 8, 2, 16, 4))
SAME = ("rewards", "length", "finished", "choices", "chosen_rules", "chosen_offsets", "lib_scores", "candidates", "scores", "order", "mean", "std")
# hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -Rpass-analysis=kernel-resource-usage csrc/swarm_cemplan.hip
RESOURCES = {"swarm_cemplan_update_kernel": {"vgprs": 52, "sgprs": 91, "scratch_bytes": 0, "lds_bytes": 12376, "lanes": "C rounded up to 64"},
             "swarm_plan_kernel<MATH_EXACT, lookahead, per env>": {"vgprs": 118, "scratch_bytes": 0, "lds_bytes": 8912, "waves_per_simd": 4},
             "swarm_plan_kernel<MATH_FAST, lookahead, per env>": {"vgprs": 122, "scratch_bytes": 0, "lds_bytes": 8912, "waves_per_simd": 4},
             "swarm_plan_kernel<MATH_REFDIV, lookahead, per env>": {"vgprs": 118, "scratch_bytes": 0, "lds_bytes": 8912, "waves_per_simd": 4},
             "swarm_plan_kernel<MATH_EXACT, commit, per env>": {"vgprs": 140, "scratch_bytes": 0, "lds_bytes": 10192, "waves_per_simd": 3},
             "swarm_plan_kernel<MATH_FAST, commit, per env>": {"vgprs": 144, "scratch_bytes": 0, "lds_bytes": 10192, "waves_per_simd": 3},
             "swarm_plan_kernel<MATH_REFDIV, commit, per env>": {"vgprs": 156, "scratch_bytes": 0, "lds_bytes": 10192, "waves_per_simd": 3}}


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def repeat(eng, fn, runs, warmup):
    ms = []
    for i in range(warmup + runs):
        eng.reset()
        eng.timer_start()
        fn()
        eng.timer_stop()
        t = eng.timer_ms()
        eng.wait()
        if i >= warmup:
            ms.append(t)
    return dict(stat(ms), clock="HIP events")


def case(E, setting, runs, warmup):
    H, K, G, C, M = setting
    lib = _ffi.load_library(extra_signatures=dict(CP.SWARMCEMPLAN_SIGNATURES, **P.SWARMPLAN_SIGNATURES))
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=1692, flags=_ffi.F_SWARM_NO_OBSERVE | _ffi.F_RESEED_EACH_RESET, max_episode_steps=STEPS)
    rules = R.check_swarm_rules(DEFAULT_SWARM_RULES)
    n = len(rules)
    eng.reset()
    best, six, best_total = select_best_swarm_rule(rules, R.swarm_rules(eng, rules, STEPS)["totals"])
    D = (STEPS + K - 1) // K
    r = {"case": "the search planner in one call", "envs": E, "horizon": H, "replan": K, "generations": G, "candidates": C, "elites": M,
         "rules": n, "steps": STEPS, "runs": runs, "warmup": warmup, "kernels": D * (2 * G + 2),
         "start": {"rule": best, "six": six, "mean_total": best_total}}
    start = np.array(six)
    z = np.ascontiguousarray(np.random.default_rng(0).standard_normal((D, G, C, 5)))
    head, off = np.ascontiguousarray(rules[:, :3]), np.ascontiguousarray(R.swarm_rule_offsets(rules))
    from goldsrl import _ffi_swarmsearch as S
    five = [np.ascontiguousarray(np.array(v, np.float64)) for v in (start[list(S.SEARCH_COLS)], S.DEFAULT_SPREAD, S.DEFAULT_FLOOR, S.DEFAULT_LO, S.DEFAULT_HI)]
    ring = S.swarm_search_ring()

    def one_call():
        eng._check(lib.grl_swarm_cemplan(eng.h, _ffi._ptr(head), _ffi._ptr(off), n, int(start[2]), *([_ffi._ptr(v) for v in five] +
                                         [_ffi._ptr(ring), _ffi._ptr(z), H, K, G, C, M, STEPS, 0, -1])))

    def plan_call():
        eng._check(lib.grl_swarm_plan(eng.h, _ffi._ptr(head), _ffi._ptr(off), n, H, K, STEPS, 0, -1))
    r["ms_one_call"] = repeat(eng, one_call, runs, warmup)
    r["ms_swarm_plan_same_H_K"] = repeat(eng, plan_call, runs, warmup)
    r["one_call_over_swarm_plan"] = r["ms_one_call"]["median"] / r["ms_swarm_plan_same_H_K"]["median"]
    r["predicted_from_the_chains"] = (G * H + K) / float(H + K)
    us_step = r["ms_swarm_plan_same_H_K"]["median"] * 1e3 / (D * (H + K))
    r["us_per_dependent_step_in_swarm_plan"] = us_step
    r["ms_one_call_predicted_from_that"] = D * (G * H + K) * us_step / 1e3
    r["ms_left_for_the_update_launches"] = r["ms_one_call"]["median"] - r["ms_one_call_predicted_from_that"]
    r["us_per_update_launch_if_all_of_it"] = r["ms_left_for_the_update_launches"] * 1e3 / (D * (G + 1))
    eng.reset()
    out = CP.swarm_cemplan(eng, rules, start, H, K, G, C, M, normals=z, max_steps=STEPS)
    plan = P.swarm_plan(eng, rules, H, K, STEPS)
    r["totals"] = {"best_default_rule": best_total, "rule_planner_same_H_K": float(plan["totals"].mean()), "search_planner": float(out["totals"].mean()),
                   "search_planner_minus_rule_planner": float(out["totals"].mean() - plan["totals"].mean()),
                   "decisions": int((out["choices"] >= 0).sum()), "decisions_searched": out["searched"]}
    eng.reset()
    t0 = time.perf_counter()
    host = CP.swarm_cemplan_host(eng, rules, start, H, K, G, C, M, normals=z, max_steps=STEPS)
    sec = time.perf_counter() - t0
    r["host_composition"] = {"clock": "wall clock, ONE run", "ms": sec * 1e3,
                             "bits_equal_to_the_one_call": bool(all(host[k].tobytes() == out[k].tobytes() for k in SAME))}
    r["host_composition_over_one_call"] = sec * 1e3 / r["ms_one_call"]["median"]
    eng.close()
    return r


def fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "swarm_cemplan.npz"))
    s = np.load(os.path.join(ROOT, "tests", "golden", "swarm_rules.npz"))
    eng = _ffi.Engine(_ffi.ENV_SWARM, 1, seed=1, max_episode_steps=STEPS)
    eng.reset()
    for f, k in (("SWARM_X", "x"), ("SWARM_XA", "xa"), ("SWARM_PNOISE", "particle_noise_row"), ("SWARM_ANOISE", "agent_noise_row")):
        eng.set_state(f, np.ascontiguousarray(s[k][None]))
    out = {"case": "the reference's seed-192 episode", "fixture_total_8_4": float(g["total"]), "rule_planner_8_4": float(g["plan_total"]),
           "best_default_rule": float(s["total"].max())}
    for setting in SETTINGS:
        H, K, G, C, M = setting
        z = g["normals"] if setting == tuple(int(v) for v in g["shape"]) else None
        o = CP.swarm_cemplan(eng, g["rules"], g["start"], H, K, G, C, M, normals=z, seed=0, max_steps=STEPS)
        key = "%d_%d_%d_%d_%d" % setting
        out["device_total_" + key] = float(o["totals"][0])
        out["decisions_searched_" + key] = o["searched"]
        if z is not None:
            rel = np.abs(o["rewards"][0] - g["rewards"]) / np.abs(g["rewards"])
            out["choices_equal_the_fixture"] = bool(np.array_equal(o["choices"][0], g["choices"]))
            out["orders_equal_the_fixture"] = bool(np.array_equal(o["order"][0], g["order"]))
            out["largest_relative_reward_deviation"] = float(rel.max())
            out["total_relative_deviation"] = float(abs(o["totals"][0] - g["total"]) / abs(g["total"]))
            tied, ctied = g["tied"], g["choice_tied"]
            out["smallest_gaps_of_the_fixture_that_are_no_admitted_tie"] = [float(g["gaps"][..., 0][~tied[..., 0]].min()),
                                                                             float(g["gaps"][..., 1][~tied[..., 1]].min()),
                                                                             float(g["choice_gaps"][~ctied].min())]
            out["admitted_exact_ties"] = [int(tied[..., 0].sum()), int(tied[..., 1].sum()), int(ctied.sum())]
    eng.close()
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "swarm_cemplan_times.json"))
    a = p.parse_args()
    out = {"times": [], "resources": RESOURCES,
           "recorded_in_swarm_search_times_json_64_envs": {"best_default_rule": -95.14, "tuned_rule": -89.22, "rule_planner_32_8": -83.28}}
    for E in ENVS:
        for setting in SETTINGS:
            out["times"].append(case(E, setting, a.runs, a.warmup))
            print(json.dumps(out["times"][-1]), flush=True)
    out["fixture"] = fixture()
    print(json.dumps(out["fixture"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
