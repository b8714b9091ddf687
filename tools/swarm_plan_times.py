"""The receding-horizon rule planner of the Swarm env in one call (include/goldsrl_swarmplan.h) next to the host composition it
replaces, measured in the same run.  The default rules (goldsrl.baselines.DEFAULT_SWARM_RULES), 128 steps, (H, K) in (4, 1), (8, 4),
(32, 8), on E envs:

  (a) grl_swarm_plan, one call: 2 * ceil(128 / K) kernels on the handle's stream, nothing read back between them; ms by HIP events
      on the stream around the call (uploads and memsets included, reads not), median and spread (min, max) of the runs after the
      warm-up, every run from a reset handle (GRL_F_RESEED_EACH_RESET: the same state every time);
  (b) at E <= 64, swarm_plan_host on the same handle: per decision one grl_swarm_rules over H steps, its reads, the scores as a Python
      loop, np.argmax and K grl_swarm_step_f64 with their reads.  WALL CLOCK, ONE RUN after a one-decision warm-up; its rewards and
      choices are compared with (a)'s as bytes.  Above 64 envs the Python loop of the scores alone (E * 20 * H adds per decision)
      takes minutes and is not run;
  (c) grl_swarm_rules over 128 steps on the same handle, HIP events: the scale of one whole-episode lookahead;
  (d) one SwarmPolicyMonitor.eval_once on Swarm-eval-v0 (the conv policy, 128 steps) and one plan_baseline() with its two resets and
      reads, wall clock, one run after a warm-up, and the planner's seed-192 totals from the device beside the fixture's
      (tests/golden/swarm_plan.npz).

    python tools/swarm_plan_times.py [--envs 1 64 4096] [--runs 5] [--warmup 1] [--json OUT]

The registers, LDS and scratch of the six instantiations are recorded next to the times.
Default output: profiles/swarm_plan_times.json."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_swarmplan as P, _ffi_swarmrules as R  # noqa: E402
from goldsrl.baselines import DEFAULT_SWARM_RULES  # noqa: E402

STEPS = 128
CASES = ((4, 1), (8, 4), (32, 8))
# hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -Rpass-analysis=kernel-resource-usage csrc/swarm_plan.hip
RESOURCES = {"swarm_plan_kernel<MATH_EXACT, lookahead>": {"vgprs": 118, "scratch_bytes": 0, "lds_bytes": 8912, "waves_per_simd": 4},
             "swarm_plan_kernel<MATH_FAST, lookahead>": {"vgprs": 122, "scratch_bytes": 0, "lds_bytes": 8912, "waves_per_simd": 4},
             "swarm_plan_kernel<MATH_REFDIV, lookahead>": {"vgprs": 118, "scratch_bytes": 0, "lds_bytes": 8912, "waves_per_simd": 4},
             "swarm_plan_kernel<MATH_EXACT, commit>": {"vgprs": 140, "scratch_bytes": 0, "lds_bytes": 10192, "waves_per_simd": 3},
             "swarm_plan_kernel<MATH_FAST, commit>": {"vgprs": 144, "scratch_bytes": 0, "lds_bytes": 10192, "waves_per_simd": 3},
             "swarm_plan_kernel<MATH_REFDIV, commit>": {"vgprs": 156, "scratch_bytes": 0, "lds_bytes": 10192, "waves_per_simd": 3}}


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def case(E, runs, warmup):
    lib = _ffi.load_library(extra_signatures=dict(P.SWARMPLAN_SIGNATURES, **R.SWARMRULES_SIGNATURES))
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=1692, flags=_ffi.F_SWARM_NO_OBSERVE | _ffi.F_RESEED_EACH_RESET, max_episode_steps=STEPS)
    rules = R.check_swarm_rules(DEFAULT_SWARM_RULES)
    n = len(rules)
    head, off = np.ascontiguousarray(rules[:, :3]), np.ascontiguousarray(R.swarm_rule_offsets(rules))
    r = {"case": "the planner in one call", "envs": E, "rules": n, "steps": STEPS, "runs": runs, "warmup": warmup, "plans": []}

    def fixed_rules():
        eng._check(lib.grl_swarm_rules(eng.h, _ffi._ptr(head), _ffi._ptr(off), n, STEPS, 0, -1))
    ms = []
    for i in range(warmup + runs):
        eng.reset()
        t = timed(eng, fixed_rules)
        eng.wait()
        if i >= warmup:
            ms.append(t)
    r["ms_swarm_rules_128_steps"] = dict(stat(ms), clock="HIP events")
    eng.reset()
    r["mean_total_of_best_fixed_rule"] = float(R.swarm_rules(eng, rules, STEPS)["totals"].mean(axis=0).max())
    for H, K in CASES:
        c = {"horizon": H, "replan": K, "decisions": (STEPS + K - 1) // K, "kernels": 2 * ((STEPS + K - 1) // K)}

        def one_call():
            eng._check(lib.grl_swarm_plan(eng.h, _ffi._ptr(head), _ffi._ptr(off), n, H, K, STEPS, 0, -1))
        ms = []
        for i in range(warmup + runs):
            eng.reset()
            t = timed(eng, one_call)
            eng.wait()
            if i >= warmup:
                ms.append(t)
        c["ms_one_call"] = dict(stat(ms), clock="HIP events")
        eng.reset()
        out = P.swarm_plan(eng, rules, H, K, STEPS)
        c["mean_total"] = float(out["totals"].mean())
        c["mean_total_minus_best_fixed_rule"] = c["mean_total"] - r["mean_total_of_best_fixed_rule"]
        if E <= 64:
            P.swarm_plan_host(eng, rules, H, K, K)                          # warm-up: one decision
            eng.reset()
            t0 = time.perf_counter()
            host = P.swarm_plan_host(eng, rules, H, K, STEPS)
            sec = time.perf_counter() - t0
            c["host_composition"] = {"clock": "wall clock, ONE run", "ms": sec * 1e3,
                                     "bits_equal_to_the_one_call": bool(all(host[k].tobytes() == out[k].tobytes()
                                                                            for k in ("rewards", "choices", "scores", "length", "finished")))}
            c["host_composition_over_one_call"] = sec * 1e3 / c["ms_one_call"]["median"]
        r["plans"].append(c)
    eng.close()
    return r


def monitor_for_scale():
    from goldsrl import envs
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import ConvSingleAgentPolicyNetwork
    from goldsrl.agents.state_processors import SwarmStateProcessor
    conf = dict(name='local_learning', num_actions=2, clip_norm=40.0, clip_norm_type='global', device='/gpu:0',
                entropy_regularisation_strength=0.02, scale=1000.0, height=84, width=84, channels=3)
    d = tempfile.mkdtemp()
    learner_eng = _ffi.Engine(_ffi.ENV_SWARM, 2, seed=5)
    learner_eng.reset()
    net = ConvSingleAgentPolicyNetwork(conf).bind(learner_eng, seed=11)
    mon = PM.SwarmPolicyMonitor(envs.make("Swarm-eval-v0"), net, SwarmStateProcessor(grid_size=84), PM.ScalarWriter(os.path.join(d, "eval")),
                                network_conf=conf)
    mon.actions_path = os.path.join(d, "swarm-eval.json")
    mon.eval_once()                                                         # warm-up
    t0 = time.perf_counter()
    total, length, _ = mon.eval_once()
    sec = time.perf_counter() - t0
    r = {"case": "SwarmPolicyMonitor on Swarm-eval-v0", "clock": "wall clock, ONE run after a warm-up", "ms_eval_once": sec * 1e3,
         "episode_length": int(length), "untrained_policy_total_reward": float(total), "plan_baseline": []}
    _, r["best_fixed_rule_total_reward"] = mon.rule_baseline()
    g = np.load(os.path.join(ROOT, "tests", "golden", "swarm_plan.npz"))
    mon.plan_baseline(1, 1)                                                 # warm-up
    for H, K in CASES:
        t0 = time.perf_counter()
        name, plan_total = mon.plan_baseline(H, K)
        sec = time.perf_counter() - t0
        row = {"horizon": H, "replan": K, "ms_with_its_two_resets_and_reads": sec * 1e3, "name": name, "total_reward": float(plan_total)}
        if "total_%d_%d" % (H, K) in g:
            row["fixture_total_reward"] = float(g["total_%d_%d" % (H, K)])
            row["choices_equal_to_the_fixture"] = bool(np.array_equal(mon.baseline_stats["choices"][0], g["choices_%d_%d" % (H, K)]))
        r["plan_baseline"].append(row)
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--envs", type=int, nargs="+", default=[1, 64, 4096])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "swarm_plan_times.json"))
    a = p.parse_args()
    out = {"times": [], "resources": RESOURCES}
    for E in a.envs:
        out["times"].append(case(E, a.runs, a.warmup))
        print(json.dumps(out["times"][-1]), flush=True)
    out["times"].append(monitor_for_scale())
    print(json.dumps(out["times"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
