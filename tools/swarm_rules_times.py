"""Feedback rules on the Swarm env in one launch (include/goldsrl_swarmrules.h) next to what a user had before, measured in the
same run.  The default rules (goldsrl.baselines.DEFAULT_SWARM_RULES) x 128 steps on E envs:

  (a) grl_swarm_rules, one launch: the action of every step computed in the kernel;
  (b) the same pairs and steps through grl_swarm_replay, the kernel this one was made from, with the actions pre-recorded: env 0's
      rows of (a) shared by every env, so that both calls upload less than half a megabyte and the ratio (a) / (b) is the cost of
      computing the rule in the kernel (the envs other than 0 play other episodes than in (a); the work per step is the same);
  (c) at E <= 64 the only form a feedback rule could take before: per rule and per step one get_state of x and xa, the rule on the
      host (swarm_rule_actions), one swarm_step_f64 and a reward read, on a twin handle without a TimeLimit set to the same state.
      WALL CLOCK, ONE RUN after a one-rule warm-up; its rewards are compared with (a)'s as bytes;
  (d) at one env, 20 rules of one anchor each next to the default set: where the rule's time goes;
  (e) one SwarmPolicyMonitor.eval_once on Swarm-eval-v0 (the conv policy, 128 steps), wall clock, one run after a warm-up: the scale
      of what the baseline stands beside.

    python tools/swarm_rules_times.py [--envs 1 64 4096] [--runs 5] [--warmup 1] [--json OUT]

(a) and (b): every run starts from a reset handle (GRL_F_RESEED_EACH_RESET: the same state every time); ms by HIP events on the
handle's stream around the call (uploads and memsets included, reads not); median and spread (min, max) of the runs, the two
alternating.  The registers and scratch of the three instantiations are recorded next to the times.
Default output: profiles/swarm_rules_times.json."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_replay, _ffi_swarmrules as R  # noqa: E402
from goldsrl.baselines import DEFAULT_SWARM_RULES  # noqa: E402

STEPS = 128
STATE = ("SWARM_X", "SWARM_XA", "SWARM_PNOISE", "SWARM_ANOISE")
# hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -Rpass-analysis=kernel-resource-usage csrc/swarm_rules.hip
RESOURCES = {"swarm_rules_kernel<MATH_EXACT>": {"vgprs": 134, "scratch_bytes": 0, "lds_bytes": 8880, "waves_per_simd": 3},
             "swarm_rules_kernel<MATH_FAST>": {"vgprs": 138, "scratch_bytes": 0, "lds_bytes": 8880, "waves_per_simd": 3},
             "swarm_rules_kernel<MATH_REFDIV>": {"vgprs": 150, "scratch_bytes": 0, "lds_bytes": 8880, "waves_per_simd": 3}}


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def host_in_the_loop(state, rules, offsets, E, n_rules=None):
    """(c): rewards (E, n_rules, STEPS) and the wall-clock seconds"""
    twin = _ffi.Engine(_ffi.ENV_SWARM, E, seed=99, max_episode_steps=0, flags=_ffi.F_SWARM_NO_OBSERVE)
    twin.reset()
    n = len(rules) if n_rules is None else n_rules
    rew = np.zeros((E, n, STEPS))
    t0 = time.perf_counter()
    for r in range(n):
        for f in STATE:
            twin.set_state(f, state[f])
        for t in range(STEPS):
            act = R.swarm_rule_actions(twin.get_state("SWARM_X"), twin.get_state("SWARM_XA"), rules[r], offsets[r])
            twin.swarm_step_f64(np.ascontiguousarray(act))
            rew[:, r, t] = twin.read("reward_f64")
    sec = time.perf_counter() - t0
    twin.close()
    return rew, sec


def case(E, runs, warmup, shared_rows):
    lib = _ffi.load_library(extra_signatures=dict(R.SWARMRULES_SIGNATURES, **_ffi_replay.REPLAY_SIGNATURES))
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=1692, flags=_ffi.F_SWARM_NO_OBSERVE | _ffi.F_RESEED_EACH_RESET, max_episode_steps=STEPS)
    rules = R.check_swarm_rules(DEFAULT_SWARM_RULES)
    n = len(rules)
    head, off = np.ascontiguousarray(rules[:, :3]), np.ascontiguousarray(R.swarm_rule_offsets(rules))
    r = {"case": "rules x steps in one launch", "envs": E, "rules": n, "steps": STEPS, "pairs": E * n, "runs": runs, "warmup": warmup,
         "clock": "HIP events"}

    def by_rules():
        eng._check(lib.grl_swarm_rules(eng.h, _ffi._ptr(head), _ffi._ptr(off), n, STEPS, 0, -1))

    def by_replay():
        eng._check(lib.grl_swarm_replay(eng.h, _ffi._ptr(shared_rows), 1, n, STEPS, None, 0, -1))
    ms = {"ms_rules": [], "ms_replay_of_recorded_actions": []}
    for i in range(warmup + runs):
        for name, fn in (("ms_rules", by_rules), ("ms_replay_of_recorded_actions", by_replay)):      # alternating
            eng.reset()
            t = timed(eng, fn)
            eng.wait()
            if i >= warmup:
                ms[name].append(t)
    for name in ms:
        r[name] = stat(ms[name])
    r["rules_over_replay"] = r["ms_rules"]["median"] / r["ms_replay_of_recorded_actions"]["median"]
    eng.reset()
    state = {f: eng.get_state(f) for f in STATE}
    out = R.swarm_rules(eng, rules, STEPS)
    r["mean_total_of_best_rule"] = float(out["totals"].mean(axis=0).max())
    r["best_rule"] = int(out["totals"].mean(axis=0).argmax())
    if E <= 64:
        host_in_the_loop(state, rules, off, E, n_rules=1)                   # warm-up: one rule
        rew, sec = host_in_the_loop(state, rules, off, E)
        r["host_in_the_loop"] = {"clock": "wall clock, ONE run", "ms": sec * 1e3, "launches": n * STEPS,
                                 "rewards_bits_equal_to_the_kernel": bool(rew.tobytes() == out["rewards"].tobytes())}
        r["host_in_the_loop_over_rules"] = sec * 1e3 / r["ms_rules"]["median"]
    eng.close()
    return r


def anchors_at_one_env(runs, warmup):
    """Where the rule's time goes on the latency chain of one env: 20 rules of one anchor each, next to the default set, whose last
    workgroup (rules 16..19) holds both anchors and so runs both loops on its agent wave."""
    lib = _ffi.load_library(extra_signatures=R.SWARMRULES_SIGNATURES)
    eng = _ffi.Engine(_ffi.ENV_SWARM, 1, seed=1692, flags=_ffi.F_SWARM_NO_OBSERVE | _ffi.F_RESEED_EACH_RESET, max_episode_steps=STEPS)
    sets = {"default rules (the last workgroup mixes the anchors)": DEFAULT_SWARM_RULES,
            "20 x rule 8 (centroid only)": np.tile(DEFAULT_SWARM_RULES[8], (20, 1)),
            "20 x rule 18 (nearest locust only)": np.tile(DEFAULT_SWARM_RULES[18], (20, 1))}
    r = {"case": "the rule's loops at one env", "envs": 1, "rules": 20, "steps": STEPS, "runs": runs, "warmup": warmup, "clock": "HIP events"}
    ms = {k: [] for k in sets}
    for i in range(warmup + runs):
        for k, rules in sets.items():                                       # alternating
            head, off = np.ascontiguousarray(rules[:, :3]), np.ascontiguousarray(R.swarm_rule_offsets(rules))
            eng.reset()
            t = timed(eng, lambda: eng._check(lib.grl_swarm_rules(eng.h, _ffi._ptr(head), _ffi._ptr(off), 20, STEPS, 0, -1)))
            eng.wait()
            if i >= warmup:
                ms[k].append(t)
    r["ms"] = {k: stat(v) for k, v in ms.items()}
    eng.close()
    return r


def recorded_rows():
    """env 0's action rows under the default rules from the reset state of seed 1692: (n_rules, STEPS, 10, 2) float64"""
    eng = _ffi.Engine(_ffi.ENV_SWARM, 1, seed=1692, flags=_ffi.F_SWARM_NO_OBSERVE | _ffi.F_RESEED_EACH_RESET, max_episode_steps=STEPS)
    eng.reset()
    out = R.swarm_rules(eng, DEFAULT_SWARM_RULES, STEPS, keep_actions=True)
    eng.close()
    return np.ascontiguousarray(out["actions"][0])


def eval_once_for_scale():
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
    t0 = time.perf_counter()
    name, best = mon.rule_baseline()
    sec_rules = time.perf_counter() - t0
    return {"case": "SwarmPolicyMonitor on Swarm-eval-v0", "clock": "wall clock, ONE run after a warm-up", "ms_eval_once": sec * 1e3,
            "episode_length": int(length), "untrained_policy_total_reward": float(total),
            "ms_rule_baseline_with_its_two_resets_and_reads": sec_rules * 1e3, "best_rule": name, "best_rule_total_reward": float(best)}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--envs", type=int, nargs="+", default=[1, 64, 4096])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "swarm_rules_times.json"))
    a = p.parse_args()
    out = {"times": [], "resources": RESOURCES}
    rows = recorded_rows()
    for E in a.envs:
        out["times"].append(case(E, a.runs, a.warmup, rows))
        print(json.dumps(out["times"][-1]), flush=True)
    out["times"].append(anchors_at_one_env(a.runs, a.warmup))
    print(json.dumps(out["times"][-1]), flush=True)
    out["times"].append(eval_once_for_scale())
    print(json.dumps(out["times"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
