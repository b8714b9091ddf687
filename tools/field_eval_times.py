"""The field policy's whole-episode evaluation (include/goldsrl_fieldeval.h) next to what stood in its place, measured in the same run.
Geometry G = 20, F = 5, L = 2 (train_paac_field's defaults), 128 steps, the TimeLimit of Swarm-eval-v0:

  (a) grl_fieldnet_eval, greedy, float64 rows, actions kept: one launch for the episodes of E envs;
  (b) grl_fieldnet_rollout(128) on the same handle without the gradient step: the per-step path (per step a fused forward launch, the
      env step, the reset launch, the bookkeeping and the reward layout), which also records what training needs;
  (c) at one env, FieldSwarmPolicyMonitor.eval_once on Swarm-eval-v0 both ways -- device_episode=True (the launch of (a) with its
      reset, its reads and the scalars) and device_episode=False (the host loop: per step predict_swarm, transform_actions and
      env.step).  WALL CLOCK, ONE RUN each after a warm-up run; the two episodes are compared as bytes;
  (d) at one env, SwarmPolicyMonitor.rule_baseline() on the same monitor (20 rules x 128 steps in one launch, with its two resets
      and its reads): the yardstick the evaluation is judged against.  Wall clock, one run after a warm-up.

    python tools/field_eval_times.py [--envs 1 64 4096] [--runs 5] [--warmup 1] [--json OUT]

(a) and (b): every run starts from a reset handle (GRL_F_RESEED_EACH_RESET: the same state every time); ms by HIP events on the
handle's stream around the call (memsets included, reads not); median and spread (min, max) of the runs, the two alternating.
The registers and scratch of the three instantiations are recorded next to the times.
Default output: profiles/field_eval_times.json."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_field  # noqa: E402

STEPS = 128
GEOM = dict(height=20, width=20, channels=2, filters=5, conv_layers=2, num_actions=2)
# hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -Rpass-analysis=kernel-resource-usage csrc/net_field.hip; LDS: 9 136 bytes of env,
# observation and actions + 13 380 of activations at this geometry, all dynamic
RESOURCES = {"field_eval_kernel<MATH_EXACT>": {"vgprs": 173, "scratch_bytes": 0, "lds_bytes": 22516, "waves_per_simd": 2},
             "field_eval_kernel<MATH_FAST>": {"vgprs": 175, "scratch_bytes": 0, "lds_bytes": 22516, "waves_per_simd": 2},
             "field_eval_kernel<MATH_REFDIV>": {"vgprs": 175, "scratch_bytes": 0, "lds_bytes": 22516, "waves_per_simd": 2}}


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def case(E, runs, warmup):
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=1692, flags=_ffi.F_RESEED_EACH_RESET, max_episode_steps=STEPS, grid_size=GEOM["height"])
    net = _ffi_field.FieldNet(eng, max_samples=min(E, 256), scale=10.0, entropy_beta=0.02, clip_norm=40.0, **GEOM)
    net.set_params(_ffi_field.glorot_uniform_flat(3, **GEOM))
    net.rollout_bind(0.99)
    r = {"case": "128 steps of E envs", "envs": E, "steps": STEPS, "runs": runs, "warmup": warmup, "clock": "HIP events"}

    def by_eval():
        net._check(net.lib.grl_fieldnet_eval(net.n, STEPS, 1, 0, 1, -1))

    def by_rollout():
        net.rollout(STEPS, 0)
    ms = {"ms_eval_one_launch": [], "ms_rollout_per_step": []}
    for i in range(warmup + runs):
        for name, fn in (("ms_eval_one_launch", by_eval), ("ms_rollout_per_step", by_rollout)):      # alternating
            eng.reset()
            t = timed(eng, fn)
            eng.wait()
            if i >= warmup:
                ms[name].append(t)
    for name in ms:
        r[name] = stat(ms[name])
    r["eval_over_rollout"] = r["ms_eval_one_launch"]["median"] / r["ms_rollout_per_step"]["median"]
    r["us_per_env_step_eval"] = r["ms_eval_one_launch"]["median"] * 1e3 / (E * STEPS)
    eng.reset()
    out = net.eval(STEPS)
    r["episode_lengths"] = {"min": int(out["length"].min()), "max": int(out["length"].max())}
    r["mean_total_reward_untrained"] = float(out["total_reward"].mean())
    net.close(); eng.close()
    return r


def monitors_at_one_env():
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import ConvPolicyVFieldNetwork
    conf = dict(GEOM, name='local_learning', clip_norm=40.0, clip_norm_type='global', device='/gpu:0', entropy_regularisation_strength=0.02, scale=10.0)
    d = tempfile.mkdtemp()
    learner_eng = _ffi.Engine(_ffi.ENV_SWARM, 2, seed=5, grid_size=GEOM["height"])
    learner_eng.reset()
    net = ConvPolicyVFieldNetwork(conf).bind(learner_eng, seed=11, gamma=0.99)
    r = {"case": "FieldSwarmPolicyMonitor on Swarm-eval-v0, one env", "clock": "wall clock, ONE run after a warm-up run", "steps": STEPS}
    got = {}
    for name, dev in (("device_episode", True), ("host_loop", False)):
        mon = PM.FieldSwarmPolicyMonitor(global_policy_net=net, summary_writer=PM.ScalarWriter(os.path.join(d, name), tfevents=False), device_episode=dev)
        mon.actions_path = os.path.join(d, name + ".json")
        mon.eval_once()                                                         # warm-up
        t0 = time.perf_counter()
        got[name] = mon.eval_once()
        r["ms_eval_once_" + name] = (time.perf_counter() - t0) * 1e3
        if dev:
            mon.rule_baseline()                                                 # warm-up
            t0 = time.perf_counter()
            best, total = mon.rule_baseline()
            r["ms_rule_baseline_with_its_two_resets_and_reads"] = (time.perf_counter() - t0) * 1e3
            r["best_rule"], r["best_rule_total_reward"] = best, float(total)
        mon.policy_net.net.close(); mon.env._eng.close()
    r["host_round_trips_of_the_loop"] = 3 * STEPS
    r["episodes_bits_equal"] = bool(got["device_episode"] == got["host_loop"])
    r["episode_length"], r["untrained_policy_total_reward"] = int(got["host_loop"][1]), float(got["host_loop"][0])
    r["host_loop_over_device_episode"] = r["ms_eval_once_host_loop"] / r["ms_eval_once_device_episode"]
    net.net.close(); learner_eng.close()
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--envs", type=int, nargs="+", default=[1, 64, 4096])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "field_eval_times.json"))
    a = p.parse_args()
    out = {"times": [], "geometry": GEOM, "resources": RESOURCES}
    for E in a.envs:
        out["times"].append(case(E, a.runs, a.warmup))
        print(json.dumps(out["times"][-1]), flush=True)
    out["times"].append(monitors_at_one_env())
    print(json.dumps(out["times"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
