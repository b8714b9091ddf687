"""The conv policy's evaluation on the device (include/goldsrl_neteval.h) next to what stood in its place, measured in the same run.
ConvSingleAgentPolicyNetwork, 128 steps, the TimeLimit of Swarm-eval-v0:

  (a) ConvNet.eval with host normals and kept actions plus its reads, the E envs in ONE chunk per step;
  (b) the same with ONE ENV per chunk (an env's bits then do not depend on its chunk mates; what DeviceSwarmPolicyMonitor does for
      env 0 alone), up to --per-env-up-to envs;
  (c) grl_net_rollout(128) on the same handle without the gradient step, joined by grl_wait: the training rollout's pipeline, which
      also records what training needs and runs the bootstrap forward and the returns;
  (d) at one env, SwarmPolicyMonitor.eval_once on Swarm-eval-v0 (the host loop: per step a blocking predict, a draw, transform_actions,
      env.step and its reads) and DeviceSwarmPolicyMonitor.eval_once with 1, 16, 64 and 1 024 envs (env 0 on its own handle, the
      others in one chunk on a second one); ONE RUN each after a warm-up run, env 0's episodes compared as bytes.

    python tools/conv_eval_times.py [--envs 1 16 64 1024] [--runs 5] [--warmup 1] [--json OUT]

Everything is WALL CLOCK around the call and its first read (the path is launch-bound: the host's enqueue time is part of its cost);
(a) to (c): every run starts from a reset handle (GRL_F_RESEED_EACH_RESET: the same state every time), median and spread (min, max) of
the runs.  Default output: profiles/conv_eval_times.json."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_net  # noqa: E402

STEPS = 128


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def case(E, runs, warmup, per_env):
    r = {"case": "128 steps of E envs", "envs": E, "steps": STEPS, "runs": runs, "warmup": warmup, "clock": "wall clock, call + first read"}
    z = np.random.RandomState(7).normal(size=(E, STEPS, 10, 2))
    forms = [("one_chunk", E * 10)] + ([("one_env_per_chunk", 10)] if per_env else [])
    for form, chunk in forms:
        eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=1692, flags=_ffi.F_RESEED_EACH_RESET, max_episode_steps=STEPS)
        net = _ffi_net.ConvNet(eng, max_chunk_samples=min(chunk, 81920))
        net.set_params(_ffi_net.glorot_uniform_flat(seed=3))
        fns = [("ms_eval_" + form, lambda: net.eval(STEPS, normals=z, keep_actions=True))]
        if form == "one_chunk":
            fns.append(("ms_rollout_and_wait", lambda: (net.rollout(STEPS, 0), eng.wait())))
        ms = {name: [] for name, _ in fns}
        for i in range(warmup + runs):
            for name, fn in fns:      # alternating
                eng.reset()
                t = wall_ms(fn)
                if i >= warmup:
                    ms[name].append(t)
        for name in ms:
            r[name] = stat(ms[name])
        if form == "one_chunk":
            eng.reset()
            out = net.eval(STEPS, normals=z)
            r["episode_lengths"] = {"min": int(out["length"].min()), "max": int(out["length"].max())}
            r["mean_total_reward_untrained"] = float(out["total_reward"].mean())
            r["chunks_per_step"] = (E * 10 + min(chunk, 81920) - 1) // min(chunk, 81920)
        net.close(); eng.close()
    r["eval_over_rollout"] = r["ms_eval_one_chunk"]["median"] / r["ms_rollout_and_wait"]["median"]
    r["us_per_env_step_eval_one_chunk"] = r["ms_eval_one_chunk"]["median"] * 1e3 / (E * STEPS)
    return r


def monitors():
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import ConvSingleAgentPolicyNetwork
    from goldsrl.envs import make
    conf = dict(num_actions=2, entropy_regularisation_strength=0.02, device="/gpu:0", height=84, width=84, channels=3, scale=1000.0, clip_norm=40.0,
                clip_norm_type="global", name="local_learning")
    d = tempfile.mkdtemp()
    learner_eng = _ffi.Engine(_ffi.ENV_SWARM, 2, seed=5)
    learner_eng.reset()
    glob = ConvSingleAgentPolicyNetwork(conf).bind(learner_eng, seed=11)
    r = {"case": "eval_once on Swarm-eval-v0", "clock": "wall clock, ONE run after a warm-up run", "steps": STEPS}
    got = {}
    for name, build in (("host_loop_1_env", lambda w: PM.SwarmPolicyMonitor(make("Swarm-eval-v0"), glob, None, w, network_conf=conf)),
                        ("device_1_env", lambda w: PM.DeviceSwarmPolicyMonitor(global_policy_net=glob, summary_writer=w, n_envs=1)),
                        ("device_16_envs", lambda w: PM.DeviceSwarmPolicyMonitor(global_policy_net=glob, summary_writer=w, n_envs=16)),
                        ("device_64_envs", lambda w: PM.DeviceSwarmPolicyMonitor(global_policy_net=glob, summary_writer=w, n_envs=64)),
                        ("device_1024_envs", lambda w: PM.DeviceSwarmPolicyMonitor(global_policy_net=glob, summary_writer=w, n_envs=1024))):
        mon = build(PM.ScalarWriter(os.path.join(d, name), tfevents=False))
        mon.actions_path = os.path.join(d, name + ".json")
        mon.eval_once()                                                         # warm-up
        t0 = time.perf_counter()
        got[name] = mon.eval_once()
        r["ms_eval_once_" + name] = (time.perf_counter() - t0) * 1e3
        if name.startswith("device_") and mon.n_envs > 1:
            r["untrained_total_reward_mean_std_" + name[7:]] = [float(mon.total_rewards.mean()), float(mon.total_rewards.std())]
        if name.startswith("device_"):
            mon.close()
        else:
            mon.policy_net.net.close(); mon.env._eng.close()
    r["host_round_trips_of_the_loop"] = 5 * STEPS
    r["env0_episodes_bits_equal"] = bool(all(got[k] == got["host_loop_1_env"] for k in got))
    r["episode_length"], r["untrained_policy_total_reward"] = int(got["host_loop_1_env"][1]), float(got["host_loop_1_env"][0])
    r["host_loop_over_device_1_env"] = r["ms_eval_once_host_loop_1_env"] / r["ms_eval_once_device_1_env"]
    glob.net.close(); learner_eng.close()
    shutil.rmtree(d, ignore_errors=True)      # the monitors' scalar files and kept episodes
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--envs", type=int, nargs="+", default=[1, 16, 64, 1024])
    p.add_argument("--per-env-up-to", type=int, default=64, dest="per_env_up_to", help="largest env count measured with one env per chunk")
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "conv_eval_times.json"))
    a = p.parse_args()
    out = {"times": []}
    for E in a.envs:
        out["times"].append(case(E, a.runs, a.warmup, E <= a.per_env_up_to))
        print(json.dumps(out["times"][-1]), flush=True)
    out["times"].append(monitors())
    print(json.dumps(out["times"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
