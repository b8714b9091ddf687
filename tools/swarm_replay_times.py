"""Scripted Swarm episodes in one launch (include/goldsrl_replay.h) next to the per-step path, measured in the same run:

  (a) one episode, 1 pair x 128 steps on Swarm-eval-v0: SwarmReplay.play with the trace (one launch plus its five reads) against
      the same 128 float64 rows through the SwarmEnv facade (per step one launch, a reward and a done read, two state copies) --
      the path the eval monitor and a GIF script would otherwise take;
  (b) the batch, E envs x 1 sequence x 128 steps: grl_swarm_replay against 128 grl_step_device calls on the SAME handle with
      GRL_F_SWARM_NO_OBSERVE and GRL_F_RESEED_EACH_RESET set (every reset gives the same state) and no TimeLimit (so no reset
      kernel runs at the end of either), the same float32 action row at every step in both; the last step's rewards of the two
      are compared as bytes.

    python tools/swarm_replay_times.py [--envs 4096 32768] [--runs 5] [--warmup 1] [--json OUT]

Every run starts from a reset handle; ms by HIP events on the handle's stream (the stop event follows the last read or the wait, so
host gaps between launches count, as they do for a user); median and spread (min, max) of the runs.  The registers and scratch of
the three instantiations (tools/kres.sh swarm_replay.hip, kept in profiles/swarm_replay_kres.txt) are recorded next to the times.
Default output: profiles/swarm_replay_times.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_replay, envs  # noqa: E402
from goldsrl.replay import SwarmReplay  # noqa: E402

STEPS = 128


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def script(shape, dtype, seed=0):
    a = np.random.RandomState(seed).normal(size=shape + (10, 2)) * 0.8
    n = np.sqrt((a ** 2).sum(axis=-1, keepdims=True))
    return np.ascontiguousarray(np.where(n >= 1, a / np.maximum(n, 1e-30), a).astype(dtype))      # transform_actions_for_env


def one_episode(runs, warmup):
    env = envs.make("Swarm-eval-v0")
    eng, rows = env._eng, script((STEPS,), np.float64)
    r = {"case": "one episode", "pairs": 1, "steps": STEPS, "runs": runs, "warmup": warmup, "clock": "HIP events"}
    got = {}

    def replay():
        got["replay"] = SwarmReplay(env).play(rows, trace_env=0)

    def facade():
        got["facade"] = [env.step(a)[1] for a in rows]
    for name, fn in (("ms_replay", replay), ("ms_facade", facade)):
        ms = []
        for i in range(warmup + runs):
            env.reset()
            t = timed(eng, fn)
            if i >= warmup:
                ms.append(t)
        r[name] = stat(ms)
    r["rewards_bits_equal"] = bool(got["replay"]["rewards"][0, 0].tobytes() == np.array(got["facade"]).tobytes())
    r["replay_over_facade"] = r["ms_replay"]["median"] / r["ms_facade"]["median"]
    return r


def batch(E, runs, warmup):
    lib = _ffi.load_library(extra_signatures=_ffi_replay.REPLAY_SIGNATURES)
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=1692, flags=_ffi.F_SWARM_NO_OBSERVE | _ffi.F_RESEED_EACH_RESET,
                      max_episode_steps=0)      # every reset gives the same state, so the two paths play the same episodes
    row = script((1,), np.float32, seed=1)                                     # (1, 10, 2)
    rows = np.ascontiguousarray(np.broadcast_to(row, (1, STEPS, 10, 2)))      # the same row at every step
    buf = eng.dev_alloc(4 * E * 20)
    eng.dev_upload(buf, np.ascontiguousarray(np.broadcast_to(row, (E, 10, 2))))
    r = {"case": "batch", "envs": E, "sequences": 1, "steps": STEPS, "runs": runs, "warmup": warmup, "clock": "HIP events"}

    def replay():
        eng._check(lib.grl_swarm_replay(eng.h, _ffi._ptr(rows), 0, 1, STEPS, None, 0, -1))

    def per_step():
        for _ in range(STEPS):
            eng.step_device(buf)
    for name, fn in (("ms_replay", replay), ("ms_per_step_path", per_step)):
        ms = []
        for i in range(warmup + runs):
            eng.reset()
            t = timed(eng, fn)
            eng.wait()
            if i >= warmup:
                ms.append(t)
        r[name] = stat(ms)
    last = eng.read("reward_f64")                                              # of the per-step path's step 128
    rew = np.empty((E, 1, STEPS), np.float64)
    eng.reset()
    replay()
    eng._check(lib.grl_swarm_replay_read(eng.h, b"rewards", _ffi._ptr(rew), rew.nbytes))
    r["last_reward_bits_equal"] = bool(rew[:, 0, STEPS - 1].tobytes() == last.tobytes())
    r["replay_over_per_step_path"] = r["ms_replay"]["median"] / r["ms_per_step_path"]["median"]
    eng.dev_free(buf)
    eng.close()
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "swarm_replay_times.json"))
    a = p.parse_args()
    out = {"times": [], "resources": None}
    kres = os.path.join(ROOT, "profiles", "swarm_replay_kres.txt")
    if os.path.exists(kres):
        out["resources"] = [ln.strip() for ln in open(kres) if ln.strip()]
    out["times"].append(one_episode(a.runs, a.warmup))
    print(json.dumps(out["times"][-1]), flush=True)
    for E in a.envs:
        out["times"].append(batch(E, a.runs, a.warmup))
        print(json.dumps(out["times"][-1]), flush=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
