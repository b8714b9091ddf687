"""The flat PAAC policy under the true history window (include/goldsrl_flatwindow.h) on the clock: ms per rollout(20), ms per update
(grl_fnet_train_rollout on that rollout) and ms per 1 024-step evaluation, for Solow at 4 096 envs (R = 5) and TradeAR1-16 at
8 192 envs (R = 20), in three variants:
  parent   the baseline checkout (--baseline, a built checkout of the parent commit), the worker's window (quirk Q11)
  quirk    this checkout with the switch off
  true     this checkout with grl_fnet_set_true_window(1)
Every repetition runs the variants one after the other, each in a fresh process (parent, quirk, true, parent, ...), so the three
see the same machine at the same time; per variant and number the median and the spread (min, max) over the repetitions.  Inside a
process: HIP events on the handle's stream around 20 rollouts (after two warm-up rollouts, an update and an evaluation), around
each of 5 updates (a fresh rollout before each, not timed), around each of 3 evaluations (from a reset handle; the bracket includes
the reset grl_fnet_eval ends with).

    python tools/flat_true_window_times.py --baseline PARENT_CHECKOUT [--reps 5] [--json profiles/flat_true_window_times.json]

Gate: quirk / parent stays within the parent's own spread (within_spread: |quirk - parent| medians <= parent max - min).  The true
mode has no parent; its ratio to quirk is recorded."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS, T = 1024, 20
CASES = (("solow", 4096, 5), ("trade", 8192, 20))
N_ASSETS = 16
METRICS = ("ms_rollout20", "ms_update", "ms_eval1024")


def worker(root, mode):
    sys.path.insert(0, os.path.join(os.path.abspath(root), "golds-rl-gym_amd"))
    from goldsrl import _ffi, _ffi_flat
    out = {}
    for kind, E, R in CASES:
        if kind == "solow":
            eng = _ffi.Engine(_ffi.ENV_SOLOW, E, seed=3, rnn_length=R, max_episode_steps=STEPS)
            sizes = dict(static_size=2, temporal_size=2, num_actions=1)
        else:
            eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=3, n_assets=N_ASSETS, rnn_length=R, max_episode_steps=STEPS)
            sizes = dict(static_size=1 + 2 * N_ASSETS, temporal_size=1 + 2 * N_ASSETS, num_actions=N_ASSETS)
        eng.reset()
        net = _ffi_flat.FlatNet(eng, rnn_length=R, scale=100.0, max_samples=T * E, **sizes)
        net.set_params(_ffi_flat.default_init_flat(3, **sizes))
        if mode == "true":
            net.set_true_window(True)

        def timed(fn):
            eng.timer_start(); fn(); eng.timer_stop()
            return eng.timer_ms()
        for _ in range(2):
            net.rollout(T)
        net.train_rollout(1e-4)
        net.lib.grl_fnet_eval(net.n, STEPS, 0, 0); eng.wait()
        r = {"ms_rollout20": timed(lambda: [net.rollout(T) for _ in range(20)]) / 20.0}
        ups = []
        for _ in range(5):
            net.rollout(T); eng.wait()
            ups.append(timed(lambda: net.train_rollout(1e-4)))
        r["ms_update"] = float(np.median(ups))
        evs = []
        for _ in range(3):
            eng.reset()
            evs.append(timed(lambda: net.lib.grl_fnet_eval(net.n, STEPS, 0, 0)))
        r["ms_eval1024"] = float(np.median(evs))
        out["%s_%d" % (kind, E)] = r
        net.close(); eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "values": [float(x) for x in v]}


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--baseline", help="a built checkout of the parent commit")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--json")
    p.add_argument("--root", default=os.path.dirname(HERE))
    p.add_argument("--worker", choices=["quirk", "true"])
    a = p.parse_args()
    if a.worker:
        return worker(a.root, a.worker)
    variants = ([("parent", a.baseline, "quirk")] if a.baseline else []) + [("quirk", a.root, "quirk"), ("true", a.root, "true")]
    runs = {v[0]: [] for v in variants}
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    for rep in range(a.reps):
        for name, root, mode in variants:      # interleaved: one process per variant and repetition
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--worker", mode], check=True, env=env,
                                 stdout=subprocess.PIPE, universal_newlines=True)
            line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")][-1]
            runs[name].append(json.loads(line[7:]))
            print(rep, name, line[7:], flush=True)
    out = {"steps_per_rollout": T, "eval_steps": STEPS, "reps": a.reps, "clock": "HIP events", "order": [v[0] for v in variants], "cases": {}}
    for kind, E, R in CASES:
        key = "%s_%d" % (kind, E)
        c = {"env": kind, "envs": E, "rnn_length": R}
        for name in runs:
            c[name] = {m: stat([r[key][m] for r in runs[name]]) for m in METRICS}
        for m in METRICS:
            c["true_over_quirk_" + m] = c["true"][m]["median"] / c["quirk"][m]["median"]
            if "parent" in c:
                b = c["parent"][m]
                c["quirk_over_parent_" + m] = c["quirk"][m]["median"] / b["median"]
                c["quirk_within_parent_spread_" + m] = bool(abs(c["quirk"][m]["median"] - b["median"]) <= b["max"] - b["min"])
        out["cases"][key] = c
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
