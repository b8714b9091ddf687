"""A3C discrete savings-grid agent on the device (include/goldsrl_discretenet.h), next to the Gaussian agent on the SAME Solow handle
in the same run: ms per rollout(64) and per update at E envs with K = 51 by HIP events on the handle's stream, and ms per 1 024-step
greedy evaluation of E envs in one launch against the per-step greedy rollout.

    python tools/discrete_update_times.py [--envs 4096 8192] [--steps 64] [--eval-envs 8192] [--runs 7] [--warmup 2] [--json OUT]

Each timed run is, for the Gaussian net and then the discrete net, one rollout(T) between two events and one train_rollout between
two events; median and spread (min, max) of the runs.  The expectation is structural only: one policy tower where the Gaussian net
runs two, so neither figure should exceed the Gaussian's beyond the Gaussian's own run-to-run spread (`within_gauss_spread`); the
evaluation should come in below the per-step rollout.  Default output: profiles/discrete_update_times.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_discrete, _ffi_gauss  # noqa: E402

K, R, EVAL_STEPS = 51, 5, 1024


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def nets(eng, max_samples, seed=3):
    g = _ffi_gauss.GaussNet(eng, rnn_length=R, scale=100.0, max_samples=max_samples)
    g.set_params(_ffi_gauss.default_init_gauss(seed, **_ffi_gauss.SOLOW_SIZES))
    d = _ffi_discrete.DiscreteNet(eng, rnn_length=R, num_choices=K, max_samples=max_samples)
    d.set_params(_ffi_discrete.default_init_discrete(seed, K))
    return {"gauss": g, "discrete": d}


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def measure_update(E, T, runs, warmup):
    eng = _ffi.Engine(_ffi.ENV_SOLOW, E, seed=3)
    eng.reset()
    ns = nets(eng, 1)
    ms = {k: {"rollout": [], "update": []} for k in ns}
    for i in range(warmup + runs):
        for k, n in ns.items():
            t_ro = timed(eng, lambda: n.rollout(T))
            t_up = timed(eng, lambda: n.train_rollout(1e-4))
            if i >= warmup:
                ms[k]["rollout"].append(t_ro); ms[k]["update"].append(t_up)
    for n in ns.values():
        n.close()
    eng.close()
    r = {"envs": E, "steps": T, "rnn_length": R, "num_choices": K, "runs": runs, "warmup": warmup, "clock": "HIP events"}
    for k in ms:
        r[k] = {"ms_per_rollout": stat(ms[k]["rollout"]), "ms_per_update": stat(ms[k]["update"])}
        r[k]["env_steps_per_s"] = E * T / ((r[k]["ms_per_rollout"]["median"] + r[k]["ms_per_update"]["median"]) * 1e-3)
    r["within_gauss_spread"] = {
        q: r["discrete"][q]["median"] <= r["gauss"][q]["median"] + (r["gauss"][q]["max"] - r["gauss"][q]["min"]) for q in ("ms_per_rollout", "ms_per_update")}
    return r


def measure_eval(E, runs, warmup):
    eng = _ffi.Engine(_ffi.ENV_SOLOW, E, seed=3, max_episode_steps=EVAL_STEPS)
    ns = nets(eng, 1)
    r = {"envs": E, "steps": EVAL_STEPS, "rnn_length": R, "num_choices": K, "runs": runs, "warmup": warmup, "clock": "HIP events"}
    for k, n in ns.items():
        ev, ro = [], []
        n.set_greedy(True)
        for i in range(warmup + runs):
            eng.reset()
            t_ev = timed(eng, lambda: n._check(n._fn("eval")(n.n, EVAL_STEPS, 0)))
            eng.reset()
            t_ro = timed(eng, lambda: n.rollout(EVAL_STEPS))
            if i >= warmup:
                ev.append(t_ev); ro.append(t_ro)
        r[k] = {"ms_eval": stat(ev), "ms_greedy_rollout": stat(ro)}
        r[k]["eval_over_greedy_rollout"] = r[k]["ms_eval"]["median"] / r[k]["ms_greedy_rollout"]["median"]
        n.close()
    eng.close()
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, nargs="+", default=[4096, 8192])
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--eval-envs", type=int, default=8192)
    p.add_argument("--runs", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "discrete_update_times.json"))
    a = p.parse_args()
    out = {"update": [], "eval": None}
    for E in a.envs:
        out["update"].append(measure_update(E, a.steps, a.runs, a.warmup))
        print(json.dumps(out["update"][-1]), flush=True)
    if a.eval_envs > 0:
        out["eval"] = measure_eval(a.eval_envs, max(1, a.runs // 2), 1)
        print(json.dumps(out["eval"]), flush=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
