"""Scripted rule baseline sweep of the Ticker env (include/goldsrl_tickersweep.h): ms per sweep of the twelve default rules x 1 023
steps by HIP events on the handle's stream, next to the same episodes through the per-step path on the SAME handle in the same run
(12 x 1 023 grl_step calls, each with the rule's actions computed on the host from the read-back TICKER_CASH / TICKER_QUANTITY /
TICKER_IDX / TICKER_START; wall clock, the host is part of that path; a rule that depletes an env goes on in that env's next
episode, so the step count is the same) and, for scale, one 1 023-step greedy evaluation of the gated trader (grl_gnet_eval).

    python tools/ticker_sweep_times.py [--envs 64 4096 8192] [--step-envs 64 4096] [--runs 5] [--warmup 1] [--json OUT]

The price table is a seeded random walk of 4 096 rows (that of tools/gated_eval_times.py's kind).  Every sweep starts from a reset
handle; median and spread (min, max) of the runs.  The expectation is structural only: the sweep is one launch of dependent float64
divide chains where the per-step path is 12 276 launches and several round trips to the host each, so it should take a small
fraction of it, and less than one policy evaluation.  Default output: profiles/ticker_sweep_times.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_gated, _ffi_tickersweep  # noqa: E402
from goldsrl.agents.a3c.policy_monitor import make_ticker_eval_engine  # noqa: E402
from goldsrl.baselines import DEFAULT_TICKER_RULES  # noqa: E402
from goldsrl.envs.data.sampler import build_matrix  # noqa: E402

STEPS = 1023


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def random_walk_table(rows=4096, seed=7):
    rng = np.random.RandomState(seed)
    days = rows // 2
    closes = 100.0 * np.exp(np.cumsum(rng.normal(2e-4, 0.008, size=days)))
    opens = closes * np.exp(rng.normal(0, 0.003, size=days))
    return build_matrix(opens, closes, rng.uniform(1e5, 5e5, size=days).round())


def measure(matrix, E, runs, warmup, per_step):
    lib = _ffi.load_library(extra_signatures=_ffi_tickersweep.TICKER_SWEEP_SIGNATURES)
    eng = make_ticker_eval_engine(matrix, E, max_episode_steps=STEPS)
    rules = np.ascontiguousarray(DEFAULT_TICKER_RULES)
    r = {"envs": E, "rules": len(rules), "steps": STEPS, "runs": runs, "warmup": warmup}
    ms = []
    for i in range(warmup + runs):
        eng.reset()
        t = timed(eng, lambda: eng._check(lib.grl_ticker_sweep(eng.h, _ffi._ptr(rules), len(rules), STEPS, -1)))
        if i >= warmup:
            ms.append(t)
    r["ms_sweep"] = stat(ms)
    st = _ffi_tickersweep.ticker_sweep(eng, rules, STEPS)
    r["mean_total_per_rule"] = [float(v) for v in st["total"].mean(axis=1)]
    r["mean_length_per_rule"] = [float(v) for v in st["length"].mean(axis=1)]
    r["ms_per_step_path"] = None
    if per_step:
        eng.reset()
        t0 = time.perf_counter()
        for rule in rules:          # the TimeLimit's auto-reset after 1 023 steps starts the next rule's episode
            for _ in range(STEPS):
                start, idx = eng.get_state("TICKER_START"), eng.get_state("TICKER_IDX")
                back = _ffi_tickersweep.ticker_rule_back(rule, matrix, start, idx)
                eng.step(_ffi_tickersweep.ticker_rule_actions(rule, eng.get_state("TICKER_CASH"), eng.get_state("TICKER_QUANTITY"),
                                                              matrix[start + idx][:, :2], back))
        r["ms_per_step_path"] = dict(stat([1e3 * (time.perf_counter() - t0)]), clock="wall", runs=1)
        r["sweep_over_per_step_path"] = r["ms_sweep"]["median"] / r["ms_per_step_path"]["median"]
    net = _ffi_gated.GatedNet(eng, rnn_length=5, max_samples=1)
    net.set_params(_ffi_gated.default_init_gated(3))
    ms = []
    for i in range(warmup + runs):
        eng.reset()
        t = timed(eng, lambda: net._check(net._fn("eval")(net.n, STEPS, 0)))
        if i >= warmup:
            ms.append(t)
    r["ms_policy_eval"] = stat(ms)
    r["sweep_over_policy_eval"] = r["ms_sweep"]["median"] / r["ms_policy_eval"]["median"]
    net.close()
    eng.close()
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", nargs="+", type=int, default=[64, 4096, 8192])
    p.add_argument("--step-envs", nargs="+", type=int, default=[64, 4096], help="the env counts at which the per-step path is timed too")
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "ticker_sweep_times.json"))
    a = p.parse_args()
    out = {"clock": "HIP events on the handle's stream (per-step path: wall clock)", "times": [], "resources": None}
    kres = os.path.join(ROOT, "profiles", "ticker_sweep_kres.txt")
    if os.path.exists(kres):
        out["resources"] = [ln.strip() for ln in open(kres) if ln.strip()]
    matrix = random_walk_table()
    for E in a.envs:
        out["times"].append(measure(matrix, E, a.runs, a.warmup, E in a.step_envs))
        print(json.dumps(out["times"][-1]), flush=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
