"""Scripted trading-rule baseline sweep of the TradeAR1 env (include/goldsrl_tradesweep.h): ms per sweep of the nine default rules
x 1 024 steps by HIP events on the handle's stream, for 1, 2 and 4 rules per lane (GRL_TRADE_SWEEP_RPL), next to the same episodes
through the per-step path on the SAME handle in the same run (9 x 1 024 grl_step calls, each with the rule's actions computed on
the host from the current prices; wall clock, the host is part of that path) and, for scale, one 1 024-step greedy evaluation of the
A3C Gaussian agent (grl_anet_eval; the agent exists for 2 assets only).

    python tools/trade_sweep_times.py [--cases 2:64 2:4096 2:8192 16:8192] [--runs 5] [--warmup 1] [--step-runs 1] [--json OUT]

Every sweep starts from a reset handle; median and spread (min, max) of the runs.  The expectation is structural only: the sweep is
one launch of dependent float64 pow / exp / log chains where the per-step path is 9 216 launches and as many round trips to the
host, so it should take a small fraction of it.  Default output: profiles/trade_sweep_times.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_gauss, _ffi_tradesweep  # noqa: E402
from goldsrl.baselines import DEFAULT_TRADE_RULES  # noqa: E402

STEPS = 1024


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def measure(n, E, runs, warmup, step_runs):
    lib = _ffi.load_library(extra_signatures=_ffi_tradesweep.TRADE_SWEEP_SIGNATURES)
    eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=1692, n_assets=n, max_episode_steps=STEPS)
    gains, biases = np.ascontiguousarray(DEFAULT_TRADE_RULES[:, 0]), np.ascontiguousarray(DEFAULT_TRADE_RULES[:, 1])
    r = {"n_assets": n, "envs": E, "rules": len(gains), "steps": STEPS, "runs": runs, "warmup": warmup, "ms_sweep": {}}
    for rpl in (1, 2, 4):
        os.environ["GRL_TRADE_SWEEP_RPL"] = str(rpl)
        ms = []
        for i in range(warmup + runs):
            eng.reset()
            t = timed(eng, lambda: eng._check(lib.grl_trade_sweep(eng.h, _ffi._ptr(gains), _ffi._ptr(biases), len(gains), None, STEPS, -1)))
            if i >= warmup:
                ms.append(t)
        r["ms_sweep"]["rpl%d" % rpl] = stat(ms)
    del os.environ["GRL_TRADE_SWEEP_RPL"]

    def per_step():
        for rule in DEFAULT_TRADE_RULES:    # the TimeLimit's auto-reset after 1 024 steps starts the next rule's episode
            for _ in range(STEPS):
                eng.step(_ffi_tradesweep.rule_actions(rule, eng.get_state("TRADE_PRICES")))
    ms = []
    for _ in range(step_runs):
        eng.reset()
        t0 = time.perf_counter()
        per_step()
        ms.append(1e3 * (time.perf_counter() - t0))
    r["ms_per_step_path"] = dict(stat(ms), clock="wall", runs=step_runs)
    r["ms_policy_eval"] = None
    if n == 2:
        net = _ffi_gauss.GaussNet(eng, rnn_length=20, max_samples=1)
        net.set_params(_ffi_gauss.default_init_gauss(3, **_ffi_gauss.TRADE_SIZES))
        ms = []
        for i in range(warmup + runs):
            eng.reset()
            t = timed(eng, lambda: net._check(net._fn("eval")(net.n, STEPS, 0)))
            if i >= warmup:
                ms.append(t)
        r["ms_policy_eval"] = stat(ms)
        net.close()
    eng.close()
    best = min(r["ms_sweep"], key=lambda k: r["ms_sweep"][k]["median"])
    r["fastest"] = best
    r["sweep_over_per_step_path"] = r["ms_sweep"][best]["median"] / r["ms_per_step_path"]["median"]
    if r["ms_policy_eval"]:
        r["sweep_over_policy_eval"] = r["ms_sweep"][best]["median"] / r["ms_policy_eval"]["median"]
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--cases", nargs="+", default=["2:64", "2:4096", "2:8192", "16:8192"], help="n_assets:envs")
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--step-runs", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "trade_sweep_times.json"))
    a = p.parse_args()
    out = {"clock": "HIP events on the handle's stream (per-step path: wall clock)", "times": [], "resources": None}
    kres = os.path.join(ROOT, "profiles", "trade_sweep_kres.txt")
    if os.path.exists(kres):
        out["resources"] = [ln.strip() for ln in open(kres) if ln.strip()]
    for case in a.cases:
        n, E = (int(v) for v in case.split(":"))
        out["times"].append(measure(n, E, a.runs, a.warmup, a.step_runs))
        print(json.dumps(out["times"][-1]), flush=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
