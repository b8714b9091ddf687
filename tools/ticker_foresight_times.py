"""Foresight ceiling of the Ticker env (include/goldsrl_tickerforesight.h): ms per call of the default horizons x 1 023 steps by HIP
events on the handle's stream -- all horizons in one launch, and each horizon in a launch of its own -- next to grl_ticker_sweep with
ONE rule (buy and hold) on the SAME handle in the same run: that kernel's code is the parent commit's, unchanged, which makes it the
yardstick, and one rule is one lane per env like one horizon.  For scale, one 1 023-step greedy evaluation of the gated trader
(grl_gnet_eval): the default call has to cost less than that.

    python tools/ticker_foresight_times.py [--envs 64 4096 8192] [--runs 5] [--warmup 1] [--json OUT]

The price table is the seeded random walk of 4 096 rows of tools/ticker_sweep_times.py.  Every call starts from a reset handle;
median and spread (min, max) of the runs.  Default output: profiles/ticker_foresight_times.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from goldsrl import _ffi, _ffi_gated, _ffi_tickerforesight, _ffi_tickersweep  # noqa: E402
from goldsrl.agents.a3c.policy_monitor import make_ticker_eval_engine  # noqa: E402
from goldsrl.baselines import DEFAULT_TICKER_HORIZONS, DEFAULT_TICKER_RULES  # noqa: E402
from ticker_sweep_times import random_walk_table, stat, timed  # noqa: E402

STEPS = 1023


def runs_of(eng, fn, runs, warmup):
    ms = []
    for i in range(warmup + runs):
        eng.reset()
        t = timed(eng, fn)
        if i >= warmup:
            ms.append(t)
    return stat(ms)


def measure(matrix, E, runs, warmup):
    sigs = dict(_ffi_tickersweep.TICKER_SWEEP_SIGNATURES, **_ffi_tickerforesight.TICKER_FORESIGHT_SIGNATURES)
    lib = _ffi.load_library(extra_signatures=sigs)
    eng = make_ticker_eval_engine(matrix, E, max_episode_steps=STEPS)
    hz = np.array(DEFAULT_TICKER_HORIZONS, np.int32)
    rule = np.ascontiguousarray(DEFAULT_TICKER_RULES[1:2])
    r = {"envs": E, "horizons": [int(h) for h in hz], "steps": STEPS, "runs": runs, "warmup": warmup}
    r["ms_all_horizons"] = runs_of(eng, lambda: eng._check(lib.grl_ticker_foresight(eng.h, _ffi._ptr(hz), len(hz), STEPS, -1)), runs, warmup)
    r["ms_per_horizon"] = {}
    for h in hz:
        one = np.array([h], np.int32)
        r["ms_per_horizon"][str(int(h))] = runs_of(eng, lambda: eng._check(lib.grl_ticker_foresight(eng.h, _ffi._ptr(one), 1, STEPS, -1)), runs, warmup)
    r["ms_sweep_one_rule"] = runs_of(eng, lambda: eng._check(lib.grl_ticker_sweep(eng.h, _ffi._ptr(rule), 1, STEPS, -1)), runs, warmup)
    base = r["ms_sweep_one_rule"]["median"]
    r["all_over_sweep_one_rule"] = r["ms_all_horizons"]["median"] / base
    r["per_horizon_over_sweep_one_rule"] = {k: v["median"] / base for k, v in r["ms_per_horizon"].items()}
    eng.reset()
    st = _ffi_tickerforesight.ticker_foresight(eng, hz, STEPS)
    r["mean_total_per_horizon"] = [float(v) for v in st["total"].mean(axis=1)]
    r["mean_trades_per_horizon"] = [float(v) for v in st["trades"].mean(axis=1)]
    net = _ffi_gated.GatedNet(eng, rnn_length=5, max_samples=1)
    net.set_params(_ffi_gated.default_init_gated(3))
    r["ms_policy_eval"] = runs_of(eng, lambda: net._check(net._fn("eval")(net.n, STEPS, 0)), runs, warmup)
    r["all_over_policy_eval"] = r["ms_all_horizons"]["median"] / r["ms_policy_eval"]["median"]
    net.close()
    eng.close()
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", nargs="+", type=int, default=[64, 4096, 8192])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "ticker_foresight_times.json"))
    a = p.parse_args()
    out = {"clock": "HIP events on the handle's stream", "times": [], "resources": None}
    kres = os.path.join(ROOT, "profiles", "ticker_foresight_kres.txt")
    if os.path.exists(kres):
        out["resources"] = [ln.strip() for ln in open(kres) if ln.strip()]
    matrix = random_walk_table()
    for E in a.envs:
        out["times"].append(measure(matrix, E, a.runs, a.warmup))
        print(json.dumps(out["times"][-1]), flush=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
