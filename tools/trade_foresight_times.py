"""Foresight ceiling of the TradeAR1 env (include/goldsrl_tradeforesight.h): ms per call of 1 024 steps by HIP events on the handle's
stream -- the default horizons in one call at (64, 4 096, 8 192 envs x 2 assets) and (8 192 envs x 16 assets), each horizon in a call
of its own at 8 192 x 2, and the path kernel alone (GRL_TRADE_FORESIGHT_PATH_ONLY=1 stops the call after it) -- next to grl_trade_sweep
with ONE rule on the SAME handle in the same run: that kernel's code is the parent commit's, unchanged, which makes it the yardstick,
and one rule is one lane per env like one horizon.  For scale, at 2 assets, one 1 024-step greedy evaluation of the Gaussian agent
(grl_anet_eval).

    python tools/trade_foresight_times.py [--runs 5] [--warmup 1] [--json OUT]

Every call starts from a reset handle; median and spread (min, max) of the runs.  Default output:
profiles/trade_foresight_times.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_gauss, _ffi_tradeforesight, _ffi_tradesweep  # noqa: E402
from goldsrl.baselines import DEFAULT_TRADE_HORIZONS  # noqa: E402

STEPS = 1024
CASES = ((64, 2), (4096, 2), (8192, 2), (8192, 16))       # (envs, assets)
ALONE = (8192, 2)                                         # where each horizon is also timed alone


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def runs_of(eng, fn, runs, warmup):
    ms = []
    for i in range(warmup + runs):
        eng.reset()
        eng.timer_start()
        fn()
        eng.timer_stop()
        t = eng.timer_ms()
        if i >= warmup:
            ms.append(t)
    return stat(ms)


def measure(E, n, runs, warmup):
    sigs = dict(_ffi_tradesweep.TRADE_SWEEP_SIGNATURES, **_ffi_tradeforesight.TRADE_FORESIGHT_SIGNATURES)
    lib = _ffi.load_library(extra_signatures=sigs)
    eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=1692, n_assets=n, max_episode_steps=STEPS)
    hz = np.array(DEFAULT_TRADE_HORIZONS, np.int32)
    gain, bias = np.array([5.0], np.float32), np.zeros(1, np.float32)

    def call(h):
        return lambda: eng._check(lib.grl_trade_foresight(eng.h, _ffi._ptr(h), len(h), None, STEPS, -1))

    r = {"envs": E, "n_assets": n, "horizons": [int(h) for h in hz], "steps": STEPS, "runs": runs, "warmup": warmup}
    r["ms_all_horizons"] = runs_of(eng, call(hz), runs, warmup)
    os.environ["GRL_TRADE_FORESIGHT_PATH_ONLY"] = "1"
    r["ms_path_kernel"] = runs_of(eng, call(hz), runs, warmup)
    del os.environ["GRL_TRADE_FORESIGHT_PATH_ONLY"]
    r["ms_sweep_one_rule"] = runs_of(eng, lambda: eng._check(lib.grl_trade_sweep(eng.h, _ffi._ptr(gain), _ffi._ptr(bias), 1, None, STEPS, -1)),
                                     runs, warmup)
    base = r["ms_sweep_one_rule"]["median"]
    r["all_over_sweep_one_rule"] = r["ms_all_horizons"]["median"] / base
    r["path_over_sweep_one_rule"] = r["ms_path_kernel"]["median"] / base
    if (E, n) == ALONE:
        r["ms_per_horizon"] = {str(int(h)): runs_of(eng, call(np.array([h], np.int32)), runs, warmup) for h in hz}
        r["per_horizon_over_sweep_one_rule"] = {k: v["median"] / base for k, v in r["ms_per_horizon"].items()}
    eng.reset()
    st = _ffi_tradeforesight.trade_foresight(eng, hz, STEPS)
    r["mean_total_per_horizon"] = [float(v) for v in st["total"].mean(axis=1)]
    r["mean_trades_per_horizon"] = [float(v) for v in st["trades"].mean(axis=1)]
    r["worst_total_minus_bound"] = float(np.abs(st["total"][-1] - st["bound"][-1]).max())
    if n == 2:
        net = _ffi_gauss.GaussNet(eng, rnn_length=20, max_samples=1)
        net.set_params(_ffi_gauss.default_init_gauss(3, **_ffi_gauss.TRADE_SIZES))
        r["ms_policy_eval"] = runs_of(eng, lambda: net.lib.grl_anet_eval(net.n, STEPS, 0), runs, warmup)
        r["all_over_policy_eval"] = r["ms_all_horizons"]["median"] / r["ms_policy_eval"]["median"]
        net.close()
    eng.close()
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "trade_foresight_times.json"))
    a = p.parse_args()
    out = {"clock": "HIP events on the handle's stream", "times": [], "resources": None}
    kres = os.path.join(ROOT, "profiles", "trade_foresight_kres.txt")
    if os.path.exists(kres):
        out["resources"] = [ln.strip() for ln in open(kres) if ln.strip()]
    for E, n in CASES:
        out["times"].append(measure(E, n, a.runs, a.warmup))
        print(json.dumps(out["times"][-1]), flush=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
