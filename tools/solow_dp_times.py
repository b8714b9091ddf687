"""Optimal-savings yardstick of the Solow env (include/goldsrl_solowdp.h): ms per solve and per play by HIP events on the handle's
stream.

    python tools/solow_dp_times.py [--envs 64 4096 8192] [--runs 5] [--warmup 1] [--json OUT]

The solve at the default grid (96 x 25 x 7, 96 actions, 256 stages: 256 launches) and at 32 x 9 x 3 with 32 actions and 128 stages;
the play of the default table at 64, 4 096 and 8 192 envs x 1 024 steps, every run from a reset handle; median and spread (min,
max) of the runs.  Beside them the largest deviation of stage 0's value from the float64 numpy restatement
(tests/_solow_dp_oracle.py) on the six cases of tests/test_gpu_solow_dp.py -- the measurement that test's bound is ten times of.
For orientation: the numpy restatement solved the default grid in 100 s on a CPU (one run; 197 s in an earlier form); the constant-savings sweep and one
policy evaluation on the same episodes are in profiles/solow_sweep_times.json.  No expectation is attached: nothing had been
measured before this tool ran.  Default output: profiles/solow_dp_times.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _solow_dp_cases as DC  # noqa: E402
import _solow_dp_oracle as DO  # noqa: E402
from goldsrl import _ffi, _ffi_solowdp  # noqa: E402
from goldsrl.agents.a3c.policy_monitor import make_eval_engine  # noqa: E402

STEPS = 1024
SOLVES = (("default", dict(nk=96, nz=25, nq=7, ns=96), 256), ("small", dict(nk=32, nz=9, nq=3, ns=32), 128))
ORACLE_CASES = ((5, 3, 1, 4, 1), (16, 7, 3, 16, 6), (33, 5, 5, 65, 3))


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def measure_solves(runs, warmup):
    lib = _ffi.load_library(extra_signatures=_ffi_solowdp.SOLOW_DP_SIGNATURES)
    eng = make_eval_engine("Solow-1-1-finite-eval-v0", 64, max_episode_steps=STEPS)
    out = []
    for name, sizes, horizon in SOLVES:
        g = _ffi_solowdp._grid_struct(_ffi_solowdp.solow_dp_grid(sigma=eng.cfg.solow_sigma, **sizes))
        ms = []
        for i in range(warmup + runs):
            t = timed(eng, lambda: eng._check(lib.grl_solow_dp_solve(eng.h, _ffi_solowdp.C.byref(g), horizon)))
            if i >= warmup:
                ms.append(t)
        pairs = sizes["nk"] * sizes["nz"] * sizes["nq"] * sizes["ns"]
        out.append({"grid": name, "sizes": sizes, "horizon": horizon, "state_action_pairs_per_stage": pairs, "runs": runs, "warmup": warmup,
                    "clock": "HIP events", "ms_solve": stat(ms), "us_per_stage": 1e3 * float(np.median(ms)) / horizon})
        print(json.dumps(out[-1]), flush=True)
    eng.close()
    return out


def measure_play(E, runs, warmup):
    lib = _ffi.load_library(extra_signatures=_ffi_solowdp.SOLOW_DP_SIGNATURES)
    eng = make_eval_engine("Solow-1-1-finite-eval-v0", E, max_episode_steps=STEPS)
    _ffi_solowdp.solow_dp_solve(eng, None, _ffi_solowdp.DEFAULT_HORIZON, read=False)
    ms = []
    for i in range(warmup + runs):
        eng.reset()
        t = timed(eng, lambda: eng._check(lib.grl_solow_dp_play(eng.h, STEPS, 0)))
        if i >= warmup:
            ms.append(t)
    total = _ffi_solowdp.solow_dp_play(eng, STEPS)["total"]
    eng.close()
    return {"envs": E, "steps": STEPS, "grid": "default", "runs": runs, "warmup": warmup, "clock": "HIP events", "ms_play": stat(ms),
            "mean_total_reward": float(total.mean())}


def value_deviation():
    """largest |value - oracle| / max(1, |oracle|) of stage 0 on the cases of tests/test_gpu_solow_dp.py"""
    rows = []
    for nk, nz, nq, ns, horizon in ORACLE_CASES:
        for q in (1, 0):
            grid = _ffi_solowdp.solow_dp_grid(nk=nk, nz=nz, nq=nq, ns=ns, sigma=DC.SIGMA)
            policy, value, gap = DO.solve(grid, horizon, DC.RHO, DC.THETA if q else 0.0, DC.DELTA, nq if q else 1)
            eng = _ffi.Engine(_ffi.ENV_SOLOW, 1, solow_p=1, solow_q=q)
            got = _ffi_solowdp.solow_dp_solve(eng, grid, horizon)
            eng.close()
            rows.append({"case": [nk, nz, nq, ns, horizon], "q": q, "oracle_min_gap": gap,
                         "value_deviation": float((np.abs(got["value"] - value) / np.maximum(1.0, np.abs(value))).max()),
                         "policy_equal": bool(got["policy"].tobytes() == policy.tobytes())})
    return {"cases": rows, "largest": max(r["value_deviation"] for r in rows)}


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, nargs="+", default=[64, 4096, 8192])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "solow_dp_times.json"))
    a = p.parse_args()
    out = {"numpy_solve_default_grid_s": {"tests/_solow_dp_oracle.py": 100.0, "an earlier form": 197.0}, "value_vs_oracle": value_deviation()}
    print(json.dumps(out["value_vs_oracle"]), flush=True)
    out["solve"] = measure_solves(a.runs, a.warmup)
    out["play"] = []
    for E in a.envs:
        out["play"].append(measure_play(E, a.runs, a.warmup))
        print(json.dumps(out["play"][-1]), flush=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
