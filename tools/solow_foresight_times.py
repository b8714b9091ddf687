"""Perfect-foresight ceiling of the Solow env (include/goldsrl_solowforesight.h): ms per call by HIP events on the handle's stream,
and the figures it adds to Solow's scale.

    python tools/solow_foresight_times.py [--envs 64 4096 8192] [--runs 5] [--warmup 1] [--json OUT]

For (1,1), (3,3) and (3,2) at the default grid (96 k nodes x 96 rates): grl_solow_foresight at 64, 4 096 and 8 192 envs x 1 024
steps, every run from a reset handle; median and spread (min, max) of the runs.  In the same run, the parent's code unchanged: the
constant-savings sweep of the reference's 20 rates, one greedy evaluation of the Gaussian A3C policy, and, where the order has an
induction, its solve and play.  Then floor, induction and ceiling on the 64 seeded envs of each order's eval registration, (2,2)
included, with the number of played steps outside the default k range and the range of k the plays visited.  No expectation is
attached: nothing of this shape had been measured before this tool ran.  Default output: profiles/solow_foresight_times.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_gauss, _ffi_solowforesight as F, _ffi_sweep  # noqa: E402
from goldsrl.agents.a3c.policy_monitor import make_eval_engine  # noqa: E402
from goldsrl.baselines import REFERENCE_RATES, ConstantSavingsBaseline, OptimalSavingsBaseline, SolowForesightCeiling  # noqa: E402

STEPS = 1024
ORDERS = ((1, 1), (3, 3), (3, 2))
SCALE_ORDERS = ((1, 1), (2, 2), (3, 3), (3, 2))


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(eng, fn, runs, warmup, before=None):
    ms = []
    for i in range(warmup + runs):
        if before:
            before()
        eng.timer_start()
        fn()
        eng.timer_stop()
        if i >= warmup:
            ms.append(eng.timer_ms())
    return stat(ms)


def env_name(p, q):
    return "Solow-%d-%d-finite-eval-v0" % (p, q)


def has_induction(p, q):
    return max(p, max(q, 1) + 1) <= 4


def measure_order(p, q, envs, runs, warmup):
    lib = _ffi.load_library(extra_signatures=F.SOLOW_FORESIGHT_SIGNATURES)
    out = {"order": [p, q], "runs": runs, "warmup": warmup, "clock": "HIP events", "calls": []}
    for E in envs:
        eng = make_eval_engine(env_name(p, q), E, max_episode_steps=STEPS)
        grid = F.solow_foresight_grid(eng)
        out["grid"] = grid
        g = F._grid_struct(grid)
        row = {"envs": E, "steps": STEPS}
        row["ms_foresight"] = timed(eng, lambda: eng._check(lib.grl_solow_foresight(eng.h, F.C.byref(g), STEPS, 0)), runs, warmup, before=eng.reset)
        row["ms_constant_sweep_20_rates_with_read_back"] = timed(eng, lambda: _ffi_sweep.solow_sweep(eng, REFERENCE_RATES, STEPS), runs, warmup, before=eng.reset)
        if has_induction(p, q):
            b = OptimalSavingsBaseline(engine=eng, max_episode_steps=STEPS)
            row["ms_induction_solve"] = timed(eng, lambda: b._solve(eng, b.grid, b.horizon, read=False), runs, warmup)
            row["ms_induction_play_with_read_back"] = timed(eng, lambda: b._play(eng, STEPS, 0), runs, warmup, before=eng.reset)
        net = _ffi_gauss.GaussNet(eng, rnn_length=20, max_samples=1)
        net.set_params(_ffi_gauss.default_init_gauss(3, **_ffi_gauss.SOLOW_SIZES))
        row["ms_policy_eval"] = timed(eng, lambda: net.lib.grl_anet_eval(net.n, STEPS, 0), runs, warmup, before=eng.reset)
        row["foresight_over_policy_eval"] = row["ms_foresight"]["median"] / row["ms_policy_eval"]["median"]
        net.close()
        out["calls"].append(row)
        eng.close()
        print(json.dumps(row), flush=True)
    return out


def measure_scale(p, q):
    eng = make_eval_engine(env_name(p, q), 64, max_episode_steps=STEPS)
    rate, floor = ConstantSavingsBaseline(engine=eng, max_episode_steps=STEPS).best_total()
    top = SolowForesightCeiling(engine=eng, max_episode_steps=STEPS)
    s = top.run(trace_steps=STEPS)
    live = np.arange(STEPS)[:, None] < s["length"][None]
    row = {"order": [p, q], "envs": 64, "floor_rate": float(rate), "floor": float(floor), "ceiling": top.ceiling(), "grid_value": top.value(),
           "ceiling_standard_error": float(s["total"].std(ddof=1) / 8.0), "clamped_steps": int(s["clamped"].sum()),
           "k_range_default": [top.grid["k_lo"], top.grid["k_hi"]],
           "k_visited": [float(np.where(live, s["k"], np.inf).min()), float(np.where(live, s["k"], -np.inf).max())]}
    if has_induction(p, q):
        total = OptimalSavingsBaseline(engine=eng, max_episode_steps=STEPS).run()["total"]
        row["induction"] = float(total.mean())
        row["envs_where_ceiling_is_below_induction"] = int((s["total"] < total).sum())
    eng.close()
    print(json.dumps(row), flush=True)
    return row


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, nargs="+", default=[64, 4096, 8192])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "solow_foresight_times.json"))
    a = p.parse_args()
    out = {"scale": [measure_scale(p, q) for p, q in SCALE_ORDERS], "orders": [measure_order(p, q, a.envs, a.runs, a.warmup) for p, q in ORDERS]}
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
