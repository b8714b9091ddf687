"""ARMA-state optimal-savings yardstick of the Solow env (include/goldsrl_solowarmadp.h): ms per solve and per play by HIP events
on the handle's stream, and the scale it gives the three orders the reference's constant_solow prints.

    python tools/solow_arma_dp_times.py [--envs 64 4096 8192] [--runs 5] [--warmup 1] [--no-oracle] [--json OUT]

For Solow-2-2 and Solow-3-3 at the default grid (48 x 9 per axis x 3, 48 rates, 128 stages): the solve, and the play at 64, 4 096
and 8 192 envs x 1 024 steps, every run from a reset handle; median and spread (min, max) of the runs.  In the same run, for
orientation: grl_solow_dp_solve at (1,1) on a (k, z, e) grid of a comparable state count, the constant-savings sweep of the
reference's 20 rates on the same envs, and the wall time of the numpy restatement (tests/_solow_arma_dp_oracle.py) for the same
solve, one run.  Then floor, ceiling and gap of (1,1), (2,2) and (3,3), each on the reference's seeded eval episode (numpy's
RandomState(1692) draws, injected) and on the 64 seeded envs of the eval registration with the standard error of the mean.  No
expectation is attached: nothing had been measured before this tool ran.  Default output: profiles/solow_arma_dp_times.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _solow_arma_dp_oracle as AO  # noqa: E402
from goldsrl import _ffi, _ffi_solowarmadp, _ffi_solowdp, _ffi_sweep  # noqa: E402
from goldsrl.agents.a3c.policy_monitor import make_eval_engine  # noqa: E402
from goldsrl.baselines import REFERENCE_RATES, ConstantSavingsBaseline, OptimalSavingsBaseline  # noqa: E402

STEPS = 1024
ORDERS = ((1, 1), (2, 2), (3, 3))
# the (k, z, e) solver at a state count next to 48 x 9^3 = 34 992 (48 x 243 x 3) and to 48 x 9^4 = 314 928 (48 x 937 x 7)
KZE_GRIDS = (dict(nk=48, nz=243, nq=3, ns=48), dict(nk=48, nz=937, nq=7, ns=48))


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


def measure_order(p, q, envs, runs, warmup, oracle):
    lib = _ffi.load_library(extra_signatures=_ffi_solowarmadp.SOLOW_ARMA_DP_SIGNATURES)
    horizon = _ffi_solowarmadp.DEFAULT_HORIZON
    out = {"order": [p, q], "horizon": horizon, "runs": runs, "warmup": warmup, "clock": "HIP events", "play": []}
    for E in envs:
        eng = make_eval_engine(env_name(p, q), E, max_episode_steps=STEPS)
        grid = _ffi_solowarmadp.engine_grid(eng)
        g = _ffi_solowarmadp._grid_struct(grid)
        if "ms_solve" not in out:
            out["grid"] = {"nk": grid["nk"], "nx": grid["nx"], "nq": grid["nq"], "ns": grid["ns"], "x_max": grid["x_max"]}
            out["states"] = int(np.prod(grid["nx"])) * grid["nk"]
            out["ms_solve"] = timed(eng, lambda: eng._check(lib.grl_solow_arma_dp_solve(eng.h, _ffi_solowarmadp.C.byref(g), horizon)), runs, warmup)
            out["us_per_stage"] = 1e3 * out["ms_solve"]["median"] / horizon
        else:
            eng._check(lib.grl_solow_arma_dp_solve(eng.h, _ffi_solowarmadp.C.byref(g), horizon))
        play = timed(eng, lambda: eng._check(lib.grl_solow_arma_dp_play(eng.h, STEPS, 0)), runs, warmup, before=eng.reset)
        sweep = timed(eng, lambda: _ffi_sweep.solow_sweep(eng, REFERENCE_RATES, STEPS), runs, warmup, before=eng.reset)
        out["play"].append({"envs": E, "steps": STEPS, "ms_play": play, "ms_constant_sweep_20_rates_with_read_back": sweep,
                            "mean_total_reward": float(_ffi_solowarmadp.solow_arma_dp_play(eng, STEPS)["total"].mean())})
        eng.close()
    if oracle:
        t = time.time()
        AO.solve(grid, horizon, grid["model"]["A"], grid["model"]["b"], 0.02)
        out["numpy_oracle_solve_s"] = time.time() - t
    print(json.dumps(out), flush=True)
    return out


def measure_kze(runs, warmup):
    lib = _ffi.load_library(extra_signatures=_ffi_solowdp.SOLOW_DP_SIGNATURES)
    eng = make_eval_engine(env_name(1, 1), 64, max_episode_steps=STEPS)
    out = []
    for sizes in KZE_GRIDS:
        g = _ffi_solowdp._grid_struct(_ffi_solowdp.solow_dp_grid(sigma=eng.cfg.solow_sigma, **sizes))
        horizon = _ffi_solowarmadp.DEFAULT_HORIZON
        ms = timed(eng, lambda: eng._check(lib.grl_solow_dp_solve(eng.h, _ffi_solowdp.C.byref(g), horizon)), runs, warmup)
        out.append({"solver": "grl_solow_dp_solve", "order": [1, 1], "sizes": sizes, "states": sizes["nk"] * sizes["nz"] * sizes["nq"],
                    "horizon": horizon, "ms_solve": ms})
        print(json.dumps(out[-1]), flush=True)
    eng.close()
    return out


def reference_episode_engine(p, q):
    """One env on the reference's seeded eval episode: SolowEnv._reset's draws under seed 1692, injected."""
    rs = np.random.RandomState(1692)
    z0, es = rs.normal(scale=0.1, size=(p,)), rs.normal(0, 0.1, (2048,))
    eng = _ffi.Engine(_ffi.ENV_SOLOW, 1, solow_p=p, solow_q=q, solow_tape_len=2048, max_episode_steps=STEPS, flags=_ffi.F_RESET_FROM_SNAPSHOT)
    eng.set_state("SOLOW_Z0", z0[None].astype(np.float32))
    eng.set_state("SOLOW_TAPE", es[None].astype(np.float32))
    eng.reset()
    return eng


def scale(eng, arma, grid=None, horizon=None):
    """floor, ceiling, gap on the engine's envs.  arma: take the ARMA-state solver at (1,1) too, where the class would not."""
    rate, floor = ConstantSavingsBaseline(engine=eng, max_episode_steps=STEPS).best_total()
    if arma:
        _ffi_solowarmadp.solow_arma_dp_solve(eng, grid, horizon or _ffi_solowarmadp.DEFAULT_HORIZON, read=False)
        eng.reset()
        total = _ffi_solowarmadp.solow_arma_dp_play(eng, STEPS)["total"]
    else:
        total = OptimalSavingsBaseline(engine=eng, max_episode_steps=STEPS).run()["total"]
    row = {"floor_rate": float(rate), "floor": float(floor), "ceiling": float(total.mean()), "gap": float(total.mean() - floor)}
    if len(total) > 1:
        row["ceiling_standard_error"] = float(total.std(ddof=1) / np.sqrt(len(total)))
    return row


def measure_scale():
    out = []
    for p, q in ORDERS:
        for solver in (("kze", "arma") if (p, q) == (1, 1) else ("arma",)):
            row = {"order": [p, q], "solver": {"kze": "grl_solow_dp_solve, default grid", "arma": "grl_solow_arma_dp_solve, default grid"}[solver]}
            eng = reference_episode_engine(p, q)
            row["reference_episode"] = scale(eng, solver == "arma")
            eng.close()
            eng = make_eval_engine(env_name(p, q), 64, max_episode_steps=STEPS)
            row["64_seeded_envs"] = scale(eng, solver == "arma")
            eng.close()
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, nargs="+", default=[64, 4096, 8192])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--no-oracle", action="store_true", help="skip the numpy restatement's solves (minutes at (3,3))")
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "solow_arma_dp_times.json"))
    a = p.parse_args()
    out = {"scale": measure_scale(), "kze_solver_at_comparable_state_counts": measure_kze(a.runs, a.warmup),
           "orders": [measure_order(p, q, a.envs, a.runs, a.warmup, not a.no_oracle) for p, q in ORDERS[1:]]}
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
