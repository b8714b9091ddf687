"""The cross-entropy search over a Ticker rule's six numbers in one call (include/goldsrl_tickersearch.h) next to what it replaces,
measured in the same run, on the fixture table (tests/golden/ticker_rules.npz) and the seeded windows of the eval registration.  The
search starts from (1, 0, 0, 1, 0.5, 8) with the default spreads, G = 8, 8 elites, 1 023 steps, (E, C) in (1, 32), (64, 64),
(4 096, 64), (8 192, 64):

  (a) grl_ticker_search, one call: G evaluations and G updates on the handle's stream, nothing read back between them; ms by HIP
      events on the stream around the call (the uploads included, reads not), median and spread (min, max) of the runs after the
      warm-up, every run from a reset handle (GRL_F_RESEED_EACH_RESET: the same state every time);
  (b) the same call with max_steps = 1: the uploads, 2 G launches and the update kernel's E loads per candidate, next to no evaluation
      -- what the update kernel and the call's fixed part cost at that size;
  (c) eight grl_ticker_sweep calls of C rules (the last generation's table) over 1 023 steps on the same handle, HIP events around
      the eight: what the evaluations alone cost in the sweep's form;
  (d) ticker_search_host on the same handle: per generation one grl_ticker_sweep, the read of its statistics, E vector adds, a sort
      and the refit in numpy.  WALL CLOCK, ONE RUN; its six outputs are compared with (a)'s as bytes;
  (e) the scale on the fixture table, 64 windows x 1 023 steps: the best default rule, the tuned rule where it was tuned, both on 64
      other windows of the same table (another seed; the table has 1 400 rows, so the two sets overlap), and the foresight ceiling.

    python tools/ticker_search_times.py [--runs 5] [--warmup 1] [--json OUT]

Default output: profiles/ticker_search_times.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_tickersearch as S, _ffi_tickersweep as W  # noqa: E402
from goldsrl.baselines import DEFAULT_TICKER_RULES, TickerForesightCeiling, TickerRuleBaseline, TickerRuleSearch  # noqa: E402

STEPS = 1023
G, ELITES = 8, 8
CASES = ((1, 32), (64, 64), (4096, 64), (8192, 64))
START = (1, 0, 0, 1, 0.5, 8)
# tools/kres.sh ticker_search.hip / ticker_sweep.hip (hipcc -O3 --offload-arch=gfx950 -ffp-contract=off)
RESOURCES = {"ticker_search_eval_kernel": {"vgprs": 72, "scratch_bytes": 0, "lds_bytes": 0, "waves_per_simd": 7},
             "ticker_search_update_kernel": {"vgprs": 50, "scratch_bytes": 0, "lds_bytes": 53344, "lanes": 1024,
                                             "with_each_lane_reading_its_own_row_of_scores": {"vgprs": 26, "lds_bytes": 12384}},
             "ticker_sweep_kernel": {"vgprs": 86, "scratch_bytes": 0, "lds_bytes": 0, "waves_per_simd": 5,
                                     "before_the_step_loop_moved_into_ticker_sweep_dev.h": {"vgprs": 84, "scratch_bytes": 0, "waves_per_simd": 5}}}


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def engine(matrix, E, seed=1692):
    eng = _ffi.Engine(_ffi.ENV_TICKER, E, seed=seed, flags=_ffi.F_RESEED_EACH_RESET, max_episode_steps=STEPS)
    eng.ticker_set_table(matrix)
    eng.reset()
    return eng


def repeat(eng, fn, runs, warmup):
    ms = []
    for i in range(warmup + runs):
        eng.reset()
        eng.timer_start()
        fn()
        eng.timer_stop()
        t = eng.timer_ms()
        eng.wait()
        if i >= warmup:
            ms.append(t)
    return dict(stat(ms), clock="HIP events")


def case(matrix, E, C, runs, warmup):
    lib = _ffi.load_library(extra_signatures=dict(S.TICKERSEARCH_SIGNATURES, **W.TICKER_SWEEP_SIGNATURES))
    eng = engine(matrix, E)
    start = np.array(START, np.float32)
    z = np.ascontiguousarray(np.random.default_rng(0).standard_normal((G, C, 6)))
    box = [np.ascontiguousarray(v) for v in S.ticker_search_defaults(start)]
    r = {"case": "the search in one call", "envs": E, "generations": G, "candidates": C, "elites": ELITES, "steps": STEPS, "runs": runs,
         "warmup": warmup, "kernels": 2 * G}

    def one_call(steps):
        eng._check(lib.grl_ticker_search(eng.h, _ffi._ptr(start), *([_ffi._ptr(v) for v in box] + [_ffi._ptr(z), G, C, ELITES, steps])))
    r["ms_one_call"] = repeat(eng, lambda: one_call(STEPS), runs, warmup)
    r["ms_one_call_of_one_step_episodes"] = repeat(eng, lambda: one_call(1), runs, warmup)
    eng.reset()
    out = S.ticker_search(eng, start, generations=G, candidates=C, elites=ELITES, normals=z, max_steps=STEPS)
    table = np.ascontiguousarray(out["candidates"][G - 1])

    def sweeps():
        for _ in range(G):
            eng._check(lib.grl_ticker_sweep(eng.h, _ffi._ptr(table), C, STEPS, -1))
    r["ms_G_sweeps_of_C_rules"] = repeat(eng, sweeps, runs, warmup)
    r["one_call_over_G_sweeps"] = r["ms_one_call"]["median"] / r["ms_G_sweeps_of_C_rules"]["median"]
    r["one_step_call_over_one_call"] = r["ms_one_call_of_one_step_episodes"]["median"] / r["ms_one_call"]["median"]
    r["found"] = {"rule": out["best_rule"], "mean_total": out["best_fit"], "best_per_generation": out["best_per_generation"].tolist()}
    eng.reset()
    t0 = time.perf_counter()
    host = S.ticker_search_host(eng, start, generations=G, candidates=C, elites=ELITES, normals=z, max_steps=STEPS)
    sec = time.perf_counter() - t0
    r["host_composition"] = {"clock": "wall clock, ONE run", "ms": sec * 1e3,
                             "bits_equal_to_the_one_call": bool(all(host[k].tobytes() == out[k].tobytes() for k in S.OUTPUTS))}
    r["host_composition_over_one_call"] = sec * 1e3 / r["ms_one_call"]["median"]
    eng.close()
    return r


def scale(matrix, E=64):
    tuned_on, held = engine(matrix, E), engine(matrix, E, seed=7)
    i, rule, floor = TickerRuleBaseline(tuned_on).best_total()
    r = {"case": "the scale on the fixture table", "envs": E, "steps": STEPS, "search": [G, 32, ELITES],
         "best_default_rule": {"index": i, "rule": rule, "in_sample": floor}}
    one = TickerRuleSearch(tuned_on, generations=G, candidates=32, elites=ELITES)
    r["best_default_rule"]["held_out"] = one.play_on(held, rule)
    found, fit = one.best()
    r["tuned_from_the_best_default_rule"] = {"rule": found, "in_sample": fit, "held_out": one.play_on(held)}
    every = TickerRuleSearch(tuned_on, starts=DEFAULT_TICKER_RULES, generations=G, candidates=32, elites=ELITES)
    found, fit = every.best()
    r["tuned_from_every_default_rule"] = {"rule": found, "in_sample": fit, "held_out": every.play_on(held),
                                          "per_start": [{"start": s, "rule": f, "in_sample": v, "held_out": every.play_on(held, f)}
                                                        for s, f, v in every.results]}
    r["foresight_ceiling"] = {"in_sample": TickerForesightCeiling(tuned_on, (0,)).ceiling(), "held_out": TickerForesightCeiling(held, (0,)).ceiling()}
    tuned_on.close(); held.close()
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "ticker_search_times.json"))
    a = p.parse_args()
    matrix = np.load(os.path.join(ROOT, "tests", "golden", "ticker_rules.npz"))["matrix"]
    out = {"times": [], "resources": RESOURCES}
    for E, C in CASES:
        out["times"].append(case(matrix, E, C, a.runs, a.warmup))
        print(json.dumps(out["times"][-1]), flush=True)
    out["scale"] = scale(matrix)
    print(json.dumps(out["scale"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
