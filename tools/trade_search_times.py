"""The cross-entropy search over a TradeAR1 rule's four numbers in one call (include/goldsrl_tradesearch.h) next to what it replaces,
measured in the same run on the eval registration's seeded envs.  The search starts from (100, 100, 0, 1) with the default spreads,
G = 8, 8 elites, 1 024 steps, (E, C) in (1, 32), (64, 64), (4 096, 64), (8 192, 64), at 2 and at 16 assets:

  (a) grl_trade_search, one call: G evaluations and G updates on the handle's stream, nothing read back between them; ms by HIP
      events on the stream around the call (the uploads included, reads not), median and spread (min, max) of the runs after the
      warm-up.  The call does not move the handle, so every run plays the same episodes.  Per GRL_TRADE_SEARCH_RPL = 1 / 2 / 4;
  (b) the same call with max_steps = 1: the uploads, 2 G launches and the update kernel's E loads per candidate, next to no evaluation
      -- what the update kernel and the call's fixed part cost at that size;
  (c) eight grl_trade_sweep calls of C rules (the last generation's (gain_buy, bias) columns) over 1 024 steps on the same handle at
      the sweep's default rules per lane, HIP events around the eight: what the evaluations cost in the sweep's form, nine outputs
      per pair where the search writes one.  That sweep is this tree's, whose kernel instantiates the shared loop of
      trade_sweep_dev.h; it stands for the parent commit's only as far as the sweep's own times before and after that move are
      equal, which LABNOTES.md (section AC) gives from both libraries in one job;
  (d) with --host, trade_search_host at the two small sizes on a noise-injecting twin with a recorded tape: per generation C x 1 024
      grl_step calls with the actions computed in numpy.  WALL CLOCK, ONE RUN; its six outputs are compared with the one call's
      on the same tape as bytes;
  (e) the scale (goldsrl/scripts/trade_search.py): 64 envs x 256 steps, seeds 1692 and 1693, at 2 and at 16 assets: the best default
      rule, the tuned rule where it was tuned and on the other seeds, the foresight ceiling.

    python tools/trade_search_times.py [--runs 5] [--warmup 1] [--host] [--json OUT]

Default output: profiles/trade_search_times.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_tradesearch as S, _ffi_tradesweep as W  # noqa: E402
from goldsrl.scripts import trade_search as scale_script  # noqa: E402

STEPS = 1024
G, ELITES = 8, 8
CASES = ((1, 32), (64, 64), (4096, 64), (8192, 64))
ASSETS = (2, 16)
START = (100, 100, 0, 1)
# hipcc -O3 --offload-arch=gfx950 -ffp-contract=off, VGPRs by asset tier NT = 2 / 4 / 8 / 16 / LDS; no scratch anywhere
RESOURCES = {"trade_search_eval_kernel": {"rpl1": [129, 161, 186, 234, 129], "rpl2": [153, 183, 216, 280, 136], "rpl4": [201, 246, 294, 388, 162],
                                          "scratch_bytes": 0, "lds_bytes_per_wave_at_17_to_64_assets": "(1 + RPL) * n * 512"},
             "trade_search_update_kernel": {"vgprs": 50, "scratch_bytes": 0, "lds_bytes": 53312, "lanes": 1024},
             "trade_sweep_kernel": {"rpl1": [136, 165, 190, 238, 128], "rpl2": [173, 213, 244, 314, 153], "rpl4": [251, 300, 344, 452, 199],
                                    "scratch_bytes": 0,
                                    "before_the_step_loop_moved_into_trade_sweep_dev.h": {"rpl1": [136, 165, 190, 238, 128], "rpl2": [174, 213, 244, 314, 150],
                                                                                          "rpl4": [251, 294, 342, 448, 189], "scratch_bytes": 0}}}


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def repeat(eng, fn, runs, warmup):
    ms = []
    for i in range(warmup + runs):
        eng.timer_start()
        fn()
        eng.timer_stop()
        t = eng.timer_ms()
        eng.wait()
        if i >= warmup:
            ms.append(t)
    return dict(stat(ms), clock="HIP events")


def case(n, E, C, runs, warmup, host):
    lib = _ffi.load_library(extra_signatures=dict(S.TRADESEARCH_SIGNATURES, **W.TRADE_SWEEP_SIGNATURES))
    eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=1692, n_assets=n, max_episode_steps=STEPS)
    eng.reset()
    start = np.array(START, np.float32)
    z = np.ascontiguousarray(np.random.default_rng(0).standard_normal((G, C, 4)))
    box = [np.ascontiguousarray(v) for v in S.trade_search_defaults(start)]
    r = {"case": "the search in one call", "n_assets": n, "envs": E, "generations": G, "candidates": C, "elites": ELITES, "steps": STEPS,
         "runs": runs, "warmup": warmup, "kernels": 2 * G, "ms_one_call": {}}

    def one_call(steps):
        eng._check(lib.grl_trade_search(eng.h, _ffi._ptr(start), *([_ffi._ptr(v) for v in box] + [_ffi._ptr(z), None, G, C, ELITES, steps])))
    for rpl in (1, 2, 4):
        os.environ["GRL_TRADE_SEARCH_RPL"] = str(rpl)
        r["ms_one_call"]["rpl%d" % rpl] = repeat(eng, lambda: one_call(STEPS), runs, warmup)
    del os.environ["GRL_TRADE_SEARCH_RPL"]
    r["ms_one_call"]["default"] = repeat(eng, lambda: one_call(STEPS), runs, warmup)
    r["ms_one_call_of_one_step_episodes"] = repeat(eng, lambda: one_call(1), runs, warmup)
    out = S.trade_search(eng, start, generations=G, candidates=C, elites=ELITES, normals=z, max_steps=STEPS)
    gains, biases = np.ascontiguousarray(out["candidates"][G - 1, :, 0]), np.ascontiguousarray(out["candidates"][G - 1, :, 2])

    def sweeps():
        for _ in range(G):
            eng._check(lib.grl_trade_sweep(eng.h, _ffi._ptr(gains), _ffi._ptr(biases), C, None, STEPS, -1))
    r["ms_G_sweeps_of_C_rules"] = repeat(eng, sweeps, runs, warmup)
    r["fastest"] = min(("rpl1", "rpl2", "rpl4"), key=lambda k: r["ms_one_call"][k]["median"])
    r["one_call_over_G_sweeps"] = r["ms_one_call"]["default"]["median"] / r["ms_G_sweeps_of_C_rules"]["median"]
    r["one_step_call_over_one_call"] = r["ms_one_call_of_one_step_episodes"]["median"] / r["ms_one_call"]["default"]["median"]
    r["found"] = {"rule": out["best_rule"], "mean_total": out["best_fit"], "best_per_generation": out["best_per_generation"].tolist()}
    eng.close()
    if host:
        twin = _ffi.Engine(_ffi.ENV_TRADE, E, seed=1692, n_assets=n, max_episode_steps=STEPS, flags=_ffi.F_INJECT_NOISE)
        twin.reset()
        tape = np.random.RandomState(n).normal(size=(STEPS, E, n)).astype(np.float32)
        kw = dict(generations=G, candidates=C, elites=ELITES, normals=z, max_steps=STEPS, tape=tape)
        dev = S.trade_search(twin, start, **kw)
        t0 = time.perf_counter()
        got = S.trade_search_host(twin, start, **kw)
        sec = time.perf_counter() - t0
        r["host_composition"] = {"clock": "wall clock, ONE run", "ms": sec * 1e3, "env_steps": G * C * STEPS,
                                 "bits_equal_to_the_one_call": bool(all(got[k].tobytes() == dev[k].tobytes() for k in S.OUTPUTS))}
        r["host_composition_over_one_call"] = sec * 1e3 / r["ms_one_call"]["default"]["median"]
        twin.close()
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--host", action="store_true", help="also time trade_search_host at the two small sizes (minutes)")
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "trade_search_times.json"))
    a = p.parse_args()
    out = {"times": [], "resources": RESOURCES, "scale": []}
    for n in ASSETS:
        for E, C in CASES:
            out["times"].append(case(n, E, C, a.runs, a.warmup, a.host and E <= 64))
            print(json.dumps(out["times"][-1]), flush=True)
    for n in ASSETS:
        out["scale"].append(scale_script.main(["--n-assets", str(n), "--envs", "64", "--steps", "256", "--search", "%d:32:%d" % (G, ELITES)]))
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
