"""Greedy evaluation of the A3C Gaussian agent (include/goldsrl_gausseval.h): ms per 1 024-step evaluation of E envs by
  (a) eval              grl_anet_eval, one launch for the whole episode (and eval_traced: with the full trace, as PolicyMonitor calls it)
  (b) greedy_rollout    rollout(1024) with greedy on, five launches per step (this commit)
  (c) rollout           the stochastic rollout(1024) of the baseline checkout on the same handle size
  (d) host_monitor      wall clock of the baseline's host-driven GreedyMonitor.eval_once (scripts/train_solow.py; Solow, one env)
for Solow (cap 1 024, R = 5, scale 100) and TradeAR1 with 2 assets (cap 1 024, R = 20).  (a)-(c) by HIP events on the handle's
stream, median and spread (min, max) of the runs after the warm-up; every run starts from a reset handle.

    python tools/gauss_eval_times.py [--envs 64 4096 8192] [--runs 5] [--warmup 1] [--baseline PARENT_CHECKOUT] [--json OUT]

--baseline names a built checkout of the commit to compare against; (c) and (d) then run from it in a fresh process of the same
job (this script, with --root), and the ratios (a)/(c) and (d)/(a) are added.  Without it (c) and (d) are left out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 1024
RNN = {"solow": 5, "trade": 20}


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def make(kind, E, seed=3):
    from goldsrl import _ffi, _ffi_gauss
    if kind == "solow":
        eng = _ffi.Engine(_ffi.ENV_SOLOW, E, seed=seed, max_episode_steps=STEPS)
        net = _ffi_gauss.GaussNet(eng, rnn_length=RNN[kind], scale=100.0, max_samples=1)
        net.set_params(_ffi_gauss.default_init_gauss(seed, **_ffi_gauss.SOLOW_SIZES))
    else:
        eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=seed, n_assets=2, max_episode_steps=STEPS)
        net = _ffi_gauss.GaussNet(eng, rnn_length=RNN[kind], max_samples=1)
        net.set_params(_ffi_gauss.default_init_gauss(seed, **_ffi_gauss.TRADE_SIZES))
    return eng, net


def timed(eng, fn, runs, warmup):
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


def measure(kind, E, runs, warmup, has_eval):
    eng, net = make(kind, E)
    r = {"env": kind, "envs": E, "steps": STEPS, "rnn_length": RNN[kind], "runs": runs, "warmup": warmup, "clock": "HIP events"}
    if has_eval:
        r["ms_eval"] = timed(eng, lambda: net.lib.grl_anet_eval(net.n, STEPS, 0), runs, warmup)
        # the form PolicyMonitor.eval_once pays for: every env's five trace arrays written (it reads back the rewards)
        r["ms_eval_traced"] = timed(eng, lambda: net.lib.grl_anet_eval(net.n, STEPS, STEPS), runs, warmup)
        eng.reset()
        ev = net.eval(STEPS)
        r["episode_length"] = {"min": int(ev["length"].min()), "max": int(ev["length"].max())}
        net.set_greedy(True)
        r["ms_greedy_rollout"] = timed(eng, lambda: net.rollout(STEPS), runs, warmup)
    else:
        r["ms_rollout"] = timed(eng, lambda: net.rollout(STEPS), runs, warmup)
    net.close(); eng.close()
    return r


def host_monitor(runs, warmup):
    from goldsrl import _ffi_gauss
    from goldsrl.scripts import train_solow
    mon = train_solow.GreedyMonitor(0, os.devnull)
    params = _ffi_gauss.default_init_gauss(3, **_ffi_gauss.SOLOW_SIZES)
    ms = []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        _, length = mon.eval_once(params)[:2]
        dt = (time.perf_counter() - t0) * 1e3
        assert length == STEPS
        if i >= warmup:
            ms.append(dt)
    mon.close()
    return {"env": "solow", "envs": 1, "steps": STEPS, "runs": runs, "warmup": warmup, "clock": "wall", "ms_host_monitor": stat(ms)}


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, nargs="+", default=[64, 4096, 8192])
    p.add_argument("--kinds", nargs="+", default=["solow", "trade"], choices=["solow", "trade"])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose library and package are measured")
    p.add_argument("--baseline", help="a built checkout of the commit to compare against: (c) and (d) run from it")
    p.add_argument("--json", help="write the results here as well")
    a = p.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.root), "golds-rl-gym_amd"))
    from goldsrl import _ffi_gauss
    has_eval = hasattr(_ffi_gauss.GaussNet, "eval")
    out = {"cases": [], "host_monitor": None}
    for kind in a.kinds:
        for E in a.envs:
            r = measure(kind, E, a.runs, a.warmup, has_eval)
            out["cases"].append(r)
            print(json.dumps(r), flush=True)
    if not has_eval or not a.baseline:
        out["host_monitor"] = host_monitor(a.runs, a.warmup)
        print(json.dumps(out["host_monitor"]), flush=True)
    if a.baseline:
        tmp = (a.json or os.path.join(os.getcwd(), "gauss_eval_times.json")) + ".baseline"
        cmd = [sys.executable, os.path.abspath(__file__), "--root", a.baseline, "--json", tmp, "--runs", str(a.runs), "--warmup", str(a.warmup),
               "--kinds"] + a.kinds + ["--envs"] + [str(e) for e in a.envs]
        subprocess.run(cmd, check=True, env={k: v for k, v in os.environ.items() if k != "PYTHONPATH"})
        with open(tmp) as f:
            base = json.load(f)
        os.remove(tmp)
        out["host_monitor"] = base["host_monitor"]
        host = base["host_monitor"]["ms_host_monitor"]["median"]
        for r, b in zip(out["cases"], base["cases"]):
            assert (r["env"], r["envs"]) == (b["env"], b["envs"])
            r["ms_rollout_baseline"] = b["ms_rollout"]
            r["eval_over_baseline_rollout"] = r["ms_eval"]["median"] / b["ms_rollout"]["median"]
            if r["env"] == "solow":      # one host-driven episode against E episodes on the device
                r["host_monitor_over_eval"] = host / r["ms_eval"]["median"]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
