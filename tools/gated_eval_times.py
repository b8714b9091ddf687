"""Greedy evaluation of the Ticker gated trader (include/goldsrl_gatedeval.h): ms per 1 023-step evaluation of E envs by
  (a) eval              grl_gnet_eval, one launch for the whole episode (and eval_traced: with the full trace, as GatedPolicyMonitor
                        calls it)
  (b) greedy_rollout    rollout(1023) with greedy on, five launches per step (this commit)
  (c) rollout           the stochastic rollout(1023) of the baseline checkout on the same handle size
on a synthetic price table (a seeded random walk of 4 096 rows), cap 1 023, R = 5.  By HIP events on the handle's stream, median and
spread (min, max) of the runs after the warm-up; every run starts from a reset handle.

    python tools/gated_eval_times.py [--envs 64 4096 8192] [--runs 5] [--warmup 1] [--baseline PARENT_CHECKOUT] [--json OUT]

--baseline names a built checkout of the commit to compare against; (c) then runs from it in a fresh process of the same job (this
script, with --root), and the ratios (a)/(c) and (a)/(b) are added.  Without it (c) is left out."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS, RNN, ROWS = 1023, 5, 4096


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def table(seed=11):
    """(ROWS,4) float64: price, inverse price, volume, volume -- the columns of OpenCloseSampler.data_matrix"""
    rng = np.random.RandomState(seed)
    logp = np.cumsum(0.01 * rng.normal(size=ROWS))
    vol = 0.1 * rng.normal(size=ROWS)
    return np.stack([100.0 * np.exp(logp), 100.0 * np.exp(-logp), vol, vol], axis=1)


def make(E, seed=3):
    from goldsrl import _ffi, _ffi_gated
    eng = _ffi.Engine(_ffi.ENV_TICKER, E, seed=seed, max_episode_steps=STEPS)
    eng.ticker_set_table(table())
    net = _ffi_gated.GatedNet(eng, rnn_length=RNN, max_samples=1)
    net.set_params(_ffi_gated.default_init_gated(seed))
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


def measure(E, runs, warmup, has_eval):
    eng, net = make(E)
    r = {"env": "ticker", "envs": E, "steps": STEPS, "rnn_length": RNN, "runs": runs, "warmup": warmup, "clock": "HIP events"}
    if has_eval:
        r["ms_eval"] = timed(eng, lambda: net.lib.grl_gnet_eval(net.n, STEPS, 0), runs, warmup)
        # the form GatedPolicyMonitor.eval_once pays for: every env's seven trace arrays written (it reads back the rewards)
        r["ms_eval_traced"] = timed(eng, lambda: net.lib.grl_gnet_eval(net.n, STEPS, STEPS), runs, warmup)
        eng.reset()
        ev = net.eval(STEPS)
        r["episode_length"] = {"min": int(ev["length"].min()), "max": int(ev["length"].max())}
        net.set_greedy(True)
        r["ms_greedy_rollout"] = timed(eng, lambda: net.rollout(STEPS), runs, warmup)
        r["eval_over_greedy_rollout"] = r["ms_eval"]["median"] / r["ms_greedy_rollout"]["median"]
    else:
        r["ms_rollout"] = timed(eng, lambda: net.rollout(STEPS), runs, warmup)
    net.close(); eng.close()
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, nargs="+", default=[64, 4096, 8192])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose library and package are measured")
    p.add_argument("--baseline", help="a built checkout of the commit to compare against: (c) runs from it")
    p.add_argument("--json", help="write the results here as well")
    a = p.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.root), "golds-rl-gym_amd"))
    from goldsrl import _ffi_gated
    has_eval = hasattr(_ffi_gated.GatedNet, "eval")
    out = {"cases": []}
    for E in a.envs:
        r = measure(E, a.runs, a.warmup, has_eval)
        out["cases"].append(r)
        print(json.dumps(r), flush=True)
    if a.baseline:
        tmp = (a.json or os.path.join(os.getcwd(), "gated_eval_times.json")) + ".baseline"
        cmd = [sys.executable, os.path.abspath(__file__), "--root", a.baseline, "--json", tmp, "--runs", str(a.runs), "--warmup", str(a.warmup),
               "--envs"] + [str(e) for e in a.envs]
        subprocess.run(cmd, check=True, env={k: v for k, v in os.environ.items() if k != "PYTHONPATH"})
        with open(tmp) as f:
            base = json.load(f)
        os.remove(tmp)
        for r, b in zip(out["cases"], base["cases"]):
            assert r["envs"] == b["envs"]
            r["ms_rollout_baseline"] = b["ms_rollout"]
            r["eval_over_baseline_rollout"] = r["ms_eval"]["median"] / b["ms_rollout"]["median"]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
