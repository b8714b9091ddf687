"""Constant-savings baseline sweep of the Solow env (include/goldsrl_sweep.h): ms per sweep of 20 rates x 1 024 steps by HIP events
on the handle's stream, for 1, 2 and 4 rates per lane (GRL_SWEEP_RPL), next to the same work through the per-step path on the SAME
handle in the same run (20 x 1 024 grl_step_device calls on a constant action buffer) and, for scale, one 1 024-step greedy
evaluation of the savings-grid policy (grl_dnet_eval).

    python tools/solow_sweep_times.py [--envs 1 4096 8192] [--runs 5] [--warmup 1] [--json OUT]

Every run starts from a reset handle; median and spread (min, max) of the runs.  The expectation is structural only: the sweep is
one launch of dependent expf / powf / logf chains where the per-step path is 20 480 launches, so it should take a small fraction
of it and well under one policy evaluation.  The registers and scratch of the three instantiations (tools/kres.sh
solow_sweep.hip, kept in profiles/solow_sweep_kres.txt) are recorded next to the times.  Default output:
profiles/solow_sweep_times.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_discrete, _ffi_sweep  # noqa: E402
from goldsrl.agents.a3c.policy_monitor import make_eval_engine  # noqa: E402

STEPS = 1024
RATES = np.linspace(0.05, 0.95, 20).astype(np.float32)


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def measure(E, runs, warmup):
    lib = _ffi.load_library(extra_signatures=_ffi_sweep.SWEEP_SIGNATURES)
    eng = make_eval_engine("Solow-1-1-finite-eval-v0", E, max_episode_steps=STEPS)
    r = {"envs": E, "rates": len(RATES), "steps": STEPS, "runs": runs, "warmup": warmup, "clock": "HIP events", "ms_sweep": {}}
    for rpl in (1, 2, 4):
        os.environ["GRL_SWEEP_RPL"] = str(rpl)
        ms = []
        for i in range(warmup + runs):
            eng.reset()
            t = timed(eng, lambda: eng._check(lib.grl_solow_sweep(eng.h, _ffi._ptr(RATES), len(RATES), STEPS, -1)))
            if i >= warmup:
                ms.append(t)
        r["ms_sweep"]["rpl%d" % rpl] = stat(ms)
    del os.environ["GRL_SWEEP_RPL"]
    bufs = []
    for s in RATES:
        bufs.append(eng.dev_alloc(4 * E))
        eng.dev_upload(bufs[-1], np.full(E, s, np.float32))

    def per_step():
        for b in bufs:          # the TimeLimit's auto-reset after 1 024 steps restarts the seeded episode for the next rate
            for _ in range(STEPS):
                eng.step_device(b)
    ms = []
    for i in range(warmup + runs):
        eng.reset()
        t = timed(eng, per_step)
        eng.wait()
        if i >= warmup:
            ms.append(t)
    r["ms_per_step_path"] = stat(ms)
    net = _ffi_discrete.DiscreteNet(eng, rnn_length=5, num_choices=51, max_samples=1)
    net.set_params(_ffi_discrete.default_init_discrete(3, 51))
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
    r["sweep_over_policy_eval"] = r["ms_sweep"][best]["median"] / r["ms_policy_eval"]["median"]
    return r


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, nargs="+", default=[1, 4096, 8192])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "solow_sweep_times.json"))
    a = p.parse_args()
    out = {"times": [], "resources": None}
    kres = os.path.join(ROOT, "profiles", "solow_sweep_kres.txt")
    if os.path.exists(kres):
        out["resources"] = [ln.strip() for ln in open(kres) if ln.strip()]
    for E in a.envs:
        out["times"].append(measure(E, a.runs, a.warmup))
        print(json.dumps(out["times"][-1]), flush=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
