"""A3C Gaussian agent on the device (include/goldsrl_gaussnet.h), both size sets, next to the Ticker gated trader as the yardstick
from the same job: ms per rollout and per update at E envs x T steps by HIP events on the handle's stream, env-steps/s, MACs counted
from the layer shapes.

    python tools/gauss_update_times.py [--envs 4096 8192] [--steps 20] [--rnn 5] [--runs 10] [--warmup 3] [--json OUT]
    python tools/gauss_update_times.py --trace solow --envs 8192 --runs 3 --warmup 1      # the workload alone, for a kernel trace

Each timed run is one rollout(T) between two events and one train_rollout between two events; median and spread (min, max) of the
runs.  The Solow envs run with the reference's 1 024-step cap and scale 100, the TradeAR1 envs with scale 1, the Ticker envs on the
synthetic 1 400-row table of tests/golden/ticker.npz."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_gated, _ffi_gauss  # noqa: E402


def macs_per_sample(net, R):
    """forward MACs of one sample, and those of the recomputing backward (forward again + data and weight gradients; the trunk is
    back-propagated once per loss)"""
    D, S0, heads = {"gated": (4, 7, (6, 12)), "solow": (2, 2, (1, 1)), "trade": (5, 5, (2, 2))}[net]
    gru = R * ((D + 32) * 64 + (D + 32) * 32)
    trunk = 32 * 64 + S0 * 64 + 64 * 32
    towers = sum(96 * 256 + 256 * 128 + 128 * h for h in heads)
    val = 96 * 256 + 256
    fwd = gru + trunk + towers + val
    return fwd, fwd + 2 * (towers + val) + 2 * 2 * (gru + trunk)


def make(net, E, R, seed=3):
    if net == "gated":
        eng = _ffi.Engine(_ffi.ENV_TICKER, E, seed=seed)
        eng.ticker_set_table(np.load(os.path.join(ROOT, "tests", "golden", "ticker.npz"))["matrix"])
        eng.reset()
        n = _ffi_gated.GatedNet(eng, rnn_length=R, max_samples=E)
        n.set_params(_ffi_gated.default_init_gated(seed))
    elif net == "solow":
        eng = _ffi.Engine(_ffi.ENV_SOLOW, E, seed=seed)
        eng.reset()
        n = _ffi_gauss.GaussNet(eng, rnn_length=R, scale=100.0, max_samples=E)
        n.set_params(_ffi_gauss.default_init_gauss(seed, **_ffi_gauss.SOLOW_SIZES))
    else:
        eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=seed, n_assets=2)
        eng.reset()
        n = _ffi_gauss.GaussNet(eng, rnn_length=R, max_samples=E)
        n.set_params(_ffi_gauss.default_init_gauss(seed, **_ffi_gauss.TRADE_SIZES))
    return eng, n


def measure(net, E, T, R, runs, warmup):
    eng, n = make(net, E, R)
    ro, up = [], []
    for i in range(warmup + runs):
        eng.timer_start()
        n.rollout(T)
        eng.timer_stop()
        t_ro = eng.timer_ms()
        eng.timer_start()
        n.train_rollout(1e-4)
        eng.timer_stop()
        t_up = eng.timer_ms()
        if i >= warmup:
            ro.append(t_ro); up.append(t_up)
    n.close(); eng.close()
    fwd, bwd = macs_per_sample(net, R)
    mro, mup = float(np.median(ro)), float(np.median(up))
    return {
        "net": net, "envs": E, "steps": T, "rnn_length": R, "runs": runs, "warmup": warmup, "clock": "HIP events",
        "ms_per_rollout": {"median": mro, "min": float(np.min(ro)), "max": float(np.max(ro))},
        "ms_per_update": {"median": mup, "min": float(np.min(up)), "max": float(np.max(up))},
        "env_steps_per_s": E * T / ((mro + mup) * 1e-3),
        "mac_per_sample": {"forward": fwd, "update": bwd},
    }


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, nargs="+", default=[4096, 8192])
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--rnn", type=int, default=5)
    p.add_argument("--runs", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--nets", nargs="+", default=["gated", "solow", "trade"], choices=["gated", "solow", "trade"])
    p.add_argument("--trace", choices=["gated", "solow", "trade"], help="run this net's workload only and print nothing but a summary")
    p.add_argument("--json", help="write the results here as well")
    a = p.parse_args()
    nets = [a.trace] if a.trace else a.nets
    out = []
    for E in a.envs:
        for net in nets:
            r = measure(net, E, a.steps, a.rnn, a.runs, a.warmup)
            out.append(r)
            print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
