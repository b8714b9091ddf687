"""Ticker gated trader on the device (include/goldsrl_gatednet.h): ms per rollout and per update at E envs x T steps, env-steps/s,
FLOPs counted from the layer shapes and the fraction of the fp32 matrix-core floor they imply.

    python tools/gated_update_times.py [--envs 4096 8192] [--steps 20] [--rnn 5] [--runs 10] [--warmup 3] [--json OUT]

Each timed run is one grl_gnet_rollout(T) (synchronised) and one grl_gnet_train_rollout; median and spread (min, max) of the runs.
The price table is the synthetic 1 400-row table of tests/golden/ticker.npz."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_gated  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12     # MI355X fp32 matrix peak (v_mfma_f32_32x32x2_f32: 64 FLOP/clk/SIMD, the vector fp32 rate)


def macs_per_sample(R):
    """forward MACs of one sample, and those of the recomputing backward (forward again + data and weight gradients; the trunk
    is back-propagated once per loss)."""
    gru = R * ((4 + 32) * 64 + (4 + 32) * 32)
    trunk = 32 * 64 + 7 * 64 + 64 * 32
    cls = 96 * 256 + 256 * 128 + 128 * 6
    nrm = 96 * 256 + 256 * 128 + 128 * 12
    val = 96 * 256 + 256
    fwd = gru + trunk + cls + nrm + val
    bwd = fwd + 2 * (cls + nrm + val) + 2 * 2 * (gru + trunk)
    return fwd, bwd


def measure(E, T, R, runs, warmup, seed=3):
    g = np.load(os.path.join(ROOT, "tests", "golden", "ticker.npz"))
    eng = _ffi.Engine(_ffi.ENV_TICKER, E, seed=seed)
    eng.ticker_set_table(g["matrix"])
    eng.reset()
    net = _ffi_gated.GatedNet(eng, rnn_length=R, max_samples=E)
    net.set_params(_ffi_gated.default_init_gated(seed))
    ro, up = [], []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        net.rollout(T)
        net.read_rollout("boot")          # synchronises the stream
        t1 = time.perf_counter()
        net.train_rollout(1e-4)           # synchronous
        t2 = time.perf_counter()
        if i >= warmup:
            ro.append((t1 - t0) * 1e3); up.append((t2 - t1) * 1e3)
    net.close(); eng.close()
    fwd, bwd = macs_per_sample(R)
    ro_flop = 2.0 * fwd * E * (T + 1)
    up_flop = 2.0 * bwd * E * T
    mro, mup = float(np.median(ro)), float(np.median(up))
    return {
        "envs": E, "steps": T, "rnn_length": R, "runs": runs, "warmup": warmup,
        "ms_per_rollout": {"median": mro, "min": float(np.min(ro)), "max": float(np.max(ro))},
        "ms_per_update": {"median": mup, "min": float(np.min(up)), "max": float(np.max(up))},
        "env_steps_per_s": E * T / ((mro + mup) * 1e-3),
        "gflop_rollout": ro_flop / 1e9, "gflop_update": up_flop / 1e9,
        "fp32_matrix_floor_ms": {"rollout": ro_flop / FP32_MATRIX_PEAK * 1e3, "update": up_flop / FP32_MATRIX_PEAK * 1e3},
        "fraction_of_floor": {"rollout": ro_flop / FP32_MATRIX_PEAK / (mro * 1e-3), "update": up_flop / FP32_MATRIX_PEAK / (mup * 1e-3)},
        "mac_per_sample": {"forward": fwd, "update": bwd},
    }


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, nargs="+", default=[4096, 8192])
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--rnn", type=int, default=5)
    p.add_argument("--runs", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--json", help="write the results here as well")
    a = p.parse_args()
    out = []
    for E in a.envs:
        r = measure(E, a.steps, a.rnn, a.runs, a.warmup)
        out.append(r)
        print(json.dumps(r), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
