#!/usr/bin/env python3
"""Golden fixture for the constant-savings baseline (reference scripts/constant_solow.py), made by running the UNMODIFIED script
under the stand-ins of _ref_stubs.py.  Build container only:  python tests/golden/gen_golden_constant_solow.py

The script itself is run (runpy, as __main__) and its three printed lines `p s_max max_mean (max, min, std)` are parsed.  Then the
same three eval envs are made through the stubs and played once per rate, recording what a device test needs to replay them: the
reset z, the last 1 024 entries of the shock tape (popped from the end), the rates, the per-rate statistics in float64 and the step
rewards of three rates.  The generator's own best rate must equal the script's printed line."""
import contextlib
import io
import os
import re
import runpy
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_stubs  # noqa: E402

REFERENCE = "/root/reference"
_ref_stubs.install(REFERENCE)
import gym  # noqa: E402

TRACED = (0, 6, 19)
_FLOAT = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"


def printed_lines():
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        runpy.run_path(os.path.join(REFERENCE, "scripts", "constant_solow.py"), run_name="__main__")
    lines = [ln for ln in buf.getvalue().splitlines() if ln.strip()]
    assert len(lines) == 3, lines
    out = {}
    for ln in lines:
        vals = [float(v) for v in re.findall(_FLOAT, ln.replace("np.float64", ""))]
        assert len(vals) == 6, ln
        out[int(vals[0])] = vals[1:]          # s_max, max_mean, max, min, std
    return out


def main():
    printed = printed_lines()
    out = {}
    rates = np.linspace(0.05, 0.95, 20)
    for p in (1, 2, 3):
        env = gym.envs.make("Solow-%d-%d-finite-eval-v0" % (p, p))
        pre = "p%d_" % p
        s_max, max_mean, stats = 0, 0, None
        mean, mx, mn, std, total, traces = [], [], [], [], [], []
        for i, s in enumerate(rates):
            env.reset()
            if i == 0:
                out[pre + "z0"] = np.array(env.unwrapped.z, np.float64)
                out[pre + "tape_tail"] = np.array(env.unwrapped.es, np.float64)[-1024:]
            else:       # the eval registration reseeds at every reset: every rate sees the same episode
                assert np.array_equal(out[pre + "z0"], env.unwrapped.z)
                assert np.array_equal(out[pre + "tape_tail"], np.array(env.unwrapped.es)[-1024:])
            done, rewards = False, []
            while not done:
                _, reward, done, _ = env.step(s)
                rewards.append(reward)
            assert len(rewards) == 1024
            r = np.array(rewards, np.float64)
            mean.append(np.mean(rewards)); mx.append(np.max(rewards)); mn.append(np.min(rewards)); std.append(np.std(rewards))
            total.append(np.sum(r))
            if i in TRACED:
                traces.append(r)
            if mean[-1] > max_mean:
                max_mean, s_max, stats = mean[-1], s, (mx[-1], mn[-1], std[-1])
        assert [s_max, max_mean] + list(stats) == printed[p], (p, s_max, max_mean, stats, printed[p])
        out[pre + "printed"] = np.array(printed[p], np.float64)
        out[pre + "best_index"] = np.array(int(np.argmin(np.abs(rates - s_max))))
        for k, v in (("mean", mean), ("max", mx), ("min", mn), ("std", std), ("total", total)):
            out[pre + k] = np.array(v, np.float64)
        out[pre + "rewards"] = np.array(traces, np.float64)
        print(p, s_max, max_mean, stats)
    out["rates"] = rates
    out["traced"] = np.array(TRACED)
    path = os.path.join(HERE, "constant_solow.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
