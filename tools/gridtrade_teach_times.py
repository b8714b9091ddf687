"""The grid trader's teach path (include/goldsrl_gridtradeteach.h) beside its plain path on the SAME handle in the same run: ms per
teach_rollout(64) beside rollout(64) and per train_teach_rollout beside train_rollout, at E envs with R = 20 and K = 17 / 48, by HIP
events on the handle's stream; and the scale rows of the taught K = 17 agent on the 64 seeded eval episodes.

    python tools/gridtrade_teach_times.py [--envs 4096 8192] [--steps 64] [--runs 5] [--warmup 1]
                                          [--teach-updates 50 200] [--a3c-updates 200] [--json OUT]

Each timed run is, per K: rollout, train_rollout, teach_rollout (agent_share 0.5: the coin is drawn), train_teach_rollout, each
between two events; median and spread (min, max) of the runs.  No ratio is gated: the design's claim is that the teacher rides on
the forward's idle waves and that the rollout is launch-bound, so `teach_rollout_over_rollout` is expected near 1, and whatever it
is is written down.  The scale rows (--teach-updates N .., each at agent_share 0 and 0.5; then --a3c-updates A3C updates started
from the largest N at agent_share 0): 4 096 envs x 64 steps per update, every yardstick played directly before the evaluation, as
tools/gridtrade_update_times.py does.  Default output: profiles/gridtrade_teach_times.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_gridtrade  # noqa: E402
from goldsrl.agents.a3c.policy_monitor import GridTradeMonitor  # noqa: E402
from goldsrl.baselines import TradeOptimalBaseline  # noqa: E402

KS, R, EVAL_STEPS = (17, 48), 20, 1024
CALLS = ("rollout", "train_rollout", "teach_rollout", "train_teach_rollout")


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def trainer(E, K, seed=3):
    """a training engine with TradeOptimalBaseline's default table solved on it, and the net at its default initialisation"""
    eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=seed, n_assets=2, max_episode_steps=EVAL_STEPS)
    eng.reset()
    TradeOptimalBaseline(eng).solve()
    net = _ffi_gridtrade.GridTradeNet(eng, rnn_length=R, num_choices=K, max_samples=1)
    net.set_params(_ffi_gridtrade.default_init_gridtrade(seed, K))
    return eng, net


def measure(E, T, runs, warmup):
    r = {"envs": E, "steps": T, "rnn_length": R, "runs": runs, "warmup": warmup, "clock": "HIP events", "agent_share": 0.5}
    for K in KS:
        eng, net = trainer(E, K)
        fns = {"rollout": lambda: net.rollout(T), "train_rollout": lambda: net.train_rollout(1e-4),
               "teach_rollout": lambda: net.teach_rollout(T, 0.5), "train_teach_rollout": lambda: net.train_teach_rollout(1e-4)}
        ms = {k: [] for k in CALLS}
        for i in range(warmup + runs):
            for k in CALLS:
                t = timed(eng, fns[k])
                if i >= warmup:
                    ms[k].append(t)
        g = {"ms_" + k: stat(ms[k]) for k in CALLS}
        g["teach_rollout_over_rollout"] = g["ms_teach_rollout"]["median"] / g["ms_rollout"]["median"]
        g["train_teach_over_train"] = g["ms_train_teach_rollout"]["median"] / g["ms_train_rollout"]["median"]
        r["grid%d" % K] = g
        net.close(); eng.close()
    return r


def scale_rows(teach_updates, a3c_updates, E=4096, T=64, K=17, eval_envs=64, lr=1e-4):
    mon = GridTradeMonitor(n_envs=eval_envs, n_grid=K, max_seq_length=R)

    def row(net, **what):
        out = dict(what, best_rule=mon.rule_baseline()[2], attainable_optimum=mon.trade_optimal())
        mon.eval_once(net.get_params())
        out["agent"] = mon.log["mean_total_reward"][-1]
        print(json.dumps(out), flush=True)
        return out

    rows = []
    for share in (0.0, 0.5):
        eng, net = trainer(E, K)
        done = 0
        for N in sorted(teach_updates):
            for _ in range(N - done):
                net.teach_rollout(T, share)
                st = net.train_teach_rollout(lr)
            done = N
            rows.append(row(net, teach_updates=N, agent_share=share, a3c_updates=0, cross_entropy=st["cross_entropy"], agreement=st["agreement"]))
        if share == 0.0 and a3c_updates > 0:
            for _ in range(a3c_updates):
                net.rollout(T)
                net.train_rollout(lr)
            rows.append(row(net, teach_updates=done, agent_share=share, a3c_updates=a3c_updates))
        net.close(); eng.close()
    mon.close()
    return {"eval_envs": eval_envs, "num_choices": K, "train_envs": E, "train_steps": T, "lr": lr, "rows": rows}


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, nargs="*", default=[4096, 8192])
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--teach-updates", type=int, nargs="*", default=[50, 200])
    p.add_argument("--a3c-updates", type=int, default=200)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "gridtrade_teach_times.json"))
    a = p.parse_args()
    out = {"times": [], "scale": None}
    for E in a.envs:
        out["times"].append(measure(E, a.steps, a.runs, a.warmup))
        print(json.dumps(out["times"][-1]), flush=True)
    if a.teach_updates:
        out["scale"] = scale_rows(a.teach_updates, a.a3c_updates)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
