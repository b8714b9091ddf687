"""A3C grid trader on the device (include/goldsrl_gridtradenet.h), next to the Gaussian agent on the SAME TradeAR1 handle in the same
run: ms per rollout(64) and per update at E envs with R = 20 and K = 17 / 48 by HIP events on the handle's stream, ms per 1 024-step
greedy evaluation of E envs in one launch against the per-step greedy rollout, and the scale row on 64 seeded eval envs.

    python tools/gridtrade_update_times.py [--envs 4096 8192] [--steps 64] [--eval-envs 8192] [--runs 5] [--warmup 1]
                                           [--scale-updates 200] [--json OUT]

Each timed run is, for the Gaussian net and then the grid net of each K, one rollout(T) between two events and one train_rollout
between two events; median and spread (min, max) of the runs.  Reported, not gated: on Solow the one-tower net's update took 0.74 of
the Gaussian's (profiles/discrete_update_times.json); whatever comes out here is written down as `update_over_gauss`.  The scale
row: best default rule / tuned rule / the K = 17 agent after --scale-updates updates of 4 096 envs x 64 steps / attainable optimum /
foresight ceiling, every one the mean total reward of the same 64 eval episodes (GridTradeMonitor, each yardstick played directly
before the evaluation).  Default output: profiles/gridtrade_update_times.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_gauss, _ffi_gridtrade  # noqa: E402
from goldsrl.agents.a3c.policy_monitor import GridTradeMonitor  # noqa: E402

KS, R, EVAL_STEPS = (17, 48), 20, 1024


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def nets(eng, seed=3):
    g = _ffi_gauss.GaussNet(eng, rnn_length=R, max_samples=1)
    g.set_params(_ffi_gauss.default_init_gauss(seed, **_ffi_gauss.TRADE_SIZES))
    out = {"gauss": g}
    for K in KS:
        out["grid%d" % K] = _ffi_gridtrade.GridTradeNet(eng, rnn_length=R, num_choices=K, max_samples=1)
        out["grid%d" % K].set_params(_ffi_gridtrade.default_init_gridtrade(seed, K))
    return out


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def measure_update(E, T, runs, warmup):
    eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=3, n_assets=2, max_episode_steps=EVAL_STEPS)
    eng.reset()
    ns = nets(eng)
    ms = {k: {"rollout": [], "update": []} for k in ns}
    for i in range(warmup + runs):
        for k, n in ns.items():
            t_ro = timed(eng, lambda: n.rollout(T))
            t_up = timed(eng, lambda: n.train_rollout(1e-4))
            if i >= warmup:
                ms[k]["rollout"].append(t_ro); ms[k]["update"].append(t_up)
    for n in ns.values():
        n.close()
    eng.close()
    r = {"envs": E, "steps": T, "rnn_length": R, "runs": runs, "warmup": warmup, "clock": "HIP events"}
    for k in ms:
        r[k] = {"ms_per_rollout": stat(ms[k]["rollout"]), "ms_per_update": stat(ms[k]["update"])}
        r[k]["env_steps_per_s"] = E * T / ((r[k]["ms_per_rollout"]["median"] + r[k]["ms_per_update"]["median"]) * 1e-3)
    for k in ms:
        if k != "gauss":
            r[k]["rollout_over_gauss"] = r[k]["ms_per_rollout"]["median"] / r["gauss"]["ms_per_rollout"]["median"]
            r[k]["update_over_gauss"] = r[k]["ms_per_update"]["median"] / r["gauss"]["ms_per_update"]["median"]
    return r


def measure_eval(E, runs, warmup):
    eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=3, n_assets=2, max_episode_steps=EVAL_STEPS)
    ns = nets(eng)
    r = {"envs": E, "steps": EVAL_STEPS, "rnn_length": R, "runs": runs, "warmup": warmup, "clock": "HIP events"}
    for k, n in ns.items():
        ev, ro = [], []
        n.set_greedy(True)
        for i in range(warmup + runs):
            eng.reset()
            t_ev = timed(eng, lambda: n._check(n._fn("eval")(n.n, EVAL_STEPS, 0)))
            eng.reset()
            t_ro = timed(eng, lambda: n.rollout(EVAL_STEPS))
            if i >= warmup:
                ev.append(t_ev); ro.append(t_ro)
        r[k] = {"ms_eval": stat(ev), "ms_greedy_rollout": stat(ro)}
        r[k]["eval_over_greedy_rollout"] = r[k]["ms_eval"]["median"] / r[k]["ms_greedy_rollout"]["median"]
        n.close()
    eng.close()
    return r


def scale_row(updates, E=4096, T=64, K=17, eval_envs=64, seed=3):
    eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=seed, n_assets=2, max_episode_steps=EVAL_STEPS)
    eng.reset()
    net = _ffi_gridtrade.GridTradeNet(eng, rnn_length=R, num_choices=K, max_samples=1)
    net.set_params(_ffi_gridtrade.default_init_gridtrade(seed, K))
    for _ in range(updates):
        net.rollout(T)
        net.train_rollout(1e-4)
    mon = GridTradeMonitor(n_envs=eval_envs, n_grid=K, max_seq_length=R)
    row = {"eval_envs": eval_envs, "num_choices": K, "updates": updates, "train_envs": E, "train_steps": T}
    row["best_rule"] = mon.rule_baseline()[2]
    row["tuned_rule"] = mon.search_baseline()[1]
    row["attainable_optimum"] = mon.trade_optimal()
    row["ceiling"] = mon.trade_ceiling()
    mon.eval_once(net.get_params())
    row["agent"] = mon.log["mean_total_reward"][-1]
    row["agent_share_of_attainable_gap"] = (row["agent"] - row["best_rule"]) / (row["attainable_optimum"] - row["best_rule"])
    mon.close(); net.close(); eng.close()
    return row


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, nargs="+", default=[4096, 8192])
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--eval-envs", type=int, default=8192)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--scale-updates", type=int, default=200)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "gridtrade_update_times.json"))
    a = p.parse_args()
    out = {"update": [], "eval": None, "scale": None}
    for E in a.envs:
        out["update"].append(measure_update(E, a.steps, a.runs, a.warmup))
        print(json.dumps(out["update"][-1]), flush=True)
    if a.eval_envs > 0:
        out["eval"] = measure_eval(a.eval_envs, a.runs, a.warmup)
        print(json.dumps(out["eval"]), flush=True)
    if a.scale_updates >= 0:
        out["scale"] = scale_row(a.scale_updates)
        print(json.dumps(out["scale"]), flush=True)
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
