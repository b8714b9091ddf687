"""Evaluation of the flat PAAC policy (include/goldsrl_flateval.h): ms per 1 024-step evaluation of E envs by
  (a) eval              grl_fnet_eval, one launch for the whole episode (and eval_traced: with the full trace)
  (b) rollouts          51 x rollout(20) + rollout(4) = 1 024 steps of the persistent rollout, on the baseline checkout
  (c) host_monitor      wall clock of the baseline's host-driven SolowPolicyMonitor.eval_once (Solow, one env)
for Solow (cap 1 024, R = 5) and TradeAR1 with 16 assets (cap 1 024, R = 20), and ms per rollout(20) -- the training path -- on both
checkouts at every env count.  (a), (b) and rollout(20) by HIP events on the handle's stream, median and spread (min, max) of the
runs after the warm-up; every run starts from a reset handle.  The bracket of (a) includes the full reset of the handle that
grl_fnet_eval ends with (iota, a 4-byte copy and the reset kernel, for Solow with the tape draw); (b)'s rollouts end without one, so
the ratio (a) / (b) is biased against the evaluation by that reset.

    python tools/flat_eval_times.py [--envs 64 4096 8192] [--runs 5] [--warmup 1] [--baseline PARENT_CHECKOUT] [--json OUT]

--baseline names a built checkout of the commit to compare against; (b), (c) and its rollout(20) then run from it in a fresh
process of the same job (this script, with --root), and the ratios are added:
  eval_over_baseline_rollouts   (a) / (b), and within_spread: (a) - (b) <= max(b) - min(b)
  rollout20_over_baseline       this checkout's rollout(20) / the baseline's, and within_spread likewise
Without --baseline (b) and (c) are measured on this checkout."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS, T = 1024, 20
RNN = {"solow": 5, "trade": 20}
N_ASSETS = 16


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def make(kind, E, seed=3):
    from goldsrl import _ffi, _ffi_flat
    if kind == "solow":
        eng = _ffi.Engine(_ffi.ENV_SOLOW, E, seed=seed, rnn_length=RNN[kind], max_episode_steps=STEPS)
        sizes = dict(static_size=2, temporal_size=2, num_actions=1)
    else:
        eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=seed, n_assets=N_ASSETS, rnn_length=RNN[kind], max_episode_steps=STEPS)
        sizes = dict(static_size=1 + 2 * N_ASSETS, temporal_size=1 + 2 * N_ASSETS, num_actions=N_ASSETS)
    net = _ffi_flat.FlatNet(eng, rnn_length=RNN[kind], scale=100.0, max_samples=T * E, **sizes)
    net.set_params(_ffi_flat.default_init_flat(seed, **sizes))
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


def rollouts(net):
    for _ in range(STEPS // T):
        net.rollout(T)
    if STEPS % T:
        net.rollout(STEPS % T)


def measure(kind, E, runs, warmup, has_eval, with_rollouts):
    eng, net = make(kind, E)
    r = {"env": kind, "envs": E, "steps": STEPS, "rnn_length": RNN[kind], "runs": runs, "warmup": warmup, "clock": "HIP events"}
    if has_eval:
        r["ms_eval"] = timed(eng, lambda: net.lib.grl_fnet_eval(net.n, STEPS, 0, 0), runs, warmup)
        r["ms_eval_greedy"] = timed(eng, lambda: net.lib.grl_fnet_eval(net.n, STEPS, 0, 1), runs, warmup)
        r["ms_eval_traced"] = timed(eng, lambda: net.lib.grl_fnet_eval(net.n, STEPS, STEPS, 0), runs, warmup)
        eng.reset()
        ev = net.eval(STEPS)
        r["episode_length"] = {"min": int(ev["length"].min()), "max": int(ev["length"].max()), "mean": float(ev["length"].mean())}
    if with_rollouts:
        r["ms_rollouts"] = timed(eng, lambda: rollouts(net), runs, warmup)
    r["ms_rollout20"] = timed(eng, lambda: net.rollout(T), 4 * runs, warmup)
    net.close(); eng.close()
    return r


def host_monitor(runs, warmup):
    from goldsrl import _ffi
    from goldsrl.agents.paac import policy_monitor as PM
    from goldsrl.agents.paac.policy_v_network import FlatPolicyVNetwork
    from goldsrl.agents.state_processors import SolowStateProcessor
    from goldsrl.envs.fed_env import SolowEnv
    conf = dict(name='local_learning', num_actions=1, clip_norm=40.0, clip_norm_type='global', device='/gpu:0', scale=100.0,
                static_size=2, temporal_size=2, entropy_regularisation_strength=0.02, static_hidden_size=32, rnn_hidden_size=32)
    eng = _ffi.Engine(_ffi.ENV_SOLOW, 64, seed=3, max_episode_steps=STEPS)
    eng.reset()
    global_net = FlatPolicyVNetwork(conf).bind(eng, max_samples=64)
    env = SolowEnv(p=1, q=1, T=STEPS, seed=1692, max_episode_steps=STEPS)
    mon = PM.SolowPolicyMonitor(env, global_net, SolowStateProcessor(), None, network_conf=conf)
    ms = []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        _, length = mon.eval_once()[:2]
        dt = (time.perf_counter() - t0) * 1e3
        assert length == STEPS
        if i >= warmup:
            ms.append(dt)
    return {"env": "solow", "envs": 1, "steps": STEPS, "runs": runs, "warmup": warmup, "clock": "wall", "ms_host_monitor": stat(ms)}


def spread(s):
    return s["max"] - s["min"]


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, nargs="+", default=[64, 4096, 8192])
    p.add_argument("--kinds", nargs="+", default=["solow", "trade"], choices=["solow", "trade"])
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose library and package are measured")
    p.add_argument("--baseline", help="a built checkout of the commit to compare against: (b) and (c) run from it")
    p.add_argument("--json", help="write the results here as well")
    a = p.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.root), "golds-rl-gym_amd"))
    from goldsrl import _ffi_flat
    has_eval = hasattr(_ffi_flat.FlatNet, "eval")
    alone = not a.baseline
    out = {"cases": [], "host_monitor": None}
    for kind in a.kinds:
        for E in a.envs:
            r = measure(kind, E, a.runs, a.warmup, has_eval, alone)
            out["cases"].append(r)
            print(json.dumps(r), flush=True)
    if alone:
        out["host_monitor"] = host_monitor(a.runs, a.warmup)
        print(json.dumps(out["host_monitor"]), flush=True)
    else:
        tmp = (a.json or os.path.join(os.getcwd(), "flat_eval_times.json")) + ".baseline"
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
            r["ms_rollouts_baseline"] = b["ms_rollouts"]
            r["ms_rollout20_baseline"] = b["ms_rollout20"]
            r["eval_over_baseline_rollouts"] = r["ms_eval"]["median"] / b["ms_rollouts"]["median"]
            r["eval_within_spread"] = bool(r["ms_eval"]["median"] - b["ms_rollouts"]["median"] <= spread(b["ms_rollouts"]))
            r["rollout20_over_baseline"] = r["ms_rollout20"]["median"] / b["ms_rollout20"]["median"]
            r["rollout20_within_spread"] = bool(r["ms_rollout20"]["median"] - b["ms_rollout20"]["median"] <= spread(b["ms_rollout20"]))
            if r["env"] == "solow":      # one host-driven episode against E episodes on the device
                r["host_monitor_over_eval"] = host / r["ms_eval"]["median"]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
