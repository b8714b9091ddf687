"""The three A3C nets (gated Ticker trader; Gaussian agent on Solow and TradeAR1; discrete savings-grid agent on Solow, "grid") on
one fixed scenario, a SHA-256 per buffer: do two builds compute the same bits?

    python tools/a3c_bits.py [--baseline PARENT_CHECKOUT] [--json OUT]

70 envs (one full 64-sample group and a group of 6, so lanes past the last sample are exercised), rnn_length 5 (gated, Solow, grid
with 51 grid points) / 20 (TradeAR1), episodes capped at 5 steps so that dones -- the window restart and, for Solow, the terminal
value pass -- fall inside the rollouts: rollout(3) + train_rollout twice, then eval(max_steps=8, trace_steps=8).  Hashed: every
read_rollout buffer of the second rollout, the parameters, both RMSProp vectors and the six stats after the second update, every output of eval.  TradeAR1's
window of 20 rows never fills in 6 steps, so its two updates carry weight 0 throughout; therefore every net also takes one host
train(apply_update=False) on the 70 recorded samples of the last step with weights 1, 0, 1, 0, .. and both gradients are hashed.

--baseline names a built checkout of the commit to compare against; the scenario then runs from it too, in a fresh process of the
same job (this script, with --root), and every hash must be equal: the exit status says so."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ENVS, CAP, RNN, GRID_K = 70, 5, {"gated": 5, "solow": 5, "trade": 20, "grid": 5}, 51
KINDS = ("gated", "solow", "trade", "grid")
ROLLOUT = {"gated": ("states", "windows", "choices", "raw", "probs", "mu", "sigma", "values", "rewards", "dones", "weights", "adv", "targets",
                     "actions", "boot"),
           "solow": ("states", "windows", "raw", "mu", "sigma", "actions", "values", "rewards", "dones", "weights", "adv", "targets",
                     "term_values", "term_states", "term_windows", "boot"),
           "trade": ("states", "windows", "raw", "mu", "sigma", "actions", "values", "rewards", "dones", "weights", "adv", "targets",
                     "term_values", "boot"),
           "grid": ("states", "windows", "probs", "choices", "actions", "values", "rewards", "dones", "weights", "adv", "targets",
                    "term_values", "term_states", "term_windows", "boot")}
# what the net's train takes between windows and weights, and what its constructor takes besides rnn_length and max_samples
TRAIN = {"gated": ("choices", "raw", "adv", "targets"), "solow": ("raw", "adv", "targets"), "trade": ("raw", "adv", "targets"),
         "grid": ("choices", "adv", "targets")}
EXTRA = {"gated": {}, "solow": {"scale": 100.0}, "trade": {}, "grid": {"num_choices": GRID_K}}


def make(kind, root, seed=3):
    from goldsrl import _ffi, _ffi_discrete, _ffi_gated, _ffi_gauss
    if kind == "gated":
        eng = _ffi.Engine(_ffi.ENV_TICKER, ENVS, seed=seed, max_episode_steps=CAP)
        eng.ticker_set_table(np.load(os.path.join(root, "tests", "golden", "ticker.npz"))["matrix"])
        net = _ffi_gated.GatedNet(eng, rnn_length=RNN[kind], max_samples=1, **EXTRA[kind])
        net.set_params(_ffi_gated.default_init_gated(seed))
    elif kind == "solow":
        eng = _ffi.Engine(_ffi.ENV_SOLOW, ENVS, seed=seed, max_episode_steps=CAP)
        net = _ffi_gauss.GaussNet(eng, rnn_length=RNN[kind], max_samples=1, **EXTRA[kind])
        net.set_params(_ffi_gauss.default_init_gauss(seed, **_ffi_gauss.SOLOW_SIZES))
    elif kind == "grid":
        eng = _ffi.Engine(_ffi.ENV_SOLOW, ENVS, seed=seed, max_episode_steps=CAP)
        net = _ffi_discrete.DiscreteNet(eng, rnn_length=RNN[kind], max_samples=1, **EXTRA[kind])
        net.set_params(_ffi_discrete.default_init_discrete(seed, GRID_K))
    else:
        eng = _ffi.Engine(_ffi.ENV_TRADE, ENVS, seed=seed, n_assets=2, max_episode_steps=CAP)
        net = _ffi_gauss.GaussNet(eng, rnn_length=RNN[kind], max_samples=1, **EXTRA[kind])
        net.set_params(_ffi_gauss.default_init_gauss(seed, **_ffi_gauss.TRADE_SIZES))
    eng.reset()
    return eng, net


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def scenario(kind, root):
    eng, net = make(kind, root)
    out = {}
    for _ in range(2):
        net.rollout(3)
        stats = net.train_rollout(1e-3)
    for k in ROLLOUT[kind]:
        out["rollout." + k] = sha(net.read_rollout(k))
    out["dones_in_rollout"] = int(net.read_rollout("dones").sum())      # a figure, not a hash: the scenario reaches the restart
    out["weighted_steps"] = int(net.read_rollout("weights").sum())
    st = net.get_optimizer_state()
    params = net.get_params()
    out["params"], out["ms_policy"], out["ms_value"] = sha(params), sha(st["ms_policy"]), sha(st["ms_value"])
    out["stats"] = sha(np.array([stats[k] for k in sorted(stats)], np.float32))
    last = {k: net.read_rollout(k)[-1] for k in ("states", "windows") + TRAIN[kind]}
    net.close()
    net = type(net)(eng, rnn_length=RNN[kind], max_samples=ENVS, **EXTRA[kind])      # room for host samples
    net.set_params(params)
    net.train(last["states"], last["windows"], *[last[k] for k in TRAIN[kind]], weights=(np.arange(ENVS) % 2 == 0).astype(np.float32),
              apply_update=False)
    out["host_train.grad_policy"], out["host_train.grad_value"] = sha(net.get_grads("policy")), sha(net.get_grads("value"))
    out["host_train.grad_policy_absmax"] = float(np.abs(net.get_grads("policy")).max())      # a figure: the gradient is not zero
    eng.reset()
    for k, v in sorted(net.eval(8, trace_steps=8).items()):
        out["eval." + k] = sha(v)
    net.close(); eng.close()
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose library and package run")
    p.add_argument("--baseline", help="a built checkout of the commit to compare against")
    p.add_argument("--json", help="write the result here as well")
    a = p.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, os.path.join(root, "golds-rl-gym_amd"))
    out = {"envs": ENVS, "episode_cap": CAP, "rnn_length": RNN, "hashes": {k: scenario(k, root) for k in KINDS}}
    if a.baseline:
        tmp = (a.json or os.path.join(os.getcwd(), "a3c_bits.json")) + ".baseline"
        subprocess.run([sys.executable, os.path.abspath(__file__), "--root", a.baseline, "--json", tmp], check=True,
                       env={k: v for k, v in os.environ.items() if k != "PYTHONPATH"}, stdout=subprocess.DEVNULL)
        with open(tmp) as f:
            base = json.load(f)["hashes"]
        os.remove(tmp)
        out["differ"] = sorted(k + "." + b for k in base for b in base[k] if base[k][b] != out["hashes"][k].get(b))
        same_keys = sorted(base) == sorted(KINDS) and all(sorted(base[k]) == sorted(out["hashes"][k]) for k in base)
        out["equal_to_baseline"] = not out["differ"] and same_keys
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
    sys.exit(0 if out.get("equal_to_baseline", True) else 1)


if __name__ == "__main__":
    main()
