"""The three PAAC nets (conv on Swarm, flat GRU on Solow and TradeAR1, field net) on small fixed scenarios, a SHA-256 per buffer: do
two builds compute the same bits?

    python tools/paac_bits.py [--baseline PARENT_CHECKOUT] [--json OUT] [--conv-envs N --conv-chunk C]

conv     3 envs (30 samples, chunks of 20: one full and a ragged one) and 256 envs (one chunk of 2560 samples: the pixel-major
         branches of nenv % 256 == 0), in every configuration of CONV_CONFIGS: the create flags and the GRL_* knobs that choose a
         launch of the gradient step.  The knobs are read when the net is created and some are per-process statics, so each
         configuration runs in a fresh child process with its own environment, one after the other.
         --conv-envs N --conv-chunk C: one more run at that size, default configuration only.
solow    70 envs (one full 64-sample group and a ragged one), rnn 5.          Each of the two flat envs three times: as it is, with
trade    TradeAR1 with 2 assets, 70 envs.                                     set_keep_activations(True), and with a world-size-1
                                                                              communicator (comm_init + comm_broadcast_params) in front.
field    height = width = 8, 2 conv layers, 5 samples: train twice.
The conv and flat nets run rollout(2) + train_rollout twice, then rollout(2), train_rollout_grads -> get_grads -> set_grads ->
apply_grads.  Hashed: parameters, gradient, both Adam vectors, adam_step, the action counter, the four stats of every call and
every read_rollout buffer of the last rollout.  The flat net's loss, policy_loss and critic_loss_mean are sums of float64 atomics
in completion order over more than one workgroup here, so they are figures compared at rtol 1e-6; its
global_norm, like everything else, is fixed-order and hashed.

--baseline names a built checkout of the commit to compare against; the scenarios then run from it too, in a fresh process of the
same job (this script, with --root), and every hash must be equal: the exit status says so."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LOSSES = ("loss", "policy_loss", "critic_loss_mean")
FLAT = tuple((k, v) for k in ("solow", "trade") for v in ("", ".keep", ".comm"))
# name -> (GrlNetConfig.reserved flags, environment of the child process)
CONV_CONFIGS = {
    "default": (0, {}),
    "per_agent_trunk": (1, {}), "recompute_forward": (2, {}), "single_stream": (4, {}),
    "trunk_skip_off": (0, {"GRL_TRUNK_SKIP": "off"}),
    "expand2_lds": (0, {"GRL_NET_EXPAND2": "lds"}),
    "patch_skip_off": (0, {"GRL_PATCH_SKIP": "off"}),
    "obs_index_off": (0, {"GRL_OBS_INDEX": "off"}),
    "pwgrad_pair_off": (0, {"GRL_PATCH_WGRAD_PAIR": "off"}),
    "pwgrad_pair_off_xcd0": (0, {"GRL_PATCH_WGRAD_PAIR": "off", "GRL_PATCH_WGRAD_XCD": "0"}),
    "pwgrad_pair_off_xcd2": (0, {"GRL_PATCH_WGRAD_PAIR": "off", "GRL_PATCH_WGRAD_XCD": "2"}),
    "pwgrad_xcd0": (0, {"GRL_PATCH_WGRAD_XCD": "0"}),
    "pdgrad_pair_off": (0, {"GRL_PATCH_DGRAD_PAIR": "off"}),
    "pdgrad_pair_off_xcd0": (0, {"GRL_PATCH_DGRAD_PAIR": "off", "GRL_PATCH_DGRAD_XCD": "0"}),
    "swgrad_pair_off": (0, {"GRL_SLOT_WGRAD_PAIR": "off"}),
    "swgrad_chunks3": (0, {"GRL_SLOT_WGRAD_CHUNKS": "3"}),
    "tn_wgs256": (0, {"GRL_TN_WGS": "256"}),
    "tn_wgs_dense128": (0, {"GRL_TN_WGS_DENSE": "128"}),
}
CONV_SIZES = ((3, 20), (256, 2560))      # (envs, max_chunk_samples)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def put_stats(out, figures, tag, stats, exact):
    """global_norm by its bits; the three loss figures by their bits too (exact) or as figures"""
    out[tag + ".global_norm"] = sha(np.float32(stats["global_norm"]))
    for k in LOSSES:
        if exact:
            out[tag + "." + k] = sha(np.float32(stats[k]))
        else:
            figures[tag + "." + k] = stats[k]


def trainer(net, rollout, read, exact):
    """the sequence of the two nets that act: -> (hashes, figures)"""
    out, fig = {}, {}
    for i in range(2):
        rollout()
        put_stats(out, fig, "train_rollout%d" % i, net.train_rollout(1e-3), exact)
    rollout()
    put_stats(out, fig, "train_rollout_grads", net.train_rollout_grads(), exact)
    g = net.get_grads()
    net.set_grads(g)
    put_stats(out, fig, "apply_grads", net.apply_grads(1e-3), exact)
    st = net.get_optimizer_state()
    out["grads"], out["params"], out["adam_m"], out["adam_v"] = sha(g), sha(net.get_params()), sha(st["adam_m"]), sha(st["adam_v"])
    out["adam_step"], out["action_counter"] = st["adam_step"], net.get_action_counter()      # figures that must be equal
    out["grad_absmax"] = float(np.abs(g).max())                                             # the gradient is not zero
    for k, a in read():
        out["rollout." + k] = sha(a)
    return out, fig


def conv(E, chunk, flags):
    from goldsrl import _ffi, _ffi_net
    T = 2
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=1692)
    eng.reset()
    net = _ffi_net.ConvNet(eng, max_chunk_samples=chunk, reserved=flags)
    net.set_params(_ffi_net.glorot_uniform_flat(seed=3))
    B = E * 10
    shapes = {"actions": ((T, B, 2), np.float32), "values": ((T, B), np.float32), "rewards": ((T, B), np.float32), "y": ((T, B), np.float32),
              "adv": ((T, B), np.float32), "boot": ((B,), np.float32), "locust_bins": ((T, E, 160), np.uint8),
              "agent_bins": ((T, E, 20), np.uint8), "positions": ((T, E, 20), np.uint8), "dones": ((T, E), np.uint8)}

    def rollout():
        net.rollout(T, 0)
        eng.wait()
    res = trainer(net, rollout, lambda: [(k, net.read_rollout(k, s, d)) for k, (s, d) in shapes.items()], True)
    net.close(); eng.close()
    return res


def conv_configs(a):
    """every configuration at every size, a child process each: -> {"conv.<config>.<envs>x<chunk>": (hashes, figures)}"""
    runs = {}
    tmp = (a.json or os.path.join(os.getcwd(), "paac_bits.json")) + ".conv"
    for name, (_, env) in CONV_CONFIGS.items():
        print("conv configuration %s" % name, file=sys.stderr, flush=True)
        cmd = [sys.executable, os.path.abspath(__file__), "--root", a.root, "--conv-config", name, "--json", tmp]
        if name == "default" and a.conv_envs:
            cmd += ["--conv-envs", str(a.conv_envs), "--conv-chunk", str(a.conv_chunk)]
        subprocess.run(cmd, check=True, env=dict(os.environ, **env), stdout=subprocess.DEVNULL)
        with open(tmp) as f:
            runs.update({k: (v, {}) for k, v in json.load(f)["hashes"].items()})
        os.remove(tmp)
    return runs


def flat(kind, variant):
    from goldsrl import _ffi, _ffi_flat
    E, T = 70, 2
    if kind == "solow":
        eng = _ffi.Engine(_ffi.ENV_SOLOW, E, seed=1692)
        sizes = dict(static_size=2, temporal_size=2, num_actions=1)
    else:
        eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=1692, n_assets=2)
        sizes = dict(static_size=5, temporal_size=5, num_actions=2)
    eng.reset()
    net = _ffi_flat.FlatNet(eng, rnn_length=eng.cfg.rnn_length, max_samples=T * E, **sizes)
    net.set_params(_ffi_flat.default_init_flat(3, **sizes))
    if variant == ".keep":
        net.set_keep_activations(True)
    if variant == ".comm":
        net.comm_init(net.comm_unique_id(), 0, 1)
        net.comm_broadcast_params(0)
    A, S0, R = sizes["num_actions"], sizes["static_size"], net.cfg.rnn_length
    shapes = {"actions": (T, E, A), "values": (T, E), "rewards": (T, E), "masks": (T, E), "y": (T, E), "adv": (T, E), "boot": (E,),
              "states": (T, E, S0), "nhist": (T, E)}      # nhist: int32 words, read for their bits
    if kind == "solow":
        shapes["histories"] = (T, E, R, 2)      # the dense windows are recorded for Solow only
    out, fig = trainer(net, lambda: net.rollout(T), lambda: [(k, net.read_rollout(k, s)) for k, s in shapes.items()], False)
    if variant == ".comm":
        out["allreduce_calls"] = net.comm_info()["allreduce_calls"]      # train_rollout twice; apply_grads reduces nothing
        net.comm_destroy()
    net.close(); eng.close()
    return out, fig


def field():
    from goldsrl import _ffi, _ffi_field
    geom = dict(height=8, width=8, channels=3, filters=5, conv_layers=2, num_actions=3)
    eng = _ffi.Engine(_ffi.ENV_SOLOW, 4, seed=1)      # any handle: the net only needs its device and stream
    net = _ffi_field.FieldNet(eng, max_samples=5, **geom)
    net.set_params(_ffi_field.glorot_uniform_flat(3, **geom))
    rng = np.random.RandomState(5)
    N = 5
    states = rng.uniform(size=(N, 8, 8, 3)).astype(np.float32)
    pos = np.stack([rng.randint(0, 8, N), rng.randint(0, 8, N)], axis=1).astype(np.int32)
    act, adv, y = rng.normal(size=(N, 3)).astype(np.float32), rng.normal(size=N).astype(np.float32), rng.normal(size=N).astype(np.float32)
    out = {}
    for i in range(2):
        put_stats(out, None, "train%d" % i, net.train(states, pos, act, adv, y, 1e-3), True)
        out["train%d.grads" % i], out["train%d.params" % i] = sha(net.get_grads()), sha(net.get_params())
    for k, v in net.predict(states, pos).items():
        out["predict." + k] = sha(v)
    out["grad_absmax"] = float(np.abs(net.get_grads()).max())
    net.close(); eng.close()
    return out, {}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose library and package run")
    p.add_argument("--baseline", help="a built checkout of the commit to compare against")
    p.add_argument("--json", help="write the result here as well")
    p.add_argument("--conv-envs", type=int, default=0, help="one more conv run with this many envs (default configuration only)")
    p.add_argument("--conv-chunk", type=int, default=0, help="max_chunk_samples of that run")
    p.add_argument("--conv-config", help="(the child process of one configuration: the conv scenario alone, at every size)")
    a = p.parse_args()
    if bool(a.conv_envs) != bool(a.conv_chunk):
        p.error("--conv-envs and --conv-chunk go together")
    sys.path.insert(0, os.path.join(os.path.abspath(a.root), "golds-rl-gym_amd"))
    if a.conv_config:
        sizes = CONV_SIZES + (((a.conv_envs, a.conv_chunk),) if a.conv_envs else ())
        runs = {"conv.%s.%dx%d" % (a.conv_config, E, c): conv(E, c, CONV_CONFIGS[a.conv_config][0]) for E, c in sizes}
    else:
        runs = conv_configs(a)
        runs["field"] = field()
        for kind, variant in FLAT:
            runs[kind + variant] = flat(kind, variant)
    out = {"hashes": {k: v[0] for k, v in runs.items()}, "figures_rtol_1e-6": {k: v[1] for k, v in runs.items() if v[1]}}
    if a.baseline:
        tmp = (a.json or os.path.join(os.getcwd(), "paac_bits.json")) + ".baseline"
        extra = ["--conv-envs", str(a.conv_envs), "--conv-chunk", str(a.conv_chunk)] if a.conv_envs else []
        subprocess.run([sys.executable, os.path.abspath(__file__), "--root", a.baseline, "--json", tmp] + extra, check=True,
                       env={k: v for k, v in os.environ.items() if k != "PYTHONPATH"}, stdout=subprocess.DEVNULL)
        with open(tmp) as f:
            base = json.load(f)
        os.remove(tmp)
        bh, bf = base["hashes"], base["figures_rtol_1e-6"]
        out["differ"] = sorted(k + "." + b for k in bh for b in bh[k] if bh[k][b] != out["hashes"][k].get(b))
        out["differ"] += sorted(k + "." + b for k in bf for b in bf[k]
                                if not np.isclose(bf[k][b], out["figures_rtol_1e-6"][k].get(b, np.nan), rtol=1e-6, atol=0.0))
        out["equal_to_baseline"] = (not out["differ"] and all(sorted(bh[k]) == sorted(out["hashes"][k]) for k in bh)
                                    and sorted(bh) == sorted(out["hashes"]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
    sys.exit(0 if out.get("equal_to_baseline", True) else 1)


if __name__ == "__main__":
    main()
