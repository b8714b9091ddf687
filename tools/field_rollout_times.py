"""The field policy (ConvPolicyVFieldNetwork) acting and learning on Swarm on the device (include/goldsrl_fieldrollout.h), timed:

  G = 20, 2 conv layers, 5 filters, T = 20 at 64, 4 096 and 32 768 envs: rollout ms, update ms and env-steps/s with training
    * fused      one workgroup per env and step (the default),
    * layers     GRL_FIELD_FUSED=off: the forward layer by layer on E env-samples, the fused kernel's A/B partner,
    * row-major  GRL_FIELD_HEADT=off: the fused forward and the update reading head columns from the stored row-major mu_w / sigma_w
                 instead of the column-major copies (the A/B of those copies);
  the three variants are built side by side and timed in turn, run by run, so drift hits them alike.
  The comparator is the per-sample host path as it was before the device rollout, in the same run, at 64 envs, by the wall clock:
  per step read the observation, swarm_field_inputs, FieldNet.predict, sample on the host, Engine.step; per update FieldNet.train
  on the T*B host samples.  Larger sizes only with --host-envs (the serial weight gradients make it quadratic in practice).

    python tools/field_rollout_times.py [--envs 64 4096 32768] [--runs 5] [--warmup 1] [--host-envs 64] [--json OUT]

Device times by HIP events on the handle's stream, median and spread (min, max) of the runs after the warm-up.  The conv policy's
figures at the same env counts are copied from profiles/r05_* for context and labelled as not re-measured.
Default output: profiles/field_rollout_times.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "golds-rl-gym_amd"))
from goldsrl import _ffi, _ffi_field  # noqa: E402
from goldsrl.agents.state_processors import swarm_field_inputs  # noqa: E402

GEOM = dict(height=20, width=20, channels=2, filters=5, conv_layers=2, num_actions=2)
T, LR, SCALE = 20, 1e-4, 1000.0
VARIANTS = (("fused", {}), ("layers", {"GRL_FIELD_FUSED": "off"}), ("row_major_heads", {"GRL_FIELD_HEADT": "off"}))
# profiles/r05_shard_probe_4096.txt (chunk = 0, rep 1) and profiles/r05_bench_n1.json: one T = 20 update, rollout + gradient step
CONV_CONTEXT = {"source": "profiles/r05_shard_probe_4096.txt, profiles/r05_bench_n1.json", "re_measured": False,
                "what": "conv policy, ms per T = 20 update (rollout + gradient step together; the files do not split them)",
                "ms_per_update": {"64": None, "4096": 48.38, "32768": 302.24}}


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def params():
    flat = _ffi_field.glorot_uniform_flat(3, **GEOM)
    shapes = _ffi_field.field_param_shapes(**GEOM)
    rng, parts, at = np.random.RandomState(1), [], 0
    for name, shape in shapes:      # small non-zero biases: no dead units at the start
        n = int(np.prod(shape))
        parts.append(rng.normal(size=n).astype(np.float32) * 0.05 if name.endswith("_b") else flat[at:at + n])
        at += n
    return np.concatenate(parts)


def build(E, env):
    for k in ("GRL_FIELD_FUSED", "GRL_FIELD_HEADT"):
        os.environ.pop(k, None)
    os.environ.update(env)
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=1692, grid_size=GEOM["height"], max_episode_steps=128)
    eng.reset()
    net = _ffi_field.FieldNet(eng, max_samples=min(E, 8192), scale=SCALE, entropy_beta=0.02, clip_norm=40.0, **GEOM)
    net.set_params(params())
    net.rollout_bind(0.99)
    net.predict_swarm()      # the switches are read here
    return eng, net


def timed(eng, fn):
    eng.timer_start()
    fn()
    eng.timer_stop()
    return eng.timer_ms()


def device(E, runs, warmup):
    built = [(name, build(E, env)) for name, env in VARIANTS]
    ms = {name: {"rollout": [], "update": []} for name, _ in VARIANTS}
    for i in range(warmup + runs):
        for name, (eng, net) in built:
            ro = timed(eng, lambda: (net.rollout(T, 0), eng.wait()))
            up = timed(eng, lambda: net.train_rollout(LR))
            if i >= warmup:
                ms[name]["rollout"].append(ro); ms[name]["update"].append(up)
    out = {"envs": E, "T": T, "runs": runs, "warmup": warmup, "clock": "HIP events", "variants": {}}
    for name, (eng, net) in built:
        ro, up = np.array(ms[name]["rollout"]), np.array(ms[name]["update"])
        out["variants"][name] = {"rollout_ms": stat(ro), "update_ms": stat(up),
                                 "env_steps_per_s_with_training": float(E * T / (np.median(ro + up) * 1e-3))}
        net.close(); eng.close()
    f = out["variants"]
    out["fused_over_layers_rollout"] = f["fused"]["rollout_ms"]["median"] / f["layers"]["rollout_ms"]["median"]
    out["column_major_over_row_major_rollout"] = f["fused"]["rollout_ms"]["median"] / f["row_major_heads"]["rollout_ms"]["median"]
    out["column_major_over_row_major_update"] = f["fused"]["update_ms"]["median"] / f["row_major_heads"]["update_ms"]["median"]
    return out


def host_path(E, runs, warmup, budget_s=60.0):
    """the per-sample host path: FieldNet.predict per step and FieldNet.train per update on host arrays"""
    for k in ("GRL_FIELD_FUSED", "GRL_FIELD_HEADT"):
        os.environ.pop(k, None)
    G, B = GEOM["height"], E * 10
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=1692, grid_size=G, max_episode_steps=128)
    eng.reset()
    net = _ffi_field.FieldNet(eng, max_samples=T * B, scale=SCALE, entropy_beta=0.02, clip_norm=40.0, **GEOM)
    net.set_params(params())
    rng = np.random.RandomState(0)
    ro_s, up_s = [], []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        S, P, A, V, R = [], [], [], [], []
        for _ in range(T):
            states, pos = swarm_field_inputs(eng.read("locust_bins"), eng.read("agent_bins"), eng.read("positions"), G)
            states, pos = np.repeat(states, 10, axis=0), pos.reshape(-1, 2)
            out = net.predict(states, pos)
            act = (out["mu"] + out["sigma"] * rng.normal(size=out["mu"].shape)).astype(np.float32)
            eng.step(eng.transform_actions(act.reshape(E, 10, 2)))
            S.append(states); P.append(pos); A.append(act); V.append(out["vs"]); R.append(np.repeat(eng.read("reward"), 10))
        states, pos = swarm_field_inputs(eng.read("locust_bins"), eng.read("agent_bins"), eng.read("positions"), G)
        boot = net.predict(np.repeat(states, 10, axis=0), pos.reshape(-1, 2))["vs"]
        y, adv = eng.returns(np.array(R), np.array(V), boot, 0.99, scale=SCALE)
        t1 = time.perf_counter()
        net.train(np.concatenate(S), np.concatenate(P), np.concatenate(A), adv.reshape(-1), y.reshape(-1), LR)
        t2 = time.perf_counter()
        if i >= warmup:
            ro_s.append((t1 - t0) * 1e3); up_s.append((t2 - t1) * 1e3)
        if t2 - t0 > budget_s:
            break
    net.close(); eng.close()
    if not ro_s:
        return {"envs": E, "T": T, "clock": "wall", "note": "the warm-up run alone took more than %.0f s: not measured" % budget_s}
    ro, up = np.array(ro_s), np.array(up_s)
    return {"envs": E, "T": T, "runs": len(ro_s), "warmup": warmup, "clock": "wall", "rollout_ms": stat(ro), "update_ms": stat(up),
            "env_steps_per_s_with_training": float(E * T / (np.median(ro + up) * 1e-3))}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--envs", type=int, nargs="+", default=[64, 4096, 32768])
    p.add_argument("--host-envs", type=int, nargs="*", default=[64], dest="host_envs")
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--json", default=os.path.join(ROOT, "profiles", "field_rollout_times.json"))
    a = p.parse_args()
    out = {"geometry": GEOM, "device": [], "host_path": [], "conv_policy_context": CONV_CONTEXT}
    for E in a.envs:
        out["device"].append(device(E, a.runs, a.warmup))
        print(json.dumps(out["device"][-1]), flush=True)
    for E in a.host_envs:
        out["host_path"].append(host_path(E, a.runs, a.warmup))
        print(json.dumps(out["host_path"][-1]), flush=True)
        dev = [d for d in out["device"] if d["envs"] == E]
        if dev and "env_steps_per_s_with_training" in out["host_path"][-1]:
            out["host_path"][-1]["device_fused_over_host_path_env_steps_per_s"] = (
                dev[0]["variants"]["fused"]["env_steps_per_s_with_training"] / out["host_path"][-1]["env_steps_per_s_with_training"])
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
