"""The eight whole-episode baseline launches on small fixed scenarios, a SHA-256 per output buffer: do two builds compute the same
bits?  And, with --calls, does a call cost the host the same?

    python tools/baseline_bits.py [--baseline PARENT_CHECKOUT] [--json OUT]
    python tools/baseline_bits.py --calls --baseline PARENT_CHECKOUT [--json OUT]

Every scenario runs twice on one handle -- a larger call, then a smaller one in the grown buffers --, each time with a traced env,
and every output the binding reads is hashed.  The sizes leave a ragged last wave or workgroup, and a TimeLimit below max_steps (or
a script that runs out) ends pairs early.

solow_sweep       70 envs, 5 rates x 40 steps then 3 x 17, TimeLimit 24 from 3 steps in; GRL_SWEEP_RPL 1 and 2.
trade_sweep       70 envs, 2 and 17 assets (the register and the LDS form), 5 rules x 40 steps then 3 x 17, GRL_TRADE_SWEEP_RPL 1 and
                  2, the engine's own normals and a tape.
trade_foresight   70 envs, 2 and 17 assets, horizons (0, 1, 16) x 40 steps then (4, 0) x 9, TimeLimit 24 from 3 steps in, the engine's
                  own normals and a tape.
ticker_sweep      70 envs on the table of tests/golden/ticker_rules.npz, 5 rules x 40 steps then 3 x 9, TimeLimit 30.
ticker_foresight  the same engine, horizons (0, 1, 16) x 40 steps then (4, 0) x 9.
solow_dp          70 envs, the tests' small grid, 4 stages: policy and value, then play 30 steps with trace_steps 30, then 12 with 5.
swarm_replay      6 envs, 3 scripts x 12 steps of lengths (12, 7, 3) then 2 x 5, TimeLimit 10; float64 and float32 rows.
swarm_rules       6 envs, 3 rules x 12 steps then 2 x 5, keep_actions.

--baseline names a built checkout of the commit to compare against; the scenarios then run from it too, in a fresh process of the
same job (this script, with --root), and every hash must be equal: the exit status says so.

--calls times the host path instead, where it is the whole cost: launch plus one read of `length` through the C ABI at 1 env, 1
rate / rule / horizon / script and 1 step, 2 000 calls after 200 of warm-up, microseconds per call.  The baseline and this build
run alternately, five fresh processes each; the baseline's own min..max is the run-to-run spread this build's median is held to."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden")
ROUNDS, CALLS, WARMUP = 5, 2000, 200


def hashes(out):
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(out.items()) if isinstance(v, np.ndarray)}


def twice(play):
    """play(larger) then play(smaller) on the caller's handle -> {call.output: sha}"""
    return {"%s.%s" % (tag, k): v for tag, big in (("larger", True), ("smaller", False)) for k, v in hashes(play(big)).items()}


def stepped(eng, actions):
    eng.reset()
    for _ in range(3):
        eng.step(actions)
    return eng


def solow_sweep(_ffi):
    from goldsrl._ffi_sweep import solow_sweep as sweep
    out = {}
    for rpl in ("1", "2"):
        os.environ["GRL_SWEEP_RPL"] = rpl
        eng = stepped(_ffi.Engine(_ffi.ENV_SOLOW, 70, seed=7, solow_p=2, solow_q=2, solow_tape_len=64, max_episode_steps=24),
                      np.full((70, 1), 0.3, np.float32))
        out["rpl" + rpl] = twice(lambda big: sweep(eng, np.linspace(0.1, 0.9, 5)[:5 if big else 3], 40 if big else 17, 69 if big else 3))
        eng.close()
    del os.environ["GRL_SWEEP_RPL"]
    return out


def trade_sweep(_ffi):
    from goldsrl._ffi_tradesweep import trade_sweep as sweep
    rules = np.array([(0, 0), (2, 0), (20, 0), (0, 1), (5, 0.5)], np.float32)
    out = {}
    for n in (2, 17):
        for rpl in ("1", "2"):
            os.environ["GRL_TRADE_SWEEP_RPL"] = rpl
            eng = stepped(_ffi.Engine(_ffi.ENV_TRADE, 70, seed=7, n_assets=n, max_episode_steps=24), np.full((70, n), 0.2, np.float32))
            for tape in (False, True):
                def play(big):
                    steps = 40 if big else 17
                    normals = np.random.RandomState(steps).normal(size=(steps, 70, n)).astype(np.float32) if tape else None
                    return sweep(eng, rules[:5 if big else 3], steps, 69 if big else 3, normals)
                out["n%d.rpl%s.%s" % (n, rpl, "tape" if tape else "own")] = twice(play)
            eng.close()
    del os.environ["GRL_TRADE_SWEEP_RPL"]
    return out


def trade_foresight(_ffi):
    from goldsrl._ffi_tradeforesight import trade_foresight as play
    out = {}
    for n in (2, 17):
        eng = stepped(_ffi.Engine(_ffi.ENV_TRADE, 70, seed=7, n_assets=n, max_episode_steps=24), np.full((70, n), 0.2, np.float32))
        for tape in (False, True):
            def run(big):
                steps = 40 if big else 9
                normals = np.random.RandomState(steps).normal(size=(steps, 70, n)).astype(np.float32) if tape else None
                return play(eng, (0, 1, 16) if big else (4, 0), steps, 69 if big else 3, normals)
            out["n%d.%s" % (n, "tape" if tape else "own")] = twice(run)
        eng.close()
    return out


def ticker_engine(_ffi, E, cap):
    matrix = np.load(os.path.join(GOLDEN, "ticker_rules.npz"))["matrix"]
    starts = np.random.RandomState(5).randint(0, matrix.shape[0] - 1024 + 1, size=E)
    starts[0] = matrix.shape[0] - 1024
    eng = _ffi.Engine(_ffi.ENV_TICKER, E, seed=0, max_episode_steps=cap, flags=_ffi.F_RESET_FROM_SNAPSHOT)
    eng.ticker_set_table(matrix)
    eng.set_state("TICKER_START0", starts.astype(np.int32))
    return stepped(eng, np.tile(np.array([1, 2, 0.5, 0.25], np.float32), (E, 1)))


def ticker_sweep(_ffi):
    from goldsrl._ffi_tickersweep import ticker_sweep as sweep
    rules = np.array([(0, 0, 0, 0, 1, 0), (0.5, 0.5, 0.5, 0.5, 0, 0), (1, 0, 0, 1, 0.5, 2), (1, 0, 0, 0, 0.5, 8), (0.3, 0.6, 0.6, 0.3, 0.02, 5)],
                     np.float32)
    eng = ticker_engine(_ffi, 70, 30)
    out = twice(lambda big: sweep(eng, rules[:5 if big else 3], 40 if big else 9, 69 if big else 3))
    eng.close()
    return out


def ticker_foresight(_ffi):
    from goldsrl._ffi_tickerforesight import ticker_foresight as play
    eng = ticker_engine(_ffi, 70, 30)
    out = twice(lambda big: play(eng, (0, 1, 16) if big else (4, 0), 40 if big else 9, 69 if big else 3))
    eng.close()
    return out


def solow_dp(_ffi):
    from goldsrl._ffi_solowdp import solow_dp_grid, solow_dp_play, solow_dp_solve
    eng = stepped(_ffi.Engine(_ffi.ENV_SOLOW, 70, seed=7, solow_p=1, solow_q=1, solow_tape_len=64, max_episode_steps=24),
                  np.full((70, 1), 0.3, np.float32))
    grid = solow_dp_grid(nk=7, nz=5, nq=3, ns=8, k_lo=30.0, k_hi=120.0, z_max=0.4, sigma=0.1)
    out = {"solve." + k: v for k, v in hashes(solow_dp_solve(eng, grid, 4)).items()}
    out.update(twice(lambda big: solow_dp_play(eng, 30 if big else 12, 30 if big else 5)))
    eng.close()
    return out


def swarm_replay(_ffi):
    from goldsrl._ffi_replay import swarm_replay as replay
    out = {}
    for dt in (np.float64, np.float32):
        eng = _ffi.Engine(_ffi.ENV_SWARM, 6, seed=7, max_episode_steps=10)
        eng.reset()
        acts = np.random.RandomState(3).uniform(-0.7, 0.7, size=(3, 12, 10, 2)).astype(dt)
        out[np.dtype(dt).name] = twice(lambda big: replay(eng, acts if big else acts[:2, :5], (12, 7, 3) if big else (5, 2), 5 if big else 0))
        eng.close()
    return out


def swarm_rules(_ffi):
    from goldsrl._ffi_swarmrules import swarm_rules as play
    rules = np.array([(0, 0, 0, 0, 0, 0), (1, 5, 0, -0.5, 0.5, 0.7), (1, 5, 1, 0.3, -0.3, 0)], np.float64)
    eng = _ffi.Engine(_ffi.ENV_SWARM, 6, seed=7, max_episode_steps=10)
    eng.reset()
    out = twice(lambda big: play(eng, rules[:3 if big else 2], 12 if big else 5, True, 5 if big else 0))
    eng.close()
    return out


SCENARIOS = (solow_sweep, trade_sweep, trade_foresight, ticker_sweep, ticker_foresight, solow_dp, swarm_replay, swarm_rules)


def flat(d, prefix=""):
    out = {}
    for k, v in d.items():
        out.update(flat(v, prefix + k + ".") if isinstance(v, dict) else {prefix + k: v})
    return out


def call_times(_ffi):
    """microseconds per call (launch + read of length) of each launch at 1 env, 1 item, 1 step"""
    from goldsrl import (_ffi_replay, _ffi_solowdp, _ffi_swarmrules, _ffi_sweep, _ffi_tickerforesight, _ffi_tickersweep, _ffi_tradeforesight,
                         _ffi_tradesweep)
    sigs = {}
    for m, name in ((_ffi_sweep, "SWEEP"), (_ffi_tradesweep, "TRADE_SWEEP"), (_ffi_tradeforesight, "TRADE_FORESIGHT"), (_ffi_tickersweep, "TICKER_SWEEP"),
                    (_ffi_tickerforesight, "TICKER_FORESIGHT"), (_ffi_solowdp, "SOLOW_DP"), (_ffi_replay, "REPLAY"), (_ffi_swarmrules, "SWARMRULES")):
        sigs.update(getattr(m, name + "_SIGNATURES"))
    lib = _ffi.load_library(extra_signatures=sigs)
    length = np.zeros(1, np.int32)
    f32, f64, i32 = (np.zeros(64, t) for t in (np.float32, np.float64, np.int32))
    f32[0] = 0.5
    p = _ffi._ptr
    solow = _ffi.Engine(_ffi.ENV_SOLOW, 1, seed=7, solow_p=1, solow_q=1, max_episode_steps=24)
    trade = _ffi.Engine(_ffi.ENV_TRADE, 1, seed=7, n_assets=2, max_episode_steps=24)
    ticker = ticker_engine(_ffi, 1, 30)
    swarm = _ffi.Engine(_ffi.ENV_SWARM, 1, seed=7, max_episode_steps=10)
    for e in (solow, trade, swarm):
        e.reset()
    _ffi_solowdp.solow_dp_solve(solow, _ffi_solowdp.solow_dp_grid(nk=7, nz=5, nq=3, ns=8, k_lo=30.0, k_hi=120.0, z_max=0.4, sigma=0.1), 4, read=False)
    launches = {
        "solow_sweep": (solow, lambda h: lib.grl_solow_sweep(h, p(f32), 1, 1, -1), lib.grl_solow_sweep_read),
        "trade_sweep": (trade, lambda h: lib.grl_trade_sweep(h, p(f32), p(f32), 1, None, 1, -1), lib.grl_trade_sweep_read),
        "trade_foresight": (trade, lambda h: lib.grl_trade_foresight(h, p(i32), 1, None, 1, -1), lib.grl_trade_foresight_read),
        "ticker_sweep": (ticker, lambda h: lib.grl_ticker_sweep(h, p(f32), 1, 1, -1), lib.grl_ticker_sweep_read),
        "ticker_foresight": (ticker, lambda h: lib.grl_ticker_foresight(h, p(i32), 1, 1, -1), lib.grl_ticker_foresight_read),
        "solow_dp_play": (solow, lambda h: lib.grl_solow_dp_play(h, 1, 0), lib.grl_solow_dp_play_read),
        "swarm_replay": (swarm, lambda h: lib.grl_swarm_replay(h, p(f64), 1, 1, 1, None, 0, -1), lib.grl_swarm_replay_read),
        "swarm_rules": (swarm, lambda h: lib.grl_swarm_rules(h, p(f64), p(f64), 1, 1, 0, -1), lib.grl_swarm_rules_read),
    }
    out = {}
    for name, (eng, launch, read) in launches.items():
        for i in range(WARMUP + CALLS):
            if i == WARMUP:
                t0 = time.perf_counter()
            eng._check(launch(eng.h))
            eng._check(read(eng.h, b"length", p(length), 4))
        out[name] = (time.perf_counter() - t0) / CALLS * 1e6
        assert length[0] == 1, (name, length)
    for e in (solow, trade, ticker, swarm):
        e.close()
    return out


def child(root, mode, tmp):
    subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--json", tmp] + mode, check=True,
                   env={k: v for k, v in os.environ.items() if k != "PYTHONPATH"}, stdout=subprocess.DEVNULL)
    with open(tmp) as f:
        res = json.load(f)
    os.remove(tmp)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose library and package run")
    ap.add_argument("--baseline", help="a built checkout of the commit to compare against")
    ap.add_argument("--calls", action="store_true", help="time the host path of a call instead of hashing outputs")
    ap.add_argument("--json", help="write the result here as well")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    tmp = (a.json or os.path.join(os.getcwd(), "baseline_bits.json")) + ".child"
    ok = True
    if a.calls and a.baseline:
        rounds = {"baseline": [], "this": []}
        for _ in range(ROUNDS):
            rounds["baseline"].append(child(a.baseline, ["--calls"], tmp))
            rounds["this"].append(child(root, ["--calls"], tmp))
        out = {"unit": "microseconds per call: launch + read of length, 1 env x 1 item x 1 step, %d calls after %d" % (CALLS, WARMUP), "launches": {}}
        for name in rounds["this"][0]:
            base, this = ([r[name] for r in rounds[k]] for k in ("baseline", "this"))
            med = float(np.median(this))
            out["launches"][name] = {"baseline_rounds": base, "this_rounds": this, "baseline_min": min(base), "baseline_max": max(base),
                                     "baseline_median": float(np.median(base)), "this_median": med, "inside_baseline_spread": min(base) <= med <= max(base)}
    else:
        sys.path.insert(0, os.path.join(root, "golds-rl-gym_amd"))
        from goldsrl import _ffi
        if a.calls:
            out = call_times(_ffi)
        else:
            out = {"hashes": {f.__name__: flat(f(_ffi)) for f in SCENARIOS}}
            if a.baseline:
                bh = child(a.baseline, [], tmp)["hashes"]
                out["differ"] = sorted(k + "." + b for k in bh for b in bh[k] if bh[k][b] != out["hashes"].get(k, {}).get(b))
                ok = out["equal_to_baseline"] = not out["differ"] and {k: sorted(v) for k, v in bh.items()} == {k: sorted(v) for k, v in out["hashes"].items()}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
