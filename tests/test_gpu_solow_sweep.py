"""GPU: the constant-savings baseline sweep of the Solow env (grl_solow_sweep / grl_solow_sweep_read of include/goldsrl_sweep.h;
csrc/solow_sweep.hip), the baseline class, the monitors' baseline() and the --baseline flag.

The yardstick of the one-launch sweep is the per-step path: grl_step with a constant action runs the same float32 operations in
the same order, so a pair's rewards -- and their sequential float64 sums -- must be the per-step path's bits.  The per-step twin
of a case is played once and shared by every sweep of that case.  The reference pins the values through
tests/golden/constant_solow.npz (the unmodified scripts/constant_solow.py)."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATES7 = np.array([0.0, 0.999, 0.05, 0.33, 0.5, 0.95, 0.2], np.float32)      # 0.0: the 1e-3 clamp
PAIR_KEYS = ("total", "sum_sq", "min", "max", "length", "finished")
STATE_FIELDS = ("SOLOW_K", "SOLOW_Z", "SOLOW_E", "SOLOW_TAPE", "SOLOW_TAPE_POS", "ELAPSED", "EPISODE", "NHIST")
OUTPUTS = ("reward", "done", "elapsed", "obs", "obs_raw", "history")


def _snapshot_engine(E, p=1, q=1, tape=64, cap=0, ss=False, seed=0):
    """A Solow engine whose reset restores injected random z0 and leaves the injected tape alone."""
    from goldsrl import _ffi
    flags = _ffi.F_RESET_FROM_SNAPSHOT | (_ffi.F_SOLOW_SS_RESET if ss else 0)
    eng = _ffi.Engine(_ffi.ENV_SOLOW, E, solow_p=p, solow_q=q, solow_tape_len=tape, max_episode_steps=cap, flags=flags)
    rng = np.random.RandomState(seed)
    eng.set_state("SOLOW_Z0", rng.normal(scale=0.1, size=(E, p)).astype(np.float32))
    eng.set_state("SOLOW_TAPE", rng.normal(scale=0.1, size=(E, tape)).astype(np.float32))
    eng.reset()
    return eng


def _play(eng, rate, n, restore=None, k_of=None):
    """The per-step path: n calls of step(full(E, rate)) from a reset (or restored) engine.  Returns rewards (n,E) float32, the
    length up to each env's first done (n where none), finished, and with k_of SOLOW_K of that env after every step."""
    E = eng.E
    if restore is None:
        eng.reset()
    else:
        for f, v in restore.items():
            eng.set_state(f, v)
    rewards, dones, ks = np.zeros((n, E), np.float32), np.zeros((n, E), bool), []
    for t in range(n):
        eng.step(np.full((E, 1), rate, np.float32))
        rewards[t], dones[t] = eng.read("reward"), eng.read("done") > 0
        if k_of is not None:
            ks.append(eng.get_state("SOLOW_K")[k_of])
    finished = dones.any(axis=0)
    length = np.where(finished, dones.argmax(axis=0) + 1, n).astype(np.int32)
    return rewards, length, finished.astype(np.uint8), np.array(ks, np.float32)


def _twin_stats(rewards, length, finished, max_steps):
    """What the sweep keeps, from the per-step rewards (n,E): sequential float64 sums (np.cumsum adds in order), float32 min / max."""
    n = np.minimum(length, max_steps)
    r64 = rewards.astype(np.float64)
    c1, c2 = np.cumsum(r64, axis=0), np.cumsum(r64 * r64, axis=0)
    env = np.arange(rewards.shape[1])
    live = np.arange(rewards.shape[0])[:, None] < n[None]
    return {"total": c1[n - 1, env], "sum_sq": c2[n - 1, env],
            "min": np.where(live, rewards, np.inf).min(axis=0).astype(np.float32),
            "max": np.where(live, rewards, -np.inf).max(axis=0).astype(np.float32),
            "length": n.astype(np.int32), "finished": (finished.astype(bool) & (length <= max_steps)).astype(np.uint8)}


def _assert_bits(got, want, r, msg):
    for k in PAIR_KEYS:
        assert got[k][r].dtype == want[k].dtype, (k, got[k].dtype, want[k].dtype)
        assert got[k][r].tobytes() == want[k].tobytes(), "%s: %s of rate %d differs" % (msg, k, r)


# ------------------------------------------------------------------------------------------ 1. bit for bit
ORDERS = [(1, 1, False), (3, 2, False), (8, 8, False), (1, 0, False), (1, 0, True)]


@pytest.mark.parametrize("p,q,ss", ORDERS, ids=["p1q1", "p3q2", "p8q8", "p1q0", "ss"])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
def test_sweep_is_the_per_step_path_bit_for_bit(E, p, q, ss, monkeypatch):
    from goldsrl import _ffi_sweep
    eng = _snapshot_engine(E, p, q, ss=ss, seed=E + 10 * p)
    twin = [_play(eng, s, 40) for s in RATES7]                          # played once, shared by the 36 sweeps below
    if E > 1:
        assert len(np.unique(twin[3][0][5])) > 1                         # the envs really differ
    for rpl in ("1", "2", "4"):                                          # every rates-per-lane instantiation, each with a ragged tail
        monkeypatch.setenv("GRL_SWEEP_RPL", rpl)
        for n_rates in (1, 3, 5, 7):
            for max_steps in (1, 7, 40):
                eng.reset()
                got = _ffi_sweep.solow_sweep(eng, RATES7[:n_rates], max_steps)
                assert got["total"].shape == (n_rates, E)
                for r in range(n_rates):
                    want = _twin_stats(*twin[r][:3], max_steps)
                    _assert_bits(got, want, r, "rpl %s n_rates %d max_steps %d" % (rpl, n_rates, max_steps))
                assert (got["length"] == max_steps).all() and not got["finished"].any()
    eng.close()


# ------------------------------------------------------------------------------------------ 2. mid-episode start
def test_sweep_from_a_mid_episode_state():
    from goldsrl import _ffi_sweep
    E, cap = 70, 12
    eng = _snapshot_engine(E, 2, 2, cap=cap, seed=5)
    rng = np.random.RandomState(1)
    for _ in range(5):
        eng.step(rng.uniform(0.05, 0.95, size=(E, 1)).astype(np.float32))
    eng.reset(np.arange(0, E, 3))                                        # elapsed 0 / 5, tape_pos 63 / 58 inside one wave
    state = {f: eng.get_state(f) for f in ("SOLOW_K", "SOLOW_Z", "SOLOW_E", "SOLOW_TAPE_POS", "ELAPSED", "NHIST")}
    assert set(state["ELAPSED"]) == {0, 5} and len(np.unique(state["SOLOW_K"])) > E // 2
    rates = RATES7[:5]
    full = _ffi_sweep.solow_sweep(eng, rates, 20)
    cut = _ffi_sweep.solow_sweep(eng, rates, 9)
    for r, s in enumerate(rates):
        rewards, length, finished, _ = _play(eng, s, cap, restore=state)
        assert np.array_equal(length, cap - state["ELAPSED"]) and finished.all()
        _assert_bits(full, _twin_stats(rewards, length, finished, 20), r, "max_steps 20")
        _assert_bits(cut, _twin_stats(rewards, length, finished, 9), r, "max_steps 9")
    assert np.array_equal(full["length"][0], cap - state["ELAPSED"]) and (full["finished"] == 1).all()
    assert np.array_equal(cut["finished"][0], (state["ELAPSED"] == 5).astype(np.uint8))
    eng.close()


# ------------------------------------------------------------------------------------------ 3. the handle is untouched
def test_sweep_leaves_the_handle_untouched_and_grows_its_buffers():
    from goldsrl import _ffi, _ffi_sweep

    def make():
        eng = _ffi.Engine(_ffi.ENV_SOLOW, 65, seed=7, solow_p=2, solow_q=2, solow_tape_len=64, max_episode_steps=24)
        eng.reset()
        eng.episodes_enable()
        rng = np.random.RandomState(2)
        for _ in range(3):
            eng.step(rng.uniform(0.05, 0.95, size=(65, 1)).astype(np.float32))
        return eng

    def everything(eng):
        d = {f: eng.get_state(f) for f in STATE_FIELDS}
        d.update({o: eng.read(o) for o in OUTPUTS})
        d["ep_total"], d["ep_len"] = eng.episodes_running()
        return d

    def same(a, b):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k

    eng, twin = make(), make()
    before = everything(eng)
    first = _ffi_sweep.solow_sweep(eng, RATES7[:3], 30)
    same(before, everything(eng))
    assert (first["length"] == 21).all() and (first["finished"] == 1).all()
    second = _ffi_sweep.solow_sweep(eng, RATES7, 40, trace_env=64)       # more rates, more steps, a trace: every buffer grows
    same(before, everything(eng))
    for k in PAIR_KEYS:
        assert second[k][:3].tobytes() == first[k].tobytes(), k
    assert second["trace_rewards"].shape == (7, 40) and (second["trace_rewards"][:, 21:] == 0).all()
    again = _ffi_sweep.solow_sweep(eng, RATES7[:3], 30)                  # a smaller one in the grown buffers
    for k in PAIR_KEYS:
        assert again[k].tobytes() == first[k].tobytes(), k
    act = np.full((65, 1), 0.4, np.float32)
    eng.step(act); twin.step(act)
    same(everything(twin), everything(eng))
    eng.close(); twin.close()


# ------------------------------------------------------------------------------------------ 4. trace
@pytest.mark.parametrize("cap,steps", [(0, 10), (6, 10)])
def test_trace_is_the_per_step_rewards_and_capital(cap, steps):
    from goldsrl import _ffi, _ffi_sweep
    E, env = 5, 3
    eng = _snapshot_engine(E, 3, 2, cap=cap, seed=9)
    rates = RATES7[:3]
    got = _ffi_sweep.solow_sweep(eng, rates, steps, trace_env=env)
    n = cap if cap else steps
    assert (got["length"] == n).all()
    for r, s in enumerate(rates):
        rewards, _, _, ks = _play(eng, s, n if cap == 0 else n - 1, k_of=env)     # the last step of a capped episode auto-resets k
        m = len(ks)
        assert got["trace_k"][r, :m].tobytes() == ks.tobytes(), r
        if cap:
            rewards = _play(eng, s, n)[0]
        assert got["trace_rewards"][r, :n].tobytes() == rewards[:, env].tobytes(), r
    no_trace = _ffi_sweep.solow_sweep(eng, rates, steps)
    assert "trace_rewards" not in no_trace
    buf = np.zeros((3, steps), np.float32)
    lib = _ffi.load_library(extra_signatures=_ffi_sweep.SWEEP_SIGNATURES)
    assert lib.grl_solow_sweep_read(eng.h, b"trace_k", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE
    eng.close()


# ------------------------------------------------------------------------------------------ 5. tape exhausted, bad arguments
def test_tape_exhausted_is_the_step_paths_error():
    from goldsrl import _ffi, _ffi_sweep
    eng = _snapshot_engine(66, tape=8, cap=0)
    with pytest.raises(_ffi.GrlError) as ei:
        _ffi_sweep.solow_sweep(eng, RATES7[:3], 10)
    assert ei.value.code == _ffi.E_STATE and "66 env(s) popped from an empty shock tape" in str(ei.value)
    ok = _ffi_sweep.solow_sweep(eng, RATES7[:3], 8)                      # the whole tape and no more
    assert (ok["length"] == 8).all() and not ok["finished"].any()
    for _ in range(8):                                                   # the handle's own error counter never saw it
        eng.step(np.full((66, 1), 0.3, np.float32))
    with pytest.raises(_ffi.GrlError) as ej:                             # the step path: the same code and message
        eng.step(np.full((66, 1), 0.3, np.float32))
    assert ej.value.code == _ffi.E_STATE and str(ej.value) == str(ei.value)
    eng.close()


def test_sweep_refuses_bad_arguments():
    from goldsrl import _ffi, _ffi_sweep
    lib = _ffi.load_library(extra_signatures=_ffi_sweep.SWEEP_SIGNATURES)
    eng = _snapshot_engine(4)
    buf = np.zeros((1, 4), np.float64)
    assert lib.grl_solow_sweep_read(eng.h, b"total", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE      # before the first sweep
    r = np.zeros(4097, np.float32)
    for n_rates, max_steps, trace_env in ((0, 4, -1), (4097, 4, -1), (2, 0, -1), (2, 4, 4), (2, 4, -2)):
        assert lib.grl_solow_sweep(eng.h, _ffi._ptr(r), n_rates, max_steps, trace_env) == _ffi.E_INVALID
    assert lib.grl_solow_sweep(eng.h, None, 2, 4, -1) == _ffi.E_INVALID
    eng.step_async(np.full((4, 1), 0.3, np.float32))
    assert lib.grl_solow_sweep(eng.h, _ffi._ptr(r), 2, 4, -1) == _ffi.E_INVALID and b"in flight" in lib.grl_last_error(eng.h)
    eng.wait()
    _ffi_sweep.solow_sweep(eng, r[:2], 4)
    assert lib.grl_solow_sweep_read(eng.h, b"total", _ffi._ptr(buf), buf.nbytes) == _ffi.E_SIZE
    assert lib.grl_solow_sweep_read(eng.h, b"nothing", _ffi._ptr(buf), buf.nbytes) == _ffi.E_INVALID
    trade = _ffi.Engine(_ffi.ENV_TRADE, 4, n_assets=2)
    assert lib.grl_solow_sweep(trade.h, _ffi._ptr(r), 2, 4, -1) == _ffi.E_INVALID
    with pytest.raises(ValueError):
        _ffi_sweep.solow_sweep(trade, r[:2], 4)
    trade.close(); eng.close()


# ------------------------------------------------------------------------------------------ 6. pinned to the reference
@pytest.mark.parametrize("p", [1, 2, 3])
def test_sweep_against_the_reference_script(golden, p):
    """tests/golden/constant_solow.npz: the unmodified scripts/constant_solow.py, float64.  Bound 1e-5 * max(1, |ref|), the
    project's Solow tolerance; the fixture's gap between the best and the second-best mean is 2.8e-4 or
    more, so the arg-max cannot flip inside it."""
    from goldsrl import _ffi
    from goldsrl.baselines import ConstantSavingsBaseline
    g, pre = golden("constant_solow"), "p%d_" % p
    eng = _ffi.Engine(_ffi.ENV_SOLOW, 1, solow_p=p, solow_q=p, solow_tape_len=1024, max_episode_steps=1024, flags=_ffi.F_RESET_FROM_SNAPSHOT)
    eng.set_state("SOLOW_Z0", g[pre + "z0"][None])
    eng.set_state("SOLOW_TAPE", g[pre + "tape_tail"][None])
    b = ConstantSavingsBaseline(rates=g["rates"], engine=eng)
    st = b.run(trace_env=0)
    assert (st["length"] == 1024).all() and (st["finished"] == 1).all()
    worst = {}
    for k in ("mean", "max", "min", "std"):
        ref = g[pre + k]
        worst[k] = float((np.abs(st[k][:, 0] - ref) / np.maximum(1.0, np.abs(ref))).max())
    ref = g[pre + "rewards"]
    worst["rewards"] = float((np.abs(st["trace_rewards"][g["traced"]] - ref) / np.maximum(1.0, np.abs(ref))).max())
    s_max, max_mean, stats = b.best(0)
    print("constant_solow p=%d worst scaled differences: %s; best rate %r mean %r" % (p, worst, s_max, max_mean))
    for k, v in worst.items():
        assert v <= 1e-5, (k, v)
    assert s_max == g["rates"][6] and int(g[pre + "best_index"]) == 6
    assert abs(max_mean - g[pre + "printed"][1]) <= 1e-5
    rate, total = b.best_total()
    assert rate == g["rates"][6] and abs(total - g[pre + "total"][6]) <= 1e-5 * 1024
    b.close()
    assert eng.h is not None                                             # a given engine stays the caller's
    eng.close()


# ------------------------------------------------------------------------------------------ 7. two kernels, one answer
@pytest.mark.parametrize("c", [0, 4])
def test_constant_grid_policy_and_sweep_agree(c):
    from goldsrl import _ffi_discrete, _ffi_sweep
    from goldsrl.agents.a3c.policy_monitor import GridPolicyMonitor
    K, E, cap = 5, 70, 64
    mon = GridPolicyMonitor("Solow-1-1-finite-eval-v0", n_envs=E, n_grid=K, max_episode_steps=cap)
    params, off = np.zeros(mon.net.num_params, np.float32), 0
    for name, shape in _ffi_discrete.discrete_param_shapes(K):
        if name == "probs3_b":
            params[off + c] = 1.0
        off += int(np.prod(shape))
    assert off == params.size
    mon.net.set_params(params)
    mon.net.eng.reset()
    ev = mon.net.eval(cap, trace_steps=1, trace_fields=("choices", "actions"))
    assert (ev["choices"] == c).all()
    action = ev["actions"][0, 0]
    assert action.dtype == np.float32 and (ev["actions"] == action).all() and abs(action - mon.net.grid[c]) < 1e-6
    sw = _ffi_sweep.solow_sweep(mon.net.eng, [action], cap)              # eval left the engine reset
    assert sw["total"][0].tobytes() == ev["total_reward"].tobytes()
    assert np.array_equal(sw["length"][0], ev["length"]) and np.array_equal(sw["finished"][0], ev["finished"])
    assert len(np.unique(sw["total"][0])) == E
    mon.close()


# ------------------------------------------------------------------------------------------ 8. monitors and scripts
class _Global(object):
    """What DeviceSolowPolicyMonitor needs of the learner's estimator: its conf and its flat parameters."""

    def __init__(self):
        from goldsrl import _ffi_flat
        self.conf = {'num_actions': 1, 'entropy_regularisation_strength': 0.02, 'device': '/gpu:0', 'scale': 100.0, 'clip_norm': 40.0,
                     'clip_norm_type': 'global', 'static_size': 2, 'temporal_size': 2, 'static_hidden_size': 32, 'rnn_hidden_size': 32}
        self.flat = _ffi_flat.default_init_flat(5)

    def get_flat_params(self):
        return self.flat


class _Writer(object):
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def flush(self):
        pass


def _monitor(kind, writer):
    from goldsrl import _ffi_discrete, _ffi_gauss
    from goldsrl.agents.a3c.policy_monitor import GridPolicyMonitor, PolicyMonitor
    from goldsrl.agents.paac.policy_monitor import DeviceSolowPolicyMonitor
    env, cap = "Solow-1-1-finite-eval-v0", 32
    if kind == "gauss":
        mon = PolicyMonitor(env, summary_writer=writer, n_envs=4, max_episode_steps=cap)
        params = _ffi_gauss.default_init_gauss(3, **_ffi_gauss.SOLOW_SIZES)
        return mon, lambda: mon.eval_once(params)
    if kind == "grid":
        mon = GridPolicyMonitor(env, summary_writer=writer, n_envs=4, n_grid=11, max_episode_steps=cap)
        params = _ffi_discrete.default_init_discrete(3, 11)
        return mon, lambda: mon.eval_once(params)
    mon = DeviceSolowPolicyMonitor(env, _Global(), summary_writer=writer, n_envs=4, max_episode_steps=cap)
    return mon, lambda: mon.eval_once()


@pytest.mark.parametrize("kind", ["gauss", "grid", "flat"])
def test_monitor_baseline_leaves_the_evaluation_alone(kind):
    from goldsrl.baselines import REFERENCE_RATES
    w = _Writer()
    mon, evaluate = _monitor(kind, w)
    twin, evaluate_twin = _monitor(kind, None)
    rate, total = mon.baseline()
    rates = mon.net.grid if kind == "grid" else REFERENCE_RATES
    assert (rate, total) == (mon.baseline_rate, mon.baseline_total_reward) and rate in list(rates) and np.isfinite(total)
    st = mon.baseline_stats
    assert st["total"].shape == (len(rates), 4) and (st["length"] == 32).all()
    assert total == st["total"].mean(axis=1).max()
    assert (mon.net.eng.get_state("ELAPSED") == 0).all() and (mon.net.eng.get_state("SOLOW_TAPE_POS") == 2047).all()
    got, want = evaluate(), evaluate_twin()
    assert got == want and mon.total_rewards.tobytes() == twin.total_rewards.tobytes()
    n = len(w.rows)
    mon.write_baseline_scalars(17)
    assert w.rows[n:] == [("eval/baseline_total_reward", total, 17),
                          ("eval/mean_total_reward_minus_baseline", mon.log["mean_total_reward"][-1] - total, 17)]
    assert mon.baseline([0.2, 0.4])[0] in (0.2, 0.4)
    twin.write_baseline_scalars(17)                                      # no baseline() yet, no writer: nothing to write
    mon.close(); twin.close()


def test_monitor_baseline_is_for_solow_only():
    from goldsrl.agents.a3c.policy_monitor import PolicyMonitor
    mon = PolicyMonitor("TradeAR1-v0", n_envs=2, max_episode_steps=8)
    with pytest.raises(ValueError):
        mon.baseline()
    mon.close()


def test_train_solow_grid_baseline_flag(tmp_path):
    from goldsrl import utils_tfevents
    from goldsrl.scripts import train_solow_grid

    def run(name, extra):
        out = tmp_path / name
        train_solow_grid.main(["--eval-envs", "4", "--envs", "64", "--updates", "2", "--eval-every", "1", "--model_dir", str(out)] + extra)
        (events,) = glob.glob(os.path.join(str(out), "events.out.tfevents.*"))
        scalars = {}
        for tag, value, step, _ in utils_tfevents.read_scalars(events):
            scalars.setdefault(tag, []).append((step, value))
        with np.load(out / "checkpoint.npz") as z:
            return scalars, z["params"].copy()

    plain, params_plain = run("plain", [])
    base, params_base = run("baseline", ["--baseline"])
    new = {"eval/baseline_total_reward", "eval/mean_total_reward_minus_baseline"}
    assert not new & set(plain) and set(base) == set(plain) | new
    for tag in new:
        assert [s for s, _ in base[tag]] == [s for s, _ in base["eval/mean_total_reward"]] and len(base[tag]) == 2
    b = [v for _, v in base["eval/baseline_total_reward"]]
    assert b[0] == b[1] and np.isfinite(b[0])
    for (_, m), (_, d) in zip(base["eval/mean_total_reward"], base["eval/mean_total_reward_minus_baseline"]):
        assert abs(d - (m - b[0])) <= 1e-6 * max(1.0, abs(m), abs(b[0]))     # scalars are stored as float32
    assert params_base.tobytes() == params_plain.tobytes()
    for tag in plain:
        if tag.startswith("perf/"):
            continue                                                     # wall-clock rates
        assert [s for s, _ in base[tag]] == [s for s, _ in plain[tag]], tag
        got, want = [v for _, v in base[tag]], [v for _, v in plain[tag]]
        if tag in ("train/policy_loss", "train/value_loss", "train/entropy_mean", "train/policy_norm", "train/value_norm"):
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=tag)      # sums in completion order, as tests/test_gpu_flat_eval.py
        else:
            assert got == want, tag
