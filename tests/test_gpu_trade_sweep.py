"""GPU: the scripted trading-rule baseline sweep of the TradeAR1 env (grl_trade_sweep / grl_trade_sweep_read of
include/goldsrl_tradesweep.h; csrc/trade_sweep.hip), the baseline class, the monitor's rule_baseline() and train_trade --baseline.

The yardstick of the one-launch sweep is the per-step path: grl_step with the rule's actions computed on the host from
get_state("TRADE_PRICES") runs the same float64 operations in the same order, so a pair's rewards -- and their sequential float64
sums -- must be the per-step path's bits.  The per-step twin of a case is played once and shared by every sweep of that case.  The
reference env pins the values through tests/golden/trade_rules.npz (the unmodified TradeAR1Env)."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# hold cash, fully invested, sell everything (nothing to sell), two mean-reversion gains, one that saturates the clamp on both sides
RULES7 = np.array([(0, 0), (0, 1), (0, -1), (100, 0), (1000, 0.3), (5, 0.25), (1, -0.5)], np.float32)
PAIR_KEYS = ("total", "sum_sq", "min", "max", "length", "finished", "depleted")
STATE_FIELDS = ("TRADE_CASH", "TRADE_ASSETS", "TRADE_QUANTITY", "TRADE_PRICES", "ELAPSED", "EPISODE", "NHIST")
OUTPUTS = ("reward", "done", "elapsed", "obs", "obs_raw", "done_count")


def _engine(E, n, cap=0, inject=True, seed=0):
    from goldsrl import _ffi
    eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=seed, n_assets=n, max_episode_steps=cap, flags=_ffi.F_INJECT_NOISE if inject else 0)
    eng.reset()
    return eng


def _play(eng, rule, steps, tape=None, reset=True):
    """The per-step path: `steps` calls of step(rule's actions on the current prices), with tape[t] (E,n) as TRADE_NORMALS before
    step t.  Returns rewards (steps,E) float32, dones (steps,E) bool, the assets after every step (steps,E) float64 (the reset
    value where the step ended an episode) and the elapsed counters at the start."""
    from goldsrl._ffi_tradesweep import rule_actions
    E = eng.E
    if reset:
        eng.reset()
    el0 = eng.get_state("ELAPSED").copy()
    rewards, dones, assets = np.zeros((steps, E), np.float32), np.zeros((steps, E), bool), np.zeros((steps, E))
    for t in range(steps):
        if tape is not None:
            eng.set_state("TRADE_NORMALS", tape[t])
        eng.step(rule_actions(rule, eng.get_state("TRADE_PRICES")))
        rewards[t], dones[t], assets[t] = eng.read("reward"), eng.read("done") > 0, eng.get_state("TRADE_ASSETS")
    return rewards, dones, assets, el0


def _twin_stats(twin, max_steps, cap=0):
    """What the sweep keeps, from the per-step path up to each env's first done: sequential float64 sums (np.cumsum adds in order),
    float32 min / max, and final_assets where the pair did not end (an ended env's assets are already the reset value)."""
    rewards, dones, assets, el0 = twin
    steps, E = rewards.shape
    ended = dones.any(axis=0)
    first = np.where(ended, dones.argmax(axis=0) + 1, steps)
    n = np.minimum(first, max_steps)
    finished = ended & (first <= max_steps)
    at_limit = (el0 + n >= cap) if cap > 0 else np.zeros(E, bool)
    r64 = rewards.astype(np.float64)
    c1, c2 = np.cumsum(r64, axis=0), np.cumsum(r64 * r64, axis=0)
    env = np.arange(E)
    live = np.arange(steps)[:, None] < n[None]
    return {"total": c1[n - 1, env], "sum_sq": c2[n - 1, env],
            "min": np.where(live, rewards, np.inf).min(axis=0).astype(np.float32),
            "max": np.where(live, rewards, -np.inf).max(axis=0).astype(np.float32),
            "length": n.astype(np.int32), "finished": finished.astype(np.uint8), "depleted": (finished & ~at_limit).astype(np.uint8),
            "final_assets": assets[n - 1, env], "open": ~finished}


def _assert_bits(got, want, r, msg):
    for k in PAIR_KEYS:
        assert got[k][r].dtype == want[k].dtype, (k, got[k].dtype, want[k].dtype)
        assert got[k][r].tobytes() == want[k].tobytes(), "%s: %s of rule %d differs" % (msg, k, r)
    o = want["open"]
    assert got["final_assets"][r][o].tobytes() == want["final_assets"][o].tobytes(), "%s: final_assets of rule %d differs" % (msg, r)


# ------------------------------------------------------------------------------------------ 1. bit for bit, tape mode
@pytest.mark.parametrize("n", [1, 2, 3, 16, 17, 64])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 130])
def test_sweep_is_the_per_step_path_bit_for_bit(E, n, monkeypatch):
    from goldsrl import _ffi_tradesweep
    eng = _engine(E, n)
    tape = np.random.RandomState(E + 1000 * n).normal(size=(40, E, n)).astype(np.float32)
    twin = [_play(eng, rule, 40, tape) for rule in RULES7]                 # played once, shared by the 36 sweeps below
    if E > 1:
        assert len(np.unique(twin[3][0][5])) > 1                           # the envs really differ
    assert np.abs(twin[4][0]).max() > 0 and (twin[0][0] == 0).all()
    for rpl in ("1", "2", "4"):                                            # every rules-per-lane instantiation, each with a ragged tail
        monkeypatch.setenv("GRL_TRADE_SWEEP_RPL", rpl)
        for n_rules in (1, 3, 5, 7):
            for max_steps in (1, 7, 40):
                eng.reset()
                got = _ffi_tradesweep.trade_sweep(eng, RULES7[:n_rules], max_steps, normals=tape[:max_steps])
                assert got["total"].shape == (n_rules, E)
                for r in range(n_rules):
                    _assert_bits(got, _twin_stats(twin[r], max_steps), r, "rpl %s n_rules %d max_steps %d" % (rpl, n_rules, max_steps))
    eng.close()


# ------------------------------------------------------------------------------------------ 2. bit for bit, device generator
@pytest.mark.parametrize("n", [2, 3])
def test_sweep_with_the_handles_generator_from_a_mid_episode_state(n):
    from goldsrl import _ffi_tradesweep
    E, cap, seed = 70, 12, 11

    def prefix():
        eng = _engine(E, n, cap=cap, inject=False, seed=seed)
        rng = np.random.RandomState(1)
        for _ in range(5):
            eng.step(rng.uniform(-1, 1, size=(E, n)).astype(np.float32))
        eng.reset(np.arange(0, E, 3))                                      # elapsed 0 / 5 and two kinds of account inside one wave
        return eng

    eng = prefix()
    el = eng.get_state("ELAPSED")
    assert set(el) == {0, 5} and len(np.unique(eng.get_state("TRADE_PRICES"))) > E
    rules = RULES7[:5]
    full = _ffi_tradesweep.trade_sweep(eng, rules, 20)
    cut = _ffi_tradesweep.trade_sweep(eng, rules, 9)
    for r, rule in enumerate(rules):
        t = prefix()                                                       # the generator counter cannot be set: replay the prefix
        twin = _play(t, rule, cap, reset=False)
        t.close()
        assert twin[1].any(axis=0).all()
        _assert_bits(full, _twin_stats(twin, 20, cap), r, "max_steps 20")
        _assert_bits(cut, _twin_stats(twin, 9, cap), r, "max_steps 9")
    assert np.array_equal(full["length"][0], cap - el) and (full["finished"] == 1).all() and not full["depleted"].any()
    assert np.array_equal(cut["finished"][0], (el == 5).astype(np.uint8))
    assert len(np.unique(full["total"][3])) > E // 2
    eng.close()


# ------------------------------------------------------------------------------------------ 3. depletion
@pytest.mark.parametrize("n", [2, 3])
def test_depletion_ends_a_pair_as_the_step_path_does(golden, n):
    from goldsrl import _ffi_tradesweep
    g, E = golden("trade_rules"), 66
    crash, rules = g["dep_n%d_normals" % n], g["dep_rules"]
    steps = len(crash)
    tape = np.zeros((steps, E, n), np.float32)
    tape[:, ::2] = crash[:, None]                                          # even envs crash, odd envs see constant prices
    eng = _engine(E, n)
    got = _ffi_tradesweep.trade_sweep(eng, rules, steps, normals=tape)
    for r, rule in enumerate(rules):
        _assert_bits(got, _twin_stats(_play(eng, rule, steps, tape), steps), r, "depletion")
    for r in range(3):
        assert (got["length"][r, ::2] == g["dep_n%d_length" % n][r]).all()                  # where the reference env ends
        assert (got["depleted"][r, ::2] == 1).all() and (got["finished"][r, ::2] == 1).all() and (got["final_assets"][r, ::2] < 1).all()
        assert (got["length"][r, 1::2] == steps).all() and not got["finished"][r, 1::2].any() and not got["depleted"][r, 1::2].any()
    assert (got["total"][3] == 0.0).all() and (got["length"][3] == steps).all() and not got["finished"][3].any()
    eng.close()


# ------------------------------------------------------------------------------------------ 4. the handle is untouched
def test_sweep_leaves_the_handle_untouched_and_grows_its_buffers():
    from goldsrl import _ffi, _ffi_tradesweep

    def make():
        eng = _ffi.Engine(_ffi.ENV_TRADE, 65, seed=7, n_assets=3, max_episode_steps=24)
        eng.reset()
        eng.episodes_enable()
        rng = np.random.RandomState(2)
        for _ in range(3):
            eng.step(rng.uniform(-1, 1, size=(65, 3)).astype(np.float32))
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
    second = _ffi_tradesweep.trade_sweep(eng, RULES7, 40, trace_env=64)    # the larger one first, with a trace
    same(before, everything(eng))
    assert (second["length"] == 21).all() and (second["finished"] == 1).all() and not second["depleted"].any()
    assert second["trace_rewards"].shape == (7, 40) and (second["trace_rewards"][:, 21:] == 0).all() and (second["trace_assets"][:, 21:] == 0).all()
    first = _ffi_tradesweep.trade_sweep(eng, RULES7[:3], 30)               # a smaller one in the grown buffers
    same(before, everything(eng))
    for k in PAIR_KEYS + ("final_assets",):
        assert second[k][:3].tobytes() == first[k].tobytes(), k
    tape = np.random.RandomState(3).normal(size=(50, 65, 3)).astype(np.float32)
    third = _ffi_tradesweep.trade_sweep(eng, RULES7, 50, trace_env=0, normals=tape)        # every buffer grows, a tape appears
    same(before, everything(eng))
    assert third["trace_assets"].shape == (7, 50) and (third["length"] == 21).all()
    again = _ffi_tradesweep.trade_sweep(eng, RULES7, 40, trace_env=64)
    for k in PAIR_KEYS + ("final_assets", "trace_rewards", "trace_assets"):
        assert again[k].tobytes() == second[k].tobytes(), k
    act = np.full((65, 3), 0.4, np.float32)
    eng.step(act); twin.step(act)                                          # the generator counters too: the next prices are the twin's
    same(everything(twin), everything(eng))
    eng.close(); twin.close()


# ------------------------------------------------------------------------------------------ 5. trace
@pytest.mark.parametrize("cap,steps", [(0, 10), (6, 10)])
def test_trace_is_the_per_step_rewards_and_assets(cap, steps):
    from goldsrl import _ffi, _ffi_tradesweep
    E, env, n = 5, 3, 3
    eng = _engine(E, n, cap=cap)
    tape = np.random.RandomState(9).normal(size=(steps, E, n)).astype(np.float32)
    rules = RULES7[3:6]
    got = _ffi_tradesweep.trade_sweep(eng, rules, steps, trace_env=env, normals=tape)
    m = cap if cap else steps
    assert (got["length"] == m).all()
    for r, rule in enumerate(rules):
        rewards, dones, assets, _ = _play(eng, rule, m, tape)
        assert got["trace_rewards"][r, :m].tobytes() == rewards[:, env].tobytes(), r
        k = m - 1 if cap else m                                            # the last step of a capped episode auto-resets the account
        assert got["trace_assets"][r, :k].tobytes() == assets[:k, env].tobytes(), r
        assert got["trace_assets"][r, m - 1] == got["final_assets"][r, env]
        assert (got["trace_rewards"][r, m:] == 0).all() and (got["trace_assets"][r, m:] == 0).all()
        assert got["trace_rewards"][r].astype(np.float64).cumsum()[-1] == got["total"][r, env]
    no_trace = _ffi_tradesweep.trade_sweep(eng, rules, steps, normals=tape)
    assert "trace_rewards" not in no_trace
    lib = _ffi.load_library(extra_signatures=_ffi_tradesweep.TRADE_SWEEP_SIGNATURES)
    buf = np.zeros((3, steps), np.float64)
    assert lib.grl_trade_sweep_read(eng.h, b"trace_assets", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE
    assert lib.grl_trade_sweep_read(eng.h, b"trace_rewards", _ffi._ptr(buf), buf.nbytes // 2) == _ffi.E_STATE
    eng.close()


# ------------------------------------------------------------------------------------------ 6. bad arguments
def test_sweep_refuses_bad_arguments():
    from goldsrl import _ffi, _ffi_tradesweep
    lib = _ffi.load_library(extra_signatures=_ffi_tradesweep.TRADE_SWEEP_SIGNATURES)
    eng = _engine(4, 2, inject=False)
    buf = np.zeros((2, 4), np.float64)
    assert lib.grl_trade_sweep_read(eng.h, b"total", _ffi._ptr(buf), buf.nbytes) == _ffi.E_STATE       # before the first sweep
    g, b = np.zeros(4097, np.float32), np.zeros(4097, np.float32)
    P = _ffi._ptr
    for n_rules, max_steps, trace_env in ((0, 4, -1), (4097, 4, -1), (2, 0, -1), (2, 4, 4), (2, 4, -2)):
        assert lib.grl_trade_sweep(eng.h, P(g), P(b), n_rules, None, max_steps, trace_env) == _ffi.E_INVALID
    assert lib.grl_trade_sweep(eng.h, None, P(b), 2, None, 4, -1) == _ffi.E_INVALID
    assert lib.grl_trade_sweep(eng.h, P(g), None, 2, None, 4, -1) == _ffi.E_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        x = np.zeros(2, np.float32)
        x[1] = bad
        assert lib.grl_trade_sweep(eng.h, P(x), P(b), 2, None, 4, -1) == _ffi.E_INVALID and b"non-finite" in lib.grl_last_error(eng.h)
        assert lib.grl_trade_sweep(eng.h, P(g), P(x), 2, None, 4, -1) == _ffi.E_INVALID
    eng.step_async(np.full((4, 2), 0.3, np.float32))
    assert lib.grl_trade_sweep(eng.h, P(g), P(b), 2, None, 4, -1) == _ffi.E_INVALID and b"in flight" in lib.grl_last_error(eng.h)
    eng.wait()
    noisy = _engine(4, 2, inject=True)
    assert lib.grl_trade_sweep(noisy.h, P(g), P(b), 2, None, 4, -1) == _ffi.E_INVALID and b"tape" in lib.grl_last_error(noisy.h)
    tape = np.zeros((4, 2, 4), np.float32)
    assert lib.grl_trade_sweep(noisy.h, P(g), P(b), 2, P(tape), 4, -1) == _ffi.OK                      # with a tape it plays
    assert lib.grl_trade_sweep_read(noisy.h, b"total", P(buf), buf.nbytes) == _ffi.OK and (buf == 0).all()
    _ffi_tradesweep.trade_sweep(eng, np.zeros((2, 2)), 4)
    assert lib.grl_trade_sweep_read(eng.h, b"total", P(buf), buf.nbytes - 8) == _ffi.E_SIZE
    assert lib.grl_trade_sweep_read(eng.h, b"length", P(buf), buf.nbytes) == _ffi.E_SIZE
    assert lib.grl_trade_sweep_read(eng.h, b"nothing", P(buf), buf.nbytes) == _ffi.E_INVALID
    solow = _ffi.Engine(_ffi.ENV_SOLOW, 4)
    assert lib.grl_trade_sweep(solow.h, P(g), P(b), 2, None, 4, -1) == _ffi.E_INVALID
    assert lib.grl_trade_sweep_read(solow.h, b"total", P(buf), buf.nbytes) == _ffi.E_INVALID
    with pytest.raises(ValueError):
        _ffi_tradesweep.trade_sweep(solow, np.zeros((2, 2)), 4)
    for bad_rules in (np.zeros((2, 3)), np.zeros(2), np.array([[np.nan, 0.0]])):
        with pytest.raises(ValueError):
            _ffi_tradesweep.trade_sweep(eng, bad_rules, 4)
    with pytest.raises(ValueError):
        _ffi_tradesweep.trade_sweep(eng, np.zeros((2, 2)), 4, normals=np.zeros((4, 2, 4)))            # (max_steps, E, n) is (4, 4, 2)
    with pytest.raises(ValueError):
        _ffi_tradesweep.trade_sweep(eng, np.zeros((1, 2)))                                            # no TimeLimit, no default
    solow.close(); noisy.close(); eng.close()


# ------------------------------------------------------------------------------------------ 7. pinned to the reference
@pytest.mark.parametrize("n", [2, 3, 16])
def test_sweep_against_the_reference_env(golden, n):
    """tests/golden/trade_rules.npz: the unmodified TradeAR1Env under the nine default rules, float64.  Step rewards within rtol 1e-5,
    atol 1e-9, the 256-step totals within 1e-5 * max(1, |ref|) + 256e-9: the bound test_trade_steps_golden holds the float64
    account to.  The fixture's best and second-best totals are further apart than twice that, so the arg-max cannot flip."""
    from goldsrl.baselines import DEFAULT_TRADE_RULES, TradingRuleBaseline
    g, pre = golden("trade_rules"), "n%d_" % n
    eng = _engine(1, n)
    b = TradingRuleBaseline(eng, max_episode_steps=256)
    assert b.rules.tobytes() == DEFAULT_TRADE_RULES.tobytes()
    st = b.run(trace_env=0, normals=g[pre + "normals"][:, None, :])
    assert (st["length"] == 256).all() and not st["finished"].any()
    ref_r, ref_a, ref_t = g[pre + "rewards"], g[pre + "assets"], g[pre + "total"]
    bound_r = 1e-5 * np.abs(ref_r) + 1e-9
    bound_t = 1e-5 * np.maximum(1.0, np.abs(ref_t)) + 256e-9
    worst_r = float((np.abs(st["trace_rewards"] - ref_r) / bound_r).max())
    worst_t = float((np.abs(st["total"][:, 0] - ref_t) / bound_t).max())
    worst_a = float((np.abs(st["trace_assets"] - ref_a) / np.abs(ref_a)).max())
    i, rule, total = b.best_total()
    print("trade_rules n=%d worst differences in units of the bound: step rewards %.3g, totals %.3g; assets relative %.3g; best rule %d %r total %r"
          % (n, worst_r, worst_t, worst_a, i, rule, total))
    assert worst_r <= 1.0 and worst_t <= 1.0
    assert i == int(g[pre + "best_index"]) and abs(total - ref_t[i]) <= bound_t[i]
    eng.close()


# ------------------------------------------------------------------------------------------ 8. two kernels, one answer
def test_constant_gaussian_policy_and_sweep_agree():
    from goldsrl import _ffi_gauss, _ffi_tradesweep
    from goldsrl.agents.a3c.policy_monitor import PolicyMonitor
    E, cap = 70, 64
    mon = PolicyMonitor("TradeAR1-v0", n_envs=E, max_episode_steps=cap)
    params, off = np.zeros(mon.net.num_params, np.float32), 0
    for name, shape in _ffi_gauss.gauss_param_shapes(**_ffi_gauss.TRADE_SIZES):
        if name == "mu3_b":
            params[off:off + 2] = 0.5
        off += int(np.prod(shape))
    assert off == params.size
    mon.net.set_params(params)
    mon.net.eng.reset()
    action = mon.net.eval(cap, trace_steps=1, trace_fields=("actions",))["actions"][0, 0, 0]
    assert action.dtype == np.float32 and 0.0 < action < 1.0
    mon.net.eng.reset()                                                    # the prices have moved on: sweep what the NEXT evaluation plays
    sw = _ffi_tradesweep.trade_sweep(mon.net.eng, [(0.0, action)], cap)
    ev = mon.net.eval(cap, trace_steps=cap, trace_fields=("actions",))
    assert (ev["actions"] == action).all()
    assert sw["total"][0].tobytes() == ev["total_reward"].tobytes()
    assert np.array_equal(sw["length"][0], ev["length"]) and np.array_equal(sw["finished"][0], ev["finished"])
    assert len(np.unique(sw["total"][0])) == E
    mon.close()


# ------------------------------------------------------------------------------------------ 9. monitor and script
class _Writer(object):
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def flush(self):
        pass


def test_rule_baseline_leaves_the_evaluation_alone():
    from goldsrl import _ffi_gauss
    from goldsrl.agents.a3c.policy_monitor import PolicyMonitor
    from goldsrl.baselines import DEFAULT_TRADE_RULES
    w = _Writer()
    mon = PolicyMonitor("TradeAR1-v0", summary_writer=w, n_envs=4, max_episode_steps=32)
    twin = PolicyMonitor("TradeAR1-v0", n_envs=4, max_episode_steps=32)
    params = _ffi_gauss.default_init_gauss(3, **_ffi_gauss.TRADE_SIZES)
    for _ in range(2):                                                     # the second evaluation plays other prices than the first
        i, rule, total = mon.rule_baseline()
        assert (i, rule) == mon.baseline_rule and total == mon.baseline_total_reward and np.isfinite(total)
        assert rule == tuple(float(v) for v in DEFAULT_TRADE_RULES[i])
        st = mon.baseline_stats
        assert st["total"].shape == (9, 4) and (st["length"] == 32).all() and (st["total"][0] == 0).all()
        assert total == st["total"].mean(axis=1).max() and total >= 0      # hold cash is rule 0
        assert (mon.net.eng.get_state("ELAPSED") == 0).all() and (mon.net.eng.get_state("TRADE_PRICES") == 1).all()
        got, want = mon.eval_once(params), twin.eval_once(params)
        assert got == want and mon.total_rewards.tobytes() == twin.total_rewards.tobytes()
    n = len(w.rows)
    mon.write_baseline_scalars(17)
    assert w.rows[n:] == [("eval/baseline_total_reward", total, 17),
                          ("eval/mean_total_reward_minus_baseline", mon.log["mean_total_reward"][-1] - total, 17)]
    assert mon.rule_baseline([(0, 0), (0, 1)])[0] in (0, 1)
    with pytest.raises(ValueError):
        mon.baseline()                                                     # the constant-savings baseline stays Solow's
    twin.write_baseline_scalars(17)                                        # no baseline yet, no writer: nothing to write
    solow = PolicyMonitor("Solow-1-1-finite-eval-v0", n_envs=2, max_episode_steps=8)
    with pytest.raises(ValueError):
        solow.rule_baseline()
    solow.close(); mon.close(); twin.close()


def test_train_trade_baseline_flag(tmp_path):
    from goldsrl import utils_tfevents
    from goldsrl.scripts import train_trade

    def run(name, extra):
        out = tmp_path / name
        train_trade.main(["--eval-envs", "4", "--envs", "64", "--updates", "2", "--eval-every", "1", "--model_dir", str(out)] + extra)
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
    assert b[0] != b[1] and np.isfinite(b).all() and min(b) >= 0           # every evaluation plays other prices; hold cash is rule 0
    for (_, m), (_, d), bv in zip(base["eval/mean_total_reward"], base["eval/mean_total_reward_minus_baseline"], b):
        assert abs(d - (m - bv)) <= 1e-6 * max(1.0, abs(m), abs(bv))       # scalars are stored as float32
    assert params_base.tobytes() == params_plain.tobytes()
    for tag in plain:
        if tag.startswith("perf/"):
            continue                                                       # wall-clock rates
        assert [s for s, _ in base[tag]] == [s for s, _ in plain[tag]], tag
        got, want = [v for _, v in base[tag]], [v for _, v in plain[tag]]
        if tag in ("train/policy_loss", "train/value_loss", "train/entropy_mean", "train/policy_norm", "train/value_norm"):
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=tag)      # sums in completion order, as tests/test_gpu_flat_eval.py
        else:
            assert got == want, tag
