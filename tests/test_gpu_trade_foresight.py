"""GPU: the foresight ceiling of the TradeAR1 env (grl_trade_foresight / grl_trade_foresight_read of
include/goldsrl_tradeforesight.h; csrc/trade_foresight.hip), TradeForesightCeiling, the monitor's trade_ceiling() and
train_trade --ceiling.

The yardstick of the one-call form is the per-step path, as in tests/test_gpu_trade_sweep.py: grl_step with the recurrence's actions
computed on the host (_ffi_tradeforesight.trade_foresight_actions) from the call's read-back "prices" runs the same float64
operations in the same order, so a pair's prices, actions, account and rewards -- and their sequential float64 sums -- must be the
per-step path's bits.  The recurrence itself is held to a brute force and to the reference env on the CPU
(tests/test_trade_foresight_oracle.py).

The allowance of every bound check: length * 2**-24 * max(|min|, |max|) + 1e-10.  Each float32 step reward is within half an ulp of
its float64 value, which the first term covers; the float64 recurrence's own rounding is orders below the second."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HORIZONS = (0, 1, 2, 4, 16, 64)
PAIR_KEYS = ("total", "sum_sq", "min", "max", "length", "trades", "finished", "depleted")
TRACE_KEYS = ("trace_rewards", "trace_assets", "trace_actions")
STATE_FIELDS = ("TRADE_CASH", "TRADE_ASSETS", "TRADE_QUANTITY", "TRADE_PRICES", "ELAPSED", "EPISODE", "NHIST")
OUTPUTS = ("reward", "done", "elapsed", "obs", "obs_raw", "done_count")


def _engine(E, n, cap=0, inject=True, seed=0):
    from goldsrl import _ffi
    eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=seed, n_assets=n, max_episode_steps=cap, flags=_ffi.F_INJECT_NOISE if inject else 0)
    eng.reset()
    return eng


def _allowance(st, r=None):
    """per pair, from the call's own statistics (or one column's)"""
    pick = (lambda a: a) if r is None else (lambda a: a[r])
    return pick(st["length"]) * 2.0 ** -24 * np.maximum(np.abs(pick(st["min"])), np.abs(pick(st["max"]))).astype(np.float64) + 1e-10


def _play(eng, horizon, prices, last, tape=None):
    """The per-step path from the engine's current state: last.max() + 1 steps of step(the recurrence's actions on the read-back
    prices), with tape[t] (E,n) as TRADE_NORMALS before step t.  While an env's pair lives its TRADE_PRICES must be row t's bytes.
    Returns actions (steps,E,n) and rewards (steps,E) float32, dones (steps,E) bool, the assets after every step (steps,E) float64
    (the reset value where the step ended an episode) and the elapsed counters at the start."""
    from goldsrl._ffi_tradeforesight import trade_foresight_actions
    E, n = eng.E, prices.shape[1]
    el0 = eng.get_state("ELAPSED").copy()
    steps = int(last.max()) + 1
    actions, rewards = np.zeros((steps, E, n), np.float32), np.zeros((steps, E), np.float32)
    dones, assets = np.zeros((steps, E), bool), np.zeros((steps, E))
    live = np.ones(E, bool)
    for t in range(steps):
        p = eng.get_state("TRADE_PRICES")
        assert p[live].tobytes() == np.ascontiguousarray(prices[t].T[live]).tobytes(), "the prices of step %d are not row %d" % (t, t)
        actions[t] = trade_foresight_actions(horizon, prices, t, last)
        if tape is not None:
            eng.set_state("TRADE_NORMALS", tape[t])
        eng.step(actions[t])
        rewards[t], dones[t], assets[t] = eng.read("reward"), eng.read("done") > 0, eng.get_state("TRADE_ASSETS")
        live &= ~dones[t]
    return actions, rewards, dones, assets, el0


def _twin_stats(twin, max_steps, cap=0):
    """What the call keeps, from the per-step path up to each env's first done: sequential float64 sums (np.cumsum adds in order),
    float32 min / max, the trades, and final_assets where the pair did not end (an ended env's assets are already the reset value)."""
    actions, rewards, dones, assets, el0 = twin
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
    traded = (actions != 0).any(axis=2) & live
    return {"total": c1[n - 1, env], "sum_sq": c2[n - 1, env],
            "min": np.where(live, rewards, np.inf).min(axis=0).astype(np.float32),
            "max": np.where(live, rewards, -np.inf).max(axis=0).astype(np.float32),
            "length": n.astype(np.int32), "trades": traded.sum(axis=0).astype(np.int32), "finished": finished.astype(np.uint8),
            "depleted": (finished & ~at_limit).astype(np.uint8), "final_assets": assets[n - 1, env], "open": ~finished}


def _assert_bits(got, want, r, msg):
    for k in PAIR_KEYS:
        assert got[k][r].dtype == want[k].dtype, (k, got[k].dtype, want[k].dtype)
        assert got[k][r].tobytes() == want[k].tobytes(), "%s: %s of horizon column %d differs" % (msg, k, r)
    o = want["open"]
    assert got["final_assets"][r][o].tobytes() == want["final_assets"][o].tobytes(), "%s: final_assets of horizon column %d differs" % (msg, r)


def _assert_trace(got, twin, want, r, env, msg):
    actions, rewards, _, assets, _ = twin
    n = int(want["length"][env])
    assert got["trace_actions"][r, :n].tobytes() == actions[:n, env].tobytes(), "%s: trace_actions of horizon column %d" % (msg, r)
    assert got["trace_rewards"][r, :n].tobytes() == rewards[:n, env].tobytes(), "%s: trace_rewards of horizon column %d" % (msg, r)
    k = n if want["open"][env] else n - 1                                  # the step that ends an episode auto-resets the account
    assert got["trace_assets"][r, :k].tobytes() == assets[:k, env].tobytes(), "%s: trace_assets of horizon column %d" % (msg, r)
    assert got["trace_assets"][r, n - 1] == got["final_assets"][r, env]
    assert not got["trace_rewards"][r, n:].any() and not got["trace_assets"][r, n:].any() and not got["trace_actions"][r, n:].any()


def _check_against_the_step_path(make, horizons, max_steps, cap=0, tape=None, trace_env=None):
    """One call with every horizon against one per-step twin per horizon, each on a fresh engine of make() in the same state."""
    from goldsrl import _ffi_tradeforesight
    from goldsrl._ffi_tradeforesight import trade_foresight_last
    eng = make()
    E, n = eng.E, eng.cfg.n_assets
    env = E - 1 if trace_env is None else trace_env
    got = _ffi_tradeforesight.trade_foresight(eng, horizons, max_steps, trace_env=env, normals=tape)
    assert got["total"].shape == (len(horizons), E) and got["trace_actions"].shape == (len(horizons), max_steps, n)
    prices = got["prices"]
    assert prices.shape == (max_steps, n, E) and prices.dtype == np.float64
    last = trade_foresight_last(max_steps, cap, eng.get_state("ELAPSED"))
    assert prices[0].T.tobytes() == eng.get_state("TRADE_PRICES").tobytes()                 # row 0 is the handle's current p
    for e in range(E):
        assert (prices[:last[e] + 1, :, e] > 0).all() and not prices[last[e] + 1:, :, e].any()    # rows at or past m read as zero
    eng.close()
    twins = []
    for r, H in enumerate(horizons):
        t = make()
        twin = _play(t, H, prices, last, tape)
        t.close()
        want = _twin_stats(twin, max_steps, cap)
        assert np.array_equal(want["length"], last + 1)
        _assert_bits(got, want, r, "E %d n %d horizon %d" % (E, n, H))
        _assert_trace(got, twin, want, r, env, "E %d n %d horizon %d" % (E, n, H))
        assert np.isnan(got["bound"][r]).all() == (H != 0) and np.isnan(got["bound"][r]).any() == (H != 0)
        twins.append(twin)
    return got, twins


# ------------------------------------------------------------------------------------------ 1. bit for bit from a reset
@pytest.mark.parametrize("n", [1, 2, 3, 5, 16, 17])
@pytest.mark.parametrize("E", [1, 65, 130])
def test_foresight_is_the_per_step_path_bit_for_bit(E, n):
    """Ragged waves, every register tier (2 / 4 / 8 / 16) and the LDS form (17), horizons shorter and longer than the 48 steps; once
    with a tape, once with the handle's own generator.  The tape's normals are scaled by 3 so that buys and sales are frequent."""
    tape = (3.0 * np.random.RandomState(E + 1000 * n).normal(size=(48, E, n))).astype(np.float32)
    got, twins = _check_against_the_step_path(lambda: _engine(E, n), HORIZONS, 48, tape=tape)
    assert (got["length"] == 48).all() and not got["finished"].any()
    a0, a1 = twins[0][0], twins[1][0]
    assert (a0 == 1).any() and (a0 == -1).any()                                             # buys and sales
    assert np.array_equal(a0, a1) == (n == 1)      # one asset takes all the cash in one buy, so one row ahead is all there is to know
    assert twins[0][0].tobytes() == twins[5][0].tobytes()                                   # 64 rows ahead is the whole 48-step episode
    assert (got["total"][0] >= got["total"][1:] - _allowance(got)[1:]).all()                # knowing everything is worth no less
    assert np.abs(got["total"][0] - got["bound"][0]).max() <= _allowance(got, 0).max()
    if E > 1:
        assert len(np.unique(got["total"][0])) > 1                                          # the envs really differ
    gen, _ = _check_against_the_step_path(lambda: _engine(E, n, inject=False, seed=5), HORIZONS, 48)
    assert (gen["length"] == 48).all() and (gen["trades"][0] > 0).all()
    assert not np.array_equal(gen["prices"], got["prices"])


# ------------------------------------------------------------------------------------------ 2. mid-episode start
@pytest.mark.parametrize("n", [3, 17])
def test_from_a_mid_episode_state_with_ends_inside_a_wave(n):
    """A prefix of random steps leaves holdings; a third of the envs is reset afterwards, so elapsed is 0 or 5 and the TimeLimit of
    12 ends the pairs at row 11 or row 6 inside one wave."""
    E, cap, seed = 70, 12, 11

    def prefix():
        eng = _engine(E, n, cap=cap, inject=False, seed=seed)
        rng = np.random.RandomState(1)
        for _ in range(5):
            eng.step(rng.uniform(-1, 1, size=(E, n)).astype(np.float32))
        eng.reset(np.arange(0, E, 3))
        return eng

    eng = prefix()
    el, q = eng.get_state("ELAPSED"), eng.get_state("TRADE_QUANTITY")
    eng.close()
    assert set(el) == {0, 5} and (q[el == 5] > 0).any() and not q[el == 0].any()
    got, _ = _check_against_the_step_path(prefix, (0, 2, 64), 20, cap=cap, trace_env=4)     # env 4 has elapsed 5
    assert np.array_equal(got["length"][0], cap - el) and (got["finished"] == 1).all() and not got["depleted"].any()
    assert np.abs(got["total"][0] - got["bound"][0]).max() <= _allowance(got, 0).max()
    cut, _ = _check_against_the_step_path(prefix, (0, 2), 9, cap=cap)                       # max_steps ends the envs of elapsed 0
    assert np.array_equal(cut["finished"][0], (el == 5).astype(np.uint8)) and np.array_equal(cut["length"][0], np.where(el == 5, 7, 9))


# ------------------------------------------------------------------------------------------ 3. pinned to the reference
@pytest.mark.parametrize("n", [2, 3, 16])
def test_foresight_against_the_reference_env(golden, n):
    """tests/golden/trade_foresight.npz: the unmodified TradeAR1Env under the plain-loop recurrence's actions, float64, on the
    normals of trade_rules.npz.  Actions and lengths equal; step rewards within rtol 1e-5, atol 1e-9 and the 256-step totals within
    1e-5 * max(1, |ref|) + 256e-9, the bounds of test_sweep_against_the_reference_env."""
    from goldsrl.baselines import TradeForesightCeiling
    f, g, pre = golden("trade_foresight"), golden("trade_rules"), "n%d_" % n
    eng = _engine(1, n)
    c = TradeForesightCeiling(eng, f["horizons"], max_episode_steps=256)
    st = c.run(trace_env=0, normals=g[pre + "normals"][:, None, :])
    assert (st["length"] == 256).all() and not st["finished"].any()
    assert np.array_equal(st["trace_actions"], f[pre + "actions"])
    ref_r, ref_t = f[pre + "rewards"], f[pre + "total"]
    bound_r = 1e-5 * np.abs(ref_r) + 1e-9
    bound_t = 1e-5 * np.maximum(1.0, np.abs(ref_t)) + 256e-9
    worst_r = float((np.abs(st["trace_rewards"] - ref_r) / bound_r).max())
    worst_t = float((np.abs(st["total"][:, 0] - ref_t) / bound_t).max())
    worst_p = float((np.abs(st["prices"][:, :, 0] - f[pre + "path"]) / f[pre + "path"]).max())
    print("trade_foresight n=%d worst differences in units of the bound: step rewards %.3g, totals %.3g; path relative %.3g; ceiling %r bound %r"
          % (n, worst_r, worst_t, worst_p, c.ceiling(), float(st["bound"][5, 0])))
    assert worst_r <= 1.0 and worst_t <= 1.0
    assert abs(st["bound"][5, 0] - float(f[pre + "bound"])) <= bound_t[5] and c.ceiling() == st["total"][5, 0]
    assert [row[0] for row in c.table()] == [1, 2, 4, 16, 64, 0]
    eng.close()


# ------------------------------------------------------------------------------------------ 4. the bound
def test_bound_holds_over_horizons_rules_and_random_play():
    from goldsrl import _ffi_tradeforesight, _ffi_tradesweep
    from goldsrl.baselines import DEFAULT_TRADE_RULES
    E, n, cap = 66, 3, 40

    def prepared():
        eng = _engine(E, n, cap=cap, inject=False, seed=21)
        rng = np.random.RandomState(4)
        for _ in range(5):
            eng.step(rng.uniform(-1, 1, size=(E, n)).astype(np.float32))
        return eng

    eng = prepared()
    assert (eng.get_state("TRADE_QUANTITY") > 0).any(axis=1).sum() > E // 2
    got = _ffi_tradeforesight.trade_foresight(eng, (0, 1, 4, 64), cap)
    bound, allow = got["bound"][0], _allowance(got)
    assert (got["length"] == 35).all() and not got["depleted"].any() and np.isfinite(bound).all() and (bound > 0).all()
    print("bound test: |total - bound| of horizon 0 at most %.3g (allowance %.3g)" % (np.abs(got["total"][0] - bound).max(), allow[0].min()))
    assert (np.abs(got["total"][0] - bound) <= allow[0]).all()
    for r in (1, 2, 3):
        assert (got["total"][r] <= bound + allow[r]).all(), r
    assert (got["total"][1] < bound - 1e-3).any()                          # one row ahead really earns less
    rules = _ffi_tradesweep.trade_sweep(eng, DEFAULT_TRADE_RULES, cap)
    assert (rules["length"] == 35).all()
    assert (rules["total"] <= bound[None] + _allowance(rules)).all()
    eng.close()
    twin = prepared()
    rng = np.random.RandomState(8)
    rewards = np.zeros((20, E), np.float32)
    for t in range(20):
        twin.step(rng.uniform(-1, 1, size=(E, n)).astype(np.float32))
        rewards[t] = twin.read("reward")
        assert not (twin.read("done") > 0).any()
    twin.close()
    total = rewards.astype(np.float64).sum(axis=0)
    assert (total <= bound + 20 * 2.0 ** -24 * np.abs(rewards).max(axis=0).astype(np.float64) + 1e-10).all()


# ------------------------------------------------------------------------------------------ 5. the handle is untouched
def test_call_leaves_the_handle_untouched_and_grows_its_buffers():
    from goldsrl import _ffi, _ffi_tradeforesight

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
    assert before["reward"].any()
    keys = PAIR_KEYS + ("final_assets", "bound")
    first = _ffi_tradeforesight.trade_foresight(eng, HORIZONS[:3], 30)
    same(before, everything(eng))
    second = _ffi_tradeforesight.trade_foresight(eng, HORIZONS, 40, trace_env=64)          # a second, larger call grows the buffers
    same(before, everything(eng))
    assert (second["length"] == 21).all() and (second["finished"] == 1).all() and not second["depleted"].any()
    assert second["trace_rewards"].shape == (6, 40) and not second["trace_rewards"][:, 21:].any()
    for k in keys:
        assert second[k][:3].tobytes() == first[k].tobytes(), k
    assert second["prices"][:30].tobytes() == first["prices"].tobytes()
    tape = np.random.RandomState(3).normal(size=(50, 65, 3)).astype(np.float32)
    third = _ffi_tradeforesight.trade_foresight(eng, HORIZONS + HORIZONS, 50, trace_env=0, normals=tape)      # every buffer grows, a tape, two plans
    same(before, everything(eng))
    for k in keys + TRACE_KEYS:
        assert third[k][6:].tobytes() == third[k][:6].tobytes(), k
    again = _ffi_tradeforesight.trade_foresight(eng, HORIZONS, 40, trace_env=64)
    for k in keys + TRACE_KEYS + ("prices",):
        assert again[k].tobytes() == second[k].tobytes(), k
    act = np.full((65, 3), 0.4, np.float32)
    eng.step(act); twin.step(act)                                          # the generator counters too: the next prices are the twin's
    same(everything(twin), everything(eng))
    eng.close(); twin.close()


# ------------------------------------------------------------------------------------------ 6. refusals
def test_call_refuses_bad_arguments():
    from goldsrl import _ffi, _ffi_tradeforesight
    lib = _ffi.load_library(extra_signatures=_ffi_tradeforesight.TRADE_FORESIGHT_SIGNATURES)
    P = _ffi._ptr
    eng = _engine(4, 2, inject=False)
    buf = np.zeros((2, 4), np.float64)
    assert lib.grl_trade_foresight_read(eng.h, b"total", P(buf), buf.nbytes) == _ffi.E_STATE        # before the first call
    good = np.arange(65, dtype=np.int32)
    for n_h, max_steps, trace_env, word in ((0, 4, -1, b"n_horizons"), (65, 4, -1, b"n_horizons"), (-1, 4, -1, b"n_horizons"),
                                            (2, 0, -1, b"max_steps"), (2, 4, 4, b"trace_env"), (2, 4, -2, b"trace_env")):
        assert lib.grl_trade_foresight(eng.h, P(good), n_h, None, max_steps, trace_env) == _ffi.E_INVALID
        assert word in lib.grl_last_error(eng.h), lib.grl_last_error(eng.h)
    assert lib.grl_trade_foresight(eng.h, None, 2, None, 4, -1) == _ffi.E_INVALID and b"null" in lib.grl_last_error(eng.h)
    for v in (-1, 1024):
        x = np.array([0, 3, v], np.int32)
        assert lib.grl_trade_foresight(eng.h, P(x), 3, None, 4, -1) == _ffi.E_INVALID
        assert b"horizon 2 is not" in lib.grl_last_error(eng.h), lib.grl_last_error(eng.h)
        with pytest.raises(ValueError, match="horizon 2"):
            _ffi_tradeforesight.trade_foresight(eng, x, 4)
    big = (1 << 25) + 1                                                    # 4 envs x 2 assets x big steps is 8 over 2^28
    assert lib.grl_trade_foresight(eng.h, P(good), 2, None, big, -1) == _ffi.E_INVALID
    msg = lib.grl_last_error(eng.h)
    assert b"max_steps * n_assets * E" in msg and str(8 * big).encode() in msg and b"268435456" in msg, msg
    with pytest.raises(ValueError, match="268435456"):
        _ffi_tradeforesight.trade_foresight(eng, [0], big)
    edge = np.array([1023, 0], np.int32)                                   # the edges of the ranges play
    assert lib.grl_trade_foresight(eng.h, P(edge), 2, None, 4, 3) == _ffi.OK
    assert lib.grl_trade_foresight(eng.h, P(good), 64, None, 4, -1) == _ffi.OK
    eng.step_async(np.full((4, 2), 0.3, np.float32))
    assert lib.grl_trade_foresight(eng.h, P(good), 2, None, 4, -1) == _ffi.E_INVALID and b"in flight" in lib.grl_last_error(eng.h)
    eng.wait()
    noisy = _engine(4, 2, inject=True)
    assert lib.grl_trade_foresight(noisy.h, P(good), 2, None, 4, -1) == _ffi.E_INVALID and b"tape" in lib.grl_last_error(noisy.h)
    tape = np.zeros((4, 2, 4), np.float32)
    assert lib.grl_trade_foresight(noisy.h, P(good), 2, P(tape), 4, -1) == _ffi.OK                   # with a tape it plays
    assert lib.grl_trade_foresight_read(noisy.h, b"total", P(buf), buf.nbytes) == _ffi.OK and (buf == 0).all()      # constant prices
    _ffi_tradeforesight.trade_foresight(eng, [0, 4], 4)
    for name in (b"total", b"bound", b"sum_sq", b"final_assets"):
        assert lib.grl_trade_foresight_read(eng.h, name, P(buf), buf.nbytes) == _ffi.OK
    path = np.zeros((4, 2, 4), np.float64)
    assert lib.grl_trade_foresight_read(eng.h, b"prices", P(path), path.nbytes) == _ffi.OK
    assert np.array_equal(path[0].T, eng.get_state("TRADE_PRICES")) and (path > 0).all()
    assert lib.grl_trade_foresight_read(eng.h, b"prices", P(path), path.nbytes - 8) == _ffi.E_SIZE
    assert lib.grl_trade_foresight_read(eng.h, b"total", P(buf), buf.nbytes - 8) == _ffi.E_SIZE
    assert lib.grl_trade_foresight_read(eng.h, b"trades", P(buf), buf.nbytes) == _ffi.E_SIZE
    assert lib.grl_trade_foresight_read(eng.h, b"finished", P(buf), buf.nbytes) == _ffi.E_SIZE
    assert lib.grl_trade_foresight_read(eng.h, b"nothing", P(buf), buf.nbytes) == _ffi.E_INVALID
    assert lib.grl_trade_foresight_read(eng.h, None, P(buf), buf.nbytes) == _ffi.E_INVALID
    assert lib.grl_trade_foresight_read(eng.h, b"total", None, buf.nbytes) == _ffi.E_INVALID
    for name in TRACE_KEYS:                                                # the last call traced no env
        assert lib.grl_trade_foresight_read(eng.h, name.encode(), P(buf), buf.nbytes) == _ffi.E_STATE
    solow = _ffi.Engine(_ffi.ENV_SOLOW, 4)
    assert lib.grl_trade_foresight(solow.h, P(good), 2, None, 4, -1) == _ffi.E_INVALID
    assert lib.grl_trade_foresight_read(solow.h, b"total", P(buf), buf.nbytes) == _ffi.E_INVALID
    with pytest.raises(ValueError):
        _ffi_tradeforesight.trade_foresight(solow, [0], 4)
    with pytest.raises(ValueError):
        _ffi_tradeforesight.trade_foresight(eng, [0], 4, normals=np.zeros((4, 2, 4)))      # (max_steps, E, n) is (4, 4, 2)
    with pytest.raises(ValueError):
        _ffi_tradeforesight.trade_foresight(eng, [0])                      # no TimeLimit, no default
    solow.close(); noisy.close(); eng.close()


# ------------------------------------------------------------------------------------------ 7. monitor and scripts
class _Writer(object):
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def flush(self):
        pass


def test_trade_ceiling_leaves_the_evaluation_alone_and_bounds_it():
    from goldsrl import _ffi_gauss
    from goldsrl.agents.a3c.policy_monitor import PolicyMonitor
    w = _Writer()
    mon = PolicyMonitor("TradeAR1-v0", summary_writer=w, n_envs=4, max_episode_steps=32)
    twin = PolicyMonitor("TradeAR1-v0", n_envs=4, max_episode_steps=32)
    params = _ffi_gauss.default_init_gauss(3, **_ffi_gauss.TRADE_SIZES)
    seen, played = [], mon.net.eval

    def spy(*a, **k):
        seen.append(played(*a, **k))
        return seen[-1]

    mon.net.eval = spy
    ceilings = []
    for _ in range(2):                                                     # the second evaluation plays other prices than the first
        total = mon.trade_ceiling()
        ceilings.append(total)
        st = mon.ceiling_stats
        assert total == mon.ceiling_total_reward == st["total"][5].mean() and total > 0
        assert [r[0] for r in mon.ceiling_table] == [1, 2, 4, 16, 64, 0] and mon.ceiling_table[5][1] == total
        assert mon.ceiling_bound.tobytes() == st["bound"][5].tobytes() and mon.ceiling_bound.shape == (4,)
        assert (st["length"] == 32).all() and (mon.net.eng.get_state("ELAPSED") == 0).all() and (mon.net.eng.get_state("TRADE_PRICES") == 1).all()
        got, want = mon.eval_once(params), twin.eval_once(params)
        assert got == want and mon.total_rewards.tobytes() == twin.total_rewards.tobytes()
        rewards = np.asarray(seen[-1]["rewards"])[:32]                     # (steps, E) float32: the evaluated episodes
        allow = 32 * 2.0 ** -24 * np.abs(rewards).max(axis=0).astype(np.float64) + 1e-10
        assert (mon.total_rewards <= mon.ceiling_bound + allow).all()       # the same episodes: no policy is above their bound
    assert ceilings[0] != ceilings[1]
    mon.write_ceiling_scalars(3)
    assert w.rows == [("eval/ceiling_total_reward", total, 3)]             # no floor yet
    _, _, floor = mon.rule_baseline()
    del w.rows[:]
    mon.write_ceiling_scalars(4)
    mean = mon.log["mean_total_reward"][-1]
    assert w.rows == [("eval/ceiling_total_reward", total, 4), ("eval/mean_total_reward_share_of_gap", (mean - floor) / (total - floor), 4)]
    assert mon.trade_ceiling([0, 3]) > 0 and len(mon.ceiling_table) == 2
    solow = PolicyMonitor("Solow-1-1-finite-eval-v0", n_envs=2, max_episode_steps=8)
    with pytest.raises(ValueError):
        solow.trade_ceiling()
    solow.close(); mon.close(); twin.close()


def test_train_trade_ceiling_flag(tmp_path, capsys):
    from goldsrl import utils_tfevents
    from goldsrl.scripts import train_trade
    with pytest.raises(SystemExit) as e:
        train_trade.parse_args(["--ceiling", "--eval-every", "1", "--eval-envs", "0"])      # refused as --baseline is
    assert e.value.code == 2 and "--eval-envs" in capsys.readouterr().err
    out = tmp_path / "run"
    train_trade.main(["--eval-envs", "4", "--envs", "64", "--updates", "2", "--eval-every", "1", "--model_dir", str(out), "--baseline", "--ceiling"])
    (events,) = glob.glob(os.path.join(str(out), "events.out.tfevents.*"))
    scalars = {}
    for tag, value, step, _ in utils_tfevents.read_scalars(events):
        scalars.setdefault(tag, []).append((step, value))
    steps = [s for s, _ in scalars["eval/mean_total_reward"]]
    for tag in ("eval/baseline_total_reward", "eval/ceiling_total_reward", "eval/mean_total_reward_share_of_gap"):
        assert [s for s, _ in scalars[tag]] == steps and len(steps) == 2, tag
    c = [v for _, v in scalars["eval/ceiling_total_reward"]]
    b = [v for _, v in scalars["eval/baseline_total_reward"]]
    assert c[0] != c[1] and c[0] > b[0] >= 0 and c[1] > b[1] >= 0          # every evaluation plays other prices
    for (_, mean), (_, share), cv, bv in zip(scalars["eval/mean_total_reward"], scalars["eval/mean_total_reward_share_of_gap"], c, b):
        want = (mean - bv) / (cv - bv)
        assert abs(share - want) <= 1e-5 * max(1.0, abs(want))              # scalars are stored as float32
        assert share <= 1 + 1e-5


def test_trade_foresight_script(tmp_path, capsys):
    from goldsrl.scripts import trade_foresight
    rec = trade_foresight.main(["--envs", "8", "--assets", "3", "--steps", "64", "--seed", "5", "--json", str(tmp_path / "f.json")])
    text = capsys.readouterr().out
    assert "whole episode" in text and "ceiling" in text and "floor" in text
    tot = {r["horizon"]: r["total"] for r in rec["horizons"]}
    assert list(tot) == [1, 2, 4, 16, 64, 0] and rec["ceiling"] == tot[0] == tot[64] and rec["gap"] == rec["ceiling"] - rec["floor"] > 0
    assert tot[0] >= max(tot.values()) - 64 * 2e-7 and os.path.exists(str(tmp_path / "f.json"))
