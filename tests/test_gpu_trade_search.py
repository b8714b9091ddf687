"""GPU: the cross-entropy search over the four numbers of a TradeAR1 rule (grl_trade_search / grl_trade_search_read of
include/goldsrl_tradesearch.h; csrc/trade_search.hip), the baseline class, the monitor's search_baseline(), train_trade
--search-baseline and the trade_search script.

The yardsticks: trade_search_host, the same search composed on the host from the numpy statements and the per-step path (grl_step
with the rule's actions computed on the host), which the one call must equal byte for byte in all six outputs; grl_trade_sweep, the
parent's kernel, whose "total" the scores of the sub-family gain_buy == gain_sell, ref == 1 must be byte for byte; and the
unmodified reference env through tests/golden/trade_search.npz."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

START = np.array((100, 100, 0, 1), np.float32)
STATE_FIELDS = ("TRADE_CASH", "TRADE_ASSETS", "TRADE_QUANTITY", "TRADE_PRICES", "ELAPSED", "EPISODE", "NHIST")
HANDLE_OUTPUTS = ("reward", "done", "elapsed", "obs", "obs_raw", "done_count")


def _engine(E, n, cap=0, inject=True, seed=0):
    from goldsrl import _ffi
    eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=seed, n_assets=n, max_episode_steps=cap, flags=_ffi.F_INJECT_NOISE if inject else 0)
    eng.reset()
    return eng


def _same(got, want, msg=""):
    from goldsrl._ffi_tradesearch import OUTPUTS
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (msg, k)
        assert got[k].tobytes() == want[k].tobytes(), "%s: %s differs" % (msg, k)


def _symmetric_normals(G, C, seed):
    """normals whose gain_sell column is the gain_buy column: with equal spreads, floors and bounds on the two gains every candidate
    keeps gain_buy == gain_sell bit for bit, generation after generation (the refit's two columns are the same chains)"""
    z = np.random.default_rng(seed).standard_normal((G, C, 4))
    z[:, :, 1] = z[:, :, 0]
    return z


SYM_BOX = dict(spread=(50, 50, 0.25, 0), floor=(2.5, 2.5, 0.0125, 0), lo=(0, 0, -1, 1), hi=(10000, 10000, 1, 1))


# ------------------------------------------------------------------------------------------ 1. the one call is the host composition
@pytest.mark.parametrize("E,n,C,K,cap", [(1, 1, 2, 1, 0), (63, 2, 5, 2, 0), (64, 3, 5, 5, 9), (65, 16, 5, 2, 0), (130, 17, 5, 2, 0), (64, 64, 2, 1, 0)])
def test_the_one_call_is_the_host_composition_byte_for_byte(E, n, C, K, cap, monkeypatch):
    from goldsrl import _ffi_tradesearch as S
    G, T = 3, 12
    eng = _engine(E, n, cap=cap)
    tape = np.random.RandomState(E + 1000 * n).normal(size=(T, E, n)).astype(np.float32)
    kw = dict(generations=G, candidates=C, elites=K, seed=E + n, max_steps=T, tape=tape)
    want = S.trade_search_host(eng, START, **kw)                            # the per-step scoring, once
    assert want["candidates"].shape == (G, C, 4) and want["scores"].shape == (G, C, E) and want["mean"].shape == (G + 1, 4)
    assert (want["candidates"][:, 1:, 0] != want["candidates"][:, 1:, 1]).all()          # asymmetric rules are played
    assert len(np.unique(want["scores"])) > G * (C - 1) * E // 2
    for rpl in ("1", "2", "4"):                                             # C = 5 leaves a ragged last group at 2 and at 4
        monkeypatch.setenv("GRL_TRADE_SEARCH_RPL", rpl)
        eng.reset()
        _same(S.trade_search(eng, START, **kw), want, "rpl " + rpl)
    eng.close()


# ------------------------------------------------------------------------------------------ 2. the symmetric sub-family is the sweep
@pytest.mark.parametrize("n,with_tape", [(2, False), (2, True), (16, False), (17, True), (1, False), (3, True)])
def test_symmetric_candidates_score_the_sweeps_totals_byte_for_byte(n, with_tape):
    from goldsrl import _ffi_tradesearch as S, _ffi_tradesweep
    E, G, C, K, T, cap = 65, 3, 70, 8, 24, 20
    eng = _engine(E, n, cap=cap, inject=False, seed=11)
    rng = np.random.RandomState(1)
    for _ in range(5):
        eng.step(rng.uniform(-1, 1, size=(E, n)).astype(np.float32))
    eng.reset(np.arange(0, E, 3))                                           # elapsed 0 / 5 and two kinds of account inside one wave
    tape = np.random.RandomState(n).normal(size=(T, E, n)).astype(np.float32) if with_tape else None
    out = S.trade_search(eng, START, generations=G, candidates=C, elites=K, normals=_symmetric_normals(G, C, n), max_steps=T, tape=tape, **SYM_BOX)
    cand = out["candidates"]
    assert cand[..., 0].tobytes() == cand[..., 1].tobytes() and (cand[..., 3] == 1).all() and len(np.unique(cand[..., 0])) > G * C // 2
    for g in range(G):
        sw = _ffi_tradesweep.trade_sweep(eng, cand[g][:, (0, 2)], T, normals=tape)
        assert out["scores"][g].tobytes() == sw["total"].tobytes(), g
        assert set(np.unique(sw["length"])) == {cap - 5, cap} and (sw["finished"] == 1).all()           # the TimeLimit falls inside max_steps
    assert len(np.unique(out["scores"][0])) > C * E // 2
    eng.close()


# ------------------------------------------------------------------------------------------ 3. every RPL, the same bytes
@pytest.mark.parametrize("n,C", [(3, 5), (17, 5), (2, 70), (64, 5)])
def test_every_rpl_gives_the_same_bytes(n, C, monkeypatch):
    from goldsrl import _ffi_tradesearch as S
    E = 64 if n == 64 else 130
    eng = _engine(E, n, inject=False, seed=5)
    got = {}
    for rpl in ("1", "2", "4", "3"):                                        # "3" is no value: the default
        monkeypatch.setenv("GRL_TRADE_SEARCH_RPL", rpl)
        got[rpl] = S.trade_search(eng, START, generations=3, candidates=C, elites=2, seed=n, max_steps=16)
    for rpl in ("2", "4", "3"):
        _same(got[rpl], got["1"], "rpl %s against 1" % rpl)
    assert len(np.unique(got["1"]["scores"])) > C * E
    eng.close()


# ------------------------------------------------------------------------------------------ 4. the stops are the sweep's
@pytest.mark.parametrize("n", [2, 3])
def test_depletion_ends_a_pair_as_the_sweep_and_the_step_path_do(golden, n):
    from goldsrl import _ffi_tradesearch as S, _ffi_tradesweep
    g, E = golden("trade_rules"), 66
    crash, rules = g["dep_n%d_normals" % n], g["dep_rules"]
    steps = len(crash)
    tape = np.zeros((steps, E, n), np.float32)
    tape[:, ::2] = crash[:, None]                                           # even envs crash, odd envs see constant prices
    eng = _engine(E, n)
    sw = _ffi_tradesweep.trade_sweep(eng, rules, steps, normals=tape)
    assert (sw["depleted"][:3, ::2] == 1).all() and (sw["length"][:3, ::2] < steps).all() and not sw["depleted"][:, 1::2].any()
    for r, (gain, bias) in enumerate(rules):
        assert S.trade_search_play(eng, (gain, gain, bias, 1), steps, tape).tobytes() == sw["total"][r].tobytes(), r
    # an asymmetric rule that depletes, against the per-step path
    kw = dict(spread=np.zeros(4), floor=np.zeros(4), generations=1, candidates=2, elites=1, max_steps=steps, tape=tape)
    for rule in ((0, 3, 1, 1.5), (2, 0, 0.5, 0.9)):
        want = S.trade_search_host(eng, rule, lo=rule, hi=rule, **kw)
        eng.reset()
        _same(S.trade_search(eng, rule, lo=rule, hi=rule, **kw), want, str(rule))
        assert (want["scores"][0, 0, ::2] < -1).all() and (np.abs(want["scores"][0, 0, 1::2]) < 1).all()
    eng.close()


# ------------------------------------------------------------------------------------------ 5. the handle is untouched
def test_search_leaves_the_handle_and_the_other_results_untouched():
    from goldsrl import _ffi, _ffi_tradeforesight, _ffi_tradesearch as S, _ffi_tradesweep

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
        d.update({o: eng.read(o) for o in HANDLE_OUTPUTS})
        d["ep_total"], d["ep_len"] = eng.episodes_running()
        return d

    def same(a, b):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k

    def last_results(eng):
        from goldsrl._ffi_episode import read_outputs
        lib = _ffi.load_library(extra_signatures=dict(_ffi_tradesweep.TRADE_SWEEP_SIGNATURES, **_ffi_tradeforesight.TRADE_FORESIGHT_SIGNATURES))
        d = read_outputs(eng, lib.grl_trade_sweep_read, (("total", np.float64, ()), ("final_assets", np.float64, ()), ("length", np.int32, ())), (4, 65))
        f = read_outputs(eng, lib.grl_trade_foresight_read, (("total", np.float64, ()), ("bound", np.float64, ())), (2, 65))
        d.update({"foresight_" + k: v for k, v in f.items()})
        return d

    eng, twin = make(), make()
    _ffi_tradesweep.trade_sweep(eng, [(0, 0), (5, 0), (100, 0), (0, 1)], 24)
    _ffi_tradeforesight.trade_foresight(eng, (1, 0), 24)
    before, kept = everything(eng), last_results(eng)
    first = S.trade_search(eng, START, generations=3, candidates=70, elites=8, seed=1, max_steps=20)
    same(before, everything(eng))
    same(kept, last_results(eng))
    small = S.trade_search(eng, START, generations=2, candidates=5, elites=2, seed=2, max_steps=12)      # a smaller one in the grown buffers
    assert small["scores"].shape == (2, 5, 65)
    tape = np.random.RandomState(3).normal(size=(24, 65, 3)).astype(np.float32)
    S.trade_search(eng, START, generations=4, candidates=80, elites=8, seed=3, max_steps=24, tape=tape)   # every buffer grows, a tape appears
    same(before, everything(eng))
    same(kept, last_results(eng))
    _same(S.trade_search(eng, START, generations=3, candidates=70, elites=8, seed=1, max_steps=20), first, "the same call again")
    act = np.full((65, 3), 0.4, np.float32)
    eng.step(act); twin.step(act)                                           # the generator counters too: the next prices are the twin's
    same(everything(twin), everything(eng))
    eng.close(); twin.close()


# ------------------------------------------------------------------------------------------ 6. ties, fixed numbers, the incumbent, errors
def test_ties_fixed_numbers_and_the_incumbent():
    from goldsrl import _ffi_tradesearch as S
    eng = _engine(70, 2, inject=False, seed=3)
    # gains of zero and no bias hold cash whatever ref is: every fit ties at 0 and the order is the index order
    hold = S.trade_search(eng, (0, 0, 0, 1), spread=(0, 0, 0, 0.02), floor=(0, 0, 0, 0.001), generations=3, candidates=9, elites=3, max_steps=12)
    assert (hold["scores"] == 0).all() and (hold["order"] == np.arange(9)).all() and len(np.unique(hold["candidates"][..., 3])) > 20
    assert (hold["candidates"][:, 0] == np.array((0, 0, 0, 1), np.float32)).all()
    want = S.trade_search_refit(np.zeros(9), hold["candidates"][1], 3, (0, 0, 0, 0.001))
    assert hold["mean"][2].tobytes() == want[1].tobytes() and hold["std"][2].tobytes() == want[2].tobytes()
    # zero spread and floor: bias and ref never move, the gains do; candidate 0 is the best row of the generation before, bit for bit
    out = S.trade_search(eng, (100, 100, 0.125, 0.987), spread=(50, 50, 0, 0), floor=(2.5, 2.5, 0, 0), generations=5, candidates=12, elites=4, max_steps=16)
    c = out["candidates"]
    assert (c[..., 2] == np.float32(0.125)).all() and (c[..., 3] == np.float32(0.987)).all() and len(np.unique(c[..., 0])) > 40
    assert (out["mean"][:, 3] == np.float64(np.float32(0.987))).all() and (out["std"][:, 2:] == 0).all() and (out["std"][1:, :2] >= 2.5).all()
    assert c[0, 0].tobytes() == np.array((100, 100, 0.125, 0.987), np.float32).tobytes()
    for g in range(4):
        assert c[g + 1, 0].tobytes() == c[g, out["order"][g, 0]].tobytes(), g
        assert out["scores"][g + 1, 0].tobytes() == out["scores"][g, out["order"][g, 0]].tobytes(), g
    assert (np.diff(out["best_per_generation"]) >= 0).all() and out["best_fit"] == out["fit"][4].max()
    assert out["best_rule"] == tuple(float(v) for v in c[4, out["order"][4, 0]])
    for g in range(5):                                                      # statements 6 and 7 on the device's own scores
        assert out["fit"][g].tobytes() == np.array([S.fit_mean(s) for s in out["scores"][g]]).tobytes()
        assert out["order"][g].tolist() == S.trade_search_rank(out["fit"][g]).tolist()
    eng.close()


def test_the_cap_of_1024_candidates_and_the_error_paths():
    from goldsrl import _ffi, _ffi_tradesearch as S
    lib = _ffi.load_library(extra_signatures=S.TRADESEARCH_SIGNATURES)
    P = _ffi._ptr
    eng = _engine(3, 2, inject=False)
    buf = np.zeros((1, 2), np.float64)
    assert lib.grl_trade_search_read(eng.h, b"fit", P(buf), buf.nbytes) == _ffi.E_STATE and b"call grl_trade_search first" in lib.grl_last_error(eng.h)
    full = S.trade_search(eng, START, generations=2, candidates=1024, elites=1024, seed=4, max_steps=12)
    assert full["order"].shape == (2, 1024) and sorted(full["order"][1].tolist()) == list(range(1024))
    assert full["fit"][1].tobytes() == np.array([S.fit_mean(s) for s in full["scores"][1]]).tobytes()
    assert full["order"][1].tolist() == S.trade_search_rank(full["fit"][1]).tolist()

    start, zero = START.copy(), np.zeros(4)
    spread, floor, lo, hi = S.trade_search_defaults(START)
    z = np.zeros((2, 1025, 4))

    def call(start=start, std0=spread, floor=floor, lo=lo, hi=hi, z=z, tape=None, G=2, C=4, K=2, T=12, h=eng):
        rc = lib.grl_trade_search(h.h, None if start is None else P(start), P(std0), P(floor), P(lo), P(hi), None if z is None else P(z),
                                  None if tape is None else P(tape), G, C, K, T)
        return rc, lib.grl_last_error(h.h)

    def bad(v, k, x):
        v = np.array(v, np.float64)
        v[k] = x
        return v

    nan_start = START.copy()
    nan_start[3] = np.nan
    nan_z = z.copy()
    nan_z.reshape(-1)[3] = np.inf
    for kw, message in ((dict(G=0), b"G must be at least 1"), (dict(C=1), b"C must be in 2..1024"), (dict(C=1025), b"C must be in 2..1024"),
                        (dict(K=0), b"K must be in 1..C"), (dict(K=5), b"K must be in 1..C"), (dict(T=0), b"max_steps must be at least 1"),
                        (dict(start=None), b"null argument"), (dict(z=None), b"null argument"),
                        (dict(start=nan_start), b"start: ref is not finite"), (dict(std0=bad(spread, 1, -1)), b"std0[1] (gain_sell) is negative"),
                        (dict(floor=bad(floor, 2, np.nan)), b"floor[2] (bias) is not finite"), (dict(lo=bad(lo, 2, 2)), b"lo[2] is above hi[2] (bias)"),
                        (dict(hi=bad(hi, 0, 1e39)), b"hi[0] (gain_buy) is not finite as float32"),
                        (dict(lo=bad(lo, 3, -1e39)), b"lo[3] (ref) is not finite as float32"), (dict(z=nan_z), b"normals[3] is not finite")):
        rc, err = call(**kw)
        assert rc == _ffi.E_INVALID and message in err, (kw.keys(), err)
    eng.step_async(np.full((3, 2), 0.3, np.float32))
    rc, err = call()
    assert rc == _ffi.E_INVALID and b"in flight" in err
    eng.wait()
    noisy = _engine(3, 2, inject=True)
    rc, err = call(h=noisy)
    assert rc == _ffi.E_INVALID and b"pass a tape" in err
    assert call(h=noisy, tape=np.zeros((12, 2, 3), np.float32))[0] == _ffi.OK                           # with a tape it plays
    solow = _ffi.Engine(_ffi.ENV_SOLOW, 3)
    rc, err = call(h=solow)
    assert rc == _ffi.E_INVALID and b"not a TradeAR1 handle" in err
    assert lib.grl_trade_search_read(solow.h, b"fit", P(buf), buf.nbytes) == _ffi.E_INVALID
    fit = np.zeros((2, 1024), np.float64)
    assert lib.grl_trade_search_read(eng.h, b"fit", P(fit), fit.nbytes - 8) == _ffi.E_SIZE and b"'fit' needs 16384 bytes" in lib.grl_last_error(eng.h)
    assert lib.grl_trade_search_read(eng.h, b"order", P(fit), fit.nbytes) == _ffi.E_SIZE
    assert lib.grl_trade_search_read(eng.h, b"total", P(fit), fit.nbytes) == _ffi.E_INVALID and b"unknown output 'total'" in lib.grl_last_error(eng.h)
    assert lib.grl_trade_search_read(eng.h, b"fit", P(fit), fit.nbytes) == _ffi.OK and fit.tobytes() == full["fit"].tobytes()   # the refusals spent nothing
    solow.close(); noisy.close(); eng.close()


# ------------------------------------------------------------------------------------------ 7. pinned to the reference
@pytest.mark.parametrize("n", [2, 16])
def test_search_against_the_reference_env(golden, n):
    """tests/golden/trade_search.npz: the search on the unmodified TradeAR1Env, float64, 3 paths x 64 steps, 4 generations of 12
    candidates, 4 elites.  The generator took a seed for which any two fits among ranks 0..K lie further apart than twice
    1e-5 * max(1, |fit|) + 64e-9, the bound test_sweep_against_the_reference_env holds a total to; so the device reproduces every
    table, every elite order, every mean and std exactly, and every fit within that bound."""
    from goldsrl import _ffi_tradesearch as S
    g, pre = golden("trade_search"), "n%d_" % n
    G, C, K = (int(v) for v in g["shape"])
    T = int(g["steps"])
    eng = _engine(3, n)
    out = S.trade_search(eng, g["start"], g[pre + "spread"], g[pre + "floor"], g[pre + "lo"], g[pre + "hi"], G, C, K, normals=g[pre + "normals"],
                         max_steps=T, tape=g[pre + "tape"])
    ref = g[pre + "fit"]
    bound = 1e-5 * np.maximum(1.0, np.abs(ref)) + T * 1e-9
    worst = float((np.abs(out["fit"] - ref) / bound).max())
    print("trade_search n=%d: worst fit difference %.3g of the bound; best fit by generation %s" % (n, worst, out["best_per_generation"].tolist()))
    assert worst <= 1.0
    assert out["candidates"].tobytes() == g[pre + "candidates"].tobytes()
    assert out["order"][:, :K].tobytes() == np.ascontiguousarray(g[pre + "order"][:, :K]).tobytes()
    assert out["mean"].tobytes() == g[pre + "mean"].tobytes() and out["std"].tobytes() == g[pre + "std"].tobytes()
    eng.close()


# ------------------------------------------------------------------------------------------ 8. monitor, script, training flag
class _Writer(object):
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))

    def flush(self):
        pass


def test_search_baseline_plays_the_episodes_of_the_evaluation_that_follows():
    from goldsrl import _ffi_gauss, _ffi_tradesearch as S
    from goldsrl.agents.a3c.policy_monitor import PolicyMonitor
    w = _Writer()
    mon = PolicyMonitor("TradeAR1-v0", summary_writer=w, n_envs=4, max_episode_steps=32)
    twin = PolicyMonitor("TradeAR1-v0", n_envs=4, max_episode_steps=32)
    params = _ffi_gauss.default_init_gauss(3, **_ffi_gauss.TRADE_SIZES)
    totals = []
    for i in range(2):                                                     # the second evaluation plays other prices than the first
        rule, total = mon.search_baseline(2, 6, 2)
        assert rule == mon.search_baseline_rule and total == mon.search_baseline_total_reward and len(rule) == 4
        assert (mon.net.eng.get_state("ELAPSED") == 0).all() and (mon.net.eng.get_state("TRADE_PRICES") == 1).all()
        twin.net.eng.reset()
        want = S.trade_search_play(twin.net.eng, rule, 32)                  # the twin's next evaluation is the monitor's
        assert mon.search_baseline_totals.tobytes() == want.tobytes() and total == S.fit_mean(want)
        got, ref = mon.eval_once(params), twin.eval_once(params)
        assert got == ref and mon.total_rewards.tobytes() == twin.total_rewards.tobytes()
        totals.append((rule, total, mon.search_baseline_in_sample_total_reward))
    assert totals[0][0] == totals[1][0] and totals[0][2] == totals[1][2] and totals[0][1] != totals[1][1]       # tuned once, played twice
    (start, found, fit), = mon.search_baseline_results
    assert start[0] == start[1] and start[3] == 1 and found == rule and fit == mon.search_baseline_in_sample_total_reward
    n = len(w.rows)
    mon.write_search_baseline_scalars(17)
    assert w.rows[n:] == [("eval/search_baseline_total_reward", total, 17),
                          ("eval/mean_total_reward_minus_search_baseline", mon.log["mean_total_reward"][-1] - total, 17),
                          ("eval/search_baseline_in_sample_total_reward", fit, 17)]
    twin.write_search_baseline_scalars(17)                                  # no search yet, no writer: nothing to write
    solow = PolicyMonitor("Solow-1-1-finite-eval-v0", n_envs=2, max_episode_steps=8)
    with pytest.raises(ValueError, match="TradeAR1 env only"):
        solow.search_baseline()
    solow.close(); mon.close(); twin.close()


def test_train_trade_search_baseline_flag(tmp_path):
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

    base, params_base = run("baseline", ["--baseline", "--ceiling"])
    both, params_both = run("search", ["--baseline", "--ceiling", "--search-baseline", "2:6:2"])
    new = {"eval/search_baseline_total_reward", "eval/mean_total_reward_minus_search_baseline", "eval/search_baseline_in_sample_total_reward"}
    assert not new & set(base) and set(both) == set(base) | new
    for tag in new:
        assert [s for s, _ in both[tag]] == [s for s, _ in both["eval/mean_total_reward"]] and len(both[tag]) == 2
    t = [v for _, v in both["eval/search_baseline_total_reward"]]
    ins = [v for _, v in both["eval/search_baseline_in_sample_total_reward"]]
    assert t[0] != t[1] and ins[0] == ins[1] and np.isfinite(t + ins).all()  # tuned once; every evaluation plays other prices
    for (_, m), (_, d), tv in zip(both["eval/mean_total_reward"], both["eval/mean_total_reward_minus_search_baseline"], t):
        assert abs(d - (m - tv)) <= 1e-6 * max(1.0, abs(m), abs(tv))        # scalars are stored as float32
    assert params_both.tobytes() == params_base.tobytes()
    for tag in base:
        if tag.startswith("perf/"):
            continue                                                        # wall-clock rates
        assert [s for s, _ in both[tag]] == [s for s, _ in base[tag]], tag
        got, want = [v for _, v in both[tag]], [v for _, v in base[tag]]
        if tag in ("train/policy_loss", "train/value_loss", "train/entropy_mean", "train/policy_norm", "train/value_norm"):
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=0, err_msg=tag)       # sums in completion order, as tests/test_gpu_flat_eval.py
        else:
            assert got == want, tag


def test_the_script_prints_the_four_point_scale(tmp_path, capsys):
    import json

    from goldsrl.scripts import trade_search
    path = tmp_path / "scale.json"
    rec = trade_search.main(["--n-assets", "3", "--envs", "5", "--steps", "24", "--search", "3:8:3", "--json", str(path)])
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("TradeAR1, 3 assets, 5 envs x 24 steps; search: 3 generations of 8 candidates, 3 elites")
    assert [line.split("  ")[0].strip() for line in lines[1:]] == ["mean total_reward", "best default rule", "tuned rule", "foresight ceiling"]
    assert "in sample" in lines[1] and "other seeds" in lines[1] and "gain_buy" in lines[3]
    assert rec["default_total"] <= rec["tuned_in_sample"] <= rec["ceiling"] and rec["tuned_other_seeds"] <= rec["ceiling_other_seeds"]
    assert rec["default_total_other_seeds"] <= rec["ceiling_other_seeds"] and len(rec["tuned_rule"]) == 4
    assert "%.6f" % rec["tuned_in_sample"] in lines[3] and "%.6f" % rec["ceiling"] in lines[4] and "%.6f" % rec["default_total"] in lines[2]
    with open(path) as f:
        assert json.load(f)["tuned_in_sample"] == rec["tuned_in_sample"]
