"""GPU: episode ends that differ from env to env inside a wave.

Everywhere else in the suite all envs of a batch finish on the same step, so every done mask a kernel sees is all-ones or
all-zeros (or the all-ones prefix of a partial tail wave).  Here the masks are scattered (tests/_async_scenarios.py; the CPU
test tests/test_async_scenarios.py asserts that they are): the staggered TimeLimit ends about 7 different envs of every wave
on every step, the TradeAR1 depletion configuration ends envs one by one.  Checked against the float64 oracles:

  1. step path of all four envs: done mask, count, compacted list, counters, untouched neighbours, the reset state, R6 records;
  2. Engine.reset(idx) with a list;
  3. TradeAR1 through its resets, injected normals and the device price generator (counter runs on across resets);
  4. the persistent flat rollout against the graph of launches (bit for bit) and against the oracle;
  5. the A3C Gaussian worker's windows, terminal values, GAE cut and update;
  6. Solow ARMA(p, q) at batch size (struct-of-arrays stride) and the set_state / get_state transposition.

E = 200 is three waves plus a partial one of 8 lanes; 20 steps."""
import os

import numpy as np
import pytest

import _async_scenarios as SC
import _gauss_oracle as A
from oracle import oracle as O
from oracle import ticker as TK

pytestmark = pytest.mark.gpu

E, T, CAP = SC.E, SC.T, SC.CAP
SEED, OFF = SC.GEN_SEED, SC.GEN_OFFSET
GOLD_TICKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ticker.npz")


def _ffi():
    from goldsrl import _ffi
    return _ffi


def _raw_done_list(eng, count):
    """The device's done list as the kernels left it (read("done_list") hands it out sorted)."""
    return eng.dev_download(eng.out_ptrs().done_list, (eng.E,), np.int32)[:count]


def _check_records(recs, oracle_recs, n_env):
    """The rule of test_gpu_bookkeeping._check: record by record, totals bit-equal."""
    assert len(recs) == len(oracle_recs) and len(recs) > 0
    for r, (gstep, env, length, total) in zip(recs, oracle_recs):
        assert (int(r["step_index"]) - 1) * n_env + int(r["env"]) + 1 == gstep
        assert int(r["env"]) == env and int(r["length"]) == length
        assert r["total_reward"] == total


# ------------------------------------------------------------------------------------------ per-kind description
class Kind(object):
    """How to build, drive and check one env kind in parts 1 and 2."""

    def __init__(self, name, n_env=None):
        self.name = name
        self.env = name.split("_")[0]
        self.E = n_env or (SC.SWARM_E if self.env == "swarm" else E)
        self.pq = (3, 2) if name == "solow_p3q2" else (1, 1)
        self.tape_len = 32
        self.matrix = np.load(GOLD_TICKER)["matrix"] if self.env == "ticker" else None

    def engine(self, cap):
        f = _ffi()
        kw = dict(seed=SEED, env_id_offset=OFF)
        if cap is not None:
            kw["max_episode_steps"] = cap
        if self.env == "solow":
            eng = f.Engine(f.ENV_SOLOW, self.E, solow_p=self.pq[0], solow_q=self.pq[1], solow_tape_len=self.tape_len, **kw)
        elif self.env == "trade":
            eng = f.Engine(f.ENV_TRADE, self.E, n_assets=3, **kw)
        elif self.env == "swarm":
            eng = f.Engine(f.ENV_SWARM, self.E, **kw)
        else:
            eng = f.Engine(f.ENV_TICKER, self.E, **kw)
            eng.ticker_set_table(self.matrix)
        eng.reset()
        return eng

    def actions(self, rng):
        n = self.E
        if self.env == "solow":
            return rng.rand(n, 1).astype(np.float32)
        if self.env == "trade":
            return np.tanh(rng.normal(size=(n, 3))).astype(np.float32)
        if self.env == "swarm":
            return O.swarm_transform_actions(rng.normal(size=(n, 10, 2)).astype(np.float32))
        cont = (1.0 / (1.0 + np.exp(-rng.normal(size=(n, 2))))).astype(np.float32)
        return np.concatenate([rng.randint(0, 3, size=(n, 2)).astype(np.float32), cont], axis=1)

    @property
    def fields(self):
        return {"solow": ("SOLOW_K", "SOLOW_Z", "SOLOW_E", "SOLOW_TAPE", "SOLOW_TAPE_POS", "NHIST"),
                "trade": ("TRADE_CASH", "TRADE_ASSETS", "TRADE_QUANTITY", "TRADE_PRICES", "NHIST"),
                "swarm": ("SWARM_X", "SWARM_XA", "SWARM_PNOISE", "SWARM_ANOISE"),
                "ticker": ("TICKER_CASH", "TICKER_ASSETS", "TICKER_QUANTITY", "TICKER_IDX", "TICKER_START", "NHIST")}[self.env]

    @property
    def outputs(self):
        return {"solow": ("reward", "obs_raw", "obs", "history"),
                "trade": ("reward", "obs_raw", "obs"),
                "swarm": ("reward", "reward_f64", "locust_bins", "agent_bins", "positions"),
                "ticker": ("reward", "reward_f64", "obs_raw", "obs")}[self.env]

    def snapshot(self, eng):
        d = {f: eng.get_state(f) for f in self.fields}
        d.update({"out_" + o: eng.read(o) for o in self.outputs})
        return d

    def check_reset_state(self, eng, idx, nhist):
        """Envs idx are in the state a reset leaves: the oracle generator's draws at episode EPISODE - 1."""
        idx = np.asarray(idx)
        ep = eng.get_state("EPISODE")[idx].astype(np.int64) - 1
        genv = idx + OFF
        assert (eng.get_state("ELAPSED")[idx] == 0).all()
        if self.env == "solow":
            p = self.pq[0]
            kss = O.solow_k_ss(0.33)
            np.testing.assert_allclose(eng.get_state("SOLOW_K")[idx], kss, rtol=1e-6)
            assert not eng.get_state("SOLOW_E")[idx].any()
            z = SC.solow_reset_z(SEED, genv, ep, p)
            np.testing.assert_allclose(eng.get_state("SOLOW_Z")[idx], z, rtol=1e-6, atol=1e-8)
            np.testing.assert_allclose(eng.get_state("SOLOW_TAPE")[idx], SC.solow_reset_tape(SEED, genv, ep, self.tape_len),
                                       rtol=1e-6, atol=1e-8)
            assert (eng.get_state("SOLOW_TAPE_POS")[idx] == self.tape_len - 1).all()
            assert (eng.get_state("NHIST")[idx] == nhist).all()
            gz = eng.get_state("SOLOW_Z")[idx]
            raw, obs, hist = eng.read("obs_raw")[idx], eng.read("obs")[idx], eng.read("history")[idx]
            np.testing.assert_allclose(raw[:, 0], kss, rtol=1e-6)
            assert np.array_equal(raw[:, 1], gz[:, p - 1])              # the observation shows the NEWEST lag
            np.testing.assert_allclose(obs[:, 0], kss / 100.0, rtol=1e-6)
            assert np.array_equal(obs[:, 1], gz[:, p - 1])
            assert np.array_equal(hist[:, 0], obs) and not hist[:, 1:].any()      # one row, zero padded (quirk Q11)
        elif self.env == "trade":
            start, n = 10.0, 3
            assert (eng.get_state("TRADE_CASH")[idx] == start).all() and (eng.get_state("TRADE_ASSETS")[idx] == start).all()
            assert not eng.get_state("TRADE_QUANTITY")[idx].any() and (eng.get_state("TRADE_PRICES")[idx] == 1.0).all()
            assert (eng.get_state("NHIST")[idx] == nhist).all()
            robs = SC.trade_reset_obs(len(idx), n, start)
            assert np.array_equal(eng.read("obs_raw")[idx], robs.astype(np.float32))
            np.testing.assert_allclose(eng.read("obs")[idx], O.trade_process_state(robs), rtol=1e-5, atol=1e-6)
        elif self.env == "swarm":
            ox, oxa, opn, oan = SC.swarm_reset_state(SEED, genv, ep)
            gx, gxa = eng.get_state("SWARM_X")[idx], eng.get_state("SWARM_XA")[idx]
            np.testing.assert_allclose(gxa, oxa, rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(gx, ox, rtol=1e-10, atol=1e-11)
            np.testing.assert_allclose(eng.get_state("SWARM_PNOISE")[idx], opn, rtol=1e-13, atol=1e-15)
            np.testing.assert_allclose(eng.get_state("SWARM_ANOISE")[idx], oan, rtol=1e-13, atol=1e-15)
            lb, ab, pos = eng.read("locust_bins")[idx], eng.read("agent_bins")[idx], eng.read("positions")[idx]
            for i in range(len(idx)):       # the observation is the reset one: the oracle's binning of the device's own positions
                olb, oab, opos = O.swarm_observe_compact(gx[i], gxa[i], 84)
                assert np.array_equal(pos[i], opos)
                assert np.array_equal(lb[i], np.where(olb < 0, 255, olb).astype(np.uint8))
                assert np.array_equal(ab[i], np.where(oab < 0, 255, oab).astype(np.uint8))
        else:
            starts = SC.ticker_reset_start(SEED, genv, ep, self.matrix.shape[0])
            st, obs = TK.ticker_reset(self.matrix, starts)
            assert np.array_equal(eng.get_state("TICKER_START")[idx], starts)
            assert np.array_equal(eng.get_state("TICKER_CASH")[idx], st["cash"])
            assert np.array_equal(eng.get_state("TICKER_ASSETS")[idx], st["assets"])
            assert np.array_equal(eng.get_state("TICKER_QUANTITY")[idx], st["qty"])
            assert np.array_equal(eng.get_state("TICKER_IDX")[idx], st["idx"])
            assert (eng.get_state("NHIST")[idx] == nhist).all()
            np.testing.assert_array_equal(eng.read("obs_raw")[idx], obs.astype(np.float32))
            np.testing.assert_allclose(eng.read("obs")[idx], TK.ticker_process_state(obs), rtol=3e-7, atol=1e-7)


KINDS = ("solow", "solow_p3q2", "trade", "swarm", "ticker")


# ------------------------------------------------------------------------------------------ 1. step path
@pytest.mark.parametrize("name", KINDS)
def test_step_path_with_staggered_time_limit(name):
    K = Kind(name)
    n = K.E
    eng, ctl = K.engine(CAP), K.engine(0)           # the control never ends an episode: same seed, same actions
    el0 = SC.staggered_elapsed(n)
    eng.set_state("ELAPSED", el0)
    eng.episodes_enable()
    want_done = SC.timelimit_dones(el0, T)
    elapsed, episode = el0.astype(np.int64), eng.get_state("EPISODE").astype(np.int64)
    assert (episode == 1).all()
    fresh = np.ones(n, bool)                        # envs that have not finished yet
    rng = np.random.RandomState(4)
    rews, dones = [], []
    for t in range(T):
        act = K.actions(rng)
        tape0 = eng.get_state("SOLOW_TAPE") if K.env == "solow" else None
        eng.step(act); ctl.step(act)
        d = eng.read("done").astype(bool)
        assert np.array_equal(d, want_done[t]), t
        cnt = int(eng.read("done_count")[0])
        assert cnt == int(d.sum())
        raw = _raw_done_list(eng, cnt)
        assert len(set(raw.tolist())) == cnt, (t, raw)
        assert np.array_equal(np.sort(raw), np.flatnonzero(d)), (t, raw)
        assert np.array_equal(eng.read("done_list"), np.flatnonzero(d))
        elapsed = np.where(d, 0, elapsed + 1)
        episode = episode + d
        assert np.array_equal(eng.get_state("ELAPSED"), elapsed) and np.array_equal(eng.read("elapsed"), elapsed)
        assert np.array_equal(eng.get_state("EPISODE"), episode)
        assert not ctl.read("done").any()
        # a neighbour's reset touches nothing else: envs that have not finished are the control's, bit for bit; the terminal
        # reward of an env's first end is the control's too (the reward stays, quirk Q6)
        live = fresh & ~d
        a, b = K.snapshot(eng), K.snapshot(ctl)
        for k in a:
            assert np.array_equal(a[k][live], b[k][live]), (t, k)
        for k in ("out_reward", "out_reward_f64"):
            if k in a:
                assert np.array_equal(a[k][fresh], b[k][fresh]), (t, k)
        fresh = live
        idx = np.flatnonzero(d)
        if len(idx):
            K.check_reset_state(eng, idx, nhist=1)
        if tape0 is not None:                       # only the finished envs' tapes were redrawn
            assert np.array_equal(eng.get_state("SOLOW_TAPE")[~d], tape0[~d]), t
        rews.append(eng.read("reward")); dones.append(d)
    rews, dones = np.array(rews), np.array(dones)
    assert not fresh.any() and SC.mixed_share(dones) >= 0.5
    orecs, total, steps, _ = O.episode_bookkeeping(rews, dones)
    _check_records(eng.episodes_read(), orecs, n)
    rt, rl = eng.episodes_running()
    assert np.array_equal(rt, total) and np.array_equal(rl, steps)
    eng.close(); ctl.close()


# ------------------------------------------------------------------------------------------ 2. reset of a list
@pytest.mark.parametrize("name", ["solow", "solow_p3q2", "trade", "swarm"])
def test_reset_of_a_list_leaves_the_other_envs_alone(name):
    f = _ffi()
    K = Kind(name, n_env=E)
    n = K.E
    idx = np.array(SC.RESET_IDX)                    # unsorted, both ends of the batch, both sides of a wave boundary
    eng = K.engine(None)
    rng = np.random.RandomState(6)
    for t in range(3):
        eng.step(K.actions(rng))
    assert not eng.read("done").any()
    before = K.snapshot(eng)
    before.update(ELAPSED=eng.get_state("ELAPSED"), EPISODE=eng.get_state("EPISODE"),
                  out_done=eng.read("done"), out_reward=eng.read("reward"))
    assert (before["ELAPSED"] == 3).all() and (before["EPISODE"] == 1).all()
    eng.reset(idx)
    after = K.snapshot(eng)
    after.update(ELAPSED=eng.get_state("ELAPSED"), EPISODE=eng.get_state("EPISODE"),
                 out_done=eng.read("done"), out_reward=eng.read("reward"))
    other = np.ones(n, bool); other[idx] = False
    for k in before:
        assert np.array_equal(after[k][other], before[k][other]), k
    assert np.array_equal(after["out_reward"], before["out_reward"]) and np.array_equal(after["out_done"], before["out_done"])
    assert (after["EPISODE"][idx] == 2).all() and (after["ELAPSED"][idx] == 0).all()
    K.check_reset_state(eng, idx, nhist=0)          # an explicit reset: the worker's list starts empty
    # the engine still steps, and the listed envs count from 0
    eng.step(K.actions(rng))
    want = np.where(other, 4, 1)
    assert np.array_equal(eng.get_state("ELAPSED"), want)
    for bad in ([n], [-1], [0, n + 5, 1]):
        with pytest.raises(f.GrlError):
            eng.reset(bad)
    with pytest.raises(f.GrlError):
        eng.reset(np.zeros(n + 1, np.int32))        # n > E
    assert np.array_equal(eng.get_state("ELAPSED"), want)      # a refused reset changed nothing
    eng.close()


# ------------------------------------------------------------------------------------------ 3. TradeAR1 through its resets
def _trade_vs_oracle(eng, n, acts, normals, inject):
    kw = SC.TRADE_DEPLETION[n]
    o = SC.trade_oracle(n, kw["trade_starting_balance"], kw["trade_std_p"], acts, normals)
    print("TradeAR1 n=%d: mixed share %.2f, depletion dones %d, min |assets' - 1| %.2e"
          % (n, SC.mixed_share(o["done"]), int(o["own_done"].sum()), o["gap"]))
    assert SC.mixed_share(o["done"]) >= 0.5 and o["own_done"].sum() >= E and o["gap"] >= SC.MIN_GAP
    robs = SC.trade_reset_obs(E, n, kw["trade_starting_balance"])
    assert np.array_equal(eng.read("obs_raw"), robs.astype(np.float32))
    for t in range(T):
        if inject:
            eng.set_state("TRADE_NORMALS", normals[t])
        eng.step(acts[t])
        d = eng.read("done").astype(bool)
        assert np.array_equal(d, o["done"][t]), (t, np.flatnonzero(d != o["done"][t]))
        # every env on every step, those that play on behind their reset included; tolerances of
        # test_trade_batch_vs_oracle_and_price_moments
        np.testing.assert_allclose(eng.read("obs_raw"), o["obs"][t], rtol=2e-5, atol=2e-6, err_msg="step %d" % t)
        np.testing.assert_allclose(eng.read("reward"), o["reward"][t], rtol=1e-5, atol=1e-9, err_msg="step %d" % t)
        np.testing.assert_allclose(eng.read("obs"), O.trade_process_state(o["obs"][t]), rtol=1e-5, atol=1e-6)
        cnt = int(eng.read("done_count")[0])
        raw = _raw_done_list(eng, cnt)
        assert cnt == d.sum() and np.array_equal(np.sort(raw), np.flatnonzero(d))
    assert np.array_equal(eng.get_state("EPISODE"), 1 + o["episodes"]) and np.array_equal(eng.get_state("ELAPSED"), o["elapsed"])
    # the float64 account: libm's pow / exp / log differ from numpy's by a few ulp per step, 20 steps
    for fld, ref in (("TRADE_CASH", o["cash"]), ("TRADE_ASSETS", o["assets"]), ("TRADE_QUANTITY", o["q"]), ("TRADE_PRICES", o["p"])):
        np.testing.assert_allclose(eng.get_state(fld), ref, rtol=1e-9, atol=1e-12, err_msg=fld)


@pytest.mark.parametrize("n", [2, 3, 16])
def test_trade_through_resets_with_injected_normals(n):
    f = _ffi()
    eng = f.Engine(f.ENV_TRADE, E, n_assets=n, flags=f.F_INJECT_NOISE, **SC.TRADE_DEPLETION[n])
    eng.reset()
    acts, nrm = SC.trade_inputs(n, SC.TRADE_INPUT_SEED[n])
    _trade_vs_oracle(eng, n, acts, nrm, inject=True)
    eng.close()


@pytest.mark.parametrize("n", [2, 3, 16])
def test_trade_through_resets_with_the_device_price_generator(n):
    """The draws of oracle.rng_block at counter nstep * pairs + a // 2: nstep does not restart at a reset, the even asset
    takes the first normal of its pair, an odd n leaves half of the last pair unused."""
    f = _ffi()
    eng = f.Engine(f.ENV_TRADE, E, n_assets=n, seed=SEED, env_id_offset=OFF, **SC.TRADE_DEPLETION[n])
    eng.reset()
    acts, _ = SC.trade_inputs(n, SC.TRADE_INPUT_SEED[n])
    _trade_vs_oracle(eng, n, acts, SC.trade_generator_normals(SEED, OFF, E, T, n), inject=False)
    eng.close()


# ------------------------------------------------------------------------------------------ 4. persistent flat rollout
FLAT_CASES = {
    "solow_stagger": dict(kind="solow", stagger=True),
    "trade16": dict(kind="trade", n=16, stagger=False),
    "trade3": dict(kind="trade", n=3, stagger=False),
    "trade16_stagger": dict(kind="trade", n=16, stagger=True),
    "trade3_gae": dict(kind="trade", n=3, stagger=False, gae_lambda=0.96),
}
ROLLOUTS = 3


def _async_flat_job(case, mode, group, monkeypatch):
    """One engine + FlatNet + three rollouts with R6 accounting on, as test_gpu_flatnet._flat_job, on an asynchronous scenario."""
    f = _ffi()
    from goldsrl import rollout as R
    c = FLAT_CASES[case]
    if mode == "graph":
        monkeypatch.setenv("GRL_FLAT_ROLLOUT", "graph")
    else:
        monkeypatch.delenv("GRL_FLAT_ROLLOUT", raising=False)
    if group is None:
        monkeypatch.delenv("GRL_FLAT_GROUP", raising=False)
    else:
        monkeypatch.setenv("GRL_FLAT_GROUP", str(group))
    cap = CAP if c["stagger"] else 1024
    if c["kind"] == "solow":
        eng = f.Engine(f.ENV_SOLOW, E, seed=SEED, env_id_offset=OFF, max_episode_steps=cap, solow_tape_len=64)
        fields = ("SOLOW_K", "SOLOW_Z", "SOLOW_E", "SOLOW_TAPE", "SOLOW_TAPE_POS", "NHIST", "ELAPSED", "EPISODE")
    else:
        eng = f.Engine(f.ENV_TRADE, E, seed=SEED, env_id_offset=OFF, n_assets=c["n"], rnn_length=20, max_episode_steps=cap,
                       **SC.TRADE_POLICY_DEPLETION[c["n"]])
        fields = ("TRADE_CASH", "TRADE_ASSETS", "TRADE_QUANTITY", "TRADE_PRICES", "NHIST", "ELAPSED", "EPISODE")
    eng.reset()
    if c["stagger"]:
        eng.set_state("ELAPSED", SC.staggered_elapsed(E))
    eng.episodes_enable(capacity=8 * E)
    kw = {"gae_lambda": c["gae_lambda"]} if "gae_lambda" in c else {}
    roll = R.FlatPolicyRollout(eng, T, train=False, **kw)
    net = roll.net
    Aa, S0 = net.cfg.num_actions, net.cfg.static_size
    out = []
    for _ in range(ROLLOUTS):
        roll.run(); eng.wait()
        d = {k: net.read_rollout(k, (T, E)) for k in ("values", "rewards", "masks", "y", "adv")}
        d["actions"] = net.read_rollout("actions", (T, E, Aa))
        d["env_actions"] = eng.transform_actions(d["actions"])       # what the envs were stepped with (the same tanhf / sigmoid)
        d["states"] = net.read_rollout("states", (T, E, S0))
        d["boot"] = net.read_rollout("boot", (E,))
        if c["kind"] == "solow":
            d["histories"] = net.read_rollout("histories", (T, E, 5, 2))
        else:
            d["nhist"] = net.read_rollout("nhist", (T, E)).view(np.int32)
        for fld in fields:
            d["st_" + fld] = eng.get_state(fld)
        for o in ("obs", "obs_raw", "reward", "done"):
            d["out_" + o] = eng.read(o)
        cnt = int(eng.read("done_count")[0])
        d["done_list"] = np.sort(_raw_done_list(eng, cnt))
        recs = eng.episodes_read()
        d["recs"] = np.array([(int(r["step_index"]), int(r["env"]), int(r["length"]), float(r["total_reward"])) for r in recs])
        out.append(d)
    pred = net.predict_env()
    info = dict(scale=float(net.cfg.scale), gamma=float(net.cfg.gamma))
    net.close(); eng.close()
    return out, pred, info


_graph_jobs = {}


def _graph_job(case, monkeypatch):
    """The launch-per-stage rollout of a case, computed once and shared (left unchanged) by 4a and 4b."""
    if case not in _graph_jobs:
        _graph_jobs[case] = _async_flat_job(case, "graph", None, monkeypatch)
    return _graph_jobs[case]


def _recorded_dones(job):
    return np.concatenate([1.0 - d["masks"] for d in job]).astype(bool)


def _trade_replay(case, job):
    """The recorded env actions of all rollouts through O.trade_step + per-env reset, with the device generator's draws: the
    counter runs on across resets AND across rollouts."""
    c = FLAT_CASES[case]
    n = c["n"]
    kw = SC.TRADE_POLICY_DEPLETION[n]
    acts = np.concatenate([d["env_actions"] for d in job])
    assert (np.abs(acts) <= 1).all()
    return SC.trade_oracle(n, kw["trade_starting_balance"], kw["trade_std_p"], acts,
                           SC.trade_generator_normals(SEED, OFF, E, ROLLOUTS * T, n),
                           SC.staggered_elapsed(E) if c["stagger"] else None, CAP if c["stagger"] else 0)


def _assert_async(case, job, replay=None):
    """The policy chose the actions, so the scenario conditions are asserted on what was recorded (first rollout: 20 steps)."""
    dones = _recorded_dones(job)
    assert np.array_equal(job[0]["done_list"], np.flatnonzero(dones[T - 1]))
    share = SC.mixed_share(dones[:T])
    print("%s: first rollout mixed share %.2f, dones %d" % (case, share, int(dones[:T].sum())))
    assert share >= 0.25
    if replay is not None:
        assert np.array_equal(dones, replay["done"])        # so the oracle's depletion flags are the rollout's
        dep = int(replay["own_done"][:T].sum())
        print("%s: first rollout depletion dones %d, oracle min |assets' - 1| %.2e over %d steps"
              % (case, dep, replay["gap"], ROLLOUTS * T))
        assert dep >= E // 4


@pytest.mark.parametrize("case", ["solow_stagger", "trade16", "trade3", "trade16_stagger"])
def test_persistent_rollout_is_bit_identical_to_the_graph_with_asynchronous_ends(case, monkeypatch):
    b, pb, _ = _graph_job(case, monkeypatch)
    _assert_async(case, b, _trade_replay(case, b) if FLAT_CASES[case]["kind"] == "trade" else None)
    for group in (64, 32, 16, None):
        a, pa, _ = _async_flat_job(case, "persistent", group, monkeypatch)
        for u, (da, db) in enumerate(zip(a, b)):
            assert sorted(da) == sorted(db)
            for k in da:
                assert np.array_equal(da[k], db[k]), (case, group, u, k)
        for k in pa:
            assert np.array_equal(pa[k], pb[k])
    assert sum(len(d["recs"]) for d in b) == _recorded_dones(b).sum()


def _gae_cut(rews, vals, masks, boot, gamma, lam):
    """test_trade_rollout_with_the_a3c_workers_gae's reference: O.gae per episode segment, bootstrap 0 behind a finished one."""
    steps, n_env = rews.shape
    oy, oadv = np.zeros((steps, n_env)), np.zeros((steps, n_env))
    for b in range(n_env):
        ends = [t for t in range(steps) if masks[t, b] == 0]
        t0 = 0
        for t1 in ends + [steps - 1]:
            seg = slice(t0, t1 + 1)
            bt = np.zeros(1) if t1 in ends else boot[b:b + 1].astype(np.float64)
            if t0 <= t1:
                a, tgt = O.gae(rews[seg, b:b + 1].astype(np.float64), vals[seg, b:b + 1].astype(np.float64), bt, gamma, lam)
                oadv[seg, b], oy[seg, b] = a[:, 0], tgt[:, 0]
            t0 = t1 + 1
    return oy, oadv


@pytest.mark.parametrize("mode", ["persistent", "graph"])
@pytest.mark.parametrize("case", ["trade16", "trade3", "trade16_stagger", "trade3_gae"])
def test_flat_trade_rollout_through_resets_against_the_oracle(case, mode, monkeypatch):
    """The recorded actions replayed through the oracle (_trade_replay): rewards, masks and the next observation on every step of
    every env, the window lengths, the returns with the recorded masks, the account the last rollout leaves, the R6 records."""
    c = FLAT_CASES[case]
    n = c["n"]
    if mode == "graph":
        job, _, info = _graph_job(case, monkeypatch)
    else:
        job, _, info = _async_flat_job(case, "persistent", None, monkeypatch)
    kw = SC.TRADE_POLICY_DEPLETION[n]
    o = _trade_replay(case, job)
    _assert_async(case, job, o)
    robs = O.trade_process_state(SC.trade_reset_obs(E, n, kw["trade_starting_balance"]))
    for u, d in enumerate(job):
        sl = slice(u * T, (u + 1) * T)
        assert np.array_equal(d["masks"], 1.0 - o["done"][sl]), (u, np.argwhere(d["masks"] != 1.0 - o["done"][sl])[:4])
        np.testing.assert_allclose(d["rewards"], o["reward"][sl], rtol=1e-5, atol=1e-9)
        nxt = O.trade_process_state(o["obs"][sl])           # the reset observation behind a done
        first = robs if u == 0 else O.trade_process_state(o["obs"][u * T - 1])
        np.testing.assert_allclose(d["states"][0], first, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(d["states"][1:], nxt[:-1], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(d["out_obs"], nxt[-1], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(d["out_obs_raw"], o["obs"][sl][-1], rtol=2e-5, atol=2e-6)
        assert np.array_equal(d["out_done"].astype(bool), o["done"][sl][-1])
        # the worker's window length: 0 after the explicit reset (shown as one row), 1 behind a done, +1 per step up to rnn + 1
        if u == 0:
            nh = np.zeros(E, np.int64)
        for t in range(T):
            assert np.array_equal(d["nhist"][t], nh), (u, t)
            nh = np.where(o["done"][u * T + t], 1, np.minimum(nh + 1, 21))
        assert np.array_equal(d["st_NHIST"], nh)
        # returns with the recorded masks
        if "gae_lambda" in c:
            oy, oadv = _gae_cut(d["rewards"], d["values"], d["masks"], d["boot"], info["gamma"], c["gae_lambda"])
        else:
            oy, oadv = O.nstep_returns(O.rescale_reward(d["rewards"]).astype(np.float64), d["values"], d["boot"], info["gamma"],
                                       d["masks"].astype(np.float64))
        np.testing.assert_allclose(d["y"], oy, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(d["adv"], oadv / info["scale"], rtol=1e-5, atol=1e-6)
    last = job[-1]
    assert np.array_equal(last["st_EPISODE"], 1 + o["episodes"]) and np.array_equal(last["st_ELAPSED"], o["elapsed"])
    for fld, ref in (("TRADE_CASH", o["cash"]), ("TRADE_ASSETS", o["assets"]), ("TRADE_QUANTITY", o["q"]), ("TRADE_PRICES", o["p"])):
        np.testing.assert_allclose(last["st_" + fld], ref, rtol=1e-9, atol=1e-12, err_msg=fld)
    orecs = O.episode_bookkeeping(np.concatenate([d["rewards"] for d in job]), o["done"])[0]
    got = np.concatenate([d["recs"] for d in job if len(d["recs"])])
    assert len(got) == len(orecs)
    for r, (gstep, env, length, total) in zip(got, orecs):
        assert (int(r[0]) - 1) * E + int(r[1]) + 1 == gstep and int(r[1]) == env and int(r[2]) == length and r[3] == total


# ------------------------------------------------------------------------------------------ 5. A3C Gaussian worker
GAUSS_REC = ("states", "windows", "raw", "values", "rewards", "dones", "weights", "adv", "targets", "boot", "term_values")


@pytest.mark.parametrize("kind", ["solow", "trade"])
def test_gauss_worker_with_asynchronous_ends(kind):
    f = _ffi()
    from goldsrl import _ffi_gauss
    R = 5
    sizes = A.SOLOW if kind == "solow" else A.TRADE
    D, Aa, P = sizes["static_size"], sizes["num_actions"], A.num_params(**sizes)
    ab = kind == "solow"
    scale = 100.0 if ab else 1.0
    if ab:
        eng = f.Engine(f.ENV_SOLOW, E, seed=SEED, env_id_offset=OFF, max_episode_steps=CAP, solow_tape_len=64)
    else:
        eng = f.Engine(f.ENV_TRADE, E, seed=SEED, env_id_offset=OFF, n_assets=2, **SC.TRADE_POLICY_DEPLETION[2])
    eng.reset()
    if ab:
        eng.set_state("ELAPSED", SC.staggered_elapsed(E))
    eng.episodes_enable()
    net = _ffi_gauss.GaussNet(eng, rnn_length=R, scale=scale, max_samples=8192)
    assert net.cfg.always_bootstrap == int(ab)
    p = A.init(4, **sizes)
    rng = np.random.RandomState(4)
    for k in p:
        if k.endswith("_b"):
            p[k] = p[k] + 0.05 * rng.normal(size=p[k].shape)
    net.set_params(A.flatten(p).astype(np.float32))
    lr = 1e-3
    hist = []                       # every rollout so far: the windows of the second one carry over from the first
    for u in range(2):
        params0, opt0 = net.get_params(), net.get_optimizer_state()
        net.rollout(T)
        r = {k: net.read_rollout(k) for k in GAUSS_REC + (("term_states", "term_windows") if ab else ())}
        eps = eng.episodes_read()
        hist.append(r)
        dn = r["dones"] > 0
        share = SC.mixed_share(dn)
        print("gauss %s rollout %d: mixed share %.2f, dones %d" % (kind, u, share, int(dn.sum())))
        assert share >= 0.25 and dn.sum() >= E // 4            # TradeAR1: every done is a depletion (cap 1024)
        if ab:
            assert np.array_equal(dn, SC.timelimit_dones(SC.staggered_elapsed(E), 2 * T)[u * T:(u + 1) * T])
        # windows restart where an episode ended and carry over elsewhere, also from one rollout to the next
        states = np.concatenate([h["states"] for h in hist]); dones = np.concatenate([h["dones"] for h in hist])
        if ab:
            win, wts, twin = A.replay_windows(states, dones, R, np.concatenate([h["term_states"] for h in hist]))
            np.testing.assert_array_equal(r["term_windows"][dn], twin[u * T:][dn])
            got = net.predict(r["term_states"][dn], r["term_windows"][dn])["values"]
            assert np.array_equal(got, r["term_values"][dn]) and np.all(got != 0)
        else:
            win, wts = A.replay_windows(states, dones, R)
        assert not r["term_values"][~dn].any() and (ab or not r["term_values"].any())
        np.testing.assert_array_equal(r["windows"], win[u * T:])
        np.testing.assert_array_equal(r["weights"], wts[u * T:])
        assert (r["weights"] == 0).any() and (r["weights"] == 1).any()
        # the worker's GAE cut at every env's own episode ends; tolerances of test_rollout_replay
        adv, tgt = A.gae_segments(r["rewards"], r["values"], r["boot"], r["dones"], r["term_values"], ab, 0.99, 0.96, scale)
        np.testing.assert_allclose(r["adv"], adv, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(r["targets"], tgt, rtol=1e-5, atol=1e-6 * scale)
        last = dn[-1]
        assert last.any() and not last.all()
        assert np.array_equal(r["boot"][last], r["term_values"][-1][last])
        assert len(eps) == int(dn.sum())
        # the device-resident update gives the bits of the host-sample update on what was read back
        s1 = net.train_rollout(lr=lr)
        g_ro, p_ro, opt_ro = (net.get_grads("policy"), net.get_grads("value")), net.get_params(), net.get_optimizer_state()
        net.set_params(params0)
        net.set_optimizer_state(opt0["ms_policy"], opt0["ms_value"], opt0["global_step"])
        s2 = net.train(r["states"].reshape(-1, D), r["windows"].reshape(-1, R, D), r["raw"].reshape(-1, Aa), r["adv"].reshape(-1),
                       r["targets"].reshape(-1), r["weights"].reshape(-1), grad_mult=1.0 / E, lr=lr)
        assert np.array_equal(net.get_grads("policy"), g_ro[0]) and np.array_equal(net.get_grads("value"), g_ro[1])
        assert np.array_equal(net.get_params(), p_ro) and not np.array_equal(p_ro, params0)
        assert s1["policy_norm"] == s2["policy_norm"] and s1["value_norm"] == s2["value_norm"]
        opt2 = net.get_optimizer_state()
        assert np.array_equal(opt2["ms_policy"], opt_ro["ms_policy"]) and opt2["global_step"] == opt_ro["global_step"]
    net.close(); eng.close()


# ------------------------------------------------------------------------------------------ 6. Solow ARMA(p, q) at batch size
@pytest.mark.parametrize("p,q", [(1, 1), (3, 2), (2, 0)])
def test_solow_arma_batch_vs_oracle(p, q):
    """test_solow_batch_vs_oracle's scheme with p, q > 1 and E > 1: lag i of env e lives at i * E + e on the device, a stride no
    E = 1 test can see; every env holds different values in every lag."""
    f = _ffi()
    TL = 32
    Q = max(q, 1)
    rng = np.random.RandomState(5)
    eng = f.Engine(f.ENV_SOLOW, E, solow_p=p, solow_q=q, solow_tape_len=TL, max_episode_steps=0, flags=f.F_RESET_FROM_SNAPSHOT)
    eng.reset()
    k = (40 + 60 * rng.rand(E)).astype(np.float32)
    z = (rng.normal(size=(E, p)) * 0.2).astype(np.float32)
    e = (rng.normal(size=(E, Q)) * 0.1).astype(np.float32)
    if q == 0:
        e[:] = 0                    # the reference's e starts empty: no MA term on the first step, then e = [e_t]
    tape = (rng.normal(size=(E, TL)) * 0.1).astype(np.float32)
    eng.set_state("SOLOW_K", k); eng.set_state("SOLOW_Z", z); eng.set_state("SOLOW_E", e); eng.set_state("SOLOW_TAPE", tape)
    for fld, v in (("SOLOW_K", k), ("SOLOW_Z", z), ("SOLOW_E", e), ("SOLOW_TAPE", tape)):
        assert np.array_equal(eng.get_state(fld), v), fld
    rho_z, rho_e = O.solow_rhos(p, q)
    ok, oz, oe = k.astype(np.float64), z.astype(np.float64), e.astype(np.float64)
    for t in range(T):
        s = rng.rand(E).astype(np.float32)
        eng.step(s[:, None])
        ok, oz, oe, oobs, orew = O.solow_step(ok, oz, oe, tape[:, TL - 1 - t].astype(np.float64), s.astype(np.float64), rho_z, rho_e)
        np.testing.assert_allclose(eng.read("obs_raw"), oobs, rtol=1e-5, atol=1e-6, err_msg="step %d" % t)
        np.testing.assert_allclose(eng.read("reward"), orew, rtol=1e-5, atol=5e-6, err_msg="step %d" % t)
        # every lag, not only the newest one the observation shows
        np.testing.assert_allclose(eng.get_state("SOLOW_Z"), oz, rtol=1e-5, atol=1e-6, err_msg="step %d" % t)
        np.testing.assert_allclose(eng.get_state("SOLOW_E"), oe, rtol=1e-5, atol=1e-6, err_msg="step %d" % t)
    assert np.array_equal(eng.get_state("SOLOW_TAPE"), tape) and (eng.get_state("SOLOW_TAPE_POS") == TL - 1 - T).all()
    eng.close()


def test_feature_major_fields_round_trip():
    """(E, P) on the host <-> [P][E] on the device: get_state(set_state(x)) == x with a different value in every (env, feature),
    and the kernels read the same layout (a step with injected normals moves price a of env e by normal (e, a))."""
    f = _ffi()
    rng = np.random.RandomState(8)
    so = f.Engine(f.ENV_SOLOW, E, solow_p=3, solow_q=2, solow_tape_len=32, flags=f.F_RESET_FROM_SNAPSHOT)
    so.reset()
    for fld, dt in (("SOLOW_Z", np.float32), ("SOLOW_E", np.float32), ("SOLOW_TAPE", np.float32), ("SOLOW_Z0", np.float32)):
        shape = so.field_shape(fld)
        x = (np.arange(int(np.prod(shape))).reshape(shape) + rng.rand(*shape)).astype(dt)
        so.set_state(fld, x)
        assert np.array_equal(so.get_state(fld), x), fld
    so.close()
    n = 3
    tr = f.Engine(f.ENV_TRADE, E, n_assets=n, flags=f.F_INJECT_NOISE)
    tr.reset()
    vals = {}
    for fld in ("TRADE_QUANTITY", "TRADE_PRICES", "TRADE_NORMALS"):
        shape = tr.field_shape(fld)
        x = 1.0 + (np.arange(int(np.prod(shape))).reshape(shape) + rng.rand(*shape)) / 1000.0
        x = x.astype(np.float32) if fld == "TRADE_NORMALS" else x
        tr.set_state(fld, x)
        assert np.array_equal(tr.get_state(fld), x), fld
        vals[fld] = x
    tr.observe()
    raw = tr.read("obs_raw")
    assert np.array_equal(raw[:, 1:1 + n], vals["TRADE_QUANTITY"].astype(np.float32))
    assert np.array_equal(raw[:, 1 + n:], vals["TRADE_PRICES"].astype(np.float32))
    tr.step(np.zeros((E, n), np.float32))           # hold: only the prices move, each by its own normal
    p1 = vals["TRADE_PRICES"] ** 0.9 * np.exp(O.trade_std_e() * vals["TRADE_NORMALS"].astype(np.float64))
    np.testing.assert_allclose(tr.get_state("TRADE_PRICES"), p1, rtol=1e-12)
    tr.close()
