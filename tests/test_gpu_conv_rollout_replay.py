"""GPU: the env half of grl_net_rollout on Swarm, replayed step by step on a twin engine.

The gradient half of the conv rollout is held to the float64 oracle (tests/test_gpu_net_tiles.py, test_gpu_keep_levels.py); of its
env half only step 0 of one chunk was (test_device_rollout_matches_oracle_pieces).  What the rollout does per chunk -- a range
step at an env base that is no multiple of SWARM_EPB = 4, the done list at done_list + env_base with one counter per lane, two
chunks of a lane sharing that counter, the reset launched from the list while other lanes step, the bookkeeping and the reward /
done copy per range, the observation record taken before the step, the bootstrap forward on the state the last reset left -- can
be wrong by an offset and still give a rollout that is consistent with ITSELF: the stored observations feed the stored values.

So every rollout here is replayed on a TWIN: a second engine of the same configuration and seed, stepped over the whole batch
(Engine.step) with the rollout's recorded actions, and a second ConvNet on it that only evaluates given observations.  Per step:
the twin's observation equals the recorded one byte for byte, values[t] equals predict_obs(recorded observation) bit for bit,
actions[t] is mu + sigma * eps of the oracle's generator (rtol 1e-6, atol 1e-7: the bound of
test_device_rollout_matches_oracle_pieces), the twin's reward and done equal the recorded ones bit for bit, and the dones are the
CPU schedule.  Behind the last step: the env state, the TimeLimit and episode counters, the bootstrap values, the R6 records
and running sums of the two engines are equal, and y / adv are the reference's unmasked grid loop (O.nstep_returns) at the
existing bounds.  The whole-batch step path the twin runs is itself held to the float64 oracle with scattered ends
(tests/test_gpu_async_dones.py part 1, swarm), so the rollout is tied to the oracle through the twin.

Scenario (tests/_async_scenarios.py, conditions asserted on the CPU by tests/test_async_scenarios.py): 37 envs in chunks of 7
-- bases 7, 14, 21, 28, 35, a last chunk of 2 envs, chunks 4 and 5 on the lanes of chunks 0 and 1 --, TimeLimit(9) with staggered
counters so that 4 or 5 scattered envs end on every step, 20 steps, action counter from 1000, biased parameters."""
import time

import numpy as np
import pytest

import _async_scenarios as SC
from oracle import nets as NN
from oracle import oracle as O
from test_gpu_net_tiles import _biased_params, _check_grads, _states

pytestmark = pytest.mark.gpu

E, T, CAP = SC.REPLAY_E, SC.T, SC.CAP
B = E * 10
CE = SC.REPLAY_CHUNK_ENVS
SEED, OFF = SC.GEN_SEED, SC.GEN_OFFSET
PARAM_SEED = 9
ACT_RTOL, ACT_ATOL = 1e-6, 1e-7
F_PER_AGENT_TRUNK, F_SINGLE_STREAM = 0x1, 0x4      # GRL_NET_F_* (include/goldsrl_net.h)
STATE_FIELDS = ("SWARM_X", "SWARM_XA", "SWARM_PNOISE", "SWARM_ANOISE", "ELAPSED", "EPISODE")
OBS = (("lb", "locust_bins", (80, 2)), ("ab", "agent_bins", (10, 2)), ("ps", "positions", (10, 2)))
STORED = ("lb", "ab", "ps", "acts", "vals", "dones", "boot")      # what the lanes must not change
EL0 = SC.staggered_elapsed(E, CAP)
SCHEDULE = SC.timelimit_dones(EL0, SC.REPLAY_ROLLOUTS * T + SC.REPLAY_GRAD_T)      # (44, E): every rollout of case A


def _engine(elapsed=EL0):
    from goldsrl import _ffi
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, seed=SEED, env_id_offset=OFF, max_episode_steps=CAP)
    eng.reset()
    eng.set_state("ELAPSED", elapsed)
    eng.episodes_enable()
    return eng


def _net(eng, flags, chunk):
    from goldsrl import _ffi_net
    net = _ffi_net.ConvNet(eng, max_chunk_samples=chunk, reserved=flags)
    net.set_params(_biased_params(PARAM_SEED)[0])
    return net


class Pair(object):
    """The engine and net under test (action counter at 1000) and their twin."""

    def __init__(self, flags=0, chunk=SC.REPLAY_CHUNK_SAMPLES, lanes=None, monkeypatch=None):
        for k in ("GRL_NET_KEEP_LEVEL", "GRL_NET_KEEP_FREE_MB"):
            monkeypatch.delenv(k, raising=False)
        if lanes is None:
            monkeypatch.delenv("GRL_NET_LANES", raising=False)
        else:
            monkeypatch.setenv("GRL_NET_LANES", str(lanes))      # read when a net is created
        self.eng, self.twin = _engine(), _engine()
        self.net, self.tnet = _net(self.eng, flags, chunk), _net(self.twin, flags, chunk)
        self.net.set_action_counter(SC.REPLAY_COUNTER0)
        self.steps = 0      # steps taken so far: the schedule's row and the action counter's offset

    def rollout(self, steps, layout):
        """One rollout and everything read back from it, the engine's state behind it included."""
        self.net.rollout(steps, layout)
        self.eng.wait()
        ro = _read(self.eng, self.net, steps)
        ro.update(layout=layout, counter0=SC.REPLAY_COUNTER0 + self.steps, t0=self.steps)
        assert self.net.get_action_counter() == ro["counter0"] + steps
        self.steps += steps
        return ro

    def close(self):
        self.net.close(); self.tnet.close(); self.eng.close(); self.twin.close()


def _read(eng, net, steps):
    ro = {"acts": net.read_rollout("actions", (steps, B, 2)), "vals": net.read_rollout("values", (steps, B)),
          "rews": net.read_rollout("rewards", (steps, B)), "dones": net.read_rollout("dones", (steps, E), np.uint8),
          "yy": net.read_rollout("y", (steps, B)), "adv": net.read_rollout("adv", (steps, B)), "boot": net.read_rollout("boot", (B,))}
    for k, name, inner in OBS:
        ro[k] = net.read_rollout(name, (steps, E) + inner, np.uint8)
    ro["state"] = {f: eng.get_state(f) for f in STATE_FIELDS}
    ro["recs"] = eng.episodes_read()
    ro["running"] = eng.episodes_running()
    return ro


def _envs(bad, per_env=1):
    """Envs behind a mismatch mask over envs, or over agent-samples (per_env = 10)."""
    bad = np.asarray(bad).reshape(-1)
    return np.unique(np.flatnonzero(bad) // per_env)


def _records_differ(a, b):
    if len(a) != len(b):
        return np.arange(E)
    bad = np.zeros(len(a), bool)
    for k in ("step_index", "env", "length", "total_reward"):
        bad |= a[k] != b[k]
    return np.unique(np.concatenate([a["env"][bad], b["env"][bad]])) if bad.any() else np.empty(0, np.int64)


def replay(ro, twin, tnet, schedule, figures=None):
    """Steps the twin through the rollout `ro` (Pair.rollout) and compares.  Returns None, or the first mismatch
    (t, field, envs): t = T for what is compared behind the last step.  schedule: (>= t0 + T, E) ends the CPU expects."""
    steps = ro["dones"].shape[0]
    layout, t0 = ro["layout"], ro["t0"]
    env, agent = np.arange(E), np.arange(10)
    for t in range(steps):
        # 1. the observation the rollout recorded is the env's
        for k, name, _ in OBS:
            bad = (twin.read(name) != ro[k][t]).reshape(E, -1).any(axis=1)
            if bad.any():
                return t, name, _envs(bad)
        # 2. the stored values are the net's on that observation
        pred = tnet.predict_obs(ro["lb"][t], ro["ab"][t], ro["ps"][t])
        bad = ~(pred["vs"] == ro["vals"][t])
        if bad.any():
            return t, "values", _envs(bad, 10)
        # 3. a = mu + sigma * N(0, 1) of block (seed, env + offset, counter0 + t, RS_ACTION = 16, agent)
        e0, e1 = O.normal_pair(O.rng_block(SEED, env[:, None] + OFF, ro["counter0"] + t, 16, agent[None]))
        eps = np.stack([e0, e1], axis=-1).reshape(B, 2)
        want = pred["mu"].astype(np.float64) + pred["sigma"].astype(np.float64) * eps
        err, bound = np.abs(ro["acts"][t] - want), ACT_ATOL + ACT_RTOL * np.abs(want)
        if figures is not None:
            figures["action_err"] = max(figures.get("action_err", 0.0), float(err.max()))
            figures["action_err_of_bound"] = max(figures.get("action_err_of_bound", 0.0), float((err / bound).max()))
        bad = ~(err <= bound)
        if bad.any():
            return t, "actions", _envs(bad.any(axis=1), 10)
        # 4. the env steps with the norm-clipped action (the same three float32 statements in sample_actions_kernel and
        # transform_kernel): reward, done
        twin.step(twin.transform_actions(ro["acts"][t].reshape(E, 10, 2)))
        rew = twin.read("reward")
        if layout == 0:
            bad = ~(ro["rews"][t].reshape(E, 10) == rew[:, None]).all(axis=1)
        else:
            bad = ~(ro["rews"][t, :E] == rew)
            tail = ro["rews"][t, E:] != 0
            if not bad.any() and tail.any():
                return t, "rewards_behind_E", E + np.flatnonzero(tail)      # columns, not envs: quirk Q4 leaves them at zero
        if bad.any():
            return t, "rewards", _envs(bad)
        bad = twin.read("done") != ro["dones"][t]
        if bad.any():
            return t, "dones", _envs(bad)
        bad = ro["dones"][t].astype(bool) != schedule[t0 + t]
        if bad.any():
            return t, "dones_schedule", _envs(bad)
    # behind the last step
    for f in STATE_FIELDS:
        bad = (twin.get_state(f) != ro["state"][f]).reshape(E, -1).any(axis=1)
        if bad.any():
            return steps, f, _envs(bad)
    bad = ro["state"]["EPISODE"] != 1 + schedule[:t0 + steps].sum(axis=0)
    if bad.any():
        return steps, "EPISODE_schedule", _envs(bad)
    bad = ~(tnet.predict()["vs"] == ro["boot"])
    if bad.any():
        return steps, "boot", _envs(bad, 10)
    recs = twin.episodes_read()
    if len(recs) != int(schedule[t0:t0 + steps].sum()):
        return steps, "records_count", np.arange(E)
    bad = _records_differ(ro["recs"], recs)
    if len(bad):
        return steps, "records", bad
    rt, rl = twin.episodes_running()
    bad = ~(rt == ro["running"][0]) | (rl != ro["running"][1])
    if bad.any():
        return steps, "running", _envs(bad)
    # the reference's grid loop does not mask (paac.py:360-372): pinned with ends present
    oy, oadv = O.nstep_returns(ro["rews"].astype(np.float64), ro["vals"], ro["boot"], 0.99)
    bad = ~(np.abs(ro["yy"] - oy) <= 1e-4 + 1e-5 * np.abs(oy)).all(axis=0)
    if bad.any():
        return steps, "y", _envs(bad, 10)
    bad = ~(np.abs(ro["adv"] - oadv / 1000.0) <= 1e-6 + 1e-5 * np.abs(oadv / 1000.0)).all(axis=0)
    if bad.any():
        return steps, "adv", _envs(bad, 10)
    return None


def _where(mismatch, lanes):
    """(t, field, envs) with the chunks and lanes of the envs, for the assertion message."""
    if mismatch is None:
        return None
    t, field, envs = mismatch
    return dict(t=t, field=field, envs=[int(e) for e in envs], chunks=sorted({int(e) // CE for e in envs if e < E}),
                lanes=sorted({(int(e) // CE) % lanes for e in envs if e < E}))


def _first_difference(ro, ref, keys, lanes):
    """First stored array, step, env, chunk and lane at which two rollouts part (None: bit-equal in all of keys)."""
    for k in keys:
        if np.array_equal(ro[k], ref[k]):
            continue
        if k == "boot":
            envs = _envs(ro[k] != ref[k], 10)
            return dict(field=k, t=T, env=int(envs[0]), chunk=int(envs[0]) // CE, lane=(int(envs[0]) // CE) % lanes)
        bad = (ro[k] != ref[k]).reshape(ro[k].shape[0], -1)
        t = int(np.flatnonzero(bad.any(axis=1))[0])
        e = int(np.flatnonzero(bad[t])[0] // (bad.shape[1] // E))
        return dict(field=k, t=t, env=e, chunk=e // CE, lane=(e // CE) % lanes)
    return None


_a_first = {}


def _case_a_first_rollout(monkeypatch):
    """Case A's first rollout (flags 0, four lanes, layout 0), computed once, shared and left unchanged."""
    if not _a_first:
        pair = Pair(monkeypatch=monkeypatch)
        _a_first.update(pair.rollout(T, 0))
        pair.close()
    return _a_first


def _assert_scenario(ro):
    st = SC.chunk_end_stats(ro["dones"], CE, SC.REPLAY_LANES)
    assert min(st["mixed"]) >= 0.7 and st["per_step"].min() >= 1 and st["shared"] >= 15, st


def test_case_a_four_lanes_chained_rollouts_and_gradient(monkeypatch):
    """A: flags 0, four lanes, layout 0.  Two chained rollouts on one engine and net with the twin carried on -- the TimeLimit and
    episode counters, the R6 running sums and the action counter (1020 at the second rollout) carry over --, then a third of 4
    steps, so the rollout length changes on the same buffers, and its gradient against NN.conv_loss_and_grads on the stored
    observations, actions, adv and y (bounds of tests/test_gpu_net_tiles.py unchanged): the resident slots of a six-chunk step
    with a 20-sample last chunk behind in-rollout resets.
    keep_info()['slots'] is what the last (re)allocation of the rollout buffers chose (include/goldsrl_net.h): the buffers of
    the 20-step rollouts are kept for the 4-step one (ensure_rollout_bufs: net->T >= T), so it reads 20 * 6 here, of which the
    4-step rollout fills and the gradient step reads slots t * 6 + c < 4 * 6."""
    wall = time.perf_counter()
    pair = Pair(monkeypatch=monkeypatch)
    figures = {}
    for u in range(SC.REPLAY_ROLLOUTS):
        ro = pair.rollout(T, 0)
        assert ro["counter0"] == SC.REPLAY_COUNTER0 + u * T
        bad = replay(ro, pair.twin, pair.tnet, SCHEDULE, figures)
        assert bad is None, ("rollout %d" % u, _where(bad, SC.REPLAY_LANES))
        if u == 0:
            _assert_scenario(ro)
            if not _a_first:
                _a_first.update(ro)      # this is the rollout cases B and C compare with
            for k in STORED + ("rews", "yy", "adv"):      # a fresh engine and net from the same seeds store the same rollout
                assert np.array_equal(ro[k], _a_first[k]), k
    print("case A: worst action error %.2e, %.3f of its bound (rtol %g, atol %g)"
          % (figures["action_err"], figures["action_err_of_bound"], ACT_RTOL, ACT_ATOL))
    # the gradient leg
    G = SC.REPLAY_GRAD_T
    ro = pair.rollout(G, 0)
    assert ro["dones"].sum() >= 10
    bad = replay(ro, pair.twin, pair.tnet, SCHEDULE, figures)
    assert bad is None, ("gradient rollout", _where(bad, SC.REPLAY_LANES))
    st = pair.net.train_rollout_grads()
    grads, info = pair.net.get_grads(), pair.net.keep_info()
    nchunks = (E + CE - 1) // CE
    assert nchunks == 6 and info["resident"] and info["slots"] == T * nchunks and G * nchunks <= info["slots"], info
    _, p = _biased_params(PARAM_SEED)
    states = np.concatenate([_states(ro["lb"][t], ro["ab"][t], ro["ps"][t]) for t in range(G)])
    assert states.shape[0] == G * B == 1480
    acts, adv, yy = ro["acts"].reshape(-1, 2), ro["adv"].reshape(-1), ro["yy"].reshape(-1)
    loss, _, _, g, _ = NN.conv_loss_and_grads(p, states, acts.astype(np.float64), adv.astype(np.float64), yy.astype(np.float64), 0.02, 1000.0)
    np.testing.assert_allclose(st["loss"], loss, rtol=1e-4)
    _check_grads(grads, g, p, states, acts, adv, yy, tag="replay-A")
    pair.close()
    print("case A: wall %.1f s" % (time.perf_counter() - wall))


@pytest.mark.parametrize("case", ["B_single_stream_layout1", "C_three_lanes", "D_per_agent_trunk", "E_one_chunk"])
def test_replay_in_other_forms_of_the_rollout(case, monkeypatch):
    """B: GRL_NET_F_SINGLE_STREAM, reward layout 1 (column e of the first E, zeros behind).  C: six chunks over three lanes.  Both
         must store A's first rollout bit for bit (B: observations, actions, values, dones, boot; C: everything): lanes change the
         timeline and nothing else.
    D: GRL_NET_F_PER_AGENT_TRUNK -- its values differ from A's by rounding, so its trajectory is its own: the replay alone.
    E: one chunk of 37 envs (max_chunk_samples = 370), the side_now = (nchunks == 1) form of the rollout."""
    wall = time.perf_counter()
    kw = {"B_single_stream_layout1": dict(flags=F_SINGLE_STREAM), "C_three_lanes": dict(lanes=3),
          "D_per_agent_trunk": dict(flags=F_PER_AGENT_TRUNK), "E_one_chunk": dict(chunk=B)}[case]
    layout = 1 if case[0] == "B" else 0
    lanes = 1 if case[0] == "B" else kw.get("lanes", SC.REPLAY_LANES)
    ref = _case_a_first_rollout(monkeypatch) if case[0] in "BC" else None      # before this case's environment is set
    pair = Pair(monkeypatch=monkeypatch, **kw)
    ro = pair.rollout(T, layout)
    figures = {}
    bad = replay(ro, pair.twin, pair.tnet, SCHEDULE, figures)
    assert bad is None, (case, _where(bad, lanes))
    _assert_scenario(ro)
    if ref is not None:
        keys = STORED if case[0] == "B" else STORED + ("rews", "yy", "adv")
        diff = _first_difference(ro, ref, keys, lanes)
        print("case %s: stored rollout %s case A's first" % (case[0], "is bit-equal to" if diff is None else "DIFFERS from"))
        assert diff is None, (case, diff)
        assert _records_differ(ro["recs"], ref["recs"]).size == 0 and np.array_equal(ro["running"][0], ref["running"][0])
    if case[0] == "E":
        info, rng = pair.net.keep_info(), pair.net.range_info()
        print("case E: keep_info %s, stayed on the fp16 form: %s (%s)" % (info, not rng["gemm_f32"], rng))
    pair.close()
    print("case %s: worst action error %.2e, %.3f of its bound; wall %.1f s"
          % (case[0], figures["action_err"], figures["action_err_of_bound"], time.perf_counter() - wall))


def test_replay_catches_a_twin_whose_time_limit_counter_is_off_by_one(monkeypatch):
    """Negative control, host side only: case A's first rollout against a twin whose ELAPSED is one less for env 23.  The twin is
    stepped with the recorded actions exactly as the matched one is; the replay must stop at the first end that either the
    rollout or the twin schedules for env 23, on `dones`, naming that env and no other."""
    ro = _case_a_first_rollout(monkeypatch)
    e = SC.REPLAY_NEG_ENV
    off = EL0.copy()
    off[e] -= 1
    own, other = SCHEDULE[:T, e], SC.timelimit_dones(off, T)[:, e]
    t_first = int(np.flatnonzero(own | other)[0])
    assert own[t_first] != other[t_first]
    for k in ("GRL_NET_LANES", "GRL_NET_KEEP_LEVEL", "GRL_NET_KEEP_FREE_MB"):
        monkeypatch.delenv(k, raising=False)
    twin = _engine(off)
    tnet = _net(twin, 0, SC.REPLAY_CHUNK_SAMPLES)
    bad = replay(ro, twin, tnet, SCHEDULE)
    tnet.close(); twin.close()
    assert bad is not None
    t, field, envs = bad
    assert (t, field, list(envs)) == (t_first, "dones", [e]), bad
