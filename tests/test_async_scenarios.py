"""CPU: the scenarios of tests/_async_scenarios.py really do end episodes asynchronously.  Oracle alone, no GPU: these are
conditions on the INPUTS of tests/test_gpu_async_dones.py, so that a kernel which mishandles a mixed done mask cannot pass
there because the masks happened to be uniform.

  1. at least half of all (step, wave) pairs see a mixed done mask (some lanes done, not all);
  2. at least E depletion dones over the 20 steps;
  3. the oracle's min |assets' - 1| over the trajectory is >= 1e-6: the account is float64 on both sides, so the device and
     the oracle cannot disagree on `assets < 1` (libm differences are ten orders of magnitude smaller)."""
import numpy as np
import pytest

import _async_scenarios as SC


@pytest.mark.parametrize("n_env", [SC.E, SC.SWARM_E])
def test_staggered_timelimit_masks_are_mixed(n_env):
    el0 = SC.staggered_elapsed(n_env)
    assert el0.min() >= 0 and el0.max() < SC.CAP
    dones = SC.timelimit_dones(el0, SC.T)
    share = SC.mixed_share(dones)
    per_wave = [sorted(set(dones[:, w:w + SC.WAVE].sum(axis=1).tolist())) for w in range(0, n_env, SC.WAVE)]
    print("E=%d staggered TimeLimit(%d): mixed share %.2f, dones per (step, wave) %s" % (n_env, SC.CAP, share, per_wave))
    assert share >= 0.5
    # the set of finished lanes differs from wave to wave on the same step (full waves)
    full = [dones[:, w:w + SC.WAVE] for w in range(0, n_env - SC.WAVE + 1, SC.WAVE)]
    for a, b in zip(full, full[1:]):
        assert not np.array_equal(a, b)
    # every env ends at least twice within the T steps: what an env does AFTER its auto-reset is covered
    assert (dones.sum(axis=0) >= 2).all()
    # the same expression as a step-by-step TimeLimit counter
    el, ref = el0.astype(np.int64), np.zeros_like(dones)
    for t in range(SC.T):
        el = el + 1
        ref[t] = el >= SC.CAP
        el[ref[t]] = 0
    assert np.array_equal(ref, dones)


def test_conv_rollout_replay_scenario_scatters_ends_over_chunks_and_lanes():
    """Conditions on the input of tests/test_gpu_conv_rollout_replay.py: 37 envs in chunks of 7 over four lanes, staggered
    TimeLimit(9), 20 steps.  Each bound is a condition of the scenario; the figure computed for these constants is printed."""
    n, ce, nl = SC.REPLAY_E, SC.REPLAY_CHUNK_ENVS, SC.REPLAY_LANES
    bases = list(range(0, n, ce))
    assert ce == 7 and bases == [0, 7, 14, 21, 28, 35] and n - bases[-1] == 2      # six chunks, the last of 2 envs
    assert sum(b % 4 != 0 for b in bases[1:]) == 4                                 # bases that are no multiple of SWARM_EPB = 4
    assert [c % nl for c in range(len(bases))] == [0, 1, 2, 3, 0, 1]               # chunks 4 and 5 share lanes 0 and 1
    el0 = SC.staggered_elapsed(n, SC.CAP)
    assert el0.min() >= 0 and el0.max() < SC.CAP
    dones = SC.timelimit_dones(el0, SC.T)
    st = SC.chunk_end_stats(dones, ce, nl)
    print("replay scenario: mixed share per full chunk %s, ends per step %d..%d, ends per env %d..%d, steps on which two chunks of "
          "a lane both hold an end %d" % (["%.2f" % m for m in st["mixed"]], st["per_step"].min(), st["per_step"].max(),
                                          st["per_env"].min(), st["per_env"].max(), st["shared"]))
    assert len(st["mixed"]) == 5 and min(st["mixed"]) >= 0.7
    assert st["per_step"].min() >= 1
    assert st["per_env"].min() >= 2
    assert st["shared"] >= 15
    # the gradient leg: a rollout of 4 steps behind the two chained ones of 20 holds at least 10 ends
    t0 = SC.REPLAY_ROLLOUTS * SC.T
    later = SC.timelimit_dones(el0, t0 + SC.REPLAY_GRAD_T)
    assert np.array_equal(later[:SC.T], dones)
    assert later[t0:].sum() >= 10
    # the negative control's env: one count less on its TimeLimit counter moves its first end, and only its
    e = SC.REPLAY_NEG_ENV
    assert el0[e] >= 1
    off = el0.copy(); off[e] -= 1
    diff = SC.timelimit_dones(off, SC.T) != dones
    assert diff[:, e].any() and not np.delete(diff, e, axis=1).any()


@pytest.mark.parametrize("source", ["injected", "generator"])
@pytest.mark.parametrize("n", [2, 3, 16])
def test_trade_depletion_scenarios(n, source):
    kw = SC.TRADE_DEPLETION[n]
    acts, nrm = SC.trade_inputs(n, SC.TRADE_INPUT_SEED[n])
    if source == "generator":
        nrm = SC.trade_generator_normals(SC.GEN_SEED, SC.GEN_OFFSET, SC.E, SC.T, n)
    o = SC.trade_oracle(n, kw["trade_starting_balance"], kw["trade_std_p"], acts, nrm)
    share, dep = SC.mixed_share(o["done"]), int(o["own_done"].sum())
    print("TradeAR1 n=%d %s (seed %d): mixed share %.2f, depletion dones %d, min |assets' - 1| %.2e"
          % (n, source, SC.TRADE_INPUT_SEED[n], share, dep, o["gap"]))
    assert share >= 0.5
    assert dep >= SC.E
    assert o["gap"] >= SC.MIN_GAP
    assert np.array_equal(o["done"], o["own_done"])
    # envs keep playing (and deplete again) after their auto-reset
    assert (o["done"].sum(axis=0) >= 2).sum() >= SC.E // 4


def test_generator_normals_layout():
    """pairs = (n + 1) // 2 blocks per step, the even asset takes the first normal; an odd n leaves half of the last pair unused."""
    from oracle import oracle as O
    n, off = 3, SC.GEN_OFFSET
    z = SC.trade_generator_normals(SC.GEN_SEED, off, 5, 4, n)
    assert z.shape == (4, 5, 3)
    for t, e in ((0, 0), (3, 4), (2, 1)):
        b0 = O.normal_pair(O.rng_block(SC.GEN_SEED, e + off, 0, 12, t * 2 + 0))
        b1 = O.normal_pair(O.rng_block(SC.GEN_SEED, e + off, 0, 12, t * 2 + 1))
        assert z[t, e].tolist() == [float(b0[0]), float(b0[1]), float(b1[0])]
