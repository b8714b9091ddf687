"""CPU: the host form of the Swarm feedback rule (goldsrl/_ffi_swarmrules.py:swarm_rule_actions) against the fixture
tests/golden/swarm_rules.npz, which tests/golden/gen_golden_swarm_rules.py recorded on the unmodified reference SwarmEnv(seed=192)
with the rule written out a second time, scalar by scalar.  Both sides are the same numpy float64 statements, so the actions are
compared as bits; the rewards are the oracle's (oracle.oracle.swarm_step), held to the reference as
tests/test_oracle_golden.py:test_swarm_trajectory_time_limit_and_autoreset holds them: equal."""
import numpy as np
import pytest

from oracle import oracle as O


def test_rule_actions_and_oracle_steps_reproduce_the_fixture(golden):
    from goldsrl import _ffi_swarmrules as R
    from goldsrl.baselines import DEFAULT_SWARM_RULES, select_best_swarm_rule
    g = golden("swarm_rules")
    rules = g["rules"]
    n = len(rules)
    assert np.array_equal(rules, DEFAULT_SWARM_RULES)                    # the whole default set was recorded
    assert np.array_equal(R.swarm_rule_offsets(rules), g["offsets"])
    assert (g["length"] == 128).all()
    # every rule as one env of a batch: x (n, 80, 2), xa (n, 10, 2)
    x, xa = np.tile(g["x"], (n, 1, 1)), np.tile(g["xa"], (n, 1, 1))
    a_row, p_row = np.tile(g["agent_noise_row"], (n, 1, 1)), np.tile(g["particle_noise_row"], (n, 1, 1))
    rewards = np.zeros((n, 128))
    for t in range(128):
        act = np.stack([R.swarm_rule_actions(x[r], xa[r], rules[r], g["offsets"][r]) for r in range(n)])
        assert act.tobytes() == g["actions"][:, t].tobytes(), t
        x, xa, rew, done = O.swarm_step(x, xa, act, a_row, p_row)
        assert not done.any()
        rewards[:, t] = rew
    assert np.array_equal(rewards, g["rewards"])
    totals = np.array([np.sum(row) for row in rewards])
    assert np.array_equal(totals, g["total"])
    i, six, best = select_best_swarm_rule(rules, totals[None])
    assert i == int(g["best_index"]) and best == g["total"].max() and six == tuple(rules[i])
    assert g["total"][i] - g["total"][1] > 100                           # the best rule is far above hold
    # drift and hold are rows 0 and 1
    assert not g["actions"][0].any() and (g["actions"][1] == [-1.0, 0.0]).all()


def test_rule_actions_take_a_batch(golden):
    from goldsrl import _ffi_swarmrules as R
    g = golden("swarm_rules")
    rng = np.random.RandomState(4)
    x, xa = rng.rand(3, 2, 80, 2) * 3, rng.rand(3, 2, 10, 2) * 3
    for r in (5, 19):                                                    # a centroid rule and a nearest-locust rule
        got = R.swarm_rule_actions(x, xa, g["rules"][r], g["offsets"][r])
        assert got.shape == (3, 2, 10, 2)
        for i in range(3):
            for k in range(2):
                assert got[i, k].tobytes() == R.swarm_rule_actions(x[i, k], xa[i, k], g["rules"][r], g["offsets"][r]).tobytes()


def test_nearest_locust_takes_the_first_of_a_tie():
    from goldsrl import _ffi_swarmrules as R
    x = np.full((80, 2), 9.0)
    x[7], x[30] = (1.0, 0.0), (-1.0, 0.0)                                # both at distance 1 from the agents
    xa = np.zeros((10, 2))
    act = R.swarm_rule_actions(x, xa, (0.0, 0.25, 1.0), np.zeros((10, 2)))
    assert (act == [0.25, 0.0]).all()                                    # towards locust 7
    x[7], x[30] = x[30].copy(), x[7].copy()
    assert (R.swarm_rule_actions(x, xa, (0.0, 0.25, 1.0), np.zeros((10, 2))) == [-0.25, 0.0]).all()


def test_check_swarm_rules_refuses():
    from goldsrl import _ffi_swarmrules as R
    good = [(1, 5, 0, -1.5, 1.5, 0.7)]
    assert R.check_swarm_rules(good).shape == (1, 6) and R.check_swarm_rules(good).dtype == np.float64
    for bad in ([(1, 5, 0)], [1, 5, 0, 0, 0, 0], np.zeros((0, 6)), np.zeros((2, 3, 6))):
        with pytest.raises(ValueError):
            R.check_swarm_rules(bad)
    with pytest.raises(ValueError) as ei:
        R.check_swarm_rules([(1, 5, 0, 0, 0, 0), (1, 5, 2, 0, 0, 0)])
    assert "rule 1" in str(ei.value) and "anchor" in str(ei.value)
    with pytest.raises(ValueError) as ei:
        R.check_swarm_rules([(1, 5, 0, 0, np.nan, 0)])
    assert "off_y" in str(ei.value)
    with pytest.raises(ValueError):
        R.check_swarm_rules([(1, np.inf, 0, 0, 0, 0)])


def test_hold_row_is_exactly_minus_one_zero(golden):
    from goldsrl import _ffi_swarmrules as R
    from goldsrl.baselines import DEFAULT_SWARM_RULES
    g = golden("swarm_rules")
    off = R.swarm_rule_offsets(DEFAULT_SWARM_RULES)
    assert not off[0].any() and not off[1].any()
    hold = R.swarm_rule_actions(g["x"], g["xa"], DEFAULT_SWARM_RULES[1], off[1])
    assert hold.shape == (10, 2) and (hold[:, 0] == -1.0).all() and (hold[:, 1] == 0.0).all()
    assert not R.swarm_rule_actions(g["x"], g["xa"], DEFAULT_SWARM_RULES[0], off[0]).any()      # drift


def test_a_row_just_below_norm_one_is_left_alone():
    from goldsrl import _ffi_swarmrules as R
    x, xa = np.zeros((80, 2)), np.zeros((10, 2))                         # centroid (0, 0), every agent on it
    below = np.nextafter(1.0, 0.0)
    off = np.zeros((10, 2))
    off[:, 0] = [below, 1.0, 2.0, 0.5, -below, -1.0, 0.0, 0.0, 0.0, 0.0]
    off[:, 1] = [0.0, 0.0, 0.0, 0.5, 0.0, 0.0, below, 1.0, -3.0, 0.0]
    act = R.swarm_rule_actions(x, xa, (0.0, 1.0, 0.0), off)              # gain 1, no cancel: the raw action is the offset
    want = np.array([(below, 0), (1, 0), (1, 0), (0.5, 0.5), (-below, 0), (-1, 0), (0, below), (0, 1), (0, -1), (0, 0)])
    assert np.array_equal(act, want)
    assert act[0, 0] < 1.0 and act[4, 0] > -1.0                          # not normalised: d < 1
