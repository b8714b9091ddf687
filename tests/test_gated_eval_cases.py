"""CPU: the scenario of tests/test_gpu_gated_eval.py has the properties the GPU test leans on -- from the oracles alone
(tests/_gated_oracle.py, oracle/ticker.py), no device."""
import numpy as np

import _async_scenarios as SC
import _gated_eval_cases as GC
from test_gpu_gatednet import _params


def test_staggered_ends_are_mixed_whatever_the_policy_does():
    el = SC.staggered_elapsed(GC.E)
    length = GC.CAP - el
    assert length.min() == 1 and length.max() == GC.CAP
    first = np.arange(GC.CAP)[:, None] + 1 == length[None]            # each env's one done, on its own last step
    assert SC.mixed_share(first) >= 0.25


def test_parameter_seed_keeps_the_oracles_choices_clear_of_ties():
    """The float64 oracle's own greedy episodes of the scenario: the two largest probabilities of every (step, env, asset) differ by
    ten times the margin under which the GPU test would not hold the device's choice to the oracle's argmax."""
    el = SC.staggered_elapsed(GC.E)
    length, gap = GC.oracle_greedy_episodes(_params(GC.PSEED), GC.matrix(), GC.starts(), el)
    assert np.array_equal(length, GC.CAP - el)
    print("smallest top-two gap %.4g" % gap)
    assert gap >= GC.PSEED_MIN_GAP > GC.MARGIN


def test_greedy_pick_takes_the_first_of_tied_probabilities():
    probs = np.array([[[0.4, 0.4, 0.2], [0.2, 0.4, 0.4]], [[1 / 3, 1 / 3, 1 / 3], [0.1, 0.2, 0.7]]], np.float32)
    mu = np.arange(12, dtype=np.float32).reshape(2, 2, 3) - 5
    ch, raw, frac = GC.greedy_pick(probs, mu)
    assert ch.tolist() == [[0, 1], [0, 2]] and ch.dtype == np.int32
    assert raw.tolist() == [[-5.0, -1.0], [1.0, 6.0]]
    assert np.array_equal(frac, (1.0 / (1.0 + np.exp(-raw.astype(np.float64)))).astype(np.float32))
