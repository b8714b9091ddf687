"""CPU: tests/_flat_windows.py, the numpy restatement of the flat net's true history window, against the two places the repository
already states the rule -- _gauss_oracle.replay_windows (fresh episodes) and the window list SolowPolicyMonitor.eval_once builds --
and the conditions on the INPUTS of tests/test_gpu_flat_true_window.py: its scenarios, under the oracle envs alone, reach every
window length, slide, carry rows over a rollout boundary and end episodes on a rollout's last step."""
import numpy as np
import pytest

import _async_scenarios as SC
import _flat_windows as FW
import _gauss_oracle as GO


def _random_rollout(seed, T, E, D, p_done):
    rng = np.random.RandomState(seed)
    return rng.normal(size=(T, E, D)).astype(np.float32), rng.uniform(size=(T, E)) < p_done


@pytest.mark.parametrize("R,D", [(5, 2), (4, 7), (20, 33), (1, 3)])
def test_replay_equals_the_gauss_oracle_on_fresh_episodes(R, D):
    states, dones = _random_rollout(R + D, 23, 9, D, 0.15)
    win, length, _ = FW.replay(states, dones, R)
    ref, wts = GO.replay_windows(states, dones, R)
    assert np.array_equal(win, ref)
    assert np.array_equal(length >= R, wts > 0)
    # the length is the number of rows, and (states without a zero row) the number of non-zero rows: true_length
    assert np.array_equal(length, (np.abs(win).max(axis=3) > 0).sum(axis=2))
    assert length.min() == 1 and length.max() == min(R, 23)


@pytest.mark.parametrize("R,T", [(5, 3), (5, 20), (4, 1), (20, 7)])
def test_rows_are_carried_across_rollout_boundaries(R, T):
    """Consecutive rollouts of T steps equal one long rollout cut into pieces -- T < R - 1 (the carry is a shift) included."""
    n = 6
    states, dones = _random_rollout(R * T, n * T, 11, 3, 0.1)
    whole, wl, _ = FW.replay(states, dones, R)
    parts = FW.replay_chain([states[i * T:(i + 1) * T] for i in range(n)], [dones[i * T:(i + 1) * T] for i in range(n)], R)
    assert np.array_equal(np.concatenate([w for w, _ in parts]), whole)
    assert np.array_equal(np.concatenate([l for _, l in parts]), wl)
    # an env the host reset between two rollouts starts at length 1
    idx = [0, 7]
    parts = FW.replay_chain([states[:T], states[T:2 * T]], [dones[:T], dones[T:2 * T]], R, reset_between=[idx])
    assert (parts[1][1][0, idx] == 1).all()
    assert np.array_equal(parts[1][0][0, idx, 0], states[T, idx])


def test_replay_equals_the_window_list_of_the_solow_monitor():
    """SolowPolicyMonitor.eval_once over a scripted 12-step episode: the (1, rnn, 2) window it hands the estimator at every step."""
    from goldsrl.agents.paac.policy_monitor import SolowPolicyMonitor
    from goldsrl.agents.state_processors import SolowStateProcessor
    steps, R = 12, 5
    rng = np.random.RandomState(5)
    raw = np.stack([rng.uniform(50, 150, size=steps + 1), rng.normal(size=steps + 1)], axis=1)

    class Scripted(object):
        def __init__(self):
            self.t = 0

        def reset(self):
            self.t = 0
            return raw[0]

        def step(self, action):
            self.t += 1
            return raw[self.t], 1.0, self.t >= steps, {}

    seen = []
    mon = object.__new__(SolowPolicyMonitor)
    mon.env, mon.state_processor, mon.summary_writer, mon.learner = Scripted(), SolowStateProcessor(), None, None
    mon.copy_params = lambda: 0
    mon.get_action_from_policy = lambda processed, window, positions, sess=None: seen.append((processed.copy(), window.copy())) or 0.5
    total, length, _ = mon.eval_once(max_sequence_length=R)
    assert length == steps and len(seen) == steps
    states = np.stack([s[0] for s, _ in seen]).astype(np.float32)[:, None, :]       # (T, 1, 2) processed
    dones = np.zeros((steps, 1), bool); dones[-1] = True
    win, wl, _ = FW.replay(states, dones, R)
    assert np.array_equal(win[:, 0], np.concatenate([w for _, w in seen]))
    assert wl[:, 0].tolist() == [min(t + 1, R) for t in range(steps)]


def test_the_scenarios_exercise_every_edge():
    """Oracle envs alone (as tests/test_async_scenarios.py): window lengths 1..R all occur, some window slides, some window carries
    rows over a rollout boundary, some done falls on the last step of a rollout."""
    got = {}
    for name, c in FW.SCENARIOS.items():
        dones = FW.oracle_dones(name)
        assert len(dones) == c["rollouts"] and dones[0].shape == (c["T"], SC.E)
        states = [np.ones((c["T"], SC.E, 1), np.float32) for _ in dones]
        parts = FW.replay_chain(states, dones, c["R"])
        got[name] = FW.edges([l for _, l in parts], dones, c["R"])
        print(name, got[name])
        assert got[name]["carried"], name
    assert got["solow"]["lengths"] == set(range(1, 6)) and got["solow"]["slides"] and got["solow"]["last_done"]
    assert got["trade3"]["lengths"] == set(range(1, 5)) and got["trade3"]["slides"]
    assert got["trade16"]["lengths"] == set(range(1, 17)) and not got["trade16"]["slides"]      # never fills: R = 20 > cap
    assert got["solow_short"]["lengths"] == set(range(1, 6)) and got["solow_short"]["last_done"] and got["solow_short"]["slides"]
