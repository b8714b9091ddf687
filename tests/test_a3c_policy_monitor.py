"""CPU: goldsrl/agents/a3c/policy_monitor.py's aggregation and JSON log with a stub evaluation net -- env 0 goes to the
reference's two keys (fed_gym/agents/a3c/policy_monitor.py:110-118), mean and std over the envs to the new ones."""
import json

import numpy as np
import pytest

from goldsrl.agents.a3c.policy_monitor import PolicyMonitor, make_eval_engine


class _Eng(object):
    def __init__(self, E):
        self.E, self.resets = E, 0

    def reset(self):
        self.resets += 1


class _Net(object):
    """canned evaluations: call i returns totals[i], lengths[i] and a rewards trace whose env-0 column sums to nothing in particular"""

    def __init__(self, totals, lengths, R=5):
        self.eng = _Eng(len(totals[0]))
        self.totals, self.lengths, self.R = totals, lengths, R
        self.calls, self.params = [], []

    def set_params(self, p):
        self.params.append(np.asarray(p).copy())

    def eval(self, max_steps, trace_steps=0, trace_fields=()):
        i = len(self.calls)
        self.calls.append((max_steps, trace_steps, tuple(trace_fields), self.eng.resets, len(self.params)))
        ln = np.asarray(self.lengths[i], np.int32)
        S = min(trace_steps, int(ln.max()))
        rewards = (np.arange(S, dtype=np.float32)[:, None] + 1) * (np.arange(len(ln), dtype=np.float32)[None] + 1)
        return {"total_reward": np.asarray(self.totals[i], np.float64), "length": ln, "finished": np.ones(len(ln), np.uint8),
                "rewards": rewards}


class _Writer(object):
    def __init__(self):
        self.scalars, self.flushes = [], 0

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, value, step))

    def flush(self):
        self.flushes += 1


class _Coord(object):
    def __init__(self, n):
        self.n = n

    def should_stop(self):
        self.n -= 1
        return self.n < 0


TOTALS = [[1.0, 2.0, 6.0], [-3.0, 0.0, 9.0]]
LENGTHS = [[4, 7, 2], [3, 3, 5]]


def test_eval_once_aggregates_and_logs(tmp_path):
    net, w = _Net(TOTALS, LENGTHS), _Writer()
    mon = PolicyMonitor("Solow-1-1-finite-eval-v0", summary_writer=w, net=net, max_episode_steps=16)
    assert mon.n_envs == 3
    total, length, rewards = mon.eval_once(np.arange(4.0), max_sequence_length=5)
    # parameters copied, then the reset, then the evaluation over the cap with the rewards trace only
    assert net.calls == [(16, 16, ("rewards",), 1, 1)] and np.array_equal(net.params[0], np.arange(4.0))
    assert (total, length) == (1.0, 4) and rewards == [1.0, 2.0, 3.0, 4.0]          # env 0, cut at its own end
    assert np.array_equal(mon.total_rewards, TOTALS[0]) and np.array_equal(mon.episode_lengths, LENGTHS[0])
    mon.write_scalars(10)
    total, length, rewards = mon.eval_once(np.zeros(4))
    assert (total, length) == (-3.0, 3) and len(rewards) == 3 and net.calls[1][3:] == (2, 2)
    assert np.array_equal(mon.total_rewards, TOTALS[1])
    mon.write_scalars(12)
    path = tmp_path / "log.json"
    mon.write_log(str(path))
    log = json.load(open(path))
    assert set(log) == {"total_reward", "episode_length", "mean_total_reward", "std_total_reward", "n_envs"}
    assert log["total_reward"] == [1.0, -3.0] and log["episode_length"] == [4, 3] and log["n_envs"] == 3
    np.testing.assert_allclose(log["mean_total_reward"], [3.0, 2.0])
    np.testing.assert_allclose(log["std_total_reward"], [np.std(TOTALS[0]), np.std(TOTALS[1])])
    assert w.scalars == [("eval/total_reward", 1.0, 10), ("eval/episode_length", 4, 10), ("eval/mean_total_reward", 3.0, 10),
                         ("eval/total_reward", -3.0, 12), ("eval/episode_length", 3, 12), ("eval/mean_total_reward", 2.0, 12)]
    with pytest.raises(ValueError):
        mon.eval_once(np.zeros(4), max_sequence_length=20)                          # the net was built with R = 5
    mon.close()
    assert net.eng.resets == 2                                                      # a net handed in is not the monitor's to close


def test_continuous_eval_writes_the_log_every_time(tmp_path):
    net = _Net(TOTALS, LENGTHS)
    mon = PolicyMonitor("TradeAR1-v0", net=net)
    path = tmp_path / "TradeAR1.json"
    seen = []

    def params():
        if path.exists():
            seen.append(json.load(open(path))["total_reward"])
        return np.zeros(2)
    mon.continuous_eval(0, params, _Coord(2), total_reward_log_file=str(path))
    assert seen == [[1.0]] and json.load(open(path))["total_reward"] == [1.0, -3.0]
    assert [c[0] for c in net.calls] == [1024, 1024]


def test_unknown_registration_is_refused():
    with pytest.raises(ValueError):
        make_eval_engine("Ticker-v0", 4)
