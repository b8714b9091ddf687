#!/usr/bin/env python3
"""Golden vectors of the A3C savings-grid worker's acting, window and update rules, captured from the UNMODIFIED reference
(read-only) under the gym/tensorflow stand-ins of _ref_stubs.py:

  * GaussianWorker.run_n_steps                            (fed_gym/agents/a3c/worker.py:191-221)
  * GridSolowWorker.get_action_from_policy                 (worker.py:360-368)
  * GridSolowWorker.get_random_action / transform_raw_action, idx_to_grid (worker.py:349, 374-379) and
    GaussianWorker.get_random_discrete_action              (:223-227)
  * GaussianWorker.update (worker.py:241-325) + GridSolowWorker.fill_feed_dict_for_update (:381-391), gae_discount (scipy's lfilter)
  * SolowStateProcessor                                  (fed_gym/agents/state_processors.py:69-77)
  * SolowEnv under the TimeLimit stand-in                (fed_gym/envs/fed_env.py:161-250)

The worker is made with object.__new__(GridSolowWorker): __init__ builds TF graphs, which the stand-ins cannot; idx_to_grid is set as
its __init__ does (:349).  Its nets are inert objects whose outputs are CANNED: the policy answers float32 probs of shape (1,1,K), a
fixed function of (state, history), the value net another one, so the rules are captured independently of any network.
np.random.rand answers recorded uniforms for the duration of run_n_steps, so the draw rule is captured independently of the
generator.  The fake session records the feed dict of
the update's session.run.  tf.keras' pad_sequences does not exist under the stand-ins: the worker module's `tf` is handed the
Keras 2.0.8 restatement that gen_golden_learner.py carries (parity unpinned at that call, as DESIGN section 4 says of it).

The value net's canned answers are float32, as a TF float32 graph's are.  Under the numpy of the capture (NEP 50) the worker's
product discount_factor * V_st[t + 1] is then rounded to float32, where numpy 1.13 keeps float64; tests/test_oracle_gauss.py bounds the
feed by that one rounding.

Four cases (t_max = 16, max_seq_length = 5): always_bootstrap on / off on the 1 024-step env, and on / off with
max_episode_steps = 9, where the episode ends inside the t_max steps -- each at K = 51 (GridSolowWorker's n_grid) and at K = 3 (the
reference test's size), scale 1 (GridSolowWorker's default).

Run in the build container only:   python tests/golden/gen_golden_grid.py
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_stubs  # noqa: E402

_ref_stubs.install()

import gym  # noqa: E402  (the stand-in)
from gen_golden_learner import pad_sequences  # noqa: E402
from fed_gym.agents.state_processors import SolowStateProcessor  # noqa: E402
from fed_gym.agents.a3c import worker as a3c_worker  # noqa: E402
from fed_gym.envs.fed_env import SolowEnv  # noqa: E402

a3c_worker.tf.keras.preprocessing.sequence.pad_sequences = pad_sequences

T_MAX, R = 16, 5


class Key(object):
    def __init__(self, name):
        self.name = name


LB, UB = 0.01, 0.99


def canned_policy(state, history, K):
    """probs (1,1,K) as float32 (what a TF float32 graph hands back), a fixed function of the inputs"""
    h = np.asarray(history, np.float64)
    z = 1.5 * np.sin(np.arange(K) * (0.7 + 3.0 * state[0]) + 5.0 * state[1]) + 0.3 * h.shape[0] * np.cos(np.arange(K)) + h[:, 1].sum()
    e = np.exp(z - z.max())
    return (e / e.sum()).astype(np.float32).reshape(1, 1, K)


def canned_value(states, history):
    s, h = np.asarray(states, np.float64), np.asarray(history, np.float64)
    return (1.0 * (0.3 * np.cos(23.0 * s[:, 0]) + s[:, 1] + 0.07 * h[:, :, 0].sum(1) + 0.01 * (np.abs(h).max(2) > 0).sum(1))).astype(np.float32)


class FakePolicy(object):
    num_outputs = 1

    def __init__(self, log, K):
        for k in ("states", "history", "advantages", "actions", "predictions", "loss", "summaries"):
            setattr(self, k, Key("policy/" + k))
        self.log, self.num_choices = log, K

    def predict(self, state, history, sess, batch=False):
        probs = canned_policy(state, history, self.num_choices)
        self.log.append((np.array(state), np.array(history), probs[0, 0].copy()))
        return {"probs": probs}


class FakeValue(object):
    def __init__(self):
        for k in ("states", "history", "targets", "predictions", "loss", "summaries"):
            setattr(self, k, Key("value/" + k))


class FakeSession(object):
    def __init__(self, w):
        self.w, self.feed, self.value_calls = w, None, []

    def run(self, fetches, feed_dict=None):
        w = self.w
        if fetches is w.value_net.predictions:
            s, h = np.asarray(feed_dict[w.value_net.states]), np.asarray(feed_dict[w.value_net.history])
            v = canned_value(s, h)
            self.value_calls.append((s.copy(), h.copy(), v.copy()))
            return {"logits": v}
        self.feed = {k.name: np.array(v) for k, v in feed_dict.items()}
        return (None, 0, 0.0, 0.0, None, None, None, None)


def capture(always_bootstrap, max_episode_steps, seed, K):
    env = gym.wrappers.TimeLimit(SolowEnv(p=1, q=1), max_episode_steps=max_episode_steps)
    stepped = []
    inner_step = env.step

    def step(action):
        stepped.append(action)
        return inner_step(action)
    env.step = step
    w = object.__new__(a3c_worker.GridSolowWorker)
    log = []
    w.name, w.discount_factor, w._lambda, w.scale = "worker_0", 0.99, 0.96, 1.0
    w.idx_to_grid = {idx: v for idx, v in zip(range(K), np.linspace(LB, UB, K))}      # GridSolowWorker.__init__ (:349)
    w.state_processor = SolowStateProcessor()
    w.env, w.summary_writer, w.max_global_steps = env, None, None
    w.policy_net = w.global_policy_net = FakePolicy(log, K)
    w.value_net = w.global_value_net = FakeValue()
    w.global_step, w.pnet_train_op, w.vnet_train_op = Key("global_step"), Key("pnet_train_op"), Key("vnet_train_op")
    w.local_counter, w.global_counter = itertools.count(), itertools.count()
    w.history, w.debug = [], None
    sess = FakeSession(w)
    np.random.seed(seed)
    # GaussianWorker.run, lines 132-133, then one pass of its loop body (:141, :149-151)
    w.state = w.env.reset()
    w.history.append(w.state_processor.process_state(w.state))
    uniforms = np.random.RandomState(seed + 1).uniform(size=T_MAX + R)      # the first R - 1 steps record no transition
    it = iter(uniforms)
    saved = np.random.rand
    try:
        np.random.rand = lambda *shape: np.full(shape, next(it))
        transitions, local_t, global_t, debug, done = w.run_n_steps(T_MAX, sess, max_seq_length=R)
    finally:
        np.random.rand = saved
    w.update(transitions, sess, always_bootstrap=always_bootstrap, max_seq_length=R)
    steps = len(log)
    assert len(stepped) == steps
    # both estimators are fed the same states and history (fill_feed_dict_for_update)
    assert np.array_equal(sess.feed["value/states"], sess.feed["policy/states"])
    assert np.array_equal(sess.feed["value/history"], sess.feed["policy/history"])
    assert np.issubdtype(sess.feed["policy/actions"].dtype, np.integer)
    out = dict(
        steps=steps, done=bool(done), n_transitions=len(transitions),
        step_states=np.stack([l[0] for l in log]), step_probs=np.stack([l[2] for l in log]).astype(np.float32), uniforms=uniforms[:steps],
        step_hist=np.stack([np.concatenate([l[1], np.zeros((R - len(l[1]), 2))]) for l in log]),
        step_env_action=np.array(stepped, np.float64),                     # what env.step was called with, every step
        history=np.stack(w.history),
        tr_state=np.stack([t.state for t in transitions]), tr_choice=np.array([int(t.action[0][0]) for t in transitions], np.int64),
        tr_reward=np.array([t.reward for t in transitions], np.float64), tr_next=np.stack([t.next_state for t in transitions]),
        tr_done=np.array([t.done for t in transitions]),
        values=sess.value_calls[-1][2],
        boot_called=len(sess.value_calls) == 2,
        boot_state=sess.value_calls[0][0][0] if len(sess.value_calls) == 2 else np.zeros(2),
        boot_hist=sess.value_calls[0][1][0] if len(sess.value_calls) == 2 else np.zeros((R, 2)),
        boot_value=sess.value_calls[0][2][0] if len(sess.value_calls) == 2 else np.float32(0),
        feed_states=sess.feed["policy/states"], feed_history=sess.feed["policy/history"], feed_adv=sess.feed["policy/advantages"],
        feed_actions=sess.feed["policy/actions"].astype(np.int64), feed_targets=sess.feed["value/targets"],
    )
    return out


def main():
    cases = {"on": (True, 1024, 11), "off": (False, 1024, 12), "short_on": (True, 9, 13), "short_off": (False, 9, 14)}
    out = {}
    for K in (51, 3):
        for name, (ab, cap, seed) in cases.items():
            pre = "k%d_%s_" % (K, name)
            for k, v in capture(ab, cap, seed + K, K).items():
                out[pre + k] = np.asarray(v)
            print(pre, "steps", out[pre + "steps"], "transitions", out[pre + "n_transitions"], "done", out[pre + "done"],
                  "boot", out[pre + "boot_value"], "choices", out[pre + "tr_choice"].tolist())
    np.savez_compressed(os.path.join(HERE, "grid_worker.npz"), t_max=T_MAX, max_seq_length=R, scale=1.0, lb=LB, ub=UB, **out)
    print("wrote grid_worker.npz", os.path.getsize(os.path.join(HERE, "grid_worker.npz")), "bytes")


if __name__ == "__main__":
    main()
