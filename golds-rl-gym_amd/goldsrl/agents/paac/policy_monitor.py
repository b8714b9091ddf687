"""Eval monitors (reference fed_gym/agents/paac/policy_monitor.py:15-208) on the device engine.

Same classes, constructor arguments and return values: `eval_once` copies the learner's parameters into a local
estimator, plays ONE episode of the eval env (`Swarm-eval-v0`, seed 192 / a Solow eval env) with actions
a = mu + sigma * N(0,1) drawn from numpy's global generator as the reference does, writes the `eval/*` scalars and, for
Swarm, keeps the best episode's actions in `swarm-eval.json` ({'score', 'actions'}: the file
scripts/make_swarm_gif.py:62-82 replays).  What has no counterpart: the gym `Monitor` video wrapper, TF sessions and
summaries (scalars go to a JSON-lines file), and the Saver (use ActorLearner.save_checkpoint).  The eval env owns
its own 1-env engine handle, so a monitor may run beside the learner."""
import json
import logging
import os
import time

import numpy as np

from ...baselines import DEFAULT_SWARM_RULES
from ..a3c.policy_monitor import _DeviceMonitor
from .emulator_runner import SolowRunner, SwarmRunner
from .policy_v_network import ConvPolicyVFieldNetwork, ConvSingleAgentPolicyNetwork, FlatPolicyVNetwork


class ScalarWriter(object):
    """Stand-in for tf.summary.FileWriter: every scalar goes to <logdir>/scalars.jsonl (one JSON object per line) and to a
    TensorBoard event file (events.out.tfevents.*, written by goldsrl.utils_tfevents without TensorFlow)."""

    def __init__(self, logdir, tfevents=True):
        self.logdir = os.path.abspath(logdir)
        os.makedirs(self.logdir, exist_ok=True)
        self._f = open(os.path.join(self.logdir, "scalars.jsonl"), "a")
        self._ev = None
        if tfevents:
            from ...utils_tfevents import EventFileWriter
            self._ev = EventFileWriter(self.logdir)

    def get_logdir(self):
        return self.logdir

    def add_scalar(self, tag, value, step):
        now = time.time()
        self._f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step), "time": now}) + "\n")
        if self._ev is not None:
            self._ev.add_scalar(tag, value, step, wall_time=now)

    def flush(self):
        self._f.flush()
        if self._ev is not None:
            self._ev.flush()

    def close(self):
        self._f.close()
        if self._ev is not None:
            self._ev.close()


class PolicyMonitor(object):
    """policy_monitor.py:15-71.  `global_policy_net` is the learner's estimator object (bound to its engine);
    `learner` (optional) supplies global_step for the scalars."""

    def __init__(self, env, global_policy_net, state_processor, summary_writer, saver=None, network_conf=None, learner=None):
        self.env = env
        self.state_processor = state_processor
        self.global_policy_net = global_policy_net
        self.summary_writer = summary_writer
        self.saver = saver
        self.learner = learner
        self.best_score = -np.inf
        logdir = summary_writer.get_logdir() if summary_writer is not None else "."
        self.checkpoint_path = os.path.abspath(os.path.join(logdir, "../checkpoints/model"))
        self.actions_path = os.path.join(os.getcwd(), 'swarm-eval.json')
        self.policy_net = self._create_policy_estimator(network_conf)      # the "policy_eval" copy
        self._bind()

    def _bind(self):
        raise NotImplementedError

    def copy_params(self):
        """copy_params_op: global -> policy_eval"""
        self.policy_net.set_flat_params(self.global_policy_net.get_flat_params())
        return int(self.learner.global_step) if self.learner is not None else 0

    def get_action_from_policy(self, processed_state, history, positions, sess=None):
        predictions = self.policy_net.predict(processed_state, history)
        mu, sigma = predictions['mu'], predictions['sigma']
        return mu + sigma * np.random.normal(size=mu.shape)

    @staticmethod
    def _create_policy_estimator(conf):
        raise NotImplementedError

    def eval_once(self, sess=None, max_sequence_length=5):
        raise NotImplementedError

    def _play(self, first_state, choose_action):
        """One episode: `choose_action(state, t)` -> env action until the env reports done.  Returns the per-step rewards
        and the actions taken."""
        rewards, taken = [], []
        state, done = first_state, False
        while not done:
            action = choose_action(state, len(rewards))
            taken.append(action)
            state, reward, done, _ = self.env.step(action)
            rewards.append(reward)
        return rewards, taken

    def _summaries(self, global_step, total_reward, episode_length, rewards):
        if self.summary_writer is not None:
            self.summary_writer.add_scalar("eval/total_reward", total_reward, global_step)
            self.summary_writer.add_scalar("eval/episode_length", episode_length, global_step)
            self.summary_writer.flush()
        logging.info("Eval results at step {}: avg_reward {}, std_reward {}, episode_length {}".format(
            global_step, np.mean(rewards), np.std(rewards), episode_length))

    def continuous_eval(self, eval_every, sess=None, coord=None, max_seq_length=5):
        """Evaluates the policy every [eval_every] seconds until coord.should_stop()."""
        while coord is None or not coord.should_stop():
            self.eval_once(sess, max_sequence_length=max_seq_length)
            if coord is None:
                return
            time.sleep(eval_every)


class SolowPolicyMonitor(PolicyMonitor):
    """policy_monitor.py:74-124"""

    def _bind(self):
        self.policy_net.bind(self.env._eng, max_samples=64)

    def get_action_from_policy(self, processed_state, history, positions, sess=None):
        raw_actions = super().get_action_from_policy(processed_state, history, positions, sess)
        return SolowRunner.transform_actions_for_env(raw_actions)

    @staticmethod
    def _create_policy_estimator(conf):
        return FlatPolicyVNetwork(conf)

    def eval_once(self, sess=None, max_sequence_length=5):
        global_step = self.copy_params()
        window_rows = []       # processed states of the episode so far (the reference keeps the last 2*max_sequence_length)

        def choose(state, t):
            processed = self.state_processor.process_state(state)
            window_rows.append(np.array(processed))
            del window_rows[:-2 * max_sequence_length]
            # the estimator takes a fixed (1, rnn_length, 2) window; rows past the episode's start are zero
            # (dynamic_rnn's sequence_length = number of non-zero rows, a3c/estimators.py:11-15)
            window = np.zeros((1, max_sequence_length, len(processed)), np.float32)
            recent = window_rows[-max_sequence_length:]
            window[0, :len(recent)] = np.array(recent)
            return self.get_action_from_policy(np.array([processed]), window, None, sess)

        rewards, _ = self._play(self.env.reset(), choose)
        total_reward, episode_length = float(np.sum(rewards)), len(rewards)
        self._summaries(global_step, total_reward, episode_length, rewards)
        return total_reward, episode_length, rewards


class DeviceSolowPolicyMonitor(_DeviceMonitor):
    """SolowPolicyMonitor with the whole episode on the device: every episode of `n_envs` seeded envs of the eval registration
    `Solow-p-q-finite-eval-v0` (seed 1692, reseeded at every reset) in one kernel launch (grl_fnet_eval,
    include/goldsrl_flateval.h).  The streams are keyed by the global env id, so env 0 is the single episode the reference plays
    and envs 1.. are further seeded episodes of the same registration; `eval_once` returns env 0's (total_reward, episode_length,
    rewards) and keeps every env's totals and lengths.  Actions are drawn, a = mu + sigma * N(0,1), as the reference's monitor
    draws them (policy_monitor.py:45-49) -- from the device's action stream at counter 0, so every evaluation plays the same
    episodes with the same noise; greedy=True acts with mu.  The window is the rollout's (the current state repeated, the window
    the policy is trained under by default), not the true last-rnn states SolowPolicyMonitor feeds -- unless
    true_window=True: then the evaluation feeds those true last-rnn states of the episode, as SolowPolicyMonitor does (for a
    policy trained with FlatPolicyVNetwork.bind(true_window=True) / --true-history)."""

    def __init__(self, env, global_policy_net, state_processor=None, summary_writer=None, saver=None, network_conf=None, learner=None,
                 n_envs=1, rnn_length=5, device_id=0, max_episode_steps=1024, true_window=False):
        from ... import _ffi
        if not (env.startswith("Solow-") and env.endswith("-finite-eval-v0")):
            raise ValueError("no device evaluation for env %r (Solow-p-q-finite-eval-v0)" % (env,))
        if n_envs < 1:
            raise ValueError("n_envs must be at least 1")
        p, q = (int(v) for v in env.split("-")[1:3])
        self.env = env
        self.global_policy_net = global_policy_net
        self.state_processor = state_processor
        self.saver = saver
        self.learner = learner
        eng = _ffi.Engine(_ffi.ENV_SOLOW, int(n_envs), device_id=device_id, seed=1692, flags=_ffi.F_RESEED_EACH_RESET, solow_p=p, solow_q=q,
                          rnn_length=int(rnn_length), max_episode_steps=int(max_episode_steps))
        conf = network_conf if network_conf is not None else global_policy_net.conf
        self.policy_net = FlatPolicyVNetwork(conf).bind(eng, rnn_length=int(rnn_length), max_samples=int(n_envs),
                                                          true_window=bool(true_window))      # the "policy_eval" copy
        self._adopt(self.policy_net.net, True, summary_writer, max_episode_steps)

    def _before_episodes(self):
        self.net.set_action_counter(0)      # every evaluation draws the same noise

    def eval_once(self, greedy=False, sess=None, max_sequence_length=None):
        global_step = int(self.learner.global_step) if self.learner is not None else 0
        out = _DeviceMonitor.eval_once(self, self.global_policy_net.get_flat_params(), max_sequence_length, greedy=greedy)
        self.write_scalars(global_step)
        return out


class SwarmPolicyMonitor(PolicyMonitor):
    """policy_monitor.py:127-208"""

    def _bind(self):
        self.policy_net.bind(self.env._eng)

    def get_action_from_policy(self, processed_state, history, positions, sess=None):
        # the device net reads the eval engine's current observation (process_state + get_local_states run on the device)
        predictions = self.policy_net.predict()
        mu, sigma = predictions['mu'], predictions['sigma']
        # policy_monitor.py:132 draws np.random.normal from the GLOBAL stream, which Swarm-eval-v0's reset has just reseeded
        # (multiagent.py:47-48): the seeded facade exposes that stream as env.np_random
        rng = getattr(self.env, "np_random", None) or np.random
        raw_actions = mu + sigma * rng.normal(size=mu.shape)
        return SwarmRunner.transform_actions_for_env(raw_actions)

    @staticmethod
    def _create_policy_estimator(conf):
        return ConvSingleAgentPolicyNetwork(conf)

    def _save_actions(self, score, actions):
        with open(self.actions_path, 'w') as f:
            json.dump({'score': score, 'actions': actions}, f)

    def eval_once(self, sess=None, max_sequence_length=5, actions=None):
        """`actions`: a queue.Queue of (10,2) arrays replayed instead of the policy (policy_monitor.py:173-176)."""
        global_step = self.copy_params()

        def choose(state, t):
            if actions:
                return np.asarray(actions.get())
            return self.get_action_from_policy(None, None, None, sess)

        rewards, taken = self._play(self.env.reset(), choose)
        return self._episode_played(global_step, rewards, taken)

    def _episode_played(self, global_step, rewards, taken):
        """What eval_once does with the episode once it is played: the kept best episode, the scalars, the return value."""
        total_reward, episode_length = float(np.sum(rewards)), len(rewards)
        if total_reward > self.best_score:
            self.best_score = total_reward
            self._save_actions(total_reward, [np.asarray(a).tolist() for a in taken])
        self._summaries(global_step, total_reward, episode_length, rewards)
        if getattr(self, "baseline_total_reward", None) is not None and self.summary_writer is not None:
            self.summary_writer.add_scalar("eval/baseline_total_reward", self.baseline_total_reward, global_step)
            self.summary_writer.add_scalar("eval/total_reward_minus_baseline", total_reward - self.baseline_total_reward, global_step)
            self.summary_writer.flush()
        if getattr(self, "search_baseline_total_reward", None) is not None and self.summary_writer is not None:
            self.summary_writer.add_scalar("eval/search_baseline_total_reward", self.search_baseline_total_reward, global_step)
            self.summary_writer.add_scalar("eval/total_reward_minus_search_baseline", total_reward - self.search_baseline_total_reward, global_step)
            self.summary_writer.flush()
        if getattr(self, "cem_plan_baseline_total_reward", None) is not None and self.summary_writer is not None:
            self.summary_writer.add_scalar("eval/cem_plan_baseline_total_reward", self.cem_plan_baseline_total_reward, global_step)
            self.summary_writer.add_scalar("eval/total_reward_minus_cem_plan_baseline", total_reward - self.cem_plan_baseline_total_reward, global_step)
            self.summary_writer.flush()
        return total_reward, episode_length, rewards

    def baseline(self):
        """The scripted do-nothing baseline (goldsrl/baselines.py:ScriptedSwarmBaseline) on the monitor's own eval env, so it plays
        exactly the seeded episode the policy is evaluated on: the env is reset, both scripts run in one kernel launch, and the env
        is reset again.  Keeps baseline_name and baseline_total_reward (every later eval_once writes eval/baseline_total_reward and
        eval/total_reward_minus_baseline) and the whole statistics in baseline_stats.  Returns the two.  The reference has no
        counterpart."""
        from ...baselines import ScriptedSwarmBaseline
        self.env.reset()
        b = ScriptedSwarmBaseline(self.env._eng)
        self.baseline_stats = b.run()
        self.baseline_name, self.baseline_total_reward = b.best(0)
        self.env.reset()
        return self.baseline_name, self.baseline_total_reward

    def rule_baseline(self, rules=DEFAULT_SWARM_RULES):
        """The feedback-rule baseline (goldsrl/baselines.py:SwarmRuleBaseline) on the monitor's own eval env: the env is reset, every
        rule plays the seeded episode in one kernel launch, and the env is reset again.  Keeps baseline_name (the best rule, spelled
        out), baseline_rule (its index and six numbers), baseline_total_reward (every later eval_once writes
        eval/baseline_total_reward and eval/total_reward_minus_baseline) and the whole outputs in baseline_stats, replacing what
        baseline() kept.  Returns (baseline_name, baseline_total_reward).  The reference has no counterpart."""
        from ...baselines import SwarmRuleBaseline
        self.env.reset()
        b = SwarmRuleBaseline(self.env._eng, rules)
        self.baseline_stats = b.run()
        i, six, total = b.best_total()
        self.baseline_rule = (i, six)
        self.baseline_name = "rule %d (cancel %g, gain %g, anchor %s, offset (%g, %g), radius %g)" % (
            (i, six[0], six[1], "nearest locust" if six[2] else "centroid") + six[3:])
        self.baseline_total_reward = total
        self.env.reset()
        return self.baseline_name, self.baseline_total_reward

    def plan_baseline(self, horizon=8, replan=4, rules=DEFAULT_SWARM_RULES):
        """The receding-horizon rule planner (goldsrl/baselines.py:SwarmRulePlanner) on the monitor's own eval env: the env is reset,
        the planner plays the seeded episode in one call -- every rule `horizon` steps ahead, the best committed for `replan` steps,
        again -- and the env is reset again.  Keeps baseline_name, baseline_total_reward (every later eval_once writes
        eval/baseline_total_reward and eval/total_reward_minus_baseline) and the whole outputs, the committed actions among them, in
        baseline_stats, replacing what baseline() or rule_baseline() kept.  Returns (baseline_name, baseline_total_reward).  The
        reference has no counterpart."""
        from ...baselines import SwarmRulePlanner
        self.env.reset()
        b = SwarmRulePlanner(self.env._eng, rules, horizon, replan)
        self.baseline_stats = b.run(keep_actions=True)
        self.baseline_name = "plan (horizon %d, replan %d, %d rules, %d switches)" % (b.horizon, b.replan, len(b.rules), b.switches())
        self.baseline_total_reward = b.total()
        self.env.reset()
        return self.baseline_name, self.baseline_total_reward

    def search_baseline(self, generations=8, candidates=32, elites=8, rules=DEFAULT_SWARM_RULES):
        """The tuned fixed rule (goldsrl/baselines.py:SwarmRuleSearch) on the monitor's own eval env: the env is reset, the search
        starts from the best rule of `rules` on the seeded episode and runs in one call, and the env is reset again.  Keeps
        search_baseline_name, search_baseline_rule (the six numbers), search_baseline_total_reward (every later eval_once writes
        eval/search_baseline_total_reward and eval/total_reward_minus_search_baseline) and the search's outputs in search_stats.  What
        baseline(), rule_baseline() or plan_baseline() kept stays, and with it every scalar they write; only when none of them has
        run does the search also supply baseline_name and baseline_total_reward.  Returns (search_baseline_name,
        search_baseline_total_reward).  The reference has no counterpart."""
        from ...baselines import SwarmRuleSearch
        self.env.reset()
        b = SwarmRuleSearch(self.env._eng, None, generations, candidates, elites, rules=rules)
        self.search_stats = b.run()
        six, total = b.best()
        mine = getattr(self, "baseline_total_reward", None) is None or getattr(self, "baseline_name", 0) == getattr(self, "search_baseline_name", 1)
        self.search_baseline_rule, self.search_baseline_total_reward = six, total
        self.search_baseline_name = "tuned rule (cancel %g, gain %g, anchor %s, offset (%g, %g), radius %g; %d generations of %d, %d elites)" % (
            (six[0], six[1], "nearest locust" if six[2] else "centroid") + six[3:] + (b.generations, b.candidates, b.elites))
        if mine:
            self.baseline_name, self.baseline_total_reward = self.search_baseline_name, total
        self.env.reset()
        return self.search_baseline_name, self.search_baseline_total_reward

    def cem_plan_baseline(self, horizon=32, replan=8, generations=2, candidates=16, elites=4, rules=DEFAULT_SWARM_RULES):
        """The search planner (goldsrl/baselines.py:SwarmSearchPlanner) on the monitor's own eval env: the env is reset, the planner
        starts from the best rule of `rules` on the seeded episode and plays it in one call -- at every decision a short search over
        `horizon`-step lookaheads, the result or the better rule of `rules` committed for `replan` steps, again -- and the env is
        reset again.  Keeps cem_plan_baseline_name, cem_plan_baseline_total_reward (every later eval_once writes
        eval/cem_plan_baseline_total_reward and eval/total_reward_minus_cem_plan_baseline) and the planner's outputs, the committed
        actions among them, in cem_plan_stats.  What the other baselines kept stays, and with it every scalar they write; only when
        none of them has run does this one also supply baseline_name and baseline_total_reward.  Returns (cem_plan_baseline_name,
        cem_plan_baseline_total_reward).  The defaults are (32, 8, 2, 16, 4), not the planner class's (8, 4, 2, 12, 4): over 64 other
        seeds the long horizon earns 5.2 more on average (profiles/swarm_cemplan_times.json), although on this env's own seed-192
        episode the short one is 3.2 ahead.  The reference has no counterpart."""
        from ...baselines import SwarmSearchPlanner
        self.env.reset()
        b = SwarmSearchPlanner(self.env._eng, rules, None, horizon, replan, generations, candidates, elites)
        self.cem_plan_stats = b.run(keep_actions=True)
        total = b.total()
        mine = getattr(self, "baseline_total_reward", None) is None or getattr(self, "baseline_name", 0) == getattr(self, "cem_plan_baseline_name", 1)
        self.cem_plan_baseline_total_reward = total
        self.cem_plan_baseline_name = "search plan (horizon %d, replan %d, %d generations of %d, %d elites, %d rules; %d of %d decisions searched)" % (
            b.horizon, b.replan, b.generations, b.candidates, b.elites, 0 if b.rules is None else len(b.rules), b.searched(),
            int((self.cem_plan_stats["choices"] >= 0).sum()))
        if mine:
            self.baseline_name, self.baseline_total_reward = self.cem_plan_baseline_name, total
        self.env.reset()
        return self.cem_plan_baseline_name, self.cem_plan_baseline_total_reward


class DeviceSwarmPolicyMonitor(SwarmPolicyMonitor):
    """SwarmPolicyMonitor with the episodes played on the device (ConvNet.eval, include/goldsrl_neteval.h): `n_envs` seeded episodes of
    the eval registration -- env 0 is the registration's episode (seed 192), env k the one of seed 192 + k -- enqueued as pipelines
    and read back once, instead of a blocking predict, a draw, a transform, a step and four reads per step.

    The noise is the host loop's: after the reset, env k's generator (SwarmEnv.np_randoms) draws the episode's normals as one
    (S, 10, 2) block, the same stream as S draws of (10, 2), and the device forms a = mu + sigma * z from them.  So env 0's episode
    is, bit for bit, the one SwarmPolicyMonitor.eval_once plays; it is what eval_once returns and what the kept best episode in
    swarm-eval.json, the scalars and the baseline scalars speak of.  Every env's total and length are kept in total_rewards /
    episode_lengths, and with n_envs > 1 eval/mean_total_reward is written too.  greedy=True acts with the norm-clipped mu.

    Two handles.  The shared evaluation of the trunk (csrc/net_shared.inc) associates an env's sums by the union of its chunk's masks,
    so an env's bits depend on its chunk mates: env 0 inside a three-env chunk differs from the one-env episode in the ninth digit
    of its total.  One env per chunk would keep every env's bits but costs a chunk's launches per env and step (measured 349 ms
    at 16 envs against 46 in one chunk, profiles/conv_eval_times.json).  So env 0 plays alone on `env`, the registration's own
    one-env handle -- exactly the parent's episode, and what baseline() / rule_baseline() (inherited) play and leave reset -- and
    envs 1.. play in one chunk on `rest_env` (seed 193, n_envs - 1 envs) under a second copy of the policy; the two evaluations are
    run one behind the other."""

    def __init__(self, env="Swarm-eval-v0", global_policy_net=None, state_processor=None, summary_writer=None, saver=None, network_conf=None,
                 learner=None, n_envs=1, greedy=False):
        from ...envs import registry
        cls, max_steps, kwargs = registry[env]
        if n_envs < 1:
            raise ValueError("n_envs must be at least 1")
        if not max_steps or not kwargs.get("seed"):
            raise ValueError("no device evaluation for env %r: it plays the seeded episodes of a registration with a TimeLimit" % (env,))
        self.n_envs, self.greedy, self.max_episode_steps = int(n_envs), bool(greedy), int(max_steps)
        self.total_rewards, self.episode_lengths = None, None       # every env's, of the last evaluation
        conf = network_conf if network_conf is not None else global_policy_net.conf
        super(DeviceSwarmPolicyMonitor, self).__init__(cls(max_episode_steps=max_steps, **kwargs), global_policy_net, state_processor,
                                                       summary_writer, saver, conf, learner)
        self.rest_env, self.rest_net = None, None
        if self.n_envs > 1:
            self.rest_env = cls(max_episode_steps=max_steps, **dict(kwargs, seed=kwargs["seed"] + 1, n_envs=self.n_envs - 1))
            self.rest_net = self._create_policy_estimator(conf).bind(self.rest_env._eng)      # one chunk up to 8 192 envs

    def copy_params(self):
        flat = self.global_policy_net.get_flat_params()
        for net in (self.policy_net, self.rest_net):
            if net is not None:
                net.set_flat_params(flat)
        return int(self.learner.global_step) if self.learner is not None else 0

    def _episodes(self):
        """Reset, draw, play: the outputs of ConvNet.eval for env 0 and for envs 1.., one evaluation behind the other (the range flag
        of the GEMMs is one word per device: it speaks of one net's work at a time).  The two policy copies are two nets, each with
        its own arithmetic form: one whose forward pass left the fp16 range has moved to the fp32 form when its read raises E_RANGE,
        and plays its own episodes once more from a reset; the other net is not touched by that."""
        from ... import _ffi
        S, out = self.max_episode_steps, []

        def play(e, n):
            e.reset()
            normals = None if self.greedy else np.stack([rs.normal(size=(S, 10, 2)) for rs in e.np_randoms])
            return n.net.eval(S, greedy=self.greedy, normals=normals, keep_actions=e is self.env)

        for e, n in ((self.env, self.policy_net), (self.rest_env, self.rest_net)):
            if e is None:
                continue
            try:
                out.append(play(e, n))
            except _ffi.GrlError as err:
                if err.code != _ffi.E_RANGE:
                    raise
                out.append(play(e, n))
        return out

    def eval_once(self, sess=None, max_sequence_length=5, actions=None):
        if actions:      # a replayed queue is the host loop's, on env 0
            return super(DeviceSwarmPolicyMonitor, self).eval_once(sess, max_sequence_length, actions)
        global_step = self.copy_params()
        out = self._episodes()
        lengths = [int(n) for r in out for n in r["length"]]
        rows = [row for r in out for row in r["rewards"]]
        episodes = [[float(v) for v in rows[e][:lengths[e]]] for e in range(self.n_envs)]
        self.total_rewards = np.array([float(np.sum(rew)) for rew in episodes])
        self.episode_lengths = np.array(lengths)
        played = self._episode_played(global_step, episodes[0], [out[0]["actions"][0, t] for t in range(lengths[0])])
        if self.n_envs > 1 and self.summary_writer is not None:
            self.summary_writer.add_scalar("eval/mean_total_reward", float(self.total_rewards.mean()), global_step)
            self.summary_writer.flush()
        return played

    def close(self):
        """Closes the nets and engines the monitor built."""
        for net, env in ((self.policy_net, self.env), (self.rest_net, self.rest_env)):
            if net is not None:
                net.net.close()
                env._eng.close()


class FieldSwarmPolicyMonitor(SwarmPolicyMonitor):
    """SwarmPolicyMonitor for ConvPolicyVFieldNetwork: one episode of the registered eval env on a one-env handle of the NET's grid
    size (the registration's own handle observes on the conv policy's 84-cell grid).  Per step the policy reads the handle's current
    observation (grl_fieldnet_predict_swarm) and acts greedily: the action is the norm-clipped mu, handed to the env as float64
    rows, so swarm-eval.json replays in make_swarm_gif's default arithmetic.  Scalars, the kept best episode and the --baseline /
    --rule-baseline yardsticks are SwarmPolicyMonitor's.  The reference never built a monitor for this net.

    device_episode (the default): the whole episode is one kernel launch (FieldNet.eval, include/goldsrl_fieldeval.h) -- the same
    greedy float64-row episode bit for bit, without the ~400 blocking round trips of the host loop.  device_episode=False, or a
    geometry whose env does not fit the kernel's LDS, plays the host loop.  n_envs > 1 (device episodes only) evaluates on n_envs
    seeded episodes: env 0 is the registration's, env k the one of seed + k; eval_once still returns env 0's episode and keeps
    every env's in total_rewards / episode_lengths, with eval/mean_total_reward among the scalars."""

    def __init__(self, env="Swarm-eval-v0", global_policy_net=None, state_processor=None, summary_writer=None, saver=None, network_conf=None,
                 learner=None, n_envs=1, device_episode=True):
        from ...envs import registry
        conf = network_conf if network_conf is not None else global_policy_net.conf
        cls, max_steps, kwargs = registry[env]
        if n_envs < 1:
            raise ValueError("n_envs must be at least 1")
        if n_envs > 1 and not device_episode:
            raise ValueError("the host loop plays one env; n_envs = %d needs device_episode" % n_envs)
        self.n_envs, self.device_episode, self.max_episode_steps = int(n_envs), bool(device_episode), int(max_steps or 0)
        self.total_rewards, self.episode_lengths = None, None       # every env's, of the last device evaluation
        more = {"n_envs": self.n_envs} if self.n_envs > 1 else {}
        super(FieldSwarmPolicyMonitor, self).__init__(cls(max_episode_steps=max_steps, grid_size=conf['height'], **dict(kwargs, **more)),
                                                      global_policy_net, state_processor, summary_writer, saver, conf, learner)

    def _bind(self):
        self.policy_net.bind(self.env._eng, max_samples=self.n_envs, gamma=0.99)      # gamma: the bind checks the geometry against the handle

    def eval_once(self, sess=None, max_sequence_length=5, actions=None):
        from ... import _ffi
        if not self.device_episode or actions or self.max_episode_steps < 1:      # a replayed queue and an env without TimeLimit are the host loop's
            return super(FieldSwarmPolicyMonitor, self).eval_once(sess, max_sequence_length, actions)
        global_step = self.copy_params()
        self.env.reset()
        try:
            r = self.policy_net.net.eval(self.max_episode_steps, greedy=True, rows32=False, keep_actions=True)
        except _ffi.GrlError as e:
            if e.code != _ffi.E_STATE or self.n_envs > 1:
                raise
            self.device_episode = False      # the geometry is past the kernel's LDS budget
            return super(FieldSwarmPolicyMonitor, self).eval_once(sess, max_sequence_length, actions)
        lengths = [int(n) for n in r["length"]]
        episodes = [[float(v) for v in r["rewards"][e, :lengths[e]]] for e in range(self.n_envs)]
        self.total_rewards = np.array([float(np.sum(rew)) for rew in episodes])
        self.episode_lengths = np.array(lengths)
        out = self._episode_played(global_step, episodes[0], [r["actions"][0, t] for t in range(lengths[0])])
        if self.n_envs > 1 and self.summary_writer is not None:
            self.summary_writer.add_scalar("eval/mean_total_reward", float(self.total_rewards.mean()), global_step)
            self.summary_writer.flush()
        return out

    def get_action_from_policy(self, processed_state, history, positions, sess=None):
        mu = self.policy_net.net.predict_swarm()['mu']
        return SwarmRunner.transform_actions_for_env(mu).astype(np.float64)

    @staticmethod
    def _create_policy_estimator(conf):
        return ConvPolicyVFieldNetwork(conf)
