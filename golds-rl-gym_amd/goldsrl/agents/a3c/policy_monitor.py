"""PolicyMonitor (reference fed_gym/agents/a3c/policy_monitor.py:11-118) on the device: the greedy evaluation of the A3C Gaussian
agent, every episode of `n_envs` seeded eval envs in one kernel launch (grl_anet_eval, include/goldsrl_gaussnet.h).

The reference plays ONE episode of the eval env per evaluation, one `sess.run` per step, with the action sigmoid(mu[0]).  Here the
monitor owns an eval engine of `n_envs` envs whose streams are keyed by the global env id, so env 0 is exactly that single episode
and envs 1.. are further seeded episodes of the same registration; `eval_once` returns env 0's `(total_reward, episode_length,
rewards)` as the reference does and keeps every env's totals for the caller.  The action is the worker's own transform of mu:
the stable sigmoid for Solow, tanh for TradeAR1 (the reference's monitor applies its sigmoid to every env kind).
What has no counterpart: the gym `Monitor` video wrapper, the TF session and summaries (the caller writes the scalars), the Saver.

GatedPolicyMonitor is the same monitor for the Ticker gated trader (grl_gnet_eval, include/goldsrl_gatedeval.h).  The reference has
nothing to compare it with: no PolicyMonitor is written for TickerGatedTraderWorker, its get_action_from_policy ignores `stochastic`
(worker.py:466-476), so the net cannot act without drawing, and there is no eval registration of the Ticker env, no held-out price
table and no episode that repeats from one evaluation to the next.  All three are stated here instead.  The greedy rule, per asset:
choice = the first index of the largest of the three float32 probabilities (np.argmax, as GridSolowWorker.get_greedy_action picks,
worker.py:370-372), raw = mu[choice], fraction = the worker's float64 sigmoid of raw rounded to float32 (worker.py:229-230).  The
eval registration: seed 1692 and a reseed at every reset, as the Solow eval registration has it, so env e trades the same 1 024-row
price window at every evaluation; the table may be another one than the training table.

GridPolicyMonitor is the monitor of the discrete savings-grid agent (grl_dnet_eval, include/goldsrl_discreteeval.h) on the Solow
eval registration.  The reference's PolicyMonitor cannot evaluate that agent -- it reads preds["mu"] -- and GridSolowWorker's own
greedy path cannot run (get_greedy_action hands the grid value to transform_raw_action, which indexes it, worker.py:370-376).  The
rule is the evident intention: choice = the first index of the largest float32 probability, action = grid[choice]."""
import json
import time

import numpy as np

ENVS = ("Solow-%d-%d-finite-eval-v0", "TradeAR1-v0")
TRADE_TUNE_SEED = 1693      # of the engine PolicyMonitor.search_baseline tunes on: the eval registration's 1692 is the monitor's own


def make_eval_engine(env, n_envs, device_id=0, max_episode_steps=1024):
    """The engine of an eval registration with n_envs envs.  env: `Solow-p-q-finite-eval-v0` (seed 1692, reseeded at every reset,
    so every evaluation plays the same episodes) or `TradeAR1-v0` (fed_gym/__init__.py:3-33, both capped at 1 024 steps)."""
    from ... import _ffi
    if env.startswith("Solow-") and env.endswith("-finite-eval-v0"):
        p, q = (int(v) for v in env.split("-")[1:3])
        return _ffi.Engine(_ffi.ENV_SOLOW, n_envs, device_id=device_id, seed=1692, flags=_ffi.F_RESEED_EACH_RESET, solow_p=p, solow_q=q,
                           max_episode_steps=max_episode_steps)
    if env == "TradeAR1-v0":
        return _ffi.Engine(_ffi.ENV_TRADE, n_envs, device_id=device_id, seed=1692, n_assets=2, max_episode_steps=max_episode_steps)
    raise ValueError("no device evaluation for env %r (one of %s)" % (env, ", ".join(ENVS)))


def make_ticker_eval_engine(table, n_envs, device_id=0, max_episode_steps=1023):
    """The engine of the Ticker eval registration with n_envs envs on `table` (the sampler's (rows,4) data matrix, or a sampler):
    seed 1692, reseeded at every reset, so env e's price window is the same at every evaluation.  1 023 steps is the longest episode
    a 1 024-row window holds."""
    from ... import _ffi
    eng = _ffi.Engine(_ffi.ENV_TICKER, n_envs, device_id=device_id, seed=1692, flags=_ffi.F_RESEED_EACH_RESET,
                      max_episode_steps=max_episode_steps)
    eng.ticker_set_table(getattr(table, "data_matrix", table))
    return eng


class _DeviceMonitor(object):
    """What the device monitors share: the evaluation net on its eval engine, the log, the scalars, the loop."""

    def _adopt(self, net, own, summary_writer, max_episode_steps):
        self.summary_writer = summary_writer
        self.max_episode_steps = int(max_episode_steps)
        self._own = own
        self.net = net
        self.n_envs = int(net.eng.E)
        self.total_rewards, self.episode_lengths = None, None       # every env's, of the last evaluation
        self.log = {"total_reward": [], "episode_length": [], "mean_total_reward": [], "std_total_reward": [], "n_envs": self.n_envs}

    def _before_episodes(self):
        """Between copying the parameters and resetting the eval envs (the flat PAAC monitor rewinds its action noise here)."""

    def eval_once(self, params, max_sequence_length=None, **eval_kw):
        """Copy the parameters (copy_params_op), reset the eval envs, play every env's episode (eval_kw: further arguments of the
        net's eval, e.g. greedy=).  Returns env 0's (total_reward, episode_length, rewards)."""
        rnn = getattr(self.net, "R", None) or self.net.cfg.rnn_length
        if max_sequence_length is not None and max_sequence_length != rnn:
            raise ValueError("max_sequence_length %r: the evaluation net was built with %r" % (max_sequence_length, rnn))
        self.net.set_params(params)
        self._before_episodes()
        self.net.eng.reset()
        r = self.net.eval(self.max_episode_steps, trace_steps=self.max_episode_steps, trace_fields=("rewards",), **eval_kw)
        self.total_rewards = np.asarray(r["total_reward"], np.float64)
        self.episode_lengths = np.asarray(r["length"])
        total_reward, episode_length = float(self.total_rewards[0]), int(self.episode_lengths[0])
        rewards = [float(v) for v in np.asarray(r["rewards"])[:episode_length, 0]]
        self.log["total_reward"].append(total_reward)
        self.log["episode_length"].append(episode_length)
        self.log["mean_total_reward"].append(float(self.total_rewards.mean()))
        self.log["std_total_reward"].append(float(self.total_rewards.std()))
        return total_reward, episode_length, rewards

    def write_scalars(self, global_step):
        """eval/total_reward and eval/episode_length of env 0 (policy_monitor.py:79-83), eval/mean_total_reward over the envs"""
        w = self.summary_writer
        if w is None or not self.log["total_reward"]:
            return
        w.add_scalar("eval/total_reward", self.log["total_reward"][-1], global_step)
        w.add_scalar("eval/episode_length", self.log["episode_length"][-1], global_step)
        w.add_scalar("eval/mean_total_reward", self.log["mean_total_reward"][-1], global_step)
        w.flush()

    def _baseline_rates(self):
        """The rates baseline() plays when given none: the reference's 20 (scripts/constant_solow.py:19)."""
        from ...baselines import REFERENCE_RATES
        return REFERENCE_RATES

    def baseline(self, rates=None):
        """The constant-savings baseline (goldsrl/baselines.py) on the monitor's own eval engine, so it plays exactly the seeded
        episodes the policy is evaluated on: one kernel launch for every (env, rate) pair.  Keeps baseline_rate and
        baseline_total_reward -- the best rate by the mean over the envs of the episode's total reward, the unit of
        eval/mean_total_reward -- and the whole statistics in baseline_stats; leaves the engine reset.  Returns the two."""
        from ... import _ffi
        from ...baselines import ConstantSavingsBaseline
        eng = self.net.eng
        if eng.kind != _ffi.ENV_SOLOW:
            raise ValueError("the constant-savings baseline exists for the Solow env only")
        b = ConstantSavingsBaseline(rates=self._baseline_rates() if rates is None else rates, max_episode_steps=self.max_episode_steps,
                                    engine=eng)
        self.baseline_stats = b.run()
        rate, total = b.best_total()
        self.baseline_rate, self.baseline_total_reward = float(rate), float(total)
        eng.reset()
        return self.baseline_rate, self.baseline_total_reward

    def optimal(self, grid=None, horizon=None):
        """The optimal-savings yardstick (goldsrl/baselines.py:OptimalSavingsBaseline) on the monitor's own eval engine, so it plays
        exactly the seeded episodes the policy is evaluated on: the backward induction (one launch per stage), then every env's
        episode in one launch.  Keeps optimal_total_reward -- the mean over the envs of the episode's total reward, the unit of
        eval/mean_total_reward -- and the whole statistics in optimal_stats; leaves the engine reset.  Returns the figure."""
        from ... import _ffi
        from ...baselines import OptimalSavingsBaseline
        eng = self.net.eng
        if eng.kind != _ffi.ENV_SOLOW:
            raise ValueError("the optimal-savings yardstick exists for the Solow env only")
        b = OptimalSavingsBaseline(grid=grid, horizon=horizon, max_episode_steps=self.max_episode_steps, engine=eng)
        self.optimal_stats = b.run()
        self.optimal_total_reward = b.total()
        eng.reset()
        return self.optimal_total_reward

    def rule_baseline(self, rules=None):
        """The scripted trading-rule baseline (goldsrl/baselines.py) on the monitor's own TradeAR1 eval engine: resets it and plays
        every (env, rule) pair in one kernel launch.  The engine's price generator moves on from one evaluation to the next, so call
        this directly before eval_once: it then plays exactly the episodes that evaluation plays.  Keeps baseline_rule (index,
        (gain, bias)), baseline_total_reward -- the best rule's mean over the envs of the episode's total reward, the unit of
        eval/mean_total_reward -- and the whole statistics in baseline_stats; leaves the engine reset.  Returns
        (rule_index, (gain, bias), baseline_total_reward)."""
        from ... import _ffi
        from ...baselines import DEFAULT_TRADE_RULES, TradingRuleBaseline
        eng = self.net.eng
        if eng.kind != _ffi.ENV_TRADE:
            raise ValueError("the trading-rule baseline exists for the TradeAR1 env only")
        b = TradingRuleBaseline(eng, DEFAULT_TRADE_RULES if rules is None else rules, self.max_episode_steps)
        eng.reset()
        self.baseline_stats = b.run()
        i, rule, total = b.best_total()
        self.baseline_rule, self.baseline_total_reward = (i, rule), total
        return i, rule, total

    def trade_ceiling(self, horizons=None):
        """The foresight ceiling (goldsrl/baselines.py:TradeForesightCeiling) on the monitor's own TradeAR1 eval engine: resets it
        and plays every (env, horizon) pair in one call.  The engine's price generator moves on from one evaluation to the next, so
        call this directly before eval_once, as rule_baseline() is: it then plays exactly the episodes that evaluation plays.
        Keeps ceiling_total_reward -- the mean over the envs of the total reward of the trader who knows every row of its episode,
        the unit of eval/mean_total_reward --, ceiling_table (one (horizon, mean total, mean length, mean trades) row per horizon),
        ceiling_bound (every env's bound, (E,)) and the whole statistics in ceiling_stats; leaves the engine reset.  Returns
        ceiling_total_reward."""
        from ... import _ffi
        from ...baselines import DEFAULT_TRADE_HORIZONS, TradeForesightCeiling
        eng = self.net.eng
        if eng.kind != _ffi.ENV_TRADE:
            raise ValueError("the foresight ceiling of TradeAR1 exists for the TradeAR1 env only")
        c = TradeForesightCeiling(eng, DEFAULT_TRADE_HORIZONS if horizons is None else horizons, self.max_episode_steps)
        eng.reset()
        self.ceiling_stats = c.run()
        self.ceiling_table = c.table()
        self.ceiling_total_reward = c.ceiling()
        self.ceiling_bound = c.bound()
        return self.ceiling_total_reward

    def write_baseline_scalars(self, global_step):
        """eval/baseline_total_reward and eval/mean_total_reward_minus_baseline of the last evaluation (after baseline() or
        rule_baseline()); after optimal() also eval/optimal_total_reward and, with both ends known,
        eval/mean_total_reward_share_of_gap = (mean - baseline) / (optimal - baseline)"""
        w = self.summary_writer
        floor, ceiling = getattr(self, "baseline_total_reward", None), getattr(self, "optimal_total_reward", None)
        if w is None or (floor is None and ceiling is None):
            return
        if floor is not None:
            w.add_scalar("eval/baseline_total_reward", floor, global_step)
            if self.log["mean_total_reward"]:
                w.add_scalar("eval/mean_total_reward_minus_baseline", self.log["mean_total_reward"][-1] - floor, global_step)
        if ceiling is not None:
            w.add_scalar("eval/optimal_total_reward", ceiling, global_step)
            if floor is not None and self.log["mean_total_reward"] and ceiling != floor:
                w.add_scalar("eval/mean_total_reward_share_of_gap", (self.log["mean_total_reward"][-1] - floor) / (ceiling - floor), global_step)
        w.flush()

    def write_ceiling_scalars(self, global_step):
        """eval/ceiling_total_reward (after ticker_ceiling() or trade_ceiling()) and, with the rule baseline's floor and an
        evaluation, eval/mean_total_reward_share_of_gap = (mean - baseline) / (ceiling - baseline) of the last evaluation"""
        w, ceiling = self.summary_writer, getattr(self, "ceiling_total_reward", None)
        if w is None or ceiling is None:
            return
        w.add_scalar("eval/ceiling_total_reward", ceiling, global_step)
        floor = getattr(self, "baseline_total_reward", None)
        if floor is not None and self.log["mean_total_reward"] and ceiling != floor:
            w.add_scalar("eval/mean_total_reward_share_of_gap", (self.log["mean_total_reward"][-1] - floor) / (ceiling - floor), global_step)
        w.flush()

    def write_log(self, total_reward_log_file):
        """The reference's two keys from env 0 (policy_monitor.py:110-118), plus mean_total_reward, std_total_reward and n_envs."""
        with open(total_reward_log_file, "w") as f:
            json.dump(self.log, f)

    def continuous_eval(self, eval_every, get_params, coord, max_seq_length=None, total_reward_log_file=None, get_global_step=None):
        """Evaluate every eval_every seconds until coord.should_stop() (policy_monitor.py:98-118).  get_params() returns the
        learner's current flat parameters."""
        while not coord.should_stop():
            self.eval_once(get_params(), max_sequence_length=max_seq_length)
            if get_global_step is not None:
                self.write_scalars(get_global_step())
            if total_reward_log_file:
                self.write_log(total_reward_log_file)
            if eval_every > 0:
                time.sleep(eval_every)

    def close(self):
        if self._own and self.net is not None:
            eng = self.net.eng
            self.net.close()
            eng.close()
        self.net = None


class PolicyMonitor(_DeviceMonitor):
    """policy_monitor.py:11-118.  env: the eval registration's id.  global_policy_net, state_processor, summary_writer, saver are
    kept as the reference keeps them (the device does the processing; summary_writer, when given, gets the eval/* scalars through
    add_scalar).  net: an evaluation net to use instead of building one (its `eng` is the eval engine)."""

    def __init__(self, env, global_policy_net=None, state_processor=None, summary_writer=None, saver=None, num_actions=None,
                 input_size=None, temporal_size=None, n_envs=1, max_seq_length=5, scale=1.0, device_id=0, max_episode_steps=1024,
                 net=None):
        self.env = env
        self.global_policy_net = global_policy_net
        self.state_processor = state_processor
        self.saver = saver
        own = net is None
        if net is None:
            from ... import _ffi_gauss
            if n_envs < 1:
                raise ValueError("n_envs must be at least 1")
            eng = make_eval_engine(env, n_envs, device_id, int(max_episode_steps))
            net = _ffi_gauss.GaussNet(eng, rnn_length=max_seq_length, scale=scale, max_samples=1)       # the "policy_eval" copy
            want = (net.A, net.S0, net.D)
            for name, got, exp in zip(("num_actions", "input_size", "temporal_size"), (num_actions, input_size, temporal_size), want):
                if got is not None and got != exp:
                    raise ValueError("%s = %r, the device net of %s has %r" % (name, got, env, exp))
        self._adopt(net, own, summary_writer, max_episode_steps)

    def search_baseline(self, generations=8, candidates=32, elites=8, starts=None, tune_seed=TRADE_TUNE_SEED, **search_kw):
        """The tuned rule (goldsrl/baselines.py:TradeRuleSearch): the four numbers (gain_buy, gain_sell, bias, ref) a cross-entropy
        search finds, every generation in one call.  The eval engine's price generator moves on between evaluations, so there is
        no fixed set of episodes to tune on: the FIRST call tunes, on a second eval-style TradeAR1 engine of the same n_envs
        and n_assets with its own seed (tune_seed) -- and so does a later call whose arguments differ from those the kept rule
        was tuned with --, and keeps search_baseline_rule, search_baseline_in_sample_total_reward (its fit
        there) and every start's (start, rule, fit) in search_baseline_results.  EVERY call then resets the monitor's own engine
        and plays the kept rule on it (_ffi_tradesearch.trade_search_play): called directly before eval_once, as rule_baseline()
        is, it plays exactly the episodes that evaluation plays -- four numbers fitted in sample, played out of sample.  Keeps
        search_baseline_total_reward, the unit of eval/mean_total_reward, and every env's total in search_baseline_totals; leaves
        the engine reset.  starts: a list of start rules (default: the best default rule on the tuning engine, lifted to (g, g, b,
        1)).  The scalars of rule_baseline() and trade_ceiling() are not touched.  Measured at the registration's 2 assets (64 envs x
        256 steps, LABNOTES AC) the tuned rule gains 0.010 in sample and nothing on other seeds, so expect a total near
        rule_baseline()'s here; at 16 assets it keeps 0.07 out of sample.  Returns (rule, search_baseline_total_reward)."""
        from ... import _ffi, _ffi_tradesearch
        from ...baselines import TradeRuleSearch
        eng = self.net.eng
        if eng.kind != _ffi.ENV_TRADE:
            raise ValueError("the TradeAR1 rule search exists for the TradeAR1 env only")
        asked = (int(generations), int(candidates), int(elites), None if starts is None else np.asarray(starts, np.float32).tobytes(),
                 int(tune_seed), sorted((k, np.asarray(v).tobytes() if v is not None else None) for k, v in search_kw.items()))
        if getattr(self, "_search_baseline_asked", None) != asked:
            tuned_on = _ffi.Engine(_ffi.ENV_TRADE, self.n_envs, device_id=eng.cfg.device_id, seed=int(tune_seed), n_assets=eng.cfg.n_assets,
                                   max_episode_steps=self.max_episode_steps)
            try:
                tuned_on.reset()
                b = TradeRuleSearch(tuned_on, generations, candidates, elites, starts=starts, max_episode_steps=self.max_episode_steps,
                                    **search_kw)
                self.search_baseline_rule, self.search_baseline_in_sample_total_reward = b.best()
                self.search_baseline_results = b.results
                self._search_baseline_asked = asked
            finally:
                tuned_on.close()
        eng.reset()
        self.search_baseline_totals = _ffi_tradesearch.trade_search_play(eng, self.search_baseline_rule, self.max_episode_steps)
        self.search_baseline_total_reward = _ffi_tradesearch.fit_mean(self.search_baseline_totals)
        return self.search_baseline_rule, self.search_baseline_total_reward

    def write_search_baseline_scalars(self, global_step):
        """eval/search_baseline_total_reward, eval/mean_total_reward_minus_search_baseline of the last evaluation and
        eval/search_baseline_in_sample_total_reward (after search_baseline())"""
        w, total = self.summary_writer, getattr(self, "search_baseline_total_reward", None)
        if w is None or total is None:
            return
        w.add_scalar("eval/search_baseline_total_reward", total, global_step)
        if self.log["mean_total_reward"]:
            w.add_scalar("eval/mean_total_reward_minus_search_baseline", self.log["mean_total_reward"][-1] - total, global_step)
        w.add_scalar("eval/search_baseline_in_sample_total_reward", self.search_baseline_in_sample_total_reward, global_step)
        w.flush()


class GatedPolicyMonitor(_DeviceMonitor):
    """The PolicyMonitor of the Ticker gated trader.  table: the eval price table (the sampler's data matrix or a sampler), the
    training one or a held-out one.  summary_writer, when given, gets the eval/* scalars through add_scalar.  net: an evaluation
    net to use instead of building one (its `eng` is the eval engine)."""

    def __init__(self, table=None, summary_writer=None, n_envs=1, max_seq_length=5, scale=1.0, device_id=0, max_episode_steps=1023,
                 net=None):
        own = net is None
        if net is None:
            from ... import _ffi_gated
            if n_envs < 1:
                raise ValueError("n_envs must be at least 1")
            if table is None:
                raise ValueError("the Ticker eval engine needs a price table")
            eng = make_ticker_eval_engine(table, n_envs, device_id, int(max_episode_steps))
            net = _ffi_gated.GatedNet(eng, rnn_length=max_seq_length, scale=scale, max_samples=1)
        self._adopt(net, own, summary_writer, max_episode_steps)

    def ticker_baseline(self, rules=None):
        """The scripted rule baseline (goldsrl/baselines.py:TickerRuleBaseline) on the monitor's own Ticker eval engine: resets it
        and plays every (env, rule) pair in one kernel launch.  The eval engine is reseeded at every reset, so every evaluation
        plays these price windows: one run before the first update serves them all.  Keeps baseline_rule (index, the six
        parameters), baseline_total_reward -- the best rule's mean over the envs of the episode's total reward, the unit of
        eval/mean_total_reward -- and the whole statistics in baseline_stats; leaves the engine reset.  Returns
        (rule_index, the six parameters, baseline_total_reward)."""
        from ...baselines import DEFAULT_TICKER_RULES, TickerRuleBaseline
        eng = self.net.eng
        b = TickerRuleBaseline(eng, DEFAULT_TICKER_RULES if rules is None else rules, self.max_episode_steps)
        eng.reset()
        self.baseline_stats = b.run()
        i, rule, total = b.best_total()
        self.baseline_rule, self.baseline_total_reward = (i, rule), total
        return i, rule, total

    def ticker_ceiling(self, horizons=None):
        """The foresight ceiling (goldsrl/baselines.py:TickerForesightCeiling) on the monitor's own Ticker eval engine: resets it and
        plays every (env, horizon) pair in one kernel launch.  The eval engine is reseeded at every reset, so one run before the
        first update holds for every evaluation, as ticker_baseline() does.  Keeps ceiling_total_reward -- the mean over the envs of
        the total reward of the trader who knows every row of its episode, the unit of eval/mean_total_reward --, ceiling_table (one
        (horizon, mean total, mean length, mean trades) row per horizon) and the whole statistics in ceiling_stats; leaves the
        engine reset.  Returns ceiling_total_reward."""
        from ...baselines import DEFAULT_TICKER_HORIZONS, TickerForesightCeiling
        eng = self.net.eng
        c = TickerForesightCeiling(eng, DEFAULT_TICKER_HORIZONS if horizons is None else horizons, self.max_episode_steps)
        eng.reset()
        self.ceiling_stats = c.run()
        self.ceiling_table = c.table()
        self.ceiling_total_reward = c.ceiling()
        return self.ceiling_total_reward

    def ticker_search_baseline(self, generations=8, candidates=32, elites=8, starts=None, tune_table=None, **search_kw):
        """The tuned rule (goldsrl/baselines.py:TickerRuleSearch): the six numbers of the rule family a cross-entropy search finds,
        every generation in one call.  With tune_table (the training table, or its sampler) the search runs on a second eval-style
        engine of the same n_envs on that table and the found rule is then played on the monitor's own engine -- six numbers fitted
        in sample, played out of sample; without it the search runs on the monitor's own engine.  starts: a list of start rules
        (default: the best default rule where the search runs).  Keeps search_baseline_rule, search_baseline_total_reward -- the
        found rule's mean total on the monitor's engine, what evaluations are compared with --,
        search_baseline_in_sample_total_reward -- its fit where it was tuned; the same number without tune_table -- and every
        start's (start, rule, fit) in search_baseline_results; leaves the engine reset.  The scalars of ticker_baseline() and
        ticker_ceiling() are not touched.  Returns (rule, search_baseline_total_reward)."""
        from ...baselines import TickerRuleSearch
        eng = self.net.eng
        tuned_on = eng if tune_table is None else make_ticker_eval_engine(tune_table, self.n_envs, eng.cfg.device_id, self.max_episode_steps)
        try:
            tuned_on.reset()
            b = TickerRuleSearch(tuned_on, starts=starts, generations=generations, candidates=candidates, elites=elites,
                                 max_episode_steps=self.max_episode_steps, **search_kw)
            rule, fit = b.best()
            self.search_baseline_results = b.results
            if tune_table is None:
                total = fit
            else:
                eng.reset()
                total = b.play_on(eng)
        finally:
            if tuned_on is not eng:
                tuned_on.close()
        self.search_baseline_rule, self.search_baseline_total_reward, self.search_baseline_in_sample_total_reward = rule, total, fit
        self._search_tuned_elsewhere = tune_table is not None
        eng.reset()
        return rule, total

    def write_search_baseline_scalars(self, global_step):
        """eval/search_baseline_total_reward and eval/mean_total_reward_minus_search_baseline of the last evaluation (after
        ticker_search_baseline()), and eval/search_baseline_in_sample_total_reward when the rule was tuned on another table"""
        w, total = self.summary_writer, getattr(self, "search_baseline_total_reward", None)
        if w is None or total is None:
            return
        w.add_scalar("eval/search_baseline_total_reward", total, global_step)
        if self.log["mean_total_reward"]:
            w.add_scalar("eval/mean_total_reward_minus_search_baseline", self.log["mean_total_reward"][-1] - total, global_step)
        if self._search_tuned_elsewhere:
            w.add_scalar("eval/search_baseline_in_sample_total_reward", self.search_baseline_in_sample_total_reward, global_step)
        w.flush()


class GridPolicyMonitor(_DeviceMonitor):
    """The PolicyMonitor of the discrete savings-grid agent.  env: the Solow eval registration's id.  n_grid, lb, ub: the
    worker's grid (GridSolowWorker's n_grid, lb, ub).  summary_writer, when given, gets the eval/* scalars through add_scalar.
    net: an evaluation net to use instead of building one (its `eng` is the eval engine)."""

    def __init__(self, env="Solow-1-1-finite-eval-v0", summary_writer=None, n_envs=1, n_grid=51, lb=0.01, ub=0.99, max_seq_length=5,
                 scale=1.0, device_id=0, max_episode_steps=1024, net=None):
        self.env = env
        own = net is None
        if net is None:
            from ... import _ffi_discrete
            if n_envs < 1:
                raise ValueError("n_envs must be at least 1")
            if not env.startswith("Solow-"):
                raise ValueError("the savings-grid agent exists for the Solow env only (got %r)" % (env,))
            eng = make_eval_engine(env, n_envs, device_id, int(max_episode_steps))
            net = _ffi_discrete.DiscreteNet(eng, rnn_length=max_seq_length, scale=scale, num_choices=n_grid, grid_lb=lb, grid_ub=ub,
                                            max_samples=1)
        self._adopt(net, own, summary_writer, max_episode_steps)

    def _baseline_rates(self):
        """The agent's own grid: the best the agent could do blind to the state."""
        return self.net.grid
