"""Baselines a trained policy is held against.

ConstantSavingsBaseline is the reference's scripts/constant_solow.py on the device: the seeded eval episode of
`Solow-p-q-finite-eval-v0` once per constant savings rate, every (env, rate) pair in one kernel launch (include/goldsrl_sweep.h).
A policy that does not beat the best constant rate has learned nothing about the shocks.  The selection rules are pure functions of
the statistics, so they run without a device.

OptimalSavingsBaseline is the other end of Solow's scale: the finite-horizon optimum by backward induction on a (k, z, e) grid, one
kernel launch per stage, and the play of the tabulated policy on the same seeded episodes (include/goldsrl_solowdp.h).  The gap
between the two is what there was to learn.  The reference has no counterpart of it.

ScriptedSwarmBaseline gives Swarm the same kind of yardstick: two do-nothing scripts played on a Swarm handle in one kernel launch
(include/goldsrl_replay.h).  The reference has no counterpart of it.

TradingRuleBaseline is TradeAR1's yardstick: a family of mean-reversion rules (gain, bias), every (env, rule) pair in one kernel
launch (include/goldsrl_tradesweep.h).  The reference has no counterpart of it either.

TickerRuleBaseline is the Ticker env's yardstick: banded target-weight rules with an optional trend switch -- hold cash, buy and
hold, a constant mix, follow the trend --, every (env, rule) pair in one kernel launch (include/goldsrl_tickersweep.h).  No
counterpart in the reference either.

TickerForesightCeiling is the other end of the Ticker env's scale: a trader who knows the next H rows of the price table, or every
row of the episode, every (env, horizon) pair in one kernel launch (include/goldsrl_tickerforesight.h).  No counterpart either.

TradeForesightCeiling is the other end of TradeAR1's scale: a trader who knows the next H rows of its price path, or every row of
the episode, every (env, horizon) pair in one call (include/goldsrl_tradeforesight.h).  No counterpart either.

SwarmRuleBaseline is Swarm's closed-loop yardstick: feedback rules that steer the agents relative to the swarm's centroid or to
their nearest locust, every (env, rule) pair in one kernel launch with the action computed on the device
(include/goldsrl_swarmrules.h).  Its first two rules are ScriptedSwarmBaseline's scripts.  No counterpart in the reference.

SwarmRulePlanner is the other end of Swarm's scale: a receding-horizon planner that looks every rule of the same table H steps
ahead, commits the best for K steps and plans again, the whole planned episode in one call (include/goldsrl_swarmplan.h).  No
counterpart either.

SwarmRuleSearch stands between the two: the best FIXED rule a cross-entropy search over the rule's five real numbers finds from
the best rule of the table, every generation of every candidate on every env in one call (include/goldsrl_swarmsearch.h).  A
yardstick that does not depend on what somebody typed into a table.  No counterpart either.

SwarmSearchPlanner is the top of the scale: the planner with the search in the place of its table.  At every decision each env
tunes the rule's five numbers by a short search over lookaheads from where it stands and commits the result unless a rule of the
table looks better, the whole planned episode in one call (include/goldsrl_swarmcemplan.h).  What a controller earns that reacts
AND may pick any rule of the family.  No counterpart either.

TickerRuleSearch is the Ticker env's counterpart of SwarmRuleSearch: the best six numbers of the banded-target rule family a
cross-entropy search finds from the best default rule (or from a list of starts), every generation in one call
(include/goldsrl_tickersearch.h), and that rule played on another engine: tuned on the training table, played on the held-out
one.  No counterpart either.

TradeRuleSearch is TradeAR1's counterpart: the best four numbers (gain_buy, gain_sell, bias, ref) of a rule family that gives each
side of the trade a gain of its own and lets the level prices revert to move, found by a cross-entropy search from the best default
rule (or from a list of starts), every generation in one call (include/goldsrl_tradesearch.h), and that rule played on another
engine: tuned on one set of seeds, played on another.  It stands between TradingRuleBaseline and TradeForesightCeiling.  No
counterpart either."""
import numpy as np

REFERENCE_RATES = np.linspace(0.05, 0.95, 20)       # constant_solow.py:19


def select_best(rates, mean, mx, mn, std):
    """constant_solow.py:16-31 on one env's per-rate statistics, in the order given: s_max = 0, max_mean = 0, stats = None, and a
    rate wins only with a strictly greater mean.  Returns (s_max, max_mean, (max, min, std))."""
    s_max, max_mean, stats = 0, 0, None
    for i, s in enumerate(rates):
        if mean[i] > max_mean:
            max_mean, s_max = mean[i], s
            stats = (mx[i], mn[i], std[i])
    return s_max, max_mean, stats


def select_best_total(rates, total):
    """The rate with the largest mean over the envs of total (n_rates, E) -- the first one on a tie -- and that mean: the unit of
    eval/mean_total_reward."""
    m = np.asarray(total, np.float64).mean(axis=1)
    i = int(np.argmax(m))
    return rates[i], float(m[i])


def _solow_engine(what, env, n_envs, device_id, max_episode_steps, engine):
    """The engine of a Solow baseline: the caller's, or the eval registration's built here.  what: the baseline's name in the
    refusals."""
    if engine is not None:
        from . import _ffi
        if engine.kind != _ffi.ENV_SOLOW:
            raise ValueError("%s exists for the Solow env only" % what)
        return engine
    from .agents.a3c.policy_monitor import make_eval_engine
    if not env.startswith("Solow-"):
        raise ValueError("%s exists for the Solow env only (got %r)" % (what, env))
    if n_envs < 1:
        raise ValueError("n_envs must be at least 1")
    return make_eval_engine(env, n_envs, device_id, max_episode_steps)


class _EngineBaseline(object):
    """What the baselines share: statistics that are played once (_stats, the two Solow classes' too) and, for the six that take
    the caller's engine, the kind check (_open) and the episode length with its default (_steps)."""

    def _open(self, engine, kind, refusal):
        """kind: the name of the env kind in _ffi, e.g. "ENV_SWARM"."""
        from . import _ffi
        if engine.kind != getattr(_ffi, kind):
            raise ValueError(refusal)
        self.eng = engine
        self.stats = None

    def _steps(self, max_episode_steps):
        self.max_episode_steps = int(self.eng.cfg.max_episode_steps if max_episode_steps is None else max_episode_steps)
        if self.max_episode_steps < 1:
            raise ValueError("max_episode_steps must be at least 1 (an engine without a TimeLimit has no default)")

    def _stats(self):
        if self.stats is None:
            self.run()
        return self.stats


class ConstantSavingsBaseline(_EngineBaseline):
    """rates: the constant savings rates, played in this order (the reference's 20 by default).  engine: a Solow engine to run on
    (the caller keeps it) instead of building the eval registration's; run() resets it."""

    def __init__(self, env="Solow-1-1-finite-eval-v0", n_envs=1, rates=REFERENCE_RATES, device_id=0, max_episode_steps=1024, engine=None):
        self.rates = np.asarray(rates, np.float64).reshape(-1)
        if self.rates.size < 1:
            raise ValueError("at least one rate")
        self.max_episode_steps = int(max_episode_steps)
        self._own = engine is None
        self.eng = _solow_engine("the constant-savings baseline", env, n_envs, device_id, self.max_episode_steps, engine)
        self.stats = None

    def run(self, trace_env=None):
        """Reset the envs and play every (env, rate) pair; returns (and keeps) the statistics of _ffi_sweep.solow_sweep."""
        from . import _ffi_sweep
        self.eng.reset()
        self.stats = _ffi_sweep.solow_sweep(self.eng, self.rates, self.max_episode_steps, trace_env)
        return self.stats

    def best(self, env=0):
        """(s_max, max_mean, (max, min, std)) of env's episode by the reference's rule, the step rewards' statistics."""
        s = self._stats()
        s_max, max_mean, stats = select_best(self.rates, s["mean"][:, env], s["max"][:, env], s["min"][:, env], s["std"][:, env])
        return float(s_max), float(max_mean), None if stats is None else tuple(float(v) for v in stats)

    def best_total(self):
        """(rate, mean over the envs of the episode's total reward) of the best rate."""
        return select_best_total(self.rates, self._stats()["total"])

    def close(self):
        if self._own and self.eng is not None:
            self.eng.close()
        self.eng = None


class OptimalSavingsBaseline(_EngineBaseline):
    """The optimal savings policy of a Solow engine with p = 1 and q in {0, 1}: solved once by backward induction on `grid` (a dict
    of _ffi_solowdp.solow_dp_grid; default 96 x 25 x 7 with 96 actions at the engine's sigma) over `horizon` stages (default 256),
    then played on every env from its reset state.  With more steps left than the horizon the policy of stage 0 is used: the
    stationary rule the induction converges to.  engine: a Solow engine to run on (the caller keeps it) instead of building the eval
    registration's; run() resets it."""

    def __init__(self, env="Solow-1-1-finite-eval-v0", n_envs=1, grid=None, horizon=None, device_id=0, max_episode_steps=1024, engine=None):
        from . import _ffi_solowdp
        self.horizon = _ffi_solowdp.DEFAULT_HORIZON if horizon is None else int(horizon)
        if self.horizon < 1:
            raise ValueError("horizon must be at least 1")
        self.max_episode_steps = int(max_episode_steps)
        self._own = engine is None
        self.eng = _solow_engine("the optimal-savings yardstick", env, n_envs, device_id, self.max_episode_steps, engine)
        self.grid = _ffi_solowdp.solow_dp_grid(sigma=self.eng.cfg.solow_sigma) if grid is None else grid
        self.solved, self.stats = False, None

    def solve(self):
        """The backward induction (once per object); the engine keeps the tables."""
        from . import _ffi_solowdp
        if not self.solved:
            _ffi_solowdp.solow_dp_solve(self.eng, self.grid, self.horizon, read=False)
            self.solved = True

    def run(self, trace_steps=0):
        """Solve if not yet solved, reset the envs and play the policy; returns (and keeps) the statistics of
        _ffi_solowdp.solow_dp_play."""
        from . import _ffi_solowdp
        self.solve()
        self.eng.reset()
        self.stats = _ffi_solowdp.solow_dp_play(self.eng, self.max_episode_steps, trace_steps)
        return self.stats

    def total(self):
        """The mean over the envs of the episode's total reward: the unit of eval/mean_total_reward."""
        return float(np.asarray(self._stats()["total"], np.float64).mean())

    def close(self):
        if self._own and self.eng is not None:
            self.eng.close()
        self.eng = None


class ScriptedSwarmBaseline(_EngineBaseline):
    """Two scripted do-nothing policies on a Swarm engine, every (env, script) pair a whole episode in one kernel launch:
      drift   the zero action: the agents go with the wind;
      hold    (-WIND_SPEED, 0): the action cancels the wind and the agents stand still.
    Each script is max_episode_steps float64 rows (default: the engine's TimeLimit).  A policy whose eval/total_reward does not
    beat the better of the two has learned nothing about herding.  The reference has no such baseline (its README shows the GIF of
    one episode and nothing to hold it against): this one is this build's own, like the gated evaluation.  run() plays from the
    engine's CURRENT state (reset it first) and leaves that state as it was."""

    NAMES = ("drift", "hold")

    def __init__(self, engine, max_episode_steps=None):
        self._open(engine, "ENV_SWARM", "the scripted baseline exists for the Swarm env only")
        self._steps(max_episode_steps)
        self.scripts = np.zeros((2, self.max_episode_steps, 10, 2), np.float64)
        self.scripts[1, :, :, 0] = -1.0        # -SwarmEnv.WIND_SPEED

    def run(self):
        """Play both scripts on every env; returns (and keeps) rewards (E, 2, T), totals, length and finished (E, 2)."""
        from .replay import SwarmReplay
        self.stats = SwarmReplay(self.eng).play(self.scripts)
        return self.stats

    def best(self, env=0):
        """(name, total reward) of the better script on `env` -- the first one on a tie"""
        totals = self._stats()["totals"][env]
        i = int(np.argmax(totals))
        return self.NAMES[i], float(totals[i])


# (gain, bias): gains 0 .. 100 at bias 0 -- (0, 0) holds cash -- then fully invested in equal weights, the constant action 1
DEFAULT_TRADE_RULES = np.array([(0, 0), (1, 0), (2, 0), (5, 0), (10, 0), (20, 0), (50, 0), (100, 0), (0, 1)], np.float32)


def select_best_rule(rules, total):
    """The rule with the largest mean over the envs of total (n_rules, E) -- the first one on a tie.  Returns
    (rule_index, (gain, bias), that mean)."""
    m = np.asarray(total, np.float64).mean(axis=1)
    i = int(np.argmax(m))
    return i, (float(rules[i][0]), float(rules[i][1])), float(m[i])


class TradingRuleBaseline(_EngineBaseline):
    """Scripted trading rules on a TradeAR1 engine, every (env, rule) pair a whole episode in one kernel launch
    (include/goldsrl_tradesweep.h).  A rule (gain, bias) trades asset a with the action clip(bias - gain * (p_a - 1), -1, 1): the
    log price is an AR(1) around 0 (fed_env.py:296-298), so a positive gain buys what is cheap and sells what is dear; (0, 0) holds
    cash and (0, b) is the constant action b.  A trader whose eval/total_reward does not beat the best rule has learned less than
    one line of script.  The reference has no such baseline: this one is this build's own, like ScriptedSwarmBaseline.  run() plays
    from the engine's CURRENT state and leaves it as it was; it does not reset -- the price generator's counters move on from one
    episode to the next, so when to reset is the caller's affair."""

    def __init__(self, engine, rules=DEFAULT_TRADE_RULES, max_episode_steps=None):
        self._open(engine, "ENV_TRADE", "the trading-rule baseline exists for the TradeAR1 env only")
        self.rules = np.asarray(rules, np.float32)
        if self.rules.ndim != 2 or self.rules.shape[1] != 2 or self.rules.shape[0] < 1:
            raise ValueError("rules must be (n_rules, 2) of (gain, bias)")
        self._steps(max_episode_steps)

    def run(self, trace_env=None, normals=None):
        """Play every (env, rule) pair; returns (and keeps) the statistics of _ffi_tradesweep.trade_sweep."""
        from . import _ffi_tradesweep
        self.stats = _ffi_tradesweep.trade_sweep(self.eng, self.rules, self.max_episode_steps, trace_env, normals)
        return self.stats

    def best_total(self):
        """(rule_index, (gain, bias), mean over the envs of the episode's total reward) of the best rule."""
        return select_best_rule(self.rules, self._stats()["total"])


# rows of the price path known beyond the one the trade executes at; 0: every row of the episode (the ceiling).  Horizon 64 is
# 23.3 of the default call's 23.5 ms (8 192 envs x 2 assets x 1 024 steps, profiles/trade_foresight_times.json) and earns 7e-9 more
# than horizon 16 there; it stays, as in DEFAULT_TICKER_HORIZONS: the whole call is a tenth of one policy evaluation (228 ms)
DEFAULT_TRADE_HORIZONS = (1, 2, 4, 16, 64, 0)


class TradeForesightCeiling(_EngineBaseline):
    """The other end of TradeAR1's scale: what a trader who knows the coming rows of its price path earns, every (env, horizon)
    pair a whole episode in one call (include/goldsrl_tradeforesight.h).  The price path does not depend on the actions, the
    account is linear in (cash, q) and there is no spread, so the best any policy could have done on an episode is exact: horizon
    0 knows every row and its total is the ceiling of eval/total_reward; a horizon H knows H rows beyond the current one and says
    what that much foresight is worth.  The gap between TradingRuleBaseline's best rule and the ceiling is what there was to
    learn.  The reference has no counterpart.  run() plays from the engine's CURRENT state and leaves it as it was; it does not
    reset -- the price generator's counters move on from one episode to the next, so when to reset is the caller's affair."""

    def __init__(self, engine, horizons=DEFAULT_TRADE_HORIZONS, max_episode_steps=None):
        from ._ffi_tradeforesight import check_trade_horizons
        self._open(engine, "ENV_TRADE", "the foresight ceiling of TradeAR1 exists for the TradeAR1 env only")
        self.horizons = check_trade_horizons(horizons)
        self._steps(max_episode_steps)

    def run(self, trace_env=None, normals=None):
        """Play every (env, horizon) pair; returns (and keeps) the statistics of _ffi_tradeforesight.trade_foresight."""
        from . import _ffi_tradeforesight
        self.stats = _ffi_tradeforesight.trade_foresight(self.eng, self.horizons, self.max_episode_steps, trace_env, normals)
        return self.stats

    def _whole(self):
        whole = np.flatnonzero(self.horizons == 0)
        if len(whole) == 0:
            raise ValueError("the ceiling is the column of horizon 0 (the whole episode), and the horizons hold none")
        return int(whole[0])

    def ceiling(self):
        """The mean over the envs of the whole-episode column's total reward, the unit of eval/mean_total_reward."""
        whole = self._whole()
        return float(self._stats()["total"][whole].mean())

    def bound(self):
        """Every env's bound (E,) float64: no policy's total on that env's episode is above it."""
        whole = self._whole()
        return self._stats()["bound"][whole].copy()

    def table(self):
        """One row per horizon, in the order given: (horizon, mean total reward, mean length, mean trades) over the envs."""
        s = self._stats()
        return [(int(h), float(s["total"][i].mean()), float(s["length"][i].mean()), float(s["trades"][i].mean()))
                for i, h in enumerate(self.horizons)]


class TradeRuleSearch(_EngineBaseline):
    """The best rule of the four-number family near a start: a cross-entropy search over (gain_buy, gain_sell, bias, ref),
    `generations` generations of `candidates` candidates refitted over `elites` elites, every candidate's episode on every env of
    the engine, all enqueued in one call (include/goldsrl_tradesearch.h; the scheme is written there).  starts=None plays
    TradingRuleBaseline over `rules` on the same envs first and starts from its best rule (gain, bias) lifted to (gain, gain, bias,
    1), which is that rule bit for bit; starts: a list of start rules instead, one call per start, the best found rule kept and
    every start's result reported in `results`.  Candidate 0 of every generation is the best so far, so a found rule is never
    below its start on the envs it was tuned on.  Tuned on one engine and played on one with another seed (play_on) it is the
    yardstick "four numbers fitted in sample, played out of sample".  spread, floor, lo, hi: None for
    _ffi_tradesearch.trade_search_defaults of each start.  run() plays from the engine's CURRENT state and leaves it as it was, the
    price generator's counters included; it does not reset.  No counterpart in the reference."""

    def __init__(self, engine, generations=8, candidates=32, elites=8, starts=None, seed=0, spread=None, floor=None, lo=None, hi=None,
                 normals=None, rules=DEFAULT_TRADE_RULES, max_episode_steps=None):
        from ._ffi_tradesearch import check_trade_rule4
        self._open(engine, "ENV_TRADE", "the TradeAR1 rule search exists for the TradeAR1 env only")
        self._steps(max_episode_steps)
        self.starts = None if starts is None else np.array([check_trade_rule4("TradeRuleSearch", r) for r in np.asarray(starts, np.float32).reshape(-1, 4)])
        self.rules = np.asarray(rules, np.float32)
        self.generations, self.candidates, self.elites, self.seed, self.normals = int(generations), int(candidates), int(elites), seed, normals
        self.box = {"spread": spread, "floor": floor, "lo": lo, "hi": hi}
        self.start_total = None                       # the table's best total, when the start came from the table
        self.results = None

    def run(self, tape=None):
        """Search from every start; keeps `results`, one (start, best_rule, best_fit) row per start in the order given, and returns
        (and keeps) the outputs of _ffi_tradesearch.trade_search for the start whose found rule is best (the first on a tie).
        tape: the price normals, as TradingRuleBaseline.run's `normals`."""
        from . import _ffi_tradesearch as S
        if self.starts is None:
            b = TradingRuleBaseline(self.eng, self.rules, self.max_episode_steps)
            b.run(normals=tape)
            _, (gain, bias), self.start_total = b.best_total()
            self.starts = np.array([(gain, gain, bias, 1.0)], np.float32)
        self.results, self.stats = [], None
        for start in self.starts:
            out = S.trade_search(self.eng, start, generations=self.generations, candidates=self.candidates, elites=self.elites,
                                 seed=self.seed, normals=self.normals, max_steps=self.max_episode_steps, tape=tape, **self.box)
            self.results.append((tuple(float(v) for v in start), out["best_rule"], out["best_fit"]))
            if self.stats is None or out["best_fit"] > self.stats["best_fit"]:
                self.stats = out
        return self.stats

    def best(self):
        """((gain_buy, gain_sell, bias, ref), the mean over the envs of its episode's total reward where it was tuned)."""
        s = self._stats()
        return s["best_rule"], s["best_fit"]

    def play_on(self, other_engine, rule=None, tape=None):
        """The mean over the envs of other_engine of the total reward of the found rule (or `rule`), played from that engine's
        CURRENT state for this search's episode length (_ffi_tradesearch.trade_search_play): the found rule out of sample.  The
        mean is the search's fit statement (adds in env order, one division), so on the engine it was tuned on it is best()[1]."""
        from . import _ffi_tradesearch as S
        return S.fit_mean(S.trade_search_play(other_engine, self.best()[0] if rule is None else rule, self.max_episode_steps, tape))


def _ticker_rules():
    rows = [(0, 0, 0, 0, 1, 0), (1, 0, 1, 0, 0.5, 0), (0, 1, 0, 1, 0.5, 0)]
    rows += [(0.5, 0.5, 0.5, 0.5, b, 0) for b in (0.25, 0.05, 0.01)]
    rows += [(1, 0, 0, 1, 0.5, L) for L in (2, 8, 32, 128)]
    rows += [(1, 0, 0, 0, 0.5, L) for L in (8, 32)]
    return np.array(rows, np.float32)


# (up0, up1, dn0, dn1, band, lookback): hold cash; buy and hold the asset; buy and hold the inverse asset; the equal mix rebalanced
# outside a band of 0.25 / 0.05 / 0.01; the asset while the price is at or above its value L rows ago and the inverse asset
# otherwise, L = 2 / 8 / 32 / 128; the same going to cash, L = 8 / 32
DEFAULT_TICKER_RULES = _ticker_rules()


def select_best_ticker_rule(rules, total):
    """select_best_rule for six-parameter rules: the rule with the largest mean over the envs of total (n_rules, E) -- the first
    one on a tie.  Returns (rule_index, (up0, up1, dn0, dn1, band, lookback), that mean)."""
    m = np.asarray(total, np.float64).mean(axis=1)
    i = int(np.argmax(m))
    return i, tuple(float(v) for v in rules[i]), float(m[i])


class TickerRuleBaseline(_EngineBaseline):
    """Scripted rules on a Ticker engine, every (env, rule) pair a whole episode in one kernel launch
    (include/goldsrl_tickersweep.h).  A rule (up0, up1, dn0, dn1, band, lookback) holds target weights of the two assets -- (up0,
    up1) while the price is at or above its value `lookback` rows ago (always, with lookback 0), (dn0, dn1) otherwise -- and trades
    an asset only when its share of the account leaves the band around its target.  The env charges a 0.6 % spread on every trade:
    holding cash totals exactly 0, buying once earns the drift of the window, whatever trades often pays the spread.  A trader
    whose eval/mean_total_reward is below the best rule has learned less than "buy at step 0 and wait".  The reference has no such
    baseline: this one is this build's own, like TradingRuleBaseline.  run() plays from the engine's CURRENT state and leaves it as
    it was; it does not reset."""

    def __init__(self, engine, rules=DEFAULT_TICKER_RULES, max_episode_steps=None):
        from ._ffi_tickersweep import check_ticker_rules
        self._open(engine, "ENV_TICKER", "the Ticker rule baseline exists for the Ticker env only")
        self.rules = check_ticker_rules(rules)
        self._steps(max_episode_steps)

    def run(self, trace_env=None):
        """Play every (env, rule) pair; returns (and keeps) the statistics of _ffi_tickersweep.ticker_sweep."""
        from . import _ffi_tickersweep
        self.stats = _ffi_tickersweep.ticker_sweep(self.eng, self.rules, self.max_episode_steps, trace_env)
        return self.stats

    def best_total(self):
        """(rule_index, the six parameters, mean over the envs of the episode's total reward) of the best rule."""
        return select_best_ticker_rule(self.rules, self._stats()["total"])


# rows of the price table known beyond the one the trade executes at; 0: every row of the episode (the ceiling)
DEFAULT_TICKER_HORIZONS = (1, 2, 4, 16, 64, 0)


class TickerForesightCeiling(_EngineBaseline):
    """The other end of the Ticker env's scale: what a trader who knows the coming rows of the price table earns, every (env,
    horizon) pair a whole episode in one kernel launch (include/goldsrl_tickerforesight.h).  The env is played on a fixed table
    and its account is linear in (cash, q0, q1), so the best any policy could have done on an episode is exact: horizon 0 knows
    every row and its total is the ceiling of eval/total_reward; a horizon H knows H rows beyond the current one and says what
    that much foresight is worth.  The gap between TickerRuleBaseline's best rule and the ceiling is what there was to learn.  The
    reference has no counterpart.  run() plays from the engine's CURRENT state and leaves it as it was; it does not reset."""

    def __init__(self, engine, horizons=DEFAULT_TICKER_HORIZONS, max_episode_steps=None):
        from ._ffi_tickerforesight import check_ticker_horizons
        self._open(engine, "ENV_TICKER", "the foresight ceiling exists for the Ticker env only")
        self.horizons = check_ticker_horizons(horizons)
        self._steps(max_episode_steps)

    def run(self, trace_env=None):
        """Play every (env, horizon) pair; returns (and keeps) the statistics of _ffi_tickerforesight.ticker_foresight."""
        from . import _ffi_tickerforesight
        self.stats = _ffi_tickerforesight.ticker_foresight(self.eng, self.horizons, self.max_episode_steps, trace_env)
        return self.stats

    def ceiling(self):
        """The mean over the envs of the whole-episode column's total reward, the unit of eval/mean_total_reward."""
        whole = np.flatnonzero(self.horizons == 0)
        if len(whole) == 0:
            raise ValueError("the ceiling is the column of horizon 0 (the whole episode), and the horizons hold none")
        return float(self._stats()["total"][whole[0]].mean())

    def table(self):
        """One row per horizon, in the order given: (horizon, mean total reward, mean length, mean trades) over the envs."""
        s = self._stats()
        return [(int(h), float(s["total"][i].mean()), float(s["length"][i].mean()), float(s["trades"][i].mean()))
                for i, h in enumerate(self.horizons)]


class TickerRuleSearch(_EngineBaseline):
    """The best rule of the six-number family near a start: a cross-entropy search over (up0, up1, dn0, dn1, band, lookback),
    `generations` generations of `candidates` candidates refitted over `elites` elites, every candidate's episode on every env of
    the engine, all enqueued in one call (include/goldsrl_tickersearch.h; the scheme is written there).  start=None plays
    TickerRuleBaseline over `rules` on the same envs first and starts from its best rule; starts: a list of start rules instead, one
    call per start, the best found rule kept and every start's result reported in `results`.  Candidate 0 of every generation is
    the best so far, so a found rule is never below its start on the envs it was tuned on.  Tuned on the training table and played
    on a held-out one (play_on) it is the yardstick "six numbers fitted in sample, played out of sample": a trader below it has
    learned less than a curve-fitted script.  spread, floor, lo, hi: None for _ffi_tickersearch.ticker_search_defaults of each
    start.  run() plays from the engine's CURRENT state (reset it first) and leaves that state as it was.  No counterpart in the
    reference."""

    def __init__(self, engine, start=None, starts=None, generations=8, candidates=32, elites=8, seed=0, spread=None, floor=None, lo=None,
                 hi=None, normals=None, rules=DEFAULT_TICKER_RULES, max_episode_steps=None):
        from ._ffi_tickersweep import check_ticker_rules
        self._open(engine, "ENV_TICKER", "the Ticker rule search exists for the Ticker env only")
        self._steps(max_episode_steps)
        if start is not None and starts is not None:
            raise ValueError("give start or starts, not both")
        if starts is not None:
            self.starts = check_ticker_rules(np.asarray(starts, np.float32).reshape(-1, 6))
        else:
            self.starts = None if start is None else check_ticker_rules(np.asarray(start, np.float32).reshape(1, 6))
        self.rules = check_ticker_rules(rules)
        self.generations, self.candidates, self.elites, self.seed, self.normals = int(generations), int(candidates), int(elites), seed, normals
        self.box = {"spread": spread, "floor": floor, "lo": lo, "hi": hi}
        self.start_total = None                       # the table's best total, when the start came from the table
        self.results = None

    def run(self):
        """Search from every start; keeps `results`, one (start, best_rule, best_fit) row per start in the order given, and returns
        (and keeps) the outputs of _ffi_tickersearch.ticker_search for the start whose found rule is best (the first on a tie)."""
        from . import _ffi_tickersearch as S
        if self.starts is None:
            _, six, self.start_total = TickerRuleBaseline(self.eng, self.rules, self.max_episode_steps).best_total()
            self.starts = np.array([six], np.float32)
        self.results, self.stats = [], None
        for start in self.starts:
            out = S.ticker_search(self.eng, start, generations=self.generations, candidates=self.candidates, elites=self.elites,
                                  seed=self.seed, normals=self.normals, max_steps=self.max_episode_steps, **self.box)
            self.results.append((tuple(float(v) for v in start), out["best_rule"], out["best_fit"]))
            if self.stats is None or out["best_fit"] > self.stats["best_fit"]:
                self.stats = out
        return self.stats

    def best(self):
        """((up0, up1, dn0, dn1, band, lookback), the mean over the envs of its episode's total reward where it was tuned)."""
        s = self._stats()
        return s["best_rule"], s["best_fit"]

    def play_on(self, other_engine, rule=None):
        """The mean over the envs of other_engine of the total reward of the found rule (or `rule`), played through
        grl_ticker_sweep from that engine's CURRENT state for this search's episode length: the found rule out of sample.  The
        mean is the search's fit statement (adds in env order, one division), so on the engine it was tuned on it is best()[1]."""
        from . import _ffi_tickersweep
        six = np.array([self.best()[0] if rule is None else rule], np.float32)
        total = _ffi_tickersweep.ticker_sweep(other_engine, six, self.max_episode_steps)["total"][0]
        s = np.float64(0.0)
        for v in total:
            s = s + v
        return float(s / np.float64(len(total)))


def _swarm_rules():
    rows = [(0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0)]
    rows += [(1, g, 0, ox, oy, r) for g in (5, 20) for (ox, oy) in ((0, 0), (-0.5, 0.5), (-1, 1), (-1.5, 1.5)) for r in (0.7, 1.0)]
    rows += [(1, 5, 1, 0, 0, 0), (1, 5, 1, 0.3, -0.3, 0)]
    return np.array(rows, np.float64)


# (cancel, gain, anchor, off_x, off_y, radius): drift; hold; with the wind cancelled, each agent steered to its place on a ring of
# radius 0.7 / 1.0 around the swarm's centroid moved by (0, 0) / (-0.5, 0.5) / (-1, 1) / (-1.5, 1.5) -- up-wind and above --, gain
# 5, then gain 20; each agent steered onto its nearest locust, and to a point (0.3, -0.3) beside it, gain 5
DEFAULT_SWARM_RULES = _swarm_rules()


def select_best_swarm_rule(rules, totals):
    """The rule with the largest mean over the envs of totals (E, n_rules) -- the first one on a tie.  Returns
    (rule_index, (cancel, gain, anchor, off_x, off_y, radius), that mean)."""
    m = np.asarray(totals, np.float64).mean(axis=0)
    i = int(np.argmax(m))
    return i, tuple(float(v) for v in rules[i]), float(m[i])


class SwarmRuleBaseline(_EngineBaseline):
    """Closed-loop feedback rules on a Swarm engine, every (env, rule) pair a whole episode in one kernel launch
    (include/goldsrl_swarmrules.h).  A rule (cancel, gain, anchor, off_x, off_y, radius) steers agent a towards
    anchor + (off_x, off_y) + radius * (cos, sin)(2 pi a / 10) with the action gain * (target - position) - (cancel, 0), clipped to
    norm 1 as the policy's actions are; the anchor is the swarm's centroid (0) or the agent's nearest locust (1).  (0, 0, ...) is
    ScriptedSwarmBaseline's drift and (1, 0, ...) its hold, so the best rule is never below the better script.  At a distance of
    ~2 the locusts are attracted to an agent: agents parked up-wind and above the swarm pull it against wind and gravity, which a
    script that cannot see the swarm cannot do.  A policy whose eval/total_reward does not beat the best rule has learned less than
    six numbers.  The reference has no such baseline: this one is this build's own, like ScriptedSwarmBaseline.  run() plays from
    the engine's CURRENT state (reset it first) and leaves that state as it was."""

    def __init__(self, engine, rules=DEFAULT_SWARM_RULES, max_episode_steps=None):
        from ._ffi_swarmrules import check_swarm_rules
        self._open(engine, "ENV_SWARM", "the Swarm rule baseline exists for the Swarm env only")
        self.rules = check_swarm_rules(rules)
        self._steps(max_episode_steps)

    def run(self, trace_env=None, keep_actions=False):
        """Play every (env, rule) pair; returns (and keeps) the outputs of _ffi_swarmrules.swarm_rules."""
        from . import _ffi_swarmrules
        self.stats = _ffi_swarmrules.swarm_rules(self.eng, self.rules, self.max_episode_steps, keep_actions, trace_env)
        return self.stats

    def best_total(self):
        """(rule_index, the six numbers, mean over the envs of the episode's total reward) of the best rule."""
        return select_best_swarm_rule(self.rules, self._stats()["totals"])


class SwarmRulePlanner(_EngineBaseline):
    """A controller that REACTS, from the same rule table: at every decision each env plays every rule `horizon` steps ahead from
    where it stands, commits the rule with the best sum for `replan` steps and plans again, the whole planned episode enqueued in
    one call (include/goldsrl_swarmplan.h).  Swarm's noise is one fixed row at amplitude 1e-4 after the burn-in (quirk Q1), so the
    env is deterministic from a given state and the lookahead knows nothing a policy could not.  What it earns above the best fixed
    rule is what switching among the rules is worth.  run() plays from the engine's CURRENT state (reset it first) and leaves that
    state as it was.  No counterpart in the reference."""

    def __init__(self, engine, rules=DEFAULT_SWARM_RULES, horizon=8, replan=4, max_episode_steps=None):
        from ._ffi_swarmrules import check_swarm_rules
        self._open(engine, "ENV_SWARM", "the Swarm rule planner exists for the Swarm env only")
        self.rules = check_swarm_rules(rules)
        self.horizon, self.replan = int(horizon), int(replan)
        if not 1 <= self.replan <= self.horizon:
            raise ValueError("1 <= replan <= horizon is required, got horizon %d, replan %d" % (self.horizon, self.replan))
        self._steps(max_episode_steps)

    def run(self, trace_env=None, keep_actions=False):
        """Plan every env's episode; returns (and keeps) the outputs of _ffi_swarmplan.swarm_plan."""
        from . import _ffi_swarmplan
        self.stats = _ffi_swarmplan.swarm_plan(self.eng, self.rules, self.horizon, self.replan, self.max_episode_steps, keep_actions, trace_env)
        return self.stats

    def total(self):
        """The mean over the envs of the planned episode's total reward."""
        return float(self._stats()["totals"].mean())

    def switches(self):
        """The number of decisions, over all envs, whose choice differs from the env's choice before."""
        c = self._stats()["choices"]
        return int(((c[:, 1:] != c[:, :-1]) & (c[:, 1:] >= 0)).sum())


class SwarmRuleSearch(_EngineBaseline):
    """The best fixed rule near a start: a cross-entropy search over (cancel, gain, off_x, off_y, radius) under the start's anchor,
    `generations` generations of `candidates` candidates refitted over `elites` elites, every candidate's episode on every env of
    the engine, all enqueued in one call (include/goldsrl_swarmsearch.h; the scheme is written there).  start=None plays
    SwarmRuleBaseline over `rules` on the same envs first and starts from its best rule: plain refitting from nowhere stalls far
    below the table's best (LABNOTES.md).  Candidate 0 of every generation is the best so far, so the found rule is never below the
    start.  A policy whose eval/mean_total_reward is below it has learned less than five numbers.  run() plays from the engine's
    CURRENT state (reset it first) and leaves that state as it was.  No counterpart in the reference."""

    def __init__(self, engine, start=None, generations=8, candidates=32, elites=8, seed=0, spread=None, floor=None, lo=None, hi=None,
                 normals=None, rules=DEFAULT_SWARM_RULES, max_episode_steps=None):
        from . import _ffi_swarmsearch as S
        self._open(engine, "ENV_SWARM", "the Swarm rule search exists for the Swarm env only")
        self._steps(max_episode_steps)
        self.start = None if start is None else S.check_swarm_rules(np.asarray(start, np.float64).reshape(1, -1))[0]
        self.rules = S.check_swarm_rules(rules)
        self.generations, self.candidates, self.elites, self.seed, self.normals = int(generations), int(candidates), int(elites), seed, normals
        self.box = {"spread": S.DEFAULT_SPREAD if spread is None else spread, "floor": S.DEFAULT_FLOOR if floor is None else floor,
                    "lo": S.DEFAULT_LO if lo is None else lo, "hi": S.DEFAULT_HI if hi is None else hi}
        self.start_total = None                       # the table's best total, when the start came from the table

    def run(self):
        """Search; returns (and keeps) the outputs of _ffi_swarmsearch.swarm_search."""
        from . import _ffi_swarmsearch as S
        if self.start is None:
            _, six, self.start_total = SwarmRuleBaseline(self.eng, self.rules, self.max_episode_steps).best_total()
            self.start = np.array(six, np.float64)
        self.stats = S.swarm_search(self.eng, self.start, generations=self.generations, candidates=self.candidates, elites=self.elites,
                                    seed=self.seed, normals=self.normals, max_steps=self.max_episode_steps, **self.box)
        return self.stats

    def best(self):
        """((cancel, gain, anchor, off_x, off_y, radius), the mean over the envs of its episode's total reward)."""
        s = self._stats()
        return s["best_rule"], s["best_fit"]

    def play_best(self, trace_env=None, keep_actions=False):
        """The found rule played through swarm_rules, so that its episode can be kept: the outputs of _ffi_swarmrules.swarm_rules
        for a table of that one rule."""
        from . import _ffi_swarmrules
        return _ffi_swarmrules.swarm_rules(self.eng, np.array([self.best()[0]], np.float64), self.max_episode_steps, keep_actions, trace_env)


class SwarmSearchPlanner(_EngineBaseline):
    """A controller that reacts and may pick ANY rule of the six-number family: at every decision each env runs `generations`
    generations of `candidates` candidates refitted over `elites` elites around its own mean, every candidate and every rule of
    `rules` played `horizon` steps ahead from where the env stands; the searched rule is committed for `replan` steps if it beats
    the table's best strictly (and becomes the env's mean), else that table rule is; then the env plans again.  The whole planned
    episode of every env is enqueued in one call (include/goldsrl_swarmcemplan.h; the scheme is written there).  start=None plays
    SwarmRuleBaseline over `rules` on the same envs first and starts from its best rule, as SwarmRuleSearch does; the start's anchor
    is the searched rules'.  rules=None: no table, every decision commits a searched rule.  run() plays from the engine's CURRENT
    state (reset it first) and leaves that state as it was.  No counterpart in the reference."""

    def __init__(self, engine, rules=DEFAULT_SWARM_RULES, start=None, horizon=8, replan=4, generations=2, candidates=12, elites=4, seed=0,
                 spread=None, floor=None, lo=None, hi=None, normals=None, max_episode_steps=None):
        from . import _ffi_swarmsearch as S
        self._open(engine, "ENV_SWARM", "the Swarm search planner exists for the Swarm env only")
        self._steps(max_episode_steps)
        self.rules = None if rules is None or len(rules) == 0 else S.check_swarm_rules(rules)
        self.start = None if start is None else S.check_swarm_rules(np.asarray(start, np.float64).reshape(1, -1))[0]
        if self.start is None and self.rules is None:
            raise ValueError("without a table of rules the search planner needs a start")
        self.horizon, self.replan = int(horizon), int(replan)
        if not 1 <= self.replan <= self.horizon:
            raise ValueError("1 <= replan <= horizon is required, got horizon %d, replan %d" % (self.horizon, self.replan))
        self.generations, self.candidates, self.elites, self.seed, self.normals = int(generations), int(candidates), int(elites), seed, normals
        self.box = {"spread": S.DEFAULT_SPREAD if spread is None else spread, "floor": S.DEFAULT_FLOOR if floor is None else floor,
                    "lo": S.DEFAULT_LO if lo is None else lo, "hi": S.DEFAULT_HI if hi is None else hi}
        self.start_total = None                       # the table's best total, when the start came from the table

    def run(self, trace_env=None, keep_actions=False):
        """Plan every env's episode; returns (and keeps) the outputs of _ffi_swarmcemplan.swarm_cemplan."""
        from . import _ffi_swarmcemplan
        if self.start is None:
            _, six, self.start_total = SwarmRuleBaseline(self.eng, self.rules, self.max_episode_steps).best_total()
            self.start = np.array(six, np.float64)
        self.stats = _ffi_swarmcemplan.swarm_cemplan(
            self.eng, self.rules, self.start, self.horizon, self.replan, self.generations, self.candidates, self.elites, seed=self.seed,
            normals=self.normals, max_steps=self.max_episode_steps, keep_actions=keep_actions, trace_env=trace_env, **self.box)
        return self.stats

    def total(self):
        """The mean over the envs of the planned episode's total reward."""
        return float(self._stats()["totals"].mean())

    def searched(self):
        """The number of decisions, over all envs, that committed a searched rule."""
        return int(self._stats()["searched"])
