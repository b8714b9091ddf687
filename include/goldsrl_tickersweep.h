/* goldsrl_tickersweep.h -- the scripted rule baseline of the Ticker env: every (env, rule) pair plays a whole episode in one kernel
 * launch (csrc/ticker_sweep.hip).
 *
 * Replaces nothing in the reference: it has no scripted baseline for TickerEnv (fed_gym/envs/fed_env.py:89-158), and no evaluation
 * of the gated trader either.  The rules are this build's own yardstick for the eval/total_reward of grl_gnet_eval, as the TradeAR1
 * rules of goldsrl_tradesweep.h are.
 *
 * A rule is six float32 numbers (up0, up1, dn0, dn1, band, lookback), widened to float64 on the device: a banded target-weight
 * rule with an optional trend switch.  Before every step the pair looks at what the agent's observation shows -- its own cash,
 * q0, q1 and the prices p0, p1 of the row the trade executes at, table[start + idx] -- and, with L = (int)lookback, at
 * back = table[start + max(idx - L, 0)][0].  One IEEE float64 operation per line, no contraction:
 *     up  = (L == 0) || (p0 >= back)
 *     t_a = up ? up_a : dn_a                                  (a = 0, 1)
 *     v0 = q0 * p0;  v1 = q1 * p1;  hold = v0 + v1;  total = cash + hold
 *     per asset a:
 *       s = v_a / total;  lo = t_a - band;  hi = t_a + band
 *       if s < lo:       choice 1 (buy);   d = t_a - s;  w = d * total;  c = fmax(cash, 1e-12);  f = w / c;  f = fmin(f, 1.0)
 *       else if s > hi:  choice 2 (sell);  d = s - t_a;  f = d / s;      f = fmin(f, 1.0)
 *       else:            choice 0 (hold);  f = 0
 *       fraction_a = (float)f
 * The action (choice0, choice1, fraction0, fraction1) then goes through the account arithmetic of grl_step on a Ticker handle,
 * operation for operation, so a pair's account and rewards are the bits the per-step path gives for the rule's actions, and the
 * same lines in numpy float64 (goldsrl/_ffi_tickersweep.py:ticker_rule_actions) give the device's decisions on the host.
 * (0,0,0,0,1,0) holds cash; (1,0,1,0,0.5,0) buys the asset at the first step and never trades again; (.5,.5,.5,.5,b,0) is a constant
 * mix rebalanced outside the band b; (1,0,0,1,0.5,L) holds the asset while p0 is at or above its value L rows ago and the inverse
 * asset otherwise (the switch takes two steps: the env buys from the cash it had before the step's sales).
 *
 * There is no auto-reset.  A pair stops on the first of: max_steps steps played; the env's TimeLimit, counted from the handle's
 * elapsed (finished = 1); assets below 1 (finished = 1, depleted = 1); idx = 1023, where the 1 024-row window holds no row for the
 * observation after a further step and the step path raises its window error (finished = 0).  The sweep never reads outside the
 * window and never raises that error.
 *
 * Why a header of its own: goldsrl_tradesweep.h is pinned to its two functions by tests/test_trade_sweep_header.py.  The two
 * functions here are held to the same rule by tests/test_ticker_sweep_header.py against _ffi_tickersweep.TICKER_SWEEP_SIGNATURES.
 */
#ifndef GOLDSRL_TICKERSWEEP_H
#define GOLDSRL_TICKERSWEEP_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rules_host: (n_rules, 6) float32, 1 <= n_rules <= 4096; max_steps >= 1; trace_env in [-1, E).
 * Plays every (env, rule) pair from the handle's CURRENT state.  The handle's env state, outputs, done list, error counter and
 * episode records are untouched.  Async on the handle's stream (the host array is copied before the call returns).
 * GRL_E_INVALID, with a message that names the rule and the field: null handle or rules, not a Ticker handle, no price table, bad
 * n_rules / max_steps / trace_env, a non-finite parameter, a weight outside [0, 1], up0 + up1 or dn0 + dn1 above 1, band < 0,
 * lookback not an integer in 0..1023, a step in flight. */
int grl_ticker_sweep(grl_handle *h, const float *rules_host, int32_t n_rules, int32_t max_steps, int32_t trace_env);
/* "total" "sum_sq" "final_assets" (n_rules,E) f64 -- total is the sum of the float32 step rewards widened to f64, the unit of
 * grl_gnet_eval's total_reward --; "min" "max" (n_rules,E) f32; "length" "trades" (n_rules,E) i32 (trades: steps on which at least
 * one choice was not hold); "finished" "depleted" (n_rules,E) u8; "trace_rewards" (n_rules,max_steps) f32, "trace_assets"
 * (n_rules,max_steps) f64 and "trace_actions" (n_rules,max_steps,4) f32, zero past the pair's length (GRL_E_STATE without
 * trace_env).  Synchronises.  GRL_E_STATE before the first sweep, GRL_E_SIZE on a wrong byte count, GRL_E_INVALID on an unknown
 * name. */
int grl_ticker_sweep_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_TICKERSWEEP_H */
