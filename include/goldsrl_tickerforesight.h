/* goldsrl_tickerforesight.h -- the ceiling of the Ticker env: what a trader who knows the coming rows of the price table earns.  Every
 * (env, horizon) pair plays a whole episode in one kernel launch (csrc/ticker_foresight.hip).
 *
 * Replaces nothing in the reference: it has neither a baseline nor a ceiling for TickerEnv (fed_gym/envs/fed_env.py:89-158).  The
 * rules of goldsrl_tickersweep.h are the floor under the eval/total_reward of grl_gnet_eval; this is the other end of the scale.
 *
 * The env is played on a fixed price table, and its account arithmetic is linear in (cash, q0, q1), a buy is limited only by the
 * cash at the start of the step and a sale only by the holding.  So under optimal play over the known rows an account is worth
 * cash * A + q0 * B0 + q1 * B1, and the three coefficients obey a backward recurrence over the rows.  A horizon H is 0 (the pair knows
 * every row of its episode: the ceiling) or 1..1023 (it knows H rows beyond the one it trades at).
 *
 * A pair plays n = min(max_steps, max_episode_steps - elapsed (at least 1) if the handle has a TimeLimit, 1023 - idx) steps, the
 * last at row last = idx + n - 1.  At the step of row t the known rows are t..e, e = last for horizon 0 and min(t + H, last)
 * otherwise.  One IEEE float64 operation per statement, no contraction; up = 1 + 0.006 and dn = 1 - 0.006 as the env forms them:
 *     A = 1;  B0 = p0[e];  B1 = p1[e]                         (marked at mid price after the last known row's trade)
 *     for j = e down to t:
 *       a0 = p0[j] * up;  a1 = p1[j] * up;  x0 = B0 / a0;  x1 = B1 / a1
 *       b0 = p0[j] * dn;  b1 = p1[j] * dn;  y0 = b0 * A;   y1 = b1 * A
 *       A' = A, hold;  if x0 > A': A' = x0, buy 0;  if x1 > A': A' = x1, buy 1
 *       if y0 > B0: B0' = y0, sell 0, else B0' = B0;  B1' the same
 *       (A, B0, B1) = (A', B0', B1')
 * Comparisons are strict: hold wins a tie, asset 0 wins a tie with asset 1.  The decisions of j = t are the action: buy a gives
 * choice_a = 1, fraction_a = 1.0f; sell a gives choice_a = 2, fraction_a = 1.0f; anything else 0, 0.0f.  Buy 0 with sell 1 occurs;
 * buy a with sell a cannot (it would need B_a >= up p A > dn p A > B_a).  The action then goes through the account arithmetic of
 * grl_step on a Ticker handle, operation for operation, so a pair's account and rewards are the bits the per-step path gives for
 * these actions, and the same lines in numpy (goldsrl/_ffi_tickerforesight.py:ticker_foresight_actions) give the device's
 * decisions on the host.  Depletion is not modelled in the recurrence: an episode that depletes totals below 0 and holding cash
 * totals exactly 0, so the bound holds over all policies.  The played pair reports `depleted` as the sweep does.
 *
 * The pairs stop as those of grl_ticker_sweep: max_steps, the TimeLimit counted from the handle's elapsed (finished = 1), assets
 * below 1 (finished = 1, depleted = 1), idx = 1023 (finished = 0).  No auto-reset, nothing read outside the window.
 *
 * Why a header of its own: goldsrl_tickersweep.h is pinned to its two functions by tests/test_ticker_sweep_header.py.  The two
 * functions here are held to the same rule by tests/test_ticker_foresight_header.py against
 * _ffi_tickerforesight.TICKER_FORESIGHT_SIGNATURES.
 */
#ifndef GOLDSRL_TICKERFORESIGHT_H
#define GOLDSRL_TICKERFORESIGHT_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* horizons: (n_horizons) int32, 1 <= n_horizons <= 64, each 0 (the whole episode) or 1..1023; max_steps >= 1; trace_env in [-1, E).
 * Plays every (env, horizon) pair from the handle's CURRENT state.  The handle's env state, outputs, done list, error counter and
 * episode records are untouched.  Async on the handle's stream (the host array is copied before the call returns).
 * GRL_E_INVALID, with a message that names the horizon's index: null handle or horizons, not a Ticker handle, no price table, bad
 * n_horizons / max_steps / trace_env, a horizon outside 0..1023, a step in flight. */
int grl_ticker_foresight(grl_handle *h, const int32_t *horizons, int32_t n_horizons, int32_t max_steps, int32_t trace_env);
/* "total" "sum_sq" "final_assets" "bound" (n_horizons,E) f64; "min" "max" (n_horizons,E) f32; "length" "trades" (n_horizons,E) i32;
 * "finished" "depleted" (n_horizons,E) u8; "trace_rewards" (n_horizons,max_steps) f32, "trace_assets" (n_horizons,max_steps) f64
 * and "trace_actions" (n_horizons,max_steps,4) f32, zero past the pair's length (GRL_E_STATE without trace_env): all as in
 * grl_ticker_sweep_read.  "bound": in a horizon-0 column log(((cash * A + q0 * B0) + q1 * B1) + 1e-4) - log(assets + 1e-4) with the
 * coefficients before the first trade -- no policy's total over these n steps is above it --, NaN in every other column.
 * Synchronises.  GRL_E_STATE before the first call, GRL_E_SIZE on a wrong byte count, GRL_E_INVALID on an unknown name. */
int grl_ticker_foresight_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_TICKERFORESIGHT_H */
