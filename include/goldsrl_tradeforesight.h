/* goldsrl_tradeforesight.h -- the ceiling of the TradeAR1 env: what a trader who knows the coming rows of its price path earns.  Every
 * (env, horizon) pair plays a whole episode in one call (csrc/trade_foresight.hip).
 *
 * Replaces nothing in the reference: it has neither a baseline nor a ceiling for TradeAR1Env (fed_gym/envs/fed_env.py:268-334).  The
 * rules of goldsrl_tradesweep.h are the floor under the eval/total_reward of grl_anet_eval; this is the other end of the scale.
 *
 * The env's account arithmetic is linear in (cash, q_0..q_{n-1}); a buy of asset a is limited only by cash / n of the cash the step
 * began with and a sale only by the holding; there is no spread; and the price path does not depend on the actions -- on the device
 * it is a pure function of (seed, env, step), or of the tape.  So under optimal play over known prices an account is worth
 * cash * A + sum_a q_a * B_a, and the n + 1 coefficients obey a backward recurrence over the rows.  The reward telescopes to
 * log(final + 1e-4) - log(initial + 1e-4), so maximising the final assets maximises the total.  A horizon H is 0 (the pair knows
 * every row of its episode: the ceiling) or 1..1023 (it knows H rows beyond the one it trades at).
 *
 * A pair plays m = min(max_steps, max_episode_steps - elapsed (at least 1) if the handle has a TimeLimit) steps.  Row t of its path,
 * t = 0..m-1, is the price its step t trades at: row 0 is the handle's current p, row t + 1 is _price_transition of row t with the
 * normals the handle's step nstep + t would draw, or with row t of the tape.  last = m - 1.  At step t the known rows are t..e,
 * e = last for horizon 0 and min(t + H, last) otherwise.  One IEEE float64 operation per statement, no contraction:
 *     A = 1;  B_a = p_a[e]                                  (marked at the last known row's price)
 *     for j = e down to t:
 *       for a in order:  x_a = B_a / p_a[j];  y_a = p_a[j] * A
 *       g = 0;  for a in order:  if x_a > A:  d = x_a - A;  g = g + d;   buy a
 *       for a in order:  if y_a > B_a:  B_a = y_a, sell a
 *       s = g / (double)n;  A = A + s
 * Comparisons are strict: hold wins a tie.  Buy a and sell a exclude each other (x_a > A needs B_a > p_a A exactly, and then the
 * rounded product y_a cannot exceed B_a).  The decisions of j = t are the action: buy a gives +1.0f, sell a gives -1.0f, anything
 * else 0.0f.  The action then goes through the account arithmetic of grl_step on a TradeAR1 handle, operation for operation, so a
 * pair's account and rewards are the bits the per-step path gives for these actions, and the same lines in numpy
 * (goldsrl/_ffi_tradeforesight.py:trade_foresight_actions) on the read-back "prices" give the device's decisions on the host.
 * Depletion is not modelled in the recurrence: holding cash is always feasible and totals exactly 0, and an episode that depletes
 * totals below 0, so the bound holds over all policies.  The played pair reports `depleted` as the sweep does.
 *
 * The pairs stop as those of grl_trade_sweep: max_steps, the TimeLimit counted from the handle's elapsed (finished = 1), assets
 * below 1 (finished = 1, depleted = 1).  No auto-reset.
 *
 * Why a header of its own: goldsrl_tradesweep.h and goldsrl_tickerforesight.h are pinned to their functions by
 * tests/test_trade_sweep_header.py and tests/test_ticker_foresight_header.py.  The two functions here are held to the same rule by
 * tests/test_trade_foresight_header.py against _ffi_tradeforesight.TRADE_FORESIGHT_SIGNATURES.
 */
#ifndef GOLDSRL_TRADEFORESIGHT_H
#define GOLDSRL_TRADEFORESIGHT_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* horizons: (n_horizons) int32, 1 <= n_horizons <= 64, each 0 (the whole episode) or 1..1023; max_steps >= 1; trace_env in [-1, E);
 * max_steps * n_assets * E at most 2^28 (the path is kept as float64, the whole-episode plan as a byte per step and asset).
 * normals_host: NULL, or a tape of float32 (max_steps, n_assets, E): row t + 1 of the path is made from row t with row t of the tape
 * instead of the handle's generator, whatever GRL_F_INJECT_NOISE says.  With NULL the generator is used at the counters the handle's
 * next steps would use (a handle with GRL_F_INJECT_NOISE is refused: its buffer holds one step).
 * Plays every (env, horizon) pair from the handle's CURRENT state.  The handle's env state, generator counters, outputs, done list
 * and episode records are untouched.  Async on the handle's stream (the host arrays are copied before the call returns).
 * GRL_E_INVALID, with a message that names the argument and the horizon's index: null handle or horizons, not a TradeAR1 handle, bad
 * n_horizons / max_steps / trace_env, a horizon outside 0..1023, a path over the limit, a noise-injecting handle without a tape, a
 * step in flight. */
int grl_trade_foresight(grl_handle *h, const int32_t *horizons, int32_t n_horizons, const float *normals_host, int32_t max_steps,
                        int32_t trace_env);
/* "total" "sum_sq" "final_assets" "bound" (n_horizons,E) f64; "min" "max" (n_horizons,E) f32; "length" "trades" (n_horizons,E) i32
 * (trades: the steps with a buy or a sale of any asset); "finished" "depleted" (n_horizons,E) u8; "prices" (max_steps,n_assets,E) f64:
 * the path, zero in the rows at or past an env's m; "trace_rewards" (n_horizons,max_steps) f32, "trace_assets"
 * (n_horizons,max_steps) f64 and "trace_actions" (n_horizons,max_steps,n_assets) f32, zero past the pair's length (GRL_E_STATE
 * without trace_env).  "bound": in a horizon-0 column log((cash * A + sum_a q_a * B_a, summed in asset order) + 1e-4) -
 * log(assets + 1e-4) with the coefficients before the first trade -- no policy's total over these m steps is above it --, NaN in
 * every other column.  Synchronises.  GRL_E_STATE before the first call, GRL_E_SIZE on a wrong byte count, GRL_E_INVALID on an
 * unknown name. */
int grl_trade_foresight_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_TRADEFORESIGHT_H */
