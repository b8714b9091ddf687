/* goldsrl_tradesweep.h -- the scripted trading-rule baseline of the TradeAR1 env: every (env, rule) pair plays a whole episode in
 * one kernel launch (csrc/trade_sweep.hip).
 *
 * Replaces nothing in the reference: it has no scripted baseline for TradeAR1Env (fed_gym/envs/fed_env.py:262-334).  The rules
 * are this build's own yardstick for eval/total_reward, as the Swarm scripts of goldsrl_replay.h are.
 *
 * A rule is two float32 numbers (gain, bias), widened to float64 on the device.  The action for asset a is computed from the
 * price p_a the trade executes at, one IEEE float64 operation per line:
 *     d = p_a - 1.0;  m = gain * d;  x = bias - m;  x = fmin(fmax(x, -1.0), 1.0);  action_a = (float)x
 * so numpy's clip(float64(bias) - float64(gain) * (p - 1.0), -1, 1).astype(float32) gives the same bits on the host.  (0, 0) holds
 * cash, (0, b) is the constant action b, a positive gain buys what is cheap and sells what is dear: the log price is an AR(1)
 * around 0.  The clamp keeps every action inside the action space, so the step path's range error cannot occur here.
 *
 * One lane keeps one env's prices and the accounts of several rules in registers (LDS columns from 17 assets on) and carries the
 * rules over one price path (the prices do not depend on the actions).  The account and price arithmetic is that of grl_step on a
 * TradeAR1 handle, operation for operation, so a pair's rewards are the bits the per-step path gives for the rule's actions.  There
 * is no auto-reset: a pair stops after max_steps steps, at the env's TimeLimit (finished = 1) or when its assets fall below 1
 * (finished = 1, depleted = 1).
 *
 * Why a header of its own: goldsrl_sweep.h is pinned to its two functions by tests/test_sweep_header.py.  The two functions here
 * are held to the same rule by tests/test_trade_sweep_header.py against _ffi_tradesweep.TRADE_SWEEP_SIGNATURES.
 */
#ifndef GOLDSRL_TRADESWEEP_H
#define GOLDSRL_TRADESWEEP_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gains_host, biases_host: n_rules float32 each (1 <= n_rules <= 4096, all finite); max_steps >= 1; trace_env in [-1, E).
 * normals_host: NULL, or a tape of float32 (max_steps, n_assets, E): step t of the sweep moves the prices with row t instead of
 * the handle's generator, whatever GRL_F_INJECT_NOISE says.  With NULL the generator is used at the counters the handle's next
 * steps would use (a handle with GRL_F_INJECT_NOISE is refused: its buffer holds one step).
 * Plays every (env, rule) pair from the handle's CURRENT state.  The handle's env state, outputs, episode records and generator
 * counters are untouched.  Async on the handle's stream (the host arrays are copied before the call returns).
 * GRL_E_INVALID: null handle or rules, not a TradeAR1 handle, bad argument, a non-finite gain or bias, a step in flight, a
 * noise-injecting handle without a tape. */
int grl_trade_sweep(grl_handle *h, const float *gains_host, const float *biases_host, int32_t n_rules,
                    const float *normals_host, int32_t max_steps, int32_t trace_env);
/* "total" "sum_sq" "final_assets" (n_rules,E) f64; "min" "max" (n_rules,E) f32; "length" (n_rules,E) i32; "finished" "depleted"
 * (n_rules,E) u8; "trace_rewards" (n_rules,max_steps) f32 and "trace_assets" (n_rules,max_steps) f64, zero past the pair's length
 * (GRL_E_STATE without trace_env).  Synchronises.  GRL_E_STATE before the first sweep, GRL_E_SIZE on a wrong byte count,
 * GRL_E_INVALID on an unknown name. */
int grl_trade_sweep_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_TRADESWEEP_H */
