/* goldsrl_sweep.h -- the constant-savings baseline of the Solow env: every (env, rate) pair plays a whole episode in one kernel
 * launch (csrc/solow_sweep.hip).
 *
 * Replaces (paths relative to the reference repo root):
 *   scripts/constant_solow.py:13-33   the eval episode once per constant savings rate, mean / max / min / std of its step rewards
 *
 * One lane keeps one env's state in registers and carries several rates over one shock path (the shocks do not depend on the
 * action).  The step arithmetic is that of grl_step on a Solow handle, operation for operation, so a pair's rewards are the bits
 * the per-step path gives for the constant action.  There is no auto-reset: a pair stops after max_steps steps, at the env's
 * TimeLimit (finished = 1) or when its shock tape is empty (an error, as in the step path).
 *
 * Why a header of its own: goldsrl.h is pinned by tests/test_cabi_symbols.py to declared = exported = bound in _ffi.SIGNATURES.
 * The two functions here are held to the same rule by tests/test_sweep_header.py against _ffi_sweep.SWEEP_SIGNATURES.
 */
#ifndef GOLDSRL_SWEEP_H
#define GOLDSRL_SWEEP_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rates_host: n_rates float32 (1 <= n_rates <= 4096); max_steps >= 1; trace_env in [-1, E).
 * Plays every (env, rate) pair from the handle's CURRENT state (the caller resets first).  The handle's env state,
 * outputs, episode records and generator counters are untouched.  Async on the handle's stream.
 * GRL_E_INVALID: null handle, not a Solow handle, bad argument, a step in flight. */
int grl_solow_sweep(grl_handle *h, const float *rates_host, int32_t n_rates, int32_t max_steps, int32_t trace_env);
/* "total" "sum_sq" (n_rates,E) f64; "min" "max" (n_rates,E) f32; "length" (n_rates,E) i32; "finished" (n_rates,E) u8;
 * "trace_rewards" "trace_k" (n_rates,max_steps) f32, defined up to the pair's length (GRL_E_STATE without trace_env).
 * Synchronises.  GRL_E_STATE before the first sweep, or when a pair ran off its tape. */
int grl_solow_sweep_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_SWEEP_H */
