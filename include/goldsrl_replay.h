/* goldsrl_replay.h -- scripted episodes of the Swarm env: every (env, action sequence) pair plays its whole script in one kernel
 * launch (csrc/swarm_replay.hip).
 *
 * Replaces (paths relative to the reference repo root):
 *   scripts/make_swarm_gif.py:62-82   the recorded actions of swarm-eval.json stepped through Swarm-eval-v0, positions kept per step
 *
 * A workgroup keeps 4 pairs' points in LDS and registers for the whole episode; the arithmetic is the step's (block_step of
 * csrc/swarm_dev.h), operation for operation, so a pair's rewards and positions are the bits grl_swarm_step_f64 (float64 rows)
 * or grl_step_async (float32 rows, quirk Q7) give for the same rows.  Wind is always added.  There is no auto-reset: a pair ends
 * after the step whose reward is >= 0 or that reaches the env's TimeLimit (finished = 1), or when its script runs out.
 *
 * Why a header of its own: goldsrl.h is pinned by tests/test_cabi_symbols.py to declared = exported = bound in _ffi.SIGNATURES.
 * The two functions here are held to the same rule by tests/test_replay_header.py against _ffi_replay.REPLAY_SIGNATURES.
 */
#ifndef GOLDSRL_REPLAY_H
#define GOLDSRL_REPLAY_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* actions_host: (n_seq, max_steps, 10, 2) shared by every env, or with per_env (E, n_seq, max_steps, 10, 2); float64 if
 * actions_f64, else float32.  1 <= n_seq <= 4096; max_steps >= 1.  seq_len_host: null, or n_seq values in 1..max_steps (rows past
 * a sequence's length are never read).  trace_env in [-1, E): all n_seq sequences of that env are traced.
 * Plays every pair from the handle's CURRENT state (the caller resets first).  The handle's env state, outputs, episode records
 * and generator counters are untouched.  Async on the handle's stream; the host arrays may be reused on return.
 * GRL_E_INVALID: null handle or argument, not a Swarm handle, bad argument, a step in flight, an output of more than 2^31 - 1
 * elements. */
int grl_swarm_replay(grl_handle *h, const void *actions_host, int32_t actions_f64, int32_t n_seq, int32_t max_steps,
                     const int32_t *seq_len_host, int32_t per_env, int32_t trace_env);
/* "rewards" (E,n_seq,max_steps) f64, zero past the pair's length; "length" (E,n_seq) i32; "finished" (E,n_seq) u8;
 * "trace_x" (n_seq,max_steps,80,2) f64 and "trace_xa" (n_seq,max_steps,10,2) f64: the positions after every step of the traced
 * env, zero past the length (GRL_E_STATE without trace_env).  Totals are the host's: np.sum of a rewards row is what the eval
 * monitor reports.  Synchronises.  GRL_E_STATE before the first replay, GRL_E_SIZE on a wrong byte count. */
int grl_swarm_replay_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_REPLAY_H */
