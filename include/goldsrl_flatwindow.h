/* goldsrl_flatwindow.h -- the flat PAAC policy under the TRUE history window (goldsrl_flatnet.h includes this header; the net, its
 * sizes and its conventions are described there).
 *
 * Replaces (paths relative to the reference repo root):
 *   fed_gym/agents/paac/policy_monitor.py:84-108   SolowPolicyMonitor.eval_once: the window is the last rnn_length states of the episode
 *   fed_gym/agents/a3c/estimators.py:11-15         true_length over rows that differ
 * The PAAC worker (paac/emulator_runner.py:48-63) feeds the net min(n, rnn_length) copies of the current state (quirk Q11), and that
 * is what the rollout, the gradient step and the evaluation do by default.  With the switch on they run the net as the recurrent
 * policy the reference's own monitor evaluates.
 *
 * Window rule: per env the last L = min(k + 1, rnn_length) processed states of the current episode, oldest first, the current
 * state last, zero rows behind; k = steps since the episode's reset.  A step that ends the episode is followed by the reset
 * observation alone (L = 1); a window never spans two episodes.  "nhist" of grl_fnet_read_rollout / grl_fnet_read_eval is L (for
 * Solow "histories" reads the dense true windows).
 *
 * The windows are kept by the net, not the env: the rollout's state buffer has rnn_length - 1 leading time slices, every window is
 * a strided view of it, and the last slices move to the front when the next rollout (or grl_fnet_predict_env) begins.  Windows
 * restart, taking the current observation as their only row,
 *   - for every env at the first call after the switch is set (either way),
 *   - for every env after grl_fnet_eval, which resets the handle,
 *   - for any env whose TimeLimit counter or episode number is not what the net left behind: the host reset or stepped it between
 *     two calls of the net, and THE NET HAS NOT SEEN THE STATES IN BETWEEN.
 * grl_fnet_rollout (both forms, same bits), grl_fnet_predict_env (the window the next rollout's first step would see; it carries
 * the rows forward, so the rollout before it can no longer be trained on or read), grl_fnet_eval and grl_fnet_train_rollout /
 * _grads / apply_grads follow the switch.  The gradient step runs the general forward and backward over the strided windows and
 * recomputes: grl_fnet_set_keep_activations is accepted and ignored.  Windows are not part of a checkpoint.
 *
 * Why a header of its own: tests/test_cabi_symbols.py pins the text of goldsrl_flatnet.h to _ffi_flat.FNET_SIGNATURES.  The two
 * functions here are held to the same rule by tests/test_flat_window_header.py against _ffi_flat.FNET_WINDOW_SIGNATURES.
 */
#ifndef GOLDSRL_FLATWINDOW_H
#define GOLDSRL_FLATWINDOW_H

#include "goldsrl_flatnet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* on != 0: the true window; the default is 0.  GRL_E_INVALID when static_size != temporal_size (the window's rows are the states).
 * Setting it, to either value, drops kept activations and restarts every window. */
int grl_fnet_set_true_window(grl_fnet *net, int32_t on);
/* The dense (count, rnn_length, temporal_size) windows of samples [first, first + count) of the last rollout's flattened
 * (T * num_envs) batch, gathered from the state buffer by the indexing the gradient step uses.  Synchronises.  GRL_E_STATE before
 * a true-window rollout (or once its rows were carried forward), GRL_E_SIZE for a wrong size or range. */
int grl_fnet_read_windows(grl_fnet *net, int32_t first, int32_t count, float *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_FLATWINDOW_H */
