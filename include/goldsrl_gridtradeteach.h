/* goldsrl_gridtradeteach.h -- the grid trader (goldsrl_gridtradenet.h, which this header includes: the net, its sizes and its
 * conventions are described there) learning from the attainable optimum's table (goldsrl_tradedp.h): the supervised half of an
 * actor-critic on the device.  A rollout in which the table on the net's handle labels every step, and the update whose policy
 * gradient is the cross-entropy to those labels.
 *
 * The reference has NO counterpart: it has neither the table nor a Trade grid worker.  What is stated here is this library's own.
 *
 * The teacher.  grl_trade_dp_solve / grl_trade_dp_set_policy leave a (horizon, [nu]^2, [nx]^2, 2) table on the handle;
 * grl_trade_dp_play looks it up from the account at every step.  grl_gtnet_teach_rollout makes the SAME look-up (one copy of the
 * statements, csrc/trade_dp_lookup.h) from the handle's raw float64 account before each step, per env:
 *   moves    = max_episode_steps - elapsed - 1 with a TimeLimit, else horizon          price moves left after the step
 *   teacher  = 0 when moves <= 0, else row min(moves, horizon) - 1 of the table at u_a = q_a p_a / W, x_a = log p_a, the 2n-linear
 *              blend (goldsrl_tradedp.h) rounded once to float32
 * It runs inside the forward launch: waves 0 and 1 of a workgroup own the two outputs' softmax and draw for 64 envs, waves 2 and 3,
 * which wait in grl_gtnet_rollout, compute the two outputs' teacher actions for the same envs at the same time.
 *
 * The label.  The teacher's float32 action a of one output becomes a soft label on the net's own grid, in float64, one IEEE
 * operation per statement (goldsrl._ffi_gridtrade.trade_grid_labels is the numpy form):
 *   step = (grid_ub - grid_lb) / (K - 1)
 *   pos  = ((double)a - grid_lb) / step
 *   lo   = clamp((int)floor(pos), 0, K - 2)
 *   w    = (float)clamp(pos - lo, 0, 1)
 * Target mass 1 - w sits on point lo and w on lo + 1: the target's mean is the teacher's action, and an action on a grid point is a
 * one-hot label.
 *
 * The coin.  The agent's own draw is made and stored as in grl_gtnet_rollout ("choices"; the action counter advances alike).  The
 * env is stepped
 *   with probability agent_share  with the agent's grid value (its arg-max's under grl_gtnet_set_greedy)
 *   otherwise                     with the teacher's float32 action as it is, not snapped to the grid
 * One uniform per (env, step), Philox stream id 22:
 *   u, _ = u01_pair(rng_block(seed, e + env_id_offset, action_counter + t, 22, 0));   the agent acts where u < agent_share
 * agent_share = 0 draws nothing and the env follows the teacher exactly; agent_share = 1 draws nothing and steps the env on the
 * agent's own states (on-policy labels).
 *
 * The update.  Per sample with c = grad_mult * weight, y_lo = 1 - w, y_hi = w, per output o:
 *   policy   c * sum_o -(y_lo log(p_lo + 1e-7) + y_hi log(p_hi + 1e-7))               the cross-entropy, in the policy-loss slot
 *   gradient with r_k = y_k * p_k / (p_k + 1e-7):  d/dlogit[o][j] = c * (p[o][j] * (r_lo + r_hi) - r_j)
 *            With w = 0 this is grl_gtnet_train's gradient with adv = 1 and choice = lo.  A term with y_k = 0 adds exactly nothing
 *            and is skipped: 0 * log never appears.
 *   There is no advantage.  Value loss and gradient (on the GAE targets of the rewards the teach rollout collected: the critic is
 *   warm when A3C takes over), the entropy (reported only), the clip, both RMSProp states and the global step's advance by 2 are
 *   grl_gtnet_train's.
 *   agreement  the weighted share of the (sample, output) pairs whose arg-max (first index of the largest float32 probability) is
 *              the label's heavier point: lo + 1 where w > 0.5, else lo (lo on the tie)
 * grl_gtnet_get_grads and the optimizer getters serve these updates as they serve grl_gtnet_train.
 * Conventions as in goldsrl.h.
 */
#ifndef GOLDSRL_GRIDTRADETEACH_H
#define GOLDSRL_GRIDTRADETEACH_H

#include "goldsrl_gridtradenet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* grl_gtnet_rollout with the teacher: windows, records, auto-reset and GAE as ever.  GRL_E_STATE if the net's handle holds no
 * table (no grl_trade_dp_solve or grl_trade_dp_set_policy yet); GRL_E_INVALID for agent_share outside [0, 1] (the message names
 * it).  Afterwards grl_gtnet_read_rollout additionally serves "teacher_actions" (T,E,O) float32, "label_lo" (T,E,O) int32 and
 * "label_w" (T,E,O) float32 -- GRL_E_STATE for these three after a plain grl_gtnet_rollout -- and "actions" are what each env was
 * stepped with.  Async. */
int grl_gtnet_teach_rollout(grl_gtnet *net, int32_t T, double agent_share);
/* the supervised update on the last teach rollout, grad_mult = 1/E.  GRL_E_STATE if the last rollout was a plain one.
 * stats_host (7): cross-entropy, value loss, entropy mean, policy norm, value norm (pre-clip), lr used, agreement. */
int grl_gtnet_train_teach_rollout(grl_gtnet *net, float lr0, float *stats_host);
/* The same update on HOST samples, the counterpart of grl_gtnet_train: label_lo (n,O) int32 in [0, K - 2], label_w (n,O) float32
 * in [0, 1] (GRL_E_INVALID otherwise; the message names the number), targets, weights (n) or NULL (all 1).  stats_host (7). */
int grl_gtnet_teach(grl_gtnet *net, int32_t n, const float *states, const float *windows, const int32_t *label_lo, const float *label_w,
                    const float *targets, const float *weights, float grad_mult, float lr0, int32_t apply_update, float *stats_host);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_GRIDTRADETEACH_H */
