/* goldsrl_tradesearch.h -- cross-entropy search over the four numbers of a TradeAR1 rule (gain_buy, gain_sell, bias, ref): every
 * generation of every candidate on every env of the handle enqueued in one call (csrc/trade_search.hip).  Nothing is read back
 * between generations; the handle is read only.
 *
 * The rule.  A candidate is a float32 row (gain_buy, gain_sell, bias, ref), widened to float64 on the device.  The action for asset
 * a at price p_a, one IEEE float64 operation per statement:
 *     d = p_a - ref;  g = d < 0.0 ? gain_buy : gain_sell;  m = g * d;  x = bias - m;
 *     x = fmin(fmax(x, -1.0), 1.0);  action_a = (float)x
 * A buy spends a fraction of cash / n, a sale releases a fraction of the holding: the two sides have different units, so each has a
 * gain of its own, and the level prices revert to is a number of the rule (E[p] > 1 for a log-AR(1) around 0).  With gain_buy ==
 * gain_sell and ref == 1.0f these are the statements of grl_trade_sweep's rule (goldsrl_tradesweep.h), and that sub-family gives
 * grl_trade_sweep's bits.  The reference has no counterpart.
 *
 * The scheme.  Everything is float64 unless a cast is written, one IEEE operation per statement (the library is built with
 * -ffp-contract=off).  max(a, b) is a >= b ? a : b and min(a, b) is a <= b ? a : b: the first operand wins a tie, as in
 * goldsrl_swarmsearch.h.  k runs over (gain_buy, gain_sell, bias, ref), g over the G generations, c over the C candidates, e over the
 * E envs of the handle.  The numbering is goldsrl_tickersearch.h's.
 *   1 start      mean[0][k] = min(max((double)start[k], lo[k]), hi[k]);  std[0][k] = std0[k].
 *   2 candidates v = std[g][k] * z[g][c][k];  v = mean[g][k] + v;  v = max(v, lo[k]);  v = min(v, hi[k]).
 *   3 row        f_k = (float)v_k, and nothing more: every four finite float32 numbers are a rule.  (The box bounds must have finite
 *                float32 casts, so every row is finite.)
 *   4 incumbent  candidate 0's row of z is ignored.  In generation 0 it is statement 3 applied to mean[0], the start's own bits when
 *                the start lies in the box; afterwards the best row of the generation before, copied bit for bit.
 *   5 evaluate   score[g][c][e]: s = 0.0; s = s + (double)r_t in step order over the float32 step rewards of (rule = row c, env e)
 *                played from the handle's current state.  The stops are grl_trade_sweep's own -- max_steps, the TimeLimit,
 *                depletion -- and the steps are computed by the sweep's own statements: the two kernels instantiate one loop.
 *   6 fit        s = 0.0; s = s + score[g][c][e] for e in index order;  fit[g][c] = s / (double)E.
 *   7 rank       order[g]: the candidates by fit descending, a tie going to the smaller index.
 *   8 refit      over the K elites p_i = (double)row[order[g][i]], i = 0..K-1 in that order, per k:
 *                m = 0.0; m = m + p_i[k];  mean[g+1][k] = m / (double)K;
 *                s = 0.0; d = p_i[k] - mean[g+1][k]; q = d * d; s = s + q;  v = s / (double)K;  sd = sqrt(v);
 *                std[g+1][k] = max(sd, floor[k]).
 *                A parameter with std0 = floor = 0 whose K-fold sum is exact never moves: ref kept at 1, a bias kept at 0.
 * The normals z come from the host.  For the search the device evaluates sqrt and the float casts, and no other function beyond
 * what the sweep's step already does.  Per generation the evaluation and one single-workgroup kernel (fit, rank, refit, the next
 * generation's table) are enqueued on the handle's stream, 2 G launches in the one call; generation 0's table is built on the host
 * from the same statements.
 *
 * Why a header of its own: goldsrl.h is pinned by tests/test_cabi_symbols.py to declared = exported = bound in _ffi.SIGNATURES.
 * The two functions here are held to the same rule by tests/test_trade_search_header.py against
 * _ffi_tradesearch.TRADESEARCH_SIGNATURES.
 */
#ifndef GOLDSRL_TRADESEARCH_H
#define GOLDSRL_TRADESEARCH_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* start: 4 finite float32.  std0, floor, lo, hi: 4 float64 each over (gain_buy, gain_sell, bias, ref).  normals: (G, C, 4) float64.
 * tape_host: NULL (the handle's own generator, at the counters its next steps would use) or float32 (max_steps, n_assets, E) whose
 * row t moves the prices after step t -- grl_trade_sweep's normals_host; a handle with GRL_F_INJECT_NOISE needs one.  G >= 1
 * generations, 2 <= C <= 1024 candidates, 1 <= K <= C elites, max_steps >= 1.  Plays from the handle's CURRENT state (the caller
 * resets first); the handle's env state, outputs, done list, error counter, generator counters, episode records and the last
 * results of grl_trade_sweep and grl_trade_foresight are untouched.  The generations run async on the handle's stream; the host
 * arrays may be reused on return.
 * GRL_E_INVALID, the message naming the argument and the index: null handle or argument, not a TradeAR1 handle, a start or another
 * number that is not finite, std0 < 0, floor < 0, lo > hi, a box bound whose float32 cast is not finite, a bad G, C, K or max_steps,
 * no tape on a noise-injecting handle, a step in flight, an output of more than 2^31 - 1 elements. */
int grl_trade_search(grl_handle *h, const float *start, const double *std0, const double *floor, const double *lo, const double *hi,
                     const double *normals, const float *tape_host, int32_t G, int32_t C, int32_t K, int32_t max_steps);
/* "candidates" (G,C,4) f32, the rows as played; "scores" (G,C,E) f64; "fit" (G,C) f64; "order" (G,C) i32; "mean" (G+1,4) f64 and
 * "std" (G+1,4) f64, row 0 the clamped start.  Synchronises.  GRL_E_STATE before the first run, GRL_E_SIZE on a wrong byte count,
 * GRL_E_INVALID on an unknown name. */
int grl_trade_search_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_TRADESEARCH_H */
