/* goldsrl_tickersearch.h -- cross-entropy search over the six numbers of a Ticker rule (up0, up1, dn0, dn1, band, lookback): every
 * generation of every candidate on every env of the handle enqueued in one call (csrc/ticker_search.hip).  Nothing is read back
 * between generations; the handle is read only.
 *
 * A candidate is a rule of grl_ticker_sweep (goldsrl_tickersweep.h): a float32 row with weights in [0, 1], up0 + up1 <= 1,
 * dn0 + dn1 <= 1, a band >= 0 and an integer lookback in 0..1023, the action of a rule the statements written there.  The reference
 * has no counterpart.
 *
 * The scheme.  Everything is float64 unless a cast is written, one IEEE operation per statement (the library is built with
 * -ffp-contract=off).  max(a, b) is a >= b ? a : b and min(a, b) is a <= b ? a : b: the first operand wins a tie, as in
 * goldsrl_swarmsearch.h.  k runs over (up0, up1, dn0, dn1, band, lookback), g over the G generations, c over the C candidates, e over
 * the E envs of the handle.
 *   1 start      mean[0][k] = min(max((double)start[k], lo[k]), hi[k]);  std[0][k] = std0[k].
 *   2 candidates v = std[g][k] * z[g][c][k];  v = mean[g][k] + v;  v = max(v, lo[k]);  v = min(v, hi[k]).
 *   3 row        what makes the six numbers a rule of grl_ticker_sweep.  f_k = (float)v_k for k < 5;  f_5 = (float)rint(v_5), ties
 *                to even.  Then for the pairs (a, b) = (0, 1) and (2, 3):  s = (double)f_a + (double)f_b;  if s > 1.0:
 *                t = 1.0 - (double)f_a;  f_b = (float)t;  s = (double)f_a + (double)f_b;  if s > 1.0: f_b = the next float32 towards
 *                zero (f_b is positive and finite there: its bit pattern minus one).  The second correction is needed -- the cast
 *                alone leaves the sum above 1 for about one f_a in six, e.g. f_a = 0.0027385002f -- and one decrement always suffices.
 *   4 incumbent  candidate 0's row of z is ignored.  In generation 0 it is statement 3 applied to mean[0], the start's own bits when
 *                the start lies in the box; afterwards the best row of the generation before, copied bit for bit.
 *   5 evaluate   score[g][c][e] is the "total" of grl_ticker_sweep for (rule = row c, env e, max_steps) from the handle's current
 *                state: s = 0.0; s = s + (double)r_t in step order over the float32 step rewards.  The stops are the sweep's own --
 *                max_steps, the TimeLimit, depletion, the end of the window -- and the steps are computed by the sweep's own
 *                statements: the two kernels instantiate one loop.
 *   6 fit        s = 0.0; s = s + score[g][c][e] for e in index order;  fit[g][c] = s / (double)E.
 *   7 rank       order[g]: the candidates by fit descending, a tie going to the smaller index.
 *   8 refit      over the K elites p_i = (double)row[order[g][i]], i = 0..K-1 in that order, per k:
 *                m = 0.0; m = m + p_i[k];  mean[g+1][k] = m / (double)K;
 *                s = 0.0; d = p_i[k] - mean[g+1][k]; q = d * d; s = s + q;  v = s / (double)K;  sd = sqrt(v);
 *                std[g+1][k] = max(sd, floor[k]).
 *                A parameter with std0 = floor = 0 whose K-fold sum is exact never moves: a lookback kept fixed, a weight of 0 or 1.
 * The normals z come from the host.  For the search the device evaluates sqrt, rint and the float casts, and no other function
 * beyond what the sweep's step already does.  Per generation the evaluation and one single-workgroup kernel (fit, rank, refit, the
 * next generation's table) are enqueued on the handle's stream, 2 G launches in the one call; generation 0's table is built on the
 * host from the same statements.
 *
 * Why a header of its own: goldsrl.h is pinned by tests/test_cabi_symbols.py to declared = exported = bound in _ffi.SIGNATURES.
 * The two functions here are held to the same rule by tests/test_ticker_search_header.py against
 * _ffi_tickersearch.TICKERSEARCH_SIGNATURES.
 */
#ifndef GOLDSRL_TICKERSEARCH_H
#define GOLDSRL_TICKERSEARCH_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* start: 6 float32, a rule of grl_ticker_sweep.  std0, floor, lo, hi: 6 float64 each over (up0, up1, dn0, dn1, band, lookback).
 * normals: (G, C, 6) float64.  G >= 1 generations, 2 <= C <= 1024 candidates, 1 <= K <= C elites, max_steps >= 1.  Plays from the
 * handle's CURRENT state (the caller resets first); the handle's env state, outputs, done list, error counter, episode records and
 * the last results of grl_ticker_sweep are untouched.  The generations run async on the handle's stream; the host arrays may be
 * reused on return.
 * GRL_E_INVALID, the message naming the argument and the index: null handle or argument, not a Ticker handle, no price table, a start
 * that is no rule of grl_ticker_sweep, a number that is not finite, std0 < 0, floor < 0, lo > hi, a weight's box outside [0, 1], a
 * band's box below 0, a lookback's box outside 0..1023, a bad G, C, K or max_steps, a step in flight, an output of more than
 * 2^31 - 1 elements. */
int grl_ticker_search(grl_handle *h, const float *start, const double *std0, const double *floor, const double *lo, const double *hi,
                      const double *normals, int32_t G, int32_t C, int32_t K, int32_t max_steps);
/* "candidates" (G,C,6) f32, the rows as played; "scores" (G,C,E) f64; "fit" (G,C) f64; "order" (G,C) i32; "mean" (G+1,6) f64 and
 * "std" (G+1,6) f64, row 0 the clamped start.  Synchronises.  GRL_E_STATE before the first run, GRL_E_SIZE on a wrong byte count,
 * GRL_E_INVALID on an unknown name. */
int grl_ticker_search_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_TICKERSEARCH_H */
