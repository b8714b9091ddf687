/* goldsrl_swarmsearch.h -- cross-entropy search over the five real numbers of a Swarm feedback rule (cancel, gain, off_x, off_y,
 * radius; the anchor is fixed): every generation of every candidate on every env of the handle enqueued in one call
 * (csrc/swarm_search.hip).  Nothing is read back between generations; the handle is read only.
 *
 * A candidate is a rule of grl_swarm_rules (goldsrl_swarmrules.h): a row (cancel, gain, anchor) and an offset table off[10][2], the
 * action of a rule the statements written there.  The reference has no counterpart.
 *
 * The scheme.  Everything is float64, one IEEE operation per statement (the library is built with -ffp-contract=off).  max(a, b) is
 * a >= b ? a : b and min(a, b) is a <= b ? a : b: the first operand wins a tie, which only signed zeros can tell.  k runs over
 * (cancel, gain, off_x, off_y, radius), g over the G generations, c over the C candidates, e over the E envs of the handle.
 *   1 start      mean[0][k] = min(max(mean0[k], lo[k]), hi[k]);  std[0][k] = std0[k].
 *   2 candidates v = std[g][k] * z[g][c][k];  v = mean[g][k] + v;  v = max(v, lo[k]);  v = min(v, hi[k]).
 *   3 incumbent  candidate 0's row of z is ignored: in generation 0 it is mean[0], afterwards the best candidate of the generation
 *                before, copied bit for bit.
 *   4 rows       the rule row is (cancel, gain, anchor);  t = radius * ring[a][0];  off[a][0] = off_x + t;  t = radius * ring[a][1];
 *                off[a][1] = off_y + t.  With ring[a] = (cos, sin)(2 pi a / 10) as the host computes them these are the bytes the
 *                host's offset table has for the six-number row (cancel, gain, anchor, off_x, off_y, radius).
 *   5 evaluate   score[e][g][c]: s = 0.0; s = s + r_t in step order over the rewards of the pair's episode from the handle's current
 *                state, exactly grl_swarm_rules(max_steps): the pair ends after a reward >= 0, at the TimeLimit or after max_steps.  It
 *                is grl_swarm_plan's lookahead score with horizon = max_steps, and the same kernel computes it.
 *   6 fit        s = 0.0; s = s + score[e][g][c] for e in index order;  fit[g][c] = s / (double)E.
 *   7 rank       order[g]: the candidates by fit descending, a tie going to the smaller index.
 *   8 refit      over the K elites p_i = candidate order[g][i], i = 0..K-1 in that order, per k:
 *                m = 0.0; m = m + p_i[k];  mean[g+1][k] = m / (double)K;
 *                s = 0.0; d = p_i[k] - mean[g+1][k]; q = d * d; s = s + q;  v = s / (double)K;  sd = sqrt(v);
 *                std[g+1][k] = max(sd, floor[k]).
 *                A parameter with std0 = floor = 0 whose K-fold sum is exact -- 0, 1, any number of few bits: cancel -- never moves.
 *                (One like 0.7 may come back from m / K an ulp away, with a std of that size.)
 * The device evaluates no transcendental function for the search: the normals z and the ring come from the host.  The handle's Swarm
 * math mode selects the step's arithmetic only.  Per generation the evaluation and one single-workgroup kernel (fit, rank, refit,
 * the next generation's table) are enqueued on the handle's stream, all G generations in the one call.
 *
 * Why a header of its own: goldsrl.h is pinned by tests/test_cabi_symbols.py to declared = exported = bound in _ffi.SIGNATURES.
 * The two functions here are held to the same rule by tests/test_swarm_search_header.py against
 * _ffi_swarmsearch.SWARMSEARCH_SIGNATURES.
 */
#ifndef GOLDSRL_SWARMSEARCH_H
#define GOLDSRL_SWARMSEARCH_H

#include "goldsrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* anchor: 0 (the centroid) or 1 (the agent's nearest locust).  mean0, std0, floor, lo, hi: 5 float64 each over (cancel, gain,
 * off_x, off_y, radius).  ring: (10, 2) float64.  normals: (G, C, 5) float64.  G >= 1 generations, 2 <= C <= 1024 candidates,
 * 1 <= K <= C elites, max_steps >= 1.  Plays from the handle's CURRENT state (the caller resets first); the handle's env state,
 * outputs, episode records and generator counters are untouched.  Async on the handle's stream; the host arrays may be reused on
 * return.
 * GRL_E_INVALID: null handle or argument, not a Swarm handle, an anchor that is not 0 or 1, a number that is not finite, std0 < 0,
 * floor < 0, lo > hi, a bad G, C, K or max_steps, a step in flight, an output of more than 2^31 - 1 elements. */
int grl_swarm_search(grl_handle *h, int32_t anchor, const double *mean0, const double *std0, const double *floor, const double *lo,
                     const double *hi, const double *ring, const double *normals, int32_t G, int32_t C, int32_t K, int32_t max_steps);
/* "candidates" (G,C,6) f64, the six-number rows as played; "offsets" (G,C,10,2) f64; "scores" (E,G,C) f64; "fit" (G,C) f64;
 * "order" (G,C) i32; "mean" (G+1,5) f64 and "std" (G+1,5) f64, row 0 the clamped start.  Synchronises.  GRL_E_STATE before the first
 * run, GRL_E_SIZE on a wrong byte count. */
int grl_swarm_search_read(grl_handle *h, const char *which, void *host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOLDSRL_SWARMSEARCH_H */
