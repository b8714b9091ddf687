// Cross-entropy search over the six numbers of a Ticker rule, all G generations enqueued in ONE call (C ABI and the scheme, statement
// by statement: include/goldsrl_tickersearch.h).  Per generation two kernels on the handle's stream, 2 G launches in the call; nothing
// is read back between them and there are no atomics.
//   evaluate  ticker_search_eval_kernel: the sweep's mapping and the sweep's step loop (ticker_sweep_play of ticker_sweep_dev.h, the
//             one copy) over generation g's float32 table in device memory; a pair keeps its running total in a register and stores
//             that one 8-byte score.  No statistics, no trace, no final account.
//   update    ticker_search_update_kernel, one workgroup: the fit of every candidate (a sequential sum over the envs), its rank, the
//             refit of mean and std over the elites, and the next generation's table.  After the last generation it builds none.
// Generation 0's table, mean[0] and std[0] are a function of the arguments alone: the host computes them with the same
// __host__ __device__ statements (ticker_search_dev.h; the clamp and the draw: search_dev.h) and uploads them with the normals.
// The handle's state is read only, and so are the sweep's last results (h->ksw): the search has buffers of its own.
#include <limits.h>
#include <math.h>

#include <vector>

#include "ticker_sweep_dev.h"
#include "ticker_search_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_tickersearch.h"

namespace grl {

// what the search keeps of a pair: statement 5's sequential float64 sum of the float32 step rewards
struct TickerScoreSink {
    double tot = 0.0;
    __device__ __forceinline__ void step(int, const float4, float rew, double) { tot = tot + (double)rew; }
    __device__ __forceinline__ void finish(int, bool, bool, double) {}
};

// The sweep's mapping unchanged: one lane per (env, rule) pair, a wave 64 consecutive envs of one rule, four rules per workgroup; the
// (C, E) scores store coalesced.  Compiled (hipcc -O3, gfx950): 72 VGPRs (the sweep's instance: 86), no LDS, 0 bytes of scratch.
__global__ __launch_bounds__(256) void ticker_search_eval_kernel(TickerParams K, const float *__restrict__ rules, int n_rules, int max_steps,
                                                                 double *__restrict__ scores) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int env = blockIdx.x * 64 + lane;
    const int r = blockIdx.y * 4 + wave;                       // wave-uniform
    if (r >= n_rules || env >= K.E) return;
    const TickerRule U = ticker_rule_load(rules, r);
    TickerScoreSink S;
    ticker_sweep_play(K, U, env, max_steps, S);
    scores[(size_t)r * K.E + env] = S.tot;
}

struct TickerSearchParams {
    const double *z;                              // (G, C, 6): the host's normals
    const double *scores;                         // (G, C, E)
    float *cand;                                  // (G, C, 6)
    double *fit;                                  // (G, C)
    int32_t *order;                               // (G, C)
    double *mean, *std;                           // (G + 1, 6) each
    TickerSearchBox B;
    int E, G, C, K, g;                            // g: the generation just evaluated; this launch builds generation g + 1's table (G: none)
};

// One workgroup of 1 024 lanes, lane c owning candidate c; lanes past C only keep the barriers (every lane reaches all of them: no
// early return).  The fit's scores come through LDS in coalesced tiles (search_fit_sum of search_dev.h; a lane reading its own
// row, 8 bytes at a stride of E * 8, made this kernel a sixth of the call at 8 192 envs x 64 candidates).  The other chains are short
// and latency bound, and there is one workgroup: the kernel exists to keep the generations on the device (measured:
// profiles/ticker_search_times.json).
// Compiled (hipcc -O3, gfx950): 50 VGPRs, 53 344 bytes of LDS (the tile 40 960, fit 8 192, order 4 096, mean and std 96), 0 bytes of
// scratch.
__global__ __launch_bounds__(SEARCH_MAX_C) void ticker_search_update_kernel(TickerSearchParams P) {
    __shared__ double fit_s[SEARCH_MAX_C];
    __shared__ int order_s[SEARCH_MAX_C];
    __shared__ double mean_s[TSEARCH_P], std_s[TSEARCH_P];
    __shared__ double tile_s[SEARCH_TILE_LDS];
    const int c = threadIdx.x, C = P.C, g = P.g;
    const bool mine = c < C;
    const size_t gen = (size_t)g * C;

    const double s = search_fit_sum(P.scores + gen * P.E, C, P.E, c, tile_s);                  // 6 fit
    double f = 0.0;
    if (mine) {
        f = s / (double)P.E;
        P.fit[gen + c] = f;
    }
    search_rank(fit_s, order_s, c, C, f, P.order + gen);                       // 7 rank
    if (c < TSEARCH_P) {                          // 8 refit
        double m, sd;
        search_refit_rows(P.cand + gen * TSEARCH_P, TSEARCH_P, order_s, P.K, c, P.B.floor[c], m, sd);
        mean_s[c] = m;
        std_s[c] = sd;
        P.mean[(size_t)(g + 1) * TSEARCH_P + c] = m;
        P.std[(size_t)(g + 1) * TSEARCH_P + c] = sd;
    }
    __syncthreads();

    if (g + 1 < P.G && mine) {                    // 2-4: generation g + 1's table
        const size_t row = gen + C + c;
        ticker_search_build(P.B, mean_s, std_s, P.z + row * TSEARCH_P, c == 0, P.cand + (gen + order_s[0]) * TSEARCH_P, P.cand + row * TSEARCH_P);
    }
}

static const char *const TSEARCH_NAMES[TSEARCH_P] = {"up0", "up1", "dn0", "dn1", "band", "lookback"};

// the box holds rules only: weights in [0, 1], a band >= 0, a lookback in 0..1023
static int tsearch_check_box(grl_handle *h, const char *fn, const double *std0, const double *floor, const double *lo, const double *hi) {
    const std::string f(fn);
    int rc;
    const struct { const char *noun; const double *v; bool non_negative; } six[] = {{"std0", std0, true}, {"floor", floor, true}, {"lo", lo, false}, {"hi", hi, false}};
    for (const auto &v : six)
        if ((rc = search_check_vector(h, fn, v.noun, v.v, TSEARCH_P, TSEARCH_NAMES, v.non_negative))) return rc;
    for (int k = 0; k < TSEARCH_P; ++k) {
        const std::string i = "[" + std::to_string(k) + "]";
        if (lo[k] > hi[k]) return fail(h, GRL_E_INVALID, f + ": lo" + i + " is above hi" + i + " (" + TSEARCH_NAMES[k] + ")");
        const double top = k < 4 ? 1.0 : (k == 4 ? INFINITY : (double)(TICKER_WINDOW - 1));
        const char *range = k < 4 ? "a weight's box must lie in [0, 1]" : (k == 4 ? "the band's box must not go below 0" : "the lookback's box must lie in 0..1023");
        if (lo[k] < 0.0) return fail(h, GRL_E_INVALID, f + ": lo" + i + " (" + TSEARCH_NAMES[k] + "): " + range);
        if (hi[k] > top) return fail(h, GRL_E_INVALID, f + ": hi" + i + " (" + TSEARCH_NAMES[k] + "): " + range);
    }
    return GRL_OK;
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_ticker_search(grl_handle *h, const float *start, const double *std0, const double *floor, const double *lo, const double *hi,
                      const double *normals, int32_t G, int32_t C, int32_t K, int32_t max_steps) {
    const char *fn = "grl_ticker_search";
    const std::string f(fn);
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_TICKER, "Ticker", start && std0 && floor && lo && hi && normals))) return rc;
    if (!h->tk.table) return fail(h, GRL_E_INVALID, f + ": the handle has no price table yet (grl_ticker_set_table first)");
    if ((rc = search_check_counts(h, fn, G, C, K)) || (rc = episode_check_steps(h, fn, max_steps))) return rc;
    const char *field = nullptr, *what = ticker_rule_fault(start, &field);
    if (what) return fail(h, GRL_E_INVALID, f + ": start: " + field + " " + what);
    if ((rc = tsearch_check_box(h, fn, std0, floor, lo, hi))) return rc;
    const size_t E = (size_t)h->E, gc = (size_t)G * C, scores = E * gc;
    if ((rc = search_check_int32(h, fn, std::max(scores, gc * TSEARCH_P), "fewer envs, generations or candidates per call")) ||
        (rc = search_check_normals(h, fn, normals, gc * TSEARCH_P)) || (rc = episode_check_idle(h, fn)))
        return rc;
    hipSetDevice(h->cfg.device_id);
    TickerSearchState &w = h->kse;
    w.G = 0;
    if ((rc = episode_reserve(h, w.cap_gc, gc, {buf(w.normals, TSEARCH_P), buf(w.cand, TSEARCH_P), buf(w.fit), buf(w.order)})) ||
        (rc = episode_reserve(h, w.cap_scores, scores, {buf(w.scores)})) ||
        (rc = episode_reserve(h, w.cap_gen, (size_t)G + 1, {buf(w.mean, TSEARCH_P), buf(w.std, TSEARCH_P)})))
        return rc;

    TickerSearchParams S{};
    S.z = w.normals; S.scores = w.scores; S.cand = w.cand; S.fit = w.fit; S.order = w.order; S.mean = w.mean; S.std = w.std;
    for (int k = 0; k < TSEARCH_P; ++k) { S.B.floor[k] = floor[k]; S.B.lo[k] = lo[k]; S.B.hi[k] = hi[k]; }
    S.E = h->E; S.G = G; S.C = C; S.K = K;

    double mean0[TSEARCH_P], sd0[TSEARCH_P];      // 1 start, and generation 0's table (2-4)
    for (int k = 0; k < TSEARCH_P; ++k) {
        mean0[k] = search_clamp((double)start[k], lo[k], hi[k]);
        sd0[k] = std0[k];
    }
    std::vector<float> table0((size_t)C * TSEARCH_P);
    for (int c = 0; c < C; ++c)
        ticker_search_build(S.B, mean0, sd0, normals + (size_t)c * TSEARCH_P, c == 0, nullptr, table0.data() + (size_t)c * TSEARCH_P);
    GRL_HIP(h, hipMemcpyAsync(w.normals, normals, gc * TSEARCH_P * 8, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipMemcpyAsync(w.cand, table0.data(), table0.size() * 4, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipMemcpyAsync(w.mean, mean0, sizeof mean0, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipMemcpyAsync(w.std, sd0, sizeof sd0, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipStreamSynchronize(h->stream));  // table0, mean0 and sd0 end with this call: the copies have left them

    const TickerParams P = ticker_params(h);
    const dim3 grid((unsigned)((E + 63) / 64), (unsigned)((C + 3) / 4)), block(256);
    rc = episode_launch(h, [&] {
        for (int g = 0; g < G; ++g) {
            hipLaunchKernelGGL(ticker_search_eval_kernel, grid, block, 0, h->stream, P, (const float *)(w.cand + (size_t)g * C * TSEARCH_P), C,
                               max_steps, w.scores + (size_t)g * C * E);
            S.g = g;
            hipLaunchKernelGGL(ticker_search_update_kernel, dim3(1), dim3(SEARCH_MAX_C), 0, h->stream, S);
        }
    });
    if (rc) return rc;
    w.G = G; w.C = C;
    return GRL_OK;
}

int grl_ticker_search_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const TickerSearchState &w = h->kse;
    const size_t E = (size_t)h->E, gc = (size_t)w.G * w.C, gen = (size_t)w.G + 1;
    const EpisodeOut outs[] = {{"candidates", w.cand, gc * TSEARCH_P * 4}, {"scores", w.scores, gc * E * 8}, {"fit", w.fit, gc * 8},
                               {"order", w.order, gc * 4}, {"mean", w.mean, gen * TSEARCH_P * 8}, {"std", w.std, gen * TSEARCH_P * 8}};
    return episode_read(h, "grl_ticker_search_read", GRL_ENV_TICKER, "Ticker", w.G != 0, "grl_ticker_search", outs, nullptr, which, host, bytes);
}

}  // extern "C"
