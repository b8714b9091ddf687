// Cross-entropy search over the four numbers of a TradeAR1 rule, all G generations enqueued in ONE call (C ABI and the scheme,
// statement by statement: include/goldsrl_tradesearch.h).  Per generation two kernels on the handle's stream, 2 G launches in the
// call; nothing is read back between them and there are no atomics.
//   evaluate  trade_search_eval_kernel: the sweep's mapping, asset tiers and step loop (trade_sweep_play of trade_sweep_dev.h, the
//             one copy) over generation g's float32 table in device memory; a pair keeps its running total in a register and stores
//             that one 8-byte score.  No statistics, no trace, no final account.
//   update    trade_search_update_kernel, one workgroup: the fit of every candidate (a sequential sum over the envs), its rank, the
//             refit of mean and std over the elites, and the next generation's table.  After the last generation it builds none.
// Generation 0's table, mean[0] and std[0] are a function of the arguments alone: the host computes them with the same
// __host__ __device__ statements (trade_search_dev.h; the clamp and the draw: search_dev.h) and uploads them with the normals.
// The handle's state is read only, and so are the last results of the sweep (h->tsw) and the foresight (h->tfs): the search has
// buffers of its own, a tape of its own among them.
#include <limits.h>
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "trade_sweep_dev.h"
#include "trade_search_dev.h"
#include "episode_host.h"
#include "../../include/goldsrl_tradesearch.h"

namespace grl {

// what the search keeps of a lane's RPL pairs: statement 5's sequential float64 sum of the float32 step rewards
template <int RPL>
struct TradeScoreSink {
    double tot[RPL];
    __device__ __forceinline__ void step(int j, int, float rew, double) { tot[j] = tot[j] + (double)rew; }
    __device__ __forceinline__ void finish(int, int, bool, bool, double) {}
};

// The sweep's mapping unchanged: one lane per env, RPL candidates per lane over one price path (pow / exp and the draws once per
// lane), a wave 64 consecutive envs, the waves of a workgroup candidate groups of the SAME 64 envs; the (C, E) scores store
// coalesced along the envs.  A ragged last group (C % RPL != 0) replays the last candidate in its spare slots and stores nothing
// for them.  Up to 16 assets in registers (NT = 2 / 4 / 8 / 16), 17 to 64 in LDS columns, (1 + RPL) * n * 512 bytes per wave:
// 96 KB at 64 assets and RPL 2, so one wave per workgroup there (two at RPL 1, one at RPL 4 with 160 KB).
// Compiled (hipcc -O3, gfx950), VGPRs by NT = 2 / 4 / 8 / 16 / 0 (the sweep's instance in brackets), 0 bytes of scratch throughout:
//   RPL 1: 129 / 161 / 186 / 234 / 129  (136 / 165 / 190 / 238 / 128)
//   RPL 2: 153 / 183 / 216 / 280 / 136  (173 / 213 / 244 / 314 / 153)
//   RPL 4: 201 / 246 / 294 / 388 / 162  (251 / 300 / 344 / 452 / 199)
// No static LDS; the dynamic LDS is the columns above, none with NT > 0.
template <int RPL, int NT>
__global__ __launch_bounds__(256) void trade_search_eval_kernel(TradeParams R, const float *__restrict__ rules, int n_rules,
                                                                const float *__restrict__ tape, int max_steps, double *__restrict__ scores) {
    extern __shared__ double tse_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int env = blockIdx.x * 64 + lane;
    const int r0 = (blockIdx.y * waves + wave) * RPL;          // wave-uniform
    if (r0 >= n_rules || env >= R.E) return;
    TradeRule4 U[RPL];
    TradeScoreSink<RPL> S;
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
        U[j] = trade_rule4_load(rules, r0 + j < n_rules ? r0 + j : n_rules - 1);
        S.tot[j] = 0.0;
    }
    trade_sweep_play<RPL, NT>(R, U, tape, env, tse_lds + (size_t)wave * (1 + RPL) * R.n * 64 + lane, max_steps, S);
#pragma unroll
    for (int j = 0; j < RPL; ++j)
        if (r0 + j < n_rules) scores[(size_t)(r0 + j) * R.E + env] = S.tot[j];
}

struct TradeSearchParams {
    const double *z;                              // (G, C, 4): the host's normals
    const double *scores;                         // (G, C, E)
    float *cand;                                  // (G, C, 4)
    double *fit;                                  // (G, C)
    int32_t *order;                               // (G, C)
    double *mean, *std;                           // (G + 1, 4) each
    TradeSearchBox B;
    int E, G, C, K, g;                            // g: the generation just evaluated; this launch builds generation g + 1's table (G: none)
};

// One workgroup of 1 024 lanes, lane c owning candidate c; lanes past C only keep the barriers (every lane reaches all of them: no
// early return).  The statements are search_dev.h's, as in ticker_search_update_kernel; only the row (trade_search_build) is this
// env's.  Compiled (hipcc -O3, gfx950): 50 VGPRs, 53 312 bytes of LDS (the tile 40 960, fit 8 192,
// order 4 096, mean and std 64), 0 bytes of scratch.
__global__ __launch_bounds__(SEARCH_MAX_C) void trade_search_update_kernel(TradeSearchParams P) {
    __shared__ double fit_s[SEARCH_MAX_C];
    __shared__ int order_s[SEARCH_MAX_C];
    __shared__ double mean_s[TRSEARCH_P], std_s[TRSEARCH_P];
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
    if (c < TRSEARCH_P) {                         // 8 refit
        double m, sd;
        search_refit_rows(P.cand + gen * TRSEARCH_P, TRSEARCH_P, order_s, P.K, c, P.B.floor[c], m, sd);
        mean_s[c] = m;
        std_s[c] = sd;
        P.mean[(size_t)(g + 1) * TRSEARCH_P + c] = m;
        P.std[(size_t)(g + 1) * TRSEARCH_P + c] = sd;
    }
    __syncthreads();

    if (g + 1 < P.G && mine) {                    // 2-4: generation g + 1's table
        const size_t row = gen + C + c;
        trade_search_build(P.B, mean_s, std_s, P.z + row * TRSEARCH_P, c == 0, P.cand + (gen + order_s[0]) * TRSEARCH_P, P.cand + row * TRSEARCH_P);
    }
}

static const char *const TRSEARCH_NAMES[TRSEARCH_P] = {"gain_buy", "gain_sell", "bias", "ref"};

// every number finite, no negative spread or floor, an ordered box whose bounds stay finite as float32: then every row is a rule
static int trsearch_check_box(grl_handle *h, const char *fn, const double *std0, const double *floor, const double *lo, const double *hi) {
    const std::string f(fn);
    int rc;
    const struct { const char *noun; const double *v; bool non_negative; } four[] = {{"std0", std0, true}, {"floor", floor, true}, {"lo", lo, false}, {"hi", hi, false}};
    for (const auto &v : four)
        if ((rc = search_check_vector(h, fn, v.noun, v.v, TRSEARCH_P, TRSEARCH_NAMES, v.non_negative))) return rc;
    for (int k = 0; k < TRSEARCH_P; ++k) {
        const std::string i = "[" + std::to_string(k) + "]";
        if (lo[k] > hi[k]) return fail(h, GRL_E_INVALID, f + ": lo" + i + " is above hi" + i + " (" + TRSEARCH_NAMES[k] + ")");
        if (!std::isfinite((float)lo[k])) return fail(h, GRL_E_INVALID, f + ": lo" + i + " (" + TRSEARCH_NAMES[k] + ") is not finite as float32");
        if (!std::isfinite((float)hi[k])) return fail(h, GRL_E_INVALID, f + ": hi" + i + " (" + TRSEARCH_NAMES[k] + ") is not finite as float32");
    }
    return GRL_OK;
}

// candidates per lane.  Measured at 64 candidates x 1 024 steps x 8 generations, ms per call for 1 / 2 / 4 (profiles/trade_search_times.json):
// 64 envs 19.8 / 26.1 / 39.3 at 2 assets and 132 / 146 / 212 at 16; 4 096 envs 60.5 / 43.2 / 40.1 and 419 / 294 / 214; 8 192 envs
// 116 / 79.3 / 64.7 and 814 / 588 / 427 (1 env x 32 candidates: 62.9 / 73.3 / 94.1 and 411 / 400 / 485).  Where the pairs do not fill
// the device one candidate per lane is the best: more waves, each with the shortest chain; where they do, four are: pow / exp and
// the draws are paid once for four candidates, and unlike the sweep's nine rules 64 candidates leave no idle slot in the last group.
// So the default is the largest of 4 / 2 / 1 that still gives every SIMD of the device (256 CUs x 4) a wave; the measured sizes
// lie on both sides of that line (4 096 envs x 64 candidates at 4 per lane are exactly 1 024 waves) and none between them.
// GRL_TRADE_SEARCH_RPL picks another for that measurement and for the tests.  Every value gives the same bits.
constexpr long TRADE_SEARCH_SIMDS = 256 * 4;
static int trade_search_rpl(int E, int C) {
    const char *v = getenv("GRL_TRADE_SEARCH_RPL");
    if (v && (v[0] == '1' || v[0] == '2' || v[0] == '4') && v[1] == 0) return v[0] - '0';
    const long env_waves = (E + 63) / 64;
    for (int rpl = 4; rpl > 1; rpl /= 2)
        if (env_waves * ((C + rpl - 1) / rpl) >= TRADE_SEARCH_SIMDS) return rpl;
    return 1;
}

using TradeSearchEval = void (*)(TradeParams, const float *, int, const float *, int, double *);

// the evaluation's instantiation for the handle's asset tier, and the launch shape that goes with it
template <int RPL>
static int trade_search_pick(grl_handle *h, int n, int C, TradeSearchEval &kern, dim3 &grid, dim3 &block, size_t &lds) {
    const int groups = (C + RPL - 1) / RPL;
    int waves;
    const size_t per_wave = (size_t)(1 + RPL) * n * 64 * sizeof(double);           // at most 5 * 64 * 512 = 160 KB
    const int rc = trade_tier(h, n, per_wave, waves, lds, [&](auto nt) { return (const void *)(kern = trade_search_eval_kernel<RPL, decltype(nt)::value>); });
    if (rc) return rc;
    grid = dim3((h->E + 63) / 64, (groups + waves - 1) / waves);
    block = dim3(64 * waves);
    return GRL_OK;
}

}  // namespace grl

using namespace grl;

extern "C" {

int grl_trade_search(grl_handle *h, const float *start, const double *std0, const double *floor, const double *lo, const double *hi,
                     const double *normals, const float *tape_host, int32_t G, int32_t C, int32_t K, int32_t max_steps) {
    const char *fn = "grl_trade_search";
    const std::string f(fn);
    int rc;
    if ((rc = episode_open(h, fn, GRL_ENV_TRADE, "TradeAR1", start && std0 && floor && lo && hi && normals))) return rc;
    if ((rc = search_check_counts(h, fn, G, C, K)) || (rc = episode_check_steps(h, fn, max_steps))) return rc;
    for (int k = 0; k < TRSEARCH_P; ++k)
        if (!std::isfinite(start[k])) return fail(h, GRL_E_INVALID, f + ": start: " + TRSEARCH_NAMES[k] + " is not finite");
    if ((rc = trsearch_check_box(h, fn, std0, floor, lo, hi))) return rc;
    const size_t E = (size_t)h->E, gc = (size_t)G * C, scores = E * gc;
    if ((rc = search_check_int32(h, fn, std::max(scores, gc * TRSEARCH_P), "fewer envs, generations or candidates per call")) ||
        (rc = search_check_normals(h, fn, normals, gc * TRSEARCH_P)) || (rc = trade_tape_check(h, fn, tape_host)) ||
        (rc = episode_check_idle(h, fn)))
        return rc;
    hipSetDevice(h->cfg.device_id);
    TradeSearchState &w = h->tse;
    w.G = 0;
    const size_t tape = tape_host ? (size_t)max_steps * h->cfg.n_assets * E : 0;
    if ((rc = episode_reserve(h, w.cap_gc, gc, {buf(w.normals, TRSEARCH_P), buf(w.cand, TRSEARCH_P), buf(w.fit), buf(w.order)})) ||
        (rc = episode_reserve(h, w.cap_scores, scores, {buf(w.scores)})) ||
        (rc = episode_reserve(h, w.cap_gen, (size_t)G + 1, {buf(w.mean, TRSEARCH_P), buf(w.std, TRSEARCH_P)})) ||
        (rc = episode_reserve(h, w.cap_tape, tape, {buf(w.tape)})))
        return rc;

    TradeSearchParams S{};
    S.z = w.normals; S.scores = w.scores; S.cand = w.cand; S.fit = w.fit; S.order = w.order; S.mean = w.mean; S.std = w.std;
    for (int k = 0; k < TRSEARCH_P; ++k) { S.B.floor[k] = floor[k]; S.B.lo[k] = lo[k]; S.B.hi[k] = hi[k]; }
    S.E = h->E; S.G = G; S.C = C; S.K = K;

    double mean0[TRSEARCH_P], sd0[TRSEARCH_P];    // 1 start, and generation 0's table (2-4)
    for (int k = 0; k < TRSEARCH_P; ++k) {
        mean0[k] = search_clamp((double)start[k], lo[k], hi[k]);
        sd0[k] = std0[k];
    }
    std::vector<float> table0((size_t)C * TRSEARCH_P);
    for (int c = 0; c < C; ++c)
        trade_search_build(S.B, mean0, sd0, normals + (size_t)c * TRSEARCH_P, c == 0, nullptr, table0.data() + (size_t)c * TRSEARCH_P);
    GRL_HIP(h, hipMemcpyAsync(w.normals, normals, gc * TRSEARCH_P * 8, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipMemcpyAsync(w.cand, table0.data(), table0.size() * 4, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipMemcpyAsync(w.mean, mean0, sizeof mean0, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipMemcpyAsync(w.std, sd0, sizeof sd0, hipMemcpyHostToDevice, h->stream));
    if (tape) GRL_HIP(h, hipMemcpyAsync(w.tape, tape_host, tape * 4, hipMemcpyHostToDevice, h->stream));
    GRL_HIP(h, hipStreamSynchronize(h->stream));  // table0, mean0 and sd0 end with this call: the copies have left them

    const TradeParams P = trade_params(h);
    const float *tp = tape ? w.tape : nullptr;
    TradeSearchEval kern = nullptr;
    dim3 grid, block;
    size_t lds = 0;
    const int rpl = trade_search_rpl(h->E, C), n = h->cfg.n_assets;
    if (rpl == 1) rc = trade_search_pick<1>(h, n, C, kern, grid, block, lds);
    else if (rpl == 2) rc = trade_search_pick<2>(h, n, C, kern, grid, block, lds);
    else rc = trade_search_pick<4>(h, n, C, kern, grid, block, lds);
    if (rc) return rc;
    rc = episode_launch(h, [&] {
        for (int g = 0; g < G; ++g) {
            hipLaunchKernelGGL(kern, grid, block, lds, h->stream, P, (const float *)(w.cand + (size_t)g * C * TRSEARCH_P), C, tp, max_steps,
                               w.scores + (size_t)g * C * E);
            S.g = g;
            hipLaunchKernelGGL(trade_search_update_kernel, dim3(1), dim3(SEARCH_MAX_C), 0, h->stream, S);
        }
    });
    if (rc) return rc;
    w.G = G; w.C = C;
    return GRL_OK;
}

int grl_trade_search_read(grl_handle *h, const char *which, void *host, size_t bytes) {
    if (!h) return GRL_E_INVALID;
    const TradeSearchState &w = h->tse;
    const size_t E = (size_t)h->E, gc = (size_t)w.G * w.C, gen = (size_t)w.G + 1;
    const EpisodeOut outs[] = {{"candidates", w.cand, gc * TRSEARCH_P * 4}, {"scores", w.scores, gc * E * 8}, {"fit", w.fit, gc * 8},
                               {"order", w.order, gc * 4}, {"mean", w.mean, gen * TRSEARCH_P * 8}, {"std", w.std, gen * TRSEARCH_P * 8}};
    return episode_read(h, "grl_trade_search_read", GRL_ENV_TRADE, "TradeAR1", w.G != 0, "grl_trade_search", outs, nullptr, which, host, bytes);
}

}  // extern "C"
