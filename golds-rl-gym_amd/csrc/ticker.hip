// TickerEnv on gfx950 (reference fed_gym/envs/fed_env.py:89-158) over an OpenCloseSampler price table
// (fed_gym/envs/data/sampler.py:8-41), with the worker loop body of fed_gym/agents/paac/emulator_runner.py:48-65
// (step, auto-reset, process_state) fused into the same launch and TickerTraderStateProcessor.process_state
// (fed_gym/agents/state_processors.py:50-63) as the processed observation.
//
// Mapping: one env per lane.  The account (cash, equity, two positions) is float64 like the reference's numpy scalars
// and evaluated in the reference's operation order (-ffp-contract=off: +, *, / are bit-exact against numpy); the
// table (rows x 4 float64: price, inverse price, volume, volume) is shared by all envs and stays in cache, each env
// owns a WINDOW-row slice starting at its `start`.  ~190 B of state and outputs per env-step: HBM/latency bound.
#include "ticker_dev.h"

namespace grl {

// the step of every env (ticker_step_env, ticker_dev.h) and the list of the envs it ended
__global__ __launch_bounds__(256) void ticker_step_kernel(TickerParams K) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    bool done = false;
    if (env < K.E) done = ticker_step_env(K, env, reinterpret_cast<const float4 *>(K.actions)[env]).done;
    unsigned long long m = __ballot(done);
    if (m != 0) {
        int lane = threadIdx.x & 63;
        int leader = __ffsll((long long)m) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(K.done_count, __popcll(m));
        base = __shfl(base, leader);
        if (done) K.done_list[base + __popcll(m & ((1ull << lane) - 1ull))] = env;
    }
}

__global__ void ticker_reset_kernel(TickerParams K) {
    const int li = blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= *K.reset_count) return;
    const int env = K.reset_list[li];
    const int st = ticker_reset_env(K, env);
    K.nhist[env] = 0;     // explicit reset: the worker's list starts empty (emulator_runner.py:23)
    ticker_write_obs(K, env, TICKER_START_BALANCE, 0.0, 0.0, K.table + (size_t)st * 4);
}

__global__ void ticker_observe_kernel(TickerParams K) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= K.E) return;
    int st = max(0, min(K.start[env], K.rows - TICKER_WINDOW));
    int idx = max(0, min(K.idx[env], TICKER_WINDOW - 1));
    const double2 qq = reinterpret_cast<const double2 *>(K.q)[env];
    ticker_write_obs(K, env, K.cash[env], qq.x, qq.y, K.table + (size_t)(st + idx) * 4);
}

template <class T>
static int tk_malloc(grl_handle *h, T **p, size_t n) {
    hipError_t e = hipMalloc((void **)p, n * sizeof(T));
    if (e != hipSuccess) return hip_fail(h, e, "hipMalloc");
    h->allocs.push_back(*p);
    e = hipMemsetAsync(*p, 0, n * sizeof(T), h->stream);
    return e == hipSuccess ? GRL_OK : hip_fail(h, e, "hipMemsetAsync");
}

int ticker_alloc(grl_handle *h) {
    size_t E = h->E;
    int rc;
    if ((rc = tk_malloc(h, &h->tk.cash, E)) || (rc = tk_malloc(h, &h->tk.assets, E)) || (rc = tk_malloc(h, &h->tk.q, E * 2)) ||
        (rc = tk_malloc(h, &h->tk.reward64, E)) || (rc = tk_malloc(h, &h->tk.idx, E)) || (rc = tk_malloc(h, &h->tk.start, E)) ||
        (rc = tk_malloc(h, &h->tk.start0, E)) || (rc = tk_malloc(h, &h->tk.nhist, E)) || (rc = tk_malloc(h, &h->tk.obs_raw, E * 7)) ||
        (rc = tk_malloc(h, &h->tk.obs, E * 7)))
        return rc;
    h->tk.table = nullptr;
    h->tk.rows = 0;
    return GRL_OK;
}

int ticker_set_table(grl_handle *h, const double *rows_host, int nrows) {
    if (nrows < TICKER_WINDOW) return fail(h, GRL_E_INVALID, "grl_ticker_set_table: the table needs at least 1024 rows (sampler.py:38 samples windows of 1024)");
    for (size_t i = 0; i < (size_t)nrows * 2; ++i) {
        const double p = rows_host[(i >> 1) * 4 + (i & 1)];
        if (!(p > 0.0)) return fail(h, GRL_E_INVALID, "grl_ticker_set_table: prices must be positive");
    }
    GRL_HIP(h, hipStreamSynchronize(h->stream));
    double *t = nullptr;
    GRL_HIP(h, hipMalloc((void **)&t, (size_t)nrows * 4 * sizeof(double)));
    h->allocs.push_back(t);          // an older table stays allocated until grl_destroy (a step using it may be in flight)
    GRL_HIP(h, hipMemcpy(t, rows_host, (size_t)nrows * 4 * sizeof(double), hipMemcpyHostToDevice));
    h->tk.table = t;
    h->tk.rows = nrows;
    return GRL_OK;
}

static int ticker_ready(grl_handle *h) {
    if (!h->tk.table) return fail(h, GRL_E_STATE, "Ticker handle has no price table yet: call grl_ticker_set_table first");
    return GRL_OK;
}

int ticker_launch_step(grl_handle *h, const float *actions_dev) {
    int rc = ticker_ready(h);
    if (rc) return rc;
    TickerParams K = ticker_params(h);
    K.actions = actions_dev;
    GRL_HIP(h, hipMemsetAsync(h->done_count, 0, sizeof(int32_t), h->stream));
    prof_begin(h);
    hipLaunchKernelGGL(ticker_step_kernel, dim3((h->E + 255) / 256), dim3(256), 0, h->stream, K);
    prof_end(h);
    GRL_HIP(h, hipGetLastError());
    return GRL_OK;
}

int ticker_launch_reset(grl_handle *h, const int32_t *list_dev, const int32_t *count_dev, int max_count) {
    int rc = ticker_ready(h);
    if (rc) return rc;
    TickerParams K = ticker_params(h);
    K.reset_list = list_dev; K.reset_count = count_dev;
    hipLaunchKernelGGL(ticker_reset_kernel, dim3((max_count + 255) / 256), dim3(256), 0, h->stream, K);
    GRL_HIP(h, hipGetLastError());
    return GRL_OK;
}

int ticker_launch_observe(grl_handle *h) {
    int rc = ticker_ready(h);
    if (rc) return rc;
    TickerParams K = ticker_params(h);
    hipLaunchKernelGGL(ticker_observe_kernel, dim3((h->E + 255) / 256), dim3(256), 0, h->stream, K);
    GRL_HIP(h, hipGetLastError());
    return GRL_OK;
}

}  // namespace grl
