// Internal declarations shared by the translation units of libgoldsrl.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/goldsrl.h"
#include "../../include/goldsrl_solowdp.h"
#include "episode_dev.h"

namespace grl {

constexpr int N_LOCUSTS = 80;   // envs/multiagent.py:8
constexpr int N_AGENTS = 10;    // envs/multiagent.py:9
constexpr int N_POINTS = 90;
constexpr int N_BURN_IN = 10;   // envs/multiagent.py:21
constexpr int SWARM_EPB = 4;    // envs per workgroup: 4*80 = 320 lanes = 5 full waves
constexpr int SWARM_TPB = SWARM_EPB * N_LOCUSTS;

// generator stream ids (ctr[3]); the CPU restatement is oracle/oracle.py:rng_block
enum : uint32_t {
    RS_SWARM_X0 = 0, RS_SWARM_XA0 = 1, RS_SWARM_RANDACT = 2, RS_SWARM_ANOISE = 3, RS_SWARM_PNOISE = 4,
    RS_SOLOW_Z0 = 8, RS_SOLOW_TAPE = 9, RS_TRADE_PRICE = 12, RS_TICKER_START = 16, RS_USER = 64
};

struct SwarmState {
    double *x, *xa, *pnoise, *anoise;              // (E,80,2) (E,10,2) (E,80,2) (E,10,2)
    double *rx, *rxa, *rpnoise, *ranoise;          // reset snapshot (allocated on first use)
    double *reward64;
    double *act64;                                 // staging of grl_swarm_step_f64 (allocated on first use)
    uint8_t *lbins, *abins, *pos;
    bool ref_div;                                  // GRL_SWARM_DIV=ref at grl_create: the exact step with three IEEE divisions per pair
};

struct SolowState {
    float *k, *z, *e, *z0;      // k (E), z (P,E) feature-major, e (Q,E), z0 (P,E)
    float *tape;                // (T,E) time-major
    int32_t *tape_pos, *nhist;
    float *obs_raw, *obs, *history;   // (E,2) (E,2) (E,rnn,2)
    float rho_z[8], rho_e[8];
    int P, Q;                   // storage orders (>=1)
};

struct TradeState {
    double *cash, *assets, *q, *p;    // float64 like the reference's numpy state (the reward is a difference of logs of two
                                      // nearly equal asset values: float32 prices would leave it at 1e-4 relative); q,p (n,E) asset-major
    float *normals;                   // (n,E) injected
    uint32_t *nstep;                  // generator counter per env
    int32_t *nhist;                   // states in the (PAAC-style) worker history list, as SolowState::nhist
    float *obs_raw, *obs;             // (E,1+2n)
    double std_e;
    double start;                     // starting_balance (fed_env.py:269,323-326)
};

struct TickerState {
    double *cash, *assets, *q;        // q (E,2)
    double *reward64;
    int32_t *idx, *start, *start0;    // row inside the window, first row of the window, start restored under SNAPSHOT
    int32_t *nhist;
    float *obs_raw, *obs;             // (E,7)
    const double *table;              // (rows,4) on the device: price, inverse price, volume, volume
    int rows;
};

// The states of the whole-episode launches (host scaffold: episode_host.h).  Every buffer in them is allocated on first use, grown
// (episode_reserve, by the cap_* group the comment beside it names) when a later call is larger, and listed in grl_handle::allocs so
// grl_destroy frees it; the int fields at the end describe the last call and are what grl_*_read sizes its outputs by.  `stats`
// (episode_dev.h) is the six per-pair statistics buffers, of the cap_pairs group (cap_envs in SolowDpState).

// grl_solow_sweep (solow_sweep.hip)
struct SolowSweepState {
    PairStats stats;
    float *rates, *trace_r, *trace_k;             // (cap_rates) (cap_trace) (cap_trace)
    int32_t *err;                                 // (1)
    size_t cap_rates, cap_pairs, cap_trace;
    int n_rates, max_steps, trace_env;            // of the last sweep; n_rates == 0: none yet
};

// grl_trade_sweep (trade_sweep.hip)
struct TradeSweepState {
    PairStats stats;
    float *gains, *biases, *trace_r, *tape;              // (cap_rules) (cap_rules) (cap_trace) (cap_tape)
    double *final_assets, *trace_a;                      // (cap_pairs) (cap_trace)
    uint8_t *depleted;                                   // (cap_pairs)
    size_t cap_rules, cap_pairs, cap_trace, cap_tape;
    int n_rules, max_steps, trace_env;                   // of the last sweep; n_rules == 0: none yet
};

// grl_trade_foresight (trade_foresight.hip)
struct TradeForesightState {
    PairStats stats;
    int32_t *horizons, *trades;                          // (cap_h) (cap_pairs)
    float *trace_r, *trace_act, *tape;                   // (cap_trace) (cap_trace,n) (cap_tape)
    double *final_assets, *bound, *trace_a;              // (cap_pairs) (cap_pairs) (cap_trace)
    double *path;                                        // (cap_path): (max_steps, n, E), the price path of the last call
    uint8_t *depleted, *decisions;                       // (cap_pairs) (cap_dec): (whole columns, max_steps, n, E), horizon 0's plans
    size_t cap_h, cap_pairs, cap_trace, cap_tape, cap_path, cap_dec;
    int n_horizons, max_steps, trace_env;                // of the last call; n_horizons == 0: none yet
};

// grl_trade_search (trade_search.hip); cap_gc counts (generation, candidate) pairs, cap_gen generations + 1
struct TradeSearchState {
    double *normals;                                     // (cap_gc,4): the host's normals
    float *cand;                                         // (cap_gc,4): the rows as played; generation g's table is the evaluation's at g * C
    double *fit;                                         // (cap_gc)
    int32_t *order;                                      // (cap_gc)
    double *scores;                                      // (cap_scores): (G, C, E)
    double *mean, *std;                                  // (cap_gen,4) each
    float *tape;                                         // (cap_tape)
    size_t cap_gc, cap_scores, cap_gen, cap_tape;
    int G, C;                                            // of the last run; G == 0: none yet
};

// grl_ticker_sweep (ticker_sweep.hip)
struct TickerSweepState {
    PairStats stats;
    float *rules, *trace_r, *trace_act;                  // (cap_rules,6) (cap_trace) (cap_trace,4)
    double *final_assets, *trace_a;                      // (cap_pairs) (cap_trace)
    int32_t *trades;                                     // (cap_pairs)
    uint8_t *depleted;                                   // (cap_pairs)
    size_t cap_rules, cap_pairs, cap_trace;
    int n_rules, max_steps, trace_env;                   // of the last sweep; n_rules == 0: none yet
};

// grl_ticker_search (ticker_search.hip); cap_gc counts (generation, candidate) pairs, cap_gen generations + 1
struct TickerSearchState {
    double *normals;                                     // (cap_gc,6): the host's normals
    float *cand;                                         // (cap_gc,6): the rows as played; generation g's table is the evaluation's at g * C
    double *fit;                                         // (cap_gc)
    int32_t *order;                                      // (cap_gc)
    double *scores;                                      // (cap_scores): (G, C, E)
    double *mean, *std;                                  // (cap_gen,6) each
    size_t cap_gc, cap_scores, cap_gen;
    int G, C;                                            // of the last run; G == 0: none yet
};

// grl_ticker_foresight (ticker_foresight.hip)
struct TickerForesightState {
    PairStats stats;
    int32_t *horizons, *trades;                          // (cap_h) (cap_pairs)
    float *trace_r, *trace_act;                          // (cap_trace) (cap_trace,4)
    double *final_assets, *bound, *trace_a;              // (cap_pairs) (cap_pairs) (cap_trace)
    uint8_t *depleted, *decisions;                       // (cap_pairs) (cap_dec): (max_steps, pairs), horizon 0's plan
    size_t cap_h, cap_pairs, cap_trace, cap_dec;
    int n_horizons, max_steps, trace_env;                // of the last call; n_horizons == 0: none yet
};

// grl_solow_dp_* (solow_dp.hip): the tables of the solve and the buffers of the play
struct SolowDpState {
    grl_solow_dp_grid grid;                       // of the table in `policy`
    double rho, theta;                            // the model the last solve used
    double *v[2];                                 // (cap_states) each; stage t's value is in v[t & 1]
    float *policy;                                // (cap_table): (horizon, nk, nz, ne)
    size_t cap_states, cap_table;
    int horizon, ne;                              // horizon == 0: no table yet
    bool has_value;                               // v[0] holds stage 0's value (a solve, not a set_policy)
    PairStats stats;                              // a pair is an env here
    float *trace_a, *trace_r, *trace_k;           // (cap_trace) x 3
    int32_t *err;                                 // (1)
    size_t cap_envs, cap_trace;
    int played, trace_steps;                      // of the last play; played == 0: none yet
};

// grl_swarm_replay (swarm_replay.hip)
struct SwarmReplayState {
    uint8_t *actions;                             // (cap_act) bytes: the float64 or float32 action rows
    int32_t *seq_len, *length;                    // (cap_seq) (cap_pairs)
    double *rewards, *trace_x, *trace_xa;         // (cap_steps) (cap_trace,80,2) (cap_trace,10,2)
    uint8_t *finished;                            // (cap_pairs)
    size_t cap_act, cap_seq, cap_steps, cap_pairs, cap_trace;
    int n_seq, max_steps, trace_env;              // of the last replay; n_seq == 0: none yet
};

// grl_swarm_rules (swarm_rules.hip)
struct SwarmRulesState {
    double *rules, *offsets;                      // (cap_rules,3) (cap_rules,10,2)
    double *rewards, *actions;                    // (cap_steps) (cap_act,10,2)
    double *trace_x, *trace_xa;                   // (cap_trace,80,2) (cap_trace,10,2)
    int32_t *length;                              // (cap_pairs)
    uint8_t *finished;                            // (cap_pairs)
    size_t cap_rules, cap_steps, cap_pairs, cap_act, cap_trace;
    int n_rules, max_steps, trace_env, keep_actions;   // of the last run; n_rules == 0: none yet
};

// grl_swarm_plan (swarm_plan.hip)
struct SwarmPlanState {
    double *rules, *offsets;                      // (cap_rules,3) (cap_rules,10,2)
    double *x, *xa;                               // (cap_envs,80,2) (cap_envs,10,2): the plan's working copy of the positions
    int32_t *length;                              // (cap_envs): steps played; the plan's clock
    uint8_t *finished;                            // (cap_envs)
    double *rewards, *actions;                    // (cap_steps) (cap_act,10,2)
    double *trace_x, *trace_xa;                   // (cap_trace,80,2) (cap_trace,10,2)
    int32_t *choices;                             // (cap_dec): (E, decisions)
    double *scores;                               // (cap_scores): (E, decisions, n_rules)
    size_t cap_rules, cap_envs, cap_steps, cap_act, cap_trace, cap_dec, cap_scores;
    int n_rules, max_steps, decisions, trace_env, keep_actions;   // of the last run; n_rules == 0: none yet
};

// grl_swarm_search (swarm_search.hip); cap_gc counts (generation, candidate) pairs, cap_gen generations + 1
struct SwarmSearchState {
    double *normals, *cand;                       // (cap_gc,5) (cap_gc,6): the host's normals; the six-number rows as played
    double *rules, *offsets;                      // (cap_gc,3) (cap_gc,10,2): generation g's table is the lookahead's at g * C
    double *fit;                                  // (cap_gc)
    int32_t *order;                               // (cap_gc)
    double *scores;                               // (cap_scores): (E, G, C)
    double *mean, *std;                           // (cap_gen,5) each
    int32_t *length;                              // (cap_envs): zero, the lookahead's clock
    uint8_t *finished;                            // (cap_envs): zero
    size_t cap_gc, cap_scores, cap_gen, cap_envs;
    int G, C;                                     // of the last run; G == 0: none yet
};

// grl_swarm_cemplan (swarm_cemplan.hip); T = C + n_rules rows per env in the working table
struct SwarmCemPlanState {
    double *lib_rules, *lib_offsets;              // (cap_rules,3) (cap_rules,10,2): the library as uploaded
    double *normals;                              // (cap_z,5): (D, G, C, 5)
    double *x, *xa;                               // (cap_envs,80,2) (cap_envs,10,2): the call's working copy of the positions
    int32_t *length, *pick;                       // (cap_envs): steps committed, the call's clock; the commit's own choice (always 0)
    uint8_t *finished;                            // (cap_envs)
    double *cur_mean, *one;                       // (cap_envs,5): the env's mean between decisions; (cap_envs): the commit's one score
    double *rewards, *actions;                    // (cap_steps) (cap_act,10,2)
    double *trace_x, *trace_xa;                   // (cap_trace,80,2) (cap_trace,10,2)
    double *table_rules, *table_offsets;          // (cap_table,3) (cap_table,10,2): (E, T), the generation's candidates, then the library
    int32_t *choices;                             // (cap_dec): (E, D)
    double *chosen_rules, *chosen_offsets;        // (cap_dec,3) (cap_dec,10,2): the commit's table, one row per env and decision
    double *look0;                                // (cap_look0): (E, D, T), generation 0's scores and the library's from one launch
    double *lib_scores;                           // (cap_lib): (E, D, n_rules)
    double *cand, *scores;                        // (cap_gc,6) (cap_gc): (E, D, G, C)
    int32_t *order;                               // (cap_gc)
    double *mean, *std;                           // (cap_gen,5) each: (E, D, G + 1)
    size_t cap_rules, cap_z, cap_envs, cap_steps, cap_act, cap_trace, cap_table, cap_dec, cap_look0, cap_lib, cap_gc, cap_gen;
    int n_rules, max_steps, decisions, G, C, trace_env, keep_actions;   // of the last run; C == 0: none yet
};

}  // namespace grl

struct grl_handle {
    grl_config cfg;
    int E;
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    std::string err;
    bool step_in_flight;
    // common per-env
    int32_t *elapsed, *episode;
    float *reward;
    uint8_t *done;
    int32_t *done_list, *done_count;
    int32_t *err_flag;            // device-side deferred error counter (Trade action range)
    float *actions;               // staging for grl_step_async
    size_t actions_elems;
    grl::SwarmState sw;
    grl::SolowState so;
    grl::TradeState tr;
    grl::TickerState tk;
    grl::SolowSweepState swp;
    grl::SwarmReplayState rpl;
    grl::SwarmRulesState srl;
    grl::SwarmPlanState spl;
    grl::SwarmSearchState ssr;
    grl::SwarmCemPlanState scp;
    grl::TradeSweepState tsw;
    grl::TradeForesightState tfs;
    grl::TradeSearchState tse;
    grl::TickerSweepState ksw;
    grl::TickerSearchState kse;
    grl::TickerForesightState kfs;
    grl::SolowDpState sdp;
    std::vector<void *> allocs;   // everything hipMalloc'ed by the handle
    std::vector<void *> user_allocs;
    // R6 episode bookkeeping (grl_episodes_*): nullptr until enabled
    double *ep_total;
    int32_t *ep_len;
    int64_t *ep_steps;
    grl_episode_record *ep_rec;
    int32_t *ep_count;
    int32_t ep_capacity;
    // per-kernel profiling (grl_profile_*)
    bool prof_on;
    std::vector<hipEvent_t> prof_ev;   // pairs
    size_t prof_used;
};

namespace grl {
int fail(grl_handle *h, int code, const std::string &msg);
// Is h a handle grl_create returned and grl_destroy has not freed?  A net keeps a pointer to the handle it was created on; a
// host binding's garbage collector may finalise the two in either order, so the grl_*net_destroy functions ask before they
// touch the handle's device id and stream.
bool grl_handle_alive(const grl_handle *h);
// binds the handle's device and drains its stream if the handle is alive, else drains the current device
void grl_sync_for_destroy(grl_handle *h);
// bracket the dominant kernel of a step with an event pair when profiling is on
void prof_begin(grl_handle *h);
void prof_end(grl_handle *h);
int hip_fail(grl_handle *h, hipError_t e, const char *what);
#define GRL_HIP(h, call)                                        \
    do {                                                        \
        hipError_t _e = (call);                                 \
        if (_e != hipSuccess) return grl::hip_fail(h, _e, #call); \
    } while (0)

// (re)allocate *p to n elements and keep grl_handle::allocs right; the old contents are dropped
template <typename T>
static int grow(grl_handle *h, T **p, size_t n) {
    if (*p) {
        auto it = std::find(h->allocs.begin(), h->allocs.end(), (void *)*p);
        if (it != h->allocs.end()) h->allocs.erase(it);
        GRL_HIP(h, hipFree(*p));
        *p = nullptr;
    }
    GRL_HIP(h, hipMalloc((void **)p, n * sizeof(T)));
    h->allocs.push_back(*p);
    return GRL_OK;
}

// api.hip: accounts the step just enqueued on the handle's stream (no-op until grl_episodes_enable)
int episodes_launch_account(grl_handle *h, int env_base = 0, int count = -1);
// swarm.hip
int swarm_alloc(grl_handle *h);
int swarm_launch_step(grl_handle *h, const float *actions_dev, const double *actions64_dev = nullptr, int no_wind = 0);
int swarm_launch_step_range(grl_handle *h, const float *actions_dev, int env_base, int count, int slot, bool counter_zeroed = false);
int swarm_launch_reset(grl_handle *h, const int32_t *list_dev, const int32_t *count_dev, int max_count);
int swarm_launch_observe(grl_handle *h);
int swarm_reset_injected(grl_handle *h, const double *x0, const double *xa0, const double *ra,
                         const double *an, const double *pn);
int swarm_materialize(grl_handle *h, int first, int count, float *out_dev);
// flat_envs.hip
int solow_alloc(grl_handle *h);
// term_obs_dev (E,2) or null: the processed observation of every env whose episode this step ended (other rows untouched)
int solow_launch_step(grl_handle *h, const float *actions_dev, float *term_obs_dev = nullptr);
int solow_launch_reset(grl_handle *h, const int32_t *list_dev, const int32_t *count_dev, int max_count, bool advance_episode);
int solow_launch_observe(grl_handle *h);
int trade_alloc(grl_handle *h);
int trade_launch_step(grl_handle *h, const float *actions_dev);
int trade_launch_reset(grl_handle *h, const int32_t *list_dev, const int32_t *count_dev, int max_count);
int trade_launch_observe(grl_handle *h);
// ticker.hip
int ticker_alloc(grl_handle *h);
int ticker_set_table(grl_handle *h, const double *rows_host, int nrows);
int ticker_launch_step(grl_handle *h, const float *actions_dev);
int ticker_launch_reset(grl_handle *h, const int32_t *list_dev, const int32_t *count_dev, int max_count);
int ticker_launch_observe(grl_handle *h);
// rollout_math.hip
int launch_returns(grl_handle *h, const float *r, const float *v, const float *mask, const float *boot, int T, int B,
                   float gamma, float lam, float scale, float clip_lo, float clip_hi, float *y, float *adv);
int launch_transform(grl_handle *h, int kind, float *actions_dev, int rows, int cols);
int launch_randn(grl_handle *h, float *dst, size_t n, uint32_t stream, uint64_t counter);
int launch_iota(grl_handle *h, int32_t *dst, int n);
}  // namespace grl
