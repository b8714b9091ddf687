// The host scaffold the whole-episode launches share (solow_sweep.hip, trade_sweep.hip, trade_foresight.hip, ticker_sweep.hip,
// ticker_foresight.hip, solow_dp.hip, swarm_replay.hip, swarm_rules.hip, swarm_plan.hip, swarm_search.hip, swarm_cemplan.hip, ticker_search.hip, trade_search.hip): one copy of what their entry points do alike -- the opening checks, the
// argument checks with the entry point's name in the message, growing a capacity group of buffers, the profiled launch and the
// table-driven grl_*_read.  The kernels, their parameter structs and what a launch uploads and clears stay in the .hip files; the
// device half of the per-pair statistics six of them keep (RewardStats, PairStats) is the sibling header episode_dev.h; the checks
// only the three cross-entropy searches make (counts, per-parameter vectors, normals, output sizes) stand with their statements in
// search_dev.h.
// Included behind common.h; static: every including translation unit has its own copy.  Functions take the C function's name:
// every message starts with it.
#pragma once

#include <initializer_list>
#include <string>

namespace grl {

// ---------------------------------------------------------------------------------------------- checks
// Each returns GRL_OK or the code fail() kept a message for; an entry point chains them with || in the order its messages have.

// a handle of the right kind and no null pointer among the arguments (args_present: their conjunction)
static int episode_open(grl_handle *h, const char *fn, int kind, const char *kind_word, bool args_present) {
    if (!h) return GRL_E_INVALID;
    if (h->cfg.env_kind != kind) return fail(h, GRL_E_INVALID, std::string(fn) + ": not a " + kind_word + " handle");
    if (!args_present) return fail(h, GRL_E_INVALID, std::string(fn) + ": null argument");
    return GRL_OK;
}

static int episode_check_count(grl_handle *h, const char *fn, const char *noun, int n, int most) {
    if (n < 1 || n > most) return fail(h, GRL_E_INVALID, std::string(fn) + ": " + noun + " must be in 1.." + std::to_string(most));
    return GRL_OK;
}

static int episode_check_steps(grl_handle *h, const char *fn, int max_steps) {
    if (max_steps < 1) return fail(h, GRL_E_INVALID, std::string(fn) + ": max_steps must be at least 1");
    return GRL_OK;
}

static int episode_check_trace_env(grl_handle *h, const char *fn, int trace_env) {
    if (trace_env < -1 || trace_env >= h->E) return fail(h, GRL_E_INVALID, std::string(fn) + ": trace_env must be -1 or an env index");
    return GRL_OK;
}

static int episode_check_idle(grl_handle *h, const char *fn) {
    if (h->step_in_flight) return fail(h, GRL_E_INVALID, std::string(fn) + ": a step is in flight (grl_wait first)");
    return GRL_OK;
}

// ---------------------------------------------------------------------------------------------- buffers
// one buffer of a capacity group: `bytes` per unit of the group's capacity
struct EpisodeBuf { void **p; size_t bytes; };
template <typename T>
static EpisodeBuf buf(T *&p, size_t per = 1) { return EpisodeBuf{(void **)&p, per * sizeof(T)}; }

// Grows the buffers of one capacity group to `need` units when that is more than `cap`.  The stream is drained first (a kernel
// in flight may still use what is freed; a later group's drain finds the stream empty), and only if the group grows.  cap is 0
// from before the first grow until after the last, so a failed hipMalloc leaves no stale capacity behind.  stats: null, or the six
// statistics buffers of the pairs, which belong to this group too.
static int episode_reserve(grl_handle *h, size_t &cap, size_t need, std::initializer_list<EpisodeBuf> bufs, PairStats *stats = nullptr) {
    if (need <= cap) return GRL_OK;
    GRL_HIP(h, hipStreamSynchronize(h->stream));
    cap = 0;
    int rc;
    for (const EpisodeBuf &b : bufs)
        if ((rc = grow(h, (uint8_t **)b.p, need * b.bytes))) return rc;
    if (stats) {
        const EpisodeBuf six[] = {buf(stats->total), buf(stats->sum_sq), buf(stats->mn), buf(stats->mx), buf(stats->length), buf(stats->finished)};
        for (const EpisodeBuf &b : six)
            if ((rc = grow(h, (uint8_t **)b.p, need * b.bytes))) return rc;
    }
    cap = need;
    return GRL_OK;
}

// ---------------------------------------------------------------------------------------------- launch
// launch() enqueues the kernel(s) on h->stream; bracketed for grl_profile_*, and a refused launch is the call's error
template <typename F>
static int episode_launch(grl_handle *h, F &&launch) {
    prof_begin(h);
    launch();
    prof_end(h);
    GRL_HIP(h, hipGetLastError());
    return GRL_OK;
}

// ---------------------------------------------------------------------------------------------- read
// one output of a grl_*_read: its name, where it is, its size, and null or why the last call did not produce it (GRL_E_STATE)
struct EpisodeOut { const char *name; const void *src; size_t bytes; const char *absent; };

// The whole of a grl_*_read behind its table.  called: the launch has run (else GRL_E_STATE "call `first` first"); err_dev: null
// or the launch's own device counter of envs that ran off the Solow shock tape, checked after the drain.  stats: null, or the
// statistics of the last call's `pairs` pairs, read as "total", "sum_sq", "min", "max", "length" and "finished".
template <size_t N>
static int episode_read(grl_handle *h, const char *fn, int kind, const char *kind_word, bool called, const char *first,
                        const EpisodeOut (&outs)[N], const int32_t *err_dev, const char *which, void *host, size_t bytes,
                        const PairStats *stats = nullptr, size_t pairs = 0) {
    int rc = episode_open(h, fn, kind, kind_word, which && host);
    if (rc) return rc;
    const std::string f(fn);
    if (!called) return fail(h, GRL_E_STATE, f + ": call " + first + " first");
    hipSetDevice(h->cfg.device_id);
    const std::string s(which);
    const EpisodeOut *o = nullptr;
    for (const EpisodeOut &e : outs)
        if (s == e.name) o = &e;
    EpisodeOut stat{};                                         // a copy: the six rows end with their block
    if (stats) {
        const EpisodeOut six[] = {{"total", stats->total, pairs * 8}, {"sum_sq", stats->sum_sq, pairs * 8}, {"min", stats->mn, pairs * 4},
                                  {"max", stats->mx, pairs * 4}, {"length", stats->length, pairs * 4}, {"finished", stats->finished, pairs}};
        for (const EpisodeOut &e : six)
            if (s == e.name) { stat = e; o = &stat; }
    }
    if (!o) return fail(h, GRL_E_INVALID, f + ": unknown output '" + s + "'");
    if (o->absent) return fail(h, GRL_E_STATE, f + ": " + o->absent);
    if (o->bytes != bytes) return fail(h, GRL_E_SIZE, f + ": '" + s + "' needs " + std::to_string(o->bytes) + " bytes, got " + std::to_string(bytes));
    GRL_HIP(h, hipStreamSynchronize(h->stream));
    if (err_dev) {
        int32_t flag = 0;
        GRL_HIP(h, hipMemcpy(&flag, err_dev, 4, hipMemcpyDeviceToHost));
        if (flag) return fail(h, GRL_E_STATE, std::to_string(flag) + " env(s) popped from an empty shock tape (no TimeLimit and more than T steps)");
    }
    GRL_HIP(h, hipMemcpy(host, o->src, bytes, hipMemcpyDeviceToHost));
    return GRL_OK;
}

}  // namespace grl
