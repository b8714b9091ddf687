// The conv net's environment switches: what grl_net_create reads once, before the net exists, and nothing reads again.  One row per
// switch -- name, dialect, field, default, bounds or keyword, meaning -- and one reader.  DESIGN.md (section 8, "Conv net switches") has the same
// rows with who sets each.  Plain C++ (no HIP): tests/test_conv_switches.py holds the reader to the parsing it replaced.
// The dialects differ (some switches hear "0", most do not; some integers are clamped, some ignored, some taken as they come).
// Tests, bench.py and the tools pass these strings, so the differences stay; the kind column is where they are written down.
// Read elsewhere, not here: GRL_NET_EVICT (a per-process static of maybe_evict, net_conv.hip: a measurement aid, not a property of
// a net) and GRL_NET_CHUNK (goldsrl/rollout.py: it becomes grl_net_config::max_chunk_samples before the C library is called).
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

namespace grl {
struct ConvSwitches {      // ConvSwitches{} is what an empty environment reads as (the rows' defaults: tests/test_conv_switches.py holds the two equal)
    int gemm_f32 = 0, range_fallback_on = 1, range_return_k = 4, loss_scale_on = 1, acc1 = 1;
    int trunk_skip = 1, patch_skip = 1, obs_index = 1, expand2_gemm = 1, expand3_gather = 1;
    int pslice_rows = 1024, pwgrad_xcd = 1, pdgrad_xcd = 1, pwgrad_pair = 1, pdgrad_pair = 1, swgrad_pair = 1, swgrad_chunks = 0, slots_xcd = 1;
    int tn_wgs = 1024, tn_wgs_dense = 512, keep_max_level = 3;
    int lanes_asked = 0, idx_side_asked = 1;      // what grl_net_create combines with the two per-create flags: not the outcome
    bool keep_free_capped = false;                // GRL_NET_KEEP_FREE_MB was set ...
    size_t keep_free_cap = 0;                     // ... to this many bytes
};
enum ConvSwitchKind {
    SW_KEYWORD,         // the keyword gives `hi`; unset and every other string give the default ("off" only: "0" is another string)
    SW_OFF_OR_0,        // "off" or "0" give 0; every other string gives 1
    SW_OFF_OR_COUNT,    // "off" gives 0; every other string max(0, atoi)
    SW_INT_ANY,         // atoi, as it comes (text that is no number reads as 0)
    SW_INT_NONZERO,     // atoi != 0
    SW_INT_FLOOR,       // max(lo, atoi)
    SW_INT_RANGE,       // atoi; outside lo..hi ignored (the default stays)
    SW_INT_POW2,        // atoi; ignored unless a power of two in lo..hi
    SW_MB_DIGITS,       // decimal digits only and below 2^44, in MB; anything else REFUSES the creation (not read as 0)
};
struct ConvSwitchRow {
    const char *name;
    ConvSwitchKind kind;
    int ConvSwitches::*field;      // null: SW_MB_DIGITS writes keep_free_capped / keep_free_cap
    int def, lo, hi;
    const char *keyword, *meaning;
};
using CSw = ConvSwitches;
static const ConvSwitchRow kConvSwitches[] = {
    // ---- arithmetic
    {"GRL_NET_GEMM", SW_KEYWORD, &CSw::gemm_f32, 0, 0, 1, "f32", "GEMMs from the start: 0 = three fp16 products (operands inside the fp16 range), 1 = v_mfma_f32_16x16x4_f32 (no range limit, 103 instead of 200 TFLOP/s); a pass that raised the range flag moves the net to 1 by itself"},
    {"GRL_NET_RANGE_FALLBACK", SW_KEYWORD, &CSw::range_fallback_on, 1, 0, 0, "off", "off: a range violation fails the call (GRL_E_RANGE) and nothing else"},
    {"GRL_NET_RANGE_RETURN", SW_OFF_OR_COUNT, &CSw::range_return_k, 4, 0, 0, nullptr, "clean updates in a row that take a net the fallback moved to fp32 back to the three-product form (0 / off: never)"},
    {"GRL_NET_LOSS_SCALE", SW_KEYWORD, &CSw::loss_scale_on, 1, 0, 0, "off", "per-pass power-of-two scale of the head gradients (net_train.inc); off: S = 1, to show what the scale is for (tests, DESIGN section 5)"},
    {"GRL_NET_ACC1", SW_KEYWORD, &CSw::acc1, 1, 0, 0, "off", "gemm_rowk instances built with ACC1 use the one-accumulator form (launch_rowk); off: the two-accumulator form everywhere"},
    // ---- which form of a layer runs
    {"GRL_TRUNK_SKIP", SW_KEYWORD, &CSw::trunk_skip, 1, 0, 0, "off", "conv2's forward / weight gradient / transposed convolution run over the rows the env's bins reach; off: all rows"},
    {"GRL_PATCH_SKIP", SW_KEYWORD, &CSw::patch_skip, 1, 0, 0, "off", "the dense1 patch GEMMs skip what the support masks say is zero; off: the plain 5x5 patch"},
    {"GRL_OBS_INDEX", SW_KEYWORD, &CSw::obs_index, 1, 0, 0, "off", "conv1's backward helpers read the observation's index record; off: the kernels that index inside"},
    {"GRL_NET_EXPAND2", SW_KEYWORD, &CSw::expand2_gemm, 1, 0, 0, "lds", "conv2's per-agent corrections as a class-sorted GEMM; lds: the LDS-resident kernel"},
    {"GRL_NET_EXPAND3", SW_KEYWORD, &CSw::expand3_gather, 1, 0, 0, "prod", "conv3's per-agent corrections as a gather GEMM at the patch pixels; prod: slot products + expansion kernel"},
    // ---- tile shapes and orders of the gradient step (A/B legs of the equality tests, tuning knobs)
    {"GRL_PATCH_SLICE", SW_INT_POW2, &CSw::pslice_rows, 1024, 256, 8192, nullptr, "dense1 patch weight gradient: rows per slice (default: PATCH_SLICE_ROWS, net_patch.inc)"},
    {"GRL_PATCH_WGRAD_XCD", SW_INT_ANY, &CSw::pwgrad_xcd, 1, 0, 0, nullptr, "tile order of that launch: 1 = a row slice per XCD, A and B of a slice fetched once (under the support masks and the lighter traffic of round 3 it wins by 0.7 %); 2, per-pixel tiles only: the plain patch's choice; else spread"},
    {"GRL_PATCH_DGRAD_XCD", SW_INT_NONZERO, &CSw::pdgrad_xcd, 1, 0, 0, nullptr, "dense1 patch data gradient: an M tile per XCD (A fetched once): 40.6 -> 38.5 ms per update at 81 920-sample chunks; spread (0) was faster at 40 960"},
    {"GRL_PATCH_WGRAD_PAIR", SW_OFF_OR_0, &CSw::pwgrad_pair, 1, 0, 0, nullptr, "128 x 128 tiles over pairs of live patch pixels (PatchRowsPair, net_gemm.h); off: the 64 x 128 per-pixel tiles of round 3"},
    {"GRL_PATCH_DGRAD_PAIR", SW_OFF_OR_0, &CSw::pdgrad_pair, 1, 0, 0, nullptr, "the same for the data gradient's N axis (PatchRowsPairN): 128 x 128 tiles on eight waves; off: 256 x 64 per pixel"},
    {"GRL_SLOT_WGRAD_PAIR", SW_OFF_OR_0, &CSw::swgrad_pair, 1, 0, 0, nullptr, "conv3's slot weight gradient on 128 x 64 tiles of two live taps (SlotGatherT3PPair); off: 64 x 64 per tap"},
    {"GRL_SLOT_WGRAD_CHUNKS", SW_INT_FLOOR, &CSw::swgrad_chunks, 0, 0, 0, nullptr, "row ranges of that launch (0: the default of the call site)"},
    {"GRL_SLOTS_XCD", SW_OFF_OR_0, &CSw::slots_xcd, 1, 0, 0, nullptr, "the sorted gather GEMMs keep a contiguous range of row tiles on one XCD (gemm_rowk, XCD_ORDER = 2); off: round-robin tiles"},
    {"GRL_TN_WGS", SW_INT_RANGE, &CSw::tn_wgs, 1024, 256, 4096, nullptr, "workgroups a split-M weight-gradient launch aims at (slab count = tn_wgs / tiles, net_slab_plan.h)"},
    {"GRL_TN_WGS_DENSE", SW_INT_RANGE, &CSw::tn_wgs_dense, 512, 128, 4096, nullptr, "the same for the dense layers' weight gradients"},
    // ---- streams
    {"GRL_NET_LANES", SW_INT_RANGE, &CSw::lanes_asked, 0, 1, 8, nullptr, "lanes (streams with a chunk workspace each); 0 = unset or outside 1..8: 4, or 1 under GRL_NET_F_SINGLE_STREAM (measured at 32 768 envs: 1.41 / 1.22 / 1.16 / 1.13 / 1.14 s per update with 1 / 2 / 3 / 4 / 8)"},
    {"GRL_NET_IDX_SIDE", SW_OFF_OR_0, &CSw::idx_side_asked, 1, 0, 0, nullptr, "a one-chunk-per-step rollout runs the forward's index kernels on lane 0's side stream (never under GRL_NET_F_SINGLE_STREAM)"},
    // ---- rollout-resident activations (ensure_rollout_bufs, net_train.inc)
    {"GRL_NET_KEEP_LEVEL", SW_INT_ANY, &CSw::keep_max_level, 3, 0, 0, nullptr, "the highest keep level tried (A/B: 2 = re-index in the gradient step)"},
    {"GRL_NET_KEEP_FREE_MB", SW_MB_DIGITS, nullptr, 0, 0, 0, nullptr, "caps the free memory the level choice sees (a comparison only: nothing is allocated for it), so that the descent 3 -> 2 -> 1 -> 0 can be walked at any size"},
};

// lookup: getenv, or a test's table.  0 and *out filled, or nonzero and *err = what was refused (GRL_NET_KEEP_FREE_MB only).
inline int conv_switches_read(const char *(*lookup)(const char *), ConvSwitches *out, const char **err) {
    *out = ConvSwitches{};
    for (const ConvSwitchRow &r : kConvSwitches) {
        const char *e = lookup(r.name);
        if (r.kind == SW_MB_DIGITS) {
            char *end = nullptr;
            const unsigned long long mb = e ? strtoull(e, &end, 10) : 0;
            if (e && (*e < '0' || *e > '9' || *end != 0 || mb >= (1ull << 44))) { *err = "GRL_NET_KEEP_FREE_MB must be a number of MB (decimal digits)"; return 1; }
            out->keep_free_capped = e != nullptr;
            out->keep_free_cap = (size_t)mb << 20;
            continue;
        }
        int &f = out->*r.field;
        f = r.def;
        if (!e) continue;
        const int v = atoi(e), off = strcmp(e, "off") == 0;
        switch (r.kind) {
            case SW_KEYWORD: if (strcmp(e, r.keyword) == 0) f = r.hi; break;
            case SW_OFF_OR_0: f = !off && strcmp(e, "0") != 0; break;
            case SW_OFF_OR_COUNT: f = off || v < 0 ? 0 : v; break;
            case SW_INT_ANY: f = v; break;
            case SW_INT_NONZERO: f = v != 0; break;
            case SW_INT_FLOOR: f = v < r.lo ? r.lo : v; break;
            case SW_INT_RANGE: if (v >= r.lo && v <= r.hi) f = v; break;
            case SW_INT_POW2: if (v >= r.lo && v <= r.hi && (v & (v - 1)) == 0) f = v; break;
            case SW_MB_DIGITS: break;
        }
    }
    return 0;
}
}  // namespace grl
