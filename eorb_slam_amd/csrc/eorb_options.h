// eorb_options.h -- every run-time switch of the library: ONE table.  A row is a member of Options (what a context runs with,
// eorb_ctx::opt), its name for eorb_debug_option / eorb_debug_option_get, the environment variable that seeds it when a context is
// created (options_from_env: the only reader of the environment) and its default.  Host-only: no HIP header, no eorb_ctx, so that a
// plain C++ compiler can build a caller (tests/host/options_check.cpp).
//
// Precedence, the same for every row: the environment seeds the member at eorb_create, an option call overwrites it.  Five rows have a
// "not set" range (unset: kNegative < 0, kNotPositive <= 0): an option call with such a value puts the value of eorb_create back.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "ev_plan.h"

namespace eorb {

enum OptionUnset { kNever, kNegative, kNotPositive };

//   X(type, option, environment, default, unset)
#define EORB_OPTIONS(X) \
    /* extractor: shrink the octree's node pools by this many nodes (forces overflows); its global-memory layout; its list algorithm for  */ \
    /* every pass.  All three take effect at the next eorb_orb_configure, as do the three EORB_OCT_* rows below.                          */ \
    X(int, octree_pool_shrink, nullptr, 0, kNever) \
    X(int, octree_force_global, nullptr, 0, kNever) \
    X(int, octree_list_algorithm, nullptr, 0, kNever) \
    /* extraction: orientation, descriptors and output order as three kernels (the path of a lapping area) for every call */ \
    X(int, orb_three_launches, nullptr, 0, kNever) \
    /* window matchers: list capacity per query / pool per pair (to force the full-scan path); entries phase 2 stages in LDS */ \
    X(int, win_list_cap, nullptr, 0, kNever) \
    X(int, win_pool_cap, nullptr, 0, kNever) \
    X(int, win_lds_entries, nullptr, 0, kNever) \
    /* accumulation: 0 by the rules of ev_plan.h, 1 list pipeline / dense gather, 2 sparse gather, 3 binning-free (<= 4 slices), 4 slot lists */ \
    X(int, gather_form, nullptr, 0, kNever) \
    /* slot form: lists per length bucket of the register-row kernel (<= 0: kHotCap), to force the overflow branch */ \
    X(int, slot_hot_cap, nullptr, 0, kNever) \
    /* KeyFrameDatabase: first capacity in slots (and 64 words per slot; <= 0: 1 024); scored entries sorted in LDS (<= 0: as many as fit) */ \
    X(int, kfdb_initial_slots, nullptr, 0, kNever) \
    X(int, kfdb_finish_lds_entries, nullptr, 0, kNever) \
    /* float events in bulk: events from which a call's positions are tabulated (<= 0: never); 0: never freeze / use the position dictionary */ \
    X(long long, dedupe_min_events, nullptr, 1 << 20, kNever) \
    X(int, position_dict, nullptr, 1, kNever) \
    /* -1 off; 0..255: the byte that new allocations, the call arena, its staging slot and the landing buffer are filled with before use */ \
    X(int, dirty_fill, nullptr, -1, kNever) \
    /* slot form: non-zero: the rank scatter may run (if the device check passed too), 0: ballot scatter */ \
    X(int, slot_rank, "EORB_SLOT_RANK", 1, kNegative) \
    /* slot form: list length from which the register-row kernel takes a list (0: that kernel off, < 0: by the batch's size); its wavefronts (<= 0: 8 per CU) */ \
    X(long long, slot_hot_min, "EORB_SLOT_HOT_MIN", -1, kNegative) \
    X(int, slot_hot_waves, "EORB_SLOT_HOT_WAVES", 0, kNotPositive) \
    /* slot form: non-zero: ranks kept by the count pass (sl_scatter_pre_kernel); < 0 by the batch's shape, 0 one part, > 0 two halves whatever the shape */ \
    X(int, slot_prerank, "EORB_SLOT_PRERANK", 1, kNegative) \
    X(int, slot_halves, "EORB_SLOT_HALVES", -1, kNegative) \
    /* list pipeline: 1: its first scatter form only; ev_gather_kernel's workgroup (192..1024 and a multiple of 64, else the build's); */ \
    /* tile columns per value wave of ev_gather_raw_kernel (2 / 4, else by the launch's size)                                          */ \
    X(int, scatter, "EORB_SCATTER", 2, kNever) \
    X(int, gather_threads, "EORB_GATHER_THREADS", 0, kNever) \
    X(int, gather_nc, "EORB_GATHER_NC", 0, kNever) \
    /* slot form: events per chunk (256 / 1024 / 2048 / 4096, else by the slices' length); gather wavefronts (1..16); spare rounds (>= 1, else 4) */ \
    X(int, slot_chunk, "EORB_SLOT_CHUNK", 0, kNever) \
    X(int, slot_waves, "EORB_SLOT_WAVES", 0, kNever) \
    X(int, slot_rounds, "EORB_SLOT_ROUNDS", 0, kNever) \
    /* window matchers: wavefronts of a phase-1 workgroup, queries per phase-1 workgroup (<= 0: by the number of pairs) */ \
    X(int, win_cand_waves, "EORB_WIN_CAND_WAVES", 0, kNever) \
    X(int, win_qpb, "EORB_WIN_QPB", 0, kNever) \
    /* host-buffer calls: bytes up to which a kernel, not the copy engine, moves a call's inputs / results (0: always the copy engine) */ \
    X(long long, upload_kernel_max, "EORB_UPLOAD_KERNEL_MAX", 1 << 20, kNever) \
    X(long long, download_kernel_max, "EORB_DOWNLOAD_KERNEL_MAX", 1 << 20, kNever) \
    /* non-zero: a host-buffer call polls for its results instead of blocking */ \
    X(int, sync_spin, "EORB_SYNC_SPIN", 0, kNever) \
    /* 0: a live slice's events / a call's one image are uploaded, not read in place from pinned host memory */ \
    X(int, slice_zero_copy, "EORB_SLICE_ZERO_COPY", 1, kNever) \
    X(int, image_zero_copy, "EORB_IMAGE_ZERO_COPY", 1, kNever) \
    /* eorb_ev_mc_contest: events up to which one binning-free launch makes every reconstruction of the window */ \
    X(long long, contest_direct_max, "EORB_CONTEST_DIRECT_MAX", 49152, kNever) \
    /* extractor: LDS budget of the octree kernel; 0: no direct passes (as octree_list_algorithm 1); 0: no dynamic placement */ \
    X(int, octree_budget_kb, "EORB_OCT_BUDGET_KB", 156, kNever) \
    X(int, octree_direct, "EORB_OCT_DIRECT", 1, kNever) \
    X(int, octree_dynamic, "EORB_OCT_DYNAMIC", 1, kNever) \
    /* extraction: 0: never the one-launch describe_kernel (as orb_three_launches 1) */ \
    X(int, orb_describe, "EORB_ORB_DESCRIBE", 1, kNever)

struct Options {
#define X(type, name, env, dflt, unset) type name = dflt;
    EORB_OPTIONS(X)
#undef X
};

struct OptionRow {
    const char* name; const char* env;
    long long (*get)(const Options&); void (*put)(Options&, long long);
    long long dflt; OptionUnset unset;
};
template <typename T, T Options::*M> long long option_member_get(const Options& o) { return o.*M; }
template <typename T, T Options::*M> void option_member_put(Options& o, long long v) { o.*M = (T)v; }
constexpr OptionRow kOptions[] = {
#define X(type, name, env, dflt, unset) {#name, env, option_member_get<type, &Options::name>, option_member_put<type, &Options::name>, dflt, unset},
    EORB_OPTIONS(X)
#undef X
};

inline const OptionRow* option_row(const char* name)
{
    for (const OptionRow& r : kOptions) if (!strcmp(r.name, name)) return &r;
    return nullptr;
}

// the defaults, then atoll(value) for every row whose environment variable `lookup` finds
typedef const char* (*EnvLookup)(const char*);
inline Options options_from_env(EnvLookup lookup)
{
    Options o;
    for (const OptionRow& r : kOptions)
        if (const char* e = r.env ? lookup(r.env) : nullptr) r.put(o, atoll(e));
    return o;
}
inline Options options_from_env() { return options_from_env([](const char* name) -> const char* { return getenv(name); }); }

// false: no such row.  created: what eorb_create left (the value a "not set" value puts back)
inline bool option_set(Options& cur, const Options& created, const char* name, long long value)
{
    const OptionRow* r = option_row(name);
    if (!r) return false;
    const bool unset = (r->unset == kNegative && value < 0) || (r->unset == kNotPositive && value <= 0);
    r->put(cur, unset ? r->get(created) : value);
    return true;
}
inline bool option_get(const Options& o, const char* name, long long* value)
{
    const OptionRow* r = option_row(name);
    if (r) *value = r->get(o);
    return r != nullptr;
}

// the rows the accumulation forms' rules read (ev_plan.h); build_gather_threads: ev_gather_kernel's workgroup as compiled
inline AccumKnobs accum_knobs(const Options& o, int build_gather_threads)
{
    AccumKnobs k;
    k.gather_form = o.gather_form; k.dd_min = o.dedupe_min_events; k.pd = o.position_dict;
    k.scatter = o.scatter;
    k.gather_threads = (o.gather_threads >= 192 && o.gather_threads <= 1024 && o.gather_threads % 64 == 0) ? o.gather_threads : build_gather_threads;
    k.gather_nc = o.gather_nc;
    k.slot_chunk = (o.slot_chunk == 256 || o.slot_chunk == 1024 || o.slot_chunk == 2048 || o.slot_chunk == 4096) ? o.slot_chunk : 0;
    k.slot_waves = o.slot_waves; k.slot_rounds = o.slot_rounds;
    k.slot_rank = o.slot_rank != 0;
    k.slot_hot_min = o.slot_hot_min;
    k.slot_hot_cap = o.slot_hot_cap; k.slot_hot_waves = std::max(o.slot_hot_waves, 0);
    k.slot_prerank = o.slot_prerank; k.slot_halves = o.slot_halves;
    return k;
}

}  // namespace eorb
