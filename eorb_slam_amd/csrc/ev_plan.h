// ev_plan.h -- which form an event-accumulation call takes: the call's derived geometry (AccumShape), the knobs that can steer it
// (AccumKnobs, filled by accum_knobs() in ev_accum.hip) and the rules, each a named function with one home.  Host-only: no HIP
// header, no eorb_ctx, so that a plain C++ compiler can build a caller of the rules (tests/host/accum_plan_check.cpp).
//
// The dispatcher (ev_accum.hip: ev_accumulate_dev, ev_accumulate_tables) asks the rules in this order:
//   plan_bulk_eligible -> plan_bulk_fits -> plan_dict_usable -> (plan_slot_shaped, plan_tables_ahead while tabulating)
//   -> plan_direct -> plan_slot_eligible -> plan_slot_shape -> (widen short records) -> plan_direct again -> plan_pipeline_chunk,
//   plan_scatter2, plan_sparse_gather, plan_gather.
// The slot form (ev_slots.hip) then asks plan_slot_binning once per call and plan_slot_gather once per part of the batch.
// plan_first_route() is the same sequence without a device: the form a call takes when nothing declines at run time.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

namespace eorb {

constexpr int kTile = 8;            // accumulation tile edge (one wavefront = 8x8 pixels)
constexpr int kChunk = 4096;        // events per binning chunk of the first scatter form (one wavefront bins one chunk)
constexpr int kScatWaves = 8;       // wavefronts of ev_scatter2_kernel
constexpr int kSlotScatWaves = 8;   // wavefronts of sl_scatter_kernel and of the 2 048-event rank scatter
constexpr int kSlotCountWaves = 16; // wavefronts of sl_count_lds_kernel: one chunk each, one row of 16-bit tile counters each in LDS
constexpr int kHotCap = 8192;       // lists per length bucket of sl_hot_kernel's work list
constexpr int kHotRows = 240;       // rows sl_hot_kernel holds in registers: tile positions with more slots never go to it
constexpr int kDdLog = 20;          // float events in bulk: the per-call position table has 2^20 rows; at most half may fill
constexpr int kDirectSlices = 8;    // slices one launch of the binning-free form takes (the dispatcher sends it at most 4)
constexpr int64_t kDirectMaxEvents = 16384;      // a call of up to this many events takes the binning-free form by its shape

// ---- the shape: everything derived from (W, H, sigma, mode_count, B, nev), made once per call ----------------------------------
struct AccumShape {
    int h;                  // half window of the stamp, lenHalfWin (0 for count images)
    int R, dup;             // tiles an event spans per axis at most; list entries an event yields at most (R * R)
    int TX, TY, NT, NTp;    // the tile grid; NT rounded up to even (16-bit counter rows are cleared as 32-bit words)
    int nbits;              // bits of a tile number
    int64_t nev, per_slice; // events of the call; per slice on average (what the chunk sizes go by)
};
inline AccumShape accum_shape(int W, int H, float sigma, int mode_count, int B, int64_t nev)
{
    AccumShape S;
    S.h = mode_count ? 0 : (int)ceil((double)sigma * 3.0);              // lenHalfWin :222
    S.R = (2 * S.h <= kTile) ? ((S.h == 0) ? 1 : 2) : 3;
    S.dup = S.R * S.R;
    S.TX = (W + kTile - 1) / kTile; S.TY = (H + kTile - 1) / kTile; S.NT = S.TX * S.TY; S.NTp = (S.NT + 1) & ~1;
    S.nbits = 1; while ((1 << S.nbits) < S.NT) S.nbits++;
    S.nev = nev; S.per_slice = B > 0 ? nev / B : 0;
    return S;
}

// what the caller asks for.  raw: 0 float events, 1 16-byte sensor records, 2 row numbers of the per-call position table (the float
// bulk path's own records), 3 eorb_raw_event4, 4 eorb_raw_event2
struct AccumRequest { int raw, pol, mode_count, B; };

// ---- the knobs (see the table at accum_knobs, ev_accum.hip, for where each comes from) -------------------------------------------
struct AccumKnobs {
    int gather_form = 0;                     // 0 by the rules below, 1 list pipeline / dense gather, 2 sparse gather, 3 binning-free, 4 slot lists
    int64_t dd_min = (int64_t)1 << 20;       // float events from which a call's positions are tabulated (<= 0: never)
    int pd = 1;                              // 0: no position dictionary
    int scatter = 2;                         // 1: the list pipeline's first scatter form only
    int gather_threads = 512, gather_nc = 0; // ev_gather_kernel's workgroup; tile columns per value wave of ev_gather_raw_kernel (0: by size)
    int slot_chunk = 0, slot_waves = 0, slot_rounds = 0;
    bool slot_rank = true;                   // the rank scatter may run (if the device check passed too)
    long long slot_hot_min = -1;             // -1: by the batch's size
    int slot_hot_cap = 0, slot_hot_waves = 0, slot_prerank = 1, slot_halves = -1;
};

// ---- the route a call took (eorb_debug_counter "accum_route"; 0: no call yet) ----------------------------------------------------
enum { kFormDirect = 1, kFormSlots = 2, kFormLists = 3, kRouteFormMask = 3 };
enum { kSetNone = 0 << 2, kSetMaps = 1 << 2, kSetPerCall = 2 << 2, kSetDict = 3 << 2 };
enum { kRouteSparse = 1 << 4, kRouteWidened = 1 << 5 };

// ---- the rules -------------------------------------------------------------------------------------------------------------------
// Float events in bulk: their distinct positions are tabulated and the call goes on with row numbers as records (raw 2).
// gather_form 1 asks for the list pipeline on the events as they are; every other forced form is still tabulated first -- so float
// events with gather_form 3 and dd_min lowered do NOT take the binning-free form.  (Why 3 is not excluded like 1: unknown.)
inline bool plan_bulk_eligible(const AccumShape& S, const AccumRequest& Q, const AccumKnobs& K)
{
    return !Q.raw && !Q.mode_count && K.gather_form != 1 && S.nev >= K.dd_min && K.dd_min > 0;
}

// events per chunk of the list pipeline (a chunk is binned by one workgroup; short slices take short chunks so that a single
// 2 000-event slice is eight waves side by side, not one serial loop)
inline int plan_pipeline_chunk(const AccumShape& S, const AccumKnobs& K)
{
    return S.per_slice >= (int64_t)1 << 17 ? (K.scatter == 1 ? kChunk : 2048) : (S.per_slice >= (int64_t)1 << 14 ? 1024 : 256);
}

// dynamic LDS of ev_scatter2_kernel for chunks of `chunk` events: records, tile numbers, entry indices, per-wave counts, offsets, bases
inline size_t plan_scatter2_lds(const AccumShape& S, int chunk)
{
    return ((size_t)chunk * 8 + (size_t)chunk * 2 + (size_t)chunk * S.dup * 2 + (size_t)kScatWaves * S.NTp * 2 + (size_t)(S.NTp + 2) * 2 + (size_t)S.NT * 4 + 15) & ~(size_t)15;
}

// The pipeline's second scatter form (the only one that reads row-number records).  wide: float events with polarity carry 16-byte
// entries, which only the first form writes.
inline bool plan_scatter2(const AccumShape& S, const AccumRequest& Q, const AccumKnobs& K)
{
    return K.scatter != 1 && !(Q.pol && !Q.raw) && plan_scatter2_lds(S, plan_pipeline_chunk(S, K)) <= 64 * 1024 && S.TX < 256 && S.TY < 256;
}

// May the bulk path hand row-number records on?  = plan_scatter2 for those records (raw 2, so the polarity clause is moot), asked
// before anything is tabulated.
inline bool plan_bulk_fits(const AccumShape& S, const AccumKnobs& K)
{
    return plan_scatter2(S, AccumRequest{2, 0, 0, 1}, K);
}

// Could the slot form serve these float events (by request, not by load)?  Governs freezing the positions into the dictionary and
// keeping the position table across calls.  gather_form 2 is NOT slot-shaped although plan_slot_eligible admits it for row-number
// records: a forced sparse call tabulates, may still run the slot form, but never freezes.  (On purpose or not: unknown.)
inline bool plan_slot_shaped(const AccumShape& S, const AccumRequest& Q, const AccumKnobs& K)
{
    return !Q.pol && !Q.mode_count && (K.gather_form == 0 || K.gather_form == 4) && S.h >= 1 && S.h <= 4;
}

// The per-call set's integer positions and slot assignment are launched ahead of the tabulation's wait (one wait per call).  Wider
// than plan_slot_shaped by gather_form 2, matching plan_slot_eligible for row-number records.
inline bool plan_tables_ahead(const AccumShape& S, const AccumRequest& Q, const AccumKnobs& K)
{
    return !Q.pol && !Q.mode_count && (K.gather_form == 0 || K.gather_form == 2 || K.gather_form == 4) && S.h >= 1 && S.h <= 4;
}

// the frozen dictionary's key, as the context holds it
struct DictState { int valid, W, H, cooldown; float sigma; };
// a bulk call is served by the dictionary of an earlier call (no sparse test: one pass over the events beats the list pipeline's two)
inline bool plan_dict_usable(const AccumShape& S, const AccumRequest& Q, const AccumKnobs& K, const DictState& D, int W, int H, float sigma)
{
    return plan_bulk_fits(S, K) && plan_slot_shaped(S, Q, K) && D.valid && D.W == W && D.H == H && D.sigma == sigma && D.cooldown == 0 && K.pd != 0;
}

// The binning-free form: one or a few small slices of float or 16-byte sensor events with a Gaussian stamp.  Short records are
// widened first (the dispatcher asks again with raw 1).
inline bool plan_direct(const AccumShape& S, const AccumRequest& Q, const AccumKnobs& K)
{
    return !(Q.raw >= 2 && Q.raw <= 4) && !Q.mode_count && Q.B <= 4 && (K.gather_form == 3 || (K.gather_form == 0 && S.nev <= kDirectMaxEvents));
}

// A host-buffer entry point leaves a slice's events in pinned host memory when the binning-free form, which reads every event once,
// is what plan_direct gives by the call's shape (a forced form is a test's business: those upload).  Float events that
// plan_bulk_eligible sends to the tabulation first (dd_min lowered to the slice's size) stay in host memory as well, although the
// tabulation and the forms behind it read them several times: kept as it was, slower but correct.
inline bool plan_host_events(const AccumShape& S, const AccumRequest& Q, const AccumKnobs& K)
{
    return S.nev > 0 && K.gather_form == 0 && plan_direct(S, Q, K);
}

// fewer than one 64-entry batch per tile on average
inline bool plan_sparse_load(const AccumShape& S, int B) { return S.nev * S.dup < (int64_t)B * S.NT * 64; }

// The slot form: sensor or row-number records, Gaussian stamp, no polarity; by load, or forced (4).  gather_form 2 on row-number
// records still passes the first clause and then the load test -- the "forced sparse" of a float bulk call is decided by its load.
// gather_form 4 on a count or polarity image is not eligible and runs the list pipeline.
inline bool plan_slot_eligible(const AccumShape& S, const AccumRequest& Q, const AccumKnobs& K)
{
    return Q.raw && !Q.mode_count && !Q.pol && (K.gather_form == 0 || K.gather_form == 4 || (Q.raw == 2 && K.gather_form == 2)) &&
           (K.gather_form == 4 || !plan_sparse_load(S, Q.B));
}

// the list pipeline's sparse gather (a wave per tile): forced, or by load; gather_form 4 that fell through gathers densely
inline bool plan_sparse_gather(const AccumShape& S, const AccumRequest& Q, const AccumKnobs& K)
{
    return Q.raw && !Q.mode_count && (K.gather_form == 2 || (K.gather_form == 0 && plan_sparse_load(S, Q.B)));
}

// the list pipeline's gather kernel
enum { kGatherSparse, kGatherRawRows, kGatherGeneric };
struct GatherPlan { int kind, NC, threads, per_wave; };
inline GatherPlan plan_gather(const AccumShape& S, const AccumRequest& Q, const AccumKnobs& K)
{
    const int nb = Q.B * S.NT;
    // sparse, large launches: 16 consecutive work items per wave (a wave per item leaves the launch bound by workgroup dispatch)
    if (plan_sparse_gather(S, Q, K)) return GatherPlan{kGatherSparse, 0, 0, nb >= 65536 ? 16 : 1};
    if (Q.raw && !Q.mode_count) {
        // the add wave + four value waves with two tile columns each (shortest chain per batch), or -- when the launch has enough
        // tiles to keep every SIMD busy anyway -- two value waves with four columns each (fewest instructions per batch)
        const int NC = K.gather_nc == 2 || K.gather_nc == 4 ? K.gather_nc : (nb >= 32768 ? 4 : 2);
        return GatherPlan{kGatherRawRows, NC, 64 * (1 + 8 / NC), 0};
    }
    return GatherPlan{kGatherGeneric, 0, K.gather_threads, 0};
}

// ---- the slot form's own shape test ----------------------------------------------------------------------------------------------
struct SlotScatterChoice { int chunk, waves; bool rank; size_t lds; };
// the scatters' whole LDS.  Pre-ranked: the chunk's gbase row (NT words) | tile of every sorted slot | its loff row (NT + 1 halves, padded
// to NTp + 2 >= plan_slot_loff_pitch) | the sorted entry bytes -- two row copies, no scan scratch.  The rank and ballot forms add their
// per-wave count rows (and a few words of static scan scratch that these sums leave out).
inline size_t plan_slot_lds_rank(int NT, int chunk, int waves) { const int NTp = (NT + 1) & ~1; return ((size_t)NT * 4 + (size_t)chunk * 4 * 2 + (size_t)waves * NTp * 2 + (size_t)(NTp + 2) * 2 + (size_t)chunk * 4 + 15) & ~(size_t)15; }
inline size_t plan_slot_lds_pre(int NT, int chunk) { const int NTp = (NT + 1) & ~1; return ((size_t)NT * 4 + (size_t)chunk * 4 * 2 + (size_t)(NTp + 2) * 2 + (size_t)chunk * 4 + 15) & ~(size_t)15; }
inline size_t plan_slot_lds_ballot(int NT, int chunk) { const int NTp = (NT + 1) & ~1; return ((size_t)chunk * 4 + (size_t)chunk * 2 + (size_t)chunk * 4 * 2 + (size_t)kSlotScatWaves * NTp * 2 + (size_t)(NTp + 2) * 2 + (size_t)NT * 4 + 15) & ~(size_t)15; }

// ---- the rows the slot form's count pass and scan leave for its scatters (BinLayout, ev_common.h) -----------------------------------
// loff[chunk][0 .. NT]: the exclusive prefix of the chunk's entries over the tiles, loff[NT] = all of them, as 16-bit words: a chunk
// has at most kSlotChunkMax events of at most 4 entries each.  gbase[chunk][0 .. NT): where tile t's run of the chunk starts in the
// slice's lists, minus loff[t] (mod 2^32).
constexpr int kSlotChunkMax = 4096;
static_assert(4 * kSlotChunkMax <= 0xffff, "a chunk's entry count, loff[NT], is a 16-bit word");
inline int plan_slot_loff_pitch(int NT) { return (NT + 2) & ~1; }      // 16-bit words per row: NT + 1 rounded up to even (rows are copied as dwords)
inline int plan_slot_gbase_pitch(int NT) { return (NT + 3) & ~3; }     // 32-bit words per row: sl_scan_kernel stores 16 bytes at a time
// the one allocation rule of the two: loff u16 [nchunks][lp] (padded to 16 bytes) | gbase u32 [nchunks][gp]
struct SlotRows { int lp, gp; size_t loff_bytes, bytes; };
inline SlotRows plan_slot_rows(int nchunks, int NT)
{
    SlotRows r;
    const size_t n = (size_t)std::max(nchunks, 1);
    r.lp = plan_slot_loff_pitch(NT); r.gp = plan_slot_gbase_pitch(NT);
    r.loff_bytes = (sizeof(uint16_t) * n * r.lp + 15) & ~(size_t)15;
    r.bytes = r.loff_bytes + sizeof(uint32_t) * n * r.gp;
    return r;
}
// sl_scan_kernel: a thread takes kSlotScanTiles consecutive tiles; the wavefronts that cover the tile grid once are one SEGMENT of the
// slice's chunks, and the workgroup's 16 wavefronts make as many segments as fit (690 tiles: 87 threads = 2 wavefronts, 8 segments)
constexpr int kSlotScanTiles = 8;
inline int plan_slot_scan_waves(int NT) { return std::min(16, ((NT + kSlotScanTiles - 1) / kSlotScanTiles + 63) / 64); }
inline int plan_slot_scan_segments(int NT) { return 16 / plan_slot_scan_waves(NT); }

// The scatter a batch will run -- decided before anything is launched: the preferred chunk size first, then shorter chunks; for each
// the rank form (its own LDS footprint, <= 160 KB with the opt-in) where the device check allows it, else the ballot form (64 KB).
// false: no form fits (e.g. VGA-class sensors without the rank scatter: 4 800 tiles x 8 per-wave counter rows alone are 77 KB).
inline bool plan_slot_scatter(const AccumShape& S, const AccumKnobs& K, bool rank_ok, SlotScatterChoice* out)
{
    // chunks of 4 096 events (16 wavefronts per scatter workgroup) where the rank scatter runs and the slices are long: per-chunk work
    // (the tiles' list bases, the prefix over the waves, the count rows) is shared by twice the events
    // (128 x 1 Mev: binning 1.46-1.51 ms with 2 048, 1.41-1.44 with 4 096)
    const int pref = K.slot_chunk ? K.slot_chunk : (S.per_slice >= (int64_t)1 << 18 ? 4096 : (S.per_slice >= (int64_t)1 << 17 ? 2048 : (S.per_slice >= (int64_t)1 << 14 ? 1024 : 256)));
    const bool rank_allowed = rank_ok && K.slot_rank;
    static const int sizes[4] = {kSlotChunkMax, 2048, 1024, 256};
    for (int i = 0; i < 4; i++) {
        const int chunk = sizes[i];
        if (chunk > pref) continue;
        if (rank_allowed) {
            const int waves = chunk == 4096 ? 16 : kSlotScatWaves;
            const size_t l = plan_slot_lds_rank(S.NT, chunk, waves);
            // (two or more workgroups per CU: the phases of different chunks overlap; one 130 KB workgroup per CU still beats falling back)
            if (l <= (size_t)(chunk == 4096 ? 79 : 158) * 1024) { *out = SlotScatterChoice{chunk, waves, true, l}; return true; }
        }
        if (chunk <= 2048) {
            const size_t l = plan_slot_lds_ballot(S.NT, chunk);
            if (l <= 64 * 1024) { *out = SlotScatterChoice{chunk, kSlotScatWaves, false, l}; return true; }
        }
    }
    return false;
}

// sl_plan_kernel keeps two words per slice in LDS and ranks a position's lists by an O(B^2) loop, sl_scan_kernel is one workgroup
// per slice: batches of more than 2 048 slices take the list pipeline; so do tile grids whose count rows do not fit the LDS
inline bool plan_slot_shape(const AccumShape& S, int B, const AccumKnobs& K, bool rank_ok, SlotScatterChoice* out)
{
    return !(B > 2048 || (size_t)S.NT * 4 > 64 * 1024 || !plan_slot_scatter(S, K, rank_ok, out));
}

// ---- the slot form's binning: which count pass runs, what it leaves for the scatter, which scatter reads it -----------------------
enum { kCountGlobal, kCountLds, kCountLdsKeyed };      // sl_count_kernel | sl_count_lds_kernel<ST> | sl_count_lds_kernel<16, KEYED>
enum { kRecAsIs, kRecShort2, kRecRanked8 };            // what the scatter reads: the count pass's own input records (with a dictionary: the
                                                       // records it writes), a 2-byte sensor index per event, an 8-byte index + ranks per event
enum { kScatBallot, kScatRank, kScatPre };             // sl_scatter_kernel | sl_scatter_rank_kernel<ST, NW> | sl_scatter_pre_kernel<NW>
struct SlotBinPlan {
    int count, record, scatter;
    int stride, scat_stride;            // record stride the count pass / the rank and ballot scatters read (-4: 4-byte row numbers, else bytes)
    size_t lds_count, lds_scatter;      // dynamic LDS of the two launches
};
// eorb_debug_counter "slot_binning"
inline int slot_binning_code(const SlotBinPlan& p) { return p.count | p.record << 2 | p.scatter << 4; }

// stride_in: 16 / 4 / 2-byte sensor records or -4 (row numbers of the per-call table); nsrc: positions of the set (the sensor's pixels);
// dict: 0 none, 1 the count pass looks float events up in the position dictionary and writes 4-byte rows, 2: 2-byte ids.
// false: a dictionary call whose tile-range table does not fit the LDS -- only the LDS count pass has the lookup.
// The asymmetries, kept as they were:
//  - ranked records are made for 16 / 4 / 2-byte sensor records and for 2-byte dictionary ids, never for 4-byte rows (stride -4 from
//    either source): a ranked record holds a 16-bit position.
//  - 2-byte transcoding is for 16-byte records only: 4- and 2-byte records are short already.  It is tied to sc.rank although the
//    ballot scatter reads stride 2 as well (the ballot form is the fallback of a failed device check, left as plain as possible).
//  - `nsrc <= 65535` is implied by lds_fits where the sensor is the image (8x8 tiles: NT >= nsrc / 64, so lds_c >= 2.5 nsrc and
//    159 KiB hold 65 126 positions at most) and by dict == 2 (fewer than 65 535 ids).  It is kept: a sensor may be larger than the
//    image, and a 16-bit index is what both record formats rest on.
//  - the global count pass never leaves records: VGA-class sensors run count and scatter on the events as they came.
//  - scat_stride is what the rank / ballot scatter reads; the pre-ranked scatter has one record format and ignores it (it keeps `stride`).
inline bool plan_slot_binning(const AccumShape& S, int stride_in, int64_t nsrc, int dict, const SlotScatterChoice& sc, const AccumKnobs& K, SlotBinPlan* out)
{
    const int stride = dict ? (dict == 2 ? 2 : -4) : stride_in;
    // the tile ranges of all positions (16 bits each, copied as dwords) + one row of counters per wavefront in the LDS of one workgroup per CU?
    const size_t lds_c = 4 * (((size_t)nsrc + 2) / 2) + (size_t)kSlotCountWaves * S.NTp * 2;
    const bool lds_fits = S.TX <= 127 && S.TY <= 127 && lds_c <= 159 * 1024;
    const size_t lds_p = plan_slot_lds_pre(S.NT, sc.chunk);
    const bool pre_fits = K.slot_prerank && sc.rank && lds_p <= 158 * 1024;
    const int scat = sc.rank ? kScatRank : kScatBallot;
    SlotBinPlan p{kCountLds, kRecAsIs, scat, stride, stride, lds_c, sc.lds};
    if (dict) {
        if (!lds_fits) return false;
        p.count = kCountLdsKeyed;
        if (pre_fits && dict == 2) { p.record = kRecRanked8; p.scatter = kScatPre; p.lds_scatter = lds_p; }
    }
    else if (!lds_fits) { p.count = kCountGlobal; p.lds_count = sizeof(uint32_t) * (size_t)S.NT; }
    else if (pre_fits && (stride == 16 || stride == 4 || stride == 2) && nsrc <= 65535) { p.record = kRecRanked8; p.scatter = kScatPre; p.lds_scatter = lds_p; }
    else if (stride == 16 && nsrc <= 65535 && sc.rank) { p.record = kRecShort2; p.scat_stride = 2; }
    *out = p;
    return true;
}

// ---- the slot form's gather: workgroup shape, task count, which lists go to the register-row kernel --------------------------------
struct SlotGatherPlan {
    size_t lds; int wg_per_cu, nw, rounds, Gt, max_per_tile;      // sl_gather_kernel: LDS, workgroups per CU, wavefronts, spare rounds, tasks, wavefronts a position gets at most
    uint32_t prio_ref, hot_min, hot_cap; int hot_waves;          // lists this long go first | to sl_hot_kernel (0: that kernel is off) | per bucket; its wavefronts
};
// B, nev: slices and events of the PART (the batch, or a half of it); sl_null: most slots of a tile of these positions; ncu: compute units
inline SlotGatherPlan plan_slot_gather(const AccumShape& S, int B, int64_t nev, int nparts, int sl_null, int ncu, const AccumKnobs& K)
{
    SlotGatherPlan g;
    g.lds = (size_t)(sl_null + 1) * 256;
    g.wg_per_cu = std::max(1, (int)((160 * 1024) / g.lds));
    // four wavefronts per SIMD saturate the vector ALUs and leave every list about full single-wave speed (measured: 8 per SIMD
    // process the same entries per second, each list at half the pace)
    g.nw = std::min(16, std::max(1, 16 / g.wg_per_cu));
    if (K.slot_waves >= 1 && K.slot_waves <= 16) g.nw = K.slot_waves;
    g.nw = std::min(g.nw, std::max(1, B));
    // one task per tile position plus a few rounds of spare ones shared out by weight; a position never gets more wavefronts than slices
    g.rounds = K.slot_rounds >= 1 ? K.slot_rounds : 4;
    g.Gt = S.NT + g.rounds * ncu * g.wg_per_cu;
    g.max_per_tile = (B + g.nw - 1) / g.nw;
    g.prio_ref = (uint32_t)std::min<int64_t>(std::max<int64_t>(4096, nev / 2000), 0x7fffffff);   // lists this long go first at the issue arbiter
    // lists of a few thousand entries or more go to the register-row kernel (when every tile's rows fit its 240 registers): 13
    // cycles per entry instead of 29, which shortens the launch's longest chains AND moves more entries per second; shorter lists
    // would not repay the 240 row loads per list (measured at 128 x 1 Mev: threshold 4 096 ... 8 192 1.40-1.45 ms, 16 384 1.53, none 2.44)
    g.hot_min = sl_null <= kHotRows ? (uint32_t)std::min<int64_t>(std::max<int64_t>(4096, nev * nparts / 16000), 0x7fffffff) : 0u;
    const long long hot_over = K.slot_hot_min;
    // (never below 64: the register-row kernel's tail load reads the 64 bytes that END at the list's end; 0 = that kernel off)
    if (hot_over >= 0) g.hot_min = (sl_null <= kHotRows && hot_over > 0) ? (uint32_t)std::min<long long>(std::max<long long>(hot_over, 64), 0x7fffffff) : 0u;
    g.hot_cap = K.slot_hot_cap > 0 ? (uint32_t)std::min(K.slot_hot_cap, kHotCap) : (uint32_t)kHotCap;
    g.hot_waves = K.slot_hot_waves > 0 ? K.slot_hot_waves : 8 * ncu;     // two per SIMD: all of its registers
    return g;
}

// ---- the whole sequence, without a device: the route of a call that nothing declines at run time ----------------------------------
// (the dictionary holds every position, the position table does not crowd; slots_usable: the positions' slot tables are, sl_ok)
inline int plan_first_route(const AccumShape& S, AccumRequest Q, const AccumKnobs& K, const DictState& D, int W, int H, float sigma, bool rank_ok,
                            bool slots_usable = true)
{
    SlotScatterChoice sc;
    int set = Q.raw ? kSetMaps : kSetNone, wide = 0;
    if (plan_bulk_eligible(S, Q, K) && plan_bulk_fits(S, K)) {
        if (plan_dict_usable(S, Q, K, D, W, H, sigma) && plan_slot_shape(S, Q.B, K, rank_ok, &sc)) return kFormSlots | kSetDict;
        Q.raw = 2; set = kSetPerCall;
    }
    else if (plan_direct(S, Q, K)) return kFormDirect | set;
    if (plan_slot_eligible(S, Q, K) && slots_usable && plan_slot_shape(S, Q.B, K, rank_ok, &sc)) return kFormSlots | set;
    if (Q.raw == 3 || Q.raw == 4) {
        Q.raw = 1; wide = kRouteWidened;
        if (plan_direct(S, Q, K)) return kFormDirect | set | wide;
    }
    return kFormLists | set | (plan_sparse_gather(S, Q, K) ? kRouteSparse : 0) | wide;
}

}  // namespace eorb
