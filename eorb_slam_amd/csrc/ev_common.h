// ev_common.h -- what the accumulation translation units share (ev_accum.hip, ev_slots.hip): the bin layout of both pipelines and small
// device helpers
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "eorb_ctx.h"

namespace eorb {

// ---- the bins of a batch: its chunk list and the workspaces count -> scan -> scatter share, one layout for the list pipeline and the
// slot form.  chunks buffer: ChunkDesc [nchunks] | the slices' first chunks, int [B + 1] (padded to 8 bytes) | their entry bases,
// int64 [B]; segoff buffer: segcnt u16 [nchunks][NT] (padded to 16 bytes) | segbase u32 [nchunks][NT] (the list pipeline; the slot
// form: loff | gbase, below); tile_order buffer: tile_cnt
// u32 [B * NT] | tile_base u32 [B * NT] (| what the pipeline adds behind them) ----
struct BinLayout {
    int B, nchunks, NT, nb;
    size_t cd, sc, eb, cnt;                      // bytes of the three parts of the chunks buffer; of segcnt
    const ChunkDesc* d_chunks = nullptr; const int* d_slice_c0 = nullptr; const int64_t* d_slice_eb = nullptr;
    uint16_t* d_segcnt = nullptr; uint32_t* d_segbase = nullptr; uint32_t* d_tile_cnt = nullptr; uint32_t* d_tile_base = nullptr;
    BinLayout() : BinLayout(0, 0, 0) {}
    BinLayout(int B_, int nchunks_, int NT_) : B(B_), nchunks(nchunks_), NT(NT_), nb(B_ * NT_)
    {
        cd = sizeof(ChunkDesc) * (size_t)std::max(nchunks, 1);
        sc = (sizeof(int) * (size_t)(B + 1) + 7) & ~(size_t)7;
        eb = sizeof(int64_t) * (size_t)B;
        cnt = (sizeof(uint16_t) * (size_t)std::max(nchunks, 1) * NT + 15) & ~(size_t)15;
        rows = plan_slot_rows(nchunks, NT); lp = rows.lp; gp = rows.gp;
    }
    // the slot form keeps other rows in its segoff buffer (ev_plan.h, plan_slot_rows): loff u16 [nchunks][lp] | gbase u32 [nchunks][gp]
    int lp = 0, gp = 0; SlotRows rows{0, 0, 0, 0};
    uint16_t* d_loff = nullptr; uint32_t* d_gbase = nullptr;
    size_t slot_rows_bytes() const { return rows.bytes; }
    void view_slot_rows(void* segoff) { d_loff = (uint16_t*)segoff; d_gbase = (uint32_t*)((char*)segoff + rows.loff_bytes); }
    size_t chunks_bytes() const { return cd + sc + eb; }
    size_t segoff_bytes() const { return cnt + sizeof(uint32_t) * (size_t)std::max(nchunks, 1) * NT; }
    void view(void* chunks, void* segoff, void* tile_order)      // (after the buffers' ensure())
    {
        d_chunks = (const ChunkDesc*)chunks; d_slice_c0 = (const int*)((char*)chunks + cd); d_slice_eb = (const int64_t*)((char*)chunks + cd + sc);
        d_segcnt = (uint16_t*)segoff; d_segbase = (uint32_t*)((char*)segoff + cnt);
        d_tile_cnt = (uint32_t*)tile_order; d_tile_base = d_tile_cnt + nb;
    }
};

// Where a slice's entries start: base(b + 1) = (base(b) + events(b) * per_event + slack + align - 1) & ~(align - 1), base(0) = 0.
// The list pipeline: dup entries per event, lists back to back {dup, 0, 1}; the slot form: at most 4 two-byte entries per event, each
// of the slice's NT lists rounded up to 16 {4, 16 NT, 16}.
struct EntryBaseRule { int per_event; int64_t slack; int64_t align; };
struct HostBins { std::vector<ChunkDesc> cds; std::vector<int> slice_c0; std::vector<int64_t> slice_eb; int64_t nchunks = 0, entries = 0; };

// the chunk list of B slices cut into chunks of `chunk` events; lists = false: the totals only (nchunks, entries)
static inline HostBins bin_chunks_host(const int64_t* h_offsets, int B, int chunk, const EntryBaseRule& R, bool lists = true)
{
    HostBins hb;
    if (lists) { hb.slice_c0.resize(B + 1); hb.slice_eb.resize(B); }
    for (int b = 0; b < B; b++) {
        const int64_t s = h_offsets[b], e = h_offsets[b + 1];
        if (lists) {
            hb.slice_c0[b] = (int)hb.nchunks; hb.slice_eb[b] = hb.entries;
            for (int64_t k = s; k < e; k += chunk) {
                ChunkDesc cd; cd.start = k; cd.n = (int32_t)std::min<int64_t>(chunk, e - k); cd.slice = b;
                hb.cds.push_back(cd);
            }
        }
        hb.entries = (hb.entries + (e - s) * R.per_event + R.slack + R.align - 1) & ~(R.align - 1);
        hb.nchunks += (e - s + chunk - 1) / chunk;
    }
    if (lists) hb.slice_c0[B] = (int)hb.nchunks;
    return hb;
}

// the three host lists into `chunks` (of L.chunks_bytes()) by one copy from the pinned ring
static inline int bin_chunks_upload(eorb_ctx* c, const BinLayout& L, const HostBins& hb, void* chunks, hipStream_t stream)
{
    char* hp = (char*)pinned(c, L.chunks_bytes());
    if (!hp) return set_err(c, EORB_E_HIP, "pinned alloc failed");
    if (L.nchunks) memcpy(hp, hb.cds.data(), sizeof(ChunkDesc) * L.nchunks);
    memcpy(hp + L.cd, hb.slice_c0.data(), sizeof(int) * (size_t)(L.B + 1));
    memcpy(hp + L.cd + L.sc, hb.slice_eb.data(), L.eb);
    EORB_HIP(c, hipMemcpyAsync(chunks, hp, L.chunks_bytes(), hipMemcpyHostToDevice, stream));
    pinned_commit(c);
    return EORB_OK;
}

__device__ __forceinline__ uint32_t enc_f32(float f)
{   // order-preserving map float -> uint32 (for atomicMax/atomicMin on floats of either sign)
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_f32(uint32_t e)
{
    uint32_t u = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
    return __uint_as_float(u);
}

// wave-wide inclusive prefix sum without LDS round trips: row_shr 1/2/4/8 inside the 16-lane rows, then row_bcast 15 / 31
__device__ __forceinline__ int wave_incl_scan(int x)
{
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);     // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);     // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);     // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);     // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);     // row_bcast:15 -> rows 1, 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);     // row_bcast:31 -> rows 2, 3
    return x;
}

// wave-wide maximum / minimum of a float by the same DPP steps (a lane without a source keeps its own value): the result is in lane 63
__device__ __forceinline__ float wave_max_to_lane63(float x)
{
#define EORB_DPP_STEP(ctrl, rmask) x = fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), ctrl, rmask, 0xf, false)))
    EORB_DPP_STEP(0x111, 0xf); EORB_DPP_STEP(0x112, 0xf); EORB_DPP_STEP(0x114, 0xf); EORB_DPP_STEP(0x118, 0xf);
    EORB_DPP_STEP(0x142, 0xa); EORB_DPP_STEP(0x143, 0xc);
#undef EORB_DPP_STEP
    return x;
}
__device__ __forceinline__ float wave_min_to_lane63(float x)
{
#define EORB_DPP_STEP(ctrl, rmask) x = fminf(x, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(x), __float_as_int(x), ctrl, rmask, 0xf, false)))
    EORB_DPP_STEP(0x111, 0xf); EORB_DPP_STEP(0x112, 0xf); EORB_DPP_STEP(0x114, 0xf); EORB_DPP_STEP(0x118, 0xf);
    EORB_DPP_STEP(0x142, 0xa); EORB_DPP_STEP(0x143, 0xc);
#undef EORB_DPP_STEP
    return x;
}

}  // namespace eorb
