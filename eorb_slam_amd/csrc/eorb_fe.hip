// eorb_fe.hip -- C ABI of libeorb_fe.so (include/eorb_fe.h): context, host-buffer entry points and the
// batched HBM-resident front end.  No CPU fallback anywhere: every entry point launches HIP kernels.
#include "eorb_ctx.h"
#include "match_args.h"
#include "project_args.h"
#include "kfdb.h"
#include "twoview.h"
#include "sim3.h"
#include "mlpnp.h"
#include "newpts.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <vector>

namespace eorb {

int set_err(eorb_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    if (c) c->err = buf;
    return code;
}

int hip_check(eorb_ctx* c, hipError_t e, const char* what)
{
    return set_err(c, EORB_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

int ensure(eorb_ctx* c, DevBuf& b, size_t bytes)
{
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return EORB_OK;
    if (b.p) { hipError_t e = hipFree(b.p); b.p = nullptr; b.cap = 0; if (e != hipSuccess) return hip_check(c, e, "hipFree"); }
    const size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) { b.p = nullptr; return hip_check(c, e, "hipMalloc"); }
    b.cap = want;
    // test hook "dirty_fill": the allocation starts out as the byte, whole, before anyone (on any stream) can use it
    if (c && c->opt.dirty_fill >= 0) {
        if ((e = hipMemset(b.p, c->opt.dirty_fill, want)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) return hip_check(c, e, "hipMemset (dirty_fill)");
    }
    return EORB_OK;
}

// every stream wait of an entry point: what it enqueued has completed, its staging slots are free again
static hipError_t fe_stream_sync(eorb_ctx* c)
{
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) pinned_release_lazy(c);
    return e;
}
// entry prologue: the context's device
static void fe_enter(eorb_ctx* c) { hipSetDevice(c->device); }

void* pinned(eorb_ctx* c, size_t bytes)
{
    eorb_ctx::PinnedSlot& s = c->pinned[c->pinned_next];
    c->pinned_cur = c->pinned_next;
    c->pinned_next = (c->pinned_next + 1) % eorb_ctx::kPinnedSlots;
    if (s.busy) {                                                   // the copy / kernel that read this slot has completed
        if (s.lazy) { hipStreamSynchronize(c->stream); pinned_release_lazy(c); }
        else hipEventSynchronize(s.ev);
        s.busy = false; s.lazy = false;
    }
    if (s.cap >= bytes) return s.p;
    if (s.p) { hipHostFree(s.p); s.p = nullptr; s.cap = 0; }
    const size_t want = bytes + bytes / 2 + 4096;
    if (hipHostMalloc(&s.p, want, hipHostMallocDefault) != hipSuccess) { s.p = nullptr; return nullptr; }
    s.cap = want;
    return s.p;
}

void pinned_release_lazy(eorb_ctx* c)
{
    for (auto& s : c->pinned) if (s.busy && s.lazy) { s.busy = false; s.lazy = false; }
}

// lazy: the host-buffer entry points wait for their results before they return, which covers every read of their staging slot: an event
// per slot was a marker in the queue in front of the call's next kernel (5 us of idle GPU per call in the time line)
void pinned_commit(eorb_ctx* c, bool lazy)
{
    if (c->pinned_cur < 0) return;
    eorb_ctx::PinnedSlot& s = c->pinned[c->pinned_cur];
    if (lazy) { s.busy = true; s.lazy = true; return; }
    if (!s.ev && hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) != hipSuccess) { s.ev = nullptr; hipStreamSynchronize(c->stream); return; }
    if (hipEventRecord(s.ev, c->stream) != hipSuccess) { hipStreamSynchronize(c->stream); return; }
    s.busy = true;
}

ProfScope::ProfScope(eorb_ctx* cc, const char* name, hipStream_t stream) : c(cc), idx(-1), st(stream ? stream : cc->stream)
{
    if (!c->prof) return;
    if (!c->prof_only.empty() && c->prof_only.find(std::string(",") + name + ",") == std::string::npos) return;
    for (size_t i = 0; i < c->profs.size(); i++) if (c->profs[i].name == name) { idx = (int)i; break; }
    if (idx < 0) { c->profs.emplace_back(); c->profs.back().name = name; idx = (int)c->profs.size() - 1; }
    // events come from a pool (creating a pair costs several microseconds: visible on the one-frame-per-call paths)
    auto take = [&](hipEvent_t& e) { if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); } else hipEventCreate(&e); };
    take(a); take(b);
    hipEventRecord(a, st);
}
ProfScope::~ProfScope()
{
    if (idx < 0) return;
    hipEventRecord(b, st);
    c->profs[idx].pending.emplace_back(a, b);
    c->profs[idx].launches++;
}

void prof_collect(eorb_ctx* c)
{
    for (auto& p : c->profs) {
        for (auto& ev : p.pending) {
            hipEventSynchronize(ev.second);
            float ms = 0; hipEventElapsedTime(&ms, ev.first, ev.second);
            p.total_ms += ms;
            c->ev_pool.push_back(ev.first); c->ev_pool.push_back(ev.second);
        }
        p.pending.clear();
    }
}

int* readback_buf(eorb_ctx* c)
{
    if (!c->rb_pinned && hipHostMalloc((void**)&c->rb_pinned, 64 * sizeof(int), hipHostMallocDefault) != hipSuccess) c->rb_pinned = nullptr;
    return c->rb_pinned;
}

static void free_buf(DevBuf& b) { if (b.p) hipFree(b.p); b.p = nullptr; b.cap = 0; }

// Host-buffer entry points are called once per frame (src/Frame.cc:467-482, src/Tracking.cc:1420, EvImBuilder.cpp:1345): their
// latency is launches and copies, not kernels.  A call lays ALL its inputs and outputs out in one device arena: the inputs are
// packed into a pinned slot and cross PCIe in ONE copy (a pageable hipMemcpy2DAsync of a 346x260 image alone cost > 1 ms), the
// outputs come back in ONE copy into a pinned landing buffer.  Beyond 1 MB the copy engine moves them: staged inputs in 4 MB pieces,
// and an array of 4 MB or more straight between the caller's buffer and the arena (Arena::upload, Arena::download_to).
// upload of a call's inputs by a kernel that reads the pinned staging buffer over the link (16 bytes per thread, coalesced): for the few
// hundred KB of a one-frame call the copy engine's turn plus its hand-over to the first kernel cost more (SearchByProjection: copy 11 us +
// 12-15 us idle before the first kernel) than these reads
__global__ void arena_upload_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

struct Arena {
    static constexpr size_t kPiece = (size_t)4 << 20;      // large calls: staged copy-engine transfers go in pieces of this size, larger arrays go directly
    eorb_ctx* c;
    size_t total = 0, in_end = 0;
    struct Part { const void* src; size_t off, bytes; int rows; size_t row_bytes, stride; bool pack = false; };
    std::vector<Part> parts;
    explicit Arena(eorb_ctx* cc) : c(cc) {}
    size_t take(size_t bytes) { const size_t o = total; total = (total + std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; return o; }
    // inputs first (they form the prefix that is uploaded), then out() for the outputs (below) and reserve() for device-only regions
    size_t in(const void* h, size_t bytes) { const size_t o = take(bytes); if (h && bytes) parts.push_back({h, o, bytes, 0, 0, 0}); in_end = total; return o; }
    // float events, packed to the 16-byte record (eorb_pack_events) straight into the staging buffer
    size_t in_events(const eorb_event* ev, size_t n)
    {
        const size_t o = in(ev, sizeof(eorb_event16) * n);
        if (ev && n) parts.back().pack = true;
        return o;
    }
    size_t in2d(const void* h, int rows, size_t row_bytes, size_t stride)
    {
        const size_t o = take((size_t)rows * row_bytes);
        if (stride == row_bytes) parts.push_back({h, o, (size_t)rows * row_bytes, 0, 0, 0});
        else parts.push_back({h, o, 0, rows, row_bytes, stride});
        in_end = total; return o;
    }
    size_t reserve(size_t bytes) { return take(bytes); }
    template <typename T> T* dev(size_t off) const { return (T*)((char*)c->arena.p + off); }
    // host_inputs: the inputs are NOT copied to the arena; the kernels that read them (once) get the pinned staging buffer itself
    // (in_ptr), which the device reads over the link.  For a few KB this saves the copy engine's turn and its hand-over to the first
    // kernel (tools/mb/call_latency.hip: 25 -> 21 us per call).  inputs_done() after the last kernel that reads them is enqueued.
    bool host_inputs = false; char* host_base = nullptr;
    template <typename T> T* in_ptr(size_t off) const { return host_inputs ? (T*)(host_base + off) : dev<T>(off); }
    void inputs_done() {}                            // (the slot stays taken until the call's wait: pinned_commit(lazy) in upload())
    int upload()
    {
        int rc = ensure(c, c->arena, total);
        if (rc) return rc;
        c->arena_gen++;                              // (whatever an earlier call left in the arena is gone)
        c->arena_calls++; c->arena_bytes += (long long)total; c->arena_in_bytes += (long long)in_end;
        const int dirty = c->opt.dirty_fill;        // test hook "dirty_fill": the whole arena and the staging slot hold the byte before any input goes in
        if (dirty >= 0) EORB_HIP(c, hipMemsetAsync(c->arena.p, dirty, c->arena.cap, c->stream));
        if (!in_end) return EORB_OK;
        char* hp = (char*)pinned(c, in_end);
        if (!hp) return set_err(c, EORB_E_HIP, "pinned alloc failed");
        if (dirty >= 0) memset(hp, dirty, in_end);
        const long kmax = (long)c->opt.upload_kernel_max;      // (bytes; 0: always the copy engine)
        // the copy engine takes the staging buffer in pieces of kPiece as it fills: tens of MB are copied in while the host packs the rest;
        // an array of kPiece or more goes straight from the caller's buffer (the runtime copies pageable memory of that size in place,
        // twice as fast as through a staging buffer: 16 MB in 0.30 ms against 0.50 ms)
        const bool engine = !host_inputs && (long)in_end > kmax;
        size_t sent = 0;
        auto send = [&](size_t upto) {
            const hipError_t e = upto > sent ? hipMemcpyAsync((char*)c->arena.p + sent, hp + sent, upto - sent, hipMemcpyHostToDevice, c->stream) : hipSuccess;
            sent = upto;
            return e;
        };
        for (const Part& p : parts) {
            if (engine && !p.rows && !p.pack && p.bytes >= kPiece) {
                EORB_HIP(c, send(p.off));
                EORB_HIP(c, hipMemcpyAsync((char*)c->arena.p + p.off, p.src, p.bytes, hipMemcpyHostToDevice, c->stream));
                sent = p.off + p.bytes;
            } else if (p.rows) for (int r = 0; r < p.rows; r++) memcpy(hp + p.off + (size_t)r * p.row_bytes, (const char*)p.src + (size_t)r * p.stride, p.row_bytes);
            else for (size_t q = 0; q < p.bytes; q += kPiece) {
                const size_t m = std::min(kPiece, p.bytes - q);
                if (p.pack) eorb_pack_events((const eorb_event*)p.src + q / sizeof(eorb_event16), m / sizeof(eorb_event16), (eorb_event16*)(hp + p.off + q));
                else memcpy(hp + p.off + q, (const char*)p.src + q, m);
                if (engine && p.off + q + m - sent >= kPiece) EORB_HIP(c, send(p.off + q + m));
            }
        }
        if (host_inputs) { host_base = hp; pinned_commit(c, true); return EORB_OK; }
        if (engine) EORB_HIP(c, send(in_end));
        else {
            const size_t n16 = (in_end + 15) / 16;          // (offsets and sizes of the arena are multiples of 256; the staging buffer is at least as long)
            arena_upload_kernel<<<(unsigned)std::min<size_t>((n16 + 255) / 256, 512), 256, 0, c->stream>>>((const uint4*)hp, (uint4*)c->arena.p, n16);
            EORB_LAUNCH_CHECK(c, "arena_upload_kernel");
        }
        pinned_commit(c, true);
        return EORB_OK;
    }
    // one D2H copy of arena[off, off + bytes) + a wait for it; returns the host view of arena offset `off` (valid until the next call).
    // download_begin / download_wait: the same in two halves -- what the caller launches in between (work the results do not depend on:
    // the LK reference kept for the next call) runs after the copy and is not waited for.
    size_t dl_off = 0;
    void count_download(size_t off, size_t bytes) { c->arena_downloads++; c->arena_download_bytes += (long long)bytes; c->arena_download_first += (long long)off; }
    long download_kmax() const { return (long)c->opt.download_kernel_max; }      // (bytes; 0: always the copy engine)
    int landing(size_t bytes)
    {
        if (c->dl_cap >= bytes) return EORB_OK;
        if (c->dl_pinned) { hipHostFree(c->dl_pinned); c->dl_pinned = nullptr; c->dl_cap = 0; }
        const size_t want = bytes + bytes / 2 + 4096;
        if (hipHostMalloc(&c->dl_pinned, want, hipHostMallocDefault) != hipSuccess) { c->dl_pinned = nullptr; return set_err(c, EORB_E_HIP, "pinned alloc failed"); }
        c->dl_cap = want;
        return EORB_OK;
    }
    int download_begin(size_t off, size_t bytes)
    {
        int rc = landing(bytes);
        if (rc) return rc;
        count_download(off, bytes);
        if (c->opt.dirty_fill >= 0) memset(c->dl_pinned, c->opt.dirty_fill, c->dl_cap);      // (test hook: a host read outside the downloaded range sees the byte)
        // (the way back like the way in: up to a few hundred KB a kernel writes the pinned buffer; offsets of the arena are multiples of
        // 256 and both buffers longer than the rounded size)
        if ((long)bytes <= download_kmax() && !(off & 15)) {
            const size_t n16 = (bytes + 15) / 16;
            arena_upload_kernel<<<(unsigned)std::min<size_t>((n16 + 255) / 256, 512), 256, 0, c->stream>>>((const uint4*)((char*)c->arena.p + off), (uint4*)c->dl_pinned, n16);
            EORB_LAUNCH_CHECK(c, "arena download kernel");
        } else
        EORB_HIP(c, hipMemcpyAsync(c->dl_pinned, (char*)c->arena.p + off, bytes, hipMemcpyDeviceToHost, c->stream));
        if (!c->dl_event && hipEventCreateWithFlags(&c->dl_event, hipEventDisableTiming) != hipSuccess) { c->dl_event = nullptr; return set_err(c, EORB_E_HIP, "event"); }
        EORB_HIP(c, hipEventRecord(c->dl_event, c->stream));
        dl_off = off;
        return EORB_OK;
    }
    int download_wait(const char** host)
    {
        // sync_spin (EORB_SYNC_SPIN=1): poll instead of blocking (one 2 000-event slice through ev2im_gauss + detect: p50 0.260 ->
        // 0.237 ms, p95 0.277 -> 0.326 ms, and a CPU core kept busy: off by default)
        if (c->opt.sync_spin) {
            hipError_t q;
            while ((q = hipEventQuery(c->dl_event)) == hipErrorNotReady) {}
            if (q != hipSuccess) return hip_check(c, q, "hipEventQuery");
        } else
            EORB_HIP(c, hipEventSynchronize(c->dl_event));
        pinned_release_lazy(c);
        *host = (const char*)c->dl_pinned - dl_off;
        return EORB_OK;
    }
    int download(size_t off, size_t bytes, const char** host)
    {
        int rc = download_begin(off, bytes);
        if (rc) return rc;
        if ((rc = download_wait(host))) return rc;
        // (profiling: the scopes' events are collected when the stream is idle -- eorb_prof_* synchronise before they read)
        return EORB_OK;
    }
    // The outputs are declared like the inputs, and registration order is layout order:
    //   out(dst, bytes)        reserves a region that fetch() copies to dst; dst == NULL: the region exists, the kernels write it, nobody takes it
    //   inout(dst, off, bytes) the same for a region that exists already (an input that comes back)
    //   want(off, bytes)       only extends the fetched span over a region: nothing is copied, the caller reads it through fetch()'s host
    //                          view (count words, and records whose number is known only after the download)
    // fetch(): ONE download of arena[first wanted offset, end of the last wanted region), the wait, then the copies.  fetch_begin() /
    // fetch_wait(): its two halves (download_begin / download_wait).  Nothing wanted: fetch() only waits for the call's kernels.
    struct Out { void* dst; size_t off, bytes; };
    static constexpr int kMaxOuts = 32;                    // (a fixed array: no allocation on the one-call paths)
    Out outs[kMaxOuts]; int nouts = 0; bool outs_full = false;
    size_t want_lo = ~(size_t)0, want_hi = 0;
    void want(size_t off, size_t bytes) { if (bytes) { want_lo = std::min(want_lo, off); want_hi = std::max(want_hi, off + bytes); } }
    void inout(void* dst, size_t off, size_t bytes)
    {
        if (!dst || !bytes) return;
        if (nouts == kMaxOuts) { outs_full = true; return; }
        want(off, bytes); outs[nouts++] = Out{dst, off, bytes};
    }
    size_t out(void* dst, size_t bytes) { const size_t o = take(bytes); inout(dst, o, bytes); return o; }
    void copy_out(const char* h) const { for (int i = 0; i < nouts; i++) memcpy(outs[i].dst, h + outs[i].off, outs[i].bytes); }
    int fetch_begin()
    {
        if (outs_full) return set_err(c, EORB_E_HIP, "internal error: a call registered more than %d outputs", kMaxOuts);
        return download_begin(want_lo, want_hi - want_lo);
    }
    int fetch_wait(const char** host = nullptr)
    {
        const char* h;
        if (const int rc = download_wait(&h)) return rc;
        copy_out(h);
        if (host) *host = h;
        return EORB_OK;
    }
    int fetch(const char** host = nullptr)
    {
        if (!want_hi) { EORB_HIP(c, fe_stream_sync(c)); return EORB_OK; }
        if (const int rc = fetch_begin()) return rc;
        return fetch_wait(host);
    }
    // download() + memcpy(dst, ...) for one result; from kPiece on the copy engine writes the caller's buffer itself (as for the inputs)
    int download_to(void* dst, size_t off, size_t bytes)
    {
        int rc;
        if (bytes < kPiece) {
            const char* h;
            if ((rc = download(off, bytes, &h))) return rc;
            memcpy(dst, h + off, bytes);
            return EORB_OK;
        }
        count_download(off, bytes);
        EORB_HIP(c, hipMemcpyAsync(dst, (char*)c->arena.p + off, bytes, hipMemcpyDeviceToHost, c->stream));
        EORB_HIP(c, fe_stream_sync(c));
        return EORB_OK;
    }
};

// setup data that persists across calls (undistortion maps, vocabulary): `fill` writes it into a pinned slot, one copy into `b`, one wait
template <typename Fill> static int upload_persistent(eorb_ctx* c, DevBuf& b, size_t bytes, Fill fill)
{
    int rc = ensure(c, b, bytes);
    if (rc) return rc;
    char* hp = (char*)pinned(c, bytes);
    if (!hp) return set_err(c, EORB_E_HIP, "pinned alloc failed");
    fill(hp);
    EORB_HIP(c, hipMemcpyAsync(b.p, hp, bytes, hipMemcpyHostToDevice, c->stream));
    pinned_commit(c, true);
    EORB_HIP(c, fe_stream_sync(c));
    return EORB_OK;
}

}  // namespace eorb

using namespace eorb;

extern "C" {

const char* eorb_version(void) { return "eorb_fe 0.1.0 (gfx950)"; }

int eorb_create(int device, void* hip_stream, eorb_ctx** out)
{
    if (!out) return EORB_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return EORB_E_HIP;
    if (device < 0 || device >= ndev) return EORB_E_ARG;
    if (hipSetDevice(device) != hipSuccess) return EORB_E_HIP;
    eorb_ctx* c = new eorb_ctx();
    c->opt = c->opt_created = options_from_env();
    c->device = device;
    if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->own_stream = false; }
    else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return EORB_E_HIP; }
        c->own_stream = true;
    }
    if (ensure(c, c->status, 64) != EORB_OK || hipMemsetAsync(c->status.p, 0, 64, c->stream) != hipSuccess) { eorb_destroy(c); return EORB_E_HIP; }
    *out = c;
    return EORB_OK;
}

void eorb_destroy(eorb_ctx* c)
{
    if (!c) return;
    fe_enter(c);
    hipStreamSynchronize(c->stream);
    prof_collect(c);
    DevBuf* bufs[] = {&c->ev16, &c->chunks, &c->segoff, &c->entries, &c->img_f32, &c->img_u8, &c->minmax, &c->tile_order, &c->order_hist, &c->sl_trace, &c->dd_ev, &c->dd_cnt, &c->focus_sd, &c->voc, &c->klt_pyr, &c->klt_der, &c->klt_scratch, &c->pyr, &c->score,
                      &c->blur, &c->cell_cnt, &c->cell_cand, &c->lvl_cnt, &c->lvl_kp, &c->kp_angle, &c->out_kp, &c->out_desc,
                      &c->out_oob, &c->out_n, &c->oct_scratch, &c->fe_prev_kp, &c->fe_prev_desc, &c->fe_prev_n, &c->fe_pm,
                      &c->fe_matches12, &c->fe_nmatches,
                      &c->orb.tabs, &c->orb.geom, &c->status, &c->win_ws, &c->win_total, &c->arena, &c->l1_ref_img, &c->l1_ref_pts, &c->ev_info, &c->ev_stamps, &c->pd_hash, &c->pd_cnt};
    for (DevBuf* b : bufs) free_buf(*b);
    for (PosTables* t : {&c->maps, &c->dd, &c->pd})
        for (DevBuf* b : {&t->lut, &t->src_info, &t->stamps, &t->sl_tab, &t->sl_tile, &t->sl_rows}) free_buf(*b);
    kfdb_free(c);
    for (auto& s : c->pinned) { if (s.ev) hipEventDestroy(s.ev); if (s.p) hipHostFree(s.p); }
    for (hipEvent_t e : c->ev_pool) hipEventDestroy(e);
    if (c->dl_pinned) hipHostFree(c->dl_pinned);
    if (c->dl_event) hipEventDestroy(c->dl_event);
    if (c->rb_pinned) hipHostFree(c->rb_pinned);
    for (hipEvent_t e : c->sl_ev) if (e) hipEventDestroy(e);
    if (c->sl_side) hipStreamDestroy(c->sl_side);
    if (c->sl_pstream) hipStreamDestroy(c->sl_pstream);
    if (c->sl_gstream) hipStreamDestroy(c->sl_gstream);
    for (auto& w : c->sl_ws) { free_buf(w.chunks); free_buf(w.segoff); free_buf(w.entries); free_buf(w.tile_order); free_buf(w.plan); free_buf(w.hot); free_buf(w.rec16); }
    if (c->own_stream) hipStreamDestroy(c->stream);
    delete c;
}

int eorb_sync(eorb_ctx* c)
{
    if (!c) return EORB_E_ARG;
    fe_enter(c);
    EORB_HIP(c, fe_stream_sync(c));
    // sticky status of the asynchronous (*_dev) paths: kernels OR their overflow bits into a device word; report it once
    int32_t bits = 0;
    EORB_HIP(c, hipMemcpyAsync(&bits, c->status.p, sizeof(bits), hipMemcpyDeviceToHost, c->stream));
    EORB_HIP(c, fe_stream_sync(c));
    if (bits) {
        EORB_HIP(c, hipMemsetAsync(c->status.p, 0, sizeof(bits), c->stream));
        if (bits & 256)
            return set_err(c, EORB_E_HIP, "internal error: the slot gather found its LDS rows at a non-zero base (status %d); the images of that call were not written", bits);
        return set_err(c, EORB_E_CAPACITY, "a batched call exceeded an internal capacity (octree flags %d: 1 = candidates, 2 = node pool / "
                       "size list, 4 = keypoints per level); its keypoints are truncated", bits);
    }
    return EORB_OK;
}

int eorb_debug_option(eorb_ctx* c, const char* name, int value)
{
    if (!c || !name) return EORB_E_ARG;
    if (!strcmp(name, "dirty_fill") && (value < -1 || value > 255)) return set_err(c, EORB_E_ARG, "dirty_fill: -1 (off) or a byte 0..255, not %d", value);
    if (option_set(c->opt, c->opt_created, name, value)) {
        if (!strcmp(name, "position_dict") && !value) { c->pd_valid = 0; c->dd_keep = 0; }
        return EORB_OK;
    }
    return set_err(c, EORB_E_ARG, "debug option '%s' unknown", name);
}

int eorb_debug_option_get(eorb_ctx* c, const char* name, long long* value)
{
    if (!c || !name || !value) return EORB_E_ARG;
    if (option_get(c->opt, name, value)) return EORB_OK;
    return set_err(c, EORB_E_ARG, "debug option '%s' unknown", name);
}

int eorb_debug_stage(eorb_ctx* c, const char* name, int slice, int level, void* out, size_t cap_bytes, int* dim0, int* dim1)
{
    if (!c || !name) return EORB_E_ARG;
    fe_enter(c);
    return orb_debug_stage(c, name, slice, level, out, cap_bytes, dim0, dim1);
}

long long eorb_debug_counter(eorb_ctx* c, const char* name)
{
    if (!c || !name) return -1;
    if (!strcmp(name, "slot_calls")) return c->sl_calls;
    if (!strcmp(name, "accum_route")) return c->accum_route;
    if (!strcmp(name, "slot_rank_ok")) return c->sl_rank_ok;
    if (!strcmp(name, "dict_hits")) return c->pd_hits;                    // bulk float calls served by the frozen position dictionary
    if (!strcmp(name, "dict_misses")) return c->pd_misses;                // ... that found a new position and tabulated afresh
    if (!strcmp(name, "dict_positions")) return c->pd_valid ? c->pd_K : 0;
    if (!strcmp(name, "slot_scatter_form")) return c->sl_last_rank;       // the scatter of the last slot-form call: 1 rank form, 0 ballot form
    if (!strcmp(name, "slot_chunk")) return c->sl_last_chunk;
    if (!strcmp(name, "slot_binning")) return c->sl_last_binning;         // count | record << 2 | scatter << 4 of the last slot-form call (ev_plan.h SlotBinPlan)
    if (!strcmp(name, "kfdb_slot_cap")) return c->kfdb.slot_cap;          // KeyFrameDatabase pools: slots / words they hold room for
    if (!strcmp(name, "kfdb_word_cap")) return c->kfdb.word_cap;
    // host-buffer calls, cumulative over the context's life: arenas laid out and their bytes (all / the uploaded prefix); downloads, their
    // bytes and the sum of their first offsets
    if (!strcmp(name, "arena_calls")) return c->arena_calls;
    if (!strcmp(name, "arena_bytes")) return c->arena_bytes;
    if (!strcmp(name, "arena_in_bytes")) return c->arena_in_bytes;
    if (!strcmp(name, "arena_downloads")) return c->arena_downloads;
    if (!strcmp(name, "arena_download_bytes")) return c->arena_download_bytes;
    if (!strcmp(name, "arena_download_first")) return c->arena_download_first;
    if (!strcmp(name, "slot_parts")) return c->sl_last_parts;              // 2: the last slot-form call ran its batch as two halves
    if (!strcmp(name, "slot_hot_overflow")) {           // lists the last slot-form call handed back to the LDS gather because their length bucket was full (synchronises)
        long long n = 0;
        for (int part = 0; part < std::max(c->sl_last_parts, 1); part++) {
            if (!c->sl_ws[part].hot.p) continue;
            uint32_t h = 0;
            if (hipMemcpyAsync(&h, (uint32_t*)c->sl_ws[part].hot.p + 33, sizeof(h), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -1;
            n += h;
        }
        return n;
    }
    if (!strcmp(name, "win_total_nonzero")) {           // window matchers: pairs whose entry counter is not back at zero (synchronises)
        const size_t n = c->win_total.p ? c->win_total.cap / sizeof(uint32_t) : 0;
        if (!n) return 0;
        std::vector<uint32_t> t(n);
        if (hipMemcpyAsync(t.data(), c->win_total.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -1;
        long long nz = 0; for (uint32_t v : t) nz += v != 0;
        return nz;
    }
    if (!strcmp(name, "oct_lds_only")) return c->orb.oct_all_lds[0] | (c->orb.oct_all_lds[1] << 1);      // octree working set entirely in LDS: single frames | batches
    if (!strcmp(name, "oct_lds_bytes")) return c->orb.oct_lds[0];
    if (!strcmp(name, "oct_dynamic")) return c->orb.oct_dyn[0] != 0 ? 1 : 0;          // single frames use the dynamic LDS placement
    if (!strcmp(name, "oct_redo_levels")) {                                            // levels of the last single-frame extraction that did not fit it (synchronises)
        const int nl = c->orb.nlevels;
        if (!c->orb.oct_dyn[0] || !c->lvl_cnt.p || nl <= 0) return 0;
        std::vector<int32_t> f((size_t)nl);
        if (hipMemcpyAsync(f.data(), (const char*)c->lvl_cnt.p + (size_t)nl * sizeof(int32_t) + 64, sizeof(int32_t) * (size_t)nl, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) return -1;
        long long r = 0; for (int v : f) r += v ? 1 : 0;
        return r;
    }
    if (!strcmp(name, "oct_direct_cap")) return c->orb.oct_direct_cap[0] | ((long long)c->orb.oct_direct_cap[1] << 16);
    if (!strcmp(name, "oct_scratch_bytes")) return c->orb.oct_scratch[0];
    if (!strcmp(name, "slot_hot_items")) {              // lists the last slot-form call handed to the register-row kernel (synchronises)
        long long n = 0;
        for (int part = 0; part < std::max(c->sl_last_parts, 1); part++) {
            if (!c->sl_ws[part].hot.p) continue;
            uint32_t h[16];
            if (hipMemcpyAsync(h, c->sl_ws[part].hot.p, sizeof(h), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -1;
            for (int i = 0; i < 16; i++) n += h[i];      // (sl_tasks_kernel capped the counts at the buckets' capacity)
        }
        return n;
    }
    if (!strcmp(name, "slot_entries") || !strcmp(name, "slot_hot_entries")) {
        // list entries the last slot-form call's gather kernels walked: all of them / those of the lists handed to the register-row kernel
        // (synchronises; reads the scan's per-(slice, tile) counts and the hot descriptors back)
        const bool hot = name[5] == 'h';
        if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
        long long n = 0;
        for (int part = 0; part < std::max(c->sl_last_parts, 1); part++) {
            const eorb_ctx::SlotWS& w = c->sl_ws[part];
            if (hot) {
                if (!w.hot.p) continue;
                uint32_t cnt[16];
                if (hipMemcpy(cnt, w.hot.p, sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess) return -1;
                for (int b = 0; b < 16; b++) {
                    std::vector<uint32_t> d(8 * (size_t)cnt[b]);
                    if (cnt[b] && hipMemcpy(d.data(), (const char*)w.hot.p + 256 + (size_t)b * 8192 * 32, 32 * (size_t)cnt[b], hipMemcpyDeviceToHost) != hipSuccess) return -1;
                    for (uint32_t k = 0; k < cnt[b]; k++) n += d[8 * (size_t)k + 2];
                }
            } else {
                if (!w.tile_order.p || !c->sl_last_nb[part]) continue;
                std::vector<uint32_t> t((size_t)c->sl_last_nb[part]);
                if (hipMemcpy(t.data(), w.tile_order.p, sizeof(uint32_t) * t.size(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
                for (uint32_t v : t) n += v;
            }
        }
        return n;
    }
    if (!strcmp(name, "slot_flags")) {
        const PosTables& T = c->maps;                         // (the maps' slot tables, whatever the float calls built)
        if (!T.sl_tile.p || !T.sl_info_off) return 0;
        int flags = 0;
        if (hipMemcpyAsync(&flags, (char*)T.sl_tile.p + T.sl_info_off + 3 * sizeof(int), sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
        return flags;
    }
    return -1;
}

const char* eorb_last_error(eorb_ctx* c) { return c ? c->err.c_str() : "null context"; }

int eorb_prof_enable(eorb_ctx* c, int on) { if (!c) return EORB_E_ARG; c->prof = on != 0; return EORB_OK; }
int eorb_prof_only(eorb_ctx* c, const char* names)
{
    if (!c) return EORB_E_ARG;
    c->prof_only = (names && *names) ? std::string(",") + names + "," : std::string();
    return EORB_OK;
}
int eorb_prof_reset(eorb_ctx* c)
{
    if (!c) return EORB_E_ARG;
    hipStreamSynchronize(c->stream);
    prof_collect(c);
    c->profs.clear();
    return EORB_OK;
}
int eorb_prof_count(eorb_ctx* c) { if (!c) return EORB_E_ARG; hipStreamSynchronize(c->stream); prof_collect(c); return (int)c->profs.size(); }
int eorb_prof_get(eorb_ctx* c, int i, const char** name, double* total_ms, int64_t* launches)
{
    if (!c || i < 0 || i >= (int)c->profs.size()) return EORB_E_ARG;
    if (name) *name = c->profs[i].name.c_str();
    if (total_ms) *total_ms = c->profs[i].total_ms;
    if (launches) *launches = c->profs[i].launches;
    return EORB_OK;
}

void eorb_pack_events(const eorb_event* ev, size_t n, eorb_event16* out)
{
    for (size_t i = 0; i < n; i++) {
        out[i].x = ev[i].x; out[i].y = ev[i].y;
        double t = ev[i].ts < 0 ? 0.0 : ev[i].ts;
        uint64_t u; memcpy(&u, &t, 8);
        if (!ev[i].p) u |= 0x8000000000000000ull;
        memcpy(&out[i].t, &u, 8);
    }
}

void* eorb_dev_alloc(eorb_ctx* c, size_t bytes)
{
    if (!c) return nullptr;
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { set_err(c, EORB_E_HIP, "hipMalloc(%zu) failed", bytes); return nullptr; }
    return p;
}
int eorb_dev_free(eorb_ctx* c, void* p) { if (!c) return EORB_E_ARG; fe_enter(c); hipStreamSynchronize(c->stream); EORB_HIP(c, hipFree(p)); return EORB_OK; }
int eorb_dev_upload(eorb_ctx* c, void* d, const void* h, size_t bytes)
{
    if (!c) return EORB_E_ARG;
    fe_enter(c);
    EORB_HIP(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    EORB_HIP(c, fe_stream_sync(c));
    return EORB_OK;
}
int eorb_dev_download(eorb_ctx* c, void* h, const void* d, size_t bytes)
{
    if (!c) return EORB_E_ARG;
    fe_enter(c);
    EORB_HIP(c, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
    EORB_HIP(c, fe_stream_sync(c));
    return EORB_OK;
}

// ---- event accumulation, host buffers -------------------------------------------------------------
static int ev_host_common(eorb_ctx* c, const eorb_event* ev, size_t n, int W, int H, float sigma, int pol, int normalized,
                          int mode_count, float* out_f32, uint8_t* out_u8, float* minmax, int* is_u8,
                          const eorb_raw_event* rawev = nullptr)
{
    if (!c) return EORB_E_ARG;
    const int raw = rawev != nullptr;
    if (raw && !c->maps.w) return set_err(c, EORB_E_NOTCONF, "ev2im_raw: eorb_set_undistort_maps not called");
    if (raw) ev = nullptr;
    if (W <= 0 || H <= 0 || (n && !ev && !raw)) return set_err(c, EORB_E_ARG, "ev2im: bad arguments");
    fe_enter(c);
    int rc;
    const size_t npix = (size_t)W * H;
    static_assert(sizeof(eorb_raw_event) == sizeof(eorb_event16), "raw and packed events share the 16-byte slot");
    std::vector<eorb_event16> packed;
    if (n && raw) {
        for (size_t i = 0; i < n; i++)
            if ((int)rawev[i].x >= c->maps.w || (int)rawev[i].y >= c->maps.h)       // the reference asserts (MyCalibrator.cpp:176)
                return set_err(c, EORB_E_ARG, "ev2im_raw: event %zu at (%u,%u) lies outside the %dx%d maps", i, rawev[i].x, rawev[i].y,
                               c->maps.w, c->maps.h);
    } else if (n) {
        packed.resize(n);
        eorb_pack_events(ev, n, packed.data());
    }
    Arena A(c);
    // (a live slice goes to the binning-free form, which reads every event once: in place, from the pinned staging buffer)
    A.host_inputs = c->opt.slice_zero_copy != 0 && plan_host_events(accum_shape(W, H, sigma, mode_count, 1, (int64_t)n), AccumRequest{raw, pol, mode_count, 1}, accum_knobs(c));
    const size_t o_ev = A.in(raw ? (const void*)rawev : (const void*)packed.data(), sizeof(eorb_event16) * n);
    // outputs: min/max (encoded | decoded; read through the host view) | u8 image | f32 image
    const size_t o_mm = A.out(nullptr, 64), o_u8 = A.out(out_u8, npix), o_f32 = A.out(out_f32, sizeof(float) * npix);
    A.want(o_mm, 64);
    if ((rc = A.upload())) return rc;
    int64_t offs[2] = {0, (int64_t)n};
    uint32_t* mm = A.dev<uint32_t>(o_mm);
    uint8_t* d_u8 = A.dev<uint8_t>(o_u8);
    float* d_f32 = A.dev<float>(o_f32);
    if (out_u8 && mode_count) EORB_HIP(c, hipMemsetAsync(d_u8, 0, npix, c->stream));     // count images stay empty when max == min
    rc = ev_accumulate_dev(c, A.in_ptr<void>(o_ev), raw, offs, 1, W, H, sigma, pol, mode_count, d_f32, d_u8, normalized, mm);
    A.inputs_done();
    if (rc) return rc;
    // the slot form reports an internal fault (its gather found no rows at LDS offset 0 and wrote no image) through the sticky status
    // word: this call's copy of it travels with the outputs (word 2 of the min/max block)
    const bool slot_ran = (c->accum_route & kRouteFormMask) == kFormSlots;
    if (slot_ran) EORB_HIP(c, hipMemcpyAsync(mm + 2, c->status.p, 4, hipMemcpyDeviceToDevice, c->stream));
    const char* h;
    if ((rc = A.fetch_begin()) || (rc = A.download_wait(&h))) return rc;
    if (slot_ran) {                                      // (checked before anything reaches the caller's buffers)
        int32_t st; memcpy(&st, h + o_mm + 8, 4);
        if (st & 256) return set_err(c, EORB_E_HIP, "internal error: the slot gather found its LDS rows at a non-zero base; no image was written");
    }
    A.copy_out(h);
    // the running extremes come back in their order-preserving integer encoding (enc_f32 of the gather kernels): decoded here
    float hmm[2];
    for (int k = 0; k < 2; k++) {
        uint32_t e; memcpy(&e, h + o_mm + 4 * k, 4);
        const uint32_t u = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
        memcpy(&hmm[k], &u, 4);
    }
    if (minmax) { minmax[0] = hmm[0]; minmax[1] = hmm[1]; }
    if (is_u8) *is_u8 = mode_count ? (normalized && hmm[1] > hmm[0]) : (normalized != 0);
    return EORB_OK;
}

int eorb_ev2im(eorb_ctx* c, const eorb_event* ev, size_t n, int W, int H, int pol, int normalized,
               float* out_f32, uint8_t* out_u8, float* minmax, int* is_u8)
{
    return ev_host_common(c, ev, n, W, H, 0.f, pol, normalized, 1, out_f32, out_u8, minmax, is_u8);
}

int eorb_ev2im_gauss(eorb_ctx* c, const eorb_event* ev, size_t n, int W, int H, float sigma, int pol,
                     int normalized, float* out_f32, uint8_t* out_u8, float* minmax)
{
    if (c && !(sigma > 0.f)) return set_err(c, EORB_E_ARG, "ev2im_gauss: sigma must be > 0");
    return ev_host_common(c, ev, n, W, H, sigma, pol, normalized, 0, out_f32, out_u8, minmax, nullptr);
}

// ---- raw sensor events + undistortion maps ----------------------------------------------------------
// the maps are in c->maps.lut (uploaded, or written there by calib_maps_dev): everything derived from them is stale
static int install_maps(eorb_ctx* c, int LW, int LH, int checkInImage)
{
    PosTables& T = c->maps;
    T.w = LW; T.h = LH; T.check = checkInImage != 0;
    T.key_W = T.key_H = T.key_mode = -1; T.key_sigma = -1.f;      // derived tables are stale
    return EORB_OK;
}

int eorb_set_undistort_maps(eorb_ctx* c, const float* mapX, const float* mapY, int LW, int LH, int checkInImage)
{
    if (!c) return EORB_E_ARG;
    if (!mapX || !mapY || LW <= 0 || LH <= 0 || LW > 65535 || LH > 65535 || (int64_t)LW * LH >= (1ll << 31))
        return set_err(c, EORB_E_ARG, "set_undistort_maps: bad arguments");
    fe_enter(c);
    const size_t n = (size_t)LW * LH;
    int rc;
    if ((rc = upload_persistent(c, c->maps.lut, sizeof(float) * 2 * n, [&](char* hp) {
            float* xy = (float*)hp;
            for (size_t i = 0; i < n; i++) { xy[2 * i] = mapX[i]; xy[2 * i + 1] = mapY[i]; }
        }))) return rc;
    return install_maps(c, LW, LH, checkInImage);
}

// MyCalibrator::generateUndistMaps (src/Utils/MyCalibrator.cpp:52-102) on the device: the kernel writes c->maps.lut, install_maps does the rest
int eorb_generate_undistort_maps(eorb_ctx* c, int LW, int LH, int checkInImage, float* mapX, float* mapY)
{
    if (!c) return EORB_E_ARG;
    if (!c->calib_set) return set_err(c, EORB_E_NOTCONF, "generate_undistort_maps: eorb_set_calibration not called");
    if (LW <= 0 || LH <= 0 || LW > 65535 || LH > 65535 || (int64_t)LW * LH >= (1ll << 31) || (mapX == nullptr) != (mapY == nullptr))
        return set_err(c, EORB_E_ARG, "generate_undistort_maps: bad arguments");
    fe_enter(c);
    const size_t n = (size_t)LW * LH;
    int rc;
    if ((rc = ensure(c, c->maps.lut, sizeof(float) * 2 * n))) return rc;
    Arena A(c);
    const size_t o_x = A.out(mapX, mapX ? sizeof(float) * n : 0), o_y = A.out(mapY, mapX ? sizeof(float) * n : 0);
    if ((rc = A.upload())) return rc;
    if ((rc = calib_maps_dev(c, LW, LH, (float*)c->maps.lut.p, mapX ? A.dev<float>(o_x) : nullptr, mapX ? A.dev<float>(o_y) : nullptr))) return rc;
    if ((rc = A.fetch())) return rc;                          // (no maps taken: the wait alone)
    return install_maps(c, LW, LH, checkInImage);
}

// MyCalibrator::undistKeyPoints* (:198-283) / undistPoint* (:119-156): records of rec_floats floats whose first two are the point
static int undistort_common(eorb_ctx* c, const char* who, const float* in, int n, float* out, int rec_floats)
{
    if (!c) return EORB_E_ARG;
    if (n < 0 || (n && (!in || !out))) return set_err(c, EORB_E_ARG, "%s: bad arguments", who);
    if (!n) return EORB_OK;                                   // empty vector: nothing to do (:202-205)
    if (!c->calib_set) return set_err(c, EORB_E_NOTCONF, "%s: eorb_set_calibration not called", who);
    const size_t bytes = sizeof(float) * rec_floats * (size_t)n;
    if (!c->calib_dev.gate) { if (out != in) memmove(out, in, bytes); return EORB_OK; }      // vUndistKPts = vDistKPts (:206-210)
    fe_enter(c);
    int rc;
    Arena A(c);
    const size_t o_in = A.in(in, bytes), o_out = A.reserve(bytes);
    if ((rc = A.upload())) return rc;
    if ((rc = calib_points_dev(c, c->calib_dev, A.dev<float>(o_in), A.dev<float>(o_out), n, rec_floats))) return rc;
    return A.download_to(out, o_out, bytes);
}

int eorb_undistort_keypoints(eorb_ctx* c, const eorb_keypoint* in, int n, eorb_keypoint* out)
{
    return undistort_common(c, "undistort_keypoints", (const float*)in, n, (float*)out, 7);
}

int eorb_undistort_points(eorb_ctx* c, const float* xy, int n, float* xy_out)
{
    return undistort_common(c, "undistort_points", xy, n, xy_out, 2);
}

int eorb_undistort_events(eorb_ctx* c, const eorb_raw_event* raw, size_t n, int W, int H, double tsFactor, eorb_event* out, size_t* n_out)
{
    if (!c) return EORB_E_ARG;
    if (!c->maps.w) return set_err(c, EORB_E_NOTCONF, "undistort_events: eorb_set_undistort_maps not called");
    if ((n && (!raw || !out)) || !n_out || W <= 0 || H <= 0) return set_err(c, EORB_E_ARG, "undistort_events: bad arguments");
    fe_enter(c);
    *n_out = 0;
    if (!n) return EORB_OK;
    for (size_t i = 0; i < n; i++)
        if ((int)raw[i].x >= c->maps.w || (int)raw[i].y >= c->maps.h)
            return set_err(c, EORB_E_ARG, "undistort_events: event %zu at (%u,%u) lies outside the %dx%d maps", i, raw[i].x, raw[i].y,
                           c->maps.w, c->maps.h);
    int rc;
    const int nblk = (int)((n + 1023) / 1024);
    Arena A(c);
    const size_t o_raw = A.in(raw, sizeof(eorb_raw_event) * n);
    // block sums (the kept count at [nblk]) | kept events
    const size_t o_blk = A.reserve(sizeof(uint32_t) * ((size_t)nblk + 2)), o_out = A.reserve(sizeof(eorb_event) * n);
    if ((rc = A.upload())) return rc;
    if ((rc = ev_undistort_dev(c, A.dev<eorb_raw_event>(o_raw), n, W, H, tsFactor, A.dev<eorb_event>(o_out), A.dev<uint32_t>(o_blk)))) return rc;
    const char* h;
    if ((rc = A.download(o_blk, sizeof(uint32_t) * ((size_t)nblk + 1), &h))) return rc;
    uint32_t kept;
    memcpy(&kept, h + o_blk + sizeof(uint32_t) * (size_t)nblk, 4);
    if (kept && (rc = A.download_to(out, o_out, sizeof(eorb_event) * kept))) return rc;
    *n_out = kept;
    return EORB_OK;
}

int eorb_parse_events_text(eorb_ctx* c, const char* text, size_t nbytes, eorb_raw_event* out, size_t cap, size_t* n_out,
                           int64_t* bad_line)
{
    if (!c) return EORB_E_ARG;
    if ((nbytes && !text) || !n_out || (cap && !out)) return set_err(c, EORB_E_ARG, "parse_events_text: bad arguments");
    fe_enter(c);
    *n_out = 0; if (bad_line) *bad_line = -1;
    if (!nbytes) return EORB_OK;
    // an event line takes at least 7 bytes (four tokens of one digit each and a byte between two of them: "0 0 0 0") and,
    // but for the last line of the buffer, its '\n': at most (nbytes + 1) / 8 events.  Lines may be as many as bytes (blank ones); the
    // workspaces per line are sized from the counted lines (ev_parse_text_dev)
    const size_t max_events = (nbytes + 1) / 8;
    int rc;
    Arena A(c);
    const size_t o_text = A.in(text, nbytes), o_out = A.reserve(sizeof(eorb_raw_event) * max_events);
    if ((rc = A.upload())) return rc;
    uint32_t res[3];
    if ((rc = ev_parse_text_dev(c, A.dev<char>(o_text), nbytes, A.dev<eorb_raw_event>(o_out), max_events, res))) return rc;
    pinned_release_lazy(c);                              // (ev_parse_text_dev has waited for the stream)
    if (res[2] != 0xffffffffu) {
        if (bad_line) *bad_line = (int64_t)res[2];
        return set_err(c, EORB_E_ARG, "parse_events_text: line %u is outside the accepted \"ts x y p\" grammar", res[2]);
    }
    if (res[1] > max_events) return set_err(c, EORB_E_HIP, "parse_events_text: %u events counted in %zu bytes", res[1], nbytes);
    if (res[1] > cap) return set_err(c, EORB_E_CAPACITY, "parse_events_text: %u events, room for %zu", res[1], cap);
    if (res[1] && (rc = A.download_to(out, o_out, sizeof(eorb_raw_event) * (size_t)res[1]))) return rc;
    *n_out = res[1];
    return EORB_OK;
}

int eorb_ev2im_gauss_raw(eorb_ctx* c, const eorb_raw_event* raw, size_t n, int W, int H, float sigma, int pol, int normalized,
                         float* out_f32, uint8_t* out_u8, float* minmax)
{
    if (c && !(sigma > 0.f)) return set_err(c, EORB_E_ARG, "ev2im_gauss_raw: sigma must be > 0");
    if (c && n && !raw) return set_err(c, EORB_E_ARG, "ev2im_gauss_raw: bad arguments");
    static const eorb_raw_event none{};
    return ev_host_common(c, nullptr, n, W, H, sigma, pol, normalized, 0, out_f32, out_u8, minmax, nullptr, raw ? raw : &none);
}

int eorb_ev2im_raw(eorb_ctx* c, const eorb_raw_event* raw, size_t n, int W, int H, int pol, int normalized,
                   float* out_f32, uint8_t* out_u8, float* minmax, int* is_u8)
{
    if (c && n && !raw) return set_err(c, EORB_E_ARG, "ev2im_raw: bad arguments");
    static const eorb_raw_event none{};
    return ev_host_common(c, nullptr, n, W, H, 0.f, pol, normalized, 1, out_f32, out_u8, minmax, is_u8, raw ? raw : &none);
}

// ---- motion-compensated accumulation (f1) ----
static int mci_common(eorb_ctx* c, const eorb_event* ev, size_t n, const eorb_camera* cam, int se3, double angle, const double* axis,
                      const double* t, float medDepth, const float* depth, const float* params, int nparams, int W, int H,
                      float sigma, int pol, int normalized, float* out_f32, uint8_t* out_u8, float* minmax)
{
    if (!c) return EORB_E_ARG;
    if (W <= 0 || H <= 0 || (n && !ev) || !cam || !(sigma > 0.f)) return set_err(c, EORB_E_ARG, "ev2mci: bad arguments");
    fe_enter(c);
    const size_t npix = (size_t)W * H;
    if (n == 0) {                         // "no events" -> zero CV_32FC1 image (:292-295)
        if (out_f32) memset(out_f32, 0, sizeof(float) * npix);
        if (out_u8) memset(out_u8, 0, npix);
        if (minmax) { minmax[0] = 0.f; minmax[1] = -1000000.0f; }
        return EORB_OK;
    }
    if (n > 0x7fffffff) return set_err(c, EORB_E_CAPACITY, "ev2mci: too many events");
    if (cam->model != 0 && cam->model != 1) return set_err(c, EORB_E_ARG, "ev2mci: camera model %d unknown", cam->model);
    int rc;
    Arena A(c);
    const size_t o_ev = A.in_events(ev, n), o_depth = A.in(depth, depth ? sizeof(float) * n : 0);
    const size_t o_warp = A.reserve(sizeof(eorb_event16) * n);
    // outputs: min/max (encoded | decoded: the block is fetched whole) | u8 image (written when normalized) | f32 image
    const size_t o_mm = A.out(nullptr, 64), o_u8 = A.out(normalized ? out_u8 : nullptr, npix), o_f32 = A.out(out_f32, sizeof(float) * npix);
    A.want(o_mm, 64); A.inout(minmax, o_mm + 16, 8);
    if ((rc = A.upload())) return rc;
    const float* d_depth = depth ? A.dev<float>(o_depth) : nullptr;
    eorb_event16* d_warp = A.dev<eorb_event16>(o_warp);
    if (se3) rc = ev_warp_se3_dev(c, A.dev<eorb_event16>(o_ev), d_warp, (int)n, cam, angle, axis, t, medDepth, d_depth);
    else rc = ev_warp_se2_dev(c, A.dev<eorb_event16>(o_ev), d_warp, (int)n, cam, params, nparams);
    if (rc) return rc;
    int64_t offs[2] = {0, (int64_t)n};
    uint32_t* mm = A.dev<uint32_t>(o_mm);
    float* mmf = A.dev<float>(o_mm + 16);
    // (warped events: no two share a position -- the position table of the bulk float form would only be filled and thrown away)
    rc = ev_accumulate_dev(c, d_warp, 0, offs, 1, W, H, sigma, pol, 0, A.dev<float>(o_f32), A.dev<uint8_t>(o_u8), normalized, mm, false, true);
    if (rc) return rc;
    if ((rc = ev_decode_minmax(c, mm, mmf, 1))) return rc;
    return A.fetch();
}

static eorb_camera pinhole_cam(const eorb_pinhole* p) { eorb_camera c{}; if (p) { c.fx = p->fx; c.fy = p->fy; c.cx = p->cx; c.cy = p->cy; } return c; }

int eorb_ev2mci_se3_cam(eorb_ctx* c, const eorb_event* ev, size_t n, const eorb_camera* cam, double angle, const double axis[3],
                        const double t[3], float medDepth, const float* depth_per_event, int W, int H, float sigma, int pol,
                        int normalized, float* out_f32, uint8_t* out_u8, float* minmax)
{
    if (c && (!axis || !t)) return set_err(c, EORB_E_ARG, "ev2mci_se3: null pose");
    return mci_common(c, ev, n, cam, 1, angle, axis, t, medDepth, depth_per_event, nullptr, 0, W, H, sigma, pol, normalized, out_f32, out_u8, minmax);
}

int eorb_ev2mci_se2_cam(eorb_ctx* c, const eorb_event* ev, size_t n, const eorb_camera* cam, const float* params2D, int nparams,
                        int W, int H, float sigma, int pol, int normalized, float* out_f32, uint8_t* out_u8, float* minmax)
{
    if (c && (!params2D || nparams < 3)) return set_err(c, EORB_E_ARG, "ev2mci_se2: need at least 3 parameters");
    return mci_common(c, ev, n, cam, 0, 0.0, nullptr, nullptr, 0.f, nullptr, params2D, nparams, W, H, sigma, pol, normalized, out_f32, out_u8, minmax);
}

int eorb_ev2mci_se3(eorb_ctx* c, const eorb_event* ev, size_t n, const eorb_pinhole* cam, double angle, const double axis[3],
                    const double t[3], float medDepth, const float* depth_per_event, int W, int H, float sigma, int pol,
                    int normalized, float* out_f32, uint8_t* out_u8, float* minmax)
{
    const eorb_camera cc = pinhole_cam(cam);
    return eorb_ev2mci_se3_cam(c, ev, n, cam ? &cc : nullptr, angle, axis, t, medDepth, depth_per_event, W, H, sigma, pol, normalized, out_f32, out_u8, minmax);
}

int eorb_ev2mci_se2(eorb_ctx* c, const eorb_event* ev, size_t n, const eorb_pinhole* cam, const float* params2D, int nparams,
                    int W, int H, float sigma, int pol, int normalized, float* out_f32, uint8_t* out_u8, float* minmax)
{
    const eorb_camera cc = pinhole_cam(cam);
    return eorb_ev2mci_se2_cam(c, ev, n, cam ? &cc : nullptr, params2D, nparams, W, H, sigma, pol, normalized, out_f32, out_u8, minmax);
}

int eorb_measure_image_focus_n(eorb_ctx* c, const float* imgs, int n, int W, int H, float* focus)
{
    if (!c) return EORB_E_ARG;
    if (!imgs || !focus || W <= 0 || H <= 0 || n < 1 || n > 64) return set_err(c, EORB_E_ARG, "measure_image_focus: bad arguments");
    fe_enter(c);
    int rc;
    Arena A(c);
    const size_t o_img = A.in(imgs, sizeof(float) * (size_t)W * H * n), o_focus = A.out(focus, sizeof(float) * n);
    if ((rc = A.upload())) return rc;
    if ((rc = ev_focus_dev(c, A.dev<float>(o_img), n, W, H, A.dev<float>(o_focus)))) return rc;
    return A.fetch();
}
int eorb_measure_image_focus(eorb_ctx* c, const float* img, int W, int H, float* focus) { return eorb_measure_image_focus_n(c, img, 1, W, H, focus); }

int eorb_normalize_minmax_u8(eorb_ctx* c, const float* img, int W, int H, uint8_t* out)
{
    if (!c) return EORB_E_ARG;
    if (!img || !out || W <= 0 || H <= 0) return set_err(c, EORB_E_ARG, "normalize_minmax_u8: bad arguments");
    fe_enter(c);
    const size_t npix = (size_t)W * H;
    int rc;
    Arena A(c);
    const size_t o_img = A.in(img, sizeof(float) * npix), o_mm = A.reserve(64), o_u8 = A.out(out, npix);
    if ((rc = A.upload())) return rc;
    if ((rc = ev_cvnormalize_dev(c, A.dev<float>(o_img), (int)npix, A.dev<uint32_t>(o_mm), A.dev<uint8_t>(o_u8)))) return rc;
    return A.fetch();
}

// ---- marshalling shared by the extraction entry points (eorb_orb_extract, eorb_frame_mono / _stereo / _fisheye, eorb_ev_slice_extract
// and the tracked pair): check the image, queue it, reserve the result block, one download, copy out -----------------------------------
// what every entry checks of its image (a pair passes NULL when either image is missing).  need_calib: eorb_frame_mono
static int image_check(eorb_ctx* c, const char* who, const uint8_t* img, int W, int H, int stride, bool need_calib = false)
{
    if (!img || W <= 0 || H <= 0) return EORB_E_EMPTY;                 // _image.empty() -> -1 (:1096), trackedImage.empty() -> return (:1270, :1319)
    const OrbState& o = c->orb;
    if (!o.configured) return set_err(c, EORB_E_NOTCONF, "%s: eorb_orb_configure not called", who);
    if (need_calib && !c->calib_set) return set_err(c, EORB_E_NOTCONF, "%s: eorb_set_calibration not called", who);
    if (W != o.W || H != o.H) return set_err(c, EORB_E_ARG, "%s: image %dx%d does not match the configured %dx%d", who, W, H, o.W, o.H);
    if (stride < W) return set_err(c, EORB_E_ARG, "%s: stride %d < width %d", who, stride, W);
    return EORB_OK;
}

// the image -> arena, its rows packed.  allow_zero_copy (the one image of a call, up to 1 MiB): it is read once, by the pyramid's first
// kernel, which then reads the pinned staging buffer itself (Arena::in_ptr): no upload in front of the launch
static size_t image_in(Arena& A, const uint8_t* img, int W, int H, int stride, bool allow_zero_copy)
{
    if (allow_zero_copy) A.host_inputs = A.c->opt.image_zero_copy != 0 && (size_t)W * H <= ((size_t)1 << 20);
    return A.in2d(img, H, (size_t)W, (size_t)stride);
}

// the result block of an extraction of nimg images (one, or the two of a pair), contiguous:
//   head | keypoints [nimg] | undistorted keypoints (eorb_frame_mono) | descriptors [nimg] | oob (one image)
// every array holds max_out records per image; what a pair adds (matches, candidates) follows the block.  One head for all entries:
// device code is handed &head->n[i] and so on
struct ExtractHead {
    int32_t n[2], mono[2];      // keypoints and monoIndex of each image
    int32_t aux[2];             // [0]: eorb_frame_stereo's matches / eorb_frame_fisheye's candidates (fisheye_lowe_kernel reads n, mono, aux[0] as lap[0..4])
    int32_t flag[2];            // internal capacity exceeded, one per extraction launch
    float corners[8];           // eorb_frame_mono: the undistorted corners (0, 0), (W, 0), (0, H), (W, H)
};
// where a call's records go (one entry per image; any pointer may be NULL)
struct ExtractDst { eorb_keypoint* kps; uint8_t* desc; uint8_t* oob; int* n; int* mono; };
struct ExtractOff { size_t head, kp, un, desc, oob, mo, ncopy; int nimg; };      // ncopy: the records a caller of this capacity can be handed
// The number of records is known only after the download, so nothing is registered for copying: the fetched span covers the head and, of
// every array the caller takes, the first ncopy records; extract_out copies n of them after its checks
static ExtractOff extract_reserve(Arena& A, int max_out, int nimg, int cap, const ExtractDst* dst, bool undist = false)
{
    ExtractOff x{};
    x.mo = (size_t)max_out; x.nimg = nimg; x.ncopy = std::min(x.mo, (size_t)std::max(cap, 0));
    x.head = A.out(nullptr, sizeof(ExtractHead));
    x.kp = A.out(nullptr, sizeof(eorb_keypoint) * x.mo * nimg);
    if (undist) x.un = A.out(nullptr, sizeof(eorb_keypoint) * x.mo);
    x.desc = A.out(nullptr, 32 * x.mo * nimg);
    if (nimg == 1) x.oob = A.out(nullptr, x.mo);
    A.want(x.head, sizeof(ExtractHead));
    for (int i = 0; i < nimg; i++) {
        if (dst[i].kps) A.want(x.kp + sizeof(eorb_keypoint) * x.mo * i, sizeof(eorb_keypoint) * x.ncopy);
        if (dst[i].desc) A.want(x.desc + 32 * x.mo * i, 32 * x.ncopy);
        if (dst[i].oob) A.want(x.oob, x.ncopy);
    }
    return x;
}
// after the fetch (h: its host view): a set flag (nflag: extraction launches of the call) and a count above cap are
// EORB_E_CAPACITY and nothing is written; else every image's n records and its counters go to the caller
static int extract_out(eorb_ctx* c, const char* who, const char* h, const ExtractOff& x, int cap, int nflag, const ExtractDst* dst, const ExtractHead** head = nullptr)
{
    const ExtractHead& hd = *(const ExtractHead*)(h + x.head);
    if (head) *head = &hd;
    // (reported here; the sticky word of the *_dev calls is not involved)
    if (nflag == 1 && hd.flag[0]) return set_err(c, EORB_E_CAPACITY, "%s: internal capacity exceeded (flag %d)", who, hd.flag[0]);
    if (nflag == 2 && (hd.flag[0] || hd.flag[1])) return set_err(c, EORB_E_CAPACITY, "%s: internal capacity exceeded (flags %d, %d)", who, hd.flag[0], hd.flag[1]);
    if (x.nimg == 1 && hd.n[0] > cap) return set_err(c, EORB_E_CAPACITY, "%s: %d keypoints > caller capacity %d", who, hd.n[0], cap);
    if (x.nimg == 2 && (hd.n[0] > cap || hd.n[1] > cap)) return set_err(c, EORB_E_CAPACITY, "%s: %d / %d keypoints > caller capacity %d", who, hd.n[0], hd.n[1], cap);
    for (int i = 0; i < x.nimg; i++) {
        const ExtractDst& d = dst[i];
        const size_t n = (size_t)std::max(hd.n[i], 0);
        if (d.kps && n) memcpy(d.kps, h + x.kp + sizeof(eorb_keypoint) * x.mo * i, sizeof(eorb_keypoint) * n);
        if (d.desc && n) memcpy(d.desc, h + x.desc + 32 * x.mo * i, 32 * n);
        if (d.oob && n) memcpy(d.oob, h + x.oob, n);
        if (d.n) *d.n = hd.n[i];
        if (d.mono) *d.mono = hd.mono[i];
    }
    return EORB_OK;
}

// ---- the L1 image builder's per-chunk path, one call per chunk (src/Event/EvImBuilder.cpp:1300-1515) ----------------------------
// resolveMinMaxVals' start values (min 0, max -1e6: src/Event/EventConversion.cc:224-225) in the order-preserving encoding of the
// gather kernels' atomics (enc_f32), uploaded with a call's events instead of being written by a kernel
static const uint32_t kMinMaxPreset[16] = {0x80000000u, 0x368bdbffu, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// events of a chunk -> arena; float EventData are packed to the 16-byte record on the host, raw sensor events go as they are
static int slice_events_in(eorb_ctx* c, Arena& A, const eorb_event* ev, const eorb_raw_event* raw, size_t n, std::vector<eorb_event16>& packed,
                           size_t* o_ev, int* is_raw, const char* who)
{
    if (n && !ev && !raw) return set_err(c, EORB_E_ARG, "%s: no events", who);
    if (ev && raw) return set_err(c, EORB_E_ARG, "%s: float events OR raw sensor events", who);
    *is_raw = raw != nullptr;
    if (raw) {
        if (!c->maps.w) return set_err(c, EORB_E_NOTCONF, "%s: raw events need eorb_set_undistort_maps first", who);
        for (size_t i = 0; i < n; i++)
            if ((int)raw[i].x >= c->maps.w || (int)raw[i].y >= c->maps.h)       // the reference asserts (MyCalibrator.cpp:176)
                return set_err(c, EORB_E_ARG, "%s: event %zu at (%u,%u) lies outside the %dx%d maps", who, i, raw[i].x, raw[i].y, c->maps.w, c->maps.h);
        *o_ev = A.in(raw, sizeof(eorb_raw_event) * n);
    } else {
        packed.resize(n);
        if (n) eorb_pack_events(ev, n, packed.data());
        *o_ev = A.in(packed.data(), sizeof(eorb_event16) * n);
    }
    return EORB_OK;
}

int eorb_ev_slice_extract(eorb_ctx* c, const eorb_event* ev, const eorb_raw_event* raw, size_t n, float sigma, int lap0, int lap1,
                          int want_desc, eorb_keypoint* kps, uint8_t* desc, uint8_t* oob, int cap, int* n_out, int* mono_index,
                          uint8_t* out_u8)
{
    if (!c) return EORB_E_ARG;
    if (n_out) *n_out = 0;
    OrbState& o = c->orb;
    if (!o.configured) return set_err(c, EORB_E_NOTCONF, "ev_slice_extract: eorb_orb_configure not called");
    if (!(sigma > 0.f)) return set_err(c, EORB_E_ARG, "ev_slice_extract: sigma must be > 0");
    fe_enter(c);
    const int W = o.W, H = o.H;
    const size_t npix = (size_t)W * H;
    int rc, is_raw = 0;
    Arena A(c);
    std::vector<eorb_event16> packed;
    size_t o_ev = 0;
    if ((rc = slice_events_in(c, A, ev, raw, n, packed, &o_ev, &is_raw, "ev_slice_extract"))) return rc;
    // the running extremes travel initialised with the events (no launch for them); device-only: float image; outputs, contiguous:
    // u8 image | the extraction's result block
    // a live slice (the binning-free form reads every event once, in ev_pre_kernel): the events stay in pinned host memory and the
    // extremes are initialised by that kernel -- no copy in front of the first launch
    const bool zc = c->opt.slice_zero_copy != 0 && plan_host_events(accum_shape(W, H, sigma, 0, 1, (int64_t)n), AccumRequest{is_raw, 0, 0, 1}, accum_knobs(c));
    A.host_inputs = zc;
    const size_t o_mm = zc ? A.reserve(sizeof(kMinMaxPreset)) : A.in(kMinMaxPreset, sizeof(kMinMaxPreset)), o_f32 = A.reserve(sizeof(float) * npix);
    const size_t o_u8 = A.out(nullptr, npix);
    if (out_u8) A.want(o_u8, npix);                       // (copied below, unless the extraction's flag is set)
    const ExtractDst dst{kps, want_desc ? desc : nullptr, oob, n_out, mono_index};
    const ExtractOff X = extract_reserve(A, o.max_out, 1, cap, &dst);
    if ((rc = A.upload())) return rc;
    int64_t offs[2] = {0, (int64_t)n};
    uint8_t* d_u8 = A.dev<uint8_t>(o_u8);
    ExtractHead* hd = A.dev<ExtractHead>(X.head);
    // EvImConverter::ev2im_gauss(l1Evs, W, H, sigma) :1345 (pol = false, normalized = true)
    // (the normalisation to u8 is left to the extraction's first kernel: one launch less)
    if ((rc = ev_accumulate_dev(c, A.in_ptr<void>(o_ev), is_raw, offs, 1, W, H, sigma, 0, 0, A.dev<float>(o_f32), d_u8, 0, A.dev<uint32_t>(o_mm), !zc))) return rc;
    A.inputs_done();
    // makeFrame :1348 -> EvFrame ctor -> ORBextractor::operator() (EventFrame.cpp:220)
    if ((rc = orb_extract_dev(c, d_u8, W, npix, 1, lap0, lap1, want_desc, A.dev<eorb_keypoint>(X.kp), A.dev<uint8_t>(X.desc), A.dev<uint8_t>(X.oob),
                              hd->n, hd->mono, hd->flag, A.dev<float>(o_f32), A.dev<uint32_t>(o_mm)))) return rc;
    if ((rc = ensure(c, c->l1_ref_img, npix)) || (rc = ensure(c, c->l1_ref_pts, sizeof(float) * 2 * X.mo))) return rc;
    c->l1_nref = -1; c->l1_W = W; c->l1_H = H; c->klt_ref_serial++;
    c->l1_img_off = o_u8; c->l1_img_gen = c->arena_gen;
    const char* h;
    if ((rc = A.fetch_begin())) return rc;
    // ELK_Tracker::setRefImage(image, keypoints) (:1363 init -> KLT_Tracker.cpp:22-46): the image and its points stay on the device --
    // queued behind the download, which does not wait for them (the next call on the stream is ordered behind them)
    EORB_HIP(c, hipMemcpyAsync(c->l1_ref_img.p, d_u8, npix, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = ev_kp_points_dev(c, A.dev<eorb_keypoint>(X.kp), hd->n, (int)X.mo, (float*)c->l1_ref_pts.p))) return rc;
    if ((rc = A.fetch_wait(&h))) return rc;
    const ExtractHead& got = *(const ExtractHead*)(h + X.head);
    if (!got.flag[0]) {                                   // the reference frame and the image stand whatever the caller's capacity is
        c->l1_nref = got.n[0];
        if (out_u8) memcpy(out_u8, h + o_u8, npix);
    }
    return extract_out(c, "ev_slice_extract", h, X, cap, 1, &dst);
}

int eorb_ev_slice_track(eorb_ctx* c, const eorb_event* ev, const eorb_raw_event* raw, size_t n, float sigma, const eorb_klt_params* klt,
                        float* pts, uint8_t* status, float* err, int nref, uint8_t* out_u8)
{
    if (!c) return EORB_E_ARG;
    if (!klt || !(sigma > 0.f) || nref < 0 || (nref && (!pts || !status || !err))) return set_err(c, EORB_E_ARG, "ev_slice_track: bad arguments");
    if (klt->win < 3 || klt->win > 63 || klt->maxLevel < 0) return set_err(c, EORB_E_ARG, "ev_slice_track: bad LK parameters");
    if (c->l1_nref < 0) return set_err(c, EORB_E_NOTCONF, "ev_slice_track: no reference frame (eorb_ev_slice_extract sets it)");
    if (nref != c->l1_nref) return set_err(c, EORB_E_ARG, "ev_slice_track: %d points, the reference frame has %d", nref, c->l1_nref);
    fe_enter(c);
    const int W = c->l1_W, H = c->l1_H;
    const size_t npix = (size_t)W * H;
    int rc, is_raw = 0;
    Arena A(c);
    std::vector<eorb_event16> packed;
    size_t o_ev = 0;
    if ((rc = slice_events_in(c, A, ev, raw, n, packed, &o_ev, &is_raw, "ev_slice_track"))) return rc;
    // in: the running extremes, initialised; in / out: the points (initial flow in, tracked points out); outputs behind them:
    // status | err | u8 image; then device-only
    const size_t o_mm = A.in(kMinMaxPreset, sizeof(kMinMaxPreset));
    const size_t o_pts = A.in(pts, sizeof(float) * 2 * (size_t)nref);
    A.inout(pts, o_pts, sizeof(float) * 2 * (size_t)nref);
    const size_t o_st = A.out(nullptr, (size_t)nref + 16), o_err = A.out(err, sizeof(float) * (size_t)nref), o_u8 = A.out(out_u8, npix);
    A.inout(status, o_st, (size_t)nref);
    const size_t o_f32 = A.reserve(sizeof(float) * npix);
    if ((rc = A.upload())) return rc;
    int64_t offs[2] = {0, (int64_t)n};
    uint8_t* d_u8 = A.dev<uint8_t>(o_u8);
    if ((rc = ev_accumulate_dev(c, A.dev<void>(o_ev), is_raw, offs, 1, W, H, sigma, 0, 0, A.dev<float>(o_f32), d_u8, 1, A.dev<uint32_t>(o_mm), true))) return rc;
    c->l1_img_off = o_u8; c->l1_img_gen = c->arena_gen;
    // ELK_Tracker::trackCurrImage (KLT_Tracker.cpp:49-74): calcOpticalFlowPyrLK(mRefFrame, currImage, mRefPoints, kpts, ..., OPTFLOW_USE_INITIAL_FLOW)
    if (nref && (rc = klt_track_dev(c, (const uint8_t*)c->l1_ref_img.p, d_u8, W, H, W, (const float*)c->l1_ref_pts.p, A.dev<float>(o_pts), nref, klt->win,
                                    klt->maxLevel, klt->maxCount, klt->epsilon, 4 /* OPTFLOW_USE_INITIAL_FLOW */, klt->minEigThreshold,
                                    A.dev<uint8_t>(o_st), A.dev<float>(o_err), c->klt_ref_serial))) return rc;
    return A.fetch();
}

int eorb_ev_slice_image(eorb_ctx* c, uint8_t* out_u8)
{
    if (!c || !out_u8) return EORB_E_ARG;
    if (c->l1_img_gen != c->arena_gen || !c->arena.p || !c->l1_W) return set_err(c, EORB_E_NOTCONF, "ev_slice_image: the image of the last slice call is gone");
    fe_enter(c);
    EORB_HIP(c, hipMemcpyAsync(out_u8, (const char*)c->arena.p + c->l1_img_off, (size_t)c->l1_W * c->l1_H, hipMemcpyDeviceToHost, c->stream));
    EORB_HIP(c, fe_stream_sync(c));
    return EORB_OK;
}

int eorb_ev_mc_contest(eorb_ctx* c, const eorb_event* ev, size_t n, const eorb_camera* cam, const eorb_se3_motion* dp, const eorb_se3_motion* ba,
                       const float* se2_params, int nparams, int W, int H, float sigma, float focus[5], int* winner, uint8_t* out_u8,
                       eorb_ctx* l2, int lap0, int lap1, eorb_keypoint* kps, int cap, int* n_out)
{
    if (!c) return EORB_E_ARG;
    if (winner) *winner = -1;
    if (n_out) *n_out = 0;
    if (W <= 0 || H <= 0 || (n && !ev) || !(sigma > 0.f) || !focus || !winner) return set_err(c, EORB_E_ARG, "ev_mc_contest: bad arguments");
    if ((dp || ba || se2_params) && !cam) return set_err(c, EORB_E_ARG, "ev_mc_contest: the motion-compensated methods need the camera");
    if (cam && cam->model != 0 && cam->model != 1) return set_err(c, EORB_E_ARG, "ev_mc_contest: camera model %d unknown", cam->model);
    if (se2_params && nparams < 3) return set_err(c, EORB_E_ARG, "ev_mc_contest: need at least 3 SE2 parameters");
    for (int k = 0; k < 5; k++) focus[k] = -1.f;
    if (n == 0) return EORB_OK;                          // "Empty ev buffer, abort" (:1149-1152)
    if (n > 0x3fffffff) return set_err(c, EORB_E_CAPACITY, "ev_mc_contest: too many events");
    if (l2) {
        if (l2->device != c->device) return set_err(c, EORB_E_ARG, "ev_mc_contest: the L2 context sits on another device");
        if (!l2->orb.configured || l2->orb.W != W || l2->orb.H != H) return set_err(c, EORB_E_NOTCONF, "ev_mc_contest: the L2 context's extractor is not configured for %dx%d", W, H);
    }
    fe_enter(c);
    const size_t npix = (size_t)W * H;
    int rc;
    // methods in the reference's insertion order (:1207-1211): 0 "DP", 1 "BA", 2 "EH", 3 "Opt"; image 4 = the event histogram of the
    // later half of the window (:1214-1216), built alongside so that the call waits once
    const eorb_se3_motion* se3[2] = {dp, ba};
    int img_of[4] = {-1, -1, -1, -1}, nimg = 0;
    for (int m = 0; m < 4; m++) if (m == 2 || (m < 2 && se3[m]) || (m == 3 && se2_params)) img_of[m] = nimg++;
    const int half_img = nimg++;
    const size_t nh = n / 2;                             // prefSize = evs.size() / 2: the window's last nh events (:1062-1066); 0 -> the whole window
    std::vector<eorb_event16> packed(n);
    eorb_pack_events(ev, n, packed.data());
    Arena A(c);
    const size_t o_ev = A.in(packed.data(), sizeof(eorb_event16) * n);
    const size_t o_warp = A.reserve(sizeof(eorb_event16) * n * 3);
    const size_t o_mm = A.reserve(256), o_f32 = A.reserve(sizeof(float) * npix * (size_t)nimg), o_u8s = A.reserve(npix * (size_t)nimg);
    const size_t o_fimg = A.reserve(64);
    const size_t mo = l2 ? (size_t)l2->orb.max_out : 0;
    // outputs: focus[5] + winner | the winner's u8 image | {n, mono, flag} | keypoints (the L2 extraction's: n of them, copied after its checks)
    const size_t ncopy = l2 ? std::min<size_t>(mo, (size_t)std::max(cap, 0)) : 0;
    const size_t o_res = A.out(nullptr, 64), o_win = A.out(out_u8, npix), o_n = A.out(nullptr, 16), o_kp = A.out(nullptr, sizeof(eorb_keypoint) * std::max<size_t>(mo, 1));
    A.want(o_res, 64);
    if (l2) { A.want(o_n, 16); if (kps) A.want(o_kp, sizeof(eorb_keypoint) * ncopy); }
    if ((rc = A.upload())) return rc;
    const eorb_event16* d_ev = A.dev<eorb_event16>(o_ev);
    eorb_event16* d_warp = A.dev<eorb_event16>(o_warp);
    const int64_t wbase = (int64_t)((o_warp - o_ev) / sizeof(eorb_event16));      // (arena offsets are multiples of 256)
    int64_t beg[8], end[8];
    int nw = 0;
    for (int m = 0; m < 4; m++) {
        if (img_of[m] < 0) continue;
        const int j = img_of[m];
        if (m == 2) { beg[j] = 0; end[j] = (int64_t)n; continue; }                // getEvHist :1060-1079
        eorb_event16* dst = d_warp + (size_t)nw * n;
        if (m < 2) rc = ev_warp_se3_dev(c, d_ev, dst, (int)n, cam, se3[m]->angle, se3[m]->axis, se3[m]->t, se3[m]->medDepth, nullptr);       // getDPoseMCI :969 / getBAMCI :1043
        else rc = ev_warp_se2_dev(c, d_ev, dst, (int)n, cam, se2_params, nparams);                                                           // getAff2DMCI :1133
        if (rc) return rc;
        beg[j] = wbase + (int64_t)nw * (int64_t)n; end[j] = beg[j] + (int64_t)n;
        nw++;
    }
    beg[half_img] = nh ? (int64_t)(n - nh) : 0; end[half_img] = (int64_t)n;
    float* d_f32 = A.dev<float>(o_f32);
    uint32_t* d_mm = A.dev<uint32_t>(o_mm);
    if ((long)n <= (long)c->opt.contest_direct_max) {
        // every reconstruction of the window in ONE launch of the binning-free kernel (float events, normalized = false).  (Beyond
        // the single-slice limit of 16 384 events too: five binned passes of 60 us each are what the alternative costs here.)
        if ((rc = ev_direct_slices_dev(c, accum_shape(W, H, sigma, 0, nimg, (int64_t)n), d_ev, 0, beg, end, nimg, W, H, sigma, 0, d_f32, nullptr, 0, d_mm))) return rc;
    } else {
        for (int j = 0; j < nimg; j++) {                                // (warped events: no two share a position)
            int64_t offs[2] = {0, end[j] - beg[j]};
            if ((rc = ev_accumulate_dev(c, d_ev + beg[j], 0, offs, 1, W, H, sigma, 0, 0, d_f32 + (size_t)j * npix, nullptr, 0, d_mm + 2 * j, false, true))) return rc;
        }
    }
    // measureImageFocus of every image, then cv::normalize(img, img, 255, 0, NORM_MINMAX, CV_8UC1) of every image (:972-976, :1052-1055, :1073-1076, :1137-1140)
    if ((rc = ev_focus_dev(c, d_f32, nimg, W, H, A.dev<float>(o_fimg)))) return rc;
    if ((rc = ev_cvnormalize_n_dev(c, d_f32, nimg, (int)npix, d_mm + 32, A.dev<uint8_t>(o_u8s)))) return rc;
    float* d_res = A.dev<float>(o_res);
    if ((rc = ev_contest_select_dev(c, A.dev<float>(o_fimg), img_of, half_img, A.dev<uint8_t>(o_u8s), (int)npix, d_res, (int*)(d_res + 8), A.dev<uint8_t>(o_win)))) return rc;
    int32_t* dn = A.dev<int32_t>(o_n);
    if (l2) {
        // isMcImageGood (:260-267): the L2 tracker's makeFrame on the winner = its detect-only extraction.  The L2 context's kernels run on
        // THIS context's stream for the call (both contexts belong to the calling thread), so the call still waits once.
        if (l2 != c) EORB_HIP(c, hipStreamSynchronize(l2->stream));
        hipStream_t saved = l2->stream; l2->stream = c->stream;
        rc = orb_extract_dev(l2, A.dev<uint8_t>(o_win), W, npix, 1, lap0, lap1, 0, A.dev<eorb_keypoint>(o_kp), nullptr, nullptr, dn, dn + 1, dn + 2);
        l2->stream = saved;
        if (rc) { if (l2 != c) c->err = l2->err; return rc; }
    }
    const char* h;
    if ((rc = A.fetch(&h))) return rc;
    memcpy(focus, h + o_res, sizeof(float) * 5);
    int32_t w; memcpy(&w, h + o_res + 32, 4);
    *winner = w;
    if (l2) {
        const int32_t* hn = (const int32_t*)(h + o_n);
        if (hn[2]) return set_err(c, EORB_E_CAPACITY, "ev_mc_contest: the L2 extraction exceeded an internal capacity (flag %d)", hn[2]);
        if (hn[0] > cap) return set_err(c, EORB_E_CAPACITY, "ev_mc_contest: %d keypoints > caller capacity %d", hn[0], cap);
        if (hn[0] > 0 && kps) memcpy(kps, h + o_kp, sizeof(eorb_keypoint) * (size_t)hn[0]);
        if (n_out) *n_out = hn[0];
    }
    return EORB_OK;
}

int eorb_selfcheck_division(eorb_ctx* c, float lo, float hi, float sigma, uint64_t* mismatches)
{
    if (!c || !mismatches || !(lo > 0.f) || !(hi >= lo) || !(sigma > 0.f)) return c ? set_err(c, EORB_E_ARG, "selfcheck_division: bad arguments") : EORB_E_ARG;
    fe_enter(c);
    unsigned long long bad = 0;
    int rc = ev_divcheck(c, lo, hi, sigma, &bad);
    *mismatches = bad;
    return rc;
}

int eorb_selfcheck_math(eorb_ctx* c, int which, uint32_t lo_bits, uint32_t hi_bits, uint64_t* hash)
{
    if (!c || !hash || which < 0 || which > 6 || hi_bits < lo_bits) return c ? set_err(c, EORB_E_ARG, "selfcheck_math: bad arguments") : EORB_E_ARG;
    fe_enter(c);
    unsigned long long h = 0;
    int rc = ev_mathhash(c, which, lo_bits, hi_bits, &h);
    *hash = h;
    return rc;
}

#ifdef EORB_DIAG
int eorb_diag_read(unsigned long long* out16) { return ev_diag_read(out16); }
int eorb_trace_read(unsigned long long* out, int n) { return ev_trace_read(out, n); }
#endif

#ifdef EORB_SLOT_TRACE
int eorb_slot_trace_read(eorb_ctx* c, unsigned long long* out, long long max_records) { return c ? ev_slots_trace_read(c, out, max_records) : -1; }
#endif

// ---- ORB extractor, host buffers -----------------------------------------------------------------------
int eorb_orb_configure(eorb_ctx* c, const eorb_orb_params* p, int W, int H)
{
    if (!c) return EORB_E_ARG;
    fe_enter(c);
    hipStreamSynchronize(c->stream);
    return orb_configure(c, p, W, H);
}

int eorb_orb_max_keypoints(eorb_ctx* c) { return (c && c->orb.configured) ? c->orb.max_out : EORB_E_NOTCONF; }

int eorb_orb_get_tables(eorb_ctx* c, float* sf, float* inv_sf, int* nfeat, int* edge)
{
    if (!c || !c->orb.configured) return EORB_E_NOTCONF;
    for (int i = 0; i < c->orb.nlevels; i++) {
        if (sf) sf[i] = c->orb.sf[i];
        if (inv_sf) inv_sf[i] = c->orb.inv_sf[i];
        if (nfeat) nfeat[i] = c->orb.nfeat[i];
    }
    if (edge) *edge = c->orb.edge;
    return EORB_OK;
}

int eorb_orb_extract(eorb_ctx* c, const uint8_t* img, int W, int H, int stride, int lap0, int lap1,
                     int want_desc, eorb_keypoint* kps, uint8_t* desc, uint8_t* oob, int cap,
                     int* n_out, int* mono_index)
{
    if (!c) return EORB_E_ARG;
    if (n_out) *n_out = 0;
    int rc;
    if ((rc = image_check(c, "orb_extract", img, W, H, stride))) return rc;
    fe_enter(c);
    Arena A(c);
    const size_t o_img = image_in(A, img, W, H, stride, true);
    const ExtractDst dst{kps, want_desc ? desc : nullptr, oob, n_out, mono_index};
    const ExtractOff X = extract_reserve(A, c->orb.max_out, 1, cap, &dst);
    if ((rc = A.upload())) return rc;
    ExtractHead* hd = A.dev<ExtractHead>(X.head);
    rc = orb_extract_dev(c, A.in_ptr<uint8_t>(o_img), W, (size_t)W * H, 1, lap0, lap1, want_desc, A.dev<eorb_keypoint>(X.kp),
                         A.dev<uint8_t>(X.desc), A.dev<uint8_t>(X.oob), hd->n, hd->mono, hd->flag);
    A.inputs_done();
    if (rc) return rc;
    const char* h;
    if ((rc = A.fetch(&h))) return rc;
    return extract_out(c, "orb_extract", h, X, cap, 1, &dst);
}

// Frame::Frame(imGray, ...) (src/Frame.cc:229-266): eorb_orb_extract with undistKeyPoints (:246-252) and ComputeImageBounds (:840-867)
// behind the extraction on the device -- the keypoints do not cross the link in between
int eorb_frame_mono(eorb_ctx* c, const uint8_t* img, int W, int H, int stride, int lap0, int lap1, int want_desc,
                    eorb_keypoint* kps, eorb_keypoint* kps_un, uint8_t* desc, uint8_t* oob, int cap,
                    int* n_out, int* mono_index, float bounds[4])
{
    if (!c) return EORB_E_ARG;
    if (n_out) *n_out = 0;
    int rc;
    if ((rc = image_check(c, "eorb_frame_mono", img, W, H, stride, true))) return rc;
    fe_enter(c);
    Arena A(c);
    const size_t o_img = image_in(A, img, W, H, stride, true);
    const bool gate = c->calib_dev.gate != 0;
    const ExtractDst dst{kps, want_desc ? desc : nullptr, oob, n_out, mono_index};
    const ExtractOff X = extract_reserve(A, c->orb.max_out, 1, cap, &dst, true);
    if (kps_un) A.want(gate ? X.un : X.kp, sizeof(eorb_keypoint) * X.ncopy);      // gate closed: vUndistKPts = vDistKPts
    if ((rc = A.upload())) return rc;
    ExtractHead* hd = A.dev<ExtractHead>(X.head);
    rc = orb_extract_dev(c, A.in_ptr<uint8_t>(o_img), W, (size_t)W * H, 1, lap0, lap1, want_desc, A.dev<eorb_keypoint>(X.kp),
                         A.dev<uint8_t>(X.desc), A.dev<uint8_t>(X.oob), hd->n, hd->mono, hd->flag);
    A.inputs_done();
    if (rc) return rc;
    if ((rc = calib_frame_dev(c, A.dev<eorb_keypoint>(X.kp), hd->n, (int)X.mo, A.dev<eorb_keypoint>(X.un), hd->corners, W, H))) return rc;
    const char* h;
    if ((rc = A.fetch(&h))) return rc;
    const ExtractHead* got;
    if ((rc = extract_out(c, "eorb_frame_mono", h, X, cap, 1, &dst, &got))) return rc;
    if (kps_un && got->n[0] > 0) memcpy(kps_un, h + (gate ? X.un : X.kp), sizeof(eorb_keypoint) * (size_t)got->n[0]);      // gate closed: vUndistKPts = vDistKPts
    if (bounds) {
        if (c->calib_bounds.gate) {                           // Frame.cc:855-858: std::min(a, b) = b < a ? b : a, std::max(a, b) = a < b ? b : a
            const float* q = got->corners;
            bounds[0] = (q[4] < q[0]) ? q[4] : q[0];
            bounds[1] = (q[2] < q[6]) ? q[6] : q[2];
            bounds[2] = (q[3] < q[1]) ? q[3] : q[1];
            bounds[3] = (q[5] < q[7]) ? q[7] : q[5];
        } else { bounds[0] = 0.0f; bounds[1] = (float)W; bounds[2] = 0.0f; bounds[3] = (float)H; }
    }
    return EORB_OK;
}

// Frame::Frame(imLeft, imRight, ...) (src/Frame.cc:97-152): both images through the extractor (two slices of one batch: the
// reference's two extractors have equal parameters, :122-125 with vLappingArea {0, 0}), then ComputeStereoMatches (:869-1048)
int eorb_frame_stereo(eorb_ctx* c, const uint8_t* imLeft, const uint8_t* imRight, int W, int H, int stride, float mb, float mbf,
                      eorb_keypoint* kpsL, uint8_t* descL, int* nL, eorb_keypoint* kpsR, uint8_t* descR, int* nR, int cap,
                      float* uRight, float* depth, int* nmatches)
{
    if (!c) return EORB_E_ARG;
    if (nL) *nL = 0; if (nR) *nR = 0; if (nmatches) *nmatches = 0;
    int rc;
    if ((rc = image_check(c, "eorb_frame_stereo", imLeft && imRight ? imLeft : nullptr, W, H, stride))) return rc;
    if (!(mb > 0.f) || !(mbf > 0.f)) return set_err(c, EORB_E_ARG, "eorb_frame_stereo: baseline %.4f, bf %.4f", mb, mbf);
    fe_enter(c);
    Arena A(c);
    const size_t o_imL = image_in(A, imLeft, W, H, stride, false), o_imR = image_in(A, imRight, W, H, stride, false);
    // outputs: the result block of the pair | uRight | depth (n[0] of each, copied after the checks) | (norms)
    const ExtractDst dst[2] = {{kpsL, descL, nullptr, nL, nullptr}, {kpsR, descR, nullptr, nR, nullptr}};
    const ExtractOff X = extract_reserve(A, c->orb.max_out, 2, cap, dst);
    const size_t o_ur = A.out(nullptr, sizeof(float) * X.mo), o_dp = A.out(nullptr, sizeof(float) * X.mo), o_sad = A.reserve(sizeof(int32_t) * X.mo);
    if (uRight) A.want(o_ur, sizeof(float) * X.ncopy);
    if (depth) A.want(o_dp, sizeof(float) * X.ncopy);
    if ((rc = A.upload())) return rc;
    ExtractHead* hd = A.dev<ExtractHead>(X.head);
    rc = orb_extract_dev(c, A.dev<uint8_t>(o_imL), W, o_imR - o_imL, 2, 0, 0, 1, A.dev<eorb_keypoint>(X.kp), A.dev<uint8_t>(X.desc), nullptr, hd->n, hd->mono, hd->flag);
    if (rc) return rc;
    if ((rc = stereo_match_dev(c, A.dev<eorb_keypoint>(X.kp), A.dev<uint8_t>(X.desc), hd->n, mb, mbf, A.dev<float>(o_ur), A.dev<float>(o_dp),
                               A.dev<int32_t>(o_sad), hd->aux))) return rc;
    const char* h;
    if ((rc = A.fetch(&h))) return rc;
    const ExtractHead* got;
    if ((rc = extract_out(c, "eorb_frame_stereo", h, X, cap, 1, dst, &got))) return rc;      // (one launch for both images: one flag)
    if (uRight && got->n[0] > 0) memcpy(uRight, h + o_ur, sizeof(float) * (size_t)got->n[0]);
    if (depth && got->n[0] > 0) memcpy(depth, h + o_dp, sizeof(float) * (size_t)got->n[0]);
    if (nmatches) *nmatches = got->aux[0];
    return EORB_OK;
}

static int tracked_common(eorb_ctx* c, const uint8_t* img, int W, int H, int stride, eorb_keypoint* kps_io, const eorb_keypoint* kps_in,
                          int n, int mode, const uint8_t* ref, uint8_t* desc, uint8_t* oob)
{
    if (!c) return EORB_E_ARG;
    int rc;
    if ((rc = image_check(c, "tracked descriptors", img, W, H, stride))) return rc;
    if (n < 0) return set_err(c, EORB_E_ARG, "tracked descriptors: %d keypoints", n);
    if (n == 0) return EORB_OK;
    fe_enter(c);
    Arena A(c);
    const size_t o_img = image_in(A, img, W, H, stride, false), o_ref = A.in(ref, ref ? 32 * (size_t)n : 0);
    // keypoints (in / out: mode 1 writes their octaves and takes them, kps_io) | outputs of mode 0 (desc, oob): descriptors | oob
    const size_t o_kp = A.in(kps_in, sizeof(eorb_keypoint) * (size_t)n);
    A.inout(kps_io, o_kp, sizeof(eorb_keypoint) * (size_t)n);
    const size_t o_desc = A.out(desc, 32 * (size_t)n), o_oob = A.out(oob, (size_t)n);
    if ((rc = A.upload())) return rc;
    if ((rc = orb_pyramid_blur_dev(c, A.dev<uint8_t>(o_img), W))) return rc;
    if ((rc = orb_tracked_dev(c, A.dev<eorb_keypoint>(o_kp), n, mode, A.dev<uint8_t>(o_ref), A.dev<uint8_t>(o_desc), A.dev<uint8_t>(o_oob)))) return rc;
    return A.fetch();
}

int eorb_orb_tracked_descriptors(eorb_ctx* c, const uint8_t* img, int W, int H, int stride, const eorb_keypoint* kps, int n,
                                 uint8_t* desc, uint8_t* oob)
{
    if (c && (!kps || !desc) && n > 0) return set_err(c, EORB_E_ARG, "tracked descriptors: null buffers");
    return tracked_common(c, img, W, H, stride, nullptr, kps, n, 0, nullptr, desc, oob);
}

int eorb_orb_assign_level_by_best_desc(eorb_ctx* c, const uint8_t* img, int W, int H, int stride, const uint8_t* ref_desc,
                                       eorb_keypoint* kps, int n)
{
    if (c && (!kps || !ref_desc) && n > 0) return set_err(c, EORB_E_ARG, "assign level: null buffers");
    return tracked_common(c, img, W, H, stride, kps, kps, n, 1, ref_desc, nullptr, nullptr);
}

// ---- matchers, host buffers ------------------------------------------------------------------------------
int eorb_search_for_initialization(eorb_ctx* c,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, int stride1, const uint8_t* is_orb1,
        const eorb_keypoint* kps2, int n2, const uint8_t* desc2, int stride2, const uint8_t* is_orb2,
        const eorb_grid_bounds* gb, float* prev_matched, int32_t* matches12,
        int windowSize, float nnratio, int checkOri, int* nmatches)
{
    if (!c) return EORB_E_ARG;
    if (n1 < 0 || n2 < 0 || !gb || !matches12 || stride1 < 32 || stride2 < 32) return set_err(c, EORB_E_ARG, "search_for_initialization: bad arguments");
    fe_enter(c);
    if (nmatches) *nmatches = 0;
    if (n1 == 0) return EORB_OK;
    int rc;
    const int c1 = std::max(n1, 1), c2 = std::max(n2, 1);
    Arena A(c);
    int32_t hn[2] = {n1, n2};
    const size_t o_n = A.in(hn, 8);
    const size_t o_k1 = A.in(kps1, sizeof(eorb_keypoint) * (size_t)n1), o_d1 = A.in(desc1, (size_t)stride1 * n1);
    const size_t o_k2 = A.in(kps2, sizeof(eorb_keypoint) * (size_t)n2), o_d2 = A.in(desc2, (size_t)stride2 * n2);
    const size_t o_o1 = A.in(is_orb1, is_orb1 ? n1 : 0), o_o2 = A.in(is_orb2, is_orb2 ? n2 : 0);
    // outputs, contiguous: nmatches | matches12 | prev_matched (uploaded: it is in/out)
    const size_t o_nm = A.in(nullptr, 16);
    const size_t o_m = A.in(nullptr, sizeof(int32_t) * (size_t)c1);
    const size_t o_pm = A.in(prev_matched, prev_matched ? sizeof(float) * 2 * (size_t)n1 : 0);
    A.inout(nmatches, o_nm, sizeof(int32_t)); A.inout(matches12, o_m, sizeof(int32_t) * (size_t)n1); A.inout(prev_matched, o_pm, sizeof(float) * 2 * (size_t)n1);
    if ((rc = A.upload())) return rc;
    const int32_t* dn = A.dev<int32_t>(o_n);
    rc = search_init_dev(c, 1, A.dev<eorb_keypoint>(o_k1), dn, 0, A.dev<uint8_t>(o_d1), stride1, 0, is_orb1 ? A.dev<uint8_t>(o_o1) : nullptr,
                         A.dev<eorb_keypoint>(o_k2), dn + 1, 0, A.dev<uint8_t>(o_d2), stride2, 0, is_orb2 ? A.dev<uint8_t>(o_o2) : nullptr,
                         c1, c2, *gb, prev_matched ? A.dev<float>(o_pm) : nullptr, A.dev<int32_t>(o_m), windowSize, nnratio, checkOri,
                         A.dev<int32_t>(o_nm));
    if (rc) return rc;
    return A.fetch();
}

// ---- marshalling shared by the projection matchers: "queue into the arena, then (after A.upload()) the device view" ---------------
// a mono searched frame
struct FrameOff { size_t k, d, o, ur; int n, stride; bool has_o, has_ur; };
static FrameOff frame_in(Arena& A, const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const uint8_t* is_orb, const float* uright)
{
    return FrameOff{A.in(kps, sizeof(eorb_keypoint) * (size_t)n), A.in(desc, (size_t)stride * n), A.in(is_orb, is_orb ? n : 0),
                    A.in(uright, uright ? sizeof(float) * (size_t)n : 0), n, stride, is_orb != nullptr, uright != nullptr};
}
static FrameDev frame_dev(const Arena& A, const FrameOff& o)
{
    return FrameDev{A.dev<eorb_keypoint>(o.k), o.n, A.dev<uint8_t>(o.d), o.stride, o.has_o ? A.dev<uint8_t>(o.o) : nullptr, o.has_ur ? A.dev<float>(o.ur) : nullptr};
}

// the result region {nmatches, n_in_view | slots (in/out)}: the head of a call's contiguous outputs.  reloc: relocalisation
// (SearchByProjection(CurrentFrame, pKF, sAlreadyFound)) -- every occupied slot is skipped (:2255-2256), only new matches are written back
struct ResultOff { size_t nm, slots; std::vector<int32_t> masked; };
static ResultOff result_in(Arena& A, int32_t* slots, int n, bool reloc = false)
{
    ResultOff o;
    if (reloc) { o.masked.assign(slots, slots + n); for (int32_t& s : o.masked) if (s != -1) s = -2; }
    o.nm = A.in(nullptr, 16); o.slots = A.in(reloc ? o.masked.data() : slots, sizeof(int32_t) * (size_t)n);
    A.want(o.nm, 16);
    if (reloc) A.want(o.slots, sizeof(int32_t) * (size_t)n);      // (merged into the caller's slots by result_out)
    else A.inout(slots, o.slots, sizeof(int32_t) * (size_t)n);
    return o;
}
// the call's fetch: the counts and the slots, and whatever else the call registered
static int result_out(Arena& A, const ResultOff& o, int32_t* slots, int* nmatches, int* n_in_view = nullptr)
{
    const char* h;
    if (const int rc = A.fetch(&h)) return rc;
    const int32_t* cnt = (const int32_t*)(h + o.nm); const int32_t* got = (const int32_t*)(h + o.slots);
    for (size_t i = 0; i < o.masked.size(); i++) if (got[i] >= 0) slots[i] = got[i];
    if (nmatches) *nmatches = cnt[0];
    if (n_in_view) *n_in_view = cnt[1];
    return EORB_OK;
}
// a fused call on an empty frame: the projection ran, no matcher did
static int result_no_matches(eorb_ctx* c, const Arena& A, const ResultOff& o) { EORB_HIP(c, hipMemsetAsync(A.dev<int32_t>(o.nm), 0, sizeof(int32_t), c->stream)); return EORB_OK; }

// a two-camera searched frame (nL left keypoints, then nR right ones) with its stereo links (NULL: the matcher takes none).  The
// checks: sizes, octaves (the kernel keeps levels in 8 bits), slot states (-3 .. nq - 1), the links' ranges
struct TcFrameOff { size_t k, d, l2r, r2l; int nL, nR, stride; bool links; };
static int twocam_frame_in(eorb_ctx* c, Arena& A, const char* who, const eorb_keypoint* kps, int nL, int nR, const uint8_t* desc, int stride,
                           const int32_t* slots, int nq, const int32_t* l2r, const int32_t* r2l, TcFrameOff& o)
{
    const int nT = nL + nR;
    if (nL < 0 || nR < 0 || nq < 0 || stride < 32 || !slots || (nT > 0 && (!kps || !desc))) return set_err(c, EORB_E_ARG, "%s: bad arguments", who);
    if (nT > kTcMaxKps) return set_err(c, EORB_E_CAPACITY, "%s: %d keypoints > %d", who, nT, kTcMaxKps);
    if (nq >= (1 << 24)) return set_err(c, EORB_E_CAPACITY, "%s: %d queries >= 2^24", who, nq);
    for (int i = 0; i < nT; i++) {
        if (kps[i].octave < 0 || kps[i].octave > 127) return set_err(c, EORB_E_ARG, "%s: keypoint %d has octave %d outside [0, 127]", who, i, kps[i].octave);
        if (slots[i] < -3 || slots[i] >= nq) return set_err(c, EORB_E_ARG, "%s: slot %d holds %d", who, i, slots[i]);
    }
    for (int i = 0; l2r && i < nL; i++) if (l2r[i] < -1 || l2r[i] >= nR) return set_err(c, EORB_E_ARG, "%s: l2r[%d] = %d", who, i, l2r[i]);
    for (int i = 0; r2l && i < nR; i++) if (r2l[i] < -1 || r2l[i] >= nL) return set_err(c, EORB_E_ARG, "%s: r2l[%d] = %d", who, i, r2l[i]);
    o.k = A.in(kps, sizeof(eorb_keypoint) * (size_t)nT); o.d = A.in(desc, (size_t)stride * nT);
    o.l2r = A.in(l2r, l2r ? sizeof(int32_t) * (size_t)nL : 0); o.r2l = A.in(r2l, r2l ? sizeof(int32_t) * (size_t)nR : 0);
    o.nL = nL; o.nR = nR; o.stride = stride; o.links = l2r || r2l;
    return EORB_OK;
}
// the block of the two-camera walk.  Q (KIND 0): the map points' records of the left and the right camera; KIND 1 adds its own fields
struct CamQuery { const uint8_t* search; const float4* rec; const int32_t* level; };      // searched or not | projX, projY, viewCos, levelScale | predicted level
static TcArgs twocam_args(const Arena& A, const TcFrameOff& f, const eorb_grid_bounds* gb, int nq, size_t o_md, size_t o_ob, float th, const ResultOff& r,
                          const CamQuery* Q = nullptr, float nnratio = 0.f)
{
    TcArgs T{};
    T.kps = A.dev<eorb_keypoint>(f.k); T.nL = f.nL; T.nR = f.nR; T.desc = A.dev<uint8_t>(f.d); T.stride = f.stride; T.g = grid_b(*gb);
    T.nq = nq; T.mp_desc = A.dev<uint8_t>(o_md); T.mp_obs = A.dev<uint8_t>(o_ob); T.th = th; T.nnratio = nnratio;
    if (f.links) { T.l2r = A.dev<int32_t>(f.l2r); T.r2l = A.dev<int32_t>(f.r2l); }
    if (Q) { T.in_view = Q[0].search; T.qf = Q[0].rec; T.qlevel = Q[0].level; T.in_view_r = Q[1].search; T.qf_r = Q[1].rec; T.qlevel_r = Q[1].level; }
    T.slots = A.dev<int32_t>(r.slots); T.nmatches = A.dev<int32_t>(r.nm);
    return T;
}

// ---- marshalling shared by the RANSAC set solvers (ransac_set.h: eorb_sim3_ransac, eorb_mlpnp_ransac): K problems, each with N
// correspondences and `iters` caller-drawn sets of set_size indices, concatenated ----
struct RansacLimit { int max; const char* name; };
#define RANSAC_LIMIT(m) RansacLimit{m, #m}
// what: the entry point's name in messages; the least N and min_inliers of a problem; the capacities
struct RansacDesc { const char* what; int set_size, min_N, min_min_inliers; RansacLimit problems, corr, iters; };
// a call's totals and its result region, contiguous and zero when the kernels start: the K records | inliers | the per-iteration aids,
// which the entry point declares (A.out) between results() and upload().  upload(): the region's end, A.upload(), the memset
struct RansacCall {
    size_t tN = 0, tI = 0; int max_N = 0, max_iters = 0;
    size_t res = 0, inl = 0;
    void results(Arena& A, void* records, size_t record_bytes, uint8_t* inliers) { res = A.out(records, record_bytes); inl = A.out(inliers, tN); }
    int upload(Arena& A) const
    {
        const size_t end = A.reserve(0);
        if (const int rc = A.upload()) return rc;
        EORB_HIP(A.c, hipMemsetAsync(A.dev<char>(res), 0, end - res, A.c->stream));
        return EORB_OK;
    }
};
static bool cam_model_ok(const eorb_camera& cam) { return cam.model == 0 || cam.model == 1; }
// The checks in their order: K, then per problem the sizes and capacities (no array is read), then the camera models, then per problem
// the set indices.  own(k, problem, pv[k]) is the solver's part of the size pass (its checks, its fields of pv[k]), arrays(k, head) its
// checks of its own arrays after problem k's sets.  Fills the heads of pv and the totals.
extern "C++" template <class Pub, class Dev, class Own, class CamOk, class Arrays>
static int ransac_problems_in(eorb_ctx* c, const RansacDesc& D, const Pub* problems, int K, const int32_t* sets, std::vector<Dev>& pv, RansacCall& R,
                              Own own, CamOk cam_ok, Arrays arrays)
{
    const char* what = D.what;
    int rc;
    if (K < 1) return set_err(c, EORB_E_ARG, "%s: %d problems (at least 1)", what, K);
    if (K > D.problems.max) return set_err(c, EORB_E_CAPACITY, "%s: %d problems, at most %s = %d", what, K, D.problems.name, D.problems.max);
    pv.assign((size_t)K, Dev{});
    for (int k = 0; k < K; k++) {
        const Pub& p = problems[k];
        if (p.N < D.min_N || p.iters < 1 || p.min_inliers < D.min_min_inliers)
            return set_err(c, EORB_E_ARG, "%s: problem %d has %d correspondences (at least %d), %d iterations (at least 1), min_inliers %d (at least %d)", what, k,
                           p.N, D.min_N, p.iters, p.min_inliers, D.min_min_inliers);
        if (p.N > D.corr.max) return set_err(c, EORB_E_CAPACITY, "%s: problem %d has %d correspondences, at most %s = %d", what, k, p.N, D.corr.name, D.corr.max);
        if (p.iters > D.iters.max) return set_err(c, EORB_E_CAPACITY, "%s: problem %d has %d iterations, at most %s = %d", what, k, p.iters, D.iters.name, D.iters.max);
        if ((rc = own(k, p, pv[k]))) return rc;
        RansacProb& d = pv[k];
        d.N = p.N; d.iters = p.iters; d.corr_off = (int)R.tN; d.set_off = (int)R.tI; d.min_inliers = p.min_inliers;
        R.tN += (size_t)p.N; R.tI += (size_t)p.iters;
        R.max_N = std::max(R.max_N, p.N); R.max_iters = std::max(R.max_iters, p.iters);
    }
    for (int k = 0; k < K; k++)
        if (!cam_ok(problems[k])) return set_err(c, EORB_E_CONFIG, "%s: problem %d has a camera model other than Pinhole (0) / KannalaBrandt8 (1)", what, k);
    for (int k = 0; k < K; k++) {
        const RansacProb& d = pv[k];
        for (int i = 0; i < D.set_size * d.iters; i++) {
            const int32_t s = sets[D.set_size * (size_t)d.set_off + i];
            if (s < 0 || s >= d.N)
                return set_err(c, EORB_E_ARG, "%s: problem %d, set %d holds the index %d of %d correspondences", what, k, i / D.set_size, s, d.N);
        }
        if ((rc = arrays(k, d))) return rc;
    }
    return EORB_OK;
}
// ---- matchers, projections given by the caller -----------------------------------------------------------------------------------
// reloc: the slot semantics of eorb_search_by_projection_kf (result_in)
static int proj_last_common(eorb_ctx* c,
        const eorb_keypoint* cur_kps, int n_cur, const uint8_t* cur_desc, int cur_stride, const uint8_t* cur_is_orb,
        const eorb_keypoint* last_kps, int n_last, const uint8_t* last_is_orb,
        const uint8_t* valid, const float* uv, const uint8_t* mp_desc, const uint8_t* mp_obs,
        const float* level_scale, const eorb_grid_bounds* gb, int32_t* cur_mp, float th, int mode, int checkOri,
        int dist_th, int* nmatches, const float* cur_uright = nullptr, const float* q_ur = nullptr, bool reloc = false)
{
    if (!c) return EORB_E_ARG;
    if (n_cur < 0 || n_last < 0 || !gb || !cur_mp || cur_stride < 32 || !level_scale || ((cur_uright != nullptr) != (q_ur != nullptr)))
        return set_err(c, EORB_E_ARG, "search_by_projection_last: bad arguments");
    fe_enter(c);
    if (nmatches) *nmatches = 0;
    if (n_last == 0 || n_cur == 0) return EORB_OK;
    int rc;
    Arena A(c);
    const FrameOff fr = frame_in(A, cur_kps, n_cur, cur_desc, cur_stride, cur_is_orb, cur_uright);
    const size_t o_lk = A.in(last_kps, sizeof(eorb_keypoint) * (size_t)n_last), o_md = A.in(mp_desc, 32 * (size_t)n_last);
    const size_t o_lo = A.in(last_is_orb, last_is_orb ? n_last : 0);
    std::vector<float> f3(3 * (size_t)n_last);
    for (int i = 0; i < n_last; i++) { f3[3 * i] = uv[2 * i]; f3[3 * i + 1] = uv[2 * i + 1]; f3[3 * i + 2] = level_scale[i]; }
    const size_t o_f3 = A.in(f3.data(), sizeof(float) * f3.size());
    const size_t o_va = A.in(valid, n_last), o_ob = A.in(mp_obs, n_last);
    const size_t o_qur = A.in(q_ur, q_ur ? sizeof(float) * (size_t)n_last : 0);
    const ResultOff r = result_in(A, cur_mp, n_cur, reloc);
    if ((rc = A.upload())) return rc;
    const ProjLastArgs P{frame_dev(A, fr), grid_b(*gb), A.dev<eorb_keypoint>(o_lk), n_last, last_is_orb ? A.dev<uint8_t>(o_lo) : nullptr,
                         A.dev<uint8_t>(o_va), A.dev<float>(o_f3), A.dev<uint8_t>(o_md), A.dev<uint8_t>(o_ob),
                         q_ur ? A.dev<float>(o_qur) : nullptr, th, mode, checkOri, dist_th, A.dev<int32_t>(r.slots), A.dev<int32_t>(r.nm)};
    if ((rc = search_proj_last_dev(c, P))) return rc;
    return result_out(A, r, cur_mp, nmatches);
}

int eorb_search_by_projection_last(eorb_ctx* c,
        const eorb_keypoint* cur_kps, int n_cur, const uint8_t* cur_desc, int cur_stride, const uint8_t* cur_is_orb,
        const eorb_keypoint* last_kps, int n_last, const uint8_t* last_is_orb,
        const uint8_t* valid, const float* uv, const uint8_t* mp_desc, const uint8_t* mp_obs,
        const float* level_scale, const eorb_grid_bounds* gb, int32_t* cur_mp, float th, int mode, int checkOri,
        int* nmatches)
{
    return proj_last_common(c, cur_kps, n_cur, cur_desc, cur_stride, cur_is_orb, last_kps, n_last, last_is_orb, valid, uv, mp_desc,
                            mp_obs, level_scale, gb, cur_mp, th, mode, checkOri, 100 /* TH_HIGH */, nmatches);
}

int eorb_search_by_projection_last_stereo(eorb_ctx* c,
        const eorb_keypoint* cur_kps, int n_cur, const uint8_t* cur_desc, int cur_stride, const uint8_t* cur_is_orb,
        const eorb_keypoint* last_kps, int n_last, const uint8_t* last_is_orb,
        const uint8_t* valid, const float* uv, const uint8_t* mp_desc, const uint8_t* mp_obs,
        const float* level_scale, const eorb_grid_bounds* gb, int32_t* cur_mp, float th, int mode, int checkOri,
        const float* cur_uright, const float* proj_ur, int* nmatches)
{
    if (c && (!cur_uright || !proj_ur)) return set_err(c, EORB_E_ARG, "search_by_projection_last_stereo: mvuRight and the projected right coordinates are needed");
    return proj_last_common(c, cur_kps, n_cur, cur_desc, cur_stride, cur_is_orb, last_kps, n_last, last_is_orb, valid, uv, mp_desc,
                            mp_obs, level_scale, gb, cur_mp, th, mode, checkOri, 100 /* TH_HIGH */, nmatches, cur_uright, proj_ur);
}

int eorb_search_by_projection_kf(eorb_ctx* c,
        const eorb_keypoint* cur_kps, int n_cur, const uint8_t* cur_desc, int cur_stride, const uint8_t* cur_is_orb,
        const eorb_keypoint* kf_kps, int n_kf, const uint8_t* kf_is_orb,
        const uint8_t* valid, const float* uv, const int32_t* pred_level, const float* level_scale, const uint8_t* mp_desc,
        const eorb_grid_bounds* gb, int32_t* cur_mp, float th, int ORBdist, int checkOri, int* nmatches)
{
    if (!c) return EORB_E_ARG;
    if (n_kf < 0 || (n_kf > 0 && (!kf_kps || !pred_level || !valid))) return set_err(c, EORB_E_ARG, "search_by_projection_kf: bad arguments");
    // the last-frame kernel with: query level = nPredictedLevel (:2236), window [L-1, L+1] (:2241), every occupied slot of the
    // current frame skipped (:2255-2256) and ORBdist in place of TH_HIGH (:2271)
    std::vector<eorb_keypoint> q(kf_kps, kf_kps + n_kf);
    for (int i = 0; i < n_kf; i++) { q[i].octave = pred_level[i]; q[i].class_id = pred_level[i]; }
    const std::vector<uint8_t> obs((size_t)n_kf, 1);
    return proj_last_common(c, cur_kps, n_cur, cur_desc, cur_stride, cur_is_orb, q.data(), n_kf, kf_is_orb, valid, uv, mp_desc,
                            obs.data(), level_scale, gb, cur_mp, th, 0, checkOri, ORBdist, nmatches, nullptr, nullptr, true);
}

static int proj_map_common(eorb_ctx* c,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const uint8_t* is_orb,
        int M, const uint8_t* in_view, const float* proj_xy, const int32_t* level, const float* view_cos,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const uint8_t* mp_is_orb, const float* level_scale,
        const eorb_grid_bounds* gb, int32_t* frame_mp, float th, float nnratio, int* nmatches, const float* uright, const float* proj_xr)
{
    if (!c) return EORB_E_ARG;
    if (n < 0 || M < 0 || !gb || !frame_mp || stride < 32 || ((uright != nullptr) != (proj_xr != nullptr))) return set_err(c, EORB_E_ARG, "search_by_projection_map: bad arguments");
    fe_enter(c);
    if (nmatches) *nmatches = 0;
    if (M == 0 || n == 0) return EORB_OK;
    int rc;
    Arena A(c);
    const FrameOff fr = frame_in(A, kps, n, desc, stride, is_orb, uright);
    const size_t o_md = A.in(mp_desc, 32 * (size_t)M);
    // per map point record: proj x, proj y, view cos, level scale (floats) | level (int) | in_view, obs, is_orb (bytes)
    std::vector<float> f4(4 * (size_t)M);
    for (int m = 0; m < M; m++) { f4[4 * m] = proj_xy[2 * m]; f4[4 * m + 1] = proj_xy[2 * m + 1]; f4[4 * m + 2] = view_cos[m]; f4[4 * m + 3] = level_scale[m]; }
    const size_t o_f4 = A.in(f4.data(), sizeof(float) * f4.size()), o_lv = A.in(level, sizeof(int32_t) * (size_t)M);
    const size_t o_iv = A.in(in_view, M), o_ob = A.in(mp_obs, M), o_mo = A.in(mp_is_orb, mp_is_orb ? M : 0);
    const size_t o_qur = A.in(proj_xr, proj_xr ? sizeof(float) * (size_t)M : 0);
    const ResultOff r = result_in(A, frame_mp, n);
    if ((rc = A.upload())) return rc;
    const ProjMapArgs P{frame_dev(A, fr), grid_b(*gb), M, A.dev<uint8_t>(o_iv), A.dev<float4>(o_f4), A.dev<int32_t>(o_lv),
                        A.dev<uint8_t>(o_md), A.dev<uint8_t>(o_ob), mp_is_orb ? A.dev<uint8_t>(o_mo) : nullptr,
                        proj_xr ? A.dev<float>(o_qur) : nullptr, th, nnratio, A.dev<int32_t>(r.slots), A.dev<int32_t>(r.nm)};
    if ((rc = search_proj_map_dev(c, P))) return rc;
    return result_out(A, r, frame_mp, nmatches);
}

int eorb_search_by_projection_map(eorb_ctx* c,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const uint8_t* is_orb,
        int M, const uint8_t* in_view, const float* proj_xy, const int32_t* level, const float* view_cos,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const uint8_t* mp_is_orb, const float* level_scale,
        const eorb_grid_bounds* gb, int32_t* frame_mp, float th, float nnratio, int* nmatches)
{
    return proj_map_common(c, kps, n, desc, stride, is_orb, M, in_view, proj_xy, level, view_cos, mp_desc, mp_obs, mp_is_orb, level_scale, gb,
                           frame_mp, th, nnratio, nmatches, nullptr, nullptr);
}

int eorb_search_by_projection_map_stereo(eorb_ctx* c,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const uint8_t* is_orb,
        int M, const uint8_t* in_view, const float* proj_xy, const int32_t* level, const float* view_cos,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const uint8_t* mp_is_orb, const float* level_scale,
        const eorb_grid_bounds* gb, int32_t* frame_mp, float th, float nnratio, const float* uright, const float* proj_xr, int* nmatches)
{
    if (c && (!uright || !proj_xr)) return set_err(c, EORB_E_ARG, "search_by_projection_map_stereo: mvuRight and mTrackProjXR are needed");
    return proj_map_common(c, kps, n, desc, stride, is_orb, M, in_view, proj_xy, level, view_cos, mp_desc, mp_obs, mp_is_orb, level_scale, gb,
                           frame_mp, th, nnratio, nmatches, uright, proj_xr);
}

// ---- map points projected on the device (project.hip) ---------------------------------------------------------------------------
static int view_check(eorb_ctx* c, const char* who, const eorb_view* v, bool has_is_orb)
{
    if (!v) return set_err(c, EORB_E_ARG, "%s: null view", who);
    if (v->nlevels < 1 || v->nlevels > 128 || !v->scale_factors) return set_err(c, EORB_E_ARG, "%s: nlevels %d outside 1..128 or no scale factors", who, v->nlevels);
    if (v->ak_nlevels < 0 || v->ak_nlevels > 128 || (v->ak_nlevels > 0 && !v->ak_scale_factors))
        return set_err(c, EORB_E_ARG, "%s: ak_nlevels %d outside 0..128 or no AKAZE scale factors", who, v->ak_nlevels);
    if (v->cam.model != 0 && v->cam.model != 1) return set_err(c, EORB_E_ARG, "%s: camera model %d", who, v->cam.model);
    if (has_is_orb && v->ak_nlevels == 0) return set_err(c, EORB_E_ARG, "%s: descriptor kinds given for a view without AKAZE tables", who);
    return EORB_OK;
}

struct ViewOff { size_t sf, ak; };
static ViewOff view_in(Arena& A, const eorb_view* v)
{
    ViewOff o;
    o.sf = A.in(v->scale_factors, sizeof(float) * (size_t)v->nlevels);
    o.ak = A.in(v->ak_scale_factors, v->ak_nlevels > 0 ? sizeof(float) * (size_t)v->ak_nlevels : 0);
    return o;
}
static ProjView view_dev(const Arena& A, const eorb_view* v, const ViewOff& o)      // after A.upload()
{
    ProjView P{};
    memcpy(P.R, v->R, sizeof(P.R)); memcpy(P.t, v->t, sizeof(P.t)); memcpy(P.Ow, v->Ow, sizeof(P.Ow));
    P.cam = warp_cam_of(v->cam);
    P.minX = v->minX; P.maxX = v->maxX; P.minY = v->minY; P.maxY = v->maxY; P.mbf = v->mbf;
    P.nlevels = v->nlevels; P.log_scale = v->log_scale; P.sf = A.dev<float>(o.sf);
    P.ak_nlevels = v->ak_nlevels; P.ak_log_scale = v->ak_log_scale; P.ak_sf = v->ak_nlevels > 0 ? A.dev<float>(o.ak) : nullptr;
    return P;
}

// the arena regions of one view's eorb_frustum_out, contiguous in the struct's order; then the matcher's records
struct FrustumOff { size_t iv, xy, xr, lv, vc, dp, ls, rs, rec, srch; };
static FrustumOff frustum_reserve(Arena& A, int M, const eorb_frustum_out* out)      // out: the view's record, or NULL (nothing of it is taken)
{
    const size_t m = (size_t)M;
    const eorb_frustum_out d = out ? *out : eorb_frustum_out{};
    FrustumOff o;
    o.iv = A.out(d.in_view, m); o.xy = A.out(d.proj_xy, 8 * m); o.xr = A.out(d.proj_xr, 4 * m); o.lv = A.out(d.level, 4 * m); o.vc = A.out(d.view_cos, 4 * m);
    o.dp = A.out(d.depth, 4 * m); o.ls = A.out(d.level_scale, 4 * m); o.rs = A.out(d.reason, m);
    return o;
}
static void frustum_reserve_recs(Arena& A, int M, FrustumOff& o) { o.rec = A.reserve(16 * (size_t)M); o.srch = A.reserve((size_t)M); }
static FrustumDev frustum_dev(const Arena& A, const FrustumOff& o)
{
    return FrustumDev{A.dev<uint8_t>(o.iv), A.dev<float2>(o.xy), A.dev<float>(o.xr), A.dev<int32_t>(o.lv), A.dev<float>(o.vc),
                      A.dev<float>(o.dp), A.dev<float>(o.ls), A.dev<uint8_t>(o.rs), A.dev<float4>(o.rec), A.dev<uint8_t>(o.srch)};
}

// the points of modes A, B and C and their arena offsets (is_orb: per map point, or per query keypoint in mode B)
struct PointsOff { size_t pos, nrm, mind, maxd, skip, orb; bool has_skip, has_orb; };
static PointsOff points_in(Arena& A, int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                           const uint8_t* skip, const uint8_t* is_orb)
{
    const size_t m = (size_t)M;
    return PointsOff{A.in(pos, 12 * m), A.in(normal, normal ? 12 * m : 0), A.in(min_dist, min_dist ? 4 * m : 0), A.in(max_dist, max_dist ? 4 * m : 0),
                     A.in(skip, skip ? m : 0), A.in(is_orb, is_orb ? m : 0), skip != nullptr, is_orb != nullptr};
}

// mode A over nviews views
static FrustumArgs frustum_args(const Arena& A, const eorb_view* views, int nviews, const ViewOff* vo, const FrustumOff* fo, int M, const PointsOff& po,
                                float cos_limit, int far, float th_far, int32_t* n_in_view)
{
    FrustumArgs F{};
    for (int v = 0; v < nviews; v++) { F.V[v] = view_dev(A, views + v, vo[v]); F.O[v] = frustum_dev(A, fo[v]); }
    F.nviews = nviews; F.M = M;
    F.pos = A.dev<float>(po.pos); F.normal = A.dev<float>(po.nrm); F.min_dist = A.dev<float>(po.mind); F.max_dist = A.dev<float>(po.maxd);
    F.skip = po.has_skip ? A.dev<uint8_t>(po.skip) : nullptr; F.is_orb = po.has_orb ? A.dev<uint8_t>(po.orb) : nullptr;
    F.cos_limit = cos_limit; F.far = far; F.th_far = th_far; F.n_in_view = n_in_view;
    return F;
}

// the output regions of modes B (ur = proj_ur, uvr) and C (lv = level, d3 = dist3d).  Each entry point reserves them in the order of
// its own outputs
struct PoseOff { size_t va, uv, lv, ls, ur, uvr, d3, rec; };
static LastArgs last_args(const Arena& A, const eorb_view* view, const ViewOff& vo, int n, const PointsOff& po, const eorb_keypoint* d_kps, const PoseOff& o)
{
    LastArgs L{};
    L.V = view_dev(A, view, vo);
    L.n = n; L.pos = A.dev<float>(po.pos); L.skip = po.has_skip ? A.dev<uint8_t>(po.skip) : nullptr; L.kps = d_kps;
    L.is_orb = po.has_orb ? A.dev<uint8_t>(po.orb) : nullptr;
    L.valid = A.dev<uint8_t>(o.va); L.uv = A.dev<float2>(o.uv); L.proj_ur = A.dev<float>(o.ur); L.level_scale = A.dev<float>(o.ls);
    L.uv_r = A.dev<float2>(o.uvr); L.rec3 = A.dev<float>(o.rec);
    return L;
}
static KfArgs kf_args(const Arena& A, const eorb_view* view, const ViewOff& vo, int n, const PointsOff& po, const PoseOff& o)
{
    KfArgs K{};
    K.V = view_dev(A, view, vo);
    K.n = n; K.pos = A.dev<float>(po.pos); K.min_dist = A.dev<float>(po.mind); K.max_dist = A.dev<float>(po.maxd);
    K.skip = po.has_skip ? A.dev<uint8_t>(po.skip) : nullptr; K.is_orb = po.has_orb ? A.dev<uint8_t>(po.orb) : nullptr;
    K.valid = A.dev<uint8_t>(o.va); K.uv = A.dev<float2>(o.uv); K.level = A.dev<int32_t>(o.lv); K.level_scale = A.dev<float>(o.ls);
    K.dist3d = A.dev<float>(o.d3); K.rec3 = A.dev<float>(o.rec);
    return K;
}

int eorb_project_frustum(eorb_ctx* c, const eorb_view* views, int nviews, int M, const float* pos, const float* normal,
                         const float* min_dist, const float* max_dist, const uint8_t* skip, const uint8_t* mp_is_orb, float cos_limit,
                         const eorb_frustum_out* out, int* n_in_view)
{
    if (!c) return EORB_E_ARG;
    if (n_in_view) *n_in_view = 0;
    if (M < 0 || nviews < 1 || nviews > 2 || !views || (M > 0 && (!pos || !normal || !min_dist || !max_dist)))
        return set_err(c, EORB_E_ARG, "project_frustum: bad arguments");
    int rc;
    for (int v = 0; v < nviews; v++) if ((rc = view_check(c, "project_frustum", views + v, mp_is_orb != nullptr))) return rc;
    fe_enter(c);
    if (M == 0) return EORB_OK;
    Arena A(c);
    const PointsOff po = points_in(A, M, pos, normal, min_dist, max_dist, skip, mp_is_orb);
    ViewOff vo[2] = {view_in(A, views), nviews > 1 ? view_in(A, views + 1) : ViewOff{0, 0}};
    // outputs: n_in_view | view 0 | view 1; then the matcher records (device only)
    const size_t o_n = A.out(nullptr, 16);
    A.inout(n_in_view, o_n, sizeof(int32_t));
    FrustumOff fo[2];
    for (int v = 0; v < nviews; v++) fo[v] = frustum_reserve(A, M, out ? out + v : nullptr);
    for (int v = 0; v < nviews; v++) frustum_reserve_recs(A, M, fo[v]);
    if ((rc = A.upload())) return rc;
    if ((rc = project_frustum_dev(c, frustum_args(A, views, nviews, vo, fo, M, po, cos_limit, 0, 0.f, A.dev<int32_t>(o_n))))) return rc;
    return A.fetch();
}

static int last_octave_check(eorb_ctx* c, const char* who, const eorb_view* v, const eorb_keypoint* kps, const uint8_t* is_orb, int n)
{
    for (int i = 0; i < n; i++) {
        const int nl = (is_orb && !is_orb[i] && v->ak_nlevels > 0) ? v->ak_nlevels : v->nlevels;
        if (kps[i].octave < 0 || kps[i].octave >= nl) return set_err(c, EORB_E_ARG, "%s: keypoint %d has octave %d outside [0, %d)", who, i, kps[i].octave, nl);
    }
    return EORB_OK;
}

int eorb_project_last_frame(eorb_ctx* c, const eorb_view* view, const eorb_camera* cam_r, const float* Trl, int n, const float* pos,
                            const uint8_t* skip, const eorb_keypoint* last_kps, const uint8_t* last_is_orb,
                            uint8_t* valid, float* uv, float* proj_ur, float* level_scale, float* uv_r)
{
    if (!c) return EORB_E_ARG;
    if (n < 0 || (n > 0 && (!pos || !last_kps)) || ((Trl != nullptr) != (cam_r != nullptr)) || (uv_r && !Trl))
        return set_err(c, EORB_E_ARG, "project_last_frame: bad arguments");
    int rc;
    if ((rc = view_check(c, "project_last_frame", view, last_is_orb != nullptr))) return rc;
    if (cam_r && cam_r->model != 0 && cam_r->model != 1) return set_err(c, EORB_E_ARG, "project_last_frame: camera model %d", cam_r->model);
    if ((rc = last_octave_check(c, "project_last_frame", view, last_kps, last_is_orb, n))) return rc;
    fe_enter(c);
    if (n == 0) return EORB_OK;
    const size_t m = (size_t)n;
    Arena A(c);
    const PointsOff po = points_in(A, n, pos, nullptr, nullptr, nullptr, skip, last_is_orb);
    const size_t o_k = A.in(last_kps, sizeof(eorb_keypoint) * m);
    const ViewOff vo = view_in(A, view);
    // outputs: valid | uv | proj_ur | level_scale | uv_r; then the matcher's record
    PoseOff o{};
    o.va = A.out(valid, m); o.uv = A.out(uv, 8 * m); o.ur = A.out(proj_ur, 4 * m); o.ls = A.out(level_scale, 4 * m); o.uvr = A.out(uv_r, 8 * m);
    o.rec = A.reserve(12 * m);
    if ((rc = A.upload())) return rc;
    LastArgs L = last_args(A, view, vo, n, po, A.dev<eorb_keypoint>(o_k), o);
    L.has_r = Trl ? 1 : 0;
    if (Trl) { L.cam_r = warp_cam_of(*cam_r); memcpy(L.Trl, Trl, sizeof(L.Trl)); }
    if ((rc = project_last_dev(c, L))) return rc;
    return A.fetch();
}

int eorb_project_keyframe_points(eorb_ctx* c, const eorb_view* view, int n, const float* pos, const float* min_dist,
                                 const float* max_dist, const uint8_t* skip, const uint8_t* mp_is_orb,
                                 uint8_t* valid, float* uv, int32_t* level, float* level_scale, float* dist3d)
{
    if (!c) return EORB_E_ARG;
    if (n < 0 || (n > 0 && (!pos || !min_dist || !max_dist))) return set_err(c, EORB_E_ARG, "project_keyframe_points: bad arguments");
    int rc;
    if ((rc = view_check(c, "project_keyframe_points", view, mp_is_orb != nullptr))) return rc;
    fe_enter(c);
    if (n == 0) return EORB_OK;
    const size_t m = (size_t)n;
    Arena A(c);
    const PointsOff po = points_in(A, n, pos, nullptr, min_dist, max_dist, skip, mp_is_orb);
    const ViewOff vo = view_in(A, view);
    // outputs: valid | uv | level | level_scale | dist3d; then the matcher's record
    PoseOff o{};
    o.va = A.out(valid, m); o.uv = A.out(uv, 8 * m); o.lv = A.out(level, 4 * m); o.ls = A.out(level_scale, 4 * m); o.d3 = A.out(dist3d, 4 * m);
    o.rec = A.reserve(12 * m);
    if ((rc = A.upload())) return rc;
    if ((rc = project_kf_dev(c, kf_args(A, view, vo, n, po, o)))) return rc;
    return A.fetch();
}

int eorb_search_local_points(eorb_ctx* c,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const uint8_t* is_orb,
        const eorb_view* view, int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
        const uint8_t* skip, const uint8_t* mp_is_orb, float cos_limit,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const eorb_grid_bounds* gb, int32_t* frame_mp, float th, float nnratio,
        const float* uright, int bFarPoints, float thFarPoints,
        const eorb_frustum_out* out, int* n_in_view, int* nmatches)
{
    if (!c) return EORB_E_ARG;
    if (nmatches) *nmatches = 0;
    if (n_in_view) *n_in_view = 0;
    if (n < 0 || M < 0 || !gb || !frame_mp || stride < 32 || (n > 0 && (!kps || !desc)) ||
        (M > 0 && (!pos || !normal || !min_dist || !max_dist || !mp_desc || !mp_obs)))
        return set_err(c, EORB_E_ARG, "search_local_points: bad arguments");
    int rc;
    if ((rc = view_check(c, "search_local_points", view, mp_is_orb != nullptr))) return rc;
    fe_enter(c);
    if (M == 0) return EORB_OK;
    Arena A(c);
    const FrameOff fr = frame_in(A, kps, n, desc, stride, is_orb, uright);
    const size_t o_md = A.in(mp_desc, 32 * (size_t)M), o_ob = A.in(mp_obs, M);
    const PointsOff po = points_in(A, M, pos, normal, min_dist, max_dist, skip, mp_is_orb);
    const ViewOff vo = view_in(A, view);
    // outputs: {nmatches, n_in_view} | slots (in/out) | the projection arrays
    const ResultOff r = result_in(A, frame_mp, n);
    FrustumOff fo = frustum_reserve(A, M, out);
    frustum_reserve_recs(A, M, fo);
    if ((rc = A.upload())) return rc;
    const FrustumArgs F = frustum_args(A, view, 1, &vo, &fo, M, po, cos_limit, bFarPoints != 0, thFarPoints, A.dev<int32_t>(r.nm) + 1);
    if ((rc = project_frustum_dev(c, F))) return rc;
    if (n > 0) {
        const ProjMapArgs P{frame_dev(A, fr), grid_b(*gb), M, F.O[0].search, F.O[0].rec, F.O[0].level, A.dev<uint8_t>(o_md), A.dev<uint8_t>(o_ob),
                            F.is_orb, uright ? F.O[0].proj_xr : nullptr, th, nnratio, A.dev<int32_t>(r.slots), A.dev<int32_t>(r.nm)};
        rc = search_proj_map_dev(c, P);
    } else rc = result_no_matches(c, A, r);
    if (rc) return rc;
    return result_out(A, r, frame_mp, nmatches, n_in_view);
}

int eorb_search_local_points_fisheye(eorb_ctx* c,
        const eorb_keypoint* kps, int nL, int nR, const uint8_t* desc, int stride, const int32_t* l2r, const int32_t* r2l,
        const eorb_view* views, int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
        const uint8_t* skip, float cos_limit,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const eorb_grid_bounds* gb, int32_t* frame_mp, float th, float nnratio,
        int bFarPoints, float thFarPoints,
        const eorb_frustum_out* out, int* n_in_view, int* nmatches)
{
    if (!c) return EORB_E_ARG;
    if (nmatches) *nmatches = 0;
    if (n_in_view) *n_in_view = 0;
    if (!gb || M < 0 || !views || (M > 0 && (!pos || !normal || !min_dist || !max_dist || !mp_desc || !mp_obs)) || (nL > 0 && !l2r) || (nR > 0 && !r2l))
        return set_err(c, EORB_E_ARG, "search_local_points_fisheye: bad arguments");
    int rc;
    for (int v = 0; v < 2; v++) if ((rc = view_check(c, "search_local_points_fisheye", views + v, false))) return rc;
    Arena A(c);
    TcFrameOff fr;
    if ((rc = twocam_frame_in(c, A, "search_local_points_fisheye", kps, nL, nR, desc, stride, frame_mp, M, l2r, r2l, fr))) return rc;
    fe_enter(c);
    const int nT = nL + nR;
    if (M == 0) return EORB_OK;
    const size_t o_md = A.in(mp_desc, 32 * (size_t)M), o_ob = A.in(mp_obs, M);
    const PointsOff po = points_in(A, M, pos, normal, min_dist, max_dist, skip, nullptr);
    const ViewOff vo[2] = {view_in(A, views), view_in(A, views + 1)};
    const ResultOff r = result_in(A, frame_mp, nT);
    FrustumOff fo[2];
    for (int v = 0; v < 2; v++) fo[v] = frustum_reserve(A, M, out ? out + v : nullptr);
    for (int v = 0; v < 2; v++) frustum_reserve_recs(A, M, fo[v]);
    if ((rc = A.upload())) return rc;
    const FrustumArgs F = frustum_args(A, views, 2, vo, fo, M, po, cos_limit, bFarPoints != 0, thFarPoints, A.dev<int32_t>(r.nm) + 1);
    if ((rc = project_frustum_dev(c, F))) return rc;
    const CamQuery Q[2] = {{F.O[0].search, F.O[0].rec, F.O[0].level}, {F.O[1].search, F.O[1].rec, F.O[1].level}};
    if ((rc = nT > 0 ? twocam_walk_dev(c, 0, twocam_args(A, fr, gb, M, o_md, o_ob, th, r, Q, nnratio)) : result_no_matches(c, A, r))) return rc;
    return result_out(A, r, frame_mp, nmatches, n_in_view);
}

// modes B and C in front of the last-frame matcher.  kf: the semantics of eorb_search_by_projection_kf (query level = the predicted
// level, every occupied slot skipped, ORBdist in place of TH_HIGH)
static int proj_pose_common(eorb_ctx* c, const char* who, bool kf,
        const eorb_keypoint* cur_kps, int n_cur, const uint8_t* cur_desc, int cur_stride, const uint8_t* cur_is_orb,
        const eorb_view* view, const eorb_keypoint* q_kps, int nq, const uint8_t* q_is_orb,
        const float* pos, const float* min_dist, const float* max_dist, const uint8_t* skip, const uint8_t* mp_desc, const uint8_t* mp_obs,
        const eorb_grid_bounds* gb, int32_t* cur_mp, float th, int mode, int checkOri, int dist_th, const float* cur_uright,
        uint8_t* valid, float* uv, int32_t* level, int* nmatches)
{
    if (!c) return EORB_E_ARG;
    if (nmatches) *nmatches = 0;
    if (n_cur < 0 || nq < 0 || !gb || !cur_mp || cur_stride < 32 || (n_cur > 0 && (!cur_kps || !cur_desc)) ||
        (nq > 0 && (!q_kps || !pos || !mp_desc || (kf ? (!min_dist || !max_dist) : !mp_obs))) || mode < 0 || mode > 2)
        return set_err(c, EORB_E_ARG, "%s: bad arguments", who);
    int rc;
    if ((rc = view_check(c, who, view, q_is_orb != nullptr))) return rc;
    if (!kf && (rc = last_octave_check(c, who, view, q_kps, q_is_orb, nq))) return rc;
    fe_enter(c);
    if (nq == 0) return EORB_OK;
    const size_t m = (size_t)nq;
    const std::vector<uint8_t> obs(kf ? m : 0, 1);
    Arena A(c);
    const FrameOff fr = frame_in(A, cur_kps, n_cur, cur_desc, cur_stride, cur_is_orb, cur_uright);
    const size_t o_qk = A.in(q_kps, sizeof(eorb_keypoint) * m);
    const size_t o_md = A.in(mp_desc, 32 * m), o_ob = A.in(kf ? obs.data() : mp_obs, m);
    const PointsOff po = points_in(A, nq, pos, nullptr, min_dist, max_dist, skip, q_is_orb);
    const ViewOff vo = view_in(A, view);
    // outputs: nmatches | slots (in/out) | valid | uv | level; then what only the matcher reads
    const ResultOff r = result_in(A, cur_mp, n_cur, kf);
    PoseOff o{};
    o.va = A.out(valid, m); o.uv = A.out(uv, 8 * m); o.lv = A.out(level, 4 * m);
    o.ls = A.reserve(4 * m); o.ur = o.d3 = A.reserve(4 * m); o.uvr = A.reserve(8 * m); o.rec = A.reserve(12 * m);      // (ur, d3: one region, by mode)
    const size_t o_q2 = A.reserve(sizeof(eorb_keypoint) * m);
    if ((rc = A.upload())) return rc;
    const eorb_keypoint* d_q = A.dev<eorb_keypoint>(o_qk);
    if (kf) {
        KfArgs K = kf_args(A, view, vo, nq, po, o);
        K.kf_kps = d_q; K.q_kps = A.dev<eorb_keypoint>(o_q2);
        rc = project_kf_dev(c, K);
        d_q = K.q_kps;
    } else rc = project_last_dev(c, last_args(A, view, vo, nq, po, d_q, o));
    if (rc) return rc;
    if (n_cur > 0) {
        const ProjLastArgs P{frame_dev(A, fr), grid_b(*gb), d_q, nq, po.has_orb ? A.dev<uint8_t>(po.orb) : nullptr, A.dev<uint8_t>(o.va),
                             A.dev<float>(o.rec), A.dev<uint8_t>(o_md), A.dev<uint8_t>(o_ob), cur_uright ? A.dev<float>(o.ur) : nullptr,
                             th, mode, checkOri, dist_th, A.dev<int32_t>(r.slots), A.dev<int32_t>(r.nm)};
        rc = search_proj_last_dev(c, P);
    } else rc = result_no_matches(c, A, r);
    if (rc) return rc;
    return result_out(A, r, cur_mp, nmatches);
}

int eorb_search_by_projection_last_pose(eorb_ctx* c,
        const eorb_keypoint* cur_kps, int n_cur, const uint8_t* cur_desc, int cur_stride, const uint8_t* cur_is_orb,
        const eorb_view* view, const eorb_keypoint* last_kps, int n_last, const uint8_t* last_is_orb,
        const float* pos, const uint8_t* skip, const uint8_t* mp_desc, const uint8_t* mp_obs,
        const eorb_grid_bounds* gb, int32_t* cur_mp, float th, int mode, int checkOri, const float* cur_uright,
        uint8_t* valid, float* uv, int* nmatches)
{
    return proj_pose_common(c, "search_by_projection_last_pose", false, cur_kps, n_cur, cur_desc, cur_stride, cur_is_orb, view, last_kps, n_last,
                            last_is_orb, pos, nullptr, nullptr, skip, mp_desc, mp_obs, gb, cur_mp, th, mode, checkOri, 100 /* TH_HIGH */,
                            cur_uright, valid, uv, nullptr, nmatches);
}

int eorb_search_by_projection_kf_pose(eorb_ctx* c,
        const eorb_keypoint* cur_kps, int n_cur, const uint8_t* cur_desc, int cur_stride, const uint8_t* cur_is_orb,
        const eorb_view* view, const eorb_keypoint* kf_kps, int n_kf, const uint8_t* kf_is_orb,
        const float* pos, const float* min_dist, const float* max_dist, const uint8_t* skip, const uint8_t* mp_desc,
        const eorb_grid_bounds* gb, int32_t* cur_mp, float th, int ORBdist, int checkOri,
        uint8_t* valid, float* uv, int32_t* level, int* nmatches)
{
    return proj_pose_common(c, "search_by_projection_kf_pose", true, cur_kps, n_cur, cur_desc, cur_stride, cur_is_orb, view, kf_kps, n_kf,
                            kf_is_orb, pos, min_dist, max_dist, skip, mp_desc, nullptr, gb, cur_mp, th, 0, checkOri, ORBdist,
                            nullptr, valid, uv, level, nmatches);
}

// ---- two-camera frames: the frame seam and the tracking matchers ------------------------------------------------------------
int eorb_frame_fisheye(eorb_ctx* c, const uint8_t* imLeft, const uint8_t* imRight, int W, int H, int stride,
                       int lapL0, int lapL1, int lapR0, int lapR1,
                       eorb_keypoint* kpsL, uint8_t* descL, int* nL, int* monoLeft,
                       eorb_keypoint* kpsR, uint8_t* descR, int* nR, int* monoRight, int cap,
                       int32_t* right_idx, int32_t* dist2, int* ncand)
{
    if (!c) return EORB_E_ARG;
    if (nL) *nL = 0; if (nR) *nR = 0; if (monoLeft) *monoLeft = 0; if (monoRight) *monoRight = 0; if (ncand) *ncand = 0;
    int rc;
    if ((rc = image_check(c, "eorb_frame_fisheye", imLeft && imRight ? imLeft : nullptr, W, H, stride))) return rc;
    if (cap < 0) return set_err(c, EORB_E_ARG, "eorb_frame_fisheye: capacity %d", cap);
    fe_enter(c);
    Arena A(c);
    const size_t o_imL = image_in(A, imLeft, W, H, stride, false), o_imR = image_in(A, imRight, W, H, stride, false);
    // outputs: the result block of the pair | candidates | distances (n[0] of each, copied after the checks); then the knn scratch
    const ExtractDst dst[2] = {{kpsL, descL, nullptr, nL, monoLeft}, {kpsR, descR, nullptr, nR, monoRight}};
    const ExtractOff X = extract_reserve(A, c->orb.max_out, 2, cap, dst);
    const size_t mo = X.mo;
    const size_t o_cand = A.out(nullptr, sizeof(int32_t) * mo), o_d2 = A.out(nullptr, 2 * sizeof(int32_t) * mo);
    if (right_idx) A.want(o_cand, sizeof(int32_t) * X.ncopy);
    if (dist2) A.want(o_d2, 2 * sizeof(int32_t) * X.ncopy);
    A.reserve(0);                                        // (an empty region; tests/golden/arena_layout.json pins the layout)
    const size_t o_idx = A.reserve(2 * sizeof(int32_t) * mo), o_kd = A.reserve(2 * sizeof(int32_t) * mo);
    if ((rc = A.upload())) return rc;
    ExtractHead* hd = A.dev<ExtractHead>(X.head);
    EORB_HIP(c, hipMemsetAsync(hd, 0, sizeof(ExtractHead), c->stream));       // (the candidates are counted by atomics)
    // ExtractORB(0, imLeft, mvLappingArea of mpCamera) and ExtractORB(1, imRight, mvLappingArea of mpCamera2) (Frame.cc:1124-1129):
    // two launches, each with its own lapping area
    rc = orb_extract_dev(c, A.dev<uint8_t>(o_imL), W, 0, 1, lapL0, lapL1, 1, A.dev<eorb_keypoint>(X.kp), A.dev<uint8_t>(X.desc), nullptr, hd->n, hd->mono, hd->flag);
    if (rc) return rc;
    rc = orb_extract_dev(c, A.dev<uint8_t>(o_imR), W, 0, 1, lapR0, lapR1, 1, A.dev<eorb_keypoint>(X.kp) + mo, A.dev<uint8_t>(X.desc) + 32 * mo,
                         nullptr, hd->n + 1, hd->mono + 1, hd->flag + 1);
    if (rc) return rc;
    if ((rc = fisheye_lowe_dev(c, A.dev<uint8_t>(X.desc), A.dev<uint8_t>(X.desc) + 32 * mo, (int)mo, hd->n, A.dev<int32_t>(o_idx), A.dev<int32_t>(o_kd),
                               A.dev<int32_t>(o_cand), A.dev<int32_t>(o_d2)))) return rc;
    const char* h;
    if ((rc = A.fetch(&h))) return rc;
    const ExtractHead* got;
    if ((rc = extract_out(c, "eorb_frame_fisheye", h, X, cap, 2, dst, &got))) return rc;
    if (right_idx && got->n[0] > 0) memcpy(right_idx, h + o_cand, sizeof(int32_t) * (size_t)got->n[0]);
    if (dist2 && got->n[0] > 0) memcpy(dist2, h + o_d2, 2 * sizeof(int32_t) * (size_t)got->n[0]);
    if (ncand) *ncand = got->aux[0];
    return EORB_OK;
}

int eorb_search_by_projection_map_fisheye(eorb_ctx* c,
        const eorb_keypoint* kps, int nL, int nR, const uint8_t* desc, int stride, const int32_t* l2r, const int32_t* r2l,
        int M, const uint8_t* in_view, const float* proj_xy, const int32_t* level, const float* view_cos, const float* level_scale,
        const uint8_t* in_view_r, const float* proj_xy_r, const int32_t* level_r, const float* view_cos_r, const float* level_scale_r,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const eorb_grid_bounds* gb, int32_t* frame_mp, float th, float nnratio,
        int* nmatches)
{
    if (!c) return EORB_E_ARG;
    if (nmatches) *nmatches = 0;
    if (!gb || M < 0 || (M > 0 && (!in_view || !proj_xy || !level || !view_cos || !level_scale || !in_view_r || !proj_xy_r || !level_r ||
                                   !view_cos_r || !level_scale_r || !mp_desc || !mp_obs)) ||
        (nL > 0 && !l2r) || (nR > 0 && !r2l))
        return set_err(c, EORB_E_ARG, "search_by_projection_map_fisheye: bad arguments");
    int rc;
    Arena A(c);
    TcFrameOff fr;
    if ((rc = twocam_frame_in(c, A, "search_by_projection_map_fisheye", kps, nL, nR, desc, stride, frame_mp, M, l2r, r2l, fr))) return rc;
    fe_enter(c);
    const int nT = nL + nR;
    if (M == 0 || nT == 0) return EORB_OK;
    const size_t o_md = A.in(mp_desc, 32 * (size_t)M);
    // per map point and camera: proj x, proj y, view cos, level scale
    std::vector<float> f4(8 * (size_t)M);
    for (int m = 0; m < M; m++) {
        float* l = &f4[4 * (size_t)m]; float* r = &f4[4 * ((size_t)M + m)];
        l[0] = proj_xy[2 * m]; l[1] = proj_xy[2 * m + 1]; l[2] = view_cos[m]; l[3] = level_scale[m];
        r[0] = proj_xy_r[2 * m]; r[1] = proj_xy_r[2 * m + 1]; r[2] = view_cos_r[m]; r[3] = level_scale_r[m];
    }
    const size_t o_f4 = A.in(f4.data(), sizeof(float) * f4.size());
    const size_t o_lv = A.in(level, sizeof(int32_t) * (size_t)M), o_lvr = A.in(level_r, sizeof(int32_t) * (size_t)M);
    const size_t o_iv = A.in(in_view, M), o_ivr = A.in(in_view_r, M), o_ob = A.in(mp_obs, M);
    const ResultOff r = result_in(A, frame_mp, nT);
    if ((rc = A.upload())) return rc;
    const CamQuery Q[2] = {{A.dev<uint8_t>(o_iv), A.dev<float4>(o_f4), A.dev<int32_t>(o_lv)},
                           {A.dev<uint8_t>(o_ivr), A.dev<float4>(o_f4) + M, A.dev<int32_t>(o_lvr)}};
    if ((rc = twocam_walk_dev(c, 0, twocam_args(A, fr, gb, M, o_md, o_ob, th, r, Q, nnratio)))) return rc;
    return result_out(A, r, frame_mp, nmatches);
}

int eorb_search_by_projection_last_fisheye(eorb_ctx* c,
        const eorb_keypoint* cur_kps, int nL, int nR, const uint8_t* cur_desc, int cur_stride,
        const eorb_keypoint* last_kps, int n_last, const uint8_t* valid, const float* uv, const float* uv_r,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const float* level_scale, const eorb_grid_bounds* gb,
        int32_t* cur_mp, float th, int mode, int checkOri, int* nmatches)
{
    if (!c) return EORB_E_ARG;
    if (nmatches) *nmatches = 0;
    if (!gb || n_last < 0 || mode < 0 || mode > 2 ||
        (n_last > 0 && (!last_kps || !valid || !uv || !uv_r || !mp_desc || !mp_obs || !level_scale)))
        return set_err(c, EORB_E_ARG, "search_by_projection_last_fisheye: bad arguments");
    int rc;
    Arena A(c);
    TcFrameOff fr;
    if ((rc = twocam_frame_in(c, A, "search_by_projection_last_fisheye", cur_kps, nL, nR, cur_desc, cur_stride, cur_mp, n_last, nullptr, nullptr, fr))) return rc;
    fe_enter(c);
    const int nT = nL + nR;
    if (n_last == 0 || nT == 0) return EORB_OK;
    const size_t o_lk = A.in(last_kps, sizeof(eorb_keypoint) * (size_t)n_last), o_md = A.in(mp_desc, 32 * (size_t)n_last);
    std::vector<float> f5(5 * (size_t)n_last);
    for (int i = 0; i < n_last; i++) {
        float* f = &f5[5 * (size_t)i];
        f[0] = uv[2 * i]; f[1] = uv[2 * i + 1]; f[2] = uv_r[2 * i]; f[3] = uv_r[2 * i + 1]; f[4] = level_scale[i];
    }
    const size_t o_f5 = A.in(f5.data(), sizeof(float) * f5.size());
    const size_t o_va = A.in(valid, n_last), o_ob = A.in(mp_obs, n_last);
    const ResultOff r = result_in(A, cur_mp, nT);
    const size_t o_rec = A.reserve(2 * sizeof(int32_t) * (size_t)n_last);
    if ((rc = A.upload())) return rc;
    TcArgs T = twocam_args(A, fr, gb, n_last, o_md, o_ob, th, r);
    T.valid = A.dev<uint8_t>(o_va); T.quv = A.dev<float>(o_f5); T.qkps = A.dev<eorb_keypoint>(o_lk); T.mode = mode; T.checkOri = checkOri;
    T.rec = A.dev<int32_t>(o_rec);
    if ((rc = twocam_walk_dev(c, 1, T))) return rc;
    return result_out(A, r, cur_mp, nmatches);
}

// ---- the node walks (SearchByBoW, SearchForTriangulation) over K keyframes per call (eorb_kf_set of include/eorb_fe.h); the single-pair
// entry points are the same code with a set of one ----------------------------------------------------------------------------------
static constexpr int kKfBatchMaxKfs = 1024;                             // K
static constexpr int64_t kKfBatchMaxOut = (int64_t)1 << 22;             // K * the length of one output row
static constexpr int64_t kKfBatchMaxRows = (int64_t)1 << 22;            // rows of all keyframes together; feature indices likewise

// one feature vector as the device walks need it (tri_entry bisects the offsets, bow_node reads off[a + 1]): offsets from 0 that never
// decrease, every index inside the side's features; k >= 0 names the keyframe of a set
static int fv_check(eorb_ctx* c, const char* what, const char* name, int k, const int32_t* off, const int32_t* idx, int nn, int n_features)
{
    char who[48];
    if (k >= 0) snprintf(who, sizeof(who), "keyframe %d", k); else snprintf(who, sizeof(who), "%s", name);
    if (nn == 0) return EORB_OK;
    if (off[0] != 0) return set_err(c, EORB_E_ARG, "%s: %s: node offsets start at %d", what, who, off[0]);
    for (int a = 0; a < nn; a++) if (off[a + 1] < off[a]) return set_err(c, EORB_E_ARG, "%s: %s: node offsets decrease at node %d", what, who, a);
    if (off[nn] > kKfBatchMaxRows) return set_err(c, EORB_E_CAPACITY, "%s: %s: %d feature indices exceed %lld", what, who, off[nn], (long long)kKfBatchMaxRows);
    for (int i = 0; i < off[nn]; i++)
        if (idx[i] < 0 || idx[i] >= n_features) return set_err(c, EORB_E_ARG, "%s: %s: feature index out of range", what, who);
    return EORB_OK;
}

// the set as a call's input: check() decides the limits from the sizes, then reads the offsets, then every index; queue() lays the
// slice table and the concatenated arrays out in the arena (pack32: descriptor rows cut to their first 32 bytes, the BoW walk's row)
struct KfSetIn {
    std::vector<KfSlice> sl; int K = 0, ntotal = 0, nnodes = 0, nidx = 0, max_nn = 0, dstride = 0;
    size_t o_sl = 0, o_kps = 0, o_desc = 0, o_flag = 0, o_nodes = 0, o_off = 0, o_idx = 0;
    int check(eorb_ctx* c, const char* what, const eorb_kf_set* S, int n_out)
    {
        if (!S || S->K < 0 || n_out < 0) return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
        K = S->K;
        if (K > kKfBatchMaxKfs || (int64_t)K * n_out > kKfBatchMaxOut)                 // (sizes only: nothing is read before this)
            return set_err(c, EORB_E_CAPACITY, "%s: %d keyframes x %d outputs exceed %d keyframes or %lld outputs", what, K, n_out, kKfBatchMaxKfs,
                           (long long)kKfBatchMaxOut);
        if (K == 0) return EORB_OK;
        if (S->stride < 32 || !S->kf_off || !S->node_off) return set_err(c, EORB_E_ARG, "%s: bad keyframe set", what);
        if (S->kf_off[0] != 0 || S->node_off[0] != 0) return set_err(c, EORB_E_ARG, "%s: kf_off[0] = %d, node_off[0] = %d", what, S->kf_off[0], S->node_off[0]);
        for (int k = 0; k < K; k++)
            if (S->kf_off[k + 1] < S->kf_off[k] || S->node_off[k + 1] < S->node_off[k])
                return set_err(c, EORB_E_ARG, "%s: kf_off or node_off decreases at keyframe %d", what, k);
        ntotal = S->kf_off[K]; nnodes = S->node_off[K];
        if (ntotal > kKfBatchMaxRows || nnodes > kKfBatchMaxRows)
            return set_err(c, EORB_E_CAPACITY, "%s: %d rows, %d nodes exceed %lld", what, ntotal, nnodes, (long long)kKfBatchMaxRows);
        if ((ntotal > 0 && (!S->kps || !S->desc || !S->flag)) || (nnodes > 0 && (!S->nodes || !S->feat_off || !S->idx)))
            return set_err(c, EORB_E_ARG, "%s: keyframe set without arrays", what);
        sl.resize(K);
        int64_t idx0 = 0;
        for (int k = 0; k < K; k++) {
            KfSlice& s = sl[k];
            s.row0 = S->kf_off[k]; s.nrows = S->kf_off[k + 1] - s.row0;
            s.node0 = S->node_off[k]; s.nn = S->node_off[k + 1] - s.node0;
            s.off0 = s.node0 + k; s.idx0 = (int32_t)idx0;
            int rc;
            if ((rc = fv_check(c, what, nullptr, k, S->feat_off + s.off0, S->idx + idx0, s.nn, s.nrows))) return rc;
            if (s.nn > 0) idx0 += S->feat_off[s.off0 + s.nn];
            if (idx0 > kKfBatchMaxRows) return set_err(c, EORB_E_CAPACITY, "%s: feature indices exceed %lld at keyframe %d", what, (long long)kKfBatchMaxRows, k);
            max_nn = std::max(max_nn, s.nn);
        }
        nidx = (int)idx0;
        return EORB_OK;
    }
    void queue(Arena& A, const eorb_kf_set* S, bool pack32)
    {
        o_sl = A.in(sl.data(), sizeof(KfSlice) * (size_t)K);
        o_kps = A.in(S->kps, sizeof(eorb_keypoint) * (size_t)ntotal);
        dstride = pack32 ? 32 : S->stride;
        o_desc = pack32 ? A.in2d(S->desc, ntotal, 32, (size_t)S->stride) : A.in(S->desc, (size_t)S->stride * ntotal);
        o_flag = A.in(S->flag, (size_t)ntotal);
        o_nodes = A.in(S->nodes, sizeof(int32_t) * (size_t)nnodes);
        o_off = A.in(S->feat_off, sizeof(int32_t) * ((size_t)nnodes + K));
        o_idx = A.in(S->idx, sizeof(int32_t) * (size_t)nidx);
    }
    FeatVec fv(const Arena& A) const { return FeatVec{A.dev<uint32_t>(o_nodes), A.dev<int32_t>(o_off), A.dev<int32_t>(o_idx), 0}; }
};

// one keyframe as a set of one: a view of the caller's arrays, nothing copied (node_off[nn + 1] is the set's feat_off at K = 1)
struct KfSetOne {
    int32_t kf_off[2], node_off[2]; eorb_kf_set S;
    KfSetOne(const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const uint8_t* flag,
             const uint32_t* nodes, const int32_t* off, const int32_t* idx, int nn)
        : kf_off{0, n}, node_off{0, nn}, S{1, kps, desc, stride, flag, kf_off, nodes, node_off, off, idx} {}
    KfSetOne(const KfSetOne&) = delete;
};

// the shared side's feature vector, straight from the caller's arrays
struct FvIn {
    size_t o_nodes = 0, o_off = 0, o_idx = 0; int nn = 0;
    void queue(Arena& A, const uint32_t* nodes, const int32_t* off, const int32_t* idx, int n)
    {
        nn = n;
        o_nodes = A.in(nodes, sizeof(int32_t) * (size_t)nn); o_off = A.in(off, sizeof(int32_t) * ((size_t)nn + 1));
        o_idx = A.in(idx, sizeof(int32_t) * (size_t)off[nn]);
    }
    FeatVec fv(const Arena& A) const { return FeatVec{A.dev<uint32_t>(o_nodes), A.dev<int32_t>(o_off), A.dev<int32_t>(o_idx), nn}; }
};

// K rows of n outputs: every slot -1, every count 0 (what a call returns where nothing can match)
static void kfbatch_clear(int K, int n, int32_t* out, int32_t* nmatches)
{
    for (size_t i = 0; i < (size_t)K * n; i++) out[i] = -1;
    if (nmatches) for (int k = 0; k < K; k++) nmatches[k] = 0;
}

// ---- CreateNewMapPoints (newpts.hip): the stage as a part of a call.  check() reads the arguments, queue() / reserve() lay its inputs and
// its results out in the call's arena (the results right behind whatever the call declared before: the call's one fetch covers both),
// launch() enqueues the kernels on a match12 that is already on the device ----
static void np_clear(int K, int n1, const eorb_newpts_out* O)
{
    const size_t n = (size_t)K * n1;
    if (!O) return;
    if (O->status) memset(O->status, EORB_NP_NO_MATCH, n);
    if (O->x3d) memset(O->x3d, 0, sizeof(float) * 3 * n);
    if (O->branch) memset(O->branch, 0, n);
    if (O->cos_parallax) memset(O->cos_parallax, 0, sizeof(float) * n);
    if (O->n_new) memset(O->n_new, 0, sizeof(int32_t) * (size_t)K);
}

struct NpJob {
    const eorb_newpts_params* P = nullptr; const eorb_newpts_out* O = nullptr;
    int K = 0, n1 = 0, ntotal = 0;
    std::vector<NpKf> kf; NpView v1[2];
    size_t o_v1 = 0, o_kf = 0, o_in[2][6] = {}, o_ls = 0, o_lg = 0;
    size_t o_st = 0, o_x = 0, o_br = 0, o_cs = 0, o_nn = 0, o_end = 0, o_tmp = 0, o_ps = 0;

    static NpView view_of(const eorb_view& v)
    {
        NpView o{};
        memcpy(o.R, v.R, sizeof o.R); memcpy(o.t, v.t, sizeof o.t); memcpy(o.Ow, v.Ow, sizeof o.Ow);
        o.cam = warp_cam_of(v.cam); o.mbf = v.mbf;
        return o;
    }
    // kps2 / kf_off: the neighbours' keypoints concatenated.  Sizes were decided by the caller (KfSetIn::check or the stage's own limits)
    int check(eorb_ctx* c, const char* what, const eorb_keypoint* kps1, int n1_, const eorb_keypoint* kps2, const int32_t* kf_off, int K_,
              const eorb_newpts_params* P_, const eorb_newpts_out* O_)
    {
        P = P_; O = O_; K = K_; n1 = n1_;
        if (!P || !O || (K > 0 && (!O->n_new || (n1 > 0 && !O->status)))) return set_err(c, EORB_E_ARG, "%s: params, out, out->status and out->n_new are required", what);
        if (P->form != EORB_NEWPTS_LOCAL_MAPPING && P->form != EORB_NEWPTS_TRACKING) return set_err(c, EORB_E_ARG, "%s: form %d", what, P->form);
        if (K == 0) return EORB_OK;
        ntotal = kf_off[K];
        if (!P->views1 || !P->views2 || (n1 > 0 && !kps1) || (ntotal > 0 && !kps2)) return set_err(c, EORB_E_ARG, "%s: views and keypoints are required", what);
        if (P->nleft1 < -1 || P->nleft1 > n1) return set_err(c, EORB_E_ARG, "%s: nleft1 %d", what, P->nleft1);
        const bool twocam = P->nleft1 >= 0;
        if (twocam && P->form == EORB_NEWPTS_TRACKING) return set_err(c, EORB_E_ARG, "%s: the Tracking form has no two-camera branch (nleft1 %d)", what, P->nleft1);
        if (twocam && !P->nleft2) return set_err(c, EORB_E_ARG, "%s: nleft2 is required with nleft1 >= 0", what);
        if (!(P->mb1 >= 0.f) || !(P->mb1 <= 3.40282347e+38f)) return set_err(c, EORB_E_ARG, "%s: mb1 is negative or not finite", what);
        const int nv = twocam ? 2 : 1;
        kf.assign((size_t)K, NpKf{});
        for (int k = 0; k < K; k++) {
            NpKf& d = kf[k];
            d.row0 = kf_off[k]; d.nrows = kf_off[k + 1] - kf_off[k];
            d.nleft2 = P->nleft2 ? P->nleft2[k] : -1;
            if (d.nleft2 < -1 || d.nleft2 > d.nrows) return set_err(c, EORB_E_ARG, "%s: keyframe %d: nleft2 %d", what, k, d.nleft2);
            if (twocam != (d.nleft2 >= 0))
                return set_err(c, P->form == EORB_NEWPTS_TRACKING ? EORB_E_ARG : EORB_E_CONFIG, "%s: keyframe %d: one keyframe of the pair has two cameras and the other one", what, k);
            d.mb = P->mb2 ? P->mb2[k] : 0.f;
            if (!(d.mb >= 0.f) || !(d.mb <= 3.40282347e+38f)) return set_err(c, EORB_E_ARG, "%s: keyframe %d: mb is negative or not finite", what, k);
        }
        for (int v = 0; v < nv; v++)
            if (P->views1[v].cam.model != 0 && P->views1[v].cam.model != 1)
                return set_err(c, EORB_E_CONFIG, "%s: pKF1's camera %d has a model other than Pinhole (0) / KannalaBrandt8 (1)", what, v);
        for (int k = 0; k < K; k++)
            for (int v = 0; v < nv; v++)
                if (P->views2[(size_t)nv * k + v].cam.model != 0 && P->views2[(size_t)nv * k + v].cam.model != 1)
                    return set_err(c, EORB_E_CONFIG, "%s: keyframe %d: camera %d has a model other than Pinhole (0) / KannalaBrandt8 (1)", what, k, v);
        for (int v = 0; v < 2; v++) v1[v] = view_of(P->views1[v < nv ? v : 0]);
        for (int k = 0; k < K; k++)
            for (int v = 0; v < 2; v++) kf[k].v[v] = view_of(P->views2[(size_t)nv * k + (v < nv ? v : 0)]);
        const eorb_newpts_side* S[2] = {&P->side1, &P->side2};
        const eorb_keypoint* kp[2] = {kps1, kps2};
        const int n[2] = {n1, ntotal};
        for (int s = 0; s < 2; s++) {
            if (S[s]->uright && !S[s]->depth) return set_err(c, EORB_E_ARG, "%s: side %d: uright without depth", what, s + 1);
            if (!S[s]->kp_sigma2 || !S[s]->kp_scale) {
                if (!P->level_scale || !P->level_sigma2 || P->nlevels <= 0 || P->nlevels > 64)
                    return set_err(c, EORB_E_ARG, "%s: side %d has no kp_sigma2 / kp_scale and the call no level tables", what, s + 1);
                for (int i = 0; i < n[s]; i++)
                    if (kp[s][i].octave < 0 || kp[s][i].octave >= P->nlevels)
                        return set_err(c, EORB_E_ARG, "%s: side %d: keypoint %d has octave %d outside [0,%d)", what, s + 1, i, kp[s][i].octave, P->nlevels);
            }
            if (S[s]->uright)
                for (int i = 0; i < n[s]; i++)
                    if (S[s]->uright[i] >= 0 && !(fabsf(S[s]->depth[i]) <= 3.40282347e+38f))
                        return set_err(c, EORB_E_ARG, "%s: side %d: keypoint %d has a right coordinate and a depth that is not finite", what, s + 1, i);
        }
        return EORB_OK;
    }
    void queue(Arena& A)
    {
        o_v1 = A.in(v1, sizeof v1); o_kf = A.in(kf.data(), sizeof(NpKf) * (size_t)K);
        const eorb_newpts_side* S[2] = {&P->side1, &P->side2};
        const size_t n[2] = {(size_t)n1, (size_t)ntotal};
        for (int s = 0; s < 2; s++) {
            o_in[s][0] = A.in(S[s]->kp_sigma2, S[s]->kp_sigma2 ? 4 * n[s] : 0); o_in[s][1] = A.in(S[s]->kp_scale, S[s]->kp_scale ? 4 * n[s] : 0);
            o_in[s][2] = A.in(S[s]->kp_is_orb, S[s]->kp_is_orb ? n[s] : 0); o_in[s][3] = A.in(S[s]->uright, S[s]->uright ? 4 * n[s] : 0);
            o_in[s][4] = A.in(S[s]->depth, S[s]->depth ? 4 * n[s] : 0); o_in[s][5] = A.in(S[s]->raw_xy, S[s]->raw_xy ? 8 * n[s] : 0);
        }
        const size_t nl = P->level_scale && P->level_sigma2 && P->nlevels > 0 ? (size_t)P->nlevels : 0;
        o_ls = A.in(P->level_scale, 4 * nl); o_lg = A.in(P->level_sigma2, 4 * nl);
    }
    // results, contiguous and zero on entry: status | x3d | branch | cos_parallax | n_new; then the scratch
    void reserve(Arena& A)
    {
        const size_t n = (size_t)K * n1;
        o_st = A.out(O->status, n); o_x = A.out(O->x3d, 12 * n); o_br = A.out(O->branch, n); o_cs = A.out(O->cos_parallax, 4 * n); o_nn = A.out(O->n_new, 4 * (size_t)K);
        o_end = A.reserve(0);
        o_tmp = A.reserve(2 * n); o_ps = A.reserve(4);
    }
    int launch(eorb_ctx* c, const Arena& A, const eorb_keypoint* d_kps1, const eorb_keypoint* d_kps2, const int32_t* d_match12)
    {
        EORB_HIP(c, hipMemsetAsync(A.dev<char>(o_st), 0, o_end - o_st, c->stream));
        EORB_HIP(c, hipMemsetAsync(A.dev<char>(o_ps), 0x7f, 4, c->stream));
        NpArgs T{};
        T.kps1 = d_kps1; T.kps2 = d_kps2; T.n1 = n1; T.K = K; T.nleft1 = P->nleft1; T.form = P->form;
        T.v1 = A.dev<NpView>(o_v1); T.mb1 = P->mb1; T.kf = A.dev<NpKf>(o_kf);
        const eorb_newpts_side* S[2] = {&P->side1, &P->side2};
        NpSide* D[2] = {&T.s1, &T.s2};
        for (int s = 0; s < 2; s++) {
            D[s]->sigma2 = S[s]->kp_sigma2 ? A.dev<float>(o_in[s][0]) : nullptr; D[s]->scale = S[s]->kp_scale ? A.dev<float>(o_in[s][1]) : nullptr;
            D[s]->is_orb = S[s]->kp_is_orb ? A.dev<uint8_t>(o_in[s][2]) : nullptr; D[s]->uright = S[s]->uright ? A.dev<float>(o_in[s][3]) : nullptr;
            D[s]->depth = S[s]->depth ? A.dev<float>(o_in[s][4]) : nullptr; D[s]->raw_xy = S[s]->raw_xy ? A.dev<float>(o_in[s][5]) : nullptr;
        }
        T.level_scale = A.dev<float>(o_ls); T.level_sigma2 = A.dev<float>(o_lg); T.nlevels = P->nlevels;
        T.rf_orb = P->ratio_factor_orb; T.rf_ak = P->ratio_factor_ak; T.far_points = P->far_points; T.th_far = P->th_far_points;
        T.match12 = d_match12; T.tmp = A.dev<uint8_t>(o_tmp); T.pstar = A.dev<int32_t>(o_ps);
        T.status = A.dev<uint8_t>(o_st); T.x3d = A.dev<float>(o_x); T.branch = A.dev<uint8_t>(o_br); T.cosp = A.dev<float>(o_cs); T.n_new = A.dev<int32_t>(o_nn);
        return new_map_points_dev(c, T);
    }
};

// outputs of a batched walk: [K x (32 histogram bins + nmatches) | K x n matches]; then the rotation bins.  The counts sit one to a
// histogram row: kfbatch_out picks them out of the host view
struct KfBatchOut { size_t o_hist, o_m, o_bin; };
static KfBatchOut kfbatch_reserve(Arena& A, int K, int n, int32_t* out, const int32_t* nmatches)
{
    KfBatchOut o;
    o.o_hist = A.out(nullptr, sizeof(int32_t) * kPairHist * (size_t)K); o.o_m = A.out(out, sizeof(int32_t) * (size_t)K * n); o.o_bin = A.reserve((size_t)K * n);
    if (nmatches) A.want(o.o_hist, sizeof(int32_t) * kPairHist * (size_t)K);
    return o;
}
// the call's fetch (a triangulation stage behind the walk has registered its results: NpJob::reserve)
static int kfbatch_out(Arena& A, const KfBatchOut& o, int K, int32_t* nmatches)
{
    const char* h;
    if (const int rc = A.fetch(&h)) return rc;
    if (nmatches) for (int k = 0; k < K; k++) memcpy(nmatches + k, h + o.o_hist + sizeof(int32_t) * ((size_t)k * kPairHist + 32), 4);
    return EORB_OK;
}

// the BoW-node walk of SearchForTriangulation (:975-1214) over the K keyframes of a set, shared by both camera models: kb == nullptr runs
// the Pinhole test on F12, otherwise KannalaBrandt8::epipolarConstrain with kb's cameras and the pairs' poses.  pKF1 and the level tables
// are uploaded once, the pairs' values go into device tables.  what: the entry point, in messages and as the profile scope
static int search_tri_common(eorb_ctx* c, const char* what,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1, const eorb_kf_set* S, KfSetIn& J,
        const float* ep, const float* F12, const float* scale2, const float* sigma2_2, const float* sigma2_1, int nlevels,
        int bCoarse, int checkOri, TriKbArgs* kb, const int32_t* nleft2, const float* Rt, int32_t* match12, int32_t* nmatches,
        NpJob* np = nullptr)
{
    const int K = J.K;
    fe_enter(c);
    kfbatch_clear(K, n1, match12, nmatches);
    if (np) np_clear(K, n1, np->O);
    if (K == 0 || n1 == 0 || nn1 == 0 || J.ntotal == 0 || J.max_nn == 0) return EORB_OK;
    int rc;
    if ((rc = fv_check(c, what, "pKF1", -1, node_off1, idx1, nn1, n1))) return rc;
    for (int k = 0; k < K; k++) {
        const KfSlice& s = J.sl[k];
        if (s.nn == 0) continue;
        for (int i = s.row0; i < s.row0 + s.nrows; i++)
            if (S->flag[i] && (S->kps[i].octave < 0 || S->kps[i].octave >= nlevels))
                return set_err(c, EORB_E_ARG, "%s: keyframe %d: keypoint %d has octave %d outside [0,%d)", what, k, i - s.row0, S->kps[i].octave, nlevels);
    }
    if (kb)
        for (int i = 0; i < n1; i++)
            if ((elig1[i] & 1) && (kps1[i].octave < 0 || kps1[i].octave >= nlevels))
                return set_err(c, EORB_E_ARG, "%s: pKF1 keypoint %d has octave %d outside [0,%d)", what, i, kps1[i].octave, nlevels);
    std::vector<TriPair> P(K);
    std::vector<TriKbPair> Q(kb ? K : 0);
    const int nrt = kb && kb->nleft1 >= 0 ? 48 : 12;
    for (int k = 0; k < K; k++) {
        P[k] = TriPair{};
        P[k].epx = ep[2 * k]; P[k].epy = ep[2 * k + 1];
        if (F12) for (int i = 0; i < 9; i++) P[k].F[i] = F12[9 * k + i];
        if (kb) {
            Q[k] = TriKbPair{};
            Q[k].nleft2 = nleft2[k];
            for (int i = 0; i < nrt; i++) Q[k].Rt[i] = Rt[(size_t)nrt * k + i];
        }
    }
    Arena A(c);
    FvIn f1;
    f1.queue(A, nodes1, node_off1, idx1, nn1);
    const size_t o_k1 = A.in(kps1, sizeof(eorb_keypoint) * n1), o_d1 = A.in(desc1, (size_t)stride1 * n1), o_e1 = A.in(elig1, n1);
    const size_t o_sc = A.in(scale2, sizeof(float) * nlevels), o_sg = A.in(sigma2_2, sizeof(float) * nlevels);
    const size_t o_s1 = kb ? A.in(sigma2_1, sizeof(float) * nlevels) : 0;
    J.queue(A, S, false);
    const size_t o_p = A.in(P.data(), sizeof(TriPair) * (size_t)K), o_q = kb ? A.in(Q.data(), sizeof(TriKbPair) * (size_t)K) : 0;
    if (np) np->queue(A);
    const KfBatchOut o = kfbatch_reserve(A, K, n1, match12, nmatches);
    if (np) np->reserve(A);
    if ((rc = A.upload())) return rc;
    TriBatchArgs B{};
    TriArgs& T = B.T;
    T.kps1 = A.dev<eorb_keypoint>(o_k1); T.n1 = n1; T.desc1 = A.dev<uint8_t>(o_d1); T.stride1 = stride1;
    T.elig1 = A.dev<uint8_t>(o_e1); T.fv1 = f1.fv(A);
    T.kps2 = A.dev<eorb_keypoint>(J.o_kps); T.n2 = 0; T.desc2 = A.dev<uint8_t>(J.o_desc); T.stride2 = J.dstride;
    T.elig2 = A.dev<uint8_t>(J.o_flag); T.fv2 = J.fv(A);
    T.scale2 = A.dev<float>(o_sc); T.sigma2_2 = A.dev<float>(o_sg); T.nlevels = nlevels;
    T.bCoarse = bCoarse; T.checkOri = checkOri;
    T.match12 = A.dev<int32_t>(o.o_m); T.bin1 = A.dev<int8_t>(o.o_bin); T.histo = A.dev<int32_t>(o.o_hist); T.nmatches = T.histo + 32;
    B.kf = A.dev<KfSlice>(J.o_sl); B.pair = A.dev<TriPair>(o_p); B.K = K;
    TriKbBatchArgs KB{};
    if (kb) {
        kb->T = T; kb->sigma2_1 = A.dev<float>(o_s1);
        KB.K = *kb; KB.kf = B.kf; KB.pair = B.pair; KB.kb = A.dev<TriKbPair>(o_q); KB.nk = K;
    }
    if ((rc = search_tri_batch_dev(c, what, B, kb ? &KB : nullptr))) return rc;
    // the stage on the rows where they are; one copy brings both halves' results back
    if (np && (rc = np->launch(c, A, T.kps1, T.kps2, T.match12))) return rc;
    return kfbatch_out(A, o, K, nmatches);
}

// the cameras of a KannalaBrandt8 walk into its block: pKF1's must be KannalaBrandt8, the other side's Pinhole or KannalaBrandt8
static int kb8_cameras(eorb_ctx* c, const char* what, int nleft1, const eorb_camera* cam1, const eorb_camera* cam2, TriKbArgs& KA)
{
    const int nc1 = nleft1 >= 0 ? 2 : 1;
    for (int k = 0; k < nc1; k++)
        if (cam1[k].model != 1)
            return set_err(c, EORB_E_CONFIG, "%s: pKF1's camera %d is not KannalaBrandt8 (Pinhole pCamera1: the entry point without kb8)", what, k);
    for (int k = 0; k < nc1; k++)
        if (cam2[k].model != 0 && cam2[k].model != 1) return set_err(c, EORB_E_ARG, "%s: pKF2's camera %d has model %d", what, k, cam2[k].model);
    KA.nleft1 = nleft1;
    for (int k = 0; k < 2; k++) { KA.cam1[k] = cam1[k < nc1 ? k : 0]; KA.cam2[k] = cam2[k < nc1 ? k : 0]; }
    return EORB_OK;
}

int eorb_search_for_triangulation_keyframes(eorb_ctx* c,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_kf_set* set, const float* ep, const float* F12, const float* scale2, const float* sigma2_2, int nlevels,
        int bCoarse, int checkOri, int32_t* match12, int32_t* nmatches)
{
    if (!c) return EORB_E_ARG;
    const char* what = "search_for_triangulation_keyframes";
    KfSetIn I;
    int rc;
    if ((rc = I.check(c, what, set, n1))) return rc;
    if (nn1 < 0 || stride1 < 32 || !scale2 || !sigma2_2 || nlevels <= 0 || nlevels > 64 ||
        (I.K > 0 && (!ep || !F12 || (n1 > 0 && (!match12 || !kps1 || !desc1 || !elig1)) || (nn1 > 0 && (!nodes1 || !node_off1 || !idx1)))))
        return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    return search_tri_common(c, what, kps1, n1, desc1, stride1, elig1, nodes1, node_off1, idx1, nn1, set, I, ep, F12, scale2, sigma2_2,
                                   nullptr, nlevels, bCoarse, checkOri, nullptr, nullptr, nullptr, match12, nmatches);
}

int eorb_search_for_triangulation_kb8_keyframes(eorb_ctx* c,
        const eorb_keypoint* kps1, int n1, int nleft1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_kf_set* set, const int32_t* nleft2,
        const eorb_camera* cam1, const eorb_camera* cam2, const float* Rt, const float* ep,
        const float* scale2, const float* sigma2_1, const float* sigma2_2, int nlevels,
        int bCoarse, int checkOri, int32_t* match12, int32_t* nmatches)
{
    if (!c) return EORB_E_ARG;
    const char* what = "search_for_triangulation_kb8_keyframes";
    KfSetIn I;
    int rc;
    if ((rc = I.check(c, what, set, n1))) return rc;
    if (nn1 < 0 || stride1 < 32 || !cam1 || !cam2 || !scale2 || !sigma2_1 || !sigma2_2 || nlevels <= 0 || nlevels > 64 || nleft1 < -1 || nleft1 > n1 ||
        (I.K > 0 && (!ep || !Rt || !nleft2 || (n1 > 0 && (!match12 || !kps1 || !desc1 || !elig1)) || (nn1 > 0 && (!nodes1 || !node_off1 || !idx1)))))
        return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    for (int k = 0; k < I.K; k++)
        if (nleft2[k] < -1 || nleft2[k] > I.sl[k].nrows) return set_err(c, EORB_E_ARG, "%s: keyframe %d: nleft2 %d", what, k, nleft2[k]);
    fe_enter(c);
    kfbatch_clear(I.K, n1, match12, nmatches);
    const bool twocam = nleft1 >= 0;
    for (int k = 0; k < I.K; k++)
        if (twocam != (nleft2[k] >= 0))       // the reference leaves R12 an empty cv::Mat (:1000-1014)
            return set_err(c, EORB_E_CONFIG, "%s: keyframe %d: one keyframe of the pair has two cameras and the other one", what, k);
    TriKbArgs KA{};
    if ((rc = kb8_cameras(c, what, nleft1, cam1, cam2, KA))) return rc;
    return search_tri_common(c, what, kps1, n1, desc1, stride1, elig1, nodes1, node_off1, idx1, nn1, set, I, ep, nullptr, scale2, sigma2_2,
                                   sigma2_1, nlevels, bCoarse, checkOri, &KA, nleft2, Rt, match12, nmatches);
}

// ---- CreateNewMapPoints: the stage alone, and behind either K-keyframe search ----
int eorb_new_map_points(eorb_ctx* c, const eorb_keypoint* kps1, int n1, const eorb_keypoint* kps2, const int32_t* kf_off, int K,
                        const int32_t* match12, const eorb_newpts_params* params, const eorb_newpts_out* out)
{
    if (!c) return EORB_E_ARG;
    const char* what = "new_map_points";
    if (K < 0 || n1 < 0 || (K > 0 && !kf_off)) return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    if (K > kKfBatchMaxKfs || (int64_t)K * n1 > kKfBatchMaxOut)                          // (sizes only: nothing is read before this)
        return set_err(c, EORB_E_CAPACITY, "%s: %d keyframes x %d outputs exceed %d keyframes or %lld outputs", what, K, n1, kKfBatchMaxKfs, (long long)kKfBatchMaxOut);
    if (K > 0) {
        if (kf_off[0] != 0) return set_err(c, EORB_E_ARG, "%s: kf_off[0] = %d", what, kf_off[0]);
        for (int k = 0; k < K; k++) if (kf_off[k + 1] < kf_off[k]) return set_err(c, EORB_E_ARG, "%s: kf_off decreases at keyframe %d", what, k);
        if (kf_off[K] > kKfBatchMaxRows) return set_err(c, EORB_E_CAPACITY, "%s: %d rows exceed %lld", what, kf_off[K], (long long)kKfBatchMaxRows);
    }
    NpJob J;
    int rc;
    if ((rc = J.check(c, what, kps1, n1, kps2, kf_off, K, params, out))) return rc;
    if (K > 0 && n1 > 0 && !match12) return set_err(c, EORB_E_ARG, "%s: match12 is required", what);
    for (int k = 0; k < K; k++)
        for (int i = 0; i < n1; i++) {
            const int32_t m = match12[(size_t)k * n1 + i];
            if (m < -1 || m >= J.kf[k].nrows) return set_err(c, EORB_E_ARG, "%s: keyframe %d: match12[%d] = %d outside [-1, %d)", what, k, i, m, J.kf[k].nrows);
        }
    fe_enter(c);
    np_clear(K, n1, out);
    if (K == 0 || n1 == 0) return EORB_OK;
    Arena A(c);
    const size_t o_k1 = A.in(kps1, sizeof(eorb_keypoint) * (size_t)n1), o_k2 = A.in(kps2, sizeof(eorb_keypoint) * (size_t)J.ntotal);
    const size_t o_m = A.in(match12, sizeof(int32_t) * (size_t)K * n1);
    J.queue(A);
    J.reserve(A);
    if ((rc = A.upload())) return rc;
    if ((rc = J.launch(c, A, A.dev<eorb_keypoint>(o_k1), A.dev<eorb_keypoint>(o_k2), A.dev<int32_t>(o_m)))) return rc;
    return A.fetch();
}

int eorb_create_new_map_points(eorb_ctx* c,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_kf_set* set, const float* ep, const float* F12, const float* scale2, const float* sigma2_2, int nlevels,
        int bCoarse, int checkOri, int32_t* match12, int32_t* nmatches,
        const eorb_newpts_params* params, const eorb_newpts_out* out)
{
    if (!c) return EORB_E_ARG;
    const char* what = "create_new_map_points";
    KfSetIn I;
    int rc;
    if ((rc = I.check(c, what, set, n1))) return rc;
    if (nn1 < 0 || stride1 < 32 || !scale2 || !sigma2_2 || nlevels <= 0 || nlevels > 64 ||
        (I.K > 0 && (!ep || !F12 || (n1 > 0 && (!match12 || !kps1 || !desc1 || !elig1)) || (nn1 > 0 && (!nodes1 || !node_off1 || !idx1)))))
        return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    NpJob J;
    if ((rc = J.check(c, what, kps1, n1, set->kps, set->kf_off, I.K, params, out))) return rc;
    return search_tri_common(c, what, kps1, n1, desc1, stride1, elig1, nodes1, node_off1, idx1, nn1, set, I, ep, F12, scale2, sigma2_2,
                             nullptr, nlevels, bCoarse, checkOri, nullptr, nullptr, nullptr, match12, nmatches, &J);
}

int eorb_create_new_map_points_kb8(eorb_ctx* c,
        const eorb_keypoint* kps1, int n1, int nleft1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_kf_set* set, const int32_t* nleft2,
        const eorb_camera* cam1, const eorb_camera* cam2, const float* Rt, const float* ep,
        const float* scale2, const float* sigma2_1, const float* sigma2_2, int nlevels,
        int bCoarse, int checkOri, int32_t* match12, int32_t* nmatches,
        const eorb_newpts_params* params, const eorb_newpts_out* out)
{
    if (!c) return EORB_E_ARG;
    const char* what = "create_new_map_points_kb8";
    KfSetIn I;
    int rc;
    if ((rc = I.check(c, what, set, n1))) return rc;
    if (nn1 < 0 || stride1 < 32 || !cam1 || !cam2 || !scale2 || !sigma2_1 || !sigma2_2 || nlevels <= 0 || nlevels > 64 || nleft1 < -1 || nleft1 > n1 ||
        (I.K > 0 && (!ep || !Rt || !nleft2 || (n1 > 0 && (!match12 || !kps1 || !desc1 || !elig1)) || (nn1 > 0 && (!nodes1 || !node_off1 || !idx1)))))
        return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    for (int k = 0; k < I.K; k++)
        if (nleft2[k] < -1 || nleft2[k] > I.sl[k].nrows) return set_err(c, EORB_E_ARG, "%s: keyframe %d: nleft2 %d", what, k, nleft2[k]);
    fe_enter(c);
    kfbatch_clear(I.K, n1, match12, nmatches);
    np_clear(I.K, n1, out);
    const bool twocam = nleft1 >= 0;
    for (int k = 0; k < I.K; k++)
        if (twocam != (nleft2[k] >= 0))       // the reference leaves R12 an empty cv::Mat (:1000-1014)
            return set_err(c, EORB_E_CONFIG, "%s: keyframe %d: one keyframe of the pair has two cameras and the other one", what, k);
    TriKbArgs KA{};
    if ((rc = kb8_cameras(c, what, nleft1, cam1, cam2, KA))) return rc;
    NpJob J;
    if ((rc = J.check(c, what, kps1, n1, set->kps, set->kf_off, I.K, params, out))) return rc;
    if (params->nleft1 != nleft1) return set_err(c, EORB_E_ARG, "%s: params->nleft1 %d is not the search's %d", what, params->nleft1, nleft1);
    for (int k = 0; k < I.K; k++)
        if (J.kf[k].nleft2 != nleft2[k]) return set_err(c, EORB_E_ARG, "%s: keyframe %d: params->nleft2 %d is not the search's %d", what, k, J.kf[k].nleft2, nleft2[k]);
    return search_tri_common(c, what, kps1, n1, desc1, stride1, elig1, nodes1, node_off1, idx1, nn1, set, I, ep, nullptr, scale2, sigma2_2,
                             sigma2_1, nlevels, bCoarse, checkOri, &KA, nleft2, Rt, match12, nmatches, &J);
}

// SearchByBoW over the K keyframes of a set.  kf_kf = 0: the set is the KeyFrame side, `one` the frame (flag1 unused; nL >= 0: a
// two-camera frame of nL left features, then right ones); kf_kf = 1: `one` is pKF1 with flag1 = has_mp1, the set is side 2.  Row k has
// n1 entries either way.  what: the entry point in messages, prof: its profile scope
static int bow_common(eorb_ctx* c, const char* what, const char* prof, int kf_kf, const eorb_kf_set* S,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, const uint8_t* flag1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        int32_t* out, float nnratio, int checkOri, int32_t* nmatches, int nL = -1)
{
    if (!c) return EORB_E_ARG;
    KfSetIn I;
    int rc;
    if ((rc = I.check(c, what, S, n1))) return rc;
    const int K = I.K;
    if (nn1 < 0 || (K > 0 && ((n1 > 0 && (!out || !kps1 || !desc1 || (kf_kf && !flag1))) || (nn1 > 0 && (!nodes1 || !node_off1 || !idx1)))))
        return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    fe_enter(c);
    kfbatch_clear(K, n1, out, nmatches);
    if (K == 0 || n1 == 0 || nn1 == 0 || I.ntotal == 0 || I.max_nn == 0) return EORB_OK;
    if ((rc = fv_check(c, what, kf_kf ? "pKF1" : "frame", -1, node_off1, idx1, nn1, n1))) return rc;
    Arena A(c);
    FvIn f1;
    f1.queue(A, nodes1, node_off1, idx1, nn1);
    const size_t o_k1 = A.in(kps1, sizeof(eorb_keypoint) * n1), o_d1 = A.in(desc1, 32 * (size_t)n1);
    const size_t o_f1 = kf_kf ? A.in(flag1, n1) : 0;
    I.queue(A, S, true);
    const KfBatchOut o = kfbatch_reserve(A, K, n1, out, nmatches);
    const int nscratch = kf_kf ? I.ntotal : 0;                          // vbMatched2 of every pair
    const size_t o_scr = A.reserve(sizeof(int32_t) * (size_t)nscratch);
    if ((rc = A.upload())) return rc;
    const eorb_keypoint* sk = A.dev<eorb_keypoint>(I.o_kps); const uint8_t* sd = A.dev<uint8_t>(I.o_desc); const uint8_t* sf = A.dev<uint8_t>(I.o_flag);
    const eorb_keypoint* k1 = A.dev<eorb_keypoint>(o_k1); const uint8_t* d1 = A.dev<uint8_t>(o_d1);
    int32_t* hist = A.dev<int32_t>(o.o_hist); int32_t* m = A.dev<int32_t>(o.o_m); int32_t* scr = A.dev<int32_t>(o_scr);
    BowBatchArgs B{};
    if (kf_kf) B.A = BowArgs{k1, d1, A.dev<uint8_t>(o_f1), f1.fv(A), sk, 0, sd, I.fv(A), scr, A.dev<int8_t>(o.o_bin), hist, hist + 32, nnratio, checkOri, 1, sf, m, n1};
    else B.A = BowArgs{sk, sd, sf, I.fv(A), k1, n1, d1, f1.fv(A), m, A.dev<int8_t>(o.o_bin), hist, hist + 32, nnratio, checkOri, 0, sf, nullptr, 0};
    B.kf = A.dev<KfSlice>(I.o_sl); B.K = K; B.n_out = n1; B.max_nn = kf_kf ? nn1 : I.max_nn;
    if ((rc = search_bow_batch_dev(c, prof, B, kf_kf ? scr : nullptr, nscratch, nL))) return rc;
    return kfbatch_out(A, o, K, nmatches);
}

int eorb_search_by_bow_keyframes(eorb_ctx* c, const eorb_kf_set* set,
        const eorb_keypoint* f_kps, int n_f, const uint8_t* f_desc,
        const uint32_t* f_nodes, const int32_t* f_node_off, const int32_t* f_idx, int f_nn,
        int32_t* match_f, float nnratio, int checkOri, int32_t* nmatches)
{
    return bow_common(c, "search_by_bow_keyframes", "search_by_bow_keyframes", 0, set, f_kps, n_f, f_desc, nullptr, f_nodes, f_node_off, f_idx, f_nn, match_f, nnratio,
                            checkOri, nmatches);
}

int eorb_search_by_bow_kf_keyframes(eorb_ctx* c,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, const uint8_t* has_mp1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_kf_set* set, int32_t* match12, float nnratio, int checkOri, int32_t* nmatches)
{
    return bow_common(c, "search_by_bow_kf_keyframes", "search_by_bow_kf_keyframes", 1, set, kps1, n1, desc1, has_mp1, nodes1, node_off1, idx1, nn1, match12, nnratio,
                            checkOri, nmatches);
}

// ---- the single-pair forms: the other keyframe (or the KeyFrame of SearchByBoW(pKF, F)) as a set of one ----
int eorb_search_for_triangulation(eorb_ctx* c,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_keypoint* kps2, int n2, const uint8_t* desc2, int stride2, const uint8_t* elig2,
        const uint32_t* nodes2, const int32_t* node_off2, const int32_t* idx2, int nn2,
        const float* ep, const float* F12, const float* scale2, const float* sigma2_2, int nlevels,
        int bCoarse, int checkOri, int32_t* match12, int* nmatches)
{
    if (!c) return EORB_E_ARG;
    const char* what = "search_for_triangulation";
    if (n1 < 0 || n2 < 0 || nn1 < 0 || nn2 < 0 || !match12 || stride1 < 32 || stride2 < 32 || !ep || !F12 || !scale2 || !sigma2_2 ||
        nlevels <= 0 || nlevels > 64)
        return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    kfbatch_clear(1, n1, match12, nmatches);          // before any error that depends on what the arrays hold
    const KfSetOne two(kps2, n2, desc2, stride2, elig2, nodes2, node_off2, idx2, nn2);
    KfSetIn I;
    int rc;
    if ((rc = I.check(c, what, &two.S, n1))) return rc;
    return search_tri_common(c, what, kps1, n1, desc1, stride1, elig1, nodes1, node_off1, idx1, nn1, &two.S, I, ep, F12, scale2, sigma2_2,
                             nullptr, nlevels, bCoarse, checkOri, nullptr, nullptr, nullptr, match12, nmatches);
}

int eorb_search_for_triangulation_kb8(eorb_ctx* c,
        const eorb_keypoint* kps1, int n1, int nleft1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_keypoint* kps2, int n2, int nleft2, const uint8_t* desc2, int stride2, const uint8_t* elig2,
        const uint32_t* nodes2, const int32_t* node_off2, const int32_t* idx2, int nn2,
        const eorb_camera* cam1, const eorb_camera* cam2, const float* Rt, const float* ep,
        const float* scale2, const float* sigma2_1, const float* sigma2_2, int nlevels,
        int bCoarse, int checkOri, int32_t* match12, int* nmatches)
{
    if (!c) return EORB_E_ARG;
    const char* what = "search_for_triangulation_kb8";
    if (n1 < 0 || n2 < 0 || nn1 < 0 || nn2 < 0 || !match12 || stride1 < 32 || stride2 < 32 || !cam1 || !cam2 || !Rt || !ep ||
        !scale2 || !sigma2_1 || !sigma2_2 || nlevels <= 0 || nlevels > 64 || nleft1 < -1 || nleft2 < -1 || nleft1 > n1 || nleft2 > n2)
        return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    kfbatch_clear(1, n1, match12, nmatches);
    if ((nleft1 < 0) != (nleft2 < 0))      // the reference leaves R12 an empty cv::Mat (:1000-1014)
        return set_err(c, EORB_E_CONFIG, "%s: one keyframe has two cameras and the other one", what);
    TriKbArgs KA{};
    int rc;
    if ((rc = kb8_cameras(c, what, nleft1, cam1, cam2, KA))) return rc;
    const KfSetOne two(kps2, n2, desc2, stride2, elig2, nodes2, node_off2, idx2, nn2);
    KfSetIn I;
    if ((rc = I.check(c, what, &two.S, n1))) return rc;
    return search_tri_common(c, what, kps1, n1, desc1, stride1, elig1, nodes1, node_off1, idx1, nn1, &two.S, I, ep, nullptr, scale2, sigma2_2,
                             sigma2_1, nlevels, bCoarse, checkOri, &KA, &nleft2, Rt, match12, nmatches);
}

// SearchByBoW(pKF, F) (kf_kf = 0: the set is the KeyFrame) and SearchByBoW(pKF1, pKF2) (kf_kf = 1: the set is pKF2)
static int bow_single(eorb_ctx* c, const char* what, const char* prof, int kf_kf,
        const eorb_keypoint* s_kps, int s_n, const uint8_t* s_desc, const uint8_t* s_flag,
        const uint32_t* s_nodes, const int32_t* s_node_off, const int32_t* s_idx, int s_nn,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, const uint8_t* flag1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        int32_t* out, float nnratio, int checkOri, int* nmatches, int nL = -1)
{
    if (!c) return EORB_E_ARG;
    if (s_n < 0 || n1 < 0 || s_nn < 0 || nn1 < 0 || !out) return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    kfbatch_clear(1, n1, out, nmatches);              // before any error that depends on what the arrays hold
    const KfSetOne one(s_kps, s_n, s_desc, 32, s_flag, s_nodes, s_node_off, s_idx, s_nn);
    return bow_common(c, what, prof, kf_kf, &one.S, kps1, n1, desc1, flag1, nodes1, node_off1, idx1, nn1, out, nnratio, checkOri, nmatches, nL);
}

int eorb_search_by_bow(eorb_ctx* c,
        const eorb_keypoint* kf_kps, int n_kf, const uint8_t* kf_desc, const uint8_t* kf_has_mp,
        const uint32_t* kf_nodes, const int32_t* kf_node_off, const int32_t* kf_idx, int kf_nn,
        const eorb_keypoint* f_kps, int n_f, const uint8_t* f_desc,
        const uint32_t* f_nodes, const int32_t* f_node_off, const int32_t* f_idx, int f_nn,
        int32_t* match_f, float nnratio, int checkOri, int* nmatches)
{
    return bow_single(c, "search_by_bow", "search_bow", 0, kf_kps, n_kf, kf_desc, kf_has_mp, kf_nodes, kf_node_off, kf_idx, kf_nn,
                      f_kps, n_f, f_desc, nullptr, f_nodes, f_node_off, f_idx, f_nn, match_f, nnratio, checkOri, nmatches);
}

int eorb_search_by_bow_kf(eorb_ctx* c,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, const uint8_t* has_mp1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_keypoint* kps2, int n2, const uint8_t* desc2, const uint8_t* has_mp2,
        const uint32_t* nodes2, const int32_t* node_off2, const int32_t* idx2, int nn2,
        int32_t* match12, float nnratio, int checkOri, int* nmatches)
{
    if (c && !has_mp2 && n2 > 0) return set_err(c, EORB_E_ARG, "search_by_bow_kf: has_mp2 is required");
    return bow_single(c, "search_by_bow_kf", "search_bow", 1, kps2, n2, desc2, has_mp2, nodes2, node_off2, idx2, nn2,
                      kps1, n1, desc1, has_mp1, nodes1, node_off1, idx1, nn1, match12, nnratio, checkOri, nmatches);
}

int eorb_search_by_bow_fisheye(eorb_ctx* c,
        const eorb_keypoint* kf_kps, int n_kf, const uint8_t* kf_desc, const uint8_t* kf_has_mp,
        const uint32_t* kf_nodes, const int32_t* kf_node_off, const int32_t* kf_idx, int kf_nn,
        const eorb_keypoint* f_kps, int n_f, int nL, const uint8_t* f_desc,
        const uint32_t* f_nodes, const int32_t* f_node_off, const int32_t* f_idx, int f_nn,
        int32_t* match_f, float nnratio, int checkOri, int* nmatches)
{
    if (c && (nL < 0 || nL > n_f)) return set_err(c, EORB_E_ARG, "search_by_bow_fisheye: nL %d of %d frame features", nL, n_f);
    return bow_single(c, "search_by_bow_fisheye", "search_bow_fisheye", 0, kf_kps, n_kf, kf_desc, kf_has_mp, kf_nodes, kf_node_off, kf_idx, kf_nn,
                      f_kps, n_f, f_desc, nullptr, f_nodes, f_node_off, f_idx, f_nn, match_f, nnratio, checkOri, nmatches, nL);
}

int eorb_kb8_triangulate_matches(eorb_ctx* c, const eorb_camera* cam1, const eorb_camera* cam2, const float* Rt,
        const eorb_keypoint* kps1, const eorb_keypoint* kps2, int n, const float* sigma2_1, const float* sigma2_2, int nlevels,
        float* z1)
{
    if (!c) return EORB_E_ARG;
    if (!cam1 || !cam2 || !Rt || n < 0 || (n > 0 && (!kps1 || !kps2 || !z1)) || !sigma2_1 || !sigma2_2 || nlevels <= 0 || nlevels > 64)
        return set_err(c, EORB_E_ARG, "kb8_triangulate_matches: bad arguments");
    if (cam1->model != 1 || (cam2->model != 0 && cam2->model != 1))
        return set_err(c, EORB_E_CONFIG, "kb8_triangulate_matches: camera 1 must be KannalaBrandt8, camera 2 Pinhole or KannalaBrandt8");
    fe_enter(c);
    if (n == 0) return EORB_OK;
    for (int i = 0; i < n; i++)
        if (kps1[i].octave < 0 || kps1[i].octave >= nlevels || kps2[i].octave < 0 || kps2[i].octave >= nlevels)
            return set_err(c, EORB_E_ARG, "kb8_triangulate_matches: pair %d has an octave outside [0,%d)", i, nlevels);
    int rc;
    Arena A(c);
    const size_t o_k1 = A.in(kps1, sizeof(eorb_keypoint) * (size_t)n), o_k2 = A.in(kps2, sizeof(eorb_keypoint) * (size_t)n);
    const size_t o_s1 = A.in(sigma2_1, sizeof(float) * nlevels), o_s2 = A.in(sigma2_2, sizeof(float) * nlevels);
    const size_t o_z = A.reserve(sizeof(float) * (size_t)n);
    if ((rc = A.upload())) return rc;
    if ((rc = kb8_tri_batch_dev(c, cam1, cam2, Rt, A.dev<eorb_keypoint>(o_k1), A.dev<eorb_keypoint>(o_k2), n, A.dev<float>(o_s1),
                                A.dev<float>(o_s2), A.dev<float>(o_z))))
        return rc;
    return A.download_to(z1, o_z, sizeof(float) * (size_t)n);
}

// the (x, y) of n keypoints, packed for the arena
static std::vector<float> tv_points(const eorb_keypoint* kps, int n)
{
    std::vector<float> p(2 * (size_t)n);
    for (int i = 0; i < n; i++) { p[2 * (size_t)i] = kps[i].x; p[2 * (size_t)i + 1] = kps[i].y; }
    return p;
}
// sizes first (nothing is read), then the match indices against the key arrays
static int tv_check_sizes(eorb_ctx* c, const char* what, int n1, int n2, int N)
{
    if (n1 > EORB_TVR_MAX_KEYS || n2 > EORB_TVR_MAX_KEYS) return set_err(c, EORB_E_CAPACITY, "%s: %d / %d keys, at most EORB_TVR_MAX_KEYS = %d", what, n1, n2, EORB_TVR_MAX_KEYS);
    if (N > EORB_TVR_MAX_MATCHES) return set_err(c, EORB_E_CAPACITY, "%s: %d matches, at most EORB_TVR_MAX_MATCHES = %d", what, N, EORB_TVR_MAX_MATCHES);
    return EORB_OK;
}
static int tv_check_matches(eorb_ctx* c, const char* what, const int32_t* match12, int N, int n1, int n2)
{
    for (int i = 0; i < N; i++)
        if (match12[2 * i] < 0 || match12[2 * i] >= n1 || match12[2 * i + 1] < 0 || match12[2 * i + 1] >= n2)
            return set_err(c, EORB_E_ARG, "%s: match %d = (%d, %d) is outside the %d / %d keys", what, i, match12[2 * i], match12[2 * i + 1], n1, n2);
    return EORB_OK;
}
static int tv_check_sets(eorb_ctx* c, const char* what, const int32_t* sets, int iters, int N)
{
    for (int i = 0; i < 8 * iters; i++)
        if (sets[i] < 0 || sets[i] >= N) return set_err(c, EORB_E_ARG, "%s: set %d holds the index %d of %d matches", what, i / 8, sets[i], N);
    return EORB_OK;
}
// vP3D / vbGood / vbTriangulated are indexed by `first`: with one first index in two matches their values would depend on the order of the writes
static int tv_check_first_once(eorb_ctx* c, const char* what, const int32_t* match12, int N, int n1)
{
    std::vector<uint8_t> seen((size_t)n1, 0);
    for (int i = 0; i < N; i++) {
        if (seen[match12[2 * i]]) return set_err(c, EORB_E_ARG, "%s: two matches have the first index %d", what, match12[2 * i]);
        seen[match12[2 * i]] = 1;
    }
    return EORB_OK;
}

// the H / F RANSAC as a part of a call (eorb_two_view_ransac, and the first stage of eorb_two_view_reconstruct): its inputs, its own space
// and its results: the 22 words | inliers_h | inliers_f | the per-iteration aids.  dst: who takes the arrays (any may be NULL); the 22
// words are read through the host view (tv_ransac_reserve's want: only when the caller takes them)
struct TvRansacDst { uint8_t* inliers_h; uint8_t* inliers_f; float* it_score_h; float* it_score_f; float* it_H; float* it_F; };
struct TvRansacOff { size_t p1, p2, m, s, n1, n2, hdr, hyp, inl, res, ih, inf, sh, sf, ith, itf; };
static TvRansacOff tv_ransac_reserve(Arena& A, const std::vector<float>& p1, const std::vector<float>& p2, const int32_t* match12, int N, const int32_t* sets,
                                     int iters, bool words, const TvRansacDst& d)
{
    const size_t sN = (size_t)N, sI = (size_t)iters;
    TvRansacOff o;
    o.p1 = A.in(p1.data(), sizeof(float) * p1.size()); o.p2 = A.in(p2.data(), sizeof(float) * p2.size());
    o.m = A.in(match12, sizeof(int32_t) * 2 * sN); o.s = A.in(sets, sizeof(int32_t) * 8 * sI);
    o.n1 = A.reserve(sizeof(float) * p1.size()); o.n2 = A.reserve(sizeof(float) * p2.size());
    o.hdr = A.reserve(sizeof(float) * kTvHdrFloats); o.hyp = A.reserve(sizeof(float) * kTvHypFloats * 2 * sI); o.inl = A.reserve(2 * sI * sN);
    o.res = A.out(nullptr, sizeof(float) * 22); o.ih = A.out(d.inliers_h, sN); o.inf = A.out(d.inliers_f, sN);
    o.sh = A.out(d.it_score_h, sizeof(float) * sI); o.sf = A.out(d.it_score_f, sizeof(float) * sI);
    o.ith = A.out(d.it_H, sizeof(float) * 9 * sI); o.itf = A.out(d.it_F, sizeof(float) * 9 * sI);
    if (words) A.want(o.res, sizeof(float) * 22);
    return o;
}
static TvRansacArgs tv_ransac_args(const Arena& A, const TvRansacOff& o, int n1, int n2, int N, int iters, float sigma, float th_score, float th_f)
{
    TvRansacArgs T{};
    T.pts1 = A.dev<float2>(o.p1); T.pts2 = A.dev<float2>(o.p2); T.n1 = n1; T.n2 = n2;
    T.match12 = A.dev<int32_t>(o.m); T.N = N; T.sets = A.dev<int32_t>(o.s); T.iters = iters;
    T.sigma = sigma; T.th_score = th_score; T.th_f = th_f;
    T.pn1 = A.dev<float2>(o.n1); T.pn2 = A.dev<float2>(o.n2); T.hdr = A.dev<float>(o.hdr); T.hyp = A.dev<float>(o.hyp); T.inl = A.dev<uint8_t>(o.inl);
    T.res = A.dev<float>(o.res); T.inliers_h = A.dev<uint8_t>(o.ih); T.inliers_f = A.dev<uint8_t>(o.inf);
    T.it_score_h = A.dev<float>(o.sh); T.it_score_f = A.dev<float>(o.sf); T.it_H = A.dev<float>(o.ith); T.it_F = A.dev<float>(o.itf);
    return T;
}

int eorb_two_view_ransac(eorb_ctx* c, const eorb_keypoint* kps1, int n1, const eorb_keypoint* kps2, int n2, const int32_t* match12, int N,
        const int32_t* sets, int iters, const eorb_tvr_params* params,
        float* H21, float* SH, int32_t* best_it_h, uint8_t* inliers_h, float* F21, float* SF, int32_t* best_it_f, uint8_t* inliers_f,
        float* it_score_h, float* it_score_f, float* it_H, float* it_F)
{
    if (!c) return EORB_E_ARG;
    const char* what = "two_view_ransac";
    if (!kps1 || !kps2 || !match12 || !sets || !params || n1 < 0 || n2 < 0 || !H21 || !SH || !best_it_h || !inliers_h || !F21 || !SF ||
        !best_it_f || !inliers_f)
        return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    if (N < 8 || iters < 1) return set_err(c, EORB_E_ARG, "%s: %d matches (at least 8), %d iterations (at least 1)", what, N, iters);
    int rc;
    if ((rc = tv_check_sizes(c, what, n1, n2, N))) return rc;
    if (iters > EORB_TVR_MAX_ITERS) return set_err(c, EORB_E_CAPACITY, "%s: %d iterations, at most EORB_TVR_MAX_ITERS = %d", what, iters, EORB_TVR_MAX_ITERS);
    if ((rc = tv_check_matches(c, what, match12, N, n1, n2))) return rc;
    if ((rc = tv_check_sets(c, what, sets, iters, N))) return rc;
    fe_enter(c);
    const std::vector<float> p1 = tv_points(kps1, n1), p2 = tv_points(kps2, n2);
    Arena A(c);
    const TvRansacOff o = tv_ransac_reserve(A, p1, p2, match12, N, sets, iters, true, TvRansacDst{inliers_h, inliers_f, it_score_h, it_score_f, it_H, it_F});
    if ((rc = A.upload())) return rc;
    if ((rc = twoview_ransac_dev(c, tv_ransac_args(A, o, n1, n2, N, iters, params->sigma, params->th_score, params->th_f)))) return rc;
    const char* h;
    if ((rc = A.fetch(&h))) return rc;
    const float* r = (const float*)(h + o.res);
    *SH = r[0]; *SF = r[1];
    memcpy(best_it_h, r + 2, sizeof(int32_t)); memcpy(best_it_f, r + 3, sizeof(int32_t));
    memcpy(H21, r + 4, sizeof(float) * 9); memcpy(F21, r + 13, sizeof(float) * 9);
    return EORB_OK;
}

int eorb_two_view_check_rt(eorb_ctx* c, const eorb_keypoint* kps1, int n1, const eorb_keypoint* kps2, int n2, const int32_t* match12, int N,
        const uint8_t* inliers, const float* K, float th2, float min_parallax_crt, int min_triangulated,
        const eorb_tvr_pose* poses, int Kp, int32_t* n_good, uint8_t* good, float* p3d, float* cos_sel, float* cos_all)
{
    if (!c) return EORB_E_ARG;
    const char* what = "two_view_check_rt";
    if (!kps1 || !kps2 || !match12 || !inliers || !K || !poses || n1 < 1 || n2 < 1 || N < 1 || Kp < 1 || min_triangulated < 0 || !n_good || !good ||
        !p3d || !cos_sel)
        return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    int rc;
    if ((rc = tv_check_sizes(c, what, n1, n2, N))) return rc;
    if (Kp > EORB_TVR_MAX_POSES) return set_err(c, EORB_E_CAPACITY, "%s: %d poses, at most EORB_TVR_MAX_POSES = %d", what, Kp, EORB_TVR_MAX_POSES);
    if ((rc = tv_check_matches(c, what, match12, N, n1, n2))) return rc;
    if ((rc = tv_check_first_once(c, what, match12, N, n1))) return rc;
    fe_enter(c);
    const std::vector<float> p1 = tv_points(kps1, n1), p2 = tv_points(kps2, n2);
    const size_t sN = (size_t)N, sK = (size_t)Kp, s1 = (size_t)n1;
    Arena A(c);
    const size_t o_p1 = A.in(p1.data(), sizeof(float) * p1.size()), o_p2 = A.in(p2.data(), sizeof(float) * p2.size());
    const size_t o_m = A.in(match12, sizeof(int32_t) * 2 * sN), o_in = A.in(inliers, sN), o_po = A.in(poses, sizeof(eorb_tvr_pose) * sK);
    // results: n_good | cos_sel | good | p3d | cos_all
    const size_t o_ng = A.out(n_good, sizeof(int32_t) * sK), o_cs = A.out(cos_sel, sizeof(float) * sK), o_g = A.out(good, sK * s1);
    const size_t o_p3 = A.out(p3d, sizeof(float) * 3 * sK * s1), o_ca = A.out(cos_all, sizeof(float) * sK * sN);
    if ((rc = A.upload())) return rc;
    EORB_HIP(c, hipMemsetAsync(A.dev<char>(o_g), 0, o_ca - o_g, c->stream));
    TvCheckRtArgs T{};
    T.pts1 = A.dev<float2>(o_p1); T.pts2 = A.dev<float2>(o_p2); T.n1 = n1; T.match12 = A.dev<int32_t>(o_m); T.N = N; T.inliers = A.dev<uint8_t>(o_in);
    memcpy(T.K, K, sizeof T.K); T.th2 = th2; T.min_parallax_crt = min_parallax_crt; T.min_triangulated = min_triangulated;
    T.poses = A.dev<float>(o_po); T.Kp = Kp;
    T.n_good = A.dev<int32_t>(o_ng); T.cos_sel = A.dev<float>(o_cs); T.good = A.dev<uint8_t>(o_g); T.p3d = A.dev<float>(o_p3); T.cos_all = A.dev<float>(o_ca);
    if ((rc = twoview_check_rt_dev(c, T))) return rc;
    return A.fetch();
}

int eorb_two_view_reconstruct(eorb_ctx* c, const eorb_keypoint* kps1, int n1, const eorb_keypoint* kps2, int n2,
        const int32_t* match12, int N, const int32_t* sets, int iters, const float* K, const eorb_tvr_recon_params* p,
        eorb_tvr_recon_result* res, float* R21, float* t21, float* p3d, uint8_t* triangulated, uint8_t* trans_inliers, eorb_tvr_pose* hyp_poses)
{
    if (!c) return EORB_E_ARG;
    const char* what = "two_view_reconstruct";
    if (!kps1 || !kps2 || !match12 || !sets || !K || !p || n1 < 1 || n2 < 1 || !res || !R21 || !t21 || !p3d || !triangulated || !trans_inliers)
        return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    if (N < 8 || iters < 1) return set_err(c, EORB_E_ARG, "%s: %d matches (at least 8), %d iterations (at least 1)", what, N, iters);
    if (p->min_triangulated < 0 || (p->form != EORB_TVR_FORM_STOCK && p->form != EORB_TVR_FORM_INFO))
        return set_err(c, EORB_E_ARG, "%s: min_triangulated %d, form %d", what, p->min_triangulated, p->form);
    int rc;
    if ((rc = tv_check_sizes(c, what, n1, n2, N))) return rc;
    if (iters > EORB_TVR_MAX_ITERS) return set_err(c, EORB_E_CAPACITY, "%s: %d iterations, at most EORB_TVR_MAX_ITERS = %d", what, iters, EORB_TVR_MAX_ITERS);
    if ((rc = tv_check_matches(c, what, match12, N, n1, n2))) return rc;
    if ((rc = tv_check_sets(c, what, sets, iters, N))) return rc;
    if ((rc = tv_check_first_once(c, what, match12, N, n1))) return rc;
    fe_enter(c);
    const std::vector<float> p1 = tv_points(kps1, n1), p2 = tv_points(kps2, n2);
    const size_t sN = (size_t)N, s1 = (size_t)n1;
    constexpr size_t kH = 8;                                       // CheckRT's launch: the 8 hypotheses of ReconstructH
    Arena A(c);
    const TvRansacOff o = tv_ransac_reserve(A, p1, p2, match12, N, sets, iters, false, TvRansacDst{});      // (its results stay on the device)
    const size_t o_sel = A.reserve(sN), o_ca = A.reserve(sizeof(float) * kH * sN);
    // zeroed, contiguous: the results that travel (res | R21 | t21 | trans_inliers | triangulated | p3d | hyp_poses), then CheckRT's for 8 poses
    const size_t o_res = A.out(res, sizeof(eorb_tvr_recon_result)), o_R = A.out(R21, sizeof(float) * 18), o_t = A.out(t21, sizeof(float) * 6);
    const size_t o_ti = A.out(trans_inliers, sN), o_tri = A.out(triangulated, 2 * s1), o_p3 = A.out(p3d, sizeof(float) * 6 * s1);
    const size_t o_po = A.out(hyp_poses, sizeof(eorb_tvr_pose) * kH), o_nh = A.reserve(sizeof(int32_t));
    const size_t o_ng = A.reserve(sizeof(int32_t) * kH), o_cs = A.reserve(sizeof(float) * kH), o_g = A.reserve(kH * s1);
    const size_t o_p8 = A.reserve(sizeof(float) * 3 * kH * s1), o_end = A.reserve(1);
    if ((rc = A.upload())) return rc;
    EORB_HIP(c, hipMemsetAsync(A.dev<char>(o_res), 0, o_end - o_res, c->stream));
    const TvRansacArgs T = tv_ransac_args(A, o, n1, n2, N, iters, p->sigma, p->th_score, p->th_f);
    TvReconArgs D{};
    D.rres = T.res; D.inliers_h = T.inliers_h; D.inliers_f = T.inliers_f; D.N = N; D.n1 = n1;
    memcpy(D.K, K, sizeof D.K); D.p = *p;
    D.res = A.dev<eorb_tvr_recon_result>(o_res); D.poses = A.dev<float>(o_po); D.n_hyp = A.dev<int32_t>(o_nh);
    D.sel_inl = A.dev<uint8_t>(o_sel); D.trans_inl = A.dev<uint8_t>(o_ti);
    D.n_good = A.dev<int32_t>(o_ng); D.cos_sel = A.dev<float>(o_cs); D.good8 = A.dev<uint8_t>(o_g); D.p3d8 = A.dev<float>(o_p8);
    D.R21 = A.dev<float>(o_R); D.t21 = A.dev<float>(o_t); D.tri = A.dev<uint8_t>(o_tri); D.p3d = A.dev<float>(o_p3);
    TvCheckRtArgs Q{};
    Q.pts1 = T.pts1; Q.pts2 = T.pts2; Q.n1 = n1; Q.match12 = T.match12; Q.N = N; Q.inliers = D.sel_inl;
    memcpy(Q.K, K, sizeof Q.K); Q.th2 = 4.0f * (p->sigma * p->sigma); Q.min_parallax_crt = p->min_parallax_crt; Q.min_triangulated = p->min_triangulated;
    Q.poses = D.poses; Q.Kp = (int)kH; Q.Kp_dev = D.n_hyp;
    Q.n_good = A.dev<int32_t>(o_ng); Q.cos_sel = A.dev<float>(o_cs); Q.good = A.dev<uint8_t>(o_g); Q.p3d = A.dev<float>(o_p8); Q.cos_all = A.dev<float>(o_ca);
    if ((rc = twoview_reconstruct_dev(c, T, D, Q))) return rc;
    return A.fetch();
}

int eorb_sim3_ransac(eorb_ctx* c, const eorb_sim3_problem* problems, int K, const float* Xw1, const float* Xw2,
        const float* sigma2_1, const float* sigma2_2, const int32_t* sets,
        eorb_sim3_result* results, uint8_t* inliers, int32_t* it_inliers, float* it_T12, float* it_T21, float* it_scale)
{
    if (!c) return EORB_E_ARG;
    static const RansacDesc D{"sim3_ransac", 3, 3, 0, RANSAC_LIMIT(EORB_S3_MAX_PROBLEMS), RANSAC_LIMIT(EORB_S3_MAX_CORR), RANSAC_LIMIT(EORB_S3_MAX_ITERS)};
    if (!problems || !Xw1 || !Xw2 || !sigma2_1 || !sigma2_2 || !sets || !results || !inliers) return set_err(c, EORB_E_ARG, "%s: bad arguments", D.what);
    std::vector<S3Prob> pv;
    RansacCall R;
    int rc = ransac_problems_in(c, D, problems, K, sets, pv, R,
        [](int, const eorb_sim3_problem& p, S3Prob& d) {
            d.fix_scale = p.fix_scale != 0;
            memcpy(d.Rt1, p.Rt1, sizeof d.Rt1); memcpy(d.Rt2, p.Rt2, sizeof d.Rt2);
            d.cam1 = warp_cam_of(p.cam1); d.cam2 = warp_cam_of(p.cam2);
            return EORB_OK;
        },
        [](const eorb_sim3_problem& p) { return cam_model_ok(p.cam1) && cam_model_ok(p.cam2); },
        [&](int k, const RansacProb& d) {
            for (int i = 0; i < d.N; i++) {
                const float s1 = sigma2_1[(size_t)d.corr_off + i], s2 = sigma2_2[(size_t)d.corr_off + i];
                if (!(s1 >= 0.f && s1 < 1e15f) || !(s2 >= 0.f && s2 < 1e15f))
                    return set_err(c, EORB_E_ARG, "%s: problem %d, correspondence %d has sigma2 = (%g, %g), outside [0, 1e15)", D.what, k, i, (double)s1, (double)s2);
            }
            return EORB_OK;
        });
    if (rc) return rc;
    fe_enter(c);
    const size_t tN = R.tN, tI = R.tI;
    Arena A(c);
    const size_t o_pr = A.in(pv.data(), sizeof(S3Prob) * (size_t)K);
    const size_t o_x1 = A.in(Xw1, sizeof(float) * 3 * tN), o_x2 = A.in(Xw2, sizeof(float) * 3 * tN);
    const size_t o_s1 = A.in(sigma2_1, sizeof(float) * tN), o_s2 = A.in(sigma2_2, sizeof(float) * tN), o_st = A.in(sets, sizeof(int32_t) * 3 * tI);
    const size_t o_c1 = A.reserve(sizeof(float) * 3 * tN), o_c2 = A.reserve(sizeof(float) * 3 * tN);
    const size_t o_p1 = A.reserve(sizeof(float) * 2 * tN), o_p2 = A.reserve(sizeof(float) * 2 * tN);
    const size_t o_b1 = A.reserve(sizeof(float) * tN), o_b2 = A.reserve(sizeof(float) * tN), o_hyp = A.reserve(sizeof(float) * kS3HypFloats * tI);
    static_assert(sizeof(eorb_sim3_result) == sizeof(int32_t) * kS3ResWords, "eorb_sim3_result is kS3ResWords words");
    R.results(A, results, sizeof(eorb_sim3_result) * (size_t)K, inliers);
    const size_t o_ii = A.out(it_inliers, sizeof(int32_t) * tI), o_is = A.out(it_scale, sizeof(float) * tI);
    const size_t o_t12 = A.out(it_T12, sizeof(float) * 16 * tI), o_t21 = A.out(it_T21, sizeof(float) * 16 * tI);
    if ((rc = R.upload(A))) return rc;
    S3Args T{};
    T.prob = A.dev<S3Prob>(o_pr); T.K = K; T.max_N = R.max_N; T.max_iters = R.max_iters;
    T.Xw1 = A.dev<float>(o_x1); T.Xw2 = A.dev<float>(o_x2); T.sigma2_1 = A.dev<float>(o_s1); T.sigma2_2 = A.dev<float>(o_s2); T.sets = A.dev<int32_t>(o_st);
    T.X1 = A.dev<float>(o_c1); T.X2 = A.dev<float>(o_c2); T.p1 = A.dev<float2>(o_p1); T.p2 = A.dev<float2>(o_p2);
    T.b1 = A.dev<float>(o_b1); T.b2 = A.dev<float>(o_b2); T.hyp = A.dev<float>(o_hyp);
    T.res = A.dev<int32_t>(R.res); T.inliers = A.dev<uint8_t>(R.inl); T.it_inliers = A.dev<int32_t>(o_ii); T.it_scale = A.dev<float>(o_is);
    T.it_T12 = A.dev<float>(o_t12); T.it_T21 = A.dev<float>(o_t21);
    if ((rc = sim3_ransac_dev(c, T))) return rc;
    return A.fetch();
}

int eorb_mlpnp_ransac(eorb_ctx* c, const eorb_mlpnp_problem* problems, int K, const float* p2d, const float* Xw, const float* sigma2,
        const int32_t* sets, eorb_mlpnp_result* results, uint8_t* inliers, int32_t* it_inliers, double* it_Rt, int32_t* it_refine_inliers)
{
    if (!c) return EORB_E_ARG;
    static const RansacDesc D{"mlpnp_ransac", 6, 6, 6, RANSAC_LIMIT(EORB_PNP_MAX_PROBLEMS), RANSAC_LIMIT(EORB_PNP_MAX_CORR), RANSAC_LIMIT(EORB_PNP_MAX_ITERS)};
    if (!problems || !p2d || !Xw || !sigma2 || !sets || !results || !inliers) return set_err(c, EORB_E_ARG, "%s: bad arguments", D.what);
    std::vector<PnpProb> pv;
    RansacCall R;
    int rc = ransac_problems_in(c, D, problems, K, sets, pv, R,
        [&](int k, const eorb_mlpnp_problem& p, PnpProb& d) {
            if (p.first_it < 0 || p.first_it >= p.iters || p.best_it < -1 || p.best_it >= p.first_it)
                return set_err(c, EORB_E_ARG, "%s: problem %d resumes at iteration %d of %d with the best %d (first_it in [0, iters), best_it in [-1, first_it))", D.what, k,
                               p.first_it, p.iters, p.best_it);
            d.first_it = p.first_it; d.best_it = p.best_it; d.th2 = p.th2; d.cam = warp_cam_of(p.cam);
            return EORB_OK;
        },
        [](const eorb_mlpnp_problem& p) { return cam_model_ok(p.cam); }, [](int, const RansacProb&) { return EORB_OK; });
    if (rc) return rc;
    fe_enter(c);
    const size_t tN = R.tN, tI = R.tI;
    Arena A(c);
    const size_t o_pr = A.in(pv.data(), sizeof(PnpProb) * (size_t)K);
    const size_t o_p2 = A.in(p2d, sizeof(float) * 2 * tN), o_xw = A.in(Xw, sizeof(float) * 3 * tN), o_sg = A.in(sigma2, sizeof(float) * tN);
    const size_t o_st = A.in(sets, sizeof(int32_t) * 6 * tI);
    const size_t o_f = A.reserve(sizeof(double) * 3 * tN), o_ns = A.reserve(sizeof(double) * 6 * tN), o_x = A.reserve(sizeof(double) * 3 * tN);
    const size_t o_bd = A.reserve(sizeof(float) * tN);
    static_assert(sizeof(eorb_mlpnp_result) == sizeof(int32_t) * kPnpResWords, "eorb_mlpnp_result is kPnpResWords words");
    R.results(A, results, sizeof(eorb_mlpnp_result) * (size_t)K, inliers);
    const size_t o_ii = A.out(it_inliers, sizeof(int32_t) * tI), o_ir = A.out(it_refine_inliers, sizeof(int32_t) * tI), o_rt = A.out(it_Rt, sizeof(double) * 12 * tI);
    if ((rc = R.upload(A))) return rc;
    PnpArgs T{};
    T.prob = A.dev<PnpProb>(o_pr); T.K = K; T.max_N = R.max_N; T.max_iters = R.max_iters;
    T.p2d = A.dev<float>(o_p2); T.Xw = A.dev<float>(o_xw); T.sigma2 = A.dev<float>(o_sg); T.sets = A.dev<int32_t>(o_st);
    T.f = A.dev<double>(o_f); T.ns = A.dev<double>(o_ns); T.X = A.dev<double>(o_x); T.bound = A.dev<float>(o_bd);
    T.res = A.dev<int32_t>(R.res); T.inliers = A.dev<uint8_t>(R.inl); T.it_inliers = A.dev<int32_t>(o_ii); T.it_refine = A.dev<int32_t>(o_ir);
    T.it_Rt = A.dev<double>(o_rt);
    if ((rc = mlpnp_ransac_dev(c, T))) return rc;
    return A.fetch();
}

// what the MixedMatcher forms take on top of the ORB ones (a NULL KfMixedIn* = an ORB entry point): kp_is_orb / kp_inv_sigma2 per
// keypoint, mp_is_orb per map point, each optional
struct KfMixedIn { const uint8_t* kp_is_orb; const float* kp_inv_sigma2; const uint8_t* mp_is_orb; };
struct KfMixedOff { size_t kio, sig, mio; };
static KfMixedOff kf_mixed_in(Arena& A, const KfMixedIn* mx, size_t n, size_t M)
{
    KfMixedOff o{};
    if (!mx) return o;
    o.kio = A.in(mx->kp_is_orb, mx->kp_is_orb ? n : 0);
    o.sig = A.in(mx->kp_inv_sigma2, mx->kp_inv_sigma2 ? sizeof(float) * n : 0);
    o.mio = A.in(mx->mp_is_orb, mx->mp_is_orb ? M : 0);
    return o;
}
static const uint8_t* kf_mixed_kp(const Arena& A, const KfMixedIn* mx, const KfMixedOff& o) { return mx && mx->kp_is_orb ? A.dev<uint8_t>(o.kio) : nullptr; }
static const float* kf_mixed_sigma(const Arena& A, const KfMixedIn* mx, const KfMixedOff& o) { return mx && mx->kp_inv_sigma2 ? A.dev<float>(o.sig) : nullptr; }
static const uint8_t* kf_mixed_mp(const Arena& A, const KfMixedIn* mx, const KfMixedOff& o) { return mx && mx->mp_is_orb ? A.dev<uint8_t>(o.mio) : nullptr; }

// ---- the searched side of the KeyFrame-side radius search (match.hip kf_radius_dev): the keypoints of K keyframes concatenated, keyframe k
// = rows kf_off[k] .. kf_off[k + 1] - 1 with grid bounds gb[k]; one keyframe is K = 1 with kf_off = {0, n} ----
struct KfSearched { size_t k, d, ur, off, g, tk, cell; int K, ntotal, stride; bool has_ur, has_tk; std::vector<GridB> gv; };
// its inputs; taken (the in-order form, in / out) comes last, so that a call's outputs can follow it.  kf_off stays the caller's until upload()
static void kf_searched_in(Arena& A, KfSearched& S, int K, const eorb_keypoint* kps, const uint8_t* desc, int stride, const float* uright,
                           const int32_t* kf_off, const eorb_grid_bounds* gb, const uint8_t* taken)
{
    const size_t n = (size_t)kf_off[K];
    S.K = K; S.ntotal = kf_off[K]; S.stride = stride; S.has_ur = uright != nullptr; S.has_tk = taken != nullptr;
    S.gv.resize(K);
    for (int k = 0; k < K; k++) S.gv[k] = grid_b(gb[k]);
    S.g = A.in(S.gv.data(), sizeof(GridB) * (size_t)K); S.off = A.in(kf_off, sizeof(int32_t) * ((size_t)K + 1));
    S.k = A.in(kps, sizeof(eorb_keypoint) * n); S.d = A.in(desc, (size_t)stride * n);
    S.ur = A.in(uright, uright ? sizeof(float) * n : 0);
    S.tk = A.in(taken, taken ? n : 0);
}
// the keypoints' cells: device only, behind the call's outputs
static void kf_searched_cells(Arena& A, KfSearched& S) { S.cell = A.reserve(sizeof(uint16_t) * (size_t)S.ntotal); }
// the block of the search: the searched side, the K * M queries Q (the projector's arrays or uploaded ones) and their descriptors
static RadBatchArgsMixed kf_searched_args(const Arena& A, const KfSearched& S, int M, const KfSideDev& Q, const uint8_t* d_q_desc, size_t q_desc_kstride,
                                          const float* d_inv_sigma2, int nlevels, float accept_thr, int32_t* d_best_idx, int32_t* d_best_dist,
                                          const KfMixedIn* mx, const KfMixedOff& mo)
{
    RadBatchArgsMixed B{};
    B.kps = A.dev<eorb_keypoint>(S.k); B.desc = A.dev<uint8_t>(S.d); B.stride = S.stride; B.cell = A.dev<uint16_t>(S.cell);
    B.uright = S.has_ur ? A.dev<float>(S.ur) : nullptr;
    B.kf_off = A.dev<int32_t>(S.off); B.g = A.dev<GridB>(S.g); B.K = S.K; B.M = M;
    B.valid = Q.valid; B.uv = (const float*)Q.uv; B.radius = Q.radius; B.level = Q.level; B.q_ur = Q.q_ur;
    B.q_desc = d_q_desc; B.q_desc_kstride = q_desc_kstride;
    B.inv_sigma2 = d_inv_sigma2; B.nlevels = nlevels;
    B.taken = S.has_tk ? A.dev<uint8_t>(S.tk) : nullptr; B.accept_thr = accept_thr;
    B.best_idx = d_best_idx; B.best_dist = d_best_dist;
    B.mp_is_orb = kf_mixed_mp(A, mx, mo); B.kp_inv_sigma2 = kf_mixed_sigma(A, mx, mo);
    return B;
}

static int kf_radius_common(eorb_ctx* c,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
        int M, const uint8_t* valid, const float* uv, const float* radius, const int32_t* level, const uint8_t* q_desc,
        const float* inv_sigma2, int nlevels, uint8_t* taken, float accept_thr, int32_t* best_idx, int32_t* best_dist,
        const float* uright, const float* q_ur, const KfMixedIn* mx = nullptr)
{
    if (!c) return EORB_E_ARG;
    const float* sigma = mx ? mx->kp_inv_sigma2 : inv_sigma2;
    if ((uright != nullptr) != (q_ur != nullptr) || (uright && !sigma)) return set_err(c, EORB_E_ARG, "kf_radius_match: the stereo gate needs uright, q_ur and inv_sigma2");
    if (n < 0 || M < 0 || stride < 32 || !gb || (M > 0 && (!valid || !uv || !radius || !level || !q_desc || !best_idx || !best_dist)) ||
        (inv_sigma2 && (nlevels <= 0 || nlevels > 64)))
        return set_err(c, EORB_E_ARG, "kf_radius_match: bad arguments");
    fe_enter(c);
    for (int m = 0; m < M; m++) { best_idx[m] = -1; best_dist[m] = 256; }
    if (M == 0 || n == 0) return EORB_OK;
    int rc;
    Arena A(c);
    const int32_t off[2] = {0, n};
    const size_t o_uv = A.in(uv, sizeof(float) * 2 * (size_t)M), o_rad = A.in(radius, sizeof(float) * M), o_lv = A.in(level, sizeof(int32_t) * M);
    const size_t o_va = A.in(valid, M), o_qd = A.in(q_desc, 32 * (size_t)M);
    const size_t o_is = A.in(inv_sigma2, inv_sigma2 ? sizeof(float) * nlevels : 0), o_qur = A.in(q_ur, q_ur ? sizeof(float) * M : 0);
    const KfMixedOff mo = kf_mixed_in(A, mx, (size_t)n, (size_t)M);
    KfSearched S;
    kf_searched_in(A, S, 1, kps, desc, stride, uright, off, gb, taken);
    // outputs: taken (in / out) | best index | best distance; then the keypoints' cells
    A.inout(taken, S.tk, (size_t)n);
    const size_t o_bi = A.out(best_idx, sizeof(int32_t) * M), o_bd = A.out(best_dist, sizeof(int32_t) * M);
    kf_searched_cells(A, S);
    if ((rc = A.upload())) return rc;
    const KfSideDev Q{A.dev<uint8_t>(o_va), A.dev<float2>(o_uv), A.dev<int32_t>(o_lv), A.dev<float>(o_rad), A.dev<float>(o_qur), nullptr, nullptr};
    const RadBatchArgsMixed B = kf_searched_args(A, S, M, Q, A.dev<uint8_t>(o_qd), 0, inv_sigma2 ? A.dev<float>(o_is) : nullptr, nlevels, accept_thr,
                                                 A.dev<int32_t>(o_bi), A.dev<int32_t>(o_bd), mx, mo);
    if ((rc = kf_radius_dev(c, mx ? "kf_radius_match_mixed" : "kf_radius_match", mx != nullptr, B, n, kf_mixed_kp(A, mx, mo)))) return rc;
    return A.fetch();
}

int eorb_kf_radius_match(eorb_ctx* c,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
        int M, const uint8_t* valid, const float* uv, const float* radius, const int32_t* level, const uint8_t* q_desc,
        const float* inv_sigma2, int nlevels, uint8_t* taken, float accept_thr, int32_t* best_idx, int32_t* best_dist)
{
    return kf_radius_common(c, kps, n, desc, stride, gb, M, valid, uv, radius, level, q_desc, inv_sigma2, nlevels, taken, accept_thr, best_idx, best_dist, nullptr, nullptr);
}

int eorb_kf_radius_match_stereo(eorb_ctx* c,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
        int M, const uint8_t* valid, const float* uv, const float* radius, const int32_t* level, const uint8_t* q_desc,
        const float* inv_sigma2, int nlevels, const float* uright, const float* q_ur, int32_t* best_idx, int32_t* best_dist)
{
    return kf_radius_common(c, kps, n, desc, stride, gb, M, valid, uv, radius, level, q_desc, inv_sigma2, nlevels, nullptr, 0.f, best_idx, best_dist, uright, q_ur);
}

int eorb_kf_radius_match_mixed(eorb_ctx* c,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
        const uint8_t* kp_is_orb, const float* kp_inv_sigma2, const float* uright,
        int M, const uint8_t* valid, const float* uv, const float* radius, const int32_t* level, const uint8_t* q_desc,
        const uint8_t* mp_is_orb, const float* q_ur, uint8_t* taken, float accept_thr, int32_t* best_idx, int32_t* best_dist)
{
    const KfMixedIn mx{kp_is_orb, kp_inv_sigma2, mp_is_orb};
    return kf_radius_common(c, kps, n, desc, stride, gb, M, valid, uv, radius, level, q_desc, nullptr, 0, taken, accept_thr, best_idx, best_dist,
                            uright, q_ur, &mx);
}

// ---- KeyFrame-side matchers: projection (project.hip modes D, E) and search behind one upload, one wait, one download ------------
// Limits of one call: the arena holds 34 B per query and 64 B per keypoint
static constexpr int64_t kKfSideMaxQueries = (int64_t)1 << 22;      // K * M
static constexpr int64_t kKfSideMaxKps = (int64_t)1 << 22;          // keypoints of all keyframes together
static constexpr int kKfSideMaxKfs = 1024;                          // K

static KfPose kf_pose_of(const eorb_view& v)
{
    KfPose P{};
    memcpy(P.R, v.R, sizeof(P.R)); memcpy(P.t, v.t, sizeof(P.t)); memcpy(P.Ow, v.Ow, sizeof(P.Ow));
    P.cam = warp_cam_of(v.cam);
    P.minX = v.minX; P.maxX = v.maxX; P.minY = v.minY; P.maxY = v.maxY; P.mbf = v.mbf;
    return P;
}

// the arena regions of the projector's K * M outputs: reason first (eorb_fuse_keyframes wants nothing else), then the members of
// eorb_kfside_out.  out: the caller's record, or NULL (nothing of it is taken)
struct KfSideOff { size_t rs, va, uv, rad, lv, qur, d3; };
static KfSideOff kfside_reserve(Arena& A, size_t n, const eorb_kfside_out* out)
{
    const eorb_kfside_out d = out ? *out : eorb_kfside_out{};
    KfSideOff o;
    o.rs = A.out(d.reason, n);
    o.va = A.out(d.valid, n); o.uv = A.out(d.uv, 8 * n); o.rad = A.out(d.radius, 4 * n); o.lv = A.out(d.level, 4 * n); o.qur = A.out(d.q_ur, 4 * n);
    o.d3 = A.out(d.dist3d, 4 * n);
    return o;
}
static KfSideDev kfside_dev(const Arena& A, const KfSideOff& o)
{
    return KfSideDev{A.dev<uint8_t>(o.va), A.dev<float2>(o.uv), A.dev<int32_t>(o.lv), A.dev<float>(o.rad), A.dev<float>(o.qur),
                     A.dev<float>(o.d3), A.dev<uint8_t>(o.rs)};
}

// the map points of mode D and the views' shared table
struct KfSideIn { size_t pos, nrm, mind, maxd, skip, sf, pose, ak; KfMixedOff mo; std::vector<KfPose> poses; };
static int kfside_check(eorb_ctx* c, const char* who, const eorb_view* views, int K, int M, const float* pos, const float* normal,
                        const float* min_dist, const float* max_dist, bool mixed = false)
{
    if (K < 0 || M < 0 || (K > 0 && !views) || (K > 0 && M > 0 && (!pos || !normal || !min_dist || !max_dist)))
        return set_err(c, EORB_E_ARG, "%s: bad arguments", who);
    int rc;
    for (int k = 0; k < K; k++) {
        if ((rc = view_check(c, who, views + k, false))) return rc;
        if (views[k].nlevels != views[0].nlevels || views[k].log_scale != views[0].log_scale)
            return set_err(c, EORB_E_ARG, "%s: keyframe %d has another scale pyramid than keyframe 0 (one table serves the batch)", who, k);
        if (mixed && (views[k].ak_nlevels != views[0].ak_nlevels || views[k].ak_log_scale != views[0].ak_log_scale))
            return set_err(c, EORB_E_ARG, "%s: keyframe %d has another AKAZE pyramid than keyframe 0 (one table serves the batch)", who, k);
    }
    return EORB_OK;
}
static void kfside_in(Arena& A, KfSideIn& I, const eorb_view* views, int K, int M, const float* pos, const float* normal,
                      const float* min_dist, const float* max_dist, const uint8_t* skip, const KfMixedIn* mx = nullptr, size_t ntotal = 0)
{
    const size_t m = (size_t)M;
    I.pos = A.in(pos, 12 * m); I.nrm = A.in(normal, 12 * m); I.mind = A.in(min_dist, 4 * m); I.maxd = A.in(max_dist, 4 * m);
    I.skip = A.in(skip, skip ? (size_t)K * m : 0);
    I.sf = A.in(views[0].scale_factors, sizeof(float) * (size_t)views[0].nlevels);
    I.ak = mx ? A.in(views[0].ak_scale_factors, views[0].ak_nlevels > 0 ? sizeof(float) * (size_t)views[0].ak_nlevels : 0) : 0;
    I.mo = kf_mixed_in(A, mx, ntotal, m);
    I.poses.resize(K);
    for (int k = 0; k < K; k++) I.poses[k] = kf_pose_of(views[k]);
    I.pose = A.in(I.poses.data(), sizeof(KfPose) * (size_t)K);
}
static KfSideArgsMixed kfside_args(const Arena& A, const KfSideIn& I, const eorb_view* views, int K, int M, bool has_skip, float th, const KfSideOff& o,
                              const KfMixedIn* mx = nullptr)
{
    KfSideArgsMixed P{};
    P.V = A.dev<KfPose>(I.pose); P.K = K; P.M = M;
    P.nlevels = views[0].nlevels; P.log_scale = views[0].log_scale; P.sf = A.dev<float>(I.sf); P.th = th;
    P.pos = A.dev<float>(I.pos); P.normal = A.dev<float>(I.nrm); P.min_dist = A.dev<float>(I.mind); P.max_dist = A.dev<float>(I.maxd);
    P.skip = has_skip ? A.dev<uint8_t>(I.skip) : nullptr;
    P.O = kfside_dev(A, o);
    if (mx) {
        P.mp_is_orb = kf_mixed_mp(A, mx, I.mo);
        P.ak_nlevels = views[0].ak_nlevels; P.ak_log_scale = views[0].ak_log_scale; P.ak_sf = P.ak_nlevels > 0 ? A.dev<float>(I.ak) : nullptr;
    }
    return P;
}

static int project_kfside_common(eorb_ctx* c, const char* who, const eorb_view* view, int M, const float* pos, const float* normal,
                                 const float* min_dist, const float* max_dist, const uint8_t* skip, float th, const eorb_kfside_out* out,
                                 const KfMixedIn* mx)
{
    if (!c) return EORB_E_ARG;
    int rc;
    if (!view) return set_err(c, EORB_E_ARG, "%s: null view", who);
    if ((rc = kfside_check(c, who, view, 1, M, pos, normal, min_dist, max_dist))) return rc;
    if (M > kKfSideMaxQueries) return set_err(c, EORB_E_CAPACITY, "%s: %d map points exceed %lld", who, M, (long long)kKfSideMaxQueries);
    fe_enter(c);
    if (M == 0) return EORB_OK;
    Arena A(c);
    KfSideIn I;
    kfside_in(A, I, view, 1, M, pos, normal, min_dist, max_dist, skip, mx);
    const KfSideOff o = kfside_reserve(A, (size_t)M, out);
    if ((rc = A.upload())) return rc;
    const KfSideArgsMixed P = kfside_args(A, I, view, 1, M, skip != nullptr, th, o, mx);
    if ((rc = mx ? project_kfside_mixed_dev(c, P) : project_kfside_dev(c, P))) return rc;
    return A.fetch();
}

int eorb_project_keyframe_side(eorb_ctx* c, const eorb_view* view, int M, const float* pos, const float* normal, const float* min_dist,
                               const float* max_dist, const uint8_t* skip, float th, const eorb_kfside_out* out)
{
    return project_kfside_common(c, "project_keyframe_side", view, M, pos, normal, min_dist, max_dist, skip, th, out, nullptr);
}

int eorb_project_keyframe_side_mixed(eorb_ctx* c, const eorb_view* view, int M, const float* pos, const float* normal, const float* min_dist,
                                     const float* max_dist, const uint8_t* mp_is_orb, const uint8_t* skip, float th, const eorb_kfside_out* out)
{
    const KfMixedIn mx{nullptr, nullptr, mp_is_orb};
    return project_kfside_common(c, "project_keyframe_side_mixed", view, M, pos, normal, min_dist, max_dist, skip, th, out, &mx);
}

// mode D over K keyframes, then the radius search; shared by eorb_fuse_pose (K = 1), eorb_fuse_keyframes and, with seq, by
// eorb_search_by_projection_kf_scw (K = 1: the queries in order, vpMatched = taken in and out, no reprojection gate)
struct KfInOrder { uint8_t* taken; float accept_thr; };
static int fuse_common(eorb_ctx* c, const char* who, const eorb_view* views, const eorb_grid_bounds* gb, int K,
                       const eorb_keypoint* kps, const uint8_t* desc, int stride, const float* uright, const int32_t* kf_off,
                       int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* q_desc,
                       const uint8_t* skip, const float* inv_sigma2, float th, int32_t* best_idx, int32_t* best_dist, const eorb_kfside_out* out,
                       const KfMixedIn* mx = nullptr, const KfInOrder* seq = nullptr)
{
    int rc;
    if (K > kKfSideMaxKfs || (K > 0 && M > 0 && (int64_t)K * M > kKfSideMaxQueries))      // (sizes only: nothing is read before this)
        return set_err(c, EORB_E_CAPACITY, "%s: %d keyframes x %d map points exceed %d keyframes or %lld queries", who, K, M, kKfSideMaxKfs,
                       (long long)kKfSideMaxQueries);
    if ((rc = kfside_check(c, who, views, K, M, pos, normal, min_dist, max_dist, mx != nullptr))) return rc;
    if (stride < 32 || (K > 0 && (!gb || !kf_off)) || (K > 0 && M > 0 && (!q_desc || !best_idx || !best_dist)) ||
        (uright && !(mx ? mx->kp_inv_sigma2 : inv_sigma2)))
        return set_err(c, EORB_E_ARG, "%s: bad arguments", who);
    if (K == 0) return EORB_OK;
    if (kf_off[0] != 0) return set_err(c, EORB_E_ARG, "%s: kf_off[0] = %d", who, kf_off[0]);
    for (int k = 0; k < K; k++) if (kf_off[k + 1] < kf_off[k]) return set_err(c, EORB_E_ARG, "%s: kf_off decreases at keyframe %d", who, k);
    const int ntotal = kf_off[K];
    if (ntotal > kKfSideMaxKps) return set_err(c, EORB_E_CAPACITY, "%s: %d keypoints exceed %lld", who, ntotal, (long long)kKfSideMaxKps);
    if (ntotal > 0 && (!kps || !desc)) return set_err(c, EORB_E_ARG, "%s: no keypoints", who);
    if (inv_sigma2 && views[0].nlevels > 64) return set_err(c, EORB_E_ARG, "%s: the reprojection gate takes at most 64 levels", who);
    fe_enter(c);
    const size_t nq = (size_t)K * M;
    for (size_t q = 0; q < nq; q++) { best_idx[q] = -1; best_dist[q] = 256; }
    if (M == 0) return EORB_OK;
    Arena A(c);
    KfSideIn I;
    kfside_in(A, I, views, K, M, pos, normal, min_dist, max_dist, skip, mx, (size_t)ntotal);
    const size_t o_qd = A.in(q_desc, 32 * (size_t)M);
    const size_t o_is = A.in(inv_sigma2, inv_sigma2 ? sizeof(float) * (size_t)views[0].nlevels : 0);
    uint8_t* taken = seq ? seq->taken : nullptr;
    KfSearched S;
    kf_searched_in(A, S, K, kps, desc, stride, uright, kf_off, gb, taken);
    // outputs: taken (in / out, the in-order form) | best index | best distance | the projector's arrays; then the keypoints' cells
    A.inout(taken, S.tk, (size_t)ntotal);
    const size_t o_bi = A.out(best_idx, 4 * nq), o_bd = A.out(best_dist, 4 * nq);
    const KfSideOff o = kfside_reserve(A, nq, out);
    kf_searched_cells(A, S);
    if ((rc = A.upload())) return rc;
    const KfSideArgsMixed P = kfside_args(A, I, views, K, M, skip != nullptr, th, o, mx);
    if ((rc = mx ? project_kfside_mixed_dev(c, P) : project_kfside_dev(c, P))) return rc;
    const RadBatchArgsMixed B = kf_searched_args(A, S, M, P.O, A.dev<uint8_t>(o_qd), 0, inv_sigma2 ? A.dev<float>(o_is) : nullptr, views[0].nlevels,
                                                 seq ? seq->accept_thr : 0.f, A.dev<int32_t>(o_bi), A.dev<int32_t>(o_bd), mx, I.mo);
    const char* scope = seq ? (mx ? "kf_radius_match_mixed" : "kf_radius_match") : (mx ? "kf_radius_batch_mixed" : "kf_radius_batch");
    if ((rc = kf_radius_dev(c, scope, mx != nullptr, B, ntotal, kf_mixed_kp(A, mx, I.mo)))) return rc;
    return A.fetch();
}

int eorb_fuse_pose(eorb_ctx* c, const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
                   const eorb_view* view, int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                   const uint8_t* skip, const uint8_t* q_desc, const float* inv_sigma2, const float* uright, float th,
                   int32_t* best_idx, int32_t* best_dist, const eorb_kfside_out* out)
{
    if (!c) return EORB_E_ARG;
    if (n < 0 || !view || !gb) return set_err(c, EORB_E_ARG, "fuse_pose: bad arguments");
    const int32_t off[2] = {0, n};
    return fuse_common(c, "fuse_pose", view, gb, 1, kps, desc, stride, uright, off, M, pos, normal, min_dist, max_dist, q_desc, skip,
                       inv_sigma2, th, best_idx, best_dist, out);
}

int eorb_fuse_keyframes(eorb_ctx* c, const eorb_view* views, const eorb_grid_bounds* gb, int K,
                        const eorb_keypoint* kps, const uint8_t* desc, int stride, const float* uright, const int32_t* kf_off,
                        int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* q_desc,
                        const uint8_t* skip, const float* inv_sigma2, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reason)
{
    if (!c) return EORB_E_ARG;
    eorb_kfside_out out{};
    out.reason = reason;
    return fuse_common(c, "fuse_keyframes", views, gb, K, kps, desc, stride, uright, kf_off, M, pos, normal, min_dist, max_dist, q_desc, skip,
                       inv_sigma2, th, best_idx, best_dist, reason ? &out : nullptr);
}

int eorb_fuse_pose_mixed(eorb_ctx* c, const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
                         const uint8_t* kp_is_orb, const float* kp_inv_sigma2, const float* uright,
                         const eorb_view* view, int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                         const uint8_t* mp_is_orb, const uint8_t* skip, const uint8_t* q_desc, float th,
                         int32_t* best_idx, int32_t* best_dist, const eorb_kfside_out* out)
{
    if (!c) return EORB_E_ARG;
    if (n < 0 || !view || !gb) return set_err(c, EORB_E_ARG, "fuse_pose_mixed: bad arguments");
    const int32_t off[2] = {0, n};
    const KfMixedIn mx{kp_is_orb, kp_inv_sigma2, mp_is_orb};
    return fuse_common(c, "fuse_pose_mixed", view, gb, 1, kps, desc, stride, uright, off, M, pos, normal, min_dist, max_dist, q_desc, skip,
                       nullptr, th, best_idx, best_dist, out, &mx);
}

int eorb_fuse_keyframes_mixed(eorb_ctx* c, const eorb_view* views, const eorb_grid_bounds* gb, int K,
                              const eorb_keypoint* kps, const uint8_t* desc, int stride, const uint8_t* kp_is_orb, const float* kp_inv_sigma2,
                              const float* uright, const int32_t* kf_off,
                              int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* mp_is_orb,
                              const uint8_t* q_desc, const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reason)
{
    if (!c) return EORB_E_ARG;
    eorb_kfside_out out{};
    out.reason = reason;
    const KfMixedIn mx{kp_is_orb, kp_inv_sigma2, mp_is_orb};
    return fuse_common(c, "fuse_keyframes_mixed", views, gb, K, kps, desc, stride, uright, kf_off, M, pos, normal, min_dist, max_dist, q_desc, skip,
                       nullptr, th, best_idx, best_dist, reason ? &out : nullptr, &mx);
}

// SearchByProjection(pKF, Scw): fuse_common at K = 1 in order; the entry points' own checks come first (no inv_sigma2, no uright)
static int kf_scw_check(eorb_ctx* c, const char* who, const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
                        const eorb_view* view, int M, const uint8_t* q_desc, const uint8_t* taken, const int32_t* best_idx, const int32_t* best_dist)
{
    if (n < 0 || !view || !gb || stride < 32 || (n > 0 && (!kps || !desc || !taken)) || (M > 0 && (!q_desc || !best_idx || !best_dist)))
        return set_err(c, EORB_E_ARG, "%s: bad arguments", who);
    return EORB_OK;
}

int eorb_search_by_projection_kf_scw(eorb_ctx* c, const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
                                     const eorb_view* view, int M, const float* pos, const float* normal, const float* min_dist,
                                     const float* max_dist, const uint8_t* skip, const uint8_t* q_desc, float th, uint8_t* taken,
                                     float accept_thr, int32_t* best_idx, int32_t* best_dist, const eorb_kfside_out* out)
{
    if (!c) return EORB_E_ARG;
    const char* who = "search_by_projection_kf_scw";
    int rc;
    if ((rc = kf_scw_check(c, who, kps, n, desc, stride, gb, view, M, q_desc, taken, best_idx, best_dist))) return rc;
    const int32_t off[2] = {0, n};
    const KfInOrder seq{taken, accept_thr};
    return fuse_common(c, who, view, gb, 1, kps, desc, stride, nullptr, off, M, pos, normal, min_dist, max_dist, q_desc, skip, nullptr, th,
                       best_idx, best_dist, out, nullptr, &seq);
}

int eorb_search_by_projection_kf_scw_mixed(eorb_ctx* c, const eorb_keypoint* kps, int n, const uint8_t* desc, int stride,
                                           const eorb_grid_bounds* gb, const uint8_t* kp_is_orb, const eorb_view* view, int M, const float* pos,
                                           const float* normal, const float* min_dist, const float* max_dist, const uint8_t* mp_is_orb,
                                           const uint8_t* skip, const uint8_t* q_desc, float th, uint8_t* taken, float accept_thr,
                                           int32_t* best_idx, int32_t* best_dist, const eorb_kfside_out* out)
{
    if (!c) return EORB_E_ARG;
    const char* who = "search_by_projection_kf_scw_mixed";
    int rc;
    if ((rc = kf_scw_check(c, who, kps, n, desc, stride, gb, view, M, q_desc, taken, best_idx, best_dist))) return rc;
    const int32_t off[2] = {0, n};
    const KfMixedIn mx{kp_is_orb, nullptr, mp_is_orb};
    const KfInOrder seq{taken, accept_thr};
    return fuse_common(c, who, view, gb, 1, kps, desc, stride, nullptr, off, M, pos, normal, min_dist, max_dist, q_desc, skip, nullptr, th,
                       best_idx, best_dist, out, &mx, &seq);
}

int eorb_search_by_sim3(eorb_ctx* c,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, int stride1, const eorb_grid_bounds* gb1, const eorb_view* view1,
        const float* pos1, const float* min_dist1, const float* max_dist1, const uint8_t* mp_desc1, const uint8_t* skip1,
        const eorb_keypoint* kps2, int n2, const uint8_t* desc2, int stride2, const eorb_grid_bounds* gb2, const eorb_view* view2,
        const float* pos2, const float* min_dist2, const float* max_dist2, const uint8_t* mp_desc2, const uint8_t* skip2,
        const float* sR12, const float* t12, const float* sR21, const float* t21, float th, int th_high,
        int32_t* match12, int* nfound, int32_t* vnMatch1, int32_t* vnMatch2)
{
    if (!c) return EORB_E_ARG;
    if (nfound) *nfound = 0;
    if (n1 < 0 || n2 < 0 || stride1 < 32 || stride2 < 32 || !gb1 || !gb2 || !sR12 || !t12 || !sR21 || !t21 || th_high < 0 || th_high > 255 ||
        (n1 > 0 && (!kps1 || !desc1 || !pos1 || !min_dist1 || !max_dist1 || !mp_desc1 || !match12)) ||
        (n2 > 0 && (!kps2 || !desc2 || !pos2 || !min_dist2 || !max_dist2 || !mp_desc2)))
        return set_err(c, EORB_E_ARG, "search_by_sim3: bad arguments");
    int rc;
    if ((rc = view_check(c, "search_by_sim3", view1, false)) || (rc = view_check(c, "search_by_sim3", view2, false))) return rc;
    if (view1->cam.model != 0 || view2->cam.model != 0)      // the reference hard-codes fx, fy, cx, cy (:1746-1749, :1811)
        return set_err(c, EORB_E_CONFIG, "search_by_sim3: pinhole keyframes only");
    if ((int64_t)n1 + n2 > kKfSideMaxKps) return set_err(c, EORB_E_CAPACITY, "search_by_sim3: %d + %d keypoints exceed %lld", n1, n2, (long long)kKfSideMaxKps);
    fe_enter(c);
    for (int i = 0; i < n1; i++) match12[i] = -1;
    if (vnMatch1) for (int i = 0; i < n1; i++) vnMatch1[i] = -1;
    if (vnMatch2) for (int i = 0; i < n2; i++) vnMatch2[i] = -1;
    if (n1 == 0 || n2 == 0) return EORB_OK;
    // a 2 x M batch: row 0 = KF1's points searched in KF2, row 1 = KF2's points searched in KF1; the searched keypoints in that order
    const int M = std::max(n1, n2), ntotal = n1 + n2;
    const size_t m = (size_t)M;
    std::vector<eorb_keypoint> kcat((size_t)ntotal);
    memcpy(kcat.data(), kps2, sizeof(eorb_keypoint) * (size_t)n2); memcpy(kcat.data() + n2, kps1, sizeof(eorb_keypoint) * (size_t)n1);
    std::vector<uint8_t> dcat(32 * (size_t)ntotal), qd(64 * m, 0);
    for (int i = 0; i < n2; i++) memcpy(&dcat[32 * (size_t)i], desc2 + (size_t)i * stride2, 32);
    for (int i = 0; i < n1; i++) memcpy(&dcat[32 * ((size_t)n2 + i)], desc1 + (size_t)i * stride1, 32);
    memcpy(qd.data(), mp_desc1, 32 * (size_t)n1); memcpy(qd.data() + 32 * m, mp_desc2, 32 * (size_t)n2);
    const int32_t off[3] = {0, n2, ntotal};
    const eorb_grid_bounds gb[2] = {*gb2, *gb1};
    Arena A(c);
    KfSearched R;
    kf_searched_in(A, R, 2, kcat.data(), dcat.data(), 32, nullptr, off, gb, nullptr);
    const size_t o_qd = A.in(qd.data(), qd.size());
    const size_t o_p1 = A.in(pos1, 12 * (size_t)n1), o_mn1 = A.in(min_dist1, 4 * (size_t)n1), o_mx1 = A.in(max_dist1, 4 * (size_t)n1);
    const size_t o_p2 = A.in(pos2, 12 * (size_t)n2), o_mn2 = A.in(min_dist2, 4 * (size_t)n2), o_mx2 = A.in(max_dist2, 4 * (size_t)n2);
    const size_t o_s1 = A.in(skip1, skip1 ? (size_t)n1 : 0), o_s2 = A.in(skip2, skip2 ? (size_t)n2 : 0);
    const size_t o_sf1 = A.in(view1->scale_factors, sizeof(float) * (size_t)view1->nlevels);
    const size_t o_sf2 = A.in(view2->scale_factors, sizeof(float) * (size_t)view2->nlevels);
    // outputs: nfound | match12 | vnMatch1 | vnMatch2; then what only the kernels read
    const size_t o_nf = A.out(nullptr, 16), o_m12 = A.out(match12, 4 * (size_t)n1), o_v1 = A.out(vnMatch1, 4 * (size_t)n1), o_v2 = A.out(vnMatch2, 4 * (size_t)n2);
    A.inout(nfound, o_nf, sizeof(int32_t));
    const size_t o_bi = A.reserve(8 * m), o_bd = A.reserve(8 * m);
    const KfSideOff o = kfside_reserve(A, 2 * m, nullptr);
    kf_searched_cells(A, R);
    if ((rc = A.upload())) return rc;
    Sim3Args S{};
    S.M = M; S.th = th; S.O = kfside_dev(A, o);
    for (int hf = 0; hf < 2; hf++) {
        Sim3Half& H = S.H[hf];
        const eorb_view* va = hf ? view2 : view1; const eorb_view* vb = hf ? view1 : view2;
        memcpy(H.Ra, va->R, sizeof(H.Ra)); memcpy(H.ta, va->t, sizeof(H.ta));
        memcpy(H.sRb, hf ? sR12 : sR21, sizeof(H.sRb)); memcpy(H.tb, hf ? t12 : t21, sizeof(H.tb));
        H.fx = view1->cam.fx; H.fy = view1->cam.fy; H.cx = view1->cam.cx; H.cy = view1->cam.cy;
        H.minX = vb->minX; H.maxX = vb->maxX; H.minY = vb->minY; H.maxY = vb->maxY;
        H.nlevels = vb->nlevels; H.log_scale = vb->log_scale; H.sf = A.dev<float>(hf ? o_sf1 : o_sf2);
        H.n = hf ? n2 : n1;
        H.pos = A.dev<float>(hf ? o_p2 : o_p1); H.min_dist = A.dev<float>(hf ? o_mn2 : o_mn1); H.max_dist = A.dev<float>(hf ? o_mx2 : o_mx1);
        H.skip = (hf ? skip2 : skip1) ? A.dev<uint8_t>(hf ? o_s2 : o_s1) : nullptr;
    }
    if ((rc = project_sim3_dev(c, S))) return rc;
    const RadBatchArgsMixed B = kf_searched_args(A, R, M, S.O, A.dev<uint8_t>(o_qd), 32 * m, nullptr, 0, 0.f, A.dev<int32_t>(o_bi), A.dev<int32_t>(o_bd),
                                                 nullptr, KfMixedOff{});
    if ((rc = kf_radius_dev(c, "kf_radius_batch", false, B, ntotal, nullptr))) return rc;
    if ((rc = sim3_agree_dev(c, B.best_idx, B.best_dist, M, n1, n2, th_high, A.dev<int32_t>(o_v1), A.dev<int32_t>(o_v2), A.dev<int32_t>(o_m12),
                             A.dev<int32_t>(o_nf)))) return rc;
    return A.fetch();
}

int eorb_bow_set_vocabulary(eorb_ctx* c, int nnodes, int L, const int32_t* child_off, const int32_t* child_ids,
                            const uint8_t* node_desc, const int32_t* word_id, const double* weight)
{
    if (!c) return EORB_E_ARG;
    if (nnodes < 1 || L < 1 || L > 32 || !child_off || !child_ids || !node_desc || !word_id || !weight)
        return set_err(c, EORB_E_ARG, "bow_set_vocabulary: bad arguments");
    // a tree rooted at node 0: monotone offsets, every node but the root has exactly one parent, depth <= 32, no cycles
    const int nch = child_off[nnodes];
    if (child_off[0] != 0 || nch != nnodes - 1) return set_err(c, EORB_E_ARG, "bow_set_vocabulary: %d child links for %d nodes", nch, nnodes);
    std::vector<int8_t> depth(nnodes, -1);
    depth[0] = 0;
    std::vector<int> stack{0};
    int visited = 0;
    while (!stack.empty()) {
        const int u = stack.back(); stack.pop_back(); visited++;
        if (child_off[u + 1] < child_off[u]) return set_err(c, EORB_E_ARG, "bow_set_vocabulary: offsets not monotone at node %d", u);
        for (int k = child_off[u]; k < child_off[u + 1]; k++) {
            const int v = child_ids[k];
            if (v <= 0 || v >= nnodes || depth[v] >= 0) return set_err(c, EORB_E_ARG, "bow_set_vocabulary: node %d is not a tree child", v);
            if (depth[u] >= 32) return set_err(c, EORB_E_ARG, "bow_set_vocabulary: tree deeper than 32");
            depth[v] = (int8_t)(depth[u] + 1);
            stack.push_back(v);
        }
    }
    if (visited != nnodes) return set_err(c, EORB_E_ARG, "bow_set_vocabulary: %d of %d nodes reachable from the root", visited, nnodes);
    fe_enter(c);
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    size_t off[6]; off[0] = 0;
    off[1] = off[0] + al(sizeof(int32_t) * ((size_t)nnodes + 1));
    off[2] = off[1] + al(sizeof(int32_t) * (size_t)std::max(nch, 1));
    off[3] = off[2] + al(32 * (size_t)nnodes);
    off[4] = off[3] + al(sizeof(int32_t) * (size_t)nnodes);
    off[5] = off[4] + al(sizeof(double) * (size_t)nnodes);
    int rc;
    if ((rc = upload_persistent(c, c->voc, off[5], [&](char* hp) {
            memset(hp, 0, off[5]);
            memcpy(hp + off[0], child_off, sizeof(int32_t) * ((size_t)nnodes + 1));
            memcpy(hp + off[1], child_ids, sizeof(int32_t) * (size_t)nch);
            memcpy(hp + off[2], node_desc, 32 * (size_t)nnodes);
            memcpy(hp + off[3], word_id, sizeof(int32_t) * (size_t)nnodes);
            memcpy(hp + off[4], weight, sizeof(double) * (size_t)nnodes);
        }))) return rc;
    c->voc_nnodes = nnodes; c->voc_L = L;
    for (int i = 0; i < 5; i++) c->voc_off[i] = off[i];
    return EORB_OK;
}

int eorb_bow_transform(eorb_ctx* c, const uint8_t* desc, int n, int stride, int levelsup, int weighting, int norm,
                       uint32_t* bow_word, double* bow_val, int* n_words, uint32_t* fv_node, int32_t* fv_off, int32_t* fv_idx,
                       int* n_fvnodes, int32_t* word_of, int32_t* node_of)
{
    if (!c) return EORB_E_ARG;
    if (!c->voc_nnodes) return set_err(c, EORB_E_NOTCONF, "bow_transform: eorb_bow_set_vocabulary not called");
    if (n < 0 || stride < 32 || weighting < 0 || weighting > 3 || norm < 0 || norm > 2 || !n_words || !n_fvnodes || !fv_off ||
        (n > 0 && (!desc || !bow_word || !bow_val || !fv_node || !fv_idx)))
        return set_err(c, EORB_E_ARG, "bow_transform: bad arguments");
    // the limit, from n alone: before the arena is built or uploaded and before any of the caller's arrays is written
    if (!plan_bow_transform(n).ok)
        return set_err(c, EORB_E_CAPACITY, "bow_transform: %d features, at most %d per call (the LDS sort)", n, kBowMaxFeatures);
    fe_enter(c);
    *n_words = 0; *n_fvnodes = 0; fv_off[0] = 0;
    if (n == 0 || c->voc_nnodes <= 1) return EORB_OK;                       // empty() (:1132)
    int rc;
    const size_t N = (size_t)n;
    Arena A(c);
    const size_t o_desc = A.in(desc, (size_t)stride * n);
    // outputs, contiguous: counts | bow_word | bow_val | fv_off (+1) | fv_node | fv_idx | word_of | node_of; then w_of
    const size_t o_cnt = A.reserve(16), o_bw = A.reserve(4 * N), o_bv = A.reserve(8 * (N + 1)), o_fo = A.reserve(4 * (N + 2));
    const size_t o_fn = A.reserve(4 * N), o_fi = A.reserve(4 * (N + 2)), o_wo = A.reserve(4 * N), o_no = A.reserve(4 * N);
    const size_t o_wf = A.reserve(8 * (N + 1));
    if ((rc = A.upload())) return rc;
    const char* vb = (const char*)c->voc.p;
    BowVoc V{c->voc_nnodes, c->voc_L, (const int32_t*)(vb + c->voc_off[0]), (const int32_t*)(vb + c->voc_off[1]),
             (const uint8_t*)(vb + c->voc_off[2]), (const int32_t*)(vb + c->voc_off[3]), (const double*)(vb + c->voc_off[4])};
    if ((rc = bow_transform_dev(c, A.dev<uint8_t>(o_desc), n, stride, V, levelsup, weighting, norm, A.dev<uint32_t>(o_wo), A.dev<double>(o_wf),
                                A.dev<uint32_t>(o_no), A.dev<uint32_t>(o_bw), A.dev<double>(o_bv), A.dev<uint32_t>(o_fn), A.dev<int32_t>(o_fo),
                                A.dev<int32_t>(o_fi), A.dev<int32_t>(o_cnt)))) return rc;
    const char* h;
    if ((rc = A.download(o_cnt, 8, &h))) return rc;
    int32_t cnt[2];
    memcpy(cnt, h + o_cnt, 8);
    *n_words = cnt[0]; *n_fvnodes = cnt[1];
    // the second fetch: the arrays at the sizes the counts give; the feature vector's indices are as many as fv_off says, which arrives
    // with them (their region is fetched whole)
    A.inout(bow_word, o_bw, 4 * (size_t)cnt[0]); A.inout(bow_val, o_bv, 8 * (size_t)cnt[0]);
    A.inout(fv_off, o_fo, 4 * ((size_t)cnt[1] + 1)); A.inout(fv_node, o_fn, 4 * (size_t)cnt[1]);
    A.want(o_fi, 4 * (N + 2));
    A.inout(word_of, o_wo, 4 * N); A.inout(node_of, o_no, 4 * N);
    if ((rc = A.fetch(&h))) return rc;
    memcpy(fv_idx, h + o_fi, 4 * (size_t)fv_off[cnt[1]]);
    return EORB_OK;
}

// ---- KeyFrameDatabase (kfdb.hip) ------------------------------------------------------------------------------------------------
int eorb_kfdb_clear(eorb_ctx* c)
{
    if (!c) return EORB_E_ARG;
    KfdbState& s = c->kfdb;
    s.n_slots = 0; s.n_live = 0; s.word_used = 0; s.word_live = 0; s.next_seq = 0;          // (the pools keep their size)
    s.h_tab.clear(); s.free_slots.clear();
    return EORB_OK;
}

int eorb_kfdb_info(eorb_ctx* c, int* n_live, int* n_slots)
{
    if (!c) return EORB_E_ARG;
    if (n_live) *n_live = c->kfdb.n_live;
    if (n_slots) *n_slots = c->kfdb.n_slots;
    return EORB_OK;
}

int eorb_kfdb_add(eorb_ctx* c, int K, const int32_t* off, const uint32_t* word, const double* val, int32_t* slots_out)
{
    if (!c) return EORB_E_ARG;
    if (K < 0 || (K > 0 && (!off || !slots_out))) return set_err(c, EORB_E_ARG, "kfdb_add: bad arguments");
    if (K == 0) return EORB_OK;
    KfdbState& s = c->kfdb;
    // limits first, from the sizes alone
    const int fresh = std::max(0, K - (int)s.free_slots.size());
    if (s.n_slots + fresh > kKfdbMaxSlots) return set_err(c, EORB_E_CAPACITY, "kfdb_add: %d slots, limit %d", s.n_slots + fresh, kKfdbMaxSlots);
    if ((uint64_t)s.next_seq + (uint64_t)K >= 0xffffffffull) return set_err(c, EORB_E_CAPACITY, "kfdb_add: add sequence numbers exhausted");
    if (off[0] != 0) return set_err(c, EORB_E_ARG, "kfdb_add: off[0] = %d", off[0]);
    for (int k = 0; k < K; k++) if (off[k + 1] < off[k]) return set_err(c, EORB_E_ARG, "kfdb_add: offsets not monotone at keyframe %d", k);
    const int64_t total = off[K];
    if (total > 0 && (!word || !val)) return set_err(c, EORB_E_ARG, "kfdb_add: bad arguments");
    if (s.word_live + total >= ((int64_t)1 << 30)) return set_err(c, EORB_E_CAPACITY, "kfdb_add: %lld words in the database, limit 2^30", (long long)(s.word_live + total));
    for (int k = 0; k < K; k++)
        for (int i = off[k] + 1; i < off[k + 1]; i++)
            if (word[i] <= word[i - 1]) return set_err(c, EORB_E_ARG, "kfdb_add: the word ids of keyframe %d do not ascend strictly (entry %d)", k, i - off[k]);
    fe_enter(c);
    int rc;
    if ((rc = kfdb_reserve(c, fresh, total))) return rc;
    std::vector<int32_t> slot(K);
    std::vector<KfdbSlot> rec(K);
    for (int k = 0; k < K; k++) {
        int sl;
        if (!s.free_slots.empty()) { std::pop_heap(s.free_slots.begin(), s.free_slots.end(), std::greater<int>()); sl = s.free_slots.back(); s.free_slots.pop_back(); }
        else { sl = s.n_slots++; s.h_tab.push_back(KfdbSlot{0u, -1, 0u, 0u}); }
        const int n = off[k + 1] - off[k];
        rec[k] = KfdbSlot{(uint32_t)s.word_used, n, s.next_seq++, 0u};
        s.word_used += n; s.word_live += n; s.n_live++;
        s.h_tab[sl] = rec[k];
        slot[k] = sl; slots_out[k] = sl;
    }
    Arena A(c);
    const size_t o_slot = A.in(slot.data(), sizeof(int32_t) * (size_t)K), o_rec = A.in(rec.data(), sizeof(KfdbSlot) * (size_t)K);
    const size_t o_src = A.in(off, sizeof(int32_t) * (size_t)K), o_w = A.in(word, sizeof(uint32_t) * (size_t)total), o_v = A.in(val, sizeof(double) * (size_t)total);
    if ((rc = A.upload())) return rc;
    if ((rc = kfdb_add_dev(c, K, A.dev<int32_t>(o_slot), A.dev<KfdbSlot>(o_rec), A.dev<int32_t>(o_src), A.dev<uint32_t>(o_w), A.dev<double>(o_v)))) return rc;
    EORB_HIP(c, fe_stream_sync(c));              // (slot, rec and the staging slot are free again)
    return EORB_OK;
}

int eorb_kfdb_erase(eorb_ctx* c, int slot)
{
    if (!c) return EORB_E_ARG;
    KfdbState& s = c->kfdb;
    if (slot < 0 || slot >= s.n_slots || s.h_tab[slot].n < 0) return set_err(c, EORB_E_ARG, "kfdb_erase: slot %d holds no keyframe", slot);
    fe_enter(c);
    int rc;
    if ((rc = kfdb_erase_dev(c, slot))) return rc;
    s.word_live -= s.h_tab[slot].n; s.n_live--;
    s.h_tab[slot] = KfdbSlot{0u, -1, 0u, 0u};
    s.free_slots.push_back(slot); std::push_heap(s.free_slots.begin(), s.free_slots.end(), std::greater<int>());
    return EORB_OK;
}

int eorb_kfdb_get_scores(eorb_ctx* c, int family, float* scores)
{
    if (!c) return EORB_E_ARG;
    if (family < 0 || family > 1 || !scores) return set_err(c, EORB_E_ARG, "kfdb_get_scores: bad arguments");
    KfdbState& s = c->kfdb;
    if (!s.n_slots) return EORB_OK;
    fe_enter(c);
    EORB_HIP(c, hipMemcpyAsync(scores, s.score[family].p, sizeof(float) * (size_t)s.n_slots, hipMemcpyDeviceToHost, c->stream));
    EORB_HIP(c, fe_stream_sync(c));
    return EORB_OK;
}

// both queries: one upload (the query, exclude, covis and the zeroed counters), three kernels, one download (counters and results)
static int kfdb_detect(eorb_ctx* c, const char* what, int nbest, int n_words, const uint32_t* word, const double* val, const uint8_t* exclude,
                       const int32_t* covis, int cap, int32_t* slot, float* si, int32_t* words, float* acc, int32_t* best_slot, uint8_t* keep,
                       float* sorted_acc, int32_t* sorted_best_slot, int* n_listed, int* n_scored, int* max_common_words, float* best_acc)
{
    if (!c) return EORB_E_ARG;
    if (n_words < 0 || cap < 0 || !n_listed || !n_scored || !max_common_words || !best_acc || (n_words > 0 && (!word || !val)) ||
        (cap > 0 && (!slot || !si || !words)) || (cap > 0 && covis && (!acc || !best_slot || (nbest ? (!sorted_acc || !sorted_best_slot) : !keep))))
        return set_err(c, EORB_E_ARG, "%s: bad arguments", what);
    KfdbState& s = c->kfdb;
    if (n_words > kKfdbMaxQueryWords) return set_err(c, EORB_E_CAPACITY, "%s: %d query words, limit %d", what, n_words, kKfdbMaxQueryWords);
    for (int i = 1; i < n_words; i++) if (word[i] <= word[i - 1]) return set_err(c, EORB_E_ARG, "%s: the query's word ids do not ascend strictly (entry %d)", what, i);
    *n_listed = 0; *n_scored = 0; *max_common_words = 0; *best_acc = 0.f;
    if (!n_words || !s.n_live) return EORB_OK;
    fe_enter(c);
    const size_t NS = (size_t)s.n_slots, CAP = (size_t)cap;
    int npad = 1;
    while (npad < s.n_slots) npad <<= 1;
    static const int32_t zero_hdr[4] = {0, 0, 0, 0};
    Arena A(c);
    KfdbQuery q{};
    q.n_slots = s.n_slots; q.nq = n_words; q.family = nbest ? EORB_KFDB_PLACE : EORB_KFDB_RELOC; q.cap = cap; q.nbest = nbest; q.npad = npad;
    q.lds_cap = c->opt.kfdb_finish_lds_entries > 0 ? c->opt.kfdb_finish_lds_entries : kKfdbMaxSlots;
    const size_t o_qw = A.in(word, sizeof(uint32_t) * (size_t)n_words), o_qv = A.in(val, sizeof(double) * (size_t)n_words);
    const size_t o_ex = exclude ? A.in(exclude, NS) : 0, o_cv = covis ? A.in(covis, sizeof(int32_t) * kKfdbCovis * NS) : 0;
    // outputs: counters | slot | si | words | acc | best_slot | keep | sorted_acc | sorted_best_slot.  The arrays hold n_scored records, known
    // after the download: the span covers their cap records, the copies follow the capacity check
    const size_t o_hdr = A.in(zero_hdr, sizeof(zero_hdr));
    A.want(o_hdr, sizeof(zero_hdr));
    auto records = [&](size_t bytes) { const size_t o = A.out(nullptr, bytes); A.want(o, bytes); return o; };
    const size_t o_slot = records(4 * CAP), o_si = records(4 * CAP), o_words = records(4 * CAP);
    const size_t o_acc = covis ? records(4 * CAP) : 0, o_best = covis ? records(4 * CAP) : 0, o_keep = covis && !nbest ? records(CAP) : 0;
    const size_t o_sacc = covis && nbest ? records(4 * CAP) : 0, o_sbest = covis && nbest ? records(4 * CAP) : 0;
    A.reserve(0);                                        // (an empty region; tests/golden/arena_layout.json pins the layout)
    const size_t o_cnt = A.reserve(4 * NS), o_first = A.reserve(4 * NS), o_listed = A.reserve(NS), o_sis = A.reserve(4 * NS);
    const size_t o_key = A.reserve(8 * (size_t)npad), o_kslot = A.reserve(4 * (size_t)npad);
    int rc;
    if ((rc = A.upload())) return rc;
    q.q_word = A.dev<uint32_t>(o_qw); q.q_val = A.dev<double>(o_qv);
    q.exclude = exclude ? A.dev<uint8_t>(o_ex) : nullptr; q.covis = covis ? A.dev<int32_t>(o_cv) : nullptr;
    q.hdr = A.dev<int32_t>(o_hdr);
    q.cnt = A.dev<int32_t>(o_cnt); q.first = A.dev<uint32_t>(o_first); q.listed = A.dev<uint8_t>(o_listed); q.si_slot = A.dev<float>(o_sis);
    q.key = A.dev<uint64_t>(o_key); q.kslot = A.dev<uint32_t>(o_kslot);
    q.o_slot = A.dev<int32_t>(o_slot); q.o_si = A.dev<float>(o_si); q.o_words = A.dev<int32_t>(o_words);
    q.o_acc = A.dev<float>(o_acc); q.o_best = A.dev<int32_t>(o_best); q.o_keep = A.dev<uint8_t>(o_keep);
    q.o_sacc = A.dev<float>(o_sacc); q.o_sbest = A.dev<int32_t>(o_sbest);
    if ((rc = kfdb_query_dev(c, q))) return rc;
    const char* h;
    if ((rc = A.fetch(&h))) return rc;
    int32_t hdr[4];
    memcpy(hdr, h + o_hdr, sizeof(hdr));
    *n_listed = hdr[0]; *n_scored = hdr[1]; *max_common_words = hdr[2]; memcpy(best_acc, &hdr[3], sizeof(float));
    if (hdr[1] > cap) return set_err(c, EORB_E_CAPACITY, "%s: %d keyframes scored, cap %d", what, hdr[1], cap);
    const size_t S = (size_t)hdr[1];
    memcpy(slot, h + o_slot, 4 * S); memcpy(si, h + o_si, 4 * S); memcpy(words, h + o_words, 4 * S);
    if (covis) {
        memcpy(acc, h + o_acc, 4 * S); memcpy(best_slot, h + o_best, 4 * S);
        if (nbest) { memcpy(sorted_acc, h + o_sacc, 4 * S); memcpy(sorted_best_slot, h + o_sbest, 4 * S); }
        else memcpy(keep, h + o_keep, S);
    }
    return EORB_OK;
}

int eorb_kfdb_detect_reloc(eorb_ctx* c, int n_words, const uint32_t* word, const double* val, const int32_t* covis, int cap,
                           int32_t* slot, float* si, int32_t* words, float* acc, int32_t* best_slot, uint8_t* keep,
                           int* n_listed, int* n_scored, int* max_common_words, float* best_acc)
{
    return kfdb_detect(c, "kfdb_detect_reloc", 0, n_words, word, val, nullptr, covis, cap, slot, si, words, acc, best_slot, keep, nullptr, nullptr,
                       n_listed, n_scored, max_common_words, best_acc);
}

int eorb_kfdb_detect_nbest(eorb_ctx* c, int n_words, const uint32_t* word, const double* val, const uint8_t* exclude, const int32_t* covis,
                           int cap, int32_t* slot, float* si, int32_t* words, float* acc, int32_t* best_slot, float* sorted_acc,
                           int32_t* sorted_best_slot, int* n_listed, int* n_scored, int* max_common_words, float* best_acc)
{
    return kfdb_detect(c, "kfdb_detect_nbest", 1, n_words, word, val, exclude, covis, cap, slot, si, words, acc, best_slot, nullptr, sorted_acc,
                       sorted_best_slot, n_listed, n_scored, max_common_words, best_acc);
}

int eorb_calc_optical_flow_pyr_lk(eorb_ctx* c, const uint8_t* prev, const uint8_t* next, int W, int H, int stride,
                                  const float* prev_pts, float* next_pts, int n, int win, int maxLevel, int maxCount, double epsilon,
                                  int flags, float minEigThreshold, uint8_t* status, float* err)
{
    if (!c) return EORB_E_ARG;
    if (!prev || !next || W <= 0 || H <= 0 || stride < W || n < 0 || win < 3 || win > 63 || maxLevel < 0 ||
        (n > 0 && (!prev_pts || !next_pts || !status || !err)))
        return set_err(c, EORB_E_ARG, "calc_optical_flow_pyr_lk: bad arguments");
    fe_enter(c);
    if (n == 0) return EORB_OK;
    int rc;
    const size_t ib = (size_t)stride * H;
    Arena A(c);
    const size_t o_prev = A.in(prev, ib), o_next = A.in(next, ib), o_pp = A.in(prev_pts, sizeof(float) * 2 * (size_t)n);
    // outputs: next points (in / out) | status | err
    const size_t o_np = A.in(next_pts, sizeof(float) * 2 * (size_t)n);
    A.inout(next_pts, o_np, sizeof(float) * 2 * (size_t)n);
    const size_t o_st = A.out(nullptr, (size_t)n + 16), o_err = A.out(err, sizeof(float) * (size_t)n);
    A.inout(status, o_st, (size_t)n);
    if ((rc = A.upload())) return rc;
    if ((rc = klt_track_dev(c, A.dev<uint8_t>(o_prev), A.dev<uint8_t>(o_next), W, H, stride, A.dev<float>(o_pp), A.dev<float>(o_np), n, win,
                            maxLevel, maxCount, epsilon, flags, minEigThreshold, A.dev<uint8_t>(o_st), A.dev<float>(o_err)))) return rc;
    return A.fetch();
}

int eorb_hamming_window_match(eorb_ctx* c, const uint8_t* q_desc, int nq, int q_stride, const uint8_t* t_desc, int nt, int t_stride,
                              const int32_t* cand_offsets, const int32_t* cand_idx, int32_t* best_idx, int32_t* best_d,
                              int32_t* second_idx, int32_t* second_d)
{
    if (!c) return EORB_E_ARG;
    if (nq < 0 || nt < 0 || q_stride < 32 || t_stride < 32 || (nq > 0 && (!q_desc || !cand_offsets || !best_idx || !best_d || !second_idx || !second_d)))
        return set_err(c, EORB_E_ARG, "hamming_window_match: bad arguments");
    fe_enter(c);
    if (nq == 0) return EORB_OK;
    const int ncand = cand_offsets[nq];
    for (int q = 0; q < nq; q++) if (cand_offsets[q + 1] < cand_offsets[q]) return set_err(c, EORB_E_ARG, "hamming_window_match: offsets not monotone");
    for (int k = 0; k < ncand; k++) if (cand_idx[k] < 0 || cand_idx[k] >= nt) return set_err(c, EORB_E_ARG, "hamming_window_match: candidate %d out of range", cand_idx[k]);
    int rc;
    Arena A(c);
    const size_t o_q = A.in(q_desc, (size_t)q_stride * nq), o_t = A.in(t_desc, (size_t)t_stride * nt);
    const size_t o_off = A.in(cand_offsets, sizeof(int32_t) * ((size_t)nq + 1)), o_cand = A.in(cand_idx, sizeof(int32_t) * (size_t)ncand);
    const size_t q4 = sizeof(int32_t) * (size_t)nq;
    const size_t o_out = A.out(nullptr, 4 * q4);      // best index | best distance | second index | second distance
    A.inout(best_idx, o_out, q4); A.inout(best_d, o_out + q4, q4); A.inout(second_idx, o_out + 2 * q4, q4); A.inout(second_d, o_out + 3 * q4, q4);
    if ((rc = A.upload())) return rc;
    if ((rc = window_match_dev(c, A.dev<uint8_t>(o_q), nq, q_stride, A.dev<uint8_t>(o_t), t_stride, A.dev<int32_t>(o_off),
                               A.dev<int32_t>(o_cand), A.dev<int32_t>(o_out)))) return rc;
    return A.fetch();
}

int eorb_distinctive_descriptors(eorb_ctx* c, const uint8_t* desc, const int32_t* offsets, int M, int32_t* best)
{
    if (!c) return EORB_E_ARG;
    if (M < 0 || (M > 0 && (!offsets || !best))) return set_err(c, EORB_E_ARG, "distinctive_descriptors: bad arguments");
    if (M == 0) return EORB_OK;
    for (int m = 0; m < M; m++) if (offsets[m + 1] < offsets[m]) return set_err(c, EORB_E_ARG, "distinctive_descriptors: offsets not monotone");
    // (distinctive_kernel counts a row's distances in 16-bit bins, two to a 32-bit word: see there)
    if (offsets[0] < 0) return set_err(c, EORB_E_ARG, "distinctive_descriptors: negative offset");
    for (int m = 0; m < M; m++)
        if ((long long)offsets[m + 1] - offsets[m] > 65535)
            return set_err(c, EORB_E_CAPACITY, "distinctive_descriptors: map point %d has %d rows, more than the 65535 a 16-bit bin counts", m, (int)(offsets[m + 1] - offsets[m]));
    fe_enter(c);
    const int n = offsets[M];
    int rc;
    Arena A(c);
    const size_t o_desc = A.in(desc, 32 * (size_t)n), o_off = A.in(offsets, sizeof(int32_t) * (size_t)(M + 1));
    const size_t o_best = A.out(best, sizeof(int32_t) * (size_t)M);
    if ((rc = A.upload())) return rc;
    if ((rc = distinctive_dev(c, A.dev<uint8_t>(o_desc), A.dev<int32_t>(o_off), M, A.dev<int32_t>(o_best)))) return rc;
    return A.fetch();
}

int eorb_sort_by_response(eorb_ctx* c, const eorb_keypoint* kps, int n, int32_t* perm)
{
    if (!c) return EORB_E_ARG;
    if (n < 0 || (n > 0 && (!kps || !perm))) return set_err(c, EORB_E_ARG, "sort_by_response: bad arguments");
    if (n == 0) return EORB_OK;
    fe_enter(c);
    int rc;
    Arena A(c);
    const size_t o_kp = A.in(kps, sizeof(eorb_keypoint) * n), o_perm = A.out(perm, sizeof(int32_t) * n);
    if ((rc = A.upload())) return rc;
    if ((rc = sort_response_dev(c, A.dev<eorb_keypoint>(o_kp), n, A.dev<int32_t>(o_perm)))) return rc;
    return A.fetch();
}

void eorb_resolve_num_mixed(int nDetectedORB, int nDetectedAK, int nDesired, int nDesiredAK, int* nORB, int* nAK)
{   // MixedFrame::resolveNumMixedPts (src/MixedFrame.cpp:281-317): pure count bookkeeping of the container
    const int nDetected = nDetectedORB + nDetectedAK;
    const int nDesiredORB = nDesired - nDesiredAK;
    if (nDetected > nDesired) {
        const int nDiff = nDetected - nDesired;
        if (nDetectedORB > nDesiredORB && nDetectedAK > nDesiredAK) { *nORB = nDesiredORB; *nAK = nDesiredAK; }
        else if (nDetectedORB > nDesiredORB) { *nORB = nDetectedORB - nDiff; *nAK = std::min(nDetectedAK, nDesiredAK); }
        else if (nDetectedAK > nDesiredAK) { *nORB = std::min(nDetectedORB, nDesiredORB); *nAK = nDetectedAK - nDiff; }
    } else { *nORB = nDetectedORB; *nAK = nDetectedAK; }
}

int eorb_hamming_bf_knn2(eorb_ctx* c, const uint8_t* q, int nq, const uint8_t* t, int nt, int32_t* idx2, int32_t* dist2)
{
    if (!c) return EORB_E_ARG;
    if (nq < 0 || nt < 0 || !idx2 || !dist2) return set_err(c, EORB_E_ARG, "bf_knn2: bad arguments");
    if (nq == 0) return EORB_OK;
    fe_enter(c);
    int rc;
    Arena A(c);
    const size_t o_q = A.in(q, 32 * (size_t)nq), o_t = A.in(t, 32 * (size_t)nt);
    const size_t o_idx = A.out(idx2, sizeof(int32_t) * 2 * (size_t)nq), o_dist = A.out(dist2, sizeof(int32_t) * 2 * (size_t)nq);
    if ((rc = A.upload())) return rc;
    rc = bf_knn2_dev(c, A.dev<uint8_t>(o_q), nq, A.dev<uint8_t>(o_t), nt, A.dev<int32_t>(o_idx), A.dev<int32_t>(o_dist));
    if (rc) return rc;
    return A.fetch();
}

// ---- batched HBM-resident front end --------------------------------------------------------------------
int eorb_fe_configure(eorb_ctx* c, const eorb_fe_config* cfg)
{
    if (!c || !cfg) return EORB_E_ARG;
    if (cfg->W <= 0 || cfg->H <= 0 || cfg->max_batch < 1 || cfg->max_events < 0 || !(cfg->sigma > 0.f))
        return set_err(c, EORB_E_ARG, "fe_configure: bad configuration");
    fe_enter(c);
    hipStreamSynchronize(c->stream);
    int rc = orb_configure(c, &cfg->orb, cfg->W, cfg->H);
    if (rc) return rc;
    c->fe = *cfg;
    const size_t B = cfg->max_batch, npix = (size_t)cfg->W * cfg->H, cap = c->orb.max_out;
    if ((rc = ensure(c, c->img_f32, sizeof(float) * npix * B))) return rc;
    if ((rc = ensure(c, c->img_u8, npix * B))) return rc;
    if ((rc = ensure(c, c->minmax, 8 * B + 64))) return rc;
    // working copies owned by the batched path alone (host entry points on the same context never touch them, so the slice
    // carried from batch to batch survives an interleaved eorb_orb_extract / matcher call): slot 0 = previous batch's last slice
    if ((rc = ensure(c, c->fe_prev_kp, sizeof(eorb_keypoint) * cap * (B + 1)))) return rc;
    if ((rc = ensure(c, c->fe_prev_desc, 32 * cap * (B + 1)))) return rc;
    if ((rc = ensure(c, c->fe_prev_n, sizeof(int32_t) * (2 * B + 4)))) return rc;
    if ((rc = ensure(c, c->fe_matches12, sizeof(int32_t) * cap * B))) return rc;
    if ((rc = ensure(c, c->fe_nmatches, sizeof(int32_t) * (B + 1)))) return rc;
    EORB_HIP(c, hipMemsetAsync(c->fe_prev_n.p, 0, sizeof(int32_t) * (2 * B + 4), c->stream));
    c->fe_configured = true;
    c->fe_has_prev = false;
    return EORB_OK;
}

// the batch's user-visible records and the slice carried to the next batch, in one launch (six device-to-device copies cost a
// 3.6 ms step 37 us of launch gaps): segment s copies n[s] bytes (multiples of 4) from src[s] to dst[s]
struct CopySegs { void* dst[6]; const void* src[6]; size_t n[6]; int count; };
__global__ __launch_bounds__(256) void fe_publish_kernel(CopySegs S)
{
    for (int s = 0; s < S.count; s++) {
        const size_t n = S.n[s];
        char* d = (char*)S.dst[s]; const char* q = (const char*)S.src[s];
        if (!(((uintptr_t)d | (uintptr_t)q | n) & 15)) {
            const size_t n16 = n >> 4;
            for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) ((uint4*)d)[i] = ((const uint4*)q)[i];
        } else {
            const size_t n4 = n >> 2;
            for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) ((uint32_t*)d)[i] = ((const uint32_t*)q)[i];
        }
    }
}

static int fe_run_batch_common(eorb_ctx* c, const void* d_events, int raw, const int64_t* h_offsets, int B,
                               uint8_t* d_images, eorb_keypoint* d_kps, uint8_t* d_desc, int32_t* d_nkps,
                               int32_t* d_matches12, int32_t* d_nmatches)
{
    if (!c) return EORB_E_ARG;
    if (!c->fe_configured) return set_err(c, EORB_E_NOTCONF, "fe_run_batch: eorb_fe_configure not called");
    const eorb_fe_config& f = c->fe;
    const bool from_images = raw < 0;                    // (eorb_fe_run_batch_images_dev: the frames are given, nothing to accumulate)
    if (B < 1 || B > f.max_batch || (!h_offsets && !from_images)) return set_err(c, EORB_E_ARG, "fe_run_batch: bad batch size %d", B);
    if (from_images && !d_images) return set_err(c, EORB_E_ARG, "fe_run_batch_images: no images");
    fe_enter(c);
    const size_t npix = (size_t)f.W * f.H, cap = c->orb.max_out;
    uint8_t* img = d_images ? d_images : (uint8_t*)c->img_u8.p;
    // working copies: slot 0 of kp/desc/n holds the last slice of the previous batch (frame-to-frame matching)
    eorb_keypoint* wk = (eorb_keypoint*)c->fe_prev_kp.p;
    uint8_t* wd = (uint8_t*)c->fe_prev_desc.p;
    int32_t* wn = (int32_t*)c->fe_prev_n.p;             // [0] prev, [1..B] this batch, then mono index
    // (the images' normalisation to u8 is left to the extraction's first kernel, which builds level 0 from the float images)
    int rc = from_images ? EORB_OK : ev_accumulate_dev(c, d_events, raw, h_offsets, B, f.W, f.H, f.sigma, f.pol, 0, (float*)c->img_f32.p, img, 0,
                                                       (uint32_t*)c->minmax.p);
    if (rc) return rc;
    rc = orb_extract_dev(c, img, f.W, npix, B, f.lap0, f.lap1, f.want_desc, wk + cap, wd + 32 * cap, nullptr, wn + 1,
                         wn + 1 + f.max_batch + 1, nullptr, from_images ? nullptr : (const float*)c->img_f32.p, from_images ? nullptr : (const uint32_t*)c->minmax.p);
    if (rc) return rc;
    if (f.match && f.want_desc) {
        eorb_grid_bounds gb;
        gb.minX = 0.f; gb.minY = 0.f; gb.maxX = (float)f.W; gb.maxY = (float)f.H;           // Frame.cc:862-866
        gb.invW = (float)kGridCols / (gb.maxX - gb.minX); gb.invH = (float)kGridRows / (gb.maxY - gb.minY);
        const int first = c->fe_has_prev ? 0 : 1;                  // pair p: slice p-1 (slot p) vs slice p (slot p+1)
        const int npairs = B - first;
        int32_t* m12 = d_matches12 ? d_matches12 : (int32_t*)c->fe_matches12.p;
        int32_t* nm = d_nmatches ? d_nmatches : (int32_t*)c->fe_nmatches.p;
        if (!c->fe_has_prev) {
            EORB_HIP(c, hipMemsetAsync(nm, 0, sizeof(int32_t), c->stream));
            EORB_HIP(c, hipMemsetAsync(m12, 0xff, sizeof(int32_t) * cap, c->stream));
        }
        rc = search_init_dev(c, npairs, wk + cap * first, wn + first, cap, wd + 32 * cap * first, 32, 32 * cap, nullptr,
                             wk + cap * (first + 1), wn + first + 1, cap, wd + 32 * cap * (first + 1), 32, 32 * cap, nullptr,
                             (int)cap, (int)cap, gb, nullptr, m12 + cap * first, f.windowSize, f.nnratio, f.checkOri, nm + first);
        if (rc) return rc;
    }
    // user-visible outputs
    // (the carried slice -- the last one into slot 0 for the next batch -- never overlaps what it is copied from: slot B, B >= 1)
    CopySegs S; S.count = 0;
    auto seg = [&](void* d, const void* q, size_t n) { if (d && n) { S.dst[S.count] = d; S.src[S.count] = q; S.n[S.count] = n; S.count++; } };
    seg(d_kps, wk + cap, sizeof(eorb_keypoint) * cap * B);
    seg(d_desc, wd + 32 * cap, 32 * cap * B);
    seg(d_nkps, wn + 1, sizeof(int32_t) * B);
    seg(wk, wk + cap * B, sizeof(eorb_keypoint) * cap);
    seg(wd, wd + 32 * cap * B, 32 * cap);
    seg(wn, wn + B, sizeof(int32_t));
    fe_publish_kernel<<<512, 256, 0, c->stream>>>(S);
    EORB_LAUNCH_CHECK(c, "fe_publish_kernel");
    c->fe_has_prev = true;
    return EORB_OK;
}

int eorb_fe_run_batch_raw4_dev(eorb_ctx* c, const eorb_raw_event4* d_events, const int64_t* h_offsets, int B,
                               uint8_t* d_images, eorb_keypoint* d_kps, uint8_t* d_desc, int32_t* d_nkps,
                               int32_t* d_matches12, int32_t* d_nmatches)
{
    if (c && !c->maps.w) return set_err(c, EORB_E_NOTCONF, "fe_run_batch_raw4: eorb_set_undistort_maps not called");
    return fe_run_batch_common(c, d_events, 3, h_offsets, B, d_images, d_kps, d_desc, d_nkps, d_matches12, d_nmatches);
}

int eorb_fe_run_batch_raw2_dev(eorb_ctx* c, const eorb_raw_event2* d_events, const int64_t* h_offsets, int B,
                               uint8_t* d_images, eorb_keypoint* d_kps, uint8_t* d_desc, int32_t* d_nkps,
                               int32_t* d_matches12, int32_t* d_nmatches)
{
    if (c && !c->maps.w) return set_err(c, EORB_E_NOTCONF, "fe_run_batch_raw2: eorb_set_undistort_maps not called");
    if (c && c->fe_configured && c->fe.pol) return set_err(c, EORB_E_ARG, "fe_run_batch_raw2: the 2-byte record carries no polarity");
    return fe_run_batch_common(c, d_events, 4, h_offsets, B, d_images, d_kps, d_desc, d_nkps, d_matches12, d_nmatches);
}

int eorb_fe_run_batch_dev(eorb_ctx* c, const eorb_event16* d_events, const int64_t* h_offsets, int B,
                          uint8_t* d_images, eorb_keypoint* d_kps, uint8_t* d_desc, int32_t* d_nkps,
                          int32_t* d_matches12, int32_t* d_nmatches)
{
    return fe_run_batch_common(c, d_events, 0, h_offsets, B, d_images, d_kps, d_desc, d_nkps, d_matches12, d_nmatches);
}

int eorb_fe_run_batch_raw_dev(eorb_ctx* c, const eorb_raw_event* d_events, const int64_t* h_offsets, int B,
                              uint8_t* d_images, eorb_keypoint* d_kps, uint8_t* d_desc, int32_t* d_nkps,
                              int32_t* d_matches12, int32_t* d_nmatches)
{
    if (c && !c->maps.w) return set_err(c, EORB_E_NOTCONF, "fe_run_batch_raw: eorb_set_undistort_maps not called");
    return fe_run_batch_common(c, d_events, 1, h_offsets, B, d_images, d_kps, d_desc, d_nkps, d_matches12, d_nmatches);
}

int eorb_fe_last_f32_dev(eorb_ctx* c, const float** d_f32, float* h_minmax, int B)
{
    if (!c) return EORB_E_ARG;
    if (!c->fe_configured || !c->img_f32.p) return set_err(c, EORB_E_NOTCONF, "fe_last_f32: eorb_fe_configure not called");
    if (B < 0 || B > c->fe.max_batch) return set_err(c, EORB_E_ARG, "fe_last_f32: bad batch size %d", B);
    if (d_f32) *d_f32 = (const float*)c->img_f32.p;
    if (h_minmax && B) {
        fe_enter(c);
        const size_t nenc = 2 * (size_t)B;
        const uint32_t* enc = (const uint32_t*)pinned(c, sizeof(uint32_t) * nenc);      // (2 x max_batch words: more than readback_buf holds)
        if (!enc) return set_err(c, EORB_E_HIP, "pinned alloc failed");
        EORB_HIP(c, hipMemcpyAsync((void*)enc, c->minmax.p, sizeof(uint32_t) * nenc, hipMemcpyDeviceToHost, c->stream));
        pinned_commit(c, true);
        EORB_HIP(c, fe_stream_sync(c));
        for (size_t k = 0; k < nenc; k++) {                 // the order-preserving integer encoding of the gather kernels' atomics
            const uint32_t e = enc[k], u = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
            memcpy(&h_minmax[k], &u, 4);
        }
    }
    return EORB_OK;
}

int eorb_fe_run_batch_images_dev(eorb_ctx* c, const uint8_t* d_images, int B, eorb_keypoint* d_kps, uint8_t* d_desc, int32_t* d_nkps,
                                 int32_t* d_matches12, int32_t* d_nmatches)
{
    return fe_run_batch_common(c, nullptr, -1, nullptr, B, const_cast<uint8_t*>(d_images), d_kps, d_desc, d_nkps, d_matches12, d_nmatches);
}

}  // extern "C"
