// kfdb.hip -- KeyFrameDatabase on gfx950: DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:783-895) and DetectNBestCandidates
// (:612-780) without an inverted file.  add() (:39-45) appends a keyframe to the list of every one of its words in the same call, so two
// keyframes stand in the same relative order in every list: that of their latest add.  The walk over the query's words therefore meets
// a keyframe first at its smallest common word, and lKFsSharingWords is the listed keyframes ordered by (smallest common word, add
// sequence).  The device keeps each live keyframe's BowVector (word ids ascending, double values) and its sequence number.
//
// A query is three launches whatever the size of the database:
//   kfdb_count_kernel   one wavefront per slot: shared-word count, smallest common word, listed flag; maxCommonWords by atomic max
//   kfdb_score_kernel   one wavefront per slot over the 0.8 threshold: L1Scoring::score, its terms added in word order in double
//   kfdb_finish_kernel  one workgroup: list order, covisibility accumulation, the 0.75 rule / the stable sort by accScore
#include "kfdb.h"
#include <string.h>
#include <algorithm>

namespace eorb {

struct KfdbDev { const KfdbSlot* tab; const uint32_t* words; const double* vals; float* score; };

constexpr int kCountWaves = 4;          // slots per workgroup of the count / score kernels
constexpr int kFinishThreads = 1024;
constexpr int kFinishLds = 4096;        // scored entries the finish kernel sorts in LDS (12 bytes each); more are sorted in global memory

// index of w in the ascending q[0, n), -1 if absent
__device__ __forceinline__ int kfdb_find(const uint32_t* q, int n, uint32_t w)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (q[mid] < w) lo = mid + 1; else hi = mid; }
    return (lo < n && q[lo] == w) ? lo : -1;
}

__device__ __forceinline__ void kfdb_stage_query(uint32_t* qw, const uint32_t* q_word, int nq)
{
    for (int i = threadIdx.x; i < nq; i += blockDim.x) qw[i] = q_word[i];
    __syncthreads();
}

// :791-806 / :624-653: mnRelocWords / mnPlaceRecognitionWords = the query's words present in the keyframe's vector; a keyframe of
// spConnectedKF is never listed (its query id is never set, :635-645)
__global__ __launch_bounds__(kCountWaves * 64) void kfdb_count_kernel(KfdbDev db, KfdbQuery q)
{
    __shared__ uint32_t qw[kKfdbMaxQueryWords];
    kfdb_stage_query(qw, q.q_word, q.nq);
    const int lane = threadIdx.x & 63, slot = blockIdx.x * kCountWaves + (threadIdx.x >> 6);
    if (slot >= q.n_slots) return;
    const KfdbSlot rec = db.tab[slot];
    int cnt = 0; uint32_t first = 0xffffffffu;
    const uint32_t qmax = qw[q.nq - 1];
    for (int base = 0; base < rec.n; base += 64) {
        const int i = base + lane;
        uint32_t w = 0; bool found = false;
        if (i < rec.n) { w = db.words[rec.off + i]; found = kfdb_find(qw, q.nq, w) >= 0; }
        const uint64_t m = __ballot(found);
        if (m) {
            if (!cnt) first = (uint32_t)__shfl((int)w, __ffsll((unsigned long long)m) - 1, 64);
            cnt += __popcll(m);
        }
        if ((uint32_t)__shfl((int)(i < rec.n ? w : 0xffffffffu), 63, 64) >= qmax) break;      // the rest is past the query's last word
    }
    if (lane == 0) {
        const bool listed = rec.n >= 0 && cnt > 0 && !(q.exclude && q.exclude[slot]);
        q.cnt[slot] = cnt; q.first[slot] = first; q.listed[slot] = listed ? 1 : 0;
        if (listed) { atomicAdd(&q.hdr[0], 1); atomicMax(&q.hdr[2], cnt); }
    }
}

// :812-837 / :659-684 and L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68): the sum runs over the common words in
// ascending word order, one term fabs(vi - wi) - fabs(vi) - fabs(wi) at a time, in double; the lower_bound jumps only skip the rest
__global__ __launch_bounds__(kCountWaves * 64) void kfdb_score_kernel(KfdbDev db, KfdbQuery q)
{
    __shared__ uint32_t qw[kKfdbMaxQueryWords];
    kfdb_stage_query(qw, q.q_word, q.nq);
    const int lane = threadIdx.x & 63, slot = blockIdx.x * kCountWaves + (threadIdx.x >> 6);
    if (slot >= q.n_slots || !q.listed[slot]) return;
    const int maxCommonWords = q.hdr[2];
    const int minCommonWords = (int)((float)maxCommonWords * 0.8f);
    if (!(q.cnt[slot] > minCommonWords)) return;
    const KfdbSlot rec = db.tab[slot];
    double score = 0;
    for (int base = 0; base < rec.n; base += 64) {
        const int i = base + lane;
        double term = 0; bool found = false;
        if (i < rec.n) {
            const int k = kfdb_find(qw, q.nq, db.words[rec.off + i]);
            if (k >= 0) { const double vi = q.q_val[k], wi = db.vals[rec.off + i]; term = fabs(vi - wi) - fabs(vi) - fabs(wi); found = true; }
        }
        uint64_t m = __ballot(found);
        while (m) {                                    // the order of this sum is the contract: every lane adds the same terms, lane by lane
            const int l = __ffsll((unsigned long long)m) - 1;
            score += __shfl(term, l, 64);
            m &= m - 1;
        }
    }
    if (lane == 0) {
        score = -score / 2.0;
        const float si = (float)score;
        q.si_slot[slot] = si;
        db.score[slot] = si;                           // mRelocScore / mPlaceRecognitionScore
        const int pos = atomicAdd(&q.hdr[1], 1);
        q.key[pos] = ((uint64_t)q.first[slot] << 32) | rec.seq;
        q.kslot[pos] = (uint32_t)slot;
    }
}

// ascending bitonic sort of K[0, n) (n a power of two) by one workgroup, V (may be NULL) carried along
__device__ void kfdb_sort(uint64_t* K, uint32_t* V, int n)
{
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                const int l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0;
                    const uint64_t a = K[i], b = K[l];
                    if ((a > b) == up) {
                        K[i] = b; K[l] = a;
                        if (V) { const uint32_t t = V[i]; V[i] = V[l]; V[l] = t; }
                    }
                }
            }
            __syncthreads();
        }
}

// descending float order as an ascending integer; -0.0 and 0.0 compare equal under compFirst (:606-609)
__device__ __forceinline__ uint32_t kfdb_desc_key(float f)
{
    uint32_t u = __float_as_uint(f == 0.f ? 0.f : f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

__global__ __launch_bounds__(kFinishThreads) void kfdb_finish_kernel(KfdbDev db, KfdbQuery q)
{
    __shared__ uint64_t s_key[kFinishLds];
    __shared__ uint32_t s_slot[kFinishLds];
    __shared__ float s_red[kFinishThreads];
    const int S = q.hdr[1], tid = threadIdx.x;
    if (S <= 0) return;
    int npad = 1;
    while (npad < S) npad <<= 1;
    const bool lds = npad <= kFinishLds && npad <= q.lds_cap;
    uint64_t* K = lds ? s_key : q.key;
    uint32_t* V = lds ? s_slot : q.kslot;
    for (int i = tid; i < npad; i += kFinishThreads) {
        if (i >= S) K[i] = ~0ull;
        else if (lds) { K[i] = q.key[i]; V[i] = q.kslot[i]; }
    }
    __syncthreads();
    kfdb_sort(K, V, npad);                             // lScoreAndMatch order: the listed order, of which the scored entries are a subsequence
    if (S > q.cap) return;                             // the caller's arrays are too short: only the counts are returned
    for (int e = tid; e < S; e += kFinishThreads) {
        const int slot = (int)V[e];
        q.o_slot[e] = slot; q.o_si[e] = q.si_slot[slot]; q.o_words[e] = q.cnt[slot];
    }
    if (!q.covis) return;
    // :846-871 / :693-718: up to ten best covisible keyframes in their order; one counts when it is listed in this query, and what is
    // added is its stored score -- the last one written, by this query or an earlier one
    float best_acc = 0.f;
    for (int e = tid; e < S; e += kFinishThreads) {
        const int slot = (int)V[e];
        float bestScore = q.si_slot[slot], accScore = bestScore;
        int pBest = slot;
        for (int j = 0; j < kKfdbCovis; j++) {
            const int nb = q.covis[(size_t)slot * kKfdbCovis + j];
            if (nb < 0 || nb >= q.n_slots || !q.listed[nb]) continue;
            const float s2 = db.score[nb];
            accScore += s2;
            if (s2 > bestScore) { pBest = nb; bestScore = s2; }
        }
        q.o_acc[e] = accScore; q.o_best[e] = pBest;
        if (accScore > best_acc) best_acc = accScore;
    }
    s_red[tid] = best_acc;
    __syncthreads();
    for (int o = kFinishThreads / 2; o > 0; o >>= 1) {
        if (tid < o && s_red[tid + o] > s_red[tid]) s_red[tid] = s_red[tid + o];
        __syncthreads();
    }
    best_acc = s_red[0];                               // (>= +0.0: every partial maximum started there)
    if (tid == 0) q.hdr[3] = (int32_t)__float_as_uint(best_acc);
    if (!q.nbest) {
        const float minScoreToRetain = 0.75f * best_acc;                       // :874
        for (int e = tid; e < S; e += kFinishThreads) q.o_keep[e] = q.o_acc[e] > minScoreToRetain ? 1 : 0;
        return;
    }
    // :722 lAccScoreAndMatch.sort(compFirst): stable, descending accScore -> key (accScore descending, list position)
    __syncthreads();
    for (int i = tid; i < npad; i += kFinishThreads) K[i] = i < S ? (((uint64_t)kfdb_desc_key(q.o_acc[i]) << 32) | (uint32_t)i) : ~0ull;
    __syncthreads();
    kfdb_sort(K, nullptr, npad);
    for (int i = tid; i < S; i += kFinishThreads) {
        const int e = (int)(uint32_t)K[i];
        q.o_sacc[i] = q.o_acc[e]; q.o_sbest[i] = q.o_best[e];
    }
}

// K new vectors from the call's arena into the pools; both stored scores start at 0
__global__ __launch_bounds__(256) void kfdb_add_kernel(KfdbSlot* tab, uint32_t* words, double* vals, float* score0, float* score1, const int32_t* slot_of,
                                                       const KfdbSlot* rec_of, const int32_t* src_of, const uint32_t* src_word, const double* src_val)
{
    const int k = blockIdx.x, slot = slot_of[k];
    const KfdbSlot rec = rec_of[k];
    const int src = src_of[k];
    for (int i = threadIdx.x; i < rec.n; i += blockDim.x) { words[rec.off + i] = src_word[src + i]; vals[rec.off + i] = src_val[src + i]; }
    if (threadIdx.x == 0) { tab[slot] = rec; score0[slot] = 0.f; score1[slot] = 0.f; }
}

__global__ void kfdb_erase_kernel(KfdbSlot* tab, int slot) { if (threadIdx.x == 0) tab[slot] = KfdbSlot{0u, -1, 0u, 0u}; }

// pool growth: every live vector from its old place to its new one
__global__ __launch_bounds__(256) void kfdb_compact_kernel(const KfdbSlot* old_tab, const KfdbSlot* new_tab, const uint32_t* ow, const double* ov, uint32_t* nw, double* nv)
{
    const KfdbSlot a = old_tab[blockIdx.x], b = new_tab[blockIdx.x];
    for (int i = threadIdx.x; i < b.n; i += blockDim.x) { nw[b.off + i] = ow[a.off + i]; nv[b.off + i] = ov[a.off + i]; }
}

static void kfdb_drop(DevBuf& b) { if (b.p) hipFree(b.p); b.p = nullptr; b.cap = 0; }

void kfdb_free(eorb_ctx* c)
{
    KfdbState& s = c->kfdb;
    kfdb_drop(s.tab); kfdb_drop(s.words); kfdb_drop(s.vals); kfdb_drop(s.score[0]); kfdb_drop(s.score[1]);
    s = KfdbState{};
}

// a larger buffer with the first `live` bytes of the old one
static int kfdb_grow(eorb_ctx* c, DevBuf& b, size_t bytes, size_t live)
{
    DevBuf n;
    int rc = ensure(c, n, bytes);
    if (rc) return rc;
    if (live) EORB_HIP(c, hipMemcpyAsync(n.p, b.p, live, hipMemcpyDeviceToDevice, c->stream));
    EORB_HIP(c, hipStreamSynchronize(c->stream));
    kfdb_drop(b);
    b = n;
    return EORB_OK;
}

int kfdb_reserve(eorb_ctx* c, int new_slots, int64_t new_words)
{
    KfdbState& s = c->kfdb;
    int rc;
    const int first_slots = c->opt.kfdb_initial_slots > 0 ? c->opt.kfdb_initial_slots : 1024;
    const int want_slots = s.n_slots + new_slots;           // (an upper bound: free slots are reused first)
    if (want_slots > s.slot_cap) {
        int cap = std::max(s.slot_cap, first_slots);
        while (cap < want_slots) cap *= 2;
        cap = std::min(cap, kKfdbMaxSlots);
        if ((rc = kfdb_grow(c, s.tab, sizeof(KfdbSlot) * (size_t)cap, sizeof(KfdbSlot) * (size_t)s.n_slots))) return rc;
        for (int f = 0; f < 2; f++) if ((rc = kfdb_grow(c, s.score[f], sizeof(float) * (size_t)cap, sizeof(float) * (size_t)s.n_slots))) return rc;
        s.slot_cap = cap;
    }
    if (s.word_used + new_words <= s.word_cap) return EORB_OK;
    // the pools are append-only between growths: what erase() left behind is dropped here, the live vectors move up in slot order
    const int64_t want = s.word_live + new_words;
    int64_t cap = std::max<int64_t>(s.word_cap, 64 * (int64_t)first_slots);
    while (cap < 2 * want) cap *= 2;
    if (cap >= ((int64_t)1 << 31)) return set_err(c, EORB_E_CAPACITY, "kfdb: the word pool would pass 2^31 entries");
    DevBuf nw, nv, ntab;
    if ((rc = ensure(c, nw, sizeof(uint32_t) * (size_t)cap)) || (rc = ensure(c, nv, sizeof(double) * (size_t)cap))) { kfdb_drop(nw); kfdb_drop(nv); return rc; }
    std::vector<KfdbSlot> t = s.h_tab;
    int64_t used = 0;
    for (int i = 0; i < s.n_slots; i++) if (t[i].n >= 0) { t[i].off = (uint32_t)used; used += t[i].n; }
    if (s.n_live > 0) {
        const size_t tb = sizeof(KfdbSlot) * (size_t)s.n_slots;
        if ((rc = ensure(c, ntab, sizeof(KfdbSlot) * (size_t)s.slot_cap))) { kfdb_drop(nw); kfdb_drop(nv); return rc; }
        void* hp = pinned(c, tb);
        if (!hp) { kfdb_drop(nw); kfdb_drop(nv); kfdb_drop(ntab); return set_err(c, EORB_E_HIP, "pinned alloc failed"); }
        memcpy(hp, t.data(), tb);
        hipError_t e = hipMemcpyAsync(ntab.p, hp, tb, hipMemcpyHostToDevice, c->stream);
        pinned_commit(c, true);
        if (e == hipSuccess) {
            kfdb_compact_kernel<<<s.n_slots, 256, 0, c->stream>>>((const KfdbSlot*)s.tab.p, (const KfdbSlot*)ntab.p, (const uint32_t*)s.words.p, (const double*)s.vals.p,
                                                                  (uint32_t*)nw.p, (double*)nv.p);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        pinned_release_lazy(c);
        if (e != hipSuccess) { kfdb_drop(nw); kfdb_drop(nv); kfdb_drop(ntab); return hip_check(c, e, "kfdb pool growth"); }
        kfdb_drop(s.tab); s.tab = ntab;
    } else EORB_HIP(c, hipStreamSynchronize(c->stream));
    kfdb_drop(s.words); kfdb_drop(s.vals);
    s.words = nw; s.vals = nv; s.word_cap = cap; s.word_used = used; s.h_tab = t;
    return EORB_OK;
}

int kfdb_add_dev(eorb_ctx* c, int K, const int32_t* d_slot, const KfdbSlot* d_rec, const int32_t* d_src, const uint32_t* d_word, const double* d_val)
{
    KfdbState& s = c->kfdb;
    ProfScope ps(c, "kfdb_add");
    kfdb_add_kernel<<<K, 256, 0, c->stream>>>((KfdbSlot*)s.tab.p, (uint32_t*)s.words.p, (double*)s.vals.p, (float*)s.score[0].p, (float*)s.score[1].p,
                                              d_slot, d_rec, d_src, d_word, d_val);
    EORB_LAUNCH_CHECK(c, "kfdb_add_kernel");
    return EORB_OK;
}

int kfdb_erase_dev(eorb_ctx* c, int slot)
{
    kfdb_erase_kernel<<<1, 64, 0, c->stream>>>((KfdbSlot*)c->kfdb.tab.p, slot);
    EORB_LAUNCH_CHECK(c, "kfdb_erase_kernel");
    return EORB_OK;
}

int kfdb_query_dev(eorb_ctx* c, const KfdbQuery& q)
{
    KfdbState& s = c->kfdb;
    const KfdbDev db{(const KfdbSlot*)s.tab.p, (const uint32_t*)s.words.p, (const double*)s.vals.p, (float*)s.score[q.family].p};
    const int blocks = (q.n_slots + kCountWaves - 1) / kCountWaves;
    { ProfScope ps(c, "kfdb_count");
      kfdb_count_kernel<<<blocks, kCountWaves * 64, 0, c->stream>>>(db, q);
      EORB_LAUNCH_CHECK(c, "kfdb_count_kernel"); }
    { ProfScope ps(c, "kfdb_score");
      kfdb_score_kernel<<<blocks, kCountWaves * 64, 0, c->stream>>>(db, q);
      EORB_LAUNCH_CHECK(c, "kfdb_score_kernel"); }
    { ProfScope ps(c, "kfdb_finish");
      kfdb_finish_kernel<<<1, kFinishThreads, 0, c->stream>>>(db, q);
      EORB_LAUNCH_CHECK(c, "kfdb_finish_kernel"); }
    return EORB_OK;
}

}  // namespace eorb
