// match.hip -- 256-bit Hamming matchers on gfx950 (wavefront __popcll), bit-exact w.r.t. the reference's
// sequential matchers.
//
//   bf_knn2_kernel        brute-force 2-NN (cv::BFMatcher::knnMatch(.,.,2) at src/Frame.cc:1228):
//                         16 lanes share one query and stride over an LDS-staged train tile; the two
//                         smallest (dist, trainIdx) keys are merged with shuffles.
//   search_init_kernel    ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:714-831) /
//                         MixedMatcher (src/MixedMatcher.cpp:20-145).  The reference is a greedy
//                         sequential loop whose state (vMatchedDistance, vnMatches21) feeds later
//                         queries, so queries stay sequential; the candidate scan of each query
//                         (Frame::GetFeaturesInArea, src/Frame.cc:710-781 + DescriptorDistance,
//                         ORBmatcher.cc:2360-2378) is spread over the 256 threads of a workgroup.
//                         Tie-breaks follow the reference's candidate order (cell ix, cell iy,
//                         insertion index) through a composed sort key.
//   search_proj_*_kernel  the two tracking SearchByProjection variants (ORBmatcher.cc:44-219,
//                         :1969-2187), same structure.
// One workgroup per frame pair; batches of pairs run concurrently.
#include "eorb_ctx.h"
#include "match_args.h"
#include "dev_math.h"
#include "kb8_dev.h"
#include <algorithm>
#include <type_traits>

namespace eorb {

constexpr int TH_HIGH = 100, TH_LOW = 50, HISTO_LENGTH = 30;      // ORBmatcher.cc:36-38

// ---------------------------------------------------------------------------------------------------
// brute force 2-NN.  LPQ lanes share a query (16, 32 or 64: 16 / 8 / 4 queries per workgroup); the launcher picks the widest
// sharing that still gives every CU a workgroup (2 000 queries: 125 workgroups at 16 lanes per query, 500 at 64)
template <int LPQ>
__global__ __launch_bounds__(256) void bf_knn2_kernel(const uint8_t* __restrict__ q, int nq,
                                                      const uint8_t* __restrict__ t, int nt,
                                                      int32_t* __restrict__ idx2, int32_t* __restrict__ dist2,
                                                      const int32_t* __restrict__ lap = nullptr)
{
    __shared__ uint64_t tile[256 * 4];
    if (lap) {
        // the lapping rows of a two-camera frame, counts read on the device: lap = {nL, nR, monoLeft, monoRight} (orb_extract_dev's
        // n / mono outputs); queries = left rows monoLeft.., train = right rows monoRight.. (ComputeStereoFishEyeMatches, Frame.cc:1216-1228)
        const int mq = lap[2], mt = lap[3];
        q += (size_t)mq * 32; nq = max(lap[0] - mq, 0);
        t += (size_t)mt * 32; nt = max(lap[1] - mt, 0);
    }
    const int tid = threadIdx.x;
    const int part = tid & (LPQ - 1);
    const int qi = blockIdx.x * (256 / LPQ) + tid / LPQ;
    uint64_t qa[4] = {0, 0, 0, 0};
    if (qi < nq) {
        const uint64_t* qp = (const uint64_t*)(q + (size_t)qi * 32);
        qa[0] = qp[0]; qa[1] = qp[1]; qa[2] = qp[2]; qa[3] = qp[3];
    }
    // keys: dist << 32 | trainIdx ; smaller key = better; ties -> lowest train index
    uint64_t k0 = ~0ull, k1 = ~0ull;
    for (int t0 = 0; t0 < nt; t0 += 256) {
        const int nload = min(256, nt - t0);
        __syncthreads();
        if (tid < nload) {
            const uint64_t* tp = (const uint64_t*)(t + (size_t)(t0 + tid) * 32);
            tile[tid * 4 + 0] = tp[0]; tile[tid * 4 + 1] = tp[1]; tile[tid * 4 + 2] = tp[2]; tile[tid * 4 + 3] = tp[3];
        }
        __syncthreads();
        for (int j = part; j < nload; j += LPQ) {
            const uint64_t* tp = &tile[j * 4];
            const int d = __popcll(qa[0] ^ tp[0]) + __popcll(qa[1] ^ tp[1]) + __popcll(qa[2] ^ tp[2]) + __popcll(qa[3] ^ tp[3]);
            const uint64_t key = ((uint64_t)d << 32) | (uint32_t)(t0 + j);
            if (key < k0) { k1 = k0; k0 = key; }
            else if (key < k1) k1 = key;
        }
    }
    // merge the LPQ partial top-2 lists of a query
#pragma unroll
    for (int d = LPQ / 2; d >= 1; d >>= 1) {
        const uint64_t o0 = __shfl_xor(k0, d, 64), o1 = __shfl_xor(k1, d, 64);
        // top-2 of {k0,k1,o0,o1}
        const uint64_t lo = k0 < o0 ? k0 : o0;
        const uint64_t hi = k0 < o0 ? o0 : k0;
        const uint64_t s = k1 < o1 ? k1 : o1;
        k0 = lo; k1 = hi < s ? hi : s;
    }
    if (part == 0 && qi < nq) {
        idx2[2 * qi] = (k0 == ~0ull) ? -1 : (int32_t)(k0 & 0xffffffffu);
        dist2[2 * qi] = (k0 == ~0ull) ? 0x7fffffff : (int32_t)(k0 >> 32);
        idx2[2 * qi + 1] = (k1 == ~0ull) ? -1 : (int32_t)(k1 & 0xffffffffu);
        dist2[2 * qi + 1] = (k1 == ~0ull) ? 0x7fffffff : (int32_t)(k1 >> 32);
    }
}


// 32 descriptor bytes -> 4 x u64 (little endian).  AKAZE rows are 61 B apart (src/MixedFrame.cpp:20-21), so a
// row may start at any byte: assemble bytewise unless 8-byte aligned.
__device__ __forceinline__ void load_desc32(const uint8_t* __restrict__ p, uint64_t& a, uint64_t& b, uint64_t& c, uint64_t& d)
{
    if ((((uintptr_t)p) & 7) == 0) {
        const uint64_t* q = (const uint64_t*)p;
        a = q[0]; b = q[1]; c = q[2]; d = q[3];
    } else {
        uint64_t v[4];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            uint64_t x = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) x |= (uint64_t)p[w * 8 + k] << (8 * k);
            v[w] = x;
        }
        a = v[0]; b = v[1]; c = v[2]; d = v[3];
    }
}

// ---------------------------------------------------------------------------------------------------
// shared pieces of the greedy window matchers

__device__ __forceinline__ int rot_bin(float a1, float a2)
{   // ORBmatcher.cc:790-796
    const float factor = 1.0f / HISTO_LENGTH;
    float rot = a1 - a2;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

// Frame::GetFeaturesInArea cell range (src/Frame.cc:722-745); returns false when the reference returns empty
__device__ __forceinline__ bool cell_range(const GridB& g, float x, float y, float r, int& cx0, int& cx1, int& cy0, int& cy1)
{
    // the reference's x86 converts NaN and every value outside int32 to INT_MIN: an upper cell index of 2^31 or more (an infinite or
    // huge radius) is negative there and the area empty, where the bare conversion saturates and would search the whole grid
    // Only the upper indices need the test.  With r >= 0 a lower index that passes 2^31 is followed by an upper one that does, and
    // both machines return "empty".  With r < 0 the lower one can pass 2^31 alone: x86 then makes cx0 = 0 and walks cells where this
    // returns "empty" -- but |dx| < r is false for every keypoint when r <= 0, so the reference's walk finds nothing either.
    cx0 = max(0, (int)floorf((x - g.minX - r) * g.invW));
    if (cx0 >= kGridCols) return false;
    const float fx1 = ceilf((x - g.minX + r) * g.invW);
    if (!(fx1 >= 0.f && fx1 < 2147483648.f)) return false;
    cx1 = min(kGridCols - 1, (int)fx1);
    cy0 = max(0, (int)floorf((y - g.minY - r) * g.invH));
    if (cy0 >= kGridRows) return false;
    const float fy1 = ceilf((y - g.minY + r) * g.invH);
    if (!(fy1 >= 0.f && fy1 < 2147483648.f)) return false;
    cy1 = min(kGridRows - 1, (int)fy1);
    return true;
}

// block-wide top-2 of 64-bit keys (smaller = better). Result valid in all threads.
__device__ __forceinline__ void block_top2(uint64_t& k0, uint64_t& k1, uint64_t* red /* 2*nwaves */)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o0 = __shfl_xor(k0, d, 64), o1 = __shfl_xor(k1, d, 64);
        const uint64_t lo = k0 < o0 ? k0 : o0;
        const uint64_t hi = k0 < o0 ? o0 : k0;
        const uint64_t s = k1 < o1 ? k1 : o1;
        k0 = lo; k1 = hi < s ? hi : s;
    }
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[2 * w] = k0; red[2 * w + 1] = k1; }
    __syncthreads();
    uint64_t a0 = red[0], a1 = red[1];
    for (int i = 1; i < nw; i++) {
        const uint64_t o0 = red[2 * i], o1 = red[2 * i + 1];
        const uint64_t lo = a0 < o0 ? a0 : o0;
        const uint64_t hi = a0 < o0 ? o0 : a0;
        const uint64_t s = a1 < o1 ? a1 : o1;
        a0 = lo; a1 = hi < s ? hi : s;
    }
    k0 = a0; k1 = a1;
}

// ComputeThreeMaxima (ORBmatcher.cc:2314-2355)
// (selects on locals: the if / else-if ladder over reference arguments was compiled to 150 scratch accesses per thread)
__device__ __forceinline__ void three_maxima(const int* histo, int L, int& ind1, int& ind2, int& ind3)
{
    int max1 = 0, max2 = 0, max3 = 0;
    int a = -1, b = -1, c = -1;
    for (int i = 0; i < L; i++) {
        const int s = histo[i];
        const bool g1 = s > max1, g2 = s > max2, g3 = s > max3;      // (max1 >= max2 >= max3: g1 implies g2 implies g3)
        c = g2 ? b : (g3 ? i : c); max3 = g2 ? max2 : (g3 ? s : max3);
        b = g1 ? a : (g2 ? i : b); max2 = g1 ? max1 : (g2 ? s : max2);
        a = g1 ? i : a;            max1 = g1 ? s : max1;
    }
    if ((float)max2 < 0.1f * (float)max1) { b = -1; c = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { c = -1; }
    ind1 = a; ind2 = b; ind3 = c;
}

__device__ __forceinline__ int kp_level(const eorb_keypoint& k, bool isorb)
{   // Frame::getKPtLevelMono / MixedFrame::getKPtLevelMono (MixedFrame.cpp:438-446)
    return isorb ? k.octave : k.class_id;
}

// ---------------------------------------------------------------------------------------------------
// The greedy window matchers: ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:714-831, MixedMatcher.cpp:20-145), the two
// tracking SearchByProjection variants (ORBmatcher.cc:44-219, :1969-2187; MixedMatcher.cpp:500-926) and the relocalisation variant
// (:2189-2312), mono branches.  The reference walks the queries in order because a query's outcome depends on what earlier queries
// matched (vMatchedDistance / vnMatches21; setMapPoint -> "holds an observed map point").  That state only FILTERS candidates; the
// expensive part -- Frame::GetFeaturesInArea (src/Frame.cc:710-781) + DescriptorDistance (ORBmatcher.cc:2360-2378) over the window
// -- does not depend on it.  Two phases:
//   win_cand_kernel     every (query, candidate) pair in parallel: one wavefront per query, lanes over the searched frame (staged in
//                       LDS), window / level / type tests, distance; the candidates whose distance can still influence the outcome
//                       (dist < dmax, see the launchers) form the query's list, sorted by key = dist | cell | index | level: the
//                       reference's candidate order (cell ix, cell iy, insertion index) rides in the key for the tie-breaks.
//   win_resolve_kernel  one wavefront per frame pair walks the queries in order: the (short) list of a query is filtered by the
//                       current state, the two smallest keys found by a wave reduction, the greedy update applied.  Everything it
//                       touches sits in LDS; the rotation histogram (ComputeThreeMaxima, :2314-2355) is filled afterwards in
//                       parallel from the recorded (query, match) pairs (a count is order-independent).
// A query whose list outgrows its capacity (or the pair's pool) is resolved by a full scan of the searched frame inside phase 2.
constexpr uint32_t kWinOver = 0xFFFFFFFFu;        // cnt value: list overflowed, resolve by a full scan

struct WinArgs {
    // searched frame (per pair: pointer + pair * stride)
    const eorb_keypoint* kps2; size_t kp2_stride; const int32_t* n2p; int n2; const uint8_t* desc2; int dstride2; size_t desc2_slice;
    const uint8_t* is_orb2; int cap2;
    // queries
    const int32_t* nqp; int nq; int capq;
    // SearchForInitialization: queries = keypoints of frame 1
    const eorb_keypoint* kps1; size_t kp1_stride; const uint8_t* desc1; int dstride1; size_t desc1_slice; const uint8_t* is_orb1;
    float* prev_matched; int windowSize;
    // SearchByProjection: queries = last-frame keypoints / map points
    const eorb_keypoint* qkps; const uint8_t* q_is_orb; const uint8_t* valid; const float* qf; const int32_t* qlevel;
    const uint8_t* mp_desc; const uint8_t* mp_obs; const uint8_t* mp_is_orb; float th; int mode; int dist_th;
    // stereo gate (src/ORBmatcher.cc:96-104, :2056-2062): uright2 = mvuRight of the searched frame's keypoints (> 0: has a right match),
    // q_ur = the query's right coordinate (mTrackProjXR, or uv.x - mbf * invzc); both NULL in the mono configurations
    const float* uright2; const float* q_ur;
    GridB g; float nnratio; int checkOri;
    int dmax;                  // phase 1 keeps candidates with dist < dmax
    int wcap;                  // list capacity of one query
    int lds_ents;              // entries of a pair that phase 2 holds in LDS
    // phase-1 products (per pair)
    uint64_t* ent; int ecap; uint32_t* off; uint32_t* cnt; uint32_t* total;
    // results
    int32_t* matches12; int32_t* slot_mp; int32_t* nmatches;
};

struct WinQuery {              // wave-uniform description of one query
    bool active;
    float qx, qy, r;
    int minLevel, maxLevel;
    bool isorb;
    uint64_t d0, d1, d2, d3;
    float ur; bool has_ur;            // stereo: the query's right coordinate
};

// searched-frame record: cell (16 bits, 0xFFFF = PosInGrid false) | level (8 bits, signed) << 16 | isORB << 24
__device__ __forceinline__ uint32_t f2_info(const eorb_keypoint& k, bool isorb, const GridB& g)
{
    // Frame::PosInGrid (Frame.cc:783-793)
    const int px = dev_round_index((k.x - g.minX) * g.invW);       // (a NaN keypoint is outside the grid, as on x86)
    const int py = dev_round_index((k.y - g.minY) * g.invH);
    const uint32_t cell = (px < 0 || px >= kGridCols || py < 0 || py >= kGridRows) ? 0xFFFFu : (uint32_t)(px * kGridRows + py);
    return cell | ((uint32_t)(kp_level(k, isorb) & 0xff) << 16) | ((uint32_t)isorb << 24);
}

// KIND 0: SearchForInitialization; 1: SearchByProjection(cur, last) / (cur, KeyFrame); 2: SearchByProjection(F, map points)
template <int KIND>
__device__ __forceinline__ WinQuery win_query(const WinArgs& A, int pair, int q)
{
    WinQuery Q;
    Q.active = true; Q.minLevel = Q.maxLevel = 0; Q.qx = Q.qy = Q.r = 0.f; Q.isorb = true; Q.d0 = Q.d1 = Q.d2 = Q.d3 = 0;
    Q.ur = 0.f; Q.has_ur = false;
    if (KIND == 0) {
        const eorb_keypoint k1 = A.kps1[(size_t)pair * A.kp1_stride + q];
        Q.isorb = A.is_orb1 ? A.is_orb1[(size_t)pair * A.capq + q] != 0 : true;
        const int level1 = kp_level(k1, Q.isorb);
        if (level1 > 0) { Q.active = false; return Q; }                                  // :730-732
        const float* PM = A.prev_matched ? A.prev_matched + ((size_t)pair * A.capq + q) * 2 : nullptr;
        Q.qx = PM ? PM[0] : k1.x; Q.qy = PM ? PM[1] : k1.y;
        Q.r = (float)A.windowSize;
        Q.minLevel = Q.maxLevel = level1;                                                // GetFeaturesInArea(x, y, windowSize, level1, level1)
        load_desc32(A.desc1 + (size_t)pair * A.desc1_slice + (size_t)q * A.dstride1, Q.d0, Q.d1, Q.d2, Q.d3);
    } else {
        if (!A.valid[q]) { Q.active = false; return Q; }
        int qlev;
        if (KIND == 2) {
            const float4 f = ((const float4*)A.qf)[q];
            Q.qx = f.x; Q.qy = f.y;
            float r = ((double)f.z > 0.998) ? 2.5f : 4.0f;            // RadiusByViewingCos (:221-227)
            if (A.th != 1.0f) r *= A.th;                                // bFactor (:49, :73-74)
            Q.r = r * f.w;
            qlev = A.qlevel[q];
            Q.minLevel = qlev - 1; Q.maxLevel = qlev;
            Q.isorb = A.mp_is_orb ? A.mp_is_orb[q] != 0 : true;
        } else {
            Q.qx = A.qf[3 * q]; Q.qy = A.qf[3 * q + 1];
            Q.isorb = A.q_is_orb ? A.q_is_orb[q] != 0 : true;
            qlev = kp_level(A.qkps[q], Q.isorb);
            Q.r = A.th * A.qf[3 * q + 2];
            if (A.mode == 1) { Q.minLevel = qlev; Q.maxLevel = -1; }
            else if (A.mode == 2) { Q.minLevel = 0; Q.maxLevel = qlev; }
            else { Q.minLevel = qlev - 1; Q.maxLevel = qlev + 1; }
        }
        const uint64_t* dq = (const uint64_t*)(A.mp_desc + (size_t)q * 32);
        Q.d0 = dq[0]; Q.d1 = dq[1]; Q.d2 = dq[2]; Q.d3 = dq[3];
        if (A.q_ur && A.uright2) { Q.ur = A.q_ur[q]; Q.has_ur = true; }
    }
    return Q;
}

// candidate test of Frame::GetFeaturesInArea (Frame.cc:747-777) + the MixedMatcher type gate (MixedMatcher.cpp:65-67, :565-568,
// :787-790).  Returns the key, or ~0 when i2 is no candidate.  key = dist << 44 | cell << 32 | index << 8 | level + 1
__device__ __forceinline__ uint64_t win_key(const WinQuery& Q, int cx0, int cx1, int cy0, int cy1, uint32_t info, float x, float y,
                                            const uint64_t* __restrict__ dp, int i2, float uright = -1.f)
{
    const int cell = (int)(info & 0xffffu);
    if (cell == 0xFFFF) return ~0ull;
    const int cx = cell / kGridRows, cy = cell - cx * kGridRows;
    if (cx < cx0 || cx > cx1 || cy < cy0 || cy > cy1) return ~0ull;
    const int lv = (int)(int8_t)((info >> 16) & 0xffu);
    if ((Q.minLevel > 0) || (Q.maxLevel >= 0)) {                     // bCheckLevels
        if (lv < Q.minLevel) return ~0ull;
        if (Q.maxLevel >= 0 && lv > Q.maxLevel) return ~0ull;
    }
    const float distx = x - Q.qx, disty = y - Q.qy;
    if (!(fabsf(distx) < Q.r && fabsf(disty) < Q.r)) return ~0ull;
    if ((((info >> 24) & 1u) != 0) != Q.isorb) return ~0ull;
    // "if(F.mvuRight[idx]>0) { er = fabs(projXR - F.mvuRight[idx]); if(er > radius) continue; }" (:96-104, :2056-2062)
    if (Q.has_ur && uright > 0.f && fabsf(Q.ur - uright) > Q.r) return ~0ull;
    const int dist = __popcll(Q.d0 ^ dp[0]) + __popcll(Q.d1 ^ dp[1]) + __popcll(Q.d2 ^ dp[2]) + __popcll(Q.d3 ^ dp[3]);
    return ((uint64_t)dist << 44) | ((uint64_t)cell << 32) | ((uint64_t)(uint32_t)i2 << 8) | (uint64_t)((lv + 1) & 0xff);
}

template <int KIND>
__global__ __launch_bounds__(1024) void win_cand_kernel(WinArgs A, int qpb)
{
    extern __shared__ unsigned char smem[];
    const int pair = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N2 = A.n2p ? A.n2p[pair] : A.n2;
    const int NQ = A.nqp ? A.nqp[pair] : A.nq;
    const int q_lo = blockIdx.x * qpb, q_hi = min(NQ, q_lo + qpb);
    if (q_lo >= NQ) return;
    const int c2 = A.cap2;
    uint64_t* d2 = (uint64_t*)smem;                                   // c2 * 4
    uint64_t* wl = d2 + (size_t)c2 * 4 + (size_t)wave * A.wcap;       // nwaves * wcap: the waves' candidate lists
    const int nwaves = (int)blockDim.x >> 6;
    float* x2 = (float*)(d2 + (size_t)c2 * 4 + (size_t)nwaves * A.wcap);
    float* y2 = x2 + c2;
    uint32_t* info2 = (uint32_t*)(y2 + c2);
    const eorb_keypoint* K2 = A.kps2 + (size_t)pair * A.kp2_stride;
    const uint8_t* D2 = A.desc2 + (size_t)pair * A.desc2_slice;
    const uint8_t* O2 = A.is_orb2 ? A.is_orb2 + (size_t)pair * A.cap2 : nullptr;
    // (the wavefront's first query is loaded with the staging loads, not behind the barrier: one global round trip less on the call's path)
#ifdef EORB_WIN_TIMING
    long long ct[6]; ct[0] = clock64();
#endif
    WinQuery Q0; Q0.active = false;
    if (q_lo + wave < q_hi) Q0 = win_query<KIND>(A, pair, q_lo + wave);
    for (int i0 = 0; i0 < N2; i0 += 2 * (int)blockDim.x) {            // two keypoints' loads in flight per thread
        eorb_keypoint k[2]; bool isorb[2]; uint64_t dd[2][4];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int i = i0 + u * (int)blockDim.x + tid;
            if (i < N2) { k[u] = K2[i]; isorb[u] = O2 ? O2[i] != 0 : true; load_desc32(D2 + (size_t)i * A.dstride2, dd[u][0], dd[u][1], dd[u][2], dd[u][3]); }
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int i = i0 + u * (int)blockDim.x + tid;
            if (i < N2) {
                x2[i] = k[u].x; y2[i] = k[u].y; info2[i] = f2_info(k[u], isorb[u], A.g);
                d2[(size_t)i * 4 + 0] = dd[u][0]; d2[(size_t)i * 4 + 1] = dd[u][1]; d2[(size_t)i * 4 + 2] = dd[u][2]; d2[(size_t)i * 4 + 3] = dd[u][3];
            }
        }
    }
    __syncthreads();
#ifdef EORB_WIN_TIMING
    ct[1] = clock64(); ct[2] = ct[3] = ct[4] = ct[1];
#endif
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    uint64_t* ent = A.ent + (size_t)pair * A.ecap;
    for (int q = q_lo + wave; q < q_hi; q += nwaves) {
        const WinQuery Q = q == q_lo + wave ? Q0 : win_query<KIND>(A, pair, q);
        uint32_t n = 0;
        int cx0 = 0, cx1 = -1, cy0 = 0, cy1 = -1;
        if (Q.active && cell_range(A.g, Q.qx, Q.qy, Q.r, cx0, cx1, cy0, cy1)) {
            for (int i0 = 0; i0 < N2; i0 += 64) {
                const int i2 = i0 + lane;
                uint64_t key = ~0ull;
                if (i2 < N2) key = win_key(Q, cx0, cx1, cy0, cy1, info2[i2], x2[i2], y2[i2], &d2[(size_t)i2 * 4], i2, Q.has_ur ? A.uright2[i2] : -1.f);
                const bool ok = key != ~0ull && (int)(key >> 44) < A.dmax;
                const uint64_t bal = __ballot(ok);
                if (ok) { const uint32_t pos = n + (uint32_t)__popcll(bal & lt_mask); if (pos < (uint32_t)A.wcap) wl[pos] = key; }
                n += (uint32_t)__popcll(bal);
            }
        }
#ifdef EORB_WIN_TIMING
        ct[2] = clock64();
#endif
        uint32_t off = 0, cnt = n;
        if (n > (uint32_t)A.wcap) cnt = kWinOver;
        else if (n > 0) {
            if (lane == 0) off = atomicAdd(&A.total[pair], n) & 0x7FFFFFFFu;
            off = (uint32_t)__shfl((int)off, 0, 64);
#ifdef EORB_WIN_TIMING
            ct[3] = clock64();
#endif
            if (off + n > (uint32_t)A.ecap) cnt = kWinOver;           // the pair's pool is full
            else {
                // the list leaves sorted by key (rank = number of smaller keys; keys are unique): phase 2 then stops at the first
                // one or two candidates that pass its state filter instead of walking the whole list
                for (uint32_t j = lane; j < n; j += 64) {
                    const uint64_t kj = wl[j];
                    uint32_t rank = 0;
                    for (uint32_t i = 0; i < n; i++) rank += (wl[i] < kj) ? 1u : 0u;
                    ent[off + rank] = kj;
                }
            }
        }
        if (lane == 0) {
            A.cnt[(size_t)pair * A.capq + q] = cnt; A.off[(size_t)pair * A.capq + q] = off;
            if (cnt == kWinOver) atomicOr(&A.total[pair], 0x80000000u);          // (bit 31 of the pair's counter: some list overflowed; phase 2 reads it there)
        }
#ifdef EORB_WIN_TIMING
        ct[4] = clock64();
        if (pair == 0 && lane == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x / 2) && (wave == 0 || wave == nwaves - 1))
            printf("win_cand<%d> wg %d wave %d (n %u): staging %lld | scan %lld | pool atomic %lld | sort + write %lld\n", KIND, (int)blockIdx.x, wave, n, ct[1] - ct[0], ct[2] - ct[1], ct[3] - ct[2], ct[4] - ct[3]);
#endif
    }
}

// wave-wide minimum of a 32-bit value in every lane: row_shr 1 / 2 / 4 / 8 inside the 16-lane rows, row_bcast 15 / 31 across them
// (lanes without a source keep their own value), then lane 63 holds the minimum
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x)
{
#define EORB_MIN_DPP(ctrl, rmask) x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, ctrl, rmask, 0xf, false))
    EORB_MIN_DPP(0x111, 0xf); EORB_MIN_DPP(0x112, 0xf); EORB_MIN_DPP(0x114, 0xf); EORB_MIN_DPP(0x118, 0xf);
    EORB_MIN_DPP(0x142, 0xa); EORB_MIN_DPP(0x143, 0xc);
#undef EORB_MIN_DPP
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// wave-wide smallest 64-bit key (every lane gets it): minimum of the high words, then of the low words among the lanes that hold it
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t k)
{
    const uint32_t hi = (uint32_t)(k >> 32), lo = (uint32_t)k;
    const uint32_t mh = wave_min_u32(hi);
    const uint32_t ml = wave_min_u32(hi == mh ? lo : 0xFFFFFFFFu);
    return ((uint64_t)mh << 32) | ml;
}

// wave-wide two smallest keys of the lanes' (k0 <= k1) pairs; keys are unique; result in every lane
__device__ __forceinline__ void wave_top2(uint64_t& k0, uint64_t& k1)
{
    const uint64_t b0 = wave_min_u64(k0);
    const uint64_t b1 = wave_min_u64(k0 == b0 ? k1 : k0);
    k0 = b0; k1 = b1;
}

constexpr int kWinLdsEntries = 6144;      // least number of a pair's entries that phase 2 stages in LDS (WinArgs::lds_ents: as many as fit; the rest is read from global memory)

__device__ __forceinline__ int wave_sum_i32(int v) { for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64); return v; }

// histo[b] += 1 for every lane with b >= 0: one LDS atomic per distinct bin of the wavefront (matches of one frame pair share two or
// three rotation bins: lane-wise atomics on them serialise, 540 of them cost 2 us)
__device__ __forceinline__ void wave_histo_add(int* histo, int b, int lane)
{
    uint64_t todo = __ballot(b >= 0);
    while (todo) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        const int bb = __shfl(b, l, 64);
        const uint64_t same = __ballot(b == bb);
        if (lane == l) atomicAdd(&histo[bb], (int)__popcll(same));
        todo &= ~same;
    }
}

// entry e of a pair: from LDS, or from the pool in global memory beyond what LDS holds.  (Written as "cond ? ents[e] : gent[e]" the
// compiler selects between the two POINTERS and emits one flat load: every walk step then goes through the flat path.)
__device__ __forceinline__ uint64_t win_entry(const uint64_t* ents, const uint64_t* __restrict__ gent, uint32_t e, uint32_t nlds)
{
    uint64_t k = ents[min(e, nlds - 1u)];
    if (e >= nlds) k = *(const volatile uint64_t*)(gent + e);        // (volatile: not to be merged with the LDS read into one flat load either)
    return k;
}

template <int KIND>
__global__ __launch_bounds__(1024) void win_resolve_kernel(WinArgs A)
{
    extern __shared__ unsigned char smem[];
    const int pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N2 = A.n2p ? A.n2p[pair] : A.n2;
    const int NQ = A.nqp ? A.nqp[pair] : A.nq;
    const int c2 = A.cap2, cq = A.capq;
#ifdef EORB_WIN_TIMING       // (experiment builds only: where the kernel's time goes, printed by pair 0)
    __shared__ long long s_wt[8]; __shared__ int s_wn[8];
    long long wt_last = clock64();
    if (threadIdx.x < 8) { s_wt[threadIdx.x] = 0; s_wn[threadIdx.x] = 0; }
#define WIN_T(k) do { if (threadIdx.x == 0) { const long long t_now = clock64(); s_wt[k] += t_now - wt_last; s_wn[k]++; wt_last = t_now; } } while (0)
#else
#define WIN_T(k) do { } while (0)
#endif
    // LDS carve-up
    const uint32_t nlds = (uint32_t)A.lds_ents;
    uint64_t* ents = (uint64_t*)smem;                                 // lds_ents
    uint32_t* offs = (uint32_t*)(ents + nlds);                        // cq
    uint32_t* cnts = offs + cq;                                       // cq
    int* histo = (int*)(cnts + cq);                                   // 32
    int* sh_nm = histo + 32;                                          // 4: matches, -, the fixed points' "somebody changed" words (2)
    unsigned int* sflag = (unsigned int*)(sh_nm + 2);
    int* st_a = sh_nm + 4;                                            // c2: KIND 0 vMatchedDistance, else the slot -> map point table
    int* match_at = st_a + c2;                                        // cq: candidate matched by query q when it was processed (-1: none)
    int16_t* m21 = (int16_t*)(match_at + cq);                         // c2: KIND 0 vnMatches21 (-1: none)  [cap1 < 32768]
    uint8_t* obs = (uint8_t*)(m21 + c2);                              // c2: KIND 1/2 "slot holds an observed map point"
    uint8_t* qobs = obs + c2;                                         // cq: KIND 1/2 mp_obs of the query's map point
    unsigned int* claim = (unsigned int*)(smem + (((size_t)((unsigned char*)(qobs + cq) - smem) + 3) & ~(size_t)3));   // 2 x c2 (an offset from smem, not a cast through an integer: the accesses stay LDS instructions): earliest query of the round / sweep matching the candidate
    float* ang2 = (float*)(claim + 2 * (c2 + 1));                     // c2: the searched keypoints' angles (rotation histogram)
    int* fx = (int*)(ang2 + c2);                                      // KIND 0 fixed point: 4 x cq (match / distance of the next sweep, chain links, distances)
    int32_t* M12 = A.matches12 ? A.matches12 + (size_t)pair * cq : nullptr;
    const uint64_t* gent = A.ent + (size_t)pair * A.ecap;
    const eorb_keypoint* K2s = A.kps2 + (size_t)pair * A.kp2_stride;
    // set-up: every global load that depends on nothing is issued before the first wait (a load is ~ 1 500 cycles here and the
    // loops below would take them one after the other: 11 000 cycles of 1 024 threads waiting)
    const int bd = (int)blockDim.x;
    uint32_t r_off[2], r_cnt[2]; uint8_t r_qo[2]; int r_slot[2]; float r_ang[2], r_qang[2];
    const eorb_keypoint* KQ = KIND == 0 ? A.kps1 + (size_t)pair * A.kp1_stride : A.qkps;       // the queries' keypoints (rotation histogram)
    const uint32_t total_raw = A.total[pair];
    const uint32_t total = min(total_raw & 0x7FFFFFFFu, (uint32_t)A.ecap);
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int i = tid + u * bd;
        r_off[u] = 0; r_cnt[u] = 0; r_qo[u] = 0; r_slot[u] = -1; r_ang[u] = 0.f; r_qang[u] = 0.f;
        if (i < NQ && KIND != 2 && A.checkOri) r_qang[u] = KQ[i].angle;
        if (i < NQ) { r_off[u] = A.off[(size_t)pair * cq + i]; r_cnt[u] = A.cnt[(size_t)pair * cq + i]; if (KIND != 0) r_qo[u] = A.mp_obs[i]; }
        if (i < N2) { if (KIND != 0) r_slot[u] = A.slot_mp[i]; if (A.checkOri) r_ang[u] = K2s[i].angle; }
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int i = tid + u * bd;
        if (i < NQ) { offs[i] = r_off[u]; cnts[i] = r_cnt[u]; match_at[i] = -1; if (KIND != 0) qobs[i] = r_qo[u] != 0; }
    }
    for (int i = tid + 2 * bd; i < NQ; i += bd) {
        offs[i] = A.off[(size_t)pair * cq + i]; cnts[i] = A.cnt[(size_t)pair * cq + i];
        match_at[i] = -1;
        if (KIND != 0) qobs[i] = A.mp_obs[i] != 0;
    }
    {   // eight loads in flight per thread
        const uint32_t nst = min(total, nlds);
        for (uint32_t i0 = 0; i0 < nst; i0 += 8u * (uint32_t)bd) {
            uint64_t t8[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { const uint32_t i = i0 + (uint32_t)(u * bd + tid); t8[u] = i < nst ? gent[i] : 0ull; }
#pragma unroll
            for (int u = 0; u < 8; u++) { const uint32_t i = i0 + (uint32_t)(u * bd + tid); if (i < nst) ents[i] = t8[u]; }
        }
    }
    // slot values of KIND 1 / 2: "if(F.getMapPoint(idx)) if(F.getMapPoint(idx)->Observations()>0) continue;" (:91-93, :2045-2047):
    // -1 / -3 = empty or unobserved, -2 = holds an observed map point, v >= 0 = map point v
    auto slot_in = [&](int i, int v, float ang) {
        if (KIND == 0) { st_a[i] = 0x7fffffff; m21[i] = -1; }
        else { st_a[i] = v; obs[i] = (v == -2) ? 1 : ((v >= 0) ? (A.mp_obs[v] != 0) : 0); }
        if (A.checkOri) ang2[i] = ang;
    };
#pragma unroll
    for (int u = 0; u < 2; u++) { const int i = tid + u * bd; if (i < N2) slot_in(i, r_slot[u], r_ang[u]); }
    for (int i = tid + 2 * bd; i < N2; i += bd) slot_in(i, KIND != 0 ? A.slot_mp[i] : -1, A.checkOri ? K2s[i].angle : 0.f);
    if (tid < 32) histo[tid] = 0;
    if (tid < 4) sh_nm[tid] = 0;
    const bool no_over = KIND != 2 && (total_raw >> 31) == 0u;          // (no list of the pair overflowed: phase 1 says so in the counter)
    __syncthreads();
    const bool fixpoint = KIND == 1 && no_over, fixpoint0 = KIND == 0 && no_over;
    // claims: the walk's are "earliest lane of the round" (empty = ~0); the fixed point's are tagged by their sweep (empty = 0), in two
    // buffers of c2 + 1 words: ~0 = closed for good (an observed map point in the slot; word c2 stands for "no entry")
    for (int i = tid; i < 2 * (c2 + 1); i += bd) {
        const int ii = i > c2 ? i - (c2 + 1) : i;
        claim[i] = !fixpoint || ii == c2 || (ii < N2 && obs[ii] != 0) ? 0xFFFFFFFFu : 0u;
    }
    if (KIND == 0 && !fixpoint0) for (int i = tid; i < NQ; i += bd) M12[i] = -1;      // (the walk keeps vnMatches12 in global memory)
    __syncthreads();
    WIN_T(0);

    if (fixpoint) {
        // SearchByProjection(cur, last / KeyFrame): a query takes the FIRST entry of its sorted list whose candidate is free (no
        // observed map point in the slot: :2045-2047 / :2231) if that entry is within the distance threshold, and its map point
        // then blocks the candidate for later queries when it is observed.  So query q's outcome is a function of the outcomes of
        // the queries before it, and the whole walk is the fixed point of "every query takes its first entry that no EARLIER query
        // with an observed map point has taken", iterated from "nobody has taken anything": query 0 is final after one sweep, and
        // each sweep finalises at least the first query that still changed -- in practice three to five sweeps settle a window of
        // 1 024 queries (dependency chains are short), where the walk below spends a round per conflict.
        // One barrier per sweep: the claims of sweep s go to buffer s & 1 tagged with s (atomicMax of s << 16 | 0xFFFF - tid: a newer
        // sweep beats what the buffer still holds, the earliest query wins inside a sweep), sweep s reads buffer (s - 1) & 1 and takes
        // only tags s - 1, nobody clears anything; "somebody changed" is the word sflag[s & 1] == s.
        int nm = 0;
        uint32_t s = 1;
        for (int base = 0; base < NQ; base += (int)blockDim.x) {
            const int q = base + tid;
            const uint32_t c = q < NQ ? cnts[q] : 0u;
            const uint32_t o = q < NQ ? offs[q] : 0u;
            const bool blocks = q < NQ && qobs[q] != 0;
            int pick = -1;
            // A sweep lasts as long as its slowest wavefront, and sixteen of them share the four SIMDs of one CU: what counts is the
            // instructions of a sweep.  Per entry one LDS word and one compare: a candidate is free for query tid in sweep s iff its
            // word is <= T = (s - 1) << 16 | 0xFFFF - tid (older tags are smaller, a claimant after tid has a smaller low half, ~0 is
            // a closed slot); the tests on the distance are vacuous here (phase 1 listed dist < dmax <= min(dist_th + 1, 256)).  The
            // candidates of the first eight entries (the longest walks of a crowded frame are about that long) stay in registers.
            auto cand4 = [&](uint32_t j0, uint32_t* a4) {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    a4[u] = (uint32_t)c2;
                    if (j0 + (uint32_t)u < c) a4[u] = (uint32_t)((win_entry(ents, gent, o + j0 + (uint32_t)u, nlds) >> 8) & 0xffffffu);
                }
            };
            uint32_t f4[4], g4[4];
            cand4(0, f4); cand4(4, g4);
            for (;; s++) {
                unsigned int* wr = claim + ((s & 1u) ? (uint32_t)(c2 + 1) : 0u);            // buffer s & 1
                const unsigned int* rd = claim + ((s & 1u) ? 0u : (uint32_t)(c2 + 1));      // buffer (s - 1) & 1
                const unsigned int T = ((s - 1u) << 16) | (0xFFFFu - (unsigned int)tid);
                int np = -1;
                {
                    const unsigned int v0 = rd[f4[0]], v1 = rd[f4[1]], v2 = rd[f4[2]], v3 = rd[f4[3]];
                    np = v0 <= T ? (int)f4[0] : v1 <= T ? (int)f4[1] : v2 <= T ? (int)f4[2] : v3 <= T ? (int)f4[3] : -1;
                }
                if (np < 0 && c > 4u) {
                    const unsigned int v0 = rd[g4[0]], v1 = rd[g4[1]], v2 = rd[g4[2]], v3 = rd[g4[3]];
                    np = v0 <= T ? (int)g4[0] : v1 <= T ? (int)g4[1] : v2 <= T ? (int)g4[2] : v3 <= T ? (int)g4[3] : -1;
                }
                for (uint32_t j0 = 8; np < 0 && j0 < c; j0 += 4) {
                    uint32_t a4[4];
                    cand4(j0, a4);
                    const unsigned int v0 = rd[a4[0]], v1 = rd[a4[1]], v2 = rd[a4[2]], v3 = rd[a4[3]];
                    np = v0 <= T ? (int)a4[0] : v1 <= T ? (int)a4[1] : v2 <= T ? (int)a4[2] : v3 <= T ? (int)a4[3] : -1;
                }
                if (np >= 0 && blocks) atomicMax(&wr[np], (s << 16) | (0xFFFFu - (unsigned int)tid));
                if (np != pick) sflag[s & 1u] = s;
                pick = np;
                __syncthreads();
                WIN_T(1);
                if (sflag[s & 1u] != s) break;
            }
            s += 2;                                                     // (the next window must not meet this one's last claims)
            // the window's commits: the LAST query that took a candidate owns its slot; an observed map point closes it
            if (pick >= 0) { match_at[q] = pick; st_a[pick] = -1; nm++; }      // (the slot's old content -- empty or an unobserved map point -- goes)
            __syncthreads();
            if (pick >= 0) atomicMax(&st_a[pick], q);
            if (pick >= 0 && blocks) { claim[pick] = 0xFFFFFFFFu; claim[c2 + 1 + pick] = 0xFFFFFFFFu; }
            __syncthreads();
            WIN_T(2);
        }
        nm = wave_sum_i32(nm);
        if (lane == 0 && nm) atomicAdd(&sh_nm[0], nm);
    } else if (fixpoint0) {
        // SearchForInitialization (:714-831): query q skips a candidate whose vMatchedDistance is <= its distance (:755), i.e. a candidate
        // that an EARLIER query matched at a distance <= its own; among the rest its best / second best decide whether it matches its
        // best (:770-772), which then carries q's distance and loses its previous owner (:774-781).  So q's outcome is a function of the
        // matches of the queries before it: D_q[i2] = min { dist(q', i2) : q' < q matched i2 }, and the walk is the fixed point of
        // "every query decides against the D of the previous sweep's matches", iterated from "nobody matched": query 0 is final after
        // one sweep, every sweep finalises at least the first query that still changed; dependency chains are short in practice (a
        // handful of sweeps for 1 000 queries, where the round-based walk below took a round per conflict: 49 us).  Per candidate the
        // sweep's matchers hang on a chain (head in st_a, links in fx): the minimum over the earlier ones is a walk of one or two links.
        int* mcur = match_at; int* mnew = fx; int* dcur = fx + cq; int* dnew = fx + 2 * cq; int* nxt = fx + 3 * cq;
        for (int i = tid; i < N2; i += blockDim.x) st_a[i] = -1;              // chain heads
        for (int i = tid; i < NQ; i += blockDim.x) dcur[i] = 0;
        __syncthreads();
        for (int sweep = 0; sweep <= NQ; sweep++) {
            int changed = 0;
            for (int q = tid; q < NQ; q += blockDim.x) {
                const uint32_t c = cnts[q], o = offs[q];
                uint64_t k0 = ~0ull, k1 = ~0ull;
                int found = 0;
                for (uint32_t j = 0; j < c && found < 2; j++) {
                    const uint32_t e = o + j;
                    const uint64_t key = win_entry(ents, gent, e, nlds);
                    const int idx = (int)((key >> 8) & 0xffffffu), dist = (int)(key >> 44);
                    int D = 0x7fffffff;                                       // vMatchedDistance[idx] as query q finds it
                    for (int p2 = st_a[idx]; p2 >= 0; p2 = nxt[p2]) if (p2 < q) D = min(D, dcur[p2]);
                    if (D > dist) { if (found == 0) k0 = key; else k1 = key; found++; }
                }
                int m = -1, d = 0;
                if (k0 != ~0ull) {
                    const int bestDist = (int)(k0 >> 44), bestDist2 = (k1 == ~0ull) ? 0x7fffffff : (int)(k1 >> 44);
                    if (bestDist <= TH_LOW && (float)bestDist < (float)bestDist2 * A.nnratio) { m = (int)((k0 >> 8) & 0xffffffu); d = bestDist; }   // :770-772
                }
                mnew[q] = m; dnew[q] = d;
                changed |= (m != mcur[q]) ? 1 : 0;
            }
            if (changed) sflag[sweep & 1] = (unsigned int)sweep + 1u;         // ("somebody changed" as a tagged word: one plain barrier)
            __syncthreads();
            WIN_T(1);
            if (sflag[sweep & 1] != (unsigned int)sweep + 1u) break;          // (mnew == mcur: the chains already describe the final matches)
            { int* t = mcur; mcur = mnew; mnew = t; t = dcur; dcur = dnew; dnew = t; }
            for (int i = tid; i < N2; i += blockDim.x) st_a[i] = -1;
            __syncthreads();
            for (int q = tid; q < NQ; q += blockDim.x) { const int m = mcur[q]; if (m >= 0) nxt[q] = atomicExch(&st_a[m], q); }
            __syncthreads();
        }
        // the walk's final state: every matched query pushed its rotation-histogram entry (match_at), a candidate belongs to the LAST of
        // its matchers (each later one came with a strictly smaller distance and took it over, :774-781)
        if (mcur != match_at) { for (int q = tid; q < NQ; q += blockDim.x) match_at[q] = mcur[q]; }
        __syncthreads();
        for (int q = tid; q < NQ; q += blockDim.x) fx[q] = -1;                // vnMatches12 while the kernel still works on it
        __syncthreads();
        int nm = 0;
        for (int i = tid; i < N2; i += blockDim.x) {
            int owner = -1;
            for (int p2 = st_a[i]; p2 >= 0; p2 = nxt[p2]) owner = max(owner, p2);
            if (owner >= 0) { fx[owner] = i; nm++; }
        }
        nm = wave_sum_i32(nm);
        if (lane == 0 && nm) atomicAdd(&sh_nm[0], nm);
    } else if (wave == 0) {
        // The queries are walked in order, 64 at a time (lane = query).  Every lane evaluates its query against the committed
        // state; a query commits in this round only if no EARLIER query of the round changes a candidate it depends on.  The state
        // only ever removes candidates (vMatchedDistance decreases, a slot turns "observed"), and a query's outcome depends on its
        // best and second-best passing candidates alone: so query j must wait exactly when an earlier query of the round matches
        // j's best or second-best candidate.  The round commits the conflict-free prefix (never empty: its first query has no
        // predecessor) and the next round starts at the first conflicting query.  Committed queries of one round have distinct best
        // candidates, so their updates are independent.
        int nm = 0;
        const eorb_keypoint* K2 = A.kps2 + (size_t)pair * A.kp2_stride;
        const uint8_t* D2 = A.desc2 + (size_t)pair * A.desc2_slice;
        const uint8_t* O2 = A.is_orb2 ? A.is_orb2 + (size_t)pair * A.cap2 : nullptr;
        auto passes = [&](uint64_t key) -> bool {
            const int idx = (int)((key >> 8) & 0xffffffu);
            const int dist = (int)(key >> 44);
            return (KIND == 0) ? (st_a[idx] > dist)                     // "if(vMatchedDistance[i2]<=dist) continue;" :755
                               : (obs[idx] == 0 && dist < 256);         // bestDist starts at 256, strict '<'
        };
        // outcome of a query from its two smallest passing keys: does it match its best candidate?
        auto matched = [&](uint64_t k0, uint64_t k1) -> bool {
            if (k0 == ~0ull) return false;
            const int bestDist = (int)(k0 >> 44), bestLevel = (int)(k0 & 0xff) - 1;
            if (KIND == 0) {
                const int bestDist2 = (k1 == ~0ull) ? 0x7fffffff : (int)(k1 >> 44);
                return bestDist <= TH_LOW && (float)bestDist < (float)bestDist2 * A.nnratio;       // :770-772
            } else if (KIND == 2) {
                int bestDist2 = 256, bestLevel2 = -1;
                if (k1 != ~0ull) { bestDist2 = (int)(k1 >> 44); bestLevel2 = (int)(k1 & 0xff) - 1; }
                if (bestDist > TH_HIGH) return false;                                              // :131-147
                const bool reject = (bestLevel == bestLevel2) && ((float)bestDist > A.nnratio * (float)bestDist2);
                return !reject && (bestLevel != bestLevel2 || (float)bestDist <= A.nnratio * (float)bestDist2);
            } else {
                return bestDist <= A.dist_th;                                                      // :2140 / :2271
            }
        };
        // the greedy update of one matched query (one lane; distinct candidates across the lanes of a round)
        auto commit = [&](int q, uint64_t k0, int& stolen) {
            const int bestIdx = (int)((k0 >> 8) & 0xffffffu);
            if (KIND == 0) {
                const int old = m21[bestIdx];
                if (old >= 0) { M12[old] = -1; stolen = 1; }                                       // :774-778
                M12[q] = bestIdx; m21[bestIdx] = (int16_t)q; st_a[bestIdx] = (int)(k0 >> 44); match_at[q] = bestIdx;
            } else {
                st_a[bestIdx] = q; obs[bestIdx] = qobs[q];
                if (KIND == 1) match_at[q] = bestIdx;
            }
        };
        int pos = 0;
        while (pos < NQ) {
            const int q = pos + lane;
            const uint32_t c = (q < NQ) ? cnts[q] : 0u;
            const uint64_t over = __ballot(c == kWinOver);
            const int limit = over ? (__ffsll((unsigned long long)over) - 1) : 64;
            if (limit == 0) {
                // the list of query `pos` overflowed: the wavefront scans the whole searched frame (global memory) for it
                uint64_t k0 = ~0ull, k1 = ~0ull;
                const WinQuery Q = win_query<KIND>(A, pair, pos);
                int cx0, cx1, cy0, cy1;
                if (Q.active && cell_range(A.g, Q.qx, Q.qy, Q.r, cx0, cx1, cy0, cy1)) {
                    for (int i2 = lane; i2 < N2; i2 += 64) {
                        const eorb_keypoint k = K2[i2];
                        const bool isorb = O2 ? O2[i2] != 0 : true;
                        uint64_t dd[4];
                        load_desc32(D2 + (size_t)i2 * A.dstride2, dd[0], dd[1], dd[2], dd[3]);
                        const uint64_t key = win_key(Q, cx0, cx1, cy0, cy1, f2_info(k, isorb, A.g), k.x, k.y, dd, i2, Q.has_ur ? A.uright2[i2] : -1.f);
                        if (key != ~0ull && passes(key)) { if (key < k0) { k1 = k0; k0 = key; } else if (key < k1) k1 = key; }
                    }
                }
                wave_top2(k0, k1);
                if (matched(k0, k1)) {
                    int stolen = 0;
                    if (lane == 0) commit(pos, k0, stolen);
                    stolen = __shfl(stolen, 0, 64);
                    nm += 1 - stolen;
                }
                pos += 1;
                continue;
            }
            // ---- evaluate (lane = query) ----
            uint64_t k0 = ~0ull, k1 = ~0ull;
            const bool live = lane < limit && c != 0u;
            if (live) {
                const uint32_t o = offs[q];
                // the list is sorted: the first passing entries are the best and the second best
                constexpr int need = (KIND == 1) ? 1 : 2;
                int found = 0;
                // the first four entries and their states in flight together (a round is a chain of LDS round trips: the two best
                // passing entries are almost always among them), the rest of the list one by one
                uint64_t e4[4]; bool p4[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { const uint32_t e = o + (uint32_t)u; e4[u] = (uint32_t)u < c ? win_entry(ents, gent, e, nlds) : ~0ull; }
#pragma unroll
                for (int u = 0; u < 4; u++) p4[u] = e4[u] != ~0ull && passes(e4[u]);
#pragma unroll
                for (int u = 0; u < 4; u++) if (p4[u] && found < need) { if (found == 0) k0 = e4[u]; else k1 = e4[u]; found++; }
                for (uint32_t j = 4; j < c && found < need; j++) {
                    const uint32_t e = o + j;
                    const uint64_t key = win_entry(ents, gent, e, nlds);
                    if (passes(key)) { if (found == 0) k0 = key; else k1 = key; found++; }
                }
            }
            const bool mt = live && matched(k0, k1);
            const int i0 = (int)((k0 >> 8) & 0xffffffu), i1 = (int)((k1 >> 8) & 0xffffffu);
            // ---- claims: the earliest query of the round that changes each candidate ----
            if (mt) atomicMin(&claim[i0], (unsigned int)lane);
            bool conflict = false;
            if (live) conflict = (k0 != ~0ull && claim[i0] < (unsigned int)lane) || (k1 != ~0ull && claim[i1] < (unsigned int)lane);
            const uint64_t cm = __ballot(conflict);
            const int ncommit = cm ? (__ffsll((unsigned long long)cm) - 1) : limit;
            int stolen = 0;
            const bool doit = mt && lane < ncommit;
            if (doit) commit(q, k0, stolen);
            if (mt) claim[i0] = 0xFFFFFFFFu;
            nm += (int)__popcll(__ballot(doit)) - (int)__popcll(__ballot(stolen != 0));
            pos += ncommit;
        }
        if (lane == 0) sh_nm[0] = nm;
    }
    __syncthreads();
    WIN_T(3);
    if (KIND == 0) {
        int8_t* bin1 = (int8_t*)qobs;                                  // free in this kind: the bin of query q's push
        int* m12s = fx;                                                // vnMatches12 in LDS until the last loop
        if (!fixpoint0) { for (int i = tid; i < NQ; i += bd) m12s[i] = M12[i]; __syncthreads(); }
        if (A.checkOri) {
            // rotHist[bin].push_back(i1) happened for every match when it was made (:785-797), stolen ones included
            auto push = [&](int i, float qang, bool have) {                // (called by whole wavefronts)
                int b = -1;
                if (i < NQ) { const int m = match_at[i]; if (m >= 0) b = rot_bin(have ? qang : KQ[i].angle, ang2[m]); bin1[i] = (int8_t)b; }
                wave_histo_add(histo, b, lane);
            };
            push(tid, r_qang[0], true);
            if (bd < NQ) push(tid + bd, r_qang[1], true);
            for (int i0 = 2 * bd; i0 < NQ; i0 += bd) push(i0 + tid, 0.f, false);
            __syncthreads();
            int ind1, ind2, ind3;
            three_maxima(histo, HISTO_LENGTH, ind1, ind2, ind3);
            int dec = 0;
            for (int i = tid; i < NQ; i += bd) {
                const int b = bin1[i];
                if (b >= 0 && b != ind1 && b != ind2 && b != ind3 && m12s[i] >= 0) { m12s[i] = -1; dec++; }
            }
            dec = wave_sum_i32(dec);
            if (lane == 0 && dec) atomicSub(&sh_nm[0], dec);
            __syncthreads();
        }
        float* PM = A.prev_matched ? A.prev_matched + (size_t)pair * cq * 2 : nullptr;
        for (int i = tid; i < NQ; i += bd) {
            const int m = m12s[i];
            M12[i] = m;
            if (PM && m >= 0) { const eorb_keypoint k = K2s[m]; PM[2 * i] = k.x; PM[2 * i + 1] = k.y; }
        }
    } else {
        if (KIND == 1 && A.checkOri) {
            // rotHist[bin].push_back(bestIdx2) per match (:2146-2160); losing bins: setMapPoint(idx, NULL), nmatches-- per push
            unsigned int* hbin = (unsigned int*)ents;                  // the entry buffer is free now: c2 words (c2 <= 2 * kWinLdsEntries <= 2 * lds_ents)
            for (int i = tid; i < N2; i += bd) hbin[i] = 0u;
            __syncthreads();
            auto push = [&](int i, float qang, bool have) {                // (called by whole wavefronts)
                int b = -1;
                if (i < NQ) {
                    const int m = match_at[i];
                    if (m >= 0) { b = rot_bin(have ? qang : KQ[i].angle, ang2[m]); atomicOr(&hbin[m], 1u << b); }
                }
                wave_histo_add(histo, b, lane);
            };
            push(tid, r_qang[0], true);
            if (bd < NQ) push(tid + bd, r_qang[1], true);
            for (int i0 = 2 * bd; i0 < NQ; i0 += bd) push(i0 + tid, 0.f, false);
            __syncthreads();
            int ind1, ind2, ind3;
            three_maxima(histo, HISTO_LENGTH, ind1, ind2, ind3);
            unsigned int keep = 0u;
            if (ind1 >= 0) keep |= 1u << ind1;
            if (ind2 >= 0) keep |= 1u << ind2;
            if (ind3 >= 0) keep |= 1u << ind3;
            for (int i = tid; i < N2; i += bd)
                if (hbin[i] & ~keep) st_a[i] = -1;
            if (wave == 0) {
                const int dec = wave_sum_i32((lane < HISTO_LENGTH && !(keep & (1u << lane))) ? histo[lane] : 0);
                if (lane == 0) sh_nm[0] -= dec;
            }
            __syncthreads();
        }
        for (int i = tid; i < N2; i += bd) A.slot_mp[i] = st_a[i];
    }
    if (tid == 0) { A.nmatches[pair] = sh_nm[0]; A.total[pair] = 0u; }        // (the counter goes back to zero for the next call's phase 1)
#ifdef EORB_WIN_TIMING
    WIN_T(4);
    if (tid == 0 && pair == 0)
        printf("win_resolve<%d> NQ %d N2 %d entries %u: set-up %lld | sweeps %d x %lld | commits %d x %lld | tail of the walk %lld | histogram + outputs %lld (clock64 ticks)\n", KIND, NQ, N2, total,
               s_wt[0], s_wn[1], s_wn[1] ? s_wt[1] / s_wn[1] : 0, s_wn[2], s_wn[2] ? s_wt[2] / s_wn[2] : 0, s_wt[3], s_wt[4]);
#endif
}

static size_t win_cand_lds(int cap2, int wcap, int nwaves) { return ((size_t)cap2 * (32 + 4 + 4 + 4) + (size_t)nwaves * wcap * 8 + 15) & ~(size_t)15; }
// phase 2's LDS without the entries: offs, cnts, match_at, qobs, fx per query; st_a, m21, obs, two claim buffers, angle per searched keypoint
static size_t win_resolve_lds_rest(int cap2, int capq)
{
    return ((size_t)capq * (4 + 4 + 4 + 1 + 16) + (32 + 4) * 4 + (size_t)cap2 * (4 + 2 + 1 + 8 + 4) + 16 + 15) & ~(size_t)15;
}

// A kernel's dynamic LDS beyond 64 KB needs an opt-in, which holds per device: made once per context (a second context on another
// GPU needs it too) and kernel; `bit` numbers the kernel in c->lds_optin
enum { kOptWinCand = 0, kOptWinResolve = 3, kOptTwocam = 6, kOptKfRadius = 8, kOptBowAssemble = 9, kOptKfRadiusMixed = 10 };
static int lds_optin(eorb_ctx* c, int bit, const void* kernel, int bytes)
{
    if (c->lds_optin & (1u << bit)) return EORB_OK;
    EORB_HIP(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    c->lds_optin |= 1u << bit;
    return EORB_OK;
}

// smallest d in [lo, 256] for which pred(d) holds, else 257 (= keep every candidate)
template <typename F> static int first_dist(int lo, F pred) { for (int d = lo; d <= 256; d++) if (pred(d)) return d; return 257; }

template <int KIND>
static int launch_win(eorb_ctx* c, WinArgs& A, int npairs, int nq_max, const char* name)
{
    if (A.cap2 >= (1 << 24) || A.capq >= 32768) return set_err(c, EORB_E_CAPACITY, "%s: too many keypoints", name);
    if (A.cap2 > 2 * kWinLdsEntries) return set_err(c, EORB_E_CAPACITY, "%s: %d keypoints in the searched frame (limit %d)", name, A.cap2, 2 * kWinLdsEntries);
    A.wcap = c->opt.win_list_cap > 0 ? c->opt.win_list_cap : 512;
    A.ecap = c->opt.win_pool_cap > 0 ? c->opt.win_pool_cap : std::max(4096, 16 * A.capq);
    // phase 2 keeps as many of a pair's entries in LDS as fit beside its tables (one read from global memory inside a sweep is what the
    // whole workgroup then waits for at the sweep's barrier), at least kWinLdsEntries
    // phase 1: every workgroup stages the searched frame (44 B per keypoint) from the L2 before its wavefronts take a query each.  A lone
    // pair (one frame per call) is latency: 16 wavefronts per workgroup stage it in two loads per thread and 4 x fewer workgroups do so
    // (SearchByProjection 24 -> ... us); a batch of pairs fills the chip either way and keeps the small workgroups.
    int cw = c->opt.win_cand_waves > 0 ? c->opt.win_cand_waves : (npairs >= 8 ? 4 : 16);
    while (cw > 4 && win_cand_lds(A.cap2, A.wcap, cw) > 159 * 1024) cw >>= 1;
    const size_t lds1 = win_cand_lds(A.cap2, A.wcap, cw), rest2 = win_resolve_lds_rest(A.cap2, A.capq);
    A.lds_ents = (int)std::min<size_t>((size_t)A.ecap, rest2 < 159 * 1024 ? (159 * 1024 - rest2) / 8 : 0);
    const bool fits = A.lds_ents >= std::min(A.ecap, kWinLdsEntries);
    if (c->opt.win_lds_entries > 0) A.lds_ents = std::min(A.lds_ents, std::max(c->opt.win_lds_entries, (A.cap2 + 1) / 2));      // (the rotation histogram's bin masks reuse the buffer)
    const size_t lds2 = (size_t)A.lds_ents * 8 + rest2;
    if (lds1 > 159 * 1024 || !fits)        // (the kernels own a few words of static LDS besides)
        return set_err(c, EORB_E_CAPACITY, "%s: %zu / %zu B of LDS needed (searched frame %d, queries %d)", name, lds1, lds2, A.cap2, A.capq);
    int rc;
    // phase-1 products: entries | off | cnt | total
    const size_t ent_b = sizeof(uint64_t) * (size_t)npairs * A.ecap, oc_b = sizeof(uint32_t) * (size_t)npairs * A.capq;
    if ((rc = ensure(c, c->win_ws, ent_b + 2 * oc_b + 64))) return rc;
    A.ent = (uint64_t*)c->win_ws.p;
    A.off = (uint32_t*)((char*)c->win_ws.p + ent_b);
    A.cnt = A.off + (size_t)npairs * A.capq;
    // the pairs' entry counters start at zero: phase 2 leaves them so (a fill per call is a dependent launch of its own: 4 + 3 us)
    if (c->win_total_n < (size_t)npairs) {
        if ((rc = ensure(c, c->win_total, sizeof(uint32_t) * (size_t)npairs))) return rc;
        EORB_HIP(c, hipMemsetAsync(c->win_total.p, 0, c->win_total.cap, c->stream));
        c->win_total_n = c->win_total.cap / sizeof(uint32_t);
    }
    A.total = (uint32_t*)c->win_total.p;
    const size_t total_n = c->win_total_n;
    c->win_total_n = 0;                                 // (until both phases are known to have been launched)
    if ((rc = lds_optin(c, kOptWinCand + KIND, (const void*)win_cand_kernel<KIND>, 159 * 1024))) return rc;
    if ((rc = lds_optin(c, kOptWinResolve + KIND, (const void*)win_resolve_kernel<KIND>, 159 * 1024))) return rc;
    ProfScope ps(c, name);
    // queries per phase-1 workgroup: a lone pair is spread over as many workgroups as it has queries per wavefront (one each: 0.091 ->
    // 0.085 ms per SearchForInitialization call against two each; every workgroup stages the searched frame, 57 KB, from the L2)
    const int qpb = c->opt.win_qpb > 0 ? c->opt.win_qpb : (npairs >= 8 ? 32 : cw);
    win_cand_kernel<KIND><<<dim3((nq_max + qpb - 1) / qpb, npairs), 64 * cw, lds1, c->stream>>>(A, qpb);
    // (the fixed points of SearchForInitialization and SearchByProjection(cur, last) settle a window of blockDim queries at a time: the widest block)
    win_resolve_kernel<KIND><<<npairs, KIND == 2 ? 256 : 1024, lds2, c->stream>>>(A);
    EORB_LAUNCH_CHECK(c, name);
    c->win_total_n = total_n;
    return EORB_OK;
}

int search_init_dev(eorb_ctx* c, int npairs,
                    const eorb_keypoint* kps1, const int32_t* n1, size_t kp1_stride, const uint8_t* desc1, int dstride1, size_t desc1_slice,
                    const uint8_t* is_orb1,
                    const eorb_keypoint* kps2, const int32_t* n2, size_t kp2_stride, const uint8_t* desc2, int dstride2, size_t desc2_slice,
                    const uint8_t* is_orb2, int cap1, int cap2,
                    eorb_grid_bounds gb, float* prev_matched, int32_t* matches12, int windowSize, float nnratio,
                    int checkOri, int32_t* nmatches)
{
    if (npairs <= 0) return EORB_OK;
    WinArgs A{};
    A.kps2 = kps2; A.kp2_stride = kp2_stride; A.n2p = n2; A.desc2 = desc2; A.dstride2 = dstride2; A.desc2_slice = desc2_slice;
    A.is_orb2 = is_orb2; A.cap2 = cap2;
    A.nqp = n1; A.capq = cap1;
    A.kps1 = kps1; A.kp1_stride = kp1_stride; A.desc1 = desc1; A.dstride1 = dstride1; A.desc1_slice = desc1_slice; A.is_orb1 = is_orb1;
    A.prev_matched = prev_matched; A.windowSize = windowSize;
    A.g = grid_b(gb); A.nnratio = nnratio; A.checkOri = checkOri;
    A.matches12 = matches12; A.nmatches = nmatches;
    // a second-best candidate only matters while "bestDist < bestDist2 * ratio" (:772) can fail for some bestDist <= TH_LOW: every
    // dist2 with TH_LOW < dist2 * ratio passes like INT_MAX does (float product monotone in dist2); best candidates need dist <= TH_LOW
    A.dmax = first_dist(TH_LOW + 1, [&](int d) { return (float)TH_LOW < (float)d * nnratio; });
    return launch_win<0>(c, A, npairs, cap1, "search_init");
}

// a lone pair's searched frame
static void win_frame(WinArgs& A, const FrameDev& f) { A.kps2 = f.kps; A.n2 = f.n; A.cap2 = std::max(f.n, 1); A.desc2 = f.desc; A.dstride2 = f.stride; A.is_orb2 = f.is_orb; A.uright2 = f.uright; }

int search_proj_last_dev(eorb_ctx* c, const ProjLastArgs& P)
{
    WinArgs A{};
    win_frame(A, P.f);
    A.dist_th = P.dist_th; A.q_ur = P.q_ur;
    A.nq = P.nq; A.capq = std::max(P.nq, 1); A.qkps = P.q_kps; A.q_is_orb = P.q_is_orb; A.valid = P.valid; A.qf = P.uvs;
    A.mp_desc = P.mp_desc; A.mp_obs = P.mp_obs;
    A.g = P.g;
    A.slot_mp = P.slots; A.th = P.th; A.mode = P.mode; A.checkOri = P.checkOri; A.nmatches = P.nmatches;
    A.dmax = P.dist_th < 0 ? 0 : std::min(P.dist_th + 1, 256);      // best only: "if(bestDist<=TH_HIGH)" (:2140), bestDist starts at 256: every listed candidate
                                                                    // passes both tests, which phase 2's fixed point relies on
    return launch_win<1>(c, A, 1, P.nq, "search_proj_last");
}

int search_proj_map_dev(eorb_ctx* c, const ProjMapArgs& P)
{
    WinArgs A{};
    win_frame(A, P.f);
    A.q_ur = P.q_ur;
    A.nq = P.M; A.capq = std::max(P.M, 1); A.valid = P.in_view; A.qf = (const float*)P.qf; A.qlevel = P.level;
    A.mp_desc = P.mp_desc; A.mp_obs = P.mp_obs; A.mp_is_orb = P.mp_is_orb;
    A.g = P.g;
    A.slot_mp = P.slots; A.th = P.th; A.nnratio = P.nnratio; A.nmatches = P.nmatches;
    // the second best rejects only while "bestDist > ratio * bestDist2" (:134) can hold for some bestDist <= TH_HIGH
    A.dmax = std::min(256, first_dist(TH_HIGH + 1, [&](int d) { return !((float)TH_HIGH > P.nnratio * (float)d); }));
    return launch_win<2>(c, A, 1, P.M, "search_proj_map");
}


// ---------------------------------------------------------------------------------------------------
// Pieces shared by the walks over two DBoW2 feature vectors (SearchByBoW, its two-camera form, SearchForTriangulation) and by
// tc_search: 64-bit keys (distance on top, candidate order below) reduced over the wavefront by shuffles.  (The window matcher
// keeps its DPP forms wave_top2 / wave_min_u64.)
__device__ __forceinline__ void top2_insert(uint64_t key, uint64_t& k0, uint64_t& k1)
{   // (k0 <= k1 going in and out; selects, not branches: stores through a chosen reference would put the keys in scratch memory)
    const uint64_t hi = key < k0 ? k0 : key;
    k0 = key < k0 ? key : k0;
    k1 = hi < k1 ? hi : k1;
}

// every lane's (k0 <= k1) -> the wavefront's two smallest keys, in every lane
__device__ __forceinline__ void shfl_top2(uint64_t& k0, uint64_t& k1)
{
    uint64_t a = k0, b = k1;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o0 = __shfl_xor(a, d, 64), o1 = __shfl_xor(b, d, 64);
        const uint64_t l0 = a < o0 ? a : o0, h0 = a < o0 ? o0 : a, s1 = b < o1 ? b : o1;
        a = l0; b = h0 < s1 ? h0 : s1;
    }
    k0 = a; k1 = b;
}

__device__ __forceinline__ uint64_t shfl_min(uint64_t k)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint64_t o = __shfl_xor(k, d, 64); k = o < k ? o : k; }
    return k;
}

// position of `node` in fv.nodes or -1 (ids are ascending and unique: the reference's lower_bound walk).  The lanes look at 64
// positions at a time -- one memory round trip, not the seven dependent ones of a binary search.
__device__ __forceinline__ int find_node(const FeatVec& fv, uint32_t node, int lane)
{
    for (int base = 0; base < fv.nn; base += 64) {
        const int pos = base + lane;
        const uint64_t hit = __ballot(pos < fv.nn && fv.nodes[pos] == node);
        if (hit) return base + __ffsll((unsigned long long)hit) - 1;
    }
    return -1;
}

// one lane records a match: slot, counter, rotation bin (rotHist holds binAt: idx1 for (KF, KF), else bestIdxF) and histogram.
// ATOMIC: match_f is read by the wavefront's next KeyFrame feature through global memory (relaxed, agent scope).
template <bool ATOMIC>
__device__ __forceinline__ void bow_commit(const BowArgs& A, int realIdxKF, int bestIdxF, int binAt)
{
    if (ATOMIC) __hip_atomic_store(&A.match_f[bestIdxF], realIdxKF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else A.match_f[bestIdxF] = realIdxKF;
    atomicAdd(A.nmatches, 1);
    if (A.kf_kf) A.match12[realIdxKF] = bestIdxF;
    if (A.checkOri) {
        const int bin = rot_bin(A.kf_kps[realIdxKF].angle, A.f_kps[bestIdxF].angle);
        A.bin_f[binAt] = (int8_t)bin;
        atomicAdd(&A.histo[bin], 1);
    }
}

// ---------------------------------------------------------------------------------------------------
// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (:276-478), mono branch.  A frame feature belongs to
// exactly one vocabulary node, so the greedy state (vpMapPointMatches) never crosses nodes: shared nodes are matched
// concurrently (one wavefront each), KeyFrame features of a node sequentially, the node's frame features over the lanes.
__device__ __forceinline__ bool bow_accept(const BowArgs& A, uint64_t k0, uint64_t k1)
{
    if (k0 == ~0ull || (int)(k0 >> 32) >= 256) return false;
    const int bestDist1 = (int)(k0 >> 32);
    const int bestDist2 = (k1 != ~0ull && (int)(k1 >> 32) < 256) ? (int)(k1 >> 32) : 256;
    return (A.kf_kf ? bestDist1 < TH_LOW : bestDist1 <= TH_LOW) && (float)bestDist1 < A.nnratio * (float)bestDist2;
}

// node a of the KeyFrame side, one wavefront
__device__ __forceinline__ void bow_node(const BowArgs& A, int a, int lane)
{
    const int lo = find_node(A.f_fv, A.kf_fv.nodes[a], lane);
    if (lo < 0) return;
    const int f0 = A.f_fv.off[lo], f1 = A.f_fv.off[lo + 1];
    const int k0n = A.kf_fv.off[a], k1n = A.kf_fv.off[a + 1];
    if (f1 - f0 <= 64 && k1n - k0n <= 64) {
        // The usual node (about ten features on either side): everything it touches is loaded once -- lane = frame feature for the
        // candidates, lane = KeyFrame feature for the queries, handed round by shuffles.  A frame feature belongs to this node
        // only, so "already matched" (vpMapPointMatches[realIdxF] / vbMatched2) is a lane-local flag: no memory round trip between
        // the KeyFrame features of the node (the walk below took three dependent global loads per feature).
        const int nF = f1 - f0, nK = k1n - k0n;
        int idxF = -1; bool availF = false; uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
        if (lane < nF) {
            idxF = A.f_fv.idx[f0 + lane];
            availF = A.match_f[idxF] < 0 && !(A.kf_kf && !A.f_has_mp[idxF]);
            const uint64_t* tp = (const uint64_t*)(A.f_desc + (size_t)idxF * 32);
            t0 = tp[0]; t1 = tp[1]; t2 = tp[2]; t3 = tp[3];
        }
        int idxK = -1; bool hasK = false; uint64_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;
        if (lane < nK) {
            idxK = A.kf_fv.idx[k0n + lane];
            hasK = A.kf_has_mp[idxK] != 0;
            const uint64_t* dq = (const uint64_t*)(A.kf_desc + (size_t)idxK * 32);
            q0 = dq[0]; q1 = dq[1]; q2 = dq[2]; q3 = dq[3];
        }
        for (int i = 0; i < nK; i++) {
            if (!__shfl((int)hasK, i, 64)) continue;
            const uint64_t b0 = __shfl(q0, i, 64), b1 = __shfl(q1, i, 64), b2 = __shfl(q2, i, 64), b3 = __shfl(q3, i, 64);
            const int realIdxKF = __shfl(idxK, i, 64);
            uint64_t k0 = ~0ull, k1 = ~0ull;
            if (availF) {
                const int dist = __popcll(b0 ^ t0) + __popcll(b1 ^ t1) + __popcll(b2 ^ t2) + __popcll(b3 ^ t3);
                k0 = ((uint64_t)dist << 32) | (uint32_t)lane;          // candidate order = vector order = lane order
            }
            shfl_top2(k0, k1);
            if (bow_accept(A, k0, k1)) {
                const int win = (int)(k0 & 63u);
                const int bestIdxF = __shfl(idxF, win, 64);
                if (lane == win) availF = false;
                if (lane == 0) bow_commit<false>(A, realIdxKF, bestIdxF, A.kf_kf ? realIdxKF : bestIdxF);
            }
        }
        return;
    }
    for (int iKF = k0n; iKF < k1n; iKF++) {
        const int realIdxKF = A.kf_fv.idx[iKF];
        if (!A.kf_has_mp[realIdxKF]) continue;
        const uint64_t* dq = (const uint64_t*)(A.kf_desc + (size_t)realIdxKF * 32);
        const uint64_t q0 = dq[0], q1 = dq[1], q2 = dq[2], q3 = dq[3];
        // candidate order = vector order (iF): key = dist << 32 | iF keeps the reference's first-wins tie rule
        uint64_t k0 = ~0ull, k1 = ~0ull;
        for (int iF = f0 + lane; iF < f1; iF += 64) {
            const int realIdxF = A.f_fv.idx[iF];
            if (__hip_atomic_load(&A.match_f[realIdxF], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0) continue;   // vpMapPointMatches[realIdxF] / vbMatched2
            if (A.kf_kf && !A.f_has_mp[realIdxF]) continue;                      // !pMP2 || pMP2->isBad()
            const uint64_t* tp = (const uint64_t*)(A.f_desc + (size_t)realIdxF * 32);
            const int dist = __popcll(q0 ^ tp[0]) + __popcll(q1 ^ tp[1]) + __popcll(q2 ^ tp[2]) + __popcll(q3 ^ tp[3]);
            top2_insert(((uint64_t)dist << 32) | (uint32_t)iF, k0, k1);
        }
        shfl_top2(k0, k1);
        if (bow_accept(A, k0, k1)) {
            if (lane == 0) {
                const int bestIdxF = A.f_fv.idx[(int)(k0 & 0xffffffffu)];
                bow_commit<true>(A, realIdxKF, bestIdxF, A.kf_kf ? realIdxKF : bestIdxF);
            }
            __threadfence();          // the next KeyFrame feature of this node must see match_f
        }
    }
}

// ---- K pairs per launch: blockIdx.y = the pair, so the pair index and everything read with it is wave-uniform ----
__device__ __forceinline__ FeatVec fv_slice(const FeatVec& all, const KfSlice& s)
{
    return FeatVec{all.nodes + s.node0, all.off + s.off0, all.idx + s.idx0, s.nn};
}

// bow_node's block for pair k.  SearchByBoW(pKF_k, F): the set is the KeyFrame side and pair k owns match_f / bin_f slice k.
// SearchByBoW(pKF1, pKF2_k): the set is side 2 (the "frame" side of the walk); pair k owns match12 / bin_f slice k, and its vbMatched2
// flags (match_f) are the set's rows row0 .. of the scratch array.  Either way a wavefront orders match_f accesses only against its
// own earlier ones: a node of pair k touches only pair k's slice, at the features of that node.
__device__ __forceinline__ BowArgs bow_pair(const BowBatchArgs& B, int k)
{
    const KfSlice s = B.kf[k];
    BowArgs A = B.A;
    const size_t o = (size_t)k * B.n_out;
    // (offsets chosen by selects, one set of pointer additions: pointers assigned under a branch end up in scratch memory)
    const bool kk = A.kf_kf != 0;
    const int r1 = kk ? 0 : s.row0, r2 = kk ? s.row0 : 0;
    A.kf_kps += r1; A.kf_desc += (size_t)r1 * 32; A.kf_has_mp += r1;
    A.f_kps += r2; A.f_desc += (size_t)r2 * 32; A.f_has_mp += r2;
    A.kf_fv = FeatVec{A.kf_fv.nodes + (kk ? 0 : s.node0), A.kf_fv.off + (kk ? 0 : s.off0), A.kf_fv.idx + (kk ? 0 : s.idx0), kk ? A.kf_fv.nn : s.nn};
    A.f_fv = FeatVec{A.f_fv.nodes + (kk ? s.node0 : 0), A.f_fv.off + (kk ? s.off0 : 0), A.f_fv.idx + (kk ? s.idx0 : 0), kk ? s.nn : A.f_fv.nn};
    A.n_kf = kk ? A.n_kf : s.nrows; A.n_f = kk ? s.nrows : A.n_f;
    A.match_f += kk ? (size_t)s.row0 : o; A.match12 += kk ? o : 0;
    A.bin_f += o;
    A.histo += k * kPairHist; A.nmatches = A.histo + 32;
    return A;
}

__global__ __launch_bounds__(256) void search_bow_batch_kernel(BowBatchArgs B)
{
    const BowArgs A = bow_pair(B, blockIdx.y);
    const int lane = threadIdx.x & 63;
    const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    for (int a = gw; a < A.kf_fv.nn; a += nw) bow_node(A, a, lane);
}

// SearchByBoW(KeyFrame*, Frame&) on a two-camera frame (ORBmatcher.cc:276-478): per KeyFrame feature two best / second-best pairs,
// one over the frame's left features (index < nL) and one over its right ones (:357-377); the right best is taken only inside
// "if(bestDist1 <= TH_LOW)" (:410) and its ratio test is "... || true" (:412).  A frame feature belongs to one vocabulary node, so
// nodes run concurrently as in search_bow_batch_kernel: one wavefront per node, KeyFrame features in order, lanes over the node's frame
// features.  The rotation check reuses search_finish_batch_kernel (every frame slot is matched at most once).
__global__ __launch_bounds__(256) void search_bow_fisheye_kernel(BowBatchArgs B, int nL)
{
    const BowArgs A = bow_pair(B, blockIdx.y);
    const int lane = threadIdx.x & 63;
    const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    for (int a = gw; a < A.kf_fv.nn; a += nw) {
        const int lo = find_node(A.f_fv, A.kf_fv.nodes[a], lane);
        if (lo < 0) continue;
        const int f0 = A.f_fv.off[lo], f1 = A.f_fv.off[lo + 1];
        for (int iKF = A.kf_fv.off[a]; iKF < A.kf_fv.off[a + 1]; iKF++) {
            const int realIdxKF = A.kf_fv.idx[iKF];
            if (!A.kf_has_mp[realIdxKF]) continue;
            const uint64_t* dq = (const uint64_t*)(A.kf_desc + (size_t)realIdxKF * 32);
            const uint64_t q0 = dq[0], q1 = dq[1], q2 = dq[2], q3 = dq[3];
            uint64_t l0 = ~0ull, l1 = ~0ull, r0 = ~0ull, r1 = ~0ull;         // key = dist << 32 | iF (vector order breaks ties)
            for (int iF = f0 + lane; iF < f1; iF += 64) {
                const int realIdxF = A.f_fv.idx[iF];
                if (__hip_atomic_load(&A.match_f[realIdxF], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0) continue;
                const uint64_t* tp = (const uint64_t*)(A.f_desc + (size_t)realIdxF * 32);
                const int dist = __popcll(q0 ^ tp[0]) + __popcll(q1 ^ tp[1]) + __popcll(q2 ^ tp[2]) + __popcll(q3 ^ tp[3]);
                if (dist >= 256) continue;
                const uint64_t key = ((uint64_t)dist << 32) | (uint32_t)iF;
                if (realIdxF < nL) top2_insert(key, l0, l1); else top2_insert(key, r0, r1);
            }
            shfl_top2(l0, l1);
            shfl_top2(r0, r1);
            const int bestDist1 = l0 == ~0ull ? 256 : (int)(l0 >> 32);
            if (bestDist1 > TH_LOW) continue;
            const int bestDist2 = l1 == ~0ull ? 256 : (int)(l1 >> 32);
            if (lane == 0) {
                if ((float)bestDist1 < A.nnratio * (float)bestDist2) {
                    const int bestIdxF = A.f_fv.idx[(int)(l0 & 0xffffffffu)];
                    bow_commit<true>(A, realIdxKF, bestIdxF, bestIdxF);
                }
                if (r0 != ~0ull && (int)(r0 >> 32) <= TH_LOW) {                  // ratio "|| true" (:412)
                    const int bestIdxFR = A.f_fv.idx[(int)(r0 & 0xffffffffu)];
                    bow_commit<true>(A, realIdxKF, bestIdxFR, bestIdxFR);
                }
            }
            __threadfence();          // the next KeyFrame feature of this node must see match_f
        }
    }
}

// three_maxima one bin at a time (the running state after bin i, then the 10 % rule) for rot_finish, whose loop over the bins is not
// unrolled.  The window matchers and the fisheye walk keep three_maxima itself, the form their generated code was measured with.
struct Maxima3 { int max1 = 0, max2 = 0, max3 = 0, a = -1, b = -1, c = -1; };
__device__ __forceinline__ void maxima3_step(Maxima3& m, int s, int i)
{
    const bool g1 = s > m.max1, g2 = s > m.max2, g3 = s > m.max3;      // (max1 >= max2 >= max3: g1 implies g2 implies g3)
    m.c = g2 ? m.b : (g3 ? i : m.c); m.max3 = g2 ? m.max2 : (g3 ? s : m.max3);
    m.b = g1 ? m.a : (g2 ? i : m.b); m.max2 = g1 ? m.max1 : (g2 ? s : m.max2);
    m.a = g1 ? i : m.a;              m.max1 = g1 ? s : m.max1;
}
__device__ __forceinline__ void maxima3_end(Maxima3 m, int& ind1, int& ind2, int& ind3)
{
    if ((float)m.max2 < 0.1f * (float)m.max1) { m.b = -1; m.c = -1; }
    else if ((float)m.max3 < 0.1f * (float)m.max1) { m.c = -1; }
    ind1 = m.a; ind2 = m.b; ind3 = m.c;
}

// the rotation check's end (ComputeThreeMaxima + the erase loop) over the n slots of out whose bins were recorded
__device__ __forceinline__ void rot_finish(int32_t* out, const int8_t* bin, int n, int32_t* histo, int32_t* nmatches)
{
    __shared__ int keep;
    if (threadIdx.x == 0) {
        // (one bin at a time: unrolled, the 30 scalar loads and the compare masks of all steps are live at once and 55 SGPRs spill)
        Maxima3 m;
#pragma unroll 1
        for (int i = 0; i < HISTO_LENGTH; i++) maxima3_step(m, histo[i], i);
        int i1, i2, i3;
        maxima3_end(m, i1, i2, i3);
        int k = 0;
        if (i1 >= 0) k |= 1 << i1; if (i2 >= 0) k |= 1 << i2; if (i3 >= 0) k |= 1 << i3;
        keep = k;
    }
    __syncthreads();
    int dec = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int b = bin[i];
        if (b >= 0 && !(keep & (1 << b)) && out[i] >= 0) { out[i] = -1; dec++; }
    }
    if (dec) atomicSub(nmatches, dec);
}

// one block per pair
__global__ void search_finish_batch_kernel(int32_t* out, const int8_t* bin, int n, int32_t* histo)
{
    const size_t o = (size_t)blockIdx.x * n;
    int32_t* h = histo + blockIdx.x * kPairHist;
    rot_finish(out + o, bin + o, n, h, h + 32);
}

// K pairs: every output slot and bin -1, histograms and counters 0, the keyframe-to-keyframe form's vbMatched2 flags -1
__global__ void search_init_batch_kernel(int32_t* out, int8_t* bin, int nout, int32_t* histo, int nhist, int32_t* scratch, int nscratch)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nout) { out[i] = -1; bin[i] = -1; }
    if (i < nhist) histo[i] = 0;
    if (i < nscratch) scratch[i] = -1;
}

static void search_init_batch(eorb_ctx* c, int32_t* out, int8_t* bin, int K, int n_out, int32_t* histo, int32_t* scratch, int nscratch)
{
    const int nout = K * n_out, nhist = K * kPairHist;          // (K * n_out <= 2^22: the entry points' limit)
    search_init_batch_kernel<<<(std::max(std::max(nout, nhist), nscratch) + 255) / 256, 256, 0, c->stream>>>(out, bin, nout, histo, nhist, scratch, nscratch);
}

// three launches for any K: init, walk (one wavefront per pair and KeyFrame-side node), rotation finish (one block per pair).  name: the
// entry point's profile scope; nL >= 0: the walk of a two-camera frame (nL left features, then right ones)
int search_bow_batch_dev(eorb_ctx* c, const char* name, const BowBatchArgs& B, int32_t* scratch, int nscratch, int nL)
{
    ProfScope ps(c, name);
    int32_t* out = B.A.kf_kf ? B.A.match12 : B.A.match_f;
    search_init_batch(c, out, B.A.bin_f, B.K, B.n_out, B.A.histo, scratch, nscratch);
    if (B.max_nn > 0) {
        const dim3 grid(std::min((B.max_nn + 3) / 4, 1024), B.K);
        if (nL >= 0) search_bow_fisheye_kernel<<<grid, 256, 0, c->stream>>>(B, nL);
        else search_bow_batch_kernel<<<grid, 256, 0, c->stream>>>(B);
        if (B.A.checkOri) search_finish_batch_kernel<<<B.K, 256, 0, c->stream>>>(out, B.A.bin_f, B.n_out, B.A.histo);
    }
    EORB_LAUNCH_CHECK(c, name);
    return EORB_OK;
}

// ---------------------------------------------------------------------------------------------------
// local-mapping matcher: mono branch of ORBmatcher::SearchForTriangulation (:975-1214; MixedMatcher.cpp:1326-1573).
// vbMatched2 is never written in the reference, so every pKF1 feature is independent: one wave per feature-vector entry of
// pKF1, lanes over the pKF2 features of the same vocabulary node.  The sequential update rule (skip dist > bestDist, replace
// on pass) keeps the passing candidate with the least distance, the LAST one among equals: key = dist << 32 | ~position.
// The geometric check has no side effects, so a lane runs it only for a candidate that would beat its own best key: the minimum
// over passing candidates is the reference's answer.
//
// tri_walk is the whole walk; a geometry policy G supplies what depends on pCamera1:
//   G(args, id1, e1, kp1)   the per-pKF1-feature setup
//   epipole_gate(e2)        whether the epipole-distance test applies to this pair (:1093-1105)
//   ok(id2, kp2)            pCamera1->epipolarConstrain(...) (:1107-1137)

__device__ __forceinline__ bool epipolar_ok(float x1, float y1, float x2, float y2, const float* F, float unc)
{   // Pinhole::epipolarConstrain (src/CameraModels/Pinhole.cpp:142-156) with F12 given
    const float a = x1 * F[0] + y1 * F[3] + F[6];
    const float b = x1 * F[1] + y1 * F[4] + F[7];
    const float c = x1 * F[2] + y1 * F[5] + F[8];
    const float num = a * x2 + b * y2 + c;
    const float den = a * a + b * b;
    if (den == 0) return false;
    const float dsqr = num * num / den;
    return dsqr < 3.84f * unc;
}

// entry p of fv1, one wavefront
template <class G, class Args>
__device__ __forceinline__ void tri_entry(const TriArgs& A, const Args& GA, int p, int lane)
{
    const int id1 = A.fv1.idx[p];
    const uint8_t e1 = A.elig1[id1];                // bit 0: eligible; bit 1: rectified-stereo keypoint (mvuRight >= 0, bStereo1 :1051)
    if (!(e1 & 1)) return;
    int lo = 0, hi = A.fv1.nn;                      // node a with off1[a] <= p < off1[a+1]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (A.fv1.off[mid] <= p) lo = mid; else hi = mid; }
    const uint32_t node = A.fv1.nodes[lo];
    int l2 = 0, h2 = A.fv2.nn;
    while (l2 < h2) { const int mid = (l2 + h2) >> 1; if (A.fv2.nodes[mid] < node) l2 = mid + 1; else h2 = mid; }
    if (l2 >= A.fv2.nn || A.fv2.nodes[l2] != node) return;
    const eorb_keypoint kp1 = A.kps1[id1];
    const G g(GA, id1, e1, kp1);
    uint64_t q0, q1, q2, q3;
    load_desc32(A.desc1 + (size_t)id1 * A.stride1, q0, q1, q2, q3);
    uint64_t k0 = ~0ull;
    for (int i2 = A.fv2.off[l2] + lane; i2 < A.fv2.off[l2 + 1]; i2 += 64) {
        const int id2 = A.fv2.idx[i2];
        const uint8_t e2 = A.elig2[id2];
        if (!(e2 & 1)) continue;
        uint64_t t0, t1, t2, t3;
        load_desc32(A.desc2 + (size_t)id2 * A.stride2, t0, t1, t2, t3);
        const int dist = __popcll(q0 ^ t0) + __popcll(q1 ^ t1) + __popcll(q2 ^ t2) + __popcll(q3 ^ t3);
        if (dist > TH_LOW) continue;
        const uint64_t key = ((uint64_t)dist << 32) | (uint32_t)(~(uint32_t)i2);
        if (key >= k0) continue;                                           // cannot change this lane's answer
        const eorb_keypoint kp2 = A.kps2[id2];
        if (kp2.octave < 0 || kp2.octave >= A.nlevels) continue;            // rejected on the host already
        if (g.epipole_gate(e2)) {
            const float distex = A.epx - kp2.x, distey = A.epy - kp2.y;
            if (distex * distex + distey * distey < 100 * A.scale2[kp2.octave]) continue;
        }
        if (!(A.bCoarse || g.ok(id2, kp2))) continue;
        k0 = key;
    }
    k0 = shfl_min(k0);
    if (lane == 0 && k0 != ~0ull) {
        const int bestIdx2 = A.fv2.idx[(int)(~(uint32_t)(k0 & 0xffffffffu))];
        A.match12[id1] = bestIdx2;
        atomicAdd(A.nmatches, 1);
        if (A.checkOri) {
            const int bin = rot_bin(kp1.angle, A.kps2[bestIdx2].angle);
            A.bin1[id1] = (int8_t)bin;
            atomicAdd(&A.histo[bin], 1);
        }
    }
}

template <class G, class Args>
__device__ __forceinline__ void tri_walk(const TriArgs& A, const Args& GA)
{
    const int lane = threadIdx.x & 63;
    const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
    const int total = A.fv1.off[A.fv1.nn];
    for (int p = gw; p < total; p += nw) tri_entry<G>(A, GA, p, lane);
}

struct TriPinhole {                  // pCamera1 = Pinhole: the test on F12
    const TriArgs& A; const uint8_t e1; const float x1, y1;
    __device__ __forceinline__ TriPinhole(const TriArgs& a, int, uint8_t e, const eorb_keypoint& kp1) : A(a), e1(e), x1(kp1.x), y1(kp1.y) {}
    __device__ __forceinline__ bool epipole_gate(uint8_t e2) const { return !((e1 | e2) & 2); }      // "if(!bStereo1 && !bStereo2 && !pKF1->mpCamera2)" :1093
    __device__ __forceinline__ bool ok(int, const eorb_keypoint& kp2) const { return epipolar_ok(x1, y1, kp2.x, kp2.y, A.F, A.sigma2_2[kp2.octave]); }
};

// pCamera1 = KannalaBrandt8: epipolarConstrain = TriangulateMatches(...) > KB8_DEF_TH_EPC (KannalaBrandt8.cpp:315-320, :416-486).
// Two-camera keyframes (nleft >= 0) pick one of four poses and cameras per (left/right, left/right) pair (:1107-1137) and skip
// the epipole test; bStereo is false for them (:1051, :1079).
struct TriKbPairView { const TriKbArgs& K; const float* Rt; int nleft2; };       // pair k: the block, its poses (ll, lr, rl, rr) and pKF2_k's nleft
struct TriKb8 {
    const TriKbArgs& K; const float* const Rt; const int nleft2; const int bRight1; const bool bStereo1; const float x1, y1, sig1;
    __device__ __forceinline__ TriKb8(const TriKbPairView& v, int id1, uint8_t e1, const eorb_keypoint& kp1)
        : K(v.K), Rt(v.Rt), nleft2(v.nleft2), bRight1(v.K.nleft1 >= 0 && id1 >= v.K.nleft1), bStereo1(v.K.nleft1 < 0 && (e1 & 2)), x1(kp1.x), y1(kp1.y),
          sig1(v.K.sigma2_1[kp1.octave]) {}
    __device__ __forceinline__ bool twocam() const { return K.nleft1 >= 0; }
    __device__ __forceinline__ bool epipole_gate(uint8_t e2) const { return !twocam() && !bStereo1 && !(e2 & 2); }      // :1097-1105
    __device__ __forceinline__ bool ok(int id2, const eorb_keypoint& kp2) const
    {
        const int bRight2 = twocam() && id2 >= nleft2;
        const int pose = twocam() ? (bRight1 << 1 | bRight2) : 0;       // ll, lr, rl, rr
        const WarpCam c1 = warp_cam_of(K.cam1[twocam() ? bRight1 : 0]);
        const WarpCam c2 = warp_cam_of(K.cam2[twocam() ? bRight2 : 0]);
        return kb8_triangulate_matches(c1, c2, x1, y1, kp2.x, kp2.y, Rt + 12 * pose, Rt + 12 * pose + 9, sig1,
                                       K.T.sigma2_2[kp2.octave]) > 0.0001f;       // KB8_DEF_TH_EPC
    }
};

// K pairs per launch (blockIdx.y = the pair): pKF1 and the level tables stay as in T; pKF2_k, its epipole and F12 come from the tables
__device__ __forceinline__ TriArgs tri_pair(const TriArgs& T, const KfSlice* kf, const TriPair* pair, int k, bool pinhole)
{
    const KfSlice s = kf[k];
    TriArgs A = T;
    A.kps2 += s.row0; A.n2 = s.nrows; A.desc2 += (size_t)s.row0 * A.stride2; A.elig2 += s.row0; A.fv2 = fv_slice(A.fv2, s);
    A.epx = pair[k].epx; A.epy = pair[k].epy;
    if (pinhole) for (int i = 0; i < 9; i++) A.F[i] = pair[k].F[i];
    const size_t o = (size_t)k * A.n1;
    A.match12 += o; A.bin1 += o;
    A.histo += k * kPairHist; A.nmatches = A.histo + 32;
    return A;
}

// two kernels, not one with a run-time camera switch: the Pinhole walk needs a third of the KannalaBrandt8 one's registers
__global__ __launch_bounds__(256) void search_tri_batch_kernel(TriBatchArgs B)
{
    const TriArgs A = tri_pair(B.T, B.kf, B.pair, blockIdx.y, true);
    tri_walk<TriPinhole>(A, A);
}

__global__ __launch_bounds__(256) void search_tri_kb8_batch_kernel(TriKbBatchArgs B)
{
    const TriArgs A = tri_pair(B.K.T, B.kf, B.pair, blockIdx.y, false);
    const TriKbPair* kb = B.kb + blockIdx.y;
    tri_walk<TriKb8>(A, TriKbPairView{B.K, kb->Rt, kb->nleft2});
}

// init, walk (one wavefront per pair and entry of fv1), rotation finish (one block per pair); name: the entry point's profile scope
int search_tri_batch_dev(eorb_ctx* c, const char* name, const TriBatchArgs& B, const TriKbBatchArgs* K)
{
    ProfScope ps(c, name);
    const TriArgs& T = B.T;
    search_init_batch(c, T.match12, T.bin1, B.K, T.n1, T.histo, nullptr, 0);
    const dim3 grid(std::min((T.n1 + 3) / 4 + 1, 2048), B.K);
    if (K) search_tri_kb8_batch_kernel<<<grid, 256, 0, c->stream>>>(*K);
    else search_tri_batch_kernel<<<grid, 256, 0, c->stream>>>(B);
    if (T.checkOri) search_finish_batch_kernel<<<B.K, 256, 0, c->stream>>>(T.match12, T.bin1, T.n1, T.histo);
    EORB_LAUNCH_CHECK(c, name);
    return EORB_OK;
}

// KannalaBrandt8::TriangulateMatches over n keypoint pairs (one thread each): z1 or -1
__global__ void kb8_tri_batch_kernel(WarpCam c1, WarpCam c2, Pose12 P, const eorb_keypoint* __restrict__ kps1,
                                     const eorb_keypoint* __restrict__ kps2, int n, const float* __restrict__ sig1,
                                     const float* __restrict__ sig2, float* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const eorb_keypoint a = kps1[i], b = kps2[i];
    out[i] = kb8_triangulate_matches(c1, c2, a.x, a.y, b.x, b.y, P.v, P.v + 9, sig1[a.octave], sig2[b.octave]);
}

int kb8_tri_batch_dev(eorb_ctx* c, const eorb_camera* cam1, const eorb_camera* cam2, const float* Rt, const eorb_keypoint* kps1,
                      const eorb_keypoint* kps2, int n, const float* sig1, const float* sig2, float* out)
{
    ProfScope ps(c, "kb8_triangulate_matches");
    Pose12 P;
    for (int i = 0; i < 12; i++) P.v[i] = Rt[i];
    kb8_tri_batch_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(warp_cam_of(*cam1), warp_cam_of(*cam2), P, kps1, kps2, n, sig1, sig2, out);
    EORB_LAUNCH_CHECK(c, "kb8_tri_batch_kernel");
    return EORB_OK;
}

// ---------------------------------------------------------------------------------------------------
// search core of ORBmatcher::Fuse (:1512-1578, :1700-1720), SearchBySim3 (:1829-1860, :1909-1940) and
// SearchByProjection(KeyFrame*, Scw, ...) (:548-588): best keypoint (least distance, first in GetFeaturesInArea order) with
// octave in [L-1, L] inside the radius.  SEQ = false: queries independent, one wave each.  SEQ = true (vpMatched feeds later
// queries): one workgroup walks the queries in order.  Both read RadBatchArgs: the keyframes' keypoints concatenated (kf_off[K + 1]),
// query (k, m) at entry k * M + m of the query arrays; a single keyframe is K = 1.

// the cell word: Frame::PosInGrid as the 12-bit cell number ix*48+iy (64 x 48 = 3072 cells), 0xFFFF outside the grid
__device__ __forceinline__ uint16_t kf_cell_of(const eorb_keypoint& k, const GridB& g)
{
    const int px = dev_round_index((k.x - g.minX) * g.invW);
    const int py = dev_round_index((k.y - g.minY) * g.invH);
    return (px < 0 || px >= kGridCols || py < 0 || py >= kGridRows) ? (uint16_t)0xFFFF : (uint16_t)(px * kGridRows + py);
}
// the mixed forms carry the row's type in the cell word: bit 15 set = not an ORB row (!isORBDescValid(idx)); 0xFFFF stays "outside"
constexpr int kCellNotOrb = 0x8000;
__device__ __forceinline__ uint16_t kf_cell_mixed(const eorb_keypoint& k, const GridB& g, const uint8_t* __restrict__ kp_is_orb, int i)
{
    const uint16_t cell = kf_cell_of(k, g);
    return (cell != 0xFFFF && kp_is_orb && !kp_is_orb[i]) ? (uint16_t)(cell | kCellNotOrb) : cell;
}

// the cells of every keyframe's keypoints in one launch
template <bool MIXED>
__global__ void kf_cells_batch_kernel(const eorb_keypoint* __restrict__ kps, int ntotal, const int32_t* __restrict__ kf_off, int K,
                                      const GridB* __restrict__ g, const uint8_t* __restrict__ kp_is_orb, uint16_t* __restrict__ cell)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntotal) return;
    int lo = 0, hi = K - 1;                                     // the keyframe of keypoint i: the last k with kf_off[k] <= i
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (kf_off[mid] <= i) lo = mid; else hi = mid - 1; }
    cell[i] = MIXED ? kf_cell_mixed(kps[i], g[lo], kp_is_orb, i) : kf_cell_of(kps[i], g[lo]);
}

// MIXED: the search loop of MixedMatcher::Fuse (src/MixedMatcher.cpp:1703-1758, :1891-1921) and MixedMatcher::SearchByProjection(pKF,
// Scw, ...) (:1136-1170, :1266-1300): a candidate of another type than the map point is skipped (isORBMP != isORBDescValid(idx)), the
// level is getKPtLevelMono(idx) (octave of an ORB row, class_id of an AKAZE row) and the reprojection gate reads getKPtInvLevelSigma2(idx)
// per keypoint.  The type test comes first and costs no load (the cell word has the bit); kp_inv_sigma2[i] is read last.
template <bool SEQ, bool MIXED, typename Args>             // Args: RadArgs, or RadArgsMixed where MIXED
__device__ __forceinline__ uint64_t radius_scan(const Args& A, int m, int first, int step, const uint8_t* taken)
{
    const float u = A.uv[2 * m], v = A.uv[2 * m + 1], r = A.radius[m];
    int cx0, cx1, cy0, cy1;
    uint64_t k0 = ~0ull;
    if (!cell_range(A.g, u, v, r, cx0, cx1, cy0, cy1)) return k0;
    const int L = A.level[m];
    int mp_type = 0;
    if constexpr (MIXED) mp_type = (A.mp_is_orb && !A.mp_is_orb[m]) ? kCellNotOrb : 0;
    uint64_t q0, q1, q2, q3;
    load_desc32(A.q_desc + (size_t)m * 32, q0, q1, q2, q3);
    for (int i = first; i < A.n; i += step) {
        int cell = A.cell[i];
        if (cell == 0xFFFF) continue;
        if (MIXED) {
            if ((cell & kCellNotOrb) != mp_type) continue;
            cell &= kCellNotOrb - 1;
        }
        const int cx = cell / kGridRows, cy = cell - cx * kGridRows;
        if (cx < cx0 || cx > cx1 || cy < cy0 || cy > cy1) continue;
        const eorb_keypoint k = A.kps[i];
        const float distx = k.x - u, disty = k.y - v;
        if (!(fabsf(distx) < r && fabsf(disty) < r)) continue;
        if (SEQ && taken[i]) continue;
        const int kpLevel = (MIXED && mp_type) ? k.class_id : k.octave;
        if (kpLevel < L - 1 || kpLevel > L) continue;
        // (two gates in full rather than one with a selected sigma: the ORB instantiation keeps the code it had, instruction for instruction)
        if constexpr (MIXED) {
            if (A.kp_inv_sigma2) {
                const float ex = u - k.x, ey = v - k.y;
                const float kpr = A.uright ? A.uright[i] : -1.f;
                if (kpr >= 0.f) {                                              // src/MixedMatcher.cpp:1721-1734
                    const float er = A.q_ur[m] - kpr;
                    const float e2 = ex * ex + ey * ey + er * er;
                    if ((double)(e2 * A.kp_inv_sigma2[i]) > 7.8) continue;     // e2*pKF->getKPtInvLevelSigma2(idx)
                } else {
                    const float e2 = ex * ex + ey * ey;
                    if ((double)(e2 * A.kp_inv_sigma2[i]) > 5.99) continue;
                }
            }
        } else if (A.inv_sigma2) {
            if (k.octave < 0 || k.octave >= A.nlevels) continue;
            const float ex = u - k.x, ey = v - k.y;
            const float kpr = A.uright ? A.uright[i] : -1.f;
            if (kpr >= 0.f) {                                                  // "Check reprojection error in stereo" :1541-1553
                const float er = A.q_ur[m] - kpr;
                const float e2 = ex * ex + ey * ey + er * er;
                if ((double)(e2 * A.inv_sigma2[k.octave]) > 7.8) continue;
            } else {
                const float e2 = ex * ex + ey * ey;
                if ((double)(e2 * A.inv_sigma2[k.octave]) > 5.99) continue;
            }
        }
        uint64_t t0, t1, t2, t3;
        load_desc32(A.desc + (size_t)i * A.stride, t0, t1, t2, t3);
        const int dist = __popcll(q0 ^ t0) + __popcll(q1 ^ t1) + __popcll(q2 ^ t2) + __popcll(q3 ^ t3);
        const uint64_t key = ((uint64_t)dist << 44) | ((uint64_t)cell << 32) | (uint32_t)i;
        if (key < k0) k0 = key;
    }
    return k0;
}

template <bool MIXED> using RadArgsOf = std::conditional_t<MIXED, RadArgsMixed, RadArgs>;
template <bool MIXED> using RadBatchArgsOf = std::conditional_t<MIXED, RadBatchArgsMixed, RadBatchArgs>;

// keyframe k of the block as radius_scan reads it: its keypoint range with its grid bounds, its M queries.  (B by value: through a
// reference to the kernel's argument the ORB batch kernel takes two more SGPRs.)
template <bool MIXED>
__device__ __forceinline__ RadArgsOf<MIXED> rad_pair(const RadBatchArgsOf<MIXED> B, int k)
{
    const int off = B.kf_off[k];
    const size_t qo = (size_t)k * B.M;
    RadArgsOf<MIXED> A{};
    A.kps = B.kps + off; A.n = B.kf_off[k + 1] - off; A.desc = B.desc + (size_t)off * B.stride; A.stride = B.stride;
    A.g = B.g[k]; A.cell = B.cell + off;
    A.M = B.M; A.valid = B.valid + qo; A.uv = B.uv + 2 * qo; A.radius = B.radius + qo; A.level = B.level + qo;
    A.q_desc = B.q_desc + (size_t)k * B.q_desc_kstride;
    A.inv_sigma2 = B.inv_sigma2; A.nlevels = B.nlevels;
    A.uright = B.uright ? B.uright + off : nullptr; A.q_ur = B.uright ? B.q_ur + qo : nullptr;
    A.taken = B.taken; A.accept_thr = B.accept_thr;
    A.best_idx = B.best_idx + qo; A.best_dist = B.best_dist + qo;
    if constexpr (MIXED) { A.mp_is_orb = B.mp_is_orb; A.kp_inv_sigma2 = B.kp_inv_sigma2 ? B.kp_inv_sigma2 + off : nullptr; }
    return A;
}

// One wavefront per query runs radius_scan<false> over keyframe k's keypoint range; the queries are independent.
template <bool MIXED>
__global__ __launch_bounds__(256) void kf_radius_batch_kernel(RadBatchArgsOf<MIXED> B)
{
    const int lane = threadIdx.x & 63;
    const int64_t gw = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t nq = (int64_t)B.K * B.M;
    for (int64_t q = gw; q < nq; q += nw) {
        const int k = (int)(q / B.M);
        const RadArgsOf<MIXED> A = rad_pair<MIXED>(B, k);
        const int m = (int)(q - (int64_t)k * B.M);
        uint64_t k0 = ~0ull;
        if (A.valid[m]) k0 = radius_scan<false, MIXED>(A, m, lane, 64, nullptr);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint64_t o = __shfl_xor(k0, d, 64); k0 = o < k0 ? o : k0; }
        if (lane == 0) {
            const bool ok = k0 != ~0ull && (int)(k0 >> 44) < 256;
            B.best_idx[q] = ok ? (int)(k0 & 0xffffffffu) : -1;
            B.best_dist[q] = ok ? (int)(k0 >> 44) : 256;
        }
    }
}

// The in-order form (K = 1): one workgroup, the vpMatched flags in LDS, the queries one after another.
template <bool MIXED>
__global__ __launch_bounds__(256) void kf_radius_seq_kernel(RadBatchArgsOf<MIXED> B)
{
    const RadArgsOf<MIXED> A = rad_pair<MIXED>(B, 0);
    extern __shared__ unsigned char smem[];
    uint64_t* red = (uint64_t*)smem;
    uint8_t* taken = (uint8_t*)(red + 8);
    for (int i = threadIdx.x; i < A.n; i += blockDim.x) taken[i] = A.taken[i];
    __syncthreads();
    for (int m = 0; m < A.M; m++) {
        uint64_t k0 = ~0ull, k1 = ~0ull;
        if (A.valid[m]) k0 = radius_scan<true, MIXED>(A, m, threadIdx.x, blockDim.x, taken);
        block_top2(k0, k1, red);
        if (threadIdx.x == 0) {
            const bool ok = k0 != ~0ull && (int)(k0 >> 44) < 256;
            const int bi = ok ? (int)(k0 & 0xffffffffu) : -1, bd = ok ? (int)(k0 >> 44) : 256;
            A.best_idx[m] = bi; A.best_dist[m] = bd;
            if (ok && (float)bd <= A.accept_thr) taken[bi] = 1;
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < A.n; i += blockDim.x) A.taken[i] = taken[i];
}

// the agreement pass of SearchBySim3 (:1948-1964) over a 2 x M batch: row 0 = KF1's points searched in KF2, row 1 the reverse
__global__ void sim3_agree_kernel(const int32_t* __restrict__ best_idx, const int32_t* __restrict__ best_dist, int M, int N1, int N2,
                                  int th_high, int32_t* __restrict__ vn1, int32_t* __restrict__ vn2, int32_t* __restrict__ match12,
                                  int32_t* __restrict__ nfound)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N2) vn2[i] = best_dist[M + i] <= th_high ? best_idx[M + i] : -1;
    bool found = false;
    if (i < N1) {
        const int idx2 = best_dist[i] <= th_high ? best_idx[i] : -1;
        vn1[i] = idx2;
        if (idx2 >= 0 && idx2 < N2) {
            const int idx1 = best_dist[M + idx2] <= th_high ? best_idx[M + idx2] : -1;
            found = idx1 == i;
        }
        match12[i] = found ? idx2 : -1;
    }
    const unsigned long long b = __ballot(found);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(nfound, __popcll(b));
}

template <bool MIXED>
static int kf_radius_launch(eorb_ctx* c, const char* name, const RadBatchArgsOf<MIXED>& B, int ntotal, const uint8_t* d_kp_is_orb)
{
    const int64_t nq = (int64_t)B.K * B.M;
    if (nq <= 0) return EORB_OK;
    if (B.taken && B.K != 1) return set_err(c, EORB_E_ARG, "%s: the in-order search takes one keyframe", name);
    ProfScope ps(c, name);
    if (ntotal > 0)
        kf_cells_batch_kernel<MIXED><<<(ntotal + 255) / 256, 256, 0, c->stream>>>(B.kps, ntotal, B.kf_off, B.K, B.g, d_kp_is_orb, B.cell);
    if (B.taken) {
        const size_t lds = 64 + (((size_t)ntotal + 15) & ~(size_t)15);
        if (lds > 160 * 1024) return set_err(c, EORB_E_CAPACITY, "kf_radius_match: %d keypoints exceed the LDS flags", ntotal);
        int rc;
        if ((rc = lds_optin(c, MIXED ? kOptKfRadiusMixed : kOptKfRadius, (const void*)kf_radius_seq_kernel<MIXED>, 160 * 1024))) return rc;
        kf_radius_seq_kernel<MIXED><<<1, 256, lds, c->stream>>>(B);
    } else {
        kf_radius_batch_kernel<MIXED><<<(unsigned)std::min<int64_t>((nq + 3) / 4, 8192), 256, 0, c->stream>>>(B);
    }
    EORB_LAUNCH_CHECK(c, name);
    return EORB_OK;
}
int kf_radius_dev(eorb_ctx* c, const char* name, bool mixed, const RadBatchArgsMixed& B, int ntotal, const uint8_t* d_kp_is_orb)
{
    return mixed ? kf_radius_launch<true>(c, name, B, ntotal, d_kp_is_orb) : kf_radius_launch<false>(c, name, B, ntotal, nullptr);
}

int sim3_agree_dev(eorb_ctx* c, const int32_t* best_idx, const int32_t* best_dist, int M, int N1, int N2, int th_high,
                   int32_t* vn1, int32_t* vn2, int32_t* match12, int32_t* nfound)
{
    EORB_HIP(c, hipMemsetAsync(nfound, 0, sizeof(int32_t), c->stream));
    const int n = std::max(N1, N2);
    if (n <= 0) return EORB_OK;
    sim3_agree_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(best_idx, best_dist, M, N1, N2, th_high, vn1, vn2, match12, nfound);
    EORB_LAUNCH_CHECK(c, "sim3_agree_kernel");
    return EORB_OK;
}

// ---------------------------------------------------------------------------------------------------
// DBoW2 TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup)
// (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1125-1250): the producer of the feature vectors the SearchByBoW kernels consume.
// K-a: one wave per feature walks the tree; lanes = children of the current node (FORB::distance = popcount), first minimum wins.
__global__ __launch_bounds__(256) void bow_descend_kernel(const uint8_t* __restrict__ desc, int n, int stride, BowVoc V, int nid_level,
                                                          uint32_t* __restrict__ word_of, double* __restrict__ w_of, uint32_t* __restrict__ node_of)
{
    const int lane = threadIdx.x & 63;
    const int f = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (f >= n) return;
    uint64_t q0, q1, q2, q3;
    load_desc32(desc + (size_t)f * stride, q0, q1, q2, q3);
    int node = 0, level = 0, nid = 0;
    do {
        ++level;
        const int c0 = V.child_off[node], nc = V.child_off[node + 1] - c0;
        uint64_t key = ~0ull;
        for (int c = lane; c < nc; c += 64) {
            const int id = V.child_ids[c0 + c];
            uint64_t t0, t1, t2, t3;
            load_desc32(V.node_desc + (size_t)id * 32, t0, t1, t2, t3);
            const int d = __popcll(q0 ^ t0) + __popcll(q1 ^ t1) + __popcll(q2 ^ t2) + __popcll(q3 ^ t3);
            const uint64_t k = ((uint64_t)d << 32) | (uint32_t)c;
            key = k < key ? k : key;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const uint64_t o = __shfl_xor(key, d, 64); key = o < key ? o : key; }
        node = V.child_ids[c0 + (int)(key & 0xffffffffu)];
        if (level == nid_level) nid = node;
    } while (V.child_off[node + 1] > V.child_off[node] && level < 64);
    if (lane == 0) {
        const double w = V.weight[node];
        const bool keep = w > 0;                               // stopped words carry weight 0
        word_of[f] = keep ? (uint32_t)V.word_id[node] : 0xffffffffu;
        w_of[f] = w;
        node_of[f] = keep ? (uint32_t)nid : 0xffffffffu;
    }
}

// bitonic sort of P (power of two) 64-bit keys in LDS by the whole workgroup (1024 threads).  Thread t keeps keys t, t + 1024, ... in
// registers: partners less than 64 apart are exchanged by lane shuffles, partners a multiple of 1024 apart are the thread's own
// registers, and only the distances 64 .. 512 go through LDS and two barriers (10 of the 55 steps of a 1024-key sort).
__device__ __forceinline__ uint64_t blk_shfl_xor_u64(uint64_t v, int j)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, j, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), j, 64);
    return ((uint64_t)hi << 32) | lo;
}
template <int M>
__device__ void block_bitonic_sort_regs(uint64_t* keys, int P)
{
    constexpr int NT = 1024;
    const int tid = threadIdx.x;
    __syncthreads();
    uint64_t v[M];
#pragma unroll
    for (int m = 0; m < M; m++) { const int i = tid + NT * m; v[m] = i < P ? keys[i] : ~0ull; }
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= NT) {
#pragma unroll
                for (int dm = 1; dm < M; dm <<= 1) {
                    if (j != dm * NT) continue;
#pragma unroll
                    for (int m = 0; m < M; m++) {
                        if ((m & dm) == 0 && (m | dm) < M) {
                            const int i = tid + NT * m;
                            const bool up = (i & k) == 0;
                            const uint64_t x = v[m], y = v[m | dm];
                            const bool sw = (x > y) == up;
                            v[m] = sw ? y : x; v[m | dm] = sw ? x : y;
                        }
                    }
                }
            } else if (j >= 64) {
#pragma unroll
                for (int m = 0; m < M; m++) { const int i = tid + NT * m; if (i < P) keys[i] = v[m]; }
                __syncthreads();
                uint64_t o[M];
#pragma unroll
                for (int m = 0; m < M; m++) { const int i = tid + NT * m; o[m] = i < P ? keys[i ^ j] : ~0ull; }
                __syncthreads();
#pragma unroll
                for (int m = 0; m < M; m++) {
                    const int i = tid + NT * m;
                    const bool up = (i & k) == 0, low = (i & j) == 0;
                    const uint64_t mn = v[m] < o[m] ? v[m] : o[m], mx = v[m] < o[m] ? o[m] : v[m];
                    v[m] = (low == up) ? mn : mx;
                }
            } else {
#pragma unroll
                for (int m = 0; m < M; m++) {
                    const int i = tid + NT * m;
                    const uint64_t o = blk_shfl_xor_u64(v[m], j);
                    const bool up = (i & k) == 0, low = (i & j) == 0;
                    const uint64_t mn = v[m] < o ? v[m] : o, mx = v[m] < o ? o : v[m];
                    v[m] = (low == up) ? mn : mx;
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < M; m++) { const int i = tid + NT * m; if (i < P) keys[i] = v[m]; }
    __syncthreads();
}
__device__ __forceinline__ void block_bitonic_sort(uint64_t* keys, int P)
{
    if (blockDim.x == 1024) {
        if (P <= 1024) { block_bitonic_sort_regs<1>(keys, P); return; }
        if (P <= 2048) { block_bitonic_sort_regs<2>(keys, P); return; }
        if (P <= 4096) { block_bitonic_sort_regs<4>(keys, P); return; }
        if (P <= 8192) { block_bitonic_sort_regs<8>(keys, P); return; }
    }
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < P; i += blockDim.x) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t a = keys[i], b = keys[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { keys[i] = b; keys[ixj] = a; }
                }
            }
        }
    }
    __syncthreads();
}

// run heads of the sorted keys (upper 32 bits = run id) -> exclusive run index per element, number of runs; wave 0 scans.  A run index
// is below m <= 8192 (bow_plan.h), so 16 bits hold it
__device__ __forceinline__ int block_run_index(const uint64_t* keys, int m, uint16_t* ridx)
{
    __shared__ int s_runs;
    if (threadIdx.x < 64) {
        int run = 0;
        for (int i0 = 0; i0 < m; i0 += 64) {
            const int i = i0 + (int)threadIdx.x;
            const int head = (i < m) && (i == 0 || (uint32_t)(keys[i] >> 32) != (uint32_t)(keys[i - 1] >> 32));
            int incl = head;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d, 64); if ((int)threadIdx.x >= d) incl += t; }
            if (i < m) ridx[i] = (uint16_t)(run + incl - 1);
            run += __shfl(incl, 63, 64);
        }
        if (threadIdx.x == 0) s_runs = run;
    }
    __syncthreads();
    return s_runs;
}

// K-b: one workgroup turns the per-feature (word, weight, node) triples into the BowVector (std::map order = ascending word id,
// weights accumulated in feature order, then BowVector::normalize) and the FeatureVector (ascending node id, features in
// push_back order).
__global__ __launch_bounds__(1024) void bow_assemble_kernel(const uint32_t* __restrict__ word_of, const double* __restrict__ w_of,
                                                            const uint32_t* __restrict__ node_of, int n, int P, int weighting, int norm,
                                                            uint32_t* __restrict__ bow_word, double* __restrict__ bow_val,
                                                            uint32_t* __restrict__ fv_node, int32_t* __restrict__ fv_off, int32_t* __restrict__ fv_idx,
                                                            int32_t* __restrict__ counts /* n_words, n_fvnodes */)
{
    extern __shared__ unsigned char smem[];
    uint64_t* keys = (uint64_t*)smem;                       // P
    double* vals = (double*)(keys + P);                     // P: the words' values (summed for the norm from here, not from global memory)
    uint16_t* ridx = (uint16_t*)(vals + P);                 // P (bow_plan.h: 18 bytes per key)
    __shared__ int s_m;
    __shared__ double s_norm;
    // ---- BowVector ----
    for (int i = threadIdx.x; i < P; i += blockDim.x)
        keys[i] = (i < n && word_of[i] != 0xffffffffu) ? (((uint64_t)word_of[i] << 32) | (uint32_t)i) : ~0ull;
    block_bitonic_sort(keys, P);
    if (threadIdx.x == 0) {                                  // valid features sort first: m = first sentinel
        int lo = 0, hi = P;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] != ~0ull) lo = mid + 1; else hi = mid; }
        s_m = lo;
    }
    __syncthreads();
    const int m = s_m;
    const int nw = block_run_index(keys, m, ridx);
    for (int i = threadIdx.x; i < m; i += blockDim.x) {
        if (i == 0 || ridx[i] != ridx[i - 1]) {              // run head: addWeight in feature order (same word -> same weight)
            const double w = w_of[(int)(keys[i] & 0xffffffffu)];
            double v = w;
            if (weighting == 0 || weighting == 1)
                for (int j = i + 1; j < m && ridx[j] == ridx[i]; j++) v += w;
            bow_word[ridx[i]] = (uint32_t)(keys[i] >> 32);
            vals[ridx[i]] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double nrm = 0.0;
        if (norm == 1) { for (int i = 0; i < nw; i++) nrm += fabs(vals[i]); }
        else if (norm == 2) { for (int i = 0; i < nw; i++) nrm += vals[i] * vals[i]; nrm = sqrt(nrm); }
        else if (weighting == 0 || weighting == 1) nrm = (double)nw;     // "unnecessary when normalizing" branch :1166-1172
        s_norm = nrm;
        counts[0] = nw;
    }
    __syncthreads();
    {
        const bool div = s_norm > 0.0 && (norm != 0 || weighting == 0 || weighting == 1);
        for (int i = threadIdx.x; i < nw; i += blockDim.x) bow_val[i] = div ? vals[i] / s_norm : vals[i];
    }
    __syncthreads();
    // ---- FeatureVector ----
    for (int i = threadIdx.x; i < P; i += blockDim.x)
        keys[i] = (i < n && node_of[i] != 0xffffffffu) ? (((uint64_t)node_of[i] << 32) | (uint32_t)i) : ~0ull;
    block_bitonic_sort(keys, P);
    const int nn = block_run_index(keys, m, ridx);
    for (int i = threadIdx.x; i < m; i += blockDim.x) {
        fv_idx[i] = (int32_t)(keys[i] & 0xffffffffu);
        if (i == 0 || ridx[i] != ridx[i - 1]) { fv_node[ridx[i]] = (uint32_t)(keys[i] >> 32); fv_off[ridx[i]] = i; }
    }
    if (threadIdx.x == 0) { fv_off[nn] = m; counts[1] = nn; }
}

int bow_transform_dev(eorb_ctx* c, const uint8_t* d_desc, int n, int stride, const BowVoc& V, int levelsup, int weighting, int norm,
                      uint32_t* d_word_of, double* d_w_of, uint32_t* d_node_of, uint32_t* d_bow_word, double* d_bow_val,
                      uint32_t* d_fv_node, int32_t* d_fv_off, int32_t* d_fv_idx, int32_t* d_counts)
{
    const BowPlan B = plan_bow_transform(n);
    if (!B.ok) return set_err(c, EORB_E_CAPACITY, "bow_transform: %d features, at most %d per call (the LDS sort)", n, kBowMaxFeatures);
    const int P = B.P;
    const size_t lds = B.lds;
    int rc;
    if ((rc = lds_optin(c, kOptBowAssemble, (const void*)bow_assemble_kernel, kBowLdsOptin))) return rc;
    ProfScope ps(c, "bow_transform");
    bow_descend_kernel<<<(n + 3) / 4, 256, 0, c->stream>>>(d_desc, n, stride, V, V.L - levelsup, d_word_of, d_w_of, d_node_of);
    bow_assemble_kernel<<<1, 1024, lds, c->stream>>>(d_word_of, d_w_of, d_node_of, n, P, weighting, norm, d_bow_word, d_bow_val,
                                                     d_fv_node, d_fv_off, d_fv_idx, d_counts);
    EORB_LAUNCH_CHECK(c, "bow_transform kernels");
    return EORB_OK;
}

// generic windowed matcher (SURVEY §8(b) eorb_hamming_window_match): one wave per query, lanes over its candidate list; key =
// dist << 32 | position keeps the reference's first-wins order for both the best and the second best
__global__ __launch_bounds__(256) void window_match_kernel(const uint8_t* __restrict__ q_desc, int nq, int q_stride,
                                                           const uint8_t* __restrict__ t_desc, int t_stride,
                                                           const int32_t* __restrict__ off, const int32_t* __restrict__ cand,
                                                           int32_t* __restrict__ out /* 4 x nq */)
{
    const int lane = threadIdx.x & 63;
    const int q = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (q >= nq) return;
    uint64_t q0, q1, q2, q3;
    load_desc32(q_desc + (size_t)q * q_stride, q0, q1, q2, q3);
    uint64_t k0 = ~0ull, k1 = ~0ull;
    const int c0 = off[q], c1 = off[q + 1];
    for (int k = c0 + lane; k < c1; k += 64) {
        const int c = cand[k];
        uint64_t t0, t1, t2, t3;
        load_desc32(t_desc + (size_t)c * t_stride, t0, t1, t2, t3);
        const int d = __popcll(q0 ^ t0) + __popcll(q1 ^ t1) + __popcll(q2 ^ t2) + __popcll(q3 ^ t3);
        const uint64_t key = ((uint64_t)d << 32) | (uint32_t)(k - c0);
        if (key < k0) { k1 = k0; k0 = key; } else if (key < k1) k1 = key;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o0 = __shfl_xor(k0, d, 64), o1 = __shfl_xor(k1, d, 64);
        const uint64_t lo = k0 < o0 ? k0 : o0, hi = k0 < o0 ? o0 : k0, s1 = k1 < o1 ? k1 : o1;
        k0 = lo; k1 = hi < s1 ? hi : s1;
    }
    if (lane == 0) {
        // the sequential rule only records a second best that was seen while it was >= the then-best: with first-wins ties the
        // top two keys of (dist, position) are exactly best and second
        const bool hb = k0 != ~0ull, hs = k1 != ~0ull;
        out[q] = hb ? cand[c0 + (int)(k0 & 0xffffffffu)] : -1;
        out[nq + q] = hb ? (int)(k0 >> 32) : 256;
        out[2 * nq + q] = hs ? cand[c0 + (int)(k1 & 0xffffffffu)] : -1;
        out[3 * nq + q] = hs ? (int)(k1 >> 32) : 256;
    }
}

int window_match_dev(eorb_ctx* c, const uint8_t* d_q, int nq, int q_stride, const uint8_t* d_t, int t_stride, const int32_t* d_off,
                     const int32_t* d_cand, int32_t* d_out)
{
    if (nq <= 0) return EORB_OK;
    ProfScope ps(c, "hamming_window_match");
    window_match_kernel<<<(nq + 3) / 4, 256, 0, c->stream>>>(d_q, nq, q_stride, d_t, t_stride, d_off, d_cand, d_out);
    EORB_LAUNCH_CHECK(c, "window_match_kernel");
    return EORB_OK;
}

// MixedFrame::sortFeaturesResponse (MixedFrame.cpp:211-225): stable descending order by response.
// rank(i) = #{j : r_j > r_i} + #{j < i : r_j == r_i}; perm[rank(i)] = i.  n is a few thousand at most.
__global__ void sort_response_kernel(const eorb_keypoint* __restrict__ kps, int n, int32_t* __restrict__ perm)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float r = kps[i].response;
    int rank = 0;
    for (int j = 0; j < n; j++) {
        const float q = kps[j].response;
        rank += (q > r) || (q == r && j < i);
    }
    perm[rank] = i;
}

int sort_response_dev(eorb_ctx* c, const eorb_keypoint* d_kps, int n, int32_t* d_perm)
{
    if (n <= 0) return EORB_OK;
    ProfScope ps(c, "sort_response");
    sort_response_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(d_kps, n, d_perm);
    EORB_LAUNCH_CHECK(c, "sort_response_kernel");
    return EORB_OK;
}


// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:349-423), batched over map points: one workgroup per map point,
// thread i owns row i of the N x N distance matrix; its median is read off a 257-bin counting histogram (distances are
// integers in [0, 256]); the first row with the smallest median wins.
// The bins are 16 bits wide and bins d and d ^ 1 share the 32-bit word that the atomic adds to, so a row may hold at most 65 535
// equal distances: one more carries out of the low bin into its neighbour (or out of the word).  A row has N distances, so
// eorb_distinctive_descriptors refuses a map point with N > 65 535 (EORB_E_CAPACITY) before anything is launched.
__global__ __launch_bounds__(256) void distinctive_kernel(const uint8_t* __restrict__ desc, const int32_t* __restrict__ offsets,
                                                          int32_t* __restrict__ best)
{
    __shared__ uint16_t hist[64 * 260];
    __shared__ unsigned long long s_best;
    const int m = blockIdx.x;
    const int o0 = offsets[m], N = offsets[m + 1] - o0;
    if (N <= 0) { if (threadIdx.x == 0) best[m] = -1; return; }
    if (threadIdx.x == 0) s_best = ~0ull;
    __syncthreads();
    const uint8_t* D = desc + 32 * (size_t)o0;
    const int k = (int)(0.5 * (double)(N - 1));          // vDists[0.5*(N-1)]
    for (int r0 = 0; r0 < N; r0 += 64) {                  // 64 rows at a time; 4 threads per row split the columns
        const int row = r0 + (threadIdx.x >> 2), part = threadIdx.x & 3;
        uint16_t* h = hist + (threadIdx.x >> 2) * 260;
        for (int b = part; b < 257; b += 4) h[b] = 0;
        __syncthreads();
        if (row < N) {
            uint64_t q[4];
            load_desc32(D + 32 * (size_t)row, q[0], q[1], q[2], q[3]);
            for (int j = part; j < N; j += 4) {
                uint64_t t0, t1, t2, t3;
                load_desc32(D + 32 * (size_t)j, t0, t1, t2, t3);
                const int d = (j == row) ? 0 : (__popcll(q[0] ^ t0) + __popcll(q[1] ^ t1) + __popcll(q[2] ^ t2) + __popcll(q[3] ^ t3));
                atomicAdd((unsigned int*)(h + (d & ~1)), (d & 1) ? 0x10000u : 1u);     // 16-bit counter inside its 32-bit word
            }
        }
        __syncthreads();
        if (row < N && part == 0) {
            int acc = 0, median = 256;
            for (int b = 0; b < 257; b++) { acc += h[b]; if (acc > k) { median = b; break; } }
            const unsigned long long key = ((unsigned long long)median << 32) | (unsigned int)row;   // first minimum wins
            atomicMin(&s_best, key);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) best[m] = (int32_t)(s_best & 0xffffffffu);
}

int distinctive_dev(eorb_ctx* c, const uint8_t* d_desc, const int32_t* d_offsets, int M, int32_t* d_best)
{
    if (M <= 0) return EORB_OK;
    ProfScope ps(c, "distinctive_descriptors");
    distinctive_kernel<<<M, 256, 0, c->stream>>>(d_desc, d_offsets, d_best);
    EORB_LAUNCH_CHECK(c, "distinctive_kernel");
    return EORB_OK;
}

int bf_knn2_dev(eorb_ctx* c, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int32_t* d_idx2, int32_t* d_dist2)
{
    if (nq <= 0) return EORB_OK;
    ProfScope ps(c, "bf_knn2");
    if (nq >= 16 * 1024) bf_knn2_kernel<16><<<(nq + 15) / 16, 256, 0, c->stream>>>(d_q, nq, d_t, nt, d_idx2, d_dist2);
    else if (nq >= 8 * 512) bf_knn2_kernel<32><<<(nq + 7) / 8, 256, 0, c->stream>>>(d_q, nq, d_t, nt, d_idx2, d_dist2);
    else bf_knn2_kernel<64><<<(nq + 3) / 4, 256, 0, c->stream>>>(d_q, nq, d_t, nt, d_idx2, d_dist2);
    EORB_LAUNCH_CHECK(c, "bf_knn2_kernel");
    return EORB_OK;
}


// ---------------------------------------------------------------------------------------------------
// Two-camera (fisheye stereo) frames: Frame::Frame(imLeft, imRight, ..., pCamera, pCamera2, Tlr) (src/Frame.cc:1101-1208) and the
// numKPtsLeft() != -1 branches of the tracking matchers.  A frame holds nL left keypoints followed by nR right ones (mvKeys, then
// mvKeysRight; descriptors concatenated, :1176) and two grids over the same bounds (AssignFeaturesToGrid :431-460: the left grid
// holds mvKeys, the right one mvKeysRight).

// ComputeStereoFishEyeMatches (:1210-1250) after the knnMatch of the lapping rows (bf_knn2_kernel with `lap`): Lowe's test
// "size() >= 2 && [0].distance < [1].distance * 0.7" (:1233; float distances against a double product).  Per left keypoint:
// cand = right keypoint index (trainIdx + monoRight) or -1, dist2 = the two knn distances (-1: none / outside the lapping area).
// lap = {nL, nR, monoLeft, monoRight}; lap[4] counts the candidates (zeroed by the caller).
__global__ __launch_bounds__(256) void fisheye_lowe_kernel(int32_t* __restrict__ lap, const int32_t* __restrict__ idx2,
                                                           const int32_t* __restrict__ kdist2, int cap, int32_t* __restrict__ cand,
                                                           int32_t* __restrict__ dist2)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int nL = lap[0], mL = lap[2], mR = lap[3];
    if (i >= cap || i >= nL) return;
    int c = -1, d0 = -1, d1 = -1;
    if (i >= mL) {
        const int qi = i - mL;
        const int i0 = idx2[2 * qi], i1 = idx2[2 * qi + 1];
        if (i0 >= 0) d0 = kdist2[2 * qi];
        if (i1 >= 0) d1 = kdist2[2 * qi + 1];
        if (i1 >= 0 && (double)(float)d0 < (double)(float)d1 * 0.7) { c = i0 + mR; atomicAdd(&lap[4], 1); }
    }
    cand[i] = c; dist2[2 * i] = d0; dist2[2 * i + 1] = d1;
}

int fisheye_lowe_dev(eorb_ctx* c, const uint8_t* d_descL, const uint8_t* d_descR, int cap, int32_t* d_lap, int32_t* d_idx2,
                     int32_t* d_kdist2, int32_t* d_cand, int32_t* d_dist2)
{
    if (cap <= 0) return EORB_OK;
    ProfScope ps(c, "fisheye_stereo_matches");
    // (the launch covers every row a frame can have: the kernel takes the counts from the device)
    bf_knn2_kernel<64><<<(cap + 3) / 4, 256, 0, c->stream>>>(d_descL, cap, d_descR, cap, d_idx2, d_kdist2, d_lap);
    fisheye_lowe_kernel<<<(cap + 255) / 256, 256, 0, c->stream>>>(d_lap, d_idx2, d_kdist2, cap, d_cand, d_dist2);
    EORB_LAUNCH_CHECK(c, "fisheye stereo matches");
    return EORB_OK;
}

// The two tracking SearchByProjection overloads on a two-camera frame (ORBmatcher.cc:44-219 and :1969-2187).  Every query makes a
// left and a right sub-query, and a match can claim two slots (the partner links); later queries see those slots through the
// Observations() > 0 test in both camera spaces, so the sub-queries run in the reference's order.  One workgroup builds both grids
// in LDS (cell starts, keypoint positions, levels, slot states); then one wavefront walks the sub-queries: lanes over the window's
// cells, each lane over its cell's keypoints, the two smallest keys by wave reduction.  key = dist << 44 | cell << 32 | index << 8
// | level + 1: the reference's candidate order (cell ix, cell iy, insertion index) rides in the key for the tie-breaks, as in
// win_key.  Descriptors are read from global memory (only those of window candidates).
constexpr int kTcCells = kGridCols * kGridRows;
constexpr int32_t kTcObs = 1 << 30;              // slot state bit: the slot's map point has Observations() > 0


struct TcLds {
    uint32_t* cst;                               // 2 * kTcCells: after the build, cst[x] = end of cell x = start of cell x + 1
    float2* pos; int32_t* slot; uint16_t* item; int8_t* lgate; int8_t* lbest;
};

// Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel, bRight = cam) (src/Frame.cc:710-781) + the Observations() > 0 skip +
// DescriptorDistance.  The level gate reads getKPtLevelMono(j) (:763), i.e. lgate (see the build).  Result: the two smallest keys
// in every lane; *hit = the window was not empty (before the slot test).
__device__ void tc_search(const TcArgs& A, const TcLds& S, int cam, float qx, float qy, float r, int minL, int maxL,
                          const uint64_t* qd, int lane, uint64_t& k0, uint64_t& k1, bool& hit)
{
    k0 = k1 = ~0ull; hit = false;
    int cx0, cx1, cy0, cy1;
    if (!cell_range(A.g, qx, qy, r, cx0, cx1, cy0, cy1)) return;
    const int ncy = cy1 - cy0 + 1, nc = (cx1 - cx0 + 1) * ncy;
    const bool chk = (minL > 0) || (maxL >= 0);
    bool any = false;
    for (int ci = lane; ci < nc; ci += 64) {
        const int ix = cx0 + ci / ncy, iy = cy0 + ci % ncy;
        const int cell = ix * kGridRows + iy, x = cam * kTcCells + cell;
        const uint32_t e = S.cst[x];
        for (uint32_t p = x ? S.cst[x - 1] : 0u; p < e; p++) {
            const int gi = S.item[p];
            if (chk) {
                const int lv = S.lgate[gi];
                if (lv < minL) continue;
                if (maxL >= 0 && lv > maxL) continue;
            }
            const float2 P = S.pos[gi];
            if (!(fabsf(P.x - qx) < r && fabsf(P.y - qy) < r)) continue;
            any = true;
            const int32_t sv = S.slot[gi];
            if (sv == -2 || (sv >= 0 && (sv & kTcObs))) continue;              // getMapPoint(idx)->Observations() > 0
            uint64_t t0, t1, t2, t3;
            load_desc32(A.desc + (size_t)gi * A.stride, t0, t1, t2, t3);
            const int dist = __popcll(qd[0] ^ t0) + __popcll(qd[1] ^ t1) + __popcll(qd[2] ^ t2) + __popcll(qd[3] ^ t3);
            if (dist >= 256) continue;                                          // (never below bestDist = 256)
            top2_insert(((uint64_t)dist << 44) | ((uint64_t)cell << 32) | ((uint64_t)(uint32_t)gi << 8) | (uint64_t)((S.lbest[gi] + 1) & 0xff), k0, k1);
        }
    }
    hit = __ballot(any) != 0;
    shfl_top2(k0, k1);
}

__device__ __forceinline__ int tc_dist(uint64_t k) { return k == ~0ull ? 256 : (int)(k >> 44); }
__device__ __forceinline__ int tc_idx(uint64_t k) { return (int)((k >> 8) & 0xffffffu); }
__device__ __forceinline__ int tc_level(uint64_t k) { return k == ~0ull ? -1 : (int)(k & 0xffu) - 1; }

// slot write by lane 0, seen by the wavefront's next sub-query
__device__ __forceinline__ void tc_set(const TcLds& S, int lane, int gi, int32_t v)
{
    if (lane == 0) S.slot[gi] = v;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

template <int KIND>
__global__ __launch_bounds__(256) void twocam_walk_kernel(TcArgs A)
{
    extern __shared__ unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int nL = A.nL, nT = A.nL + A.nR;
    TcLds S;
    S.cst = (uint32_t*)smem;
    S.pos = (float2*)(smem + (((size_t)2 * kTcCells * 4 + 15) & ~(size_t)15));
    S.slot = (int32_t*)(S.pos + nT);
    S.item = (uint16_t*)(S.slot + nT);
    S.lgate = (int8_t*)(S.item + nT);
    S.lbest = S.lgate + nT;
    __shared__ uint32_t s_part[256];
    __shared__ int s_hist[HISTO_LENGTH];
    // ---- both grids (AssignFeaturesToGrid :431-460): counts, scan, placement ----
    for (int i = tid; i < 2 * kTcCells; i += blockDim.x) S.cst[i] = 0;
    if (tid < HISTO_LENGTH) s_hist[tid] = 0;
    __syncthreads();
    for (int gi = tid; gi < nT; gi += blockDim.x) {
        const eorb_keypoint k = A.kps[gi];
        const int cam = gi >= nL;
        S.pos[gi] = make_float2(k.x, k.y);
        S.lbest[gi] = (int8_t)k.octave;
        // getKPtLevelMono(j) = mvKeysUn[j].octave for the right grid's j too (Frame.cc:763, :1417-1420): LEFT keypoint j; for j >= nL
        // (past mvKeysUn) the right keypoint's own octave (upstream ORB-SLAM3's reading)
        const int j = gi - nL;
        S.lgate[gi] = (int8_t)(cam && j < nL ? A.kps[j].octave : k.octave);
        int32_t v = A.slots[gi];
        if (v >= 0 && A.mp_obs[v]) v |= kTcObs;
        S.slot[gi] = v;
        const int px = dev_round_index((k.x - A.g.minX) * A.g.invW), py = dev_round_index((k.y - A.g.minY) * A.g.invH);   // PosInGrid :783-793
        if (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows) atomicAdd(&S.cst[cam * kTcCells + px * kGridRows + py], 1u);
    }
    __syncthreads();
    {   // exclusive scan of the 2 * kTcCells counts: chunk per thread, then the chunk totals
        const int per = (2 * kTcCells + (int)blockDim.x - 1) / (int)blockDim.x;
        const int lo = tid * per, hi = min(lo + per, 2 * kTcCells);
        uint32_t sum = 0;
        for (int i = lo; i < hi; i++) sum += S.cst[i];
        s_part[tid] = sum;
        __syncthreads();
        for (int o = 1; o < (int)blockDim.x; o <<= 1) {
            const uint32_t add = tid >= o ? s_part[tid - o] : 0u;
            __syncthreads();
            s_part[tid] += add;
            __syncthreads();
        }
        uint32_t run = tid ? s_part[tid - 1] : 0u;
        for (int i = lo; i < hi; i++) { const uint32_t n = S.cst[i]; S.cst[i] = run; run += n; }
    }
    __syncthreads();
    for (int gi = tid; gi < nT; gi += blockDim.x) {
        const float2 P = S.pos[gi];
        const int px = dev_round_index((P.x - A.g.minX) * A.g.invW), py = dev_round_index((P.y - A.g.minY) * A.g.invH);
        if (px >= 0 && px < kGridCols && py >= 0 && py < kGridRows)
            S.item[atomicAdd(&S.cst[(gi >= nL) * kTcCells + px * kGridRows + py], 1u)] = (uint16_t)gi;   // (order inside a cell: the key's index)
    }
    __syncthreads();
    if (tid >= 64) return;
    // ---- the sub-queries, in the reference's order ----
    int nm = 0, nrec = 0;
    for (int q = 0; q < A.nq; q++) {
        uint64_t qd[4];
        const uint64_t* dq = (const uint64_t*)(A.mp_desc + (size_t)q * 32);
        uint64_t k0, k1; bool hit;
        if (KIND == 0) {
            const bool iv = A.in_view[q] != 0, ivr = A.in_view_r[q] != 0 && A.qlevel_r[q] != -1;
            if (!iv && !ivr) continue;
            qd[0] = dq[0]; qd[1] = dq[1]; qd[2] = dq[2]; qd[3] = dq[3];
            const int32_t mark = q | (A.mp_obs[q] ? kTcObs : 0);
            if (iv) {
                const float4 f = A.qf[q];
                const int lev = A.qlevel[q];
                float r = ((double)f.z > 0.998) ? 2.5f : 4.0f;                  // RadiusByViewingCos (:221-227)
                if (A.th != 1.0f) r *= A.th;                                    // bFactor (:49, :70-71)
                tc_search(A, S, 0, f.x, f.y, r * f.w, lev - 1, lev, qd, lane, k0, k1, hit);
                const int bestDist = tc_dist(k0);
                if (bestDist <= TH_HIGH) {
                    const int bestLevel = tc_level(k0), bestLevel2 = tc_level(k1), bestDist2 = tc_dist(k1);
                    if (bestLevel == bestLevel2 && (float)bestDist > A.nnratio * (float)bestDist2) continue;   // :130: no right search either
                    const int bestIdx = tc_idx(k0);
                    tc_set(S, lane, bestIdx, mark); nm++;
                    const int rj = A.l2r[bestIdx];
                    if (rj != -1) { tc_set(S, lane, nL + rj, mark); nm++; }     // :136-137
                }
            }
            if (ivr) {
                const float4 f = A.qf_r[q];
                const int lev = A.qlevel_r[q];
                const float r = ((double)f.z > 0.998) ? 2.5f : 4.0f;            // mTrackViewCosR, no th (:152)
                tc_search(A, S, 1, f.x, f.y, r * f.w, lev - 1, lev, qd, lane, k0, k1, hit);
                const int bestDist = tc_dist(k0);
                if (bestDist <= TH_HIGH) {
                    const int bestLevel = tc_level(k0), bestLevel2 = tc_level(k1), bestDist2 = tc_dist(k1);
                    if (bestLevel == bestLevel2 && (float)bestDist > A.nnratio * (float)bestDist2) continue;
                    const int bestIdx = tc_idx(k0) - nL;
                    const int li = A.r2l[bestIdx];
                    if (li != -1) { tc_set(S, lane, li, mark); nm++; }         // :204-205
                    tc_set(S, lane, nL + bestIdx, mark); nm++;
                }
            }
        } else {
            if (!A.valid[q]) continue;
            qd[0] = dq[0]; qd[1] = dq[1]; qd[2] = dq[2]; qd[3] = dq[3];
            const float* u = A.quv + (size_t)q * 5;
            const eorb_keypoint qk = A.qkps[q];
            const int oct = qk.octave;                                          // getKPtLevelMono(i) (:2014, :2114)
            const float radius = A.th * u[4];
            const int minL = A.mode == 1 ? oct : (A.mode == 2 ? 0 : oct - 1);
            const int maxL = A.mode == 1 ? -1 : (A.mode == 2 ? oct : oct + 1);
            const int32_t mark = q | (A.mp_obs[q] ? kTcObs : 0);
            tc_search(A, S, 0, u[0], u[1], radius, minL, maxL, qd, lane, k0, k1, hit);
            if (!hit) continue;                                                 // vIndices2.empty() (:2032-2033): no right search
            if (tc_dist(k0) <= TH_HIGH) {
                const int gi = tc_idx(k0);
                tc_set(S, lane, gi, mark); nm++;
                if (A.checkOri) {
                    const int bin = rot_bin(qk.angle, A.kps[gi].angle);
                    if (lane == 0) { A.rec[nrec] = gi << 5 | bin; s_hist[bin]++; }
                    nrec++;
                }
            }
            tc_search(A, S, 1, u[2], u[3], radius, minL, maxL, qd, lane, k0, k1, hit);    // (:2116-2123: no bounds check)
            if (tc_dist(k0) <= TH_HIGH) {
                const int gi = tc_idx(k0);
                tc_set(S, lane, gi, mark); nm++;
                if (A.checkOri) {
                    const int bin = rot_bin(qk.angle, A.kps[gi].angle);         // rotHist gets nL + j (:2155)
                    if (lane == 0) { A.rec[nrec] = gi << 5 | bin; s_hist[bin]++; }
                    nrec++;
                }
            }
        }
    }
    if (KIND == 1 && A.checkOri) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        int h[HISTO_LENGTH];
        for (int i = 0; i < HISTO_LENGTH; i++) h[i] = s_hist[i];
        int i1, i2, i3;
        three_maxima(h, HISTO_LENGTH, i1, i2, i3);                              // ComputeThreeMaxima (:2167-2184): both camera spaces
        int drop = 0;
        for (int e = lane; e < nrec; e += 64) {
            const int32_t rv = A.rec[e];
            const int b = rv & 31;
            if (b != i1 && b != i2 && b != i3) { S.slot[rv >> 5] = -1; drop++; }   // setMapPoint(NULL); nmatches-- per entry
        }
        nm -= wave_sum_i32(drop);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    for (int gi = lane; gi < nT; gi += 64) {
        const int32_t v = S.slot[gi];
        A.slots[gi] = v >= 0 ? (v & ~kTcObs) : v;
    }
    if (lane == 0) *A.nmatches = nm;
}

int twocam_walk_dev(eorb_ctx* c, int kind, const TcArgs& A)
{
    const int nT = A.nL + A.nR;
    if (nT > kTcMaxKps) return set_err(c, EORB_E_CAPACITY, "two-camera matcher: %d keypoints > %d", nT, kTcMaxKps);
    const size_t lds = (((size_t)2 * kTcCells * 4 + 15) & ~(size_t)15) + (size_t)nT * 16;
    int rc;
    if ((rc = lds_optin(c, kOptTwocam + kind, kind ? (const void*)twocam_walk_kernel<1> : (const void*)twocam_walk_kernel<0>, 160 * 1024 - 2048))) return rc;
    ProfScope ps(c, kind ? "twocam_last" : "twocam_map");
    if (kind) twocam_walk_kernel<1><<<1, 256, lds, c->stream>>>(A);
    else twocam_walk_kernel<0><<<1, 256, lds, c->stream>>>(A);
    EORB_LAUNCH_CHECK(c, "twocam_walk_kernel");
    return EORB_OK;
}

}  // namespace eorb
