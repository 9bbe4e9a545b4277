// twoview.hip -- TwoViewReconstruction on gfx950: FindHomography + FindFundamental (src/TwoViewReconstruction.cc:264-363) over the
// caller's RANSAC sets, and CheckRT (:1242-1352) for Kp pose hypotheses.  The OpenCV 3.4.1 scalar paths they reach are restated in the
// fixed operation order of tests/twoview_ref/twoview_ref.c (-ffp-contract=off; DESIGN.md section 2 lists every choice).
//
// eorb_two_view_ransac is four launches:
//   tv_normalize_kernel  one wavefront per image: Normalize's float sums over all keys in index order, T1, T2, T2.inv(), T2.t()
//   tv_hyp_kernel        one lane per hypothesis (iters homographies, then iters fundamentals): the 16x9 / 8x9 + 3x3 Jacobi SVDs, whose
//                        rotation order is serial, with the lane's matrices in LDS columns; H21i, H12i / F21i
//   tv_score_kernel      one wavefront per hypothesis: the chi-square terms of 64 matches at a time, then the score's float add chain in
//                        match order; vbCurrentInliers
//   tv_finish_kernel     the first-wins scan over the iterations' scores and the copy of the winners
// eorb_two_view_check_rt is two: tv_check_rt_kernel (one thread per (pose, match)) and tv_select_kernel (one workgroup per pose: nGood
// and the element of the sorted vCosParallax by a radix select, no sort).
// eorb_two_view_reconstruct is those six with two more on one stream and no host step between them:
//   tv_decide_kernel     after tv_finish_kernel: the SH+SF == 0 exit, RH and the H/F choice, the inlier count, DecomposeE or the Faugeras
//                        decomposition on one lane (twoview_core.h), the 4 or 8 eorb_tvr_pose records and their count in device memory
//   tv_resolve_kernel    after tv_select_kernel: the parallax (fdlibm acos), the decision rule of the form, the one or two result slots
// CheckRT is launched for 8 poses and reads the count and the chosen flags from device memory.
#include "twoview.h"
#include "kb8_dev.h"

namespace eorb {

constexpr int kTvLanes = 64;            // hypotheses per workgroup of tv_hyp_kernel (one wavefront)
constexpr int kTvHypLds = (9 * 16 + 9 * 9) * 4 + 9 * 8;      // bytes per lane: At 9x16 and Vt 9x9 in float, W[9] in double (the 16x9 system)

__device__ __forceinline__ float tv_lane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// Mat::inv() 3x3: cv::invert DECOMP_LU, n == 3 closed form; determinant and cofactors in double, d = 1./d, d == 0 -> zeros
__device__ __forceinline__ void tv_inv33(const float* S, float* D)
{
#define Sf(r, c) S[3 * (r) + (c)]
    double d = Sf(0, 0) * ((double)Sf(1, 1) * Sf(2, 2) - (double)Sf(1, 2) * Sf(2, 1)) -
               Sf(0, 1) * ((double)Sf(1, 0) * Sf(2, 2) - (double)Sf(1, 2) * Sf(2, 0)) +
               Sf(0, 2) * ((double)Sf(1, 0) * Sf(2, 1) - (double)Sf(1, 1) * Sf(2, 0));
    if (d != 0.) {
        d = 1. / d;
        D[0] = (float)(((double)Sf(1, 1) * Sf(2, 2) - (double)Sf(1, 2) * Sf(2, 1)) * d);
        D[1] = (float)(((double)Sf(0, 2) * Sf(2, 1) - (double)Sf(0, 1) * Sf(2, 2)) * d);
        D[2] = (float)(((double)Sf(0, 1) * Sf(1, 2) - (double)Sf(0, 2) * Sf(1, 1)) * d);
        D[3] = (float)(((double)Sf(1, 2) * Sf(2, 0) - (double)Sf(1, 0) * Sf(2, 2)) * d);
        D[4] = (float)(((double)Sf(0, 0) * Sf(2, 2) - (double)Sf(0, 2) * Sf(2, 0)) * d);
        D[5] = (float)(((double)Sf(0, 2) * Sf(1, 0) - (double)Sf(0, 0) * Sf(1, 2)) * d);
        D[6] = (float)(((double)Sf(1, 0) * Sf(2, 1) - (double)Sf(1, 1) * Sf(2, 0)) * d);
        D[7] = (float)(((double)Sf(0, 1) * Sf(2, 0) - (double)Sf(0, 0) * Sf(2, 1)) * d);
        D[8] = (float)(((double)Sf(0, 0) * Sf(1, 1) - (double)Sf(0, 1) * Sf(1, 0)) * d);
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++) D[i] = 0.f;
    }
#undef Sf
}

// Normalize (:1193-1239) of both images; the sums run over every key in index order: 64 keys are loaded at a time, then added lane by lane
__global__ __launch_bounds__(128) void tv_normalize_kernel(TvRansacArgs a)
{
    const int lane = threadIdx.x & 63, img = threadIdx.x >> 6;
    const float2* pts = img ? a.pts2 : a.pts1;
    float2* pn = img ? a.pn2 : a.pn1;
    const int n = img ? a.n2 : a.n1;
    float meanX = 0, meanY = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane, cnt = min(64, n - base);
        const float2 p = i < n ? pts[i] : make_float2(0.f, 0.f);
        for (int l = 0; l < cnt; l++) { meanX += tv_lane(p.x, l); meanY += tv_lane(p.y, l); }
    }
    meanX = meanX / n; meanY = meanY / n;
    float meanDevX = 0, meanDevY = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane, cnt = min(64, n - base);
        const float2 p = i < n ? pts[i] : make_float2(0.f, 0.f);
        const float dx = fabsf(p.x - meanX), dy = fabsf(p.y - meanY);
        for (int l = 0; l < cnt; l++) { meanDevX += tv_lane(dx, l); meanDevY += tv_lane(dy, l); }
    }
    meanDevX = meanDevX / n; meanDevY = meanDevY / n;
    const float sX = 1.0f / meanDevX, sY = 1.0f / meanDevY;
    for (int i = lane; i < n; i += 64) {
        const float2 p = pts[i];
        const float x = p.x - meanX, y = p.y - meanY;
        pn[i] = make_float2(x * sX, y * sY);
    }
    if (lane == 0) {
        const float T[9] = {sX, 0.f, -meanX * sX, 0.f, sY, -meanY * sY, 0.f, 0.f, 1.f};
        float* o = a.hdr + 9 * img;
#pragma unroll
        for (int k = 0; k < 9; k++) o[k] = T[k];
        if (img) {
            float Ti[9];
            tv_inv33(T, Ti);
#pragma unroll
            for (int k = 0; k < 9; k++) { a.hdr[18 + k] = Ti[k]; a.hdr[27 + k] = T[3 * (k % 3) + k / 3]; }
        }
    }
}

// ---- JacobiSVDImpl_<float> (OpenCV 3.4.1 lapack.cpp) on one lane's matrices, stored as LDS columns: element e of a lane sits at [e * 64 + lane]
#define TV_A(i, k) At[((i) * M + (k)) * kTvLanes]
#define TV_V(i, k) Vt[((i) * N + (k)) * kTvLanes]
#define TV_W(i) W[(i) * kTvLanes]
// At: N1 rows of length M (rows >= N zero on entry); Vt: N x N (WANT_V); W: N doubles.  COMPLETE: the 1/W normalisation of At's rows and
// the cv::RNG completion of rows with W <= FLT_MIN (needed where At is an output: u, or vt of a wide matrix).
template <int M, int N, int N1, bool WANT_V, bool COMPLETE>
__device__ void tv_jacobi(float* At, float* Vt, double* W)
{
    const float eps = 1.19209290e-07f * 2;
    const double minval = 1.17549435e-38f;
    const int max_iter = M > 30 ? M : 30;
    for (int i = 0; i < N; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) { const float t = TV_A(i, k); sd += (double)t * t; }
        TV_W(i) = sd;
        if (WANT_V)
            for (int k = 0; k < N; k++) TV_V(i, k) = (k == i) ? 1.f : 0.f;
    }
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < N - 1; i++)
            for (int j = i + 1; j < N; j++) {
                float Ai[M], Aj[M];
                double a = TV_W(i), p = 0, b = TV_W(j);
#pragma unroll
                for (int k = 0; k < M; k++) { Ai[k] = TV_A(i, k); Aj[k] = TV_A(j, k); }
#pragma unroll
                for (int k = 0; k < M; k++) p += (double)Ai[k] * Aj[k];
                if (fabs(p) <= (double)eps * sqrt((double)a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = kt_hypot(p, beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
#pragma unroll
                for (int k = 0; k < M; k++) {
                    const float t0 = c * Ai[k] + s * Aj[k];
                    const float t1 = -s * Ai[k] + c * Aj[k];
                    TV_A(i, k) = t0; TV_A(j, k) = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                TV_W(i) = a; TV_W(j) = b;
                changed = true;
                if (WANT_V) {
#pragma unroll
                    for (int k = 0; k < N; k++) {
                        const float vi = TV_V(i, k), vj = TV_V(j, k);
                        const float t0 = c * vi + s * vj;
                        const float t1 = -s * vi + c * vj;
                        TV_V(i, k) = t0; TV_V(j, k) = t1;
                    }
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < N; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; k++) { const float t = TV_A(i, k); sd += (double)t * t; }
        TV_W(i) = sqrt(sd);
    }
    for (int i = 0; i < N - 1; i++) {
        int j = i;
        for (int k = i + 1; k < N; k++) if (TV_W(j) < TV_W(k)) j = k;
        if (i != j) {
            const double tw = TV_W(i); TV_W(i) = TV_W(j); TV_W(j) = tw;
            for (int k = 0; k < M; k++) { const float t = TV_A(i, k); TV_A(i, k) = TV_A(j, k); TV_A(j, k) = t; }
            if (WANT_V)
                for (int k = 0; k < N; k++) { const float t = TV_V(i, k); TV_V(i, k) = TV_V(j, k); TV_V(j, k) = t; }
        }
    }
    if (!COMPLETE) return;
    uint64_t rng = 0x12345678;                         // cv::RNG rng(0x12345678), one per SVD call
    for (int i = 0; i < N1; i++) {
        double sd = i < N ? TV_W(i) : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const float val0 = (float)(1. / M);
            for (int k = 0; k < M; k++) {
                rng = (uint64_t)(unsigned)rng * 4164903690U + (unsigned)(rng >> 32);
                TV_A(i, k) = ((unsigned)rng & 256) != 0 ? val0 : -val0;
            }
            for (int pass = 0; pass < 2; pass++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < M; k++) sd += TV_A(i, k) * TV_A(j, k);      // a float product, summed in double
                    float asum = 0;
                    for (int k = 0; k < M; k++) {
                        const float t = (float)(TV_A(i, k) - sd * TV_A(j, k));
                        TV_A(i, k) = t;
                        asum += fabsf(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < M; k++) TV_A(i, k) *= asum;
                }
            sd = 0;
            for (int k = 0; k < M; k++) { const float t = TV_A(i, k); sd += (double)t * t; }
            sd = sqrt(sd);
        }
        const float s = (float)(sd > minval ? 1 / sd : 0.);
        for (int k = 0; k < M; k++) TV_A(i, k) *= s;
    }
}

// workgroups [0, hb) solve the homographies, [hb, 2 hb) the fundamentals; hb = ceil(iters / 64)
__global__ __launch_bounds__(kTvLanes) void tv_hyp_kernel(TvRansacArgs a, int hb)
{
    __shared__ double smem[kTvHypLds * kTvLanes / 8];
    const int lane = threadIdx.x;
    const bool isF = (int)blockIdx.x >= hb;
    const int it = ((int)blockIdx.x - (isF ? hb : 0)) * kTvLanes + lane;
    if (it >= a.iters) return;                         // (no barrier below: every lane works on its own LDS column)
    float p1[16], p2[16];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int idx = a.sets[8 * it + j];
        const float2 q1 = a.pn1[a.match12[2 * idx]], q2 = a.pn2[a.match12[2 * idx + 1]];
        p1[2 * j] = q1.x; p1[2 * j + 1] = q1.y; p2[2 * j] = q2.x; p2[2 * j + 1] = q2.y;
    }
    float T1[9], X21[9], tmp[9], Xn[9];
#pragma unroll
    for (int k = 0; k < 9; k++) T1[k] = a.hdr[k];
    float* out = a.hyp + (size_t)((isF ? a.iters : 0) + it) * kTvHypFloats;
    if (!isF) {
        // ComputeH21 (:366-406): At = A^T, 9 rows of 16; vt.row(8) needs the rotations and the sort only
        constexpr int M = 16, N = 9;
        double* W = smem + lane;
        float* At = (float*)(smem + N * kTvLanes) + lane;
        float* Vt = At + N * M * kTvLanes;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
            const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
            const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
#pragma unroll
            for (int k = 0; k < 9; k++) { TV_A(k, 2 * i) = r0[k]; TV_A(k, 2 * i + 1) = r1[k]; }
        }
        tv_jacobi<M, N, N, true, false>(At, Vt, W);
#pragma unroll
        for (int k = 0; k < 9; k++) Xn[k] = TV_V(8, k);
        float T2inv[9], X12[9];
#pragma unroll
        for (int k = 0; k < 9; k++) T2inv[k] = a.hdr[18 + k];
        cv_gemm33(T2inv, Xn, tmp); cv_gemm33(tmp, T1, X21);      // H21i = T2inv*Hn*T1
        tv_inv33(X21, X12);                                      // H12i = H21i.inv()
#pragma unroll
        for (int k = 0; k < 9; k++) { out[k] = X21[k]; out[9 + k] = X12[k]; }
        return;
    }
    float Fpre[9];
    {
        // ComputeF21 (:408-443), the 8x9 system: at = true, At = A with a zero ninth row; vt = At after the completion stage
        constexpr int M = 9, N = 8;
        double* W = smem + lane;
        float* At = (float*)(smem + N * kTvLanes) + lane;
        float* Vt = nullptr;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
            const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
#pragma unroll
            for (int k = 0; k < 9; k++) TV_A(i, k) = r[k];
        }
#pragma unroll
        for (int k = 0; k < 9; k++) TV_A(8, k) = 0.f;
        tv_jacobi<M, N, 9, false, true>(At, Vt, W);
#pragma unroll
        for (int k = 0; k < 9; k++) Fpre[k] = TV_A(8, k);
    }
    {
        // SVDecomp(Fpre): At = Fpre^T, u = At^T after the normalisation, w = (float)W with w[2] = 0, then u*diag(w)*vt as two products
        constexpr int M = 3, N = 3;
        double* W = smem + lane;
        float* At = (float*)(smem + N * kTvLanes) + lane;
        float* Vt = At + N * M * kTvLanes;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) TV_A(i, k) = Fpre[3 * k + i];
        tv_jacobi<M, N, N, true, true>(At, Vt, W);
        float u[9], vt[9], d[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) { u[3 * i + k] = TV_A(k, i); vt[3 * i + k] = TV_V(i, k); }
        d[0] = (float)TV_W(0); d[4] = (float)TV_W(1); d[8] = 0.f;
        cv_gemm33(u, d, tmp); cv_gemm33(tmp, vt, Xn);
    }
    float T2t[9];
#pragma unroll
    for (int k = 0; k < 9; k++) T2t[k] = a.hdr[27 + k];
    cv_gemm33(T2t, Xn, tmp); cv_gemm33(tmp, T1, X21);            // F21i = T2t*Fn*T1
#pragma unroll
    for (int k = 0; k < 9; k++) { out[k] = X21[k]; out[9 + k] = 0.f; }
}

// cv::SVD::compute of a 3x3 (with or without FULL_UV: one computation on a square matrix) for one lane of a workgroup, in an LDS
// column as SVDecomp(Fpre) above: At = A^T, u = At^T after the normalisation, w = (float)W
__device__ __noinline__ void tv_svd33(const float* A, float* w, float* u, float* vt)
{
    constexpr int M = 3, N = 3;
    __shared__ double smem[(3 * 8 + 2 * 9 * 4) * kTvLanes / 8];      // tv_jacobi's column layout; the one calling lane uses column 0
    double* W = smem;
    float* At = (float*)(smem + N * kTvLanes);
    float* Vt = At + N * M * kTvLanes;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) TV_A(i, k) = A[3 * k + i];
    tv_jacobi<M, N, N, true, true>(At, Vt, W);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int k = 0; k < 3; k++) { u[3 * i + k] = TV_A(k, i); vt[3 * i + k] = TV_V(i, k); }
        w[i] = (float)TV_W(i);
    }
}
#undef TV_A
#undef TV_V
#undef TV_W

// CheckHomography (:445-528) / CheckFundamental (:530-608) of hypothesis blockIdx.x: each lane computes the two terms of one match, then
// every lane adds the terms of the 64 matches in match order -- that order is the contract
__global__ __launch_bounds__(64) void tv_score_kernel(TvRansacArgs a)
{
    const int lane = threadIdx.x, hyp = blockIdx.x;
    const bool isF = hyp >= a.iters;
    const float* X = a.hyp + (size_t)hyp * kTvHypFloats;
    float m[18];
#pragma unroll
    for (int k = 0; k < 18; k++) m[k] = X[k];
    const float th = isF ? a.th_f : a.th_score, thScore = a.th_score;
    const float invSigmaSquare = 1.0f / (a.sigma * a.sigma);
    uint8_t* inl = a.inl + (size_t)hyp * a.N;
    float score = 0;
    for (int base = 0; base < a.N; base += 64) {
        const int i = base + lane, cnt = min(64, a.N - base);
        float t1 = 0.f, t2 = 0.f;
        bool add1 = false, add2 = false;
        if (i < a.N) {
            const float2 k1 = a.pts1[a.match12[2 * i]], k2 = a.pts2[a.match12[2 * i + 1]];
            const float u1 = k1.x, v1 = k1.y, u2 = k2.x, v2 = k2.y;
            float chiSquare1, chiSquare2;
            if (!isF) {
                const float w2in1inv = 1.0f / (m[15] * u2 + m[16] * v2 + m[17]);
                const float u2in1 = (m[9] * u2 + m[10] * v2 + m[11]) * w2in1inv;
                const float v2in1 = (m[12] * u2 + m[13] * v2 + m[14]) * w2in1inv;
                const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
                chiSquare1 = squareDist1 * invSigmaSquare;
                const float w1in2inv = 1.0f / (m[6] * u1 + m[7] * v1 + m[8]);
                const float u1in2 = (m[0] * u1 + m[1] * v1 + m[2]) * w1in2inv;
                const float v1in2 = (m[3] * u1 + m[4] * v1 + m[5]) * w1in2inv;
                const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
                chiSquare2 = squareDist2 * invSigmaSquare;
            } else {
                const float a2 = m[0] * u1 + m[1] * v1 + m[2];
                const float b2 = m[3] * u1 + m[4] * v1 + m[5];
                const float c2 = m[6] * u1 + m[7] * v1 + m[8];
                const float num2 = a2 * u2 + b2 * v2 + c2;
                const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
                chiSquare1 = squareDist1 * invSigmaSquare;
                const float a1 = m[0] * u2 + m[3] * v2 + m[6];
                const float b1 = m[1] * u2 + m[4] * v2 + m[7];
                const float c1 = m[2] * u2 + m[5] * v2 + m[8];
                const float num1 = a1 * u1 + b1 * v1 + c1;
                const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
                chiSquare2 = squareDist2 * invSigmaSquare;
            }
            add1 = !(chiSquare1 > th); add2 = !(chiSquare2 > th);      // (a NaN chi-square is added: the score becomes NaN)
            t1 = thScore - chiSquare1; t2 = thScore - chiSquare2;
            inl[i] = (add1 && add2) ? 1 : 0;
        }
        const uint64_t m1 = __ballot(add1), m2 = __ballot(add2);
        for (int l = 0; l < cnt; l++) {
            if ((m1 >> l) & 1) score += tv_lane(t1, l);
            if ((m2 >> l) & 1) score += tv_lane(t2, l);
        }
    }
    if (lane == 0) (isF ? a.it_score_f : a.it_score_h)[hyp - (isF ? a.iters : 0)] = score;
    if (lane < 9) (isF ? a.it_F : a.it_H)[(size_t)(hyp - (isF ? a.iters : 0)) * 9 + lane] = X[lane];
}

// :305 / :356 "if(currentScore>score)" from score = 0.0: the first iteration above the running best wins, a NaN never does
__global__ __launch_bounds__(256) void tv_finish_kernel(TvRansacArgs a)
{
    __shared__ int s_best[2];
    __shared__ float s_score[2];
    const int tid = threadIdx.x;
    if (tid == 0 || tid == 64) {
        const int f = tid >> 6;
        const float* sc = f ? a.it_score_f : a.it_score_h;
        float score = 0.0f; int best = -1;
        for (int it = 0; it < a.iters; it++) { const float cs = sc[it]; if (cs > score) { score = cs; best = it; } }
        s_best[f] = best; s_score[f] = score;
    }
    __syncthreads();
    for (int f = 0; f < 2; f++) {
        const int best = s_best[f];
        uint8_t* dst = f ? a.inliers_f : a.inliers_h;
        const uint8_t* src = a.inl + (size_t)(f * a.iters + (best < 0 ? 0 : best)) * a.N;
        for (int i = tid; i < a.N; i += 256) dst[i] = best < 0 ? 0 : src[i];
        if (tid < 9) a.res[4 + 9 * f + tid] = best < 0 ? 0.f : a.hyp[(size_t)(f * a.iters + best) * kTvHypFloats + tid];
    }
    if (tid < 2) { a.res[tid] = s_score[tid]; ((int32_t*)a.res)[2 + tid] = s_best[tid]; }
}

int twoview_ransac_dev(eorb_ctx* c, const TvRansacArgs& a)
{
    const int hb = (a.iters + kTvLanes - 1) / kTvLanes;
    { ProfScope ps(c, "tv_normalize");
      tv_normalize_kernel<<<1, 128, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "tv_normalize_kernel"); }
    { ProfScope ps(c, "tv_hyp");
      tv_hyp_kernel<<<2 * hb, kTvLanes, 0, c->stream>>>(a, hb);
      EORB_LAUNCH_CHECK(c, "tv_hyp_kernel"); }
    { ProfScope ps(c, "tv_score");
      tv_score_kernel<<<2 * a.iters, 64, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "tv_score_kernel"); }
    { ProfScope ps(c, "tv_finish");
      tv_finish_kernel<<<1, 256, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "tv_finish_kernel"); }
    return EORB_OK;
}

// ---- CheckRT (:1242-1352) ----------------------------------------------------------------------------------------------------------------
// the ascending order of vCosParallax as an integer: -0 before +0, every NaN last
__device__ __forceinline__ uint32_t tv_cos_key(float f)
{
    if (f != f) return 0xffffffffu;
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void tv_check_rt_kernel(TvCheckRtArgs a)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    const int Kp = a.Kp_dev ? min(*a.Kp_dev, a.Kp) : a.Kp;      // (the launch is sized for a.Kp: workgroups past a device-side count leave)
    if (id >= (long long)Kp * a.N) return;
    const int h = (int)(id / a.N), i = (int)(id % a.N);
    float* cosv = a.cos_all + (size_t)h * a.N + i;
    *cosv = -2.f;
    if (!a.inliers[i]) return;
    const float* pose = a.poses + kTvPoseFloats * h;
    const float *R = pose, *t = pose + 9, *P2 = pose + 12, *O2 = pose + 24;
    const int i1 = a.match12[2 * i], i2 = a.match12[2 * i + 1];
    const float2 kp1 = a.pts1[i1], kp2 = a.pts2[i2];
    const float fx = a.K[0], fy = a.K[4], cx = a.K[2], cy = a.K[5];
    const float P1[12] = {a.K[0], a.K[1], a.K[2], 0.f, a.K[3], a.K[4], a.K[5], 0.f, a.K[6], a.K[7], a.K[8], 0.f};
    // Triangulate (:1177-1191)
    float A[16], v3[4], P2r[12];
#pragma unroll
    for (int k = 0; k < 12; k++) P2r[k] = P2[k];
    cv_a_row(kp1.x, P1 + 8, P1 + 0, A + 0);
    cv_a_row(kp1.y, P1 + 8, P1 + 4, A + 4);
    cv_a_row(kp2.x, P2r + 8, P2r + 0, A + 8);
    cv_a_row(kp2.y, P2r + 8, P2r + 4, A + 12);
    cv_svd4_vt3(A, v3);
    const float sc = (float)(1. / (double)v3[3]);
    const float p3dC1[3] = {v3[0] * sc + 0.0f, v3[1] * sc + 0.0f, v3[2] * sc + 0.0f};
    if (!isfinite(p3dC1[0]) || !isfinite(p3dC1[1]) || !isfinite(p3dC1[2])) return;      // (:1288 vbGood = false: it is)
    float normal1[3], normal2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { normal1[k] = p3dC1[k] - 0.f; normal2[k] = p3dC1[k] - O2[k]; }
    const float dist1 = (float)cv_norm3(normal1), dist2 = (float)cv_norm3(normal2);
    const float cosParallax = (float)(cv_dot3(normal1, normal2) / (double)(dist1 * dist2));
    const float thMinParallex = a.min_parallax_crt;
    if (p3dC1[2] <= 0 && cosParallax < thMinParallex) return;
    float Rr[9], tr[3], p3dC2[3];
#pragma unroll
    for (int k = 0; k < 9; k++) Rr[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) tr[k] = t[k];
    cv_gemm3x1(Rr, p3dC1, tr, 1.0, p3dC2);
    if (p3dC2[2] <= 0 && cosParallax < thMinParallex) return;
    const float invZ1 = 1.0f / p3dC1[2];
    const float im1x = fx * p3dC1[0] * invZ1 + cx, im1y = fy * p3dC1[1] * invZ1 + cy;
    const float squareError1 = (im1x - kp1.x) * (im1x - kp1.x) + (im1y - kp1.y) * (im1y - kp1.y);
    if (squareError1 > a.th2) return;
    const float invZ2 = 1.0f / p3dC2[2];
    const float im2x = fx * p3dC2[0] * invZ2 + cx, im2y = fy * p3dC2[1] * invZ2 + cy;
    const float squareError2 = (im2x - kp2.x) * (im2x - kp2.x) + (im2y - kp2.y) * (im2y - kp2.y);
    if (squareError2 > a.th2) return;
    *cosv = cosParallax;
    float* o = a.p3d + ((size_t)h * a.n1 + i1) * 3;      // (the entry point refuses two matches with the same first index)
    o[0] = p3dC1[0]; o[1] = p3dC1[1]; o[2] = p3dC1[2];
    if (cosParallax < thMinParallex) a.good[(size_t)h * a.n1 + i1] = 1;
}

// nGood and vCosParallax[min(min_triangulated, size - 1)] of the ascending sort, for pose blockIdx.x: a most-significant-byte-first radix
// select over the counted matches' keys
__global__ __launch_bounds__(256) void tv_select_kernel(TvCheckRtArgs a)
{
    __shared__ int hist[256];
    __shared__ uint32_t s_prefix;
    __shared__ int s_k, s_total;
    const int tid = threadIdx.x, h = blockIdx.x;
    if (a.Kp_dev && h >= *a.Kp_dev) return;            // (uniform over the workgroup, before any barrier)
    const float* cosv = a.cos_all + (size_t)h * a.N;
    uint32_t prefix = 0, mask = 0;
    int k = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < a.N; i += 256) {
            const float cv = cosv[i];
            if (cv == -2.f) continue;
            const uint32_t key = tv_cos_key(cv);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid == 0) {
            if (shift == 24) {
                int total = 0;
                for (int b = 0; b < 256; b++) total += hist[b];
                s_total = total;
                k = a.min_triangulated < total - 1 ? a.min_triangulated : total - 1;
            } else k = s_k;
            int cum = 0, b = 0;
            if (s_total > 0) for (; b < 255; b++) { if (cum + hist[b] > k) break; cum += hist[b]; }
            s_k = k - cum;
            s_prefix = prefix | ((uint32_t)b << shift);
        }
        __syncthreads();
        prefix = s_prefix; mask |= 255u << shift;
        if (s_total <= 0) break;
    }
    if (tid == 0) {
        a.n_good[h] = s_total;
        const uint32_t kk = prefix;
        const uint32_t u = kk == 0xffffffffu ? 0x7fc00000u : (kk & 0x80000000u) ? (kk & 0x7fffffffu) : ~kk;
        a.cos_sel[h] = s_total > 0 ? __uint_as_float(u) : 0.f;
    }
}

int twoview_check_rt_dev(eorb_ctx* c, const TvCheckRtArgs& a)
{
    const long long total = (long long)a.Kp * a.N;
    { ProfScope ps(c, "tv_check_rt");
      tv_check_rt_kernel<<<(unsigned)((total + 255) / 256), 256, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "tv_check_rt_kernel"); }
    { ProfScope ps(c, "tv_select");
      tv_select_kernel<<<a.Kp, 256, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "tv_select_kernel"); }
    return EORB_OK;
}

// ---- Reconstruct (:67-262): what stands between and after the two stages ----------------------------------------------------------------
#define TVC_FN __device__ static inline
#define TVC_HI(x) ((int32_t)__double2hiint(x))
#define TVC_LO(x) ((uint32_t)__double2loint(x))
#define TVC_MK(hi, lo) __hiloint2double((int)(hi), (int)(lo))
#define TVC_SVD33(A, w, u, vt) tv_svd33((A), (w), (u), (vt))
#define TVC_UNROLL _Pragma("unroll")
#include "twoview_core.h"

// :139-157 / :236-261 and the heads of ReconstructF / ReconstructH: the SH+SF == 0 exit, RH and the H/F choice; every lane copies the
// chosen model's flags and the wavefronts count them (integers: no order); lane 0 then forms the 4 or 8 hypotheses with their P2 and O2
__global__ __launch_bounds__(256) void tv_decide_kernel(TvReconArgs a)
{
    __shared__ int s_stage, s_isH, s_N;
    const int tid = threadIdx.x;
    eorb_tvr_recon_result* r = a.res;
    if (tid == 0) {
        const float SH = a.rres[0], SF = a.rres[1];
        r->SH = SH; r->SF = SF;
        r->best_it_h = ((const int32_t*)a.rres)[2]; r->best_it_f = ((const int32_t*)a.rres)[3];
#pragma unroll
        for (int k = 0; k < 9; k++) { r->H21[k] = a.rres[4 + k]; r->F21[k] = a.rres[13 + k]; }
        int stage = 2, isH = 0;
        if (SH + SF == 0.f) stage = 0;
        else {
            const float RH = SH / (SH + SF);
            r->RH = RH;
            isH = RH > a.p.th_hf_ratio;
        }
        r->is_homography = isH;
        s_stage = stage; s_isH = isH; s_N = 0;
    }
    __syncthreads();
    int stage = s_stage;
    const int isH = s_isH;
    const uint8_t* src = (stage == 0 || !isH) ? a.inliers_f : a.inliers_h;
    int cnt = 0;
    for (int base = 0; base < a.N; base += 256) {
        const int i = base + tid;
        const uint8_t f = i < a.N ? src[i] : 0;
        if (i < a.N) {
            a.sel_inl[i] = f;
            if (a.p.form == EORB_TVR_FORM_INFO) a.trans_inl[i] = f;
        }
        cnt += __popcll(__ballot(f != 0));
    }
    if ((tid & 63) == 0 && stage != 0) atomicAdd(&s_N, cnt);
    __syncthreads();
    if (tid != 0) return;
    int n_hyp = 0;
    if (stage != 0) {
        r->n_inliers = s_N;
        if (!isH) { tvc_hypotheses_f(a.K, r->F21, a.poses); n_hyp = 4; }
        else if (tvc_hypotheses_h(a.K, r->H21, a.p.th_rd_homo, a.poses)) n_hyp = 8;
        else stage = 1;
    }
    r->stage = stage; r->n_hyp = n_hyp;
    *a.n_hyp = n_hyp;
}

// after CheckRT: the parallax of every hypothesis, the decision rule of the form, and the copy of the one or two chosen hypotheses into
// the result slots (R, t by lane 0; the n1 rows of vP3D and vbTriangulated by every lane)
__global__ __launch_bounds__(256) void tv_resolve_kernel(TvReconArgs a)
{
    __shared__ int s_slot[2];
    const int tid = threadIdx.x;
    eorb_tvr_recon_result* r = a.res;
    if (tid == 0) {
        s_slot[0] = s_slot[1] = -1;
        r->hyp_best = r->hyp_second = -1;
        if (r->stage == 2) {
            int32_t ng[8]; float par[8];
#pragma unroll
            for (int h = 0; h < 8; h++) {
                ng[h] = h < r->n_hyp ? a.n_good[h] : 0;
                par[h] = h < r->n_hyp ? tvc_parallax(ng[h], a.cos_sel[h]) : 0.f;
            }
            tvc_resolve(&a.p, r->n_inliers, ng, par, r);
            s_slot[0] = r->hyp_best; s_slot[1] = r->hyp_second;
            for (int s = 0; s < 2; s++) {
                const int h = s_slot[s];
                if (h < 0) continue;
                const float* pose = a.poses + kTvPoseFloats * h;
                for (int k = 0; k < 9; k++) a.R21[9 * s + k] = pose[k];
                for (int k = 0; k < 3; k++) a.t21[3 * s + k] = pose[9 + k];
            }
        }
    }
    __syncthreads();
    for (int s = 0; s < 2; s++) {
        const int h = s_slot[s];
        if (h < 0) continue;
        const uint8_t* g = a.good8 + (size_t)h * a.n1;
        const float* p = a.p3d8 + (size_t)h * a.n1 * 3;
        for (int i = tid; i < a.n1; i += 256) a.tri[(size_t)s * a.n1 + i] = g[i];
        for (int i = tid; i < 3 * a.n1; i += 256) a.p3d[(size_t)s * a.n1 * 3 + i] = p[i];
    }
}

int twoview_reconstruct_dev(eorb_ctx* c, const TvRansacArgs& R, const TvReconArgs& A, const TvCheckRtArgs& T)
{
    int rc;
    if ((rc = twoview_ransac_dev(c, R))) return rc;
    { ProfScope ps(c, "tv_decide");
      tv_decide_kernel<<<1, 256, 0, c->stream>>>(A);
      EORB_LAUNCH_CHECK(c, "tv_decide_kernel"); }
    if ((rc = twoview_check_rt_dev(c, T))) return rc;
    { ProfScope ps(c, "tv_resolve");
      tv_resolve_kernel<<<1, 256, 0, c->stream>>>(A);
      EORB_LAUNCH_CHECK(c, "tv_resolve_kernel"); }
    return EORB_OK;
}

}  // namespace eorb
