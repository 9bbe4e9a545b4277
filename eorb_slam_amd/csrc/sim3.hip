// sim3.hip -- Sim3Solver on gfx950: Horn's closed form (ComputeSim3, src/Sim3Solver.cc:316-427) for every RANSAC set of K independent
// problems, CheckInliers (:430-454) for every hypothesis, and the result the loop of LoopClosing.cc:698-701 ends with.  The OpenCV 3.4.1
// scalar paths they reach are restated in the fixed operation order of tests/sim3_ref/sim3_ref.c (-ffp-contract=off; DESIGN.md section 2
// lists every choice).
//
// eorb_sim3_ransac is four launches:
//   s3_prepare_kernel  one thread per correspondence: mvX3Dc1 / mvX3Dc2 (:107, :110), FromCameraToImage (:492-506), the truncated bounds
//   s3_hyp_kernel      one lane per (problem, iteration): ComputeSim3; the 4x4 Jacobi eigen-solver picks its pivots from the data, so the
//                      lane's A, V, W, indR, indC sit in LDS columns; T12i, T21i, R12i, t12i, s12i
//   s3_inlier_kernel   one wavefront per hypothesis: Project (:472-490) both ways for 64 correspondences at a time, the two comparisons,
//                      the count by ballot
//   s3_finish_kernel   one workgroup per problem: the result rule over the counts, the winner's copy, its flags computed again
#include "sim3.h"
#include <limits.h>

namespace eorb {

constexpr int kS3Lanes = 64;            // hypotheses per workgroup of s3_hyp_kernel (one wavefront)
constexpr int kS3HypWords = 16 + 16 + 4 + 4 + 4;      // per lane: A, V, W in float, indR, indC

// Mat::convertTo(dst, CV_32F, alpha): a copy when |alpha - 1| < DBL_EPSILON (noScale), else cvtScale32f: src*(float)alpha + 0.0f
template <int N>
__device__ __forceinline__ void s3_scale(const float* src, double alpha, float* dst)
{
    const bool copy = fabs(alpha - 1) < 2.2204460492503131e-16;
    const float a = (float)alpha;
#pragma unroll
    for (int i = 0; i < N; i++) dst[i] = copy ? src[i] : src[i] * a + 0.0f;
}
// the templated hypot of lapack.cpp, float
__device__ __forceinline__ float s3_hypotf(float a, float b)
{
    a = fabsf(a); b = fabsf(b);
    if (a > b) { b /= a; return a * sqrtf(1 + b * b); }
    if (b > 0) { a /= b; return b * sqrtf(1 + a * a); }
    return 0;
}

// ComputeCentroid (:305-314): reduceC_'s two accumulators give (p0 + p2) + p1; C/3 is a MatExpr scale by 1./3
__device__ __forceinline__ void s3_centroid(const float* P, float* Pr, float* C)
{
    float sum[3];
#pragma unroll
    for (int r = 0; r < 3; r++) sum[r] = (P[3 * r] + P[3 * r + 2]) + P[3 * r + 1];
    s3_scale<3>(sum, 1. / 3, C);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int i = 0; i < 3; i++) Pr[3 * r + i] = P[3 * r + i] - C[r];
}

// ---- JacobiImpl_<float> (OpenCV 3.4.1 lapack.cpp), n = 4, on one lane's LDS columns: element e of a lane sits at [e * 64 + lane]
#define S3_A(i, j) As[((i) * 4 + (j)) * kS3Lanes]
#define S3_V(i, j) Vs[((i) * 4 + (j)) * kS3Lanes]
#define S3_W(i) Ws[(i) * kS3Lanes]
#define S3_IR(i) Ir[(i) * kS3Lanes]
#define S3_IC(i) Ic[(i) * kS3Lanes]
#define S3_ROTATE(v0, v1) do { const float a0 = v0, b0 = v1; v0 = a0 * c - b0 * s; v1 = a0 * s + b0 * c; } while (0)
// the largest |element| right of the diagonal in row idx / above it in column idx
__device__ __forceinline__ void s3_jacobi_index(const float* As, int* Ir, int* Ic, int idx)
{
    if (idx < 3) {
        int m = idx + 1;
        float mv = fabsf(S3_A(idx, m));
        for (int i = idx + 2; i < 4; i++) { const float val = fabsf(S3_A(idx, i)); if (mv < val) { mv = val; m = i; } }
        S3_IR(idx) = m;
    }
    if (idx > 0) {
        int m = 0;
        float mv = fabsf(S3_A(0, idx));
        for (int i = 1; i < idx; i++) { const float val = fabsf(S3_A(i, idx)); if (mv < val) { mv = val; m = i; } }
        S3_IC(idx) = m;
    }
}
// A holds the symmetric matrix on entry; on return row 0 of V is the eigenvector of the largest eigenvalue
__device__ void s3_jacobi4(float* As, float* Vs, float* Ws, int* Ir, int* Ic)
{
    const float eps = 1.19209290e-07f;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) S3_V(i, j) = (i == j) ? 1.f : 0.f;
    for (int k = 0; k < 4; k++) {
        S3_W(k) = S3_A(k, k);
        s3_jacobi_index(As, Ir, Ic, k);
    }
    for (int iters = 0; iters < 4 * 4 * 30; iters++) {
        int k = 0;
        float mv = fabsf(S3_A(0, S3_IR(0)));
        for (int i = 1; i < 3; i++) { const float val = fabsf(S3_A(i, S3_IR(i))); if (mv < val) { mv = val; k = i; } }
        int l = S3_IR(k);
        for (int i = 1; i < 4; i++) { const int ci = S3_IC(i); const float val = fabsf(S3_A(ci, i)); if (mv < val) { mv = val; k = ci; l = i; } }
        const float p = S3_A(k, l);
        if (fabsf(p) <= eps) break;
        const float y = (float)((double)(S3_W(l) - S3_W(k)) * 0.5);
        float t = fabsf(y) + s3_hypotf(p, y);
        float s = s3_hypotf(p, t);
        const float c = t / s;
        s = p / s; t = (p / t) * p;
        if (y < 0) { s = -s; t = -t; }
        S3_A(k, l) = 0;
        S3_W(k) -= t;
        S3_W(l) += t;
        for (int i = 0; i < k; i++) S3_ROTATE(S3_A(i, k), S3_A(i, l));
        for (int i = k + 1; i < l; i++) S3_ROTATE(S3_A(k, i), S3_A(i, l));
        for (int i = l + 1; i < 4; i++) S3_ROTATE(S3_A(k, i), S3_A(l, i));
        for (int i = 0; i < 4; i++) S3_ROTATE(S3_V(k, i), S3_V(l, i));
        s3_jacobi_index(As, Ir, Ic, k);
        s3_jacobi_index(As, Ir, Ic, l);
    }
    for (int k = 0; k < 3; k++) {
        int m = k;
        for (int i = k + 1; i < 4; i++) if (S3_W(m) < S3_W(i)) m = i;
        if (k != m) {
            const float tw = S3_W(m); S3_W(m) = S3_W(k); S3_W(k) = tw;
            for (int i = 0; i < 4; i++) { const float tv = S3_V(m, i); S3_V(m, i) = S3_V(k, i); S3_V(k, i) = tv; }
        }
    }
}

__global__ __launch_bounds__(256) void s3_prepare_kernel(S3Args a)
{
    const S3Prob& P = a.prob[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.N) return;
    const size_t g = (size_t)P.corr_off + i;
    float Xw[3], Xc[3], u, v;
#pragma unroll
    for (int k = 0; k < 3; k++) Xw[k] = a.Xw1[3 * g + k];
    cv_gemm3x1(P.Rt1, Xw, P.Rt1 + 9, 1.0, Xc);                          // Rcw1*X3D1w + tcw1
    cam_project_f(P.cam1, Xc, u, v);
#pragma unroll
    for (int k = 0; k < 3; k++) a.X1[3 * g + k] = Xc[k];
    a.p1[g] = make_float2(u, v);
#pragma unroll
    for (int k = 0; k < 3; k++) Xw[k] = a.Xw2[3 * g + k];
    cv_gemm3x1(P.Rt2, Xw, P.Rt2 + 9, 1.0, Xc);
    cam_project_f(P.cam2, Xc, u, v);
#pragma unroll
    for (int k = 0; k < 3; k++) a.X2[3 * g + k] = Xc[k];
    a.p2[g] = make_float2(u, v);
    // mvnMaxError is a vector<size_t> (include/Sim3Solver.h:78-79): 9.210*sigma2 truncated, compared as a float (:446)
    a.b1[g] = (float)(unsigned long long)(9.210 * (double)a.sigma2_1[g]);
    a.b2[g] = (float)(unsigned long long)(9.210 * (double)a.sigma2_2[g]);
}

__global__ __launch_bounds__(kS3Lanes) void s3_hyp_kernel(S3Args a)
{
    __shared__ float smem[kS3HypWords * kS3Lanes];
    const S3Prob& P = a.prob[blockIdx.y];
    const int lane = threadIdx.x, it = blockIdx.x * kS3Lanes + lane;
    if (it >= P.iters || ransac_skips(P)) return;      // (no barrier below: every lane works on its own LDS column)
    const size_t h = (size_t)P.set_off + it;
    float P1[9], P2[9], Pr1[9], Pr2[9], O1[3], O2[3], M[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const size_t g = (size_t)P.corr_off + a.sets[3 * h + i];
#pragma unroll
        for (int r = 0; r < 3; r++) { P1[3 * r + i] = a.X1[3 * g + r]; P2[3 * r + i] = a.X2[3 * g + r]; }
    }
    s3_centroid(P1, Pr1, O1);
    s3_centroid(P2, Pr2, O2);
    // M = Pr2*Pr1.t(): GEMMSingleMul<float, double>, "A * Bt": products and sum in double
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s0 = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s0 += (double)Pr2[3 * i + k] * (double)Pr1[3 * j + k];
            M[3 * i + j] = (float)(s0 * 1.0);
        }
    float* As = smem + lane;
    float* Vs = As + 16 * kS3Lanes;
    float* Ws = Vs + 16 * kS3Lanes;
    int* Ir = (int*)(Ws + 4 * kS3Lanes);
    int* Ic = Ir + 4 * kS3Lanes;
    {
#define Mf(r, c) M[3 * (r) + (c)]
        const float N11 = Mf(0, 0) + Mf(1, 1) + Mf(2, 2), N12 = Mf(1, 2) - Mf(2, 1), N13 = Mf(2, 0) - Mf(0, 2), N14 = Mf(0, 1) - Mf(1, 0);
        const float N22 = Mf(0, 0) - Mf(1, 1) - Mf(2, 2), N23 = Mf(0, 1) + Mf(1, 0), N24 = Mf(2, 0) + Mf(0, 2);
        const float N33 = -Mf(0, 0) + Mf(1, 1) - Mf(2, 2), N34 = Mf(1, 2) + Mf(2, 1), N44 = -Mf(0, 0) - Mf(1, 1) + Mf(2, 2);
#undef Mf
        S3_A(0, 0) = N11; S3_A(0, 1) = N12; S3_A(0, 2) = N13; S3_A(0, 3) = N14;
        S3_A(1, 0) = N12; S3_A(1, 1) = N22; S3_A(1, 2) = N23; S3_A(1, 3) = N24;
        S3_A(2, 0) = N13; S3_A(2, 1) = N23; S3_A(2, 2) = N33; S3_A(2, 3) = N34;
        S3_A(3, 0) = N14; S3_A(3, 1) = N24; S3_A(3, 2) = N34; S3_A(3, 3) = N44;
    }
    s3_jacobi4(As, Vs, Ws, Ir, Ic);
    const float q0 = S3_V(0, 0);
    float vec[3] = {S3_V(0, 1), S3_V(0, 2), S3_V(0, 3)};
    const double nrm = cv_norm3(vec);
    const double ang = dev_datan2(nrm, (double)q0);
    s3_scale<3>(vec, (2 * ang) * (1. / nrm), vec);      // vec = 2*ang*vec/norm(vec): one MatExpr scale, applied as a float
    float R[9];
    {   // cv::Rodrigues, vector to matrix, double throughout
        double rx = vec[0], ry = vec[1], rz = vec[2];
        const double theta = sqrt(rx * rx + ry * ry + rz * rz);
        if (theta < 2.2204460492503131e-16) {
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.f : 0.f;
        } else {
            double sn, c;
            dev_dsincos_nan(theta, &sn, &c);
            const double c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
            rx *= itheta; ry *= itheta; rz *= itheta;
            const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
            const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = (float)((c * ((i % 4 == 0) ? 1. : 0.) + c1 * rrt[i]) + sn * r_x[i]);
        }
    }
    float P3[9], s12;
    cv_gemm33(R, Pr2, P3);
    if (!P.fix_scale) {
        // Mat::dot, len 9, unrolled by four; cv::pow(P3, 2) is a float product, den a double sum of floats
        double nom = 0;
        nom += (double)Pr1[0] * P3[0] + (double)Pr1[1] * P3[1] + (double)Pr1[2] * P3[2] + (double)Pr1[3] * P3[3];
        nom += (double)Pr1[4] * P3[4] + (double)Pr1[5] * P3[5] + (double)Pr1[6] * P3[6] + (double)Pr1[7] * P3[7];
        nom += (double)Pr1[8] * P3[8];
        nom = 0.0 + nom;
        double den = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) { const float q = P3[i] * P3[i]; den += q; }
        s12 = (float)(nom / den);
    } else s12 = 1.0f;
    float t[3], sR[9], Rt[9], sRinv[9], tinv[3];
    cv_gemm3x1(R, O2, O1, -(double)s12, t);             // mt12i = O1 - ms12i*mR12i*O2: one gemm(R, O2, -s, O1, 1)
    s3_scale<9>(R, (double)s12, sR);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rt[3 * i + j] = R[3 * j + i];
    {   // (1.0/ms12i)*mR12i.t(): MatOp_T with alpha; transpose, then convertTo when alpha != 1
        const double alpha = 1.0 / (double)s12;
        if (alpha != 1) s3_scale<9>(Rt, alpha, sRinv);
        else {
#pragma unroll
            for (int i = 0; i < 9; i++) sRinv[i] = Rt[i];
        }
    }
    cv_gemm3x1(sRinv, t, nullptr, -1.0, tinv);          // -sRinv*mt12i: gemm with alpha = -1
    float* T12 = a.it_T12 + 16 * h;
    float* T21 = a.it_T21 + 16 * h;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) { T12[4 * i + j] = sR[3 * i + j]; T21[4 * i + j] = sRinv[3 * i + j]; }
        T12[4 * i + 3] = t[i]; T21[4 * i + 3] = tinv[i];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) { T12[12 + j] = T21[12 + j] = (j == 3) ? 1.f : 0.f; }
    float* o = a.hyp + kS3HypFloats * h;
#pragma unroll
    for (int i = 0; i < 9; i++) o[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) o[9 + i] = t[i];
    o[12] = s12;
    a.it_scale[h] = s12;
}
#undef S3_A
#undef S3_V
#undef S3_W
#undef S3_IR
#undef S3_IC
#undef S3_ROTATE

// the 3x3 / 3x1 views of a 4x4 (:474-475)
struct S3Pose { float R[9], t[3]; };
__device__ __forceinline__ S3Pose s3_pose_of(const float* T)
{
    S3Pose p;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) p.R[3 * i + j] = T[4 * i + j];
        p.t[i] = T[4 * i + 3];
    }
    return p;
}
// Project (:472-490) both ways and the test of CheckInliers (:440-446) for correspondence g; Mat::dot of the 2x1 differences: the squares
// summed in double, narrowed to float.  A NaN error fails its comparison.
__device__ __forceinline__ bool s3_is_inlier(const S3Args& a, const S3Prob& P, const S3Pose& T12, const S3Pose& T21, size_t g)
{
    float X[3], q[3], u, v;
#pragma unroll
    for (int k = 0; k < 3; k++) X[k] = a.X2[3 * g + k];
    cv_gemm3x1(T12.R, X, T12.t, 1.0, q);
    cam_project_f(P.cam1, q, u, v);
    const float2 p1 = a.p1[g];
    const float d1x = p1.x - u, d1y = p1.y - v;
#pragma unroll
    for (int k = 0; k < 3; k++) X[k] = a.X1[3 * g + k];
    cv_gemm3x1(T21.R, X, T21.t, 1.0, q);
    cam_project_f(P.cam2, q, u, v);
    const float2 p2 = a.p2[g];
    const float d2x = u - p2.x, d2y = v - p2.y;
    double e = 0; e += (double)d1x * d1x; e += (double)d1y * d1y;
    const float err1 = (float)(0.0 + e);
    e = 0; e += (double)d2x * d2x; e += (double)d2y * d2y;
    const float err2 = (float)(0.0 + e);
    return err1 < a.b1[g] && err2 < a.b2[g];
}

__global__ __launch_bounds__(64) void s3_inlier_kernel(S3Args a)
{
    const S3Prob& P = a.prob[blockIdx.y];
    const int lane = threadIdx.x, it = blockIdx.x;
    if (it >= P.iters || ransac_skips(P)) return;
    const size_t h = (size_t)P.set_off + it;
    const S3Pose T12 = s3_pose_of(a.it_T12 + 16 * h), T21 = s3_pose_of(a.it_T21 + 16 * h);
    const int n = ransac_count_inliers(P.N, [&](int i) { return s3_is_inlier(a, P, T12, T21, (size_t)P.corr_off + i); });
    if (lane == 0) a.it_inliers[h] = n;
}

// the state after "while(!bConverge && !bNoMore) iterate(20, ...)" (:243-291): the first iteration whose count is > min_inliers, else the
// last iteration among those with the largest count (the running best starts at 0 and is replaced on >=)
__global__ __launch_bounds__(256) void s3_finish_kernel(S3Args a)
{
    __shared__ int s_first, s_key;
    const S3Prob& P = a.prob[blockIdx.x];
    const int tid = threadIdx.x;
    int32_t* res = a.res + kS3ResWords * blockIdx.x;
    if (ransac_skips(P)) { if (tid == 0) res[1] = -1; return; }      // (:228-232; everything else stays zero)
    if (tid == 0) { s_first = INT_MAX; s_key = -1; }
    __syncthreads();
    const int32_t* cnt = a.it_inliers + P.set_off;
    for (int it = tid; it < P.iters; it += 256) {
        const int n = cnt[it];
        if (n > P.min_inliers) atomicMin(&s_first, it);
        atomicMax(&s_key, n * 1024 + it);                                 // n <= 16 384, it < 1 024
    }
    __syncthreads();
    const bool conv = s_first != INT_MAX;
    const int best = conv ? s_first : (s_key & 1023);
    const size_t h = (size_t)P.set_off + best;
    if (tid == 0) { res[0] = conv; res[1] = best; res[2] = cnt[best]; res[3] = conv ? best + 1 : P.iters; }
    float* rf = (float*)res;
    if (tid < 16) rf[4 + tid] = a.it_T12[16 * h + tid];
    if (tid < kS3HypFloats) rf[20 + tid] = a.hyp[kS3HypFloats * h + tid];
    const S3Pose T12 = s3_pose_of(a.it_T12 + 16 * h), T21 = s3_pose_of(a.it_T21 + 16 * h);
    for (int i = tid; i < P.N; i += 256) {
        const size_t g = (size_t)P.corr_off + i;
        a.inliers[g] = s3_is_inlier(a, P, T12, T21, g) ? 1 : 0;
    }
}

int sim3_ransac_dev(eorb_ctx* c, const S3Args& a)
{
    { ProfScope ps(c, "s3_prepare");
      s3_prepare_kernel<<<dim3((a.max_N + 255) / 256, a.K), 256, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "s3_prepare_kernel"); }
    { ProfScope ps(c, "s3_hyp");
      s3_hyp_kernel<<<dim3((a.max_iters + kS3Lanes - 1) / kS3Lanes, a.K), kS3Lanes, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "s3_hyp_kernel"); }
    { ProfScope ps(c, "s3_inlier");
      s3_inlier_kernel<<<dim3(a.max_iters, a.K), 64, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "s3_inlier_kernel"); }
    { ProfScope ps(c, "s3_finish");
      s3_finish_kernel<<<a.K, 256, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "s3_finish_kernel"); }
    return EORB_OK;
}

}  // namespace eorb
