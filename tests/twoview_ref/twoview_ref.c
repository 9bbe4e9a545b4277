/*
 * twoview_ref.c -- TEST INFRASTRUCTURE: what eorb_two_view_ransac and eorb_two_view_check_rt compute, restated sequentially in strict
 * IEEE C (no FMA contraction) from src/TwoViewReconstruction.cc and the scalar paths of OpenCV 3.4.1 that it reaches (no IPP, no
 * LAPACK HAL).  None of the OpenCV choices is pinned against a build of the reference; the device equals this
 * file bit for bit.  The 4x4 SVD sequence is the one of oracle/orc_kb8tri.c (orc_svd4), generalised to (m, n, n1).
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define TV_MAXD 16

/* ---- OpenCV 3.4.1 primitives, scalar paths ------------------------------------------------------------------------------------ */
/* cv::RNG::next (multiply-with-carry) */
static unsigned rng_next(uint64_t* state)
{
    *state = (uint64_t)(unsigned)*state * 4164903690U + (unsigned)(*state >> 32);
    return (unsigned)*state;
}

/* hypot restated as sqrt(x*x + y*y) in double (the host libm's hypot is not pinned) */
static double hypot_d(double x, double y) { return sqrt(x * x + y * y); }

/* JacobiSVDImpl_<float>(At, astep, _W, Vt, vstep, m, n, n1, minval = FLT_MIN, eps = 2 FLT_EPSILON) (modules/core/src/lapack.cpp):
 * one-sided Jacobi on the n rows of At (length m); W and the inner products in double, the rotations in float; max_iter = max(m, 30);
 * descending selection sort of W swapping the rows of both At and Vt; then rows i < n1 of At are scaled by 1/W[i], and a row whose
 * W is <= minval (always a row i >= n) is first replaced by a +-1/m vector drawn from cv::RNG(0x12345678) and orthogonalised against
 * the rows before it.  At has n1 rows. */
static void jacobi_svd(float* At, int astep, double* W, float* Vt, int vstep, int m, int n, int n1)
{
    const float eps = FLT_EPSILON * 2;
    const double minval = FLT_MIN;
    const int max_iter = m > 30 ? m : 30;
    int i, j, k, iter;
    double sd;
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) { const float t = At[i * astep + k]; sd += (double)t * t; }
        W[i] = sd;
        for (k = 0; k < n; k++) Vt[i * vstep + k] = 0;
        Vt[i * vstep + i] = 1;
    }
    for (iter = 0; iter < max_iter; iter++) {
        int changed = 0;
        for (i = 0; i < n - 1; i++)
            for (j = i + 1; j < n; j++) {
                float *Ai = At + i * astep, *Aj = At + j * astep;
                double a = W[i], p = 0, b = W[j];
                for (k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
                if (fabs(p) <= (double)eps * sqrt((double)a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = hypot_d(p, beta);
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
                for (k = 0; k < m; k++) {
                    const float t0 = c * Ai[k] + s * Aj[k];
                    const float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = 1;
                float *Vi = Vt + i * vstep, *Vj = Vt + j * vstep;
                for (k = 0; k < n; k++) {       /* VBLAS<float>::givens gives the scalar loop's values */
                    const float t0 = c * Vi[k] + s * Vj[k];
                    const float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0; Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) { const float t = At[i * astep + k]; sd += (double)t * t; }
        W[i] = sqrt(sd);
    }
    for (i = 0; i < n - 1; i++) {
        j = i;
        for (k = i + 1; k < n; k++) if (W[j] < W[k]) j = k;
        if (i != j) {
            const double tw = W[i]; W[i] = W[j]; W[j] = tw;
            for (k = 0; k < m; k++) { const float t = At[i * astep + k]; At[i * astep + k] = At[j * astep + k]; At[j * astep + k] = t; }
            for (k = 0; k < n; k++) { const float t = Vt[i * vstep + k]; Vt[i * vstep + k] = Vt[j * vstep + k]; Vt[j * vstep + k] = t; }
        }
    }
    uint64_t rng = 0x12345678;
    for (i = 0; i < n1; i++) {
        sd = i < n ? W[i] : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const float val0 = (float)(1. / m);
            for (k = 0; k < m; k++) At[i * astep + k] = (rng_next(&rng) & 256) != 0 ? val0 : -val0;
            for (iter = 0; iter < 2; iter++)
                for (j = 0; j < i; j++) {
                    sd = 0;
                    for (k = 0; k < m; k++) sd += At[i * astep + k] * At[j * astep + k];      /* a float product, summed in double */
                    float asum = 0;
                    for (k = 0; k < m; k++) {
                        const float t = (float)(At[i * astep + k] - sd * At[j * astep + k]);
                        At[i * astep + k] = t;
                        asum += fabsf(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (k = 0; k < m; k++) At[i * astep + k] *= asum;
                }
            sd = 0;
            for (k = 0; k < m; k++) { const float t = At[i * astep + k]; sd += (double)t * t; }
            sd = sqrt(sd);
        }
        const float s = (float)(sd > minval ? 1 / sd : 0.);
        for (k = 0; k < m; k++) At[i * astep + k] *= s;
    }
}

/* _SVDcompute with MODIFY_A | FULL_UV on a rows x cols float matrix (rows, cols <= 16): works on At = A^T when rows >= cols; when
 * rows < cols on A itself (at = true) with the roles of the outputs swapped.  w: min(rows, cols); u: rows x rows; vt: cols x cols. */
void tvr_svd(const float* A, int rows, int cols, float* w, float* u, float* vt)
{
    int m = rows, n = cols, at = 0;
    if (m < n) { m = cols; n = rows; at = 1; }
    const int urows = m;
    float ta[TV_MAXD * TV_MAXD], tv[TV_MAXD * TV_MAXD];
    double W[TV_MAXD];
    memset(ta, 0, sizeof ta);                       /* temp_u = Scalar::all(0): the rows past n */
    for (int i = 0; i < n; i++)
        for (int k = 0; k < m; k++) ta[i * m + k] = at ? A[i * cols + k] : A[k * cols + i];
    jacobi_svd(ta, m, W, tv, n, m, n, urows);
    for (int i = 0; i < n; i++) w[i] = (float)W[i];
    if (!at) {
        if (u) for (int r = 0; r < m; r++) for (int c = 0; c < m; c++) u[r * m + c] = ta[c * m + r];
        if (vt) memcpy(vt, tv, sizeof(float) * n * n);
    } else {
        if (u) for (int r = 0; r < n; r++) for (int c = 0; c < n; c++) u[r * n + c] = tv[c * n + r];
        if (vt) memcpy(vt, ta, sizeof(float) * m * m);
    }
}

/* cv::gemm, the small-matrix branch (flags = 0, len = 3, 3x3 result, no C): three float products summed in float, then
 * (float)(t*alpha + c*beta) in double with alpha = 1 and c*beta = 0*0 */
static void gemm33(const float* a, const float* b, float* d)
{
    float r[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const float t = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
            r[3 * i + j] = (float)((double)t * 1.0 + 0.0 * 0.0);
        }
    memcpy(d, r, sizeof r);
}
/* the same branch with one column and an added vector: R*x + c (the KB8 triangulation) */
static void gemm3x1(const float R[9], const float x[3], const float* c, double alpha, float out[3])
{
    for (int i = 0; i < 3; i++) {
        const float t = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2];
        out[i] = (float)((double)t * alpha + (c ? (double)c[i] * 1.0 : 0.0 * 0.0));
    }
}

/* Mat::inv() of a 3x3 float matrix: cv::invert, DECOMP_LU, the n == 3 closed form.  det3 and the cofactors in double, d = 1./d, each
 * entry (float)(cofactor * d); d == 0 leaves a zero matrix */
static void inv33(const float* S, float* D)
{
#define Sf(r, c) S[3 * (r) + (c)]
    double d = Sf(0, 0) * ((double)Sf(1, 1) * Sf(2, 2) - (double)Sf(1, 2) * Sf(2, 1)) -
               Sf(0, 1) * ((double)Sf(1, 0) * Sf(2, 2) - (double)Sf(1, 2) * Sf(2, 0)) +
               Sf(0, 2) * ((double)Sf(1, 0) * Sf(2, 1) - (double)Sf(1, 1) * Sf(2, 0));
    if (d != 0.) {
        double t[9];
        d = 1. / d;
        t[0] = ((double)Sf(1, 1) * Sf(2, 2) - (double)Sf(1, 2) * Sf(2, 1)) * d;
        t[1] = ((double)Sf(0, 2) * Sf(2, 1) - (double)Sf(0, 1) * Sf(2, 2)) * d;
        t[2] = ((double)Sf(0, 1) * Sf(1, 2) - (double)Sf(0, 2) * Sf(1, 1)) * d;
        t[3] = ((double)Sf(1, 2) * Sf(2, 0) - (double)Sf(1, 0) * Sf(2, 2)) * d;
        t[4] = ((double)Sf(0, 0) * Sf(2, 2) - (double)Sf(0, 2) * Sf(2, 0)) * d;
        t[5] = ((double)Sf(0, 2) * Sf(1, 0) - (double)Sf(0, 0) * Sf(1, 2)) * d;
        t[6] = ((double)Sf(1, 0) * Sf(2, 1) - (double)Sf(1, 1) * Sf(2, 0)) * d;
        t[7] = ((double)Sf(0, 1) * Sf(2, 0) - (double)Sf(0, 0) * Sf(2, 1)) * d;
        t[8] = ((double)Sf(0, 0) * Sf(1, 1) - (double)Sf(0, 1) * Sf(1, 0)) * d;
        for (int i = 0; i < 9; i++) D[i] = (float)t[i];
    } else
        for (int i = 0; i < 9; i++) D[i] = 0.f;
#undef Sf
}
void tvr_inv33(const float* S, float* D) { inv33(S, D); }

/* ---- src/TwoViewReconstruction.cc -------------------------------------------------------------------------------------------------- */
/* Normalize (:1193-1239): over every key in index order, in float.  pn: n x 2; T = {sX, sY, meanX, meanY} -> the 3x3 matrix */
static void normalize(const float* pts, int n, float* pn, float T[9])
{
    float meanX = 0, meanY = 0;
    for (int i = 0; i < n; i++) { meanX += pts[2 * i]; meanY += pts[2 * i + 1]; }
    meanX = meanX / n; meanY = meanY / n;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < n; i++) {
        pn[2 * i] = pts[2 * i] - meanX; pn[2 * i + 1] = pts[2 * i + 1] - meanY;
        meanDevX += fabsf(pn[2 * i]); meanDevY += fabsf(pn[2 * i + 1]);
    }
    meanDevX = meanDevX / n; meanDevY = meanDevY / n;
    const float sX = 1.0f / meanDevX, sY = 1.0f / meanDevY;
    for (int i = 0; i < n; i++) { pn[2 * i] = pn[2 * i] * sX; pn[2 * i + 1] = pn[2 * i + 1] * sY; }
    const float t[9] = {sX, 0.f, -meanX * sX, 0.f, sY, -meanY * sY, 0.f, 0.f, 1.f};
    memcpy(T, t, sizeof t);
}

/* ComputeH21 (:366-406): vt.row(8) of the 16x9 system */
static void compute_h21(const float* p1, const float* p2, float Hn[9])
{
    float A[16 * 9], w[9], vt[81];
    for (int i = 0; i < 8; i++) {
        const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        float* r = A + 18 * i;
        r[0] = 0.f; r[1] = 0.f; r[2] = 0.f; r[3] = -u1; r[4] = -v1; r[5] = -1; r[6] = v2 * u1; r[7] = v2 * v1; r[8] = v2;
        r += 9;
        r[0] = u1; r[1] = v1; r[2] = 1; r[3] = 0.f; r[4] = 0.f; r[5] = 0.f; r[6] = -u2 * u1; r[7] = -u2 * v1; r[8] = -u2;
    }
    tvr_svd(A, 16, 9, w, NULL, vt);
    memcpy(Hn, vt + 72, 9 * sizeof(float));
}

/* ComputeF21 (:408-443): vt.row(8) of the 8x9 system, then the rank-2 projection u*diag(w0, w1, 0)*vt */
static void compute_f21(const float* p1, const float* p2, float Fn[9])
{
    float A[8 * 9], w[9], vt[81], u[9], vt3[9], Fpre[9], d[9] = {0}, ud[9];
    for (int i = 0; i < 8; i++) {
        const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        float* r = A + 9 * i;
        r[0] = u2 * u1; r[1] = u2 * v1; r[2] = u2; r[3] = v2 * u1; r[4] = v2 * v1; r[5] = v2; r[6] = u1; r[7] = v1; r[8] = 1;
    }
    tvr_svd(A, 8, 9, w, NULL, vt);
    memcpy(Fpre, vt + 72, sizeof Fpre);
    tvr_svd(Fpre, 3, 3, w, u, vt3);
    w[2] = 0;
    d[0] = w[0]; d[4] = w[1]; d[8] = w[2];
    gemm33(u, d, ud);
    gemm33(ud, vt3, Fn);
}
void tvr_compute_h21(const float* p1, const float* p2, float* Hn) { compute_h21(p1, p2, Hn); }
void tvr_compute_f21(const float* p1, const float* p2, float* Fn) { compute_f21(p1, p2, Fn); }

/* CheckHomography (:445-528) */
float tvr_check_homography(const float* H21, const float* H12, const float* pts1, const float* pts2, const int32_t* match12, int N,
                           float sigma, float th, uint8_t* inl)
{
    const float h11 = H21[0], h12 = H21[1], h13 = H21[2], h21 = H21[3], h22 = H21[4], h23 = H21[5], h31 = H21[6], h32 = H21[7], h33 = H21[8];
    const float h11inv = H12[0], h12inv = H12[1], h13inv = H12[2], h21inv = H12[3], h22inv = H12[4], h23inv = H12[5], h31inv = H12[6],
                h32inv = H12[7], h33inv = H12[8];
    float score = 0;
    const float invSigmaSquare = 1.0f / (sigma * sigma);
    for (int i = 0; i < N; i++) {
        int bIn = 1;
        const float u1 = pts1[2 * match12[2 * i]], v1 = pts1[2 * match12[2 * i] + 1];
        const float u2 = pts2[2 * match12[2 * i + 1]], v2 = pts2[2 * match12[2 * i + 1] + 1];
        const float w2in1inv = 1.0f / (h31inv * u2 + h32inv * v2 + h33inv);
        const float u2in1 = (h11inv * u2 + h12inv * v2 + h13inv) * w2in1inv;
        const float v2in1 = (h21inv * u2 + h22inv * v2 + h23inv) * w2in1inv;
        const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
        const float chiSquare1 = squareDist1 * invSigmaSquare;
        if (chiSquare1 > th) bIn = 0; else score += th - chiSquare1;
        const float w1in2inv = 1.0f / (h31 * u1 + h32 * v1 + h33);
        const float u1in2 = (h11 * u1 + h12 * v1 + h13) * w1in2inv;
        const float v1in2 = (h21 * u1 + h22 * v1 + h23) * w1in2inv;
        const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
        const float chiSquare2 = squareDist2 * invSigmaSquare;
        if (chiSquare2 > th) bIn = 0; else score += th - chiSquare2;
        inl[i] = (uint8_t)bIn;
    }
    return score;
}

/* CheckFundamental (:530-608) */
float tvr_check_fundamental(const float* F21, const float* pts1, const float* pts2, const int32_t* match12, int N, float sigma, float th,
                            float thScore, uint8_t* inl)
{
    const float f11 = F21[0], f12 = F21[1], f13 = F21[2], f21 = F21[3], f22 = F21[4], f23 = F21[5], f31 = F21[6], f32 = F21[7], f33 = F21[8];
    float score = 0;
    const float invSigmaSquare = 1.0f / (sigma * sigma);
    for (int i = 0; i < N; i++) {
        int bIn = 1;
        const float u1 = pts1[2 * match12[2 * i]], v1 = pts1[2 * match12[2 * i] + 1];
        const float u2 = pts2[2 * match12[2 * i + 1]], v2 = pts2[2 * match12[2 * i + 1] + 1];
        const float a2 = f11 * u1 + f12 * v1 + f13;
        const float b2 = f21 * u1 + f22 * v1 + f23;
        const float c2 = f31 * u1 + f32 * v1 + f33;
        const float num2 = a2 * u2 + b2 * v2 + c2;
        const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
        const float chiSquare1 = squareDist1 * invSigmaSquare;
        if (chiSquare1 > th) bIn = 0; else score += thScore - chiSquare1;
        const float a1 = f11 * u2 + f21 * v2 + f31;
        const float b1 = f12 * u2 + f22 * v2 + f32;
        const float c1 = f13 * u2 + f23 * v2 + f33;
        const float num1 = a1 * u1 + b1 * v1 + c1;
        const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
        const float chiSquare2 = squareDist2 * invSigmaSquare;
        if (chiSquare2 > th) bIn = 0; else score += thScore - chiSquare2;
        inl[i] = (uint8_t)bIn;
    }
    return score;
}

/* FindHomography (:264-312, which & 1) and FindFundamental (:315-363, which & 2) over the caller's sets.  The winner is the first
 * iteration whose score is > the running best, from 0.0f: a NaN never wins; with no winner best_it = -1, the matrix and the flags are
 * zeros.  it_*: per-iteration scores and matrices, or NULL.  Returns 0. */
int tvr_ransac(const float* pts1, int n1, const float* pts2, int n2, const int32_t* match12, int N, const int32_t* sets, int iters,
               float sigma, float th_score, float th_f, int which,
               float* H21, float* SH, int32_t* best_it_h, uint8_t* inliers_h, float* F21, float* SF, int32_t* best_it_f, uint8_t* inliers_f,
               float* it_score_h, float* it_score_f, float* it_H, float* it_F)
{
    float* pn1 = (float*)malloc(sizeof(float) * 2 * (size_t)(n1 > 0 ? n1 : 1));
    float* pn2 = (float*)malloc(sizeof(float) * 2 * (size_t)(n2 > 0 ? n2 : 1));
    uint8_t* cur = (uint8_t*)malloc((size_t)N);
    float T1[9], T2[9], T2inv[9], T2t[9];
    normalize(pts1, n1, pn1, T1);
    normalize(pts2, n2, pn2, T2);
    inv33(T2, T2inv);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) T2t[3 * i + j] = T2[3 * j + i];
    for (int pass = 0; pass < 2; pass++) {
        if (!(which & (1 << pass))) continue;
        float score = 0.0f;
        int best = -1;
        float* M = pass ? F21 : H21;
        uint8_t* inl = pass ? inliers_f : inliers_h;
        memset(M, 0, 9 * sizeof(float));
        memset(inl, 0, (size_t)N);
        for (int it = 0; it < iters; it++) {
            float p1[16], p2[16], Xn[9], tmp[9], X21[9], X12[9], cs;
            for (int j = 0; j < 8; j++) {
                const int idx = sets[8 * it + j];
                p1[2 * j] = pn1[2 * match12[2 * idx]]; p1[2 * j + 1] = pn1[2 * match12[2 * idx] + 1];
                p2[2 * j] = pn2[2 * match12[2 * idx + 1]]; p2[2 * j + 1] = pn2[2 * match12[2 * idx + 1] + 1];
            }
            if (!pass) {
                compute_h21(p1, p2, Xn);
                gemm33(T2inv, Xn, tmp); gemm33(tmp, T1, X21);      /* H21i = T2inv*Hn*T1 */
                inv33(X21, X12);                                    /* H12i = H21i.inv() */
                cs = tvr_check_homography(X21, X12, pts1, pts2, match12, N, sigma, th_score, cur);
            } else {
                compute_f21(p1, p2, Xn);
                gemm33(T2t, Xn, tmp); gemm33(tmp, T1, X21);        /* F21i = T2t*Fn*T1 */
                cs = tvr_check_fundamental(X21, pts1, pts2, match12, N, sigma, th_f, th_score, cur);
            }
            float* its = pass ? it_score_f : it_score_h;
            float* itm = pass ? it_F : it_H;
            if (its) its[it] = cs;
            if (itm) memcpy(itm + 9 * it, X21, sizeof X21);
            if (cs > score) { memcpy(M, X21, sizeof X21); memcpy(inl, cur, (size_t)N); score = cs; best = it; }
        }
        *(pass ? SF : SH) = score;
        *(pass ? best_it_f : best_it_h) = best;
    }
    free(pn1); free(pn2); free(cur);
    return 0;
}

/* Mat::dot (dotProd_32f, length 3: double accumulation, 0.0 + result) and cv::norm(NORM_L2) (normL2Sqr<float, double>, std::sqrt) */
static double dot3(const float* a, const float* b)
{
    double s = 0;
    for (int i = 0; i < 3; i++) s += (double)a[i] * b[i];
    return 0.0 + s;
}
static double norm3(const float* a)
{
    double s = 0;
    for (int i = 0; i < 3; i++) { const double v = a[i]; s += v * v; }
    const double result = 0 + s;
    return sqrt(result);
}
/* "p*P.row(2) - P.row(j)": MatExpr AddEx assigned by cv::subtract when p == 1, else addWeighted_<float, double> */
static void a_row(float p, const float* r2, const float* rj, float* out)
{
    for (int k = 0; k < 4; k++) {
        if ((double)p == 1.0) out[k] = r2[k] - rj[k];
        else out[k] = (float)((double)r2[k] * (double)p + (double)rj[k] * -1.0 + 0.0);
    }
}
/* Triangulate (:1177-1191): vt.row(3) of the 4x4 system, then x*(float)(1./w) + 0 (MatExpr scale through cvtScale32f) */
static void triangulate(const float* kp1, const float* kp2, const float* P1, const float* P2, float x3D[3])
{
    float A[16], w[4], vt[16];
    a_row(kp1[0], P1 + 8, P1 + 0, A + 0);
    a_row(kp1[1], P1 + 8, P1 + 4, A + 4);
    a_row(kp2[0], P2 + 8, P2 + 0, A + 8);
    a_row(kp2[1], P2 + 8, P2 + 4, A + 12);
    tvr_svd(A, 4, 4, w, NULL, vt);
    const float sc = (float)(1. / (double)vt[15]);
    for (int i = 0; i < 3; i++) x3D[i] = vt[12 + i] * sc + 0.0f;
}

/* the order of the ascending sort of vCosParallax as an integer key: -0 before +0, every NaN last (std::sort is undefined with a NaN) */
static uint32_t cos_key(float f)
{
    uint32_t u;
    if (f != f) return 0xffffffffu;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static float cos_of_key(uint32_t k)
{
    uint32_t u = k == 0xffffffffu ? 0x7fc00000u : (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static int cmp_u32(const void* a, const void* b) { const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b; return x < y ? -1 : x > y; }

/* CheckRT (:1242-1352) for Kp poses; pose = R[9] t[3] P2[12] O2[3] (27 floats).  Per pose: n_good, good[n1], p3d[n1*3] (zeros where not
 * written), cos_sel = vCosParallax[min(min_triangulated, size - 1)] after the ascending sort (0 when n_good == 0), cos_all[N] (the
 * cosParallax of a counted match, -2 otherwise; may be NULL) */
int tvr_check_rt(const float* pts1, int n1, const float* pts2, int n2, const int32_t* match12, int N, const uint8_t* inliers, const float* K,
                 float th2, float min_parallax_crt, int min_triangulated, const float* poses, int Kp,
                 int32_t* n_good, uint8_t* good, float* p3d, float* cos_sel, float* cos_all)
{
    (void)n2;
    const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const float P1[12] = {K[0], K[1], K[2], 0.f, K[3], K[4], K[5], 0.f, K[6], K[7], K[8], 0.f};
    const float O1[3] = {0.f, 0.f, 0.f};
    uint32_t* keys = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(N > 0 ? N : 1));
    for (int h = 0; h < Kp; h++) {
        const float *R = poses + 27 * h, *t = R + 9, *P2 = R + 12, *O2 = R + 24;
        uint8_t* vbGood = good + (size_t)h * n1;
        float* vP3D = p3d + (size_t)h * n1 * 3;
        memset(vbGood, 0, (size_t)n1);
        memset(vP3D, 0, sizeof(float) * 3 * (size_t)n1);
        int nGood = 0;
        const float thMinParallex = min_parallax_crt;
        for (int i = 0; i < N; i++) {
            if (cos_all) cos_all[(size_t)h * N + i] = -2.f;
            if (!inliers[i]) continue;
            const int i1 = match12[2 * i], i2 = match12[2 * i + 1];
            const float *kp1 = pts1 + 2 * i1, *kp2 = pts2 + 2 * i2;
            float p3dC1[3];
            triangulate(kp1, kp2, P1, P2, p3dC1);
            if (!isfinite(p3dC1[0]) || !isfinite(p3dC1[1]) || !isfinite(p3dC1[2])) { vbGood[i1] = 0; continue; }
            float normal1[3], normal2[3];
            for (int k = 0; k < 3; k++) { normal1[k] = p3dC1[k] - O1[k]; normal2[k] = p3dC1[k] - O2[k]; }
            const float dist1 = (float)norm3(normal1), dist2 = (float)norm3(normal2);
            const float cosParallax = (float)(dot3(normal1, normal2) / (double)(dist1 * dist2));
            if (p3dC1[2] <= 0 && cosParallax < thMinParallex) continue;
            float p3dC2[3];
            gemm3x1(R, p3dC1, t, 1.0, p3dC2);
            if (p3dC2[2] <= 0 && cosParallax < thMinParallex) continue;
            const float invZ1 = 1.0f / p3dC1[2];
            const float im1x = fx * p3dC1[0] * invZ1 + cx, im1y = fy * p3dC1[1] * invZ1 + cy;
            const float squareError1 = (im1x - kp1[0]) * (im1x - kp1[0]) + (im1y - kp1[1]) * (im1y - kp1[1]);
            if (squareError1 > th2) continue;
            const float invZ2 = 1.0f / p3dC2[2];
            const float im2x = fx * p3dC2[0] * invZ2 + cx, im2y = fy * p3dC2[1] * invZ2 + cy;
            const float squareError2 = (im2x - kp2[0]) * (im2x - kp2[0]) + (im2y - kp2[1]) * (im2y - kp2[1]);
            if (squareError2 > th2) continue;
            keys[nGood] = cos_key(cosParallax);
            if (cos_all) cos_all[(size_t)h * N + i] = cosParallax;
            memcpy(vP3D + 3 * i1, p3dC1, sizeof p3dC1);
            nGood++;
            if (cosParallax < thMinParallex) vbGood[i1] = 1;
        }
        n_good[h] = nGood;
        if (nGood > 0) {
            qsort(keys, (size_t)nGood, sizeof(uint32_t), cmp_u32);
            const int idx = min_triangulated < nGood - 1 ? min_triangulated : nGood - 1;
            cos_sel[h] = cos_of_key(keys[idx < 0 ? 0 : idx]);
        } else
            cos_sel[h] = 0.f;
    }
    free(keys);
    return 0;
}
