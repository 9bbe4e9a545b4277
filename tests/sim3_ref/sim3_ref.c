/*
 * sim3_ref.c -- TEST INFRASTRUCTURE: what eorb_sim3_ransac computes, restated sequentially in strict IEEE C (no FMA contraction) from
 * src/Sim3Solver.cc and the scalar paths of OpenCV 3.4.1 that it reaches (no IPP, no LAPACK HAL).  None of the OpenCV choices is pinned
 * against a build of the reference ("Parity choices of the Sim3 solver"); the device equals this file bit for bit.
 * The camera projections are proj_ref.c's (Pinhole quotient form; KannalaBrandt8 through pr_set_project).
 */
#include "../proj_ref/proj_ref.c"
#include <float.h>
#include <stdlib.h>

/* ---- options and the branch probe ------------------------------------------------------------------------------------------------ */
enum { S3O_FLOAT_BOUND = 0, S3O_HOST_ATAN2 = 1, S3O_N };      /* the named wrong variant "float bound 9.21*sigma2"; libm's atan2 */
static int g_opt[S3O_N];
void s3r_set_option(int which, int v) { if (which >= 0 && which < S3O_N) g_opt[which] = v; }

enum {
    S3P_JACOBI_EPS, S3P_JACOBI_MAXITERS, S3P_Y_NEG, S3P_Y_NONNEG, S3P_SWAP0, S3P_SWAP1, S3P_SWAP2, S3P_NOSWAP, S3P_HYPOT_A, S3P_HYPOT_B,
    S3P_HYPOT_ZERO, S3P_NAN_TRANSFORM, S3P_RODRIGUES_IDENTITY, S3P_RODRIGUES_GENERAL, S3P_SCALE_COPY, S3P_SCALE_MUL, S3P_PINHOLE, S3P_KB8,
    S3P_FIX_SCALE, S3P_FREE_SCALE, S3P_RULE_FEW, S3P_RULE_CONVERGED, S3P_RULE_GREATER, S3P_RULE_EQUAL, S3P_RULE_BELOW, S3P_RULE_EXHAUSTED,
    S3P_ATAN2_Q, S3P_N = S3P_ATAN2_Q + 4
};
static long g_probe[S3P_N];
void s3r_probe_reset(void) { memset(g_probe, 0, sizeof g_probe); }
void s3r_probe_read(long* out) { memcpy(out, g_probe, sizeof g_probe); }
int s3r_probe_count(void) { return S3P_N; }

/* ---- fdlibm e_atan2.c / s_atan.c, the text of dev_datan2 (eorb_slam_amd/csrc/dev_math.h) ----------------------------------------------- */
static uint32_t d_hi(double x) { uint64_t u; memcpy(&u, &x, 8); return (uint32_t)(u >> 32); }
static uint32_t d_lo(double x) { uint64_t u; memcpy(&u, &x, 8); return (uint32_t)u; }
static double s3_atan(double x)
{
    static const double atanhi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00};
    static const double atanlo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17};
    static const double aT[11] = {3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
                                  9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
                                  4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02};
    const int32_t hx = (int32_t)d_hi(x), ix = hx & 0x7fffffff;
    int id;
    if (ix >= 0x44100000) {
        if (ix > 0x7ff00000 || (ix == 0x7ff00000 && d_lo(x) != 0)) return x + x;
        return hx > 0 ? atanhi[3] + atanlo[3] : -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3fdc0000) {
        if (ix < 0x3e200000) return x;
        id = -1;
    } else {
        x = fabs(x);
        if (ix < 0x3ff30000) {
            if (ix < 0x3fe60000) { id = 0; x = (2.0 * x - 1.0) / (2.0 + x); }
            else { id = 1; x = (x - 1.0) / (x + 1.0); }
        } else {
            if (ix < 0x40038000) { id = 2; x = (x - 1.5) / (1.0 + 1.5 * x); }
            else { id = 3; x = -1.0 / x; }
        }
    }
    double z = x * x;
    const double w = z * z;
    const double s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
    const double s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
    if (id < 0) return x - x * (s1 + s2);
    z = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return hx < 0 ? -z : z;
}
double s3r_atan2(double y, double x)
{
    const double tiny = 1.0e-300, pi_o_4 = 7.8539816339744827900E-01, pi_o_2 = 1.5707963267948965580E+00, pi = 3.1415926535897931160E+00,
                 pi_lo = 1.2246467991473531772E-16;
    const int32_t hx = (int32_t)d_hi(x), ix = hx & 0x7fffffff, hy = (int32_t)d_hi(y), iy = hy & 0x7fffffff;
    const uint32_t lx = d_lo(x), ly = d_lo(y);
    if (((uint32_t)ix | ((lx | (0u - lx)) >> 31)) > 0x7ff00000u || ((uint32_t)iy | ((ly | (0u - ly)) >> 31)) > 0x7ff00000u) return x + y;
    if ((((uint32_t)hx - 0x3ff00000u) | lx) == 0) return s3_atan(y);
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);
    if (((uint32_t)iy | ly) == 0) {
        if (m < 2) return y;
        return m == 2 ? pi + tiny : -pi - tiny;
    }
    if (((uint32_t)ix | lx) == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7ff00000) {
        if (iy == 0x7ff00000) return m == 0 ? pi_o_4 + tiny : m == 1 ? -pi_o_4 - tiny : m == 2 ? 3.0 * pi_o_4 + tiny : -3.0 * pi_o_4 - tiny;
        return m == 0 ? 0.0 : m == 1 ? -0.0 : m == 2 ? pi + tiny : -pi - tiny;
    }
    if (iy == 0x7ff00000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int k = (iy - ix) >> 20;
    double z;
    if (k > 60) z = pi_o_2 + 0.5 * pi_lo;
    else if (hx < 0 && k < -60) z = 0.0;
    else z = s3_atan(fabs(y / x));
    g_probe[S3P_ATAN2_Q + m]++;
    if (m == 0) return z;
    if (m == 1) return -z;
    if (m == 2) return pi - (z - pi_lo);
    return (z - pi_lo) - pi;
}
void s3r_atan2_n(const double* y, const double* x, long n, double* out) { for (long i = 0; i < n; i++) out[i] = s3r_atan2(y[i], x[i]); }
void s3r_host_atan2_n(const double* y, const double* x, long n, double* out) { for (long i = 0; i < n; i++) out[i] = atan2(y[i], x[i]); }

/* ---- fdlibm k_sin / k_cos with the two-term pi/2 reduction, the text of dev_dsincos (|x| < 100; a NaN gives two NaNs) ------------------ */
static double s3_ksin(double x, double y, int iy)
{
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double z = x * x, v = z * x, r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    if (iy == 0) return x + v * (S1 + z * r);
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
static double s3_kcos(double x, double y)
{
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = x * x, r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6))))), ax = fabs(x);
    if (ax < 0.3) return 1.0 - (0.5 * z - (z * r - x * y));
    double qx = 0.28125;
    if (!(ax > 0.78125)) {
        const double q = 0.25 * ax;
        uint64_t u; memcpy(&u, &q, 8); u &= 0xffffffff00000000ull; memcpy(&qx, &u, 8);
    }
    const double hz = 0.5 * z - qx, a = 1.0 - qx;
    return a - (hz - (z * r - x * y));
}
static void s3_dsincos(double x, double* sn, double* cs)
{
    if (x != x) { *sn = x; *cs = x; return; }
    if (fabs(x) <= 0.78539816339744830962) { *sn = s3_ksin(x, 0.0, 0); *cs = s3_kcos(x, 0.0); return; }
    const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00, pio2_1t = 6.07710050650619224932e-11;
    const double t = fabs(x);
    int n = (int)(t * invpio2 + 0.5);
    const double fn = (double)n, r = t - fn * pio2_1, w = fn * pio2_1t;
    double a = r - w, b = (r - a) - w;
    if (x < 0) { a = -a; b = -b; n = -n; }
    const double ks = s3_ksin(a, b, 1), kc = s3_kcos(a, b);
    switch (n & 3) {
        case 0: *sn = ks; *cs = kc; break;
        case 1: *sn = kc; *cs = -ks; break;
        case 2: *sn = -ks; *cs = -kc; break;
        default: *sn = -kc; *cs = ks; break;
    }
}

/* ---- OpenCV 3.4.1 primitives, scalar paths ------------------------------------------------------------------------------------------ */
/* the templated hypot of lapack.cpp, float */
static float s3_hypotf(float a, float b)
{
    a = fabsf(a); b = fabsf(b);
    if (a > b) { g_probe[S3P_HYPOT_A]++; b /= a; return a * sqrtf(1 + b * b); }
    if (b > 0) { g_probe[S3P_HYPOT_B]++; a /= b; return b * sqrtf(1 + a * a); }
    g_probe[S3P_HYPOT_ZERO]++;
    return 0;
}

/* cv::eigen on a symmetric 4x4 CV_32F: JacobiImpl_<float>(A, astep = 4, W, V, vstep = 4, n = 4): eps = FLT_EPSILON compared with |p|
 * itself, maxIters = n*n*30, the indR / indC bookkeeping of the largest off-diagonal element per row / column, the rotation order, the
 * descending selection sort that swaps the rows of V.  stats (optional): {rotations executed, 1 when the loop ended at maxIters} */
void s3r_eigen4(const float* src, float* W, float* V, int* stats)
{
    enum { n = 4 };
    float A[16];
    const float eps = FLT_EPSILON;
    int i, j, k, m, iters, indR[n], indC[n];
    const int maxIters = n * n * 30;
    float mv;
    memcpy(A, src, sizeof A);
    for (i = 0; i < n; i++) { for (j = 0; j < n; j++) V[i * n + j] = 0; V[i * n + i] = 1; }
    for (k = 0; k < n; k++) {
        W[k] = A[(n + 1) * k];
        if (k < n - 1) {
            for (m = k + 1, mv = fabsf(A[n * k + m]), i = k + 2; i < n; i++) { const float val = fabsf(A[n * k + i]); if (mv < val) mv = val, m = i; }
            indR[k] = m;
        }
        if (k > 0) {
            for (m = 0, mv = fabsf(A[k]), i = 1; i < k; i++) { const float val = fabsf(A[n * i + k]); if (mv < val) mv = val, m = i; }
            indC[k] = m;
        }
    }
    for (iters = 0; iters < maxIters; iters++) {
        for (k = 0, mv = fabsf(A[indR[0]]), i = 1; i < n - 1; i++) { const float val = fabsf(A[n * i + indR[i]]); if (mv < val) mv = val, k = i; }
        int l = indR[k];
        for (i = 1; i < n; i++) { const float val = fabsf(A[n * indC[i] + i]); if (mv < val) mv = val, k = indC[i], l = i; }
        const float p = A[n * k + l];
        if (fabsf(p) <= eps) break;
        const float y = (float)((W[l] - W[k]) * 0.5);
        float t = fabsf(y) + s3_hypotf(p, y);
        float s = s3_hypotf(p, t);
        const float c = t / s;
        s = p / s; t = (p / t) * p;
        if (y < 0) { g_probe[S3P_Y_NEG]++; s = -s; t = -t; } else g_probe[S3P_Y_NONNEG]++;
        A[n * k + l] = 0;
        W[k] -= t;
        W[l] += t;
        float a0, b0;
#define S3_ROTATE(v0, v1) (a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c)
        for (i = 0; i < k; i++) S3_ROTATE(A[n * i + k], A[n * i + l]);
        for (i = k + 1; i < l; i++) S3_ROTATE(A[n * k + i], A[n * i + l]);
        for (i = l + 1; i < n; i++) S3_ROTATE(A[n * k + i], A[n * l + i]);
        for (i = 0; i < n; i++) S3_ROTATE(V[n * k + i], V[n * l + i]);
#undef S3_ROTATE
        for (j = 0; j < 2; j++) {
            const int idx = j == 0 ? k : l;
            if (idx < n - 1) {
                for (m = idx + 1, mv = fabsf(A[n * idx + m]), i = idx + 2; i < n; i++) { const float val = fabsf(A[n * idx + i]); if (mv < val) mv = val, m = i; }
                indR[idx] = m;
            }
            if (idx > 0) {
                for (m = 0, mv = fabsf(A[idx]), i = 1; i < idx; i++) { const float val = fabsf(A[n * i + idx]); if (mv < val) mv = val, m = i; }
                indC[idx] = m;
            }
        }
    }
    g_probe[iters < maxIters ? S3P_JACOBI_EPS : S3P_JACOBI_MAXITERS]++;
    if (stats) { stats[0] = iters; stats[1] = iters >= maxIters; }
    for (k = 0; k < n - 1; k++) {
        m = k;
        for (i = k + 1; i < n; i++) if (W[m] < W[i]) m = i;
        if (k != m) {
            g_probe[S3P_SWAP0 + k]++;
            const float tw = W[m]; W[m] = W[k]; W[k] = tw;
            for (i = 0; i < n; i++) { const float tv = V[n * m + i]; V[n * m + i] = V[n * k + i]; V[n * k + i] = tv; }
        } else g_probe[S3P_NOSWAP]++;
    }
}

/* Mat::convertTo(dst, CV_32F, alpha): a copy when |alpha - 1| < DBL_EPSILON (noScale), else cvtScale32f: src*(float)alpha + 0.0f */
static void s3_scale(const float* src, int n, double alpha, float* dst)
{
    if (fabs(alpha - 1) < DBL_EPSILON) { g_probe[S3P_SCALE_COPY]++; for (int i = 0; i < n; i++) dst[i] = src[i]; return; }
    g_probe[S3P_SCALE_MUL]++;
    const float a = (float)alpha;
    for (int i = 0; i < n; i++) dst[i] = src[i] * a + 0.0f;
}
/* gemm, small-matrix branch (flags == 0, len 3), 3x3 by 3x1: float products summed in float, then (float)(t*alpha + c*beta) in double */
static void s3_gemm3x1(const float* R, int rstep, const float* x, const float* c, int cstep, double alpha, float* out)
{
    for (int i = 0; i < 3; i++) {
        const float t = R[rstep * i] * x[0] + R[rstep * i + 1] * x[1] + R[rstep * i + 2] * x[2];
        out[i] = (float)((double)t * alpha + (c ? (double)c[cstep * i] * 1.0 : 0.0 * 0.0));
    }
}
/* the same branch, 3x3 by 3x3 */
static void s3_gemm33(const float* a, const float* b, float* d)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const float t = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
            d[3 * i + j] = (float)((double)t * 1.0 + 0.0 * 0.0);
        }
}

/* ComputeCentroid (:305-314): reduceC_<float, float, OpAdd> keeps two accumulators, (p0 + p2) + p1; C/3 is a MatExpr scale by 1./3 */
static void s3_centroid(const float* P, float* Pr, float* C)
{
    float sum[3];
    for (int r = 0; r < 3; r++) sum[r] = (P[3 * r] + P[3 * r + 2]) + P[3 * r + 1];
    s3_scale(sum, 3, 1. / 3, C);
    for (int r = 0; r < 3; r++)
        for (int i = 0; i < 3; i++) Pr[3 * r + i] = P[3 * r + i] - C[r];
}

/* ComputeSim3 (:316-427).  P1, P2: 3x3 row-major, column i = point i.  T12 / T21: 4x4; R: 3x3; t: 3; *s */
void s3r_compute_sim3(const float* P1, const float* P2, int fix_scale, float* T12, float* T21, float* R, float* t, float* s_out)
{
    float Pr1[9], Pr2[9], O1[3], O2[3], M[9], Nm[16], eval[4], evec[16];
    int i, j, k;
    g_probe[fix_scale ? S3P_FIX_SCALE : S3P_FREE_SCALE]++;
    s3_centroid(P1, Pr1, O1);
    s3_centroid(P2, Pr2, O2);
    /* M = Pr2*Pr1.t(): gemm with GEMM_2_T is not the small-matrix branch (that one needs flags == 0) but GEMMSingleMul<float, double>,
     * "A * Bt": the three products and their sum in double, narrowed once */
    for (i = 0; i < 3; i++)
        for (j = 0; j < 3; j++) {
            double s0 = 0;
            for (k = 0; k < 3; k++) s0 += (double)Pr2[3 * i + k] * (double)Pr1[3 * j + k];
            M[3 * i + j] = (float)(s0 * 1.0);
        }
#define Mf(r, c) M[3 * (r) + (c)]
    const float N11 = Mf(0, 0) + Mf(1, 1) + Mf(2, 2), N12 = Mf(1, 2) - Mf(2, 1), N13 = Mf(2, 0) - Mf(0, 2), N14 = Mf(0, 1) - Mf(1, 0);
    const float N22 = Mf(0, 0) - Mf(1, 1) - Mf(2, 2), N23 = Mf(0, 1) + Mf(1, 0), N24 = Mf(2, 0) + Mf(0, 2);
    const float N33 = -Mf(0, 0) + Mf(1, 1) - Mf(2, 2), N34 = Mf(1, 2) + Mf(2, 1), N44 = -Mf(0, 0) - Mf(1, 1) + Mf(2, 2);
#undef Mf
    const float Nn[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    memcpy(Nm, Nn, sizeof Nm);
    s3r_eigen4(Nm, eval, evec, 0);
    float vec[3] = {evec[1], evec[2], evec[3]};
    const double nrm = norm3(vec);
    const double ang = g_opt[S3O_HOST_ATAN2] ? atan2(nrm, (double)evec[0]) : s3r_atan2(nrm, (double)evec[0]);
    /* vec = 2*ang*vec/norm(vec): one MatExpr scale, alpha = (2*ang)*(1./norm), applied as a float by cvtScale32f */
    s3_scale(vec, 3, (2 * ang) * (1. / nrm), vec);
    {   /* cv::Rodrigues, vector to matrix, double throughout */
        double rx = vec[0], ry = vec[1], rz = vec[2];
        const double theta = sqrt(rx * rx + ry * ry + rz * rz);
        if (theta < DBL_EPSILON) {
            g_probe[S3P_RODRIGUES_IDENTITY]++;
            for (i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.f : 0.f;
        } else {
            g_probe[S3P_RODRIGUES_GENERAL]++;
            double sn, c;
            s3_dsincos(theta, &sn, &c);
            const double c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
            rx *= itheta; ry *= itheta; rz *= itheta;
            const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
            const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
            for (i = 0; i < 9; i++) R[i] = (float)((c * ((i % 4 == 0) ? 1. : 0.) + c1 * rrt[i]) + sn * r_x[i]);
        }
    }
    float P3[9], s12;
    s3_gemm33(R, Pr2, P3);
    if (!fix_scale) {
        /* Mat::dot: dotProd_<float>, len 9, unrolled by four: the products in double, each group of four summed before it is added */
        double nom = 0;
        for (i = 0; i <= 9 - 4; i += 4)
            nom += (double)Pr1[i] * P3[i] + (double)Pr1[i + 1] * P3[i + 1] + (double)Pr1[i + 2] * P3[i + 2] + (double)Pr1[i + 3] * P3[i + 3];
        for (; i < 9; i++) nom += (double)Pr1[i] * P3[i];
        nom = 0.0 + nom;
        double den = 0;
        for (i = 0; i < 9; i++) { const float q = P3[i] * P3[i]; den += q; }
        s12 = (float)(nom / den);
    } else s12 = 1.0f;
    /* mt12i = O1 - ms12i*mR12i*O2: one gemm(R, O2, -s, O1, 1) */
    s3_gemm3x1(R, 3, O2, O1, 1, -(double)s12, t);
    float sR[9], Rt[9], sRinv[9], tinv[3];
    s3_scale(R, 9, (double)s12, sR);
    for (i = 0; i < 3; i++) for (j = 0; j < 3; j++) Rt[3 * i + j] = R[3 * j + i];
    {   /* (1.0/ms12i)*mR12i.t(): MatOp_T with alpha; transpose, then convertTo when alpha != 1 */
        const double alpha = 1.0 / (double)s12;
        if (alpha != 1) s3_scale(Rt, 9, alpha, sRinv); else memcpy(sRinv, Rt, sizeof Rt);
    }
    s3_gemm3x1(sRinv, 3, t, 0, 0, -1.0, tinv);      /* -sRinv*mt12i: gemm with alpha = -1 */
    for (i = 0; i < 16; i++) T12[i] = T21[i] = (i % 5 == 0) ? 1.f : 0.f;
    for (i = 0; i < 3; i++) {
        for (j = 0; j < 3; j++) { T12[4 * i + j] = sR[3 * i + j]; T21[4 * i + j] = sRinv[3 * i + j]; }
        T12[4 * i + 3] = t[i]; T21[4 * i + 3] = tinv[i];
    }
    *s_out = s12;
    for (i = 0, k = 0; i < 16; i++) k |= (T12[i] != T12[i]);
    if (k) g_probe[S3P_NAN_TRANSFORM]++;
}

/* mvnMaxError (include/Sim3Solver.h:78-79, src/Sim3Solver.cc:99-100): a size_t, compared as a float (:446) */
float s3r_bound(float sigma2)
{
    if (g_opt[S3O_FLOAT_BOUND]) return (float)(9.210 * (double)sigma2);
    return (float)(size_t)(9.210 * (double)sigma2);
}

/* the result rule (:243-291 under the loop of LoopClosing.cc:698-701) over the iterations' counts -> best_it; out3 = {converged,
 * n_inliers, iterations_used} */
int s3r_result_rule(const int32_t* it_inliers, int iters, int N, int min_inliers, int32_t* out3)
{
    int best = 0, best_it = -1;
    out3[0] = out3[1] = out3[2] = 0;
    if (N < min_inliers) { g_probe[S3P_RULE_FEW]++; return -1; }
    for (int it = 0; it < iters; it++) {
        const int n = it_inliers[it];
        if (n >= best) {
            g_probe[n > best ? S3P_RULE_GREATER : S3P_RULE_EQUAL]++;
            best = n; best_it = it;
            if (n > min_inliers) { g_probe[S3P_RULE_CONVERGED]++; out3[0] = 1; out3[1] = n; out3[2] = it + 1; return it; }
        } else g_probe[S3P_RULE_BELOW]++;
    }
    g_probe[S3P_RULE_EXHAUSTED]++;
    out3[1] = best; out3[2] = iters;
    return best_it;
}

typedef struct s3r_result { int32_t converged, best_it, n_inliers, iterations_used; float T12[16], R12[9], t12[3], s12; } s3r_result;

/* Project (:472-490) + the two squared distances and comparisons of CheckInliers (:438-453) for correspondence i */
static int s3_is_inlier(const float* T12, const float* T21, const pr_camera* cam1, const pr_camera* cam2, const float* X1, const float* X2,
                        const float* p1, const float* p2, float b1, float b2)
{
    float q[3], u, v;
    s3_gemm3x1(T12, 4, X2, T12 + 3, 4, 1.0, q);
    project(cam1, q, &u, &v);
    const float d1x = p1[0] - u, d1y = p1[1] - v;
    s3_gemm3x1(T21, 4, X1, T21 + 3, 4, 1.0, q);
    project(cam2, q, &u, &v);
    const float d2x = u - p2[0], d2y = v - p2[1];
    double e = 0; e += (double)d1x * d1x; e += (double)d1y * d1y;
    const float err1 = (float)(0.0 + e);
    e = 0; e += (double)d2x * d2x; e += (double)d2y * d2y;
    const float err2 = (float)(0.0 + e);
    return err1 < b1 && err2 < b2;
}

/* Project of one point: the image of T*X in the camera (a test builds its planted correspondences around it) */
void s3r_project(const float* T, const pr_camera* cam, const float* X, float* uv)
{
    float q[3];
    s3_gemm3x1(T, 4, X, T + 3, 4, 1.0, q);
    project(cam, q, uv, uv + 1);
}

/* one problem of eorb_sim3_ransac. Returns 0; the aids may be NULL.  work: 12*N floats */
int s3r_ransac(int N, const float* Xw1, const float* Xw2, const float* Rt1, const float* Rt2, const pr_camera* cam1, const pr_camera* cam2,
               const float* sigma2_1, const float* sigma2_2, int fix_scale, int min_inliers, int iters, const int32_t* sets, int stop_early,
               s3r_result* res, uint8_t* inliers, int32_t* it_inliers, float* it_T12, float* it_T21, float* it_scale, float* work)
{
    float *X1 = work, *X2 = X1 + 3 * N, *p1 = X2 + 3 * N, *p2 = p1 + 2 * N, *b1 = p2 + 2 * N, *b2 = b1 + N;
    int i, it;
    memset(res, 0, sizeof *res);
    memset(inliers, 0, (size_t)N);
    res->best_it = -1;
    if (N < min_inliers) { int32_t o[3]; s3r_result_rule(0, 0, N, min_inliers, o); return 0; }
    g_probe[cam1->model ? S3P_KB8 : S3P_PINHOLE]++; g_probe[cam2->model ? S3P_KB8 : S3P_PINHOLE]++;
    for (i = 0; i < N; i++) {
        s3_gemm3x1(Rt1, 3, Xw1 + 3 * i, Rt1 + 9, 1, 1.0, X1 + 3 * i);
        s3_gemm3x1(Rt2, 3, Xw2 + 3 * i, Rt2 + 9, 1, 1.0, X2 + 3 * i);
        project(cam1, X1 + 3 * i, p1 + 2 * i, p1 + 2 * i + 1);
        project(cam2, X2 + 3 * i, p2 + 2 * i, p2 + 2 * i + 1);
        b1[i] = s3r_bound(sigma2_1[i]); b2[i] = s3r_bound(sigma2_2[i]);
    }
    int32_t* cnt = it_inliers ? it_inliers : (int32_t*)malloc(sizeof(int32_t) * (size_t)iters);
    float* hyp = (float*)malloc(sizeof(float) * 45 * (size_t)iters);
    int done = iters;
    for (it = 0; it < iters; it++) {
        float P1[9], P2[9], *h = hyp + 45 * (size_t)it;
        for (i = 0; i < 3; i++) {
            const int idx = sets[3 * it + i];
            for (int r = 0; r < 3; r++) { P1[3 * r + i] = X1[3 * idx + r]; P2[3 * r + i] = X2[3 * idx + r]; }
        }
        s3r_compute_sim3(P1, P2, fix_scale, h, h + 16, h + 32, h + 41, h + 44);
        int n = 0;
        for (i = 0; i < N; i++) n += s3_is_inlier(h, h + 16, cam1, cam2, X1 + 3 * i, X2 + 3 * i, p1 + 2 * i, p2 + 2 * i, b1[i], b2[i]);
        cnt[it] = n;
        if (it_T12) memcpy(it_T12 + 16 * (size_t)it, h, 64);
        if (it_T21) memcpy(it_T21 + 16 * (size_t)it, h + 16, 64);
        if (it_scale) it_scale[it] = h[44];
        if (stop_early && n > min_inliers) { done = it + 1; break; }      /* what the reference computes: the timing baseline */
    }
    int32_t o[3];
    const int best = s3r_result_rule(cnt, done, N, min_inliers, o);
    res->converged = o[0]; res->best_it = best; res->n_inliers = o[1]; res->iterations_used = o[0] ? o[2] : iters;
    if (best >= 0) {
        const float* h = hyp + 45 * (size_t)best;
        memcpy(res->T12, h, 64); memcpy(res->R12, h + 32, 36); memcpy(res->t12, h + 41, 12); res->s12 = h[44];
        for (i = 0; i < N; i++) inliers[i] = (uint8_t)s3_is_inlier(h, h + 16, cam1, cam2, X1 + 3 * i, X2 + 3 * i, p1 + 2 * i, p2 + 2 * i, b1[i], b2[i]);
    }
    if (!it_inliers) free(cnt);
    free(hyp);
    return 0;
}
