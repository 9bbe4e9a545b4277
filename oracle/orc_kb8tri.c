/*
 * orc_kb8tri.c -- ORACLE (test infrastructure only): KannalaBrandt8::epipolarConstrain (src/CameraModels/KannalaBrandt8.cpp:315-320)
 * = TriangulateMatches (:416-486) and Triangulate (:505-518), the geometric test of SearchForTriangulation (orc_match.c) on
 * KannalaBrandt8 cameras, restated sequentially in strict IEEE C.  The OpenCV 3.4.1 primitives it reaches are restated on their
 * scalar paths (no IPP, no LAPACK HAL, no FMA contraction): gemm's small-matrix branch, Mat::dot, cv::norm(NORM_L2),
 * addWeighted / subtract of the MatExpr rows, JacobiSVDImpl_<float> and the MatExpr scale of x3D.  The cameras' unproject and
 * project are orc_events.c's.
 */
#include "eorb_oracle.h"
#include <float.h>
#include <math.h>
#include <string.h>

#define KB8_DEF_TH_EPC 0.0001f      /* include/CameraModels/KannalaBrandt8.h:37 */
#define KB8_DEF_MIN_PLX 0.9998      /* :38 */
#define KB8_DEF_CHISQ_COEF 5.991    /* :39 */

/* ---- OpenCV 3.4.1 primitives, scalar paths ------------------------------------------------------------------------- */
/* gemm (matmul.cpp, 2 <= len <= 4 branch, d_size.width == 1): the products summed in float, then (float)(t*alpha + c*beta) in
 * double; alpha = 1, c = 0 or the added vector with beta = 1, or alpha = -1 for "-R*t" */
static void gemm3x1(const float R[9], const float x[3], const float* c, double alpha, float out[3])
{
    for (int i = 0; i < 3; i++) {
        const float t = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2];
        out[i] = (float)((double)t * alpha + (c ? (double)c[i] * 1.0 : 0.0 * 0.0));
    }
}
/* Mat::dot -> dotProd_32f (len 3 < 4: no SIMD block; dotProd_ accumulates in double), returned as r + result */
static double dot3(const float* a, const float* b)
{
    double s = 0;
    for (int i = 0; i < 3; i++) s += (double)a[i] * b[i];
    return 0.0 + s;
}
/* cv::norm(NORM_L2) on a continuous float Mat: normL2_32f = normL2Sqr<float, double>, then std::sqrt */
static double norm3(const float* a)
{
    double s = 0;
    for (int i = 0; i < 3; i++) { const double v = a[i]; s += v * v; }
    const double result = 0 + s;
    return sqrt(result);
}
/* "A.row(k) = p*T.row(2) - T.row(j)": MatExpr AddEx(a = row 2, alpha = p, b = row j, beta = -1) assigned by MatOp_AddEx::assign:
 * alpha == 1 -> cv::subtract (float), otherwise cv::addWeighted(a, p, b, -1, 0) = addWeighted_<float, double> */
static void a_row(float p, const float* r2, const float* rj, float* out)
{
    for (int k = 0; k < 4; k++) {
        if ((double)p == 1.0) out[k] = r2[k] - rj[k];
        else out[k] = (float)((double)r2[k] * (double)p + (double)rj[k] * -1.0 + 0.0);
    }
}
/* hypot: restated as sqrt(x*x + y*y) in double (the host libm's hypot is not pinned) */
static double hypot_d(double x, double y) { return sqrt(x * x + y * y); }

/* cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) on a 4x4 float matrix: _SVDcompute transposes A into At and calls
 * JacobiSVDImpl_<float>(At, W, Vt, m = n = 4, n1 = 4, minval = FLT_MIN, eps = 2 FLT_EPSILON) (lapack.cpp).  W and the inner
 * products in double, the rotations in float, max_iter = max(m, 30); W sorted descending with Vt's rows.  The RNG completion
 * of zero singular values touches At (u) only and is left out.  A row-major; returns vt row-major and W. */
void orc_svd4(const float A[16], double Wout[4], float Vt[16])
{
    float At[16];
    double W[4];
    const float eps = FLT_EPSILON * 2;
    const int m = 4, n = 4, max_iter = 30;
    for (int i = 0; i < 4; i++) for (int k = 0; k < 4; k++) At[4 * i + k] = A[4 * k + i];
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const float t = At[4 * i + k]; sd += (double)t * t; }
        W[i] = sd;
        for (int k = 0; k < n; k++) Vt[4 * i + k] = 0;
        Vt[4 * i + i] = 1;
    }
    for (int iter = 0; iter < max_iter; iter++) {
        int changed = 0;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                float *Ai = At + 4 * i, *Aj = At + 4 * j;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
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
                for (int k = 0; k < m; k++) {
                    const float t0 = c * Ai[k] + s * Aj[k];
                    const float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = 1;
                float *Vi = Vt + 4 * i, *Vj = Vt + 4 * j;
                for (int k = 0; k < n; k++) {       /* VBLAS<float>::givens: (a c + b s, b c - a s) = the scalar loop's values */
                    const float t0 = c * Vi[k] + s * Vj[k];
                    const float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0; Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const float t = At[4 * i + k]; sd += (double)t * t; }
        W[i] = sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++) if (W[j] < W[k]) j = k;
        if (i != j) {
            double tw = W[i]; W[i] = W[j]; W[j] = tw;
            for (int k = 0; k < n; k++) { float t = Vt[4 * i + k]; Vt[4 * i + k] = Vt[4 * j + k]; Vt[4 * j + k] = t; }
        }
    }
    for (int i = 0; i < 4; i++) Wout[i] = W[i];
}

/* KannalaBrandt8::Triangulate (:505-518) with Tcw1 = [I | 0]; "x3D.rowRange(0,3)/w" is MatExpr AddEx(alpha = 1./w) assigned
 * through convertTo -> cvtScale32f: (float)(1./(double)w) as the scale, dst = src*scale + 0 in float */
static void triangulate(const float p1[2], const float p2[2], const float Tcw2[12], float x3D[3])
{
    static const float Tcw1[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    float A[16], Vt[16];
    double W[4];
    a_row(p1[0], Tcw1 + 8, Tcw1 + 0, A + 0);
    a_row(p1[1], Tcw1 + 8, Tcw1 + 4, A + 4);
    a_row(p2[0], Tcw2 + 8, Tcw2 + 0, A + 8);
    a_row(p2[1], Tcw2 + 8, Tcw2 + 4, A + 12);
    orc_svd4(A, W, Vt);
    const float w = Vt[15];
    const float sc = (float)(1. / (double)w);
    for (int i = 0; i < 3; i++) x3D[i] = Vt[12 + i] * sc + 0.0f;
}

/* KannalaBrandt8::TriangulateMatches (:416-486): z1, or -1 */
float orc_kb8_triangulate_matches(const orc_camera* cam1, const orc_camera* cam2, const orc_keypoint* kp1, const orc_keypoint* kp2,
                                  const float R12[9], const float t12[3], float sigmaLevel, float unc, float* p3D)
{
    float r1[3], r2[3], r21[3];
    orc_camera_unproject(cam1, kp1->x, kp1->y, r1);
    orc_camera_unproject(cam2, kp2->x, kp2->y, r2);
    gemm3x1(R12, r2, NULL, 1.0, r21);                                        /* r21 = R12*r2 */
    const float cosParallaxRays = (float)(dot3(r1, r21) / (norm3(r1) * norm3(r21)));
    if (cosParallaxRays > KB8_DEF_MIN_PLX) return -1;
    const float p11[2] = {r1[0], r1[1]}, p22[2] = {r2[0], r2[1]};
    float R21[9], t21[3], Tcw2[12], x3D[3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R21[3 * i + j] = R12[3 * j + i];
    gemm3x1(R21, t12, NULL, -1.0, t21);                                      /* t21 = -R21*t12 */
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) Tcw2[4 * i + j] = R21[3 * i + j]; Tcw2[4 * i + 3] = t21[i]; }
    triangulate(p11, p22, Tcw2, x3D);
    const float z1 = x3D[2];
    if (z1 <= 0) return -1;
    const float z2 = (float)(dot3(R21 + 6, x3D) + (double)t21[2]);
    if (z2 <= 0) return -1;
    float u, v;
    orc_camera_project(cam1, x3D, &u, &v);
    const float errX1 = u - kp1->x, errY1 = v - kp1->y;
    if ((errX1 * errX1 + errY1 * errY1) > KB8_DEF_CHISQ_COEF * sigmaLevel) return -1;
    float x3D2[3];
    gemm3x1(R21, x3D, t21, 1.0, x3D2);                                       /* R21*x3D + t21 */
    orc_camera_project(cam2, x3D2, &u, &v);
    const float errX2 = u - kp2->x, errY2 = v - kp2->y;
    if ((errX2 * errX2 + errY2 * errY2) > KB8_DEF_CHISQ_COEF * unc) return -1;
    if (p3D) memcpy(p3D, x3D, sizeof x3D);
    return z1;
}

/* KannalaBrandt8::epipolarConstrain (:315-320) */
int orc_kb8_epipolar_constrain(const orc_camera* cam1, const orc_camera* cam2, const orc_keypoint* kp1, const orc_keypoint* kp2,
                               const float R12[9], const float t12[3], float sigmaLevel, float unc)
{
    return orc_kb8_triangulate_matches(cam1, cam2, kp1, kp2, R12, t12, sigmaLevel, unc, NULL) > KB8_DEF_TH_EPC;
}

/* batch of TriangulateMatches calls: out[i] for (kps1[i], kps2[i]) with sigma tables indexed by octave */
void orc_kb8_triangulate_batch(const orc_camera* cam1, const orc_camera* cam2, const float Rt[12], const orc_keypoint* kps1,
                               const orc_keypoint* kps2, int n, const float* sigma2_1, const float* sigma2_2, float* out)
{
    for (int i = 0; i < n; i++)
        out[i] = orc_kb8_triangulate_matches(cam1, cam2, &kps1[i], &kps2[i], Rt, Rt + 9, sigma2_1[kps1[i].octave],
                                             sigma2_2[kps2[i].octave], NULL);
}
