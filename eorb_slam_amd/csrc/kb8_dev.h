// kb8_dev.h -- device GeometricCamera math shared by the motion-compensated warps (ev_accum.hip) and the KannalaBrandt8
// SearchForTriangulation (match.hip).  Same fixed IEEE operation order as dev_math.h (-ffp-contract=off); the CPU
// restatement is oracle/orc_kb8tri.c (cameras: oracle/orc_events.c).  DESIGN.md §2 lists each OpenCV choice.
#pragma once
#include "dev_math.h"
#include "../../include/eorb_fe.h"

namespace eorb {

// GeometricCamera: model 0 = Pinhole (CameraModels/Pinhole.cpp:30-62), 1 = KannalaBrandt8 (KannalaBrandt8.cpp:87-190)
struct WarpCam { int model; float fx, fy, cx, cy, k0, k1, k2, k3, precision; };

__host__ __device__ inline WarpCam warp_cam_of(const eorb_camera& c)
{
    return WarpCam{c.model, c.fx, c.fy, c.cx, c.cy, c.k[0], c.k[1], c.k[2], c.k[3], c.precision};
}

// pCamera->unproject(cv::Point2f) -> (X, Y, 1)
__device__ __forceinline__ void cam_unproject(const WarpCam& c, float x, float y, float& X, float& Y)
{
    const float pwx = (x - c.cx) / c.fx, pwy = (y - c.cy) / c.fy;
    if (c.model == 0) { X = pwx; Y = pwy; return; }
    // Newton iterations on theta, all in float (:164-187)
    float scale = 1.f;
    float theta_d = sqrtf(pwx * pwx + pwy * pwy);
    theta_d = fminf(fmaxf((float)(-3.1415926535897932384626433832795 / 2.f), theta_d), (float)(3.1415926535897932384626433832795 / 2.f));
    if ((double)theta_d > 1e-8) {
        float theta = theta_d;
        for (int j = 0; j < 10; j++) {
            const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
            const float k0_theta2 = c.k0 * theta2, k1_theta4 = c.k1 * theta4;
            const float k2_theta6 = c.k2 * theta6, k3_theta8 = c.k3 * theta8;
            const float theta_fix = (theta * (1 + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                                    (1 + 3 * k0_theta2 + 5 * k1_theta4 + 7 * k2_theta6 + 9 * k3_theta8);
            theta = theta - theta_fix;
            if (fabsf(theta_fix) < c.precision) break;
        }
        scale = dev_tanf(theta) / theta_d;
    }
    X = pwx * scale; Y = pwy * scale;
}

// KannalaBrandt8::project(cv::Point3f) (:87-103), float throughout
__device__ __forceinline__ void kb8_project_f(const WarpCam& c, float X, float Y, float Z, float& u, float& v)
{
    const float x2_plus_y2 = X * X + Y * Y;
    const float theta = dev_atan2f(sqrtf(x2_plus_y2), Z);
    const float psi = dev_atan2f(Y, X);
    const float theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
    const float r = theta + c.k0 * theta3 + c.k1 * theta5 + c.k2 * theta7 + c.k3 * theta9;
    float ps, pc;
    dev_sincosf(psi, &ps, &pc);
    u = c.fx * r * pc + c.cx;
    v = c.fy * r * ps + c.cy;
}

// pCamera->project(const cv::Mat&) -> project(cv::Point3f) of either model (Pinhole.cpp:30-39)
__device__ __forceinline__ void cam_project_f(const WarpCam& c, const float p[3], float& u, float& v)
{
    if (c.model == 0) { u = c.fx * p[0] / p[2] + c.cx; v = c.fy * p[1] / p[2] + c.cy; return; }
    kb8_project_f(c, p[0], p[1], p[2], u, v);
}

// ---- OpenCV 3.4.1 primitives of KannalaBrandt8::TriangulateMatches, scalar paths (no IPP, no LAPACK HAL) ------------------
// gemm, 2 <= len <= 4 and d_size.width == 1 (matmul.cpp): products summed in float, then (float)(t*alpha + c*beta) in double
__device__ __forceinline__ void cv_gemm3x1(const float* R, const float* x, const float* c, double alpha, float* out)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float t = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2];
        out[i] = (float)((double)t * alpha + (c ? (double)c[i] * 1.0 : 0.0 * 0.0));
    }
}
// cv::gemm, small-matrix branch (len = 3, 3x3 by 3x3, no C): float products summed in float, then (float)(t*alpha + c*beta) in double;
// d may be a or b
__device__ __forceinline__ void cv_gemm33(const float* a, const float* b, float* d)
{
    float r[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float t = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
            r[3 * i + j] = (float)((double)t * 1.0 + 0.0 * 0.0);
        }
#pragma unroll
    for (int i = 0; i < 9; i++) d[i] = r[i];
}
// Mat::dot (dotProd_32f, len 3: the double accumulation of dotProd_, returned as 0.0 + result)
__device__ __forceinline__ double cv_dot3(const float* a, const float* b)
{
    double s = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) s += (double)a[i] * b[i];
    return 0.0 + s;
}
// cv::norm(NORM_L2) of a continuous float Mat: normL2Sqr<float, double>, std::sqrt
__device__ __forceinline__ double cv_norm3(const float* a)
{
    double s = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) { const double v = a[i]; s += v * v; }
    const double result = 0 + s;
    return sqrt(result);
}
// "p*T.row(2) - T.row(j)": cv::subtract when p == 1, else addWeighted_<float, double>(row 2, p, row j, -1, 0)
__device__ __forceinline__ void cv_a_row(float p, const float* r2, const float* rj, float* out)
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if ((double)p == 1.0) out[k] = r2[k] - rj[k];
        else out[k] = (float)((double)r2[k] * (double)p + (double)rj[k] * -1.0 + 0.0);
    }
}
// hypot restated as sqrt(x*x + y*y) in double, as the oracle does
__device__ __forceinline__ double kt_hypot(double x, double y) { return sqrt(x * x + y * y); }

// cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV), 4x4 float: JacobiSVDImpl_<float> on At = A^T (lapack.cpp), W and inner
// products in double, rotations in float, eps = 2 FLT_EPSILON, max_iter = 30, rows of Vt sorted by descending W.
// Returns vt.row(3) only (the RNG completion of zero singular values touches u alone).
__device__ __forceinline__ void cv_svd4_vt3(const float* A, float* v3)
{
    float At[16], Vt[16];
    double W[4];
    const float eps = 1.19209290e-07f * 2;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < 4; k++) At[4 * i + k] = A[4 * k + i];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { const float t = At[4 * i + k]; sd += (double)t * t; }
        W[i] = sd;
#pragma unroll
        for (int k = 0; k < 4; k++) Vt[4 * i + k] = (k == i) ? 1.f : 0.f;
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i + 1; j < 4; j++) {
                float *Ai = At + 4 * i, *Aj = At + 4 * j;
                double a = W[i], p = 0, b = W[j];
#pragma unroll
                for (int k = 0; k < 4; k++) p += (double)Ai[k] * Aj[k];
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
                for (int k = 0; k < 4; k++) {
                    const float t0 = c * Ai[k] + s * Aj[k];
                    const float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                float *Vi = Vt + 4 * i, *Vj = Vt + 4 * j;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float t0 = c * Vi[k] + s * Vj[k];
                    const float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0; Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { const float t = At[4 * i + k]; sd += (double)t * t; }
        W[i] = sqrt(sd);
    }
    // selection sort (descending); only the row that lands last is needed: track the permutation of row indices
    int perm[4] = {0, 1, 2, 3};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        int j = i;
#pragma unroll
        for (int k = i + 1; k < 4; k++) if (W[j] < W[k]) j = k;
        if (i != j) {
            const double tw = W[i]; W[i] = W[j]; W[j] = tw;
            const int tp = perm[i]; perm[i] = perm[j]; perm[j] = tp;
        }
    }
    const int r = perm[3];
#pragma unroll
    for (int k = 0; k < 4; k++) v3[k] = r == 0 ? Vt[k] : r == 1 ? Vt[4 + k] : r == 2 ? Vt[8 + k] : Vt[12 + k];
}

// KannalaBrandt8::TriangulateMatches (:416-486) with Triangulate (:505-518): z1, or -1.  R12 row-major.
__device__ __forceinline__ float kb8_triangulate_matches(const WarpCam& cam1, const WarpCam& cam2, float x1, float y1, float x2,
                                                         float y2, const float* R12, const float* t12, float sigmaLevel, float unc)
{
    float r1[3], r2[3], r21[3];
    cam_unproject(cam1, x1, y1, r1[0], r1[1]); r1[2] = 1.f;
    cam_unproject(cam2, x2, y2, r2[0], r2[1]); r2[2] = 1.f;
    cv_gemm3x1(R12, r2, nullptr, 1.0, r21);
    const float cosParallaxRays = (float)(cv_dot3(r1, r21) / (cv_norm3(r1) * cv_norm3(r21)));
    if ((double)cosParallaxRays > 0.9998) return -1;                                 // KB8_DEF_MIN_PLX
    float R21[9], t21[3], T2[12], A[16], v3[4];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R21[3 * i + j] = R12[3 * j + i];
    cv_gemm3x1(R21, t12, nullptr, -1.0, t21);                                          // t21 = -R21*t12
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) T2[4 * i + j] = R21[3 * i + j];
        T2[4 * i + 3] = t21[i];
    }
    const float T1r0[4] = {1.f, 0.f, 0.f, 0.f}, T1r1[4] = {0.f, 1.f, 0.f, 0.f}, T1r2[4] = {0.f, 0.f, 1.f, 0.f};
    cv_a_row(r1[0], T1r2, T1r0, A + 0);
    cv_a_row(r1[1], T1r2, T1r1, A + 4);
    cv_a_row(r2[0], T2 + 8, T2 + 0, A + 8);
    cv_a_row(r2[1], T2 + 8, T2 + 4, A + 12);
    cv_svd4_vt3(A, v3);
    // x3D.rowRange(0,3)/w: MatExpr scale 1./w -> convertTo -> cvtScale32f with the float scale (float)(1./w), src*scale + 0
    const float sc = (float)(1. / (double)v3[3]);
    const float x3D[3] = {v3[0] * sc + 0.0f, v3[1] * sc + 0.0f, v3[2] * sc + 0.0f};
    const float z1 = x3D[2];
    if (z1 <= 0) return -1;
    const float z2 = (float)(cv_dot3(R21 + 6, x3D) + (double)t21[2]);
    if (z2 <= 0) return -1;
    float u, v;
    cam_project_f(cam1, x3D, u, v);
    const float errX1 = u - x1, errY1 = v - y1;
    if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigmaLevel) return -1;   // KB8_DEF_CHISQ_COEF
    float x3D2[3];
    cv_gemm3x1(R21, x3D, t21, 1.0, x3D2);
    cam_project_f(cam2, x3D2, u, v);
    const float errX2 = u - x2, errY2 = v - y2;
    if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)unc) return -1;
    return z1;
}

}  // namespace eorb
