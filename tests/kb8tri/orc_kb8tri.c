/*
 * orc_kb8tri.c -- ORACLE (test infrastructure only): ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs,
 * bOnlyStereo=false, bCoarse) (src/ORBmatcher.cc:975-1214) with KannalaBrandt8::epipolarConstrain (src/CameraModels/
 * KannalaBrandt8.cpp:315-320) = TriangulateMatches (:416-486) and Triangulate (:505-518), restated sequentially in strict
 * IEEE C.  The OpenCV 3.4.1 primitives it reaches are restated on their scalar paths (no IPP, no LAPACK HAL, no FMA
 * contraction): gemm's small-matrix branch, Mat::dot, cv::norm(NORM_L2), addWeighted / subtract of the
 * MatExpr rows, JacobiSVDImpl_<float> and the MatExpr scale of x3D.  Links oracle/_build/liboracle.so for orc_tanf,
 * orc_atan2f, orc_sinf_any, orc_cosf_any, orc_descriptor_distance and orc_three_maxima.
 *
 * Keyframes: numAllKPtsLeft() = nleft (-1: monocular, kps = mvKeysUn; >= 0: the nleft distorted left keypoints then the right
 * ones).  Poses Rt[4][12] = (R row-major, t) of ll, lr, rl, rr (:1005-1013); a monocular pair reads Rt[0] = R12, t12 (:1001-1002).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { float x, y, size, angle, response; int32_t octave, class_id; } kt_keypoint;   /* cv::KeyPoint, 28 B */
/* GeometricCamera: model 0 = Pinhole, 1 = KannalaBrandt8 (mvParameters = fx fy cx cy k0..k3); eorb_camera's layout */
typedef struct { int model; float fx, fy, cx, cy; float k[4]; float precision; } kt_camera;

float orc_tanf(float x);
float orc_atan2f(float y, float x);
float orc_sinf_any(float x);
float orc_cosf_any(float x);
int  orc_descriptor_distance(const uint8_t* a, const uint8_t* b);                   /* ORBmatcher.cc:2360-2378 */
void orc_three_maxima(const int* sizes, int L, int* ind1, int* ind2, int* ind3);    /* :2314-2355 */

#define TH_LOW 50                   /* ORBmatcher.cc:37 */
#define HISTO_LENGTH 30             /* :38 */
#define KB8_DEF_TH_EPC 0.0001f      /* include/CameraModels/KannalaBrandt8.h:37 */
#define KB8_DEF_MIN_PLX 0.9998      /* :38 */
#define KB8_DEF_CHISQ_COEF 5.991    /* :39 */
#define FLT_EPS 1.19209290e-07f     /* FLT_EPSILON */

/* ---- cameras -------------------------------------------------------------------------------------------------------- */
/* unprojectMat (KannalaBrandt8.cpp:157-190: Newton on theta in float, std::tan(float); Pinhole.cpp:59-62) -> (X, Y, 1) */
void orc_kt_unproject(const kt_camera* c, float x, float y, float r[3])
{
    const float pwx = (x - c->cx) / c->fx, pwy = (y - c->cy) / c->fy;
    r[2] = 1.f;
    if (c->model == 0) { r[0] = pwx; r[1] = pwy; return; }
    float scale = 1.f;
    float theta_d = sqrtf(pwx * pwx + pwy * pwy);
    theta_d = fminf(fmaxf((float)(-3.1415926535897932384626433832795 / 2.f), theta_d), (float)(3.1415926535897932384626433832795 / 2.f));
    if ((double)theta_d > 1e-8) {
        float theta = theta_d;
        for (int j = 0; j < 10; j++) {
            const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
            const float k0_theta2 = c->k[0] * theta2, k1_theta4 = c->k[1] * theta4;
            const float k2_theta6 = c->k[2] * theta6, k3_theta8 = c->k[3] * theta8;
            const float theta_fix = (theta * (1 + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                                    (1 + 3 * k0_theta2 + 5 * k1_theta4 + 7 * k2_theta6 + 9 * k3_theta8);
            theta = theta - theta_fix;
            if (fabsf(theta_fix) < c->precision) break;
        }
        scale = orc_tanf(theta) / theta_d;
    }
    r[0] = pwx * scale; r[1] = pwy * scale;
}

/* project(const cv::Mat&) -> project(cv::Point3f) (KannalaBrandt8.cpp:86-109, float throughout; Pinhole.cpp:30-39) */
void orc_kt_project(const kt_camera* c, const float p[3], float* u, float* v)
{
    if (c->model == 0) { *u = c->fx * p[0] / p[2] + c->cx; *v = c->fy * p[1] / p[2] + c->cy; return; }
    const float x2_plus_y2 = p[0] * p[0] + p[1] * p[1];
    const float theta = orc_atan2f(sqrtf(x2_plus_y2), p[2]);
    const float psi = orc_atan2f(p[1], p[0]);
    const float theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
    const float r = theta + c->k[0] * theta3 + c->k[1] * theta5 + c->k[2] * theta7 + c->k[3] * theta9;
    *u = c->fx * r * orc_cosf_any(psi) + c->cx;
    *v = c->fy * r * orc_sinf_any(psi) + c->cy;
}

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
static double kt_hypot(double x, double y) { return sqrt(x * x + y * y); }

/* cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) on a 4x4 float matrix: _SVDcompute transposes A into At and calls
 * JacobiSVDImpl_<float>(At, W, Vt, m = n = 4, n1 = 4, minval = FLT_MIN, eps = 2 FLT_EPSILON) (lapack.cpp).  W and the inner
 * products in double, the rotations in float, max_iter = max(m, 30); W sorted descending with Vt's rows.  The RNG completion
 * of zero singular values touches At (u) only and is left out.  A row-major; returns vt row-major and W. */
void orc_kt_svd4(const float A[16], double Wout[4], float Vt[16])
{
    float At[16];
    double W[4];
    const float eps = FLT_EPS * 2;
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
void orc_kt_triangulate(const float p1[2], const float p2[2], const float Tcw2[12], float x3D[3])
{
    static const float Tcw1[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    float A[16], Vt[16];
    double W[4];
    a_row(p1[0], Tcw1 + 8, Tcw1 + 0, A + 0);
    a_row(p1[1], Tcw1 + 8, Tcw1 + 4, A + 4);
    a_row(p2[0], Tcw2 + 8, Tcw2 + 0, A + 8);
    a_row(p2[1], Tcw2 + 8, Tcw2 + 4, A + 12);
    orc_kt_svd4(A, W, Vt);
    const float w = Vt[15];
    const float sc = (float)(1. / (double)w);
    for (int i = 0; i < 3; i++) x3D[i] = Vt[12 + i] * sc + 0.0f;
}

/* KannalaBrandt8::TriangulateMatches (:416-486): z1, or -1 */
float orc_kt_triangulate_matches(const kt_camera* cam1, const kt_camera* cam2, const kt_keypoint* kp1, const kt_keypoint* kp2,
                                 const float R12[9], const float t12[3], float sigmaLevel, float unc, float* p3D)
{
    float r1[3], r2[3], r21[3];
    orc_kt_unproject(cam1, kp1->x, kp1->y, r1);
    orc_kt_unproject(cam2, kp2->x, kp2->y, r2);
    gemm3x1(R12, r2, NULL, 1.0, r21);                                        /* r21 = R12*r2 */
    const float cosParallaxRays = (float)(dot3(r1, r21) / (norm3(r1) * norm3(r21)));
    if (cosParallaxRays > KB8_DEF_MIN_PLX) return -1;
    const float p11[2] = {r1[0], r1[1]}, p22[2] = {r2[0], r2[1]};
    float R21[9], t21[3], Tcw2[12], x3D[3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R21[3 * i + j] = R12[3 * j + i];
    gemm3x1(R21, t12, NULL, -1.0, t21);                                      /* t21 = -R21*t12 */
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) Tcw2[4 * i + j] = R21[3 * i + j]; Tcw2[4 * i + 3] = t21[i]; }
    orc_kt_triangulate(p11, p22, Tcw2, x3D);
    const float z1 = x3D[2];
    if (z1 <= 0) return -1;
    const float z2 = (float)(dot3(R21 + 6, x3D) + (double)t21[2]);
    if (z2 <= 0) return -1;
    float u, v;
    orc_kt_project(cam1, x3D, &u, &v);
    const float errX1 = u - kp1->x, errY1 = v - kp1->y;
    if ((errX1 * errX1 + errY1 * errY1) > KB8_DEF_CHISQ_COEF * sigmaLevel) return -1;
    float x3D2[3];
    gemm3x1(R21, x3D, t21, 1.0, x3D2);                                       /* R21*x3D + t21 */
    orc_kt_project(cam2, x3D2, &u, &v);
    const float errX2 = u - kp2->x, errY2 = v - kp2->y;
    if ((errX2 * errX2 + errY2 * errY2) > KB8_DEF_CHISQ_COEF * unc) return -1;
    if (p3D) memcpy(p3D, x3D, sizeof x3D);
    return z1;
}

/* batch of TriangulateMatches calls: out[i] for (kps1[i], kps2[i]) with sigma tables indexed by octave */
void orc_kt_triangulate_batch(const kt_camera* cam1, const kt_camera* cam2, const float Rt[12], const kt_keypoint* kps1,
                              const kt_keypoint* kps2, int n, const float* sigma2_1, const float* sigma2_2, float* out)
{
    for (int i = 0; i < n; i++)
        out[i] = orc_kt_triangulate_matches(cam1, cam2, &kps1[i], &kps2[i], Rt, Rt + 9, sigma2_1[kps1[i].octave],
                                            sigma2_2[kps2[i].octave], NULL);
}

static int rot_bin(float a1, float a2)
{   /* :1157-1162 */
    const float factor = 1.0f / HISTO_LENGTH;
    float rot = a1 - a2;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

/* ---- ORBmatcher::SearchForTriangulation :975-1214 ------------------------------------------------------------------ */
/* elig bit 0: no map point and a valid ORB descriptor (:1043-1049, :1073-1077); bit 1 (monocular pairs only): mvuRight >= 0
 * (bStereo :1051, :1079; false whenever pKF1 has mpCamera2).  vbMatched2 is never written.  Returns nmatches. */
int orc_kt_search_for_triangulation(const kt_keypoint* kps1, int n1, int nleft1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
                                    const uint32_t* nodes1, const int32_t* off1, const int32_t* idx1, int nn1,
                                    const kt_keypoint* kps2, int n2, int nleft2, const uint8_t* desc2, int stride2, const uint8_t* elig2,
                                    const uint32_t* nodes2, const int32_t* off2, const int32_t* idx2, int nn2,
                                    const kt_camera cam1[2], const kt_camera cam2[2], const float Rt[48], const float ep[2],
                                    const float* scale2, const float* sigma2_1, const float* sigma2_2, int bCoarse, int checkOri,
                                    int32_t* match12)
{
    (void)n2;
    const int twocam = nleft1 >= 0;                 /* pKF1->mpCamera2 && pKF2->mpCamera2 (both or neither: the caller checks) */
    int nmatches = 0;
    for (int i = 0; i < n1; i++) match12[i] = -1;
    int* rotHist[HISTO_LENGTH]; int rotN[HISTO_LENGTH];
    for (int i = 0; i < HISTO_LENGTH; i++) { rotHist[i] = (int*)malloc(sizeof(int) * (n1 ? n1 : 1)); rotN[i] = 0; }
    int a = 0, b = 0;
    while (a < nn1 && b < nn2) {
        if (nodes1[a] == nodes2[b]) {
            for (int i1 = off1[a]; i1 < off1[a + 1]; i1++) {
                const int id1 = idx1[i1];
                if (!(elig1[id1] & 1)) continue;
                const int bStereo1 = !twocam && (elig1[id1] & 2);
                const kt_keypoint* kp1 = &kps1[id1];                               /* :1058-1060 */
                const int bRight1 = twocam && id1 >= nleft1;                        /* :1062 */
                const uint8_t* d1 = desc1 + (size_t)stride1 * id1;
                int bestDist = TH_LOW, bestIdx2 = -1;
                for (int i2 = off2[b]; i2 < off2[b + 1]; i2++) {
                    const int id2 = idx2[i2];
                    if (!(elig2[id2] & 1)) continue;
                    const int bStereo2 = !twocam && (elig2[id2] & 2);
                    const int dist = orc_descriptor_distance(d1, desc2 + (size_t)stride2 * id2);
                    if (dist > TH_LOW || dist > bestDist) continue;                 /* :1089 */
                    const kt_keypoint* kp2 = &kps2[id2];                           /* :1092-1094 */
                    const int bRight2 = twocam && id2 >= nleft2;                    /* :1095 */
                    if (!bStereo1 && !bStereo2 && !twocam) {                        /* :1097-1105 */
                        const float distex = ep[0] - kp2->x, distey = ep[1] - kp2->y;
                        if (distex * distex + distey * distey < 100 * scale2[kp2->octave]) continue;
                    }
                    const int pose = twocam ? (bRight1 << 1 | bRight2) : 0;         /* :1107-1137: ll, lr, rl, rr */
                    const kt_camera* pc1 = &cam1[twocam ? bRight1 : 0];
                    const kt_camera* pc2 = &cam2[twocam ? bRight2 : 0];
                    if (bCoarse || orc_kt_triangulate_matches(pc1, pc2, kp1, kp2, Rt + 12 * pose, Rt + 12 * pose + 9,
                                                              sigma2_1[kp1->octave], sigma2_2[kp2->octave], NULL) > KB8_DEF_TH_EPC) {
                        bestIdx2 = id2; bestDist = dist;                            /* :1139-1144 (no side effects: order free) */
                    }
                }
                if (bestIdx2 >= 0) {
                    match12[id1] = bestIdx2;
                    nmatches++;
                    if (checkOri) {
                        const int bin = rot_bin(kp1->angle, kps2[bestIdx2].angle);
                        rotHist[bin][rotN[bin]++] = id1;
                    }
                }
            }
            a++; b++;
        } else if (nodes1[a] < nodes2[b]) {
            while (a < nn1 && nodes1[a] < nodes2[b]) a++;
        } else {
            while (b < nn2 && nodes2[b] < nodes1[a]) b++;
        }
    }
    if (checkOri) {
        int ind1 = -1, ind2 = -1, ind3 = -1;
        orc_three_maxima(rotN, HISTO_LENGTH, &ind1, &ind2, &ind3);
        for (int i = 0; i < HISTO_LENGTH; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (int j = 0; j < rotN[i]; j++) { match12[rotHist[i][j]] = -1; nmatches--; }
        }
    }
    for (int i = 0; i < HISTO_LENGTH; i++) free(rotHist[i]);
    return nmatches;
}
