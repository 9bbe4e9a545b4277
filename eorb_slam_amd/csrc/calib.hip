// calib.hip -- MyCalibrator on the device (src/Utils/MyCalibrator.cpp): cv::undistortPoints and cv::fisheye::undistortPoints of
// OpenCV 3.4.1 restated in double, one thread per point, in the operation order of their scalar paths (-ffp-contract=off: every
// operation below is one IEEE operation).  The CPU restatement the tests compare with is tests/calib_ref/calib_ref.c; DESIGN.md
// section 2 lists every choice.  Nothing here shares data between lanes: no LDS, no cross-lane operation.
#include "eorb_ctx.h"
#include <string.h>

namespace eorb {

// ---- fdlibm's double tan (k_tan.c, s_tan.c, the |x| < 3 pi / 4 branch of e_rem_pio2.c) ---------------------------------------------
// cv::fisheye::undistortPoints ends in std::tan(theta) with theta in (0, pi/2] for every sane calibration (theta_d is clamped to
// pi/2): that is the branch of the reduction restated exactly; beyond 3 pi / 4 the two-term form of dev_dsincos is used.
__device__ __forceinline__ double cal_lo0(double v) { return __longlong_as_double(__double_as_longlong(v) & (long long)0xffffffff00000000ull); }

__device__ __forceinline__ double cal_ktan(double x, double y, int iy)
{
    const double T0 = 3.33333333333334091986e-01, T1 = 1.33333333333201242699e-01, T2 = 5.39682539762260521377e-02,
                 T3 = 2.18694882948595424599e-02, T4 = 8.86323982359930005737e-03, T5 = 3.59207910759131235356e-03,
                 T6 = 1.45620945432529025516e-03, T7 = 5.88041240820264096874e-04, T8 = 2.46463134818469906812e-04,
                 T9 = 7.81794442939557092300e-05, T10 = 7.14072491382608190305e-05, T11 = -1.85586374855275456654e-05,
                 T12 = 2.59073051863633712884e-05;
    const double pio4 = 7.85398163397448278999e-01, pio4lo = 3.06161699786838301793e-17;
    const long long xb = __double_as_longlong(x);
    const int hx = (int)(xb >> 32), ix = hx & 0x7fffffff;
    const unsigned lx = (unsigned)xb;
    double z, r, v, w, s;
    if (ix < 0x3e300000) {                                    // |x| < 2^-28
        if ((int)x == 0) {
            if (((ix | lx) | (unsigned)(iy + 1)) == 0) return 1.0 / fabs(x);
            if (iy == 1) return x;
            z = w = x + y;
            z = cal_lo0(z);
            v = y - (z - x);
            const double a = -1.0 / w;
            const double t = cal_lo0(a);
            s = 1.0 + t * z;
            return t + a * (s + t * v);
        }
    }
    if (ix >= 0x3FE59428) {                                   // |x| >= 0.6744
        if (hx < 0) { x = -x; y = -y; }
        z = pio4 - x;
        w = pio4lo - y;
        x = z + w; y = 0.0;
    }
    z = x * x;
    w = z * z;
    r = T1 + w * (T3 + w * (T5 + w * (T7 + w * (T9 + w * T11))));
    v = z * (T2 + w * (T4 + w * (T6 + w * (T8 + w * (T10 + w * T12)))));
    s = z * x;
    r = y + z * (s * (r + v) + y);
    r += T0 * s;
    w = x + r;
    if (ix >= 0x3FE59428) {
        v = (double)iy;
        return (double)(1 - ((hx >> 30) & 2)) * (v - 2.0 * (x - (w * w / (w + v) - r)));
    }
    if (iy == 1) return w;
    z = cal_lo0(w);
    v = r - (z - x);
    const double a = -1.0 / w;
    const double t = cal_lo0(a);
    s = 1.0 + t * z;
    return t + a * (s + t * v);
}

__device__ __forceinline__ double cal_tan(double x)
{
    const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00, pio2_1t = 6.07710050650619224932e-11,
                 pio2_2 = 6.07710050630396597660e-11, pio2_2t = 2.02226624879595063154e-21;
    const int hx = (int)(__double_as_longlong(x) >> 32), ix = hx & 0x7fffffff;
    if (ix <= 0x3fe921fb) return cal_ktan(x, 0.0, 1);
    if (ix >= 0x41d00000) return (x - x) / (x - x);           // inf, NaN (fdlibm: x - x) and, here, |x| >= 2^30: NaN
    const double t = fabs(x);
    double a, b;
    int n;
    if (ix < 0x4002d97c) {                                    // |x| < 3 pi / 4: n = 1
        double z = t - pio2_1;
        if (ix != 0x3ff921fb) { a = z - pio2_1t; b = (z - a) - pio2_1t; }
        else { z -= pio2_2; a = z - pio2_2t; b = (z - a) - pio2_2t; }
        n = 1;
    } else {
        n = (int)(t * invpio2 + 0.5);
        const double fn = (double)n;
        const double r = t - fn * pio2_1;
        const double w = fn * pio2_1t;
        a = r - w;
        b = (r - a) - w;
    }
    if (hx < 0) { a = -a; b = -b; n = -n; }
    return cal_ktan(a, b, 1 - ((n & 1) << 1));
}

// ---- cvUndistortPoints (imgproc/src/undistort.cpp), one point ---------------------------------------------------------------
__device__ __forceinline__ void cal_pinhole(const CalibDev& P, float sx, float sy, float& ox, float& oy)
{
    double x = ((double)sx - P.cx) * P.ifx, y = ((double)sy - P.cy) * P.ify;
    // invMatTilt * Vec3d(x, y, 1) with the identity the default tilt terms leave: Matx product, s = 0; s += a * b in index order
    const double u0 = ((0.0 + 1.0 * x) + 0.0 * y) + 0.0 * 1.0;
    const double u1 = ((0.0 + 0.0 * x) + 1.0 * y) + 0.0 * 1.0;
    const double u2 = ((0.0 + 0.0 * x) + 0.0 * y) + 1.0 * 1.0;
    const double invProj = u2 != 0.0 ? 1. / u2 : 1;
    const double x0 = x = invProj * u0, y0 = y = invProj * u1;
    const double* k = P.k;
    for (int j = 0; j < 5; j++) {                             // criteria (COUNT, 5, 0.01): no EPS exit
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    const double* RR = P.RR;
    const double xx = RR[0] * x + RR[1] * y + RR[2];
    const double yy = RR[3] * x + RR[4] * y + RR[5];
    const double ww = 1. / (RR[6] * x + RR[7] * y + RR[8]);
    ox = (float)(xx * ww);
    oy = (float)(yy * ww);
}

// ---- cv::fisheye::undistortPoints (calib3d/src/fisheye.cpp), one point: the fixed-point form of 3.4.1 ----------------------------------
__device__ __forceinline__ void cal_fisheye(const CalibDev& P, float sx, float sy, float& ox, float& oy)
{
    const double pwx = ((double)sx - P.cx) / P.fx, pwy = ((double)sy - P.cy) / P.fy;
    double scale = 1.0;
    double theta_d = sqrt(pwx * pwx + pwy * pwy);
    const double hpi = 3.1415926535897932384626433832795 / 2.;
    theta_d = (-hpi < theta_d) ? theta_d : -hpi;              // std::max(-CV_PI/2., theta_d): a NaN gives -pi/2
    theta_d = (hpi < theta_d) ? hpi : theta_d;                // std::min(.., CV_PI/2.)
    if (theta_d > 1e-8) {
        double theta = theta_d;
        for (int j = 0; j < 10; j++) {
            const double theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta6 * theta2;
            theta = theta_d / (1 + P.k[0] * theta2 + P.k[1] * theta4 + P.k[2] * theta6 + P.k[3] * theta8);
        }
        scale = cal_tan(theta) / theta_d;
    }
    const double pux = pwx * scale, puy = pwy * scale;
    const double* RR = P.RR;
    const double p0 = ((0.0 + RR[0] * pux) + RR[1] * puy) + RR[2] * 1.0;
    const double p1 = ((0.0 + RR[3] * pux) + RR[4] * puy) + RR[5] * 1.0;
    const double p2 = ((0.0 + RR[6] * pux) + RR[7] * puy) + RR[8] * 1.0;
    ox = (float)(p0 / p2);
    oy = (float)(p1 / p2);
}

__device__ __forceinline__ void cal_point(const CalibDev& P, float sx, float sy, float& ox, float& oy)
{
    if (!P.gate) { ox = sx; oy = sy; return; }
    if (P.model == 0) cal_pinhole(P, sx, sy, ox, oy); else cal_fisheye(P, sx, sy, ox, oy);
}

// records of REC floats whose first two are the point: REC = 2 points, 7 cv::KeyPoint (the other fields copied through)
template <int REC>
__global__ __launch_bounds__(256) void calib_points_kernel(CalibDev P, const float* __restrict__ in, float* __restrict__ out, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float r[REC];
#pragma unroll
    for (int k = 0; k < REC; k++) r[k] = in[(size_t)i * REC + k];
    float ox, oy;
    cal_point(P, r[0], r[1], ox, oy);
    r[0] = ox; r[1] = oy;
#pragma unroll
    for (int k = 0; k < REC; k++) out[(size_t)i * REC + k] = r[k];
}

// the monocular frame: the keypoints the extractor left on the device (their count too), and in the last block the four corners of
// Frame::ComputeImageBounds (Frame.cc:840-867), one lane each: corners[4][2] = (0, 0), (W, 0), (0, H), (W, H) undistorted; the host
// pairs them (comparisons only, :855-858)
__global__ __launch_bounds__(256) void calib_frame_kernel(CalibDev P, CalibDev PB, const float* __restrict__ kps, const int32_t* __restrict__ d_n,
                                                          int cap, float* __restrict__ un, float* __restrict__ corners, float fW, float fH)
{
    if (blockIdx.x == gridDim.x - 1) {
        if (threadIdx.x < 4 && PB.gate) {
            float ox, oy;
            cal_pinhole(PB, (threadIdx.x & 1) ? fW : 0.0f, (threadIdx.x & 2) ? fH : 0.0f, ox, oy);
            corners[2 * threadIdx.x] = ox; corners[2 * threadIdx.x + 1] = oy;
        }
        return;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    int n = *d_n;
    if (n > cap) n = cap;
    if (i >= n) return;
    float r[7];
#pragma unroll
    for (int k = 0; k < 7; k++) r[k] = kps[(size_t)i * 7 + k];
    float ox, oy;
    cal_point(P, r[0], r[1], ox, oy);
    r[0] = ox; r[1] = oy;
#pragma unroll
    for (int k = 0; k < 7; k++) un[(size_t)i * 7 + k] = r[k];
}

// MyCalibrator::generateUndistMaps* (:64-102): one thread per sensor pixel, straight into the context's interleaved maps
__global__ __launch_bounds__(256) void calib_maps_kernel(CalibDev P, int LW, int npix, float2* __restrict__ lut, float* __restrict__ mx,
                                                         float* __restrict__ my)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const int y = i / LW, x = i - y * LW;
    float ox, oy;
    cal_point(P, (float)x, (float)y, ox, oy);
    lut[i] = make_float2(ox, oy);
    if (mx) { mx[i] = ox; my[i] = oy; }
}

int calib_points_dev(eorb_ctx* c, const CalibDev& P, const float* d_in, float* d_out, int n, int rec_floats)
{
    if (n <= 0) return EORB_OK;
    ProfScope ps(c, "calib_points");
    const int grid = (n + 255) / 256;
    if (rec_floats == 7) calib_points_kernel<7><<<grid, 256, 0, c->stream>>>(P, d_in, d_out, n);
    else calib_points_kernel<2><<<grid, 256, 0, c->stream>>>(P, d_in, d_out, n);
    EORB_LAUNCH_CHECK(c, "calib_points_kernel");
    return EORB_OK;
}

int calib_frame_dev(eorb_ctx* c, const eorb_keypoint* d_kps, const int32_t* d_n, int cap, eorb_keypoint* d_un, float* d_bounds, int W, int H)
{
    ProfScope ps(c, "calib_frame");
    if (!c->calib_dev.gate && !c->calib_bounds.gate) return EORB_OK;       // (both gates closed: copies and 0, W, 0, H are the caller's)
    const int grid = (c->calib_dev.gate ? (cap + 255) / 256 : 0) + 1;      // (gate closed: the caller copies the keypoints itself)
    calib_frame_kernel<<<grid, 256, 0, c->stream>>>(c->calib_dev, c->calib_bounds, (const float*)d_kps, d_n, cap, (float*)d_un, d_bounds,
                                                    (float)W, (float)H);
    EORB_LAUNCH_CHECK(c, "calib_frame_kernel");
    return EORB_OK;
}

int calib_maps_dev(eorb_ctx* c, int LW, int LH, float* d_lut, float* d_mx, float* d_my)
{
    ProfScope ps(c, "calib_maps");
    const int npix = LW * LH;
    calib_maps_kernel<<<(npix + 255) / 256, 256, 0, c->stream>>>(c->calib_dev, LW, npix, (float2*)d_lut, d_mx, d_my);
    EORB_LAUNCH_CHECK(c, "calib_maps_kernel");
    return EORB_OK;
}

}  // namespace eorb

using namespace eorb;

extern "C" int eorb_set_calibration(eorb_ctx* c, const eorb_calib* q)
{
    if (!c) return EORB_E_ARG;
    if (!q) return set_err(c, EORB_E_ARG, "set_calibration: null calibration");
    if (q->model != 0 && q->model != 1) return set_err(c, EORB_E_ARG, "set_calibration: model %d", q->model);
    if (q->model == 0 ? (q->n_dist != 4 && q->n_dist != 5 && q->n_dist != 8) : q->n_dist != 4)
        return set_err(c, EORB_E_ARG, "set_calibration: %d distortion coefficients for model %d", q->n_dist, q->model);
    if (q->p_cols != 0 && q->p_cols != 3 && q->p_cols != 4) return set_err(c, EORB_E_ARG, "set_calibration: P with %d columns", q->p_cols);
    if (q->has_R != 0 && q->has_R != 1) return set_err(c, EORB_E_ARG, "set_calibration: has_R %d", q->has_R);
    CalibDev D{}, B{};
    D.model = q->model;
    D.gate = fabs((double)q->dist[0]) > 1e-9;                 // MyCalibrator::isDistorted (:46-50)
    D.fx = q->K[0]; D.fy = q->K[4]; D.cx = q->K[2]; D.cy = q->K[5];
    D.ifx = 1. / D.fx; D.ify = 1. / D.fy;
    for (int i = 0; i < q->n_dist; i++) D.k[i] = q->dist[i];
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (q->has_R) for (int i = 0; i < 9; i++) R[i] = q->R[i];
    if (q->p_cols) {
        double PP[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) PP[3 * i + j] = q->P[q->p_cols * i + j];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                // pinhole: cvMatMul's 3 x 3 case, a0*b0 + a1*b1 + a2*b2; fisheye: the Matx product, s = 0; s += a*b
                if (q->model == 0) D.RR[3 * i + j] = PP[3 * i] * R[j] + PP[3 * i + 1] * R[3 + j] + PP[3 * i + 2] * R[6 + j];
                else { double s = 0; for (int k = 0; k < 3; k++) s += PP[3 * i + k] * R[3 * k + j]; D.RR[3 * i + j] = s; }
            }
    } else
        for (int i = 0; i < 9; i++) D.RR[i] = R[i];
    // Frame::ComputeImageBounds (Frame.cc:840-867): cv::undistortPoints(mat, mat, K, mDistCoef, cv::Mat(), mK)
    B = D;
    B.model = 0;
    B.gate = q->dist[0] != 0.0;
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) B.RR[3 * i + j] = (double)q->K[3 * i] * I[j] + (double)q->K[3 * i + 1] * I[3 + j] + (double)q->K[3 * i + 2] * I[6 + j];
    c->calib = *q; c->calib_dev = D; c->calib_bounds = B; c->calib_set = true;
    return EORB_OK;
}
