/* calib_ref.c -- strict-IEEE, single-threaded CPU restatement of MyCalibrator (src/Utils/MyCalibrator.cpp of the reference) over
 * cv::undistortPoints and cv::fisheye::undistortPoints of OpenCV 3.4.1 (scalar paths), and of Frame::ComputeImageBounds
 * (src/Frame.cc:840-867).  Test infrastructure only: the product never loads it.  Build: -O2 -ffp-contract=off -fno-fast-math.
 * The OpenCV arithmetic is restated from the published 3.4.1 algorithms and is pinned by nothing the reference ships: every choice is
 * listed as "unpinned" in DESIGN.md section 2. */
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct cr_calib {       /* = eorb_calib of include/eorb_fe.h */
    int   model;
    float K[9];
    float dist[8];
    int   n_dist;
    float R[9];  int has_R;
    float P[12]; int p_cols;
} cr_calib;

typedef struct { float x, y, size, angle, response; int32_t octave, class_id; } cr_keypoint;     /* cv::KeyPoint, 28 B */

/* ---- fdlibm double tan: k_tan.c (__kernel_tan), s_tan.c, and the |x| < 3 pi / 4 branch of e_rem_pio2.c -------------------------- */
static double lo0(double v) { uint64_t b; memcpy(&b, &v, 8); b &= 0xffffffff00000000ull; memcpy(&v, &b, 8); return v; }

static double k_tan(double x, double y, int iy)
{
    static const double T[13] = {
        3.33333333333334091986e-01, 1.33333333333201242699e-01, 5.39682539762260521377e-02, 2.18694882948595424599e-02,
        8.86323982359930005737e-03, 3.59207910759131235356e-03, 1.45620945432529025516e-03, 5.88041240820264096874e-04,
        2.46463134818469906812e-04, 7.81794442939557092300e-05, 7.14072491382608190305e-05, -1.85586374855275456654e-05,
        2.59073051863633712884e-05};
    static const double pio4 = 7.85398163397448278999e-01, pio4lo = 3.06161699786838301793e-17;
    uint64_t xb; memcpy(&xb, &x, 8);
    const int32_t hx = (int32_t)(xb >> 32), ix = hx & 0x7fffffff;
    const uint32_t lx = (uint32_t)xb;
    double z, r, v, w, s, a, t;
    if (ix < 0x3e300000) {                                    /* |x| < 2^-28 (k_tan.c) */
        if ((int)x == 0) {
            if (((uint32_t)ix | lx | (uint32_t)(iy + 1)) == 0) return 1.0 / fabs(x);
            if (iy == 1) return x;
            z = w = x + y;
            z = lo0(z);
            v = y - (z - x);
            t = a = -1.0 / w;
            t = lo0(t);
            s = 1.0 + t * z;
            return t + a * (s + t * v);
        }
    }
    if (ix >= 0x3FE59428) {                                   /* |x| >= 0.6744 */
        if (hx < 0) { x = -x; y = -y; }
        z = pio4 - x;
        w = pio4lo - y;
        x = z + w; y = 0.0;
    }
    z = x * x;
    w = z * z;
    r = T[1] + w * (T[3] + w * (T[5] + w * (T[7] + w * (T[9] + w * T[11]))));
    v = z * (T[2] + w * (T[4] + w * (T[6] + w * (T[8] + w * (T[10] + w * T[12])))));
    s = z * x;
    r = y + z * (s * (r + v) + y);
    r += T[0] * s;
    w = x + r;
    if (ix >= 0x3FE59428) {
        v = (double)iy;
        return (double)(1 - ((hx >> 30) & 2)) * (v - 2.0 * (x - (w * w / (w + v) - r)));
    }
    if (iy == 1) return w;
    z = lo0(w);                                               /* -1 / (x + r) accurately */
    v = r - (z - x);
    t = a = -1.0 / w;
    t = lo0(t);
    s = 1.0 + t * z;
    return t + a * (s + t * v);
}

/* s_tan.c; the argument of cv::fisheye::undistortPoints lies in (0, pi/2] for every sane calibration (theta_d is clamped), which
 * the n = 1 branch of e_rem_pio2.c covers exactly; beyond 3 pi / 4 the plain two-term reduction (not fdlibm's iteration) */
double cr_tan(double x)
{
    static const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00, pio2_1t = 6.07710050650619224932e-11,
                        pio2_2 = 6.07710050630396597660e-11, pio2_2t = 2.02226624879595063154e-21;
    uint64_t xb; memcpy(&xb, &x, 8);
    const int32_t hx = (int32_t)(xb >> 32), ix = hx & 0x7fffffff;
    double t, a, b, z;
    int n;
    if (ix <= 0x3fe921fb) return k_tan(x, 0.0, 1);
    if (ix >= 0x41d00000) return (x - x) / (x - x);           /* inf, NaN (fdlibm: x - x) and, here, |x| >= 2^30: NaN */
    t = fabs(x);
    if (ix < 0x4002d97c) {
        z = t - pio2_1;
        if (ix != 0x3ff921fb) { a = z - pio2_1t; b = (z - a) - pio2_1t; }
        else { z -= pio2_2; a = z - pio2_2t; b = (z - a) - pio2_2t; }
        n = 1;
    } else {
        double fn, r, w;
        n = (int)(t * invpio2 + 0.5);
        fn = (double)n;
        r = t - fn * pio2_1;
        w = fn * pio2_1t;
        a = r - w;
        b = (r - a) - w;
    }
    if (hx < 0) { a = -a; b = -b; n = -n; }
    return k_tan(a, b, 1 - ((n & 1) << 1));
}

void cr_tan_n(const double* x, long n, double* out) { for (long i = 0; i < n; i++) out[i] = cr_tan(x[i]); }

/* ---- the widened calibration ----------------------------------------------------------------------------------------------------- */
typedef struct { int model, gate; double fx, fy, cx, cy, ifx, ify, k[12], RR[9]; } cr_dev;

int cr_is_distorted(const cr_calib* q) { return fabs((double)q->dist[0]) > 1e-9; }      /* MyCalibrator::isDistorted :46-50 */

int cr_valid(const cr_calib* q)
{
    if (q->model != 0 && q->model != 1) return 0;
    if (q->model == 0 ? (q->n_dist != 4 && q->n_dist != 5 && q->n_dist != 8) : q->n_dist != 4) return 0;
    if (q->p_cols != 0 && q->p_cols != 3 && q->p_cols != 4) return 0;
    return q->has_R == 0 || q->has_R == 1;
}

static void widen(const cr_calib* q, cr_dev* D)
{
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, PP[9];
    int i, j, k;
    memset(D, 0, sizeof *D);
    D->model = q->model;
    D->gate = cr_is_distorted(q);
    D->fx = q->K[0]; D->fy = q->K[4]; D->cx = q->K[2]; D->cy = q->K[5];
    D->ifx = 1. / D->fx; D->ify = 1. / D->fy;                 /* cvUndistortPoints: ifx = 1./fx */
    for (i = 0; i < q->n_dist; i++) D->k[i] = q->dist[i];
    if (q->has_R) for (i = 0; i < 9; i++) R[i] = q->R[i];
    if (q->p_cols) {
        for (i = 0; i < 3; i++) for (j = 0; j < 3; j++) PP[3 * i + j] = q->P[q->p_cols * i + j];
        for (i = 0; i < 3; i++)
            for (j = 0; j < 3; j++) {
                if (q->model == 0)                            /* cvMatMul(&_PP, &_RR, &_RR): the 3 x 3 case of gemm */
                    D->RR[3 * i + j] = PP[3 * i] * R[j] + PP[3 * i + 1] * R[3 + j] + PP[3 * i + 2] * R[6 + j];
                else {                                        /* RR = PP * RR: Matx product, s = 0; s += a * b */
                    double s = 0;
                    for (k = 0; k < 3; k++) s += PP[3 * i + k] * R[3 * k + j];
                    D->RR[3 * i + j] = s;
                }
            }
    } else
        for (i = 0; i < 9; i++) D->RR[i] = R[i];
}

/* cvUndistortPoints (imgproc/src/undistort.cpp, 3.4.1), one CV_32FC2 point */
static void pinhole(const cr_dev* P, float sx, float sy, float* ox, float* oy)
{
    const double* k = P->k;
    const double* RR = P->RR;
    double x = ((double)sx - P->cx) * P->ifx, y = ((double)sy - P->cy) * P->ify;
    /* invMatTilt * Vec3d(x, y, 1), invMatTilt = the identity of the default tilt terms; invProj = 1./1 */
    const double u0 = ((0.0 + 1.0 * x) + 0.0 * y) + 0.0 * 1.0;
    const double u1 = ((0.0 + 0.0 * x) + 1.0 * y) + 0.0 * 1.0;
    const double u2 = ((0.0 + 0.0 * x) + 0.0 * y) + 1.0 * 1.0;
    const double invProj = u2 != 0.0 ? 1. / u2 : 1;
    double x0, y0, xx, yy, ww;
    int j;
    x0 = x = invProj * u0; y0 = y = invProj * u1;
    for (j = 0; j < 5; j++) {                                 /* TermCriteria(COUNT, 5, 0.01) */
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2;
        const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    xx = RR[0] * x + RR[1] * y + RR[2];
    yy = RR[3] * x + RR[4] * y + RR[5];
    ww = 1. / (RR[6] * x + RR[7] * y + RR[8]);
    *ox = (float)(xx * ww);
    *oy = (float)(yy * ww);
}

/* cv::fisheye::undistortPoints (calib3d/src/fisheye.cpp, 3.4.1), one CV_32FC2 point; tan_fn: cr_tan, or the host libm's for the
 * comparison DESIGN.md records */
static void fisheye(const cr_dev* P, float sx, float sy, float* ox, float* oy, double (*tan_fn)(double))
{
    const double* RR = P->RR;
    const double pwx = ((double)sx - P->cx) / P->fx, pwy = ((double)sy - P->cy) / P->fy;
    const double hpi = 3.1415926535897932384626433832795 / 2.;
    double scale = 1.0, pux, puy, p0, p1, p2;
    double theta_d = sqrt(pwx * pwx + pwy * pwy);
    int j;
    theta_d = (-hpi < theta_d) ? theta_d : -hpi;              /* std::max(-CV_PI/2., theta_d) */
    theta_d = (hpi < theta_d) ? hpi : theta_d;                /* std::min(.., CV_PI/2.) */
    if (theta_d > 1e-8) {
        double theta = theta_d;
        for (j = 0; j < 10; j++) {
            const double theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta6 * theta2;
            theta = theta_d / (1 + P->k[0] * theta2 + P->k[1] * theta4 + P->k[2] * theta6 + P->k[3] * theta8);
        }
        scale = tan_fn(theta) / theta_d;
    }
    pux = pwx * scale; puy = pwy * scale;
    p0 = ((0.0 + RR[0] * pux) + RR[1] * puy) + RR[2] * 1.0;
    p1 = ((0.0 + RR[3] * pux) + RR[4] * puy) + RR[5] * 1.0;
    p2 = ((0.0 + RR[6] * pux) + RR[7] * puy) + RR[8] * 1.0;
    *ox = (float)(p0 / p2);
    *oy = (float)(p1 / p2);
}

static void point(const cr_dev* D, float sx, float sy, float* ox, float* oy, double (*tan_fn)(double))
{
    if (!D->gate) { *ox = sx; *oy = sy; return; }             /* dstPt = srcPt (:122-126, :144-148) */
    if (D->model == 0) pinhole(D, sx, sy, ox, oy); else fisheye(D, sx, sy, ox, oy, tan_fn);
}

/* MyCalibrator::undistPointPinhole / undistPointFishEye (:119-156) over n points; host_tan != 0: std::tan of the host libm */
void cr_undistort_points(const cr_calib* q, const float* xy, long n, float* out, int host_tan)
{
    cr_dev D;
    long i;
    widen(q, &D);
    for (i = 0; i < n; i++) point(&D, xy[2 * i], xy[2 * i + 1], &out[2 * i], &out[2 * i + 1], host_tan ? tan : cr_tan);
}

/* the two point functions without the gate (cv::undistortPoints / cv::fisheye::undistortPoints themselves) */
void cr_cv_undistort_points(const cr_calib* q, const float* xy, long n, float* out)
{
    cr_dev D;
    long i;
    widen(q, &D);
    D.gate = 1;
    for (i = 0; i < n; i++) point(&D, xy[2 * i], xy[2 * i + 1], &out[2 * i], &out[2 * i + 1], cr_tan);
}

/* MyCalibrator::undistKeyPointsPinhole / FishEye (:198-283): empty input leaves the output alone (:202-205) */
void cr_undistort_keypoints(const cr_calib* q, const cr_keypoint* in, long n, cr_keypoint* out)
{
    cr_dev D;
    long i;
    if (n <= 0) return;
    widen(q, &D);
    if (!D.gate) { memmove(out, in, sizeof(cr_keypoint) * (size_t)n); return; }      /* vUndistKPts = vDistKPts (:206-210) */
    for (i = 0; i < n; i++) {
        cr_keypoint kp = in[i];
        point(&D, in[i].x, in[i].y, &kp.x, &kp.y, cr_tan);
        out[i] = kp;
    }
}

/* MyCalibrator::generateUndistMapsPinhole / FishEye (:64-102): map[y][x] = undistPoint((float)x, (float)y) */
void cr_generate_maps(const cr_calib* q, int LW, int LH, float* mapX, float* mapY, int host_tan)
{
    cr_dev D;
    int x, y;
    widen(q, &D);
    for (y = 0; y < LH; y++)
        for (x = 0; x < LW; x++)
            point(&D, (float)x, (float)y, &mapX[(size_t)y * LW + x], &mapY[(size_t)y * LW + x], host_tan ? tan : cr_tan);
}

/* Frame::ComputeImageBounds (src/Frame.cc:840-867): gate dist[0] != 0.0 (:842); cv::undistortPoints(corners, K, mDistCoef, cv::Mat(), mK)
 * (:851) whatever the camera model; bounds = mnMinX, mnMaxX, mnMinY, mnMaxY */
void cr_image_bounds(const cr_calib* q, int W, int H, float bounds[4])
{
    cr_calib b = *q;
    cr_dev D;
    float cx[4], cy[4];
    if (!(q->dist[0] != 0.0)) { bounds[0] = 0.0f; bounds[1] = (float)W; bounds[2] = 0.0f; bounds[3] = (float)H; return; }
    b.model = 0; b.has_R = 0; b.p_cols = 3;
    memcpy(b.P, q->K, sizeof(float) * 9);
    widen(&b, &D);
    pinhole(&D, 0.0f, 0.0f, &cx[0], &cy[0]);
    pinhole(&D, (float)W, 0.0f, &cx[1], &cy[1]);
    pinhole(&D, 0.0f, (float)H, &cx[2], &cy[2]);
    pinhole(&D, (float)W, (float)H, &cx[3], &cy[3]);
    bounds[0] = (cx[2] < cx[0]) ? cx[2] : cx[0];              /* min(mat(0,0), mat(2,0)): std::min(a, b) = b < a ? b : a */
    bounds[1] = (cx[1] < cx[3]) ? cx[3] : cx[1];              /* max(mat(1,0), mat(3,0)): std::max(a, b) = a < b ? b : a */
    bounds[2] = (cy[1] < cy[0]) ? cy[1] : cy[0];              /* min(mat(0,1), mat(1,1)) */
    bounds[3] = (cy[2] < cy[3]) ? cy[3] : cy[2];              /* max(mat(2,1), mat(3,1)) */
}
