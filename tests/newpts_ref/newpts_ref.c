/* newpts_ref.c -- CPU restatement of the per-match half of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:527-784) and of
 * Tracking::CreateNewMapPoints (src/Tracking.cc:3232-3408), strict IEEE (-ffp-contract=off), as the plain sequential double loop:
 * neighbours in order, matches idx1 ascending (src/ORBmatcher.cc:1206-1211), a map point on idx1 (:775) skips it in the later
 * neighbours, ratioFactor is a variable declared outside both loops (:464).  What eorb_slam_amd/csrc/newpts.hip must equal bit for bit;
 * the device resolves the two sequential rules in parallel, this file does not.  Test infrastructure: compiled into a temporary
 * directory by tests/newpts_ref/__init__.py, never loaded by the product.  The OpenCV 3.4.1 scalar paths are proj_ref.c's (gemm, dot,
 * norm); the cameras, the 4x4 Jacobi SVD and the float atan2 / cos are the oracle's, handed in as function pointers. */
#include "../proj_ref/proj_ref.c"

enum { NP_NEW, NP_NO_MATCH, NP_CLAIMED, NP_TYPE, NP_PARALLAX, NP_W_ZERO, NP_EMPTY_STEREO, NP_Z1, NP_Z2, NP_REPROJ1, NP_REPROJ2, NP_ZERO_DIST,
       NP_FAR, NP_SCALE, NP_NONFINITE, NP_NSTATUS };
enum { FORM_LOCAL_MAPPING, FORM_TRACKING };

typedef struct { const float* sigma2; const float* scale; const uint8_t* is_orb; const float* uright; const float* depth; const float* raw_xy; } npr_side;
typedef struct {                                                                                      /* = eorb_newpts_params */
    int form;
    const pr_view* views1; int nleft1; float mb1;
    const pr_view* views2; const int32_t* nleft2; const float* mb2;
    npr_side side1, side2;
    const float* level_scale; const float* level_sigma2; int nlevels;
    float rf_orb, rf_ak; int far_points; float th_far;
} npr_params;

typedef void (*npr_unproject_fn)(const pr_camera*, float, float, float*);
typedef void (*npr_svd4_fn)(const float*, double*, float*);
typedef float (*npr_atan2f_fn)(float, float);
typedef float (*npr_cosf_fn)(float);
static npr_unproject_fn g_unproject = 0;
static npr_svd4_fn g_svd4 = 0;
static npr_atan2f_fn g_atan2f = 0;
static npr_cosf_fn g_cosf = 0;
void npr_set_fns(npr_unproject_fn u, npr_svd4_fn s, npr_atan2f_fn a, npr_cosf_fn c) { g_unproject = u; g_svd4 = s; g_atan2f = a; g_cosf = c; }

/* "p*T.row(2) - T.row(j)": cv::subtract when p == 1, else addWeighted_<float, double>(row 2, p, row j, -1, 0) */
static void a_row(float p, const float* r2, const float* rj, float* out)
{
    for (int k = 0; k < 4; k++) {
        if ((double)p == 1.0) out[k] = r2[k] - rj[k];
        else out[k] = (float)((double)r2[k] * (double)p + (double)rj[k] * -1.0 + 0.0);
    }
}
/* Rwc*x: gemm without an added vector, (float)(t*1 + 0*0) */
static void rot3(const float* R, const float* x, float* out)
{
    for (int i = 0; i < 3; i++) {
        const float t = R[3 * i] * x[0] + R[3 * i + 1] * x[1] + R[3 * i + 2] * x[2];
        out[i] = (float)((double)t * 1.0 + 0.0 * 0.0);
    }
}
/* cos(2*atan2(mb/2, depth)) (:643): the float overloads */
static float cos_stereo(float mb, float depth) { return g_cosf(2 * g_atan2f(mb / 2, depth)); }

/* KeyFrame::UnprojectStereo (src/KeyFrame.cc:924-940); 0 = the empty Mat */
static int unproject_stereo(const pr_view* V, const float* Rwc, float u, float v, float z, float* x3d)
{
    if (z > 0) {
        const float invfx = 1.0f / V->cam.fx, invfy = 1.0f / V->cam.fy;
        const float x = (u - V->cam.cx) * z * invfx;
        const float y = (v - V->cam.cy) * z * invfy;
        const float xc[3] = {x, y, z};
        gemm3x1(Rwc, xc, V->Ow, x3d);
        return 1;
    }
    return 0;
}

typedef struct { int branch; float cosp, x3d[3]; } npr_aid;

/* the loop body for one pair under ratioFactor; every exit but the claim */
static int pair(const npr_params* P, const pr_keypoint* kps1, const pr_keypoint* kps2, int k, int row0, int idx1, int idx2, float ratioFactor, npr_aid* o)
{
    const int g2 = row0 + idx2;
    const int lm = P->form == FORM_LOCAL_MAPPING, twocam = lm && P->nleft1 >= 0;
    const int nv = twocam ? 2 : 1;
    o->branch = 0; o->cosp = 0.f; o->x3d[0] = o->x3d[1] = o->x3d[2] = 0.f;
    const int bRight1 = twocam && idx1 >= P->nleft1, bRight2 = twocam && idx2 >= P->nleft2[k];
    const pr_view* V1 = P->views1 + bRight1;
    const pr_view* V2 = P->views2 + (size_t)nv * k + bRight2;
    const pr_view* KF1 = P->views1;                               /* mpCurrentKeyFrame->fx .. mbf */
    const pr_view* KF2 = P->views2 + (size_t)nv * k;
    const pr_keypoint* kp1 = kps1 + idx1;
    const pr_keypoint* kp2 = kps2 + g2;
    const float kp1_ur = P->side1.uright ? P->side1.uright[idx1] : -1.f, kp2_ur = P->side2.uright ? P->side2.uright[g2] : -1.f;
    const int bStereo1 = !twocam && kp1_ur >= 0, bStereo2 = !twocam && kp2_ur >= 0;

    float xn1[3], xn2[3], Rwc1[9], Rwc2[9], ray1[3], ray2[3];
    if (lm) { g_unproject(&V1->cam, kp1->x, kp1->y, xn1); g_unproject(&V2->cam, kp2->x, kp2->y, xn2); }
    else {
        const float invfx1 = 1.0f / V1->cam.fx, invfy1 = 1.0f / V1->cam.fy, invfx2 = 1.0f / V2->cam.fx, invfy2 = 1.0f / V2->cam.fy;
        xn1[0] = (kp1->x - V1->cam.cx) * invfx1; xn1[1] = (kp1->y - V1->cam.cy) * invfy1; xn1[2] = 1.f;
        xn2[0] = (kp2->x - V2->cam.cx) * invfx2; xn2[1] = (kp2->y - V2->cam.cy) * invfy2; xn2[2] = 1.f;
    }
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { Rwc1[3 * i + j] = V1->R[3 * j + i]; Rwc2[3 * i + j] = V2->R[3 * j + i]; }
    rot3(Rwc1, xn1, ray1);
    rot3(Rwc2, xn2, ray2);
    const float cosParallaxRays = (float)(dot3(ray1, ray2) / (norm3(ray1) * norm3(ray2)));
    o->cosp = cosParallaxRays;

    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = cos_stereo(P->mb1, P->side1.depth[idx1]);
    else if (bStereo2) cosParallaxStereo2 = cos_stereo(P->mb2 ? P->mb2[k] : 0.f, P->side2.depth[g2]);
    cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;      /* std::min */

    float x3D[3];
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || cosParallaxRays < 0.9998)) {
        float Tcw1[12], Tcw2[12], A[16], Vt[16];
        double W[4];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) { Tcw1[4 * i + j] = V1->R[3 * i + j]; Tcw2[4 * i + j] = V2->R[3 * i + j]; }
            Tcw1[4 * i + 3] = V1->t[i]; Tcw2[4 * i + 3] = V2->t[i];
        }
        a_row(xn1[0], Tcw1 + 8, Tcw1 + 0, A + 0);
        a_row(xn1[1], Tcw1 + 8, Tcw1 + 4, A + 4);
        a_row(xn2[0], Tcw2 + 8, Tcw2 + 0, A + 8);
        a_row(xn2[1], Tcw2 + 8, Tcw2 + 4, A + 12);
        g_svd4(A, W, Vt);
        o->branch = 1;
        if (Vt[15] == 0) return NP_W_ZERO;
        const float sc = (float)(1. / (double)Vt[15]);           /* x3D.rowRange(0,3)/x3D.at<float>(3): the MatExpr fold */
        for (int i = 0; i < 3; i++) x3D[i] = Vt[12 + i] * sc + 0.0f;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        o->branch = 2;
        const float u = P->side1.raw_xy ? P->side1.raw_xy[2 * idx1] : kp1->x, v = P->side1.raw_xy ? P->side1.raw_xy[2 * idx1 + 1] : kp1->y;
        if (!unproject_stereo(V1, Rwc1, u, v, P->side1.depth[idx1], x3D)) return NP_EMPTY_STEREO;
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        o->branch = 3;
        const float u = P->side2.raw_xy ? P->side2.raw_xy[2 * (size_t)g2] : kp2->x, v = P->side2.raw_xy ? P->side2.raw_xy[2 * (size_t)g2 + 1] : kp2->y;
        if (!unproject_stereo(V2, Rwc2, u, v, P->side2.depth[g2], x3D)) return NP_EMPTY_STEREO;
    } else return NP_PARALLAX;
    if (!isfinite(x3D[0]) || !isfinite(x3D[1]) || !isfinite(x3D[2])) return NP_NONFINITE;

    float z1 = (float)(dot3(V1->R + 6, x3D) + (double)V1->t[2]);
    if (!isfinite(z1)) return NP_NONFINITE;
    if (z1 <= 0) return NP_Z1;
    float z2 = (float)(dot3(V2->R + 6, x3D) + (double)V2->t[2]);
    if (!isfinite(z2)) return NP_NONFINITE;
    if (z2 <= 0) return NP_Z2;

    const float sigmaSquare1 = P->side1.sigma2 ? P->side1.sigma2[idx1] : P->level_sigma2[kp1->octave];
    const float x1 = (float)(dot3(V1->R, x3D) + (double)V1->t[0]);
    const float y1 = (float)(dot3(V1->R + 3, x3D) + (double)V1->t[1]);
    const float invz1 = (float)(1.0 / (double)z1);
    if (!bStereo1) {
        float u1, v1;
        if (lm) { const float p[3] = {x1, y1, z1}; project(&V1->cam, p, &u1, &v1); }
        else { u1 = KF1->cam.fx * x1 * invz1 + KF1->cam.cx; v1 = KF1->cam.fy * y1 * invz1 + KF1->cam.cy; }
        const float errX1 = u1 - kp1->x, errY1 = v1 - kp1->y;
        const float e = errX1 * errX1 + errY1 * errY1;
        if (!isfinite(e)) return NP_NONFINITE;
        if (e > 5.991 * sigmaSquare1) return NP_REPROJ1;
    } else {
        const float u1 = KF1->cam.fx * x1 * invz1 + KF1->cam.cx;
        const float u1_r = u1 - KF1->mbf * invz1;
        const float v1 = KF1->cam.fy * y1 * invz1 + KF1->cam.cy;
        const float errX1 = u1 - kp1->x, errY1 = v1 - kp1->y, errX1_r = u1_r - kp1_ur;
        const float e = errX1 * errX1 + errY1 * errY1 + errX1_r * errX1_r;
        if (!isfinite(e)) return NP_NONFINITE;
        if (e > 7.8 * sigmaSquare1) return NP_REPROJ1;
    }

    const float sigmaSquare2 = P->side2.sigma2 ? P->side2.sigma2[g2] : P->level_sigma2[kp2->octave];
    const float x2 = (float)(dot3(V2->R, x3D) + (double)V2->t[0]);
    const float y2 = (float)(dot3(V2->R + 3, x3D) + (double)V2->t[1]);
    const float invz2 = (float)(1.0 / (double)z2);
    if (!bStereo2) {
        float u2, v2;
        if (lm) { const float p[3] = {x2, y2, z2}; project(&V2->cam, p, &u2, &v2); }
        else { u2 = KF2->cam.fx * x2 * invz2 + KF2->cam.cx; v2 = KF2->cam.fy * y2 * invz2 + KF2->cam.cy; }
        const float errX2 = u2 - kp2->x, errY2 = v2 - kp2->y;
        const float e = errX2 * errX2 + errY2 * errY2;
        if (!isfinite(e)) return NP_NONFINITE;
        if (e > 5.991 * sigmaSquare2) return NP_REPROJ2;
    } else {
        const float u2 = KF2->cam.fx * x2 * invz2 + KF2->cam.cx;
        const float u2_r = u2 - KF1->mbf * invz2;                  /* mpCurrentKeyFrame->mbf (:741), kept */
        const float v2 = KF2->cam.fy * y2 * invz2 + KF2->cam.cy;
        const float errX2 = u2 - kp2->x, errY2 = v2 - kp2->y, errX2_r = u2_r - kp2_ur;
        const float e = errX2 * errX2 + errY2 * errY2 + errX2_r * errX2_r;
        if (!isfinite(e)) return NP_NONFINITE;
        if (e > 7.8 * sigmaSquare2) return NP_REPROJ2;
    }

    const float normal1[3] = {x3D[0] - V1->Ow[0], x3D[1] - V1->Ow[1], x3D[2] - V1->Ow[2]};
    const float dist1 = (float)norm3(normal1);
    const float normal2[3] = {x3D[0] - V2->Ow[0], x3D[1] - V2->Ow[1], x3D[2] - V2->Ow[2]};
    const float dist2 = (float)norm3(normal2);
    if (!isfinite(dist1) || !isfinite(dist2)) return NP_NONFINITE;
    if (dist1 == 0 || dist2 == 0) return NP_ZERO_DIST;
    if (lm && P->far_points && (dist1 >= P->th_far || dist2 >= P->th_far)) return NP_FAR;
    const float ratioDist = dist2 / dist1;
    const float s1 = P->side1.scale ? P->side1.scale[idx1] : P->level_scale[kp1->octave];
    const float s2 = P->side2.scale ? P->side2.scale[g2] : P->level_scale[kp2->octave];
    const float ratioOctave = s1 / s2;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return NP_SCALE;
    o->x3d[0] = x3D[0]; o->x3d[1] = x3D[1]; o->x3d[2] = x3D[2];
    return NP_NEW;
}

static int is_orb(const uint8_t* a, long i) { return a ? a[i] != 0 : 1; }

/* the sequential loop.  status / n_new required; x3d, branch, cosp optional (K*n1 entries, zero where the loop did not get there) */
void npr_loop(const npr_params* P, const pr_keypoint* kps1, int n1, const pr_keypoint* kps2, const int32_t* kf_off, int K, const int32_t* match12,
              uint8_t* status, float* x3d, uint8_t* branch, float* cosp, int32_t* n_new, uint8_t* has_mp)
{
    float ratioFactor = P->rf_orb;                                 /* :464 */
    memset(has_mp, 0, (size_t)n1);
    for (int k = 0; k < K; k++) {
        n_new[k] = 0;
        for (int idx1 = 0; idx1 < n1; idx1++) {
            const size_t slot = (size_t)k * n1 + idx1;
            const int idx2 = match12[slot];
            if (x3d) x3d[3 * slot] = x3d[3 * slot + 1] = x3d[3 * slot + 2] = 0.f;
            if (branch) branch[slot] = 0;
            if (cosp) cosp[slot] = 0.f;
            if (idx2 < 0) { status[slot] = NP_NO_MATCH; continue; }
            if (has_mp[idx1]) { status[slot] = NP_CLAIMED; continue; }          /* the search left idx1 out: GetMapPoint(idx1) */
            const int o1 = is_orb(P->side1.is_orb, idx1), o2 = is_orb(P->side2.is_orb, (long)kf_off[k] + idx2);
            if (o1 != o2) { status[slot] = NP_TYPE; continue; }                 /* :542 */
            if (!o1 && !o2) ratioFactor = P->rf_ak;                               /* :545-546 */
            npr_aid a;
            const int st = pair(P, kps1, kps2, k, kf_off[k], idx1, idx2, ratioFactor, &a);
            status[slot] = (uint8_t)st;
            if (branch) branch[slot] = (uint8_t)a.branch;
            if (cosp) cosp[slot] = a.cosp;
            if (st == NP_NEW) {
                if (x3d) { x3d[3 * slot] = a.x3d[0]; x3d[3 * slot + 1] = a.x3d[1]; x3d[3 * slot + 2] = a.x3d[2]; }
                has_mp[idx1] = 1;                                                 /* AddMapPoint(pMP, idx1) :775 */
                n_new[k]++;
            }
        }
    }
}

/* every matched pair on its own, under both factors: st[2*slot] = the exit with the ORB factor, st[2*slot + 1] with the AKAZE factor,
 * ak[slot] = an AKAZE-AKAZE pair.  The inputs of the parallel resolution that tests/test_newpts_ref.py writes in numpy. */
void npr_pairs(const npr_params* P, const pr_keypoint* kps1, int n1, const pr_keypoint* kps2, const int32_t* kf_off, int K, const int32_t* match12,
               uint8_t* st, uint8_t* ak, float* x3d)
{
    for (int k = 0; k < K; k++)
        for (int idx1 = 0; idx1 < n1; idx1++) {
            const size_t slot = (size_t)k * n1 + idx1;
            const int idx2 = match12[slot];
            ak[slot] = 0;
            if (x3d) x3d[3 * slot] = x3d[3 * slot + 1] = x3d[3 * slot + 2] = 0.f;
            if (idx2 < 0) { st[2 * slot] = st[2 * slot + 1] = NP_NO_MATCH; continue; }
            const int o1 = is_orb(P->side1.is_orb, idx1), o2 = is_orb(P->side2.is_orb, (long)kf_off[k] + idx2);
            if (o1 != o2) { st[2 * slot] = st[2 * slot + 1] = NP_TYPE; continue; }
            ak[slot] = !o1;
            npr_aid a, b;
            st[2 * slot] = (uint8_t)pair(P, kps1, kps2, k, kf_off[k], idx1, idx2, P->rf_orb, &a);
            st[2 * slot + 1] = (uint8_t)pair(P, kps1, kps2, k, kf_off[k], idx1, idx2, P->rf_ak, &b);
            if (x3d && (st[2 * slot] == NP_NEW || st[2 * slot + 1] == NP_NEW)) {
                const npr_aid* w = st[2 * slot] == NP_NEW ? &a : &b;
                x3d[3 * slot] = w->x3d[0]; x3d[3 * slot + 1] = w->x3d[1]; x3d[3 * slot + 2] = w->x3d[2];
            }
        }
}
