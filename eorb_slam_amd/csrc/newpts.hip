// newpts.hip -- the per-match half of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:527-784) and of
// Tracking::CreateNewMapPoints (src/Tracking.cc:3232-3408) for the K neighbours of one keyframe.  Same fixed IEEE operation order
// as the rest (-ffp-contract=off); the OpenCV 3.4.1 primitives and the cameras are kb8_dev.h's, the float atan2 / cos dev_math.h's.
// The CPU restatement is tests/newpts_ref/newpts_ref.c (the sequential double loop); DESIGN.md section 2 lists each reading.
//
// eorb_new_map_points is two launches:
//   np_pair_kernel   a workgroup takes kNpSlotsPerBlock slots of match12, compacts the matched ones into LDS (most slots hold no
//                    match and the SVD is long, so the geometry runs on full wavefronts) and evaluates each pair once: acceptance
//                    depends on nothing but the pair.  Only the scale test (:766) reads ratioFactor, so both outcomes are kept.
//                    p*, the position k*n1 + idx1 where the sequential loop overwrites ratioFactor, is the smallest position of an
//                    AKAZE-AKAZE pair: a minimum over positions.  (The loop reaches a pair unless its idx1 was claimed by an earlier
//                    neighbour; the pair that claimed a non-ORB idx1 passed the type gate, so it is an AKAZE-AKAZE pair at a smaller
//                    position.  The smallest such position is therefore always reached: DESIGN.md section 2.)
//   np_claim_kernel  one thread per idx1 walks k with the outcome each position has (ORB factor before p*, AKAZE from p* on):
//                    the first accepted pair wins, later matches are EORB_NP_CLAIMED; n_new[k] counts.
// The SVD is kb8_dev.h's cv_svd4_vt3 on registers: its loops are unrolled over constant indices, and the compiler's resource report
// for np_pair_kernel shows no scratch (DESIGN.md section 7m has the figures).
#include <hip/hip_runtime.h>
#include "newpts.h"

namespace eorb {

struct NpPair { int st_orb, st_ak, ak, branch; float x3d[3], cosp; };

__device__ __forceinline__ bool np_finite(float v) { return fabsf(v) <= 3.40282347e+38f; }

// cos(2*atan2(mb/2, depth)) (:643): float overloads (std::atan2(float, float), int*float, std::cos(float))
__device__ __forceinline__ float np_cos_stereo(float mb, float depth)
{
    const float ang = 2 * dev_atan2f(mb / 2, depth);
    float sn, cs;
    dev_sincosf(ang, &sn, &cs);
    return cs;
}

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:924-940): false = the empty Mat
__device__ __forceinline__ bool np_unproject_stereo(const NpView& V, const float* Rwc, float u, float v, float z, float* x3d)
{
    if (!(z > 0)) return false;
    const float invfx = 1.0f / V.cam.fx, invfy = 1.0f / V.cam.fy;
    const float xc[3] = {(u - V.cam.cx) * z * invfx, (v - V.cam.cy) * z * invfy, z};
    cv_gemm3x1(Rwc, xc, V.Ow, 1.0, x3d);                       // Twc.rowRange(0,3).colRange(0,3)*x3Dc + Twc.rowRange(0,3).col(3)
    return true;
}

// one chi-square gate (:698-748): 0 passes, else the exit (`fail`, or EORB_NP_NONFINITE)
__device__ __forceinline__ int np_reproj(const NpArgs& a, const NpView& V, const NpView& V0, bool stereo, const float* x3d, float z, float kx, float ky,
                                         float ur, float mbf, float sigma2, int fail)
{
    const float x = (float)(cv_dot3(V.R, x3d) + (double)V.t[0]);
    const float y = (float)(cv_dot3(V.R + 3, x3d) + (double)V.t[1]);
    const float invz = (float)(1.0 / (double)z);
    float e;
    double lim;
    if (!stereo) {
        float u, v;
        if (a.form == EORB_NEWPTS_LOCAL_MAPPING) { const float p[3] = {x, y, z}; cam_project_f(V.cam, p, u, v); }
        else { u = V0.cam.fx * x * invz + V0.cam.cx; v = V0.cam.fy * y * invz + V0.cam.cy; }
        const float ex = u - kx, ey = v - ky;
        e = ex * ex + ey * ey;
        lim = 5.991 * (double)sigma2;
    } else {
        const float u = V0.cam.fx * x * invz + V0.cam.cx;
        const float u_r = u - mbf * invz;
        const float v = V0.cam.fy * y * invz + V0.cam.cy;
        const float ex = u - kx, ey = v - ky, er = u_r - ur;
        e = ex * ex + ey * ey + er * er;
        lim = 7.8 * (double)sigma2;
    }
    if (!np_finite(e)) return EORB_NP_NONFINITE;
    return (double)e > lim ? fail : 0;
}

// the loop body for one pair (:531-767), every exit but the claim
__device__ void np_pair(const NpArgs& a, const NpKf& kf, int idx1, int idx2, NpPair& o)
{
    o.st_orb = o.st_ak = EORB_NP_TYPE; o.ak = 0; o.branch = EORB_NP_BRANCH_NONE; o.cosp = 0.f;
    o.x3d[0] = o.x3d[1] = o.x3d[2] = 0.f;
    const int g2 = kf.row0 + idx2;
    const bool orb1 = a.s1.is_orb ? a.s1.is_orb[idx1] != 0 : true, orb2 = a.s2.is_orb ? a.s2.is_orb[g2] != 0 : true;
    if (orb1 != orb2) return;
    o.ak = !orb1;
    const bool lm = a.form == EORB_NEWPTS_LOCAL_MAPPING, twocam = lm && a.nleft1 >= 0;
    const int r1 = twocam && idx1 >= a.nleft1, r2 = twocam && idx2 >= kf.nleft2;
    const NpView& V1 = a.v1[r1];
    const NpView& V2 = kf.v[r2];
    const float k1x = a.kps1[idx1].x, k1y = a.kps1[idx1].y, k2x = a.kps2[g2].x, k2y = a.kps2[g2].y;
    const float ur1 = a.s1.uright ? a.s1.uright[idx1] : -1.f, ur2 = a.s2.uright ? a.s2.uright[g2] : -1.f;
    const bool st1 = !twocam && ur1 >= 0, st2 = !twocam && ur2 >= 0;

    float xn1[3], xn2[3], Rwc1[9], Rwc2[9], ray1[3], ray2[3];
    if (lm) {
        cam_unproject(V1.cam, k1x, k1y, xn1[0], xn1[1]);
        cam_unproject(V2.cam, k2x, k2y, xn2[0], xn2[1]);
    } else {
        xn1[0] = (k1x - V1.cam.cx) * (1.0f / V1.cam.fx); xn1[1] = (k1y - V1.cam.cy) * (1.0f / V1.cam.fy);
        xn2[0] = (k2x - V2.cam.cx) * (1.0f / V2.cam.fx); xn2[1] = (k2y - V2.cam.cy) * (1.0f / V2.cam.fy);
    }
    xn1[2] = xn2[2] = 1.f;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { Rwc1[3 * i + j] = V1.R[3 * j + i]; Rwc2[3 * i + j] = V2.R[3 * j + i]; }
    cv_gemm3x1(Rwc1, xn1, nullptr, 1.0, ray1);
    cv_gemm3x1(Rwc2, xn2, nullptr, 1.0, ray2);
    const float cosr = (float)(cv_dot3(ray1, ray2) / (cv_norm3(ray1) * cv_norm3(ray2)));
    o.cosp = cosr;

    float cs = cosr + 1, cs1 = cs, cs2 = cs;
    if (st1) cs1 = np_cos_stereo(a.mb1, a.s1.depth[idx1]);
    else if (st2) cs2 = np_cos_stereo(kf.mb, a.s2.depth[g2]);
    cs = cs2 < cs1 ? cs2 : cs1;                                   // std::min(cs1, cs2)

    float x3d[3];
    if (cosr < cs && cosr > 0 && (st1 || st2 || (double)cosr < 0.9998)) {
        float T1[12], T2[12], A[16], v3[4];
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) { T1[4 * i + j] = V1.R[3 * i + j]; T2[4 * i + j] = V2.R[3 * i + j]; }
            T1[4 * i + 3] = V1.t[i]; T2[4 * i + 3] = V2.t[i];
        }
        cv_a_row(xn1[0], T1 + 8, T1 + 0, A + 0);
        cv_a_row(xn1[1], T1 + 8, T1 + 4, A + 4);
        cv_a_row(xn2[0], T2 + 8, T2 + 0, A + 8);
        cv_a_row(xn2[1], T2 + 8, T2 + 4, A + 12);
        cv_svd4_vt3(A, v3);
        o.branch = EORB_NP_BRANCH_DLT;
        if (v3[3] == 0) { o.st_orb = o.st_ak = EORB_NP_W_ZERO; return; }
        const float sc = (float)(1. / (double)v3[3]);             // the MatExpr fold of x3D.rowRange(0,3)/x3D.at<float>(3)
#pragma unroll
        for (int i = 0; i < 3; i++) x3d[i] = v3[i] * sc + 0.0f;
    } else if (st1 && cs1 < cs2) {
        o.branch = EORB_NP_BRANCH_STEREO1;
        const float u = a.s1.raw_xy ? a.s1.raw_xy[2 * idx1] : k1x, v = a.s1.raw_xy ? a.s1.raw_xy[2 * idx1 + 1] : k1y;
        if (!np_unproject_stereo(V1, Rwc1, u, v, a.s1.depth[idx1], x3d)) { o.st_orb = o.st_ak = EORB_NP_EMPTY_STEREO; return; }
    } else if (st2 && cs2 < cs1) {
        o.branch = EORB_NP_BRANCH_STEREO2;
        const float u = a.s2.raw_xy ? a.s2.raw_xy[2 * (size_t)g2] : k2x, v = a.s2.raw_xy ? a.s2.raw_xy[2 * (size_t)g2 + 1] : k2y;
        if (!np_unproject_stereo(V2, Rwc2, u, v, a.s2.depth[g2], x3d)) { o.st_orb = o.st_ak = EORB_NP_EMPTY_STEREO; return; }
    } else { o.st_orb = o.st_ak = EORB_NP_PARALLAX; return; }
    if (!np_finite(x3d[0]) || !np_finite(x3d[1]) || !np_finite(x3d[2])) { o.st_orb = o.st_ak = EORB_NP_NONFINITE; return; }

    const float z1 = (float)(cv_dot3(V1.R + 6, x3d) + (double)V1.t[2]);
    if (!np_finite(z1)) { o.st_orb = o.st_ak = EORB_NP_NONFINITE; return; }
    if (z1 <= 0) { o.st_orb = o.st_ak = EORB_NP_Z1; return; }
    const float z2 = (float)(cv_dot3(V2.R + 6, x3d) + (double)V2.t[2]);
    if (!np_finite(z2)) { o.st_orb = o.st_ak = EORB_NP_NONFINITE; return; }
    if (z2 <= 0) { o.st_orb = o.st_ak = EORB_NP_Z2; return; }

    const int oc1 = a.kps1[idx1].octave, oc2 = a.kps2[g2].octave;
    const float sg1 = a.s1.sigma2 ? a.s1.sigma2[idx1] : a.level_sigma2[oc1], sg2 = a.s2.sigma2 ? a.s2.sigma2[g2] : a.level_sigma2[oc2];
    const float mbf1 = a.v1[0].mbf;                               // keyframe 2's stereo gate reads mpCurrentKeyFrame->mbf too (:741)
    int rc = np_reproj(a, V1, a.v1[0], st1, x3d, z1, k1x, k1y, ur1, mbf1, sg1, EORB_NP_REPROJ1);
    if (rc) { o.st_orb = o.st_ak = rc; return; }
    rc = np_reproj(a, V2, kf.v[0], st2, x3d, z2, k2x, k2y, ur2, mbf1, sg2, EORB_NP_REPROJ2);
    if (rc) { o.st_orb = o.st_ak = rc; return; }

    const float n1v[3] = {x3d[0] - V1.Ow[0], x3d[1] - V1.Ow[1], x3d[2] - V1.Ow[2]};
    const float n2v[3] = {x3d[0] - V2.Ow[0], x3d[1] - V2.Ow[1], x3d[2] - V2.Ow[2]};
    const float dist1 = (float)cv_norm3(n1v), dist2 = (float)cv_norm3(n2v);
    if (!np_finite(dist1) || !np_finite(dist2)) { o.st_orb = o.st_ak = EORB_NP_NONFINITE; return; }
    if (dist1 == 0 || dist2 == 0) { o.st_orb = o.st_ak = EORB_NP_ZERO_DIST; return; }
    if (lm && a.far_points && (dist1 >= a.th_far || dist2 >= a.th_far)) { o.st_orb = o.st_ak = EORB_NP_FAR; return; }
    const float ratioDist = dist2 / dist1;
    const float sc1 = a.s1.scale ? a.s1.scale[idx1] : a.level_scale[oc1], sc2 = a.s2.scale ? a.s2.scale[g2] : a.level_scale[oc2];
    const float ratioOctave = sc1 / sc2;
    o.st_orb = (ratioDist * a.rf_orb < ratioOctave || ratioDist > ratioOctave * a.rf_orb) ? EORB_NP_SCALE : EORB_NP_NEW;
    o.st_ak = (ratioDist * a.rf_ak < ratioOctave || ratioDist > ratioOctave * a.rf_ak) ? EORB_NP_SCALE : EORB_NP_NEW;
    o.x3d[0] = x3d[0]; o.x3d[1] = x3d[1]; o.x3d[2] = x3d[2];
}

__global__ void __launch_bounds__(256) np_pair_kernel(NpArgs a)
{
    __shared__ int32_t s_slot[kNpSlotsPerBlock];
    __shared__ int s_n;
    const int64_t total = (int64_t)a.K * a.n1, base = (int64_t)blockIdx.x * kNpSlotsPerBlock;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < kNpSlotsPerBlock; i += 256) {
        const int64_t slot = base + i;
        if (slot >= total) break;
        const int k = (int)(slot / a.n1);
        const int32_t m = a.match12[slot];
        if (m >= 0 && m < a.kf[k].nrows) s_slot[atomicAdd(&s_n, 1)] = i;
        else { a.tmp[2 * slot] = EORB_NP_NO_MATCH; a.tmp[2 * slot + 1] = EORB_NP_NO_MATCH; }
    }
    __syncthreads();
    const int n = s_n;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int64_t slot = base + s_slot[i];
        const int k = (int)(slot / a.n1), idx1 = (int)(slot - (int64_t)k * a.n1);
        NpPair o;
        np_pair(a, a.kf[k], idx1, a.match12[slot], o);
        a.tmp[2 * slot] = (uint8_t)o.st_orb;
        a.tmp[2 * slot + 1] = (uint8_t)o.st_ak;
        if (o.ak) atomicMin(a.pstar, (int32_t)slot);
        if (a.x3d) { a.x3d[3 * slot] = o.x3d[0]; a.x3d[3 * slot + 1] = o.x3d[1]; a.x3d[3 * slot + 2] = o.x3d[2]; }
        if (a.branch) a.branch[slot] = (uint8_t)o.branch;
        if (a.cosp) a.cosp[slot] = o.cosp;
    }
}

__global__ void __launch_bounds__(256) np_claim_kernel(NpArgs a)
{
    const int idx1 = blockIdx.x * 256 + threadIdx.x;
    if (idx1 >= a.n1) return;
    const int32_t pstar = *a.pstar;
    bool claimed = false;
    for (int k = 0; k < a.K; k++) {
        const int64_t slot = (int64_t)k * a.n1 + idx1;
        int st = slot < pstar ? a.tmp[2 * slot] : a.tmp[2 * slot + 1];
        if (st == EORB_NP_NO_MATCH) { a.status[slot] = EORB_NP_NO_MATCH; continue; }
        if (claimed) {
            st = EORB_NP_CLAIMED;
            if (a.branch) a.branch[slot] = 0;
            if (a.cosp) a.cosp[slot] = 0.f;
        } else if (st == EORB_NP_NEW) { claimed = true; atomicAdd(a.n_new + k, 1); }
        if (st != EORB_NP_NEW && a.x3d) { a.x3d[3 * slot] = 0.f; a.x3d[3 * slot + 1] = 0.f; a.x3d[3 * slot + 2] = 0.f; }
        a.status[slot] = (uint8_t)st;
    }
}

int new_map_points_dev(eorb_ctx* c, const NpArgs& a)
{
    const int64_t total = (int64_t)a.K * a.n1;
    { ProfScope ps(c, "newpts_pair");
      np_pair_kernel<<<(unsigned)((total + kNpSlotsPerBlock - 1) / kNpSlotsPerBlock), 256, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "np_pair_kernel"); }
    { ProfScope ps(c, "newpts_claim");
      np_claim_kernel<<<(a.n1 + 255) / 256, 256, 0, c->stream>>>(a);
      EORB_LAUNCH_CHECK(c, "np_claim_kernel"); }
    return EORB_OK;
}

}  // namespace eorb
