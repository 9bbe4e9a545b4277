// project.hip -- map points projected on the device: Frame::isInFrustum / isInFrustumChecks (src/Frame.cc:548-637, :1252-1325),
// MapPoint::PredictScale (src/MapPoint.cc:570-593) and the projection loops of ORBmatcher::SearchByProjection (src/ORBmatcher.cc
// :1999-2022, :2092-2095, :2215-2239), and the KeyFrame-side projections of Fuse, SearchByProjection(pKF, Scw, ...) and SearchBySim3
// (:1463-1513, :1650-1690, :511-550, :1799-1830).  One thread per map point (and keyframe), float arithmetic in the reference's order with the double steps
// of OpenCV 3.4.1 ("Parity choices of the projector"); the CPU restatement is tests/proj_ref/proj_ref.c.
// The kernels write the caller-visible arrays and the packed records the matcher kernels read (match.hip), so a fused entry point
// launches the matcher straight behind them.
#include "project_args.h"
#include <type_traits>

namespace eorb {

// MapPoint::PredictScale: ceil(log(ratio) / fLogScaleFactor) with float ratio -> std::log(float), a float quotient, std::ceil(float),
// then the conversion to int.  A value no int holds (ratio 0, inf or NaN) converts as cvttss2si does: INT_MIN, which clamps to 0.
__device__ __forceinline__ int predict_scale(float max_dist, float dist, int nlevels, float log_scale)
{
    const float ratio = max_dist / dist;
    const float cf = ceilf(dev_logf(ratio) / log_scale);
    int n = (cf >= -2147483648.0f && cf < 2147483648.0f) ? (int)cf : (int)0x80000000;
    if (n < 0) n = 0;
    else if (n >= nlevels) n = nlevels - 1;
    return n;
}

// the tables PredictScale reads: AKAZE's for a non-ORB point of a mixed view (MapPoint.cc:580-584)
__device__ __forceinline__ void scale_tables(const ProjView& V, bool is_orb, int& nlevels, float& log_scale, const float*& sf)
{
    if (!is_orb && V.ak_nlevels > 0) { nlevels = V.ak_nlevels; log_scale = V.ak_log_scale; sf = V.ak_sf; }
    else { nlevels = V.nlevels; log_scale = V.log_scale; sf = V.sf; }
}

__device__ __forceinline__ bool finite2(float u, float v)
{
    return (__float_as_uint(u) & 0x7f800000u) != 0x7f800000u && (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
}

struct FrustumRec { int in_view, reason, level; float x, y, xr, cos, depth, lscale; };

// Frame::isInFrustumChecks of one view; the mono branch of isInFrustum (:550-625) is the same sequence plus mTrackProjXR
__device__ __forceinline__ FrustumRec frustum_view(const ProjView& V, const float P[3], const float Pn[3], float minD, float maxD,
                                                   bool is_orb, float cos_limit)
{
    FrustumRec o{0, 0, -1, -1.f, -1.f, 0.f, 0.f, 0.f, 0.f};
    float Pc[3];
    cv_gemm3x1(V.R, P, V.t, 1.0, Pc);                                   // mRcw*P + mtcw
    o.depth = (float)cv_norm3(Pc);                                      // Pc_dist
    const float PcZ = Pc[2];
    if (PcZ < 0.0f) { o.reason = 2; return o; }
    float u, v;
    cam_project_f(V.cam, Pc, u, v);
    if (!finite2(u, v)) { o.reason = 7; return o; }
    if (u < V.minX || u > V.maxX) { o.reason = 3; return o; }
    if (v < V.minY || v > V.maxY) { o.reason = 4; return o; }
    o.x = u; o.y = v;
    const float PO[3] = {P[0] - V.Ow[0], P[1] - V.Ow[1], P[2] - V.Ow[2]};
    const float dist = (float)cv_norm3(PO);
    if (dist < 0.8f * minD || dist > 1.2f * maxD) { o.reason = 5; return o; }
    const float viewCos = (float)(cv_dot3(PO, Pn) / (double)dist);
    o.cos = viewCos;
    if (viewCos < cos_limit) { o.reason = 6; return o; }
    int nlevels; float log_scale; const float* sf;
    scale_tables(V, is_orb, nlevels, log_scale, sf);
    o.level = predict_scale(maxD, dist, nlevels, log_scale);
    o.lscale = sf[o.level];
    o.xr = u - V.mbf * (1.0f / PcZ);
    o.in_view = 1;
    return o;
}

__device__ __forceinline__ void frustum_store(const FrustumDev& O, int m, const FrustumRec& r, bool search)
{
    O.in_view[m] = (uint8_t)r.in_view;
    O.proj_xy[m] = make_float2(r.x, r.y);
    O.proj_xr[m] = r.xr;
    O.level[m] = r.level;
    O.view_cos[m] = r.cos;
    O.depth[m] = r.depth;
    O.level_scale[m] = r.lscale;
    O.reason[m] = (uint8_t)r.reason;
    O.rec[m] = make_float4(r.x, r.y, r.cos, r.lscale);
    O.search[m] = (uint8_t)(search ? 1 : 0);
}

__global__ __launch_bounds__(256) void project_frustum_kernel(const FrustumArgs A)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    bool any = false;
    if (m < A.M) {
        FrustumRec r[2];
        if (A.skip && A.skip[m]) {
            r[0] = FrustumRec{0, 1, -1, -1.f, -1.f, 0.f, 0.f, 0.f, 0.f};
            r[1] = r[0];
        } else {
            const float P[3] = {A.pos[3 * (size_t)m], A.pos[3 * (size_t)m + 1], A.pos[3 * (size_t)m + 2]};
            const float Pn[3] = {A.normal[3 * (size_t)m], A.normal[3 * (size_t)m + 1], A.normal[3 * (size_t)m + 2]};
            const float minD = A.min_dist[m], maxD = A.max_dist[m];
            const bool is_orb = A.is_orb ? A.is_orb[m] != 0 : true;
            r[0] = frustum_view(A.V[0], P, Pn, minD, maxD, is_orb, A.cos_limit);
            if (A.nviews > 1) r[1] = frustum_view(A.V[1], P, Pn, minD, maxD, is_orb, A.cos_limit);
            else r[1] = r[0];
        }
        // "if(bFarPoints && pMP->mTrackDepth>thFarPoints) continue;" (ORBmatcher.cc:57): the left view's depth when it accepted the
        // point, else the right view's
        const float d = (A.nviews > 1 && !r[0].in_view) ? r[1].depth : r[0].depth;
        const bool gate = A.far && d > A.th_far;
        frustum_store(A.O[0], m, r[0], r[0].in_view && !gate);
        any = r[0].in_view != 0;
        if (A.nviews > 1) {
            frustum_store(A.O[1], m, r[1], r[1].in_view && !gate);
            any = any || r[1].in_view != 0;
        }
    }
    const unsigned long long b = __ballot(any);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(A.n_in_view, __popcll(b));
}

__global__ __launch_bounds__(256) void project_last_kernel(const LastArgs A)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    int nlevels; float log_scale; const float* sf;
    scale_tables(A.V, A.is_orb ? A.is_orb[i] != 0 : true, nlevels, log_scale, sf);
    const float ls = sf[A.kps[i].octave];                               // getORBScaleFactor(nLastOctave) (:2019-2022)
    bool valid = false;
    float u = -1.f, v = -1.f, ur = 0.f, u_r = -1.f, v_r = -1.f;
    if (!(A.skip && A.skip[i])) {
        const float P[3] = {A.pos[3 * (size_t)i], A.pos[3 * (size_t)i + 1], A.pos[3 * (size_t)i + 2]};
        float x3Dc[3];
        cv_gemm3x1(A.V.R, P, A.V.t, 1.0, x3Dc);                         // Rcw*x3Dw + tcw
        const float invzc = (float)(1.0 / (double)x3Dc[2]);
        if (!(invzc < 0)) {
            float pu, pv;
            cam_project_f(A.V.cam, x3Dc, pu, pv);
            if (finite2(pu, pv) && !(pu < A.V.minX || pu > A.V.maxX) && !(pv < A.V.minY || pv > A.V.maxY)) {
                valid = true;
                u = pu; v = pv;
                ur = pu - A.V.mbf * invzc;                              // :2051
                if (A.has_r) {                                          // mTrl * x3Dc (:2093-2095), no bounds test
                    float x3Dr[3];
                    cv_gemm3x1(A.Trl, x3Dc, A.Trl + 9, 1.0, x3Dr);
                    cam_project_f(A.cam_r, x3Dr, u_r, v_r);
                }
            }
        }
    }
    A.valid[i] = (uint8_t)(valid ? 1 : 0);
    A.uv[i] = make_float2(u, v);
    A.proj_ur[i] = ur;
    A.level_scale[i] = ls;
    A.uv_r[i] = make_float2(u_r, v_r);
    A.rec3[3 * (size_t)i] = u; A.rec3[3 * (size_t)i + 1] = v; A.rec3[3 * (size_t)i + 2] = ls;
}

__global__ __launch_bounds__(256) void project_kf_kernel(const KfArgs A)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n) return;
    bool valid = false;
    float u = -1.f, v = -1.f, ls = 0.f, dist3D = 0.f;
    int level = -1;
    if (!(A.skip && A.skip[i])) {
        const float P[3] = {A.pos[3 * (size_t)i], A.pos[3 * (size_t)i + 1], A.pos[3 * (size_t)i + 2]};
        float x3Dc[3];
        cv_gemm3x1(A.V.R, P, A.V.t, 1.0, x3Dc);
        float pu, pv;
        cam_project_f(A.V.cam, x3Dc, pu, pv);                           // no depth-sign test (:2216-2218)
        if (finite2(pu, pv) && !(pu < A.V.minX || pu > A.V.maxX) && !(pv < A.V.minY || pv > A.V.maxY)) {
            u = pu; v = pv;
            const float PO[3] = {P[0] - A.V.Ow[0], P[1] - A.V.Ow[1], P[2] - A.V.Ow[2]};
            dist3D = (float)cv_norm3(PO);
            const float minD = A.min_dist[i], maxD = A.max_dist[i];
            if (!(dist3D < 0.8f * minD || dist3D > 1.2f * maxD)) {
                int nlevels; float log_scale; const float* sf;
                scale_tables(A.V, A.is_orb ? A.is_orb[i] != 0 : true, nlevels, log_scale, sf);
                level = predict_scale(maxD, dist3D, nlevels, log_scale);
                ls = sf[level];
                valid = true;
            }
        }
    }
    A.valid[i] = (uint8_t)(valid ? 1 : 0);
    A.uv[i] = make_float2(u, v);
    A.level[i] = level;
    A.level_scale[i] = ls;
    A.dist3d[i] = dist3D;
    A.rec3[3 * (size_t)i] = u; A.rec3[3 * (size_t)i + 1] = v; A.rec3[3 * (size_t)i + 2] = ls;
    if (A.q_kps) {
        eorb_keypoint k = A.kf_kps[i];
        k.octave = level; k.class_id = level;                           // query level = nPredictedLevel (:2236)
        A.q_kps[i] = k;
    }
}

// ---- the KeyFrame-side modes -------------------------------------------------------------------------------------------------------
// KeyFrame::IsInImage (src/KeyFrame.cc:919-922): the upper bounds are strict, and a NaN or an infinity fails by itself
__device__ __forceinline__ bool kf_is_in_image(float x, float y, float minX, float maxX, float minY, float maxY)
{
    return x >= minX && x < maxX && y >= minY && y < maxY;
}

__device__ __forceinline__ void kfside_store(const KfSideDev& O, size_t i, bool valid, int reason, float u, float v, int level, float radius,
                                             float q_ur, float dist)
{
    O.valid[i] = (uint8_t)(valid ? 1 : 0);
    O.uv[i] = make_float2(u, v);
    O.level[i] = level;
    O.radius[i] = radius;
    O.q_ur[i] = q_ur;
    O.dist3d[i] = dist;
    O.reason[i] = (uint8_t)reason;
}

// mode D: the projection of Fuse(pKF, vpMapPoints, th, bRight) (src/ORBmatcher.cc:1463-1513), Fuse(pKF, Scw, ...) (:1650-1690) and
// SearchByProjection(pKF, Scw, ...) (:511-550, :595-), one thread per (keyframe, map point).  A rejected point keeps uv = (-1, -1)
// and q_ur = 0 until IsInImage has passed, dist3d = 0 until it was computed, level = -1 and radius = 0 throughout.
// MIXED: MixedMatcher's forms (src/MixedMatcher.cpp:1632-1688, :1837-1876, :1098-1134, :1226-1262), which differ in the tables alone: a
// non-ORB point of a keyframe with AKAZE tables takes its level from getAKAZENLevels / getAKAZELogScaleFactor (src/MapPoint.cc:545-568)
// and its radius from getAKAZEScaleFactor(level); the rule of scale_tables() above.
template <bool MIXED>
__global__ __launch_bounds__(256) void project_kfside_kernel(const std::conditional_t<MIXED, KfSideArgsMixed, KfSideArgs> A)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)A.K * A.M) return;
    const int k = (int)(i / A.M), m = (int)(i - (size_t)k * A.M);
    bool valid = false;
    int reason = 0, level = -1;
    float u = -1.f, v = -1.f, radius = 0.f, q_ur = 0.f, dist3D = 0.f;
    if (A.skip && A.skip[i]) reason = 1;
    else {
        const KfPose& V = A.V[k];
        const float P[3] = {A.pos[3 * (size_t)m], A.pos[3 * (size_t)m + 1], A.pos[3 * (size_t)m + 2]};
        float p3Dc[3];
        cv_gemm3x1(V.R, P, V.t, 1.0, p3Dc);                             // Rcw*p3Dw + tcw
        const float z = p3Dc[2];
        float pu = -1.f, pv = -1.f;
        if (!(z < 0.0f)) cam_project_f(V.cam, p3Dc, pu, pv);           // a zero depth goes on (:1467)
        if (z < 0.0f) reason = 2;
        else if (!kf_is_in_image(pu, pv, V.minX, V.maxX, V.minY, V.maxY)) reason = 3;
        else {
            u = pu; v = pv;
            q_ur = pu - V.mbf * (1.0f / z);                             // ur = uv.x - bf*invz (:1473, :1487)
            const float PO[3] = {P[0] - V.Ow[0], P[1] - V.Ow[1], P[2] - V.Ow[2]};
            dist3D = (float)cv_norm3(PO);
            const float minD = A.min_dist[m], maxD = A.max_dist[m];
            const float Pn[3] = {A.normal[3 * (size_t)m], A.normal[3 * (size_t)m + 1], A.normal[3 * (size_t)m + 2]};
            if (dist3D < 0.8f * minD || dist3D > 1.2f * maxD) reason = 5;
            else if (cv_dot3(PO, Pn) < 0.5 * (double)dist3D) reason = 6;   // "PO.dot(Pn)<0.5*dist3D": a comparison of doubles (:1504)
            else {
                bool ak = false;                                                 // the rule of scale_tables()
                if constexpr (MIXED) ak = A.ak_nlevels > 0 && A.mp_is_orb && !A.mp_is_orb[m];
                if constexpr (MIXED) {
                    level = predict_scale(maxD, dist3D, ak ? A.ak_nlevels : A.nlevels, ak ? A.ak_log_scale : A.log_scale);
                    radius = A.th * (ak ? A.ak_sf : A.sf)[level];
                } else {
                    level = predict_scale(maxD, dist3D, A.nlevels, A.log_scale);
                    radius = A.th * A.sf[level];
                }
                valid = true;
            }
        }
    }
    kfside_store(A.O, i, valid, reason, u, v, level, radius, q_ur, dist3D);
}

// mode E: the two projections of SearchBySim3 (:1799-1830, :1879-1910), one thread per (direction, keypoint slot)
__global__ __launch_bounds__(256) void project_sim3_kernel(const Sim3Args A)
{
    const int h = blockIdx.y, m = blockIdx.x * 256 + threadIdx.x;
    if (m >= A.M) return;
    const Sim3Half& S = A.H[h];
    bool valid = false;
    int reason = 0, level = -1;
    float u = -1.f, v = -1.f, radius = 0.f, dist3D = 0.f;
    if (m >= S.n || (S.skip && S.skip[m])) reason = 1;
    else {
        const float P[3] = {S.pos[3 * (size_t)m], S.pos[3 * (size_t)m + 1], S.pos[3 * (size_t)m + 2]};
        float pa[3], pb[3];
        cv_gemm3x1(S.Ra, P, S.ta, 1.0, pa);                             // R1w*p3Dw + t1w
        cv_gemm3x1(S.sRb, pa, S.tb, 1.0, pb);                           // sR21*p3Dc1 + t21
        if (pb[2] < 0.0f) reason = 2;
        else {
            const float invz = (float)(1.0 / (double)pb[2]);
            const float x = pb[0] * invz, y = pb[1] * invz;
            const float pu = S.fx * x + S.cx, pv = S.fy * y + S.cy;
            if (!kf_is_in_image(pu, pv, S.minX, S.maxX, S.minY, S.maxY)) reason = 3;
            else {
                u = pu; v = pv;
                dist3D = (float)cv_norm3(pb);                           // cv::norm(p3Dc2): the camera-frame norm
                const float minD = S.min_dist[m], maxD = S.max_dist[m];
                if (dist3D < 0.8f * minD || dist3D > 1.2f * maxD) reason = 5;
                else {
                    level = predict_scale(maxD, dist3D, S.nlevels, S.log_scale);
                    radius = A.th * S.sf[level];
                    valid = true;
                }
            }
        }
    }
    kfside_store(A.O, (size_t)h * A.M + m, valid, reason, u, v, level, radius, 0.f, dist3D);
}

int project_kfside_dev(eorb_ctx* c, const KfSideArgs& A)
{
    const size_t n = (size_t)A.K * A.M;
    if (n == 0) return EORB_OK;
    ProfScope ps(c, "project_kfside");
    project_kfside_kernel<false><<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(A);
    EORB_LAUNCH_CHECK(c, "project_kfside_kernel");
    return EORB_OK;
}

int project_kfside_mixed_dev(eorb_ctx* c, const KfSideArgsMixed& A)
{
    const size_t n = (size_t)A.K * A.M;
    if (n == 0) return EORB_OK;
    ProfScope ps(c, "project_kfside_mixed");
    project_kfside_kernel<true><<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(A);
    EORB_LAUNCH_CHECK(c, "project_kfside_mixed_kernel");
    return EORB_OK;
}

int project_sim3_dev(eorb_ctx* c, const Sim3Args& A)
{
    if (A.M <= 0) return EORB_OK;
    ProfScope ps(c, "project_sim3");
    project_sim3_kernel<<<dim3((A.M + 255) / 256, 2), 256, 0, c->stream>>>(A);
    EORB_LAUNCH_CHECK(c, "project_sim3_kernel");
    return EORB_OK;
}

int project_frustum_dev(eorb_ctx* c, const FrustumArgs& A)
{
    EORB_HIP(c, hipMemsetAsync(A.n_in_view, 0, sizeof(int32_t), c->stream));
    if (A.M <= 0) return EORB_OK;
    ProfScope ps(c, "project_frustum");
    project_frustum_kernel<<<(A.M + 255) / 256, 256, 0, c->stream>>>(A);
    EORB_LAUNCH_CHECK(c, "project_frustum_kernel");
    return EORB_OK;
}

int project_last_dev(eorb_ctx* c, const LastArgs& A)
{
    if (A.n <= 0) return EORB_OK;
    ProfScope ps(c, "project_last");
    project_last_kernel<<<(A.n + 255) / 256, 256, 0, c->stream>>>(A);
    EORB_LAUNCH_CHECK(c, "project_last_kernel");
    return EORB_OK;
}

int project_kf_dev(eorb_ctx* c, const KfArgs& A)
{
    if (A.n <= 0) return EORB_OK;
    ProfScope ps(c, "project_kf");
    project_kf_kernel<<<(A.n + 255) / 256, 256, 0, c->stream>>>(A);
    EORB_LAUNCH_CHECK(c, "project_kf_kernel");
    return EORB_OK;
}

}  // namespace eorb
