// project.hip -- map points projected on the device: Frame::isInFrustum / isInFrustumChecks (src/Frame.cc:548-637, :1252-1325),
// MapPoint::PredictScale (src/MapPoint.cc:570-593) and the projection loops of ORBmatcher::SearchByProjection (src/ORBmatcher.cc
// :1999-2022, :2092-2095, :2215-2239).  One thread per map point, float arithmetic in the reference's order with the double steps
// of OpenCV 3.4.1 ("Parity choices of the projector"); the CPU restatement is tests/proj_ref/proj_ref.c.
// The kernels write the caller-visible arrays and the packed records the matcher kernels read (match.hip), so a fused entry point
// launches the matcher straight behind them.
#include "project_args.h"

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
