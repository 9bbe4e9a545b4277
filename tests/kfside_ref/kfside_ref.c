/* kfside_ref.c -- CPU restatement of the projector's KeyFrame-side modes (eorb_slam_amd/csrc/project.hip), strict IEEE
 * (-ffp-contract=off): mode D = the projection of ORBmatcher::Fuse (src/ORBmatcher.cc:1463-1513, :1650-1690) and of
 * SearchByProjection(pKF, Scw, ...) (:511-550, :595-), mode E = the two projections of SearchBySim3 (:1799-1830, :1879-1910).
 * Test infrastructure: compiled into a temporary directory by tests/kfside_ref/__init__.py, never loaded by the product.  The logf,
 * gemm, norm, dot and projection statics are proj_ref.c's (included as source; its exported names are part of this library too). */
#include "../proj_ref/proj_ref.c"

/* KeyFrame::IsInImage (src/KeyFrame.cc:919-922): strict upper bounds; a NaN or an infinity fails by itself */
static int kf_is_in_image(float x, float y, float minX, float maxX, float minY, float maxY)
{
    return x >= minX && x < maxX && y >= minY && y < maxY;
}

typedef struct kr_out { uint8_t* valid; float* uv; float* radius; int32_t* level; float* q_ur; float* dist3d; uint8_t* reason; } kr_out;

static void kr_store(const kr_out* O, long i, int valid, int reason, float u, float v, int level, float radius, float q_ur, float dist)
{
    if (O->valid) O->valid[i] = (uint8_t)valid;
    if (O->uv) { O->uv[2 * i] = u; O->uv[2 * i + 1] = v; }
    if (O->radius) O->radius[i] = radius;
    if (O->level) O->level[i] = level;
    if (O->q_ur) O->q_ur[i] = q_ur;
    if (O->dist3d) O->dist3d[i] = dist;
    if (O->reason) O->reason[i] = (uint8_t)reason;
}

/* mode D over K views and M shared map points: entry k * M + m; skip (optional) has K * M entries.  The tables are views[0]'s. */
void kr_keyframe_side(const pr_view* views, int K, long M, const float* pos, const float* normal, const float* min_dist,
                      const float* max_dist, const uint8_t* skip, float th, const kr_out* out)
{
    for (int k = 0; k < K; k++)
        for (long m = 0; m < M; m++) {
            const pr_view* V = views + k;
            const long i = (long)k * M + m;
            int valid = 0, reason = 0, level = -1;
            float u = -1.f, v = -1.f, radius = 0.f, q_ur = 0.f, dist3D = 0.f;
            if (skip && skip[i]) reason = 1;
            else {
                const float* P = pos + 3 * m;
                float p3Dc[3], pu = -1.f, pv = -1.f;
                gemm3x1(V->R, P, V->t, p3Dc);
                const float z = p3Dc[2];
                if (!(z < 0.0f)) project(&V->cam, p3Dc, &pu, &pv);
                if (z < 0.0f) reason = 2;
                else if (!kf_is_in_image(pu, pv, V->minX, V->maxX, V->minY, V->maxY)) reason = 3;
                else {
                    u = pu; v = pv;
                    q_ur = pu - V->mbf * (1.0f / z);
                    const float PO[3] = {P[0] - V->Ow[0], P[1] - V->Ow[1], P[2] - V->Ow[2]};
                    dist3D = (float)norm3(PO);
                    if (dist3D < 0.8f * min_dist[m] || dist3D > 1.2f * max_dist[m]) reason = 5;
                    else if (dot3(PO, normal + 3 * m) < 0.5 * (double)dist3D) reason = 6;
                    else {
                        level = pr_predict_scale(max_dist[m], dist3D, views->nlevels, views->log_scale);
                        radius = th * views->scale_factors[level];
                        valid = 1;
                    }
                }
            }
            kr_store(out, i, valid, reason, u, v, level, radius, q_ur, dist3D);
        }
}

/* the viewing-angle test as a float quotient would decide it (Frame::isInFrustum's form), for the known-answer test of the
 * double comparison: 1 = rejected */
int kr_angle_rejects_float(const float* PO, const float* Pn, float limit)
{
    const float dist = (float)norm3(PO);
    return (float)(dot3(PO, Pn) / (double)dist) < limit;
}
int kr_angle_rejects_double(const float* PO, const float* Pn)
{
    const float dist = (float)norm3(PO);
    return dot3(PO, Pn) < 0.5 * (double)dist;
}

/* mode E, one direction: points of keyframe a (pose Ra, ta) into keyframe b through (sRb, tb); cam = fx, fy, cx, cy; bounds, tables
 * of keyframe b (Vb) */
void kr_sim3_half(const float* Ra, const float* ta, const float* sRb, const float* tb, const float* cam, const pr_view* Vb, long n,
                  const float* pos, const float* min_dist, const float* max_dist, const uint8_t* skip, float th, const kr_out* out)
{
    for (long m = 0; m < n; m++) {
        int valid = 0, reason = 0, level = -1;
        float u = -1.f, v = -1.f, radius = 0.f, dist3D = 0.f;
        if (skip && skip[m]) reason = 1;
        else {
            float pa[3], pb[3];
            gemm3x1(Ra, pos + 3 * m, ta, pa);
            gemm3x1(sRb, pa, tb, pb);
            if (pb[2] < 0.0f) reason = 2;
            else {
                const float invz = (float)(1.0 / (double)pb[2]);
                const float x = pb[0] * invz, y = pb[1] * invz;
                const float pu = cam[0] * x + cam[2], pv = cam[1] * y + cam[3];
                if (!kf_is_in_image(pu, pv, Vb->minX, Vb->maxX, Vb->minY, Vb->maxY)) reason = 3;
                else {
                    u = pu; v = pv;
                    dist3D = (float)norm3(pb);
                    if (dist3D < 0.8f * min_dist[m] || dist3D > 1.2f * max_dist[m]) reason = 5;
                    else {
                        level = pr_predict_scale(max_dist[m], dist3D, Vb->nlevels, Vb->log_scale);
                        radius = th * Vb->scale_factors[level];
                        valid = 1;
                    }
                }
            }
        }
        kr_store(out, m, valid, reason, u, v, level, radius, 0.f, dist3D);
    }
}
