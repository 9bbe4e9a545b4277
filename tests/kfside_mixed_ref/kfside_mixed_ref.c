/* kfside_mixed_ref.c -- CPU restatement of MixedMatcher's KeyFrame-side matchers on a MixedKeyFrame, strict IEEE (-ffp-contract=off),
 * written from src/MixedMatcher.cpp: Fuse(pKF, vpMapPoints, th, bRight) (:1575-1797), Fuse(pKF, Scw, ...) (:1799-1933) and both
 * SearchByProjection(pKF, Scw, ...) (:1065-1189, :1191-1324).  The projection is mode D of kfside_ref.c (included as source) with the
 * scale tables picked per point; the search loop walks KeyFrame::GetFeaturesInArea in its order -- the oracle's
 * orc_get_features_in_area, handed in through km_set_area -- and applies the type gate, getKPtLevelMono, the per-keypoint sigma gate
 * and the descriptor distance as the reference writes them.  Test infrastructure: compiled into a temporary directory by
 * tests/kfside_mixed_ref/__init__.py, never loaded by the product. */
#include "../kfside_ref/kfside_ref.c"

/* mode D over K views and M shared map points (entry k * M + m), each point with the tables of its type: isORBMP =
 * pMP->isORBMapPoint() (:1632); PredictScale(dist3D, pKF) reads getAKAZENLevels / getAKAZELogScaleFactor for a non-ORB point of a
 * MixedKeyFrame (src/MapPoint.cc:545-568); radius = th * getAKAZEScaleFactor(level) instead of th * getORBScaleFactor(level)
 * (:1684-1688).  A view without AKAZE tables (ak_nlevels == 0) serves every point with the ORB ones. */
void km_keyframe_side(const pr_view* views, int K, long M, const float* pos, const float* normal, const float* min_dist,
                      const float* max_dist, const uint8_t* mp_is_orb, const uint8_t* skip, float th, const kr_out* out)
{
    for (int k = 0; k < K; k++)
        for (long m = 0; m < M; m++) {
            const pr_view* V = views + k;
            const long i = (long)k * M + m;
            int valid = 0, reason = 0, level = -1;
            float u = -1.f, v = -1.f, radius = 0.f, q_ur = 0.f, dist3D = 0.f;
            if (skip && skip[i]) reason = 1;
            else {
                const int isORBMP = !mp_is_orb || mp_is_orb[m];
                const float* P = pos + 3 * m;
                float p3Dc[3], pu = -1.f, pv = -1.f;
                gemm3x1(V->R, P, V->t, p3Dc);                                      /* Rcw*p3Dw + tcw (:1635) */
                const float z = p3Dc[2];
                if (!(z < 0.0f)) project(&V->cam, p3Dc, &pu, &pv);
                if (z < 0.0f) reason = 2;                                          /* :1638 */
                else if (!kf_is_in_image(pu, pv, V->minX, V->maxX, V->minY, V->maxY)) reason = 3;      /* :1652 */
                else {
                    u = pu; v = pv;
                    q_ur = pu - V->mbf * (1.0f / z);                               /* :1644, :1658 */
                    const float PO[3] = {P[0] - V->Ow[0], P[1] - V->Ow[1], P[2] - V->Ow[2]};
                    dist3D = (float)norm3(PO);
                    if (dist3D < 0.8f * min_dist[m] || dist3D > 1.2f * max_dist[m]) reason = 5;          /* :1666 */
                    else if (dot3(PO, normal + 3 * m) < 0.5 * (double)dist3D) reason = 6;                /* :1675 */
                    else {
                        int nlevels; float log_scale; const float* sf;
                        tables(V, isORBMP, &nlevels, &log_scale, &sf);
                        level = pr_predict_scale(max_dist[m], dist3D, nlevels, log_scale);               /* :1681 */
                        radius = th * sf[level];                                                         /* :1684-1688 */
                        valid = 1;
                    }
                }
            }
            kr_store(out, i, valid, reason, u, v, level, radius, q_ur, dist3D);
        }
}

/* KeyFrame::GetFeaturesInArea on the oracle's frame: candidates in the reference's order */
typedef int (*km_area_fn)(const void* frame, float x, float y, float r, int minLevel, int maxLevel, int* out, int cap);
static km_area_fn g_area = 0;
void km_set_area(km_area_fn f) { g_area = f; }

static int descriptor_distance32(const uint8_t* a, const uint8_t* b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

/* what a wrong reading of the reference would do, for the tests that show each rule decides results on their scenes */
enum { KM_NO_TYPE_GATE = 1, KM_LEVEL_FROM_OCTAVE = 2, KM_ORB_SIGMA_TABLE = 4 };

/* the search loop (:1690-1758; :1888-1921; :1143-1185; :1277-1320) over the projected points.  cand: room for n indices.
 * kp_is_orb[n] = pKF->isORBDescValid(idx), kp_inv_sigma2[n] = pKF->getKPtInvLevelSigma2(idx) (NULL: the forms without a reprojection
 * gate), uright[n] = pKF->mvuRight (NULL: none has one), taken[n] = vpMatched[idx] != NULL (NULL: Fuse).  wrong = 0 is the reference;
 * orb_inv_sigma2 is read only by KM_ORB_SIGMA_TABLE. */
void km_search(const void* frame, const pr_keypoint* kps, int n, const uint8_t* desc, int stride, const uint8_t* kp_is_orb,
               const float* kp_inv_sigma2, const float* uright, long M, const uint8_t* valid, const float* uv, const float* radius,
               const int32_t* level, const uint8_t* q_desc, const uint8_t* mp_is_orb, const float* q_ur, uint8_t* taken, float accept_thr,
               int wrong, const float* orb_inv_sigma2, int* cand, int32_t* best_idx, int32_t* best_dist)
{
    for (long m = 0; m < M; m++) {
        best_idx[m] = -1; best_dist[m] = 256;
        if (!valid[m] || n == 0) continue;
        const int isORBMP = !mp_is_orb || mp_is_orb[m];
        const float u = uv[2 * m], v = uv[2 * m + 1];
        const int nPredictedLevel = level[m];
        const int nc = g_area(frame, u, v, radius[m], -1, -1, cand, n);
        int bestDist = 256, bestIdx = -1;
        for (int j = 0; j < nc; j++) {
            const int idx = cand[j];
            if (taken && taken[idx]) continue;                                         /* if(vpMatched[idx]) continue; (:1150) */
            const int isORBPt = !kp_is_orb || kp_is_orb[idx];
            if (!(wrong & KM_NO_TYPE_GATE) && isORBMP != isORBPt) continue;            /* :1707-1710 */
            /* getKPtLevelMono(idx): octave of an ORB row, class_id of an AKAZE row (src/MixedFrame.cpp:438-446) */
            const int kpLevel = (isORBPt || (wrong & KM_LEVEL_FROM_OCTAVE)) ? kps[idx].octave : kps[idx].class_id;
            if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;  /* :1718 */
            if (kp_inv_sigma2) {
                const float invSigma2 = (wrong & KM_ORB_SIGMA_TABLE) ? orb_inv_sigma2[kps[idx].octave] : kp_inv_sigma2[idx];
                const float ex = u - kps[idx].x, ey = v - kps[idx].y;
                if (uright && uright[idx] >= 0) {                                      /* :1721-1734 */
                    const float er = q_ur[m] - uright[idx];
                    const float e2 = ex * ex + ey * ey + er * er;
                    if (e2 * invSigma2 > 7.8) continue;
                } else {                                                               /* :1735-1745 */
                    const float e2 = ex * ex + ey * ey;
                    if (e2 * invSigma2 > 5.99) continue;
                }
            }
            const int dist = descriptor_distance32(q_desc + 32 * (size_t)m, desc + (size_t)stride * idx);
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }                   /* :1753-1757 */
        }
        best_idx[m] = bestIdx; best_dist[m] = bestDist;
        if (taken && bestIdx >= 0 && (float)bestDist <= accept_thr) taken[bestIdx] = 1;    /* bestDist<=TH_LOW*ratioHamming (:1180) */
    }
}
