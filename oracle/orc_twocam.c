/*
 * orc_twocam.c -- ORACLE (test infrastructure only): the two-camera (fisheye stereo) frame of the reference, restated
 * sequentially in strict IEEE C.  Frame::Frame(imLeft, imRight, ..., pCamera, pCamera2, Tlr) (src/Frame.cc:1101-1208),
 * Frame::ComputeStereoFishEyeMatches (:1210-1250) up to TriangulateMatches, and the numKPtsLeft() != -1 branches of
 * ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:44-219), SearchByProjection(CurF, LastF, th, bMono)
 * (:1969-2187) and SearchByBoW(pKF, F, vpMapPointMatches) (:276-478).
 *
 * A frame holds nL left keypoints then nR right ones (mvKeys, mvKeysRight); slots frame_mp[nL + nR] as holds_observed reads them.
 */
#include "orc_matcher.h"
#include <stdlib.h>

/* ---- ComputeStereoFishEyeMatches (:1210-1250) without TriangulateMatches ------------------------------------------- */
/* cand[nL] = trainIdx + monoRight of a left keypoint passing Lowe's test (-1 otherwise), dist2[2 nL] = the knn distances (-1 none) */
int orc_fisheye_matches(const uint8_t* descL, int nL, int monoLeft, const uint8_t* descR, int nR, int monoRight,
                        int32_t* cand, int32_t* dist2)
{
    const int nq = nL - monoLeft, nt = nR - monoRight;
    int n = 0;
    for (int i = 0; i < nL; i++) { cand[i] = -1; dist2[2 * i] = dist2[2 * i + 1] = -1; }
    if (nq <= 0) return 0;
    int32_t* idx = (int32_t*)malloc(sizeof(int32_t) * 2 * nq);
    int32_t* d = (int32_t*)malloc(sizeof(int32_t) * 2 * nq);
    orc_bf_knn2(descL + 32 * (size_t)monoLeft, nq, descR + 32 * (size_t)(monoRight > 0 ? monoRight : 0), nt > 0 ? nt : 0, idx, d);
    for (int qi = 0; qi < nq; qi++) {
        const int i = qi + monoLeft;
        const int size = (idx[2 * qi] >= 0) + (idx[2 * qi + 1] >= 0);           /* matches[qi].size() */
        if (idx[2 * qi] >= 0) dist2[2 * i] = d[2 * qi];
        if (idx[2 * qi + 1] >= 0) dist2[2 * i + 1] = d[2 * qi + 1];
        /* (*it).size() >= 2 && (*it)[0].distance < (*it)[1].distance * 0.7  (:1233: float distance, double product) */
        if (size >= 2 && (double)(float)d[2 * qi] < (double)(float)d[2 * qi + 1] * 0.7) { cand[i] = idx[2 * qi] + monoRight; n++; }
    }
    free(idx); free(d);
    return n;
}

/* ---- the two grids (AssignFeaturesToGrid :431-460) -------------------------------------------------------------------- */
typedef struct {
    int nL;
    const orc_keypoint* kps;
    orc_frame* grid[2];                /* mGrid / mGridRight: each camera's keypoints, camera-local indices */
} twocam_frame;

static void frame_init(twocam_frame* f, const orc_keypoint* kps, int nL, int nR, const orc_grid_bounds* gb)
{
    f->nL = nL; f->kps = kps;
    f->grid[0] = orc_frame_create(kps, nL, NULL, 0, NULL, gb);
    f->grid[1] = orc_frame_create(kps + nL, nR, NULL, 0, NULL, gb);
}

static void frame_free(twocam_frame* f) { orc_frame_destroy(f->grid[0]); orc_frame_destroy(f->grid[1]); }

/* Frame::getKPtLevelMono(j) = mvKeysUn[j].octave (:1417-1420).  mvKeysUn holds the nL left keypoints (:1191); past them (j >= nL,
 * an out-of-range read in the reference) the right keypoint's own octave, as upstream ORB-SLAM3 reads it. */
static int level_mono(const twocam_frame* f, int j) { return j < f->nL ? f->kps[j].octave : f->kps[f->nL + j].octave; }

/* Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel, bRight) (:710-781); returns camera-local indices in the reference's order */
static int features_in_area(const twocam_frame* f, float x, float y, float r, int minLevel, int maxLevel, int bRight, int* out)
{
    const orc_frame* g = f->grid[bRight];
    int n = 0;
    const float factorX = r, factorY = r;
    int t = (int)floorf((x - g->gb.minX - factorX) * g->gb.invW);
    const int nMinCellX = t > 0 ? t : 0;
    if (nMinCellX >= FRAME_GRID_COLS) return 0;
    t = (int)ceilf((x - g->gb.minX + factorX) * g->gb.invW);
    const int nMaxCellX = t < FRAME_GRID_COLS - 1 ? t : FRAME_GRID_COLS - 1;
    if (nMaxCellX < 0) return 0;
    t = (int)floorf((y - g->gb.minY - factorY) * g->gb.invH);
    const int nMinCellY = t > 0 ? t : 0;
    if (nMinCellY >= FRAME_GRID_ROWS) return 0;
    t = (int)ceilf((y - g->gb.minY + factorY) * g->gb.invH);
    const int nMaxCellY = t < FRAME_GRID_ROWS - 1 ? t : FRAME_GRID_ROWS - 1;
    if (nMaxCellY < 0) return 0;
    const int bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
        for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
            const int c = ix * FRAME_GRID_ROWS + iy;
            for (int p = g->cell_start[c]; p < g->cell_start[c + 1]; p++) {
                const int j = g->cell_items[p];
                /* kpUn = getDistKPtMono(j) (left) / getKPtRight(j) (right) (:751-753) */
                const orc_keypoint* kp = &g->kps[j];
                if (bCheckLevels) {
                    const int level = level_mono(f, j);                       /* :763: the LEFT keypoint j, even for bRight */
                    if (level < minLevel) continue;
                    if (maxLevel >= 0 && level > maxLevel) continue;
                }
                const float distx = kp->x - x, disty = kp->y - y;
                if (fabsf(distx) < factorX && fabsf(disty) < factorY) out[n++] = j;
            }
        }
    return n;
}

/* ---- SearchByProjection(F, vpMapPoints, th) :44-219, numKPtsLeft() != -1 ------------------------------------------------ */
/* per map point m: left in_view / proj_xy / level / view_cos / level_scale (= F.getORBScaleFactor(level)), right the same with _r
 * (level_r = mnTrackScaleLevelR, -1 = skip); l2r / r2l = mvLeftToRightMatch / mvRightToLeftMatch */
int orc_search_by_projection_map_fisheye(const orc_keypoint* kps, int nL, int nR, const uint8_t* desc, int stride,
                                         const orc_grid_bounds* gb, const int32_t* l2r, const int32_t* r2l, int M,
                                         const uint8_t* in_view, const float* proj_xy, const int32_t* level, const float* view_cos,
                                         const float* level_scale, const uint8_t* in_view_r, const float* proj_xy_r, const int32_t* level_r,
                                         const float* view_cos_r, const float* level_scale_r, const uint8_t* mp_desc, const uint8_t* mp_obs,
                                         int32_t* frame_mp, float th, float nnratio)
{
    twocam_frame F;
    frame_init(&F, kps, nL, nR, gb);
    int nmatches = 0;
    const int bFactor = th != 1.0;                                            /* :49 */
    int* idxs = (int*)malloc(sizeof(int) * (nL + nR + 1));
    for (int m = 0; m < M; m++) {
        if (!in_view[m] && !in_view_r[m]) continue;                           /* :54-55 (far points, isBad: on the host) */
        const uint8_t* dMP = mp_desc + 32 * (size_t)m;
        if (in_view[m]) {                                                     /* :63 */
            const int nPredictedLevel = level[m];
            float r = radius_by_viewing_cos(view_cos[m]);
            if (bFactor) r *= th;
            const int nc = features_in_area(&F, proj_xy[2 * m], proj_xy[2 * m + 1], r * level_scale[m], nPredictedLevel - 1, nPredictedLevel, 0, idxs);
            if (nc > 0) {
                int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
                for (int c = 0; c < nc; c++) {
                    const int idx = idxs[c];
                    if (holds_observed(frame_mp, idx, mp_obs)) continue;
                    /* (:95: the mvuRight gate only when numKPtsLeft() == -1) */
                    const int dist = orc_descriptor_distance(dMP, desc + (size_t)idx * stride);
                    if (dist < bestDist) {
                        bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel;
                        bestLevel = level_mono(&F, idx); bestIdx = idx;       /* :114 */
                    } else if (dist < bestDist2) {
                        bestLevel2 = level_mono(&F, idx); bestDist2 = dist;
                    }
                }
                if (bestDist <= TH_HIGH) {                                    /* :127-145 */
                    if (bestLevel == bestLevel2 && (float)bestDist > nnratio * (float)bestDist2) continue;   /* :130: skips the right block */
                    if (bestLevel != bestLevel2 || (float)bestDist <= nnratio * (float)bestDist2) {
                        frame_mp[bestIdx] = m;
                        if (l2r[bestIdx] != -1) { frame_mp[l2r[bestIdx] + nL] = m; nmatches++; }   /* :135-140 */
                        nmatches++;
                    }
                }
            }
        }
        if (in_view_r[m]) {                                                   /* :148 */
            const int nPredictedLevel = level_r[m];
            if (nPredictedLevel != -1) {
                const float r = radius_by_viewing_cos(view_cos_r[m]);         /* :152: no th */
                const int nc = features_in_area(&F, proj_xy_r[2 * m], proj_xy_r[2 * m + 1], r * level_scale_r[m], nPredictedLevel - 1, nPredictedLevel, 1, idxs);
                if (nc == 0) continue;
                int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
                for (int c = 0; c < nc; c++) {
                    const int idx = idxs[c];
                    if (holds_observed(frame_mp, idx + nL, mp_obs)) continue;
                    const int dist = orc_descriptor_distance(dMP, desc + (size_t)(idx + nL) * stride);
                    if (dist < bestDist) {
                        bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel;
                        bestLevel = kps[nL + idx].octave; bestIdx = idx;      /* getKPtRight(idx).octave :184-190 */
                    } else if (dist < bestDist2) {
                        bestLevel2 = kps[nL + idx].octave; bestDist2 = dist;
                    }
                }
                if (bestDist <= TH_HIGH) {
                    if (bestLevel == bestLevel2 && (float)bestDist > nnratio * (float)bestDist2) continue;
                    if (r2l[bestIdx] != -1) { frame_mp[r2l[bestIdx]] = m; nmatches++; }   /* :202-207 */
                    frame_mp[bestIdx + nL] = m;
                    nmatches++;
                }
            }
        }
    }
    free(idxs); frame_free(&F);
    return nmatches;
}

/* ---- SearchByProjection(CurF, LastF, th, bMono) :1969-2187, two-camera frames ------------------------------------------ */
/* queries: the n_last points of the last frame; valid / uv = the left projection with invzc < 0, bounds and outliers folded in
 * (:1998-2012); uv_r = mpCamera->project(mTrl x3Dc) (:2093-2095); last_kps in index order (octave = getKPtLevelMono(i), with
 * the rule of level_mono for i >= nL_last; angle); level_scale = getORBScaleFactor(octave); mode 0 / 1 forward / 2 backward */
int orc_search_by_projection_last_fisheye(const orc_keypoint* kps, int nL, int nR, const uint8_t* desc, int stride,
                                          const orc_grid_bounds* gb, const orc_keypoint* last_kps, int n_last, const uint8_t* valid,
                                          const float* uv, const float* uv_r, const uint8_t* mp_desc, const uint8_t* mp_obs,
                                          const float* level_scale, int32_t* cur_mp, float th, int mode, int checkOri)
{
    twocam_frame F;
    frame_init(&F, kps, nL, nR, gb);
    int nmatches = 0;
    int* rotHist[HISTO_LENGTH]; int rotN[HISTO_LENGTH];
    for (int i = 0; i < HISTO_LENGTH; i++) { rotHist[i] = (int*)malloc(sizeof(int) * (2 * n_last + 1)); rotN[i] = 0; }
    int* idxs = (int*)malloc(sizeof(int) * (nL + nR + 1));
    for (int i = 0; i < n_last; i++) {
        if (!valid[i]) continue;
        const int nLastOctave = last_kps[i].octave;
        const float radius = th * level_scale[i];                             /* :2017 */
        const uint8_t* dMP = mp_desc + 32 * (size_t)i;
        int nc;
        if (mode == 1) nc = features_in_area(&F, uv[2 * i], uv[2 * i + 1], radius, nLastOctave, -1, 0, idxs);
        else if (mode == 2) nc = features_in_area(&F, uv[2 * i], uv[2 * i + 1], radius, 0, nLastOctave, 0, idxs);
        else nc = features_in_area(&F, uv[2 * i], uv[2 * i + 1], radius, nLastOctave - 1, nLastOctave + 1, 0, idxs);
        if (nc == 0) continue;                                                /* :2032-2033: the right search is skipped too */
        int bestDist = 256, bestIdx2 = -1;
        for (int c = 0; c < nc; c++) {
            const int i2 = idxs[c];
            if (holds_observed(cur_mp, i2, mp_obs)) continue;
            const int dist = orc_descriptor_distance(dMP, desc + (size_t)i2 * stride);
            if (dist < bestDist) { bestDist = dist; bestIdx2 = i2; }
        }
        if (bestDist <= TH_HIGH) {
            cur_mp[bestIdx2] = i;
            nmatches++;
            if (checkOri) { const int bin = rot_bin(last_kps[i].angle, kps[bestIdx2].angle); rotHist[bin][rotN[bin]++] = bestIdx2; }
        }
        /* :2092-2162, right camera: same radius and levels, right grid, no bounds check */
        if (mode == 1) nc = features_in_area(&F, uv_r[2 * i], uv_r[2 * i + 1], radius, nLastOctave, -1, 1, idxs);
        else if (mode == 2) nc = features_in_area(&F, uv_r[2 * i], uv_r[2 * i + 1], radius, 0, nLastOctave, 1, idxs);
        else nc = features_in_area(&F, uv_r[2 * i], uv_r[2 * i + 1], radius, nLastOctave - 1, nLastOctave + 1, 1, idxs);
        bestDist = 256; bestIdx2 = -1;
        for (int c = 0; c < nc; c++) {
            const int i2 = idxs[c];
            if (holds_observed(cur_mp, i2 + nL, mp_obs)) continue;
            const int dist = orc_descriptor_distance(dMP, desc + (size_t)(i2 + nL) * stride);
            if (dist < bestDist) { bestDist = dist; bestIdx2 = i2; }
        }
        if (bestDist <= TH_HIGH) {
            cur_mp[bestIdx2 + nL] = i;
            nmatches++;
            if (checkOri) {
                const int bin = rot_bin(last_kps[i].angle, kps[nL + bestIdx2].angle);
                rotHist[bin][rotN[bin]++] = bestIdx2 + nL;                   /* :2155 */
            }
        }
    }
    if (checkOri) {                                                           /* :2165-2184 */
        int ind1 = -1, ind2 = -1, ind3 = -1;
        orc_three_maxima(rotN, HISTO_LENGTH, &ind1, &ind2, &ind3);
        for (int i = 0; i < HISTO_LENGTH; i++)
            if (i != ind1 && i != ind2 && i != ind3)
                for (int j = 0; j < rotN[i]; j++) { cur_mp[rotHist[i][j]] = -1; nmatches--; }
    }
    for (int i = 0; i < HISTO_LENGTH; i++) free(rotHist[i]);
    free(idxs); frame_free(&F);
    return nmatches;
}

/* ---- SearchByBoW(pKF, F, vpMapPointMatches) :276-478, numKPtsLeft() != -1 ---------------------------------------------- */
/* feature vectors as CSR (node ids ascending); the frame's features are nL left then the right ones (n_f in all); kf_kps in the
 * KeyFrame's index order (:391-393 picks its right keypoint for realIdxKF >= NLeft); match_f[n_f] out */
int orc_search_by_bow_fisheye(const orc_keypoint* kf_kps, const uint8_t* kf_desc, const uint8_t* kf_has_mp,
                              const uint32_t* kf_nodes, const int32_t* kf_node_off, const int32_t* kf_idx, int kf_nn,
                              const orc_keypoint* f_kps, int n_f, int nL, const uint8_t* f_desc,
                              const uint32_t* f_nodes, const int32_t* f_node_off, const int32_t* f_idx, int f_nn,
                              int32_t* match_f, float nnratio, int checkOri)
{
    int nmatches = 0;
    for (int i = 0; i < n_f; i++) match_f[i] = -1;
    int* rotHist[HISTO_LENGTH]; int rotN[HISTO_LENGTH];
    for (int i = 0; i < HISTO_LENGTH; i++) { rotHist[i] = (int*)malloc(sizeof(int) * (n_f + 1)); rotN[i] = 0; }
    int a = 0, b = 0;
    while (a < kf_nn && b < f_nn) {
        if (kf_nodes[a] == f_nodes[b]) {
            for (int iKF = kf_node_off[a]; iKF < kf_node_off[a + 1]; iKF++) {
                const int realIdxKF = kf_idx[iKF];
                if (!kf_has_mp[realIdxKF]) continue;                          /* !pMP || pMP->isBad() */
                const uint8_t* dKF = kf_desc + 32 * (size_t)realIdxKF;
                int bestDist1 = 256, bestIdxF = -1, bestDist2 = 256;
                int bestDist1R = 256, bestIdxFR = -1, bestDist2R = 256;
                for (int iF = f_node_off[b]; iF < f_node_off[b + 1]; iF++) {  /* :357-377 */
                    const int realIdxF = f_idx[iF];
                    if (match_f[realIdxF] >= 0) continue;
                    const int dist = orc_descriptor_distance(dKF, f_desc + 32 * (size_t)realIdxF);
                    if (realIdxF < nL && dist < bestDist1) { bestDist2 = bestDist1; bestDist1 = dist; bestIdxF = realIdxF; }
                    else if (realIdxF < nL && dist < bestDist2) bestDist2 = dist;
                    if (realIdxF >= nL && dist < bestDist1R) { bestDist2R = bestDist1R; bestDist1R = dist; bestIdxFR = realIdxF; }
                    else if (realIdxF >= nL && dist < bestDist2R) bestDist2R = dist;
                }
                if (bestDist1 <= TH_LOW) {                                    /* :382 */
                    if ((float)bestDist1 < nnratio * (float)bestDist2) {
                        match_f[bestIdxF] = realIdxKF;
                        if (checkOri) { const int bin = rot_bin(kf_kps[realIdxKF].angle, f_kps[bestIdxF].angle); rotHist[bin][rotN[bin]++] = bestIdxF; }
                        nmatches++;
                    }
                    if (bestDist1R <= TH_LOW) {                               /* :410 */
                        if ((float)bestDist1R < nnratio * (float)bestDist2R || 1) {   /* :412 "|| true" */
                            match_f[bestIdxFR] = realIdxKF;
                            if (checkOri) { const int bin = rot_bin(kf_kps[realIdxKF].angle, f_kps[bestIdxFR].angle); rotHist[bin][rotN[bin]++] = bestIdxFR; }
                            nmatches++;
                        }
                    }
                }
            }
            a++; b++;
        } else if (kf_nodes[a] < f_nodes[b]) {
            while (a < kf_nn && kf_nodes[a] < f_nodes[b]) a++;                /* lower_bound */
        } else {
            while (b < f_nn && f_nodes[b] < kf_nodes[a]) b++;
        }
    }
    if (checkOri) {
        int ind1 = -1, ind2 = -1, ind3 = -1;
        orc_three_maxima(rotN, HISTO_LENGTH, &ind1, &ind2, &ind3);
        for (int i = 0; i < HISTO_LENGTH; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (int j = 0; j < rotN[i]; j++) { match_f[rotHist[i][j]] = -1; nmatches--; }
        }
    }
    for (int i = 0; i < HISTO_LENGTH; i++) free(rotHist[i]);
    return nmatches;
}
