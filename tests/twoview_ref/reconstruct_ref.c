/*
 * reconstruct_ref.c -- TEST INFRASTRUCTURE: what eorb_two_view_reconstruct computes, restated sequentially in strict IEEE C (no FMA
 * contraction): TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc:67-262) over the caller's sets, with ReconstructF,
 * ReconstructH, DecomposeE, resolveReconstStat* and CheckRT.  The RANSAC, CheckRT and the SVD are twoview_ref.c's (included as source; its
 * exported names are part of this library too).  The 3x3 algebra and the four decision rules are the text of
 * eorb_slam_amd/csrc/twoview_core.h, which the device compiles as well (the pattern of mlpnp_core.h); what is written here alone is the
 * sequence around them.  The independent second writing of the rules and of the hypotheses is reconstruct_model.py.  Nothing is pinned
 * against a build of the reference.
 */
#include "twoview_ref.c"
#include "../../include/eorb_fe.h"

static double tvr_mk_double(uint32_t hi, uint32_t lo) { const uint64_t u = ((uint64_t)hi << 32) | lo; double d; memcpy(&d, &u, 8); return d; }
static int32_t tvr_hi_word(double x) { uint64_t u; memcpy(&u, &x, 8); return (int32_t)(u >> 32); }
static uint32_t tvr_lo_word(double x) { uint64_t u; memcpy(&u, &x, 8); return (uint32_t)u; }

#define TVC_FN static
#define TVC_HI(x) tvr_hi_word(x)
#define TVC_LO(x) tvr_lo_word(x)
#define TVC_MK(hi, lo) tvr_mk_double((uint32_t)(hi), (uint32_t)(lo))
#define TVC_SVD33(A, w, u, vt) tvr_svd((A), 3, 3, (w), (u), (vt))
#define TVC_UNROLL
#include "../../eorb_slam_amd/csrc/twoview_core.h"

double tvr_acos(double x) { return tvc_dacos(x); }
float tvr_parallax(int n_good, float cos_sel) { return tvc_parallax(n_good, cos_sel); }
void tvr_hypotheses_f(const float* K, const float* F21, float* poses) { tvc_hypotheses_f(K, F21, poses); }
int tvr_hypotheses_h(const float* K, const float* H21, float th_rd_homo, float* poses) { return tvc_hypotheses_h(K, H21, th_rd_homo, poses); }

/* Reconstruct between its two stages (:139-157 / :236-261 and the heads of ReconstructF / ReconstructH): from the RANSAC's results to the
 * hypotheses.  res: zeroed here, then SH .. F21, RH, is_homography, stage, n_inliers, n_hyp; poses[8][27] (zeros past n_hyp);
 * sel_inliers[N]: the chosen model's flags, CheckRT's vbMatchesInliers; trans_inliers[N]: vbTransInliers (zeros in the STOCK form).
 * Returns n_hyp. */
int tvr_decide(float SH, float SF, int best_it_h, int best_it_f, const float* H21, const float* F21, const uint8_t* inliers_h,
               const uint8_t* inliers_f, int N, const float* K, const eorb_tvr_recon_params* p,
               eorb_tvr_recon_result* r, float* poses, uint8_t* sel_inliers, uint8_t* trans_inliers)
{
    memset(r, 0, sizeof *r);
    memset(poses, 0, sizeof(float) * 27 * 8);
    memset(trans_inliers, 0, (size_t)N);
    r->SH = SH; r->SF = SF; r->best_it_h = best_it_h; r->best_it_f = best_it_f;
    memcpy(r->H21, H21, sizeof r->H21); memcpy(r->F21, F21, sizeof r->F21);
    r->hyp_best = r->hyp_second = -1;
    if (SH + SF == 0.f) {
        memcpy(sel_inliers, inliers_f, (size_t)N);
        if (p->form == EORB_TVR_FORM_INFO) memcpy(trans_inliers, inliers_f, (size_t)N);
        return 0;                                           /* stage 0 */
    }
    r->RH = SH / (SH + SF);
    r->is_homography = r->RH > p->th_hf_ratio;
    const uint8_t* src = r->is_homography ? inliers_h : inliers_f;
    memcpy(sel_inliers, src, (size_t)N);
    if (p->form == EORB_TVR_FORM_INFO) memcpy(trans_inliers, src, (size_t)N);
    for (int i = 0; i < N; i++) if (src[i]) r->n_inliers++;
    if (!r->is_homography) { tvc_hypotheses_f(K, r->F21, poses); r->n_hyp = 4; r->stage = 2; }
    else if (tvc_hypotheses_h(K, r->H21, p->th_rd_homo, poses)) { r->n_hyp = 8; r->stage = 2; }
    else r->stage = 1;
    return r->n_hyp;
}

/* Reconstruct after CheckRT: the parallax, the decision, the result slots.  n_good / cos_sel / good / p3d: tvr_check_rt's results for the
 * n_hyp poses (not read when stage < 2).  R21[2][9], t21[2][3], p3d_out[2][n1][3], tri_out[2][n1]: zeroed, then the chosen slots. */
void tvr_finish(const eorb_tvr_recon_params* p, eorb_tvr_recon_result* r, const float* poses, int n1, const int32_t* n_good,
                const float* cos_sel, const uint8_t* good, const float* p3d, float* R21, float* t21, float* p3d_out, uint8_t* tri_out)
{
    memset(R21, 0, sizeof(float) * 18); memset(t21, 0, sizeof(float) * 6);
    memset(p3d_out, 0, sizeof(float) * 6 * (size_t)n1); memset(tri_out, 0, 2 * (size_t)n1);
    if (r->stage != 2) return;
    int32_t ng[8] = {0};
    float par[8] = {0};
    for (int h = 0; h < r->n_hyp; h++) { ng[h] = n_good[h]; par[h] = tvc_parallax(n_good[h], cos_sel[h]); }
    tvc_resolve(p, r->n_inliers, ng, par, r);
    const int slot[2] = {r->hyp_best, r->hyp_second};
    for (int s = 0; s < 2; s++) {
        const int h = slot[s];
        if (h < 0) continue;
        memcpy(R21 + 9 * s, poses + 27 * h, sizeof(float) * 9);
        memcpy(t21 + 3 * s, poses + 27 * h + 9, sizeof(float) * 3);
        memcpy(p3d_out + (size_t)s * n1 * 3, p3d + (size_t)h * n1 * 3, sizeof(float) * 3 * (size_t)n1);
        memcpy(tri_out + (size_t)s * n1, good + (size_t)h * n1, (size_t)n1);
    }
}

/* the whole call, with the outputs of eorb_two_view_reconstruct (hyp_poses: 8 x 27 floats, or NULL).  Returns 0. */
int tvr_reconstruct(const float* pts1, int n1, const float* pts2, int n2, const int32_t* match12, int N, const int32_t* sets, int iters,
                    const float* K, const eorb_tvr_recon_params* p, eorb_tvr_recon_result* res, float* R21, float* t21, float* p3d,
                    uint8_t* triangulated, uint8_t* trans_inliers, float* hyp_poses)
{
    float H21[9], F21[9], SH = 0, SF = 0, poses[27 * 8], cos_sel[8] = {0};
    int32_t bh = -1, bf = -1, n_good[8] = {0};
    uint8_t* ih = (uint8_t*)malloc((size_t)N);
    uint8_t* jf = (uint8_t*)malloc((size_t)N);
    uint8_t* sel = (uint8_t*)malloc((size_t)N);
    uint8_t* good = (uint8_t*)calloc(8 * (size_t)n1, 1);
    float* p8 = (float*)calloc(8 * 3 * (size_t)n1, sizeof(float));
    tvr_ransac(pts1, n1, pts2, n2, match12, N, sets, iters, p->sigma, p->th_score, p->th_f, 3, H21, &SH, &bh, ih, F21, &SF, &bf, jf,
               NULL, NULL, NULL, NULL);
    const int nh = tvr_decide(SH, SF, bh, bf, H21, F21, ih, jf, N, K, p, res, poses, sel, trans_inliers);
    if (nh > 0)
        tvr_check_rt(pts1, n1, pts2, n2, match12, N, sel, K, 4.0f * (p->sigma * p->sigma), p->min_parallax_crt, p->min_triangulated, poses, nh,
                     n_good, good, p8, cos_sel, NULL);
    tvr_finish(p, res, poses, n1, n_good, cos_sel, good, p8, R21, t21, p3d, triangulated);
    if (hyp_poses) memcpy(hyp_poses, poses, sizeof poses);
    free(ih); free(jf); free(sel); free(good); free(p8);
    return 0;
}
