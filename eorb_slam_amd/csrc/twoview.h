// Two-view reconstruction on the device: argument blocks and launchers shared by twoview.hip (kernels) and eorb_fe.hip (C ABI).
#pragma once
#include <stdint.h>
#include "eorb_ctx.h"

namespace eorb {

// the matrices Normalize leaves for every iteration (tv_normalize_kernel): T1, T2, T2.inv(), T2.t(), 9 floats each
constexpr int kTvHdrFloats = 36;
// one hypothesis as tv_hyp_kernel leaves it: H21i then H12i, or F21i then nine unused floats
constexpr int kTvHypFloats = 18;

// eorb_two_view_ransac; every pointer is device memory
struct TvRansacArgs {
    const float2* pts1; const float2* pts2; int n1, n2;
    const int32_t* match12; int N;
    const int32_t* sets; int iters;
    float sigma, th_score, th_f;
    float2* pn1; float2* pn2;           // the normalised keys
    float* hdr;                         // kTvHdrFloats
    float* hyp;                         // 2 * iters * kTvHypFloats: the H hypotheses, then the F hypotheses
    uint8_t* inl;                       // 2 * iters * N: vbCurrentInliers of every hypothesis
    // results: {SH, SF, best_it_h, best_it_f, H21[9], F21[9]} as 22 words | inliers_h[N] | inliers_f[N] | it_score_h | it_score_f | it_H | it_F
    float* res; uint8_t* inliers_h; uint8_t* inliers_f; float* it_score_h; float* it_score_f; float* it_H; float* it_F;
};
int twoview_ransac_dev(eorb_ctx* c, const TvRansacArgs& a);

// eorb_two_view_check_rt; pose = R[9] t[3] P2[12] O2[3]
constexpr int kTvPoseFloats = 27;
struct TvCheckRtArgs {
    const float2* pts1; const float2* pts2; int n1;
    const int32_t* match12; int N; const uint8_t* inliers;
    float K[9]; float th2, min_parallax_crt; int min_triangulated;
    const float* poses; int Kp;
    int32_t* n_good; float* cos_sel; uint8_t* good; float* p3d;      // good | p3d are contiguous and zero on entry
    float* cos_all;                                                     // Kp * N: cosParallax of a counted match, -2 otherwise
    const int32_t* Kp_dev = nullptr;    // eorb_two_view_reconstruct: the hypothesis count tv_decide_kernel left (0, 4 or 8 <= Kp); null: Kp
};
int twoview_check_rt_dev(eorb_ctx* c, const TvCheckRtArgs& a);

// eorb_two_view_reconstruct: what tv_decide_kernel and tv_resolve_kernel add around the two stages above; every pointer is device memory
struct TvReconArgs {
    const float* rres; const uint8_t* inliers_h; const uint8_t* inliers_f;      // what tv_finish_kernel left (TvRansacArgs::res, ...)
    int N, n1;
    float K[9]; eorb_tvr_recon_params p;
    eorb_tvr_recon_result* res;         // zero on entry, as every output below
    float* poses;                       // 8 * kTvPoseFloats: the hypotheses, zeros past the count
    int32_t* n_hyp;                     // the device-side hypothesis count for CheckRT
    uint8_t* sel_inl;                   // N: the flags of the chosen model, CheckRT's vbMatchesInliers
    uint8_t* trans_inl;                 // N: vbTransInliers (INFO form)
    const int32_t* n_good; const float* cos_sel; const uint8_t* good8; const float* p3d8;      // CheckRT's results for 8 poses
    float* R21; float* t21; uint8_t* tri; float* p3d;                                          // the two result slots
};
// the RANSAC, tv_decide_kernel, CheckRT on its hypotheses, tv_resolve_kernel; R.res / inliers_* must be A.rres / inliers_*, and
// T.poses / inliers / Kp_dev must be A.poses / sel_inl / n_hyp with T.Kp = 8
int twoview_reconstruct_dev(eorb_ctx* c, const TvRansacArgs& R, const TvReconArgs& A, const TvCheckRtArgs& T);

}  // namespace eorb
