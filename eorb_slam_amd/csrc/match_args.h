// Argument blocks and launchers of the matchers, shared by match.hip (kernels) and eorb_fe.hip (C ABI).
#pragma once
#include <stdint.h>
#include "eorb_ctx.h"
#include "bow_plan.h"

namespace eorb {

struct GridB { float minX, minY, invW, invH; };
inline GridB grid_b(const eorb_grid_bounds& gb) { return GridB{gb.minX, gb.minY, gb.invW, gb.invH}; }

// a searched frame on the device; is_orb, uright: NULL without AKAZE features / outside the rectified-stereo configurations
struct FrameDev { const eorb_keypoint* kps; int n; const uint8_t* desc; int stride; const uint8_t* is_orb; const float* uright; };

// SearchByProjection(CurrentFrame, LastFrame / pKF) (match.hip launch_win<1>): per query keypoint its record uvs = (u, v, levelScale);
// q_ur (stereo, with f.uright): the queries' right coordinates
struct ProjLastArgs {
    FrameDev f; GridB g;
    const eorb_keypoint* q_kps; int nq; const uint8_t* q_is_orb; const uint8_t* valid; const float* uvs;
    const uint8_t* mp_desc; const uint8_t* mp_obs; const float* q_ur;
    float th; int mode, checkOri, dist_th; int32_t* slots; int32_t* nmatches;
};

// SearchByProjection(Frame, map points) (match.hip launch_win<2>): per map point its record qf = (projX, projY, viewCos, levelScale);
// q_ur (stereo, with f.uright): mTrackProjXR
struct ProjMapArgs {
    FrameDev f; GridB g;
    int M; const uint8_t* in_view; const float4* qf; const int32_t* level;
    const uint8_t* mp_desc; const uint8_t* mp_obs; const uint8_t* mp_is_orb; const float* q_ur;
    float th, nnratio; int32_t* slots; int32_t* nmatches;
};

// DBoW2::FeatureVector as CSR, device resident: node ids ascending, off[nn + 1], feature indices
struct FeatVec { const uint32_t* nodes; const int32_t* off; const int32_t* idx; int nn; };

// SearchByBoW: the block of one pair (match.hip bow_node; bow_pair makes it from BowBatchArgs)
struct BowArgs {
    const eorb_keypoint* kf_kps; const uint8_t* kf_desc; const uint8_t* kf_has_mp; FeatVec kf_fv;
    const eorb_keypoint* f_kps; int n_f; const uint8_t* f_desc; FeatVec f_fv;
    int32_t* match_f; int8_t* bin_f; int32_t* histo; int32_t* nmatches;
    float nnratio; int checkOri;
    int kf_kf;                       // 1: SearchByBoW(KF, KF) (:833-973): output per idx1, vbMatched2 flags, strict TH_LOW
    const uint8_t* f_has_mp; int32_t* match12; int n_kf;
};

struct TriArgs {
    const eorb_keypoint* kps1; int n1; const uint8_t* desc1; int stride1; const uint8_t* elig1; FeatVec fv1;
    const eorb_keypoint* kps2; int n2; const uint8_t* desc2; int stride2; const uint8_t* elig2; FeatVec fv2;
    float epx, epy; float F[9]; const float* scale2; const float* sigma2_2; int nlevels;
    int bCoarse, checkOri;
    int32_t* match12; int8_t* bin1; int32_t* histo; int32_t* nmatches;
};

// SearchForTriangulation with KannalaBrandt8::epipolarConstrain (match.hip search_tri_kb8_batch_kernel); T.F is unused
struct Pose12 { float v[12]; };              // R row-major, t

struct TriKbArgs {
    TriArgs T;
    int nleft1;                                     // numAllKPtsLeft() of pKF1: -1 (monocular) or >= 0 (two cameras); pKF2_k's is TriKbPair::nleft2
    eorb_camera cam1[2], cam2[2];                   // mpCamera, mpCamera2 of pKF1 / pKF2
    const float* sigma2_1;
};

// ---- the node walks over K keyframes per call, a single pair being K = 1 (match.hip search_bow_batch_kernel, search_bow_fisheye_kernel,
// search_tri_batch_kernel, search_tri_kb8_batch_kernel) ----
// Keyframe k of the set: rows row0 .. row0 + nrows - 1 of the concatenated keypoints / descriptors / flags, nodes node0 .. node0 + nn - 1
// of the concatenated node ids, its nn + 1 offsets from off0 and its feature indices from idx0 (offsets and indices relative to the
// keyframe).  One record per pair in a device table that the kernels read with the wave-uniform pair index.
struct KfSlice { int32_t row0, nrows, node0, nn, off0, idx0; };
struct TriPair { float epx, epy, F[9]; };           // F unused by the KannalaBrandt8 walk
struct TriKbPair { int32_t nleft2; float Rt[48]; };   // ll, lr, rl, rr: R12 row-major then t12 (monocular: Rt[0..11])
constexpr int kPairHist = 33;                       // per pair: 32 rotation bins, then nmatches

// A = the block of one pair with the shared side filled in and, on the set's side, the bases of the concatenated arrays;
// match_f / match12 / bin_f hold K slices of n_out entries, histo K * kPairHist
struct BowBatchArgs { BowArgs A; const KfSlice* kf; int K, n_out, max_nn; };
struct TriBatchArgs { TriArgs T; const KfSlice* kf; const TriPair* pair; int K; };
struct TriKbBatchArgs { TriKbArgs K; const KfSlice* kf; const TriPair* pair; const TriKbPair* kb; int nk; };

// the KeyFrame-side radius search (match.hip kf_radius_batch_kernel, kf_radius_seq_kernel) over K keyframes, a single keyframe being
// K = 1: keypoints / descriptors / cells / uright of all keyframes concatenated, keyframe k = rows kf_off[k] .. kf_off[k + 1] - 1 with
// grid bounds g[k]; the query arrays hold K * M queries, (k, m) at k * M + m; the descriptor of query (k, m) is row m of
// q_desc + k * q_desc_kstride (0: all keyframes share the M rows).  taken (K = 1 only): the in-order form, vpMatched in and out
struct RadBatchArgs {
    const eorb_keypoint* kps; const uint8_t* desc; int stride;
    uint16_t* cell;                                 // per keypoint: ix*48+iy or 0xFFFF (Frame::PosInGrid); the launcher fills it (kf_cells_batch_kernel)
    const float* uright;                            // Fuse, rectified stereo: mvuRight per keypoint (>= 0: has one); q_ur: the map points' predicted right coordinates
    const int32_t* kf_off; const GridB* g; int K, M;
    const uint8_t* valid; const float* uv; const float* radius; const int32_t* level; const float* q_ur;
    const uint8_t* q_desc; size_t q_desc_kstride;
    const float* inv_sigma2; int nlevels;
    int32_t* best_idx; int32_t* best_dist;
    uint8_t* taken; float accept_thr;
};

// one keyframe of it as radius_scan reads it: the device-side view that rad_pair (match.hip) makes from the block and a keyframe index
struct RadArgs {
    const eorb_keypoint* kps; int n; const uint8_t* desc; int stride; GridB g; const uint16_t* cell;
    int M; const uint8_t* valid; const float* uv; const float* radius; const int32_t* level; const uint8_t* q_desc;
    const float* inv_sigma2; int nlevels;
    const float* uright; const float* q_ur;
    uint8_t* taken; float accept_thr;
    int32_t* best_idx; int32_t* best_dist;
};

// the mixed kernels' arguments (MixedMatcher's KeyFrame-side forms): the ORB ones plus mp_is_orb[M] (NULL = every map point ORB; one
// array for all keyframes of a batch) and kp_inv_sigma2 = getKPtInvLevelSigma2(idx) per keypoint (NULL = no reprojection gate; inv_sigma2
// / nlevels are unused).  The keypoints' types are bit 15 of their cell words (kf_cells_batch_kernel<true>).
struct RadArgsMixed : RadArgs { const uint8_t* mp_is_orb; const float* kp_inv_sigma2; };
struct RadBatchArgsMixed : RadBatchArgs { const uint8_t* mp_is_orb; const float* kp_inv_sigma2; };

// DBoW2 vocabulary tree, device resident (TemplatedVocabulary::m_nodes flattened; node 0 = root)
struct BowVoc {
    int nnodes, L;
    const int32_t* child_off; const int32_t* child_ids; const uint8_t* node_desc; const int32_t* word_id; const double* weight;
};

// two-camera tracking matchers (match.hip twocam_walk_kernel): the searched frame holds nL left keypoints, then nR right ones
constexpr int kTcMaxKps = 8192;                  // nL + nR: 16 B of LDS each next to the 2 x 3072 cell starts
struct TcArgs {
    const eorb_keypoint* kps; int nL, nR; const uint8_t* desc; int stride; GridB g;
    int nq; const uint8_t* mp_desc; const uint8_t* mp_obs; float th; float nnratio;
    // map points (KIND 0): x, y, viewCos, levelScale per camera; predicted levels; stereo links of the frame
    const uint8_t* in_view; const float4* qf; const int32_t* qlevel;
    const uint8_t* in_view_r; const float4* qf_r; const int32_t* qlevel_r;
    const int32_t* l2r; const int32_t* r2l;
    // last frame (KIND 1): u, v, u_r, v_r, levelScale per query; the query keypoints (octave, angle); window mode
    const uint8_t* valid; const float* quv; const eorb_keypoint* qkps; int mode; int checkOri;
    int32_t* rec;                                // KIND 1: (slot << 5 | bin) of every match in order, 2 * nq entries
    int32_t* slots; int32_t* nmatches;
};

// ---- the launchers of match.hip: window matchers, node walks, two-camera frames (kind: 0 map points, 1 last frame), the rest ----
int search_init_dev(eorb_ctx* c, int npairs,
                    const eorb_keypoint* kps1, const int32_t* n1, size_t kp1_stride, const uint8_t* desc1, int dstride1, size_t desc1_slice,
                    const uint8_t* is_orb1,
                    const eorb_keypoint* kps2, const int32_t* n2, size_t kp2_stride, const uint8_t* desc2, int dstride2, size_t desc2_slice,
                    const uint8_t* is_orb2, int cap1, int cap2,
                    eorb_grid_bounds gb, float* prev_matched, int32_t* matches12, int windowSize, float nnratio,
                    int checkOri, int32_t* nmatches);
int search_proj_last_dev(eorb_ctx* c, const ProjLastArgs& P);
int search_proj_map_dev(eorb_ctx* c, const ProjMapArgs& P);
// the node walks over K pairs; name: the profile scope of the entry point.  scratch (keyframe-to-keyframe form): the vbMatched2 flags, one
// per row of the set; nL >= 0: the frame holds nL left features, then right ones; K: the KannalaBrandt8 walk (K->K.T is the block)
int search_bow_batch_dev(eorb_ctx* c, const char* name, const BowBatchArgs& B, int32_t* scratch, int nscratch, int nL = -1);
int search_tri_batch_dev(eorb_ctx* c, const char* name, const TriBatchArgs& B, const TriKbBatchArgs* K = nullptr);
int kb8_tri_batch_dev(eorb_ctx* c, const eorb_camera* cam1, const eorb_camera* cam2, const float* Rt, const eorb_keypoint* kps1,
                      const eorb_keypoint* kps2, int n, const float* sig1, const float* sig2, float* out);
int twocam_walk_dev(eorb_ctx* c, int kind, const TcArgs& A);
int fisheye_lowe_dev(eorb_ctx* c, const uint8_t* d_descL, const uint8_t* d_descR, int cap, int32_t* d_lap, int32_t* d_idx2,
                     int32_t* d_kdist2, int32_t* d_cand, int32_t* d_dist2);
// the radius search of B (its cells first); name: the profile scope of the entry point; mixed: the MixedMatcher kernels (the ORB ones
// take B's base); B.taken chooses the in-order kernel; d_kp_is_orb: the keypoints' types for the cell words (mixed, may be NULL)
int kf_radius_dev(eorb_ctx* c, const char* name, bool mixed, const RadBatchArgsMixed& B, int ntotal, const uint8_t* d_kp_is_orb);
int sim3_agree_dev(eorb_ctx* c, const int32_t* best_idx, const int32_t* best_dist, int M, int N1, int N2, int th_high,
                   int32_t* vn1, int32_t* vn2, int32_t* match12, int32_t* nfound);
int bow_transform_dev(eorb_ctx* c, const uint8_t* d_desc, int n, int stride, const BowVoc& V, int levelsup, int weighting, int norm,
                      uint32_t* d_word_of, double* d_w_of, uint32_t* d_node_of, uint32_t* d_bow_word, double* d_bow_val,
                      uint32_t* d_fv_node, int32_t* d_fv_off, int32_t* d_fv_idx, int32_t* d_counts);
int window_match_dev(eorb_ctx* c, const uint8_t* d_q, int nq, int q_stride, const uint8_t* d_t, int t_stride, const int32_t* d_off,
                     const int32_t* d_cand, int32_t* d_out);
int distinctive_dev(eorb_ctx* c, const uint8_t* d_desc, const int32_t* d_offsets, int M, int32_t* d_best);
int sort_response_dev(eorb_ctx* c, const eorb_keypoint* d_kps, int n, int32_t* d_perm);
int bf_knn2_dev(eorb_ctx* c, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int32_t* d_idx2, int32_t* d_dist2);

}  // namespace eorb
