// CreateNewMapPoints on the device: the argument block and launcher shared by newpts.hip (kernels) and eorb_fe.hip (C ABI).
#pragma once
#include <stdint.h>
#include "eorb_ctx.h"
#include "kb8_dev.h"

namespace eorb {

// what the stage reads of an eorb_view
struct NpView { float R[9], t[3], Ow[3]; WarpCam cam; float mbf; };
// one neighbour: its rows in the concatenated arrays, numAllKPtsLeft(), KeyFrame::mb, its left and right view
struct NpKf { int32_t row0, nrows, nleft2; float mb; NpView v[2]; };
// the per-keypoint arrays of eorb_newpts_side; any of them may be null
struct NpSide { const float* sigma2; const float* scale; const uint8_t* is_orb; const float* uright; const float* depth; const float* raw_xy; };

constexpr int kNpSlotsPerBlock = 1024;      // slots of match12 one workgroup of np_pair_kernel compacts

// eorb_new_map_points; every pointer is device memory
struct NpArgs {
    const eorb_keypoint* kps1; const eorb_keypoint* kps2; int n1, K, nleft1, form;
    const NpView* v1; float mb1;                       // pKF1: left, right
    const NpKf* kf;
    NpSide s1, s2;
    const float* level_scale; const float* level_sigma2; int nlevels;
    float rf_orb, rf_ak; int far_points; float th_far;
    const int32_t* match12;
    uint8_t* tmp;                                      // 2 per slot: the pair's exit under the ORB factor, under the AKAZE factor
    int32_t* pstar;                                    // smallest position of an AKAZE-AKAZE pair (:545-546; 0x7f7f7f7f on entry)
    // results, zero on entry
    uint8_t* status; float* x3d; uint8_t* branch; float* cosp; int32_t* n_new;
};
int new_map_points_dev(eorb_ctx* c, const NpArgs& a);

}  // namespace eorb
