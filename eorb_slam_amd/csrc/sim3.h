// Sim3Solver on the device: the argument block and launcher shared by sim3.hip (kernels) and eorb_fe.hip (C ABI).
#pragma once
#include <stdint.h>
#include "eorb_ctx.h"
#include "kb8_dev.h"
#include "ransac_set.h"

namespace eorb {

// one problem as the kernels read it
struct S3Prob : RansacProb {
    int fix_scale;
    float Rt1[12], Rt2[12];
    WarpCam cam1, cam2;
};
// one hypothesis as s3_hyp_kernel leaves it: R[9], t[3], s (T12 and T21 go to it_T12 / it_T21)
constexpr int kS3HypFloats = 13;
// eorb_sim3_result as words: converged, best_it, n_inliers, iterations_used, T12[16], R12[9], t12[3], s12
constexpr int kS3ResWords = 33;

// eorb_sim3_ransac; every pointer is device memory
struct S3Args : RansacSet<S3Prob> {
    const float* Xw1; const float* Xw2; const float* sigma2_1; const float* sigma2_2;      // per correspondence
    const int32_t* sets;                                                                   // 3 per hypothesis
    float* X1; float* X2; float2* p1; float2* p2; float* b1; float* b2;                    // s3_prepare_kernel: mvX3Dc, mvP?im?, the bounds
    float* hyp;                                                                            // kS3HypFloats per hypothesis
    // results (zero on entry): K * kS3ResWords | inliers | it_inliers | it_scale | it_T12 | it_T21
    int32_t* res; uint8_t* inliers; int32_t* it_inliers; float* it_scale; float* it_T12; float* it_T21;
};
int sim3_ransac_dev(eorb_ctx* c, const S3Args& a);

}  // namespace eorb
