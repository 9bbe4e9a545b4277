// MLPnPsolver on the device: the argument block and launcher shared by mlpnp.hip (kernels) and eorb_fe.hip (C ABI).
#pragma once
#include <stdint.h>
#include "eorb_ctx.h"
#include "kb8_dev.h"
#include "ransac_set.h"

namespace eorb {

// one problem as the kernels read it
struct PnpProb : RansacProb {
    int first_it, best_it;
    float th2;
    WarpCam cam;
};
// eorb_mlpnp_result as words: stop_it, iterations_used, best_it, n_best, refined, n_inliers, Tcw[16]
constexpr int kPnpResWords = 22;
// per correspondence of pnp_compute_pose's Gauss-Newton step: two Jacobian rows of 6, then the two residuals
constexpr int kPnpRowDoubles = 14;

// eorb_mlpnp_ransac; every pointer is device memory
struct PnpArgs : RansacSet<PnpProb> {
    const float* p2d; const float* Xw; const float* sigma2;          // per correspondence
    const int32_t* sets;                                             // 6 per hypothesis
    double* f; double* ns; double* X; float* bound;                  // pnp_prepare_kernel: bearing vector, nullspace (3x2), point, mvMaxError
    // results (zero on entry): K * kPnpResWords | inliers | it_inliers | it_refine_inliers | it_Rt
    int32_t* res; uint8_t* inliers; int32_t* it_inliers; int32_t* it_refine; double* it_Rt;
};
int mlpnp_ransac_dev(eorb_ctx* c, const PnpArgs& a);

}  // namespace eorb
