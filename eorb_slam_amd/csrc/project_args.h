// Argument blocks of the map-point projector, shared by project.hip (kernels) and eorb_fe.hip (C ABI).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "eorb_ctx.h"
#include "kb8_dev.h"

namespace eorb {

// eorb_view with its tables on the device
struct ProjView {
    float R[9], t[3], Ow[3];
    WarpCam cam;
    float minX, maxX, minY, maxY, mbf;
    int nlevels; float log_scale; const float* sf;
    int ak_nlevels; float ak_log_scale; const float* ak_sf;
};

// eorb_frustum_out on the device (every array present) + the records search_proj_map_dev / twocam_walk_dev read
struct FrustumDev {
    uint8_t* in_view; float2* proj_xy; float* proj_xr; int32_t* level; float* view_cos; float* depth; float* level_scale; uint8_t* reason;
    float4* rec;           // proj x, proj y, view cos, level scale
    uint8_t* search;       // in_view and not beyond thFarPoints: the matcher's "valid"
};

struct FrustumArgs {       // mode A: Frame::isInFrustum
    ProjView V[2]; FrustumDev O[2];
    int nviews, M;
    const float* pos; const float* normal; const float* min_dist; const float* max_dist; const uint8_t* skip; const uint8_t* is_orb;
    float cos_limit; int far; float th_far;
    int32_t* n_in_view;
};

struct LastArgs {          // mode B: SearchByProjection(CurrentFrame, LastFrame)
    ProjView V; int has_r; WarpCam cam_r; float Trl[12];
    int n; const float* pos; const uint8_t* skip; const eorb_keypoint* kps; const uint8_t* is_orb;
    uint8_t* valid; float2* uv; float* proj_ur; float* level_scale; float2* uv_r;
    float* rec3;           // u, v, level scale: the last-frame matcher's query record
};

struct KfArgs {            // mode C: SearchByProjection(CurrentFrame, pKF, sAlreadyFound)
    ProjView V;
    int n; const float* pos; const float* min_dist; const float* max_dist; const uint8_t* skip; const uint8_t* is_orb;
    uint8_t* valid; float2* uv; int32_t* level; float* level_scale; float* dist3d;
    float* rec3;
    const eorb_keypoint* kf_kps; eorb_keypoint* q_kps;      // optional: the matcher's query keypoints, octave = class_id = level
};

// pose, camera and image bounds of one keyframe of the KeyFrame-side modes (an eorb_view without its tables: the batch shares one)
struct KfPose {
    float R[9], t[3], Ow[3];
    WarpCam cam;
    float minX, maxX, minY, maxY, mbf;
};

// per (keyframe, map point) outputs of modes D and E, K * M entries each: what kf_radius_dev (match.hip) reads, plus the test aids
struct KfSideDev {
    uint8_t* valid; float2* uv; int32_t* level; float* radius; float* q_ur; float* dist3d; uint8_t* reason;
};

struct KfSideArgs {        // mode D: Fuse (both overloads), SearchByProjection(pKF, Scw, ...)
    const KfPose* V; int K, M;                                  // V: device array of K poses
    int nlevels; float log_scale; const float* sf; float th;
    const float* pos; const float* normal; const float* min_dist; const float* max_dist;
    const uint8_t* skip;                                        // K * M or NULL
    KfSideDev O;
};

// mode D for MixedMatcher: M flags (NULL = every point ORB) and the batch's AKAZE tables (ak_nlevels == 0: none)
struct KfSideArgsMixed : KfSideArgs { const uint8_t* mp_is_orb; int ak_nlevels; float ak_log_scale; const float* ak_sf; };

struct Sim3Half {          // mode E, one direction: p3Dc_b = sRba * (Raw * p3Dw + taw) + tba, searched in keyframe b
    float Ra[9], ta[3], sRb[9], tb[3];
    float fx, fy, cx, cy;                                       // pKF1's in both directions (:1746-1749)
    float minX, maxX, minY, maxY;                               // keyframe b's IsInImage
    int nlevels; float log_scale; const float* sf;              // keyframe b's tables
    int n; const float* pos; const float* min_dist; const float* max_dist; const uint8_t* skip;
};

struct Sim3Args {          // both halves in one launch; outputs as a 2 x M batch (M >= both n, the tail of a half invalid)
    Sim3Half H[2]; int M; float th;
    KfSideDev O;
};

int project_frustum_dev(eorb_ctx* c, const FrustumArgs& A);
int project_kfside_dev(eorb_ctx* c, const KfSideArgs& A);
int project_kfside_mixed_dev(eorb_ctx* c, const KfSideArgsMixed& A);
int project_sim3_dev(eorb_ctx* c, const Sim3Args& A);
int project_last_dev(eorb_ctx* c, const LastArgs& A);
int project_kf_dev(eorb_ctx* c, const KfArgs& A);

}  // namespace eorb
