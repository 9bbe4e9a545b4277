// eorb_ctx.h -- internal context shared by the translation units of libeorb_fe.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/eorb_fe.h"
#include "ev_plan.h"
#include "eorb_options.h"

namespace eorb {

constexpr int kMaxLevels = 16;
constexpr int kGridCols = 64;       // FRAME_GRID_COLS include/Frame.h:46
constexpr int kGridRows = 48;       // FRAME_GRID_ROWS include/Frame.h:45

struct DevBuf {
    void*  p = nullptr;
    size_t cap = 0;
};

struct ProfEntry {
    std::string name;
    double total_ms = 0;
    int64_t launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

struct ChunkDesc {       // one binning chunk = a run of <= kChunk consecutive events of one slice
    int64_t start;       // index of the first event (into the batch's event array)
    int32_t n;
    int32_t slice;
};

// geometry of one pyramid level (ComputePyramid / ComputeKeyPointsOctTree, ORBextractor.cc:784-808,1240-1265)
struct LevelGeom {
    int w, h;            // level (ROI) size
    int bw, bh;          // bordered buffer size (w+2E, h+2E)
    int buf_off;         // byte offset of the bordered buffer inside a slice's pyramid block
    int roi_off;         // byte offset of the un-bordered (w*h) planes (score / blur) inside a slice block
    int minBX, minBY, maxBX, maxBY;
    int nCols, nRows, wCell, hCell;
    int cell_off;        // index of this level's first cell in the per-slice cell arrays
    int cand_cap;        // candidate capacity of the level
    int cand_off;        // offset (entries) of the level's candidate array inside a slice block
    int nfeat;           // mnFeaturesPerLevel
    int kp_cap;          // max(nfeat + slack, 4 * octree roots)
    int kp_off;          // offset (entries) of the level's keypoint array inside a slice block
    int xtab_off, ytab_off;   // resize coefficient tables (int offsets into the table buffer)
    int xmax;            // first dx whose source column is clamped (HResize)
    float scale;         // mvScaleFactor[level]
    int patch_size;      // (int)(31*scale)
    int node_cap;        // octree node pool capacity
};

struct OrbState {
    bool configured = false;
    eorb_orb_params p{};
    int W = 0, H = 0, edge = 0, nlevels = 0;
    float sf[kMaxLevels]{}, inv_sf[kMaxLevels]{};
    int nfeat[kMaxLevels]{};
    int umax[16]{};
    LevelGeom lv[kMaxLevels]{};
    int pyr_bytes = 0;       // per slice: all bordered level buffers
    int roi_bytes = 0;       // per slice: all un-bordered level planes
    int ncells = 0;          // per slice: cells over all levels
    int cell_cap = 0;        // candidates per cell (capacity)
    int cand_total = 0;      // per slice: sum of cand_cap
    int kp_total = 0;        // per slice: sum of kp_cap  (= eorb_orb_max_keypoints)
    int max_out = 0;
    int oct_lds[2] = {0, 0};       // dynamic LDS bytes of the octree kernel, per placement (single frames / many workgroups)
    int oct_direct_cap[2] = {0, 0};
    int oct_dyn[2] = {0, 0}, oct_dyn_lds[2] = {0, 0};   // dynamic placement in use (its direct-pass cap, -1: none), its LDS bytes
    int oct_all_lds[2] = {0, 0};   // every item of that placement is in LDS: the kernel variant with LDS-typed pointers
    int oct_scratch[2] = {0, 0};   // per (slice, level) global scratch bytes
    // what the last call left in the context's pyr / blur / cell_cnt / cell_cand buffers (eorb_debug_stage): its slices (0: nothing),
    // whether it blurred the levels, whether it ran FAST
    int last_B = 0; bool last_blur = false, last_cells = false;
    DevBuf tabs;             // resize tables (short/int), level geometry, pattern, umax
    DevBuf geom;
};

// eorb_set_calibration in the form the kernels of calib.hip take by value: everything widened to double on the host once, RR = P(3x3) * R
// (cv::undistortPoints / cv::fisheye::undistortPoints)
struct CalibDev {
    int model, gate;         // gate: MyCalibrator::isDistorted (:46-50) for the point calls, dist[0] != 0.0 for ComputeImageBounds
    double fx, fy, cx, cy, ifx, ify;
    double k[12];            // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 (absent: 0); fisheye: k[0..3]
    double RR[9];
};

// KeyFrameDatabase on the device (kfdb.hip): no inverted file -- every list of the reference's holds its keyframes in the order of their
// latest add(), so a live keyframe's BowVector and an add sequence number say the same
struct KfdbSlot { uint32_t off; int32_t n; uint32_t seq, pad; };      // words [off, off + n) of the pools; n < 0: the slot is free
struct KfdbState {
    DevBuf tab, words, vals, score[2];          // KfdbSlot per slot | word ids | values | stored score per slot and query family
    int slot_cap = 0; int64_t word_cap = 0, word_used = 0, word_live = 0;
    int n_slots = 0, n_live = 0; uint32_t next_seq = 0;
    std::vector<KfdbSlot> h_tab;                // the host's copy of tab
    std::vector<int> free_slots;                // min-heap: the lowest free slot is reused first
};

// A set of positions and the device tables derived from it.  The context holds three (eorb_ctx: maps, dd, pd); every function that builds
// or reads the tables receives the set it works on.
struct PosTables {
    DevBuf lut, src_info, stamps;                // float2 per position | its integer position (ev_src_info_kernel) | its stamp (ev_stamp_kernel)
    DevBuf sl_tab, sl_tile, sl_rows;             // slot form (ev_slots.hip): per position its tiles / slot numbers, per tile its rows; valid when sl_ok
    int w = 0, h = 0, check = 1;                 // the positions as a (w x h) sensor; check: checkInImage of the maps
    int key_W = -1, key_H = -1, key_mode = -1; float key_sigma = -1.f;      // what the derived tables were built for (-1: nothing)
    int sl_ok = 0, sl_null = 0; size_t sl_info_off = 0;
    int sl_launched = 0;                         // assignment kernels launched, their info on its way to the read-back buffer (ev_slots_prepare_launch / _finish)
    int src_info_done = 0;                       // src_info launched ahead of ev_raw_tables (float bulk path)
};

}  // namespace eorb

struct eorb_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    bool prof = false;
    std::string prof_only;                       // ",name,name,": only these scopes are timed (empty: all)
    std::vector<eorb::ProfEntry> profs;
    std::vector<hipEvent_t> ev_pool;

    // accumulation workspaces
    eorb::DevBuf ev16, chunks, segoff, entries, img_f32, img_u8, minmax, tile_order, order_hist;
    // raw sensor events: undistortion maps (float2 per sensor pixel) and the tables derived from them
    eorb::PosTables maps;
    eorb::DevBuf ev_info, ev_stamps;              // float events of the per-slice calls: the same tables per EVENT (ev_direct_slices_dev)
    eorb::DevBuf sl_trace; long long sl_trace_n = 0;
    // per-batch workspaces of the slot form, one set per part of a batch (a batch runs as two halves only on request: "slot_halves")
    struct SlotWS { eorb::DevBuf chunks, segoff, entries, tile_order, plan, hot, rec16; };
    SlotWS sl_ws[2];
    // its streams (made together, ev_slots.hip sl_streams): sl_side = the register-row kernel (high priority), sl_pstream = the plan,
    // sl_gstream = the LDS gather of one half while the next half is binned; five events per part
    static constexpr int kSlotEvents = 10;
    hipStream_t sl_side = nullptr, sl_pstream = nullptr, sl_gstream = nullptr; hipEvent_t sl_ev[kSlotEvents] = {};
    int sl_last_parts = 0, sl_last_nb[2] = {0, 0};      // the last slot-form call: its parts, (slices x tiles) of each
    int sl_rank_ok = -1;
    int ncu = 0;                                 // compute units of c->device (per context: a second context may sit on another GPU)
    std::vector<const void*> sl_optins;          // kernel instantiations whose dynamic-LDS opt-in was made on c->device (ev_slots.hip sl_optin)
    int sl_last_rank = -1, sl_last_chunk = 0;    // the scatter the last slot-form call ran (1 rank form, 0 ballot form), its chunk size
    int sl_last_binning = -1;                    // ... and its whole SlotBinPlan (ev_plan.h slot_binning_code)
    int* rb_pinned = nullptr;                   // 64 ints of pinned host memory: the landing place of small read-backs (position count, slot info)
    long long sl_calls = 0;                      // test hook counter (eorb_debug_counter)
    int accum_route = 0;                         // what served the last ev_accumulate_dev call (ev_plan.h: form | position set | sparse | widened)
    // float events in bulk: the distinct positions of a call are tabulated in a hash table (dd.lut, 8 bytes per row: the positions as a
    // 65 536-wide sensor) and the raw path runs on the tables of that per-call set (ev_accumulate_dev)
    eorb::PosTables dd;
    eorb::DevBuf dd_ev, dd_cnt;
    // ... and across calls: once a call's positions are known, the next calls of the context look theirs up in a frozen dictionary
    // (compact hash -> dense id < 65 536; pd: the positions per id as a (pd_K x 1) sensor, their tables) and only fall back to the
    // per-call tabulation when a new position turns up
    eorb::PosTables pd;
    eorb::DevBuf pd_hash, pd_cnt;
    int pd_valid = 0, pd_K = 0, pd_W = 0, pd_H = 0, pd_cooldown = 0; float pd_sigma = 0.f;
    int dd_keep = 0;                             // the per-call position table holds an earlier call's positions and is extended, not cleared
    long long pd_hits = 0, pd_misses = 0;        // calls served by the dictionary / calls that found a new position (eorb_debug_counter)
    eorb::DevBuf focus_sd;                       // measureImageFocus: per-patch deviations
    // extractor workspaces
    eorb::OrbState orb;
    eorb::DevBuf pyr, score, blur, cell_cnt, cell_cand, lvl_cnt, lvl_kp, kp_angle, out_kp, out_desc, out_oob,
        out_n, oct_scratch;
    // matcher workspaces
    eorb::DevBuf win_ws;                 // candidate lists of the two-phase window matchers
    eorb::DevBuf win_total;              // their per-pair entry counters: zero between calls (phase 2 puts its pair's back), win_total_n of them known to be
    size_t win_total_n = 0;
    unsigned lds_optin = 0;              // bit per matcher kernel whose dynamic-LDS opt-in was made on this context's device (match.hip lds_optin)
    eorb::DevBuf arena;                  // host-buffer entry points: all inputs / outputs of one call, one H2D and one D2H copy
    void* dl_pinned = nullptr; size_t dl_cap = 0;      // pinned landing buffer of the D2H copy (the call synchronises before reading it)
    hipEvent_t dl_event = nullptr;                     // recorded behind that copy: what the call waits for
    // cumulative over the context's life (eorb_debug_counter "arena_*"): calls, their arena and input bytes; downloads, their bytes and first offsets
    long long arena_calls = 0, arena_bytes = 0, arena_in_bytes = 0, arena_downloads = 0, arena_download_bytes = 0, arena_download_first = 0;
    // pyramidal LK workspaces; klt_ref_key: the reference frame whose pyramid and derivatives the buffers hold (0 = none)
    eorb::DevBuf klt_pyr, klt_der, klt_scratch;
    unsigned long long klt_ref_key = 0, klt_ref_geo = 0, klt_ref_serial = 0;
    // L1 chain (eorb_ev_slice_extract / eorb_ev_slice_track): the tracker's reference image and points stay on the device
    eorb::DevBuf l1_ref_img, l1_ref_pts;
    int l1_nref = -1, l1_W = 0, l1_H = 0;
    size_t l1_img_off = 0; unsigned long long arena_gen = 0, l1_img_gen = 0;      // the last slice's u8 image inside the arena (eorb_ev_slice_image)
    // eorb_set_calibration: the caller's record, its device form, and the form Frame::ComputeImageBounds uses (pinhole, R = I, P = K)
    bool calib_set = false; eorb_calib calib{}; eorb::CalibDev calib_dev{}, calib_bounds{};
    // DBoW2 vocabulary (device copy) for eorb_bow_transform
    eorb::DevBuf voc;
    int voc_nnodes = 0, voc_L = 0; size_t voc_off[5] = {0, 0, 0, 0, 0};
    eorb::KfdbState kfdb;
    // batched front end
    bool fe_configured = false;
    eorb_fe_config fe{};
    eorb::DevBuf fe_prev_kp, fe_prev_desc, fe_prev_n, fe_pm;
    eorb::DevBuf fe_matches12, fe_nmatches;     // the batch's frame-to-frame matches and counts when the caller passes no buffers for them
    bool fe_has_prev = false;
    // pinned staging: a ring of slots, each guarded by an event recorded right after the H2D copy that reads it, so that
    // back-to-back un-synchronised *_dev calls never overwrite a slot whose copy is still queued
    static constexpr int kPinnedSlots = 4;
    struct PinnedSlot { void* p = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool busy = false, lazy = false; };
    PinnedSlot pinned[kPinnedSlots];
    int pinned_next = 0, pinned_cur = -1;
    // sticky device status word (bits OR-ed by kernels of the *_dev paths: candidate / node-pool / keypoint overflow);
    // read back by eorb_sync / eorb_fe_status
    eorb::DevBuf status;
    // every switch the context runs with (eorb_options.h): opt_created as eorb_create read it from the environment, opt with what
    // eorb_debug_option has set since
    eorb::Options opt, opt_created;
};

namespace eorb {

int  set_err(eorb_ctx* c, int code, const char* fmt, ...);
int  ensure(eorb_ctx* c, DevBuf& b, size_t bytes);
void* pinned(eorb_ctx* c, size_t bytes);        // next free slot of the pinned ring (waits for the slot's previous copy)
void pinned_commit(eorb_ctx* c, bool lazy = false);   // call right after the hipMemcpyAsync that reads the slot; lazy: no event (the caller waits for the stream anyway: pinned_release_lazy)
void pinned_release_lazy(eorb_ctx* c);          // everything enqueued before the caller's last wait has completed
int  hip_check(eorb_ctx* c, hipError_t e, const char* what);
int* readback_buf(eorb_ctx* c);                 // c->rb_pinned, allocated on first use (nullptr: allocation failed)

// scoped per-kernel timing (HIP events on the ctx stream) when profiling is enabled
struct ProfScope {
    eorb_ctx* c; int idx; hipEvent_t a = nullptr, b = nullptr; hipStream_t st = nullptr;
    ProfScope(eorb_ctx* c, const char* name, hipStream_t stream = nullptr);      // stream: where the scope's kernels run (default: the context's)
    ~ProfScope();
};

#define EORB_HIP(c, call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return eorb::hip_check((c), e__, #call); } while (0)
#define EORB_LAUNCH_CHECK(c, what) do { hipError_t e__ = hipGetLastError(); if (e__ != hipSuccess) return eorb::hip_check((c), e__, what); } while (0)

// ev_accum.hip
AccumKnobs accum_knobs(const eorb_ctx* c);      // accum_knobs(c->opt, the build's gather workgroup)
int ev_accumulate_dev(eorb_ctx* c, const void* d_events, int raw, const int64_t* h_offsets, int B, int W, int H,
                      float sigma, int pol, int mode_count, float* d_f32, uint8_t* d_u8, int normalized,
                      uint32_t* d_minmax_enc, bool mm_preset = false, bool distinct_positions = false);
// mm_preset: the caller has initialised the running extremes (the per-slice calls; only the binning-free form takes its word for it)
// distinct_positions: no two float events share a position (warped events): the call runs with dd_min = 0, nothing is tabulated
int ev_direct_slices_dev(eorb_ctx* c, const AccumShape& S, const void* d_events, int raw, const int64_t* beg, const int64_t* end, int B, int W, int H,
                         float sigma, int pol, float* d_f32, uint8_t* d_u8, int normalized, uint32_t* d_minmax_enc, bool mm_preset = false);
int ev_undistort_dev(eorb_ctx* c, const eorb_raw_event* d_raw, size_t n, int W, int H, double tsFactor, eorb_event* d_out, uint32_t* d_blk);
int ev_parse_text_dev(eorb_ctx* c, const char* d_text, size_t nbytes, eorb_raw_event* d_out, size_t max_out, uint32_t h_res[3]);
int ev_decode_minmax(eorb_ctx* c, const uint32_t* d_enc, float* d_out, int B);
int ev_divcheck(eorb_ctx* c, float lo, float hi, float sigma, unsigned long long* bad_out);
int ev_diag_read(unsigned long long* out16);
int ev_trace_read(unsigned long long* out, int n);
int ev_warp_se3_dev(eorb_ctx* c, const eorb_event16* d_in, eorb_event16* d_out, int n, const eorb_camera* cam, double angle,
                    const double axis[3], const double tt[3], float medDepth, const float* d_depth);
int ev_warp_se2_dev(eorb_ctx* c, const eorb_event16* d_in, eorb_event16* d_out, int n, const eorb_camera* cam, const float* params, int nparams);
int ev_focus_dev(eorb_ctx* c, const float* d_img, int nimg, int W, int H, float* d_out);
int ev_cvnormalize_dev(eorb_ctx* c, const float* d_img, int npix, uint32_t* d_mm, uint8_t* d_out);
int ev_mathhash(eorb_ctx* c, int which, uint32_t lo_bits, uint32_t hi_bits, unsigned long long* out);
int ev_cvnormalize_n_dev(eorb_ctx* c, const float* d_imgs, int nimg, int npix, uint32_t* d_mm, uint8_t* d_outs);
int ev_contest_select_dev(eorb_ctx* c, const float* d_focus_img, const int img_of[4], int half_img, const uint8_t* d_u8s, int npix,
                          float* d_focus_out, int* d_winner, uint8_t* d_out);
int ev_kp_points_dev(eorb_ctx* c, const eorb_keypoint* d_kps, const int32_t* d_n, int cap, float* d_pts);
// ev_slots.hip
int ev_slots_prepare_launch(eorb_ctx* c, PosTables& T, int W, int H, int h, int TX, int TY);
int ev_slots_prepare(eorb_ctx* c, PosTables& T, int W, int H, int h, int TX, int TY, const float* d_stamps /* nullptr: taps from T.lut */, int stamp_stride, int SWP,
                      float two_sig2, float norm);
struct SlotDict {              // float events looked up in the context's position dictionary by the count pass (ev_slots.hip)
    const uint4* hash; uint32_t mask; uint32_t* rec; int* miss;
    int rec2;                  // the dictionary holds fewer than 65 535 positions: rec is written as 2-byte records (0xffff = none), else 4-byte
};
int ev_slots_accumulate(eorb_ctx* c, const PosTables& T, const AccumShape& S, const void* d_events, int stride, const int64_t* h_offsets, int B, int W, int H,
                        float* d_f32, uint32_t* d_minmax_enc, const SlotDict* dict = nullptr);
int ev_slots_trace_read(eorb_ctx* c, unsigned long long* out, long long max_records);
// klt.hip
int klt_track_dev(eorb_ctx* c, const uint8_t* d_prev, const uint8_t* d_next, int W, int H, int stride, const float* d_prev_pts,
                  float* d_next_pts, int n, int win, int maxLevel, int maxCount, double epsilon, int flags, float minEig,
                  uint8_t* d_status, float* d_err, unsigned long long ref_key = 0);
// ref_key != 0: d_prev is the reference frame `ref_key` -- its pyramid and derivatives are built once and reused while the key stays
// orb_extract.hip
int stereo_match_dev(eorb_ctx* c, const eorb_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n, float mb, float mbf,
                     float* d_uright, float* d_depth, int32_t* d_sad, int32_t* d_nmatch);
int orb_extract_dev(eorb_ctx* c, const uint8_t* d_img, int img_stride, size_t img_slice_bytes, int B, int lap0, int lap1,
                    int want_desc, eorb_keypoint* d_kps, uint8_t* d_desc, uint8_t* d_oob, int32_t* d_n, int32_t* d_mono,
                    int32_t* d_flag_out = nullptr,       // d_flag_out: receives the overflow flag of this extraction (host entry point)
                    const float* d_level0_f32 = nullptr, const uint32_t* d_level0_mm = nullptr);
// d_level0_f32: the float event images (and their running extremes d_level0_mm) are still to be normalised: the first kernel does it while
// it builds level 0, and writes the u8 images to d_img
int orb_configure(eorb_ctx* c, const eorb_orb_params* p, int W, int H);
int orb_err_flag(eorb_ctx* c, int B, int* flag);
int orb_err_flag_to(eorb_ctx* c, int B, int32_t* d_dst);
int orb_pyramid_blur_dev(eorb_ctx* c, const uint8_t* d_img, int img_stride);
int orb_tracked_dev(eorb_ctx* c, eorb_keypoint* d_kps, int n, int mode, const uint8_t* d_ref, uint8_t* d_desc, uint8_t* d_oob);
int orb_debug_stage(eorb_ctx* c, const char* name, int slice, int level, void* out, size_t cap_bytes, int* dim0, int* dim1);
// calib.hip
int calib_points_dev(eorb_ctx* c, const CalibDev& P, const float* d_in, float* d_out, int n, int rec_floats);
int calib_frame_dev(eorb_ctx* c, const eorb_keypoint* d_kps, const int32_t* d_n, int cap, eorb_keypoint* d_un, float* d_bounds, int W, int H);
int calib_maps_dev(eorb_ctx* c, int LW, int LH, float* d_lut, float* d_mx, float* d_my);
// match.hip: match_args.h

}  // namespace eorb
