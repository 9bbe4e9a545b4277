/*
 * eorb_fe.h -- C ABI of the MI355X-native event-frame front end (libeorb_fe.so).
 *
 * Drop-in boundary for the hot path of m-dayani/EORB_SLAM: event->image accumulation, ORB
 * extraction and 256-bit Hamming matching.  The reference has no FFI for this path: it is reached
 * through three C++ seams, and every entry point below names the seam (file:line in the
 * reference repository) it replaces.  INTEGRATION.md shows the adapter a maintainer adds on the
 * reference side.  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   - every call returns 0 on success, <0 on error (EORB_E_*); never throws, never aborts.
 *   - an eorb_ctx owns device workspaces and runs on ONE HIP stream; it is single-threaded: one
 *     thread uses it at a time.  The reference also calls ev2im_gauss from 4 transient threads per
 *     motion-compensated image (src/Event/EvImBuilder.cpp:1165-1193): let those BORROW warm contexts
 *     from a pool instead of creating one per thread (eorb_host::ContextPool).
 *   - "host" entry points take host pointers, copy in/out and synchronise before returning.
 *   - "_dev" entry points take DEVICE pointers (HBM resident), enqueue on the ctx stream and do
 *     not synchronise: this is the throughput path (batches of slices).
 *   - results are bit-identical to the strict-IEEE CPU restatement of the reference (oracle/).
 */
#ifndef EORB_FE_H
#define EORB_FE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EORB_OK            0
#define EORB_E_EMPTY      -1   /* empty image: ORBextractor::operator() returns -1 (ORBextractor.cc:1096) */
#define EORB_E_CONFIG     -2   /* configuration the reference cannot run (division by zero) */
#define EORB_E_CAPACITY   -3   /* caller buffer / configured capacity too small */
#define EORB_E_ARG        -4   /* bad argument */
#define EORB_E_HIP        -5   /* HIP runtime error (see eorb_last_error) */
#define EORB_E_NOTCONF    -6   /* call needs a prior eorb_*_configure */

typedef struct eorb_ctx eorb_ctx;

/* include/Event/EventData.h:36-58 : struct EventData {double ts; float x; float y; bool p} (24 B) */
typedef struct {
    double  ts;
    float   x, y;
    uint8_t p;
    uint8_t pad_[7];
} eorb_event;

/* HBM-resident compact event record (16 B = the algorithmic bytes/event of SURVEY §8(d)):
 * x, y as the loader produced them; t = timestamp with the polarity packed in its sign bit
 * (t >= 0 always: sign bit SET means p == false). */
typedef struct {
    float  x, y;
    double t;
} eorb_event16;

/* one event as the sensor / dataset delivers it (src/Event/EventLoader.cpp:80-92 "ts x y p"): integer pixel, polarity,
 * timestamp.  16 B, the same HBM footprint as eorb_event16. */
typedef struct {
    uint16_t x, y;
    uint32_t p;         /* 0 = negative, otherwise positive */
    double   t;
} eorb_raw_event;

/* the same event as a 4-byte wire record for the event IMAGES (they never read the time stamp: ev2im / ev2im_gauss use x, y and the
 * polarity, src/Event/EventConversion.cc:173-269): x | p << 15 | y << 16, sensor sizes up to 32767 x 65535.  A quarter of the bytes
 * on the host -> HBM link (bench.py --stream). */
typedef uint32_t eorb_raw_event4;
/* the 2-byte wire record: the sensor pixel's linear index y * LW + x in the maps of eorb_set_undistort_maps (0xffff = no event); for
 * polarity-free images on sensors of at most 65 535 pixels, which read nothing else of an event */
typedef uint16_t eorb_raw_event2;

/* cv::KeyPoint (28 B): what ORBextractor::operator() fills (_keypoints) */
typedef struct {
    float   x, y;
    float   size;
    float   angle;
    float   response;
    int32_t octave;
    int32_t class_id;
} eorb_keypoint;

/* include/ORBextractor.h:33-47 : struct ORBxParams */
typedef struct {
    int   nfeatures;
    float scaleFactor;
    int   nlevels;
    int   iniThFAST;
    int   minThFAST;
    int   edgeTh;       /* Features.imMargin; <0 = adaptive rule of ORBextractor.cc:481-488 */
    int   imWidth;      /* used only by the adaptive rule */
} eorb_orb_params;

/* Frame image bounds + grid pitch: Frame::mnMinX.., mfGridElementWidthInv (Frame.cc:362-363, 855-866) */
typedef struct {
    float minX, minY, maxX, maxY;
    float invW, invH;
} eorb_grid_bounds;

/* ---- context --------------------------------------------------------------------------------- */
/* hip_stream: a hipStream_t to launch on (e.g. torch's current stream), or NULL for a private one */
int         eorb_create(int device, void* hip_stream, eorb_ctx** out);
void        eorb_destroy(eorb_ctx* ctx);
/* waits for the ctx stream; also reports (once, then clears) the sticky status of the asynchronous *_dev paths:
 * EORB_E_CAPACITY when a kernel of an earlier batched call overflowed an internal capacity (its keypoints are truncated).
 * The host-buffer entry points report the same condition from the call itself (eorb_orb_extract). */
int         eorb_sync(eorb_ctx* ctx);
/* test hooks, not part of the reference's interface: "octree_pool_shrink" (n > 0: shrink the octree node pool by n at the
 * next configure, to force the overflow path), "octree_force_global" (1: keep the whole octree working set in global memory), "orb_three_launches" (1: orientation, descriptors and output order as the three kernels of a call with a lapping area), "win_lds_entries" (window matchers: entries of a pair that the second phase stages in LDS; default: as many as fit), "win_list_cap" / "win_pool_cap" (window matchers:
 * candidate list capacity per query / pool per pair, to force the full-scan path), "gather_form" (event images with a Gaussian
 * stamp; the rules are csrc/ev_plan.h: 0 = choose the form by the call's shape; 1 = the list pipeline with its dense gather, float events
 * are not tabulated; 2 = the list pipeline with the wave per tile (float events: only those the bulk path tabulates, and their slot
 * lists still run when the batch is dense); 3 = no binning, every tile's wave reads all events of its slice (float or 16-byte sensor
 * records, at most 4 slices; float events the bulk path tabulates are not served this way); 4 = two-byte slot lists whatever the
 * batch's load (sensor records and tabulated float events; a count image, polarity, sigma > 4/3, a tile with more than 254 slots or
 * more than 2 048 slices run the list pipeline with its dense gather)), "dedupe_min_events" (float events:
 * number of events per call from which their distinct positions are tabulated, default 2^20), "kfdb_initial_slots" (KeyFrameDatabase:
 * the capacity in slots, and 64 pool words per slot, that the first eorb_kfdb_add allocates, to cross a pool growth with a handful of adds),
 * "kfdb_finish_lds_entries" (KeyFrameDatabase queries: scored keyframes up to which the last kernel sorts in LDS, 0 = as many as fit (4096),
 * to force its sort in global memory), "dirty_fill" (-1, the default: off; 0 .. 255: every device allocation of the context is filled with
 * that byte when it is made, the call arena is filled whole in front of every host-buffer call, and so are the pinned staging slot the
 * call's inputs are packed into and the pinned buffer its results land in -- what a call reads without having written it is then that
 * byte and not the zero of fresh memory or the previous call's values; tests/test_gpu_dirty.py).
 * These and every other switch are the rows of one table, csrc/eorb_options.h: eorb_create seeds a row from its environment variable,
 * if the table names one and it is set, else from the default; this call overwrites the context's value, whatever the row.  The slot
 * form's rows "slot_rank", "slot_hot_min", "slot_prerank", "slot_halves" (value < 0) and "slot_hot_waves" (value <= 0) take such a value
 * as "not set": the row goes back to what eorb_create gave it.  The other rows, settable per context by the same names:
 * "octree_list_algorithm" (1: the octree's list algorithm for every pass, from the next configure on).
 * "position_dict" (0: float events in bulk never freeze or use the position dictionary; drops the one the context holds).
 * "slot_hot_cap" (slot form: lists per length bucket of the register-row kernel, to force its overflow branch).
 * "scatter" (EORB_SCATTER; 1: the list pipeline's first scatter form only).
 * "gather_threads" (EORB_GATHER_THREADS; the generic gather's workgroup, 192 .. 1024 in steps of 64, else the build's).
 * "gather_nc" (EORB_GATHER_NC; 2 / 4 tile columns per value wave of the raw gather, else by the launch's size).
 * "slot_chunk" (EORB_SLOT_CHUNK; slot form: 256 / 1024 / 2048 / 4096 events per binning chunk, else by the slices' length).
 * "slot_waves" (EORB_SLOT_WAVES; slot form: 1 .. 16 wavefronts of the gather's workgroup).
 * "slot_rounds" (EORB_SLOT_ROUNDS; slot form: rounds of spare gather tasks, default 4).
 * "slot_rank" (EORB_SLOT_RANK; 0: the ballot scatter although the device check passed).
 * "slot_hot_min" (EORB_SLOT_HOT_MIN; list length from which the register-row kernel takes a list, 0: that kernel off).
 * "slot_hot_waves" (EORB_SLOT_HOT_WAVES; wavefronts of the register-row kernel, default 8 per compute unit).
 * "slot_prerank" (EORB_SLOT_PRERANK; 0: the count pass keeps no ranks, the rank scatter makes its own).
 * "slot_halves" (EORB_SLOT_HALVES; 0: a batch runs as one part, 1: as two halves, whatever its shape).
 * "win_cand_waves" / "win_qpb" (EORB_WIN_CAND_WAVES / EORB_WIN_QPB; window matchers: wavefronts / queries of a phase-1 workgroup).
 * "upload_kernel_max" / "download_kernel_max" (EORB_UPLOAD_KERNEL_MAX / EORB_DOWNLOAD_KERNEL_MAX; host-buffer calls: bytes up to which a
 * kernel, not the copy engine, moves a call's inputs / results; default 2^20).
 * "sync_spin" (EORB_SYNC_SPIN; 1: host-buffer calls poll for their results instead of blocking).
 * "slice_zero_copy" / "image_zero_copy" (EORB_SLICE_ZERO_COPY / EORB_IMAGE_ZERO_COPY; 0: a live slice's events / a call's one image are
 * uploaded, not read in place from pinned host memory).
 * "contest_direct_max" (EORB_CONTEST_DIRECT_MAX; eorb_ev_mc_contest: events up to which one launch makes every image; default 49152).
 * "octree_budget_kb" / "octree_direct" / "octree_dynamic" (EORB_OCT_BUDGET_KB / EORB_OCT_DIRECT / EORB_OCT_DYNAMIC; the octree kernel's
 * LDS budget, its direct passes and its dynamic placement, from the next configure on).
 * "orb_describe" (EORB_ORB_DESCRIBE; 0: orientation, descriptors and output order never as one launch).
 * Returns EORB_E_ARG for an unknown name. */
int         eorb_debug_option(eorb_ctx* ctx, const char* name, int value);
/* test hook: the value the context runs with for a row of that table; EORB_E_ARG for an unknown name */
int         eorb_debug_option_get(eorb_ctx* ctx, const char* name, long long* value);
/* test hook: counters a test can read to see which path served its calls.  "slot_calls": accumulation calls that took the slot
 * lists (gather_form 0 on dense batches, or 4); "slot_flags": sticky device flags of that path (0 = fine; synchronises); "slot_hot_items": lists the last such call handed to
 * the register-row kernel (synchronises); "slot_rank_ok": 1 when the scatter takes its ranks from LDS atomics; "kfdb_slot_cap" /
 * "kfdb_word_cap": slots / words the KeyFrameDatabase pools hold room for; "accum_route": what served the context's last accumulation
 * call (0: none yet) = form (1 binning-free, 2 slot lists, 3 list pipeline) | position set << 2 (0 none: float events as they are,
 * 1 the undistortion maps, 2 the call's own tabulated positions, 3 the position dictionary) | 16 if the pipeline's sparse gather ran
 * | 32 if short records (eorb_raw_event4 / eorb_raw_event2) were widened first; "slot_scatter_form" (1 rank or pre-ranked scatter, 0 ballot),
 * "slot_chunk" (events per binning chunk) and "slot_binning" of the last call that took the slot lists (-1: none yet) = count pass (0 global
 * counters, 1 tile ranges in LDS, 2 the same with the position dictionary's lookup) | record the scatter reads << 2 (0 the events as they
 * are, 1 2-byte sensor indices, 2 8-byte ranked records) | scatter << 4 (0 ballot, 1 rank, 2 pre-ranked); "win_total_nonzero": pairs of the
 * window matchers whose entry counter is not back at zero after the last call (0 = fine; synchronises).
 * The host-buffer calls' arena, cumulative over the context's life (a test reads them before and after a call): "arena_calls" (arenas laid
 * out), "arena_bytes" (their sizes), "arena_in_bytes" (their uploaded prefixes), "arena_downloads", "arena_download_bytes" and
 * "arena_download_first" (the sum of the downloads' first arena offsets); tests/test_gpu_arena_layout.py.
 * Returns the value, or -1 for an unknown name. */
long long   eorb_debug_counter(eorb_ctx* ctx, const char* name);
/* test hook, not part of the reference's interface: the intermediate images of the extractor, for stage-by-stage comparison with
 * the CPU oracle.  Waits for the ctx stream, then copies what the LAST extraction of the context left in its workspaces:
 *   "pyr"   the bordered buffer of pyramid level `level`, bh rows of bw bytes (bw = w + 2 * edge).  The kernels write the WHOLE
 *           bordered buffer (level 0 and every resized level, BORDER_REFLECT_101 included), so all of it is comparable;
 *   "blur"  the blurred level the descriptors read, h rows of w bytes; EORB_E_ARG when that call computed no descriptors;
 *   "cand"  the level's FAST candidates after the per-cell iniThFAST / minThFAST rule, i.e. the octree's input: dim0 records of
 *           three floats (x, y, response), x and y relative to the level's minimum border like the reference's vToDistributeKeys,
 *           in no particular order; EORB_E_ARG after eorb_orb_tracked_descriptors / _assign_level_by_best_desc (pyramid only).
 * slice: the frame of a batched call (eorb_fe_run_batch_*), the image of eorb_frame_stereo (0 left, 1 right); 0 otherwise.
 * dim0 / dim1 (may be NULL) receive rows / columns ("cand": records / 3).  out == NULL: only the dimensions are returned.
 * Unknown name, level or slice out of range, cap_bytes too small: EORB_E_ARG; no extraction since the last eorb_orb_configure:
 * EORB_E_NOTCONF.  The hook launches nothing and allocates nothing on the device, and the extractor keeps no buffer for it. */
int         eorb_debug_stage(eorb_ctx* ctx, const char* name, int slice, int level, void* out, size_t cap_bytes, int* dim0, int* dim1);
const char* eorb_last_error(eorb_ctx* ctx);
const char* eorb_version(void);
/* per-kernel HIP-event timing on the ctx stream (off by default; used by bench.py) */
int         eorb_prof_enable(eorb_ctx* ctx, int on);
int         eorb_prof_reset(eorb_ctx* ctx);
/* names: comma-separated scope names to time, NULL or "" = all (two event records per scope and call are a visible share of a
 * short step: bench.py times only the accumulation scopes inside its timed steps) */
int         eorb_prof_only(eorb_ctx* ctx, const char* names);
int         eorb_prof_count(eorb_ctx* ctx);
int         eorb_prof_get(eorb_ctx* ctx, int i, const char** name, double* total_ms, int64_t* launches);

/* ---- event accumulation (host buffers) -------------------------------------------------------- */
/* replaces EvImConverter::ev2im, src/Event/EventConversion.cc:173-212 (include/Event/EventConversion.h:52).
 * out_f32 (W*H, optional) = accumulated CV_32FC1 image; out_u8 (W*H, optional) = normalised image;
 * *is_u8 = 1 when the reference would return CV_8UC1 (normalized && max > min). minmax optional [2]. */
int eorb_ev2im(eorb_ctx* ctx, const eorb_event* ev, size_t n, int W, int H, int pol, int normalized,
               float* out_f32, uint8_t* out_u8, float* minmax, int* is_u8);

/* replaces EvImConverter::ev2im_gauss, src/Event/EventConversion.cc:215-269
 * (include/Event/EventConversion.h:54-56; callers EvImBuilder.cpp:1345,1070) */
int eorb_ev2im_gauss(eorb_ctx* ctx, const eorb_event* ev, size_t n, int W, int H, float sigma, int pol,
                     int normalized, float* out_f32, uint8_t* out_u8, float* minmax);

/* ---- raw sensor events through the undistortion maps ------------------------------
 * mapX / mapY = MyCalibrator::mUndistMapX / mUndistMapY (Utils/MyCalibrator.cpp:60-101, LH x LW floats each, built by the
 * caller with cv::undistortPoints as the reference does, or on the device by eorb_generate_undistort_maps below).  checkInImage = the flag the loader passes to
 * getEventChunkRectified (EventLoader.cpp:264-305): events whose undistorted point fails MyCalibrator::isInImage(x, y)
 * for the accumulation image (:31-34) are dropped. */
int eorb_set_undistort_maps(eorb_ctx* ctx, const float* mapX, const float* mapY, int LW, int LH, int checkInImage);

/* replaces the rectification loop of EventDataStore::getEventChunkRectified (src/Event/EventLoader.cpp:264-305) after
 * parsing: out[k] = {raw.t / tsFactor, mapX[y][x], mapY[y][x], p} (MyCalibrator::undistPointMaps :164-180) for the events
 * kept by checkInImage against a W x H image, in order.  out has room for n events; *n_out = number kept. */
int eorb_undistort_events(eorb_ctx* ctx, const eorb_raw_event* raw, size_t n, int W, int H, double tsFactor,
                          eorb_event* out, size_t* n_out);

/* replaces the text half of the loader: getline + EventDataStore::parseLine ("stream >> ts >> x >> y >> p",
 * src/Event/EventLoader.cpp:80-92) + BaseLoader::isComment (Utils/DataStore.cpp:111-114) over a whole buffer of the dataset's
 * events.txt.  The accepted grammar (the kernel, the oracle and tests/loader_model.py follow this text):
 *   lines     a line ends at '\n', or at the last byte of a buffer that does not end in '\n'; one trailing '\r' is dropped.  There is
 *             no limit on a line's length.
 *   skipped   a line that, after its leading blanks (' ' and '\t'), is empty or starts with '#', whatever bytes follow.
 *   tokens    a number token is \d+\.?\d* or \.\d+ : no sign, no exponent, no other byte.  Tokens are taken greedily; blanks and tabs
 *             between them are optional separators, as "stream >> ts >> x >> y >> p" reads them: `1.0.0 3 1` is (1.0, 0, 3, 1).  An
 *             event line holds exactly four tokens, and only blanks may follow the fourth.
 *   digits    a token of more than 19 significant digits is outside the grammar; significant digits count from the first non-zero
 *             digit on, zeros of the fraction included (`1.0000000000000000000` has 20).  This holds for all four tokens.
 *   ts        mantissa (the digits read as one integer) below 2^53 and at most 22 fraction digits: the value is the double nearest
 *             to mantissa / 10^frac (one IEEE division of two exact doubles gives it, and so does a correct strtod).
 *   x, y      every fraction digit is 0 and the value lies in 0..65535 (the reference truncates them, MyCalibrator.cpp:172-173).
 *   p         no point, value 0 or 1 (`01` is 1; `1.` and `0.` are malformed).
 * Any other line is malformed: EORB_E_ARG with *bad_line = the smallest 0-based index of a malformed line, comment and blank lines
 * counted (the caller falls back to its own parser for that file); *n_out = 0 and out is not written.  This takes precedence over
 * EORB_E_CAPACITY, which is returned when the text holds more than cap events (*n_out = 0, out not written, *bad_line = -1).
 * out has room for cap events; bad_line may be NULL. */
int eorb_parse_events_text(eorb_ctx* ctx, const char* text, size_t nbytes, eorb_raw_event* out, size_t cap, size_t* n_out,
                           int64_t* bad_line);

/* = eorb_undistort_events followed by eorb_ev2im_gauss / eorb_ev2im on the kept events, fused: the stamp of a sensor
 * pixel depends only on its map entry, so the (2h+1)^2 values per pixel are tabulated once per (maps, sigma) and the
 * accumulation kernel only orders and adds them.  Bit-identical to the two-step path. */
int eorb_ev2im_gauss_raw(eorb_ctx* ctx, const eorb_raw_event* raw, size_t n, int W, int H, float sigma, int pol,
                         int normalized, float* out_f32, uint8_t* out_u8, float* minmax);
int eorb_ev2im_raw(eorb_ctx* ctx, const eorb_raw_event* raw, size_t n, int W, int H, int pol, int normalized,
                   float* out_f32, uint8_t* out_u8, float* minmax, int* is_u8);

/* ---- motion-compensated accumulation (host buffers) ------------------------------------------------ */
typedef struct { float fx, fy, cx, cy; } eorb_pinhole;     /* Pinhole::mvParameters (CameraModels/Pinhole.cpp:30-62) */

/* replaces EvImConverter::ev2mci_gg_f(evs, pCamera, Tcw, medDepth, W, H, sigma, pol, normalized)
 * (src/Event/EventConversion.cc:280-360) and the depth-map overload (:451-531, pass depth_per_event[n] =
 * depthMapObj.getDepthLinInterp(ex, ey)).  angle / axis = Eigen::AngleAxisd(R of Tcw), t = translation of Tcw (the
 * adapter computes them once per call with Eigen, as the reference does at :297-301).  n == 0 -> zero image. */
int eorb_ev2mci_se3(eorb_ctx* ctx, const eorb_event* ev, size_t n, const eorb_pinhole* cam, double angle,
                    const double axis[3], const double t[3], float medDepth, const float* depth_per_event,
                    int W, int H, float sigma, int pol, int normalized, float* out_f32, uint8_t* out_u8, float* minmax);
/* replaces the SE2 overload (params2D = {omega, vx, vy[, scale]}), src/Event/EventConversion.cc:363-448 */
int eorb_ev2mci_se2(eorb_ctx* ctx, const eorb_event* ev, size_t n, const eorb_pinhole* cam, const float* params2D, int nparams,
                    int W, int H, float sigma, int pol, int normalized, float* out_f32, uint8_t* out_u8, float* minmax);
/* GeometricCamera of the motion-compensated images: model 0 = Pinhole (fx, fy, cx, cy), 1 = KannalaBrandt8 (+ k[0..3] =
 * mvParameters[4..7], precision = KB8_DEF_PRECISION 1e-6: include/CameraModels/KannalaBrandt8.h:36; the MVSEC configuration,
 * Examples/Event/EvMVSEC_ETHZ.yaml:54-67).  unproject / project follow src/CameraModels/KannalaBrandt8.cpp:87-190. */
typedef struct { int model; float fx, fy, cx, cy; float k[4]; float precision; } eorb_camera;
int eorb_ev2mci_se3_cam(eorb_ctx* ctx, const eorb_event* ev, size_t n, const eorb_camera* cam, double angle,
                        const double axis[3], const double t[3], float medDepth, const float* depth_per_event,
                        int W, int H, float sigma, int pol, int normalized, float* out_f32, uint8_t* out_u8, float* minmax);
int eorb_ev2mci_se2_cam(eorb_ctx* ctx, const eorb_event* ev, size_t n, const eorb_camera* cam, const float* params2D, int nparams,
                        int W, int H, float sigma, int pol, int normalized, float* out_f32, uint8_t* out_u8, float* minmax);
/* replaces EvImConverter::measureImageFocus (src/Event/EventConversion.cc:74-111) */
int eorb_measure_image_focus(eorb_ctx* ctx, const float* img, int W, int H, float* focus);
/* n images of W x H back to back in one call (the motion-compensation contest scores its reconstructions together,
 * src/Event/EvImBuilder.cpp:1165-1203): focus[n] */
int eorb_measure_image_focus_n(eorb_ctx* ctx, const float* imgs, int n, int W, int H, float* focus);
/* replaces cv::normalize(img, img, 255, 0, NORM_MINMAX, CV_8UC1) at src/Event/EvImBuilder.cpp:976,1055,1076,1140 */
int eorb_normalize_minmax_u8(eorb_ctx* ctx, const float* img, int W, int H, uint8_t* out);

/* ---- camera calibration: undistorted points, keypoints and the calibrator's maps ------------------------------------------
 * MyCalibrator (src/Utils/MyCalibrator.cpp) keeps K, the distortion coefficients, R and P (:11-29) and sends every point through
 * cv::undistortPoints (Pinhole) or cv::fisheye::undistortPoints (KannalaBrandt8) of OpenCV 3.4.1; both are restated in double, in
 * the operation order of their scalar paths.  The calibration is per-context state like the maps and the
 * vocabulary.  R: 3 x 3 row-major; P: 3 rows of p_cols floats, of which the left 3 x 3 block is used. */
typedef struct eorb_calib {
    int   model;        /* 0 = pinhole (cv::undistortPoints), 1 = fisheye (cv::fisheye::undistortPoints) */
    float K[9];         /* CV_32F 3x3 as the reference holds it (mK) */
    float dist[8];      /* pinhole: k1 k2 p1 p2 [k3 [k4 k5 k6]]; fisheye: k1..k4 */
    int   n_dist;       /* pinhole 4, 5 or 8; fisheye 4; anything else EORB_E_ARG */
    float R[9];  int has_R;     /* 0 = cv::Mat(): identity */
    float P[12]; int p_cols;    /* 0 = cv::Mat() (normalised coordinates out), 3 or 4 (left 3x3 block used) */
} eorb_calib;

/* replaces MyCalibrator::MyCalibrator's members (:11-17): copied into the context; bad model / n_dist / has_R / p_cols: EORB_E_ARG */
int eorb_set_calibration(eorb_ctx* ctx, const eorb_calib* calib);

/* replaces MyCalibrator::undistKeyPointsPinhole / undistKeyPointsFishEye (src/Utils/MyCalibrator.cpp:198-283; callers Frame.cc:246-252,
 * :339-340, :1186-1192, MixedFrame.cpp:133,138, EventFrame.cpp:435-446): out[i] = in[i] with pt undistorted, every other field
 * copied.  n == 0: EORB_OK, nothing written (:202-205).  When MyCalibrator::isDistorted fails (:46-50: fabs(dist[0]) > 1e-9 in
 * double) out is a copy of in, whatever the other coefficients are (:206-210).  No calibration: EORB_E_NOTCONF. */
int eorb_undistort_keypoints(eorb_ctx* ctx, const eorb_keypoint* in, int n, eorb_keypoint* out);

/* replaces MyCalibrator::undistPointPinhole / undistPointFishEye (:119-156) over n points (x, y) -> xy_out (n x 2); same gate */
int eorb_undistort_points(eorb_ctx* ctx, const float* xy, int n, float* xy_out);

/* replaces MyCalibrator::generateUndistMapsPinhole / FishEye (:64-102): map[y][x] = undistPoint((float)x, (float)y) for every
 * sensor pixel, written on the device into the context's maps, which are then installed exactly as eorb_set_undistort_maps
 * installs uploaded ones (checkInImage as there): afterwards every raw-event entry point behaves as if the caller had uploaded
 * them.  mapX / mapY (LH x LW floats each, optional): the maps downloaded.  Gate closed: the identity maps (float)x, (float)y. */
int eorb_generate_undistort_maps(eorb_ctx* ctx, int LW, int LH, int checkInImage, float* mapX, float* mapY);

/* replaces the hot path of the monocular Frame constructor (src/Frame.cc:229-266): ExtractORB (:240), undistKeyPoints on the
 * keypoints while they are still on the device (:246-252) and Frame::ComputeImageBounds (:840-867).  kps / desc / oob / n_out /
 * mono_index exactly as eorb_orb_extract; kps_un[cap] = eorb_undistort_keypoints of kps; bounds = mnMinX, mnMaxX, mnMinY, mnMaxY.
 * ComputeImageBounds has its own gate, dist[0] != 0.0 (:842), and always calls cv::undistortPoints(corners, K, dist, cv::Mat(), K)
 * (:851): the pinhole arithmetic on all n_dist coefficients with R = identity and P = K, whatever model, R and P the calibration
 * holds; gate closed: 0, W, 0, H.  One upload, one wait, one download. */
int eorb_frame_mono(eorb_ctx* ctx, const uint8_t* img, int W, int H, int stride, int lap0, int lap1, int want_desc,
                    eorb_keypoint* kps, eorb_keypoint* kps_un, uint8_t* desc, uint8_t* oob, int cap,
                    int* n_out, int* mono_index, float bounds[4]);

/* ---- ORB extractor (host buffers) --------------------------------------------------------------- */
/* replaces ORBextractor::ORBextractor, src/ORBextractor.cc:420-489: scale tables, per-level quotas,
 * edge threshold (per context, not a process global: SURVEY App.B H3) for images of W x H */
int eorb_orb_configure(eorb_ctx* ctx, const eorb_orb_params* p, int W, int H);
int eorb_orb_max_keypoints(eorb_ctx* ctx);               /* output capacity needed */
int eorb_orb_get_tables(eorb_ctx* ctx, float* scale_factors, float* inv_scale_factors,
                        int* features_per_level, int* edge_threshold);   /* getters hdr:83-107 */

/* replaces ORBextractor::operator() with descriptors (src/ORBextractor.cc:1092-1176) and the
 * detect-only overload (:1178-1238); include/ORBextractor.h:75-81.  lap0/lap1 = vLappingArea.
 * kps[cap], desc[cap*32] (may be NULL when !want_desc), oob[cap] optional (1 = some rBRIEF tap of
 * that keypoint left the blurred level buffer: the reference reads out of bounds there, H4).
 * *mono_index = the reference's return value. */
int eorb_orb_extract(eorb_ctx* ctx, const uint8_t* img, int W, int H, int stride, int lap0, int lap1,
                     int want_desc, eorb_keypoint* kps, uint8_t* desc, uint8_t* oob, int cap,
                     int* n_out, int* mono_index);

/* replaces ORBextractor::ComputeTrackedKPtsDesc (src/ORBextractor.cc:1316-1363; callers EvAsynchTrackerU.cpp:794,812):
 * descriptor of every tracked keypoint at the pyramid level of its octave (pt * mvInvScaleFactor[octave], kp.angle).
 * desc: n x 32; rows whose octave is outside [0, nlevels) are zero (uninitialised in the reference). oob optional. */
int eorb_orb_tracked_descriptors(eorb_ctx* ctx, const uint8_t* img, int W, int H, int stride,
                                 const eorb_keypoint* kps, int n, uint8_t* desc, uint8_t* oob);

/* replaces ORBextractor::AssignKPtLevelByBestDesc (src/ORBextractor.cc:1267-1314; caller EvSynchTracker.cpp:790):
 * kps[i].octave <- the level whose descriptor at pt * invScale[level] is closest (Hamming) to ref_desc row i. */
int eorb_orb_assign_level_by_best_desc(eorb_ctx* ctx, const uint8_t* img, int W, int H, int stride,
                                       const uint8_t* ref_desc, eorb_keypoint* kps, int n);

/* ---- matchers (host buffers) ------------------------------------------------------------------------ */
/* replaces ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:714-831) and
 * MixedMatcher::SearchForInitialization (src/MixedMatcher.cpp:20-145; is_orb* = isORBDescValid gate,
 * NULL = all ORB).  kps*: undistorted keypoints; desc*: n x stride bytes, first 32 compared
 * (ORBmatcher.cc:2360-2378).  prev_matched: n1 (x,y) in/out; matches12: n1 out. */
int eorb_search_for_initialization(eorb_ctx* ctx,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, int stride1, const uint8_t* is_orb1,
        const eorb_keypoint* kps2, int n2, const uint8_t* desc2, int stride2, const uint8_t* is_orb2,
        const eorb_grid_bounds* gb, float* prev_matched, int32_t* matches12,
        int windowSize, float nnratio, int checkOri, int* nmatches);

/* replaces the mono branch of ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)
 * (src/ORBmatcher.cc:1969-2187; MixedMatcher.cpp:693-).  The projection is the caller's, on the host or with
 * eorb_project_last_frame; eorb_search_by_projection_last_pose does both in one call:
 * valid/uv per last-frame keypoint, mp_desc (n_last x 32), mp_obs; cur_mp in/out
 * (-1 none, k>=0 last-frame point k, -2 foreign observed, -3 foreign unobserved).
 * mode 0: levels [o-1,o+1]; 1 forward (>= o); 2 backward ([0,o]). */
int eorb_search_by_projection_last(eorb_ctx* ctx,
        const eorb_keypoint* cur_kps, int n_cur, const uint8_t* cur_desc, int cur_stride, const uint8_t* cur_is_orb,
        const eorb_keypoint* last_kps, int n_last, const uint8_t* last_is_orb,
        const uint8_t* valid, const float* uv, const uint8_t* mp_desc, const uint8_t* mp_obs,
        const float* level_scale /* n_last: getORBScaleFactor(octave) or the AKAZE factor */,
        const eorb_grid_bounds* gb, int32_t* cur_mp, float th, int mode, int checkOri, int* nmatches);

/* replaces ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist)
 * (src/ORBmatcher.cc:2189-2312; MixedMatcher.cpp:928-1063; relocalisation, f3).  One query per pKF feature i:
 * valid[i] = map point present, !isBad(), not in sAlreadyFound, projection inside the image and distance gates passed
 * (:2207-2234, by the caller: eorb_project_keyframe_points, or eorb_search_by_projection_kf_pose for both steps); uv, pred_level = PredictScale, level_scale = getORBScaleFactor / getAKAZEScaleFactor of that level,
 * mp_desc = pMP->GetDescriptor().  cur_mp in/out: -1 free, anything else occupied; a match writes i (the pKF feature index). */
int eorb_search_by_projection_kf(eorb_ctx* ctx,
        const eorb_keypoint* cur_kps, int n_cur, const uint8_t* cur_desc, int cur_stride, const uint8_t* cur_is_orb,
        const eorb_keypoint* kf_kps, int n_kf, const uint8_t* kf_is_orb,
        const uint8_t* valid, const float* uv, const int32_t* pred_level, const float* level_scale, const uint8_t* mp_desc,
        const eorb_grid_bounds* gb, int32_t* cur_mp, float th, int ORBdist, int checkOri, int* nmatches);

/* replaces the mono branch of ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)
 * (src/ORBmatcher.cc:44-219; MixedMatcher.cpp:500-691). */
int eorb_search_by_projection_map(eorb_ctx* ctx,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const uint8_t* is_orb,
        int M, const uint8_t* in_view, const float* proj_xy, const int32_t* level, const float* view_cos,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const uint8_t* mp_is_orb, const float* level_scale,
        const eorb_grid_bounds* gb, int32_t* frame_mp, float th, float nnratio, int* nmatches);

/* The rectified-stereo / RGB-D gate of the two matchers above -- "if(F.mvuRight[idx]>0) { er = fabs(projXR - F.mvuRight[idx]);
 * if(er > radius) continue; }" (src/ORBmatcher.cc:96-104 with pMP->mTrackProjXR and r * getORBScaleFactor(level); :2056-2062 with
 * ur = uv.x - mbf * invzc and th * getORBScaleFactor(octave)): uright = mvuRight of the searched frame's keypoints (n floats, <= 0: no
 * right match), proj_xr / proj_ur = the right coordinate of every query, computed by the caller with the projection.  Everything else
 * as the mono entry points (whose configurations pass no mvuRight: Frame::numKPtsLeft() != -1 or all mvuRight = -1). */
int eorb_search_by_projection_map_stereo(eorb_ctx* ctx,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const uint8_t* is_orb,
        int M, const uint8_t* in_view, const float* proj_xy, const int32_t* level, const float* view_cos,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const uint8_t* mp_is_orb, const float* level_scale,
        const eorb_grid_bounds* gb, int32_t* frame_mp, float th, float nnratio, const float* uright, const float* proj_xr, int* nmatches);
int eorb_search_by_projection_last_stereo(eorb_ctx* ctx,
        const eorb_keypoint* cur_kps, int n_cur, const uint8_t* cur_desc, int cur_stride, const uint8_t* cur_is_orb,
        const eorb_keypoint* last_kps, int n_last, const uint8_t* last_is_orb,
        const uint8_t* valid, const float* uv, const uint8_t* mp_desc, const uint8_t* mp_obs,
        const float* level_scale, const eorb_grid_bounds* gb, int32_t* cur_mp, float th, int mode, int checkOri,
        const float* cur_uright, const float* proj_ur, int* nmatches);

/* replaces the stereo constructor's hot path, Frame::Frame(imLeft, imRight, ...) (src/Frame.cc:97-152): ExtractORB on both images
 * (:122-125, two extractors of equal parameters, vLappingArea {0, 0}) and Frame::ComputeStereoMatches (:869-1048: row-band candidates,
 * best descriptor distance below (TH_HIGH + TH_LOW) / 2, 11 x 11 L1 correlation over the shifts -5..5 on the keypoint's level image,
 * parabola, median cut).  mb = baseline in metres (mbf / fx), mbf = baseline x fx.  Out: the keypoints and descriptors of both images
 * (mvKeys / mvKeysRight order), uRight / depth [nL] = mvuRight / mvDepth (-1: none), nmatches = correlated matches before the median
 * cut.  One upload, one wait, one download.  The rectified images are what the caller passes (the reference assumes undistorted
 * images here, :136-141). */
int eorb_frame_stereo(eorb_ctx* ctx, const uint8_t* imLeft, const uint8_t* imRight, int W, int H, int stride, float mb, float mbf,
                      eorb_keypoint* kpsL, uint8_t* descL, int* nL, eorb_keypoint* kpsR, uint8_t* descR, int* nR, int cap,
                      float* uRight, float* depth, int* nmatches);

/* ---- two-camera (fisheye stereo) frames ------------------------------------------------------------------------------------
 * Frame::Frame(imLeft, imRight, ..., pCamera, pCamera2, Tlr) (src/Frame.cc:1101-1208; built by Tracking.cc:245-256 for STEREO /
 * IMU_STEREO with a second camera, KannalaBrandt8) and the numKPtsLeft() != -1 branches of the tracking matchers.  Such a frame holds
 * nL left keypoints followed by nR right ones (mvKeys, then mvKeysRight), descriptors concatenated the same way (cv::vconcat :1176),
 * map-point slots frame_mp[nL + nR].  Both grids use the caller's eorb_grid_bounds (ComputeImageBounds(imLeft), :1145-1148): the
 * left grid holds the mvKeys positions (distorted: getDistKPtMono :758-760), the right grid the mvKeysRight positions.  Projection,
 * isInFrustum, isBad, far-point and outlier gates are the caller's, as for the mono entry points; eorb_project_frustum with
 * two views, eorb_project_last_frame with Trl and eorb_search_local_points_fisheye move the projection to the device.
 * Right grid level gate: GetFeaturesInArea(..., bRight = true) tests getKPtLevelMono(j) = mvKeysUn[j].octave (:763, :1417-1420),
 * i.e. the octave of LEFT keypoint j, for right keypoint j; for j >= nL the reference reads past mvKeysUn (nL entries, :1191) and
 * this library uses the right keypoint's own octave (upstream ORB-SLAM3's reading).  The query octave getKPtLevelMono(i) of a
 * last-frame point i >= nL_last follows the same rule: the caller passes the last frame's keypoints in index order.
 * Limits: nL + nR <= 8192 keypoints per searched frame (octaves 0..127), fewer than 2^24 queries; EORB_E_CAPACITY beyond. */

/* replaces the hot path of the fisheye constructor (src/Frame.cc:1101-1208) and ComputeStereoFishEyeMatches (:1210-1250) up to
 * the triangulation: ExtractORB on both images with each camera's lapping area (mvLappingArea of mpCamera: lapL0/lapL1, of mpCamera2:
 * lapR0/lapR1, :1124-1129), then knnMatch(k = 2) of the left lapping descriptors (rows monoLeft..) against the right ones (rows
 * monoRight..) (:1228, the tie rule of eorb_hamming_bf_knn2) and Lowe's test "size() >= 2 && d0 < d1 * 0.7" (:1233, in double).
 * Out: keypoints / descriptors / monoIndex of both images; per left keypoint right_idx[nL] = the candidate right keypoint index
 * (trainIdx + monoRight) or -1, dist2[2 * nL] = the two knn distances (-1: none, or outside the lapping area); *ncand = candidates.
 * KannalaBrandt8::TriangulateMatches (an SVD per candidate) stays on the host: it turns the candidates into mvLeftToRightMatch,
 * mvRightToLeftMatch and mvDepth.  One upload, one wait, one download. */
int eorb_frame_fisheye(eorb_ctx* ctx, const uint8_t* imLeft, const uint8_t* imRight, int W, int H, int stride,
                       int lapL0, int lapL1, int lapR0, int lapR1,
                       eorb_keypoint* kpsL, uint8_t* descL, int* nL, int* monoLeft,
                       eorb_keypoint* kpsR, uint8_t* descR, int* nR, int* monoRight, int cap,
                       int32_t* right_idx, int32_t* dist2, int* ncand);

/* replaces the two-camera path of ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:44-219).
 * Per map point, left (mbTrackInView, mTrackProjX/Y, mnTrackScaleLevel, mTrackViewCos, getORBScaleFactor(level)) and right
 * (mbTrackInViewR, mTrackProjXR/YR, mnTrackScaleLevelR (-1: skip), mTrackViewCosR, its scale factor); l2r[nL] / r2l[nR] =
 * mvLeftToRightMatch / mvRightToLeftMatch.  frame_mp[nL + nR] in/out as in eorb_search_by_projection_map.  Reproduced: a left
 * ratio rejection skips the right block (the `continue` at :130); the right radius ignores th (:152); a left match also writes
 * slot nL + l2r[best] (:136-137) and a right match slot r2l[best] (:204-205), each counted; no mvuRight gate (:95). */
int eorb_search_by_projection_map_fisheye(eorb_ctx* ctx,
        const eorb_keypoint* kps, int nL, int nR, const uint8_t* desc, int stride, const int32_t* l2r, const int32_t* r2l,
        int M, const uint8_t* in_view, const float* proj_xy, const int32_t* level, const float* view_cos, const float* level_scale,
        const uint8_t* in_view_r, const float* proj_xy_r, const int32_t* level_r, const float* view_cos_r, const float* level_scale_r,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const eorb_grid_bounds* gb, int32_t* frame_mp, float th, float nnratio,
        int* nmatches);

/* replaces the two-camera path of ORBmatcher::SearchByProjection(CurF, LastF, th, bMono) (src/ORBmatcher.cc:1969-2187).  Queries:
 * all n_last = nL_last + nR_last points of the last frame; valid / uv = the left projection (invzc, bounds and outlier folded
 * into valid), uv_r = mpCamera->project(mTrl * x3Dc) (no bounds check in the reference), last_kps = the query keypoints in index
 * order (octave, angle), level_scale = getORBScaleFactor(octave), mp_desc / mp_obs per query.  cur_mp[nL + nR] in/out and mode as
 * in eorb_search_by_projection_last; a right match writes nL + j.  Reproduced: the right search runs only when the left window was
 * not empty (:2033), whatever the left search found; one rotation histogram holds both cameras' matches (:2155, :2167-2184). */
int eorb_search_by_projection_last_fisheye(eorb_ctx* ctx,
        const eorb_keypoint* cur_kps, int nL, int nR, const uint8_t* cur_desc, int cur_stride,
        const eorb_keypoint* last_kps, int n_last, const uint8_t* valid, const float* uv, const float* uv_r,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const float* level_scale, const eorb_grid_bounds* gb,
        int32_t* cur_mp, float th, int mode, int checkOri, int* nmatches);

/* replaces the two-camera path of ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:276-478):
 * inputs as eorb_search_by_bow, frame features = nL left then the right ones (n_f in all).  Two best / second-best pairs, over
 * frame indices below nL and over the rest (:357-377); the right best is taken only inside "if(bestDist1 <= TH_LOW)" (:410) and
 * its ratio test always passes ("|| true", :412).  kf_kps in the KeyFrame's index order (its right keypoints after its left ones).
 * The KeyFrame goes through the set form's path as a set of one (eorb_kf_set below): its checks and limits apply, as at eorb_search_by_bow. */
int eorb_search_by_bow_fisheye(eorb_ctx* ctx,
        const eorb_keypoint* kf_kps, int n_kf, const uint8_t* kf_desc, const uint8_t* kf_has_mp,
        const uint32_t* kf_nodes, const int32_t* kf_node_off, const int32_t* kf_idx, int kf_nn,
        const eorb_keypoint* f_kps, int n_f, int nL, const uint8_t* f_desc,
        const uint32_t* f_nodes, const int32_t* f_node_off, const int32_t* f_idx, int f_nn,
        int32_t* match_f, float nnratio, int checkOri, int* nmatches);

/* ---- map points projected on the device -----------------------------------------------------------------------------------
 * Frame::isInFrustum (src/Frame.cc:548-637, isInFrustumChecks :1252-1325), MapPoint::PredictScale (src/MapPoint.cc:570-593) and the
 * projection loops of the tracking matchers (src/ORBmatcher.cc:1999-2022, :2092-2095, :2215-2239), one thread per map point, in the
 * reference's operation order: cv::Mat products on OpenCV 3.4.1's small-matrix path, cv::norm / Mat::dot accumulated in double,
 * std::log(float) = glibc's logf ("Parity choices of the projector").  The standalone entry points return what
 * the existing matchers take, so the host loops they replace become optional; the fused ones run projector and matcher behind one
 * upload, one wait and one download and return exactly what the two calls in sequence return. */

/* one camera of a frame and its pose */
typedef struct eorb_view {
    float R[9], t[3], Ow[3];           /* mRcw (row-major), mtcw, mOw; right camera: Rrl*mRcw, Rrl*mtcw+trl, mRwc*tlr+mOw (Frame.cc:1257-1263, computed by the caller) */
    eorb_camera cam;                   /* mpCamera / mpCamera2 */
    float minX, maxX, minY, maxY, mbf; /* mnMinX .. mnMaxY, mbf (0 without a rectified right image) */
    int nlevels;    float log_scale;    const float* scale_factors;     /* getORBNLevels, getORBLogScaleFactor, getORBScaleFactor(0 .. nlevels - 1) */
    int ak_nlevels; float ak_log_scale; const float* ak_scale_factors;  /* MixedFrame only, else 0 / NULL (MapPoint.cc:580-584) */
} eorb_view;

/* what isInFrustum leaves in a MapPoint, per point; any pointer may be NULL.  A rejected point keeps proj_xy = (-1, -1) until its
 * bounds test has passed (then uv, as the mono branch leaves mTrackProjX/Y), level = -1, proj_xr = level_scale = 0, view_cos = 0
 * unless it was computed (reason 6); depth = cv::norm(Pc) is written for every point that was not skipped.
 * reason (test aid): 0 in view, 1 skipped by the caller, 2 negative depth, 3 x bounds, 4 y bounds, 5 distance, 6 view cosine,
 * 7 non-finite projection (this library's rule: the reference goes on with a NaN there). */
typedef struct eorb_frustum_out {
    uint8_t* in_view;      /* mbTrackInView / mbTrackInViewR */
    float*   proj_xy;      /* 2 per point: mTrackProjX, mTrackProjY */
    float*   proj_xr;      /* mTrackProjXR = uv.x - mbf * (1.0f / PcZ) */
    int32_t* level;        /* mnTrackScaleLevel */
    float*   view_cos;     /* mTrackViewCos */
    float*   depth;        /* mTrackDepth */
    float*   level_scale;  /* scale factor of `level` in the table PredictScale chose */
    uint8_t* reason;
} eorb_frustum_out;

/* Frame::isInFrustum over M map points and nviews = 1 (Nleft == -1) or 2 (left, right) views.  pos / normal: 3 floats per point
 * (GetWorldPos, GetNormal); min_dist / max_dist = mfMinDistance / mfMaxDistance (the 0.8f / 1.2f of Get*DistanceInvariance are
 * applied here); skip[m] != 0 (optional): the caller's isBad / already-matched points (Tracking.cc:2390-2400), left untouched;
 * mp_is_orb (optional): isORBMapPoint, non-ORB points use the AKAZE tables of a mixed view.  out[v] belongs to views[v];
 * *n_in_view = points in view of at least one view (nToMatch).  M == 0: EORB_OK, nothing written. */
int eorb_project_frustum(eorb_ctx* ctx, const eorb_view* views, int nviews, int M, const float* pos, const float* normal,
                         const float* min_dist, const float* max_dist, const uint8_t* skip, const uint8_t* mp_is_orb, float cos_limit,
                         const eorb_frustum_out* out, int* n_in_view);

/* the projection of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (:1999-2022): view = the current frame, pos =
 * the world position of last-frame point i, skip[i] != 0 (optional) = no map point or an outlier (:1995-1997), last_kps = the last
 * frame's keypoints (octave; getKPtLevelMono), last_is_orb (optional) as mp_is_orb above.  Out, all optional: valid (invzc >= 0, inside
 * the bounds, finite), uv, proj_ur = uv.x - mbf * invzc (:2051), level_scale = the scale factor of the octave.  Trl (optional, 12
 * floats: R row-major then t) and cam_r: uv_r = cam_r->project(Trl * x3Dc) (:2093-2095, no bounds test; the reference passes mpCamera
 * there).  Octaves outside [0, nlevels): EORB_E_ARG. */
int eorb_project_last_frame(eorb_ctx* ctx, const eorb_view* view, const eorb_camera* cam_r, const float* Trl, int n, const float* pos,
                            const uint8_t* skip, const eorb_keypoint* last_kps, const uint8_t* last_is_orb,
                            uint8_t* valid, float* uv, float* proj_ur, float* level_scale, float* uv_r);

/* the projection of ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:2215-2239; relocalisation).  No
 * depth-sign test: a point behind the camera is projected like any other.  view->Ow = -Rcw.t()*tcw (:2196, the caller's); skip[i] != 0
 * = no map point, isBad() or in sAlreadyFound.  Out, all optional: valid, uv, level = PredictScale(dist3D), level_scale, dist3d. */
int eorb_project_keyframe_points(eorb_ctx* ctx, const eorb_view* view, int n, const float* pos, const float* min_dist,
                                 const float* max_dist, const uint8_t* skip, const uint8_t* mp_is_orb,
                                 uint8_t* valid, float* uv, int32_t* level, float* level_scale, float* dist3d);

/* Tracking::SearchLocalPoints (src/Tracking.cc:2390-2430) for a one-camera frame: eorb_project_frustum of one view, then
 * eorb_search_by_projection_map (uright == NULL) or eorb_search_by_projection_map_stereo (uright = mvuRight, proj_xr from the
 * projector) over its results.  bFarPoints / thFarPoints (ORBmatcher.cc:57): a point with depth > thFarPoints stays in_view in `out`
 * but is not searched.  out (optional): the projection arrays, for IncreaseVisible and mmProjectPoints. */
int eorb_search_local_points(eorb_ctx* ctx,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const uint8_t* is_orb,
        const eorb_view* view, int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
        const uint8_t* skip, const uint8_t* mp_is_orb, float cos_limit,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const eorb_grid_bounds* gb, int32_t* frame_mp, float th, float nnratio,
        const float* uright, int bFarPoints, float thFarPoints,
        const eorb_frustum_out* out, int* n_in_view, int* nmatches);

/* the same for a two-camera frame: eorb_project_frustum of views[2], then eorb_search_by_projection_map_fisheye.  The far-point gate
 * reads the left view's depth when the left view accepted the point, else the right view's (the reference reads mTrackDepth, which the
 * right view never writes: a stale member when only the right view accepted). */
int eorb_search_local_points_fisheye(eorb_ctx* ctx,
        const eorb_keypoint* kps, int nL, int nR, const uint8_t* desc, int stride, const int32_t* l2r, const int32_t* r2l,
        const eorb_view* views, int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
        const uint8_t* skip, float cos_limit,
        const uint8_t* mp_desc, const uint8_t* mp_obs, const eorb_grid_bounds* gb, int32_t* frame_mp, float th, float nnratio,
        int bFarPoints, float thFarPoints,
        const eorb_frustum_out* out, int* n_in_view, int* nmatches);

/* TrackWithMotionModel's search: eorb_project_last_frame, then eorb_search_by_projection_last (cur_uright == NULL) or
 * eorb_search_by_projection_last_stereo.  mode (0 none, 1 forward, 2 backward) stays the caller's: tlc is 3 x 3 host algebra.
 * valid / uv (optional): the projection, as eorb_project_last_frame returns it. */
int eorb_search_by_projection_last_pose(eorb_ctx* ctx,
        const eorb_keypoint* cur_kps, int n_cur, const uint8_t* cur_desc, int cur_stride, const uint8_t* cur_is_orb,
        const eorb_view* view, const eorb_keypoint* last_kps, int n_last, const uint8_t* last_is_orb,
        const float* pos, const uint8_t* skip, const uint8_t* mp_desc, const uint8_t* mp_obs,
        const eorb_grid_bounds* gb, int32_t* cur_mp, float th, int mode, int checkOri, const float* cur_uright,
        uint8_t* valid, float* uv, int* nmatches);

/* Relocalization's search: eorb_project_keyframe_points, then eorb_search_by_projection_kf. */
int eorb_search_by_projection_kf_pose(eorb_ctx* ctx,
        const eorb_keypoint* cur_kps, int n_cur, const uint8_t* cur_desc, int cur_stride, const uint8_t* cur_is_orb,
        const eorb_view* view, const eorb_keypoint* kf_kps, int n_kf, const uint8_t* kf_is_orb,
        const float* pos, const float* min_dist, const float* max_dist, const uint8_t* skip, const uint8_t* mp_desc,
        const eorb_grid_bounds* gb, int32_t* cur_mp, float th, int ORBdist, int checkOri,
        uint8_t* valid, float* uv, int32_t* level, int* nmatches);

/* replaces the mono branch of ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:276-478;
 * MixedMatcher.cpp:148-356).  DBoW2::FeatureVector as CSR (node ids ascending, offsets, feature indices in vector
 * order).  kf_has_mp[i] = map point present and !isBad().  match_f[n_f] out = KeyFrame feature index or -1.
 * This is eorb_search_by_bow_keyframes with K = 1 (the KeyFrame as a set of one, a view of these arrays) and inherits its checks and
 * limits: on either side node offsets start at 0 and never decrease and every feature index lies inside the side (EORB_E_ARG, match_f
 * all -1 and *nmatches 0); 2^22 rows, outputs and feature indices (EORB_E_CAPACITY). */
int eorb_search_by_bow(eorb_ctx* ctx,
        const eorb_keypoint* kf_kps, int n_kf, const uint8_t* kf_desc, const uint8_t* kf_has_mp,
        const uint32_t* kf_nodes, const int32_t* kf_node_off, const int32_t* kf_idx, int kf_nn,
        const eorb_keypoint* f_kps, int n_f, const uint8_t* f_desc,
        const uint32_t* f_nodes, const int32_t* f_node_off, const int32_t* f_idx, int f_nn,
        int32_t* match_f, float nnratio, int checkOri, int* nmatches);

/* replaces the mono branch of ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (src/ORBmatcher.cc:833-973; loop
 * closing / place recognition).  match12[n1] out = index of the pKF2 feature, or -1.  This is
 * eorb_search_by_bow_kf_keyframes with K = 1 (pKF2 as a set of one) and inherits its checks and limits, as eorb_search_by_bow does. */
int eorb_search_by_bow_kf(eorb_ctx* ctx,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, const uint8_t* has_mp1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_keypoint* kps2, int n2, const uint8_t* desc2, const uint8_t* has_mp2,
        const uint32_t* nodes2, const int32_t* node_off2, const int32_t* idx2, int nn2,
        int32_t* match12, float nnratio, int checkOri, int* nmatches);

/* replaces the mono branch of ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo=false, bCoarse)
 * (src/ORBmatcher.cc:975-1214; MixedMatcher.cpp:1326-1573; local mapping, f3).  elig1[i] = !pKF1->GetMapPoint(i) &&
 * isORBDescValid(i), elig2 likewise (vbMatched2 is never written by the reference).  ep[2] = the epipole
 * pKF2->mpCamera->project(R2w*Cw+t2w) (:982-987); F12[9] row-major = K1.t().inv()*t12x*R12*K2.inv(), the matrix
 * Pinhole::epipolarConstrain rebuilds for every candidate (Pinhole.cpp:137-140).  scale2[l] = pKF2->getORBScaleFactor(l),
 * sigma2_2[l] = pKF2->getORBLevelSigma2(l).  match12[n1] out = vMatches12 (the caller forms vMatchedPairs, :1203-1211).
 * Rectified stereo: bit 1 of elig1[i] / elig2[i] set = the keypoint has a right coordinate (bStereo1 / bStereo2: mvuRight >= 0, :1051,
 * :1079): the epipole-distance test (:1093-1100) is skipped for a pair with such a keypoint; bOnlyStereo = clear bit 0 of the others.
 * This is eorb_search_for_triangulation_keyframes with K = 1 (pKF2 as a set of one, a view of these arrays with stride2 its stride) and
 * inherits its checks and limits, as eorb_search_by_bow does. */
int eorb_search_for_triangulation(eorb_ctx* ctx,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_keypoint* kps2, int n2, const uint8_t* desc2, int stride2, const uint8_t* elig2,
        const uint32_t* nodes2, const int32_t* node_off2, const int32_t* idx2, int nn2,
        const float* ep, const float* F12, const float* scale2, const float* sigma2_2, int nlevels,
        int bCoarse, int checkOri, int32_t* match12, int* nmatches);

/* the same matcher when pCamera1 is KannalaBrandt8 (fisheye: MVSEC, TUM-VI): epipolarConstrain = TriangulateMatches(...) >
 * KB8_DEF_TH_EPC (src/CameraModels/KannalaBrandt8.cpp:315-320, :416-486), and the two-camera branch (:1007-1017, :1058-1135).
 * nleft1 / nleft2 = numAllKPtsLeft():
 *   both -1: monocular keyframes; kps = getUndistKPtMono; Rt[0..11] = R12 (row-major) then t12 (:1001-1002); the epipole test
 *            ep / scale2 (:1097-1104) applies, with elig bit 1 (bStereo) as in eorb_search_for_triangulation;
 *   both >= 0: two-camera keyframes; kps = the nleft distorted left keypoints then the right ones; Rt[48] = ll, lr, rl, rr
 *            (:1005-1013), each R row-major then t; the pose and cameras follow (idx1 >= nleft1, idx2 >= nleft2); no epipole
 *            test and bStereo false (elig bit 1 ignored); ep / scale2 are still read;
 *   one -1 and the other not: EORB_E_CONFIG (the reference's R12 is an empty cv::Mat there).
 * cam1[2] / cam2[2] = mpCamera, mpCamera2 of pKF1 / pKF2 (only [0] read for monocular pairs).  pCamera1 (cam1[0], and cam1[1] for
 * two cameras) must be model 1, else EORB_E_CONFIG: a Pinhole pCamera1 is eorb_search_for_triangulation.  pCamera2 may be
 * either model.  sigma2_1 / sigma2_2 = getORBLevelSigma2 of pKF1 / pKF2 (both keyframes share nlevels); eligible keypoints of
 * both keyframes need an octave in [0, nlevels).  Outputs as eorb_search_for_triangulation: ties go to the last passing
 * candidate, the rotation histogram keeps its three maxima.  One upload, one wait, one download.  This is
 * eorb_search_for_triangulation_kb8_keyframes with K = 1 and inherits its checks and limits, as eorb_search_by_bow does. */
int eorb_search_for_triangulation_kb8(eorb_ctx* ctx,
        const eorb_keypoint* kps1, int n1, int nleft1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_keypoint* kps2, int n2, int nleft2, const uint8_t* desc2, int stride2, const uint8_t* elig2,
        const uint32_t* nodes2, const int32_t* node_off2, const int32_t* idx2, int nn2,
        const eorb_camera* cam1, const eorb_camera* cam2, const float* Rt, const float* ep,
        const float* scale2, const float* sigma2_1, const float* sigma2_2, int nlevels,
        int bCoarse, int checkOri, int32_t* match12, int* nmatches);

/* KannalaBrandt8::TriangulateMatches (src/CameraModels/KannalaBrandt8.cpp:416-486) over n pairs (kps1[i], kps2[i]):
 * z1[i] = the triangulated depth in camera 1, or -1.  cam1 must be model 1 (EORB_E_CONFIG otherwise), cam2 either model;
 * Rt[12] = R12 row-major then t12; the sigmas are read at each keypoint's octave. */
int eorb_kb8_triangulate_matches(eorb_ctx* ctx, const eorb_camera* cam1, const eorb_camera* cam2, const float* Rt,
        const eorb_keypoint* kps1, const eorb_keypoint* kps2, int n, const float* sigma2_1, const float* sigma2_2, int nlevels,
        float* z1);

/* ---- TwoViewReconstruction (src/TwoViewReconstruction.cc): the two stages whose cost grows with the match count ----------------------
 * The call after SearchForInitialization in Tracking::MonocularInitialization (src/Tracking.cc:3559) and after the KLT match of the
 * event trackers (EvImBuilder.cpp:622, EvAsynchTracker.cpp:1044, ...).  What stays with the caller of these two is 3x3 algebra and
 * decisions: the set draw (DUtils::Random, :107-124), SH/(SH+SF) and the H/F choice, K.t()*F21*K, DecomposeE, the Faugeras decomposition
 * of ReconstructH, resolveReconstStat*, and the acos of the parallax.  eorb_two_view_reconstruct, after them, is Reconstruct whole.
 *
 * Limits, decided from the sizes before any array is read (EORB_E_CAPACITY): */
#define EORB_TVR_MAX_ITERS    1024
#define EORB_TVR_MAX_MATCHES  16384
#define EORB_TVR_MAX_KEYS     1048576
#define EORB_TVR_MAX_POSES    64
typedef struct eorb_tvr_params {
    float sigma;        /* mSigma */
    float th_score;     /* mParams2VR.mThChiSqScore, 5.991f */
    float th_f;         /* mParams2VR.mThChiSqF, 3.841f */
} eorb_tvr_params;
/* one pose hypothesis of CheckRT: R, t, and the caller's 3x3 algebra P2 = K*[R|t] (3x4 row-major) and O2 = -R.t()*t */
typedef struct eorb_tvr_pose { float R[9]; float t[3]; float P2[12]; float O2[3]; } eorb_tvr_pose;

/* replaces the two threads of Reconstruct (:131-136 / :228-233): FindHomography (:264-312) and FindFundamental (:315-363) with Normalize
 * (:1193-1239), ComputeH21 (:366-406), ComputeF21 (:408-443), CheckHomography (:445-528) and CheckFundamental (:530-608).
 * kps1[n1] / kps2[n2]: ALL keys of the two frames (only x, y are read; Normalize runs over every key, matched or not, in index order);
 * match12[N][2]: the mvMatches12 pairs (first, second) in order; sets[iters][8]: indices into match12, drawn by the caller.
 * Results: H21[9] / F21[9] row-major, SH / SF, best_it_h / best_it_f, inliers_h[N] / inliers_f[N] (0 / 1).  The winner is the first
 * iteration whose score is > the running best, which starts at 0.0f (:305, :356): equal scores keep the earlier iteration and a NaN
 * score never wins.  When no iteration scores above 0: best_it = -1, the matrix is zeros and the flags are zeros; the reference leaves
 * H21 / F21 empty cv::Mats there, and FindFundamental's inlier vector has length 0, because it takes N from the size of its output
 * argument (:318) -- which is also why a caller that passes a non-empty vector gets N flags.
 * Test aids, NULL to skip: it_score_h[iters], it_score_f[iters], it_H[iters*9], it_F[iters*9] (every iteration's score, H21i, F21i).
 * EORB_E_ARG: N < 8, iters < 1, a set index outside [0, N), a match index outside the key arrays.  The OpenCV 3.4.1 arithmetic
 * (JacobiSVDImpl_<float> with its cv::RNG completion, gemm's small-matrix branch, Mat::inv 3x3) is restated on its scalar paths:
 * DESIGN.md section 2. */
int eorb_two_view_ransac(eorb_ctx* ctx, const eorb_keypoint* kps1, int n1, const eorb_keypoint* kps2, int n2, const int32_t* match12, int N,
        const int32_t* sets, int iters, const eorb_tvr_params* params,
        float* H21, float* SH, int32_t* best_it_h, uint8_t* inliers_h, float* F21, float* SF, int32_t* best_it_f, uint8_t* inliers_f,
        float* it_score_h, float* it_score_f, float* it_H, float* it_F);

/* CheckRT (:1242-1352) with Triangulate (:1177-1191) for Kp pose hypotheses (the 4 of ReconstructF :633-636, the 8 of ReconstructH).
 * inliers[N]: vbMatchesInliers; K: 3x3 row-major (fx, fy, cx, cy and P1 = K[I|0] are copies); min_parallax_crt: mMinParallaxCRT as the
 * float the reference narrows 0.99998 into.  Per pose h: n_good[h]; good[h*n1 + first] = vbGood; p3d[(h*n1 + first)*3 ..] = vP3D, zeros
 * where not written -- written for every counted match, not only the good ones (:1334); cos_sel[h] = vCosParallax[min(min_triangulated,
 * size - 1)] after the ascending sort, or 0 when n_good == 0: parallax = acos(cos_sel)*180/CV_PI in double stays with the caller.  The
 * sort orders -0 before +0 and every NaN last (returned as the canonical NaN); std::sort in the reference is undefined with a NaN.
 * cos_all (NULL to skip): Kp*N, the cosParallax of each counted match, -2 for a match that was not counted.
 * EORB_E_ARG: a match index outside the key arrays, two matches with the same first index (mvMatches12 has none), min_triangulated < 0. */
int eorb_two_view_check_rt(eorb_ctx* ctx, const eorb_keypoint* kps1, int n1, const eorb_keypoint* kps2, int n2, const int32_t* match12, int N,
        const uint8_t* inliers, const float* K, float th2, float min_parallax_crt, int min_triangulated,
        const eorb_tvr_pose* poses, int Kp, int32_t* n_good, uint8_t* good, float* p3d, float* cos_sel, float* cos_all);

/* TwoViewReconstruction::Reconstruct as one call: the two stages above and everything the reference does between and after them -- the
 * SH+SF == 0 exit, RH = SH/(SH+SF) and the H/F choice, K.t()*F21*K and DecomposeE (:1354-1375) or the Faugeras decomposition of
 * ReconstructH, P2 = K*[R|t] and O2 = -R.t()*t of CheckRT (:1258-1270), CheckRT for the 4 or 8 hypotheses, the acos of the parallax, and
 * the decision.  One upload, one wait, one download; nothing returns to the host between the stages.  What stays with the caller: the
 * set draw (DUtils::Random, :107-124) and KannalaBrandt8's un-distortion of the keys before the call.
 * Keys, matches and sets mean what they mean in eorb_two_view_ransac, with its limits (EORB_TVR_MAX_*, EORB_E_CAPACITY from the sizes,
 * before any array is read) and errors; EORB_E_ARG besides for N < 8, a match or set index out of range, two matches with one `first`
 * index (as eorb_two_view_check_rt), min_triangulated < 0, or a form that is neither of the two. */
#define EORB_TVR_FORM_STOCK 0   /* Reconstruct :67-158 with ReconstructF :610-710, ReconstructH :712-873 */
#define EORB_TVR_FORM_INFO  1   /* Reconstruct :162-262 with ReconstructF :902-979, ReconstructH :991-1175 */
typedef struct eorb_tvr_recon_params {
    float sigma, th_score, th_f;             /* as eorb_tvr_params */
    float th_hf_ratio;                       /* mThHFRatio 0.45f */
    float min_parallax;                      /* mDefMinParallax 1.0f */
    float min_parallax_crt;                  /* (float)0.99998 */
    int   min_triangulated;                  /* 50 */
    float th_min_good_r, th_max_good_r_f, th_max_good_r_h;   /* 0.9f 0.7f 0.75f */
    float th_rd_homo;                        /* (float)1.00001 */
    int   form;
} eorb_tvr_recon_params;
typedef struct eorb_tvr_recon_result {
    int32_t ok;              /* what Reconstruct returns */
    int32_t stage;           /* 0: SH+SF == 0;  1: ReconstructH left at the d1/d2, d2/d3 test;  2: hypotheses checked */
    int32_t is_homography;   /* RH > th_hf_ratio */
    float   SH, SF, RH;  int32_t best_it_h, best_it_f;  float H21[9], F21[9];
    int32_t n_inliers;       /* N of ReconstructF / ReconstructH */
    int32_t n_min_good, n_similar;           /* F forms; 0 in the H forms */
    int32_t n_hyp;           /* 4 or 8; 0 when stage < 2 */
    int32_t hyp_good[8]; float hyp_parallax[8];   /* per hypothesis in hypothesis order (R1t1, R2t1, R1t2, R2t2 / vR[0..7]) */
    int32_t info_good[8];    /* ReconstInfo::mvnGood as the reference writes it: F sorted descending in [0..3], H in hypothesis order */
    int32_t hyp_best, hyp_second;            /* hypothesis index of slot 0 / slot 1, -1: none */
    int32_t best_good, second_good; float best_parallax, second_parallax;
} eorb_tvr_recon_result;
/* Outputs: R21[2][9], t21[2][3], p3d[2][n1][3] (vP3D, indexed by `first`), triangulated[2][n1] (vbTriangulated), trans_inliers[N],
 * hyp_poses[8] (test aid, NULL to skip: the hypotheses as CheckRT takes them, zeros past n_hyp).  A slot that is not written is zeros.
 * - stage 0 (SH+SF == 0.f): ok = 0, RH = 0, is_homography = 0, n_inliers = 0, everything after F21 in the result is zero (hyp_best =
 *   hyp_second = -1).  stage 1: is_homography = 1, n_inliers is counted, n_hyp = 0, the rest as at stage 0.  At either, every output array
 *   is zero apart from trans_inliers below.
 * - STOCK form.  Slot 0 is written only when ok == 1, and hyp_best is then its hypothesis (else -1); the reference leaves R21 empty
 *   otherwise.  Slot 1, hyp_second (-1), second_parallax, info_good (the form has no ReconstInfo) and trans_inliers are always zero.
 *   F: best_good = maxGood, best_parallax = the parallax of the first hypothesis whose count equals maxGood (the one the if / else-if
 *   chain :663-707 looks at), second_good = 0.  H: best_good / second_good / best_parallax as the walk :837-858 leaves them
 *   (best_parallax = -1 when no hypothesis has nGood > 0).
 * - INFO form, F.  Slots 0 and 1 are the first two entries of the multimap<int, ..., greater<int>> (:937-971): descending nGood, equal
 *   counts in insertion order 1, 2, 3, 4 (C++11 inserts an equal key at the upper bound).  info_good[0..3] is that sorted order and
 *   [4..7] are 0 -- a reused ReconstInfo would keep stale values there, which resolveReconstStatF then counts: the caller's business.
 *   ok = resolveReconstStatF (:876-900); n_similar is its unsigned char.
 * - INFO form, H.  Slots 0 and 1 follow the best / second walk of :1118-1148 (strict >: the earlier hypothesis keeps a tie; a new best
 *   hands the old best down to second).  The reference reads vR[-1] (:1160, :1167) when no hypothesis, or only one, has nGood > 0:
 *   undefined behaviour.  Here such a slot is zeros with index -1 (its parallax field keeps the walk's initial -1); ok still follows
 *   resolveReconstStatH (:981-989), which is false then.  info_good is nGood in hypothesis order.
 * - trans_inliers (vbTransInliers; INFO only, zeros in STOCK): at stage 0 inliers_f (:237), otherwise the chosen model's flags (:906,
 *   :995), also at stage 1.
 * - Comparisons keep the reference's types: nGood > thMaxGoodR*maxGood compares floats (an int against a float product in the STOCK
 *   form, (float)nGood > thMaxGoodR*float(maxGood) in the INFO form); nMinGood = max(static_cast<int>(mThMinGoodR*N), minTriangulated)
 *   with the product in float; d1/d2 < thRDH and d2/d3 < thRDH in float; th2 = 4.0f*(sigma*sigma); RH > th_hf_ratio and SH+SF == 0.f in
 *   float; parallax = (float)(acos((double)cos)*180/CV_PI), 0 when nGood == 0, with acos as fdlibm's e_acos.c on both sides.
 * - NaN.  A NaN anywhere makes its comparison false as IEEE has it; nothing is special-cased.
 * The OpenCV 3.4.1 arithmetic is restated on its scalar paths and pinned to nothing outside this repository. */
int eorb_two_view_reconstruct(eorb_ctx* ctx, const eorb_keypoint* kps1, int n1, const eorb_keypoint* kps2, int n2,
        const int32_t* match12, int N, const int32_t* sets, int iters, const float* K, const eorb_tvr_recon_params* p,
        eorb_tvr_recon_result* res, float* R21 /*[2][9]*/, float* t21 /*[2][3]*/, float* p3d /*[2][n1][3]*/,
        uint8_t* triangulated /*[2][n1]*/, uint8_t* trans_inliers /*[N]*/, eorb_tvr_pose* hyp_poses /*[8], test aid, NULL to skip*/);

/* ---- Sim3Solver (src/Sim3Solver.cc): Horn's closed form and its RANSAC loop ------------------------------------------------------------
 * The stage between SearchByBoW(KF, KF) and SearchByProjection(KF, Scw) in LoopClosing::DetectCommonRegionsFromBoW
 * (src/LoopClosing.cc:690-701): one solver per BoW candidate, so one call solves K independent problems; a single solver is K = 1.
 * What stays with the caller: the constructor's filter (:71-91: null, isBad, index < 0) and the mvnIndices1 map, the iteration count of
 * SetRansacParameters (:137-147), the set draw (DUtils::Random, :178-189), and the g2o::Sim3 composition after the solver.
 *
 * Limits, decided from the sizes before any array is read (EORB_E_CAPACITY): */
#define EORB_S3_MAX_ITERS     1024
#define EORB_S3_MAX_CORR      16384   /* per problem */
#define EORB_S3_MAX_PROBLEMS  64
/* One problem.  The per-correspondence and per-set arrays of a call are flat: problem k owns the N correspondences after those of the
 * problems before it (rows sum(N[0..k)) ...), and the iters sets after theirs; the outputs inliers and it_* are laid out the same way. */
typedef struct eorb_sim3_problem {
    int32_t N;              /* correspondences the caller has already compacted (>= 3) */
    int32_t iters;          /* mRansacMaxIts after SetRansacParameters (>= 1): the sets drawn for this problem */
    int32_t fix_scale;      /* mbFixScale */
    int32_t min_inliers;    /* mRansacMinInliers */
    float Rt1[12], Rt2[12]; /* Rcw row-major then tcw of pKF1 / pKF2: the device computes mvX3Dc = Rcw*Xw + tcw (:107, :110) */
    eorb_camera cam1, cam2; /* pCamera1 / pCamera2, either model */
} eorb_sim3_problem;
typedef struct eorb_sim3_result {
    int32_t converged;        /* bConverge */
    int32_t best_it;          /* the iteration the results come from, -1 when N < min_inliers */
    int32_t n_inliers;        /* its count */
    int32_t iterations_used;  /* mnIterations when "while(!bConverge && !bNoMore) iterate(20, ...)" ends */
    float T12[16], R12[9], t12[3], s12;      /* mBestT12, mBestRotation, mBestTranslation, mBestScale */
} eorb_sim3_result;

/* Sim3Solver::iterate (:221-297) run to its end for K problems: ComputeSim3 (:316-427) and CheckInliers (:430-454) of every set, then the
 * state the loop of LoopClosing.cc:698-701 is left in.
 * Xw1 / Xw2 [sum N][3]: GetWorldPos() of both sides; sigma2_1 / sigma2_2 [sum N]: getKPtLevelSigma2 per correspondence (a mixed keyframe
 * passes its AKAZE sigmas the same way); sets [sum iters][3]: indices into the problem's own N correspondences, drawn by the caller
 * (repeated indices inside a set are accepted: the arithmetic is defined).
 * The inlier bound is the reference's: mvnMaxError is a vector<size_t> (include/Sim3Solver.h:78-79), so 9.210*sigma2 is truncated to an
 * integer and err < bound compares the float error with that integer (:446): 9 at sigma2 = 1, and 0 -- no inlier ever -- at 0.1.
 * The result rule (:268-290): the running best starts at 0 and is replaced on >=, so among equal counts the later iteration wins; the
 * first iteration whose count is > min_inliers ends the search (any earlier best was <= min_inliers); a count equal to min_inliers does
 * not converge.  N < min_inliers (:228-232): converged = 0, best_it = -1, iterations_used = 0, everything else zero.  When nothing
 * converges the running best is returned anyway, with converged = 0 and iterations_used = iters; the reference hands back only what the
 * last chunk of 20 improved, and its caller ignores that unless bConverge.
 * results[K]; inliers[sum N] (0 / 1, in compacted order).  Test aids, NULL to skip, with which a caller can replay any chunking of
 * iterate: it_inliers[sum iters], it_T12[sum iters * 16], it_T21[sum iters * 16], it_scale[sum iters] (zeros for a problem with
 * N < min_inliers).  Identical point triples give an all-NaN transform with 0 inliers (:370, 0/0), as in the reference.
 * EORB_E_ARG: K < 1, N < 3, iters < 1, min_inliers < 0, a set index outside [0, N), a sigma2 that is negative, NaN or >= 1e15 (its
 * conversion to size_t is undefined in the source).  EORB_E_CONFIG: a camera model other than 0 / 1.  No output is written on an error.
 * The OpenCV 3.4.1 arithmetic (reduce, gemm, JacobiImpl_<float> of cv::eigen, Rodrigues, the MatExpr folds) is restated on its scalar
 * paths: DESIGN.md section 2. */
int eorb_sim3_ransac(eorb_ctx* ctx, const eorb_sim3_problem* problems, int K, const float* Xw1, const float* Xw2,
        const float* sigma2_1, const float* sigma2_2, const int32_t* sets,
        eorb_sim3_result* results, uint8_t* inliers, int32_t* it_inliers, float* it_T12, float* it_T21, float* it_scale);

/* ---- MLPnPsolver (src/MLPnPsolver.cpp): the pose RANSAC of Tracking::Relocalization ---------------------------------------------------
 * The stage between SearchByBoW(KF, F) and PoseOptimization in Tracking::Relocalization (src/Tracking.cc:2697-2729): one solver per
 * candidate keyframe, so one call solves K independent problems; a single solver is K = 1.
 * What stays with the caller: the constructor's filter (:67-96: null, isBad) and mvKeyPointIndices, the iteration count and the minimum
 * inliers of SetRansacParameters (:268-298), the set draw (DUtils::Random, :176-188), and everything after the solver.
 * What the device computes: the bearing vectors (unproject of the undistorted keypoint, then /= z, in float, either camera model,
 * :80-82), mvMaxError[i] = sigma2[i]*th2 as a float product (:302), computePose (:395-701) with mlpnp_gn (:737-802) and
 * mlpnp_residuals_and_jacs (:804-851), CheckInliers (:305-336), and what Refine (:338-392) returns (below).
 *
 * Limits, decided from the sizes before any array is read (EORB_E_CAPACITY).  The correspondence limit is a choice: a frame's BoW
 * matches with one keyframe do not approach it. */
#define EORB_PNP_MAX_ITERS     1024
#define EORB_PNP_MAX_CORR      4096    /* per problem */
#define EORB_PNP_MAX_PROBLEMS  64
/* One problem; the flat layout of eorb_sim3_problem: problem k's correspondences and sets follow those of the problems before it. */
typedef struct eorb_mlpnp_problem {
    int32_t N;              /* correspondences the caller has already compacted (>= 6) */
    int32_t iters;          /* the sets passed for this problem (>= 1): iterations [0, iters) of this solver */
    int32_t min_inliers;    /* mRansacMinInliers after the clamps of :280-285 (>= 6: the reference's Refine calls computePose on that many points) */
    float th2;              /* SetRansacParameters' th2 (5.991) */
    eorb_camera cam;        /* F.mpCamera, either model */
    int32_t first_it;       /* the iteration the walk starts at: 0 for a fresh solver */
    int32_t best_it;        /* the running best carried in, an index into the same sets below first_it, or -1: a fresh solver */
} eorb_mlpnp_problem;
typedef struct eorb_mlpnp_result {
    int32_t stop_it;          /* the iteration at which Refine returned true, else -1 */
    int32_t iterations_used;  /* mnIterations when the walk ends: stop_it + 1, else iters; 0 when N < min_inliers */
    int32_t best_it, n_best;  /* the running best the loop is left with (mvbBestInliers / mnBestInliers): -1, 0 when there is none */
    int32_t refined;          /* 1: Tcw is mRefinedTcw and inliers are mvbRefinedInliers: the pose and flags of iteration stop_it */
    int32_t n_inliers;        /* mnRefinedInliers (the count of iteration stop_it), else n_best when n_best >= min_inliers, else 0 */
    float Tcw[16];            /* mRefinedTcw when refined, else mBestTcw when n_best >= min_inliers, else zeros */
} eorb_mlpnp_result;

/* MLPnPsolver::iterate (:149-266) run to its end for K problems.
 * p2d [sum N][2]: the undistorted keypoints; Xw [sum N][3]: GetWorldPos(); sigma2 [sum N]: getKPtLevelSigma2; sets [sum iters][6]:
 * indices into the problem's own N correspondences, drawn by the caller (repeated indices inside a set are accepted: the arithmetic is
 * defined, and a set of fewer than six distinct points gives a rank-deficient system, a NaN or a poor pose, and few inliers).
 * The result rule (:163-265).  The running best starts at 0 and is replaced on > only (:220), so among equal counts the earlier
 * iteration stays.  An iteration whose count is >= min_inliers (:217) invokes Refine.  Refine (:338-392) runs computePose on the running
 * best's inliers into a local `result` that it never stores (:367-371): mRi / mti are written only at :200-212, so its CheckInliers
 * (:374) counts the current hypothesis again.  Hence mnRefinedInliers is this iteration's count, Refine returns true exactly when that
 * is > min_inliers (:379, strict, unlike the trigger), and mRefinedTcw / mvbRefinedInliers are this iteration's pose and flags.  The
 * pose Refine computes affects nothing that is returned, and the device does not compute it; this reproduces the reference, it does not
 * repair it.  The call ends at the first iteration whose count is > min_inliers; a count equal to min_inliers becomes the running best
 * and the walk goes on.  N < min_inliers (:154-158): stop_it = best_it = -1, iterations_used = 0, everything else zero.  When no Refine
 * succeeds the running best is returned as :249-262 do.
 * Resuming (Relocalization calls iterate(5, ...) again on a solver whose pose failed PoseOptimization) needs no device state: first_it
 * is where the walk starts, best_it the running best carried in; the device computes that one hypothesis and its flags again.
 * results[K]; inliers[sum N] (0 / 1, in compacted order).  Test aids, NULL to skip: it_inliers[sum iters]; it_Rt[sum iters][12] as
 * double, mRi row-major then mti of every hypothesis; it_refine_inliers[sum iters]: mnRefinedInliers at every iteration the rule
 * invoked Refine at (the iteration's own count again, up to and including stop_it), -1 elsewhere.  Iterations
 * below first_it other than best_it are not computed: their aids are zero (it_refine_inliers -1).
 * A NaN coordinate gives NaN errors, which fail their <.  EORB_E_ARG: K < 1, N < 6, iters < 1, min_inliers < 6, first_it outside
 * [0, iters), best_it outside [-1, first_it), a set index outside [0, N).  EORB_E_CONFIG: a camera model other than 0 / 1.  No output is
 * written on an error.  Eigen 3.3's algorithms (JacobiSVD, FullPivHouseholderQR, SelfAdjointEigenSolver, LDLT, the small products)
 * are restated on their scalar paths: DESIGN.md section 2. */
int eorb_mlpnp_ransac(eorb_ctx* ctx, const eorb_mlpnp_problem* problems, int K, const float* p2d, const float* Xw, const float* sigma2,
        const int32_t* sets, eorb_mlpnp_result* results, uint8_t* inliers, int32_t* it_inliers, double* it_Rt, int32_t* it_refine_inliers);

/* replaces the search core shared by ORBmatcher::Fuse (src/ORBmatcher.cc:1512-1578 and :1700-1720), SearchBySim3
 * (:1829-1860, :1909-1940) and SearchByProjection(KeyFrame*, Scw, ...) (:548-588, :667-706): for every projected map point
 * m (valid[m], uv, radius = th*getORBScaleFactor(level), predicted level, descriptor) the best keypoint among
 * KeyFrame::GetFeaturesInArea(u, v, radius) (src/KeyFrame.cc:873-917) with octave in [level-1, level].  This entry point takes
 * projections the caller computed; eorb_fuse_pose, eorb_search_by_projection_kf_scw, eorb_search_by_sim3 and eorb_fuse_keyframes
 * below project on the device in front of the same search.  The map update stays with the caller.
 *   inv_sigma2 != NULL : Fuse's mono reprojection gate e2*inv_sigma2[octave] > 5.99 (:1557-1564)
 *   taken != NULL      : n flags in/out, SearchByProjection(KF,Scw) semantics: queries in order, flagged keypoints skipped,
 *                        taken[best] = 1 when (float)best_dist <= accept_thr (= TH_LOW*ratioHamming, :582-586)
 * best_idx[m] = -1 and best_dist[m] = 256 when no keypoint qualifies. */
int eorb_kf_radius_match(eorb_ctx* ctx,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
        int M, const uint8_t* valid, const float* uv, const float* radius, const int32_t* level, const uint8_t* q_desc,
        const float* inv_sigma2, int nlevels, uint8_t* taken, float accept_thr, int32_t* best_idx, int32_t* best_dist);
/* Fuse on a rectified-stereo KeyFrame (src/ORBmatcher.cc:1541-1553; the same in the Sim3 overload :1683-): a keypoint with a right
 * coordinate (uright[i] = pKF->mvuRight[i] >= 0) is gated by the three-term error ex^2 + ey^2 + (q_ur[m] - uright[i])^2 against 7.8
 * instead of the two-term one against 5.99; q_ur[m] = u - bf * invz of map point m.  inv_sigma2 must be given. */
int eorb_kf_radius_match_stereo(eorb_ctx* ctx,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
        int M, const uint8_t* valid, const float* uv, const float* radius, const int32_t* level, const uint8_t* q_desc,
        const float* inv_sigma2, int nlevels, const float* uright, const float* q_ur, int32_t* best_idx, int32_t* best_dist);

/* ---- KeyFrame-side matchers with the projection on the device ----------------------------------------------------------------------
 * The projection loops in front of that search core, one thread per (keyframe, map point), in the reference's operation order with
 * its double steps, then the search behind the same upload, wait and download.  These five serve ORB keyframes
 * and ignore the views' AKAZE tables; MixedMatcher's forms on a MixedKeyFrame (type gate, per-keypoint level and sigma, AKAZE tables)
 * are the *_mixed entry points further down.  The Sim3 decomposition
 * (sRcw/scw, Ow = -Rcw.t()*tcw, :1628-1632) and the right camera's pose of bRight (:1400-1425) are 3 x 3 host algebra on cv::Mat
 * expressions and stay with the caller, who hands the result in as an eorb_view.
 *
 * mode D, the sequence shared by Fuse(pKF, vpMapPoints, th, bRight) (src/ORBmatcher.cc:1463-1513), Fuse(pKF, Scw, ...) (:1650-1690)
 * and both SearchByProjection(pKF, Scw, ...) (:511-550, :595-): p3Dc = Rcw*p3Dw + tcw; p3Dc.z < 0 rejected (a zero depth goes on);
 * uv = camera.project(p3Dc); KeyFrame::IsInImage (src/KeyFrame.cc:919-922: x >= minX && x < maxX, the upper bound strict, unlike
 * Frame's; a NaN or an infinity fails here by itself); dist3D = (float)cv::norm(p3Dw - Ow) inside [0.8f*min_dist, 1.2f*max_dist];
 * PO.dot(Pn) < 0.5*dist3D rejected, a comparison of doubles; level = PredictScale(dist3D); radius = th * scale_factors[level];
 * q_ur = uv.x - mbf * (1/z).
 * Per point, any pointer may be NULL: valid, uv, radius, level, q_ur are what eorb_kf_radius_match[_stereo] takes.  A rejected point
 * keeps uv = (-1, -1) and q_ur = 0 until IsInImage has passed, dist3d = 0 until it was computed, level = -1, radius = 0.
 * reason: 0 accepted, 1 skipped by the caller, 2 negative depth, 3 outside the image, 5 distance, 6 viewing angle. */
typedef struct eorb_kfside_out {
    uint8_t* valid; float* uv; float* radius; int32_t* level; float* q_ur; float* dist3d; uint8_t* reason;
} eorb_kfside_out;

/* mode D alone for one view.  skip[m] != 0 (optional): no map point, isBad(), IsInKeyFrame(pKF) / spAlreadyFound (:1443-1460, :1647).
 * M == 0: EORB_OK, nothing written. */
int eorb_project_keyframe_side(eorb_ctx* ctx, const eorb_view* view, int M, const float* pos, const float* normal, const float* min_dist,
                               const float* max_dist, const uint8_t* skip, float th, const eorb_kfside_out* out);

/* replaces ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) up to the map update (:1439-1578): mode D, then the radius match of
 * eorb_kf_radius_match (uright == NULL) or eorb_kf_radius_match_stereo (uright = pKF->mvuRight, q_ur from the projector) over its
 * results; inv_sigma2[view->nlevels].  inv_sigma2 == NULL: the Sim3 overload Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
 * (:1642-1720), which has no reprojection gate.  best_idx / best_dist as eorb_kf_radius_match returns them: the caller thresholds
 * with TH_LOW (:1581, :1723).  bRight: the caller passes the right camera's view, keypoints, descriptors and grid and adds
 * numAllKPtsLeft() to the indices (:1567).  out (optional): the projection.  Returns exactly what eorb_project_keyframe_side and
 * eorb_kf_radius_match[_stereo] in sequence return. */
int eorb_fuse_pose(eorb_ctx* ctx, const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
                   const eorb_view* view, int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                   const uint8_t* skip, const uint8_t* q_desc, const float* inv_sigma2, const float* uright, float th,
                   int32_t* best_idx, int32_t* best_dist, const eorb_kfside_out* out);

/* replaces both ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, [vpPointsKFs,] vpMatched, th, ratioHamming) (:487-590, :592-706)
 * up to the assignment of vpMatched: mode D, then the in-order form of eorb_kf_radius_match (taken[n] in / out = keypoints holding a
 * vpMatched entry, accept_thr = TH_LOW*ratioHamming). */
int eorb_search_by_projection_kf_scw(eorb_ctx* ctx, const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
                                     const eorb_view* view, int M, const float* pos, const float* normal, const float* min_dist,
                                     const float* max_dist, const uint8_t* skip, const uint8_t* q_desc, float th, uint8_t* taken,
                                     float accept_thr, int32_t* best_idx, int32_t* best_dist, const eorb_kfside_out* out);

/* replaces ORBmatcher::SearchBySim3 (:1743-1967) in one call: both projections (mode E, :1799-1830 and :1879-1910: two chained
 * products R1w*p + t1w, sR21*(.) + t21; z < 0 rejected; invz = (float)(1.0/z); u = fx*(X*invz) + cx; IsInImage of the searched
 * keyframe; dist3D = (float)cv::norm(p3Dc2), the camera-frame norm, inside the invariance region; no camera centre and no viewing
 * angle), both radius matches (:1832-1866, :1912-1946, bestDist <= th_high = TH_HIGH) and the agreement pass (:1948-1964).
 * Per keyframe: keypoints, descriptors, grid bounds, the view (pose, IsInImage bounds, scale tables), and per keypoint slot i the
 * map point's pos / min_dist / max_dist / descriptor with skip[i] != 0 for no map point, isBad() or vbAlreadyMatched (:1773-1783).
 * sR12, t12, sR21, t21: the caller's (:1760-1762).  fx, fy, cx, cy are view1's in both directions, as the reference reads pKF1's
 * (:1746-1749).  Pinhole only: a KannalaBrandt8 view returns EORB_E_CONFIG.  match12[n1] = index in KF2 or -1; vnMatch1[n1] /
 * vnMatch2[n2] (optional): the two searches before the agreement pass.  An empty side: EORB_OK, every output -1, *nfound = 0. */
int eorb_search_by_sim3(eorb_ctx* ctx,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, int stride1, const eorb_grid_bounds* gb1, const eorb_view* view1,
        const float* pos1, const float* min_dist1, const float* max_dist1, const uint8_t* mp_desc1, const uint8_t* skip1,
        const eorb_keypoint* kps2, int n2, const uint8_t* desc2, int stride2, const eorb_grid_bounds* gb2, const eorb_view* view2,
        const float* pos2, const float* min_dist2, const float* max_dist2, const uint8_t* mp_desc2, const uint8_t* skip2,
        const float* sR12, const float* t12, const float* sR21, const float* t21, float th, int th_high,
        int32_t* match12, int* nfound, int32_t* vnMatch1, int32_t* vnMatch2);

/* Fuse of M shared map points into K keyframes at once: LocalMapping::SearchInNeighbors (src/LocalMapping.cc:840-892) and
 * LoopClosing::SearchAndFuse (src/LoopClosing.cc:2348-2420) up to the map update.  views[K], gb[K]; keypoints / descriptors /
 * optional uright of all keyframes concatenated, keyframe k = rows kf_off[k] .. kf_off[k+1]-1 (the convention of
 * eorb_distinctive_descriptors); one inv_sigma2[nlevels] / scale_factors table (views[0]'s; every view must name the same pyramid)
 * serves all keyframes, inv_sigma2 == NULL = the Sim3 overload; skip[K*M] (optional) = isBad() and IsInKeyFrame(pKF_k) at call time.
 * best_idx[K*M] (relative to the keyframe) / best_dist[K*M] / reason[K*M] (optional): entry k*M + m is what eorb_fuse_pose returns
 * for keyframe k and point m.  Limits: K <= 1024, K*M <= 2^22, 2^22 keypoints in all; beyond them EORB_E_CAPACITY.
 *
 * Why the batch is exact: the search result of (k, m) depends only on geometry, descriptors and keyframe k's keypoints, and
 * Replace / AddObservation / AddMapPoint change none of those within one SearchInNeighbors / SearchAndFuse pass.  What they do
 * change is which points the reference skips, so the caller applies the results keyframe by keyframe in the reference's order and
 * re-tests the skip conditions immediately before applying each:
 *     eorb_fuse_keyframes(..., best_idx, best_dist, NULL);
 *     for k in the reference's keyframe order:
 *         for m in 0 .. M-1:
 *             if (vpMapPoints[m]->isBad() || vpMapPoints[m]->IsInKeyFrame(pKF_k)) continue;   // Sim3 overload: spAlreadyFound of pKF_k
 *             if (best_dist[k*M + m] <= TH_LOW) { Replace / AddObservation + AddMapPoint as at :1581-1600; nFused++; }
 * One input can change inside a pass: pMPinKF->Replace(pMP) ends in pMP->ComputeDistinctiveDescriptors() (src/MapPoint.cc:317), so a
 * shared point that absorbs another may come out with another descriptor.  So the caller also compares, before applying row
 * (k, m), the point's descriptor with the one it uploaded; where it changed, that row is stale and the caller searches the point in
 * pKF_k again with the new descriptor (eorb_fuse_pose, alone or grouped with the other changed points) and applies that result.
 * tests/test_kfside_ref.py runs this adapter against the sequential loop on a model map. */
int eorb_fuse_keyframes(eorb_ctx* ctx, const eorb_view* views, const eorb_grid_bounds* gb, int K,
                        const eorb_keypoint* kps, const uint8_t* desc, int stride, const float* uright, const int32_t* kf_off,
                        int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* q_desc,
                        const uint8_t* skip, const float* inv_sigma2, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reason);

/* ---- the same for mixed ORB + AKAZE keyframes: MixedMatcher on a MixedKeyFrame --------------------------------------------------------
 * MixedMatcher::Fuse(pKF, vpMapPoints, th, bRight) (src/MixedMatcher.cpp:1575-1797), Fuse(pKF, Scw, ...) (:1799-1933) and both
 * SearchByProjection(pKF, Scw, ...) (:1065-1189, :1191-1324) differ from the ORBmatcher forms above in four places, and in nothing else:
 *   tables   a map point with mp_is_orb[m] == 0 (!pMP->isORBMapPoint()) takes its level from the view's AKAZE pyramid (ak_nlevels,
 *            ak_log_scale: MapPoint::PredictScale(dist, pKF), src/MapPoint.cc:545-568) and radius = th * ak_scale_factors[level]
 *            (getAKAZEScaleFactor, :1684-1688); on a view with ak_nlevels == 0 it falls back to the ORB tables, as in
 *            eorb_project_frustum
 *   type     a candidate with kp_is_orb[idx] != mp_is_orb[m] is skipped (isORBMP != pKF->isORBDescValid(idx), :1707-1710)
 *   level    getKPtLevelMono(idx): octave of an ORB row, class_id of an AKAZE row (src/MixedFrame.cpp:438-446), in [level-1, level]
 *   sigma    the reprojection gate of the first Fuse overload multiplies by kp_inv_sigma2[idx] = pKF->getKPtInvLevelSigma2(idx)
 *            (:1732, :1743; the ORB table at octave for an ORB row, mvInvLevelSigma2AK[octave][layer of class_id] for an AKAZE row,
 *            src/MixedFrame.cpp:486-497): a float product compared with the double 5.99, or 7.8 where uright[idx] >= 0
 * kp_is_orb[n] / mp_is_orb[M]: 1 = ORB, NULL = all ORB on that side.  kp_inv_sigma2[n]: NULL = no reprojection gate (the Sim3
 * overload and SearchByProjection have none); NULL with uright given is EORB_E_ARG.  AKAZE rows are compared on the first 32 bytes of
 * their descriptor row at the caller's stride.  bRight, limits and error codes as the ORB forms.  With every flag NULL and
 * kp_inv_sigma2[i] = inv_sigma2[octave of i], each function returns what its ORB counterpart returns. */

/* eorb_kf_radius_match and eorb_kf_radius_match_stereo in one, with the type gate, the keypoint level and the per-keypoint sigma of
 * the MixedMatcher search loops (:1703-1758, :1891-1921, :1136-1170, :1266-1300).  uright[n] / q_ur[M] (both or neither): the stereo
 * gate; taken[n] / accept_thr (optional): the in-order form of SearchByProjection. */
int eorb_kf_radius_match_mixed(eorb_ctx* ctx,
        const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
        const uint8_t* kp_is_orb, const float* kp_inv_sigma2, const float* uright,
        int M, const uint8_t* valid, const float* uv, const float* radius, const int32_t* level, const uint8_t* q_desc,
        const uint8_t* mp_is_orb, const float* q_ur, uint8_t* taken, float accept_thr, int32_t* best_idx, int32_t* best_dist);

/* mode D with the tables picked per point (:1632-1688, :1837-1876, :1098-1134, :1226-1262): eorb_project_keyframe_side otherwise */
int eorb_project_keyframe_side_mixed(eorb_ctx* ctx, const eorb_view* view, int M, const float* pos, const float* normal, const float* min_dist,
                                     const float* max_dist, const uint8_t* mp_is_orb, const uint8_t* skip, float th, const eorb_kfside_out* out);

/* replaces MixedMatcher::Fuse(pKF, vpMapPoints, th, bRight) up to the map update (:1575-1758) and, with kp_inv_sigma2 == NULL,
 * MixedMatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:1799-1921): one upload, one wait, one download.  Returns exactly what
 * eorb_project_keyframe_side_mixed followed by eorb_kf_radius_match_mixed returns. */
int eorb_fuse_pose_mixed(eorb_ctx* ctx, const eorb_keypoint* kps, int n, const uint8_t* desc, int stride, const eorb_grid_bounds* gb,
                         const uint8_t* kp_is_orb, const float* kp_inv_sigma2, const float* uright,
                         const eorb_view* view, int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist,
                         const uint8_t* mp_is_orb, const uint8_t* skip, const uint8_t* q_desc, float th,
                         int32_t* best_idx, int32_t* best_dist, const eorb_kfside_out* out);

/* replaces both MixedMatcher::SearchByProjection(pKF, Scw, vpPoints, [vpPointsKFs,] vpMatched, th, ratioHamming) (:1065-1189,
 * :1191-1324) up to the assignment of vpMatched: eorb_search_by_projection_kf_scw with the tables, type gate and level above. */
int eorb_search_by_projection_kf_scw_mixed(eorb_ctx* ctx, const eorb_keypoint* kps, int n, const uint8_t* desc, int stride,
                                           const eorb_grid_bounds* gb, const uint8_t* kp_is_orb, const eorb_view* view, int M, const float* pos,
                                           const float* normal, const float* min_dist, const float* max_dist, const uint8_t* mp_is_orb,
                                           const uint8_t* skip, const uint8_t* q_desc, float th, uint8_t* taken, float accept_thr,
                                           int32_t* best_idx, int32_t* best_dist, const eorb_kfside_out* out);

/* MixedMatcher::Fuse of M shared map points into K MixedKeyFrames at once (LocalMapping::SearchInNeighbors, LoopClosing::SearchAndFuse):
 * eorb_fuse_keyframes with kp_is_orb / kp_inv_sigma2 concatenated like kps and one mp_is_orb[M] for all keyframes.  Every view must
 * name the same ORB pyramid and the same AKAZE pyramid (ak_nlevels, ak_log_scale; the tables are views[0]'s), otherwise EORB_E_ARG.
 * Entry k*M + m is what eorb_fuse_pose_mixed returns for keyframe k and point m.  The caller-side recipe above eorb_fuse_keyframes
 * (apply in the reference's keyframe order, re-test the skip conditions, search stale descriptors again) applies word for word. */
int eorb_fuse_keyframes_mixed(eorb_ctx* ctx, const eorb_view* views, const eorb_grid_bounds* gb, int K,
                              const eorb_keypoint* kps, const uint8_t* desc, int stride, const uint8_t* kp_is_orb, const float* kp_inv_sigma2,
                              const float* uright, const int32_t* kf_off,
                              int M, const float* pos, const float* normal, const float* min_dist, const float* max_dist, const uint8_t* mp_is_orb,
                              const uint8_t* q_desc, const uint8_t* skip, float th, int32_t* best_idx, int32_t* best_dist, uint8_t* reason);

/* ---- the node-walk matchers over K keyframes per call ----------------------------------------------------------------------------------
 * Three loops of the reference call a node-walk matcher once per keyframe of a list: LocalMapping::CreateNewMapPoints
 * (src/LocalMapping.cc:467-511; the same loop at src/Tracking.cc:3212-3215) runs SearchForTriangulation(mpCurrentKeyFrame, pKF2_k, ...)
 * over the neighbours, Tracking::Relocalization (src/Tracking.cc:2674-2689) SearchByBoW(pKF_k, CurrentFrame, ...) over the candidates,
 * LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:628-648) SearchByBoW(mpCurrentKF, vpCovKFi[j], ...) over a candidate and
 * its covisibles.  The four entry points below take the K keyframes of such a loop in one eorb_kf_set and return K rows; row k is what
 * the single entry point returns for pair k, bit for bit.  One upload (the shared side once), one wait, one download; three kernel
 * launches for any K.
 *
 * eorb_kf_set: keypoints, descriptors (one stride >= 32) and the flag byte of all keyframes concatenated, keyframe k = rows
 * kf_off[k] .. kf_off[k+1]-1 (the convention of eorb_fuse_keyframes and eorb_distinctive_descriptors).  flag = what the single form
 * takes per feature of that side: elig2 (SearchForTriangulation), kf_has_mp (eorb_search_by_bow), has_mp2 (eorb_search_by_bow_kf).
 * The K DBoW2 feature vectors are concatenated the same way: keyframe k owns node ids nodes[node_off[k] .. node_off[k+1]-1]
 * (ascending within the keyframe); its nn_k + 1 per-node offsets are feat_off[node_off[k] + k ..] (the first is 0, relative to the
 * keyframe), so feat_off holds node_off[K] + K entries; its feature indices (relative to the keyframe's first row) follow those of
 * keyframe k-1 in idx.  A keyframe with no rows or no nodes is legal: its row is all -1 and its count 0, the others are unaffected.
 * Every keyframe's feature vector is checked (offsets from 0 that never decrease, indices inside the keyframe's rows; eligible keypoints'
 * octaves where they index a table) and the message names k; the single entry points are these with K = 1 and have no checks of the
 * feature vectors of their own.  Limits, decided from the sizes before any array is
 * read: K <= 1024, K * n (n = the length of one output row) <= 2^22, then 2^22 rows in all; beyond them EORB_E_CAPACITY.  kf_off /
 * node_off that do not start at 0 or decrease: EORB_E_ARG. */
typedef struct eorb_kf_set {
    int K;
    const eorb_keypoint* kps; const uint8_t* desc; int stride; const uint8_t* flag; const int32_t* kf_off;
    const uint32_t* nodes; const int32_t* node_off; const int32_t* feat_off; const int32_t* idx;
} eorb_kf_set;

/* SearchForTriangulation(pKF1, pKF2_k, F12_k, ...) for the K neighbours in `set` (flag = elig2): pKF1 as in
 * eorb_search_for_triangulation; ep[2K] and F12[9K] per neighbour; one scale2 / sigma2_2[nlevels] table serves all keyframes (they
 * share one pyramid, as in eorb_fuse_keyframes); bCoarse and checkOri are shared.  match12[K*n1], nmatches[K] (optional).
 *
 * Why the batch is exact, and the caller's recipe for CreateNewMapPoints.  The reference never writes vbMatched2, so the result for a
 * pKF1 feature depends on that feature, pKF2_k and F12_k only; what changes between neighbours is which pKF1 features are eligible:
 * AddMapPoint(pMP, idx1) (src/LocalMapping.cc:775) takes idx1 out of the later neighbours' searches, pKF2->AddMapPoint (:776) touches
 * only that neighbour.  So the caller batches the neighbours that pass the baseline tests (:477-494), computes each F12_k, passes
 * elig1 as it stands before the loop, and hands the rows to the triangulation stage, which applies them in the reference's order
 * and resolves "set by an earlier neighbour of this pass" itself (eorb_new_map_points below; eorb_create_new_map_points is this
 * search and that stage in one call):
 *     eorb_create_new_map_points(..., match12, NULL, &params, &out);
 *     for k in the reference's neighbour order:
 *         for idx1 with out.status[k*n1 + idx1] == EORB_NP_NEW:
 *             new MapPoint(out.x3d + 3*(k*n1 + idx1)), observations, AddMapPoint(idx1), AddMapPoint(match12[k*n1 + idx1]) (:770-783)
 * This reproduces the sequential loop exactly while checkOri is false, and both callers construct the matcher that way
 * (src/LocalMapping.cc:443, src/Tracking.cc:3152).  With checkOri set a row equals the single call with the same elig1, which is not
 * the reference's sequence once elig1 has changed: the rotation histogram of a later neighbour would have been built without the
 * features taken meanwhile.  The reference may leave the loop early (CheckNewKeyFrames(), :469); the batch has then computed the
 * remaining rows for nothing.  tests/test_kfbatch_recipe.py runs this recipe against the sequential loop on a model map with a made-up
 * triangulation rule, tests/test_newpts_recipe.py with the real stage. */
int eorb_search_for_triangulation_keyframes(eorb_ctx* ctx,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_kf_set* set, const float* ep, const float* F12, const float* scale2, const float* sigma2_2, int nlevels,
        int bCoarse, int checkOri, int32_t* match12, int32_t* nmatches);

/* the same with the KannalaBrandt8 test of eorb_search_for_triangulation_kb8: Rt[12K] (monocular keyframes) or Rt[48K] (two-camera
 * keyframes: ll, lr, rl, rr per neighbour); cam1[2] / cam2[2] and the level tables are shared; nleft1 once, nleft2[K] per neighbour,
 * all -1 or all >= 0 like nleft1 (EORB_E_CONFIG otherwise, as every EORB_E_CONFIG rule of the single form).  A Pinhole pCamera2 is
 * allowed.  The recipe above applies word for word. */
int eorb_search_for_triangulation_kb8_keyframes(eorb_ctx* ctx,
        const eorb_keypoint* kps1, int n1, int nleft1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_kf_set* set, const int32_t* nleft2,
        const eorb_camera* cam1, const eorb_camera* cam2, const float* Rt, const float* ep,
        const float* scale2, const float* sigma2_1, const float* sigma2_2, int nlevels,
        int bCoarse, int checkOri, int32_t* match12, int32_t* nmatches);

/* ---- CreateNewMapPoints on the device: triangulation and its checks -----------------------------------------------------------
 * replaces the per-match half of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:527-784) and of its copy
 * Tracking::CreateNewMapPoints (src/Tracking.cc:3232-3408) for the K neighbours of one keyframe: per pair (idx1, idx2 =
 * match12[k*n1 + idx1]) the type gate (:542), the pose / camera choice (:563-628), unprojectMat and the ray parallax (:631-636), the
 * stereo parallax (:642-647), linear triangulation through cv::SVD::compute or UnprojectStereo (:650-683; src/KeyFrame.cc:924-940),
 * the two depth signs (:689-695), the two chi-square reprojection gates (:698-748), the far-point test (:760) and the scale
 * consistency test (:763-767), in the reference's operation order on OpenCV 3.4.1's scalar paths ("Parity
 * choices of CreateNewMapPoints").  The two sequential rules of the loop are resolved in the call:
 *   the claim: AddMapPoint(pMP, idx1) (:775) takes idx1 out of the later neighbours, so the pair that counts for idx1 is the first k,
 *     in neighbour order, whose pair is accepted; its later matches get EORB_NP_CLAIMED.  Two idx1 on one idx2 of a neighbour are both
 *     reported (the reference creates both points and pKF2->AddMapPoint overwrites; that stays with the caller);
 *   ratioFactor (:464): overwritten with the AKAZE factor at the first AKAZE-AKAZE pair the loop reaches (:545-546) and never set back;
 *     pairs are visited k-major, idx1 ascending (src/ORBmatcher.cc:1206-1211), a claimed idx1 is not visited.
 * After the call the caller still does, per EORB_NP_NEW entry in the reference's order: new MapPoint(x3d), the two AddObservation,
 * the two AddMapPoint, ComputeDistinctiveDescriptors (eorb_distinctive_descriptors), UpdateNormalAndDepth, Atlas::AddMapPoint.
 * The baseline tests that leave a neighbour out (:477-494) stay with the caller, as in eorb_search_for_triangulation_keyframes.
 * EvLocalMapping's variants are not covered. */
#define EORB_NEWPTS_LOCAL_MAPPING 0   /* src/LocalMapping.cc:527-784 */
#define EORB_NEWPTS_TRACKING      1   /* src/Tracking.cc:3232-3408: xn = ((u-cx)*invfx, (v-cy)*invfy, 1), fx*x*invz+cx in the non-stereo
                                         gate too, no two-camera branch, no far-point test, bStereo = uRight >= 0 */
/* status, one value per exit of the loop body */
#define EORB_NP_NEW           0   /* triangulation is successful (:769) */
#define EORB_NP_NO_MATCH      1   /* match12 < 0 */
#define EORB_NP_CLAIMED       2   /* idx1 got its map point from an earlier neighbour of this call (:775) */
#define EORB_NP_TYPE          3   /* isORBKPt1 != isORBKPt2 (:542) */
#define EORB_NP_PARALLAX      4   /* no stereo and very low parallax (:680-683) */
#define EORB_NP_W_ZERO        5   /* x3D.at<float>(3) == 0 (:665) */
#define EORB_NP_EMPTY_STEREO  6   /* UnprojectStereo returned an empty Mat: depth <= 0 (:687; Tracking.cc would fault there) */
#define EORB_NP_Z1            7   /* z1 <= 0 (:690) */
#define EORB_NP_Z2            8   /* z2 <= 0 (:694) */
#define EORB_NP_REPROJ1       9   /* chi-square gate in keyframe 1 (:709, :721) */
#define EORB_NP_REPROJ2      10   /* chi-square gate in keyframe 2 (:735, :746) */
#define EORB_NP_ZERO_DIST    11   /* dist1 == 0 || dist2 == 0 (:757) */
#define EORB_NP_FAR          12   /* mbFarPoints && (dist1 >= mThFarPoints || dist2 >= mThFarPoints) (:760) */
#define EORB_NP_SCALE        13   /* ratioDist*ratioFactor < ratioOctave || ratioDist > ratioOctave*ratioFactor (:766) */
#define EORB_NP_NONFINITE    14   /* x3D, z, the reprojection error or a distance is not finite: this library's rule, as reason 7 of
                                     eorb_project_frustum (the reference goes on with a NaN there: every comparison is false) */
/* branch (test aid): how x3D was formed */
#define EORB_NP_BRANCH_NONE    0
#define EORB_NP_BRANCH_DLT     1
#define EORB_NP_BRANCH_STEREO1 2
#define EORB_NP_BRANCH_STEREO2 3

/* per-keypoint arrays of one side: pKF1 (n1 entries) or the K neighbours concatenated like their keypoints (kf_off) */
typedef struct eorb_newpts_side {
    const float*   kp_sigma2;   /* getKPtLevelSigma2(i); NULL: level_sigma2[octave] (the convention of kp_inv_sigma2 in the mixed forms) */
    const float*   kp_scale;    /* getKPtScaleFactor(i); NULL: level_scale[octave] */
    const uint8_t* kp_is_orb;   /* isORBDescValid(i); NULL: all ORB */
    const float*   uright;      /* mvuRight; NULL: no rectified right image (bStereo false) */
    const float*   depth;       /* mvDepth; NULL with uright given is EORB_E_ARG; finite wherever uright >= 0 */
    const float*   raw_xy;      /* mvKeys[i].pt, 2 per keypoint: what UnprojectStereo reads (KeyFrame.cc:929-930); NULL: the same as kps */
} eorb_newpts_side;

/* views1: pKF1's eorb_view (R, t, Ow, cam and mbf are read), two of them (left, right as eorb_view documents) when nleft1 >= 0;
 * views2: one per neighbour, or two per neighbour (2k, 2k+1) when nleft1 >= 0.  nleft1 / nleft2[K] = numAllKPtsLeft() as in
 * eorb_search_for_triangulation_kb8 (nleft2 NULL = all -1); one side with two cameras and the other with one: EORB_E_CONFIG.  With two
 * cameras kps = the distorted left keypoints then the right ones, otherwise the undistorted ones (:548-557).  mpCamera2 != NULL is
 * taken to be nleft >= 0.  fx, fy, cx, cy of the stereo gates and of UnprojectStereo are views[0].cam's, invfx = 1.0f/fx.
 * mb1 / mb2[K] = KeyFrame::mb (finite, >= 0; mb2 NULL = 0).  The form EORB_NEWPTS_TRACKING takes nleft1 = -1 only. */
typedef struct eorb_newpts_params {
    int form;
    const eorb_view* views1; int nleft1; float mb1;
    const eorb_view* views2; const int32_t* nleft2; const float* mb2;
    eorb_newpts_side side1, side2;
    const float* level_scale; const float* level_sigma2; int nlevels;   /* read where kp_scale / kp_sigma2 is NULL */
    float ratio_factor_orb, ratio_factor_ak;   /* 1.5f*getORBScaleFactor(), 1.5f*getAKAZEScaleFactor() */
    int far_points; float th_far_points;       /* mbFarPoints, mThFarPoints */
} eorb_newpts_params;

/* dense like eorb_fuse_keyframes: entry k*n1 + idx1.  status and n_new[K] are required; x3d (3 per entry: the new point, zero unless
 * status is EORB_NP_NEW), branch and cos_parallax (test aids: zero where the loop did not get that far) may be NULL */
typedef struct eorb_newpts_out { uint8_t* status; float* x3d; uint8_t* branch; float* cos_parallax; int32_t* n_new; } eorb_newpts_out;

/* the stage alone: match12[K*n1] from the host (what eorb_search_for_triangulation_keyframes returned), kps2 / kf_off[K + 1] the
 * neighbours' keypoints concatenated as in eorb_kf_set.  A match12 entry outside [-1, rows of keyframe k): EORB_E_ARG.  Limits as the
 * K-keyframe search: K <= 1024, K*n1 <= 2^22, 2^22 rows in all (EORB_E_CAPACITY).  Camera models other than 0 / 1: EORB_E_CONFIG.
 * K == 0 and an all -1 match12: EORB_OK.  One upload, one wait, one download; two launches. */
int eorb_new_map_points(eorb_ctx* ctx, const eorb_keypoint* kps1, int n1, const eorb_keypoint* kps2, const int32_t* kf_off, int K,
                        const int32_t* match12, const eorb_newpts_params* params, const eorb_newpts_out* out);

/* eorb_search_for_triangulation_keyframes followed by the stage: match12 stays on the device between the two halves; one upload,
 * one wait, one download.  Returns exactly what the two calls in sequence return, match12 / nmatches included.  The arguments of both
 * halves are checked before anything runs; the stage reads kps1 and set->kps. */
int eorb_create_new_map_points(eorb_ctx* ctx,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_kf_set* set, const float* ep, const float* F12, const float* scale2, const float* sigma2_2, int nlevels,
        int bCoarse, int checkOri, int32_t* match12, int32_t* nmatches,
        const eorb_newpts_params* params, const eorb_newpts_out* out);

/* the same over eorb_search_for_triangulation_kb8_keyframes; nleft1 / nleft2 are the search's, params->nleft1 / nleft2 must agree */
int eorb_create_new_map_points_kb8(eorb_ctx* ctx,
        const eorb_keypoint* kps1, int n1, int nleft1, const uint8_t* desc1, int stride1, const uint8_t* elig1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_kf_set* set, const int32_t* nleft2,
        const eorb_camera* cam1, const eorb_camera* cam2, const float* Rt, const float* ep,
        const float* scale2, const float* sigma2_1, const float* sigma2_2, int nlevels,
        int bCoarse, int checkOri, int32_t* match12, int32_t* nmatches,
        const eorb_newpts_params* params, const eorb_newpts_out* out);

/* SearchByBoW(pKF_k, F, vvpMapPointMatches[k]) for the K candidates in `set` (the pKF side; flag = kf_has_mp) against one frame
 * (f_desc n_f x 32): Tracking::Relocalization.  match_f[K*n_f] = KeyFrame feature index relative to keyframe k, or -1; nmatches[K]
 * (optional).  Exact without a recipe: each k writes a fresh vector and the K searches share no state.  isBad() keyframes are left
 * out by the caller (:2677).  The first 32 bytes of each descriptor row of the set are read. */
int eorb_search_by_bow_keyframes(eorb_ctx* ctx, const eorb_kf_set* set,
        const eorb_keypoint* f_kps, int n_f, const uint8_t* f_desc,
        const uint32_t* f_nodes, const int32_t* f_node_off, const int32_t* f_idx, int f_nn,
        int32_t* match_f, float nnratio, int checkOri, int32_t* nmatches);

/* SearchByBoW(pKF1, pKF2_k, vvpMatchedMPs[k]) for the K keyframes in `set` (side 2; flag = has_mp2, required) against one keyframe
 * (side 1, desc1 n1 x 32): LoopClosing::DetectCommonRegionsFromBoW.  match12[K*n1] = index in keyframe k, or -1; nmatches[K]
 * (optional).  Exact without a recipe, as above; isBad() keyframes are left out by the caller. */
int eorb_search_by_bow_kf_keyframes(eorb_ctx* ctx,
        const eorb_keypoint* kps1, int n1, const uint8_t* desc1, const uint8_t* has_mp1,
        const uint32_t* nodes1, const int32_t* node_off1, const int32_t* idx1, int nn1,
        const eorb_kf_set* set, int32_t* match12, float nnratio, int checkOri, int32_t* nmatches);

/* replaces MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:349-423; f3), batched over M map points: the
 * descriptors observed for map point m are rows offsets[m] .. offsets[m+1]-1 of desc (n x 32); best[m] = the row (relative
 * to offsets[m]) with the least median Hamming distance to the others, -1 when there is none.  At most 65 535 rows per map point
 * (EORB_E_CAPACITY beyond, decided from the offsets before desc is read); offsets[0] >= 0 (EORB_E_ARG). */
int eorb_distinctive_descriptors(eorb_ctx* ctx, const uint8_t* desc, const int32_t* offsets, int M, int32_t* best);

/* ---- KLT tracker ----------------------------------------------------------------------------------
 * replaces cv::calcOpticalFlowPyrLK(mRefFrame, currImage, mRefPoints, kpts, status, err, Size(mPatchSz, mPatchSz), mMaxLevel,
 * mLKCriteria, flags) inside ELK_Tracker::trackCurrImage (src/Event/KLT_Tracker.cpp:49-98; Event.klt.* of
 * Examples/Event/EvETHZ.yaml:205-208: winSize 23, maxLevel 1, maxIter 10, eps 0.03).  8-bit single-channel images.
 * TermCriteria(COUNT + EPS, maxCount, epsilon); flags: 4 = OPTFLOW_USE_INITIAL_FLOW (next_pts holds the initial guess),
 * 8 = OPTFLOW_LK_GET_MIN_EIGENVALS; minEigThreshold = 1e-4 is OpenCV's default.  next_pts (n x 2) in/out, status / err (n) out.
 * The match bookkeeping around it (refineTrackedPts :104-151, refineFirstOctaveLevel :153-205) is host logic and stays in the
 * adapter. */
int eorb_calc_optical_flow_pyr_lk(eorb_ctx* ctx, const uint8_t* prev, const uint8_t* next, int W, int H, int stride,
                                  const float* prev_pts, float* next_pts, int n, int win, int maxLevel, int maxCount, double epsilon,
                                  int flags, float minEigThreshold, uint8_t* status, float* err);

/* ---- DBoW2 vocabulary transform: the producer of the feature vectors SearchByBoW consumes ----------
 * The vocabulary tree (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h: m_nodes after loadFromTextFile :1338-1430) flattened:
 * node 0 = root; children of node i = child_ids[child_off[i] .. child_off[i+1]) in `children` order; a node without children
 * is a word (Node::isLeaf) with word_id / weight; node_desc = nnodes x 32 bytes (FORB).  Copied to the device once. */
int eorb_bow_set_vocabulary(eorb_ctx* ctx, int nnodes, int L, const int32_t* child_off, const int32_t* child_ids,
                            const uint8_t* node_desc, const int32_t* word_id, const double* weight);

/* replaces ORBVocabulary::transform(vCurrentDesc, mBowVec, mFeatVec, levelsup) as called by Frame::ComputeBoW
 * (src/Frame.cc: levelsup = 4) = TemplatedVocabulary::transform :1125-1190 + the per-feature descent :1208-1250 with
 * FORB::distance (FORB.cpp:81-101).  weighting: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY (WeightingType); norm: 0 none, 1 L1, 2 L2 =
 * ScoringObject::mustNormalize of the vocabulary's scoring type (ORBvoc.txt: TF_IDF + L1_NORM -> 0, 1).
 * BowVector out: ascending (bow_word, bow_val)[*n_words]; FeatureVector out: CSR (fv_node ascending, fv_off[*n_fvnodes + 1],
 * fv_idx in push_back order) -- the layout eorb_search_by_bow takes.  Output arrays sized n (fv_off n + 1).
 * word_of / node_of (n, may be NULL): word and nid-level node of every feature, -1 for stopped words.
 * A feature whose descent ends on a leaf above level L - levelsup has node 0 (the reference leaves nid unset there, :1151, :1251), as
 * has every feature when L - levelsup <= 0 (:1227).
 * Limit, decided from n before any array is read or written: EORB_BOW_MAX_FEATURES features per call (one workgroup sorts them in
 * LDS), EORB_E_CAPACITY beyond; the monocular initialiser's 5 x nFeatures frames (Tracking.cc:4216, :1482-1483) fit up to
 * nFeatures = 1638.  A BowVector of more than EORB_KFDB_MAX_QUERY_WORDS words is refused by the KeyFrameDatabase queries. */
#define EORB_BOW_MAX_FEATURES  8192
int eorb_bow_transform(eorb_ctx* ctx, const uint8_t* desc, int n, int stride, int levelsup, int weighting, int norm,
                       uint32_t* bow_word, double* bow_val, int* n_words, uint32_t* fv_node, int32_t* fv_off, int32_t* fv_idx,
                       int* n_fvnodes, int32_t* word_of, int32_t* node_of);

/* ---- KeyFrameDatabase: the place-recognition queries (src/KeyFrameDatabase.cc) -------------------------------------------------
 * The consumer of eorb_bow_transform's BowVector and the producer of the keyframe lists eorb_search_by_bow_keyframes /
 * eorb_search_by_bow_kf_keyframes take.  The database belongs to the context and lives on the device.  There is no inverted file:
 * add() (:39-45) appends a keyframe to the list of each of its words in one call, so every list holds its keyframes in the order of
 * their latest add; the database keeps each live keyframe's BowVector (word ids strictly ascending, double values) and an add
 * sequence number, and lKFsSharingWords (first-encounter order of the walk at :791-806 / :624-653) is the listed keyframes ordered by
 * (smallest word shared with the query, add sequence).  Keyframes are named by slots: eorb_kfdb_add returns them, the lowest free slot
 * first, so the slot of an erased keyframe is reused.  What stays with the caller (pointers and mutexes): the slot <-> KeyFrame* table,
 * the map test (GetMap), isBad(), the already-added set and the nNumCandidates cut (eorb_slam_amd/host/eorb_host.hpp performs them).
 *
 * Stored scores: one float per slot and query family, EORB_KFDB_RELOC = mRelocScore, EORB_KFDB_PLACE = mPlaceRecognitionScore.  A query
 * writes it for every keyframe it scores; the covisibility accumulation (:846-871 / :693-718) adds the stored score of every LISTED
 * neighbour, which is the one an earlier query left when the neighbour shares a word but is under the threshold this time -- as the
 * reference does.  Both are 0 at add (the reference initialises mPlaceRecognitionScore to 0 and leaves mRelocScore uninitialised:
 * here both are defined as 0).
 *
 * Limits, decided from the sizes before any array is read: EORB_KFDB_MAX_SLOTS slots; EORB_KFDB_MAX_QUERY_WORDS words in a query (its
 * word ids are staged in LDS); fewer than 2^30 words in the live vectors and 2^32 adds since the last clear; beyond them EORB_E_CAPACITY.  Values must be finite. */
#define EORB_KFDB_MAX_SLOTS        65536
#define EORB_KFDB_MAX_QUERY_WORDS  4096
#define EORB_KFDB_COVIS            10      /* GetBestCovisibilityKeyFrames(10) */
#define EORB_KFDB_RELOC            0
#define EORB_KFDB_PLACE            1

/* clear() :68-72: empties the database; the next slot returned is 0 again */
int eorb_kfdb_clear(eorb_ctx* ctx);

/* add(pKF) :39-45 for K keyframes in order (K = 1: one add; K > 1: PostLoad, tests): keyframe k's BowVector is (word, val)[off[k] ..
 * off[k + 1]), off[0] = 0; a vector without words is legal.  Word ids that do not ascend strictly: EORB_E_ARG, naming k; nothing is
 * added then.  slots_out[k]: the slot of keyframe k.  Only the new vectors are uploaded; a pool that has to grow is copied on the device. */
int eorb_kfdb_add(eorb_ctx* ctx, int K, const int32_t* off, const uint32_t* word, const double* val, int32_t* slots_out);

/* erase(pKF) :47-66.  A slot that holds no keyframe: EORB_E_ARG. */
int eorb_kfdb_erase(eorb_ctx* ctx, int slot);

/* *n_live keyframes in the database; *n_slots = one more than the highest slot returned since the last clear (the length of the per-slot
 * arrays below) */
int eorb_kfdb_info(eorb_ctx* ctx, int* n_live, int* n_slots);

/* the stored scores of one family (EORB_KFDB_RELOC / EORB_KFDB_PLACE), n_slots floats; free slots read 0 or what their last keyframe left */
int eorb_kfdb_get_scores(eorb_ctx* ctx, int family, float* scores);

/* DetectRelocalizationCandidates(F, pMap) :783-895 for the query BowVector (word, val)[n_words] (F->mBowVec, ascending).
 * covis: n_slots * EORB_KFDB_COVIS slot ids, row s = GetBestCovisibilityKeyFrames(10) of slot s in their order, -1 = none / not in the
 * database (ids outside [0, n_slots) and free slots count as none); NULL: no accumulation, only the scored list is returned.
 * Outputs, cap entries each, in lScoreAndMatch order (:826-837: listed keyframes with words > minCommonWords, minCommonWords =
 * (int)(maxCommonWords * 0.8f), :819): slot, si (L1Scoring::score as a float, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68: the sum over
 * the common words in ascending word order in double, -score / 2.0; the sign of a -0.0 is kept), words (mnRelocWords); with covis also acc
 * (accScore), best_slot (pBestKF) and keep (1: accScore > 0.75f * bestAccScore, :873-882).  *n_listed = lKFsSharingWords.size(),
 * *n_scored = lScoreAndMatch.size(), *max_common_words, *best_acc (0 without covis).  *n_scored > cap: EORB_E_CAPACITY with the needed
 * count in *n_scored (the family's stored scores are this query's all the same).  Nothing listed: zero counts, EORB_OK. */
int eorb_kfdb_detect_reloc(eorb_ctx* ctx, int n_words, const uint32_t* word, const double* val, const int32_t* covis, int cap,
                           int32_t* slot, float* si, int32_t* words, float* acc, int32_t* best_slot, uint8_t* keep,
                           int* n_listed, int* n_scored, int* max_common_words, float* best_acc);

/* DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, n) :612-780 for pKF->mBowVec.  exclude: n_slots bytes, non-zero = the keyframe is in
 * spConnectedKF: never listed, and never counted as a covisible neighbour (its query id is not set, :635-645); NULL = none.  The scored
 * list and acc / best_slot as above; sorted_acc / sorted_best_slot: lAccScoreAndMatch after sort(compFirst) (:606-609, :722), a stable sort
 * by descending accScore -- what the loop at :731-752 walks. */
int eorb_kfdb_detect_nbest(eorb_ctx* ctx, int n_words, const uint32_t* word, const double* val, const uint8_t* exclude, const int32_t* covis,
                           int cap, int32_t* slot, float* si, int32_t* words, float* acc, int32_t* best_slot, float* sorted_acc,
                           int32_t* sorted_best_slot, int* n_listed, int* n_scored, int* max_common_words, float* best_acc);

/* The loop body every windowed matcher of src/ORBmatcher.cc shares (e.g. :754-774, :95-130, :2050-2070): for query q the
 * candidates cand_idx[cand_offsets[q] .. cand_offsets[q+1]) (what GetFeaturesInArea returned, after the caller's gates) are
 * visited in order with `if (d < best) {second = best; best = d} else if (d < second) second = d` on the first 32 descriptor
 * bytes.  For adapters that keep the greedy bookkeeping on the host.  Absent: index -1, distance 256. */
int eorb_hamming_window_match(eorb_ctx* ctx, const uint8_t* q_desc, int nq, int q_stride, const uint8_t* t_desc, int nt, int t_stride,
                              const int32_t* cand_offsets, const int32_t* cand_idx, int32_t* best_idx, int32_t* best_d,
                              int32_t* second_idx, int32_t* second_d);

/* replaces MixedFrame::sortFeaturesResponse (src/MixedFrame.cpp:211-225): perm[k] = index of the k-th keypoint in
 * descending-response order, equal responses in insertion order (std::multimap semantics). */
int eorb_sort_by_response(eorb_ctx* ctx, const eorb_keypoint* kps, int n, int32_t* perm);
/* MixedFrame::resolveNumMixedPts (src/MixedFrame.cpp:281-317): how many ORB / AKAZE features the mixed frame keeps */
void eorb_resolve_num_mixed(int nDetectedORB, int nDetectedAK, int nDesired, int nDesiredAK, int* nORB, int* nAK);

/* replaces cv::BFMatcher(NORM_HAMMING)::knnMatch(q, t, matches, 2) at src/Frame.cc:1228
 * (+ the ORBmatcher::DescriptorDistance core, ORBmatcher.cc:2360-2378).  idx2/dist2: nq*2. */
int eorb_hamming_bf_knn2(eorb_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt,
                         int32_t* idx2, int32_t* dist2);

/* ---- batched, HBM-resident front end (throughput path) ------------------------------------------- */
typedef struct {
    int   W, H;
    float sigma;            /* Event.image.l1Sigma */
    int   pol;
    eorb_orb_params orb;
    int   lap0, lap1;       /* vLappingArea (mono: 0, 1000) */
    int   want_desc;
    int   max_batch;        /* slices per batch */
    int   max_events;       /* events per slice (capacity) */
    int   match;            /* 1: SearchForInitialization of slice b against slice b-1 */
    int   windowSize;       /* 100 */
    float nnratio;          /* 0.9 */
    int   checkOri;
} eorb_fe_config;

int eorb_fe_configure(eorb_ctx* ctx, const eorb_fe_config* cfg);

/* One pass of the hot path over a batch of B time-slices, everything resident in HBM:
 *   accumulate (ev2im_gauss, normalised u8) -> ORB extract -> match slice b against slice b-1
 *   (slice 0 against `prev` state carried in the ctx from the previous batch, if any).
 * d_events: all slices' events back to back; h_offsets[B+1]: slice boundaries (host array).
 * Outputs (device pointers, any may be NULL): d_images u8 B*W*H; d_kps B*cap; d_desc B*cap*32;
 * d_nkps int32 B; d_matches12 int32 B*cap (for slice b: index into slice b, per keypoint of b-1);
 * d_nmatches int32 B.  cap = eorb_orb_max_keypoints(). */
/* as eorb_fe_run_batch_dev, for raw sensor events resident in HBM (eorb_set_undistort_maps first) */
int eorb_fe_run_batch_raw_dev(eorb_ctx* ctx, const eorb_raw_event* d_events, const int64_t* h_offsets, int B,
                              uint8_t* d_images, eorb_keypoint* d_kps, uint8_t* d_desc, int32_t* d_nkps,
                              int32_t* d_matches12, int32_t* d_nmatches);

/* as eorb_fe_run_batch_raw_dev, for 4-byte sensor records (eorb_raw_event4) resident in HBM */
int eorb_fe_run_batch_raw4_dev(eorb_ctx* ctx, const eorb_raw_event4* d_events, const int64_t* h_offsets, int B,
                               uint8_t* d_images, eorb_keypoint* d_kps, uint8_t* d_desc, int32_t* d_nkps,
                               int32_t* d_matches12, int32_t* d_nmatches);

/* as eorb_fe_run_batch_raw_dev, for 2-byte sensor records (eorb_raw_event2) resident in HBM: polarity-free images on sensors of at
 * most 65 535 pixels (a DAVIS 240x180 has 43 200) never read more of an event than its pixel */
int eorb_fe_run_batch_raw2_dev(eorb_ctx* ctx, const eorb_raw_event2* d_events, const int64_t* h_offsets, int B,
                               uint8_t* d_images, eorb_keypoint* d_kps, uint8_t* d_desc, int32_t* d_nkps,
                               int32_t* d_matches12, int32_t* d_nmatches);

/* (float events: a call with 2^20 events or more waits for the stream once, to learn how many distinct positions its events take --
 * the raw variant above never waits) */
int eorb_fe_run_batch_dev(eorb_ctx* ctx, const eorb_event16* d_events, const int64_t* h_offsets, int B,
                          uint8_t* d_images, eorb_keypoint* d_kps, uint8_t* d_desc, int32_t* d_nkps,
                          int32_t* d_matches12, int32_t* d_nmatches);

/* ---- the L1 image builder's per-chunk path, one call per chunk ----------------------------------------------------------------
 * EvImBuilder::Track (src/Event/EvImBuilder.cpp:1300-1515) makes, per chunk of l1ChunkSize events, the event image (:1345) and a frame
 * from it (:1348); the frame of an INIT chunk runs the detect-only ORBextractor (EvBaseTracker::makeFrame -> EvFrame ctor,
 * src/Event/EventFrame.cpp:199-247) and becomes the reference of the LK tracker (init :568-592 -> ELK_Tracker::setRefImage), the frame
 * of a TRACKING chunk tracks the reference points into the new image (makeFrame :528-548 -> ELK_Tracker::trackAndMatchCurrImage,
 * src/Event/KLT_Tracker.cpp:215-234).  Through eorb_ev2im_gauss + eorb_orb_extract / eorb_calc_optical_flow_pyr_lk that is two or three
 * host-buffer calls, each with its own upload, wait and download, and the image crosses the link three times; the calls below take the
 * chunk's events and hand back keypoints / tracked points with ONE upload, ONE wait and ONE download.  The u8 image stays on the device
 * (out_u8 != NULL downloads it with the results; eorb_ev_slice_image fetches it later, until the next call on the context).
 * Events: `ev` (the reference's float EventData) or `raw` (sensor events resolved through eorb_set_undistort_maps), not both.
 * The image size is the extractor's (eorb_orb_configure). */
typedef struct eorb_klt_params {      /* Event.klt.* of Examples/Event/EvETHZ.yaml:205-208 -> ELK_Tracker (KLT_Tracker.cpp:14-20) */
    int    win;                       /* kltWinSize (23) */
    int    maxLevel;                  /* maxLevel (1) */
    int    maxCount;                  /* kltMaxItr (10) */
    double epsilon;                   /* kltEps (0.03) */
    float  minEigThreshold;           /* cv::calcOpticalFlowPyrLK's default 1e-4 */
} eorb_klt_params;

/* INIT chunk: ev2im_gauss(events, W, H, sigma) -> ORBextractor::operator() (both overloads: want_desc) -> the image and its keypoints
 * become the LK reference kept on the device.  Outputs as eorb_orb_extract. */
int eorb_ev_slice_extract(eorb_ctx* ctx, const eorb_event* ev, const eorb_raw_event* raw, size_t n, float sigma, int lap0, int lap1,
                          int want_desc, eorb_keypoint* kps, uint8_t* desc, uint8_t* oob, int cap, int* n_out, int* mono_index,
                          uint8_t* out_u8);

/* TRACKING chunk: ev2im_gauss(events) -> cv::calcOpticalFlowPyrLK(reference image, image, reference points, pts, status, err, win,
 * maxLevel, criteria, OPTFLOW_USE_INITIAL_FLOW) (ELK_Tracker::trackCurrImage, KLT_Tracker.cpp:49-74).  pts[2 * nref]: in = the last
 * tracked points (mLastTrackedPts: the reference points on the first tracking chunk), out = the tracked points; nref = the number of
 * keypoints the last eorb_ev_slice_extract returned.  The reference frame's pyramid and derivatives are built once per reference. */
int eorb_ev_slice_track(eorb_ctx* ctx, const eorb_event* ev, const eorb_raw_event* raw, size_t n, float sigma, const eorb_klt_params* klt,
                        float* pts, uint8_t* status, float* err, int nref, uint8_t* out_u8);

/* the u8 image of the context's last eorb_ev_slice_extract / _track call (W x H of the extractor), while no other host-buffer call
 * has run on the context since: the adapter's lazy download behind the cv::Mat seam */
int eorb_ev_slice_image(eorb_ctx* ctx, uint8_t* out_u8);

/* The reconstruction contest of a dispatch, EvImBuilder::generateMCImage (src/Event/EvImBuilder.cpp:1146-1247), in one call: for the
 * accumulated window `ev` (float EventData with their time stamps) the reconstructions
 *   0 "DP"  ev2mci_gg_f(evs, camera, Tcw, medDepth)     getDPoseMCI :958-979    present when dp != NULL
 *   1 "BA"  the same with the BA pose                   getBAMCI :1033-1058     present when ba != NULL
 *   2 "EH"  ev2im_gauss(evs, normalized = false)        getEvHist :1060-1079    always
 *   3 "Opt" ev2mci_gg_f(evs, camera, paramsSE2)         getAff2DMCI :1124-1143  present when se2_params != NULL
 * each with measureImageFocus and cv::normalize(img, img, 255, 0, NORM_MINMAX, CV_8UC1); the winner is the largest focus, the first
 * of equals in that order (MciInfo = std::multimap<float, PoseImagePtr, std::greater<float>>, include/Utils/Visualization.h:29); a
 * winning "EH" is replaced by the histogram of the later half of the window (:1214-1216).  The poses come from the optimisers (out of
 * this library's scope): AngleAxisd(R) of Tcw's rotation, its translation and the median depth, exactly what eorb_ev2mci_se3 takes.
 * focus[0..3] = the methods' focus (-1: absent), focus[4] = the later-half histogram's; *winner = the winning method; out_u8
 * (optional) = the winner's image; with `l2` (a context on the same device whose extractor is the L2 tracker's; the contexts belong to
 * the calling thread) the winner goes through its detect-only extraction (isMcImageGood :260-267 = the L2 frame): kps / cap / n_out.
 * No events: returns with *winner = -1 (:1149-1152). */
typedef struct eorb_se3_motion { double angle; double axis[3]; double t[3]; float medDepth; } eorb_se3_motion;
int eorb_ev_mc_contest(eorb_ctx* ctx, const eorb_event* ev, size_t n, const eorb_camera* cam, const eorb_se3_motion* dp,
                       const eorb_se3_motion* ba, const float* se2_params, int nparams, int W, int H, float sigma, float focus[5],
                       int* winner, uint8_t* out_u8, eorb_ctx* l2, int lap0, int lap1, eorb_keypoint* kps, int cap, int* n_out);

/* The float images of the context's last eorb_fe_run_batch_*_dev call (what ev2im_gauss(..., normalized = false) returns,
 * src/Event/EventConversion.cc:264-268: the CV_32FC1 sums before normaliseImage): *d_f32 = device pointer to B x H x W floats, valid
 * until the next batch call on the context; h_minmax (optional, 2 * B floats: min, max per slice = the running extremes of
 * resolveMinMaxVals :32-39) is downloaded, which waits for the stream.  For callers that want the un-normalised image of a slice
 * (EvImBuilder::getEvHist, src/Event/EvImBuilder.cpp:1060-1079) and for bit-level verification of a batch. */
int eorb_fe_last_f32_dev(eorb_ctx* ctx, const float** d_f32, float* h_minmax, int B);

/* the same pass for B camera frames resident in HBM (u8, W x H each, back to back; the image side of the front end,
 * Frame::ExtractORB src/Frame.cc:467-482 + SearchForInitialization of frame b against frame b-1): no accumulation, the frames
 * are only read.  eorb_fe_configure as above (sigma / pol / max_events unused). */
int eorb_fe_run_batch_images_dev(eorb_ctx* ctx, const uint8_t* d_images, int B, eorb_keypoint* d_kps, uint8_t* d_desc,
                                 int32_t* d_nkps, int32_t* d_matches12, int32_t* d_nmatches);

/* self-check used by tests: number of floats v in [lo, hi] (0 < lo <= hi) for which the reciprocal+fma quotient the
 * accumulation kernel uses for v / (2*pi*sigma^2) differs from the IEEE-754 quotient (must be 0). */
int eorb_selfcheck_division(eorb_ctx* ctx, float lo, float hi, float sigma, uint64_t* mismatches);

/* self-check used by tests: order-independent 64-bit hash of a device math function over every float whose bit pattern
 * lies in [lo_bits, hi_bits]: which = 0 exp(-x) as used by exp_XY2f, 1 sin(x), 2 cos(x) as used by computeOrbDescriptor,
 * 3 tan(x), 4 atan(x), 5 atan2 over generated pairs (KannalaBrandt8), 6 log(x) as used by MapPoint::PredictScale.
 * The CPU oracle computes the same hash of its own functions: equality proves the two agree on every input. */
int eorb_selfcheck_math(eorb_ctx* ctx, int which, uint32_t lo_bits, uint32_t hi_bits, uint64_t* hash);

/* helpers: convert host AoS events to the compact record; device alloc/copy without a HIP binding */
void  eorb_pack_events(const eorb_event* ev, size_t n, eorb_event16* out);
void* eorb_dev_alloc(eorb_ctx* ctx, size_t bytes);
int   eorb_dev_free(eorb_ctx* ctx, void* p);
int   eorb_dev_upload(eorb_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int   eorb_dev_download(eorb_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
