"""ctypes binding of libeorb_fe.so (include/eorb_fe.h).  There is no CPU fallback: if the HIP library
is missing or fails to load, importing/using the front end raises."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EORB_FE_LIB") or os.path.join(_HERE, "csrc", "libeorb_fe.so")   # override: kernel experiments

EORB_OK, EORB_E_EMPTY, EORB_E_CONFIG, EORB_E_CAPACITY, EORB_E_ARG, EORB_E_HIP, EORB_E_NOTCONF = 0, -1, -2, -3, -4, -5, -6

# every symbol include/eorb_fe.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "eorb_create", "eorb_destroy", "eorb_sync", "eorb_debug_option", "eorb_debug_option_get", "eorb_debug_counter", "eorb_debug_stage", "eorb_last_error", "eorb_version",
    "eorb_prof_enable", "eorb_prof_reset", "eorb_prof_only", "eorb_prof_count", "eorb_prof_get",
    "eorb_ev2im", "eorb_ev2im_gauss", "eorb_set_undistort_maps", "eorb_undistort_events", "eorb_parse_events_text", "eorb_ev2im_gauss_raw", "eorb_ev2im_raw", "eorb_fe_run_batch_raw_dev", "eorb_fe_run_batch_raw4_dev", "eorb_fe_run_batch_raw2_dev", "eorb_fe_run_batch_images_dev", "eorb_ev2mci_se3", "eorb_ev2mci_se2", "eorb_ev2mci_se3_cam", "eorb_ev2mci_se2_cam", "eorb_measure_image_focus", "eorb_measure_image_focus_n", "eorb_normalize_minmax_u8",
    "eorb_set_calibration", "eorb_undistort_keypoints", "eorb_undistort_points", "eorb_generate_undistort_maps", "eorb_frame_mono",
    "eorb_orb_configure", "eorb_orb_max_keypoints", "eorb_orb_get_tables", "eorb_orb_extract",
    "eorb_search_for_initialization", "eorb_search_by_projection_last", "eorb_search_by_projection_map", "eorb_search_by_projection_kf", "eorb_search_by_projection_last_stereo", "eorb_search_by_projection_map_stereo", "eorb_frame_stereo",
    "eorb_frame_fisheye", "eorb_search_by_projection_map_fisheye", "eorb_search_by_projection_last_fisheye", "eorb_search_by_bow_fisheye",
    "eorb_hamming_bf_knn2", "eorb_search_by_bow", "eorb_search_by_bow_kf", "eorb_distinctive_descriptors", "eorb_hamming_window_match", "eorb_calc_optical_flow_pyr_lk", "eorb_bow_set_vocabulary", "eorb_bow_transform", "eorb_search_for_triangulation", "eorb_search_for_triangulation_kb8", "eorb_kb8_triangulate_matches", "eorb_kf_radius_match", "eorb_kf_radius_match_stereo", "eorb_sort_by_response", "eorb_resolve_num_mixed",
    "eorb_orb_tracked_descriptors", "eorb_orb_assign_level_by_best_desc",
    "eorb_fe_configure", "eorb_fe_run_batch_dev", "eorb_fe_last_f32_dev",
    "eorb_ev_slice_extract", "eorb_ev_slice_track", "eorb_ev_slice_image", "eorb_ev_mc_contest",
    "eorb_project_frustum", "eorb_project_last_frame", "eorb_project_keyframe_points", "eorb_search_local_points", "eorb_search_local_points_fisheye", "eorb_search_by_projection_last_pose", "eorb_search_by_projection_kf_pose",
    "eorb_project_keyframe_side", "eorb_fuse_pose", "eorb_search_by_projection_kf_scw", "eorb_search_by_sim3", "eorb_fuse_keyframes",
    "eorb_kf_radius_match_mixed", "eorb_project_keyframe_side_mixed", "eorb_fuse_pose_mixed", "eorb_search_by_projection_kf_scw_mixed",
    "eorb_fuse_keyframes_mixed",
    "eorb_search_for_triangulation_keyframes", "eorb_search_for_triangulation_kb8_keyframes", "eorb_search_by_bow_keyframes",
    "eorb_search_by_bow_kf_keyframes",
    "eorb_new_map_points", "eorb_create_new_map_points", "eorb_create_new_map_points_kb8",
    "eorb_kfdb_clear", "eorb_kfdb_add", "eorb_kfdb_erase", "eorb_kfdb_info", "eorb_kfdb_get_scores", "eorb_kfdb_detect_reloc", "eorb_kfdb_detect_nbest",
    "eorb_two_view_ransac", "eorb_two_view_check_rt", "eorb_two_view_reconstruct",
    "eorb_sim3_ransac", "eorb_mlpnp_ransac",
    "eorb_selfcheck_division", "eorb_selfcheck_math",
    "eorb_pack_events", "eorb_dev_alloc", "eorb_dev_free", "eorb_dev_upload", "eorb_dev_download",
]


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int), ("scaleFactor", C.c_float), ("nlevels", C.c_int),
                ("iniThFAST", C.c_int), ("minThFAST", C.c_int), ("edgeTh", C.c_int), ("imWidth", C.c_int)]


class Pinhole(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("model", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("k", C.c_float * 4), ("precision", C.c_float)]


def camera(cam):
    """(fx, fy, cx, cy) -> Pinhole; (fx, fy, cx, cy, k1, k2, k3, k4[, precision]) -> KannalaBrandt8 (KB8_DEF_PRECISION 1e-6)"""
    c = Camera()
    c.fx, c.fy, c.cx, c.cy = [float(v) for v in cam[:4]]
    if len(cam) > 4:
        c.model = 1
        for i in range(4):
            c.k[i] = float(cam[4 + i])
        c.precision = float(cam[8]) if len(cam) > 8 else 1e-6
    return c


class View(C.Structure):
    """eorb_view: one camera of a frame and its pose (the scale tables are host pointers: keep the arrays alive)"""
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("Ow", C.c_float * 3), ("cam", Camera),
                ("minX", C.c_float), ("maxX", C.c_float), ("minY", C.c_float), ("maxY", C.c_float), ("mbf", C.c_float),
                ("nlevels", C.c_int), ("log_scale", C.c_float), ("scale_factors", C.c_void_p),
                ("ak_nlevels", C.c_int), ("ak_log_scale", C.c_float), ("ak_scale_factors", C.c_void_p)]


class FrustumOut(C.Structure):
    """eorb_frustum_out: what isInFrustum leaves in a MapPoint, one array per member (any may be NULL)"""
    _fields_ = [("in_view", C.c_void_p), ("proj_xy", C.c_void_p), ("proj_xr", C.c_void_p), ("level", C.c_void_p),
                ("view_cos", C.c_void_p), ("depth", C.c_void_p), ("level_scale", C.c_void_p), ("reason", C.c_void_p)]


class KfSideOut(C.Structure):
    """eorb_kfside_out: the KeyFrame-side projection per (keyframe, map point), one array per member (any may be NULL)"""
    _fields_ = [("valid", C.c_void_p), ("uv", C.c_void_p), ("radius", C.c_void_p), ("level", C.c_void_p), ("q_ur", C.c_void_p),
                ("dist3d", C.c_void_p), ("reason", C.c_void_p)]


class KfSet(C.Structure):
    """eorb_kf_set: K keyframes concatenated (rows and feature vectors; the arrays are host pointers: keep them alive)"""
    _fields_ = [("K", C.c_int), ("kps", C.c_void_p), ("desc", C.c_void_p), ("stride", C.c_int), ("flag", C.c_void_p), ("kf_off", C.c_void_p),
                ("nodes", C.c_void_p), ("node_off", C.c_void_p), ("feat_off", C.c_void_p), ("idx", C.c_void_p)]


class Calib(C.Structure):
    """eorb_calib: MyCalibrator's K, distortion coefficients, R and P (src/Utils/MyCalibrator.cpp:11-17)"""
    _fields_ = [("model", C.c_int), ("K", C.c_float * 9), ("dist", C.c_float * 8), ("n_dist", C.c_int),
                ("R", C.c_float * 9), ("has_R", C.c_int), ("P", C.c_float * 12), ("p_cols", C.c_int)]


def calib(model, K, dist, R=None, P=None):
    """model 0 pinhole / 1 fisheye, K 3x3, dist (4, 5 or 8 / 4 coefficients), R 3x3 or None (cv::Mat()), P 3x3 / 3x4 or None"""
    import numpy as np
    q = Calib()
    q.model = int(model)
    K = np.asarray(K, np.float32).reshape(9)
    dist = np.asarray(dist, np.float32).reshape(-1)
    for i in range(9):
        q.K[i] = float(K[i])
    for i in range(min(len(dist), 8)):
        q.dist[i] = float(dist[i])
    q.n_dist = len(dist)
    if R is not None:
        R = np.asarray(R, np.float32).reshape(9)
        for i in range(9):
            q.R[i] = float(R[i])
        q.has_R = 1
    if P is not None:
        P = np.asarray(P, np.float32)
        q.p_cols = int(P.shape[1])
        P = P.reshape(-1)
        for i in range(min(len(P), 12)):
            q.P[i] = float(P[i])
    return q


class TvrParams(C.Structure):
    """eorb_tvr_params: mSigma, mThChiSqScore, mThChiSqF"""
    _fields_ = [("sigma", C.c_float), ("th_score", C.c_float), ("th_f", C.c_float)]


TVR_MAX_ITERS, TVR_MAX_MATCHES, TVR_MAX_KEYS, TVR_MAX_POSES = 1024, 16384, 1048576, 64
TVR_FORM_STOCK, TVR_FORM_INFO = 0, 1


class TvrReconParams(C.Structure):
    """eorb_tvr_recon_params: Params2VR as eorb_two_view_reconstruct takes it"""
    _fields_ = [("sigma", C.c_float), ("th_score", C.c_float), ("th_f", C.c_float), ("th_hf_ratio", C.c_float), ("min_parallax", C.c_float),
                ("min_parallax_crt", C.c_float), ("min_triangulated", C.c_int), ("th_min_good_r", C.c_float), ("th_max_good_r_f", C.c_float),
                ("th_max_good_r_h", C.c_float), ("th_rd_homo", C.c_float), ("form", C.c_int)]


class TvrReconResult(C.Structure):
    """eorb_tvr_recon_result"""
    _fields_ = [("ok", C.c_int32), ("stage", C.c_int32), ("is_homography", C.c_int32), ("SH", C.c_float), ("SF", C.c_float), ("RH", C.c_float),
                ("best_it_h", C.c_int32), ("best_it_f", C.c_int32), ("H21", C.c_float * 9), ("F21", C.c_float * 9), ("n_inliers", C.c_int32),
                ("n_min_good", C.c_int32), ("n_similar", C.c_int32), ("n_hyp", C.c_int32), ("hyp_good", C.c_int32 * 8),
                ("hyp_parallax", C.c_float * 8), ("info_good", C.c_int32 * 8), ("hyp_best", C.c_int32), ("hyp_second", C.c_int32),
                ("best_good", C.c_int32), ("second_good", C.c_int32), ("best_parallax", C.c_float), ("second_parallax", C.c_float)]


class Sim3Problem(C.Structure):
    """eorb_sim3_problem: one Sim3Solver (its correspondences and sets follow those of the problems before it in the flat arrays)"""
    _fields_ = [("N", C.c_int32), ("iters", C.c_int32), ("fix_scale", C.c_int32), ("min_inliers", C.c_int32),
                ("Rt1", C.c_float * 12), ("Rt2", C.c_float * 12), ("cam1", Camera), ("cam2", Camera)]


class Sim3Result(C.Structure):
    """eorb_sim3_result: bConverge, the winning iteration, its count, mnIterations, mBestT12 / Rotation / Translation / Scale"""
    _fields_ = [("converged", C.c_int32), ("best_it", C.c_int32), ("n_inliers", C.c_int32), ("iterations_used", C.c_int32),
                ("T12", C.c_float * 16), ("R12", C.c_float * 9), ("t12", C.c_float * 3), ("s12", C.c_float)]


S3_MAX_ITERS, S3_MAX_CORR, S3_MAX_PROBLEMS = 1024, 16384, 64


class MlpnpProblem(C.Structure):
    """eorb_mlpnp_problem: one MLPnPsolver (its correspondences and sets follow those of the problems before it in the flat arrays)"""
    _fields_ = [("N", C.c_int32), ("iters", C.c_int32), ("min_inliers", C.c_int32), ("th2", C.c_float), ("cam", Camera),
                ("first_it", C.c_int32), ("best_it", C.c_int32)]


class MlpnpResult(C.Structure):
    """eorb_mlpnp_result: where Refine returned true, mnIterations, the running best, mRefinedTcw or mBestTcw and its count"""
    _fields_ = [("stop_it", C.c_int32), ("iterations_used", C.c_int32), ("best_it", C.c_int32), ("n_best", C.c_int32),
                ("refined", C.c_int32), ("n_inliers", C.c_int32), ("Tcw", C.c_float * 16)]


PNP_MAX_ITERS, PNP_MAX_CORR, PNP_MAX_PROBLEMS = 1024, 4096, 64


class NewptsSide(C.Structure):
    """eorb_newpts_side: the per-keypoint arrays of one side of CreateNewMapPoints (host pointers, any may be NULL)"""
    _fields_ = [("kp_sigma2", C.c_void_p), ("kp_scale", C.c_void_p), ("kp_is_orb", C.c_void_p), ("uright", C.c_void_p), ("depth", C.c_void_p),
                ("raw_xy", C.c_void_p)]


class NewptsParams(C.Structure):
    """eorb_newpts_params"""
    _fields_ = [("form", C.c_int), ("views1", C.c_void_p), ("nleft1", C.c_int), ("mb1", C.c_float),
                ("views2", C.c_void_p), ("nleft2", C.c_void_p), ("mb2", C.c_void_p), ("side1", NewptsSide), ("side2", NewptsSide),
                ("level_scale", C.c_void_p), ("level_sigma2", C.c_void_p), ("nlevels", C.c_int),
                ("ratio_factor_orb", C.c_float), ("ratio_factor_ak", C.c_float), ("far_points", C.c_int), ("th_far_points", C.c_float)]


class NewptsOut(C.Structure):
    """eorb_newpts_out: dense K x n1 arrays (x3d, branch, cos_parallax may be NULL)"""
    _fields_ = [("status", C.c_void_p), ("x3d", C.c_void_p), ("branch", C.c_void_p), ("cos_parallax", C.c_void_p), ("n_new", C.c_void_p)]


NEWPTS_LOCAL_MAPPING, NEWPTS_TRACKING = 0, 1
NP_STATUS = ("new", "no_match", "claimed", "type", "parallax", "w_zero", "empty_stereo", "z1", "z2", "reproj1", "reproj2", "zero_dist", "far",
             "scale", "nonfinite")          # EORB_NP_*: the value is the index


class KltParams(C.Structure):
    _fields_ = [("win", C.c_int), ("maxLevel", C.c_int), ("maxCount", C.c_int), ("epsilon", C.c_double), ("minEigThreshold", C.c_float)]


class Se3Motion(C.Structure):
    _fields_ = [("angle", C.c_double), ("axis", C.c_double * 3), ("t", C.c_double * 3), ("medDepth", C.c_float)]


def se3_motion(m):
    """dict(angle, axis, t, medDepth) -> eorb_se3_motion (None -> None)"""
    if m is None:
        return None
    o = Se3Motion()
    o.angle = float(m["angle"]); o.medDepth = float(m["medDepth"])
    for i in range(3):
        o.axis[i] = float(m["axis"][i]); o.t[i] = float(m["t"][i])
    return o


class GridBounds(C.Structure):
    _fields_ = [("minX", C.c_float), ("minY", C.c_float), ("maxX", C.c_float), ("maxY", C.c_float),
                ("invW", C.c_float), ("invH", C.c_float)]


class FeConfig(C.Structure):
    _fields_ = [("W", C.c_int), ("H", C.c_int), ("sigma", C.c_float), ("pol", C.c_int),
                ("orb", OrbParams), ("lap0", C.c_int), ("lap1", C.c_int), ("want_desc", C.c_int),
                ("max_batch", C.c_int), ("max_events", C.c_int), ("match", C.c_int),
                ("windowSize", C.c_int), ("nnratio", C.c_float), ("checkOri", C.c_int)]


def build(force=False):
    """Compile libeorb_fe.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))
            if f.endswith((".hip", ".h"))] + [os.path.join(_HERE, "..", "include", "eorb_fe.h")]
    if not force and os.path.exists(LIB_PATH):
        newest = max(os.path.getmtime(s) for s in srcs)
        if os.path.getmtime(LIB_PATH) >= newest:
            return LIB_PATH
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-s"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libeorb_fe.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C eorb_slam_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    pi = C.POINTER(C.c_int)
    L.eorb_create.restype = ci; L.eorb_create.argtypes = [ci, vp, C.POINTER(vp)]
    L.eorb_destroy.restype = None; L.eorb_destroy.argtypes = [vp]
    L.eorb_sync.restype = ci; L.eorb_sync.argtypes = [vp]
    L.eorb_debug_option.restype = ci; L.eorb_debug_option.argtypes = [vp, C.c_char_p, ci]
    L.eorb_debug_option_get.restype = ci; L.eorb_debug_option_get.argtypes = [vp, C.c_char_p, C.POINTER(C.c_longlong)]
    L.eorb_debug_counter.restype = C.c_longlong; L.eorb_debug_counter.argtypes = [vp, C.c_char_p]
    L.eorb_debug_stage.restype = ci; L.eorb_debug_stage.argtypes = [vp, C.c_char_p, ci, ci, vp, C.c_size_t, pi, pi]
    L.eorb_last_error.restype = C.c_char_p; L.eorb_last_error.argtypes = [vp]
    L.eorb_version.restype = C.c_char_p; L.eorb_version.argtypes = []
    L.eorb_prof_enable.restype = ci; L.eorb_prof_enable.argtypes = [vp, ci]
    L.eorb_prof_reset.restype = ci; L.eorb_prof_reset.argtypes = [vp]
    L.eorb_prof_only.restype = ci; L.eorb_prof_only.argtypes = [vp, C.c_char_p]
    L.eorb_prof_count.restype = ci; L.eorb_prof_count.argtypes = [vp]
    L.eorb_prof_get.restype = ci
    L.eorb_prof_get.argtypes = [vp, ci, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.eorb_ev2im.restype = ci; L.eorb_ev2im.argtypes = [vp, vp, C.c_size_t, ci, ci, ci, ci, vp, vp, vp, pi]
    L.eorb_set_undistort_maps.restype = ci; L.eorb_set_undistort_maps.argtypes = [vp, vp, vp, ci, ci, ci]
    L.eorb_undistort_events.restype = ci
    L.eorb_undistort_events.argtypes = [vp, vp, C.c_size_t, ci, ci, C.c_double, vp, C.POINTER(C.c_size_t)]
    L.eorb_parse_events_text.restype = ci
    L.eorb_parse_events_text.argtypes = [vp, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]
    L.eorb_ev2im_gauss_raw.restype = ci; L.eorb_ev2im_gauss_raw.argtypes = [vp, vp, C.c_size_t, ci, ci, cf, ci, ci, vp, vp, vp]
    L.eorb_ev2im_raw.restype = ci; L.eorb_ev2im_raw.argtypes = [vp, vp, C.c_size_t, ci, ci, ci, ci, vp, vp, vp, pi]
    L.eorb_fe_run_batch_raw_dev.restype = ci
    L.eorb_fe_run_batch_raw_dev.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.eorb_fe_run_batch_raw4_dev.restype = ci
    L.eorb_fe_run_batch_raw4_dev.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.eorb_fe_run_batch_raw2_dev.restype = ci
    L.eorb_fe_run_batch_raw2_dev.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.eorb_fe_run_batch_images_dev.restype = ci
    L.eorb_fe_run_batch_images_dev.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp]
    L.eorb_ev2im_gauss.restype = ci; L.eorb_ev2im_gauss.argtypes = [vp, vp, C.c_size_t, ci, ci, cf, ci, ci, vp, vp, vp]
    cd = C.c_double
    L.eorb_ev2mci_se3.restype = ci
    L.eorb_ev2mci_se3.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pinhole), cd, vp, vp, cf, vp, ci, ci, cf, ci, ci, vp, vp, vp]
    L.eorb_ev2mci_se2.restype = ci
    L.eorb_ev2mci_se2.argtypes = [vp, vp, C.c_size_t, C.POINTER(Pinhole), vp, ci, ci, ci, cf, ci, ci, vp, vp, vp]
    L.eorb_ev2mci_se3_cam.restype = ci
    L.eorb_ev2mci_se3_cam.argtypes = [vp, vp, C.c_size_t, C.POINTER(Camera), cd, vp, vp, cf, vp, ci, ci, cf, ci, ci, vp, vp, vp]
    L.eorb_ev2mci_se2_cam.restype = ci
    L.eorb_ev2mci_se2_cam.argtypes = [vp, vp, C.c_size_t, C.POINTER(Camera), vp, ci, ci, ci, cf, ci, ci, vp, vp, vp]
    L.eorb_measure_image_focus.restype = ci; L.eorb_measure_image_focus.argtypes = [vp, vp, ci, ci, C.POINTER(cf)]
    L.eorb_measure_image_focus_n.restype = ci; L.eorb_measure_image_focus_n.argtypes = [vp, vp, ci, ci, ci, vp]
    L.eorb_normalize_minmax_u8.restype = ci; L.eorb_normalize_minmax_u8.argtypes = [vp, vp, ci, ci, vp]
    L.eorb_set_calibration.restype = ci; L.eorb_set_calibration.argtypes = [vp, C.POINTER(Calib)]
    L.eorb_undistort_keypoints.restype = ci; L.eorb_undistort_keypoints.argtypes = [vp, vp, ci, vp]
    L.eorb_undistort_points.restype = ci; L.eorb_undistort_points.argtypes = [vp, vp, ci, vp]
    L.eorb_generate_undistort_maps.restype = ci; L.eorb_generate_undistort_maps.argtypes = [vp, ci, ci, ci, vp, vp]
    L.eorb_frame_mono.restype = ci
    L.eorb_frame_mono.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, pi, pi, vp]
    L.eorb_orb_configure.restype = ci; L.eorb_orb_configure.argtypes = [vp, C.POINTER(OrbParams), ci, ci]
    L.eorb_orb_max_keypoints.restype = ci; L.eorb_orb_max_keypoints.argtypes = [vp]
    L.eorb_orb_get_tables.restype = ci; L.eorb_orb_get_tables.argtypes = [vp, vp, vp, vp, pi]
    L.eorb_orb_extract.restype = ci
    L.eorb_orb_extract.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, ci, pi, pi]
    L.eorb_search_for_initialization.restype = ci
    L.eorb_search_for_initialization.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, ci, vp,
                                                 C.POINTER(GridBounds), vp, vp, ci, cf, ci, pi]
    L.eorb_search_by_projection_last.restype = ci
    L.eorb_search_by_projection_last.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp,
                                                 C.POINTER(GridBounds), vp, cf, ci, ci, pi]
    L.eorb_search_by_projection_kf.restype = ci
    L.eorb_search_by_projection_kf.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, cf, ci, ci, pi]
    L.eorb_search_by_projection_map.restype = ci
    L.eorb_search_by_projection_map.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp,
                                                C.POINTER(GridBounds), vp, cf, cf, pi]
    L.eorb_search_by_projection_last_stereo.restype = ci
    L.eorb_search_by_projection_last_stereo.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp,
                                                        C.POINTER(GridBounds), vp, cf, ci, ci, vp, vp, pi]
    L.eorb_frame_stereo.restype = ci
    L.eorb_frame_stereo.argtypes = [vp, vp, vp, ci, ci, ci, cf, cf, vp, vp, pi, vp, vp, pi, ci, vp, vp, pi]
    L.eorb_search_by_projection_map_stereo.restype = ci
    L.eorb_search_by_projection_map_stereo.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp,
                                                       C.POINTER(GridBounds), vp, cf, cf, vp, vp, pi]
    L.eorb_orb_tracked_descriptors.restype = ci; L.eorb_orb_tracked_descriptors.argtypes = [vp, vp, ci, ci, ci, vp, ci, vp, vp]
    L.eorb_orb_assign_level_by_best_desc.restype = ci
    L.eorb_orb_assign_level_by_best_desc.argtypes = [vp, vp, ci, ci, ci, vp, vp, ci]
    L.eorb_frame_fisheye.restype = ci
    L.eorb_frame_fisheye.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, pi, pi, vp, vp, pi, pi, ci, vp, vp, pi]
    L.eorb_search_by_projection_map_fisheye.restype = ci
    L.eorb_search_by_projection_map_fisheye.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                        vp, vp, vp, vp, cf, cf, pi]
    L.eorb_search_by_projection_last_fisheye.restype = ci
    L.eorb_search_by_projection_last_fisheye.argtypes = [vp, vp, ci, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, cf, ci, ci, pi]
    L.eorb_search_by_bow_fisheye.restype = ci
    L.eorb_search_by_bow_fisheye.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, ci, ci, vp, vp, vp, vp, ci, vp, cf, ci, pi]
    L.eorb_search_by_bow.restype = ci
    L.eorb_search_by_bow.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, ci, vp, cf, ci, pi]
    L.eorb_search_by_bow_kf.restype = ci
    L.eorb_search_by_bow_kf.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, ci, vp, cf, ci, pi]
    L.eorb_search_for_triangulation.restype = ci
    L.eorb_search_for_triangulation.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, ci,
                                                vp, vp, vp, vp, ci, ci, ci, vp, pi]
    L.eorb_search_for_triangulation_kb8.restype = ci
    L.eorb_search_for_triangulation_kb8.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, ci, vp, ci, ci, vp, ci, vp, vp, vp, vp, ci,
                                                    vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, pi]
    L.eorb_kb8_triangulate_matches.restype = ci
    L.eorb_kb8_triangulate_matches.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, vp, ci, vp]
    L.eorb_kf_radius_match.restype = ci
    L.eorb_kf_radius_match.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, cf, vp, vp]
    L.eorb_kf_radius_match_stereo.restype = ci
    L.eorb_kf_radius_match_stereo.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp]
    L.eorb_calc_optical_flow_pyr_lk.restype = ci
    L.eorb_calc_optical_flow_pyr_lk.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp, ci, ci, ci, ci, C.c_double, ci, cf, vp, vp]
    L.eorb_bow_set_vocabulary.restype = ci; L.eorb_bow_set_vocabulary.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp]
    L.eorb_bow_transform.restype = ci
    L.eorb_bow_transform.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, pi, vp, vp, vp, pi, vp, vp]
    L.eorb_hamming_window_match.restype = ci
    L.eorb_hamming_window_match.argtypes = [vp, vp, ci, ci, vp, ci, ci, vp, vp, vp, vp, vp, vp]
    L.eorb_distinctive_descriptors.restype = ci; L.eorb_distinctive_descriptors.argtypes = [vp, vp, vp, ci, vp]
    L.eorb_sort_by_response.restype = ci; L.eorb_sort_by_response.argtypes = [vp, vp, ci, vp]
    L.eorb_resolve_num_mixed.restype = None; L.eorb_resolve_num_mixed.argtypes = [ci, ci, ci, ci, pi, pi]
    L.eorb_hamming_bf_knn2.restype = ci; L.eorb_hamming_bf_knn2.argtypes = [vp, vp, ci, vp, ci, vp, vp]
    L.eorb_fe_configure.restype = ci; L.eorb_fe_configure.argtypes = [vp, C.POINTER(FeConfig)]
    L.eorb_fe_run_batch_dev.restype = ci
    L.eorb_fe_run_batch_dev.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.eorb_fe_last_f32_dev.restype = ci; L.eorb_fe_last_f32_dev.argtypes = [vp, C.POINTER(vp), vp, ci]
    L.eorb_ev_slice_extract.restype = ci
    L.eorb_ev_slice_extract.argtypes = [vp, vp, vp, C.c_size_t, cf, ci, ci, ci, vp, vp, vp, ci, pi, pi, vp]
    L.eorb_ev_slice_track.restype = ci
    L.eorb_ev_slice_track.argtypes = [vp, vp, vp, C.c_size_t, cf, C.POINTER(KltParams), vp, vp, vp, ci, vp]
    L.eorb_ev_slice_image.restype = ci; L.eorb_ev_slice_image.argtypes = [vp, vp]
    L.eorb_ev_mc_contest.restype = ci
    L.eorb_ev_mc_contest.argtypes = [vp, vp, C.c_size_t, C.POINTER(Camera), C.POINTER(Se3Motion), C.POINTER(Se3Motion), vp, ci, ci, ci, cf,
                                     vp, pi, vp, vp, ci, ci, vp, ci, pi]
    L.eorb_project_frustum.restype = ci
    L.eorb_project_frustum.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, cf, vp, pi]
    L.eorb_project_last_frame.restype = ci
    L.eorb_project_last_frame.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.eorb_project_keyframe_points.restype = ci
    L.eorb_project_keyframe_points.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.eorb_search_local_points.restype = ci
    L.eorb_search_local_points.argtypes = [vp, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, cf, vp, vp, C.POINTER(GridBounds), vp, cf, cf,
                                           vp, ci, cf, vp, pi, pi]
    L.eorb_search_local_points_fisheye.restype = ci
    L.eorb_search_local_points_fisheye.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, cf, vp, vp, C.POINTER(GridBounds),
                                                   vp, cf, cf, ci, cf, vp, pi, pi]
    L.eorb_search_by_projection_last_pose.restype = ci
    L.eorb_search_by_projection_last_pose.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, C.POINTER(GridBounds), vp, cf, ci, ci,
                                                      vp, vp, vp, pi]
    L.eorb_search_by_projection_kf_pose.restype = ci
    L.eorb_search_by_projection_kf_pose.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, C.POINTER(GridBounds), vp, cf, ci, ci,
                                                    vp, vp, vp, pi]
    gbp = C.POINTER(GridBounds)
    L.eorb_project_keyframe_side.restype = ci
    L.eorb_project_keyframe_side.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, cf, vp]
    L.eorb_fuse_pose.restype = ci
    L.eorb_fuse_pose.argtypes = [vp, vp, ci, vp, ci, gbp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, cf, vp, vp, vp]
    L.eorb_search_by_projection_kf_scw.restype = ci
    L.eorb_search_by_projection_kf_scw.argtypes = [vp, vp, ci, vp, ci, gbp, vp, ci, vp, vp, vp, vp, vp, vp, cf, vp, cf, vp, vp, vp]
    L.eorb_search_by_sim3.restype = ci
    L.eorb_search_by_sim3.argtypes = [vp, vp, ci, vp, ci, gbp, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci, gbp, vp, vp, vp, vp, vp, vp,
                                      vp, vp, vp, vp, cf, ci, vp, pi, vp, vp]
    L.eorb_fuse_keyframes.restype = ci
    L.eorb_fuse_keyframes.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, cf, vp, vp, vp]
    L.eorb_kf_radius_match_mixed.restype = ci
    L.eorb_kf_radius_match_mixed.argtypes = [vp, vp, ci, vp, ci, gbp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, cf, vp, vp]
    L.eorb_project_keyframe_side_mixed.restype = ci
    L.eorb_project_keyframe_side_mixed.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, cf, vp]
    L.eorb_fuse_pose_mixed.restype = ci
    L.eorb_fuse_pose_mixed.argtypes = [vp, vp, ci, vp, ci, gbp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, cf, vp, vp, vp]
    L.eorb_search_by_projection_kf_scw_mixed.restype = ci
    L.eorb_search_by_projection_kf_scw_mixed.argtypes = [vp, vp, ci, vp, ci, gbp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, cf, vp, cf, vp, vp, vp]
    L.eorb_fuse_keyframes_mixed.restype = ci
    L.eorb_fuse_keyframes_mixed.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, cf, vp, vp, vp]
    ksp = C.POINTER(KfSet)
    L.eorb_search_for_triangulation_keyframes.restype = ci
    L.eorb_search_for_triangulation_keyframes.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp, ci, ksp, vp, vp, vp, vp, ci, ci, ci, vp, vp]
    L.eorb_search_for_triangulation_kb8_keyframes.restype = ci
    L.eorb_search_for_triangulation_kb8_keyframes.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, ci, ksp, vp, vp, vp, vp, vp, vp, vp, vp, ci,
                                                              ci, ci, vp, vp]
    L.eorb_search_by_bow_keyframes.restype = ci
    L.eorb_search_by_bow_keyframes.argtypes = [vp, ksp, vp, ci, vp, vp, vp, vp, ci, vp, cf, ci, vp]
    L.eorb_search_by_bow_kf_keyframes.restype = ci
    L.eorb_search_by_bow_kf_keyframes.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, ci, ksp, vp, cf, ci, vp]
    npp, npo = C.POINTER(NewptsParams), C.POINTER(NewptsOut)
    L.eorb_new_map_points.restype = ci; L.eorb_new_map_points.argtypes = [vp, vp, ci, vp, vp, ci, vp, npp, npo]
    L.eorb_create_new_map_points.restype = ci
    L.eorb_create_new_map_points.argtypes = L.eorb_search_for_triangulation_keyframes.argtypes + [npp, npo]
    L.eorb_create_new_map_points_kb8.restype = ci
    L.eorb_create_new_map_points_kb8.argtypes = L.eorb_search_for_triangulation_kb8_keyframes.argtypes + [npp, npo]
    L.eorb_kfdb_clear.restype = ci; L.eorb_kfdb_clear.argtypes = [vp]
    L.eorb_kfdb_add.restype = ci; L.eorb_kfdb_add.argtypes = [vp, ci, vp, vp, vp, vp]
    L.eorb_kfdb_erase.restype = ci; L.eorb_kfdb_erase.argtypes = [vp, ci]
    L.eorb_kfdb_info.restype = ci; L.eorb_kfdb_info.argtypes = [vp, pi, pi]
    L.eorb_kfdb_get_scores.restype = ci; L.eorb_kfdb_get_scores.argtypes = [vp, ci, vp]
    L.eorb_kfdb_detect_reloc.restype = ci
    L.eorb_kfdb_detect_reloc.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, pi, pi, pi, C.POINTER(cf)]
    L.eorb_kfdb_detect_nbest.restype = ci
    L.eorb_kfdb_detect_nbest.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, pi, pi, pi, C.POINTER(cf)]
    L.eorb_two_view_ransac.restype = ci
    L.eorb_two_view_ransac.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, ci, C.POINTER(TvrParams), vp, C.POINTER(cf), pi, vp, vp, C.POINTER(cf), pi, vp,
                                       vp, vp, vp, vp]
    L.eorb_sim3_ransac.restype = ci
    L.eorb_sim3_ransac.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.eorb_mlpnp_ransac.restype = ci
    L.eorb_mlpnp_ransac.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.eorb_two_view_check_rt.restype = ci
    L.eorb_two_view_check_rt.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, vp, cf, cf, ci, vp, ci, vp, vp, vp, vp, vp]
    L.eorb_two_view_reconstruct.restype = ci
    L.eorb_two_view_reconstruct.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, ci, vp, C.POINTER(TvrReconParams), C.POINTER(TvrReconResult),
                                            vp, vp, vp, vp, vp, vp]
    L.eorb_selfcheck_division.restype = ci; L.eorb_selfcheck_division.argtypes = [vp, cf, cf, cf, C.POINTER(C.c_uint64)]
    L.eorb_selfcheck_math.restype = ci; L.eorb_selfcheck_math.argtypes = [vp, ci, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.eorb_pack_events.restype = None; L.eorb_pack_events.argtypes = [vp, C.c_size_t, vp]
    L.eorb_dev_alloc.restype = vp; L.eorb_dev_alloc.argtypes = [vp, C.c_size_t]
    L.eorb_dev_free.restype = ci; L.eorb_dev_free.argtypes = [vp, vp]
    L.eorb_dev_upload.restype = ci; L.eorb_dev_upload.argtypes = [vp, vp, vp, C.c_size_t]
    L.eorb_dev_download.restype = ci; L.eorb_dev_download.argtypes = [vp, vp, vp, C.c_size_t]
    _lib = L
    return L
