"""Loader of the CPU restatement of MyCalibrator (calib_ref.c, beside this file): compiled with the host C compiler into a temporary
directory when first used, strict IEEE.  Test infrastructure: nothing under eorb_slam_amd/ imports it."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-std=c99", "-Wall"]

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


class Calib(C.Structure):
    _fields_ = [("model", C.c_int), ("K", C.c_float * 9), ("dist", C.c_float * 8), ("n_dist", C.c_int),
                ("R", C.c_float * 9), ("has_R", C.c_int), ("P", C.c_float * 12), ("p_cols", C.c_int)]


_libs = {}


def lib(timing=False):
    """the strict build the tests compare with; timing=True: the same source with -O3 -march=native (still -ffp-contract=off, same
    results), what tools/calib_latency.py times on one core"""
    if timing in _libs:
        return _libs[timing]
    tmp = tempfile.mkdtemp(prefix="calib_ref_")
    atexit.register(shutil.rmtree, tmp, True)
    so = os.path.join(tmp, "libcalib_ref.so")
    flags = (["-O3", "-march=native"] + CFLAGS[1:]) if timing else CFLAGS
    subprocess.check_call([os.environ.get("CC", "gcc")] + flags + [os.path.join(_HERE, "calib_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, ci, cl = C.c_void_p, C.c_int, C.c_long
    L.cr_tan.restype = C.c_double; L.cr_tan.argtypes = [C.c_double]
    L.cr_tan_n.restype = None; L.cr_tan_n.argtypes = [vp, cl, vp]
    L.cr_is_distorted.restype = ci; L.cr_is_distorted.argtypes = [C.POINTER(Calib)]
    L.cr_valid.restype = ci; L.cr_valid.argtypes = [C.POINTER(Calib)]
    L.cr_undistort_points.restype = None; L.cr_undistort_points.argtypes = [C.POINTER(Calib), vp, cl, vp, ci]
    L.cr_cv_undistort_points.restype = None; L.cr_cv_undistort_points.argtypes = [C.POINTER(Calib), vp, cl, vp]
    L.cr_undistort_keypoints.restype = None; L.cr_undistort_keypoints.argtypes = [C.POINTER(Calib), vp, cl, vp]
    L.cr_generate_maps.restype = None; L.cr_generate_maps.argtypes = [C.POINTER(Calib), ci, ci, vp, vp, ci]
    L.cr_image_bounds.restype = None; L.cr_image_bounds.argtypes = [C.POINTER(Calib), ci, ci, vp]
    _libs[timing] = L
    return L


def calib(d):
    """a calibration dict (model, K 3x3, dist, R 3x3 | None, P 3x3 | 3x4 | None) -> the C record"""
    q = Calib()
    q.model = int(d["model"])
    K = np.asarray(d["K"], np.float32).reshape(9)
    dist = np.asarray(d["dist"], np.float32).reshape(-1)
    for i in range(9):
        q.K[i] = float(K[i])
    for i in range(min(len(dist), 8)):
        q.dist[i] = float(dist[i])
    q.n_dist = len(dist)
    if d.get("R") is not None:
        R = np.asarray(d["R"], np.float32).reshape(9)
        for i in range(9):
            q.R[i] = float(R[i])
        q.has_R = 1
    if d.get("P") is not None:
        P = np.asarray(d["P"], np.float32)
        q.p_cols = int(P.shape[1])
        for i, v in enumerate(P.reshape(-1)[:12]):
            q.P[i] = float(v)
    return q


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def tan(x):
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty_like(x)
    lib().cr_tan_n(_ptr(x), x.size, _ptr(out))
    return out


def undistort_points(d, xy, host_tan=False):
    """MyCalibrator::undistPointPinhole / undistPointFishEye over (n, 2) float32 points"""
    xy = np.ascontiguousarray(xy, np.float32)
    out = np.empty_like(xy)
    q = calib(d)
    lib().cr_undistort_points(C.byref(q), _ptr(xy), xy.size // 2, _ptr(out), int(host_tan))
    return out


def cv_undistort_points(d, xy):
    """cv::undistortPoints / cv::fisheye::undistortPoints themselves (no isDistorted gate)"""
    xy = np.ascontiguousarray(xy, np.float32)
    out = np.empty_like(xy)
    q = calib(d)
    lib().cr_cv_undistort_points(C.byref(q), _ptr(xy), xy.size // 2, _ptr(out))
    return out


def undistort_keypoints(d, kps, out=None, timing=False):
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    if out is None:
        out = np.zeros(len(kps), KP_DTYPE)
    q = calib(d)
    lib(timing).cr_undistort_keypoints(C.byref(q), _ptr(kps), len(kps), _ptr(out))
    return out


def generate_maps(d, LW, LH, host_tan=False, timing=False):
    mx = np.empty((LH, LW), np.float32); my = np.empty((LH, LW), np.float32)
    q = calib(d)
    lib(timing).cr_generate_maps(C.byref(q), LW, LH, _ptr(mx), _ptr(my), int(host_tan))
    return mx, my


def image_bounds(d, W, H):
    b = np.zeros(4, np.float32)
    q = calib(d)
    lib().cr_image_bounds(C.byref(q), W, H, _ptr(b))
    return b
