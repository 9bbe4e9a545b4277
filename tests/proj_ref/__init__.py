"""Loader of the CPU restatement of the map-point projector (proj_ref.c, beside this file): compiled with the host C compiler into a
temporary directory when first used, strict IEEE.  Test infrastructure: nothing under eorb_slam_amd/ imports it.  The KannalaBrandt8
projection is the oracle's orc_camera_project, handed to the restatement as a function pointer."""
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
FRUSTUM_FIELDS = (("in_view", np.uint8, 1), ("proj_xy", np.float32, 2), ("proj_xr", np.float32, 1), ("level", np.int32, 1),
                  ("view_cos", np.float32, 1), ("depth", np.float32, 1), ("level_scale", np.float32, 1), ("reason", np.uint8, 1))


class Camera(C.Structure):
    _fields_ = [("model", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("k", C.c_float * 4), ("precision", C.c_float)]


class View(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("Ow", C.c_float * 3), ("cam", Camera),
                ("minX", C.c_float), ("maxX", C.c_float), ("minY", C.c_float), ("maxY", C.c_float), ("mbf", C.c_float),
                ("nlevels", C.c_int), ("log_scale", C.c_float), ("scale_factors", C.c_void_p),
                ("ak_nlevels", C.c_int), ("ak_log_scale", C.c_float), ("ak_scale_factors", C.c_void_p)]


class FrustumOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _, _ in FRUSTUM_FIELDS] + [("search", C.c_void_p)]


_libs = {}
_project_set = {}


def lib(timing=False):
    """the strict build the tests compare with; timing=True: the same source with -O3 -march=native (still -ffp-contract=off, same
    results), what tools/project_latency.py times on one core and what the whole-range hashes use"""
    if timing in _libs:
        return _libs[timing]
    tmp = tempfile.mkdtemp(prefix="proj_ref_")
    atexit.register(shutil.rmtree, tmp, True)
    so = os.path.join(tmp, "libproj_ref.so")
    flags = (["-O3", "-march=native"] + CFLAGS[1:]) if timing else CFLAGS
    subprocess.check_call([os.environ.get("CC", "gcc")] + flags + [os.path.join(_HERE, "proj_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, ci, cl, cf, u32 = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_uint32
    L.pr_set_project.restype = None; L.pr_set_project.argtypes = [vp]
    L.pr_logf.restype = cf; L.pr_logf.argtypes = [cf]
    L.pr_logf_n.restype = None; L.pr_logf_n.argtypes = [vp, cl, vp]
    L.pr_logf_mismatches.restype = C.c_uint64; L.pr_logf_mismatches.argtypes = [u32, u32, C.POINTER(u32)]
    L.pr_math_hash.restype = C.c_uint64; L.pr_math_hash.argtypes = [ci, u32, u32]
    L.pr_predict_scale.restype = ci; L.pr_predict_scale.argtypes = [cf, cf, ci, cf]
    L.pr_frustum.restype = ci; L.pr_frustum.argtypes = [vp, ci, cl, vp, vp, vp, vp, vp, vp, cf, ci, cf, vp]
    L.pr_last.restype = None; L.pr_last.argtypes = [vp, vp, vp, cl, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.pr_kf.restype = None; L.pr_kf.argtypes = [vp, cl, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    _libs[timing] = L
    return L


def use_oracle_camera(oracle, timing=False):
    """KannalaBrandt8 views: project through the oracle's orc_camera_project (same record layout as eorb_camera)"""
    if not _project_set.get("done"):
        fn = C.cast(oracle.lib().orc_camera_project, C.c_void_p)
        for t in (False, True):
            lib(t).pr_set_project(fn)
        _project_set["done"] = True
    return lib(timing)


def camera(cam):
    """(fx, fy, cx, cy) -> Pinhole; (fx, fy, cx, cy, k1..k4[, precision]) -> KannalaBrandt8"""
    c = Camera()
    c.fx, c.fy, c.cx, c.cy = [float(v) for v in cam[:4]]
    if len(cam) > 4:
        c.model = 1
        for i in range(4):
            c.k[i] = float(cam[4 + i])
        c.precision = float(cam[8]) if len(cam) > 8 else 1e-6
    return c


def view(R, t, Ow, cam, bounds, nlevels, log_scale, scale_factors, mbf=0.0, ak_nlevels=0, ak_log_scale=0.0, ak_scale_factors=None):
    v = View()
    for dst, src, k in ((v.R, R, 9), (v.t, t, 3), (v.Ow, Ow, 3)):
        a = np.asarray(src, np.float32).reshape(-1)
        for i in range(k):
            dst[i] = float(a[i])
    v.cam = camera(cam)
    v.minX, v.maxX, v.minY, v.maxY = [float(b) for b in bounds]
    v.mbf = float(mbf)
    v.nlevels = int(nlevels); v.log_scale = float(log_scale)
    v._sf = np.ascontiguousarray(scale_factors, np.float32); v.scale_factors = v._sf.ctypes.data
    v.ak_nlevels = int(ak_nlevels); v.ak_log_scale = float(ak_log_scale)
    v._ak = None if ak_scale_factors is None else np.ascontiguousarray(ak_scale_factors, np.float32)
    v.ak_scale_factors = None if v._ak is None else v._ak.ctypes.data
    return v


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f(a, dt):
    return None if a is None else np.ascontiguousarray(a, dt)


def logf(x):
    return np.float32(lib().pr_logf(float(np.float32(x))))


def logf_n(x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    lib().pr_logf_n(_ptr(x), x.size, _ptr(out))
    return out


def logf_mismatches(lo_bits, hi_bits):
    first = C.c_uint32(0)
    n = lib(True).pr_logf_mismatches(lo_bits, hi_bits, C.byref(first))
    return int(n), int(first.value)


def math_hash(which, lo_bits, hi_bits):
    return int(lib(True).pr_math_hash(which, lo_bits, hi_bits))


def predict_scale(max_dist, dist, nlevels, log_scale):
    return int(lib().pr_predict_scale(float(np.float32(max_dist)), float(np.float32(dist)), int(nlevels), float(np.float32(log_scale))))


def frustum(views, pos, normal, min_dist, max_dist, cos_limit=0.5, skip=None, mp_is_orb=None, far=False, th_far=0.0, timing=False):
    """mode A over one view or a (left, right) pair -> (n_in_view, [dict per view]) with the eorb_frustum_out arrays plus `search`"""
    vs = [views] if isinstance(views, View) else list(views)
    va = (View * len(vs))(*vs)
    pos = _f(pos, np.float32); normal = _f(normal, np.float32); min_dist = _f(min_dist, np.float32); max_dist = _f(max_dist, np.float32)
    skip = _f(skip, np.uint8); mp_is_orb = _f(mp_is_orb, np.uint8)
    M = len(min_dist)
    recs = (FrustumOut * len(vs))()
    outs = []
    for v in range(len(vs)):
        d = {}
        for name, dt, k in FRUSTUM_FIELDS + (("search", np.uint8, 1),):
            d[name] = np.zeros((M, k) if k > 1 else M, dt)
            setattr(recs[v], name, d[name].ctypes.data)
        outs.append(d)
    n = lib(timing).pr_frustum(va, len(vs), M, _ptr(pos), _ptr(normal), _ptr(min_dist), _ptr(max_dist), _ptr(skip), _ptr(mp_is_orb),
                               float(cos_limit), int(far), float(th_far), recs)
    return n, outs


def last_frame(v, pos, last_kps, skip=None, last_is_orb=None, cam_r=None, Trl=None, timing=False):
    """mode B -> dict(valid, uv, proj_ur, level_scale, uv_r)"""
    pos = _f(pos, np.float32); kps = np.ascontiguousarray(last_kps, KP_DTYPE); n = len(kps)
    skip = _f(skip, np.uint8); lio = _f(last_is_orb, np.uint8)
    o = dict(valid=np.zeros(n, np.uint8), uv=np.zeros((n, 2), np.float32), proj_ur=np.zeros(n, np.float32), level_scale=np.zeros(n, np.float32),
             uv_r=np.zeros((n, 2), np.float32))
    camr = None if Trl is None else camera(cam_r)
    trl = None if Trl is None else np.ascontiguousarray(Trl, np.float32).reshape(12)
    lib(timing).pr_last(C.byref(v), None if camr is None else C.byref(camr), _ptr(trl), n, _ptr(pos), _ptr(skip), _ptr(kps), _ptr(lio),
                        _ptr(o["valid"]), _ptr(o["uv"]), _ptr(o["proj_ur"]), _ptr(o["level_scale"]), _ptr(o["uv_r"]))
    if Trl is None:
        del o["uv_r"]
    return o


def keyframe_points(v, pos, min_dist, max_dist, skip=None, mp_is_orb=None, timing=False):
    """mode C -> dict(valid, uv, level, level_scale, dist3d)"""
    pos = _f(pos, np.float32); min_dist = _f(min_dist, np.float32); max_dist = _f(max_dist, np.float32)
    skip = _f(skip, np.uint8); mio = _f(mp_is_orb, np.uint8)
    n = len(min_dist)
    o = dict(valid=np.zeros(n, np.uint8), uv=np.zeros((n, 2), np.float32), level=np.zeros(n, np.int32), level_scale=np.zeros(n, np.float32),
             dist3d=np.zeros(n, np.float32))
    lib(timing).pr_kf(C.byref(v), n, _ptr(pos), _ptr(min_dist), _ptr(max_dist), _ptr(skip), _ptr(mio),
                      _ptr(o["valid"]), _ptr(o["uv"]), _ptr(o["level"]), _ptr(o["level_scale"]), _ptr(o["dist3d"]))
    return o
