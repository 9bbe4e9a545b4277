"""Loader of the CPU restatement of the projector's KeyFrame-side modes (kfside_ref.c, beside this file): compiled with the host C
compiler into a temporary directory when first used, strict IEEE.  Test infrastructure: nothing under eorb_slam_amd/ imports it.  Views
and cameras are proj_ref's records; the KannalaBrandt8 projection is the oracle's orc_camera_project, as in proj_ref."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
import proj_ref                                     # noqa: E402
from proj_ref import View, view, camera            # noqa: E402,F401

OUT_FIELDS = (("valid", np.uint8, 1), ("uv", np.float32, 2), ("radius", np.float32, 1), ("level", np.int32, 1), ("q_ur", np.float32, 1),
              ("dist3d", np.float32, 1), ("reason", np.uint8, 1))


class Out(C.Structure):
    _fields_ = [(n, C.c_void_p) for n, _, _ in OUT_FIELDS]


_libs = {}
_project_set = {}


def lib(timing=False):
    """the strict build the tests compare with; timing=True: the same source with -O3 -march=native (still -ffp-contract=off, same
    results), what tools/kfside_latency.py times on one core"""
    if timing in _libs:
        return _libs[timing]
    tmp = tempfile.mkdtemp(prefix="kfside_ref_")
    atexit.register(shutil.rmtree, tmp, True)
    so = os.path.join(tmp, "libkfside_ref.so")
    flags = (["-O3", "-march=native"] + proj_ref.CFLAGS[1:]) if timing else proj_ref.CFLAGS
    subprocess.check_call([os.environ.get("CC", "gcc")] + flags + [os.path.join(_HERE, "kfside_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, ci, cl, cf = C.c_void_p, C.c_int, C.c_long, C.c_float
    L.pr_set_project.restype = None; L.pr_set_project.argtypes = [vp]
    L.kr_keyframe_side.restype = None; L.kr_keyframe_side.argtypes = [vp, ci, cl, vp, vp, vp, vp, vp, cf, vp]
    L.kr_sim3_half.restype = None; L.kr_sim3_half.argtypes = [vp, vp, vp, vp, vp, vp, cl, vp, vp, vp, vp, cf, vp]
    L.kr_angle_rejects_float.restype = ci; L.kr_angle_rejects_float.argtypes = [vp, vp, cf]
    L.kr_angle_rejects_double.restype = ci; L.kr_angle_rejects_double.argtypes = [vp, vp]
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


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f(a, dt):
    return None if a is None else np.ascontiguousarray(a, dt)


def _out(n):
    rec = Out()
    d = {}
    for name, dt, k in OUT_FIELDS:
        d[name] = np.zeros((n, k) if k > 1 else n, dt)
        setattr(rec, name, d[name].ctypes.data)
    return rec, d


def keyframe_side(views, pos, normal, min_dist, max_dist, th, skip=None, timing=False):
    """mode D over one view or a list of K views -> dict(valid, uv, radius, level, q_ur, dist3d, reason), M entries for one view,
    K * M (entry k * M + m) for a list; skip has as many"""
    vs = [views] if isinstance(views, View) else list(views)
    va = (View * max(len(vs), 1))(*vs)
    pos = _f(pos, np.float32); normal = _f(normal, np.float32); min_dist = _f(min_dist, np.float32); max_dist = _f(max_dist, np.float32)
    skip = _f(skip, np.uint8)
    M = len(min_dist)
    rec, d = _out(len(vs) * M)
    lib(timing).kr_keyframe_side(va, len(vs), M, _ptr(pos), _ptr(normal), _ptr(min_dist), _ptr(max_dist), _ptr(skip), float(th), C.byref(rec))
    return d


def sim3_half(va, sRb, tb, cam4, vb, pos, min_dist, max_dist, th, skip=None, timing=False):
    """mode E, one direction: the points of keyframe a (view va: R, t) through (sRb, tb) into keyframe b (view vb: bounds, tables),
    projected with cam4 = (fx, fy, cx, cy)"""
    pos = _f(pos, np.float32); min_dist = _f(min_dist, np.float32); max_dist = _f(max_dist, np.float32); skip = _f(skip, np.uint8)
    Ra = np.array(list(va.R), np.float32); ta = np.array(list(va.t), np.float32)
    sRb = np.ascontiguousarray(sRb, np.float32).reshape(9); tb = np.ascontiguousarray(tb, np.float32).reshape(3)
    cam = np.array(cam4[:4], np.float32)
    n = len(min_dist)
    rec, d = _out(n)
    lib(timing).kr_sim3_half(_ptr(Ra), _ptr(ta), _ptr(sRb), _ptr(tb), _ptr(cam), C.byref(vb), n, _ptr(pos), _ptr(min_dist), _ptr(max_dist),
                             _ptr(skip), float(th), C.byref(rec))
    del d["q_ur"]
    return d


def angle_rejects(PO, Pn):
    """(as the double comparison of Fuse decides, as a float quotient against 0.5f would) for one point"""
    PO = np.ascontiguousarray(PO, np.float32); Pn = np.ascontiguousarray(Pn, np.float32)
    return bool(lib().kr_angle_rejects_double(_ptr(PO), _ptr(Pn))), bool(lib().kr_angle_rejects_float(_ptr(PO), _ptr(Pn), 0.5))
