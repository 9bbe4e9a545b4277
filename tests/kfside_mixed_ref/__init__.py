"""Loader of the CPU restatement of MixedMatcher's KeyFrame-side matchers (kfside_mixed_ref.c, beside this file): compiled with the
host C compiler into a temporary directory when first used, strict IEEE.  Test infrastructure: nothing under eorb_slam_amd/ imports it.
Views and cameras are proj_ref's records.  The candidates of every search come from the oracle's orc_get_features_in_area, so
use_oracle(oracle) has to be called before search(); it also routes KannalaBrandt8 projections through the oracle's camera."""
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
from kfside_ref import OUT_FIELDS, Out, _ptr, _f, _out     # noqa: E402,F401

NO_TYPE_GATE, LEVEL_FROM_OCTAVE, ORB_SIGMA_TABLE = 1, 2, 4      # the wrong readings search(wrong=...) can be asked for

_libs = {}
_oracle_set = {}


def lib(timing=False):
    """the strict build the tests compare with; timing=True: the same source with -O3 -march=native (still -ffp-contract=off, same
    results), what tools/kfside_latency.py --mixed times on one core"""
    if timing in _libs:
        return _libs[timing]
    tmp = tempfile.mkdtemp(prefix="kfside_mixed_ref_")
    atexit.register(shutil.rmtree, tmp, True)
    so = os.path.join(tmp, "libkfside_mixed_ref.so")
    flags = (["-O3", "-march=native"] + proj_ref.CFLAGS[1:]) if timing else proj_ref.CFLAGS
    subprocess.check_call([os.environ.get("CC", "gcc")] + flags + [os.path.join(_HERE, "kfside_mixed_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, ci, cl, cf = C.c_void_p, C.c_int, C.c_long, C.c_float
    L.pr_set_project.restype = None; L.pr_set_project.argtypes = [vp]
    L.km_set_area.restype = None; L.km_set_area.argtypes = [vp]
    L.km_keyframe_side.restype = None; L.km_keyframe_side.argtypes = [vp, ci, cl, vp, vp, vp, vp, vp, vp, cf, vp]
    L.km_search.restype = None
    L.km_search.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, cl, vp, vp, vp, vp, vp, vp, vp, vp, cf, ci, vp, vp, vp, vp]
    _libs[timing] = L
    return L


def use_oracle(oracle):
    """GetFeaturesInArea and the KannalaBrandt8 projection are the oracle's"""
    if not _oracle_set.get("done"):
        area = C.cast(oracle.lib().orc_get_features_in_area, C.c_void_p)
        proj = C.cast(oracle.lib().orc_camera_project, C.c_void_p)
        for t in (False, True):
            lib(t).km_set_area(area); lib(t).pr_set_project(proj)
        _oracle_set["done"] = True
    return sys.modules[__name__]


def keyframe_side(views, pos, normal, min_dist, max_dist, th, mp_is_orb=None, skip=None, timing=False):
    """mode D with the tables picked per point, over one view or a list of K views -> dict(valid, uv, radius, level, q_ur, dist3d,
    reason), M entries for one view, K * M (entry k * M + m) for a list; skip has as many, mp_is_orb has M"""
    vs = [views] if isinstance(views, View) else list(views)
    va = (View * max(len(vs), 1))(*vs)
    pos = _f(pos, np.float32); normal = _f(normal, np.float32); min_dist = _f(min_dist, np.float32); max_dist = _f(max_dist, np.float32)
    skip = _f(skip, np.uint8); mio = _f(mp_is_orb, np.uint8)
    M = len(min_dist)
    rec, d = _out(len(vs) * M)
    lib(timing).km_keyframe_side(va, len(vs), M, _ptr(pos), _ptr(normal), _ptr(min_dist), _ptr(max_dist), _ptr(mio), _ptr(skip), float(th),
                                 C.byref(rec))
    return d


def search(frame, p, q_desc, kp_is_orb=None, kp_inv_sigma2=None, mp_is_orb=None, uright=None, taken=None, accept_thr=0.0, wrong=0,
           orb_inv_sigma2=None, timing=False):
    """the MixedMatcher search loop in an oracle Frame (its grid, keypoints and descriptors) over the projection p = dict(valid, uv,
    radius, level[, q_ur]).  kp_inv_sigma2 None: no reprojection gate; uright: the stereo gate (reads p["q_ur"]); taken: the in-order
    form.  -> (best_idx, best_dist[, taken]).  wrong: a sum of NO_TYPE_GATE, LEVEL_FROM_OCTAVE, ORB_SIGMA_TABLE (the last reads
    orb_inv_sigma2[octave])"""
    valid = _f(p["valid"], np.uint8); uv = _f(p["uv"], np.float32); radius = _f(p["radius"], np.float32); level = _f(p["level"], np.int32)
    q_desc = _f(q_desc, np.uint8)
    M = len(valid)
    bi = np.full(M, -1, np.int32); bd = np.full(M, 256, np.int32)
    tk = None if taken is None else np.array(taken, np.uint8)
    if frame is None or frame.N == 0:
        return (bi, bd) if tk is None else (bi, bd, tk)
    kio = _f(kp_is_orb, np.uint8); sig = _f(kp_inv_sigma2, np.float32); mio = _f(mp_is_orb, np.uint8); ur = _f(uright, np.float32)
    qur = None if ur is None else _f(p["q_ur"], np.float32)
    osig = _f(orb_inv_sigma2, np.float32)
    cand = np.zeros(frame.N, np.int32)
    lib(timing).km_search(frame.h, _ptr(frame.kps), frame.N, _ptr(frame.desc), frame.desc.shape[1], _ptr(kio), _ptr(sig), _ptr(ur), M, _ptr(valid),
                          _ptr(uv), _ptr(radius), _ptr(level), _ptr(q_desc), _ptr(mio), _ptr(qur), _ptr(tk), float(accept_thr), int(wrong),
                          _ptr(osig), _ptr(cand), _ptr(bi), _ptr(bd))
    return (bi, bd) if tk is None else (bi, bd, tk)
