"""Loader of the CPU restatement of the two-view reconstruction stages (twoview_ref.c, beside this file): compiled with the host C
compiler into a temporary directory when first used, strict IEEE.  Test infrastructure: nothing under eorb_slam_amd/ imports it."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-std=c99", "-Wall"]

_libs = {}


def lib(timing=False):
    """the strict build the tests compare with; timing=True: the same source with -O3 -march=native (still -ffp-contract=off, same
    results), what tools/twoview_latency.py times"""
    if timing in _libs:
        return _libs[timing]
    tmp = tempfile.mkdtemp(prefix="twoview_ref_")
    atexit.register(shutil.rmtree, tmp, True)
    so = os.path.join(tmp, "libtwoview_ref.so")
    flags = (["-O3", "-march=native"] + CFLAGS[1:]) if timing else CFLAGS
    subprocess.check_call([os.environ.get("CC", "gcc")] + flags + [os.path.join(_HERE, "twoview_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.tvr_svd.restype = None; L.tvr_svd.argtypes = [vp, ci, ci, vp, vp, vp]
    L.tvr_inv33.restype = None; L.tvr_inv33.argtypes = [vp, vp]
    L.tvr_compute_h21.restype = None; L.tvr_compute_h21.argtypes = [vp, vp, vp]
    L.tvr_compute_f21.restype = None; L.tvr_compute_f21.argtypes = [vp, vp, vp]
    L.tvr_check_homography.restype = cf; L.tvr_check_homography.argtypes = [vp, vp, vp, vp, vp, ci, cf, cf, vp]
    L.tvr_check_fundamental.restype = cf; L.tvr_check_fundamental.argtypes = [vp, vp, vp, vp, ci, cf, cf, cf, vp]
    L.tvr_ransac.restype = ci
    L.tvr_ransac.argtypes = [vp, ci, vp, ci, vp, ci, vp, ci, cf, cf, cf, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tvr_check_rt.restype = ci
    L.tvr_check_rt.argtypes = [vp, ci, vp, ci, vp, ci, vp, vp, cf, cf, ci, vp, ci, vp, vp, vp, vp, vp]
    _libs[timing] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _pts(kps):
    """(x, y) of keypoints given as a structured array with x / y fields or as an [n, 2] array -> contiguous float32 [n, 2]"""
    kps = np.asarray(kps)
    if kps.dtype.names:
        return np.ascontiguousarray(np.stack([kps["x"], kps["y"]], axis=1), np.float32)
    return np.ascontiguousarray(kps, np.float32).reshape(-1, 2)


def svd(A):
    """cv::SVDecomp(A, w, u, vt, MODIFY_A | FULL_UV) on a float matrix of at most 16 x 16 -> (w, u, vt)"""
    A = np.ascontiguousarray(A, np.float32)
    r, c = A.shape
    w = np.zeros(min(r, c), np.float32); u = np.zeros((r, r), np.float32); vt = np.zeros((c, c), np.float32)
    lib().tvr_svd(_p(A), r, c, _p(w), _p(u), _p(vt))
    return w, u, vt


def inv33(S):
    S = np.ascontiguousarray(S, np.float32); D = np.zeros((3, 3), np.float32)
    lib().tvr_inv33(_p(S), _p(D))
    return D


def compute_h21(p1, p2):
    p1 = np.ascontiguousarray(p1, np.float32); p2 = np.ascontiguousarray(p2, np.float32); H = np.zeros((3, 3), np.float32)
    assert p1.shape == (8, 2) and p2.shape == (8, 2)
    lib().tvr_compute_h21(_p(p1), _p(p2), _p(H))
    return H


def compute_f21(p1, p2):
    p1 = np.ascontiguousarray(p1, np.float32); p2 = np.ascontiguousarray(p2, np.float32); F = np.zeros((3, 3), np.float32)
    assert p1.shape == (8, 2) and p2.shape == (8, 2)
    lib().tvr_compute_f21(_p(p1), _p(p2), _p(F))
    return F


def check_homography(H21, H12, kps1, kps2, matches12, sigma=1.0, th=5.991):
    """CheckHomography -> (score, inliers)"""
    p1, p2 = _pts(kps1), _pts(kps2); m = np.ascontiguousarray(matches12, np.int32)
    H21 = np.ascontiguousarray(H21, np.float32); H12 = np.ascontiguousarray(H12, np.float32)
    inl = np.zeros(len(m), np.uint8)
    s = lib().tvr_check_homography(_p(H21), _p(H12), _p(p1), _p(p2), _p(m), len(m), sigma, th, _p(inl))
    return np.float32(s), inl


def check_fundamental(F21, kps1, kps2, matches12, sigma=1.0, th=3.841, th_score=5.991):
    """CheckFundamental -> (score, inliers)"""
    p1, p2 = _pts(kps1), _pts(kps2); m = np.ascontiguousarray(matches12, np.int32)
    F21 = np.ascontiguousarray(F21, np.float32)
    inl = np.zeros(len(m), np.uint8)
    s = lib().tvr_check_fundamental(_p(F21), _p(p1), _p(p2), _p(m), len(m), sigma, th, th_score, _p(inl))
    return np.float32(s), inl


class TwoViewReconstruction:
    """mirrors eorb_slam_amd.frontend.TwoViewReconstruction: the same methods, arguments and result dicts"""

    def __init__(self, K, sigma=1.0, iterations=200, th_score=5.991, th_f=3.841, min_parallax_crt=0.99998, min_triangulated=50, timing=False):
        self.L = lib(timing)
        self.K = np.ascontiguousarray(np.asarray(K, np.float32).reshape(3, 3))
        self.sigma, self.iterations, self.th_score, self.th_f = float(sigma), int(iterations), float(th_score), float(th_f)
        self.min_parallax_crt, self.min_triangulated = float(np.float32(min_parallax_crt)), int(min_triangulated)

    def prepare(self, kps1, kps2, matches12, sets):
        """the arrays of a find_homography_fundamental call, for a caller that times `run` alone"""
        p1, p2 = _pts(kps1), _pts(kps2)
        m = np.ascontiguousarray(matches12, np.int32); sets = np.ascontiguousarray(sets, np.int32)
        assert m.ndim == 2 and m.shape[1] == 2 and sets.ndim == 2 and sets.shape[1] == 8
        N, it = len(m), len(sets)
        o = dict(H21=np.zeros((3, 3), np.float32), F21=np.zeros((3, 3), np.float32), inliers_h=np.zeros(N, np.uint8), inliers_f=np.zeros(N, np.uint8),
                 it_score_h=np.zeros(it, np.float32), it_score_f=np.zeros(it, np.float32), it_H=np.zeros((it, 3, 3), np.float32),
                 it_F=np.zeros((it, 3, 3), np.float32))
        return p1, p2, m, sets, o

    def run(self, prep, which=3):
        """which: 1 FindHomography, 2 FindFundamental, 3 both (ctypes releases the GIL: two threads can run one each)"""
        p1, p2, m, sets, o = prep
        SH, SF, bh, bf = C.c_float(0), C.c_float(0), C.c_int(-1), C.c_int(-1)
        self.L.tvr_ransac(_p(p1), len(p1), _p(p2), len(p2), _p(m), len(m), _p(sets), len(sets), self.sigma, self.th_score, self.th_f, which,
                          _p(o["H21"]), C.byref(SH), C.byref(bh), _p(o["inliers_h"]), _p(o["F21"]), C.byref(SF), C.byref(bf), _p(o["inliers_f"]),
                          _p(o["it_score_h"]), _p(o["it_score_f"]), _p(o["it_H"]), _p(o["it_F"]))
        return SH.value, SF.value, bh.value, bf.value

    def find_homography_fundamental(self, kps1, kps2, matches12, sets, aids=False):
        prep = self.prepare(kps1, kps2, matches12, sets)
        SH, SF, bh, bf = self.run(prep)
        o = prep[4]
        if not aids:
            for k in ("it_score_h", "it_score_f", "it_H", "it_F"):
                o.pop(k)
        o.update(SH=np.float32(SH), SF=np.float32(SF), best_it_h=bh, best_it_f=bf)
        return o

    def check_rt(self, kps1, kps2, matches12, inliers, poses, th2=None, min_parallax_crt=None, min_triangulated=None, want_cos_all=False):
        p1, p2 = _pts(kps1), _pts(kps2)
        m = np.ascontiguousarray(matches12, np.int32)
        inl = np.ascontiguousarray(inliers, np.uint8); poses = np.ascontiguousarray(poses, np.float32)
        assert inl.shape == (len(m),) and poses.ndim == 2 and poses.shape[1] == 27
        Kp, n1, N = len(poses), len(p1), len(m)
        th2 = 4.0 * self.sigma * self.sigma if th2 is None else th2
        mp = self.min_parallax_crt if min_parallax_crt is None else float(np.float32(min_parallax_crt))
        mt = self.min_triangulated if min_triangulated is None else int(min_triangulated)
        o = dict(n_good=np.zeros(Kp, np.int32), good=np.zeros((Kp, n1), np.uint8), p3d=np.zeros((Kp, n1, 3), np.float32), cos_sel=np.zeros(Kp, np.float32))
        ca = np.zeros((Kp, N), np.float32) if want_cos_all else None
        self.L.tvr_check_rt(_p(p1), n1, _p(p2), len(p2), _p(m), N, _p(inl), _p(self.K), th2, mp, mt, _p(poses), Kp,
                            _p(o["n_good"]), _p(o["good"]), _p(o["p3d"]), _p(o["cos_sel"]), _p(ca))
        if want_cos_all:
            o["cos_all"] = ca
        return o
