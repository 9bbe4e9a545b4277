"""Loader of the CPU restatement of TwoViewReconstruction::Reconstruct (reconstruct_ref.c, beside this file, which includes twoview_ref.c
and eorb_slam_amd/csrc/twoview_core.h): compiled with the host C compiler into a temporary directory when first used, strict IEEE, as the
loader in __init__.py does.  Test infrastructure: nothing under eorb_slam_amd/ imports it."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from . import CFLAGS, _p, _pts

_HERE = os.path.dirname(os.path.abspath(__file__))
FORM_STOCK, FORM_INFO = 0, 1


class ReconParams(C.Structure):
    """eorb_tvr_recon_params"""
    _fields_ = [("sigma", C.c_float), ("th_score", C.c_float), ("th_f", C.c_float), ("th_hf_ratio", C.c_float), ("min_parallax", C.c_float),
                ("min_parallax_crt", C.c_float), ("min_triangulated", C.c_int), ("th_min_good_r", C.c_float), ("th_max_good_r_f", C.c_float),
                ("th_max_good_r_h", C.c_float), ("th_rd_homo", C.c_float), ("form", C.c_int)]


class ReconResult(C.Structure):
    """eorb_tvr_recon_result"""
    _fields_ = [("ok", C.c_int32), ("stage", C.c_int32), ("is_homography", C.c_int32), ("SH", C.c_float), ("SF", C.c_float), ("RH", C.c_float),
                ("best_it_h", C.c_int32), ("best_it_f", C.c_int32), ("H21", C.c_float * 9), ("F21", C.c_float * 9), ("n_inliers", C.c_int32),
                ("n_min_good", C.c_int32), ("n_similar", C.c_int32), ("n_hyp", C.c_int32), ("hyp_good", C.c_int32 * 8),
                ("hyp_parallax", C.c_float * 8), ("info_good", C.c_int32 * 8), ("hyp_best", C.c_int32), ("hyp_second", C.c_int32),
                ("best_good", C.c_int32), ("second_good", C.c_int32), ("best_parallax", C.c_float), ("second_parallax", C.c_float)]


RESULT_FIELDS = [f[0] for f in ReconResult._fields_]


def params(form=FORM_STOCK, sigma=1.0, th_score=5.991, th_f=3.841, th_hf_ratio=0.45, min_parallax=1.0, min_parallax_crt=0.99998,
           min_triangulated=50, th_min_good_r=0.9, th_max_good_r_f=0.7, th_max_good_r_h=0.75, th_rd_homo=1.00001, cls=ReconParams):
    """the defaults of Params2VR; cls: this module's structure or eorb_slam_amd._lib's"""
    return cls(sigma, th_score, th_f, th_hf_ratio, min_parallax, float(np.float32(min_parallax_crt)), int(min_triangulated), th_min_good_r,
               th_max_good_r_f, th_max_good_r_h, float(np.float32(th_rd_homo)), int(form))


def result_dict(r):
    """a ReconResult (of either module) -> dict of numpy values, the arrays copied"""
    o = {}
    for name, typ in r._fields_:
        v = getattr(r, name)
        if hasattr(v, "__len__"):
            o[name] = np.array(v[:], np.float32 if typ._type_ is C.c_float else np.int32)
        else:
            o[name] = np.float32(v) if typ is C.c_float else int(v)
    for k in ("H21", "F21"):
        o[k] = o[k].reshape(3, 3)
    return o


_libs = {}


def lib(timing=False):
    if timing in _libs:
        return _libs[timing]
    tmp = tempfile.mkdtemp(prefix="twoview_recon_ref_")
    atexit.register(shutil.rmtree, tmp, True)
    so = os.path.join(tmp, "libreconstruct_ref.so")
    flags = (["-O3", "-march=native"] + CFLAGS[1:]) if timing else CFLAGS
    subprocess.check_call([os.environ.get("CC", "gcc")] + flags + [os.path.join(_HERE, "reconstruct_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.tvr_acos.restype = C.c_double; L.tvr_acos.argtypes = [C.c_double]
    L.tvr_parallax.restype = cf; L.tvr_parallax.argtypes = [ci, cf]
    L.tvr_hypotheses_f.restype = None; L.tvr_hypotheses_f.argtypes = [vp, vp, vp]
    L.tvr_hypotheses_h.restype = ci; L.tvr_hypotheses_h.argtypes = [vp, vp, cf, vp]
    L.tvr_decide.restype = ci
    L.tvr_decide.argtypes = [cf, cf, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    L.tvr_finish.restype = None
    L.tvr_finish.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tvr_reconstruct.restype = ci
    L.tvr_reconstruct.argtypes = [vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    _libs[timing] = L
    return L


def acos(x):
    return lib().tvr_acos(float(x))


def parallax(n_good, cos_sel):
    return np.float32(lib().tvr_parallax(int(n_good), float(np.float32(cos_sel))))


def hypotheses_f(K, F21):
    """the 4 eorb_tvr_pose records of ReconstructF -> [4, 27] float32"""
    K = np.ascontiguousarray(K, np.float32); F21 = np.ascontiguousarray(F21, np.float32); po = np.zeros((4, 27), np.float32)
    lib().tvr_hypotheses_f(_p(K), _p(F21), _p(po))
    return po


def hypotheses_h(K, H21, th_rd_homo=1.00001):
    """the 8 records of ReconstructH -> [8, 27] float32, or None when the d1/d2, d2/d3 test leaves"""
    K = np.ascontiguousarray(K, np.float32); H21 = np.ascontiguousarray(H21, np.float32); po = np.zeros((8, 27), np.float32)
    return po if lib().tvr_hypotheses_h(_p(K), _p(H21), float(np.float32(th_rd_homo)), _p(po)) else None


def outputs(n1, N):
    return dict(R21=np.zeros((2, 3, 3), np.float32), t21=np.zeros((2, 3), np.float32), p3d=np.zeros((2, n1, 3), np.float32),
                triangulated=np.zeros((2, n1), np.uint8), trans_inliers=np.zeros(N, np.uint8), hyp_poses=np.zeros((8, 27), np.float32))


def decide(K, ransac, par):
    """Reconstruct between its stages, from a find_homography_fundamental result dict -> (ReconResult, poses [8, 27], sel_inliers [N],
    trans_inliers [N])"""
    K = np.ascontiguousarray(K, np.float32)
    N = len(ransac["inliers_h"])
    r = ReconResult(); po = np.zeros((8, 27), np.float32); sel = np.zeros(N, np.uint8); ti = np.zeros(N, np.uint8)
    H = np.ascontiguousarray(ransac["H21"], np.float32); F = np.ascontiguousarray(ransac["F21"], np.float32)
    ih = np.ascontiguousarray(ransac["inliers_h"], np.uint8); jf = np.ascontiguousarray(ransac["inliers_f"], np.uint8)
    lib().tvr_decide(float(ransac["SH"]), float(ransac["SF"]), int(ransac["best_it_h"]), int(ransac["best_it_f"]), _p(H), _p(F), _p(ih), _p(jf), N,
                     _p(K), C.addressof(par), C.addressof(r), _p(po), _p(sel), _p(ti))
    return r, po, sel, ti


def finish(par, r, poses, n1, rt):
    """Reconstruct after CheckRT, from a check_rt result dict (None when stage < 2) -> dict(R21, t21, p3d, triangulated); r is completed"""
    o = outputs(n1, 1)
    z = rt or dict(n_good=np.zeros(8, np.int32), cos_sel=np.zeros(8, np.float32), good=np.zeros((8, n1), np.uint8), p3d=np.zeros((8, n1, 3), np.float32))
    ng = np.ascontiguousarray(z["n_good"], np.int32); cs = np.ascontiguousarray(z["cos_sel"], np.float32)
    g = np.ascontiguousarray(z["good"], np.uint8); p3 = np.ascontiguousarray(z["p3d"], np.float32)
    lib().tvr_finish(C.addressof(par), C.addressof(r), _p(np.ascontiguousarray(poses, np.float32)), n1, _p(ng), _p(cs), _p(g), _p(p3),
                     _p(o["R21"]), _p(o["t21"]), _p(o["p3d"]), _p(o["triangulated"]))
    return {k: o[k] for k in ("R21", "t21", "p3d", "triangulated")}


def reconstruct(K, kps1, kps2, matches12, sets, par, timing=False):
    """tvr_reconstruct -> dict of the result fields and the output arrays (the names of eorb_two_view_reconstruct)"""
    K = np.ascontiguousarray(np.asarray(K, np.float32).reshape(3, 3))
    p1, p2 = _pts(kps1), _pts(kps2)
    m = np.ascontiguousarray(matches12, np.int32); sets = np.ascontiguousarray(sets, np.int32)
    assert m.ndim == 2 and m.shape[1] == 2 and sets.ndim == 2 and sets.shape[1] == 8
    r = ReconResult(); o = outputs(len(p1), len(m))
    lib(timing).tvr_reconstruct(_p(p1), len(p1), _p(p2), len(p2), _p(m), len(m), _p(sets), len(sets), _p(K), C.addressof(par), C.addressof(r),
                                _p(o["R21"]), _p(o["t21"]), _p(o["p3d"]), _p(o["triangulated"]), _p(o["trans_inliers"]), _p(o["hyp_poses"]))
    o.update(result_dict(r))
    return o
