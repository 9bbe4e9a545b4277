"""The two-camera oracle (tests/twocam/orc_twocam.c) behind ctypes, and the inputs the two-camera tests share.

build(dirpath) compiles orc_twocam.c with oracle/Makefile's parity flags into dirpath (a pytest temporary directory), linked
against oracle/_build/liboracle.so (built by oracle_py.build()) for orc_descriptor_distance, orc_three_maxima and orc_bf_knn2."""
import ctypes as C
import os
import subprocess

import numpy as np

from eorb_slam_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
KP = synth.KP_DTYPE
CFLAGS = ["-O2", "-std=gnu11", "-fPIC", "-shared", "-Wall", "-ffp-contract=off", "-fno-fast-math"]   # oracle/Makefile


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Bounds(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("minX", "minY", "maxX", "maxY", "invW", "invH")]


def bounds(W, H):
    """ComputeImageBounds without distortion (Frame.cc:862-866) and the grid pitch (:1145-1148)"""
    return Bounds(0.0, 0.0, float(W), float(H), np.float32(64) / np.float32(W), np.float32(48) / np.float32(H))


class TwoCamOracle:
    def __init__(self, dirpath, oracle_py):
        oracle_py.build()
        libdir = os.path.join(ROOT, "oracle", "_build")
        out = os.path.join(str(dirpath), "liborc_twocam.so")
        cc = os.environ.get("CC", "gcc")
        subprocess.run([cc] + CFLAGS + ["-o", out, os.path.join(HERE, "orc_twocam.c"), os.path.join(libdir, "liboracle.so"),
                                        "-Wl,-rpath," + libdir, "-lm"], check=True)
        self.L = L = C.CDLL(out)
        vp, ci, cf = C.c_void_p, C.c_int, C.c_float
        L.orc_tc_fisheye_matches.restype = ci
        L.orc_tc_fisheye_matches.argtypes = [vp, ci, ci, vp, ci, ci, vp, vp]
        L.orc_tc_search_by_projection_map.restype = ci
        L.orc_tc_search_by_projection_map.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp, ci] + [vp] * 12 + [vp, cf, cf]
        L.orc_tc_search_by_projection_last.restype = ci
        L.orc_tc_search_by_projection_last.argtypes = [vp, ci, ci, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, cf, ci, ci]
        L.orc_tc_search_by_bow.restype = ci
        L.orc_tc_search_by_bow.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, ci, ci, vp, vp, vp, vp, ci, vp, cf, ci]

    def fisheye_matches(self, descL, monoLeft, descR, monoRight):
        dL = np.ascontiguousarray(descL, np.uint8); dR = np.ascontiguousarray(descR, np.uint8)
        cand = np.zeros(len(dL), np.int32); d2 = np.zeros((len(dL), 2), np.int32)
        n = self.L.orc_tc_fisheye_matches(_p(dL), len(dL), monoLeft, _p(dR), len(dR), monoRight, _p(cand), _p(d2))
        return n, cand, d2

    def map(self, kps, nL, desc, gb, l2r, r2l, left, right, mp_desc, mp_obs, frame_mp, th, nnratio):
        kps = np.ascontiguousarray(kps, KP); desc = np.ascontiguousarray(desc, np.uint8)
        l2r = np.ascontiguousarray(l2r, np.int32); r2l = np.ascontiguousarray(r2l, np.int32)
        cam = [[np.ascontiguousarray(a, t) for a, t in zip(c, (np.uint8, np.float32, np.int32, np.float32, np.float32))] for c in (left, right)]
        mp_desc = np.ascontiguousarray(mp_desc, np.uint8); mp_obs = np.ascontiguousarray(mp_obs, np.uint8)
        fm = np.ascontiguousarray(frame_mp, np.int32).copy()
        n = self.L.orc_tc_search_by_projection_map(_p(kps), nL, len(kps) - nL, _p(desc), 32, C.byref(gb), _p(l2r), _p(r2l), len(mp_obs),
                                                   *[_p(a) for a in cam[0]], *[_p(a) for a in cam[1]], _p(mp_desc), _p(mp_obs), _p(fm),
                                                   float(th), float(nnratio))
        return n, fm

    def last(self, kps, nL, desc, gb, last_kps, valid, uv, uv_r, mp_desc, mp_obs, cur_mp, th, level_scale, mode, checkOri):
        kps = np.ascontiguousarray(kps, KP); desc = np.ascontiguousarray(desc, np.uint8); lk = np.ascontiguousarray(last_kps, KP)
        valid = np.ascontiguousarray(valid, np.uint8); uv = np.ascontiguousarray(uv, np.float32); uv_r = np.ascontiguousarray(uv_r, np.float32)
        mp_desc = np.ascontiguousarray(mp_desc, np.uint8); mp_obs = np.ascontiguousarray(mp_obs, np.uint8)
        ls = np.ascontiguousarray(level_scale, np.float32)
        cm = np.ascontiguousarray(cur_mp, np.int32).copy()
        n = self.L.orc_tc_search_by_projection_last(_p(kps), nL, len(kps) - nL, _p(desc), 32, C.byref(gb), _p(lk), len(lk), _p(valid), _p(uv),
                                                    _p(uv_r), _p(mp_desc), _p(mp_obs), _p(ls), _p(cm), float(th), int(mode), int(checkOri))
        return n, cm

    def bow(self, kf_kps, kf_desc, kf_has_mp, kf_fv, f_kps, nL, f_desc, f_fv, nnratio, checkOri):
        kf_kps = np.ascontiguousarray(kf_kps, KP); f_kps = np.ascontiguousarray(f_kps, KP)
        kf_desc = np.ascontiguousarray(kf_desc, np.uint8); f_desc = np.ascontiguousarray(f_desc, np.uint8)
        hm = np.ascontiguousarray(kf_has_mp, np.uint8)
        kn, ko, ki = [np.ascontiguousarray(a, t) for a, t in zip(kf_fv, (np.uint32, np.int32, np.int32))]
        fn, fo, fi = [np.ascontiguousarray(a, t) for a, t in zip(f_fv, (np.uint32, np.int32, np.int32))]
        m = np.full(len(f_kps), -1, np.int32)
        n = self.L.orc_tc_search_by_bow(_p(kf_kps), _p(kf_desc), _p(hm), _p(kn), _p(ko), _p(ki), len(kn), _p(f_kps), len(f_kps), int(nL),
                                        _p(f_desc), _p(fn), _p(fo), _p(fi), len(fn), _p(m), float(nnratio), int(checkOri))
        return n, m


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
def image_pair(W=512, H=512, seed=5, shift=(2, -7)):
    """a textured image and the same scene shifted: a stand-in for a fisheye stereo pair (TUM-VI 512 x 512)"""
    img = synth.texture_image(W, H, seed=seed)
    return img, np.roll(img, shift, axis=(0, 1))


def feature_vector_of(node_of, rng):
    """DBoW2::FeatureVector as CSR from a node id per feature (vector order inside a node: shuffled insertion order)"""
    ids = np.unique(node_of)
    off = [0]; idx = []
    for nid in ids:
        m = np.nonzero(node_of == nid)[0]; rng.shuffle(m); idx.extend(m.tolist()); off.append(len(idx))
    return ids.astype(np.uint32), np.array(off, np.int32), np.array(idx, np.int32)


def frame_links(nL, nR, rng, frac=0.4):
    """mvLeftToRightMatch / mvRightToLeftMatch: a random partial one-to-one pairing"""
    l2r = np.full(nL, -1, np.int32); r2l = np.full(nR, -1, np.int32)
    k = int(min(nL, nR) * frac)
    if k:
        li = rng.choice(nL, k, replace=False); ri = rng.choice(nR, k, replace=False)
        l2r[li] = ri; r2l[ri] = li
    return l2r, r2l


def map_inputs(kps, nL, scale_factors, rng, M=None, src=None):
    """map points near the frame's keypoints: (left, right, mp_desc, mp_obs); src = (kps, desc) the map points are drawn from"""
    sk, sd = src
    M = len(sk) if M is None else M
    pick = rng.integers(0, len(sk), M)
    k = sk[pick]
    nl = len(scale_factors)
    cams = []
    for cam in range(2):
        iv = (rng.uniform(size=M) < (0.9 if cam == 0 else 0.7)).astype(np.uint8)
        pxy = np.stack([k["x"] + rng.normal(0, 1.0, M), k["y"] + rng.normal(0, 1.0, M)], axis=1).astype(np.float32)
        if cam:
            pxy[:, 0] += rng.normal(-6.0, 1.0, M)
        lv = np.clip(k["octave"] + rng.integers(-1, 2, M), 0, nl - 1).astype(np.int32)
        if cam:
            lv[rng.uniform(size=M) < 0.1] = -1
        vc = rng.uniform(0.99, 1.0, M).astype(np.float32)
        ls = np.asarray(scale_factors, np.float32)[np.clip(lv, 0, nl - 1)]
        cams.append((iv, pxy, lv, vc, ls))
    mp_obs = (rng.uniform(size=M) < 0.6).astype(np.uint8)
    return cams[0], cams[1], sd[pick].copy(), mp_obs
