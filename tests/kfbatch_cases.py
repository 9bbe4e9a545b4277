"""Cases of the batched node-walk matchers (the *_keyframes entry points of include/eorb_fe.h), shared by the GPU tests, the C++ mirror and
the recipe test.  Each case is a synth neighbourhood plus, per keyframe k, the oracle's single-pair result on pair k: the expected row.
The oracle rows are computed once per (case, options) and cached; callers must not modify them."""
import functools

import numpy as np

from eorb_slam_amd import synth

ANGLE_STEP = 50.0            # the neighbours' orientations differ by k * 50 degrees: every pair keeps other rotation bins


def _oracle():
    from oracle import oracle_py
    oracle_py.build()
    return oracle_py


@functools.lru_cache(maxsize=None)
def tri_scene(kind, K=4):
    """kind: 'pinhole' (npts 250, nnodes 10), 'pinhole_small' (npts 120, nnodes 6: about 110 rows), 'kb8' (monocular KannalaBrandt8),
    'twocam' (two-camera keyframes, about 510 rows)"""
    if kind == "pinhole":
        return synth.triangulation_neighbourhood(101, K, pinhole=True, angle_step=ANGLE_STEP)
    if kind == "pinhole_small":
        return synth.triangulation_neighbourhood(102, K, pinhole=True, npts=120, ndistract=30, nties=8, nnodes=6, angle_step=ANGLE_STEP)
    if kind == "kb8":
        return synth.triangulation_neighbourhood(103, K, angle_step=ANGLE_STEP)
    if kind == "twocam":
        return synth.triangulation_neighbourhood(104, K, twocam=True, angle_step=ANGLE_STEP)
    raise KeyError(kind)


def tri_set(s, ks=None, elig=None):
    """the (kps, desc, flag, fv) list of a scene's neighbours ks (default all)"""
    ks = range(len(s["kfs"])) if ks is None else ks
    return [(s["kfs"][k]["kps"], s["kfs"][k]["desc"], s["kfs"][k]["elig"] if elig is None else elig[k], s["kfs"][k]["fv"]) for k in ks]


@functools.lru_cache(maxsize=None)
def tri_rows(kind, K=4, coarse=False, ori=False):
    """oracle rows of a triangulation scene: (nmatches[K], match12 K x n1)"""
    o = _oracle()
    s = tri_scene(kind, K)
    e1 = s["elig1"]
    nm, rows = [], []
    for k, kf in enumerate(s["kfs"]):
        e2 = kf["elig"]
        if "F12" in s:
            n, m = o.search_for_triangulation(s["kps1"], s["desc1"], e1, s["fv1"], kf["kps"], kf["desc"], e2, kf["fv"], s["ep"][k], s["F12"][k],
                                              s["scale2"], s["sigma2_2"], coarse, ori)
        else:
            n, m = o.search_for_triangulation_kb8(s["kps1"], s["nleft1"], s["desc1"], e1, s["fv1"], kf["kps"], kf["nleft"], kf["desc"], e2, kf["fv"],
                                                  s["cams1"], s["cams2"], s["Rt"][k], s["ep"][k], s["scale2"], s["sigma2_1"], s["sigma2_2"],
                                                  coarse, ori)
        nm.append(n); rows.append(m)
    return np.array(nm, np.int32), np.stack(rows)


# per-node caps of the BoW scenes' keyframes (synth.cap_nodes): with three scene nodes every uncapped node holds 75-91 features, past
# the 64-feature limit of the walk's register path; the capped ones sit at and under it.  (Node 1, the "stray" node, comes first.)
BOW_CAPS = [[None, None, 40, 64], [None, 65, None, 30], None, [None, 30, 30, None]]


@functools.lru_cache(maxsize=None)
def bow_scene(kind, K=4):
    """kind: 'small' (nnodes 10: nodes of 28-35 features, the register path), 'big' (nnodes 3 with BOW_CAPS: both paths in one batch)"""
    if kind == "small":
        return synth.bow_neighbourhood(201, K, nnodes=10, angle_step=ANGLE_STEP)
    if kind == "big":
        return synth.bow_neighbourhood(202, K, nnodes=3, caps=BOW_CAPS[:K] + [None] * max(0, K - 4), angle_step=ANGLE_STEP)
    raise KeyError(kind)


def bow_set(s, ks=None):
    ks = range(len(s["kfs"])) if ks is None else ks
    return [(s["kfs"][k]["kps"], s["kfs"][k]["desc"], s["kfs"][k]["has_mp"], s["kfs"][k]["fv"]) for k in ks]


@functools.lru_cache(maxsize=None)
def bow_rows(kind, K=4, kf_kf=False, ratio=0.7, ori=True):
    """oracle rows: kf_kf False: SearchByBoW(pKF_k, F) -> match_f K x n_f; True: SearchByBoW(pKF1, pKF2_k) -> match12 K x n1"""
    o = _oracle()
    s = bow_scene(kind, K)
    nm, rows = [], []
    for kf in s["kfs"]:
        if kf_kf:
            n, m = o.search_by_bow_kf(s["kps"], s["desc"], s["has_mp"], s["fv"], kf["kps"], kf["desc"], kf["has_mp"], kf["fv"], ratio, ori)
        else:
            n, m = o.search_by_bow(kf["kps"], kf["desc"], kf["has_mp"], kf["fv"], s["kps"], s["desc"], s["fv"], ratio, ori)
        nm.append(n); rows.append(m)
    return np.array(nm, np.int32), np.stack(rows)


def node_sizes(fv):
    return np.diff(fv[1])


def kept_bins(a1, a2):
    """the rotation bins of matched orientation pairs (ORBmatcher.cc: rot = a1 - a2 (+360), bin = round(rot / 12) mod 30), as a set"""
    rot = np.asarray(a1, np.float32) - np.asarray(a2, np.float32)
    rot = np.where(rot < 0, rot + np.float32(360), rot)
    return set((np.round(rot * np.float32(1.0 / 12.0)).astype(int) % 30).tolist())
