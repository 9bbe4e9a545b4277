"""The scenes and references that tests/test_kfside_mixed_ref.py (no GPU) and tests/test_gpu_kfside_mixed.py share: the mixed ORB +
AKAZE neighbourhood of eorb_slam_amd.synth, projected and searched once by the CPU restatement (tests/kfside_mixed_ref)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfside_mixed_ref as mref                     # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

W, H = 346, 260
TH_LOW = 50
SEED, M, N = 43, 1000, 1000                         # the single-keyframe scene of the GPU tests
GATES = ("none", "mono", "stereo")
BATCH = {1: ((1000,), ("mixed",)),
         3: ((0, 777, 513), ("mixed", "orb", "akaze")),
         8: ((1000, 0, 700, 999, 65, 1, 513, 640), ("mixed", "mixed", "orb", "mixed", "akaze", "mixed", "mixed", "mixed"))}


@functools.lru_cache(None)
def scene(seed=SEED, K=1, m=M, n_kps=(N,), kinds=None):
    return synth.mixed_keyframe_neighbourhood(seed, K, m, n_kps=list(n_kps), kinds=kinds)


def geom(sc):
    return sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"]


@functools.lru_cache(None)
def projection(th, seed=SEED, K=1, m=M, n_kps=(N,), kinds=None, skip_key=None):
    """the restatement's mode D over the scene's keyframes -> list per keyframe of dict(valid, uv, radius, level, q_ur, dist3d, reason)"""
    sc = scene(seed, K, m, n_kps, kinds)
    p = mref.keyframe_side([mref.view(**kw) for kw in sc["views"]], *geom(sc), th, mp_is_orb=sc["mp_is_orb"], skip=skip_of(skip_key, K, m))
    for a in p.values():
        a.setflags(write=False)
    return [{n: p[n][k * m:(k + 1) * m] for n in p} for k in range(K)]


def skip_of(key, K, m):
    """the skip flags of a test, by name, so that the cached projection can be keyed on them"""
    if key is None:
        return None
    if key == "every13":
        return np.tile((np.arange(m) % 13 == 12).astype(np.uint8), K)
    if key == "random10":
        return (np.random.default_rng(5).random(K * m) < 0.1).astype(np.uint8)
    raise KeyError(key)


def frame(oracle, sc, k, n=None):
    """the oracle Frame (grid, keypoints, descriptors) of keyframe k, or of its first n rows; None when empty"""
    kps, desc = sc["kps"][k][:n], sc["desc"][k][:n]
    return oracle.Frame(kps, desc, W, H) if len(kps) else None


def gate_kw(sc, k, gate, n=None):
    """the keyword arguments that select a reprojection gate, for the restatement's search and the product's wrappers alike"""
    kw = dict(kp_is_orb=sc["kp_is_orb"][k][:n], mp_is_orb=sc["mp_is_orb"])
    if gate != "none":
        kw["kp_inv_sigma2"] = sc["kp_inv_sigma2"][k][:n]
    if gate == "stereo":
        kw["uright"] = sc["uright"][k][:n]
    return kw


def search(oracle, sc, k, p, gate, n=None, m=None, **extra):
    """the restatement's search of the first m projected points in the first n rows of keyframe k"""
    mref.use_oracle(oracle)
    kw = gate_kw(sc, k, gate, n)
    kw["mp_is_orb"] = kw["mp_is_orb"][:m]
    kw.update(extra)
    return mref.search(frame(oracle, sc, k, n), {a: p[a][:m] for a in p}, sc["mp_desc"][:m], **kw)
