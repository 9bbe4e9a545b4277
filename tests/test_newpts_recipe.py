"""The caller's recipe above eorb_search_for_triangulation_keyframes (include/eorb_fe.h) with the real triangulation stage in place of
tests/test_kfbatch_recipe.py's made-up rule, on a model map with the oracle's search and the stage's CPU restatement (tests/newpts_ref):
LocalMapping::CreateNewMapPoints searches the neighbours one after another and a successful triangulation takes its pKF1 feature out
of the later searches (AddMapPoint, src/LocalMapping.cc:775); the batch searches every neighbour with the initial elig1 and hands all
rows to one stage call, which resolves the claim itself.  Both must create the same points, neighbour by neighbour.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newpts_ref as nr                             # noqa: E402
from newpts_ref import scenes                       # noqa: E402

K = 4


def _search(oracle, s, k, elig1):
    kf = s["kfs"][k]
    return oracle.search_for_triangulation(s["kps1"], s["desc1"], elig1, s["fv1"], kf["kps"], kf["desc"], kf["elig"], kf["fv"], s["ep"][k], s["F12"][k],
                                           s["scale2"], s["sigma2_2"], False, False)[1]


def _points(r, rows):
    """per neighbour, the points the caller creates: (idx1, idx2, the bytes of x3d)"""
    return [[(int(i), int(rows[k][i]), r["x3d"][k, i].tobytes()) for i in np.nonzero(r["status"][k] == nr.S["new"])[0]] for k in range(len(rows))]


def _sequential(oracle, S):
    """the reference's loop: search neighbour k with elig1 as it stands, triangulate its matches, AddMapPoint"""
    s = S[0]
    elig1 = s["elig1"].copy()
    made = []
    for k in range(K):
        m = _search(oracle, s, k, elig1)
        r = nr.loop(scenes.scene_of_search(*S, m[None], "pinhole", ks=[k]))
        new = _points(r, [m])[0]
        for i, _, _ in new:
            elig1[i] &= 0xFE                       # mpCurrentKeyFrame->AddMapPoint(pMP, idx1): GetMapPoint(idx1) is set from here on
        made.append(new)
    return made


def _batched(oracle, S):
    """the recipe: every neighbour searched with the initial elig1 (one batch call), all rows to one stage call"""
    s = S[0]
    rows = np.stack([_search(oracle, s, k, s["elig1"]) for k in range(K)])
    r = nr.loop(scenes.scene_of_search(*S, rows, "pinhole"))
    return _points(r, rows), r, rows


def test_search_then_stage_reproduces_the_sequential_loop(oracle):
    S = scenes.search_scene("pinhole", K)
    seq = _sequential(oracle, S)
    bat, r, rows = _batched(oracle, S)
    assert seq == bat
    counts = np.bincount(r["status"].ravel(), minlength=len(nr.STATUS))
    print("points per neighbour", [len(p) for p in seq], dict(zip(nr.STATUS, counts.tolist())))
    # the claim bites, and the stage rejects matches for its own reasons: neither half of the recipe is idle on this map
    assert counts[nr.S["claimed"]] >= 10 and len(seq[0]) >= 20 and all(len(p) >= 1 for p in seq)
    assert sum(counts[nr.S[n]] for n in ("parallax", "z1", "z2", "reproj1", "reproj2", "scale")) >= 10
    assert r["n_new"].tolist() == [len(p) for p in seq]
