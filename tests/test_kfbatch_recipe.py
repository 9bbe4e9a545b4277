"""The caller's recipe above eorb_search_for_triangulation_keyframes (include/eorb_fe.h), on a model map with the oracle standing in for
both sides: LocalMapping::CreateNewMapPoints searches the neighbours one after another and a successful triangulation takes its pKF1
feature out of the later searches (AddMapPoint, src/LocalMapping.cc:775); the batch searches every neighbour with the initial elig1 and
the caller drops a pair whose idx1 got a map point meanwhile.  Both must give the same pair lists per neighbour.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfbatch_cases as kc                          # noqa: E402

K = 4


def _search(oracle, s, k, elig1, ori=False):
    kf = s["kfs"][k]
    return oracle.search_for_triangulation(s["kps1"], s["desc1"], elig1, s["fv1"], kf["kps"], kf["desc"], kf["elig"], kf["fv"], s["ep"][k], s["F12"][k],
                                           s["scale2"], s["sigma2_2"], False, ori)[1]


def _triangulates(k, idx1, idx2):
    """the model's deterministic 'triangulation succeeded' rule (the parallax, depth and reprojection tests of :530-770)"""
    return (7 * idx1 + 3 * idx2 + k) % 5 != 0


def _sequential(oracle, s, ori=False):
    elig1 = s["elig1"].copy()
    pairs, gone = [], []
    for k in range(K):
        gone.append(int(((s["elig1"] & 1) != 0).sum() - ((elig1 & 1) != 0).sum()))
        m = _search(oracle, s, k, elig1, ori)
        made = [(int(i), int(m[i])) for i in np.nonzero(m >= 0)[0] if _triangulates(k, int(i), int(m[i]))]
        for i, _ in made:
            elig1[i] &= 0xFE                       # mpCurrentKeyFrame->AddMapPoint(pMP, idx1): GetMapPoint(idx1) is set from here on
        pairs.append(made)
    return pairs, gone


def _batched(oracle, s, ori=False):
    rows = [_search(oracle, s, k, s["elig1"], ori) for k in range(K)]          # what one batch call returns
    has_mp = np.zeros(len(s["kps1"]), bool)
    pairs = []
    for k in range(K):
        made = []
        for i in np.nonzero(rows[k] >= 0)[0]:
            if has_mp[i]:
                continue                           # set by an earlier neighbour of this pass
            if _triangulates(k, int(i), int(rows[k][i])):
                made.append((int(i), int(rows[k][i])))
        for i, _ in made:
            has_mp[i] = True
        pairs.append(made)
    return pairs, rows


def test_recipe_reproduces_the_sequential_loop(oracle):
    s = kc.tri_scene("pinhole", K)
    seq, gone = _sequential(oracle, s)
    bat, rows = _batched(oracle, s)
    assert seq == bat
    n_elig = int(((s["elig1"] & 1) != 0).sum())
    print("eligible", n_elig, "taken before each neighbour", gone, "pairs", [len(p) for p in seq])
    assert gone[-1] * 10 >= n_elig, (gone, n_elig)                     # the filter bites: a tenth of pKF1 is gone before the last neighbour
    dropped = [sum(1 for i in np.nonzero(rows[k] >= 0)[0] if any(i == j for q in bat[:k] for j, _ in q)) for k in range(K)]     # by the filter
    assert all(d > 0 for d in dropped[1:]) and dropped[0] == 0 and len(seq[0]) >= 20 and all(len(p) > 0 for p in seq)


def test_with_the_rotation_check_the_batch_is_k_independent_calls(oracle):
    """checkOri set: a row is the single call with the initial elig1, which is not the reference's sequence once elig1 has changed, as
    the header says.  On this scene the two do differ after the first neighbour, so the statement is not vacuous."""
    s = kc.tri_scene("pinhole", K)
    seq, _ = _sequential(oracle, s, True)
    bat, _ = _batched(oracle, s, True)
    print("pairs with checkOri: sequential", [len(p) for p in seq], "recipe", [len(p) for p in bat])
    assert seq[0] == bat[0] and seq != bat
