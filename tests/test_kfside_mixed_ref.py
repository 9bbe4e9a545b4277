"""The CPU restatement of MixedMatcher's KeyFrame-side matchers (tests/kfside_mixed_ref): hand-derived known answers of the type gate,
the keypoint level and the per-keypoint sigma, its agreement with the ORB restatements where nothing is mixed, the conditions that the
scene of the GPU tests has to meet (asserted on the restatement alone, so that the GPU tests cannot pass on empty sets), the batched
Fuse adapter on a model map with mixed data, and the new exports.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfside_ref                                   # noqa: E402
import kfside_mixed_cases as cases                  # noqa: E402
import kfside_mixed_ref as mref                     # noqa: E402
from test_kfside_ref import _Map, TH_LOW            # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402
KP_DTYPE = synth.KP_DTYPE

F32 = np.float32
W, H = cases.W, cases.H
SF, LOGS = synth.scale_tables(8, 1.2)
AK_SF, AK_LOGS = synth.akaze_tables()
NEW_EXPORTS = ("eorb_kf_radius_match_mixed", "eorb_project_keyframe_side_mixed", "eorb_fuse_pose_mixed",
               "eorb_search_by_projection_kf_scw_mixed", "eorb_fuse_keyframes_mixed")


@pytest.fixture(scope="module")
def ref(oracle):
    return mref.use_oracle(oracle)


def _kp(x, y, octave, class_id=-1):
    k = np.zeros(1, KP_DTYPE)
    k["x"], k["y"], k["octave"], k["class_id"], k["size"] = x, y, octave, class_id, 31.0
    return k


def _one(oracle, ref, kp, desc, level, q_desc, uv=(100.0, 100.0), radius=6.0, **kw):
    """one projected point at uv against a keyframe of the given rows -> (best_idx, best_dist)"""
    Fr = oracle.Frame(kp, desc, W, H)
    p = dict(valid=np.ones(1, np.uint8), uv=np.array([uv], F32), radius=np.array([radius], F32), level=np.array([level], np.int32),
             q_ur=np.zeros(1, F32))
    bi, bd = ref.search(Fr, p, q_desc, **kw)
    return int(bi[0]), int(bd[0])


# ---- known answers ------------------------------------------------------------------------------------------------------------------
def test_an_akaze_point_does_not_match_an_orb_row_at_distance_zero(oracle, ref):
    d = synth.random_descriptors(1, seed=1)
    kp = _kp(101.0, 99.0, 2)
    assert _one(oracle, ref, kp, d, 2, d, kp_is_orb=[1], mp_is_orb=[0]) == (-1, 256)
    assert _one(oracle, ref, kp, d, 2, d, kp_is_orb=[1], mp_is_orb=[1]) == (0, 0)           # the same row for an ORB point
    assert _one(oracle, ref, kp, d, 2, d, kp_is_orb=[1], mp_is_orb=[0], wrong=mref.NO_TYPE_GATE) == (0, 0)
    kpa = _kp(101.0, 99.0, 0, class_id=2)                                                   # and the mirror: an AKAZE row, an ORB point
    assert _one(oracle, ref, kpa, d, 2, d, kp_is_orb=[0], mp_is_orb=[1]) == (-1, 256)
    assert _one(oracle, ref, kpa, d, 2, d, kp_is_orb=[0], mp_is_orb=[0]) == (0, 0)


def test_an_akaze_row_is_levelled_by_class_id_not_by_octave(oracle, ref):
    """class_id = 9 is inside the window [8, 9] of a point predicted at level 9; its octave 9 / 4 = 2 is not"""
    d = synth.random_descriptors(1, seed=2)
    kp = _kp(100.5, 100.5, 2, class_id=9)
    kw = dict(kp_is_orb=[0], mp_is_orb=[0])
    assert _one(oracle, ref, kp, d, 9, d, **kw) == (0, 0)
    assert _one(oracle, ref, kp, d, 10, d, **kw) == (0, 0)                                  # 9 = L - 1
    assert _one(oracle, ref, kp, d, 8, d, **kw) == (-1, 256) and _one(oracle, ref, kp, d, 11, d, **kw) == (-1, 256)
    assert _one(oracle, ref, kp, d, 9, d, wrong=mref.LEVEL_FROM_OCTAVE, **kw) == (-1, 256)
    assert _one(oracle, ref, kp, d, 2, d, **kw) == (-1, 256)                                # the octave's own window does not admit it
    assert _one(oracle, ref, kp, d, 2, d, wrong=mref.LEVEL_FROM_OCTAVE, **kw) == (0, 0)
    # an ORB row keeps octave, whatever its class_id holds
    assert _one(oracle, ref, _kp(100.5, 100.5, 2, class_id=9), d, 2, d, kp_is_orb=[1], mp_is_orb=[1]) == (0, 0)


def test_the_reprojection_gate_reads_the_keypoints_own_sigma(oracle, ref):
    """An AKAZE row at class_id 8, octave 2: its own inverse sigma^2 is 1 / 2^(8/4)^2 = 1/16, the ORB table's entry at octave 2 is
    1 / 1.2^4 = 0.482.  With ex = 4, ey = 2: e2 = 20, e2/16 = 1.25 passes 5.99 and 20 * 0.482 = 9.6 fails.  The mirror is an AKAZE row
    at class_id 1, octave 0: its own 1 / 2^(1/2) = 0.707 against the ORB table's 1 at octave 0; e2 = 2.5^2 + 1 = 7.25 fails with
    7.25 (the ORB table's) and passes with 5.13."""
    d = synth.random_descriptors(1, seed=3)
    orb_is2 = (F32(1) / (SF * SF)).astype(F32)
    ak_is2 = (F32(1) / (AK_SF * AK_SF)).astype(F32)
    kp = _kp(96.0, 98.0, 2, class_id=8)
    kw = dict(kp_is_orb=[0], mp_is_orb=[0], orb_inv_sigma2=orb_is2)
    e2 = F32(4) * F32(4) + F32(2) * F32(2)
    assert float(e2 * ak_is2[8]) <= 5.99 < float(e2 * orb_is2[2])
    assert _one(oracle, ref, kp, d, 8, d, kp_inv_sigma2=[ak_is2[8]], **kw) == (0, 0)
    assert _one(oracle, ref, kp, d, 8, d, kp_inv_sigma2=[ak_is2[8]], wrong=mref.ORB_SIGMA_TABLE, **kw) == (-1, 256)
    assert _one(oracle, ref, kp, d, 8, d, kp_inv_sigma2=[orb_is2[2]], **kw) == (-1, 256)   # (the same through the array)
    assert _one(oracle, ref, kp, d, 8, d, **kw) == (0, 0)                                   # no sigma array: no gate
    # the mirror: an ORB row at octave 0 passes only with a table that is not its own
    kpo = _kp(97.5, 99.0, 0)
    e2 = F32(2.5) * F32(2.5) + F32(1) * F32(1)
    assert float(e2 * ak_is2[1]) <= 5.99 < float(e2 * orb_is2[0])
    kwo = dict(kp_is_orb=[1], mp_is_orb=[1])
    assert _one(oracle, ref, kpo, d, 0, d, kp_inv_sigma2=[orb_is2[0]], **kwo) == (-1, 256)
    assert _one(oracle, ref, kpo, d, 0, d, kp_inv_sigma2=[ak_is2[1]], **kwo) == (0, 0)
    # the stereo form: a third term and 7.8
    ur = [50.0]
    p_qur = F32(50.0) + F32(2.0)
    Fr = oracle.Frame(kpo, d, W, H)
    p = dict(valid=np.ones(1, np.uint8), uv=np.array([[100.0, 100.0]], F32), radius=np.array([6.0], F32), level=np.zeros(1, np.int32),
             q_ur=np.array([p_qur], F32))
    e3 = e2 + F32(2) * F32(2)
    assert float(e3 * ak_is2[1]) > 7.8 >= float(e3 * ak_is2[2])
    assert int(ref.search(Fr, p, d, kp_inv_sigma2=[ak_is2[1]], uright=ur, **kwo)[0][0]) == -1
    assert int(ref.search(Fr, p, d, kp_inv_sigma2=[ak_is2[2]], uright=ur, **kwo)[0][0]) == 0
    assert int(ref.search(Fr, p, d, kp_inv_sigma2=[ak_is2[1]], uright=[-1.0], **kwo)[0][0]) == 0      # no right coordinate: 5.99 on two terms


def test_an_akaze_point_takes_the_akaze_pyramid(ref):
    """dist = 2, max_dist = 9: ratio 4.5; ORB level ceil(log 4.5 / log 1.2) = 9 -> 7 (the last of 8), AKAZE level ceil(log 4.5 /
    log 2^(1/4)) = 9 of 16; the radius follows the same table"""
    kw = dict(R=np.eye(3, dtype=F32), t=np.zeros(3, F32), Ow=np.zeros(3, F32), cam=(100.0, 100.0, 100.0, 100.0), bounds=(0.0, 200.0, 0.0, 200.0),
              nlevels=8, log_scale=LOGS, scale_factors=SF)
    P = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 2.0]], F32); Pn = np.array([[0, 0, 1.0]] * 2, F32)
    mixed = ref.view(ak_nlevels=16, ak_log_scale=AK_LOGS, ak_scale_factors=AK_SF, **kw)
    o = ref.keyframe_side(mixed, P, Pn, [0.1, 0.1], [9.0, 9.0], 3.0, mp_is_orb=[1, 0])
    assert o["level"].tolist() == [7, 9] and o["valid"].tolist() == [1, 1]
    assert o["radius"][0] == F32(3.0) * SF[7] and o["radius"][1] == F32(3.0) * AK_SF[9]
    # a view without AKAZE tables serves both from the ORB ones
    o = ref.keyframe_side(ref.view(**kw), P, Pn, [0.1, 0.1], [9.0, 9.0], 3.0, mp_is_orb=[1, 0])
    assert o["level"].tolist() == [7, 7] and o["radius"][1] == F32(3.0) * SF[7]


def test_with_nothing_mixed_it_is_the_orb_restatement(oracle, ref):
    sc = synth.keyframe_neighbourhood(43, 2, 1000, n_kps=[1000, 640])
    g = cases.geom(sc)
    views = [ref.view(**kw) for kw in sc["views"]]
    want = kfside_ref.keyframe_side([kfside_ref.view(**kw) for kw in sc["views"]], *g, 3.0)
    got = ref.keyframe_side(views, *g, 3.0, mp_is_orb=np.ones(1000, np.uint8))
    got_null = ref.keyframe_side(views, *g, 3.0)
    for n in want:
        assert got[n].tobytes() == want[n].tobytes() == got_null[n].tobytes(), n
    taken = (np.random.default_rng(3).random(1000) < 0.2).astype(np.uint8)
    for k in range(2):
        n = len(sc["kps"][k])
        p = {a: want[a][k * 1000:(k + 1) * 1000] for a in want}
        Fr = oracle.Frame(sc["kps"][k], sc["desc"][k], W, H)
        q = (p["valid"], p["uv"], p["radius"], p["level"], sc["mp_desc"])
        sig = sc["inv_sigma2"][sc["kps"][k]["octave"]]
        flags = dict(kp_is_orb=np.ones(n, np.uint8), mp_is_orb=np.ones(1000, np.uint8))
        for kw_o, kw_m in ((dict(), dict()),
                           (dict(inv_sigma2=sc["inv_sigma2"]), dict(kp_inv_sigma2=sig)),
                           (dict(inv_sigma2=sc["inv_sigma2"], uright=sc["uright"][k], q_ur=p["q_ur"]), dict(kp_inv_sigma2=sig, uright=sc["uright"][k])),
                           (dict(taken=taken[:n], accept_thr=50.0), dict(taken=taken[:n], accept_thr=50.0))):
            w = oracle.kf_radius_match(Fr, *q, **kw_o)
            for fl in (flags, {}):
                got = ref.search(Fr, p, sc["mp_desc"], **kw_m, **fl)
                assert len(got) == len(w) and all(a.tobytes() == b.tobytes() for a, b in zip(got, w)), (k, list(kw_m))
            assert int((w[1] <= TH_LOW).sum()) >= 30


# ---- the scene of the GPU tests -----------------------------------------------------------------------------------------------------
def test_the_scene_of_the_gpu_tests_exercises_every_rule(oracle, ref):
    sc = cases.scene()
    p = cases.projection(3.0)[0]
    is_orb = sc["mp_is_orb"] == 1
    assert 0.25 <= 1 - is_orb.mean() <= 0.42 and 0.25 <= 1 - sc["kp_is_orb"][0].mean() <= 0.42      # about a third of each is AKAZE
    ak = sc["kp_is_orb"][0] == 0
    assert np.all(sc["kps"][0]["octave"][ak] == sc["kps"][0]["class_id"][ak] // 4)
    assert np.all(sc["kp_inv_sigma2"][0][ak] == sc["ak_inv_sigma2"][sc["kps"][0]["class_id"][ak]])
    assert np.any(sc["kp_inv_sigma2"][0][ak] != sc["inv_sigma2"][sc["kps"][0]["octave"][ak]])
    bi, bd = cases.search(oracle, sc, 0, p, "mono")
    acc_orb, acc_ak = int(((bd <= TH_LOW) & is_orb).sum()), int(((bd <= TH_LOW) & ~is_orb).sum())
    changed = {}
    for name, w in (("type gate", mref.NO_TYPE_GATE), ("octave", mref.LEVEL_FROM_OCTAVE), ("sigma", mref.ORB_SIGMA_TABLE)):
        wi, wd = cases.search(oracle, sc, 0, p, "mono", wrong=w, orb_inv_sigma2=sc["inv_sigma2"])
        changed[name] = int(((wi != bi) | (wd != bd)).sum())
    levels = np.unique(p["level"][(p["valid"] == 1) & ~is_orb])
    print("accepted", acc_orb, acc_ak, "changed", changed, "AKAZE levels", levels.tolist())
    assert acc_orb >= 20 and acc_ak >= 20
    assert all(c >= 5 for c in changed.values()), changed
    assert len(levels) >= 6 and levels.max() > 7


# ---- the batch is exact: the model map of tests/test_kfside_ref.py with mixed data --------------------------------------------------
def test_the_batched_mixed_fuse_equals_the_sequential_fuse_on_a_model_map(oracle, ref):
    K, M = 4, 300
    sc = synth.mixed_keyframe_neighbourhood(31, K, M, n_kps=[400, 350, 0, 420], jitter=1.5)
    p = ref.keyframe_side([ref.view(**kw) for kw in sc["views"]], *cases.geom(sc), 3.0, mp_is_orb=sc["mp_is_orb"])
    proj = [{a: p[a][k * M:(k + 1) * M] for a in p} for k in range(K)]
    frames = [cases.frame(oracle, sc, k) for k in range(K)]

    def search(k, ms, descs):
        ms = np.asarray(ms, np.int64)
        kw = cases.gate_kw(sc, k, "mono")
        kw["mp_is_orb"] = kw["mp_is_orb"][ms]
        return ref.search(frames[k], {a: proj[k][a][ms] for a in proj[k]}, np.ascontiguousarray(descs), **kw)
    seq = _Map(sc, 5)
    fused_seq = []
    for k in range(K):                                                               # the reference: every search on the map as it is
        n = 0
        for m in range(M):
            if seq.bad[m] or k in seq.obs[m]:
                continue
            bi, bd = search(k, [m], [seq.desc[m]])
            n += seq.apply(k, m, int(bi[0]), int(bd[0]))
        fused_seq.append(n)
    bat = _Map(sc, 5)                                                                # the adapter of eorb_fuse_keyframes_mixed
    rows = [search(k, np.arange(M), sc["mp_desc"]) for k in range(K)]
    uploaded = {m: sc["mp_desc"][m].tobytes() for m in range(M)}
    fused_bat, refreshed, dropped = [], 0, 0
    for k in range(K):
        n = 0
        for m in range(M):
            if bat.bad[m] or k in bat.obs[m]:
                dropped += int(rows[k][1][m] <= TH_LOW)
                continue
            bi, bd = int(rows[k][0][m]), int(rows[k][1][m])
            if bat.desc[m].tobytes() != uploaded[m]:
                r = search(k, [m], [bat.desc[m]])
                bi, bd = int(r[0][0]), int(r[1][0]); refreshed += 1
            n += bat.apply(k, m, bi, bd)
        fused_bat.append(n)
    assert fused_bat == fused_seq and bat.state() == seq.state()
    is_orb = sc["mp_is_orb"] == 1
    acc = np.concatenate([r[1] for r in rows]).reshape(K, M) <= TH_LOW
    print("fused", fused_seq, "went bad", seq.went_bad, "dropped", dropped, "refreshed", refreshed, "rows accepted", int(acc[:, is_orb].sum()), int(acc[:, ~is_orb].sum()))
    assert seq.went_bad >= 5 and dropped >= 3 and refreshed >= 1
    assert sum(fused_seq) >= 30 and fused_seq[2] == 0
    assert acc[:, is_orb].sum() >= 10 and acc[:, ~is_orb].sum() >= 10


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_mixed_keyframe_side_entry_points():
    from eorb_slam_amd import _lib, frontend
    L = C.CDLL(_lib.build())
    for sym in NEW_EXPORTS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTS
    for name in ("KeyFrameRadiusMatchMixed", "ProjectKeyFrameSideMixed", "FusePoseMixed", "SearchByProjectionKFScwMixed", "FuseKeyFramesMixed"):
        assert callable(getattr(frontend, name))
    assert callable(synth.mixed_keyframe_neighbourhood)
