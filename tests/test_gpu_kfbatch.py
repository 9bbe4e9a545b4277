"""GPU parity of the node-walk matchers over K keyframes per call (eorb_search_for_triangulation_keyframes, its KannalaBrandt8 form,
eorb_search_by_bow_keyframes, eorb_search_by_bow_kf_keyframes): row k of a batch is the oracle's single-pair function on pair k, as
integers, with no tolerance.  Cases and oracle rows: tests/kfbatch_cases.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfbatch_cases as kc                          # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

pytestmark = pytest.mark.gpu

E_CONFIG, E_CAPACITY, E_ARG = -2, -3, -4


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


def _tri_batch(fe, ctx, s, kfs, ks, coarse, ori, e1=None):
    e1 = s["elig1"] if e1 is None else e1
    if "F12" in s:
        return fe.SearchForTriangulationKeyFrames(s["kps1"], s["desc1"], e1, s["fv1"], kfs, s["ep"][ks], s["F12"][ks], s["scale2"], s["sigma2_2"],
                                                  coarse, ori, ctx=ctx)
    return fe.SearchForTriangulationKB8KeyFrames(s["kps1"], s["nleft1"], s["desc1"], e1, s["fv1"], kfs, [s["kfs"][k]["nleft"] for k in ks],
                                                 s["cams1"], s["cams2"], s["Rt"][ks], s["ep"][ks], s["scale2"], s["sigma2_1"], s["sigma2_2"],
                                                 coarse, ori, ctx=ctx)


def _tri_single(fe, ctx, s, k, coarse, ori):
    kf = s["kfs"][k]
    if "F12" in s:
        n, pairs = fe.SearchForTriangulation(s["kps1"], s["desc1"], s["elig1"], s["fv1"], kf["kps"], kf["desc"], kf["elig"], kf["fv"], s["ep"][k],
                                             s["F12"][k], s["scale2"], s["sigma2_2"], coarse, ori, ctx=ctx)
    else:
        n, pairs = fe.SearchForTriangulationKB8(s["kps1"], s["nleft1"], s["desc1"], s["elig1"], s["fv1"], kf["kps"], kf["nleft"], kf["desc"],
                                                kf["elig"], kf["fv"], s["cams1"], s["cams2"], s["Rt"][k], s["ep"][k], s["scale2"], s["sigma2_1"],
                                                s["sigma2_2"], coarse, ori, ctx=ctx)
    m = np.full(len(s["kps1"]), -1, np.int32)
    m[pairs[:, 0]] = pairs[:, 1]
    return n, m


def _check_conditions(nm_plain, nm_ori, bins):
    """the cases' conditions, on the oracle's results: every pair has at least 20 matches, the rotation check removes some from every pair,
    and the pairs keep different histogram bins (a histogram shared across k could not pass)"""
    assert (nm_ori >= 20).all() and (nm_plain >= 20).all(), (nm_plain, nm_ori)
    assert (nm_ori < nm_plain).all(), (nm_plain, nm_ori)
    assert all(bins[k] != bins[k + 1] for k in range(len(bins) - 1)), bins


def _tri_bins(s, rows):
    return [kc.kept_bins(s["kps1"]["angle"][m >= 0], kf["kps"]["angle"][m[m >= 0]]) for kf, m in zip(s["kfs"], rows)]


@pytest.mark.parametrize("kind", ["pinhole", "pinhole_small", "kb8", "twocam"])
def test_triangulation_rows_equal_the_oracle(oracle, fe, ctx, kind):
    """K = 4 (K = 3 for the KannalaBrandt8 forms): every row equals its oracle row with checkOri off and on and with bCoarse; the elig
    bytes of the monocular scenes carry stereo bits (bit 1).  K = 1: row 0 equals the single entry point and the oracle."""
    K = 4 if kind.startswith("pinhole") else 3
    s = kc.tri_scene(kind, K)
    ks = list(range(K))
    S = fe.KeyFrameSet(kc.tri_set(s))
    got = {}
    for coarse, ori in ((False, False), (False, True), (True, False), (True, True)):
        on, om = kc.tri_rows(kind, K, coarse, ori)
        gn, gm = _tri_batch(fe, ctx, s, S, ks, coarse, ori)
        print(kind, "coarse", coarse, "ori", ori, "oracle", on.tolist(), "gpu", gn.tolist())
        assert np.array_equal(on, gn) and np.array_equal(om, gm)
        got[coarse, ori] = (on, om)
    _check_conditions(got[False, False][0], got[False, True][0], _tri_bins(s, got[False, True][1]))
    if not s["nleft1"] >= 0:
        assert any(((kf["elig"] & 3) == 3).any() for kf in s["kfs"]) and ((s["elig1"] & 3) == 3).any()
    for ori in (False, True):
        on, om = kc.tri_rows(kind, K, False, ori)
        gn, gm = _tri_batch(fe, ctx, s, kc.tri_set(s, [1]), [1], False, ori)
        sn, sm = _tri_single(fe, ctx, s, 1, False, ori)
        assert gn[0] == on[1] == sn and np.array_equal(gm[0], om[1]) and np.array_equal(gm[0], sm)


def test_triangulation_stride_and_pinhole_camera2(oracle, fe, ctx):
    """Mixed rows (stride 61) through the set's one stride, and a KannalaBrandt8 pKF1 against neighbours seen by a Pinhole pCamera2"""
    s = synth.triangulation_neighbourhood(105, 3, pinhole=True, stride=61, angle_step=kc.ANGLE_STEP)
    S = kc.tri_set(s)
    gn, gm = fe.SearchForTriangulationKeyFrames(s["kps1"], s["desc1"], s["elig1"], s["fv1"], S, s["ep"], s["F12"], s["scale2"], s["sigma2_2"],
                                                False, True, ctx=ctx)
    for k, kf in enumerate(s["kfs"]):
        on, om = oracle.search_for_triangulation(s["kps1"], s["desc1"], s["elig1"], s["fv1"], kf["kps"], kf["desc"], kf["elig"], kf["fv"], s["ep"][k],
                                                 s["F12"][k], s["scale2"], s["sigma2_2"], False, True)
        assert on >= 20 and on == gn[k] and np.array_equal(om, gm[k])
    s = kc.tri_scene("kb8", 3)
    pin = synth.CAM_MONO[:4]
    gn, gm = fe.SearchForTriangulationKB8KeyFrames(s["kps1"], -1, s["desc1"], s["elig1"], s["fv1"], kc.tri_set(s), [-1] * 3, s["cams1"], pin, s["Rt"],
                                                   s["ep"], s["scale2"], s["sigma2_1"], s["sigma2_2"], False, False, ctx=ctx)
    total = 0
    for k, kf in enumerate(s["kfs"]):
        on, om = oracle.search_for_triangulation_kb8(s["kps1"], -1, s["desc1"], s["elig1"], s["fv1"], kf["kps"], -1, kf["desc"], kf["elig"], kf["fv"],
                                                     s["cams1"], pin, s["Rt"][k], s["ep"][k], s["scale2"], s["sigma2_1"], s["sigma2_2"], False, False)
        assert on == gn[k] and np.array_equal(om, gm[k])
        total += on
    assert total >= 20


@pytest.mark.parametrize("kind", ["small", "big"])
@pytest.mark.parametrize("kf_kf", [False, True])
def test_bow_rows_equal_the_oracle(oracle, fe, ctx, kind, kf_kf):
    """K = 4: every row equals its oracle row, checkOri on and off.  'big' holds nodes on both sides of the walk's 64-feature limit in one
    batch.  K = 1: row 0 equals the single entry point and the oracle."""
    K = 4
    s = kc.bow_scene(kind, K)
    if kind == "big":
        sizes = np.concatenate([kc.node_sizes(kf["fv"]) for kf in s["kfs"]] + [kc.node_sizes(s["fv"])])
        assert (sizes > 64).sum() >= 4 and ((sizes <= 64) & (sizes >= 30)).sum() >= 4, sizes
    S = fe.KeyFrameSet(kc.bow_set(s))
    ratio = 0.8 if kf_kf else 0.7

    def batch(kfs, ori):
        if kf_kf:
            return fe.SearchByBoW_KF_KeyFrames(s["kps"], s["desc"], s["has_mp"], s["fv"], kfs, ratio, ori, ctx=ctx)
        return fe.SearchByBoWKeyFrames(kfs, s["kps"], s["desc"], s["fv"], ratio, ori, ctx=ctx)
    got = {}
    for ori in (False, True):
        on, om = kc.bow_rows(kind, K, kf_kf, ratio, ori)
        gn, gm = batch(S, ori)
        print(kind, "kf_kf", kf_kf, "ori", ori, "oracle", on.tolist(), "gpu", gn.tolist())
        assert np.array_equal(on, gn) and np.array_equal(om, gm)
        got[ori] = (on, om)
    om = got[True][1]
    if kf_kf:
        bins = [kc.kept_bins(s["kps"]["angle"][m >= 0], kf["kps"]["angle"][m[m >= 0]]) for kf, m in zip(s["kfs"], om)]
    else:
        bins = [kc.kept_bins(kf["kps"]["angle"][m[m >= 0]], s["kps"]["angle"][m >= 0]) for kf, m in zip(s["kfs"], om)]
    _check_conditions(got[False][0], got[True][0], bins)
    for ori in (False, True):
        on, om = kc.bow_rows(kind, K, kf_kf, ratio, ori)
        kf = s["kfs"][2]
        gn, gm = batch(kc.bow_set(s, [2]), ori)
        if kf_kf:
            sn, sm = fe.SearchByBoW_KF(s["kps"], s["desc"], s["has_mp"], s["fv"], kf["kps"], kf["desc"], kf["has_mp"], kf["fv"], ratio, ori, ctx=ctx)
        else:
            sn, sm = fe.SearchByBoW(kf["kps"], kf["desc"], kf["has_mp"], kf["fv"], s["kps"], s["desc"], s["fv"], ratio, ori, ctx=ctx)
        assert gn[0] == on[2] == sn and np.array_equal(gm[0], om[2]) and np.array_equal(gm[0], sm)


_EMPTY_FV = (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.int32))


def _empty_kf(stride=32):
    return (np.zeros(0, synth.KP_DTYPE), np.zeros((0, stride), np.uint8), np.zeros(0, np.uint8), _EMPTY_FV)


def _one_row_kf(kf):
    """a keyframe of one row: row 0 of kf under its own node"""
    kps, desc, flag, fv = kf
    r = int(fv[2][0])
    return (kps[r:r + 1], desc[r:r + 1], np.ones(1, np.uint8), (fv[0][:1], np.array([0, 1], np.int32), np.zeros(1, np.int32)))


def test_independence_of_the_pairs(oracle, fe, ctx):
    """[A, empty keyframe, A, B, one-row keyframe] with different row counts, none a multiple of 64: rows 0 and 2 are identical, row 1 is
    all -1 with count 0, row 3 equals B alone, and the single row finds what the oracle finds -- for each of the four entry points"""
    s = kc.tri_scene("pinhole", 4)
    A, B = kc.tri_set(s, [0])[0], kc.tri_set(s, [3])[0]
    one = _one_row_kf(A)
    assert len(A[0]) != len(B[0]) and len(A[0]) % 64 and len(B[0]) % 64
    ks = [0, 0, 0, 3, 0]
    on, om = kc.tri_rows("pinhole", 4, False, True)
    gn, gm = _tri_batch(fe, ctx, s, [A, _empty_kf(), A, B, one], ks, False, True)
    assert np.array_equal(gm[0], om[0]) and np.array_equal(gm[2], om[0]) and gn[0] == gn[2] == on[0]
    assert gn[1] == 0 and (gm[1] == -1).all()
    assert gn[3] == on[3] and np.array_equal(gm[3], om[3])
    o1n, o1m = oracle.search_for_triangulation(s["kps1"], s["desc1"], s["elig1"], s["fv1"], one[0], one[1], one[2], one[3], s["ep"][0], s["F12"][0],
                                               s["scale2"], s["sigma2_2"], False, True)
    assert gn[4] == o1n and np.array_equal(gm[4], o1m)
    # a keyframe with rows and no nodes
    nonodes = (A[0], A[1], A[2], _EMPTY_FV)
    gn, gm = _tri_batch(fe, ctx, s, [nonodes, B], [0, 3], False, True)
    assert gn[0] == 0 and (gm[0] == -1).all() and gn[1] == on[3] and np.array_equal(gm[1], om[3])

    k8 = kc.tri_scene("kb8", 3)
    A8, B8 = kc.tri_set(k8, [0])[0], kc.tri_set(k8, [2])[0]
    on, om = kc.tri_rows("kb8", 3, False, True)
    gn, gm = _tri_batch(fe, ctx, k8, [A8, _empty_kf(), A8, B8], [0, 0, 0, 2], False, True)
    assert np.array_equal(gm[0], om[0]) and np.array_equal(gm[2], om[0]) and gn[1] == 0 and (gm[1] == -1).all()
    assert gn[3] == on[2] and np.array_equal(gm[3], om[2])

    b = kc.bow_scene("big", 4)
    A, B = kc.bow_set(b, [0])[0], kc.bow_set(b, [3])[0]
    one = _one_row_kf(A)
    assert len(A[0]) != len(B[0]) and len(A[0]) % 64 and len(B[0]) % 64
    for kf_kf in (False, True):
        ratio = 0.8 if kf_kf else 0.7
        on, om = kc.bow_rows("big", 4, kf_kf, ratio, True)
        kfs = [A, _empty_kf(), A, B, one]
        if kf_kf:
            gn, gm = fe.SearchByBoW_KF_KeyFrames(b["kps"], b["desc"], b["has_mp"], b["fv"], kfs, ratio, True, ctx=ctx)
            o1n, o1m = oracle.search_by_bow_kf(b["kps"], b["desc"], b["has_mp"], b["fv"], one[0], one[1], one[2], one[3], ratio, True)
        else:
            gn, gm = fe.SearchByBoWKeyFrames(kfs, b["kps"], b["desc"], b["fv"], ratio, True, ctx=ctx)
            o1n, o1m = oracle.search_by_bow(one[0], one[1], one[2], one[3], b["kps"], b["desc"], b["fv"], ratio, True)
        assert np.array_equal(gm[0], om[0]) and np.array_equal(gm[2], om[0]) and gn[0] == gn[2] == on[0]
        assert gn[1] == 0 and (gm[1] == -1).all()
        assert gn[3] == on[3] and np.array_equal(gm[3], om[3])
        assert gn[4] == o1n and np.array_equal(gm[4], o1m)


def test_errors_come_back_as_codes(fe, ctx):
    """an out-of-range octave in keyframe 2 of 3, mixed nleft2 signs, non-monotone kf_off, and sizes beyond the limits (sizes only: every
    array pointer is NULL, so the limit is decided before any buffer is read)"""
    from eorb_slam_amd import _lib
    s = kc.tri_scene("pinhole", 4)
    kfs = kc.tri_set(s, [0, 1, 2])
    bad = kfs[2][0].copy()
    bad["octave"][np.nonzero(kfs[2][2])[0][0]] = 9
    with pytest.raises(fe.EorbError) as e:
        _tri_batch(fe, ctx, s, [kfs[0], kfs[1], (bad,) + kfs[2][1:]], [0, 1, 2], False, False)
    assert e.value.code == E_ARG and "keyframe 2" in str(e.value)
    k8 = kc.tri_scene("kb8", 3)
    with pytest.raises(fe.EorbError) as e:
        fe.SearchForTriangulationKB8KeyFrames(k8["kps1"], -1, k8["desc1"], k8["elig1"], k8["fv1"], kc.tri_set(k8), [-1, 5, -1], k8["cams1"],
                                              k8["cams2"], k8["Rt"], k8["ep"], k8["scale2"], k8["sigma2_1"], k8["sigma2_2"], ctx=ctx)
    assert e.value.code == E_CONFIG and "keyframe 1" in str(e.value)
    S = fe.KeyFrameSet(kfs)
    S.kf_off[1], S.kf_off[2] = S.kf_off[2], S.kf_off[1]
    with pytest.raises(fe.EorbError) as e:
        _tri_batch(fe, ctx, s, S, [0, 1, 2], False, False)
    assert e.value.code == E_ARG
    b = kc.bow_scene("small", 4)
    with pytest.raises(fe.EorbError) as e:
        fe.SearchByBoWKeyFrames(S, b["kps"], b["desc"], b["fv"], ctx=ctx)
    assert e.value.code == E_ARG
    # sizes only
    L = ctx.L
    nm = np.zeros(4, np.int32)
    for K, n in ((1025, 1), (4, (1 << 20) + 1)):
        hollow = _lib.KfSet(K, None, None, 32, None, None, None, None, None, None)
        assert L.eorb_search_for_triangulation_keyframes(ctx.h, None, n, None, 32, None, None, None, None, 1, C.byref(hollow), None, None, None, None, 8,
                                                         0, 0, None, None) == E_CAPACITY
        assert L.eorb_search_for_triangulation_kb8_keyframes(ctx.h, None, n, -1, None, 32, None, None, None, None, 1, C.byref(hollow), None, None, None,
                                                             None, None, None, None, None, 8, 0, 0, None, None) == E_CAPACITY
        assert L.eorb_search_by_bow_keyframes(ctx.h, C.byref(hollow), None, n, None, None, None, None, 1, None, 0.7, 1, None) == E_CAPACITY
        assert L.eorb_search_by_bow_kf_keyframes(ctx.h, None, n, None, None, None, None, None, 1, C.byref(hollow), None, 0.8, 1, None) == E_CAPACITY
    # rows in all: the offsets are read, nothing else
    off = np.array([0, (1 << 22) + 1], np.int32); noff = np.zeros(2, np.int32)
    big = _lib.KfSet(1, None, None, 32, None, off.ctypes.data_as(C.c_void_p), None, noff.ctypes.data_as(C.c_void_p), None, None)
    assert L.eorb_search_by_bow_keyframes(ctx.h, C.byref(big), None, 10, None, None, None, None, 1, None, 0.7, 1, None) == E_CAPACITY
    # the context still works
    gn, gm = _tri_batch(fe, ctx, s, kfs, [0, 1, 2], False, False)
    on, om = kc.tri_rows("pinhole", 4, False, False)
    assert np.array_equal(gn, on[:3]) and np.array_equal(gm, om[:3])
