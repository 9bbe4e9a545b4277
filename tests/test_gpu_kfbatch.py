"""GPU parity of the node-walk matchers over K keyframes per call (eorb_search_for_triangulation_keyframes, its KannalaBrandt8 form,
eorb_search_by_bow_keyframes, eorb_search_by_bow_kf_keyframes): row k of a batch is the oracle's single-pair function on pair k, as
integers, with no tolerance.  Cases and oracle rows: tests/kfbatch_cases.py.  The single-pair entry points are the same path with K = 1:
their checks, empty sides, strides and profile scopes are tested at the end."""
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


# ---- the single-pair entry points: the set form with K = 1 -------------------------------------------------------------------------
def _fisheye_scene():
    """the 32-keypoint two-camera frame (nL = 20) of test_gpu_twocam.py's empty-sides case against a KeyFrame made of its own rows with a
    few bits flipped; four vocabulary nodes"""
    rng = np.random.default_rng(71)
    kps = synth.random_keypoints(32, 512, 512, nlevels=8, seed=72); desc = synth.random_descriptors(32, seed=73)
    perm = rng.permutation(32)
    kd = np.stack([synth.flip_bits(desc[i], 6, rng) for i in perm])
    node = np.arange(32) % 4
    return dict(kf=(kps[perm], kd, (rng.uniform(size=32) < 0.8).astype(np.uint8), synth.feature_vector_of(node[perm], rng)),
                f=(kps, desc, np.ones(32, np.uint8), synth.feature_vector_of(node, rng)), nL=20)


class _Single:
    """One single-pair entry point on one small scene as a raw call: a side is (kps, desc, flag, fv); `set` is the side the entry point
    wraps into a set of one (pKF2, or the KeyFrame of SearchByBoW(pKF, F)), `shared` the other, which owns the output row.  call()
    -> (code, count, row) with the row prefilled with 7 and the count with -7."""

    def __init__(self, name, oracle):
        self.name = name
        if name == "tri":
            s = kc.tri_scene("pinhole_small")
            self.expect = [r[0] for r in kc.tri_rows("pinhole_small", 4, False, True)]
        elif name in ("tri_kb8", "tri_twocam"):
            s = kc.tri_scene(name[4:], 3)
            self.expect = [r[0] for r in kc.tri_rows(name[4:], 3, False, True)]
        if name.startswith("tri"):
            self.s = s
            self.set, self.shared = kc.tri_set(s, [0])[0], (s["kps1"], s["desc1"], s["elig1"], s["fv1"])
            self.nleft = (s["kfs"][0]["nleft"], s["nleft1"]) if "F12" not in s else None
        elif name in ("bow", "bow_kf"):
            s = kc.bow_scene("small")
            self.set, self.shared = kc.bow_set(s, [0])[0], (s["kps"], s["desc"], s["has_mp"], s["fv"])
            self.ratio = 0.8 if name == "bow_kf" else 0.7
            self.expect = [r[0] for r in kc.bow_rows("small", 4, name == "bow_kf", self.ratio, True)]
        else:
            s = _fisheye_scene()
            self.set, self.shared, self.nL = s["kf"], s["f"], s["nL"]
            self.expect = oracle.search_by_bow_fisheye(*self.set, self.shared[0], self.nL, self.shared[1], self.shared[3], 0.7, True)

    def call(self, fe, ctx, set_side, shared):
        L, h, p = ctx.L, ctx.h, fe._p
        keep = []                                           # the arrays the pointers refer to

        def side(sd, with_stride):
            kps, desc, flag, fv = sd
            a = [np.ascontiguousarray(kps, synth.KP_DTYPE), np.ascontiguousarray(desc, np.uint8), np.ascontiguousarray(flag, np.uint8)] + fe._fv(fv)
            keep.append(a)
            k, d, f, n, o, i = a
            stride = (int(d.shape[1]),) if with_stride else ()
            return (p(k), len(k)), (p(d),) + stride + (p(f),), (p(n), p(o), p(i), len(n))
        tri = self.name.startswith("tri")
        (k2, d2, v2), (k1, d1, v1) = side(set_side, tri), side(shared, tri)
        row = np.full(len(shared[0]), 7, np.int32); nm = C.c_int(-7)
        tail = (p(row), C.byref(nm))
        if tri:
            s = self.s
            f32 = lambda a: np.ascontiguousarray(a, np.float32)
            ep, sc, sg = f32(s["ep"][0]), f32(s["scale2"]), f32(s["sigma2_2"])
            if self.nleft is None:
                F = f32(s["F12"][0]).reshape(9)
                rc = L.eorb_search_for_triangulation(h, *k1, *d1, *v1, *k2, *d2, *v2, p(ep), p(F), p(sc), p(sg), len(sc), 0, 1, *tail)
            else:
                nl2, nl1 = (min(nl, len(sd[0])) for nl, sd in zip(self.nleft, (set_side, shared)))
                rt = np.zeros(48, np.float32); r = f32(s["Rt"][0]).reshape(-1); rt[:len(r)] = r
                c1, c2, s1 = fe._cams(s["cams1"]), fe._cams(s["cams2"]), f32(s["sigma2_1"])
                rc = L.eorb_search_for_triangulation_kb8(h, *k1, nl1, *d1, *v1, *k2, nl2, *d2, *v2, C.byref(c1), C.byref(c2), p(rt), p(ep), p(sc),
                                                         p(s1), p(sg), len(sg), 0, 1, *tail)
        elif self.name == "bow":
            rc = L.eorb_search_by_bow(h, *k2, *d2, *v2, *k1, d1[0], *v1, *tail[:1], self.ratio, 1, tail[1])
        elif self.name == "bow_kf":
            rc = L.eorb_search_by_bow_kf(h, *k1, *d1, *v1, *k2, *d2, *v2, *tail[:1], self.ratio, 1, tail[1])
        else:
            rc = L.eorb_search_by_bow_fisheye(h, *k2, *d2, *v2, *k1, min(self.nL, len(shared[0])), d1[0], *v1, *tail[:1], 0.7, 1, tail[1])
        return rc, nm.value, row


_SINGLES = ["tri", "tri_kb8", "tri_twocam", "bow", "bow_kf", "bow_fisheye"]


def _broken_fvs(sd):
    """the side with its feature vector broken in three ways: offsets that start at 1, an offset below its predecessor, an index equal to
    the side's feature count"""
    kps, desc, flag, (nodes, off, idx) = sd
    assert len(nodes) >= 2 and off[1] >= 1
    a = off.copy(); a[0] = 1
    b = off.copy(); b[2] = off[1] - 1
    c = idx.copy(); c[len(c) // 2] = len(kps)
    return [(kps, desc, flag, fv) for fv in ((nodes, a, idx), (nodes, b, idx), (nodes, off, c))]


@pytest.mark.parametrize("name", _SINGLES)
def test_single_forms_refuse_malformed_feature_vectors(oracle, fe, ctx, name):
    """offsets that do not start at 0 or decrease and an index past the side's features, on either side of each of the five single-pair
    entry points (the KannalaBrandt8 one on monocular and on two-camera keyframes): EORB_E_ARG with the row all -1 and the count 0, and
    the context then gives the oracle's result for the intact scene"""
    e = _Single(name, oracle)
    for bad in _broken_fvs(e.set):
        rc, n, row = e.call(fe, ctx, bad, e.shared)
        assert rc == E_ARG and n == 0 and (row == -1).all(), (rc, n)
    for bad in _broken_fvs(e.shared):
        rc, n, row = e.call(fe, ctx, e.set, bad)
        assert rc == E_ARG and n == 0 and (row == -1).all(), (rc, n)
    rc, n, row = e.call(fe, ctx, e.set, e.shared)
    print(name, "oracle", e.expect[0], "gpu", n)
    assert rc == 0 and n == e.expect[0] and np.array_equal(row, e.expect[1])


@pytest.mark.parametrize("name", _SINGLES)
def test_single_forms_on_empty_sides(oracle, fe, ctx, name):
    """no rows on the set's side, rows without nodes there, no rows on the shared side: EORB_OK, count 0, every slot -1"""
    e = _Single(name, oracle)
    stride = e.set[1].shape[1]
    for set_side, shared in ((_empty_kf(stride), e.shared), (e.set[:3] + (_EMPTY_FV,), e.shared), (e.set, _empty_kf(stride))):
        rc, n, row = e.call(fe, ctx, set_side, shared)
        assert rc == 0 and n == 0 and len(row) == len(shared[0]) and (row == -1).all(), (rc, n)


def test_triangulation_pair_with_unequal_strides(oracle, fe, ctx):
    """stride1 = 32 against stride2 = 61 and the reverse (padding: random bytes): the set carries pKF2's stride and pKF1 its own"""
    s = kc.tri_scene("pinhole_small")
    kf = s["kfs"][0]
    on, om = (r[0] for r in kc.tri_rows("pinhole_small", 4, False, True))
    assert on >= 20
    rng = np.random.default_rng(9)
    pad = lambda d: np.concatenate([d, rng.integers(0, 256, (len(d), 29), dtype=np.uint8)], axis=1)
    for d1, d2 in ((s["desc1"], pad(kf["desc"])), (pad(s["desc1"]), kf["desc"])):
        assert {d1.shape[1], d2.shape[1]} == {32, 61}
        gn, pairs = fe.SearchForTriangulation(s["kps1"], d1, s["elig1"], s["fv1"], kf["kps"], d2, kf["elig"], kf["fv"], s["ep"][0], s["F12"][0],
                                              s["scale2"], s["sigma2_2"], False, True, ctx=ctx)
        ok = np.nonzero(om >= 0)[0]
        assert gn == on and np.array_equal(pairs, np.stack([ok, om[ok]], axis=1))


def test_profile_scopes_keep_the_entry_points_names(oracle, fe, ctx):
    """one call of each single-pair entry point and one set call, profiled: the single calls are recorded under their own scopes (both
    SearchByBoW forms under search_bow), the set call under its own, each once per call"""
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        for name in ("tri", "tri_kb8", "bow", "bow_kf", "bow_fisheye"):
            e = _Single(name, oracle)
            assert e.call(fe, ctx, e.set, e.shared)[0] == 0
        b = kc.bow_scene("small")
        fe.SearchByBoWKeyFrames(kc.bow_set(b), b["kps"], b["desc"], b["fv"], 0.7, True, ctx=ctx)
        got = {k: v[1] for k, v in ctx.prof_results().items()}
    finally:
        ctx.prof_enable(False)
    assert got == {"search_for_triangulation": 1, "search_for_triangulation_kb8": 1, "search_bow": 2, "search_bow_fisheye": 1,
                   "search_by_bow_keyframes": 1}, got
