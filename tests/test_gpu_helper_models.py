"""The HIP kernels behind ORBextractor.stereo, BFMatcher.knnMatch2, ORBextractor.fisheye's Lowe test, HammingWindowMatch,
ComputeDistinctiveDescriptors and sortFeaturesResponse on the planted scenes of tests/helper_scenes.py: equal to the plain models of
tests/helper_models.py (and so to the oracle, which tests/test_oracle_helper_models.py holds to the same models on the CPU, where it
also shows that these scenes tell every wrong variant from the rule) as integers and bit patterns.

bf_knn2_dev launches bf_knn2_kernel<16> for nq >= 16384, <32> for nq >= 4096 and <64> below: the eight query counts of
helper_scenes.KNN_NQ sit on both sides of both thresholds, so all three instantiations run."""
import ctypes as C

import numpy as np
import pytest

from eorb_slam_amd import synth

import helper_models as hm
import helper_scenes as hs

pytestmark = pytest.mark.gpu

F = np.float32
E_CAPACITY, E_ARG = -3, -4


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def extractor(fe):
    """one extractor for every stereo pair, in the order of the scenes: a call follows whatever the one before left behind"""
    ge = fe.ORBextractor(*hs.ORB_ARGS, (hs.W, hs.H))
    yield ge
    ge.ctx.close()


def bits(a):
    return np.asarray(a, F).view(np.uint32)


# ---- ORBextractor.stereo -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(hs.STEREO_PAIRS))
def test_stereo(oracle, extractor, name):
    I, mb, mbf, sites = hs.stereo_case(oracle, name)
    ur, dp, n, P = hs.stereo_model(oracle, name)
    our, odp, on = I.oracle(mb, mbf)
    assert on == n and np.array_equal(bits(our), bits(ur)) and np.array_equal(bits(odp), bits(dp)), "the oracle differs from the model"
    assert all(P[s] > 0 for s in sites)
    for call in range(2):                                                   # twice in a row on one extractor
        g = extractor.stereo(I.left, I.right, mb, mbf)
        assert len(g["kpsL"]) == len(I.kL) and len(g["kpsR"]) == len(I.kR), (call, len(g["kpsL"]), len(g["kpsR"]))
        assert np.array_equal(g["kpsL"].view(np.uint8), I.kL.view(np.uint8)) and np.array_equal(g["kpsR"].view(np.uint8), I.kR.view(np.uint8))
        assert np.array_equal(g["descL"], I.dL) and np.array_equal(g["descR"], I.dR)
        bad = np.flatnonzero((bits(g["uRight"]) != bits(ur)) | (bits(g["depth"]) != bits(dp)))
        assert g["nmatches"] == n and len(bad) == 0, "%s call %d: %d accepted, model %d; %d keypoints differ, first %s: uRight %s, model %s" % (
            name, call, g["nmatches"], n, len(bad), bad[:5], g["uRight"][bad[:5]], ur[bad[:5]])
    if name == "mixed":                                                     # the 0.01 branch's value in a final uRight / depth
        z = np.flatnonzero(bits(g["depth"]) == bits(np.array(F(mbf) / F(0.01), F)))
        assert len(z) == P["zero_branch_kept"] >= 1
        assert np.array_equal(bits(g["uRight"][z]), bits((I.kL["x"][z].astype(np.float64) - 0.01).astype(F)))
    if name in ("identical", "mirror"):                                     # median 0: everything is taken back
        assert g["nmatches"] > 100 and np.all(g["uRight"] == -1) and np.all(g["depth"] == -1)


# ---- BFMatcher.knnMatch2 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", hs.KNN_NQ)
def test_knn2(oracle, fe, ctx, nq):
    m = fe.BFMatcher(ctx)
    for nt in hs.KNN_NT:
        q, t = hs.knn_scene(nq, nt)
        idx, dist = hm.knn2(q, t)
        gi, gd = m.knnMatch2(q.reshape(-1, 32), t.reshape(-1, 32))
        bad = np.flatnonzero((gi != idx).any(axis=1) | (gd != dist).any(axis=1))
        assert len(bad) == 0, "nq %d nt %d: %d queries differ, first %s: %s / %s, model %s / %s" % (
            nq, nt, len(bad), bad[:5], gi[bad[:3]].tolist(), gd[bad[:3]].tolist(), idx[bad[:3]].tolist(), dist[bad[:3]].tolist())
    if nq:                                                                  # the oracle once per launch shape, at the largest train set
        oi, od = oracle.bf_knn2(q, t)
        assert np.array_equal(oi, gi) and np.array_equal(od, gd)


# ---- ORBextractor.fisheye: knn2 of the lapping rows and Lowe's test ----------------------------------------------------------------
@pytest.mark.parametrize("laps", [((0, 511), (0, 511)), ((0, 300), (200, 511))])
def test_fisheye_lowe(fe, ctx, laps):
    """the two-camera scene of tests/test_gpu_twocam.py (1500 features, seed 8).  With the full lapping areas 4 of its left keypoints
    have 10 * d0 == 7 * d1, the equality that `<` against the double product d1 * 0.7 decides, and 1 with the partial ones: on both,
    helper_models.lowe with `ratio_le` gives another answer (asserted below)."""
    W = H = 512
    imL, imR = synth.image_pair(W, H, seed=8)
    ge = fe.ORBextractor(1500, 1.2, 8, 20, 7, 19, imSize=(W, H), ctx=ctx)
    g = ge.fisheye(imL, imR, laps[0], laps[1])
    mL, mR = g["monoLeft"], g["monoRight"]
    idx, dist = hm.knn2(g["descL"][mL:], g["descR"][mR:])
    cand, n = hm.lowe(idx, dist, mL, mR)
    assert np.array_equal(g["dist2"][mL:], dist) and np.all(g["dist2"][:mL] == -1)
    assert g["right_idx"][mL:].tolist() == cand and np.all(g["right_idx"][:mL] == -1) and g["ncand"] == n > 100
    ties = int((10 * dist[:, 0] == 7 * dist[:, 1]).sum())
    print("pairs with 10 * d0 == 7 * d1: %d" % ties)
    assert ties >= 1 and hm.lowe(idx, dist, mL, mR, "ratio_le")[0] != cand


# ---- HammingWindowMatch ------------------------------------------------------------------------------------------------------------
def test_window_match(fe, ctx):
    q, t, offs, cand, sites = hs.window_scene()
    want = hm.window_match(q, t, offs, cand)
    got = fe.HammingWindowMatch(q, t, offs, cand, ctx=ctx)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), [int((a != b).sum()) for a, b in zip(got, want)]
    # rows 61 bytes apart (AKAZE's, src/MixedFrame.cpp:20-21) and other strides >= 32 through the C ABI: load_desc32's bytewise path
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # also with the first row 1 to 7 bytes into the caller's buffer
    for qs, ts, lead in ((32, 61, 0), (61, 32, 3), (61, 61, 1), (33, 40, 7), (32, 32, 5)):
        qb, tb = hs.strided(q, qs, lead), hs.strided(t, ts, lead)
        out = [np.full(len(q), -7, np.int32) for _ in range(4)]
        rc = ctx.L.eorb_hamming_window_match(ctx.h, C.c_void_p(qb.ctypes.data + lead), len(q), qs, C.c_void_p(tb.ctypes.data + lead), len(t), ts,
                                             p(offs), p(cand), *[p(o) for o in out])
        assert rc == 0, (qs, ts, lead, rc)
        assert all(np.array_equal(a, b) for a, b in zip(out, want)), (qs, ts, lead, [int((a != b).sum()) for a, b in zip(out, want)])


# ---- ComputeDistinctiveDescriptors -------------------------------------------------------------------------------------------------
def test_distinctive(fe, ctx):
    desc, offs, names = hs.distinctive_scene()
    want = hm.distinctive(desc, offs)
    got = fe.ComputeDistinctiveDescriptors(desc, offs, ctx=ctx).tolist()
    assert got == want, [(n, a, b) for n, a, b in zip(names, got, want) if a != b][:8]


def test_distinctive_capacity(fe, ctx):
    """distinctive_kernel's bins are 16 bits wide: a map point with more than 65 535 rows is refused from the sizes alone; 65 535
    identical rows put 65 535 into one bin, the most it holds, and every median is 0, so the first row wins"""
    desc = np.zeros((65536 + 3, 32), np.uint8)
    for offs in ([0, 65536], [0, 3, 65536 + 3], [0, 65536, 65536 + 3]):
        with pytest.raises(fe.EorbError) as e:
            fe.ComputeDistinctiveDescriptors(desc[:offs[-1]], np.array(offs, np.int32), ctx=ctx)
        assert e.value.code == E_CAPACITY, offs
    rc = ctx.L.eorb_distinctive_descriptors(ctx.h, desc.ctypes.data_as(C.c_void_p), np.array([-2 ** 31, 0, 3], np.int32).ctypes.data_as(C.c_void_p), 2,
                                            np.zeros(2, np.int32).ctypes.data_as(C.c_void_p))
    assert rc == E_ARG                                                      # (a negative offset: refused, and the size is taken in 64 bits)
    assert fe.ComputeDistinctiveDescriptors(desc[:65538], np.array([0, 3, 65538], np.int32), ctx=ctx).tolist() == [0, 0]


# ---- sortFeaturesResponse ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", hs.SORT_N)
def test_sort_by_response(oracle, fe, ctx, n):
    k = hs.response_keypoints(synth.KP_DTYPE, n)
    want = hm.sort_by_response(k["response"])
    assert fe.sortFeaturesResponse(k, ctx).tolist() == want
    assert oracle.sort_by_response(k).tolist() == want
