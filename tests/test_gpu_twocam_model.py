"""The two-camera HIP matchers (twocam_walk_kernel<0|1>, search_bow_fisheye_kernel) on the planted scenes of tests/twocam_scenes.py:
byte equality with the oracle and integer equality with the brute-force models of tests/twocam_model.py
(tests/test_oracle_twocam_model.py shows on the CPU that these scenes tell every wrong variant from the rule).  The size scenes take
the walk's three loops past one trip: a window of more than 64 cells, a cell of more than 64 keypoints, a frame of kTcMaxKps keypoints."""
import numpy as np
import pytest

import kfside_model as km
import kfside_mixed_ref as mref
import kfside_ref
import twocam_scenes as ts
from twocam_scenes import CASES, scenes

pytestmark = pytest.mark.gpu

E_CAPACITY = -3


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


def _differs(got, want, names):
    bad = np.flatnonzero(np.asarray(got[1]) != np.asarray(want[1]))
    return "nmatches %d, expected %d; %d entries differ, first %s" % (got[0], want[0], len(bad), bad[:5])


@pytest.mark.parametrize("kind,name", CASES)
def test_kernels_equal_oracle_and_model(oracle, fe, ctx, kind, name):
    sc = dict(scenes(kind))[name]
    for cfg in ts.configs(kind):
        for check_ori in ((True, False) if kind != "map" else (True,)):
            want = ts.run_oracle(oracle, kind, sc, cfg, check_ori)
            model = ts.run_model(kind, sc, cfg, check_ori)
            assert ts.same(want, model), "%s %s %s: the oracle differs from the model" % (kind, name, ts.config_id(cfg))
            got = ts.run_kernels(fe, ctx, kind, sc, cfg, check_ori)
            assert got[0] == want[0] and np.asarray(got[1]).tobytes() == np.asarray(want[1]).tobytes(), "%s %s %s ori=%d: %s" % (
                kind, name, ts.config_id(cfg), check_ori, _differs(got, want, sc.get("names")))


@pytest.mark.parametrize("kind", ["map", "last"])
def test_full_frame(oracle, fe, ctx, kind):
    """kTcMaxKps = 8 192 keypoints over both cameras (24 592 + 16 x 8 192 bytes of LDS, under the opt-in), eight queries, one call"""
    sc = ts.full_scene()
    want = ts.run_oracle(oracle, kind, sc, ts.MAIN[kind])
    assert ts.same(want, ts.run_model(kind, sc, ts.MAIN[kind])) and want[0] >= 16
    got = ts.run_kernels(fe, ctx, kind, sc, ts.MAIN[kind])
    assert got[0] == want[0] and np.asarray(got[1]).tobytes() == np.asarray(want[1]).tobytes(), _differs(got, want, None)


@pytest.mark.parametrize("kind", ["map", "last"])
def test_one_keypoint_past_the_capacity_is_refused(fe, ctx, kind):
    """8 193 keypoints: the call returns EORB_E_CAPACITY"""
    sc = ts.full_scene(ts.MAX_KPS + 1)
    assert len(sc["kps"]) == ts.MAX_KPS + 1
    with pytest.raises(fe.EorbError) as e:
        ts.run_kernels(fe, ctx, kind, sc, ts.MAIN[kind])
    assert e.value.code == E_CAPACITY


# ---- the KeyFrame-side radius search: stereo gate, octave skip, in-order claim ----------------------------------------------------
@pytest.mark.parametrize("form", km.FORMS)
def test_kf_radius_equals_oracle_and_model(oracle, fe, ctx, form):
    """radius_scan through eorb_kf_radius_match / eorb_kf_radius_match_stereo (K = 1 of kf_radius_batch_kernel, kf_radius_seq_kernel
    with the taken flags): the model on every query, the oracle where every candidate's octave lies inside the levels"""
    sc = km.scene()
    got = km.run_kernels(fe, ctx, sc, form)
    want = km.run_model(sc, form)
    assert len(got) == len(want), "%s: %d outputs, the model has %d" % (form, len(got), len(want))
    bad = np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), "%s: %d queries differ from the model, first %s (%s)" % (
        form, len(bad), bad[:5], sc["names"][bad[:1]])
    ok = km.in_range(sc, form).astype(bool)
    o = km.run_oracle(oracle, sc, form)
    assert all(np.asarray(a)[ok].tobytes() == np.asarray(b)[ok].tobytes() for a, b in zip(got[:2], o[:2])) and (ok.all() or "gate" in form)
    if len(got) == 3:
        assert np.asarray(got[2]).tobytes() == np.asarray(o[2]).tobytes()


# ---- the forms that project on the device ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref(oracle):
    kfside_ref.use_oracle_camera(oracle)
    return kfside_ref


def _rows_equal(got, want, what):
    bad = np.flatnonzero((np.asarray(got[0]) != want[0]) | (np.asarray(got[1]) != want[1]))
    assert len(bad) == 0, "%s: %d queries differ from the model, first %s: got %s / %s, expected %s / %s" % (
        what, len(bad), bad[:5], np.asarray(got[0])[bad[:5]], np.asarray(got[1])[bad[:5]], want[0][bad[:5]], want[1][bad[:5]])


@pytest.mark.parametrize("gate", ["mono", "stereo", "none"])
def test_fuse_keyframes_k3_with_edge_values(fe, ctx, ref, gate):
    """FuseKeyFrames with K = 3 (keyframe 0 empty; keyframes 1 and 2 on grids of their own, edge values among their keypoint positions,
    the radius through th in TH_VALUES), each keyframe again as K = 1 of the batch and as a single FusePose call: the model, row by row"""
    sc = km.batch_scene()
    K, M = 3, len(sc["min_dist"])
    views = [fe.view(**kw) for kw in sc["views"]]
    gbs = [fe.grid_bounds(*km.SIZES[k]) for k in range(K)]
    kps, desc, ur, off = km.cat(sc)
    kw = dict(inv_sigma2=None if gate == "none" else sc["inv_sigma2"], ctx=ctx)
    for th in km.TH_VALUES:
        p = ref.keyframe_side([ref.view(**v) for v in sc["views"]], *km.geom(sc), th)
        bi, bd = fe.FuseKeyFrames(views, gbs, kps, desc, off, *km.geom(sc), sc["mp_desc"], th=th, uright=ur if gate == "stereo" else None, **kw)
        for k in range(K):
            want = km.batch_model(sc, p, gate, k)
            _rows_equal((bi[k], bd[k]), want, "K = 3, th %r, keyframe %d" % (th, k))
            urk = sc["uright"][k] if gate == "stereo" else None
            one = fe.FuseKeyFrames(views[k:k + 1], gbs[k:k + 1], sc["kps"][k], sc["desc"][k], np.int32([0, len(sc["kps"][k])]), *km.geom(sc), sc["mp_desc"],
                                   th=th, uright=urk, **kw)
            _rows_equal((one[0][0], one[1][0]), want, "K = 1, th %r, keyframe %d" % (th, k))
            if len(sc["kps"][k]):
                _rows_equal(fe.FusePose(sc["kps"][k], sc["desc"][k], gbs[k], views[k], *km.geom(sc), sc["mp_desc"], th=th, uright=urk, **kw), want,
                            "FusePose, th %r, keyframe %d" % (th, k))


@pytest.mark.parametrize("gate", ["mono", "stereo", "none"])
def test_fuse_keyframes_mixed_k3_with_edge_values(oracle, fe, ctx, gate):
    """FuseKeyFramesMixed, K = 3, the same scene with mixed rows and points; the projection is tests/kfside_mixed_ref's"""
    mref.use_oracle(oracle)
    sc = km.batch_scene(mixed=True)
    K = 3
    views = [fe.view(**kw) for kw in sc["views"]]
    gbs = [fe.grid_bounds(*km.SIZES[k]) for k in range(K)]
    kps, desc, ur, off = km.cat(sc)
    kio = np.concatenate(sc["kp_is_orb"]); sig = np.concatenate(sc["kp_inv_sigma2"])
    hits = 0
    for th in km.TH_VALUES:
        p = mref.keyframe_side([mref.view(**v) for v in sc["views"]], *km.geom(sc), th, mp_is_orb=sc["mp_is_orb"])
        bi, bd = fe.FuseKeyFramesMixed(views, gbs, kps, desc, off, *km.geom(sc), sc["mp_desc"], kp_is_orb=kio, kp_inv_sigma2=None if gate == "none" else sig,
                                       mp_is_orb=sc["mp_is_orb"], th=th, uright=ur if gate == "stereo" else None, ctx=ctx)
        for k in range(K):
            want = km.batch_model(sc, p, gate, k)
            _rows_equal((bi[k], bd[k]), want, "mixed K = 3, th %r, keyframe %d" % (th, k))
            hits += int((want[0] >= 0).sum())
            kw = dict(kp_is_orb=sc["kp_is_orb"][k], kp_inv_sigma2=None if gate == "none" else sc["kp_inv_sigma2"][k], mp_is_orb=sc["mp_is_orb"], th=th,
                      uright=sc["uright"][k] if gate == "stereo" else None, ctx=ctx)
            one = fe.FuseKeyFramesMixed(views[k:k + 1], gbs[k:k + 1], sc["kps"][k], sc["desc"][k], np.int32([0, len(sc["kps"][k])]), *km.geom(sc),
                                        sc["mp_desc"], **kw)
            _rows_equal((one[0][0], one[1][0]), want, "mixed K = 1, th %r, keyframe %d" % (th, k))
            if len(sc["kps"][k]):
                _rows_equal(fe.FusePoseMixed(sc["kps"][k], sc["desc"][k], gbs[k], views[k], *km.geom(sc), sc["mp_desc"], **kw), want,
                            "FusePoseMixed, th %r, keyframe %d" % (th, k))
    assert hits >= 30


def test_search_by_projection_kf_scw_mixed_in_order(oracle, fe, ctx):
    """eorb_search_by_projection_kf_scw_mixed on keyframe 1 of the mixed K = 3 scene: the mixed projection with the AKAZE tables, then the
    type gate, class_id levels and the taken flags together"""
    mref.use_oracle(oracle)
    sc = km.batch_scene(mixed=True)
    k = 1
    taken = (np.arange(len(sc["kps"][k])) % 5 == 0).astype(np.uint8)
    p = mref.keyframe_side([mref.view(**v) for v in sc["views"]], *km.geom(sc), 4.0, mp_is_orb=sc["mp_is_orb"])
    for ratio in (1.0, 0.75):
        want = km.batch_model(sc, p, "none", k, taken=taken, accept_thr=float(np.float32(50) * np.float32(ratio)))
        got = fe.SearchByProjectionKFScwMixed(sc["kps"][k], sc["desc"][k], fe.grid_bounds(*km.SIZES[k]), fe.view(**sc["views"][k]), *km.geom(sc),
                                              sc["mp_desc"], taken, 4.0, kp_is_orb=sc["kp_is_orb"][k], mp_is_orb=sc["mp_is_orb"], ratioHamming=ratio, ctx=ctx)
        _rows_equal(got, want, "kf_scw mixed ratio %r" % ratio)
        assert np.array_equal(got[2], want[2]) and (want[2] != taken).sum() >= 10
        info = {}
        km.batch_model(sc, p, "none", k, taken=taken, accept_thr=50.0, info=info)
        assert info["probe"]["other type"] > 0 and info["probe"]["class_id level != octave"] > 0 and info["probe"]["taken met"] > 0


def test_search_by_projection_kf_scw_in_order(fe, ctx, ref):
    """eorb_search_by_projection_kf_scw on keyframe 1 of the K = 3 scene: the projection, then the in-order form with taken flags"""
    sc = km.batch_scene()
    k = 1
    taken = (np.arange(len(sc["kps"][k])) % 5 == 0).astype(np.uint8)
    for ratio in (1.0, 0.75):
        p = ref.keyframe_side([ref.view(**v) for v in sc["views"]], *km.geom(sc), 4.0)
        want = km.batch_model(sc, p, "none", k, taken=taken, accept_thr=float(np.float32(50) * np.float32(ratio)))
        got = fe.SearchByProjectionKFScw(sc["kps"][k], sc["desc"][k], fe.grid_bounds(*km.SIZES[k]), fe.view(**sc["views"][k]), *km.geom(sc), sc["mp_desc"],
                                         taken, 4.0, ratioHamming=ratio, ctx=ctx)
        _rows_equal(got, want, "kf_scw ratio %r" % ratio)
        assert np.array_equal(got[2], want[2]) and (want[2] != taken).sum() >= 10


def test_second_trip_of_the_grid_stride_loop_with_k5(fe, ctx, ref):
    """K * M = 5 x 6 600 = 33 000 > 32 768 on keyframes of 40 keypoints, each on its own grid: the batch kernel's second trip, where a wrong
    keyframe of a query (k = q / M, kf_off[k], g[k]) would show; every query against the model"""
    sc = km.batch_scene(K=5, M=6600, n_kps=(40, 40, 40, 40, 40), seed=62, edges=False)
    K, M = 5, 6600
    kps, desc, ur, off = km.cat(sc)
    p = ref.keyframe_side([ref.view(**v) for v in sc["views"]], *km.geom(sc), 3.0)
    bi, bd = fe.FuseKeyFrames([fe.view(**kw) for kw in sc["views"]], [fe.grid_bounds(*km.SIZES[k]) for k in range(K)], kps, desc, off, *km.geom(sc),
                              sc["mp_desc"], th=3.0, ctx=ctx)
    found = []
    for k in range(K):
        want = km.batch_model(sc, p, "none", k)
        _rows_equal((bi[k], bd[k]), want, "keyframe %d" % k)
        found.append(int((want[0] >= 0).sum()))
    assert K * M > 4 * 8192 and min(found) >= 5 and (np.asarray(bi[4][M - 232:]) >= 0).any(), found       # (queries 32 768 .. 32 999 are the second trip)


def test_search_by_sim3_agreement(fe, ctx, ref):
    """eorb_search_by_sim3 with th_high on both sides of a pair's two distances: both searches and sim3_agree_kernel against the model"""
    sp = km.sim3_scene()
    p12, p21 = km.sim3_projections(ref, sp)
    bi1, bd1, bi2, bd2 = km.sim3_searches(sp, p12, p21)
    gb = fe.grid_bounds(sp["W"], sp["H"])
    kf = [dict(k, gb=gb, view=fe.view(**k["view"])) for k in (sp["kf1"], sp["kf2"])]
    for th_high in km.sim3_th_values(bd1, bd2, bi1, bi2):
        n, m12, vn1, vn2 = km.sim3_agree(bi1, bd1, bi2, bd2, th_high)
        nf, g12, g1, g2 = fe.SearchBySim3Pose(kf[0], kf[1], sp["sR12"], sp["t12"], sp["sR21"], sp["t21"], th=7.5, th_high=th_high, ctx=ctx)
        assert np.array_equal(g1, vn1) and np.array_equal(g2, vn2) and np.array_equal(g12, m12) and nf == n, th_high
