"""KeyFrame-side matchers for mixed ORB + AKAZE keyframes (GPU): eorb_project_keyframe_side_mixed, eorb_kf_radius_match_mixed,
eorb_fuse_pose_mixed, eorb_search_by_projection_kf_scw_mixed and eorb_fuse_keyframes_mixed against the CPU restatement of MixedMatcher
(tests/kfside_mixed_ref), byte for byte.  tests/test_kfside_mixed_ref.py asserts, without a GPU, that the scene used here makes the
type gate, the keypoint level and the per-keypoint sigma each decide results."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfside_mixed_cases as cases                  # noqa: E402
import kfside_mixed_ref as mref                     # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = cases.W, cases.H
E_CAPACITY, E_ARG = -3, -4
TH_LOW = cases.TH_LOW
KB8 = (226.38018519795807, 226.15002947047415, 173.6470807871759, 133.73271487507847,
       -0.048031442223833355, 0.011330957517194437, -0.055378166304281135, 0.021500973881459395)
PROJ = [f[0] for f in mref.OUT_FIELDS]
AK_SF, AK_LOGS = synth.akaze_tables()


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
def ref(oracle):
    return mref.use_oracle(oracle)


def _eq(got, want, keys=PROJ):
    for k in keys:
        assert got[k].tobytes() == want[k].tobytes(), k


def _same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), i


def _cat(sc):
    off = np.concatenate([[0], np.cumsum([len(k) for k in sc["kps"]])]).astype(np.int32)
    return (np.concatenate(sc["kps"]), np.concatenate(sc["desc"]), np.concatenate(sc["uright"]), np.concatenate(sc["kp_is_orb"]),
            np.concatenate(sc["kp_inv_sigma2"]), off)


# ---- mode D with the tables picked per point ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 1000])
@pytest.mark.parametrize("cfg", ["pinhole", "kb8", "skip"])
def test_mixed_projection_equals_the_restatement(fe, ctx, ref, M, cfg):
    s = synth.map_scene(41, M)
    kw = dict(R=s["R"], t=s["t"], Ow=s["Ow"], cam=KB8 if cfg == "kb8" else s["cam"], bounds=s["bounds"], nlevels=s["nlevels"],
              log_scale=s["log_scale"], scale_factors=s["scale_factors"], mbf=35.0, ak_nlevels=16, ak_log_scale=AK_LOGS, ak_scale_factors=AK_SF)
    mio = (np.random.default_rng(7).random(M) >= 1 / 3).astype(np.uint8)
    skip = (np.arange(M) % 3 == 2).astype(np.uint8) if cfg == "skip" else None
    g = (s["pos"], s["normal"], s["min_dist"], s["max_dist"])
    want = ref.keyframe_side(ref.view(**kw), *g, 3.0, mp_is_orb=mio, skip=skip)
    got = fe.ProjectKeyFrameSideMixed(fe.view(**kw), *g, 3.0, mp_is_orb=mio, skip=skip, ctx=ctx)
    _eq(got, want)
    if M == 1000:
        ak = (want["valid"] == 1) & (mio == 0)
        lv = np.unique(want["level"][ak])
        print("AKAZE points accepted", int(ak.sum()), "levels", lv.tolist())
        assert ak.sum() >= 20 and len(lv) >= 6 and lv.max() > 7
        # the ORB-only projector gives these points other levels and radii
        orb = fe.ProjectKeyFrameSide(fe.view(**kw), *g, 3.0, skip=skip, ctx=ctx)
        assert int((orb["level"][ak] != want["level"][ak]).sum()) >= 5 and np.all(orb["level"][mio == 1] == want["level"][mio == 1])


# ---- eorb_kf_radius_match_mixed alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 65, 1000])
@pytest.mark.parametrize("n", [0, 1, 64, 65, 1000])
def test_mixed_radius_match_equals_the_restatement(fe, ctx, ref, oracle, n, M):
    sc = cases.scene()
    p = {a: v[:M] for a, v in cases.projection(3.0)[0].items()}
    gb = fe.grid_bounds(W, H)
    q = (p["valid"], p["uv"], p["radius"], p["level"], sc["mp_desc"][:M])
    for gate in cases.GATES:
        want = cases.search(oracle, sc, 0, p, gate, n=n, m=M)
        kw = cases.gate_kw(sc, 0, gate, n)
        kw["mp_is_orb"] = kw["mp_is_orb"][:M]
        got = fe.KeyFrameRadiusMatchMixed(sc["kps"][0][:n], sc["desc"][0][:n], gb, *q, q_ur=p["q_ur"] if gate == "stereo" else None, ctx=ctx, **kw)
        _same(got, want)
    # the in-order form with some flags preset
    taken = (np.random.default_rng(3).random(n) < 0.2).astype(np.uint8)
    want = cases.search(oracle, sc, 0, p, "none", n=n, m=M, taken=taken, accept_thr=50.0)
    kw = cases.gate_kw(sc, 0, "none", n)
    kw["mp_is_orb"] = kw["mp_is_orb"][:M]
    got = fe.KeyFrameRadiusMatchMixed(sc["kps"][0][:n], sc["desc"][0][:n], gb, *q, taken=taken, accept_thr=50.0, ctx=ctx, **kw)
    _same(got, want)
    if n == 1000 and M == 1000:
        assert int(want[2].sum()) - int(taken.sum()) >= 30 and np.all(want[2][taken == 1] == 1)
        free = cases.search(oracle, sc, 0, p, "none", taken=np.zeros(n, np.uint8), accept_thr=50.0)
        assert int((free[0] != want[0]).sum()) >= 5                          # the flags matter


def test_akaze_rows_are_compared_on_their_first_32_bytes_at_the_callers_stride(fe, ctx, oracle):
    sc = cases.scene()
    p = cases.projection(3.0)[0]
    wide = np.concatenate([sc["desc"][0], synth.random_descriptors(cases.N, seed=9, width=29)], axis=1)      # 61-byte rows
    want = cases.search(oracle, sc, 0, p, "mono")
    got = fe.KeyFrameRadiusMatchMixed(sc["kps"][0], wide, fe.grid_bounds(W, H), p["valid"], p["uv"], p["radius"], p["level"], sc["mp_desc"],
                                      ctx=ctx, **cases.gate_kw(sc, 0, "mono"))
    _same(got, want)


# ---- the fused forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th", [3.0, 4.0])
@pytest.mark.parametrize("gate", cases.GATES)
def test_fuse_pose_mixed(fe, ctx, ref, oracle, th, gate):
    sc = cases.scene()
    p = cases.projection(th)[0]
    want = cases.search(oracle, sc, 0, p, gate)
    gb = fe.grid_bounds(W, H)
    v = fe.view(**sc["views"][0])
    kw = cases.gate_kw(sc, 0, gate)
    for _ in range(2):                                                      # the second call reuses the context's arena
        bi, bd, g = fe.FusePoseMixed(sc["kps"][0], sc["desc"][0], gb, v, *cases.geom(sc), sc["mp_desc"], th=th, want_projection=True, ctx=ctx, **kw)
        _eq(g, p)
        _same((bi, bd), want)
    _same(fe.FusePoseMixed(sc["kps"][0], sc["desc"][0], gb, v, *cases.geom(sc), sc["mp_desc"], th=th, ctx=ctx, **kw), want)
    # the product's own two calls
    q = fe.ProjectKeyFrameSideMixed(v, *cases.geom(sc), th, mp_is_orb=sc["mp_is_orb"], ctx=ctx)
    two = fe.KeyFrameRadiusMatchMixed(sc["kps"][0], sc["desc"][0], gb, q["valid"], q["uv"], q["radius"], q["level"], sc["mp_desc"],
                                      q_ur=q["q_ur"] if gate == "stereo" else None, ctx=ctx, **kw)
    _same(two, (bi, bd))
    is_orb = sc["mp_is_orb"] == 1
    acc = want[1] <= TH_LOW
    print("fuse_pose_mixed", th, gate, "accepted", int((acc & is_orb).sum()), int((acc & ~is_orb).sum()))
    assert (acc & is_orb).sum() >= 20 and (acc & ~is_orb).sum() >= 20
    if gate != "none":
        assert int((cases.search(oracle, sc, 0, p, "none")[0] != want[0]).sum()) >= 5      # the reprojection gate changes results


@pytest.mark.parametrize("ratio", [1.0, 1.5])
def test_search_by_projection_kf_scw_mixed(fe, ctx, ref, oracle, ratio):
    sc = cases.scene()
    th = 4.0
    taken = (np.random.default_rng(3).random(cases.N) < 0.2).astype(np.uint8)
    skip = cases.skip_of("every13", 1, cases.M)
    p = cases.projection(th, skip_key="every13")[0]
    thr = float(F32(TH_LOW) * F32(ratio))
    want = cases.search(oracle, sc, 0, p, "none", taken=taken, accept_thr=thr)
    gb = fe.grid_bounds(W, H)
    v = fe.view(**sc["views"][0])
    flags = dict(kp_is_orb=sc["kp_is_orb"][0], mp_is_orb=sc["mp_is_orb"])
    bi, bd, tk, g = fe.SearchByProjectionKFScwMixed(sc["kps"][0], sc["desc"][0], gb, v, *cases.geom(sc), sc["mp_desc"], taken, th,
                                                    ratioHamming=ratio, skip=skip, want_projection=True, ctx=ctx, **flags)
    _eq(g, p)
    _same((bi, bd, tk), want)
    q = fe.ProjectKeyFrameSideMixed(v, *cases.geom(sc), th, mp_is_orb=sc["mp_is_orb"], skip=skip, ctx=ctx)
    two = fe.KeyFrameRadiusMatchMixed(sc["kps"][0], sc["desc"][0], gb, q["valid"], q["uv"], q["radius"], q["level"], sc["mp_desc"], taken=taken,
                                      accept_thr=thr, ctx=ctx, **flags)
    _same(two, (bi, bd, tk))
    newly = int(want[2].sum()) - int(taken.sum())
    print("kf_scw_mixed", ratio, "accepted", int((want[1] <= thr).sum()), "newly taken", newly)
    assert newly >= 30


# ---- eorb_fuse_keyframes_mixed ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 8])
def test_fuse_keyframes_mixed_equals_k_calls_of_fuse_pose_mixed(fe, ctx, ref, oracle, K):
    n_kps, kinds = cases.BATCH[K]
    M = cases.M
    sc = cases.scene(49, K, M, n_kps, kinds)
    gate = {1: "mono", 3: "none", 8: "stereo"}[K]
    th = 3.0
    skip_key = "random10" if K == 8 else None
    skip = cases.skip_of(skip_key, K, M)
    kps, desc, ur, kio, sig, off = _cat(sc)
    gb = fe.grid_bounds(W, H)
    views = [fe.view(**kw) for kw in sc["views"]]
    kw = dict(kp_is_orb=kio, mp_is_orb=sc["mp_is_orb"], kp_inv_sigma2=None if gate == "none" else sig, uright=ur if gate == "stereo" else None)
    bi, bd, rs = fe.FuseKeyFramesMixed(views, [gb] * K, kps, desc, off, *cases.geom(sc), sc["mp_desc"], th=th, skip=skip, want_reason=True,
                                       ctx=ctx, **kw)
    _same(fe.FuseKeyFramesMixed(views, [gb] * K, kps, desc, off, *cases.geom(sc), sc["mp_desc"], th=th, skip=skip, ctx=ctx, **kw), (bi, bd))
    proj = cases.projection(th, 49, K, M, n_kps, kinds, skip_key)
    acc = []
    for k in range(K):
        got = fe.FusePoseMixed(sc["kps"][k], sc["desc"][k], gb, views[k], *cases.geom(sc), sc["mp_desc"], th=th,
                               skip=None if skip is None else skip[k * M:(k + 1) * M], want_projection=True, ctx=ctx, **cases.gate_kw(sc, k, gate))
        assert bi[k].tobytes() == got[0].tobytes() and bd[k].tobytes() == got[1].tobytes() and rs[k].tobytes() == got[2]["reason"].tobytes(), k
        want = cases.search(oracle, sc, k, proj[k], gate)
        assert bi[k].tobytes() == want[0].tobytes() and bd[k].tobytes() == want[1].tobytes() and rs[k].tobytes() == proj[k]["reason"].tobytes(), k
        acc.append(int((want[1] <= TH_LOW).sum()))
    print("fuse_keyframes_mixed", K, "accepted per keyframe", acc)
    assert all(a == 0 for a, n in zip(acc, n_kps) if n == 0) and all(a >= 20 for a, n in zip(acc, n_kps) if n >= 500)
    is_orb = sc["mp_is_orb"] == 1
    for k, kind in enumerate(kinds):                                        # an all-ORB keyframe takes no AKAZE point, and the reverse
        if kind == "orb":
            assert np.all(bi[k][~is_orb] == -1)
        if kind == "akaze":
            assert np.all(bi[k][is_orb] == -1)


# ---- nothing mixed: the ORB entry points' bytes -------------------------------------------------------------------------------------
def test_with_every_flag_null_the_mixed_functions_return_their_orb_counterparts_bytes(fe, ctx):
    K, M = 3, 1000
    sc = synth.keyframe_neighbourhood(43, K, M, n_kps=[1000, 0, 640])
    g = (sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"])
    gb = fe.grid_bounds(W, H)
    views = [fe.view(**kw) for kw in sc["views"]]
    sig = [sc["inv_sigma2"][k["octave"]] for k in sc["kps"]]
    k0, d0, u0 = sc["kps"][0], sc["desc"][0], sc["uright"][0]
    a = fe.ProjectKeyFrameSide(views[0], *g, 3.0, ctx=ctx)
    _eq(fe.ProjectKeyFrameSideMixed(views[0], *g, 3.0, ctx=ctx), a)
    q = (a["valid"], a["uv"], a["radius"], a["level"], sc["mp_desc"])
    _same(fe.KeyFrameRadiusMatchMixed(k0, d0, gb, *q, ctx=ctx), fe.KeyFrameRadiusMatch(k0, d0, gb, *q, ctx=ctx))
    _same(fe.KeyFrameRadiusMatchMixed(k0, d0, gb, *q, kp_inv_sigma2=sig[0], ctx=ctx), fe.KeyFrameRadiusMatch(k0, d0, gb, *q, inv_sigma2=sc["inv_sigma2"], ctx=ctx))
    _same(fe.KeyFrameRadiusMatchMixed(k0, d0, gb, *q, kp_inv_sigma2=sig[0], uright=u0, q_ur=a["q_ur"], ctx=ctx),
          fe.KeyFrameRadiusMatch(k0, d0, gb, *q, inv_sigma2=sc["inv_sigma2"], uright=u0, q_ur=a["q_ur"], ctx=ctx))
    taken = (np.random.default_rng(3).random(1000) < 0.2).astype(np.uint8)
    _same(fe.KeyFrameRadiusMatchMixed(k0, d0, gb, *q, taken=taken, accept_thr=50.0, ctx=ctx),
          fe.KeyFrameRadiusMatch(k0, d0, gb, *q, taken=taken, accept_thr=50.0, ctx=ctx))
    for isg, s, ur in ((None, None, None), (sc["inv_sigma2"], sig[0], None), (sc["inv_sigma2"], sig[0], u0)):
        w = fe.FusePose(k0, d0, gb, views[0], *g, sc["mp_desc"], inv_sigma2=isg, uright=ur, want_projection=True, ctx=ctx)
        m = fe.FusePoseMixed(k0, d0, gb, views[0], *g, sc["mp_desc"], kp_inv_sigma2=s, uright=ur, want_projection=True, ctx=ctx)
        _same(m[:2], w[:2]); _eq(m[2], w[2])
        assert int((w[1] <= TH_LOW).sum()) >= 30
    w = fe.SearchByProjectionKFScw(k0, d0, gb, views[0], *g, sc["mp_desc"], taken, 4.0, ratioHamming=1.5, ctx=ctx)
    _same(fe.SearchByProjectionKFScwMixed(k0, d0, gb, views[0], *g, sc["mp_desc"], taken, 4.0, ratioHamming=1.5, ctx=ctx), w)
    kps = np.concatenate(sc["kps"]); desc = np.concatenate(sc["desc"]); ur = np.concatenate(sc["uright"])
    off = np.concatenate([[0], np.cumsum([len(k) for k in sc["kps"]])]).astype(np.int32)
    w = fe.FuseKeyFrames(views, [gb] * K, kps, desc, off, *g, sc["mp_desc"], inv_sigma2=sc["inv_sigma2"], uright=ur, want_reason=True, ctx=ctx)
    _same(fe.FuseKeyFramesMixed(views, [gb] * K, kps, desc, off, *g, sc["mp_desc"], kp_inv_sigma2=np.concatenate(sig), uright=ur, want_reason=True,
                                ctx=ctx), w)


# ---- the feature decides ------------------------------------------------------------------------------------------------------------
def test_the_orb_only_fuse_gives_other_answers_on_the_mixed_scene(fe, ctx, oracle):
    """tests/test_kfside_mixed_ref.py guarantees at least 5 queries of this scene for each of the type gate, the level and the sigma"""
    sc = cases.scene()
    gb = fe.grid_bounds(W, H)
    v = fe.view(**sc["views"][0])
    mixed = fe.FusePoseMixed(sc["kps"][0], sc["desc"][0], gb, v, *cases.geom(sc), sc["mp_desc"], ctx=ctx, **cases.gate_kw(sc, 0, "mono"))
    orb = fe.FusePose(sc["kps"][0], sc["desc"][0], gb, v, *cases.geom(sc), sc["mp_desc"], inv_sigma2=sc["inv_sigma2"], ctx=ctx)
    differ = int(((mixed[0] != orb[0]) | (mixed[1] != orb[1])).sum())
    print("rows that differ", differ)
    assert differ >= 5


# ---- arguments, empty sides, limits -------------------------------------------------------------------------------------------------
def test_mixed_argument_errors_empty_sides_and_limits(fe, ctx):
    sc = cases.scene()
    L, h = ctx.L, ctx.h
    v = fe.view(**sc["views"][0])
    gb = fe.grid_bounds(W, H)
    c = np.ascontiguousarray
    kps, desc, ur = c(sc["kps"][0]), c(sc["desc"][0]), c(sc["uright"][0])
    kio, sig, mio = c(sc["kp_is_orb"][0]), c(sc["kp_inv_sigma2"][0]), c(sc["mp_is_orb"])
    pos, nrm, mn, mx = [c(a) for a in cases.geom(sc)]
    qd = c(sc["mp_desc"])
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    M, n = cases.M, cases.N
    bi = np.full(M, 7, np.int32); bd = np.full(M, 7, np.int32)

    def fuse_ok():
        assert L.eorb_fuse_pose_mixed(h, p(kps), n, p(desc), 32, C.byref(gb), p(kio), p(sig), None, C.byref(v), M, p(pos), p(nrm), p(mn), p(mx),
                                      p(mio), None, p(qd), 3.0, p(bi), p(bd), None) == 0
        assert (bd <= TH_LOW).sum() >= 40
    fuse_ok()
    # a stereo gate without sigmas
    assert L.eorb_fuse_pose_mixed(h, p(kps), n, p(desc), 32, C.byref(gb), p(kio), None, p(ur), C.byref(v), M, p(pos), p(nrm), p(mn), p(mx),
                                  p(mio), None, p(qd), 3.0, p(bi), p(bd), None) == E_ARG
    fuse_ok()
    pr = cases.projection(3.0)[0]
    va, uv, rad, lv, qur = c(pr["valid"]), c(pr["uv"]), c(pr["radius"]), c(pr["level"]), c(pr["q_ur"])
    assert L.eorb_kf_radius_match_mixed(h, p(kps), n, p(desc), 32, C.byref(gb), p(kio), None, p(ur), M, p(va), p(uv), p(rad), p(lv), p(qd),
                                        p(mio), p(qur), None, 0.0, p(bi), p(bd)) == E_ARG
    assert L.eorb_kf_radius_match_mixed(h, p(kps), n, p(desc), 32, C.byref(gb), p(kio), p(sig), p(ur), M, p(va), p(uv), p(rad), p(lv), p(qd),
                                        p(mio), None, None, 0.0, p(bi), p(bd)) == E_ARG           # uright without q_ur
    assert L.eorb_kf_radius_match_mixed(h, p(kps), n, p(desc), 16, C.byref(gb), p(kio), p(sig), None, M, p(va), p(uv), p(rad), p(lv), p(qd),
                                        p(mio), None, None, 0.0, p(bi), p(bd)) == E_ARG
    assert L.eorb_kf_radius_match_mixed(h, p(kps), n, p(desc), 32, C.byref(gb), p(kio), p(sig), None, M, p(va), p(uv), p(rad), p(lv), p(qd),
                                        p(mio), None, None, 0.0, p(bi), p(bd)) == 0
    assert (bd <= TH_LOW).sum() >= 40
    assert L.eorb_project_keyframe_side_mixed(h, None, M, p(pos), p(nrm), p(mn), p(mx), p(mio), None, 3.0, None) == E_ARG
    assert L.eorb_project_keyframe_side_mixed(h, C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), p(mio), None, 3.0, None) == 0
    assert L.eorb_search_by_projection_kf_scw_mixed(h, p(kps), n, p(desc), 32, C.byref(gb), p(kio), C.byref(v), M, p(pos), p(nrm), p(mn), p(mx),
                                                    p(mio), None, p(qd), 4.0, None, 50.0, p(bi), p(bd), None) == E_ARG      # no taken flags
    # a batch whose views name different AKAZE pyramids, or different ORB ones
    kw = dict(sc["views"][0]); kw["ak_log_scale"] = float(AK_LOGS) * 1.5
    other = fe.view(**kw)
    kw = dict(sc["views"][0]); kw["ak_nlevels"] = 12
    fewer = fe.view(**kw)
    g2 = (type(gb) * 2)(gb, gb)
    off = np.array([0, n, n], np.int32)
    bi2 = np.zeros(2 * M, np.int32); bd2 = np.zeros(2 * M, np.int32)

    def batch(v0, v1, K=2, m=M, o=off):
        return L.eorb_fuse_keyframes_mixed(h, (type(v) * 2)(v0, v1), g2, K, p(kps), p(desc), 32, p(kio), p(sig), None, p(o), m, p(pos), p(nrm),
                                           p(mn), p(mx), p(mio), p(qd), None, 3.0, p(bi2), p(bd2), None)
    assert batch(v, other) == E_ARG and b"AKAZE pyramid" in L.eorb_last_error(h)
    assert batch(v, v) == 0 and (bd2[:M] <= TH_LOW).sum() >= 40 and np.all(bd2[M:] == 256)
    assert batch(v, fewer) == E_ARG
    assert batch(v, v) == 0
    # empty sides: EORB_OK, outputs untouched (no queries) or -1-filled (no keypoints)
    bi[:] = 7; bd[:] = 7
    assert L.eorb_fuse_pose_mixed(h, p(kps), n, p(desc), 32, C.byref(gb), p(kio), p(sig), None, C.byref(v), 0, None, None, None, None,
                                  None, None, None, 3.0, p(bi), p(bd), None) == 0
    assert np.all(bi == 7) and np.all(bd == 7)
    assert L.eorb_fuse_pose_mixed(h, None, 0, None, 32, C.byref(gb), None, None, None, C.byref(v), M, p(pos), p(nrm), p(mn), p(mx),
                                  p(mio), None, p(qd), 3.0, p(bi), p(bd), None) == 0
    assert np.all(bi == -1) and np.all(bd == 256)
    assert L.eorb_fuse_keyframes_mixed(h, None, None, 0, None, None, 32, None, None, None, None, M, p(pos), p(nrm), p(mn), p(mx), p(mio), p(qd),
                                       None, 3.0, None, None, None) == 0
    bi[:] = 7; bd[:] = 7
    assert L.eorb_kf_radius_match_mixed(h, None, 0, None, 32, C.byref(gb), None, None, None, M, p(va), p(uv), p(rad), p(lv), p(qd),
                                        p(mio), None, None, 0.0, p(bi), p(bd)) == 0
    assert np.all(bi == -1) and np.all(bd == 256)
    # capacity, by sizes only: nothing this large is allocated or read
    assert batch(v, v, 2, (1 << 21) + 1) == E_CAPACITY
    assert batch(v, v) == 0
    assert batch(v, v, 1025, 1) == E_CAPACITY
    assert batch(v, v, 1, M, np.array([0, (1 << 22) + 1], np.int32)) == E_CAPACITY
    assert L.eorb_project_keyframe_side_mixed(h, C.byref(v), (1 << 22) + 1, p(pos), p(nrm), p(mn), p(mx), p(mio), None, 3.0, None) == E_CAPACITY
    assert b"exceed" in L.eorb_last_error(h)
    # the in-order form keeps the capacity rule of its LDS flags: 160 KB less the 64 bytes of the reduction
    big = 160 * 1024 - 64 + 1
    zk = np.zeros(big, kps.dtype); zd = np.zeros((big, 32), np.uint8); tk = np.zeros(big, np.uint8)
    one = lambda a: c(a[:1])
    args = (1, p(one(va)), p(one(uv)), p(one(rad)), p(one(lv)), p(one(qd)), p(one(mio)), None)
    assert L.eorb_kf_radius_match_mixed(h, p(zk), big, p(zd), 32, C.byref(gb), None, None, None, *args, p(tk), 50.0, p(bi), p(bd)) == E_CAPACITY
    assert L.eorb_kf_radius_match_mixed(h, p(zk), big - 1, p(zd), 32, C.byref(gb), None, None, None, *args, p(tk), 50.0, p(bi), p(bd)) == 0
    fuse_ok()


# ---- a single keyframe is K = 1 of the batch: the shapes at which the shared path can go wrong ----------------------------------------
def _both(bi):
    return bool((bi >= 0).any()) and bool((bi < 0).any())


_CASES = {}


def _sub_case(oracle, n, M, th=4.0):
    """n rows and M points of the 1 000 x 1 000 mixed scene.  Row 0 is the keypoint that point 0 finds in the whole keyframe under every
    gate, so it finds it among fewer rows too; three quarters of the rows are such winners, the rest carry no point.  The points are
    the winners' own in turns with points nobody wins; the second half of the points repeats the first (in order the repeats lose
    their keypoints; beyond 1 000 points the first 128 repeat).  -> the sub-scene, its geometry and the restatement's projection of it"""
    if (n, M) in _CASES:
        return _CASES[n, M]
    sc = cases.scene()
    p = cases.projection(th)[0]
    src = sc["src"][0]
    wins = np.ones(cases.N, bool)
    for gate in cases.GATES:
        bi = cases.search(oracle, sc, 0, p, gate)[0]
        wins &= (src >= 0) & (bi[np.maximum(src, 0)] == np.arange(cases.N))
    rows = np.concatenate([np.flatnonzero(wins)[:max(1, (3 * n) // 4)], np.flatnonzero(src < 0)])[:n]
    won = src[rows[src[rows] >= 0]]
    rest = np.setdiff1d(np.arange(cases.M), won)
    pts = np.concatenate([np.stack([won, rest[:len(won)]], 1).reshape(-1), rest[len(won):]])      # won and not won take turns
    pts = np.resize(pts[:(M + 1) // 2 if M <= cases.M else 128], M)
    c = np.ascontiguousarray
    s = dict(kps=sc["kps"][0][rows], desc=c(sc["desc"][0][rows]), uright=sc["uright"][0][rows], kp_is_orb=sc["kp_is_orb"][0][rows],
             kp_inv_sigma2=sc["kp_inv_sigma2"][0][rows], mp_is_orb=sc["mp_is_orb"][pts], mp_desc=c(sc["mp_desc"][pts]),
             geom=tuple(c(a[pts]) for a in cases.geom(sc)), view=sc["views"][0])
    s["p"] = mref.keyframe_side(mref.view(**s["view"]), *s["geom"], th, mp_is_orb=s["mp_is_orb"])
    _CASES[n, M] = s
    return s


def _sub_kw(s, gate):
    kw = dict(kp_is_orb=s["kp_is_orb"], mp_is_orb=s["mp_is_orb"])
    if gate != "none":
        kw["kp_inv_sigma2"] = s["kp_inv_sigma2"]
    if gate == "stereo":
        kw["uright"] = s["uright"]
    return kw


def _sub_q(s):
    p = s["p"]
    return p["valid"], p["uv"], p["radius"], p["level"], s["mp_desc"]


def _sub_ref(oracle, s, gate, **extra):
    return mref.search(oracle.Frame(s["kps"], s["desc"], W, H), s["p"], s["mp_desc"], **_sub_kw(s, gate), **extra)


def _taken(n, seed):
    tk = (np.random.default_rng(seed).random(n) < 0.2).astype(np.uint8)
    tk[0] = 0                                                                              # (row 0 is what point 0 and its repeat want)
    return tk


@pytest.mark.parametrize("gate", cases.GATES)
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_mixed_independent_radius_search_lane_and_wave_edges(fe, ctx, ref, oracle, n, gate):
    """eorb_kf_radius_match_mixed: the lanes stride the keypoints by 64, four waves share a workgroup"""
    gb = fe.grid_bounds(W, H)
    hits = misses = 0
    for M in (1, 3, 4, 5, 257):
        s = _sub_case(oracle, n, M)
        want = _sub_ref(oracle, s, gate)
        got = fe.KeyFrameRadiusMatchMixed(s["kps"], s["desc"], gb, *_sub_q(s), q_ur=s["p"]["q_ur"] if gate == "stereo" else None, ctx=ctx,
                                          **_sub_kw(s, gate))
        _same(got, want)
        assert want[0][0] == 0 and (M < 257 or _both(want[0])), M
        hits += int((want[0] >= 0).sum()); misses += int((want[0] < 0).sum())
    print("mixed independent", n, gate, "hits", hits, "misses", misses)
    assert hits >= 5 and misses >= 50


def test_mixed_independent_radius_search_goes_round_the_grid_stride_loop(fe, ctx, ref, oracle):
    """K = 1 with more queries than the 8192 workgroups of four waves take in one round"""
    n, M = 65, 4 * 8192 + 5
    s = _sub_case(oracle, n, M)
    gb = fe.grid_bounds(W, H)
    for gate in cases.GATES:
        want = _sub_ref(oracle, s, gate)
        got = fe.KeyFrameRadiusMatchMixed(s["kps"], s["desc"], gb, *_sub_q(s), q_ur=s["p"]["q_ur"] if gate == "stereo" else None, ctx=ctx,
                                          **_sub_kw(s, gate))
        _same(got, want)
        assert _both(want[0]) and _both(want[0][4 * 8192:]), gate


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_mixed_in_order_searches(fe, ctx, ref, oracle, n):
    """eorb_kf_radius_match_mixed(taken, accept_thr) and eorb_search_by_projection_kf_scw_mixed on the same sub-scenes"""
    gb = fe.grid_bounds(W, H)
    taken = _taken(n, 3)
    for M in (1, 2, 65):
        s = _sub_case(oracle, n, M)
        free = _sub_ref(oracle, s, "none")
        v = fe.view(**s["view"])
        flags = dict(kp_is_orb=s["kp_is_orb"], mp_is_orb=s["mp_is_orb"])
        for ratio in (1.0, 0.8):
            thr = float(F32(TH_LOW) * F32(ratio))
            want = _sub_ref(oracle, s, "none", taken=taken, accept_thr=thr)
            _same(fe.KeyFrameRadiusMatchMixed(s["kps"], s["desc"], gb, *_sub_q(s), taken=taken, accept_thr=thr, ctx=ctx, **flags), want)
            bi, bd, tk, g = fe.SearchByProjectionKFScwMixed(s["kps"], s["desc"], gb, v, *s["geom"], s["mp_desc"], taken, 4.0, ratioHamming=ratio,
                                                            want_projection=True, ctx=ctx, **flags)
            _eq(g, s["p"])
            _same((bi, bd, tk), want)
            assert want[0][0] == 0 and want[2][0] == 1 and np.all(want[2][taken == 1] == 1)
            if M > 1:
                r = (M + 1) // 2                                                           # the first repeat: point 0 again
                assert free[0][r] == 0 and want[0][r] != 0                                 # in order it loses keypoint 0
            assert M < 65 or _both(want[0])                                                # (at M = 2 the repeat may find a second best)


def test_mixed_radius_search_profile_scopes_keep_the_entry_points_names(fe, ctx, ref, oracle):
    s = _sub_case(oracle, 65, 65)
    gb = fe.grid_bounds(W, H)
    v = fe.view(**s["view"])
    flags = dict(kp_is_orb=s["kp_is_orb"], mp_is_orb=s["mp_is_orb"])
    off = np.array([0, 65], np.int32)
    calls = [("kf_radius_match_mixed", lambda: fe.KeyFrameRadiusMatchMixed(s["kps"], s["desc"], gb, *_sub_q(s), ctx=ctx, **flags)),
             ("kf_radius_match_mixed", lambda: fe.KeyFrameRadiusMatchMixed(s["kps"], s["desc"], gb, *_sub_q(s), taken=_taken(65, 3), accept_thr=50.0,
                                                                           ctx=ctx, **flags)),
             ("kf_radius_match_mixed", lambda: fe.SearchByProjectionKFScwMixed(s["kps"], s["desc"], gb, v, *s["geom"], s["mp_desc"], _taken(65, 3), 4.0,
                                                                               ctx=ctx, **flags)),
             ("kf_radius_batch_mixed", lambda: fe.FusePoseMixed(s["kps"], s["desc"], gb, v, *s["geom"], s["mp_desc"], ctx=ctx, **flags)),
             ("kf_radius_batch_mixed", lambda: fe.FuseKeyFramesMixed([v], [gb], s["kps"], s["desc"], off, *s["geom"], s["mp_desc"], ctx=ctx, **flags))]
    ctx.prof_enable(True)
    try:
        for name, call in calls:
            ctx.prof_reset()
            call()
            got = {k: c[1] for k, c in ctx.prof_results().items() if k.startswith("kf_radius")}
            assert got == {name: 1}, (name, got)
    finally:
        ctx.prof_enable(False)


def test_mixed_one_keyframe_without_keypoints(fe, ctx, ref, oracle):
    """K = 1 with kf_off = {0, 0}: EORB_OK, -1 / 256 everywhere, no keypoint read (every keypoint pointer is NULL)"""
    s = _sub_case(oracle, 65, 65)
    L, h = ctx.L, ctx.h
    v = fe.view(**s["view"]); gb = fe.grid_bounds(W, H)
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    pos, nrm, mn, mx = s["geom"]
    qd, mio = s["mp_desc"], np.ascontiguousarray(s["mp_is_orb"])
    M = 65
    va, uv, rad, lv = [np.ascontiguousarray(s["p"][k]) for k in ("valid", "uv", "radius", "level")]
    out = lambda: (np.full(M, 7, np.int32), np.full(M, 7, np.int32))
    bi, bd = out()
    assert L.eorb_kf_radius_match_mixed(h, None, 0, None, 32, C.byref(gb), None, None, None, M, p(va), p(uv), p(rad), p(lv), p(qd), p(mio), None,
                                        None, 0.0, p(bi), p(bd)) == 0
    assert np.all(bi == -1) and np.all(bd == 256)
    bi, bd = out()
    assert L.eorb_fuse_pose_mixed(h, None, 0, None, 32, C.byref(gb), None, None, None, C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), p(mio), None,
                                  p(qd), 3.0, p(bi), p(bd), None) == 0
    assert np.all(bi == -1) and np.all(bd == 256)
    for tk in (None, np.zeros(1, np.uint8)):                                               # no flags, or flags of no keypoint
        bi, bd = out()
        assert L.eorb_search_by_projection_kf_scw_mixed(h, None, 0, None, 32, C.byref(gb), None, C.byref(v), M, p(pos), p(nrm), p(mn), p(mx),
                                                        p(mio), None, p(qd), 4.0, p(tk), 50.0, p(bi), p(bd), None) == 0
        assert np.all(bi == -1) and np.all(bd == 256) and (tk is None or tk[0] == 0)
