"""KeyFrame-side matchers with the projection on the device (GPU): eorb_project_keyframe_side, eorb_fuse_pose,
eorb_search_by_projection_kf_scw, eorb_search_by_sim3 and eorb_fuse_keyframes -- the projection half against the CPU restatement
(tests/kfside_ref), the search half against the oracle's radius match fed with the restatement's outputs, bit for bit."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfside_ref                                   # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 346, 260
E_CONFIG, E_CAPACITY, E_ARG = -2, -3, -4
TH_LOW, TH_HIGH = 50, 100
KB8 = (226.38018519795807, 226.15002947047415, 173.6470807871759, 133.73271487507847,
       -0.048031442223833355, 0.011330957517194437, -0.055378166304281135, 0.021500973881459395)
PROJ = [f[0] for f in kfside_ref.OUT_FIELDS]


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
    kfside_ref.use_oracle_camera(oracle)
    return kfside_ref


def _eq(got, want, keys):
    for k in keys:
        assert got[k].tobytes() == want[k].tobytes(), k


@functools.lru_cache(None)
def _nbh(seed, K, M, n_kps, cam=None):
    return synth.keyframe_neighbourhood(seed, K, M, n_kps=list(n_kps), cam=cam)


def _geom(sc):
    return sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"]


def _cat(sc):
    off = np.concatenate([[0], np.cumsum([len(k) for k in sc["kps"]])]).astype(np.int32)
    return np.concatenate(sc["kps"]), np.concatenate(sc["desc"]), np.concatenate(sc["uright"]), off


def _ref_search(oracle, sc, k, p, q_desc, gate, taken=None, accept_thr=0.0):
    """the oracle's radius match in keyframe k over the restatement's projection p"""
    M = len(p["valid"])
    if len(sc["kps"][k]) == 0:
        return np.full(M, -1, np.int32), np.full(M, 256, np.int32)
    Fr = oracle.Frame(sc["kps"][k], sc["desc"][k], W, H)
    kw = dict(inv_sigma2=None if gate == "none" else sc["inv_sigma2"])
    if gate == "stereo":
        kw.update(uright=sc["uright"][k], q_ur=p["q_ur"])
    if taken is not None:
        kw.update(taken=taken, accept_thr=accept_thr)
    return oracle.kf_radius_match(Fr, p["valid"], p["uv"], p["radius"], p["level"], q_desc, **kw)


# ---- mode D alone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [0, 1, 63, 64, 65, 1000])
@pytest.mark.parametrize("cfg", ["pinhole", "kb8", "skip"])
def test_keyframe_side_projection_equals_the_restatement(fe, ctx, ref, M, cfg):
    s = synth.map_scene(41, M)
    kw = dict(R=s["R"], t=s["t"], Ow=s["Ow"], cam=KB8 if cfg == "kb8" else s["cam"], bounds=s["bounds"], nlevels=s["nlevels"],
              log_scale=s["log_scale"], scale_factors=s["scale_factors"], mbf=35.0)
    skip = (np.arange(M) % 3 == 2).astype(np.uint8) if cfg == "skip" else None
    want = ref.keyframe_side(ref.view(**kw), *_geom(s), 3.0, skip=skip)
    got = fe.ProjectKeyFrameSide(fe.view(**kw), *_geom(s), 3.0, skip=skip, ctx=ctx)
    _eq(got, want, PROJ)
    if M == 1000:
        cnt = np.bincount(want["reason"], minlength=8)
        print("reasons", cfg, cnt.tolist())
        assert all(cnt[r] >= 20 for r in (0, 2, 3, 5, 6)), cnt
        assert cnt[4] == cnt[7] == 0 and cnt[1] == (333 if cfg == "skip" else 0)
        assert len(np.unique(want["level"][want["valid"] == 1])) >= 6


# ---- eorb_fuse_pose -----------------------------------------------------------------------------------------------------------------
def _stereo_gate_decides(sc, k, p):
    """planted candidates that the two-term error would pass against 5.99 and the three-term error rejects against 7.8"""
    kp, src, ur = sc["kps"][k], sc["src"][k], sc["uright"][k]
    n = 0
    for i in np.flatnonzero((src >= 0) & (ur >= 0)):
        m = src[i]
        if not p["valid"][m] or not (p["level"][m] - 1 <= kp["octave"][i] <= p["level"][m]):
            continue
        ex = p["uv"][m, 0] - kp["x"][i]; ey = p["uv"][m, 1] - kp["y"][i]; er = p["q_ur"][m] - ur[i]
        if not (abs(ex) < p["radius"][m] and abs(ey) < p["radius"][m]):
            continue
        inv = sc["inv_sigma2"][kp["octave"][i]]
        n += bool(float((ex * ex + ey * ey) * inv) <= 5.99 and float((ex * ex + ey * ey + er * er) * inv) > 7.8)
    return n


@pytest.mark.parametrize("th", [3.0, 4.0])
@pytest.mark.parametrize("gate", ["mono", "stereo", "none"])
def test_fuse_pose(fe, ctx, ref, oracle, th, gate):
    sc = _nbh(43, 1, 1000, (1000,))
    kw = sc["views"][0]
    p = ref.keyframe_side(ref.view(**kw), *_geom(sc), th)
    wbi, wbd = _ref_search(oracle, sc, 0, p, sc["mp_desc"], gate)
    gb = fe.grid_bounds(W, H)
    v = fe.view(**kw)
    isg = None if gate == "none" else sc["inv_sigma2"]
    ur = sc["uright"][0] if gate == "stereo" else None
    for _ in range(2):                                                      # the second call reuses the context's arena
        bi, bd, g = fe.FusePose(sc["kps"][0], sc["desc"][0], gb, v, *_geom(sc), sc["mp_desc"], inv_sigma2=isg, th=th, uright=ur,
                                want_projection=True, ctx=ctx)
        _eq(g, p, PROJ)
        assert bi.tobytes() == wbi.tobytes() and bd.tobytes() == wbd.tobytes()
    bi2, bd2 = fe.FusePose(sc["kps"][0], sc["desc"][0], gb, v, *_geom(sc), sc["mp_desc"], inv_sigma2=isg, th=th, uright=ur, ctx=ctx)
    assert bi2.tobytes() == wbi.tobytes() and bd2.tobytes() == wbd.tobytes()
    # the product's own two calls
    q = fe.ProjectKeyFrameSide(v, *_geom(sc), th, ctx=ctx)
    ci, cd = fe.KeyFrameRadiusMatch(sc["kps"][0], sc["desc"][0], gb, q["valid"], q["uv"], q["radius"], q["level"], sc["mp_desc"], inv_sigma2=isg,
                                    ctx=ctx, uright=ur, q_ur=q["q_ur"] if gate == "stereo" else None)
    assert ci.tobytes() == bi.tobytes() and cd.tobytes() == bd.tobytes()
    # the reference side: not a comparison of empty sets
    acc = int((wbd <= TH_LOW).sum())
    print("fuse_pose", th, gate, "accepted", acc, "valid", int(p["valid"].sum()))
    assert acc >= 30
    if gate != "none":
        nbi, nbd = _ref_search(oracle, sc, 0, p, sc["mp_desc"], "none")
        assert int((nbi != wbi).sum()) >= 5                                 # the reprojection gate changes results
    if gate == "stereo":
        dec = _stereo_gate_decides(sc, 0, p)
        print("stereo gate decides", dec)
        assert dec >= 5


# ---- eorb_search_by_projection_kf_scw -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [1.0, 1.5])
def test_search_by_projection_kf_scw(fe, ctx, ref, oracle, ratio):
    sc = _nbh(45, 1, 1000, (1000,))
    kw = sc["views"][0]
    th = 4.0
    taken = (np.random.default_rng(3).random(1000) < 0.2).astype(np.uint8)
    skip = (np.arange(1000) % 13 == 12).astype(np.uint8)
    p = ref.keyframe_side(ref.view(**kw), *_geom(sc), th, skip=skip)
    thr = float(F32(TH_LOW) * F32(ratio))
    wbi, wbd, wtk = _ref_search(oracle, sc, 0, p, sc["mp_desc"], "none", taken=taken, accept_thr=thr)
    bi, bd, tk, g = fe.SearchByProjectionKFScw(sc["kps"][0], sc["desc"][0], fe.grid_bounds(W, H), fe.view(**kw), *_geom(sc), sc["mp_desc"], taken, th,
                                               ratioHamming=ratio, skip=skip, want_projection=True, ctx=ctx)
    _eq(g, p, PROJ)
    assert bi.tobytes() == wbi.tobytes() and bd.tobytes() == wbd.tobytes() and tk.tobytes() == wtk.tobytes()
    acc = int((wbd <= thr).sum())
    print("kf_scw", ratio, "accepted", acc, "newly taken", int(wtk.sum()) - int(taken.sum()))
    assert acc >= 30 and int(wtk.sum()) - int(taken.sum()) >= 30 and np.all(wtk[taken == 1] == 1)
    # the flags matter: without them other keypoints win
    fbi, _, _ = _ref_search(oracle, sc, 0, p, sc["mp_desc"], "none", taken=np.zeros(1000, np.uint8), accept_thr=thr)
    assert int((fbi != wbi).sum()) >= 5


# ---- eorb_search_by_sim3 ------------------------------------------------------------------------------------------------------------
def _sim3_ref(ref, oracle, sp, th):
    k1, k2 = sp["kf1"], sp["kf2"]
    v1, v2 = ref.view(**k1["view"]), ref.view(**k2["view"])
    cam = k1["view"]["cam"]
    p12 = ref.sim3_half(v1, sp["sR21"], sp["t21"], cam, v2, k1["pos"], k1["min_dist"], k1["max_dist"], th, skip=k1["skip"])
    p21 = ref.sim3_half(v2, sp["sR12"], sp["t12"], cam, v1, k2["pos"], k2["min_dist"], k2["max_dist"], th, skip=k2["skip"])
    F1 = oracle.Frame(k1["kps"], k1["desc"], W, H); F2 = oracle.Frame(k2["kps"], k2["desc"], W, H)
    bi1, bd1 = oracle.kf_radius_match(F2, p12["valid"], p12["uv"], p12["radius"], p12["level"], k1["mp_desc"])
    bi2, bd2 = oracle.kf_radius_match(F1, p21["valid"], p21["uv"], p21["radius"], p21["level"], k2["mp_desc"])
    vn1 = np.where(bd1 <= TH_HIGH, bi1, -1).astype(np.int32); vn2 = np.where(bd2 <= TH_HIGH, bi2, -1).astype(np.int32)
    m12 = np.full(len(vn1), -1, np.int32)
    for i1, i2 in enumerate(vn1):                                            # :1948-1964
        if i2 >= 0 and vn2[i2] == i1:
            m12[i1] = i2
    return p12, p21, vn1, vn2, m12


@pytest.mark.parametrize("s12", [1.0, 0.8])
def test_search_by_sim3(fe, ctx, ref, oracle, s12):
    sp = synth.sim3_pair(47, n=1000, s12=s12)
    th = 7.5
    p12, p21, vn1, vn2, m12 = _sim3_ref(ref, oracle, sp, th)
    gb = fe.grid_bounds(W, H)
    kf = [dict(k, gb=gb, view=fe.view(**k["view"])) for k in (sp["kf1"], sp["kf2"])]
    for _ in range(2):
        nf, g12, g1, g2 = fe.SearchBySim3Pose(kf[0], kf[1], sp["sR12"], sp["t12"], sp["sR21"], sp["t21"], th=th, ctx=ctx)
        assert g1.tobytes() == vn1.tobytes() and g2.tobytes() == vn2.tobytes()
        assert g12.tobytes() == m12.tobytes() and nf == int((m12 >= 0).sum())
    agreed = int((m12 >= 0).sum()); removed = int(((vn1 >= 0) & (m12 < 0)).sum())
    c12 = np.bincount(p12["reason"], minlength=8); c21 = np.bincount(p21["reason"], minlength=8)
    print("sim3", s12, "agreed", agreed, "removed", removed, c12.tolist(), c21.tolist())
    assert agreed >= 30 and removed >= 10
    assert all(c[r] >= 20 for c in (c12, c21) for r in (0, 1, 2, 3, 5)) and c12[6] == c21[6] == 0      # (mode E has no reason 6)


# ---- eorb_fuse_keyframes ------------------------------------------------------------------------------------------------------------
NKPS = {1: (1000,), 2: (0, 777), 7: (1000, 0, 700, 999, 65, 1, 513)}


@pytest.mark.parametrize("M", [1, 65, 1000])
@pytest.mark.parametrize("K", [1, 2, 7])
def test_fuse_keyframes_equals_k_calls_of_fuse_pose(fe, ctx, ref, oracle, K, M):
    sc = _nbh(49, K, M, NKPS[K])
    gate = {1: "mono", 2: "none", 7: "stereo"}[K]
    th = 3.0
    skip = (np.random.default_rng(5).random((K, M)) < 0.1).astype(np.uint8) if K == 7 else None
    kps, desc, ur, off = _cat(sc)
    gb = fe.grid_bounds(W, H)
    views = [fe.view(**kw) for kw in sc["views"]]
    isg = None if gate == "none" else sc["inv_sigma2"]
    bi, bd, rs = fe.FuseKeyFrames(views, [gb] * K, kps, desc, off, *_geom(sc), sc["mp_desc"], inv_sigma2=isg, th=th, skip=skip,
                                  uright=ur if gate == "stereo" else None, want_reason=True, ctx=ctx)
    bi2, bd2 = fe.FuseKeyFrames(views, [gb] * K, kps, desc, off, *_geom(sc), sc["mp_desc"], inv_sigma2=isg, th=th, skip=skip,
                                uright=ur if gate == "stereo" else None, ctx=ctx)
    assert bi2.tobytes() == bi.tobytes() and bd2.tobytes() == bd.tobytes()
    for k in range(K):
        pi, pd, g = fe.FusePose(sc["kps"][k], sc["desc"][k], gb, views[k], *_geom(sc), sc["mp_desc"], inv_sigma2=isg, th=th,
                                skip=None if skip is None else skip[k], uright=sc["uright"][k] if gate == "stereo" else None,
                                want_projection=True, ctx=ctx)
        assert bi[k].tobytes() == pi.tobytes() and bd[k].tobytes() == pd.tobytes() and rs[k].tobytes() == g["reason"].tobytes(), k
    if M == 1000:
        # against the restatement and the oracle, keyframe by keyframe
        p = ref.keyframe_side([ref.view(**kw) for kw in sc["views"]], *_geom(sc), th, skip=None if skip is None else skip.reshape(-1))
        assert rs.tobytes() == p["reason"].tobytes()
        acc = []
        for k in range(K):
            pk = {n: p[n][k * M:(k + 1) * M] for n in p}
            wbi, wbd = _ref_search(oracle, sc, k, pk, sc["mp_desc"], gate)
            assert bi[k].tobytes() == wbi.tobytes() and bd[k].tobytes() == wbd.tobytes(), k
            acc.append(int((wbd <= TH_LOW).sum()))
        print("fuse_keyframes", K, "accepted per keyframe", acc)
        assert sum(acc) >= 30 and all(a == 0 for a, n in zip(acc, NKPS[K]) if n == 0)
        assert all(a >= 30 for a, n in zip(acc, NKPS[K]) if n >= 500)


# ---- arguments, empty sides, limits -------------------------------------------------------------------------------------------------
def test_argument_errors_empty_sides_and_limits(fe, ctx):
    sc = _nbh(43, 1, 1000, (1000,))
    L, h = ctx.L, ctx.h
    v = fe.view(**sc["views"][0])
    gb = fe.grid_bounds(W, H)
    kps, desc = np.ascontiguousarray(sc["kps"][0]), np.ascontiguousarray(sc["desc"][0])
    pos, nrm, mn, mx = [np.ascontiguousarray(a) for a in _geom(sc)]
    qd = np.ascontiguousarray(sc["mp_desc"])
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    M, n = 1000, 1000
    bi = np.full(M, 7, np.int32); bd = np.full(M, 7, np.int32)
    off = np.array([0, n], np.int32)
    # every optional output NULL
    assert L.eorb_project_keyframe_side(h, C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), None, 3.0, None) == 0
    assert L.eorb_fuse_pose(h, p(kps), n, p(desc), 32, C.byref(gb), C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), None, p(qd), None, None, 3.0,
                            p(bi), p(bd), None) == 0
    assert (bd <= TH_LOW).sum() >= 30
    m12 = np.full(n, 7, np.int32)
    assert L.eorb_search_by_sim3(h, p(kps), n, p(desc), 32, C.byref(gb), C.byref(v), p(pos), p(mn), p(mx), p(qd), None,
                                 p(kps), n, p(desc), 32, C.byref(gb), C.byref(v), p(pos), p(mn), p(mx), p(qd), None,
                                 p(pos), p(pos), p(pos), p(pos), 7.5, TH_HIGH, p(m12), None, None, None) == 0
    # argument errors
    assert L.eorb_project_keyframe_side(h, None, M, p(pos), p(nrm), p(mn), p(mx), None, 3.0, None) == E_ARG
    assert L.eorb_project_keyframe_side(h, C.byref(v), -1, p(pos), p(nrm), p(mn), p(mx), None, 3.0, None) == E_ARG
    assert L.eorb_project_keyframe_side(h, C.byref(v), M, p(pos), None, p(mn), p(mx), None, 3.0, None) == E_ARG
    assert L.eorb_fuse_pose(h, p(kps), n, p(desc), 16, C.byref(gb), C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), None, p(qd), None, None, 3.0,
                            p(bi), p(bd), None) == E_ARG
    ur = np.ascontiguousarray(sc["uright"][0])
    assert L.eorb_fuse_pose(h, p(kps), n, p(desc), 32, C.byref(gb), C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), None, p(qd), None, p(ur), 3.0,
                            p(bi), p(bd), None) == E_ARG                     # the stereo gate needs inv_sigma2
    assert L.eorb_fuse_pose(h, p(kps), n, p(desc), 32, C.byref(gb), C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), None, p(qd), None, None, 3.0,
                            None, p(bd), None) == E_ARG
    bad_off = np.array([0, 5, 3], np.int32)
    v2 = (type(v) * 2)(v, v); g2 = (type(gb) * 2)(gb, gb)
    bi2 = np.zeros(2 * M, np.int32); bd2 = np.zeros(2 * M, np.int32)
    assert L.eorb_fuse_keyframes(h, v2, g2, 2, p(kps), p(desc), 32, None, p(bad_off), M, p(pos), p(nrm), p(mn), p(mx), p(qd), None, None, 3.0,
                                 p(bi2), p(bd2), None) == E_ARG
    tk = np.zeros(n, np.uint8)
    assert L.eorb_search_by_projection_kf_scw(h, p(kps), n, p(desc), 32, C.byref(gb), C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), None, p(qd),
                                              4.0, None, 50.0, p(bi), p(bd), None) == E_ARG
    assert L.eorb_search_by_sim3(h, p(kps), n, p(desc), 32, C.byref(gb), C.byref(v), p(pos), p(mn), p(mx), p(qd), None,
                                 p(kps), n, p(desc), 32, C.byref(gb), C.byref(v), p(pos), p(mn), p(mx), p(qd), None,
                                 p(pos), p(pos), p(pos), p(pos), 7.5, 300, p(m12), None, None, None) == E_ARG
    # a KannalaBrandt8 view into SearchBySim3
    kw = dict(sc["views"][0]); kw["cam"] = KB8
    vk = fe.view(**kw)
    assert L.eorb_search_by_sim3(h, p(kps), n, p(desc), 32, C.byref(gb), C.byref(vk), p(pos), p(mn), p(mx), p(qd), None,
                                 p(kps), n, p(desc), 32, C.byref(gb), C.byref(v), p(pos), p(mn), p(mx), p(qd), None,
                                 p(pos), p(pos), p(pos), p(pos), 7.5, TH_HIGH, p(m12), None, None, None) == E_CONFIG
    # empty sides: EORB_OK, outputs untouched (no queries) or -1-filled (no keypoints)
    bi[:] = 7; bd[:] = 7
    assert L.eorb_fuse_pose(h, p(kps), n, p(desc), 32, C.byref(gb), C.byref(v), 0, None, None, None, None, None, None, None, None, 3.0,
                            p(bi), p(bd), None) == 0
    assert np.all(bi == 7) and np.all(bd == 7)
    assert L.eorb_fuse_pose(h, None, 0, None, 32, C.byref(gb), C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), None, p(qd), None, None, 3.0,
                            p(bi), p(bd), None) == 0
    assert np.all(bi == -1) and np.all(bd == 256)
    assert L.eorb_fuse_keyframes(h, None, None, 0, None, None, 32, None, None, M, p(pos), p(nrm), p(mn), p(mx), p(qd), None, None, 3.0,
                                 None, None, None) == 0
    bi[:] = 7; bd[:] = 7
    assert L.eorb_search_by_projection_kf_scw(h, None, 0, None, 32, C.byref(gb), C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), None, p(qd),
                                              4.0, None, 50.0, p(bi), p(bd), None) == 0
    assert np.all(bi == -1) and np.all(bd == 256)
    nf = C.c_int(5)
    m12[:] = 7
    assert L.eorb_search_by_sim3(h, p(kps), n, p(desc), 32, C.byref(gb), C.byref(v), p(pos), p(mn), p(mx), p(qd), None,
                                 None, 0, None, 32, C.byref(gb), C.byref(v), None, None, None, None, None,
                                 p(pos), p(pos), p(pos), p(pos), 7.5, TH_HIGH, p(m12), C.byref(nf), None, None) == 0
    assert nf.value == 0 and np.all(m12 == -1)
    # capacity, by sizes only: nothing this large is allocated or read
    assert L.eorb_fuse_keyframes(h, v2, g2, 2, p(kps), p(desc), 32, None, p(off), (1 << 21) + 1, p(pos), p(nrm), p(mn), p(mx), p(qd), None, None, 3.0,
                                 p(bi2), p(bd2), None) == E_CAPACITY
    assert L.eorb_fuse_keyframes(h, v2, g2, 1025, p(kps), p(desc), 32, None, p(off), 1, p(pos), p(nrm), p(mn), p(mx), p(qd), None, None, 3.0,
                                 p(bi2), p(bd2), None) == E_CAPACITY
    big_off = np.array([0, (1 << 22) + 1], np.int32)
    assert L.eorb_fuse_keyframes(h, v2, g2, 1, p(kps), p(desc), 32, None, p(big_off), M, p(pos), p(nrm), p(mn), p(mx), p(qd), None, None, 3.0,
                                 p(bi2), p(bd2), None) == E_CAPACITY
    assert L.eorb_project_keyframe_side(h, C.byref(v), (1 << 22) + 1, p(pos), p(nrm), p(mn), p(mx), None, 3.0, None) == E_CAPACITY
    assert b"exceed" in L.eorb_last_error(h)
    # the context still works
    assert L.eorb_fuse_pose(h, p(kps), n, p(desc), 32, C.byref(gb), C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), None, p(qd), None, None, 3.0,
                            p(bi), p(bd), None) == 0
    assert (bd <= TH_LOW).sum() >= 30


# ---- a single keyframe is K = 1 of the batch: the shapes at which the shared path can go wrong ----------------------------------------
SCALE = (1.2 ** np.arange(8)).astype(F32)
INV_SIGMA2 = (F32(1.0) / (SCALE * SCALE)).astype(F32)


@functools.lru_cache(None)
def _radius_case(n, M, seed, contend=False):
    """n random keypoints and M queries aimed at picked ones: the keypoint's position and descriptor with noise (half of the queries a few
    flipped bits, half about 43 of 256, around TH_LOW and 0.8 TH_LOW), the level at or one above its octave.  Query 0 is an exact copy of
    keypoint 0 (a hit under every gate); every fourth query asks for a level no keypoint near it has, a tenth are invalid, a few lie
    outside the grid.  contend: query 1 is query 0 again, so that in order it loses keypoint 0.  uright: none for 40 % of the keypoints."""
    rng = np.random.default_rng(seed)
    kps = synth.random_keypoints(n, W, H, nlevels=6, seed=seed + 1)
    desc = synth.random_descriptors(n, seed=seed + 2)
    pick = rng.integers(0, n, M); pick[0] = 0
    if contend and M > 1:
        pick[1] = 0
    noise = rng.normal(0, 1.5, (M, 2)); noise[0] = 0
    if contend and M > 1:
        noise[1] = 0.25
    uv = (np.stack([kps["x"][pick], kps["y"][pick]], 1) + noise).astype(F32)
    level = (kps["octave"][pick] + rng.integers(0, 2, M)).astype(np.int32); level[0] = kps["octave"][0]
    miss = np.arange(M) % 4 == (3 if contend else 1)
    level[miss] += 3
    out = rng.random(M) < 0.03; out[:2] = False
    uv[out] = rng.uniform(-40, 0, (int(out.sum()), 2)).astype(F32)
    p = np.where(rng.random(M) < 0.5, 0.02, 0.17); p[0] = 0
    qd = desc[pick] ^ np.packbits(rng.random((M, 256)) < p[:, None], axis=1)
    valid = (rng.random(M) < 0.9).astype(np.uint8); valid[:2] = 1
    uright = np.where(rng.random(n) < 0.6, kps["x"] - rng.uniform(2, 30, n), -1).astype(F32)
    q_ur = (np.where(uright[pick] >= 0, uright[pick], 0) + rng.normal(0, 1.5, M)).astype(F32); q_ur[0] = max(uright[0], 0)
    radius = (F32(3.0) * SCALE[np.minimum(level, 7)]).astype(F32)
    d = dict(kps=kps, desc=desc, valid=valid, uv=uv, radius=radius, level=level, qd=qd, uright=uright, q_ur=q_ur)
    for a in d.values():
        a.setflags(write=False)
    return d


def _gate_kw(s, gate):
    kw = {} if gate == "plain" else dict(inv_sigma2=INV_SIGMA2)
    if gate == "stereo":
        kw.update(uright=s["uright"], q_ur=s["q_ur"])
    return kw


def _q(s):
    return s["valid"], s["uv"], s["radius"], s["level"], s["qd"]


def _both(bi):
    return bool((bi >= 0).any()) and bool((bi < 0).any())


@pytest.mark.parametrize("gate", ["plain", "sigma", "stereo"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_independent_radius_search_lane_and_wave_edges(fe, ctx, oracle, n, gate):
    """eorb_kf_radius_match / _stereo: the lanes stride the keypoints by 64, four waves share a workgroup"""
    gb = fe.grid_bounds(W, H)
    hits = misses = 0
    for M in (1, 3, 4, 5, 257):
        s = _radius_case(n, M, 100 + n)
        want = oracle.kf_radius_match(oracle.Frame(s["kps"], s["desc"], W, H), *_q(s), **_gate_kw(s, gate))
        got = fe.KeyFrameRadiusMatch(s["kps"], s["desc"], gb, *_q(s), ctx=ctx, **_gate_kw(s, gate))
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), M
        assert want[0][0] == 0 and want[1][0] == 0 and (M == 1 or _both(want[0])), M      # (one query cannot both hit and miss)
        hits += int((want[0] >= 0).sum()); misses += int((want[0] < 0).sum())
    print("independent", n, gate, "hits", hits, "misses", misses)
    assert hits >= 50 and misses >= 50


def test_independent_radius_search_goes_round_the_grid_stride_loop(fe, ctx, oracle):
    """K = 1 with more queries than the 8192 workgroups of four waves take in one round"""
    n, M = 65, 4 * 8192 + 5
    s = _radius_case(n, M, 7)
    Fr = oracle.Frame(s["kps"], s["desc"], W, H)
    gb = fe.grid_bounds(W, H)
    for gate in ("plain", "sigma", "stereo"):
        want = oracle.kf_radius_match(Fr, *_q(s), **_gate_kw(s, gate))
        got = fe.KeyFrameRadiusMatch(s["kps"], s["desc"], gb, *_q(s), ctx=ctx, **_gate_kw(s, gate))
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), gate
        assert _both(want[0]) and _both(want[0][4 * 8192:]), gate                          # the second round has both as well


def _taken(n, seed):
    tk = (np.random.default_rng(seed).random(n) < 0.2).astype(np.uint8)
    tk[0] = 0                                                                              # (keypoint 0 is what queries 0 and 1 want)
    return tk


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_in_order_radius_search(fe, ctx, oracle, n):
    """eorb_kf_radius_match(taken, accept_thr): one workgroup, the flags in LDS"""
    gb = fe.grid_bounds(W, H)
    taken = _taken(n, 3)
    newly = 0
    for M in (1, 2, 65):
        s = _radius_case(n, M, 200 + n, contend=True)
        Fr = oracle.Frame(s["kps"], s["desc"], W, H)
        free = oracle.kf_radius_match(Fr, *_q(s))
        for thr in (float(TH_LOW), float(F32(0.8) * F32(TH_LOW))):
            want = oracle.kf_radius_match(Fr, *_q(s), taken=taken, accept_thr=thr)
            got = fe.KeyFrameRadiusMatch(s["kps"], s["desc"], gb, *_q(s), taken=taken, accept_thr=thr, ctx=ctx)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), (M, thr)
            assert want[0][0] == 0 and want[2][0] == 1 and np.all(want[2][taken == 1] == 1)
            if M > 1:
                assert free[0][1] == 0 and want[0][1] != 0                                 # query 1 loses keypoint 0 to query 0
                assert not np.array_equal(want[0], free[0])
            if M == 65:
                assert _both(want[0])
                newly += int(want[2].sum()) - int(taken.sum())
        if M == 65 and n > 1:                                                              # the threshold decides who keeps a keypoint
            a, b = (oracle.kf_radius_match(Fr, *_q(s), taken=taken, accept_thr=t)[2] for t in (50.0, 40.0))
            print("in order", n, "taken at TH_LOW", int(a.sum()), "at 0.8 TH_LOW", int(b.sum()))
            assert a.sum() > b.sum()
    assert newly >= 2


@functools.lru_cache(None)
def _scw_case(n, M, th=4.0):
    """n keypoints of the 1 000-keypoint scene, most of them planted on map points that project validly, and M map points chosen among
    the planted ones; the second half of the points repeats the first, so that in order the repeats lose their keypoints"""
    sc = _nbh(45, 1, 1000, (1000,))
    p = kfside_ref.keyframe_side(kfside_ref.view(**sc["views"][0]), *_geom(sc), th)
    src = sc["src"][0]
    good = np.flatnonzero((src >= 0) & (p["valid"][np.maximum(src, 0)] == 1))
    other = np.flatnonzero(src < 0)
    rows = np.concatenate([good[:max(1, (3 * n) // 4)], other])[:n]
    pts = src[rows[src[rows] >= 0]]
    pts = np.concatenate([pts, np.setdiff1d(np.arange(1000), pts)])[:(M + 1) // 2]         # (points nobody was planted on: mostly misses)
    pts = np.concatenate([pts, pts])[:M]
    g = tuple(np.ascontiguousarray(a[pts]) for a in _geom(sc))
    return dict(kps=sc["kps"][0][rows], desc=sc["desc"][0][rows], geom=g, mp_desc=np.ascontiguousarray(sc["mp_desc"][pts]), view=sc["views"][0])


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_in_order_search_by_projection_kf_scw(fe, ctx, ref, oracle, n):
    """eorb_search_by_projection_kf_scw: mode D, then the in-order kernel, as fuse_common's K = 1"""
    gb = fe.grid_bounds(W, H)
    taken = _taken(n, 5)
    for M in (1, 2, 65):
        s = _scw_case(n, M)
        p = ref.keyframe_side(ref.view(**s["view"]), *s["geom"], 4.0)
        Fr = oracle.Frame(s["kps"], s["desc"], W, H)
        q = (p["valid"], p["uv"], p["radius"], p["level"], s["mp_desc"])
        free = oracle.kf_radius_match(Fr, *q)
        for ratio in (1.0, 0.8):
            thr = float(F32(TH_LOW) * F32(ratio))
            want = oracle.kf_radius_match(Fr, *q, taken=taken, accept_thr=thr)
            bi, bd, tk, g = fe.SearchByProjectionKFScw(s["kps"], s["desc"], gb, fe.view(**s["view"]), *s["geom"], s["mp_desc"], taken, 4.0,
                                                       ratioHamming=ratio, want_projection=True, ctx=ctx)
            _eq(g, p, PROJ)
            assert bi.tobytes() == want[0].tobytes() and bd.tobytes() == want[1].tobytes() and tk.tobytes() == want[2].tobytes(), (M, ratio)
            assert want[0][0] >= 0 and np.all(want[2][taken == 1] == 1)
            if M > 1:
                r = (M + 1) // 2                                                           # the first repeat: point 0 again
                assert free[0][r] == free[0][0] and want[0][r] != want[0][0]               # in order it loses its keypoint
                assert _both(want[0])


@pytest.mark.parametrize("n1,n2", [(65, 300), (300, 65), (1, 300), (300, 1)])
def test_search_by_sim3_with_unequal_sides(fe, ctx, ref, oracle, n1, n2):
    """row 1 of the 2 x M batch: its query offset M = max(n1, n2) and its descriptors' stride differ from its keypoint count"""
    sp = synth.sim3_pair(47, n=300, n_both=80, n_one=40, n_cross=40)
    cut = lambda kf, a, n: {k: (v[a:a + n] if isinstance(v, np.ndarray) else v) for k, v in kf.items()}
    full = _sim3_ref(ref, oracle, sp, 7.5)[4]
    i1 = int(np.flatnonzero(full >= 0)[0])                                                 # a side of one keeps a slot of an agreed pair
    sp = dict(sp, kf1=cut(sp["kf1"], i1 if n1 == 1 else 0, n1), kf2=cut(sp["kf2"], int(full[i1]) if n2 == 1 else 0, n2))
    th = 7.5
    p12, p21, vn1, vn2, m12 = _sim3_ref(ref, oracle, sp, th)
    gb = fe.grid_bounds(W, H)
    kf = [dict(k, gb=gb, view=fe.view(**k["view"])) for k in (sp["kf1"], sp["kf2"])]
    nf, g12, g1, g2 = fe.SearchBySim3Pose(kf[0], kf[1], sp["sR12"], sp["t12"], sp["sR21"], sp["t21"], th=th, ctx=ctx)
    assert g1.tobytes() == vn1.tobytes() and g2.tobytes() == vn2.tobytes()
    assert g12.tobytes() == m12.tobytes() and nf == int((m12 >= 0).sum())
    print("sim3", n1, n2, "found", int((vn1 >= 0).sum()), int((vn2 >= 0).sum()), "agreed", nf)
    assert (vn1 >= 0).any() and (vn2 >= 0).any() and _both(vn1 if n1 > 1 else vn2) and nf >= (5 if min(n1, n2) > 1 else 1)


def test_radius_search_profile_scopes_keep_the_entry_points_names(fe, ctx, ref):
    """one call of each entry point, profiled: the single-keyframe calls under kf_radius_match, the fused ones under kf_radius_batch"""
    s = _radius_case(65, 65, 9)
    c = _scw_case(65, 65)
    sc = _nbh(49, 2, 65, NKPS[2])
    kps, desc, ur, off = _cat(sc)
    sp = synth.sim3_pair(47, n=300, n_both=80, n_one=40, n_cross=40)
    gb = fe.grid_bounds(W, H)
    kf = [dict(k, gb=gb, view=fe.view(**k["view"])) for k in (sp["kf1"], sp["kf2"])]
    calls = [("kf_radius_match", lambda: fe.KeyFrameRadiusMatch(s["kps"], s["desc"], gb, *_q(s), ctx=ctx)),
             ("kf_radius_match", lambda: fe.KeyFrameRadiusMatch(s["kps"], s["desc"], gb, *_q(s), ctx=ctx, **_gate_kw(s, "stereo"))),
             ("kf_radius_match", lambda: fe.KeyFrameRadiusMatch(s["kps"], s["desc"], gb, *_q(s), taken=_taken(65, 3), accept_thr=50.0, ctx=ctx)),
             ("kf_radius_match", lambda: fe.SearchByProjectionKFScw(c["kps"], c["desc"], gb, fe.view(**c["view"]), *c["geom"], c["mp_desc"],
                                                                    _taken(65, 5), 4.0, ctx=ctx)),
             ("kf_radius_batch", lambda: fe.FusePose(c["kps"], c["desc"], gb, fe.view(**c["view"]), *c["geom"], c["mp_desc"], ctx=ctx)),
             ("kf_radius_batch", lambda: fe.FuseKeyFrames([fe.view(**kw) for kw in sc["views"]], [gb] * 2, kps, desc, off, *_geom(sc), sc["mp_desc"],
                                                          ctx=ctx)),
             ("kf_radius_batch", lambda: fe.SearchBySim3Pose(kf[0], kf[1], sp["sR12"], sp["t12"], sp["sR21"], sp["t21"], ctx=ctx))]
    ctx.prof_enable(True)
    try:
        for name, call in calls:
            ctx.prof_reset()
            call()
            got = {k: v[1] for k, v in ctx.prof_results().items() if k.startswith("kf_radius")}
            assert got == {name: 1}, (name, got)
    finally:
        ctx.prof_enable(False)


def test_one_keyframe_without_keypoints(fe, ctx):
    """K = 1 with kf_off = {0, 0}: EORB_OK, -1 / 256 everywhere, no keypoint read (every keypoint pointer is NULL)"""
    c = _scw_case(65, 65)
    s = _radius_case(65, 65, 9)
    L, h = ctx.L, ctx.h
    v = fe.view(**c["view"]); gb = fe.grid_bounds(W, H)
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    pos, nrm, mn, mx = [np.ascontiguousarray(a) for a in c["geom"]]
    qd = np.ascontiguousarray(c["mp_desc"])
    M = 65
    va, uv, rad, lv, sqd = [np.ascontiguousarray(a) for a in _q(s)]
    out = lambda: (np.full(M, 7, np.int32), np.full(M, 7, np.int32))
    bi, bd = out()
    assert L.eorb_kf_radius_match(h, None, 0, None, 32, C.byref(gb), M, p(va), p(uv), p(rad), p(lv), p(sqd), None, 0, None, 0.0, p(bi), p(bd)) == 0
    assert np.all(bi == -1) and np.all(bd == 256)
    bi, bd = out()
    assert L.eorb_fuse_pose(h, None, 0, None, 32, C.byref(gb), C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), None, p(qd), None, None, 3.0,
                            p(bi), p(bd), None) == 0
    assert np.all(bi == -1) and np.all(bd == 256)
    for tk in (None, np.zeros(1, np.uint8)):                                               # no flags, or flags of no keypoint
        bi, bd = out()
        assert L.eorb_search_by_projection_kf_scw(h, None, 0, None, 32, C.byref(gb), C.byref(v), M, p(pos), p(nrm), p(mn), p(mx), None, p(qd),
                                                  4.0, p(tk), 50.0, p(bi), p(bd), None) == 0
        assert np.all(bi == -1) and np.all(bd == 256) and (tk is None or tk[0] == 0)
