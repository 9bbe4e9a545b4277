"""GPU parity of the two-camera (fisheye stereo) entry points against the two-camera oracle (oracle/orc_twocam.c):
eorb_frame_fisheye, eorb_search_by_projection_map_fisheye, eorb_search_by_projection_last_fisheye, eorb_search_by_bow_fisheye.
TUM-VI sized frames: 512 x 512, 8 levels."""
import numpy as np
import pytest

from eorb_slam_amd import synth

pytestmark = pytest.mark.gpu

W = H = 512
E_CAPACITY, E_ARG, E_NOTCONF = -3, -4, -6


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


def _orb(oracle, nfeat):
    return oracle.OrbExtractor(nfeat, 1.2, 8, 20, 7, edgeTh=19)


def _oracle_frame(oracle, nfeat, imL, imR, lapL, lapR):
    e = _orb(oracle, nfeat)
    mL, kL, dL, _ = e.extract(imL, lapL)
    mR, kR, dR, _ = e.extract(imR, lapR)
    n, cand, d2 = oracle.fisheye_matches(dL, mL, dR, mR)
    return dict(kpsL=kL, descL=dL, monoLeft=mL, kpsR=kR, descR=dR, monoRight=mR, right_idx=cand, dist2=d2, ncand=n)


_frames = {}


def _frame(oracle, nfeat=1500, seed=5, shift=(2, -7)):
    """an oracle two-camera frame (full lapping areas) and its concatenated keypoints / descriptors / links"""
    key = (nfeat, seed, shift)
    if key not in _frames:
        imL, imR = synth.image_pair(W, H, seed, shift)
        f = _oracle_frame(oracle, nfeat, imL, imR, (0, W - 1), (0, W - 1))
        nL, nR = len(f["kpsL"]), len(f["kpsR"])
        l2r = np.where(f["right_idx"] >= 0, f["right_idx"], -1).astype(np.int32)
        r2l = np.full(nR, -1, np.int32)
        r2l[l2r[l2r >= 0]] = np.nonzero(l2r >= 0)[0]
        _frames[key] = (np.concatenate([f["kpsL"], f["kpsR"]]), np.concatenate([f["descL"], f["descR"]]), nL, l2r, r2l)
    return _frames[key]


# ---- the frame seam --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfeat", [1000, 1500])
@pytest.mark.parametrize("laps", [((0, 511), (0, 511)), ((0, 300), (200, 511))])
def test_frame_fisheye(oracle, fe, ctx, nfeat, laps):
    imL, imR = synth.image_pair(W, H, seed=5 + nfeat // 500)
    ge = fe.ORBextractor(nfeat, 1.2, 8, 20, 7, 19, imSize=(W, H), ctx=ctx)
    g = ge.fisheye(imL, imR, laps[0], laps[1])
    o = _oracle_frame(oracle, nfeat, imL, imR, laps[0], laps[1])
    for side in ("L", "R"):
        assert np.array_equal(o["kps" + side].view(np.uint8), g["kps" + side].view(np.uint8)), side
        assert np.array_equal(o["desc" + side], g["desc" + side]), side
    assert (o["monoLeft"], o["monoRight"]) == (g["monoLeft"], g["monoRight"])
    assert np.array_equal(o["right_idx"], g["right_idx"]) and np.array_equal(o["dist2"], g["dist2"]) and o["ncand"] == g["ncand"]
    assert g["ncand"] > 50
    if laps[0] != (0, 511):
        assert 0 < g["monoLeft"] < len(g["kpsL"]) and 0 < g["monoRight"] < len(g["kpsR"])
    # a second call on the same context (the arena is reused)
    g2 = ge.fisheye(imL, imR, laps[0], laps[1])
    assert np.array_equal(g2["right_idx"], g["right_idx"]) and np.array_equal(g2["kpsR"].view(np.uint8), g["kpsR"].view(np.uint8))


def test_frame_fisheye_errors(fe, ctx):
    c = fe.Context()
    img = np.zeros((H, W), np.uint8)
    z = np.zeros(8, np.int32)
    rc = c.L.eorb_frame_fisheye(c.h, fe._p(img), fe._p(img), W, H, W, 0, W, 0, W, None, None, None, None, None, None, None, None, 0, None, None, None)
    assert rc == E_NOTCONF
    ge = fe.ORBextractor(1000, 1.2, 8, 20, 7, 19, imSize=(W, H), ctx=c)
    assert c.L.eorb_frame_fisheye(c.h, fe._p(img), fe._p(img), W + 1, H, W + 1, 0, W, 0, W, None, None, None, None, None, None, None, None, 0, None, None, None) == E_ARG
    imL, imR = synth.image_pair(W, H, seed=9)
    with pytest.raises(fe.EorbError) as e:
        ge.cap = 10                                                          # caller capacity below the keypoint count
        ge.fisheye(imL, imR, (0, 511), (0, 511))
    assert e.value.code == E_CAPACITY
    c.close()


# ---- SearchByProjection(F, map points) ------------------------------------------------------------------------------------------
def _map_case(oracle, seed, M=None):
    kps, desc, nL, l2r, r2l = _frame(oracle)
    rng = np.random.default_rng(seed)
    left, right, mp_desc, mp_obs = synth.map_inputs(kps, nL, _orb(oracle, 1500).scale_factors, rng, M, src=(kps, desc))
    fm = np.full(len(kps), -1, np.int32); fm[::29] = -2; fm[7::31] = -3
    return kps, desc, nL, l2r, r2l, left, right, mp_desc, mp_obs, fm


@pytest.mark.parametrize("th", [1.0, 3.0])
def test_map_fisheye(oracle, fe, ctx, th):
    kps, desc, nL, l2r, r2l, left, right, mp_desc, mp_obs, fm = _map_case(oracle, 31)
    gb = oracle.grid_bounds(W, H)
    on, ofm = oracle.search_by_projection_map_fisheye(kps, nL, desc, gb, l2r, r2l, left, right, mp_desc, mp_obs, fm, th, 0.8)
    m = fe.ORBmatcher(0.8, True, ctx)
    for _ in range(2):                                                      # the second call reuses the context's arena
        gn, gfm = m.SearchByProjectionMapFisheye(kps, nL, desc, l2r, r2l, gb, left, right, mp_desc, mp_obs, fm, th)
        assert on == gn and np.array_equal(ofm, gfm)
    assert on > 200 and (ofm[nL:] >= 0).sum() > 100


def test_map_fisheye_one_camera_empty(oracle, fe, ctx):
    kps, desc, nL, l2r, r2l, left, right, mp_desc, mp_obs, fm = _map_case(oracle, 32)
    gb = oracle.grid_bounds(W, H)
    m = fe.ORBmatcher(0.8, True, ctx)
    # nR = 0: the left keypoints only (no links)
    k0, d0 = kps[:nL], desc[:nL]
    on, ofm = oracle.search_by_projection_map_fisheye(k0, nL, d0, gb, np.full(nL, -1, np.int32), np.zeros(0, np.int32), left, right, mp_desc, mp_obs, fm[:nL], 1.0, 0.8)
    gn, gfm = m.SearchByProjectionMapFisheye(k0, nL, d0, np.full(nL, -1, np.int32), np.zeros(0, np.int32), gb, left, right, mp_desc, mp_obs, fm[:nL], 1.0)
    assert on == gn and np.array_equal(ofm, gfm) and on > 100
    # nL = 0: the right keypoints only
    k1, d1 = kps[nL:], desc[nL:]
    nR = len(k1)
    on, ofm = oracle.search_by_projection_map_fisheye(k1, 0, d1, gb, np.zeros(0, np.int32), np.full(nR, -1, np.int32), left, right, mp_desc, mp_obs, fm[nL:], 1.0, 0.8)
    gn, gfm = m.SearchByProjectionMapFisheye(k1, 0, d1, np.zeros(0, np.int32), np.full(nR, -1, np.int32), gb, left, right, mp_desc, mp_obs, fm[nL:], 1.0)
    assert on == gn and np.array_equal(ofm, gfm) and on > 50


def test_map_fisheye_crowded(oracle, fe, ctx):
    """hundreds of keypoints in a few cells of both grids and every map point searching there"""
    kps, desc, nL, l2r, r2l, left, right, mp_desc, mp_obs, fm = _map_case(oracle, 33, M=600)
    rng = np.random.default_rng(34)
    kps = kps.copy()
    kps["x"] = (250 + rng.uniform(0, 12, len(kps))).astype(np.float32); kps["y"] = (250 + rng.uniform(0, 12, len(kps))).astype(np.float32)
    for cam in (left, right):
        cam[1][:] = (256, 256); cam[3][:] = 0.5                             # r = 4 x scale: every search covers the crowd
    gb = oracle.grid_bounds(W, H)
    on, ofm = oracle.search_by_projection_map_fisheye(kps, nL, desc, gb, l2r, r2l, left, right, mp_desc, mp_obs, fm, 3.0, 0.9)
    gn, gfm = fe.ORBmatcher(0.9, True, ctx).SearchByProjectionMapFisheye(kps, nL, desc, l2r, r2l, gb, left, right, mp_desc, mp_obs, fm, 3.0)
    assert on == gn and np.array_equal(ofm, gfm) and on > 20


# ---- SearchByProjection(CurF, LastF) ---------------------------------------------------------------------------------------------
def _last_case(oracle, seed):
    kps, desc, nL, l2r, r2l = _frame(oracle)
    lk, ld, nLl, _, _ = _frame(oracle, seed=5, shift=(5, -3))
    rng = np.random.default_rng(seed)
    nq = len(lk)
    valid = (rng.uniform(size=nq) < 0.85).astype(np.uint8)
    uv = np.stack([lk["x"] - 3 + rng.normal(0, 1, nq), lk["y"] - 5 + rng.normal(0, 1, nq)], axis=1).astype(np.float32)
    uv_r = np.stack([uv[:, 0] + 7 + rng.normal(0, 1, nq), uv[:, 1] + rng.normal(0, 1, nq)], axis=1).astype(np.float32)
    uv_r[::41] = (-3.0, 600.0)                                              # no bounds check on the right projection
    mp_obs = (rng.uniform(size=nq) < 0.7).astype(np.uint8)
    ls = _orb(oracle, 1500).scale_factors[np.clip(lk["octave"], 0, 7)].astype(np.float32)
    cur = np.full(len(kps), -1, np.int32); cur[::17] = -2; cur[5::23] = -3
    return kps, desc, nL, lk, valid, uv, uv_r, ld, mp_obs, cur, ls


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("ori", [True, False])
def test_last_fisheye(oracle, fe, ctx, mode, ori):
    kps, desc, nL, lk, valid, uv, uv_r, ld, mp_obs, cur, ls = _last_case(oracle, 41)
    gb = oracle.grid_bounds(W, H)
    on, ocm = oracle.search_by_projection_last_fisheye(kps, nL, desc, gb, lk, valid, uv, uv_r, ld, mp_obs, cur, 7.0, ls, mode, ori)
    gn, gcm = fe.ORBmatcher(0.9, ori, ctx).SearchByProjectionLastFisheye(kps, nL, desc, gb, lk, valid, uv, uv_r, ld, mp_obs, cur, 7.0, ls, mode)
    assert on == gn and np.array_equal(ocm, gcm)
    assert on > 100 and (ocm[nL:] >= 0).sum() > 30


def test_last_fisheye_one_camera_empty(oracle, fe, ctx):
    kps, desc, nL, lk, valid, uv, uv_r, ld, mp_obs, cur, ls = _last_case(oracle, 42)
    gb = oracle.grid_bounds(W, H)
    m = fe.ORBmatcher(0.9, True, ctx)
    for sl, n in ((slice(0, nL), nL), (slice(nL, None), 0)):
        on, ocm = oracle.search_by_projection_last_fisheye(kps[sl], n, desc[sl], gb, lk, valid, uv, uv_r, ld, mp_obs, cur[sl], 7.0, ls, 0, True)
        gn, gcm = m.SearchByProjectionLastFisheye(kps[sl], n, desc[sl], gb, lk, valid, uv, uv_r, ld, mp_obs, cur[sl], 7.0, ls, 0)
        assert on == gn and np.array_equal(ocm, gcm)


# ---- SearchByBoW(KF, F) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ori", [True, False])
def test_bow_fisheye(oracle, fe, ctx, ori):
    kps, desc, nL, _, _ = _frame(oracle)
    kk, kd, _, _, _ = _frame(oracle, seed=5, shift=(5, -3))
    rng = np.random.default_rng(51)
    nn = 120
    kfv = synth.feature_vector_of(rng.integers(0, nn, len(kk)), rng)
    node_kf = np.zeros(len(kk), np.int64)
    for a in range(len(kfv[0])):
        node_kf[kfv[2][kfv[1][a]:kfv[1][a + 1]]] = kfv[0][a]
    dx = kps["x"][:, None] - (kk["x"][None, :] - 3); dy = kps["y"][:, None] - (kk["y"][None, :] - 5)
    near = np.argmin(dx * dx + dy * dy, axis=1)
    ffv = synth.feature_vector_of(np.where(rng.uniform(size=len(kps)) < 0.85, node_kf[near], rng.integers(0, nn, len(kps))), rng)
    has_mp = (rng.uniform(size=len(kk)) < 0.8).astype(np.uint8)
    for ratio in (0.7, 0.95):
        on, om = oracle.search_by_bow_fisheye(kk, kd, has_mp, kfv, kps, nL, desc, ffv, ratio, ori)
        gn, gm = fe.SearchByBoWFisheye(kk, kd, has_mp, kfv, kps, nL, desc, ffv, ratio, ori, ctx=ctx)
        assert on == gn and np.array_equal(om, gm)
        assert (om[nL:] >= 0).sum() > 20
    for n in (0, len(kps)):                                                 # nL = 0 / nR = 0
        on, om = oracle.search_by_bow_fisheye(kk, kd, has_mp, kfv, kps, n, desc, ffv, 0.7, ori)
        gn, gm = fe.SearchByBoWFisheye(kk, kd, has_mp, kfv, kps, n, desc, ffv, 0.7, ori, ctx=ctx)
        assert on == gn and np.array_equal(om, gm)


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def test_matcher_errors(oracle, fe, ctx):
    kps, desc, nL, l2r, r2l, left, right, mp_desc, mp_obs, fm = _map_case(oracle, 61)
    gb = oracle.grid_bounds(W, H)
    m = fe.ORBmatcher(0.8, True, ctx)

    def code(f, *a):
        with pytest.raises(fe.EorbError) as e:
            f(*a)
        return e.value.code
    bad = l2r.copy(); bad[0] = len(kps) - nL                                # a link past the right keypoints
    assert code(m.SearchByProjectionMapFisheye, kps, nL, desc, bad, r2l, gb, left, right, mp_desc, mp_obs, fm, 1.0) == E_ARG
    badfm = fm.copy(); badfm[3] = len(mp_obs)                               # a slot naming a map point that does not exist
    assert code(m.SearchByProjectionMapFisheye, kps, nL, desc, l2r, r2l, gb, left, right, mp_desc, mp_obs, badfm, 1.0) == E_ARG
    # more than 8192 keypoints in the two grids: refused, not truncated
    big = np.concatenate([kps] * 3); bigd = np.concatenate([desc] * 3)
    nb = len(big)
    assert nb > 8192
    assert code(m.SearchByProjectionMapFisheye, big, nb, bigd, np.full(nb, -1, np.int32), np.zeros(0, np.int32), gb, left, right,
                mp_desc, mp_obs, np.full(nb, -1, np.int32), 1.0) == E_CAPACITY
    lk = kps[:10]
    z = np.zeros((10, 2), np.float32)
    assert code(m.SearchByProjectionLastFisheye, big, nb, bigd, gb, lk, np.ones(10, np.uint8), z, z, desc[:10], np.ones(10, np.uint8),
                np.full(nb, -1, np.int32), 1.0, np.ones(10, np.float32), 0) == E_CAPACITY
    assert code(m.SearchByProjectionLastFisheye, kps, nL, desc, gb, lk, np.ones(10, np.uint8), z, z, desc[:10], np.ones(10, np.uint8),
                np.full(len(kps), -1, np.int32), 1.0, np.ones(10, np.float32), 3) == E_ARG
    rng = np.random.default_rng(1)
    fv = synth.feature_vector_of(rng.integers(0, 5, len(kps)), rng)
    assert code(fe.SearchByBoWFisheye, kps, desc, np.ones(len(kps), np.uint8), fv, kps, len(kps) + 1, desc, fv, 0.7, True, ctx) == E_ARG


# ---- empty sides; a second device ------------------------------------------------------------------------------------------------
def _synthetic_case(n, nL, M, seed):
    """n random keypoints (nL of them left), M map points / last-frame points drawn from them; no stereo links"""
    rng = np.random.default_rng(seed)
    kps = synth.random_keypoints(n, W, H, nlevels=8, seed=seed + 1); desc = synth.random_descriptors(n, seed=seed + 2)
    sf = synth.scale_tables(8, 1.2)[0]
    left, right, mp_desc, mp_obs = synth.map_inputs(kps, nL, sf, rng, M, src=(kps, desc))
    return dict(kps=kps, desc=desc, nL=nL, l2r=np.full(nL, -1, np.int32), r2l=np.full(n - nL, -1, np.int32), left=left, right=right,
                mp_desc=mp_desc, mp_obs=mp_obs, sf=sf)


def test_empty_sides_of_the_two_camera_matchers(fe, ctx):
    """nL + nR == 0 or no queries: EORB_OK, *nmatches = 0, the slots untouched"""
    import ctypes as C
    n, nL, M = 32, 20, 16
    sc = _synthetic_case(n, nL, M, 71)
    L, h, p = ctx.L, ctx.h, fe._p
    gb = fe.grid_bounds(W, H)
    (a0, a1, a2, a3, a4), (b0, b1, b2, b3, b4) = sc["left"], sc["right"]
    lk = sc["kps"][:M].copy(); z = np.zeros((M, 2), np.float32); ones = np.ones(M, np.uint8); ls = np.ones(M, np.float32)

    def map_(l, r, m, slots, nm):
        return L.eorb_search_by_projection_map_fisheye(h, p(sc["kps"]), l, r, p(sc["desc"]), 32, p(sc["l2r"]), p(sc["r2l"]), m, p(a0), p(a1), p(a2),
                                                       p(a3), p(a4), p(b0), p(b1), p(b2), p(b3), p(b4), p(sc["mp_desc"]), p(sc["mp_obs"]),
                                                       C.byref(gb), p(slots), 1.0, 0.8, C.byref(nm))

    def last(l, r, m, slots, nm):
        return L.eorb_search_by_projection_last_fisheye(h, p(sc["kps"]), l, r, p(sc["desc"]), 32, p(lk), m, p(ones), p(z), p(z), p(sc["mp_desc"]),
                                                        p(ones), p(ls), C.byref(gb), p(slots), 7.0, 0, 1, C.byref(nm))
    for call in (map_, last):
        for l, r, m in ((0, 0, M), (nL, n - nL, 0), (0, 0, 0)):
            slots = np.where(np.arange(n) % 2, -3, -2).astype(np.int32); before = slots.copy()     # (valid states: the slots are checked first)
            nm = C.c_int(-7)
            assert call(l, r, m, slots, nm) == 0
            assert nm.value == 0 and np.array_equal(slots, before)
        slots = np.full(n, M, np.int32); nm = C.c_int(-7)                    # validation still comes before the early return
        assert call(nL, n - nL, 0, slots, nm) == E_ARG and nm.value == 0 and np.all(slots == M)


def test_matchers_on_a_second_device(fe, ctx):
    """a context on device 1 gives what device 0 gives: the two-camera walk with more than 64 KB of LDS (24 592 + 16 * 2600 bytes) and a
    window matcher both need their dynamic-LDS opt-in on that device"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("fewer than two visible devices")
    c1 = fe.Context(device=1)
    try:
        n, nL, M = 2600, 1500, 64
        sc = _synthetic_case(n, nL, M, 81)
        gb = fe.grid_bounds(W, H)
        fm = np.full(n, -1, np.int32); fm[::29] = -2
        one = _synthetic_case(64, 64, M, 91)
        F = fe.FrameView(one["kps"], one["desc"], W, H)
        iv, pxy, lv, vc, ls = one["left"]
        got = []
        for c in (ctx, c1):
            m = fe.ORBmatcher(0.8, True, c)
            got.append((m.SearchByProjectionMapFisheye(sc["kps"], nL, sc["desc"], sc["l2r"], sc["r2l"], gb, sc["left"], sc["right"], sc["mp_desc"],
                                                       sc["mp_obs"], fm, 3.0),
                        m.SearchByProjectionMap(F, iv, pxy, lv, vc, one["mp_desc"], one["mp_obs"], np.full(64, -1, np.int32), 3.0, ls)))
        for (n0, s0), (n1, s1) in zip(got[0], got[1]):
            assert n0 == n1 and np.array_equal(s0, s1)
        assert got[0][0][0] >= 10 and got[0][1][0] >= 10
    finally:
        c1.close()
