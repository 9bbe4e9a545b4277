"""The two-camera oracle (oracle/orc_twocam.c) on hand-built inputs: one known answer per quirk of the reference's
two-camera branches, and the reduction to the mono oracle (oracle/) when the frame has no right camera."""
import numpy as np
import pytest

from eorb_slam_amd import synth

W = H = 512


def _desc(rng, n=1):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _flip(d, k, seed=0):
    """d with k of its 256 bits flipped: Hamming distance k"""
    bits = np.unpackbits(d.copy())
    bits[np.random.default_rng(seed).choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def _kps(xy, octave=0, angle=0.0):
    k = np.zeros(len(xy), synth.KP_DTYPE)
    k["x"] = [p[0] for p in xy]; k["y"] = [p[1] for p in xy]
    k["octave"] = octave; k["angle"] = angle; k["size"] = 31.0; k["class_id"] = -1
    return k


def _cam(M, xy=(0.0, 0.0), level=0, iv=1, vc=1.0, ls=1.0):
    return (np.full(M, iv, np.uint8), np.tile(np.float32(xy), (M, 1)), np.full(M, level, np.int32),
            np.full(M, vc, np.float32), np.full(M, ls, np.float32))


# ---- ComputeStereoFishEyeMatches ---------------------------------------------------------------------------------------------
def test_lowe_boundary(oracle):
    rng = np.random.default_rng(1)
    q = _desc(rng)
    dR = np.stack([_flip(q[0], 7, 1), _flip(q[0], 10, 2)])
    n, cand, d2 = oracle.fisheye_matches(q, 0, dR, 0)
    assert d2.tolist() == [[7, 10]] and n == 0 and cand[0] == -1          # 7 < 10 * 0.7 is false in double
    dR = np.stack([_flip(q[0], 6, 1), _flip(q[0], 10, 2)])
    n, cand, _ = oracle.fisheye_matches(q, 0, dR, 0)
    assert n == 1 and cand[0] == 0
    # a right lapping set of one row: knnMatch returns one neighbour, size() < 2
    n, cand, d2 = oracle.fisheye_matches(q, 0, np.concatenate([_desc(rng, 3), q]), 3)
    assert n == 0 and cand[0] == -1 and d2.tolist() == [[0, -1]]


def test_lapping_rows_only(oracle):
    """left rows before monoLeft get no candidate; candidates are right indices (trainIdx + monoRight)"""
    rng = np.random.default_rng(2)
    dL = _desc(rng, 6)
    dR = np.concatenate([dL[4:5], _desc(rng, 2), dL[[5, 3]]])               # right row 0 (mono) equals left 4
    n, cand, d2 = oracle.fisheye_matches(dL, 3, dR, 3)
    assert cand.tolist() == [-1, -1, -1, 4, -1, 3] and n == 2
    assert (d2[:3] == -1).all() and d2[3, 0] == 0 and d2[5, 0] == 0


# ---- SearchByProjection(F, map points) -----------------------------------------------------------------------------------------
def _map_frame(rng):
    """3 left + 3 right keypoints; l2r / r2l link left 0 and right 0"""
    base = _desc(rng, 6)
    kps = np.concatenate([_kps([(100, 100), (101, 100), (300, 300)]), _kps([(100, 100), (200, 200), (400, 400)])])
    l2r = np.array([0, -1, -1], np.int32); r2l = np.array([0, -1, -1], np.int32)
    return kps, base, l2r, r2l


def test_map_left_ratio_rejection_skips_right(oracle):
    rng = np.random.default_rng(3)
    kps, desc, l2r, r2l = _map_frame(rng)
    q = _flip(desc[3 + 1], 0)[None]                                         # exact match of right keypoint 1
    desc[0] = _flip(q[0], 40, 1); desc[1] = _flip(q[0], 41, 2)              # two left candidates, same level: ratio fails
    right = _cam(1, (200, 200))
    fm = np.full(6, -1, np.int32)
    n, out = oracle.search_by_projection_map_fisheye(kps, 3, desc, oracle.grid_bounds(W, H), l2r, r2l, _cam(1, (100.5, 100)), right, q, np.ones(1, np.uint8), fm, 1.0, 0.8)
    assert n == 0 and (out == -1).all()                                     # the `continue` at :130 leaves the map-point loop
    n, out = oracle.search_by_projection_map_fisheye(kps, 3, desc, oracle.grid_bounds(W, H), l2r, r2l, _cam(1, (100.5, 100), iv=0), right, q, np.ones(1, np.uint8), fm, 1.0, 0.8)
    assert n == 1 and out[3 + 1] == 0


def test_map_right_radius_ignores_th(oracle):
    rng = np.random.default_rng(4)
    kps, desc, l2r, r2l = _map_frame(rng)
    q = desc[3 + 2][None].copy()
    fm = np.full(6, -1, np.int32)
    args = (kps, 3, desc, oracle.grid_bounds(W, H), l2r, r2l, _cam(1, iv=0))
    # viewCos > 0.998: r = 2.5; a right keypoint 3 px away is outside whatever th is
    for th in (1.0, 3.0):
        n, out = oracle.search_by_projection_map_fisheye(*args, _cam(1, (403, 400)), q, np.ones(1, np.uint8), fm, th, 0.8)
        assert n == 0
        n, out = oracle.search_by_projection_map_fisheye(*args, _cam(1, (402, 400)), q, np.ones(1, np.uint8), fm, th, 0.8)
        assert n == 1 and out[5] == 0
    # the left block applies th: 3 px away matches with th = 3 (r = 7.5) only
    q = desc[2][None].copy()
    args = (kps, 3, desc, oracle.grid_bounds(W, H), l2r, r2l)
    assert oracle.search_by_projection_map_fisheye(*args, _cam(1, (303, 300)), _cam(1, iv=0), q, np.ones(1, np.uint8), fm, 1.0, 0.8)[0] == 0
    assert oracle.search_by_projection_map_fisheye(*args, _cam(1, (303, 300)), _cam(1, iv=0), q, np.ones(1, np.uint8), fm, 3.0, 0.8)[0] == 1


def test_map_partner_propagation(oracle):
    rng = np.random.default_rng(5)
    kps, desc, l2r, r2l = _map_frame(rng)
    kps["x"][1] = 250                                                       # left 1 out of the way
    q = np.stack([desc[0], desc[3], desc[3 + 1]])
    left = _cam(3, (100, 100)); left[0][1:] = 0
    right = _cam(3, (100, 100)); right[0][0] = 0; right[1][2] = (200, 200)
    fm = np.full(6, -1, np.int32)
    # map point 0: left match at 0 also claims right slot 0 (l2r[0] = 0), two matches; map point 1 (same place in the right camera,
    # descriptor of right 0) then finds that slot observed and nothing else; map point 2 matches right 1 (no partner)
    n, out = oracle.search_by_projection_map_fisheye(kps, 3, desc, oracle.grid_bounds(W, H), l2r, r2l, left, right, q, np.ones(3, np.uint8), fm, 1.0, 0.8)
    assert out.tolist() == [0, -1, -1, 0, 2, -1] and n == 3
    # unobserved map point 0: map point 1 may take right 0 again, and writes left 0 through r2l
    n, out = oracle.search_by_projection_map_fisheye(kps, 3, desc, oracle.grid_bounds(W, H), l2r, r2l, left, right, q, np.array([0, 1, 1], np.uint8), fm, 1.0, 0.8)
    assert out.tolist() == [1, -1, -1, 1, 2, -1] and n == 5
    # a right match writes r2l[best] first
    n, out = oracle.search_by_projection_map_fisheye(kps, 3, desc, oracle.grid_bounds(W, H), l2r, r2l, _cam(1, iv=0), _cam(1, (100, 100)), desc[3][None], np.ones(1, np.uint8), fm, 1.0, 0.8)
    assert out.tolist() == [0, -1, -1, 0, -1, -1] and n == 2


def test_map_right_level_gate_reads_left_octave(oracle):
    rng = np.random.default_rng(6)
    kps, desc, l2r, r2l = _map_frame(rng)
    q = desc[3 + 1][None].copy()
    fm = np.full(6, -1, np.int32)
    args = (kps, 3, desc, oracle.grid_bounds(W, H), np.full(3, -1, np.int32), np.full(3, -1, np.int32), _cam(1, iv=0))
    kps["octave"][3 + 1] = 0; kps["octave"][1] = 5                          # right 1 at level 0, LEFT 1 at level 5
    assert oracle.search_by_projection_map_fisheye(kps, *args[1:], _cam(1, (200, 200), level=0), q, np.ones(1, np.uint8), fm, 1.0, 0.8)[0] == 0
    kps["octave"][3 + 1] = 5; kps["octave"][1] = 0                          # and the other way round
    n, out = oracle.search_by_projection_map_fisheye(kps, *args[1:], _cam(1, (200, 200), level=0), q, np.ones(1, np.uint8), fm, 1.0, 0.8)
    assert n == 1 and out[4] == 0
    # right keypoints j >= nL: their own octave (one left keypoint, three right)
    k2 = np.concatenate([kps[:1], kps[3:]]); d2 = np.concatenate([desc[:1], desc[3:]])
    k2["octave"][:] = 0; k2["octave"][3] = 4
    q = d2[3][None].copy()
    a2 = (oracle.grid_bounds(W, H), np.full(1, -1, np.int32), np.full(3, -1, np.int32), _cam(1, iv=0))
    assert oracle.search_by_projection_map_fisheye(k2, 1, d2, *a2, _cam(1, (400, 400), level=0), q, np.ones(1, np.uint8), np.full(4, -1, np.int32), 1.0, 0.8)[0] == 0
    assert oracle.search_by_projection_map_fisheye(k2, 1, d2, *a2, _cam(1, (400, 400), level=4), q, np.ones(1, np.uint8), np.full(4, -1, np.int32), 1.0, 0.8)[0] == 1


# ---- SearchByProjection(CurF, LastF) ------------------------------------------------------------------------------------------------
def test_last_right_search_needs_a_left_window(oracle):
    rng = np.random.default_rng(7)
    kps = np.concatenate([_kps([(100, 100)]), _kps([(200, 200)])])
    desc = _desc(rng, 2)
    lk = _kps([(0, 0)]); q = desc[1][None].copy()
    gb = oracle.grid_bounds(W, H)
    uv_r = np.float32([[200, 200]])
    # left window empty: no right search
    n, out = oracle.search_by_projection_last_fisheye(kps, 1, desc, gb, lk, np.ones(1, np.uint8), np.float32([[300, 300]]), uv_r, q, np.ones(1, np.uint8), np.full(2, -1, np.int32), 3.0, np.ones(1, np.float32), 0, False)
    assert n == 0 and (out == -1).all()
    # left window holds left 0, which is taken (observed): no left match, the right search still runs
    n, out = oracle.search_by_projection_last_fisheye(kps, 1, desc, gb, lk, np.ones(1, np.uint8), np.float32([[100, 100]]), uv_r, q, np.ones(1, np.uint8), np.int32([-2, -1]), 3.0, np.ones(1, np.float32), 0, False)
    assert n == 1 and out.tolist() == [-2, 0]
    # the right search has no bounds check: a right projection outside the image still searches the border cells
    kps["x"][1] = 0.5
    n, out = oracle.search_by_projection_last_fisheye(kps, 1, desc, gb, lk, np.ones(1, np.uint8), np.float32([[100, 100]]), np.float32([[-1.0, 200]]), q, np.ones(1, np.uint8), np.int32([-2, -1]), 3.0, np.ones(1, np.float32), 0, False)
    assert n == 1 and out[1] == 0


def test_last_one_rotation_histogram(oracle):
    rng = np.random.default_rng(8)
    nL = 21
    xy = [(20 + 20 * i, 50) for i in range(nL)]
    kps = np.concatenate([_kps(xy, angle=10.0), _kps([(300, 300)], angle=160.0)])
    desc = _desc(rng, nL + 1)
    desc[20] = ~desc[21]                                                    # left 20: distance 256 to the right query
    lk = _kps([(0, 0)] * 21, angle=10.0)
    uv = np.float32(xy); uv_r = np.full((21, 2), 480, np.float32); uv_r[20] = (300, 300)
    q = np.concatenate([desc[:20], desc[21:22]])                            # queries 0..19 match left 0..19, query 20 right 0
    args = (kps, nL, desc, oracle.grid_bounds(W, H), lk, np.ones(21, np.uint8), uv, uv_r, q, np.ones(21, np.uint8), np.full(nL + 1, -1, np.int32), 3.0, np.ones(21, np.float32), 0)
    n, out = oracle.search_by_projection_last_fisheye(*args, False)
    assert n == 21 and out[nL] == 20 and out[:20].tolist() == list(range(20))
    # rotation 10 - 160 + 360 = 210 -> bin 7: one entry against twenty in bin 0 (< 0.1 x 20): cleared, nmatches - 1
    n, out = oracle.search_by_projection_last_fisheye(*args, True)
    assert n == 20 and out[nL] == -1 and out[:20].tolist() == list(range(20))


# ---- SearchByBoW(KF, F) ---------------------------------------------------------------------------------------------------------
def _bow_case(rng, dl, dl2, dr, dr2):
    """one KeyFrame feature, frame = left 0, left 1, right 2, right 3 in one node, at the given distances"""
    kd = _desc(rng)
    fd = np.stack([_flip(kd[0], dl, 1), _flip(kd[0], dl2, 2), _flip(kd[0], dr, 3), _flip(kd[0], dr2, 4)])
    fv = (np.uint32([7]), np.int32([0, 4]), np.int32([0, 1, 2, 3]))
    kfv = (np.uint32([7]), np.int32([0, 1]), np.int32([0]))
    return _kps([(0, 0)]), kd, np.ones(1, np.uint8), kfv, _kps([(0, 0)] * 4), fd, fv


def test_bow_right_only_inside_left_th_low(oracle):
    rng = np.random.default_rng(9)
    kk, kd, hm, kfv, fk, fd, fv = _bow_case(rng, 60, 90, 10, 90)            # left best 60 > TH_LOW: no right match either
    n, m = oracle.search_by_bow_fisheye(kk, kd, hm, kfv, fk, 2, fd, fv, 0.7, False)
    assert n == 0 and (m == -1).all()
    kk, kd, hm, kfv, fk, fd, fv = _bow_case(rng, 40, 42, 10, 90)            # left ratio fails, right still taken
    n, m = oracle.search_by_bow_fisheye(kk, kd, hm, kfv, fk, 2, fd, fv, 0.7, False)
    assert n == 1 and m.tolist() == [-1, -1, 0, -1]


def test_bow_right_ratio_always_passes(oracle):
    rng = np.random.default_rng(10)
    kk, kd, hm, kfv, fk, fd, fv = _bow_case(rng, 10, 90, 20, 20)            # equal right distances: the first wins
    n, m = oracle.search_by_bow_fisheye(kk, kd, hm, kfv, fk, 2, fd, fv, 0.7, False)
    assert n == 2 and m.tolist() == [0, -1, 0, -1]


# ---- with no right camera the two-camera oracle is the mono oracle ------------------------------------------------------------
def _mono_frames(oracle, seed, shift):
    img1 = synth.texture_image(240, 180, seed=seed)
    img2 = np.roll(img1, (shift, -shift), axis=(0, 1))
    e = oracle.OrbExtractor(1000, 1.2, 4, 10, 0, edgeTh=19)
    _, k1, d1, _ = e.extract(img1)
    _, k2, d2, _ = e.extract(img2)
    return k1, d1, k2, d2


def test_reduces_to_mono_map(oracle):
    k1, d1, k2, d2 = _mono_frames(oracle, 22, 1)
    rng = np.random.default_rng(3)
    M = len(k1)
    in_view = (rng.uniform(size=M) < 0.9).astype(np.uint8)
    proj = np.stack([k1["x"] - 1 + rng.normal(0, 0.7, M), k1["y"] + 1 + rng.normal(0, 0.7, M)], axis=1).astype(np.float32)
    level = k1["octave"].astype(np.int32)
    vc = rng.uniform(0.99, 1.0, M).astype(np.float32)
    mp_obs = (rng.uniform(size=M) < 0.6).astype(np.uint8)
    ls = oracle.OrbExtractor(1000, 1.2, 4).scale_factors[np.clip(level, 0, 3)]
    fm = np.full(len(k2), -1, np.int32); fm[::19] = -2
    none = (np.zeros(M, np.uint8), proj, level, vc, ls)
    for th in (1.0, 3.0):
        on, ofm = oracle.search_by_projection_map(oracle.Frame(k2, d2, 240, 180), in_view, proj, level, vc, d1, mp_obs, fm, th, 0.8, ls)
        tn, tfm = oracle.search_by_projection_map_fisheye(k2, len(k2), d2, oracle.grid_bounds(240, 180), np.full(len(k2), -1, np.int32), np.zeros(0, np.int32),
                         (in_view, proj, level, vc, ls), none, d1, mp_obs, fm, th, 0.8)
        assert on == tn and np.array_equal(ofm, tfm)
    assert on > 10


def test_reduces_to_mono_last(oracle):
    k1, d1, k2, d2 = _mono_frames(oracle, 21, 2)
    rng = np.random.default_rng(2)
    n1 = len(k1)
    valid = (rng.uniform(size=n1) < 0.8).astype(np.uint8)
    uv = np.stack([k1["x"] - 2 + rng.normal(0, 1, n1), k1["y"] + 2 + rng.normal(0, 1, n1)], axis=1).astype(np.float32)
    mp_obs = (rng.uniform(size=n1) < 0.7).astype(np.uint8)
    ls = oracle.OrbExtractor(1000, 1.2, 4).scale_factors[np.clip(k1["octave"], 0, 3)]
    cur_mp = np.full(len(k2), -1, np.int32); cur_mp[::17] = -2; cur_mp[5::23] = -3
    for mode in (0, 1, 2):
        for ori in (True, False):
            on, ocm = oracle.search_by_projection_last(oracle.Frame(k2, d2, 240, 180), oracle.Frame(k1, d1, 240, 180), valid, uv, d1, mp_obs, cur_mp, 15.0, ls, mode, ori)
            tn, tcm = oracle.search_by_projection_last_fisheye(k2, len(k2), d2, oracle.grid_bounds(240, 180), k1, valid, uv, uv, d1, mp_obs, cur_mp, 15.0, ls, mode, ori)
            assert on == tn and np.array_equal(ocm, tcm)
    assert on > 10


@pytest.mark.parametrize("ori", [True, False])
def test_reduces_to_mono_bow(oracle, ori):
    k1, d1, k2, d2 = _mono_frames(oracle, 41, 2)
    rng = np.random.default_rng(11)
    kfv = synth.feature_vector_of(rng.integers(0, 60, len(k1)), rng)
    node_kf = np.zeros(len(k1), np.int64)
    for a in range(len(kfv[0])):
        node_kf[kfv[2][kfv[1][a]:kfv[1][a + 1]]] = kfv[0][a]
    dx = k2["x"][:, None] - (k1["x"][None, :] - 2); dy = k2["y"][:, None] - (k1["y"][None, :] + 2)
    near = np.argmin(dx * dx + dy * dy, axis=1)
    ffv = synth.feature_vector_of(np.where(rng.uniform(size=len(k2)) < 0.85, node_kf[near], rng.integers(0, 60, len(k2))), rng)
    has_mp = (rng.uniform(size=len(k1)) < 0.8).astype(np.uint8)
    for ratio in (0.7, 0.95):
        on, om = oracle.search_by_bow(k1, d1, has_mp, kfv, k2, d2, ffv, ratio, ori)
        tn, tm = oracle.search_by_bow_fisheye(k1, d1, has_mp, kfv, k2, len(k2), d2, ffv, ratio, ori)
        assert on == tn and np.array_equal(om, tm)
    assert on > 20
