"""GPU parity of eorb_search_for_triangulation_kb8 and eorb_kb8_triangulate_matches against the KB8 triangulation oracle
(oracle/orc_kb8tri.c, orc_match.c): SearchForTriangulation with KannalaBrandt8::epipolarConstrain (src/ORBmatcher.cc:975-1214,
src/CameraModels/KannalaBrandt8.cpp:416-486), monocular and two-camera keyframes, bit for bit."""
import hashlib

import numpy as np
import pytest

from eorb_slam_amd import synth

pytestmark = pytest.mark.gpu

E_CONFIG, E_ARG = -2, -4


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


def _both(oracle, fe, ctx, s, coarse, ori):
    on, om = oracle.search_for_triangulation_kb8(**s, coarse=coarse, checkOri=ori)
    gn, pairs = fe.SearchForTriangulationKB8(s["kps1"], s["nleft1"], s["desc1"], s["elig1"], s["fv1"], s["kps2"], s["nleft2"], s["desc2"],
                                             s["elig2"], s["fv2"], s["cams1"], s["cams2"], s["Rt"], s["ep"], s["scale2"], s["sigma2_1"],
                                             s["sigma2_2"], coarse, ori, ctx=ctx)
    gm = np.full(len(s["kps1"]), -1, np.int32)
    gm[pairs[:, 0]] = pairs[:, 1]
    return on, om, gn, gm


@pytest.mark.parametrize("twocam", [False, True])
@pytest.mark.parametrize("stride", [32, 61])
@pytest.mark.parametrize("coarse", [False, True])
@pytest.mark.parametrize("ori", [False, True])
def test_search_for_triangulation_kb8(oracle, fe, ctx, twocam, stride, coarse, ori):
    for seed in range(3):
        s = synth.keyframe_pair(seed=seed + 10 * stride, twocam=twocam, stride=stride)
        if twocam:
            assert s["nleft1"] != len(s["kps1"]) - s["nleft1"] and s["nleft2"] != len(s["kps2"]) - s["nleft2"]
        on, om, gn, gm = _both(oracle, fe, ctx, s, coarse, ori)
        assert on > 20
        assert gn == on and np.array_equal(gm, om), (seed, gn, on, np.nonzero(gm != om)[0][:10])
        if not coarse:
            cn, _, _, _ = _both(oracle, fe, ctx, s, True, ori)
            assert cn > on                                          # the geometry rejects the distractors


def test_search_kb8_pinhole_pcamera2(oracle, fe, ctx):
    """pCamera2 may be a Pinhole camera (only pCamera1 must be KannalaBrandt8)"""
    s = synth.keyframe_pair(seed=3)
    s["cams2"] = synth.CAM_MONO[:4]
    on, om, gn, gm = _both(oracle, fe, ctx, s, False, True)
    assert gn == on and np.array_equal(gm, om)


def test_search_kb8_empty_and_errors(oracle, fe, ctx):
    from eorb_slam_amd.frontend import EorbError
    s = synth.keyframe_pair(seed=4)
    e = dict(s)
    e["fv2"] = (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    on, om, gn, gm = _both(oracle, fe, ctx, e, False, True)
    assert gn == on == 0 and (gm == -1).all() and (om == -1).all()
    e = dict(s)
    e["elig1"] = np.zeros_like(s["elig1"])                              # no eligible pKF1 feature: nmatches = 0
    on, om, gn, gm = _both(oracle, fe, ctx, e, False, True)
    assert gn == on == 0 and (gm == -1).all()
    t = synth.keyframe_pair(seed=5, twocam=True)
    bad = dict(t); bad["nleft2"] = -1                                   # one keyframe with two cameras, the other without
    with pytest.raises(EorbError) as ei:
        _both(oracle, fe, ctx, bad, False, True)
    assert ei.value.code == E_CONFIG
    bad = dict(s); bad["cams1"] = synth.CAM_MONO[:4]                        # Pinhole pCamera1: the other entry point
    with pytest.raises(EorbError) as ei:
        _both(oracle, fe, ctx, bad, False, True)
    assert ei.value.code == E_CONFIG
    bad = dict(t); bad["cams1"] = (synth.CAM_L, synth.CAM_R[:4])               # a Pinhole mpCamera2 of pKF1 on a two-camera pair
    with pytest.raises(EorbError) as ei:
        _both(oracle, fe, ctx, bad, False, True)
    assert ei.value.code == E_CONFIG


def _pairs(rng, n, cam1, cam2, Rt, near):
    """pairs around true correspondences of random points (z1 > 0 mostly), a share pushed near the reprojection threshold"""
    W, H = 512, 512
    R = Rt[:9].reshape(3, 3).astype(np.float64); t = Rt[9:].astype(np.float64)
    z = rng.uniform(0.5, 12.0, n)
    X = np.stack([rng.uniform(-1.2, 1.2, n) * z, rng.uniform(-1.2, 1.2, n) * z, z], axis=1)
    uv1 = synth.project_np(cam1, X)
    X2 = (X - t) @ R                                                    # R21 (X - ... ): camera 2 coordinates of X
    uv2 = synth.project_np(cam2, X2)
    oc1 = rng.integers(0, 8, n); oc2 = rng.integers(0, 8, n)
    _, sig = synth.level_tables()
    k1 = np.zeros(n, synth.KP_DTYPE); k2 = np.zeros(n, synth.KP_DTYPE)
    noise = rng.normal(0, 1, (n, 2)) * np.where(near, np.sqrt(5.991 * sig[oc2]) / np.sqrt(2), 0.3)[:, None]
    k1["x"], k1["y"], k1["octave"] = uv1[:, 0] + rng.normal(0, 0.2, n), uv1[:, 1] + rng.normal(0, 0.2, n), oc1
    k2["x"], k2["y"], k2["octave"] = uv2[:, 0] + noise[:, 0], uv2[:, 1] + noise[:, 1], oc2
    wild = rng.uniform(size=n) < 0.1                                    # unrelated pairs
    k2["x"][wild] = rng.uniform(0, W, wild.sum()); k2["y"][wild] = rng.uniform(0, H, wild.sum())
    return k1, k2, sig


@pytest.mark.parametrize("which", ["mono", "lr", "pinhole2"])
def test_triangulate_matches_hash(oracle, fe, ctx, which):
    """z1 bits (or -1) of TriangulateMatches on ~10^6 generated pairs, including near-threshold ones: device == oracle"""
    rng = np.random.default_rng({"mono": 1, "lr": 2, "pinhole2": 3}[which])
    n = 1 << 20 if which == "mono" else 1 << 18
    R2 = synth.rot(0.03, -0.08, 0.02); t2 = np.array([-0.35, 0.04, 0.06], np.float32)
    cam1, cam2 = {"mono": (synth.CAM_MONO, synth.CAM_MONO), "lr": (synth.CAM_L, synth.CAM_R), "pinhole2": (synth.CAM_L, synth.CAM_R[:4])}[which]
    Rt = synth.rel_pose(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), R2, t2)
    near = rng.uniform(size=n) < 0.5
    k1, k2, sig = _pairs(rng, n, cam1, cam2, Rt, near)
    oz = oracle.triangulate_batch(cam1, cam2, Rt, k1, k2, sig, sig)
    gz = fe.KB8TriangulateMatches(cam1, cam2, Rt, k1, k2, sig, sig, ctx=ctx)
    npass = int((oz > np.float32(0.0001)).sum())
    assert 0.1 * n < npass < 0.9 * n                                    # both outcomes well represented
    ho, hg = hashlib.sha256(oz.view(np.uint32).tobytes()).hexdigest(), hashlib.sha256(gz.view(np.uint32).tobytes()).hexdigest()
    bad = np.nonzero(oz.view(np.uint32) != gz.view(np.uint32))[0]
    assert ho == hg, (len(bad), bad[:5], oz[bad[:5]], gz[bad[:5]])


def test_fuse_right_block(oracle, fe, ctx):
    """Fuse(pKF, vpMapPoints, th, bRight=true) (:1407-1578) on a two-camera KeyFrame: the radius core over the right block
    (right keypoints and grid, desc + Nleft rows, + Nleft on the result; every right keypoint gated as monocular, :1541 / :1563)
    against the oracle's walk of :1512-1578 on the same block"""
    s = synth.keyframe_pair(seed=30, twocam=True)
    kps, desc, nL = s["kps1"], s["desc1"][:, :32].copy(), s["nleft1"]
    kR, dR = kps[nL:], desc[nL:]
    rng = np.random.default_rng(31)
    M = 700
    pick = rng.integers(0, len(kR), M)
    valid = (rng.uniform(size=M) < 0.9).astype(np.uint8)
    uv = np.stack([kR["x"][pick] + rng.normal(0, 1.5, M), kR["y"][pick] + rng.normal(0, 1.5, M)], axis=1).astype(np.float32)
    level = np.clip(kR["octave"][pick] + rng.integers(0, 2, M), 0, synth.NLEV - 1).astype(np.int32)
    qd = np.stack([synth.flip_bits(dR[p], rng.integers(0, 40), rng) for p in pick])
    scale, sig = synth.level_tables()
    inv_sigma2 = (np.float32(1) / sig).astype(np.float32)
    radius = (np.float32(3.0) * scale[level]).astype(np.float32)
    gb = fe.grid_bounds(512, 512)
    obi, obd = oracle.kf_radius_match(oracle.Frame(kR, dR, 512, 512), valid, uv, radius, level, qd, inv_sigma2=inv_sigma2)
    gbi, gbd = fe.FuseRightMatch(kps, nL, desc, gb, valid, uv, radius, level, qd, inv_sigma2, ctx=ctx)
    assert np.array_equal(np.where(obi >= 0, obi + nL, -1), gbi) and np.array_equal(obd, gbd)
    assert (gbi >= nL).sum() > 200 and (gbi[valid == 0] == -1).all()
