"""GPU parity of eorb_two_view_ransac / eorb_two_view_check_rt with the CPU restatement (tests/twoview_ref) through the ABI.  Every
comparison is an equality of bytes after every NaN is mapped to one canonical NaN on both sides: host and device produce different NaN
sign and payload bits, and a NaN in the same place counts as equal.  The per-iteration aids are compared before the winners, so that a
failure names the iteration and the stage (an it_H / it_F difference is the SVD or the 3x3 algebra, a score difference with equal
matrices is the scoring)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twoview_ref as tv                            # noqa: E402
from twoview_ref import scenes                      # noqa: E402

pytestmark = pytest.mark.gpu

E_CAPACITY, E_ARG = -3, -4
RANSAC_SHAPES = [(8, 1), (9, 2), (63, 63), (64, 64), (65, 65), (300, 200), (1000, 200)]
RANSAC_KEYS = ("it_H", "it_F", "it_score_h", "it_score_f", "best_it_h", "best_it_f", "SH", "SF", "H21", "F21", "inliers_h", "inliers_f")
RT_KEYS = ("n_good", "cos_all", "cos_sel", "good", "p3d")


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


def _canon(a):
    a = np.array(a)
    if a.dtype == np.float32:
        a = a.copy()
        a[np.isnan(a)] = np.float32(np.nan)
    return a


def _same(got, want, keys, what):
    for k in keys:
        g, w = _canon(got[k]), _canon(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.reshape(-1).view(np.uint8 if g.dtype.itemsize == 1 else np.uint32) !=
                                 w.reshape(-1).view(np.uint8 if w.dtype.itemsize == 1 else np.uint32)) if g.ndim else np.array([0])
            i = int(bad[0])
            raise AssertionError("%s: %s differs in %d places, first at flat index %d: device %r, restatement %r"
                                 % (what, k, len(bad), i, g.reshape(-1)[i], w.reshape(-1)[i]))


def _ransac_both(fe, ctx, sc, sets, what, sigma=1.0):
    dev = fe.TwoViewReconstruction(scenes.K, sigma=sigma, ctx=ctx).find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], sets, aids=True)
    ref = tv.TwoViewReconstruction(scenes.K, sigma=sigma).find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], sets, aids=True)
    _same(dev, ref, RANSAC_KEYS, what)
    return ref


# ---- eorb_two_view_ransac ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,iters", RANSAC_SHAPES)
def test_ransac_parity_over_scenes(fe, ctx, N, iters):
    assert len(scenes.scene("general", N)["kps1"]) != len(scenes.scene("general", N)["kps2"])
    for kind in ("planar", "general", "noise", "mixed"):
        sc = scenes.scene(kind, N, seed=N + iters)
        ref = _ransac_both(fe, ctx, sc, scenes.make_sets(N, iters, seed=N), "%s N=%d iters=%d" % (kind, N, iters))
        if N >= 63 and kind in ("planar", "general"):
            RH = float(ref["SH"]) / (float(ref["SH"]) + float(ref["SF"]))
            assert (RH > 0.45) == (kind == "planar"), (kind, N, RH)
            assert ref["best_it_h"] >= 0 and ref["best_it_f"] >= 0


def test_ransac_parity_sigma(fe, ctx):
    sc = scenes.scene("mixed", 120, seed=2, noise=1.0)
    _ransac_both(fe, ctx, sc, scenes.make_sets(120, 40, seed=3), "sigma 2", sigma=2.0)


@pytest.mark.parametrize("N,iters", [(65, 65), (300, 200)])
def test_ransac_parity_ties(fe, ctx, N, iters):
    """several iterations tie exactly (a set repeated, the winner among them): the first one wins on both sides"""
    sc = scenes.scene("general", N, seed=11)
    sets = scenes.make_sets(N, iters, seed=12)
    first = tv.TwoViewReconstruction(scenes.K).find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], sets)
    bh, bf = first["best_it_h"], first["best_it_f"]
    assert bh >= 0 and bf >= 0
    sets[-1] = sets[bh]; sets[-2] = sets[bf]; sets[iters // 2] = sets[bf]
    ref = _ransac_both(fe, ctx, sc, sets, "ties N=%d" % N)
    assert ref["best_it_h"] == min(bh, iters - 1) and ref["best_it_f"] <= bf
    assert ref["it_score_f"][iters - 2].tobytes() == ref["SF"].tobytes()


@pytest.mark.parametrize("N,iters", [(64, 64), (300, 200)])
def test_ransac_parity_degenerate_sets(fe, ctx, N, iters):
    """sets whose 8 points are collinear, or hold two keys at identical coordinates: a degenerate A, zero singular values, the completion
    stage on rows < n"""
    sc = scenes.scene("general", N, seed=21)
    m = sc["matches"]
    for j in range(8):                                     # matches 0 .. 7: collinear in both images
        sc["kps1"]["x"][m[j, 0]] = 50.0 + 10.0 * j; sc["kps1"]["y"][m[j, 0]] = 100.0 + 5.0 * j
        sc["kps2"]["x"][m[j, 1]] = 60.0 + 10.0 * j; sc["kps2"]["y"][m[j, 1]] = 90.0 + 5.0 * j
    for a, b in ((9, 8), (11, 10), (12, 10)):              # matches 8 = 9 and 10 = 11 = 12: identical coordinates
        for kp, col in ((sc["kps1"], 0), (sc["kps2"], 1)):
            kp["x"][m[a, col]] = kp["x"][m[b, col]]; kp["y"][m[a, col]] = kp["y"][m[b, col]]
    sets = scenes.make_sets(N, iters, seed=22)
    sets[0] = np.arange(8)
    sets[1] = [8, 9, 20, 21, 22, 23, 24, 25]
    sets[2 % iters] = [8, 9, 10, 11, 12, 30, 31, 32]
    sets[3 % iters] = [0, 1, 2, 3, 4, 5, 6, 40]
    ref = _ransac_both(fe, ctx, sc, sets, "degenerate sets N=%d" % N)
    # the rank of the 8x9 system really drops there (five distinct rows): the restated SVD reports an exactly zero eighth singular value,
    # which sends row 7 (a row < n) through the completion stage, and two more at the rounding level
    p = tv._pts(sc["kps1"])[m[sets[2 % iters], 0]]; q = tv._pts(sc["kps2"])[m[sets[2 % iters], 1]]
    A = np.stack([np.array([b[0] * a[0], b[0] * a[1], b[0], b[1] * a[0], b[1] * a[1], b[1], a[0], a[1], 1.0], np.float32) for a, b in zip(p, q)])
    w, _, _ = tv.svd(A)
    assert w[7] == 0.0 and w[5] <= 1e-9 * w[0], w
    assert ref["best_it_f"] >= 0


@pytest.mark.parametrize("which", [1, 2])
def test_ransac_parity_all_keys_of_one_image_identical(fe, ctx, which):
    """meanDev = 0: infinities and NaNs throughout, best_it = -1"""
    N, iters = 65, 9
    sc = scenes.scene("general", N, seed=31)
    kp = sc["kps%d" % which]
    kp["x"] = 100.0; kp["y"] = 50.0
    ref = _ransac_both(fe, ctx, sc, scenes.make_sets(N, iters, seed=32), "identical keys in image %d" % which)
    assert ref["best_it_h"] == -1 and ref["best_it_f"] == -1 and np.isnan(ref["it_score_h"]).all() and np.isnan(ref["it_score_f"]).all()
    assert not ref["H21"].any() and not ref["inliers_f"].any()


def test_ransac_without_aids_gives_the_same_winners(fe, ctx):
    sc = scenes.scene("mixed", 90, seed=41)
    sets = scenes.make_sets(90, 30, seed=42)
    T = fe.TwoViewReconstruction(scenes.K, ctx=ctx)
    a = T.find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], sets, aids=True)
    b = T.find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], sets)
    assert "it_H" not in b
    _same(b, a, RANSAC_KEYS[4:], "no aids")


def _rc(fe, call):
    with pytest.raises(fe.EorbError) as e:
        call()
    return e.value.code


def test_ransac_error_paths(fe, ctx):
    from eorb_slam_amd import _lib
    T = fe.TwoViewReconstruction(scenes.K, ctx=ctx)
    sc = scenes.scene("general", 20, seed=51)
    k1, k2, m = sc["kps1"], sc["kps2"], sc["matches"]
    assert _rc(fe, lambda: T.find_homography_fundamental(k1, k2, m[:7], np.zeros((3, 8), np.int32))) == E_ARG            # N = 7
    s = scenes.make_sets(20, 3); s[2, 5] = 20
    assert _rc(fe, lambda: T.find_homography_fundamental(k1, k2, m, s)) == E_ARG                                          # a set index equal to N
    s[2, 5] = -1
    assert _rc(fe, lambda: T.find_homography_fundamental(k1, k2, m, s)) == E_ARG
    bad = m.copy(); bad[3, 1] = len(k2)
    assert _rc(fe, lambda: T.find_homography_fundamental(k1, k2, bad, scenes.make_sets(20, 3))) == E_ARG                  # a match outside the keys
    bad = m.copy(); bad[3, 0] = -1
    assert _rc(fe, lambda: T.find_homography_fundamental(k1, k2, bad, scenes.make_sets(20, 3))) == E_ARG
    # the limits, each exceeded by one; decided from the sizes: the set indices of the first and the match indices of the second are garbage
    assert _rc(fe, lambda: T.find_homography_fundamental(k1, k2, m, np.full((_lib.TVR_MAX_ITERS + 1, 8), 10 ** 6, np.int32))) == E_CAPACITY
    assert _rc(fe, lambda: T.find_homography_fundamental(k1, k2, np.full((_lib.TVR_MAX_MATCHES + 1, 2), 10 ** 6, np.int32),
                                                         np.zeros((1, 8), np.int32))) == E_CAPACITY
    # ... and exactly at the iteration limit the call runs
    big = scenes.make_sets(20, _lib.TVR_MAX_ITERS, seed=5)
    dev = T.find_homography_fundamental(k1, k2, m, big, aids=True)
    ref = tv.TwoViewReconstruction(scenes.K).find_homography_fundamental(k1, k2, m, big, aids=True)
    _same(dev, ref, RANSAC_KEYS, "iters at the limit")


# ---- eorb_two_view_check_rt ------------------------------------------------------------------------------------------------------------
def _poses(sc, Kp):
    four = scenes.decompose_e_poses(sc["R"], sc["t"])
    if Kp == 1:
        return [(sc["R"], sc["t"])]
    if Kp == 4:
        return four
    eye = np.eye(3)
    return four + [(eye, sc["t"]), (eye, np.zeros(3)), (scenes.rot([0, 1, 0], 0.5), -sc["t"]), (sc["R"], sc["t"] * 1e-4)]


def _true_index(sc, Kp):
    """where the true pose stands among _poses(sc, Kp)"""
    if Kp == 1:
        return 0
    hit = [h for h, (R, t) in enumerate(scenes.decompose_e_poses(sc["R"], sc["t"])) if np.abs(R - sc["R"]).max() < 1e-9 and np.abs(t - sc["t"]).max() < 1e-9]
    assert len(hit) == 1
    return hit[0]


def _rt_both(fe, ctx, sc, inl, poses, what, **kw):
    dev = fe.TwoViewReconstruction(scenes.K, ctx=ctx).check_rt(sc["kps1"], sc["kps2"], sc["matches"], inl, poses, want_cos_all=True, **kw)
    ref = tv.TwoViewReconstruction(scenes.K).check_rt(sc["kps1"], sc["kps2"], sc["matches"], inl, poses, want_cos_all=True, **kw)
    _same(dev, ref, RT_KEYS, what)
    return ref


@pytest.mark.parametrize("Kp", [1, 4, 8])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 300])
def test_check_rt_parity(fe, ctx, Kp, N):
    # a third of the points without parallax: with the noise they land in front of and behind the cameras, with cosParallax on both sides
    # of the threshold; the twisted poses put the near points behind one camera with parallax
    sc = scenes.scene("mixed", N, seed=100 + N, noise=0.5, far=0.35)
    poses = scenes.poses27(_poses(sc, Kp))
    rng = np.random.default_rng(N)
    inl = (rng.random(N) < 0.8).astype(np.uint8)
    if N > 1:
        inl[0] = 1
        sc["kps2"]["x"][sc["matches"][0, 1]] = np.inf          # a non-finite p3d: the :1286 skip
    ref = _rt_both(fe, ctx, sc, inl, poses, "check_rt Kp=%d N=%d" % (Kp, N))
    if N >= 63:
        h = _true_index(sc, Kp)
        ng = int(ref["n_good"][h])
        assert 0 < ng < inl.sum(), (ng, inl.sum())
        assert 0 < ref["good"][h].sum() < ng, (ref["good"][h].sum(), ng)      # counted matches above the parallax threshold exist
        assert not ref["p3d"][h][sc["matches"][0, 0]].any() and ref["cos_all"][h, 0] == -2.0
        # min_triangulated below and above n_good
        lo = _rt_both(fe, ctx, sc, inl, poses, "min_triangulated below", min_triangulated=ng // 2)
        hi = _rt_both(fe, ctx, sc, inl, poses, "min_triangulated above", min_triangulated=ng + 7)
        c = np.sort(ref["cos_all"][h][ref["cos_all"][h] != -2.0])
        assert lo["cos_sel"][h] == c[ng // 2] and hi["cos_sel"][h] == c[-1]
    # no inlier at all
    none = _rt_both(fe, ctx, sc, np.zeros(N, np.uint8), poses, "no inliers")
    assert not none["n_good"].any() and not none["cos_sel"].any() and not none["good"].any() and not none["p3d"].any()


def test_check_rt_without_cos_all(fe, ctx):
    sc = scenes.scene("general", 70, seed=7)
    poses = scenes.poses27(_poses(sc, 4))
    T = fe.TwoViewReconstruction(scenes.K, ctx=ctx)
    a = T.check_rt(sc["kps1"], sc["kps2"], sc["matches"], np.ones(70, np.uint8), poses, want_cos_all=True)
    b = T.check_rt(sc["kps1"], sc["kps2"], sc["matches"], np.ones(70, np.uint8), poses)
    assert "cos_all" not in b
    _same(b, a, ("n_good", "cos_sel", "good", "p3d"), "no cos_all")


def test_check_rt_error_paths(fe, ctx):
    from eorb_slam_amd import _lib
    T = fe.TwoViewReconstruction(scenes.K, ctx=ctx)
    sc = scenes.scene("general", 20, seed=61)
    k1, k2, m = sc["kps1"], sc["kps2"], sc["matches"]
    one = scenes.poses27([(sc["R"], sc["t"])])
    inl = np.ones(20, np.uint8)
    bad = m.copy(); bad[4, 0] = len(k1)
    assert _rc(fe, lambda: T.check_rt(k1, k2, bad, inl, one)) == E_ARG
    bad = m.copy(); bad[4, 0] = bad[3, 0]
    assert _rc(fe, lambda: T.check_rt(k1, k2, bad, inl, one)) == E_ARG                     # two matches with one first index
    assert _rc(fe, lambda: T.check_rt(k1, k2, m, inl, one, min_triangulated=-1)) == E_ARG
    assert _rc(fe, lambda: T.check_rt(k1, k2, m, inl, np.repeat(one, _lib.TVR_MAX_POSES + 1, axis=0))) == E_CAPACITY
    big = np.full((_lib.TVR_MAX_MATCHES + 1, 2), 10 ** 6, np.int32)
    assert _rc(fe, lambda: T.check_rt(k1, k2, big, np.ones(len(big), np.uint8), one)) == E_CAPACITY


def test_python_mirror_gives_the_abi_bytes(fe, ctx):
    """frontend.TwoViewReconstruction against a direct ctypes call of the two entry points"""
    import ctypes as C
    from eorb_slam_amd import _lib
    N, it = 65, 10
    sc = scenes.scene("mixed", N, seed=71)
    sets = fe.make_sets(N, it, seed=72)
    T = fe.TwoViewReconstruction(scenes.K, ctx=ctx)
    o = T.find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], sets, aids=True)
    L, p = ctx.L, fe._p
    H = np.zeros(9, np.float32); F = np.zeros(9, np.float32); ih = np.zeros(N, np.uint8); jf = np.zeros(N, np.uint8)
    sh = np.zeros(it, np.float32); sf = np.zeros(it, np.float32); iH = np.zeros(it * 9, np.float32); iF = np.zeros(it * 9, np.float32)
    SH, SF, bh, bf = C.c_float(0), C.c_float(0), C.c_int(0), C.c_int(0)
    par = _lib.TvrParams(1.0, 5.991, 3.841)
    assert L.eorb_two_view_ransac(ctx.h, p(sc["kps1"]), len(sc["kps1"]), p(sc["kps2"]), len(sc["kps2"]), p(sc["matches"]), N, p(sets), it, C.byref(par),
                                  p(H), C.byref(SH), C.byref(bh), p(ih), p(F), C.byref(SF), C.byref(bf), p(jf), p(sh), p(sf), p(iH), p(iF)) == 0
    raw = dict(H21=H.reshape(3, 3), F21=F.reshape(3, 3), inliers_h=ih, inliers_f=jf, it_score_h=sh, it_score_f=sf, it_H=iH.reshape(it, 3, 3),
               it_F=iF.reshape(it, 3, 3), SH=np.float32(SH.value), SF=np.float32(SF.value), best_it_h=bh.value, best_it_f=bf.value)
    _same(o, raw, RANSAC_KEYS, "python mirror, ransac")
    poses = fe.tvr_poses(scenes.K, [sc["R"]], [sc["t"]])
    assert poses.shape == (1, 27) and np.allclose(poses, scenes.poses27([(sc["R"], sc["t"])]), rtol=1e-5, atol=1e-4)
    inl = (~sc["bad"]).astype(np.uint8)                    # the matches the scene generated as correct
    r = T.check_rt(sc["kps1"], sc["kps2"], sc["matches"], inl, poses, want_cos_all=True)
    n1 = len(sc["kps1"])
    ng = np.zeros(1, np.int32); g = np.zeros(n1, np.uint8); p3 = np.zeros(n1 * 3, np.float32); cs = np.zeros(1, np.float32); ca = np.zeros(N, np.float32)
    Kf = np.ascontiguousarray(scenes.K, np.float32)
    assert L.eorb_two_view_check_rt(ctx.h, p(sc["kps1"]), n1, p(sc["kps2"]), len(sc["kps2"]), p(sc["matches"]), N, p(inl), p(Kf), 4.0,
                                    float(np.float32(0.99998)), 50, p(poses), 1, p(ng), p(g), p(p3), p(cs), p(ca)) == 0
    _same(r, dict(n_good=ng, good=g.reshape(1, n1), p3d=p3.reshape(1, n1, 3), cos_sel=cs, cos_all=ca.reshape(1, N)), RT_KEYS, "python mirror, check_rt")
    assert r["n_good"][0] > 20
