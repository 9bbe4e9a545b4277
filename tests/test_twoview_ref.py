"""The CPU restatement of the two-view reconstruction stages (tests/twoview_ref): properties of the restated Jacobi SVD against numpy,
hand-derived known answers of CheckHomography / CheckFundamental, the arg-max rules, CheckRT on a scene with known motion, and the new
exports of the library.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twoview_ref as tv                            # noqa: E402
from twoview_ref import scenes                      # noqa: E402

F32 = np.float32
SEEDS = range(1000, 1040)
# Jacobi in float with double inner products has no tighter a-priori bound to cite: these are the largest deviations over SEEDS on
# standard-normal matrices (relative to the largest singular value where a length is compared), and the tests allow FACTOR times them.
#            rows of vt orthonormal   | |A v_last| - sigma_min |   | w - sigma |
MEASURED = {(16, 9): (6.87e-07, 6.36e-08, 2.48e-07), (8, 9): (2.43e-07, 1.63e-07, 2.84e-07), (3, 3): (2.84e-07, 1.92e-08, 2.02e-07)}
ROW8_MEASURED = 9.22e-08      # 8x9: the larger of | |vt.row(8)| - 1 | and | vt.row(j) . vt.row(8) |, j < 8, over SEEDS
FACTOR = 4.0


def _chain(terms):
    """a float32 add chain from 0, as `score += term` runs"""
    s = F32(0)
    for t in terms:
        s = F32(s + F32(t))
    return s


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_two_view_entry_points():
    from eorb_slam_amd import _lib
    L = C.CDLL(_lib.build())
    for sym in ("eorb_two_view_ransac", "eorb_two_view_check_rt"):
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTS
    from eorb_slam_amd import frontend
    assert callable(frontend.TwoViewReconstruction) and callable(frontend.make_sets)
    s = frontend.make_sets(20, 7, seed=1)
    assert s.shape == (7, 8) and s.dtype == np.int32 and all(len(set(r)) == 8 and min(r) >= 0 and max(r) < 20 for r in s.tolist())


# ---- the restated SVD ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(MEASURED))
def test_svd_properties_against_numpy(shape):
    m_orth, m_null, m_w = MEASURED[shape]
    worst = [0.0, 0.0, 0.0]
    for seed in SEEDS:
        A = np.random.default_rng(seed).normal(0, 1, shape).astype(F32)
        w, u, vt = tv.svd(A)
        A64, vt64 = A.astype(np.float64), vt.astype(np.float64)
        s = np.linalg.svd(A64, compute_uv=False)
        smin = s[-1] if shape[0] >= shape[1] else 0.0           # a wide matrix has a null vector
        worst[0] = max(worst[0], np.abs(vt64 @ vt64.T - np.eye(shape[1])).max())
        worst[1] = max(worst[1], abs(np.linalg.norm(A64 @ vt64[-1]) - smin) / s[0])
        worst[2] = max(worst[2], np.abs(w.astype(np.float64) - s[:len(w)]).max() / s[0])
        assert np.all(w[:-1] >= w[1:]), (seed, w)
    print("svd %s: orthonormality %.3g, null residual %.3g, singular values %.3g" % (shape, *worst))
    assert worst[0] <= FACTOR * m_orth and worst[1] <= FACTOR * m_null and worst[2] <= FACTOR * m_w, worst


def test_svd_8x9_ninth_row_is_a_unit_null_vector():
    """row 8 of vt is the zero-initialised ninth row of At: it always goes through the completion stage (a +-1/9 vector from the RNG,
    orthogonalised against rows 0-7 twice, normalised), whatever the RNG draws"""
    worst = 0.0
    for seed in SEEDS:
        A = np.random.default_rng(seed).normal(0, 1, (8, 9)).astype(F32)
        _, _, vt = tv.svd(A)
        v = vt.astype(np.float64)
        worst = max(worst, abs(np.linalg.norm(v[8]) - 1.0), np.abs(v[:8] @ v[8]).max())
    print("8x9 row 8: worst of | |v| - 1 | and | v_j . v | = %.3g" % worst)
    assert worst <= FACTOR * ROW8_MEASURED


def test_svd_degenerate_rows_are_completed_in_row_order():
    """two identical rows of A: one singular value is 0 and row 7 of At goes through the completion stage before row 8 does; vt stays
    orthonormal and both rows are null vectors"""
    A = np.random.default_rng(5).normal(0, 1, (8, 9)).astype(F32)
    A[6] = A[2]
    w, _, vt = tv.svd(A)
    v = vt.astype(np.float64)
    assert w[7] <= 4e-7 * w[0], w
    assert np.abs(v @ v.T - np.eye(9)).max() <= 1e-5
    assert np.abs(A.astype(np.float64) @ v[7]).max() <= 1e-5 * w[0] and np.abs(A.astype(np.float64) @ v[8]).max() <= 1e-5 * w[0]


def test_inv33_closed_form():
    S = np.array([[2, 0, 1], [0, 4, 0], [0, 0, 1]], F32)
    assert np.array_equal(tv.inv33(S), np.array([[0.5, 0, -0.5], [0, 0.25, 0], [0, 0, 1]], F32))
    assert np.array_equal(tv.inv33(np.ones((3, 3), F32)), np.zeros((3, 3), F32))       # d == 0: a zero matrix


# ---- known answers for the scores ----------------------------------------------------------------------------------------------------
def _grid(N):
    xy = np.stack([10.0 + 7.0 * (np.arange(N) % 9), 20.0 + 5.0 * (np.arange(N) // 9)], axis=1)
    return xy.astype(F32), np.stack([np.arange(N), np.arange(N)], axis=1).astype(np.int32)


def test_check_homography_exact_scene_scores_two_terms_per_match():
    N, th = 40, F32(5.991)
    xy, m = _grid(N)
    H21 = np.array([[1, 0, 3], [0, 1, -2], [0, 0, 1]], F32); H12 = np.array([[1, 0, -3], [0, 1, 2], [0, 0, 1]], F32)
    xy2 = xy + np.array([3, -2], F32)                     # integers: every product and sum is exact, both distances are 0
    s, inl = tv.check_homography(H21, H12, xy, xy2, m, sigma=1.0, th=th)
    assert inl.all() and s.tobytes() == _chain([th] * (2 * N)).tobytes()
    assert abs(float(s) - 2 * N * float(th)) <= 2 * N * float(th) * 2 * N * 2.0 ** -24       # 2 N th, up to the chain's roundings
    # a match displaced by more than sqrt(th)*sigma loses exactly its two terms
    xy3 = xy2.copy(); xy3[17, 0] += 3.0                   # 3 > sqrt(5.991) = 2.4477
    s3, inl3 = tv.check_homography(H21, H12, xy, xy3, m, sigma=1.0, th=th)
    assert inl3.sum() == N - 1 and inl3[17] == 0 and s3.tobytes() == _chain([th] * (2 * N - 2)).tobytes()
    # ... and one displaced by less keeps them, reduced by its two chi-squares (2 px: 4 and 4)
    xy4 = xy2.copy(); xy4[17, 0] += 2.0
    s4, inl4 = tv.check_homography(H21, H12, xy, xy4, m, sigma=1.0, th=th)
    assert inl4.all() and s4.tobytes() == _chain([th] * 34 + [F32(th - F32(4))] * 2 + [th] * 44).tobytes()
    # sigma = 2 quarters the chi-square: the 3 px displacement is an inlier again
    s5, inl5 = tv.check_homography(H21, H12, xy, xy3, m, sigma=2.0, th=th)
    assert inl5.all() and s5.tobytes() == _chain([th] * 34 + [F32(th - F32(2.25))] * 2 + [th] * 44).tobytes()


def test_check_fundamental_pure_x_translation():
    N, th, ths = 40, F32(3.841), F32(5.991)
    xy, m = _grid(N)
    F = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], F32)           # [t]x for t = (1, 0, 0): the epipolar lines are the rows v2 = v1
    xy2 = xy + np.array([11, 0], F32)
    s, inl = tv.check_fundamental(F, xy, xy2, m, sigma=1.0, th=th, th_score=ths)
    assert inl.all() and s.tobytes() == _chain([ths] * (2 * N)).tobytes()
    xy3 = xy2.copy(); xy3[5, 1] += 2.0                    # 2 px off its line: chi-square 4 > 3.841 in both images
    s3, inl3 = tv.check_fundamental(F, xy, xy3, m, sigma=1.0, th=th, th_score=ths)
    assert inl3.sum() == N - 1 and inl3[5] == 0 and s3.tobytes() == _chain([ths] * (2 * N - 2)).tobytes()
    xy4 = xy2.copy(); xy4[5, 1] += 1.0                    # 1 px: inside, the terms are thScore - 1
    s4, inl4 = tv.check_fundamental(F, xy, xy4, m, sigma=1.0, th=th, th_score=ths)
    assert inl4.all() and s4.tobytes() == _chain([ths] * 10 + [F32(ths - F32(1))] * 2 + [ths] * 68).tobytes()


def test_nan_chi_square_is_added_and_keeps_the_inlier_flag():
    """chiSquare > th is false for a NaN: bIn stays true and the score becomes NaN"""
    xy, m = _grid(9)
    s, inl = tv.check_homography(np.zeros((3, 3), F32), np.zeros((3, 3), F32), xy, xy, m)      # 1/0 = inf, 0*inf = NaN
    assert np.isnan(s) and inl.all()


# ---- the arg-max rules ---------------------------------------------------------------------------------------------------------------
def test_equal_scores_keep_the_first_iteration():
    sc = scenes.scene("general", 60, seed=3)
    sets = scenes.make_sets(60, 6, seed=4)
    T = tv.TwoViewReconstruction(scenes.K)
    base = T.find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], sets, aids=True)
    bh, bf = base["best_it_h"], base["best_it_f"]
    assert bh >= 0 and bf >= 0
    rep = np.concatenate([sets, sets[[bh, bf]], sets[[bf, bh]]])          # the winners again, twice, later
    o = T.find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], rep, aids=True)
    assert o["best_it_h"] == bh and o["best_it_f"] == bf
    assert o["it_score_h"][6].tobytes() == o["it_score_h"][bh].tobytes() == o["SH"].tobytes()
    assert o["it_score_f"][6 + 1].tobytes() == o["it_score_f"][bf].tobytes() == o["SF"].tobytes()
    assert np.array_equal(o["H21"], o["it_H"][bh]) and np.array_equal(o["F21"], o["it_F"][bf])
    same = np.concatenate([sets[[bh]]] * 3)
    o = T.find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], same)
    assert o["best_it_h"] == 0


def test_nan_scores_never_win():
    """all keys of image 2 identical: meanDev = 0, sX = inf, NaNs throughout; best_it = -1, zero matrices, zero flags"""
    sc = scenes.scene("general", 30, seed=5)
    k2 = sc["kps2"].copy(); k2["x"] = 100.0; k2["y"] = 50.0
    T = tv.TwoViewReconstruction(scenes.K)
    o = T.find_homography_fundamental(sc["kps1"], k2, sc["matches"], scenes.make_sets(30, 5, seed=6), aids=True)
    assert np.isnan(o["it_score_h"]).all() and np.isnan(o["it_score_f"]).all()
    assert o["best_it_h"] == -1 and o["best_it_f"] == -1 and o["SH"] == 0 and o["SF"] == 0
    assert not o["H21"].any() and not o["F21"].any() and not o["inliers_h"].any() and not o["inliers_f"].any()


def test_ransac_finds_the_model_of_the_scene():
    for kind, h_wins in (("planar", True), ("general", False)):
        sc = scenes.scene(kind, 120, seed=7)
        o = tv.TwoViewReconstruction(scenes.K).find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], scenes.make_sets(120, 50, seed=8))
        RH = float(o["SH"]) / (float(o["SH"]) + float(o["SF"]))
        assert (RH > 0.45) == h_wins, (kind, RH)
        assert o["inliers_f"].sum() >= 110 and (o["inliers_h"].sum() >= 110) == h_wins


# ---- CheckRT ---------------------------------------------------------------------------------------------------------------------------
# noise-free scene: the deviation of p3d from the true points is that of the float keys and the float SVD; the largest relative deviation
# over the seeds below is P3D_MEASURED, and the test allows FACTOR times it
P3D_SEEDS = range(20, 30)
P3D_MEASURED = 1.58e-06


def test_check_rt_true_pose_counts_every_inlier_and_the_twisted_ones_fewer():
    worst = 0.0
    for seed in P3D_SEEDS:
        N = 80
        sc = scenes.scene("general", N, seed=seed, noise=0.0)
        T = tv.TwoViewReconstruction(scenes.K, min_triangulated=50)
        Rts = scenes.decompose_e_poses(sc["R"], sc["t"])
        true = [h for h, (R, t) in enumerate(Rts) if np.abs(R - sc["R"]).max() < 1e-9 and np.abs(t - sc["t"]).max() < 1e-9]
        assert len(true) == 1
        inl = np.ones(N, np.uint8); inl[::7] = 0
        o = T.check_rt(sc["kps1"], sc["kps2"], sc["matches"], inl, scenes.poses27(Rts), want_cos_all=True)
        h = true[0]
        assert o["n_good"][h] == inl.sum()
        assert all(o["n_good"][j] < inl.sum() // 4 for j in range(4) if j != h), o["n_good"]
        first = sc["matches"][:, 0]
        used = first[inl != 0]
        assert o["good"][h][used].all() and o["good"][h].sum() == inl.sum()           # every parallax is far under 0.99998
        assert not o["p3d"][h][first[inl == 0]].any()
        rel = np.abs(o["p3d"][h][used] - sc["X_by_first"][used]).max(axis=1) / np.linalg.norm(sc["X_by_first"][used], axis=1)
        worst = max(worst, float(rel.max()))
        for j in range(4):
            c = o["cos_all"][j]; counted = np.sort(c[c != -2.0])
            assert len(counted) == o["n_good"][j]
            if len(counted):
                assert o["cos_sel"][j] == counted[min(50, len(counted) - 1)]
            else:
                assert o["cos_sel"][j] == 0
    print("check_rt p3d: largest relative deviation %.3g" % worst)
    assert worst <= FACTOR * P3D_MEASURED


def test_check_rt_min_triangulated_and_no_inliers():
    N = 40
    sc = scenes.scene("general", N, seed=31, noise=0.1)
    T = tv.TwoViewReconstruction(scenes.K)
    P = scenes.poses27([(sc["R"], sc["t"])])
    o = T.check_rt(sc["kps1"], sc["kps2"], sc["matches"], np.ones(N, np.uint8), P, min_triangulated=5, want_cos_all=True)
    assert o["n_good"][0] == N and o["cos_sel"][0] == np.sort(o["cos_all"][0])[5]
    o = T.check_rt(sc["kps1"], sc["kps2"], sc["matches"], np.ones(N, np.uint8), P, min_triangulated=500, want_cos_all=True)
    assert o["cos_sel"][0] == np.sort(o["cos_all"][0])[N - 1]
    o = T.check_rt(sc["kps1"], sc["kps2"], sc["matches"], np.zeros(N, np.uint8), P, want_cos_all=True)
    assert o["n_good"][0] == 0 and o["cos_sel"][0] == 0 and not o["good"].any() and not o["p3d"].any() and (o["cos_all"] == -2.0).all()
