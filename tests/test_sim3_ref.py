"""The CPU restatement of the Sim3 solver (tests/sim3_ref): ComputeSim3 against a float64 Horn solution in numpy, the restated 4x4 Jacobi
eigen-solver against numpy.linalg.eigh, the fdlibm atan2 against the host's, hand-derived edge cases, the truncated inlier bound and the
result rule against named wrong variants, the branch probe over the scene set, and the new export of the library.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_ref as s3                               # noqa: E402
from sim3_ref import scenes                         # noqa: E402

F32 = np.float32
SEEDS = range(2000, 2040)
FACTOR = 4.0
# Jacobi in float has no tighter a-priori bound to cite (the convention of tests/test_twoview_ref.py): these are the largest deviations of
# the restatement over SEEDS, and the tests allow FACTOR times them.
#                    | R - R64 |   | s - s64 | / s64   | t - t64 | / (1 + |t64|)   | T21*T12 - I |
SIM3_MEASURED = {False: (3.75e-06, 7.26e-08, 9.44e-06, 1.77e-07), True: (3.68e-06, 0.0, 8.46e-06, 1.32e-07)}
#                    | V V^T - I |   | w - eigh | / max|w|   (random symmetric 4x4, standard normal entries)
EIGEN_MEASURED = (6.30e-07, 1.67e-07)


# ---- the ABI and the mirrors' host arithmetic ----------------------------------------------------------------------------------------
def test_the_library_exports_the_sim3_entry_point():
    from eorb_slam_amd import _lib
    L = C.CDLL(_lib.build())
    assert hasattr(L, "eorb_sim3_ransac") and "eorb_sim3_ransac" in _lib.EXPORTS
    assert C.sizeof(_lib.Sim3Result) == C.sizeof(s3.Result) == 33 * 4
    assert C.sizeof(_lib.Sim3Problem) == 4 * 4 + 24 * 4 + 2 * C.sizeof(_lib.Camera)
    from eorb_slam_amd import frontend
    assert callable(frontend.Sim3Solver)


def test_ransac_iterations_formula_and_set_draw():
    from eorb_slam_amd import frontend
    # log(0.01) / log(1 - (6/20)^3) = 168.2 -> 169; the cap; minInliers == N -> 1; epsilon = 0 and epsilon > 1 convert to INT_MIN -> 1
    for args, want in (((20, 0.99, 6, 300), 169), ((20, 0.99, 6, 100), 100), ((6, 0.99, 6, 300), 1), ((50, 0.99, 0, 300), 1), ((4, 0.99, 6, 300), 1),
                       ((12, 0.99, 6, 300), 35), ((1000, 0.99, 6, 300), 300)):
        assert s3.ransac_iterations(*args) == want == frontend.sim3_ransac_iterations(*args), args
    for N in (3, 4, 50):
        a, b = s3.draw_sets(N, 200, seed=N), frontend.sim3_draw_sets(N, 200, seed=N)
        assert np.array_equal(a, b) and a.dtype == np.int32 and a.shape == (200, 3)
        assert all(len(set(r)) == 3 and min(r) >= 0 and max(r) < N for r in a.tolist())
    assert len({tuple(r) for r in s3.draw_sets(4, 400, seed=1).tolist()}) == 24          # every ordered triple of four turns up


# ---- ComputeSim3 against float64 ----------------------------------------------------------------------------------------------------------
def _horn64(P1, P2, fix_scale):
    """Horn 1987 in float64 on the float32 triples [3 points, 3]: numpy.linalg.eigh of the same N"""
    P1 = np.asarray(P1, F32).astype(np.float64); P2 = np.asarray(P2, F32).astype(np.float64)
    O1, O2 = P1.mean(axis=0), P2.mean(axis=0)
    Pr1, Pr2 = (P1 - O1).T, (P2 - O2).T
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, v = np.linalg.eigh(N)
    q = v[:, -1]
    ang = np.arctan2(np.linalg.norm(q[1:]), q[0])
    R = scenes.rot(q[1:], 2 * ang)
    P3 = R @ Pr2
    s = 1.0 if fix_scale else (Pr1 * P3).sum() / (P3 * P3).sum()
    return R, s, O1 - s * R @ O2


def _planted(seed, fix_scale):
    rng = np.random.default_rng(seed)
    R = scenes.rot(rng.normal(size=3), rng.uniform(0.05, 3.0))
    s = 1.0 if fix_scale else rng.uniform(0.5, 2.0)
    t = rng.uniform(-2.0, 2.0, 3)
    P2 = rng.uniform(-3.0, 3.0, (3, 3)) + [0.0, 0.0, 6.0]
    return (s * P2 @ R.T + t).astype(F32), P2.astype(F32), R, s, t


@pytest.mark.parametrize("fix_scale", [False, True])
def test_compute_sim3_recovers_a_planted_similarity(fix_scale):
    worst = [0.0, 0.0, 0.0, 0.0]
    for seed in SEEDS:
        P1, P2, R, s, t = _planted(seed, fix_scale)
        o = s3.compute_sim3(P1, P2, fix_scale)
        R64, s64, t64 = _horn64(P1, P2, fix_scale)
        assert np.abs(R64 - R).max() < 1e-5 and abs(s64 - s) < 1e-5 * s and np.abs(t64 - t).max() < 1e-4          # (the float64 solution finds the plant)
        worst[0] = max(worst[0], np.abs(o["R12"] - R64).max())
        worst[1] = max(worst[1], abs(float(o["s12"]) - s64) / s64)
        worst[2] = max(worst[2], np.abs(o["t12"] - t64).max() / (1 + np.abs(t64).max()))
        worst[3] = max(worst[3], np.abs(o["T21"].astype(np.float64) @ o["T12"].astype(np.float64) - np.eye(4)).max())
        assert np.array_equal(o["T12"][3], [0, 0, 0, 1]) and np.array_equal(o["T21"][3], [0, 0, 0, 1])
        assert np.array_equal(o["T12"][:3, 3], o["t12"])
        if fix_scale:
            assert o["s12"] == 1 and np.array_equal(o["T12"][:3, :3], o["R12"]) and np.array_equal(o["T21"][:3, :3], o["R12"].T)
    print("compute_sim3 fix_scale=%d: R %.3g, s %.3g, t %.3g, T21*T12 %.3g" % (fix_scale, *worst))
    for got, measured in zip(worst, SIM3_MEASURED[fix_scale]):
        assert got <= FACTOR * measured, (worst, SIM3_MEASURED[fix_scale])


# ---- the eigen-solver alone ----------------------------------------------------------------------------------------------------------------
def test_eigen4_properties_against_eigh():
    worst = [0.0, 0.0]
    for seed in SEEDS:
        B = np.random.default_rng(seed).normal(0, 1, (4, 4))
        A = ((B + B.T) / 2).astype(F32)
        A = np.triu(A) + np.triu(A, 1).T
        w, V, rotations, hit_max = s3.eigen4(A)
        assert rotations > 0 and not hit_max
        assert np.all(w[:-1] >= w[1:]), (seed, w)
        V64 = V.astype(np.float64)
        w64 = np.linalg.eigh(A.astype(np.float64))[0][::-1]
        worst[0] = max(worst[0], np.abs(V64 @ V64.T - np.eye(4)).max())
        worst[1] = max(worst[1], np.abs(w - w64).max() / np.abs(w64).max())
        # each row is an eigenvector of its eigenvalue, to the same order
        assert np.abs(A.astype(np.float64) @ V64.T - V64.T * w.astype(np.float64)).max() <= 1e-5 * np.abs(w64).max()
    print("eigen4: orthonormality %.3g, eigenvalues %.3g" % tuple(worst))
    assert worst[0] <= FACTOR * EIGEN_MEASURED[0] and worst[1] <= FACTOR * EIGEN_MEASURED[1], worst


def test_eigen4_diagonal_matrix_executes_no_rotation():
    w, V, rotations, hit_max = s3.eigen4(np.diag([1.0, 4.0, -2.0, 3.0]).astype(F32))
    assert rotations == 0 and not hit_max
    assert np.array_equal(w, [4, 3, 1, -2])
    assert np.array_equal(V, np.eye(4, dtype=F32)[[1, 3, 0, 2]])          # the selection sort swaps rows: 0<->1, then 1<->3, then 2<->3


def test_eigen4_repeated_top_eigenvalue():
    Q = np.linalg.qr(np.random.default_rng(7).normal(size=(4, 4)))[0]
    A64 = Q @ np.diag([5.0, 5.0, 1.0, -3.0]) @ Q.T
    A = A64.astype(F32); A = np.triu(A) + np.triu(A, 1).T
    w, V, _, hit_max = s3.eigen4(A)
    V64 = V.astype(np.float64)
    assert not hit_max and np.abs(w - [5, 5, 1, -3]).max() <= FACTOR * EIGEN_MEASURED[1] * 5
    assert np.abs(V64 @ V64.T - np.eye(4)).max() <= FACTOR * EIGEN_MEASURED[0]
    # rows 0 and 1 span the eigenspace of 5: A v = 5 v for both
    assert np.abs(A.astype(np.float64) @ V64[:2].T - 5 * V64[:2].T).max() <= 1e-5


# ---- atan2 ------------------------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / np.spacing(np.abs(b))
    d[(a == b) | (np.isnan(a) & np.isnan(b))] = 0
    return d


def test_atan2_against_host_libm():
    """fdlibm's atan2 is within 1 ulp of the true value, the host's is correctly rounded: they differ by at most 1 ulp, on a minority of
    the inputs; the signs of zero and the special values agree exactly"""
    rng = np.random.default_rng(11)
    n = 100000
    mag = np.exp(rng.uniform(-40, 40, (2, n)))
    y = np.concatenate([rng.normal(size=n), mag[0] * rng.choice([-1, 1], n), np.linspace(0, 1, 1001), np.full(1001, 1.0)])
    x = np.concatenate([rng.normal(size=n), mag[1] * rng.choice([-1, 1], n), np.full(1001, 1.0), np.linspace(-1, 1, 1001)])
    got, want = s3.atan2(y, x), s3.atan2(y, x, host=True)
    d = _ulps(got, want)
    for q, m in enumerate([(y > 0) & (x > 0), (y < 0) & (x > 0), (y > 0) & (x < 0), (y < 0) & (x < 0)]):
        assert m.sum() > 10000
        print("atan2 quadrant %d: %d of %d inputs differ from the host, largest distance %.0f ulp" % (q, int((d[m] > 0).sum()), int(m.sum()), d[m].max()))
    assert d.max() <= 1
    sp = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-310, -1e-310, 1e300, -1e300, 2.0 ** -1074]
    ys, xs = np.meshgrid(sp, sp)
    got, want = s3.atan2(ys.ravel(), xs.ravel()), s3.atan2(ys.ravel(), xs.ravel(), host=True)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.signbit(got[~np.isnan(got)]), np.signbit(want[~np.isnan(want)]))
    assert _ulps(got, want).max() <= 1
    yy, xx = ys.ravel(), xs.ravel()
    axes = ((yy == 0) | (xx == 0) | (np.isinf(yy) != np.isinf(xx))) & ~np.isnan(want)
    assert axes.sum() >= 60 and np.array_equal(got[axes], want[axes])     # a zero or one infinity among the arguments: +-0, +-pi/2, +-pi exactly


def test_host_atan2_changes_few_transform_entries():
    """how much of the parity depends on atan2: the share of it_T12 entries of the test scenes that change when the host's atan2 is used"""
    changed = total = 0
    for seed, pair in ((1, "pp"), (2, "kk"), (3, "pk")):
        pb = scenes.scene(65, seed=seed, pair=pair, iters=300)
        a = scenes.find(s3, pb)["it_T12"]
        s3.set_option(s3.OPT_HOST_ATAN2, 1)
        try:
            b = scenes.find(s3, pb)["it_T12"]
        finally:
            s3.set_option(s3.OPT_HOST_ATAN2, 0)
        changed += int((a.view(np.uint32) != b.view(np.uint32)).sum()); total += a.size
        assert np.abs(a - b).max() <= 2.0 ** -20
    print("host atan2: %d of %d it_T12 entries change" % (changed, total))
    assert changed <= total // 100


# ---- hand-derived cases -------------------------------------------------------------------------------------------------------------------
EDGE = scenes.edge_problems()


def test_identical_triples_give_a_nan_transform_that_is_still_the_best():
    o = scenes.find(s3, EDGE["identical"])
    assert np.isnan(o["it_T12"][:, :3, :]).all() and np.isnan(o["it_T21"][:, :3, :]).all() and np.isnan(o["it_scale"]).all()
    assert np.array_equal(o["it_T12"][:, 3], [[0, 0, 0, 1]] * 3)
    assert not o["it_inliers"].any() and not o["inliers"].any()
    # 0 >= 0: every iteration replaces the running best, the last one stays
    assert (o["converged"], o["best_it"], o["n_inliers"], o["iterations_used"]) == (0, 2, 0, 3)
    assert np.isnan(o["T12"][:3]).all() and np.isnan(o["R12"]).all() and np.isnan(o["t12"]).all() and np.isnan(o["s12"])


@pytest.mark.parametrize("name,R", [("half_turn_z", np.diag([-1.0, -1.0, 1.0])), ("half_turn_oblique", scenes.rot([1.0, 2.0, 2.0], np.pi))])
def test_half_turn(name, R):
    """X2 = R X1 + t with R a rotation by pi: R12 = R^T = R; the quaternion's real part is at or near 0"""
    o = scenes.find(s3, EDGE[name])
    assert np.abs(o["it_T12"][:, :3, :3] - R).max() <= 2e-6 and np.abs(o["it_scale"] - 1).max() <= 2e-6
    assert o["converged"] == 1 and o["best_it"] == 0 and o["n_inliers"] == 5 and o["inliers"].all()


def test_collinear_triple_is_finite_and_fits_its_own_points():
    o = scenes.find(s3, EDGE["collinear"])
    assert np.isfinite(o["it_T12"]).all() and np.isfinite(o["it_T21"]).all()
    assert o["it_inliers"][0] >= 3 and o["inliers"][:3].all()            # the three points of the line fit any rotation about it
    assert o["it_inliers"][1] == 5                                       # a proper triple finds the similarity


def test_repeated_index_sets_are_accepted():
    o = scenes.find(s3, EDGE["repeated_index"])
    assert np.isfinite(o["it_T12"][0]).all()                             # two distinct points: a line, as above
    assert np.isnan(o["it_T12"][1][:3]).all() and o["it_inliers"][1] == 0         # one point three times: Pr = 0, M = 0, the NaN path
    assert o["best_it"] == 2 and o["n_inliers"] == 5


@pytest.mark.parametrize("cams", ["pp", "kk"])
def test_a_point_with_z_zero_is_an_outlier_or_judged_by_its_angle(cams):
    a, b = scenes.find(s3, EDGE["z0_first_" + cams]), scenes.find(s3, EDGE["z0_second_" + cams])
    assert np.array_equal(a["inliers"], [1, 1, 1, 0, 1]) and np.array_equal(b["inliers"], [1, 1, 1, 1, 0])
    assert a["n_inliers"] == 4 and b["n_inliers"] == 4


def test_tiny_rotation_vector_takes_the_identity_branch_of_rodrigues():
    s3.probe_reset()
    o = scenes.find(s3, EDGE["tiny_angle"])
    assert s3.probe_read()["rodrigues_identity"] == 1
    assert np.array_equal(o["R12"], np.eye(3, dtype=F32))


def test_nan_input_ends_in_a_nan_transform():
    o = scenes.find(s3, EDGE["nan_point"])
    assert np.isnan(o["it_T12"][0, :3]).all() and o["it_inliers"][0] == 0
    assert np.isfinite(o["it_T12"][1]).all() and o["inliers"][1] == 0     # the set without the NaN point is sound; that point is an outlier of it


# ---- the truncated bound ----------------------------------------------------------------------------------------------------------------
def test_bound_is_truncated_to_an_integer():
    assert s3.bound(1.0) == 9 and s3.bound(0.1) == 0 and s3.bound(1.44) == 13 and s3.bound(0.0) == 0
    assert s3.bound(F32(1.2) ** 14) == int(9.210 * float(F32(1.2) ** 14))
    s3.set_option(s3.OPT_FLOAT_BOUND, 1)
    try:
        assert s3.bound(1.0) == F32(9.21)
    finally:
        s3.set_option(s3.OPT_FLOAT_BOUND, 0)


def test_threshold_quirk_rejects_the_float_bound_variant():
    pb, names = scenes.threshold_problem(s3)
    assert names == ["between_9_and_9.21", "exactly_9", "one_float_below_9", "err_4"]
    o = scenes.find(s3, pb)
    # err 9.12: an outlier (9.12 < 9 fails); exactly 9.0f: an outlier, the comparison is strict; one float below: an inlier
    assert np.array_equal(o["inliers"], [1, 1, 1, 0, 0, 1, 1]) and o["n_inliers"] == 5
    s3.set_option(s3.OPT_FLOAT_BOUND, 1)
    try:
        v = scenes.find(s3, pb)
    finally:
        s3.set_option(s3.OPT_FLOAT_BOUND, 0)
    assert np.array_equal(v["inliers"], [1, 1, 1, 1, 1, 1, 1])          # the variant "float bound 9.21*sigma2" takes both
    z, _ = scenes.threshold_problem(s3, sigma2=0.1)
    o = scenes.find(s3, z)
    assert not o["inliers"].any() and o["n_inliers"] == 0 and o["converged"] == 0          # the bound is 0: nothing is ever an inlier


# ---- the result rule ------------------------------------------------------------------------------------------------------------------------
def _rule_model(counts, N, min_inliers, replace=lambda n, best: n >= best, converge=lambda n, m: n > m):
    """the loop of :243-291 under LoopClosing.cc:698-701 in plain Python"""
    if N < min_inliers:
        return dict(converged=0, best_it=-1, n_inliers=0, iterations_used=0)
    best, best_it = 0, -1
    for it, n in enumerate(counts):
        if replace(n, best):
            best, best_it = n, it
            if converge(n, min_inliers):
                return dict(converged=1, best_it=it, n_inliers=n, iterations_used=it + 1)
    return dict(converged=0, best_it=best_it, n_inliers=best, iterations_used=len(counts))


def _earliest_of_equal(counts, N, min_inliers):
    o = _rule_model(counts, N, min_inliers)
    if not o["converged"] and o["best_it"] >= 0:
        o["best_it"] = list(counts).index(o["n_inliers"])
    return o


RULE_VARIANTS = {
    "running best replaced on > instead of >=": lambda c, N, m: _rule_model(c, N, m, replace=lambda n, best: n > best),
    "convergence on >= instead of >": lambda c, N, m: _rule_model(c, N, m, converge=lambda n, mm: n >= mm),
    "earliest of equal counts": _earliest_of_equal,
}
# the scene that rejects each variant
RULE_REJECTED_BY = {"running best replaced on > instead of >=": "two_equal_maxima", "convergence on >= instead of >": "equal_then_above",
                    "earliest of equal counts": "two_equal_maxima"}
RULE = scenes.rule_problems()


@pytest.mark.parametrize("name", sorted(RULE))
def test_result_rule_scenes(name):
    pb, _, want = RULE[name]
    o = scenes.find(s3, pb)
    counts, N, m = o["it_inliers"].tolist(), len(pb["Xw1"]), pb["min_inliers"]
    got = {k: o[k] for k in want}
    assert got == want, (name, counts)
    assert got == _rule_model(counts, N, m) == s3.result_rule(counts, N, m)
    if o["best_it"] >= 0:
        b = o["best_it"]
        assert o["T12"].tobytes() == o["it_T12"][b].tobytes() and o["s12"].tobytes() == o["it_scale"][b].tobytes()
        assert o["inliers"].sum() == o["n_inliers"] == counts[b]
    else:
        assert not o["T12"].any() and not o["inliers"].any() and not o["it_inliers"].any() and not o["it_T12"].any()


@pytest.mark.parametrize("variant", sorted(RULE_VARIANTS))
def test_result_rule_rejects_the_wrong_variants(variant):
    pb, _, want = RULE[RULE_REJECTED_BY[variant]]
    counts = scenes.find(s3, pb)["it_inliers"].tolist()
    wrong = RULE_VARIANTS[variant](counts, len(pb["Xw1"]), pb["min_inliers"])
    assert wrong != want, (variant, counts)
    # ... and on random counts the rule and the model agree everywhere while each variant is caught somewhere
    rng = np.random.default_rng(5)
    caught = 0
    for _ in range(300):
        c = rng.integers(0, 9, rng.integers(1, 12)).tolist(); m = int(rng.integers(0, 9))
        assert s3.result_rule(c, 8, m) == _rule_model(c, 8, m)
        caught += RULE_VARIANTS[variant](c, 8, m) != _rule_model(c, 8, m)
    assert caught > 0


def test_the_winners_do_not_depend_on_the_aids_and_early_stop_gives_the_same_result():
    pb = scenes.scene(64, seed=9, pair="pk", iters=65)
    with_aids, without = scenes.find(s3, pb, aids=True), scenes.find(s3, pb, aids=False)
    S = scenes.solver(s3, pb)
    prep = S.prepare(pb["sets"], aids=False)
    early = s3.result_dict(S.run(prep, stop_early=True), prep[1], prep[2])
    for k in without:
        assert np.asarray(with_aids[k]).tobytes() == np.asarray(without[k]).tobytes() == np.asarray(early[k]).tobytes(), k
    assert with_aids["converged"] == 1 and 0 < with_aids["best_it"] < 64


# ---- the probe ----------------------------------------------------------------------------------------------------------------------------
def probe_scene_set():
    """every problem the CPU and GPU tests run"""
    out = [scenes.scene(N, seed=N, pair=pair, wrong=w, fix_scale=fs, iters=it)
           for N, it, pair, w, fs in ((130, 65, "pp", 0.3, False), (65, 64, "kk", 0.0, True), (64, 63, "pk", 1.0, False), (63, 300, "kp", 0.3, True))]
    out += list(EDGE.values()) + [v[0] for v in RULE.values()] + [scenes.threshold_problem(s3)[0], scenes.large_coordinates()]
    return out


# The cap of the eigen-solver (maxIters = 480) is no branch a scene can reach: every rotation zeroes its pivot exactly and the others keep
# their own floating-point scale, so they fall under eps whatever the size of the diagonal.  Over 60 000 random symmetric matrices, with
# entries spread over 1e-35 .. 1e35 among them, the longest run was 27 rotations; NaN and inf entries end within three (the zeroed pivot is
# chosen next).  The cap stays in both restatements, as the source has it.
PROBE_UNREACHED = ("jacobi_exit_max_iters",)


def test_probe_every_branch_is_reached_by_the_scene_set():
    s3.probe_reset()
    for pb in probe_scene_set():
        scenes.find(s3, pb)
    p = s3.probe_read()
    print("probe:", ", ".join("%s %d" % kv for kv in p.items()))
    for k, v in p.items():
        assert v > 0 or k in s3.PROBE_ATAN2_ONLY or k in PROBE_UNREACHED, k
    s3.atan2([-1.0, -1.0], [2.0, -2.0])
    p = s3.probe_read()
    assert all(p[k] > 0 for k in s3.PROBE_ATAN2_ONLY)
