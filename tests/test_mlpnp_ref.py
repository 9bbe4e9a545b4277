"""The CPU restatement of the MLPnP solver (tests/mlpnp_ref, whose scalar algebra is eorb_slam_amd/csrc/mlpnp_core.h, the text the device
compiles too) held to plain float64 numpy models, piece by piece; the result rule held to a Python model with every named wrong variant
rejected by a named scene; and the branch probe.  No GPU.  Every tolerance in TOL is four times the largest deviation its seeds produce
against the numpy model (the `dev_*` functions below return those deviations; DESIGN.md section 2 lists them)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlpnp_ref as mr                              # noqa: E402
from mlpnp_ref import scenes                        # noqa: E402

TOL = {
    "nullspace_nf": 4 * 5.8e-16, "nullspace_orth": 4 * 6.7e-16,
    "svd_values": 4 * 4.2e-15, "svd_orth": 4 * 6.3e-15, "svd_last": 4 * 1.2e-15, "svd_deficient_value": 4 * 1.2e-16, "svd_deficient_residual": 4 * 3.1e-16,
    "eig_values": 4 * 2.2e-15, "eig_residual": 4 * 2.1e-15, "ldlt": 4 * 5.7e-15,
    # (n, planar, camera).  The planar branch ends its refinement at |dl| < 1e-5 a step earlier than the non-planar one, which leaves
    # ~1e-7; the KannalaBrandt8 rows carry the float32 pixel and the float unproject.
    "pose_planted": {(6, False, "p"): 4 * 1.1e-14, (6, False, "k"): 4 * 1.8e-6, (6, True, "p"): 4 * 6.6e-8, (6, True, "k"): 4 * 7.9e-7,
                     (60, False, "p"): 4 * 1.3e-15, (60, False, "k"): 4 * 4.1e-7, (60, True, "p"): 4 * 5.4e-8, (60, True, "k"): 4 * 2.7e-7},
    "pose_model": {(6, False, "p"): 4 * 2.0e-14, (6, False, "k"): 4 * 1.2e-13, (6, True, "p"): 4 * 2.2e-13, (6, True, "k"): 4 * 7.8e-14,
                   (60, False, "p"): 4 * 1.6e-15, (60, False, "k"): 4 * 1.5e-15, (60, True, "p"): 4 * 5.3e-14, (60, True, "k"): 4 * 1.1e-13},
    "jacobian": 4 * 3.4e-10,
}


def test_the_library_exports_the_entry_point():
    """fails on the parent commit: the ABI has no eorb_mlpnp_ransac"""
    from eorb_slam_amd import _lib
    assert "eorb_mlpnp_ransac" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "eorb_mlpnp_ransac")
    assert (_lib.PNP_MAX_ITERS, _lib.PNP_MAX_CORR, _lib.PNP_MAX_PROBLEMS) == (1024, 4096, 64)
    import ctypes as C
    assert C.sizeof(_lib.MlpnpResult) == 88 and C.sizeof(_lib.MlpnpProblem) == C.sizeof(mr.Problem) == 24 + C.sizeof(mr.Camera)


# ---- nullspace ---------------------------------------------------------------------------------------------------------------------------
def dev_nullspace():
    rng = np.random.default_rng(1)
    f = np.concatenate([rng.normal(size=(1000, 2)) * rng.choice([0.01, 0.5, 3.0], (1000, 1)), np.ones((1000, 1))], axis=1)
    ns = mr.nullspace(f)
    fu = f / np.linalg.norm(f, axis=1, keepdims=True)
    return np.abs(np.einsum("nij,ni->nj", ns, fu)).max(), np.abs(np.einsum("nij,nik->njk", ns, ns) - np.eye(2)).max()


def test_nullspace_against_numpy_and_by_hand():
    nf, orth = dev_nullspace()
    print("nullspace |n.f| %.3g |N^T N - I| %.3g" % (nf, orth))
    assert nf <= TOL["nullspace_nf"] and orth <= TOL["nullspace_orth"]
    # by hand: f = (0, 0, 1): beta = -1, essential (0, 1), tau = 1: Q = [[0, 0, -1], [0, 1, 0], [-1, 0, 0]]
    assert np.array_equal(mr.nullspace([[0, 0, 1.0]])[0], [[0, -1], [1, 0], [0, 0]])
    # f along x: the tail is zero, no reflection, Q = I; f along y: beta = -1, essential (1, 0): Q = [[0, -1, 0], [-1, 0, 0], [0, 0, 1]]
    assert np.array_equal(mr.nullspace([[1.0, 0, 0]])[0], [[0, 0], [1, 0], [0, 1]])
    assert np.array_equal(mr.nullspace([[0, 1.0, 0]])[0], [[-1, 0], [0, 0], [0, 1]])
    assert np.array_equal(mr.nullspace([[0, 0, 7.0]])[0], mr.nullspace([[0, 0, 1.0]])[0])       # the scale by the largest |entry|


# ---- Jacobi SVD --------------------------------------------------------------------------------------------------------------------------
def dev_svd():
    rng = np.random.default_rng(2)
    dv = do = dl = 0.0
    for n in (3, 9, 12):
        for _ in range(40):
            A = rng.normal(size=(n, n)) * 10.0 ** rng.integers(-3, 4)
            sv, V, U, rot = mr.jsvd(A, True)
            u, s, vt = np.linalg.svd(A)
            dv = max(dv, np.abs(sv - s).max() / s[0])
            do = max(do, np.abs(V.T @ V - np.eye(n)).max(), np.abs(U.T @ U - np.eye(n)).max())
            last = V[:, -1] * np.sign(V[:, -1] @ vt[-1])
            dl = max(dl, np.abs(last - vt[-1]).max() * (s[-2] - s[-1]) / s[0])      # scaled by the gap that conditions the vector
            assert np.all(np.diff(sv) <= 0) and rot > 0
    return dv, do, dl


def dev_svd_deficient():
    """A^T A of a minimal set: 12 rows, so rank 11 of 12"""
    rng = np.random.default_rng(3)
    dv = dr = 0.0
    for _ in range(40):
        A = rng.normal(size=(12, 12)); A[11] = 0
        S = A.T @ A
        sv, V, _, _ = mr.jsvd(S)
        dv = max(dv, sv[-1] / sv[0])
        dr = max(dr, np.abs(S @ V[:, -1]).max() / sv[0])
    return dv, dr


def test_jacobi_svd_against_numpy():
    dv, do, dl = dev_svd()
    print("svd values %.3g orthogonality %.3g last vector %.3g" % (dv, do, dl))
    assert dv <= TOL["svd_values"] and do <= TOL["svd_orth"] and dl <= TOL["svd_last"]
    dv, dr = dev_svd_deficient()
    print("rank-deficient: smallest value %.3g, |S v| %.3g" % (dv, dr))
    assert dv <= TOL["svd_deficient_value"] and dr <= TOL["svd_deficient_residual"]
    sv, V, U, rot = mr.jsvd(np.diag([3.0, -5.0, 1.0, 0.0, 2.0, 4.0, 6.0, 7.0, 8.0]), True)
    assert rot == 0                                     # a diagonal matrix executes no rotation: signs and the sort only
    assert np.array_equal(sv, [8, 7, 6, 5, 4, 3, 2, 1, 0]) and np.array_equal(np.abs(V).sum(axis=0), np.ones(9)) and U[1, 3] == -1


# ---- rank, eigen-solver, LDLT ------------------------------------------------------------------------------------------------------------
def test_rank_of_planted_matrices():
    rng = np.random.default_rng(4)
    for _ in range(50):
        B = rng.normal(size=(3, 3))
        for r in (1, 2, 3):
            M = B[:, :r] @ B[:, :r].T
            assert mr.rank3(M) == r
    P = rng.uniform(-3, 3, (3, 12)); P[2] = 0
    assert mr.rank3(P @ P.T) == 2                       # a z = 0 world: the planar branch
    P[2] = 1e-9 * rng.uniform(-1, 1, 12)
    # lifted by 1e-9 the third pivot is ~1e-18 * 12 against a largest pivot of ~40 and a threshold of 3 eps * 40 = 2.7e-14: still planar
    assert mr.rank3(P @ P.T) == 2
    P[2] = 1e-6 * rng.uniform(-1, 1, 12)                # ~1e-12 * 12 / 3: above the threshold, non-planar
    assert mr.rank3(P @ P.T) == 3


def dev_eig():
    rng = np.random.default_rng(5)
    dv = dr = 0.0
    for k in range(200):
        B = rng.normal(size=(3, 3 if k % 2 else 2)) * 10.0 ** rng.integers(-2, 3)
        S = B @ B.T
        w, Q = mr.eig3(S)
        dv = max(dv, np.abs(w - np.linalg.eigh(S)[0]).max() / np.abs(S).max())
        dr = max(dr, np.abs(Q @ np.diag(w) @ Q.T - S).max() / np.abs(S).max(), np.abs(Q.T @ Q - np.eye(3)).max())
        assert w[0] <= w[1] <= w[2]
    return dv, dr


def test_self_adjoint_eigen_solver_against_numpy():
    dv, dr = dev_eig()
    print("eig values %.3g residual %.3g" % (dv, dr))
    assert dv <= TOL["eig_values"] and dr <= TOL["eig_residual"]


def dev_ldlt():
    rng = np.random.default_rng(6)
    d = 0.0
    for _ in range(200):
        J = rng.normal(size=(20, 6)) * rng.uniform(0.1, 10, 6)
        A, g = J.T @ J, rng.normal(size=6)
        x = np.linalg.solve(A, g)
        d = max(d, np.abs(mr.ldlt_solve(A, g) - x).max() / np.abs(x).max())
    return d


def test_ldlt_solve_against_numpy():
    d = dev_ldlt()
    print("ldlt %.3g" % d)
    assert d <= TOL["ldlt"]


# ---- computePose -------------------------------------------------------------------------------------------------------------------------
def _planted(n, planar, cam, seed):
    """Pinhole: exact bearing vectors in float64.  KannalaBrandt8: what the solver's constructor makes of the float32 pixel, the
    oracle's float unproject (:80-82), so the planted pose is met to float accuracy only; the numpy model gets the same vectors."""
    R, t = scenes.planar_pose(seed) if planar else scenes.true_pose(seed)
    Xw = scenes.world_points(n, np.random.default_rng(seed), R, t, planar)
    Xc = Xw @ R.T + t
    if cam == "p":
        return Xc / Xc[:, 2:3], Xw, R, t
    from oracle import oracle_py
    px = scenes.project(scenes.KB8, Xc).astype(np.float32)
    f = np.array([oracle_py.unproject(scenes.KB8, float(x), float(y)) for x, y in px], np.float64)
    return f / f[:, 2:3], Xw, R, t


def dev_pose(n, planar, cam):
    dp = dm = 0.0
    for seed in range(40):
        f, Xw, R, t = _planted(n, planar, cam, seed)
        Rr, tr = mr.compute_pose(f, Xw)
        Rm, tm = scenes.model_pose(f, Xw)
        dp = max(dp, np.abs(Rr - R).max(), np.abs(tr - t).max())
        dm = max(dm, np.abs(Rr - Rm).max(), np.abs(tr - tm).max())
    return dp, dm


@pytest.mark.parametrize("n", [6, 60])
@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("cam", ["p", "k"])
def test_compute_pose_on_planted_poses(n, planar, cam):
    dp, dm = dev_pose(n, planar, cam)
    print("computePose n=%d planar=%d %s: against the planted pose %.3g, against the numpy model %.3g" % (n, planar, cam, dp, dm))
    assert dp <= TOL["pose_planted"][(n, planar, cam)] and dm <= TOL["pose_model"][(n, planar, cam)]


# ---- the Jacobian ------------------------------------------------------------------------------------------------------------------------
def dev_jacobian():
    rng = np.random.default_rng(7)
    d = 0.0
    for _ in range(200):
        x = np.concatenate([rng.normal(size=3) * rng.choice([0.01, 0.5, 1.5]), rng.normal(size=3)])
        X = rng.normal(size=3) + [0, 0, 5]
        ns = mr.nullspace([np.append(rng.normal(size=2) * 0.4, 1.0)])[0]
        _, J = mr.residual_jac(x, X, ns)
        Jn = np.zeros((2, 6))
        for k in range(6):
            h = np.zeros(6); h[k] = 1e-6
            Jn[:, k] = (mr.residual_jac(x + h, X, ns)[0] - mr.residual_jac(x - h, X, ns)[0]) / 2e-6
        d = max(d, np.abs(J - Jn).max())
    return d


def test_jacobian_against_central_differences():
    d = dev_jacobian()
    print("jacobian %.3g" % d)
    assert d <= TOL["jacobian"]
    # omega = 0: (w_i w + w x c_i) / (w . w) is 0/0, so the rotation columns are NaN as the source's 1/sqrt(0) makes them; the
    # translation columns and the residual are finite
    r, J = mr.residual_jac(np.array([0, 0, 0, 0.1, 0.2, 0.3]), np.array([0.5, -0.5, 4.0]), mr.nullspace([[0.1, 0.2, 1.0]])[0])
    assert np.isnan(J[:, :3]).all() and np.isfinite(J[:, 3:]).all() and np.isfinite(r).all()


# ---- acos / pow against the host libm ----------------------------------------------------------------------------------------------------
def _ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


def test_dacos_and_dpow_against_the_host_libm():
    """fdlibm documents < 1 ulp for both, glibc < 1 ulp: never more than 2 ulp apart.  Measured with glibc 2.35: acos at most 1 ulp apart
    on 7.6 % of 2^20 arguments, pow(x, 1/3) at most 1 ulp apart on 9.7 %."""
    rng = np.random.default_rng(8)
    x = rng.uniform(-1, 1, 1 << 20); x[:4] = [1.0, -1.0, 0.0, 0.5]
    u = _ulps(mr.acos(x), mr.acos(x, host=True))
    print("acos: max %d ulp, differing share %.4f" % (u.max(), (u > 0).mean()))
    assert u.max() <= 2
    x = 1.0 - rng.uniform(0, 1, 1 << 20); x[:3] = [1.0, 0.5, 1e-300]
    u = _ulps(mr.pow_(x, 1.0 / 3.0), mr.pow_(x, 1.0 / 3.0, host=True))
    print("pow: max %d ulp, differing share %.4f" % (u.max(), (u > 0).mean()))
    assert u.max() <= 2
    assert np.isnan(mr.acos([1.5, np.nan])).all() and np.isnan(mr.pow_([np.nan], 1 / 3)).all() and mr.pow_([0.0], 1 / 3)[0] == 0


SCENE_SET = [dict(N=N, seed=s, cam=c, wrong=w, planar=p, iters=30) for N in (30, 100) for s in (1, 2) for c in "pk" for w in (0.0, 0.3, 1.0)
             for p in (False, True)]


def test_host_libm_changes_are_counted():
    """how many float entries of Tcw and how many counts change over the scene set when the restatement uses the host's acos / pow:
    recorded, not bounded"""
    base = [scenes.find(mr, scenes.scene(**kw)) for kw in SCENE_SET]
    mr.set_option(mr.OPT_HOST_LIBM, 1)
    try:
        host = [scenes.find(mr, scenes.scene(**kw)) for kw in SCENE_SET]
    finally:
        mr.set_option(mr.OPT_HOST_LIBM, 0)
    tcw = sum(int((a["Tcw"].view(np.uint32) != b["Tcw"].view(np.uint32)).sum()) for a, b in zip(base, host))
    cnt = sum(int((a["it_inliers"] != b["it_inliers"]).sum()) for a, b in zip(base, host))
    print("host acos / pow: %d of %d Tcw floats and %d of %d counts change" % (tcw, 16 * len(base), cnt, 30 * len(base)))


# ---- the bound ---------------------------------------------------------------------------------------------------------------------------
def test_the_bound_is_a_float_product_and_strict():
    s2, th2 = np.float32(1.44), np.float32(5.991)
    b = s2 * th2
    assert mr.bound_test(np.nextafter(b, np.float32(0)), s2, th2) and not mr.bound_test(b, s2, th2) and not mr.bound_test(np.nextafter(b, np.float32(100)), s2, th2)
    mr.set_option(mr.OPT_BOUND_LE, 1)
    try:
        assert mr.bound_test(b, s2, th2)                 # the named wrong variant <= accepts the planted error: the scene rejects it
    finally:
        mr.set_option(mr.OPT_BOUND_LE, 0)
    assert not mr.bound_test(np.nan, s2, th2)


# ---- the result rule ---------------------------------------------------------------------------------------------------------------------
def _rule(pb, variant=None, first_it=0, best_it=-1):
    """the Python model of the rule on the restatement's own per-iteration counts (and, for the variant in which Refine stores its pose,
    on the count of the pose re-estimated from iteration b's flags)"""
    s = scenes.solver(mr, pb)
    o = s.find(pb["sets"], aids=True)
    return scenes.rule_model(o["it_inliers"], pb["min_inliers"], first_it, best_it, variant, stored=lambda b: s.refine_from(o["it_Rt"][b])[0])


VARIANTS = {"best_ge": mr.OPT_BEST_GE, "refine_stores": mr.OPT_REFINE_STORES, "refine_ge": mr.OPT_REFINE_GE, "trigger_gt": mr.OPT_TRIGGER_GT}
RULE_SCENES = {
    # two sets of pose A (12 = min_inliers inliers each): on >= the later one becomes the best
    "best_ge": lambda: scenes.two_pose_scene(12, 0, 28, seed=6, head="AJA"),
    # Refine computes a pose from the best's inliers and never stores it (:367-371): what it returns is the current hypothesis, 39
    # inliers here; the pose it drops would have 46
    "refine_stores": lambda: scenes.scene(64, seed=6463, cam="k", wrong=0.3, planar=True, iters=63, min_inliers=10),
    # exactly min_inliers: the trigger fires (>=), Refine's own test (>) fails
    "refine_ge": lambda: scenes.best_returned_scene(),
    "trigger_gt": lambda: scenes.best_returned_scene(),
}


@pytest.mark.parametrize("name", sorted(RULE_SCENES))
def test_result_rule_against_the_python_model(name):
    pb = RULE_SCENES[name]()
    o = scenes.find(mr, pb)
    got = {k: o[k] for k in scenes.RULE_KEYS}
    assert got == _rule(pb), name
    wrong = _rule(pb, name)
    assert wrong != got, "the scene does not tell the variant %s from the rule" % name
    mr.set_option(VARIANTS[name], 1)                     # the restatement built with the wrong variant gives the model's wrong answer
    try:
        w = scenes.find(mr, pb)
    finally:
        mr.set_option(VARIANTS[name], 0)
    assert {k: w[k] for k in scenes.RULE_KEYS} == wrong


def test_refined_is_the_current_hypothesis():
    """mRefinedTcw / mvbRefinedInliers are the pose and flags of the iteration Refine returned true at (:374-387 read mRi / mti, which
    only :200-212 write), and it_refine_inliers holds the count again at every iteration that invoked Refine"""
    pb = RULE_SCENES["refine_stores"]()
    o = scenes.find(mr, pb)
    s = o["stop_it"]
    assert o["refined"] == 1 and o["n_inliers"] == o["it_inliers"][s] == o["n_best"] and o["best_it"] == s
    Rt = o["it_Rt"][s]
    want = np.eye(4, dtype=np.float32); want[:3, :3] = Rt[:9].reshape(3, 3).astype(np.float32); want[:3, 3] = Rt[9:].astype(np.float32)
    assert o["Tcw"].tobytes() == want.tobytes() and int(o["inliers"].sum()) == o["n_inliers"]
    invoked = np.arange(len(o["it_inliers"])) <= s
    invoked &= o["it_inliers"] >= pb["min_inliers"]
    assert np.array_equal(o["it_refine_inliers"], np.where(invoked, o["it_inliers"], -1))


def test_rule_model_on_the_scene_set():
    for kw in SCENE_SET[::3]:
        pb = scenes.scene(**kw)
        o = scenes.find(mr, pb)
        assert {k: o[k] for k in scenes.RULE_KEYS} == _rule(pb), kw


def test_resumed_walks_equal_the_one_shot_walk():
    pb = scenes.resume_scene()
    one = scenes.find(mr, pb)
    assert one["stop_it"] == 100
    s = scenes.solver(mr, pb)
    for first_it in range(1, 130):
        carried = scenes.rule_model(one["it_inliers"][:first_it], pb["min_inliers"])["best_it"]
        o = s.find(pb["sets"], aids=True, first_it=first_it, best_it=carried)
        replay = scenes.rule_model(one["it_inliers"], pb["min_inliers"], first_it, carried)      # a replay from the aids
        assert {k: o[k] for k in scenes.RULE_KEYS} == replay, first_it
        if first_it <= 100:
            assert {k: o[k] for k in scenes.RULE_KEYS} == {k: one[k] for k in scenes.RULE_KEYS}
            assert o["Tcw"].tobytes() == one["Tcw"].tobytes() and o["inliers"].tobytes() == one["inliers"].tobytes()


def test_the_loop_condition_is_an_or():
    """iterate(5, ...): the first call runs to mRansacMaxIts unless Refine returns, every later call five more; with && the first call
    would stop after five.  This holds the test helper iterate_calls, which tests/test_gpu_mlpnp.py and tests/test_host_mlpnp_cpp.py
    hold the Python and the C++ mirror to."""
    pb = scenes.false_scene(40, seed=9, iters=60)
    s = scenes.solver(mr, pb)
    s.iters = 50
    calls = mr.iterate_calls(s, pb["sets"], 5, 3)
    assert [c["iterations"] for c in calls] == [50, 55, 60] and all(c["no_more"] for c in calls)
    wrong = mr.iterate_calls(s, pb["sets"], 5, 3, loop_and=True)
    assert [c["iterations"] for c in wrong] == [5, 10, 15]


def test_ransac_parameters():
    assert mr.ransac_parameters(65) == (32, 35) and mr.ransac_parameters(12) == (10, 6) and mr.ransac_parameters(10) == (10, 1)
    assert mr.ransac_parameters(8) == (10, 1)            # epsilon = 10/8: log of a negative number, NaN, INT_MIN, 1
    assert mr.ransac_parameters(1000, max_iterations=20) == (500, 20)
    # (mr.ransac_parameters / mr.draw_sets are the product's own functions: the values above are computed by hand, 65: int(32.5) = 32,
    # epsilon 0.5, ceil(log 0.01 / log 0.875) = ceil(34.49); 12: epsilon 10/12, ceil(log 0.01 / log(1 - 0.5787)) = ceil(5.33))
    sets = mr.draw_sets(7, 50, 1)
    assert all(len(set(r)) == 6 for r in sets.tolist()) and sets.min() == 0 and sets.max() == 6


# ---- the branch probe --------------------------------------------------------------------------------------------------------------------
# every branch is reached; the probe test fails if one is not, and a branch that cannot be reached has to be named here with its reason
UNREACHED = {}


def test_branch_probe():
    mr.probe_reset()
    for kw in SCENE_SET:
        scenes.find(mr, scenes.scene(**kw))
    for name in ("records_scene", "best_returned_scene"):
        scenes.find(mr, getattr(scenes, name)())
    scenes.find(mr, scenes.scene(8, seed=1, iters=3, min_inliers=10))                      # N < min_inliers
    # a tilted plane through the origin: M(2, 0) != 0, the general tridiagonalisation
    rng = np.random.default_rng(11)
    R, t = scenes.planar_pose(3)
    Xw = scenes.world_points(12, rng, R, t, True) @ scenes.rot([1, 2, 0.5], 0.7).T
    Xc = Xw @ R.T + t
    mr.compute_pose(Xc / Xc[:, 2:3], Xw)
    mr.residual_jac(np.array([0, 0, 0, 0.1, 0.2, 0.3]), np.array([0.5, -0.5, 4.0]), mr.nullspace([[0.1, 0.2, 1.0]])[0])      # omega = 0
    # the identity pose with exact data: the rotation estimate is the identity to the last bit, rot2rodrigues takes its zero branch, and
    # omega = 0 makes the Jacobian NaN (above) as the source's 1/sqrt(0) does: the step and the translation are NaN, and rodrigues2rot of a
    # NaN omega fails its > eps and leaves the identity
    Xi = np.array([[1, 2, 4], [-2, 1, 5], [3, -1, 6], [-1, -2, 8], [2, 3, 7], [0, 1, 3]], np.float64)
    before = mr.probe_read()["rodrigues_zero"]
    Ri, ti = mr.compute_pose(Xi / Xi[:, 2:3], Xi)
    assert mr.probe_read()["rodrigues_zero"] == before + 1 and np.array_equal(Ri, np.eye(3)) and np.isnan(ti).all()
    mr.jsvd(np.diag([2.0, 1.0, 3.0]))                                                      # a diagonal matrix: no rotation (no scene gives one)
    p = mr.probe_read()
    missing = [k for k, v in p.items() if v == 0 and k not in UNREACHED]
    assert not missing, missing
