"""Synthetic problems for the tests and the latency tool of the Sim3 solver: two keyframes of two maps that see the same points, the
maps related by a similarity; hand-derived edge problems; problems whose per-iteration counts are planted for the result rule; and the
planted correspondences of the threshold quirk.  A problem is a dict(Xw1, Xw2, Rt1, Rt2, cam1, cam2, sigma2_1, sigma2_2, fix_scale,
min_inliers, sets)."""
import numpy as np

PIN = (500.0, 500.0, 320.0, 240.0)
KB8 = (190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504, 0.0034823894022493434, 0.0007150348452162257,
       -0.0020532361418706202, 0.00020293673591811182)
UNIT = (1.0, 1.0, 100.0, 100.0)         # a pinhole whose image of (x, y, 1) is exactly (x + 100, y + 100) for |x|, |y| < 28
CAMS = {"p": PIN, "k": KB8}
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


def rot(axis, angle):
    axis = np.asarray(axis, np.float64); axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def rt12(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]).astype(np.float32)


def problem(Xw1, Xw2, Rt1=IDENT, Rt2=IDENT, cam1=PIN, cam2=PIN, sigma2_1=1.0, sigma2_2=1.0, fix_scale=False, min_inliers=6, sets=None):
    Xw1 = np.ascontiguousarray(Xw1, np.float32).reshape(-1, 3); Xw2 = np.ascontiguousarray(Xw2, np.float32).reshape(-1, 3)
    N = len(Xw1)
    return dict(Xw1=Xw1, Xw2=Xw2, Rt1=np.array(Rt1, np.float32), Rt2=np.array(Rt2, np.float32), cam1=tuple(cam1), cam2=tuple(cam2),
                sigma2_1=np.broadcast_to(np.asarray(sigma2_1, np.float32), (N,)).copy(),
                sigma2_2=np.broadcast_to(np.asarray(sigma2_2, np.float32), (N,)).copy(),
                fix_scale=bool(fix_scale), min_inliers=int(min_inliers),
                sets=np.ascontiguousarray(np.arange(3, dtype=np.int32).reshape(1, 3) if sets is None else sets, np.int32).reshape(-1, 3))


def solver(mod, pb, **kw):
    """mod: tests/sim3_ref or eorb_slam_amd.frontend -> its Sim3Solver on the problem"""
    s = mod.Sim3Solver(pb["Xw1"], pb["Xw2"], pb["Rt1"], pb["Rt2"], pb["cam1"], pb["cam2"], pb["sigma2_1"], pb["sigma2_2"], fix_scale=pb["fix_scale"], **kw)
    s.min_inliers = pb["min_inliers"]
    return s


def find(mod, pb, aids=True, **kw):
    return solver(mod, pb, **kw).find(pb["sets"], aids=aids)


def make_sets(N, iterations, seed=0):
    from . import draw_sets
    return draw_sets(N, iterations, seed)


def true_sim3(fix_scale):
    """camera 1 against camera 2: X1 = s R X2 + t"""
    return (1.0 if fix_scale else 1.3), rot([0.3, 1.0, -0.2], 0.35), np.array([0.4, -0.1, 0.25])


def scene(N, seed=0, pair="pp", wrong=0.3, fix_scale=False, noise=2e-3, iters=None, min_inliers=None):
    """N correspondences between keyframe 1 of map 1 and keyframe 2 of map 2; `wrong`: the share of correspondences whose second point is
    another point of the scene.  pair: the camera models of the two keyframes, p = Pinhole, k = KannalaBrandt8."""
    rng = np.random.default_rng(seed)
    cam1, cam2 = CAMS[pair[0]], CAMS[pair[1]]
    s, R, t = true_sim3(fix_scale)
    X1 = np.stack([rng.uniform(-2.0, 2.0, N), rng.uniform(-1.5, 1.5, N), rng.uniform(3.0, 9.0, N)], axis=1)      # in camera 1
    X2 = ((X1 - t) @ R) / s                                                                                     # in camera 2
    X2 = X2 + rng.normal(0, noise, (N, 3))
    bad = rng.random(N) < wrong
    X2[bad] = np.stack([rng.uniform(-2.0, 2.0, bad.sum()), rng.uniform(-1.5, 1.5, bad.sum()), rng.uniform(2.0, 7.0, bad.sum())], axis=1)
    R1, t1 = rot([0.1, -0.4, 1.0], 0.8), np.array([0.3, 1.2, -0.7])                                             # Tcw of the keyframes
    R2, t2 = rot([1.0, 0.2, 0.3], -0.5), np.array([-2.0, 0.4, 1.1])
    Xw1 = (X1 - t1) @ R1; Xw2 = (X2 - t2) @ R2
    lv1 = rng.integers(0, 8, N); lv2 = rng.integers(0, 8, N)
    pb = problem(Xw1, Xw2, rt12(R1, t1), rt12(R2, t2), cam1, cam2, (1.2 ** (2 * lv1)).astype(np.float32), (1.2 ** (2 * lv2)).astype(np.float32),
                 fix_scale, 6 if min_inliers is None else min_inliers)
    pb["sets"] = make_sets(N, 40 if iters is None else iters, seed + 1)
    pb["bad"] = bad
    return pb


# ---- hand-derived edge problems -----------------------------------------------------------------------------------------------------------
TRI = np.array([[0.5, -0.25, 4.0], [-1.0, 0.75, 5.0], [0.25, 1.0, 6.5]])       # a non-collinear triple in front of a camera
EXTRA = np.array([[0.75, 0.5, 3.5], [-0.5, -1.0, 7.0]])


def edge_problems():
    """name -> problem.  Every one has N = 5 and min_inliers = 2 unless it says otherwise."""
    P = np.concatenate([TRI, EXTRA])
    out = {}
    # identical triples: q = (1, 0, 0, 0), norm(vec) = 0, the factor 0/0: an all-NaN transform, 0 inliers, and still the running best
    out["identical"] = problem(P, P, min_inliers=2, sets=[[0, 1, 2], [2, 3, 4], [4, 0, 1]])
    # a 180 degree rotation about z, then about an oblique axis: evec(0, 0) at or near 0
    Rz = np.diag([-1.0, -1.0, 1.0])
    out["half_turn_z"] = problem(P, P @ Rz.T, min_inliers=2, sets=[[0, 1, 2], [1, 3, 4]])
    Ro = rot([1.0, 2.0, 2.0], np.pi)
    out["half_turn_oblique"] = problem(P, P @ Ro.T + [0.5, 0.0, 9.0], min_inliers=2, sets=[[0, 1, 2], [0, 2, 4]])
    # a collinear triple: M has rank 1, the rotation about the line is undetermined
    L = np.array([[0.0, 0.0, 4.0], [0.5, 0.25, 5.0], [1.0, 0.5, 6.0]])
    s, R, t = true_sim3(False)
    PL = np.concatenate([L, EXTRA])
    out["collinear"] = problem(PL, ((PL - t) @ R) / s, min_inliers=2, sets=[[0, 1, 2], [0, 1, 3]])
    # a set with a repeated index: two and three times
    out["repeated_index"] = problem(P, ((P - t) @ R) / s, min_inliers=2, sets=[[0, 0, 1], [3, 3, 3], [0, 1, 2]])
    # a point with z = 0 in camera 1 / in camera 2 (not in the set): the Pinhole quotient gives inf or NaN, the KannalaBrandt8 angle pi/2
    for cams in ("pp", "kk"):
        Z1 = P.copy(); Z1[3, 2] = 0.0
        out["z0_first_" + cams] = problem(Z1, ((P - t) @ R) / s, cam1=CAMS[cams[0]], cam2=CAMS[cams[1]], min_inliers=2, sets=[[0, 1, 2]])
        Z2 = ((P - t) @ R) / s; Z2[4] = [0.0, 0.0, 0.0]
        out["z0_second_" + cams] = problem(P, Z2, cam1=CAMS[cams[0]], cam2=CAMS[cams[1]], min_inliers=2, sets=[[0, 1, 2]])
    # N = 3, one iteration, fixed scale
    out["three_points"] = problem(TRI, (TRI - t) @ R, fix_scale=True, min_inliers=2, sets=[[2, 0, 1]])
    # coordinates of 1e15 against 1e-21: the pivot is above eps while s underflows towards 0, the quaternion's vector part is ~1e-36 and
    # the rotation vector shorter than DBL_EPSILON: Rodrigues takes its identity branch
    H = np.array([[1e15, 0.0, 1e-21], [-1e15, 0.0, -1e-21], [0.0, 1e-21, 2e-21], [0.5, 0.5, 4.0], [0.1, 0.2, 5.0]])
    H2 = H.copy(); H2[0, 2] = -1e-21; H2[1, 2] = 1e-21
    out["tiny_angle"] = problem(H, H2, min_inliers=2, sets=[[0, 1, 2]])
    # a NaN coordinate in a set point: N is all NaN, hypot falls through to its "return 0", and the solver ends within three rotations,
    # because every comparison with a NaN fails and the pivot search then lands on the entry it has just zeroed
    Q = P.copy(); Q[1, 0] = np.nan
    out["nan_point"] = problem(Q, ((P - t) @ R) / s, min_inliers=2, sets=[[0, 1, 2], [0, 2, 3]])
    return out


def large_coordinates(scale=1000.0):
    """the edge points in millimetres: M's entries are ~1e7, a float step of N's diagonal (~1) is far above the eigen-solver's absolute eps;
    the off-diagonal entries still fall under it, because they keep a floating-point scale of their own"""
    P = np.concatenate([TRI, EXTRA]) * scale
    s, R, t = true_sim3(False)
    return problem(P, ((P - t * scale) @ R) / s, min_inliers=2, sets=[[0, 1, 2], [1, 2, 3], [0, 3, 4]])


# ---- the result rule: two groups of correspondences, each consistent with its own similarity --------------------------------------------
def two_groups(a, b, min_inliers, order, extra=0):
    """group A (a correspondences, the first ones) fits one similarity exactly up to rounding, group B (b of them) another, `extra` fit
    neither.  order: a string over A / B / X, one iteration each: a set of three from that group (X: one of each kind, fits nothing).
    A set from group A counts a inliers, one from B counts b."""
    rng = np.random.default_rng(1000 * a + 10 * b + extra)
    N = a + b + extra
    assert a >= 3 and b >= 3
    X1 = np.stack([rng.uniform(-2.0, 2.0, N), rng.uniform(-1.5, 1.5, N), rng.uniform(3.0, 9.0, N)], axis=1)
    s, R, t = true_sim3(False)
    X2 = ((X1 - t) @ R) / s
    Rb, tb = rot([1.0, -0.5, 0.2], -0.6), np.array([-1.5, 0.8, 2.0])
    X2[a:a + b] = ((X1[a:a + b] - tb) @ Rb) / 0.8
    X2[a + b:] = X2[a + b:] + rng.uniform(1.0, 2.0, (extra, 3))
    sets = []
    for j, g in enumerate(order):
        if g == "A":
            sets.append([(j + i) % a for i in range(3)])
        elif g == "B":
            sets.append([a + (j + i) % b for i in range(3)])
        else:
            sets.append([0, a, 1])
    return problem(X1, X2, min_inliers=min_inliers, sets=sets)


def rule_problems():
    """name -> (problem, the counts the iterations must have, dict of the expected result)"""
    out = {}
    out["equal_then_above"] = (two_groups(6, 7, 6, "XAB"), None, dict(converged=1, best_it=2, n_inliers=7, iterations_used=3))
    out["two_equal_maxima"] = (two_groups(5, 5, 6, "AXBX"), None, dict(converged=0, best_it=2, n_inliers=5, iterations_used=4))
    out["converges_at_0"] = (two_groups(8, 4, 6, "ABA"), None, dict(converged=1, best_it=0, n_inliers=8, iterations_used=1))
    out["converges_at_last"] = (two_groups(4, 8, 6, "AXAB"), None, dict(converged=1, best_it=3, n_inliers=8, iterations_used=4))
    out["n_below_min"] = (two_groups(3, 3, 7, "AB"), None, dict(converged=0, best_it=-1, n_inliers=0, iterations_used=0))
    out["n_equals_min"] = (two_groups(3, 3, 6, "AB"), None, dict(converged=0, best_it=1, n_inliers=3, iterations_used=2))
    return out


# ---- the threshold quirk ------------------------------------------------------------------------------------------------------------------
def threshold_problem(ref, sigma2=1.0):
    """Correspondences 0-2 are the set (exact up to rounding); 3.. are planted around the image the hypothesis gives their second point in
    camera 1, with the UNIT camera and an identity pose so that the first point's image is set exactly: the u difference is
    3.02 (err 9.12: between 9 and 9.21), exactly 3 (err = 9.0f), one float below 3, and 2.  The second error always passes (sigma2_2 = 1e6).
    ref: tests/sim3_ref (the hypothesis is read from its it_T12).  -> (problem, names of the planted correspondences in order)"""
    s, R, t = true_sim3(True)
    X1 = np.concatenate([TRI, np.zeros((4, 3))])
    X2q = np.array([[0.2, -0.4, 5.0], [-0.6, 0.1, 4.0], [0.8, 0.3, 6.0], [-0.3, -0.2, 7.0]])
    X2 = np.concatenate([(TRI - t) @ R, X2q])
    pb = problem(X1, X2, cam1=UNIT, cam2=UNIT, sigma2_1=sigma2, sigma2_2=[1.0, 1.0, 1.0, 1e6, 1e6, 1e6, 1e6], fix_scale=True, min_inliers=2)
    T12 = find(ref, pb)["it_T12"][0]
    names = ["between_9_and_9.21", "exactly_9", "one_float_below_9", "err_4"]
    for j, name in enumerate(names):
        uq, vq = ref.project(T12, UNIT, pb["Xw2"][3 + j])
        assert 64.0 <= uq < 120.0 and 64.0 <= vq < 128.0
        du = {0: np.float32(3.02), 1: np.float32(3.0), 2: np.float32(3.0), 3: np.float32(2.0)}[j]
        u = np.float32(uq + du)
        if j == 2:
            u = np.nextafter(u, np.float32(0))
        pb["Xw1"][3 + j] = [np.float32(u - np.float32(100.0)), np.float32(vq - np.float32(100.0)), 1.0]
    return pb, names
