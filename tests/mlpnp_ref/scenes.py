"""Synthetic problems for the tests and the latency tool of the MLPnP solver: a frame that sees map points under a planted pose, with a
share of wrong matches; a plain float64 numpy model of MLPnP (independent of the C text); and the Python model of the result rule.
A problem is a dict(p2d, Xw, sigma2, cam, min_inliers, th2, sets, R, t, bad)."""
import numpy as np

PIN = (500.0, 500.0, 320.0, 240.0)
KB8 = (190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504, 0.0034823894022493434, 0.0007150348452162257,
       -0.0020532361418706202, 0.00020293673591811182)
CAMS = {"p": PIN, "k": KB8}
TH2 = 5.991


def rot(axis, angle):
    axis = np.asarray(axis, np.float64); axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def project(cam, Xc):
    """float64 model of both cameras: [n, 3] camera points -> [n, 2] pixels"""
    Xc = np.asarray(Xc, np.float64)
    if len(cam) == 4:
        return np.stack([cam[0] * Xc[:, 0] / Xc[:, 2] + cam[2], cam[1] * Xc[:, 1] / Xc[:, 2] + cam[3]], axis=1)
    r = np.hypot(Xc[:, 0], Xc[:, 1]); th = np.arctan2(r, Xc[:, 2]); psi = np.arctan2(Xc[:, 1], Xc[:, 0])
    d = th + cam[4] * th ** 3 + cam[5] * th ** 5 + cam[6] * th ** 7 + cam[7] * th ** 9
    return np.stack([cam[0] * d * np.cos(psi) + cam[2], cam[1] * d * np.sin(psi) + cam[3]], axis=1)


def true_pose(seed=0):
    """Tcw of the frame: Xc = R Xw + t"""
    rng = np.random.default_rng(1000 + seed)
    return rot(rng.normal(size=3), rng.uniform(0.2, 1.2)), rng.uniform(-1.0, 1.0, 3)


def world_points(N, rng, R, t, planar=False):
    """points in front of the camera; planar: on the plane z = 0 of the world (a plane through the origin, which the rank test sees)"""
    if not planar:
        Xc = np.stack([rng.uniform(-2.0, 2.0, N), rng.uniform(-1.5, 1.5, N), rng.uniform(3.0, 9.0, N)], axis=1)
        return (Xc - t) @ R
    # the plane z = 0 of the world, in camera coordinates: normal R[:, 2], through t; rays of the image hit it
    out = []
    while len(out) < N:
        d = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), 1.0])
        nrm = R[:, 2]
        den = nrm @ d
        if abs(den) < 0.2:
            continue
        lam = (nrm @ t) / den
        if not 0.8 < lam < 4.0:
            continue
        Xw = (lam * d - t) @ R
        out.append([Xw[0], Xw[1], 0.0])
    return np.array(out)


def planar_pose(seed=0):
    """a pose that looks at the world's z = 0 plane from about two units away.  The distance matters: the planar branch takes its
    translation scale from the columns of the transposed matrix (:585-587), which is right only near unit scale, and from farther away
    the first Gauss-Newton step exceeds the dx guard (:788) and the linear translation is returned as it is."""
    rng = np.random.default_rng(2000 + seed)
    R = rot([1.0, 0.0, 0.0], np.pi - rng.uniform(0.1, 0.5)) @ rot(rng.normal(size=3), rng.uniform(0.05, 0.4))
    return R, np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(1.5, 2.5)])


def problem(p2d, Xw, sigma2=1.0, cam=PIN, min_inliers=10, th2=TH2, sets=None, **extra):
    p2d = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2); Xw = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
    N = len(p2d)
    pb = dict(p2d=p2d, Xw=Xw, sigma2=np.broadcast_to(np.asarray(sigma2, np.float32), (N,)).copy(), cam=tuple(cam), min_inliers=int(min_inliers),
              th2=float(th2), sets=np.ascontiguousarray(np.arange(6, dtype=np.int32).reshape(1, 6) if sets is None else sets, np.int32).reshape(-1, 6))
    pb.update(extra)
    return pb


def solver(mod, pb, **kw):
    """mod: tests/mlpnp_ref or eorb_slam_amd.frontend -> its MLPnPsolver on the problem"""
    s = mod.MLPnPsolver(pb["p2d"], pb["Xw"], pb["sigma2"], pb["cam"], **kw)
    s.min_inliers = pb["min_inliers"]; s.th2 = pb["th2"]
    return s


def find(mod, pb, aids=True, first_it=0, best_it=-1, **kw):
    return solver(mod, pb, **kw).find(pb["sets"], aids=aids, first_it=first_it, best_it=best_it)


def make_sets(N, iterations, seed=0):
    from . import draw_sets
    return draw_sets(N, iterations, seed)


def scene(N, seed=0, cam="p", wrong=0.3, planar=False, noise=0.3, iters=40, min_inliers=None):
    """N matches of a frame with map points; `wrong`: the share of matches whose keypoint is somewhere else in the image; noise: pixels"""
    rng = np.random.default_rng(seed)
    c = CAMS[cam]
    R, t = planar_pose(seed) if planar else true_pose(seed)
    Xw = world_points(N, rng, R, t, planar).astype(np.float32)
    p2d = project(c, Xw.astype(np.float64) @ R.T + t) + rng.normal(0, noise, (N, 2))
    bad = rng.random(N) < wrong
    p2d[bad] = np.stack([rng.uniform(40, 600, bad.sum()), rng.uniform(40, 440, bad.sum())], axis=1) if cam == "p" else \
        np.stack([rng.uniform(100, 400, bad.sum()), rng.uniform(100, 400, bad.sum())], axis=1)
    lv = rng.integers(0, 8, N)
    from . import ransac_parameters
    mi = ransac_parameters(N)[0] if min_inliers is None else min_inliers
    return problem(p2d, Xw, (1.2 ** (2 * lv)).astype(np.float32), c, mi, TH2, make_sets(N, iters, seed + 1), R=R, t=t, bad=bad)


def false_scene(N, seed=0, cam="p", iters=40):
    """a false candidate: no pose explains the matches"""
    return scene(N, seed, cam, wrong=1.0, iters=iters)


def two_pose_scene(nA, nB, njunk, seed=0, cam="p", min_inliers=12, head=()):
    """matches of two populations: the first nA agree with pose A, the next nB with pose B, the last njunk with nothing.  head: for each
    leading set, 'A' / 'B' (six matches of that population) or 'J' (junk); random sets follow.  Without noise, so that every match of a
    population is an inlier of its pose."""
    rng = np.random.default_rng(seed)
    c = CAMS[cam]
    N = nA + nB + njunk
    poses = [true_pose(seed), true_pose(seed + 50)]
    Xw = np.zeros((N, 3), np.float32); p2d = np.zeros((N, 2))
    for lo, hi, (R, t) in ((0, nA, poses[0]), (nA, nA + nB, poses[1])):
        if hi > lo:
            Xw[lo:hi] = world_points(hi - lo, rng, R, t).astype(np.float32)
            p2d[lo:hi] = project(c, Xw[lo:hi].astype(np.float64) @ R.T + t)
    Xw[nA + nB:] = world_points(njunk, rng, *poses[0]).astype(np.float32)
    p2d[nA + nB:] = np.stack([rng.uniform(40, 600, njunk), rng.uniform(40, 440, njunk)], axis=1)
    pick = {"A": lambda: rng.permutation(nA)[:6], "B": lambda: nA + rng.permutation(nB)[:6], "J": lambda: nA + nB + rng.permutation(njunk)[:6]}
    sets = np.concatenate([np.array([pick[h]() for h in head], np.int32).reshape(-1, 6), make_sets(N, 6, seed + 1)])
    return problem(p2d, Xw, 1.0, c, min_inliers, TH2, sets, R=poses[1][0], t=poses[1][1])


def records_scene():
    """more than one record before the successful Refine: set 1 agrees with the 12 matches of pose A, exactly min_inliers, so it becomes
    the running best and Refine is invoked, but 12 is not > 12; set 3 agrees with the 30 of pose B, replaces it and Refine returns true"""
    return two_pose_scene(12, 30, 18, seed=3, head="JAJB")


def resume_scene():
    """130 iterations with a record at 10 (pose A, 12 = min_inliers: Refine fails) and one at 100 (pose B, 30: Refine succeeds)"""
    return two_pose_scene(12, 30, 18, seed=5, head="J" * 10 + "A" + "J" * 89 + "B" + "J" * 23)


def best_returned_scene():
    """no Refine succeeds: the only consistent population has exactly min_inliers matches; the running best is returned (:249-262)"""
    return two_pose_scene(12, 0, 28, seed=4, head="JA")


# ---- a plain float64 numpy model of MLPnP (Urban et al. 2016), written from the paper's equations with numpy.linalg ----------------------
def model_nullspace(f):
    """an orthonormal basis of the plane orthogonal to f, by numpy's SVD"""
    f = np.asarray(f, np.float64)
    return np.linalg.svd(f.reshape(1, 3))[2][1:].T


def model_residuals(x, X, ns):
    R = rot(x[:3], np.linalg.norm(x[:3])) if np.linalg.norm(x[:3]) > 0 else np.eye(3)
    v = X @ R.T + x[3:]
    u = v / np.linalg.norm(v, axis=1, keepdims=True)
    return np.einsum("nij,ni->nj", ns, u).reshape(-1)


def model_pose(f, X, steps=5):
    """the linear MLPnP solution and `steps` Gauss-Newton steps with a numeric Jacobian and lstsq -> (R, t).  The sign and the planar
    four-fold ambiguity are decided by the reprojection direction as in the paper."""
    f = np.asarray(f, np.float64); X = np.asarray(X, np.float64); n = len(f)
    f = f / np.linalg.norm(f, axis=1, keepdims=True)
    ns = np.stack([model_nullspace(v) for v in f])
    S = X.T @ X
    planar = np.linalg.matrix_rank(S, tol=1e-9 * np.abs(S).max()) == 2
    E = np.eye(3)
    Xr = X
    if planar:
        E = np.linalg.eigh(S)[1].T
        Xr = X @ E.T
    cols = [(i, j) for i in range(3) for j in (range(1, 3) if planar else range(3))]
    A = np.zeros((2 * n, len(cols) + 3))
    for a in range(2):
        for c, (i, j) in enumerate(cols):
            A[a::2, c] = ns[:, i, a] * Xr[:, j]
        for i in range(3):
            A[a::2, len(cols) + i] = ns[:, i, a]
    v = np.linalg.svd(A)[2][-1]
    cands = []
    if planar:
        P = np.zeros((3, 3)); P[:, 1] = v[0:6:2]; P[:, 2] = v[1:6:2]; P[:, 0] = np.cross(P[:, 1], P[:, 2])
        P = P.T
        scale = 1.0 / np.sqrt(np.linalg.norm(P[:, 1]) * np.linalg.norm(P[:, 2]))
        U, _, Vt = np.linalg.svd(P)
        Rr = U @ Vt
        if np.linalg.det(Rr) < 0:
            Rr = -Rr
        Rr = -(E.T @ Rr).T
        if np.linalg.det(Rr) < 0:
            Rr[:, 2] *= -1
        tt = scale * v[6:9]
        R2 = Rr.copy(); R2[:, :2] *= -1
        cands = [(Rr, tt), (Rr, -tt), (R2, tt), (R2, -tt)]
    else:
        P = v[:9].reshape(3, 3).T      # v[:9] holds the rows of the world-to-camera rotation up to scale; the solver works on its transpose
        scale = 1.0 / np.cbrt(np.prod(np.linalg.norm(P, axis=0)))
        U, _, Vt = np.linalg.svd(P)
        Rr = U @ Vt
        if np.linalg.det(Rr) < 0:
            Rr = -Rr
        tt = Rr @ (scale * v[9:12])
        for s in (1.0, -1.0):
            Ti = np.linalg.inv(np.block([[Rr, (s * tt).reshape(3, 1)], [np.zeros((1, 3)), np.ones((1, 1))]]))
            cands.append((Ti[:3, :3], Ti[:3, 3]))

    def err(Rc, tc):
        w = X[:6] @ Rc.T + tc
        return np.sum(1.0 - np.sum(w / np.linalg.norm(w, axis=1, keepdims=True) * f[:6], axis=1))
    Rb, tb = min(cands, key=lambda c: err(*c))
    ang = np.arccos(np.clip((np.trace(Rb) - 1) / 2, -1, 1))
    om = np.zeros(3) if ang < 1e-12 else ang / (2 * np.sin(ang)) * np.array([Rb[2, 1] - Rb[1, 2], Rb[0, 2] - Rb[2, 0], Rb[1, 0] - Rb[0, 1]])
    x = np.concatenate([om, tb])
    for _ in range(steps):
        r0 = model_residuals(x, X, ns)
        J = np.zeros((2 * n, 6))
        for k in range(6):
            h = np.zeros(6); h[k] = 1e-6
            J[:, k] = (model_residuals(x + h, X, ns) - model_residuals(x - h, X, ns)) / 2e-6
        dx = np.linalg.lstsq(J, r0, rcond=None)[0]
        x = x - dx
        if np.abs(J @ dx).max() < 1e-5:
            break
    th = np.linalg.norm(x[:3])
    return (rot(x[:3], th) if th > 0 else np.eye(3)), x[3:]


# ---- the result rule (:163-265) as a Python model ---------------------------------------------------------------------------------------
def rule_model(counts, min_inliers, first_it=0, best_it=-1, variant=None, stored=None):
    """counts[it]: the inliers of every hypothesis.  Refine (:338-392) never stores the pose it computes, so the count it reaches is the
    current iteration's again and it succeeds when that is > min_inliers.
    variant: None, or one of the named wrong variants 'best_ge', 'refine_ge', 'trigger_gt', 'refine_stores' (Refine's count is that of
    the pose re-estimated from the running best's inliers: stored(b) gives it).
    -> dict(stop_it, iterations_used, best_it, n_best, refined, n_inliers)"""
    bi, bn = -1, 0
    if best_it >= 0 and counts[best_it] >= min_inliers:
        bi, bn = best_it, int(counts[best_it])
    stop, refn = -1, 0
    for it in range(first_it, len(counts)):
        n = int(counts[it])
        if (n > min_inliers) if variant == "trigger_gt" else (n >= min_inliers):
            if (n >= bn) if variant == "best_ge" else (n > bn):
                bi, bn = it, n
            refn = stored(bi) if variant == "refine_stores" else n
            if (refn >= min_inliers) if variant == "refine_ge" else (refn > min_inliers):
                stop = it
                break
    refined = int(stop >= 0)
    return dict(stop_it=stop, iterations_used=stop + 1 if refined else len(counts), best_it=bi, n_best=bn, refined=refined,
                n_inliers=refn if refined else (bn if bn >= min_inliers else 0))


RULE_KEYS = ("stop_it", "iterations_used", "best_it", "n_best", "refined", "n_inliers")
