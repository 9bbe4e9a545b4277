"""Synthetic two-view scenes for the tests and the latency tool of the two-view reconstruction calls: two pinhole frames of a moving
camera, all keys of both (n1 != n2, the unmatched ones shift Normalize's means), the matches and the RANSAC sets."""
import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
K = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]], np.float32)
W, H = 640.0, 480.0


def kp_array(xy):
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"] = xy[:, 0]; k["y"] = xy[:, 1]; k["size"] = 31.0
    return k


def rot(axis, angle):
    axis = np.asarray(axis, np.float64); axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def true_pose():
    """camera 2 against camera 1: a small rotation and a unit translation, mostly sideways"""
    R = rot([0.2, 1.0, 0.1], 0.06)
    t = np.array([1.0, 0.05, 0.1]); t = t / np.linalg.norm(t)
    return R, t


def project(R, t, X):
    Xc = X @ R.T + t
    uv = Xc[:, :2] / Xc[:, 2:3]
    return uv * np.array([K[0, 0], K[1, 1]], np.float64) + np.array([K[0, 2], K[1, 2]], np.float64)


def points(kind, N, rng):
    """N scene points seen by camera 1 inside the image: planar (a slanted plane), general (depths 3 .. 9)"""
    uv = np.stack([rng.uniform(20, W - 20, N), rng.uniform(20, H - 20, N)], axis=1)
    ray = np.concatenate([(uv - [K[0, 2], K[1, 2]]) / [K[0, 0], K[1, 1]], np.ones((N, 1))], axis=1)
    if kind == "planar":
        n, d = np.array([0.1, -0.15, 1.0]), 6.0
        z = d / (ray @ n)
    else:
        z = rng.uniform(3.0, 9.0, N)
    return ray * z[:, None]


def scene(kind, N, seed=0, extra1=37, extra2=64, noise=0.3, outliers=0.0, far=0.0):
    """-> dict(kps1 [n1], kps2 [n2], matches [N, 2], X [N, 3] the matched scene points in camera 1, R, t).  kind: planar | general | noise |
    mixed (general, 30 % of the matches wrong).  far: the share of the points moved 3 000 times further away (no parallax: with the
    noise they triangulate to either side of the cameras)."""
    rng = np.random.default_rng(seed)
    R, t = true_pose()
    n1, n2 = N + extra1, N + extra2
    X = points("planar" if kind == "planar" else "general", N, rng)
    X[rng.random(N) < far] *= 3000.0
    uv1 = project(np.eye(3), np.zeros(3), X) + rng.normal(0, noise, (N, 2))
    uv2 = project(R, t, X) + rng.normal(0, noise, (N, 2))
    if kind == "mixed":
        outliers = 0.3
    if kind == "noise":
        outliers = 1.0
    bad = rng.random(N) < outliers
    uv2[bad] = np.stack([rng.uniform(0, W, bad.sum()), rng.uniform(0, H, bad.sum())], axis=1)
    first = np.sort(rng.permutation(n1)[:N]); second = rng.permutation(n2)[:N]
    k1 = np.stack([rng.uniform(0, W, n1), rng.uniform(0, H, n1)], axis=1); k2 = np.stack([rng.uniform(0, W, n2), rng.uniform(0, H, n2)], axis=1)
    k1[first] = uv1; k2[second] = uv2
    Xall = np.zeros((n1, 3)); Xall[first] = X
    return dict(kps1=kp_array(k1), kps2=kp_array(k2), matches=np.stack([first, second], axis=1).astype(np.int32), X=X, X_by_first=Xall, R=R, t=t,
                bad=bad)


def make_sets(N, iterations, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(N)[:8] for _ in range(iterations)]).astype(np.int32)


def decompose_e_poses(R, t):
    """the four (R, t) of DecomposeE (:1354-1375) + ReconstructF (:633-636) for E = [t]x R, in float64 with numpy"""
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    U, _, Vt = np.linalg.svd(tx @ R)
    tt = U[:, 2] / np.linalg.norm(U[:, 2])
    Wm = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1 = U @ Wm @ Vt
    R2 = U @ Wm.T @ Vt
    if np.linalg.det(R1) < 0:
        R1 = -R1
    if np.linalg.det(R2) < 0:
        R2 = -R2
    return [(R1, tt), (R2, tt), (R1, -tt), (R2, -tt)]


def poses27(Rts):
    """[Kp, 27] float32: R, t, P2 = K*[R|t], O2 = -R.t()*t (the caller's algebra, formed in float64 here and rounded)"""
    out = np.zeros((len(Rts), 27), np.float32)
    for h, (R, t) in enumerate(Rts):
        R = np.asarray(R, np.float32).astype(np.float64); t = np.asarray(t, np.float32).astype(np.float64)
        out[h, :9] = R.reshape(9); out[h, 9:12] = t
        out[h, 12:24] = (K.astype(np.float64) @ np.concatenate([R, t[:, None]], axis=1)).reshape(12)
        out[h, 24:27] = -(R.T @ t)
    return out
