"""Plain float64 / int64 numpy restatements of the float stages, written from the formulas of the algorithms alone: event
accumulation, the cameras, the motion-compensating warps, focus and min-max normalisation, IC_Angle, steered rBRIEF and pyramidal
Lucas-Kanade.  No fixed point, no float32 intermediates, no particular order of operations: where the oracle and the kernels
share a slip, these disagree with both.  tests/test_oracle_plain.py holds the oracle to them, tests/test_gpu_plain.py the kernels.

Every function takes a `wrong=` keyword naming a deliberately wrong variant (None: the right one); the tests use the variants
to show that their tolerances reject a real error."""
import os
import re

import numpy as np

F64 = np.float64
U = 2.0 ** -24                                    # unit roundoff of float32


# ---------------------------------------------------------------------------------------------------
# accumulation
def stamp_radius(sigma):
    """h = ceil(3 sigma), sigma being the float32 parameter the entry points receive."""
    return int(np.ceil(3.0 * F64(np.float32(sigma))))


def gauss_image(ev, W, H, sigma, pol, xy=None, wrong=None):
    """For every event k in order, with position (ex, ey) and sign s (-1 for a polarity-0 event when `pol`, else +1), every
    pixel (x, y) of the image with |x - floor(ex)| <= h and |y - floor(ey)| <= h, h = ceil(3 sigma), receives

        s exp(-((x - ex)^2 + (y - ey)^2) / (2 sigma^2)) / (2 pi sigma^2).

    `xy` (n, 2) float64 replaces the events' positions (the warped positions of a motion-compensated image).
    Returns dict(img, S = per-pixel sum of the terms' absolute values, M = per-pixel number of stamps that touched it,
    min, max = the running extremes (minVal from 0, maxVal from -1e6, updated after every event's stamp: extremes of partial
    sums), min_at, max_at = (y, x) of the pixel that set them (None: never set).
    wrong: "radius" uses h - 1; "swap" exchanges the fractional parts of x and y."""
    sigma = F64(np.float32(sigma))
    h = stamp_radius(sigma) - (1 if wrong == "radius" else 0)
    if xy is None:
        xy = np.stack([ev["x"].astype(F64), ev["y"].astype(F64)], axis=1)
    xy = np.asarray(xy, F64)
    sign = np.where(ev["p"] == 0, -1.0, 1.0) if pol else np.ones(len(ev))
    img = np.zeros((H, W), F64); S = np.zeros((H, W), F64); M = np.zeros((H, W), np.int64)
    lo, hi, lo_at, hi_at = 0.0, -1e6, None, None
    norm = 2.0 * np.pi * sigma * sigma
    for k in range(len(xy)):
        ex, ey = xy[k]
        if not (np.isfinite(ex) and np.isfinite(ey)):
            continue
        fx, fy = int(np.floor(ex)), int(np.floor(ey))
        if wrong == "swap":
            ex, ey = fx + (ey - fy), fy + (ex - fx)
        x0, x1, y0, y1 = max(fx - h, 0), min(fx + h, W - 1), max(fy - h, 0), min(fy + h, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        dx = np.arange(x0, x1 + 1, dtype=F64) - ex
        dy = np.arange(y0, y1 + 1, dtype=F64) - ey
        term = np.exp(-(dy[:, None] ** 2 + dx[None, :] ** 2) / (2.0 * sigma * sigma)) / norm
        sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        img[sl] += sign[k] * term; S[sl] += term; M[sl] += 1
        patch = img[sl]
        j = np.unravel_index(np.argmax(patch), patch.shape)
        if patch[j] > hi:
            hi, hi_at = float(patch[j]), (y0 + j[0], x0 + j[1])
        j = np.unravel_index(np.argmin(patch), patch.shape)
        if patch[j] < lo:
            lo, lo_at = float(patch[j]), (y0 + j[0], x0 + j[1])
    return dict(img=img, S=S, M=M, min=lo, max=hi, min_at=lo_at, max_at=hi_at, h=h, sigma=float(sigma))


def gauss_bound(ref):
    """Per-pixel bound of |float32 accumulation - plain|: (M + C) 2^-24 S with C = 8 + 4 (h + 1)^2 / sigma^2.

    Derivation.  A pixel's float32 value is a chain of M additions of terms t_k.  (a) Every addition rounds a partial sum whose
    magnitude is at most S, the sum of the |t_k|: M roundings of at most 2^-24 S each.  (b) One term is
    exp(-d) / (2 pi sigma^2) with d = (dx^2 + dy^2) / (2 sigma^2): the roundings of 2 pi, sigma^2, their product, the quotient,
    the exponential itself (under one ulp = two half-ulps), the negation-free product with the sign and the conversion of the
    pixel offset make at most 8 relative errors of 2^-24.  (c) d is computed with four roundings (two squares, their sum, the
    quotient by 2 sigma^2 whose sigma^2 is itself rounded) and e^-d turns a relative error r of d into the relative error r d of the
    term; |dx|, |dy| <= h + 1, so d <= (h + 1)^2 / sigma^2 and that part is at most 4 (h + 1)^2 / sigma^2 units of 2^-24.  Terms of
    second order are dropped; summed over a pixel's terms, (b) and (c) give C 2^-24 S."""
    h, sigma = ref["h"], ref["sigma"]
    C = 8.0 + 4.0 * (h + 1) ** 2 / sigma ** 2
    return (ref["M"] + C) * U * ref["S"]


def stamp_slope(sigma):
    """G = e^(-1/2) / (2 pi sigma^3): the steepest slope of one stamp (at distance sigma from its centre)."""
    sigma = F64(np.float32(sigma))
    return np.exp(-0.5) / (2.0 * np.pi * sigma ** 3)


def minmax_u8(img, wrong=None):
    """rint((v - min) 255 / (max - min)); 0 everywhere for a flat image.  wrong: "range" divides by max alone."""
    img = np.asarray(img, F64)
    lo, hi = img.min(), img.max()
    if hi <= lo:
        return np.zeros(img.shape, F64)
    return np.rint((img - lo) * 255.0 / (hi if wrong == "range" else hi - lo))


def scale_u8(img, lo, hi):
    """The event image's grey levels from its running extremes: (v - lo) 255 / (hi - lo), not rounded, clipped to [0, 255]."""
    return np.clip((np.asarray(img, F64) - lo) * 255.0 / (hi - lo), 0.0, 255.0)


def focus(img, wrong=None):
    """The image in tiles of 30 x 30 pixels from its top-left corner (the last ones cut by the image): the mean over the tiles of
    the population standard deviation sqrt(mean(v^2) - mean(v)^2) of a tile's pixels.
    wrong: "sample" divides by N - 1."""
    img = np.asarray(img, F64)
    H, W = img.shape
    out = []
    for y in range(0, H, 30):
        for x in range(0, W, 30):
            t = img[y:y + 30, x:x + 30]
            out.append(np.std(t, ddof=1 if (wrong == "sample" and t.size > 1) else 0))
    return float(np.mean(out))


# ---------------------------------------------------------------------------------------------------
# cameras: cam = (fx, fy, cx, cy) pinhole, (fx, fy, cx, cy, k1, k2, k3, k4) KannalaBrandt8
def _kb8_r(theta, k):
    t2 = theta * theta
    return theta * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))


def unproject(cam, x, y):
    """Pinhole: ((x - cx) / fx, (y - cy) / fy, 1).  KannalaBrandt8: with m = that point's (X, Y) and theta_d = |m| (at most pi / 2),
    theta solves theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) = theta_d (Newton's iteration from theta_d until it
    stops moving in float64), and the ray is (m tan(theta) / theta_d, 1)."""
    cam = np.asarray(cam, F64)
    X = (np.asarray(x, F64) - cam[2]) / cam[0]; Y = (np.asarray(y, F64) - cam[3]) / cam[1]
    if len(cam) > 4:
        k = cam[4:8]
        td = np.minimum(np.hypot(X, Y), np.pi / 2)
        th = td.copy()
        for _ in range(100):
            t2 = th * th
            d = 1.0 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])))
            step = (_kb8_r(th, k) - td) / d
            th = th - step
            if np.all(np.abs(step) <= 4e-16 * np.maximum(np.abs(th), 1e-300)):
                break
        scale = np.where(td > 1e-8, np.tan(th) / np.where(td > 1e-8, td, 1.0), 1.0)
        X, Y = X * scale, Y * scale
    return np.stack([X, Y, np.ones_like(X)], axis=-1)


def project(cam, P):
    """Pinhole: (fx X / Z + cx, fy Y / Z + cy).  KannalaBrandt8: theta = atan2(|(X, Y)|, Z), psi = atan2(Y, X),
    r = theta + k1 theta^3 + k2 theta^5 + k3 theta^7 + k4 theta^9, (fx r cos psi + cx, fy r sin psi + cy)."""
    cam = np.asarray(cam, F64); P = np.asarray(P, F64)
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    if len(cam) > 4:
        theta = np.arctan2(np.hypot(X, Y), Z); psi = np.arctan2(Y, X)
        r = _kb8_r(theta, cam[4:8])
        return np.stack([cam[0] * r * np.cos(psi) + cam[2], cam[1] * r * np.sin(psi) + cam[3]], axis=-1)
    return np.stack([cam[0] * X / Z + cam[2], cam[1] * Y / Z + cam[3]], axis=-1)


def _rate(ts, wrong=None):
    ts = np.asarray(ts, F64)
    if wrong == "rate":
        return (ts - ts[0]) / (ts[-1] - ts[0])
    return (ts[-1] - ts) / (ts[-1] - ts[0])


def warp_se3(ev, cam, angle, axis, t, depth, wrong=None):
    """Event k seen from the pose of the last event: rate = (t_last - t_k) / (t_last - t_first), R = the rotation by
    angle rate about the unit `axis` (Rodrigues: cos a I + sin a [axis]x + (1 - cos a) axis axis^T), P = unproject(x_k, y_k),
    uv = project(d R P + t rate), d = `depth` (one median depth, or one depth per event).  Returns (n, 2) float64.
    wrong: "rate" measures the rate from the first event, (t_k - t_first) / (t_last - t_first)."""
    return project(cam, warp_se3_points(ev, cam, angle, axis, t, depth, wrong))


def warp_se3_points(ev, cam, angle, axis, t, depth, wrong=None):
    """the 3-D points d R P + t rate that warp_se3 projects, (n, 3) float64"""
    rate = _rate(ev["ts"], wrong)
    a = np.asarray(axis, F64); t = np.asarray(t, F64)
    P = unproject(cam, ev["x"].astype(F64), ev["y"].astype(F64))
    ang = F64(angle) * rate
    c, s = np.cos(ang)[:, None], np.sin(ang)[:, None]
    RP = c * P + s * np.cross(a[None, :], P) + (1.0 - c) * (P @ a)[:, None] * a[None, :]
    d = np.broadcast_to(np.asarray(depth, F64), rate.shape)
    return d[:, None] * RP + t[None, :] * rate[:, None]


def warp_se2(ev, cam, params, wrong=None):
    """params = (omega, vx, vy[, scale]) over the whole window.  With rate as in warp_se3 and (X, Y, 1) = unproject(x_k, y_k):
    s_k = (1 - scale) (1 - rate) + scale (1 when there is no fourth parameter), (X', Y') = s_k Rot(omega rate) (X, Y) +
    (vx, vy) rate, uv = project(X', Y', 1).  wrong: "rate" as in warp_se3."""
    rate = _rate(ev["ts"], wrong)
    p = np.asarray(params, F64)
    sc = p[3] if len(p) > 3 else 1.0
    P = unproject(cam, ev["x"].astype(F64), ev["y"].astype(F64))
    th = p[0] * rate
    s = (1.0 - sc) * (1.0 - rate) + sc
    X = s * (P[:, 0] * np.cos(th) - P[:, 1] * np.sin(th)) + p[1] * rate
    Y = s * (P[:, 0] * np.sin(th) + P[:, 1] * np.cos(th)) + p[2] * rate
    return project(cam, np.stack([X, Y, np.ones_like(X)], axis=-1))


# ---------------------------------------------------------------------------------------------------
# orientation and descriptor
HALF_PATCH = 15


def circle_umax(r=HALF_PATCH):
    """The half widths of the rows of the circular patch of radius r: rint(sqrt(r^2 - v^2)) for the rows up to the diagonal
    (v <= floor(r / sqrt 2 + 1)), and the rows beyond it such that the patch is its own mirror image in the diagonal:
    umax[v] = the last u with umax[u] >= v."""
    vmax = int(np.floor(r * np.sqrt(2.0) / 2 + 1))
    um = [int(np.rint(np.sqrt(F64(r * r - v * v)))) for v in range(vmax + 1)]
    for v in range(vmax + 1, r + 1):
        um.append(max(u for u in range(vmax + 1) if um[u] >= v))
    return um


def ic_angle(level, cx, cy, umax, wrong=None):
    """m10 = sum u I(cx + u, cy + v), m01 = sum v I(cx + u, cy + v) over |v| <= 15, |u| <= umax[|v|] in integers; the angle is
    degrees(atan2(m01, m10)) mod 360.  wrong: "umax" shortens the rows v = +-7 by one pixel at either end."""
    um = list(umax)
    if wrong == "umax":
        um[7] -= 1
    I = np.asarray(level).astype(np.int64)
    m10 = m01 = 0
    for v in range(-HALF_PATCH, HALF_PATCH + 1):
        d = um[abs(v)]
        u = np.arange(-d, d + 1, dtype=np.int64)
        row = I[cy + v, cx - d:cx + d + 1]
        m10 += int((u * row).sum()); m01 += v * int(row.sum())
    return float(np.degrees(np.arctan2(F64(m01), F64(m10))) % 360.0)


def load_pattern():
    """The 256 test pairs (x0, y0, x1, y1) of the rBRIEF pattern: the numbers of the data table oracle/orc_pattern.h."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "orc_pattern.h")
    body = open(path).read().split("{", 1)[1].split("}", 1)[0]
    v = np.array([int(s) for s in re.findall(r"-?\d+", body)], np.int64)
    assert v.size == 1024 and np.abs(v).max() <= 13
    return v.reshape(256, 4)


def rbrief(blur, cx, cy, angle_deg, pattern, wrong=None):
    """Every pattern point (px, py) turned by the keypoint's angle a: (px cos a - py sin a, px sin a + py cos a), each coordinate
    rounded to the nearest integer; bit i of the descriptor is I(first point of pair i) < I(second point), I read from the blurred
    level at (cx, cy) + the rounded point; bit i is bit i % 8 of byte i // 8.
    Returns (32 bytes, mask[256]): the mask marks the bits of which a turned coordinate lies within 1e-4 of a half-integer, where
    rounding in float32 and in float64 may legitimately part.  wrong: "angle" turns by -a."""
    a = np.radians(F64(angle_deg)) * (-1.0 if wrong == "angle" else 1.0)
    pts = np.asarray(pattern, F64).reshape(512, 2)
    rx = pts[:, 0] * np.cos(a) - pts[:, 1] * np.sin(a)
    ry = pts[:, 0] * np.sin(a) + pts[:, 1] * np.cos(a)
    near = lambda c: np.abs(np.abs(c - np.floor(c)) - 0.5) < 1e-4
    mask = (near(rx) | near(ry)).reshape(256, 2).any(axis=1)
    I = np.asarray(blur)
    t = I[cy + np.rint(ry).astype(np.int64), cx + np.rint(rx).astype(np.int64)].astype(np.int64).reshape(256, 2)
    bits = (t[:, 0] < t[:, 1]).astype(np.uint8)
    return np.packbits(bits, bitorder="little"), mask


# ---------------------------------------------------------------------------------------------------
# pyramidal Lucas-Kanade (Bouguet)
def _pyr_down(img):
    """[1 4 6 4 1]^2 / 256 over a reflected (101) border, every second pixel in both axes: ((w + 1) // 2, (h + 1) // 2), not rounded."""
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    h, w = img.shape
    p = np.pad(img, 2, mode="reflect")
    rows = sum(k[i] * p[:, i:i + w] for i in range(5))
    full = sum(k[i] * rows[i:i + h, :] for i in range(5))
    return full[::2, ::2]


def _scharr(img, wrong=None):
    """The Scharr derivatives / 32: d/dx = ([3 10 3]^T / 16 down the columns) x ([-1 0 1] / 2 along the rows), d/dy its transpose.
    wrong: "scharr" puts the weights 1, 2, 1 in the place of 3, 10, 3 (still / 32: a Sobel derivative a quarter as large)."""
    a, b = (1.0, 2.0) if wrong == "scharr" else (3.0, 10.0)
    n = 32.0
    p = np.pad(img, 1, mode="reflect")
    h, w = img.shape
    c = lambda dy, dx: p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    gx = (a * (c(-1, 1) - c(-1, -1)) + b * (c(0, 1) - c(0, -1)) + a * (c(1, 1) - c(1, -1))) / n
    gy = (a * (c(1, -1) - c(-1, -1)) + b * (c(1, 0) - c(-1, 0)) + a * (c(1, 1) - c(-1, 1))) / n
    return gx, gy


def _bilinear(p, pad, x, y):
    """Bilinear samples of the padded image p at the (unpadded) positions x, y."""
    x = x + pad; y = y + pad
    x0 = np.floor(x).astype(np.int64); y0 = np.floor(y).astype(np.int64)
    a = x - x0; b = y - y0
    return ((1 - a) * (1 - b) * p[y0, x0] + a * (1 - b) * p[y0, x0 + 1] + (1 - a) * b * p[y0 + 1, x0] + a * b * p[y0 + 1, x0 + 1])


def lk(I, J, pts, win, maxLevel, maxCount, eps, minEig=1e-4, wrong=None):
    """Bouguet's pyramidal Lucas-Kanade tracker in float64.  Pyramids of I and J by _pyr_down, as many levels as maxLevel allows
    while a level stays larger than the window.  From the coarsest level down, for a point p (its position / 2^level) and its
    guess g (p on the coarsest level, twice the finer result below): the win x win window of I and of its Scharr / 32 derivatives
    (Ix, Iy), sampled bilinearly at p - (win - 1) / 2 + (i, j); A = sum [Ix^2, Ix Iy; Ix Iy, Iy^2]; then up to maxCount times:
    b = sum (J(window at g) - I(window at p)) (Ix, Iy), delta = -A^-1 b, g += delta; stop when |delta|^2 <= eps^2, or when from the
    second iteration on |delta + previous delta| < 0.01 in both axes (an oscillation: g steps half of delta back).
    A point loses its status when the window's corner leaves the image padded by `win`, or when the smaller eigenvalue of A
    (in OpenCV's scale: A / 1024, divided by win^2) is below minEig on level 0.  Outside an image the reflected (101) border is read,
    outside a derivative image zeros.  Returns (next points (n, 2) float64, status (n,) uint8).
    wrong: "scharr" as in _scharr."""
    pts = np.asarray(pts, F64).reshape(-1, 2)
    PI, PJ = [np.asarray(I, F64)], [np.asarray(J, F64)]
    for _ in range(maxLevel):
        h, w = PI[-1].shape
        if (w + 1) // 2 <= win or (h + 1) // 2 <= win:
            break
        PI.append(_pyr_down(PI[-1])); PJ.append(_pyr_down(PJ[-1]))
    pad = win + 2
    half = (win - 1) * 0.5
    gi, gj = np.meshgrid(np.arange(win, dtype=F64), np.arange(win, dtype=F64))
    out = pts.copy(); status = np.ones(len(pts), np.uint8)
    g = None
    for level in range(len(PI) - 1, -1, -1):
        Il, Jl = PI[level], PJ[level]
        h, w = Il.shape
        gx, gy = _scharr(Il, wrong)
        pIl = np.pad(Il, pad, mode="reflect"); pJl = np.pad(Jl, pad, mode="reflect")
        pgx = np.pad(gx, pad); pgy = np.pad(gy, pad)
        p_all = pts / float(1 << level)
        g = p_all.copy() if g is None else g * 2.0
        inside = lambda q: (-win <= np.floor(q[0] - half) < w) and (-win <= np.floor(q[1] - half) < h)
        for n in range(len(pts)):
            p = p_all[n]
            if not inside(p):
                if level == 0:
                    status[n] = 0
                continue
            wx, wy = p[0] - half + gi, p[1] - half + gj
            Iw = _bilinear(pIl, pad, wx, wy); Ix = _bilinear(pgx, pad, wx, wy); Iy = _bilinear(pgy, pad, wx, wy)
            A11, A12, A22 = (Ix * Ix).sum(), (Ix * Iy).sum(), (Iy * Iy).sum()
            det = A11 * A22 - A12 * A12
            lam = (A11 + A22 - np.sqrt((A11 - A22) ** 2 + 4 * A12 * A12)) / 2.0 / 1024.0 / (win * win)
            if lam < minEig or det / 1024.0 ** 2 < 2.0 ** -23:
                if level == 0:
                    status[n] = 0
                continue
            prev = None
            for j in range(maxCount):
                if not inside(g[n]):
                    if level == 0:
                        status[n] = 0
                    break
                Jw = _bilinear(pJl, pad, g[n, 0] - half + gi, g[n, 1] - half + gj)
                d = Jw - Iw
                b1, b2 = (d * Ix).sum(), (d * Iy).sum()
                delta = np.array([(A12 * b2 - A22 * b1) / det, (A12 * b1 - A11 * b2) / det])
                g[n] = g[n] + delta
                if delta @ delta <= eps * eps:
                    break
                if j > 0 and abs(delta[0] + prev[0]) < 0.01 and abs(delta[1] + prev[1]) < 0.01:
                    g[n] = g[n] - 0.5 * delta
                    break
                prev = delta
    return g, status
