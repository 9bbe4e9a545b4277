"""Seeded synthetic stand-ins for the reference's datasets.

Real EvETHZ / MVSEC recordings are not available offline; these generators reproduce their SHAPES:
240x180 DAVIS event slices (integer raw pixels, optionally LUT-undistorted with the EvETHZ
intrinsics of Examples/Event/EvETHZ.yaml:62-70, as the reference's loader does at
src/Event/EventLoader.cpp:111-125 / src/Utils/MyCalibrator.cpp:164-179), textured grey frames, 256-bit descriptor sets,
two-camera (fisheye) frame inputs and KannalaBrandt8 keyframe pairs.  Pure numpy, deterministic per seed.
"""
import numpy as np

# layout of one event at the drop-in boundary: include/Event/EventData.h:36-58 (24 B, AoS)
EVENT_DTYPE = np.dtype([("ts", "<f8"), ("x", "<f4"), ("y", "<f4"), ("p", "u1"), ("pad", "u1", (7,))])
# eorb_raw_event (16 B): sensor pixel, polarity, timestamp
RAW_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("p", "<u4"), ("t", "<f8")])
# cv::KeyPoint layout (28 B)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

EVETHZ_K = dict(fx=199.092366542, fy=198.82882047, cx=132.192071378, cy=110.712660011,
                k1=-0.368436311798, k2=0.150947243557, p1=-0.000296130534385, p2=-0.000759431726241)


def undistort_lut(W=240, H=180, K=EVETHZ_K, iters=8):
    """Per-raw-pixel undistorted position (radtan model inverted by fixed-point iteration, then
    re-projected with the same K: what cv::undistortPoints(src, K, D, R=I, P=K) yields)."""
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x0 = (u - K["cx"]) / K["fx"]; y0 = (v - K["cy"]) / K["fy"]
    x, y = x0.copy(), y0.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        icd = 1.0 / (1.0 + (K["k2"] * r2 + K["k1"]) * r2)
        dx = 2 * K["p1"] * x * y + K["p2"] * (r2 + 2 * x * x)
        dy = K["p1"] * (r2 + 2 * y * y) + 2 * K["p2"] * x * y
        x = (x0 - dx) * icd; y = (y0 - dy) * icd
    return (x * K["fx"] + K["cx"]).astype(np.float32), (y * K["fy"] + K["cy"]).astype(np.float32)


def shapes_events(n, W=240, H=180, seed=1, undistort=False, n_poly=3, noise_frac=0.05, t0=0.0, dt=1e-6,
                  motion=1.0, return_raw=False):
    """`n` events from the edges of `n_poly` moving quadrilaterals (K = 4*n_poly = 12 edges by
    default) plus uniform noise.  Raw coordinates are integer pixels; with undistort=True they are
    mapped through the EvETHZ LUT and events leaving the image are dropped and re-drawn, like the
    loader's checkInImage (src/Event/EventLoader.cpp:295-296).  Returns EVENT_DTYPE[n]."""
    rng = np.random.default_rng(seed)
    lut = undistort_lut(W, H) if undistort else None
    out = np.zeros(n, EVENT_DTYPE)
    rawx = np.zeros(n, np.uint16); rawy = np.zeros(n, np.uint16)
    filled = 0
    # polygon vertices at slice start and their displacement over the slice
    ctr = rng.uniform([0.25 * W, 0.25 * H], [0.75 * W, 0.75 * H], size=(n_poly, 1, 2))
    rad = rng.uniform(0.12 * H, 0.33 * H, size=(n_poly, 4, 1))
    ang = np.sort(rng.uniform(0, 2 * np.pi, size=(n_poly, 4)), axis=1)[..., None]
    v0 = ctr + rad * np.concatenate([np.cos(ang), np.sin(ang)], axis=2)
    vel = rng.uniform(-6.0, 6.0, size=(n_poly, 1, 2)) * motion
    while filled < n:
        m = int((n - filled) * 1.15) + 64
        tt = rng.uniform(0, 1, m)
        poly = rng.integers(0, n_poly, m); edge = rng.integers(0, 4, m); s = rng.uniform(0, 1, m)
        a = v0[poly, edge] + vel[poly, 0] * tt[:, None]
        b = v0[poly, (edge + 1) % 4] + vel[poly, 0] * tt[:, None]
        pt = a + (b - a) * s[:, None] + rng.normal(0, 0.6, size=(m, 2))
        noise = rng.uniform(0, 1, m) < noise_frac
        pt[noise] = rng.uniform([0, 0], [W, H], size=(int(noise.sum()), 2))
        xi = np.floor(pt[:, 0]).astype(np.int64); yi = np.floor(pt[:, 1]).astype(np.int64)
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        xi, yi, tt = xi[ok], yi[ok], tt[ok]
        if lut is not None:
            xf = lut[0][yi, xi]; yf = lut[1][yi, xi]
            ok = (xf >= 0) & (xf < W) & (yf >= 0) & (yf < H)       # MyCalibrator::isInImage on floats
            xf, yf, tt, xi, yi = xf[ok], yf[ok], tt[ok], xi[ok], yi[ok]
        else:
            xf = xi.astype(np.float32); yf = yi.astype(np.float32)
        k = min(len(xf), n - filled)
        out["x"][filled:filled + k] = xf[:k]; out["y"][filled:filled + k] = yf[:k]
        out["ts"][filled:filled + k] = tt[:k]
        rawx[filled:filled + k] = xi[:k]; rawy[filled:filled + k] = yi[:k]
        filled += k
    order = np.argsort(out["ts"], kind="stable")
    out = out[order]
    out["ts"] = t0 + np.arange(n) * dt                      # monotone, us resolution
    out["p"] = rng.integers(0, 2, n).astype(np.uint8)
    if not return_raw:
        return out
    raw = np.zeros(n, RAW_DTYPE)
    raw["x"] = rawx[order]; raw["y"] = rawy[order]; raw["p"] = out["p"]; raw["t"] = out["ts"]
    return out, raw


def random_raw_events(n, W=240, H=180, seed=0):
    """Uniform sensor-pixel events (eorb_raw_event records)."""
    rng = np.random.default_rng(seed)
    raw = np.zeros(n, RAW_DTYPE)
    raw["x"] = rng.integers(0, W, n); raw["y"] = rng.integers(0, H, n)
    raw["p"] = rng.integers(0, 2, n); raw["t"] = 1e6 + np.arange(n) * 3.0
    return raw


def random_events(n, W=240, H=180, seed=0, frac=True, margin=4.0):
    """Uniform float events, including positions slightly outside the image (stamp clipping)."""
    rng = np.random.default_rng(seed)
    ev = np.zeros(n, EVENT_DTYPE)
    x = rng.uniform(-margin, W + margin, n); y = rng.uniform(-margin, H + margin, n)
    if not frac:
        x = np.floor(x); y = np.floor(y)
    ev["x"] = x.astype(np.float32); ev["y"] = y.astype(np.float32)
    ev["ts"] = np.arange(n) * 1e-6
    ev["p"] = rng.integers(0, 2, n).astype(np.uint8)
    return ev


def texture_image(W=240, H=180, seed=3, octaves=4):
    """Band-limited noise + a few hard-edged rectangles: gives FAST corners on every level."""
    rng = np.random.default_rng(seed)
    img = np.zeros((H, W), np.float64)
    for o in range(octaves):
        gh, gw = max(2, H >> (o + 2)), max(2, W >> (o + 2))
        g = rng.uniform(0, 1, (gh, gw))
        yy = np.linspace(0, gh - 1, H); xx = np.linspace(0, gw - 1, W)
        y0 = np.floor(yy).astype(int); x0 = np.floor(xx).astype(int)
        y1 = np.minimum(y0 + 1, gh - 1); x1 = np.minimum(x0 + 1, gw - 1)
        fy = (yy - y0)[:, None]; fx = (xx - x0)[None, :]
        up = (g[y0][:, x0] * (1 - fy) * (1 - fx) + g[y0][:, x1] * (1 - fy) * fx +
              g[y1][:, x0] * fy * (1 - fx) + g[y1][:, x1] * fy * fx)
        img += up * (0.5 ** (octaves - 1 - o))
    img = (img - img.min()) / (img.max() - img.min())
    for _ in range(40):
        w, h = rng.integers(6, 40), rng.integers(6, 40)
        x, y = rng.integers(0, W - 6), rng.integers(0, H - 6)
        img[y:y + h, x:x + w] = np.clip(img[y:y + h, x:x + w] + rng.uniform(-0.5, 0.5), 0, 1)
    return np.round(img * 255).astype(np.uint8)


def random_descriptors(n, seed=4, width=32):
    return np.random.default_rng(seed).integers(0, 256, (n, width), dtype=np.uint8)


def planted_descriptors(train, seed=5, max_flips=40):
    """Each query = a (permuted) train row with k ~ U[0, max_flips] flipped bits (first 32 B)."""
    rng = np.random.default_rng(seed)
    n = len(train)
    perm = rng.permutation(n)
    q = train[perm].copy()
    for i in range(n):
        k = rng.integers(0, max_flips + 1)
        bits = rng.choice(256, size=k, replace=False)
        for b in bits:
            q[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return q, perm


def random_keypoints(n, W=240, H=180, nlevels=4, scale=1.2, seed=6):
    """Keypoints shaped like extractor output (level-coordinates scaled to the image)."""
    rng = np.random.default_rng(seed)
    kp = np.zeros(n, KP_DTYPE)
    kp["x"] = rng.uniform(10, W - 10, n).astype(np.float32)
    kp["y"] = rng.uniform(10, H - 10, n).astype(np.float32)
    kp["octave"] = rng.integers(0, nlevels, n)
    kp["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    kp["size"] = (31 * scale ** kp["octave"]).astype(np.int32).astype(np.float32)
    kp["response"] = rng.integers(1, 120, n).astype(np.float32)
    kp["class_id"] = -1
    return kp


def random_vocabulary(k=10, L=3, seed=0, ragged=False, stop_frac=0.02):
    """A DBoW2-shaped vocabulary tree with random 256-bit node descriptors: k children per node and L levels (ragged=True:
    2..k children and some branches ending early).  Children of a node are near copies of their parent, so descents are
    meaningful.  Returns dict(L, child_off, child_ids, node_desc, word_id, weight) with node 0 = root."""
    rng = np.random.default_rng(seed)
    desc = [rng.integers(0, 256, 32, dtype=np.uint8)]
    children = [[]]
    level = [0]
    frontier = [0]
    for lv in range(1, L + 1):
        nxt = []
        for u in frontier:
            if ragged and lv > 1 and rng.uniform() < 0.15:
                continue                                                # this branch ends early: u stays a word
            nc = int(rng.integers(2, k + 1)) if ragged else k
            for _ in range(nc):
                flip = rng.uniform(size=256) < (0.25 / lv)
                d = desc[u] ^ np.packbits(flip)
                desc.append(d); children.append([]); level.append(lv)
                children[u].append(len(desc) - 1); nxt.append(len(desc) - 1)
        frontier = nxt
    n = len(desc)
    # DBoW2 stores children in creation order but node ids need not be contiguous per parent: shuffle ids (root stays 0)
    perm = np.concatenate([[0], 1 + rng.permutation(n - 1)])
    inv = np.empty(n, np.int64); inv[perm] = np.arange(n)
    child_off = [0]; child_ids = []
    for new in range(n):
        old = perm[new]
        child_ids.extend(int(inv[c]) for c in children[old]); child_off.append(len(child_ids))
    node_desc = np.stack([desc[perm[i]] for i in range(n)])
    is_leaf = np.array([len(children[perm[i]]) == 0 for i in range(n)])
    word_id = np.full(n, -1, np.int32); word_id[is_leaf] = rng.permutation(int(is_leaf.sum())).astype(np.int32)
    weight = np.zeros(n, np.float64); weight[is_leaf] = rng.uniform(0.5, 9.0, int(is_leaf.sum()))
    stop = is_leaf & (rng.uniform(size=n) < stop_frac)
    weight[stop] = 0.0                                                  # stopWords()
    return dict(L=L, child_off=np.array(child_off, np.int32), child_ids=np.array(child_ids, np.int32), node_desc=node_desc,
                word_id=word_id, weight=weight)


# ---- config 1 as the reference executes it (EvImBuilder::Track): a stream with enough motion for the window-size rule to fire, and
# stand-ins for what the optimisers hand the motion-compensated reconstructions (they are outside the front end) ----
EVETHZ_PINHOLE = (EVETHZ_K["fx"], EVETHZ_K["fy"], EVETHZ_K["cx"], EVETHZ_K["cy"])       # rectified events: a calibrated pinhole camera


def l1_stream(n_chunks=60, chunk=2000, seed=5, motion=14.0, W=240, H=180):
    """One long time-ordered slice of the shapes generator (float EventData, monotone time stamps 1 us apart)."""
    return shapes_events(n_chunks * chunk, W, H, seed=seed, motion=motion, undistort=True)


def l1_mci_poses(window):
    """What resolveLastDPose / resolveLastPoseMap / resolveLastAtt2Params would hand generateMCImage (src/Event/EvImBuilder.cpp:958-1143):
    fixed small motions scaled by the window's length.  Deterministic in the window."""
    n = len(window)
    s = min(n / 6000.0, 2.0)
    return dict(dp=dict(angle=0.010 * s, axis=(0.1, -0.2, 0.97), t=(0.004 * s, -0.003 * s, 0.001), medDepth=1.0),
                ba=dict(angle=0.016 * s, axis=(-0.3, 0.1, 0.95), t=(-0.002 * s, 0.005 * s, 0.0), medDepth=1.3),
                se2=np.array([0.012 * s, 1.5 * s, -0.8 * s], np.float32))


def stereo_pair(seed, W=346, H=260, dmax=14):
    """A rectified stereo pair: the right image is the left one warped by a smooth disparity field in [2, dmax] pixels -- d(x, y) = 2 +
    (dmax - 2) (0.5 + 0.5 sin(y / 37 + x / 91)), bilinear in x, nothing vertical -- plus a little independent noise.  Returns (left, right) u8."""
    rng = np.random.default_rng(seed)
    left = texture_image(W + 32, H, seed=seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    disp = 2.0 + (dmax - 2.0) * (0.5 + 0.5 * np.sin(yy / 37.0 + xx / 91.0))
    xs = xx + disp                                                         # right(x) = left(x + d)
    x0 = np.floor(xs).astype(np.int64); fr = xs - x0
    rows = yy.astype(np.int64)
    right = (1 - fr) * left[rows, x0] + fr * left[rows, np.minimum(x0 + 1, W + 31)]
    right = np.clip(np.rint(right + rng.normal(0, 1.0, right.shape)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(left[:, :W]), right


def feature_vector_of(node_of, rng):
    """DBoW2::FeatureVector as CSR from a node id per feature: (node ids ascending, offsets, feature indices; inside a node the
    insertion order shuffled)"""
    ids = np.unique(node_of)
    off = [0]; idx = []
    for nid in ids:
        m = np.nonzero(node_of == nid)[0]; rng.shuffle(m); idx.extend(m.tolist()); off.append(len(idx))
    return ids.astype(np.uint32), np.array(off, np.int32), np.array(idx, np.int32)


def flip_bits(d, nbits, rng):
    """a copy of descriptor d with nbits of its first 256 bits flipped"""
    d = d.copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


# ---- two-camera (fisheye stereo) frames: TUM-VI sized ----
def image_pair(W=512, H=512, seed=5, shift=(2, -7)):
    """a textured image and the same scene shifted: a stand-in for a fisheye stereo pair (TUM-VI 512 x 512)"""
    img = texture_image(W, H, seed=seed)
    return img, np.roll(img, shift, axis=(0, 1))


def map_inputs(kps, nL, scale_factors, rng, M=None, src=None):
    """map points near a two-camera frame's keypoints: (left, right, mp_desc, mp_obs), left / right = (in_view, proj_xy, level,
    view_cos, level_scale) per map point; src = (kps, desc) the map points are drawn from"""
    sk, sd = src
    M = len(sk) if M is None else M
    pick = rng.integers(0, len(sk), M)
    k = sk[pick]
    nl = len(scale_factors)
    cams = []
    for cam in range(2):
        iv = (rng.uniform(size=M) < (0.9 if cam == 0 else 0.7)).astype(np.uint8)
        pxy = np.stack([k["x"] + rng.normal(0, 1.0, M), k["y"] + rng.normal(0, 1.0, M)], axis=1).astype(np.float32)
        if cam:
            pxy[:, 0] += rng.normal(-6.0, 1.0, M)
        lv = np.clip(k["octave"] + rng.integers(-1, 2, M), 0, nl - 1).astype(np.int32)
        if cam:
            lv[rng.uniform(size=M) < 0.1] = -1
        vc = rng.uniform(0.99, 1.0, M).astype(np.float32)
        ls = np.asarray(scale_factors, np.float32)[np.clip(lv, 0, nl - 1)]
        cams.append((iv, pxy, lv, vc, ls))
    mp_obs = (rng.uniform(size=M) < 0.6).astype(np.uint8)
    return cams[0], cams[1], sd[pick].copy(), mp_obs


# ---- keyframe pairs for SearchForTriangulation with KannalaBrandt8 cameras ----
# KB8 parameters chosen for the tests (a 346 x 260 event camera and a 512 x 512 fisheye pair), not taken from any configuration
CAM_MONO = (226.0, 226.5, 172.0, 131.0, -0.02, 0.004, -0.001, 0.0002)
CAM_L = (190.5, 190.2, 254.9, 256.8, 0.0034, 0.0007, -0.0021, 0.0003)
CAM_R = (190.1, 189.9, 256.2, 255.1, 0.0030, 0.0011, -0.0018, 0.0002)
NLEV, SCALE = 8, 1.2


def level_tables(nlev=NLEV, sf=SCALE):
    """mvScaleFactor and mvLevelSigma2 in float"""
    s = [np.float32(1.0)]
    for _ in range(1, nlev):
        s.append(np.float32(s[-1] * np.float32(sf)))
    s = np.array(s, np.float32)
    return s, (s * s).astype(np.float32)


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float32)


def rel_pose(Ra, ta, Rb, tb):
    """R12, t12 of camera a (1) w.r.t. camera b (2): R1w R2w^T, -R1w R2w^T t2w + t1w (float rows, computed in float64 then rounded)"""
    R = (Ra.astype(np.float64) @ Rb.T.astype(np.float64)).astype(np.float32)
    t = (-(R.astype(np.float64) @ tb.astype(np.float64)) + ta).astype(np.float32)
    return np.concatenate([R.reshape(9), t]).astype(np.float32)


def project_np(c, P):
    """KB8 / Pinhole projection in float64 (test-data generation only; the oracle's float path decides every outcome)"""
    P = np.asarray(P, np.float64)
    if len(c) == 4:
        return np.stack([c[0] * P[:, 0] / P[:, 2] + c[2], c[1] * P[:, 1] / P[:, 2] + c[3]], axis=1)
    th = np.arctan2(np.hypot(P[:, 0], P[:, 1]), P[:, 2]); psi = np.arctan2(P[:, 1], P[:, 0])
    r = th + c[4] * th ** 3 + c[5] * th ** 5 + c[6] * th ** 7 + c[7] * th ** 9
    return np.stack([c[0] * r * np.cos(psi) + c[2], c[1] * r * np.sin(psi) + c[3]], axis=1)


def _scene(rng, npts, nnodes):
    """3D points in front of the first camera with a descriptor, a vocabulary node and an orientation each"""
    z = rng.uniform(1.5, 9.0, npts)
    X = np.stack([rng.uniform(-1.1, 1.1, npts) * z, rng.uniform(-0.9, 0.9, npts) * z, z], axis=1)
    base = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    node = rng.integers(0, nnodes, npts) * 7 + 3
    ang = rng.uniform(0, 360, npts)
    return X, base, node, ang


def _observe(rng, scene, poses, cams, W, H, ndistract, nties, stride, second, angle_offset=0.0):
    """One keyframe's view of a scene: per camera (poses[cidx] = (R, t), cams[cidx]) the visible points with near-duplicate
    descriptors and distractors, shuffled; then elig, nodes and the feature vector.  second: the keyframe searched in (pKF2) -- nties
    exact-descriptor ties and noise on the orientations.  Two cameras: bit 1 of elig stays clear."""
    X, base, node, ang = scene
    npts, ncam, twocam = len(X), len(poses), len(poses) == 2
    blocks = []
    for cidx in range(ncam):
        R, t = poses[cidx]
        Pc = X @ R.T.astype(np.float64) + t
        uv = project_np(cams[cidx], Pc)
        vis = (Pc[:, 2] > 0.2) & (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)
        vis &= rng.uniform(size=npts) < 0.9
        pid = np.nonzero(vis)[0]
        rows = []
        for p in pid:
            rows.append((uv[p, 0] + rng.normal(0, 0.4), uv[p, 1] + rng.normal(0, 0.4), p, flip_bits(base[p], rng.integers(0, 11), rng)))
        for _ in range(ndistract // ncam):
            p = rng.integers(npts)
            rows.append((rng.uniform(0, W), rng.uniform(0, H), p, flip_bits(base[p], rng.integers(12, 31), rng)))
        if second:
            for j in rng.choice(len(pid), min(nties // ncam, len(pid)), replace=False):
                x, y, p, d = rows[j]
                rows.append((x + rng.uniform(-1.5, 1.5), y + rng.uniform(-1.5, 1.5), p, d.copy()))
        order = rng.permutation(len(rows))
        blocks.append([rows[i] for i in order])
    allrows = [r for b in blocks for r in b]
    n = len(allrows)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = np.array([r[0] for r in allrows], np.float32); kps["y"] = np.array([r[1] for r in allrows], np.float32)
    kps["octave"] = rng.integers(0, 4, n); kps["size"] = 31.0; kps["class_id"] = -1
    pids = np.array([r[2] for r in allrows], np.int64)
    a = ang[pids] + (rng.normal(0, 4, n) if second else 0) + np.where(rng.uniform(size=n) < 0.1, rng.uniform(0, 360, n), 0)
    kps["angle"] = np.mod(a + angle_offset, 360).astype(np.float32)
    desc = np.zeros((n, stride), np.uint8)
    if n:
        desc[:, :32] = np.stack([r[3] for r in allrows])
    if stride > 32:
        desc[:, 32:] = rng.integers(0, 256, (n, stride - 32), dtype=np.uint8)
    elig = (rng.uniform(size=n) < 0.85).astype(np.uint8)
    if stride > 32:
        elig[rng.uniform(size=n) < 0.15] = 0                         # non-ORB rows of a Mixed keyframe
    if not twocam:
        elig |= ((rng.uniform(size=n) < 0.1) << 1).astype(np.uint8) & (elig << 1)
    nodes = node[pids].copy()
    nodes[rng.uniform(size=n) < 0.05] = 1                              # a node the other keyframe may lack
    fv = feature_vector_of(nodes, rng)
    return dict(kps=kps, nleft=len(blocks[0]) if twocam else -1, desc=desc, elig=elig, fv=fv)


def keyframe_pair(seed=0, twocam=False, npts=600, ndistract=150, nties=30, stride=32, nnodes=60, size=None, ep_near=True):
    """A keyframe pair seeing one 3D scene.  Returns a dict of the matcher's inputs (kps / nleft / desc / elig / fv per keyframe,
    cams, Rt, ep, scale2, sigma2).  True observations carry near-duplicate descriptors (<= 10 flipped bits); distractors copy a
    point's descriptor with 12-30 flipped bits at a random position (pass Hamming, fail geometry); ties copy an observation of
    pKF2 with its exact descriptor 0.2-1.5 px away.  stride 61: Mixed rows, ~15 % of them non-ORB (elig 0: the type gate)."""
    rng = np.random.default_rng(seed)
    scale, sigma2 = level_tables()
    if twocam:
        W = H = 512 if size is None else size
        cams = (CAM_L, CAM_R)
        Rrl, trl = rot(0.002, -0.01, 0.003), np.array([-0.11, 0.001, 0.002], np.float32)   # right camera w.r.t. left
    else:
        W, H = (346, 260) if size is None else size
        cams = (CAM_MONO,)
        Rrl, trl = None, None
    R1, t1 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    R2 = rot(0.03, -0.08, 0.02); t2 = np.array([-0.35, 0.04, 0.06], np.float32)
    poses = {(0, 0): (R1, t1), (1, 0): (R2, t2)}
    if twocam:
        poses[(0, 1)] = ((Rrl.astype(np.float64) @ R1).astype(np.float32), (Rrl.astype(np.float64) @ t1 + trl).astype(np.float32))
        poses[(1, 1)] = ((Rrl.astype(np.float64) @ R2).astype(np.float32), (Rrl.astype(np.float64) @ t2 + trl).astype(np.float32))
    scene = _scene(rng, npts, nnodes)
    kf = [_observe(rng, scene, [poses[(k, cidx)] for cidx in range(2 if twocam else 1)], cams, W, H, ndistract, nties, stride,
                   second=bool(k)) for k in range(2)]
    if twocam:
        Rt = np.concatenate([rel_pose(*poses[(0, a)], *poses[(1, b)]) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1))])
    else:
        Rt = rel_pose(R1, t1, R2, t2)
    k2 = kf[1]["kps"]
    ep = (k2["x"][0] + 4.0, k2["y"][0]) if ep_near else (-1000.0, -1000.0)
    camsp = cams if twocam else cams[0]
    return dict(kps1=kf[0]["kps"], nleft1=kf[0]["nleft"], desc1=kf[0]["desc"], elig1=kf[0]["elig"], fv1=kf[0]["fv"],
                kps2=kf[1]["kps"], nleft2=kf[1]["nleft"], desc2=kf[1]["desc"], elig2=kf[1]["elig"], fv2=kf[1]["fv"],
                cams1=camsp, cams2=camsp, Rt=Rt, ep=np.array(ep, np.float32), scale2=scale, sigma2_1=sigma2, sigma2_2=sigma2)


def cap_nodes(fv, caps, x):
    """fv with node a cut to its caps[a] leftmost features by x (None or missing: all), vector order kept; the rest appear in no node,
    which is legal input"""
    nodes, off, idx = fv
    keep = []
    for a in range(len(nodes)):
        m = idx[off[a]:off[a + 1]]
        cap = caps[a] if a < len(caps) else None
        keep.append(m if cap is None else m[np.sort(np.argsort(x[m], kind="stable")[:cap])])
    return nodes, np.cumsum([0] + [len(k) for k in keep]).astype(np.int32), np.concatenate(keep + [np.zeros(0, np.int32)]).astype(np.int32)


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


def neighbour_pose(k):
    """pose k of a neighbourhood: a few degrees of rotation and a baseline that differ for every k (five patterns, nudged every fifth
    keyframe), part of the baseline along the optical axis so that the epipole of a Pinhole pair lies in or near the image"""
    a, b = k % 5, k // 5
    R = rot(0.03 - 0.011 * a + 0.004 * b, -0.08 + 0.027 * a - 0.006 * b, 0.02 * (1 - a) + 0.003 * b)
    t = np.array([-0.35 + 0.16 * a + 0.03 * b, 0.04 - 0.03 * a + 0.01 * b, 0.06 + 0.09 * (a % 3) + 0.02 * b], np.float32)
    return R, t


def triangulation_neighbourhood(seed, K, twocam=False, pinhole=False, npts=250, ndistract=60, nties=12, stride=32, nnodes=10, size=None,
                                angle_step=50.0):
    """One current keyframe (pKF1) and K neighbours at different poses over one scene, built like keyframe_pair: the inputs of
    LocalMapping::CreateNewMapPoints' SearchForTriangulation loop.  Returns pKF1's arrays (kps1, nleft1, desc1, elig1, fv1), the list
    kfs of neighbours (dicts kps, nleft, desc, elig, fv), cams1 / cams2, the level tables and per neighbour Rt[k] (12 or 48 floats) and
    ep[k].  pinhole: both cameras are the Pinhole part of CAM_MONO, ep[k] = the true epipole project(R2w * Cw + t2w) and F12[k] =
    K1^-T [t12]x R12 K2^-1 in float.  Otherwise KannalaBrandt8 as in keyframe_pair, ep[k] near a keypoint of the neighbour.  The
    neighbours' orientations are offset by k * angle_step degrees, so every pair keeps other bins of the rotation histogram."""
    assert not (twocam and pinhole)
    rng = np.random.default_rng(seed)
    scale, sigma2 = level_tables()
    if twocam:
        W = H = 512 if size is None else size
        cams = (CAM_L, CAM_R)
        Rrl, trl = rot(0.002, -0.01, 0.003), np.array([-0.11, 0.001, 0.002], np.float32)
    else:
        W, H = (346, 260) if size is None else size
        cams = (CAM_MONO[:4],) if pinhole else (CAM_MONO,)

    def rig(R, t):
        if not twocam:
            return [(R, t)]
        return [(R, t), ((Rrl.astype(np.float64) @ R).astype(np.float32), (Rrl.astype(np.float64) @ t + trl).astype(np.float32))]

    R1, t1 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    scene = _scene(rng, npts, nnodes)
    kf1 = _observe(rng, scene, rig(R1, t1), cams, W, H, ndistract, nties, stride, second=False)
    kfs, Rts, eps, Fs = [], [], [], []
    for k in range(K):
        R2, t2 = neighbour_pose(k)
        kf = _observe(rng, scene, rig(R2, t2), cams, W, H, ndistract, nties, stride, second=True, angle_offset=angle_step * k)
        kfs.append(kf)
        if twocam:
            Rts.append(np.concatenate([rel_pose(*rig(R1, t1)[a], *rig(R2, t2)[b]) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1))]))
        else:
            Rts.append(rel_pose(R1, t1, R2, t2))
        if pinhole:
            fx, fy, cx, cy = cams[0]
            Kinv = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64))
            R12 = Rts[-1][:9].reshape(3, 3).astype(np.float64); t12 = Rts[-1][9:].astype(np.float64)
            Fs.append((Kinv.T @ _skew(t12) @ R12 @ Kinv).astype(np.float32))
            C2 = R2.astype(np.float64) @ (-(R1.T.astype(np.float64) @ t1)) + t2           # pKF1's centre in camera 2
            eps.append(project_np(cams[0], C2[None])[0].astype(np.float32))
        else:
            k2 = kf["kps"]
            eps.append(np.array((k2["x"][0] + 4.0, k2["y"][0]) if len(k2) else (-1000.0, -1000.0), np.float32))
    camsp = cams if twocam else cams[0]
    out = dict(kps1=kf1["kps"], nleft1=kf1["nleft"], desc1=kf1["desc"], elig1=kf1["elig"], fv1=kf1["fv"], kfs=kfs, cams1=camsp, cams2=camsp,
               Rt=np.stack(Rts).astype(np.float32) if K else np.zeros((0, 12), np.float32),
               ep=np.stack(eps).astype(np.float32) if K else np.zeros((0, 2), np.float32), scale2=scale, sigma2_1=sigma2, sigma2_2=sigma2)
    if pinhole:
        out["F12"] = np.stack(Fs) if K else np.zeros((0, 3, 3), np.float32)
    return out


def bow_neighbourhood(seed, K, npts=250, ndistract=60, nties=12, nnodes=10, caps=None, p_mp=0.8, angle_step=50.0):
    """One frame (or current keyframe) and K keyframes over one scene for the SearchByBoW loops of Tracking::Relocalization and
    LoopClosing::DetectCommonRegionsFromBoW: a point's observations share its vocabulary node, so matching features mostly share a
    node.  caps[k] (optional) = per-node caps of keyframe k's feature vector (cap_nodes by image x: a keyframe's nodes can sit on
    either side of a kernel's per-node limit).  Returns the frame's kps / desc / fv / has_mp and kfs (dicts kps, desc, fv, has_mp)."""
    s = triangulation_neighbourhood(seed, K, npts=npts, ndistract=ndistract, nties=nties, nnodes=nnodes, angle_step=angle_step)
    rng = np.random.default_rng(seed + 7919)
    kfs = []
    for k, kf in enumerate(s["kfs"]):
        fv = kf["fv"] if not caps or caps[k] is None else cap_nodes(kf["fv"], caps[k], kf["kps"]["x"])
        kfs.append(dict(kps=kf["kps"], desc=kf["desc"], fv=fv, has_mp=(rng.uniform(size=len(kf["kps"])) < p_mp).astype(np.uint8)))
    return dict(kps=s["kps1"], desc=s["desc1"], fv=s["fv1"], has_mp=(rng.uniform(size=len(s["kps1"])) < p_mp).astype(np.uint8), kfs=kfs)


# ---- camera calibrations (eorb_calib of include/eorb_fe.h): model 0 = Pinhole / cv::undistortPoints, 1 = KannalaBrandt8 /
# cv::fisheye::undistortPoints; K, dist as the reference reads them from its settings (CV_32F); R = None: cv::Mat(); P = None: cv::Mat()
def _K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def _calibration(model, K, dist, size, R=None, P="K"):
    return dict(model=model, K=K, dist=np.asarray(dist, np.float32), size=size, R=None if R is None else np.asarray(R, np.float32),
                P=(K.copy() if isinstance(P, str) else (None if P is None else np.asarray(P, np.float32))))


_K_ETHZ = _K(EVETHZ_K["fx"], EVETHZ_K["fy"], EVETHZ_K["cx"], EVETHZ_K["cy"])
_D_ETHZ = [EVETHZ_K["k1"], EVETHZ_K["k2"], EVETHZ_K["p1"], EVETHZ_K["p2"]]
_K_EUROC = _K(458.654, 457.296, 367.215, 248.375)
_K_MVSEC = _K(226.38018519795807, 226.15002947047415, 173.6470807871759, 133.73271487507847)

CALIBRATIONS = {
    # Examples/Event/EvETHZ.yaml:59-73 (PinHole, k1 k2 p1 p2, 240 x 180); the call sites pass R = cv::Mat(), P = mK (Frame.cc:248)
    "EvETHZ": _calibration(0, _K_ETHZ, _D_ETHZ, (240, 180)),
    # Examples/Event/EuRoC.yaml:58-87 (PinHole, 752 x 480)
    "EuRoC": _calibration(0, _K_EUROC, [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05], (752, 480)),
    # Examples/Event/EvMVSEC_ETHZ.yaml:54-89 (KannalaBrandt8, equidistant k1..k4, 346 x 260)
    "MVSEC_KB8": _calibration(1, _K_MVSEC, [-0.048031442223833355, 0.011330957517194437, -0.055378166304281135, 0.021500973881459395],
                              (346, 260)),
    # the five- and eight-coefficient forms of cv::undistortPoints (k3; k4 k5 k6 of the rational model)
    "pinhole5": _calibration(0, _K_ETHZ, _D_ETHZ + [0.021], (240, 180)),
    "pinhole8": _calibration(0, _K_EUROC, [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.011, 0.013, -0.006, 0.002], (752, 480)),
    # a rectifying rotation and a 3 x 4 projection that is not K (a stereo-rectified pair's R1 / P1 shape), both models
    "pinhole_RP": _calibration(0, _K_EUROC, [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05], (752, 480),
                               R=None, P=[[435.2, 0, 367.45, 0], [0, 435.2, 252.2, 0], [0, 0, 1, 0]]),
    "fisheye_RP": _calibration(1, _K_MVSEC, [-0.048031442223833355, 0.011330957517194437, -0.055378166304281135, 0.021500973881459395],
                               (346, 260), R=None, P=[[190.98, 0, 172.9, -12.5], [0, 190.97, 130.9, 0], [0, 0, 1, 0]]),
    # normalised coordinates out (P = cv::Mat()), and the closed gate: |k1| <= 1e-9 with the other coefficients large
    "pinhole_noP": _calibration(0, _K_ETHZ, _D_ETHZ, (240, 180), P=None),
    "gate_closed": _calibration(0, _K_ETHZ, [1e-10, 0.5, 0.1, -0.2], (240, 180)),
}


def _small_rotation(ax=0.011, ay=-0.007, az=0.004):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float32)


CALIBRATIONS["pinhole_RP"]["R"] = _small_rotation()
CALIBRATIONS["fisheye_RP"]["R"] = _small_rotation(-0.006, 0.009, -0.003)


def calib_keypoints(n, W, H, seed=0, margin=0.1, nlevels=4):
    """n seeded keypoints inside the image plus a margin (fraction of the size) around it: integer, half-pixel and arbitrary
    sub-pixel positions, every other field filled so that a copy can be told from a default."""
    rng = np.random.RandomState(seed)
    kps = np.zeros(n, KP_DTYPE)
    x = rng.uniform(-margin * W, (1 + margin) * W, n); y = rng.uniform(-margin * H, (1 + margin) * H, n)
    kind = rng.randint(0, 3, n)
    x = np.where(kind == 0, np.round(x), np.where(kind == 1, np.round(x * 2) / 2, x))
    y = np.where(kind == 0, np.round(y), np.where(kind == 1, np.round(y * 2) / 2, y))
    kps["x"] = x.astype(np.float32); kps["y"] = y.astype(np.float32)
    kps["octave"] = rng.randint(0, nlevels, n)
    kps["size"] = (31.0 * 1.2 ** kps["octave"]).astype(np.float32)
    kps["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    kps["response"] = rng.uniform(1, 200, n).astype(np.float32)
    kps["class_id"] = rng.randint(-1, 1000, n)
    return kps


# ---- map points around a posed camera (the projector: eorb_project_frustum and its kin) ----------------------------------------
def scale_tables(nlevels=8, scaleFactor=1.2):
    """mvScaleFactor as ORBextractor builds it (float products, src/ORBextractor.cc:430-437) and mfLogScaleFactor = log(float)"""
    sf = np.ones(nlevels, np.float32)
    for i in range(1, nlevels):
        sf[i] = sf[i - 1] * np.float32(scaleFactor)
    return sf, np.float32(np.log(np.float32(scaleFactor)))


def map_scene(seed, M, W=346, H=260, f=280.0, nlevels=8, scaleFactor=1.2, angle=0.3):
    """M seeded map points around a camera rotated by `angle` rad about a random axis, made so that every outcome of
    Frame::isInFrustum occurs often: positions uniform in the camera-frame box [-6, 6] x [-5, 5] x [-2, 12], normals tilted 0-100
    degrees from the viewing ray, maxD = dist * 1.2^U(-3, nlevels + 2), minD = maxD / 1.2^(nlevels - 1).
    -> dict(R, t, Ow, pos, normal, min_dist, max_dist, cam = (fx, fy, cx, cy), bounds = (minX, maxX, minY, maxY), nlevels,
    log_scale, scale_factors); everything float32."""
    r = np.random.default_rng(seed)
    ax = r.normal(size=3); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).astype(np.float32)
    t = r.uniform(-1, 1, 3).astype(np.float32)
    Ow = (-R.T.astype(np.float64) @ t).astype(np.float32)
    Pc = np.stack([r.uniform(-6, 6, M), r.uniform(-5, 5, M), r.uniform(-2, 12, M)], 1)
    P = ((Pc - t) @ R.astype(np.float64)).astype(np.float32)            # R^T (Pc - t)
    PO = P.astype(np.float64) - Ow
    dist = np.linalg.norm(PO, axis=1)
    n = PO / np.maximum(dist, 1e-12)[:, None]
    tilt = r.uniform(0, np.deg2rad(100), M)
    o = np.cross(n, r.normal(size=(M, 3)))
    o /= np.maximum(np.linalg.norm(o, axis=1), 1e-12)[:, None]
    nrm = (np.cos(tilt)[:, None] * n + np.sin(tilt)[:, None] * o).astype(np.float32)
    dmax = (dist * scaleFactor ** r.uniform(-3, nlevels + 2, M)).astype(np.float32)
    dmin = (dmax / scaleFactor ** (nlevels - 1)).astype(np.float32)
    sf, log_scale = scale_tables(nlevels, scaleFactor)
    return dict(R=R, t=t, Ow=Ow, pos=np.ascontiguousarray(P), normal=np.ascontiguousarray(nrm), min_dist=dmin, max_dist=dmax,
                cam=(float(f), float(f), W / 2.0, H / 2.0), bounds=(0.0, float(W), 0.0, float(H)), nlevels=nlevels,
                log_scale=log_scale, scale_factors=sf)


def planted_frame(valid, uv, level, q_desc, n, W, H, nlevels=8, seed=0, jitter=1.5, max_flips=30, frac=0.7, dlevel=(-1, 0)):
    """n keypoints and descriptors of a frame that observes some of the projected queries: up to frac * n of the valid ones get a
    keypoint within `jitter` pixels of uv, at level + one of dlevel, with the query's descriptor and up to max_flips bits flipped; the
    other keypoints are random.  -> (kps, desc n x 32, src = the planted query of each keypoint or -1), shuffled."""
    rng = np.random.default_rng(seed)
    idx = np.flatnonzero(np.asarray(valid) != 0)
    pick = rng.choice(idx, min(len(idx), int(frac * n)), replace=False) if len(idx) else idx
    kps = random_keypoints(n, W, H, nlevels=nlevels, seed=seed + 1)
    desc = random_descriptors(n, seed=seed + 2)
    src = np.full(n, -1, np.int32)
    k = len(pick)
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    kps["x"][:k] = uv[pick, 0] + rng.uniform(-jitter, jitter, k).astype(np.float32)
    kps["y"][:k] = uv[pick, 1] + rng.uniform(-jitter, jitter, k).astype(np.float32)
    kps["octave"][:k] = np.clip(np.asarray(level)[pick] + rng.choice(dlevel, k), 0, nlevels - 1)
    for j, q in enumerate(pick):
        desc[j] = flip_bits(q_desc[q], int(rng.integers(0, max_flips + 1)), rng)
    src[:k] = pick
    perm = rng.permutation(n)
    return kps[perm], np.ascontiguousarray(desc[perm]), src[perm]


# ---- KeyFrame-side matchers: a neighbourhood of keyframes around shared points, and a Sim3 pair -----------------------------------
def _approx_side_projection(R, t, Ow, cam, bounds, P, nrm, dmin, dmax, nlevels, scaleFactor):
    """float64 sketch of the KeyFrame-side projection, for planting keypoints only (the restatement decides every outcome)
    -> (valid, uv, level, z)"""
    P = P.astype(np.float64)
    Pc = P @ R.astype(np.float64).T + t
    z = Pc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = project_np(cam, Pc)
    PO = P - Ow
    dist = np.linalg.norm(PO, axis=1)
    ok = (z > 0) & (uv[:, 0] >= bounds[0]) & (uv[:, 0] < bounds[1]) & (uv[:, 1] >= bounds[2]) & (uv[:, 1] < bounds[3])
    ok &= (dist >= 0.8 * dmin) & (dist <= 1.2 * dmax) & (np.sum(PO * nrm, axis=1) >= 0.5 * dist)
    with np.errstate(divide="ignore", invalid="ignore"):
        lv = np.ceil(np.log(dmax / np.maximum(dist, 1e-12)) / np.log(scaleFactor))
    lv = np.clip(np.nan_to_num(lv), 0, nlevels - 1).astype(np.int32)
    return ok.astype(np.uint8), np.nan_to_num(uv).astype(np.float32), lv, z


def keyframe_neighbourhood(seed, K, M, n_kps=1000, W=346, H=260, nlevels=8, scaleFactor=1.2, mbf=35.0, cam=None, jitter=2.5):
    """K keyframes around the M shared map points of map_scene(seed, M): keyframe k is the scene's camera moved a little, and holds
    n_kps[k] keypoints (an int serves all; 0 gives an empty keyframe) planted by planted_frame on a float64 sketch of its projection.
    uright: none (-1) for a third of the keypoints, near the point's predicted right coordinate for most of the rest, 2-6 px off for
    some (the stereo gate's third term then decides).  -> dict(views = [keyword dicts for frontend.view / proj_ref.view], kps, desc,
    src, uright = lists per keyframe, pos, normal, min_dist, max_dist, mp_desc, scale_factors, inv_sigma2)"""
    s = map_scene(seed, M, W, H, nlevels=nlevels, scaleFactor=scaleFactor)
    rng = np.random.default_rng(seed + 1000)
    n_kps = [int(n_kps)] * K if np.isscalar(n_kps) else [int(n) for n in n_kps]
    cam = tuple(cam) if cam is not None else s["cam"]
    mp_desc = random_descriptors(M, seed=seed + 1)
    sf = s["scale_factors"]
    inv_sigma2 = (np.float32(1.0) / (sf * sf)).astype(np.float32)
    views, kps, desc, src, uright = [], [], [], [], []
    R0, t0 = s["R"].astype(np.float64), s["t"].astype(np.float64)
    for k in range(K):
        dR = rot(*(rng.uniform(-0.06, 0.06, 3) * (k > 0))).astype(np.float64)
        R = (dR @ R0).astype(np.float32)
        t = (dR @ t0 + rng.uniform(-0.4, 0.4, 3) * (k > 0)).astype(np.float32)
        Ow = (-R.T.astype(np.float64) @ t).astype(np.float32)
        views.append(dict(R=R, t=t, Ow=Ow, cam=cam, bounds=s["bounds"], nlevels=nlevels, log_scale=s["log_scale"], scale_factors=sf, mbf=mbf))
        ok, uv, lv, z = _approx_side_projection(R, t, Ow, cam, s["bounds"], s["pos"], s["normal"], s["min_dist"], s["max_dist"], nlevels, scaleFactor)
        kp, d, sr = planted_frame(ok, uv, lv, mp_desc, n_kps[k], W, H, nlevels=nlevels, seed=seed + 10 * k + 2, jitter=jitter)
        n = n_kps[k]
        qur = uv[:, 0] - mbf / np.where(z > 0, z, 1.0)
        ur = np.where(sr >= 0, qur[np.maximum(sr, 0)] + rng.uniform(-1, 1, n), kp["x"] - rng.uniform(1, 30, n)).astype(np.float32)
        off = rng.random(n) < 0.3
        ur[off] += (rng.uniform(2, 6, n) * rng.choice([-1, 1], n)).astype(np.float32)[off]
        ur[rng.random(n) < 0.33] = -1.0
        kps.append(kp); desc.append(d); src.append(sr); uright.append(ur)
    return dict(views=views, kps=kps, desc=desc, src=src, uright=uright, pos=s["pos"], normal=s["normal"], min_dist=s["min_dist"],
                max_dist=s["max_dist"], mp_desc=mp_desc, scale_factors=sf, inv_sigma2=inv_sigma2, W=W, H=H)


def akaze_tables(n_octaves=4, n_layers=4):
    """the AKAZE pyramid of a MixedFrame, one entry per level = octave * n_layers + layer: scale 2^(level / n_layers)
    -> (scale factors, log scale factor)"""
    sf = np.array([2.0 ** (l / n_layers) for l in range(n_octaves * n_layers)], np.float32)
    return sf, np.float32(np.log(np.float32(2.0 ** (1.0 / n_layers))))


def mixed_keyframe_neighbourhood(seed, K, M, n_kps=1000, kinds=None, ak_frac=1.0 / 3.0, cross_frac=0.3, jitter=3.0, **kw):
    """keyframe_neighbourhood(seed, K, M, n_kps) turned into K MixedKeyFrames: about ak_frac of the map points and of each keyframe's
    rows are AKAZE.  The AKAZE pyramid has 16 levels at 2^(1/4) (4 octaves x 4 layers) against the ORB one's 8 at 1.2.  An AKAZE row
    carries class_id = level and octave = class_id / 4 (a reader of octave gets the wrong level); an ORB row keeps octave = level,
    class_id = -1.  A planted row is of its point's type except for cross_frac of them, which are of the other type, sit at a level
    inside the point's window and carry the closer descriptor: only the type gate keeps them out.  kp_inv_sigma2 is the ORB table at
    octave for an ORB row and the AKAZE table at class_id for an AKAZE row (not the ORB table's entry at that row's octave).
    kinds[k] in ("mixed", "orb", "akaze") fixes keyframe k's row types.
    -> keyframe_neighbourhood's dict (views with the AKAZE tables) plus mp_is_orb, kp_is_orb / kp_inv_sigma2 = lists per keyframe,
    ak_scale_factors, ak_inv_sigma2"""
    sc = keyframe_neighbourhood(seed, K, M, n_kps=n_kps, jitter=jitter, **kw)
    rng = np.random.default_rng(seed + 2000)
    ak_sf, ak_log = akaze_tables()
    nA, nO = len(ak_sf), len(sc["scale_factors"])
    ak_is2 = (np.float32(1.0) / (ak_sf * ak_sf)).astype(np.float32)
    mp_is_orb = (rng.random(M) >= ak_frac).astype(np.uint8)
    kinds = ["mixed"] * K if kinds is None else list(kinds)
    kp_is_orb, kp_is2 = [], []
    for k in range(K):
        v = sc["views"][k]
        v.update(ak_nlevels=nA, ak_log_scale=ak_log, ak_scale_factors=ak_sf)
        kp, src, d = sc["kps"][k], sc["src"][k], sc["desc"][k]
        n = len(kp)
        planted = src >= 0
        pt_orb = mp_is_orb[np.maximum(src, 0)]
        if kinds[k] == "mixed":
            cross = rng.random(n) < cross_frac
            io = np.where(planted, np.where(cross, 1 - pt_orb, pt_orb), rng.random(n) >= ak_frac).astype(np.uint8)
        else:
            io = np.full(n, kinds[k] == "orb", np.uint8)
        # the planted rows' levels: the point's predicted level in the point's own pyramid, minus 0 or 1
        _, _, lvA, _ = _approx_side_projection(v["R"], v["t"], v["Ow"], v["cam"], v["bounds"], sc["pos"], sc["normal"], sc["min_dist"],
                                               sc["max_dist"], nA, 2.0 ** 0.25)
        lvl = np.where(pt_orb == 1, kp["octave"], lvA[np.maximum(src, 0)] - rng.integers(0, 2, n))
        lvl = np.where(planted, lvl, np.where(io == 1, kp["octave"], rng.integers(0, nA, n)))
        lvl = np.clip(lvl, 0, np.where(io == 1, nO - 1, nA - 1)).astype(np.int32)
        kp["octave"] = np.where(io == 1, lvl, lvl // 4)
        kp["class_id"] = np.where(io == 1, -1, lvl)
        # a planted row of the other type is the closer one: at most 3 flipped bits
        for i in np.flatnonzero(planted & (io != pt_orb)):
            d[i] = flip_bits(sc["mp_desc"][src[i]], int(rng.integers(0, 4)), rng)
        kp_is_orb.append(io)
        kp_is2.append(np.where(io == 1, sc["inv_sigma2"][np.clip(kp["octave"], 0, nO - 1)], ak_is2[np.clip(lvl, 0, nA - 1)]).astype(np.float32))
    sc.update(mp_is_orb=mp_is_orb, kp_is_orb=kp_is_orb, kp_inv_sigma2=kp_is2, ak_scale_factors=ak_sf, ak_inv_sigma2=ak_is2)
    return sc


def sim3_pair(seed, n=1000, s12=1.0, W=346, H=260, f=280.0, nlevels=8, scaleFactor=1.2, n_both=220, n_one=120, n_cross=120):
    """Two keyframes of n keypoint slots each and a similarity S12 between their cameras (p_c1 = s12*R12*p_c2 + t12), for
    ORBmatcher::SearchBySim3.  Physical points seen by both cameras get a keypoint in each keyframe, with the point's descriptor:
      - n_both of them hold consistent map points in both slots: the two searches agree;
      - n_one have no map point in KF2's slot (skip2): found from KF1 only, removed by the agreement pass;
      - n_cross hold in KF2's slot the map point of another pair (its position and descriptor): the two directions disagree.
    The other slots hold map points from a box around the camera (behind it, outside the image, outside the distance range) or none.
    -> dict(kf1, kf2 = dict(kps, desc, view = keyword dict, pos, min_dist, max_dist, mp_desc, skip), sR12, t12, sR21, t21, W, H)"""
    rng = np.random.default_rng(seed)
    sf, log_scale = scale_tables(nlevels, scaleFactor)
    cam = (float(f), float(f), W / 2.0, H / 2.0)
    bounds = (0.0, float(W), 0.0, float(H))
    Rw = [rot(0.05, -0.1, 0.02), rot(-0.2, 0.15, 0.1)]                         # R1w, R2w
    tw = [np.array([0.3, -0.2, 0.1], np.float32), np.array([-1.0, 0.4, 0.6], np.float32)]
    R12 = rot(0.03, -0.05, 0.02).astype(np.float32)
    t12 = np.array([0.25, -0.1, 0.15], np.float32)
    # :1760-1762 in float, as cv::Mat evaluates them: scalar products, then a 3x3 by 3x1 product
    sR12 = (np.float32(s12) * R12).astype(np.float32)
    sR21 = (np.float64(1.0 / np.float32(s12)) * R12.T.astype(np.float64)).astype(np.float32)
    t21 = (-(sR21.astype(np.float64) @ t12.astype(np.float64))).astype(np.float32)
    S21 = lambda X: X @ sR21.astype(np.float64).T + t21
    S12 = lambda X: X @ sR12.astype(np.float64).T + t12
    world = lambda k, Xc: ((Xc - tw[k]) @ Rw[k].astype(np.float64)).astype(np.float32)          # R^T (Xc - t)
    ng = n_both + n_one + n_cross
    assert ng <= n
    X1 = np.stack([rng.uniform(-2.0, 2.0, ng), rng.uniform(-1.5, 1.5, ng), rng.uniform(4.0, 9.0, ng)], 1)      # in camera 1
    X2 = S21(X1)
    L = rng.integers(0, nlevels, ng)
    d = random_descriptors(ng, seed=seed + 1)
    kf = []
    for k, X in ((0, X1), (1, X2)):
        kps = random_keypoints(n, W, H, nlevels=nlevels, seed=seed + 2 + k)
        desc = random_descriptors(n, seed=seed + 4 + k)
        uv = project_np(cam, X)
        kps["x"][:ng] = uv[:, 0] + rng.uniform(-1.5, 1.5, ng); kps["y"][:ng] = uv[:, 1] + rng.uniform(-1.5, 1.5, ng)
        kps["octave"][:ng] = np.clip(L + rng.choice([-1, 0], ng), 0, nlevels - 1)
        for j in range(ng):
            desc[j] = flip_bits(d[j], int(rng.integers(0, 25)), rng)
        # the slots' own map points: the physical point for the planted slots, a box around the camera for the rest
        Xc = np.stack([rng.uniform(-6, 6, n), rng.uniform(-5, 5, n), rng.uniform(-2, 12, n)], 1)
        Xc[:ng] = X
        dist_other = np.linalg.norm(S21(Xc) if k == 0 else S12(Xc), axis=1)                     # the norm the other camera's test reads
        dmax = dist_other * scaleFactor ** rng.uniform(-3, nlevels + 2, n)
        dmax[:ng] = dist_other[:ng] * scaleFactor ** (L - 0.5)
        mp_desc = random_descriptors(n, seed=seed + 6 + k)
        for j in range(ng):
            mp_desc[j] = flip_bits(d[j], int(rng.integers(0, 25)), rng)
        skip = (rng.random(n) < 0.15).astype(np.uint8)
        skip[:ng] = 0
        kf.append(dict(kps=kps, desc=desc, Xc=Xc, dmax=dmax, mp_desc=mp_desc, skip=skip))
    # KF2's slots of the one-sided pairs hold no map point; those of the crossed pairs hold another pair's point
    one = np.arange(n_both, n_both + n_one); cross = np.arange(n_both + n_one, ng)
    kf[1]["skip"][one] = 1
    other = np.roll(cross, 1)
    kf[1]["Xc"][cross] = X2[other]
    kf[1]["dmax"][cross] = np.linalg.norm(X1[other], axis=1) * scaleFactor ** (L[other] - 0.5)
    for j, o in zip(cross, other):
        kf[1]["mp_desc"][j] = flip_bits(d[o], int(rng.integers(0, 25)), rng)
    out = {}
    for k in (0, 1):
        perm = rng.permutation(n)
        g = kf[k]
        dmax = g["dmax"].astype(np.float32)
        out["kf%d" % (k + 1)] = dict(
            kps=g["kps"][perm], desc=np.ascontiguousarray(g["desc"][perm]),
            view=dict(R=Rw[k], t=tw[k], Ow=(-Rw[k].T.astype(np.float64) @ tw[k]).astype(np.float32), cam=cam, bounds=bounds, nlevels=nlevels,
                      log_scale=log_scale, scale_factors=sf),
            pos=np.ascontiguousarray(world(k, g["Xc"])[perm]), max_dist=dmax[perm],
            min_dist=(dmax / np.float32(scaleFactor ** (nlevels - 1))).astype(np.float32)[perm],
            mp_desc=np.ascontiguousarray(g["mp_desc"][perm]), skip=g["skip"][perm])
    out.update(sR12=sR12, t12=t12, sR21=sR21, t21=t21, W=W, H=H)
    return out


# ---- bag-of-words database (KeyFrameDatabase queries): keyframes of a "place" share most of their words
def _bow_vector(rng, pool, vocab_words, n, p_place):
    """n distinct word ids, a share p_place of them from `pool`, with positive L1-normalised weights (TF-IDF + L1_NORM)"""
    n = int(min(n, vocab_words))
    n_in = int(min(len(pool), round(n * p_place)))
    w_in = rng.choice(pool, size=n_in, replace=False)
    if vocab_words <= 20000:
        rest = rng.choice(np.setdiff1d(np.arange(vocab_words, dtype=np.int64), w_in), size=n - n_in, replace=False)
    else:                                              # a large vocabulary (the latency tool's): draw and reject instead of listing the rest
        rest = np.zeros(0, np.int64)
        while len(rest) < n - n_in:
            c = rng.integers(vocab_words, size=2 * (n - n_in) + 16)
            c = c[np.sort(np.unique(c, return_index=True)[1])]
            rest = np.concatenate([rest, c[~np.isin(c, w_in) & ~np.isin(c, rest)]])
        rest = rest[:n - n_in]
    w = np.sort(np.concatenate([w_in, rest])).astype(np.uint32)
    v = rng.uniform(0.2, 1.0, size=n)
    if n:
        v = v / v.sum()
    return w, v.astype(np.float64)


def bow_database(seed, K, vocab_words=2000, words_per_kf=120, nplaces=4, nqueries=3, p_place=0.85, kf_words=None, query_words=None):
    """K keyframes over `nplaces` places for the KeyFrameDatabase queries (src/KeyFrameDatabase.cc:612-895).  A place owns a subset of the
    vocabulary; a keyframe draws a share of its words (between 0.45 and p_place, so that the 0.8 rule splits the keyframes of a place) from
    its place's subset and the rest from anywhere, with L1-normalised positive weights.  kf_words (optional, K ints): the length of each
    keyframe's vector instead of about words_per_kf; query_words: the length of each query's.
    Returns dict(vocab_words, place (K), kfs = [(word, val)], covis (K, 10) int32: up to ten neighbours in order, a mix of same-place and
    other-place keyframes and -1, queries = [dict(word, val, place)])."""
    rng = np.random.default_rng(seed)
    nplaces = max(1, min(nplaces, max(K, 1)))
    sub = int(max(min(vocab_words // nplaces, 2 * words_per_kf), 1))
    pools = [np.arange(p * sub, (p + 1) * sub, dtype=np.int64) % vocab_words for p in range(nplaces)]
    place = (np.arange(K) % nplaces).astype(np.int32)
    rng.shuffle(place)
    kfs = []
    for k in range(K):
        n = int(kf_words[k]) if kf_words is not None else int(rng.integers(max(words_per_kf * 3 // 4, 1), words_per_kf * 5 // 4 + 1))
        kfs.append(_bow_vector(rng, pools[place[k]], vocab_words, n, rng.uniform(0.45, p_place)))
    covis = np.full((K, 10), -1, np.int32)
    for k in range(K):
        same = np.flatnonzero((place == place[k]) & (np.arange(K) != k)); other = np.flatnonzero(place != place[k])
        for j in range(10):
            u = rng.uniform()
            if u < 0.6 and len(same):
                covis[k, j] = rng.choice(same)
            elif u < 0.8 and len(other):
                covis[k, j] = rng.choice(other)
    queries = []
    for i in range(nqueries):
        p = int(rng.integers(nplaces))
        n = int(query_words[i]) if query_words is not None else words_per_kf
        w, v = _bow_vector(rng, pools[p], vocab_words, n, p_place)
        queries.append(dict(word=w, val=v, place=p))
    return dict(vocab_words=vocab_words, place=place, kfs=kfs, covis=covis, queries=queries)
