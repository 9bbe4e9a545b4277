"""Scenes of CreateNewMapPoints' per-match half: small keyframes (n1, n2 of 48 to 200; K = 1, 3, 4) as plain dicts that
tests/newpts_ref (restatement, models) and the device entry points read alike.  Random geometry gives the bulk; the rest is planted:
pairs whose compared quantity sits on, or on the floats either side of, every comparison of the loop (found with the Python model by
bisection over a per-keypoint input, or built from powers of two so that the arithmetic is exact), and the map-level cases the two
sequential rules need.  Everything is generated from seeds; nothing is stored."""
import numpy as np

from eorb_slam_amd.synth import KP_DTYPE

LOCAL_MAPPING, TRACKING = 0, 1
PIN = (458.0, 457.0, 367.0, 248.0)
PIN2 = (512.0, 512.0, 1024.0, 512.0)
KB8 = (190.9, 190.9, 254.9, 256.9, 0.0034, 0.0007, -0.0020, 0.0002)
LEVEL_SCALE = np.array([1.2 ** i for i in range(8)], np.float32)
LEVEL_SIGMA2 = (LEVEL_SCALE * LEVEL_SCALE).astype(np.float32)


def rot(axis, ang):
    axis = np.asarray(axis, np.float64); axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def make_view(R, t, cam, mbf=0.0, Ow=None):
    """R, t = mRcw, mtcw in float; Ow = -R^T t computed in float64 and narrowed unless given"""
    R = np.asarray(R, np.float32).reshape(3, 3); t = np.asarray(t, np.float32).reshape(3)
    Ow = (-(R.astype(np.float64).T @ t.astype(np.float64))).astype(np.float32) if Ow is None else np.asarray(Ow, np.float32)
    return dict(R=R, t=t, Ow=Ow, cam=tuple(cam), mbf=float(mbf))


def project64(cam, R, t, X):
    """float64 projection of world points by either camera model -> (uv, z)"""
    P = X @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    fx, fy, cx, cy = cam[:4]
    if len(cam) <= 4:
        return np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], 1), P[:, 2]
    k = cam[4:8]
    th = np.arctan2(np.hypot(P[:, 0], P[:, 1]), P[:, 2]); psi = np.arctan2(P[:, 1], P[:, 0])
    r = th + k[0] * th ** 3 + k[1] * th ** 5 + k[2] * th ** 7 + k[3] * th ** 9
    return np.stack([fx * r * np.cos(psi) + cx, fy * r * np.sin(psi) + cy], 1), P[:, 2]


def kps_of(uv, octave):
    k = np.zeros(len(uv), KP_DTYPE)
    k["x"] = uv[:, 0]; k["y"] = uv[:, 1]; k["size"] = 31.0; k["angle"] = 0.0; k["response"] = 1.0; k["octave"] = octave
    return k


def base(name, form, K, kps1, kf_kps, match12, views1, views2, **kw):
    kf_off = np.cumsum([0] + [len(k) for k in kf_kps]).astype(np.int32)
    sc = dict(name=name, form=form, K=K, n1=len(kps1), kps1=np.ascontiguousarray(kps1, KP_DTYPE),
              kps2=np.ascontiguousarray(np.concatenate(list(kf_kps) + [np.zeros(0, KP_DTYPE)]), KP_DTYPE), kf_off=kf_off,
              match12=np.ascontiguousarray(match12, np.int32).reshape(K, len(kps1)), views1=views1, views2=views2, nleft1=-1, nleft2=None,
              mb1=0.0, mb2=None, side1={}, side2={}, level_scale=LEVEL_SCALE, level_sigma2=LEVEL_SIGMA2, rf_orb=np.float32(1.5) * np.float32(1.2),
              rf_ak=np.float32(1.5) * np.float32(1.3), far_points=False, th_far=0.0)
    sc.update(kw)
    return sc


def random_scene(name, seed, K=3, n1=96, n2=80, form=LOCAL_MAPPING, cam1=PIN, cam2=None, stereo=False, mixed=False, wrong=0.15, far=None):
    """pKF1 near the origin, K neighbours 0.3-0.9 m away, points 2-20 m ahead (a few very far: low parallax), keypoints = the float64
    projection plus up to half a pixel; neighbour k sees a random subset; a share `wrong` of the matches goes to another keypoint"""
    rng = np.random.default_rng(seed)
    cam2 = cam2 or [cam1] * K
    R1 = rot(rng.normal(size=3), 0.05); t1 = rng.normal(size=3) * 0.1
    X = np.stack([rng.uniform(-4, 4, n1), rng.uniform(-3, 3, n1), rng.uniform(2, 20, n1)], 1)
    X[rng.random(n1) < 0.1, 2] *= 40                                    # low parallax
    X = (X - t1) @ R1                                                   # world = R1^T (Pc - t1)
    oct1 = rng.integers(0, 8, n1)
    uv1, z1 = project64(cam1, R1, t1, X)
    kps1 = kps_of(uv1 + rng.uniform(-0.5, 0.5, uv1.shape) * LEVEL_SCALE[oct1][:, None], oct1)
    mb = 0.11
    v1 = make_view(R1, t1, cam1, mbf=mb * cam1[0] if stereo else 0.0)
    views2, kf_kps, match12, mbs = [], [], np.full((K, n1), -1, np.int32), []
    side1, side2 = {}, {k: [] for k in ("uright", "depth", "raw_xy", "kp_is_orb", "kp_sigma2", "kp_scale")}
    if stereo:
        has = rng.random(n1) < 0.6
        d = np.where(z1 > 0, z1, 1.0) * rng.uniform(0.97, 1.03, n1)
        side1 = dict(uright=np.where(has, kps1["x"] - mb * cam1[0] / d, -1).astype(np.float32), depth=np.where(has, d, -1).astype(np.float32),
                     raw_xy=np.stack([kps1["x"] + rng.uniform(-2, 2, n1), kps1["y"] + rng.uniform(-2, 2, n1)], 1).astype(np.float32))
    if mixed:
        side1["kp_is_orb"] = (rng.random(n1) < 0.6).astype(np.uint8)
    for k in range(K):
        R2 = rot(rng.normal(size=3), 0.08) @ R1
        c2 = -R1.T @ t1 + rng.normal(size=3) * np.array([0.5, 0.3, 0.15]) + np.array([0.4 * (k + 1), 0, 0])
        if stereo and k == 0:                                           # closer than the stereo baseline: UnprojectStereo is chosen
            c2 = -R1.T @ t1 + np.array([0.02, 0.005, 0.0])
        t2 = -R2 @ c2
        mb2 = 0.11 + 0.06 * k
        sel = rng.permutation(n1)[:min(n2, n1)]
        extra = n2 - len(sel)
        Xk = np.concatenate([X[sel], np.stack([rng.uniform(-4, 4, extra), rng.uniform(-3, 3, extra), rng.uniform(2, 20, extra)], 1)]) if extra > 0 else X[sel]
        octk = np.clip(np.concatenate([oct1[sel], rng.integers(0, 8, max(extra, 0))]) + rng.integers(-1, 2, n2) * (rng.random(n2) < 0.3), 0, 7)
        uv2, z2 = project64(cam2[k], R2, t2, Xk)
        kk = kps_of(uv2 + rng.uniform(-0.5, 0.5, uv2.shape) * LEVEL_SCALE[octk][:, None], octk)
        perm = rng.permutation(n2)
        kk = kk[perm]; z2 = z2[perm]
        inv = np.argsort(perm)
        matched = rng.random(len(sel)) < 0.55
        for j, i1 in enumerate(sel):
            if matched[j]:
                match12[k, i1] = inv[j] if rng.random() > wrong else rng.integers(0, n2)
        kf_kps.append(kk); mbs.append(mb2)
        views2.append([make_view(R2, t2, cam2[k], mbf=mb2 * cam2[k][0] if stereo else 0.0)])
        if stereo:
            has = rng.random(n2) < 0.6
            d = np.where(z2 > 0, z2, 1.0) * rng.uniform(0.97, 1.03, n2)
            side2["uright"].append(np.where(has, kk["x"] - mb2 * cam2[k][0] / d, -1)); side2["depth"].append(np.where(has, d, -1))
            side2["raw_xy"].append(np.stack([kk["x"] + rng.uniform(-2, 2, n2), kk["y"] + rng.uniform(-2, 2, n2)], 1))
        if mixed:
            o = np.ones(n2, np.uint8)
            for j, i1 in enumerate(sel):
                o[inv[j]] = side1["kp_is_orb"][i1] if rng.random() > 0.1 else 1 - side1["kp_is_orb"][i1]
            side2["kp_is_orb"].append(o)
    s2 = {}
    for key, t in (("uright", np.float32), ("depth", np.float32), ("raw_xy", np.float32), ("kp_is_orb", np.uint8)):
        if side2[key]:
            s2[key] = np.ascontiguousarray(np.concatenate(side2[key]), t)
    sc = base(name, form, K, kps1, kf_kps, match12, [v1], views2, side1=side1, side2=s2, mb1=mb if stereo else 0.0,
              mb2=np.array(mbs, np.float32) if stereo else None)
    if far is not None:
        sc["far_points"] = True; sc["th_far"] = float(far)
    return sc


def twocam_scene(name, seed, K=3, nl=60, nr=40):
    """two-camera keyframes: a KannalaBrandt8 mpCamera and, per keyframe, a KannalaBrandt8 or a Pinhole mpCamera2; kps = left then right;
    the matches reach ll, lr, rl and rr"""
    rng = np.random.default_rng(seed)
    Rrl = rot([0, 1, 0], 0.05); trl = np.array([-0.1, 0.0, 0.0])

    def pair_views(R, t, camr):
        Rr, tr = Rrl @ R, Rrl @ t + trl
        return [make_view(R, t, KB8), make_view(Rr, tr, camr)]
    n1 = nl + nr
    R1 = rot(rng.normal(size=3), 0.05); t1 = rng.normal(size=3) * 0.1
    X = np.stack([rng.uniform(-3, 3, n1), rng.uniform(-2, 2, n1), rng.uniform(2, 12, n1)], 1)
    X = (X - t1) @ R1
    camr1 = PIN
    v1 = pair_views(R1, t1, camr1)
    oct1 = rng.integers(0, 8, n1)
    uvl, _ = project64(KB8, v1[0]["R"], v1[0]["t"], X[:nl]); uvr, _ = project64(camr1, v1[1]["R"], v1[1]["t"], X[nl:])
    kps1 = kps_of(np.concatenate([uvl, uvr]) + rng.uniform(-0.4, 0.4, (n1, 2)), oct1)
    views2, kf_kps, match12, nleft2 = [], [], np.full((K, n1), -1, np.int32), []
    for k in range(K):
        R2 = rot(rng.normal(size=3), 0.08) @ R1
        c2 = -R1.T @ t1 + np.array([0.4 * (k + 1), 0.1, 0.05])
        t2 = -R2 @ c2
        camr = KB8 if k % 2 == 0 else PIN
        v2 = pair_views(R2, t2, camr)
        side = rng.random(n1) < 0.5                                     # which camera of keyframe k sees point i
        order = np.concatenate([np.nonzero(~side)[0], np.nonzero(side)[0]]); nl2 = int((~side).sum())
        uv = np.zeros((n1, 2))
        uv[:nl2], _ = project64(KB8, v2[0]["R"], v2[0]["t"], X[order[:nl2]])
        uv[nl2:], _ = project64(camr, v2[1]["R"], v2[1]["t"], X[order[nl2:]])
        kf_kps.append(kps_of(uv + rng.uniform(-0.4, 0.4, uv.shape), oct1[order]))
        inv = np.argsort(order)
        m = rng.random(n1) < 0.6
        match12[k, m] = inv[m]
        views2.append(v2); nleft2.append(nl2)
    return base(name, LOCAL_MAPPING, K, kps1, kf_kps, match12, v1, views2, nleft1=nl, nleft2=np.array(nleft2, np.int32))


def exact_scene(name="exact", form=LOCAL_MAPPING, nonfinite=False):
    """identity rotations, focal length 512 and coordinates that are sums of a few powers of two: every step of the stereo branch is exact,
    so the compared quantities can be put ON their thresholds.  K = 3: neighbour 0 half a metre to the right, neighbour 1 turned by a
    quarter turn about y (a ray at right angles to pKF1's optical axis), neighbour 2 with a camera centre that coincides with a point."""
    cam = PIN2
    I = np.eye(3)
    v1 = make_view(I, [0, 0, 0], cam, mbf=2048.0)                      # mb = 4: wider than the baselines, so UnprojectStereo is chosen
    Ry = np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]])                # Rcw of neighbour 1: Rwc*(0,0,1) = (1,0,0)
    rows1, rows = [], {0: [], 1: [], 2: []}
    s1 = dict(uright=[], depth=[], kp_sigma2=[], kp_scale=[], raw_xy=[])
    s2 = {k: dict(uright=[], depth=[], kp_sigma2=[], kp_scale=[]) for k in range(3)}
    match = []

    def add(k, kp1, kp2, ur1=-1.0, d1=-1.0, sg1=1.0, scl1=1.0, ur2=-1.0, d2=-1.0, sg2=1.0, scl2=1.0, raw1=None):
        rows1.append(kp1); rows[k].append(kp2); match.append((k, len(rows1) - 1, len(rows[k]) - 1))
        for key, v in (("uright", ur1), ("depth", d1), ("kp_sigma2", sg1), ("kp_scale", scl1), ("raw_xy", raw1 or kp1)):
            s1[key].append(v)
        for key, v in (("uright", ur2), ("depth", d2), ("kp_sigma2", sg2), ("kp_scale", scl2)):
            s2[k][key].append(v)
    # a stereo point of pKF1 on its axis at (0, 0, 4): u = 1024, v = 512, u_r = 1024 - 2048/4 = 512; neighbour 0 is 3 m to the right
    # (t = (-3, 0, 0)) and sees it at (-3, 0, 4): u = 512*(-3)/4 + 1024 = 640.  dist1 = 4, dist2 = 5, ratioDist = 1.25, the cosine of the
    # rays 0.8 against cos(2*atan2(2, 4)) = 0.6 of the stereo pair: no linear triangulation, UnprojectStereo(idx1).
    P = dict(kp1=(1024.0, 512.0), kp2=(640.0, 512.0), ur1=512.0, d1=4.0)
    nxt = lambda x, up: float(np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf)))      # noqa: E731
    add(0, **P)                                                          # 0: accepted; both errors are exactly 0
    add(0, **P, sg1=0.0)                                                 # 1: e1 == 7.8*sigma2 == 0: ">" passes, ">=" would not
    add(0, **P, sg2=0.0)                                                 # 2: e2 == 5.991*sigma2 == 0
    add(0, **P, scl1=2.5)                                                # 3: ratioDist*ratioFactor == ratioOctave (ratioFactor = 2): passes
    add(0, **P, scl1=nxt(2.5, True))                                     # 4: one float beyond: scale
    add(0, **P, scl1=0.625)                                              # 5: ratioDist == ratioOctave*ratioFactor: passes
    add(0, **P, scl1=nxt(0.625, False))                                  # 6: one float beyond: scale
    add(0, **dict(P, d1=0.0))                                            # 7: depth <= 0 with a right coordinate: the empty Mat
    add(0, **dict(P, d1=-4.0))                                           # 8: likewise, negative
    # z2 == 0: neighbour 2 sits 4 m ahead on the axis (t = (0, 0, -4)): z2 = 4 - 4; and one float of depth either side
    add(2, kp1=(1024.0, 512.0), kp2=(1024.0, 512.0), ur1=512.0, d1=4.0)                 # 9: z2 == 0
    add(2, kp1=(1024.0, 512.0), kp2=(1024.0, 512.0), ur1=512.0, d1=nxt(4.0, True))      # 10: z2 the smallest step above 0
    add(2, kp1=(1024.0, 512.0), kp2=(1024.0, 512.0), ur1=512.0, d1=nxt(4.0, False))     # 11: below
    # cosParallaxRays == 0: the principal rays of pKF1 and of neighbour 1 are at right angles
    add(1, kp1=(1024.0, 512.0), kp2=(1024.0, 512.0))                     # 12
    add(1, kp1=(1024.0, 512.0), kp2=(1024.0, 512.0), ur1=512.0, d1=4.0)  # 13: the same with a stereo keypoint
    # z1 == 0: a stereo point of neighbour 1 four metres along its axis is at (3.5, 0, 0), in pKF1's image plane
    add(1, kp1=(1024.0, 512.0), kp2=(1024.0, 512.0), ur2=896.0, d2=4.0)  # 14
    if nonfinite:
        add(0, **dict(P, raw1=(3e38, 512.0)))                            # 15: mvKeys far outside: (u - cx)*z overflows a float
    v2 = [[make_view(I, [-3.0, 0, 0], cam, mbf=512.0)], [make_view(Ry, [0, 0, 0.5], cam, mbf=512.0)], [make_view(I, [0, 0, -4.0], cam, mbf=512.0)]]
    kps1 = kps_of(np.array(rows1, np.float64), 0)
    kf_kps = [kps_of(np.array(rows[k], np.float64).reshape(-1, 2), 0) for k in range(3)]
    n1 = len(rows1)
    m = np.full((3, n1), -1, np.int32)
    for k, i1, i2 in match:
        m[k, i1] = i2
    cat = lambda key: np.concatenate([np.array(s2[k][key], np.float32) for k in range(3)])      # noqa: E731
    side1 = {key: np.array(v, np.float32) for key, v in s1.items()}
    side2 = {key: cat(key) for key in s2[0]}
    return base(name, form, 3, kps1, kf_kps, m, [v1], v2, side1=side1, side2=side2, mb1=4.0, mb2=np.array([1.0, 1.0, 1.0], np.float32),
                rf_orb=np.float32(2.0), rf_ak=np.float32(2.0), far_points=True, th_far=nxt(5.0, True))


def exact_far(on):
    """exact_scene with mThFarPoints ON dist2 = 5 of neighbour 0's pairs (all far) or one float above it (none)"""
    sc = exact_scene("exact_far_on" if on else "exact_far_above")
    sc["th_far"] = 5.0 if on else float(np.nextafter(np.float32(5.0), np.float32(np.inf)))
    return sc


def zero_dist_scene():
    """dist2 == 0: neighbour 0's Ow on the point (an Ow that is not -R^T t is the caller's to give; the depth signs pass first)"""
    sc = exact_scene("zero_dist")
    sc["views2"][0][0]["Ow"] = np.array([0.0, 0.0, 4.0], np.float32)
    return sc


def claim_scene(seed=11):
    """the claim: every idx1 matched in neighbours 1 and 2 gets a wrong keypoint of neighbour 0 as its match there, so it is rejected at 0,
    accepted at 1 and claimed at 2; pairs of other idx1 become twins (the same keypoint) on one idx2 of neighbour 0 and are both accepted"""
    sc = random_scene("claim", seed, K=3, n1=64, n2=64, wrong=0.0)
    m = sc["match12"]
    rng = np.random.default_rng(seed)
    for i in np.nonzero((m[1] >= 0) & (m[2] >= 0))[0]:
        m[0, i] = (max(m[0, i], 0) + 1 + rng.integers(0, 60)) % 64        # a keypoint of neighbour 0 that is not this point's
    both = np.nonzero((m[0] >= 0) & ~((m[1] >= 0) & (m[2] >= 0)))[0]
    for b, c in zip(both[0::2], both[1::2]):                              # idx1 = c becomes a twin of b: same keypoint, same idx2
        sc["kps1"][c] = sc["kps1"][b]; m[:, c] = -1; m[0, c] = m[0, b]
    return sc


def mixed_scene(seed=6):
    """mixed ORB + AKAZE keyframes, K = 4, with the first AKAZE-AKAZE pair in the middle of neighbour 1: neighbour 0's keypoints are all
    ORB (a non-ORB idx1 matched there leaves at the type gate and does not switch the factor), and so are neighbour 1's and 2's for
    idx1 < n1/2 and all of neighbour 3's.
    The two factors are far apart so that the switch decides pairs."""
    sc = random_scene("mixed", seed, K=4, n1=64, n2=64, mixed=True, wrong=0.05)
    o2 = sc["side2"]["kp_is_orb"]; off = sc["kf_off"]
    o2[off[0]:off[1]] = 1
    for k in (1, 2):
        for i in range(sc["n1"] // 2):
            if sc["match12"][k, i] >= 0:
                o2[off[k] + sc["match12"][k, i]] = 1
    o2[off[3]:off[4]] = 1                                               # neighbour 3 is all ORB and is judged with the AKAZE factor
    sc["rf_orb"] = np.float32(1.02); sc["rf_ak"] = np.float32(1.5) * np.float32(1.4)
    return sc


def bisect_float(lo, hi, pred):
    """floats lo < hi with pred(lo) != pred(hi) -> adjacent floats (a, b), a < b, with pred(a) == pred(lo) and pred(b) == pred(hi)"""
    lo, hi = np.float32(lo), np.float32(hi)
    plo = pred(lo)
    assert plo != pred(hi)
    while np.nextafter(lo, np.float32(np.inf)) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if mid <= lo or mid >= hi:
            break
        if pred(mid) == plo:
            lo = mid
        else:
            hi = mid
    return lo, hi


def sides_scenes():
    """pairs of scenes that differ in one float by one step and sit either side of a comparison no exact construction reaches: name ->
    (scene a, scene b, what differs).  Found with the Python model by bisection, so they are planted for the model's arithmetic, which the
    restatement must share.
      parallax: a monocular pair whose cosParallaxRays is the float below 0.9998 in a (linear triangulation) and 0.9998f, the float above the
                double 0.9998, in b (low parallax): kps2.x of the pair moves;
      chi1 / chi2: an accepted pair whose kp_sigma2 shrinks until 5.991*sigma2 is the first double below the float error."""
    import newpts_ref as nr
    out = {}
    sc0 = random_scene("sides", 21, K=1, n1=48, n2=48, wrong=0.0)
    n1 = sc0["n1"]
    sc0["side1"] = dict(kp_sigma2=LEVEL_SIGMA2[sc0["kps1"]["octave"]].copy()); sc0["side2"] = dict(kp_sigma2=LEVEL_SIGMA2[sc0["kps2"]["octave"]].copy())
    ref = nr.loop_model(sc0)

    def twin(edit, v):
        sc = dict(sc0)
        sc["kps2"] = sc0["kps2"].copy(); sc["side1"] = {k: a.copy() for k, a in sc0["side1"].items()}; sc["side2"] = {k: a.copy() for k, a in sc0["side2"].items()}
        edit(sc, np.float32(v))
        return sc
    ok = [i for i in range(n1) if ref["status"][0, i] == nr.S["new"]]
    i = ok[0]; j = int(sc0["match12"][0, i])
    st = lambda sc: int(nr.pair_model(sc, 0, i, j, sc["rf_orb"])[0])      # noqa: E731
    for name, side, row in (("chi1", "side1", i), ("chi2", "side2", j)):
        def edit(sc, v, side=side, row=row):
            sc[side]["kp_sigma2"][row] = v
        a, b = bisect_float(0.0, sc0[side]["kp_sigma2"][row], lambda v: st(twin(edit, v)) == nr.S["new"])
        out[name] = (twin(edit, a), twin(edit, b), (side, row, a, b))
    low = [q for q in range(n1) if ref["status"][0, q] == nr.S["parallax"] and sc0["match12"][0, q] >= 0]
    i2 = low[0]; j2 = int(sc0["match12"][0, i2])

    def editx(sc, v):
        sc["kps2"]["x"][j2] = v
    stx = lambda v: int(nr.pair_model(twin(editx, v), 0, i2, j2, sc0["rf_orb"])[0]) == nr.S["parallax"]      # noqa: E731
    x0 = sc0["kps2"]["x"][j2]
    hi = next(x0 + d for d in (8.0, -8.0, 16.0, -16.0, 40.0, -40.0) if not stx(x0 + d))
    a, b = bisect_float(min(x0, hi), max(x0, hi), stx)
    sa, sb = (twin(editx, b), twin(editx, a)) if stx(a) else (twin(editx, a), twin(editx, b))      # a: triangulated, b: low parallax
    out["parallax"] = (sa, sb, ("kps2.x", j2, a, b, i2))
    for name, (sa, sb, _) in out.items():
        sa["name"] = "sides_%s_a" % name; sb["name"] = "sides_%s_b" % name
    return out


def all_scenes():
    """name -> scene, every committed scene (the planted-margin ones first)"""
    out = {}
    for sc in (exact_scene(), exact_scene("exact_tracking", TRACKING), exact_far(True), exact_far(False), zero_dist_scene(),
               exact_scene("nonfinite", nonfinite=True)):
        out[sc["name"]] = sc
    for sa, sb, _ in sides_scenes().values():
        out[sa["name"]] = sa; out[sb["name"]] = sb
    out["mono"] = random_scene("mono", 1, K=3, n1=96, n2=80, far=15.0)
    out["mono_k1"] = random_scene("mono_k1", 2, K=1, n1=200, n2=150)
    out["mono_wide"] = random_scene("mono_wide", 7, K=4, n1=300, n2=200)        # 1200 slots: more than one workgroup of the device's pair kernel
    out["mono_tracking"] = random_scene("mono_tracking", 1, K=3, n1=96, n2=80, form=TRACKING)
    out["kb8"] = random_scene("kb8", 3, K=3, n1=80, n2=64, cam1=KB8, cam2=[KB8, PIN, KB8])
    out["stereo"] = random_scene("stereo", 4, K=3, n1=96, n2=96, stereo=True)
    out["stereo_tracking"] = random_scene("stereo_tracking", 4, K=3, n1=96, n2=96, stereo=True, form=TRACKING)
    out["twocam"] = twocam_scene("twocam", 5)
    out["mixed"] = mixed_scene()
    out["claim"] = claim_scene()
    return out


PLANTED = ("exact", "exact_tracking", "exact_far_on", "exact_far_above", "zero_dist", "sides_chi1_a", "sides_chi1_b", "sides_chi2_a", "sides_chi2_b",
           "sides_parallax_a", "sides_parallax_b")


# ---- the triangulation neighbourhoods of tests/kfbatch_cases.py (descriptors, feature vectors, F12) with the views of their poses --------
def search_scene(kind, K=4):
    """-> (the neighbourhood, views1, views2, level_scale, level_sigma2): the search's inputs and the stage's"""
    import kfbatch_cases as kc
    from eorb_slam_amd import synth
    s = kc.tri_scene(kind, K)
    scale, sigma2 = synth.level_tables()
    I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    if kind == "twocam":
        Rrl, trl = synth.rot(0.002, -0.01, 0.003), np.array([-0.11, 0.001, 0.002], np.float32)

        def rig(R, t):
            return [make_view(R, t, synth.CAM_L),
                    make_view((Rrl.astype(np.float64) @ R).astype(np.float32), (Rrl.astype(np.float64) @ t + trl).astype(np.float32), synth.CAM_R)]
    else:
        cam = synth.CAM_MONO[:4] if kind.startswith("pinhole") else synth.CAM_MONO

        def rig(R, t):
            return [make_view(R, t, cam)]
    return s, rig(I, z), [rig(*synth.neighbour_pose(k)) for k in range(K)], scale, sigma2


def scene_of_search(s, views1, views2, scale, sigma2, match12, kind, ks=None):
    """the stage's scene for rows match12 of the neighbours ks (default all) of a search scene"""
    ks = list(range(len(s["kfs"]))) if ks is None else list(ks)
    sc = base("search_" + kind, LOCAL_MAPPING, len(ks), s["kps1"], [s["kfs"][k]["kps"] for k in ks], match12, views1, [views2[k] for k in ks],
              level_scale=scale, level_sigma2=sigma2, rf_orb=np.float32(1.5) * scale[1], rf_ak=np.float32(1.5) * scale[1])
    if kind == "twocam":
        sc["nleft1"] = int(s["nleft1"]); sc["nleft2"] = np.array([s["kfs"][k]["nleft"] for k in ks], np.int32)
    return sc
