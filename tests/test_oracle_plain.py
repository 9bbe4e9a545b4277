"""The oracle's float stages against the plain float64 restatements of tests/plain_ref.py (no GPU): Gaussian event accumulation,
the motion-compensating warps (SE3 / SE2, pinhole / KannalaBrandt8) and their images, measureImageFocus, cv::normalize,
IC_Angle, steered rBRIEF and pyramidal Lucas-Kanade.  Bit parity between the kernels and the oracle proves that the two agree; these
tests prove that what they agree on is the formula.  tests/test_gpu_plain.py imports the inputs, the checks and the tolerances
below and applies them to the kernels.

Tolerances.  Where a bound follows from the arithmetic it is derived (plain_ref.gauss_bound).  Where it cannot be (float Newton
iterations, tanf, the polynomial atan2, fixed-point Lucas-Kanade) the oracle's worst deviation from the plain reference was
measured on the CPU and stands in MEASURED; a test allows FACTOR times it (the convention of tests/test_twoview_ref.py; the
margin covers other libm builds).  No number of MEASURED was taken from a kernel.

Teeth.  Every check also runs against a deliberately wrong variant of the plain reference (wrong=...) and must fail."""
import functools

import numpy as np
import pytest

from eorb_slam_amd import synth
import plain_ref as pr

F64 = np.float64
FACTOR = 4.0

# the oracle's worst deviation from the plain reference over the cases of this module
MEASURED = {
    ("uv", "pinhole", "se3"): 1.28e-5,        # px, either axis (median depth 1.28e-5, per-event depth 1.26e-5)
    ("uv", "pinhole", "se2"): 2.96e-5,        # (3 parameters 2.44e-5, 4 parameters 2.96e-5)
    ("uv", "kb8", "se3"): 4.32e-5,            # (4.01e-5, 4.32e-5)
    ("uv", "kb8", "se2"): 6.35e-5,            # (6.12e-5, 6.35e-5)
    "focus": 9.9e-9,                          # absolute, of focus values 0.12 .. 0.13 (float32 results: half an ulp is 3.7e-9); 1.8e-9, 8.5e-10, 9.9e-9
    "ic_angle": 0.00936,                      # degrees (0.00903 .. 0.00936 over the four images)
    "lk": 0.00155,                            # px, either axis (0.00014 .. 0.00155 over the six cases, medians 0.00006 .. 0.00025)
}

EVETHZ_CAM = (199.092366542, 198.82882047, 132.192071378, 110.712660011)                  # as tests/test_gpu_parity.py
MVSEC_KB8 = (226.38018519795807, 226.15002947047415, 173.6470807871759, 133.73271487507847,
             -0.048031442223833355, 0.011330957517194437, -0.055378166304281135, 0.021500973881459395)


def cam64(cam):
    """the camera as the float32 structure of the entry points holds it"""
    return tuple(np.asarray(cam, np.float32).astype(F64).tolist())


# ---------------------------------------------------------------------------------------------------
# accumulation
ACC_CASES = [(W, H, sigma, pol) for (W, H) in ((64, 48), (61, 47), (37, 29)) for sigma in (0.7, 1.0, 1.5, 2.0) for pol in (False, True)]
_ACC_N = {64: 2600, 61: 3000, 37: 1500}


@functools.lru_cache(maxsize=None)
def acc_events(W, H):
    """Uniform fractional positions up to 4 px outside all four edges (one event pinned 3 - 4 px outside each edge), 50 exactly
    integer positions, and a hot pixel: 500 - 800 events at one fractional position whose x and y remainders differ; shuffled."""
    rng = np.random.default_rng(1000 * W + H)
    n = _ACC_N[W]
    hot = int(rng.integers(500, 801))
    x = rng.uniform(-4.0, W + 4.0, n); y = rng.uniform(-4.0, H + 4.0, n)
    x[:4] = (-3.75, W + 3.5, W / 2 + 0.3, W / 3 + 0.6); y[:4] = (H / 2 + 0.2, H / 3 + 0.7, -3.25, H + 3.625)
    x[4:54] = rng.integers(0, W, 50); y[4:54] = rng.integers(0, H, 50)
    x[54:54 + hot] = W // 2 + 0.27; y[54:54 + hot] = H // 3 + 0.81
    order = rng.permutation(n)
    ev = np.zeros(n, synth.EVENT_DTYPE)
    ev["x"] = x[order].astype(np.float32); ev["y"] = y[order].astype(np.float32)
    ev["ts"] = np.arange(n) * 1e-6
    ev["p"] = rng.integers(0, 2, n).astype(np.uint8)
    ev.flags.writeable = False
    assert (ev["x"] < 0).any() and (ev["x"] >= W).any() and (ev["y"] < 0).any() and (ev["y"] >= H).any()
    return ev


@functools.lru_cache(maxsize=None)
def acc_plain(W, H, sigma, pol, wrong=None):
    return pr.gauss_image(acc_events(W, H), W, H, sigma, pol, wrong=wrong)


def check_accumulation(what, f32, mm, u8, ref, mask=None, extra=0.0):
    """f32, mm, u8: an accumulation's float image, running extremes (min, max) and normalised image (or None); ref: plain_ref.gauss_image.
    |f32 - plain| <= gauss_bound (+ extra) per pixel; the extremes within the bound at the pixel that set them; u8 within one grey level
    of rint of the plain image scaled by the plain extremes.  Returns the worst ratio error / bound."""
    bound = pr.gauss_bound(ref) + extra
    err = np.abs(f32.astype(F64) - ref["img"])
    ok = err <= bound
    if mask is not None:
        ok |= mask
    touched = ref["M"] > 0
    ratio = float((err[touched & ok] / bound[touched & ok]).max()) if (touched & ok).any() else 0.0
    bad = np.argwhere(~ok)
    assert len(bad) == 0, "%s: %d pixels outside the bound, first (x, y) = (%d, %d): got %.9g, plain %.9g, bound %.3g" % (
        what, len(bad), bad[0][1], bad[0][0], f32[tuple(bad[0])], ref["img"][tuple(bad[0])], bound[tuple(bad[0])])
    if mm is not None:
        for got, key in ((mm[0], "min"), (mm[1], "max")):
            at = ref[key + "_at"]
            b = 0.0 if at is None else bound[at]
            assert abs(F64(got) - ref[key]) <= b, "%s: %sVal %.9g, plain %.9g at %s, bound %.3g" % (what, key, got, ref[key], at, b)
    share = 0.0
    if u8 is not None:
        want = np.rint(pr.scale_u8(ref["img"], ref["min"], ref["max"]))
        d = np.abs(u8.astype(F64) - want)
        if mask is not None:
            d = np.where(mask, 0.0, d)
        share = float((d > 0).mean())
        assert d.max() <= 1.0, "%s: u8 image differs from rint(plain) by %d grey levels (%d pixels by more than one)" % (
            what, int(d.max()), int((d > 1).sum()))
    return ratio, share


@pytest.mark.parametrize("W,H,sigma,pol", ACC_CASES)
def test_ev2im_gauss_against_plain(oracle, W, H, sigma, pol):
    ev = acc_events(W, H)
    of, ou, omm = oracle.ev2im_gauss(ev, W, H, sigma, pol, True)
    what = "%dx%d sigma %.1f pol %d" % (W, H, sigma, pol)
    ratio, share = check_accumulation(what, of, omm, ou, acc_plain(W, H, sigma, pol))
    print("%s: worst |oracle - plain| / bound %.4f, u8 pixels != rint(plain) %.5f" % (what, ratio, share))
    for wrong in ("radius", "swap"):
        with pytest.raises(AssertionError):
            check_accumulation(what, of, omm, None, acc_plain(W, H, sigma, pol, wrong))
    with pytest.raises(AssertionError, match="u8 image"):
        bad = acc_plain(W, H, sigma, pol, "swap")
        check_accumulation(what, bad["img"].astype(np.float32), None, ou, bad)          # (passes the float check by construction)


# ---------------------------------------------------------------------------------------------------
# warps and motion-compensated images
WARP_CAMS = {"pinhole": (EVETHZ_CAM, 240, 180), "kb8": (MVSEC_KB8, 346, 260)}
_AXIS = np.array([0.1, -0.2, 0.97]); _AXIS = _AXIS / np.linalg.norm(_AXIS)
WARP_MOTIONS = {       # name: (group, arguments)
    "se3_median": ("se3", dict(angle=0.031, axis=tuple(_AXIS.tolist()), t=(0.012, -0.008, 0.004), medDepth=1.7, per_event=False)),
    "se3_per_event": ("se3", dict(angle=-0.045, axis=tuple(_AXIS.tolist()), t=(-0.01, 0.006, 0.003), medDepth=1.4, per_event=True)),
    "se2_3": ("se2", [0.02, 0.03, -0.02]),
    "se2_4": ("se2", [-0.015, 0.02, 0.01, 0.97]),
}
WARP_CASES = [(c, m) for c in sorted(WARP_CAMS) for m in sorted(WARP_MOTIONS)]
MCI_SIGMA = 1.0


@functools.lru_cache(maxsize=None)
def warp_events(camname):
    """4 000 events: fractional positions over the whole image, irregular increasing time stamps"""
    _, W, H = WARP_CAMS[camname]
    rng = np.random.default_rng(W)
    n = 4000
    ev = np.zeros(n, synth.EVENT_DTYPE)
    ev["x"] = rng.uniform(0, W - 1, n).astype(np.float32); ev["y"] = rng.uniform(0, H - 1, n).astype(np.float32)
    ev["ts"] = 12.5 + np.cumsum(rng.uniform(1e-6, 9e-6, n))
    ev["p"] = rng.integers(0, 2, n).astype(np.uint8)
    depth = rng.uniform(0.8, 3.0, n).astype(np.float32)
    ev.flags.writeable = False; depth.flags.writeable = False
    return ev, depth


@functools.lru_cache(maxsize=None)
def warp_plain(camname, motion, wrong=None):
    cam = cam64(WARP_CAMS[camname][0])
    ev, depth = warp_events(camname)
    group, m = WARP_MOTIONS[motion]
    if group == "se3":
        return pr.warp_se3(ev, cam, m["angle"], m["axis"], m["t"], depth.astype(F64) if m["per_event"] else F64(np.float32(m["medDepth"])), wrong)
    return pr.warp_se2(ev, cam, np.asarray(m, np.float32).astype(F64), wrong)


def warp_oracle(oracle, camname, motion):
    cam = WARP_CAMS[camname][0]
    ev, depth = warp_events(camname)
    group, m = WARP_MOTIONS[motion]
    if group == "se3":
        return oracle.mci_warp_se3(ev, cam, m["angle"], m["axis"], m["t"], m["medDepth"], depth if m["per_event"] else None)
    return oracle.mci_warp_se2(ev, cam, m)


def uv_tolerance(camname, motion):
    return FACTOR * MEASURED[("uv", camname, WARP_MOTIONS[motion][0])]


def check_uv(what, uv, plain, tol):
    d = np.abs(uv.astype(F64) - plain)
    k = np.unravel_index(np.argmax(d), d.shape)
    assert d[k] <= tol, "%s: warped position of event %d differs by %.3g px (allowed %.3g): %s, plain %s" % (what, k[0], d[k], tol, uv[k[0]], plain[k[0]])
    return float(d[k])


@pytest.mark.parametrize("camname,motion", WARP_CASES)
def test_warp_against_plain(oracle, camname, motion):
    uv = warp_oracle(oracle, camname, motion)
    what = "%s %s" % (camname, motion)
    worst = check_uv(what, uv, warp_plain(camname, motion), uv_tolerance(camname, motion))
    print("%s: worst |oracle uv - plain uv| %.3g px" % (what, worst))
    _, W, H = WARP_CAMS[camname]
    inside = (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)
    assert inside.mean() > 0.9 and np.abs(uv - np.stack([warp_events(camname)[0][k] for k in ("x", "y")], axis=1)).max() > 2.0     # (the warp moves)
    with pytest.raises(AssertionError):
        check_uv(what, uv, warp_plain(camname, motion, "rate"), uv_tolerance(camname, motion))


@functools.lru_cache(maxsize=None)
def mci_plain(camname, motion, pol, wrong=None):
    """gauss_image of the plain warp, the mask of the pixels an event near an integer position may legitimately move (its floor
    may differ between float32 and float64: the (2h + 2)^2 pixels either stamp covers), and the slack M G delta."""
    _, W, H = WARP_CAMS[camname]
    ev, _ = warp_events(camname)
    uv = warp_plain(camname, motion, wrong)
    ref = pr.gauss_image(ev, W, H, MCI_SIGMA, pol, xy=uv)
    delta = np.sqrt(2.0) * uv_tolerance(camname, motion)
    h = ref["h"]
    near = np.abs(uv - np.rint(uv)) <= delta
    mask = np.zeros((H, W), bool)
    for k in np.nonzero(near.any(axis=1))[0]:
        lo = [int(np.rint(uv[k, a])) - 1 - h if near[k, a] else int(np.floor(uv[k, a])) - h for a in (0, 1)]
        hi = [int(np.rint(uv[k, a])) + h if near[k, a] else int(np.floor(uv[k, a])) + h for a in (0, 1)]
        mask[max(lo[1], 0):max(hi[1] + 1, 0), max(lo[0], 0):max(hi[0] + 1, 0)] = True
    return ref, mask, ref["M"] * pr.stamp_slope(MCI_SIGMA) * delta


def mci_call(conv_se3, conv_se2, camname, motion, pol):
    """one motion-compensated image through an ev2mci_se3 / ev2mci_se2 pair with the oracle's argument order"""
    cam, W, H = WARP_CAMS[camname]
    ev, depth = warp_events(camname)
    group, m = WARP_MOTIONS[motion]
    if group == "se3":
        return conv_se3(ev, cam, m["angle"], m["axis"], m["t"], m["medDepth"], W, H, MCI_SIGMA, pol, False, depth if m["per_event"] else None)
    return conv_se2(ev, cam, m, W, H, MCI_SIGMA, pol, False)


def check_mci(what, f32, camname, motion, pol, wrong=None):
    ref, mask, slack = mci_plain(camname, motion, pol, wrong)
    assert mask.mean() <= 0.02, "%s: %.4f of the pixels masked" % (what, mask.mean())
    ratio, _ = check_accumulation(what, f32, None, None, ref, mask=mask, extra=slack)
    return ratio, float(mask.mean())


@pytest.mark.parametrize("camname,motion", WARP_CASES)
def test_motion_compensated_image_against_plain(oracle, camname, motion):
    pol = motion in ("se3_per_event", "se2_4")
    f32, _, _ = mci_call(lambda *a: oracle.ev2mci_se3(*a[:-1], depth=a[-1]), oracle.ev2mci_se2, camname, motion, pol)
    what = "%s %s" % (camname, motion)
    ratio, masked = check_mci(what, f32, camname, motion, pol)
    print("%s: worst |oracle - plain| / bound %.4f, %.4f of the pixels masked" % (what, ratio, masked))
    with pytest.raises(AssertionError):
        check_mci(what, f32, camname, motion, pol, "rate")


# ---------------------------------------------------------------------------------------------------
# focus and cv::normalize
@functools.lru_cache(maxsize=None)
def focus_image():
    """an accumulated 97 x 71 image (float32, not normalised): four 30-px tiles by three, the last ones cut"""
    W, H = 97, 71
    ev = synth.shapes_events(3000, W, H, seed=97, motion=0.5)
    rng = np.random.default_rng(97)
    x = ev["x"] + rng.uniform(0, 1, len(ev)).astype(np.float32); y = ev["y"] + rng.uniform(0, 1, len(ev)).astype(np.float32)
    img = pr.gauss_image(ev, W, H, 1.0, True, xy=np.stack([x, y], axis=1).astype(F64))["img"].astype(np.float32)
    img.flags.writeable = False
    return img


def focus_images():
    """the image, the image upside down (other tiles are cut) and its absolute value"""
    img = focus_image()
    return [img, np.ascontiguousarray(img[::-1]), np.abs(img)]


def check_focus(what, got, img, wrong=None):
    want = pr.focus(img, wrong)
    tol = FACTOR * MEASURED["focus"]
    assert abs(F64(got) - want) <= tol, "%s: focus %.9g, plain %.9g (allowed %.3g)" % (what, got, want, tol)
    return abs(F64(got) - want)


def check_minmax_u8(what, got, img, wrong=None):
    d = np.abs(got.astype(F64) - pr.minmax_u8(img, wrong))
    assert d.max() <= 1.0, "%s: %d pixels differ from the plain grey level by more than one" % (what, int((d > 1).sum()))
    return float((d > 0).mean())


def test_focus_and_normalize_against_plain(oracle):
    img = focus_image()
    assert img.min() < 0 < img.max()
    for k, im in enumerate(focus_images()):
        worst = check_focus("oracle", oracle.measure_image_focus(im), im)
        share = check_minmax_u8("oracle", oracle.cv_normalize_minmax_u8(im), im)
        print("image %d: focus |oracle - plain| %.3g (value %.6g); cv::normalize: %.5f of the pixels != plain" % (k, worst, pr.focus(im), share))
        with pytest.raises(AssertionError):
            check_focus("oracle", oracle.measure_image_focus(im), im, "sample")
    with pytest.raises(AssertionError):
        check_minmax_u8("oracle", oracle.cv_normalize_minmax_u8(img), img, "range")
    flat = np.full((7, 5), 3.25, np.float32)
    assert (oracle.cv_normalize_minmax_u8(flat) == 0).all() and (pr.minmax_u8(flat) == 0).all()


# ---------------------------------------------------------------------------------------------------
# IC_Angle and rBRIEF
ORB_CONFIGS = [(173, 131, 3, 1.2, 19), (241, 181, 4, 1.2, 19)]          # W, H, nlevels, scaleFactor, edgeTh: rows of tests/test_gpu_stages.py
ORB_MARGIN = 20            # the turned pattern reaches ceil(13 sqrt 2) = 19 px; nearer keypoints read wrapped pixels (H4) and stay with the bit tests
PATTERN = pr.load_pattern()


def orb_image(kind, W, H):
    return synth.texture_image(W, H, seed=W) if kind == "texture" else np.random.default_rng(W).integers(0, 256, (H, W), dtype=np.uint8)


def check_orientation_and_descriptors(what, kps, desc, scale, E, pyr, blur, wrong=None):
    """kps, desc: an extraction's output; scale: the scale factor of every level; pyr / blur: the bordered and the blurred buffer of
    every level that the same extraction produced.  Every keypoint at least ORB_MARGIN px from each edge of its level: the angle against
    ic_angle within FACTOR x measured and below the 0.3 degrees OpenCV documents for fastAtan2; every unmasked descriptor bit
    against rbrief.  Returns (worst angle deviation, bits compared, share masked, share of keypoints that qualified)."""
    umax = pr.circle_umax()
    tol = FACTOR * MEASURED["ic_angle"]
    worst, nbits, nmasked, nq, per_level = 0.0, 0, 0, 0, [0] * len(pyr)
    for i, kp in enumerate(kps):
        l = int(kp["octave"])
        fx, fy = F64(kp["x"]) / F64(scale[l]), F64(kp["y"]) / F64(scale[l])
        x, y = int(np.rint(fx)), int(np.rint(fy))
        assert abs(fx - x) < 1e-3 and abs(fy - y) < 1e-3, "%s: keypoint %d is not at a pixel of level %d: (%.5f, %.5f)" % (what, i, l, fx, fy)
        h, w = blur[l].shape
        if not (ORB_MARGIN <= x <= w - 1 - ORB_MARGIN and ORB_MARGIN <= y <= h - 1 - ORB_MARGIN):
            continue
        nq += 1; per_level[l] += 1
        if wrong != "angle":
            want = pr.ic_angle(pyr[l], x + E, y + E, umax, wrong)
            d = abs((F64(kp["angle"]) - want + 180.0) % 360.0 - 180.0)
            assert d <= tol and d < 0.3, "%s: keypoint %d (level %d, %d, %d): angle %.5f, plain %.5f" % (what, i, l, x, y, kp["angle"], want)
            worst = max(worst, d)
        if wrong != "umax":
            bits, mask = pr.rbrief(blur[l], x, y, kp["angle"], PATTERN, wrong)
            diff = np.unpackbits(bits ^ desc[i], bitorder="little").astype(bool) & ~mask
            assert not diff.any(), "%s: keypoint %d (level %d, %d, %d, %.3f deg): %d unmasked descriptor bits differ, first %d" % (
                what, i, l, x, y, kp["angle"], int(diff.sum()), int(np.argmax(diff)))
            nbits += 256; nmasked += int(mask.sum())
    assert nq >= 0.9 * len(kps), "%s: only %d of %d keypoints qualify" % (what, nq, len(kps))
    assert min(per_level) >= 20, "%s: keypoints per level %s" % (what, per_level)
    assert nmasked <= 0.01 * max(nbits, 1), "%s: %d of %d bits masked" % (what, nmasked, nbits)
    return worst, nbits, nmasked / max(nbits, 1), nq / len(kps)


def test_umax_is_the_circle(oracle):
    assert oracle.OrbExtractor().umax == pr.circle_umax() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


@pytest.mark.parametrize("kind", ["texture", "noise"])
@pytest.mark.parametrize("W,H,nl,sf,E", ORB_CONFIGS)
def test_orientation_and_descriptors_against_plain(oracle, W, H, nl, sf, E, kind):
    img = orb_image(kind, W, H)
    oe = oracle.OrbExtractor(1000, sf, nl, 10, 0, edgeTh=E, imWidth=W)
    mono, kps, desc, _ = oe.extract(img)
    assert mono >= 0 and len(kps) > 100
    lk_ = [oe.level_keypoints(l) for l in range(nl)]
    assert sum(len(k) for k in lk_) == len(kps)
    pyr = [oe.level_buffer(l) for l in range(nl)]; blur = [oe.level_blur(l) for l in range(nl)]
    what = "%dx%d %s" % (W, H, kind)
    args = (what, kps, desc, oe.scale_factors, E, pyr, blur)
    worst, nbits, masked, share = check_orientation_and_descriptors(*args)
    print("%s: worst |angle - plain| %.5f deg, %d descriptor bits equal, %.5f masked, %.3f of %d keypoints qualify" % (
        what, worst, nbits, masked, share, len(kps)))
    for wrong in ("umax", "angle"):
        with pytest.raises(AssertionError, match="angle" if wrong == "umax" else "descriptor bits"):
            check_orientation_and_descriptors(*args, wrong=wrong)


# ---------------------------------------------------------------------------------------------------
# Lucas-Kanade
LK_W, LK_H = 112, 88
LK_SHIFTS = [(1.3, -0.7), (2.6, 1.9)]
LK_PARAMS = [(23, 1), (15, 2), (9, 2)]
LK_COUNT, LK_EPS = 10, 0.03
# amplitude, period (px), direction, phase.  The periods: at most twice the smallest window (9 px), so that every window holds half a
# period of every wave, and at least 2.75 px on the coarsest level (/ 4), above its Nyquist period of 2 px
_LK_WAVES = [(45.0, 11.0, 0.35, 0.4), (35.0, 14.0, 1.9, 1.1), (30.0, 18.0, 2.8, 2.3)]


def lk_image(shift=(0.0, 0.0)):
    """127.5 + three sinusoids, the content moved by `shift` and sampled at the pixel centres, rounded to u8"""
    yy, xx = np.mgrid[0:LK_H, 0:LK_W].astype(F64)
    xx = xx - shift[0]; yy = yy - shift[1]
    v = 127.5 + sum(a * np.sin(2 * np.pi * (xx * np.cos(d) + yy * np.sin(d)) / p + ph) for a, p, d, ph in _LK_WAVES)
    return np.rint(v).astype(np.uint8)


def lk_points(win, maxLevel):
    """A 6 x 4 grid at fractional positions whose windows, moved ones included, stay inside the image on every level.  (On 112 x 88 a
    23-px window cannot keep a margin of another 23 px on the 56 x 44 level: 2 px are kept, so that no border rule is read.)"""
    s = 1 << maxLevel
    m = s * ((win - 1) / 2.0 + 2.0) + 3.0
    xs = np.linspace(m, LK_W - 1 - m, 6) + 0.37; ys = np.linspace(m, LK_H - 1 - m, 4) + 0.21
    return np.array([[x, y] for y in ys for x in xs], np.float32)


@functools.lru_cache(maxsize=None)
def lk_plain(win, maxLevel, shift, wrong=None):
    return pr.lk(lk_image(), lk_image(shift), lk_points(win, maxLevel), win, maxLevel, LK_COUNT, LK_EPS, wrong=wrong)


def check_lk(what, nxt, status, win, maxLevel, shift, wrong=None):
    want, wst = lk_plain(win, maxLevel, shift, wrong)
    pts = lk_points(win, maxLevel).astype(F64)
    assert len(pts) >= 24 and status.tolist() == [1] * len(pts) and wst.tolist() == [1] * len(pts), "%s: status %s, plain %s" % (what, status.tolist(), wst.tolist())
    d = np.abs(nxt.astype(F64) - want).max(axis=1)
    tol = FACTOR * MEASURED["lk"]
    assert d.max() <= tol, "%s: point %d differs from the plain tracker by %.4f px (allowed %.4f)" % (what, int(np.argmax(d)), d.max(), tol)
    truth = pts + np.asarray(shift)
    e_got, e_plain = np.abs(nxt.astype(F64) - truth).max(), np.abs(want - truth).max()
    assert e_got <= 0.05 and e_plain <= 0.05, "%s: distance from the true translation %.4f px, plain %.4f px" % (what, e_got, e_plain)
    return float(d.max()), float(np.median(d)), float(e_got), float(e_plain)


@pytest.mark.parametrize("shift", LK_SHIFTS)
@pytest.mark.parametrize("win,maxLevel", LK_PARAMS)
def test_pyr_lk_against_plain(oracle, win, maxLevel, shift):
    nxt, st, _ = oracle.calc_optical_flow_pyr_lk(lk_image(), lk_image(shift), lk_points(win, maxLevel), None, win, maxLevel, LK_COUNT, LK_EPS, 0)
    what = "win %d maxLevel %d shift %s" % (win, maxLevel, shift)
    worst, med, e_got, e_plain = check_lk(what, nxt, st, win, maxLevel, shift)
    print("%s: |oracle - plain| worst %.5f median %.5f px; from the truth: oracle %.4f, plain %.4f px" % (what, worst, med, e_got, e_plain))
    with pytest.raises(AssertionError):
        check_lk(what, nxt, st, win, maxLevel, shift, "scharr")
