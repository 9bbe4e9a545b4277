"""Non-finite and out-of-range inputs at the float-to-index steps: the case tables and the expected values that follow from THE RULE.

The rule.  The reference on x86-64 is the specification: the conversion of NaN, +-inf or a value outside int32 to an index yields
INT_MIN (cvttss2si / cvtss2si: what the reference binary, OpenCV's cvFloor / cvRound and the oracle execute), and whatever the
reference's next comparison does with INT_MIN is the expected result -- an event contributes nothing, a point gets status 0.
gfx950's v_cvt_i32_f32 saturates instead and turns NaN into 0; C++ leaves the cast undefined, so nothing but these tests pins it.

Everything here is Python integers and float64 (float32 values are exact in float64; np.float32(...) only rounds a float64 to the
float32 a kernel would hold): no float-to-int cast of the kind under test.  Every conversion takes `wrong=`, a named wrong variant
the tests must be able to tell from the rule:
    "saturate"   NaN -> 0, values beyond int32 -> INT_MAX / INT_MIN  (the bare device conversion)
    "half_even"  ties of the count form's roundf go to the even neighbour  (v_rndne_f32 / rint in place of roundf)
    "alias16"    the index keeps its low 16 bits as an int16  (65546 -> column 10)
tests/test_oracle_edges.py holds the oracle to these expectations, tests/test_gpu_edges.py the kernels."""
import functools
import math

import numpy as np

from eorb_slam_amd import synth
import plain_ref as pr
import test_oracle_plain as op                  # (the accumulation, focus and warp checks and their inputs)

F64 = np.float64
NAN, INF = float("nan"), float("inf")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
WRONG = ("saturate", "half_even", "alias16")

SIZES = [(61, 45), (240, 180)]


def f32(v):
    """the float32 nearest to v, as a Python float"""
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------
# the conversions
def to_index(v, wrong=None):
    """v: an integral float64 (the result of floor / round), NaN or +-inf -> the int32 the rule prescribes"""
    if v != v:
        return 0 if wrong == "saturate" else INT_MIN
    if not (-2.0 ** 31 <= v < 2.0 ** 31):
        return (INT_MAX if v > 0 else INT_MIN) if wrong == "saturate" else INT_MIN
    i = int(v)                                           # exact: v is integral and inside int32
    if wrong == "alias16":
        i = (i + 32768) % 65536 - 32768
    return i


def floor_index(x, wrong=None):
    """(int)floorf(x), (int)floor((double)x), cvFloor"""
    x = float(x)
    return to_index(math.floor(x) if math.isfinite(x) else x, wrong)


def round_index(x, wrong=None):
    """(int)roundf(x): halves away from zero (roundFloatCoord).  "half_even": to the even neighbour."""
    x = float(x)
    if not math.isfinite(x):
        return to_index(x, wrong)
    if wrong == "half_even":
        return to_index(float(round(x)), wrong)          # Python's round() of a float is round-half-even
    return to_index(math.copysign(math.floor(abs(x) + 0.5), x), wrong)


# ---------------------------------------------------------------------------------------------------
# the value set of a coordinate
SPECIALS = [
    ("nan", NAN), ("+inf", INF), ("-inf", -INF), ("+3e9", 3e9), ("-3e9", -3e9), ("+1e30", f32(1e30)), ("-1e30", f32(-1e30)),
    ("+2^31", 2147483648.0), ("-2^31", -2147483648.0), ("2^31-128", 2147483520.0),          # the largest float below 2^31
    ("65546.25", 65546.25), ("-65525.75", -65525.75),                                        # column 10 in 16 bits
    ("32778.25", 32778.25), ("-32757.75", -32757.75), ("-32768", -32768.0),                  # column 10 as int16; the "dropped" mark
    ("+1e-40", f32(1e-40)), ("-1e-40", f32(-1e-40)),                                         # floor(-1e-40) = -1; flushed: 0
    ("-0.0", -0.0),
]
assert all(f32(v) == v or v != v for _, v in SPECIALS) and f32(1e-40) != 0.0


def axis_values(L, h):
    """V for one axis of length L and a stamp (or window) half width h: the specials, then the positions whose stamp just misses
    and just reaches each end"""
    return SPECIALS + [("-h-1", float(-h - 1)), ("-h", float(-h)), ("L-1+h", float(L - 1 + h)), ("L+h", float(L + h))]


def interleave(ordinary, special):
    """every special entry between ordinary ones: ordinary[i] is followed by special[i::n]"""
    n = len(ordinary)
    out, is_special = [], []
    for i in range(n):
        out.append(ordinary[i]); is_special.append(False)
        for s in special[i::n]:
            out.append(s); is_special.append(True)
    return out, np.array(is_special)


# ---------------------------------------------------------------------------------------------------
# family 1: accumulation
N_ORDINARY = 64


@functools.lru_cache(maxsize=None)
def ordinary_xy(W, H):
    """64 fractional positions inside the image, a few of them near its edges (their stamps are cut)"""
    rng = np.random.default_rng(7 * W + H)
    xy = np.stack([rng.uniform(0.0, W - 0.01, N_ORDINARY), rng.uniform(0.0, H - 0.01, N_ORDINARY)], axis=1)
    xy[:4] = [(0.3, 0.6), (W - 0.7, 0.2), (0.9, H - 0.4), (W - 0.2, H - 0.8)]
    xy = xy.astype(np.float32).astype(F64)
    xy.flags.writeable = False
    return xy


def edge_positions(W, H, h):
    """[(name, x, y)]: every value of V in x (at an ordinary y), in y (at an ordinary x) and in both; the four corners, reaching and
    missing"""
    o = ordinary_xy(W, H)
    vx, vy = axis_values(W, h), axis_values(H, h)
    out = []
    for k, (name, v) in enumerate(vx):
        out.append(("x=" + name, v, float(o[(3 * k) % N_ORDINARY][1])))
    for k, (name, v) in enumerate(vy):
        out.append(("y=" + name, float(o[(3 * k + 1) % N_ORDINARY][0]), v))
    for (name, a), (_, b) in zip(vx, vy):
        out.append(("xy=" + name, a, b))
    for cx, nx in ((-h, "l"), (W - 1 + h, "r")):
        for cy, ny in ((-h, "t"), (H - 1 + h, "b")):
            out.append(("corner " + ny + nx, float(cx), float(cy)))
            out.append(("corner " + ny + nx + " missing x", float(cx + (-1 if cx < 0 else 1)), float(cy)))
            out.append(("corner " + ny + nx + " missing y", float(cx), float(cy + (-1 if cy < 0 else 1))))
    return out


def reaches(x, y, W, H, h, count=False, wrong=None):
    """Does an event at (x, y) write a pixel?  breakFloatCoords + the stamp loop's isInImage (h = ceil(3 sigma)), or, for the count
    form, roundFloatCoord + isInImage (h = 0).  Returns the integer position when it does, else None."""
    conv = round_index if count else floor_index
    xi, yi = conv(x, wrong), conv(y, wrong)
    if xi + h < 0 or xi - h > W - 1 or yi + h < 0 or yi - h > H - 1:
        return None
    return xi, yi


def make_events(xy, pol_seed=3):
    xy = np.asarray(xy, F64).reshape(-1, 2)
    ev = np.zeros(len(xy), synth.EVENT_DTYPE)
    ev["x"] = xy[:, 0].astype(np.float32); ev["y"] = xy[:, 1].astype(np.float32)
    ev["ts"] = np.arange(len(xy)) * 1e-6
    ev["p"] = np.random.default_rng(pol_seed).integers(0, 2, len(xy)).astype(np.uint8)
    return ev


@functools.lru_cache(maxsize=None)
def acc_case(W, H, h, count=False):
    """(all events, is_special mask, names of the special ones): the ordinary events with the edge positions between them"""
    pos = edge_positions(W, H, h)
    merged, special = interleave([("", float(x), float(y)) for x, y in ordinary_xy(W, H)], pos)
    ev = make_events([(x, y) for _, x, y in merged])
    ev.flags.writeable = False
    return ev, special, [n for n, _, _ in merged]


def acc_expected_events(ev, W, H, h, count=False, wrong=None):
    """The events that reach the frame according to the rule, in order.  Under a wrong variant an event whose index differs from
    the rule's is moved to the integer position that variant would write to."""
    keep = np.zeros(len(ev), bool)
    out = ev.copy()
    for k in range(len(ev)):
        x, y = float(ev["x"][k]), float(ev["y"][k])
        r = reaches(x, y, W, H, h, count, wrong)
        if r is None:
            continue
        keep[k] = True
        if wrong is not None and r != reaches(x, y, W, H, h, count):
            out["x"][k], out["y"][k] = r
    return out[keep], keep


# ---------------------------------------------------------------------------------------------------
# family 2: raw sensor events through undistortion maps
@functools.lru_cache(maxsize=None)
def raw_case(W, H, h):
    """(mapX, mapY, raw events, is_special mask): W x H maps, a shifted identity, in which chosen sensor pixels map to the edge
    positions of family 1; 64 events at ordinary pixels with one event at every chosen pixel between them"""
    yy, xx = np.mgrid[0:H, 0:W]
    mx = (xx + 0.31).astype(np.float32); my = (yy + 0.17).astype(np.float32)
    mx[:, W - 1] = W - 0.5; my[H - 1, :] = H - 0.5                           # (the shift keeps the last column and row inside)
    pos = edge_positions(W, H, h)
    chosen = [(11 * j + 3) % (W * H) for j in range(len(pos))]
    assert len(set(chosen)) == len(pos)
    for c, (_, x, y) in zip(chosen, pos):
        mx[c // W, c % W] = x; my[c // W, c % W] = y
    rng = np.random.default_rng(W + 5 * H)
    free = np.setdiff1d(np.arange(W * H), chosen)
    ordinary = rng.choice(free, N_ORDINARY, replace=False)
    merged, special = interleave([int(c) for c in ordinary], [int(c) for c in chosen])
    raw = np.zeros(len(merged), synth.RAW_DTYPE)
    raw["x"] = np.array(merged) % W; raw["y"] = np.array(merged) // W
    raw["p"] = rng.integers(0, 2, len(merged)); raw["t"] = np.arange(len(merged)) * 1e-6
    for a in (mx, my, raw):
        a.flags.writeable = False
    return mx, my, raw, special


def raw_expected_events(mx, my, raw, W, H, check):
    """getEventChunkRectified by hand: the maps' entries as the events' positions; with checkInImage only those with
    0 <= x < W and 0 <= y < H (a NaN fails every comparison)"""
    x = mx[raw["y"], raw["x"]].astype(F64); y = my[raw["y"], raw["x"]].astype(F64)
    keep = ((x >= 0) & (x < W) & (y >= 0) & (y < H)) if check else np.ones(len(raw), bool)
    ev = np.zeros(int(keep.sum()), synth.EVENT_DTYPE)
    ev["x"] = x[keep].astype(np.float32); ev["y"] = y[keep].astype(np.float32)
    ev["ts"] = raw["t"][keep]; ev["p"] = raw["p"][keep] != 0
    return ev


def same_events(a, b):
    return len(a) == len(b) and same_f32(a["x"], b["x"]) and same_f32(a["y"], b["y"]) and np.array_equal(a["ts"], b["ts"]) and np.array_equal(a["p"], b["p"])


# ---------------------------------------------------------------------------------------------------
# family 3: motion-compensated images.  name -> (group, camera, events, arguments); the cameras and the ordinary events are those of
# tests/test_oracle_plain.py (passed in: this module does not import a test module)
MCI_SIGMA = 1.0


def mci_cases(cams, events):
    """cams: name -> (camera tuple, W, H); events(name) -> (events, per-event depths)"""
    axis = (0.1 / 0.99549, -0.2 / 0.99549, 0.97 / 0.99549)
    out = {}
    for cn in sorted(cams):
        cam, W, H = cams[cn]
        ev = events(cn)[0][:200].copy()
        se3 = lambda d, e=ev: ("se3", cn, e, dict(angle=0.031, axis=axis, t=(0.012, -0.008, 0.004), medDepth=d))
        for name, d in (("depth 0", 0.0), ("depth -1", -1.0), ("depth 1e-30", 1e-30), ("depth nan", NAN)):
            out["%s se3 %s" % (cn, name)] = se3(d)
        out["%s se3 one event" % cn] = se3(1.7, ev[:1].copy())
        same = ev.copy(); same["ts"] = 12.5
        out["%s se3 one time stamp" % cn] = se3(1.7, same)
        out["%s se2 one event" % cn] = ("se2", cn, ev[:1].copy(), [0.02, 0.03, -0.02])
        out["%s se2 one time stamp" % cn] = ("se2", cn, same, [0.02, 0.03, -0.02, 0.97])
        out["%s se2 scale 0" % cn] = ("se2", cn, ev, [0.02, 0.03, -0.02, 0.0])
        if len(cam) > 4:
            # pixels whose |m| = |((x - cx) / fx, (y - cy) / fy)| passes pi / 2, where KannalaBrandt8::unproject clamps theta_d
            far = ev.copy()
            far["x"][1::2] = np.float32(cam[2] + cam[0] * 1.7); far["y"][1::4] = np.float32(cam[3] - cam[1] * 2.5)
            out["%s se3 past the clamp" % cn] = se3(1.7, far)
            out["%s se2 past the clamp" % cn] = ("se2", cn, far, [0.02, 0.03, -0.02])
    return out


def events_at(ev, uv):
    """the events moved to their warped positions"""
    out = ev.copy()
    out["x"] = uv[:, 0]; out["y"] = uv[:, 1]
    return out


# the count form's exact ties: x -> the expected column (None: dropped), W being the image width
def count_ties(W):
    return [(0.5, 1), (1.5, 2), (2.5, 3), (-0.5, None), (W - 0.5, None), (W - 1.5, W - 1)]


# ---------------------------------------------------------------------------------------------------
# family 4: pyramidal Lucas-Kanade
LK_W, LK_H, LK_WIN, LK_MAXLEVEL, LK_COUNT, LK_EPS = 61, 45, 9, 2, 10, 0.03
LK_HALF = (LK_WIN - 1) * 0.5
_LK_WAVES = [(45.0, 11.0, 0.35, 0.4), (35.0, 14.0, 1.9, 1.1), (30.0, 18.0, 2.8, 2.3)]      # amplitude, period (px), direction, phase


@functools.lru_cache(maxsize=None)
def lk_image(shift=0.0):
    """127.5 + three sinusoids, the content moved by `shift` px in x"""
    yy, xx = np.mgrid[0:LK_H, 0:LK_W].astype(F64)
    xx = xx - shift
    v = 127.5 + sum(a * np.sin(2 * np.pi * (xx * np.cos(d) + yy * np.sin(d)) / p + ph) for a, p, d, ph in _LK_WAVES)
    img = np.rint(v).astype(np.uint8)
    img.flags.writeable = False
    return img


def lk_level_sizes():
    """buildOpticalFlowPyramid: halve while both sides stay above the window"""
    w, h, out = LK_W, LK_H, []
    for _ in range(LK_MAXLEVEL + 1):
        out.append((w, h))
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= LK_WIN or h <= LK_WIN:
            break
    return out


@functools.lru_cache(maxsize=None)
def lk_ordinary():
    """an 8 x 8 grid of points whose windows stay inside the image on every level"""
    m = 4 * (LK_HALF + 2.0) - 6.0
    xs = np.linspace(m, LK_W - 1 - m, 8) + 0.37; ys = np.linspace(m, LK_H - 1 - m, 8) + 0.21
    pts = np.array([[x, y] for y in ys for x in xs], np.float32)
    pts.flags.writeable = False
    return pts


def lk_window_index(v, level, wrong=None):
    """the corner of a point's window on a level: floor of float32(float32(v * 2^-level) - halfWin)"""
    scaled = float(np.float32(np.float32(v) * np.float32(1.0 / (1 << level))))
    return floor_index(float(np.float32(np.float32(scaled) - np.float32(LK_HALF))), wrong)


def lk_accepted(x, y, level, wrong=None):
    """the window test of lkpyramid.cpp on a level: rejected when ipx < -win || ipx >= w || ipy < -win || ipy >= h"""
    w, h = lk_level_sizes()[level]
    ix, iy = lk_window_index(x, level, wrong), lk_window_index(y, level, wrong)
    return not (ix < -LK_WIN or ix >= w or iy < -LK_WIN or iy >= h)


def lk_inside(x, y, level, wrong=None):
    """the window lies wholly inside the level's image (the derivative image is zero outside it: a window in the padding has no
    gradient and is given up like a flat one)"""
    w, h = lk_level_sizes()[level]
    ix, iy = lk_window_index(x, level, wrong), lk_window_index(y, level, wrong)
    return 0 <= ix and ix + LK_WIN <= w and 0 <= iy and iy + LK_WIN <= h


def _around(b):
    b = np.float32(b)
    return [float(np.nextafter(b, np.float32(-np.inf))), float(b), float(np.nextafter(b, np.float32(np.inf)))]


def lk_boundary_values(L, level):
    """The last floats on each side of the window test of an axis of (level-0) length L, seen from level `level`:
    floor(v 2^-level - halfWin) = -win  <=>  v = 2^level (halfWin - win), and = l  <=>  v = 2^level (l + halfWin), l the level's length"""
    l = L
    for _ in range(level):
        l = (l + 1) // 2
    s = float(1 << level)
    return _around(s * (LK_HALF - LK_WIN)) + _around(s * (l + LK_HALF))


def lk_cases():
    """name -> (prevPts, initial flow or None, is_special mask).  The specials sit between the ordinary points."""
    o = lk_ordinary().astype(F64)
    vx, vy = axis_values(LK_W, LK_WIN), axis_values(LK_H, LK_WIN)
    gx, gy = float(o[27][0]), float(o[27][1])                                 # an ordinary point's coordinates for the other axis
    sets = {
        "x": [(v, gy) for _, v in vx],
        "y": [(gx, v) for _, v in vy],
        "xy": [(a, b) for (_, a), (_, b) in zip(vx, vy)],
        "boundary": [(v, gy) for lv in (0, LK_MAXLEVEL) for v in lk_boundary_values(LK_W, lv)] +
                    [(gx, v) for lv in (0, LK_MAXLEVEL) for v in lk_boundary_values(LK_H, lv)],
    }
    cases = {}
    for name, sp in sets.items():
        merged, mask = interleave([tuple(p) for p in o], sp)
        pts = np.array(merged, np.float32)
        cases["prev_" + name] = (pts, None, mask)
        if name != "boundary":
            good = np.where(mask[:, None], np.float32([gx, gy])[None, :], pts).astype(np.float32)
            cases["flow_" + name] = (good, pts, mask)                        # flags = 4: good prevPts, the value in the initial flow
    return cases


def same_f32(a, b):
    """bytes, except that a NaN equals any NaN (x86 makes 0xffc00000, the GPU 0x7fc00000)"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    an, bn = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(an, bn) and np.array_equal(a.view(np.uint32)[~an], b.view(np.uint32)[~bn]))


def check_lk_rule(what, case, nxt, status, err, plain, wrong=None):
    """A tracker's answer (nxt, status, err) for lk_cases()[case] against the rule.  `plain`: the same tracker's answer (nxt, status,
    err) for the ordinary points alone.

    * the ordinary points: what they are without the special ones between them, bytes (a wrong lane shows here)
    * a point whose level-0 window test fails: status 0, err 0
    * ... and fails on every level (NaN, +-inf, beyond int32, far outside): the point comes back untouched -- next = prevPts, or
      = the initial flow with flags = 4 (the per-level scaling by powers of two is exact)
    * a point whose window lies wholly inside the image on some level was processed there: it is not (status 0, err 0, untouched)
    * -0.0 and +-1e-40 in prevPts are the point at 0: its status, its position to 1e-5 px"""
    pts, flow, mask = lk_cases()[case]
    nlev = len(lk_level_sizes())
    assert same_f32(nxt[~mask], plain[0]) and np.array_equal(status[~mask], plain[1]) and same_f32(err[~mask], plain[2]), \
        "%s: the ordinary points differ from their run without the special ones" % what
    moving = pts if flow is None else flow                                   # what the tested value enters through
    for k in np.flatnonzero(mask):
        x, y = float(moving[k][0]), float(moving[k][1])
        acc = [lk_accepted(x, y, lv, wrong) for lv in range(nlev)]
        inside = any(lk_inside(x, y, lv, wrong) for lv in range(nlev))
        tag = "%s: point %d (%r, %r)" % (what, k, x, y)
        untouched = same_f32(nxt[k], moving[k])
        if flow is None:
            if not acc[0]:
                assert status[k] == 0 and err[k] == 0.0, "%s fails the level-0 window test: status %d err %r" % (tag, status[k], err[k])
            if not any(acc):
                assert untouched, "%s fails every window test but came back as %r" % (tag, nxt[k].tolist())
            elif inside:
                assert not (status[k] == 0 and err[k] == 0.0 and untouched), "%s has a window inside the image but was not processed" % tag
        else:
            # the flow's window test is the iteration's (inx, iny): it ends the iteration, at level 0 with status 0, and err is only
            # written after an iteration at level 0 that ran through.  A flow that passes the test on an upper level moves there, so
            # only a flow that fails on every level has a known answer
            if not any(acc):
                assert status[k] == 0 and err[k] == 0.0, "%s fails every window test: status %d err %r" % (tag, status[k], err[k])
                assert untouched, "%s fails every window test but came back as %r" % (tag, nxt[k].tolist())
            elif inside:
                assert not (status[k] == 0 and err[k] == 0.0 and untouched), "%s has a window inside the image but was not processed" % tag
    if flow is None and case in ("prev_x", "prev_y"):
        axis = 0 if case == "prev_x" else 1
        special = np.flatnonzero(mask)
        names = [n for n, _ in axis_values(LK_W if axis == 0 else LK_H, LK_WIN)]
        zero = special[names.index("-0.0")]
        for n in ("+1e-40", "-1e-40"):
            k = special[names.index(n)]
            assert status[k] == status[zero] and np.abs(nxt[k].astype(F64) - nxt[zero].astype(F64)).max() <= 1e-5, \
                "%s: %s is not the point at 0: status %d / %d, %r / %r" % (what, n, status[k], status[zero], nxt[k].tolist(), nxt[zero].tolist())


# ---------------------------------------------------------------------------------------------------
# family 5 (SearchForInitialization only): vbPrevMatched from V
INIT_W, INIT_H = 240, 180


def init_prev_matched(kps):
    """(vbPrevMatched, is_special, beyond): the keypoints' own positions as the search centres, with every special value in x, in y
    and in both, every fourth keypoint keeping its own position.  beyond: the centres that are NaN, +-inf or at least 2^31 in size -- farther than any
    window from every keypoint, whatever the conversion of their cell index gives."""
    pm = np.stack([kps["x"], kps["y"]], axis=1).astype(np.float32)
    special = np.zeros(len(kps), bool); beyond = np.zeros(len(kps), bool)
    k = 1
    for _, v in SPECIALS:
        for a in range(3):                                                       # x, y, both
            if a != 1: pm[k, 0] = v
            if a != 0: pm[k, 1] = v
            special[k] = True
            beyond[k] = not abs(v) < 2.0 ** 31
            k += 2 if k % 4 == 3 else 1                                          # (every fourth keypoint keeps its own position)
    assert k <= len(kps)
    return pm, special, beyond


def check_init_rule(what, run, kps):
    """run(vbPrevMatched, windowSize) -> (nmatches, vnMatches12, vbPrevMatched out).  A centre beyond every window finds nothing;
    the other keypoints match as they do when those centres are merely far away (1e6, 1e6); windowSize 0 finds nothing at all
    (GetFeaturesInArea keeps |dx| < r); with windowSize 1e9 the beyond centres still find nothing."""
    pm, special, beyond = init_prev_matched(kps)
    for ws in (100, 1000000000):
        n, m12, out = run(pm, ws)
        assert (m12[beyond] == -1).all(), "%s windowSize %d: centres %s found a match" % (what, ws, pm[beyond][m12[beyond] >= 0][:4].tolist())
        far = pm.copy(); far[beyond] = 1e6
        n2, m2, _ = run(far, ws) if ws == 100 else (n, m12, None)
        assert n == n2 and np.array_equal(m12, m2) and n == int((m12 >= 0).sum()), "%s windowSize %d: %d matches, %d with the centres far away" % (what, ws, n, n2)
        assert n > 20, (what, ws, n)
        assert same_f32(out[m12 < 0], pm[m12 < 0]), "%s: an unmatched centre was rewritten" % what
    n, m12, out = run(pm, 0)
    assert n == 0 and (m12 == -1).all() and same_f32(out, pm), "%s: windowSize 0 found %d matches" % (what, n)


def init_special_keypoints(k1, d1, k2, d2):
    """(kps, desc, outside): the searched frame of SearchForInitialization with a keypoint at every special position (x, y, both)
    between its own, each carrying the descriptor of a query keypoint of the other frame (it would win the match if the search could
    reach it).  outside: PosInGrid fails for it by the rule."""
    extra = np.zeros(3 * len(SPECIALS), k2.dtype); ed = np.zeros((len(extra), d2.shape[1]), np.uint8)
    for k, (_, v) in enumerate(SPECIALS):
        for a in range(3):
            e = extra[3 * k + a]; i = (3 * k + a) % len(k1)
            e["x"] = v if a != 1 else k1["x"][i]; e["y"] = v if a != 0 else k1["y"][i]
            e["size"] = k1["size"][i]; e["angle"] = k1["angle"][i]; e["octave"] = 0; e["class_id"] = -1
            ed[3 * k + a] = d1[i]
    order = np.random.default_rng(23).permutation(len(k2) + len(extra))
    kps = np.concatenate([k2, extra])[order]; desc = np.ascontiguousarray(np.concatenate([d2, ed])[order])
    class GB: minX, minY, invW, invH = 0.0, 0.0, GRID_COLS / INIT_W, GRID_ROWS / INIT_H
    outside = np.array([pos_in_grid(x, y, GB) is None for x, y in zip(kps["x"], kps["y"])])
    return kps, desc, outside


def check_init_keypoints_rule(what, run, k1, d1, k2, d2):
    """run(kps2, desc2) -> (nmatches, vnMatches12) of SearchForInitialization (window 100) from frame 1's own positions.  A keypoint
    outside the grid is never matched, and the others match as they do when those keypoints lie far away at (1e6, 1e6)."""
    kps, desc, outside = init_special_keypoints(k1, d1, k2, d2)
    assert outside.sum() >= 40 and (~outside).sum() > len(k2)                # (-0.0 and +-1e-40 are cell 0: inside)
    n, m12 = run(kps, desc)
    hit = m12[m12 >= 0]
    assert not outside[hit].any(), "%s: matched keypoints outside the grid at %s" % (what, kps[hit][outside[hit]][["x", "y"]].tolist()[:4])
    far = kps.copy(); far["x"][outside] = 1e6; far["y"][outside] = 1e6
    n2, m2 = run(far, desc)
    assert n == n2 and np.array_equal(m12, m2) and n > 20, "%s: %d matches, %d with the keypoints far away" % (what, n, n2)


# caller-fed projection queries: the centre uv from V, level_scale from RADII
def inject_queries(uv, ls):
    """(uv, level_scale, is_special): every special value in u, in v and in both (level scale 1), then every value of RADII as the
    level scale; every fourth query stays ordinary"""
    uv = np.array(uv, np.float32); ls = np.array(ls, np.float32); special = np.zeros(len(uv), bool)
    k = 1
    def step(k):
        return k + (2 if k % 4 == 3 else 1)
    for _, v in SPECIALS:
        for a in range(3):
            if a != 1: uv[k, 0] = v
            if a != 0: uv[k, 1] = v
            special[k] = True; k = step(k)
    for _, r in RADII:
        ls[k] = r; special[k] = True; k = step(k)
    assert k <= len(uv)
    return uv, ls, special


def check_projection_rule(what, run, uv0, ls0, gb, th, factor=1.0, query_of=None, wrong=None):
    """run(uv, level_scale, th) -> (nmatches, slots out, slots in): a window matcher whose radius is factor * th * level_scale and whose
    slot i2 receives the index of the query matched to keypoint i2.  A query whose area is empty by the rule is matched to nothing;
    the ordinary ones still match; with a threshold of PROJ_TH every area is empty."""
    uv, ls, special = inject_queries(uv0, ls0)
    with np.errstate(all="ignore"):
        empty = np.array([area_is_empty(float(u), float(v), float(np.float32(factor * th) * np.float32(l)), gb, wrong) for (u, v), l in zip(uv, ls)])
    assert (wrong is not None or empty[special].sum() >= 50) and not empty[~special].any()
    n, out, before = run(uv, ls, th)
    matched = out[(out >= 0) & (out != before)]
    q = matched if query_of is None else query_of(matched)
    assert not empty[q].any(), "%s: queries %s with an empty area were matched" % (what, np.unique(q[empty[q]])[:6].tolist())
    assert n > 10, (what, n)
    if wrong is not None:
        assert np.isin(np.flatnonzero(~empty & special & (ls > 1e8)), q).any(), "%s: no query with a whole-grid area was matched" % what
    for name, t in PROJ_TH:
        n, out, before = run(uv0, ls0, t)
        assert n == 0 and np.array_equal(out, before), "%s th %s: %d matches where every area is empty" % (what, name, n)


# tracked keypoints: ComputeTrackedKPtsDesc / AssignKPtLevelByBestDesc read the descriptor's taps at cvRound(pt * scale)
def cvround_index(v, wrong=None):
    """cvRound: to the nearest integer, ties to even (cvtsd2si), INT_MIN for NaN and beyond int32"""
    v = float(v)
    return to_index(float(round(v)) if math.isfinite(v) else v, wrong)


def tracked_keypoints(kps):
    """(keypoints, is_special, beyond): level-0 keypoints of an extraction with a keypoint at every special position (x, y, both)
    after every second one.  beyond: a coordinate converts to INT_MIN -- every tap of its descriptor lies outside the level."""
    sp = []
    for k, (_, v) in enumerate(SPECIALS):
        for a in range(3):
            e = kps[(3 * k + a) % len(kps)].copy()
            if a != 1: e["x"] = v
            if a != 0: e["y"] = v
            sp.append(e)
    merged, special = interleave([kps[i] for i in range(min(len(kps), 60))], sp)
    out = np.array(merged, kps.dtype)
    beyond = np.array([cvround_index(x) == INT_MIN or cvround_index(y) == INT_MIN for x, y in zip(out["x"], out["y"])])
    return out, special, beyond


def check_tracked_rule(what, describe, assign, kps, wrong=None):
    """describe(kps) -> (desc, oob); assign(ref_desc, kps) -> kps with octaves.  A keypoint beyond int32 or at NaN has no tap inside
    its level: an all-zero descriptor with the oob flag, on every level, so that AssignKPtLevelByBestDesc leaves it on level 0 (the
    first of equal distances); the ordinary keypoints are what they are without the special ones between them."""
    pts, special, beyond = tracked_keypoints(kps)
    assert beyond.sum() >= 25 and (special & ~beyond).sum() >= 9
    desc, oob = describe(pts)
    if wrong == "saturate":                                                  # NaN -> 0: the keypoint would be described at column / row 0
        nan = np.isnan(pts["x"]) | np.isnan(pts["y"])
        at0 = pts.copy(); at0["x"] = np.nan_to_num(pts["x"], nan=0.0, posinf=np.inf, neginf=-np.inf); at0["y"] = np.nan_to_num(pts["y"], nan=0.0, posinf=np.inf, neginf=-np.inf)
        assert np.array_equal(desc[nan], describe(at0)[0][nan]), "%s: %d keypoints beyond every level have taps (expected: those of row / column 0)" % (what, int(nan.sum()))
        beyond = beyond & ~nan
    assert not desc[beyond].any() and oob[beyond].all(), "%s: %d keypoints beyond every level have taps" % (what, int(desc[beyond].any(axis=1).sum()))
    d0, o0 = describe(pts[~special])
    assert np.array_equal(desc[~special], d0) and np.array_equal(oob[~special], o0) and d0.any(axis=1).all() and not o0.all(), what
    ref = np.full((len(pts), 32), 0x5a, np.uint8)
    lv = assign(ref, pts)
    assert (lv["octave"][beyond] == 0).all(), "%s: keypoints beyond every level moved to octaves %s" % (what, sorted(set(lv["octave"][beyond].tolist())))
    assert np.array_equal(lv["octave"][~special], assign(ref[~special], pts[~special])["octave"]), what


# family 5, SearchByProjectionLast: the caller's threshold as the search radius (level scale 1)
GRID_COLS, GRID_ROWS = 64, 48
PROJ_TH = [("0", 0.0), ("-1", -1.0), ("nan", NAN), ("inf", INF), ("1e12", f32(1e12)), ("2^31 cells", f32(2.0 ** 31 * INIT_W / GRID_COLS))]


def cell_range_rule(x, y, r, gb, wrong=None):
    """Frame::GetFeaturesInArea's cell range by the rule: (cx0, cx1, cy0, cy1), or None where the reference returns before it looks
    at a cell.  float32 arithmetic as the reference's; the conversions are floor_index and its ceil twin.  gb: minX, minY, invW, invH."""
    f = np.float32
    with np.errstate(all="ignore"):
        lo_x = f(f(f(f(x) - f(gb.minX)) - f(r)) * f(gb.invW)); hi_x = f(f(f(f(x) - f(gb.minX)) + f(r)) * f(gb.invW))
        lo_y = f(f(f(f(y) - f(gb.minY)) - f(r)) * f(gb.invH)); hi_y = f(f(f(f(y) - f(gb.minY)) + f(r)) * f(gb.invH))
    ceil_index = lambda v: to_index(math.ceil(v) if math.isfinite(v) else v, wrong)
    cx0 = max(0, floor_index(float(lo_x), wrong))
    if cx0 >= GRID_COLS:
        return None
    cx1 = min(GRID_COLS - 1, ceil_index(float(hi_x)))
    if cx1 < 0:
        return None
    cy0 = max(0, floor_index(float(lo_y), wrong))
    if cy0 >= GRID_ROWS:
        return None
    cy1 = min(GRID_ROWS - 1, ceil_index(float(hi_y)))
    if cy1 < 0:
        return None
    return cx0, cx1, cy0, cy1


def area_is_empty(x, y, r, gb, wrong=None):
    """True when the reference returns before it looks at a cell, or when no keypoint can pass |dx| < r (r <= 0 or NaN)"""
    return cell_range_rule(x, y, r, gb, wrong) is None or not r > 0


def pos_in_grid(x, y, gb, wrong=None):
    """Frame::PosInGrid by the rule: the cell (px, py) of a keypoint, None outside the grid"""
    f = np.float32
    with np.errstate(all="ignore"):
        px = round_index(float(f(f(f(x) - f(gb.minX)) * f(gb.invW))), wrong); py = round_index(float(f(f(f(y) - f(gb.minY)) * f(gb.invH))), wrong)
    return (px, py) if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS else None


def radius_match_model(kps, desc, gb, valid, uv, radius, level, q_desc, inv_sigma2=None, wrong=None):
    """The search core of Fuse / SearchBySim3 / SearchByProjection(KeyFrame, Scw) by brute force and by the rule: per query the keypoint
    of least descriptor distance, first in GetFeaturesInArea's order (cells column by column, a cell's keypoints by index), among
    those in the grid, in the cell range, with |dx| < r and |dy| < r, octave in [level - 1, level] and, with inv_sigma2, a squared
    reprojection error e2 inv_sigma2[octave] <= 5.99.  -> (best_idx, best_dist), (-1, 256) when nothing qualifies."""
    f = np.float32
    cells = {}
    for i in range(len(kps)):
        c = pos_in_grid(kps["x"][i], kps["y"][i], gb, wrong)
        if c is not None:
            cells.setdefault(c, []).append(i)
    bits = np.unpackbits(np.asarray(desc, np.uint8)[:, :32], axis=1)
    bi = np.full(len(valid), -1, np.int32); bd = np.full(len(valid), 256, np.int32)
    for m in range(len(valid)):
        if not valid[m]:
            continue
        u, v, r = f(uv[m][0]), f(uv[m][1]), f(radius[m])
        cr = cell_range_rule(u, v, r, gb, wrong)
        if cr is None:
            continue
        qb = np.unpackbits(np.asarray(q_desc[m], np.uint8)[:32])
        for ix in range(cr[0], cr[1] + 1):
            for iy in range(cr[2], cr[3] + 1):
                for i in cells.get((ix, iy), ()):
                    with np.errstate(all="ignore"):
                        dx, dy = f(kps["x"][i] - u), f(kps["y"][i] - v)
                    if not (abs(dx) < r and abs(dy) < r):
                        continue
                    o = int(kps["octave"][i])
                    if o < level[m] - 1 or o > level[m]:
                        continue
                    with np.errstate(all="ignore"):
                        e2 = f(f(f(dx * dx) + f(dy * dy)) * f(inv_sigma2[o])) if inv_sigma2 is not None else f(0)
                    if e2 > 5.99:
                        continue
                    d = int((bits[i] != qb).sum())
                    if d < bd[m]:
                        bd[m], bi[m] = d, i
    return bi, bd


RADII = [("0", 0.0), ("-1", -1.0), ("nan", NAN), ("inf", INF), ("1e12", f32(1e12)), ("2^31 cells", f32(2.0 ** 31 * INIT_W / GRID_COLS)), ("1e9", 1e9)]


@functools.lru_cache(maxsize=None)
def radius_scene(kind):
    """kind "queries": 120 ordinary keypoints; the queries are exact copies of keypoints (position + 0.25 px, descriptor, octave, radius
    5), every second one with a special value in u, in v or in both, or with a radius of RADII.
    kind "keypoints": the searched frame also holds a keypoint at every special position (x, y, both), each with a descriptor of its
    own, and the query that goes with it asks at that very position for that very descriptor.
    -> dict(kps, desc, valid, uv, radius, level, qd, special)"""
    W, H = INIT_W, INIT_H
    rng = np.random.default_rng(17 if kind == "queries" else 18)
    n = 120
    kps = synth.random_keypoints(n, W, H, nlevels=2, seed=91); desc = synth.random_descriptors(n, seed=92)
    pick = rng.permutation(n)
    ordinary = [(float(kps["x"][i]) + 0.25, float(kps["y"][i]) - 0.25, 5.0, int(kps["octave"][i]), desc[i]) for i in pick[:60]]
    sp = []
    if kind == "queries":
        j = 60
        for _, v in SPECIALS:
            for a in range(3):
                i = pick[j % n]; j += 1
                sp.append((v if a != 1 else float(kps["x"][i]), v if a != 0 else float(kps["y"][i]), 5.0, int(kps["octave"][i]), desc[i]))
        for _, r in RADII:
            i = pick[j % n]; j += 1
            sp.append((float(kps["x"][i]), float(kps["y"][i]), r, int(kps["octave"][i]), desc[i]))
    else:
        extra = np.zeros(3 * len(SPECIALS), kps.dtype); ed = synth.random_descriptors(len(extra), seed=93)
        for k, (_, v) in enumerate(SPECIALS):
            for a in range(3):
                e = extra[3 * k + a]; i = pick[(60 + 3 * k + a) % n]
                e["x"] = v if a != 1 else kps["x"][i]; e["y"] = v if a != 0 else kps["y"][i]
                e["size"] = 31.0; e["octave"] = 0; e["class_id"] = -1
                sp.append((float(e["x"]), float(e["y"]), 5.0, 0, ed[3 * k + a]))
        order = rng.permutation(n + len(extra))                              # the special keypoints between the ordinary ones
        kps = np.concatenate([kps, extra])[order]; desc = np.concatenate([desc, ed])[order]
    merged, special = interleave(ordinary, sp)
    d = dict(kps=kps, desc=np.ascontiguousarray(desc), valid=np.ones(len(merged), np.uint8),
             uv=np.array([[q[0], q[1]] for q in merged], np.float32), radius=np.array([q[2] for q in merged], np.float32),
             level=np.array([q[3] for q in merged], np.int32), qd=np.ascontiguousarray(np.stack([q[4] for q in merged])), special=special)
    for a in d.values():
        a.setflags(write=False)
    return d


INV_SIGMA2 = (1.0 / np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)


def check_radius_rule(what, run, kind, gb, sigma=False, wrong=None):
    """run(kps, desc, valid, uv, radius, level, qd) -> (best_idx, best_dist) against the brute-force model"""
    s = radius_scene(kind)
    args = (s["kps"], s["desc"], s["valid"], s["uv"], s["radius"], s["level"], s["qd"])
    bi, bd = run(*args)
    wi, wd = radius_match_model(args[0], args[1], gb, *args[2:], inv_sigma2=INV_SIGMA2 if sigma else None, wrong=wrong)
    bad = np.flatnonzero((bi != wi) | (bd != wd))
    assert len(bad) == 0, "%s %s: %d queries differ from the rule, first %d (uv %s radius %r): got %d / %d, expected %d / %d" % (
        what, kind, len(bad), bad[0], s["uv"][bad[0]].tolist(), float(s["radius"][bad[0]]), bi[bad[0]], bd[bad[0]], wi[bad[0]], wd[bad[0]])
    hit = wi >= 0
    assert hit[~s["special"]].all() and (wd[~s["special"]] == 0).all() and (~hit[s["special"]]).sum() >= 40, what     # (ordinary queries find their keypoint)


def check_proj_th_rule(what, run, uv, gb, wrong=None):
    """run(th) -> (nmatches, cur_mp out, cur_mp in).  Where every query's area is empty by the rule nothing is matched and the
    frame's map points come back untouched; where the rule lets every query see keypoints, something is."""
    for name, th in PROJ_TH + [("15", 15.0)]:
        empty = [area_is_empty(float(u), float(v), th, gb, wrong) for u, v in uv]
        n, out, before = run(th)
        if all(empty):
            assert n == 0 and np.array_equal(out, before), "%s th %s: %d matches where every area is empty" % (what, name, n)
        else:
            assert not any(empty) and n > 10, "%s th %s: %d matches where every query sees keypoints" % (what, name, n)


# ---------------------------------------------------------------------------------------------------
# family 6: projection on the device.  The hand view of tests/test_proj_ref.py: identity pose, fx = fy = 100, c = (50, 40), bounds
# [0, 100] x [0, 80], eight levels of 1.2; map points are therefore given in camera coordinates
def hand_view_kw(**kw):
    sf, ls = synth.scale_tables(8, 1.2)
    a = dict(R=np.eye(3), t=np.zeros(3), Ow=np.zeros(3), cam=(100.0, 100.0, 50.0, 40.0), bounds=(0.0, 100.0, 0.0, 80.0), nlevels=8,
             log_scale=ls, scale_factors=sf, mbf=40.0)
    a.update(kw)
    return a


# name, P, normal, minD, maxD, the reject reason derived by hand (isInFrustum: 2 depth, 3 / 4 bounds, 5 distance, 6 angle, 7 projection not finite)
MAP_POINTS = [
    ("x nan", (NAN, 0, 5), (0, 0, 1), 1, 10, 7),                 # u = NaN
    ("z nan", (0, 0, NAN), (0, 0, 1), 1, 10, 7),                 # NaN < 0 is false: the depth test passes, the projection is NaN
    ("x +inf", (INF, 0, 5), (0, 0, 1), 1, 10, 7),
    ("y -inf", (0, -INF, 5), (0, 0, 1), 1, 10, 7),
    ("x 1e30", (1e30, 0, 5), (0, 0, 1), 1, 10, 3),               # u = 2e31: finite, right of the image
    ("y -1e30", (0, -1e30, 5), (0, 0, 1), 1, 10, 4),
    ("z 1e30", (0, 0, 1e30), (0, 0, 1), 1, 10, 5),               # projects onto the principal point, 1e30 away
    ("z +inf", (0, 0, INF), (0, 0, 1), 1, 10, 7),                # mRcw * P: the x row's 0 * inf is NaN
    ("z -inf", (0, 0, -INF), (0, 0, 1), 1, 10, 2),
    ("z 0", (1, 0, 0), (0, 0, 1), 1, 10, 7),                     # u = 100 / 0 = inf
    ("origin", (0, 0, 0), (0, 0, 1), 1, 10, 7),                  # 0 / 0
    ("z 1e-38", (1, 0, 1e-38), (0, 0, 1), 1, 10, 7),             # u = 1e40 overflows to inf
    ("z -1e-38", (1, 0, -1e-38), (0, 0, 1), 1, 10, 2),
    ("z denormal", (1, 0, 1e-40), (0, 0, 1), 1, 10, 7),
    ("z denormal on the axis", (0, 0, 1e-40), (0, 0, 1), 1, 10, 5),   # u = 50: in the image, 1e-40 away < 0.8
    ("zero normal", (0, 0, 5), (0, 0, 0), 1, 10, 6),             # cos = 0 / 5 = 0 < 0.5
    ("distances 0", (0, 0, 5), (0, 0, 1), 0, 0, 5),              # 5 > 1.2 * 0
    ("nan normal", (0, 0, 5), (NAN, 0, 1), 1, 10, 0),            # cos NaN: "NaN < limit" is false, the point stays in view
    ("ordinary", (0, 0, 5), (0, 0, 1), 1, 10, 0),
]


@functools.lru_cache(maxsize=None)
def map_point_scene():
    """dict(pos, normal, min_dist, max_dist, reason, special): 64 ordinary points in front of the hand view with MAP_POINTS between them"""
    rng = np.random.default_rng(61)
    ordinary = [((float(rng.uniform(-2, 2)), float(rng.uniform(-1.5, 1.5)), float(rng.uniform(3, 8))), (0.0, 0.0, 1.0), 1.0, 10.0, None) for _ in range(64)]
    merged, special = interleave(ordinary, [m[1:] for m in MAP_POINTS])
    d = dict(pos=np.array([m[0] for m in merged], np.float32), normal=np.array([m[1] for m in merged], np.float32),
             min_dist=np.array([m[2] for m in merged], np.float32), max_dist=np.array([m[3] for m in merged], np.float32),
             reason=np.array([-1 if m[4] is None else m[4] for m in merged], np.int32), special=special)
    for a in d.values():
        a.setflags(write=False)
    return d


def predict_scale_rule(max_dist, dist, nlevels, log_scale, wrong=None):
    """MapPoint::PredictScale by the rule: ceil(log(maxDistance / dist) / logScaleFactor) converted to int, clamped to
    [0, nlevels - 1].  Returns (level, decided): decided is False where the quotient lies within 1e-4 of an integer, where float32
    logf and this float64 log may round to different sides."""
    with np.errstate(all="ignore"):
        ratio = float(np.float32(max_dist) / np.float32(dist))
        q = (math.log(ratio) if ratio > 0 and math.isfinite(ratio) else (INF if ratio > 0 else (-INF if ratio == 0 else NAN))) / float(log_scale)
    n = to_index(float(math.ceil(q)) if math.isfinite(q) else q, wrong)
    return min(max(n, 0), nlevels - 1), not (math.isfinite(q) and abs(q - round(q)) < 1e-4)


def check_frustum_rule(what, frustum, wrong=None):
    """frustum(view keywords, pos, normal, min_dist, max_dist) -> the dict of isInFrustum's outputs for one view.  The hand-derived
    reject reasons; a rejected point has level -1 and is not searched; the levels of the points in view are PredictScale's by the
    rule, that of an infinite ratio 0.  wrong: the conversion of predict_scale_rule."""
    s = map_point_scene()
    o = frustum(hand_view_kw(), s["pos"], s["normal"], s["min_dist"], s["max_dist"])
    want = s["reason"][s["special"]]; got = o["reason"][s["special"]]
    assert np.array_equal(got, want), "%s: reject reasons %s, by hand %s" % (what, got.tolist(), want.tolist())
    rej = o["reason"] != 0
    assert (o["in_view"][rej] == 0).all() and (o["level"][rej] == -1).all() and (o["level_scale"][rej] == 0).all()
    assert "search" not in o or (o["search"][rej] == 0).all()               # (the restatement and the fused entries report it)
    assert (o["in_view"][~rej] == 1).all() and ((o["level"][~rej] >= 0) & (o["level"][~rej] < 8)).all() and (~rej[~s["special"]]).sum() >= 30
    ls = hand_view_kw()["log_scale"]
    ndec = 0
    for m in np.flatnonzero(~rej):
        lv, decided = predict_scale_rule(s["max_dist"][m], np.sqrt((s["pos"][m].astype(F64) ** 2).sum()), 8, ls, wrong)
        if decided:
            ndec += 1
            assert o["level"][m] == lv, "%s: point %d at %s has level %d, PredictScale by the rule %d" % (what, m, s["pos"][m].tolist(), o["level"][m], lv)
    assert ndec >= 30
    # the camera 5 in front of the world origin, the frame's centre mOw AT the origin: the point at the origin projects onto the
    # principal point at distance 0 from mOw.  With minDistance 0 the distance gate passes, cos = 0 / 0 passes "NaN < limit", and
    # PredictScale's ratio 10 / 0 = inf has no int: INT_MIN, clamped to level 0 (the saturating conversion gives level 7)
    z = frustum(hand_view_kw(t=(0.0, 0.0, 5.0)), np.zeros((1, 3), np.float32), np.float32([[0, 0, 1]]), np.zeros(1, np.float32), np.float32([10.0]))
    lv0, _ = predict_scale_rule(10.0, 0.0, 8, ls, wrong)                     # 0 by the rule
    assert z["in_view"][0] == 1 and z["reason"][0] == 0 and z["level"][0] == lv0 and np.isnan(z["view_cos"][0]), \
        "%s: the point at mOw: in_view %d reason %d level %d, PredictScale of an infinite ratio %d" % (what, z["in_view"][0], z["reason"][0], z["level"][0], lv0)
    assert wrong is not None or (lv0 == 0 and z["level_scale"][0] == 1.0)
    # a NaN in R: every point's projection is NaN
    R = np.eye(3); R[0, 1] = NAN
    o = frustum(hand_view_kw(R=R), s["pos"], s["normal"], s["min_dist"], s["max_dist"])
    assert np.isin(o["reason"], (2, 7)).all() and (o["reason"][~s["special"]] == 7).all(), "%s: NaN in R: reasons %s" % (what, np.unique(o["reason"]).tolist())


# ---------------------------------------------------------------------------------------------------
# family 7: degenerate images
def degenerate_images(W=61, H=45):
    """name -> float32 image"""
    const = np.full((H, W), 0.375, np.float32)
    patch = np.zeros((H, W), np.float32); patch[3:9, 31:40] = np.linspace(0.1, 0.9, 54, dtype=np.float32).reshape(6, 9)
    return {"constant": const, "single_patch": patch}


# ===================================================================================================
# the checks and scenes that tests/test_oracle_edges.py (the oracle) and tests/test_gpu_edges.py (the kernels) share
BUILDS = [False, True]                                  # the `fast` argument of the oracle's wrappers


SIGMAS = [1.0, 2.5]


# ---------------------------------------------------------------------------------------------------
# family 1: accumulation
def check_acc_rule(what, got, oracle, ev, W, H, sigma, pol, fast=False, wrong=None):
    """got = (f32, u8, minmax) of ev2im_gauss over `ev`.  The image, the extremes and the grey levels equal, as bytes, the oracle's
    image of those events alone that reach the frame by the rule; the float image lies inside plain_ref.gauss_bound of their float64
    image."""
    h = pr.stamp_radius(sigma)
    sub, keep = acc_expected_events(ev, W, H, h, wrong=wrong)
    ef, eu, emm = oracle.ev2im_gauss(sub, W, H, sigma, pol, True, fast=fast)
    gf, gu, gmm = got
    nbad = int((gf.view(np.uint32) != ef.view(np.uint32)).sum())
    assert nbad == 0, "%s: %d pixels differ from the image of the %d events that reach the frame (of %d)" % (what, nbad, len(sub), len(ev))
    assert same_f32(gmm, emm) and np.array_equal(gu, eu), "%s: extremes %s, expected %s" % (what, gmm, emm)
    ref = pr.gauss_image(sub, W, H, sigma, pol)
    op.check_accumulation(what, gf, gmm, gu, ref)
    return int(keep.sum())


def check_blank(what, got, W, H):
    """a call none of whose events reaches the frame: an all-zero image and the untouched extremes (minVal 0, maxVal -1e6)"""
    gf, gu, gmm = got
    assert gf.shape == (H, W) and not gf.view(np.uint32).any(), "%s: %d pixels written" % (what, int((gf != 0).sum()))
    assert gmm.tolist() == [0.0, -1000000.0], "%s: extremes %s" % (what, gmm.tolist())
    assert gu is None or not gu.any(), what


def blank_events(W, H, h):
    """every edge position that does not reach the frame, and nothing else"""
    ev, special, _ = acc_case(W, H, h)
    sp = ev[special]
    miss = np.array([reaches(float(e["x"]), float(e["y"]), W, H, h) is None for e in sp])
    assert miss.sum() >= 3 * len(SPECIALS) - 12
    return sp[miss]


def count_events(W, H):
    """the count form's inputs: the ordinary events with V (h = 0) between them, then the exact ties in x on row 7 and in y on
    column 5"""
    ev, _, _ = acc_case(W, H, 0)
    ties = [(x, 7.0) for x, _ in count_ties(W)] + [(5.0, y) for y, _ in count_ties(H)]
    return np.concatenate([ev, make_events(ties)])


def tie_image(W, H, wrong=None):
    """the ties alone: one count of 0.001f at each expected pixel"""
    img = np.zeros((H, W), np.float32)
    for (x, col), (y, row) in zip(count_ties(W), count_ties(H)):
        if wrong == "half_even":
            col, row = round_index(x, wrong), round_index(y, wrong)
            col = col if 0 <= col < W else None; row = row if 0 <= row < H else None
        if col is not None:
            img[7, col] = np.float32(0.001)
        if row is not None:
            img[row, 5] = np.float32(0.001)
    return img


def check_count_rule(what, run, oracle, W, H, fast=False, wrong=None):
    """run(ev, pol) -> (f32, u8 or None, minmax) of ev2im.  The ties alone give the hand-written image; the mixed call equals the
    oracle's image of the events that reach the frame by the rule."""
    ties = make_events([(x, 7.0) for x, _ in count_ties(W)] + [(5.0, y) for y, _ in count_ties(H)])
    tf = run(ties, False)[0]
    want = tie_image(W, H, wrong)
    assert np.array_equal(tf.view(np.uint32), want.view(np.uint32)), "%s: the ties land in %s, expected %s" % (
        what, np.argwhere(tf != 0).tolist(), np.argwhere(want != 0).tolist())
    ev = count_events(W, H)
    for pol in (False, True):
        gf, gu, gmm = run(ev, pol)
        sub, keep = acc_expected_events(ev, W, H, 0, count=True, wrong=wrong)
        ef, eu, emm = oracle.ev2im(sub, W, H, pol, True, fast=fast)
        assert np.array_equal(gf.view(np.uint32), ef.view(np.uint32)), "%s pol %d: the count image differs from that of the %d events that reach the frame" % (what, pol, len(sub))
        assert same_f32(gmm, emm) and (gu is None) == (eu is None) and (gu is None or np.array_equal(gu, eu)), what
        # ... and from the counts themselves: every pixel is the float32 sum, in order, of +-0.001f per event
        cnt = np.zeros((H, W), np.float32)
        for e in sub:
            xi, yi = reaches(float(e["x"]), float(e["y"]), W, H, 0, count=True)
            cnt[yi, xi] = cnt[yi, xi] + np.float32(-0.001 if (pol and not e["p"]) else 0.001)
        if wrong is None:
            assert np.array_equal(gf.view(np.uint32), cnt.view(np.uint32)), what


# ---------------------------------------------------------------------------------------------------
# family 2: raw sensor events through undistortion maps
RAW_W, RAW_H = 61, 45


# ---------------------------------------------------------------------------------------------------
# family 3: motion-compensated images
MCI = mci_cases(op.WARP_CAMS, op.warp_events)


MCI_BLANK = ("depth nan", "one event", "one time stamp")          # 0 * inf and NaN depths: every warped position is NaN


def mci_oracle(oracle, case, pol):
    """(image, u8, extremes) and the warped positions of a case from the oracle"""
    group, cn, ev, m = MCI[case]
    cam, W, H = op.WARP_CAMS[cn]
    if group == "se3":
        return (oracle.ev2mci_se3(ev, cam, m["angle"], m["axis"], m["t"], m["medDepth"], W, H, MCI_SIGMA, pol, True),
                oracle.mci_warp_se3(ev, cam, m["angle"], m["axis"], m["t"], m["medDepth"]))
    return oracle.ev2mci_se2(ev, cam, m, W, H, MCI_SIGMA, pol, True), oracle.mci_warp_se2(ev, cam, m)


def check_mci_rule(what, case, got, uv, oracle, pol, wrong=None):
    """got: a motion-compensated image (f32, u8, extremes); uv: the oracle's warped positions.  The image is that of the events
    whose warped position reaches the frame by the rule; a window whose positions are all NaN leaves a blank image."""
    group, cn, ev, m = MCI[case]
    _, W, H = op.WARP_CAMS[cn]
    if any(k in case for k in MCI_BLANK):
        assert np.isnan(uv).all(), "%s: warped positions %s" % (what, uv[:3].tolist())
        if wrong is None:
            check_blank(what, (got[0], None, got[2]), W, H)
            return 0
    return check_acc_rule(what, got, oracle, events_at(ev, uv), W, H, MCI_SIGMA, pol, wrong=wrong)


def mci_plain_uv(case, wrong=None):
    """the warped positions by plain_ref's float64 warp (NaN where the formula is 0 * inf or 0 / 0)"""
    group, cn, ev, m = MCI[case]
    cam = op.cam64(op.WARP_CAMS[cn][0])
    with np.errstate(all="ignore"):
        if group == "se3":
            return pr.warp_se3(ev, cam, m["angle"], m["axis"], m["t"], F64(np.float32(m["medDepth"])), wrong)
        return pr.warp_se2(ev, cam, np.asarray(m, np.float32).astype(F64), wrong)


def mci_uv_tolerance(case, plain):
    """per coordinate: the tolerance of tests/test_oracle_plain.py for this camera and motion, which holds for positions inside a
    346-px image, grown in proportion for positions farther out (a float32 position's rounding grows with its size)"""
    group, cn, ev, m = MCI[case]
    base = op.FACTOR * op.MEASURED[("uv", cn, group)]
    with np.errstate(all="ignore"):
        tol = base * np.maximum(1.0, np.abs(plain) / 346.0)
        if group == "se3" and cn == "kb8":
            # KannalaBrandt8::project(Vector3d) takes theta and psi from atan2f of float arguments: each carries up to 2^-23 (|angle| + 1)
            # (one ulp of the result, half an ulp of either argument).  u = fx r(theta) cos psi + cx turns that into
            # fx (|r'(theta)| dtheta + r dpsi): far from the axis r' = 1 + 3 k1 theta^2 + ... + 9 k4 theta^8 reaches 10^3.
            # Where x^2 + y^2 is below the smallest normal float its float copy is 0 or has lost its digits: no position to compare
            cam = op.cam64(op.WARP_CAMS[cn][0]); k = cam[4:8]
            P3 = pr.warp_se3_points(ev, cam, m["angle"], m["axis"], m["t"], F64(np.float32(m["medDepth"])))
            rho2 = P3[:, 0] ** 2 + P3[:, 1] ** 2
            th = np.arctan2(np.sqrt(rho2), P3[:, 2]); psi = np.arctan2(P3[:, 1], P3[:, 0]); t2 = th * th
            r = th * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
            dr = np.abs(1.0 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3]))))
            extra = max(cam[0], cam[1]) * 2.0 ** -23 * (dr * (th + 1.0) + np.abs(r) * (np.abs(psi) + 1.0))
            tol = tol + extra[:, None]
            tol[rho2 < 2.0 ** -126] = np.inf
        return tol


def check_mci_plain(what, case, got, uv, pol, wrong=None):
    """plain_ref's warp decides.  (a) uv, warped positions as the oracle or a kernel holds them: NaN exactly where the plain warp is
    NaN, else within the tolerance.  (b) an event reaches the frame by the rule from uv iff it does from the plain position, unless
    the plain position lies within the tolerance of an integer (its floor is then not decided).  (c) the image lies inside the
    accumulation bound of the plain image of the plain positions, the pixels of the undecided events masked."""
    group, cn, ev, m = MCI[case]
    _, W, H = op.WARP_CAMS[cn]
    plain = mci_plain_uv(case, wrong)
    tol = mci_uv_tolerance(case, plain)
    h = pr.stamp_radius(MCI_SIGMA)
    pn = ~np.isfinite(plain)
    assert np.array_equal(np.isnan(uv) | np.isinf(uv), pn), "%s: non-finite warped positions at %s, plain at %s" % (
        what, np.flatnonzero(~np.isfinite(uv).all(axis=1))[:6].tolist(), np.flatnonzero(pn.any(axis=1))[:6].tolist())
    fin = ~pn
    d = np.abs(uv.astype(F64)[fin] - plain[fin])
    worst = np.argmax(d / tol[fin]) if d.size else 0
    assert (d <= tol[fin]).all(), "%s: a warped position differs from the plain one by %.3g px (allowed %.3g)" % (what, d[worst], tol[fin][worst])
    with np.errstate(all="ignore"):
        near = fin & ((np.abs(plain - np.rint(plain)) <= tol) | np.isinf(tol))
    undecided = near.any(axis=1)
    mask = np.zeros((H, W), bool)
    for k in range(len(ev)):
        if pn[k].any():
            assert reaches(float(uv[k, 0]), float(uv[k, 1]), W, H, h) is None, "%s: event %d at %s reaches the frame" % (what, k, uv[k].tolist())
            continue
        if undecided[k]:
            lo = [int(np.rint(plain[k, a])) - 1 - h if near[k, a] else int(np.floor(plain[k, a])) - h for a in (0, 1)]
            hi = [int(np.rint(plain[k, a])) + h if near[k, a] else int(np.floor(plain[k, a])) + h for a in (0, 1)]
            mask[max(lo[1], 0):max(hi[1] + 1, 0), max(lo[0], 0):max(hi[0] + 1, 0)] = True
            if np.isinf(tol[k]).any():                                       # theta = atan2f(0, z) = 0: the principal point
                cx, cy = op.WARP_CAMS[cn][0][2:4]
                mask[max(int(cy) - h - 1, 0):int(cy) + h + 2, max(int(cx) - h - 1, 0):int(cx) + h + 2] = True
            continue
        a = reaches(float(uv[k, 0]), float(uv[k, 1]), W, H, h); b = reaches(float(plain[k, 0]), float(plain[k, 1]), W, H, h)
        assert a == b, "%s: event %d reaches %s from %s, %s from the plain %s" % (what, k, a, uv[k].tolist(), b, plain[k].tolist())
    assert mask.mean() <= 0.02, "%s: %.4f of the pixels masked" % (what, mask.mean())
    ref = pr.gauss_image(ev, W, H, MCI_SIGMA, pol, xy=plain)
    inside = fin.all(axis=1)
    with np.errstate(all="ignore"):
        slack = ref["M"] * pr.stamp_slope(MCI_SIGMA) * np.sqrt(2.0) * float(np.nanmax(np.where(
            (np.abs(plain) < 2.0 * max(W, H)) & inside[:, None] & np.isfinite(tol), tol, 0.0), initial=0.0))
    op.check_accumulation(what, got[0], None, None, ref, mask=mask, extra=slack)
    # a coordinate lies within tol of an integer with probability 2 tol: per event 2 (tol_u + tol_v), summed over the events; twice that
    # expectation plus 3 bounds the count (the events without a position to compare, tol = inf, count fully)
    with np.errstate(all="ignore"):
        expect = float(np.minimum(1.0, 2.0 * np.where(fin, np.minimum(tol, 0.5), 0.0).sum(axis=1)).sum())
    allowed = int(np.ceil(2.0 * expect)) + 3
    assert undecided.sum() <= allowed, "%s: %d events undecided, %d allowed" % (what, int(undecided.sum()), allowed)
    return int(undecided.sum())


# ---------------------------------------------------------------------------------------------------
# family 4: pyramidal Lucas-Kanade
LK_CASES = sorted(lk_cases())


def lk_run(track, case):
    """track(prevPts, initial flow or None) -> (nextPts, status, err); returns the answers for the case and for its ordinary points
    alone"""
    pts, flow, mask = lk_cases()[case]
    plain = track(pts[~mask], None if flow is None else flow[~mask])
    return track(pts, flow), plain


def oracle_tracker(oracle, fast):
    return lambda p, f: oracle.calc_optical_flow_pyr_lk(lk_image(), lk_image(1.0), p, f, LK_WIN, LK_MAXLEVEL, LK_COUNT, LK_EPS,
                                                        0 if f is None else 4, fast=fast)


# ---------------------------------------------------------------------------------------------------
# family 5, SearchForInitialization
_INIT = {}


def init_frames(oracle):
    """two event images a small motion apart and their level-0 keypoints (one pyramid level: every keypoint is a query)"""
    if not _INIT:
        from eorb_slam_amd import synth
        W, H = INIT_W, INIT_H
        ext = oracle.OrbExtractor(200, 1.2, 1, 10, 0, edgeTh=19, imWidth=W)
        for k in range(2):
            ev = synth.shapes_events(3000, W, H, seed=5, motion=0.3 + 0.02 * k, undistort=True)
            u8 = oracle.ev2im_gauss(ev, W, H, 1.0, False, True)[1]
            _, kps, desc, _ = ext.extract(u8)
            _INIT[k] = (kps, desc)
        assert 4 * len(SPECIALS) + 4 <= len(_INIT[0][0]) <= 200
    return _INIT[0], _INIT[1]


def projection_runs(oracle_or_none, call_last, call_kf, call_map, k1, d1, k2, n2):
    """the three window matchers fed by the caller, as run(uv, level_scale, th) of check_projection_rule; call_* take the keyword
    arguments of the product's and the oracle's wrappers alike"""
    n1 = len(k1)
    valid = np.ones(n1, np.uint8); mp_obs = np.ones(n1, np.uint8)
    slots = np.full(n2, -1, np.int32); slots[::17] = -2
    lvl = k1["octave"].astype(np.int32); vc = np.full(n1, 0.9995, np.float32)
    return {
        "SearchByProjectionLast": (lambda uv, ls, th: call_last(valid, uv, d1, mp_obs, slots, th, ls) + (slots,), 1.0),
        "SearchByProjectionKF": (lambda uv, ls, th: call_kf(k1, valid, uv, lvl, ls, d1, slots, th) + (slots,), 1.0),
        "SearchByProjectionMap": (lambda uv, ls, th: call_map(valid, uv, lvl, vc, d1, mp_obs, slots, th, ls) + (slots,), 2.5),   # RadiusByViewingCos: 2.5 above 0.998
    }


def projection_uv(k1):
    rng = np.random.default_rng(11)
    return np.stack([k1["x"] + 1.0 + rng.normal(0, 0.5, len(k1)), k1["y"] - 1.0 + rng.normal(0, 0.5, len(k1))], axis=1).astype(np.float32)


_TRACKED = {}


def tracked_scene(oracle):
    """an event image, its keypoints on three levels (octaves as extracted) and the extractor's parameters"""
    if not _TRACKED:
        from eorb_slam_amd import synth
        W, H = INIT_W, INIT_H
        ev = synth.shapes_events(3000, W, H, seed=5, motion=0.3, undistort=True)
        u8 = oracle.ev2im_gauss(ev, W, H, 1.0, False, True)[1]
        _, kps, _, _ = oracle.OrbExtractor(300, 1.2, 3, 10, 0, edgeTh=19, imWidth=W).extract(u8)
        assert len(kps) >= 60 and len(set(kps["octave"].tolist())) == 3
        _TRACKED["img"], _TRACKED["kps"] = u8, kps
    return _TRACKED["img"], _TRACKED["kps"]


def proj_last_args(oracle):
    """SearchByProjectionLast of frame 2 against frame 1's keypoints as map points, projected 1 px off their own positions"""
    (k1, d1), (k2, d2) = init_frames(oracle)
    n1 = len(k1)
    rng = np.random.default_rng(11)
    uv = np.stack([k1["x"] + 1.0 + rng.normal(0, 0.5, n1), k1["y"] - 1.0 + rng.normal(0, 0.5, n1)], axis=1).astype(np.float32)
    valid = np.ones(n1, np.uint8); mp_obs = np.ones(n1, np.uint8); ls = np.ones(n1, np.float32)
    cur_mp = np.full(len(k2), -1, np.int32); cur_mp[::17] = -2
    return k1, d1, k2, d2, valid, uv, mp_obs, cur_mp, ls


# the radius search shared by Fuse, SearchBySim3 and SearchByProjection(KeyFrame, Scw): special query centres and radii, special keypoints
SCALE_FACTORS = (np.float32(1.2) ** np.arange(8)).astype(np.float32)


def fuse_expected(gb, th, wrong=None):
    """Fuse over the "queries" scene with the threshold th: radius = th * scaleFactor[level], the mono reprojection gate, TH_LOW"""
    s = radius_scene("queries")
    radius = (np.float32(th) * SCALE_FACTORS[s["level"]]).astype(np.float32)
    bi, bd = radius_match_model(s["kps"], s["desc"], gb, s["valid"], s["uv"], radius, s["level"], s["qd"], inv_sigma2=INV_SIGMA2, wrong=wrong)
    return np.where(bd <= 50, bi, -1).astype(np.int32)


def sim3_expected(gb, th):
    """SearchBySim3 of the "keypoints" frame with itself, every keypoint projected onto its own position: the mutual best matches"""
    s = radius_scene("keypoints")
    n = len(s["kps"])
    uv = np.stack([s["kps"]["x"], s["kps"]["y"]], axis=1).astype(np.float32)
    lv = s["kps"]["octave"].astype(np.int32)
    radius = (np.float32(th) * SCALE_FACTORS[lv]).astype(np.float32)
    bi, bd = radius_match_model(s["kps"], s["desc"], gb, np.ones(n, np.uint8), uv, radius, lv, s["desc"])
    vn = np.where(bd <= 100, bi, -1)
    ok = (vn >= 0) & (vn[np.clip(vn, 0, n - 1)] == np.arange(n))
    return int(ok.sum()), np.where(ok, vn, -1).astype(np.int32), (np.ones(n, np.uint8), uv, lv, s["desc"])


# ---------------------------------------------------------------------------------------------------
# family 7: degenerate images
def check_degenerate_images(normalize, focus):
    """normalize(img) -> u8, focus(img) -> float.  cv::normalize of a constant image is 0 everywhere (max - min <= DBL_EPSILON: scale 0);
    so is that of an image holding +inf (scale = 255 / inf = 0) and a NaN -- inf * 0 and NaN * 0 are NaN, whose cvRound is INT_MIN,
    which saturates to 0.  (The non-finite pixels are not the first: the oracle seeds its extremes with pixel 0, which cv::minMaxLoc
    does not.)  measureImageFocus of a constant image is exactly 0; of a single patch, the plain value."""
    imgs = degenerate_images()
    const = imgs["constant"]
    assert not normalize(const).any()
    bad = imgs["single_patch"].copy(); bad[20, 30] = np.inf; bad[31, 7] = np.nan
    assert not normalize(bad).any()
    assert float(focus(const)) == 0.0
    op.check_focus("single patch", focus(imgs["single_patch"]), imgs["single_patch"])
    assert pr.focus(imgs["single_patch"]) > 0.01
