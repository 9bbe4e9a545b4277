"""Planted inputs for tests/helper_models.py: named, small, deterministic.

Stereo pairs: 240 x 180, ORBextractor(500, 1.2, 4, 20, 7, edge 19), built from synth.texture_image in horizontal bands; the right band
is the left one moved by (dx, dy), mirror-symmetric about a column, or noisy.  STEREO_PAIRS names them with the probe sites each must
reach (asserted with the model's probe by tests/test_oracle_helper_models.py).  The planted-keypoint cases reuse the level images of one
real extract() call and set keypoints and descriptors by hand; the device entry takes images, so these run on the oracle only.

The other scenes (knn2, window_match, distinctive, sort_by_response) are plain arrays."""
import functools

import numpy as np

from eorb_slam_amd import synth

import helper_models as hm

F = np.float32
W, H = 240, 180
ORB = dict(nfeatures=500, scaleFactor=1.2, nlevels=4, iniThFAST=20, minThFAST=7, edgeTh=19)
ORB_ARGS = (500, 1.2, 4, 20, 7, 19)


# ---- stereo pairs built from images ------------------------------------------------------------------------------------------------
def band_pair(bands, seed0=100):
    """bands = [(rows, dx, dy, sigma, mirror)]: the right band holds the left one moved dx pixels to the left and dy rows down, with
    Gaussian noise of that sigma; mirror = c makes the band symmetric about column c - 1 before anything else"""
    L, R = [], []
    for i, (rows, dx, dy, sigma, mirror) in enumerate(bands):
        T = synth.texture_image(W + 16, rows + 8, seed=seed0 + i)
        if mirror:
            half = T[:, :mirror]
            T = np.concatenate([half, half[:, ::-1][:, 1:], T], axis=1)[:, :W + 16]
        r = T[4 - dy:4 - dy + rows, dx:dx + W].astype(np.float64)
        if sigma:
            r = r + np.random.default_rng(seed0 + 50 + i).normal(0, sigma, r.shape)
        L.append(T[4:4 + rows, :W]); R.append(np.clip(np.rint(r), 0, 255).astype(np.uint8))
    return np.ascontiguousarray(np.concatenate(L)), np.ascontiguousarray(np.concatenate(R))


def _flat():
    return np.full((H, W), 128, np.uint8)


# name -> (images, mb, mbf, probe sites that must be non-zero).  mbf = "minU" is taken from the extracted keypoints (minu_mbf).
_MOVED = [(180, 6, 0, 0, 0)]
STEREO_PAIRS = {
    # (a) median 0: thDist = 0 and `0 < 0` is false, so the cut takes back every accepted match
    "identical": (lambda: band_pair([(180, 0, 0, 0, 0)]), 1.0, 30.0, ["disp_negative", "zero_branch", "n_eq_thDist"]),
    "mirror": (lambda: band_pair([(180, 0, 0, 0, 121)]), 1.0, 30.0, ["disp_negative", "zero_branch"]),
    # (b) identical bands between noisy moved ones: the median is > 0 and the 0.01 branch survives the cut
    "mixed": (lambda: band_pair([(60, 0, 0, 0, 0), (60, 6, 0, 2.0, 0), (60, 0, 0, 0, 61)]), 1.0, 30.0,
              ["zero_branch_kept", "disp_negative", "desc_tie", "sad_tie", "delta_half", "best_shift_edge", "best_shift_4", "scaled_half"]),
    # (c) dx = 6 against maxD = 6, 6.5 and a maxD that puts minU on a right keypoint
    "moved_maxd_6": (lambda: band_pair(_MOVED), 1.0, 6.0, ["disp_ge_maxD", "disp_eq_maxD", "uR_eq_minU"]),
    # the same against a band with noise: the median is > 0, so what `disparity < maxD` lets through shows in uRight and depth
    "moved_maxd_6_noisy": (lambda: band_pair([(90, 6, 0, 0, 0), (90, 6, 0, 1.0, 0)], 604), 1.0, 6.0, ["disp_ge_maxD", "disp_eq_maxD", "uR_eq_minU"]),
    "moved_maxd_6p5": (lambda: band_pair(_MOVED), 1.0, 6.5, ["uR_eq_maxU"]),
    "moved_minu": (lambda: band_pair(_MOVED), 1.0, "minU", ["uR_eq_minU"]),
    # (d) the row band decides
    "down_2": (lambda: band_pair([(180, 6, 2, 0, 0)]), 1.0, 30.0, ["row_eq_minr", "row_eq_maxr", "row_below_minr", "row_above_maxr"]),
    "down_3": (lambda: band_pair([(180, 6, 3, 0, 0)]), 1.0, 30.0, ["row_eq_minr", "row_below_minr", "best_dist_74", "best_dist_75"]),
    "down_4": (lambda: band_pair([(180, 6, 4, 0, 0)]), 1.0, 30.0, ["row_eq_minr", "row_below_minr"]),
    # (e) nothing to match
    "flat_right": (lambda: (band_pair(_MOVED)[0], _flat()), 1.0, 30.0, ["nmatch_zero"]),
    "flat_left": (lambda: (_flat(), band_pair(_MOVED)[1]), 1.0, 30.0, ["nmatch_zero"]),
    "no_match": (lambda: band_pair(_MOVED), 1.0, 2.0, ["nmatch_zero"]),
    # (f) noisy: N % 4 != 0, Nr % 64 != 0, Nr > 64, norms and the median > 0
    "noisy": (lambda: band_pair([(180, 6, 0, 2.0, 0)]), 1.0, 30.0, ["desc_tie", "desc_tie_across_64", "best_dist_75", "best_dist_99"]),
    # three noisy bands moved by 3, 6 (and a row down) and 12: an equal-distance pair of right keypoints and an equal-norm pair of
    # shifts whose order decides the result; two bands where a scaled coordinate at k + 0.5 decides it
    "ties": (lambda: band_pair([(60, 3, 0, 3.0, 0), (60, 6, 1, 1.0, 0), (60, 12, 0, 2.0, 0)], 444), 1.0, 30.0, ["desc_tie", "sad_tie"]),
    "halves": (lambda: band_pair([(90, 6, 0, 1.0, 0), (90, 9, 1, 2.0, 0)], 420), 1.0, 30.0, ["scaled_half"]),
}


class StereoInputs:
    """one real extract() of a pair by the oracle: the extractors (for the oracle's call), keypoints, descriptors, level images"""

    def __init__(self, oracle, left, right, fast=False):
        self.left, self.right = left, right
        self.eL = oracle.OrbExtractor(*ORB_ARGS[:5], edgeTh=ORB_ARGS[5], imWidth=W, fast=fast)
        self.eR = oracle.OrbExtractor(*ORB_ARGS[:5], edgeTh=ORB_ARGS[5], imWidth=W, fast=fast)
        _, self.kL, self.dL, _ = self.eL.extract(left, (0, 0))
        _, self.kR, self.dR, _ = self.eR.extract(right, (0, 0))
        if self.kL is None:
            self.kL, self.dL = np.zeros(0, oracle.KP_DTYPE), np.zeros((0, 32), np.uint8)
        if self.kR is None:
            self.kR, self.dR = np.zeros(0, oracle.KP_DTYPE), np.zeros((0, 32), np.uint8)
        E = self.eL.edge
        self.sizes = [self.eL.level_size(l) for l in range(ORB["nlevels"])]
        self.LL = [self.eL.level_buffer(l)[E:E + h, E:E + w] for l, (w, h) in enumerate(self.sizes)]
        self.LR = [self.eR.level_buffer(l)[E:E + h, E:E + w] for l, (w, h) in enumerate(self.sizes)]
        self.sf, self.inv = self.eL.scale_factors, self.eL.inv_scale_factors

    def with_keypoints(self, kL, dL, kR, dR):
        import copy
        o = copy.copy(self)
        o.kL, o.dL, o.kR, o.dR = kL, dL, kR, dR
        return o

    def model(self, mb, mbf, wrong=None):
        return hm.stereo_matches(self.LL, self.LR, self.sizes, self.sf, self.inv, self.kL, self.dL, self.kR, self.dR, mb, mbf, wrong)

    def oracle(self, mb, mbf):
        return self.eL.compute_stereo_matches(self.eR, self.kL, self.dL, self.kR, self.dR, mb, mbf)


_CACHE = {}


def stereo_inputs(oracle, name, fast=False):
    key = (name, fast)
    if key not in _CACHE:
        _CACHE[key] = StereoInputs(oracle, *STEREO_PAIRS[name][0](), fast=fast)
    return _CACHE[key]


def minu_mbf(I):
    """a maxD (= mbf / 1.0f, exact) that puts minU = uL - maxD exactly on the x of a right keypoint which is the left keypoint's true
    partner one level up from the base (so that x is no integer): the first left keypoint of level >= 1 with such a partner"""
    for iL in np.flatnonzero(I.kL["octave"] >= 1):
        uL = F(I.kL["x"][iL])
        for iR in np.flatnonzero((I.kR["octave"] == I.kL["octave"][iL]) & (np.abs(I.kR["y"] - I.kL["y"][iL]) < 0.01)):
            maxD = F(uL - F(I.kR["x"][iR]))
            if 5.5 < maxD < 6.5 and F(uL - maxD) == F(I.kR["x"][iR]) and float(maxD) != round(float(maxD)):
                return float(maxD)
    raise AssertionError("no level >= 1 keypoint with its partner at the same row")


def stereo_case(oracle, name, fast=False):
    """(inputs, mb, mbf, sites) of a named pair"""
    _, mb, mbf, sites = STEREO_PAIRS[name]
    I = stereo_inputs(oracle, name, fast)
    if mbf == "minU":
        mbf = minu_mbf(I)
    return I, mb, mbf, sites


_MODEL = {}


def stereo_model(oracle, name, wrong=None):
    if (name, wrong) not in _MODEL:
        I, mb, mbf, _ = stereo_case(oracle, name)
        _MODEL[(name, wrong)] = I.model(mb, mbf, wrong)
    return _MODEL[(name, wrong)]


# ---- planted keypoints on the level images of one real extraction (oracle only) --------------------------------------------------
def _flip(desc, k, start=0):
    """desc with the k bits start .. start + k - 1 flipped"""
    bits = np.unpackbits(np.asarray(desc, np.uint8))
    bits[start:start + k] ^= 1
    return np.packbits(bits)


def _half_coordinate(k, inv, lo, hi):
    """a float32 x in [lo, hi] with float32(x * inv) == k + 0.5 exactly"""
    x = F((k + 0.5) / float(inv))
    for _ in range(64):
        x = np.nextafter(x, F(-np.inf))
    for _ in range(128):
        if float(F(x * inv)) == k + 0.5 and lo <= x <= hi:
            return x
        x = np.nextafter(x, F(np.inf))
    raise AssertionError("no float32 maps to %d.5" % k)


class _Plant:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.L, self.R, self.pinned, self.site = [], [], {}, {}

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def left(self, name, x, y, octave, desc):
        self.site[name] = len(self.L)
        self.L.append((x, y, octave, desc))

    def right(self, x, y, octave, desc, at=None):
        if at is None:
            self.R.append((x, y, octave, desc))
        else:
            self.pinned[at] = (x, y, octave, desc)

    def pair(self, name, x, y, octave=0, flips=5, dx=6.0, r_octave=None, ry=None):
        d = self.desc()
        self.left(name, x, y, octave, d)
        self.right(F(x) - F(dx), y if ry is None else ry, octave if r_octave is None else r_octave, _flip(d, flips))

    def arrays(self, kp_dtype, filler_row=8.0):
        """right keypoints in planting order, the pinned ones at their positions, fillers (a row no left keypoint looks at) between"""
        n = max(len(self.R) + len(self.pinned), max(self.pinned, default=-1) + 1)
        free = iter(self.R)
        R = []
        for i in range(n):
            if i in self.pinned:
                R.append(self.pinned[i])
            else:
                R.append(next(free, None) or (F(30 + i), F(filler_row), 0, self.desc()))
        def pack(rows):
            k = np.zeros(len(rows), kp_dtype); d = np.zeros((len(rows), 32), np.uint8)
            for i, (x, y, o, dd) in enumerate(rows):
                k["x"][i], k["y"][i], k["octave"][i] = x, y, o
                k["size"][i] = 31.0; k["angle"][i] = 0.0; k["response"][i] = 50.0; k["class_id"][i] = -1
                d[i] = dd
            return k, d
        return pack(self.L) + pack(R)


PLANTED_MBF = 30.0              # mb = 1: maxD = 30, so the sites of the two columns (x about 70 and about 190) do not see each other


def planted_moved(oracle, fast=False):
    """Hand-set keypoints on the pair `right = left moved 6 pixels`.  Sites are 9 rows apart (a band reaches at most 4 rows) in two
    columns 120 pixels apart (maxD = 30).  Returns (inputs, expectations): name -> ("accepted" | "rejected", the reason)."""
    T = synth.texture_image(W + 16, H, seed=21)
    left = np.ascontiguousarray(T[:, :W])
    right = T[:, 6:6 + W] + np.random.default_rng(22).normal(0, 1.0, (H, W))       # (noise: the median norm must not be 0)
    right = np.clip(np.rint(right), 0, 255).astype(np.uint8)
    # the site `sad_tie`: a patch of period 2 along x, 11 columns wide on the left and 13 on the right, so that the shifts 0 and +2
    # both have a zero norm and the shifts -2 and +4 do not
    ty, tx = 150, 190
    stripes = np.random.default_rng(23).integers(0, 2, (11, 1)) * 120 + np.array([[40, 90]])[:, np.arange(13) % 2]
    left[ty - 5:ty + 6, tx - 5:tx + 6] = stripes[:, :11]
    right[ty - 5:ty + 6, tx - 6 - 5:tx - 6 + 8] = stripes
    I = StereoInputs(oracle, left, right, fast=fast)
    p = _Plant(7)
    inv1, sf1 = I.inv[1], I.sf[1]
    rows = iter([(x, float(y)) for y in range(24, 142, 9) for x in (70.0, 190.0)])
    nxt = lambda: next(rows)
    want = {}

    def site(name, verdict, why, *a, **k):
        want[name] = (verdict, why)
        p.pair(name, *a, **k)

    x, y = nxt(); site("plain", "accepted", "level 0, partner 6 px to the left", x, y)
    # x * inv == k + 0.5: roundf goes up, rintf to the even k
    even = lambda v: int(v * float(inv1)) // 2 * 2                   # (k even: rintf(k + 0.5) = k, roundf = k + 1)
    x, y = nxt(); site("half_uL", "accepted", "scaled uL at k + 0.5", _half_coordinate(even(x), inv1, x - 3, x + 3), y, octave=1)
    x, y = nxt(); site("half_vL", "accepted", "scaled vL at k + 0.5", x, _half_coordinate(even(y), inv1, y - 3, y + 3), octave=1)
    x, y = nxt(); d = p.desc(); xr = _half_coordinate(even(x - 6), inv1, x - 12, x - 3)
    want["half_uR0"] = ("any", "scaled uR0 at k + 0.5"); p.left("half_uR0", x, y, 1, d); p.right(xr, y, 1, _flip(d, 5))
    # the last columns of the level: endu = scaleduR0 + 11 >= cols rejects
    x, y = nxt(); site("endu_inside", "accepted", "scaleduR0 = cols - 12", 234.0, y)
    x, y = nxt(); site("endu_reject", "rejected", "scaleduR0 = cols - 11: endu >= cols", 234.0, y, dx=5.0)
    x, y = nxt(); site("left_patch_outside", "rejected", "the left patch leaves the level (OpenCV throws; skipped)", 236.0, y, dx=8.0)
    # rows
    want["row_outside"] = ("rejected", "vL >= rows"); d = p.desc(); p.left("row_outside", 70.0, 180.0, 0, d); p.right(64.0, 178.5, 0, _flip(d, 5))
    x, y = nxt(); site("band_hi_integer_l0", "accepted", "row == maxr == y + r exactly", x, y + 2.0, ry=y)
    x, y = nxt(); site("band_lo_integer_l0", "accepted", "row == minr == y - r exactly", x, y - 2.0, ry=y)
    x, y = nxt(); site("band_above_l0", "rejected", "row == maxr + 1", x, y + 3.0, ry=y)
    r1 = F(F(2.0) * sf1)
    x, y = nxt(); yr = F(F(y) - r1); assert float(F(yr + r1)) == y
    site("band_hi_integer_l1", "accepted", "level 1: y + r an integer, row == maxr", x, y, octave=1, ry=yr)
    x, y = nxt(); yr = F(F(y - 1) - r1); assert float(F(yr + r1)) == y - 1
    site("band_above_l1", "rejected", "level 1: row == maxr + 1", x, y, octave=1, ry=yr)
    x, y = nxt(); site("band_fraction", "accepted", "y + r = row - 0.75: ceil keeps the row, rounding does not", x, y + 3.0, ry=y + 0.25)
    # octaves
    x, y = nxt(); site("octave_plus_1", "accepted", "right octave = left + 1", x, y, r_octave=1)
    x, y = nxt(); site("octave_plus_2", "rejected", "right octave = left + 2", x, y, r_octave=2)
    x, y = nxt(); site("octave_minus_1", "accepted", "right octave = left - 1", x, y, octave=2, r_octave=1)
    # descriptor distances
    for dist, verdict in ((74, "accepted"), (75, "rejected"), (99, "rejected"), (100, "rejected")):
        x, y = nxt(); site("dist_%d" % dist, verdict, "best distance %d against thOrbDist = 75" % dist, x, y, flips=dist)
    # equal best distances at iR = 3 and iR = 67 (across the 64 lanes of a wavefront); the later one is 20 px further left
    x, y = nxt(); d = p.desc(); want["tie_3_67"] = ("accepted", "the candidate at iR = 3 wins the tie")
    p.left("tie_3_67", x, y, 0, d); p.right(F(x - 6), y, 0, _flip(d, 9), at=3); p.right(F(x - 26), y, 0, _flip(d, 9, 100), at=67)
    # shifts
    x, y = nxt(); site("shift_4", "accepted", "best shift + 4", x, y, dx=10.0)
    x, y = nxt(); site("shift_5", "rejected", "best shift + 5", x, y, dx=11.0)
    x, y = nxt(); yr = F(F(y) + r1); assert float(F(yr - r1)) == y
    site("band_lo_integer_l1", "accepted", "level 1: y - r an integer, row == minr", x, y, octave=1, ry=yr)
    x, y = nxt(); yr = F(F(y + 1) + r1); assert float(F(yr - r1)) == y + 1
    site("band_below_l1", "rejected", "level 1: row == minr - 1", x, y, octave=1, ry=yr)
    site("sad_tie", "accepted", "zero norms at the shifts 0 and +2: the first wins", float(tx), float(ty))
    kL, dL, kR, dR = p.arrays(oracle.KP_DTYPE)
    return I.with_keypoints(kL, dL, kR, dR), p.site, want


def planted_cut(oracle, fast=False):
    """Nine accepted matches at level 0 whose norms are set by hand: at each site one to four pixels of the right image's patch
    differ from the left's by a chosen amount, so the norm of the best shift is that amount.  The sites are where every other shift
    has a norm above 1500.  Norms 3, 5, 6, 8, 10 (the median, rank 9 / 2 = 4), 20, 21, 22, 400: thDist = 2.1f * 10 = 21.0 exactly in
    float (21 - 2^-20 is a tie between two floats and rounds to the even one), so the norm 21 EQUALS thDist: `21 < 21` is false and
    the match is taken back with 22 and 400, while 20 is kept."""
    norms = [3, 5, 6, 8, 10, 20, 21, 22, 400]
    T = synth.texture_image(W + 16, H, seed=21)
    left = np.ascontiguousarray(T[:, :W]); right = np.ascontiguousarray(T[:, 6:6 + W]).copy()
    A = np.abs(left[:, 1:].astype(np.int64) - left[:, :-1].astype(np.int64))
    # norm of a patch against itself moved by one pixel, a lower bound of what a textured site needs
    box = lambda a: np.array([[a[y - 5:y + 6, x - 5:x + 6].sum() for x in range(30, W - 30)] for y in range(20, H - 20)])
    tex = box(A)
    sites = []
    for y in range(24, 160, 12):
        xs = np.argsort(-tex[y - 20])
        x = int(next(v for v in xs if 40 <= v + 30 <= 200)) + 30
        sites.append((x, y))
    sites = sites[:len(norms)]
    for (x, y), n in zip(sites, norms):
        for k in range((n + 99) // 100):
            v = min(100, n - 100 * k)
            old = int(right[y + k, x - 6])
            right[y + k, x - 6] = old + v if old + v <= 255 else old - v
    I = StereoInputs(oracle, left, right, fast=fast)
    p = _Plant(9)
    for i, (x, y) in enumerate(sites):
        p.pair("norm_%d" % norms[i], float(x), float(y))
    kL, dL, kR, dR = p.arrays(oracle.KP_DTYPE)
    return I.with_keypoints(kL, dL, kR, dR), p.site, norms


# ---- knn2 ----------------------------------------------------------------------------------------------------------------------------
KNN_NQ = [0, 1, 4095, 4096, 4097, 16383, 16384, 16385]
KNN_NT = [0, 1, 2, 255, 256, 257, 300]


@functools.lru_cache(maxsize=None)
def knn_train(nt):
    """nt train rows; identical rows planted at j, j + 16, j + 32, j + 64 (j = 5) and at 255 / 256 (across the 256-row tile), where
    nt reaches that far"""
    t = np.random.default_rng(1000 + nt).integers(0, 256, (nt, 32), dtype=np.uint8)
    for j in (21, 37, 69):
        if j < nt: t[j] = t[5]
    if nt > 256: t[256] = t[255]
    return t


@functools.lru_cache(maxsize=None)
def knn_queries(nq, nt):
    """queries = train rows with k bits flipped: query i copies row (i * 37) % nt with i % 7 bits flipped.  The first query and every
    97th copy row 5 with two bits flipped, so the identical rows 5 / 21 / 37 / 69 tie for them; the last query copies row 255 with three
    bits flipped: the pair 255 / 256, across the tile."""
    rng = np.random.default_rng(2000 + nq)
    if nt == 0:
        return rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    src = (np.arange(nq) * 37) % nt
    i = np.arange(nq)[:, None]; pos = np.arange(256)[None, :]
    flips = (pos >= (i * 13) % 200) & (pos < (i * 13) % 200 + i % 7)
    q = np.packbits(np.unpackbits(knn_train(nt)[src], axis=1) ^ flips.astype(np.uint8), axis=1) if nq else knn_train(nt)[:0].copy()
    for i in range(0, nq, 97):
        q[i] = _flip(knn_train(nt)[5 if nt > 5 else 0], 2, 50)
    if nq and nt > 256:
        q[nq - 1] = _flip(knn_train(nt)[255], 3, 10)
    return q


def knn_scene(nq, nt):
    """(queries, train).  With nt > 256 and nq > 1, train row 0 is row nt - 1 with 3 bits flipped and query 1 is row nt - 1 itself:
    best in the last partial tile, second in the first."""
    t = knn_train(nt).copy(); q = knn_queries(nq, nt).copy()
    if nt > 256 and nt % 256 and nq > 1:
        t[0] = _flip(t[nt - 1], 3, 77)
        q[1] = t[nt - 1]
    return q, t


# ---- window_match --------------------------------------------------------------------------------------------------------------------
WINDOW_LENGTHS = [0, 1, 2, 63, 64, 65, 128, 129, 200]


@functools.lru_cache(maxsize=None)
def window_scene():
    """(q_desc, t_desc, cand_offsets, cand_idx, sites).  Per list length five queries: random distances; equal smallest distances at
    positions p and p + 64 (p = 1; and p, p + 1 where the list is shorter); the same train index twice as the two smallest; best
    equal to second at p, p + 1; a best late in the list with the second before it."""
    rng = np.random.default_rng(77)
    nt = 260
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    t[:8] = [_flip(base, k, 30) for k in (4, 4, 6, 6, 9, 9, 2, 3)]     # rows 0 / 1, 2 / 3, 4 / 5 are at equal distances from `base`
    q, offs, cand, sites = [], [0], [], {}
    far = lambda n: rng.integers(8, nt, n).tolist()
    for n in WINDOW_LENGTHS:
        lists = {"random": far(n)}
        c = far(n)
        if n >= 66: c[1], c[65] = 0, 1
        elif n >= 2: c[0], c[1] = 0, 1
        lists["tie_p_p64"] = c
        c = far(n)
        if n >= 2: c[0], c[n - 1] = 2, 2
        lists["same_index_twice"] = c
        c = far(n)
        if n >= 3: c[n - 2], c[n - 1] = 4, 5
        if n >= 3: c[0] = 6
        lists["tie_for_second"] = c
        c = far(n)
        if n >= 2: c[n - 1], c[0] = 6, 7
        lists["best_last"] = c
        for name, c in lists.items():
            sites[(n, name)] = len(q)
            q.append(base); cand.extend(c); offs.append(len(cand))
    return np.array(q, np.uint8), t, np.array(offs, np.int32), np.array(cand, np.int32), sites


def strided(desc, stride, lead=0):
    """the rows of desc `stride` bytes apart in one buffer (0xA5 between them), starting `lead` bytes in"""
    desc = np.asarray(desc, np.uint8)
    buf = np.full(lead + max(len(desc), 1) * stride + 32, 0xA5, np.uint8)
    for i, d in enumerate(desc):
        buf[lead + i * stride:lead + i * stride + 32] = d
    return buf


# ---- distinctive ---------------------------------------------------------------------------------------------------------------------
DISTINCTIVE_N = [1, 2, 3, 4, 5, 63, 64, 65, 66, 128, 129, 257]


@functools.lru_cache(maxsize=None)
def distinctive_scene():
    """(desc, offsets, names).  Per N: rows at distances d and d + 1 from row 0 -- (0 via a copy, 1), (1, 2), (127, 128), (254, 255),
    (255, 256 = the complement) --, so that both halves of one packed counter word fill; random rows; all rows identical; then
    the pairs whose order decides and empty points between."""
    rng = np.random.default_rng(91)
    pts, names = [], []

    def add(name, rows):
        names.append(name); pts.append(np.array(rows, np.uint8).reshape(-1, 32))

    for N in DISTINCTIVE_N:
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        for lo in (0, 1, 127, 254, 255):
            rows = [base] + [_flip(base, lo + (i % 2), 0) for i in range(1, N)]
            add("N%d_d%d_%d" % (N, lo, lo + 1), rows)
        add("N%d_random" % N, [_flip(base, int(k), int(s)) for k, s in zip(rng.integers(0, 60, N), rng.integers(0, 190, N))])
        add("N%d_identical" % N, [base] * N)
        add("empty_after_N%d" % N, [])
    z = np.zeros(32, np.uint8)
    # two rows with equal medians, the first wins; and the same rows in the other order
    a, b, c, d = _flip(z, 8), _flip(z, 8, 8), _flip(z, 16), z
    add("equal_medians", [a, b, d, c]); add("equal_medians_swapped", [b, a, c, d])
    # even N: index 0.5 * (N - 1) truncates to N / 2 - 1, which N / 2 would not: rows 0, 0, +10, +10 bits
    add("even_truncates_4", [z, _flip(z, 1), _flip(z, 40), _flip(z, 41)])
    add("even_truncates_6", [z, _flip(z, 1), _flip(z, 2), _flip(z, 40), _flip(z, 41), _flip(z, 42)])
    offs = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)
    return np.concatenate([p for p in pts if len(p)]), offs, names


# ---- sort_by_response ----------------------------------------------------------------------------------------------------------------
SORT_N = [1, 2, 255, 256, 257, 1500]


@functools.lru_cache(maxsize=None)
def response_scene(n):
    """n responses from eight values with 0.0 next to -0.0: with n > 8 every run of equal responses is long, and with n >= 257 the
    runs cross the 256-thread blocks of the launch"""
    rng = np.random.default_rng(500 + n)
    vals = np.array([0.0, -0.0, 3.5, 3.5, 20.0, -1.0, 1e-30, 7.0], F)
    r = vals[rng.integers(0, len(vals), n)]
    if n >= 2:
        r[0], r[n - 1] = F(0.0), F(-0.0)
    return r


def response_keypoints(kp_dtype, n):
    k = np.zeros(n, kp_dtype)
    k["response"] = response_scene(n)
    k["x"] = np.arange(n)
    return k
