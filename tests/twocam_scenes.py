"""Planted scenes for the three matchers of a two-camera frame (tests/twocam_model.py names the comparisons and the wrong variants).

As tests/match_scenes.py: a 240 x 180 frame, sites on the 24 px lattice, one comparison of the reference on its boundary per site;
both cameras' grids use the same lattice.  A query's descriptor is random and a candidate at Hamming distance k is the query with k
bits flipped; candidates that several queries see come from match_scenes._Cluster.

Indices.  The level gate of right keypoint j reads left keypoint j's octave (twocam_model.gate_levels), so the builder starts every
site at the same index in both cameras (the shorter list is padded with keypoints at the lattice's last site, where nothing
searches): right keypoint k of a site is gated by the octave of left keypoint k of that site, or, where the site has none, by a
padding keypoint of the octave the site asks for (`gate=`).

Worked example.  Both lists hold 10 keypoints when a site starts.  The site adds left keypoints of octaves 1 and 0 (left 10, 11)
and then a right keypoint of octave 1 with gate=1: it becomes right 10, gated by left 10 (octave 1), and nothing is padded.  A second
right keypoint of octave 1 with no `gate=` wants its own octave 1 as gate, but right 11 would read left 11 (octave 0): `kp` pads
right 11 with a keypoint at the empty site and appends the new one as right 12, which no left keypoint faces yet.  The next site pads
the left list to 13; `finish` sees that left 12 is padding, gives it octave 1, and asserts for every right keypoint that the left
keypoint of its index has the octave it wants.

Scenes are seeded, cached and read-only."""
import functools

import numpy as np

from oracle.oracle_py import KP_DTYPE
import match_model as mm
import match_scenes as ms
import twocam_model as tm

F = np.float32
W, H = ms.W, ms.H
SITES = ms.SITES
RATIOS = ms.RATIOS
KINDS = ("map", "last", "bow")
CELL = 3.75
MAX_KPS = 8192                                                                # kTcMaxKps
_OFF = [(0.0, 0.0), (1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0)]
_EMPTY = SITES[-1]


def ratio_equal_pair(r, th):
    """(best, second) with (float)best == (float)second * nnratio exactly and best <= th: the pair with the largest second"""
    out = [(b, s) for s in range(1, 256) for b in range(1, min(s, th) + 1) if F(b) == F(s) * F(r)]
    return out[-1] if out else None


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.K = ([], [])                                                     # left, right keypoints
        self.Q, self.names, self.free = [], [], list(SITES[:-1])
        self.links = []

    def rand_desc(self):
        return int.from_bytes(self.rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little")

    def flipped(self, d, k):
        return ms._flip(d, self.rng.permutation(256)[:k])

    def _pad(self, cam, octave=0):
        self.K[cam].append(dict(x=F(_EMPTY[0]), y=F(_EMPTY[1]), octave=octave, desc=self.rand_desc(), slot=-1, angle=0.0, pad=True))

    def site(self, name, at=None):
        assert self.free, "the lattice is full"
        c = self.free.pop(0 if at is None else self.free.index(at))
        while len(self.K[0]) < len(self.K[1]):
            self._pad(0)
        while len(self.K[1]) < len(self.K[0]):
            self._pad(1)
        self.name = name
        return c

    @staticmethod
    def _want(r):
        return r["octave"] if r.get("gate") is None else r["gate"]

    def kp(self, cam, c, desc, off=(0.0, 0.0), octave=0, slot=-1, gate=None, pos=None):
        """a keypoint of the current site -> its camera-local index.  A right keypoint without `gate=` is gated by its own octave:
        where the keypoint of the same index in the other camera says otherwise, padding moves the new one past it"""
        x, y = pos if pos is not None else (F(c[0] + off[0]), F(c[1] + off[1]))
        new = dict(x=F(x), y=F(y), octave=octave, desc=desc, slot=slot, angle=0.0, gate=gate)
        L, R = self.K
        if cam == 1:
            while len(R) < len(L) and not L[len(R)].get("pad") and L[len(R)]["octave"] != self._want(new):
                self._pad(1)
        else:
            while len(L) < len(R) and not R[len(L)].get("pad") and self._want(R[len(L)]) != octave:
                self._pad(0, self._want(R[len(L)]))
        self.K[cam].append(new)
        return len(self.K[cam]) - 1

    def link(self, l, r):
        self.links.append((l, r))

    def query(self, c, desc, **kw):
        q = dict(x=F(c[0]), y=F(c[1]), xr=F(c[0]), yr=F(c[1]), iv=1, ivr=1, level=0, level_r=None, vc=0.5, vcr=0.5, obs=0, desc=desc)
        q.update(kw)
        if q["level_r"] is None:
            q["level_r"] = q["level"]
        self.Q.append(q); self.names.append(self.name)
        return len(self.Q) - 1

    def simple(self, name, left=(), right=(), at=None, **q):
        """one query; per camera a list of distances or (distance, keypoint settings)"""
        c = self.site(name, at)
        d = self.rand_desc()
        for cam, spec in ((0, left), (1, right)):
            for k, e in enumerate(spec):
                dist, kw = e if isinstance(e, tuple) else (e, {})
                kw = dict(kw)
                kw.setdefault("off", _OFF[k]); kw.setdefault("octave", q.get("level", 0))
                self.kp(cam, c, self.flipped(d, dist), **kw)
        self.query(c, d, **q)
        return c

    def finish(self):
        """the arrays; the padding that the right keypoints' gates ask for"""
        L, R = self.K
        for j, r in enumerate(R):
            if r.get("pad"):
                continue
            want = self._want(r)
            while len(L) <= j:
                self._pad(0, want)
            if L[j].get("pad"):
                L[j]["octave"] = want
            assert L[j]["octave"] == want, "right keypoint %d wants gate %d, left keypoint %d has octave %d" % (j, want, j, L[j]["octave"])
        nL = len(L)
        kps = np.zeros(nL + len(R), KP_DTYPE)
        for f in ("x", "y", "octave", "angle"):
            kps[f] = [k[f] for k in L + R]
        kps["size"] = 31.0; kps["class_id"] = -1
        l2r = np.full(nL, -1, np.int32); r2l = np.full(len(R), -1, np.int32)
        for l, r in self.links:
            l2r[l] = r; r2l[r] = l
        Q = self.Q
        ones = np.ones(len(Q), np.float32)
        cam = lambda iv, x, y, lv, vc: (np.array([q[iv] for q in Q], np.uint8), np.array([[q[x], q[y]] for q in Q], np.float32).reshape(len(Q), 2),
                                        np.array([q[lv] for q in Q], np.int32), np.array([q[vc] for q in Q], np.float32), ones)
        q_kps = np.zeros(len(Q), KP_DTYPE)
        q_kps["x"] = [q["x"] for q in Q]; q_kps["y"] = [q["y"] for q in Q]; q_kps["octave"] = [q["level"] for q in Q]
        q_kps["size"] = 31.0; q_kps["class_id"] = -1
        sc = dict(kps=kps, nL=nL, desc=ms._to_u8([k["desc"] for k in L + R]), l2r=l2r, r2l=r2l, slot=np.array([k["slot"] for k in L + R], np.int32),
                  left=cam("iv", "x", "y", "level", "vc"), right=cam("ivr", "xr", "yr", "level_r", "vcr"),
                  q_desc=ms._to_u8([q["desc"] for q in Q]), q_obs=np.array([q["obs"] for q in Q], np.uint8), q_kps=q_kps, q_ls=ones,
                  names=np.array(self.names), n_sites=len(SITES) - 1 - len(self.free))
        return sc


def _freeze(sc):
    for a in sc.values():
        for b in (a if isinstance(a, tuple) else (a,)):
            if isinstance(b, np.ndarray):
                b.setflags(write=False)
    return sc


def _common_sites(b, th, radius_l, radius_r):
    """the sites both projection forms have: thresholds, ties, window edges, occupancy, on both cameras"""
    for side in ("left", "right"):
        other = "right" if side == "left" else "left"
        for d in (th - 1, th, th + 1):
            b.simple("threshold %s: lone candidate at %d" % (side, d), **{side: [d], other: [(30, {})] if side == "right" else []})
        b.simple("tie %s: three cells that differ in ix" % side, **{side: [(20, dict(off=o)) for o in ((0, 0), (CELL, 0), (-CELL, 0))], other: [30]})
        b.simple("tie %s: three cells that differ in iy" % side, **{side: [(20, dict(off=o)) for o in ((0, 0), (0, CELL), (0, -CELL))], other: [30]})
        b.simple("tie %s: one cell" % side, **{side: [(20, dict(off=o)) for o in ((0, 0), (0.25, 0), (0, 0.25))], other: [30]})
        b.simple("occupancy %s: slot -2" % side, **{side: [(10, dict(slot=-2)), 30], other: [35]})
        b.simple("occupancy %s: slot -3" % side, **{side: [(10, dict(slot=-3))], other: [35]})
    gb = mm.frame(np.zeros(0, KP_DTYPE), [], W, H).gb
    for side, r in (("left", radius_l if radius_l >= 8 else 2 * radius_l), ("right", radius_r)):
        if r < 8:
            continue                                                        # (the second candidate lies up to 5 px from the site)
        c = next(c for c in b.free if ms._half_cell(gb, c[0], 0)[0] is not None)
        x, k = ms._half_cell(gb, c[0], 0)
        b.simple("grid %s: a tie whose second candidate has cell coordinate %d.5 in x" % (side, k), at=c,
                 **{side: [(20, dict(pos=(F(CELL * (k + 1)), F(c[1])))), (20, dict(pos=(x, F(c[1]))))], "right" if side == "left" else "left": [30]})
    # |dx| == r and the float inside, per camera (the left radius is radius_l, the right radius_r)
    for side, r in (("left", radius_l), ("right", radius_r)):
        for inside in (False, True):
            c = b.free[0]
            edge = F(c[0] + r)
            x = np.nextafter(edge, F(0)) if inside else edge
            assert (abs(F(x - F(c[0]))) == r) == (not inside)
            b.simple("window %s: %s" % (side, "x the float below x + r" if inside else "|dx| == r"),
                     **{side: [(10, dict(pos=(x, F(c[1])))), (40, {"off": (0.0, 1.0)})], "right" if side == "left" else "left": [30]})


@functools.lru_cache(maxsize=None)
def map_scene():
    """SearchByProjection(F, map points): every query has viewing cosine 0.5 (r = 4) and level scale 1 unless its site says otherwise;
    run with th 1 and 2, so the left radius is 4 or 8 and the right radius 4"""
    b = _Builder(301)
    th = mm.TH_HIGH
    _common_sites(b, th, 4.0, 4.0)
    for r in RATIOS:
        p = ratio_equal_pair(r, th)
        if p is None:                                                       # (1.5: best <= second leaves no equality)
            continue
        for side in ("left", "right"):
            b.simple("ratio %s %.1f: best %d == nnratio * %d" % ((side, r) + p), **{side: list(p)})
        b.simple("ratio right %.1f: best %d == nnratio * %d, gates differ" % ((r,) + p), right=[(p[0], dict(octave=1, gate=1)), (p[1], dict(octave=1, gate=0))],
                 level=1, iv=0)
    for side in ("left", "right"):
        b.simple("ratio %s: 40 against 41 on another level" % side, **{side: [(40, dict(octave=1)), (41, dict(octave=0))]}, level=1)
        b.simple("ratio %s: 40 against 41" % side, **{side: [40, 41]})
        b.simple("levels %s: octaves 0..3 around level 2" % side, **{side: [(d, dict(octave=o)) for d, o in ((10, 0), (20, 1), (30, 2), (5, 3))]}, level=2)
    b.simple("right levels: own octaves equal, gate octaves differ", right=[(40, dict(octave=1, gate=1)), (41, dict(octave=1, gate=0))], level=1, iv=0)
    b.simple("right levels: own octaves differ, gate octaves equal", right=[(40, dict(octave=1, gate=1)), (41, dict(octave=0, gate=1))], level=1, iv=0)
    b.simple("right gate: own octave 1 passes, gate octave 3 does not", right=[(10, dict(octave=1, gate=3)), (40, dict(octave=1, gate=1))], level=1, iv=0)
    b.simple("right gate: own octave 3 does not pass, gate octave 1 does", right=[(10, dict(octave=3, gate=1)), (40, dict(octave=1, gate=1))], level=1, iv=0)
    D = mm.first_dist(th, 0.9, True)                                       # (the bound a pruning walk may use; `second_cut` is that bound off by one)
    for side in ("left", "right"):
        b.simple("first_dist %s: best %d, second %d" % (side, th, D - 1), **{side: [th, D - 1]})
    b.simple("left ratio-rejected, the right sub-query would match", left=[40, 41], right=[10])
    b.simple("th: a right candidate between r and th r", left=[30], right=[(10, dict(off=(6.0, 0.0)))])
    b.simple("th: a left candidate between r and th r", left=[(10, dict(off=(6.0, 0.0)))], right=[30])
    b.simple("right level -1", left=[30], right=[10], level_r=-1)
    b.simple("right in view only", right=[10], iv=0)
    b.simple("left in view only", left=[10], right=[10], ivr=0)
    for vc, tag in ((ms.VIEW_COS_EDGE, "(float)0.998"), (float(np.nextafter(F(0.998), F(0))), "the float below (float)0.998"),
                    (float(np.nextafter(F(0.998), F(1))), "the float above (float)0.998")):
        b.simple("viewing cosine left " + tag, left=[(10, dict(off=(6.0, 0.0))), (20, dict(off=(3.0, 0.0)))], vc=vc, ivr=0)
        b.simple("viewing cosine right " + tag, right=[(20, dict(off=(3.0, 0.0)))], vcr=vc, iv=0)
    # ---- partner links
    for obs in (1, 0):
        c = b.site("partner: a left match claims right A', obs %d; a right-only query then finds A' best" % obs)
        cl = ms._Cluster(b, 3, 30)
        A = b.kp(0, c, cl.desc[0]); A_ = b.kp(1, c, cl.desc[1]); b.kp(1, c, cl.desc[2], off=_OFF[1]); b.link(A, A_)
        b.query(c, cl.query({0: 10}), ivr=0, obs=obs); b.query(c, cl.query({1: 10, 2: 50}), iv=0)
        c = b.site("partner: a right match claims left A, obs %d; a left-only query then finds A best" % obs)
        cl = ms._Cluster(b, 3, 30)
        A = b.kp(0, c, cl.desc[0]); b.kp(0, c, cl.desc[2], off=_OFF[1]); A_ = b.kp(1, c, cl.desc[1]); b.link(A, A_)
        b.query(c, cl.query({1: 10}), iv=0, obs=obs); b.query(c, cl.query({0: 10, 2: 50}), ivr=0)
    c = b.site("partner: a linked and an unlinked keypoint side by side, both cameras")
    cl = ms._Cluster(b, 4, 20)
    A = b.kp(0, c, cl.desc[0]); b.kp(0, c, cl.desc[1], off=_OFF[1]); A_ = b.kp(1, c, cl.desc[2]); b.kp(1, c, cl.desc[3], off=_OFF[1]); b.link(A, A_)
    b.query(c, cl.query({1: 10, 0: 30}), ivr=0, obs=1); b.query(c, cl.query({3: 10, 2: 30}), iv=0, obs=1); b.query(c, cl.query({0: 10, 2: 30}), obs=1)
    k = 0
    while b.free:
        b.simple("plain %d" % k, left=[10 + k], right=[12 + k]); k += 1
    return _freeze(b.finish())


LAST_TH = 8.0


@functools.lru_cache(maxsize=None)
def last_scene():
    """SearchByProjection(CurrentFrame, LastFrame): th = 8 and level scale 1, so both radii are 8; run in the three modes"""
    b = _Builder(302)
    th = mm.TH_HIGH
    _common_sites(b, th, 8.0, 8.0)
    b.simple("empty left window, the right window matches", right=[10])
    b.simple("left window all closed, the right window matches", left=[(10, dict(slot=-2))], right=[10])
    b.simple("right projection far outside the image", left=[10], right=[10], xr=F(-3000.0), yr=F(5000.0))
    c = b.free[0]
    b.simple("right projection outside, its window reaches column 0", left=[10], right=[(10, dict(pos=(F(0.25), F(c[1]))))], xr=F(-7.5))
    for side in ("left", "right"):
        b.simple("levels %s: octaves 0..4 around level 2" % side, **{side: [(d, dict(octave=o)) for d, o in ((10, 0), (20, 1), (30, 2), (25, 3), (5, 4))],
                                                                       "left" if side == "right" else "right": [(40, dict(octave=2))]}, level=2)
    b.simple("right gate: own octave 2 passes every mode, gate octave 5 only forward", left=[(40, dict(octave=2))],
             right=[(10, dict(octave=2, gate=5)), (30, dict(octave=2, gate=2))], level=2)
    b.simple("right gate: own octave 5, gate octave 2", left=[(40, dict(octave=2))], right=[(10, dict(octave=5, gate=2)), (30, dict(octave=2, gate=2))], level=2)
    for cam in (0, 1):
        side = "LR"[cam]
        c = b.site("chain %s: slot overwritten by a later unobserved query" % side)
        cl = ms._Cluster(b, 2, 30); b.kp(cam, c, cl.desc[0]); b.kp(1 - cam, c, cl.desc[1])
        b.query(c, cl.query({0: 40, 1: 30})); b.query(c, cl.query({0: 60, 1: 110}))
        c = b.site("chain %s: slot closed by an observed query" % side)
        cl = ms._Cluster(b, 3, 25); b.kp(cam, c, cl.desc[0]); b.kp(cam, c, cl.desc[1], off=_OFF[1]); b.kp(1 - cam, c, cl.desc[2])
        b.query(c, cl.query({0: 40, 2: 30}), obs=1); b.query(c, cl.query({0: 31, 1: 61, 2: 81}))
    k = 0
    while b.free:
        b.simple("plain %d" % k, left=[10 + k], right=[12 + k]); k += 1
    return _freeze(b.finish())


# ---------------------------------------------------------------------------------------------------
# the sizes: small scenes around one loop of the walk each
@functools.lru_cache(maxsize=None)
def wide_scene():
    """a window of more than 64 cells: radius 36 (a level scale of 9 on r = 4 and on th = 4) around (120, 90) covers 21 x 21 cells.  Equal best distances in the first cell of the window's cell order, in the cell 64 places later (ix-major) and beyond, in
    both cameras; a second query whose only tie lies in the later cells"""
    b = _Builder(303)
    c = b.site("window of more than 64 cells", at=SITES[34])
    cx, cy = F(120.0), F(90.0)
    gb = mm.frame(np.zeros(0, KP_DTYPE), [], W, H).gb
    cr = mm.ei.cell_range_rule(cx, cy, F(36.0), gb)
    nx, ny = cr[1] - cr[0] + 1, cr[3] - cr[2] + 1
    assert nx >= 9 and ny >= 8 and nx * ny > 64

    def cell_pos(order):
        """a place in cell `order` of the window's cell order (ix-major) that lies inside the window"""
        ix, iy = cr[0] + order // ny, cr[2] + order % ny
        return F(84.2) if ix == cr[0] else F(ix * CELL), F(54.2) if iy == cr[2] else F(iy * CELL)
    d1, d2 = b.rand_desc(), b.rand_desc()
    places = [0, 64, 128, 200]
    for cam in (0, 1):
        for o in reversed(places):                                          # (the later cells get the lower indices)
            b.kp(cam, c, b.flipped(d1, 20), pos=cell_pos(o))
        for o in places[1:3]:
            b.kp(cam, c, b.flipped(d2, 25), pos=cell_pos(o + 2))
        for o in range(3, nx * ny - ny, 17):                                # a sprinkle of far candidates over the whole window
            p = cell_pos(o)
            if abs(float(p[0]) - 120) < 36 and abs(float(p[1]) - 90) < 36:
                b.kp(cam, c, b.flipped(d1, 90 + o % 40), pos=p)
    b.query((cx, cy), d1, x=cx, y=cy, xr=cx, yr=cy); b.query((cx, cy), d2, x=cx, y=cy, xr=cx, yr=cy)
    sc = b.finish()
    nine = np.full(2, 9.0, np.float32)
    sc["left"], sc["right"], sc["q_ls"] = sc["left"][:4] + (nine,), sc["right"][:4] + (nine,), nine
    sc["th_map"], sc["th_last"] = 1.0, 4.0
    fr = mm.frame(sc["kps"], sc["desc"], W, H)
    assert sum(abs(fr.x[i] - 120) < 36 and abs(fr.y[i] - 90) < 36 for i in range(fr.N)) >= 30
    return _freeze(sc)


@functools.lru_cache(maxsize=None)
def crowded_scene():
    """a cell of more than 64 keypoints, in both cameras: 140 keypoints in the cell of site 0, equal best distances at places 3, 67 and
    131 of the cell for one query and at 70 and 134 for another"""
    b = _Builder(304)
    c = b.site("cell of 140 keypoints")
    d1, d2 = b.rand_desc(), b.rand_desc()
    for cam in (0, 1):
        for k in range(140):
            pos = (F(c[0] + 0.01 * (k % 50)), F(c[1] + 0.01 * (k // 50)))
            desc = b.flipped(d1, 20) if k in (3, 67, 131) else b.flipped(d2, 25) if k in (70, 134) else b.flipped(d1 if k % 2 else d2, 60 + k % 35)
            b.kp(cam, c, desc, pos=pos)
    b.query(c, d1); b.query(c, d2)
    sc = b.finish()
    sc["th_map"], sc["th_last"] = 1.0, 4.0
    fr = mm.frame(sc["kps"][:sc["nL"]], sc["desc"][:sc["nL"]], W, H)
    assert len({mm.ei.pos_in_grid(fr.x[i], fr.y[i], fr.gb, None) for i in range(140)}) == 1
    return _freeze(sc)


@functools.lru_cache(maxsize=None)
def full_scene(n=MAX_KPS):
    """n keypoints over both cameras at random places (5 000 left when n is the walk's capacity) with random descriptors, and eight
    queries that each have a planted left and right candidate, two of them linked"""
    rng = np.random.default_rng(305)
    nL = n * 5000 // MAX_KPS
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = rng.uniform(1, W - 1, n).astype(np.float32); kps["y"] = rng.uniform(1, H - 1, n).astype(np.float32)
    kps["octave"] = 0; kps["size"] = 31.0; kps["class_id"] = -1
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    nq = 8
    q_desc = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    l2r = np.full(nL, -1, np.int32); r2l = np.full(n - nL, -1, np.int32)
    xy = np.array([SITES[7 * k] for k in range(nq)], np.float32)
    for k in range(nq):
        l, r = (nL - 1 - k, n - nL - 1 - k) if k % 2 else (k, k)             # the first and the last indices of both cameras
        for gi, dist in ((l, 20 + k), (nL + r, 30 + k)):
            bits = np.unpackbits(q_desc[k]); bits[rng.permutation(256)[:dist]] ^= 1
            desc[gi] = np.packbits(bits); kps["x"][gi], kps["y"][gi] = xy[k]
        if k < 2:
            l2r[l] = r; r2l[r] = l
    ones = np.ones(nq, np.float32)
    cam = (np.ones(nq, np.uint8), xy, np.zeros(nq, np.int32), np.full(nq, 0.5, np.float32), ones)
    q_kps = np.zeros(nq, KP_DTYPE); q_kps["x"] = xy[:, 0]; q_kps["y"] = xy[:, 1]; q_kps["size"] = 31.0; q_kps["class_id"] = -1
    slot = np.full(n, -1, np.int32); slot[5::97] = -2; slot[11::89] = -3
    return _freeze(dict(kps=kps, nL=nL, desc=desc, l2r=l2r, r2l=r2l, slot=slot, left=cam, right=cam, q_desc=q_desc, q_obs=np.ones(nq, np.uint8),
                        q_kps=q_kps, q_ls=ones, th_map=1.0, th_last=4.0))


def one_camera(sc, which):
    """the scene with nL = 0 (which = "right": the right keypoints alone), nR = 0 ("left") or no query ("none")"""
    sc = dict(sc)
    nL, n = sc["nL"], len(sc["kps"])
    if which == "none":
        cut = lambda a: a[:0]
        sc["left"] = tuple(cut(a) for a in sc["left"]); sc["right"] = tuple(cut(a) for a in sc["right"])
        for k in ("q_desc", "q_obs", "q_kps", "q_ls"):
            sc[k] = sc[k][:0]
        sc["slot"] = np.where(sc["slot"] >= 0, -1, sc["slot"])
        return sc
    sl = slice(0, nL) if which == "left" else slice(nL, n)
    for k in ("kps", "desc", "slot"):
        sc[k] = sc[k][sl]
    sc["nL"] = nL if which == "left" else 0
    sc["l2r"] = np.full(sc["nL"], -1, np.int32); sc["r2l"] = np.full(len(sc["kps"]) - sc["nL"], -1, np.int32)
    return sc


# ---------------------------------------------------------------------------------------------------
# calls
def configs(kind):
    if kind == "map":
        return [dict(ratio=r, th=2.0) for r in RATIOS] + [dict(ratio=0.9, th=1.0)]
    if kind == "last":
        return [dict(mode=m) for m in (0, 1, 2)]
    return [dict(ratio=r) for r in RATIOS]


MAIN = {"map": dict(ratio=0.9, th=2.0), "last": dict(mode=0), "bow": dict(ratio=0.9)}
config_id = ms.config_id
same = ms.same


def _th(sc, cfg, kind):
    return sc.get("th_" + kind, cfg.get("th", 1.0) if kind == "map" else LAST_TH)


def run_model(kind, sc, cfg, check_ori=True, wrong=None, info=None):
    if kind == "bow":
        return tm.search_by_bow_twocam(sc["kf_kps"], sc["kf_desc"], sc["kf_has_mp"], sc["kf_fv"], sc["kps"], sc["nL"], sc["desc"], sc["fv"], cfg["ratio"],
                                       check_ori, wrong, info)
    Fr = tm.twocam_frame(sc["kps"], sc["desc"], sc["nL"], W, H)
    if kind == "map":
        return tm.search_by_projection_map_twocam(Fr, sc["l2r"], sc["r2l"], sc["left"], sc["right"], sc["q_desc"], sc["q_obs"], sc["slot"], _th(sc, cfg, kind),
                                                  cfg["ratio"], wrong, info)
    return tm.search_by_projection_last_twocam(Fr, sc["q_kps"], sc["left"][0], sc["left"][1], sc["right"][1], sc["q_desc"], sc["q_obs"], sc["slot"],
                                               _th(sc, cfg, kind), sc["q_ls"], cfg["mode"], check_ori, wrong, info)


def run_oracle(oracle, kind, sc, cfg, check_ori=True, fast=False):
    if kind == "bow":
        return oracle.search_by_bow_fisheye(sc["kf_kps"], sc["kf_desc"], sc["kf_has_mp"], sc["kf_fv"], sc["kps"], sc["nL"], sc["desc"], sc["fv"], cfg["ratio"],
                                            check_ori, fast=fast)
    gb = oracle.grid_bounds(W, H)
    if kind == "map":
        return oracle.search_by_projection_map_fisheye(sc["kps"], sc["nL"], sc["desc"], gb, sc["l2r"], sc["r2l"], sc["left"], sc["right"], sc["q_desc"],
                                                       sc["q_obs"], sc["slot"], _th(sc, cfg, kind), cfg["ratio"], fast=fast)
    return oracle.search_by_projection_last_fisheye(sc["kps"], sc["nL"], sc["desc"], gb, sc["q_kps"], sc["left"][0], sc["left"][1], sc["right"][1], sc["q_desc"],
                                                    sc["q_obs"], sc["slot"], _th(sc, cfg, kind), sc["q_ls"], cfg["mode"], check_ori, fast=fast)


def run_kernels(fe, ctx, kind, sc, cfg, check_ori=True):
    if kind == "bow":
        return fe.SearchByBoWFisheye(sc["kf_kps"], sc["kf_desc"], sc["kf_has_mp"], sc["kf_fv"], sc["kps"], sc["nL"], sc["desc"], sc["fv"], cfg["ratio"], check_ori,
                                     ctx=ctx)
    gb = fe.grid_bounds(W, H)
    m = fe.ORBmatcher(cfg.get("ratio", 0.9), check_ori, ctx)
    if kind == "map":
        return m.SearchByProjectionMapFisheye(sc["kps"], sc["nL"], sc["desc"], sc["l2r"], sc["r2l"], gb, sc["left"], sc["right"], sc["q_desc"], sc["q_obs"],
                                              sc["slot"], _th(sc, cfg, kind))
    return m.SearchByProjectionLastFisheye(sc["kps"], sc["nL"], sc["desc"], gb, sc["q_kps"], sc["left"][0], sc["left"][1], sc["right"][1], sc["q_desc"],
                                           sc["q_obs"], sc["slot"], _th(sc, cfg, kind), sc["q_ls"], cfg["mode"])


# ---------------------------------------------------------------------------------------------------
# SearchByBoW(KF, F): one vocabulary node per site
@functools.lru_cache(maxsize=None)
def bow_scene():
    """A node's feature list is ascending (FeatureVector::addFeature in keypoint order), so inside a node the left features come before
    the right ones; across the nodes the two sides alternate.  Every KeyFrame feature holds a map point unless its node says otherwise."""
    rng = np.random.default_rng(306)
    b = _Builder(306)
    TH = mm.TH_LOW
    nodes = []                                                              # (name, [KeyFrame descriptors], [left descriptors], [right descriptors], has_mp)

    def node(name, left=(), right=(), has_mp=1):
        d = b.rand_desc()
        nodes.append((name, [d], [b.flipped(d, k) for k in left], [b.flipped(d, k) for k in right], has_mp))
    for lb in (TH - 1, TH, TH + 1):
        for rb in (TH, TH + 1):
            node("left best %d, right best %d" % (lb, rb), [lb], [rb])
    for r in RATIOS:
        p = ratio_equal_pair(r, TH)
        if p is not None:
            node("left ratio %.1f: best %d == nnratio * %d, a right best of 10" % ((r,) + p), list(p), [10])
            node("right ratio %.1f: best %d == nnratio * %d under a left best of 10" % ((r,) + p), [10], list(p))
    node("left 40 against 41, a right best of 10", [40, 41], [10])
    node("right 20 against 20 under a left best of 10", [10], [20, 20])
    node("left 20 against 20, a right best of 10", [20, 20], [10])
    node("left best 60, a right best of 10", [60], [10])
    node("no left feature, a right best of 10", [], [10])
    node("no right feature", [10], [])
    node("equal distances across the sides", [20], [20])
    node("equal distances across the sides, the right one twice", [30], [30, 30])
    node("no map point", [10], [10], has_mp=0)
    cl = ms._Cluster(b, 4, 5)                                              # two KeyFrame features compete for one frame feature, through either side
    nodes.append(("two KeyFrame features, one left and one right frame feature each wants", [cl.query({0: 10, 2: 12}), cl.query({0: 8, 1: 14, 2: 10, 3: 16})],
                  [cl.desc[0], cl.desc[1]], [cl.desc[2], cl.desc[3]], 1))
    d = b.rand_desc()                                                       # a node of more than 64 frame features, ties on both sides
    nodes.append(("node of 80 frame features", [d], [b.flipped(d, 20 if k in (5, 37) else 60 + k) for k in range(40)],
                  [b.flipped(d, 22 if k in (2, 39) else 70 + k) for k in range(40)], 1))
    for k in range(24):
        node("plain %d" % k, [10 + k], [12 + k])
    kf_desc, kf_has, left, right = [], [], [], []
    for name, kd, ld, rd, hm in nodes:
        kf_desc += kd; kf_has += [hm] * len(kd); left += ld; right += rd
    nL = len(left)
    fv_nodes, fv_off, fv_idx, kfv_off, kfv_idx = [], [0], [], [0], []
    names, l_at, r_at, k_at = [], 0, 0, 0
    for j, (name, kd, ld, rd, hm) in enumerate(nodes):
        fv_nodes.append(3 * j + 1)
        fv_idx += list(range(l_at, l_at + len(ld))) + list(range(nL + r_at, nL + r_at + len(rd)))
        kfv_idx += list(range(k_at, k_at + len(kd)))
        l_at += len(ld); r_at += len(rd); k_at += len(kd)
        fv_off.append(len(fv_idx)); kfv_off.append(len(kfv_idx)); names += [name] * len(kd)
    mk = lambda n: np.zeros(n, KP_DTYPE)
    f_kps, kf_kps = mk(len(left) + len(right)), mk(len(kf_desc))
    for a in (f_kps, kf_kps):
        a["x"] = rng.uniform(1, W - 1, len(a)); a["y"] = rng.uniform(1, H - 1, len(a)); a["size"] = 31.0; a["class_id"] = -1
    nid = np.array(fv_nodes, np.uint32)
    return _freeze(dict(kf_kps=kf_kps, kf_desc=ms._to_u8(kf_desc), kf_has_mp=np.array(kf_has, np.uint8), kf_fv=(nid, np.array(kfv_off, np.int32), np.array(kfv_idx, np.int32)),
                        kps=f_kps, nL=nL, desc=ms._to_u8(left + right), fv=(nid, np.array(fv_off, np.int32), np.array(fv_idx, np.int32)), names=np.array(names)))


def bow_no_query():
    """the BoW scene with no KeyFrame feature holding a map point (nq = 0)"""
    sc = dict(bow_scene())
    sc["kf_has_mp"] = np.zeros_like(sc["kf_has_mp"])
    return sc


def bow_one_side(which):
    """the BoW scene with every frame feature counted as right (nL = 0) or left (nR = 0)"""
    sc = dict(bow_scene())
    sc["nL"] = 0 if which == "right" else len(sc["kps"])
    return sc


# ---------------------------------------------------------------------------------------------------
# the rotation histogram
def histogram_applies(name, kind):
    """the map form has no histogram; nothing steals; only the last-frame form writes a slot twice"""
    return kind != "map" and name != "stolen" and (name != "pushed twice" or kind == "last")


@functools.lru_cache(maxsize=None)
def histogram_scene(kind, name):
    """the scene cut down to the sites that give 30 to 32 pushes under the MAIN configuration (what match_scenes.with_angles plans
    for; the chain sites first), with the angles of match_scenes.HISTOGRAMS[name].  A query left out is not valid / holds no map point."""
    sc = dict(last_scene() if kind == "last" else bow_scene())
    info = {}
    run_model(kind, sc, MAIN[kind], True, None, info)
    per = {}
    for q, _ in info["pushes"]:
        per[sc["names"][q]] = per.get(sc["names"][q], 0) + 1
    order = sorted(per, key=lambda s_: (not s_.startswith("chain"), list(sc["names"]).index(s_)))
    keep, total = set(), 0
    for s_ in order:
        if total + per[s_] <= 32:
            keep.add(s_); total += per[s_]
    on = np.array([n in keep for n in sc["names"]], np.uint8)
    if kind == "last":
        sc["left"] = (sc["left"][0] & on,) + sc["left"][1:]
    else:
        sc["kf_has_mp"] = sc["kf_has_mp"] & on
    info = {}
    run_model(kind, sc, MAIN[kind], True, None, info)
    pushes = info["pushes"]
    assert 30 <= len(pushes) <= 32, len(pushes)
    slots = [c for _, c in pushes]
    twice = next((q for q, c in pushes if slots.count(c) == 2), None)
    qk = "q_kps" if kind == "last" else "kf_kps"
    sc[qk], sc["kps"] = ms.with_angles(sc[qk], sc["kps"], pushes, name, (), twice)
    sc["n_pushes"] = len(pushes)
    return _freeze(sc)


# ---------------------------------------------------------------------------------------------------
# every scene of a matcher, by name: what both test files run
BASE = {"map": map_scene, "last": last_scene, "bow": bow_scene}


def scenes(kind):
    """(name, scene) of every scene of a matcher"""
    out = [("base", BASE[kind]())]
    if kind != "bow":
        out += [("wide", wide_scene()), ("crowded", crowded_scene())]
        out += [("%s: %s only" % (n, w), one_camera(sc, w)) for n, sc in out[:2] for w in ("left", "right")] + [("base: no query", one_camera(out[0][1], "none"))]
    else:
        out += [("every feature %s" % w, bow_one_side(w)) for w in ("left", "right")]
        out += [("bow: no query", bow_no_query())]
    out += [(h, histogram_scene(kind, h)) for h in ms.HISTOGRAMS if histogram_applies(h, kind)]
    return out


def scene_names(kind):
    names = ["base"] + (["wide", "crowded", "base: left only", "base: right only", "wide: left only", "wide: right only", "base: no query"] if kind != "bow"
                        else ["every feature left", "every feature right", "bow: no query"])
    return names + [h for h in ms.HISTOGRAMS if histogram_applies(h, kind)]


CASES = [(k, n) for k in KINDS for n in scene_names(k)]
