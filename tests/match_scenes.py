"""Planted scenes for the descriptor matchers: every site puts one comparison of the reference on its boundary (tests/match_model.py
names the comparisons and their wrong variants).

Window matchers: a 240 x 180 frame with its own grid bounds; sites on a lattice 24 px apart (x = 12 + 24 i, y = 12 + 24 j) and a search
radius of 8, so that no site sees another site's candidates.  A query's descriptor is random; a candidate at Hamming distance k is the
query with k chosen bits flipped.  Where queries share candidates, the candidates are a common base with disjoint bit sets P_k flipped
and a query flips parts of the P_k plus bits of its own, which gives it the wanted distance to each.

Node-walk matchers: one vocabulary node per site.

Scenes are seeded, cached and read-only."""
import functools
import math

import numpy as np

from oracle.oracle_py import KP_DTYPE
import match_model as mm

F = np.float32
W, H = 240, 180
RADIUS = 8
SITES = [(12 + 24 * i, 12 + 24 * j) for j in range(7) for i in range(10)]
RATIOS = (0.9, 0.6, 0.5, 1.0, 1.5)
KINDS = ("init", "last", "kf", "map")
TH = {"init": mm.TH_LOW, "last": mm.TH_HIGH, "kf": 80, "map": mm.TH_HIGH}            # kf: the ORBdist of the calls
VIEW_COS_EDGE = float(F(0.998))
_OFFSETS = [(0.0, 0.0), (1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0)]


def _flip(d, bits):
    for b in bits:
        d ^= 1 << int(b)
    return d


def _to_u8(ints):
    return np.array([list(int(d).to_bytes(32, "little")) for d in ints], np.uint8).reshape(len(ints), 32)


class _Cluster:
    """candidates that several queries see: a base with disjoint bit sets P_k (|P_k| = p) flipped; two candidates are 2 p apart"""

    def __init__(self, b, n, p):
        perm = [int(v) for v in b.rng.permutation(256)]
        self.base = b.rand_desc()
        self.P = [perm[k * p:(k + 1) * p] for k in range(n)]
        self.spare = perm[n * p:]
        self.p = p
        self.desc = [_flip(self.base, P) for P in self.P]

    def query(self, want):
        """a descriptor at distance want[k] of candidate k; a candidate not named lies at p + T"""
        p = self.p
        for T in range(0, 200):
            x = {k: (p + T - d) / 2.0 for k, d in want.items()}
            if any(v != int(v) or v < 0 or v > p for v in x.values()):
                continue
            e = T - sum(int(v) for v in x.values())
            if 0 <= e <= len(self.spare):
                bits = list(self.spare[:e])
                for k, v in x.items():
                    bits += self.P[k][:int(v)]
                q = _flip(self.base, bits)
                assert all(mm.hamming(q, self.desc[k]) == d for k, d in want.items())
                return q
        raise AssertionError("no descriptor at distances %r" % (want,))


class _Window:
    def __init__(self, kind, seed):
        self.kind, self.th = kind, TH[kind]
        self.rng = np.random.default_rng(seed)
        self.used, self.free = 0, list(SITES[:-1])                          # (the last site stays empty for the plain queries)
        self.S, self.blocks, self.names = [], [], []

    def rand_desc(self):
        return int.from_bytes(self.rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little")

    def site(self, name, at=None):
        assert self.free, "the lattice is full"
        c = self.free.pop(0 if at is None else self.free.index(at))
        self.used += 1
        self.names.append(name)
        self.blocks.append(dict(name=name, queries=[], repeat=None))
        return c

    def cand(self, c, off, desc, octave=0, orb=1, ur=-1.0, slot=-1, pos=None):
        x, y = pos if pos is not None else (F(c[0] + off[0]), F(c[1] + off[1]))
        self.S.append(dict(x=F(x), y=F(y), octave=octave, orb=orb, ur=ur, slot=slot, desc=desc))
        return len(self.S) - 1

    def query(self, c, desc, level=0, obs=0, orb=1, ur=0.0, vc=0.5):
        self.blocks[-1]["queries"].append(dict(x=F(c[0]), y=F(c[1]), level=level, obs=obs, orb=orb, ur=ur, vc=vc, desc=desc))

    def simple(self, name, dists, offsets=None, octaves=None, level=0, **q):
        """one query; candidates at the given distances (the query's descriptor with that many bits flipped)"""
        c = self.site(name)
        d = self.rand_desc()
        for k, dist in enumerate(dists):
            kw = dist[1] if isinstance(dist, tuple) else {}
            dist = dist[0] if isinstance(dist, tuple) else dist
            bits = self.rng.permutation(256)[:dist]
            self.cand(c, (offsets or _OFFSETS)[k], _flip(d, bits), octave=(octaves[k] if octaves else level), **kw)
        self.query(c, d, level=level, **q)
        return c


def _half_cell(gb, center, axis):
    """a float32 coordinate within 3 px of the site whose cell coordinate is exactly k + 0.5 with k even: roundf gives k + 1, rounding
    to even k"""
    inv = F(gb.invW if axis == 0 else gb.invH)
    for k in range(0, 64, 2):
        x0 = F(3.75 * (k + 0.5))
        if abs(float(x0) - center) > 3:
            continue
        x = x0
        for _ in range(16):
            x = np.nextafter(x, F(0))
        for _ in range(32):
            if float(F(x * inv)) == k + 0.5:
                return x, k
            x = np.nextafter(x, F(1000))
    return None, None


def _chains(b, tag, repeat):
    """the sites whose answer depends on what earlier queries of the call did"""
    kind = b.kind
    first = len(b.blocks)
    if kind == "init":
        c = b.site(tag + "chain: matched at 30, met again at 30 (skipped)")
        cl = _Cluster(b, 1, 30); b.cand(c, (0, 0), cl.desc[0])
        b.query(c, cl.query({0: 30})); b.query(c, cl.query({0: 30}))
        c = b.site(tag + "chain: matched at 30, met again at 29 (stolen)")
        cl = _Cluster(b, 1, 30); b.cand(c, (0, 0), cl.desc[0])
        b.query(c, cl.query({0: 30})); b.query(c, _flip(cl.query({0: 30}), cl.P[0][-1:]))
        assert mm.hamming(b.blocks[-1]["queries"][-1]["desc"], cl.desc[0]) == 29
        c = b.site(tag + "chain: first candidate skipped, the second passes the ratio")
        cl = _Cluster(b, 2, 20); [b.cand(c, _OFFSETS[k], cl.desc[k]) for k in range(2)]
        b.query(c, cl.query({0: 20})); b.query(c, cl.query({0: 26, 1: 40}))
        c = b.site(tag + "chain: first candidate skipped, the second fails the ratio")
        cl = _Cluster(b, 3, 20); [b.cand(c, _OFFSETS[k], cl.desc[k]) for k in range(3)]
        b.query(c, cl.query({0: 20})); b.query(c, cl.query({0: 26, 1: 40, 2: 42}))
        c = b.site(tag + "chain of three steps and a steal")
        cl = _Cluster(b, 3, 16); [b.cand(c, _OFFSETS[k], cl.desc[k]) for k in range(3)]
        b.query(c, cl.query({0: 20})); b.query(c, cl.query({0: 22, 1: 30})); b.query(c, cl.query({0: 46, 1: 36, 2: 40}))
        b.query(c, cl.query({0: 10}))
    else:
        c = b.site(tag + "chain: slot overwritten by a later unobserved query")
        cl = _Cluster(b, 1, 30); b.cand(c, (0, 0), cl.desc[0])
        b.query(c, cl.query({0: 40})); b.query(c, cl.query({0: 60}))
        c = b.site(tag + "chain: slot closed by an observed query")
        cl = _Cluster(b, 2, 25); [b.cand(c, _OFFSETS[k], cl.desc[k]) for k in range(2)]
        b.query(c, cl.query({0: 40}), obs=1); b.query(c, cl.query({0: 31, 1: 61}))
    for blk in b.blocks[first:]:
        blk["repeat"] = repeat


@functools.lru_cache(maxsize=None)
def window_scene(kind, positions=False):
    """kind: "init" SearchForInitialization, "last" / "kf" SearchByProjection(cur, last / KF), "map" SearchByProjection(F, map points).
    positions: the chain sites once more with their queries at indices straddling a multiple of 64 and 1024, plain queries between.
    -> dict: the searched frame (s_*: kps, desc, is_orb, uright, slot), the queries (q_*: kps, desc, level, obs, is_orb, ur, view_cos,
    level_scale, valid; uv) and names (the site of every query)"""
    b = _Window(kind, 100 + KINDS.index(kind))
    th = b.th
    ratio_kind = kind in ("init", "map")
    gb = mm.frame(np.zeros(0, KP_DTYPE), [], W, H).gb
    for d in (th - 1, th, th + 1):
        b.simple("threshold: lone candidate at %d" % d, [d])
    if ratio_kind:
        pairs = []
        for r in (0.9, 0.6, 0.5):
            b0 = int(round(float(F(th) * F(r))))
            pairs += [(b0 - 1, th), (b0, th), (b0 + 1, th)]
        pairs += [(th * 4 // 5, th * 4 // 5), (th * 4 // 5 - 1, th * 4 // 5)]
        for r in RATIOS:                                                   # where the float32 product and the float64 one decide differently
            flips = [(b_, s_) for s_ in range(1, 256) for b_ in range(min(s_, th) + 1)
                     if mm._ratio_ok(b_, s_, r, None, kind == "map") != mm._ratio_ok(b_, s_, r, "ratio_double", kind == "map")]
            pairs += [p for p in flips[-1:] if p not in pairs]
        for p in pairs:
            b.simple("ratio: best %d, second %d" % p, list(p))
        if kind == "map":
            for p in pairs[2::3] + pairs[-2:-1]:
                b.simple("ratio: best %d, second %d on another level" % p, list(p), octaves=[1, 0], level=1)
        for D in sorted({mm.first_dist(th, r, kind == "map") for r in RATIOS}):
            for s in (D - 1, D, D + 1):
                if s <= 255:
                    b.simple("first_dist %d: best %d, second %d" % (D, th, s), [th, s])
            if D + 2 <= 255:
                b.simple("first_dist %d: best %d, second %d, third %d" % (D, th, D, D + 2), [th, D, D + 2])
    cell = 3.75
    b.simple("tie: three cells that differ in ix", [20, 20, 20], offsets=[(0, 0), (cell, 0), (-cell, 0)])
    b.simple("tie: three cells that differ in iy", [20, 20, 20], offsets=[(0, 0), (0, cell), (0, -cell)])
    b.simple("tie: one cell", [20, 20, 20], offsets=[(0, 0), (0.25, 0), (0, 0.25)])
    for name, axis, sign, at_r in (("|dx| == r", 0, 1, True), ("x the float below x + r", 0, 1, False), ("|dy| == r", 1, -1, True),
                                   ("y the float above y - r", 1, -1, False)):
        c = b.free[0]
        edge = F(c[axis] + sign * RADIUS)                                   # representable; its neighbour towards the site lies inside
        v = edge if at_r else np.nextafter(edge, F(c[axis]))
        assert (abs(F(v - F(c[axis]))) == RADIUS) == at_r and abs(F(v - F(c[axis]))) <= RADIUS
        b.simple("window: " + name, [10])
        b.S[-1]["xy"[axis]] = v
    for axis in (0, 1):                                                    # a tie whose order depends on the cell of the second candidate
        c = next((c for c in b.free if _half_cell(gb, c[axis], axis)[0] is not None), None)
        assert c is not None, "no free site with a half-cell coordinate"
        x, k = _half_cell(gb, c[axis], axis)
        other = F(3.75 * (k + 1))
        c = b.site("grid: cell coordinate %d.5 in %s" % (k, "xy"[axis]), at=c)
        d = b.rand_desc(); perm = [int(v) for v in b.rng.permutation(256)]
        pos = [(other, F(c[1])), (x, F(c[1]))] if axis == 0 else [(F(c[0]), other), (F(c[0]), x)]
        b.cand(c, None, _flip(d, perm[:20]), pos=pos[0]); b.cand(c, None, _flip(d, perm[20:40]), pos=pos[1])
        b.query(c, d)
    if kind == "init":
        b.simple("levels: the nearest candidate on octave 1", [5, 20], octaves=[1, 0])
        b.simple("levels: a query on level 1", [10], level=1, octaves=[0])
    else:
        b.simple("levels: octaves 0..4 around level 2", [10, 20, 30, 25, 5], octaves=[0, 1, 2, 3, 4], level=2)
        b.simple("levels: octaves 1, 2, 3 around level 2", [8, 30, 12], octaves=[1, 2, 3], level=2)
        b.simple("levels: octaves 2, 3 around level 2", [30, 12], octaves=[2, 3], level=2)
    b.simple("type gate: the nearest candidate is of the other type", [(5, dict(orb=0)), 20])
    if kind in ("last", "map"):
        up = float(np.nextafter(F(108.0), F(1000)))
        b.simple("stereo gate: er == radius", [(10, dict(ur=108.0)), 30], ur=100.0)
        b.simple("stereo gate: er the float above radius", [(10, dict(ur=up)), 30], ur=100.0)
    if kind == "map":
        b.simple("viewing cosine (float)0.998, candidate 3 px away", [10], offsets=[(3.0, 0.0)], vc=VIEW_COS_EDGE)
        b.simple("viewing cosine the float below (float)0.998", [10], offsets=[(3.0, 0.0)], vc=float(np.nextafter(F(0.998), F(0))))
    if kind != "init":
        b.simple("occupancy: slot -2", [(10, dict(slot=-2)), 30])
        b.simple("occupancy: slot -3", [(10, dict(slot=-3))])
    _chains(b, "", None)
    for k in range({"init": 0, "last": 10, "kf": 14, "map": 0}[kind]):            # (the histograms of HISTOGRAMS need 30 to 32 pushes)
        b.simple("plain %d" % k, [10 + k])
    if positions:
        _chains(b, "at 64: ", 64)
        _chains(b, "at 1024: ", 1024)
    # ---- the order of the queries
    empty = SITES[-1]
    Q, names = [], []

    def put(blk):
        for q in blk["queries"]:
            Q.append(q); names.append(blk["name"])

    def pad(until):
        while not until(len(Q)):
            Q.append(dict(x=F(empty[0]), y=F(empty[1]), level=0, obs=0, orb=1, ur=0.0, vc=0.5, desc=b.rand_desc())); names.append("plain query at an empty site")
    if not positions:
        for blk in b.blocks:
            put(blk)
    else:
        rest = [blk for blk in b.blocks if blk["repeat"] is None]
        while rest and len(Q) + len(rest[0]["queries"]) <= 63:
            put(rest.pop(0))
        pad(lambda n: n == 63)
        for blk in [blk for blk in b.blocks if blk["repeat"] == 64]:
            pad(lambda n: n % 64 == 63); put(blk)
        for blk in rest:
            put(blk)
        pad(lambda n: n == 1023)
        for blk in [blk for blk in b.blocks if blk["repeat"] == 1024]:
            pad(lambda n: n % 64 == 63); put(blk)
    s_kps = np.zeros(len(b.S), KP_DTYPE)
    for f in ("x", "y", "octave"):
        s_kps[f] = [s[f] for s in b.S]
    s_kps["class_id"] = s_kps["octave"]; s_kps["size"] = 31.0
    q_kps = np.zeros(len(Q), KP_DTYPE)
    q_kps["x"] = [q["x"] for q in Q]; q_kps["y"] = [q["y"] for q in Q]; q_kps["octave"] = [q["level"] for q in Q]
    q_kps["class_id"] = q_kps["octave"]; q_kps["size"] = 31.0
    sc = dict(kind=kind, th=th, n_sites=b.used, names=np.array(names),
              s_kps=s_kps, s_desc=_to_u8([s["desc"] for s in b.S]), s_is_orb=np.array([s["orb"] for s in b.S], np.uint8),
              s_uright=np.array([s["ur"] for s in b.S], np.float32), slot=np.array([s["slot"] for s in b.S], np.int32),
              q_kps=q_kps, q_desc=_to_u8([q["desc"] for q in Q]), q_level=np.array([q["level"] for q in Q], np.int32),
              q_obs=np.array([q["obs"] for q in Q], np.uint8), q_is_orb=np.array([q["orb"] for q in Q], np.uint8),
              q_ur=np.array([q["ur"] for q in Q], np.float32), q_vc=np.array([q["vc"] for q in Q], np.float32),
              q_ls=np.ones(len(Q), np.float32), q_valid=np.ones(len(Q), np.uint8),
              uv=np.stack([q_kps["x"], q_kps["y"]], axis=1).astype(np.float32))
    for a in sc.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc


# ---------------------------------------------------------------------------------------------------
# calls: one description of a matcher call, applied to the model, the oracle and the kernels alike
def window_configs(kind):
    """the settings every window scene is run with: dicts of ratio / mode / th (map), form "plain" / "mixed" / "stereo" """
    out = []
    if kind == "init":
        out = [dict(ratio=r, form=f) for r in RATIOS for f in ("plain",)] + [dict(ratio=0.9, form="mixed")]
    elif kind == "last":
        out = [dict(mode=m, form="plain") for m in (0, 1, 2)] + [dict(mode=0, form="mixed"), dict(mode=0, form="stereo")]
    elif kind == "kf":
        out = [dict(form="plain"), dict(form="mixed")]
    else:
        out = [dict(ratio=r, th=2.0, form="plain") for r in RATIOS] + [dict(ratio=0.9, th=1.0, form="plain"), dict(ratio=0.9, th=2.0, form="mixed"),
                                                                       dict(ratio=0.9, th=2.0, form="stereo")]
    return out


def config_id(cfg):
    return " ".join("%s=%s" % kv for kv in sorted(cfg.items()))


MAIN = {"init": dict(ratio=0.9, form="mixed"), "last": dict(mode=0, form="mixed"), "kf": dict(form="mixed"), "map": dict(ratio=0.9, th=2.0, form="mixed")}


def run_model(sc, cfg, check_ori=True, wrong=None, info=None):
    """the model on a window scene -> (nmatches, match / slot array[, vbPrevMatched])"""
    kind = sc["kind"]
    mixed = cfg["form"] == "mixed"
    S = mm.frame(sc["s_kps"], sc["s_desc"], W, H, sc["s_is_orb"] if mixed else None)
    qo = sc["q_is_orb"] if mixed else None
    ur = (sc["s_uright"], sc["q_ur"]) if cfg["form"] == "stereo" else (None, None)
    if kind == "init":
        return mm.search_for_initialization(mm.frame(sc["q_kps"], sc["q_desc"], W, H, qo), S, sc["uv"], RADIUS, cfg["ratio"], check_ori, wrong, info)
    if kind == "last":
        return mm.search_by_projection_last(S, mm.frame(sc["q_kps"], sc["q_desc"], W, H, qo), sc["q_valid"], sc["uv"], sc["q_desc"], sc["q_obs"],
                                            sc["slot"], float(RADIUS), sc["q_ls"], cfg["mode"], check_ori, ur[0], ur[1], wrong, info)
    if kind == "kf":
        return mm.search_by_projection_kf(S, sc["q_kps"], qo, sc["q_valid"], sc["uv"], sc["q_level"], sc["q_ls"], sc["q_desc"], sc["slot"],
                                          float(RADIUS), TH["kf"], check_ori, wrong, info)
    return mm.search_by_projection_map(S, sc["q_valid"], sc["uv"], sc["q_level"], sc["q_vc"], sc["q_desc"], sc["q_obs"], sc["slot"], cfg["th"],
                                       cfg["ratio"], sc["q_ls"], qo, ur[0], ur[1], wrong, info)


def run_oracle(oracle, sc, cfg, check_ori=True, fast=False):
    kind = sc["kind"]
    mixed = cfg["form"] == "mixed"
    S = oracle.Frame(sc["s_kps"], sc["s_desc"], W, H, sc["s_is_orb"] if mixed else None, fast=fast)
    qo = sc["q_is_orb"] if mixed else None
    ur = dict(uright=sc["s_uright"], proj_ur=sc["q_ur"]) if cfg["form"] == "stereo" else {}
    if kind == "init":
        return oracle.search_for_initialization(oracle.Frame(sc["q_kps"], sc["q_desc"], W, H, qo, fast=fast), S, sc["uv"], RADIUS, cfg["ratio"], check_ori)
    if kind == "last":
        return oracle.search_by_projection_last(S, oracle.Frame(sc["q_kps"], sc["q_desc"], W, H, qo, fast=fast), sc["q_valid"], sc["uv"], sc["q_desc"],
                                                sc["q_obs"], sc["slot"], float(RADIUS), sc["q_ls"], cfg["mode"], check_ori, **ur)
    if kind == "kf":
        return oracle.search_by_projection_kf(S, sc["q_kps"], qo, sc["q_valid"], sc["uv"], sc["q_level"], sc["q_ls"], sc["q_desc"], sc["slot"],
                                              float(RADIUS), TH["kf"], check_ori)
    if ur:
        ur = dict(uright=ur["uright"], proj_xr=ur["proj_ur"])
    return oracle.search_by_projection_map(S, sc["q_valid"], sc["uv"], sc["q_level"], sc["q_vc"], sc["q_desc"], sc["q_obs"], sc["slot"], cfg["th"],
                                           cfg["ratio"], sc["q_ls"], mp_is_orb=qo, **ur)


def run_kernels(fe, ctx, sc, cfg, check_ori=True):
    kind = sc["kind"]
    mixed = cfg["form"] == "mixed"
    S = fe.FrameView(sc["s_kps"], sc["s_desc"], W, H, sc["s_is_orb"] if mixed else None)
    qo = sc["q_is_orb"] if mixed else None
    m = fe.ORBmatcher(cfg.get("ratio", 0.9), check_ori, ctx)
    ur = dict(uright=sc["s_uright"], proj_ur=sc["q_ur"]) if cfg["form"] == "stereo" else {}
    if kind == "init":
        return m.SearchForInitialization(fe.FrameView(sc["q_kps"], sc["q_desc"], W, H, qo), S, sc["uv"], RADIUS)
    if kind == "last":
        return m.SearchByProjectionLast(S, fe.FrameView(sc["q_kps"], sc["q_desc"], W, H, qo), sc["q_valid"], sc["uv"], sc["q_desc"], sc["q_obs"],
                                        sc["slot"], float(RADIUS), sc["q_ls"], cfg["mode"], **ur)
    if kind == "kf":
        return m.SearchByProjectionKF(S, sc["q_kps"], qo, sc["q_valid"], sc["uv"], sc["q_level"], sc["q_ls"], sc["q_desc"], sc["slot"], float(RADIUS),
                                      TH["kf"])
    if ur:
        ur = dict(uright=ur["uright"], proj_xr=ur["proj_ur"])
    return m.SearchByProjectionMap(S, sc["q_valid"], sc["uv"], sc["q_level"], sc["q_vc"], sc["q_desc"], sc["q_obs"], sc["slot"], cfg["th"], sc["q_ls"],
                                   mp_is_orb=qo, **ur)


def same(a, b):
    """two results of a matcher equal as integers (vbPrevMatched bit for bit)"""
    bits = lambda v: np.asarray(v).view(np.uint32) if np.asarray(v).dtype == np.float32 else np.asarray(v)
    return len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------
# the rotation histogram: variants of a scene that differ in the keypoints' angles only
HISTOGRAMS = ("one bin", "four equal", "max2 = 2", "max2 = 1", "max3 = 2", "max3 = 1", "rounding", "stolen", "pushed twice")


def tie_rots():
    """angle differences whose float32 product with 1.0f / 30 is exactly k + 0.5 with k even (roundf and rounding to even part)"""
    out = []
    for q in range(0, 360 * 4):
        v = float(F(F(q / 4.0) * (F(1.0) / F(30))))
        if v == math.floor(v) + 0.5 and math.floor(v) % 2 == 0:
            out.append(q / 4.0)
    return out


def histogram_applies(name, kind):
    """the map matcher has no histogram; only SearchForInitialization steals; only SearchByProjection(cur, last) writes a slot twice"""
    return kind != "map" and (name != "stolen" or kind == "init") and (name != "pushed twice" or kind == "last")


def with_angles(q_kps, s_kps, pushes, name, stolen=(), twice=None, side="q"):
    """copies of the two keypoint arrays with the angles of histogram `name`.  pushes: the (query, candidate) pairs that enter the
    histogram, in order; stolen: queries among them whose match is stolen later; twice: the first query of a slot pushed twice.
    side "q": the difference is the query's angle (the candidates stay at 0, but for a few negative differences); side "c": it is
    made on the candidate (angle 360 - difference, so every difference takes the `+ 360`) and the queries stay at 0 -- for calls
    that share the queries among several candidate sets; side "q30": made on the query against candidates that all stay at 30
    (differences from 330 on take the `+ 360`) -- for calls that share the candidates among several query sets."""
    q_kps, s_kps = q_kps.copy(), s_kps.copy()
    q_kps["angle"] = 0; s_kps["angle"] = 0
    if side == "q30":
        q_kps["angle"] = 30; s_kps["angle"] = 30
    n = len(pushes)
    if side == "c":                                                         # pushes that share a candidate share its bin: they go first
        pushes = sorted(pushes, key=lambda p: -sum(1 for _, c in pushes if c == p[1]))
    ties = tie_rots()
    assert 15.0 in ties and mm.rot_bin(15.0, 0.0) == 1 and mm.rot_bin(15.0, 0.0, "rot_half_even") == 0

    def put(push, rot):
        if side == "q":
            q_kps["angle"][push[0]] = rot
        elif side == "q30":
            q_kps["angle"][push[0]] = rot + 30.0 if rot + 30.0 < 360 else rot + 30.0 - 360.0
        else:
            s_kps["angle"][push[1]] = 360.0 - rot if rot > 0 else 0.0
            assert rot == 0 or float(F(F(0.0) - s_kps["angle"][push[1]]) + F(360.0)) == float(F(rot))
            assert all(mm.rot_bin(0.0, s_kps["angle"][c]) == mm.rot_bin(0.0, s_kps["angle"][push[1]]) for _, c in pushes if c == push[1])
    mid = lambda b: 30.0 * b                                                 # a difference in the middle of bin b

    def fill(counts, rest_bins, cap):
        """counts: [(bin, count)]; the other pushes go to rest_bins, at most cap each"""
        at = 0
        for b_, k in counts:
            assert at + k <= n, "%s needs %d pushes, the scene has %d" % (name, at + k, n)
            for p in pushes[at:at + k]:
                put(p, mid(b_))
            at += k
        assert n - at <= cap * len(rest_bins), "%s: %d pushes left for %d bins of %d" % (name, n - at, len(rest_bins), cap)
        for j, p in enumerate(pushes[at:]):
            put(p, mid(rest_bins[j % len(rest_bins)]))
    others = [0, 1, 2, 4, 6, 8, 9, 10, 11, 12]
    if name == "one bin":
        pass
    elif name == "four equal":
        k = n // 4
        fill([(2, k), (4, k), (6, k), (8, k)], [10, 11, 12], 1)
    elif name == "max2 = 2":
        fill([(3, 20), (5, 2)], others + [7], 2)
    elif name == "max2 = 1":
        fill([(3, 20)], others + [5, 7], 1)
    elif name == "max3 = 2":
        assert n - 22 >= 2
        fill([(3, 20), (7, 2), (5, n - 22)], [], 0)
    elif name == "max3 = 1":
        assert n - 21 >= 1
        fill([(3, 20), (7, 1), (5, n - 21)], [], 0)
    elif name == "rounding":
        once = [p for p in pushes if sum(1 for _, c in pushes if c == p[1]) == 1]
        if side == "q":
            special = [(15.0, 0.0)] * 3 + [(0.0, 30.0)] * 3 + [(345.0, 0.0), (10.0, 25.0), (359.99, 0.0), (-0.0, 0.0), (45.0, 0.0), (75.0, 0.0), (359.0, 359.5)]
        else:
            special = [15.0] * 3 + [330.0] * 3 + [345.0, 345.0, 359.99, 45.0, 75.0, 359.5]
        assert len(once) >= len(special) and n >= len(special) + 9
        used = set()
        for (q, c), a in zip(once, special):
            if side == "q":
                q_kps["angle"][q], s_kps["angle"][c] = a
            else:
                put((q, c), a)
            used.add(q)
        for j, p in enumerate([p for p in pushes if p[0] not in used]):
            put(p, mid((1, 5, 6)[j % 3]))
    elif name == "stolen":
        assert stolen, "no stolen query among the pushes"
        st = stolen[0]
        rest = [p for p in pushes if p[0] != st]
        assert len(rest) >= 9
        q_kps["angle"][st] = mid(6)
        for j, p in enumerate(rest):
            put(p, mid(6) if j < 2 else mid(8) if j < 5 else mid((2, 4)[j % 2]))
    elif name == "pushed twice":
        assert twice is not None
        q_kps["angle"][twice] = mid(9)
    return q_kps, s_kps


@functools.lru_cache(maxsize=None)
def histogram_scene(kind, name):
    """window_scene(kind) with the angles of histogram `name`, planned on the pushes of the MAIN configuration"""
    sc = dict(window_scene(kind))
    info = {}
    _, m = run_model(sc, MAIN[kind], True, None, info)[:2]
    pushes = info.get("pushes", [])
    stolen = [q for q, _ in pushes if m[q] < 0] if kind == "init" else []
    slots = [c for _, c in pushes]
    twice = next((q for q, c in pushes if slots.count(c) == 2), None)
    sc["q_kps"], sc["s_kps"] = with_angles(sc["q_kps"], sc["s_kps"], pushes, name, stolen, twice)
    sc["q_kps"].setflags(write=False); sc["s_kps"].setflags(write=False)
    sc["n_pushes"] = len(pushes)
    return sc


# ---------------------------------------------------------------------------------------------------
def probe(sc, ratio=None):
    """How often a scene lands on the comparisons, by brute force and ignoring the state filter: the number of queries, and of those
    with best == TH, best == TH + 1, exact float32 equality in the ratio test, a ratio decision that flips when best or second moves
    by one."""
    kind, th = sc["kind"], sc["th"]
    S = mm.frame(sc["s_kps"], sc["s_desc"], W, H)
    qd = mm.as_ints(sc["q_desc"])
    out = dict(queries=0, best_eq_th=0, best_eq_th1=0, ratio_equal=0, ratio_near=0)
    for i in range(len(qd)):
        L = int(sc["q_level"][i])
        if kind == "init" and L > 0:
            continue
        lo, hi = {"init": (L, L), "last": (L - 1, L + 1), "kf": (L - 1, L + 1), "map": (L - 1, L)}[kind]
        ds = sorted(mm.hamming(qd[i], S.desc[j]) for j in mm.candidates(S, sc["uv"][i][0], sc["uv"][i][1], float(RADIUS), lo, hi))
        if not ds:
            continue
        out["queries"] += 1
        best = ds[0]
        out["best_eq_th"] += best == th
        out["best_eq_th1"] += best == th + 1
        if ratio is not None and len(ds) > 1:
            second = ds[1]
            ok = lambda b_, s_: mm._ratio_ok(b_, s_, ratio, None, kind == "map")
            out["ratio_equal"] += bool(F(best) == F(second) * F(ratio))
            out["ratio_near"] += any(ok(best, second) != ok(best + db, second + ds_) for db, ds_ in ((1, 0), (-1, 0), (0, 1), (0, -1)))
    return out


# ---------------------------------------------------------------------------------------------------
# the node-walk matchers: one vocabulary node per site
NODE_KINDS = ("bow", "bowkf", "tri")
NODE_RATIOS = (0.9, 0.6, 0.5, 1.0, 1.5)
EPIPOLE = (0.0, 0.0)
F12_HORIZONTAL = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)      # epipolar lines y2 = y1: dsqr = (y2 - y1)^2 < 3.84 sigma2
TRI_SCALE = np.array([1.0, 1.2], np.float32)
TRI_SIGMA2 = np.array([1.0, 1.44], np.float32)


class _Nodes:
    def __init__(self, kind, seed):
        self.kind = kind
        self.rng = np.random.default_rng(seed)
        self.A, self.B, self.names = [], [], []                             # side 1 (the queries), side 2 (the candidates)
        self.nodes = []                                                     # (node id, [indices on side 1], [indices on side 2])

    rand_desc = _Window.rand_desc

    def site(self, name, common=True):
        self.names.append(name)
        self.nodes.append((10 * len(self.nodes) + 7, [], [], common))

    def a(self, desc, flag=1, y=50.0):
        self.A.append(dict(desc=desc, flag=flag, x=float(20 + len(self.nodes)), y=y))
        self.nodes[-1][1].append(len(self.A) - 1)
        return len(self.A) - 1

    def b(self, desc, flag=1, x=None, y=50.0):
        self.B.append(dict(desc=desc, flag=flag, x=float(100 + len(self.nodes)) if x is None else x, y=y))
        self.nodes[-1][2].append(len(self.B) - 1)

    def simple(self, name, dists, flag=1, **kw):
        """one query; candidates at the given distances, in the node's order"""
        self.site(name)
        d = self.rand_desc()
        for dist in dists:
            opt = dict(dist[1]) if isinstance(dist, tuple) else {}
            dist = dist[0] if isinstance(dist, tuple) else dist
            self.b(_flip(d, self.rng.permutation(256)[:dist]), **opt)
        return self.a(d, flag, **kw)


def _csr(nodes, side, skip_odd):
    """a feature vector as (node ids ascending, offsets, indices); the uncommon nodes are those of one side only"""
    ids, off, idx = [], [0], []
    for k, (nid, a, b_, common) in enumerate(nodes):
        feats = (a, b_)[side]
        if not feats or (not common and k % 2 == skip_odd):
            continue
        ids.append(nid); idx += feats; off.append(len(idx))
    return np.array(ids, np.uint32), np.array(off, np.int32), np.array(idx, np.int32)


@functools.lru_cache(maxsize=None)
def node_scene(kind):
    """kind: "bow" SearchByBoW(KF, F), "bowkf" SearchByBoW(KF, KF), "tri" SearchForTriangulation.  Side 1 holds the queries (the
    keyframe of "bow", KF1 of the others), side 2 what is searched.  -> dict(kps1, desc1, flag1, fv1, kps2, desc2, flag2, fv2, names);
    the flags are kf_has_mp / has_mp / elig (bit 0: no map point yet, bit 1: a stereo observation)."""
    b = _Nodes(kind, 200 + NODE_KINDS.index(kind))
    th = mm.TH_LOW
    for d in (th - 1, th, th + 1):
        b.simple("threshold: lone candidate at %d" % d, [d])
    if kind != "tri":
        pairs = []
        for r in (0.9, 0.6, 0.5):
            b0 = int(round(float(F(th) * F(r))))
            pairs += [(b0 - 1, th), (b0, th), (b0 + 1, th)]
        pairs += [(40, 40), (39, 40)]
        for r in NODE_RATIOS:
            flips = [(b_, s_) for s_ in range(1, 256) for b_ in range(min(s_, th) + 1) if mm._ratio_ok(b_, s_, r, None) != mm._ratio_ok(b_, s_, r, "ratio_double")]
            pairs += [p for p in flips[-1:] if p not in pairs]
        for p in pairs:
            b.simple("ratio: best %d, second %d" % p, list(p))
        best = th if kind == "bow" else th - 1                              # (KF, KF) accepts bestDist1 < TH_LOW only
        for D in sorted({mm.first_dist(best, r) for r in NODE_RATIOS}):
            for s in (D - 1, D, D + 1):
                b.simple("first_dist %d: best %d, second %d" % (D, best, s), [best, s])
            b.simple("first_dist %d: best %d, second %d, third %d" % (D, best, D, D + 2), [best, D, D + 2])
        b.simple("tie: three equal distances", [20, 20, 20])
        b.simple("tie: the second best equals the best at the threshold", [best, best])
        b.simple("flags: a query without a map point", [10], flag=0)
        if kind == "bowkf":
            b.simple("flags: the nearest candidate has no map point", [(5, dict(flag=0)), 20])
        b.site("chain: the best candidate was matched by an earlier query")
        cl = _Cluster(b, 2, 15); [b.b(d) for d in cl.desc]
        b.a(cl.query({0: 20})); b.a(cl.query({0: 16, 1: 30}))
        b.site("chain: the best candidate was matched, the second fails the ratio")
        cl = _Cluster(b, 3, 15); [b.b(d) for d in cl.desc]
        b.a(cl.query({0: 20})); b.a(cl.query({0: 16, 1: 30, 2: 32}))
        b.site("chain of three")
        cl = _Cluster(b, 3, 15); [b.b(d) for d in cl.desc]
        b.a(cl.query({0: 20})); b.a(cl.query({0: 16, 1: 24})); b.a(cl.query({0: 18, 1: 22, 2: 30}))
    else:
        b.simple("tie: three equal distances, the last fails the epipolar test", [20, 20, (20, dict(y=53.0))])
        b.simple("tie: two equal distances at the threshold", [th, th])
        b.simple("order: a nearer candidate after a farther one", [30, 20])
        b.simple("order: a farther candidate after a nearer one", [20, 30])
        b.simple("epipolar: dsqr on both sides of 3.84 sigma2", [(10, dict(y=51.96)), (20, dict(y=51.95))])
        b.simple("flags: a query that has a map point", [10], flag=0)
        b.simple("flags: the nearest candidate has a map point", [(5, dict(flag=0)), 20])
        x_in = float(np.nextafter(F(10.0), F(0)))
        b.simple("epipole: squared distance 100 * scale exactly", [(10, dict(x=10.0, y=0.0))], y=0.0)
        b.simple("epipole: the float below", [(10, dict(x=x_in, y=0.0)), (30, dict(x=30.0, y=0.0))], y=0.0)
        b.simple("epipole: inside, but the candidate is a stereo observation", [(10, dict(x=5.0, y=0.0, flag=3))], y=0.0)
        b.simple("epipole: inside, but the query is a stereo observation", [(10, dict(x=5.0, y=0.0))], flag=3, y=0.0)
        b.site("two queries take the same candidate")
        cl = _Cluster(b, 1, 20); b.b(cl.desc[0]); b.a(cl.query({0: 20})); b.a(cl.query({0: 24}))
    for k in range({"bow": 6, "bowkf": 5, "tri": 17}[kind]):                 # (the histograms of HISTOGRAMS need 30 to 32 pushes)
        b.simple("plain %d" % k, [10 + k])
    for k in range(4):                                                      # nodes that one side only holds: the lower_bound steps
        b.site("a node of one side only", common=False)
        b.a(b.rand_desc()); b.b(b.rand_desc())

    def kps(side):
        k = np.zeros(len(side), KP_DTYPE)
        k["x"] = [s["x"] for s in side]; k["y"] = [s["y"] for s in side]; k["size"] = 31.0; k["class_id"] = -1
        return k
    sc = dict(kind=kind, th=th, n_sites=len(b.nodes), names=np.array(b.names),
              kps1=kps(b.A), desc1=_to_u8([s["desc"] for s in b.A]), flag1=np.array([s["flag"] for s in b.A], np.uint8), fv1=_csr(b.nodes, 0, 0),
              kps2=kps(b.B), desc2=_to_u8([s["desc"] for s in b.B]), flag2=np.array([s["flag"] for s in b.B], np.uint8), fv2=_csr(b.nodes, 1, 1))
    for a in list(sc.values()) + list(sc["fv1"]) + list(sc["fv2"]):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc


def node_configs(kind):
    return [dict(coarse=c) for c in (False, True)] if kind == "tri" else [dict(ratio=r) for r in NODE_RATIOS]


NODE_MAIN = {"bow": dict(ratio=0.9), "bowkf": dict(ratio=0.9), "tri": dict(coarse=False)}


def run_node_model(sc, cfg, check_ori=True, wrong=None, info=None):
    a = (sc["kps1"], sc["desc1"], sc["flag1"], sc["fv1"], sc["kps2"], sc["desc2"])
    if sc["kind"] == "bow":
        return mm.search_by_bow(*a, sc["fv2"], cfg["ratio"], check_ori, wrong, info)
    if sc["kind"] == "bowkf":
        return mm.search_by_bow_kf(*a, sc["flag2"], sc["fv2"], cfg["ratio"], check_ori, wrong, info)
    return mm.search_for_triangulation(*a, sc["flag2"], sc["fv2"], EPIPOLE, F12_HORIZONTAL, TRI_SCALE, TRI_SIGMA2, cfg["coarse"], check_ori, wrong, info)


def run_node_oracle(oracle, sc, cfg, check_ori=True):
    a = (sc["kps1"], sc["desc1"], sc["flag1"], sc["fv1"], sc["kps2"], sc["desc2"])
    if sc["kind"] == "bow":
        return oracle.search_by_bow(*a, sc["fv2"], cfg["ratio"], check_ori)
    if sc["kind"] == "bowkf":
        return oracle.search_by_bow_kf(*a, sc["flag2"], sc["fv2"], cfg["ratio"], check_ori)
    return oracle.search_for_triangulation(*a, sc["flag2"], sc["fv2"], EPIPOLE, F12_HORIZONTAL, TRI_SCALE, TRI_SIGMA2, cfg["coarse"], check_ori)


def _pairs(m):
    k = np.flatnonzero(np.asarray(m) >= 0)
    return np.stack([k, np.asarray(m)[k]], axis=1).astype(np.int32)


def run_node_kernels(fe, ctx, scenes, cfg, check_ori=True, batched=True):
    """scenes: K scenes of one kind that share the side the batched form shares (side 2 of "bow", side 1 of the others).  batched:
    the *_KeyFrames entry point; else the single-pair one (K = 1).  -> [(nmatches, match array)] per scene"""
    sc = scenes[0]
    kind = sc["kind"]
    if not batched:
        assert len(scenes) == 1
        a = (sc["kps1"], sc["desc1"], sc["flag1"], sc["fv1"], sc["kps2"], sc["desc2"])
        if kind == "bow":
            return [fe.SearchByBoW(*a, sc["fv2"], cfg["ratio"], check_ori, ctx=ctx)]
        if kind == "bowkf":
            return [fe.SearchByBoW_KF(*a, sc["flag2"], sc["fv2"], cfg["ratio"], check_ori, ctx=ctx)]
        n, pairs = fe.SearchForTriangulation(*a, sc["flag2"], sc["fv2"], EPIPOLE, F12_HORIZONTAL, TRI_SCALE, TRI_SIGMA2, cfg["coarse"], check_ori, ctx=ctx)
        m = np.full(len(sc["kps1"]), -1, np.int32); m[pairs[:, 0]] = pairs[:, 1]
        return [(n, m)]
    K = len(scenes)
    if kind == "bow":
        nm, m = fe.SearchByBoWKeyFrames([(s["kps1"], s["desc1"], s["flag1"], s["fv1"]) for s in scenes], sc["kps2"], sc["desc2"], sc["fv2"], cfg["ratio"],
                                        check_ori, ctx=ctx)
    else:
        kfs = [(s["kps2"], s["desc2"], s["flag2"], s["fv2"]) for s in scenes]
        if kind == "bowkf":
            nm, m = fe.SearchByBoW_KF_KeyFrames(sc["kps1"], sc["desc1"], sc["flag1"], sc["fv1"], kfs, cfg["ratio"], check_ori, ctx=ctx)
        else:
            nm, m = fe.SearchForTriangulationKeyFrames(sc["kps1"], sc["desc1"], sc["flag1"], sc["fv1"], kfs, np.tile(np.array(EPIPOLE, np.float32), K),
                                                       np.tile(F12_HORIZONTAL.reshape(-1), K), TRI_SCALE, TRI_SIGMA2, cfg["coarse"], check_ori, ctx=ctx)
    return [(int(nm[k]), m[k]) for k in range(K)]


def node_histogram_applies(name, kind):
    """nothing is stolen and no slot is written twice in a node walk"""
    return name not in ("stolen", "pushed twice")


@functools.lru_cache(maxsize=None)
def node_histogram_scene(kind, name):
    """node_scene(kind) with the angles of histogram `name`, planned on the pushes of the NODE_MAIN configuration and made on the side
    that the batched calls do not share (side 1 of "bow", side 2 of the others): the shared side is the same array in every variant"""
    sc = dict(node_scene(kind))
    info = {}
    run_node_model(sc, NODE_MAIN[kind], True, None, info)
    pushes = info["pushes"]
    if kind == "bow":                                                       # the difference is (keyframe angle) - (frame angle): the keyframe is side 1
        sc["kps1"], sc["kps2"] = with_angles(sc["kps1"], sc["kps2"], pushes, name, side="q30")
    else:
        sc["kps1"], sc["kps2"] = with_angles(sc["kps1"], sc["kps2"], pushes, name, side="c")
    sc["kps1"].setflags(write=False); sc["kps2"].setflags(write=False)
    sc["n_pushes"] = len(pushes)
    return sc


def node_probe(sc, ratio=None):
    """probe() for a node-walk scene: best / second over a node's candidates, ignoring the state and the flags"""
    d1, d2 = mm.as_ints(sc["desc1"]), mm.as_ints(sc["desc2"])
    out = dict(queries=0, best_eq_th=0, best_eq_th1=0, ratio_equal=0, ratio_near=0)
    for l1, l2 in mm._common_nodes(sc["fv1"], sc["fv2"]):
        for i1 in l1:
            ds = sorted(mm.hamming(d1[i1], d2[i2]) for i2 in l2)
            out["queries"] += 1
            out["best_eq_th"] += ds[0] == sc["th"]
            out["best_eq_th1"] += ds[0] == sc["th"] + 1
            if ratio is not None and len(ds) > 1:
                ok = lambda b_, s_: mm._ratio_ok(b_, s_, ratio, None)
                out["ratio_equal"] += bool(F(ds[0]) == F(ds[1]) * F(ratio))
                out["ratio_near"] += any(ok(ds[0], ds[1]) != ok(ds[0] + db, ds[1] + ds_) for db, ds_ in ((1, 0), (-1, 0), (0, 1), (0, -1)))
    return out
