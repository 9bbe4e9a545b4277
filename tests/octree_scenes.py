"""Planted inputs for the keypoint selection (tests/octree_model.py): level-0 images of lone bright pixels on a black ground, which
put a FAST candidate exactly where a scene wants it, plus a few texture / noise frames for what planting cannot reach.

A lone pixel of value v is a FAST-9/16 corner of response v - 1 (all 16 ring pixels are darker by v), detected at threshold t iff
v > t.  Two planted pixels leave each other alone when they are no 8-neighbours (non-maximum suppression) and the black pixels
around them never see 9 contiguous bright ring pixels; the lattices used here (2 px x 4 px and coarser) keep that.  Every scene
states the candidates it expects (`expect`), and the tests assert them against the oracle and against the device's `cand` stage
before anything else: a scene that does not produce its candidates is a broken scene, not a finding.

Each scene carries the quotas N it is run with.  They are read off the model's own pass log (pass k: list size L, divisible nodes X)
so that the comparison under test is decided by one unit: N = L, L + 1, L - 1 (`size >= N`), N = L + 3X, L + 3X - 1, L + 3X + 1
(`size + 3 * nToExpand > N`).  `claims` are predicates on the model's probe: the scene did reach what it was planted for."""
import functools

import numpy as np

from eorb_slam_amd import synth
import octree_model as m

INI, MINTH = 20, 7          # thresholds of the planted scenes
BIG = 10 ** 9


class Scene:
    def __init__(self, name, W, H, edge, img, Ns, expect=None, claims=(), ini=INI, minth=MINTH, sf=1.0, nlevels=1):
        self.name, self.W, self.H, self.edge, self.img = name, W, H, edge, img
        self.Ns = list(Ns)                    # nfeatures values (single level: the level's quota)
        self.expect = expect                  # [(x, y, response)] relative to the border window, any order; None: not planted
        self.claims = list(claims)            # [(N or None for every N, text, predicate(probe))]
        self.ini, self.minth, self.sf, self.nlevels = ini, minth, sf, nlevels

    def params(self, N):
        return dict(nfeatures=N, scaleFactor=self.sf, nlevels=self.nlevels, iniThFAST=self.ini, minThFAST=self.minth, edgeTh=self.edge)

    def window(self):
        b = m.borders(self.W, self.H, self.edge)
        return b[0], b[2] - b[0], b[3] - b[1]      # minBorder, w, h

    def __repr__(self):
        return self.name


def value(x, y):
    """pixel value of a planted point: 30 .. 240, so responses differ between most neighbours and all exceed INI"""
    return 30 + (x * 37 + y * 101) % 211


def plant(W, H, edge, pts):
    """pts = [(x, y, v)] relative to the border window -> (image, expected candidates)"""
    img = np.zeros((H, W), np.uint8)
    mb = edge - 3
    for x, y, v in pts:
        assert img[y + mb, x + mb] == 0
        img[y + mb, x + mb] = v
    return img, [(x, y, v - 1) for x, y, v in pts]


def lattice(x0, x1, y0, y1, dx=2, dy=4):
    return [(x, y) for y in range(y0, y1 + 1, dy) for x in range(x0, x1 + 1, dx)]


def valued(pts):
    return [(x, y, value(x, y)) for x, y in pts]


def subset(pts, n, seed):
    idx = np.random.default_rng(seed).permutation(len(pts))[:n]
    return [pts[i] for i in sorted(idx)]


def ordered(W, H, edge, expect):
    """the expected candidates in the reference's order (cell row, cell column, raster): what distribute() is fed"""
    _, _, wCell, hCell = m.cell_grid(W, H, edge)
    # a key at window-relative x lies in cell column (x - 3) // wCell (its detection domain starts 3 px inside the window)
    return sorted(expect, key=lambda c: ((c[1] - 3) // hCell, (c[0] - 3) // wCell, c[1], c[0]))


def pass_log(cands, w, h, trace=None):
    return m.distribute(cands, w, h, BIG, trace=trace)[1]["passes"]


def n_from_log(cands, w, h, k, formula):
    p = pass_log(cands, w, h)[k]
    L, X = p["size"], p["expand"]
    return {"L": L, "L+1": L + 1, "L-1": L - 1, "L+3X": L + 3 * X, "L+3X-1": L + 3 * X - 1, "L+3X+1": L + 3 * X + 1}[formula]


FORMULAS = ["L", "L+1", "L-1", "L+3X", "L+3X-1", "L+3X+1"]

# 240 x 180, edge 9: window 228 x 168 at (6, 6), 7 x 5 cells of 33 x 34, one root.  Candidates exist for 3 <= x <= 224, 3 <= y <= 164.
W0, H0, E0 = 240, 180, 9
FULL = lattice(3, 223, 3, 163)                # 111 x 41 = 4 551 positions


def _planted(name, pts, Ns, claims=(), W=W0, H=H0, edge=E0, expect=None, **kw):
    img, exp = plant(W, H, edge, pts)
    return Scene(name, W, H, edge, img, Ns, exp if expect is None else expect, claims, **kw)


def _mid_pass(cands, w, h, share):
    """index of the first pass whose list is at least `share` of the candidates"""
    log = pass_log(cands, w, h)
    for k, p in enumerate(log):
        if p["size"] >= share * len(cands):
            return k
    return len(log) - 1


# ---- level sizes ---------------------------------------------------------------------------------------------------------------
LEVEL_SIZES = [1, 2, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097]
# quotas at which the direct passes' capacity min(4096, 2 * vsp_pow2), vsp_pow2 = the power of two >= 2 * (N + 16), is 256 and 512: the
# level of exactly that many candidates is the last one computed directly, the next one runs the list algorithm
DIRECT_CAP_N = {256: [40, 48], 257: [40, 48], 512: [49, 100], 513: [49, 100]}


def level_size_scene(n, extra_N=()):
    pts = valued(subset(FULL, n, 1000 + n))
    cands = ordered(W0, H0, E0, [(x, y, v - 1) for x, y, v in pts])
    Ns = list(extra_N)
    if n > 2:
        k = _mid_pass(cands, 228, 168, 0.2)
        f = FORMULAS[LEVEL_SIZES.index(n) % 6]
        Ns += [n_from_log(cands, 228, 168, k, f), n_from_log(cands, 228, 168, k, "L+3X-1"), n + 5]
    else:
        Ns += [1, 2, 3, 50]
    return _planted("level_%d" % n, pts, sorted(set(Ns)), [(None, "n == %d" % n, lambda p, n=n: p["n"] == n)])


# ---- node sizes by partition route -----------------------------------------------------------------------------------------------
NODE_SIZES = [1, 2, 16, 17, 64, 65, 1023, 1024, 1025]
Q1 = lattice(3, 111, 3, 81)                   # 55 x 20 = 1 100 positions inside the root's first quadrant (x < 114, y < 84)
Q2 = lattice(115, 223, 3, 81)
Q3 = lattice(3, 111, 87, 163)
Q4 = lattice(115, 223, 87, 163)


def node_size_scene(K):
    pts = valued(subset(Q1, K, 2000 + K) + [(151, 31), (41, 123), (171, 131)])
    n = K + 3
    return _planted("node_%d" % K, pts, sorted({n + 1, max(n // 2, 2), max(n // 5, 1)}),
                    [(n + 1, "a node of %d keys was divided" % K, lambda p, K=K: K == 1 or K in p["divided_sizes"])])


def two_big_nodes_scene():
    pts = valued(subset(Q1, 1024, 31) + subset(Q4, 1030, 32) + [(151, 31), (41, 123)])
    return _planted("two_big_nodes", pts, [2056, 700, 64],
                    [(2056, "nodes of 1 024 and 1 030 keys divided in one pass", lambda p: {1024, 1030} <= p["divided_sizes"])])


def quartet_scene():
    pts = valued(subset(Q1, 3, 41) + subset(Q2, 20, 42) + subset(Q3, 5, 43) + subset(Q4, 30, 44))
    return _planted("quartet_3_20_5_30", pts, [59, 30, 12],
                    [(59, "siblings of 3, 20, 5 and 30 keys", lambda p: {3, 20, 5, 30} <= p["divided_sizes"])])


# ---- cut-off size lists of a wanted length -----------------------------------------------------------------------------------------
def cut_list_scene(target):
    """The cut-off stage sorts one entry per divisible node.  Node boundaries do not depend on the keys, so thinning a node of pass k
    to a single key takes exactly one entry off that pass's list."""
    pts = list(FULL)
    for _ in range(2):                        # (thinning turns nodes into leaves one pass earlier: settle once more)
        cands = ordered(W0, H0, E0, [(x, y, value(x, y) - 1) for x, y in pts])
        seen = {}
        log = pass_log(cands, 228, 168, trace=lambda i, nodes: seen.__setitem__(i, nodes))
        k = next(i for i, p in enumerate(log) if p["expand"] >= target)
        drop = set()
        over = log[k]["expand"] - target
        for keys in seen[k]:
            if over and len(keys) > 1:
                drop.update(keys[1:])
                over -= 1
        pts = [(c[0], c[1]) for i, c in enumerate(cands) if i not in drop]
    cands = ordered(W0, H0, E0, [(x, y, value(x, y) - 1) for x, y in pts])
    N = n_from_log(cands, 228, 168, k, "L+3X-1")
    N2 = n_from_log(cands, 228, 168, k, "L") + target // 2          # the walk breaks about half-way through the sorted list
    return _planted("cut_list_%d" % target, valued(pts), [N, N2],
                    [(None, "a size list of %d entries was sorted" % target, lambda p, t=target: t in p["sorted_lengths"])])


# ---- the pass loop's doors ---------------------------------------------------------------------------------------------------------
def close_pair_scene():
    """two candidates 2 px apart: one division of the root leaves both in one child, the list keeps its size, the loop ends with a
    divisible node in the list; equal responses, so the kept key is the first in cell order"""
    pts = [(11, 11, 90), (13, 11, 90)]
    return _planted("close_pair", pts, [2, 5, 400],
                    [(5, "size == prevSize with a divisible node left", lambda p: p["door"] == "size == prevSize, divisible nodes left"),
                     (5, "the kept node's best response is tied", lambda p: p["best_ties"] == 1)])


def exact_doors_scene():
    """a sparse lattice whose every pass is read off the log: N = L, L + 1, L - 1, L + 3X, L + 3X - 1, L + 3X + 1 of two passes"""
    pts = valued(subset(lattice(3, 223, 3, 163, 6, 8), 300, 77))
    cands = ordered(W0, H0, E0, [(x, y, v - 1) for x, y, v in pts])
    Ns = sorted({n_from_log(cands, 228, 168, k, f) for k in (2, 3) for f in FORMULAS})
    L2, X3 = pass_log(cands, 228, 168)[2]["size"], pass_log(cands, 228, 168)[3]
    top = X3["size"] + 3 * X3["expand"]
    return _planted("exact_doors", pts, Ns, [
        (None, "300 candidates", lambda p: p["n"] == 300),
        (L2, "size == N after a full pass", lambda p: p["door"] == "size >= N" and p["passes"][-1]["size"] == L2 and p["cut_rounds"] == 0),
        (L2 + 1, "size == N - 1: the cut-off walk ends on its first division", lambda p: p["cut_first_division_exit"] == 1),
        (L2 - 1, "N = L - 1 = 16 + 3 * 16 - 1: the cut-off stage starts a pass earlier and its walk ends on its last division", lambda p: p["cut_last_division_exit"] == 1),
        (top, "size + 3 * nToExpand == N: one more full pass", lambda p: p["cut_rounds"] == 0 and len(p["passes"]) > 4),
        (top - 1, "size + 3 * nToExpand == N + 1: the cut-off stage", lambda p: p["cut_rounds"] >= 1 and p["passes"][4]["kind"] == "cut"),
        (186, "equal sizes walked: siblings of one division, and children of different divisions",
         lambda p: p["tie_walked_same_division"] > 0 and p["tie_walked_other_division"] > 0)])


# ---- mid-lines and roots -----------------------------------------------------------------------------------------------------------
def midline_scene():
    """keys on midx = 114 and midy = 84 of the root, on 57 / 42 of its first child, on 29 / 21 of the odd-sized grandchild (57 x 42 ->
    halves 29 x 21), and ordinary keys around them so that every node involved is divided"""
    on = [(114, 11), (114, 84), (11, 84), (57, 23), (57, 42), (23, 42), (29, 7), (29, 21), (9, 21), (171, 42), (171, 126), (143, 21)]
    off = [(113, 15), (115, 19), (15, 83), (19, 87), (55, 27), (59, 31), (27, 11), (31, 15), (7, 25), (15, 17), (201, 151), (121, 91)]
    pts = valued(on + off)
    return _planted("midlines", pts, [len(pts) + 1, 12, 7],
                    [(len(pts) + 1, "keys on mid-lines", lambda p: p["midline_keys"] >= 10)])


def _with_helpers(pair, W, H, edge):
    """the 2 x 4 lattice everywhere but around the pair: the list grows in every pass, so the loop does not stop at `size == prevSize`
    before the pair is separated"""
    _, w, h = Scene("", W, H, edge, None, []).window()
    x0, y0 = pair[0][0], pair[0][1]
    return valued([p for p in lattice(3, w - 4, 3, h - 4) if abs(p[0] - x0) > 4 or abs(p[1] - y0) > 6]) + pair


def column_pair_scene(deep):
    """two equal pixels one above the other across a cell-row boundary (rows 36 | 37 of the window): both are kept by FAST and share
    their column.  Alone, one division leaves both in one child and the loop ends; among helpers they are divided until a mid-line
    falls between them."""
    pair = [(100, 36, 120), (100, 37, 120)]
    if not deep:
        return _planted("column_pair", pair + [(40, 120, 77), (190, 50, 66)], [5, 4, 3])
    pts = _with_helpers(pair, W0, H0, E0)
    return _planted("column_pair_deep", pts, [len(pts) + 1], [(None, "the pair is separated", lambda p, n=len(pts): p["n"] == n and p["deepest"] >= 5)])


def row_pair_scene(deep):
    """the same across a cell-column boundary (columns 35 | 36): two candidates one pixel apart in x"""
    pair = [(35, 50, 120), (36, 50, 120)]
    if not deep:
        return _planted("row_pair", pair + [(40, 120, 77), (190, 50, 66)], [5, 4, 3])
    pts = _with_helpers(pair, W0, H0, E0)
    return _planted("row_pair_deep", pts, [len(pts) + 1], [(None, "deep division", lambda p: p["deepest"] >= 5)])


def one_px_wide_scene():
    """132 x 240, edge 9 (window 120 x 228, one root, nodes half as wide as high): the column pair (14, 101 | 102) across the cell-row
    boundary shares a node 1 px wide; halfX = ceil(1 / 2) = 1 sends every key to n1 / n3.  (In a landscape frame a node is 1 px
    high before it is 1 px wide, and no two candidates share a 1 x 1 node.)"""
    W, H, edge = 132, 240, 9
    pts = _with_helpers([(14, 101, 120), (14, 102, 120)], W, H, edge)
    return _planted("one_px_wide", pts, [len(pts) + 1, len(pts) // 2],
                    [(len(pts) + 1, "a node 1 px wide was divided", lambda p: p["narrowest_w"] == 1)], W=W, H=H, edge=edge)


def wide_scene(name, W, H, edge, seed, n, Ns, on_boundaries=True):
    """frames with several roots; keys on every root boundary int(hX * i) and one pixel to either side of it"""
    b = m.borders(W, H, edge)
    w, h = b[2] - b[0], b[3] - b[1]
    nIni = m.n_roots(w, h)
    hX = np.float32(w) / np.float32(nIni)
    pts = set()
    if on_boundaries:
        for i in range(1, nIni):
            e = int(np.float32(hX * np.float32(i)))
            for k, x in enumerate((e - 2, e, e + 2)):
                if 3 <= x <= w - 4:
                    pts.add((x, 3 + 4 * ((5 * i + 3 * k) % ((h - 8) // 4))))
    free = [p for p in lattice(3, w - 4, 3, h - 4, 4, 4) if all(abs(p[0] - q[0]) > 3 or abs(p[1] - q[1]) > 3 for q in pts)]
    pts.update(subset(free, n, seed))
    pts = valued(sorted(pts, key=lambda p: (p[1], p[0])))
    return _planted(name, pts, Ns, [(None, "%d roots" % nIni, lambda p, r=nIni: p["nIni"] == r)], W=W, H=H, edge=edge)


# ---- kept-node ties --------------------------------------------------------------------------------------------------------------
def kept_tie_scene():
    """a kept node over two FAST cells (columns 3..35 | 36..68): the right-hand cell's key lies on an earlier row and ties the
    left-hand cell's, so the first key in cell order (left cell) is not the first in raster order"""
    pts = [(31, 21, 150), (41, 13, 150), (21, 29, 100), (200, 150, 60)]
    return _planted("kept_tie", pts, [1, 2],
                    [(1, "tied best response in a kept node", lambda p: p["best_ties"] >= 1)])


# ---- the per-cell rule -----------------------------------------------------------------------------------------------------------
def _cell11(extra=()):
    # cell (1, 1) detects window-relative columns 36..68 and rows 37..70
    weak = [(40, 41, MINTH + 1), (46, 45, INI), (52, 49, 14), (58, 53, MINTH)]          # responses MINTH, INI - 1, 13 and MINTH - 1
    return weak + list(extra) + [(150, 120, 99), (200, 20, 201)]


def weak_cell_scene():
    pts = _cell11()
    exp = [(x, y, v - 1) for x, y, v in pts if v > MINTH]
    return _planted("weak_cell", pts, [10, 3], [(None, "retried in", lambda p: p["n"] == 5)], expect=exp)


def weak_cell_with_strong_scene():
    pts = _cell11([(64, 65, INI + 1)])
    exp = [(x, y, v - 1) for x, y, v in pts if v > INI]
    return _planted("weak_cell_with_strong", pts, [10, 3], [(None, "weak ones dropped", lambda p: p["n"] == 3)], expect=exp)


def domain_edges_scene():
    """first and last column and row of cell (1, 1)'s detection domain, of the clipped last cell (6, 4), and of the window"""
    pts = [(36, 37), (68, 37), (36, 70), (68, 70), (52, 53),            # cell (1, 1)
           (201, 139), (224, 139), (201, 164), (224, 164),                # cell (6, 4): clipped at maxBorder
           (3, 3), (224, 3), (3, 164)]                                    # the window's corners
    return _planted("domain_edges", valued(pts), [13, 6])


def adjacent_scene():
    """two equal neighbours inside one cell suppress each other; the same pair across a cell boundary is kept"""
    inside = [(50, 50, 130), (51, 50, 130)]
    across = [(68, 100, 131), (69, 100, 131)]
    pts = inside + across + [(150, 30, 88)]
    exp = [(x, y, v - 1) for x, y, v in across + [(150, 30, 88)]]
    return _planted("adjacent", pts, [4, 2], expect=exp)


def skipped_column_scene():
    """883 x 132, edge 9: window 871 x 120, 29 cell columns of 31 px; the last column starts at 868 >= maxBorderX - 3 and is
    skipped (:825).  Keys on the window's last detectable column (867) belong to the column before it."""
    W, H, edge = 883, 132, 9
    pts = valued([(867, 11), (867, 59), (865, 35), (836, 19), (3, 3), (500, 60), (440, 100)])
    s = _planted("skipped_column", pts, [8, 30], W=W, H=H, edge=edge)
    assert m.skipped_cells(W, H, edge) == 4
    return s


# ---- multi-level, capacity, the generic sort ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def multilevel_scenes():
    pts = valued(subset(lattice(3, 223, 3, 163, 6, 8), 400, 5))
    planted_img = plant(W0, H0, 19, [(x, y, v) for x, y, v in pts if x <= 204 and y <= 144])[0]
    # (lone pixels fade in the pyramid: 3 x 3 blobs survive two or three levels)
    for x, y, v in pts[::7]:
        planted_img[y + 14:y + 17, x + 14:x + 17] = v
    tex = synth.texture_image(W0, H0, seed=21)
    return [Scene("multi4_planted", W0, H0, 19, planted_img, [300], ini=20, minth=7, sf=1.2, nlevels=4),
            Scene("multi8_texture", 346, 260, 15, synth.texture_image(346, 260, seed=22), [1000], ini=20, minth=7, sf=1.2, nlevels=8),
            Scene("multi4_texture", W0, H0, 19, tex, [500], ini=10, minth=0, sf=1.2, nlevels=4)]


@functools.lru_cache(maxsize=None)
def capacity_scenes():
    """the first pass over nIni roots yields up to 4 * nIni nodes before any comparison with N: with a level quota below that, the
    reference returns them all"""
    out = [Scene("capacity_640x120", 640, 120, 19, synth.texture_image(640, 120, seed=9), [1, 5, 12], ini=10, minth=0),
           Scene("capacity_1000x100", 1000, 100, 19, synth.texture_image(1000, 100, seed=9), [1, 5, 12], ini=10, minth=0),
           Scene("capacity_640x120_3levels", 640, 120, 19, synth.texture_image(640, 120, seed=9), [30], ini=10, minth=0, sf=1.2, nlevels=3)]
    return out


def _whole_lattice(name, W, H, edge, dx, dy, formulas, claim):
    b = m.borders(W, H, edge)
    w, h = b[2] - b[0], b[3] - b[1]
    img, exp = plant(W, H, edge, valued(lattice(3, w - 4, 3, h - 4, dx, dy)))
    cands = ordered(W, H, edge, exp)
    log = pass_log(cands, w, h)
    k = max(i for i, p in enumerate(log) if p["size"] + 40 < 16000 and p["expand"])          # the last pass a level's 16 000 nodes allow
    L, X = log[k]["size"], log[k]["expand"]
    Ns = sorted({{"L+1": L + 1, "L+X/2": L + X // 2, "L+3X-1": L + 3 * X - 1}[f] for f in formulas})
    return Scene(name, W, H, edge, img, Ns, exp, [(None, claim[0], claim[1])])


@functools.lru_cache(maxsize=None)
def big_list_scenes():
    """The longest cut-off size lists.  A frame with two roots has 2 * 4^5 = 8 192 nodes after its fifth pass, and N only has to pass
    that for the cut-off stage to sort their divisible children: the 2 x 4 lattice on 752 x 480 (window 740 x 468, 42 572 candidates)
    sorts 8 180 entries, at N = L + 1 (the walk ends on its first division) and at N = L + X / 2 (it ends half-way); the 4 x 6 lattice
    sorts 2 048 and then 4 536.  Both are beyond the register sorts of 4 096 items.  With one root the longest lists stay below that:
    346 x 260 white noise at thresholds 1 / 1 (8 929 candidates, a list of 2 987) and its lattice (10 004 candidates, 3 843)."""
    W, H, edge = 346, 260, 9
    b = m.borders(W, H, edge)
    w, h = b[2] - b[0], b[3] - b[1]
    noise = np.random.default_rng(346).integers(0, 256, (H, W), dtype=np.uint8)
    Nn = n_from_log(m.cell_candidates(noise, edge, 1, 1), w, h, 5, "L+3X-1")
    above = ("a size list above 4 096 entries", lambda p: p["largest_sort"] > 4096)
    below = ("a size list above 2 048 entries", lambda p: 2048 < p["largest_sort"] <= 4096)
    return (Scene("noise_346x260", W, H, edge, noise, [Nn], None, [(None,) + below], ini=1, minth=1),
            _whole_lattice("lattice_346x260", W, H, edge, 2, 4, ["L+3X-1"], below),
            _whole_lattice("lattice_752x480", 752, 480, edge, 2, 4, ["L+1", "L+X/2"], above),
            _whole_lattice("lattice46_752x480", 752, 480, edge, 4, 6, ["L+1"], above))


@functools.lru_cache(maxsize=None)
def single_level_scenes():
    s = [level_size_scene(n, DIRECT_CAP_N.get(n, ())) for n in LEVEL_SIZES]
    s += [node_size_scene(K) for K in NODE_SIZES]
    s += [two_big_nodes_scene(), quartet_scene()]
    s += [cut_list_scene(t) for t in (511, 512, 513, 1024, 1025)]
    s += [close_pair_scene(), exact_doors_scene()]
    s += [midline_scene(), column_pair_scene(False), column_pair_scene(True), row_pair_scene(False), row_pair_scene(True), one_px_wide_scene(),
          kept_tie_scene()]
    s += [wide_scene("roots_2", 240, 132, 9, 51, 60, [70, 31, 8]),
          wide_scene("roots_3_ratio_2p5", 312, 132, 9, 52, 80, [100, 40, 12]),
          wide_scene("roots_5", 620, 132, 9, 53, 150, [170, 77, 20]),
          wide_scene("roots_7", 640, 120, 19, 54, 120, [140, 60, 28])]
    s += [weak_cell_scene(), weak_cell_with_strong_scene(), domain_edges_scene(), adjacent_scene(), skipped_column_scene()]
    return tuple(s)


def scene_cases():
    """(scene, N) pairs of the single-level planted scenes"""
    return [(s, N) for s in single_level_scenes() for N in s.Ns]
