"""Keypoint selection of the ORB extractor as a list model: ORBextractor's per-level quotas (src/ORBextractor.cc:444-455), the
FAST cell grid of ComputeKeyPointsOctTree (:792-878), ExtractorNode::DivideNode (:500-556) and DistributeOctTree (:558-782),
and the keypoint record a level and a frame carry out (:886-896, :1131-1172).

Written from the reference's text in Python integers and a doubly linked list of node objects (std::list); where the reference
computes in float, numpy.float32 one operation at a time.  Nothing here is shared with oracle/orc_orb.c or with octree_kernel,
which does not run this algorithm but computes its result: a mistake either of them makes is not made here for the same reason.

`wrong=NAME` changes one comparison or one order (WRONG_VARIANTS): tests/test_oracle_octree_model.py shows for every name a
scene of tests/octree_scenes.py on which that variant differs from the rule, so the scenes do reach the comparison."""
import numpy as np

from fast_ref import fast_np

F = np.float32

WRONG_VARIANTS = {
    # DivideNode
    "mid_le": "`<=` at the mid-lines (:534, :536, :541)",
    "half_floor": "halfX / halfY by floor instead of ceil (:502-503)",
    # roots
    "root_round_half_even": "nIni by rint instead of round (:562)",
    "root_edge_float": "root edges hX * i kept as floats, not truncated to int (:574-575)",
    "root_by_edges": "(added) a key goes to the root whose integer edges hold it, not to root kp.pt.x / hX (:588)",
    # full passes
    "push_back_children": "children appended at the back of the list (:642)",
    "parent_keeps_place": "children inserted at the parent's position (:642, :681)",
    "n_strict": "`size > N` after a full pass (:688)",
    "expand_ge": "`size + 3 * nToExpand >= N` (:692)",
    "no_prevsize_exit": "no `size == prevSize` exit (:688): the loop ends when nothing was divided",
    # cut-off stage
    "cut_no_break": "the cut-off walk runs to its end (:749)",
    "cut_n_strict": "(added) `size > N` inside the cut-off walk (:749)",
    "cut_smallest_first": "the cut-off walk starts at the smallest node (:704)",
    "size_tie_first_created": "among equal sizes the node created first is divided first (:703)",
    "cut_once": "one cut-off round only (:695)",
    # selection
    "best_tie_last": "`>=` in the selection (:771)",
    "best_raster_order": "a node's keys in raster order, not in cell order (:869-874)",
    # cells
    "retry_always": "minThFAST also when the cell had candidates (:849)",
    "retry_never": "no minThFAST retry (:849)",
    "cell_order_raster": "the level's candidates in image raster order (:810, :820)",
    "nms_across_cells": "one FAST over the whole level window (:832)",
    "cell_shift_ini": "(added) candidates shifted by the clipped window origin only: same as the rule (see INDISTINGUISHABLE)",
    # quotas
    "quota_floor": "floor instead of cvRound (:451)",
    "quota_last_unclamped": "last level nfeatures - sum without max(., 0) (:455)",
}

# variants no reachable input can tell from the rule, with the reason
INDISTINGUISHABLE = {
    "cell_shift_ini": "iniX - minBorderX == j * wCell by construction (:822), so shifting by the window origin relative to the border "
                      "IS the reference's `j * wCell` shift; kept as a note that the two spellings are one rule",
}


def cv_round(v):
    """cvRound(double): nearest, halves to even"""
    return int(np.rint(np.float64(v)))


def c_round(v):
    """round(float): nearest, halves away from zero (v >= 0 here)"""
    v = F(v)
    fl = F(np.floor(v))
    return int(fl) + (1 if F(v - fl) >= F(0.5) else 0)


# ---- constructor ------------------------------------------------------------------------------------------------------------
def scale_factors(scaleFactor, nlevels):
    """mvScaleFactor :426-431: float vector, each entry the float product with the double member scaleFactor, stored as float"""
    sf = [F(1.0)]
    for _ in range(1, nlevels):
        sf.append(F(np.float64(sf[-1]) * np.float64(F(scaleFactor))))
    return sf


def features_per_level(nfeatures, scaleFactor, nlevels, wrong=None):
    """mnFeaturesPerLevel :445-455"""
    factor = F(np.float64(1.0) / np.float64(F(scaleFactor)))                 # float factor = 1.0f / (double)scaleFactor
    with np.errstate(all="ignore"):
        n_desired = F(F(F(nfeatures) * F(F(1) - factor)) / F(F(1) - F(np.power(np.float64(factor), np.float64(nlevels)))))
    out, total = [], 0
    for _ in range(nlevels - 1):
        q = int(np.floor(n_desired)) if wrong == "quota_floor" else cv_round(n_desired)
        out.append(q)
        total += q
        n_desired = F(n_desired * factor)
    last = nfeatures - total
    out.append(last if wrong == "quota_last_unclamped" else max(last, 0))
    return out


# ---- the cell grid ----------------------------------------------------------------------------------------------------------
def borders(cols, rows, edge):
    return edge - 3, edge - 3, cols - edge + 3, rows - edge + 3          # minBorderX, minBorderY, maxBorderX, maxBorderY


def cell_grid(cols, rows, edge):
    """:794-808 -> (nCols, nRows, wCell, hCell)"""
    minBX, minBY, maxBX, maxBY = borders(cols, rows, edge)
    width, height = F(maxBX - minBX), F(maxBY - minBY)
    nCols, nRows = int(F(width / F(30))), int(F(height / F(30)))
    wCell, hCell = int(np.ceil(F(width / F(nCols)))), int(np.ceil(F(height / F(nRows))))
    return nCols, nRows, wCell, hCell


def cell_windows(cols, rows, edge):
    """The FAST windows :810-828 as (i, j, x0, x1, y0, y1) in level pixel coordinates, skipped cells left out"""
    minBX, minBY, maxBX, maxBY = borders(cols, rows, edge)
    nCols, nRows, wCell, hCell = cell_grid(cols, rows, edge)
    out = []
    for i in range(nRows):
        iniY = F(minBY + i * hCell)
        maxY = F(iniY + F(hCell + 6))
        if iniY >= maxBY - 3:
            continue
        if maxY > maxBY:
            maxY = F(maxBY)
        for j in range(nCols):
            iniX = F(minBX + j * wCell)
            maxX = F(iniX + F(wCell + 6))
            if iniX >= maxBX - 3:
                continue
            if maxX > maxBX:
                maxX = F(maxBX)
            out.append((i, j, int(iniX), int(maxX), int(iniY), int(maxY)))
    return out


def skipped_cells(cols, rows, edge):
    nCols, nRows, _, _ = cell_grid(cols, rows, edge)
    return nCols * nRows - len(cell_windows(cols, rows, edge))


def cell_candidates(level_image, edge, iniTh, minTh, wrong=None):
    """:792-878: level_image is the level without its border (rows x cols uint8).  Returns [(x, y, response)] relative to
    (minBorderX, minBorderY), in the reference's order: cell row, cell column, raster inside the cell."""
    rows, cols = level_image.shape
    minBX, minBY, maxBX, maxBY = borders(cols, rows, edge)
    _, _, wCell, hCell = cell_grid(cols, rows, edge)
    if wrong == "nms_across_cells":
        return [(int(x), int(y), int(r)) for x, y, r in fast_np(level_image[minBY:maxBY, minBX:maxBX], iniTh)]
    out = []
    for i, j, x0, x1, y0, y1 in cell_windows(cols, rows, edge):
        win = level_image[y0:y1, x0:x1]
        cell = fast_np(win, iniTh)
        if wrong == "retry_always" or (len(cell) == 0 and wrong != "retry_never"):
            cell = fast_np(win, minTh)
        for x, y, r in cell:
            if wrong == "cell_shift_ini":
                out.append((int(x) + x0 - minBX, int(y) + y0 - minBY, int(r)))
            else:
                out.append((int(x) + j * wCell, int(y) + i * hCell, int(r)))
    if wrong == "cell_order_raster":
        out.sort(key=lambda c: (c[1], c[0]))
    return out


# ---- std::list ---------------------------------------------------------------------------------------------------------------
class _Node:
    __slots__ = ("ULx", "URx", "ULy", "BRy", "keys", "nomore", "prev", "next", "seq", "depth")

    def __init__(self, ULx, URx, ULy, BRy, seq, depth):
        self.ULx, self.URx, self.ULy, self.BRy = ULx, URx, ULy, BRy
        self.keys, self.nomore, self.prev, self.next, self.seq, self.depth = [], False, None, None, seq, depth


class _List:
    def __init__(self):
        self.head = self.tail = None
        self.size = 0

    def insert_before(self, pos, node):        # pos None: push_back
        node.next = pos
        node.prev = pos.prev if pos is not None else self.tail
        if node.prev is not None:
            node.prev.next = node
        else:
            self.head = node
        if pos is not None:
            pos.prev = node
        else:
            self.tail = node
        self.size += 1

    def push_front(self, node):
        self.insert_before(self.head, node)

    def push_back(self, node):
        self.insert_before(None, node)

    def erase(self, node):                     # returns the node after it
        if node.prev is not None:
            node.prev.next = node.next
        else:
            self.head = node.next
        if node.next is not None:
            node.next.prev = node.prev
        else:
            self.tail = node.prev
        self.size -= 1
        return node.next

    def __iter__(self):
        n = self.head
        while n is not None:
            yield n
            n = n.next


def _half(extent, wrong):
    v = F(F(extent) / F(2))
    return int(np.floor(v)) if wrong == "half_floor" else int(np.ceil(v))


def _divide(node, cands, seq, probe, wrong):
    """DivideNode :500-556.  Only UL.x, UR.x, UL.y and BR.y of a node are ever read; the children n1..n4 get them as the
    reference's eight corner assignments give them."""
    halfX, halfY = _half(node.URx - node.ULx, wrong), _half(node.BRy - node.ULy, wrong)
    midx, midy = node.ULx + halfX, node.ULy + halfY
    d = node.depth + 1
    n1 = _Node(node.ULx, midx, node.ULy, midy, seq, d)
    n2 = _Node(midx, node.URx, node.ULy, midy, seq + 1, d)
    n3 = _Node(node.ULx, midx, midy, node.BRy, seq + 2, d)
    n4 = _Node(midx, node.URx, midy, node.BRy, seq + 3, d)
    le = wrong == "mid_le"
    for k in node.keys:
        x, y = cands[k][0], cands[k][1]
        if x == midx or y == midy:
            probe["midline_keys"] += 1
        left = (x <= midx) if le else (x < midx)
        top = (y <= midy) if le else (y < midy)
        (n1 if top else n3).keys.append(k) if left else (n2 if top else n4).keys.append(k)
    for c in (n1, n2, n3, n4):
        if len(c.keys) == 1:
            c.nomore = True
    probe["largest_divided"] = max(probe["largest_divided"], len(node.keys))
    probe["deepest"] = max(probe["deepest"], d)
    probe["divided_sizes"].add(len(node.keys))
    probe["narrowest_w"] = min(probe["narrowest_w"], node.URx - node.ULx)
    probe["narrowest_h"] = min(probe["narrowest_h"], node.BRy - node.ULy)
    probe["divisions"] += 1
    return [n1, n2, n3, n4]


def n_roots(w, h, wrong=None):
    ratio = F(F(w) / F(h))
    return int(np.rint(ratio)) if wrong == "root_round_half_even" else c_round(ratio)


def distribute(cands, w, h, N, wrong=None, trace=None):
    """DistributeOctTree :558-782 over cands = [(x, y, response)] (coordinates relative to the border window of w x h pixels).

    Returns (kept, probe): kept = indices into cands in list order, front to back.  trace(i, keys_per_node) is called after pass i
    with the key indices of every node in list order (tests/octree_scenes.py builds its planted scenes from it).

    The reference sorts (size, ExtractorNode*) pairs (:703): equal sizes are ordered by address, which no text fixes.  The
    project defines it (H8 in oracle/README.md) as creation order, a later node comparing greater.  The cut-off stage walks the
    sorted list from its back, so among equal sizes THE NODE CREATED LATER IS DIVIDED FIRST (n4 before n3 before n2 before n1 of
    one division, and any child of a later division before any child of an earlier one).  A size list only ever holds children of
    one pass or of one cut-off round (:623, :701 clear it), so ties between nodes of different passes never meet in a sort: the probe
    counts the walked ties between siblings of one division and between children of different divisions."""
    probe = dict(n=len(cands), nIni=0, roots_kept=0, passes=[], exit_pass=None, door=None, cut_rounds=0, largest_divided=0, largest_sort=0,
                 adjacent_equal_sizes=0, best_ties=0, midline_keys=0, deepest=0, divisions=0, cut_first_division_exit=0,
                 cut_last_division_exit=0, root_boundary_keys=0, divided_sizes=set(), narrowest_w=1 << 30, narrowest_h=1 << 30, sorted_lengths=[],
                 tie_walked_same_division=0, tie_walked_other_division=0, kept_nodes=[])
    nIni = n_roots(w, h, wrong)
    probe["nIni"] = nIni
    hX = F(F(w) / F(nIni))
    L = _List()
    seq = 0
    roots = []
    for i in range(nIni):
        lo, hi = F(hX * F(i)), F(hX * F(i + 1))
        if wrong != "root_edge_float":
            lo, hi = int(lo), int(hi)
        ni = _Node(lo, hi, 0, h, seq, 0)
        seq += 1
        L.push_back(ni)
        roots.append(ni)
    for k, c in enumerate(cands):
        r = int(F(F(c[0]) / hX))
        by_edges = [i for i, ni in enumerate(roots) if ni.ULx <= c[0] < ni.URx]
        if by_edges != [r]:
            probe["root_boundary_keys"] += 1
            if wrong == "root_by_edges" and by_edges:
                r = by_edges[0]
        roots[r].keys.append(k)
    lit = L.head
    while lit is not None:
        if len(lit.keys) == 1:
            lit.nomore = True
            lit = lit.next
        elif not lit.keys:
            lit = L.erase(lit)
        else:
            lit = lit.next
    probe["roots_kept"] = L.size

    def add_children(children, vsp, pos):
        """:640-679: each non-empty child is linked in (front of the list by the rule), those with more than one key are noted"""
        n = 0
        for c in children:
            if c.keys:
                if wrong == "push_back_children":
                    L.push_back(c)
                elif wrong == "parent_keeps_place":
                    L.insert_before(pos, c)
                else:
                    L.push_front(c)
                if len(c.keys) > 1:
                    n += 1
                    vsp.append((len(c.keys), c))
        return n

    finish = False
    while not finish:
        prev_size = L.size
        n_to_expand, divided = 0, 0
        vsp = []
        lit, last = L.head, L.tail
        while lit is not None:
            at_last = lit is last
            if lit.nomore:
                lit = lit.next
            else:
                children = _divide(lit, cands, seq, probe, wrong)
                seq += 4
                divided += 1
                n_to_expand += add_children(children, vsp, lit)
                lit = L.erase(lit)
            if at_last:                    # (only push_back_children puts anything behind the pass's last node: it waits for the next pass)
                break
        probe["passes"].append(dict(kind="full", before=prev_size, size=L.size, expand=n_to_expand))
        if trace is not None:
            trace(len(probe["passes"]) - 1, [list(n.keys) for n in L])
        reached = L.size > N if wrong == "n_strict" else L.size >= N
        stalled = divided == 0 if wrong == "no_prevsize_exit" else L.size == prev_size
        if reached or stalled:
            finish = True
            probe["exit_pass"] = len(probe["passes"]) - 1
            probe["door"] = "size >= N" if reached else "size == prevSize"
            if not reached and any(not n.nomore for n in L):
                probe["door"] = "size == prevSize, divisible nodes left"
        elif (L.size + 3 * n_to_expand >= N) if wrong == "expand_ge" else (L.size + 3 * n_to_expand > N):
            while not finish:
                prev_size = L.size
                prev, vsp = vsp, []
                # sort(:703) ascending by (size, pointer); pointer order = creation order (see the docstring)
                prev.sort(key=lambda sp: (sp[0], -sp[1].seq if wrong == "size_tie_first_created" else sp[1].seq))
                probe["largest_sort"] = max(probe["largest_sort"], len(prev))
                probe["sorted_lengths"].append(len(prev))
                probe["adjacent_equal_sizes"] += sum(1 for a, b in zip(prev, prev[1:]) if a[0] == b[0])
                probe["cut_rounds"] += 1
                walk = prev if wrong == "cut_smallest_first" else prev[::-1]
                for j, (_, node) in enumerate(walk):
                    if j and walk[j - 1][0] == walk[j][0]:        # an equal-size pair whose order the walk did use: both were divided
                        same = (walk[j - 1][1].seq - nIni) // 4 == (node.seq - nIni) // 4
                        probe["tie_walked_same_division" if same else "tie_walked_other_division"] += 1
                    children = _divide(node, cands, seq, probe, wrong)
                    seq += 4
                    add_children(children, vsp, node)
                    L.erase(node)
                    if wrong != "cut_no_break" and (L.size > N if wrong == "cut_n_strict" else L.size >= N):
                        probe["cut_first_division_exit"] += j == 0
                        probe["cut_last_division_exit"] += j == len(walk) - 1 and len(walk) > 1
                        break
                probe["passes"].append(dict(kind="cut", before=prev_size, size=L.size, expand=len(vsp)))
                if L.size >= N or L.size == prev_size or wrong == "cut_once":
                    finish = True
                    probe["exit_pass"] = len(probe["passes"]) - 1
                    probe["door"] = "cut: size >= N" if L.size >= N else "cut: size == prevSize" if L.size == prev_size else "cut_once"
        if len(probe["passes"]) > 64:
            raise RuntimeError("the pass loop does not end")
    kept = []
    for node in L:                             # :763-779
        keys = sorted(node.keys, key=lambda k: (cands[k][1], cands[k][0])) if wrong == "best_raster_order" else node.keys
        best, max_response = keys[0], cands[keys[0]][2]
        for k in keys[1:]:
            r = cands[k][2]
            if (r >= max_response) if wrong == "best_tie_last" else (r > max_response):
                best, max_response = k, r
        if sum(1 for k in keys if cands[k][2] == max_response) > 1:
            probe["best_ties"] += 1
        kept.append(best)
        probe["kept_nodes"].append((node.ULx, node.URx, node.ULy, node.BRy))
    return kept, probe


# ---- the records ---------------------------------------------------------------------------------------------------------------
def level_keypoints(level_image, level, edge, N, sf_level, iniTh, minTh, wrong=None):
    """:792-896 for one level: ([(x, y, response, octave, size)] with the border added, probe, candidates)"""
    rows, cols = level_image.shape
    minBX, minBY, maxBX, maxBY = borders(cols, rows, edge)
    cands = cell_candidates(level_image, edge, iniTh, minTh, wrong)
    kept, probe = distribute(cands, maxBX - minBX, maxBY - minBY, N, wrong)
    size = int(F(F(31) * F(sf_level)))                                      # const int scaledPatchSize = PATCH_SIZE * mvScaleFactor[level]
    return [(cands[k][0] + minBX, cands[k][1] + minBY, cands[k][2], level, size) for k in kept], probe, cands


def frame_keypoints(levels, sfs, lap=(0, 1000)):
    """operator() :1131-1172: levels[l] = level_keypoints records.  Returns (monoIndex, [(x, y, response, octave, size)]) with x, y as
    float32 scaled to level 0 and the records in output order: outside the lapping area from the front, inside it from the back."""
    n = sum(len(lv) for lv in levels)
    out = [None] * n
    mono, stereo = 0, n - 1
    for level, kps in enumerate(levels):
        for x, y, r, o, s in kps:
            x, y = F(x), F(y)
            if level != 0:
                x, y = F(x * F(sfs[level])), F(y * F(sfs[level]))
            if lap[0] <= x <= lap[1]:
                out[stereo] = (x, y, r, o, s)
                stereo -= 1
            else:
                out[mono] = (x, y, r, o, s)
                mono += 1
    return mono, out
