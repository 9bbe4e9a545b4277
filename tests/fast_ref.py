"""cv::FAST(TYPE_9_16, nonmax suppression) by brute force, shared by tests/test_oracle_stages.py (whole images) and
tests/octree_model.py (one call per cell window).  Written from the definition of the detector, not from fast.cpp."""
import numpy as np

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
        (-2, 2), (-1, 3)]


def fast_np(img, threshold):
    """score = the largest t for which 9 contiguous ring pixels are all brighter than centre + t or all darker than centre - t
    = max over the 16 arcs of min(d) - 1 and min(-d) - 1; corner iff score >= threshold; kept iff strictly above its 8 neighbours'
    scores (non-corners count 0); 3-px margin.  Returns (n, 3) int32 rows x, y, score in raster order."""
    h, w = img.shape
    if h < 7 or w < 7:
        return np.zeros((0, 3), np.int32)
    s = img.astype(np.int64)
    d = np.stack([s[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - s[3:h - 3, 3:w - 3] for dx, dy in RING])      # ring - centre
    best = np.full(d.shape[1:], -(1 << 20), np.int64)
    for k in range(16):
        arc = d[[(k + i) % 16 for i in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(axis=0) - 1, (-arc).min(axis=0) - 1))
    score = np.zeros((h, w), np.int64)
    score[3:h - 3, 3:w - 3] = np.where(best >= threshold, best, 0)
    out = []
    for y, x in np.argwhere(score >= max(threshold, 1)):          # (row-major: raster order; the margin holds zeros)
        v = score[y, x]
        nb = score[y - 1:y + 2, x - 1:x + 2].copy()
        nb[1, 1] = -1
        if v > nb.max():
            out.append((x, y, v))
    return np.array(out, np.int32).reshape(-1, 3)
