"""Frame::ComputeStereoMatches, the brute-force 2-NN with Lowe's test, the window matchers' best / second rule,
MapPoint::ComputeDistinctiveDescriptors and the stable response sort as plain models, written from the reference's text (src/Frame.cc
:869-1048, :1228-1240; src/ORBmatcher.cc:754-774; src/MapPoint.cc:349-423; src/MixedFrame.cpp:211-225), not from oracle/*.c or the
kernels.  Python integers throughout; numpy.float32, one operation at a time, only where the reference computes in float (the row
band, the u window, the three scaled coordinates, the parabola, the disparity and the median cut; Lowe's test compares float distances
with a double product).  The 2-NN takes its nq x nt distance table from numpy (exact small integers, see hamming_table) because the
largest scene has 4.9 million pairs; the selection is on integer keys.

Every model takes `wrong=`: a named wrong variant that changes one comparison (the *_WRONG tables below).  tests/helper_scenes.py plants
the inputs, tests/test_oracle_helper_models.py holds the oracle to the models and shows that the scenes tell every variant from the
rule, tests/test_gpu_helper_models.py holds the kernels."""
import collections
import math

import numpy as np

F = np.float32
TH_LOW, TH_HIGH = 50, 100                                      # ORBmatcher.cc:36-37
INT_MAX = 2 ** 31 - 1
KNN_NONE = (-1, 0x7fffffff)                                    # a missing neighbour: (trainIdx, distance)

STEREO_WRONG = {
    "band_exclusive": "the row band without its two end rows: minr < row < maxr",
    "band_round": "the row band's ends rounded to nearest in place of ceil / floor",
    "octave_strict": "only right keypoints of the left keypoint's own octave",
    "u_strict": "uR > minU && uR < maxU",
    "desc_tie_last": "dist <= bestDist: the last of equal descriptor distances wins",
    "th_orb_le": "bestDist <= thOrbDist: 75 accepted",
    "level_round_half_even": "rintf for the three scaled coordinates",
    "sad_tie_last": "dist <= bestDist over the shifts: the last of equal norms wins",
    "inc_edge_keep": "a best shift at -5 / +5 is kept (the missing neighbour read as the edge value itself)",
    "disp_zero_rejected": "disparity > minD",
    "disp_le_max": "disparity <= maxD",
    "zero_branch_float": "disparity <= 0: bestuR = uL - 0.01f in float",
    "median_lower": "the median taken at rank (n - 1) / 2",
    "cut_gt": "only norms > thDist are taken back",
    "th_double": "thDist = (float)(1.5 * 1.4 * median) with the product in double",
}
KNN_WRONG = {"tie_last": "equal distances resolved by the higher train index"}
LOWE_WRONG = {"ratio_le": "<= for <", "ratio_float": "the product d1 * 0.7f in float"}
WINDOW_WRONG = {"tie_last": "dist <= bestDist: the last of equal distances becomes the best",
                "second_needs_strict": "a candidate equal to the best never becomes the second"}
DISTINCTIVE_WRONG = {"median_upper": "the median read at N / 2", "first_tie_last": "median <= BestMedian: the last smallest median wins"}
SORT_WRONG = {"unstable_reverse": "equal responses in descending index order"}


def as_ints(desc):
    return [int.from_bytes(bytes(bytearray(np.asarray(d, np.uint8)[:32])), "little") for d in desc]


def popcount(v):
    return bin(v).count("1")


def c_round(v):
    """roundf / round of a float32: halves away from zero; the value stays a float32"""
    v = float(v)
    return F(math.floor(v + 0.5) if v >= 0 else -math.floor(-v + 0.5)) if abs(v) < 2.0 ** 23 else F(v)


# ---- Frame::ComputeStereoMatches -----------------------------------------------------------------------------------------------
def stereo_matches(levels_left, levels_right, level_sizes, scale_factors, inv_scale_factors, kL, dL, kR, dR, mb, mbf, wrong=None):
    """src/Frame.cc:869-1048.  levels_* = mvImagePyramid of the two extractors (2-D uint8 arrays, level_sizes = their (cols, rows)),
    scale_factors / inv_scale_factors = mvScaleFactors / mvInvScaleFactors, kL / kR keypoint records (x, y, octave), dL / dR 32-byte
    descriptors.  Returns (mvuRight, mvDepth as float32 arrays, the number of accepted matches before the median cut, probe).

    No row table is kept: the candidates of a left keypoint are the right keypoints whose band [floor(y - r), ceil(y + r)] holds the
    row (size_t)vL, in iR order -- vRowIndices[vL]'s push_back order.

    What the reference leaves undefined and the model defines (each counted in the probe): a left keypoint whose row is outside
    [0, nRows) has no candidates (`row_outside`; the reference indexes vRowIndices out of range); band rows outside the image are
    dropped; a patch that leaves its level image skips the keypoint (`patch_outside`; cv::Mat::rowRange / colRange throw there, and
    the iniu / endu test does not cover the shifts to the left of scaleduR0); with no accepted match nothing is cut (`nmatch_zero`;
    the reference reads vDistIdx[0] of an empty vector).

    `deltaR < -1 || deltaR > 1` cannot fire.  The shift kept is the FIRST smallest norm and it is neither -5 nor +5, so with
    a = dist1 - dist2 > 0 (strictly: an equal earlier norm would have been kept instead) and b = dist3 - dist2 >= 0, integers below
    2^15 and exact in float, deltaR = (dist1 - dist3) / (2 (dist1 + dist3 - 2 dist2)) = (a - b) / (2 (a + b)) with a + b > 0, and
    |a - b| <= a + b gives |deltaR| <= 0.5; the division rounds a quotient of magnitude <= 0.5 to at most 0.5.  The denominator is
    not 0 for the same reason.  Both comparisons are kept below, as the reference has them; the probe counts `delta_rejected`."""
    assert wrong is None or wrong in STEREO_WRONG, wrong
    P = collections.Counter()
    N, Nr = len(kL), len(kR)
    uRight = np.full(N, -1.0, F); depth = np.full(N, -1.0, F)
    thOrbDist = (TH_HIGH + TH_LOW) // 2
    nRows = level_sizes[0][1]
    sf = [F(v) for v in scale_factors]; inv_sf = [F(v) for v in inv_scale_factors]
    mbf = F(mbf)
    minZ = F(mb); minD = F(0); maxD = F(mbf / minZ)
    dLi, dRi = as_ints(dL), as_ints(dR)
    xL = [F(v) for v in kL["x"]]; yL = [F(v) for v in kL["y"]]; oL = [int(v) for v in kL["octave"]]
    xR = [F(v) for v in kR["x"]]; oR = [int(v) for v in kR["octave"]]
    rnd = (lambda v: F(np.rint(F(v)))) if wrong == "level_round_half_even" else c_round
    band = []
    for iR in range(Nr):                                          # :886-896
        kpY = F(kR["y"][iR])
        r = F(F(2.0) * sf[oR[iR]])
        hi, lo = F(kpY + r), F(kpY - r)
        if wrong == "band_round":
            maxr, minr = int(c_round(hi)), int(c_round(lo))
        else:
            maxr, minr = math.ceil(float(hi)), math.floor(float(lo))
        if float(hi) == maxr: P["band_hi_integer_l%d" % min(oR[iR], 1)] += 1
        if float(lo) == minr: P["band_lo_integer_l%d" % min(oR[iR], 1)] += 1
        if minr < 0 or maxr >= nRows: P["band_row_outside"] += 1
        band.append((minr, maxr))
    vDistIdx = []
    for iL in range(N):                                           # :907-1031
        levelL, vL, uL = oL[iL], yL[iL], xL[iL]
        row = int(float(vL)) if float(vL) >= 0 else -1            # vRowIndices[vL]: float -> size_t
        if row < 0 or row >= nRows:
            P["row_outside"] += 1
            continue
        minU = F(uL - maxD); maxU = F(uL - minD)
        if maxU < 0:
            continue
        bestDist, bestIdxR = TH_HIGH, 0
        tied = []
        for iR in range(Nr):
            minr, maxr = band[iR]
            octave_ok = (oR[iR] == levelL) if wrong == "octave_strict" else not (oR[iR] < levelL - 1 or oR[iR] > levelL + 1)
            uR = xR[iR]
            u_ok = (uR > minU and uR < maxU) if wrong == "u_strict" else (uR >= minU and uR <= maxU)
            if octave_ok and u_ok:                                # (the probe counts the band's edges only where the band decides)
                P["row_eq_minr"] += row == minr; P["row_eq_maxr"] += row == maxr
                P["row_below_minr"] += row == minr - 1; P["row_above_maxr"] += row == maxr + 1
            in_band = (minr < row < maxr) if wrong == "band_exclusive" else (minr <= row <= maxr)
            if not in_band:
                continue
            if octave_ok and oR[iR] != levelL: P["octave_diff_1"] += 1
            if abs(oR[iR] - levelL) == 2: P["octave_diff_2"] += 1
            if not octave_ok:
                continue
            P["uR_eq_minU"] += int(uR == minU); P["uR_eq_maxU"] += int(uR == maxU)
            if not u_ok:
                continue
            dist = popcount(dLi[iL] ^ dRi[iR])
            if dist < bestDist or (wrong == "desc_tie_last" and dist == bestDist):
                tied = [iR] if dist < bestDist else tied + [iR]
                bestDist, bestIdxR = dist, iR
            elif dist == bestDist and tied:
                tied.append(iR)
        if bestDist in (74, 75, 99, 100): P["best_dist_%d" % bestDist] += 1
        if len(tied) > 1:
            P["desc_tie"] += 1
            P["desc_tie_across_64"] += min(tied) < 64 <= max(tied)
        if not (bestDist <= thOrbDist if wrong == "th_orb_le" else bestDist < thOrbDist):
            continue
        uR0 = xR[bestIdxR]                                        # :958-962
        scaleFactor = inv_sf[levelL]
        scaleduL = rnd(F(uL * scaleFactor)); scaledvL = rnd(F(vL * scaleFactor)); scaleduR0 = rnd(F(uR0 * scaleFactor))
        for v in (F(uL * scaleFactor), F(vL * scaleFactor), F(uR0 * scaleFactor)):
            P["scaled_half"] += float(v) - math.floor(float(v)) == 0.5
        w, L = 5, 5
        cols, rows = level_sizes[levelL]
        iniu = F(F(scaleduR0 + F(L)) - F(w)); endu = F(F(F(scaleduR0 + F(L)) + F(w)) + F(1))
        if iniu < 0 or endu >= cols:                              # :978-981
            P["iniu_endu_rejected"] += 1
            continue
        r0, cL0, cR = int(scaledvL) - w, int(scaleduL) - w, int(scaleduR0)
        if r0 < 0 or r0 + 2 * w + 1 > rows or cL0 < 0 or cL0 + 2 * w + 1 > cols or cR - L - w < 0 or cR + L + w + 1 > cols:
            P["patch_outside"] += 1
            continue
        IL = [[int(v) for v in rw] for rw in levels_left[levelL][r0:r0 + 2 * w + 1, cL0:cL0 + 2 * w + 1]]
        bestD, bestincR = INT_MAX, 0
        vDists = [0] * (2 * L + 1)
        for incR in range(-L, L + 1):                             # :983-999
            c0 = cR + incR - w
            IR = levels_right[levelL][r0:r0 + 2 * w + 1, c0:c0 + 2 * w + 1]
            dist = sum(abs(a - int(b)) for ra, rb in zip(IL, IR) for a, b in zip(ra, rb))      # cv::norm(IL, IR, NORM_L1), exact
            if dist < bestD or (wrong == "sad_tie_last" and dist == bestD):
                bestD, bestincR = dist, incR
            vDists[L + incR] = dist
        P["sad_tie"] += vDists.count(bestD) > 1
        P["best_shift_edge"] += abs(bestincR) == L; P["best_shift_4"] += abs(bestincR) == L - 1
        if abs(bestincR) == L and wrong != "inc_edge_keep":       # :1001-1002
            continue
        dist1 = F(vDists[max(L + bestincR - 1, 0)]); dist2 = F(vDists[L + bestincR]); dist3 = F(vDists[min(L + bestincR + 1, 2 * L)])
        with np.errstate(divide="ignore", invalid="ignore"):
            deltaR = F(F(dist1 - dist3) / F(F(2.0) * F(F(dist1 + dist3) - F(F(2.0) * dist2))))
        if deltaR < -1 or deltaR > 1:                             # :1011 (see the docstring)
            P["delta_rejected"] += 1
            continue
        P["delta_half"] += abs(float(deltaR)) == 0.5
        bestuR = F(sf[levelL] * F(F(scaleduR0 + F(bestincR)) + deltaR))
        disparity = F(uL - bestuR)
        P["disp_negative"] += int(disparity < 0); P["disp_zero"] += int(disparity == 0); P["disp_ge_maxD"] += int(disparity >= maxD)
        P["disp_eq_maxD"] += int(disparity == maxD)
        lo_ok = disparity > minD if wrong == "disp_zero_rejected" else disparity >= minD
        hi_ok = disparity <= maxD if wrong == "disp_le_max" else disparity < maxD
        if lo_ok and hi_ok:                                       # :1019-1029
            if disparity <= 0:
                disparity = F(0.01)                               # disparity = 0.01: the double literal stored in a float
                bestuR = F(uL - F(0.01)) if wrong == "zero_branch_float" else F(float(uL) - 0.01)
                P["zero_branch"] += 1
            depth[iL] = F(mbf / disparity); uRight[iL] = bestuR
            vDistIdx.append((bestD, iL))
    n = len(vDistIdx)
    if n == 0:
        P["nmatch_zero"] += 1
        return uRight, depth, 0, P
    vDistIdx.sort()                                               # :1033-1046
    median = F(vDistIdx[(n - 1) // 2 if wrong == "median_lower" else n // 2][0])
    thDist = F(1.5 * 1.4 * float(median)) if wrong == "th_double" else F(F(F(1.5) * F(1.4)) * median)
    for d, iL in reversed(vDistIdx):
        if (F(d) <= thDist) if wrong == "cut_gt" else (F(d) < thDist):
            break
        uRight[iL] = F(-1); depth[iL] = F(-1)
    P["median"] = int(median); P["thDist"] = float(thDist)
    P["n_eq_median"] = sum(d == int(median) for d, _ in vDistIdx)
    P["n_within_1_of_thDist"] = sum(abs(d - float(thDist)) <= 1 for d, _ in vDistIdx)
    P["n_eq_thDist"] = sum(d == float(thDist) for d, _ in vDistIdx)
    P["kept"] = int((uRight != F(-1)).sum())
    P["zero_branch_kept"] = sum(1 for d, iL in vDistIdx if uRight[iL] != F(-1) and depth[iL] == F(mbf / F(0.01)))
    return uRight, depth, n, P


# ---- BFMatcher::knnMatch(k = 2) and Lowe's test ------------------------------------------------------------------------------------
def hamming_table(q, t):
    """nq x nt Hamming distances as int64: |q| + |t| - 2 (the ones q and t share), the shared ones counted by a float32 product of
    the 0 / 1 bit rows (sums of at most 256 ones: exact)"""
    qb = np.unpackbits(np.asarray(q, np.uint8).reshape(-1, 32), axis=1).astype(F)
    tb = np.unpackbits(np.asarray(t, np.uint8).reshape(-1, 32), axis=1).astype(F)
    return (qb.sum(axis=1)[:, None] + tb.sum(axis=1)[None, :] - F(2) * (qb @ tb.T)).astype(np.int64)


def knn2(q, t, wrong=None, table=None):
    """BFMatcher(NORM_HAMMING)::knnMatch(q, t, 2): per query the two smallest (distance, trainIdx) pairs.  Returns (idx, dist), nq x 2;
    a missing neighbour is KNN_NONE.  table = hamming_table(q, t) if the caller has it."""
    assert wrong is None or wrong in KNN_WRONG, wrong
    nq, nt = len(q), len(t)
    idx = np.full((nq, 2), KNN_NONE[0], np.int64); dist = np.full((nq, 2), KNN_NONE[1], np.int64)
    if nq == 0 or nt == 0:
        return idx, dist
    j = np.arange(nt, dtype=np.int64)
    key = ((hamming_table(q, t) if table is None else table) << 32) | (nt - 1 - j if wrong == "tie_last" else j)[None, :]
    key = np.sort(np.partition(key, min(1, nt - 1), axis=1)[:, :2], axis=1)
    k = key.shape[1]
    lowbits = key & 0xffffffff
    idx[:, :k] = nt - 1 - lowbits if wrong == "tie_last" else lowbits
    dist[:, :k] = key >> 32
    return idx, dist


def lowe(idx2, dist2, monoLeft, monoRight, wrong=None):
    """ComputeStereoFishEyeMatches :1229-1240 over the knnMatch of the lapping rows: per query the right keypoint index
    (trainIdx + monoRight) when `size() >= 2 && [0].distance < [1].distance * 0.7` -- DMatch::distance is a float, 0.7 a double --, else
    -1.  Returns (candidates per query, their number)."""
    assert wrong is None or wrong in LOWE_WRONG, wrong
    out = []
    for (i0, i1), (d0, d1) in zip(np.asarray(idx2).tolist(), np.asarray(dist2).tolist()):
        size = (i0 >= 0) + (i1 >= 0)
        ok = False
        if size >= 2:
            a = float(F(d0))
            b = float(F(F(d1) * F(0.7))) if wrong == "ratio_float" else float(F(d1)) * 0.7
            ok = a <= b if wrong == "ratio_le" else a < b
        out.append(i0 + monoRight if ok else -1)
    return out, sum(c >= 0 for c in out)


# ---- the window matchers' best / second rule ----------------------------------------------------------------------------------------
def window_match(q_desc, t_desc, cand_offsets, cand_idx, wrong=None):
    """ORBmatcher.cc:754-774 over a candidate list, visited in list order: `dist < bestDist` moves the best to the second,
    `else if dist < bestDist2` replaces the second.  The reference keeps the second's distance only; its index follows the same moves.
    Returns (best_idx, best_dist, second_idx, second_dist) per query, -1 / 256 where there is none."""
    assert wrong is None or wrong in WINDOW_WRONG, wrong
    qi, ti = as_ints(q_desc), as_ints(t_desc)
    out = []
    for q in range(len(qi)):
        bd, bi, sd, si = 256, -1, 256, -1
        for k in range(int(cand_offsets[q]), int(cand_offsets[q + 1])):
            c = int(cand_idx[k])
            d = popcount(qi[q] ^ ti[c])
            if d < bd or (wrong == "tie_last" and d == bd):
                sd, si, bd, bi = bd, bi, d, c
            elif d < sd and not (wrong == "second_needs_strict" and d == bd):
                sd, si = d, c
        out.append((bi, bd, si, sd))
    return tuple(np.array([o[k] for o in out], np.int64) for k in range(4))


# ---- MapPoint::ComputeDistinctiveDescriptors ---------------------------------------------------------------------------------------
def distinctive(desc, offsets, wrong=None):
    """src/MapPoint.cc:349-423 per map point (rows offsets[m] .. offsets[m + 1]): every row of the N x N distance table sorted, its
    median read at vDists[0.5 * (N - 1)] (the double product truncated), the first row with the smallest median; -1 for a point
    without rows (the reference returns before it writes)."""
    assert wrong is None or wrong in DISTINCTIVE_WRONG, wrong
    d = as_ints(desc)
    out = []
    for m in range(len(offsets) - 1):
        rows = d[int(offsets[m]):int(offsets[m + 1])]
        N = len(rows)
        if N == 0:
            out.append(-1)
            continue
        best_median, best_idx = INT_MAX, 0
        k = N // 2 if wrong == "median_upper" else int(0.5 * (N - 1))
        for i in range(N):
            v = sorted(0 if i == j else popcount(rows[i] ^ rows[j]) for j in range(N))
            if v[k] < best_median or (wrong == "first_tie_last" and v[k] == best_median):
                best_median, best_idx = v[k], i
        out.append(best_idx)
    return out


# ---- MixedFrame::sortFeaturesResponse -----------------------------------------------------------------------------------------------
def sort_by_response(resp, wrong=None):
    """the permutation of a stable sort by descending response (0.0 and -0.0 compare equal; no NaN)"""
    assert wrong is None or wrong in SORT_WRONG, wrong
    r = [float(v) for v in resp]
    assert not any(math.isnan(v) for v in r)
    order = list(range(len(r)))
    if wrong == "unstable_reverse":
        order.reverse()
    return sorted(order, key=lambda i: -r[i])                    # (sorted is stable; -(-0.0) == 0.0 == -(0.0) as keys)
