"""The descriptor matchers by brute force, written from the reference's text (src/ORBmatcher.cc :44-219, :276-478, :714-831, :833-973,
:1018-1214, :1969-2312, :2314-2355; the type gate of src/MixedMatcher.cpp; src/Frame.cc:710-793), not from oracle/orc_match.c or the
kernels.  Python integers throughout; numpy float32 only where the reference computes in float (the ratio test, the window test, the
stereo gate, the rotation bin, the 10 % rule, the epipole and epipolar tests).

No grid table and no candidate list kept between queries: per query the candidate set is every keypoint of the searched frame that
passes edge_inputs.pos_in_grid, lies in edge_inputs.cell_range_rule, and passes the level gate and |dx| < r and |dy| < r, ordered by
(cell ix, cell iy, index) -- Frame::GetFeaturesInArea's order.  (A keypoint farther than r + 1 px in Python floats is dropped before the
float32 test; for the finite coordinates of tests/match_scenes.py that changes nothing.)

Every model takes `wrong=`: a named wrong variant that changes one comparison (WRONG below).  tests/test_oracle_match_model.py holds the
oracle to the models and shows that the planted scenes tell every variant from the rule; tests/test_gpu_match_model.py holds the kernels."""
import types

import numpy as np

import edge_inputs as ei

TH_LOW, TH_HIGH, HISTO_LENGTH = 50, 100, 30                     # ORBmatcher.cc:36-38
INT_MAX = 2 ** 31 - 1
F = np.float32

WRONG = {
    "th_strict": "< for <= at TH_LOW / TH_HIGH / ORBdist; <= for < in SearchByBoW(KF, KF)",
    "ratio_le": "<= for < in the ratio test (map matcher: >= for >)",
    "ratio_double": "the ratio product computed in float64",
    "second_cut": "a second best of first_dist - 1 or more counts as absent",
    "tie_index": "equal distances resolved by the lowest index",
    "tie_last": "the last of equal distances wins",
    "tri_first": "SearchForTriangulation keeps the first of equal distances",
    "window_le": "|dx| <= r",
    "grid_half_even": "PosInGrid rounds ties to even",
    "level_off": "each level gate one level too wide",
    "state_lt": "vMatchedDistance < dist skips",
    "steal_keep": "the earlier owner keeps its match after a steal",
    "count_slots": "nmatches taken as the number of filled slots",
    "obs_unobserved": "slot value -3 treated as observed",
    "obs_own": "a query's own mp_obs flag ignored: a slot taken in this call is closed",
    "type_gate_off": "the mixed type gate ignored",
    "stereo_ge": "er >= radius rejects",
    "viewcos_float": "viewCos > 0.998f",
    "rot_half_even": "the rotation bin rounds ties to even",
    "rot_no_wrap": "no + 360",
    "maxima_le": "the 10 % rule with <=",
    "maxima_later": "equal bin counts go to the later bin",
    "rot_skip_stolen": "a query whose match was stolen is left out of the histogram",
    "rot_last_push": "projection matchers: a slot written twice is cleared only if its last push lies in a losing bin",
}


def frame(kps, desc, W, H, is_orb=None):
    """what a model reads of a Frame: keypoints, 32-byte descriptors as Python integers, the type flags, the grid bounds of an
    undistorted W x H image (Frame.cc:862-866, :362-363)"""
    gb = types.SimpleNamespace(minX=0.0, minY=0.0, maxX=float(W), maxY=float(H), invW=float(F(64.0) / F(W)), invH=float(F(48.0) / F(H)))
    return types.SimpleNamespace(kps=kps, N=len(kps), desc=as_ints(desc), is_orb=None if is_orb is None else [int(v) for v in is_orb], gb=gb,
                                 x=[float(v) for v in kps["x"]], y=[float(v) for v in kps["y"]])


def as_ints(desc):
    return [int.from_bytes(bytes(bytearray(np.asarray(d, np.uint8)[:32])), "little") for d in desc]


def hamming(a, b):
    return bin(a ^ b).count("1")


def level_of(fr, i):
    """Frame::getKPtLevelMono: the octave of an ORB keypoint, class_id of the other type (MixedFrame.cpp:438-446)"""
    return int(fr.kps["octave"][i]) if fr.is_orb is None or fr.is_orb[i] else int(fr.kps["class_id"][i])


def is_orb(flags, i):
    return True if flags is None else bool(flags[i])


# ---------------------------------------------------------------------------------------------------
def three_maxima(sizes, wrong=None):
    """ORBmatcher::ComputeThreeMaxima :2314-2355"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    gt = (lambda a, b: a >= b and a > 0) if wrong == "maxima_later" else (lambda a, b: a > b)
    for i, s in enumerate(sizes):
        s = int(s)
        if gt(s, max1):
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif gt(s, max2):
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif gt(s, max3):
            max3, ind3 = s, i
    lt = (lambda a, b: a <= b) if wrong == "maxima_le" else (lambda a, b: a < b)
    lim = F(0.1) * F(max1)
    if lt(F(max2), lim):
        ind2 = ind3 = -1
    elif lt(F(max3), lim):
        ind3 = -1
    return ind1, ind2, ind3


def rot_bin(a1, a2, wrong=None):
    """rot = a1 - a2; if(rot<0.0) rot+=360.0f; bin = round(rot*factor) (e.g. :786-791): float32, C round (halves away from zero)"""
    rot = F(a1) - F(a2)
    if rot < 0.0 and wrong != "rot_no_wrap":
        rot = F(rot + F(360.0))
    v = float(F(rot * (F(1.0) / F(HISTO_LENGTH))))
    b = ei.round_index(v, "half_even" if wrong == "rot_half_even" else None)
    return 0 if b == HISTO_LENGTH else b


class _Hist:
    """the rotation histogram: bins of (key, order of the push)"""

    def __init__(self, on, wrong):
        self.on, self.wrong, self.bins, self.n = on, wrong, {}, 0

    def push(self, a1, a2, key):
        if self.on:
            self.bins.setdefault(rot_bin(a1, a2, self.wrong), []).append((key, self.n))
            self.n += 1

    def losers(self):
        """the entries of every bin outside the three maxima, bin by bin"""
        sizes = [len(self.bins.get(i, ())) for i in range(HISTO_LENGTH)]
        keep = three_maxima(sizes, self.wrong)
        return [e for i in range(HISTO_LENGTH) if i not in keep for e in self.bins.get(i, ())]


# ---------------------------------------------------------------------------------------------------
def candidates(fr, x, y, r, min_level, max_level, wrong=None, levels=None):
    """Frame::GetFeaturesInArea :710-781 by brute force, in its order.  levels: what getKPtLevelMono(vCell[j]) (:763) gives for the
    keypoints of this grid where that is not the keypoint's own level (the right grid of a two-camera frame, tests/twocam_model.py)"""
    x, y, r = F(x), F(y), F(r)
    cr = ei.cell_range_rule(x, y, r, fr.gb)
    if cr is None:
        return []
    if wrong == "level_off":
        min_level -= 1
        max_level = max_level + 1 if max_level >= 0 else max_level
    check = min_level > 0 or max_level >= 0
    inside = (lambda d: abs(d) <= r) if wrong == "window_le" else (lambda d: abs(d) < r)
    out = []
    fx, fy, fr_ = float(x), float(y), float(r) + 1.0
    for i in range(fr.N):
        if abs(fr.x[i] - fx) > fr_ or abs(fr.y[i] - fy) > fr_:
            continue
        c = ei.pos_in_grid(fr.x[i], fr.y[i], fr.gb, "half_even" if wrong == "grid_half_even" else None)
        if c is None or not (cr[0] <= c[0] <= cr[1] and cr[2] <= c[1] <= cr[3]):
            continue
        if check:
            lv = level_of(fr, i) if levels is None else levels[i]
            if lv < min_level or (max_level >= 0 and lv > max_level):
                continue
        if inside(F(fr.kps["x"][i]) - x) and inside(F(fr.kps["y"][i]) - y):
            out.append((c[0], c[1], i))
    return [i for _, _, i in sorted(out)]


def _scan(dists, wrong, absent):
    """best / second best over (distance, index) in candidate order: the `if(dist<bestDist) ... else if(dist<bestDist2)` of every
    matcher -> (best, best index, position of the best, second, position of the second)"""
    best, idx, pos, second, pos2 = absent, -1, -1, absent, -1
    if wrong == "tie_index":
        dists = sorted(enumerate(dists), key=lambda e: (e[1][0], e[1][1]))
        dists = [(d, i, p) for p, (d, i) in dists]
    else:
        dists = [(d, i, p) for p, (d, i) in enumerate(dists)]
    for d, i, p in dists:
        if d < best or (wrong == "tie_last" and d == best and idx >= 0):
            second, pos2 = best, pos
            best, idx, pos = d, i, p
        elif d < second:
            second, pos2 = d, p
    return best, idx, pos, second, pos2


def first_dist(th, ratio, map_form=False):
    """the least second-best distance above th that lets every best <= th pass the ratio test: candidates at this distance or beyond
    cannot change a decision (the pruning bound of the window kernels; `second_cut` is that bound off by one)"""
    r = F(ratio)
    for d in range(th + 1, 257):
        if (not (F(th) > r * F(d))) if map_form else (F(th) < F(d) * r):
            return d
    return 257


def _ratio_ok(best, second, ratio, wrong, map_form=False):
    """(float)bestDist < (float)bestDist2 * mfNNratio, or the map matcher's !(bestDist > mfNNratio * bestDist2)"""
    if wrong == "ratio_double":
        prod = float(F(ratio)) * float(second)
        b = float(best)
    else:
        prod = F(second) * F(ratio)
        b = F(best)
    if map_form:
        return not (b >= prod if wrong == "ratio_le" else b > prod)
    return b <= prod if wrong == "ratio_le" else b < prod


# ---------------------------------------------------------------------------------------------------
def search_for_initialization(F1, F2, prev_matched, window, ratio, check_ori=True, wrong=None, info=None):
    """ORBmatcher::SearchForInitialization :714-831 with MixedMatcher.cpp:47-63's type gate -> (nmatches, vnMatches12, vbPrevMatched)"""
    n = 0
    m12 = [-1] * F1.N
    matched_dist = [INT_MAX] * F2.N
    m21 = [-1] * F2.N
    hist = _Hist(check_ori, wrong)
    stolen = set()
    D = first_dist(TH_LOW, ratio)
    for i1 in range(F1.N):
        level1 = level_of(F1, i1)
        if level1 > 0:
            continue
        cand = candidates(F2, prev_matched[i1][0], prev_matched[i1][1], float(window), level1, level1, wrong)
        if not cand:
            continue
        ds = []
        for i2 in cand:
            if wrong != "type_gate_off" and is_orb(F1.is_orb, i1) != is_orb(F2.is_orb, i2):
                continue
            d = hamming(F1.desc[i1], F2.desc[i2])
            if (matched_dist[i2] < d) if wrong == "state_lt" else (matched_dist[i2] <= d):
                continue
            ds.append((d, i2))
        best, idx, _, second, _ = _scan(ds, wrong, INT_MAX)
        if wrong == "second_cut" and second >= D - 1:
            second = INT_MAX
        if info is not None:
            info.setdefault("best", []).append((i1, best, second))
        if (best < TH_LOW) if wrong == "th_strict" else (best <= TH_LOW):
            if _ratio_ok(best, second, ratio, wrong):
                if m21[idx] >= 0 and wrong != "steal_keep":
                    m12[m21[idx]] = -1
                    stolen.add(m21[idx])
                    n -= 1
                m12[i1] = idx
                m21[idx] = i1
                matched_dist[idx] = best
                n += 1
                hist.push(F1.kps["angle"][i1], F2.kps["angle"][idx], i1)
                if info is not None:
                    info.setdefault("pushes", []).append((i1, idx))
    if check_ori:
        if wrong == "rot_skip_stolen":
            for b in hist.bins:
                hist.bins[b] = [e for e in hist.bins[b] if e[0] not in stolen]
        for i1, _ in hist.losers():
            if m12[i1] >= 0:
                m12[i1] = -1
                n -= 1
    pm = np.array(prev_matched, np.float32).copy()
    for i1 in range(F1.N):
        if m12[i1] >= 0:
            pm[i1, 0] = F2.kps["x"][m12[i1]]
            pm[i1, 1] = F2.kps["y"][m12[i1]]
    if wrong == "count_slots":
        n = sum(1 for v in m12 if v >= 0)
    return n, np.array(m12, np.int32), pm


def holds_observed(slot, obs, wrong=None):
    """`if(F.getMapPoint(idx)) if(F.getMapPoint(idx)->Observations()>0) continue;` (:91-93, :2045-2047) on the slot encoding of the
    calls: -1 no map point, -2 one of another call that is observed, -3 one that is not, k >= 0 query k of this call"""
    if slot == -1:
        return False
    if slot == -3:
        return wrong == "obs_unobserved"
    if slot == -2:
        return True
    return True if wrong == "obs_own" else bool(obs[slot])


def _stereo_rejects(ur, uright, radius, wrong):
    """`if(mvuRight[i2]>0) { er = fabs(ur - mvuRight[i2]); if(er>radius) continue; }` (:95-100, :2049-2055)"""
    if not F(uright) > 0:
        return False
    er = abs(F(ur) - F(uright))
    return er >= radius if wrong == "stereo_ge" else er > radius


def _clear_losers(hist, slots, n, wrong):
    """`setMapPoint(rotHist[i][j], NULL); nmatches--;` for every entry of a losing bin (:2173-2183, :2298-2308)"""
    last = {}
    for b in hist.bins.values():
        for key, order in b:
            last[key] = max(order, last.get(key, -1))
    for key, order in hist.losers():
        if wrong == "rot_last_push" and order != last[key]:
            continue
        slots[key] = -1
        n -= 1
    return n


def search_by_projection_last(cur, last, valid, uv, mp_desc, mp_obs, cur_mp, th, level_scale, mode=0, check_ori=True, uright=None,
                              proj_ur=None, wrong=None, info=None):
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono) :1969-2187 after the projection (valid, uv); mode 0 / 1 / 2: neither,
    bForward, bBackward; MixedMatcher.cpp:723-790's type gate.  -> (nmatches, the current frame's slots)"""
    return _best_only(cur, last.kps, last.is_orb, [level_of(last, i) for i in range(last.N)], valid, uv, mp_desc, mp_obs, cur_mp, th,
                      level_scale, mode, TH_HIGH, check_ori, uright, proj_ur, wrong, info)


def search_by_projection_kf(cur, kf_kps, kf_is_orb, valid, uv, pred_level, level_scale, mp_desc, cur_mp, th, orb_dist, check_ori=True,
                            wrong=None, info=None):
    """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) :2189-2312 after the projection; MixedMatcher.cpp:990-1005"""
    return _best_only(cur, kf_kps, kf_is_orb, [int(v) for v in pred_level], valid, uv, mp_desc, None, cur_mp, th, level_scale, 3, orb_dist,
                      check_ori, None, None, wrong, info)


def _best_only(cur, q_kps, q_is_orb, q_level, valid, uv, mp_desc, mp_obs, cur_mp, th, level_scale, mode, dist_th, check_ori, uright, proj_ur,
               wrong, info):
    n = 0
    slots = [int(v) for v in cur_mp]
    qd = as_ints(mp_desc)
    hist = _Hist(check_ori, wrong)
    for i in range(len(q_kps)):
        if not valid[i]:
            continue
        L = q_level[i]
        radius = F(th) * F(level_scale[i])
        lo, hi = {0: (L - 1, L + 1), 1: (L, -1), 2: (0, L), 3: (L - 1, L + 1)}[mode]
        cand = candidates(cur, uv[i][0], uv[i][1], radius, lo, hi, wrong)
        if not cand:
            continue
        ds = []
        for i2 in cand:
            if mode == 3:
                if slots[i2] != -1:                                          # `if(CurrentFrame.getMapPoint(i2)) continue;` :2254
                    continue
            elif holds_observed(slots[i2], mp_obs, wrong):
                continue
            if uright is not None and _stereo_rejects(proj_ur[i], uright[i2], radius, wrong):
                continue
            if wrong != "type_gate_off" and is_orb(q_is_orb, i) != is_orb(cur.is_orb, i2):
                continue
            ds.append((hamming(qd[i], cur.desc[i2]), i2))
        best, idx, _, _, _ = _scan(ds, wrong, 256)
        if info is not None:
            info.setdefault("best", []).append((i, best, None))
        if (best < dist_th) if wrong == "th_strict" else (best <= dist_th):
            slots[idx] = i
            n += 1
            hist.push(q_kps["angle"][i], cur.kps["angle"][idx], idx)
            if info is not None:
                info.setdefault("pushes", []).append((i, idx))
    if check_ori:
        n = _clear_losers(hist, slots, n, wrong)
    if wrong == "count_slots":
        n = sum(1 for v in slots if v >= 0)
    return n, np.array(slots, np.int32)


def radius_by_viewing_cos(view_cos, wrong=None):
    """ORBmatcher::RadiusByViewingCos :221-227: `viewCos>0.998`, a float against a double constant"""
    if wrong == "viewcos_float":
        return F(2.5) if F(view_cos) > F(0.998) else F(4.0)
    return F(2.5) if float(F(view_cos)) > 0.998 else F(4.0)


def search_by_projection_map(Fr, in_view, proj_xy, level, view_cos, mp_desc, mp_obs, frame_mp, th, ratio, level_scale, mp_is_orb=None,
                             uright=None, proj_xr=None, wrong=None, info=None):
    """SearchByProjection(F, vpMapPoints, th) :44-147 (the mbTrackInView branch of a frame without a second camera) after isInFrustum;
    MixedMatcher.cpp:539-567's type gate.  -> (nmatches, the frame's slots)"""
    n = 0
    slots = [int(v) for v in frame_mp]
    qd = as_ints(mp_desc)
    D = min(256, first_dist(TH_HIGH, ratio, True))
    for m in range(len(in_view)):
        if not in_view[m]:
            continue
        L = int(level[m])
        r = radius_by_viewing_cos(view_cos[m], wrong)
        if float(th) != 1.0:
            r = F(r * F(th))
        rs = F(r * F(level_scale[m]))
        cand = candidates(Fr, proj_xy[m][0], proj_xy[m][1], rs, L - 1, L, wrong)
        if not cand:
            continue
        ds = []
        for idx in cand:
            if holds_observed(slots[idx], mp_obs, wrong):
                continue
            if uright is not None and _stereo_rejects(proj_xr[m], uright[idx], rs, wrong):
                continue
            if wrong != "type_gate_off" and is_orb(mp_is_orb, m) != is_orb(Fr.is_orb, idx):
                continue
            ds.append((hamming(qd[m], Fr.desc[idx]), idx))
        best, idx, _, second, pos2 = _scan(ds, wrong, 256)
        lvl = level_of(Fr, idx) if idx >= 0 else -1
        lvl2 = -1
        if pos2 >= 0:
            lvl2 = level_of(Fr, ds[pos2][1])
        if wrong == "second_cut" and second >= D - 1:
            second, lvl2 = 256, -1
        if info is not None:
            info.setdefault("best", []).append((m, best, second if lvl == lvl2 else None))
        if (best < TH_HIGH) if wrong == "th_strict" else (best <= TH_HIGH):
            if lvl == lvl2 and not _ratio_ok(best, second, ratio, wrong, True):
                continue
            slots[idx] = m
            n += 1
    if wrong == "count_slots":
        n = sum(1 for v in slots if v >= 0)
    return n, np.array(slots, np.int32)


# ---------------------------------------------------------------------------------------------------
# the node walk
def _common_nodes(fv1, fv2):
    """the feature lists of the nodes both vectors hold, ascending: what the lower_bound walk (:297-455) visits"""
    n1 = {int(k): [int(v) for v in fv1[2][fv1[1][j]:fv1[1][j + 1]]] for j, k in enumerate(fv1[0])}
    n2 = {int(k): [int(v) for v in fv2[2][fv2[1][j]:fv2[1][j + 1]]] for j, k in enumerate(fv2[0])}
    return [(n1[k], n2[k]) for k in sorted(n1) if k in n2]


def search_by_bow(kf_kps, kf_desc, kf_has_mp, kf_fv, f_kps, f_desc, f_fv, ratio, check_ori=True, wrong=None, info=None):
    """SearchByBoW(pKF, F, vpMapPointMatches) :276-478, a frame without a second camera -> (nmatches, the KF index per frame feature)"""
    n = 0
    match_f = [-1] * len(f_kps)
    d1, d2 = as_ints(kf_desc), as_ints(f_desc)
    hist = _Hist(check_ori, wrong)
    D = first_dist(TH_LOW, ratio)
    for l1, l2 in _common_nodes(kf_fv, f_fv):
        for ikf in l1:
            if not kf_has_mp[ikf]:
                continue
            ds = [(hamming(d1[ikf], d2[i]), i) for i in l2 if match_f[i] < 0]
            best, idx, _, second, _ = _scan(ds, wrong, 256)
            if wrong == "second_cut" and second >= D - 1:
                second = 256
            if info is not None:
                info.setdefault("best", []).append((ikf, best, second))
            if (best < TH_LOW) if wrong == "th_strict" else (best <= TH_LOW):
                if _ratio_ok(best, second, ratio, wrong):
                    match_f[idx] = ikf
                    hist.push(kf_kps["angle"][ikf], f_kps["angle"][idx], idx)
                    if info is not None:
                        info.setdefault("pushes", []).append((ikf, idx))
                    n += 1
    if check_ori:
        for idx, _ in hist.losers():
            match_f[idx] = -1
            n -= 1
    if wrong == "count_slots":
        n = sum(1 for v in match_f if v >= 0)
    return n, np.array(match_f, np.int32)


def search_by_bow_kf(kps1, desc1, has_mp1, fv1, kps2, desc2, has_mp2, fv2, ratio, check_ori=True, wrong=None, info=None):
    """SearchByBoW(pKF1, pKF2, vpMatches12) :833-973 -> (nmatches, the index in KF2 per keypoint of KF1)"""
    n = 0
    m12 = [-1] * len(kps1)
    matched2 = [False] * len(kps2)
    d1, d2 = as_ints(desc1), as_ints(desc2)
    hist = _Hist(check_ori, wrong)
    D = first_dist(TH_LOW - 1, ratio)                                        # (the best is at most TH_LOW - 1 here)
    for l1, l2 in _common_nodes(fv1, fv2):
        for i1 in l1:
            if not has_mp1[i1]:
                continue
            ds = [(hamming(d1[i1], d2[i]), i) for i in l2 if not matched2[i] and has_mp2[i]]
            best, idx, _, second, _ = _scan(ds, wrong, 256)
            if wrong == "second_cut" and second >= D - 1:
                second = 256
            if info is not None:
                info.setdefault("best", []).append((i1, best, second))
            if (best <= TH_LOW) if wrong == "th_strict" else (best < TH_LOW):
                if _ratio_ok(best, second, ratio, wrong):
                    m12[i1] = idx
                    matched2[idx] = True
                    hist.push(kps1["angle"][i1], kps2["angle"][idx], i1)
                    if info is not None:
                        info.setdefault("pushes", []).append((i1, idx))
                    n += 1
    if check_ori:
        for i1, _ in hist.losers():
            m12[i1] = -1
            n -= 1
    if wrong == "count_slots":
        n = sum(1 for v in m12 if v >= 0)
    return n, np.array(m12, np.int32)


def epipolar_ok(kp1, kp2, F12, unc):
    """Pinhole::epipolarConstrain (src/CameraModels/Pinhole.cpp:142-156) with F12 given, float32 left to right"""
    x1, y1, x2, y2 = F(kp1["x"]), F(kp1["y"]), F(kp2["x"]), F(kp2["y"])
    f = np.asarray(F12, np.float32).reshape(3, 3)
    a = x1 * f[0, 0] + y1 * f[1, 0] + f[2, 0]
    b = x1 * f[0, 1] + y1 * f[1, 1] + f[2, 1]
    c = x1 * f[0, 2] + y1 * f[1, 2] + f[2, 2]
    num = a * x2 + b * y2 + c
    den = a * a + b * b
    if den == 0:
        return False
    return bool(num * num / den < F(3.84) * F(unc))


def search_for_triangulation(kps1, desc1, elig1, fv1, kps2, desc2, elig2, fv2, ep, F12, scale2, sigma2_2, coarse=False, check_ori=True,
                             wrong=None, info=None):
    """SearchForTriangulation :1018-1214 with bOnlyStereo false and pinhole cameras.  elig bit 0: no map point yet, bit 1: a stereo
    observation (mvuRight >= 0).  scale2: KF2's scale factor per octave (the `100*getORBScaleFactor(octave)` of :1101).
    -> (nmatches, the index in KF2 per keypoint of KF1)"""
    n = 0
    m12 = [-1] * len(kps1)
    d1, d2 = as_ints(desc1), as_ints(desc2)
    hist = _Hist(check_ori, wrong)
    for l1, l2 in _common_nodes(fv1, fv2):
        for i1 in l1:
            if not int(elig1[i1]) & 1:
                continue
            best, idx = TH_LOW, -1
            for i2 in l2:
                if not int(elig2[i2]) & 1:
                    continue
                d = hamming(d1[i1], d2[i2])
                if wrong == "th_strict" and d >= TH_LOW:
                    continue
                if d > TH_LOW or d > best or (wrong == "tri_first" and d == best and idx >= 0):
                    continue
                if not (int(elig1[i1]) | int(elig2[i2])) & 2:
                    ex, ey = F(ep[0]) - F(kps2["x"][i2]), F(ep[1]) - F(kps2["y"][i2])
                    if ex * ex + ey * ey < F(100) * F(scale2[int(kps2["octave"][i2])]):
                        continue
                if coarse or epipolar_ok(kps1[i1], kps2[i2], F12, sigma2_2[int(kps2["octave"][i2])]):
                    idx, best = i2, d
            if idx >= 0:
                m12[i1] = idx
                n += 1
                hist.push(kps1["angle"][i1], kps2["angle"][idx], i1)
                if info is not None:
                    info.setdefault("pushes", []).append((i1, idx))
    if check_ori:
        for i1, _ in hist.losers():
            m12[i1] = -1
            n -= 1
    if wrong == "count_slots":
        n = sum(1 for v in m12 if v >= 0)
    return n, np.array(m12, np.int32)
