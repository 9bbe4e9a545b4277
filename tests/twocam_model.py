"""The three matchers of a two-camera (fisheye stereo) frame by brute force, written from the reference's text: the
`numKPtsLeft() != -1` branches of src/ORBmatcher.cc:44-219, :276-478 and :1969-2187, and Frame::GetFeaturesInArea with bRight
(src/Frame.cc:710-781) -- not from oracle/orc_twocam.c or the kernels.  The conventions are those of tests/match_model.py: Python
integers, numpy float32 one operation at a time where the reference computes in float, candidate sets over all keypoints in the order
(cell ix, cell iy, index), `wrong=` for a named wrong variant, `info=` for a probe.

A frame is the nL left keypoints followed by the nR right ones; slots, links and matches use that global index (right keypoint j is
nL + j), l2r[left] is a right-local index and r2l[right-local] a left one, -1 for none.

The level gate of the right grid (gate_levels): GetFeaturesInArea reads `getKPtLevelMono(vCell[j])` (Frame.cc:763) with the
right-local index j of mGridRight, and getKPtLevelMono(j) is mvKeysUn[j].octave (:1417-1420), the LEFT keypoint j.  So the gate of
right keypoint j reads the octave of left keypoint j.  For j >= nL the reference reads past mvKeysUn; the project reads the right
keypoint's own octave there (upstream ORB-SLAM3's rule), and that is a convention, not the reference's text.  bestLevel / bestLevel2
of a right candidate are its own octave (`getKPtRight(idx).octave`, :188, :193).

info["probe"] counts how often the input reached a comparison (PROBES names them)."""
import collections
import types

import numpy as np

import match_model as mm
from match_model import F, TH_HIGH, TH_LOW

WRONG = dict(mm.WRONG)
WRONG.update({
    "right_uses_th": "the map form's right radius is multiplied by th",
    "right_after_left_reject": "the map form's right search still runs after the left ratio rejection",
    "right_gate_own_octave": "the right grid's level gate reads the right keypoint's own octave",
    "best_level_from_gate": "bestLevel / bestLevel2 of a right candidate are taken from the gate's table",
    "partner_not_claimed": "the l2r / r2l partner slot is not written",
    "partner_not_counted": "the partner slot is written but nmatches grows by one",
    "partner_open": "a slot claimed through a link does not close for later queries of the other camera",
    "last_right_without_left_window": "the last-frame form's right search runs although the left window was empty",
    "last_empty_after_slots": "the last-frame form decides `empty` after the Observations() > 0 skip",
    "last_right_forward_capped": "forward mode's right gate gets the upper level L + 1",
    "rot_right_local_index": "the histogram records j for a right match, so slot j is cleared",
    "bow_sides_merged": "one best / second pair over both sides of a node",
    "bow_right_ratio": "the right side's ratio test is applied",
    "bow_right_ungated": "the right best is taken although bestDist1 > TH_LOW",
    "bow_right_needs_left_ratio": "the right best is taken only if the left match was made",
    "bow_right_first": "the right commit comes before the left",
})

PROBES = {
    "L best == TH": "a left sub-query whose best distance is the threshold", "L best == TH + 1": "... the threshold + 1",
    "R best == TH": "a right sub-query whose best distance is the threshold", "R best == TH + 1": "... the threshold + 1",
    "L ratio equal": "left, same level: (float)best == nnratio * second exactly", "R ratio equal": "the same on the right",
    "L second on another level": "left: best <= TH and bestLevel != bestLevel2 with a second present",
    "R second on another level": "the same on the right",
    "R gate != own, kept": "a right candidate whose gate octave passes and whose own octave would not",
    "R gate != own, dropped": "a right candidate whose gate octave fails and whose own octave would pass",
    "R levels differ by table": "a right sub-query whose bestLevel == bestLevel2 decision differs between the two tables",
    "left rejected, right would match": "the left ratio rejection skipped a right search that had a match",
    "right only inside th x radius": "a right candidate outside the radius and inside th times the radius",
    "tie": "a sub-query with two candidates at the best distance", "tie across cells": "... in different cells",
    "tie across a 64 stride": "... in one cell, 64 or more places apart", "tie across 64 cells": "... 64 or more cells apart in the window",
    "window cells > 64": "a sub-query over more than 64 cells", "cell > 64": "a sub-query that visits a cell of more than 64 keypoints",
    "partner claimed": "a match that wrote its partner slot", "no partner": "a match without a link",
    "closed through a link": "a candidate skipped because a partner write closed it", "reopened through a link": "a candidate met again in a slot that a partner write of an unobserved query took",
    "slot -2": "a candidate skipped for slot value -2", "slot -3": "a candidate met in a slot of value -3",
    "left window empty, right matches": "the empty left window skipped a right search that had a match",
    "left window all closed": "a left window whose candidates were all closed, the right search run",
    "right projection outside": "a right projection whose cell range is empty", "right level one outside": "a right keypoint in the window one level outside the gate",
    "slot written twice": "a match into a slot that this call had written",
    "bow left == TH, right <= TH": "", "bow left == TH, right > TH": "", "bow left == TH + 1, right <= TH": "", "bow left == TH + 1, right > TH": "",
    "bow left ratio fails, right taken": "", "bow right ratio would fail": "", "bow tie across sides": "best1 == best1R",
    "bow both sides": "a KeyFrame feature that matched on both sides", "bow node > 64": "a node of more than 64 frame features",
    "bow competed": "a KeyFrame feature that met a frame feature already taken",
}


def twocam_frame(kps, desc, nL, W, H):
    """both cameras' keypoints of a frame as two match_model.frame views plus the right grid's gate table"""
    kps = np.asarray(kps)
    nL = int(nL)
    d = np.asarray(desc, np.uint8).reshape(len(kps), -1)
    return types.SimpleNamespace(nL=nL, nR=len(kps) - nL, cam=(mm.frame(kps[:nL], d[:nL], W, H), mm.frame(kps[nL:], d[nL:], W, H)),
                                 gate=gate_levels(kps, nL), own=[int(v) for v in kps["octave"][nL:]], kps=kps)


def gate_levels(kps, nL):
    """what the level gate reads for every right keypoint (Frame.cc:763 with :1417-1420; see the module text)"""
    nR = len(kps) - nL
    return [int(kps["octave"][j]) if j < nL else int(kps["octave"][nL + j]) for j in range(nR)]


def _count(info, key, n=1):
    if info is not None and n:
        info.setdefault("probe", collections.Counter())[key] += int(n)


def _cells(fr, idxs):
    return [mm.ei.pos_in_grid(fr.x[i], fr.y[i], fr.gb, None) for i in idxs]


def _window_probe(Fr, cam, x, y, r, cand, dists, info):
    """the size facts of a sub-query's window: more than 64 cells, a cell of more than 64 keypoints, ties and where they lie"""
    if info is None:
        return
    fr = Fr.cam[cam]
    cr = mm.ei.cell_range_rule(F(x), F(y), F(r), fr.gb)
    if cr is None:
        return
    ncy = cr[3] - cr[2] + 1
    _count(info, "window cells > 64", (cr[1] - cr[0] + 1) * ncy > 64)
    cells = _cells(fr, cand)
    per = collections.Counter(cells)
    _count(info, "cell > 64", any(v > 64 for v in per.values()))
    if dists:
        best = min(d for d, _ in dists)
        at = [cand.index(i) for d, i in dists if d == best]
        if len(at) > 1:
            _count(info, "tie")
            cs = [cells[p] for p in at]
            _count(info, "tie across cells", len(set(cs)) > 1)
            order = lambda c: (c[0] - cr[0]) * ncy + (c[1] - cr[2])
            _count(info, "tie across 64 cells", max(order(c) for c in cs) - min(order(c) for c in cs) >= 64)
            for c in set(cs):
                inside = [k for k, cc in enumerate(cells) if cc == c]
                pl = [inside.index(p) for p in at if cells[p] == c]
                _count(info, "tie across a 64 stride", len(pl) > 1 and max(pl) - min(pl) >= 64)


def _open(slot, gi, mp_obs, via_link, wrong, info):
    """the Observations() > 0 skip on one candidate -> True when the candidate is met"""
    if wrong == "partner_open" and gi in via_link:
        return True
    held = mm.holds_observed(slot, mp_obs, wrong)
    if info is not None:
        _count(info, "slot -2", slot == -2)
        _count(info, "slot -3", slot == -3)
        if gi in via_link:
            _count(info, "closed through a link" if held else "reopened through a link")
    return not held


def _right_candidates(Fr, x, y, r, lo, hi, wrong, info):
    fr = Fr.cam[1]
    levels = Fr.own if wrong == "right_gate_own_octave" else Fr.gate
    cand = mm.candidates(fr, x, y, r, lo, hi, wrong, levels=levels)
    if info is not None and Fr.gate != Fr.own:
        other = mm.candidates(fr, x, y, r, lo, hi, wrong, levels=Fr.own)
        _count(info, "R gate != own, kept", len(set(cand) - set(other)))
        _count(info, "R gate != own, dropped", len(set(other) - set(cand)))
    if info is not None:
        wide = mm.candidates(fr, x, y, r, lo - 1, hi + 1 if hi >= 0 else hi, wrong, levels=levels)
        _count(info, "right level one outside", len(set(wide) - set(cand)))
        _count(info, "right projection outside", mm.ei.cell_range_rule(F(x), F(y), F(r), fr.gb) is None)
    return cand


# ---------------------------------------------------------------------------------------------------
def _map_sub(Fr, cam, x, y, rs, L, qd, m, slots, mp_obs, ratio, via_link, wrong, info, probe_only=False):
    """one camera's block of SearchByProjection(F, map points): the window, best / second with their levels, the threshold and the
    ratio rule -> ("none" | "far" | "rejected" | "match", global index of the best)"""
    side = "LR"[cam]
    fr, base = Fr.cam[cam], cam * Fr.nL
    info = None if probe_only else info
    cand = mm.candidates(fr, x, y, rs, L - 1, L, wrong) if cam == 0 else _right_candidates(Fr, x, y, rs, L - 1, L, wrong, info)
    if not cand:
        return "none", -1
    ds = [(mm.hamming(qd, fr.desc[i]), i) for i in cand if _open(slots[base + i], base + i, mp_obs, via_link, wrong, info)]
    _window_probe(Fr, cam, x, y, rs, cand, ds, info)
    best, idx, _, second, pos2 = mm._scan(ds, wrong, 256)
    table = (lambda i: int(fr.kps["octave"][i])) if cam == 0 or wrong != "best_level_from_gate" else (lambda i: Fr.gate[i])
    lvl = table(idx) if idx >= 0 else -1
    lvl2 = table(ds[pos2][1]) if pos2 >= 0 else -1
    if wrong == "second_cut" and second >= min(256, mm.first_dist(TH_HIGH, ratio, True)) - 1:
        second, lvl2 = 256, -1
    if info is not None:
        info.setdefault("best", []).append((m, cam, best, second if lvl == lvl2 else None))
        _count(info, side + " best == TH", best == TH_HIGH)
        _count(info, side + " best == TH + 1", best == TH_HIGH + 1)
        if best <= TH_HIGH and pos2 >= 0:
            _count(info, side + " second on another level", lvl != lvl2)
            _count(info, side + " ratio equal", lvl == lvl2 and bool(F(best) == F(second) * F(ratio)))
            if cam == 1:
                o2, g2 = Fr.own[ds[pos2][1]], Fr.gate[ds[pos2][1]]
                _count(info, "R levels differ by table", (Fr.own[idx] == o2) != (Fr.gate[idx] == g2))
    if not ((best < TH_HIGH) if wrong == "th_strict" else (best <= TH_HIGH)):
        return "far", -1
    if lvl == lvl2 and not mm._ratio_ok(best, second, ratio, wrong, True):
        return "rejected", -1
    return "match", base + idx


def search_by_projection_map_twocam(Fr, l2r, r2l, left, right, mp_desc, mp_obs, frame_mp, th, ratio, wrong=None, info=None):
    """SearchByProjection(F, vpMapPoints, th) :44-219 on a two-camera frame, after isInFrustum.  left / right: per camera (in_view,
    proj_xy, level, view_cos, level_scale) of every map point, as the calls take them.  -> (nmatches, the frame's slots)"""
    n = 0
    slots = [int(v) for v in frame_mp]
    qd = mm.as_ints(mp_desc)
    via_link = set()
    nL = Fr.nL

    def claim(gi, m, partner):
        nonlocal n
        if info is not None:
            _count(info, "slot written twice", slots[gi] >= 0)
        if partner and wrong == "partner_not_claimed":
            return
        slots[gi] = m
        if partner:
            via_link.add(gi)
            n += 0 if wrong == "partner_not_counted" else 1
        else:
            via_link.discard(gi)
            n += 1
    for m in range(len(mp_obs)):
        ivl, ivr = bool(left[0][m]), bool(right[0][m])
        if not ivl and not ivr:                                              # :54
            continue
        if ivl:
            L = int(left[2][m])
            r = mm.radius_by_viewing_cos(left[3][m], wrong)
            if float(th) != 1.0:                                             # bFactor :49, :70-71
                r = F(r * F(th))
            rs = F(r * F(left[4][m]))
            what, gi = _map_sub(Fr, 0, left[1][m][0], left[1][m][1], rs, L, qd[m], m, slots, mp_obs, ratio, via_link, wrong, info)
            if what == "rejected":                                           # `continue` :130-131 leaves the map point
                if info is not None and ivr and int(right[2][m]) != -1:
                    rr = F(mm.radius_by_viewing_cos(right[3][m], wrong) * F(right[4][m]))
                    w2, _ = _map_sub(Fr, 1, right[1][m][0], right[1][m][1], rr, int(right[2][m]), qd[m], m, slots, mp_obs, ratio, via_link,
                                     wrong, info, probe_only=True)
                    _count(info, "left rejected, right would match", w2 == "match")
                if wrong != "right_after_left_reject":
                    continue
            elif what == "match":
                claim(gi, m, False)
                if l2r[gi] != -1:                                            # :136-140
                    claim(nL + int(l2r[gi]), m, True)
                    _count(info, "partner claimed")
                else:
                    _count(info, "no partner")
        if ivr:
            L = int(right[2][m])
            if L == -1:                                                      # :151
                continue
            r = mm.radius_by_viewing_cos(right[3][m], wrong)                 # no th (:152)
            if info is not None and float(th) != 1.0:
                inside = set(mm.candidates(Fr.cam[1], right[1][m][0], right[1][m][1], F(r * F(right[4][m])), -1, -1))
                wider = set(mm.candidates(Fr.cam[1], right[1][m][0], right[1][m][1], F(F(r * F(th)) * F(right[4][m])), -1, -1))
                _count(info, "right only inside th x radius", len(wider - inside))
            if wrong == "right_uses_th" and float(th) != 1.0:
                r = F(r * F(th))
            rs = F(r * F(right[4][m]))
            what, gi = _map_sub(Fr, 1, right[1][m][0], right[1][m][1], rs, L, qd[m], m, slots, mp_obs, ratio, via_link, wrong, info)
            if what == "match":
                li = int(r2l[gi - nL])
                if li != -1:                                                 # :204-208, before the right slot
                    claim(li, m, True)
                    _count(info, "partner claimed")
                else:
                    _count(info, "no partner")
                claim(gi, m, False)
    if wrong == "count_slots":
        n = sum(1 for v in slots if v >= 0)
    return n, np.array(slots, np.int32)


# ---------------------------------------------------------------------------------------------------
def search_by_projection_last_twocam(Fr, last_kps, valid, uv, uv_r, mp_desc, mp_obs, cur_mp, th, level_scale, mode=0, check_ori=True,
                                     wrong=None, info=None):
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono) :1969-2187 on a two-camera current frame, after the two projections:
    valid / uv the left one with :2007-2015 folded in, uv_r = project(mTrl x3Dc) (:2093-2095, no bounds check).  last_kps: octave =
    LastFrame.getKPtLevelMono(i), angle.  mode 0 / 1 / 2: neither, bForward, bBackward.  -> (nmatches, the current frame's slots)"""
    n = 0
    slots = [int(v) for v in cur_mp]
    qd = mm.as_ints(mp_desc)
    hist = mm._Hist(check_ori, wrong)
    nL = Fr.nL
    none = set()

    def best_of(cam, i, cand):
        fr, base = Fr.cam[cam], cam * nL
        ds = [(mm.hamming(qd[i], fr.desc[c]), c) for c in cand if _open(slots[base + c], base + c, mp_obs, none, wrong, info)]
        best, idx, _, _, _ = mm._scan(ds, wrong, 256)
        if info is not None:
            info.setdefault("best", []).append((i, cam, best, None))
            _count(info, "LR"[cam] + " best == TH", best == TH_HIGH)
            _count(info, "LR"[cam] + " best == TH + 1", best == TH_HIGH + 1)
        return best, idx, ds

    def commit(cam, i, idx):
        nonlocal n
        gi = cam * nL + idx
        _count(info, "slot written twice", slots[gi] >= 0)
        slots[gi] = i
        n += 1
        key = idx if cam and wrong == "rot_right_local_index" else gi       # rotHist gets bestIdx2 + numKPtsLeft() :2155
        hist.push(last_kps["angle"][i], Fr.cam[cam].kps["angle"][idx], key)
        if info is not None:
            info.setdefault("pushes", []).append((i, gi))
    for i in range(len(last_kps)):
        if not valid[i]:
            continue
        L = int(last_kps["octave"][i])
        radius = F(th) * F(level_scale[i])
        lo, hi = {0: (L - 1, L + 1), 1: (L, -1), 2: (0, L)}[mode]
        cand = mm.candidates(Fr.cam[0], uv[i][0], uv[i][1], radius, lo, hi, wrong)
        empty = not cand
        if cand:
            best, idx, ds = best_of(0, i, cand)
            _window_probe(Fr, 0, uv[i][0], uv[i][1], radius, cand, ds, info)
            _count(info, "left window all closed", not ds)
            if wrong == "last_empty_after_slots":
                empty = not ds
        if empty:                                                            # vIndices2.empty() :2033-2034: the right block is skipped too
            if info is not None:
                rc = mm.candidates(Fr.cam[1], uv_r[i][0], uv_r[i][1], radius, lo, hi, wrong, levels=Fr.gate)
                rb = [mm.hamming(qd[i], Fr.cam[1].desc[c]) for c in rc if not mm.holds_observed(slots[nL + c], mp_obs, wrong)]
                _count(info, "left window empty, right matches", bool(rb) and min(rb) <= TH_HIGH)
            if wrong != "last_right_without_left_window":
                continue
        elif (best < TH_HIGH) if wrong == "th_strict" else (best <= TH_HIGH):
            commit(0, i, idx)
        hi_r = L + 1 if mode == 1 and wrong == "last_right_forward_capped" else hi
        cand = _right_candidates(Fr, uv_r[i][0], uv_r[i][1], radius, lo, hi_r, wrong, info)
        best, idx, ds = best_of(1, i, cand)
        _window_probe(Fr, 1, uv_r[i][0], uv_r[i][1], radius, cand, ds, info)
        if (best < TH_HIGH) if wrong == "th_strict" else (best <= TH_HIGH):
            commit(1, i, idx)
    if check_ori:
        n = mm._clear_losers(hist, slots, n, wrong)
    if wrong == "count_slots":
        n = sum(1 for v in slots if v >= 0)
    return n, np.array(slots, np.int32)


# ---------------------------------------------------------------------------------------------------
def search_by_bow_twocam(kf_kps, kf_desc, kf_has_mp, kf_fv, f_kps, nL, f_desc, f_fv, ratio, check_ori=True, wrong=None, info=None):
    """SearchByBoW(pKF, F, vpMapPointMatches) :276-478 with F.numKPtsLeft() != -1 -> (nmatches, the KeyFrame index per frame feature)"""
    n = 0
    match_f = [-1] * len(f_kps)
    d1, d2 = mm.as_ints(kf_desc), mm.as_ints(f_desc)
    hist = mm._Hist(check_ori, wrong)
    D = mm.first_dist(TH_LOW, ratio)
    below = (lambda d: d < TH_LOW) if wrong == "th_strict" else (lambda d: d <= TH_LOW)

    def commit(ikf, idx):
        nonlocal n
        match_f[idx] = ikf
        hist.push(kf_kps["angle"][ikf], f_kps["angle"][idx], idx)
        if info is not None:
            info.setdefault("pushes", []).append((ikf, idx))
        n += 1
    for l1, l2 in mm._common_nodes(kf_fv, f_fv):
        for ikf in l1:
            if not kf_has_mp[ikf]:
                continue
            free = [i for i in l2 if match_f[i] < 0]
            ds = [(mm.hamming(d1[ikf], d2[i]), i) for i in free]
            if wrong == "bow_sides_merged":
                dl, dr = ds, []
            else:
                dl, dr = [e for e in ds if e[1] < nL], [e for e in ds if e[1] >= nL]      # `realIdxF < F.numKPtsLeft()` :359-375
            best, idx, _, second, _ = mm._scan(dl, wrong, 256)
            bestr, idxr, _, secondr, _ = mm._scan(dr, wrong, 256)
            if wrong == "second_cut" and second >= D - 1:
                second = 256
            if info is not None:
                info.setdefault("best", []).append((ikf, best, second, bestr, secondr))
                _count(info, "bow node > 64", len(l2) > 64)
                _count(info, "bow competed", len(free) < len(l2))
                for t, name in ((TH_LOW, "TH"), (TH_LOW + 1, "TH + 1")):
                    _count(info, "bow left == %s, right <= TH" % name, best == t and bestr <= TH_LOW)
                    _count(info, "bow left == %s, right > TH" % name, best == t and TH_LOW < bestr < 256)
                _count(info, "L best == TH", best == TH_LOW); _count(info, "L best == TH + 1", best == TH_LOW + 1)
                _count(info, "R best == TH", best <= TH_LOW and bestr == TH_LOW); _count(info, "R best == TH + 1", best <= TH_LOW and bestr == TH_LOW + 1)
                _count(info, "L ratio equal", best <= TH_LOW and bool(F(best) == F(second) * F(ratio)))
                _count(info, "bow tie across sides", best <= TH_LOW and best == bestr)
                _count(info, "tie", sum(1 for d, _ in dl if d == best) > 1 or (best <= TH_LOW and sum(1 for d, _ in dr if d == bestr) > 1))
                if best <= TH_LOW and bestr <= TH_LOW:
                    lok = mm._ratio_ok(best, second, ratio, None)
                    _count(info, "bow left ratio fails, right taken", not lok)
                    _count(info, "bow both sides", lok)
                    _count(info, "bow right ratio would fail", not mm._ratio_ok(bestr, secondr, ratio, None))
            do_l = below(best) and mm._ratio_ok(best, second, ratio, wrong)                 # :380-382
            do_r = (below(best) or wrong == "bow_right_ungated") and below(bestr)           # :410 inside :380; `|| true` :412
            if wrong == "bow_right_ratio":
                do_r = do_r and mm._ratio_ok(bestr, secondr, ratio, wrong)
            if wrong == "bow_right_needs_left_ratio":
                do_r = do_r and do_l
            if wrong == "bow_right_first":
                if do_r:
                    commit(ikf, idxr)
                if do_l:
                    commit(ikf, idx)
            else:
                if do_l:
                    commit(ikf, idx)
                if do_r:
                    commit(ikf, idxr)
    if check_ori:
        for idx, _ in hist.losers():
            match_f[idx] = -1
            n -= 1
    if wrong == "count_slots":
        n = sum(1 for v in match_f if v >= 0)
    return n, np.array(match_f, np.int32)
