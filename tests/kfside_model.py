"""The KeyFrame-side radius search beyond the mono core of edge_inputs.radius_match_model, written from the reference's text: the search
loop of Fuse (src/ORBmatcher.cc:1512-1578) with its stereo gate (:1541-1566), of SearchByProjection(pKF, Scw, vpPoints, vpMatched,
th, ratioHamming) (:548-588) with its in-order claim, of MixedMatcher::Fuse (src/MixedMatcher.cpp:1703-1758: the type gate,
getKPtLevelMono and getKPtInvLevelSigma2 per keypoint) and the agreement pass of SearchBySim3 (:1948-1964).  Conventions of
tests/match_model.py: Python integers, numpy float32 one operation at a time, candidates over all keypoints in GetFeaturesInArea's
order, `wrong=`, and a probe through `info=`.

The forms that project on the device (FusePose, SearchByProjectionKFScw, SearchBySim3Pose, FuseKeyFrames) are modelled as the
projection of tests/kfside_ref (held to the kernels by tests/test_gpu_kfside.py) followed by radius_search."""
import collections
import functools
import types

import numpy as np

from oracle.oracle_py import KP_DTYPE
import match_model as mm
import match_scenes as ms

F = np.float32
W, H = ms.W, ms.H
RADIUS = 8.0
NLEVELS = 8
INV_SIGMA2 = (1.0 / np.float32(1.2) ** (2 * np.arange(NLEVELS))).astype(np.float32)

WRONG = {
    "stereo_gate_mono": "5.99 without er where uright >= 0",
    "uright_gt_zero": "> 0 for >= 0 on mvuRight",
    "chi2_float": "the chi-square compared in float",
    "chi2_ge": ">= for > at 5.99 / 7.8",
    "octave_unchecked": "the octave skip left out (the sigma of the nearest level is read)",
    "taken_ignored": "the taken flags ignored",
    "taken_always": "a keypoint closes whatever its distance",
    "accept_lt": "< for <= at accept_thr",
    "mixed_level_octave": "a non-ORB keypoint's level read from octave",
    "type_gate_off": mm.WRONG["type_gate_off"],
    "agree_one_way": "the agreement checked in one direction only",
    "agree_th_one_side": "th_high applied to one direction only",
    "tie_last": mm.WRONG["tie_last"], "tie_index": mm.WRONG["tie_index"], "window_le": mm.WRONG["window_le"], "level_off": mm.WRONG["level_off"],
}


def grid_of(minX, minY, maxX, maxY):
    """the grid bounds of a keyframe as the models read them (Frame.cc:362-363: 64 / 48 cells over the bounds, in float)"""
    return types.SimpleNamespace(minX=float(F(minX)), minY=float(F(minY)), maxX=float(F(maxX)), maxY=float(F(maxY)),
                                 invW=float(F(64.0) / (F(maxX) - F(minX))), invH=float(F(48.0) / (F(maxY) - F(minY))))


def _gate_rejects(u, v, kp, s, kpr, ur, wrong, probe):
    """the reprojection gate of Fuse (:1541-1566; MixedMatcher.cpp:1719-1745) on one candidate: e2 with er against 7.8 where
    mvuRight[idx] >= 0, else e2 against 5.99; the float product e2 * s against the double constant"""
    ex, ey = F(u - F(kp["x"])), F(v - F(kp["y"]))
    kpr = F(-1.0) if kpr is None else F(kpr)
    probe["uright == 0"] += int(kpr == 0)
    if (kpr > 0 if wrong == "uright_gt_zero" else kpr >= 0) and wrong != "stereo_gate_mono":
        er = F(F(ur) - kpr)
        e2, limit, name = F(F(F(ex * ex) + F(ey * ey)) + F(er * er)), 7.8, "7.8"
    else:
        e2, limit, name = F(F(ex * ex) + F(ey * ey)), 5.99, "5.99"
    p = F(e2 * s)
    lo, hi = float_pair_around(limit)
    probe["chi2 == the float above " + name] += int(p == hi)
    probe["chi2 == the float below " + name] += int(p == lo)
    probe["stereo gate" if limit == 7.8 else "mono gate"] += 1
    if wrong == "chi2_float":
        out = bool(p > F(limit))
    elif wrong == "chi2_ge":
        out = float(p) >= limit
    else:
        out = float(p) > limit
    probe["gate rejects"] += int(out)
    return out


def radius_search(kps, desc, valid, uv, radius, level, q_desc, inv_sigma2=None, uright=None, q_ur=None, taken=None, accept_thr=0.0, wrong=None,
                  info=None, gb=None, kp_is_orb=None, mp_is_orb=None, kp_inv_sigma2=None):
    """-> (best_idx, best_dist[, taken out]); (-1, 256) where nothing qualifies.  inv_sigma2: the reprojection gate (5.99, or 7.8 with
    er where uright[i] >= 0); taken: vpMatched in, a keypoint closes when (float)bestDist <= accept_thr (`bestDist<=TH_LOW*ratioHamming`)"""
    fr = mm.frame(kps, desc, W, H)
    if gb is not None:
        fr.gb = gb
    qd = mm.as_ints(q_desc)
    mixed = kp_is_orb is not None or mp_is_orb is not None or kp_inv_sigma2 is not None
    M = len(valid)
    bi, bd = np.full(M, -1, np.int32), np.full(M, 256, np.int32)
    tk = None if taken is None else [int(v) for v in taken]
    probe = collections.Counter()
    for m in range(M):
        if not valid[m]:
            continue
        u, v, L = F(uv[m][0]), F(uv[m][1]), int(level[m])
        ds = []
        for i in mm.candidates(fr, u, v, F(radius[m]), -1, -1, wrong):
            if tk is not None and tk[i] and wrong != "taken_ignored":       # `if(vpMatched[idx]) continue;` :563
                probe["taken met"] += 1
                continue
            o = int(kps["octave"][i])
            if mixed:                                                        # MixedMatcher.cpp:1706-1717
                orb = mm.is_orb(kp_is_orb, i)
                probe["other type"] += int(orb != mm.is_orb(mp_is_orb, m))
                if orb != mm.is_orb(mp_is_orb, m) and wrong != "type_gate_off":
                    continue
                if not orb and wrong != "mixed_level_octave":                # getKPtLevelMono: class_id of a non-ORB row
                    probe["class_id level != octave"] += int(int(kps["class_id"][i]) != o)
                    o = int(kps["class_id"][i])
            lo, hi = (L - 2, L + 1) if wrong == "level_off" else (L - 1, L)
            if o < lo or o > hi:
                continue
            if mixed and kp_inv_sigma2 is not None:
                s = F(kp_inv_sigma2[i])                                      # getKPtInvLevelSigma2(idx), MixedMatcher.cpp:1732, :1743
            elif not mixed and inv_sigma2 is not None:
                if o < 0 or o >= len(inv_sigma2):                            # (getORBInvLevelSigma2 asserts the range, KeyFrame.cc:1414-1417)
                    probe["octave outside the levels"] += 1
                    if wrong != "octave_unchecked":
                        continue
                s = F(inv_sigma2[min(max(o, 0), len(inv_sigma2) - 1)])
            else:
                s = None
            if s is not None and _gate_rejects(u, v, kps[i], s, None if uright is None else uright[i], None if q_ur is None else q_ur[m], wrong, probe):
                continue
            ds.append((mm.hamming(qd[m], fr.desc[i]), i))
        best, idx, _, _, _ = mm._scan(ds, wrong, 256)
        if idx >= 0:
            bi[m], bd[m] = idx, best
            probe["tie"] += int(sum(1 for d, _ in ds if d == best) > 1)
            if tk is not None:
                thr = F(accept_thr)
                probe["best == accept_thr"] += int(F(best) == thr)
                probe["best just above accept_thr"] += int(F(best) > thr and F(best - 1) <= thr)
                if wrong == "taken_always" or ((F(best) < thr) if wrong == "accept_lt" else (F(best) <= thr)):
                    tk[idx] = 1
    if info is not None:
        info["probe"] = probe
    return (bi, bd) if tk is None else (bi, bd, np.array(tk, np.uint8))


def sim3_agree(bi1, bd1, bi2, bd2, th_high, wrong=None, info=None):
    """SearchBySim3 after its two searches: vnMatch1 / vnMatch2 = the best of each side where bestDist <= TH_HIGH (:1862-1866,
    :1942-1946), then the agreement pass (:1948-1964).  -> (nFound, match12, vnMatch1, vnMatch2)"""
    vn1 = [int(i) if int(d) <= th_high else -1 for i, d in zip(bi1, bd1)]
    vn2 = [int(i) if int(d) <= th_high or wrong == "agree_th_one_side" else -1 for i, d in zip(bi2, bd2)]
    probe = collections.Counter()
    for d in list(bd1) + list(bd2):
        probe["best == th_high"] += int(d == th_high); probe["best == th_high + 1"] += int(d == th_high + 1)
    m12 = [-1] * len(vn1)
    for i1, idx2 in enumerate(vn1):
        if idx2 >= 0:
            back = vn2[idx2]
            probe["agreed" if back == i1 else "one way only"] += 1
            if back == i1 or wrong == "agree_one_way":
                m12[i1] = idx2
    if info is not None:
        info["probe"] = probe
    return sum(1 for v in m12 if v >= 0), np.array(m12, np.int32), np.array(vn1, np.int32), np.array(vn2, np.int32)


# ---------------------------------------------------------------------------------------------------
def float_pair_around(c):
    """the largest float not above the double c and the float after it"""
    lo = F(c) if float(F(c)) <= c else np.nextafter(F(c), F(0))
    return lo, np.nextafter(lo, F(100))


def plant_e2(target, kx, ky):
    """(u, v) as floats with fl(fl(ex ex) + fl(ey ey)) == target for ex = u - kx, ey = v - ky; None when the search finds none"""
    target = F(target)
    for back in (1e-6, 2e-6, 5e-6, 1e-5, 3e-5, 1e-4, 3e-4, 1e-3):
        u = F(kx + np.sqrt(float(target) - back))
        ex = F(u - F(kx)); a = F(ex * ex)
        if not a < target:
            continue
        base = F(ky + np.sqrt(float(target) - float(a)))
        vs = (np.array([base], np.float32).view(np.int32) + np.arange(-4000, 4000, dtype=np.int32)).view(np.float32)
        ey = vs - F(ky)
        hit = np.flatnonzero((a + ey * ey) == target)
        if len(hit):
            return u, vs[hit[0]]
    return None


ACCEPT = (50.0, 37.5)                                                        # TH_LOW * ratioHamming for ratios 1.0 and 0.75
FORMS = ("plain", "mono gate", "stereo gate", "in order 50", "in order 37.5", "mixed", "mixed gate", "mixed in order 50")


@functools.lru_cache(maxsize=None)
def scene():
    """Sites on the lattice of tests/match_scenes.py, radius 8, one or two queries each.  Keypoints of octave 0 have inv_sigma2 = 1, so
    the chi-square is e2 itself."""
    rng = np.random.default_rng(401)
    free = list(ms.SITES[:-1])
    K, Q, names = [], [], []
    rand = lambda: int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little")
    flip = lambda d, k: ms._flip(d, rng.permutation(256)[:k])

    def kp(x, y, desc, octave=0, ur=-1.0, taken=0, orb=1, cid=-1, sig=None):
        sig = INV_SIGMA2[min(max(octave, 0), NLEVELS - 1)] if sig is None else sig
        K.append(dict(x=F(x), y=F(y), octave=octave, desc=desc, ur=F(ur), taken=taken, orb=orb, cid=cid, sig=F(sig))); return len(K) - 1

    def query(name, u, v, desc, level=0, ur=0.0, orb=1):
        Q.append(dict(u=F(u), v=F(v), level=level, desc=desc, ur=F(ur), orb=orb)); names.append(name)
    lo599, hi599 = float_pair_around(5.99)
    lo78, hi78 = float_pair_around(7.8)
    assert float(hi78) == float(F(7.8)) and float(lo599) == float(F(5.99))
    for name, target, ur, qur in (("mono chi2 the float below 5.99", lo599, -1.0, 0.0), ("mono chi2 the float above 5.99", hi599, -1.0, 0.0),
                                  ("stereo chi2 the float below 7.8, er 0", lo78, 50.0, 50.0), ("stereo chi2 == 7.8f, er 0", hi78, 50.0, 50.0),
                                  ("stereo chi2 the float below 7.8, er 1", F(lo78 - F(1)), 50.0, 51.0), ("stereo chi2 == 7.8f, er 1", F(hi78 - F(1)), 50.0, 51.0),
                                  ("uright 0: e2 6.5 under the stereo gate", F(6.5), 0.0, 0.0), ("uright -0: e2 6.5 under the stereo gate", F(6.5), -0.0, 0.0),
                                  ("stereo: e2 6.5 without er passes 7.8, not 5.99", F(6.5), 30.0, 30.0), ("stereo: ex ey small, er 3", F(0.5), 30.0, 33.0)):
        c = free.pop(0)
        uv = plant_e2(target, float(c[0]), float(c[1]))
        assert uv is not None, name
        d = rand()
        kp(c[0], c[1], flip(d, 10), ur=ur)
        kp(F(uv[0] + F(1.0)), F(uv[1] + F(1.0)), flip(d, 40))                # a second keypoint inside every gate: ex = ey = -1, e2 = 2
        query(name, uv[0], uv[1], d, ur=qur)
    for name, octave, level in (("octave 8 of 8 levels", NLEVELS, NLEVELS), ("octave -1", -1, 0)):
        c = free.pop(0); d = rand()
        kp(c[0], c[1], flip(d, 10), octave=octave); kp(c[0] + 1, c[1] + 1, flip(d, 40), octave=min(max(octave, 0), NLEVELS - 1))
        query(name, c[0], c[1], d, level=level)
    c = free.pop(0); d = rand()
    for o, dist in ((0, 10), (1, 20), (2, 30), (3, 5)):
        kp(c[0] + o, c[1], flip(d, dist), octave=o)
    query("levels: octaves 0..3 around level 2", c[0], c[1], d, level=2)
    for name, offs in (("tie: two cells, the later cell first", ((3.75, 0), (0, 0))), ("tie: one cell", ((0, 0), (0.25, 0)))):
        c = free.pop(0); d = rand()
        for o in offs:
            kp(c[0] + o[0], c[1] + o[1], flip(d, 20))
        query(name, c[0], c[1], d)
    c = free.pop(0); d = rand()
    kp(F(c[0] + 8.0), c[1], flip(d, 10)); kp(c[0], c[1] + 1, flip(d, 40))
    query("window: |dx| == r", c[0], c[1], d)
    # ---- the in-order form
    c = free.pop(0); d = rand()
    kp(c[0], c[1], flip(d, 10), taken=1); kp(c[0] + 1, c[1] + 1, flip(d, 30))
    query("taken on entry: the second best is found", c[0], c[1], d)
    for thr in ACCEPT:
        t = int(thr)                                                        # 50 <= 50.0 and 37 <= 37.5 close; 51 and 38 do not
        for best in (t, t + 1):
            c = free.pop(0)
            cl = ms._Cluster(type("B", (), dict(rng=rng, rand_desc=staticmethod(rand)))(), 2, 20)
            kp(c[0], c[1], cl.desc[0]); kp(c[0] + 1, c[1] + 1, cl.desc[1])
            query("in order: best %d against accept_thr %.1f, a second query then wants the same keypoint" % (best, thr), c[0], c[1], cl.query({0: best, 1: best + 30}))
            query("in order: the second query after best %d against %.1f" % (best, thr), c[0], c[1], cl.query({0: 10, 1: 40}))
    # ---- the mixed form: rows of the other type carry their level in class_id and a sigma of their own
    c = free.pop(0); d = rand()
    kp(c[0], c[1], flip(d, 10), octave=0, orb=0, cid=2); kp(c[0] + 1, c[1] + 1, flip(d, 40), octave=2, orb=0, cid=2)
    query("mixed: class_id 2 passes level 2, octave 0 would not", c[0], c[1], d, level=2, orb=0)
    c = free.pop(0); d = rand()
    kp(c[0], c[1], flip(d, 10), octave=2, orb=0, cid=5); kp(c[0] + 1, c[1] + 1, flip(d, 40), octave=1, orb=0, cid=2)
    query("mixed: class_id 5 fails level 2, octave 2 would pass", c[0], c[1], d, level=2, orb=0)
    c = free.pop(0); d = rand()
    kp(c[0], c[1], flip(d, 5), orb=1); kp(c[0] + 1, c[1] + 1, flip(d, 20), orb=0, cid=0)
    query("mixed: the nearest keypoint is of the other type (point not ORB)", c[0], c[1], d, orb=0)
    c = free.pop(0); d = rand()
    kp(c[0], c[1], flip(d, 5), orb=0, cid=0); kp(c[0] + 1, c[1] + 1, flip(d, 20), orb=1)
    query("mixed: the nearest keypoint is of the other type (point ORB)", c[0], c[1], d, orb=1)
    c = free.pop(0); d = rand()
    kp(c[0] + 2.0, c[1], flip(d, 10), orb=0, cid=0, sig=1.6); kp(c[0] + 1, c[1] + 1, flip(d, 40), orb=0, cid=0, sig=1.0)
    query("mixed: e2 4 under a sigma of its own, 1.6 (6.4 > 5.99)", c[0], c[1], d, orb=0)
    k = 0
    while free:
        c = free.pop(0); d = rand()
        kp(c[0] + 0.5, c[1] - 0.5, flip(d, 10 + k), octave=k % 2, ur=-1.0 if k % 3 else 40.0 + k)
        query("plain %d" % k, c[0], c[1], d, level=k % 2 + (k % 4 == 3), ur=41.0 + k); k += 1
    kps = np.zeros(len(K), KP_DTYPE)
    for f in ("x", "y", "octave"):
        kps[f] = [k_[f] for k_ in K]
    kps["size"] = 31.0; kps["class_id"] = [k_["cid"] for k_ in K]
    sc = dict(kp_is_orb=np.array([k_["orb"] for k_ in K], np.uint8), kp_inv_sigma2=np.array([k_["sig"] for k_ in K], np.float32),
              mp_is_orb=np.array([q["orb"] for q in Q], np.uint8), kps=kps, desc=ms._to_u8([k_["desc"] for k_ in K]), uright=np.array([k_["ur"] for k_ in K], np.float32),
              taken=np.array([k_["taken"] for k_ in K], np.uint8), valid=np.ones(len(Q), np.uint8),
              uv=np.array([[q["u"], q["v"]] for q in Q], np.float32), radius=np.full(len(Q), RADIUS, np.float32),
              level=np.array([q["level"] for q in Q], np.int32), q_desc=ms._to_u8([q["desc"] for q in Q]), q_ur=np.array([q["ur"] for q in Q], np.float32),
              names=np.array(names))
    for a in sc.values():
        a.setflags(write=False)
    return sc


def form_kw(sc, form):
    kw = {}
    if form.startswith("mixed"):
        kw = dict(kp_is_orb=sc["kp_is_orb"], mp_is_orb=sc["mp_is_orb"])
        if form == "mixed gate":
            kw.update(kp_inv_sigma2=sc["kp_inv_sigma2"], uright=sc["uright"], q_ur=sc["q_ur"])
    elif form == "mono gate":
        kw = dict(inv_sigma2=INV_SIGMA2)
    elif form == "stereo gate":
        kw = dict(inv_sigma2=INV_SIGMA2, uright=sc["uright"], q_ur=sc["q_ur"])
    if "in order" in form:
        kw.update(taken=sc["taken"], accept_thr=float(form.split()[-1]))
    return kw


def in_range(sc, form):
    """the queries the oracle is given.  With the ORB forms' gate, those whose candidates all have an octave inside the levels: outside
    them the reference is undefined (getORBInvLevelSigma2 asserts, KeyFrame.cc:1414-1417) and the oracle, which is not told the number
    of levels, would index past inv_sigma2.  The kernels skip such a keypoint; the two sites built for it hold them to that
    convention through the model alone"""
    return np.array([not (n.startswith("octave") and form in ("mono gate", "stereo gate")) for n in sc["names"]], np.uint8)


def run_model(sc, form, wrong=None, info=None, valid=None):
    return radius_search(sc["kps"], sc["desc"], sc["valid"] if valid is None else valid, sc["uv"], sc["radius"], sc["level"], sc["q_desc"],
                         wrong=wrong, info=info, **form_kw(sc, form))


def run_oracle(oracle, sc, form):
    """oracle/orc_match.c; for the mixed forms the restatement of tests/kfside_mixed_ref over the oracle's grid"""
    fr = oracle.Frame(sc["kps"], sc["desc"], W, H)
    if form.startswith("mixed"):
        import kfside_mixed_ref as mref
        mref.use_oracle(oracle)
        kw = form_kw(sc, form)
        kw.pop("q_ur", None)
        p = dict(valid=sc["valid"], uv=sc["uv"], radius=sc["radius"], level=sc["level"], q_ur=sc["q_ur"])
        return mref.search(fr, p, sc["q_desc"], **kw)
    return oracle.kf_radius_match(fr, in_range(sc, form), sc["uv"], sc["radius"], sc["level"], sc["q_desc"], **form_kw(sc, form))


def run_kernels(fe, ctx, sc, form):
    call = fe.KeyFrameRadiusMatchMixed if form.startswith("mixed") else fe.KeyFrameRadiusMatch
    return call(sc["kps"], sc["desc"], fe.grid_bounds(W, H), sc["valid"], sc["uv"], sc["radius"], sc["level"], sc["q_desc"], ctx=ctx,
                **form_kw(sc, form))


# ---------------------------------------------------------------------------------------------------
# the forms that project on the device: K keyframes with grid bounds, sizes and edge values of their own
SIZES = ((346, 260), (320, 240), (400, 300), (346, 260), (300, 200))         # keyframe k's grid covers SIZES[k]; the views keep 346 x 260
TH_VALUES = (3.0, 0.0, -1.0, float("nan"), float("inf"))                    # radius = th * scale factor: the edge values of the radius


def edge_keypoints(kps, Wk, Hk):
    """the last rows of a keyframe's keypoints moved to the special values of tests/edge_inputs.py in x, in y and in both, and to the
    positions that just reach and just miss the grid's first and last column and row"""
    import edge_inputs as ei
    kps = kps.copy()
    xs = [v for _, v in ei.SPECIALS] + [Wk * 63.4 / 64, Wk * 63.6 / 64, -Wk * 0.4 / 64, -Wk * 0.6 / 64]
    ys = [v for _, v in ei.SPECIALS] + [Hk * 47.4 / 48, Hk * 47.6 / 48, -Hk * 0.4 / 48, -Hk * 0.6 / 48]
    at = len(kps) - 1
    for x, y in zip(xs, ys):
        for a in range(3):
            if a != 1:
                kps["x"][at] = x
            if a != 0:
                kps["y"][at] = y
            at -= 1
    assert at > 40, "the keyframe is too small for the edge values"
    return kps


@functools.lru_cache(maxsize=None)
def batch_scene(K=3, M=500, n_kps=(0, 260, 230), seed=61, edges=True, mixed=False):
    """synth.keyframe_neighbourhood with keyframe k on its own grid (SIZES[k]), its own keypoint count (one of them 0) and, in every
    keyframe but the first, edge values among the keypoint positions"""
    from eorb_slam_amd import synth
    sc = (synth.mixed_keyframe_neighbourhood if mixed else synth.keyframe_neighbourhood)(seed, K, M, n_kps=list(n_kps))
    sc = dict(sc)
    if edges:
        sc["kps"] = [k if i == 0 or len(k) == 0 else edge_keypoints(k, *SIZES[i]) for i, k in enumerate(sc["kps"])]
    return sc


def batch_model(sc, p, gate, k, wrong=None, info=None, taken=None, accept_thr=0.0):
    """radius_search in keyframe k over rows k of the projection p (tests/kfside_ref.keyframe_side over all K views)"""
    M = len(sc["min_dist"])
    pk = {n: p[n][k * M:(k + 1) * M] for n in p}
    if len(sc["kps"][k]) == 0:
        return np.full(M, -1, np.int32), np.full(M, 256, np.int32)
    kw = {}
    if "mp_is_orb" in sc:
        kw = dict(kp_is_orb=sc["kp_is_orb"][k], mp_is_orb=sc["mp_is_orb"])
        if gate != "none":
            kw["kp_inv_sigma2"] = sc["kp_inv_sigma2"][k]
    elif gate != "none":
        kw = dict(inv_sigma2=sc["inv_sigma2"])
    if gate == "stereo":
        kw.update(uright=sc["uright"][k], q_ur=pk["q_ur"])
    if taken is not None:
        kw.update(taken=taken, accept_thr=accept_thr)
    return radius_search(sc["kps"][k], sc["desc"][k], pk["valid"], pk["uv"], pk["radius"], pk["level"], sc["mp_desc"], wrong=wrong, info=info,
                         gb=grid_of(0.0, 0.0, *SIZES[k]), **kw)


def batch_oracle(oracle, sc, p, gate, k):
    M = len(sc["min_dist"])
    pk = {n: p[n][k * M:(k + 1) * M] for n in p}
    if len(sc["kps"][k]) == 0:
        return np.full(M, -1, np.int32), np.full(M, 256, np.int32)
    kw = dict(inv_sigma2=None if gate == "none" else sc["inv_sigma2"])
    if gate == "stereo":
        kw.update(uright=sc["uright"][k], q_ur=pk["q_ur"])
    return oracle.kf_radius_match(oracle.Frame(sc["kps"][k], sc["desc"][k], *SIZES[k]), pk["valid"], pk["uv"], pk["radius"], pk["level"], sc["mp_desc"], **kw)


def cat(sc):
    off = np.concatenate([[0], np.cumsum([len(k) for k in sc["kps"]])]).astype(np.int32)
    return np.concatenate(sc["kps"]), np.concatenate(sc["desc"]), np.concatenate(sc["uright"]), off


def geom(sc):
    return sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"]


# ---- SearchBySim3
@functools.lru_cache(maxsize=None)
def sim3_scene():
    from eorb_slam_amd import synth
    return synth.sim3_pair(47, n=300, n_both=80, n_one=40, n_cross=40)


def sim3_projections(ref, sp, th=7.5):
    k1, k2 = sp["kf1"], sp["kf2"]
    v1, v2 = ref.view(**k1["view"]), ref.view(**k2["view"])
    cam = k1["view"]["cam"]
    return (ref.sim3_half(v1, sp["sR21"], sp["t21"], cam, v2, k1["pos"], k1["min_dist"], k1["max_dist"], th, skip=k1["skip"]),
            ref.sim3_half(v2, sp["sR12"], sp["t12"], cam, v1, k2["pos"], k2["min_dist"], k2["max_dist"], th, skip=k2["skip"]))


def sim3_searches(sp, p12, p21):
    """the two radius searches by the model: KF1's points in KF2, KF2's in KF1 -> (bi1, bd1, bi2, bd2)"""
    k1, k2 = sp["kf1"], sp["kf2"]
    gb = grid_of(0.0, 0.0, sp["W"], sp["H"])
    a = radius_search(k2["kps"], k2["desc"], p12["valid"], p12["uv"], p12["radius"], p12["level"], k1["mp_desc"], gb=gb)
    b = radius_search(k1["kps"], k1["desc"], p21["valid"], p21["uv"], p21["radius"], p21["level"], k2["mp_desc"], gb=gb)
    return a[0], a[1], b[0], b[1]


def sim3_th_values(bd1, bd2, bi1, bi2):
    """TH_HIGH, and the thresholds that put a pair's two distances on either side: the larger distance of an agreeing pair and one less"""
    out = [100]
    for i1, i2 in enumerate(bi1):
        if i2 >= 0 and bi2[i2] == i1 and bd1[i1] != bd2[i2]:
            out += [int(max(bd1[i1], bd2[i2])), int(max(bd1[i1], bd2[i2])) - 1]
            if len(out) >= 7:
                break
    return out
