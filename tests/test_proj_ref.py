"""The CPU restatement of the map-point projector (tests/proj_ref): its logf against the host libm, MapPoint::PredictScale known
answers, hand-derived Frame::isInFrustum cases and a numpy restatement of mode A, bit for bit.  No GPU."""
import ctypes as C
import os
import re
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proj_ref                                     # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

F32 = np.float32
LO_BITS = int(F32(2.0 ** -10).view(np.uint32))      # every float in [2^-10, 2^20]: 251 658 241 inputs
HI_BITS = int(F32(2.0 ** 20).view(np.uint32))


def _bits(x):
    return int(np.asarray(x, F32).view(np.uint32))


def _host_is_known_glibc():
    """glibc 2.27 .. 2.40 ship the e_logf.c that proj_ref restates"""
    try:
        f = C.CDLL(None).gnu_get_libc_version
    except (OSError, AttributeError):
        return False
    f.restype = C.c_char_p
    m = re.match(rb"(\d+)\.(\d+)", f())
    return bool(m) and (2, 27) <= (int(m.group(1)), int(m.group(2))) <= (2, 40)


def test_logf_equals_the_host_logf_on_every_float_of_the_range():
    bad, first = proj_ref.logf_mismatches(LO_BITS, HI_BITS)
    if bad and not _host_is_known_glibc():
        # another libm: its results are not the reference's; the inputs on which it disagrees are left out, every other one matched
        warnings.warn("host logf is not glibc 2.27-2.40's: %d of %d inputs differ (first bits %08x) and were skipped"
                      % (bad, HI_BITS - LO_BITS + 1, first))
        return
    assert bad == 0, "pr_logf differs from the host logf on %d inputs, first bits %08x" % (bad, first)


def test_logf_special_values():
    assert _bits(proj_ref.logf(1.0)) == 0                                             # +0, not -0
    assert np.isposinf(proj_ref.logf(np.inf))
    assert np.isneginf(proj_ref.logf(0.0))
    assert np.isnan(proj_ref.logf(-1.0))
    # subnormals go through x * 2^23: the smallest ones, the largest ones and a stride through the rest
    sub = np.concatenate([np.arange(1, 4097), np.arange(0x007ff000, 0x00800000), np.arange(1, 0x00800000, 4099)]).astype(np.uint32)
    x = sub.view(F32)
    got = proj_ref.logf_n(x)
    want = np.array([np.float32(np.log(np.float64(v))) for v in x[:64]], F32)      # correctly rounded here: log in double, far from a tie
    assert np.array_equal(got[:64], want)
    if _host_is_known_glibc():
        for lo, hi in ((1, 4096), (0x007ff000, 0x007fffff)):
            assert proj_ref.logf_mismatches(lo, hi)[0] == 0
    assert np.all(np.diff(got[:4096].astype(np.float64)) >= 0)                        # monotone over consecutive subnormals


def test_predict_scale_known_answers():
    ls = proj_ref.logf(F32(1.2))
    assert proj_ref.predict_scale(1.0, 2.0, 8, ls) == 0                                # ratio < 1: negative -> 0
    assert proj_ref.predict_scale(3.0, 3.0, 8, ls) == 0                                # ratio == 1: log = +0 -> ceil 0
    assert proj_ref.predict_scale(F32(1.2), 1.0, 8, ls) == 1                           # log(1.2f) / log(1.2f) = 1 exactly
    assert proj_ref.predict_scale(np.nextafter(F32(1.2), F32(2)), 1.0, 8, ls) == 2     # just above: the quotient exceeds 1
    assert proj_ref.predict_scale(1e30, 1.0, 8, ls) == 7                               # huge -> nlevels - 1
    assert proj_ref.predict_scale(1e30, 1.0, 3, ls) == 2
    assert proj_ref.predict_scale(1.0, 0.0, 8, ls) == 0                                # ratio inf: no int holds ceil(inf): INT_MIN -> 0


def _hand_view(**kw):
    sf, ls = synth.scale_tables(8, 1.2)
    a = dict(R=np.eye(3), t=np.zeros(3), Ow=np.zeros(3), cam=(100.0, 100.0, 50.0, 40.0), bounds=(0.0, 100.0, 0.0, 80.0), nlevels=8,
             log_scale=ls, scale_factors=sf, mbf=40.0)
    a.update(kw)
    return proj_ref.view(**a)


def _one(P, n=(0, 0, 1), minD=1.0, maxD=10.0, view=None, **kw):
    v = view or _hand_view()
    nin, (o,) = proj_ref.frustum(v, np.array([P], F32), np.array([n], F32), np.array([minD], F32), np.array([maxD], F32), **kw)
    return nin, {k: a[0] for k, a in o.items()}


def test_hand_derived_frustum_case():
    """identity pose, P = (0, 0, 5), fx = fy = 100, c = (50, 40), normal (0, 0, 1): uv = (50, 40), dist 5, cos 1;
    ratio = 10 / 5 = 2, log 2 / log 1.2 = 3.8 -> level 4, scale 1.2^4; projXR = 50 - 40 / 5 = 42"""
    nin, o = _one((0, 0, 5))
    assert nin == 1 and o["in_view"] == 1 and o["reason"] == 0
    assert tuple(o["proj_xy"]) == (50.0, 40.0)
    assert o["depth"] == 5.0 and o["view_cos"] == 1.0
    assert o["level"] == 4 and o["level_scale"] == synth.scale_tables(8, 1.2)[0][4]
    assert o["proj_xr"] == F32(50.0) - F32(40.0) * (F32(1.0) / F32(5.0))
    assert o["search"] == 1
    assert _one((0, 0, 5), far=True, th_far=4.0)[1]["search"] == 0                     # a far point stays in view, is not searched
    assert _one((0, 0, 5), far=True, th_far=4.0)[1]["in_view"] == 1
    assert _one((0, 0, 5), far=True, th_far=5.0)[1]["search"] == 1                     # "> thFarPoints"


@pytest.mark.parametrize("reason,kw", [
    (1, dict(P=(0, 0, 5), skip=np.array([1], np.uint8))),
    (2, dict(P=(0, 0, -1))),                       # behind the camera
    (3, dict(P=(10, 0, 5))),                       # u = 100 * 2 + 50 = 250 > 100
    (3, dict(P=(-10, 0, 5))),                      # u = -150 < 0
    (4, dict(P=(0, 10, 5))),                       # v = 240 > 80
    (5, dict(P=(0, 0, 5), maxD=1.0)),              # 5 > 1.2 * 1
    (5, dict(P=(0, 0, 5), minD=7.0)),              # 5 < 0.8 * 7
    (6, dict(P=(0, 0, 5), n=(0, 0, -1))),          # cos = -1 < 0.5
    (7, dict(P=(0, 0, 0))),                        # 0 / 0: the projection is NaN
])
def test_hand_derived_reject_reasons(reason, kw):
    nin, o = _one(**kw)
    assert nin == 0 and o["in_view"] == 0 and o["search"] == 0 and o["reason"] == reason and o["level"] == -1
    if reason in (1, 2, 3, 4, 7):
        assert tuple(o["proj_xy"]) == (-1.0, -1.0)
    else:
        assert tuple(o["proj_xy"]) == (50.0, 40.0)                                      # bounds passed: mTrackProjX/Y are written
    assert o["proj_xr"] == 0 and o["level_scale"] == 0
    assert o["view_cos"] == (-1.0 if reason == 6 else 0.0)
    if reason == 1:
        assert o["depth"] == 0                                                           # a skipped point is not touched at all
    elif reason != 7:
        assert o["depth"] > 0                                                            # cv::norm(Pc) precedes every test


def test_distance_gate_edges_are_inclusive():
    # dist == 1.2f * maxD and dist == 0.8f * minD pass ("<" and ">")
    maxD = F32(5.0) / F32(1.2)
    if F32(1.2) * maxD == F32(5.0):
        assert _one((0, 0, 5), maxD=maxD)[1]["reason"] == 0
    assert _one((0, 0, 4), minD=5.0)[1]["reason"] == (0 if F32(0.8) * F32(5.0) <= F32(4.0) else 5)


def test_akaze_tables_only_for_non_orb_points_of_a_mixed_view():
    ak = np.array([1.0, 1.5, 2.25], F32)
    mixed = _hand_view(ak_nlevels=3, ak_log_scale=proj_ref.logf(F32(1.5)), ak_scale_factors=ak)
    plain = _hand_view()
    P = np.array([(0, 0, 5)] * 2, F32); n = np.array([(0, 0, 1)] * 2, F32)
    minD = np.ones(2, F32); maxD = np.full(2, 50.0, F32)                               # ratio 10: ORB ceil(12.6) -> 7; AKAZE ceil(5.7) -> 2
    is_orb = np.array([1, 0], np.uint8)
    _, (o,) = proj_ref.frustum(mixed, P, n, minD, maxD, mp_is_orb=is_orb)
    assert o["level"].tolist() == [7, 2]
    assert o["level_scale"].tolist() == [float(synth.scale_tables(8, 1.2)[0][7]), 2.25]
    _, (o,) = proj_ref.frustum(plain, P, n, minD, maxD, mp_is_orb=is_orb)              # not a MixedFrame: ORB tables for every point
    assert o["level"].tolist() == [7, 7]
    _, (o,) = proj_ref.frustum(mixed, P, n, minD, maxD)                                # no flags: every point is an ORB point
    assert o["level"].tolist() == [7, 7]


# ---- mode A in numpy: float32 arithmetic, the double steps named in the issue ------------------------------------------------
def _np_gemm(R, X, t):
    out = np.empty_like(X)
    for i in range(3):
        tt = R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1] + R[i, 2] * X[:, 2]
        out[:, i] = (tt.astype(np.float64) * 1.0 + np.float64(t[i]) * 1.0).astype(F32)
    return out


def _np_norm(A):
    s = np.zeros(len(A))
    for i in range(3):
        v = A[:, i].astype(np.float64)
        s = s + v * v
    return np.sqrt(0 + s)


def _np_frustum(s, lim, mbf):
    R, t, Ow, P, Pn = s["R"], s["t"], s["Ow"], s["pos"], s["normal"]
    fx, fy, cx, cy = [F32(v) for v in s["cam"]]
    minX, maxX, minY, maxY = [F32(v) for v in s["bounds"]]
    M = len(P)
    with np.errstate(all="ignore"):
        Pc = _np_gemm(R, P, t)
        depth = _np_norm(Pc).astype(F32)
        z = Pc[:, 2]
        u = fx * Pc[:, 0] / z + cx
        v = fy * Pc[:, 1] / z + cy
        PO = P - Ow[None, :]
        dist = _np_norm(PO).astype(F32)
        dot = np.zeros(M)
        for i in range(3):
            dot = dot + PO[:, i].astype(np.float64) * Pn[:, i].astype(np.float64)
        cos = ((0.0 + dot) / dist.astype(np.float64)).astype(F32)
        ratio = s["max_dist"] / dist
        cf = np.ceil(proj_ref.logf_n(ratio) / F32(s["log_scale"]))
        ok = (cf >= F32(-2147483648.0)) & (cf < F32(2147483648.0))
        lvl = np.where(ok, np.where(ok, cf, 0).astype(np.int64), -2 ** 31)
        lvl = np.clip(lvl, 0, s["nlevels"] - 1).astype(np.int32)
        xr = u - F32(mbf) * (F32(1.0) / z)
    reason = np.zeros(M, np.uint8)
    for code, cond in ((6, cos < F32(lim)), (5, (dist < F32(0.8) * s["min_dist"]) | (dist > F32(1.2) * s["max_dist"])),
                       (4, (v < minY) | (v > maxY)), (3, (u < minX) | (u > maxX)), (7, ~(np.isfinite(u) & np.isfinite(v))), (2, z < 0)):
        reason[cond] = code
    iv = reason == 0
    bounds_ok = np.isin(reason, (0, 5, 6))
    o = dict(in_view=iv.astype(np.uint8), reason=reason, depth=depth)
    o["proj_xy"] = np.where(bounds_ok[:, None], np.stack([u, v], 1), F32(-1)).astype(F32)
    o["proj_xr"] = np.where(iv, xr, F32(0)).astype(F32)
    o["level"] = np.where(iv, lvl, -1).astype(np.int32)
    o["view_cos"] = np.where(np.isin(reason, (0, 6)), cos, F32(0)).astype(F32)
    o["level_scale"] = np.where(iv, s["scale_factors"][lvl], F32(0)).astype(F32)
    return o


def _scene_view(s, mbf=0.0, **kw):
    return proj_ref.view(s["R"], s["t"], s["Ow"], s["cam"], s["bounds"], s["nlevels"], s["log_scale"], s["scale_factors"], mbf=mbf, **kw)


@pytest.mark.parametrize("seed,M", [(7, 1000), (8, 4099)])
def test_mode_a_equals_the_numpy_restatement(seed, M):
    s = synth.map_scene(seed, M)
    nin, (got,) = proj_ref.frustum(_scene_view(s, mbf=35.0), s["pos"], s["normal"], s["min_dist"], s["max_dist"], cos_limit=0.5)
    want = _np_frustum(s, 0.5, 35.0)
    assert nin == int(want["in_view"].sum())
    for k, a in want.items():
        assert np.array_equal(got[k].view(np.uint8), a.view(np.uint8)), k
    if M == 1000:
        # the scene recipe: every outcome and every level often enough that a test over it cannot pass on an empty case
        cnt = np.bincount(got["reason"], minlength=8)
        assert all(cnt[r] >= 50 for r in (0, 2, 3, 4, 5, 6)), cnt
        lv = np.bincount(got["level"][got["in_view"] == 1], minlength=8)
        assert all(lv[:8] >= 5), lv


def test_mode_c_accepts_a_point_with_negative_depth():
    v = _hand_view()
    o = proj_ref.keyframe_points(v, np.array([(0, 0, -5), (0, 0, 5)], F32), np.ones(2, F32), np.full(2, 10.0, F32))
    assert o["valid"].tolist() == [1, 1]                                               # no depth-sign test (ORBmatcher.cc:2216-2223)
    assert o["uv"].tolist() == [[50.0, 40.0], [50.0, 40.0]] and o["level"].tolist() == [4, 4] and o["dist3d"].tolist() == [5.0, 5.0]
    nin, (a,) = proj_ref.frustum(v, np.array([(0, 0, -5)], F32), np.array([(0, 0, 1)], F32), np.ones(1, F32), np.full(1, 10.0, F32))
    assert nin == 0 and a["reason"][0] == 2                                            # mode A rejects the same point


def test_mode_b_hand_case():
    v = _hand_view()
    kps = np.zeros(4, proj_ref.KP_DTYPE); kps["octave"] = [0, 3, 2, 1]
    P = np.array([(0, 0, 5), (0, 0, -5), (10, 0, 5), (0, 0, 5)], F32)
    o = proj_ref.last_frame(v, P, kps, skip=np.array([0, 0, 0, 1], np.uint8), cam_r=(100.0, 100.0, 50.0, 40.0),
                            Trl=np.concatenate([np.eye(3).reshape(-1), [-1.0, 0.0, 0.0]]))
    assert o["valid"].tolist() == [1, 0, 0, 0]                                         # in view; invzc < 0; x bounds; skipped
    assert o["uv"][0].tolist() == [50.0, 40.0] and o["proj_ur"][0] == F32(50.0) - F32(40.0) * F32(1.0 / 5.0)
    assert o["uv_r"][0].tolist() == [30.0, 40.0]                                       # x3Dr = (-1, 0, 5): 100 * -1 / 5 + 50
    assert o["uv"][1:].tolist() == [[-1.0, -1.0]] * 3 and o["uv_r"][1:].tolist() == [[-1.0, -1.0]] * 3
    sf = synth.scale_tables(8, 1.2)[0]
    assert o["level_scale"].tolist() == [float(sf[0]), float(sf[3]), float(sf[2]), float(sf[1])]
