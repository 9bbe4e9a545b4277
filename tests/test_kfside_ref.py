"""The CPU restatement of the projector's KeyFrame-side modes (tests/kfside_ref): hand-derived known answers of modes D and E, the
exactness of the batched Fuse on a model map, and the new exports of the library.  No GPU."""
import ctypes as C
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfside_ref                                   # noqa: E402
import proj_ref                                     # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

F32 = np.float32
EYE = np.eye(3, dtype=F32)
ZERO = np.zeros(3, F32)
SF, LOGS = synth.scale_tables(8, 1.2)
NEW_EXPORTS = ("eorb_project_keyframe_side", "eorb_fuse_pose", "eorb_search_by_projection_kf_scw", "eorb_search_by_sim3", "eorb_fuse_keyframes")


def _view(mbf=0.0, size=200.0):
    """identity pose, fx = fy = 100, cx = cy = 100, image [0, size) x [0, size)"""
    return kfside_ref.view(EYE, ZERO, ZERO, (100.0, 100.0, 100.0, 100.0), (0.0, size, 0.0, size), 8, LOGS, SF, mbf=mbf)


def _d(P, Pn=None, min_dist=0.1, max_dist=10.0, th=3.0, mbf=0.0, size=200.0):
    P = np.asarray(P, F32).reshape(1, 3)
    Pn = (P / np.linalg.norm(P)).astype(F32) if Pn is None else np.asarray(Pn, F32).reshape(1, 3)
    o = kfside_ref.keyframe_side(_view(mbf, size), P, Pn, [min_dist], [max_dist], th)
    return {k: v[0] for k, v in o.items()}


# ---- known answers ------------------------------------------------------------------------------------------------------------------
def test_an_accepted_point_and_every_output():
    o = _d((0.5, -0.25, 2.0), max_dist=3.0, mbf=40.0)
    u = F32(100) * F32(0.5) / F32(2) + F32(100); v = F32(100) * F32(-0.25) / F32(2) + F32(100)
    dist = F32(np.sqrt(0.25 + 0.0625 + 4.0))
    lvl = proj_ref.predict_scale(3.0, dist, 8, LOGS)
    assert lvl == int(np.ceil(np.log(3.0 / float(dist)) / np.log(1.2))) == 3
    assert (o["valid"], o["reason"], o["level"]) == (1, 0, lvl)
    assert tuple(o["uv"]) == (u, v) == (F32(125), F32(87.5))
    assert o["dist3d"] == dist and o["radius"] == F32(3.0) * SF[lvl]
    assert o["q_ur"] == u - F32(40.0) * (F32(1) / F32(2)) == F32(105)


def test_a_point_on_maxX_is_outside_the_keyframe_and_inside_the_frame():
    """u = 100*1/1 + 100 = 200 = maxX: KeyFrame::IsInImage is strict above (reason 3), Frame::isInFrustum's bound is not"""
    P = np.array([[1.0, 0.0, 1.0]], F32); Pn = (P / np.sqrt(2.0)).astype(F32)
    o = kfside_ref.keyframe_side(_view(), P, Pn, [0.1], [10.0], 3.0)
    assert (o["valid"][0], o["reason"][0]) == (0, 3) and tuple(o["uv"][0]) == (-1.0, -1.0)
    _, (f,) = proj_ref.frustum(_view(), P, Pn, [0.1], [10.0], cos_limit=0.5)
    assert f["in_view"][0] == 1 and f["proj_xy"][0, 0] == F32(200.0)
    # just below maxX is inside; minX itself is inside
    inside = _d((0.9999, 0.0, 1.0))
    assert inside["valid"] == 1 and inside["uv"][0] < F32(200.0)
    assert _d((-1.0, 0.0, 1.0))["valid"] == 1 and _d((-1.0, 0.0, 1.0))["uv"][0] == F32(0.0)


def test_zero_depth_passes_the_depth_test_and_fails_the_image_test():
    for P in ((1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (-1.0, 1.0, 0.0)):                     # +inf, NaN, -inf / +inf
        o = _d(P, Pn=(0.0, 0.0, 1.0))
        assert (o["valid"], o["reason"]) == (0, 3), P
    assert _d((0.0, 0.0, -0.0), Pn=(0.0, 0.0, 1.0))["reason"] == 3                      # -0.0 < 0.0f is false
    assert _d((0.1, 0.1, -1e-3), Pn=(0.0, 0.0, 1.0))["reason"] == 2


def test_the_viewing_angle_is_compared_in_double():
    """PO = (1, 2, 2): dist3D = 3 exactly.  Pn = (-2^-30, 0.25, 0.5): PO.dot(Pn) = 1.5 - 2^-30 exactly in double, below 0.5*dist3D =
    1.5, so Fuse rejects; the quotient (1.5 - 2^-30)/3 rounds to 0.5f, which Frame::isInFrustum's float viewCos < 0.5 accepts."""
    PO = np.array([1.0, 2.0, 2.0], F32); Pn = np.array([-2.0 ** -30, 0.25, 0.5], F32)
    assert kfside_ref.angle_rejects(PO, Pn) == (True, False)
    o = _d(PO, Pn=Pn, size=400.0)
    assert (o["valid"], o["reason"], o["dist3d"]) == (0, 6, F32(3.0)) and tuple(o["uv"]) == (F32(150), F32(200))
    _, (f,) = proj_ref.frustum(_view(size=400.0), PO.reshape(1, 3), Pn.reshape(1, 3), [0.1], [10.0], cos_limit=0.5)
    assert f["in_view"][0] == 1 and f["view_cos"][0] == F32(0.5)
    # exactly on the limit and one step above it: accepted by both
    assert kfside_ref.angle_rejects(PO, np.array([0.0, 0.25, 0.5], F32)) == (False, False)
    assert kfside_ref.angle_rejects(PO, np.array([0.0, 0.25, 0.4999], F32)) == (True, True)


def test_distance_gates():
    assert _d((0.0, 0.0, 2.0), min_dist=2.6, max_dist=20.0)["reason"] == 5             # 2 < 0.8f * 2.6
    assert _d((0.0, 0.0, 2.0), min_dist=2.5, max_dist=20.0)["reason"] == 0             # 2 < 0.8f * 2.5 = 2 is false
    assert _d((0.0, 0.0, 2.0), min_dist=0.1, max_dist=1.6)["reason"] == 5              # 2 > 1.2f * 1.6 = 1.92
    sk = kfside_ref.keyframe_side(_view(), [[0, 0, 2.0]], [[0, 0, 1.0]], [0.1], [10.0], 3.0, skip=[1])
    assert (sk["valid"][0], sk["reason"][0], sk["level"][0], sk["radius"][0]) == (0, 1, -1, 0.0)


def test_mode_e_multiplies_by_invz_where_mode_d_divides():
    """x = 1, z = 3, fx = 100: mode D's camera.project gives 100*1/3 + 100, mode E's 100*(1*(float)(1.0/3)) + 100: one ulp apart"""
    P = np.array([[1.0, 0.0, 3.0]], F32)
    d = _d(P[0], Pn=(0.0, 0.0, 1.0))
    v = _view()
    e = kfside_ref.sim3_half(v, EYE, ZERO, (100.0, 100.0, 100.0, 100.0), v, P, [0.1], [10.0], 7.5)
    invz = F32(1.0 / np.float64(F32(3.0)))
    assert invz == F32(1) / F32(3)                                                      # the rounding from double changes nothing here
    ud = F32(100) * F32(1) / F32(3) + F32(100)
    ue = F32(100) * (F32(1) * invz) + F32(100)
    assert d["uv"][0] == ud and e["uv"][0, 0] == ue and e["valid"][0] == 1
    raw_d, raw_e = F32(100) * F32(1) / F32(3), F32(100) * (F32(1) * invz)
    assert raw_d != raw_e and abs(int(raw_d.view(np.uint32)) - int(raw_e.view(np.uint32))) == 1
    # mode E reads the camera-frame norm and has no viewing-angle test
    assert e["dist3d"][0] == F32(np.sqrt(10.0)) and e["reason"][0] == 0
    assert e["radius"][0] == F32(7.5) * SF[e["level"][0]]


def test_mode_e_chains_two_products_and_tests_the_second_depth():
    v = _view()
    sR = (F32(1.25) * EYE).astype(F32)
    P = np.array([[0.5, 0.25, 2.0], [0.5, 0.25, 2.0]], F32)
    e = kfside_ref.sim3_half(v, sR, np.array([0.0, 0.0, -3.0], F32), (100.0, 100.0, 100.0, 100.0), v, P, [0.1, 0.1], [10.0, 10.0], 7.5, skip=[0, 1])
    assert e["reason"].tolist() == [2, 1]                                              # 1.25*2 - 3 < 0
    e = kfside_ref.sim3_half(v, sR, np.array([0.0, 0.0, 1.5], F32), (100.0, 100.0, 100.0, 100.0), v, P[:1], [0.1], [10.0], 7.5)
    z = F32(1.25) * F32(2.0) + F32(1.5)
    invz = F32(1.0 / np.float64(z))
    assert e["uv"][0, 0] == F32(100) * (F32(0.625) * invz) + F32(100) and e["dist3d"][0] == F32(np.sqrt(0.625 ** 2 + 0.3125 ** 2 + 16.0))


# ---- the batch is exact: a model map ------------------------------------------------------------------------------------------------
TH_LOW = 50


class _Map:
    """the bookkeeping of MapPoint / KeyFrame that Fuse touches (src/ORBmatcher.cc:1581-1600, src/MapPoint.cc:160-330): observations,
    Replace with its descriptor recomputation, AddObservation / AddMapPoint"""

    def __init__(self, sc, seed):
        rng = np.random.default_rng(seed)
        self.sc = sc
        K, M = len(sc["kps"]), len(sc["pos"])
        self.bad = {m: False for m in range(M)}
        self.obs = {m: {} for m in range(M)}
        self.base = {m: int(rng.integers(0, 4)) for m in range(M)}                     # observations outside the neighbourhood
        self.desc = {m: sc["mp_desc"][m].copy() for m in range(M)}
        self.slots = [np.full(len(sc["kps"][k]), -1, np.int64) for k in range(K)]
        nxt = M
        for k in range(K):                                                           # other map points already in the keyframes
            for i in np.flatnonzero(rng.random(len(self.slots[k])) < 0.6):
                self.bad[nxt] = bool(rng.random() < 0.05); self.obs[nxt] = {k: int(i)}; self.base[nxt] = int(rng.integers(0, 5))
                self.desc[nxt] = sc["desc"][k][i].copy()
                self.slots[k][i] = nxt
                nxt += 1
        self.went_bad = 0

    def nobs(self, p):
        return len(self.obs[p]) + self.base[p]

    def compute_distinctive_descriptor(self, p):
        """the model's ComputeDistinctiveDescriptors: the descriptor of the observation in the first keyframe"""
        if self.obs[p]:
            k = min(self.obs[p])
            self.desc[p] = self.sc["desc"][k][self.obs[p][k]].copy()

    def replace(self, a, b):
        """a->Replace(b)"""
        if a == b:
            return
        obs = self.obs[a]; self.obs[a] = {}; self.bad[a] = True; self.went_bad += 1
        for k, i in obs.items():
            if k not in self.obs[b]:
                self.slots[k][i] = b; self.obs[b][k] = i
            else:
                self.slots[k][i] = -1
        self.base[b] += self.base[a]
        self.compute_distinctive_descriptor(b)

    def apply(self, k, m, best_idx, best_dist):
        """:1581-1600 -> 1 when the point counts as fused"""
        if best_dist > TH_LOW:
            return 0
        q = int(self.slots[k][best_idx])
        if q >= 0:
            if not self.bad[q]:
                if self.nobs(q) > self.nobs(m):
                    self.replace(m, q)
                else:
                    self.replace(q, m)
        else:
            self.obs[m][k] = int(best_idx); self.slots[k][best_idx] = m
        return 1

    def state(self):
        return ([s.tolist() for s in self.slots], dict(self.bad), {p: dict(o) for p, o in self.obs.items()},
                {p: d.tobytes() for p, d in self.desc.items()})


@functools.lru_cache(None)
def _toy():
    K, M = 4, 300
    sc = synth.keyframe_neighbourhood(31, K, M, n_kps=[400, 350, 0, 420], jitter=1.5)
    views = [kfside_ref.view(**kw) for kw in sc["views"]]
    proj = kfside_ref.keyframe_side(views, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], 3.0)
    return sc, {k: v.reshape((K, M) + v.shape[1:]) for k, v in proj.items()}


def _search(oracle, frames, sc, proj, k, ms, descs):
    """the oracle's radius match of points ms (with descriptors descs) in keyframe k, on the restatement's projection"""
    ms = np.asarray(ms, np.int64)
    if len(sc["kps"][k]) == 0:
        return np.full(len(ms), -1, np.int32), np.full(len(ms), 256, np.int32)
    p = {n: proj[n][k][ms] for n in ("valid", "uv", "radius", "level")}
    return oracle.kf_radius_match(frames[k], p["valid"], p["uv"], p["radius"], p["level"], np.ascontiguousarray(descs), inv_sigma2=sc["inv_sigma2"])


def test_the_batched_fuse_equals_the_sequential_fuse_on_a_model_map(oracle):
    sc, proj = _toy()
    K, M = proj["valid"].shape
    frames = [oracle.Frame(sc["kps"][k], sc["desc"][k], sc["W"], sc["H"]) if len(sc["kps"][k]) else None for k in range(K)]
    # the reference: keyframe by keyframe, point by point, every search with the map as it is at that moment
    seq = _Map(sc, 5)
    fused_seq = []
    for k in range(K):
        n = 0
        for m in range(M):
            if seq.bad[m] or k in seq.obs[m]:
                continue
            bi, bd = _search(oracle, frames, sc, proj, k, [m], [seq.desc[m]])
            n += seq.apply(k, m, int(bi[0]), int(bd[0]))
        fused_seq.append(n)
    # the adapter of eorb_fuse_keyframes: every (k, m) searched first, then applied in order with the re-tests
    bat = _Map(sc, 5)
    rows = [_search(oracle, frames, sc, proj, k, np.arange(M), sc["mp_desc"]) for k in range(K)]
    uploaded = {m: sc["mp_desc"][m].tobytes() for m in range(M)}
    fused_bat, refreshed, dropped = [], 0, 0
    for k in range(K):
        n = 0
        for m in range(M):
            if bat.bad[m] or k in bat.obs[m]:
                dropped += int(rows[k][1][m] <= TH_LOW)
                continue
            bi, bd = int(rows[k][0][m]), int(rows[k][1][m])
            if bat.desc[m].tobytes() != uploaded[m]:                                 # a Replace recomputed the descriptor: the row is stale
                r = _search(oracle, frames, sc, proj, k, [m], [bat.desc[m]])
                bi, bd = int(r[0][0]), int(r[1][0]); refreshed += 1
            n += bat.apply(k, m, bi, bd)
        fused_bat.append(n)
    assert fused_bat == fused_seq
    assert bat.state() == seq.state()
    # the scene exercises what the claim is about
    assert seq.went_bad >= 10 and sum(seq.bad[m] for m in range(M)) >= 10, (seq.went_bad, sum(seq.bad[m] for m in range(M)))
    assert dropped >= 5 and refreshed >= 1, (dropped, refreshed)
    assert sum(fused_seq) >= 60 and fused_seq[2] == 0, fused_seq


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_keyframe_side_entry_points():
    from eorb_slam_amd import _lib
    L = C.CDLL(_lib.build())
    for sym in NEW_EXPORTS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTS
    from eorb_slam_amd import frontend
    for name in ("ProjectKeyFrameSide", "FusePose", "SearchByProjectionKFScw", "SearchBySim3Pose", "FuseKeyFrames"):
        assert callable(getattr(frontend, name))
