"""The KannalaBrandt8 SearchForTriangulation oracle (tests/kb8tri/orc_kb8tri.c) behind ctypes, and the synthetic keyframe pairs
the KB8 tests share.

build(dirpath) compiles orc_kb8tri.c with oracle/Makefile's parity flags into dirpath (a pytest temporary directory), linked
against oracle/_build/liboracle.so (built by oracle_py.build()) for orc_tanf, orc_atan2f, orc_sinf_any, orc_cosf_any,
orc_descriptor_distance and orc_three_maxima."""
import ctypes as C
import os
import subprocess

import numpy as np

from eorb_slam_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
KP = synth.KP_DTYPE
CFLAGS = ["-O2", "-std=gnu11", "-fPIC", "-shared", "-Wall", "-ffp-contract=off", "-fno-fast-math"]   # oracle/Makefile


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Cam(C.Structure):
    _fields_ = [("model", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("k", C.c_float * 4), ("precision", C.c_float)]


def cam(c):
    """(fx, fy, cx, cy) -> Pinhole, (fx, fy, cx, cy, k0..k3) -> KannalaBrandt8 (precision 1e-6), as eorb_slam_amd._lib.camera"""
    o = Cam()
    o.fx, o.fy, o.cx, o.cy = [float(v) for v in c[:4]]
    if len(c) > 4:
        o.model = 1
        for i in range(4):
            o.k[i] = float(c[4 + i])
        o.precision = 1e-6
    return o


def cam_pair(cs):
    if np.ndim(cs[0]) == 0:
        cs = (cs, cs)
    a = (Cam * 2)()
    a[0], a[1] = cam(cs[0]), cam(cs[-1])
    return a


class KB8TriOracle:
    def __init__(self, dirpath, oracle_py):
        oracle_py.build()
        libdir = os.path.join(ROOT, "oracle", "_build")
        out = os.path.join(str(dirpath), "liborc_kb8tri.so")
        cc = os.environ.get("CC", "gcc")
        subprocess.run([cc] + CFLAGS + ["-o", out, os.path.join(HERE, "orc_kb8tri.c"), os.path.join(libdir, "liboracle.so"),
                                        "-Wl,-rpath," + libdir, "-lm"], check=True)
        self.L = L = C.CDLL(out)
        vp, ci, cf = C.c_void_p, C.c_int, C.c_float
        L.orc_kt_svd4.argtypes = [vp, vp, vp]
        L.orc_kt_triangulate_matches.restype = cf
        L.orc_kt_triangulate_matches.argtypes = [vp, vp, vp, vp, vp, vp, cf, cf, vp]
        L.orc_kt_triangulate_batch.argtypes = [vp, vp, vp, vp, vp, ci, vp, vp, vp]
        L.orc_kt_unproject.argtypes = [vp, cf, cf, vp]
        L.orc_kt_project.argtypes = [vp, vp, vp, vp]
        L.orc_kt_search_for_triangulation.restype = ci
        L.orc_kt_search_for_triangulation.argtypes = [vp, ci, ci, vp, ci, vp, vp, vp, vp, ci, vp, ci, ci, vp, ci, vp, vp, vp, vp, ci,
                                                      vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]

    def svd4(self, A):
        A = np.ascontiguousarray(A, np.float32).reshape(16)
        W = np.zeros(4, np.float64); Vt = np.zeros(16, np.float32)
        self.L.orc_kt_svd4(_p(A), _p(W), _p(Vt))
        return W, Vt.reshape(4, 4)

    def unproject(self, c, x, y):
        r = np.zeros(3, np.float32)
        cc = cam(c)
        self.L.orc_kt_unproject(C.byref(cc), float(x), float(y), _p(r))
        return r

    def project(self, c, p):
        p = np.ascontiguousarray(p, np.float32); u = C.c_float(); v = C.c_float()
        cc = cam(c)
        self.L.orc_kt_project(C.byref(cc), _p(p), C.byref(u), C.byref(v))
        return np.float32(u.value), np.float32(v.value)

    def triangulate_matches(self, cam1, cam2, kp1, kp2, R12, t12, sigma1, sigma2):
        k1 = np.ascontiguousarray([kp1], KP); k2 = np.ascontiguousarray([kp2], KP)
        R = np.ascontiguousarray(R12, np.float32).reshape(9); t = np.ascontiguousarray(t12, np.float32).reshape(3)
        x = np.zeros(3, np.float32)
        c1, c2 = cam(cam1), cam(cam2)
        z = self.L.orc_kt_triangulate_matches(C.byref(c1), C.byref(c2), _p(k1), _p(k2), _p(R), _p(t), float(sigma1), float(sigma2), _p(x))
        return np.float32(z), x

    def triangulate_batch(self, cam1, cam2, Rt, kps1, kps2, sigma2_1, sigma2_2):
        k1 = np.ascontiguousarray(kps1, KP); k2 = np.ascontiguousarray(kps2, KP)
        rt = np.ascontiguousarray(np.asarray(Rt, np.float32).reshape(12))
        s1 = np.ascontiguousarray(sigma2_1, np.float32); s2 = np.ascontiguousarray(sigma2_2, np.float32)
        out = np.zeros(len(k1), np.float32)
        c1, c2 = cam(cam1), cam(cam2)
        self.L.orc_kt_triangulate_batch(C.byref(c1), C.byref(c2), _p(rt), _p(k1), _p(k2), len(k1), _p(s1), _p(s2), _p(out))
        return out

    def search(self, kps1, nleft1, desc1, elig1, fv1, kps2, nleft2, desc2, elig2, fv2, cams1, cams2, Rt, ep, scale2, sigma2_1,
               sigma2_2, coarse=False, checkOri=True):
        k1 = np.ascontiguousarray(kps1, KP); k2 = np.ascontiguousarray(kps2, KP)
        d1 = np.ascontiguousarray(desc1, np.uint8); d2 = np.ascontiguousarray(desc2, np.uint8)
        e1 = np.ascontiguousarray(elig1, np.uint8); e2 = np.ascontiguousarray(elig2, np.uint8)
        n1, o1, i1 = [np.ascontiguousarray(a, t) for a, t in zip(fv1, (np.uint32, np.int32, np.int32))]
        n2, o2, i2 = [np.ascontiguousarray(a, t) for a, t in zip(fv2, (np.uint32, np.int32, np.int32))]
        rt = np.zeros(48, np.float32); r = np.asarray(Rt, np.float32).reshape(-1); rt[:len(r)] = r
        ep = np.ascontiguousarray(ep, np.float32); sc = np.ascontiguousarray(scale2, np.float32)
        s1 = np.ascontiguousarray(sigma2_1, np.float32); s2 = np.ascontiguousarray(sigma2_2, np.float32)
        m = np.full(len(k1), -1, np.int32)
        c1, c2 = cam_pair(cams1), cam_pair(cams2)
        n = self.L.orc_kt_search_for_triangulation(_p(k1), len(k1), int(nleft1), _p(d1), d1.shape[1], _p(e1), _p(n1), _p(o1), _p(i1), len(n1),
                                                   _p(k2), len(k2), int(nleft2), _p(d2), d2.shape[1], _p(e2), _p(n2), _p(o2), _p(i2), len(n2),
                                                   c1, c2, _p(rt), _p(ep), _p(sc), _p(s1), _p(s2), int(coarse), int(checkOri), _p(m))
        return n, m


# ---- synthetic inputs ---------------------------------------------------------------------------------------------------------
# KB8 parameters chosen for the tests (a 346 x 260 event camera and a 512 x 512 fisheye pair), not taken from any configuration
CAM_MONO = (226.0, 226.5, 172.0, 131.0, -0.02, 0.004, -0.001, 0.0002)
CAM_L = (190.5, 190.2, 254.9, 256.8, 0.0034, 0.0007, -0.0021, 0.0003)
CAM_R = (190.1, 189.9, 256.2, 255.1, 0.0030, 0.0011, -0.0018, 0.0002)
NLEV, SCALE = 8, 1.2


def level_tables(nlev=NLEV, sf=SCALE):
    s = [np.float32(1.0)]
    for _ in range(1, nlev):
        s.append(np.float32(s[-1] * np.float32(sf)))
    s = np.array(s, np.float32)
    return s, (s * s).astype(np.float32)


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float32)


def rel_pose(Ra, ta, Rb, tb):
    """R12, t12 of camera a (1) w.r.t. camera b (2): R1w R2w^T, -R1w R2w^T t2w + t1w (float rows, computed in float64 then rounded)"""
    R = (Ra.astype(np.float64) @ Rb.T.astype(np.float64)).astype(np.float32)
    t = (-(R.astype(np.float64) @ tb.astype(np.float64)) + ta).astype(np.float32)
    return np.concatenate([R.reshape(9), t]).astype(np.float32)


def project_np(c, P):
    """KB8 / Pinhole projection in float64 (test-data generation only; the oracle's float path decides every outcome)"""
    P = np.asarray(P, np.float64)
    if len(c) == 4:
        return np.stack([c[0] * P[:, 0] / P[:, 2] + c[2], c[1] * P[:, 1] / P[:, 2] + c[3]], axis=1)
    th = np.arctan2(np.hypot(P[:, 0], P[:, 1]), P[:, 2]); psi = np.arctan2(P[:, 1], P[:, 0])
    r = th + c[4] * th ** 3 + c[5] * th ** 5 + c[6] * th ** 7 + c[7] * th ** 9
    return np.stack([c[0] * r * np.cos(psi) + c[2], c[1] * r * np.sin(psi) + c[3]], axis=1)


def _flip(d, nbits, rng):
    d = d.copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def feature_vector_of(node_of, rng):
    """DBoW2::FeatureVector as CSR from a node id per feature (inside a node: shuffled insertion order)"""
    ids = np.unique(node_of)
    off = [0]; idx = []
    for nid in ids:
        m = np.nonzero(node_of == nid)[0]; rng.shuffle(m); idx.extend(m.tolist()); off.append(len(idx))
    return ids.astype(np.uint32), np.array(off, np.int32), np.array(idx, np.int32)


def scene(seed=0, twocam=False, npts=600, ndistract=150, nties=30, stride=32, nnodes=60, size=None, ep_near=True):
    """A keyframe pair seeing one 3D scene.  Returns a dict of the matcher's inputs (kps / nleft / desc / elig / fv per keyframe,
    cams, Rt, ep, scale2, sigma2).  True observations carry near-duplicate descriptors (<= 10 flipped bits); distractors copy a
    point's descriptor with 12-30 flipped bits at a random position (pass Hamming, fail geometry); ties copy an observation of
    pKF2 with its exact descriptor 0.2-1.5 px away.  stride 61: Mixed rows, ~15 % of them non-ORB (elig 0: the type gate)."""
    rng = np.random.default_rng(seed)
    scale, sigma2 = level_tables()
    if twocam:
        W = H = 512 if size is None else size
        cams = (CAM_L, CAM_R)
        Rrl, trl = rot(0.002, -0.01, 0.003), np.array([-0.11, 0.001, 0.002], np.float32)   # right camera w.r.t. left
    else:
        W, H = (346, 260) if size is None else size
        cams = (CAM_MONO,)
        Rrl, trl = None, None
    R1, t1 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    R2 = rot(0.03, -0.08, 0.02); t2 = np.array([-0.35, 0.04, 0.06], np.float32)
    poses = {(0, 0): (R1, t1), (1, 0): (R2, t2)}
    if twocam:
        poses[(0, 1)] = ((Rrl.astype(np.float64) @ R1).astype(np.float32), (Rrl.astype(np.float64) @ t1 + trl).astype(np.float32))
        poses[(1, 1)] = ((Rrl.astype(np.float64) @ R2).astype(np.float32), (Rrl.astype(np.float64) @ t2 + trl).astype(np.float32))
    z = rng.uniform(1.5, 9.0, npts)
    X = np.stack([rng.uniform(-1.1, 1.1, npts) * z, rng.uniform(-0.9, 0.9, npts) * z, z], axis=1)
    base = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    node = rng.integers(0, nnodes, npts) * 7 + 3
    ang = rng.uniform(0, 360, npts)
    ncam = 2 if twocam else 1
    kf = []
    for k in range(2):
        blocks = []
        for cidx in range(ncam):
            R, t = poses[(k, cidx)]
            Pc = X @ R.T.astype(np.float64) + t
            uv = project_np(cams[cidx], Pc)
            vis = (Pc[:, 2] > 0.2) & (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)
            vis &= rng.uniform(size=npts) < 0.9
            pid = np.nonzero(vis)[0]
            rows = []
            for p in pid:
                rows.append((uv[p, 0] + rng.normal(0, 0.4), uv[p, 1] + rng.normal(0, 0.4), p, _flip(base[p], rng.integers(0, 11), rng)))
            for _ in range(ndistract // ncam):
                p = rng.integers(npts)
                rows.append((rng.uniform(0, W), rng.uniform(0, H), p, _flip(base[p], rng.integers(12, 31), rng)))
            if k == 1:
                for j in rng.choice(len(pid), min(nties // ncam, len(pid)), replace=False):
                    x, y, p, d = rows[j]
                    rows.append((x + rng.uniform(-1.5, 1.5), y + rng.uniform(-1.5, 1.5), p, d.copy()))
            order = rng.permutation(len(rows))
            blocks.append([rows[i] for i in order])
        allrows = [r for b in blocks for r in b]
        n = len(allrows)
        kps = np.zeros(n, KP)
        kps["x"] = np.array([r[0] for r in allrows], np.float32); kps["y"] = np.array([r[1] for r in allrows], np.float32)
        kps["octave"] = rng.integers(0, 4, n); kps["size"] = 31.0; kps["class_id"] = -1
        pids = np.array([r[2] for r in allrows])
        a = ang[pids] + (rng.normal(0, 4, n) if k else 0) + np.where(rng.uniform(size=n) < 0.1, rng.uniform(0, 360, n), 0)
        kps["angle"] = np.mod(a, 360).astype(np.float32)
        desc = np.zeros((n, stride), np.uint8)
        desc[:, :32] = np.stack([r[3] for r in allrows])
        if stride > 32:
            desc[:, 32:] = rng.integers(0, 256, (n, stride - 32), dtype=np.uint8)
        elig = (rng.uniform(size=n) < 0.85).astype(np.uint8)
        if stride > 32:
            elig[rng.uniform(size=n) < 0.15] = 0                         # non-ORB rows of a Mixed keyframe
        if not twocam:
            elig |= ((rng.uniform(size=n) < 0.1) << 1).astype(np.uint8) & (elig << 1)
        nodes = node[pids].copy()
        nodes[rng.uniform(size=n) < 0.05] = 1                              # a node the other keyframe may lack
        fv = feature_vector_of(nodes, rng)
        kf.append(dict(kps=kps, nleft=len(blocks[0]) if twocam else -1, desc=desc, elig=elig, fv=fv))
    if twocam:
        Rt = np.concatenate([rel_pose(*poses[(0, a)], *poses[(1, b)]) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1))])
    else:
        Rt = rel_pose(R1, t1, R2, t2)
    k2 = kf[1]["kps"]
    ep = (k2["x"][0] + 4.0, k2["y"][0]) if ep_near else (-1000.0, -1000.0)
    camsp = cams if twocam else cams[0]
    return dict(kps1=kf[0]["kps"], nleft1=kf[0]["nleft"], desc1=kf[0]["desc"], elig1=kf[0]["elig"], fv1=kf[0]["fv"],
                kps2=kf[1]["kps"], nleft2=kf[1]["nleft"], desc2=kf[1]["desc"], elig2=kf[1]["elig"], fv2=kf[1]["fv"],
                cams1=camsp, cams2=camsp, Rt=Rt, ep=np.array(ep, np.float32), scale2=scale, sigma2_1=sigma2, sigma2_2=sigma2)
