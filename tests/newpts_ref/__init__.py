"""Loader of the CPU restatement of CreateNewMapPoints' per-match half (newpts_ref.c, beside this file: the sequential double loop),
compiled with the host C compiler into a temporary directory when first used, strict IEEE; and two models of it in Python:

    pair_model / loop_model   the same arithmetic written a second time, in numpy scalars (float32 operations one at a time, the double
                              steps in float64), with the loop's rules in plain Python and one named wrong variant per comparison
                              (VARIANTS).  The restatement must equal it exactly.
    pair_f64                  one pair in float64 with numpy's SVD and plain formulas: what the float arithmetic approximates.

Test infrastructure: nothing under eorb_slam_amd/ imports it.  The cameras, the 4x4 Jacobi SVD and the float atan2 / cos are the oracle's
(orc_camera_unproject / _project, orc_svd4, orc_atan2f, orc_cosf), handed to the restatement as function pointers (as tests/proj_ref
does) and called by the Python model through oracle_py."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-std=c99", "-Wall", "-Wno-unused-function"]
STATUS = ("new", "no_match", "claimed", "type", "parallax", "w_zero", "empty_stereo", "z1", "z2", "reproj1", "reproj2", "zero_dist", "far",
          "scale", "nonfinite")
S = {n: i for i, n in enumerate(STATUS)}
LOCAL_MAPPING, TRACKING = 0, 1
# one wrong comparison (or rule) each; tests/test_newpts_ref.py names the scene that rejects it
VARIANTS = ("parallax_le_float", "cos_ge_0", "z1_lt", "z2_lt", "chi1_ge", "chi2_ge", "far_gt", "scale_low_le", "scale_high_ge",
            "stereo_two_ifs", "mbf2_repaired", "ratio_reset_per_neighbour", "ratio_reset_per_pair", "claim_ignored", "unproject_stereo_undistorted")
# A float cosParallaxRays never equals the double 0.9998, so "<" and "<=" against the double agree on every input; the nearest wrong
# reading that an input can show is the float comparison "<= 0.9998f" (parallax_le_float), rejected by the pair whose cosine is 0.9998f.
# 5.991 * sigma2 in double equals a float error only in special cases; the exact scene has one (error 0 against sigma2 0).

_libs = {}


def lib(timing=False):
    """the strict build the tests compare with; timing=True: the same source with -O3 -march=native (still -ffp-contract=off, same
    results), what tools/newpts_latency.py times"""
    if timing in _libs:
        return _libs[timing]
    tmp = tempfile.mkdtemp(prefix="newpts_ref_")
    atexit.register(shutil.rmtree, tmp, True)
    so = os.path.join(tmp, "libnewpts_ref.so")
    flags = (["-O3", "-march=native"] + CFLAGS[1:]) if timing else CFLAGS
    subprocess.check_call([os.environ.get("CC", "gcc")] + flags + [os.path.join(_HERE, "newpts_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    L.pr_set_project.restype = None; L.pr_set_project.argtypes = [vp]
    L.npr_set_fns.restype = None; L.npr_set_fns.argtypes = [vp, vp, vp, vp]
    L.npr_loop.restype = None; L.npr_loop.argtypes = [vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp]
    L.npr_pairs.restype = None; L.npr_pairs.argtypes = [vp, vp, ci, vp, vp, ci, vp, vp, vp, vp]
    from oracle import oracle_py
    O = oracle_py.lib(fast=timing)
    cast = lambda f: C.cast(f, C.c_void_p)      # noqa: E731
    L.pr_set_project(cast(O.orc_camera_project))
    L.npr_set_fns(cast(O.orc_camera_unproject), cast(O.orc_svd4), cast(O.orc_atan2f), cast(O.orc_cosf))
    _libs[timing] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def args(sc, aids=True):
    """a scene (tests/newpts_ref/scenes.py) -> frontend.NewPointsArgs: the record both the library and the restatement read"""
    from eorb_slam_amd import frontend as fe
    dummy = dict(bounds=(0, 1, 0, 1), nlevels=len(sc["level_scale"]), log_scale=0.0, scale_factors=sc["level_scale"])
    mk = lambda v: fe.view(v["R"], v["t"], v["Ow"], v["cam"], mbf=v.get("mbf", 0.0), **dummy)      # noqa: E731
    v1 = [mk(v) for v in sc["views1"]]
    v2 = [[mk(v) for v in vs] for vs in sc["views2"]]
    return fe.NewPointsArgs(sc["K"], sc["n1"], v1, v2, **params(sc), aids=aids)


def params(sc):
    """the keyword arguments of frontend.NewPointsArgs / NewMapPoints for a scene"""
    return dict(form=sc["form"], nleft1=sc["nleft1"], nleft2=sc["nleft2"], mb1=sc["mb1"], mb2=sc["mb2"], side1=sc["side1"], side2=sc["side2"],
                level_scale=sc["level_scale"], level_sigma2=sc["level_sigma2"], ratio_factor_orb=sc["rf_orb"], ratio_factor_ak=sc["rf_ak"],
                far_points=sc["far_points"], th_far_points=sc["th_far"])


def views(sc):
    from eorb_slam_amd import frontend as fe
    dummy = dict(bounds=(0, 1, 0, 1), nlevels=len(sc["level_scale"]), log_scale=0.0, scale_factors=sc["level_scale"])
    mk = lambda v: fe.view(v["R"], v["t"], v["Ow"], v["cam"], mbf=v.get("mbf", 0.0), **dummy)      # noqa: E731
    return [mk(v) for v in sc["views1"]], [[mk(v) for v in vs] for vs in sc["views2"]]


def loop(sc, timing=False, A=None):
    """the restatement on a scene -> dict as frontend.NewMapPoints returns it"""
    A = A or args(sc)
    has = np.zeros(max(sc["n1"], 1), np.uint8)
    m = np.ascontiguousarray(sc["match12"], np.int32)
    lib(timing).npr_loop(C.byref(A.P), _p(sc["kps1"]), sc["n1"], _p(sc["kps2"]), _p(sc["kf_off"]), sc["K"], _p(m), _p(A.status), _p(A.x3d), _p(A.branch),
                         _p(A.cos_parallax), _p(A.n_new), _p(has))
    return A.out()


def pairs(sc):
    """every matched pair on its own under both factors -> (st (K, n1, 2), ak (K, n1), x3d (K, n1, 3))"""
    A = args(sc)
    K, n1 = sc["K"], sc["n1"]
    st = np.zeros((K, n1, 2), np.uint8); ak = np.zeros((K, n1), np.uint8); x = np.zeros((K, n1, 3), np.float32)
    m = np.ascontiguousarray(sc["match12"], np.int32)
    lib().npr_pairs(C.byref(A.P), _p(sc["kps1"]), n1, _p(sc["kps2"]), _p(sc["kf_off"]), K, _p(m), _p(st), _p(ak), _p(x))
    return st, ak, x


# ---- the second writing of the arithmetic: numpy scalars, one IEEE operation at a time ------------------------------------------------
f32, f64 = np.float32, np.float64
_ONE, _ZERO = f32(1), f32(0)


def _gemm(R, x, c=None):
    """OpenCV's small gemm, d_size.width == 1: the products summed in float, then (float)(t*1 + c*1) in double"""
    out = np.zeros(3, f32)
    for i in range(3):
        t = f32(f32(f32(R[3 * i] * x[0]) + f32(R[3 * i + 1] * x[1])) + f32(R[3 * i + 2] * x[2]))
        out[i] = f32(f64(t) * f64(1.0) + (f64(c[i]) * f64(1.0) if c is not None else f64(0.0)))
    return out


def _dot(a, b):
    s = f64(0)
    for i in range(3):
        s = s + f64(a[i]) * f64(b[i])
    return f64(0.0) + s


def _norm(a):
    s = f64(0)
    for i in range(3):
        s = s + f64(a[i]) * f64(a[i])
    return np.sqrt(f64(0) + s)


def _a_row(p, r2, rj):
    out = np.zeros(4, f32)
    for k in range(4):
        out[k] = f32(r2[k] - rj[k]) if f64(p) == 1.0 else f32(f64(r2[k]) * f64(p) + f64(rj[k]) * f64(-1.0) + f64(0.0))
    return out


def _cam(v):
    return tuple(float(x) for x in v["cam"])


def pair_model(sc, k, idx1, idx2, ratioFactor, variant=None):
    """one pair -> (status, branch, cosParallaxRays, x3d or None), with `variant` (one of VARIANTS that lives in the pair) applied"""
    from oracle import oracle_py as orc
    O = orc.lib()
    with np.errstate(all="ignore"):
        lm = sc["form"] == LOCAL_MAPPING
        twocam = lm and sc["nleft1"] >= 0
        g2 = int(sc["kf_off"][k]) + idx2
        r1 = int(twocam and idx1 >= sc["nleft1"]); r2 = int(twocam and idx2 >= sc["nleft2"][k])
        V1, V2 = sc["views1"][r1], sc["views2"][k][r2]
        KF1, KF2 = sc["views1"][0], sc["views2"][k][0]
        R1, t1, Ow1 = [np.asarray(V1[n], f32).reshape(-1) for n in ("R", "t", "Ow")]
        R2, t2, Ow2 = [np.asarray(V2[n], f32).reshape(-1) for n in ("R", "t", "Ow")]
        c1, c2 = [f32(x) for x in V1["cam"][:4]], [f32(x) for x in V2["cam"][:4]]
        kc1, kc2 = [f32(x) for x in KF1["cam"][:4]], [f32(x) for x in KF2["cam"][:4]]
        k1x, k1y = f32(sc["kps1"]["x"][idx1]), f32(sc["kps1"]["y"][idx1])
        k2x, k2y = f32(sc["kps2"]["x"][g2]), f32(sc["kps2"]["y"][g2])
        s1, s2 = sc["side1"], sc["side2"]
        ur1 = f32(s1["uright"][idx1]) if s1.get("uright") is not None else f32(-1)
        ur2 = f32(s2["uright"][g2]) if s2.get("uright") is not None else f32(-1)
        st1 = bool(not twocam and ur1 >= 0); st2 = bool(not twocam and ur2 >= 0)
        if lm:
            xn1 = orc.unproject(_cam(V1), k1x, k1y); xn2 = orc.unproject(_cam(V2), k2x, k2y)
        else:
            xn1 = np.array([f32(k1x - c1[2]) * f32(_ONE / c1[0]), f32(k1y - c1[3]) * f32(_ONE / c1[1]), _ONE], f32)
            xn2 = np.array([f32(k2x - c2[2]) * f32(_ONE / c2[0]), f32(k2y - c2[3]) * f32(_ONE / c2[1]), _ONE], f32)
        Rwc1 = R1.reshape(3, 3).T.reshape(-1).copy(); Rwc2 = R2.reshape(3, 3).T.reshape(-1).copy()
        ray1, ray2 = _gemm(Rwc1, xn1), _gemm(Rwc2, xn2)
        cosr = f32(_dot(ray1, ray2) / (_norm(ray1) * _norm(ray2)))

        def cos_stereo(mb, depth):
            a = f32(f32(2) * f32(O.orc_atan2f(f32(f32(mb) / f32(2)), f32(depth))))
            return f32(O.orc_cosf(a))
        cs = f32(cosr + _ONE); cs1 = cs; cs2 = cs
        if st1:
            cs1 = cos_stereo(sc["mb1"], s1["depth"][idx1])
        if st2 and (variant == "stereo_two_ifs" or not st1):
            cs2 = cos_stereo(sc["mb2"][k] if sc["mb2"] is not None else 0.0, s2["depth"][g2])
        cs = cs2 if cs2 < cs1 else cs1
        below = (cosr <= f32(0.9998)) if variant == "parallax_le_float" else (f64(cosr) < 0.9998)
        pos = (cosr >= 0) if variant == "cos_ge_0" else (cosr > 0)

        def unproject_stereo(V, Rwc, side, i, kx, ky):
            z = f32(side["depth"][i])
            if not z > 0:
                return None
            raw = side.get("raw_xy")
            u, v = (f32(raw[i][0]), f32(raw[i][1])) if raw is not None and variant != "unproject_stereo_undistorted" else (kx, ky)
            cam = [f32(x) for x in V["cam"][:4]]
            x = f32(f32(f32(u - cam[2]) * z) * f32(_ONE / cam[0])); y = f32(f32(f32(v - cam[3]) * z) * f32(_ONE / cam[1]))
            return _gemm(Rwc, np.array([x, y, z], f32), np.asarray(V["Ow"], f32).reshape(-1))
        if cosr < cs and pos and (st1 or st2 or below):
            T1 = np.concatenate([R1.reshape(3, 3), t1.reshape(3, 1)], axis=1); T2 = np.concatenate([R2.reshape(3, 3), t2.reshape(3, 1)], axis=1)
            A = np.stack([_a_row(xn1[0], T1[2], T1[0]), _a_row(xn1[1], T1[2], T1[1]), _a_row(xn2[0], T2[2], T2[0]), _a_row(xn2[1], T2[2], T2[1])])
            _, Vt = orc.svd4(A)
            branch = 1
            if Vt[3, 3] == 0:
                return S["w_zero"], branch, cosr, None
            scl = f32(f64(1.0) / f64(Vt[3, 3]))
            x3d = np.array([f32(f32(Vt[3, i] * scl) + _ZERO) for i in range(3)], f32)
        elif st1 and cs1 < cs2:
            branch = 2
            x3d = unproject_stereo(V1, Rwc1, s1, idx1, k1x, k1y)
        elif st2 and cs2 < cs1:
            branch = 3
            x3d = unproject_stereo(V2, Rwc2, s2, g2, k2x, k2y)
        else:
            return S["parallax"], 0, cosr, None
        if x3d is None:
            return S["empty_stereo"], branch, cosr, None
        if not np.all(np.isfinite(x3d)):
            return S["nonfinite"], branch, cosr, None
        z1 = f32(_dot(R1[6:9], x3d) + f64(t1[2]))
        if not np.isfinite(z1):
            return S["nonfinite"], branch, cosr, None
        if (z1 < 0) if variant == "z1_lt" else (z1 <= 0):
            return S["z1"], branch, cosr, None
        z2 = f32(_dot(R2[6:9], x3d) + f64(t2[2]))
        if not np.isfinite(z2):
            return S["nonfinite"], branch, cosr, None
        if (z2 < 0) if variant == "z2_lt" else (z2 <= 0):
            return S["z2"], branch, cosr, None
        oc1, oc2 = int(sc["kps1"]["octave"][idx1]), int(sc["kps2"]["octave"][g2])
        sg1 = f32(s1["kp_sigma2"][idx1]) if s1.get("kp_sigma2") is not None else f32(sc["level_sigma2"][oc1])
        sg2 = f32(s2["kp_sigma2"][g2]) if s2.get("kp_sigma2") is not None else f32(sc["level_sigma2"][oc2])
        mbf1 = f32(KF1.get("mbf", 0.0))

        def gate(V, R, t, z, stereo, kx, ky, ur, kc, mbf, sg, which):
            x = f32(_dot(R[0:3], x3d) + f64(t[0])); y = f32(_dot(R[3:6], x3d) + f64(t[1]))
            invz = f32(f64(1.0) / f64(z))
            if not stereo:
                if lm:
                    u, v = orc.project(_cam(V), np.array([x, y, z], f32))
                else:
                    u = f32(f32(f32(kc[0] * x) * invz) + kc[2]); v = f32(f32(f32(kc[1] * y) * invz) + kc[3])
                ex, ey = f32(u - kx), f32(v - ky)
                e = f32(f32(ex * ex) + f32(ey * ey)); coef = 5.991
            else:
                u = f32(f32(f32(kc[0] * x) * invz) + kc[2]); u_r = f32(u - f32(mbf * invz)); v = f32(f32(f32(kc[1] * y) * invz) + kc[3])
                ex, ey, er = f32(u - kx), f32(v - ky), f32(u_r - ur)
                e = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er)); coef = 7.8
            if not np.isfinite(e):
                return S["nonfinite"]
            lim = f64(coef) * f64(sg)
            return S["reproj%d" % which] if ((f64(e) >= lim) if variant == "chi%d_ge" % which else (f64(e) > lim)) else 0
        rc = gate(V1, R1, t1, z1, st1, k1x, k1y, ur1, kc1, mbf1, sg1, 1)
        if rc:
            return rc, branch, cosr, None
        mbf2 = f32(KF2.get("mbf", 0.0)) if variant == "mbf2_repaired" else mbf1
        rc = gate(V2, R2, t2, z2, st2, k2x, k2y, ur2, kc2, mbf2, sg2, 2)
        if rc:
            return rc, branch, cosr, None
        dist1 = f32(_norm(np.array([f32(x3d[i] - Ow1[i]) for i in range(3)], f32)))
        dist2 = f32(_norm(np.array([f32(x3d[i] - Ow2[i]) for i in range(3)], f32)))
        if not (np.isfinite(dist1) and np.isfinite(dist2)):
            return S["nonfinite"], branch, cosr, None
        if dist1 == 0 or dist2 == 0:
            return S["zero_dist"], branch, cosr, None
        th = f32(sc["th_far"])
        if lm and sc["far_points"] and ((dist1 > th or dist2 > th) if variant == "far_gt" else (dist1 >= th or dist2 >= th)):
            return S["far"], branch, cosr, None
        ratioDist = f32(dist2 / dist1)
        sc1 = f32(s1["kp_scale"][idx1]) if s1.get("kp_scale") is not None else f32(sc["level_scale"][oc1])
        sc2 = f32(s2["kp_scale"][g2]) if s2.get("kp_scale") is not None else f32(sc["level_scale"][oc2])
        ratioOctave = f32(sc1 / sc2)
        rf = f32(ratioFactor)
        lo = f32(ratioDist * rf); hi = f32(ratioOctave * rf)
        low = (lo <= ratioOctave) if variant == "scale_low_le" else (lo < ratioOctave)
        high = (ratioDist >= hi) if variant == "scale_high_ge" else (ratioDist > hi)
        if low or high:
            return S["scale"], branch, cosr, None
        return S["new"], branch, cosr, x3d


def loop_model(sc, variant=None):
    """the loop in plain Python over pair_model -> dict(status, x3d, branch, cos_parallax, n_new)"""
    K, n1 = sc["K"], sc["n1"]
    status = np.zeros((K, n1), np.uint8); x3d = np.zeros((K, n1, 3), f32); branch = np.zeros((K, n1), np.uint8)
    cosp = np.zeros((K, n1), f32); n_new = np.zeros(K, np.int32)
    o1 = sc["side1"].get("kp_is_orb"); o2 = sc["side2"].get("kp_is_orb")
    has_mp = np.zeros(n1, bool)
    ratioFactor = sc["rf_orb"]
    for k in range(K):
        if variant == "ratio_reset_per_neighbour":
            ratioFactor = sc["rf_orb"]
        for idx1 in range(n1):
            idx2 = int(sc["match12"][k, idx1])
            if idx2 < 0:
                status[k, idx1] = S["no_match"]; continue
            if has_mp[idx1] and variant != "claim_ignored":
                status[k, idx1] = S["claimed"]; continue
            a = True if o1 is None else bool(o1[idx1]); b = True if o2 is None else bool(o2[int(sc["kf_off"][k]) + idx2])
            if a != b:
                status[k, idx1] = S["type"]; continue
            if variant == "ratio_reset_per_pair":
                ratioFactor = sc["rf_orb"]
            if not a and not b:
                ratioFactor = sc["rf_ak"]
            st, br, cr, x = pair_model(sc, k, idx1, idx2, ratioFactor, variant)
            status[k, idx1] = st; branch[k, idx1] = br; cosp[k, idx1] = cr
            if st == S["new"]:
                x3d[k, idx1] = x; has_mp[idx1] = True; n_new[k] += 1
    return dict(status=status, x3d=x3d, branch=branch, cos_parallax=cosp, n_new=n_new)


# ---- one pair in float64: numpy's SVD, plain formulas --------------------------------------------------------------------------------
def _unproject64(cam, x, y):
    fx, fy, cx, cy = [float(v) for v in cam[:4]]
    px, py = (x - cx) / fx, (y - cy) / fy
    if len(cam) <= 4:
        return np.array([px, py, 1.0])
    k = [float(v) for v in cam[4:8]]
    td = min(max(np.hypot(px, py), -np.pi / 2), np.pi / 2)
    if td <= 1e-8:
        return np.array([px, py, 1.0])
    th = td
    for _ in range(50):
        t2 = th * th
        th -= (th * (1 + k[0] * t2 + k[1] * t2 ** 2 + k[2] * t2 ** 3 + k[3] * t2 ** 4) - td) / (1 + 3 * k[0] * t2 + 5 * k[1] * t2 ** 2 + 7 * k[2] * t2 ** 3 + 9 * k[3] * t2 ** 4)
    s = np.tan(th) / td
    return np.array([px * s, py * s, 1.0])


def _project64(cam, p):
    fx, fy, cx, cy = [float(v) for v in cam[:4]]
    if len(cam) <= 4:
        return fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy
    k = [float(v) for v in cam[4:8]]
    th = np.arctan2(np.hypot(p[0], p[1]), p[2]); psi = np.arctan2(p[1], p[0])
    r = th + k[0] * th ** 3 + k[1] * th ** 5 + k[2] * th ** 7 + k[3] * th ** 9
    return fx * r * np.cos(psi) + cx, fy * r * np.sin(psi) + cy


def pair_f64(sc, k, idx1, idx2, ratioFactor):
    """-> (status, x3d or None, margin): margin = the smallest relative distance of a compared quantity to its threshold on the path
    taken (how far the float64 decision is from flipping)"""
    with np.errstate(all="ignore"):
        lm = sc["form"] == LOCAL_MAPPING
        twocam = lm and sc["nleft1"] >= 0
        g2 = int(sc["kf_off"][k]) + idx2
        r1 = int(twocam and idx1 >= sc["nleft1"]); r2 = int(twocam and idx2 >= sc["nleft2"][k])
        V1, V2 = sc["views1"][r1], sc["views2"][k][r2]
        KF1, KF2 = sc["views1"][0], sc["views2"][k][0]
        R1, t1, Ow1 = np.asarray(V1["R"], f64).reshape(3, 3), np.asarray(V1["t"], f64).reshape(3), np.asarray(V1["Ow"], f64).reshape(3)
        R2, t2, Ow2 = np.asarray(V2["R"], f64).reshape(3, 3), np.asarray(V2["t"], f64).reshape(3), np.asarray(V2["Ow"], f64).reshape(3)
        p1 = np.array([sc["kps1"]["x"][idx1], sc["kps1"]["y"][idx1]], f64); p2 = np.array([sc["kps2"]["x"][g2], sc["kps2"]["y"][g2]], f64)
        s1, s2 = sc["side1"], sc["side2"]
        ur1 = float(s1["uright"][idx1]) if s1.get("uright") is not None else -1.0
        ur2 = float(s2["uright"][g2]) if s2.get("uright") is not None else -1.0
        st1 = not twocam and ur1 >= 0; st2 = not twocam and ur2 >= 0
        margins = []

        def cmp(a, b, scale=None):
            margins.append(abs(a - b) / max(abs(b) if scale is None else scale, 1e-300))
        if lm:
            xn1, xn2 = _unproject64(V1["cam"], *p1), _unproject64(V2["cam"], *p2)
        else:
            c1, c2 = [float(v) for v in V1["cam"][:4]], [float(v) for v in V2["cam"][:4]]
            xn1 = np.array([(p1[0] - c1[2]) / c1[0], (p1[1] - c1[3]) / c1[1], 1.0]); xn2 = np.array([(p2[0] - c2[2]) / c2[0], (p2[1] - c2[3]) / c2[1], 1.0])
        ray1, ray2 = R1.T @ xn1, R2.T @ xn2
        cosr = ray1 @ ray2 / (np.linalg.norm(ray1) * np.linalg.norm(ray2))
        cs1 = cs2 = cosr + 1
        if st1:
            cs1 = np.cos(2 * np.arctan2(float(sc["mb1"]) / 2, float(s1["depth"][idx1])))
        elif st2:
            cs2 = np.cos(2 * np.arctan2(float(sc["mb2"][k]) / 2, float(s2["depth"][g2])))
        cs = min(cs1, cs2)
        # (1 - cos is the quantity with a scale: a relative margin on cos itself would call every low-parallax pair close)
        cmp(1 - cosr, 1 - cs, 1 - min(cs, 0.9998)); cmp(cosr, 0.0, 1.0)
        if not (st1 or st2):
            cmp(1 - cosr, 1 - 0.9998)

        def unproject_stereo(V, side, i, p):
            z = float(side["depth"][i])
            if not z > 0:
                return None
            raw = side.get("raw_xy")
            u, v = (float(raw[i][0]), float(raw[i][1])) if raw is not None else p
            c = [float(x) for x in V["cam"][:4]]
            Rv, Ov = np.asarray(V["R"], f64).reshape(3, 3), np.asarray(V["Ow"], f64).reshape(3)
            return Rv.T @ np.array([(u - c[2]) * z / c[0], (v - c[3]) * z / c[1], z]) + Ov
        if cosr < cs and cosr > 0 and (st1 or st2 or cosr < 0.9998):
            T1, T2 = np.concatenate([R1, t1.reshape(3, 1)], 1), np.concatenate([R2, t2.reshape(3, 1)], 1)
            A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
            Vt = np.linalg.svd(A)[2]
            if Vt[3, 3] == 0:
                return S["w_zero"], None, min(margins)
            x3d = Vt[3, :3] / Vt[3, 3]
        elif st1 and cs1 < cs2:
            cmp(1 - cs1, 1 - cs2)
            x3d = unproject_stereo(V1, s1, idx1, p1)
        elif st2 and cs2 < cs1:
            cmp(1 - cs2, 1 - cs1)
            x3d = unproject_stereo(V2, s2, g2, p2)
        else:
            return S["parallax"], None, min(margins)
        if x3d is None:
            return S["empty_stereo"], None, min(margins)
        if not np.all(np.isfinite(x3d)):
            return S["nonfinite"], None, min(margins)
        P1, P2 = R1 @ x3d + t1, R2 @ x3d + t2
        depth = max(np.linalg.norm(x3d - Ow1), 1e-300)
        cmp(P1[2], 0.0, depth)
        if P1[2] <= 0:
            return S["z1"], x3d, min(margins)
        cmp(P2[2], 0.0, depth)
        if P2[2] <= 0:
            return S["z2"], x3d, min(margins)
        oc1, oc2 = int(sc["kps1"]["octave"][idx1]), int(sc["kps2"]["octave"][g2])
        sg1 = float(s1["kp_sigma2"][idx1]) if s1.get("kp_sigma2") is not None else float(sc["level_sigma2"][oc1])
        sg2 = float(s2["kp_sigma2"][g2]) if s2.get("kp_sigma2") is not None else float(sc["level_sigma2"][oc2])
        mbf1 = float(KF1.get("mbf", 0.0))

        def gate(V, KF, Pc, stereo, p, ur, sg):
            kc = [float(x) for x in KF["cam"][:4]]
            if not stereo:
                u, v = _project64(V["cam"], Pc) if lm else (kc[0] * Pc[0] / Pc[2] + kc[2], kc[1] * Pc[1] / Pc[2] + kc[3])
                e = (u - p[0]) ** 2 + (v - p[1]) ** 2; lim = 5.991 * sg
            else:
                u, v = kc[0] * Pc[0] / Pc[2] + kc[2], kc[1] * Pc[1] / Pc[2] + kc[3]
                e = (u - p[0]) ** 2 + (v - p[1]) ** 2 + (u - mbf1 / Pc[2] - ur) ** 2; lim = 7.8 * sg
            if not np.isfinite(e):
                return None
            cmp(e, lim)
            return e > lim
        for which, g in ((1, gate(V1, KF1, P1, st1, p1, ur1, sg1)), (2, None)):
            if which == 2:
                g = gate(V2, KF2, P2, st2, p2, ur2, sg2)
            if g is None:
                return S["nonfinite"], x3d, min(margins)
            if g:
                return S["reproj%d" % which], x3d, min(margins)
        d1, d2 = np.linalg.norm(x3d - Ow1), np.linalg.norm(x3d - Ow2)
        if d1 == 0 or d2 == 0:
            return S["zero_dist"], x3d, min(margins)
        if lm and sc["far_points"]:
            cmp(d1, float(sc["th_far"])); cmp(d2, float(sc["th_far"]))
            if d1 >= sc["th_far"] or d2 >= sc["th_far"]:
                return S["far"], x3d, min(margins)
        rd = d2 / d1
        sc1 = float(s1["kp_scale"][idx1]) if s1.get("kp_scale") is not None else float(sc["level_scale"][oc1])
        sc2 = float(s2["kp_scale"][g2]) if s2.get("kp_scale") is not None else float(sc["level_scale"][oc2])
        ro = sc1 / sc2
        cmp(rd * ratioFactor, ro); cmp(rd, ro * ratioFactor)
        if rd * ratioFactor < ro or rd > ro * ratioFactor:
            return S["scale"], x3d, min(margins)
        return S["new"], x3d, min(margins)
