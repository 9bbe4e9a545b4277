"""Loader of the CPU restatement of the Sim3 solver (sim3_ref.c, beside this file): compiled with the host C compiler into a temporary
directory when first used, strict IEEE.  Test infrastructure: nothing under eorb_slam_amd/ imports it.  The KannalaBrandt8 projection
is the oracle's orc_camera_project, handed to the restatement as a function pointer (as tests/proj_ref does)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-std=c99", "-Wall", "-Wno-unused-function"]

OPT_FLOAT_BOUND, OPT_HOST_ATAN2 = 0, 1
PROBE_NAMES = ["jacobi_exit_eps", "jacobi_exit_max_iters", "y_negative", "y_non_negative", "sort_swap_0", "sort_swap_1", "sort_swap_2",
               "sort_no_swap", "hypot_a_larger", "hypot_b_positive", "hypot_zero", "nan_transform", "rodrigues_identity", "rodrigues_general",
               "scale_copy", "scale_multiply", "camera_pinhole", "camera_kb8", "fix_scale", "free_scale", "rule_too_few", "rule_converged",
               "rule_greater", "rule_equal", "rule_below", "rule_exhausted", "atan2_q0", "atan2_q1", "atan2_q2", "atan2_q3"]
# branches no caller of ComputeSim3 reaches: norm(vec) >= 0 and both arguments are finite or NaN together, so atan2 is only entered with
# y >= +0 (quadrants 1 and 3 need y < 0; tests/test_sim3_ref.py reaches them through atan2 itself)
PROBE_ATAN2_ONLY = ("atan2_q1", "atan2_q3")


class Camera(C.Structure):
    """= eorb_camera"""
    _fields_ = [("model", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k", C.c_float * 4), ("precision", C.c_float)]


class Result(C.Structure):
    """= eorb_sim3_result"""
    _fields_ = [("converged", C.c_int32), ("best_it", C.c_int32), ("n_inliers", C.c_int32), ("iterations_used", C.c_int32),
                ("T12", C.c_float * 16), ("R12", C.c_float * 9), ("t12", C.c_float * 3), ("s12", C.c_float)]


def camera(cam):
    """(fx, fy, cx, cy) -> Pinhole; (fx, fy, cx, cy, k1, k2, k3, k4[, precision]) -> KannalaBrandt8"""
    c = Camera()
    c.fx, c.fy, c.cx, c.cy = [float(v) for v in cam[:4]]
    if len(cam) > 4:
        c.model = 1
        for i in range(4):
            c.k[i] = float(cam[4 + i])
        c.precision = float(cam[8]) if len(cam) > 8 else 1e-6
    return c


_libs = {}


def lib(timing=False):
    """the strict build the tests compare with; timing=True: the same source with -O3 -march=native (still -ffp-contract=off, same
    results), what tools/sim3_latency.py times"""
    if timing in _libs:
        return _libs[timing]
    tmp = tempfile.mkdtemp(prefix="sim3_ref_")
    atexit.register(shutil.rmtree, tmp, True)
    so = os.path.join(tmp, "libsim3_ref.so")
    flags = (["-O3", "-march=native"] + CFLAGS[1:]) if timing else CFLAGS
    subprocess.check_call([os.environ.get("CC", "gcc")] + flags + [os.path.join(_HERE, "sim3_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, ci, cd, cl = C.c_void_p, C.c_int, C.c_double, C.c_long
    L.pr_set_project.restype = None; L.pr_set_project.argtypes = [vp]
    L.s3r_set_option.restype = None; L.s3r_set_option.argtypes = [ci, ci]
    L.s3r_probe_reset.restype = None; L.s3r_probe_read.restype = None; L.s3r_probe_read.argtypes = [vp]
    L.s3r_probe_count.restype = ci
    L.s3r_atan2.restype = cd; L.s3r_atan2.argtypes = [cd, cd]
    L.s3r_atan2_n.restype = None; L.s3r_atan2_n.argtypes = [vp, vp, cl, vp]
    L.s3r_host_atan2_n.restype = None; L.s3r_host_atan2_n.argtypes = [vp, vp, cl, vp]
    L.s3r_eigen4.restype = None; L.s3r_eigen4.argtypes = [vp, vp, vp, vp]
    L.s3r_compute_sim3.restype = None; L.s3r_compute_sim3.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp]
    L.s3r_project.restype = None; L.s3r_project.argtypes = [vp, vp, vp, vp]
    L.s3r_bound.restype = C.c_float; L.s3r_bound.argtypes = [C.c_float]
    L.s3r_result_rule.restype = ci; L.s3r_result_rule.argtypes = [vp, ci, ci, ci, vp]
    L.s3r_ransac.restype = ci
    L.s3r_ransac.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp]
    assert L.s3r_probe_count() == len(PROBE_NAMES)
    from oracle import oracle_py
    L.pr_set_project(C.cast(oracle_py.lib().orc_camera_project, C.c_void_p))
    _libs[timing] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def set_option(which, value):
    for t in _libs.values():
        t.s3r_set_option(which, int(value))
    if not _libs:
        lib().s3r_set_option(which, int(value))


def probe_reset():
    lib().s3r_probe_reset()


def probe_read():
    a = np.zeros(len(PROBE_NAMES), np.int64 if C.sizeof(C.c_long) == 8 else np.int32)
    lib().s3r_probe_read(_p(a))
    return dict(zip(PROBE_NAMES, (int(v) for v in a)))


def atan2(y, x, host=False):
    y, x = np.broadcast_arrays(np.asarray(y, np.float64), np.asarray(x, np.float64))
    y = np.ascontiguousarray(y); x = np.ascontiguousarray(x); out = np.zeros(y.shape, np.float64)
    (lib().s3r_host_atan2_n if host else lib().s3r_atan2_n)(_p(y), _p(x), y.size, _p(out))
    return out


def eigen4(A):
    """cv::eigen of a symmetric 4x4 float matrix -> (eigenvalues descending, eigenvectors as rows, rotations executed, hit maxIters)"""
    A = np.ascontiguousarray(A, np.float32); assert A.shape == (4, 4)
    w = np.zeros(4, np.float32); V = np.zeros((4, 4), np.float32); st = np.zeros(2, np.int32)
    lib().s3r_eigen4(_p(A), _p(w), _p(V), _p(st))
    return w, V, int(st[0]), bool(st[1])


def compute_sim3(P1, P2, fix_scale=False):
    """ComputeSim3 on two point triples given as [3 points, 3] arrays -> dict(T12, T21, R12, t12, s12)"""
    P1 = np.ascontiguousarray(np.asarray(P1, np.float32).reshape(3, 3).T); P2 = np.ascontiguousarray(np.asarray(P2, np.float32).reshape(3, 3).T)
    T12 = np.zeros((4, 4), np.float32); T21 = np.zeros((4, 4), np.float32); R = np.zeros((3, 3), np.float32); t = np.zeros(3, np.float32)
    s = np.zeros(1, np.float32)
    lib().s3r_compute_sim3(_p(P1), _p(P2), int(bool(fix_scale)), _p(T12), _p(T21), _p(R), _p(t), _p(s))
    return dict(T12=T12, T21=T21, R12=R, t12=t, s12=s[0])


def project(T, cam, X):
    """Project (:472-490) of one point: the image of T*X in the camera -> float32 (u, v)"""
    T = np.ascontiguousarray(T, np.float32).reshape(16); X = np.ascontiguousarray(X, np.float32).reshape(3); uv = np.zeros(2, np.float32)
    cam = camera(cam)
    lib().s3r_project(_p(T), C.byref(cam), _p(X), _p(uv))
    return uv


def bound(sigma2):
    return np.float32(lib().s3r_bound(float(np.float32(sigma2))))


def result_rule(it_inliers, N, min_inliers):
    """-> dict(converged, best_it, n_inliers, iterations_used)"""
    cnt = np.ascontiguousarray(it_inliers, np.int32); o = np.zeros(3, np.int32)
    best = lib().s3r_result_rule(_p(cnt), len(cnt), int(N), int(min_inliers), _p(o))
    conv = int(o[0])
    return dict(converged=conv, best_it=int(best), n_inliers=int(o[1]), iterations_used=0 if best < 0 else (int(o[2]) if conv else len(cnt)))


def ransac_iterations(N, probability, min_inliers, max_iterations):
    """mRansacMaxIts of SetRansacParameters (:137-147).  int nIterations = ceil(...) of a value no int holds converts as the reference's
    x86 build does (cvttsd2si: INT_MIN), which max(1, min(...)) turns into 1."""
    epsilon = float(np.float32(min_inliers) / np.float32(N))
    if min_inliers == N:
        n = 1
    else:
        with np.errstate(all="ignore"):
            v = np.ceil(np.log(np.float64(1 - probability)) / np.log(np.float64(1) - np.float64(epsilon) ** 3))
        n = int(v) if np.isfinite(v) and -2147483648.0 <= v < 2147483648.0 else -2147483648
    return max(1, min(n, int(max_iterations)))


def draw_sets(N, iterations, seed):
    """the minimal sets of :178-189 on a numpy generator: three draws without replacement by the swap-with-back scheme"""
    rng = np.random.default_rng(seed)
    sets = np.zeros((iterations, 3), np.int32)
    for it in range(iterations):
        moved = {}
        for i in range(3):
            size = N - i
            randi = int(rng.integers(0, size))
            sets[it, i] = moved.get(randi, randi)
            moved[randi] = moved.get(size - 1, size - 1)
    return sets


class Sim3Solver:
    """mirrors eorb_slam_amd.frontend.Sim3Solver: the same methods, arguments and result dicts"""

    def __init__(self, Xw1, Xw2, Rt1, Rt2, cam1, cam2, sigma2_1, sigma2_2, fix_scale=True, timing=False):
        self.L = lib(timing)
        self.Xw1 = np.ascontiguousarray(Xw1, np.float32).reshape(-1, 3); self.Xw2 = np.ascontiguousarray(Xw2, np.float32).reshape(-1, 3)
        self.N = len(self.Xw1)
        assert len(self.Xw2) == self.N
        self.Rt1 = np.ascontiguousarray(Rt1, np.float32).reshape(12); self.Rt2 = np.ascontiguousarray(Rt2, np.float32).reshape(12)
        self.cam1, self.cam2 = camera(cam1), camera(cam2)
        self.sigma2_1 = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma2_1, np.float32), (self.N,)))
        self.sigma2_2 = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma2_2, np.float32), (self.N,)))
        self.fix_scale = bool(fix_scale)
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        self.probability, self.min_inliers = float(probability), int(min_inliers)
        self.iters = ransac_iterations(self.N, probability, min_inliers, max_iterations)
        return self.iters

    def draw_sets(self, seed):
        return draw_sets(self.N, self.iters, seed)

    def prepare(self, sets, aids=True):
        sets = np.ascontiguousarray(sets, np.int32)
        assert sets.ndim == 2 and sets.shape[1] == 3
        it, N = len(sets), self.N
        o = dict(inliers=np.zeros(N, np.uint8))
        a = dict(it_inliers=np.zeros(it, np.int32), it_T12=np.zeros((it, 4, 4), np.float32), it_T21=np.zeros((it, 4, 4), np.float32),
                 it_scale=np.zeros(it, np.float32)) if aids else {}
        return sets, o, a, np.zeros(12 * N, np.float32), Result()

    def run(self, prep, stop_early=False):
        """stop_early: end at the first converging iteration as the reference does (the timing baseline; the same results)"""
        sets, o, a, work, res = prep
        self.L.s3r_ransac(self.N, _p(self.Xw1), _p(self.Xw2), _p(self.Rt1), _p(self.Rt2), C.byref(self.cam1), C.byref(self.cam2), _p(self.sigma2_1),
                          _p(self.sigma2_2), int(self.fix_scale), self.min_inliers, len(sets), _p(sets), int(stop_early), C.byref(res), _p(o["inliers"]),
                          _p(a.get("it_inliers")), _p(a.get("it_T12")), _p(a.get("it_T21")), _p(a.get("it_scale")), _p(work))
        return res

    def find(self, sets, aids=False):
        prep = self.prepare(sets, aids)
        return result_dict(self.run(prep), prep[1], prep[2])

    @staticmethod
    def solve_candidates(solvers, sets_list, aids=False):
        return [s.find(sets, aids) for s, sets in zip(solvers, sets_list)]


def result_dict(res, o, a):
    o = dict(o)
    o.update(converged=int(res.converged), best_it=int(res.best_it), n_inliers=int(res.n_inliers), iterations_used=int(res.iterations_used),
             T12=np.array(res.T12, np.float32).reshape(4, 4), R12=np.array(res.R12, np.float32).reshape(3, 3), t12=np.array(res.t12, np.float32),
             s12=np.float32(res.s12))
    o.update(a)
    return o
