"""Loader of the CPU restatement of the MLPnP solver (mlpnp_ref.c, beside this file): compiled with the host C compiler into a temporary
directory when first used, strict IEEE.  Test infrastructure: nothing under eorb_slam_amd/ imports it.  The KannalaBrandt8 projection
and both unprojections are the oracle's, handed to the restatement as function pointers (as tests/proj_ref does)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-std=c99", "-Wall", "-Wno-unused-function"]

OPT_HOST_LIBM, OPT_BOUND_LE, OPT_BEST_GE, OPT_REFINE_STORES, OPT_REFINE_GE, OPT_TRIGGER_GT = range(6)
PROBE_NAMES = ["planar", "non_planar", "det_flip_1", "det_keep_1", "det_flip_2", "det_keep_2", "planar_choice_0", "planar_choice_1",
               "planar_choice_2", "planar_choice_3", "non_planar_choice_0", "non_planar_choice_1", "gn_exit_dl", "gn_exit_max_it",
               "gn_exit_dx", "ldlt_moved", "ldlt_kept", "rodrigues_zero", "rodrigues_general", "rot_identity", "rot_general",
               "householder_zero", "householder_general", "svd_no_rotation", "svd_rotation", "svd_swap", "eig_v1_zero", "eig_v1_general",
               "too_few", "refined", "best_returned", "nothing_returned", "camera_pinhole", "camera_kb8"]


class Camera(C.Structure):
    """= eorb_camera"""
    _fields_ = [("model", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k", C.c_float * 4), ("precision", C.c_float)]


class Problem(C.Structure):
    """= eorb_mlpnp_problem"""
    _fields_ = [("N", C.c_int32), ("iters", C.c_int32), ("min_inliers", C.c_int32), ("th2", C.c_float), ("cam", Camera),
                ("first_it", C.c_int32), ("best_it", C.c_int32)]


class Result(C.Structure):
    """= eorb_mlpnp_result"""
    _fields_ = [("stop_it", C.c_int32), ("iterations_used", C.c_int32), ("best_it", C.c_int32), ("n_best", C.c_int32),
                ("refined", C.c_int32), ("n_inliers", C.c_int32), ("Tcw", C.c_float * 16)]


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
    results), what tools/mlpnp_latency.py times"""
    if timing in _libs:
        return _libs[timing]
    tmp = tempfile.mkdtemp(prefix="mlpnp_ref_")
    atexit.register(shutil.rmtree, tmp, True)
    so = os.path.join(tmp, "libmlpnp_ref.so")
    flags = (["-O3", "-march=native"] + CFLAGS[1:]) if timing else CFLAGS
    subprocess.check_call([os.environ.get("CC", "gcc")] + flags + [os.path.join(_HERE, "mlpnp_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, ci, cd, cl, cf = C.c_void_p, C.c_int, C.c_double, C.c_long, C.c_float
    L.pr_set_project.restype = None; L.pr_set_project.argtypes = [vp]
    L.mlr_set_unproject.restype = None; L.mlr_set_unproject.argtypes = [vp]
    L.mlr_set_option.restype = None; L.mlr_set_option.argtypes = [ci, ci]
    L.mlr_probe_reset.restype = None; L.mlr_probe_read.restype = None; L.mlr_probe_read.argtypes = [vp]
    L.mlr_probe_count.restype = ci
    for name in ("mlr_acos_n", "mlr_host_acos_n"):
        getattr(L, name).restype = None; getattr(L, name).argtypes = [vp, cl, vp]
    for name in ("mlr_pow_n", "mlr_host_pow_n"):
        getattr(L, name).restype = None; getattr(L, name).argtypes = [vp, cd, cl, vp]
    L.mlr_nullspace_n.restype = None; L.mlr_nullspace_n.argtypes = [vp, cl, vp]
    L.mlr_jsvd.restype = ci; L.mlr_jsvd.argtypes = [vp, ci, vp, vp, vp]
    L.mlr_rank3.restype = ci; L.mlr_rank3.argtypes = [vp]
    L.mlr_eig3.restype = None; L.mlr_eig3.argtypes = [vp, vp, vp]
    L.mlr_ldlt_solve.restype = None; L.mlr_ldlt_solve.argtypes = [vp, vp, vp]
    L.mlr_residual_jac.restype = None; L.mlr_residual_jac.argtypes = [vp, vp, vp, vp, vp]
    L.mlr_bound_test.restype = ci; L.mlr_bound_test.argtypes = [cf, cf, cf]
    L.mlr_compute_pose.restype = None; L.mlr_compute_pose.argtypes = [vp, vp, ci, vp]
    L.mlr_ransac.restype = ci; L.mlr_ransac.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci]
    L.mlr_refine_from.restype = ci; L.mlr_refine_from.argtypes = [vp, vp, vp, vp, vp, vp]
    assert L.mlr_probe_count() == len(PROBE_NAMES)
    from oracle import oracle_py
    L.pr_set_project(C.cast(oracle_py.lib().orc_camera_project, C.c_void_p))
    L.mlr_set_unproject(C.cast(oracle_py.lib().orc_camera_unproject, C.c_void_p))
    _libs[timing] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def set_option(which, value):
    for t in _libs.values():
        t.mlr_set_option(which, int(value))
    if not _libs:
        lib().mlr_set_option(which, int(value))


def probe_reset():
    lib().mlr_probe_reset()


def probe_read():
    a = np.zeros(len(PROBE_NAMES), np.int64 if C.sizeof(C.c_long) == 8 else np.int32)
    lib().mlr_probe_read(_p(a))
    return dict(zip(PROBE_NAMES, (int(v) for v in a)))


def _map1(fn, x, *extra):
    x = np.ascontiguousarray(x, np.float64); out = np.zeros(x.shape, np.float64)
    fn(_p(x), *extra, x.size, _p(out))
    return out


def acos(x, host=False):
    return _map1(lib().mlr_host_acos_n if host else lib().mlr_acos_n, x)


def pow_(x, y, host=False):
    return _map1(lib().mlr_host_pow_n if host else lib().mlr_pow_n, x, float(y))


def nullspace(f):
    """[n, 3] bearing vectors -> [n, 3, 2]"""
    f = np.ascontiguousarray(f, np.float64).reshape(-1, 3); ns = np.zeros((len(f), 3, 2), np.float64)
    lib().mlr_nullspace_n(_p(f), len(f), _p(ns))
    return ns


def jsvd(A, want_u=False):
    """JacobiSVD of a square matrix -> (singular values, V, U or None, rotations executed)"""
    A = np.ascontiguousarray(A, np.float64); n = A.shape[0]; assert A.shape == (n, n) and n <= 12
    V = np.zeros((n, n)); U = np.zeros((n, n)) if want_u else None; sv = np.zeros(n)
    rot = lib().mlr_jsvd(_p(A), n, _p(V), _p(U), _p(sv))
    return sv, V, U, rot


def rank3(M):
    return int(lib().mlr_rank3(_p(np.ascontiguousarray(M, np.float64).reshape(3, 3))))


def eig3(M):
    """SelfAdjointEigenSolver<Matrix3d> -> (eigenvalues increasing, eigenvectors as columns)"""
    w = np.zeros(3); Q = np.zeros((3, 3))
    lib().mlr_eig3(_p(np.ascontiguousarray(M, np.float64).reshape(3, 3)), _p(w), _p(Q))
    return w, Q


def ldlt_solve(A, g):
    dx = np.zeros(6)
    lib().mlr_ldlt_solve(_p(np.ascontiguousarray(A, np.float64).reshape(6, 6)), _p(np.ascontiguousarray(g, np.float64)), _p(dx))
    return dx


def residual_jac(x, X, ns):
    """x = (omega, T), one point X and its nullspace [3, 2] -> (r [2], J [2, 6])"""
    r = np.zeros(2); J = np.zeros((2, 6))
    lib().mlr_residual_jac(_p(np.ascontiguousarray(x, np.float64)), _p(np.ascontiguousarray(X, np.float64)),
                           _p(np.ascontiguousarray(ns, np.float64).reshape(3, 2)), _p(r), _p(J))
    return r, J


def bound_test(error2, sigma2, th2):
    return bool(lib().mlr_bound_test(float(np.float32(error2)), float(np.float32(sigma2)), float(np.float32(th2))))


def compute_pose(f, X):
    """computePose of bearing vectors f [n, 3] and points X [n, 3] (n >= 6) -> (R [3, 3], t [3]), Xc = R*Xw + t"""
    f = np.ascontiguousarray(f, np.float64).reshape(-1, 3); X = np.ascontiguousarray(X, np.float64).reshape(-1, 3); Rt = np.zeros(12)
    lib().mlr_compute_pose(_p(f), _p(X), len(f), _p(Rt))
    return Rt[:9].reshape(3, 3).copy(), Rt[9:].copy()


def ransac_parameters(*args, **kw):
    """SetRansacParameters (:268-298) -> (mRansacMinInliers, mRansacMaxIts): the product's one text (frontend.mlpnp_ransac_parameters),
    which tests/test_mlpnp_ref.py holds to hand-computed values and tests/test_host_mlpnp_cpp.py to the C++ mirror's"""
    from eorb_slam_amd.frontend import mlpnp_ransac_parameters
    return mlpnp_ransac_parameters(*args, **kw)


def draw_sets(N, iterations, seed):
    """the minimal sets of :176-188 on a numpy generator: the product's one text (frontend.mlpnp_draw_sets); the C++ mirror's DrawSets
    is held to the same swap-with-back scheme by tests/test_host_mlpnp_cpp.py"""
    from eorb_slam_amd.frontend import mlpnp_draw_sets
    return mlpnp_draw_sets(N, iterations, seed)


class MLPnPsolver:
    """mirrors eorb_slam_amd.frontend.MLPnPsolver: the same methods, arguments and result dicts"""

    def __init__(self, p2d, Xw, sigma2, cam, timing=False):
        self.L = lib(timing)
        self.p2d = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2); self.Xw = np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
        self.N = len(self.p2d)
        assert len(self.Xw) == self.N
        self.sigma2 = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma2, np.float32), (self.N,)))
        self.cam = camera(cam)
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=10, max_iterations=300, min_set=6, epsilon=0.5, th2=5.991):
        self.th2 = float(th2)
        self.min_inliers, self.iters = ransac_parameters(self.N, probability, min_inliers, max_iterations, min_set, epsilon)
        return self.iters

    def draw_sets(self, seed, iterations=None):
        return draw_sets(self.N, self.iters if iterations is None else iterations, seed)

    def problem(self, iters, first_it=0, best_it=-1):
        p = Problem()
        p.N, p.iters, p.min_inliers, p.th2, p.cam, p.first_it, p.best_it = self.N, int(iters), self.min_inliers, self.th2, self.cam, int(first_it), int(best_it)
        return p

    def find(self, sets, aids=False, first_it=0, best_it=-1, stop_early=False):
        return MLPnPsolver.solve_candidates([self], [sets], aids, [first_it], [best_it], stop_early)[0]

    @staticmethod
    def solve_candidates(solvers, sets_list, aids=False, first_its=None, best_its=None, stop_early=False):
        K = len(solvers)
        sets_list = [np.ascontiguousarray(s, np.int32) for s in sets_list]
        first_its = first_its or [0] * K; best_its = best_its or [-1] * K
        probs = (Problem * K)(*[s.problem(len(st), f, b) for s, st, f, b in zip(solvers, sets_list, first_its, best_its)])
        p2d = np.concatenate([s.p2d for s in solvers]); Xw = np.concatenate([s.Xw for s in solvers]); sg = np.concatenate([s.sigma2 for s in solvers])
        sets = np.concatenate(sets_list)
        tN, tI = len(p2d), len(sets)
        res = (Result * K)(); inl = np.zeros(tN, np.uint8)
        a = aid_arrays(tI) if aids else {}
        solvers[0].L.mlr_ransac(probs, K, _p(p2d), _p(Xw), _p(sg), _p(sets), res, _p(inl), _p(a.get("it_inliers")), _p(a.get("it_Rt")),
                                _p(a.get("it_refine_inliers")), int(stop_early))
        return split_results(solvers, sets_list, res, inl, a)

    def prepare(self, sets):
        """preallocated arguments of one mlr_ransac call without aids (what tools/mlpnp_latency.py times)"""
        sets = np.ascontiguousarray(sets, np.int32)
        return (Problem * 1)(self.problem(len(sets))), sets, (Result * 1)(), np.zeros(self.N, np.uint8)

    def run(self, prep, stop_early=False):
        probs, sets, res, inl = prep
        self.L.mlr_ransac(probs, 1, _p(self.p2d), _p(self.Xw), _p(self.sigma2), _p(sets), res, _p(inl), None, None, None, int(stop_early))
        return res[0]

    def refine_from(self, Rt):
        """the pose Refine computes from the flags of the pose Rt [12] and never stores, with the count it would have (-1: fewer than
        six flags): what the named wrong variant OPT_REFINE_STORES returns"""
        out = np.zeros(12)
        p = self.problem(1)
        n = self.L.mlr_refine_from(C.byref(p), _p(self.p2d), _p(self.Xw), _p(self.sigma2), _p(np.ascontiguousarray(Rt, np.float64).reshape(12)), _p(out))
        return int(n), out


def iterate_calls(solver, sets, n, calls, loop_and=False):
    """`calls` calls of iterate(n, ...) (:149-266) on a solver of either module, each one walk resumed from the state of the one before
    -> a list of dict(no_more, n_inliers, iterations, Tcw or None, inliers or None).  The loop condition is mnIterations < mRansacMaxIts
    || nCurrentIterations < nIterations; loop_and = the named wrong variant with &&."""
    out, done, best = [], 0, -1
    for _ in range(calls):
        if solver.N < solver.min_inliers:
            out.append(dict(no_more=1, n_inliers=0, iterations=0, Tcw=None, inliers=None))
            continue
        end = min(solver.iters, done + n) if loop_and else max(solver.iters, done + n)
        if end <= done:      # (the && variant runs nothing once the maximum is reached)
            out.append(dict(no_more=1, n_inliers=0, iterations=done, Tcw=None, inliers=None))
            continue
        o = solver.find(sets[:end], first_it=done, best_it=best)
        done, best = o["iterations_used"], o["best_it"]
        got = o["refined"] or o["n_best"] >= solver.min_inliers
        out.append(dict(no_more=int(not o["refined"]), n_inliers=o["n_inliers"] if got else 0, iterations=done, Tcw=o["Tcw"] if got else None,
                        inliers=o["inliers"] if got else None))
    return out


def aid_arrays(tI):
    return dict(it_inliers=np.zeros(tI, np.int32), it_Rt=np.zeros((tI, 12), np.float64), it_refine_inliers=np.zeros(tI, np.int32))


def split_results(solvers, sets_list, res, inl, a):
    out, n0, i0 = [], 0, 0
    for k, (s, st) in enumerate(zip(solvers, sets_list)):
        r = res[k]
        o = dict(inliers=inl[n0:n0 + s.N].copy(), stop_it=int(r.stop_it), iterations_used=int(r.iterations_used), best_it=int(r.best_it),
                 n_best=int(r.n_best), refined=int(r.refined), n_inliers=int(r.n_inliers), Tcw=np.array(r.Tcw, np.float32).reshape(4, 4))
        o.update({key: v[i0:i0 + len(st)].copy() for key, v in a.items()})
        out.append(o)
        n0 += s.N; i0 += len(st)
    return out
