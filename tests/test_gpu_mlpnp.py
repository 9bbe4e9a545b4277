"""GPU parity of eorb_mlpnp_ransac with the CPU restatement (tests/mlpnp_ref) through the ABI.  Every comparison is an equality of bytes
after every NaN, float and double, is mapped to one canonical NaN on both sides (host and device produce different NaN sign and payload
bits; a NaN in the same place counts as equal).  The per-iteration aids are compared before the winners, so that a failure names the
iteration and the stage: an it_Rt difference is computePose, a count difference with equal poses is CheckInliers, an it_refine_inliers
difference with equal counts is the walk, a winner difference with equal aids is the result rule."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlpnp_ref as mr                              # noqa: E402
from mlpnp_ref import scenes                        # noqa: E402

pytestmark = pytest.mark.gpu

E_CONFIG, E_CAPACITY, E_ARG = -2, -3, -4
AIDS = ("it_Rt", "it_inliers", "it_refine_inliers")
KEYS = AIDS + scenes.RULE_KEYS + ("Tcw", "inliers")
NS = [6, 7, 63, 64, 65, 130]
ITERS = [1, 15, 16, 17, 63, 64, 65, 300]


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


def _canon(a):
    a = np.array(a)
    if a.dtype in (np.float32, np.float64):
        a = a.copy()
        a[np.isnan(a)] = np.nan
    return a


def _same(got, want, keys, what):
    for k in keys:
        g, w = _canon(got[k]), _canon(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1)) if g.ndim else np.array([0])
            bad = bad if len(bad) else np.array([0])
            i = int(bad[0])
            raise AssertionError("%s: %s differs in %d places, first at flat index %d: device %r, restatement %r"
                                 % (what, k, len(bad), i, g.reshape(-1)[i], w.reshape(-1)[i]))


_REF = {}


def _both(fe, ctx, pb, what, first_it=0, best_it=-1):
    dev = scenes.find(fe, pb, aids=True, first_it=first_it, best_it=best_it, ctx=ctx)
    key = (what, first_it, best_it)
    if key not in _REF:      # the restatement's answer, computed once per problem
        _REF[key] = scenes.find(mr, pb, aids=True, first_it=first_it, best_it=best_it)
    _same(dev, _REF[key], KEYS, what)
    return _REF[key]


def _min_inliers(N):
    return max(6, min(10, N // 2))


# ---- parity over shapes, cameras and scenes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("iters", ITERS)
def test_parity_over_shapes(fe, ctx, N, iters):
    """every N with every iteration count; the camera, planarity and the share of wrong matches rotate with them, and
    test_parity_over_cameras_and_scenes below covers their full product at one shape"""
    i = NS.index(N) + ITERS.index(iters)
    cam, planar, wrong = "pk"[i % 2], bool((i // 2) % 2), (0.0, 0.3, 1.0)[i % 3]
    pb = scenes.scene(N, seed=100 * N + iters, cam=cam, wrong=wrong, planar=planar, iters=iters, min_inliers=_min_inliers(N))
    _both(fe, ctx, pb, "N=%d iters=%d %s planar=%d wrong=%.1f" % (N, iters, cam, planar, wrong))


@pytest.mark.parametrize("cam", ["p", "k"])
@pytest.mark.parametrize("planar", [False, True])
def test_parity_over_cameras_and_scenes(fe, ctx, cam, planar):
    for wrong in (0.0, 0.3, 1.0):
        pb = scenes.scene(130, seed=7, cam=cam, wrong=wrong, planar=planar, iters=65)
        ref = _both(fe, ctx, pb, "%s planar=%d wrong=%.1f" % (cam, planar, wrong))
        if wrong == 1.0:
            assert ref["refined"] == 0 and ref["iterations_used"] == 65
        elif not planar:
            assert ref["refined"] == 1 and pb["min_inliers"] < ref["n_inliers"] <= int((~pb["bad"]).sum()) + 3


# ---- K problems per call -----------------------------------------------------------------------------------------------------------------
def _solve_k(fe, ctx, pbs, aids=True):
    solvers = [scenes.solver(fe, pb, ctx=ctx) for pb in pbs]
    return fe.MLPnPsolver.solve_candidates(solvers, [pb["sets"] for pb in pbs], aids=aids, ctx=ctx)


def test_k3_equals_three_k1_calls_and_a_short_problem_stays_zero(fe, ctx):
    pbs = [scenes.scene(65, seed=31, cam="p", iters=64), scenes.scene(8, seed=32, cam="k", iters=17, min_inliers=10),
           scenes.scene(130, seed=33, cam="k", wrong=1.0, iters=33)]
    together = _solve_k(fe, ctx, pbs)
    refs = mr.MLPnPsolver.solve_candidates([scenes.solver(mr, pb) for pb in pbs], [pb["sets"] for pb in pbs], aids=True)
    for k, pb in enumerate(pbs):
        _same(together[k], refs[k], KEYS, "K=3 problem %d" % k)
        if k != 1:
            _same(together[k], scenes.find(fe, pb, aids=True, ctx=ctx), KEYS, "K=3 against K=1, problem %d" % k)
    short = together[1]                                 # N = 8 < min_inliers = 10 (:154-158)
    assert (short["stop_it"], short["best_it"], short["iterations_used"], short["n_best"], short["refined"], short["n_inliers"]) == (-1, -1, 0, 0, 0, 0)
    assert not short["Tcw"].any() and not short["inliers"].any() and not short["it_inliers"].any() and not short["it_Rt"].any()
    assert (short["it_refine_inliers"] == -1).all()


def test_short_problem_between_two_live_ones(fe, ctx):
    """K = 3 with N = 65 / 8 / 63 and 65 / 1 / 1 iterations: the middle problem has N < min_inliers, so every kernel's skip path runs between
    two live problems whose sizes leave a tail in the count's 64-wide loop and in the hypothesis grid, at offsets that are no multiple of 64"""
    pbs = [scenes.scene(65, seed=71, cam="k", iters=65), scenes.scene(8, seed=72, cam="p", iters=1, min_inliers=10),
           scenes.scene(63, seed=73, cam="p", wrong=1.0, planar=True, iters=1)]
    assert [(len(pb["p2d"]), len(pb["sets"])) for pb in pbs] == [(65, 65), (8, 1), (63, 1)]
    out = _solve_k(fe, ctx, pbs)
    refs = mr.MLPnPsolver.solve_candidates([scenes.solver(mr, pb) for pb in pbs], [pb["sets"] for pb in pbs], aids=True)
    for k in (0, 2):
        _same(out[k], refs[k], KEYS, "K=3 problem %d" % k)
        _same(out[k], scenes.find(fe, pbs[k], aids=True, ctx=ctx), KEYS, "K=3 against K=1, problem %d" % k)
    s = out[1]                                                             # (:154-158)
    assert (s["stop_it"], s["best_it"], s["iterations_used"], s["n_best"], s["refined"], s["n_inliers"]) == (-1, -1, 0, 0, 0, 0)
    assert not any(np.frombuffer(np.asarray(s[k]).tobytes(), np.uint8).any() for k in ("Tcw", "inliers", "it_inliers", "it_Rt"))
    assert (s["it_refine_inliers"] == -1).all()                           # Refine was invoked at no iteration


# ---- the result rule, resuming, odd inputs -----------------------------------------------------------------------------------------------
def test_more_than_one_record_before_the_successful_refine(fe, ctx):
    pb = scenes.records_scene()
    ref = _both(fe, ctx, pb, "records")
    assert ref["refined"] == 1 and (ref["it_refine_inliers"] >= 0).sum() >= 2


def test_no_refine_succeeds_and_the_best_is_returned(fe, ctx):
    pb = scenes.best_returned_scene()
    ref = _both(fe, ctx, pb, "best returned")
    assert ref["refined"] == 0 and ref["best_it"] >= 0 and ref["n_inliers"] == ref["n_best"] >= pb["min_inliers"] and ref["Tcw"][3, 3] == 1


@pytest.mark.parametrize("first_it", [1, 64, 129])
def test_resume_through_the_abi(fe, ctx, first_it):
    pb = scenes.resume_scene()
    one = _both(fe, ctx, pb, "resume, one shot")
    assert len(pb["sets"]) == 130 and one["stop_it"] == 100 and one["it_refine_inliers"][10] == 12
    best = scenes.rule_model(one["it_inliers"][:first_it], pb["min_inliers"])["best_it"]      # -1, 10, 100
    ref = _both(fe, ctx, pb, "resume", first_it=first_it, best_it=best)
    if first_it <= 100:
        assert {k: ref[k] for k in scenes.RULE_KEYS} == {k: one[k] for k in scenes.RULE_KEYS}
    else:
        assert (ref["refined"], ref["best_it"], ref["n_inliers"]) == (0, 100, 30)
    _both(fe, ctx, pb, "resume without a best", first_it=first_it, best_it=-1)


def test_nan_coordinates(fe, ctx):
    pb = scenes.scene(65, seed=51, iters=20)
    pb["Xw"][pb["sets"][2, 1], 0] = np.nan              # a NaN point in set 2: that hypothesis is NaN and has no inliers
    pb["p2d"][pb["sets"][5, 0], 1] = np.nan
    ref = _both(fe, ctx, pb, "NaN coordinates")
    assert np.isnan(ref["it_Rt"][2]).any() and ref["it_inliers"][2] == 0


def test_repeated_indices_inside_a_set_are_accepted(fe, ctx):
    pb = scenes.scene(65, seed=52, iters=8)
    pb["sets"][2] = [0, 0, 1, 2, 3, 4]
    pb["sets"][3] = [5, 5, 5, 5, 5, 5]
    _both(fe, ctx, pb, "repeated indices")


def test_python_mirror_iterate_equals_the_restatement(fe, ctx):
    """frontend.MLPnPsolver.iterate(5, ...) over four calls, as Relocalization makes them after a rejected pose, against the restatement
    driven by iterate_calls: a scene that refines in the first call and a false candidate that runs to the maximum, then five more"""
    for wrong in (0.3, 1.0):
        pb = scenes.scene(65, seed=81, cam="k", wrong=wrong, iters=320)
        dev, ref = fe.MLPnPsolver(pb["p2d"], pb["Xw"], pb["sigma2"], pb["cam"], ctx=ctx), mr.MLPnPsolver(pb["p2d"], pb["Xw"], pb["sigma2"], pb["cam"])
        assert (dev.min_inliers, dev.iters) == (ref.min_inliers, ref.iters) == (32, 35)
        want = mr.iterate_calls(ref, pb["sets"], 5, 4)
        for call, w in enumerate(want):
            Tcw, no_more, inl, n = dev.iterate(5, pb["sets"])
            assert (int(no_more), n, dev.mnIterations) == (w["no_more"], w["n_inliers"], w["iterations"]), (wrong, call)
            assert (Tcw is None) == (w["Tcw"] is None)
            if Tcw is not None:
                assert _canon(Tcw).tobytes() == _canon(w["Tcw"]).tobytes() and inl.tobytes() == w["inliers"].tobytes()
        if wrong == 1.0:
            assert [w["iterations"] for w in want] == [35, 40, 45, 50]
        else:
            assert want[0]["Tcw"] is not None and want[0]["iterations"] < 35 and want[1]["iterations"] > want[0]["iterations"]


# ---- error paths ---------------------------------------------------------------------------------------------------------------------------
def _raw_call(fe, ctx, pbs, K=None, edit=None):
    """eorb_mlpnp_ransac on the problems with sentinel-filled outputs; edit(probs, arrays) may spoil the inputs -> (rc, outputs untouched)"""
    solvers = [scenes.solver(fe, pb, ctx=ctx) for pb in pbs]
    from eorb_slam_amd import _lib
    probs = (_lib.MlpnpProblem * len(pbs))(*[s.problem(len(pb["sets"])) for s, pb in zip(solvers, pbs)])
    arr = dict(p2d=np.concatenate([s.p2d for s in solvers]), Xw=np.concatenate([s.Xw for s in solvers]),
               sg=np.concatenate([s.sigma2 for s in solvers]), sets=np.concatenate([pb["sets"] for pb in pbs]).copy())
    if edit:
        edit(probs, arr)
    tN, tI = len(arr["Xw"]), len(arr["sets"])
    outs = [np.full(22 * 4 * len(pbs), 0x5A, np.uint8), np.full(tN, 0x5A, np.uint8), np.full(tI * 4, 0x5A, np.uint8),
            np.full(tI * 96, 0x5A, np.uint8), np.full(tI * 4, 0x5A, np.uint8)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = ctx.L.eorb_mlpnp_ransac(ctx.h, probs, len(pbs) if K is None else K, p(arr["p2d"]), p(arr["Xw"]), p(arr["sg"]), p(arr["sets"]),
                                 *[p(o) for o in outs])
    _raw_call.outs = outs
    return rc, all((o == 0x5A).all() for o in outs)


def _set(field, value, k=0):
    def edit(probs, arr):
        setattr(probs[k], field, value)
    return edit


def _arr(name, index, value):
    def edit(probs, arr):
        arr[name].reshape(-1)[index] = value
    return edit


def _cam(model):
    def edit(probs, arr):
        probs[1].cam.model = model
    return edit


ERRORS = [
    ("K = 0", E_ARG, dict(K=0)), ("K above the limit", E_CAPACITY, dict(K=65)),
    ("N = 5", E_ARG, dict(edit=_set("N", 5))), ("iters = 0", E_ARG, dict(edit=_set("iters", 0, 1))), ("min_inliers = 5", E_ARG, dict(edit=_set("min_inliers", 5))),
    ("N above the limit", E_CAPACITY, dict(edit=_set("N", 4097, 1))), ("iters above the limit", E_CAPACITY, dict(edit=_set("iters", 1025))),
    ("camera model 2", E_CONFIG, dict(edit=_cam(2))), ("camera model -1", E_CONFIG, dict(edit=_cam(-1))),
    ("set index = N", E_ARG, dict(edit=_arr("sets", 4, 20))), ("set index -1", E_ARG, dict(edit=_arr("sets", -1, -1))),
    ("first_it = iters", E_ARG, dict(edit=_set("first_it", 8))), ("best_it = first_it", E_ARG, dict(edit=_set("best_it", 0, 1))),
]


@pytest.mark.parametrize("what,code,kw", ERRORS, ids=[e[0] for e in ERRORS])
def test_error_paths_leave_the_outputs_untouched(fe, ctx, what, code, kw):
    pbs = [scenes.scene(20, seed=61, iters=8), scenes.scene(20, seed=62, cam="k", iters=8)]
    rc, untouched = _raw_call(fe, ctx, pbs, **kw)
    assert rc == code and untouched, (what, rc, untouched)
    rc, untouched = _raw_call(fe, ctx, pbs)                               # the next valid call on the same context succeeds
    assert rc == 0 and not untouched
    _both(fe, ctx, pbs[0], "after an error")


def test_the_limits_themselves_are_accepted(fe, ctx):
    """iters = EORB_PNP_MAX_ITERS and N = EORB_PNP_MAX_CORR are valid"""
    _both(fe, ctx, scenes.scene(20, seed=63, iters=1024), "iteration limit")
    ref = _both(fe, ctx, scenes.scene(4096, seed=64, wrong=0.1, iters=3), "correspondence limit")
    assert ref["refined"] == 1
