"""GPU parity of eorb_sim3_ransac with the CPU restatement (tests/sim3_ref) through the ABI.  Every comparison is an equality of bytes after
every NaN is mapped to one canonical NaN on both sides (host and device produce different NaN sign and payload bits; a NaN in the same
place counts as equal).  The per-iteration aids are compared before the winners, so that a failure names the iteration and the stage (an
it_T12 difference is ComputeSim3, a count difference with equal transforms is CheckInliers, a winner difference with equal counts is the
result rule)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_ref as s3                               # noqa: E402
from sim3_ref import scenes                         # noqa: E402

pytestmark = pytest.mark.gpu

E_CONFIG, E_CAPACITY, E_ARG = -2, -3, -4
KEYS = ("it_scale", "it_T12", "it_T21", "it_inliers", "converged", "best_it", "n_inliers", "iterations_used", "s12", "R12", "t12", "T12", "inliers")
AIDS = ("it_scale", "it_T12", "it_T21", "it_inliers")


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
    if a.dtype == np.float32:
        a = a.copy()
        a[np.isnan(a)] = np.float32(np.nan)
    return a


def _same(got, want, keys, what):
    for k in keys:
        g, w = _canon(got[k]), _canon(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.reshape(-1).view(np.uint8 if g.dtype.itemsize == 1 else np.uint32) !=
                                 w.reshape(-1).view(np.uint8 if w.dtype.itemsize == 1 else np.uint32)) if g.ndim else np.array([0])
            i = int(bad[0])
            raise AssertionError("%s: %s differs in %d places, first at flat index %d: device %r, restatement %r"
                                 % (what, k, len(bad), i, g.reshape(-1)[i], w.reshape(-1)[i]))


_REF = {}


def _ref(key, pb):
    """the restatement's answer, computed once per problem"""
    if key not in _REF:
        _REF[key] = scenes.find(s3, pb, aids=True)
    return _REF[key]


def _both(fe, ctx, pb, what):
    dev = scenes.find(fe, pb, aids=True, ctx=ctx)
    ref = _ref(what, pb)
    _same(dev, ref, KEYS, what)
    return ref


# ---- parity over shapes, cameras and scenes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 4, 63, 64, 65, 130])
@pytest.mark.parametrize("iters", [1, 63, 64, 65, 300])
def test_parity_over_shapes(fe, ctx, N, iters):
    """every N with every iteration count; the camera pair, fix_scale and the share of wrong correspondences rotate with them, and
    test_parity_over_cameras_and_scenes below covers their full product at one shape"""
    i = [3, 4, 63, 64, 65, 130].index(N) + [1, 63, 64, 65, 300].index(iters)
    pair, wrong, fs = ("pp", "kk", "pk", "kp")[i % 4], (0.0, 0.3, 1.0)[i % 3], bool(i & 1)
    pb = scenes.scene(N, seed=100 * N + iters, pair=pair, wrong=wrong, fix_scale=fs, iters=iters, min_inliers=min(6, max(N - 2, 1)))
    _both(fe, ctx, pb, "N=%d iters=%d %s wrong=%.1f fix=%d" % (N, iters, pair, wrong, fs))


@pytest.mark.parametrize("pair", ["pp", "kk", "pk", "kp"])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_parity_over_cameras_and_scenes(fe, ctx, pair, fix_scale):
    for wrong in (0.0, 0.3, 1.0):
        pb = scenes.scene(130, seed=7, pair=pair, wrong=wrong, fix_scale=fix_scale, iters=65)
        ref = _both(fe, ctx, pb, "%s fix=%d wrong=%.1f" % (pair, fix_scale, wrong))
        good = int((~pb["bad"]).sum())
        if wrong < 1.0:
            assert ref["converged"] == 1 and ref["n_inliers"] >= good - 3 and abs(float(ref["s12"]) - (1.0 if fix_scale else 1.3)) < 0.02
        else:
            assert ref["converged"] == 0 and ref["iterations_used"] == 65 and ref["n_inliers"] <= 6


# ---- K problems per call -----------------------------------------------------------------------------------------------------------------
def _solve_k(fe, ctx, pbs, aids=True):
    solvers = [scenes.solver(fe, pb, ctx=ctx) for pb in pbs]
    return fe.Sim3Solver.solve_candidates(solvers, [pb["sets"] for pb in pbs], aids=aids, ctx=ctx)


def test_k3_equals_three_k1_calls(fe, ctx):
    pbs = [scenes.scene(65, seed=31, pair="pp", iters=64), scenes.scene(65, seed=32, pair="kk", wrong=1.0, iters=64),
           scenes.scene(65, seed=33, pair="pk", fix_scale=True, iters=64)]
    together = _solve_k(fe, ctx, pbs)
    for k, pb in enumerate(pbs):
        alone = scenes.find(fe, pb, aids=True, ctx=ctx)
        _same(together[k], alone, KEYS, "K=3 against K=1, problem %d" % k)
        _same(alone, _ref(("k3", k), pb), KEYS, "K=1 problem %d" % k)


def test_k5_of_different_shapes(fe, ctx):
    few = scenes.two_groups(3, 3, 7, "AB")                                 # N = 6 < min_inliers = 7
    tiny = scenes.edge_problems()["three_points"]                          # N = 3, one iteration
    pbs = [scenes.scene(130, seed=41, pair="kp", iters=300), few, scenes.scene(4, seed=42, pair="kk", iters=63, min_inliers=2), tiny,
           scenes.scene(63, seed=43, pair="pp", wrong=1.0, fix_scale=True, iters=65)]
    out = _solve_k(fe, ctx, pbs)
    for k, pb in enumerate(pbs):
        _same(out[k], _ref(("k5", k), pb), KEYS, "K=5 problem %d" % k)
    assert out[1]["best_it"] == -1 and out[1]["iterations_used"] == 0 and not out[1]["it_T12"].any() and not out[1]["inliers"].any()
    assert out[3]["converged"] == 1 and out[3]["n_inliers"] == 3


def test_short_problem_between_two_live_ones(fe, ctx):
    """K = 3 with N = 65 / 6 / 63 and 65 / 1 / 1 iterations: the middle problem has N < min_inliers, so every kernel's skip path runs between
    two live problems whose sizes leave a tail in the count's 64-wide loop and in the hypothesis grid, at offsets that are no multiple of 64"""
    short = scenes.two_groups(3, 3, 7, "AB")                               # N = 6 < min_inliers = 7
    short["sets"] = short["sets"][:1]
    pbs = [scenes.scene(65, seed=71, pair="pk", iters=65), short, scenes.scene(63, seed=72, pair="kp", wrong=1.0, fix_scale=True, iters=1)]
    assert [(len(pb["Xw1"]), len(pb["sets"])) for pb in pbs] == [(65, 65), (6, 1), (63, 1)]
    out = _solve_k(fe, ctx, pbs)
    for k in (0, 2):
        _same(out[k], _ref(("short between", k), pbs[k]), KEYS, "K=3 problem %d" % k)
        _same(out[k], scenes.find(fe, pbs[k], aids=True, ctx=ctx), KEYS, "K=3 against K=1, problem %d" % k)
    s = out[1]                                                             # (:228-232)
    assert (s["converged"], s["best_it"], s["n_inliers"], s["iterations_used"]) == (0, -1, 0, 0)
    assert not any(np.frombuffer(np.asarray(s[k]).tobytes(), np.uint8).any() for k in ("T12", "R12", "t12", "s12", "inliers") + AIDS)


def test_winners_without_the_aids_equal_those_with_them(fe, ctx):
    pbs = [scenes.scene(64, seed=51, pair="pk", iters=65), scenes.scene(65, seed=52, pair="kk", wrong=1.0, iters=63)]
    with_aids, without = _solve_k(fe, ctx, pbs, aids=True), _solve_k(fe, ctx, pbs, aids=False)
    for a, b in zip(with_aids, without):
        assert not any(k in b for k in AIDS)
        _same(b, a, [k for k in KEYS if k not in AIDS], "without aids")


# ---- edge scenes of the CPU test through the ABI ----------------------------------------------------------------------------------------
EDGE = scenes.edge_problems()
RULE = scenes.rule_problems()


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_problems(fe, ctx, name):
    _both(fe, ctx, EDGE[name], name)


def test_large_coordinates(fe, ctx):
    _both(fe, ctx, scenes.large_coordinates(), "large coordinates")


@pytest.mark.parametrize("name", sorted(RULE))
def test_result_rule_scenes(fe, ctx, name):
    pb, _, want = RULE[name]
    ref = _both(fe, ctx, pb, name)
    assert {k: ref[k] for k in want} == want


@pytest.mark.parametrize("sigma2", [1.0, 0.1])
def test_threshold_quirk(fe, ctx, sigma2):
    pb, _ = scenes.threshold_problem(s3, sigma2)
    ref = _both(fe, ctx, pb, "threshold sigma2=%g" % sigma2)
    assert np.array_equal(ref["inliers"], [1, 1, 1, 0, 0, 1, 1] if sigma2 == 1.0 else [0] * 7)


# ---- error paths ---------------------------------------------------------------------------------------------------------------------------
def _raw_call(fe, ctx, pbs, K=None, edit=None):
    """eorb_sim3_ransac on the problems with sentinel-filled outputs; edit(probs, arrays) may spoil the inputs -> (rc, outputs untouched)"""
    from eorb_slam_amd import _lib
    solvers = [scenes.solver(fe, pb, ctx=ctx) for pb in pbs]
    probs = (_lib.Sim3Problem * len(pbs))(*[s.problem(len(pb["sets"])) for s, pb in zip(solvers, pbs)])
    arr = dict(Xw1=np.concatenate([s.Xw1 for s in solvers]), Xw2=np.concatenate([s.Xw2 for s in solvers]),
               sg1=np.concatenate([s.sigma2_1 for s in solvers]), sg2=np.concatenate([s.sigma2_2 for s in solvers]),
               sets=np.concatenate([pb["sets"] for pb in pbs]).copy())
    if edit:
        edit(probs, arr)
    tN, tI = len(arr["Xw1"]), len(arr["sets"])
    outs = [np.full(33 * 4 * len(pbs), 0x5A, np.uint8), np.full(tN, 0x5A, np.uint8), np.full(tI * 4, 0x5A, np.uint8),
            np.full(tI * 64, 0x5A, np.uint8), np.full(tI * 64, 0x5A, np.uint8), np.full(tI * 4, 0x5A, np.uint8)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = ctx.L.eorb_sim3_ransac(ctx.h, probs, len(pbs) if K is None else K, p(arr["Xw1"]), p(arr["Xw2"]), p(arr["sg1"]), p(arr["sg2"]),
                                p(arr["sets"]), *[p(o) for o in outs])
    _raw_call.outs = outs
    return rc, all((o == 0x5A).all() for o in outs)


def test_python_mirror_gives_the_abi_bytes(fe, ctx):
    pbs = [scenes.scene(20, seed=64, iters=8), scenes.scene(33, seed=65, pair="kp", wrong=1.0, iters=5)]
    rc, untouched = _raw_call(fe, ctx, pbs)
    assert rc == 0 and not untouched
    res, inl, cnt, t12, t21, sc = _raw_call.outs
    mirror = _solve_k(fe, ctx, pbs, aids=True)
    n0 = i0 = 0
    for k, (pb, m) in enumerate(zip(pbs, mirror)):
        N, it = len(pb["Xw1"]), len(pb["sets"])
        rec = res[132 * k:132 * (k + 1)]
        assert rec[:16].view(np.int32).tolist() == [m["converged"], m["best_it"], m["n_inliers"], m["iterations_used"]]
        want = np.concatenate([m["T12"].reshape(16), m["R12"].reshape(9), m["t12"], [m["s12"]]]).astype(np.float32)
        assert _canon(rec[16:].view(np.float32)).tobytes() == _canon(want).tobytes()
        assert inl[n0:n0 + N].tobytes() == m["inliers"].tobytes()
        assert cnt.view(np.int32)[i0:i0 + it].tobytes() == m["it_inliers"].tobytes()
        assert _canon(sc.view(np.float32)[i0:i0 + it]).tobytes() == _canon(m["it_scale"]).tobytes()
        assert _canon(t12.view(np.float32)[16 * i0:16 * (i0 + it)]).tobytes() == _canon(m["it_T12"].reshape(-1)).tobytes()
        assert _canon(t21.view(np.float32)[16 * i0:16 * (i0 + it)]).tobytes() == _canon(m["it_T21"].reshape(-1)).tobytes()
        n0 += N; i0 += it


def _set(field, value, k=0):
    def edit(probs, arr):
        setattr(probs[k], field, value)
    return edit


def _arr(name, index, value):
    def edit(probs, arr):
        arr[name].reshape(-1)[index] = value
    return edit


def _cam(which, model):
    def edit(probs, arr):
        getattr(probs[1], which).model = model
    return edit


ERRORS = [
    ("K = 0", E_ARG, dict(K=0)), ("K = -1", E_ARG, dict(K=-1)), ("K above the limit", E_CAPACITY, dict(K=65)),
    ("N = 2", E_ARG, dict(edit=_set("N", 2))), ("iters = 0", E_ARG, dict(edit=_set("iters", 0, 1))), ("min_inliers = -1", E_ARG, dict(edit=_set("min_inliers", -1))),
    ("N above the limit", E_CAPACITY, dict(edit=_set("N", 16385, 1))), ("iters above the limit", E_CAPACITY, dict(edit=_set("iters", 1025))),
    ("camera model 2", E_CONFIG, dict(edit=_cam("cam1", 2))), ("camera model -1", E_CONFIG, dict(edit=_cam("cam2", -1))),
    ("set index = N", E_ARG, dict(edit=_arr("sets", 4, 20))), ("set index -1", E_ARG, dict(edit=_arr("sets", -1, -1))),
    ("negative sigma2", E_ARG, dict(edit=_arr("sg1", 3, -1.0))), ("NaN sigma2", E_ARG, dict(edit=_arr("sg2", 21, np.nan))),
    ("sigma2 = 1e15", E_ARG, dict(edit=_arr("sg1", 0, 1e15))), ("infinite sigma2", E_ARG, dict(edit=_arr("sg2", 5, np.inf))),
]


@pytest.mark.parametrize("what,code,kw", ERRORS, ids=[e[0] for e in ERRORS])
def test_error_paths_leave_the_outputs_untouched(fe, ctx, what, code, kw):
    pbs = [scenes.scene(20, seed=61, iters=8), scenes.scene(20, seed=62, pair="kk", iters=8)]
    rc, untouched = _raw_call(fe, ctx, pbs, **kw)
    assert rc == code and untouched, (what, rc, untouched)
    rc, untouched = _raw_call(fe, ctx, pbs)                               # the next valid call on the same context succeeds
    assert rc == 0 and not untouched
    _both(fe, ctx, pbs[0], "after an error")


def test_the_limits_themselves_are_accepted(fe, ctx):
    """sigma2 just under 1e15 is valid, and so is iters = EORB_S3_MAX_ITERS"""
    pb = scenes.scene(20, seed=63, iters=1024)
    pb["sigma2_1"][0] = np.nextafter(np.float32(1e15), np.float32(0))
    _both(fe, ctx, pb, "limits")
