"""GPU parity of eorb_two_view_reconstruct with the CPU restatement (tests/twoview_ref/reconstruct_ref.c) through the ABI, for both forms.
Bytes are compared as in test_gpu_twoview.py (every NaN mapped to one canonical NaN on both sides), in the order of the stages: the
hypotheses (hyp_poses: tv_decide_kernel's algebra, after the RANSAC's H21 / F21), then CheckRT's counts and the parallax, then the decision
fields, then the slots -- so a failure names the stage."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twoview_ref as tv                                                    # noqa: E402
from twoview_ref import scenes                                              # noqa: E402
from twoview_ref import reconstruct_ref as rr                               # noqa: E402
from twoview_ref import reconstruct_scenes as rs                            # noqa: E402

pytestmark = pytest.mark.gpu

E_CAPACITY, E_ARG = -3, -4
SHAPES = [(8, 1), (9, 2), (63, 63), (64, 64), (65, 65), (300, 200)]
FORMS = (rr.FORM_STOCK, rr.FORM_INFO)
STAGE_KEYS = ("SH", "SF", "best_it_h", "best_it_f", "H21", "F21", "RH", "is_homography", "stage", "n_inliers", "n_hyp", "hyp_poses",
              "hyp_good", "hyp_parallax",
              "ok", "n_min_good", "n_similar", "info_good", "hyp_best", "hyp_second", "best_good", "second_good", "best_parallax", "second_parallax",
              "R21", "t21", "triangulated", "p3d", "trans_inliers")
assert set(STAGE_KEYS) == set(rr.RESULT_FIELDS) | {"hyp_poses", "R21", "t21", "triangulated", "p3d", "trans_inliers"}


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
            view = np.uint8 if g.dtype.itemsize == 1 else np.uint32 if g.dtype.itemsize == 4 else np.uint64
            bad = np.flatnonzero(g.reshape(-1).view(view) != w.reshape(-1).view(view))
            i = int(bad[0])
            raise AssertionError("%s: %s differs in %d places, first at flat index %d: device %r, restatement %r"
                                 % (what, k, len(bad), i, g.reshape(-1)[i], w.reshape(-1)[i]))


def _dev_params(par):
    from eorb_slam_amd import _lib
    return _lib.TvrReconParams(*[getattr(par, f[0]) for f in par._fields_])


def _device(fe, ctx, sc, sets, par):
    return fe.TwoViewReconstruction(scenes.K, sigma=par.sigma, ctx=ctx).reconstruct(sc["kps1"], sc["kps2"], sc["matches"], sets,
                                                                                    params=_dev_params(par), want_poses=True)


def _both(fe, ctx, sc, sets, par, what):
    dev = _device(fe, ctx, sc, sets, par)
    ref = rr.reconstruct(scenes.K, sc["kps1"], sc["kps2"], sc["matches"], sets, par)
    _same(dev, ref, STAGE_KEYS, what)
    return ref


_planted = {}


def _scene(name):
    if name not in _planted:
        build, N, iters, sets_seed, over, _ = rs.SCENES[name]
        _planted[name] = (build(), scenes.make_sets(N, iters, seed=sets_seed), over)
    return _planted[name]


# ---- parity ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,iters", SHAPES)
def test_parity_over_shapes(fe, ctx, N, iters):
    for kind in ("planar", "general", "noise", "mixed"):
        sc = scenes.scene(kind, N, seed=N + iters)
        assert len(sc["kps1"]) != len(sc["kps2"])
        sets = scenes.make_sets(N, iters, seed=N)
        for form in FORMS:
            ref = _both(fe, ctx, sc, sets, rr.params(form), "%s N=%d iters=%d form=%d" % (kind, N, iters, form))
            if N >= 63 and kind in ("planar", "general"):
                assert ref["stage"] == 2 and bool(ref["is_homography"]) == (kind == "planar"), (kind, N, ref["RH"])


@pytest.mark.parametrize("name", list(rs.SCENES))
def test_parity_on_planted_scenes(fe, ctx, name):
    sc, sets, over = _scene(name)
    exits = set()
    for form in FORMS:
        par = rr.params(form, **over)
        ref = _both(fe, ctx, sc, sets, par, "%s form=%d" % (name, form))
        exits.add(rs.probe(ref, par)[0])
    assert len(exits) == 2                                  # (one exit of each form)


def test_parity_sigma_and_parameters(fe, ctx):
    """sigma = 2 (th2 = 4.0f*(sigma*sigma) and the chi-square scale), and decision parameters away from their defaults"""
    sc = scenes.scene("mixed", 120, seed=2, noise=1.0)
    sets = scenes.make_sets(120, 40, seed=3)
    for form in FORMS:
        _both(fe, ctx, sc, sets, rr.params(form, sigma=2.0), "sigma 2")
        _both(fe, ctx, sc, sets, rr.params(form, min_triangulated=10, th_min_good_r=0.5, th_max_good_r_f=0.01, min_parallax=0.05), "loose rules")
        _both(fe, ctx, sc, sets, rr.params(form, th_hf_ratio=0.0, th_rd_homo=1.5), "H forced, a d test that leaves")


# ---- the new kernels apart from the old ones ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planar", "general", "mixed", "far_general", "tie_f_second", "tie_h_best", "pure_rotation", "same_keys", "h_none"])
def test_one_call_is_the_composition_the_library_offered(fe, ctx, name):
    """eorb_two_view_ransac -> the restated host algebra -> eorb_two_view_check_rt -> the restated decision: the same bytes as the one call"""
    sc, sets, over = _scene(name)
    n1 = len(sc["kps1"])
    T = fe.TwoViewReconstruction(scenes.K, ctx=ctx)
    for form in FORMS:
        par = rr.params(form, **over)
        one = _device(fe, ctx, sc, sets, par)
        ran = T.find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], sets)
        r, poses, sel, ti = rr.decide(scenes.K, ran, par)
        rt = None
        if r.n_hyp:
            rt = T.check_rt(sc["kps1"], sc["kps2"], sc["matches"], sel, poses[:r.n_hyp], th2=np.float32(4.0) * np.float32(par.sigma * par.sigma),
                            min_parallax_crt=par.min_parallax_crt, min_triangulated=par.min_triangulated)
        out = rr.finish(par, r, poses, n1, rt)
        two = dict(rr.result_dict(r), trans_inliers=ti, hyp_poses=poses, **out)
        _same(one, two, STAGE_KEYS, "%s form=%d against the two calls" % (name, form))


@pytest.mark.parametrize("name", ["same_keys", "pure_rotation"])
def test_early_stages_leave_everything_zero(fe, ctx, name):
    sc, sets, over = _scene(name)
    for form in FORMS:
        o = _device(fe, ctx, sc, sets, _dev_params(rr.params(form, **over)))
        assert o["stage"] == (0 if name == "same_keys" else 1) and o["ok"] == 0 and o["n_hyp"] == 0
        for k in ("R21", "t21", "p3d", "triangulated", "hyp_poses", "hyp_good", "hyp_parallax", "info_good"):
            assert not np.asarray(o[k]).any(), (name, form, k)
        for k in ("n_min_good", "n_similar", "best_good", "second_good", "best_parallax", "second_parallax"):
            assert o[k] == 0, (name, form, k)
        assert o["hyp_best"] == -1 and o["hyp_second"] == -1
        if name == "same_keys":
            assert o["RH"] == 0 and o["is_homography"] == 0 and o["n_inliers"] == 0 and not o["trans_inliers"].any()
        else:
            assert o["is_homography"] == 1 and o["n_inliers"] > 250
            assert int(o["trans_inliers"].sum()) == (o["n_inliers"] if form == rr.FORM_INFO else 0)


def test_a_second_call_gives_the_same_bytes(fe, ctx):
    """after every exit: the same call again, with another scene's call in between, gives the first call's bytes (nothing stays in the arena)"""
    names = ["planar", "general", "far_general", "far_similar", "small_baseline", "pure_rotation", "same_keys", "h_none", "tie_h_second"]
    first, exits = {}, set()
    for form in FORMS:
        for name in names:
            sc, sets, over = _scene(name)
            par = rr.params(form, **over)
            first[(name, form)] = _device(fe, ctx, sc, sets, par)
            exits.add(rs.probe(first[(name, form)], par)[0])
    assert exits == set(rs.EXITS), sorted(set(rs.EXITS) - exits)
    for form in FORMS:
        for name in reversed(names):
            sc, sets, over = _scene(name)
            _same(_device(fe, ctx, sc, sets, rr.params(form, **over)), first[(name, form)], STAGE_KEYS, "%s form=%d again" % (name, form))


def _rc(fe, call):
    with pytest.raises(fe.EorbError) as e:
        call()
    return e.value.code


def test_error_paths(fe, ctx):
    from eorb_slam_amd import _lib
    T = fe.TwoViewReconstruction(scenes.K, ctx=ctx)
    sc = scenes.scene("general", 20, seed=51)
    k1, k2, m = sc["kps1"], sc["kps2"], sc["matches"]
    ok_sets = scenes.make_sets(20, 3)
    assert _rc(fe, lambda: T.reconstruct(k1, k2, m[:7], np.zeros((3, 8), np.int32))) == E_ARG                    # N = 7
    s = ok_sets.copy(); s[2, 5] = 20
    assert _rc(fe, lambda: T.reconstruct(k1, k2, m, s)) == E_ARG                                                  # a set index equal to N
    s[2, 5] = -1
    assert _rc(fe, lambda: T.reconstruct(k1, k2, m, s)) == E_ARG
    bad = m.copy(); bad[3, 1] = len(k2)
    assert _rc(fe, lambda: T.reconstruct(k1, k2, bad, ok_sets)) == E_ARG                                          # a match outside the keys
    bad = m.copy(); bad[3, 0] = -1
    assert _rc(fe, lambda: T.reconstruct(k1, k2, bad, ok_sets)) == E_ARG
    bad = m.copy(); bad[4, 0] = bad[3, 0]
    assert _rc(fe, lambda: T.reconstruct(k1, k2, bad, ok_sets)) == E_ARG                                          # a repeated first index
    assert _rc(fe, lambda: T.reconstruct(k1, k2, m, ok_sets, min_triangulated=-1)) == E_ARG
    assert _rc(fe, lambda: T.reconstruct(k1, k2, m, ok_sets, form=2)) == E_ARG
    # the limits, each exceeded by one, decided from the sizes: the indices in these arrays are garbage and are not read
    assert _rc(fe, lambda: T.reconstruct(k1, k2, m, np.full((_lib.TVR_MAX_ITERS + 1, 8), 10 ** 6, np.int32))) == E_CAPACITY
    assert _rc(fe, lambda: T.reconstruct(k1, k2, np.full((_lib.TVR_MAX_MATCHES + 1, 2), 10 ** 6, np.int32), np.zeros((1, 8), np.int32))) == E_CAPACITY
    # ... and after the refusals the context still serves a call
    _both(fe, ctx, sc, ok_sets, rr.params(rr.FORM_INFO), "after the errors")


def test_python_mirror_gives_the_abi_bytes(fe, ctx):
    """frontend.TwoViewReconstruction.reconstruct against a direct ctypes call, without the test aid"""
    import ctypes as C
    from eorb_slam_amd import _lib
    sc, sets, _ = _scene("mixed")
    N, n1 = len(sc["matches"]), len(sc["kps1"])
    T = fe.TwoViewReconstruction(scenes.K, ctx=ctx)
    o = T.reconstruct(sc["kps1"], sc["kps2"], sc["matches"], sets, form=_lib.TVR_FORM_INFO)
    assert "hyp_poses" not in o and o["ok"] == 1
    par = T.recon_params(_lib.TVR_FORM_INFO)
    r = _lib.TvrReconResult()
    R = np.zeros(18, np.float32); t = np.zeros(6, np.float32); p3 = np.zeros(6 * n1, np.float32); tri = np.zeros(2 * n1, np.uint8); ti = np.zeros(N, np.uint8)
    L, p = ctx.L, fe._p
    Kf = np.ascontiguousarray(scenes.K, np.float32)
    assert L.eorb_two_view_reconstruct(ctx.h, p(sc["kps1"]), n1, p(sc["kps2"]), len(sc["kps2"]), p(sc["matches"]), N, p(sets), len(sets), p(Kf),
                                       C.byref(par), C.byref(r), p(R), p(t), p(p3), p(tri), p(ti), None) == 0
    raw = dict(rr.result_dict(r), R21=R.reshape(2, 3, 3), t21=t.reshape(2, 3), p3d=p3.reshape(2, n1, 3), triangulated=tri.reshape(2, n1), trans_inliers=ti)
    _same(o, raw, [k for k in STAGE_KEYS if k != "hyp_poses"], "python mirror")
