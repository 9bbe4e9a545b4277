"""GPU parity of CreateNewMapPoints on the device (eorb_new_map_points, eorb_create_new_map_points and its KannalaBrandt8 form): status,
x3d, n_new and the test aids equal the CPU restatement (tests/newpts_ref, the sequential double loop) as bytes on every scene of
tests/newpts_ref/scenes.py in both forms; K = 1 is row 0 of K = 3; a fused call returns what the search and the stage return in sequence,
byte for byte, and that is the restatement on the search's rows; the argument errors; K == 0."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfbatch_cases as kc                          # noqa: E402
import newpts_ref as nr                             # noqa: E402
from newpts_ref import scenes                       # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

pytestmark = pytest.mark.gpu

E_CONFIG, E_CAPACITY, E_ARG = -2, -3, -4
KEYS = ("status", "x3d", "branch", "cos_parallax", "n_new")


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def all_scenes():
    return scenes.all_scenes()


def _dev(fe, ctx, sc):
    v1, v2 = nr.views(sc)
    return fe.NewMapPoints(sc["kps1"], sc["kps2"], sc["kf_off"], sc["match12"], v1, v2, ctx=ctx, **nr.params(sc))


def _assert_same(got, ref, what):
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, k, np.argwhere(a != b)[:5].tolist())


def _other_form(sc):
    o = dict(sc)
    o["form"] = scenes.TRACKING if sc["form"] == scenes.LOCAL_MAPPING else scenes.LOCAL_MAPPING
    o["name"] = sc["name"] + "_other_form"
    return o


def test_stage_equals_the_restatement_on_every_scene_in_both_forms(fe, ctx, all_scenes):
    for name, sc in all_scenes.items():
        _assert_same(_dev(fe, ctx, sc), nr.loop(sc), name)
        if sc["nleft1"] < 0:                                         # (the Tracking form has no two-camera branch)
            o = _other_form(sc)
            _assert_same(_dev(fe, ctx, o), nr.loop(o), o["name"])


def _first_neighbour(sc):
    o = dict(sc)
    n2 = int(sc["kf_off"][1])
    o["K"] = 1; o["kf_off"] = sc["kf_off"][:2].copy(); o["kps2"] = sc["kps2"][:n2].copy(); o["match12"] = sc["match12"][:1].copy()
    o["views2"] = sc["views2"][:1]; o["nleft2"] = None if sc["nleft2"] is None else sc["nleft2"][:1].copy()
    o["mb2"] = None if sc["mb2"] is None else sc["mb2"][:1].copy()
    o["side2"] = {k: a[:n2].copy() for k, a in sc["side2"].items()}
    return o


@pytest.mark.parametrize("name", ["mono", "stereo", "twocam", "exact"])
def test_one_neighbour_is_row_0_of_three(fe, ctx, all_scenes, name):
    sc = all_scenes[name]
    assert sc["K"] == 3
    full, one = _dev(fe, ctx, sc), _dev(fe, ctx, _first_neighbour(sc))
    for k in KEYS:
        assert np.array_equal(np.ascontiguousarray(one[k][0]).view(np.uint8), np.ascontiguousarray(full[k][0]).view(np.uint8)), (name, k)


@pytest.mark.parametrize("kind", ["pinhole", "kb8", "twocam"])
def test_fused_call_equals_search_then_stage(fe, ctx, kind):
    s, views1, views2, scale, sigma2 = scenes.search_scene(kind)
    kfs = fe.KeyFrameSet(kc.tri_set(s))
    K = len(s["kfs"])
    ks = list(range(K))
    mk = lambda vs: nr.views(dict(views1=views1, views2=vs, level_scale=scale))      # noqa: E731
    v1, v2 = mk(views2)
    kw = dict(level_scale=scale, level_sigma2=sigma2, ratio_factor_orb=np.float32(1.5) * scale[1], ratio_factor_ak=np.float32(1.5) * scale[1])
    if kind == "pinhole":
        nm, m = fe.SearchForTriangulationKeyFrames(s["kps1"], s["desc1"], s["elig1"], s["fv1"], kfs, s["ep"][ks], s["F12"][ks], s["scale2"], s["sigma2_2"],
                                                   False, False, ctx=ctx)
        nm2, m2, out = fe.CreateNewMapPoints(s["kps1"], s["desc1"], s["elig1"], s["fv1"], kfs, s["ep"][ks], s["F12"][ks], s["scale2"], s["sigma2_2"],
                                             v1, v2, False, False, ctx=ctx, **kw)
        extra = {}
    else:
        nl2 = [s["kfs"][k]["nleft"] for k in ks]
        a = (s["kps1"], s["nleft1"], s["desc1"], s["elig1"], s["fv1"], kfs, nl2, s["cams1"], s["cams2"], s["Rt"][ks], s["ep"][ks], s["scale2"], s["sigma2_1"],
             s["sigma2_2"])
        nm, m = fe.SearchForTriangulationKB8KeyFrames(*a, False, False, ctx=ctx)
        nm2, m2, out = fe.CreateNewMapPointsKB8(*a, v1, v2, False, False, ctx=ctx, **kw)
        extra = dict(nleft1=s["nleft1"], nleft2=np.array(nl2, np.int32))
    assert np.array_equal(nm, nm2) and np.array_equal(m, m2)
    assert nm.min() >= 20                                            # real rows
    if kind == "twocam":
        assert K * len(s["kps1"]) > 1024                             # more than one workgroup of the pair kernel
    kf_off = np.cumsum([0] + [len(kf["kps"]) for kf in s["kfs"]]).astype(np.int32)
    two = fe.NewMapPoints(s["kps1"], kfs.kps, kf_off, m, v1, v2, ctx=ctx, **kw, **extra)
    _assert_same(out, two, kind)
    # and both are the sequential loop on the search's rows
    ref = nr.loop(scenes.scene_of_search(s, views1, views2, scale, sigma2, m, kind))
    _assert_same(out, ref, kind + " against the restatement")
    assert (out["status"] == nr.S["new"]).sum() >= 20 and (out["status"] == nr.S["claimed"]).sum() >= 1, np.bincount(out["status"].ravel())


def _code(fe, f):
    with pytest.raises(fe.EorbError) as e:
        f()
    return e.value.code


def test_argument_errors(fe, ctx, all_scenes):
    sc = all_scenes["mono"]
    v1, v2 = nr.views(sc)
    base = nr.params(sc)
    run = lambda **kw: fe.NewMapPoints(sc["kps1"], sc["kps2"], sc["kf_off"], kw.pop("match12", sc["match12"]), kw.pop("v1", v1), kw.pop("v2", v2),      # noqa: E731
                                       ctx=ctx, **{**base, **kw})
    assert _code(fe, lambda: run(form=2)) == E_ARG
    bad = sc["match12"].copy(); bad[1, 3] = int(sc["kf_off"][2] - sc["kf_off"][1])
    assert _code(fe, lambda: run(match12=bad)) == E_ARG                                  # a match outside its keyframe
    bad[1, 3] = -2
    assert _code(fe, lambda: run(match12=bad)) == E_ARG
    assert _code(fe, lambda: run(nleft1=10, nleft2=np.array([-1, 5, 5], np.int32))) == E_CONFIG      # one camera against two
    assert _code(fe, lambda: run(nleft1=10)) == E_ARG                                    # two cameras without nleft2
    assert _code(fe, lambda: run(form=1, nleft1=10, nleft2=np.array([5, 5, 5], np.int32))) == E_ARG      # Tracking has no two-camera branch
    assert _code(fe, lambda: run(mb1=-1.0)) == E_ARG
    assert _code(fe, lambda: run(level_scale=None, level_sigma2=None)) == E_ARG        # no per-keypoint arrays and no tables
    k = sc["kps1"].copy(); k["octave"][5] = 8
    assert _code(fe, lambda: fe.NewMapPoints(k, sc["kps2"], sc["kf_off"], sc["match12"], v1, v2, ctx=ctx, **base)) == E_ARG
    ur = np.full(sc["n1"], -1, np.float32)
    assert _code(fe, lambda: run(side1=dict(uright=ur))) == E_ARG                        # uright without depth
    ur[2] = 10.0
    assert _code(fe, lambda: run(side1=dict(uright=ur, depth=np.full(sc["n1"], np.nan, np.float32)))) == E_ARG
    w = nr.views(sc | dict(views1=[dict(sc["views1"][0], cam=(1.0,) * 4)]))[0]
    w[0].cam.model = 2
    assert _code(fe, lambda: run(v1=w)) == E_CONFIG
    # sizes are decided before any array is read
    big = np.zeros(1026, np.int32)
    assert _code(fe, lambda: fe.NewMapPoints(sc["kps1"], sc["kps2"], big, np.zeros((1025, sc["n1"]), np.int32), v1, [v2[0]] * 1025, ctx=ctx, **base)) == E_CAPACITY


def test_no_neighbours_and_no_matches(fe, ctx, all_scenes):
    sc = all_scenes["mono"]
    v1, v2 = nr.views(sc)
    r = fe.NewMapPoints(sc["kps1"], sc["kps2"][:0], np.zeros(1, np.int32), np.zeros((0, sc["n1"]), np.int32), v1, [], ctx=ctx, **nr.params(sc))
    assert r["status"].shape == (0, sc["n1"]) and r["n_new"].shape == (0,)
    none = np.full_like(sc["match12"], -1)
    r = fe.NewMapPoints(sc["kps1"], sc["kps2"], sc["kf_off"], none, v1, v2, ctx=ctx, **nr.params(sc))
    assert np.all(r["status"] == nr.S["no_match"]) and not r["x3d"].any() and not r["n_new"].any()
