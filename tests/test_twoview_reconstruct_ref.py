"""The CPU restatement of TwoViewReconstruction::Reconstruct (tests/twoview_ref/reconstruct_ref.c with eorb_slam_amd/csrc/twoview_core.h)
against its second writing (tests/twoview_ref/reconstruct_model.py) on the planted scenes of tests/twoview_ref/reconstruct_scenes.py.  No
GPU: tests/test_gpu_twoview_reconstruct.py holds the device to the restatement byte for byte."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twoview_ref as tv                                                    # noqa: E402
from twoview_ref import scenes                                              # noqa: E402
from twoview_ref import reconstruct_model as model                          # noqa: E402
from twoview_ref import reconstruct_ref as rr                               # noqa: E402
from twoview_ref import reconstruct_scenes as rs                            # noqa: E402

FORMS = (rr.FORM_STOCK, rr.FORM_INFO)
# test_hypotheses_against_the_float64_model: the largest deviations measured over the scenes, and the bounds (4 x)
MEASURED_DR, MEASURED_DT = 3.835e-05, 2.254e-05
BOUND_DR, BOUND_DT = 4 * MEASURED_DR, 4 * MEASURED_DT

_cache = {}


def run(name, form, **over):
    """the restatement on a planted scene -> (result dict, parameters, scene); cached, the arrays are not to be changed"""
    key = (name, form, tuple(sorted(over.items())))
    if key not in _cache:
        build, N, iters, sets_seed, par_over, _ = rs.SCENES[name]
        sc = _cache.setdefault(("scene", name), build())
        p = rr.params(form, **dict(par_over, **over))
        o = rr.reconstruct(scenes.K, sc["kps1"], sc["kps2"], sc["matches"], scenes.make_sets(N, iters, seed=sets_seed), p)
        _cache[key] = (o, p, sc)
    return _cache[key]


def _agree(o, m, what):
    for k in model.RULE_KEYS:
        a, b = np.asarray(o[k]), np.asarray(m[k])
        assert a.shape == b.shape and a.tobytes() == b.astype(a.dtype).tobytes(), (what, k, o[k], m[k])


def _differs(o, m):
    return any(np.asarray(o[k]).tobytes() != np.asarray(m[k]).astype(np.asarray(o[k]).dtype).tobytes() for k in model.RULE_KEYS)


def _model(o, p, variant=None):
    nh = o["n_hyp"]
    return model.rules(p, bool(o["is_homography"]), o["hyp_good"][:nh], o["hyp_parallax"][:nh], o["n_inliers"], variant)


# ---- acos ----------------------------------------------------------------------------------------------------------------------------------
def test_acos_over_the_whole_domain():
    """fdlibm's e_acos.c as twoview_core.h states it, against the host libm: within one ulp on [-1, 1], exact at the ends, NaN outside"""
    rng = np.random.default_rng(0)
    xs = np.concatenate([np.linspace(-1, 1, 20001), rng.uniform(-1, 1, 20000), 1 - np.logspace(-16, -1, 200), -1 + np.logspace(-16, -1, 200),
                         np.logspace(-30, -1, 100), -np.logspace(-30, -1, 100)])
    for x in xs:
        a, b = rr.acos(x), math.acos(x)
        assert abs(a - b) <= math.ulp(b), (x, a, b)
    assert rr.acos(1.0) == 0.0 and rr.acos(-1.0) == math.pi and rr.acos(0.0) == math.pi / 2
    assert math.isnan(rr.acos(1.0000001)) and math.isnan(rr.acos(-2.0)) and math.isnan(rr.acos(float("nan")))
    assert rr.parallax(0, 0.5) == 0.0 and rr.parallax(3, 0.5) == np.float32(60.0) and rr.parallax(3, -1.0) == np.float32(180.0)


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_restatement_agrees_with_the_model_on_every_scene(form):
    for name in rs.SCENES:
        o, p, _ = run(name, form)
        if o["stage"] == 2:
            _agree(o, _model(o, p), (name, form))
        else:
            assert o["ok"] == 0 and o["n_hyp"] == 0 and o["hyp_best"] == -1 and o["hyp_second"] == -1 and not o["hyp_good"].any()


def _variant_cases():
    """variant -> (scene, form, parameter overrides or a function of the plain result giving them)"""
    return {
        "h_best_ge": ("tie_h_best", rr.FORM_INFO, None),
        "multimap_reversed": ("tie_f_second", rr.FORM_INFO, None),
        "nsimilar_ge1": ("general", rr.FORM_STOCK, None),
        "h_parallax_gt": ("planar", rr.FORM_STOCK, lambda o: dict(min_parallax=float(o["best_parallax"]))),
        "h_second_ge": ("tie_h_second", rr.FORM_INFO, None),
        "min_good_round": ("general", rr.FORM_INFO, lambda o: dict(th_min_good_r=(o["best_good"] + 0.6) / o["n_inliers"])),
    }


@pytest.mark.parametrize("variant", model.VARIANTS)
def test_every_wrong_variant_is_rejected_by_a_named_scene(variant):
    name, form, over = _variant_cases()[variant]
    o, p, _ = run(name, form)
    if over is not None:
        o, p, _ = run(name, form, **over(o))
    _agree(o, _model(o, p), (variant, name, "the right reading"))
    assert _differs(o, _model(o, p, variant)), (variant, name, o["hyp_good"], o["hyp_parallax"])
    if variant in ("nsimilar_ge1", "h_parallax_gt", "min_good_round"):
        assert o["ok"] == 1 and _model(o, p, variant)["ok"] == 0                # the scene sits on the accepting side of the comparison


@pytest.mark.parametrize("form", FORMS)
def test_one_and_no_hypothesis_on_given_counts(form):
    """the cases behind vR[-1] on counts no scene produces (reconstruct_scenes.py says why): one hypothesis with points, then none"""
    p = rr.params(form)
    n1 = 5
    for counts in ([0, 0, 0, 0, 0, 7, 0, 0], [0] * 8):
        r = rr.ReconResult(); r.stage = 2; r.is_homography = 1; r.n_hyp = 8; r.n_inliers = 7; r.hyp_best = r.hyp_second = -1
        poses = np.arange(8 * 27, dtype=np.float32).reshape(8, 27) + 1
        rt = dict(n_good=np.array(counts, np.int32), cos_sel=np.full(8, 0.5, np.float32), good=np.ones((8, n1), np.uint8),
                  p3d=np.ones((8, n1, 3), np.float32) * np.arange(1, 9, dtype=np.float32)[:, None, None])
        out = rr.finish(p, r, poses, n1, rt)
        o = rr.result_dict(r)
        _agree(o, model.rules(p, True, counts, [rr.parallax(c, 0.5) for c in counts], 7), counts)
        assert o["ok"] == 0 and o["hyp_second"] == -1
        assert not out["R21"][1].any() and not out["t21"][1].any() and not out["p3d"][1].any() and not out["triangulated"][1].any()
        if form == rr.FORM_INFO and any(counts):
            assert o["hyp_best"] == 5 and o["best_parallax"] == np.float32(60.0) and o["second_parallax"] == np.float32(-1.0)
            assert out["R21"][0].reshape(9).tolist() == poses[5, :9].tolist() and (out["p3d"][0] == 6.0).all() and out["triangulated"][0].all()
        else:
            assert o["hyp_best"] == -1 and not out["R21"][0].any() and not out["p3d"][0].any()


def test_probe_table_reaches_every_exit(capsys):
    """a condition of the scenes: every exit of both forms is reached, and each comparison of the rules falls both ways somewhere"""
    reached, outcomes, rows = set(), {}, []
    for name in rs.SCENES:
        for form in FORMS:
            o, p, _ = run(name, form)
            ex, c = rs.probe(o, p)
            reached.add(ex)
            for k, v in c.items():
                outcomes.setdefault((ex.split(":")[1], k), set()).add(v)
            rows.append("%-15s %-22s %s" % (name, ex, " ".join("%s=%s" % kv for kv in sorted(c.items()))))
    with capsys.disabled():
        print("\n" + "\n".join(rows))
    assert reached == set(rs.EXITS), sorted(set(rs.EXITS) - reached)
    for key in (("F", "few_good"), ("F", "similar"), ("F", "parallax"), ("H", "second"), ("H", "parallax"), ("H", "min_triangulated"), ("H", "min_good_r")):
        assert outcomes[key] == {True, False}, (key, outcomes[key])
    assert outcomes[("F", "min_good_from")] == {"N", "min_triangulated"}
    assert 0 in outcomes[("H", "hypotheses_with_points")]


# ---- the outputs around the rules ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_slots_and_flags_follow_the_rules_of_the_form(form):
    for name in rs.SCENES:
        o, p, sc = run(name, form)
        N = len(sc["matches"])
        r = tv.TwoViewReconstruction(scenes.K).find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"],
                                                                           scenes.make_sets(N, rs.SCENES[name][2], seed=rs.SCENES[name][3]))
        for k in ("SH", "SF", "best_it_h", "best_it_f", "H21", "F21"):
            assert np.asarray(o[k]).tobytes() == np.asarray(r[k]).astype(np.asarray(o[k]).dtype).tobytes(), (name, k)
        chosen = r["inliers_f"] if (o["stage"] == 0 or not o["is_homography"]) else r["inliers_h"]
        assert (o["trans_inliers"] == (chosen if form == rr.FORM_INFO else 0)).all(), name
        assert o["n_inliers"] == (0 if o["stage"] == 0 else int(chosen.sum())), name
        slots = (o["hyp_best"], o["hyp_second"])
        if form == rr.FORM_STOCK:
            assert slots[1] == -1 and (slots[0] >= 0) == bool(o["ok"]) and not o["info_good"].any(), name
        if o["stage"] < 2:
            assert slots == (-1, -1) and not o["hyp_poses"].any(), name
        for s, h in enumerate(slots):
            if h < 0:
                assert not o["R21"][s].any() and not o["t21"][s].any() and not o["p3d"][s].any() and not o["triangulated"][s].any(), (name, s)
            else:
                assert o["R21"][s].tobytes() == o["hyp_poses"][h, :9].tobytes() and o["t21"][s].tobytes() == o["hyp_poses"][h, 9:12].tobytes()
                assert o["triangulated"][s].sum() <= o["hyp_good"][h] and (o["p3d"][s].any(axis=1).sum() == o["hyp_good"][h]), (name, s)


def test_the_call_is_the_composition_of_its_parts():
    """tvr_reconstruct against ransac -> tvr_decide -> check_rt -> tvr_finish through the loaders the GPU test composes; the parallax of each
    hypothesis against the host's acos"""
    T = tv.TwoViewReconstruction(scenes.K)
    for name in ("planar", "general", "far_general", "pure_rotation", "same_keys", "h_none"):
        for form in FORMS:
            o, p, sc = run(name, form)
            N, n1 = len(sc["matches"]), len(sc["kps1"])
            ran = T.find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], scenes.make_sets(N, rs.SCENES[name][2], seed=rs.SCENES[name][3]))
            r, poses, sel, ti = rr.decide(scenes.K, ran, p)
            rt = None
            if r.n_hyp:
                rt = T.check_rt(sc["kps1"], sc["kps2"], sc["matches"], sel, poses[:r.n_hyp], th2=np.float32(4.0) * np.float32(p.sigma * p.sigma),
                                min_parallax_crt=p.min_parallax_crt, min_triangulated=p.min_triangulated)
            out = rr.finish(p, r, poses, n1, rt)
            got = dict(rr.result_dict(r), trans_inliers=ti, hyp_poses=poses, **out)
            for k in got:
                a, b = np.asarray(got[k]), np.asarray(o[k])
                assert a.shape == b.shape and (a.tobytes() == b.tobytes() or np.array_equal(a, b, equal_nan=True)), (name, form, k)
            for h in range(r.n_hyp):
                if rt["n_good"][h] > 0 and abs(rt["cos_sel"][h]) <= 1:
                    want = np.float32(math.acos(float(rt["cos_sel"][h])) * 180 / math.pi)
                    assert abs(float(o["hyp_parallax"][h]) - float(want)) <= float(np.spacing(want)), (name, h)


# ---- the hypotheses ------------------------------------------------------------------------------------------------------------------------
def _stage2_scenes():
    return [n for n in rs.SCENES if run(n, rr.FORM_INFO)[0]["stage"] == 2 and n != "d_test_off"]


def test_hypotheses_against_the_float64_model(capsys):
    """DecomposeE and the Faugeras hypotheses of the restatement (float32, OpenCV's operation order) against numpy in float64 from the same
    F21 / H21, every float64 pose matched to the nearest restated one, over every scene that reaches its hypotheses -- but d_test_off,
    whose d1, d2, d3 differ by rounding only: its square roots of differences carry no digit.  The bound is four times the largest deviation
    measured over these scenes on the CPU: headroom for scene seeds and nothing more.
    Measured: |R - R64| 3.835e-05, |t - t64| 2.254e-05, both on small_baseline (d1/d3 = 1.004, so the roots lose three digits; every other
    scene stays below 2.8e-06 and 1.5e-06); bounds 1.534e-04 and 9.016e-05."""
    worst = [0.0, 0.0, None]
    for name in _stage2_scenes():
        o, _, _ = run(name, rr.FORM_INFO)
        if o["is_homography"]:
            m, _ = model.faugeras(scenes.K, o["H21"])
        else:
            m = model.decompose_e(scenes.K, o["F21"])
        dR, dt = model.pose_deviation(m, o["hyp_poses"][:o["n_hyp"]])
        with capsys.disabled():
            print("%-15s %s dR %.3e dt %.3e" % (name, "H" if o["is_homography"] else "F", dR, dt))
        if max(dR, dt) > max(worst[:2]):
            worst[2] = name
        worst[0], worst[1] = max(worst[0], dR), max(worst[1], dt)
        assert dR <= BOUND_DR and dt <= BOUND_DT, (name, dR, dt)
    with capsys.disabled():
        print("largest: dR %.3e dt %.3e (%s)" % tuple(worst))
    # P2 and O2 of every record are K*[R|t] and -R^T t of its own R and t
    for name in _stage2_scenes():
        o, _, _ = run(name, rr.FORM_INFO)
        for q in o["hyp_poses"][:o["n_hyp"]].astype(np.float64):
            R, t = q[:9].reshape(3, 3), q[9:12]
            assert np.abs(q[12:24].reshape(3, 4) - scenes.K.astype(np.float64) @ np.concatenate([R, t[:, None]], axis=1)).max() <= 1e-4 * 500
            assert np.abs(q[24:27] + R.T @ t).max() <= 1e-6


@pytest.mark.parametrize("kind,N", [("planar", 63), ("planar", 300), ("general", 63), ("general", 300)])
def test_accepted_pose_is_the_true_pose(kind, N):
    """noise-free planar and general scenes: Reconstruct accepts, and the accepted hypothesis is the scene's motion within the bounds of
    test_hypotheses_against_the_float64_model"""
    sc = rs.moved(kind, N, seed=N, normal=rs._SLANT, noise=0.0, window=(20, 20, 400, 460))      # (the part of the plane the twin solution loses)
    for form in FORMS:
        o = rr.reconstruct(scenes.K, sc["kps1"], sc["kps2"], sc["matches"], scenes.make_sets(N, 64, seed=N), rr.params(form))
        assert o["ok"] == 1 and bool(o["is_homography"]) == (kind == "planar"), (kind, N, form, o["hyp_good"])
        dR, dt = np.abs(o["R21"][0] - sc["R"]).max(), np.abs(o["t21"][0] - sc["t"]).max()
        print(kind, N, form, "dR %.3e dt %.3e" % (dR, dt))
        assert dR <= BOUND_DR and dt <= BOUND_DT, (kind, N, dR, dt)
