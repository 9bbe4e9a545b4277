"""The two-camera oracle (oracle/orc_twocam.c) against the brute-force models of tests/twocam_model.py on the planted scenes of
tests/twocam_scenes.py, as integers; and the scenes themselves: every wrong variant of the models is told from the rule by a named
scene of every matcher that has the comparison, or is shown here to be indistinguishable; the probe counts each scene was built for
are non-zero.  No GPU."""
import collections
import itertools

import numpy as np
import pytest

import kfside_model as km
import match_scenes as ms
import twocam_model as tm
import twocam_scenes as ts

BASE, scenes, scene_names, CASES = ts.BASE, ts.scenes, ts.scene_names, ts.CASES

# the wrong variants every matcher must tell from the rule
WRONG = {
    "map": ["th_strict", "ratio_le", "ratio_double", "second_cut", "tie_index", "tie_last", "window_le", "grid_half_even", "level_off", "count_slots",
            "obs_unobserved", "obs_own", "viewcos_float", "right_uses_th", "right_after_left_reject", "right_gate_own_octave", "best_level_from_gate",
            "partner_not_claimed", "partner_not_counted", "partner_open"],
    "last": ["th_strict", "tie_index", "tie_last", "window_le", "grid_half_even", "level_off", "count_slots", "obs_unobserved", "obs_own",
             "rot_half_even", "rot_no_wrap", "maxima_le", "maxima_later", "rot_last_push", "right_gate_own_octave", "last_right_without_left_window",
             "last_empty_after_slots", "last_right_forward_capped", "rot_right_local_index"],
    "bow": ["th_strict", "ratio_le", "ratio_double", "second_cut", "tie_last", "rot_half_even", "rot_no_wrap", "maxima_le", "maxima_later",
            "bow_sides_merged", "bow_right_ratio", "bow_right_ungated", "bow_right_needs_left_ratio"],
}
# what no reachable input can tell from the rule, and why
INDISTINGUISHABLE = {
    ("bow", "tie_index"): "a node's feature list is ascending (FeatureVector::addFeature in keypoint order), so the first of equal distances is the lowest "
                          "index, on either side",
    ("bow", "count_slots"): "a matched frame feature is skipped by every later KeyFrame feature (:352), so every match and every histogram entry is a slot "
                            "of its own",
    ("bow", "bow_right_first"): "the two commits of one KeyFrame feature write different slots (one on each side) and none is read before the next KeyFrame "
                                "feature; the order shows only in the order of the entries inside the histogram's bins, and the bins are read as sets: "
                                "every entry of a losing bin clears its own slot and takes one from nmatches (:465-474), whatever its place",
    ("last", "partner_not_claimed"): "the last-frame form writes no partner slot (:2070, :2138)",
    ("last", "best_level_from_gate"): "the last-frame form keeps no level of its best",
}
# the probes a scene was built for: non-zero under at least one of its settings
PROBES = {
    "map": ["L best == TH", "L best == TH + 1", "R best == TH", "R best == TH + 1", "L ratio equal", "R ratio equal", "L second on another level",
            "R second on another level", "R gate != own, kept", "R gate != own, dropped", "R levels differ by table", "left rejected, right would match",
            "right only inside th x radius", "tie", "tie across cells", "partner claimed", "no partner", "closed through a link", "reopened through a link",
            "slot -2", "slot -3", "slot written twice", "right level one outside"],
    "last": ["L best == TH", "L best == TH + 1", "R best == TH", "R best == TH + 1", "R gate != own, kept", "R gate != own, dropped", "tie", "tie across cells",
             "slot -2", "slot -3", "left window empty, right matches", "left window all closed", "right projection outside", "right level one outside",
             "slot written twice"],
    "bow": ["L best == TH", "L best == TH + 1", "R best == TH", "R best == TH + 1", "bow left == TH, right <= TH", "bow left == TH, right > TH",
            "bow left == TH + 1, right <= TH", "bow left == TH + 1, right > TH", "L ratio equal", "bow left ratio fails, right taken",
            "bow right ratio would fail", "bow tie across sides", "bow both sides", "bow node > 64", "bow competed", "tie"],
    "wide": ["window cells > 64", "tie across 64 cells"],
    "crowded": ["cell > 64", "tie across a 64 stride"],
}


_MODEL = {}


def model_result(kind, name, cfg, check_ori=True, wrong=None):
    key = (kind, name, ts.config_id(cfg), check_ori, wrong)
    if key not in _MODEL:
        _MODEL[key] = ts.run_model(kind, dict(scenes(kind))[name], cfg, check_ori, wrong)
    return _MODEL[key]


def test_scene_names():
    for kind in ts.KINDS:
        assert [n for n, _ in scenes(kind)] == scene_names(kind)


@pytest.mark.parametrize("kind,name", CASES)
def test_oracle_equals_model(oracle, kind, name):
    sc = dict(scenes(kind))[name]
    for cfg, check_ori in itertools.product(ts.configs(kind), (True, False) if kind != "map" else (True,)):
        want = model_result(kind, name, cfg, check_ori)
        for fast in (False, True):
            got = ts.run_oracle(oracle, kind, sc, cfg, check_ori, fast)
            bad = np.flatnonzero(np.asarray(got[1]) != want[1])
            assert ts.same(got, want), "%s %s %s ori=%d fast=%d: nmatches %d, model %d; %d entries differ, first %s" % (
                kind, name, ts.config_id(cfg), check_ori, fast, got[0], want[0], len(bad), bad[:5])


@pytest.mark.parametrize("kind", ["map", "last"])
def test_oracle_equals_model_on_a_full_frame(oracle, kind):
    """kTcMaxKps keypoints over both cameras, eight queries"""
    sc = ts.full_scene()
    assert len(sc["kps"]) == ts.MAX_KPS
    want = ts.run_model(kind, sc, ts.MAIN[kind])
    assert ts.same(ts.run_oracle(oracle, kind, sc, ts.MAIN[kind]), want)
    assert want[0] >= 16 and (want[1][sc["nL"]:] >= 0).sum() >= 8


@pytest.mark.parametrize("kind", ts.KINDS)
def test_every_scene_matches(kind):
    """a matcher that matches nothing cannot pass"""
    for name, sc in scenes(kind):
        # no left window, no right search (:2033); no left best, no right match (:380)
        if name in ("base: no query", "bow: no query") or (kind == "last" and name.endswith("right only")) or name == "every feature right":
            assert all(model_result(kind, name, cfg)[0] == 0 for cfg in ts.configs(kind))
            continue
        best = max(model_result(kind, name, cfg)[0] for cfg in ts.configs(kind))
        assert best >= (2 if name.split(":")[0] in ("wide", "crowded") else 20), "%s %s: %d matches" % (kind, name, best)
    assert BASE[kind]().get("n_sites", 0) <= len(ts.SITES) and len(BASE[kind]()["kps"]) <= 320


@pytest.mark.parametrize("kind,wrong", [(k, w) for k in ts.KINDS for w in WRONG[k]])
def test_wrong_variant_is_rejected(kind, wrong):
    """the evidence that the boundary is reached: some scene and setting tells the variant from the rule"""
    hits = [(name, ts.config_id(cfg)) for (name, sc), cfg in itertools.product(scenes(kind), ts.configs(kind))
            if not ts.same(ts.run_model(kind, sc, cfg, True, wrong), model_result(kind, name, cfg))]
    print(kind, wrong, sorted({n for n, _ in hits}))
    assert hits, "%s: no scene tells %s (%s) from the rule" % (kind, wrong, tm.WRONG[wrong])


@pytest.mark.parametrize("kind,wrong", sorted(INDISTINGUISHABLE))
def test_indistinguishable_variants_change_nothing(kind, wrong):
    """the variants argued away above do give the rule's answer on every scene"""
    for (name, sc), cfg in itertools.product(scenes(kind), ts.configs(kind)):
        assert ts.same(ts.run_model(kind, sc, cfg, True, wrong), model_result(kind, name, cfg)), (name, cfg)


def test_variant_lists_are_complete():
    """a variant neither listed nor explained names a comparison the matcher does not have: it changes nothing"""
    for kind in ts.KINDS:
        for w in set(tm.WRONG) - set(WRONG[kind]) - {w for k, w in INDISTINGUISHABLE if k == kind}:
            for name in ("base",) + (("pushed twice",) if kind == "last" else ()):
                sc = dict(scenes(kind))[name]
                assert all(ts.same(ts.run_model(kind, sc, cfg, True, w), model_result(kind, name, cfg)) for cfg in ts.configs(kind)), (kind, w)


def _probe(kind, sc):
    total = {}
    for cfg in ts.configs(kind):
        info = {}
        ts.run_model(kind, sc, cfg, True, None, info)
        for k, v in info.get("probe", {}).items():
            total[k] = max(total.get(k, 0), v)
    return total


@pytest.mark.parametrize("kind", ts.KINDS)
def test_probe_counts(kind):
    """how often each scene reaches the comparisons it was built for (the largest count over the settings): none is zero"""
    p = _probe(kind, BASE[kind]())
    print(kind, {k: p.get(k, 0) for k in PROBES[kind]})
    assert all(p.get(k, 0) > 0 for k in PROBES[kind]), [k for k in PROBES[kind] if not p.get(k, 0)]
    assert set(PROBES[kind]) <= set(tm.PROBES)
    if kind != "bow":
        for name in ("wide", "crowded"):
            p = _probe(kind, dict(scenes(kind))[name])
            print(kind, name, {k: p.get(k, 0) for k in PROBES[name]})
            assert all(p.get(k, 0) > 0 for k in PROBES[name]), (name, p)


def test_gate_rule():
    """the right grid's gate table: left keypoint j's octave for j < nL, the right keypoint's own past that"""
    kps = np.zeros(7, ts.KP_DTYPE)
    kps["octave"] = [5, 6, 10, 11, 12, 13, 14]
    assert tm.gate_levels(kps, 2) == [5, 6, 12, 13, 14]
    sc = ts.map_scene()
    Fr = tm.twocam_frame(sc["kps"], sc["desc"], sc["nL"], ts.W, ts.H)
    assert sum(g != o for g, o in zip(Fr.gate, Fr.own)) >= 6


def test_histogram_scenes_hold_a_right_match_in_a_losing_bin():
    for kind in ("last", "bow"):
        found = 0
        for h in ms.HISTOGRAMS:
            if not ts.histogram_applies(h, kind):
                continue
            sc = ts.histogram_scene(kind, h)
            assert 30 <= sc["n_pushes"] <= 32
            on = ts.run_model(kind, sc, ts.MAIN[kind], True)[1]
            off = ts.run_model(kind, sc, ts.MAIN[kind], False)[1]
            found += int(((off >= 0) & (on < 0))[sc["nL"]:].sum() > 0)
        assert found >= 3, kind


# ---- the KeyFrame-side radius search: stereo gate, octave skip, in-order claim (oracle/orc_match.c) ---------------------------------

KF_WRONG = {
    "plain": ["tie_last", "tie_index", "window_le", "level_off"],
    "mono gate": ["octave_unchecked", "tie_last", "level_off"],
    "stereo gate": ["stereo_gate_mono", "uright_gt_zero", "chi2_float", "octave_unchecked"],
    "in order 50": ["taken_ignored", "taken_always", "accept_lt"],
    "in order 37.5": ["taken_ignored", "taken_always"],                     # (no integer is 37.5: `<` and `<=` agree)
    "mixed": ["mixed_level_octave", "type_gate_off", "tie_last", "level_off"],
    "mixed gate": ["mixed_level_octave", "type_gate_off", "stereo_gate_mono", "uright_gt_zero", "chi2_float"],
    "mixed in order 50": ["mixed_level_octave", "type_gate_off", "taken_ignored", "taken_always", "accept_lt"],
}
KF_PROBES = {
    "mono gate": ["mono gate", "chi2 == the float above 5.99", "chi2 == the float below 5.99", "octave outside the levels", "tie"],
    "stereo gate": ["stereo gate", "mono gate", "chi2 == the float above 7.8", "chi2 == the float below 7.8", "uright == 0", "octave outside the levels"],
    "in order 50": ["taken met", "best == accept_thr", "best just above accept_thr"],
    "in order 37.5": ["taken met", "best just above accept_thr"],
    "mixed": ["other type", "class_id level != octave"],
    "mixed gate": ["other type", "class_id level != octave", "stereo gate", "mono gate", "gate rejects", "chi2 == the float above 7.8", "uright == 0"],
}


def _same_kf(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("form", km.FORMS)
def test_kf_radius_oracle_equals_model(oracle, form):
    sc = km.scene()
    want = km.run_model(sc, form, valid=km.in_range(sc, form))
    got = km.run_oracle(oracle, sc, form)
    bad = np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))
    assert _same_kf(got, want), "%s: %d queries differ, first %s (%s)" % (form, len(bad), bad[:5], sc["names"][bad[:1]])
    assert (want[0] >= 0).sum() >= 40 and len(sc["kps"]) <= 260


@pytest.mark.parametrize("form,wrong", [(f, w) for f in km.FORMS for w in KF_WRONG[f]])
def test_kf_radius_wrong_variant_is_rejected(form, wrong):
    sc = km.scene()
    got, want = km.run_model(sc, form, wrong), km.run_model(sc, form)
    bad = np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))
    print(form, wrong, sorted(set(sc["names"][bad])))
    assert not _same_kf(got, want), "%s: the scene does not tell %s (%s) from the rule" % (form, wrong, km.WRONG[wrong])


def test_kf_radius_variant_lists_are_complete():
    """a variant not listed for a form names a comparison the form does not have (or one argued away below): it changes nothing"""
    sc = km.scene()
    for form in km.FORMS:
        for w in set(km.WRONG) - set(KF_WRONG[form]) - {"tie_index", "tie_last", "window_le", "level_off"}:
            assert _same_kf(km.run_model(sc, form, w), km.run_model(sc, form)), (form, w)


@pytest.mark.parametrize("form", sorted(KF_PROBES))
def test_kf_radius_probe_counts(form):
    info = {}
    km.run_model(km.scene(), form, None, info)
    print(form, dict(info["probe"]))
    assert all(info["probe"][k] > 0 for k in KF_PROBES[form]), [k for k in KF_PROBES[form] if not info["probe"][k]]


def test_chi2_constants_as_floats():
    """What `chi2_float` and `chi2_ge` can change.  The product is a float and the constants are doubles.
    5.99: (float)5.99 < 5.99, so no float lies in ((float)5.99, 5.99]: p > 5.99 and p > 5.99f hold for the same floats, and chi2_float
    cannot be told from the rule at the mono gate.  7.8: (float)7.8 > 7.8, so p == 7.8f is rejected by the rule and accepted in float:
    the scene plants fl(ex ex + ey ey + er er) == 7.8f (found by plant_e2's search, with er = 0 and with er = 1).
    chi2_ge: neither constant is a float (asserted), so p >= c and p > c hold for the same floats at both gates."""
    f = np.float32
    assert float(f(5.99)) < 5.99 and float(np.nextafter(f(5.99), f(10))) > 5.99
    assert float(f(7.8)) > 7.8 and float(np.nextafter(f(7.8), f(0))) < 7.8
    assert float(f(5.99)) != 5.99 and float(f(7.8)) != 7.8
    sc = km.scene()
    for form in ("mono gate", "stereo gate"):
        assert _same_kf(km.run_model(sc, form, "chi2_ge"), km.run_model(sc, form))
    assert _same_kf(km.run_model(sc, "mono gate", "chi2_float"), km.run_model(sc, "mono gate"))
    names = list(sc["names"])
    for n in ("stereo chi2 == 7.8f, er 0", "stereo chi2 == 7.8f, er 1"):
        m = names.index(n)
        rule, flt = km.run_model(sc, "stereo gate"), km.run_model(sc, "stereo gate", "chi2_float")
        assert rule[1][m] == 40 and flt[1][m] == 10, n                      # the rule rejects the near keypoint, the float comparison keeps it


# ---- the forms that project first: the projection of tests/kfside_ref, then the model --------------------------------------------------
@pytest.fixture(scope="module")
def ref(oracle):
    import kfside_ref
    kfside_ref.use_oracle_camera(oracle)
    return kfside_ref


@pytest.mark.parametrize("gate", ["mono", "stereo", "none"])
def test_k3_edge_values_oracle_equals_model(oracle, ref, gate):
    """K = 3: keyframe 0 empty, keyframes 1 and 2 on grids of their own with the edge values among their keypoint positions; the radius
    takes its edge values through th.  (A query centre comes out of the projector, which lets no non-finite or outside position pass
    IsInImage: those reach the search only in the caller-fed forms of tests/test_gpu_edges.py.)"""
    sc = km.batch_scene()
    views = [ref.view(**kw) for kw in sc["views"]]
    hits = 0
    for th in km.TH_VALUES:
        p = ref.keyframe_side(views, *km.geom(sc), th)
        for k in range(3):
            want = km.batch_model(sc, p, gate, k)
            got = km.batch_oracle(oracle, sc, p, gate, k)
            assert _same_kf(got, want), (th, k, np.flatnonzero(got[0] != want[0])[:5])
            hits += int((want[0] >= 0).sum())
    assert hits >= 60 and sum(len(k) == 0 for k in sc["kps"]) == 1
    for k in (1, 2):                                                        # the edge values are there, and outside the grid by the rule
        x = sc["kps"][k]["x"]
        assert np.isnan(x).any() and np.isinf(x).any() and (x == 2147483520.0).any() and (x == 65546.25).any()


def test_sim3_agreement(oracle, ref):
    """the agreement pass with th_high on both sides of a pair's two distances: the model against the oracle's searches thresholded and
    crossed in numpy, and the two variants rejected"""
    sp = km.sim3_scene()
    p12, p21 = km.sim3_projections(ref, sp)
    bi1, bd1, bi2, bd2 = km.sim3_searches(sp, p12, p21)
    F1 = oracle.Frame(sp["kf1"]["kps"], sp["kf1"]["desc"], sp["W"], sp["H"]); F2 = oracle.Frame(sp["kf2"]["kps"], sp["kf2"]["desc"], sp["W"], sp["H"])
    o1 = oracle.kf_radius_match(F2, p12["valid"], p12["uv"], p12["radius"], p12["level"], sp["kf1"]["mp_desc"])
    o2 = oracle.kf_radius_match(F1, p21["valid"], p21["uv"], p21["radius"], p21["level"], sp["kf2"]["mp_desc"])
    assert _same_kf(o1, (bi1, bd1)) and _same_kf(o2, (bi2, bd2))
    ths = km.sim3_th_values(bd1, bd2, bi1, bi2)
    assert len(ths) >= 5
    told = {"agree_one_way": 0, "agree_th_one_side": 0}
    total = collections.Counter()
    for th_high in ths:
        info = {}
        n, m12, vn1, vn2 = km.sim3_agree(bi1, bd1, bi2, bd2, th_high, None, info)
        total.update(info["probe"])
        w1 = np.where(o1[1] <= th_high, o1[0], -1); w2 = np.where(o2[1] <= th_high, o2[0], -1)
        assert np.array_equal(vn1, w1) and np.array_equal(vn2, w2)
        assert n == (m12 >= 0).sum() and all((m12[i] >= 0) == (w1[i] >= 0 and w2[w1[i]] == i) for i in range(len(w1)))
        for w in told:
            told[w] += int(not np.array_equal(km.sim3_agree(bi1, bd1, bi2, bd2, th_high, w)[1], m12))
    print(dict(total), told)
    assert all(told.values()), told
    assert total["best == th_high"] > 0 and total["best == th_high + 1"] > 0 and total["agreed"] >= 30 and total["one way only"] >= 10
