"""The oracle's matchers (oracle/orc_match.c) against the brute-force models of tests/match_model.py on the planted scenes of
tests/match_scenes.py, as integers; and the scenes themselves: every wrong variant of the models is told from the rule by at least one
scene of every matcher it applies to, the boundary probe counts are non-zero, and no scene passes with nothing matched.  No GPU."""
import itertools

import numpy as np
import pytest

import match_model as mm
import match_scenes as ms

BUILDS = {"init": [False, True], "last": [False, True], "map": [False, True], "kf": [False]}     # (search_by_projection_kf takes no `fast`)

# the wrong variants every window matcher must tell from the rule; what a matcher cannot tell apart, and why
WINDOW_WRONG = {
    "init": ["th_strict", "ratio_le", "ratio_double", "second_cut", "tie_index", "tie_last", "window_le", "grid_half_even", "level_off",
             "state_lt", "steal_keep", "type_gate_off", "rot_half_even", "rot_no_wrap", "maxima_le", "maxima_later", "rot_skip_stolen"],
    "last": ["th_strict", "tie_index", "tie_last", "window_le", "grid_half_even", "level_off", "count_slots", "obs_unobserved", "obs_own",
             "type_gate_off", "stereo_ge", "rot_half_even", "rot_no_wrap", "maxima_le", "maxima_later", "rot_last_push"],
    "kf": ["th_strict", "tie_index", "tie_last", "window_le", "grid_half_even", "level_off", "type_gate_off", "rot_half_even", "rot_no_wrap",
           "maxima_le", "maxima_later"],
    "map": ["th_strict", "ratio_le", "ratio_double", "second_cut", "tie_index", "tie_last", "window_le", "grid_half_even", "level_off",
            "count_slots", "obs_unobserved", "obs_own", "type_gate_off", "stereo_ge", "viewcos_float"],
}
INDISTINGUISHABLE = {
    ("init", "count_slots"): "a steal takes one from nmatches and clears the slot in the same step, and the histogram clears only filled slots: "
                             "the counter is the number of filled slots at every point of the function",
    ("kf", "count_slots"): "`if(CurrentFrame.getMapPoint(i2)) continue;` lets no slot be written twice",
    ("kf", "rot_last_push"): "no slot is written twice",
    ("kf", "obs_unobserved"): "the keyframe form skips every slot that holds a map point, observed or not",
    ("kf", "obs_own"): "the same",
}


def _scenes(kind):
    """(name, scene) of every scene variant of a window matcher"""
    out = [("base", ms.window_scene(kind)), ("positions", ms.window_scene(kind, True))]
    out += [(h, ms.histogram_scene(kind, h)) for h in ms.HISTOGRAMS if ms.histogram_applies(h, kind)]
    return out


CASES = [(k, name, ms.config_id(c)) for k in ms.KINDS for name in ["base", "positions"] + [h for h in ms.HISTOGRAMS if ms.histogram_applies(h, k)]
         for c in ms.window_configs(k)]


_MODEL = {}


def model_result(kind, name, cfg, wrong=None):
    key = (kind, name, ms.config_id(cfg), wrong)
    if key not in _MODEL:
        _MODEL[key] = ms.run_model(dict(_scenes(kind))[name], cfg, True, wrong)
    return _MODEL[key]


@pytest.mark.parametrize("kind,name,cfg_id", CASES)
def test_oracle_equals_model(oracle, kind, name, cfg_id):
    sc = dict(_scenes(kind))[name]
    cfg = next(c for c in ms.window_configs(kind) if ms.config_id(c) == cfg_id)
    want = model_result(kind, name, cfg)
    for fast in BUILDS[kind]:
        got = ms.run_oracle(oracle, sc, cfg, True, fast)
        bad = np.flatnonzero(np.asarray(got[1]) != want[1])
        assert ms.same(got, want), "%s %s %s fast=%d: nmatches %d, model %d; %d entries differ, first %s" % (
            kind, name, cfg_id, fast, got[0], want[0], len(bad), bad[:5])
    if kind != "map":                                                   # and with mbCheckOrientation off
        got = ms.run_oracle(oracle, sc, cfg, False)
        assert ms.same(got, ms.run_model(sc, cfg, False)), "%s %s %s without the orientation check" % (kind, name, cfg_id)


@pytest.mark.parametrize("kind", ms.KINDS)
def test_every_scene_matches(kind):
    """a matcher that matches nothing cannot pass"""
    for name, sc in _scenes(kind):
        n = model_result(kind, name, ms.MAIN[kind])[0]
        assert n >= 20 and all(model_result(kind, name, cfg)[0] > 0 for cfg in ms.window_configs(kind)), "%s %s: %d matches" % (kind, name, n)
        assert sc["n_sites"] <= len(ms.SITES)


@pytest.mark.parametrize("kind,wrong", [(k, w) for k in ms.KINDS for w in WINDOW_WRONG[k]])
def test_wrong_variant_is_rejected(kind, wrong):
    """the evidence that the boundary is reached: some scene and setting tells the variant from the rule"""
    hits = []
    for (name, sc), cfg in itertools.product(_scenes(kind), ms.window_configs(kind)):
        if name == "positions":
            continue                                                     # (the same sites again)
        if not ms.same(ms.run_model(sc, cfg, True, wrong), model_result(kind, name, cfg)):
            hits.append((name, ms.config_id(cfg)))
    assert hits, "%s: no scene tells %s (%s) from the rule" % (kind, wrong, mm.WRONG[wrong])


def test_variant_lists_are_complete():
    window_variants = set(mm.WRONG) - {"tri_first"}
    for kind in ms.KINDS:
        listed = set(WINDOW_WRONG[kind]) | {w for k, w in INDISTINGUISHABLE if k == kind}
        absent = window_variants - listed
        # what is left names a comparison the matcher does not have
        for w in absent:
            sc = ms.window_scene(kind)
            assert all(ms.same(ms.run_model(sc, cfg, True, w), model_result(kind, "base", cfg)) for cfg in ms.window_configs(kind)), (kind, w)


@pytest.mark.parametrize("kind", ms.KINDS)
def test_probe_counts(kind):
    """the table of the boundary probe on the planted scenes: no column is zero"""
    sc = ms.window_scene(kind)
    ratio = 0.5 if kind in ("init", "map") else None
    p = ms.probe(sc, ratio)
    print(kind, p)
    assert p["queries"] >= 20 and p["best_eq_th"] > 0 and p["best_eq_th1"] > 0, p
    if ratio is not None:
        assert p["ratio_equal"] > 0 and p["ratio_near"] > 0, p
        assert all(ms.probe(sc, r)["ratio_near"] > 0 for r in (0.9, 0.6)) and ms.probe(sc, 1.0)["ratio_equal"] > 0


# ---- ComputeThreeMaxima ------------------------------------------------------------------------------------------------------
def test_three_maxima_exhaustive(oracle):
    """all histograms of three non-zero bins with counts in 0..21, in every order of the bins"""
    for a, b, c in itertools.product(range(22), repeat=3):
        h = np.zeros(mm.HISTO_LENGTH, np.int32)
        h[2], h[11], h[12] = a, b, c
        assert oracle.three_maxima(h) == mm.three_maxima(h), (a, b, c)


def test_three_maxima_planted(oracle):
    for h in ([0] * 30, [7] * 30, [20, 2, 2, 1] + [0] * 26, [20, 1, 1] + [0] * 27, [1, 2, 20] + [0] * 27, [5, 5, 5, 5] + [0] * 26,
              [0] * 26 + [5, 5, 5, 5], [30, 3, 2] + [0] * 27, [10, 1, 0] + [0] * 27, [0, 0, 9, 0, 9, 1, 9, 9] + [0] * 22):
        assert oracle.three_maxima(h) == mm.three_maxima(h), h
    assert mm.three_maxima([20, 2, 2] + [0] * 27) == (0, 1, 2) and mm.three_maxima([20, 2, 2] + [0] * 27, "maxima_le") == (0, -1, -1)
    assert mm.three_maxima([5, 5, 5, 5] + [0] * 26) == (0, 1, 2) and mm.three_maxima([5, 5, 5, 5] + [0] * 26, "maxima_later") == (3, 2, 1)


def test_rotation_bin():
    """float32 and C round: ties exist and go away from zero; -0.0 is not negative; a negative difference wraps"""
    assert len(ms.tie_rots()) >= 3
    for r in ms.tie_rots():
        assert mm.rot_bin(r, 0.0) == mm.rot_bin(r, 0.0, "rot_half_even") + 1
    assert mm.rot_bin(-0.0, 0.0) == 0 and mm.rot_bin(0.0, 30.0) == 11 and mm.rot_bin(359.99, 0.0) == 12 and mm.rot_bin(45.0, 0.0) == 2


# ---- the node-walk matchers ------------------------------------------------------------------------------------------------------
NODE_WRONG = {
    "bow": ["th_strict", "ratio_le", "ratio_double", "second_cut", "tie_last", "rot_half_even", "rot_no_wrap", "maxima_le", "maxima_later"],
    "bowkf": ["th_strict", "ratio_le", "ratio_double", "second_cut", "tie_last", "rot_half_even", "rot_no_wrap", "maxima_le", "maxima_later"],
    "tri": ["th_strict", "tri_first", "rot_half_even", "rot_no_wrap", "maxima_le", "maxima_later"],
}
NODE_INDISTINGUISHABLE = {
    ("bow", "tie_index"): "a node's feature list is ascending (FeatureVector::addFeature in keypoint order), so the first of equal distances is the "
                          "lowest index",
    ("bowkf", "tie_index"): "the same",
    ("tri", "tie_index"): "the same; and the rule here is the last of equal distances (tri_first is the variant)",
    ("tri", "tie_last"): "the rule itself: `if(dist>TH_LOW || dist>bestDist) continue;` lets an equal distance replace the best",
    ("bow", "count_slots"): "a matched frame feature is skipped by every later query, so every match and every histogram entry is a slot of its own",
    ("bowkf", "count_slots"): "every query writes its own entry of vpMatches12 at most once",
    ("tri", "count_slots"): "every query writes its own entry of vMatches12 at most once",
}
NODE_SCENES = [(k, n) for k in ms.NODE_KINDS for n in ["base"] + [h for h in ms.HISTOGRAMS if ms.node_histogram_applies(h, k)]]


def _node_scene(kind, name):
    return ms.node_scene(kind) if name == "base" else ms.node_histogram_scene(kind, name)


@pytest.mark.parametrize("kind,name", NODE_SCENES)
def test_node_oracle_equals_model(oracle, kind, name):
    sc = _node_scene(kind, name)
    for cfg in ms.node_configs(kind):
        for check_ori in (True, False):
            got, want = ms.run_node_oracle(oracle, sc, cfg, check_ori), ms.run_node_model(sc, cfg, check_ori)
            assert ms.same(got, want), "%s %s %s ori=%d: nmatches %d, model %d, entries %s differ" % (
                kind, name, cfg, check_ori, got[0], want[0], np.flatnonzero(got[1] != want[1])[:5])
    assert ms.run_node_model(sc, ms.NODE_MAIN[kind])[0] >= 20, "a matcher that matches nothing cannot pass"


@pytest.mark.parametrize("kind,wrong", [(k, w) for k in ms.NODE_KINDS for w in NODE_WRONG[k]])
def test_node_wrong_variant_is_rejected(kind, wrong):
    hits = [(name, cfg) for k, name in NODE_SCENES if k == kind for cfg in ms.node_configs(kind)
            if not ms.same(ms.run_node_model(_node_scene(kind, name), cfg, True, wrong), ms.run_node_model(_node_scene(kind, name), cfg))]
    assert hits, "%s: no scene tells %s (%s) from the rule" % (kind, wrong, mm.WRONG[wrong])


def test_node_variant_lists_are_complete():
    """a variant neither listed nor explained names a comparison the matcher does not have: it changes nothing"""
    for kind in ms.NODE_KINDS:
        for w in set(mm.WRONG) - set(NODE_WRONG[kind]) - {w for k, w in NODE_INDISTINGUISHABLE if k == kind}:
            sc = ms.node_scene(kind)
            assert all(ms.same(ms.run_node_model(sc, cfg, True, w), ms.run_node_model(sc, cfg)) for cfg in ms.node_configs(kind)), (kind, w)


@pytest.mark.parametrize("kind", ms.NODE_KINDS)
def test_node_probe_counts(kind):
    sc = ms.node_scene(kind)
    p = ms.node_probe(sc, None if kind == "tri" else 0.5)
    print(kind, p)
    assert p["queries"] >= 20 and p["best_eq_th"] > 0 and p["best_eq_th1"] > 0, p
    if kind != "tri":
        assert p["ratio_equal"] > 0 and p["ratio_near"] > 0 and ms.node_probe(sc, 0.9)["ratio_near"] > 0, p


def test_epipole_and_epipolar_sites():
    """the triangulation scene's geometric sites sit where they claim to"""
    sc = ms.node_scene("tri")
    f = np.float32
    d2 = (f(ms.EPIPOLE[0]) - sc["kps2"]["x"]) ** 2 + (f(ms.EPIPOLE[1]) - sc["kps2"]["y"]) ** 2
    assert (d2 == f(100)).sum() == 1 and ((d2 < f(100)) & (d2 > f(99.99))).sum() == 1
    k1 = np.zeros(1, sc["kps1"].dtype)[0]; k1["y"] = 50.0
    k2 = k1.copy()
    k2["y"] = 51.95; inside = mm.epipolar_ok(k1, k2, ms.F12_HORIZONTAL, 1.0)
    k2["y"] = 51.96; outside = mm.epipolar_ok(k1, k2, ms.F12_HORIZONTAL, 1.0)
    assert inside and not outside


@pytest.mark.parametrize("kind", ms.KINDS)
def test_chain_positions(kind):
    """the chain sites of the `positions` scenes sit where the kernels change rounds: the first query of a chain at 63 and at 1023"""
    sc = ms.window_scene(kind, True)
    names = sc["names"]
    for at, tag in ((63, "at 64: "), (1023, "at 1024: ")):
        assert names[at].startswith(tag + "chain") and names[at + 1] == names[at], (kind, at, names[at], names[at + 1])
    starts = [i for i in range(len(names)) if "chain" in names[i] and names[i].startswith("at ") and (i == 0 or names[i - 1] != names[i])]
    assert all(i % 64 == 63 for i in starts) and len(starts) >= 4
    assert len(sc["s_kps"]) < 400, "the searched frame stays small"
