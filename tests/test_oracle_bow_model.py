"""The oracle's ORBVocabulary::transform against the plain model of tests/bow_model.py on the planted scenes of tests/bow_scenes.py
(CPU).  Three things: orc_bow_transform equals the model bit for bit in every output, word_of and node_of included; every scene
exercises what it exists for (its probe condition -- a failing condition is a failing test); and every wrong variant of the model is
told from the rule by the scene named for it, so the scenes can see the mistakes the model knows of."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_model as bm                              # noqa: E402
import bow_scenes as bs                             # noqa: E402

CASES = bs.cases()


@pytest.mark.parametrize("case", CASES, ids=[bs.case_id(c) for c in CASES])
def test_oracle_equals_the_model(oracle, case):
    s, weighting, norm = case
    exp = bs.want(s.name, weighting, norm)
    got = oracle.bow_transform(s.voc, s.desc, s.levelsup, weighting, norm)
    assert bs.same(got, exp) is None, "%s: %s differs (probe %s)" % (bs.case_id(case), bs.same(got, exp), exp[5])


@pytest.mark.parametrize("s", bs.scenes(), ids=[s.name for s in bs.scenes()])
def test_scene_exercises_what_it_names(s):
    for weighting, norm in s.pairs:
        p = bs.want(s.name, weighting, norm)[5]
        assert p["n"] == s.n and (p["P"], p["M"]) == bm.sort_size(s.n)
        assert s.cond(p), "%s does not show '%s': probe %s" % (s.name, s.what, p)


def test_the_sizes_cover_every_register_class_and_its_edges():
    by_m = {}
    for s in bs.scenes():
        if "fill" in s.tags:
            by_m.setdefault(bm.sort_size(s.n)[1], set()).add(s.n)
    assert sorted(by_m) == [1, 2, 4, 8]
    assert {1024, 1025, 2048, 2049, 4096, 4097, 8192} <= set().union(*by_m.values())
    assert min(by_m[2]) == 1025 and min(by_m[4]) == 2049 and min(by_m[8]) == 4097 and max(by_m[8]) == bs.MAX_FEATURES
    p = bs.want("many-8192", 0, 1)[5]
    assert p["words"] > 4096, p                                            # the upper half of every output array, run indices past 64 x 64
    assert bs.want("many-4096", 0, 1)[5]["words"] > 2048
    assert any(bs.want(s.name, 0, 1)[5]["short_leaf"] for s in bs.scenes() if "levels" in s.tags)
    assert bs.want("wide", 0, 1)[5]["widest"] > 128 and bs.want("tie", 0, 1)[5]["tie"]


@pytest.mark.parametrize("wrong", sorted(bm.WRONG))
def test_a_named_scene_catches_every_wrong_variant(wrong):
    name, weighting, norm = bs.CAUGHT_BY[wrong]
    assert (weighting, norm) in bs.scene(name).pairs
    right = bs.want(name, weighting, norm)
    bad = bs.want(name, weighting, norm, wrong)
    assert bs.same(bad, right) is not None, "%s (%s) is not told from the rule by %s" % (wrong, bm.WRONG[wrong], name)


def test_seven_additions_are_not_seven_times():
    """what lets a scene tell repeated addWeight from count x w: for most weights the two round differently"""
    import numpy as np
    w = np.random.default_rng(3).uniform(0.5, 9.0, 2000)
    acc = w.copy()
    for _ in range(6):
        acc = acc + w
    assert (acc != 7 * w).sum() > 500
