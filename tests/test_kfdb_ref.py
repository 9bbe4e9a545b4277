"""Known answers of the KeyFrameDatabase restatement (tests/kfdb_ref): every expected value below is derived by hand from the cited lines
of src/KeyFrameDatabase.cc and Thirdparty/DBoW2/DBoW2/ScoringObject.cpp, none from running the code.  No GPU."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfdb_ref                                     # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _db(vectors, vocab=64):
    db = kfdb_ref.KeyFrameDatabase(vocab)
    slots = [db.add(w, v) for w, v in vectors]
    return db, slots


def _uniform(words):
    """a vector with the weight 1/4, 1/8 ... (a power of two: every sum below is exact)"""
    return list(words), [1.0 / 8.0] * len(words)


NO_COVIS = np.full((0, 10), -1, np.int32)


def _covis(n, rows=None):
    c = np.full((n, 10), -1, np.int32)
    for k, r in (rows or {}).items():
        c[k, :len(r)] = r
    return c


def test_identical_l1_normalised_vectors_score_exactly_one():
    # every term is |v - v| - |v| - |v| = -2v; the weights are powers of two that sum to 1: score = -(-2)/2 = 1 exactly
    w = [3, 5, 9, 20]
    v = [0.5, 0.25, 0.125, 0.125]
    assert kfdb_ref.l1_score(w, v, w, v) == 1.0


def test_disjoint_vectors_score_minus_zero():
    # no common word: score stays 0 and -score / 2.0 = -0.0; the sign bit is part of the result
    s = kfdb_ref.l1_score([1, 3, 5], [0.5, 0.25, 0.25], [2, 4, 6, 8], [0.25, 0.25, 0.25, 0.25])
    assert _bits(s) == _bits(-0.0)
    assert _bits(kfdb_ref.l1_score([], [], [2], [1.0])) == _bits(-0.0)


def test_three_word_example_by_hand():
    # v1 = {2: 0.5, 7: 0.25, 9: 0.25}, v2 = {2: 0.25, 5: 0.5, 9: 0.25}: common words 2 and 9
    #   word 2: |0.5 - 0.25| - 0.5 - 0.25 = -0.5;  word 9: |0| - 0.25 - 0.25 = -0.5;  sum -1.0;  score = 0.5
    # (the walk: equal at 2; then 7 < 5 is false -> v2 jumps to lower_bound(7) = 9; 7 < 9 -> v1 jumps to lower_bound(9) = 9; equal)
    assert kfdb_ref.l1_score([2, 7, 9], [0.5, 0.25, 0.25], [2, 5, 9], [0.25, 0.5, 0.25]) == 0.5
    # the order of the sum is the word order.  Identical vectors: the terms are -2v.  v = (2^53, 1, 1): -2^54, then -2 twice, each half
    # an ulp (4) of 2^54 and rounded to even, i.e. lost: score = 2^53.  v = (1, 1, 2^53): -2 - 2 = -4, then -2^54 - 4 is exact: 2^53 + 2
    w = [1, 2, 3]
    assert kfdb_ref.l1_score(w, [2.0 ** 53, 1.0, 1.0], w, [2.0 ** 53, 1.0, 1.0]) == 2.0 ** 53
    assert kfdb_ref.l1_score(w, [1.0, 1.0, 2.0 ** 53], w, [1.0, 1.0, 2.0 ** 53]) == 2.0 ** 53 + 2.0


@pytest.mark.parametrize("maxw,need", [(10, 9), (5, 5)])
def test_threshold_is_a_truncated_float_product(maxw, need):
    # int minCommonWords = maxCommonWords * 0.8f: 10 -> 8 (scored from 9 words on), 5 -> 4 (only 5 words are scored)
    q = _uniform(range(maxw))
    vecs = [_uniform(range(n)) for n in range(1, maxw + 1)]          # keyframe k shares k + 1 words with the query
    db, _ = _db(vecs)
    r = db.detect_relocalization_candidates(*q)
    assert r["max_common_words"] == maxw and r["n_listed"] == maxw
    assert sorted(r["words"].tolist()) == list(range(need, maxw + 1))
    assert r["n_scored"] == maxw - need + 1


def test_first_encounter_order_follows_the_query_words_then_the_add_order():
    # A (added first) holds words {8, 9}, B {1, 9}, C {8}: the walk over the query {1, 8, 9} meets B at word 1, then A and C at word 8
    # in add order -> B, A, C although A was added before B
    db, (a, b, c) = _db([([8, 9], [0.5, 0.5]), ([1, 9], [0.5, 0.5]), ([8], [1.0])])
    r = db.detect_relocalization_candidates([1, 8, 9], [0.25, 0.5, 0.25], cap=3)
    # max = 2 -> minCommonWords = 1: C (1 word) is listed, not scored
    assert r["n_listed"] == 3 and r["slot"].tolist() == [b, a]


def test_erase_then_add_again_moves_a_keyframe_to_the_end():
    va, vb = ([4, 6], [0.5, 0.5]), ([4, 7], [0.5, 0.5])
    db, (a, b) = _db([va, vb])
    q = ([4, 6, 7], [0.5, 0.25, 0.25])
    assert db.detect_relocalization_candidates(*q)["slot"].tolist() == [a, b]
    db.erase(a)
    a2 = db.add(*va)
    assert a2 == a                                     # the lowest free slot is reused
    assert db.detect_relocalization_candidates(*q)["slot"].tolist() == [b, a]
    with pytest.raises(ValueError):
        db.erase(5)


def test_excluded_keyframe_is_neither_listed_nor_a_neighbour():
    # three keyframes share both query words; slot 1 is connected to the query keyframe.  identical vectors: si = 1 each
    v = ([2, 3], [0.5, 0.5])
    db, (s0, s1, s2) = _db([v, v, v])
    cov = _covis(3, {0: [1, 2], 2: [1]})
    ex = np.array([0, 1, 0], np.uint8)
    r = db.detect_nbest_candidates(*v, exclude=ex, covis=cov)
    assert r["n_listed"] == 2 and r["slot"].tolist() == [s0, s2]
    # slot 0 adds only slot 2 (1 + 1 = 2), slot 2 adds nothing (its only neighbour is excluded)
    assert r["acc"].tolist() == [2.0, 1.0] and r["best_slot"].tolist() == [s0, s2]
    assert db.scores(1).tolist() == [1.0, 0.0, 1.0]
    # without the exclusion all three are listed and slot 1 counts
    r = db.detect_nbest_candidates(*v, covis=cov)
    assert r["slot"].tolist() == [s0, s1, s2] and r["acc"].tolist() == [3.0, 1.0, 2.0]


def test_stale_score_of_a_listed_neighbour_under_the_threshold():
    # N = {1, 2}: 0.5 each, M = {1, 2, 3, 4, 5}: 0.125 * 5 (not normalised: exact arithmetic is all that matters here); N is M's neighbour
    N, M = ([1, 2], [0.5, 0.5]), ([1, 2, 3, 4, 5], [0.125] * 5)
    db, (n, m) = _db([N, M])
    cov = _covis(2, {m: [n]})
    # query 1 = N's vector: both share 2 words, max 2 -> min 1, both scored.  si(N) = 1; si(M): two terms |0.5 - 0.125| - 0.5 - 0.125 =
    # -0.25 -> 0.25.  acc(M) = 0.25 + 1 = 1.25 with pBestKF = N
    r = db.detect_relocalization_candidates(*N, covis=cov)
    assert r["slot"].tolist() == [n, m] and r["si"].tolist() == [1.0, 0.25]
    assert r["acc"].tolist() == [1.0, 1.25] and r["best_slot"].tolist() == [n, n] and r["stale"] == 0
    assert r["best_acc"] == 1.25 and r["keep"].tolist() == [1, 1]                   # 1.0 > 0.9375
    # query 2 = M's vector: N shares 2 words, M 5 -> min 4: N is listed but not scored, its stored score stays 1 and is what M adds:
    # si(M) = 5 * 0.125 = 0.625, acc = 1.625, pBestKF = N (1 > 0.625)
    r = db.detect_relocalization_candidates(*M, covis=cov)
    assert r["n_listed"] == 2 and r["slot"].tolist() == [m] and r["si"].tolist() == [0.625]
    assert r["acc"].tolist() == [1.625] and r["best_slot"].tolist() == [n] and r["stale"] == 1
    assert db.scores(0).tolist() == [1.0, 0.625]
    assert db.scores(1).tolist() == [0.0, 0.0]                                      # the other family is untouched


def test_equal_acc_scores_keep_list_order_under_the_sort():
    # four keyframes, si = 0.5, 1, 0.5, 1 in list order: sort(compFirst) is stable -> (1, slot 1), (1, slot 3), (0.5, slot 0), (0.5, slot 2)
    half, full = ([1, 2], [0.25, 0.25]), ([1, 2], [0.5, 0.5])
    db, s = _db([half, full, half, full])
    r = db.detect_nbest_candidates(*full, covis=_covis(4))
    assert r["si"].tolist() == [0.5, 1.0, 0.5, 1.0]
    assert r["sorted_acc"].tolist() == [1.0, 1.0, 0.5, 0.5] and r["sorted_best_slot"].tolist() == [s[1], s[3], s[0], s[2]]


def test_relocalisation_keeps_what_passes_three_quarters_of_the_best():
    # si = 1, 0.75, 0.5 without neighbours: bestAccScore 1 -> keep acc > 0.75: only the first (0.75 > 0.75 is false)
    q = ([1, 2], [0.5, 0.5])
    db, _ = _db([q, ([1, 2], [0.5, 0.25]), ([1, 2], [0.25, 0.25])])
    r = db.detect_relocalization_candidates(*q, covis=_covis(3))
    assert r["acc"].tolist() == [1.0, 0.75, 0.5] and r["keep"].tolist() == [1, 0, 0]


def test_clear_and_capacity():
    v = ([1, 2], [0.5, 0.5])
    db, _ = _db([v, v, v])
    with pytest.raises(kfdb_ref.CapacityError) as e:
        db.detect_relocalization_candidates(*v, cap=2)
    assert e.value.n_scored == 3
    db.clear()
    assert db.n_slots == 0 and db.detect_relocalization_candidates(*v)["n_listed"] == 0
    assert db.add(*v) == 0


def test_generator_cases_are_not_vacuous():
    """synth.bow_database: the 0.8 rule splits the listed keyframes and some listed neighbours are under the threshold"""
    d = synth.bow_database(3, 65, vocab_words=600, words_per_kf=64, nplaces=3, nqueries=3)
    assert d["covis"].shape == (65, 10) and (d["covis"] == -1).any() and (d["covis"] >= 0).any()
    for w, v in d["kfs"]:
        assert np.all(np.diff(w.astype(np.int64)) > 0) and abs(v.sum() - 1.0) < 1e-12 and (v > 0).all()
    db, _ = _db(d["kfs"], d["vocab_words"])
    stale = 0
    for q in d["queries"]:
        r = db.detect_relocalization_candidates(q["word"], q["val"], covis=d["covis"])
        assert 0 < r["n_scored"] < r["n_listed"]
        stale += r["stale"]
    assert stale > 0
