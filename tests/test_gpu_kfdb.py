"""GPU parity of the device KeyFrameDatabase (eorb_kfdb_*) with the CPU restatement of the reference's (tests/kfdb_ref: real inverted
lists, per-keyframe query / words / score members, L1Scoring::score with its lower_bound jumps).  Every comparison is an equality of
bytes: float and integer arrays as their bits, the stored scores of both families after every query.

Non-vacuity: every generated case asserts, on the restatement's side, that its queries score something, that at least one of them lists a
keyframe it does not score, and that across its queries at least one stale score (written by an earlier query, the neighbour listed but
under the threshold now) is added.  A database of one keyframe cannot list what it does not score, and a keyframe alone has no neighbour:
K = 1 asserts only that the keyframe is scored."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfdb_ref                                     # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

pytestmark = pytest.mark.gpu

E_CAPACITY, E_ARG = -3, -4
RELOC, PLACE = 0, 1
ARRAYS = ("slot", "si", "words", "acc", "best_slot", "keep", "sorted_acc", "sorted_best_slot")
COUNTS = ("n_listed", "n_scored", "max_common_words")


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


def _same(got, want, what):
    """device result against the restatement's, as bytes"""
    for k in COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.float32(got["best_acc"]).tobytes() == np.float32(want["best_acc"]).tobytes(), (what, "best_acc", got["best_acc"], want["best_acc"])
    for k in ARRAYS:
        assert (k in got) == (k in want), (what, k)
        if k in want:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])


class Pair:
    """the device database and the restatement, driven together"""

    def __init__(self, fe, ctx, vocab_words):
        self.dev = fe.KeyFrameDatabase(ctx)
        self.dev.clear()
        self.ref = kfdb_ref.KeyFrameDatabase(vocab_words)
        self.stale = 0; self.unscored = 0; self.scored = 0

    def add(self, vectors):
        got = self.dev.add_many(vectors).tolist()
        want = [self.ref.add(w, v) for w, v in vectors]
        assert got == want
        return got

    def erase(self, slot):
        self.dev.erase(slot); self.ref.erase(slot)

    def scores_same(self, what):
        for fam in (RELOC, PLACE):
            assert self.dev.scores(fam).tobytes() == self.ref.scores(fam).tobytes(), (what, "stored scores", fam)

    def query(self, nbest, q, covis=None, exclude=None, what=""):
        assert self.dev.n_slots == self.ref.n_slots
        if nbest:
            want = self.ref.detect_nbest_candidates(q["word"], q["val"], exclude=exclude, covis=covis)
            got = self.dev.detect_nbest_candidates(q["word"], q["val"], exclude=exclude, covis=covis)
        else:
            want = self.ref.detect_relocalization_candidates(q["word"], q["val"], covis=covis)
            got = self.dev.detect_relocalization_candidates(q["word"], q["val"], covis=covis)
        self.stale += want.pop("stale")
        self.scored += want["n_scored"]
        self.unscored += want["n_listed"] - want["n_scored"]
        _same(got, want, what)
        self.scores_same(what)
        return want


def _slots_table(covis, slots, n_slots):
    """the generator's covisibility table (keyframe indices) as the database's (slot ids, one row per slot)"""
    t = np.full((n_slots, 10), -1, np.int32)
    m = np.full(len(covis) + 1, -1, np.int32)
    for k, s in enumerate(slots):
        if s is not None:
            m[k] = s
    for k, s in enumerate(slots):
        if s is not None:
            t[s] = m[covis[k]]                         # (-1 indexes the spare last entry: -1)
    return t


# vector lengths on both sides of the wavefront and of nothing: 0, 1, 63, 64, 65 and a few hundred words
KF_WORDS = [64, 0, 1, 63, 65, 300, 40, 200]
QUERY_WORDS = [64, 1, 65, 64]
# K -> seed for which the conditions in the module docstring hold (checked on the restatement, which needs no GPU)
CASES = {1: 11, 3: 100, 63: 13, 64: 14, 65: 15, 257: 16}


@functools.lru_cache(maxsize=None)
def _case(K):
    kw = [KF_WORDS[k % len(KF_WORDS)] if k % 3 == 0 else 64 + (k * 7) % 23 for k in range(K)]
    if K <= 3:
        kw = [64, 40, 65][:K]
    return synth.bow_database(CASES[K], K, vocab_words=700, words_per_kf=64, nplaces=3, nqueries=len(QUERY_WORDS), kf_words=kw,
                              query_words=QUERY_WORDS)


@pytest.mark.parametrize("K", sorted(CASES))
def test_queries_match_the_restatement(fe, ctx, K):
    d = _case(K)
    p = Pair(fe, ctx, d["vocab_words"])
    slots = p.add(d["kfs"])
    assert slots == list(range(K)) and p.dev.info() == (K, K)
    covis = _slots_table(d["covis"], slots, K)
    rng = np.random.default_rng(K)
    exclude = (rng.uniform(size=K) < 0.15).astype(np.uint8)
    for i, q in enumerate(d["queries"]):
        # both families, with and without the covisibility table; the queries without it still write the stored scores
        p.query(0, q, covis, what=(K, i, "reloc"))
        p.query(1, q, covis, exclude, what=(K, i, "nbest"))
        p.query(0, q, None, what=(K, i, "reloc, no covis"))
        p.query(1, q, None, exclude, what=(K, i, "nbest, no covis"))
        p.query(1, q, covis, None, what=(K, i, "nbest, no exclude"))
    assert p.scored > 0
    if K > 1:
        assert p.unscored > 0 and p.stale > 0, (p.unscored, p.stale)


def test_sequence_with_adds_and_an_erase(fe, ctx):
    d = _case(65)
    p = Pair(fe, ctx, d["vocab_words"])
    K = 65
    slots = [None] * K
    cov = lambda: _slots_table(d["covis"], slots, p.ref.n_slots)      # noqa: E731
    for k, s in zip(range(40), p.add(d["kfs"][:40])):
        slots[k] = s
    q = d["queries"]
    p.query(0, q[0], cov(), what="first 40")
    p.query(1, q[0], cov(), what="first 40")
    for k in range(40, K):                              # one add(pKF) at a time
        slots[k] = p.add([d["kfs"][k]])[0]
    p.query(0, q[1], cov(), what="all")
    p.query(1, q[1], cov(), what="all")
    for k in (3, 17, 64):
        p.erase(slots[k]); slots[k] = None
    assert p.dev.info() == (K - 3, K)
    r = p.query(0, q[2], cov(), what="after erase")
    assert not set(r["slot"].tolist()) & {3, 17, 64}
    p.query(1, q[2], cov(), what="after erase")
    # the erased keyframes come back in another order: slots are reused lowest first, and they are now last in every list
    for k, s in zip((64, 3, 17), (3, 17, 64)):
        slots[k] = p.add([d["kfs"][k]])[0]
        assert slots[k] == s
    for i in (0, 1, 2, 3):
        p.query(i & 1, q[i], cov(), what=("after re-add", i))
    assert p.scored > 0 and p.unscored > 0 and p.stale > 0
    with pytest.raises(fe.EorbError) as e:
        p.dev.erase(K + 5)
    assert e.value.code == E_ARG
    p.dev.erase(7)
    with pytest.raises(fe.EorbError) as e:
        p.dev.erase(7)
    assert e.value.code == E_ARG


def test_pool_reallocation_keeps_the_earlier_keyframes(fe):
    """the debug hook makes the first pools 2 slots and 128 words: nine adds cross several growths of both, one of them with erased
    vectors to drop; after each the database answers as the restatement does"""
    c = fe.Context()
    try:
        c.debug_option("kfdb_initial_slots", 2)
        d = _case(63)
        p = Pair(fe, c, d["vocab_words"])
        q = d["queries"][0]
        kfs = [d["kfs"][k] for k in range(63) if len(d["kfs"][k][0]) >= 40][:9]
        caps = set()
        for k, v in enumerate(kfs):
            p.add([v])
            if k == 4:
                p.erase(1); p.erase(2)
            caps.add((c.debug_counter("kfdb_slot_cap"), c.debug_counter("kfdb_word_cap")))
            p.query(k & 1, q, np.full((p.ref.n_slots, 10), -1, np.int32), what=("growth", k))
        assert min(caps) == (2, 128) and len({s for s, _ in caps}) >= 3 and len({w for _, w in caps}) >= 2, caps
        p.erase(0); p.erase(4)
        assert p.add(kfs[:3]) == [0, 4, 7]              # K > 1 in one call, two of them into the freed slots
        assert p.scored > 0
        p.query(0, q, None, what="after growth")
    finally:
        c.close()


def test_scored_list_sorted_in_global_memory(fe):
    """past 4096 scored keyframes the last kernel sorts in global memory, not in LDS: the debug hook moves that threshold to 4, so the
    257-keyframe case takes the other path with its scored lists of 5 to 43 entries"""
    c = fe.Context()
    try:
        c.debug_option("kfdb_finish_lds_entries", 4)
        d = _case(257)
        p = Pair(fe, c, d["vocab_words"])
        slots = p.add(d["kfs"])
        covis = _slots_table(d["covis"], slots, 257)
        longest = 0
        for i, q in enumerate(d["queries"]):
            longest = max(longest, p.query(0, q, covis, what=("global sort, reloc", i))["n_scored"],
                          p.query(1, q, covis, what=("global sort, nbest", i))["n_scored"])
        assert longest > 32 and p.unscored > 0 and p.stale > 0
    finally:
        c.close()


def test_clear_empty_and_no_shared_word(fe, ctx):
    d = _case(3)
    p = Pair(fe, ctx, d["vocab_words"])
    q = d["queries"][0]
    r = p.dev.detect_relocalization_candidates(q["word"], q["val"])          # empty database
    assert r["n_listed"] == 0 and r["n_scored"] == 0 and len(r["slot"]) == 0
    p.add(d["kfs"])
    used = np.unique(np.concatenate([w for w, _ in d["kfs"]]))
    free = np.setdiff1d(np.arange(d["vocab_words"]), used)[:5].astype(np.uint32)
    for nbest in (0, 1):
        r = p.query(nbest, dict(word=free, val=np.full(5, 0.2)), np.full((3, 10), -1, np.int32), what="no shared word")
        assert r["n_listed"] == 0 and r["n_scored"] == 0 and r["max_common_words"] == 0 and len(r["slot"]) == 0
    r = p.query(0, dict(word=np.zeros(0, np.uint32), val=np.zeros(0)), None, what="empty query")
    assert r["n_listed"] == 0
    p.query(0, q, None, what="before clear")
    p.dev.clear(); p.ref.clear()
    assert p.dev.info() == (0, 0)
    assert p.dev.detect_relocalization_candidates(q["word"], q["val"])["n_listed"] == 0
    assert p.add(d["kfs"][:2]) == [0, 1]
    p.query(0, q, None, what="after clear")
    assert p.dev.scores(PLACE).tolist() == [0.0, 0.0]   # add starts both stored scores at 0


def test_capacity_and_argument_errors(fe, ctx):
    d = _case(65)
    p = Pair(fe, ctx, d["vocab_words"])
    p.add(d["kfs"])
    q = d["queries"][0]
    want = p.ref.detect_relocalization_candidates(q["word"], q["val"])
    assert want["n_scored"] >= 2
    with pytest.raises(fe.EorbError) as e:
        p.dev.detect_relocalization_candidates(q["word"], q["val"], cap=want["n_scored"] - 1)
    assert e.value.code == E_CAPACITY and e.value.n_scored == want["n_scored"]
    p.scores_same("cap too small")                      # the stored scores are the query's all the same
    got = p.dev.detect_relocalization_candidates(q["word"], q["val"], cap=want["n_scored"])
    want.pop("stale")
    _same(got, want, "cap exact")
    # word ids that do not ascend strictly: the add names the keyframe and adds nothing
    w, v = d["kfs"][0]
    bad = w.copy(); bad[5] = bad[4]
    with pytest.raises(fe.EorbError) as e:
        p.dev.add_many([(w, v), (bad, v), (w, v)])
    assert e.value.code == E_ARG and "keyframe 1" in str(e.value)
    assert p.dev.info() == (65, 65)
    with pytest.raises(fe.EorbError) as e:
        p.dev.detect_nbest_candidates(bad, v)
    assert e.value.code == E_ARG
    with pytest.raises(fe.EorbError) as e:
        p.dev.scores(2)
    assert e.value.code == E_ARG


def test_query_at_and_past_the_staging_limit(fe, ctx):
    limit = fe.KeyFrameDatabase.MAX_QUERY_WORDS
    d = synth.bow_database(21, 65, vocab_words=6000, words_per_kf=300, nplaces=3, nqueries=1, query_words=[limit])
    p = Pair(fe, ctx, d["vocab_words"])
    slots = p.add(d["kfs"])
    covis = _slots_table(d["covis"], slots, 65)
    q = d["queries"][0]
    assert len(q["word"]) == limit
    for nbest in (0, 1):
        r = p.query(nbest, q, covis, what="query at the limit")
        assert 0 < r["n_scored"] < r["n_listed"]
    rest = np.setdiff1d(np.arange(6000), q["word"])[:1]
    w = np.sort(np.concatenate([q["word"], rest.astype(np.uint32)])); v = np.full(limit + 1, 1.0 / (limit + 1))
    for f in (p.dev.detect_relocalization_candidates, p.dev.detect_nbest_candidates):
        with pytest.raises(fe.EorbError) as e:
            f(w, v)
        assert e.value.code == E_CAPACITY


def test_chain_transform_query_search_by_bow(oracle, fe, ctx):
    """Tracking::Relocalization (src/Tracking.cc:2641-2700) on the device: eorb_bow_transform of the frame, eorb_kfdb_detect_reloc on a
    database filled from eorb_bow_transform of the keyframes, eorb_search_by_bow_keyframes on the kept candidates -- against the same chain
    on the CPU: the oracle's transform and matcher, the restatement's query"""
    K = 6
    voc = synth.random_vocabulary(10, 3, seed=9)
    s = synth.bow_neighbourhood(77, K, npts=120, ndistract=30, nnodes=10)
    V = fe.ORBVocabulary(voc, 0, 1, ctx=ctx)
    nwords = int(np.max(voc["word_id"])) + 1
    p = Pair(fe, ctx, nwords)
    dev_kf, cpu_kf = [], []
    for kf in s["kfs"]:
        bw, bv, fv = V.transform(kf["desc"], 1)
        ow, ov, ofv, _, _ = oracle.bow_transform(voc, kf["desc"], 1, 0, 1)
        assert p.dev.add(bw, bv) == p.ref.add(ow, ov)
        dev_kf.append((kf["kps"], kf["desc"], kf["has_mp"], fv)); cpu_kf.append((kf["kps"], kf["desc"], kf["has_mp"], ofv))
    covis = np.full((K, 10), -1, np.int32)
    for k in range(K):
        covis[k, :2] = [(k + 1) % K, (k + K - 1) % K]
    bw, bv, fv = V.transform(s["desc"], 1)
    ow, ov, ofv, _, _ = oracle.bow_transform(voc, s["desc"], 1, 0, 1)
    got = p.dev.detect_relocalization_candidates(bw, bv, covis)
    want = p.ref.detect_relocalization_candidates(ow, ov, covis)
    want.pop("stale")
    _same(got, want, "chain query")
    kept = lambda r: list(dict.fromkeys(int(b) for b, k in zip(r["best_slot"], r["keep"]) if k))      # noqa: E731  (:878-891, one map)
    cand = kept(want)
    assert cand and kept(got) == cand
    gn, gm = fe.SearchByBoWKeyFrames([dev_kf[k] for k in cand], s["kps"], s["desc"], fv, 0.75, True, ctx=ctx)
    for row, k in enumerate(cand):
        n, m = oracle.search_by_bow(*cpu_kf[k], s["kps"], s["desc"], ofv, 0.75, True)
        assert int(gn[row]) == n and np.asarray(gm[row], np.int32).tobytes() == m.tobytes(), k
