"""Planted scenes for ORBVocabulary::transform (tests/bow_model.py): vocabularies in the layout of synth.random_vocabulary and descriptor
sets at the sizes where bow_assemble_kernel (eorb_slam_amd/csrc/match.hip) changes shape -- P, the power of two >= max(n, 64), picks
the register class M of block_bitonic_sort_regs: M = 1 up to n = 1024, 2 up to 2048, 4 up to 4096, 8 up to 8192 -- and at the edges
of the descent.  Every scene names the probe condition it exists for (Scene.cond, a function of the model's probe);
tests/test_oracle_bow_model.py asserts it, so a scene that stops exercising its path is a failing test, not a quiet one.

Vocabularies:
  v10      10 children, 4 levels, no stopped word (10 000 words)
  v10s     v10 with a third of its words stopped
  ragged   2..7 children, 5 levels, branches that end early (the short-leaf choice of bow_model)
  wide     2 levels; the root has 130 children, which have 65, 96 and 130 children in turn (bow_descend_kernel's child loop strides
           by 64: two and three rounds, with 1, 32 and 2 lanes in the last)
  tie      4 children, 4 levels; on every level the second child of a node carries the descriptor of the first
  stopped  10 children, 3 levels, every word stopped (m = 0)
  one(w)   v10 with every word but w stopped (m = 1)

Fills of the size scenes: `sparse` draws noisy copies of a small pool of v10s leaves, so that about a third of the features are stopped
all through the order (the sentinels interleave before the sort) and words repeat (runs of several lengths); `oneword` puts every
feature on one word and one node (one run of n: the longest serial addWeight loop); `many` takes the descriptors of distinct leaves
without replacement (more than P / 2 distinct words: the upper half of every output array)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_model as bm                                       # noqa: E402
from eorb_slam_amd import synth                              # noqa: E402

SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192)
PAIRS = ((0, 1), (1, 0), (2, 2), (3, 1), (0, 0))             # (weighting, norm), those of test_gpu_parity.py::test_bow_transform
ALL_PAIRS_AT = (65, 2049, 4097)
AFTER_LARGER = {65: 127, 2049: 4095, 8192: None}             # the next larger size of SIZES (8192 has none: a second 8192 call of another fill)
MAX_FEATURES = 8192


def planted_vocabulary(fanout, L, seed, dup_second=False):
    """A tree in the layout of synth.random_vocabulary with fanout(level, index among the level's nodes) children per node; children
    are near copies of their parent.  dup_second: every node's second child carries the first child's descriptor."""
    rng = np.random.default_rng(seed)
    desc, children, frontier = [rng.integers(0, 256, 32, dtype=np.uint8)], [[]], [0]
    for lv in range(1, L + 1):
        nxt = []
        for at, u in enumerate(frontier):
            for c in range(fanout(lv, at)):
                d = desc[u] ^ np.packbits(rng.uniform(size=256) < (0.25 / lv))
                if dup_second and c == 1:
                    d = desc[children[u][0]].copy()
                desc.append(d); children.append([])
                children[u].append(len(desc) - 1); nxt.append(len(desc) - 1)
        frontier = nxt
    n = len(desc)
    perm = np.concatenate([[0], 1 + rng.permutation(n - 1)])                # node ids are not contiguous per parent; the root stays 0
    inv = np.empty(n, np.int64); inv[perm] = np.arange(n)
    child_off, child_ids = [0], []
    for new in range(n):
        child_ids.extend(int(inv[c]) for c in children[perm[new]]); child_off.append(len(child_ids))
    is_leaf = np.array([len(children[perm[i]]) == 0 for i in range(n)])
    word_id = np.full(n, -1, np.int32); word_id[is_leaf] = rng.permutation(int(is_leaf.sum())).astype(np.int32)
    weight = np.zeros(n, np.float64); weight[is_leaf] = rng.uniform(0.5, 9.0, int(is_leaf.sum()))
    return dict(L=L, child_off=np.array(child_off, np.int32), child_ids=np.array(child_ids, np.int32),
                node_desc=np.stack([desc[perm[i]] for i in range(n)]), word_id=word_id, weight=weight)


def _reweighted(voc, weight):
    out = dict(voc); out["weight"] = weight
    return out


@functools.lru_cache(maxsize=None)
def vocabulary(name):
    if name == "v10":
        return synth.random_vocabulary(10, 4, seed=41, stop_frac=0)
    if name == "v10s":
        v = vocabulary("v10")
        w = v["weight"].copy(); w[np.random.default_rng(42).uniform(size=len(w)) < 1 / 3] = 0.0
        return _reweighted(v, w)
    if name == "ragged":
        return synth.random_vocabulary(7, 5, seed=10, ragged=True)
    if name == "wide":
        return planted_vocabulary(lambda lv, at: 130 if lv == 1 else (65, 96, 130)[at % 3], 2, seed=43)
    if name == "tie":
        return planted_vocabulary(lambda lv, at: 4, 4, seed=44, dup_second=True)
    if name == "stopped":
        v = synth.random_vocabulary(10, 3, seed=45, stop_frac=0)
        return _reweighted(v, np.zeros_like(v["weight"]))
    if name.startswith("one:"):                                             # every word but one stopped
        v = vocabulary("v10")
        leaf = int(name[4:])
        w = np.zeros_like(v["weight"]); w[leaf] = v["weight"][leaf]
        return _reweighted(v, w)
    raise KeyError(name)


def leaves(voc):
    return np.flatnonzero(voc["word_id"] >= 0)


def _noisy(voc, rng, picks, p=0.04):
    return voc["node_desc"][picks] ^ np.packbits(rng.uniform(size=(len(picks), 256)) < p, axis=1)


class Scene:
    """name; voc: a name for vocabulary(); desc (n x stride); levelsup; pairs: the (weighting, norm) pairs; what / cond: the probe
    condition the scene exists for, in words and as a function of the probe; tags: what selects it in the tests"""

    def __init__(self, name, voc, desc, levelsup, pairs, what, cond, **tags):
        self.name, self.voc_name, self.desc, self.levelsup, self.pairs, self.what, self.cond, self.tags = name, voc, desc, levelsup, pairs, what, cond, tags
        self.n = len(desc)

    @property
    def voc(self):
        return vocabulary(self.voc_name)

    def __repr__(self):
        return self.name


def _size_scene(n, fill):
    rng = np.random.default_rng(1000 + n)
    P, M = bm.sort_size(n)
    pairs = PAIRS if n in ALL_PAIRS_AT else PAIRS[:1]
    if fill == "sparse":
        voc = vocabulary("v10s")
        k = max(3, n // 3)                                                  # the pool: a third of it stopped words
        lv = leaves(voc)
        is_stopped = voc["weight"][lv] == 0
        pool = np.concatenate([rng.choice(lv[is_stopped], k // 3, replace=False), rng.choice(lv[~is_stopped], k - k // 3, replace=False)])
        desc = _noisy(voc, rng, rng.choice(pool, n))
        if n < 63:                                                          # (one or two features: nothing to spread)
            return Scene("sparse-%d" % n, "v10s", desc, 1, pairs, "M = 1", lambda p: p["M"] == 1, n=n, fill=fill)
        lo, hi = n // 6, n // 2
        return Scene("sparse-%d" % n, "v10s", desc, 1, pairs, "M = %d; %d..%d of %d features stopped, a word seen three times or more" % (M, lo, hi, n),
                     lambda p: p["M"] == M and lo <= p["n"] - p["m"] <= hi and p["longest_word_run"] >= 3 and (n < 1023 or p["nodes"] < p["words"]), n=n, fill=fill)
    if fill == "oneword":
        voc = vocabulary("v10")
        leaf = int(rng.choice(leaves(voc)))
        desc = np.repeat(voc["node_desc"][leaf][None], n, axis=0)
        bit = rng.integers(0, 257, n)                                       # one flipped bit, or none: 257 different descriptors
        for i in np.flatnonzero(bit < 256):
            desc[i, bit[i] >> 3] ^= np.uint8(1 << (bit[i] & 7))
        return Scene("oneword-%d" % n, "v10", desc, 1, pairs, "M = %d; one word, one node: a run of n" % M,
                     lambda p: p["M"] == M and p["m"] == n and p["words"] == 1 and p["nodes"] == 1 and p["longest_word_run"] == n and p["longest_node_run"] == n,
                     n=n, fill=fill)
    voc = vocabulary("v10")
    desc = voc["node_desc"][rng.choice(leaves(voc), n, replace=False)].copy()
    need = n // 2 if n >= 64 else 0
    return Scene("many-%d" % n, "v10", desc, 1, pairs, "M = %d; more than %d words" % (M, need),
                 lambda p: p["M"] == M and p["m"] == n and p["words"] > need and (n < 1023 or p["nodes"] < p["words"]), n=n, fill=fill)


def _edge_scenes(n):
    rng = np.random.default_rng(2000 + n)
    v10 = vocabulary("v10")
    lv = leaves(v10)
    out = []
    st = vocabulary("stopped")
    out.append(Scene("edge-m0-%d" % n, "stopped", _noisy(st, rng, rng.choice(leaves(st), n)), 1, PAIRS, "every word stopped: m = 0",
                     lambda p: p["m"] == 0 and p["words"] == 0 and p["nodes"] == 0, n=n, fill="edge"))
    keep = int(lv[7])
    others = lv[lv != keep]
    for tag, at in (("m1", n // 3), ("last", n - 1)):
        desc = v10["node_desc"][rng.choice(others, n)].copy()
        desc[at] = v10["node_desc"][keep]
        out.append(Scene("edge-%s-%d" % (tag, n), "one:%d" % keep, desc, 1, PAIRS[:1], "only feature %d kept: m = 1" % at,
                         lambda p: p["m"] == 1 and p["words"] == 1 and p["nodes"] == 1, n=n, fill="edge", kept=at))
    return out


@functools.lru_cache(maxsize=None)
def scenes():
    out = [_size_scene(n, fill) for n in SIZES for fill in ("sparse", "oneword", "many")]
    for n in (2049, 4097):
        out += _edge_scenes(n)
    rng = np.random.default_rng(3000)
    v10s = vocabulary("v10s")
    base = _noisy(v10s, rng, rng.choice(leaves(v10s), 130))
    for stride in (32, 40, 61):                                             # load_desc32's unaligned path: rows at 61-byte steps
        desc = rng.integers(0, 256, (130, stride), dtype=np.uint8); desc[:, :32] = base
        out.append(Scene("stride-%d" % stride, "v10s", desc, 1, PAIRS[:1], "row stride %d, noise past byte 32" % stride,
                         lambda p: p["m"] > 40, stride=stride))
    rag = vocabulary("ragged")
    L = int(rag["L"])
    desc = _noisy(rag, rng, rng.choice(leaves(rag), 300), 0.08)
    for levelsup in (0, 1, L - 1, L, L + 2):
        short = levelsup in (0, 1)                                          # a branch that ends on level 2 or 3 lies above level L - levelsup
        out.append(Scene("levels-%d" % levelsup, "ragged", desc, levelsup, PAIRS[:1],
                         "ragged tree, levelsup %d: %s" % (levelsup, "a leaf above the nid level" if short else "no level left: node 0" if levelsup >= L else "nid on level 1"),
                         (lambda p: p["short_leaf"] and p["nodes"] > 1) if short else (lambda p: p["nodes"] == 1) if levelsup >= L else (lambda p: not p["short_leaf"] and p["nodes"] > 1),
                         levels=True))
    wide = vocabulary("wide")
    out.append(Scene("wide", "wide", _noisy(wide, rng, rng.choice(leaves(wide), 200), 0.08), 1, PAIRS[:1], "a node of more than 128 children",
                     lambda p: p["widest"] > 128 and p["nodes"] > 64, wide=True))
    tie = vocabulary("tie")
    out.append(Scene("tie", "tie", _noisy(tie, rng, rng.choice(leaves(tie), 200), 0.02), 2, PAIRS[:1], "a descent tie", lambda p: p["tie"], tie=True))
    assert len({s.name for s in out}) == len(out)
    return tuple(out)


def scene(name):
    return next(s for s in scenes() if s.name == name)


def cases():
    """(scene, weighting, norm) of every scene"""
    return [(s, w, nrm) for s in scenes() for w, nrm in s.pairs]


def case_id(c):
    return "%s-w%dn%d" % (c[0].name, c[1], c[2])


@functools.lru_cache(maxsize=None)
def _walked(name, wrong=None):
    s = scene(name)
    return bm.descend(s.voc, s.desc, s.levelsup, wrong)


@functools.lru_cache(maxsize=None)
def want(name, weighting, norm, wrong=None):
    """the model's answer for a scene: computed once, shared by the tests; the descent is shared by a scene's (weighting, norm) pairs"""
    s = scene(name)
    walk_wrong = wrong if wrong in ("tie_last_child", "nid_level_off_by_one", "short_leaf_nid_is_leaf") else None
    return bm.transform(s.voc, s.desc, s.levelsup, weighting, norm, wrong, walked=_walked(name, walk_wrong))


def same(got, exp):
    """None if the five outputs agree bit for bit, else the name of the first that does not"""
    gw, gv, gfv, gwo, gno = got[:5]
    ew, ev, efv, ewo, eno = exp[:5]
    pairs = (("word_of", gwo, ewo), ("node_of", gno, eno), ("bow_word", gw, ew), ("bow_val", np.asarray(gv, np.float64).view(np.uint64), np.asarray(ev, np.float64).view(np.uint64)),
             ("fv_node", gfv[0], efv[0]), ("fv_off", gfv[1], efv[1]), ("fv_idx", gfv[2], efv[2]))
    for what, g, e in pairs:
        g, e = np.asarray(g), np.asarray(e)
        if g.shape != e.shape or not np.array_equal(g.astype(np.int64) if g.dtype != np.uint64 else g, e.astype(np.int64) if e.dtype != np.uint64 else e):
            return what
    return None


# the scene that tells each wrong variant of bow_model.WRONG from the rule: (scene, weighting, norm)
CAUGHT_BY = {
    "tie_last_child": ("tie", 0, 1),
    "nid_level_off_by_one": ("levels-1", 0, 1),
    "short_leaf_nid_is_leaf": ("levels-0", 0, 1),
    "stopped_kept_in_fv": ("sparse-65", 0, 1),
    "idf_accumulates": ("sparse-65", 2, 2),
    "count_times_w": ("oneword-65", 0, 0),
    "norm_in_feature_order": ("sparse-2049", 0, 1),
    "tf_unnormalised_not_divided": ("sparse-65", 1, 0),
    "fv_keyed_by_word": ("sparse-65", 0, 1),
}
