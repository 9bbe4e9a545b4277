"""The oracle's keypoint selection (oracle/orc_orb.c: cell grid, DistributeOctTree, level bookkeeping) against the list model of
tests/octree_model.py on the planted scenes of tests/octree_scenes.py (no GPU), on both oracle builds.  Every comparison is an
equality of integers; the scenes' premises (planted candidates, probe counts) are asserted before the results are compared."""
import functools

import numpy as np
import pytest

import octree_model as m
import octree_scenes as sc

BUILDS = [False, True]          # the parity build and the timing build of the oracle


def _xyr(kps, off=0):
    return [(int(x) - off, int(y) - off, int(r)) for x, y, r in zip(kps["x"], kps["y"], kps["response"])]


@functools.lru_cache(maxsize=None)
def model_cands(scene):
    return tuple(m.cell_candidates(scene.img, scene.edge, scene.ini, scene.minth))


@functools.lru_cache(maxsize=None)
def model_run(scene, N):
    _, w, h = scene.window()
    cands = model_cands(scene)
    kept, probe = m.distribute(cands, w, h, N)
    return [cands[k] for k in kept], probe


def model_frame(oracle_extractor, scene, N, lap=(0, 1000)):
    """the model's records of a whole frame: every level's image is the oracle's level buffer without its border (held byte for byte
    by tests/test_oracle_stages.py and tests/test_gpu_stages.py)"""
    E = scene.edge
    sfs = m.scale_factors(scene.sf, scene.nlevels)
    quotas = m.features_per_level(N, scene.sf, scene.nlevels)
    levels, probes = [], []
    for l in range(scene.nlevels):
        buf = oracle_extractor.level_buffer(l)
        img = buf[E:buf.shape[0] - E, E:buf.shape[1] - E]
        kps, probe, _ = m.level_keypoints(img, l, E, quotas[l], sfs[l], scene.ini, scene.minth)
        levels.append(kps)
        probes.append(probe)
    mono, recs = m.frame_keypoints(levels, sfs, lap)
    return mono, recs, levels, probes


def kept_cells_are_disjoint(cands, kept, probe, w, h):
    """No two kept keys share a final cell, stated without the list algorithm: the final nodes are pairwise disjoint boxes that tile
    nothing twice, one kept key each, and every kept key lies in its own box.  (A key that `kp.pt.x / hX` puts left of its root's integer
    edge lies beside its boxes in x, which may then shrink to no width at all: with such keys only the rows are checked.)"""
    assert len(probe["kept_nodes"]) == len(kept) == len(set(probe["kept_nodes"]))
    cover = np.zeros((h, w), np.int32)
    for (x0, x1, y0, y1), (x, y, _) in zip(probe["kept_nodes"], kept):
        assert y0 <= y < y1 and (x0 <= x < x1 or probe["root_boundary_keys"]), (x0, x1, y0, y1, x, y)
        cover[y0:y1, x0:x1] += 1
    assert cover.max() <= 1


def records(kps):
    return [(np.float32(k["x"]), np.float32(k["y"]), int(k["response"]), int(k["octave"]), int(k["size"])) for k in kps]


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", BUILDS)
def test_planted_scenes_produce_their_candidates(oracle, fast):
    """premise of every planted scene: the oracle's level-0 candidates are exactly the planted set, and in the model's order"""
    for s in sc.single_level_scenes():
        oe = oracle.OrbExtractor(imWidth=s.W, fast=fast, **s.params(50))
        assert oe.extract(s.img, want_desc=False)[0] >= 0, s
        got = _xyr(oe.level_candidates(0))
        assert sorted(got) == sorted(s.expect), "%s: %d candidates, %d planted" % (s, len(got), len(s.expect))
        assert got == list(model_cands(s)), "%s: candidate order" % s
        assert got == sc.ordered(s.W, s.H, s.edge, s.expect), "%s: cell row, cell column, raster" % s
        assert len(set((x, y) for x, y, _ in got)) == len(got)


@pytest.mark.parametrize("fast", BUILDS)
def test_distribute_equals_model_on_planted_scenes(oracle, fast):
    reached = set()
    for s, N in sc.scene_cases():
        mb, w, h = s.window()
        cands = model_cands(s)
        want, probe = model_run(s, N)
        arr = np.zeros(len(cands), oracle.KP_DTYPE)
        arr["x"], arr["y"], arr["response"] = [c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands]
        got = _xyr(oracle.distribute_octree(arr, mb, mb + w, mb, mb + h, N, fast=fast))
        assert got == want, "%s N=%d: oracle keeps %d, model %d (door %s)" % (s, N, len(got), len(want), probe["door"])
        for n_claim, text, pred in s.claims:
            if n_claim in (None, N):
                assert pred(probe), "%s N=%d does not reach: %s" % (s, N, text)
        # invariants that need no restatement
        assert set(got) <= set(cands) and len(set(got)) == len(got)
        assert len(got) <= max(N + 2, 4 * probe["nIni"]), (s, N, len(got))
        kept_cells_are_disjoint(cands, want, probe, w, h)
        reached.add(probe["door"])
        reached.update(k for k in ("cut_first_division_exit", "cut_last_division_exit", "adjacent_equal_sizes", "best_ties", "midline_keys",
                                   "root_boundary_keys", "tie_walked_same_division", "tie_walked_other_division") if probe[k])
        if probe["cut_rounds"]:
            reached.add("cut rounds: 1" if probe["cut_rounds"] == 1 else "cut rounds: 3+" if probe["cut_rounds"] >= 3 else "cut rounds: 2")
        reached.update("nIni %d" % probe["nIni"] for _ in [0])
    assert {"size >= N", "size == prevSize", "size == prevSize, divisible nodes left", "cut: size >= N", "cut: size == prevSize",
            "cut rounds: 1", "cut rounds: 3+", "cut_first_division_exit", "cut_last_division_exit", "adjacent_equal_sizes", "best_ties",
            "midline_keys", "root_boundary_keys", "tie_walked_same_division", "tie_walked_other_division", "nIni 1", "nIni 2", "nIni 3", "nIni 5", "nIni 7"} <= reached, reached


def test_separable_candidates_are_all_kept():
    """len(kept) == n when n <= N and no two candidates are so close that the list stops growing before they part: the helper
    scenes (a dense lattice around the pair) and the level-size scenes at N = n + 5"""
    names = {"column_pair_deep", "row_pair_deep", "one_px_wide"} | {"level_%d" % n for n in sc.LEVEL_SIZES if n > 2}
    seen = set()
    for s, N in sc.scene_cases():
        if s.name in names and N > len(s.expect):
            assert len(model_run(s, N)[0]) == len(s.expect), (s, N)
            seen.add(s.name)
    assert seen == names


@pytest.mark.parametrize("fast", BUILDS)
def test_distribute_equals_model_on_random_lists(oracle, fast):
    """300 random candidate lists: random window sizes (1 to 17 roots), 1 to 3 000 distinct positions, responses from 8 values (ties
    inside kept nodes everywhere), random N"""
    rng = np.random.default_rng(2025)
    doors = set()
    for it in range(300):
        w, h = int(rng.integers(40, 700)), int(rng.integers(40, 300))
        if m.n_roots(w, h) < 1:
            continue
        n = min(int(rng.integers(1, 3001 if it % 4 == 0 else 400)), w * h // 2)
        idx = rng.choice(w * h, n, replace=False)
        cands = [(int(i % w), int(i // w), int(r) * 10) for i, r in zip(idx, rng.integers(1, 9, n))]
        N = int(rng.integers(1, 2 * n + 2))
        kept, probe = m.distribute(cands, w, h, N)
        arr = np.zeros(n, oracle.KP_DTYPE)
        arr["x"], arr["y"], arr["response"] = [c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands]
        got = _xyr(oracle.distribute_octree(arr, 0, w, 0, h, N, fast=fast))
        assert got == [cands[k] for k in kept], "list %d: %dx%d, n %d, N %d: oracle keeps %d, model %d" % (it, w, h, n, N, len(got), len(kept))
        assert len(got) <= max(N + 2, 4 * probe["nIni"])
        kept_cells_are_disjoint(cands, got, probe, w, h)
        doors.add(probe["door"])
    assert len(doors) >= 4, doors


@pytest.mark.parametrize("fast", BUILDS)
def test_level_and_frame_records_equal_model(oracle, fast):
    """a sample of the single-level scenes through OrbExtractor.extract (level keypoints with the border added, octave, size, and the
    frame's output order), the multi-level frames (quotas, octave, size, scaling to level 0) and the two largest size lists"""
    sample = [(s, N) for s, N in sc.scene_cases() if s.name in ("exact_doors", "roots_7", "roots_5", "kept_tie", "weak_cell", "adjacent",
                                                                 "skipped_column", "one_px_wide", "level_513", "node_17")]
    multi = [(s, N) for s in list(sc.multilevel_scenes()) + list(sc.big_list_scenes()) for N in s.Ns]
    assert len(sample) >= 20 and len(multi) >= 5
    for s, N in sample + multi:
        oe = oracle.OrbExtractor(imWidth=s.W, fast=fast, **s.params(N))
        for lap in ((0, 1000), (60, 120)) if s.W < 700 else ((0, 1000),):
            omono, okp, _, _ = oe.extract(s.img, lap, want_desc=False)
            assert omono >= 0, (s, N, omono)
            assert oe.features_per_level == m.features_per_level(N, s.sf, s.nlevels)
            assert [float(v) for v in oe.scale_factors] == [float(v) for v in m.scale_factors(s.sf, s.nlevels)]
            mono, recs, levels, probes = model_frame(oe, s, N, lap)
            for l in range(s.nlevels):
                assert records(oe.level_keypoints(l)) == [(np.float32(x), np.float32(y), r, o, sz) for x, y, r, o, sz in levels[l]], (s, N, l)
            assert omono == mono and records(okp) == recs, (s, N, lap)
        if s.nlevels > 1:
            assert all(len(lv) > 0 for lv in levels[:3]), (s, [len(lv) for lv in levels])
        for n_claim, text, pred in s.claims:
            if n_claim in (None, N):
                assert pred(probes[0]), "%s N=%d does not reach: %s" % (s, N, text)


@pytest.mark.parametrize("fast", BUILDS)
def test_first_pass_nodes_are_all_returned(oracle, fast):
    """The first pass over nIni roots yields up to 4 * nIni nodes before the list is compared with N; the reference returns them all.
    640 x 120 (7 roots) and 1000 x 100 (14 roots) with level quotas of 1, 5 and 12, and 640 x 120 on three levels of 12 / 10 / 8."""
    counts = {}
    for s in sc.capacity_scenes():
        for N in s.Ns:
            oe = oracle.OrbExtractor(imWidth=s.W, fast=fast, **s.params(N))
            omono, okp, _, _ = oe.extract(s.img)
            assert omono == 0 and okp is not None, (s, N, omono)
            mono, recs, levels, probes = model_frame(oe, s, N)
            assert records(okp) == recs
            counts[(s.name, N)] = [len(lv) for lv in levels]
            for l, lv in enumerate(levels):
                assert len(lv) <= 4 * probes[l]["nIni"] and len(lv) > m.features_per_level(N, s.sf, s.nlevels)[l] + 8, (s, N, l, len(lv))
    assert counts[("capacity_640x120", 5)] == [28] and counts[("capacity_640x120_3levels", 30)] == [28, 28, 32], counts


def test_default_shaped_configurations_keep_their_capacity(oracle):
    """max(N + 8, 4 * nIni) per level is N + 8 on every level of the benchmark's and the suite's usual configurations (one root per
    level): their output capacity is what it has always been, nfeatures + 8 * nlevels"""
    for W, H, nf, sf, nl, E in ((240, 180, 1000, 1.2, 4, 19), (240, 180, 800, 1.0, 1, 9), (240, 180, 400, 1.0, 1, 9), (346, 260, 2000, 1.2, 8, 15),
                                (752, 480, 1200, 1.2, 8, 19)):
        oe = oracle.OrbExtractor(nf, sf, nl, 10, 0, edgeTh=E, imWidth=W)
        assert oe.L.orc_orb_max_keypoints_for(oe.h, W, H) == nf + 8 * nl == oe.cap, (W, H, nf, nl)
    oe = oracle.OrbExtractor(5, 1.0, 1, 10, 0, edgeTh=19, imWidth=640)
    assert oe.L.orc_orb_max_keypoints_for(oe.h, 640, 120) == 28 and oe.cap == 13


# ---- the constructor's quotas --------------------------------------------------------------------------------------------------
QUOTA_CONFIGS = [(nf, sf, nl) for nf in (1, 2, 5, 8, 30, 100, 500, 1000, 1200, 3000) for sf in (1.1, 1.2, 1.26, 1.5, 2.0) for nl in (1, 2, 3, 4, 8, 12)]


def test_features_per_level_equal_model(oracle):
    half, over = 0, 0
    for nf, sf, nl in QUOTA_CONFIGS:
        want = m.features_per_level(nf, sf, nl)
        assert oracle.OrbExtractor(nf, sf, nl).features_per_level == want, (nf, sf, nl)
        half += m.features_per_level(nf, sf, nl, "quota_floor") != want
        over += m.features_per_level(nf, sf, nl, "quota_last_unclamped") != want
    assert half > 100 and over >= 1, (half, over)      # (the list does tell cvRound from floor and reaches a negative remainder)


# ---- every wrong variant is rejected by a named scene ------------------------------------------------------------------------------
REJECTED_BY = {          # variant -> (scene, N): the list of oracle/README.md
    "mid_le": ("midlines", 25),
    "half_floor": ("midlines", 25),
    "root_round_half_even": ("roots_3_ratio_2p5", 40),
    "root_edge_float": ("roots_5", 77),
    "root_by_edges": ("roots_7", 28),
    "push_back_children": ("quartet_3_20_5_30", 59),
    "parent_keeps_place": ("quartet_3_20_5_30", 59),
    "n_strict": ("exact_doors", 64),
    "expand_ge": ("exact_doors", 436),
    "no_prevsize_exit": ("close_pair", 5),
    "cut_no_break": ("exact_doors", 186),
    "cut_n_strict": ("exact_doors", 186),
    "cut_smallest_first": ("exact_doors", 186),
    "size_tie_first_created": ("exact_doors", 186),
    "cut_once": ("midlines", 25),
    "best_tie_last": ("kept_tie", 1),
    "best_raster_order": ("kept_tie", 1),
    "retry_always": ("weak_cell_with_strong", 10),
    "retry_never": ("weak_cell", 10),
    "cell_order_raster": ("kept_tie", 1),
    "nms_across_cells": ("adjacent", 4),
}


def test_every_wrong_variant_is_rejected():
    assert set(REJECTED_BY) | set(m.INDISTINGUISHABLE) | {"quota_floor", "quota_last_unclamped"} == set(m.WRONG_VARIANTS)
    by_name = {s.name: s for s in sc.single_level_scenes()}
    for variant, (name, N) in REJECTED_BY.items():
        s = by_name[name]
        assert N in s.Ns, (variant, name, N)
        _, w, h = s.window()
        cands = m.cell_candidates(s.img, s.edge, s.ini, s.minth, variant)
        kept, _ = m.distribute(cands, w, h, N, variant)
        assert [cands[k] for k in kept] != model_run(s, N)[0], "%s is not told from the rule by %s at N = %d" % (variant, name, N)
    for variant in m.INDISTINGUISHABLE:          # ... and the listed ones indeed never differ
        for s in by_name.values():
            assert m.cell_candidates(s.img, s.edge, s.ini, s.minth, variant) == list(model_cands(s)), (variant, s)
