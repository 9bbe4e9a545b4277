"""octree_kernel and fast_cells_kernel (eorb_slam_amd/csrc/orb_extract.hip) on the planted scenes of tests/octree_scenes.py: the
keypoint records must equal the oracle's as bytes and the list model's (tests/octree_model.py) per level in position, response,
octave and size, in every form of the kernel: direct passes, the list algorithm, the mixed placement with generic pointers, the
dynamic placement with and without redone levels, and the second placement of calls with more than 256 workgroups.  Each test
asserts from the debug counters that the form it names is the one configured; which route inside the kernel a scene takes is not
repeated here: the model's probe (asserted in tests/test_oracle_octree_model.py) says which sizes the scene reaches."""
import numpy as np
import pytest

import octree_model as m
import octree_scenes as sc
import test_oracle_octree_model as om
from test_gpu_stages import _cands_equal

pytestmark = pytest.mark.gpu

FORMS = {"direct": {}, "list": {"octree_list_algorithm": 1}, "global": {"octree_force_global": 1}}

GROUPS = {
    "level_sizes_small": lambda n: n.startswith("level_") and int(n[6:]) <= 1025,
    "level_sizes_large": lambda n: n.startswith("level_") and int(n[6:]) > 1025,
    "node_sizes": lambda n: n.startswith(("node_", "two_big", "quartet")),
    "cut_lists": lambda n: n.startswith("cut_list"),
    "doors_midlines_roots": lambda n: n.startswith(("close_pair", "exact_doors", "midlines", "column_pair", "row_pair", "one_px", "kept_tie", "roots_")),
    "cells": lambda n: n.startswith(("weak_cell", "domain_edges", "adjacent", "skipped_column")),
}


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


def test_groups_cover_every_scene():
    for s in sc.single_level_scenes():
        assert sum(1 for g in GROUPS.values() if g(s.name)) == 1, s


# Where the octree's working set lives for a single frame (eorb_orb_configure's greedy placement into 156 KB of LDS): "lds" = all of it
# (direct passes run), "dynamic" = the arrays sized by the features at fixed offsets and the candidates' arrays sized per frame, "mixed"
# = some arrays in global scratch.  240 x 180 with edge 9 and one level: the candidates' arrays take 80 940 bytes, the node arrays
# 51 bytes per node of N + 28, the two size lists 16 bytes per entry of the power of two >= 2 * (N + 16): everything fits up to N = 874,
# the fixed part and 8 KB for candidates up to N = 1 658.  The other frames' quotas are listed.
NOT_IN_LDS = {(132, 240, 9, 1, 1589): "dynamic", (132, 240, 9, 1, 3179): "mixed", (620, 132, 9, 1, 77): "dynamic", (620, 132, 9, 1, 170): "dynamic",
              (883, 132, 9, 1, 8): "dynamic", (883, 132, 9, 1, 30): "dynamic", (346, 260, 15, 8, 1000): "dynamic"}


def _expected_placement(s, N):
    if (s.W, s.H, s.edge, s.nlevels) == (240, 180, 9, 1):
        return "lds" if N <= 874 else "dynamic" if N <= 1658 else "mixed"
    if (s.W, s.H) in ((346, 260), (752, 480)) and s.nlevels == 1:
        return "mixed"                                   # (the long-list frames: quotas of 8 065 and more)
    return NOT_IN_LDS.get((s.W, s.H, s.edge, s.nlevels, N), "lds")


def _assert_form(c, form, s, N):
    direct, lds_only = c.debug_counter("oct_direct_cap") & 0xffff, c.debug_counter("oct_lds_only") & 1
    placement = "lds" if lds_only else "dynamic" if c.debug_counter("oct_dynamic") == 1 else "mixed"
    assert placement != "mixed" or c.debug_counter("oct_scratch_bytes") > 0
    if form in ("direct", "list"):
        assert placement == _expected_placement(s, N), (s, N, placement)
        # direct passes run where the whole working set is in LDS and the list algorithm is not asked for, and only there
        assert (direct > 0) == (form == "direct" and placement == "lds"), (s, N, direct)
    elif form == "global":
        assert placement == "mixed" and c.debug_counter("oct_lds_bytes") == 0 and direct == 0
    elif form == "dynamic":
        assert placement == "dynamic"


def _model_records(oe, s, N, lap):
    """single-level planted scenes: the cached list model of the scene; other frames: the model on the oracle's level images"""
    if s.nlevels == 1 and s.expect is not None:
        mb = s.window()[0]
        kept, _ = om.model_run(s, N)
        return m.frame_keypoints([[(x + mb, y + mb, r, 0, 31) for x, y, r in kept]], [np.float32(1)], lap)
    mono, recs, _, _ = om.model_frame(oe, s, N, lap)
    return mono, recs


def _check(oracle, fe, c, s, N, form, laps=((0, 1000),)):
    oe = oracle.OrbExtractor(imWidth=s.W, **s.params(N))
    ge = fe.ORBextractor(imSize=(s.W, s.H), ctx=c, **s.params(N))
    _assert_form(c, form, s, N)
    for lap in laps:
        omono, okp, odesc, ooob = oe.extract(s.img, lap)
        assert omono >= 0, (s, N, omono)
        gmono, gkp, gdesc, goob = ge(s.img, lap)                     # (a status bit of the kernel raises here)
        what = "%s N=%d %s lap=%s" % (s, N, form, lap)
        for l in range(s.nlevels):
            ocand = oe.level_candidates(l)
            if s.expect is not None:                                 # the scene's premise, on the device too
                assert sorted(om._xyr(ocand)) == sorted(s.expect), what
            _cands_equal(what, l, c.debug_stage("cand", l), ocand)
        assert gmono == omono and len(gkp) == len(okp), "%s: GPU %d keypoints, oracle %d" % (what, len(gkp), len(okp))
        assert np.array_equal(okp.view(np.uint8), gkp.view(np.uint8)) and np.array_equal(odesc, gdesc) and np.array_equal(ooob, goob), what
        mono, recs = _model_records(oe, s, N, lap)
        assert gmono == mono and om.records(gkp) == recs, what
    return len(gkp)


@pytest.mark.parametrize("group", sorted(GROUPS))
@pytest.mark.parametrize("form", sorted(FORMS))
def test_planted_scenes(oracle, fe, form, group):
    cases = [(s, N) for s, N in sc.scene_cases() if GROUPS[group](s.name)]
    assert cases
    c = fe.Context()
    try:
        for k, v in FORMS[form].items():
            c.debug_option(k, v)
        for s, N in cases:
            _check(oracle, fe, c, s, N, form, ((0, 1000), (60, 120)) if group == "cells" else ((0, 1000),))
    finally:
        c.close()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_multilevel_frames(oracle, fe, form):
    """quotas per level, octave, size, the border offset and the scaling to level 0 as the keypoint record has them: 4 and 8 levels at
    scale factor 1.2, a planted and two texture frames"""
    c = fe.Context()
    try:
        for k, v in FORMS[form].items():
            c.debug_option(k, v)
        for s in sc.multilevel_scenes():
            for N in s.Ns:
                _check(oracle, fe, c, s, N, form, ((0, 1000), (60, 120)))
    finally:
        c.close()


@pytest.mark.parametrize("form", ["direct", "list"])
def test_longest_size_lists(oracle, fe, form):
    """the 2 x 4 and 4 x 6 lattices on 752 x 480 (two roots: 8 192 nodes after the fifth pass): cut-off lists of 8 180 and 4 536 entries,
    the generic sort above 4 096 items; 346 x 260 white noise at thresholds 1 / 1 and its lattice: 2 987 and 3 843 entries, the register
    sort of 4 096 items"""
    c = fe.Context()
    try:
        for k, v in FORMS[form].items():
            c.debug_option(k, v)
        for s in sc.big_list_scenes():
            for N in s.Ns:
                assert _check(oracle, fe, c, s, N, form) > 8000
    finally:
        c.close()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_first_pass_nodes_are_all_returned(oracle, fe, form):
    """level quotas below 4 * nIni on 640 x 120 (7 roots) and 1000 x 100 (14 roots): all first-pass nodes come back, as in the
    reference, and no status bit is raised (the extractor call would raise)"""
    c = fe.Context()
    counts = {}
    try:
        for k, v in FORMS[form].items():
            c.debug_option(k, v)
        for s in sc.capacity_scenes():
            for N in s.Ns:
                counts[(s.name, N)] = _check(oracle, fe, c, s, N, form)
    finally:
        c.close()
    assert counts[("capacity_640x120", 5)] == 28 and counts[("capacity_640x120_3levels", 30)] == 28 + 28 + 32, counts
    assert counts[("capacity_1000x100", 1)] > 1 + 8, counts


def test_levels_at_the_direct_passes_capacity(oracle, fe):
    """n == oct_direct_cap (the last level computed directly) and n == oct_direct_cap + 1 (the first one run as a list), at quotas where
    the capacity is 256 and 512"""
    by_name = {s.name: s for s in sc.single_level_scenes()}
    c = fe.Context()
    try:
        for n, Ns in sc.DIRECT_CAP_N.items():
            for N in Ns:
                _check(oracle, fe, c, by_name["level_%d" % n], N, "direct")
                cap = c.debug_counter("oct_direct_cap") & 0xffff
                assert cap in (n, n - 1) and cap in (256, 512), (n, N, cap)
    finally:
        c.close()


DYNAMIC_N = 1500        # one level of 1 500 features at 240 x 180: the node and size-list arrays leave LDS room for 2 034 candidates


def test_dynamic_placement_fits_and_redone(oracle, fe):
    """the dynamic placement (key buffers and points sized by the level's candidates): three scenes whose level fits the LDS kernel
    and three whose level is redone by the mixed-placement kernel (`oct_redo_levels`)"""
    c = fe.Context()
    try:
        by_name = {s.name: s for s in sc.single_level_scenes()}
        for name, redone in (("level_1025", 0), ("exact_doors", 0), ("node_1024", 0), ("level_2049", 1), ("level_4097", 1), ("cut_list_1024", 1)):
            _check(oracle, fe, c, by_name[name], DYNAMIC_N, "dynamic")
            assert c.debug_counter("oct_redo_levels") == redone, name
    finally:
        c.close()


BATCH_N = 300


def test_second_placement_in_a_batch_of_257_frames(oracle, fe):
    """FrontEndBatch.run_images_dev with B * nlevels = 257 > 256 workgroups selects the octree's second placement (two workgroups per
    CU); the frames cycle through the 240 x 180 planted scenes; every slice is compared"""
    scenes = [s for s in sc.single_level_scenes() if (s.W, s.H, s.edge) == (sc.W0, sc.H0, sc.E0)]
    assert len(scenes) >= 35
    B = 257
    fb = fe.FrontEndBatch(sc.W0, sc.H0, 1.0, False, BATCH_N, 1.0, 1, sc.INI, sc.MINTH, sc.E0, max_batch=B, max_events=1, match=False)
    c, cap = fb.ctx, fb.cap
    try:
        # more workgroups than CUs: the call takes the second placement (half the LDS per workgroup).  At this quota it is not the
        # single-frame one: that holds everything in LDS and runs direct passes, the second does neither
        assert B * 1 > 256 and c.debug_counter("oct_lds_only") == 1 and c.debug_counter("oct_direct_cap") == 2048
        blob = np.concatenate([scenes[b % len(scenes)].img.ravel() for b in range(B)])
        d_img = c.dev_alloc(blob.nbytes); c.upload(d_img, blob)
        d_kp = c.dev_alloc(B * cap * 28); d_desc = c.dev_alloc(B * cap * 32); d_n = c.dev_alloc(B * 4)
        d_m = c.dev_alloc(B * cap * 4); d_nm = c.dev_alloc(B * 4)
        fb.run_images_dev(d_img, B, d_kp, d_desc, d_n, d_m, d_nm)
        c.sync()
        nk = np.zeros(B, np.int32); c.download(nk, d_n)
        kps = np.zeros((B, cap), oracle.KP_DTYPE); c.download(kps, d_kp)
        desc = np.zeros((B, cap, 32), np.uint8); c.download(desc, d_desc)
        want = {}
        for b in range(B):
            s = scenes[b % len(scenes)]
            if s.name not in want:
                oe = oracle.OrbExtractor(imWidth=s.W, **s.params(BATCH_N))
                omono, okp, odesc, _ = oe.extract(s.img)
                want[s.name] = (okp, odesc, oe.level_candidates(0), _model_records(oe, s, BATCH_N, (0, 1000))[1])
            okp, odesc, ocand, recs = want[s.name]
            what = "slice %d (%s)" % (b, s)
            _cands_equal(what, 0, c.debug_stage("cand", 0, b), ocand)
            assert nk[b] == len(okp), "%s: GPU %d keypoints, oracle %d" % (what, nk[b], len(okp))
            assert np.array_equal(okp.view(np.uint8), kps[b, :nk[b]].view(np.uint8)) and np.array_equal(odesc, desc[b, :nk[b]]), what
            assert om.records(kps[b, :nk[b]]) == recs, what
    finally:
        c.close()
