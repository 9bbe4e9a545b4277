"""The accumulation dispatcher's rules without a device: eorb_slam_amd/csrc/ev_plan.h is host-only, so a plain g++ program
(tests/host/accum_plan_check.cpp) answers which form a call takes.  Every row of tests/accum_routes.py against the table, and the
rows that cost nothing here: shapes the slot form declines, tile grids the second scatter does not take, the chunk-size thresholds."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accum_routes as ar                           # noqa: E402

CALLS = [call for row in ar.ROWS for call in row]


@pytest.mark.parametrize("call", CALLS, ids=[c["name"] for c in CALLS])
def test_first_choice_route_of_every_table_row(call):
    got = ar.plan([ar.query_of(call)])[0]["route"]
    assert got == call["want"], (call["name"], ar.describe(got), ar.describe(call["want"]))


def test_both_sides_of_the_direct_threshold_keep_their_events_where_the_form_reads_them_once():
    """A host-buffer entry point leaves a slice in pinned host memory exactly when the direct-form rule holds by the call's shape -- not
    for a forced form; float events the bulk path tabulates first stay there too (as they always did)."""
    q = lambda **kw: ar.plan([kw])[0]["host_events"]      # noqa: E731
    assert q(nev=16384) == 1 and q(nev=16385) == 0 and q(nev=0) == 0
    assert q(nev=16384, raw=1) == 1 and q(nev=16384, raw=1, mode_count=1) == 0
    assert q(nev=2000, gather_form=3) == 0 and q(nev=2000, gather_form=4, raw=1) == 0
    assert q(nev=2000, dedupe_min_events=1) == 1 and q(nev=2000, dedupe_min_events=2001) == 1
    assert q(nev=2000, raw=3) == 0 and q(nev=2000, raw=1, B=5) == 0


def test_shapes_the_slot_form_declines():
    dense = dict(raw=1, B=2, nev=500000)
    vga = ar.plan([dict(dense, W=640, H=480), dict(dense, W=640, H=480, slot_rank=0), dict(dense, W=640, H=480, rank_ok=0)])
    assert vga[0]["route"] == ar.SLOTS | ar.MAPS and vga[0]["slot_scatter_rank"] == 1
    for r in vga[1:]:       # 4 800 tiles x 8 per-wave counter rows of the ballot scatter exceed 64 KB: the list pipeline, dense gather
        assert r["slot_ok"] == 0 and r["route"] == ar.LISTS | ar.MAPS, r
    nev = 2049 * 690 * 16                                     # dense by load at either size
    many = ar.plan([dict(raw=1, B=2048, nev=nev), dict(raw=1, B=2049, nev=nev)])
    assert many[0]["route"] == ar.SLOTS | ar.MAPS and many[1]["slot_ok"] == 0 and many[1]["route"] == ar.LISTS | ar.MAPS
    assert ar.plan([dict(raw=1, B=1, nev=1 << 20, W=1032, H=1024)])[0]["route"] == ar.LISTS | ar.MAPS      # 16 512 tiles: no count rows in LDS


def test_bulk_records_that_do_not_fit_the_second_scatter_are_not_tabulated():
    n = 1 << 20
    a, b, c = ar.plan([dict(nev=n, W=2040, H=8), dict(nev=n, W=2048, H=8), dict(nev=n, W=2040, H=8, scatter=1)])
    assert a["bulk_fits"] == 1 and a["route"] == ar.SLOTS | ar.PER_CALL
    assert b["bulk_fits"] == 0 and b["route"] == ar.LISTS | ar.NONE          # 256 tile columns: tile numbers no longer fit a byte pair
    assert c["bulk_fits"] == 0 and c["route"] == ar.LISTS | ar.NONE


@pytest.mark.parametrize("per_slice,pipeline,slot,slot_ballot", [
    ((1 << 14) - 1, 256, 256, 256), (1 << 14, 1024, 1024, 1024), ((1 << 17) - 1, 1024, 1024, 1024), (1 << 17, 2048, 2048, 2048),
    ((1 << 18) - 1, 2048, 2048, 2048), (1 << 18, 2048, 4096, 2048)])
def test_chunk_sizes_at_their_thresholds(per_slice, pipeline, slot, slot_ballot):
    B = 3
    for nev in (per_slice * B, per_slice * B + B - 1):       # (per slice = floor(nev / B))
        r, r0, r1 = ar.plan([dict(raw=1, B=B, nev=nev), dict(raw=1, B=B, nev=nev, slot_rank=0), dict(raw=1, B=B, nev=nev, scatter=1)])
        assert r["pipeline_chunk"] == pipeline and r["slot_chunk"] == slot and r["slot_scatter_rank"] == 1, (nev, r)
        assert r0["slot_chunk"] == slot_ballot and r0["slot_scatter_rank"] == 0, (nev, r0)
        assert r1["pipeline_chunk"] == (4096 if per_slice >= 1 << 17 else pipeline), (nev, r1)


# ---- the slot form's own plans: SlotBinPlan and SlotGatherPlan (csrc/ev_plan.h) -----------------------------------------------------
DENSE = dict(raw=1, B=2, nev=600000)                 # 240x180, 2 x 300 000 events: chunks of 4 096, 16 scatter wavefronts
G, L, K = ar.COUNT_GLOBAL, ar.COUNT_LDS, ar.COUNT_LDS_KEYED
ASIS, SHORT2, RANKED8 = ar.REC_AS_IS, ar.REC_SHORT2, ar.REC_RANKED8
BALLOT, RANK, PRE = ar.SCAT_BALLOT, ar.SCAT_RANK, ar.SCAT_PRE
DICT_SENSOR = dict(sensor_w=60000, sensor_h=1)       # a frozen dictionary's positions as a (K x 1) sensor


def _bin(**q):
    r = ar.plan([dict(DENSE, **q)])[0]
    assert r["slot_ok"] == 1, r
    if r["bin_ok"]:
        assert r["slot_binning"] == ar.binning(r["count"], r["record"], r["scatter"]), r
    return r


@pytest.mark.parametrize("q,count,record,scatter,chunk,waves,stride,scat_stride", [
    (dict(stride=16), L, RANKED8, PRE, 4096, 16, 16, 16),
    (dict(stride=16, slot_prerank=0), L, SHORT2, RANK, 4096, 16, 16, 2),
    (dict(stride=16, slot_rank=0), L, ASIS, BALLOT, 2048, 8, 16, 16),
    (dict(stride=16, rank_ok=0), L, ASIS, BALLOT, 2048, 8, 16, 16),
    (dict(stride=4), L, RANKED8, PRE, 4096, 16, 4, 4),
    (dict(stride=2), L, RANKED8, PRE, 4096, 16, 2, 2),
    (dict(stride=4, slot_prerank=0), L, ASIS, RANK, 4096, 16, 4, 4),
    (dict(stride=2, slot_prerank=0), L, ASIS, RANK, 4096, 16, 2, 2),
    (dict(stride=4, slot_rank=0), L, ASIS, BALLOT, 2048, 8, 4, 4),
    # per-call rows: never ranked, never transcoded
    (dict(stride=-4), L, ASIS, RANK, 4096, 16, -4, -4),
    (dict(stride=-4, slot_prerank=0), L, ASIS, RANK, 4096, 16, -4, -4),
    (dict(stride=-4, slot_rank=0), L, ASIS, BALLOT, 2048, 8, -4, -4),
    # a sensor of more than 65 535 pixels behind a 240x180 image, its table still in LDS: 16-bit records of neither kind
    (dict(stride=16, sensor_w=280, sensor_h=240), L, ASIS, RANK, 4096, 16, 16, 16),
    # VGA-class sensors: the tile-range table does not fit the LDS
    (dict(stride=16, W=640, H=480, nev=500000), G, ASIS, RANK, 2048, 8, 16, 16),
    (dict(stride=16, W=752, H=480, nev=500000), G, ASIS, RANK, 2048, 8, 16, 16),
    (dict(stride=4, W=640, H=480, nev=500000, slot_prerank=0), G, ASIS, RANK, 2048, 8, 4, 4),
    # the position dictionary: the stride handed in is the float events', the records are the dictionary's
    (dict(stride=16, dict=2, **DICT_SENSOR), K, RANKED8, PRE, 4096, 16, 2, 2),
    (dict(stride=16, dict=2, slot_prerank=0, **DICT_SENSOR), K, ASIS, RANK, 4096, 16, 2, 2),
    (dict(stride=16, dict=2, slot_rank=0, **DICT_SENSOR), K, ASIS, BALLOT, 2048, 8, 2, 2),
    (dict(stride=16, dict=1, sensor_w=65535, sensor_h=1), K, ASIS, RANK, 4096, 16, -4, -4),
    (dict(stride=16, dict=1, slot_prerank=0, sensor_w=65535, sensor_h=1), K, ASIS, RANK, 4096, 16, -4, -4),
])
def test_slot_binning_plan(q, count, record, scatter, chunk, waves, stride, scat_stride):
    r = _bin(**q)
    got = (r["bin_ok"], r["count"], r["record"], r["scatter"], r["slot_chunk"], r["slot_waves"], r["bin_stride"], r["scat_stride"])
    assert got == (1, count, record, scatter, chunk, waves, stride, scat_stride), (q, ar.describe_binning(r["slot_binning"]), r)


def test_slot_binning_lds_of_the_dense_batch():
    """690 tiles, 43 200 sensor pixels: 4 * 21 601 bytes of tile ranges + 16 rows of 690 16-bit counters; the pre-ranked scatter's
    4 096-event chunk: 690 list bases (4) + 4 096 x 2 words + 692 offsets (2) + 4 096 words; the rank scatter adds 16 counter rows."""
    pre, rank, ballot = _bin(stride=16), _bin(stride=16, slot_prerank=0), _bin(stride=16, slot_rank=0)
    assert pre["lds_count"] == rank["lds_count"] == ballot["lds_count"] == 86404 + 22080
    assert pre["lds_scatter"] == 2760 + 32768 + 1384 + 16384
    assert rank["lds_scatter"] == 2760 + 32768 + 22080 + 1384 + 16384
    assert ballot["lds_scatter"] == 8192 + 4096 + 16384 + 11040 + 1384 + 2760
    vga = _bin(stride=16, W=640, H=480, nev=500000)
    assert vga["lds_count"] == 4 * 4800                      # the global count pass: one 32-bit counter per tile


def test_vga_without_the_rank_scatter_is_declined_before_any_binning_plan():
    for q in (dict(rank_ok=0), dict(slot_rank=0)):
        r = ar.plan([dict(DENSE, W=640, H=480, nev=500000, **q)])[0]
        assert r["slot_ok"] == 0 and r["bin_ok"] == 0 and r["route"] == ar.LISTS | ar.MAPS, r


def test_a_dictionary_call_without_the_lds_count_pass_has_no_binning_plan():
    """Only the LDS count pass looks float events up: 4 800 tiles x 16 counter rows leave no room for 60 000 positions' tile ranges."""
    for d in (1, 2):
        r = _bin(W=640, H=480, nev=500000, dict=d, **DICT_SENSOR)
        assert r["bin_ok"] == 0, r
    assert _bin(W=640, H=480, nev=500000, dict=2, sensor_w=4000, sensor_h=1)["bin_ok"] == 1      # (153 600 + 8 004 bytes: fits)
    assert _bin(W=1024, H=400, nev=500000, dict=2, sensor_w=4000, sensor_h=1)["bin_ok"] == 0     # 128 tile columns: 7-bit tile ranges


def test_slot_gather_plan_of_the_headline_batch():
    """240x180, 128 slices, 128 M events, 256 CUs, tiles of up to 240 slots: 241 rows of 256 bytes; two such workgroups share a CU's
    160 KB, so 8 wavefronts each; 690 + 4 rounds x 256 x 2 tasks; 16 slices per wavefront at most; lists of 64 000 entries first;
    lists of 8 000 or more to the register-row kernel, 8 of its wavefronts per CU."""
    q = dict(raw=1, B=128, nev=128000000, ncu=256, sl_null=240)
    r = ar.plan([q])[0]
    got = tuple(r[k] for k in ("g_lds", "g_wg_per_cu", "g_nw", "g_rounds", "g_tasks", "g_max_per_tile", "g_prio_ref", "g_hot_min", "g_hot_cap", "g_hot_waves"))
    assert got == (61696, 2, 8, 4, 2738, 16, 64000, 8000, 8192, 2048), r
    by_size, off, floor, above = ar.plan([dict(q, slot_hot_min=-1), dict(q, slot_hot_min=0), dict(q, slot_hot_min=10), dict(q, slot_hot_min=5000)])
    assert (by_size["g_hot_min"], off["g_hot_min"], floor["g_hot_min"], above["g_hot_min"]) == (8000, 0, 64, 5000)
    # tiles of more than 240 slots: no register-row kernel whatever the hook says; one 62 KB + workgroup per CU, 16 wavefronts
    big = ar.plan([dict(q, sl_null=250), dict(q, sl_null=250, slot_hot_min=10)])
    assert [b["g_hot_min"] for b in big] == [0, 0] and big[0]["g_lds"] == 251 * 256 and big[0]["g_wg_per_cu"] == 2
    # two halves: each plans its own 64 slices, the threshold stays the batch's
    half = ar.plan([dict(q, B=64, nev=64000000, nparts=2)])[0]
    assert (half["g_hot_min"], half["g_prio_ref"], half["g_max_per_tile"]) == (8000, 32000, 8)
    # a single short slice: one wavefront, the floors
    one = ar.plan([dict(q, B=1, nev=20000)])[0]
    assert (one["g_nw"], one["g_max_per_tile"], one["g_prio_ref"], one["g_hot_min"]) == (1, 1, 4096, 4096)
