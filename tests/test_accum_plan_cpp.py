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
