"""The slot form's binning rows without a device (eorb_slam_amd/csrc/ev_plan.h through tests/host/slot_rows_check.cpp, plain g++):
the count pass leaves loff[chunk][0 .. NT] (16-bit tile offsets, loff[NT] = the chunk's entries), the scan gbase[chunk][0 .. NT)
(32-bit list bases minus those offsets); BinLayout allocates both by plan_slot_rows.  Checked here: the row pitches, the bytes of
the allocation, the LDS the three scatters ask for (the pre-ranked one keeps the loff row and no scan scratch) and the scan's split
into chunk segments, for 690 tiles (240x180), 1, 64, 65 and the largest tile grid the slot form accepts."""
import os
import subprocess
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accum_routes as ar                           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lp", "gp", "loff_bytes", "rows_bytes", "lds_pre", "lds_rank", "lds_ballot", "scan_waves", "scan_segments", "scan_tiles", "chunk_max")


@pytest.fixture(scope="module")
def rows():
    d = tempfile.mkdtemp(prefix="slot_rows_")
    exe = os.path.join(d, "slot_rows_check")
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "host", "slot_rows_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def ask(queries):
        out = subprocess.run([exe], input="".join("%d %d %d %d\n" % q for q in queries), capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        res = [dict(zip(NAMES, (int(x) for x in ln.split()))) for ln in out.stdout.strip().split("\n")]
        assert len(res) == len(queries), out.stdout
        return res
    return ask


def _up(x, a):
    return (x + a - 1) // a * a


def _slot_ok(NT):
    """Does the slot form take a dense batch on a grid of NT x 1 tiles (NT * 8 x 8 pixels)?"""
    return ar.plan([dict(raw=1, B=2, nev=64 * NT * 2 * 16, W=8 * NT, H=8)])[0]["slot_ok"] == 1


def largest_nt():
    """The largest tile count plan_slot_shape accepts: the rank scatter's 256-event chunk -- NT list bases (4 bytes), 8 per-wave count
    rows and the offsets (2 bytes each, NT rounded up to even), 3 KB for the chunk itself -- must fit 158 KB: 7 214 tiles."""
    lo, hi = 690, 16385                              # (accepted, declined: 4 * 16 385 bytes of count rows exceed 64 KB)
    assert _slot_ok(lo) and not _slot_ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _slot_ok(mid) else (lo, mid)
    return lo


def test_largest_tile_grid_of_the_slot_form():
    nt = largest_nt()
    assert nt == 7214 and not _slot_ok(nt + 1) and not _slot_ok(nt + 2)


@pytest.mark.parametrize("NT,lp,gp", [(690, 692, 692), (1, 2, 4), (64, 66, 64), (65, 66, 68), (7214, 7216, 7216)])
def test_row_pitches_and_allocation(rows, NT, lp, gp):
    """loff: NT + 1 16-bit words rounded up to even (a row is copied as dwords and starts on one); gbase: NT words rounded up to 4 (the
    scan stores 16 bytes at a time, every row starts on 16); the loff block padded to 16 bytes so that gbase starts on 16."""
    for nchunks in (0, 1, 3, 245 * 128):
        r = rows([(NT, nchunks, 4096, 16)])[0]
        n = max(nchunks, 1)
        assert (r["lp"], r["gp"]) == (lp, gp), r
        assert r["lp"] >= NT + 1 and r["lp"] % 2 == 0 and r["lp"] - (NT + 1) <= 1
        assert r["gp"] >= NT and r["gp"] % 4 == 0 and r["gp"] - NT <= 3
        assert r["loff_bytes"] == _up(2 * n * lp, 16) and r["rows_bytes"] == r["loff_bytes"] + 4 * n * gp, r
    assert rows([(NT, 1, 4096, 16)])[0]["chunk_max"] == 4096 and 4 * 4096 <= 0xffff     # loff[NT] of a full chunk is a 16-bit word


@pytest.mark.parametrize("NT", [690, 1, 64, 65, 7214])
@pytest.mark.parametrize("chunk,waves", [(4096, 16), (2048, 8), (1024, 8), (256, 8)])
def test_scatter_lds_footprints(rows, NT, chunk, waves):
    """Pre-ranked: gbase row (4 NT) | tiles of the sorted slots (2 x 4 per event) | loff row (NT + 1 halves in NTp + 2) | entry bytes
    (4 per event) and nothing else -- the offsets are copied, not scanned.  The rank form adds one 16-bit count row per wavefront; the
    ballot form keeps slot bytes (4), first tiles (2) and sorted indices (2 x 4) per event and 8 count rows."""
    r = rows([(NT, 1, chunk, waves)])[0]
    NTp = _up(NT, 2)
    loff_row = 2 * (NTp + 2)
    assert NTp + 2 >= r["lp"]                                          # the LDS row holds the whole global row, copied as lp / 2 dwords
    assert r["lds_pre"] == _up(4 * NT + 8 * chunk + loff_row + 4 * chunk, 16), r
    assert r["lds_rank"] == _up(4 * NT + 8 * chunk + waves * NTp * 2 + loff_row + 4 * chunk, 16), r
    assert r["lds_rank"] - r["lds_pre"] in (waves * NTp * 2 - 8, waves * NTp * 2, waves * NTp * 2 + 8), r      # (rounding to 16 aside)
    assert r["lds_ballot"] == _up(4 * chunk + 2 * chunk + 8 * chunk + 8 * NTp * 2 + loff_row + 4 * NT, 16), r
    if NT == 690 and chunk == 4096:
        assert r["lds_pre"] == 2760 + 32768 + 1384 + 16384 and r["lds_rank"] == r["lds_pre"] + 22080
    if NT == 7214 and chunk == 256:                                    # the largest grid: its rank scatter just fits 158 KB
        assert r["lds_rank"] == _up(161784, 16) == 158 * 1024 and r["lds_pre"] == _up(46360, 16)


@pytest.mark.parametrize("NT,waves,segments", [(690, 2, 8), (1, 1, 16), (64, 1, 16), (65, 1, 16), (512, 1, 16), (513, 2, 8), (7214, 15, 1), (16384, 16, 1)])
def test_scan_segments(rows, NT, waves, segments):
    """A scan thread owns 8 consecutive tiles; the wavefronts that cover the grid once are one segment of a slice's chunks, the
    workgroup's 16 wavefronts make as many segments as fit."""
    r = rows([(NT, 1, 4096, 16)])[0]
    assert r["scan_tiles"] == 8 and (r["scan_waves"], r["scan_segments"]) == (waves, segments), r
    assert r["scan_waves"] * 64 * 8 >= min(NT, 16 * 64 * 8) and r["scan_waves"] * r["scan_segments"] <= 16
