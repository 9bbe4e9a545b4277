"""The slot form's binning bookkeeping: the count pass leaves a chunk's tile offsets (loff, 16 bits, loff[NT] = the chunk's entries),
the scan the lists' bases minus those offsets (gbase), the scatters copy both rows.  Every case below runs through every binning
variant the hooks reach, the variant asserted by eorb_debug_counter "slot_binning", and every slice's float image, running extremes
and u8 image equal oracle_py.ev2im_gauss bit for bit (raw events through set_undistort_maps, sigma 1).

    LDS count + ranked records + pre-ranked scatter     default
    LDS count + 2-byte records + rank scatter           option slot_prerank 0
    LDS count + ballot scatter                          option slot_rank 0
    global count pass (+ rank / ballot scatter)         a sensor of 1021 x 100 pixels: 128 tile columns do not fit the 7-bit tile
                                                        ranges of the LDS table (1017 is the narrowest such sensor; 100 rows keep
                                                        the image behind the batch call large enough for its extractor)
    keyed LDS count (float events in bulk)              the second call on a context whose position dictionary the first one froze

The scan splits a slice's chunks into segments (ev_plan.h plan_slot_scan_segments: 8 for the 690 tiles of 240x180, 4 for the 1 664
of 1021x100), each of SEG = ceil(chunks of the slice / segments) chunks."""
import os
import sys

import numpy as np
import pytest

from eorb_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accum_routes as ar                           # noqa: E402
from test_gpu_parity import _maps, _raw_batch, _same_bits      # noqa: E402

pytestmark = pytest.mark.gpu

G, L, K = ar.COUNT_GLOBAL, ar.COUNT_LDS, ar.COUNT_LDS_KEYED
ASIS, SHORT2, RANKED8 = ar.REC_AS_IS, ar.REC_SHORT2, ar.REC_RANKED8
BALLOT, RANK, PRE = ar.SCAT_BALLOT, ar.SCAT_RANK, ar.SCAT_PRE
SENSORS = {
    "240x180": dict(W=240, H=180, variants=((("pre", ()), (L, RANKED8, PRE)), (("rank", (("slot_prerank", 0),)), (L, SHORT2, RANK)),
                                            (("ballot", (("slot_rank", 0),)), (L, ASIS, BALLOT)))),
    "1021x100": dict(W=1021, H=100, variants=((("global+rank", ()), (G, ASIS, RANK)), (("global+ballot", (("slot_rank", 0),)), (G, ASIS, BALLOT)))),
}


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


_MAPS = {}


def _sensor_maps(W, H):
    if (W, H) not in _MAPS:
        if (W, H) == (240, 180):
            _MAPS[(W, H)] = _maps(W, H)
        else:       # a mild smooth distortion, as the VGA-class test of test_gpu_parity.py uses
            yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
            _MAPS[(W, H)] = ((xx + 3.0 * np.sin(yy / 41.0) - 1.5).astype(np.float32), (yy + 2.5 * np.cos(xx / 57.0) + 0.75).astype(np.float32))
    return _MAPS[(W, H)]


def _four_tile_pixel(mx, my, W, H):
    """A sensor pixel whose 7x7 stamp reaches four tiles however its position is rounded: floor and ceil of both coordinates are at
    most two pixels from a tile boundary, inside the image."""
    fx, fy = np.floor(mx).astype(int), np.floor(my).astype(int)
    near = lambda v: np.isin(v % 8, (6, 7, 0)) & np.isin((v + 1) % 8, (7, 0, 1))      # noqa: E731
    ok = near(fx) & near(fy) & (fx >= 8) & (fx < W - 16) & (fy >= 8) & (fy < H - 16)
    ys, xs = np.nonzero(ok)
    assert len(ys) > 0
    return int(xs[len(xs) // 2]), int(ys[len(ys) // 2])


def _edge(raw, W, H, frac, seed):
    """`frac` of the events onto the last tile column and row (240x180: 180 is no multiple of 8, the last row of tiles has 4 pixel rows)"""
    rng = np.random.default_rng(seed)
    n = len(raw)
    m = rng.uniform(size=n) < frac
    k = int(m.sum())
    col = rng.uniform(size=k) < 0.5
    x0, y0 = (W - 1) // 8 * 8, (H - 1) // 8 * 8
    raw["x"][m] = np.where(col, rng.integers(x0 - 3, W, k), rng.integers(0, W, k))
    raw["y"][m] = np.where(col, rng.integers(0, H, k), rng.integers(y0 - 3, H, k))
    return raw


def _case(name, W, H, mx, my):
    rnd = lambda n, seed: synth.random_raw_events(max(n, 1), W, H, seed=seed)[:n]      # noqa: E731
    if name == "chunk boundaries":              # a chunk boundary, a one-event chunk, a one-event slice, an empty slice between others
        sizes = [4095, 4096, 0, 4097, 1]
        return [_edge(rnd(n, 300 + b), W, H, 0.5 if b == 0 else 0.0, 310 + b) for b, n in enumerate(sizes)]
    if name == "segments and a full chunk":
        # mean slice length >= 2^18: chunks of 4 096 events where the rank scatter runs (2 048 for the ballot scatter, and on 1021x100
        # whose rank scatter does not fit two workgroups per CU at 4 096).  Slices 0 and 1: 3 full chunks and one of 7 events = 4
        # scan segments of SEG = 1 chunk.  Slice 2: 196 chunks = 8 segments of SEG = 25 chunks (the last of 21), each walked 8 (pass 2:
        # 4) chunks at a time with a remainder; its first chunk is 4 096 events on ONE sensor pixel whose stamp reaches four tiles:
        # loff[NT] = 16 384, the largest 16-bit offset, and ranks up to 4 095.
        raws = [_edge(rnd(3 * 4096 + 7, 320 + b), W, H, 0.2, 325 + b) for b in range(2)] + [rnd(800000, 322)]
        x, y = _four_tile_pixel(mx, my, W, H)
        raws[2]["x"][:4096] = x; raws[2]["y"][:4096] = y
        return raws
    if name == "short chunks of 256":           # a 2 000-event slice in a 16-slice batch: chunk_shift 8
        return [_edge(rnd(2000, 340 + b), W, H, 0.1, 345 + b) for b in range(16)]
    if name == "short chunks of 1024":          # ... among slices long enough for chunk_shift 10 (mean >= 2^14)
        return [rnd(2000 if b == 5 else 18000, 360 + b) for b in range(16)]
    raise KeyError(name)


CHUNKS = {"chunk boundaries": 256, "segments and a full chunk": 4096, "short chunks of 256": 256, "short chunks of 1024": 1024}


@pytest.mark.parametrize("sensor", list(SENSORS))
@pytest.mark.parametrize("case", list(CHUNKS))
def test_every_binning_variant_equals_the_oracle(oracle, fe, case, sensor):
    S = SENSORS[sensor]
    W, H = S["W"], S["H"]
    mx, my = _sensor_maps(W, H)
    raws = _case(case, W, H, mx, my)
    want = []
    for raw in raws:
        ev = oracle.undistort_events(raw, mx, my, W, H, True, 1.0)
        want.append(oracle.ev2im_gauss(ev, W, H, 1.0, False, True, fast=True))
    for (vname, hooks), binning in S["variants"]:
        opts = (("gather_form", 4),) + hooks
        imgs, f32, mm, cnt = _raw_batch(fe, raws, W, H, mx, my, opts)
        what = (case, sensor, vname)
        planned = ar.plan([dict(raw=1, B=len(raws), nev=sum(len(r) for r in raws), W=W, H=H, stride=16, **dict(opts))])[0]
        assert cnt["slot_calls"] == 1 and cnt["slot_flags"] == 0 and cnt["slot_rank_ok"] == 1, (what, cnt)
        assert cnt["slot_binning"] == ar.binning(*binning) == planned["slot_binning"], (what, ar.describe_binning(cnt["slot_binning"]), planned)
        assert cnt["slot_chunk"] == planned["slot_chunk"], (what, cnt, planned)
        if sensor == "240x180":
            assert cnt["slot_chunk"] == (min(CHUNKS[case], 2048) if binning[2] == BALLOT else CHUNKS[case]), (what, cnt)
        for b, (of, ou, omm) in enumerate(want):
            assert _same_bits(of, f32[b]), (what, b, len(raws[b]), int((of.view(np.uint32) != f32[b].view(np.uint32)).sum()))
            assert _same_bits(np.asarray(omm, np.float32), mm[b]), (what, b, omm, mm[b])
            assert np.array_equal(ou, imgs[b]), (what, b)


@pytest.mark.parametrize("vname,hooks,binning", [("pre", (), (K, RANKED8, PRE)), ("rank", (("slot_prerank", 0),), (K, ASIS, RANK)),
                                                 ("ballot", (("slot_rank", 0),), (K, ASIS, BALLOT))])
def test_keyed_count_pass_of_float_events_in_bulk(oracle, fe, vname, hooks, binning):
    """Float events in bulk: the first call tabulates its positions and freezes them into the dictionary, the second call's count pass
    looks every event up there (sl_count_lds_kernel<16, KEYED>) and leaves the offsets like every other count pass.  3 x 4 096 + 7
    events, chunks of 256."""
    W, H, n = ar.W, ar.H, 3 * 4096 + 7
    mx, my = _maps(W, H)
    ev = np.ascontiguousarray(oracle.undistort_events(synth.random_raw_events(2 * n + 64, W, H, seed=380), mx, my, W, H, True, 1.0)[:n])
    assert len(ev) == n
    want = oracle.ev2im_gauss(ev, W, H, 1.0, False, True, fast=True)
    c = fe.Context()
    try:
        fe.EvImConverter.set_undistort_maps(mx, my, True, ctx=c)
        for name, v in (("dedupe_min_events", 1),) + hooks:
            c.debug_option(name, v)
        for call in range(2):
            gf, gu, gmm = fe.EvImConverter.ev2im_gauss(ev, W, H, 1.0, False, True, ctx=c, return_all=True)
            route = c.debug_counter("accum_route")
            assert route == ar.SLOTS | (ar.DICT if call else ar.PER_CALL), (vname, call, ar.describe(route))
            if call:
                planned = ar.plan([dict(B=1, nev=n, dict_valid=1, dedupe_min_events=1, stride=16, dict=2, sensor_w=n, sensor_h=1, **dict(hooks))])[0]
                got = c.debug_counter("slot_binning")
                assert got == ar.binning(*binning) == planned["slot_binning"], (vname, ar.describe_binning(got), planned)
            assert _same_bits(want[0], gf), (vname, call, int((want[0].view(np.uint32) != gf.view(np.uint32)).sum()))
            assert _same_bits(np.asarray(want[2], np.float32), gmm), (vname, call, want[2], gmm)
            assert np.array_equal(want[1], gu), (vname, call)
    finally:
        c.close()
