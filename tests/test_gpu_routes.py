"""Every row of tests/accum_routes.py through the existing entry points: the route the dispatcher recorded (eorb_debug_counter
"accum_route") equals the table's, and the images equal the oracle's bit for bit -- float image, running extremes, u8 image."""
import os
import sys

import numpy as np
import pytest

from eorb_slam_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accum_routes as ar                           # noqa: E402
from test_gpu_parity import _check_raw_batch, _maps, _raw_batch, _same_bits      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


def _events(oracle, call, seed, mx, my, prev):
    W, H = ar.W, ar.H
    if call["events"] == "same":
        return prev[:call["sizes"][0]]
    if call["entry"] == "gauss":
        n = call["sizes"][0]
        if call["events"] == "mapped":
            ev = oracle.undistort_events(synth.random_raw_events(2 * n + 64, W, H, seed=seed), mx, my, W, H, True, 1.0)[:n]
            assert len(ev) == n
            return np.ascontiguousarray(ev)
        return synth.random_events(n, W, H, seed=seed, frac=True)
    return [synth.random_raw_events(n, W, H, seed=seed + b) for b, n in enumerate(call["sizes"])]


def _equal_oracle(want, got, what):
    (of, ou, omm), (gf, gu, gmm) = want, got
    assert _same_bits(of, gf), (what, int((of.view(np.uint32) != gf.view(np.uint32)).sum()))
    assert _same_bits(np.asarray(omm, np.float32), gmm), (what, omm, gmm)
    assert (ou is None) == (gu is None) and (ou is None or np.array_equal(ou, gu)), what


@pytest.mark.parametrize("row", ar.ROWS, ids=[r[0]["name"] for r in ar.ROWS])
def test_route_and_images_of_every_table_row(oracle, fe, row):
    W, H, sigma = ar.W, ar.H, ar.SIGMA
    mx, my = _maps(W, H)
    c, prev = None, None
    try:
        for k, call in enumerate(row):
            ev = prev = _events(oracle, call, 900 + 17 * k + len(call["name"]), mx, my, prev)
            what = call["name"]
            if call["entry"].startswith("batch"):
                got = _raw_batch(fe, ev, W, H, mx, my, call["opts"], fmt=4 if call["entry"] == "batch_raw4" else True)
                route = got[3]["accum_route"]
                assert route == call["want"], (what, ar.describe(route), ar.describe(call["want"]))
                _check_raw_batch(oracle, ev, W, H, mx, my, got, what)
                continue
            if c is None:
                c = fe.Context()
                fe.EvImConverter.set_undistort_maps(mx, my, True, ctx=c)
            for name, v in call["opts"]:
                c.debug_option(name, v)
            pol = call["pol"]
            if call["entry"] == "gauss":
                want = oracle.ev2im_gauss(ev, W, H, sigma, pol, True, fast=True)
                got = fe.EvImConverter.ev2im_gauss(ev, W, H, sigma, pol, True, ctx=c, return_all=True)
            else:
                und = oracle.undistort_events(ev[0], mx, my, W, H, True, 1.0)
                if call["entry"] == "count_raw":
                    want = oracle.ev2im(und, W, H, pol, True)
                    got = fe.EvImConverter.ev2im_raw(ev[0], W, H, pol, True, ctx=c, return_all=True)
                else:
                    want = oracle.ev2im_gauss(und, W, H, sigma, pol, True, fast=True)
                    got = fe.EvImConverter.ev2im_gauss_raw(ev[0], W, H, sigma, pol, True, ctx=c, return_all=True)
            route = c.debug_counter("accum_route")
            assert route == call["want"], (what, ar.describe(route), ar.describe(call["want"]))
            if call["want_count"] is not None:      # (the dictionary's positions: at most one per event, 2-byte ids)
                planned = ar.plan([dict(ar.query_of(call), stride=16, dict=2, sensor_w=call["sizes"][0], sensor_h=1)])[0]
                got_bin = c.debug_counter("slot_binning")
                assert got_bin & 3 == call["want_count"] == planned["count"], (what, ar.describe_binning(got_bin), planned)
            _equal_oracle(want, got, what)
    finally:
        if c is not None:
            c.close()
