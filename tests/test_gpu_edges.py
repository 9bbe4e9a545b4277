"""The HIP kernels at non-finite and out-of-range inputs of their float-to-index steps: the cases and the rule-derived expectations of
tests/edge_inputs.py, through its checks (which tests/test_oracle_edges.py applies to the oracle on the CPU), and byte equality
with the oracle on the same inputs.  A NaN in an output equals any NaN; every other output is compared as bytes."""
import numpy as np
import pytest

import accum_routes as ar
import edge_inputs as ei
import plain_ref as pr

pytestmark = pytest.mark.gpu

# gather forms of ev2im_gauss: by size (0), the list pipeline (1), the binning-free kernel (3), bulk (2 with dedupe_min_events 1),
# slot lists (4 with dedupe_min_events 1).  The labels name what is asked for, not always what runs: count images take the list
# pipeline under every label; "slots" and "bulk" with polarity or a half window beyond 4 run the list pipeline on the tabulated
# positions; "bulk" (the sparse gather forced) still runs the slot lists when the call is dense.  Each test reads the route back.
FORMS = {"auto": (0, 1 << 20), "lists": (1, 1 << 20), "direct": (3, 1 << 20), "bulk": (2, 1), "slots": (4, 1)}


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


def _equal_oracle(what, got, want):
    gf, gu, gmm = got; of, ou, omm = want
    nbad = int((gf.view(np.uint32) != of.view(np.uint32)).sum())
    assert nbad == 0, "%s: f32 image differs from the oracle in %d px" % (what, nbad)
    assert ei.same_f32(gmm, omm) and (gu is None) == (ou is None) and (gu is None or np.array_equal(gu, ou)), "%s: extremes %s, oracle %s" % (what, gmm, omm)


# ---- family 1: accumulation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("pol", [False, True])
@pytest.mark.parametrize("sigma", ei.SIGMAS)
@pytest.mark.parametrize("W,H", ei.SIZES)
def test_ev2im_gauss_edges(oracle, fe, W, H, sigma, pol, form):
    h = pr.stamp_radius(sigma)
    ev, _, _ = ei.acc_case(W, H, h)
    blank = ei.blank_events(W, H, h)
    what = "%dx%d sigma %.1f pol %d %s" % (W, H, sigma, pol, form)
    c = fe.Context()                                                       # (its own: the bulk forms keep positions between calls)
    try:
        opts = (("gather_form", FORMS[form][0]), ("dedupe_min_events", FORMS[form][1]))
        c.debug_option("gather_form", FORMS[form][0]); c.debug_option("dedupe_min_events", FORMS[form][1])
        got = fe.EvImConverter.ev2im_gauss(ev, W, H, sigma, pol, True, ctx=c, return_all=True)
        route = ar.assert_route(c, what, "gauss", [len(ev)], pol, opts, dict_valid=False, W=W, H=H, sigma=sigma)
        if form in ("auto", "lists", "direct"):
            assert route == ((ar.LISTS if form == "lists" else ar.DIRECT) | ar.NONE), (what, ar.describe(route))
        elif pol:
            assert route & ~ar.SPARSE == ar.LISTS | ar.PER_CALL, (what, ar.describe(route))
        _equal_oracle(what, got, oracle.ev2im_gauss(ev, W, H, sigma, pol, True))
        ei.check_acc_rule(what, got, oracle, ev, W, H, sigma, pol)
        got = fe.EvImConverter.ev2im_gauss(blank, W, H, sigma, pol, True, ctx=c, return_all=True)
        _equal_oracle(what + " blank", got, oracle.ev2im_gauss(blank, W, H, sigma, pol, True))
        ei.check_blank(what + " blank", got, W, H)
    finally:
        c.close()


@pytest.mark.parametrize("W,H", ei.SIZES)
def test_position_dictionary_meets_the_value_set(oracle, fe, W, H):
    """Call 1 holds the ordinary events and freezes their positions; call 2 adds V: new positions, so the dictionary misses (the NaN
    events are dropped before the lookup) and the call is redone; call 3, the ordinary events again, is served by the dictionary."""
    sigma, h = 1.0, 3
    ev, special, _ = ei.acc_case(W, H, h)
    plain = ev[~special]
    c = fe.Context()
    try:
        c.debug_option("dedupe_min_events", 1)
        def call(e, what):
            got = fe.EvImConverter.ev2im_gauss(e, W, H, sigma, False, True, ctx=c, return_all=True)
            _equal_oracle(what, got, oracle.ev2im_gauss(e, W, H, sigma, False, True))
            ei.check_acc_rule(what, got, oracle, e, W, H, sigma, False)
        call(plain, "call 1")
        assert c.debug_counter("dict_positions") == ei.N_ORDINARY and c.debug_counter("dict_hits") == 0 and c.debug_counter("dict_misses") == 0
        call(ev, "call 2")
        assert c.debug_counter("dict_misses") == 1 and c.debug_counter("dict_hits") == 0
        npos = c.debug_counter("dict_positions")
        assert npos > ei.N_ORDINARY                                       # the table now holds V's positions too
        call(plain, "call 3")
        assert c.debug_counter("dict_hits") == 1 and c.debug_counter("dict_misses") == 1
        call(ev, "call 4")                                                 # ... and V itself, looked up: the non-reaching ids have no tile
        assert c.debug_counter("dict_hits") == 2 and c.debug_counter("dict_misses") == 1
        blank = ei.blank_events(W, H, h)
        got = fe.EvImConverter.ev2im_gauss(blank, W, H, sigma, False, True, ctx=c, return_all=True)
        ei.check_blank("blank through the dictionary", got, W, H)
        assert c.debug_counter("dict_hits") == 3
    finally:
        c.close()


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("W,H", ei.SIZES)
def test_ev2im_count_ties_and_edges(oracle, fe, W, H, form):
    c = fe.Context()
    try:
        c.debug_option("gather_form", FORMS[form][0]); c.debug_option("dedupe_min_events", FORMS[form][1])

        def run(ev, pol):
            res = fe.EvImConverter.ev2im(ev, W, H, pol, True, ctx=c, return_all=True)
            assert c.debug_counter("accum_route") == ar.LISTS | ar.NONE == ar.planned_route("count", [len(ev)], pol, (("gather_form", FORMS[form][0]), ("dedupe_min_events", FORMS[form][1])), W=W, H=H)
            return res
        what = "%dx%d %s" % (W, H, form)
        ei.check_count_rule(what, run, oracle, W, H)
        ev = ei.count_events(W, H)
        for pol in (False, True):
            _equal_oracle("%s pol %d" % (what, pol), run(ev, pol), oracle.ev2im(ev, W, H, pol, True))
    finally:
        c.close()


@pytest.mark.parametrize("raw", [False, True])
def test_batch_of_blank_empty_and_ordinary_slices(oracle, fe, raw):
    """FrontEndBatch.run_dev, B = 3: a slice none of whose events reaches the frame, an empty slice, an ordinary slice.  The blank
    images are all zero and hold no keypoint; the ordinary slice is the oracle's, and matches nothing (its predecessor is blank).
    raw: the positions come out of undistortion maps in which chosen sensor pixels hold the values (checkInImage off)."""
    from eorb_slam_amd import synth
    W, H, B, sigma, h = 240, 180, 3, 1.0, 3
    blank = ei.blank_events(W, H, h)
    if raw:
        mx, my = [m.copy() for m in synth.undistort_lut(W, H)]
        chosen = [(11 * j + 3) % (W * H) for j in range(len(blank))]
        for cpx, e in zip(chosen, blank):
            mx[cpx // W, cpx % W] = e["x"]; my[cpx // W, cpx % W] = e["y"]
        r0 = np.zeros(len(blank), synth.RAW_DTYPE); r0["x"] = np.array(chosen) % W; r0["y"] = np.array(chosen) // W; r0["p"] = blank["p"]; r0["t"] = blank["ts"]
        r2 = synth.shapes_events(3000, W, H, seed=71, motion=0.3, undistort=True, return_raw=True)[1]
        parts = [r0, r0[:0], r2]
        slices = [oracle.undistort_events(p, mx, my, W, H, False, 1.0) for p in parts]
        assert ei.same_events(slices[0], blank)
        blob = np.concatenate(parts)
    else:
        slices = [blank, blank[:0], synth.shapes_events(3000, W, H, seed=71, motion=0.3, undistort=True)]
        blob = np.concatenate([fe.pack_events(p) for p in slices])
    offsets = np.cumsum([0] + [len(p) for p in slices]).astype(np.int64)
    fb = fe.FrontEndBatch(W, H, sigma, False, 1000, 1.2, 4, 10, 0, 19, max_batch=B, max_events=4096)
    c, cap = fb.ctx, fb.cap
    try:
        if raw:
            fe.EvImConverter.set_undistort_maps(mx, my, False, ctx=c)
        d_ev = c.dev_alloc(blob.nbytes); c.upload(d_ev, blob)
        d_img = c.dev_alloc(B * W * H); d_kp = c.dev_alloc(B * cap * 28); d_desc = c.dev_alloc(B * cap * 32)
        d_n = c.dev_alloc(B * 4); d_m = c.dev_alloc(B * cap * 4); d_nm = c.dev_alloc(B * 4)
        fb.run_dev(d_ev, offsets, d_img, d_kp, d_desc, d_n, d_m, d_nm, raw=raw)
        c.sync()
        imgs = np.zeros((B, H, W), np.uint8); c.download(imgs, d_img)
        kps = np.zeros((B, cap), synth.KP_DTYPE); c.download(kps, d_kp)
        desc = np.zeros((B, cap, 32), np.uint8); c.download(desc, d_desc)
        nk = np.zeros(B, np.int32); c.download(nk, d_n)
        nm = np.zeros(B, np.int32); c.download(nm, d_nm)
        d_f32, mm = fb.last_f32(B)
        f32 = np.zeros((B, H, W), np.float32); c.download(f32, d_f32)
    finally:
        c.close()
    for b in range(B):
        of, ou, omm = oracle.ev2im_gauss(slices[b], W, H, sigma, False, True)
        _equal_oracle("slice %d" % b, (f32[b], imgs[b], mm[b]), (of, ou, omm))
    for b in (0, 1):
        ei.check_blank("slice %d" % b, (f32[b], imgs[b], mm[b]), W, H)
    assert nk[0] == 0 and nk[1] == 0 and nm.tolist() == [0, 0, 0], (nk.tolist(), nm.tolist())
    _, okp, odesc, _ = oracle.OrbExtractor(1000, 1.2, 4, 10, 0, edgeTh=19).extract(imgs[2])
    assert nk[2] == len(okp) > 50 and np.array_equal(okp.view(np.uint8), kps[2, :nk[2]].view(np.uint8)) and np.array_equal(odesc, desc[2, :nk[2]])


# ---- family 2: raw sensor events through undistortion maps ---------------------------------------------------------------------
@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("sigma", ei.SIGMAS)
def test_raw_path_edges(oracle, fe, sigma, check):
    W, H = ei.RAW_W, ei.RAW_H
    h = pr.stamp_radius(sigma)
    mx, my, raw, _ = ei.raw_case(W, H, h)
    want = ei.raw_expected_events(mx, my, raw, W, H, check)
    oev = oracle.undistort_events(raw, mx, my, W, H, check, 1.0)
    c = fe.Context()
    try:
        fe.EvImConverter.set_undistort_maps(mx, my, check, ctx=c)
        got = fe.EvImConverter.undistort_events(raw, W, H, 1.0, ctx=c)
        assert ei.same_events(got, oev) and ei.same_events(got, want), "undistort_events keeps %d events, the oracle %d, by hand %d" % (len(got), len(oev), len(want))
        for form in sorted(FORMS):
            c.debug_option("gather_form", FORMS[form][0]); c.debug_option("dedupe_min_events", FORMS[form][1])
            opts = (("gather_form", FORMS[form][0]), ("dedupe_min_events", FORMS[form][1]))
            for pol in (False, True):
                what = "raw sigma %.1f check %d pol %d %s" % (sigma, check, pol, form)
                res = fe.EvImConverter.ev2im_gauss_raw(raw, W, H, sigma, pol, True, ctx=c, return_all=True)
                route = ar.assert_route(c, what, "gauss_raw", [len(raw)], pol, opts, W=W, H=H, sigma=sigma)
                assert route & ar.MAPS and (ar.forms_of(route) != ar.SLOTS or (not pol and form in ("auto", "slots"))), (what, ar.describe(route))
                _equal_oracle(what, res, oracle.ev2im_gauss(oev, W, H, sigma, pol, True))
                ei.check_acc_rule(what, res, oracle, want, W, H, sigma, pol)
            for pol in (False, True):                                        # the count form under the same settings
                res = fe.EvImConverter.ev2im_raw(raw, W, H, pol, True, ctx=c, return_all=True)
                assert c.debug_counter("accum_route") == ar.LISTS | ar.MAPS == ar.planned_route("count_raw", [len(raw)], pol, opts, W=W, H=H)
                _equal_oracle("raw count check %d pol %d %s" % (check, pol, form), res, oracle.ev2im(oev, W, H, pol, True))
                sub, _ = ei.acc_expected_events(want, W, H, 0, count=True)
                _equal_oracle("raw count check %d pol %d %s, rule" % (check, pol, form), res, oracle.ev2im(sub, W, H, pol, True))
    finally:
        c.close()


# ---- family 3: motion-compensated images ------------------------------------------------------------------------------------
def _mci_device(fe, ctx, case, pol, pinhole_export=False):
    import ctypes as C
    from eorb_slam_amd import _lib, synth
    import test_oracle_plain as op
    group, cn, ev, m = ei.MCI[case]
    cam, W, H = op.WARP_CAMS[cn]
    if not pinhole_export:
        if group == "se3":
            return fe.EvImConverter.ev2mci_gg_f_se3(ev, cam, m["angle"], m["axis"], m["t"], m["medDepth"], W, H, ei.MCI_SIGMA, pol, True, None, ctx=ctx)
        return fe.EvImConverter.ev2mci_gg_f_se2(ev, cam, m, W, H, ei.MCI_SIGMA, pol, True, ctx=ctx)
    # eorb_ev2mci_se3 / eorb_ev2mci_se2: the pinhole-only exports of include/eorb_fe.h
    ev = np.ascontiguousarray(ev, synth.EVENT_DTYPE)
    ph = _lib.Pinhole(*[float(v) for v in cam])
    f32 = np.empty((H, W), np.float32); u8 = np.zeros((H, W), np.uint8); mm = np.zeros(2, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    if group == "se3":
        ax = np.ascontiguousarray(m["axis"], np.float64); tt = np.ascontiguousarray(m["t"], np.float64)
        ctx.check(ctx.L.eorb_ev2mci_se3(ctx.h, p(ev), len(ev), C.byref(ph), float(m["angle"]), p(ax), p(tt), float(m["medDepth"]), None, W, H,
                                        ei.MCI_SIGMA, int(pol), 1, p(f32), p(u8), p(mm)))
    else:
        prm = np.ascontiguousarray(m, np.float32)
        ctx.check(ctx.L.eorb_ev2mci_se2(ctx.h, p(ev), len(ev), C.byref(ph), p(prm), len(prm), W, H, ei.MCI_SIGMA, int(pol), 1, p(f32), p(u8), p(mm)))
    return f32, u8, mm


@pytest.mark.parametrize("case", sorted(ei.MCI))
def test_motion_compensated_edges(oracle, fe, ctx, case):
    for pol in (False, True):
        want, uv = ei.mci_oracle(oracle, case, pol)
        for export in ((False, True) if case.startswith("pinhole") else (False,)):
            what = "%s pol %d%s" % (case, pol, " (pinhole export)" if export else "")
            got = _mci_device(fe, ctx, case, pol, export)
            _equal_oracle(what, got, want)
            ei.check_mci_rule(what, case, got, uv, oracle, pol)
            ei.check_mci_plain(what, case, got, uv, pol)


# ---- family 4: pyramidal Lucas-Kanade ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ei.LK_CASES)
def test_pyr_lk_edges(oracle, fe, ctx, case):
    trk = fe.ELK_Tracker(ei.LK_WIN, ei.LK_MAXLEVEL, ei.LK_COUNT, ei.LK_EPS, ctx=ctx)
    track = lambda p, f: trk.calcOpticalFlowPyrLK(ei.lk_image(), ei.lk_image(1.0), p, f, flags=0 if f is None else 4)
    got, plain = ei.lk_run(track, case)
    want, _ = ei.lk_run(ei.oracle_tracker(oracle, False), case)
    bad = [k for k in range(len(got[1])) if not (ei.same_f32(got[0][k], want[0][k]) and got[1][k] == want[1][k] and ei.same_f32(got[2][k], want[2][k]))]
    pts, flow, _ = ei.lk_cases()[case]
    assert not bad, "%s: %d points differ from the oracle, first %d (%s): next %s status %d err %r, oracle %s %d %r" % (
        case, len(bad), bad[0], (pts if flow is None else flow)[bad[0]].tolist(), got[0][bad[0]].tolist(), got[1][bad[0]], got[2][bad[0]],
        want[0][bad[0]].tolist(), want[1][bad[0]], want[2][bad[0]])
    ei.check_lk_rule(case, case, *got, plain)


def test_slice_track_chain_edges(oracle, fe):
    """eorb_ev_slice_extract -> eorb_ev_slice_track: the tracker's points are the extraction's keypoints, so the value enters through
    the initial flow (the points the caller carries from chunk to chunk).  Every value of V that lies outside every level (NaN,
    +-inf, beyond int32, the 16-bit aliases) in x, in y and in both, between untouched points: status 0, err 0, the point unchanged."""
    import ctypes as C
    from eorb_slam_amd import _lib, synth
    W, H = 240, 180
    c = fe.Context()
    try:
        ge = fe.ORBextractor(400, 1.0, 1, 0, 0, 9, imSize=(W, H), ctx=c)
        klt = _lib.KltParams(23, 1, 10, 0.03, 1e-4)
        evs = [np.ascontiguousarray(synth.shapes_events(2000, W, H, seed=30 + k, motion=0.4 + 0.3 * k, undistort=True)) for k in range(2)]
        cap = ge.cap
        kps = np.zeros(cap, synth.KP_DTYPE); n = C.c_int(0); mono = C.c_int(0)
        c.check(c.L.eorb_ev_slice_extract(c.h, fe._p(evs[0]), None, len(evs[0]), 1.0, 0, 1000, 0, fe._p(kps), None, None, cap, C.byref(n), C.byref(mono), None))
        ref = np.zeros((H, W), np.uint8); c.check(c.L.eorb_ev_slice_image(c.h, fe._p(ref)))
        n = n.value
        values = [v for _, v in ei.SPECIALS if not abs(v) < 32000.0]                 # (NaN included: abs(NaN) < x is false)
        assert len(values) == 15 and n >= 6 * len(values) + 2
        refpts = np.stack([kps["x"][:n], kps["y"][:n]], axis=1).astype(np.float32)
        flow = refpts.copy(); special = np.zeros(n, bool)
        for j, v in enumerate(values):
            for a, k in enumerate((6 * j + 1, 6 * j + 3, 6 * j + 5)):               # x, y, both
                if a != 1: flow[k, 0] = v
                if a != 0: flow[k, 1] = v
                special[k] = True
        pts = flow.copy(); st = np.zeros(n, np.uint8); er = np.zeros(n, np.float32); cur = np.zeros((H, W), np.uint8)
        c.check(c.L.eorb_ev_slice_track(c.h, fe._p(evs[1]), None, len(evs[1]), 1.0, C.byref(klt), fe._p(pts), fe._p(st), fe._p(er), n, fe._p(cur)))
        assert np.array_equal(cur, oracle.ev2im_gauss(evs[1], W, H, 1.0, False, True)[1])
        op_, os_, oe_ = oracle.calc_optical_flow_pyr_lk(ref, cur, refpts, flow, 23, 1, 10, 0.03, 4)
        assert ei.same_f32(pts, op_) and np.array_equal(st, os_) and ei.same_f32(er, oe_), "the chain differs from the oracle at points %s" % np.flatnonzero(
            (st != os_) | (er.view(np.uint32) != oe_.view(np.uint32)))[:8].tolist()
        assert not st[special].any() and not er[special].view(np.uint32).any() and ei.same_f32(pts[special], flow[special])
        pp, ps, pe = oracle.calc_optical_flow_pyr_lk(ref, cur, refpts[~special], refpts[~special], 23, 1, 10, 0.03, 4)
        assert ei.same_f32(pts[~special], pp) and np.array_equal(st[~special], ps) and ei.same_f32(er[~special], pe) and ps.sum() > 10
    finally:
        c.close()


# ---- family 5, SearchForInitialization ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wcap,ecap,lds", [(0, 0, 0), (2, 0, 0), (0, 0, 1)])
def test_search_for_initialization_edges(oracle, fe, wcap, ecap, lds):
    """vbPrevMatched from V, windowSize 100, 1e9 and 0: the default candidate lists, the full-scan path (a list capacity of 2) and
    the lists left in global memory (one LDS entry)."""
    (k1, d1), (k2, d2) = ei.init_frames(oracle)
    W, H = ei.INIT_W, ei.INIT_H
    c = fe.Context()
    try:
        if lds: c.debug_option("win_lds_entries", lds)
        if wcap: c.debug_option("win_list_cap", wcap)
        if ecap: c.debug_option("win_pool_cap", ecap)
        F1, F2 = oracle.Frame(k1, d1, W, H), oracle.Frame(k2, d2, W, H)
        G1, G2 = fe.FrameView(k1, d1, W, H), fe.FrameView(k2, d2, W, H)
        run = lambda pm, ws: fe.ORBmatcher(0.9, True, c).SearchForInitialization(G1, G2, pm, ws)
        pm, _, _ = ei.init_prev_matched(k1)
        for ws in (100, 1000000000, 0):
            on, om, opm = oracle.search_for_initialization(F1, F2, pm, ws, 0.9, True)
            gn, gm, gpm = run(pm, ws)
            assert on == gn and np.array_equal(om, gm) and ei.same_f32(opm, gpm), "windowSize %d: %d matches, the oracle %d" % (ws, gn, on)
        ei.check_init_rule("caps %d %d %d" % (wcap, ecap, lds), run, k1)
    finally:
        c.close()


def test_window_matchers_special_keypoints(oracle, fe, ctx):
    """keypoints at V in the searched frame (Frame::PosInGrid): SearchForInitialization and SearchByProjectionLast"""
    (k1, d1), (k2, d2) = ei.init_frames(oracle)
    W, H = ei.INIT_W, ei.INIT_H
    pm = np.stack([k1["x"], k1["y"]], axis=1)
    G1 = fe.FrameView(k1, d1, W, H)
    run = lambda k, d: fe.ORBmatcher(0.9, True, ctx).SearchForInitialization(G1, fe.FrameView(k, d, W, H), pm, 100)[:2]
    ei.check_init_keypoints_rule("device", run, k1, d1, k2, d2)
    kps, desc, outside = ei.init_special_keypoints(k1, d1, k2, d2)
    on, om, _ = oracle.search_for_initialization(oracle.Frame(k1, d1, W, H), oracle.Frame(kps, desc, W, H), pm, 100, 0.9, True)
    gn, gm = run(kps, desc)
    assert on == gn and np.array_equal(om, gm)
    _, _, _, _, valid, uv, mp_obs, _, ls = ei.proj_last_args(oracle)
    cur_mp = np.full(len(kps), -1, np.int32)
    on, ocm = oracle.search_by_projection_last(oracle.Frame(kps, desc, W, H), oracle.Frame(k1, d1, W, H), valid, uv, d1, mp_obs, cur_mp, 15.0, ls, 0, True)
    gn, gcm = fe.ORBmatcher(0.9, True, ctx).SearchByProjectionLast(fe.FrameView(kps, desc, W, H), G1, valid, uv, d1, mp_obs, cur_mp, 15.0, ls, 0)
    assert on == gn and np.array_equal(ocm, gcm) and on > 10 and (gcm[outside] == -1).all()


def test_projection_matchers_fed_by_the_caller(oracle, fe, ctx):
    """SearchByProjectionLast, SearchByProjectionKF, SearchByProjectionMap: centre uv from V, level_scale and th from the radius set"""
    (k1, d1), (k2, d2) = ei.init_frames(oracle)
    W, H = ei.INIT_W, ei.INIT_H
    G2, G1 = fe.FrameView(k2, d2, W, H), fe.FrameView(k1, d1, W, H)
    cur, last = oracle.Frame(k2, d2, W, H), oracle.Frame(k1, d1, W, H)
    m = fe.ORBmatcher(0.9, True, ctx); m8 = fe.ORBmatcher(0.8, True, ctx)
    dev = ei.projection_runs(None,
                             lambda valid, uv, d, obs, slots, th, ls: m.SearchByProjectionLast(G2, G1, valid, uv, d, obs, slots, th, ls, 0),
                             lambda kk, valid, uv, lvl, ls, d, slots, th: m.SearchByProjectionKF(G2, kk, None, valid, uv, lvl, ls, d, slots, th, 100),
                             lambda valid, uv, lvl, vc, d, obs, slots, th, ls: m8.SearchByProjectionMap(G2, valid, uv, lvl, vc, d, obs, slots, th, ls),
                             k1, d1, k2, len(k2))
    orc = ei.projection_runs(oracle,
                             lambda valid, uv, d, obs, slots, th, ls: oracle.search_by_projection_last(cur, last, valid, uv, d, obs, slots, th, ls, 0, True),
                             lambda kk, valid, uv, lvl, ls, d, slots, th: oracle.search_by_projection_kf(cur, kk, None, valid, uv, lvl, ls, d, slots, th, 100, True),
                             lambda valid, uv, lvl, vc, d, obs, slots, th, ls: oracle.search_by_projection_map(cur, valid, uv, lvl, vc, d, obs, slots, th, 0.8, ls),
                             k1, d1, k2, len(k2))
    uv0, ls0 = ei.projection_uv(k1), np.ones(len(k1), np.float32)
    uv, ls, _ = ei.inject_queries(uv0, ls0)
    for name, (run, factor) in dev.items():
        th = 15.0 if factor == 1.0 else 6.0
        for t in [th] + [v for _, v in ei.PROJ_TH]:
            gn, gs, _ = run(uv, ls, t); on, os_, _ = orc[name][0](uv, ls, t)
            assert gn == on and np.array_equal(gs, os_), "%s th %r: %d matches, the oracle %d" % (name, t, gn, on)
        ei.check_projection_rule(name, run, uv0, ls0, cur.gb, th, factor)


def test_fisheye_projection_matchers_fed_by_the_caller(oracle, fe, ctx):
    """the two-camera SearchByProjection(F, map points) and SearchByProjection(Cur, Last): the left projections from V, the level
    scales and th from the radius set; against the oracle, and nothing matched where th empties every area"""
    from eorb_slam_amd import synth
    W, H = 346, 260
    rng = np.random.default_rng(77)
    n, nL, M = 260, 150, 100
    kps = synth.random_keypoints(n, W, H, nlevels=8, seed=78); desc = synth.random_descriptors(n, seed=79)
    sf = synth.scale_tables(8, 1.2)[0]
    left, right, mp_desc, mp_obs = synth.map_inputs(kps, nL, sf, rng, M, src=(kps, desc))
    l2r = np.full(nL, -1, np.int32); r2l = np.full(n - nL, -1, np.int32)
    gb = fe.grid_bounds(W, H)
    puv, pls, special = ei.inject_queries(left[1], left[4])
    ruv, rls, _ = ei.inject_queries(right[1][::-1], right[4][::-1])
    leftv = (left[0], puv, left[2], left[3], pls); rightv = (right[0], ruv[::-1].copy(), right[2], rls[::-1].copy())
    rightv = (right[0], rightv[1], right[2], right[3], rightv[3])
    fm = np.full(n, -1, np.int32); fm[::29] = -2
    m = fe.ORBmatcher(0.8, True, ctx)
    ths = [v for _, v in ei.PROJ_TH[:-1]] + [ei.f32(2.0 ** 31 * W / ei.GRID_COLS)]             # (the last one: 2^31 cells of this frame's width)
    for th in [3.0] + ths:
        on, ofm = oracle.search_by_projection_map_fisheye(kps, nL, desc, gb, l2r, r2l, leftv, rightv, mp_desc, mp_obs, fm, th, 0.8)
        gn, gfm = m.SearchByProjectionMapFisheye(kps, nL, desc, l2r, r2l, gb, leftv, rightv, mp_desc, mp_obs, fm, th)
        assert on == gn and np.array_equal(ofm, gfm), "map, th %r: %d matches, the oracle %d" % (th, gn, on)
        # (the right camera's search takes no th, :152: with every left area empty only right keypoints are matched)
        assert (on > 10) if th == 3.0 else np.array_equal(gfm[:nL], fm[:nL]), (th, on)
    lk = kps[rng.integers(0, n, M)].copy()
    uv = np.stack([lk["x"] + 1.0, lk["y"] - 1.0], axis=1).astype(np.float32); uvr = uv - np.float32([6.0, 0.0])
    ls = sf[np.clip(lk["octave"], 0, 7)]
    uvv, lsv, _ = ei.inject_queries(uv, ls); uvrv, _, _ = ei.inject_queries(uvr[::-1], ls)
    uvrv = uvrv[::-1].copy()
    valid = np.ones(M, np.uint8); ld = desc[:M]
    m9 = fe.ORBmatcher(0.9, True, ctx)
    for th in [7.0] + ths:
        on, ocm = oracle.search_by_projection_last_fisheye(kps, nL, desc, gb, lk, valid, uvv, uvrv, ld, valid, fm, th, lsv, 0, True)
        gn, gcm = m9.SearchByProjectionLastFisheye(kps, nL, desc, gb, lk, valid, uvv, uvrv, ld, valid, fm, th, lsv, 0)
        assert on == gn and np.array_equal(ocm, gcm), "last, th %r: %d matches, the oracle %d" % (th, gn, on)
        assert th == 7.0 or (on == 0 and np.array_equal(gcm, fm)), (th, on)


def test_tracked_keypoints_edges(oracle, fe):
    """ComputeTrackedKPtsDesc / AssignKPtLevelByBestDesc with keypoints at V, the oob flag included"""
    img, kps = ei.tracked_scene(oracle)
    ge = fe.ORBextractor(300, 1.2, 3, 10, 0, 19, imSize=(ei.INIT_W, ei.INIT_H))
    ext = oracle.OrbExtractor(300, 1.2, 3, 10, 0, edgeTh=19, imWidth=ei.INIT_W)
    try:
        describe = lambda k: ge.ComputeTrackedKPtsDesc(img, k)
        assign = lambda ref, k: ge.AssignKPtLevelByBestDesc(ref, img, k)
        pts, _, _ = ei.tracked_keypoints(kps)
        gd, go = describe(pts); od, oo = ext.tracked_descriptors(img, pts)
        assert np.array_equal(gd, od) and np.array_equal(go, oo), "%d descriptors, %d oob flags differ from the oracle" % (int((gd != od).any(axis=1).sum()), int((go != oo).sum()))
        ref = np.full((len(pts), 32), 0x5a, np.uint8)
        assert np.array_equal(assign(ref, pts)["octave"], ext.assign_level_by_best_desc(img, ref, pts)["octave"])
        ei.check_tracked_rule("device", describe, assign, kps)
    finally:
        ge.ctx.close()


def test_search_by_projection_last_thresholds(oracle, fe, ctx):
    """th from {0, -1, NaN, inf, 1e12, 2^31 cell widths}: the radius whose upper cell index passes 2^31 is an empty area on x86"""
    k1, d1, k2, d2, valid, uv, mp_obs, cur_mp, ls = ei.proj_last_args(oracle)
    W, H = ei.INIT_W, ei.INIT_H
    cur, last = oracle.Frame(k2, d2, W, H), oracle.Frame(k1, d1, W, H)
    G2, G1 = fe.FrameView(k2, d2, W, H), fe.FrameView(k1, d1, W, H)
    run = lambda th: fe.ORBmatcher(0.9, True, ctx).SearchByProjectionLast(G2, G1, valid, uv, d1, mp_obs, cur_mp, th, ls, 0) + (cur_mp,)
    for name, th in ei.PROJ_TH + [("15", 15.0)]:
        on, ocm = oracle.search_by_projection_last(cur, last, valid, uv, d1, mp_obs, cur_mp, th, ls, 0, True)
        gn, gcm, _ = run(th)
        assert on == gn and np.array_equal(ocm, gcm), "th %s: %d matches, the oracle %d" % (name, gn, on)
    ei.check_proj_th_rule("device", run, uv, cur.gb)


# ---- family 5: the radius search of Fuse / FuseRightMatch / SearchBySim3 / SearchByProjection(KeyFrame, Scw) and its Mixed form -----------
@pytest.mark.parametrize("kind", ["queries", "keypoints"])
def test_radius_search_edges(oracle, fe, ctx, kind):
    gb = fe.grid_bounds(ei.INIT_W, ei.INIT_H)
    s = ei.radius_scene(kind)
    q = (s["valid"], s["uv"], s["radius"], s["level"], s["qd"])
    Fr = oracle.Frame(s["kps"], s["desc"], ei.INIT_W, ei.INIT_H)
    n = len(s["kps"])
    for sigma in (False, True):
        isg = ei.INV_SIGMA2 if sigma else None
        want = oracle.kf_radius_match(Fr, *q, inv_sigma2=isg)
        got = fe.KeyFrameRadiusMatch(s["kps"], s["desc"], gb, *q, inv_sigma2=isg, ctx=ctx)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (kind, sigma)
        ei.check_radius_rule("KeyFrameRadiusMatch", lambda k, d, *qq: fe.KeyFrameRadiusMatch(k, d, gb, *qq, inv_sigma2=isg, ctx=ctx), kind, gb, sigma)
        # the Mixed form without type flags, the sequential form with nothing taken (accept_thr -1: no match takes its keypoint), and
        # the right block of a two-camera KeyFrame behind 7 left rows
        ei.check_radius_rule("KeyFrameRadiusMatchMixed", lambda k, d, *qq: fe.KeyFrameRadiusMatchMixed(
            k, d, gb, *qq, kp_inv_sigma2=None if isg is None else isg[np.clip(k["octave"], 0, 7)], ctx=ctx)[:2], kind, gb, sigma)
        ei.check_radius_rule("sequential", lambda k, d, *qq: fe.KeyFrameRadiusMatch(k, d, gb, *qq, inv_sigma2=isg, taken=np.zeros(len(k), np.uint8),
                                                                                   accept_thr=-1.0, ctx=ctx)[:2], kind, gb, sigma)
    def right(k, d, *qq):
        bi, bd = fe.FuseRightMatch(np.concatenate([k[:7], k]), 7, np.concatenate([d[:7], d]), gb, *qq, ei.INV_SIGMA2, ctx=ctx)
        return np.where(bi >= 0, bi - 7, -1).astype(np.int32), bd
    ei.check_radius_rule("FuseRightMatch", right, kind, gb, True)


def test_fuse_and_sim3_thresholds(oracle, fe, ctx):
    """Fuse and SearchBySim3 are the product's thin layers over the radius search (radius = th * scaleFactor[level], TH_LOW / TH_HIGH,
    the mutual check): the oracle has no entry of their own, so they are held to the rule's model here, and the search they share is
    held to oracle.kf_radius_match as bytes in test_radius_search_edges."""
    gb = fe.grid_bounds(ei.INIT_W, ei.INIT_H)
    s = ei.radius_scene("queries")
    for name, th in ei.PROJ_TH + [("3", 3.0)]:
        got = fe.Fuse(s["kps"], s["desc"], gb, s["valid"], s["uv"], s["level"], ei.SCALE_FACTORS, ei.INV_SIGMA2, s["qd"], th=th, ctx=ctx)
        want = ei.fuse_expected(gb, th)
        assert np.array_equal(got, want), "Fuse th %s: %d map points differ from the rule" % (name, int((got != want).sum()))
    k = ei.radius_scene("keypoints")
    for name, th in ei.PROJ_TH + [("7.5", 7.5)]:
        n, m12, qq = ei.sim3_expected(gb, th)
        kf = (k["kps"], k["desc"], gb, ei.SCALE_FACTORS)
        gn, gm = fe.SearchBySim3(kf, kf, qq, qq, th=th, ctx=ctx)
        assert gn == n and np.array_equal(gm, m12), "SearchBySim3 th %s: %d matches, by the rule %d" % (name, gn, n)


# ---- family 6: projection on the device ---------------------------------------------------------------------------------------
KB8_CAM = (226.38018519795807, 226.15002947047415, 173.6470807871759, 133.73271487507847,
           -0.048031442223833355, 0.011330957517194437, -0.055378166304281135, 0.021500973881459395)


def _same_dict(what, got, want, keys=None):
    for k in (keys or sorted(want)):
        a = np.asarray(got[k]); b = np.asarray(want[k])
        ok = ei.same_f32(a, b) if a.dtype == np.float32 else np.array_equal(a, b)
        assert ok, "%s: %s differs from the restatement at %s" % (what, k, np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[:6].tolist())


def test_projection_of_degenerate_map_points(oracle, fe, ctx):
    """isInFrustum, ProjectLastFrame, ProjectKeyFramePoints, ProjectKeyFrameSide (+Mixed) at NaN / inf / 1e30 map points, z = 0, +-1e-38
    and denormal, a zero normal, zero distances, a NaN in R: the hand-derived outcomes, and the restatements field by field"""
    import proj_ref, kfside_ref, kfside_mixed_ref
    from eorb_slam_amd import synth
    proj_ref.use_oracle_camera(oracle); kfside_ref.use_oracle_camera(oracle); kfside_mixed_ref.use_oracle(oracle)
    s = ei.map_point_scene()
    args = (s["pos"], s["normal"], s["min_dist"], s["max_dist"])
    ei.check_frustum_rule("isInFrustum", lambda kw, *a: fe.isInFrustum(fe.view(**kw), *a, viewingCosLimit=0.5, ctx=ctx)[1])
    Rn = np.eye(3); Rn[2, 0] = ei.NAN
    kps = synth.random_keypoints(len(s["pos"]), 100, 80, nlevels=8, seed=5)
    for name, kw in (("pinhole", ei.hand_view_kw()), ("kb8", ei.hand_view_kw(cam=KB8_CAM, bounds=(0.0, 346.0, 0.0, 260.0))),
                     ("moved", ei.hand_view_kw(t=(0.1, -0.2, 5.0), Ow=(-0.1, 0.2, -5.0))), ("nan in R", ei.hand_view_kw(R=Rn))):
        rv, gv = proj_ref.view(**kw), fe.view(**kw)
        wn, (want,) = proj_ref.frustum(rv, *args, cos_limit=0.5)
        gn, got = fe.isInFrustum(gv, *args, viewingCosLimit=0.5, ctx=ctx)
        assert gn == wn, (name, gn, wn)
        _same_dict("isInFrustum " + name, got, want, [f[0] for f in proj_ref.FRUSTUM_FIELDS])
        _same_dict("ProjectLastFrame " + name, fe.ProjectLastFrame(gv, s["pos"], kps, ctx=ctx), proj_ref.last_frame(rv, s["pos"], kps))
        _same_dict("ProjectKeyFramePoints " + name, fe.ProjectKeyFramePoints(gv, s["pos"], s["min_dist"], s["max_dist"], ctx=ctx),
                   proj_ref.keyframe_points(rv, s["pos"], s["min_dist"], s["max_dist"]))
        for th in (3.0, ei.INF):
            _same_dict("ProjectKeyFrameSide %s th %r" % (name, th), fe.ProjectKeyFrameSide(gv, *args, th, ctx=ctx),
                       kfside_ref.keyframe_side(kfside_ref.view(**kw), *args, th), [f[0] for f in kfside_ref.OUT_FIELDS])
        is_orb = (np.arange(len(s["pos"])) % 3 != 0).astype(np.uint8)
        ak, akl = synth.scale_tables(4, 1.4)
        mkw = dict(kw, ak_nlevels=4, ak_log_scale=akl, ak_scale_factors=ak)
        _same_dict("ProjectKeyFrameSideMixed " + name, fe.ProjectKeyFrameSideMixed(fe.view(**mkw), *args, 3.0, mp_is_orb=is_orb, ctx=ctx),
                   kfside_mixed_ref.keyframe_side([kfside_mixed_ref.view(**mkw)], *args, 3.0, mp_is_orb=is_orb))


def test_fused_searches_over_degenerate_map_points(oracle, fe, ctx):
    """SearchLocalPoints, SearchByProjectionLastPose and FusePose: the projection of the degenerate map points feeds the search in one
    call; against the restatement's projection handed to the oracle's search"""
    import proj_ref, kfside_ref
    from eorb_slam_amd import synth
    proj_ref.use_oracle_camera(oracle); kfside_ref.use_oracle_camera(oracle)
    s = ei.map_point_scene()
    M = len(s["pos"]); W, H = 100, 80
    args = (s["pos"], s["normal"], s["min_dist"], s["max_dist"])
    kw = ei.hand_view_kw()
    mp_desc = synth.random_descriptors(M, seed=12); mp_obs = np.ones(M, np.uint8)
    _, (r,) = proj_ref.frustum(proj_ref.view(**kw), *args, cos_limit=0.5)
    kps, desc, _ = synth.planted_frame(r["in_view"], r["proj_xy"], r["level"], mp_desc, 150, W, H, seed=13)
    fm = np.full(len(kps), -1, np.int32); fm[::19] = -2
    OF = oracle.Frame(kps, desc, W, H); F = fe.FrameView(kps, desc, W, H); v = fe.view(**kw)
    for th in (3.0, ei.INF, ei.NAN):
        on, ofm = oracle.search_by_projection_map(OF, r["search"], r["proj_xy"], r["level"], r["view_cos"], mp_desc, mp_obs, fm, th, 0.8, r["level_scale"])
        gm, gfm, gn, g = fe.SearchLocalPoints(F, v, *args, mp_desc, mp_obs, fm, th=th, nnratio=0.8, viewingCosLimit=0.5, ctx=ctx)
        assert gm == on and np.array_equal(gfm, ofm), "SearchLocalPoints th %r: %d matches, the oracle %d" % (th, gm, on)
        _same_dict("SearchLocalPoints", g, r, [f[0] for f in proj_ref.FRUSTUM_FIELDS])
        assert (on >= 10) if th == 3.0 else (on == 0), (th, on)
    last_kps = synth.random_keypoints(M, W, H, nlevels=8, seed=23)
    rl = proj_ref.last_frame(proj_ref.view(**kw), s["pos"], last_kps)
    OL = oracle.Frame(last_kps, np.zeros((M, 32), np.uint8), W, H); Last = fe.FrameView(last_kps, np.zeros((M, 32), np.uint8), W, H)
    for th in (15.0, ei.INF):
        on, ocm = oracle.search_by_projection_last(OF, OL, rl["valid"], rl["uv"], mp_desc, mp_obs, fm, th, rl["level_scale"], mode=0, checkOri=False)
        gm, gcm, gvalid, guv = fe.SearchByProjectionLastPose(F, v, Last, s["pos"], mp_desc, mp_obs, fm, th, mode=0, checkOri=False, ctx=ctx)
        assert gm == on and np.array_equal(gcm, ocm) and np.array_equal(gvalid, rl["valid"]) and ei.same_f32(guv, rl["uv"]), (th, gm, on)
        assert (on >= 5) if th == 15.0 else (on == 0), (th, on)
    gb = fe.grid_bounds(W, H)
    for th in (3.0, ei.INF):
        p = kfside_ref.keyframe_side(kfside_ref.view(**kw), *args, th)
        wbi, wbd = oracle.kf_radius_match(OF, p["valid"], p["uv"], p["radius"], p["level"], mp_desc)
        bi, bd, g = fe.FusePose(kps, desc, gb, v, *args, mp_desc, inv_sigma2=None, th=th, want_projection=True, ctx=ctx)
        _same_dict("FusePose th %r" % th, g, p, [f[0] for f in kfside_ref.OUT_FIELDS])
        assert bi.tobytes() == wbi.tobytes() and bd.tobytes() == wbd.tobytes(), th
        assert ((wbi >= 0).sum() >= 10) if th == 3.0 else (wbi == -1).all(), th


def sim3_pose_scene():
    """Two keyframes of the hand view whose keypoint slot i holds the degenerate or ordinary map point i of map_point_scene; the
    keypoint lies at the point's projection (elsewhere when it has none) and carries the point's descriptor; the Sim3 is the identity."""
    import proj_ref
    from eorb_slam_amd import synth
    s = ei.map_point_scene()
    M = len(s["pos"]); W, H = 100, 80
    kw = ei.hand_view_kw()
    _, (r,) = proj_ref.frustum(proj_ref.view(**kw), s["pos"], s["normal"], s["min_dist"], s["max_dist"], cos_limit=0.5)
    kps = synth.random_keypoints(M, W, H, nlevels=8, seed=31).copy()
    inv = r["in_view"] == 1
    kps["x"][inv] = r["proj_xy"][inv, 0]; kps["y"][inv] = r["proj_xy"][inv, 1]; kps["octave"][inv] = r["level"][inv]
    desc = synth.random_descriptors(M, seed=32)
    kf = dict(kps=kps, desc=desc, view=kw, pos=s["pos"], min_dist=s["min_dist"], max_dist=s["max_dist"], mp_desc=desc, skip=None)
    I = np.eye(3, dtype=np.float32); z = np.zeros(3, np.float32)
    return kf, I, z, W, H


def test_search_by_sim3_pose_over_degenerate_map_points(oracle, fe, ctx):
    """SearchBySim3Pose: both projections and both radius searches in one call, over the degenerate map points and th from
    {7.5, 0, -1, NaN, inf, 1e12}; against the restatement's projection (tests/kfside_ref, mode E) handed to the oracle's radius search"""
    import kfside_ref
    kfside_ref.use_oracle_camera(oracle)
    kf, I, z, W, H = sim3_pose_scene()
    v = kfside_ref.view(**kf["view"]); cam = kf["view"]["cam"]
    F = oracle.Frame(kf["kps"], kf["desc"], W, H)
    g = dict(kf, gb=fe.grid_bounds(W, H), view=fe.view(**kf["view"]))
    for th in [7.5] + [t for _, t in ei.PROJ_TH[:-1]]:
        p = kfside_ref.sim3_half(v, I, z, cam, v, kf["pos"], kf["min_dist"], kf["max_dist"], th)
        bi, bd = oracle.kf_radius_match(F, p["valid"], p["uv"], p["radius"], p["level"], kf["mp_desc"])
        vn = np.where(bd <= 100, bi, -1).astype(np.int32)
        m12 = np.where((vn >= 0) & (vn[np.clip(vn, 0, len(vn) - 1)] == np.arange(len(vn))), vn, -1).astype(np.int32)
        nf, g12, g1, g2 = fe.SearchBySim3Pose(g, g, I, z, I, z, th=th, ctx=ctx)
        assert np.array_equal(g1, vn) and np.array_equal(g2, vn), "th %r: %d / %d of vnMatch1 / 2 differ" % (th, int((g1 != vn).sum()), int((g2 != vn).sum()))
        assert np.array_equal(g12, m12) and nf == int((m12 >= 0).sum()), th
        assert (nf >= 30) if th == 7.5 else (nf == 0), (th, nf)
        assert (m12[p["valid"] == 0] == -1).all()


# ---- family 7: degenerate images --------------------------------------------------------------------------------------------
def test_degenerate_images(oracle, fe, ctx):
    normalize = lambda im: fe.cv_normalize_minmax_u8(im, ctx=ctx)
    focus = lambda im: fe.EvImConverter.measureImageFocus(im, ctx=ctx)
    ei.check_degenerate_images(normalize, focus)
    imgs = ei.degenerate_images()
    bad = imgs["single_patch"].copy(); bad[20, 30] = np.inf; bad[31, 7] = np.nan
    for name, im in list(imgs.items()) + [("non-finite", bad)]:
        assert np.array_equal(normalize(im), oracle.cv_normalize_minmax_u8(im)), name
    for name, im in imgs.items():
        assert ei.same_f32(np.float32(focus(im)), np.float32(oracle.measure_image_focus(im))), name
