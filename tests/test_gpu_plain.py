"""The HIP kernels of the float stages against the plain float64 restatements of tests/plain_ref.py: the inputs, the checks and the
tolerances are those of tests/test_oracle_plain.py (where the oracle passes them on the CPU; nothing here is re-measured), the product is
called through the frontend.  A kernel that fails here reports its distance from the formula, not only from the oracle.  The
accumulation and the motion-compensated images are, besides, compared with the oracle bit for bit: out-of-image positions together
with a hot pixel, and these cameras' warps, are inputs the bit tests do not have."""
import ctypes as C

import numpy as np
import pytest

from eorb_slam_amd import synth
import accum_routes as ar
import plain_ref as pr
import test_oracle_plain as op

pytestmark = pytest.mark.gpu

F64 = np.float64


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


def _same_bits(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- accumulation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,sigma,pol", op.ACC_CASES)
def test_ev2im_gauss_every_gather_form_against_plain(oracle, fe, ctx, W, H, sigma, pol):
    """the forms of test_ev2im_gauss_bit_exact: by size (0), the list pipeline (1), the binning-free kernel (3), the two bulk forms
    (which run the list pipeline on the tabulated positions with polarity or a half window beyond 4); the route is read back"""
    ev = op.acc_events(W, H)
    ref = op.acc_plain(W, H, sigma, pol)
    of, ou, omm = oracle.ev2im_gauss(ev, W, H, sigma, pol, True)
    try:
        for form in (0, 1, 3, -1, -4):
            opts = (("gather_form", (2 if form == -1 else 4) if form < 0 else form), ("dedupe_min_events", 1 if form < 0 else 1 << 20))
            for k, v in opts:
                ctx.debug_option(k, v)
            gf, gu, gmm = fe.EvImConverter.ev2im_gauss(ev, W, H, sigma, pol, True, ctx=ctx, return_all=True)
            what = "%dx%d sigma %.1f pol %d form %d" % (W, H, sigma, pol, form)
            route = ar.assert_route(ctx, what, "gauss", [len(ev)], pol, opts, W=W, H=H, sigma=sigma)
            if form >= 0:
                assert route == ((ar.LISTS if form == 1 else ar.DIRECT) | ar.NONE), (what, ar.describe(route))
            elif pol or sigma > 4.0 / 3.0:
                assert ar.forms_of(route) == ar.LISTS and route & ar.PER_CALL, (what, ar.describe(route))
            op.check_accumulation(what, gf, gmm, gu, ref)
            assert _same_bits(of, gf), "%s: f32 image differs from the oracle in %d px" % (what, int((of.view(np.uint32) != gf.view(np.uint32)).sum()))
            assert _same_bits(omm, gmm) and np.array_equal(ou, gu), what
    finally:
        ctx.debug_option("gather_form", 0)
        ctx.debug_option("dedupe_min_events", 1 << 20)


def test_raw_ev2im_gauss_against_plain(oracle, fe, ctx):
    """The map-based entry (raw sensor events + undistortion maps): the plain positions are the maps' entries in float64, kept when
    they lie in the image (checkInImage); a hot sensor pixel of 600 events."""
    W, H, sigma, pol = 64, 48, 1.0, True
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    r2 = ((xx - 30.0) / 40.0) ** 2 + ((yy - 25.0) / 40.0) ** 2
    mx = (xx + (xx - 30.0) * (0.12 * r2 - 0.03 * r2 * r2) + 0.37).astype(np.float32)
    my = (yy + (yy - 25.0) * (0.12 * r2 - 0.03 * r2 * r2) - 0.21).astype(np.float32)
    raw = synth.random_raw_events(2600, W, H, seed=64)
    raw["x"][100:700] = 41; raw["y"][100:700] = 17
    np.random.default_rng(5).shuffle(raw)
    raw["t"] = np.arange(len(raw)) * 1e-6
    ux = mx[raw["y"], raw["x"]].astype(F64); uy = my[raw["y"], raw["x"]].astype(F64)
    keep = (ux >= 0) & (ux < W) & (uy >= 0) & (uy < H)
    assert 0.5 < keep.mean() < 1.0                                            # (the maps push the corners out of the image)
    pe = np.zeros(int(keep.sum()), synth.EVENT_DTYPE); pe["p"] = raw["p"][keep] != 0
    ref = pr.gauss_image(pe, W, H, sigma, pol, xy=np.stack([ux[keep], uy[keep]], axis=1))
    fe.EvImConverter.set_undistort_maps(mx, my, True, ctx=ctx)
    gf, gu, gmm = fe.EvImConverter.ev2im_gauss_raw(raw, W, H, sigma, pol, True, ctx=ctx, return_all=True)
    op.check_accumulation("raw", gf, gmm, gu, ref)
    oev = oracle.undistort_events(raw, mx, my, W, H, True, 1.0)
    assert len(oev) == len(pe)
    of, ou, omm = oracle.ev2im_gauss(oev, W, H, sigma, pol, True)
    assert _same_bits(of, gf) and _same_bits(omm, gmm) and np.array_equal(ou, gu)


# ---- motion-compensated images ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camname,motion", op.WARP_CASES)
def test_motion_compensated_image_against_plain(oracle, fe, ctx, camname, motion):
    pol = motion in ("se3_per_event", "se2_4")
    se3 = lambda *a: fe.EvImConverter.ev2mci_gg_f_se3(*a, ctx=ctx)
    se2 = lambda *a: fe.EvImConverter.ev2mci_gg_f_se2(*a, ctx=ctx)
    gf, _, gmm = op.mci_call(se3, se2, camname, motion, pol)
    what = "%s %s" % (camname, motion)
    op.check_mci(what, gf, camname, motion, pol)
    of, _, omm = op.mci_call(lambda *a: oracle.ev2mci_se3(*a[:-1], depth=a[-1]), oracle.ev2mci_se2, camname, motion, pol)
    assert _same_bits(of, gf) and _same_bits(omm, gmm), what


@pytest.mark.parametrize("motion", sorted(op.WARP_MOTIONS))
def test_pinhole_exports_equal_the_camera_forms(fe, ctx, motion):
    """eorb_ev2mci_se3 / eorb_ev2mci_se2 (the pinhole-only exports of include/eorb_fe.h) against the _cam forms with a pinhole camera:
    f32 image, extremes and u8 image bit for bit."""
    from eorb_slam_amd import _lib
    cam, W, H = op.WARP_CAMS["pinhole"]
    ev, depth = op.warp_events("pinhole")
    ev = np.ascontiguousarray(ev, synth.EVENT_DTYPE)
    group, m = op.WARP_MOTIONS[motion]
    ph = _lib.Pinhole(*[float(v) for v in cam])
    f32 = np.empty((H, W), np.float32); u8 = np.zeros((H, W), np.uint8); mm = np.zeros(2, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    if group == "se3":
        ax = np.ascontiguousarray(m["axis"], F64); tt = np.ascontiguousarray(m["t"], F64)
        dp = np.ascontiguousarray(depth, np.float32) if m["per_event"] else None
        ctx.check(ctx.L.eorb_ev2mci_se3(ctx.h, p(ev), len(ev), C.byref(ph), float(m["angle"]), p(ax), p(tt), float(m["medDepth"]),
                                        None if dp is None else p(dp), W, H, op.MCI_SIGMA, 1, 1, p(f32), p(u8), p(mm)))
        cf, cu, cmm = fe.EvImConverter.ev2mci_gg_f_se3(ev, cam, m["angle"], m["axis"], m["t"], m["medDepth"], W, H, op.MCI_SIGMA, True, True, dp, ctx=ctx)
    else:
        prm = np.ascontiguousarray(m, np.float32)
        ctx.check(ctx.L.eorb_ev2mci_se2(ctx.h, p(ev), len(ev), C.byref(ph), p(prm), len(prm), W, H, op.MCI_SIGMA, 1, 1, p(f32), p(u8), p(mm)))
        cf, cu, cmm = fe.EvImConverter.ev2mci_gg_f_se2(ev, cam, m, W, H, op.MCI_SIGMA, True, True, ctx=ctx)
    assert f32.max() > 0 and _same_bits(f32, cf) and _same_bits(mm, cmm) and np.array_equal(u8, cu), motion


# ---- focus and cv::normalize ------------------------------------------------------------------------------------------------
def test_focus_and_normalize_against_plain(fe, ctx):
    img = op.focus_image()
    op.check_focus("measureImageFocus", fe.EvImConverter.measureImageFocus(img, ctx=ctx), img)
    others = op.focus_images()
    fn = fe.EvImConverter.measureImageFocusN(np.stack(others), ctx=ctx)
    for k, im in enumerate(others):
        op.check_focus("measureImageFocusN[%d]" % k, fn[k], im)
        op.check_minmax_u8("cv_normalize_minmax_u8[%d]" % k, fe.cv_normalize_minmax_u8(im, ctx=ctx), im)


# ---- IC_Angle and rBRIEF ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["texture", "noise"])
@pytest.mark.parametrize("W,H,nl,sf,E", op.ORB_CONFIGS)
def test_orientation_and_descriptors_against_plain(fe, W, H, nl, sf, E, kind):
    """one extraction; the device's own pyramid and blurred levels (eorb_debug_stage) are what the plain angle and descriptor read"""
    img = op.orb_image(kind, W, H)
    ge = fe.ORBextractor(1000, sf, nl, 10, 0, E, imSize=(W, H))
    try:
        mono, kps, desc, _ = ge(img)
        assert mono >= 0 and len(kps) > 100 and ge.edge == E
        pyr = [ge.ctx.debug_stage("pyr", l) for l in range(nl)]
        blur = [ge.ctx.debug_stage("blur", l) for l in range(nl)]
    finally:
        ge.ctx.close()
    op.check_orientation_and_descriptors("%dx%d %s" % (W, H, kind), kps, desc, ge.mvScaleFactor, E, pyr, blur)


# ---- Lucas-Kanade -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", op.LK_SHIFTS)
@pytest.mark.parametrize("win,maxLevel", op.LK_PARAMS)
def test_pyr_lk_against_plain(fe, ctx, win, maxLevel, shift):
    trk = fe.ELK_Tracker(win, maxLevel, op.LK_COUNT, op.LK_EPS, ctx=ctx)
    nxt, st, _ = trk.calcOpticalFlowPyrLK(op.lk_image(), op.lk_image(shift), op.lk_points(win, maxLevel))
    op.check_lk("win %d maxLevel %d shift %s" % (win, maxLevel, shift), nxt, st, win, maxLevel, shift)
