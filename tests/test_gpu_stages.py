"""Stage-by-stage parity of the ORB extractor: the pyramid levels (pyr_level0_kernel / pyr_level0_f32_kernel / pyr_resize_kernel), the
blurred levels (blur_kernel) and the FAST candidates (fast_cells_kernel) of the HIP path, read back with the eorb_debug_stage test
hook, against the oracle's stage introspection (oracle/eorb_oracle.h), byte for byte on every level.  The end-of-chain tests see
these kernels only through the corners the octree keeps and the 512 rBRIEF taps; here every byte and every candidate counts.  The
sizes are chosen off the friendly ones: width, height and pixel count that are no multiples of 4, partial blur tiles and FAST cells."""
import ctypes as C

import numpy as np
import pytest

from eorb_slam_amd import synth
import accum_routes as ar
import test_gpu_parity as parity

pytestmark = pytest.mark.gpu

E_ARG, E_NOTCONF = -4, -6

# W, H, nlevels, scaleFactor, edgeTh (nfeatures 1000, iniThFAST 10, minThFAST 0); every one is accepted by eorb_orb_configure
CONFIGS = [
    (240, 180, 4, 1.2, 19),
    (173, 131, 3, 1.2, 19),
    (241, 181, 4, 1.2, 19),
    (127, 97, 2, 1.2, 19),
    (255, 193, 4, 1.1, 19),
    (321, 243, 5, 1.3, 21),
    (347, 261, 8, 1.2, 9),
    (753, 481, 8, 1.2, 19),
    (97, 71, 1, 1.2, 19),
]


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


def _noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def _image(kind, W, H):
    return synth.texture_image(W, H, seed=W) if kind == "texture" else _noise(W, H, W)


def _params(nl, sf, E):
    return dict(nfeatures=1000, scaleFactor=sf, nlevels=nl, iniThFAST=10, minThFAST=0, edgeTh=E)


def _bytes_equal(what, level, got, want):
    assert got.shape == want.shape, "%s level %d: shape %s, oracle %s" % (what, level, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s level %d: %d of %d bytes differ, first (x, y) = (%d, %d): GPU %d, oracle %d" % (
        what, level, len(bad), want.size, bad[0][1], bad[0][0], got[tuple(bad[0])], want[tuple(bad[0])])


def _cands_equal(what, level, got, ocand):
    """got: (n, 3) f32 = x, y, response in any order; ocand: the oracle's candidate keypoints.  Equal as sets, response as f32 bits."""
    want = np.stack([ocand["x"], ocand["y"], ocand["response"]], axis=1).astype(np.float32) if len(ocand) else np.zeros((0, 3), np.float32)
    got = got[np.lexsort((got[:, 0], got[:, 1]))]
    want = want[np.lexsort((want[:, 0], want[:, 1]))]
    if got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        return
    gs = {tuple(r) for r in got.view(np.uint32).tolist()}
    ws = {tuple(r) for r in want.view(np.uint32).tolist()}
    only_g = sorted(gs - ws, key=lambda r: (r[1], r[0])); only_w = sorted(ws - gs, key=lambda r: (r[1], r[0]))
    f = lambda r: tuple(np.array(r, np.uint32).view(np.float32).tolist())
    raise AssertionError("%s level %d: candidates differ: GPU %d, oracle %d; %d only on the GPU (first (x, y, response) %s), %d only in the "
                         "oracle (first %s)" % (what, level, len(got), len(want), len(only_g), f(only_g[0]) if only_g else None,
                                                len(only_w), f(only_w[0]) if only_w else None))


def _stages_equal(what, ctx, oe, slice=0, blur=True):
    """Every level of the context's last extraction (slice `slice`) against the oracle extractor's last extraction."""
    for l in range(oe.nlevels):
        ocand = oe.level_candidates(l)
        assert len(ocand) > 0, "%s: the oracle found no candidate on level %d: the comparison would be empty" % (what, l)
        _bytes_equal(what + " pyr", l, ctx.debug_stage("pyr", l, slice), oe.level_buffer(l))
        if blur:
            ob = oe.level_blur(l)
            assert ob is not None
            _bytes_equal(what + " blur", l, ctx.debug_stage("blur", l, slice), ob)
        _cands_equal(what, l, ctx.debug_stage("cand", l, slice), ocand)


@pytest.mark.parametrize("kind", ["texture", "noise"])
@pytest.mark.parametrize("W,H,nl,sf,E", CONFIGS)
def test_extractor_stages_equal_oracle(oracle, fe, W, H, nl, sf, E, kind):
    """One oracle and one GPU extraction of the same image; pyr, blur and candidates of every level; then the end-of-chain check of
    tests/test_gpu_parity.py (keypoints, descriptors, the three-launch form) on the same image.  A configuration that
    eorb_orb_configure rejected would raise here: a failure, not a skip."""
    img = _image(kind, W, H)
    p = _params(nl, sf, E)
    oe = oracle.OrbExtractor(imWidth=W, **p)
    omono, okp, odesc, ooob = oe.extract(img)
    assert omono == 0 and len(okp) > 40
    ge = fe.ORBextractor(imSize=(W, H), **p)
    try:
        gmono, gkp, gdesc, goob = ge(img)
        _stages_equal("%dx%d %s" % (W, H, kind), ge.ctx, oe)
    finally:
        ge.ctx.close()
    parity._check_extract(oracle, fe, img, **p)


@pytest.mark.parametrize("W,H,nl,sf,E", [CONFIGS[1], CONFIGS[6]])
def test_three_launch_form_and_lapping_area_blur(oracle, fe, W, H, nl, sf, E):
    """The describe path as three kernels (debug option) and a lapping area inside the image: the stages, blur included, are the
    same images in both forms."""
    img = _image("texture", W, H)
    p = _params(nl, sf, E)
    oe = oracle.OrbExtractor(imWidth=W, **p)
    ge = fe.ORBextractor(imSize=(W, H), **p)
    try:
        lap = (W // 4, W // 2)
        for three, area in ((1, (0, 1000)), (0, lap), (1, lap)):
            ge.ctx.debug_option("orb_three_launches", three)
            o = oe.extract(img, area)
            g = ge(img, area)
            what = "%dx%d three_launches=%d lap=%s" % (W, H, three, area)
            assert o[0] == g[0] and np.array_equal(o[1].view(np.uint8), g[1].view(np.uint8)) and np.array_equal(o[2], g[2]), what
            _stages_equal(what, ge.ctx, oe)
    finally:
        ge.ctx.close()


def _download_batch(c, B, cap, d_kp, d_desc, d_n):
    nk = np.zeros(B, np.int32); c.download(nk, d_n)
    kps = np.zeros((B, cap), synth.KP_DTYPE); c.download(kps, d_kp)
    desc = np.zeros((B, cap, 32), np.uint8); c.download(desc, d_desc)
    return nk, kps, desc


def test_batched_event_slices_stage_by_stage(oracle, fe):
    """eorb_fe_run_batch_dev, 3 slices of 173 x 131: level 0 comes from the float event image and its running extremes
    (pyr_level0_f32_kernel), not from a u8 upload; stages of every slice against three oracle runs."""
    W, H, B, n = 173, 131, 3, 30000
    nl, sf, E = 3, 1.2, 19
    slices = [synth.shapes_events(n, W, H, seed=60 + b, motion=0.3) for b in range(B)]
    fb = fe.FrontEndBatch(W, H, 1.0, False, 1000, sf, nl, 10, 0, E, max_batch=B, max_events=n)
    c, cap = fb.ctx, fb.cap
    try:
        ev16 = np.concatenate([fe.pack_events(s) for s in slices])
        d_ev = c.dev_alloc(ev16.nbytes); c.upload(d_ev, ev16)
        d_img = c.dev_alloc(B * W * H); d_kp = c.dev_alloc(B * cap * 28); d_desc = c.dev_alloc(B * cap * 32)
        d_n = c.dev_alloc(B * 4); d_m = c.dev_alloc(B * cap * 4); d_nm = c.dev_alloc(B * 4)
        fb.run_dev(d_ev, np.arange(B + 1, dtype=np.int64) * n, d_img, d_kp, d_desc, d_n, d_m, d_nm)
        c.sync()
        imgs = np.zeros((B, H, W), np.uint8); c.download(imgs, d_img)
        nk, kps, desc = _download_batch(c, B, cap, d_kp, d_desc, d_n)
        oe = oracle.OrbExtractor(1000, sf, nl, 10, 0, edgeTh=E, imWidth=W)
        for b in range(B):
            _, ou, _ = oracle.ev2im_gauss(slices[b], W, H, 1.0, False, True)
            assert np.array_equal(ou, imgs[b]), "slice %d: event image" % b
            _, okp, odesc, _ = oe.extract(ou)
            assert len(okp) >= 30                                          # (short slices of three quadrilaterals: 40 - 125 keypoints)
            _stages_equal("events slice %d" % b, c, oe, slice=b)
            assert nk[b] == len(okp) and np.array_equal(okp.view(np.uint8), kps[b, :nk[b]].view(np.uint8)) and np.array_equal(odesc, desc[b, :nk[b]]), b
        with pytest.raises(fe.EorbError) as ei:
            c.debug_stage("pyr", 0, B)
        assert ei.value.code == E_ARG
    finally:
        c.close()


def test_batched_camera_frames_stage_by_stage(oracle, fe):
    """eorb_fe_run_batch_images_dev, 3 frames of 173 x 131 (two textures and white noise): stages of every slice."""
    W, H, B = 173, 131, 3
    nl, sf, E = 3, 1.2, 19
    frames = [synth.texture_image(W, H, seed=W), _noise(W, H, W), synth.texture_image(W, H, seed=W + 1)]
    fb = fe.FrontEndBatch(W, H, 1.0, False, 1000, sf, nl, 10, 0, E, max_batch=B, max_events=1)
    c, cap = fb.ctx, fb.cap
    try:
        blob = np.concatenate([f.ravel() for f in frames])
        d_img = c.dev_alloc(blob.nbytes); c.upload(d_img, blob)
        d_kp = c.dev_alloc(B * cap * 28); d_desc = c.dev_alloc(B * cap * 32); d_n = c.dev_alloc(B * 4)
        d_m = c.dev_alloc(B * cap * 4); d_nm = c.dev_alloc(B * 4)
        fb.run_images_dev(d_img, B, d_kp, d_desc, d_n, d_m, d_nm)
        c.sync()
        nk, kps, desc = _download_batch(c, B, cap, d_kp, d_desc, d_n)
        oe = oracle.OrbExtractor(1000, sf, nl, 10, 0, edgeTh=E, imWidth=W)
        for b in range(B):
            _, okp, odesc, _ = oe.extract(frames[b])
            _stages_equal("frames slice %d" % b, c, oe, slice=b)
            assert nk[b] == len(okp) and np.array_equal(okp.view(np.uint8), kps[b, :nk[b]].view(np.uint8)) and np.array_equal(odesc, desc[b, :nk[b]]), b
    finally:
        c.close()


def test_stage_hook_errors_leave_the_context_usable(oracle, fe):
    """Unknown name, level = nlevels, slice = batch size, a buffer one byte short, "blur" after a detect-only call, the hook before
    any extraction: error codes, never a fault; one good extraction afterwards is compared in full."""
    W, H, nl, sf, E = 173, 131, 3, 1.2, 19
    img = _image("texture", W, H)
    p = _params(nl, sf, E)
    ge = fe.ORBextractor(imSize=(W, H), **p)
    c = ge.ctx
    d0, d1 = C.c_int(-1), C.c_int(-1)
    buf = np.zeros(4 << 20, np.uint8)
    raw = lambda name, sl, lv, cap: c.L.eorb_debug_stage(c.h, name, sl, lv, buf.ctypes.data_as(C.c_void_p), cap, C.byref(d0), C.byref(d1))
    try:
        assert raw(b"pyr", 0, 0, buf.nbytes) == E_NOTCONF                   # nothing extracted yet
        ge(img, (0, 1000), False)                                              # detect only: no blurred levels
        assert raw(b"blur", 0, 0, buf.nbytes) == E_ARG and b"descriptors" in c.L.eorb_last_error(c.h)
        assert raw(b"pyr", 0, 0, buf.nbytes) == 0 and (d0.value, d1.value) == (H + 2 * E, W + 2 * E)
        assert raw(b"cand", 0, 0, buf.nbytes) == 0 and d0.value > 0 and d1.value == 3
        ncand = d0.value
        ge(img)
        assert raw(b"score", 0, 0, buf.nbytes) == E_ARG and b"unknown" in c.L.eorb_last_error(c.h)
        assert raw(b"pyr", 0, nl, buf.nbytes) == E_ARG and raw(b"pyr", 0, -1, buf.nbytes) == E_ARG
        assert raw(b"pyr", 1, 0, buf.nbytes) == E_ARG and raw(b"pyr", -1, 0, buf.nbytes) == E_ARG
        assert c.L.eorb_debug_stage(c.h, None, 0, 0, None, 0, None, None) == E_ARG
        for name, need in ((b"pyr", (H + 2 * E) * (W + 2 * E)), (b"blur", W * H), (b"cand", ncand * 12)):
            buf[:] = 0xa5
            assert raw(name, 0, 0, need - 1) == E_ARG, name
            assert (buf == 0xa5).all(), name                                   # a refused call writes nothing
            assert raw(name, 0, 0, need) == 0, name
            assert (buf[need:] == 0xa5).all() and not (buf[:need] == 0xa5).all(), name
        assert c.L.eorb_debug_stage(c.h, b"blur", 0, 1, None, 0, C.byref(d0), None) == 0 and d0.value == ge.ctx.debug_stage("blur", 1).shape[0]
        oe = oracle.OrbExtractor(imWidth=W, **p)
        o = oe.extract(img)
        g = ge(img)
        assert np.array_equal(o[1].view(np.uint8), g[1].view(np.uint8)) and np.array_equal(o[2], g[2])
        _stages_equal("after the errors", c, oe)
        # the tracked-keypoint helpers rebuild pyramid and blur of one image and detect nothing
        ge.ComputeTrackedKPtsDesc(img, o[1][:10])
        assert raw(b"cand", 0, 0, buf.nbytes) == E_ARG
        _bytes_equal("tracked pyr", 1, c.debug_stage("pyr", 1), oe.level_buffer(1))
        _bytes_equal("tracked blur", 1, c.debug_stage("blur", 1), oe.level_blur(1))
    finally:
        c.close()


# ---- the other image-sized entry points at sizes whose width, height and pixel count are no multiples of 4 ------------------
OFF_SIZES = [(173, 131), (250, 131), (33, 17)]


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


_same_bits = parity._same_bits


@pytest.mark.parametrize("W,H", OFF_SIZES)
def test_float_accumulation_off_sizes(oracle, fe, ctx, W, H):
    """ev2im_gauss / ev2im from float events as tests/test_gpu_parity.py checks them at 240 x 180 (every gather form, normalised and
    not): partial 8 x 8 accumulation tiles in both axes at once, an odd pixel count in the extremes and the normalisation."""
    ev = synth.random_events(5000, W, H, seed=11 + W, frac=True)
    try:
        for form in (0, 1, 3, -1, -4):
            opts = (("gather_form", (2 if form == -1 else 4) if form < 0 else form), ("dedupe_min_events", 1 if form < 0 else 1 << 20))
            for k, v in opts:
                ctx.debug_option(k, v)
            for sigma, pol in ((1.0, False), (1.5, True), (0.5, False)):
                for normalized in (True, False):
                    of, ou, omm = oracle.ev2im_gauss(ev, W, H, sigma, pol, normalized)
                    gf, gu, gmm = fe.EvImConverter.ev2im_gauss(ev, W, H, sigma, pol, normalized, ctx=ctx, return_all=True)
                    what = (form, sigma, pol, normalized)
                    route = ar.assert_route(ctx, what, "gauss", [len(ev)], pol, opts, W=W, H=H, sigma=sigma)
                    if form >= 0:
                        assert route == ((ar.LISTS if form == 1 else ar.DIRECT) | ar.NONE), (what, ar.describe(route))
                    elif pol:                       # (the bulk forms with polarity: the list pipeline on the tabulated positions)
                        assert ar.forms_of(route) == ar.LISTS and route & ar.PER_CALL, (what, ar.describe(route))
                    assert _same_bits(of, gf), "%s: f32 image differs: %d px" % (what, int((of.view(np.uint32) != gf.view(np.uint32)).sum()))
                    assert _same_bits(omm, gmm), what
                    if normalized:
                        assert np.array_equal(ou, gu), what
    finally:
        ctx.debug_option("gather_form", 0)
        ctx.debug_option("dedupe_min_events", 1 << 20)
    for pol in (False, True):
        for normalized in (True, False):
            of, ou, omm = oracle.ev2im(ev, W, H, pol, normalized)
            gf, gu, gmm = fe.EvImConverter.ev2im(ev, W, H, pol, normalized, ctx=ctx, return_all=True)
            assert _same_bits(of, gf) and _same_bits(omm, gmm), (pol, normalized)
            assert (ou is None) == (gu is None)
            if ou is not None:
                assert np.array_equal(ou, gu), (pol, normalized)


@pytest.mark.parametrize("W,H", OFF_SIZES)
def test_normalize_extremes_in_the_last_pixels(oracle, fe, ctx, W, H):
    """cv::normalize(MINMAX) of an image whose minimum and maximum sit in its last 1 - 3 pixels (what a loop over groups of four
    pixels leaves to its tail), and in its first pixel; one image and n images per call for the focus."""
    rng = np.random.default_rng(W)
    base = rng.uniform(1.0, 2.0, (H, W)).astype(np.float32)
    imgs = []
    for lo, hi in ((-1, -2), (-3, -1), (-2, -3), (0, -1), (-1, 0)):
        img = base.copy()
        img.flat[lo] = -4.25; img.flat[hi] = 9.5
        imgs.append(img)
        want = oracle.cv_normalize_minmax_u8(img)
        assert want.flat[lo] == 0 and want.flat[hi] == 255
        assert np.array_equal(want, fe.cv_normalize_minmax_u8(img, ctx=ctx)), (lo, hi)
        assert np.float32(oracle.measure_image_focus(img)).tobytes() == np.float32(fe.EvImConverter.measureImageFocus(img, ctx=ctx)).tobytes(), (lo, hi)
    fn = fe.EvImConverter.measureImageFocusN(np.stack(imgs), ctx=ctx)
    assert [np.float32(oracle.measure_image_focus(i)).tobytes() for i in imgs] == [np.float32(v).tobytes() for v in fn]


OFF_CAM = (150.0, 149.5, 86.3, 65.2)                                 # a pinhole camera for 173 x 131
OFF_KB8 = OFF_CAM + parity.MVSEC_KB8[4:]


def _corner_events(n, W, H, seed, k=80):
    """Shapes events at fractional positions, k of them moved onto pixel (0, 0) and k onto (W - 1, H - 1): the maximum of the event
    histogram is then the first pixel, and the reconstructions put weight into the first and the last pixels."""
    ev = synth.shapes_events(n, W, H, seed=seed, motion=1.5)
    rng = np.random.default_rng(seed)
    ev["x"] = np.minimum(ev["x"] + rng.uniform(0, 1, n).astype(np.float32), np.float32(W - 1))
    ev["y"] = np.minimum(ev["y"] + rng.uniform(0, 1, n).astype(np.float32), np.float32(H - 1))
    idx = rng.choice(n, 2 * k, replace=False)
    ev["x"][idx[:k]] = 0; ev["y"][idx[:k]] = 0
    ev["x"][idx[k:]] = W - 1; ev["y"][idx[k:]] = H - 1
    return ev


def test_motion_compensation_and_contest_off_size(oracle, fe, ctx):
    """ev2mci_se3 / ev2mci_se2 with the pinhole and the KannalaBrandt8 camera and the reconstruction contest on 173 x 131: 22 663
    pixels, so of the images the contest normalises back to back every second one starts off a 16-byte boundary."""
    from oracle import orc_chain
    W, H = 173, 131
    ev = _corner_events(6000, W, H, 82)
    p = synth.l1_mci_poses(ev)
    eh = oracle.ev2im_gauss(ev, W, H, 1.0, False, False)[0]
    assert np.argmax(eh) == 0                                             # the histogram's maximum is pixel (0, 0)
    recon = {"EH": (eh, fe.EvImConverter.ev2im_gauss(ev, W, H, 1.0, False, False, ctx=ctx, return_all=True)[0])}
    for name, cam in (("pinhole", OFF_CAM), ("kb8", OFF_KB8)):
        for pol in (False, True):
            for normalized in (False, True):
                for key in ("dp", "ba"):
                    m = p[key]
                    of, ou, omm = oracle.ev2mci_se3(ev, cam, m["angle"], m["axis"], m["t"], m["medDepth"], W, H, 1.0, pol, normalized)
                    gf, gu, gmm = fe.EvImConverter.ev2mci_gg_f_se3(ev, cam, m["angle"], m["axis"], m["t"], m["medDepth"], W, H, 1.0, pol, normalized, ctx=ctx)
                    what = (name, key, pol, normalized)
                    assert _same_bits(of, gf) and _same_bits(omm, gmm), what
                    if normalized:
                        assert np.array_equal(ou, gu), what
                    elif not pol:
                        recon[name + key] = (of, gf)
                for params in (p["se2"], [-0.015, 0.002, 0.001, 0.97]):
                    of, ou, omm = oracle.ev2mci_se2(ev, cam, params, W, H, 1.0, pol, normalized)
                    gf, gu, gmm = fe.EvImConverter.ev2mci_gg_f_se2(ev, cam, params, W, H, 1.0, pol, normalized, ctx=ctx)
                    what = (name, len(params), pol, normalized)
                    assert _same_bits(of, gf) and _same_bits(omm, gmm), what
                    if normalized:
                        assert np.array_equal(ou, gu), what
                    elif not pol:
                        recon[name + "se2_%d" % len(params)] = (of, gf)
    keys = sorted(recon)
    for k in keys:
        of, gf = recon[k]
        assert np.float32(oracle.measure_image_focus(of)).tobytes() == np.float32(fe.EvImConverter.measureImageFocus(gf, ctx=ctx)).tobytes(), k
        assert np.array_equal(oracle.cv_normalize_minmax_u8(of), fe.cv_normalize_minmax_u8(gf, ctx=ctx)), k
    fn = fe.EvImConverter.measureImageFocusN(np.stack([recon[k][1] for k in keys]), ctx=ctx)
    assert [np.float32(oracle.measure_image_focus(recon[k][0])).tobytes() for k in keys] == [np.float32(v).tobytes() for v in fn]
    # the contest (eorb_ev_mc_contest): winner, the five focus values as bits, the winner's u8 image, the L2 detection on it
    g = fe.EvImBuilder(W, H, cam=OFF_CAM)
    try:
        l2 = oracle.OrbExtractor(800, 1.0, 1, 0, 0, edgeTh=9, imWidth=W)
        strong = dict(p, se2=np.array([0.0, 0.0, 0.0], np.float32))       # the SE2 reconstruction equals the histogram: the first of equals wins
        shift = dict(p, dp=dict(angle=0.0, axis=(0.0, 0.0, 1.0), t=(-0.01, 0.0, 0.0), medDepth=1.0))      # ... and this one beats it
        winners = set()
        for poses in (p, None, dict(dp=p["dp"]), dict(ba=p["ba"], se2=p["se2"]), strong, shift):
            for evs in (ev, ev[:5999], ev[:1001]):
                gm = g.generateMCImage(evs, poses)
                om = orc_chain.generate_mc_image(evs, W, H, 1.0, OFF_CAM, poses, l2)
                what = (len(evs), None if poses is None else sorted(poses))
                assert gm["winner"] == om["winner"], (what, gm["focus"], om["focus"])
                assert np.array_equal(gm["focus"].view(np.uint32), om["focus"].view(np.uint32)), (what, gm["focus"], om["focus"])
                assert np.array_equal(gm["image"], om["image"]), what
                assert len(gm["l2_kps"]) == len(om["l2_kps"]) and np.array_equal(gm["l2_kps"].view(np.uint8), om["l2_kps"].view(np.uint8)), what
                assert len(om["l2_kps"]) > 20
                winners.add(om["winner"])
        assert {0, 2} <= winners, winners                               # a motion-compensated image and the histogram both won
    finally:
        g.close()


@pytest.mark.parametrize("win", [23, 9])
@pytest.mark.parametrize("W,H", [(173, 131), (241, 181)])
def test_klt_pyr_lk_odd_sizes(oracle, fe, ctx, W, H, win):
    """calcOpticalFlowPyrLK with maxLevel 3 on images whose pyrDown sizes are odd at every level (173 x 131 -> 87 x 66 -> 44 x 33 ->
    22 x 17, the last smaller than the 23-px window), points at all four borders and outside, as test_klt_pyr_lk."""
    maxLevel = 3
    img1 = synth.texture_image(W, H, seed=W)
    rng = np.random.default_rng(4)
    img2 = np.clip(np.roll(img1, (2, -3), axis=(0, 1)).astype(np.int32) + rng.integers(-3, 4, (H, W)), 0, 255).astype(np.uint8)
    img2[H // 2:H // 2 + 30, W // 2:W // 2 + 40] = 90
    e = oracle.OrbExtractor(600, 1.2, 3, 10, 0, edgeTh=19, imWidth=W)
    _, k, _, _ = e.extract(img1)
    interior = np.stack([k["x"], k["y"]], axis=1).astype(np.float32)
    extra = np.array([[0.0, 0.0], [W - 0.1, H - 0.1], [1.5, H / 2 + 0.25], [W - 2.0, 3.0], [-20.0, 50.0], [W + 60.0, 90.0], [W / 2, -30.0],
                      [W / 2 + 0.5, H - 1.0], [5.0, 5.0], [0.0, H - 1.0], [W - 1.0, 0.0]], np.float32)
    pts = np.concatenate([interior + rng.uniform(-0.5, 0.5, interior.shape).astype(np.float32), extra])
    trk = fe.ELK_Tracker(win, maxLevel, 10, 0.03, ctx=ctx)
    for flags, guess in ((0, None), (4, pts + np.float32([-2.5, 1.5])), (8, None), (4, pts + np.float32([40.0, -40.0]))):
        on, os_, oe = oracle.calc_optical_flow_pyr_lk(img1, img2, pts, guess, win, maxLevel, 10, 0.03, flags)
        gn, gs, ge = trk.calcOpticalFlowPyrLK(img1, img2, pts, guess, flags)
        assert np.array_equal(os_, gs), (flags, int((os_ != gs).sum()))
        assert np.array_equal(on.view(np.uint32), gn.view(np.uint32)) and np.array_equal(oe.view(np.uint32), ge.view(np.uint32)), flags
    on, os_, oe = oracle.calc_optical_flow_pyr_lk(img1, img2, pts, None, win, maxLevel, 10, 0.03, 0)
    good = os_[:len(interior)] == 1
    assert good.sum() > len(interior) // 2 and len(interior) > 200, (int(good.sum()), len(interior))
    assert (os_[len(interior):] == 0).sum() >= 3                           # the points outside the image are lost


def test_frame_stereo_off_size(oracle, fe):
    """eorb_frame_stereo on 347 x 261 (accepted: level 7 is 97 x 73, two 30-px cells by one with edge 19): as test_frame_stereo_matches."""
    W, H, mb, mbf = 347, 261, 0.11, 40.0
    left, right = synth.stereo_pair(35, W, H)
    oL = oracle.OrbExtractor(1000, 1.2, 8, 20, 7, edgeTh=19, imWidth=W)
    oR = oracle.OrbExtractor(1000, 1.2, 8, 20, 7, edgeTh=19, imWidth=W)
    _, kL, dL, _ = oL.extract(left, (0, 0)); _, kR, dR, _ = oR.extract(right, (0, 0))
    our, odp, on = oL.compute_stereo_matches(oR, kL, dL, kR, dR, mb, mbf)
    ge = fe.ORBextractor(1000, 1.2, 8, 20, 7, 19, (W, H))
    try:
        for _ in range(2):
            g = ge.stereo(left, right, mb, mbf)
            assert len(g["kpsL"]) == len(kL) and len(g["kpsR"]) == len(kR)
            assert np.array_equal(g["kpsL"].view(np.uint8), kL.view(np.uint8)) and np.array_equal(g["kpsR"].view(np.uint8), kR.view(np.uint8))
            assert np.array_equal(g["descL"], dL) and np.array_equal(g["descR"], dR)
            assert g["nmatches"] == on
            assert np.array_equal(g["uRight"].view(np.uint32), our.view(np.uint32)) and np.array_equal(g["depth"].view(np.uint32), odp.view(np.uint32))
            _stages_equal("stereo left", ge.ctx, oL, slice=0)
            _stages_equal("stereo right", ge.ctx, oR, slice=1)
        assert (our > 0).sum() > 150
    finally:
        ge.ctx.close()


@pytest.mark.parametrize("laps", [((0, 508), (0, 508)), ((0, 300), (200, 508))])
def test_frame_fisheye_off_size(oracle, fe, laps):
    """eorb_frame_fisheye on 509 x 511 (accepted: the aspect of the bordered area rounds to one octree root): as test_frame_fisheye."""
    W, H, nfeat = 509, 511, 1000
    imL, imR = synth.image_pair(W, H, 7)
    e = oracle.OrbExtractor(nfeat, 1.2, 8, 20, 7, edgeTh=19, imWidth=W)
    mL, kL, dL, _ = e.extract(imL, laps[0])
    mR, kR, dR, _ = e.extract(imR, laps[1])
    n, cand, d2 = oracle.fisheye_matches(dL, mL, dR, mR)
    ge = fe.ORBextractor(nfeat, 1.2, 8, 20, 7, 19, imSize=(W, H))
    try:
        for _ in range(2):
            g = ge.fisheye(imL, imR, laps[0], laps[1])
            assert np.array_equal(kL.view(np.uint8), g["kpsL"].view(np.uint8)) and np.array_equal(kR.view(np.uint8), g["kpsR"].view(np.uint8))
            assert np.array_equal(dL, g["descL"]) and np.array_equal(dR, g["descR"])
            assert (mL, mR) == (g["monoLeft"], g["monoRight"])
            assert np.array_equal(cand, g["right_idx"]) and np.array_equal(d2, g["dist2"]) and n == g["ncand"]
            _stages_equal("fisheye right", ge.ctx, e)                      # the context's last extraction is the right image's
        assert n > 50
        if laps[0] != (0, 508):
            assert 0 < mL < len(kL) and 0 < mR < len(kR)
    finally:
        ge.ctx.close()
