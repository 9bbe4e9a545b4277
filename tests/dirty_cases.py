"""One table, keyed by export name, of what tests/test_gpu_dirty.py runs on dirty device memory and what it expects.

Every name of eorb_slam_amd._lib.EXPORTS has an entry (tests/test_dirty_cases_table.py holds the table to that):
  * a list of Case: the export lays a call out in the context's arena (or reaches one of the shared bodies that do).  run(fe, ctx) calls
    it through the front end on the given context and returns a dict of arrays, want() returns the same dict from the CPU side the
    export's parity test uses (oracle/, tests/*_ref, tests/*_model.py) -- never from the device.  run_big(fe, ctx) is the same entry point
    on a scene about three times as large with another seed; its results are thrown away (it only leaves the arena full of values that
    look like results);
  * WALK: a *_dev batch entry; its buffers are the caller's and its workspaces persist, so a per-call fill does not reach them: the shape
    walks of tests/test_gpu_dirty.py cover it;
  * a str: why the export needs no case (no arena, no ensure(): a setter, a getter, a host function).

Sizes are the smallest at which a tail exists: counts that are no multiple of 4, 16 or 64 (3, 63, 65), images of 70 x 50 and 64 x 48, K = 3
problems or keyframes with the skipped / empty one in the middle.  The references are computed once per case (Case.want caches)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eorb_slam_amd import _lib, synth               # noqa: E402

F32 = np.float32
W, H = 70, 50                                       # the image of every case that needs one
WALK = "walk"


def orc():
    from oracle import oracle_py
    oracle_py.build()
    return oracle_py


class Case:
    """make(big) -> (run(fe, ctx) -> dict, want() -> dict); canon: every NaN counts as one NaN (host and device give them other sign
    and payload bits), as the export's parity test does it"""

    def __init__(self, name, make, canon=False):
        self.name, self.make, self.canon = name, make, canon
        self._built = {}
        self._want = None

    def _get(self, big):
        if big not in self._built:
            self._built[big] = self.make(big)
        return self._built[big]

    def run(self, fe, ctx):
        return self._get(False)[0](fe, ctx)

    def run_big(self, fe, ctx):
        return self._get(True)[0](fe, ctx)

    def want(self):
        if self._want is None:
            self._want = self._get(False)[1]()
        return self._want


def canon(a):
    a = np.ascontiguousarray(np.asarray(a))
    if a.dtype in (np.float32, np.float64):
        a = a.copy()
        a[np.isnan(a)] = np.nan
    return a


def same(got, want, what, nan_canon=False):
    """both dicts hold the same names; every array equal in dtype, shape and bytes.  The message names the case, the state, the first
    output that differs and where"""
    assert sorted(got) == sorted(want), "%s: outputs %s, the reference has %s" % (what, sorted(got), sorted(want))
    for k in want:
        g, w = np.ascontiguousarray(np.asarray(got[k])), np.ascontiguousarray(np.asarray(want[k]))
        if nan_canon:
            g, w = canon(g), canon(w)
        if g.dtype != w.dtype and g.dtype.kind in "iub" and w.dtype.kind in "iub":      # (integers compare by value, as np.array_equal does)
            g, w = g.astype(np.int64), w.astype(np.int64)
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s %s, the reference %s %s" % (what, k, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            gb = g.reshape(-1).view(np.uint8).reshape(g.size, -1) if g.size else g.reshape(0, 1)
            wb = w.reshape(-1).view(np.uint8).reshape(w.size, -1) if w.size else w.reshape(0, 1)
            bad = np.flatnonzero((gb != wb).any(axis=1))
            i = int(bad[0])
            raise AssertionError("%s: %s differs in %d of %d places, first at flat index %d: device %r, reference %r"
                                 % (what, k, len(bad), g.size, i, g.reshape(-1)[i], w.reshape(-1)[i]))


def _i(x):
    return np.int64(x)


def _kp(k):
    """records (keypoints, events) as rows of bytes"""
    k = np.ascontiguousarray(k)
    return k.view(np.uint8).reshape(len(k), k.dtype.itemsize)


def _only(d, keys):
    return {k: np.asarray(d[k]) for k in keys}


def _opt(a, dt=np.uint8):
    return np.zeros(0, dt) if a is None else a


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------------------------------------------------
# event images
def _events(n, seed):
    ev = synth.random_events(n, W, H, seed=seed, frac=True)
    return ev


def _img3(f32, u8, mm):
    return dict(f32=f32, u8=_opt(u8), mm=np.asarray(mm, F32))


def _gauss(n, pol, count=False):
    def make(big):
        ev = _events(3 * n + 2 if big else n, 40 + big)

        def run(fe, ctx):
            if count:
                return _img3(*fe.EvImConverter.ev2im(ev, W, H, pol, True, ctx=ctx, return_all=True))
            return _img3(*fe.EvImConverter.ev2im_gauss(ev, W, H, 1.0, pol, True, ctx=ctx, return_all=True))

        def want():
            return _img3(*(orc().ev2im(ev, W, H, pol, True) if count else orc().ev2im_gauss(ev, W, H, 1.0, pol, True)))
        return run, want
    return make


def maps(off=0.0):
    """undistortion maps of the W x H sensor that move a pixel by up to two pixels (off = 0) or out of the image (off = -100)"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    r2 = ((xx - 33.0) / 40.0) ** 2 + ((yy - 26.0) / 40.0) ** 2
    mx = (xx + (xx - 33.0) * (0.08 * r2 - 0.03 * r2 * r2) + 0.37 + off).astype(F32)
    my = (yy + (yy - 26.0) * (0.08 * r2 - 0.03 * r2 * r2) - 0.21 + off).astype(F32)
    return mx, my


def _raw(n, seed):
    return synth.random_raw_events(n, W, H, seed=seed)


def _gauss_raw(n, pol, count=False):
    def make(big):
        raw = _raw(3 * n + 2 if big else n, 50 + big)
        mx, my = maps()

        def run(fe, ctx):
            fe.EvImConverter.set_undistort_maps(mx, my, True, ctx=ctx)
            if count:
                return _img3(*fe.EvImConverter.ev2im_raw(raw, W, H, pol, True, ctx=ctx, return_all=True))
            return _img3(*fe.EvImConverter.ev2im_gauss_raw(raw, W, H, 1.0, pol, True, ctx=ctx, return_all=True))

        def want():
            ev = orc().undistort_events(raw, mx, my, W, H, True, 1.0)
            return _img3(*(orc().ev2im(ev, W, H, pol, True) if count else orc().ev2im_gauss(ev, W, H, 1.0, pol, True)))
        return run, want
    return make


def _undistort_events(n, off):
    def make(big):
        raw = _raw(3 * n + 2 if big else n, 60 + big)
        mx, my = maps(0.0 if big else off)

        def run(fe, ctx):
            fe.EvImConverter.set_undistort_maps(mx, my, True, ctx=ctx)
            return dict(ev=_kp(fe.EvImConverter.undistort_events(raw, W, H, 1e6, ctx=ctx)))

        def want():
            return dict(ev=_kp(orc().undistort_events(raw, mx, my, W, H, True, 1e6)))
        return run, want
    return make


def _text(n, seed):
    rng = np.random.default_rng(seed)
    ts = np.cumsum(rng.integers(1, 2000, n)) * 1e-6
    lines = [b"# events: ts x y p", b""]
    for i in range(n):
        tss = ("%.9f" % ts[i], "%.6f" % (1468941032.0 + ts[i]), "%d" % int(ts[i] * 1e6))[i % 3]
        lines.append(("%s %d %d %d%s" % (tss, rng.integers(0, W), rng.integers(0, H), rng.integers(0, 2), "\r" if i % 11 == 0 else "")).encode())
        if i % 20 == 7:
            lines.append(b"   # a comment in the middle")
    return b"\n".join(lines)


def _parse(n):
    def make(big):
        text = _text(3 * n + 2 if big else n, 23 + big)

        def run(fe, ctx):
            return dict(ev=_kp(fe.EvImConverter.parse_events_text(text, ctx=ctx)))

        def want():
            return dict(ev=_kp(orc().parse_events_text(text)))
        return run, want
    return make


CAM = (60.0, 59.5, 35.5, 24.5)                      # a pinhole camera of the W x H image
KB8 = (60.0, 59.5, 35.5, 24.5, -0.048, 0.011, -0.055, 0.021)
AXIS = np.array([0.12, -0.3, 0.946484], np.float64) / np.linalg.norm([0.12, -0.3, 0.946484])
TVEC = np.array([0.013, -0.007, 0.002])
SE2 = np.array([0.03, 0.4, -0.3], F32)


def _mci(n, kind, cam, pol, export=False):
    """kind "se3" / "se2"; export: the pinhole-only entry points eorb_ev2mci_se3 / eorb_ev2mci_se2, through the raw ABI"""
    def make(big):
        ev = _events(3 * n + 2 if big else n, 70 + big)
        ev["ts"] = np.sort(ev["ts"])

        def run(fe, ctx):
            if not export:
                if kind == "se3":
                    return _img3(*fe.EvImConverter.ev2mci_gg_f_se3(ev, cam, 0.031, AXIS, TVEC, 1.7, W, H, 1.0, pol, True, ctx=ctx))
                return _img3(*fe.EvImConverter.ev2mci_gg_f_se2(ev, cam, SE2, W, H, 1.0, pol, True, ctx=ctx))
            e = np.ascontiguousarray(ev, synth.EVENT_DTYPE)
            ph = _lib.Pinhole(*[float(v) for v in cam])
            f32 = np.empty((H, W), F32); u8 = np.zeros((H, W), np.uint8); mm = np.zeros(2, F32)
            if kind == "se3":
                ctx.check(ctx.L.eorb_ev2mci_se3(ctx.h, _p(e), len(e), C.byref(ph), 0.031, _p(AXIS), _p(TVEC), 1.7, None, W, H, 1.0, int(pol), 1,
                                                _p(f32), _p(u8), _p(mm)))
            else:
                ctx.check(ctx.L.eorb_ev2mci_se2(ctx.h, _p(e), len(e), C.byref(ph), _p(SE2), len(SE2), W, H, 1.0, int(pol), 1, _p(f32), _p(u8), _p(mm)))
            return _img3(f32, u8, mm)

        def want():
            if kind == "se3":
                return _img3(*orc().ev2mci_se3(ev, cam, 0.031, AXIS, TVEC, 1.7, W, H, 1.0, pol, True))
            return _img3(*orc().ev2mci_se2(ev, cam, SE2, W, H, 1.0, pol, True))
        return run, want
    return make


def _float_images(n, seed, flat_at=None):
    rng = np.random.default_rng(seed)
    imgs = rng.uniform(0, 9, (n, H, W)).astype(F32)
    for k in range(n):
        imgs[k] = np.cumsum(imgs[k], axis=1) * F32(0.1 + k)
    if flat_at is not None:
        imgs[flat_at] = F32(2.5)
    return imgs


def _focus(n, single=False):
    def make(big):
        imgs = _float_images(3 * n if big else n, 5 + big, flat_at=None if big or single else n // 2)

        def run(fe, ctx):
            if single:
                return dict(focus=np.array([fe.EvImConverter.measureImageFocus(imgs[0], ctx=ctx)], F32))
            return dict(focus=fe.EvImConverter.measureImageFocusN(imgs, ctx=ctx))

        def want():
            return dict(focus=np.array([orc().measure_image_focus(im) for im in (imgs[:1] if single else imgs)], F32))
        return run, want
    return make


def _normalize(flat):
    def make(big):
        img = _float_images(1, 9 + big, flat_at=0 if flat and not big else None)[0]

        def run(fe, ctx):
            return dict(u8=fe.cv_normalize_minmax_u8(img, ctx=ctx))

        def want():
            return dict(u8=orc().cv_normalize_minmax_u8(img))
        return run, want
    return make


# ---------------------------------------------------------------------------------------------------------------------------------------
# the calibrator
def _cal():
    return dict(synth.CALIBRATIONS["EvETHZ"])


def _undist(n, points):
    def make(big):
        import calib_ref
        d = _cal()
        kps = synth.calib_keypoints(3 * n + 2 if big else n, *d["size"], seed=100 + big, margin=0.1)

        def run(fe, ctx):
            cal = fe.MyCalibrator.from_dict(d, ctx=ctx)
            if points:
                return dict(xy=cal.undistPoint(np.stack([kps["x"], kps["y"]], axis=1)))
            return dict(kps=_kp(cal.undistKeyPoints(kps)))

        def want():
            if points:
                return dict(xy=calib_ref.undistort_points(d, np.stack([kps["x"], kps["y"]], axis=1)))
            return dict(kps=_kp(calib_ref.undistort_keypoints(d, kps)))
        return run, want
    return make


def _gen_maps():
    def make(big):
        import calib_ref
        d = _cal()
        size = (3 * W + 1, 2 * H + 1) if big else (W, H)

        def run(fe, ctx):
            mx, my = fe.MyCalibrator.from_dict(d, ctx=ctx).generateUndistMaps(True, size=size)
            return dict(mx=mx, my=my)

        def want():
            mx, my = calib_ref.generate_maps(d, *size)
            return dict(mx=mx, my=my)
        return run, want
    return make


# ---------------------------------------------------------------------------------------------------------------------------------------
# the extractor.  One level (a 70 x 50 image holds no second one), edge threshold 9, FAST 20 / 7
ORB1 = dict(nfeatures=200, scaleFactor=1.2, nlevels=1, iniThFAST=20, minThFAST=7, edgeTh=9)
ORB_BIG = dict(nfeatures=600, scaleFactor=1.2, nlevels=2, iniThFAST=20, minThFAST=7, edgeTh=19)
BIG_W, BIG_H = 173, 131                             # the larger call's image: three times the pixels and a second level


def image(seed, w=W, h=H):
    return synth.texture_image(w, h, seed=seed)


def flat(w=W, h=H):
    return np.full((h, w), 128, np.uint8)


def half_flat(seed):
    """texture on the left half only: cells without a corner beside cells with some"""
    im = image(seed)
    im[:, W // 2:] = 128
    return im


def _ext_args(big):
    return (ORB_BIG, BIG_W, BIG_H) if big else (ORB1, W, H)


def _ext4(mono, kps, desc, oob):
    n = 0 if kps is None else len(kps)
    return dict(mono=_i(mono), kps=_kp(kps) if n else np.zeros((0, synth.KP_DTYPE.itemsize), np.uint8),
                desc=np.asarray(desc, np.uint8).reshape(n, 32) if n else np.zeros((0, 32), np.uint8), oob=np.asarray(oob, np.uint8) if n else np.zeros(0, np.uint8))


def _extract(img_of, lap=(0, 1000)):
    def make(big):
        p, w, h = _ext_args(big)
        img = image(31, w, h) if big else img_of()

        def run(fe, ctx):
            ge = fe.ORBextractor(imSize=(w, h), ctx=ctx, **p)
            return _ext4(*ge(img, lap))

        def want():
            return _ext4(*orc().OrbExtractor(imWidth=w, **p).extract(img, lap))
        return run, want
    return make


def _frame_mono(img_of):
    def make(big):
        import calib_ref
        p, w, h = _ext_args(big)
        img = image(32, w, h) if big else img_of()
        d = _cal()

        def run(fe, ctx):
            ge = fe.ORBextractor(imSize=(w, h), ctx=ctx, **p)
            fe.MyCalibrator.from_dict(d, ctx=ctx)
            g = ge.frame_mono(img)
            return dict(_ext4(g["mono"], g["kps"], g["desc"], g["oob"]), kps_un=_kp(g["kps_un"]), bounds=g["bounds"])

        def want():
            mono, kps, desc, oob = orc().OrbExtractor(imWidth=w, **p).extract(img)
            un = calib_ref.undistort_keypoints(d, kps) if kps is not None and len(kps) else np.zeros(0, synth.KP_DTYPE)
            return dict(_ext4(mono, kps, desc, oob), kps_un=_kp(un), bounds=np.asarray(calib_ref.image_bounds(d, w, h), F32))
        return run, want
    return make


MB, MBF = 0.11, 8.0


def _stereo(right_of):
    def make(big):
        p, w, h = _ext_args(big)
        left, pair_right = synth.stereo_pair(33 + big, w, h, 6)
        right = pair_right if big else right_of(left, pair_right)

        def run(fe, ctx):
            ge = fe.ORBextractor(imSize=(w, h), ctx=ctx, **p)
            g = ge.stereo(left, right, MB, MBF)
            return dict(kpsL=_kp(g["kpsL"]), descL=g["descL"], kpsR=_kp(g["kpsR"]), descR=g["descR"], uRight=g["uRight"], depth=g["depth"],
                        nmatches=_i(g["nmatches"]))

        def want():
            oL, oR = orc().OrbExtractor(imWidth=w, **p), orc().OrbExtractor(imWidth=w, **p)
            _, kL, dL, _ = oL.extract(left, (0, 0)); _, kR, dR, _ = oR.extract(right, (0, 0))
            ur, dp, nm = oL.compute_stereo_matches(oR, kL, dL, kR, dR, MB, MBF)
            return dict(kpsL=_kp(kL), descL=dL, kpsR=_kp(kR), descR=dR, uRight=ur, depth=dp, nmatches=_i(nm))
        return run, want
    return make


def _fisheye(right_of, laps):
    def make(big):
        p, w, h = _ext_args(big)
        left = image(35 + big, w, h)
        right = np.ascontiguousarray(np.roll(left, -3, axis=1)) if big else right_of(left)
        lapL, lapR = ((0, w), (0, w)) if big else laps

        def run(fe, ctx):
            ge = fe.ORBextractor(imSize=(w, h), ctx=ctx, **p)
            g = ge.fisheye(left, right, lapL, lapR)
            return dict(kpsL=_kp(g["kpsL"]), descL=g["descL"], monoLeft=_i(g["monoLeft"]), kpsR=_kp(g["kpsR"]), descR=g["descR"],
                        monoRight=_i(g["monoRight"]), right_idx=g["right_idx"], dist2=g["dist2"], ncand=_i(g["ncand"]))

        def want():
            oe = orc().OrbExtractor(imWidth=w, **p)
            mL, kL, dL, _ = oe.extract(left, lapL); mR, kR, dR, _ = oe.extract(right, lapR)
            nc, cand, d2 = orc().fisheye_matches(dL, mL, dR, mR)
            return dict(kpsL=_kp(kL), descL=dL, monoLeft=_i(mL), kpsR=_kp(kR), descR=dR, monoRight=_i(mR), right_idx=cand, dist2=d2, ncand=_i(nc))
        return run, want
    return make


def _tracked(assign):
    def make(big):
        p, w, h = _ext_args(big)
        img = image(37 + big, w, h)
        oe = orc().OrbExtractor(imWidth=w, **p)
        _, kps, desc, _ = oe.extract(img)
        rng = np.random.default_rng(7)
        tk = kps.copy()
        tk["x"] += rng.normal(0, 1.5, len(tk)).astype(F32); tk["y"] += rng.normal(0, 1.5, len(tk)).astype(F32)
        tk["octave"][::7] = p["nlevels"]; tk["octave"][3::11] = -1           # outside the levels: no descriptor, every level tried
        tk["x"][::13] = 3.5

        def run(fe, ctx):
            ge = fe.ORBextractor(imSize=(w, h), ctx=ctx, **p)
            if assign:
                return dict(kps=_kp(ge.AssignKPtLevelByBestDesc(desc, img, tk)))
            d, o = ge.ComputeTrackedKPtsDesc(img, tk)
            return dict(desc=d, oob=o)

        def want():
            if assign:
                return dict(kps=_kp(oe.assign_level_by_best_desc(img, desc, tk)))
            d, o = oe.tracked_descriptors(img, tk)
            return dict(desc=d, oob=o)
        return run, want
    return make


# ---- the L1 chain's one-call seams -----------------------------------------------------------------------------------------------------
L1 = dict(maxNumPts=100, fastTh=0, imMargin=9)


def _slice_events(n, seed, motion=0.4):
    return np.ascontiguousarray(synth.shapes_events(n, W, H, seed=seed, motion=motion, undistort=False))


def _l1_builder(fe, ctx):
    """the contest's builder: the context is its own L2 context too (the contest extracts with the L2 tracker's 2 x maxNumPts)"""
    return fe.EvImBuilder(W, H, cam=CAM, ctx=ctx, ctx_l2=ctx, **L1)


def _sl_extract(fe, ctx, ev):
    ge = fe.ORBextractor(L1["maxNumPts"], 1.0, 1, L1["fastTh"], 0, L1["imMargin"], imSize=(W, H), ctx=ctx)
    kps = np.zeros(ge.cap, synth.KP_DTYPE); n = C.c_int(0); mono = C.c_int(0); img = np.zeros((H, W), np.uint8)
    ctx.check(ctx.L.eorb_ev_slice_extract(ctx.h, _p(ev), None, len(ev), 1.0, 0, 1000, 0, _p(kps), None, None, ge.cap, C.byref(n), C.byref(mono), _p(img)))
    return kps[:n.value].copy(), img


def _sl_track(fe, ctx, ev, pts):
    klt = _lib.KltParams(23, 1, 10, 0.03, 1e-4)
    pts = np.ascontiguousarray(pts, F32).copy(); n = len(pts)
    st = np.zeros(max(n, 1), np.uint8); er = np.zeros(max(n, 1), F32); img = np.zeros((H, W), np.uint8)
    ctx.check(ctx.L.eorb_ev_slice_track(ctx.h, _p(ev), None, len(ev), 1.0, C.byref(klt), _p(pts), _p(st), _p(er), n, _p(img)))
    return pts, st[:n], er[:n], img


def _slice(which, n=2003):
    """which: "extract" (keypoints and image of the INIT frame), "image" (eorb_ev_slice_image after it), "track" (the next chunk's LK)"""
    def make(big):
        e0, e1 = _slice_events(3 * n + 2 if big else n, 30 + big), _slice_events(3 * n + 2 if big else n, 31 + big, 0.7)

        def run(fe, ctx):
            kps, img = _sl_extract(fe, ctx, e0)
            if which == "extract":
                return dict(kps=_kp(kps), img=img)
            if which == "image":
                lazy = np.zeros((H, W), np.uint8)
                ctx.check(ctx.L.eorb_ev_slice_image(ctx.h, _p(lazy)))
                return dict(img=lazy)
            ref = np.stack([kps["x"], kps["y"]], axis=1).astype(F32)
            pts, st, er, cur = _sl_track(fe, ctx, e1, ref)
            return dict(pts=pts, status=st, err=er, img=cur)

        def want():
            o = orc()
            u8 = o.ev2im_gauss(e0, W, H, 1.0, False, True)[1]
            _, kps, _, _ = o.OrbExtractor(L1["maxNumPts"], 1.0, 1, L1["fastTh"], 0, edgeTh=L1["imMargin"], imWidth=W).extract(u8, (0, 1000), False)
            if which == "extract":
                return dict(kps=_kp(kps), img=u8)
            if which == "image":
                return dict(img=u8)
            cur = o.ev2im_gauss(e1, W, H, 1.0, False, True)[1]
            ref = np.stack([kps["x"], kps["y"]], axis=1).astype(F32)
            pts, st, er = o.calc_optical_flow_pyr_lk(u8, cur, ref, ref, 23, 1, 10, 0.03, 4)
            return dict(pts=pts, status=st, err=er, img=cur)
        return run, want
    return make


def _contest(n, which):
    """which: the methods that take part ("all", "none": the event histogram alone)"""
    def make(big):
        evs = _slice_events(3 * n + 2 if big else n, 9 + big, motion=6.0)
        p = synth.l1_mci_poses(evs)
        poses = None if which == "none" and not big else p

        def run(fe, ctx):
            g = _l1_builder(fe, ctx).generateMCImage(evs, poses)
            return dict(focus=g["focus"], winner=_i(g["winner"]), image=g["image"], l2_kps=_kp(g["l2_kps"]))

        def want():
            from oracle import orc_chain
            l2 = orc().OrbExtractor(2 * L1["maxNumPts"], 1.0, 1, L1["fastTh"], 0, edgeTh=L1["imMargin"], imWidth=W, fast=True)
            g = orc_chain.generate_mc_image(evs, W, H, 1.0, CAM, poses, l2, fast=True)
            return dict(focus=np.asarray(g["focus"], F32), winner=_i(g["winner"]), image=g["image"], l2_kps=_kp(g["l2_kps"]))
        return run, want
    return make


# ---------------------------------------------------------------------------------------------------------------------------------------
# the window matchers on the planted scenes of tests/match_scenes.py (the larger call: the scene three times over)
def _tile(sc, times=3):
    out = dict(sc)
    lens = {len(sc["s_kps"]), len(sc["q_kps"]) if "q_kps" in sc else -1, len(sc["uv"])}
    for k, v in sc.items():
        if isinstance(v, np.ndarray) and v.ndim >= 1 and len(v) in lens and v.dtype.kind != "U":
            out[k] = np.ascontiguousarray(np.concatenate([v] * times))
    return out


def _mres(r):
    d = dict(n=_i(r[0]), m=np.asarray(r[1]))
    if len(r) > 2:
        d["prev"] = np.asarray(r[2])
    return d


def _window(kind, form, empty=False):
    """empty: no query is valid / no searched keypoint is free -- the matcher lists no candidate at all"""
    def make(big):
        import match_scenes as ms
        sc = ms.window_scene(kind, False)
        cfg = dict(ms.MAIN[kind], form=form)
        if big:                                                             # (the positions scene of "init" is 20 times the base scene as it is)
            sc = ms.window_scene(kind, True) if kind == "init" else _tile(ms.window_scene(kind, True))
        elif empty:
            sc = dict(sc)
            if kind == "init":
                sc["uv"] = np.full_like(sc["uv"], -1000.0)
            else:
                sc["q_valid"] = np.zeros_like(sc["q_valid"])

        def run(fe, ctx):
            return _mres(ms.run_kernels(fe, ctx, sc, cfg, True))

        def want():
            return _mres(ms.run_oracle(orc(), sc, cfg, True))
        return run, want
    return make


def _twocam(kind, name):
    def make(big):
        import twocam_scenes as ts
        by = dict(ts.scenes(kind))
        sc = by["crowded" if kind != "bow" else "base"] if big else by[name]
        cfg = ts.MAIN[kind]

        def run(fe, ctx):
            return _mres(ts.run_kernels(fe, ctx, kind, sc, cfg, True))

        def want():
            return _mres(ts.run_oracle(orc(), kind, sc, cfg, True))
        return run, want
    return make


# ---- the node walks ----------------------------------------------------------------------------------------------------------------------
def _node_single(kind):
    """SearchByBoW, SearchByBoW(KF, KF), SearchForTriangulation on the planted node scene; the larger call: a neighbourhood of
    tests/kfbatch_cases.py through the same entry point"""
    def make(big):
        import kfbatch_cases as kc
        import match_scenes as ms
        sc = ms.node_scene(kind)
        cfg = ms.NODE_MAIN[kind]

        def run(fe, ctx):
            if not big:
                return _mres(ms.run_node_kernels(fe, ctx, [sc], cfg, True, False)[0])
            if kind == "tri":
                s = kc.tri_scene("pinhole", 4); kf = s["kfs"][0]
                fe.SearchForTriangulation(s["kps1"], s["desc1"], s["elig1"], s["fv1"], kf["kps"], kf["desc"], kf["elig"], kf["fv"], s["ep"][0], s["F12"][0],
                                          s["scale2"], s["sigma2_2"], False, True, ctx=ctx)
            else:
                s = kc.bow_scene("big", 4); kf = s["kfs"][0]
                if kind == "bowkf":
                    fe.SearchByBoW_KF(s["kps"], s["desc"], s["has_mp"], s["fv"], kf["kps"], kf["desc"], kf["has_mp"], kf["fv"], 0.8, True, ctx=ctx)
                else:
                    fe.SearchByBoW(kf["kps"], kf["desc"], kf["has_mp"], kf["fv"], s["kps"], s["desc"], s["fv"], 0.7, True, ctx=ctx)
            return {}

        def want():
            return _mres(ms.run_node_oracle(orc(), sc, cfg, True))
        return run, want
    return make


EMPTY_FV = (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.int32))


def _tri_single_no_candidate():
    """SearchForTriangulation on a pair without a vocabulary node in common: zero candidates"""
    def make(big):
        import kfbatch_cases as kc
        s = kc.tri_scene("pinhole", 4) if big else _small_tri("pinhole")
        kp2, d2, e2, fv2 = kc.tri_set(s, [0])[0] if big else _no_common_node(kc.tri_set(s, [0])[0])

        def run(fe, ctx):
            n, pairs = fe.SearchForTriangulation(s["kps1"], s["desc1"], s["elig1"], s["fv1"], kp2, d2, e2, fv2, s["ep"][0], s["F12"][0], s["scale2"],
                                                 s["sigma2_2"], False, True, ctx=ctx)
            m = np.full(len(s["kps1"]), -1, np.int32)
            m[pairs[:, 0]] = pairs[:, 1]
            return dict(n=_i(n), m=m)

        def want():
            n, m = orc().search_for_triangulation(s["kps1"], s["desc1"], s["elig1"], s["fv1"], kp2, d2, e2, fv2, s["ep"][0], s["F12"][0], s["scale2"],
                                                  s["sigma2_2"], False, True)
            return dict(n=_i(n), m=np.asarray(m, np.int32))
        return run, want
    return make


def _no_common_node(kf):
    """the keyframe with every node id moved past the other side's: no vocabulary node in common"""
    kps, desc, flag, fv = kf
    return (kps, desc, flag, ((np.asarray(fv[0], np.uint32) + np.uint32(1 << 20)), fv[1], fv[2]))


def _rows(nm, m):
    return dict(n=np.asarray(nm, np.int32), m=np.asarray(m, np.int32))


def _tri_batch(kind, middle):
    """K = 3 keyframes [A, middle, B] of a triangulation neighbourhood; middle: "no_node" (no node in common with pKF1: zero candidates),
    "empty" (a keyframe without rows)"""
    def make(big):
        import kfbatch_cases as kc
        s = kc.tri_scene(kind, 4 if kind.startswith("pinhole") else 3) if big else _small_tri(kind)
        ks = list(range(len(s["kfs"]))) if big else [0, 1, 2]
        kfs = kc.tri_set(s, ks)
        if not big:
            kfs[1] = _no_common_node(kfs[1]) if middle == "no_node" else (kfs[1][0][:0], kfs[1][1][:0], kfs[1][2][:0], EMPTY_FV)

        def run(fe, ctx):
            if "F12" in s:
                return _rows(*fe.SearchForTriangulationKeyFrames(s["kps1"], s["desc1"], s["elig1"], s["fv1"], kfs, s["ep"][ks], s["F12"][ks], s["scale2"],
                                                                 s["sigma2_2"], False, True, ctx=ctx))
            nl2 = [s["kfs"][k]["nleft"] if len(kfs[i][0]) else (-1 if s["nleft1"] < 0 else 0) for i, k in enumerate(ks)]
            return _rows(*fe.SearchForTriangulationKB8KeyFrames(s["kps1"], s["nleft1"], s["desc1"], s["elig1"], s["fv1"], kfs, nl2, s["cams1"], s["cams2"],
                                                                s["Rt"][ks], s["ep"][ks], s["scale2"], s["sigma2_1"], s["sigma2_2"], False, True, ctx=ctx))

        def want():
            o = orc()
            nm, rows = [], []
            for i, k in enumerate(ks):
                kp2, d2, e2, fv2 = kfs[i]
                if len(kp2) == 0:                                           # (ORBmatcher.cc:975-: no feature vector entry, no match)
                    n, m = 0, np.full(len(s["kps1"]), -1, np.int32)
                elif "F12" in s:
                    n, m = o.search_for_triangulation(s["kps1"], s["desc1"], s["elig1"], s["fv1"], kp2, d2, e2, fv2, s["ep"][k], s["F12"][k], s["scale2"],
                                                      s["sigma2_2"], False, True)
                else:
                    n, m = o.search_for_triangulation_kb8(s["kps1"], s["nleft1"], s["desc1"], s["elig1"], s["fv1"], kp2, s["kfs"][k]["nleft"], d2, e2, fv2,
                                                          s["cams1"], s["cams2"], s["Rt"][k], s["ep"][k], s["scale2"], s["sigma2_1"], s["sigma2_2"], False, True)
                nm.append(n); rows.append(m)
            return _rows(nm, np.stack(rows))
        return run, want
    return make


_SMALL = {}


def _small_tri(kind):
    """a neighbourhood of 63-odd points: about 65 rows per keyframe, six nodes"""
    if kind not in _SMALL:
        kw = dict(npts=63, ndistract=9, nties=4, nnodes=6, angle_step=50.0)
        _SMALL[kind] = synth.triangulation_neighbourhood(301, 3, pinhole=kind == "pinhole", twocam=kind == "twocam", **kw)
    return _SMALL[kind]


def _small_bow():
    if "bow" not in _SMALL:
        _SMALL["bow"] = synth.bow_neighbourhood(302, 3, npts=63, ndistract=9, nties=4, nnodes=6, angle_step=50.0)
    return _SMALL["bow"]


def _bow_batch(kf_kf):
    def make(big):
        import kfbatch_cases as kc
        s = kc.bow_scene("big", 4) if big else _small_bow()
        kfs = kc.bow_set(s)
        if not big:
            kfs[1] = _no_common_node(kfs[1])
        ratio = 0.8 if kf_kf else 0.7

        def run(fe, ctx):
            if kf_kf:
                return _rows(*fe.SearchByBoW_KF_KeyFrames(s["kps"], s["desc"], s["has_mp"], s["fv"], kfs, ratio, True, ctx=ctx))
            return _rows(*fe.SearchByBoWKeyFrames(kfs, s["kps"], s["desc"], s["fv"], ratio, True, ctx=ctx))

        def want():
            o = orc()
            nm, rows = [], []
            for kp2, d2, f2, fv2 in kfs:
                if kf_kf:
                    n, m = o.search_by_bow_kf(s["kps"], s["desc"], s["has_mp"], s["fv"], kp2, d2, f2, fv2, ratio, True)
                else:
                    n, m = o.search_by_bow(kp2, d2, f2, fv2, s["kps"], s["desc"], s["fv"], ratio, True)
                nm.append(n); rows.append(m)
            return _rows(nm, np.stack(rows))
        return run, want
    return make


def _tri_kb8_single():
    def make(big):
        s = synth.keyframe_pair(seed=3 + big, npts=600 if big else 63, ndistract=150 if big else 9, nties=30 if big else 4, nnodes=60 if big else 6)

        def run(fe, ctx):
            n, pairs = fe.SearchForTriangulationKB8(s["kps1"], s["nleft1"], s["desc1"], s["elig1"], s["fv1"], s["kps2"], s["nleft2"], s["desc2"], s["elig2"],
                                                    s["fv2"], s["cams1"], s["cams2"], s["Rt"], s["ep"], s["scale2"], s["sigma2_1"], s["sigma2_2"], False, True,
                                                    ctx=ctx)
            m = np.full(len(s["kps1"]), -1, np.int32)
            m[pairs[:, 0]] = pairs[:, 1]
            return dict(n=_i(n), m=m)

        def want():
            n, m = orc().search_for_triangulation_kb8(**s, coarse=False, checkOri=True)
            return dict(n=_i(n), m=np.asarray(m, np.int32))
        return run, want
    return make


def _kb8_triangulate(n):
    def make(big):
        rng = np.random.default_rng(5 + big)
        N = 3 * n + 2 if big else n
        R2 = synth.rot(0.03, -0.08, 0.02); t2 = np.array([-0.35, 0.04, 0.06], F32)
        Rt = synth.rel_pose(np.eye(3, dtype=F32), np.zeros(3, F32), R2, t2)
        R = Rt[:9].reshape(3, 3).astype(np.float64); t = Rt[9:].astype(np.float64)
        z = rng.uniform(0.5, 12.0, N)
        X = np.stack([rng.uniform(-1.2, 1.2, N) * z, rng.uniform(-1.2, 1.2, N) * z, z], axis=1)
        uv1 = synth.project_np(synth.CAM_MONO, X); uv2 = synth.project_np(synth.CAM_MONO, (X - t) @ R)
        _, sig = synth.level_tables()
        k1 = np.zeros(N, synth.KP_DTYPE); k2 = np.zeros(N, synth.KP_DTYPE)
        k1["x"], k1["y"], k1["octave"] = uv1[:, 0], uv1[:, 1], rng.integers(0, 8, N)
        k2["x"], k2["y"], k2["octave"] = uv2[:, 0] + rng.normal(0, 1.5, N), uv2[:, 1] + rng.normal(0, 1.5, N), rng.integers(0, 8, N)

        def run(fe, ctx):
            return dict(z=fe.KB8TriangulateMatches(synth.CAM_MONO, synth.CAM_MONO, Rt, k1, k2, sig, sig, ctx=ctx))

        def want():
            return dict(z=orc().triangulate_batch(synth.CAM_MONO, synth.CAM_MONO, Rt, k1, k2, sig, sig))
        return run, want
    return make


# ---- the small helpers -------------------------------------------------------------------------------------------------------------------
def _knn(nq, nt):
    def make(big):
        q = synth.random_descriptors(3 * nq + 2 if big else nq, seed=14 + big); t = synth.random_descriptors(3 * nt + 2 if big else nt, seed=4 + big)
        if nt:
            q[::5] = t[(np.arange(len(q[::5])) * 7) % len(t)]                 # exact copies: distance 0, and equal rows tie
            t[len(t) // 2] = t[0]

        def run(fe, ctx):
            idx, dist = fe.BFMatcher(ctx).knnMatch2(q, t)
            return dict(idx=idx, dist=dist)

        def want():
            import helper_models as hm
            idx, dist = hm.knn2(q, t)
            return dict(idx=np.asarray(idx, np.int32), dist=np.asarray(dist, np.int32))
        return run, want
    return make


def _window_match():
    def make(big):
        import helper_models as hm
        import helper_scenes as hs
        q, t, offs, cand, _ = hs.window_scene()
        if big:
            q = np.concatenate([q] * 3); cand = np.concatenate([cand] * 3)
            offs = np.concatenate([offs[:-1] + k * offs[-1] for k in range(3)] + [[3 * offs[-1]]]).astype(np.int32)

        def run(fe, ctx):
            return dict(zip(("bi", "bd", "si", "sd"), fe.HammingWindowMatch(q, t, offs, cand, ctx=ctx)))

        def want():
            return dict(zip(("bi", "bd", "si", "sd"), [np.asarray(a, np.int32) for a in hm.window_match(q, t, offs, cand)]))
        return run, want
    return make


def _distinctive():
    def make(big):
        import helper_models as hm
        import helper_scenes as hs
        desc, offs, _ = hs.distinctive_scene()
        if not big:                                                         # the points of up to 65 rows, the empty ones between them
            keep = np.flatnonzero(np.diff(offs) <= 65)
            desc = np.concatenate([desc[offs[m]:offs[m + 1]] for m in keep]); offs = np.concatenate([[0], np.cumsum(np.diff(offs)[keep])]).astype(np.int32)

        def run(fe, ctx):
            return dict(best=fe.ComputeDistinctiveDescriptors(desc, offs, ctx=ctx))

        def want():
            return dict(best=np.asarray(hm.distinctive(desc, offs), np.int32))
        return run, want
    return make


def _sort(n):
    def make(big):
        import helper_models as hm
        import helper_scenes as hs
        k = hs.response_keypoints(synth.KP_DTYPE, 257 if big else n)

        def run(fe, ctx):
            return dict(perm=fe.sortFeaturesResponse(k, ctx))

        def want():
            return dict(perm=np.asarray(hm.sort_by_response(k["response"]), np.int32))
        return run, want
    return make


def _lk(n):
    def make(big):
        w, h = (BIG_W, BIG_H) if big else (W, H)
        img1 = image(21 + big, w, h)
        rng = np.random.default_rng(4)
        img2 = np.clip(np.roll(img1, (1, -2), axis=(0, 1)).astype(np.int32) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)
        img2[h // 2:h // 2 + 12, w // 2:w // 2 + 16] = 90                    # a flat block: the minEig test and lost tracks
        N = 3 * n if big else n
        pts = np.stack([rng.uniform(2, w - 2, N), rng.uniform(2, h - 2, N)], axis=1).astype(F32)
        pts[:4] = [[0.0, 0.0], [w - 0.1, h - 0.1], [-20.0, 10.0], [w + 30.0, 20.0]]

        def run(fe, ctx):
            nxt, st, er = fe.ELK_Tracker(9, 1, 10, 0.03, ctx=ctx).calcOpticalFlowPyrLK(img1, img2, pts, None, 0)
            return dict(next=nxt, status=st, err=er)

        def want():
            nxt, st, er = orc().calc_optical_flow_pyr_lk(img1, img2, pts, None, 9, 1, 10, 0.03, 0)
            return dict(next=nxt, status=st, err=er)
        return run, want
    return make


def _bow_transform(n):
    def make(big):
        voc = synth.random_vocabulary(7, 3, seed=8, ragged=True)
        rng = np.random.default_rng(17 + big)
        leaves = np.nonzero(voc["word_id"] >= 0)[0]
        N = 3 * n + 2 if big else n
        desc = voc["node_desc"][rng.choice(leaves, N)].copy()
        desc ^= np.packbits(rng.uniform(size=(N, 256)) < 0.08, axis=1)
        if N > 9:
            desc[:5] = rng.integers(0, 256, (5, 32), dtype=np.uint8)         # far from every node: ties and odd descents
            desc[5:9] = desc[5]                                             # one word several times

        def run(fe, ctx):
            bw, bv, fv, wo, no = fe.ORBVocabulary(voc, 0, 1, ctx=ctx).transform(desc, 1, return_assignments=True)
            return dict(bw=bw, bv=bv, fn=fv[0], fo=fv[1], fi=fv[2], wo=wo, no=no)

        def want():
            ow, ov, ofv, owo, ono = orc().bow_transform(voc, desc, 1, 0, 1)
            return dict(bw=ow, bv=np.asarray(ov, np.float64), fn=ofv[0], fo=ofv[1], fi=ofv[2], wo=owo, no=ono)
        return run, want
    return make


# ---- KeyFrameDatabase ----------------------------------------------------------------------------------------------------------------------
def _kfdb_data(big):
    K = 9 if big else 3
    return synth.bow_database(100 + big, K, vocab_words=700, words_per_kf=64, nplaces=3, nqueries=2, kf_words=([64, 40, 65] * 3)[:K], query_words=[65, 3])


def _kfdb(which, nbest, empty=False):
    """which "add": the slots and the stored scores after add; "detect": a query with the covisibility table.  empty: a query that shares
    no word with any keyframe -- the candidate list is empty"""
    def make(big):
        import kfdb_ref
        d = _kfdb_data(big)
        K = len(d["kfs"])
        q = d["queries"][0]
        if empty and not big:
            used = np.unique(np.concatenate([w for w, _ in d["kfs"]]))
            free = np.setdiff1d(np.arange(d["vocab_words"]), used)[:5].astype(np.uint32)
            q = dict(word=free, val=np.full(5, 0.2))
        covis = np.full((K, 10), -1, np.int32)
        for k in range(K):
            covis[k, :2] = [(k + 1) % K, (k + K - 1) % K]
        exclude = (np.arange(K) % 3 == 2).astype(np.uint8) if nbest else None

        def query(db):
            if nbest:
                return db.detect_nbest_candidates(q["word"], q["val"], exclude=exclude, covis=covis)
            return db.detect_relocalization_candidates(q["word"], q["val"], covis=covis)

        def pack(r, scores):
            r = dict(r); r.pop("stale", None)
            out = {k: np.asarray(v) for k, v in r.items() if isinstance(v, np.ndarray)}
            out.update(counts=np.array([r["n_listed"], r["n_scored"], r["max_common_words"]], np.int64), best_acc=np.asarray(r["best_acc"], F32),
                       scores=scores)
            return out

        def run(fe, ctx):
            db = fe.KeyFrameDatabase(ctx)
            db.clear()
            slots = db.add_many(d["kfs"])
            if which == "add":
                return dict(slots=np.asarray(slots, np.int32), s0=db.scores(0), s1=db.scores(1), info=np.asarray(db.info(), np.int64))
            return pack(query(db), np.stack([db.scores(0), db.scores(1)]))

        def want():
            db = kfdb_ref.KeyFrameDatabase(d["vocab_words"])
            slots = [db.add(w, v) for w, v in d["kfs"]]
            if which == "add":
                return dict(slots=np.asarray(slots, np.int32), s0=db.scores(0), s1=db.scores(1), info=np.array([K, K], np.int64))
            return pack(query(db), np.stack([db.scores(0), db.scores(1)]))
        return run, want
    return make


# ---------------------------------------------------------------------------------------------------------------------------------------
# the projections (tests/proj_ref) and the fused searches
PW, PH = 346, 260


def _view_kw(s, cam=None, mbf=0.0, mixed=False):
    kw = dict(R=s["R"], t=s["t"], Ow=s["Ow"], cam=cam or s["cam"], bounds=s["bounds"], nlevels=s["nlevels"], log_scale=s["log_scale"],
              scale_factors=s["scale_factors"], mbf=mbf)
    if mixed:
        ak, akl = synth.scale_tables(4, 1.4)
        kw.update(ak_nlevels=4, ak_log_scale=akl, ak_scale_factors=ak)
    return kw


def _right_kw(kw):
    Rrl = synth.rot(0.004, -0.02, 0.003).astype(np.float64)
    trl = np.array([-0.11, 0.002, 0.001])
    R = np.asarray(kw["R"], np.float64); t = np.asarray(kw["t"], np.float64)
    tlr = -Rrl.T @ trl
    r = dict(kw)
    r.update(R=(Rrl @ R).astype(F32), t=(Rrl @ t + trl).astype(F32), Ow=(R.T @ tlr + np.asarray(kw["Ow"], np.float64)).astype(F32))
    return r, np.concatenate([Rrl.reshape(-1), trl]).astype(F32)


def proj_ref_():
    import proj_ref
    proj_ref.use_oracle_camera(orc())
    return proj_ref


FR_FIELDS = ("in_view", "proj_xy", "proj_xr", "level", "view_cos", "depth", "level_scale", "reason")
LAST_FIELDS = ("valid", "uv", "proj_ur", "level_scale")
KF_FIELDS = ("valid", "uv", "level", "level_scale", "dist3d")
SIDE_FIELDS = ("valid", "uv", "radius", "level", "q_ur", "dist3d", "reason")


def _flat_dict(prefix, d):
    return {"%s%s" % (prefix, k): v for k, v in d.items()}


def _frustum(M, two):
    def make(big):
        m = 3 * M + 2 if big else M
        s = synth.map_scene(7 + big, m)
        kw = _view_kw(s, cam=(226.38, 226.15, 173.65, 133.73, -0.048, 0.011, -0.055, 0.021) if two else None, mbf=0.0 if two else 35.0)
        kws = [kw, _right_kw(kw)[0]] if two else [kw]
        skip = (np.arange(m) % 3 == 2).astype(np.uint8)
        args = (s["pos"], s["normal"], s["min_dist"], s["max_dist"])

        def pack(n, outs):
            d = dict(n=_i(n))
            for v, o in enumerate(outs):
                d.update(_flat_dict("v%d_" % v, _only(o, FR_FIELDS)))
            return d

        def run(fe, ctx):
            views = [fe.view(**k) for k in kws]
            n, got = fe.isInFrustum(views if two else views[0], *args, viewingCosLimit=0.5, skip=skip, ctx=ctx)
            return pack(n, got if two else [got])

        def want():
            ref = proj_ref_()
            n, outs = ref.frustum([ref.view(**k) for k in kws], *args, cos_limit=0.5, skip=skip)
            return pack(n, outs)
        return run, want
    return make


def _project_last(n):
    def make(big):
        m = 3 * n + 2 if big else n
        s = synth.map_scene(9 + big, m)
        kw = _view_kw(s, mbf=35.0)
        kps = synth.random_keypoints(m, PW, PH, nlevels=8, seed=5)
        skip = (np.arange(m) % 5 == 4).astype(np.uint8)

        def run(fe, ctx):
            return _only(fe.ProjectLastFrame(fe.view(**kw), s["pos"], kps, skip=skip, ctx=ctx), LAST_FIELDS)

        def want():
            ref = proj_ref_()
            return _only(ref.last_frame(ref.view(**kw), s["pos"], kps, skip=skip), LAST_FIELDS)
        return run, want
    return make


def _project_kf(n):
    def make(big):
        m = 3 * n + 2 if big else n
        s = synth.map_scene(10 + big, m)
        kw = _view_kw(s)
        skip = (np.arange(m) % 5 == 4).astype(np.uint8)

        def run(fe, ctx):
            return _only(fe.ProjectKeyFramePoints(fe.view(**kw), s["pos"], s["min_dist"], s["max_dist"], skip=skip, ctx=ctx), KF_FIELDS)

        def want():
            ref = proj_ref_()
            return _only(ref.keyframe_points(ref.view(**kw), s["pos"], s["min_dist"], s["max_dist"], skip=skip), KF_FIELDS)
        return run, want
    return make


def _slots(n, seed):
    rng = np.random.default_rng(seed)
    fm = np.full(n, -1, np.int32)
    fm[rng.random(n) < 0.08] = -2
    fm[rng.random(n) < 0.04] = -3
    return fm


def _local_points(M, n, empty=False):
    """empty: every point is skipped -- nothing in view, no candidate, the slots come back as they went in"""
    def make(big):
        proj_ref = proj_ref_()
        m, nk = (3 * M + 2, 3 * n + 2) if big else (M, n)
        s = synth.map_scene(11 + big, m)
        kw = _view_kw(s, mbf=35.0)
        args = (s["pos"], s["normal"], s["min_dist"], s["max_dist"])
        skip = np.ones(m, np.uint8) if empty and not big else (np.arange(m) % 11 == 10).astype(np.uint8)
        _, (r,) = proj_ref.frustum(proj_ref.view(**kw), *args, cos_limit=0.5, skip=(np.arange(m) % 11 == 10).astype(np.uint8))
        mp_desc = synth.random_descriptors(m, seed=12)
        kps, desc, _ = synth.planted_frame(r["in_view"], r["proj_xy"], r["level"], mp_desc, nk, PW, PH, seed=13)
        mp_obs = (np.random.default_rng(14).random(m) < 0.9).astype(np.uint8)
        fm = _slots(nk, 15)

        def run(fe, ctx):
            nm, gfm, nv, g = fe.SearchLocalPoints(fe.FrameView(kps, desc, PW, PH), fe.view(**kw), *args, mp_desc, mp_obs, fm, th=3.0, nnratio=0.8,
                                                  viewingCosLimit=0.5, skip=skip, ctx=ctx)
            return dict(nm=_i(nm), nv=_i(nv), fm=gfm, **_flat_dict("p_", _only(g, FR_FIELDS)))

        def want():
            ref = proj_ref_()
            wn, (p,) = ref.frustum(ref.view(**kw), *args, cos_limit=0.5, skip=skip)
            o = orc()
            on, ofm = o.search_by_projection_map(o.Frame(kps, desc, PW, PH), p["search"], p["proj_xy"], p["level"], p["view_cos"], mp_desc, mp_obs, fm, 3.0,
                                                 0.8, p["level_scale"])
            return dict(nm=_i(on), nv=_i(wn), fm=np.asarray(ofm, np.int32), **_flat_dict("p_", _only(p, FR_FIELDS)))
        return run, want
    return make


KB8_MVSEC = (226.38018519795807, 226.15002947047415, 173.6470807871759, 133.73271487507847,
             -0.048031442223833355, 0.011330957517194437, -0.055378166304281135, 0.021500973881459395)


def _local_points_fisheye(M, nL, nR):
    def make(big):
        proj_ref = proj_ref_()
        m, a, b = (3 * M + 2, 3 * nL + 1, 3 * nR + 1) if big else (M, nL, nR)
        s = synth.map_scene(16 + big, m)
        kwl = _view_kw(s, cam=KB8_MVSEC)
        kwr, _ = _right_kw(kwl)
        args = (s["pos"], s["normal"], s["min_dist"], s["max_dist"])
        skip = (np.arange(m) % 11 == 10).astype(np.uint8)
        _, (l, r) = proj_ref.frustum([proj_ref.view(**kwl), proj_ref.view(**kwr)], *args, cos_limit=0.5, skip=skip)
        mp_desc = synth.random_descriptors(m, seed=17)
        kl, dl, _ = synth.planted_frame(l["in_view"], l["proj_xy"], l["level"], mp_desc, a, PW, PH, seed=18)
        kr, dr, _ = synth.planted_frame(r["in_view"], r["proj_xy"], r["level"], mp_desc, b, PW, PH, seed=19)
        rng = np.random.default_rng(20)
        l2r = np.full(a, -1, np.int32); r2l = np.full(b, -1, np.int32)
        ia = rng.choice(a, min(a, b) // 4, replace=False); ib = rng.choice(b, min(a, b) // 4, replace=False)
        l2r[ia] = ib; r2l[ib] = ia
        mp_obs = (rng.random(m) < 0.9).astype(np.uint8)
        kps, desc, fm = np.concatenate([kl, kr]), np.concatenate([dl, dr]), _slots(a + b, 21)

        def run(fe, ctx):
            nm, gfm, nv, got = fe.SearchLocalPointsFisheye(kps, a, desc, l2r, r2l, fe.grid_bounds(PW, PH), [fe.view(**kwl), fe.view(**kwr)], *args, mp_desc,
                                                           mp_obs, fm, th=3.0, nnratio=0.8, viewingCosLimit=0.5, skip=skip, ctx=ctx)
            return dict(nm=_i(nm), nv=_i(nv), fm=gfm, **_flat_dict("l_", _only(got[0], FR_FIELDS)), **_flat_dict("r_", _only(got[1], FR_FIELDS)))

        def want():
            ref = proj_ref_()
            wn, w = ref.frustum([ref.view(**kwl), ref.view(**kwr)], *args, cos_limit=0.5, skip=skip)
            o = orc()
            cams = [(q["search"], q["proj_xy"], q["level"], q["view_cos"], q["level_scale"]) for q in w]
            on, ofm = o.search_by_projection_map_fisheye(kps, a, desc, o.grid_bounds(PW, PH), l2r, r2l, cams[0], cams[1], mp_desc, mp_obs, fm, 3.0, 0.8)
            return dict(nm=_i(on), nv=_i(wn), fm=np.asarray(ofm, np.int32), **_flat_dict("l_", _only(w[0], FR_FIELDS)), **_flat_dict("r_", _only(w[1], FR_FIELDS)))
        return run, want
    return make


def _last_pose(M, n):
    def make(big):
        proj_ref = proj_ref_()
        m, nk = (3 * M + 2, 3 * n + 2) if big else (M, n)
        s = synth.map_scene(22 + big, m)
        kw = _view_kw(s, mbf=35.0)
        last_kps = synth.random_keypoints(m, PW, PH, nlevels=8, seed=23)
        skip = (np.arange(m) % 7 == 6).astype(np.uint8)
        r = proj_ref.last_frame(proj_ref.view(**kw), s["pos"], last_kps, skip=skip)
        mp_desc = synth.random_descriptors(m, seed=24)
        kps, desc, _ = synth.planted_frame(r["valid"], r["uv"], last_kps["octave"], mp_desc, nk, PW, PH, seed=25, dlevel=(-1, 0, 1))
        mp_obs = (np.random.default_rng(26).random(m) < 0.9).astype(np.uint8)
        cm = _slots(nk, 27)
        none = np.zeros((m, 32), np.uint8)

        def run(fe, ctx):
            nm, gcm, valid, uv = fe.SearchByProjectionLastPose(fe.FrameView(kps, desc, PW, PH), fe.view(**kw), fe.FrameView(last_kps, none, PW, PH), s["pos"],
                                                               mp_desc, mp_obs, cm, 15.0, mode=0, checkOri=True, skip=skip, ctx=ctx)
            return dict(nm=_i(nm), cm=gcm, valid=valid, uv=uv)

        def want():
            ref = proj_ref_()
            p = ref.last_frame(ref.view(**kw), s["pos"], last_kps, skip=skip)
            o = orc()
            on, ocm = o.search_by_projection_last(o.Frame(kps, desc, PW, PH), o.Frame(last_kps, none, PW, PH), p["valid"], p["uv"], mp_desc, mp_obs, cm, 15.0,
                                                  p["level_scale"], mode=0, checkOri=True)
            return dict(nm=_i(on), cm=np.asarray(ocm, np.int32), valid=p["valid"], uv=p["uv"])
        return run, want
    return make


def _kf_pose(M, n):
    def make(big):
        proj_ref = proj_ref_()
        m, nk = (3 * M + 2, 3 * n + 2) if big else (M, n)
        s = synth.map_scene(28 + big, m)
        kw = _view_kw(s)
        kf_kps = synth.random_keypoints(m, PW, PH, nlevels=8, seed=29)
        skip = (np.arange(m) % 7 == 6).astype(np.uint8)
        r = proj_ref.keyframe_points(proj_ref.view(**kw), s["pos"], s["min_dist"], s["max_dist"], skip=skip)
        mp_desc = synth.random_descriptors(m, seed=30)
        kps, desc, _ = synth.planted_frame(r["valid"], r["uv"], r["level"], mp_desc, nk, PW, PH, seed=31, dlevel=(-1, 0, 1))
        cm = np.full(nk, -1, np.int32)
        cm[np.random.default_rng(32).random(nk) < 0.1] = 5

        def run(fe, ctx):
            nm, gcm, valid, uv, level = fe.SearchByProjectionKFPose(fe.FrameView(kps, desc, PW, PH), fe.view(**kw), kf_kps, s["pos"], s["min_dist"],
                                                                    s["max_dist"], mp_desc, cm, 30.0, 100, checkOri=True, skip=skip, ctx=ctx)
            return dict(nm=_i(nm), cm=gcm, valid=valid, uv=uv, level=level)

        def want():
            ref = proj_ref_()
            p = ref.keyframe_points(ref.view(**kw), s["pos"], s["min_dist"], s["max_dist"], skip=skip)
            o = orc()
            on, ocm = o.search_by_projection_kf(o.Frame(kps, desc, PW, PH), kf_kps, None, p["valid"], p["uv"], p["level"], p["level_scale"], mp_desc, cm, 30.0,
                                                100, True)
            return dict(nm=_i(on), cm=np.asarray(ocm, np.int32), valid=p["valid"], uv=p["uv"], level=p["level"])
        return run, want
    return make


# ---- the KeyFrame-side matchers ------------------------------------------------------------------------------------------------------------
def kfside_ref_():
    import kfside_ref
    kfside_ref.use_oracle_camera(orc())
    return kfside_ref


def mref_():
    import kfside_mixed_ref as mref
    mref.use_oracle(orc())
    return mref


def _geom(sc):
    return sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"]


def _nbh(big, K, M, n_kps, mixed, seed=43):
    m = 3 * M + 2 if big else M
    nk = [3 * n + (2 if n else 0) for n in n_kps] if big else list(n_kps)
    f = synth.mixed_keyframe_neighbourhood if mixed else synth.keyframe_neighbourhood
    return f(seed + big, K, m, n_kps=nk)


def _kf_radius(form):
    """the forms of tests/kfside_model.py: plain, the stereo gate (eorb_kf_radius_match_stereo), in order, mixed"""
    def make(big):
        import kfside_model as km
        sc = km.scene()
        if big:                                                             # the scene three times over: keypoints and queries alike
            sc = {k: (v if k == "names" else np.ascontiguousarray(np.concatenate([v] * 3))) for k, v in sc.items()}

        def pack(r):
            return dict(zip(("bi", "bd", "taken"), [np.asarray(a) for a in r]))

        def run(fe, ctx):
            return pack(km.run_kernels(fe, ctx, sc, form))

        def want():
            return pack(km.run_model(sc, form))
        return run, want
    return make


def _side_projection(M, mixed):
    def make(big):
        m = 3 * M + 2 if big else M
        s = synth.map_scene(41 + big, m)
        kw = dict(R=s["R"], t=s["t"], Ow=s["Ow"], cam=s["cam"], bounds=s["bounds"], nlevels=s["nlevels"], log_scale=s["log_scale"],
                  scale_factors=s["scale_factors"], mbf=35.0)
        mio = None
        if mixed:
            ak_sf, ak_log = synth.akaze_tables()
            kw.update(ak_nlevels=len(ak_sf), ak_log_scale=ak_log, ak_scale_factors=ak_sf)
            mio = (np.random.default_rng(7).random(m) >= 1 / 3).astype(np.uint8)
        skip = (np.arange(m) % 3 == 2).astype(np.uint8)

        def run(fe, ctx):
            if mixed:
                return _only(fe.ProjectKeyFrameSideMixed(fe.view(**kw), *_geom(s), 3.0, mp_is_orb=mio, skip=skip, ctx=ctx), SIDE_FIELDS)
            return _only(fe.ProjectKeyFrameSide(fe.view(**kw), *_geom(s), 3.0, skip=skip, ctx=ctx), SIDE_FIELDS)

        def want():
            if mixed:
                ref = mref_()
                return _only(ref.keyframe_side(ref.view(**kw), *_geom(s), 3.0, mp_is_orb=mio, skip=skip), SIDE_FIELDS)
            ref = kfside_ref_()
            return _only(ref.keyframe_side(ref.view(**kw), *_geom(s), 3.0, skip=skip), SIDE_FIELDS)
        return run, want
    return make


def _mixed_kw(sc, k, gate):
    kw = dict(kp_is_orb=sc["kp_is_orb"][k], mp_is_orb=sc["mp_is_orb"])
    if gate != "none":
        kw["kp_inv_sigma2"] = sc["kp_inv_sigma2"][k]
    if gate == "stereo":
        kw["uright"] = sc["uright"][k]
    return kw


def _side_search(sc, k, p, gate, mixed, taken=None, accept_thr=0.0):
    """the reference's radius search of the projection p (rows of keyframe k) in keyframe k"""
    M = len(p["valid"])
    if len(sc["kps"][k]) == 0:
        return np.full(M, -1, np.int32), np.full(M, 256, np.int32)
    o = orc()
    fr = o.Frame(sc["kps"][k], sc["desc"][k], PW, PH)
    extra = {} if taken is None else dict(taken=taken, accept_thr=accept_thr)
    if mixed:
        return mref_().search(fr, p, sc["mp_desc"], **_mixed_kw(sc, k, gate), **extra)
    kw = dict(inv_sigma2=None if gate == "none" else sc["inv_sigma2"])
    if gate == "stereo":
        kw.update(uright=sc["uright"][k], q_ur=p["q_ur"])
    return o.kf_radius_match(fr, p["valid"], p["uv"], p["radius"], p["level"], sc["mp_desc"], **kw, **extra)


def _side_proj(sc, th, mixed, skip=None):
    if mixed:
        ref = mref_()
        return ref.keyframe_side([ref.view(**v) for v in sc["views"]], *_geom(sc), th, mp_is_orb=sc["mp_is_orb"], skip=skip)
    ref = kfside_ref_()
    return ref.keyframe_side([ref.view(**v) for v in sc["views"]], *_geom(sc), th, skip=skip)


def _fuse_pose(M, n, gate, mixed):
    def make(big):
        sc = _nbh(big, 1, M, (n,), mixed)

        def run(fe, ctx):
            gb, v = fe.grid_bounds(PW, PH), fe.view(**sc["views"][0])
            if mixed:
                bi, bd, g = fe.FusePoseMixed(sc["kps"][0], sc["desc"][0], gb, v, *_geom(sc), sc["mp_desc"], th=3.0, want_projection=True, ctx=ctx,
                                             **_mixed_kw(sc, 0, gate))
            else:
                bi, bd, g = fe.FusePose(sc["kps"][0], sc["desc"][0], gb, v, *_geom(sc), sc["mp_desc"], inv_sigma2=None if gate == "none" else sc["inv_sigma2"],
                                        th=3.0, uright=sc["uright"][0] if gate == "stereo" else None, want_projection=True, ctx=ctx)
            return dict(bi=bi, bd=bd, **_flat_dict("p_", _only(g, SIDE_FIELDS)))

        def want():
            p = _side_proj(sc, 3.0, mixed)
            bi, bd = _side_search(sc, 0, p, gate, mixed)[:2]
            return dict(bi=np.asarray(bi, np.int32), bd=np.asarray(bd, np.int32), **_flat_dict("p_", _only(p, SIDE_FIELDS)))
        return run, want
    return make


def _kf_scw(M, n, mixed):
    def make(big):
        sc = _nbh(big, 1, M, (n,), mixed, seed=45)
        nk, m = len(sc["kps"][0]), len(sc["min_dist"])
        taken = (np.random.default_rng(3).random(nk) < 0.2).astype(np.uint8)
        skip = (np.arange(m) % 13 == 12).astype(np.uint8)

        def run(fe, ctx):
            gb, v = fe.grid_bounds(PW, PH), fe.view(**sc["views"][0])
            if mixed:
                bi, bd, tk, g = fe.SearchByProjectionKFScwMixed(sc["kps"][0], sc["desc"][0], gb, v, *_geom(sc), sc["mp_desc"], taken, 4.0, ratioHamming=1.0,
                                                                skip=skip, want_projection=True, ctx=ctx, kp_is_orb=sc["kp_is_orb"][0], mp_is_orb=sc["mp_is_orb"])
            else:
                bi, bd, tk, g = fe.SearchByProjectionKFScw(sc["kps"][0], sc["desc"][0], gb, v, *_geom(sc), sc["mp_desc"], taken, 4.0, ratioHamming=1.0,
                                                           skip=skip, want_projection=True, ctx=ctx)
            return dict(bi=bi, bd=bd, taken=tk, **_flat_dict("p_", _only(g, SIDE_FIELDS)))

        def want():
            p = _side_proj(sc, 4.0, mixed, skip=skip)
            bi, bd, tk = _side_search(sc, 0, p, "none", mixed, taken=taken, accept_thr=50.0)
            return dict(bi=np.asarray(bi, np.int32), bd=np.asarray(bd, np.int32), taken=np.asarray(tk, np.uint8), **_flat_dict("p_", _only(p, SIDE_FIELDS)))
        return run, want
    return make


def _fuse_keyframes(M, n_kps, gate, mixed):
    """K = 3 with an empty keyframe in the middle"""
    def make(big):
        sc = _nbh(big, 3, M, n_kps, mixed, seed=49)
        K, m = 3, len(sc["min_dist"])
        skip = (np.random.default_rng(5).random((K, m)) < 0.1).astype(np.uint8)
        off = np.concatenate([[0], np.cumsum([len(k) for k in sc["kps"]])]).astype(np.int32)
        kps, desc, ur = np.concatenate(sc["kps"]), np.concatenate(sc["desc"]), np.concatenate(sc["uright"])

        def run(fe, ctx):
            gb, views = fe.grid_bounds(PW, PH), [fe.view(**kw) for kw in sc["views"]]
            if mixed:
                bi, bd, rs = fe.FuseKeyFramesMixed(views, [gb] * K, kps, desc, off, *_geom(sc), sc["mp_desc"], kp_is_orb=np.concatenate(sc["kp_is_orb"]),
                                                   kp_inv_sigma2=None if gate == "none" else np.concatenate(sc["kp_inv_sigma2"]), mp_is_orb=sc["mp_is_orb"],
                                                   th=3.0, skip=skip, uright=ur if gate == "stereo" else None, want_reason=True, ctx=ctx)
            else:
                bi, bd, rs = fe.FuseKeyFrames(views, [gb] * K, kps, desc, off, *_geom(sc), sc["mp_desc"], inv_sigma2=None if gate == "none" else sc["inv_sigma2"],
                                              th=3.0, skip=skip, uright=ur if gate == "stereo" else None, want_reason=True, ctx=ctx)
            return dict(bi=np.asarray(bi).reshape(-1), bd=np.asarray(bd).reshape(-1), reason=np.asarray(rs).reshape(-1))

        def want():
            p = _side_proj(sc, 3.0, mixed, skip=skip.reshape(-1))
            bi, bd = [], []
            for k in range(K):
                pk = {a: p[a][k * m:(k + 1) * m] for a in p}
                a, b = _side_search(sc, k, pk, gate, mixed)[:2]
                bi.append(a); bd.append(b)
            return dict(bi=np.concatenate(bi).astype(np.int32), bd=np.concatenate(bd).astype(np.int32), reason=np.asarray(p["reason"]).reshape(-1))
        return run, want
    return make


def _search_by_sim3(n):
    def make(big):
        import kfside_model as km
        k = 3 if big else 1
        sp = synth.sim3_pair(47 + big, n=k * n, n_both=k * (n // 4), n_one=k * (n // 8), n_cross=k * (n // 8))

        def run(fe, ctx):
            gb = fe.grid_bounds(sp["W"], sp["H"])
            kf = [dict(q, gb=gb, view=fe.view(**q["view"])) for q in (sp["kf1"], sp["kf2"])]
            nf, m12, v1, v2 = fe.SearchBySim3Pose(kf[0], kf[1], sp["sR12"], sp["t12"], sp["sR21"], sp["t21"], th=7.5, ctx=ctx)
            return dict(nf=_i(nf), m12=m12, v1=v1, v2=v2)

        def want():
            p12, p21 = km.sim3_projections(kfside_ref_(), sp)
            nf, m12, v1, v2 = km.sim3_agree(*km.sim3_searches(sp, p12, p21), 100)
            return dict(nf=_i(nf), m12=np.asarray(m12, np.int32), v1=np.asarray(v1, np.int32), v2=np.asarray(v2, np.int32))
        return run, want
    return make


# ---------------------------------------------------------------------------------------------------------------------------------------
# the RANSAC solvers, CreateNewMapPoints, the two-view reconstruction
S3_KEYS = ("it_scale", "it_T12", "it_T21", "it_inliers", "converged", "best_it", "n_inliers", "iterations_used", "s12", "R12", "t12", "T12", "inliers")


def _k_results(out, keys):
    return {"%d_%s" % (k, name): np.asarray(r[name]) for k, r in enumerate(out) for name in keys}


def _sim3(short_middle):
    def make(big):
        import sim3_ref as s3
        from sim3_ref import scenes
        if big:
            pbs = [scenes.scene(195, seed=171, pair="kp", iters=65), scenes.scene(190, seed=172, pair="pp", iters=33), scenes.scene(189, seed=173, pair="kk", iters=9)]
        elif short_middle:
            short = scenes.two_groups(3, 3, 7, "AB")                       # N = 6 < min_inliers = 7
            short["sets"] = short["sets"][:1]
            pbs = [scenes.scene(65, seed=71, pair="pk", iters=65), short, scenes.scene(63, seed=72, pair="kp", wrong=1.0, fix_scale=True, iters=1)]
        else:
            pbs = [scenes.edge_problems()["three_points"], scenes.scene(65, seed=31, pair="kk", wrong=1.0, iters=3)]

        def solve(mod, **kw):
            solvers = [scenes.solver(mod, pb, **kw) for pb in pbs]
            return _k_results(mod.Sim3Solver.solve_candidates(solvers, [pb["sets"] for pb in pbs], aids=True, **kw), S3_KEYS)

        def run(fe, ctx):
            return solve(fe, ctx=ctx)

        def want():
            return solve(s3)
        return run, want
    return make


def _mlpnp(short_middle):
    def make(big):
        import mlpnp_ref as mr
        from mlpnp_ref import scenes
        keys = ("it_Rt", "it_inliers", "it_refine_inliers") + scenes.RULE_KEYS + ("Tcw", "inliers")
        if big:
            pbs = [scenes.scene(195, seed=171, cam="p", iters=33), scenes.scene(190, seed=172, cam="k", iters=17), scenes.scene(189, seed=173, cam="k", iters=9)]
        elif short_middle:
            pbs = [scenes.scene(65, seed=71, cam="k", iters=17), scenes.scene(8, seed=72, cam="p", iters=1, min_inliers=10),
                   scenes.scene(63, seed=73, cam="p", wrong=1.0, planar=True, iters=1)]
        else:
            pbs = [scenes.scene(7, seed=31, cam="p", wrong=0.0, iters=3, min_inliers=6), scenes.scene(65, seed=32, cam="k", wrong=1.0, iters=3)]

        def solve(mod, **kw):
            solvers = [scenes.solver(mod, pb, **kw) for pb in pbs]
            return _k_results(mod.MLPnPsolver.solve_candidates(solvers, [pb["sets"] for pb in pbs], aids=True, **kw), keys)

        def run(fe, ctx):
            return solve(fe, ctx=ctx)

        def want():
            return solve(mr)
        return run, want
    return make


NP_KEYS = ("status", "x3d", "branch", "cos_parallax", "n_new")


def no_parallax_middle(sc):
    """the scene with keyframe 1 moved onto pKF1: every ray pair of its matches is parallel, so every one of them fails the parallax test"""
    o = dict(sc)
    n1 = int(sc["kf_off"][1] - sc["kf_off"][0]); n2 = int(sc["kf_off"][2] - sc["kf_off"][1])
    n = min(n2, len(sc["kps1"]))
    kps2 = sc["kps2"].copy()
    kps2[n1:n1 + n] = sc["kps1"][:n]
    m = sc["match12"].copy()
    m[1] = -1
    m[1, :n] = np.arange(n)
    v2 = list(sc["views2"])
    v2[1] = sc["views1"]
    o.update(kps2=kps2, match12=m, views2=v2, name=sc["name"] + "_no_parallax")
    return o


def _newpts(kind):
    def make(big):
        import newpts_ref as nr
        from newpts_ref import scenes
        if big:
            sc = scenes.random_scene("big", 17, K=3, n1=197, n2=191, stereo=kind == "stereo")
        elif kind == "twocam":
            sc = scenes.twocam_scene("twocam", 5, K=3, nl=38, nr=27)
        else:
            sc = no_parallax_middle(scenes.random_scene(kind, 1, K=3, n1=65, n2=63, stereo=kind == "stereo", far=15.0))

        def run(fe, ctx):
            v1, v2 = nr.views(sc)
            out = fe.NewMapPoints(sc["kps1"], sc["kps2"], sc["kf_off"], sc["match12"], v1, v2, ctx=ctx, **nr.params(sc))
            return {k: np.asarray(out[k]) for k in NP_KEYS}

        def want():
            out = nr.loop(sc)
            return {k: np.asarray(out[k]) for k in NP_KEYS}
        return run, want
    return make


def _create_newpts(kind):
    """the fused call on a small neighbourhood whose middle keyframe shares no node with pKF1: its row of the search is empty, and so is
    its row of the stage"""
    def make(big):
        import kfbatch_cases as kc
        import newpts_ref as nr
        from newpts_ref import scenes
        K = 3
        s = kc.tri_scene(kind, 4 if kind.startswith("pinhole") else 3) if big else _small_tri(kind)
        ks = [0, 1, 2]
        kfs = kc.tri_set(s, ks)
        if not big:
            kfs[1] = _no_common_node(kfs[1])
        scale, sigma2 = synth.level_tables()
        I, z = np.eye(3, dtype=F32), np.zeros(3, F32)
        cam = synth.CAM_MONO[:4] if kind.startswith("pinhole") else synth.CAM_MONO
        views1 = [scenes.make_view(I, z, cam)]
        views2 = [[scenes.make_view(*synth.neighbour_pose(k), cam)] for k in ks]
        kw = dict(level_scale=scale, level_sigma2=sigma2, ratio_factor_orb=F32(1.5) * scale[1], ratio_factor_ak=F32(1.5) * scale[1])

        def search_args():
            if "F12" in s:
                return (s["kps1"], s["desc1"], s["elig1"], s["fv1"], kfs, s["ep"][ks], s["F12"][ks], s["scale2"], s["sigma2_2"])
            return (s["kps1"], s["nleft1"], s["desc1"], s["elig1"], s["fv1"], kfs, [s["kfs"][k]["nleft"] for k in ks], s["cams1"], s["cams2"], s["Rt"][ks],
                    s["ep"][ks], s["scale2"], s["sigma2_1"], s["sigma2_2"])

        def run(fe, ctx):
            v1, v2 = nr.views(dict(views1=views1, views2=views2, level_scale=scale))
            f = fe.CreateNewMapPoints if "F12" in s else fe.CreateNewMapPointsKB8
            nm, m, out = f(*search_args(), v1, v2, False, False, ctx=ctx, **kw)
            return dict(nm=np.asarray(nm, np.int32), m=np.asarray(m, np.int32), **{k: np.asarray(out[k]) for k in NP_KEYS})

        def want():
            o = orc()
            nm, rows = [], []
            for i, k in enumerate(ks):
                kp2, d2, e2, fv2 = kfs[i]
                if "F12" in s:
                    n, m = o.search_for_triangulation(s["kps1"], s["desc1"], s["elig1"], s["fv1"], kp2, d2, e2, fv2, s["ep"][k], s["F12"][k], s["scale2"],
                                                      s["sigma2_2"], False, False)
                else:
                    n, m = o.search_for_triangulation_kb8(s["kps1"], s["nleft1"], s["desc1"], s["elig1"], s["fv1"], kp2, s["kfs"][k]["nleft"], d2, e2, fv2,
                                                          s["cams1"], s["cams2"], s["Rt"][k], s["ep"][k], s["scale2"], s["sigma2_1"], s["sigma2_2"], False, False)
                nm.append(n); rows.append(m)
            m = np.stack(rows).astype(np.int32)
            sub = dict(s, kfs=[s["kfs"][k] for k in ks])
            ref = nr.loop(scenes.scene_of_search(sub, views1, views2, scale, sigma2, m, "pinhole" if "F12" in s else "kb8"))
            return dict(nm=np.asarray(nm, np.int32), m=m, **{k: np.asarray(ref[k]) for k in NP_KEYS})
        return run, want
    return make


TV_RANSAC = ("it_H", "it_F", "it_score_h", "it_score_f", "best_it_h", "best_it_f", "SH", "SF", "H21", "F21", "inliers_h", "inliers_f")
TV_RT = ("n_good", "cos_all", "cos_sel", "good", "p3d")


def _tv_scene(big, kind, N, seed):
    from twoview_ref import reconstruct_scenes as rs
    from twoview_ref import scenes
    n = 3 * N + 2 if big else N
    if kind == "same_keys":
        return rs.same_keys(n, seed=seed), n
    if kind in ("planar", "general"):
        return rs.moved(kind, n, seed=seed + big, normal=(0.6, -0.15, 1.0)), n
    return scenes.scene(kind, n, seed=seed + big), n


def _tv_ransac(kind, N, iters):
    def make(big):
        import twoview_ref as tv
        from twoview_ref import scenes
        sc, n = _tv_scene(big, kind, N, 11)
        sets = scenes.make_sets(n, 3 * iters if big else iters, seed=12)

        def find(T):
            r = T.find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], sets, aids=True)
            return {k: np.asarray(r[k]) for k in TV_RANSAC}

        def run(fe, ctx):
            return find(fe.TwoViewReconstruction(scenes.K, ctx=ctx))

        def want():
            return find(tv.TwoViewReconstruction(scenes.K))
        return run, want
    return make


def _tv_check_rt(N, Kp, no_inliers):
    def make(big):
        import twoview_ref as tv
        from twoview_ref import scenes
        n = 3 * N + 2 if big else N
        sc = scenes.scene("mixed", n, seed=100 + n, noise=0.5, far=0.35)
        four = scenes.decompose_e_poses(sc["R"], sc["t"])
        poses = scenes.poses27(four if Kp == 4 or big else [(sc["R"], sc["t"])])
        inl = (np.random.default_rng(n).random(n) < 0.8).astype(np.uint8)
        if no_inliers and not big:
            inl[:] = 0

        def check(T):
            r = T.check_rt(sc["kps1"], sc["kps2"], sc["matches"], inl, poses, want_cos_all=True)
            return {k: np.asarray(r[k]) for k in TV_RT}

        def run(fe, ctx):
            return check(fe.TwoViewReconstruction(scenes.K, ctx=ctx))

        def want():
            return check(tv.TwoViewReconstruction(scenes.K))
        return run, want
    return make


def _tv_reconstruct(kind, N, iters, form, seed=3, sets_seed=2, **over):
    def make(big):
        from twoview_ref import reconstruct_ref as rr
        from twoview_ref import scenes
        sc, n = _tv_scene(big, "general" if big else kind, N, 3 if big else seed)
        sets = scenes.make_sets(n, 3 * iters if big else iters, seed=sets_seed)
        par = rr.params(rr.FORM_INFO if form else rr.FORM_STOCK, **over)
        keys = sorted(set(rr.RESULT_FIELDS) | {"hyp_poses", "R21", "t21", "triangulated", "p3d", "trans_inliers"})

        def run(fe, ctx):
            dp = _lib.TvrReconParams(*[getattr(par, f[0]) for f in par._fields_])
            r = fe.TwoViewReconstruction(scenes.K, sigma=par.sigma, ctx=ctx).reconstruct(sc["kps1"], sc["kps2"], sc["matches"], sets, params=dp, want_poses=True)
            return {k: np.asarray(r[k]) for k in keys}

        def want():
            r = rr.reconstruct(scenes.K, sc["kps1"], sc["kps2"], sc["matches"], sets, par)
            return {k: np.asarray(r[k]) for k in keys}
        return run, want
    return make


# ---------------------------------------------------------------------------------------------------------------------------------------
def _cases():
    T = {}
    right_shift = lambda left: np.ascontiguousarray(np.roll(left, -3, axis=1))        # noqa: E731
    # ---- events
    T["eorb_ev2im_gauss"] = [Case("2003 events", _gauss(2003, False)), Case("no event", _gauss(0, False)), Case("polarity, 65 events", _gauss(65, True))]
    T["eorb_ev2im"] = [Case("2003 events", _gauss(2003, False, count=True)), Case("no event: max == min, no u8 image", _gauss(0, False, count=True))]
    T["eorb_ev2im_gauss_raw"] = [Case("2003 raw events", _gauss_raw(2003, False)), Case("no event", _gauss_raw(0, False))]
    T["eorb_ev2im_raw"] = [Case("2003 raw events", _gauss_raw(2003, True, count=True))]
    T["eorb_undistort_events"] = [Case("2003 raw events", _undistort_events(2003, 0.0)), Case("none kept", _undistort_events(65, -100.0))]
    T["eorb_parse_events_text"] = [Case("65 lines", _parse(65)), Case("3 lines", _parse(3))]
    T["eorb_ev2mci_se3_cam"] = [Case("2003 events, KannalaBrandt8", _mci(2003, "se3", KB8, False)), Case("65 events, polarity", _mci(65, "se3", CAM, True))]
    T["eorb_ev2mci_se2_cam"] = [Case("2003 events", _mci(2003, "se2", KB8, False))]
    T["eorb_ev2mci_se3"] = [Case("2003 events", _mci(2003, "se3", CAM, False, export=True))]
    T["eorb_ev2mci_se2"] = [Case("65 events", _mci(65, "se2", CAM, True, export=True))]
    T["eorb_measure_image_focus_n"] = [Case("3 images, the middle one flat", _focus(3))]
    T["eorb_measure_image_focus"] = [Case("one image", _focus(1, single=True))]
    T["eorb_normalize_minmax_u8"] = [Case("ramp", _normalize(False)), Case("flat image: max == min", _normalize(True))]
    # ---- calibrator
    T["eorb_undistort_keypoints"] = [Case("65 keypoints", _undist(65, False)), Case("3 keypoints", _undist(3, False))]
    T["eorb_undistort_points"] = [Case("65 points", _undist(65, True))]
    T["eorb_generate_undistort_maps"] = [Case("70 x 50 maps", _gen_maps())]
    # ---- extractor
    T["eorb_orb_extract"] = [Case("texture", _extract(lambda: image(3))), Case("no corner at all", _extract(flat)),
                             Case("half of the cells without a corner, a lapping area", _extract(lambda: half_flat(4), (10, 40)))]
    T["eorb_frame_mono"] = [Case("texture", _frame_mono(lambda: image(5))), Case("no corner", _frame_mono(flat))]
    T["eorb_frame_stereo"] = [Case("a pair with disparities up to 6", _stereo(lambda left, right: right)),
                              Case("no stereo match: a flat right image", _stereo(lambda left, right: flat())),
                              Case("no keypoint on either side", _stereo_flat_both())]
    T["eorb_frame_fisheye"] = [Case("shifted pair", _fisheye(right_shift, ((0, W), (0, W)))),
                               Case("no keypoint in the lapping areas", _fisheye(right_shift, ((0, 0), (0, 0)))),
                               Case("flat right image", _fisheye(lambda left: flat(), ((0, W), (0, W))))]
    T["eorb_orb_tracked_descriptors"] = [Case("tracked keypoints, some outside the levels", _tracked(False))]
    T["eorb_orb_assign_level_by_best_desc"] = [Case("tracked keypoints", _tracked(True))]
    T["eorb_ev_slice_extract"] = [Case("2003 events", _slice("extract")), Case("65 events: hardly a corner", _slice("extract", 65))]
    T["eorb_ev_slice_image"] = [Case("the image of the last slice", _slice("image"))]
    T["eorb_ev_slice_track"] = [Case("the next chunk", _slice("track"))]
    T["eorb_ev_mc_contest"] = [Case("every method", _contest(2003, "all")), Case("the event histogram alone", _contest(2003, "none"))]
    # ---- window matchers
    T["eorb_search_for_initialization"] = [Case("planted scene, mixed", _window("init", "mixed")), Case("no candidate", _window("init", "plain", empty=True))]
    T["eorb_search_by_projection_last"] = [Case("planted scene, mixed", _window("last", "mixed")), Case("no valid query", _window("last", "plain", empty=True))]
    T["eorb_search_by_projection_last_stereo"] = [Case("planted scene", _window("last", "stereo"))]
    T["eorb_search_by_projection_kf"] = [Case("planted scene, mixed", _window("kf", "mixed")), Case("no valid query", _window("kf", "plain", empty=True))]
    T["eorb_search_by_projection_map"] = [Case("planted scene, mixed", _window("map", "mixed")), Case("nothing in view", _window("map", "plain", empty=True))]
    T["eorb_search_by_projection_map_stereo"] = [Case("planted scene", _window("map", "stereo"))]
    T["eorb_search_by_projection_map_fisheye"] = [Case("planted scene", _twocam("map", "base")), Case("no query", _twocam("map", "base: no query"))]
    T["eorb_search_by_projection_last_fisheye"] = [Case("planted scene", _twocam("last", "base")), Case("no query", _twocam("last", "base: no query"))]
    T["eorb_search_by_bow_fisheye"] = [Case("planted scene", _twocam("bow", "base")), Case("no KeyFrame feature holds a map point", _twocam("bow", "bow: no query"))]
    # ---- node walks
    T["eorb_search_by_bow"] = [Case("planted nodes", _node_single("bow"))]
    T["eorb_search_by_bow_kf"] = [Case("planted nodes", _node_single("bowkf"))]
    T["eorb_search_for_triangulation"] = [Case("planted nodes", _node_single("tri")), Case("no node in common: zero candidates", _tri_single_no_candidate())]
    T["eorb_search_for_triangulation_kb8"] = [Case("63 points", _tri_kb8_single())]
    T["eorb_search_for_triangulation_keyframes"] = [Case("K = 3, no node in common in the middle", _tri_batch("pinhole", "no_node")),
                                                    Case("K = 3, an empty keyframe in the middle", _tri_batch("pinhole", "empty"))]
    T["eorb_search_for_triangulation_kb8_keyframes"] = [Case("K = 3, no node in common in the middle", _tri_batch("kb8", "no_node"))]
    T["eorb_search_by_bow_keyframes"] = [Case("K = 3, no node in common in the middle", _bow_batch(False))]
    T["eorb_search_by_bow_kf_keyframes"] = [Case("K = 3, no node in common in the middle", _bow_batch(True))]
    T["eorb_kb8_triangulate_matches"] = [Case("65 pairs", _kb8_triangulate(65))]
    # ---- helpers
    T["eorb_hamming_bf_knn2"] = [Case("65 x 63", _knn(65, 63)), Case("3 queries, one train row", _knn(3, 1)), Case("no train row", _knn(3, 0))]
    T["eorb_hamming_window_match"] = [Case("lists of 0 to 200 candidates", _window_match())]
    T["eorb_distinctive_descriptors"] = [Case("points of 0 to 65 rows", _distinctive())]
    T["eorb_sort_by_response"] = [Case("65 keypoints", _sort(65)), Case("3 keypoints", _sort(3))]
    T["eorb_calc_optical_flow_pyr_lk"] = [Case("65 points", _lk(65))]
    T["eorb_bow_transform"] = [Case("65 descriptors", _bow_transform(65)), Case("3 descriptors", _bow_transform(3))]
    # ---- KeyFrameDatabase
    T["eorb_kfdb_add"] = [Case("three keyframes", _kfdb("add", 0))]
    T["eorb_kfdb_detect_reloc"] = [Case("a query", _kfdb("detect", 0)), Case("no shared word: an empty candidate list", _kfdb("detect", 0, empty=True))]
    T["eorb_kfdb_detect_nbest"] = [Case("a query", _kfdb("detect", 1)), Case("no shared word: an empty candidate list", _kfdb("detect", 1, empty=True))]
    # ---- projections
    T["eorb_project_frustum"] = [Case("65 points", _frustum(65, False)), Case("63 points, two cameras", _frustum(63, True))]
    T["eorb_project_last_frame"] = [Case("65 points", _project_last(65))]
    T["eorb_project_keyframe_points"] = [Case("65 points", _project_kf(65))]
    T["eorb_search_local_points"] = [Case("195 points, 130 keypoints", _local_points(195, 130)), Case("every point skipped", _local_points(65, 63, empty=True))]
    T["eorb_search_local_points_fisheye"] = [Case("195 points, 65 + 63 keypoints", _local_points_fisheye(195, 65, 63))]
    T["eorb_search_by_projection_last_pose"] = [Case("195 points, 130 keypoints", _last_pose(195, 130))]
    T["eorb_search_by_projection_kf_pose"] = [Case("195 points, 130 keypoints", _kf_pose(195, 130))]
    # ---- KeyFrame side
    T["eorb_kf_radius_match"] = [Case("planted scene", _kf_radius("plain")), Case("in order", _kf_radius("in order 50"))]
    T["eorb_kf_radius_match_stereo"] = [Case("planted scene, the stereo gate", _kf_radius("stereo gate"))]
    T["eorb_kf_radius_match_mixed"] = [Case("planted scene", _kf_radius("mixed gate")), Case("in order", _kf_radius("mixed in order 50"))]
    T["eorb_project_keyframe_side"] = [Case("65 points", _side_projection(65, False))]
    T["eorb_project_keyframe_side_mixed"] = [Case("65 points", _side_projection(65, True))]
    T["eorb_fuse_pose"] = [Case("195 points, 130 keypoints, stereo gate", _fuse_pose(195, 130, "stereo", False))]
    T["eorb_fuse_pose_mixed"] = [Case("195 points, 130 keypoints", _fuse_pose(195, 130, "mono", True))]
    T["eorb_search_by_projection_kf_scw"] = [Case("195 points, 130 keypoints", _kf_scw(195, 130, False))]
    T["eorb_search_by_projection_kf_scw_mixed"] = [Case("195 points, 130 keypoints", _kf_scw(195, 130, True))]
    T["eorb_fuse_keyframes"] = [Case("K = 3, an empty keyframe in the middle", _fuse_keyframes(195, (130, 0, 65), "stereo", False))]
    T["eorb_fuse_keyframes_mixed"] = [Case("K = 3, an empty keyframe in the middle", _fuse_keyframes(195, (130, 0, 65), "none", True))]
    T["eorb_search_by_sim3"] = [Case("130 slots a keyframe", _search_by_sim3(130))]
    # ---- the newest four
    T["eorb_sim3_ransac"] = [Case("K = 3, a short problem between two live ones", _sim3(True), canon=True), Case("N = 3 and a problem of wrong matches", _sim3(False), canon=True)]
    T["eorb_mlpnp_ransac"] = [Case("K = 3, a short problem between two live ones", _mlpnp(True), canon=True), Case("N = 7 and a problem of wrong matches", _mlpnp(False), canon=True)]
    T["eorb_new_map_points"] = [Case("K = 3, every match of the middle keyframe fails the parallax test", _newpts("mono")),
                                Case("stereo keyframes", _newpts("stereo")), Case("two-camera keyframes", _newpts("twocam"))]
    T["eorb_create_new_map_points"] = [Case("K = 3, no node in common in the middle", _create_newpts("pinhole"))]
    T["eorb_create_new_map_points_kb8"] = [Case("K = 3, no node in common in the middle", _create_newpts("kb8"))]
    T["eorb_two_view_ransac"] = [Case("65 matches, 9 sets", _tv_ransac("general", 65, 9), canon=True),
                                 Case("every key of image 2 in one place: no winner", _tv_ransac("same_keys", 65, 3), canon=True)]
    T["eorb_two_view_check_rt"] = [Case("65 matches, 4 poses", _tv_check_rt(65, 4, False), canon=True), Case("no inlier", _tv_check_rt(63, 1, True), canon=True)]
    T["eorb_two_view_reconstruct"] = [Case("H wins and reconstructs", _tv_reconstruct("planar", 65, 33, 0, min_triangulated=10), canon=True),
                                      Case("H wins, the other form", _tv_reconstruct("planar", 65, 33, 1, min_triangulated=10), canon=True),
                                      Case("F wins and reconstructs", _tv_reconstruct("general", 65, 33, 0, min_triangulated=10), canon=True),
                                      Case("F wins, the other form", _tv_reconstruct("general", 65, 33, 1, min_triangulated=10), canon=True),
                                      Case("F wins on 9 sets and is rejected", _tv_reconstruct("general", 65, 9, 0), canon=True),
                                      Case("noise: neither reconstructs", _tv_reconstruct("noise", 65, 9, 0), canon=True),
                                      Case("SH + SF == 0: the first exit", _tv_reconstruct("same_keys", 65, 3, 1), canon=True),
                                      Case("H forced on noise: no hypothesis has a point", _tv_reconstruct("noise", 10, 10, 0, seed=10, sets_seed=10, th_hf_ratio=0.0),
                                           canon=True)]
    return T


def _stereo_flat_both():
    def make(big):
        run_want = _stereo(lambda left, right: flat())(big)
        if big:
            return run_want
        p, w, h = _ext_args(False)
        left = right = flat()

        def run(fe, ctx):
            g = fe.ORBextractor(imSize=(w, h), ctx=ctx, **p).stereo(left, right, MB, MBF)
            return dict(nL=_i(len(g["kpsL"])), nR=_i(len(g["kpsR"])), nmatches=_i(g["nmatches"]), uRight=g["uRight"], depth=g["depth"])

        def want():
            return dict(nL=_i(0), nR=_i(0), nmatches=_i(0), uRight=np.zeros(0, F32), depth=np.zeros(0, F32))
        return run, want
    return make


NO_CASE = {
    "eorb_create": "makes the context; its one ensure() (the status word) is followed by a memset",
    "eorb_destroy": "frees the context",
    "eorb_sync": "waits and reads the status word",
    "eorb_debug_option": "a setter of host fields",
    "eorb_debug_option_get": "a getter of host fields",
    "eorb_debug_counter": "a getter: host fields, or a workspace read back",
    "eorb_debug_stage": "a getter: copies a workspace of the last extraction to the host",
    "eorb_last_error": "a getter of a host string",
    "eorb_version": "a getter of a constant string",
    "eorb_prof_enable": "profiler control",
    "eorb_prof_reset": "profiler control",
    "eorb_prof_only": "profiler control",
    "eorb_prof_count": "profiler control",
    "eorb_prof_get": "profiler control",
    "eorb_set_undistort_maps": "a setter: uploads the whole table it allocates; every raw-event case runs behind it",
    "eorb_set_calibration": "a setter of host fields",
    "eorb_orb_configure": "a setter: uploads the whole tables it allocates; every extraction case runs behind it",
    "eorb_orb_max_keypoints": "a getter of a host field",
    "eorb_orb_get_tables": "a getter of host tables",
    "eorb_bow_set_vocabulary": "a setter: uploads the whole table it allocates; the eorb_bow_transform cases run behind it",
    "eorb_resolve_num_mixed": "host arithmetic",
    "eorb_fe_configure": "a setter: allocates the batch's buffers and clears the counters; the batch walk runs behind it",
    "eorb_fe_last_f32_dev": "a getter: hands out the batch's float images, which the batch walk compares",
    "eorb_kfdb_clear": "a setter of host fields; every KeyFrameDatabase case starts with it",
    "eorb_kfdb_erase": "writes one slot record; the KeyFrameDatabase walk erases and queries",
    "eorb_kfdb_info": "a getter of host fields",
    "eorb_kfdb_get_scores": "a getter: copies the stored scores, which the KeyFrameDatabase cases compare",
    "eorb_selfcheck_division": "no arena: a kernel that adds into one word, cleared by a memset in front of it",
    "eorb_selfcheck_math": "no arena: a kernel that adds into one word, cleared by a memset in front of it",
    "eorb_pack_events": "a host function",
    "eorb_dev_alloc": "the caller's own memory",
    "eorb_dev_free": "the caller's own memory",
    "eorb_dev_upload": "the caller's own memory",
    "eorb_dev_download": "the caller's own memory",
}

WALKS = ("eorb_fe_run_batch_dev", "eorb_fe_run_batch_raw_dev", "eorb_fe_run_batch_raw4_dev", "eorb_fe_run_batch_raw2_dev", "eorb_fe_run_batch_images_dev")

TABLE = dict(_cases())
TABLE.update(NO_CASE)
TABLE.update({name: WALK for name in WALKS})


def all_cases():
    """(export, case) in table order"""
    return [(name, case) for name, v in TABLE.items() if isinstance(v, list) for case in v]
