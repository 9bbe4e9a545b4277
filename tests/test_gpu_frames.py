"""The host boundary of the extraction entry points, through the raw C ABI: eorb_orb_extract, eorb_frame_mono, eorb_frame_stereo,
eorb_frame_fisheye, eorb_ev_slice_extract and the tracked pair (eorb_orb_tracked_descriptors / eorb_orb_assign_level_by_best_desc).
What each returns for each bad argument, which bytes of the caller's buffers a good call writes, images with a row stride, both
describe forms without descriptors, tracked keypoints outside the level range.  Two configurations of tests/test_gpu_stages.py: its
smallest with more than one level and its 1-level one; every reference is computed once per configuration."""
import ctypes as C
import itertools

import numpy as np
import pytest

import calib_ref
import test_gpu_stages as stages
from eorb_slam_amd import _lib, synth

pytestmark = pytest.mark.gpu

OK, E_EMPTY, E_CAP, E_ARG, E_NOTCONF = _lib.EORB_OK, _lib.EORB_E_EMPTY, _lib.EORB_E_CAPACITY, _lib.EORB_E_ARG, _lib.EORB_E_NOTCONF
CFGS = [min((c for c in stages.CONFIGS if c[2] > 1), key=lambda c: c[0] * c[1]), next(c for c in stages.CONFIGS if c[2] == 1)]
MB, MBF, SIGMA, PAD = 0.11, 40.0, 1.0, 13
KP = synth.KP_DTYPE
ENTRIES = ("extract", "mono", "stereo", "fisheye", "slice")
# the caller's arrays of each entry: name -> (dtype, shape of one record); the counters behind them
ARRAYS = dict(extract=("kps", "desc", "oob"), slice=("kps", "desc", "oob"), mono=("kps", "un", "desc", "oob"),
              stereo=("kpsL", "descL", "kpsR", "descR", "uRight", "depth"), fisheye=("kpsL", "descL", "kpsR", "descR", "right_idx", "dist2"))
RECORD = dict(kps=(KP, ()), un=(KP, ()), kpsL=(KP, ()), kpsR=(KP, ()), desc=(np.uint8, (32,)), descL=(np.uint8, (32,)), descR=(np.uint8, (32,)),
              oob=(np.uint8, ()), uRight=(np.float32, ()), depth=(np.float32, ()), right_idx=(np.int32, ()), dist2=(np.int32, (2,)))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _a5(name, n):
    dt, shape = RECORD[name]
    return np.full(n * int(np.prod(shape, dtype=int)) * np.dtype(dt).itemsize, 0xA5, np.uint8).view(dt).reshape((n,) + shape)


class Scene:
    """One configuration: its images and events, the oracle's result of every entry point (cached), contexts"""

    def __init__(self, oracle, fe, cfg):
        self.oracle, self.fe = oracle, fe
        self.W, self.H, self.nl, sf, E = cfg
        self.p = stages._params(self.nl, sf, E)
        self.img = stages._image("texture", self.W, self.H)
        self.right = np.ascontiguousarray(np.roll(self.img, -4, axis=1))
        self.ev = synth.shapes_events(6000, self.W, self.H, seed=self.W, motion=0.4)
        self.lap = (self.W // 4, self.W // 2)
        self.cal = dict(open=synth.CALIBRATIONS["EvETHZ"], closed=dict(synth.CALIBRATIONS["EvETHZ"], dist=np.array([0.0, 0.3, 0.01, 0.02], np.float32)))
        self.oe = oracle.OrbExtractor(imWidth=self.W, **self.p)
        self.oe2 = oracle.OrbExtractor(imWidth=self.W, **self.p)
        self.ev_img = oracle.ev2im_gauss(self.ev, self.W, self.H, SIGMA, False, True)[1]
        self.cache = {}

    def extractor(self, cal="open"):
        ge = self.fe.ORBextractor(imSize=(self.W, self.H), **self.p)
        d = self.cal[cal]
        q = _lib.calib(d["model"], d["K"], d["dist"], d["R"], d["P"])
        ge.ctx.check(ge.ctx.L.eorb_set_calibration(ge.ctx.h, C.byref(q)))
        return ge

    def want(self, entry, lap=(0, 1000), want_desc=1, cal="open"):
        """(arrays, counters) of a good call; arrays[name] is None where the call must leave the caller's buffer alone"""
        key = (entry, lap, want_desc, cal)
        if key not in self.cache:
            self.cache[key] = self._want(entry, lap, want_desc, cal)
        return self.cache[key]

    def _want(self, entry, lap, want_desc, cal):
        if entry in ("extract", "mono", "slice"):
            mono, kp, desc, oob = self.oe.extract(self.ev_img if entry == "slice" else self.img, lap, bool(want_desc))
            assert len(kp) > 8
            arrays = dict(kps=kp, desc=desc, oob=oob if want_desc else np.zeros(len(kp), np.uint8))
            counters = dict(n=len(kp), mono=mono)
            if entry == "mono":
                arrays["un"] = calib_ref.undistort_keypoints(self.cal[cal], kp)
                assert (arrays["un"].tobytes() == kp.tobytes()) == (cal == "closed")
                counters["bounds"] = calib_ref.image_bounds(self.cal[cal], self.W, self.H).tobytes()
            return arrays, counters
        if entry == "stereo":
            _, kL, dL, _ = self.oe.extract(self.img, (0, 0)); _, kR, dR, _ = self.oe2.extract(self.right, (0, 0))
            ur, dp, nm = self.oe.compute_stereo_matches(self.oe2, kL, dL, kR, dR, MB, MBF)
            return dict(kpsL=kL, descL=dL, kpsR=kR, descR=dR, uRight=ur, depth=dp), dict(nL=len(kL), nR=len(kR), nmatches=nm)
        mL, kL, dL, _ = self.oe.extract(self.img, lap); mR, kR, dR, _ = self.oe.extract(self.right, lap)
        nc, cand, d2 = self.oracle.fisheye_matches(dL, mL, dR, mR)
        return dict(kpsL=kL, descL=dL, kpsR=kR, descR=dR, right_idx=cand, dist2=d2), dict(nL=len(kL), nR=len(kR), monoLeft=mL, monoRight=mR, ncand=nc)


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module", params=CFGS, ids=lambda c: "%dx%dx%d" % c[:3])
def scene(oracle, fe, request):
    return Scene(oracle, fe, request.param)


def _wide(img):
    w = np.full((img.shape[0], img.shape[1] + PAD), 0x5A, np.uint8)
    w[:, :img.shape[1]] = img
    return w


def _call(entry, c, S, cap, lap=(0, 1000), want_desc=1, use=None, img=True, W=None, H=None, stride=None, wide=False, ev=True):
    """One raw call; the caller's arrays hold `cap` records of 0xA5 bytes, those not in `use` are NULL.  Returns (code, arrays, counters)."""
    W = S.W if W is None else W; H = S.H if H is None else H
    left, right = (_wide(S.img), _wide(S.right)) if wide else (S.img, S.right)
    stride = left.strides[0] if stride is None else stride
    pl, pr = (_p(left), _p(right)) if img else (None, None)
    use = ARRAYS[entry] if use is None else use
    a = {k: _a5(k, max(cap, 1)) for k in ARRAYS[entry] if k in use}
    g = lambda k: _p(a.get(k))
    i = {k: C.c_int(77) for k in ("n", "mono", "nL", "nR", "monoLeft", "monoRight", "nmatches", "ncand")}
    r = lambda k: C.byref(i[k])
    L, h = c.L, c.h
    if entry == "extract":
        rc = L.eorb_orb_extract(h, pl, W, H, stride, lap[0], lap[1], want_desc, g("kps"), g("desc"), g("oob"), cap, r("n"), r("mono"))
        names = ("n", "mono")
    elif entry == "mono":
        bounds = np.full(4, -1.0, np.float32)
        rc = L.eorb_frame_mono(h, pl, W, H, stride, lap[0], lap[1], want_desc, g("kps"), g("un"), g("desc"), g("oob"), cap, r("n"), r("mono"), _p(bounds))
        names = ("n", "mono")
    elif entry == "slice":
        e = np.ascontiguousarray(S.ev)
        rc = L.eorb_ev_slice_extract(h, _p(e) if ev else None, None, len(e), SIGMA, lap[0], lap[1], want_desc, g("kps"), g("desc"), g("oob"), cap, r("n"), r("mono"), None)
        names = ("n", "mono")
    elif entry == "stereo":
        rc = L.eorb_frame_stereo(h, pl, pr, W, H, stride, MB, MBF, g("kpsL"), g("descL"), r("nL"), g("kpsR"), g("descR"), r("nR"), cap, g("uRight"), g("depth"), r("nmatches"))
        names = ("nL", "nR", "nmatches")
    else:
        rc = L.eorb_frame_fisheye(h, pl, pr, W, H, stride, lap[0], lap[1], lap[0], lap[1], g("kpsL"), g("descL"), r("nL"), r("monoLeft"),
                                  g("kpsR"), g("descR"), r("nR"), r("monoRight"), cap, g("right_idx"), g("dist2"), r("ncand"))
        names = ("nL", "nR", "monoLeft", "monoRight", "ncand")
    counters = {k: i[k].value for k in names}
    if entry == "mono" and rc == OK:
        counters["bounds"] = bounds.tobytes()
    return rc, a, counters


def _equals_oracle(S, entry, got, what, lap=(0, 1000), want_desc=1, cal="open"):
    """A good call: the counters, the records, and 0xA5 in every byte behind them (and in all of a buffer the call must not write)"""
    rc, arrays, counters = got
    warr, wcnt = S.want(entry, lap, want_desc, cal)
    assert rc == OK and counters == wcnt, (what, rc, counters, wcnt)
    for k, a in arrays.items():
        w = warr[k]
        raw = a.view(np.uint8).reshape(len(a), -1)
        n = 0 if w is None else len(w)
        assert raw[:n].tobytes() == (b"" if w is None else np.ascontiguousarray(w).tobytes()), (what, k)
        assert (raw[n:] == 0xA5).all(), (what, k, "written behind the %d records" % n)


def _zeroed(counters):
    return all(counters[k] == 0 for k in ("n", "nL", "nR") if k in counters)


@pytest.mark.parametrize("entry", ENTRIES)
def test_return_codes_and_the_context_survives(scene, fe, entry):
    """Every bad argument: the code, a zero keypoint count, untouched buffers; then a good call on the same context equals the oracle."""
    S = scene
    bare = fe.Context()
    ge = S.extractor()
    try:
        c, cap = ge.ctx, ge.cap
        n = max(v for k, v in S.want(entry)[1].items() if k in ("n", "nL", "nR"))
        rc, a, cnt = _call(entry, bare, S, cap)
        assert rc == E_NOTCONF and _zeroed(cnt), cnt
        bad = [("cap below the count", dict(cap=n - 1), E_CAP), ("cap 0", dict(cap=0), E_CAP)]
        if entry == "slice":
            bad += [("no events", dict(cap=cap, ev=False), E_ARG)]
        else:
            bad += [("NULL image", dict(cap=cap, img=False), E_EMPTY), ("W + 1", dict(cap=cap, W=S.W + 1), E_ARG), ("H + 1", dict(cap=cap, H=S.H + 1), E_ARG),
                    ("W - 1", dict(cap=cap, W=S.W - 1, stride=S.W), E_ARG), ("stride < W", dict(cap=cap, stride=S.W - 1), E_ARG),
                    ("W 0", dict(cap=cap, W=0), E_EMPTY), ("H -1", dict(cap=cap, H=-1), E_EMPTY)]
        if entry == "fisheye":
            bad += [("cap -1", dict(cap=-1), E_ARG)]
        else:
            bad += [("cap -1", dict(cap=-1), E_CAP)]
        for what, kw, code in bad:
            rc, a, cnt = _call(entry, c, S, **kw)
            assert rc == code, (what, rc, code)
            assert _zeroed(cnt), (what, cnt)
            assert all((v.view(np.uint8) == 0xA5).all() for v in a.values()), what
            _equals_oracle(S, entry, _call(entry, c, S, cap), "after " + what)
    finally:
        bare.close(); ge.ctx.close()


def test_return_codes_of_the_tracked_pair(scene, fe):
    S = scene
    _, kp, desc, _ = S.oe.extract(S.img)
    kp = kp[:16].copy(); ref = desc[:16].copy(); n = len(kp)
    od, oo = S.oe.tracked_descriptors(S.img, kp)
    ok = S.oe.assign_level_by_best_desc(S.img, ref, kp)
    bare = fe.Context()
    ge = S.extractor()
    try:
        def run(c, img=True, W=S.W, H=S.H, stride=S.W, n=n, null=False):
            d = _a5("desc", 16); o = _a5("oob", 16); k = kp.copy()
            r0 = c.L.eorb_orb_tracked_descriptors(c.h, _p(S.img) if img else None, W, H, stride, None if null else _p(k), n, None if null else _p(d), _p(o))
            r1 = c.L.eorb_orb_assign_level_by_best_desc(c.h, _p(S.img) if img else None, W, H, stride, None if null else _p(ref), None if null else _p(k), n)
            return r0, r1, d, o, k
        assert run(bare)[:2] == (E_NOTCONF, E_NOTCONF)
        for what, kw, code in (("NULL image", dict(img=False), E_EMPTY), ("W + 1", dict(W=S.W + 1), E_ARG), ("H + 1", dict(H=S.H + 1), E_ARG),
                               ("stride < W", dict(stride=S.W - 1), E_ARG), ("n -1", dict(n=-1), E_ARG), ("NULL buffers", dict(null=True), E_ARG)):
            r0, r1, d, o, k = run(ge.ctx, **kw)
            assert (r0, r1) == (code, code), (what, r0, r1)
            assert (d == 0xA5).all() and (o == 0xA5).all() and k.tobytes() == kp.tobytes(), what
            r0, r1, d, o, k = run(ge.ctx)
            assert (r0, r1) == (OK, OK) and np.array_equal(d, od) and np.array_equal(o, oo) and k.tobytes() == ok.tobytes(), what
        r0, r1, d, o, k = run(ge.ctx, n=0)
        assert (r0, r1) == (OK, OK) and (d == 0xA5).all() and (o == 0xA5).all() and k.tobytes() == kp.tobytes()
    finally:
        bare.close(); ge.ctx.close()


def _subsets(names):
    return [tuple(k for k, on in zip(names, m) if on) for m in itertools.product((1, 0), repeat=len(names))]


@pytest.mark.parametrize("entry", ENTRIES)
def test_copy_ranges(scene, entry):
    """Every combination of NULL and non-NULL caller arrays the end of the one download distinguishes, with and without descriptors,
    mono with the undistortion gate open and closed, and a capacity of exactly the count: the records equal the oracle's bit for bit,
    every byte behind them keeps its 0xA5, and want_desc = 0 leaves all of a non-NULL desc alone."""
    S = scene
    single = entry in ("extract", "mono", "slice")
    for cal in (("open", "closed") if entry == "mono" else ("open",)):
        ge = S.extractor(cal)
        try:
            for want_desc in ((1, 0) if single else (1,)):
                for lap in ((0, 1000), S.lap):
                    n = max(v for k, v in S.want(entry, lap, want_desc, cal)[1].items() if k in ("n", "nL", "nR"))
                    uses = _subsets(ARRAYS[entry]) if single else (ARRAYS[entry], (), ("kpsR", "descR"), ("kpsL", "right_idx", "uRight"))
                    for use in uses:
                        for cap in (ge.cap, n):
                            _equals_oracle(S, entry, _call(entry, ge.ctx, S, cap, lap, want_desc, use), (cal, want_desc, lap, use, cap), lap, want_desc, cal)
        finally:
            ge.ctx.close()


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e != "slice"])
def test_row_stride(scene, entry):
    """The images as the left columns of a buffer PAD bytes wider (eorb_ev_slice_extract takes no image)."""
    S = scene
    ge = S.extractor()
    try:
        for lap in ((0, 1000), S.lap):
            _equals_oracle(S, entry, _call(entry, ge.ctx, S, ge.cap, lap, wide=True), lap, lap)
            _equals_oracle(S, entry, _call(entry, ge.ctx, S, ge.cap, lap), lap, lap)
    finally:
        ge.ctx.close()


def _tracked_points(S):
    """Extractor keypoints moved off their pixels; every fifth one outside the level range: octave -1 and octave nlevels in turns"""
    _, kp, desc, _ = S.oe.extract(S.img)
    rng = np.random.default_rng(S.W)
    tk = kp.copy()
    tk["x"] += rng.normal(0, 1.5, len(tk)).astype(np.float32); tk["y"] += rng.normal(0, 1.5, len(tk)).astype(np.float32)
    tk["octave"][::10] = -1; tk["octave"][5::10] = S.nl
    return tk, desc


def test_row_stride_and_level_range_of_tracked_keypoints(scene):
    """tests/test_gpu_parity.py::test_tracked_descriptors_and_level_assignment has octaves -1 and 9 of 4 levels; here the first octave
    past the last level, both configurations, and the image with a row stride.  Mode 0: a zero descriptor and oob 0 outside the level
    range, the oracle's inside; mode 1 reassigns every keypoint as the oracle does."""
    S = scene
    tk, ref = _tracked_points(S)
    out = (tk["octave"] < 0) | (tk["octave"] >= S.nl)
    assert 0 < out.sum() < len(tk) and (tk["octave"] == S.nl).any() and (tk["octave"] == -1).any()
    od, oo = S.oe.tracked_descriptors(S.img, tk)
    ok = S.oe.assign_level_by_best_desc(S.img, ref, tk)
    assert od[~out].any() and (ok["octave"] >= 0).all() and (ok["octave"] < S.nl).all()
    ge = S.extractor()
    try:
        c = ge.ctx
        for img in (S.img, _wide(S.img)):
            d = _a5("desc", len(tk)); o = _a5("oob", len(tk)); k = tk.copy()
            assert c.L.eorb_orb_tracked_descriptors(c.h, _p(img), S.W, S.H, img.strides[0], _p(k), len(k), _p(d), _p(o)) == OK
            assert not d[out].any() and not o[out].any()
            assert np.array_equal(d, od) and np.array_equal(o, oo) and k.tobytes() == tk.tobytes()
            d = _a5("desc", len(tk)); k = tk.copy()
            assert c.L.eorb_orb_tracked_descriptors(c.h, _p(img), S.W, S.H, img.strides[0], _p(k), len(k), _p(d), None) == OK      # oob is optional
            assert np.array_equal(d, od)
            assert c.L.eorb_orb_assign_level_by_best_desc(c.h, _p(img), S.W, S.H, img.strides[0], _p(ref), _p(k), len(k)) == OK
            assert k.tobytes() == ok.tobytes()
    finally:
        ge.ctx.close()


def test_both_describe_forms_without_descriptors(scene):
    """want_desc = 0 through describe_kernel<false> and through orient_kernel + assemble_kernel (no brief_kernel), for the lapping
    area that holds every keypoint and one inside the image: keypoints and mono_index are the oracle's, oob is all zero."""
    S = scene
    ge = S.extractor()
    try:
        for lap in ((0, 1000), S.lap):
            for three in (0, 1):
                ge.ctx.debug_option("orb_three_launches", three)
                for entry in ("extract", "mono"):
                    got = _call(entry, ge.ctx, S, ge.cap, lap, 0)
                    _equals_oracle(S, entry, got, (lap, three, entry), lap, 0)
                    assert not got[1]["oob"][:got[2]["n"]].any() and got[2]["n"] > 8
        mono = S.want("extract", S.lap, 0)[1]
        assert S.nl == 1 or 0 < mono["mono"] < mono["n"]
    finally:
        ge.ctx.close()
