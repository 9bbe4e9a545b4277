"""MyCalibrator on the device (GPU): eorb_set_calibration, eorb_undistort_keypoints / _points, eorb_generate_undistort_maps and
eorb_frame_mono through the C ABI, every output compared bit for bit with the CPU restatement tests/calib_ref/calib_ref.c."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_ref                                    # noqa: E402
from eorb_slam_amd import _lib, synth               # noqa: E402

pytestmark = pytest.mark.gpu

CAL = synth.CALIBRATIONS
NAMES = sorted(CAL)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def ctx():
    from eorb_slam_amd import frontend
    c = frontend.Context()
    yield c
    c.close()


def _set(ctx, d):
    q = _lib.calib(d["model"], d["K"], d["dist"], d["R"], d["P"])
    ctx.check(ctx.L.eorb_set_calibration(ctx.h, C.byref(q)))


def _points(ctx, xy):
    xy = np.ascontiguousarray(xy, np.float32)
    out = np.full_like(xy, -12345.0)
    ctx.check(ctx.L.eorb_undistort_points(ctx.h, _p(xy), len(xy), _p(out)))
    return out


def _keypoints(ctx, kps):
    out = np.zeros(len(kps), synth.KP_DTYPE); out["class_id"] = -77
    ctx.check(ctx.L.eorb_undistort_keypoints(ctx.h, _p(kps), len(kps), _p(out)))
    return out


# ---- maps ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_generated_maps_equal_the_restatement(ctx, name):
    d = CAL[name]
    W, H = d["size"]
    _set(ctx, d)
    mx = np.zeros((H, W), np.float32); my = np.zeros((H, W), np.float32)
    ctx.check(ctx.L.eorb_generate_undistort_maps(ctx.h, W, H, 1, _p(mx), _p(my)))
    rx, ry = calib_ref.generate_maps(d, W, H)
    assert np.array_equal(_bits(mx), _bits(rx)) and np.array_equal(_bits(my), _bits(ry))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("check", [1, 0])
def test_raw_events_through_generated_maps_equal_uploaded_maps(name, check):
    """eorb_ev2im_gauss_raw (sigma 1) after eorb_generate_undistort_maps == the same call after eorb_set_undistort_maps with the
    restatement's maps: the u8 image, the float image, and the events the loader's rectification keeps."""
    from eorb_slam_amd import frontend
    d = CAL[name]
    W, H = d["size"]
    raw = synth.random_raw_events(60000, W, H, seed=21)
    rx, ry = calib_ref.generate_maps(d, W, H)
    res = []
    for generated in (True, False):
        c = frontend.Context()
        if generated:
            _set(c, d)
            c.check(c.L.eorb_generate_undistort_maps(c.h, W, H, check, None, None))
        else:
            c.check(c.L.eorb_set_undistort_maps(c.h, _p(rx), _p(ry), W, H, check))
        f32, u8, mm = frontend.EvImConverter.ev2im_gauss_raw(raw, W, H, 1.0, False, True, ctx=c, return_all=True)
        kept = frontend.EvImConverter.undistort_events(raw, W, H, 1.0, ctx=c)
        res.append((f32.copy(), u8.copy(), mm.copy(), kept))
        c.close()
    a, b = res
    assert a[1].tobytes() == b[1].tobytes()
    assert len(a[3]) == len(b[3]) and a[3].tobytes() == b[3].tobytes()
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[2]), _bits(b[2]))
    if check and name != "pinhole_noP":
        assert 0 < len(a[3]) <= len(raw)


# ---- keypoints and points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_keypoints_and_points_equal_the_restatement(ctx, name):
    d = CAL[name]
    W, H = d["size"]
    _set(ctx, d)
    for n in (0, 1, 63, 64, 65, 5000):
        kps = synth.calib_keypoints(n, W, H, seed=100 + n, margin=0.1)
        want = calib_ref.undistort_keypoints(d, kps)
        assert np.isfinite(want["x"]).all() and np.isfinite(want["y"]).all()          # the margin keeps the restatement finite
        got = _keypoints(ctx, kps)
        assert got.tobytes() == want.tobytes() if n else (got["class_id"] == -77).all(), (name, n)
        xy = np.stack([kps["x"], kps["y"]], axis=1) if n else np.zeros((0, 2), np.float32)
        wxy = calib_ref.undistort_points(d, xy)
        assert np.array_equal(_bits(_points(ctx, xy)), _bits(wxy)), (name, n)
        if n:
            assert np.array_equal(_bits(wxy[:, 0]), _bits(want["x"]))
    if name == "gate_closed":
        kps = synth.calib_keypoints(500, W, H, seed=9)
        assert _keypoints(ctx, kps).tobytes() == kps.tobytes()


def test_empty_input_writes_nothing(ctx):
    _set(ctx, CAL["EvETHZ"])
    out = np.zeros(3, synth.KP_DTYPE); out["x"] = 5; keep = out.copy()
    assert ctx.L.eorb_undistort_keypoints(ctx.h, None, 0, _p(out)) == 0
    assert ctx.L.eorb_undistort_points(ctx.h, None, 0, None) == 0
    assert out.tobytes() == keep.tobytes()


@pytest.mark.parametrize("name", ["EvETHZ", "pinhole8", "MVSEC_KB8", "fisheye_RP"])
def test_far_outside_points_agree_by_class(ctx, name):
    """Far outside the image the iterations overflow: non-finite outputs are compared by class (host and device differ in the sign of
    a generated NaN), finite ones still by bits."""
    d = CAL[name]
    _set(ctx, d)
    v = np.array([-1e30, -1e12, -1e6, -3e4, -5000, 0, 5000, 3e4, 1e6, 1e12, 1e30, np.inf, -np.inf, np.nan], np.float32)
    xy = np.stack(np.meshgrid(v, v), axis=-1).reshape(-1, 2)
    got = _points(ctx, xy).ravel()
    want = calib_ref.undistort_points(d, xy).ravel()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(np.isinf(got[ok]), np.isinf(want[ok]))
    assert np.array_equal(_bits(got[ok]), _bits(want[ok]))                            # (an infinity's bits carry its sign)
    assert (~np.isfinite(want)).any()


# ---- hash sweep -----------------------------------------------------------------------------------------------------------------------------
def _hash(xy, out):
    i = np.arange(len(xy), dtype=np.uint64)
    ob = _bits(out).astype(np.uint64)
    h = ((i * np.uint64(0x9E3779B97F4A7C15)) ^ (ob[:, 0] | (ob[:, 1] << np.uint64(32)))) * np.uint64(0xC2B2AE3D27D4EB4F)
    return int(np.add.reduce(h, dtype=np.uint64))


@pytest.mark.parametrize("name", ["EvETHZ", "pinhole8", "pinhole_RP", "MVSEC_KB8", "fisheye_RP"])
def test_hash_sweep_over_a_subpixel_lattice(ctx, name):
    """2^22 points of a 2048 x 2048 lattice over the image (steps of W / 2048, H / 2048 pixels): the hash of the device's output bits
    equals the restatement's."""
    d = CAL[name]
    W, H = d["size"]
    _set(ctx, d)
    N = 2048
    xs = (np.arange(N, dtype=np.float64) * (W / N)).astype(np.float32)
    ys = (np.arange(N, dtype=np.float64) * (H / N)).astype(np.float32)
    xy = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)
    assert len(xy) == 1 << 22
    with np.errstate(over="ignore"):
        want = _hash(xy, calib_ref.undistort_points(d, xy))
        got = _hash(xy, _points(ctx, xy))
    assert got == want


# ---- the monocular frame ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,nlevels,nfeat,cal", [(240, 180, 4, 1000, "EvETHZ"), (752, 480, 8, 1500, "EuRoC"), (752, 480, 8, 1500, "pinhole_RP"),
                                                   (240, 180, 4, 1000, "fisheye_RP"), (240, 180, 4, 1000, "gate_closed")])
def test_frame_mono(W, H, nlevels, nfeat, cal):
    from eorb_slam_amd import frontend
    d = CAL[cal]
    ex = frontend.ORBextractor(nfeat, 1.2, nlevels, 20, 7, 19, (W, H))
    c = ex.ctx
    _set(c, d)
    for seed in (3, 4):
        img = synth.texture_image(W, H, seed=seed)
        mono, kps, desc, oob = ex(img, (0, 1000), True)
        r = ex.frame_mono(img, (0, 1000), True)
        assert len(kps) > 100
        assert r["mono"] == mono and len(r["kps"]) == len(kps)
        assert r["kps"].tobytes() == kps.tobytes() and r["desc"].tobytes() == desc.tobytes() and r["oob"].tobytes() == oob.tobytes()
        assert r["kps_un"].tobytes() == calib_ref.undistort_keypoints(d, kps).tobytes()
        assert np.array_equal(_bits(r["bounds"]), _bits(calib_ref.image_bounds(d, W, H)))
        if cal == "gate_closed":
            assert r["kps_un"].tobytes() == kps.tobytes()
        else:
            assert r["kps_un"].tobytes() != kps.tobytes()
    # detect-only, a lapping area, and only the undistorted keypoints wanted
    img = synth.texture_image(W, H, seed=5)
    mono, kps, _, _ = ex(img, (W // 3, 2 * W // 3), False)
    r = ex.frame_mono(img, (W // 3, 2 * W // 3), False)
    assert r["mono"] == mono and r["kps"].tobytes() == kps.tobytes()
    assert r["kps_un"].tobytes() == calib_ref.undistort_keypoints(d, kps).tobytes()
    un = np.zeros(ex.cap, synth.KP_DTYPE); n = C.c_int()
    c.check(c.L.eorb_frame_mono(c.h, _p(img), W, H, W, W // 3, 2 * W // 3, 0, None, _p(un), None, None, ex.cap, C.byref(n), None, None))
    assert n.value == len(kps) and un[:n.value].tobytes() == r["kps_un"].tobytes()
    c.close()


def test_frame_mono_closed_bounds_gate():
    """dist[0] == 0.0 closes both gates: kps_un == kps and the bounds are 0, W, 0, H"""
    from eorb_slam_amd import frontend
    W, H = 240, 180
    d = dict(CAL["EvETHZ"]); d["dist"] = np.array([0.0, 0.3, 0.01, 0.02], np.float32)
    ex = frontend.ORBextractor(1000, 1.2, 4, 20, 7, 19, (W, H))
    _set(ex.ctx, d)
    r = ex.frame_mono(synth.texture_image(W, H, seed=3))
    assert len(r["kps"]) > 100 and r["kps_un"].tobytes() == r["kps"].tobytes()
    assert np.array_equal(r["bounds"], np.array([0, W, 0, H], np.float32))
    ex.ctx.close()


# ---- error paths --------------------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    from eorb_slam_amd import frontend
    c = frontend.Context()
    L = c.L
    xy = np.zeros((4, 2), np.float32); out = np.zeros((4, 2), np.float32)
    kps = synth.calib_keypoints(4, 240, 180); kout = np.zeros(4, synth.KP_DTYPE)
    assert L.eorb_undistort_points(c.h, _p(xy), 4, _p(out)) == _lib.EORB_E_NOTCONF
    assert L.eorb_undistort_keypoints(c.h, _p(kps), 4, _p(kout)) == _lib.EORB_E_NOTCONF
    assert L.eorb_generate_undistort_maps(c.h, 240, 180, 1, None, None) == _lib.EORB_E_NOTCONF
    ex = frontend.ORBextractor(500, 1.2, 4, 20, 7, 19, (240, 180), ctx=c)
    img = synth.texture_image(240, 180, seed=3)
    n = C.c_int()
    assert L.eorb_frame_mono(c.h, _p(img), 240, 180, 240, 0, 1000, 0, None, None, None, None, ex.cap, C.byref(n), None, None) == _lib.EORB_E_NOTCONF
    d = CAL["EvETHZ"]
    for field, bad in (("n_dist", 6), ("n_dist", 3), ("n_dist", 0), ("model", 2), ("model", -1), ("p_cols", 2), ("p_cols", 5)):
        q = _lib.calib(d["model"], d["K"], d["dist"], d["R"], d["P"]); setattr(q, field, bad)
        assert L.eorb_set_calibration(c.h, C.byref(q)) == _lib.EORB_E_ARG, (field, bad)
    k = CAL["MVSEC_KB8"]
    q = _lib.calib(1, k["K"], k["dist"], k["R"], k["P"]); q.n_dist = 5
    assert L.eorb_set_calibration(c.h, C.byref(q)) == _lib.EORB_E_ARG
    assert L.eorb_set_calibration(c.h, None) == _lib.EORB_E_ARG
    assert L.eorb_undistort_points(c.h, _p(xy), 4, _p(out)) == _lib.EORB_E_NOTCONF          # a refused calibration sets nothing
    _set(c, d)
    assert L.eorb_undistort_points(c.h, _p(xy), -1, _p(out)) == _lib.EORB_E_ARG
    assert L.eorb_undistort_points(c.h, None, 4, _p(out)) == _lib.EORB_E_ARG
    assert L.eorb_generate_undistort_maps(c.h, 0, 180, 1, None, None) == _lib.EORB_E_ARG
    want = calib_ref.undistort_keypoints(d, kps)
    # the calibration survives an unrelated eorb_orb_configure
    frontend.ORBextractor(300, 1.2, 2, 20, 7, 19, (346, 260), ctx=c)
    c.check(L.eorb_undistort_keypoints(c.h, _p(kps), 4, _p(kout)))
    assert kout.tobytes() == want.tobytes()
    c.close()


def test_python_mirror(ctx):
    from eorb_slam_amd import frontend
    d = CAL["MVSEC_KB8"]
    W, H = d["size"]
    cal = frontend.MyCalibrator.from_dict(d, ctx=ctx)
    kps = synth.calib_keypoints(777, W, H, seed=2)
    assert cal.undistKeyPoints(kps).tobytes() == calib_ref.undistort_keypoints(d, kps).tobytes()
    xy = np.stack([kps["x"], kps["y"]], axis=1)
    assert np.array_equal(_bits(cal.undistPoint(xy)), _bits(calib_ref.undistort_points(d, xy)))
    mx, my = cal.generateUndistMaps()
    rx, ry = calib_ref.generate_maps(d, W, H)
    assert np.array_equal(_bits(mx), _bits(rx)) and np.array_equal(_bits(my), _bits(ry))
    assert len(cal.undistKeyPoints(np.zeros(0, synth.KP_DTYPE))) == 0
