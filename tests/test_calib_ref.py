"""The CPU restatement of MyCalibrator (tests/calib_ref/calib_ref.c: cv::undistortPoints and cv::fisheye::undistortPoints of OpenCV
3.4.1, Frame::ComputeImageBounds, fdlibm's double tan) checked without a GPU: answers that can be derived by hand, a vectorised
float64 numpy restatement written here (bit for bit over whole sensor grids), and its tan against the host libm."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_ref                                    # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

CAL = synth.CALIBRATIONS
GRIDS = [(240, 180), (346, 260), (752, 480)]


# ---- the numpy restatement: the same operations, one numpy call per IEEE operation -------------------------------------------------
def _widen(d):
    K = np.asarray(d["K"], np.float32).astype(np.float64)
    k = np.zeros(12)
    k[:len(d["dist"])] = np.asarray(d["dist"], np.float32).astype(np.float64)
    R = np.eye(3) if d["R"] is None else np.asarray(d["R"], np.float32).astype(np.float64)
    if d["P"] is None:
        RR = R
    else:
        PP = np.asarray(d["P"], np.float32).astype(np.float64)[:, :3]
        RR = np.zeros((3, 3))
        for i in range(3):
            for j in range(3):
                if d["model"] == 0:
                    RR[i, j] = PP[i, 0] * R[0, j] + PP[i, 1] * R[1, j] + PP[i, 2] * R[2, j]
                else:
                    RR[i, j] = ((0.0 + PP[i, 0] * R[0, j]) + PP[i, 1] * R[1, j]) + PP[i, 2] * R[2, j]
    return K, k, RR


def np_pinhole(d, xy):
    K, k, RR = _widen(d)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    ifx, ify = 1.0 / fx, 1.0 / fy
    x = (xy[:, 0].astype(np.float64) - cx) * ifx
    y = (xy[:, 1].astype(np.float64) - cy) * ify
    one = np.float64(1.0)
    u0 = ((0.0 + one * x) + 0.0 * y) + 0.0
    u1 = ((0.0 + 0.0 * x) + one * y) + 0.0
    u2 = ((0.0 + 0.0 * x) + 0.0 * y) + 1.0
    inv = one / u2
    x = inv * u0; y = inv * u1
    x0, y0 = x, y
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    xx = RR[0, 0] * x + RR[0, 1] * y + RR[0, 2]
    yy = RR[1, 0] * x + RR[1, 1] * y + RR[1, 2]
    ww = one / (RR[2, 0] * x + RR[2, 1] * y + RR[2, 2])
    return np.stack([(xx * ww).astype(np.float32), (yy * ww).astype(np.float32)], axis=1)


def np_fisheye(d, xy):
    K, k, RR = _widen(d)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    pwx = (xy[:, 0].astype(np.float64) - cx) / fx
    pwy = (xy[:, 1].astype(np.float64) - cy) / fy
    hpi = np.pi / 2.0
    td = np.sqrt(pwx * pwx + pwy * pwy)
    td = np.where(-hpi < td, td, -hpi)
    td = np.where(hpi < td, hpi, td)
    big = td > 1e-8
    th = td.copy()
    with np.errstate(all="ignore"):
        for _ in range(10):
            t2 = th * th; t4 = t2 * t2; t6 = t4 * t2; t8 = t6 * t2
            th = td / (1 + k[0] * t2 + k[1] * t4 + k[2] * t6 + k[3] * t8)
        scale = np.where(big, calib_ref.tan(np.where(big, th, 0.0)) / td, 1.0)     # the C library's tan: everything around it is pinned
    pux = pwx * scale; puy = pwy * scale
    p = [((0.0 + RR[i, 0] * pux) + RR[i, 1] * puy) + RR[i, 2] * 1.0 for i in range(3)]
    return np.stack([(p[0] / p[2]).astype(np.float32), (p[1] / p[2]).astype(np.float32)], axis=1)


def np_undistort(d, xy):
    xy = np.ascontiguousarray(xy, np.float32)
    if not (abs(float(np.float32(d["dist"][0]))) > 1e-9):
        return xy.copy()
    return np_pinhole(d, xy) if d["model"] == 0 else np_fisheye(d, xy)


def _grid(W, H):
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    return np.stack([xs.ravel(), ys.ravel()], axis=1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- known answers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["EvETHZ", "EuRoC", "MVSEC_KB8", "pinhole5", "pinhole8"])
def test_principal_point_maps_to_the_principal_point_of_P(name):
    d = dict(CAL[name])
    d["P"] = np.array([[300.5, 0, 123.25, 7], [0, 301.5, 77.125, 0], [0, 0, 1, 0]], np.float32)
    K = np.asarray(d["K"], np.float32)
    out = calib_ref.undistort_points(d, np.array([[K[0, 2], K[1, 2]]], np.float32))
    assert out[0, 0] == np.float32(123.25) and out[0, 1] == np.float32(77.125)
    d["P"] = d["K"]
    out = calib_ref.undistort_points(d, np.array([[K[0, 2], K[1, 2]]], np.float32))
    assert np.array_equal(_bits(out[0]), _bits(np.array([K[0, 2], K[1, 2]], np.float32)))


@pytest.mark.parametrize("model", [0, 1])
def test_gate_copies_when_k1_is_tiny_whatever_the_rest(model):
    d = dict(CAL["gate_closed"]); d["model"] = model
    assert abs(float(d["dist"][0])) <= 1e-9 and abs(float(d["dist"][1])) > 0.1
    kps = synth.calib_keypoints(300, 240, 180, seed=3)
    out = calib_ref.undistort_keypoints(d, kps)
    assert out.tobytes() == kps.tobytes()
    xy = np.stack([kps["x"], kps["y"]], axis=1)
    assert np.array_equal(_bits(calib_ref.undistort_points(d, xy)), _bits(xy))
    mx, my = calib_ref.generate_maps(d, 240, 180)
    g = _grid(240, 180)
    assert np.array_equal(mx.ravel(), g[:, 0]) and np.array_equal(my.ravel(), g[:, 1])
    # just above the gate the same coefficients do move the points
    d["dist"] = d["dist"].copy(); d["dist"][0] = np.float32(2e-9)
    assert not np.array_equal(_bits(calib_ref.undistort_points(d, xy)), _bits(xy))


def test_fisheye_small_angle_has_scale_one():
    d = dict(model=1, K=np.eye(3, dtype=np.float32), dist=np.array([1e15, 0, 0, 0], np.float32), R=None, P=None, size=(1, 1))
    xy = np.array([[5e-9, 0], [0, -1e-8], [6e-9, 7.9e-9]], np.float32)        # theta_d <= 1e-8
    td = np.sqrt(xy[:, 0].astype(np.float64) ** 2 + xy[:, 1].astype(np.float64) ** 2)
    assert np.all(td <= 1e-8)
    assert np.array_equal(_bits(calib_ref.undistort_points(d, xy)), _bits(xy))
    far = np.array([[2e-8, 0]], np.float32)                                      # above the threshold the (huge) coefficient acts
    o = calib_ref.undistort_points(d, far)
    assert o[0, 0] != far[0, 0] and o[0, 0] < far[0, 0]


def test_empty_input_is_left_alone():
    out = np.zeros(4, calib_ref.KP_DTYPE); out["x"] = 7; out["class_id"] = -5
    keep = out.copy()
    calib_ref.undistort_keypoints(CAL["EvETHZ"], np.zeros(0, calib_ref.KP_DTYPE), out=out)
    assert out.tobytes() == keep.tobytes()


def test_keypoint_fields_are_copied_through():
    kps = synth.calib_keypoints(500, 240, 180, seed=5)
    out = calib_ref.undistort_keypoints(CAL["EvETHZ"], kps)
    for f in ("size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(out[f], kps[f])
    xy = calib_ref.undistort_points(CAL["EvETHZ"], np.stack([kps["x"], kps["y"]], axis=1))
    assert np.array_equal(_bits(out["x"]), _bits(xy[:, 0])) and np.array_equal(_bits(out["y"]), _bits(xy[:, 1]))
    assert not np.array_equal(out["x"], kps["x"])


def test_image_bounds_has_its_own_gate_and_pairing():
    # dist[0] != 0.0, not isDistorted: 1e-10 closes the calibrator's gate and opens this one
    d = CAL["gate_closed"]
    W, H = 240, 180
    b = calib_ref.image_bounds(d, W, H)
    assert not np.array_equal(b, np.array([0, W, 0, H], np.float32))
    z = dict(d); z["dist"] = d["dist"].copy(); z["dist"][0] = 0.0
    assert np.array_equal(calib_ref.image_bounds(z, W, H), np.array([0, W, 0, H], np.float32))
    # the corners go through cv::undistortPoints(K, dist, cv::Mat(), K) whatever the model, R and P are; min / max pair them as :855-858
    for name in ("EvETHZ", "MVSEC_KB8", "pinhole_RP", "fisheye_RP", "pinhole8"):
        d = CAL[name]
        W, H = d["size"]
        pin = dict(d); pin["model"] = 0; pin["R"] = None; pin["P"] = d["K"]
        c = calib_ref.cv_undistort_points(pin, np.array([[0, 0], [W, 0], [0, H], [W, H]], np.float32))
        want = np.array([min(c[0, 0], c[2, 0]), max(c[1, 0], c[3, 0]), min(c[0, 1], c[1, 1]), max(c[2, 1], c[3, 1])], np.float32)
        assert np.array_equal(_bits(calib_ref.image_bounds(d, W, H)), _bits(want)), name
    # the pairing is not the extreme of all four corners: with a strong tangential term the two differ
    t = dict(CAL["EvETHZ"]); t["dist"] = np.array([-0.3, 0.1, 0.05, -0.04], np.float32)
    c = calib_ref.cv_undistort_points(t, np.array([[0, 0], [240, 0], [0, 180], [240, 180]], np.float32))
    b = calib_ref.image_bounds(t, 240, 180)
    assert b[0] == min(c[0, 0], c[2, 0]) and b[3] == max(c[2, 1], c[3, 1])


def test_validity_of_the_record():
    L = calib_ref.lib()
    import ctypes as C
    q = calib_ref.calib(CAL["EvETHZ"])
    assert L.cr_valid(C.byref(q)) == 1
    for field, bad in (("n_dist", 6), ("n_dist", 3), ("model", 2), ("p_cols", 2), ("p_cols", 5)):
        q = calib_ref.calib(CAL["EvETHZ"]); setattr(q, field, bad)
        assert L.cr_valid(C.byref(q)) == 0, (field, bad)
    q = calib_ref.calib(CAL["MVSEC_KB8"]); q.n_dist = 5
    assert L.cr_valid(C.byref(q)) == 0


# ---- the numpy restatement, whole grids -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CAL))
@pytest.mark.parametrize("size", GRIDS)
def test_c_equals_numpy_on_whole_grids(name, size):
    d = CAL[name]
    W, H = size
    mx, my = calib_ref.generate_maps(d, W, H)
    want = np_undistort(d, _grid(W, H))
    assert np.array_equal(_bits(mx.ravel()), _bits(want[:, 0])) and np.array_equal(_bits(my.ravel()), _bits(want[:, 1]))
    assert np.isfinite(mx).all() and np.isfinite(my).all()


@pytest.mark.parametrize("name", sorted(CAL))
def test_c_equals_numpy_on_subpixel_keypoints(name):
    d = CAL[name]
    W, H = d["size"]
    kps = synth.calib_keypoints(20000, W, H, seed=11)
    xy = np.stack([kps["x"], kps["y"]], axis=1)
    assert np.array_equal(_bits(calib_ref.undistort_points(d, xy)), _bits(np_undistort(d, xy)))


# ---- the restated tan against the host libm ------------------------------------------------------------------------------------------------
def test_tan_against_host_libm():
    n = 1 << 22
    x = np.concatenate([np.linspace(1e-8, np.pi / 2, n), np.geomspace(1e-8, np.pi / 2, n),
                        np.nextafter(np.pi / 2, 0) - np.arange(0, 4096) * 2.220446049250313e-16, np.array([np.pi / 4, np.pi / 2])])
    x = x[(x > 1e-8) & (x <= np.pi / 2)]
    a = calib_ref.tan(x)
    b = np.tan(x)
    ulp = np.abs(a.view(np.int64) - b.view(np.int64))
    ndiff = int((ulp > 0).sum())
    print("restated tan against the host libm: %d arguments, %d differ, largest difference %d ulp" % (len(x), ndiff, int(ulp.max())))
    assert ulp.max() <= 1
    # how many float map entries of the MVSEC grid change when the host's tan takes the restated one's place (recorded, not asserted)
    d = CAL["MVSEC_KB8"]
    W, H = d["size"]
    r = calib_ref.generate_maps(d, W, H)
    h = calib_ref.generate_maps(d, W, H, host_tan=True)
    changed = int((_bits(r[0]) != _bits(h[0])).sum() + (_bits(r[1]) != _bits(h[1])).sum())
    print("MVSEC %dx%d maps: %d of %d float entries change with the host tan" % (W, H, changed, 2 * W * H))


def test_tan_special_arguments():
    x = np.array([0.0, -0.0, 1e-300, 2.0 ** -30, -0.5, 0.7, -1.2, 2.0, -2.5, np.inf, np.nan])
    a = calib_ref.tan(x)
    with np.errstate(invalid="ignore"):
        b = np.tan(x)
    fin = np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.all(np.abs(a[fin].view(np.int64) - b[fin].view(np.int64)) <= 1)
    assert np.signbit(a[1]) and a[0] == 0.0
