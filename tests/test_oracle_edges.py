"""The oracle at non-finite and out-of-range inputs of its float-to-index steps (no GPU), in both builds: parity and fast=True.

The expectations are those of tests/edge_inputs.py and follow from its rule alone (a conversion of NaN, +-inf or a value outside
int32 yields INT_MIN; the reference's next comparison decides).  The oracle's own answers for such inputs rest on what gcc makes of an
out-of-range cast, which C leaves undefined: these tests are what pins them.  The checks themselves live in tests/edge_inputs.py;
tests/test_gpu_edges.py applies the same ones to the kernels, next to byte equality with the oracle.

Teeth.  Every family's expectation also runs against a named wrong variant of the conversion ("saturate": the bare device
conversion, NaN -> 0; "half_even"; "alias16") and must fail."""

import numpy as np
import pytest

import edge_inputs as ei
import plain_ref as pr
import test_oracle_plain as op
from edge_inputs import (BUILDS, LK_CASES, MCI, MCI_BLANK, RAW_H, RAW_W, SCALE_FACTORS, SIGMAS, blank_events,
                         check_acc_rule, check_blank, check_count_rule, check_degenerate_images, check_mci_plain,
                         check_mci_rule, count_events, fuse_expected, init_frames, lk_run, mci_oracle, mci_plain_uv,
                         mci_uv_tolerance, oracle_tracker, proj_last_args, projection_runs, projection_uv,
                         sim3_expected, tie_image, tracked_scene)

F64 = np.float64

# ---------------------------------------------------------------------------------------------------
# the rule itself
def test_the_rule_and_its_wrong_variants():
    big = [ei.NAN, ei.INF, -ei.INF, 3e9, -3e9, 1e30, 2147483648.0, -2147483904.0]
    assert [ei.floor_index(v) for v in big] == [ei.INT_MIN] * len(big)
    assert ei.floor_index(-2147483648.0) == ei.INT_MIN and ei.floor_index(2147483520.0) == 2147483520
    assert [ei.floor_index(v, "saturate") for v in big[:4]] == [0, ei.INT_MAX, ei.INT_MIN, ei.INT_MAX]
    assert ei.floor_index(ei.f32(-1e-40)) == -1 and ei.floor_index(ei.f32(1e-40)) == 0 and ei.floor_index(-0.0) == 0
    assert ei.floor_index(65546.25) == 65546 and ei.floor_index(65546.25, "alias16") == 10 and ei.floor_index(-65525.75, "alias16") == 10
    assert ei.floor_index(32778.25, "alias16") == -32758 and ei.floor_index(-32757.75, "alias16") == -32758
    assert [ei.round_index(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 60.5)] == [1, 2, 3, -1, -2, 61]
    assert [ei.round_index(v, "half_even") for v in (0.5, 1.5, 2.5, -0.5)] == [0, 2, 2, 0]
    assert ei.round_index(ei.NAN) == ei.INT_MIN and ei.round_index(3e9) == ei.INT_MIN

@pytest.mark.parametrize("fast", BUILDS)
@pytest.mark.parametrize("pol", [False, True])
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("W,H", ei.SIZES)
def test_ev2im_gauss_edges(oracle, W, H, sigma, pol, fast):
    h = pr.stamp_radius(sigma)
    ev, special, _ = ei.acc_case(W, H, h)
    what = "%dx%d sigma %.1f pol %d fast %d" % (W, H, sigma, pol, fast)
    got = oracle.ev2im_gauss(ev, W, H, sigma, pol, True, fast=fast)
    nkeep = check_acc_rule(what, got, oracle, ev, W, H, sigma, pol, fast)
    # the ordinary events, -0.0, +-1e-40 and the reaching edge and corner positions: 3 + 3 + 1 specials per placement reach at least
    assert ei.N_ORDINARY + 10 <= nkeep < len(ev) - 3 * 12, (nkeep, len(ev))
    for wrong in ("saturate", "alias16"):
        with pytest.raises(AssertionError, match="pixels differ"):
            check_acc_rule(what, got, oracle, ev, W, H, sigma, pol, fast, wrong=wrong)
    blank = blank_events(W, H, h)
    check_blank(what + " blank", oracle.ev2im_gauss(blank, W, H, sigma, pol, True, fast=fast), W, H)

@pytest.mark.parametrize("fast", BUILDS)
@pytest.mark.parametrize("W,H", ei.SIZES)
def test_ev2im_count_ties_and_edges(oracle, W, H, fast):
    run = lambda ev, pol: oracle.ev2im(ev, W, H, pol, True, fast=fast)
    what = "%dx%d fast %d" % (W, H, fast)
    check_count_rule(what, run, oracle, W, H, fast)
    for wrong in ("half_even", "saturate", "alias16"):
        with pytest.raises(AssertionError):
            check_count_rule(what, run, oracle, W, H, fast, wrong=wrong)

@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_raw_path_edges(oracle, sigma, check):
    W, H = RAW_W, RAW_H
    h = pr.stamp_radius(sigma)
    mx, my, raw, special = ei.raw_case(W, H, h)
    want = ei.raw_expected_events(mx, my, raw, W, H, check)
    got = oracle.undistort_events(raw, mx, my, W, H, check, 1.0)
    assert ei.same_events(got, want), "undistort_events keeps %d events, by hand %d" % (len(got), len(want))
    assert (len(want) < len(raw)) == check and len(want) >= ei.N_ORDINARY + 4      # (-0.0 and +1e-40 pass the check)
    for fast in BUILDS:
        for pol in (False, True):
            what = "raw sigma %.1f check %d pol %d fast %d" % (sigma, check, pol, fast)
            res = oracle.ev2im_gauss(got, W, H, sigma, pol, True, fast=fast)
            check_acc_rule(what, res, oracle, want, W, H, sigma, pol, fast)
            if not check:                                                # (with the check no position of V is left to convert)
                for wrong in ("saturate", "alias16"):
                    with pytest.raises(AssertionError, match="pixels differ"):
                        check_acc_rule(what, res, oracle, want, W, H, sigma, pol, fast, wrong=wrong)
    run = lambda ev, pol: oracle.ev2im(ev, W, H, pol, True)
    for pol in (False, True):
        sub, _ = ei.acc_expected_events(want, W, H, 0, count=True)
        assert np.array_equal(run(got, pol)[0].view(np.uint32), run(sub, pol)[0].view(np.uint32))

@pytest.mark.parametrize("case", sorted(MCI))
def test_motion_compensated_edges(oracle, case):
    for pol in (False, True):
        got, uv = mci_oracle(oracle, case, pol)
        nkeep = check_mci_rule(case, case, got, uv, oracle, pol)
        check_mci_plain(case, case, got, uv, pol)
        if any(k in case for k in MCI_BLANK):
            with pytest.raises(AssertionError, match="pixels differ"):           # NaN -> 0 stamps every event on the corner
                check_mci_rule(case, case, got, uv, oracle, pol, wrong="saturate")
        elif "past the clamp" in case or "scale 0" in case:
            assert nkeep > 20, nkeep                                             # (the image is not empty)
            with pytest.raises(AssertionError):                                   # the rate measured from the wrong end of the window
                check_mci_plain(case, case, got, uv, pol, wrong="rate")

@pytest.mark.parametrize("fast", BUILDS)
@pytest.mark.parametrize("case", LK_CASES)
def test_pyr_lk_edges(oracle, case, fast):
    assert len(ei.lk_level_sizes()) == ei.LK_MAXLEVEL + 1
    got, plain = lk_run(oracle_tracker(oracle, fast), case)
    assert plain[1].tolist() == [1] * len(plain[1])                       # the ordinary points are tracked: by 1 px in x
    assert np.abs(plain[0].astype(F64) - ei.lk_ordinary() - [1.0, 0.0]).max() < 0.05
    what = "%s fast %d" % (case, fast)
    ei.check_lk_rule(what, case, *got, plain)
    if "boundary" not in case:                                           # (the boundary cases hold no NaN)
        with pytest.raises(AssertionError, match="was not processed"):
            ei.check_lk_rule(what, case, *got, plain, wrong="saturate")

@pytest.mark.parametrize("fast", BUILDS)
def test_search_for_initialization_edges(oracle, fast):
    (k1, d1), (k2, d2) = init_frames(oracle)
    F1 = oracle.Frame(k1, d1, ei.INIT_W, ei.INIT_H, fast=fast); F2 = oracle.Frame(k2, d2, ei.INIT_W, ei.INIT_H, fast=fast)
    ei.check_init_rule("fast %d" % fast, lambda pm, ws: oracle.search_for_initialization(F1, F2, pm, ws, 0.9, True), k1)

@pytest.mark.parametrize("fast", BUILDS)
def test_search_for_initialization_special_keypoints(oracle, fast):
    (k1, d1), (k2, d2) = init_frames(oracle)
    W, H = ei.INIT_W, ei.INIT_H
    F1 = oracle.Frame(k1, d1, W, H, fast=fast)
    pm = np.stack([k1["x"], k1["y"]], axis=1)
    run = lambda k, d: oracle.search_for_initialization(F1, oracle.Frame(k, d, W, H, fast=fast), pm, 100, 0.9, True)[:2]
    ei.check_init_keypoints_rule("fast %d" % fast, run, k1, d1, k2, d2)

@pytest.mark.parametrize("fast", BUILDS)
def test_projection_matchers_fed_by_the_caller(oracle, fast):
    (k1, d1), (k2, d2) = init_frames(oracle)
    W, H = ei.INIT_W, ei.INIT_H
    cur, last = oracle.Frame(k2, d2, W, H, fast=fast), oracle.Frame(k1, d1, W, H, fast=fast)
    runs = projection_runs(oracle,
                           lambda valid, uv, d, obs, slots, th, ls: oracle.search_by_projection_last(cur, last, valid, uv, d, obs, slots, th, ls, 0, True),
                           lambda kk, valid, uv, lvl, ls, d, slots, th: oracle.search_by_projection_kf(cur, kk, None, valid, uv, lvl, ls, d, slots, th, 100, True),
                           lambda valid, uv, lvl, vc, d, obs, slots, th, ls: oracle.search_by_projection_map(cur, valid, uv, lvl, vc, d, obs, slots, th, 0.8, ls),
                           k1, d1, k2, len(k2))
    for name, (run, factor) in runs.items():
        ei.check_projection_rule("%s fast %d" % (name, fast), run, projection_uv(k1), np.ones(len(k1), np.float32), cur.gb, 15.0 if factor == 1.0 else 6.0, factor)
        with pytest.raises(AssertionError, match="no query with a whole-grid area"):
            ei.check_projection_rule("%s fast %d" % (name, fast), run, projection_uv(k1), np.ones(len(k1), np.float32), cur.gb,
                                     15.0 if factor == 1.0 else 6.0, factor, wrong="saturate")

@pytest.mark.parametrize("fast", BUILDS)
def test_tracked_keypoints_edges(oracle, fast):
    img, kps = tracked_scene(oracle)
    ext = oracle.OrbExtractor(300, 1.2, 3, 10, 0, edgeTh=19, imWidth=ei.INIT_W, fast=fast)
    describe = lambda k: ext.tracked_descriptors(img, k)
    assign = lambda ref, k: ext.assign_level_by_best_desc(img, ref, k)
    ei.check_tracked_rule("fast %d" % fast, describe, assign, kps)
    with pytest.raises(AssertionError, match="have taps"):
        ei.check_tracked_rule("fast %d" % fast, describe, assign, kps, wrong="saturate")

@pytest.mark.parametrize("fast", BUILDS)
def test_search_by_projection_last_thresholds(oracle, fast):
    k1, d1, k2, d2, valid, uv, mp_obs, cur_mp, ls = proj_last_args(oracle)
    W, H = ei.INIT_W, ei.INIT_H
    cur, last = oracle.Frame(k2, d2, W, H, fast=fast), oracle.Frame(k1, d1, W, H, fast=fast)
    run = lambda th: oracle.search_by_projection_last(cur, last, valid, uv, d1, mp_obs, cur_mp, th, ls, 0, True) + (cur_mp,)
    ei.check_proj_th_rule("fast %d" % fast, run, uv, cur.gb)
    with pytest.raises(AssertionError, match="every query sees keypoints"):      # saturating: inf and 1e12 search the whole grid
        ei.check_proj_th_rule("fast %d" % fast, run, uv, cur.gb, wrong="saturate")

@pytest.mark.parametrize("sigma", [False, True])
@pytest.mark.parametrize("kind", ["queries", "keypoints"])
def test_radius_search_edges(oracle, kind, sigma):
    gb = oracle.grid_bounds(ei.INIT_W, ei.INIT_H)
    run = lambda k, d, *q: oracle.kf_radius_match(oracle.Frame(k, d, ei.INIT_W, ei.INIT_H), *q, inv_sigma2=ei.INV_SIGMA2 if sigma else None)
    ei.check_radius_rule("oracle", run, kind, gb, sigma)
    if kind == "queries":
        with pytest.raises(AssertionError, match="differ from the rule"):       # saturating: inf and 1e12 search the whole grid
            ei.check_radius_rule("oracle", run, kind, gb, sigma, wrong="saturate")
    else:
        # a keypoint at NaN lands in cell 0 under the saturating conversion, but |dx| < r is false for it: on this path no output can
        # tell the conversions apart, which is why the kernels are held to the rule by construction (dev_round_index) and not by a case
        ei.check_radius_rule("oracle", run, kind, gb, sigma, wrong="saturate")

def test_fuse_and_sim3_expectations():
    """the thresholds' effect by the rule: an ordinary th finds the ordinary queries, 0 / -1 / NaN / inf / 1e12 / 2^31 cells nothing;
    a keypoint outside the grid is nobody's mutual match"""
    class GB: minX, minY, invW, invH = 0.0, 0.0, ei.GRID_COLS / ei.INIT_W, ei.GRID_ROWS / ei.INIT_H
    s = ei.radius_scene("queries")
    assert (fuse_expected(GB, 3.0)[~s["special"]] >= 0).all()
    for name, th in ei.PROJ_TH:
        assert (fuse_expected(GB, th) == -1).all(), name
    assert (fuse_expected(GB, ei.INF, wrong="saturate") >= 0).any()
    k = ei.radius_scene("keypoints")["kps"]
    n, m12, _ = sim3_expected(GB, 7.5)
    outside = np.array([ei.pos_in_grid(x, y, GB) is None for x, y in zip(k["x"], k["y"])])
    assert n == int((~outside).sum()) and (m12[outside] == -1).all() and (m12[~outside] == np.flatnonzero(~outside)).all() and outside.sum() >= 40

# ---------------------------------------------------------------------------------------------------
# family 6: the projection restatement (tests/proj_ref) at degenerate map points, by hand
def test_frustum_restatement_edges():
    import proj_ref
    def frustum(kw, pos, normal, mind, maxd):
        return proj_ref.frustum(proj_ref.view(**kw), pos, normal, mind, maxd)[1][0]
    ei.check_frustum_rule("proj_ref", frustum)
    assert ei.predict_scale_rule(10.0, 0.0, 8, 0.18, "saturate")[0] == 7
    with pytest.raises(AssertionError, match="PredictScale of an infinite ratio 7"):      # ceil(inf) saturated to INT_MAX: the top level
        ei.check_frustum_rule("proj_ref", frustum, wrong="saturate")

def test_degenerate_images(oracle):
    check_degenerate_images(oracle.cv_normalize_minmax_u8, oracle.measure_image_focus)
    with pytest.raises(AssertionError):
        op.check_focus("single patch", oracle.measure_image_focus(ei.degenerate_images()["single_patch"]), ei.degenerate_images()["single_patch"], "sample")
