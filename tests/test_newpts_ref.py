"""The CPU restatement of CreateNewMapPoints' per-match half (tests/newpts_ref/newpts_ref.c, the sequential double loop of
src/LocalMapping.cc:527-784 and src/Tracking.cc:3232-3408) held to three things written independently of it: the same arithmetic a
second time in numpy scalars with the loop in plain Python (exactly), every named wrong variant of that model (each rejected by a
named scene), the parallel resolution of the two sequential rules written in numpy over per-pair results (what the device does), and one
pair in float64 with numpy's SVD (decisions, and the triangulated point within a measured bound).  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newpts_ref as nr                     # noqa: E402
from newpts_ref import scenes              # noqa: E402

S = nr.S
KEYS = ("status", "x3d", "branch", "cos_parallax", "n_new")


@pytest.fixture(scope="module")
def all_scenes():
    return scenes.all_scenes()


@pytest.fixture(scope="module")
def loops(all_scenes):
    """the restatement on every scene, computed once"""
    return {name: nr.loop(sc) for name, sc in all_scenes.items()}


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in KEYS)


def test_restatement_equals_the_python_model_on_every_scene(all_scenes, loops):
    for name, sc in all_scenes.items():
        m = nr.loop_model(sc)
        for k in KEYS:
            assert np.array_equal(np.ascontiguousarray(loops[name][k]).view(np.uint8), np.ascontiguousarray(m[k]).view(np.uint8)), (name, k)


def test_every_exit_is_reached(all_scenes, loops):
    """the probe: how often each scene reaches each exit.  w_zero is reached by no planted input: vt.row(3) of the Jacobi SVD has a last
    component of exactly 0 only for a point at infinity whose rotations leave an exact zero, and none of the constructions tried gave one
    (DESIGN.md section 2 says so); every other exit is reached, each form reaches its own set, and the DLT and both UnprojectStereo
    branches are taken"""
    total = np.zeros(len(nr.STATUS), np.int64); branches = np.zeros(4, np.int64)
    for name in all_scenes:
        total += np.bincount(loops[name]["status"].ravel(), minlength=len(nr.STATUS))
        branches += np.bincount(loops[name]["branch"].ravel(), minlength=4)
    missing = [n for n, c in zip(nr.STATUS, total) if c == 0]
    assert missing == ["w_zero"], (missing, dict(zip(nr.STATUS, total)))
    assert np.all(branches[1:] > 0), branches
    # the two-camera scene reaches all four pose choices
    sc = all_scenes["twocam"]
    seen = set()
    for k, i in np.argwhere(loops["twocam"]["status"] == S["new"]):
        seen.add((bool(i >= sc["nleft1"]), bool(sc["match12"][k, i] >= sc["nleft2"][k])))
    assert seen == {(False, False), (False, True), (True, False), (True, True)}, seen
    assert {len(v["cam"]) for vs in sc["views2"] for v in vs} == {4, 8}          # a Pinhole and a KannalaBrandt8 mpCamera2


def test_claim_scene_holds_its_cases(all_scenes, loops):
    sc, r = all_scenes["claim"], loops["claim"]
    st = r["status"]
    first_at_1 = [i for i in range(sc["n1"]) if st[0, i] not in (S["new"], S["no_match"]) and st[1, i] == S["new"] and st[2, i] == S["claimed"]]
    assert first_at_1, "no idx1 matched in neighbours 0, 1 and 2 that is accepted first at 1"
    m0 = sc["match12"][0]
    twins = [(a, b) for a in range(sc["n1"]) for b in range(a + 1, sc["n1"]) if m0[a] >= 0 and m0[a] == m0[b] and st[0, a] == S["new"] and st[0, b] == S["new"]]
    assert twins, "no two idx1 on one idx2 that are both reported as new"
    assert r["n_new"].tolist() == [(st[k] == S["new"]).sum() for k in range(sc["K"])]


def test_mixed_scene_switches_the_factor_inside_neighbour_1(all_scenes, loops):
    sc = all_scenes["mixed"]
    st, ak, _ = nr.pairs(sc)
    pos = np.arange(sc["K"] * sc["n1"]).reshape(sc["K"], sc["n1"])
    pstar = pos[ak.astype(bool)].min()
    assert sc["n1"] + sc["n1"] // 2 <= pstar < 2 * sc["n1"], pstar
    # a non-ORB idx1 matched in neighbour 0 leaves at the type gate and does not switch the factor
    o1 = sc["side1"]["kp_is_orb"]
    assert any(not o1[i] and sc["match12"][0, i] >= 0 for i in range(sc["n1"]))
    assert np.all(loops["mixed"]["status"][0][(sc["match12"][0] >= 0) & (o1 == 0)] == S["type"])
    # the switch decides pairs: some pair is accepted under one factor only, on either side of p*
    differs = st[..., 0] != st[..., 1]
    assert differs[pos < pstar].any() and differs[pos >= pstar].any()


# variant -> the scene that rejects it (the model with the variant gives other results than the model without, which equals the restatement)
REJECTED_BY = {
    "parallax_le_float": "sides_parallax_b",       # cosParallaxRays == 0.9998f, the float above the double 0.9998
    "cos_ge_0": "exact",                           # pair 12: cosParallaxRays == 0
    "z1_lt": "exact",                              # pair 14: z1 == 0
    "z2_lt": "exact",                              # pair 9: z2 == 0
    "chi1_ge": "exact",                            # pair 1: error 0 against 7.8 * 0
    "chi2_ge": "exact",                            # pair 2: error 0 against 5.991 * 0
    "far_gt": "exact_far_on",                      # dist2 == mThFarPoints
    "scale_low_le": "exact",                       # pair 3: ratioDist*ratioFactor == ratioOctave
    "scale_high_ge": "exact",                      # pair 5: ratioDist == ratioOctave*ratioFactor
    "stereo_two_ifs": "stereo",                    # both keypoints have a right coordinate
    "mbf2_repaired": "stereo",                     # the neighbours' mbf differ from pKF1's
    "ratio_reset_per_neighbour": "mixed",
    "ratio_reset_per_pair": "mixed",
    "claim_ignored": "claim",
    "unproject_stereo_undistorted": "stereo",      # mvKeys differ from the undistorted keys by up to 2 px
}


def test_variant_table_is_complete():
    assert sorted(REJECTED_BY) == sorted(nr.VARIANTS)


@pytest.mark.parametrize("variant", nr.VARIANTS)
def test_wrong_variant_is_rejected(all_scenes, loops, variant):
    name = REJECTED_BY[variant]
    sc = all_scenes[name]
    good = nr.loop_model(sc)
    assert _same(good, loops[name])
    bad = nr.loop_model(sc, variant)
    assert not _same(bad, good), "%s gives the reference's results on scene %s" % (variant, name)


def test_sides_are_adjacent_floats_with_different_exits(all_scenes, loops):
    """the comparisons that no exact construction reaches: the two scenes of a pair differ in one input by one float step and take
    different exits"""
    for name, (a, b, what) in scenes.sides_scenes().items():
        lo, hi = np.float32(what[2]), np.float32(what[3])
        assert np.nextafter(lo, np.float32(np.inf)) == hi, (name, lo, hi)
        ra, rb = nr.loop(a), nr.loop(b)
        assert not np.array_equal(ra["status"], rb["status"]), name
        assert (ra["status"] != rb["status"]).sum() == 1, name
    what = scenes.sides_scenes()["parallax"][2]
    i2 = what[4]
    assert loops["sides_parallax_b"]["cos_parallax"][0, i2] == np.float32(0.9998) and loops["sides_parallax_b"]["status"][0, i2] == S["parallax"]
    assert loops["sides_parallax_a"]["cos_parallax"][0, i2] == np.nextafter(np.float32(0.9998), np.float32(0))
    assert loops["sides_parallax_a"]["branch"][0, i2] == 1
    assert np.float64(np.float32(0.9998)) > 0.9998          # no float equals the double: "<" and "<=" against it agree everywhere


# ---- the parallel resolution of the two sequential rules, over per-pair results ------------------------------------------------------
def resolve(st, ak):
    """st (K, n1, 2): each pair's exit under the ORB / the AKAZE factor; ak (K, n1): an AKAZE-AKAZE pair.  -> (status (K, n1), p*)"""
    K, n1 = ak.shape
    pos = np.arange(K * n1).reshape(K, n1)
    acc_orb = st[..., 0] == S["new"]
    earlier_orb = (np.cumsum(acc_orb, axis=0) - acc_orb) > 0          # an accepted-under-the-ORB-factor pair at a smaller k
    cand = ak.astype(bool) & ~earlier_orb
    pstar = int(pos[cand].min()) if cand.any() else K * n1
    eff = np.where(pos < pstar, st[..., 0], st[..., 1])
    acc = eff == S["new"]
    claimed = ((np.cumsum(acc, axis=0) - acc) > 0) & (eff != S["no_match"])
    return np.where(claimed, S["claimed"], eff).astype(np.uint8), pstar


def _check_resolution(sc, r):
    st, ak, x = nr.pairs(sc)
    status, pstar = resolve(st, ak)
    assert np.array_equal(status, r["status"]), sc["name"]
    new = status == S["new"]
    assert np.array_equal(np.where(new[..., None], x, 0).view(np.uint8), r["x3d"].view(np.uint8)), sc["name"]
    assert np.array_equal(new.sum(axis=1), r["n_new"]), sc["name"]
    # the position where the factor switches is simply the smallest position of an AKAZE-AKAZE pair: the pair that claimed a non-ORB
    # idx1 passed the type gate, so it is such a pair at a smaller position (what the device relies on)
    pos = np.arange(ak.size).reshape(ak.shape)
    assert pstar == (int(pos[ak.astype(bool)].min()) if ak.any() else ak.size), sc["name"]


def test_parallel_resolution_equals_the_loop_on_every_scene(all_scenes, loops):
    for name, sc in all_scenes.items():
        _check_resolution(sc, loops[name])


@pytest.mark.parametrize("seed", range(100, 112))
def test_parallel_resolution_on_random_mixed_sets(seed):
    rng = np.random.default_rng(seed)
    sc = scenes.random_scene("mixed_%d" % seed, seed, K=int(rng.integers(1, 5)), n1=48, n2=48, mixed=True, wrong=0.1)
    sc["rf_orb"] = np.float32(rng.uniform(1.0, 1.3)); sc["rf_ak"] = np.float32(rng.uniform(1.3, 2.5))
    if seed % 3 == 0:
        sc["side1"]["kp_is_orb"][:] = 1; sc["side1"]["kp_is_orb"][rng.integers(0, 48, 3)] = 0      # a late, rare switch
    _check_resolution(sc, nr.loop(sc))


# ---- against float64 ------------------------------------------------------------------------------------------------------------------
EXACT = ("exact", "exact_tracking", "exact_far_on", "exact_far_above", "zero_dist")
RANDOM = ("mono", "mono_k1", "mono_tracking", "kb8", "stereo", "stereo_tracking", "twocam", "claim")
# the largest relative deviation |x3d - x3d_f64| / |x3d_f64| of the restatement over the pairs of RANDOM that both sides accept, measured on
# an x86-64 host with gcc -O2 -ffp-contract=off: a float Jacobi SVD against LAPACK on the scenes' conditioning (rays a few hundredths of a
# radian apart at the far end).  The bound is 4 times that.
X3D_MEASURED = 4.2e-6
X3D_BOUND = 4 * X3D_MEASURED


def _f64_compare(sc):
    st, _, x = nr.pairs(sc)
    rows = []
    for k, i in np.argwhere(sc["match12"] >= 0):
        s64, x64, margin = nr.pair_f64(sc, int(k), int(i), int(sc["match12"][k, i]), float(sc["rf_orb"]))
        if st[k, i, 0] == S["type"]:
            continue
        rows.append((int(k), int(i), int(st[k, i, 0]), int(s64), float(margin), x[k, i], x64))
    return rows


def test_decisions_agree_with_float64_on_the_exact_scenes(all_scenes):
    """the scenes whose arithmetic is exact: every pair, none left out, although their compared quantities sit ON the thresholds"""
    for name in EXACT:
        for k, i, s32, s64, margin, _, _ in _f64_compare(all_scenes[name]):
            assert s32 == s64, (name, k, i, nr.STATUS[s32], nr.STATUS[s64])


def test_sides_straddle_the_float64_decision(all_scenes):
    """the bisected pairs sit one float apart either side of a comparison whose operands carry float rounding: float64 cannot agree with both.
    It agrees with one of them and its own margin there is far below the 1e-3 of the random scenes"""
    for name, (a, b, what) in scenes.sides_scenes().items():
        if name == "parallax":
            k, i, j = 0, what[4], what[1]
        else:
            i = next(q for q in range(a["n1"]) if nr.loop(a)["status"][0, q] != nr.loop(b)["status"][0, q]); k, j = 0, int(a["match12"][0, i])
        sa, sb = int(nr.pairs(a)[0][k, i, 0]), int(nr.pairs(b)[0][k, i, 0])
        s64a, _, ma = nr.pair_f64(a, k, i, j, float(a["rf_orb"])); s64b, _, mb = nr.pair_f64(b, k, i, j, float(b["rf_orb"]))
        assert s64a == s64b and s64a in (sa, sb), (name, sa, sb, s64a, s64b)
        assert max(ma, mb) < 1e-3, (name, ma, mb)


def test_decisions_and_points_agree_with_float64_on_the_random_scenes(all_scenes):
    worst = 0.0
    for name in RANDOM:
        rows = _f64_compare(all_scenes[name])
        left_out = 0
        for k, i, s32, s64, margin, x32, x64 in rows:
            if s32 != s64:
                assert margin < 1e-3, (name, k, i, nr.STATUS[s32], nr.STATUS[s64], margin)
                left_out += 1
                continue
            if s32 == S["new"]:
                dev = float(np.linalg.norm(x32.astype(np.float64) - x64) / np.linalg.norm(x64))
                worst = max(worst, dev)
                assert dev <= X3D_BOUND, (name, k, i, dev)
        assert left_out <= 0.05 * len(rows), (name, left_out, len(rows))
    print("largest relative deviation of x3d from float64: %.3g (recorded %.3g)" % (worst, X3D_MEASURED))
    assert worst >= X3D_MEASURED / 4, "the recorded deviation is stale: measured %.3g" % worst
