"""The oracle's ComputeStereoMatches, bf_knn2 with Lowe's test, hamming_window_match, ComputeDistinctiveDescriptors and the response
sort against the plain models of tests/helper_models.py on the planted scenes of tests/helper_scenes.py: integers and bit patterns, no
tolerance.  And the scenes themselves: every wrong variant of a model is told from the rule by a named scene (those that no reachable
input can tell apart are listed with the reason and an exhaustive check of it), and the probe counts of the planted sites are
non-zero.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import helper_models as hm
import helper_scenes as hs

F = np.float32


def same_stereo(a, b):
    """(uRight, depth, n) as bit patterns"""
    return a[2] == b[2] and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ---- ComputeStereoMatches ------------------------------------------------------------------------------------------------------------
# the scene that tells each wrong variant from the rule.  `planted_*` are the hand-set keypoints (oracle only); every variant that
# has an image-built scene names that one, so that tests/test_gpu_helper_models.py exposes the kernels to the same comparison.
STEREO_REJECTED_BY = {
    "band_exclusive": ["down_2", "planted_moved"], "band_round": ["down_3", "planted_moved"], "octave_strict": ["noisy", "planted_moved"],
    "u_strict": ["moved_minu", "moved_maxd_6"], "desc_tie_last": ["ties", "planted_moved"], "th_orb_le": ["down_3", "planted_moved"],
    "level_round_half_even": ["halves", "planted_moved"], "sad_tie_last": ["ties", "planted_moved"], "inc_edge_keep": ["mixed", "planted_moved"],
    "disp_zero_rejected": ["mixed", "identical", "mirror"], "disp_le_max": ["moved_maxd_6_noisy", "moved_maxd_6"], "median_lower": ["moved_minu", "down_3"],
    "cut_gt": ["identical", "planted_cut"],
}
STEREO_INDISTINGUISHABLE = {
    "zero_branch_float": "(float)((double)uL - 0.01) and uL - 0.01f are the same float for every float32 uL in [1, 2^24): uL lies on its binade's "
                         "grid, so which way uL - 0.01 rounds depends on the binade and 0.01 alone, and in none of them does a rounding "
                         "boundary fall into the 2.2e-10 between 0.01 and 0.01f (test_zero_branch_float_is_the_same_float)",
    "th_double": "for every median an 11 x 11 patch can give (0 .. 30 855) no integer norm lies on different sides of 2.1f * median in "
                 "float and of (float)(1.5 * 1.4 * median) (test_th_double_cuts_the_same_norms)",
}


def planted(oracle, name, fast=False):
    if name == "planted_moved":
        return hs.planted_moved(oracle, fast)[0], 1.0, hs.PLANTED_MBF
    return hs.planted_cut(oracle, fast)[0], 1.0, hs.PLANTED_MBF


def stereo_run(oracle, name, wrong=None):
    if name.startswith("planted"):
        I, mb, mbf = planted(oracle, name)
        return I.model(mb, mbf, wrong)
    return hs.stereo_model(oracle, name, wrong)


@pytest.mark.parametrize("name", list(hs.STEREO_PAIRS))
def test_stereo_oracle_equals_model(oracle, name):
    want = hs.stereo_model(oracle, name)
    for fast in (False, True):
        I, mb, mbf, sites = hs.stereo_case(oracle, name, fast)
        assert same_stereo(I.oracle(mb, mbf), want), "%s fast=%d" % (name, fast)
    P = want[3]
    assert all(P[s] > 0 for s in sites), {s: P[s] for s in sites}


def test_stereo_scene_properties(oracle):
    """what the named pairs are for, beyond their probe sites"""
    for name in ("identical", "mirror", "moved_maxd_6", "moved_maxd_6p5"):      # median 0: `0 < 0` is false, every match is taken back
        ur, dp, n, P = hs.stereo_model(oracle, name)
        assert n > 100 and P["median"] == 0 and P["thDist"] == 0.0 and P["kept"] == 0 and np.all(ur == -1) and np.all(dp == -1), name
    ur, dp, n, P = hs.stereo_model(oracle, "mixed")                              # the 0.01 branch's value in a final uRight / depth
    I, mb, mbf, _ = hs.stereo_case(oracle, "mixed")
    z = np.flatnonzero(dp.view(np.uint32) == np.array(F(mbf) / F(0.01), F).view(np.uint32))
    assert P["median"] > 0 and len(z) == P["zero_branch_kept"] >= 1
    assert np.array_equal(ur[z].view(np.uint32), (I.kL["x"][z].astype(np.float64) - 0.01).astype(F).view(np.uint32))
    assert hs.stereo_model(oracle, "moved_maxd_6")[3]["disp_ge_maxD"] > 50 and hs.stereo_model(oracle, "moved_minu")[3]["kept"] > 50
    kept = [hs.stereo_model(oracle, "down_%d" % d)[2] for d in (2, 3, 4)]
    assert kept[0] > kept[1] > kept[2] > 100, kept                              # the row band lets fewer through, row by row
    for name, empty in (("flat_right", "kR"), ("flat_left", "kL")):
        assert len(getattr(hs.stereo_inputs(oracle, name), empty)) == 0
    I = hs.stereo_inputs(oracle, "no_match")
    assert len(I.kL) > 100 and len(I.kR) > 100 and hs.stereo_model(oracle, "no_match")[2] == 0
    # `disparity < maxD` and `disparity >= minD` show in the output VALUES, not only in the accepted count, where the median is > 0
    for name, wrong in (("moved_maxd_6_noisy", "disp_le_max"), ("mixed", "disp_zero_rejected")):
        m, w = hs.stereo_model(oracle, name), hs.stereo_model(oracle, name, wrong)
        assert m[3]["median"] > 0 and not np.array_equal(m[0].view(np.uint32), w[0].view(np.uint32)), (name, wrong)
    I = hs.stereo_inputs(oracle, "noisy")
    assert len(I.kL) % 4 != 0 and len(I.kR) % 64 != 0 and len(I.kR) > 64, (len(I.kL), len(I.kR))
    assert hs.stereo_model(oracle, "noisy")[3]["median"] > 0


def test_stereo_planted_keypoints(oracle):
    I, site, want = hs.planted_moved(oracle)
    m = I.model(1.0, hs.PLANTED_MBF)
    for fast in (False, True):
        J = hs.planted_moved(oracle, fast)[0]
        assert same_stereo(J.oracle(1.0, hs.PLANTED_MBF), m), fast
    for name, (verdict, why) in want.items():
        if verdict != "any":
            assert (m[0][site[name]] != -1) == (verdict == "accepted"), (name, why, m[0][site[name]])
    P = m[3]
    for s in ("scaled_half", "iniu_endu_rejected", "patch_outside", "row_outside", "band_row_outside", "band_hi_integer_l0", "band_lo_integer_l0",
              "band_hi_integer_l1", "band_lo_integer_l1", "row_eq_minr", "row_eq_maxr", "row_above_maxr", "row_below_minr", "octave_diff_1", "octave_diff_2", "best_dist_74",
              "best_dist_75", "best_dist_99", "best_dist_100", "desc_tie_across_64", "best_shift_4", "best_shift_edge", "sad_tie"):
        assert P[s] > 0, s
    assert P["median"] > 0 and P["delta_rejected"] == 0
    # the tie at iR = 3 / 67 went to the lower index: the partner 6 px away, not the one 26 px away
    assert abs(float(I.kL["x"][site["tie_3_67"]] - m[0][site["tie_3_67"]]) - 6.0) < 0.6


def test_stereo_planted_cut(oracle):
    """nine hand-set norms; 2.1f * 10 is exactly 21.0f, so a norm EQUAL to thDist exists and is taken back"""
    I, site, norms = hs.planted_cut(oracle)
    m = I.model(1.0, hs.PLANTED_MBF)
    for fast in (False, True):
        assert same_stereo(hs.planted_cut(oracle, fast)[0].oracle(1.0, hs.PLANTED_MBF), m), fast
    P = m[3]
    assert m[2] == 9 and P["median"] == 10 and P["thDist"] == 21.0 and P["n_eq_thDist"] == 1 and P["n_within_1_of_thDist"] == 3
    assert [bool(m[0][site["norm_%d" % n]] != -1) for n in norms] == [n < 21 for n in norms]


@pytest.mark.parametrize("wrong", list(STEREO_REJECTED_BY))
def test_stereo_wrong_variant_is_rejected(oracle, wrong):
    for name in STEREO_REJECTED_BY[wrong]:
        assert not same_stereo(stereo_run(oracle, name, wrong), stereo_run(oracle, name)), "%s passes on %s" % (wrong, name)


def test_stereo_every_variant_is_accounted_for():
    assert set(STEREO_REJECTED_BY) | set(STEREO_INDISTINGUISHABLE) == set(hm.STEREO_WRONG)
    assert not set(STEREO_REJECTED_BY) & set(STEREO_INDISTINGUISHABLE)
    image_built = {w for w, names in STEREO_REJECTED_BY.items() if any(not n.startswith("planted") for n in names)}
    assert image_built == set(STEREO_REJECTED_BY)                              # the kernels see every distinguishable comparison too


def test_zero_branch_float_is_the_same_float():
    """every float32 in [1, 2^24): all 2^23 of each binade"""
    for e in range(0, 24):
        u = (np.array(2.0 ** e, F).view(np.uint32) + np.arange(2 ** 23, dtype=np.uint32)).view(F)
        assert np.array_equal((u.astype(np.float64) - 0.01).astype(F), u - F(0.01)), e


def test_th_double_cuts_the_same_norms():
    m = np.arange(0, 121 * 255 + 1)
    a = (F(F(1.5) * F(1.4)) * m.astype(F)).astype(np.float64); b = (1.5 * 1.4 * m.astype(np.float64)).astype(F).astype(np.float64)
    assert (a != b).sum() > 1000                                               # the two thresholds do differ ...
    assert not np.any(np.ceil(np.minimum(a, b)) < np.maximum(a, b))            # ... but no integer n has n < a and not n < b, or the reverse


# ---- knn2 and Lowe's test ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", hs.KNN_NQ)
def test_knn2_oracle_equals_model(oracle, nq):
    for nt in hs.KNN_NT:
        q, t = hs.knn_scene(nq, nt)
        idx, dist = hm.knn2(q, t)
        for fast in (False, True):
            oi, od = oracle.bf_knn2(q.reshape(-1, 32), t.reshape(-1, 32), fast)
            assert np.array_equal(oi, idx) and np.array_equal(od, dist), (nq, nt, fast)
        if nt > 69 and (nq > 1 or (nq == 1 and nt <= 256)):
            assert idx[0].tolist() == [5, 21] and dist[0].tolist() == [2, 2]                      # the first query: rows 5 / 21 / 37 / 69 tie
        if nq and nt > 256:
            assert idx[nq - 1].tolist() == [255, 256] and dist[nq - 1].tolist() == [3, 3]         # the last one: a tie across the tile
        if nq > 1 and nt == 300:
            assert idx[1].tolist() == [299, 0] and dist[1].tolist() == [0, 3]                     # best in the last tile, second in the first
        if nt == 1 and nq:
            assert np.all(idx[:, 1] == -1) and np.all(dist[:, 1] == 0x7fffffff) and np.all(idx[:, 0] == 0)
        if nt == 0:
            assert np.all(idx == -1) and np.all(dist == 0x7fffffff)
        if nq and nt >= 2:
            wi, wd = hm.knn2(q, t, "tie_last")
            assert np.array_equal(wd, dist)
            assert (not np.array_equal(wi, idx)) == (nt > 69), (nq, nt)                           # told apart wherever a tie is planted


LOWE_PAIRS = [(0, 0), (0, 1), (1, 1), (6, 10), (7, 10), (8, 10), (14, 20), (13, 20), (21, 30), (28, 40), (35, 50), (42, 60), (49, 70), (48, 70)]
LOWE_PAIRS_ALONE = [(63, 90), (70, 100), (69, 100), (119, 170), (126, 180), (175, 250), (176, 250), (256, 256)]    # (random rows are nearer)


def a_lt_b(d0, d1):
    """Lowe's test in exact arithmetic where the double product is exact or falls on the same side; (119, 170) and (126, 180) are where
    170 * 0.7 and 180 * 0.7 in double fall just BELOW 119 and 126, as the exact products do not: equality either way, rejected"""
    return int(10 * d0 < 7 * d1)


def lowe_scene(mono_left, mono_right):
    """left rows whose two nearest right rows are at the distances LOWE_PAIRS; mono_* rows outside the lapping area lead both sets"""
    rng = np.random.default_rng(31)
    L = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(mono_left)]
    R = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(mono_right)]
    for d0, d1 in LOWE_PAIRS:
        q = rng.integers(0, 256, 32, dtype=np.uint8)
        L.append(q); R.append(hs._flip(q, d1, 128 - d1 // 2 if d1 > 120 else 128)); R.append(hs._flip(q, d0, 0))
    return np.array(L, np.uint8), np.array(R, np.uint8)


@pytest.mark.parametrize("mono", [(0, 0), (3, 5)])
def test_lowe_oracle_equals_model(oracle, mono):
    dL, dR = lowe_scene(*mono)
    idx, dist = hm.knn2(dL[mono[0]:], dR[mono[1]:])
    pairs = LOWE_PAIRS
    assert [tuple(d) for d in dist.tolist()] == pairs                          # the scene plants what it says
    cand, n = hm.lowe(idx, dist, *mono)
    for fast in (False, True):
        on, oc, od = oracle.fisheye_matches(dL, mono[0], dR, mono[1], fast)
        assert on == n and oc[mono[0]:].tolist() == cand and np.all(oc[:mono[0]] == -1)
        assert np.array_equal(od[mono[0]:], dist) and np.all(od[:mono[0]] == -1)
    want = [10 * a < 7 * b for a, b in pairs]                                  # on these pairs the double product agrees with the integers
    assert [c >= 0 for c in cand] == want
    assert hm.lowe(idx, dist, *mono, wrong="ratio_le")[0] != cand
    assert sum(10 * a == 7 * b for a, b in pairs) >= 5
    for d0, d1 in LOWE_PAIRS_ALONE:                                            # a left row and its two right rows alone
        q = dL[-1]; R = np.array([hs._flip(q, d1, 0), hs._flip(q, d0, 256 - d0)])
        i2, d2 = hm.knn2(q[None], R)
        assert tuple(d2[0].tolist()) == (d0, d1)
        c, n = hm.lowe(i2, d2, 0, 0)
        on, oc, od = oracle.fisheye_matches(q[None], 0, R, 0)
        assert (on, oc.tolist()) == (n, c) and np.array_equal(od, d2) and n == (a_lt_b(d0, d1)), (d0, d1)
    # one right row in the lapping area: size() < 2, no candidate
    on, oc, od = oracle.fisheye_matches(dL, mono[0], dR[:mono[1] + 1], mono[1])
    i1, d1 = hm.knn2(dL[mono[0]:], dR[mono[1]:mono[1] + 1])
    assert on == 0 and hm.lowe(i1, d1, *mono)[1] == 0 and np.array_equal(od[mono[0]:, 0], d1[:, 0]) and np.all(od[:, 1] == -1)


def test_lowe_ratio_float_cannot_be_told():
    """LOWE_INDISTINGUISHABLE: `ratio_float` (d1 * 0.7f in float) decides every pair of Hamming distances 0 .. 256 as the rule does"""
    for d1 in range(257):
        idx = [[0, 1]] * (d1 + 1); dist = [[d0, d1] for d0 in range(d1 + 1)]
        assert hm.lowe(idx, dist, 0, 0) == hm.lowe(idx, dist, 0, 0, wrong="ratio_float"), d1
    assert set(hm.LOWE_WRONG) == {"ratio_le", "ratio_float"}


# ---- window_match ------------------------------------------------------------------------------------------------------------------
def oracle_window_strided(oracle, q, qs, t, ts, offs, cand, lead):
    """orc_hamming_window_match through the raw C ABI, the rows qs / ts bytes apart and the first one `lead` bytes into its buffer"""
    qb, tb = hs.strided(q, qs, lead), hs.strided(t, ts, lead)
    nq = len(q)
    out = [np.zeros(max(nq, 1), np.int32) for _ in range(4)]
    L = oracle.lib(); L.orc_hamming_window_match.restype = None
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L.orc_hamming_window_match(C.c_void_p(qb.ctypes.data + lead), C.c_int(nq), C.c_int(qs), C.c_void_p(tb.ctypes.data + lead), C.c_int(ts),
                               p(offs), p(cand), *[p(o) for o in out])
    return tuple(o[:nq] for o in out)


def test_window_match_oracle_equals_model(oracle):
    q, t, offs, cand, sites = hs.window_scene()
    want = hm.window_match(q, t, offs, cand)
    got = oracle.hamming_window_match(q, t, offs, cand)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    for qs, ts, lead in ((32, 61, 0), (61, 32, 3), (61, 61, 1), (33, 40, 7), (32, 32, 5)):
        got = oracle_window_strided(oracle, q, qs, t, ts, offs, cand, lead)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (qs, ts, lead)
    bi, bd, si, sd = want
    for n in hs.WINDOW_LENGTHS:
        k = sites[(n, "tie_p_p64")]
        if n >= 2: assert (bi[k], bd[k], si[k], sd[k]) == (0, 4, 1, 4), n       # equal distances at p / p + 64 (p / p + 1): the first is best
        k = sites[(n, "same_index_twice")]
        if n >= 2: assert (bi[k], bd[k], si[k], sd[k]) == (2, 6, 2, 6), n
        k = sites[(n, "tie_for_second")]
        if n >= 3: assert (bi[k], bd[k], si[k], sd[k]) == (6, 2, 4, 9), n
        k = sites[(n, "best_last")]
        if n >= 2: assert (bi[k], bd[k], si[k], sd[k]) == (6, 2, 7, 3), n
        k = sites[(n, "random")]
        if n == 0: assert (bi[k], bd[k], si[k], sd[k]) == (-1, 256, -1, 256)
        if n == 1: assert bi[k] >= 0 and (si[k], sd[k]) == (-1, 256)
    for wrong in hm.WINDOW_WRONG:
        w = hm.window_match(q, t, offs, cand, wrong)
        assert not all(np.array_equal(a, b) for a, b in zip(w, want)), wrong


# ---- distinctive -------------------------------------------------------------------------------------------------------------------
def test_distinctive_oracle_equals_model(oracle):
    desc, offs, names = hs.distinctive_scene()
    want = hm.distinctive(desc, offs)
    assert oracle.distinctive_descriptors(desc, offs).tolist() == want
    by = dict(zip(names, want))
    assert all(by[n] == -1 for n in names if n.startswith("empty")) and all(by["N%d_identical" % N] == 0 for N in hs.DISTINCTIVE_N)
    assert by["equal_medians"] == 0 and by["equal_medians_swapped"] == 0 and by["even_truncates_4"] == 0 and by["even_truncates_6"] == 1
    assert len({by["N%d_random" % N] for N in hs.DISTINCTIVE_N}) > 5
    rejected = {w: [n for n, a, b in zip(names, hm.distinctive(desc, offs, w), want) if a != b] for w in hm.DISTINCTIVE_WRONG}
    assert "even_truncates_4" in rejected["median_upper"] and "even_truncates_6" in rejected["median_upper"]
    assert "equal_medians" in rejected["first_tie_last"] and "N64_identical" in rejected["first_tie_last"]


# ---- sort_by_response --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", hs.SORT_N)
def test_sort_by_response_oracle_equals_model(oracle, n):
    k = hs.response_keypoints(oracle.KP_DTYPE, n)
    want = hm.sort_by_response(k["response"])
    assert oracle.sort_by_response(k).tolist() == want
    r = k["response"][want]
    assert np.all(r[:-1] >= r[1:]) and sorted(want) == list(range(n))
    if n >= 2:
        z = [i for i in want if k["response"][i] == 0]                          # 0.0 and -0.0 are one run, in index order
        assert z == sorted(z) and z[0] == 0 and z[-1] == n - 1
        assert hm.sort_by_response(k["response"], "unstable_reverse") != want
