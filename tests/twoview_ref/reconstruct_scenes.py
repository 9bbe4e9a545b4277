"""Planted scenes for eorb_two_view_reconstruct, built on scenes.scene: each is made to reach one exit or one comparison outcome of
TwoViewReconstruction::Reconstruct (both forms), and `probe` reports from a result which it reached.  SCENES maps a name to
(builder, parameter overrides); tests/test_twoview_reconstruct_ref.py checks that the table of exits is covered."""
import numpy as np

from . import scenes

K = scenes.K


def _replace(sc, uv1, uv2, X, R, t):
    """put new matched coordinates into a scene's key arrays (the unmatched keys stay)"""
    m = sc["matches"]
    sc["kps1"]["x"][m[:, 0]] = uv1[:, 0]; sc["kps1"]["y"][m[:, 0]] = uv1[:, 1]
    sc["kps2"]["x"][m[:, 1]] = uv2[:, 0]; sc["kps2"]["y"][m[:, 1]] = uv2[:, 1]
    sc["X"] = X; sc["R"] = R; sc["t"] = t
    sc["X_by_first"] = np.zeros((len(sc["kps1"]), 3)); sc["X_by_first"][m[:, 0]] = X
    return sc


def moved(kind, N, seed=0, R=None, t=None, normal=(0.1, -0.15, 1.0), noise=0.3, mirror=False, window=(20, 20, scenes.W - 20, scenes.H - 20)):
    """scenes.scene's frame (keys, matches, n1 != n2) with another motion (R, t: t need not be a unit vector) and, for kind == "planar",
    another plane normal; mirror: image 2 is flipped left to right (a homography no camera motion produces); window: the part of image 1
    (x0, y0, x1, y1) the matched points are seen in"""
    sc = scenes.scene(kind, N, seed=seed, noise=noise)
    rng = np.random.default_rng(seed + 7919)
    R0, t0 = scenes.true_pose()
    R = R0 if R is None else np.asarray(R, np.float64); t = t0 if t is None else np.asarray(t, np.float64)
    uv = np.stack([rng.uniform(window[0], window[2], N), rng.uniform(window[1], window[3], N)], axis=1)
    ray = np.concatenate([(uv - [K[0, 2], K[1, 2]]) / [K[0, 0], K[1, 1]], np.ones((N, 1))], axis=1)
    z = 6.0 / (ray @ np.asarray(normal, np.float64)) if kind == "planar" else rng.uniform(3.0, 9.0, N)
    X = ray * z[:, None]
    uv1 = scenes.project(np.eye(3), np.zeros(3), X) + rng.normal(0, noise, (N, 2))
    uv2 = scenes.project(R, t, X) + rng.normal(0, noise, (N, 2))
    if mirror:
        uv2[:, 0] = scenes.W - uv2[:, 0]
    return _replace(sc, uv1, uv2, X, R, t)


def same_keys(N, seed=0):
    """every key of image 2 at one place: Normalize divides by zero, every score is NaN, no iteration wins, SH + SF == 0"""
    sc = scenes.scene("general", N, seed=seed)
    sc["kps2"]["x"] = 100.0; sc["kps2"]["y"] = 50.0
    return sc


def probe(o, p):
    """which exit of Reconstruct a result reached, and the outcome of each comparison on the way -> (exit name, dict)"""
    form = "info" if int(p.form) == 1 else "stock"
    if o["stage"] == 0:
        return form + ":SH+SF==0", {}
    if o["stage"] == 1:
        return form + ":H:d-test", {}
    f32 = np.float32
    if not o["is_homography"]:
        c = dict(few_good=bool(o["best_good"] < o["n_min_good"]), similar=bool(o["n_similar"] > 1),
                 parallax=bool(o["best_parallax"] > f32(p.min_parallax)), min_good_from=("N" if int(f32(p.th_min_good_r) * f32(o["n_inliers"])) >
                                                                                         p.min_triangulated else "min_triangulated"))
        if form == "stock":
            name = "F:reject" if (c["few_good"] or c["similar"]) else ("F:ok" if o["ok"] else "F:low-parallax")
        else:
            name = "F:ok" if o["ok"] else "F:not-ok"
        return form + ":" + name, c
    b, s = f32(o["best_good"]), f32(o["second_good"])
    c = dict(second=bool(s < f32(p.th_max_good_r_h) * b), parallax=bool(o["best_parallax"] >= f32(p.min_parallax)),
             min_triangulated=bool(o["best_good"] > p.min_triangulated), min_good_r=bool(b > f32(p.th_min_good_r) * f32(o["n_inliers"])),
             hypotheses_with_points=int((np.asarray(o["hyp_good"]) > 0).sum()))
    return form + ":" + ("H:ok" if o["ok"] else "H:not-ok"), c


_R0, _T0 = scenes.true_pose()
_SLANT = (0.6, -0.15, 1.0)          # a plane slanted enough that the second Faugeras solution loses a quarter of the points

# name -> (builder, N, iterations, seed of the sets, parameter overrides, what it is planted for)
SCENES = {
    "planar": (lambda: moved("planar", 300, seed=3, normal=_SLANT), 300, 200, 2, {}, "H chosen and accepted"),
    "general": (lambda: scenes.scene("general", 300, seed=1), 300, 200, 2, {}, "F chosen and accepted"),
    "noise": (lambda: scenes.scene("noise", 300, seed=1), 300, 200, 2, {}, "rejected: no hypothesis triangulates anything"),
    "mixed": (lambda: scenes.scene("mixed", 300, seed=1), 300, 200, 2, {}, "F accepted on the inliers of a 30 % outlier set"),
    "planar_twofold": (lambda: scenes.scene("planar", 300, seed=1), 300, 200, 2, {}, "H: the second solution keeps too many points"),
    "planar_both": (lambda: moved("planar", 300, seed=3, t=np.array([0.3, 0.1, 1.0]) / np.linalg.norm([0.3, 0.1, 1.0])), 300, 200, 2, {},
                    "H: two hypotheses hold every point, the earlier one is the best"),
    "far_general": (lambda: scenes.scene("general", 100, seed=5, far=0.6), 100, 100, 2, {}, "F: counts pass, the parallax gate decides"),
    "far_similar": (lambda: scenes.scene("general", 300, seed=5, far=0.8), 300, 200, 2, {}, "F: two hypotheses above 0.7 of the best"),
    "small_baseline": (lambda: moved("planar", 300, seed=3, normal=_SLANT, t=_T0 * 0.02), 300, 200, 2, {}, "H: the parallax gate fails"),
    "few": (lambda: scenes.scene("general", 30, seed=5), 30, 30, 2, {}, "N below min_triangulated: n_min_good decides"),
    "pure_rotation": (lambda: moved("planar", 300, seed=3, R=_R0, t=np.zeros(3), noise=0.0), 300, 200, 2, {}, "ReconstructH leaves at the d test"),
    "same_keys": (lambda: same_keys(65), 65, 9, 2, {}, "every iteration scores NaN: SH + SF == 0"),
    "tie_f_second": (lambda: moved("general", 8, seed=3, normal=_SLANT, noise=0.1), 8, 8, 3, {}, "F: counts 1, 8, 1, 0: the multimap's order of equals"),
    "tie_h_best": (lambda: moved("planar", 8, seed=2, normal=_SLANT, noise=0.1), 8, 8, 2, {}, "H: counts 8, 8, 1: strict > keeps the earlier best"),
    "tie_h_second": (lambda: moved("planar", 8, seed=1, normal=_SLANT, noise=0.1), 8, 8, 1, {}, "H: counts 8, 5, 5: strict > keeps the earlier second"),
    "n9": (lambda: moved("general", 9, seed=7, normal=_SLANT, noise=0.1), 9, 9, 7, {}, "small N"),
    "n12": (lambda: moved("planar", 12, seed=4, normal=_SLANT, noise=0.1), 12, 12, 4, {}, "small N"),
    "h_none": (lambda: scenes.scene("noise", 10, seed=10), 10, 10, 10, dict(th_hf_ratio=0.0), "H forced on noise: no hypothesis has a point (vR[-1] twice)"),
    "d_test_off": (lambda: moved("planar", 300, seed=3, R=_R0, t=np.zeros(3), noise=0.0), 300, 200, 2, dict(th_rd_homo=0.0),
                   "the d test switched off on a pure rotation: hypotheses from roots of rounding differences"),
}
# The one-hypothesis case behind vR[-1] (exactly one hypothesis with nGood > 0) has no scene.  Faugeras' hypotheses come as two geometries,
# each with its (R, t) / (R, -t) pair; a point that reprojects under one geometry reprojects under the other too, and of each pair exactly
# one member sees it in front of both cameras, so a point counted by one hypothesis is counted by one of the other pair as well.  The
# case is exercised on given counts (tests/test_twoview_reconstruct_ref.py), and on the device the slot code it reaches is the one the
# no-hypothesis scenes reach for both slots.

EXITS = ("stock:SH+SF==0", "stock:H:d-test", "stock:F:reject", "stock:F:ok", "stock:F:low-parallax", "stock:H:ok", "stock:H:not-ok",
         "info:SH+SF==0", "info:H:d-test", "info:F:ok", "info:F:not-ok", "info:H:ok", "info:H:not-ok")
