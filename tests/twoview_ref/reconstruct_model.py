"""A second writing of what stands between and after the two stages of TwoViewReconstruction::Reconstruct, independent of
eorb_slam_amd/csrc/twoview_core.h: the four decision rules and the slot ordering over given (nGood, parallax) lists in Python integers and
numpy float32 scalars (ReconstructF :638-709 / :937-978 with resolveReconstStatF :876-900, ReconstructH :828-872 / :1110-1174 with
resolveReconstStatH :981-989), and DecomposeE (:1354-1375) and the Faugeras hypotheses (:722-825) in float64 numpy.

`variant` names one deliberately wrong reading of one comparison; tests/test_twoview_reconstruct_ref.py shows for each a scene on which it
differs from the restatement:
    h_best_ge        the H walk takes a new best on >= (a later hypothesis wins a tie) instead of >
    multimap_reversed  equal counts leave the multimap in the order 4, 3, 2, 1 instead of 1, 2, 3, 4
    nsimilar_ge1     "nsimilar > 1" read as "nsimilar >= 1"
    h_parallax_gt    "bestParallax >= minParallax" read as ">"
    h_second_ge      the H walk's second best is replaced on >= instead of >
    min_good_round   static_cast<int>(mThMinGoodR*N) rounded to nearest instead of truncated
"""
import numpy as np

VARIANTS = ("h_best_ge", "multimap_reversed", "nsimilar_ge1", "h_parallax_gt", "h_second_ge", "min_good_round")
f32 = np.float32
RULE_KEYS = ("ok", "n_min_good", "n_similar", "info_good", "hyp_best", "hyp_second", "best_good", "second_good", "best_parallax", "second_parallax")


def _n_min_good(p, N, variant):
    x = f32(p.th_min_good_r) * f32(N)
    n = int(np.rint(x)) if variant == "min_good_round" else int(x)
    return max(n, int(p.min_triangulated))


def rules(p, is_homography, n_good, parallax, N, variant=None):
    """p: the parameter structure (form, min_parallax, min_triangulated, th_min_good_r, th_max_good_r_f, th_max_good_r_h); n_good / parallax:
    per hypothesis in hypothesis order (4 or 8) -> dict of RULE_KEYS as eorb_tvr_recon_result has them"""
    assert variant is None or variant in VARIANTS
    ng = [int(v) for v in n_good]; par = [f32(v) for v in parallax]
    info = int(p.form) == 1
    min_par, min_tri = f32(p.min_parallax), int(p.min_triangulated)
    o = dict(ok=0, n_min_good=0, n_similar=0, info_good=[0] * 8, hyp_best=-1, hyp_second=-1, best_good=0, second_good=0, best_parallax=f32(0),
             second_parallax=f32(0))
    many = (lambda n: n >= 1) if variant == "nsimilar_ge1" else (lambda n: n > 1)
    if not is_homography:
        assert len(ng) == 4
        thr = f32(p.th_max_good_r_f)
        if not info:
            max_good = max(ng)
            n_min = _n_min_good(p, N, variant)
            nsim = sum(1 for g in ng if f32(g) > thr * f32(max_good))
            first = ng.index(max_good)
            o.update(n_min_good=n_min, n_similar=nsim, best_good=max_good, best_parallax=par[first])
            if not (max_good < n_min or many(nsim)) and par[first] > min_par:
                o.update(ok=1, hyp_best=first)
        else:
            idx = list(range(4))
            if variant == "multimap_reversed":
                idx.reverse()
            order = sorted(idx, key=lambda i: -ng[i])                       # stable: equal counts keep the order of idx
            o["info_good"][:4] = [ng[i] for i in order]
            o.update(hyp_best=order[0], hyp_second=order[1], best_good=ng[order[0]], second_good=ng[order[1]], best_parallax=par[order[0]],
                     second_parallax=par[order[1]])
            max_good = o["best_good"]
            n_min = _n_min_good(p, N, variant)
            nsim = sum(1 for g in o["info_good"] if f32(g) > thr * f32(max_good)) & 255
            distinct = not (max_good < n_min or many(nsim))
            o.update(n_min_good=n_min, n_similar=nsim, ok=int(bool(o["best_parallax"] > min_par) and distinct))
    else:
        assert len(ng) == 8
        best = second = 0
        bi = si = -1
        bp = sp = f32(-1)
        for i, g in enumerate(ng):
            if (g >= best) if variant == "h_best_ge" else (g > best):
                second, best, si, bi, sp, bp = best, g, bi, i, bp, par[i]
            elif (g >= second) if variant == "h_second_ge" else (g > second):
                second, si, sp = g, i, par[i]
        par_ok = (bp > min_par) if variant == "h_parallax_gt" else (bp >= min_par)
        ok = bool(f32(second) < f32(p.th_max_good_r_h) * f32(best)) and bool(par_ok) and best > min_tri and bool(f32(best) > f32(p.th_min_good_r) * f32(N))
        o.update(best_good=best, second_good=second, best_parallax=bp, ok=int(ok))
        if info:
            o.update(info_good=list(ng), hyp_best=bi, hyp_second=si, second_parallax=sp)
        elif ok:
            o.update(hyp_best=bi)
    o["info_good"] = np.array(o["info_good"], np.int32)
    return o


# ---- the hypotheses in float64 ----------------------------------------------------------------------------------------------------------
def decompose_e(K, F21):
    """ReconstructF's four (R, t) for E = K^T F K, in float64 (scenes.decompose_e_poses, from F instead of a known motion)"""
    K = np.asarray(K, np.float64); F = np.asarray(F21, np.float64)
    U, _, Vt = np.linalg.svd(K.T @ F @ K)
    t = U[:, 2] / np.linalg.norm(U[:, 2])
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1 = U @ W @ Vt
    R2 = U @ W.T @ Vt
    if np.linalg.det(R1) < 0:
        R1 = -R1
    if np.linalg.det(R2) < 0:
        R2 = -R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def faugeras(K, H21):
    """ReconstructH's eight (R, t) in float64, in the reference's order; (d1, d2, d3) as well"""
    K = np.asarray(K, np.float64); H = np.asarray(H21, np.float64)
    U, w, Vt = np.linalg.svd(np.linalg.inv(K) @ H @ K)
    s = np.linalg.det(U) * np.linalg.det(Vt)
    d1, d2, d3 = w
    aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)); aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1 = [aux1, aux1, -aux1, -aux1]; x3 = [aux3, -aux3, aux3, -aux3]
    root = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
    st = root / ((d1 + d3) * d2); ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    sp = root / ((d1 - d3) * d2); cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    out = []
    for i, sg in enumerate([st, -st, -st, st]):
        Rp = np.array([[ct, 0, -sg], [0, 1, 0], [sg, 0, ct]])
        t = U @ (np.array([x1[i], 0, -x3[i]]) * (d1 - d3))
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    for i, sg in enumerate([sp, -sp, -sp, sp]):
        Rp = np.array([[cp, 0, sg], [0, -1, 0], [sg, 0, -cp]])
        t = U @ (np.array([x1[i], 0, x3[i]]) * (d1 + d3))
        out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    return out, (d1, d2, d3)


def pose_deviation(model, restated):
    """every float64 (R, t) matched to the nearest restated pose ([Kp, 27] float32) -> (largest |R - R'|, largest |t - t'|) over the model's
    poses.  The SVD's sign and order freedoms permute the hypotheses and nothing else, so the nearest one is the counterpart."""
    dR = dt = 0.0
    for R, t in model:
        best = None
        for q in np.asarray(restated, np.float64):
            e = (np.abs(q[:9].reshape(3, 3) - R).max(), np.abs(q[9:12] - t).max())
            if best is None or max(e) < max(best):
                best = e
        dR, dt = max(dR, best[0]), max(dt, best[1])
    return dR, dt
