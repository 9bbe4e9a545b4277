#!/usr/bin/env python3
"""Per-call latency (through ctypes, each call ends in its own wait) of the KeyFrame-side matchers with the projection on the device,
against the path callers have without them.  346 x 260, 1 000 keypoints per keyframe, M = 1 000 map points:

  fuse K = 1, 8, 20
    batched          eorb_fuse_keyframes, one call for the K keyframes
    fused_per_kf     eorb_fuse_pose, K calls
    cpu_path         per keyframe: the CPU restatement of the projection on one core of the same host (tests/kfside_ref, its timing
                     build: -O3 -march=native), then eorb_kf_radius_match: what callers have without the projector
  sim3 (one pair)
    fused            eorb_search_by_sim3
    cpu_path         the restatement of both projections, eorb_kf_radius_match twice, the agreement loop in numpy

--mixed: the same shape on mixed ORB + AKAZE keyframes (synth.mixed_keyframe_neighbourhood), fuse K = 1, 8, 20
    mixed_batched    eorb_fuse_keyframes_mixed, one call for the K keyframes
    mixed_per_kf     eorb_fuse_pose_mixed, K calls
    cpu_restatement  per keyframe: the CPU restatement of MixedMatcher's projection and search on one core of the same host
                     (tests/kfside_mixed_ref, timing build)
    orb_batched      eorb_fuse_keyframes on the same keypoints and points read as ORB ones: the ORB-only kernels in the same build

--parent-root DIR: every entry point of the radius search on its own, against the parent commit in the same visit.  DIR names a checkout
of the parent with its library built (git worktree add DIR HEAD~1 && make -C DIR/eorb_slam_amd/csrc).  Child processes of this tool
(--rows-only --pkg-root) time the rows alone, in the order parent, this tree, parent, this tree; a child imports the package from its
root and the scenes from this tree.  Rows: fuse_pose_K* (K calls), fuse_keyframes_K* (one call), sim3, and on one keyframe
radius_independent (eorb_kf_radius_match), radius_in_order (the same with taken / accept_thr) and kf_scw
(eorb_search_by_projection_kf_scw); with --mixed the *_mixed entry points (no sim3).  vs_parent states per row the better p50 of this
tree's two runs against the worse p50 of the parent's two plus the margin, the larger of the two differences between the runs of one
library.

The calls of a shape take turns inside one loop, so that a drift of the clocks or of the shared host touches them alike.  Prints one
JSON object (and writes it to --out)."""
import argparse, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H = 346, 260


def _time(calls, n, np):
    for _ in range(5):
        for fn in calls.values():
            fn()
    ts = {k: [] for k in calls}
    for _ in range(n):
        for k, fn in calls.items():
            t = time.perf_counter(); fn(); ts[k].append((time.perf_counter() - t) * 1e3)
    return {k: {"p50_ms": float(np.percentile(x, 50)), "p95_ms": float(np.percentile(x, 95)), "calls": len(x)} for k, x in ts.items()}


def _rows(a, np, fe, synth, ctx):
    """name -> call of every entry point of the radius search (its *_mixed form with --mixed), each a whole call ending in its wait"""
    M, n, mixed = a.M, a.n, a.mixed
    gb = fe.grid_bounds(W, H)
    rows = {}
    taken = (np.random.default_rng(3).random(n) < 0.2).astype(np.uint8)
    for K in (1, 8, 20):
        sc = (synth.mixed_keyframe_neighbourhood if mixed else synth.keyframe_neighbourhood)(200 + K, K, M, n_kps=n)
        geom = (sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"])
        views = [fe.view(**kw) for kw in sc["views"]]
        kps = np.concatenate(sc["kps"]); desc = np.concatenate(sc["desc"])
        off = (np.arange(K + 1) * n).astype(np.int32)
        qd = sc["mp_desc"]
        if mixed:
            kio = np.concatenate(sc["kp_is_orb"]); sig = np.concatenate(sc["kp_inv_sigma2"]); mio = sc["mp_is_orb"]
            one = lambda k, sc=sc: dict(kp_is_orb=sc["kp_is_orb"][k], kp_inv_sigma2=sc["kp_inv_sigma2"][k], mp_is_orb=sc["mp_is_orb"])
            rows["fuse_pose_mixed_K%d" % K] = lambda sc=sc, views=views, geom=geom, qd=qd, K=K, one=one: [
                fe.FusePoseMixed(sc["kps"][k], sc["desc"][k], gb, views[k], *geom, qd, th=3.0, ctx=ctx, **one(k)) for k in range(K)]
            rows["fuse_keyframes_mixed_K%d" % K] = lambda views=views, kps=kps, desc=desc, off=off, geom=geom, qd=qd, K=K, kio=kio, sig=sig, mio=mio: \
                fe.FuseKeyFramesMixed(views, [gb] * K, kps, desc, off, *geom, qd, kp_is_orb=kio, kp_inv_sigma2=sig, mp_is_orb=mio, th=3.0, ctx=ctx)
        else:
            isg = sc["inv_sigma2"]
            rows["fuse_pose_K%d" % K] = lambda sc=sc, views=views, geom=geom, qd=qd, K=K, isg=isg: [
                fe.FusePose(sc["kps"][k], sc["desc"][k], gb, views[k], *geom, qd, inv_sigma2=isg, th=3.0, ctx=ctx) for k in range(K)]
            rows["fuse_keyframes_K%d" % K] = lambda views=views, kps=kps, desc=desc, off=off, geom=geom, qd=qd, K=K, isg=isg: \
                fe.FuseKeyFrames(views, [gb] * K, kps, desc, off, *geom, qd, inv_sigma2=isg, th=3.0, ctx=ctx)
        if K == 1:
            _single_rows(rows, np, fe, ctx, mixed, gb, sc, views[0], geom, taken)
    if not mixed:
        sp = synth.sim3_pair(300, n=n, s12=0.9)
        kf = [dict(k, gb=gb, view=fe.view(**k["view"])) for k in (sp["kf1"], sp["kf2"])]
        rows["sim3"] = lambda: fe.SearchBySim3Pose(kf[0], kf[1], sp["sR12"], sp["t12"], sp["sR21"], sp["t21"], th=7.5, ctx=ctx)
    return rows


def _single_rows(rows, np, fe, ctx, mixed, gb, sc, v0, geom, taken):
    """one keyframe on its own: the projection of its scene (made once, by the device) feeds the search-only entry point"""
    k0, d0, qd = sc["kps"][0], sc["desc"][0], sc["mp_desc"]
    if mixed:
        mio = sc["mp_is_orb"]
        fl = dict(kp_is_orb=sc["kp_is_orb"][0], mp_is_orb=mio)
        p = fe.ProjectKeyFrameSideMixed(v0, *geom, 3.0, mp_is_orb=mio, ctx=ctx)
        q = (p["valid"], p["uv"], p["radius"], p["level"], qd)
        rows["radius_independent_mixed"] = lambda: fe.KeyFrameRadiusMatchMixed(k0, d0, gb, *q, kp_inv_sigma2=sc["kp_inv_sigma2"][0], ctx=ctx, **fl)
        rows["radius_in_order_mixed"] = lambda: fe.KeyFrameRadiusMatchMixed(k0, d0, gb, *q, taken=taken, accept_thr=50.0, ctx=ctx, **fl)
        rows["kf_scw_mixed"] = lambda: fe.SearchByProjectionKFScwMixed(k0, d0, gb, v0, *geom, qd, taken, 3.0, ctx=ctx, **fl)
    else:
        p = fe.ProjectKeyFrameSide(v0, *geom, 3.0, ctx=ctx)
        q = (p["valid"], p["uv"], p["radius"], p["level"], qd)
        rows["radius_independent"] = lambda: fe.KeyFrameRadiusMatch(k0, d0, gb, *q, inv_sigma2=sc["inv_sigma2"], ctx=ctx)
        rows["radius_in_order"] = lambda: fe.KeyFrameRadiusMatch(k0, d0, gb, *q, taken=taken, accept_thr=50.0, ctx=ctx)
        rows["kf_scw"] = lambda: fe.SearchByProjectionKFScw(k0, d0, gb, v0, *geom, qd, taken, 3.0, ctx=ctx)


def _vs_parent(a, np):
    """parent, this tree, parent, this tree: the rows alone in a child process each, so that the two libraries are timed under the same
    conditions and the spread between two runs of one library shows beside their difference"""
    def child(root):
        cmd = [sys.executable, os.path.abspath(__file__), "--rows-only", "--pkg-root", root, "--calls", str(a.calls), "--M", str(a.M), "--n", str(a.n)]
        out = subprocess.run(cmd + (["--mixed"] if a.mixed else []), capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads(out.stdout.strip().split("\n")[-1])["rows"]
    runs = [child(r) for r in (a.parent_root, ROOT, a.parent_root, ROOT)]
    res = {}
    for key in runs[0]:
        e = dict(zip(("parent", "this", "parent_2", "this_2"), (r[key] for r in runs)))
        pp, tt = [e[k]["p50_ms"] for k in ("parent", "parent_2")], [e[k]["p50_ms"] for k in ("this", "this_2")]
        margin = max(abs(pp[0] - pp[1]), abs(tt[0] - tt[1]))
        e.update(this_best_ms=min(tt), parent_worst_ms=max(pp), margin_ms=margin, no_slower=bool(min(tt) <= max(pp) + margin))
        res[key] = e
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--M", type=int, default=1000)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mixed", action="store_true", help="time the *_mixed entry points instead (profiles/kfside_mixed_latency.json)")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: child processes time every row on both libraries")
    ap.add_argument("--rows-only", action="store_true", help="time only the entry points' rows (what a child process runs)")
    ap.add_argument("--pkg-root", default=None, help="with --rows-only: import eorb_slam_amd from this checkout (the scenes still come from this tree)")
    a = ap.parse_args()
    import numpy as np
    if a.rows_only:
        import importlib.util
        spec = importlib.util.spec_from_file_location("kfside_synth", os.path.join(ROOT, "eorb_slam_amd", "synth.py"))
        synth = importlib.util.module_from_spec(spec); spec.loader.exec_module(synth)
        if a.pkg_root:
            sys.path.insert(0, os.path.abspath(a.pkg_root))
        from eorb_slam_amd import frontend as fe
        assert os.path.abspath(fe.__file__).startswith(os.path.abspath(a.pkg_root or ROOT)), fe.__file__
        ctx = fe.Context()
        res = {"rows": _time(_rows(a, np, fe, synth, ctx), a.calls, np)}
        ctx.close()
        return _emit(res, a.out)
    from eorb_slam_amd import frontend as fe, synth
    from twocam_latency import _sources_hash
    import kfside_ref as ref
    M, n = a.M, a.n
    if a.mixed:
        return _mixed(a, np, fe, synth, _sources_hash())
    res = {"sources_hash": _sources_hash(), "M": M, "n": n, "size": [W, H], "fuse": {}, "sim3": {}}
    ctx = fe.Context()
    gb = fe.grid_bounds(W, H)
    for K in (1, 8, 20):
        sc = synth.keyframe_neighbourhood(200 + K, K, M, n_kps=n)
        geom = (sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"])
        views = [fe.view(**kw) for kw in sc["views"]]; rviews = [ref.view(**kw) for kw in sc["views"]]
        kps = np.concatenate(sc["kps"]); desc = np.concatenate(sc["desc"])
        off = (np.arange(K + 1) * n).astype(np.int32)
        isg, qd = sc["inv_sigma2"], sc["mp_desc"]

        def batched():
            return fe.FuseKeyFrames(views, [gb] * K, kps, desc, off, *geom, qd, inv_sigma2=isg, th=3.0, ctx=ctx)

        def per_kf():
            return [fe.FusePose(sc["kps"][k], sc["desc"][k], gb, views[k], *geom, qd, inv_sigma2=isg, th=3.0, ctx=ctx) for k in range(K)]

        def cpu_path():
            out = []
            for k in range(K):
                p = ref.keyframe_side(rviews[k], *geom, 3.0, timing=True)
                out.append(fe.KeyFrameRadiusMatch(sc["kps"][k], sc["desc"][k], gb, p["valid"], p["uv"], p["radius"], p["level"], qd, inv_sigma2=isg, ctx=ctx))
            return out
        b, f, c = batched(), per_kf(), cpu_path()
        for k in range(K):
            assert np.array_equal(b[0][k], f[k][0]) and np.array_equal(b[0][k], c[k][0]) and np.array_equal(b[1][k], c[k][1])
        assert int((b[1] <= 50).sum()) >= 30 * K
        e = _time({"batched": batched, "fused_per_kf": per_kf, "cpu_path": cpu_path}, a.calls, np)
        e["batched_beats_cpu_path"] = bool(e["batched"]["p50_ms"] < e["cpu_path"]["p50_ms"])
        e["fused_per_kf_beats_cpu_path"] = bool(e["fused_per_kf"]["p50_ms"] < e["cpu_path"]["p50_ms"])
        res["fuse"]["K%d" % K] = e
    # one Sim3 pair
    sp = synth.sim3_pair(300, n=n, s12=0.9)
    k1, k2 = sp["kf1"], sp["kf2"]
    kf = [dict(k, gb=gb, view=fe.view(**k["view"])) for k in (k1, k2)]
    rv1, rv2 = ref.view(**k1["view"]), ref.view(**k2["view"])
    cam = k1["view"]["cam"]

    def sim3_fused():
        return fe.SearchBySim3Pose(kf[0], kf[1], sp["sR12"], sp["t12"], sp["sR21"], sp["t21"], th=7.5, ctx=ctx)

    def sim3_cpu():
        p12 = ref.sim3_half(rv1, sp["sR21"], sp["t21"], cam, rv2, k1["pos"], k1["min_dist"], k1["max_dist"], 7.5, skip=k1["skip"], timing=True)
        p21 = ref.sim3_half(rv2, sp["sR12"], sp["t12"], cam, rv1, k2["pos"], k2["min_dist"], k2["max_dist"], 7.5, skip=k2["skip"], timing=True)
        bi1, bd1 = fe.KeyFrameRadiusMatch(k2["kps"], k2["desc"], gb, p12["valid"], p12["uv"], p12["radius"], p12["level"], k1["mp_desc"], ctx=ctx)
        bi2, bd2 = fe.KeyFrameRadiusMatch(k1["kps"], k1["desc"], gb, p21["valid"], p21["uv"], p21["radius"], p21["level"], k2["mp_desc"], ctx=ctx)
        vn1 = np.where(bd1 <= 100, bi1, -1); vn2 = np.where(bd2 <= 100, bi2, -1)
        ok = (vn1 >= 0) & (vn2[np.clip(vn1, 0, len(vn2) - 1)] == np.arange(len(vn1)))
        return int(ok.sum()), np.where(ok, vn1, -1).astype(np.int32)
    g, w = sim3_fused(), sim3_cpu()
    assert g[0] == w[0] and np.array_equal(g[1], w[1]) and g[0] >= 30
    e = _time({"fused": sim3_fused, "cpu_path": sim3_cpu}, a.calls, np)
    e["fused_beats_cpu_path"] = bool(e["fused"]["p50_ms"] < e["cpu_path"]["p50_ms"])
    res["sim3"] = e
    ctx.close()
    if a.parent_root:
        res["vs_parent"] = _vs_parent(a, np)
    _emit(res, a.out)


def _emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(line + "\n")


def _mixed(a, np, fe, synth, sources_hash):
    import kfside_mixed_ref as mref
    from oracle import oracle_py as oracle
    oracle.build()
    mref.use_oracle(oracle)
    M, n = a.M, a.n
    res = {"sources_hash": sources_hash, "M": M, "n": n, "size": [W, H], "mixed_fuse": {}}
    ctx = fe.Context()
    gb = fe.grid_bounds(W, H)
    for K in (1, 8, 20):
        sc = synth.mixed_keyframe_neighbourhood(200 + K, K, M, n_kps=n)
        geom = (sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"])
        views = [fe.view(**kw) for kw in sc["views"]]; rviews = [mref.view(**kw) for kw in sc["views"]]
        frames = [oracle.Frame(sc["kps"][k], sc["desc"][k], W, H) for k in range(K)]
        kps = np.concatenate(sc["kps"]); desc = np.concatenate(sc["desc"])
        kio = np.concatenate(sc["kp_is_orb"]); sig = np.concatenate(sc["kp_inv_sigma2"]); mio = sc["mp_is_orb"]
        off = (np.arange(K + 1) * n).astype(np.int32)
        isg, qd = sc["inv_sigma2"], sc["mp_desc"]

        def mixed_batched():
            return fe.FuseKeyFramesMixed(views, [gb] * K, kps, desc, off, *geom, qd, kp_is_orb=kio, kp_inv_sigma2=sig, mp_is_orb=mio, th=3.0, ctx=ctx)

        def mixed_per_kf():
            return [fe.FusePoseMixed(sc["kps"][k], sc["desc"][k], gb, views[k], *geom, qd, kp_is_orb=sc["kp_is_orb"][k],
                                     kp_inv_sigma2=sc["kp_inv_sigma2"][k], mp_is_orb=mio, th=3.0, ctx=ctx) for k in range(K)]

        def cpu_restatement():
            out = []
            for k in range(K):
                p = mref.keyframe_side(rviews[k], *geom, 3.0, mp_is_orb=mio, timing=True)
                out.append(mref.search(frames[k], p, qd, kp_is_orb=sc["kp_is_orb"][k], kp_inv_sigma2=sc["kp_inv_sigma2"][k], mp_is_orb=mio, timing=True))
            return out

        def orb_batched():
            return fe.FuseKeyFrames(views, [gb] * K, kps, desc, off, *geom, qd, inv_sigma2=isg, th=3.0, ctx=ctx)
        b, f, c = mixed_batched(), mixed_per_kf(), cpu_restatement()
        for k in range(K):
            assert np.array_equal(b[0][k], f[k][0]) and np.array_equal(b[0][k], c[k][0]) and np.array_equal(b[1][k], c[k][1])
        assert int((b[1] <= 50).sum()) >= 30 * K
        e = _time({"mixed_batched": mixed_batched, "mixed_per_kf": mixed_per_kf, "cpu_restatement": cpu_restatement, "orb_batched": orb_batched},
                  a.calls, np)
        e["mixed_over_orb_batched"] = e["mixed_batched"]["p50_ms"] / e["orb_batched"]["p50_ms"]
        e["accepted"] = {"mixed": int((b[1] <= 50).sum()), "orb_only": int((orb_batched()[1] <= 50).sum())}
        res["mixed_fuse"]["K%d" % K] = e
    ctx.close()
    if a.parent_root:
        res["vs_parent"] = _vs_parent(a, np)
    _emit(res, a.out)


if __name__ == "__main__":
    main()
