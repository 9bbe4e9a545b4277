#!/usr/bin/env python3
"""Per-call latency (through ctypes, each call ends in its own wait) of the node-walk matchers over K keyframes per call against the loop of
K single calls they replace.  346 x 260, about 1 000 rows per keyframe, K = 1, 8, 20, for each of the four entry points:

  tri       eorb_search_for_triangulation_keyframes      vs K x eorb_search_for_triangulation       (Pinhole, checkOri off as the reference's callers)
  tri_kb8   eorb_search_for_triangulation_kb8_keyframes  vs K x eorb_search_for_triangulation_kb8   (monocular KannalaBrandt8)
  bow       eorb_search_by_bow_keyframes                 vs K x eorb_search_by_bow                  (Tracking::Relocalization)
  bow_kf    eorb_search_by_bow_kf_keyframes              vs K x eorb_search_by_bow_kf               (LoopClosing::DetectCommonRegionsFromBoW)

    batched        the one call for the K keyframes
    single_loop    K single calls on this library.  A single call is the set form with K = 1 (one marshalling path, one kernel per walk), so
                   at K = 1 batched and single_loop time the same code and differ by the Python wrappers only
    oracle_1core   K calls of the oracle's timing build (-O3 -march=native) on one core of the same host
    parent_loop    K single calls on the parent commit, measured by a child process of this tool in the same visit: --parent-root names a
                   checkout of the parent with its library built (git worktree add DIR HEAD~1 && make -C DIR/eorb_slam_amd/csrc); the
                   child imports the package from there and the scenes from this tree.  The yardstick for the batch.
    alone_loop     K single calls on this library, alone in a child process like parent_loop.  The children run in the order parent, this
                   tree, parent, this tree (parent_loop, alone_loop, parent_loop_2, alone_loop_2): whether the single entry points moved
                   is read off these four, not off single_loop, which shares its process and its loop with the batch.  single_vs_parent
                   states the comparison: the better p50 of the two alone runs against the worse p50 of the two parent runs plus the
                   margin, the larger of the two differences between the runs of one library.

batched and single_loop take turns inside one loop, so that a drift of the clocks or of the shared host touches them alike.  Prints one JSON
object (and writes it to --out)."""
import argparse, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
KS = (1, 8, 20)


def _time(calls, n, np):
    for _ in range(5):
        for fn in calls.values():
            fn()
    ts = {k: [] for k in calls}
    for _ in range(n):
        for k, fn in calls.items():
            t = time.perf_counter(); fn(); ts[k].append((time.perf_counter() - t) * 1e3)
    return {k: {"p50_ms": float(np.percentile(x, 50)), "p95_ms": float(np.percentile(x, 95)), "calls": len(x)} for k, x in ts.items()}


def _scenes(synth):
    # (the Pinhole part of the camera sees about 0.37 of the scene's points, the KannalaBrandt8 camera about 0.66)
    kw = dict(ndistract=150, nties=30, nnodes=250)
    return {"tri": synth.triangulation_neighbourhood(400, max(KS), pinhole=True, npts=1950, **kw),
            "tri_kb8": synth.triangulation_neighbourhood(401, max(KS), npts=1300, **kw),
            "bow": synth.bow_neighbourhood(402, max(KS), npts=1300, **kw)}


def _calls(name, s, K, fe, ctx):
    """(batched, single_loop) of one entry point over the first K keyframes of its scene; both return K rows.  (A parent checkout has no
    batched form: its child process only calls single_loop.)"""
    import numpy as np
    ks = list(range(K))
    mk_set = getattr(fe, "KeyFrameSet", lambda kfs: None)

    def rows(pairs, n1):
        m = np.full(n1, -1, np.int32); m[pairs[:, 0]] = pairs[:, 1]
        return m
    if name in ("tri", "tri_kb8"):
        S = mk_set([(kf["kps"], kf["desc"], kf["elig"], kf["fv"]) for kf in s["kfs"][:K]])
        one = (s["kps1"], s["desc1"], s["elig1"], s["fv1"])
        n1 = len(s["kps1"])
        if name == "tri":
            tabs = (s["scale2"], s["sigma2_2"])
            return (lambda: fe.SearchForTriangulationKeyFrames(*one, S, s["ep"][ks], s["F12"][ks], *tabs, False, False, ctx=ctx)[1],
                    lambda: [rows(fe.SearchForTriangulation(*one, kf["kps"], kf["desc"], kf["elig"], kf["fv"], s["ep"][k], s["F12"][k], *tabs, False, False,
                                                            ctx=ctx)[1], n1) for k, kf in enumerate(s["kfs"][:K])])
        tabs = (s["scale2"], s["sigma2_1"], s["sigma2_2"])
        return (lambda: fe.SearchForTriangulationKB8KeyFrames(s["kps1"], -1, *one[1:], S, [-1] * K, s["cams1"], s["cams2"], s["Rt"][ks], s["ep"][ks], *tabs,
                                                              False, False, ctx=ctx)[1],
                lambda: [rows(fe.SearchForTriangulationKB8(s["kps1"], -1, *one[1:], kf["kps"], -1, kf["desc"], kf["elig"], kf["fv"], s["cams1"], s["cams2"],
                                                           s["Rt"][k], s["ep"][k], *tabs, False, False, ctx=ctx)[1], n1) for k, kf in enumerate(s["kfs"][:K])])
    S = mk_set([(kf["kps"], kf["desc"], kf["has_mp"], kf["fv"]) for kf in s["kfs"][:K]])
    if name == "bow":
        return (lambda: fe.SearchByBoWKeyFrames(S, s["kps"], s["desc"], s["fv"], 0.7, True, ctx=ctx)[1],
                lambda: [fe.SearchByBoW(kf["kps"], kf["desc"], kf["has_mp"], kf["fv"], s["kps"], s["desc"], s["fv"], 0.7, True, ctx=ctx)[1]
                         for kf in s["kfs"][:K]])
    return (lambda: fe.SearchByBoW_KF_KeyFrames(s["kps"], s["desc"], s["has_mp"], s["fv"], S, 0.8, True, ctx=ctx)[1],
            lambda: [fe.SearchByBoW_KF(s["kps"], s["desc"], s["has_mp"], s["fv"], kf["kps"], kf["desc"], kf["has_mp"], kf["fv"], 0.8, True, ctx=ctx)[1]
                     for kf in s["kfs"][:K]])


def _oracle_loop(name, s, K, oracle):
    """K single-pair calls of the oracle's timing build.  Its Python wrappers of three of these walks take no `fast` flag, so they are called
    here on oracle.lib(True) with the wrappers' own marshalling."""
    import ctypes
    import numpy as np
    L = oracle.lib(True)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    c = lambda a, t: np.ascontiguousarray(a, t)
    kp, u8, f32 = oracle.KP_DTYPE, np.uint8, np.float32
    fv = lambda t: [c(a, d) for a, d in zip(t, (np.uint32, np.int32, np.int32))]

    def side(kps, desc, flag, t):
        k, d, f, (n, o, i) = c(kps, kp), c(desc, u8), c(flag, u8), fv(t)
        return dict(k=k, d=d, f=f, n=n, o=o, i=i)
    kfs = [side(kf["kps"], kf["desc"], kf["elig"] if "elig" in kf else kf["has_mp"], kf["fv"]) for kf in s["kfs"][:K]]
    if name == "tri_kb8":
        return lambda: [oracle.search_for_triangulation_kb8(s["kps1"], -1, s["desc1"], s["elig1"], s["fv1"], kf["kps"], -1, kf["desc"], kf["elig"], kf["fv"],
                                                            s["cams1"], s["cams2"], s["Rt"][k], s["ep"][k], s["scale2"], s["sigma2_1"], s["sigma2_2"], False,
                                                            False, fast=True)[1] for k, kf in enumerate(s["kfs"][:K])]
    if name == "tri":
        a = side(s["kps1"], s["desc1"], s["elig1"], s["fv1"])
        ep, F, sc, sg = c(s["ep"], f32), c(s["F12"], f32).reshape(-1, 9), c(s["scale2"], f32), c(s["sigma2_2"], f32)

        def tri():
            out = []
            for k, b in enumerate(kfs):
                m = np.full(len(a["k"]), -1, np.int32)
                L.orc_search_for_triangulation(vp(a["k"]), len(a["k"]), vp(a["d"]), a["d"].shape[1], vp(a["f"]), vp(a["n"]), vp(a["o"]), vp(a["i"]), len(a["n"]),
                                               vp(b["k"]), len(b["k"]), vp(b["d"]), b["d"].shape[1], vp(b["f"]), vp(b["n"]), vp(b["o"]), vp(b["i"]), len(b["n"]),
                                               vp(ep[k]), vp(F[k]), vp(sc), vp(sg), 0, 0, vp(m))
                out.append(m)
            return out
        return tri
    a = side(s["kps"], s["desc"], s["has_mp"], s["fv"])

    def bow():
        out = []
        for b in kfs:
            m = np.full(len(a["k"]), -1, np.int32)
            if name == "bow":
                L.orc_search_by_bow(vp(b["k"]), len(b["k"]), vp(b["d"]), vp(b["f"]), vp(b["n"]), vp(b["o"]), vp(b["i"]), len(b["n"]),
                                    vp(a["k"]), len(a["k"]), vp(a["d"]), vp(a["n"]), vp(a["o"]), vp(a["i"]), len(a["n"]), vp(m), 0.7, 1)
            else:
                L.orc_search_by_bow_kf(vp(a["k"]), len(a["k"]), vp(a["d"]), vp(a["f"]), vp(a["n"]), vp(a["o"]), vp(a["i"]), len(a["n"]),
                                       vp(b["k"]), len(b["k"]), vp(b["d"]), vp(b["f"]), vp(b["n"]), vp(b["o"]), vp(b["i"]), len(b["n"]), vp(m), 0.8, 1)
            out.append(m)
        return out
    return bow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--cpu-calls", type=int, default=20, help="oracle loops per shape (0: skip)")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its loop of K single calls is timed by a child process")
    ap.add_argument("--singles-only", action="store_true", help="time only the loop of K single calls (what the child process runs)")
    ap.add_argument("--pkg-root", default=None, help="with --singles-only: import eorb_slam_amd from this checkout (the scenes still come from this tree)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    if a.pkg_root:
        import importlib.util
        spec = importlib.util.spec_from_file_location("kfbatch_synth", os.path.join(ROOT, "eorb_slam_amd", "synth.py"))
        synth = importlib.util.module_from_spec(spec); spec.loader.exec_module(synth)
        sys.path.insert(0, os.path.abspath(a.pkg_root))
        from eorb_slam_amd import frontend as fe
        assert os.path.abspath(fe.__file__).startswith(os.path.abspath(a.pkg_root)), fe.__file__
    else:
        from eorb_slam_amd import frontend as fe, synth
    from twocam_latency import _sources_hash
    scenes = _scenes(synth)
    scenes["bow_kf"] = scenes["bow"]
    res = {"size": [346, 260], "rows_per_keyframe": {n: int(np.mean([len(kf["kps"]) for kf in s["kfs"]])) for n, s in scenes.items()}, "shapes": {}}
    if not a.singles_only:
        res["sources_hash"] = _sources_hash()
    ctx = fe.Context()
    oracle = None
    if a.cpu_calls and not a.singles_only:
        from oracle import oracle_py as oracle
        oracle.build()
    for name, s in scenes.items():
        for K in KS:
            batched, single = _calls(name, s, K, fe, ctx)
            if a.singles_only:
                e = _time({"single_loop": single}, a.calls, np)
            else:
                b, f = batched(), single()
                assert all(np.array_equal(b[k], f[k]) for k in range(K)) and min(int((r >= 0).sum()) for r in b) >= 20, name
                e = _time({"batched": batched, "single_loop": single}, a.calls, np)
                e["matches_per_keyframe"] = int(np.mean([(r >= 0).sum() for r in b]))
                if oracle is not None:
                    o = _oracle_loop(name, s, K, oracle)
                    assert all(np.array_equal(b[k], r) for k, r in enumerate(o())), name
                    e.update({"oracle_1core": _time({"o": o}, a.cpu_calls, np)["o"]})
            res["shapes"]["%s_K%d" % (name, K)] = e
    ctx.close()
    if a.parent_root and not a.singles_only:
        # parent, this tree, parent, this tree: each loop of K single calls alone in a child process, so that the two libraries are timed
        # under the same conditions and the spread between two runs of one library shows beside their difference
        def child(root):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--singles-only", "--pkg-root", root, "--calls", str(a.calls)],
                                 capture_output=True, text=True, timeout=900)
            assert out.returncode == 0, out.stderr[-2000:]
            return json.loads(out.stdout.strip().split("\n")[-1])["shapes"]
        runs = [child(r) for r in (a.parent_root, ROOT, a.parent_root, ROOT)]
        for key, e in res["shapes"].items():
            e["parent_loop"], e["alone_loop"], e["parent_loop_2"], e["alone_loop_2"] = [r[key]["single_loop"] for r in runs]
            pp, aa = [e[k]["p50_ms"] for k in ("parent_loop", "parent_loop_2")], [e[k]["p50_ms"] for k in ("alone_loop", "alone_loop_2")]
            margin = max(abs(pp[0] - pp[1]), abs(aa[0] - aa[1]))
            e["single_vs_parent"] = {"alone_best_ms": min(aa), "parent_worst_ms": max(pp), "margin_ms": margin, "no_slower": bool(min(aa) <= max(pp) + margin)}
            e["batched_beats_parent_loop"] = bool(e["batched"]["p50_ms"] < min(e["parent_loop"]["p50_ms"], e["parent_loop_2"]["p50_ms"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
