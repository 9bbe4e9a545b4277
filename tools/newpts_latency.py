#!/usr/bin/env python3
"""Per-call latency (through ctypes, each call ends in its own wait) of CreateNewMapPoints' triangulation stage on the device against the
CPU restatement (tests/newpts_ref, its timing build -O3 -march=native -ffp-contract=off, one core of the same host, the same matches):
346x260 Pinhole keyframes of about 1 000 rows (synth.triangulation_neighbourhood), K = 1, 8 and 20 neighbours per call.

    stage_dev        eorb_new_map_points on match12 handed in from the host
    stage_cpu_1t     the restatement's sequential loop on the same match12
    fused_dev        eorb_create_new_map_points: search and stage, match12 stays on the device
    parent_path      what the library offered before: eorb_search_for_triangulation_keyframes, match12 downloaded, the restatement
    search_dev       the search call alone
    chain_dev        fused_dev, then eorb_fuse_keyframes of the new points into the K neighbours (the next device call of local mapping)
    chain_parent     parent_path, then the same eorb_fuse_keyframes

The device and the restatement take turns inside one loop; their results are compared as bytes before anything is timed.  The per-kernel
split of one fused call comes from the library's own event timers (eorb_prof_*), in a pass of its own.  Prints one JSON object (and
writes it to --out)."""
import argparse, ctypes as C, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
KS = (1, 8, 20)
KEYS = ("status", "x3d", "n_new")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--neighbours", type=int, nargs="*", default=list(KS))
    ap.add_argument("--npts", type=int, default=1700)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from eorb_slam_amd import frontend as fe, synth
    import newpts_ref as nr
    from newpts_ref import scenes
    from twoview_latency import _time, _canon, _prof
    from twocam_latency import _sources_hash
    W, H = 346, 260
    res = {"sources_hash": _sources_hash(), "shapes": {}}
    ctx = fe.Context()
    scale, sigma2 = synth.level_tables()
    for K in a.neighbours:
        s = synth.triangulation_neighbourhood(900 + K, K, pinhole=True, npts=a.npts, ndistract=150, nties=30, nnodes=40)
        cam = synth.CAM_MONO[:4]
        views1 = [scenes.make_view(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), cam)]
        views2 = [[scenes.make_view(*synth.neighbour_pose(k), cam)] for k in range(K)]
        kfs = fe.KeyFrameSet([(kf["kps"], kf["desc"], kf["elig"], kf["fv"]) for kf in s["kfs"]])
        sa = (s["kps1"], s["desc1"], s["elig1"], s["fv1"], kfs, s["ep"], s["F12"], s["scale2"], s["sigma2_2"])
        nm, m = fe.SearchForTriangulationKeyFrames(*sa, False, False, ctx=ctx)
        sc = scenes.scene_of_search(s, views1, views2, scale, sigma2, m, "pinhole")
        v1, v2 = nr.views(sc)
        kw = nr.params(sc)
        # results equal as bytes before anything is timed
        ref = nr.loop(sc, timing=True)
        dev = fe.NewMapPoints(sc["kps1"], sc["kps2"], sc["kf_off"], m, v1, v2, ctx=ctx, **kw)
        nm2, m2, fused = fe.CreateNewMapPoints(*sa, v1, v2, False, False, ctx=ctx, **kw)
        assert np.array_equal(m, m2)
        for key in KEYS:
            assert _canon(dev[key], np) == _canon(ref[key], np) == _canon(fused[key], np), (K, key)
        # the next device call of local mapping on the new points (SearchInNeighbors' Fuse), on its own inputs: what is timed is the call
        new = np.argwhere(ref["status"] == nr.S["new"])
        pos = ref["x3d"][new[:, 0], new[:, 1]]
        M = len(pos)
        nrm = pos / np.maximum(np.linalg.norm(pos, axis=1, keepdims=True), 1e-6)
        fviews = [fe.view(v[0]["R"], v[0]["t"], v[0]["Ow"], cam, (0, W, 0, H), len(scale), float(np.log(1.2)), scale) for v in views2]
        gbs = [fe.grid_bounds(W, H)] * K
        fa = (fviews, gbs, kfs.kps, kfs.desc, kfs.kf_off, pos, nrm.astype(np.float32), np.full(M, 0.1, np.float32), np.full(M, 200.0, np.float32),
              s["desc1"][new[:, 1]][:, :32].copy())
        A = nr.args(sc, aids=False)
        cpu = nr.lib(timing=True)
        has = np.zeros(sc["n1"], np.uint8)
        p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731

        def stage_cpu(rows=m):
            cpu.npr_loop(C.byref(A.P), p(sc["kps1"]), sc["n1"], p(sc["kps2"]), p(sc["kf_off"]), K, p(rows), p(A.status), p(A.x3d), None, None, p(A.n_new), p(has))

        def stage_dev():
            fe.NewMapPoints(sc["kps1"], sc["kps2"], sc["kf_off"], m, v1, v2, ctx=ctx, aids=False, **kw)

        def search_dev():
            return fe.SearchForTriangulationKeyFrames(*sa, False, False, ctx=ctx)[1]

        def fused_dev():
            fe.CreateNewMapPoints(*sa, v1, v2, False, False, ctx=ctx, aids=False, **kw)

        def parent_path():
            stage_cpu(search_dev())

        def fuse():
            fe.FuseKeyFrames(*fa, ctx=ctx)
        e = _time({"stage_dev": stage_dev, "stage_cpu_1t": stage_cpu, "fused_dev": fused_dev, "parent_path": parent_path, "search_dev": search_dev,
                   "chain_dev": lambda: (fused_dev(), fuse()), "chain_parent": lambda: (parent_path(), fuse())}, a.calls, np)
        e["n1"] = int(sc["n1"]); e["rows2"] = int(sc["kf_off"][-1]); e["matches"] = int((m >= 0).sum()); e["new_points"] = int(M)
        e["status"] = dict(zip(nr.STATUS, np.bincount(ref["status"].ravel(), minlength=len(nr.STATUS)).tolist()))
        e["stage_speedup"] = e["stage_cpu_1t"]["p50_ms"] / e["stage_dev"]["p50_ms"]
        e["fused_speedup_over_parent_path"] = e["parent_path"]["p50_ms"] / e["fused_dev"]["p50_ms"]
        e["chain_saving_ms"] = e["chain_parent"]["p50_ms"] - e["chain_dev"]["p50_ms"]
        e["kernels_ms"] = _prof(ctx, fused_dev, 20)
        res["shapes"]["K%d" % K] = e
    ctx.close()
    res["stage_faster_on_device_at_K"] = [K for K in a.neighbours if res["shapes"]["K%d" % K]["stage_speedup"] > 1.0]
    res["fused_faster_than_parent_path_at_K"] = [K for K in a.neighbours if res["shapes"]["K%d" % K]["fused_speedup_over_parent_path"] > 1.0]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
