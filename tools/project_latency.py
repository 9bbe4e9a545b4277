#!/usr/bin/env python3
"""Per-call latency (through ctypes, each call ends in its own wait) of the map-point projector and the fused tracking searches,
against what a caller does without them.  M map points, n keypoints, two image sizes; per shape and per search (local = isInFrustum +
SearchByProjection(F, map points), last = the last-frame search, kf = the relocalisation search):

  fused              eorb_search_local_points / eorb_search_by_projection_last_pose / eorb_search_by_projection_kf_pose
  matcher_alone      (a) eorb_search_by_projection_map / _last / _kf on projections computed beforehand
  cpu_project_plus_matcher   (b) the CPU restatement of the projection on one core of the same host (tests/proj_ref/proj_ref.c, its timing
                     build: -O3 -march=native) followed by (a): the path callers have without the projector
  projector_gpu / projector_1core   eorb_project_frustum / _last_frame / _keyframe_points alone against the restatement alone

The calls of a shape take turns inside one loop, so that a drift of the clocks or of the shared host touches them alike.  Prints one
JSON object (and writes it to --out)."""
import argparse, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--M", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from eorb_slam_amd import frontend as fe, synth
    from twocam_latency import _sources_hash
    import proj_ref
    M = a.M
    res = {"sources_hash": _sources_hash(), "M": M, "shapes": {}}
    ctx = fe.Context()
    for (W, H, f) in ((346, 260, 280.0), (752, 480, 458.0)):
        for n in (1000, 2000):
            s = synth.map_scene(100 + n, M, W=W, H=H, f=f)
            kw = dict(R=s["R"], t=s["t"], Ow=s["Ow"], cam=s["cam"], bounds=s["bounds"], nlevels=s["nlevels"], log_scale=s["log_scale"],
                      scale_factors=s["scale_factors"], mbf=35.0)
            v, rv = fe.view(**kw), proj_ref.view(**kw)
            A = (s["pos"], s["normal"], s["min_dist"], s["max_dist"])
            mp_desc = synth.random_descriptors(M, seed=1); mp_obs = np.ones(M, np.uint8)
            m = fe.ORBmatcher(0.8, True, ctx)
            fns = {}
            # local points
            _, (r,) = proj_ref.frustum(rv, *A, timing=True)
            kps, desc, _ = synth.planted_frame(r["in_view"], r["proj_xy"], r["level"], mp_desc, n, W, H, seed=2)
            F = fe.FrameView(kps, desc, W, H); fm = np.full(n, -1, np.int32)

            def local_a(r=r):
                return m.SearchByProjectionMap(F, r["in_view"], r["proj_xy"], r["level"], r["view_cos"], mp_desc, mp_obs, fm, 1.0, r["level_scale"])

            def local_b():
                return local_a(proj_ref.frustum(rv, *A, timing=True)[1][0])
            fused = fe.SearchLocalPoints(F, v, *A, mp_desc, mp_obs, fm, th=1.0, nnratio=0.8, ctx=ctx)
            ref = local_b()
            assert fused[0] == ref[0] and np.array_equal(fused[1], ref[1]) and fused[0] > 0
            fns["local"] = {"fused": lambda: fe.SearchLocalPoints(F, v, *A, mp_desc, mp_obs, fm, th=1.0, nnratio=0.8, ctx=ctx),
                            "matcher_alone": local_a, "cpu_project_plus_matcher": local_b,
                            "projector_gpu": lambda: fe.isInFrustum(v, *A, ctx=ctx), "projector_1core": lambda: proj_ref.frustum(rv, *A, timing=True)}
            # last frame
            last_kps = synth.random_keypoints(M, W, H, nlevels=8, seed=3)
            rl = proj_ref.last_frame(rv, s["pos"], last_kps, timing=True)
            kps2, desc2, _ = synth.planted_frame(rl["valid"], rl["uv"], last_kps["octave"], mp_desc, n, W, H, seed=4, dlevel=(-1, 0, 1))
            Cur = fe.FrameView(kps2, desc2, W, H); Last = fe.FrameView(last_kps, np.zeros((M, 32), np.uint8), W, H)

            def last_a(r=rl):
                return m.SearchByProjectionLast(Cur, Last, r["valid"], r["uv"], mp_desc, mp_obs, fm, 7.0, r["level_scale"])

            def last_b():
                return last_a(proj_ref.last_frame(rv, s["pos"], last_kps, timing=True))
            fused = fe.SearchByProjectionLastPose(Cur, v, Last, s["pos"], mp_desc, mp_obs, fm, 7.0, ctx=ctx)
            ref = last_b()
            assert fused[0] == ref[0] and np.array_equal(fused[1], ref[1]) and fused[0] > 0
            fns["last"] = {"fused": lambda: fe.SearchByProjectionLastPose(Cur, v, Last, s["pos"], mp_desc, mp_obs, fm, 7.0, ctx=ctx),
                           "matcher_alone": last_a, "cpu_project_plus_matcher": last_b,
                           "projector_gpu": lambda: fe.ProjectLastFrame(v, s["pos"], last_kps, ctx=ctx),
                           "projector_1core": lambda: proj_ref.last_frame(rv, s["pos"], last_kps, timing=True)}
            # keyframe (relocalisation)
            rk = proj_ref.keyframe_points(rv, s["pos"], s["min_dist"], s["max_dist"], timing=True)
            kps3, desc3, _ = synth.planted_frame(rk["valid"], rk["uv"], rk["level"], mp_desc, n, W, H, seed=5, dlevel=(-1, 0, 1))
            Cur3 = fe.FrameView(kps3, desc3, W, H)

            def kf_a(r=rk):
                return m.SearchByProjectionKF(Cur3, last_kps, None, r["valid"], r["uv"], r["level"], r["level_scale"], mp_desc, fm, 10.0, 100)

            def kf_b():
                return kf_a(proj_ref.keyframe_points(rv, s["pos"], s["min_dist"], s["max_dist"], timing=True))
            fused = fe.SearchByProjectionKFPose(Cur3, v, last_kps, s["pos"], s["min_dist"], s["max_dist"], mp_desc, fm, 10.0, 100, ctx=ctx)
            ref = kf_b()
            assert fused[0] == ref[0] and np.array_equal(fused[1], ref[1]) and fused[0] > 0
            fns["kf"] = {"fused": lambda: fe.SearchByProjectionKFPose(Cur3, v, last_kps, s["pos"], s["min_dist"], s["max_dist"], mp_desc, fm, 10.0, 100, ctx=ctx),
                         "matcher_alone": kf_a, "cpu_project_plus_matcher": kf_b,
                         "projector_gpu": lambda: fe.ProjectKeyFramePoints(v, s["pos"], s["min_dist"], s["max_dist"], ctx=ctx),
                         "projector_1core": lambda: proj_ref.keyframe_points(rv, s["pos"], s["min_dist"], s["max_dist"], timing=True)}
            shape = {}
            for search, calls in fns.items():
                for _ in range(5):
                    for fn in calls.values():
                        fn()
                ts = {k: [] for k in calls}
                for _ in range(a.calls):
                    for k, fn in calls.items():
                        t = time.perf_counter(); fn(); ts[k].append((time.perf_counter() - t) * 1e3)
                e = {k: {"p50_ms": float(np.percentile(x, 50)), "p95_ms": float(np.percentile(x, 95)), "calls": len(x)} for k, x in ts.items()}
                e["fused_beats_cpu_path"] = bool(e["fused"]["p50_ms"] < e["cpu_project_plus_matcher"]["p50_ms"])
                e["projector_beats_one_core"] = bool(e["projector_gpu"]["p50_ms"] < e["projector_1core"]["p50_ms"])
                shape[search] = e
            res["shapes"]["%dx%d_n%d" % (W, H, n)] = shape
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
