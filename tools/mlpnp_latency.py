#!/usr/bin/env python3
"""Per-call latency (through ctypes, preallocated arrays, each call ends in its own wait) of eorb_mlpnp_ransac against the CPU restatement
(tests/mlpnp_ref, its timing build -O3 -march=native -ffp-contract=off, one core of the same host, the same data): N = 30, 100 and 500
correspondences, 300 iterations, K = 1, 3 and 8 problems per call, on two scenes reported separately:

    refines     70 % of the matches correct: the reference stops at the first iteration whose Refine succeeds (cpu = mlr_ransac with
                stop_early), the device computes all 300 hypotheses
    never       a false candidate, every match wrong: both sides run all 300

The CPU solves the K problems one after the other, as Relocalization does.  The device and the restatement take turns inside one loop;
their results are compared as bytes before anything is timed.  The restatement keeps the computePose of Refine, whose result the reference
never stores, because the reference spends that time; the device does not compute it.  The per-kernel split of one device call comes from the library's own event
timers (eorb_prof_*), in a pass of its own.  The `chain` entry times the three device-side stages of Tracking::Relocalization as calls in
a row (_chain below), with stage 2 on the device and on one core.  Prints one JSON object (and writes it to --out)."""
import argparse, ctypes as C, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
NS = (30, 100, 500)
KS = (1, 3, 8)
ITERS = 300
SCENES = {"refines": 0.3, "never": 1.0}
KEYS = ("stop_it", "iterations_used", "best_it", "n_best", "refined", "n_inliers", "Tcw", "inliers")


def _arrays(np, _lib, dev, pbs):
    K = len(dev)
    return dict(probs=(_lib.MlpnpProblem * K)(*[s.problem(ITERS) for s in dev]), p2d=np.concatenate([s.p2d for s in dev]),
                Xw=np.concatenate([s.Xw for s in dev]), sg=np.concatenate([s.sigma2 for s in dev]), st=np.concatenate([pb["sets"] for pb in pbs]),
                out=(_lib.MlpnpResult * K)(), inl=np.zeros(sum(s.N for s in dev), np.uint8))


def _chain(calls, np, fe, mr, scenes, ctx, _time, K=8, N=100):
    """The three device-side stages of Tracking::Relocalization as calls in a row, with stage 2 on the device and on one core:
    eorb_search_by_bow_keyframes over K candidates (the scene of tools/kfbatch_latency.py), the MLPnP solvers of those K candidates (one
    of them true, the others false: N matches each, 300 iterations), eorb_search_by_projection_kf_pose on one keyframe (the scene of
    tools/project_latency.py).  The stages run on their own synthetic inputs: what is timed is the calls, not a data flow."""
    from eorb_slam_amd import synth, _lib
    import proj_ref
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731
    b = synth.bow_neighbourhood(402, K, npts=1300, ndistract=150, nties=30, nnodes=250)
    S = fe.KeyFrameSet([(kf["kps"], kf["desc"], kf["has_mp"], kf["fv"]) for kf in b["kfs"][:K]])
    W, H, M, n = 752, 480, 2000, 1000
    s = synth.map_scene(100 + n, M, W=W, H=H, f=458.0)
    kw = dict(R=s["R"], t=s["t"], Ow=s["Ow"], cam=s["cam"], bounds=s["bounds"], nlevels=s["nlevels"], log_scale=s["log_scale"],
              scale_factors=s["scale_factors"], mbf=35.0)
    v, rv = fe.view(**kw), proj_ref.view(**kw)
    mp_desc = synth.random_descriptors(M, seed=1)
    last_kps = synth.random_keypoints(M, W, H, nlevels=8, seed=3)
    rk = proj_ref.keyframe_points(rv, s["pos"], s["min_dist"], s["max_dist"], timing=True)
    kps3, desc3, _ = synth.planted_frame(rk["valid"], rk["uv"], rk["level"], mp_desc, n, W, H, seed=5, dlevel=(-1, 0, 1))
    Cur3 = fe.FrameView(kps3, desc3, W, H); fm = np.full(n, -1, np.int32)
    pbs = [scenes.scene(N, seed=5000 + k, cam="p", wrong=0.3 if k == K // 2 else 1.0, iters=ITERS) for k in range(K)]
    dev = [scenes.solver(fe, pb, ctx=ctx) for pb in pbs]
    ref = [scenes.solver(mr, pb, timing=True) for pb in pbs]
    A = _arrays(np, _lib, dev, pbs)

    def stage1():
        fe.SearchByBoWKeyFrames(S, b["kps"], b["desc"], b["fv"], 0.7, True, ctx=ctx)

    def stage2_dev():
        assert ctx.L.eorb_mlpnp_ransac(ctx.h, A["probs"], K, p(A["p2d"]), p(A["Xw"]), p(A["sg"]), p(A["st"]), A["out"], p(A["inl"]), None, None, None) == 0

    preps = [sv.prepare(pb["sets"]) for sv, pb in zip(ref, pbs)]

    def stage2_cpu():
        for sv, pr in zip(ref, preps):
            sv.run(pr, stop_early=True)

    def stage3():
        fe.SearchByProjectionKFPose(Cur3, v, last_kps, s["pos"], s["min_dist"], s["max_dist"], mp_desc, fm, 10.0, 100, ctx=ctx)
    e = _time({"chain_dev": lambda: (stage1(), stage2_dev(), stage3()), "chain_cpu_stage2": lambda: (stage1(), stage2_cpu(), stage3()),
               "stage1_bow_keyframes": stage1, "stage2_dev": stage2_dev, "stage2_cpu_1t": stage2_cpu, "stage3_kf_pose": stage3}, calls, np)
    e["K"], e["N"] = K, N
    e["saving_ms"] = e["chain_cpu_stage2"]["p50_ms"] - e["chain_dev"]["p50_ms"]
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--no-chain", action="store_true", help="skip the three-stage chain")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(NS))
    ap.add_argument("--problems", type=int, nargs="*", default=list(KS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from eorb_slam_amd import frontend as fe, _lib
    import mlpnp_ref as mr
    from mlpnp_ref import scenes
    from twoview_latency import _time, _canon, _prof
    from twocam_latency import _sources_hash
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731
    res = {"iterations": ITERS, "sources_hash": _sources_hash(), "shapes": {}}
    ctx = fe.Context()
    L, h = ctx.L, ctx.h
    for name, wrong in SCENES.items():
        for N in a.sizes:
            for K in a.problems:
                pbs = [scenes.scene(N, seed=1000 * N + 10 * K + k, cam="pk"[k % 2], wrong=wrong, iters=ITERS) for k in range(K)]
                dev = [scenes.solver(fe, pb, ctx=ctx) for pb in pbs]
                ref = [scenes.solver(mr, pb, timing=True) for pb in pbs]
                sets = [pb["sets"] for pb in pbs]
                # results equal as bytes before anything is timed
                g = fe.MLPnPsolver.solve_candidates(dev, sets, aids=False, ctx=ctx)
                r = [sv.find(st, stop_early=True) for sv, st in zip(ref, sets)]
                for k in range(K):
                    for key in KEYS:
                        assert _canon(g[k][key], np) == _canon(r[k][key], np), (name, N, K, k, key)
                    assert r[k]["refined"] == (wrong < 1.0), (name, N, K, k)
                A = _arrays(np, _lib, dev, pbs)

                def dev_call():
                    rc = L.eorb_mlpnp_ransac(h, A["probs"], K, p(A["p2d"]), p(A["Xw"]), p(A["sg"]), p(A["st"]), A["out"], p(A["inl"]), None, None, None)
                    assert rc == 0, rc

                preps = [sv.prepare(st) for sv, st in zip(ref, sets)]

                def cpu_call():
                    for sv, pr in zip(ref, preps):
                        sv.run(pr, stop_early=True)
                e = _time({"dev": dev_call, "cpu_1t": cpu_call}, a.calls, np)
                e["speedup"] = e["cpu_1t"]["p50_ms"] / e["dev"]["p50_ms"]
                e["cpu_iterations"] = [int(x["iterations_used"]) for x in r]
                e["kernels_ms"] = _prof(ctx, dev_call, 20)
                res["shapes"]["%s_N%d_K%d" % (name, N, K)] = e
    if not a.no_chain:
        res["chain"] = _chain(a.calls, np, fe, mr, scenes, ctx, _time)
    ctx.close()
    for name in SCENES:
        faster = sorted((N, K) for N in a.sizes for K in a.problems if res["shapes"]["%s_N%d_K%d" % (name, N, K)]["speedup"] > 1.0)
        res["device_faster_at_" + name] = faster
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
