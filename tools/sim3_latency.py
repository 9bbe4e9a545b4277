#!/usr/bin/env python3
"""Per-call latency (through ctypes, preallocated arrays, each call ends in its own wait) of eorb_sim3_ransac against the CPU restatement
(tests/sim3_ref, its timing build -O3 -march=native -ffp-contract=off, one core of the same host, the same data): N = 50, 200 and 1 000
correspondences, 300 iterations, K = 1, 3 and 8 problems per call, on two scenes reported separately:

    converges   70 % of the correspondences correct: the reference stops at the first converging iteration (cpu = s3r_ransac with
                stop_early), the device computes all 300
    never       a false candidate, every correspondence wrong: both sides run all 300

The CPU solves the K problems one after the other, as LoopClosing does.  The device and the restatement take turns inside one loop; their
results are compared as bytes before anything is timed.  The per-kernel split of one device call comes from the library's own event
timers (eorb_prof_*), in a pass of its own.  The `chain` entry times the three device-side stages of DetectCommonRegionsFromBoW as calls
in a row (_chain below), with stage 2 on the device and on one core; --chain-only adds it to an existing --out file.  Prints one JSON
object (and writes it to --out)."""
import argparse, ctypes as C, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
NS = (50, 200, 1000)
KS = (1, 3, 8)
ITERS = 300
SCENES = {"converges": 0.3, "never": 1.0}
KEYS = ("converged", "best_it", "n_inliers", "iterations_used", "T12", "R12", "t12", "s12", "inliers")


def _chain(calls, np, fe, s3, scenes, ctx, _time, K=8, N=200):
    """The three device-side stages of DetectCommonRegionsFromBoW as calls in a row, with stage 2 on the device and on one core:
    eorb_search_by_bow_kf_keyframes over K candidates (the scene of tools/kfbatch_latency.py), the Sim3 solvers of those K candidates
    (one of them true, the others false: N correspondences each, 300 iterations), eorb_search_by_projection_kf_scw on one keyframe (the
    scene of tools/kfside_latency.py).  The stages run on their own synthetic inputs: what is timed is the calls, not a data flow."""
    from eorb_slam_amd import synth, _lib
    import kfside_latency as ks
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731
    b = synth.bow_neighbourhood(402, K, npts=1300, ndistract=150, nties=30, nnodes=250)
    S = fe.KeyFrameSet([(kf["kps"], kf["desc"], kf["has_mp"], kf["fv"]) for kf in b["kfs"][:K]])
    sc = synth.keyframe_neighbourhood(201, 1, 1000, n_kps=1000)
    gb = fe.grid_bounds(ks.W, ks.H)
    geom = (sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"])
    v0 = fe.view(**sc["views"][0])
    taken = np.zeros(1000, np.uint8)
    pbs = [scenes.scene(N, seed=5000 + k, pair="pp", wrong=0.3 if k == K // 2 else 1.0, iters=ITERS, min_inliers=max(6, N // 5)) for k in range(K)]
    dev = [scenes.solver(fe, pb, ctx=ctx) for pb in pbs]
    ref = [scenes.solver(s3, pb, timing=True) for pb in pbs]
    probs = (_lib.Sim3Problem * K)(*[s.problem(ITERS) for s in dev])
    Xw1 = np.concatenate([s.Xw1 for s in dev]); Xw2 = np.concatenate([s.Xw2 for s in dev])
    sg1 = np.concatenate([s.sigma2_1 for s in dev]); sg2 = np.concatenate([s.sigma2_2 for s in dev]); st = np.concatenate([pb["sets"] for pb in pbs])
    out = (_lib.Sim3Result * K)(); inl = np.zeros(K * N, np.uint8)
    preps = [s.prepare(pb["sets"], aids=False) for s, pb in zip(ref, pbs)]

    def stage1():
        fe.SearchByBoW_KF_KeyFrames(b["kps"], b["desc"], b["has_mp"], b["fv"], S, 0.8, True, ctx=ctx)

    def stage2_dev():
        assert ctx.L.eorb_sim3_ransac(ctx.h, probs, K, p(Xw1), p(Xw2), p(sg1), p(sg2), p(st), out, p(inl), None, None, None, None) == 0

    def stage2_cpu():
        for s, pr in zip(ref, preps):
            s.run(pr, stop_early=True)

    def stage3():
        fe.SearchByProjectionKFScw(sc["kps"][0], sc["desc"][0], gb, v0, *geom, sc["mp_desc"], taken.copy(), 3.0, ctx=ctx)
    e = _time({"chain_dev": lambda: (stage1(), stage2_dev(), stage3()), "chain_cpu_stage2": lambda: (stage1(), stage2_cpu(), stage3()),
               "stage1_bow_kf_keyframes": stage1, "stage2_dev": stage2_dev, "stage2_cpu_1t": stage2_cpu, "stage3_kf_scw": stage3}, calls, np)
    e["K"], e["N"] = K, N
    e["saving_ms"] = e["chain_cpu_stage2"]["p50_ms"] - e["chain_dev"]["p50_ms"]
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--chain-only", action="store_true", help="time only the three-stage chain (the `chain` entry of the profile)")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(NS))
    ap.add_argument("--problems", type=int, nargs="*", default=list(KS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from eorb_slam_amd import frontend as fe, _lib
    import sim3_ref as s3
    from sim3_ref import scenes
    from twoview_latency import _time, _canon, _prof
    from twocam_latency import _sources_hash
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731
    res = {"iterations": ITERS, "sources_hash": _sources_hash(), "shapes": {}}
    ctx = fe.Context()
    L, h = ctx.L, ctx.h
    if a.chain_only and a.out and os.path.exists(a.out):
        res = json.load(open(a.out))                                      # (the shapes of an earlier run stay; the chain is added to them)
    for name, wrong in ({} if a.chain_only else SCENES).items():
        for N in a.sizes:
            for K in a.problems:
                pbs = [scenes.scene(N, seed=1000 * N + 10 * K + k, pair=("pp", "kk", "pk")[k % 3], wrong=wrong, iters=ITERS, min_inliers=max(6, N // 5))
                       for k in range(K)]
                dev = [scenes.solver(fe, pb, ctx=ctx) for pb in pbs]
                ref = [scenes.solver(s3, pb, timing=True) for pb in pbs]
                sets = [pb["sets"] for pb in pbs]
                # results equal as bytes before anything is timed
                g = fe.Sim3Solver.solve_candidates(dev, sets, aids=False, ctx=ctx)
                r = [s.find(st) for s, st in zip(ref, sets)]
                for k in range(K):
                    for key in KEYS:
                        assert _canon(g[k][key], np) == _canon(r[k][key], np), (name, N, K, k, key)
                    assert r[k]["converged"] == (wrong < 1.0), (name, N, K, k)
                # the timed calls: raw ABI, preallocated outputs
                probs = (_lib.Sim3Problem * K)(*[s.problem(ITERS) for s in dev])
                Xw1 = np.concatenate([s.Xw1 for s in dev]); Xw2 = np.concatenate([s.Xw2 for s in dev])
                sg1 = np.concatenate([s.sigma2_1 for s in dev]); sg2 = np.concatenate([s.sigma2_2 for s in dev]); st = np.concatenate(sets)
                out = (_lib.Sim3Result * K)(); inl = np.zeros(K * N, np.uint8)

                def dev_call():
                    rc = L.eorb_sim3_ransac(h, probs, K, p(Xw1), p(Xw2), p(sg1), p(sg2), p(st), out, p(inl), None, None, None, None)
                    assert rc == 0, rc
                preps = [s.prepare(x, aids=False) for s, x in zip(ref, sets)]

                def cpu_call():
                    for s, pr in zip(ref, preps):
                        s.run(pr, stop_early=True)
                e = _time({"dev": dev_call, "cpu_1t": cpu_call}, a.calls, np)
                e["speedup"] = e["cpu_1t"]["p50_ms"] / e["dev"]["p50_ms"]
                e["cpu_iterations"] = [int(x["iterations_used"]) for x in r]
                e["kernels_ms"] = _prof(ctx, dev_call, 20)
                res["shapes"]["%s_N%d_K%d" % (name, N, K)] = e
    res["chain"] = _chain(a.calls, np, fe, s3, scenes, ctx, _time)
    ctx.close()
    for name in ({} if a.chain_only else SCENES):
        faster = sorted((N, K) for N in a.sizes for K in a.problems if res["shapes"]["%s_N%d_K%d" % (name, N, K)]["speedup"] > 1.0)
        res["device_faster_at_" + name] = faster
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
