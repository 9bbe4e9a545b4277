#!/usr/bin/env python3
"""Per-call latency of eorb_search_for_triangulation_kb8 (SearchForTriangulation with a KannalaBrandt8 pCamera1) and the KB8
oracle's time for the same call on one core (its timing build, -O3 -march=native, as bench.py's cpu_baseline).  Prints one JSON
object (and writes it to --out).

  twocam   two-camera keyframes on 512 x 512 (about 1 000 left + 1 000 right features per keyframe), bCoarse = 0, checkOri
  mono     monocular keyframes on 346 x 260 (MVSEC sized, about 1 500 features per keyframe), bCoarse = 0, checkOri

The keyframe pairs are synth.keyframe_pair's scenes (3D points seen by both keyframes, near-duplicate descriptors, distractors).
Run it under `rocprofv3 --kernel-trace --stats -d DIR -o kb8tri -- python tools/kb8tri_latency.py` for the kernel summary."""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--cpu-calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from eorb_slam_amd import frontend as fe, synth
    from oracle import oracle_py as oracle
    from twocam_latency import _med, _sources_hash
    ctx = fe.Context()
    scenes = {"twocam": synth.keyframe_pair(seed=40, twocam=True, npts=980, ndistract=260, nnodes=250),
              "mono": synth.keyframe_pair(seed=41, npts=1950, ndistract=230, nnodes=250)}
    res = {"sources_hash": _sources_hash(), "sizes": {}, "gpu": {}, "oracle_1core": {}}
    for name, s in scenes.items():
        def g():
            return fe.SearchForTriangulationKB8(s["kps1"], s["nleft1"], s["desc1"], s["elig1"], s["fv1"], s["kps2"], s["nleft2"],
                                                s["desc2"], s["elig2"], s["fv2"], s["cams1"], s["cams2"], s["Rt"], s["ep"], s["scale2"],
                                                s["sigma2_1"], s["sigma2_2"], False, True, ctx=ctx)

        def c():
            return oracle.search_for_triangulation_kb8(**s, coarse=False, checkOri=True, fast=True)
        gn, _ = g()
        on, _ = c()
        assert gn == on
        res["sizes"][name] = {"n1": len(s["kps1"]), "n2": len(s["kps2"]), "nleft1": int(s["nleft1"]), "nleft2": int(s["nleft2"]),
                              "nmatches": int(gn)}
        for _ in range(3):
            g()
        res["gpu"][name] = _med(g, a.calls)
        if a.cpu_calls:
            res["oracle_1core"][name] = _med(c, a.cpu_calls)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
