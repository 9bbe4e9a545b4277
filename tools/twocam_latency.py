#!/usr/bin/env python3
"""Per-call latency of the two-camera entry points on a TUM-VI sized frame (512 x 512, 8 levels, 1 500 features per camera) and
the oracle's time for the same calls on one core (its timing build, -O3 -march=native, as bench.py's cpu_baseline).  Prints one JSON
object (and writes it to --out).

  eorb_frame_fisheye                      both extractions + knnMatch of the lapping rows + Lowe's test
  eorb_search_by_projection_map_fisheye   every keypoint of the frame as a map point, both cameras
  eorb_search_by_projection_last_fisheye  every point of a second frame as a query, mode 0, checkOri
  eorb_search_by_bow_fisheye              random feature vectors (120 nodes)

Run it under `rocprofv3 --kernel-trace --stats -d DIR -o twocam -- python tools/twocam_latency.py` for the kernel summary."""
import argparse, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _sources_hash():
    """hash of the library sources, as bench.py's source_hash()"""
    import glob, hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(ROOT, "eorb_slam_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "eorb_slam_amd", "csrc", "*.h")) +
                   [os.path.join(ROOT, "include", "eorb_fe.h")])
    for f in files:
        h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def _med(f, n):
    ts = []
    for _ in range(n):
        t = time.perf_counter(); f(); ts.append(time.perf_counter() - t)
    a = np.sort(np.array(ts)) * 1e3
    return {"p50_ms": float(np.percentile(a, 50)), "p95_ms": float(np.percentile(a, 95)), "calls": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--cpu-calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from eorb_slam_amd import frontend as fe, synth
    from oracle import oracle_py as oracle
    W = H = 512
    imL, imR = synth.image_pair(W, H, 5, (2, -7))
    imL2, imR2 = synth.image_pair(W, H, 5, (5, -3))
    ctx = fe.Context()
    ge = fe.ORBextractor(1500, 1.2, 8, 20, 7, 19, imSize=(W, H), ctx=ctx)
    oe = oracle.OrbExtractor(1500, 1.2, 8, 20, 7, edgeTh=19, fast=True)
    lap = (0, W - 1)

    def cpu_frame(l, r):
        mL, kL, dL, _ = oe.extract(l, lap); mR, kR, dR, _ = oe.extract(r, lap)
        n, cand, _ = oracle.fisheye_matches(dL, mL, dR, mR, fast=True)
        return kL, dL, kR, dR, cand

    kL, dL, kR, dR, cand = cpu_frame(imL, imR)
    kps = np.concatenate([kL, kR]); desc = np.concatenate([dL, dR]); nL = len(kL)
    l2r = cand.astype(np.int32); r2l = np.full(len(kR), -1, np.int32); r2l[l2r[l2r >= 0]] = np.nonzero(l2r >= 0)[0]
    lkL, ldL, lkR, ldR, _ = cpu_frame(imL2, imR2)
    lk = np.concatenate([lkL, lkR]); ld = np.concatenate([ldL, ldR])
    rng = np.random.default_rng(7)
    gb = oracle.grid_bounds(W, H)
    left, right, mp_desc, mp_obs = synth.map_inputs(kps, nL, oe.scale_factors, rng, src=(kps, desc))
    fm = np.full(len(kps), -1, np.int32)
    nq = len(lk)
    valid = np.ones(nq, np.uint8)
    uv = np.stack([lk["x"] - 3, lk["y"] - 5], axis=1).astype(np.float32); uv_r = (uv + np.float32([7, 0])).astype(np.float32)
    lobs = (rng.uniform(size=nq) < 0.7).astype(np.uint8)
    ls = oe.scale_factors[np.clip(lk["octave"], 0, 7)].astype(np.float32)
    cur = np.full(len(kps), -1, np.int32)
    kfv = synth.feature_vector_of(rng.integers(0, 120, len(lk)), rng)
    ffv = synth.feature_vector_of(rng.integers(0, 120, len(kps)), rng)
    has_mp = np.ones(len(lk), np.uint8)
    m = fe.ORBmatcher(0.8, True, ctx)
    calls = {
        "frame_fisheye": (lambda: ge.fisheye(imL, imR, lap, lap), lambda: cpu_frame(imL, imR)),
        "map_fisheye": (lambda: m.SearchByProjectionMapFisheye(kps, nL, desc, l2r, r2l, gb, left, right, mp_desc, mp_obs, fm, 1.0),
                        lambda: oracle.search_by_projection_map_fisheye(kps, nL, desc, gb, l2r, r2l, left, right, mp_desc, mp_obs, fm, 1.0, 0.8,
                                                                        fast=True)),
        "last_fisheye": (lambda: m.SearchByProjectionLastFisheye(kps, nL, desc, gb, lk, valid, uv, uv_r, ld, lobs, cur, 7.0, ls, 0),
                         lambda: oracle.search_by_projection_last_fisheye(kps, nL, desc, gb, lk, valid, uv, uv_r, ld, lobs, cur, 7.0, ls, 0, True,
                                                                          fast=True)),
        "bow_fisheye": (lambda: fe.SearchByBoWFisheye(lk, ld, has_mp, kfv, kps, nL, desc, ffv, 0.7, True, ctx=ctx),
                        lambda: oracle.search_by_bow_fisheye(lk, ld, has_mp, kfv, kps, nL, desc, ffv, 0.7, True, fast=True)),
    }
    res = {"frame": "512x512, 8 levels, 1500 features per camera", "nL": nL, "nR": len(kR), "queries_map": len(mp_obs),
           "queries_last": nq, "sources_hash": _sources_hash(), "gpu": {}, "oracle_1core": {}}
    for name, (g, c) in calls.items():
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
