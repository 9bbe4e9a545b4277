#!/usr/bin/env python3
"""Per-call latency (p50 through ctypes) of the calibrator's device calls, and the CPU restatement's time for the same work on one
core of the same host (tests/calib_ref/calib_ref.c, its timing build: -O3 -march=native).  Prints one JSON object (and writes it
to --out).

  maps        eorb_generate_undistort_maps with both maps downloaded, and without ("install"): 240 x 180 (EvETHZ pinhole),
              346 x 260 (MVSEC fisheye), 752 x 480 (EuRoC pinhole)
  keypoints   eorb_undistort_keypoints at 400 and 2 000 points (EvETHZ pinhole, MVSEC fisheye)
  frame       eorb_frame_mono against eorb_orb_extract alone and against eorb_orb_extract + eorb_undistort_keypoints on its output, the
              same texture frames in the same run: 240 x 180 x 4 levels, 752 x 480 x 8 levels
"""
import argparse, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--cpu-calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from eorb_slam_amd import frontend as fe, synth
    from twocam_latency import _med, _sources_hash
    import calib_ref
    CAL = synth.CALIBRATIONS
    res = {"sources_hash": _sources_hash(), "maps": {}, "keypoints": {}, "frame": {}}
    ctx = fe.Context()
    for name in ("EvETHZ", "MVSEC_KB8", "EuRoC"):
        d = CAL[name]
        W, H = d["size"]
        cal = fe.MyCalibrator.from_dict(d, ctx=ctx)
        mx, my = cal.generateUndistMaps()
        rx, ry = calib_ref.generate_maps(d, W, H, timing=True)
        assert mx.tobytes() == rx.tobytes() and my.tobytes() == ry.tobytes()
        for _ in range(3):
            cal.generateUndistMaps()
        res["maps"]["%s_%dx%d" % (name, W, H)] = {
            "gpu_download": _med(lambda: cal.generateUndistMaps(), a.calls),
            "gpu_install": _med(lambda: cal.generateUndistMaps(download=False), a.calls),
            "restatement_1core": _med(lambda: calib_ref.generate_maps(d, W, H, timing=True), a.cpu_calls)}
    for name in ("EvETHZ", "MVSEC_KB8"):
        d = CAL[name]
        W, H = d["size"]
        cal = fe.MyCalibrator.from_dict(d, ctx=ctx)
        for n in (400, 2000):
            kps = synth.calib_keypoints(n, W, H, seed=n)
            assert cal.undistKeyPoints(kps).tobytes() == calib_ref.undistort_keypoints(d, kps, timing=True).tobytes()
            for _ in range(3):
                cal.undistKeyPoints(kps)
            res["keypoints"]["%s_%d" % (name, n)] = {"gpu": _med(lambda: cal.undistKeyPoints(kps), a.calls),
                                                     "restatement_1core": _med(lambda: calib_ref.undistort_keypoints(d, kps, timing=True), max(a.cpu_calls, 50))}
    ctx.close()
    for name, nlev, nfeat in (("EvETHZ", 4, 1000), ("EuRoC", 8, 1500)):
        d = CAL[name]
        W, H = d["size"]
        ex = fe.ORBextractor(nfeat, 1.2, nlev, 20, 7, 19, (W, H))
        cal = fe.MyCalibrator.from_dict(d, ctx=ex.ctx)
        imgs = [synth.texture_image(W, H, seed=s) for s in (3, 4, 5, 6)]
        k = [0]

        def nxt():
            k[0] += 1
            return imgs[k[0] % len(imgs)]

        def both():
            _, kps, _, _ = ex(nxt())
            return cal.undistKeyPoints(kps)
        r = ex.frame_mono(imgs[0])
        assert r["kps_un"].tobytes() == calib_ref.undistort_keypoints(d, r["kps"]).tobytes()
        for _ in range(5):
            ex(nxt()); ex.frame_mono(nxt()); both()
        # the three calls take turns, so that a drift of the clocks or of the shared host touches them alike
        import time
        fns = {"orb_extract": lambda: ex(nxt()), "frame_mono": lambda: ex.frame_mono(nxt()), "orb_extract_plus_undistort": both}
        ts = {kk: [] for kk in fns}
        for _ in range(a.calls):
            for kk, fn in fns.items():
                t = time.perf_counter(); fn(); ts[kk].append((time.perf_counter() - t) * 1e3)
        res["frame"]["%s_%dx%dx%d" % (name, W, H, nlev)] = dict(
            {kk: {"p50_ms": float(np.percentile(v, 50)), "p95_ms": float(np.percentile(v, 95)), "calls": len(v)} for kk, v in ts.items()},
            keypoints=len(r["kps"]))
        f = res["frame"]["%s_%dx%dx%d" % (name, W, H, nlev)]
        f["fused_is_cheaper"] = bool(f["frame_mono"]["p50_ms"] < f["orb_extract_plus_undistort"]["p50_ms"])
        ex.ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    bad = [kk for kk, v in res["frame"].items() if not v["fused_is_cheaper"]]
    if bad:
        sys.exit("eorb_frame_mono is not cheaper than eorb_orb_extract + eorb_undistort_keypoints: %s" % ", ".join(bad))


if __name__ == "__main__":
    main()
