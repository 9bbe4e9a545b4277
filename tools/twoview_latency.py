#!/usr/bin/env python3
"""Per-call latency (through ctypes, each call ends in its own wait) of eorb_two_view_ransac and eorb_two_view_check_rt against the CPU
restatement (tests/twoview_ref, its timing build -O3 -march=native, the same host, the same data): N = 100, 300 and 1 000 matches with
200 RANSAC iterations, CheckRT with 4 and 8 pose hypotheses.

    dev_ransac       eorb_two_view_ransac without the per-iteration aids, preallocated result arrays
    cpu_ransac_1t    tvr_ransac, FindHomography then FindFundamental on one core
    cpu_ransac_2t    the same as two threads, one each, as the reference runs them (:131-136); the threads are started per call, as there
    dev_rt4 / dev_rt8, cpu_rt4 / cpu_rt8    CheckRT for 4 / 8 poses over the matches the scene generated as correct

The device and the restatement take turns inside one loop; their results are compared as bytes before anything is timed.  The per-kernel
split of one device call comes from the library's own event timers (eorb_prof_*), in a pass of its own.  Prints one JSON object (and
writes it to --out).

--reconstruct times eorb_two_view_reconstruct instead (see reconstruct() below) and puts its object under the key "reconstruct" of --out."""
import argparse, ctypes as C, json, os, sys, threading, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
NS = (100, 300, 1000)
ITERS = 200


def _stats(x, np):
    return {"p50_ms": float(np.percentile(x, 50)), "p95_ms": float(np.percentile(x, 95)), "calls": len(x)}


def _time(calls, n, np, warm=5):
    """calls: name -> f(); they take turns inside one loop"""
    for _ in range(warm):
        for fn in calls.values():
            fn()
    ts = {k: [] for k in calls}
    for _ in range(n):
        for k, fn in calls.items():
            t = time.perf_counter(); fn(); ts[k].append((time.perf_counter() - t) * 1e3)
    return {k: _stats(x, np) for k, x in ts.items()}


def _canon(a, np):
    a = np.array(a)
    if a.dtype == np.float32:
        a[np.isnan(a)] = np.float32(np.nan)
    return a.tobytes()


def _prof(ctx, fn, n):
    """mean milliseconds per call of each timed scope over n calls"""
    L, h = ctx.L, ctx.h
    L.eorb_prof_enable(h, 1); L.eorb_prof_reset(h)
    for _ in range(n):
        fn()
    out = {}
    name, ms, cnt = C.c_char_p(), C.c_double(0), C.c_int64(0)
    for i in range(L.eorb_prof_count(h)):
        L.eorb_prof_get(h, i, C.byref(name), C.byref(ms), C.byref(cnt))
        if cnt.value:
            out[name.value.decode()] = ms.value / n
    L.eorb_prof_enable(h, 0)
    return out


def reconstruct(a):
    """--reconstruct: eorb_two_view_reconstruct (one call) against the two calls the library offered before it with the restated host algebra
    between and after them (eorb_two_view_ransac -> tvr_decide -> eorb_two_view_check_rt -> tvr_finish, the C of tests/twoview_ref through
    ctypes, preallocated arrays) and against the whole restatement on one core (tvr_reconstruct, timing build), both forms.  The three take
    turns inside one loop; the one call equals the restatement as bytes before anything is timed.  Returns the dict for the "reconstruct"
    key of the output."""
    import numpy as np
    from eorb_slam_amd import frontend as fe, _lib
    import twoview_ref as tv
    from twoview_ref import scenes, reconstruct_ref as rr
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731
    out = {"iterations": ITERS, "shapes": {}}
    ctx = fe.Context()
    L, h = ctx.L, ctx.h
    RL = rr.lib(timing=True)
    for N in a.sizes:
        sc = scenes.scene("mixed", N, seed=900 + N, extra1=N // 2, extra2=N // 2 + 17)
        k1, k2, m = sc["kps1"], sc["kps2"], sc["matches"]
        sets = scenes.make_sets(N, ITERS, seed=N)
        n1, n2 = len(k1), len(k2)
        p1, p2 = tv._pts(k1), tv._pts(k2)
        Kf = np.ascontiguousarray(scenes.K, np.float32)
        e = {"n1": n1, "n2": n2}
        for form, fname in ((_lib.TVR_FORM_STOCK, "stock"), (_lib.TVR_FORM_INFO, "info")):
            par = rr.params(form, cls=_lib.TvrReconParams); rpar = rr.params(form)
            g = fe.TwoViewReconstruction(scenes.K, ctx=ctx).reconstruct(k1, k2, m, sets, params=par, want_poses=True)
            r = rr.reconstruct(scenes.K, k1, k2, m, sets, rpar, timing=True)
            for key in r:
                assert _canon(g[key], np) == _canon(r[key], np), (N, fname, key)
            res = _lib.TvrReconResult(); R = np.zeros(18, np.float32); t = np.zeros(6, np.float32); p3 = np.zeros(6 * n1, np.float32)
            tri = np.zeros(2 * n1, np.uint8); ti = np.zeros(N, np.uint8)

            def one_call(par=par, res=res, R=R, t=t, p3=p3, tri=tri, ti=ti):
                rc = L.eorb_two_view_reconstruct(h, p(k1), n1, p(k2), n2, p(m), N, p(sets), ITERS, p(Kf), C.byref(par), C.byref(res), p(R), p(t), p(p3),
                                                 p(tri), p(ti), None)
                assert rc == 0, rc
            H = np.zeros(9, np.float32); F = np.zeros(9, np.float32); ih = np.zeros(N, np.uint8); jf = np.zeros(N, np.uint8)
            SH, SF, bh, bf = C.c_float(0), C.c_float(0), C.c_int(0), C.c_int(0)
            tp = _lib.TvrParams(1.0, 5.991, 3.841)
            r2 = rr.ReconResult(); po = np.zeros((8, 27), np.float32); sel = np.zeros(N, np.uint8); ti2 = np.zeros(N, np.uint8)
            ng = np.zeros(8, np.int32); gd = np.zeros(8 * n1, np.uint8); p8 = np.zeros(8 * n1 * 3, np.float32); cs = np.zeros(8, np.float32)
            R2 = np.zeros(18, np.float32); t2 = np.zeros(6, np.float32); p32 = np.zeros(6 * n1, np.float32); tri2 = np.zeros(2 * n1, np.uint8)
            th2 = float(np.float32(4.0) * np.float32(1.0))

            def two_calls(rpar=rpar, r2=r2):
                rc = L.eorb_two_view_ransac(h, p(k1), n1, p(k2), n2, p(m), N, p(sets), ITERS, C.byref(tp), p(H), C.byref(SH), C.byref(bh), p(ih), p(F),
                                            C.byref(SF), C.byref(bf), p(jf), None, None, None, None)
                assert rc == 0, rc
                nh = RL.tvr_decide(SH.value, SF.value, bh.value, bf.value, p(H), p(F), p(ih), p(jf), N, p(Kf), C.addressof(rpar), C.addressof(r2), p(po),
                                   p(sel), p(ti2))
                if nh:
                    rc = L.eorb_two_view_check_rt(h, p(k1), n1, p(k2), n2, p(m), N, p(sel), p(Kf), th2, rpar.min_parallax_crt, rpar.min_triangulated, p(po),
                                                  nh, p(ng), p(gd), p(p8), p(cs), None)
                    assert rc == 0, rc
                RL.tvr_finish(C.addressof(rpar), C.addressof(r2), p(po), n1, p(ng), p(cs), p(gd), p(p8), p(R2), p(t2), p(p32), p(tri2))
            r3 = rr.ReconResult(); R3 = R2.copy(); t3 = t2.copy(); p33 = p32.copy(); tri3 = tri2.copy(); ti3 = ti2.copy()

            def cpu_1t(rpar=rpar, r3=r3, R3=R3, t3=t3, p33=p33, tri3=tri3, ti3=ti3):
                RL.tvr_reconstruct(p(p1), n1, p(p2), n2, p(m), N, p(sets), ITERS, p(Kf), C.addressof(rpar), C.addressof(r3), p(R3), p(t3), p(p33), p(tri3),
                                   p(ti3), None)
            one_call(); two_calls()
            assert _canon(R, np) == _canon(R2, np) and _canon(p3, np) == _canon(p32, np) and tri.tobytes() == tri2.tobytes() and res.ok == r2.ok, (N, fname)
            s = _time({"one_call": one_call, "two_calls": two_calls, "cpu_1t": cpu_1t}, a.calls, np)
            s["two_calls_over_one_call"] = s["two_calls"]["p50_ms"] / s["one_call"]["p50_ms"]
            s["cpu_1t_over_one_call"] = s["cpu_1t"]["p50_ms"] / s["one_call"]["p50_ms"]
            s["ok"], s["is_homography"], s["n_hyp"] = int(res.ok), int(res.is_homography), int(res.n_hyp)
            s["kernels_ms"] = _prof(ctx, one_call, 20)
            e[fname] = s
        out["shapes"]["N%d" % N] = e
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(NS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--reconstruct", action="store_true", help="time eorb_two_view_reconstruct; the result goes under the key 'reconstruct' of --out, "
                    "whose other keys are kept")
    a = ap.parse_args()
    if a.reconstruct:
        from twocam_latency import _sources_hash
        res = {}
        if a.out and os.path.exists(a.out):
            res = json.loads(open(a.out).read())
        res["reconstruct"] = dict(reconstruct(a), sources_hash=_sources_hash())
        line = json.dumps(res)
        print(json.dumps(res["reconstruct"]))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write(line + "\n")
        return
    import numpy as np
    from eorb_slam_amd import frontend as fe, _lib
    import twoview_ref as tv
    from twoview_ref import scenes
    from twocam_latency import _sources_hash
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731
    res = {"iterations": ITERS, "sources_hash": _sources_hash(), "shapes": {}}
    ctx = fe.Context()
    L, h = ctx.L, ctx.h
    for N in a.sizes:
        sc = scenes.scene("mixed", N, seed=900 + N, extra1=N // 2, extra2=N // 2 + 17)
        k1, k2, m = sc["kps1"], sc["kps2"], sc["matches"]
        sets = scenes.make_sets(N, ITERS, seed=N)
        dev = fe.TwoViewReconstruction(scenes.K, ctx=ctx)
        ref = tv.TwoViewReconstruction(scenes.K, timing=True)
        # results equal as bytes before anything is timed
        g = dev.find_homography_fundamental(k1, k2, m, sets, aids=True); r = ref.find_homography_fundamental(k1, k2, m, sets, aids=True)
        for key in r:
            assert _canon(g[key], np) == _canon(r[key], np), (N, key)
        inl = (~sc["bad"]).astype(np.uint8)
        four = scenes.decompose_e_poses(sc["R"], sc["t"])
        poses = {4: scenes.poses27(four), 8: scenes.poses27(four + [(R, -t) for R, t in four])}
        for Kp, P in poses.items():
            g = dev.check_rt(k1, k2, m, inl, P, want_cos_all=True); r = ref.check_rt(k1, k2, m, inl, P, want_cos_all=True)
            for key in r:
                assert _canon(g[key], np) == _canon(r[key], np), (N, Kp, key)
        # the timed calls: raw ABI, preallocated outputs
        H = np.zeros(9, np.float32); F = np.zeros(9, np.float32); ih = np.zeros(N, np.uint8); jf = np.zeros(N, np.uint8)
        SH, SF, bh, bf = C.c_float(0), C.c_float(0), C.c_int(0), C.c_int(0)
        par = _lib.TvrParams(1.0, 5.991, 3.841)
        n1, n2 = len(k1), len(k2)

        def dev_ransac():
            rc = L.eorb_two_view_ransac(h, p(k1), n1, p(k2), n2, p(m), N, p(sets), ITERS, C.byref(par), p(H), C.byref(SH), C.byref(bh), p(ih), p(F),
                                        C.byref(SF), C.byref(bf), p(jf), None, None, None, None)
            assert rc == 0, rc
        prep = ref.prepare(k1, k2, m, sets)

        def cpu_ransac_1t():
            ref.run(prep, 3)

        def cpu_ransac_2t():
            th = threading.Thread(target=ref.run, args=(prep, 1)); tf = threading.Thread(target=ref.run, args=(prep, 2))
            th.start(); tf.start(); th.join(); tf.join()
        calls = {"dev_ransac": dev_ransac, "cpu_ransac_1t": cpu_ransac_1t, "cpu_ransac_2t": cpu_ransac_2t}
        Kf = np.ascontiguousarray(scenes.K, np.float32); mp = float(np.float32(0.99998))
        p1, p2 = tv._pts(k1), tv._pts(k2)
        for Kp, P in poses.items():
            ng = np.zeros(Kp, np.int32); gd = np.zeros(Kp * n1, np.uint8); p3 = np.zeros(Kp * n1 * 3, np.float32); cs = np.zeros(Kp, np.float32)

            def dev_rt(P=P, Kp=Kp, ng=ng, gd=gd, p3=p3, cs=cs):
                rc = L.eorb_two_view_check_rt(h, p(k1), n1, p(k2), n2, p(m), N, p(inl), p(Kf), 4.0, mp, 50, p(P), Kp, p(ng), p(gd), p(p3), p(cs), None)
                assert rc == 0, rc

            def cpu_rt(P=P, Kp=Kp, ng=ng.copy(), gd=gd.copy(), p3=p3.copy(), cs=cs.copy()):
                ref.L.tvr_check_rt(p(p1), n1, p(p2), n2, p(m), N, p(inl), p(Kf), 4.0, mp, 50, p(P), Kp, p(ng), p(gd), p(p3), p(cs), None)
            calls["dev_rt%d" % Kp] = dev_rt; calls["cpu_rt%d" % Kp] = cpu_rt
        e = _time(calls, a.calls, np)
        e["speedup_ransac_vs_1t"] = e["cpu_ransac_1t"]["p50_ms"] / e["dev_ransac"]["p50_ms"]
        e["speedup_ransac_vs_2t"] = e["cpu_ransac_2t"]["p50_ms"] / e["dev_ransac"]["p50_ms"]
        for Kp in poses:
            e["speedup_rt%d" % Kp] = e["cpu_rt%d" % Kp]["p50_ms"] / e["dev_rt%d" % Kp]["p50_ms"]
        e["n1"], e["n2"], e["inliers"] = n1, n2, int(inl.sum())
        e["kernels_ms_ransac"] = _prof(ctx, dev_ransac, 20)
        e["kernels_ms_rt8"] = _prof(ctx, calls["dev_rt8"], 20)
        res["shapes"]["N%d" % N] = e
    ctx.close()
    for key in ("ransac_vs_1t", "ransac_vs_2t", "rt4", "rt8"):
        faster = [N for N in a.sizes if res["shapes"]["N%d" % N]["speedup_" + key] > 1.0]
        res["device_faster_from_N_" + key] = min(faster) if faster else None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
