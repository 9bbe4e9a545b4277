#!/usr/bin/env python3
"""Per-call latency (through ctypes, each call ends in its own wait) of the device KeyFrameDatabase queries against the CPU restatement of
the reference's (tests/kfdb_ref, its timing build -O3 -march=native, one core of the same host, the same data): 100, 1 000 and 5 000
keyframes of about 1 000 words, a query of about 1 000 words, places of about 25 keyframes.

    dev_reloc / dev_nbest    eorb_kfdb_detect_reloc / eorb_kfdb_detect_nbest with the covisibility table, cap = n_slots (what the C++ mirror
                             passes), preallocated result arrays
    dev_reloc_cap256         the same with cap = 256: the download is the counters and 256 entries per array, not n_slots
    cpu_reloc / cpu_nbest    kfdb_ref's DetectRelocalizationCandidates / DetectNBestCandidates.  Its BowVectors are sorted arrays and its
                             lists hold slot numbers: it is no slower than the reference's std::map and pointer chasing
    dev_add / cpu_add        one add() of one keyframe (the erase that keeps the database at its size is not timed)

The device and the restatement take turns inside one loop, over eight query vectors of different places; their results are compared as
bytes before anything is timed.  Prints one JSON object (and writes it to --out)."""
import argparse, ctypes as C, json, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
KS = (100, 1000, 5000)
WORDS, NQ = 1000, 8


def _stats(x, np):
    return {"p50_ms": float(np.percentile(x, 50)), "p95_ms": float(np.percentile(x, 95)), "calls": len(x)}


def _time(calls, n, np, warm=5):
    """calls: name -> f(i); they take turns inside one loop"""
    for i in range(warm):
        for fn in calls.values():
            fn(i)
    ts = {k: [] for k in calls}
    for i in range(n):
        for k, fn in calls.items():
            t = time.perf_counter(); fn(i); ts[k].append((time.perf_counter() - t) * 1e3)
    return {k: _stats(x, np) for k, x in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(KS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from eorb_slam_amd import frontend as fe, synth
    import kfdb_ref
    from twocam_latency import _sources_hash
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731
    res = {"words_per_keyframe": WORDS, "query_words": WORDS, "sources_hash": _sources_hash(), "shapes": {}}
    for K in a.sizes:
        nplaces = max(K // 25, 2)
        d = synth.bow_database(500 + K, K, vocab_words=max(2 * WORDS * nplaces, 100000), words_per_kf=WORDS, nplaces=nplaces, nqueries=NQ)
        ctx = fe.Context()
        dev = fe.KeyFrameDatabase(ctx)
        ref = kfdb_ref.KeyFrameDatabase(d["vocab_words"], timing=True)
        for k0 in range(0, K, 256):
            got = dev.add_many(d["kfs"][k0:k0 + 256]).tolist()
            assert got == [ref.add(w, v) for w, v in d["kfs"][k0:k0 + 256]]
        covis = np.ascontiguousarray(d["covis"], np.int32)
        qs = [(np.ascontiguousarray(q["word"], np.uint32), np.ascontiguousarray(q["val"], np.float64)) for q in d["queries"]]
        ex = []
        for q in d["queries"]:
            e = np.zeros(K, np.uint8); e[np.flatnonzero(d["place"] == q["place"])[:10]] = 1
            ex.append(e)
        # results equal as bytes, the stored scores included, before anything is timed
        shape = {"n_listed": [], "n_scored": []}
        for (w, v), e in zip(qs, ex):
            for nb in (0, 1):
                r = ref.detect_nbest_candidates(w, v, e, covis) if nb else ref.detect_relocalization_candidates(w, v, covis)
                g = dev.detect_nbest_candidates(w, v, e, covis) if nb else dev.detect_relocalization_candidates(w, v, covis)
                r.pop("stale")
                assert sorted(r) == sorted(g)
                for key in r:
                    assert np.asarray(r[key]).tobytes() == np.asarray(g[key]).tobytes(), (K, nb, key)
                assert dev.scores(nb).tobytes() == ref.scores(nb).tobytes()
            shape["n_listed"].append(r["n_listed"]); shape["n_scored"].append(r["n_scored"])
        L, h = ctx.L, ctx.h

        def outs(m):
            i32 = lambda: np.zeros(m, np.int32)      # noqa: E731
            f32 = lambda: np.zeros(m, np.float32)    # noqa: E731
            return dict(slot=i32(), si=f32(), words=i32(), acc=f32(), best=i32(), keep=np.zeros(m, np.uint8), sacc=f32(), sbest=i32())
        o, o256 = outs(K), outs(256)
        cnt = [C.c_int(0) for _ in range(3)]; ba = C.c_float(0); st = C.c_int(0)
        tail = [C.byref(x) for x in cnt] + [C.byref(ba)]

        def dev_reloc(i, o=o, cap=K):
            w, v = qs[i % NQ]
            rc = L.eorb_kfdb_detect_reloc(h, len(w), p(w), p(v), p(covis), cap, p(o["slot"]), p(o["si"]), p(o["words"]), p(o["acc"]), p(o["best"]),
                                          p(o["keep"]), *tail)
            assert rc == 0, rc

        def dev_nbest(i):
            w, v = qs[i % NQ]
            rc = L.eorb_kfdb_detect_nbest(h, len(w), p(w), p(v), p(ex[i % NQ]), p(covis), K, p(o["slot"]), p(o["si"]), p(o["words"]), p(o["acc"]),
                                          p(o["best"]), p(o["sacc"]), p(o["sbest"]), *tail)
            assert rc == 0, rc
        R, rh = ref.L, ref.h
        ro = outs(K)

        def cpu_reloc(i):
            w, v = qs[i % NQ]
            R.kr_detect_reloc(rh, len(w), p(w), p(v), p(covis), K, p(ro["slot"]), p(ro["si"]), p(ro["words"]), p(ro["acc"]), p(ro["best"]), p(ro["keep"]),
                              *tail, C.byref(st))

        def cpu_nbest(i):
            w, v = qs[i % NQ]
            R.kr_detect_nbest(rh, len(w), p(w), p(v), p(ex[i % NQ]), p(covis), K, p(ro["slot"]), p(ro["si"]), p(ro["words"]), p(ro["acc"]), p(ro["best"]),
                              p(ro["sacc"]), p(ro["sbest"]), *tail, C.byref(st))
        calls = {"dev_reloc": dev_reloc, "dev_nbest": dev_nbest, "cpu_reloc": cpu_reloc, "cpu_nbest": cpu_nbest}
        if max(shape["n_scored"]) <= 256:
            calls["dev_reloc_cap256"] = lambda i: dev_reloc(i, o256, 256)
        e = _time(calls, a.calls, np)
        # one add(pKF): the last keyframe leaves and comes back (same slot)
        w, v = np.ascontiguousarray(d["kfs"][K - 1][0], np.uint32), np.ascontiguousarray(d["kfs"][K - 1][1], np.float64)
        off = np.array([0, len(w)], np.int32); slot = np.zeros(1, np.int32)
        ta, tc = [], []
        for i in range(min(a.calls, 100) + 5):
            dev.erase(K - 1); ref.erase(K - 1)
            t = time.perf_counter(); rc = L.eorb_kfdb_add(h, 1, p(off), p(w), p(v), p(slot)); ta.append((time.perf_counter() - t) * 1e3)
            assert rc == 0 and slot[0] == K - 1
            t = time.perf_counter(); s = R.kr_add(rh, len(w), p(w), p(v)); tc.append((time.perf_counter() - t) * 1e3)
            assert s == K - 1
        e["dev_add"], e["cpu_add"] = _stats(ta[5:], np), _stats(tc[5:], np)
        e["n_listed_mean"] = float(np.mean(shape["n_listed"])); e["n_scored_mean"] = float(np.mean(shape["n_scored"]))
        e["n_scored_max"] = int(max(shape["n_scored"]))
        for q in ("reloc", "nbest"):
            e["speedup_" + q] = e["cpu_" + q]["p50_ms"] / e["dev_" + q]["p50_ms"]
        res["shapes"]["K%d" % K] = e
        ctx.close()
    faster = [K for K in a.sizes if res["shapes"]["K%d" % K]["speedup_reloc"] > 1.0 and res["shapes"]["K%d" % K]["speedup_nbest"] > 1.0]
    res["device_faster_from_K"] = min(faster) if faster else None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
