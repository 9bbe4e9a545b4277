"""The C++ mirror of the KeyFrameDatabase (ORB_SLAM3::KeyFrameDatabase, eorb_slam_amd/host/eorb_host.hpp) from a plain g++ caller
(tests/host/kfdb_check.cpp): it must compile and link against libeorb_fe.so, and on a GPU box the candidate slots it returns -- the device
queries plus the caller-side tail: map test, isBad(), the already-added set, nNumCandidates -- equal those of the restatement
(tests/kfdb_ref) with the same tail written out here, on a model with three maps (one of them bad) and bad keyframes."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfdb_ref                                     # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, NUM, AGAIN, BAD_MAP = 40, 3, 5, 2


def _build(tmp):
    from eorb_slam_amd import _lib
    lib = _lib.build()
    exe = os.path.join(tmp, "kfdb_check")
    libdir = os.path.dirname(lib)
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "host", "kfdb_check.cpp"), "-o", exe, "-L", libdir,
                        "-leorb_fe", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_database_mirror_compiles_and_links(tmp_path):
    exe = _build(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "linked" in out.stdout


def _reloc_tail(r, kf_map, qmap):
    """:873-892"""
    out, seen = [], set()
    for b, keep in zip(r["best_slot"].tolist(), r["keep"].tolist()):
        if keep and kf_map[b] == qmap and b not in seen:
            out.append(b); seen.add(b)
    return out


def _nbest_tail(r, kf_map, kf_bad, qmap, stats):
    """:731-752, a bad keyframe skipped"""
    loop, merge, seen = [], [], set()
    for b in r["sorted_best_slot"].tolist():
        if not (len(loop) < NUM or len(merge) < NUM):
            break
        if kf_bad[b]:
            stats["bad"] += 1
            continue
        if b in seen:
            stats["dup"] += 1
            continue
        if kf_map[b] == qmap and len(loop) < NUM:
            loop.append(b)
        elif kf_map[b] != qmap and len(merge) < NUM:
            if kf_map[b] != BAD_MAP:
                merge.append(b)
            else:
                stats["badmap"] += 1
        seen.add(b)
    return loop, merge


def model():
    d = synth.bow_database(42, K, vocab_words=200, words_per_kf=80, nplaces=2, nqueries=3, p_place=0.9, kf_words=[80] * K)
    kf_map = (np.arange(K) % 3).astype(np.int32)
    covis = d["covis"].copy()
    db = kfdb_ref.KeyFrameDatabase(d["vocab_words"])
    for w, v in d["kfs"]:
        db.add(w, v)
    db.erase(AGAIN)
    assert db.add(*d["kfs"][AGAIN]) == AGAIN
    q_map = [0, 1, 0]
    conn = [[1, 4], [], [7, 8, 9]]
    # the bad keyframes: the head of the first query's sorted list and one more of its entries, so that the walk has to pass them
    ex = np.zeros(K, np.uint8); ex[conn[0]] = 1
    probe = kfdb_ref.KeyFrameDatabase(d["vocab_words"])
    for w, v in d["kfs"]:
        probe.add(w, v)
    head = probe.detect_nbest_candidates(d["queries"][0]["word"], d["queries"][0]["val"], exclude=ex, covis=covis)["sorted_best_slot"]
    kf_bad = np.zeros(K, np.uint8); kf_bad[[int(head[0]), int(head[2])]] = 1
    want, stats = [], dict(bad=0, dup=0, badmap=0)
    for q, qm, cn in zip(d["queries"], q_map, conn):
        ex = np.zeros(K, np.uint8); ex[cn] = 1
        r = db.detect_relocalization_candidates(q["word"], q["val"], covis=covis)
        n = db.detect_nbest_candidates(q["word"], q["val"], exclude=ex, covis=covis)
        want.append((_reloc_tail(r, kf_map, qm),) + _nbest_tail(n, kf_map, kf_bad, qm, stats))
    return d, kf_map, kf_bad, covis, q_map, conn, want, stats


def test_model_exercises_the_tail():
    *_, want, stats = model()
    assert stats["bad"] > 0 and stats["dup"] > 0 and stats["badmap"] > 0, stats
    assert all(len(r) > 0 and len(lo) > 0 for r, lo, _ in want) and any(len(m) > 0 for _, _, m in want), want


def _put(tmp, name, a, dt):
    np.ascontiguousarray(a, dt).tofile(str(tmp / (name + ".bin")))


@pytest.mark.gpu
def test_database_mirror_equals_the_restatement_with_the_same_tail(tmp_path):
    exe = _build(str(tmp_path))
    d, kf_map, kf_bad, covis, q_map, conn, want, _ = model()
    _put(tmp_path, "hdr", [K, len(d["queries"]), NUM, AGAIN], np.int32)
    _put(tmp_path, "kf_off", np.concatenate([[0], np.cumsum([len(w) for w, _ in d["kfs"]])]), np.int32)
    _put(tmp_path, "kf_word", np.concatenate([w for w, _ in d["kfs"]]), np.uint32)
    _put(tmp_path, "kf_val", np.concatenate([v for _, v in d["kfs"]]), np.float64)
    _put(tmp_path, "kf_map", kf_map, np.int32); _put(tmp_path, "kf_bad", kf_bad, np.uint8); _put(tmp_path, "covis", covis, np.int32)
    _put(tmp_path, "badmaps", [BAD_MAP], np.int32)
    _put(tmp_path, "q_off", np.concatenate([[0], np.cumsum([len(q["word"]) for q in d["queries"]])]), np.int32)
    _put(tmp_path, "q_word", np.concatenate([q["word"] for q in d["queries"]]), np.uint32)
    _put(tmp_path, "q_val", np.concatenate([q["val"] for q in d["queries"]]), np.float64)
    _put(tmp_path, "q_map", q_map, np.int32)
    _put(tmp_path, "conn_off", np.concatenate([[0], np.cumsum([len(c) for c in conn])]), np.int32)
    _put(tmp_path, "conn", [s for c in conn for s in c], np.int32)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "done" in out.stdout, out.stdout + out.stderr
    get = lambda n: np.fromfile(str(tmp_path / (n + ".bin")), np.int32).tolist()      # noqa: E731
    assert get("cnt") == [len(x) for t in want for x in t]
    for i, name in enumerate(("reloc", "loop", "merge")):
        assert get(name) == [s for t in want for s in t[i]], name
