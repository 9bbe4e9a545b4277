"""Loader of the CPU restatement of the reference's KeyFrameDatabase (kfdb_ref.c, beside this file): compiled with the host C compiler
into a temporary directory when first used, strict IEEE.  Test infrastructure: nothing under eorb_slam_amd/ imports it."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-std=c99", "-Wall"]

_libs = {}


def lib(timing=False):
    """the strict build the tests compare with; timing=True: the same source with -O3 -march=native (still -ffp-contract=off, same
    results), what tools/kfdb_latency.py times on one core"""
    if timing in _libs:
        return _libs[timing]
    tmp = tempfile.mkdtemp(prefix="kfdb_ref_")
    atexit.register(shutil.rmtree, tmp, True)
    so = os.path.join(tmp, "libkfdb_ref.so")
    flags = (["-O3", "-march=native"] + CFLAGS[1:]) if timing else CFLAGS
    subprocess.check_call([os.environ.get("CC", "gcc")] + flags + [os.path.join(_HERE, "kfdb_ref.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    vp, ci, pi = C.c_void_p, C.c_int, C.POINTER(C.c_int)
    L.kr_create.restype = vp; L.kr_create.argtypes = [ci]
    L.kr_destroy.restype = None; L.kr_destroy.argtypes = [vp]
    L.kr_clear.restype = None; L.kr_clear.argtypes = [vp]
    L.kr_add.restype = ci; L.kr_add.argtypes = [vp, ci, vp, vp]
    L.kr_erase.restype = ci; L.kr_erase.argtypes = [vp, ci]
    L.kr_n_slots.restype = ci; L.kr_n_slots.argtypes = [vp]
    L.kr_get_scores.restype = None; L.kr_get_scores.argtypes = [vp, ci, vp]
    L.kr_l1_score.restype = C.c_double; L.kr_l1_score.argtypes = [ci, vp, vp, ci, vp, vp]
    L.kr_detect_reloc.restype = ci
    L.kr_detect_reloc.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, pi, pi, pi, C.POINTER(C.c_float), pi]
    L.kr_detect_nbest.restype = ci
    L.kr_detect_nbest.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, pi, pi, pi, C.POINTER(C.c_float), pi]
    _libs[timing] = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _vec(word, val):
    return np.ascontiguousarray(word, np.uint32), np.ascontiguousarray(val, np.float64)


def l1_score(w1, v1, w2, v2):
    """L1Scoring::score(v1, v2) as a double (the caller's `float si = ...` is np.float32 of it)"""
    w1, v1 = _vec(w1, v1); w2, v2 = _vec(w2, v2)
    return lib().kr_l1_score(len(w1), _p(w1), _p(v1), len(w2), _p(w2), _p(v2))


class CapacityError(RuntimeError):
    def __init__(self, n_scored):
        super().__init__("lScoreAndMatch holds %d entries" % n_scored)
        self.n_scored = n_scored


class KeyFrameDatabase:
    """the reference's database over `vocab_words` inverted lists; the methods and results mirror eorb_slam_amd.frontend.KeyFrameDatabase
    (dicts of numpy arrays), plus `stale`: neighbour scores added that the query itself did not write"""

    def __init__(self, vocab_words, timing=False):
        self.L = lib(timing)
        self.h = C.c_void_p(self.L.kr_create(int(vocab_words)))
        self.vocab_words = int(vocab_words)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.kr_destroy(self.h); self.h = None

    def add(self, word, val):
        word, val = _vec(word, val)
        assert len(word) == len(val) and (len(word) == 0 or int(word.max()) < self.vocab_words)
        return self.L.kr_add(self.h, len(word), _p(word), _p(val))

    def erase(self, slot):
        if self.L.kr_erase(self.h, int(slot)) != 0:
            raise ValueError("slot %d holds no keyframe" % slot)

    def clear(self):
        self.L.kr_clear(self.h)

    @property
    def n_slots(self):
        return self.L.kr_n_slots(self.h)

    def scores(self, family):
        out = np.zeros(self.n_slots, np.float32)
        self.L.kr_get_scores(self.h, int(family), _p(out))
        return out

    def _detect(self, nbest, word, val, exclude, covis, cap):
        word, val = _vec(word, val)
        assert len(word) == len(val) and (len(word) == 0 or int(word.max()) < self.vocab_words)
        ns = self.n_slots
        cap = ns if cap is None else int(cap)
        if covis is not None:
            covis = np.ascontiguousarray(covis, np.int32); assert covis.shape == (ns, 10)
        if exclude is not None:
            exclude = np.ascontiguousarray(exclude, np.uint8); assert exclude.shape == (ns,)
        m = max(cap, 1)
        o = dict(slot=np.zeros(m, np.int32), si=np.zeros(m, np.float32), words=np.zeros(m, np.int32), acc=np.zeros(m, np.float32),
                 best_slot=np.zeros(m, np.int32))
        if nbest:
            o["sorted_acc"] = np.zeros(m, np.float32); o["sorted_best_slot"] = np.zeros(m, np.int32)
        else:
            o["keep"] = np.zeros(m, np.uint8)
        nl, nsc, mc, st, ba = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_float(0)
        tail = (C.byref(nl), C.byref(nsc), C.byref(mc), C.byref(ba), C.byref(st))
        if nbest:
            rc = self.L.kr_detect_nbest(self.h, len(word), _p(word), _p(val), _p(exclude), _p(covis), cap, _p(o["slot"]), _p(o["si"]), _p(o["words"]),
                                        _p(o["acc"]), _p(o["best_slot"]), _p(o["sorted_acc"]), _p(o["sorted_best_slot"]), *tail)
        else:
            rc = self.L.kr_detect_reloc(self.h, len(word), _p(word), _p(val), _p(covis), cap, _p(o["slot"]), _p(o["si"]), _p(o["words"]),
                                        _p(o["acc"]), _p(o["best_slot"]), _p(o["keep"]), *tail)
        if rc != 0:
            raise CapacityError(nsc.value)
        res = {k: v[:nsc.value].copy() for k, v in o.items()}
        if covis is None:
            for k in ("acc", "best_slot", "keep", "sorted_acc", "sorted_best_slot"):
                res.pop(k, None)
        res.update(n_listed=nl.value, n_scored=nsc.value, max_common_words=mc.value, best_acc=np.float32(ba.value), stale=st.value)
        return res

    def detect_relocalization_candidates(self, word, val, covis=None, cap=None):
        return self._detect(0, word, val, None, covis, cap)

    def detect_nbest_candidates(self, word, val, exclude=None, covis=None, cap=None):
        return self._detect(1, word, val, exclude, covis, cap)
