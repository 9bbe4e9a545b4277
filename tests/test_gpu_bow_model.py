"""eorb_bow_transform (bow_descend_kernel + bow_assemble_kernel, eorb_slam_amd/csrc/match.hip) against the plain model of
tests/bow_model.py and the oracle on the planted scenes of tests/bow_scenes.py (GPU), bit for bit in every output, word_of and node_of
included: every size class of the block sort (M = 1, 2, 4, 8) at its edges, m = 0 and m = 1, one run of n, more than 4096 words, nodes
of more than 128 children, descent ties, short leaves, unaligned rows.

Every case runs on a clean context and on one whose memory is filled with 0xFF (eorb_debug_option("dirty_fill"), as
tests/test_gpu_dirty.py); the scenes of 65, 2049 and 8192 features run once more directly after a larger call on the same context
(8192 is the largest: after another 8192-feature scene), so that stale keys in LDS and stale results in the arena cannot pass.  The
limit: 8192 features pass, 8193 are refused with EORB_E_CAPACITY before anything is uploaded or written.

The references are computed once per case (bow_scenes.want, the oracle here) and never from the device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_scenes as bs                             # noqa: E402
from eorb_slam_amd import _lib                      # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xFF
CASES = bs.cases()
IDS = [bs.case_id(c) for c in CASES]
AFTER = [c for c in CASES if c[0].tags.get("n") in bs.AFTER_LARGER and c[0].tags.get("fill") in ("sparse", "oneword", "many")]
_ORACLE = {}


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module", params=["clean", "filled"])
def state(fe, request):
    c = fe.Context()
    if request.param == "filled":
        c.debug_option("dirty_fill", FILL)
    yield request.param, c
    c.close()


@pytest.fixture(scope="module")
def after(fe):
    c = fe.Context()
    yield c
    c.close()


def _oracle(oracle, case):
    s, weighting, norm = case
    key = bs.case_id(case)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.bow_transform(s.voc, s.desc, s.levelsup, weighting, norm)
    return _ORACLE[key]


def _run(fe, c, case):
    s, weighting, norm = case
    return fe.ORBVocabulary(s.voc, weighting, norm, ctx=c).transform(s.desc, s.levelsup, return_assignments=True)


def _check(fe, c, oracle, case, where):
    s, weighting, norm = case
    got = _run(fe, c, case)
    exp = bs.want(s.name, weighting, norm)
    assert bs.same(got, exp) is None, "%s, %s: %s differs from the model (probe %s)" % (bs.case_id(case), where, bs.same(got, exp), exp[5])
    orc = _oracle(oracle, case)
    assert bs.same(got, orc) is None, "%s, %s: %s differs from the oracle" % (bs.case_id(case), where, bs.same(got, orc))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_equals_model_and_oracle(fe, state, oracle, case):
    _check(fe, state[1], oracle, case, state[0])


@pytest.mark.parametrize("case", AFTER, ids=[bs.case_id(c) for c in AFTER])
def test_after_a_larger_call(fe, after, oracle, case):
    s, weighting, norm = case
    larger = bs.AFTER_LARGER[s.n]
    if larger is None:                                                      # the largest size: another fill of it
        big = bs.scene("%s-%d" % ({"sparse": "many", "oneword": "sparse", "many": "oneword"}[s.tags["fill"]], s.n))
    else:
        big = bs.scene("%s-%d" % (s.tags["fill"], larger))
    _run(fe, after, (big, weighting, norm))
    _check(fe, after, oracle, case, "after %s" % big.name)


def test_limit(fe, after, oracle):
    """MAX_FEATURES descriptors pass (the many-8192 scene above is the bit-exact check); one more is refused from n alone: the error is
    EORB_E_CAPACITY and no byte of the caller's arrays or counts changes"""
    assert fe.ORBVocabulary.MAX_FEATURES == bs.MAX_FEATURES == 8192
    s = bs.scene("many-8192")
    V = fe.ORBVocabulary(s.voc, 0, 1, ctx=after)
    n = bs.MAX_FEATURES + 1
    desc = np.concatenate([s.desc, s.desc[:1]])
    with pytest.raises(fe.EorbError) as e:
        V.transform(desc, 1)
    assert e.value.code == _lib.EORB_E_CAPACITY
    arrs = [np.full(n + 1, 0x5A5A5A5A, np.uint32), np.full(n + 1, -7.25, np.float64), np.full(n + 1, 0x5A5A5A5A, np.uint32), np.full(n + 2, -77, np.int32),
            np.full(n + 1, -77, np.int32), np.full(n + 1, -77, np.int32), np.full(n + 1, -77, np.int32)]
    keep = [a.copy() for a in arrs]
    bw, bv, fn, fo, fi, wo, no = arrs
    nw, nn = C.c_int(-5), C.c_int(-6)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                             # noqa: E731
    rc = after.L.eorb_bow_transform(after.h, p(desc), n, 32, 1, 0, 1, p(bw), p(bv), C.byref(nw), p(fn), p(fo), p(fi), C.byref(nn), p(wo), p(no))
    assert rc == _lib.EORB_E_CAPACITY
    assert (nw.value, nn.value) == (-5, -6) and all(a.tobytes() == k.tobytes() for a, k in zip(arrs, keep))
    _check(fe, after, oracle, (s, 0, 1), "after the refused call")          # and the context is as good as before
