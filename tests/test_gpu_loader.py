"""The event loader on the device (GPU): eorb_parse_events_text and eorb_undistort_events against the exact model of
tests/loader_model.py first and the oracle second, on the lines and texts of tests/loader_lines.py.  A failure names which of the
three (device, model, oracle) is alone.  eorb_parse_events_text is called through ctypes, so that *bad_line, *n_out and the part of
`out` that must stay untouched are seen.  Every test runs on one context for the whole module and again on one whose device memory
is filled with 0xFF (eorb_debug_option "dirty_fill")."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loader_lines as ll                           # noqa: E402
import loader_model as lm                           # noqa: E402
from eorb_slam_amd import _lib                      # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4                                           # events behind `cap` that no call may touch
MARK = 0xA5


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module")
def contexts(fe):
    clean, filled = fe.Context(), fe.Context()
    filled.debug_option("dirty_fill", 0xFF)
    yield {"clean": clean, "filled": filled}
    clean.close(); filled.close()


@pytest.fixture(params=["clean", "filled"])
def ctx(request, contexts):
    return contexts[request.param]


def dev_parse(c, text, cap=None):
    """-> (rc, n_out, bad_line, the events written, whether everything else of `out` still holds the mark)"""
    if cap is None:
        cap = text.count(b"\n") + 1
    out = np.full((cap + GUARD) * lm.RAW_DTYPE.itemsize, MARK, np.uint8)
    k = C.c_size_t(12345); bad = C.c_int64(-7)
    rc = c.L.eorb_parse_events_text(c.h, text, len(text), out.ctypes.data_as(C.c_void_p), cap, C.byref(k), C.byref(bad))
    n = k.value if rc == 0 else 0
    rest_untouched = n <= cap and bool((out[n * lm.RAW_DTYPE.itemsize:] == MARK).all())
    return rc, k.value, bad.value, out[:n * lm.RAW_DTYPE.itemsize].view(lm.RAW_DTYPE).copy(), rest_untouched


def dev_result(c, text):
    rc, n, bad, ev, untouched = dev_parse(c, text)
    assert untouched, "out was written behind the %d events returned (rc %d)" % (n, rc)
    if rc == 0:
        assert bad == -1 and n == len(ev)
        return ev, None
    assert n == 0, "*n_out = %d with rc %d" % (n, rc)
    if rc == _lib.EORB_E_ARG and bad >= 0:
        return None, bad
    return None, "rc %d, bad_line %d: %s" % (rc, bad, c.L.eorb_last_error(c.h).decode())


def oracle_result(oracle, text):
    try:
        return oracle.parse_events_text(text), None
    except ValueError as e:
        return None, e.args[0]


def agree(a, b):
    if (a[0] is None) != (b[0] is None) or a[1] != b[1]:
        return False
    return a[0] is None or a[0].tobytes() == b[0].tobytes()


def show(r):
    return "malformed line %s" % (r[1],) if r[0] is None else "%d events" % len(r[0])


def hold(c, oracle, name, text, want):
    """The device against the model first, the oracle second."""
    m = lm.parse_text(text)
    assert m == want, "%s: the model gives %s, by hand %s" % (name, show(m), show(want))
    m = (None if m[0] is None else lm.as_raw(m[0]), m[1])
    d = dev_result(c, text)
    if agree(d, m):
        o = oracle_result(oracle, text)
        assert agree(o, m), "%s: the oracle is alone: %s; device and model: %s" % (name, show(o), show(m))
        return
    o = oracle_result(oracle, text)
    who = "the device is alone" if agree(o, m) else "the model is alone" if agree(o, d) else "all three differ"
    first = ""
    if d[0] is not None and m[0] is not None and len(d[0]) == len(m[0]):
        k = int(np.flatnonzero(d[0] != m[0])[0])
        first = "; first at event %d: device %r, model %r" % (k, d[0][k], m[0][k])
    raise AssertionError("%s: %s: device %s, model %s, oracle %s%s" % (name, who, show(d), show(m), show(o), first))


LINE_TEXTS = {}
for _name, _text, _want in ll.line_texts():
    LINE_TEXTS.setdefault(_name.split("[")[0], []).append((_name, _text, _want))


@pytest.mark.parametrize("group", sorted(ll.GROUPS))
def test_lines_at_every_position_and_block_edge(oracle, ctx, group):
    for name, text, want in LINE_TEXTS[group]:
        hold(ctx, oracle, name, text, want)


@pytest.mark.parametrize("kind", ["count", "nothing", "malformed"])
def test_whole_texts(oracle, ctx, kind):
    for name, (text, want) in getattr(ll, kind + "_texts")():
        hold(ctx, oracle, name, text, want)


def test_capacity(ctx):
    for n in (1, 300, 1025, 2049):
        text, (events, _) = ll.compose(ll.mixed_rows(n, 40 + n) + [ll.GOOD])
        want = lm.as_raw(events)
        rc, k, bad, ev, untouched = dev_parse(ctx, text, len(events))
        assert rc == 0 and k == len(events) and bad == -1 and ev.tobytes() == want.tobytes() and untouched, "cap = the kept count"
        rc, k, bad, ev, untouched = dev_parse(ctx, text, len(events) - 1)
        assert rc == _lib.EORB_E_CAPACITY and k == 0 and bad == -1 and untouched, "cap one below the kept count: rc %d, n_out %d, bad %d" % (rc, k, bad)
        text, (_, first) = ll.compose(ll.mixed_rows(n, 40 + n, (n // 2, n - 1)) + [ll.GOOD])
        rc, k, bad, ev, untouched = dev_parse(ctx, text, 0)
        assert rc == _lib.EORB_E_ARG and k == 0 and bad == first == n // 2 and untouched, "a malformed line and no room: rc %d, bad %d" % (rc, bad)
    rc, k, bad, ev, untouched = dev_parse(ctx, b"# nothing\n\n", 0)
    assert rc == 0 and k == 0 and bad == -1 and untouched
    k = C.c_size_t(5)
    assert ctx.L.eorb_parse_events_text(ctx.h, ll.GOOD[0], len(ll.GOOD[0]), None, 0, C.byref(k), None) == _lib.EORB_E_CAPACITY and k.value == 0
    assert ctx.L.eorb_parse_events_text(ctx.h, b"1 2 3 4", 7, None, 0, C.byref(k), None) == _lib.EORB_E_ARG, "bad_line may be NULL"


@pytest.mark.parametrize("part", sorted(ll.GROUPS) + ["whole texts"])
def test_frontend_mirror_equals_the_c_call(fe, ctx, part):
    rows = LINE_TEXTS[part] if part in LINE_TEXTS else [(n, t, w) for n, (t, w) in ll.unit_texts()]
    for name, text, want in rows:
        d = dev_result(ctx, text)
        try:
            f = (fe.EvImConverter.parse_events_text(text, ctx=ctx), None)
        except fe.EorbError as e:
            assert e.code == _lib.EORB_E_ARG, "%s: %s" % (name, e)
            f = (None, e.bad_line)
        assert agree(f, d), "%s: the mirror gives %s, the C call %s" % (name, show(f), show(d))
        assert (want[0] is None) == (f[0] is None) and want[1] == f[1], name


@pytest.mark.parametrize("check", [True, False])
def test_undistort_events_against_the_model(oracle, fe, ctx, check):
    mx, my, _, _ = ll.undistort_maps()
    fe.EvImConverter.set_undistort_maps(mx, my, check, ctx=ctx)
    for n in ll.UND_N:
        for pattern in ll.UND_PATTERNS:
            raw, keep = ll.undistort_events_case(n, pattern)
            for tsf in ll.UND_TSFACTORS:
                want, mask = lm.undistort_events(raw, mx, my, ll.LW, ll.LH, check, tsf)
                assert np.array_equal(mask, keep if check else np.ones(n, bool))
                out = np.full((n + GUARD) * lm.EVENT_DTYPE.itemsize, MARK, np.uint8); k = C.c_size_t(12345)
                rc = ctx.L.eorb_undistort_events(ctx.h, raw.ctypes.data_as(C.c_void_p), n, ll.LW, ll.LH, float(tsf), out.ctypes.data_as(C.c_void_p), C.byref(k))
                what = "n %d, %s, checkInImage %d, tsFactor %g" % (n, pattern, check, tsf)
                assert rc == 0 and k.value == len(want), "%s: rc %d, %d events kept, the model keeps %d" % (what, rc, k.value, len(want))
                nb = len(want) * lm.EVENT_DTYPE.itemsize
                assert (out[nb:] == MARK).all(), what + ": out written behind the kept events"
                if out[:nb].tobytes() != want.tobytes():
                    o = oracle.undistort_events(raw, mx, my, ll.LW, ll.LH, check, tsf)
                    who = "the device is alone" if o.tobytes() == want.tobytes() else "the model is alone" if o.tobytes() == out[:nb].tobytes() else "all three differ"
                    got = out[:nb].view(lm.EVENT_DTYPE)
                    j = int(np.flatnonzero(got != want)[0])
                    raise AssertionError("%s: %s; first at kept event %d: device %r, model %r" % (what, who, j, got[j], want[j]))
