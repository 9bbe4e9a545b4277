"""The event loader's text grammar (include/eorb_fe.h, eorb_parse_events_text) on the CPU: the hand-written expectations of
tests/loader_lines.py, the exact model tests/loader_model.py and the oracle (oracle/orc_events.c) agree on every line and every text,
event bytes and malformed index alike; every `wrong=` variant of the model is rejected by a named line or text; the rounding group is
not vacuous.  tests/test_gpu_loader.py holds the kernels to the same three."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loader_lines as ll                           # noqa: E402
import loader_model as lm                           # noqa: E402


def oracle_parse(oracle, text, cap=None):
    try:
        return oracle.parse_events_text(text, cap), None
    except ValueError as e:
        return None, e.args[0]


def same(got, want):
    """got: (RAW_DTYPE array or None, index); want: (list of events or None, index)."""
    if (got[0] is None) != (want[0] is None) or got[1] != want[1]:
        return False
    return got[0] is None or got[0].tobytes() == lm.as_raw(want[0]).tobytes()


def show(r):
    return "malformed line %s" % r[1] if r[0] is None else "%d events" % len(r[0])


def test_the_model_gives_the_hand_written_answer_on_every_line():
    for g, i, line, want, why in ll.all_lines():
        got = lm.parse_line(line)
        assert type(got) is type(want) and got == want, "%s[%d] (%s): the model gives %r, by hand %r" % (g, i, why, got, want)
        if isinstance(want, tuple):
            assert np.float64(got[0]).tobytes() == np.float64(want[0]).tobytes()


def test_model_and_oracle_agree_with_the_expectation_on_every_text(oracle):
    n = 0
    for name, text, want in ll.texts():
        m = lm.parse_text(text)
        assert m == want, "%s: the model gives %s, by hand %s" % (name, show(m), show(want))
        o = oracle_parse(oracle, text)
        assert same(o, want), "%s: the oracle gives %s, by hand and by the model %s" % (name, show(o), show(want))
        n += 1
    assert n > 5000 and max(len(t) for _, t, _ in ll.texts()) < 128 * 1024


def test_capacity_of_the_oracle(oracle):
    text, (events, _) = ll.compose(ll.mixed_rows(300, 3))
    assert len(oracle.parse_events_text(text, len(events))) == len(events)
    with pytest.raises(OverflowError):
        oracle.parse_events_text(text, len(events) - 1)
    text, (_, bad) = ll.compose(ll.mixed_rows(300, 3, (200,)))
    assert oracle_parse(oracle, text, 1) == (None, 200) and bad == 200, "a malformed line takes precedence over the capacity"


# the four disagreements between the header and the parent's kernel / oracle, by name
FINDINGS = {
    "blank lines are lines (half_lines)": [t for t in ll.nothing_texts() if t[1][0] == b"\n" * 5],
    "polarity takes no point": [("1.", ll.compose([r[:2]])) for r in ll.GROUPS["polarity"] if r[0].endswith(b" 1.") or r[0].endswith(b" 0.")],
    "coordinates by their digits": [(r[2], ll.compose([r[:2]])) for r in ll.GROUPS["coordinates"] if b"2.00000001" in r[0] or b"65535.0000000001" in r[0]
                                    or r[0].startswith(b"1.5 7.000000000000000000 ")],
    "no limit on a line's length": [(r[2], ll.compose([r[:2]])) for r in ll.GROUPS["length"] if len(r[0]) == 256 and r[1] not in (None, ll.SKIP)],
}


@pytest.mark.parametrize("finding", sorted(FINDINGS))
def test_findings_are_represented(oracle, finding):
    rows = FINDINGS[finding]
    assert rows, "no line or text stands for this finding"
    for name, (text, want) in rows:
        assert same(oracle_parse(oracle, text), want) and lm.parse_text(text) == want, name


# ---- the wrong variants ----------------------------------------------------------------------------------------------------------------
def _rejected_by_lines(wrong, group, pick):
    rows = [r for r in ll.GROUPS[group] if pick(r)]
    assert rows
    return [r for r in rows if lm.parse_line(r[0], wrong) != r[1]]


def test_wrong_p_point():
    assert _rejected_by_lines("p_point", "polarity", lambda r: r[0].endswith(b" 1."))


def test_wrong_xy_rounded():
    assert len(_rejected_by_lines("xy_rounded", "coordinates", lambda r: b"2.00000001" in r[0] or b"65535.0000000001" in r[0])) == 4


def test_wrong_line_255():
    bad = _rejected_by_lines("line_255", "length", lambda r: len(r[0]) >= 256 and r[1] not in (None, ll.SKIP))
    assert any(len(r[0]) == 256 for r in bad) and not _rejected_by_lines("line_255", "length", lambda r: len(r[0]) == 255)


def test_wrong_half_lines():
    for k in (5, 1023, 3000):
        with pytest.raises(lm.Capacity):
            lm.parse_text(b"\n" * k, "half_lines")
    assert lm.parse_text(b"\n" * 4, "half_lines") == ([], None)
    assert sum(1 for name, (text, want) in ll.nothing_texts() if _raises(text)) >= 6


def _raises(text):
    try:
        lm.parse_text(text, "half_lines")
    except lm.Capacity:
        return True
    return False


def test_wrong_last_bad():
    bad = [name for name, (text, want) in ll.malformed_texts() if lm.parse_text(text, "last_bad") != want]
    assert len(bad) >= 10, bad


def test_wrong_no_cr():
    assert _rejected_by_lines("no_cr", "separators", lambda r: r[0].endswith(b"\r"))


def test_the_rounding_group_is_not_vacuous():
    pairs = ll.rounding_mantissas()
    assert sorted(set(f for f, _ in pairs)) == list(range(1, 23)) and len(pairs) == 22 * 8 and len(set(pairs)) == len(pairs)
    for f, m in pairs:
        # 10^5 draws: the 8th nearest of uniform distances in [0, 1/2] lies near 4e-5 ulp; 2e-4 is missed with 40 draws expected below
        # it.  For few fraction digits the quotient's scaled fractions are multiples of 1 / 5^f: none lies nearer than 1 / (2 5^f).
        assert 0 < m < 2 ** 53 and 0 < ll.midpoint_distance(m, f) <= max(Fraction(2, 10 ** 4), Fraction(1, 2 * 5 ** f)), (f, m)
    wrong = _rejected_by_lines("div_recip", "ts_rounding", lambda r: True)
    assert len(wrong) >= 1, "mant * (1 / 10^frac) gets none of the rounding lines wrong: draw more"
    assert not _rejected_by_lines(None, "ts_rounding", lambda r: True)


# ---- eorb_undistort_events -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check", [True, False])
def test_undistort_model_and_oracle(oracle, check):
    mx, my, _, _ = ll.undistort_maps()
    for n in ll.UND_N:
        for pattern in ll.UND_PATTERNS:
            raw, keep = ll.undistort_events_case(n, pattern)
            for tsf in ll.UND_TSFACTORS:
                want, mask = lm.undistort_events(raw, mx, my, ll.LW, ll.LH, check, tsf)
                assert np.array_equal(mask, keep if check else np.ones(n, bool)), "the model keeps other events than the case says"
                got = oracle.undistort_events(raw, mx, my, ll.LW, ll.LH, check, tsf)
                assert got.tobytes() == want.tobytes(), "n %d, %s, tsFactor %g: the oracle differs from the model" % (n, pattern, tsf)
