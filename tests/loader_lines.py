"""The lines and texts that hold the event loader's text parser to the grammar of include/eorb_fe.h (eorb_parse_events_text).

GROUPS: name -> list of (bytes of one line without its '\\n', expected, reason).  expected is the event (ts, x, y, p), None for a
malformed line, or SKIP for a comment / blank line.  Every expected value is written by hand or comes from an exact rational in this
file (float(Fraction) rounds correctly); nothing is taken from the model, the oracle or the kernel.

texts(): (name, text, expected) with expected = (events, None) or (None, first malformed index), composed from the lines above and
their expectations, which put those lines where the kernels' units meet: 1024-byte blocks (line ends), 256 lines per block (parse),
1024 lines per block (compaction)."""
import json
import os
import random
from fractions import Fraction

SKIP = "skip"
GOOD = (b"2.25 5 6 0", (2.25, 5, 6, 0))
GOLDEN_ROUNDING = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loader_ts_rounding.json")
LENGTHS = (255, 256, 257, 1023, 1024, 1025, 5000)
OUTSIDE = (b"+", b"-", b"e", b"E", b",", b"x", b"\x00", b"\x80", b"\xff")


def exact(mant, frac):
    return float(Fraction(mant, 10 ** frac))


# ---- ts rounding: mantissas whose quotient lies next to a rounding boundary of double ----------------------------------------------
def midpoint_distance(mant, frac):
    """Distance of mant / 10^frac from the nearest midpoint between two neighbouring doubles, in ulps of the quotient (exact)."""
    q = Fraction(mant, 10 ** frac)
    e = q.numerator.bit_length() - q.denominator.bit_length() - 53
    while q / Fraction(2) ** e >= 2 ** 53:
        e += 1
    while q / Fraction(2) ** e < 2 ** 52:
        e -= 1
    s = q / Fraction(2) ** e                          # in [2^52, 2^53): one ulp is 1
    return abs((s - s.__floor__()) - Fraction(1, 2))


def find_rounding_mantissas(per_length=8, draws=10 ** 5, seed=20240607):
    """For every fraction length 1..22 the `per_length` mantissas, out of `draws` drawn below 2^53, nearest to a rounding boundary.
    Integer arithmetic; it takes some seconds, so the result is committed (GOLDEN_ROUNDING: pairs [fraction length, mantissa]) and
    test_loader_model.py checks every pair's distance with Fraction."""
    rng = random.Random(seed)
    out = []
    for frac in range(1, 23):
        den = 10 ** frac
        best = []
        for _ in range(draws):
            mant = rng.randrange(1, 2 ** 53)
            sh = 53 - (mant.bit_length() - den.bit_length())          # mant * 2^sh / den has 53 or 54 bits
            num = mant << sh if sh >= 0 else mant
            d = den if sh >= 0 else den << -sh
            if num // d >= 2 ** 53:
                d <<= 1
            r = (2 * (num % d) - d)                                   # (fractional part - 1/2) * 2d
            best.append((abs(r) / d, mant))
        best.sort()
        out += [[frac, m] for _, m in best[:per_length]]
    return out


def rounding_mantissas():
    with open(GOLDEN_ROUNDING) as f:
        return [tuple(v) for v in json.load(f)]


def _digits(mant, frac):
    s = str(mant).rjust(frac + 1, "0")
    return (s[:-frac] + "." + s[-frac:]).encode()


# ---- the lines ---------------------------------------------------------------------------------------------------------------------
def _ts(tok, ts, why):
    return (tok + b" 3 4 1", None if ts is None else (ts, 3, 4, 1), "ts " + why)


def _xy(tok, v, why):
    return [(b"1.5 " + tok + b" 4 1", None if v is None else (1.5, v, 4, 1), "x " + why),
            (b"1.5 3 " + tok + b" 0", None if v is None else (1.5, 3, v, 0), "y " + why)]


def _p(tok, v, why):
    return (b"1.5 3 4 " + tok, None if v is None else (1.5, 3, 4, v), "p " + why)


def _pad(line, n, how):
    k = n - len(line)
    if how == "trailing":
        return line + b" " * k
    if how == "inner":
        return line[:3] + b" " * (k // 2) + b"\t" * (k - k // 2) + line[3:]
    return b"0" * k + line                                   # leading zeros of ts


def groups():
    G = {}
    G["ts_edges"] = [
        _ts(b"0", 0.0, "0"), _ts(b"000", 0.0, "000"), _ts(b"0.", 0.0, "point without fraction"), _ts(b".0", 0.0, "point without whole"),
        _ts(b".5", 0.5, ".5"), _ts(b"5.", 5.0, "5."), _ts(b".", None, "a point alone is no token"),
        _ts(b"9007199254740991", 9007199254740991.0, "2^53 - 1"), _ts(b"9007199254740992", None, "2^53"),
        _ts(b"900719925474099.1", exact(9007199254740991, 1), "2^53 - 1 with a fraction digit"),
        _ts(b"900719925474099.2", None, "mantissa 2^53 with a fraction digit"),
        _ts(b"1234567890123456789", None, "19 significant digits: mantissa over 2^53"),
        _ts(b"12345678901234567890", None, "20 significant digits"),
        _ts(b"0.0000009007199254740991", exact(9007199254740991, 22), "22 fraction digits, mantissa 2^53 - 1"),
        _ts(b"0.00000009007199254740991", None, "23 fraction digits"),
        _ts(b"0." + b"0" * 21 + b"1", exact(1, 22), "1e-22"), _ts(b"0." + b"0" * 22 + b"1", None, "1e-23: 23 fraction digits"),
        _ts(b"0." + b"0" * 22, 0.0, "22 zeros of fraction"), _ts(b"0." + b"0" * 23, None, "23 zeros of fraction"),
        _ts(b"0" * 300 + b"1.5", 1.5, "300 leading zeros"), _ts(b"0" * 300, 0.0, "300 zeros"),
        _ts(b"1." + b"0" * 15, 1.0, "16 significant digits by trailing zeros"),
        _ts(b"1." + b"0" * 18, None, "19 significant digits by trailing zeros: mantissa 10^18"),
        _ts(b"1." + b"0" * 19, None, "20 significant digits by trailing zeros"),
        _ts(b"1468941032.229165", exact(1468941032229165, 6), "a dataset stamp"),
        _ts(b"0.1", 0.1, "0.1"), _ts(b"0.3", 0.3, "0.3"), _ts(b"123456789.123456", exact(123456789123456, 6), "15 digits"),
    ]
    G["ts_rounding"] = [_ts(_digits(m, f), exact(m, f), "next to a rounding boundary, %d fraction digits" % f) for f, m in rounding_mantissas()]
    C = []
    for tok, v, why in [(b"007", 7, "leading zeros"), (b"8.000", 8, "zero fraction"), (b"7.", 7, "point without fraction"), (b".0", 0, ".0"),
                        (b"0", 0, "0"), (b"65535", 65535, "65535"), (b"65535.0", 65535, "65535.0"), (b"65536", None, "65536"),
                        (b"65536.0", None, "65536.0"), (b"65535.0000000001", None, "rounds to 65535 in float32"),
                        (b"2.00000001", None, "rounds to 2 in float32"), (b"2.5", None, "2.5"), (b".5", None, ".5"),
                        (b"7." + b"0" * 18, 7, "19 significant digits, integer-valued"),
                        (b"7." + b"0" * 19, None, "20 significant digits, integer-valued"),
                        (b"7." + b"0" * 25, None, "26 significant digits, integer-valued"),
                        (b"0" * 24 + b"7", 7, "24 leading zeros"), (b"0" * 24 + b"7." + b"0" * 18, 7, "24 leading zeros, 19 significant"),
                        (b"4294967297", None, "2^32 + 1"), (b"18446744073709551617", None, "2^64 + 1"),
                        (b"1844674407370955162", None, "19 digits over 2^60"), (b"65537", None, "2^16 + 1")]:
        C += _xy(tok, v, why)
    G["coordinates"] = C
    G["polarity"] = [_p(b"0", 0, "0"), _p(b"1", 1, "1"), _p(b"01", 1, "01"), _p(b"00", 0, "00"), _p(b"2", None, "2"), _p(b"10", None, "10"),
                     _p(b"1.", None, "1. has a point"), _p(b"0.", None, "0. has a point"), _p(b"1.0", None, "1.0"), _p(b".1", None, ".1"),
                     _p(b".0", None, ".0"), _p(b"0" * 23 + b"1", 1, "23 zeros and a 1"), _p(b"4294967297", None, "2^32 + 1"),
                     _p(b"18446744073709551617", None, "2^64 + 1"), _p(b"1" + b"0" * 19, None, "20 significant digits")]
    G["separators"] = [
        (b"1.5\t3\t4\t1", (1.5, 3, 4, 1), "tabs"), (b"1.5   3 \t 4    1", (1.5, 3, 4, 1), "runs of blanks"),
        (b"  \t1.5 3 4 1 \t ", (1.5, 3, 4, 1), "leading and trailing blanks"),
        (b"1.0.0 3 1", (1.0, 0, 3, 1), "no separator: 1.0 | .0 | 3 | 1"), (b"0.0.0.0", None, "greedy: 0.0 | .0 | .0, three tokens"), (b"0. 0. 0. 0", (0.0, 0, 0, 0), "points without fractions"),
        (b"1.5.0.0 1", (1.5, 0, 0, 1), "1.5 | .0 | .0 | 1"), (b"1. .0 3 1", (1.0, 0, 3, 1), "1. | .0"),
        (b"1..2 3 1", None, "1. | .2: x has a fraction"), (b"1..0 3 1", (1.0, 0, 3, 1), "1. | .0 without a blank"),
        (b"1.0.0.0.1", None, "1.0 | .0 | .0 | .1: p has a point"), (b"0.0.0.0.", None, "0.0 | .0 | .0 | a point alone"),
        (b"1.5 3 4", None, "three tokens"), (b"1.5 3 41", None, "three tokens"), (b"1.5 3 4 1 0", None, "five tokens"),
        (b"1.5 3 4 1 #c", None, "# after the fourth token"), (b"1.5 3 4 1#", None, "# right after the fourth token"),
        (b"1.5 3 4 1\r", (1.5, 3, 4, 1), "\\r at the end"), (b" 1.5 3 4 1 \r", (1.5, 3, 4, 1), "blank and \\r at the end"),
        (b"1.5 3\r 4 1", None, "\\r in the middle"), (b"\r", SKIP, "\\r alone"), (b"\r\r", None, "two \\r: one is dropped"),
        (b"1.5 3 4 1\r\r", None, "two \\r at the end"), (b" \t\r", SKIP, "blanks and \\r"), (b"#\r", SKIP, "comment and \\r"),
        (b"", SKIP, "empty"), (b" ", SKIP, "one blank"), (b"\t \t", SKIP, "blanks"), (b"#", SKIP, "# alone"), (b"  # 1 2 3", SKIP, "comment after blanks"),
        (b"1.5\x0b3 4 1", None, "vertical tab is no separator"), (b"1.5\x0c3 4 1", None, "form feed is no separator"),
        (b"1.5 . 4 1", None, "a point alone as x"), (b"1 2 3 1", (1.0, 2, 3, 1), "integers"), (b"0 0 0 0", (0.0, 0, 0, 0), "the shortest line"),
    ]
    O = []
    for b in OUTSIDE:
        n = repr(b)[1:]
        O += [(b + b"1.5 3 4 1", None, n + " first"), (b"1.5" + b + b"0 3 4 1", None, n + " inside ts"), (b"1.5 " + b + b"3 4 1", None, n + " before x"),
              (b"1.5 3 4" + b + b" 1", None, n + " after y"), (b"1.5 3 4 1" + b, None, n + " last"), (b"1.5 3 4 1 " + b, None, n + " after a blank at the end"),
              (b"#" + b + b" 1.5 3 4 1", SKIP, n + " in a comment"), (b" \t# c" + b, SKIP, n + " last in a comment")]
    G["outside"] = O
    L = []
    for n in LENGTHS:
        for how in ("trailing", "inner", "zeros"):
            L.append((_pad(b"1.5 3 4 1", n, how), (1.5, 3, 4, 1), "event line of %d bytes, %s" % (n, how)))
        L.append((_pad(b"1.5 3 4 2", n, "inner"), None, "malformed line of %d bytes" % n))
        L.append((_pad(b"1.5 3 4 1", n - 1, "trailing") + b"\r", (1.5, 3, 4, 1), "event line of %d bytes with \\r" % n))
        L.append((b"#" + b"c" * (n - 1), SKIP, "comment line of %d bytes" % n))
        L.append((b" " * n, SKIP, "blank line of %d bytes" % n))
    G["length"] = L
    return G


GROUPS = groups() if __name__ != "__main__" else {}


def all_lines():
    return [(g, i, line, want, why) for g, rows in GROUPS.items() for i, (line, want, why) in enumerate(rows)]


# ---- texts -------------------------------------------------------------------------------------------------------------------------
def compose(rows, final_newline=True):
    """rows: (line, expected).  Returns (text, (events, None) or (None, first malformed index))."""
    text = b"\n".join(r[0] for r in rows) + (b"\n" if final_newline and rows else b"")
    bad = [k for k, r in enumerate(rows) if r[1] is None]
    if bad:
        return text, (None, bad[0])
    return text, ([r[1] for r in rows if r[1] != SKIP], None)


def position_texts(line, want):
    """The line alone, first, last with and without a final '\\n', and between two good lines."""
    row = (line, want)
    out = [("alone", compose([row], False)), ("first", compose([row, GOOD])), ("last", compose([GOOD, row])),
           ("last, no newline", compose([GOOD, row], False)), ("between", compose([GOOD, row, GOOD]))]
    if line:                                          # (an empty line alone without '\n' is the empty text, and as the last line
        out.append(("alone, newline", compose([row])))   # without '\n' it does not exist)
        return out
    return [("alone, newline", compose([row])), out[1], out[2], out[4]]


def block_edge_texts(line, want):
    """A comment in front puts the line's '\\n' (or, without one, its last byte) on bytes b - 2 .. b + 1 of the buffer, b the first
    multiple of 1024 with room for the line; once followed by a good line, once as the last byte of the buffer."""
    base = 1024 * ((len(line) + 8) // 1024 + 1)
    out = []
    for d in (-2, -1, 0, 1):
        n = base + d - len(line) - 1                  # the comment's bytes; its '\n' is byte n
        com = (b"#" + b"c" * (n - 1), SKIP)
        out.append(("newline at byte %d, a line after it" % (base + d), compose([com, (line, want), GOOD])))
        out.append(("newline at byte %d, the last" % (base + d), compose([com, (line, want)])))
        if line:
            out.append(("last byte at %d, no newline" % (base + d), compose([com, (b" " + line, want)], False)))
    return out


def mixed_rows(n, seed, bad_at=()):
    """n lines: events with rising stamps, blanks and comments mixed by a fixed seed; the lines of `bad_at` are malformed."""
    rng = random.Random(seed)
    rows = []
    for k in range(n):
        r = rng.random()
        if k in bad_at:
            rows.append((b"%d.5 %d 7 2" % (k, k % 640), None))
        elif r < 0.15:
            rows.append((rng.choice([b"", b" ", b"\r", b"\t\t"]), SKIP))
        elif r < 0.3:
            rows.append((b"# line %d" % k, SKIP))
        else:
            x, y, p = rng.randrange(65536), rng.randrange(65536), rng.randrange(2)
            rows.append((b"%d.%03d %d %d %d" % (k, k % 1000, x, y, p) + (b"\r" if r > 0.9 else b""), (exact(k * 1000 + k % 1000, 3), x, y, p)))
    return rows


COUNTS = (255, 256, 257, 1023, 1024, 1025, 2049)
NOTHING = [b"", b"#", b" ", b"\r\n" * 5] + [b"\n" * k for k in (1, 4, 5, 1023, 1024, 1025, 3000)]


def count_texts():
    out = []
    for n in COUNTS:
        for nl in (True, False):
            rows = mixed_rows(n, 100 + n)
            if not nl and not rows[-1][0]:
                rows[-1] = GOOD                       # (a text cannot end in an empty line without its '\n')
            out.append(("%d lines%s" % (n, "" if nl else ", no final newline"), compose(rows, nl)))
        out.append(("%d event lines" % n, compose([(b"%d 1 2 1" % k, (float(k), 1, 2, 1)) for k in range(n)])))
    return out


def nothing_texts():
    out = [("nothing: %r, %d bytes" % (t[:10], len(t)), (t, ([], None))) for t in NOTHING]
    out.append(("one event among 60 blank lines", (b"\n" * 30 + GOOD[0] + b"\n" * 30, ([GOOD[1]], None))))
    out.append(("a malformed line among 60 blank lines", (b"\n" * 30 + b"1 2 3 4" + b"\n" * 30, (None, 30))))
    return out


def malformed_texts():
    out = []
    for n, bad in [(2500, (1500, 2100, 2499)), (2500, (5, 1030)), (2500, (2499,)), (2500, (1023, 1024)), (2500, (1024, 2048)), (2049, (2048, 255, 256)),
                   (1025, (1024,)), (300, (299, 64, 63))]:
        for nl in (True, False):
            out.append(("%d lines, malformed %s%s" % (n, bad, "" if nl else ", no final newline"), compose(mixed_rows(n, 7 + n, bad), nl)))
    return out


def unit_texts():
    """The texts of whole files: line counts, nothing, several malformed lines."""
    return count_texts() + nothing_texts() + malformed_texts()


def line_texts():
    """Every line of GROUPS at every position and block edge: (name, text, expected)."""
    out = []
    for g, i, line, want, why in all_lines():
        for name, (text, exp) in position_texts(line, want) + block_edge_texts(line, want):
            out.append(("%s[%d] %s: %s" % (g, i, why, name), text, exp))
    return out


def texts():
    return line_texts() + [(name, t, e) for name, (t, e) in unit_texts()]


# ---- eorb_undistort_events -----------------------------------------------------------------------------------------------------------
LW, LH = 64, 48                                       # the maps; the image they are checked against has the same size
UND_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
UND_PATTERNS = ("all", "none", "alternating", "last", "lane0")
UND_TSFACTORS = (1.0, 1e6, 3.0)


def undistort_maps():
    """Plain maps (x + 0.25, y + 0.5), and in row 0 the values at which isInImage turns.  Returns (mapX, mapY, kept pixels, dropped
    pixels) as (x, y) lists, by hand: -0.0 and the float below W or H pass, exactly W or H, a negative denormal, NaN and +-inf fail."""
    import numpy as np
    mx = (np.arange(LW, dtype=np.float32)[None, :] + np.float32(0.25)).repeat(LH, 0)
    my = (np.arange(LH, dtype=np.float32)[:, None] + np.float32(0.5)).repeat(LW, 1)
    nan = np.array([0x7fc01234], np.uint32).view(np.float32)[0]
    wf, hf = np.float32(LW), np.float32(LH)
    special = [(-0.0, None, True), (wf, None, False), (np.nextafter(wf, np.float32(0)), None, True), (nan, None, False), (np.inf, None, False),
               (-np.inf, None, False), (None, hf, False), (None, np.nextafter(hf, np.float32(0)), True), (None, -0.0, True), (None, nan, False),
               (-1e-45, None, False), (None, -1e-45, False), (None, np.inf, False), (None, -np.inf, False), (-0.0, -0.0, True), (0.0, 0.0, True)]
    kept, dropped = [], []
    for x, (u, v, k) in enumerate(special):
        if u is not None:
            mx[0, x] = u
        if v is not None:
            my[0, x] = v
        (kept if k else dropped).append((x, 0))
    kept += [(x, y) for y in range(1, LH, 5) for x in range(0, LW, 7)]
    return mx, my, kept, dropped


def undistort_events_case(n, pattern, seed=5):
    """n raw events whose pixels are taken from the kept or the dropped list as the pattern says.  Returns (raw, keep mask by hand)."""
    import numpy as np
    _, _, kept, dropped = undistort_maps()
    rng = random.Random(seed * 10007 + n)
    keep = {"all": [True] * n, "none": [False] * n, "alternating": [k % 2 == 0 for k in range(n)], "last": [k == n - 1 for k in range(n)],
            "lane0": [k % 64 == 0 for k in range(n)]}[pattern]
    raw = np.zeros(n, [("x", "<u2"), ("y", "<u2"), ("p", "<u4"), ("t", "<f8")])
    for k in range(n):
        raw[k] = rng.choice(kept if keep[k] else dropped) + (rng.randrange(2), 1468941032.229165 + rng.randrange(10 ** 9) * 1e-6)
    return raw, np.array(keep, bool)


if __name__ == "__main__":                            # regenerate the committed mantissas
    with open(GOLDEN_ROUNDING, "w") as f:
        json.dump(find_rounding_mantissas(), f)
