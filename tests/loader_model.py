"""An exact model of the event loader, written from the text of include/eorb_fe.h alone (eorb_parse_events_text and
eorb_undistort_events): neither from the kernels nor from oracle/orc_events.c.

The parser works on Python bytes and integers.  A time stamp is float(Fraction(mantissa, 10 ** frac)): Python rounds an exact rational
to the nearest double, so the value depends neither on a strtod nor on one IEEE division.  x, y and p are Python integers.

    parse_line(line)  -> SKIP, BAD or (ts, x, y, p)         one line, without its '\\n'
    parse_text(text)  -> (events, None) or (None, index of the first malformed line)
    as_raw(events)    -> the RAW_DTYPE array the device call and the oracle return

`wrong=` names a deliberately wrong variant (None: the right one), as in plain_ref.py; tests/test_loader_model.py shows that the lines
and texts of tests/loader_lines.py reject each of them:

    "p_point"     accepts a polarity token that ends in a point (`1.`)
    "xy_rounded"  accepts a coordinate whose value rounds to an integer in float32 (`2.00000001`)
    "line_255"    refuses event lines of 256 bytes or more
    "half_lines"  refuses texts of more than nbytes / 2 + 2 lines (parse_text raises Capacity)
    "last_bad"    reports the largest malformed index
    "no_cr"       keeps the '\\r' at the end of a line
    "div_recip"   computes mantissa * (1.0 / 10 ** frac)
"""
import struct
from fractions import Fraction

import numpy as np

RAW_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("p", "<u4"), ("t", "<f8")])
EVENT_DTYPE = np.dtype([("ts", "<f8"), ("x", "<f4"), ("y", "<f4"), ("p", "u1"), ("pad", "u1", (7,))])

SKIP = "skip"
BAD = None
WRONG = ("p_point", "xy_rounded", "line_255", "half_lines", "last_bad", "no_cr", "div_recip")

DIGITS = b"0123456789"
BLANKS = b" \t"


class Capacity(Exception):
    """What a too-small capacity gives (EORB_E_CAPACITY); only the "half_lines" variant raises it from parse_text itself."""


def split_lines(text):
    """A line ends at '\\n', or at the last byte of a buffer that does not end in '\\n'."""
    if not text:
        return []
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    return lines


def take_token(line, i):
    r"""The longest \d+\.?\d* or \.\d+ at line[i:].  Returns (digits before the point, digits after it, has a point, index after the
    token), or None when no token starts here."""
    j = i
    while j < len(line) and line[j] in DIGITS:
        j += 1
    whole = line[i:j]
    if j < len(line) and line[j] == ord("."):
        k = j + 1
        while k < len(line) and line[k] in DIGITS:
            k += 1
        frac = line[j + 1:k]
        if not whole and not frac:
            return None                              # a point alone
        return whole, frac, True, k
    if not whole:
        return None
    return whole, b"", False, j


def significant(whole, frac):
    """Digits from the first non-zero one on, zeros of the fraction included."""
    return len((whole + frac).lstrip(b"0"))


def skip_blanks(line, i):
    while i < len(line) and line[i] in BLANKS:
        i += 1
    return i


def parse_line(line, wrong=None):
    if wrong != "no_cr" and line.endswith(b"\r"):
        line = line[:-1]
    i = skip_blanks(line, 0)
    if i == len(line) or line[i] == ord("#"):
        return SKIP
    if wrong == "line_255" and len(line) >= 256:
        return BAD
    toks = []
    for _ in range(4):
        t = take_token(line, i)
        if t is None:
            return BAD
        toks.append(t[:3])
        i = skip_blanks(line, t[3])
    if i != len(line):
        return BAD
    for whole, frac, _ in toks:
        if significant(whole, frac) > 19:
            return BAD
    # ts
    whole, frac, _ = toks[0]
    mant = int((whole + frac).lstrip(b"0") or b"0")           # (at most 19 digits: checked above)
    if mant >= 2 ** 53 or len(frac) > 22:
        return BAD
    if wrong == "div_recip":
        ts = mant * (1.0 / 10 ** len(frac))
    else:
        ts = float(Fraction(mant, 10 ** len(frac)))
    # x, y
    xy = []
    for whole, frac, _ in toks[1:3]:
        v = int(whole.lstrip(b"0") or b"0")
        if frac.strip(b"0"):
            if wrong != "xy_rounded":
                return BAD
            q = Fraction(int((whole + frac).lstrip(b"0") or b"0"), 10 ** len(frac))
            f = struct.unpack("<f", struct.pack("<f", float(q)))[0]
            if f != int(f):
                return BAD
            v = int(f)
        if v > 65535:
            return BAD
        xy.append(v)
    # p
    whole, frac, point = toks[3]
    if frac or (point and wrong != "p_point"):
        return BAD
    p = int(whole.lstrip(b"0") or b"0")
    if p > 1:
        return BAD
    return (ts, xy[0], xy[1], p)


def parse_text(text, wrong=None):
    lines = split_lines(text)
    if wrong == "half_lines" and len(lines) > len(text) // 2 + 2:
        raise Capacity("%d lines, room for %d" % (len(lines), len(text) // 2 + 2))
    events, bad = [], None
    for k, line in enumerate(lines):
        r = parse_line(line, wrong)
        if r is BAD:
            if wrong != "last_bad":
                return None, k
            bad = k
        elif r is not SKIP:
            events.append(r)
    if bad is not None:
        return None, bad
    return events, None


def as_raw(events):
    out = np.zeros(len(events), RAW_DTYPE)
    for k, (ts, x, y, p) in enumerate(events):
        out[k] = (x, y, p, ts)
    return out


def undistort_events(raw, mapX, mapY, W, H, checkInImage, tsFactor):
    """out = {raw.t / tsFactor, mapX[y][x], mapY[y][x], p} for the events kept, in order; with checkInImage an event is kept when its
    undistorted point (u, v) has 0 <= u < W and 0 <= v < H (a NaN fails, -0.0 passes).  The maps' values are copied bit for bit."""
    mapX = np.asarray(mapX, np.float32); mapY = np.asarray(mapY, np.float32)
    x = raw["x"].astype(np.int64); y = raw["y"].astype(np.int64)
    u = mapX[y, x]; v = mapY[y, x]
    if checkInImage:
        with np.errstate(invalid="ignore"):
            keep = (u >= 0) & (u < np.float32(W)) & (v >= 0) & (v < np.float32(H))
    else:
        keep = np.ones(len(raw), bool)
    out = np.zeros(int(keep.sum()), EVENT_DTYPE)
    out["ts"] = raw["t"][keep].astype(np.float64) / np.float64(tsFactor)
    out["x"] = u[keep]; out["y"] = v[keep]
    out["p"] = (raw["p"][keep] != 0).astype(np.uint8)
    return out, keep
