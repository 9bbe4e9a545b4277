#!/usr/bin/env python3
"""Extract the constants the product and the oracle must share with the reference (m-dayani/EORB_SLAM) into
reference_constants.json, the fixture tests/test_reference_constants.py checks both implementations against.

Only values are recorded (numbers, the BRIEF sampling table, the EventData member layout), each with the reference
file and lines it was read from; nothing is imported, compiled or copied from the reference as code.

Run from the repository root with the path of a checkout of the reference:
    python tests/golden/make_reference_constants.py <reference tree>
"""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_constants.json")


def _read(ref, rel):
    with open(os.path.join(ref, rel)) as f:
        return f.read()


def _ints_of_table(text, name):
    i = text.index(name)
    body = text[text.index("{", i) + 1:text.index("};", i)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = re.sub(r"//[^\n]*", "", body)
    return [int(x) for x in re.findall(r"-?\d+", body)]


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return float(m.group(1)) if "." in m.group(1) else int(m.group(1))


def main(ref):
    orb = _read(ref, "src/ORBextractor.cc")
    pattern = _ints_of_table(orb, "static int bit_pattern_31_[256*4]")
    assert len(pattern) == 1024
    hdr = _read(ref, "include/ORBextractor.h")
    match = _read(ref, "src/ORBmatcher.cc")
    mixed = _read(ref, "src/MixedMatcher.cpp")
    frame = _read(ref, "include/Frame.h")
    ev = _read(ref, "include/Event/EventData.h")
    body = ev[ev.index("struct EventData"):]
    members = re.findall(r"^\s*(double|float|bool|int)\s+(\w+)\s*=[^;]*;", body[:body.index("};")], flags=re.M)
    conv = _read(ref, "src/Event/EventConversion.cc")
    halfwin = re.search(r"ceil\(sigma\s*\*\s*(3)(?:\.0)?\)", conv)
    incr = re.search(r"polSign\s*\*\s*([0-9.]+)f", conv)
    assert halfwin and incr
    doc = {
        "what": "constants of the reference read from its source text by tests/golden/make_reference_constants.py",
        "orb_bit_pattern_31": {"source": "src/ORBextractor.cc:160-418 (bit_pattern_31_)", "values": pattern},
        "orb_extractor": {"source": "src/ORBextractor.cc:71-74, include/ORBextractor.h (DEF_IMAGE_WIDTH)",
                          "PATCH_SIZE": _const(orb, r"const int PATCH_SIZE = (\d+);"),
                          "HALF_PATCH_SIZE": _const(orb, r"const int HALF_PATCH_SIZE = (\d+);"),
                          "EDGE_THRESHOLD": _const(orb, r"int EDGE_THRESHOLD = (\d+);"),
                          "W_denom": _const(orb, r"const float W_denom = (\d+);"),
                          "DEF_IMAGE_WIDTH": _const(hdr, r"#define DEF_IMAGE_WIDTH (\d+)")},
        "orb_matcher": {"source": "src/ORBmatcher.cc:36-38",
                        "TH_HIGH": _const(match, r"ORBmatcher::TH_HIGH = (\d+);"),
                        "TH_LOW": _const(match, r"ORBmatcher::TH_LOW = (\d+);"),
                        "HISTO_LENGTH": _const(match, r"ORBmatcher::HISTO_LENGTH = (\d+);"),
                        "mixed_matcher_uses_class_constants": "TH_HIGH" in mixed and "HISTO_LENGTH" in mixed},
        "frame_grid": {"source": "include/Frame.h:45-46",
                       "FRAME_GRID_ROWS": _const(frame, r"#define FRAME_GRID_ROWS (\d+)"),
                       "FRAME_GRID_COLS": _const(frame, r"#define FRAME_GRID_COLS (\d+)")},
        "event_data": {"source": "include/Event/EventData.h:36-58", "members": [list(m) for m in members]},
        "ev2im_gauss": {"source": "src/Event/EventConversion.cc:173-269",
                        "half_window_sigma_factor": int(halfwin.group(1)), "count_increment": incr.group(1)},
    }
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
