"""The constants the product and the oracle carry still equal the reference's.

The reference's values live in tests/golden/reference_constants.json, read from its source text by
tests/golden/make_reference_constants.py (rerun it against a checkout of the reference to refresh them): values only,
nothing is imported, compiled or copied from the reference."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "reference_constants.json")) as _f:
    REF = json.load(_f)


def _read(*p):
    with open(os.path.join(*p)) as f:
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


def test_brief_pattern_equals_reference_table():
    ref = REF["orb_bit_pattern_31"]["values"]                                                          # src/ORBextractor.cc:160-418
    assert len(ref) == 1024 and max(abs(v) for v in ref) == 13
    prod = _ints_of_table(_read(ROOT, "eorb_slam_amd/csrc/orb_pattern.h"), "k_orb_pattern_31[1024]")
    orc = _ints_of_table(_read(ROOT, "oracle/orc_pattern.h"), "orc_bit_pattern_31[1024]")
    assert prod == ref and orc == ref


def test_extractor_constants_equal_reference():
    ref = REF["orb_extractor"]                                                                         # src/ORBextractor.cc:71-74
    patch, half, edge, wden = ref["PATCH_SIZE"], ref["HALF_PATCH_SIZE"], ref["EDGE_THRESHOLD"], ref["W_denom"]
    assert (patch, half, edge, wden) == (31, 15, 19, 30)
    orc = _read(ROOT, "oracle/orc_orb.c")
    assert _const(orc, r"#define PATCH_SIZE (\d+)") == patch and _const(orc, r"#define HALF_PATCH_SIZE (\d+)") == half
    # the adaptive edge rule (:481-488) and the cell width (:805-808) as literals in both implementations
    assert ref["DEF_IMAGE_WIDTH"] == 752                                                               # include/ORBextractor.h
    prod = _read(ROOT, "eorb_slam_amd/csrc/orb_extract.hip")
    for src in (prod, orc):
        assert re.search(r"19 \* \(\(float\)\s*\w[\w>\-\.]*imWidth / \(float\)752\)", src), "adaptive edge rule 19*(imWidth/752)"
        assert re.search(r"31\.0f \* |\(float\)PATCH_SIZE \* ", src), "scaledPatchSize"
    assert re.search(r"width / 30\.0f", prod) and re.search(r"height / 30\.0f", prod), "W_denom (product)"
    assert _const(orc, r"#define W_DENOM (\d+)\.0f") == wden and "width / W_DENOM" in orc and "height / W_DENOM" in orc
    # HALF_PATCH_SIZE in IC_Angle (:77-104): columns -15 .. 15 (one lane each), row pairs 1 .. 15 inside the disc
    assert "au <= G->umax[v]" in prod and "(int)(threadIdx.x & 31) - 15" in prod and "for (int v = 1; v <= 15; ++v)" in prod and "if (au <= 15)" in prod


def test_matcher_constants_equal_reference():
    ref = REF["orb_matcher"]                                                                           # src/ORBmatcher.cc:36-38
    th = (ref["TH_HIGH"], ref["TH_LOW"], ref["HISTO_LENGTH"])
    assert th == (100, 50, 30)
    prod = _read(ROOT, "eorb_slam_amd/csrc/match.hip")
    m = re.search(r"constexpr int TH_HIGH = (\d+), TH_LOW = (\d+), HISTO_LENGTH = (\d+);", prod)
    assert m and tuple(int(g) for g in m.groups()) == th
    orc = _read(ROOT, "oracle/orc_matcher.h")                         # the oracle's matchers (orc_match.c, orc_twocam.c) include it
    assert (_const(orc, r"#define TH_HIGH (\d+)"), _const(orc, r"#define TH_LOW (\d+)"), _const(orc, r"#define HISTO_LENGTH (\d+)")) == th
    assert ref["mixed_matcher_uses_class_constants"]                    # the Mixed variants (src/MixedMatcher.cpp) use the same class constants


def test_frame_grid_equals_reference():
    ref = REF["frame_grid"]                                                                            # include/Frame.h:45-46
    rows, cols = ref["FRAME_GRID_ROWS"], ref["FRAME_GRID_COLS"]
    assert (rows, cols) == (48, 64)
    ctxh = _read(ROOT, "eorb_slam_amd/csrc/eorb_ctx.h")
    assert _const(ctxh, r"constexpr int kGridCols = (\d+);") == cols and _const(ctxh, r"constexpr int kGridRows = (\d+);") == rows
    orc = _read(ROOT, "oracle/orc_matcher.h")
    assert _const(orc, r"#define FRAME_GRID_ROWS (\d+)") == rows and _const(orc, r"#define FRAME_GRID_COLS (\d+)") == cols


def test_event_record_and_stamp_constants_equal_reference():
    # EventData = {double ts; float x, y; bool p} (include/Event/EventData.h:36-58): 24 bytes with padding
    members = REF["event_data"]["members"]                                                             # member order = layout
    assert members == [["double", "ts"], ["float", "x"], ["float", "y"], ["bool", "p"]], "EventData member order changed"
    api = _read(ROOT, "include/eorb_fe.h")
    assert re.search(r"double\s+ts;", api) and "eorb_event" in api
    # ev2im_gauss: half window = ceil(sigma * 3) and the 0.001f count increment (src/Event/EventConversion.cc:173-269)
    conv = REF["ev2im_gauss"]
    assert conv["half_window_sigma_factor"] == 3
    assert conv["count_increment"] == "0.001"
    orc = _read(ROOT, "oracle/orc_events.c")
    assert re.search(r"ceil\(\(double\)sigma \* 3\.0\)", orc) and "0.001f" in orc
    prod = _read(ROOT, "eorb_slam_amd/csrc/ev_accum.hip")
    plan = _read(ROOT, "eorb_slam_amd/csrc/ev_plan.h")                          # (the half window is computed in one place: accum_shape)
    assert len(re.findall(r"ceil\(\(double\)sigma \* 3\.0\)", plan)) == 1 and "0.001f" in prod
