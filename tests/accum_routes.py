"""Which form an event-accumulation call takes: one table, written by hand from the dispatcher's rules, with two readers --
tests/test_accum_plan_cpp.py asks the rules themselves (eorb_slam_amd/csrc/ev_plan.h, compiled into tests/host/accum_plan_check.cpp, no
GPU) for the first-choice route of every row; tests/test_gpu_routes.py runs every row and reads what served it
(eorb_debug_counter "accum_route").  planned_route() gives the other tests that force a form the route their parametrisation takes,
from the same header.

All rows: 240x180 (690 tiles), sigma 1 (half window 3, an event yields at most 4 list entries), default options unless stated.
The load threshold between the slot form and the sparse gather is nev * 4 >= B * 690 * 64: 11 040 events for one slice, 55 200 for five."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DIRECT, SLOTS, LISTS = 1, 2, 3                       # include/eorb_fe.h, "accum_route"
NONE, MAPS, PER_CALL, DICT = 0 << 2, 1 << 2, 2 << 2, 3 << 2
SPARSE, WIDENED = 1 << 4, 1 << 5
# the slot form's binning (csrc/ev_plan.h SlotBinPlan, "slot_binning" = count | record << 2 | scatter << 4)
COUNT_GLOBAL, COUNT_LDS, COUNT_LDS_KEYED = 0, 1, 2
REC_AS_IS, REC_SHORT2, REC_RANKED8 = 0, 1, 2
SCAT_BALLOT, SCAT_RANK, SCAT_PRE = 0, 1, 2

W, H, SIGMA = 240, 180, 1.0
BULK = (("dedupe_min_events", 1),)                   # the float bulk path at test size

# entry: how the row is called -> (raw code of the dispatcher, count image)
ENTRIES = {"gauss": (0, 0), "count": (0, 1), "gauss_raw": (1, 0), "count_raw": (1, 1), "batch_raw": (1, 0), "batch_raw4": (3, 0)}


def describe(route):
    form = {0: "none", DIRECT: "direct", SLOTS: "slots", LISTS: "lists"}[route & 3]
    pset = {NONE: "none", MAPS: "maps", PER_CALL: "per-call", DICT: "dictionary"}[route & (3 << 2)]
    return "%s / %s%s%s" % (form, pset, ", sparse" if route & SPARSE else "", ", widened" if route & WIDENED else "")


def binning(count, record, scatter):
    return count | record << 2 | scatter << 4


def describe_binning(code):
    return "%s / %s / %s" % (("global", "lds", "lds-keyed", "?")[code & 3], ("as-is", "short2", "ranked8", "?")[(code >> 2) & 3],
                             ("ballot", "rank", "pre", "?")[(code >> 4) & 3])


def _row(name, entry, sizes, want, pol=False, opts=(), events="random", dict_valid=False, want_count=None):
    """want_count: the count pass a SLOTS row must record in "slot_binning" (None: not asserted)"""
    return dict(name=name, entry=entry, sizes=list(sizes), want=want, pol=pol, opts=tuple(opts), events=events, dict_valid=dict_valid,
                want_count=want_count)


# A row is a list of calls on ONE context, in order (only the dictionary row has more than one).
# events: "random" (float events anywhere / raw events anywhere), "mapped" (float events a loader resolved through the maps: the
# positions repeat), "same" (the previous call's events, cut to the call's size)
ROWS = [
    [_row("float 16384", "gauss", [16384], DIRECT | NONE)],
    [_row("float 16385", "gauss", [16385], LISTS | NONE)],
    [_row("raw 16384", "gauss_raw", [16384], DIRECT | MAPS)],
    [_row("raw 16385", "gauss_raw", [16385], SLOTS | MAPS)],
    [_row("raw pol 16385", "gauss_raw", [16385], LISTS | MAPS, pol=True)],
    [_row("raw count image", "count_raw", [3000], LISTS | MAPS)],
    [_row("raw count image, large", "count_raw", [20000], LISTS | MAPS)],
    [_row("float bulk 11040, no dictionary", "gauss", [11040], SLOTS | PER_CALL, opts=BULK + (("position_dict", 0),), events="mapped")],
    [_row("float bulk 11039, no dictionary", "gauss", [11039], LISTS | PER_CALL | SPARSE, opts=BULK + (("position_dict", 0),), events="mapped")],
    [_row("float bulk 11040, first call", "gauss", [11040], SLOTS | PER_CALL, opts=BULK, events="mapped"),
     _row("float bulk 11040, same events again", "gauss", [11040], SLOTS | DICT, opts=BULK, events="same", dict_valid=True, want_count=COUNT_LDS_KEYED),
     # (the dictionary path has no load test)
     _row("float bulk 5000, third call", "gauss", [5000], SLOTS | DICT, opts=BULK, events="same", dict_valid=True, want_count=COUNT_LDS_KEYED)],
    [_row("raw batch 5 x 11040", "batch_raw", [11040] * 5, SLOTS | MAPS)],
    [_row("raw batch 5, sum 55199", "batch_raw", [11040] * 4 + [11039], LISTS | MAPS | SPARSE)],
    [_row("raw batch 4 x 4096", "batch_raw", [4096] * 4, DIRECT | MAPS)],
    # (not direct: more than 4 slices; 4 * 16384 < 5 * 690 * 64, so the sparse gather)
    [_row("raw batch 5, sum 16384", "batch_raw", [3277] * 4 + [3276], LISTS | MAPS | SPARSE)],
    [_row("raw4 batch 3 x 1500", "batch_raw4", [1500] * 3, DIRECT | MAPS | WIDENED)],
    [_row("raw4 batch 5, sum 55199", "batch_raw4", [11040] * 4 + [11039], LISTS | MAPS | SPARSE | WIDENED)],
    [_row("raw 10, slot lists forced", "gauss_raw", [10], SLOTS | MAPS, opts=(("gather_form", 4),))],
    [_row("raw 16385, sparse gather forced", "gauss_raw", [16385], LISTS | MAPS | SPARSE, opts=(("gather_form", 2),))],
    [_row("raw 16385, dense gather forced", "gauss_raw", [16385], LISTS | MAPS, opts=(("gather_form", 1),))],
    [_row("raw 20000, binning-free forced", "gauss_raw", [20000], DIRECT | MAPS, opts=(("gather_form", 3),))],
    # (slot lists forced on a polarity image: not eligible, the list pipeline with its dense gather)
    [_row("raw pol 16385, slot lists forced", "gauss_raw", [16385], LISTS | MAPS, pol=True, opts=(("gather_form", 4),))],
]


# ---- the rules themselves, from a plain g++ build of the header ---------------------------------------------------------------------
_exe = None


def plan_exe():
    global _exe
    if _exe is None:
        d = tempfile.mkdtemp(prefix="accum_plan_")
        exe = os.path.join(d, "accum_plan_check")
        p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "host", "accum_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        _exe = exe
    return _exe


def plan(queries):
    """queries: dicts with any of W H sigma mode_count B nev raw pol gather_form dedupe_min_events position_dict slot_rank rank_ok
    dict_valid scatter slots_usable, and for the slot form's own plans stride sensor_w sensor_h (0: the image) dict (0 none, 1 4-byte rows,
    2 2-byte ids) slot_prerank ncu sl_null slot_hot_min nparts -> per query a dict(route, pipeline_chunk, slot_ok, slot_chunk,
    slot_scatter_rank, bulk_fits, host_events; slot_waves, bin_ok, count, record, scatter, bin_stride, scat_stride, lds_count, lds_scatter,
    slot_binning; g_lds ... g_hot_waves: the SlotGatherPlan of the whole batch as one part)."""
    keys = ("W", "H", "sigma", "mode_count", "B", "nev", "raw", "pol", "gather_form", "dedupe_min_events", "position_dict", "slot_rank", "rank_ok",
            "dict_valid", "scatter", "slots_usable", "stride", "sensor_w", "sensor_h", "dict", "slot_prerank", "ncu", "sl_null", "slot_hot_min", "nparts")
    dflt = dict(W=W, H=H, sigma=SIGMA, mode_count=0, B=1, nev=0, raw=0, pol=0, gather_form=0, dedupe_min_events=1 << 20, position_dict=1, slot_rank=-1,
                rank_ok=1, dict_valid=0, scatter=2, slots_usable=1, stride=16, sensor_w=0, sensor_h=0, dict=0, slot_prerank=-1, ncu=256, sl_null=240,
                slot_hot_min=-1, nparts=1)
    lines = []
    for q in queries:
        assert set(q) <= set(keys), q
        v = dict(dflt, **q)
        lines.append(" ".join(repr(float(v[k])) if k == "sigma" else str(int(v[k])) for k in keys))
    out = subprocess.run([plan_exe()], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = ("route", "pipeline_chunk", "slot_ok", "slot_chunk", "slot_scatter_rank", "bulk_fits", "host_events",
             "slot_waves", "bin_ok", "count", "record", "scatter", "bin_stride", "scat_stride", "lds_count", "lds_scatter", "slot_binning",
             "g_lds", "g_wg_per_cu", "g_nw", "g_rounds", "g_tasks", "g_max_per_tile", "g_prio_ref", "g_hot_min", "g_hot_cap", "g_hot_waves")
    res = [dict(zip(names, (int(x) for x in ln.split()))) for ln in out.stdout.strip().split("\n")]
    assert len(res) == len(lines), out.stdout
    return res


def query_of(call):
    raw, mode = ENTRIES[call["entry"]]
    q = dict(B=len(call["sizes"]), nev=sum(call["sizes"]), raw=raw, mode_count=mode, pol=int(call["pol"]), dict_valid=int(call["dict_valid"]))
    q.update(dict(call["opts"]))
    return q


def planned_route(entry, sizes, pol=False, opts=(), dict_valid=False, W=W, H=H, sigma=SIGMA, **more):
    """The first-choice route of one call: what serves it when nothing declines at run time."""
    q = query_of(dict(entry=entry, sizes=list(sizes), pol=pol, opts=tuple(opts), dict_valid=dict_valid))
    q.update(W=W, H=H, sigma=sigma, **more)
    return plan([q])[0]["route"]


def possible_routes(entry, sizes, pol=False, opts=(), dict_valid=None, W=W, H=H, sigma=SIGMA):
    """What may serve one call when the test does not control the run-time state: the planned route with the positions' slot tables
    usable or not (half windows beyond 4, tiles of more than 254 slots) and, unless the caller knows (dict_valid), with a frozen
    dictionary or without."""
    q = query_of(dict(entry=entry, sizes=list(sizes), pol=pol, opts=tuple(opts), dict_valid=False))
    q.update(W=W, H=H, sigma=sigma)
    dicts = (0, 1) if dict_valid is None else (int(dict_valid),)
    return {r["route"] for r in plan([dict(q, dict_valid=d, slots_usable=u) for d in dicts for u in (0, 1)])}


def assert_route(ctx, what, entry, sizes, pol=False, opts=(), dict_valid=None, W=W, H=H, sigma=SIGMA):
    """The route the context recorded for its last call is one the rules give for these arguments; returns it."""
    route = ctx.debug_counter("accum_route")
    ok = possible_routes(entry, sizes, pol, opts, dict_valid, W, H, sigma)
    assert route in ok, (what, describe(route), sorted(describe(r) for r in ok))
    return route


def forms_of(route):
    return route & 3
