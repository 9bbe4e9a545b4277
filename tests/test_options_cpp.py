"""The switch table without a device (eorb_slam_amd/csrc/eorb_options.h through tests/host/options_check.cpp, plain g++): the defaults,
the environment as seed, option calls over it, and the five rows whose "not set" value puts the created value back.  The expectations
are literals, written from the rule table that stood above accum_knobs in ev_accum.hip:

    knob             option                     environment             rule
    gather_form      "gather_form"              --                      option
    dd_min           "dedupe_min_events"        --                      option
    pd               "position_dict"            --                      option
    scatter          --                         EORB_SCATTER (2)        environment
    gather_threads   --                         EORB_GATHER_THREADS     environment if 192..1024 and a multiple of 64, else the build's
    gather_nc        --                         EORB_GATHER_NC (0)      environment
    slot_chunk       --                         EORB_SLOT_CHUNK (0)     environment if 256 / 1024 / 2048 / 4096, else 0
    slot_waves       --                         EORB_SLOT_WAVES (0)     environment
    slot_rounds      --                         EORB_SLOT_ROUNDS (0)    environment
    slot_rank        "slot_rank" (-1)           EORB_SLOT_RANK (1)      option if >= 0, else environment; non-zero: allowed
    slot_hot_min     "slot_hot_min" (-1)        EORB_SLOT_HOT_MIN (-1)  option if >= 0, else environment
    slot_hot_cap     "slot_hot_cap" (0)         --                      option
    slot_hot_waves   "slot_hot_waves" (0)       EORB_SLOT_HOT_WAVES (0) option if > 0, else environment if > 0, else 0
    slot_prerank     "slot_prerank" (-1)        EORB_SLOT_PRERANK (1)   option if >= 0, else environment
    slot_halves      "slot_halves" (-1)         EORB_SLOT_HALVES (-1)   option if >= 0, else environment
"""
import os
import subprocess
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from options_rows import DEFAULTS, NOT_SET, ROWS, SEED, SEEDED       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eorb_slam_amd", "csrc")

# a default-constructed AccumKnobs (ev_plan.h) with gather_threads 512
KNOB_DEFAULTS = {"gather_form": 0, "dd_min": 1 << 20, "pd": 1, "scatter": 2, "gather_threads": 512, "gather_nc": 0, "slot_chunk": 0, "slot_waves": 0,
                 "slot_rounds": 0, "slot_rank": 1, "slot_hot_min": -1, "slot_hot_cap": 0, "slot_hot_waves": 0, "slot_prerank": 1, "slot_halves": -1}

@pytest.fixture(scope="module")
def exe():
    d = tempfile.mkdtemp(prefix="options_")
    path = os.path.join(d, "options_check")
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "host", "options_check.cpp"), "-o", path],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return path


@pytest.fixture(scope="module")
def run(exe):
    def ask(scenarios):
        """scenarios: [(environment dict, [(option, value), ...])] -> [{"opt": {..}, "knob": {..}, "call": [(name, known), ..]}]"""
        text = "".join(" ".join("%s=%s" % kv for kv in env.items()) + " | " + " ".join("%s %d" % c for c in calls) + "\n" for env, calls in scenarios)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        res, cur = [], {"opt": {}, "knob": {}, "call": []}
        for ln in out.stdout.split("\n"):
            t = ln.split()
            if not t:
                continue
            if t[0] == "end":
                res.append(cur); cur = {"opt": {}, "knob": {}, "call": []}
            elif t[0] == "call":
                cur["call"].append((t[1], int(t[2])))
            else:
                assert t[1] not in cur[t[0]], ln
                cur[t[0]][t[1]] = int(t[2])
        assert len(res) == len(scenarios), out.stdout
        return res

    def one(env=None, calls=()):
        return ask([(env or {}, list(calls))])[0]
    ask.one = one
    return ask


def test_the_table(exe):
    out = subprocess.run([exe, "table"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = [ln.split()[1:] for ln in out.stdout.strip().split("\n")]
    names = [r[0] for r in rows]
    envs = [r[1] for r in rows if r[1] != "-"]
    assert len(set(names)) == len(names) == 37 and len(set(envs)) == len(envs) == 23
    assert all(e.startswith("EORB_") for e in envs)
    assert {r[0]: (None if r[1] == "-" else r[1], int(r[2])) for r in rows} == ROWS
    # "not set": 1 = a value < 0, 2 = a value <= 0; every other row takes any value
    assert {r[0]: int(r[3]) for r in rows if r[3] != "0"} == {"slot_rank": 1, "slot_hot_min": 1, "slot_hot_waves": 2, "slot_prerank": 1, "slot_halves": 1}


def test_nothing_set(run):
    r = run.one()
    assert r["opt"] == DEFAULTS and r["knob"] == KNOB_DEFAULTS and r["call"] == []


def test_every_environment_name_seeds_its_row(run):
    assert len(SEED) == 23 == len(set(SEED.values())) and all(SEEDED[o] != DEFAULTS[o] for o, (e, _) in ROWS.items() if e)
    r = run.one({k: str(v) for k, v in SEED.items()})
    assert r["opt"] == SEEDED
    assert r["knob"] == {"gather_form": 0, "dd_min": 1 << 20, "pd": 1, "scatter": 1, "gather_threads": 384, "gather_nc": 4, "slot_chunk": 1024,
                         "slot_waves": 8, "slot_rounds": 6, "slot_rank": 1, "slot_hot_min": 5000, "slot_hot_cap": 0, "slot_hot_waves": 96,
                         "slot_prerank": 26, "slot_halves": 3}
    # one at a time: only its own row moves
    for (env, v), r in zip(SEED.items(), run([({env: str(v)}, []) for env, v in SEED.items()])):
        opt = [o for o, (e, _) in ROWS.items() if e == env][0]
        assert r["opt"] == dict(DEFAULTS, **{opt: v}), env


def test_gather_threads_and_slot_chunk_are_validated_in_the_knob(run):
    gt = [191, 192, 200, 1024, 1088]
    res = run([({"EORB_GATHER_THREADS": str(v)}, []) for v in gt])
    assert [r["knob"]["gather_threads"] for r in res] == [512, 192, 512, 1024, 512]
    assert [r["opt"]["gather_threads"] for r in res] == gt                       # the row holds what was given
    sc = [256, 512, 4096, 8192]
    res = run([({"EORB_SLOT_CHUNK": str(v)}, []) for v in sc])
    assert [r["knob"]["slot_chunk"] for r in res] == [256, 0, 4096, 0]
    assert [r["opt"]["slot_chunk"] for r in res] == sc
    # the same through option calls
    assert [r["knob"]["gather_threads"] for r in run([({}, [("gather_threads", v)]) for v in gt])] == [512, 192, 512, 1024, 512]
    assert [r["knob"]["slot_chunk"] for r in run([({}, [("slot_chunk", v)]) for v in sc])] == [256, 0, 4096, 0]


def test_negative_hot_waves_is_zero_in_the_knob(run):
    r = run.one({"EORB_SLOT_HOT_WAVES": "-3"})
    assert r["knob"]["slot_hot_waves"] == 0 and r["opt"]["slot_hot_waves"] == -3
    r = run.one({"EORB_SLOT_HOT_WAVES": "-3"}, [("slot_hot_waves", 0)])
    assert r["knob"]["slot_hot_waves"] == 0


# row, environment name, default d, environment value a, set value b, a "not set" value u, the knob of a row value
R_ROWS = [
    ("slot_rank", "EORB_SLOT_RANK", 1, 0, 2, -1, lambda v: int(v != 0)),
    ("slot_hot_min", "EORB_SLOT_HOT_MIN", -1, 5000, 7000, -1, lambda v: v),
    ("slot_hot_min", "EORB_SLOT_HOT_MIN", -1, 5000, 0, -7, lambda v: v),           # (0 is a set value: the register-row kernel off)
    ("slot_hot_waves", "EORB_SLOT_HOT_WAVES", 0, 96, 64, 0, lambda v: max(v, 0)),
    ("slot_hot_waves", "EORB_SLOT_HOT_WAVES", 0, 96, 64, -2, lambda v: max(v, 0)),
    ("slot_prerank", "EORB_SLOT_PRERANK", 1, 0, 2, -1, lambda v: v),
    ("slot_halves", "EORB_SLOT_HALVES", -1, 1, 0, -1, lambda v: v),                # (0 is a set value: one part)
]


@pytest.mark.parametrize("row,env,d,a,b,u,knob", R_ROWS)
def test_not_set_puts_the_created_value_back(run, row, env, d, a, b, u, knob):
    assert ROWS[row] == (env, d)
    calls = [[], [(row, u)], [(row, b)], [(row, b), (row, u)]]
    want = {False: [d, d, b, d], True: [a, a, b, a]}                            # "option if set, else environment, else default"
    for seeded in (False, True):
        res = run([({env: str(a)} if seeded else {}, c) for c in calls])
        assert [r["opt"][row] for r in res] == want[seeded], (row, seeded)
        assert [r["knob"][row] for r in res] == [knob(v) for v in want[seeded]], (row, seeded)
        for r, c in zip(res, calls):
            assert r["call"] == [(row, 1)] * len(c)
            others = dict(DEFAULTS, **{row: r["opt"][row]})
            assert r["opt"] == others                                           # no other row moves


def test_other_rows_store_a_negative_value_as_given(run):
    names = [n for n in ROWS if n not in NOT_SET]
    assert len(names) == 32 and set(NOT_SET) == {r[0] for r in R_ROWS}
    for n, r in zip(names, run([({}, [(n, -1)]) for n in names])):
        assert r["opt"] == dict(DEFAULTS, **{n: -1}) and r["call"] == [(n, 1)], n
    r = run.one({}, [("win_list_cap", -5), ("dedupe_min_events", 0), ("contest_direct_max", -2)])
    assert (r["opt"]["win_list_cap"], r["opt"]["dedupe_min_events"], r["opt"]["contest_direct_max"]) == (-5, 0, -2)
    assert r["knob"]["dd_min"] == 0


def test_option_over_environment(run):
    r = run.one({"EORB_SCATTER": "1", "EORB_WIN_QPB": "32"}, [("scatter", 2), ("gather_form", 4), ("position_dict", 0), ("slot_hot_cap", 3)])
    assert r["opt"] == dict(DEFAULTS, scatter=2, win_qpb=32, gather_form=4, position_dict=0, slot_hot_cap=3)
    assert r["knob"] == dict(KNOB_DEFAULTS, gather_form=4, pd=0, slot_hot_cap=3)


def test_unknown_name(run):
    r = run.one({"EORB_NOT_A_KNOB": "5", "SLOT_RANK": "0"}, [("no_such_option", 3), ("EORB_SLOT_RANK", 0)])
    assert r["call"] == [("no_such_option", 0), ("EORB_SLOT_RANK", 0)]
    assert r["opt"] == DEFAULTS and r["knob"] == KNOB_DEFAULTS


def test_environment_value_that_is_no_number(run):
    res = run([({"EORB_SCATTER": "fast"}, []), ({"EORB_UPLOAD_KERNEL_MAX": "x1"}, []), ({"EORB_SLOT_HALVES": "12abc"}, [])])
    assert res[0]["opt"] == dict(DEFAULTS, scatter=0) and res[1]["opt"] == dict(DEFAULTS, upload_kernel_max=0)
    assert res[2]["opt"] == dict(DEFAULTS, slot_halves=12)                      # atoll: the leading digits


def test_one_reader_of_the_environment_and_no_debug_fields():
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h")):
            continue
        txt = open(os.path.join(CSRC, f)).read()
        assert "dbg_" not in txt, f
        assert f == "eorb_options.h" or "getenv(" not in txt, f
    assert open(os.path.join(CSRC, "eorb_options.h")).read().count("getenv(") == 1
