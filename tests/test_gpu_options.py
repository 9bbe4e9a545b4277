"""The switches of a context (eorb_slam_amd/csrc/eorb_options.h) through the C ABI: eorb_create seeds every row from the environment
or its default, eorb_debug_option sets a row of one context, eorb_debug_option_get reads it back.  A device is needed because
eorb_create needs one; only the last test launches kernels."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from options_rows import DEFAULTS, NOT_SET, ROWS, SEED, SEEDED       # noqa: E402
from eorb_slam_amd import synth                                       # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a legal value per row that is not its default: the seeded one where the row has an environment name
LEGAL = dict(SEEDED, octree_pool_shrink=3, octree_force_global=1, octree_list_algorithm=1, orb_three_launches=1, win_list_cap=64, win_pool_cap=2048,
             win_lds_entries=512, gather_form=4, slot_hot_cap=16, kfdb_initial_slots=8, kfdb_finish_lds_entries=32, dedupe_min_events=1000,
             position_dict=0, dirty_fill=0xA5)


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


def _read(c):
    return {name: c.debug_option_get(name) for name in ROWS}


def test_a_fresh_context_runs_with_the_defaults(fe):
    assert not any(e in os.environ for e in SEED), "this test needs the switches' environment names unset"
    c = fe.Context()
    assert _read(c) == DEFAULTS == {
        "octree_pool_shrink": 0, "octree_force_global": 0, "octree_list_algorithm": 0, "orb_three_launches": 0, "win_list_cap": 0, "win_pool_cap": 0,
        "win_lds_entries": 0, "gather_form": 0, "slot_hot_cap": 0, "kfdb_initial_slots": 0, "kfdb_finish_lds_entries": 0,
        "dedupe_min_events": 1048576, "position_dict": 1, "dirty_fill": -1, "slot_rank": 1, "slot_hot_min": -1, "slot_hot_waves": 0, "slot_prerank": 1,
        "slot_halves": -1, "scatter": 2, "gather_threads": 0, "gather_nc": 0, "slot_chunk": 0, "slot_waves": 0, "slot_rounds": 0, "win_cand_waves": 0,
        "win_qpb": 0, "upload_kernel_max": 1048576, "download_kernel_max": 1048576, "sync_spin": 0, "slice_zero_copy": 1, "image_zero_copy": 1,
        "contest_direct_max": 49152, "octree_budget_kb": 156, "octree_direct": 1, "octree_dynamic": 1, "orb_describe": 1}
    c.close()


def test_set_and_read_back(fe):
    c = fe.Context()
    assert set(LEGAL) == set(ROWS) and all(LEGAL[n] != DEFAULTS[n] for n in ROWS)
    want = dict(DEFAULTS)
    for name in ROWS:
        c.debug_option(name, LEGAL[name])
        want[name] = LEGAL[name]
        assert _read(c) == want, name                                           # the row moved, no other did
    for name, u in NOT_SET.items():                                             # "not set": what eorb_create gave
        c.debug_option(name, u)
        assert c.debug_option_get(name) == DEFAULTS[name], name
    with pytest.raises(fe.EorbError) as e:
        c.debug_option("no_such_option", 1)
    assert e.value.code == -4 and "debug option 'no_such_option' unknown" in str(e.value)
    with pytest.raises(fe.EorbError) as e:
        c.debug_option_get("no_such_option")
    assert e.value.code == -4 and "debug option 'no_such_option' unknown" in str(e.value)
    c.debug_option("dirty_fill", -1)
    for bad in (256, -2):
        with pytest.raises(fe.EorbError) as e:
            c.debug_option("dirty_fill", bad)
        assert e.value.code == -4 and "dirty_fill: -1 (off) or a byte 0..255, not %d" % bad in str(e.value)
        assert c.debug_option_get("dirty_fill") == -1
    for ok in (0, 255, -1):
        c.debug_option("dirty_fill", ok)
        assert c.debug_option_get("dirty_fill") == ok
    c.close()


def test_two_contexts_do_not_share_a_row(fe):
    a, b = fe.Context(), fe.Context()
    for name in ROWS:
        a.debug_option(name, LEGAL[name])
    assert _read(a) == LEGAL and _read(b) == DEFAULTS
    b.debug_option("slot_halves", 1)
    assert a.debug_option_get("slot_halves") == LEGAL["slot_halves"] and b.debug_option_get("slot_halves") == 1
    a.close(); b.close()


def test_the_environment_seeds_a_context():
    code = r"""
import json, os, sys
sys.path.insert(0, os.getcwd())
from eorb_slam_amd import frontend as fe
names = json.loads(sys.argv[1])
c = fe.Context()
seeded = {n: c.debug_option_get(n) for n in names}
c.debug_option("slot_hot_min", 7000); set_ = c.debug_option_get("slot_hot_min")
c.debug_option("slot_hot_min", -1); back = c.debug_option_get("slot_hot_min")
c.debug_option("scatter", 2)
d = fe.Context()
print("RESULT " + json.dumps({"seeded": seeded, "set": set_, "back": back, "scatter": [c.debug_option_get("scatter"), d.debug_option_get("scatter")]}))
c.close(); d.close()
"""
    env = dict(os.environ, **{k: str(v) for k, v in SEED.items()})
    p = subprocess.run([sys.executable, "-c", code, json.dumps(sorted(ROWS))], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    r = json.loads([ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")][0][7:])
    assert r["seeded"] == SEEDED
    assert r["set"] == 7000 and r["back"] == 5000                               # an option over the seed; "not set" puts the seed back
    assert r["scatter"] == [2, 1]                                               # a second context is seeded afresh


def test_warped_events_are_not_tabulated_and_the_threshold_stays(fe):
    """eorb_ev2mci_* hand the accumulation warped events, of which no two share a position: that call runs with dd_min = 0 whatever
    "dedupe_min_events" says, and the context's row is not touched -- the next plain float call is tabulated again.
    accum_route: form | position set << 2 (0 none, 1 the maps, 2 the call's own tabulated positions, 3 the dictionary).  With the
    threshold borrowed as a parameter (saved, zeroed, restored around the call) the two routes at this size were 1 and 10."""
    W, H, n = 64, 48, 4096
    ev = synth.random_events(n, W, H, seed=31)
    c = fe.Context()
    c.debug_option("dedupe_min_events", 1)
    fe.EvImConverter.ev2mci_gg_f_se2(ev, (60.0, 59.5, 31.5, 23.5), [0.03, 0.4, -0.3], W, H, 1.0, False, False, ctx=c)
    assert c.debug_option_get("dedupe_min_events") == 1
    route = c.debug_counter("accum_route")
    assert route != 0 and route & 12 == 0, route
    fe.EvImConverter.ev2im_gauss(ev, W, H, 1.0, False, False, ctx=c)
    route = c.debug_counter("accum_route")
    assert (route >> 2) & 3 in (2, 3), route
    assert c.debug_option_get("dedupe_min_events") == 1
    c.close()
