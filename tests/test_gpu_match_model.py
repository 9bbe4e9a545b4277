"""The HIP matchers on the planted scenes of tests/match_scenes.py: byte equality with the oracle and with the brute-force models of
tests/match_model.py (tests/test_oracle_match_model.py shows on the CPU that these scenes tell every wrong variant from the rule).
The window matchers run on a default context and on three whose capacities force the full scan, the pool overflow and the global-memory
lists, so that the fixed points, the 64-lane walk and the full scan each meet every site."""
import numpy as np
import pytest

import match_model as mm
import match_scenes as ms

pytestmark = pytest.mark.gpu

CONTEXTS = {"default": {}, "list cap 2": {"win_list_cap": 2}, "pool cap 40": {"win_pool_cap": 40}, "lds entries 1": {"win_lds_entries": 1}}


@pytest.fixture(scope="module")
def fe():
    from eorb_slam_amd import frontend
    return frontend


@pytest.fixture(scope="module", params=sorted(CONTEXTS))
def wctx(fe, request):
    c = fe.Context()
    for k, v in CONTEXTS[request.param].items():
        c.debug_option(k, v)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx(fe):
    c = fe.Context()
    yield c
    c.close()


_WANT = {}


def _expected(oracle, key, sc, cfg, check_ori, run_oracle, run_model):
    """the oracle's answer, which must be the model's: computed once per scene and setting"""
    if key not in _WANT:
        o = run_oracle(oracle, sc, cfg, check_ori)
        m = run_model(sc, cfg, check_ori)
        assert ms.same(o, m), "%s: the oracle differs from the model" % (key,)
        _WANT[key] = o
    return _WANT[key]


def _differs(got, want, names):
    bad = np.flatnonzero(np.asarray(got[1]) != np.asarray(want[1]))
    return "nmatches %d, expected %d; %d entries differ, first %s%s" % (got[0], want[0], len(bad), bad[:5],
                                                                        "" if names is None or not len(bad) or len(names) != len(got[1]) else " (%s)" % names[bad[0]])


WINDOW_SCENES = [(k, n) for k in ms.KINDS for n in ["base", "positions"] + [h for h in ms.HISTOGRAMS if ms.histogram_applies(h, k)]]


@pytest.mark.parametrize("kind,name", WINDOW_SCENES)
def test_window_matchers(oracle, fe, wctx, kind, name):
    sc = ms.window_scene(kind, name == "positions") if name in ("base", "positions") else ms.histogram_scene(kind, name)
    for cfg in ms.window_configs(kind):
        for check_ori in (True, False) if kind != "map" and cfg == ms.MAIN[kind] else (True,):
            want = _expected(oracle, (kind, name, ms.config_id(cfg), check_ori), sc, cfg, check_ori, ms.run_oracle, ms.run_model)
            got = ms.run_kernels(fe, wctx, sc, cfg, check_ori)
            assert ms.same(got, want), "%s %s %s ori=%d: %s" % (kind, name, ms.config_id(cfg), check_ori,
                                                                 _differs(got, want, sc["names"] if kind == "init" else None))


# ---- the node-walk matchers ------------------------------------------------------------------------------------------------------
NODE_SCENES = [(k, n) for k in ms.NODE_KINDS for n in ["base"] + [h for h in ms.HISTOGRAMS if ms.node_histogram_applies(h, k)]]
TRIPLES = [("four equal", "max2 = 2", "rounding"), ("max2 = 1", "max3 = 2", "max3 = 1"), ("rounding", "one bin", "max3 = 1")]


def _node_scene(kind, name):
    return ms.node_scene(kind) if name == "base" else ms.node_histogram_scene(kind, name)


def _node_expected(oracle, kind, name, cfg, check_ori):
    return _expected(oracle, (kind, name, ms.config_id(cfg), check_ori), _node_scene(kind, name), cfg, check_ori, ms.run_node_oracle, ms.run_node_model)


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("kind,name", NODE_SCENES)
def test_node_walk_matchers(oracle, fe, ctx, kind, name, batched):
    """SearchByBoW, SearchByBoW KF-KF and SearchForTriangulation: the single-pair entry points, and the *_KeyFrames ones with K = 1"""
    sc = _node_scene(kind, name)
    for cfg in ms.node_configs(kind):
        for check_ori in (True, False):
            want = _node_expected(oracle, kind, name, cfg, check_ori)
            got = ms.run_node_kernels(fe, ctx, [sc], cfg, check_ori, batched)[0]
            assert ms.same(got, want), "%s %s %s ori=%d batched=%d: %s" % (kind, name, ms.config_id(cfg), check_ori, batched, _differs(got, want, None))


@pytest.mark.parametrize("triple", TRIPLES)
@pytest.mark.parametrize("kind", ms.NODE_KINDS)
def test_node_walk_keyframes_k3(oracle, fe, ctx, kind, triple):
    """K = 3: keyframe k takes histogram variant k, so that every pair of the call has a histogram and a counter of its own"""
    scenes = [_node_scene(kind, name) for name in triple]
    for cfg in ms.node_configs(kind):
        got = ms.run_node_kernels(fe, ctx, scenes, cfg, True, True)
        for k, name in enumerate(triple):
            want = _node_expected(oracle, kind, name, cfg, True)
            assert ms.same(got[k], want), "%s %s keyframe %d (%s): %s" % (kind, ms.config_id(cfg), k, name, _differs(got[k], want, None))
