"""eorb_bow_transform's limit without a device (eorb_slam_amd/csrc/bow_plan.h through tests/host/bow_plan_check.cpp, plain g++): from the
feature count alone the call knows P (the power of two >= max(n, 64) that bow_assemble_kernel sorts), the register class of
block_bitonic_sort_regs (keys per thread of the 1024), the LDS it asks for (18 bytes per key: key, value, 16-bit run index) and
whether it is accepted.  The documented limit is the real one: 8192 features pass, 8193 do not; the header, the front end and the
model's size classes say the same."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_model as bm                              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("P", "regs", "lds", "ok", "max_features", "lds_optin")


@pytest.fixture(scope="module")
def plan():
    d = tempfile.mkdtemp(prefix="bow_plan_")
    exe = os.path.join(d, "bow_plan_check")
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "host", "bow_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def ask(ns):
        out = subprocess.run([exe], input="".join("%d\n" % n for n in ns), capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        res = [dict(zip(NAMES, (int(x) for x in ln.split()))) for ln in out.stdout.strip().split("\n")]
        assert len(res) == len(ns), out.stdout
        return res
    return ask


@pytest.mark.parametrize("n,P,regs", [(0, 64, 1), (1, 64, 1), (64, 64, 1), (65, 128, 1), (1024, 1024, 1), (1025, 2048, 2), (4096, 4096, 4),
                                      (4097, 8192, 8), (8192, 8192, 8)])
def test_accepted_sizes(plan, n, P, regs):
    r = plan([n])[0]
    assert r["ok"] == 1 and (r["P"], r["regs"]) == (P, regs) and r["lds"] == 18 * P, r
    assert (P, regs) == bm.sort_size(n)                                     # the size classes the scenes of tests/bow_scenes.py go by
    assert P >= max(n, 64) and P & (P - 1) == 0 and (P == 64 or P // 2 < n)
    assert r["lds"] + 16 <= r["lds_optin"] == 150 * 1024                    # (16: the kernel's three static words, rounded up)
    assert P - 1 < 1 << 16                                                  # a run index fits its 16 bits


def test_refused_sizes(plan):
    for r in plan([8193, 8194, 16384, 1 << 30, 2 ** 31 - 1, -1]):
        assert r["ok"] == 0 and r["P"] == 0 and r["lds"] == 0, r
    assert plan([8192])[0]["lds"] == 147456


def test_one_limit_everywhere(plan):
    from eorb_slam_amd import frontend
    hdr = open(os.path.join(ROOT, "include", "eorb_fe.h")).read()
    m = re.search(r"#define\s+EORB_BOW_MAX_FEATURES\s+(\d+)", hdr)
    assert m and int(m.group(1)) == 8192 == plan([0])[0]["max_features"] == frontend.ORBVocabulary.MAX_FEATURES
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "`eorb_bow_transform`: ≤ 8192 features per call" in design
