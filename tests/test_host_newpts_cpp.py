"""The C++ mirror of the triangulation stage (ORB_SLAM3::CreateNewMapPoints, eorb_slam_amd/host/eorb_host.hpp) from a plain g++ caller
(tests/host/newpts_check.cpp): it must compile and link against libeorb_fe.so, and on a GPU box what it returns on two scenes equals the
restatement (tests/newpts_ref), byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newpts_ref as nr                             # noqa: E402
from newpts_ref import scenes                       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = (("status", np.uint8), ("x3d", np.float32), ("branch", np.uint8), ("cos_parallax", np.float32), ("n_new", np.int32))


def _build(tmp):
    from eorb_slam_amd import _lib
    lib = _lib.build()
    exe = os.path.join(tmp, "newpts_check")
    libdir = os.path.dirname(lib)
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "host", "newpts_check.cpp"), "-o", exe, "-L", libdir,
                        "-leorb_fe", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_newpts_mirror_compiles_and_links(tmp_path):
    exe = _build(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "linked" in out.stdout


def _write(tmp_path, sc):
    put = lambda n, a, dt: np.ascontiguousarray(a, dt).tofile(str(tmp_path / (n + ".bin")))      # noqa: E731
    put("kps1", sc["kps1"], sc["kps1"].dtype); put("kps2", sc["kps2"], sc["kps2"].dtype); put("kf_off", sc["kf_off"], np.int32)
    put("match12", sc["match12"], np.int32)
    v1, v2 = nr.views(sc)
    for name, vs in (("views1", v1), ("views2", [v for pair in v2 for v in pair])):
        with open(str(tmp_path / (name + ".bin")), "wb") as f:
            for v in vs:
                f.write(bytes(v))
    put("par_i", [sc["form"], sc["nleft1"], int(sc["far_points"])], np.int32)
    put("par_f", [sc["mb1"], sc["rf_orb"], sc["rf_ak"], sc["th_far"]], np.float32)
    put("level_scale", sc["level_scale"], np.float32); put("level_sigma2", sc["level_sigma2"], np.float32)
    if sc["nleft2"] is not None:
        put("nleft2", sc["nleft2"], np.int32)
    if sc["mb2"] is not None:
        put("mb2", sc["mb2"], np.float32)
    for side in ("side1", "side2"):
        for key, a in sc[side].items():
            put(side + "_" + key, a, np.uint8 if key == "kp_is_orb" else np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stereo", "mixed"])
def test_newpts_mirror_equals_the_restatement(tmp_path, name):
    exe = _build(str(tmp_path))
    sc = scenes.all_scenes()[name]
    _write(tmp_path, sc)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "done" in out.stdout, out.stdout + out.stderr
    ref = nr.loop(sc)
    for key, dt in OUT:
        got = np.fromfile(str(tmp_path / (key + ".bin")), dt)
        assert got.tobytes() == np.ascontiguousarray(ref[key]).tobytes(), (name, key)
    assert (ref["status"] == nr.S["new"]).sum() >= 20
