"""The C++ mirror of the matchers over K keyframes per call (the ORB_SLAM3::ORBmatcher::SearchForTriangulation / SearchByBoW overloads that
take a vector of keyframes, eorb_slam_amd/host/eorb_host.hpp) from a plain g++ caller (tests/host/kfbatch_check.cpp): it must compile and
link against libeorb_fe.so, and on a GPU box the rows it returns equal the oracle rows of tests/kfbatch_cases.py as bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfbatch_cases as kc                          # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3


def _build(tmp):
    from eorb_slam_amd import _lib
    lib = _lib.build()
    exe = os.path.join(tmp, "kfbatch_check")
    libdir = os.path.dirname(lib)
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "host", "kfbatch_check.cpp"), "-o", exe, "-L", libdir,
                        "-leorb_fe", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_keyframe_list_mirror_compiles_and_links(tmp_path):
    exe = _build(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "linked" in out.stdout


def _put(tmp, name, a):
    np.ascontiguousarray(a).tofile(str(tmp / (name + ".bin")))


def _put_kf(tmp, base, kps, desc, flag, fv):
    for name, a in (("kps", kps), ("desc", desc), ("flag", flag), ("nodes", fv[0].astype(np.uint32)), ("off", fv[1].astype(np.int32)),
                    ("idx", fv[2].astype(np.int32))):
        _put(tmp, base + "_" + name, a)


@pytest.mark.gpu
def test_keyframe_list_mirror_equals_the_oracle_rows(tmp_path, oracle):
    exe = _build(str(tmp_path))
    for scene, kind in (("tri", "pinhole"), ("kb8", "kb8")):
        s = kc.tri_scene(kind, K)
        _put(tmp_path, scene + "_hdr", np.array([K, s["desc1"].shape[1]], np.int32))
        _put_kf(tmp_path, scene + "_c", s["kps1"], s["desc1"], s["elig1"], s["fv1"])
        for k, kf in enumerate(s["kfs"]):
            _put_kf(tmp_path, "%s_k%d" % (scene, k), kf["kps"], kf["desc"], kf["elig"], kf["fv"])
        _put(tmp_path, scene + "_ep", s["ep"]); _put(tmp_path, scene + "_scale", s["scale2"]); _put(tmp_path, scene + "_sigma2", s["sigma2_2"])
    _put(tmp_path, "tri_F12", kc.tri_scene("pinhole", K)["F12"])
    _put(tmp_path, "kb8_Rt", kc.tri_scene("kb8", K)["Rt"])
    _put(tmp_path, "kb8_cam", np.array(synth.CAM_MONO, np.float32))
    b = kc.bow_scene("big", K)
    _put(tmp_path, "bow_hdr", np.array([K, 32], np.int32))
    _put_kf(tmp_path, "bow_c", b["kps"], b["desc"], b["has_mp"], b["fv"])
    for k, kf in enumerate(b["kfs"]):
        _put_kf(tmp_path, "bow_k%d" % k, kf["kps"], kf["desc"], kf["has_mp"], kf["fv"])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "done" in out.stdout, out.stdout + out.stderr
    want = {"tri": kc.tri_rows("pinhole", K, False, False), "kb8": kc.tri_rows("kb8", K, False, False),
            "bow": kc.bow_rows("big", K, False, 0.7, True), "bowkf": kc.bow_rows("big", K, True, 0.8, True)}
    for name, (nm, rows) in want.items():
        assert (nm >= 20).all(), (name, nm)
        got_nm = np.fromfile(str(tmp_path / (name + "_nm.bin")), np.int32)
        got = np.fromfile(str(tmp_path / (name + "_rows.bin")), np.int32)
        assert got_nm.tobytes() == nm.astype(np.int32).tobytes(), (name, got_nm, nm)
        assert got.tobytes() == np.ascontiguousarray(rows, np.int32).tobytes(), name
