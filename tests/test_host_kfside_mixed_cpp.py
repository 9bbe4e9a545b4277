"""The C++ mirror of the mixed KeyFrame-side matchers (ORB_SLAM3::ORBmatcher::ProjectKeyFrameSideMixed / KeyFrameRadiusMatchMixed /
FuseMixed / SearchByProjectionMixed / FuseKeyFramesMixed in eorb_slam_amd/host/eorb_host.hpp) from a plain g++ caller
(tests/host/kfside_mixed_check.cpp): it must compile and link against libeorb_fe.so, and on a GPU box its outputs equal the CPU
restatement of MixedMatcher (tests/kfside_mixed_ref), bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfside_mixed_cases as cases                  # noqa: E402
import kfside_mixed_ref as mref                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp):
    from eorb_slam_amd import _lib
    lib = _lib.build()
    exe = os.path.join(tmp, "kfside_mixed_check")
    libdir = os.path.dirname(lib)
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "host", "kfside_mixed_check.cpp"), "-o", exe, "-L", libdir,
                        "-leorb_fe", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_mixed_keyframe_side_mirror_compiles_and_links(tmp_path):
    exe = _build(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "linked" in out.stdout


@pytest.mark.gpu
def test_mixed_keyframe_side_mirror_equals_the_restatement(tmp_path, oracle):
    exe = _build(str(tmp_path))
    M, n, th = cases.M, cases.N, 3.0
    sc = cases.scene()
    kw = sc["views"][0]
    p = cases.projection(th)[0]
    wbi, wbd = cases.search(oracle, sc, 0, p, "stereo")
    taken = (np.random.default_rng(3).random(n) < 0.2).astype(np.uint8)
    sbi, sbd, stk = cases.search(oracle, sc, 0, p, "none", taken=taken, accept_thr=50.0)
    assert int((wbd <= 50).sum()) >= 40 and int((sbd <= 50).sum()) >= 40

    def put(name, a):
        np.ascontiguousarray(a).tofile(str(tmp_path / (name + ".bin")))
    put("pose", np.concatenate([kw["R"].ravel(), kw["t"], kw["Ow"], np.array(kw["cam"], np.float32),
                                np.array([kw["mbf"], kw["log_scale"], kw["ak_log_scale"], th], np.float32)]).astype(np.float32))
    for name, a in (("sf", kw["scale_factors"]), ("ak_sf", kw["ak_scale_factors"]), ("kps", sc["kps"][0]), ("desc", sc["desc"][0]),
                    ("uright", sc["uright"][0]), ("pos", sc["pos"]), ("normal", sc["normal"]), ("min_dist", sc["min_dist"]),
                    ("max_dist", sc["max_dist"]), ("mp_desc", sc["mp_desc"]), ("kp_is_orb", sc["kp_is_orb"][0]),
                    ("kp_inv_sigma2", sc["kp_inv_sigma2"][0]), ("mp_is_orb", sc["mp_is_orb"]), ("taken", taken)):
        put(name, a)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr

    def got(name, dt):
        return np.fromfile(str(tmp_path / (name + ".bin")), dt)
    for name, dt, _ in mref.OUT_FIELDS:
        assert got("a_" + name, dt).tobytes() == p[name].tobytes(), name
    assert got("b_reason", np.uint8).tobytes() == p["reason"].tobytes() and got("b_level", np.int32).tobytes() == p["level"].tobytes()
    for name in ("match", "fuse"):
        assert got(name + "_idx", np.int32).tobytes() == wbi.tobytes() and got(name + "_dist", np.int32).tobytes() == wbd.tobytes(), name
    assert got("scw_idx", np.int32).tobytes() == sbi.tobytes() and got("scw_dist", np.int32).tobytes() == sbd.tobytes()
    assert got("scw_taken", np.uint8).tobytes() == stk.tobytes()
    empty_i, empty_d = np.full(M, -1, np.int32), np.full(M, 256, np.int32)
    assert got("batch_idx", np.int32).tobytes() == np.concatenate([wbi, empty_i, wbi]).tobytes()
    assert got("batch_dist", np.int32).tobytes() == np.concatenate([wbd, empty_d, wbd]).tobytes()
