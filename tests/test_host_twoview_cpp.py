"""The C++ mirror of the two-view reconstruction calls (ORB_SLAM3::TwoViewReconstruction, eorb_slam_amd/host/eorb_host.hpp) from a plain
g++ caller (tests/host/twoview_check.cpp): it must compile and link against libeorb_fe.so, and on a GPU box what it returns equals the
restatement (tests/twoview_ref) byte for byte, NaNs made canonical."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twoview_ref as tv                            # noqa: E402
from twoview_ref import scenes                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp):
    from eorb_slam_amd import _lib
    lib = _lib.build()
    exe = os.path.join(tmp, "twoview_check")
    libdir = os.path.dirname(lib)
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "host", "twoview_check.cpp"), "-o", exe, "-L", libdir,
                        "-leorb_fe", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_two_view_mirror_compiles_and_links(tmp_path):
    exe = _build(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "linked" in out.stdout


def _canon(a):
    a = np.array(a)
    if a.dtype == np.float32:
        a[np.isnan(a)] = np.float32(np.nan)
    return a.tobytes()


@pytest.mark.gpu
def test_two_view_mirror_equals_the_restatement(tmp_path):
    exe = _build(str(tmp_path))
    N, it = 130, 40
    sc = scenes.scene("mixed", N, seed=5, far=0.2)
    sets = scenes.make_sets(N, it, seed=6)
    poses = scenes.poses27(scenes.decompose_e_poses(sc["R"], sc["t"]))
    inl = (~sc["bad"]).astype(np.uint8)
    put = lambda n, a, dt: np.ascontiguousarray(a, dt).tofile(str(tmp_path / (n + ".bin")))      # noqa: E731
    put("kps1", sc["kps1"], scenes.KP_DTYPE); put("kps2", sc["kps2"], scenes.KP_DTYPE); put("matches", sc["matches"], np.int32); put("sets", sets, np.int32)
    put("K", scenes.K, np.float32); put("par", [1.0, 4.0], np.float32); put("inliers", inl, np.uint8); put("poses", poses, np.float32)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "done" in out.stdout, out.stdout + out.stderr
    get = lambda n, dt: np.fromfile(str(tmp_path / (n + ".bin")), dt)      # noqa: E731
    T = tv.TwoViewReconstruction(scenes.K)
    r = T.find_homography_fundamental(sc["kps1"], sc["kps2"], sc["matches"], sets, aids=True)
    assert r["best_it_h"] >= 0 and r["best_it_f"] >= 0
    res = get("res", np.float32)
    assert _canon(res) == _canon(np.concatenate([[r["SH"], r["SF"]], r["H21"].reshape(9), r["F21"].reshape(9)]).astype(np.float32))
    assert get("best", np.int32).tolist() == [r["best_it_h"], r["best_it_f"]]
    for name, key in (("inl_h", "inliers_h"), ("inl_f", "inliers_f")):
        assert get(name, np.uint8).tobytes() == r[key].tobytes(), name
    for name in ("it_score_h", "it_score_f", "it_H", "it_F"):
        assert _canon(get(name, np.float32)) == _canon(r[name].reshape(-1)), name
    c = T.check_rt(sc["kps1"], sc["kps2"], sc["matches"], inl, poses, th2=4.0, want_cos_all=True)
    assert c["n_good"].max() > 40
    assert get("n_good", np.int32).tobytes() == c["n_good"].tobytes() and get("good", np.uint8).tobytes() == c["good"].tobytes()
    for name, key in (("p3d", "p3d"), ("cos_sel", "cos_sel"), ("cos_all", "cos_all")):
        assert _canon(get(name, np.float32)) == _canon(c[key].reshape(-1)), name
    want = [np.degrees(np.arccos(np.float64(cs))) if ng > 0 else 0.0 for cs, ng in zip(c["cos_sel"], c["n_good"])]
    assert np.allclose(get("parallax", np.float64), want, rtol=1e-12, atol=0)
