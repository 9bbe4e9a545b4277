"""The C++ mirror of the MLPnP solver (ORB_SLAM3::MLPnPsolver, eorb_slam_amd/host/eorb_host.hpp) from a plain g++ caller
(tests/host/mlpnp_check.cpp): it must compile and link against libeorb_fe.so, and on a GPU box what the iterate(5, ...) calls of
Tracking::Relocalization return equals the restatement (tests/mlpnp_ref) driven the same way, byte for byte, NaNs made canonical."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlpnp_ref as mr                              # noqa: E402
from mlpnp_ref import scenes                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp):
    from eorb_slam_amd import _lib
    lib = _lib.build()
    exe = os.path.join(tmp, "mlpnp_check")
    libdir = os.path.dirname(lib)
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "host", "mlpnp_check.cpp"), "-o", exe, "-L", libdir,
                        "-leorb_fe", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_mlpnp_mirror_compiles_and_links(tmp_path):
    exe = _build(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "linked" in out.stdout


def test_draw_sets_is_the_swap_with_back_scheme(tmp_path):
    """DrawSets (:176-188) on a small linear congruential generator against the scheme written out here: six draws without replacement,
    the drawn slot refilled with the back of the list; and frontend.mlpnp_draw_sets draws sets of the same kind"""
    exe = _build(str(tmp_path))
    N, n_sets, seed = 9, 7, 12345
    out = subprocess.run([exe, "draw", str(N), str(n_sets), str(seed)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.array(out.stdout.split(), np.int32).reshape(n_sets, 6)
    state, want = seed, []
    for _ in range(n_sets):
        avail = list(range(N))
        for _ in range(6):
            state = (state * 1103515245 + 12345) & 0x7fffffff
            randi = state % len(avail)
            want.append(avail[randi])
            avail[randi] = avail[-1]; avail.pop()
    assert got.reshape(-1).tolist() == want and all(len(set(r)) == 6 for r in got.tolist())
    from eorb_slam_amd import frontend
    sets = frontend.mlpnp_draw_sets(7, 50, 1)
    assert sets.shape == (50, 6) and all(len(set(r)) == 6 for r in sets.tolist()) and sets.min() == 0 and sets.max() == 6


def _canon(a):
    a = np.array(a, np.float32)
    a[np.isnan(a)] = np.float32(np.nan)
    return a.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("wrong", [0.3, 1.0])
def test_mlpnp_mirror_equals_the_restatement(tmp_path, wrong):
    """30 % wrong: the first call stops at the first hypothesis with more than min_inliers inliers and every later call walks on from
    there to the next such hypothesis; all wrong: the first call runs all 35 iterations of SetRansacParameters, every later one five more, none returns a pose"""
    exe = _build(str(tmp_path))
    N, NK, calls = 65, 200, 4
    pb = scenes.scene(N, seed=81, cam="k", wrong=wrong, iters=320)
    ref = scenes.solver(mr, pb)
    min_inliers, iters = mr.ransac_parameters(N, 0.99, 10, 300, 6, 0.5)
    ref.min_inliers, ref.iters = min_inliers, iters
    assert (min_inliers, iters) == (32, 35)
    idx = np.sort(np.random.default_rng(82).permutation(NK)[:N]).astype(np.int32)
    put = lambda n, a, dt: np.ascontiguousarray(a, dt).tofile(str(tmp_path / (n + ".bin")))      # noqa: E731
    put("p2d", pb["p2d"], np.float32); put("Xw", pb["Xw"], np.float32); put("sigma2", pb["sigma2"], np.float32); put("sets", pb["sets"], np.int32)
    put("par", [10, 300, NK, calls], np.int32); put("indices", idx, np.int32)
    with open(str(tmp_path / "cam.bin"), "wb") as f:
        f.write(bytes(mr.camera(pb["cam"])))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "done" in out.stdout, out.stdout + out.stderr
    get = lambda n, dt: np.fromfile(str(tmp_path / (n + ".bin")), dt)      # noqa: E731
    log = get("log", np.int32).tolist()
    assert log[:2] == [min_inliers, iters]
    want = mr.iterate_calls(ref, pb["sets"], 5, calls)
    poses, flags = get("poses", np.float32), get("flags", np.uint8)
    p0 = f0 = 0
    for call, w in enumerate(want):
        no_more, n, iterations, tsize, fsize = log[2 + 5 * call:7 + 5 * call]
        assert (no_more, n, iterations) == (w["no_more"], w["n_inliers"], w["iterations"]), (call, log, w)
        if w["Tcw"] is None:
            assert tsize == 0 and fsize == 0                               # cv::Mat() and a cleared vbInliers
        else:
            assert tsize == 16 and fsize == NK
            assert _canon(poses[p0:p0 + 16]) == _canon(w["Tcw"].reshape(-1))
            f = np.zeros(NK, np.uint8); f[idx[w["inliers"] != 0]] = 1
            assert flags[f0:f0 + NK].tobytes() == f.tobytes()
        p0 += tsize; f0 += fsize
    if wrong == 1.0:
        assert [w["iterations"] for w in want] == [35, 40, 45, 50] and all(w["Tcw"] is None for w in want)
    else:
        assert want[0]["Tcw"] is not None and want[0]["no_more"] == 0 and want[0]["iterations"] < 35
