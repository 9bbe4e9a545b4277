"""The C++ mirror of the Sim3 solver (ORB_SLAM3::Sim3Solver, eorb_slam_amd/host/eorb_host.hpp) from a plain g++ caller
(tests/host/sim3_check.cpp): it must compile and link against libeorb_fe.so, and on a GPU box what the loop of LoopClosing.cc:698-701 and
find() return equals the restatement (tests/sim3_ref) byte for byte, NaNs made canonical."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_ref as s3                               # noqa: E402
from sim3_ref import scenes                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp):
    from eorb_slam_amd import _lib
    lib = _lib.build()
    exe = os.path.join(tmp, "sim3_check")
    libdir = os.path.dirname(lib)
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "host", "sim3_check.cpp"), "-o", exe, "-L", libdir,
                        "-leorb_fe", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_sim3_mirror_compiles_and_links(tmp_path):
    exe = _build(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "linked" in out.stdout


def _canon(a):
    a = np.array(a)
    if a.dtype == np.float32:
        a[np.isnan(a)] = np.float32(np.nan)
    return a.tobytes()


def _replay(o, min_inliers, chunk=20):
    """the loop "while(!bConverge && !bNoMore) iterate(20, ...)" over the restatement's per-iteration aids: what the last call returns"""
    best, done, iters = 0, 0, len(o["it_inliers"])
    while True:
        best_sim3 = None
        for it in range(done, min(done + chunk, iters)):
            done = it + 1
            n = int(o["it_inliers"][it])
            if n >= best:
                best = n
                if n > min_inliers:
                    return dict(converge=1, no_more=0, n=n, iterations=done, T12=o["it_T12"][it])
                best_sim3 = o["it_T12"][it]
        if done >= iters:
            return dict(converge=0, no_more=1, n=0, iterations=done, T12=best_sim3)


@pytest.mark.gpu
@pytest.mark.parametrize("wrong,min_inliers", [(0.3, 20), (0.7, 10), (1.0, 6)])
def test_sim3_mirror_equals_the_restatement(tmp_path, wrong, min_inliers):
    """30 % wrong: converges in the first chunk of 20 (156 iterations by the formula); 70 %: in the second chunk, at iteration 39; all
    wrong: never, 15 chunks"""
    exe = _build(str(tmp_path))
    N, N1 = 65, 200
    iters = s3.ransac_iterations(N, 0.99, min_inliers, 300)
    assert iters == (156 if min_inliers == 20 else 300)
    pb = scenes.scene(N, seed=71, pair="pk", wrong=wrong, iters=iters, min_inliers=min_inliers)
    idx = np.sort(np.random.default_rng(72).permutation(N1)[:N]).astype(np.int32)
    put = lambda n, a, dt: np.ascontiguousarray(a, dt).tofile(str(tmp_path / (n + ".bin")))      # noqa: E731
    put("Xw1", pb["Xw1"], np.float32); put("Xw2", pb["Xw2"], np.float32); put("Rt", np.concatenate([pb["Rt1"], pb["Rt2"]]), np.float32)
    put("sigma2_1", pb["sigma2_1"], np.float32); put("sigma2_2", pb["sigma2_2"], np.float32); put("sets", pb["sets"], np.int32)
    put("par", [int(pb["fix_scale"]), min_inliers, 300, N1], np.int32); put("indices1", idx, np.int32)
    cams = (s3.Camera * 2)(s3.camera(pb["cam1"]), s3.camera(pb["cam2"]))
    with open(str(tmp_path / "cams.bin"), "wb") as f:
        f.write(bytes(cams))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "done" in out.stdout, out.stdout + out.stderr
    get = lambda n, dt: np.fromfile(str(tmp_path / (n + ".bin")), dt)      # noqa: E731
    r = scenes.find(s3, pb, aids=True)
    want = _replay(r, min_inliers)
    assert r["converged"] == want["converge"] == (1 if wrong < 1.0 else 0)
    conv, no_more, n, iterations, chunks, tsize = get("loop", np.int32).tolist()
    assert (conv, no_more, n, iterations) == (want["converge"], want["no_more"], want["n"], want["iterations"])
    assert iterations == r["iterations_used"] and chunks == -(-iterations // 20)
    assert chunks == {0.3: 1, 0.7: 2, 1.0: 15}[wrong]
    assert get("it_inliers", np.int32).tobytes() == r["it_inliers"].tobytes()
    if want["T12"] is None:
        assert tsize == 0                                                 # the last chunk improved nothing: an empty matrix, as cv::Mat()
    else:
        assert _canon(get("loop_T12", np.float32)) == _canon(want["T12"].reshape(-1))
    flags = np.zeros(N1, np.uint8)
    if conv:
        flags[idx[r["inliers"] != 0]] = 1
        assert _canon(get("loop_T12", np.float32)) == _canon(r["T12"].reshape(-1))
    assert get("loop_inliers", np.uint8).tobytes() == flags.tobytes()
    assert _canon(get("loop_est", np.float32)) == _canon(np.concatenate([r["R12"].reshape(9), r["t12"], [r["s12"]]]).astype(np.float32))
    # find(): the four-argument iterate over all iterations, a matrix only on convergence
    n12, its = get("find", np.int32).tolist()
    assert (n12, its) == ((r["n_inliers"], r["iterations_used"]) if conv else (0, iters))
    assert _canon(get("find_T12", np.float32)) == (_canon(r["T12"].reshape(-1)) if conv else b"")
    assert get("find_inliers", np.uint8).tobytes() == flags.tobytes()
