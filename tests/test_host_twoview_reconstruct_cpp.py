"""The C++ mirror of eorb_two_view_reconstruct (ORB_SLAM3::TwoViewReconstruction::Reconstruct in both overload shapes,
eorb_slam_amd/host/eorb_host.hpp) from a plain g++ caller (tests/host/twoview_reconstruct_check.cpp): it must compile and link against
libeorb_fe.so, and on a GPU box what it returns equals the restatement (tests/twoview_ref/reconstruct_ref.c) byte for byte, NaNs made
canonical, on scenes that leave at each stage."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from twoview_ref import scenes                                              # noqa: E402
from twoview_ref import reconstruct_ref as rr                               # noqa: E402
from twoview_ref import reconstruct_scenes as rs                            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp):
    from eorb_slam_amd import _lib
    lib = _lib.build()
    exe = os.path.join(tmp, "twoview_reconstruct_check")
    libdir = os.path.dirname(lib)
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, os.path.join(ROOT, "tests", "host", "twoview_reconstruct_check.cpp"), "-o", exe, "-L",
                        libdir, "-leorb_fe", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_reconstruct_mirror_compiles_and_links(tmp_path):
    exe = _build(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "linked" in out.stdout


def _canon(a):
    a = np.array(a)
    if a.dtype == np.float32:
        a[np.isnan(a)] = np.float32(np.nan)
    return a.tobytes()


def _result(path):
    r = rr.ReconResult.from_buffer_copy(open(path, "rb").read())
    return rr.result_dict(r)


@pytest.mark.gpu
def test_reconstruct_mirror_equals_the_restatement(tmp_path):
    exe = _build(str(tmp_path))
    assert C.sizeof(rr.ReconResult) == 240                 # sizeof(eorb_tvr_recon_result): the file the caller writes is read through it
    stages = set()
    for name in ("planar", "general", "far_similar", "pure_rotation", "same_keys"):
        build, N, iters, sets_seed, over, _ = rs.SCENES[name]
        assert not over
        sc = build()
        sets = scenes.make_sets(N, iters, seed=sets_seed)
        n1 = len(sc["kps1"])
        m12 = np.full(n1, -1, np.int32); m12[sc["matches"][:, 0]] = sc["matches"][:, 1]      # the reference's vMatches12
        assert (np.diff(sc["matches"][:, 0]) > 0).all()
        d = tmp_path / name
        d.mkdir()
        put = lambda n, a, dt: np.ascontiguousarray(a, dt).tofile(str(d / (n + ".bin")))      # noqa: E731
        put("kps1", sc["kps1"], scenes.KP_DTYPE); put("kps2", sc["kps2"], scenes.KP_DTYPE); put("matches12", m12, np.int32); put("sets", sets, np.int32)
        put("K", scenes.K, np.float32)
        out = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "done" in out.stdout, out.stdout + out.stderr
        get = lambda n, dt: np.fromfile(str(d / (n + ".bin")), dt)      # noqa: E731
        # the stock overload
        ref = rr.reconstruct(scenes.K, sc["kps1"], sc["kps2"], sc["matches"], sets, rr.params(rr.FORM_STOCK))
        res = _result(str(d / "stock_res.bin"))
        for k in rr.RESULT_FIELDS:
            assert _canon(res[k]) == _canon(ref[k]), (name, "stock", k)
        assert get("stock_ok", np.int32)[0] == ref["ok"]
        f = get("stock_f", np.float32)
        if ref["ok"]:
            assert _canon(f) == _canon(np.concatenate([ref["R21"][0].reshape(9), ref["t21"][0], ref["p3d"][0].reshape(-1)])), name
            assert get("stock_tri", np.uint8).tobytes() == ref["triangulated"][0].tobytes()
        else:
            assert not f.any() and len(f) == 12 and len(get("stock_tri", np.uint8)) == 0                # the arguments as they were
        # the ReconstInfo overload
        ref = rr.reconstruct(scenes.K, sc["kps1"], sc["kps2"], sc["matches"], sets, rr.params(rr.FORM_INFO))
        res = _result(str(d / "info_res.bin"))
        for k in rr.RESULT_FIELDS:
            assert _canon(res[k]) == _canon(ref[k]), (name, "info", k)
        stages.add((ref["stage"], bool(ref["is_homography"]), ref["ok"]))
        assert get("info_trans", np.uint8).tobytes() == ref["trans_inliers"].tobytes(), name
        iv, sv = get("info_i", np.int32), get("info_s", np.float32)
        assert iv[0] == ref["ok"]
        if ref["stage"] == 2:
            want = np.concatenate([np.concatenate([ref["R21"][s].reshape(9), ref["t21"][s], ref["p3d"][s].reshape(-1)]) for s in range(2)])
            assert _canon(get("info_f", np.float32)) == _canon(want), name
            assert get("info_tri", np.uint8).tobytes() == ref["triangulated"].tobytes()
            isH = bool(ref["is_homography"])
            assert iv[1:6].tolist() == [ref["best_good"], 0 if isH else ref["n_min_good"], ref["second_good"], 1 if isH else 0, 0 if isH else ref["n_similar"]]
            assert iv[6:].tolist() == ref["info_good"].tolist()
            assert _canon(sv) == _canon(np.array([ref["best_parallax"], ref["second_parallax"], ref["SH"], ref["SF"], ref["RH"]], np.float32))
        else:
            assert len(get("info_f", np.float32)) == 0 and iv[1:].tolist() == [0, 0, 0, 1, 0] + [0] * 8          # ReconstInfo's initial values
            assert sv[:2].tolist() == [-1.0, -1.0]
            assert _canon(sv[2:]) == _canon(np.array([ref["SH"], ref["SF"], ref["RH"]] if ref["stage"] == 1 else [0, 0, 0], np.float32))
    assert stages == {(2, True, 1), (2, False, 1), (2, False, 0), (1, True, 0), (0, False, 0)}
