"""The C++ MyCalibrator mirror (eorb_slam_amd/host/eorb_host.hpp) from a plain g++ caller: it must compile and link against
libeorb_fe.so, and on a GPU box its undistorted keypoints, points, maps and the monocular frame's outputs equal the CPU restatement
(tests/calib_ref/calib_ref.c) bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calib_ref                                    # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "eorb_slam_amd/host/eorb_host.hpp"
#include <cstdio>
#include <thread>
template <typename T> static std::vector<T> rd(const std::string& path) {
    std::vector<T> v; FILE* f = std::fopen(path.c_str(), "rb"); if (!f) return v;
    std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T)); if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear(); std::fclose(f); return v;
}
template <typename T> static void wr(const std::string& path, const T* p, size_t n) { FILE* f = std::fopen(path.c_str(), "wb"); std::fwrite(p, sizeof(T), n, f); std::fclose(f); }
int main(int argc, char** argv) {
    if (argc < 2) { std::puts("linked"); return 0; }          // link check only (no GPU touched)
    const std::string dir = argv[1];
    try {
        // calib.bin: model, W, H, nK = 9, nd, nR, nP as floats, then the values
        auto c = rd<float>(dir + "/calib.bin");
        const int model = (int)c[0], W = (int)c[1], H = (int)c[2], nd = (int)c[4], nR = (int)c[5], nP = (int)c[6];
        const float* K = &c[7];
        std::vector<float> dist(c.begin() + 16, c.begin() + 16 + nd), R(c.begin() + 16 + nd, c.begin() + 16 + nd + nR),
                           P(c.begin() + 16 + nd + nR, c.begin() + 16 + nd + nR + nP);
        EORB_SLAM::MyCalibrator cal(K, dist, W, H, R, P, model == 1);
        auto kps = rd<eorb_host::KeyPoint>(dir + "/kps.bin");
        std::vector<eorb_host::KeyPoint> un, none, untouched(3);
        cal.undistKeyPoints(kps, un);
        cal.undistKeyPoints(none, untouched);                   // empty in: the output is left alone
        wr(dir + "/un.bin", un.data(), un.size());
        std::vector<float> xy(2 * kps.size());
        for (size_t i = 0; i < kps.size(); i++) { xy[2 * i] = kps[i].x; xy[2 * i + 1] = kps[i].y; }
        auto uxy = cal.undistPoints(xy);
        float ux, uy; cal.undistPoint(xy[0], xy[1], ux, uy);
        uxy.push_back(ux); uxy.push_back(uy);
        wr(dir + "/uxy.bin", uxy.data(), uxy.size());
        cal.generateUndistMaps(true);
        wr(dir + "/mapx.bin", cal.mUndistMapX.data(), cal.mUndistMapX.size());
        wr(dir + "/mapy.bin", cal.mUndistMapY.data(), cal.mUndistMapY.size());
        // a thread started afterwards borrows a context that loads the calibration and the maps from the pool
        std::vector<eorb_host::KeyPoint> un2; size_t nrect = 0;
        std::thread th([&] {
            cal.undistKeyPoints(kps, un2);
            std::vector<eorb_raw_event> raw(1000);
            for (int i = 0; i < 1000; i++) { raw[i].x = (uint16_t)((i * 53) % W); raw[i].y = (uint16_t)((i * 29) % H); raw[i].p = i & 1; raw[i].t = 1e-6 * i; }
            nrect = EORB_SLAM::EventDataStore::rectify(raw, W, H, 1.0).size();
        });
        th.join();
        const bool same = un2.size() == un.size() && std::memcmp(un2.data(), un.data(), un.size() * sizeof(eorb_host::KeyPoint)) == 0;
        // the monocular frame
        auto img = rd<uint8_t>(dir + "/img.bin");
        eorb_host::Mat8 im(H, W); std::memcpy(im.ptr(), img.data(), img.size());
        ORB_SLAM3::ORBxParams p; p.nfeatures = 1000; p.scaleFactor = 1.2f; p.nlevels = 4; p.iniThFAST = 20; p.minThFAST = 7; p.edgeTh = 19; p.imWidth = W; p.imHeight = H;
        ORB_SLAM3::ORBextractor ex(p);
        std::vector<eorb_host::KeyPoint> k0, k1, k1un; eorb_host::Mat8 d0, d1; float b[4];
        const int m0 = ex(im, k0, d0, std::vector<int>{0, 1000});
        const int m1 = ex.ExtractMono(im, std::vector<int>{0, 1000}, cal.calibration(), k1, k1un, d1, b);
        const bool ext = m0 == m1 && k0.size() == k1.size() && !k0.empty() && std::memcmp(k0.data(), k1.data(), k0.size() * sizeof(eorb_host::KeyPoint)) == 0 &&
                         std::memcmp(d0.ptr(), d1.ptr(), k0.size() * 32) == 0;
        wr(dir + "/fk.bin", k1.data(), k1.size()); wr(dir + "/fkun.bin", k1un.data(), k1un.size()); wr(dir + "/fb.bin", b, 4);
        std::printf("kps=%zu same=%d untouched=%zu rect=%zu ext=%d frame=%zu\n", un.size(), (int)same, untouched.size(), nrect, (int)ext, k1.size());
        return (same && untouched.size() == 3 && nrect > 0 && ext) ? 0 : 1;
    } catch (const eorb_host::Error& e) { std::printf("error %d: %s\n", e.code, e.what()); return 2; }
}
'''


def _build(tmp):
    from eorb_slam_amd import _lib
    lib = _lib.build()
    src = os.path.join(tmp, "calib_check.cpp"); exe = os.path.join(tmp, "calib_check")
    open(src, "w").write(SRC)
    libdir = os.path.dirname(lib)
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, src, "-o", exe, "-L", libdir, "-leorb_fe",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_calibrator_mirror_compiles_and_links(tmp_path):
    exe = _build(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "linked" in out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["EvETHZ", "fisheye_RP", "pinhole_RP"])
def test_calibrator_mirror_equals_the_restatement(tmp_path, name):
    exe = _build(str(tmp_path))
    d = synth.CALIBRATIONS[name]
    W, H = 240, 180
    R = np.zeros(0, np.float32) if d["R"] is None else d["R"].ravel()
    P = np.zeros(0, np.float32) if d["P"] is None else d["P"].ravel()
    head = np.array([d["model"], W, H, 9, len(d["dist"]), len(R), len(P)], np.float32)
    np.concatenate([head, d["K"].ravel(), d["dist"], R, P]).astype(np.float32).tofile(str(tmp_path / "calib.bin"))
    kps = synth.calib_keypoints(3000, W, H, seed=17)
    kps.tofile(str(tmp_path / "kps.bin"))
    img = synth.texture_image(W, H, seed=3)
    img.tofile(str(tmp_path / "img.bin"))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    want = calib_ref.undistort_keypoints(d, kps)
    assert np.fromfile(str(tmp_path / "un.bin"), synth.KP_DTYPE).tobytes() == want.tobytes()
    uxy = np.fromfile(str(tmp_path / "uxy.bin"), np.float32).reshape(-1, 2)
    wxy = calib_ref.undistort_points(d, np.stack([kps["x"], kps["y"]], axis=1))
    assert uxy[:-1].tobytes() == wxy.tobytes() and uxy[-1].tobytes() == wxy[0].tobytes()
    rx, ry = calib_ref.generate_maps(d, W, H)
    assert np.fromfile(str(tmp_path / "mapx.bin"), np.float32).tobytes() == rx.tobytes()
    assert np.fromfile(str(tmp_path / "mapy.bin"), np.float32).tobytes() == ry.tobytes()
    fk = np.fromfile(str(tmp_path / "fk.bin"), synth.KP_DTYPE)
    assert len(fk) > 100
    assert np.fromfile(str(tmp_path / "fkun.bin"), synth.KP_DTYPE).tobytes() == calib_ref.undistort_keypoints(d, fk).tobytes()
    assert np.fromfile(str(tmp_path / "fb.bin"), np.float32).tobytes() == calib_ref.image_bounds(d, W, H).tobytes()
