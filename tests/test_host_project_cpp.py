"""The C++ mirror of Frame::isInFrustum and Tracking::SearchLocalPoints (eorb_slam_amd/host/eorb_host.hpp) from a plain g++ caller:
it must compile and link against libeorb_fe.so, and on a GPU box its outputs equal the CPU restatement (tests/proj_ref/proj_ref.c)
followed by the oracle's matcher, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proj_ref                                     # noqa: E402
from eorb_slam_amd import synth                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 346, 260

SRC = r'''
#include "eorb_slam_amd/host/eorb_host.hpp"
#include <cstdio>
template <typename T> static std::vector<T> rd(const std::string& path) {
    std::vector<T> v; FILE* f = std::fopen(path.c_str(), "rb"); if (!f) return v;
    std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T)); if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear(); std::fclose(f); return v;
}
template <typename T> static void wr(const std::string& path, const std::vector<T>& v) { FILE* f = std::fopen(path.c_str(), "wb"); std::fwrite(v.data(), sizeof(T), v.size(), f); std::fclose(f); }
static void dump(const std::string& dir, const std::string& tag, const ORB_SLAM3::TrackedPoints& t) {
    wr(dir + "/" + tag + "_in_view.bin", t.inView); wr(dir + "/" + tag + "_proj_xy.bin", t.projXY); wr(dir + "/" + tag + "_proj_xr.bin", t.projXR);
    wr(dir + "/" + tag + "_level.bin", t.level); wr(dir + "/" + tag + "_view_cos.bin", t.viewCos); wr(dir + "/" + tag + "_depth.bin", t.depth);
    wr(dir + "/" + tag + "_level_scale.bin", t.levelScale); wr(dir + "/" + tag + "_reason.bin", t.reason);
}
int main(int argc, char** argv) {
    if (argc < 2) { std::puts("linked"); return 0; }          // link check only (no GPU touched)
    const std::string dir = argv[1];
    try {
        // pose.bin: R[9] t[3] Ow[3] fx fy cx cy mbf logScale thFar th, then the scale factors
        auto p = rd<float>(dir + "/pose.bin");
        eorb_camera cam{}; cam.model = 0; cam.fx = p[15]; cam.fy = p[16]; cam.cx = p[17]; cam.cy = p[18];
        auto kps = rd<eorb_host::KeyPoint>(dir + "/kps.bin");
        auto dsc = rd<uint8_t>(dir + "/desc.bin");
        eorb_host::Mat8 desc((int)kps.size(), 32); std::memcpy(desc.ptr(), dsc.data(), dsc.size());
        ORB_SLAM3::FrameView F(kps, desc, 346, 260);
        ORB_SLAM3::FramePose pose(&p[0], &p[9], &p[12], cam, F.gb, p[19], std::vector<float>(p.begin() + 23, p.end()), p[20]);
        ORB_SLAM3::MapPointsView mps;
        mps.worldPos = rd<float>(dir + "/pos.bin"); mps.normal = rd<float>(dir + "/normal.bin");
        mps.minDistance = rd<float>(dir + "/min_dist.bin"); mps.maxDistance = rd<float>(dir + "/max_dist.bin");
        mps.skip = rd<uint8_t>(dir + "/skip.bin"); mps.observed = rd<uint8_t>(dir + "/obs.bin");
        auto md = rd<uint8_t>(dir + "/mp_desc.bin");
        mps.descriptors = eorb_host::Mat8(mps.size(), 32); std::memcpy(mps.descriptors.ptr(), md.data(), md.size());
        ORB_SLAM3::TrackedPoints a, b;
        const int nA = ORB_SLAM3::isInFrustum(pose, mps, 0.5f, a);
        dump(dir, "a", a);
        auto frameMP = rd<int>(dir + "/fm.bin");
        ORB_SLAM3::ORBmatcher matcher(0.8f, true);
        int nToMatch = -1;
        const int nm = matcher.SearchLocalPoints(F, pose, mps, frameMP, p[22], true, p[21], b, &nToMatch);
        dump(dir, "b", b);
        wr(dir + "/fm_out.bin", frameMP);
        std::printf("M=%d in_view=%d to_match=%d matches=%d\n", mps.size(), nA, nToMatch, nm);
        wr(dir + "/counts.bin", std::vector<int>{nA, nToMatch, nm});
        return 0;
    } catch (const eorb_host::Error& e) { std::printf("error %d: %s\n", e.code, e.what()); return 2; }
}
'''


def _build(tmp):
    from eorb_slam_amd import _lib
    lib = _lib.build()
    src = os.path.join(tmp, "project_check.cpp"); exe = os.path.join(tmp, "project_check")
    open(src, "w").write(SRC)
    libdir = os.path.dirname(lib)
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-I", ROOT, src, "-o", exe, "-L", libdir, "-leorb_fe",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe


def test_projector_mirror_compiles_and_links(tmp_path):
    exe = _build(str(tmp_path))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "linked" in out.stdout


@pytest.mark.gpu
def test_projector_mirror_equals_the_restatement(tmp_path, oracle):
    exe = _build(str(tmp_path))
    M, n, th, mbf = 1500, 1000, 1.0, 35.0
    s = synth.map_scene(41, M)
    v = proj_ref.view(s["R"], s["t"], s["Ow"], s["cam"], s["bounds"], s["nlevels"], s["log_scale"], s["scale_factors"], mbf=mbf)
    args = (s["pos"], s["normal"], s["min_dist"], s["max_dist"])
    skip = (np.arange(M) % 11 == 10).astype(np.uint8)
    _, (r0,) = proj_ref.frustum(v, *args, cos_limit=0.5, skip=skip)
    th_far = float(np.float32(np.median(r0["depth"][r0["in_view"] == 1])))
    wn, (r,) = proj_ref.frustum(v, *args, cos_limit=0.5, skip=skip, far=True, th_far=th_far)
    mp_desc = synth.random_descriptors(M, seed=42)
    kps, desc, _ = synth.planted_frame(r["in_view"], r["proj_xy"], r["level"], mp_desc, n, W, H, seed=43)
    obs = (np.random.default_rng(44).random(M) < 0.9).astype(np.uint8)
    fm = np.full(n, -1, np.int32); fm[::29] = -2; fm[7::31] = -3
    on, ofm = oracle.search_by_projection_map(oracle.Frame(kps, desc, W, H), r["search"], r["proj_xy"], r["level"], r["view_cos"], mp_desc, obs,
                                              fm, th, 0.8, r["level_scale"])
    assert on >= 40 and wn >= 150 and int(r["search"].sum()) < wn

    def put(name, a):
        np.ascontiguousarray(a).tofile(str(tmp_path / (name + ".bin")))
    put("pose", np.concatenate([s["R"].ravel(), s["t"], s["Ow"], np.array(s["cam"], np.float32),
                                np.array([mbf, s["log_scale"], th_far, th], np.float32), s["scale_factors"]]).astype(np.float32))
    for name, a in (("kps", kps), ("desc", desc), ("pos", s["pos"]), ("normal", s["normal"]), ("min_dist", s["min_dist"]),
                    ("max_dist", s["max_dist"]), ("skip", skip), ("obs", obs), ("mp_desc", mp_desc), ("fm", fm)):
        put(name, a)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    for tag in ("a", "b"):
        for name, dt, _ in proj_ref.FRUSTUM_FIELDS:
            got = np.fromfile(str(tmp_path / ("%s_%s.bin" % (tag, name))), dt)
            assert got.tobytes() == r[name].tobytes(), (tag, name)
    assert np.fromfile(str(tmp_path / "counts.bin"), np.int32).tolist() == [wn, wn, on]
    assert np.array_equal(np.fromfile(str(tmp_path / "fm_out.bin"), np.int32), ofm)
