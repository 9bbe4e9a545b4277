// A plain g++ caller of the keyframe-list overloads of ORB_SLAM3::ORBmatcher (SearchForTriangulation / SearchByBoW over a vector of
// keyframes, eorb_slam_amd/host/eorb_host.hpp), built and run by tests/test_host_kfbatch_cpp.py.  Without arguments it only proves that it
// linked; with a directory it reads the neighbourhood the test wrote there (one current keyframe "c" and K keyframes "k0", "k1", ...),
// runs the four overloads and writes the K rows each returned.
#include "eorb_slam_amd/host/eorb_host.hpp"
#include <cstdio>
#include <memory>
template <typename T> static std::vector<T> rd(const std::string& path) {
    std::vector<T> v; FILE* f = std::fopen(path.c_str(), "rb"); if (!f) return v;
    std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T)); if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear(); std::fclose(f); return v;
}
template <typename T> static void wr(const std::string& path, const std::vector<T>& v) { FILE* f = std::fopen(path.c_str(), "wb"); std::fwrite(v.data(), sizeof(T), v.size(), f); std::fclose(f); }
using ORB_SLAM3::ORBmatcher;
struct Kf {                        // one keyframe as the test wrote it: <name>_kps / _desc / _flag / _nodes / _off / _idx .bin
    std::vector<eorb_host::KeyPoint> kps; eorb_host::Mat8 desc; std::vector<uint8_t> flag; ORBmatcher::FeatureVector fv;
    std::unique_ptr<ORB_SLAM3::FrameView> view;
    Kf(const std::string& base, int stride) {
        kps = rd<eorb_host::KeyPoint>(base + "_kps.bin");
        auto d = rd<uint8_t>(base + "_desc.bin");
        desc = eorb_host::Mat8((int)kps.size(), stride); std::memcpy(desc.ptr(), d.data(), d.size());
        flag = rd<uint8_t>(base + "_flag.bin");
        fv.nodes = rd<uint32_t>(base + "_nodes.bin"); fv.off = rd<int32_t>(base + "_off.bin"); fv.idx = rd<int32_t>(base + "_idx.bin");
        view.reset(new ORB_SLAM3::FrameView(kps, desc, 346, 260));
    }
};
static std::vector<int> rows(const std::vector<std::vector<std::pair<size_t, size_t>>>& vv, size_t n1) {
    std::vector<int> m(vv.size() * n1, -1);
    for (size_t k = 0; k < vv.size(); k++) for (const auto& p : vv[k]) m[k * n1 + p.first] = (int)p.second;
    return m;
}
static std::vector<int> flat(const std::vector<std::vector<int>>& vv) { std::vector<int> m; for (const auto& v : vv) m.insert(m.end(), v.begin(), v.end()); return m; }
int main(int argc, char** argv) {
    if (argc < 2) { std::puts("linked"); return 0; }          // link check only (no GPU touched)
    const std::string dir = argv[1];
    try {
        for (const std::string scene : {"tri", "kb8", "bow"}) {
            const auto hdr = rd<int32_t>(dir + "/" + scene + "_hdr.bin");        // K, stride
            if (hdr.size() < 2) { std::printf("no %s scene\n", scene.c_str()); return 3; }
            const int K = hdr[0];
            Kf cur(dir + "/" + scene + "_c", hdr[1]);
            std::vector<std::unique_ptr<Kf>> kfs;
            std::vector<ORBmatcher::KeyFrameNodes> list;
            for (int k = 0; k < K; k++) {
                kfs.emplace_back(new Kf(dir + "/" + scene + "_k" + std::to_string(k), hdr[1]));
                list.push_back({kfs.back()->view.get(), &kfs.back()->flag, &kfs.back()->fv});
            }
            const size_t n1 = cur.kps.size();
            if (scene == "bow") {
                ORBmatcher reloc(0.7f, true), loop(0.8f, true);
                std::vector<std::vector<int>> vv;
                wr(dir + "/bow_nm.bin", reloc.SearchByBoW(list, *cur.view, cur.fv, vv)); wr(dir + "/bow_rows.bin", flat(vv));
                wr(dir + "/bowkf_nm.bin", loop.SearchByBoW(*cur.view, cur.flag, cur.fv, list, vv)); wr(dir + "/bowkf_rows.bin", flat(vv));
                continue;
            }
            const auto ep = rd<float>(dir + "/" + scene + "_ep.bin"), scale = rd<float>(dir + "/" + scene + "_scale.bin"),
                       sigma2 = rd<float>(dir + "/" + scene + "_sigma2.bin");
            ORBmatcher matcher(0.6f, false);                    // (LocalMapping.cc:443: no rotation check)
            std::vector<std::vector<std::pair<size_t, size_t>>> vvPairs;
            if (scene == "tri") {
                wr(dir + "/tri_nm.bin", matcher.SearchForTriangulation(*cur.view, cur.flag, cur.fv, list, ep, rd<float>(dir + "/tri_F12.bin"), scale, sigma2, vvPairs));
                wr(dir + "/tri_rows.bin", rows(vvPairs, n1));
            } else {
                const auto cam = rd<float>(dir + "/kb8_cam.bin");        // fx fy cx cy k1..k4
                eorb_camera c{}; c.model = 1; c.fx = cam[0]; c.fy = cam[1]; c.cx = cam[2]; c.cy = cam[3];
                for (int i = 0; i < 4; i++) c.k[i] = cam[4 + i];
                c.precision = 1e-6f;
                const eorb_camera cams[2] = {c, c};
                wr(dir + "/kb8_nm.bin", matcher.SearchForTriangulation(*cur.view, -1, cur.flag, cur.fv, list, std::vector<int>(K, -1), cams, cams,
                                                                       rd<float>(dir + "/kb8_Rt.bin"), ep, scale, sigma2, sigma2, vvPairs));
                wr(dir + "/kb8_rows.bin", rows(vvPairs, n1));
            }
        }
        std::puts("done");
        return 0;
    } catch (const eorb_host::Error& e) { std::printf("error %d: %s\n", e.code, e.what()); return 2; }
}
