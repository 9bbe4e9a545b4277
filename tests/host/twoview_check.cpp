// A plain g++ caller of ORB_SLAM3::TwoViewReconstruction (eorb_slam_amd/host/eorb_host.hpp), built and run by
// tests/test_host_twoview_cpp.py.  Without arguments it only proves that it linked; with a directory it reads the scene the test wrote
// there (keys, matches, sets, K, inlier flags, poses), runs FindHomographyFundamental and CheckRT and writes what they returned.
#include "eorb_slam_amd/host/eorb_host.hpp"
#include <cstdio>
template <typename T> static std::vector<T> rd(const std::string& path) {
    std::vector<T> v; FILE* f = std::fopen(path.c_str(), "rb"); if (!f) return v;
    std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T)); if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear(); std::fclose(f); return v;
}
template <typename T> static void wr(const std::string& path, const std::vector<T>& v) { FILE* f = std::fopen(path.c_str(), "wb"); std::fwrite(v.data(), sizeof(T), v.size(), f); std::fclose(f); }
using ORB_SLAM3::TwoViewReconstruction;
int main(int argc, char** argv) {
    if (argc < 2) { std::puts("linked"); return 0; }          // link check only (no GPU touched)
    const std::string dir = argv[1];
    try {
        const auto k1 = rd<eorb_keypoint>(dir + "/kps1.bin"), k2 = rd<eorb_keypoint>(dir + "/kps2.bin");
        const auto m = rd<int32_t>(dir + "/matches.bin"), sets = rd<int32_t>(dir + "/sets.bin");
        const auto K = rd<float>(dir + "/K.bin"), par = rd<float>(dir + "/par.bin");        // par: sigma, th2
        const auto inl = rd<uint8_t>(dir + "/inliers.bin"); const auto poses = rd<eorb_tvr_pose>(dir + "/poses.bin");
        if (K.size() != 9 || par.size() != 2 || m.empty() || poses.empty()) { std::puts("no scene"); return 3; }
        std::vector<TwoViewReconstruction::Match> vMatches12;
        for (size_t i = 0; i + 1 < m.size(); i += 2) vMatches12.emplace_back(m[i], m[i + 1]);
        TwoViewReconstruction tvr(K.data(), par[0], (int)(sets.size() / 8));
        const auto hf = tvr.FindHomographyFundamental(k1, k2, vMatches12, sets, true);
        std::vector<float> res = {hf.SH, hf.SF};
        res.insert(res.end(), hf.H21, hf.H21 + 9); res.insert(res.end(), hf.F21, hf.F21 + 9);
        wr(dir + "/res.bin", res); wr(dir + "/best.bin", std::vector<int32_t>{hf.best_it_h, hf.best_it_f});
        wr(dir + "/inl_h.bin", hf.vbMatchesInliersH); wr(dir + "/inl_f.bin", hf.vbMatchesInliersF);
        wr(dir + "/it_score_h.bin", hf.it_score_h); wr(dir + "/it_score_f.bin", hf.it_score_f); wr(dir + "/it_H.bin", hf.it_H); wr(dir + "/it_F.bin", hf.it_F);
        const auto rt = tvr.CheckRT(k1, k2, vMatches12, inl, poses, par[1], true);
        wr(dir + "/n_good.bin", rt.nGood); wr(dir + "/good.bin", rt.vbGood); wr(dir + "/p3d.bin", rt.vP3D); wr(dir + "/cos_sel.bin", rt.cosParallax);
        wr(dir + "/cos_all.bin", rt.cosAll);
        std::vector<double> par_deg;
        for (size_t h = 0; h < poses.size(); h++) par_deg.push_back(rt.parallax((int)h));
        wr(dir + "/parallax.bin", par_deg);
    } catch (const eorb_host::Error& e) { std::printf("error %d: %s\n", e.code, e.what()); return 2; }
    std::puts("done");
    return 0;
}
