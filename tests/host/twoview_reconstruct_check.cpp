// A plain g++ caller of ORB_SLAM3::TwoViewReconstruction::Reconstruct (eorb_slam_amd/host/eorb_host.hpp), built and run by
// tests/test_host_twoview_reconstruct_cpp.py.  Without arguments it only proves that it linked; with a directory it reads the scene the
// test wrote there (keys, the reference's vMatches12, sets, K), runs both overloads and writes what they returned.
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
        const auto m12 = rd<int32_t>(dir + "/matches12.bin"), sets = rd<int32_t>(dir + "/sets.bin");
        const auto K = rd<float>(dir + "/K.bin");
        if (K.size() != 9 || m12.size() != k1.size() || sets.empty()) { std::puts("no scene"); return 3; }
        const std::vector<int> vMatches12(m12.begin(), m12.end());
        TwoViewReconstruction tvr(K.data(), 1.0f, (int)(sets.size() / 8));
        // the stock overload
        TwoViewReconstruction::Mat33 R{}; TwoViewReconstruction::Vec3 t{};
        std::vector<TwoViewReconstruction::Vec3> P; std::vector<bool> tri;
        const bool ok = tvr.Reconstruct(k1, k2, vMatches12, sets, R, t, P, tri);
        std::vector<float> f(R.m, R.m + 9); f.insert(f.end(), t.v, t.v + 3);
        for (const auto& q : P) f.insert(f.end(), q.v, q.v + 3);
        wr(dir + "/stock_f.bin", f);
        std::vector<uint8_t> b(tri.begin(), tri.end());
        wr(dir + "/stock_tri.bin", b);
        wr(dir + "/stock_res.bin", std::vector<eorb_tvr_recon_result>{tvr.last});
        wr(dir + "/stock_ok.bin", std::vector<int32_t>{ok ? 1 : 0});
        // the ReconstInfo overload
        std::vector<TwoViewReconstruction::Mat33> vR; std::vector<TwoViewReconstruction::Vec3> vt;
        std::vector<std::vector<TwoViewReconstruction::Vec3>> vP; std::vector<std::vector<bool>> vtri; std::vector<bool> trans;
        TwoViewReconstruction::ReconstInfo info;
        const bool ok2 = tvr.Reconstruct(k1, k2, vMatches12, sets, vR, vt, vP, vtri, trans, info);
        f.clear(); b.clear();
        for (size_t s = 0; s < vR.size(); s++) {
            f.insert(f.end(), vR[s].m, vR[s].m + 9); f.insert(f.end(), vt[s].v, vt[s].v + 3);
            for (const auto& q : vP[s]) f.insert(f.end(), q.v, q.v + 3);
            b.insert(b.end(), vtri[s].begin(), vtri[s].end());
        }
        wr(dir + "/info_f.bin", f); wr(dir + "/info_tri.bin", b);
        wr(dir + "/info_trans.bin", std::vector<uint8_t>(trans.begin(), trans.end()));
        wr(dir + "/info_res.bin", std::vector<eorb_tvr_recon_result>{tvr.last});
        std::vector<int32_t> iv = {ok2 ? 1 : 0, info.mnBestGood, info.mnMinGood, info.mnSecondBest, info.isHomography ? 1 : 0, (int32_t)info.mnSimilar};
        iv.insert(iv.end(), info.mvnGood.begin(), info.mvnGood.end());
        wr(dir + "/info_i.bin", iv);
        wr(dir + "/info_s.bin", std::vector<float>{info.mBestParallax, info.mSecondBestPar, info.mHScore, info.mFScore, info.mHFRatio});
    } catch (const eorb_host::Error& e) { std::printf("error %d: %s\n", e.code, e.what()); return 2; }
    std::puts("done");
    return 0;
}
