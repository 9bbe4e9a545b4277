// A plain g++ caller of ORB_SLAM3::MLPnPsolver (eorb_slam_amd/host/eorb_host.hpp), built and run by tests/test_host_mlpnp_cpp.py.  Without
// arguments it only proves that it linked; with `draw N nSets seed` it prints what DrawSets draws from a small generator; with a
// directory it reads the problem the test wrote there and calls iterate(5, ...) as Tracking::Relocalization does
// (src/Tracking.cc:2716-2729), again after every returned pose as if PoseOptimization had rejected it, and writes what every call
// returned.
#include "eorb_slam_amd/host/eorb_host.hpp"
#include <cstdio>
#include <cstdlib>
template <typename T> static std::vector<T> rd(const std::string& path) {
    std::vector<T> v; FILE* f = std::fopen(path.c_str(), "rb"); if (!f) return v;
    std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T)); if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear(); std::fclose(f); return v;
}
template <typename T> static void wr(const std::string& path, const std::vector<T>& v) { FILE* f = std::fopen(path.c_str(), "wb"); std::fwrite(v.data(), sizeof(T), v.size(), f); std::fclose(f); }
using ORB_SLAM3::MLPnPsolver;
int main(int argc, char** argv) {
    if (argc < 2) { std::puts("linked"); return 0; }          // link check only (no GPU touched)
    if (argc == 5 && std::string(argv[1]) == "draw") {       // draw N nSets seed: DrawSets on a small generator of the test's, printed (no GPU)
        const int N = std::atoi(argv[2]), nSets = std::atoi(argv[3]); uint32_t state = (uint32_t)std::atoi(argv[4]);
        eorb_camera cam{}; cam.fx = cam.fy = 1.f;
        MLPnPsolver solver(std::vector<float>(2 * (size_t)N), std::vector<float>(3 * (size_t)N), std::vector<float>((size_t)N, 1.f), cam);
        auto randomInt = [&state](int lo, int hi) { state = (state * 1103515245u + 12345u) & 0x7fffffffu; return lo + (int)(state % (uint32_t)(hi - lo + 1)); };
        solver.DrawSets(randomInt, nSets / 2);
        solver.DrawSets(randomInt, nSets);                     // sets already drawn stay; more are appended
        for (int32_t v : solver.sets()) std::printf("%d ", v);
        std::puts("");
        return 0;
    }
    const std::string dir = argv[1];
    try {
        const auto p2d = rd<float>(dir + "/p2d.bin"), Xw = rd<float>(dir + "/Xw.bin"), sg = rd<float>(dir + "/sigma2.bin");
        const auto cams = rd<eorb_camera>(dir + "/cam.bin"); const auto sets = rd<int32_t>(dir + "/sets.bin");
        const auto par = rd<int32_t>(dir + "/par.bin");        // minInliers, maxIterations, nKeyPoints, calls
        const auto idx = rd<int32_t>(dir + "/indices.bin");
        if (cams.size() != 1 || par.size() != 4 || Xw.empty()) { std::puts("no problem"); return 3; }
        MLPnPsolver solver(p2d, Xw, sg, cams[0], std::vector<int>(idx.begin(), idx.end()), par[2]);
        solver.SetRansacParameters(0.99, par[0], par[1], 6, 0.5f, 5.991f);
        solver.SetSets(sets);
        std::vector<int32_t> log; std::vector<float> poses; std::vector<uint8_t> flags;
        log.push_back(solver.GetMinInliers()); log.push_back(solver.GetMaxIterations());
        for (int call = 0; call < par[3]; call++) {
            bool bNoMore = false; std::vector<bool> vbInliers; int nInliers = 0;
            const MLPnPsolver::Mat Tcw = solver.iterate(5, bNoMore, vbInliers, nInliers);
            log.push_back(bNoMore); log.push_back(nInliers); log.push_back(solver.mnIterations); log.push_back((int)Tcw.size()); log.push_back((int)vbInliers.size());
            poses.insert(poses.end(), Tcw.begin(), Tcw.end());
            flags.insert(flags.end(), vbInliers.begin(), vbInliers.end());
        }
        wr(dir + "/log.bin", log); wr(dir + "/poses.bin", poses); wr(dir + "/flags.bin", flags);
    } catch (const eorb_host::Error& e) { std::printf("error %d: %s\n", e.code, e.what()); return 2; }
    std::puts("done");
    return 0;
}
