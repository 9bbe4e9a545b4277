// A plain g++ caller of ORB_SLAM3::CreateNewMapPoints (eorb_slam_amd/host/eorb_host.hpp), built and run by tests/test_host_newpts_cpp.py.
// Without arguments it only proves that it linked; with a directory it reads the scene the test wrote there (one file per array; an
// optional array that is not there is NULL), calls the stage once and writes what it returned.
#include "eorb_slam_amd/host/eorb_host.hpp"
#include <cstdio>
template <typename T> static std::vector<T> rd(const std::string& path) {
    std::vector<T> v; FILE* f = std::fopen(path.c_str(), "rb"); if (!f) return v;
    std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T)); if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear(); std::fclose(f); return v;
}
template <typename T> static void wr(const std::string& path, const std::vector<T>& v) { FILE* f = std::fopen(path.c_str(), "wb"); std::fwrite(v.data(), sizeof(T), v.size(), f); std::fclose(f); }
template <typename T> static const T* opt(const std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }
struct Side {
    std::vector<float> sigma2, scale, uright, depth, raw; std::vector<uint8_t> isOrb;
    explicit Side(const std::string& pre) : sigma2(rd<float>(pre + "kp_sigma2.bin")), scale(rd<float>(pre + "kp_scale.bin")), uright(rd<float>(pre + "uright.bin")),
                                            depth(rd<float>(pre + "depth.bin")), raw(rd<float>(pre + "raw_xy.bin")), isOrb(rd<uint8_t>(pre + "kp_is_orb.bin")) {}
    eorb_newpts_side get() const { return eorb_newpts_side{opt(sigma2), opt(scale), opt(isOrb), opt(uright), opt(depth), opt(raw)}; }
};
int main(int argc, char** argv) {
    if (argc < 2) { std::puts("linked"); return 0; }          // link check only (no GPU touched)
    const std::string dir = argv[1];
    try {
        const auto kps1 = rd<eorb_keypoint>(dir + "/kps1.bin"), kps2 = rd<eorb_keypoint>(dir + "/kps2.bin");
        const auto kfOff = rd<int32_t>(dir + "/kf_off.bin"), m12 = rd<int32_t>(dir + "/match12.bin"), nleft2 = rd<int32_t>(dir + "/nleft2.bin");
        auto views1 = rd<eorb_view>(dir + "/views1.bin"), views2 = rd<eorb_view>(dir + "/views2.bin");
        const auto pari = rd<int32_t>(dir + "/par_i.bin");      // form, nleft1, far_points
        const auto parf = rd<float>(dir + "/par_f.bin");        // mb1, ratio_factor_orb, ratio_factor_ak, th_far_points
        const auto mb2 = rd<float>(dir + "/mb2.bin"), ls = rd<float>(dir + "/level_scale.bin"), lg = rd<float>(dir + "/level_sigma2.bin");
        if (pari.size() != 3 || parf.size() != 4 || views1.empty() || kfOff.empty()) { std::puts("no scene"); return 3; }
        const Side s1(dir + "/side1_"), s2(dir + "/side2_");
        eorb_newpts_params P{};
        P.form = pari[0]; P.views1 = views1.data(); P.nleft1 = pari[1]; P.mb1 = parf[0];
        P.views2 = views2.data(); P.nleft2 = opt(nleft2); P.mb2 = opt(mb2);
        P.side1 = s1.get(); P.side2 = s2.get();
        P.level_scale = opt(ls); P.level_sigma2 = opt(lg); P.nlevels = (int)ls.size();
        P.ratio_factor_orb = parf[1]; P.ratio_factor_ak = parf[2]; P.far_points = pari[2]; P.th_far_points = parf[3];
        const ORB_SLAM3::NewMapPoints r = ORB_SLAM3::CreateNewMapPoints(kps1, kps2, kfOff, m12, P);
        wr(dir + "/status.bin", r.status); wr(dir + "/x3d.bin", r.x3D); wr(dir + "/branch.bin", r.branch); wr(dir + "/cos_parallax.bin", r.cosParallax);
        wr(dir + "/n_new.bin", r.nNew);
    } catch (const eorb_host::Error& e) { std::printf("error %d: %s\n", e.code, e.what()); return 2; }
    std::puts("done");
    return 0;
}
