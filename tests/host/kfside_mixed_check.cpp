// A plain g++ caller of the MixedMatcher forms of the KeyFrame-side methods of ORB_SLAM3::ORBmatcher (eorb_slam_amd/host/eorb_host.hpp),
// built and run by tests/test_host_kfside_mixed_cpp.py.  Without arguments it only proves that it linked; with a directory it reads
// the mixed scene the test wrote there, runs ProjectKeyFrameSideMixed, KeyFrameRadiusMatchMixed, FuseMixed, SearchByProjectionMixed
// and FuseKeyFramesMixed, and writes what they returned.
#include "eorb_slam_amd/host/eorb_host.hpp"
#include <cstdio>
template <typename T> static std::vector<T> rd(const std::string& path) {
    std::vector<T> v; FILE* f = std::fopen(path.c_str(), "rb"); if (!f) return v;
    std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T)); if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear(); std::fclose(f); return v;
}
template <typename T> static void wr(const std::string& path, const std::vector<T>& v) { FILE* f = std::fopen(path.c_str(), "wb"); std::fwrite(v.data(), sizeof(T), v.size(), f); std::fclose(f); }
int main(int argc, char** argv) {
    if (argc < 2) { std::puts("linked"); return 0; }          // link check only (no GPU touched)
    const std::string dir = argv[1];
    try {
        // pose.bin: R[9] t[3] Ow[3] fx fy cx cy mbf logScale akLogScale th; sf.bin / ak_sf.bin: the two pyramids' scale factors
        auto p = rd<float>(dir + "/pose.bin");
        const auto sf = rd<float>(dir + "/sf.bin"), akSf = rd<float>(dir + "/ak_sf.bin");
        eorb_view view{};
        std::memcpy(view.R, &p[0], 36); std::memcpy(view.t, &p[9], 12); std::memcpy(view.Ow, &p[12], 12);
        view.cam.model = 0; view.cam.fx = p[15]; view.cam.fy = p[16]; view.cam.cx = p[17]; view.cam.cy = p[18];
        view.minX = 0.f; view.maxX = 346.f; view.minY = 0.f; view.maxY = 260.f; view.mbf = p[19];
        view.nlevels = (int)sf.size(); view.log_scale = p[20]; view.scale_factors = sf.data();
        view.ak_nlevels = (int)akSf.size(); view.ak_log_scale = p[21]; view.ak_scale_factors = akSf.data();
        const float th = p[22];
        auto kps = rd<eorb_host::KeyPoint>(dir + "/kps.bin");
        auto dsc = rd<uint8_t>(dir + "/desc.bin");
        eorb_host::Mat8 desc((int)kps.size(), 32); std::memcpy(desc.ptr(), dsc.data(), dsc.size());
        ORB_SLAM3::FrameView KF(kps, desc, 346, 260);
        ORB_SLAM3::ORBmatcher::MapPoints P;
        P.pos = rd<float>(dir + "/pos.bin"); P.normal = rd<float>(dir + "/normal.bin");
        P.minDist = rd<float>(dir + "/min_dist.bin"); P.maxDist = rd<float>(dir + "/max_dist.bin");
        auto md = rd<uint8_t>(dir + "/mp_desc.bin");
        P.desc = eorb_host::Mat8(P.size(), 32); std::memcpy(P.desc.ptr(), md.data(), md.size());
        ORB_SLAM3::ORBmatcher::MixedKinds kinds;
        kinds.kpIsOrb = rd<uint8_t>(dir + "/kp_is_orb.bin"); kinds.kpInvSigma2 = rd<float>(dir + "/kp_inv_sigma2.bin");
        kinds.mpIsOrb = rd<uint8_t>(dir + "/mp_is_orb.bin");
        const auto uright = rd<float>(dir + "/uright.bin");
        ORB_SLAM3::ORBmatcher matcher(0.8f, true);
        ORB_SLAM3::ORBmatcher::SideProjection a, b;
        matcher.ProjectKeyFrameSideMixed(view, P, kinds, th, a);
        wr(dir + "/a_valid.bin", a.valid); wr(dir + "/a_uv.bin", a.uv); wr(dir + "/a_radius.bin", a.radius); wr(dir + "/a_level.bin", a.level);
        wr(dir + "/a_q_ur.bin", a.qUr); wr(dir + "/a_dist3d.bin", a.dist3D); wr(dir + "/a_reason.bin", a.reason);
        std::vector<int> bi, bd;
        matcher.KeyFrameRadiusMatchMixed(KF, kinds, a.valid, a.uv, a.radius, a.level, P.desc, &uright, &a.qUr, nullptr, 0.f, bi, bd);
        wr(dir + "/match_idx.bin", bi); wr(dir + "/match_dist.bin", bd);
        matcher.FuseMixed(KF, view, P, kinds, &uright, th, bi, bd, &b);
        wr(dir + "/fuse_idx.bin", bi); wr(dir + "/fuse_dist.bin", bd); wr(dir + "/b_reason.bin", b.reason); wr(dir + "/b_level.bin", b.level);
        auto taken = rd<uint8_t>(dir + "/taken.bin");
        matcher.SearchByProjectionMixed(KF, view, P, kinds, taken, th, 1.0f, bi, bd);
        wr(dir + "/scw_idx.bin", bi); wr(dir + "/scw_dist.bin", bd); wr(dir + "/scw_taken.bin", taken);
        // the same keyframe twice and an empty one between them
        std::vector<eorb_host::KeyPoint> k2(kps); k2.insert(k2.end(), kps.begin(), kps.end());
        eorb_host::Mat8 d2((int)k2.size(), 32);
        std::memcpy(d2.ptr(), dsc.data(), dsc.size()); std::memcpy(d2.ptr() + dsc.size(), dsc.data(), dsc.size());
        std::vector<float> u2(uright); u2.insert(u2.end(), uright.begin(), uright.end());
        ORB_SLAM3::ORBmatcher::MixedKinds kk(kinds);
        kk.kpIsOrb.insert(kk.kpIsOrb.end(), kinds.kpIsOrb.begin(), kinds.kpIsOrb.end());
        kk.kpInvSigma2.insert(kk.kpInvSigma2.end(), kinds.kpInvSigma2.begin(), kinds.kpInvSigma2.end());
        const int n = (int)kps.size();
        matcher.FuseKeyFramesMixed(std::vector<eorb_view>(3, view), std::vector<eorb_grid_bounds>(3, KF.gb), k2, d2,
                                   std::vector<int32_t>{0, n, n, 2 * n}, P, kk, &u2, th, bi, bd);
        wr(dir + "/batch_idx.bin", bi); wr(dir + "/batch_dist.bin", bd);
        std::printf("M=%d n=%d\n", P.size(), n);
        return 0;
    } catch (const eorb_host::Error& e) { std::printf("error %d: %s\n", e.code, e.what()); return 2; }
}
