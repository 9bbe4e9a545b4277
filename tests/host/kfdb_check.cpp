// A plain g++ caller of ORB_SLAM3::KeyFrameDatabase (eorb_slam_amd/host/eorb_host.hpp), built and run by tests/test_host_kfdb_cpp.py.
// Without arguments it only proves that it linked; with a directory it reads the model the test wrote there (K keyframes with map ids,
// bad flags and covisibility rows, the bad maps, queries with their map and connected keyframes), replays the test's script of adds and an
// erase, runs both queries per query vector and writes the candidate slots each returned.
#include "eorb_slam_amd/host/eorb_host.hpp"
#include <cstdio>
template <typename T> static std::vector<T> rd(const std::string& path) {
    std::vector<T> v; FILE* f = std::fopen(path.c_str(), "rb"); if (!f) return v;
    std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(T)); if (n && std::fread(v.data(), 1, (size_t)n, f) != (size_t)n) v.clear(); std::fclose(f); return v;
}
template <typename T> static void wr(const std::string& path, const std::vector<T>& v) { FILE* f = std::fopen(path.c_str(), "wb"); std::fwrite(v.data(), sizeof(T), v.size(), f); std::fclose(f); }
using ORB_SLAM3::KeyFrameDatabase;
static KeyFrameDatabase::BowVector vec(const std::vector<uint32_t>& w, const std::vector<double>& v, int a, int b) {
    KeyFrameDatabase::BowVector o;
    for (int i = a; i < b; i++) o.emplace_back(w[i], v[i]);
    return o;
}
int main(int argc, char** argv) {
    if (argc < 2) { std::puts("linked"); return 0; }          // link check only (no GPU touched)
    const std::string dir = argv[1];
    try {
        const auto hdr = rd<int32_t>(dir + "/hdr.bin");        // K, number of queries, nNumCandidates, keyframe erased and added again
        if (hdr.size() < 4) { std::puts("no model"); return 3; }
        const int K = hdr[0], Q = hdr[1], nNum = hdr[2], again = hdr[3];
        const auto off = rd<int32_t>(dir + "/kf_off.bin"); const auto w = rd<uint32_t>(dir + "/kf_word.bin"); const auto v = rd<double>(dir + "/kf_val.bin");
        const auto map = rd<int32_t>(dir + "/kf_map.bin"); const auto bad = rd<uint8_t>(dir + "/kf_bad.bin"); const auto covis = rd<int32_t>(dir + "/covis.bin");
        const auto badmaps = rd<int32_t>(dir + "/badmaps.bin");
        const auto qoff = rd<int32_t>(dir + "/q_off.bin"); const auto qw = rd<uint32_t>(dir + "/q_word.bin"); const auto qv = rd<double>(dir + "/q_val.bin");
        const auto qmap = rd<int32_t>(dir + "/q_map.bin"); const auto coff = rd<int32_t>(dir + "/conn_off.bin"); const auto conn = rd<int32_t>(dir + "/conn.bin");
        KeyFrameDatabase db;
        std::vector<int> slot(K);
        for (int k = 0; k < K; k++) slot[k] = db.add(vec(w, v, off[k], off[k + 1]), map[k]);
        db.erase(slot[again]);                                  // ... and back: the keyframe is now the last of every list
        slot[again] = db.add(vec(w, v, off[again], off[again + 1]), map[again]);
        for (int k = 0; k < K; k++) {
            if (slot[k] != k) { std::printf("keyframe %d in slot %d\n", k, slot[k]); return 4; }
            db.SetBadFlag(k, bad[k] != 0);
            db.SetBestCovisibility(k, std::vector<int>(covis.begin() + (size_t)k * 10, covis.begin() + (size_t)(k + 1) * 10));
        }
        for (int m : badmaps) db.SetMapBad(m);
        std::vector<int32_t> reloc, loop, merge, cnt;
        for (int q = 0; q < Q; q++) {
            const auto bow = vec(qw, qv, qoff[q], qoff[q + 1]);
            const std::vector<int> r = db.DetectRelocalizationCandidates(bow, qmap[q]);
            std::vector<int> vpLoopCand, vpMergeCand;
            db.DetectNBestCandidates(bow, qmap[q], std::vector<int>(conn.begin() + coff[q], conn.begin() + coff[q + 1]), vpLoopCand, vpMergeCand, nNum);
            cnt.push_back((int32_t)r.size()); cnt.push_back((int32_t)vpLoopCand.size()); cnt.push_back((int32_t)vpMergeCand.size());
            reloc.insert(reloc.end(), r.begin(), r.end()); loop.insert(loop.end(), vpLoopCand.begin(), vpLoopCand.end());
            merge.insert(merge.end(), vpMergeCand.begin(), vpMergeCand.end());
        }
        wr(dir + "/cnt.bin", cnt); wr(dir + "/reloc.bin", reloc); wr(dir + "/loop.bin", loop); wr(dir + "/merge.bin", merge);
        db.clearMap(map[0]);
        db.clear();
    } catch (const eorb_host::Error& e) { std::printf("error %d: %s\n", e.code, e.what()); return 2; }
    std::puts("done");
    return 0;
}
