// eorb_host.hpp -- C++ host side above the C ABI (include/eorb_fe.h), mirroring the reference's three seams
// with the same names, argument meaning and error behaviour, but OpenCV-free (own minimal Mat / KeyPoint):
//
//   EORB_SLAM::EvImConverter::ev2im / ev2im_gauss     include/Event/EventConversion.h:52-56
//   ORB_SLAM3::ORBextractor::operator()                include/ORBextractor.h:75-81 (both overloads)
//   ORB_SLAM3::ORBmatcher::SearchForInitialization      include/ORBmatcher.h (ORBmatcher.cc:714-831)
//
// The reference's own build keeps cv::Mat / cv::KeyPoint: INTEGRATION.md shows that adapter.  This header is
// what a C++ host without OpenCV uses, and what tests/test_host_cpp.py compiles.  Everything runs on the GPU
// through libeorb_fe.so; there is no CPU path here.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/eorb_fe.h"

namespace eorb_host {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// one context per calling thread AT A TIME (the ABI's threading contract)
class Context {
public:
    explicit Context(int device = 0, void* hipStream = nullptr) {
        int rc = eorb_create(device, hipStream, &h_);
        if (rc != EORB_OK) throw Error(rc, "eorb_create failed");
    }
    ~Context() { eorb_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    eorb_ctx* get() const { return h_; }
    void check(int rc) const { if (rc != EORB_OK) throw Error(rc, eorb_last_error(h_)); }
    unsigned maps_epoch = 0, voc_epoch = 0, calib_epoch = 0;      // which shared state of the pool this context has loaded
private:
    eorb_ctx* h_ = nullptr;
};

// Warm contexts shared by the threads of the process.  The reference calls the converters from long-lived tracker threads AND
// from four transient std::threads per motion-compensated image (src/Event/EvImBuilder.cpp:1165-1193): a context per thread
// would be created (device workspaces, pinned staging) and destroyed on every dispatch.  A thread borrows a context on its first
// call and hands it back when it exits; state that the reference keeps in process-wide objects (the calibrator's undistortion maps,
// the vocabulary) is recorded in the pool and loaded into a borrowed context that has not seen its current version yet.
class ContextPool {
public:
    static ContextPool& instance() { static ContextPool p; return p; }
    Context* acquire() {
        Context* c = nullptr;
        {
            std::lock_guard<std::mutex> g(m_);
            if (!free_.empty()) { c = free_.back(); free_.pop_back(); }
        }
        if (!c) {
            std::unique_ptr<Context> n(new Context());
            c = n.get();
            std::lock_guard<std::mutex> g(m_);
            all_.push_back(std::move(n));
        }
        try { sync_state(*c); }
        catch (...) { release(c); throw; }           // (a failed upload must not strand the context outside the free list)
        return c;
    }
    void release(Context* c) { std::lock_guard<std::mutex> g(m_); free_.push_back(c); }
    size_t created() const { std::lock_guard<std::mutex> g(m_); return all_.size(); }
    // process-wide state: immutable snapshots, replaced as a whole
    struct Maps { std::vector<float> mapX, mapY; int LW = 0, LH = 0; bool check = true; };
    struct Voc { int L = 0; std::vector<int32_t> childOff, childIds, wordId; std::vector<uint8_t> nodeDesc; std::vector<double> weight; };
    void set_maps(const std::vector<float>& mapX, const std::vector<float>& mapY, int LW, int LH, bool check) {
        auto m = std::make_shared<Maps>(); m->mapX = mapX; m->mapY = mapY; m->LW = LW; m->LH = LH; m->check = check;
        std::lock_guard<std::mutex> g(m_);
        maps_ = std::move(m); maps_epoch_.store(maps_epoch_.load(std::memory_order_relaxed) + 1, std::memory_order_release);
    }
    // the calibrator's K, distortion coefficients, R and P (MyCalibrator.cpp:11-17): every context of the process
    // (`load` = eorb_set_calibration, named by the caller: the pool itself then links against a library without that entry, such as
    // the stub the thread-sanitizer test of the pool uses)
    void set_calibration(const eorb_calib& q, int (*load)(eorb_ctx*, const eorb_calib*)) {
        auto p = std::make_shared<eorb_calib>(q);
        std::lock_guard<std::mutex> g(m_);
        calib_load_ = load;
        calib_ = std::move(p); calib_epoch_.store(calib_epoch_.load(std::memory_order_relaxed) + 1, std::memory_order_release);
    }
    // maps that context `c` has just built on the device (eorb_generate_undistort_maps) and downloaded: the other contexts upload them,
    // `c` already holds them
    void set_maps_built_by(Context& c, const std::vector<float>& mapX, const std::vector<float>& mapY, int LW, int LH, bool check) {
        auto m = std::make_shared<Maps>(); m->mapX = mapX; m->mapY = mapY; m->LW = LW; m->LH = LH; m->check = check;
        std::lock_guard<std::mutex> g(m_);
        maps_ = std::move(m);
        const unsigned e = maps_epoch_.load(std::memory_order_relaxed) + 1;
        maps_epoch_.store(e, std::memory_order_release);
        c.maps_epoch = e;
    }
    void set_vocabulary(Voc v) {
        auto p = std::make_shared<Voc>(std::move(v));
        std::lock_guard<std::mutex> g(m_);
        voc_ = std::move(p); voc_epoch_.store(voc_epoch_.load(std::memory_order_relaxed) + 1, std::memory_order_release);
    }
    // Loads the maps / the vocabulary into a context that has not seen their current version.  Called on every API call of a
    // thread: the common case is two atomic loads; the process-wide mutex is only held to take a reference to the snapshot, never
    // across the GPU upload (other threads' calls do not wait for it).  `c` belongs to the calling thread.
    void sync_state(Context& c) {
        if (c.maps_epoch != maps_epoch_.load(std::memory_order_acquire)) {
            std::shared_ptr<const Maps> m; unsigned e;
            { std::lock_guard<std::mutex> g(m_); m = maps_; e = maps_epoch_.load(std::memory_order_relaxed); }
            if (m) c.check(eorb_set_undistort_maps(c.get(), m->mapX.data(), m->mapY.data(), m->LW, m->LH, m->check));
            c.maps_epoch = e;
        }
        if (c.calib_epoch != calib_epoch_.load(std::memory_order_acquire)) {
            std::shared_ptr<const eorb_calib> q; unsigned e;
            { std::lock_guard<std::mutex> g(m_); q = calib_; e = calib_epoch_.load(std::memory_order_relaxed); }
            if (q) c.check(calib_load_(c.get(), q.get()));
            c.calib_epoch = e;
        }
        if (c.voc_epoch != voc_epoch_.load(std::memory_order_acquire)) {
            std::shared_ptr<const Voc> v; unsigned e;
            { std::lock_guard<std::mutex> g(m_); v = voc_; e = voc_epoch_.load(std::memory_order_relaxed); }
            if (v) c.check(eorb_bow_set_vocabulary(c.get(), (int)v->childOff.size() - 1, v->L, v->childOff.data(), v->childIds.data(),
                                                   v->nodeDesc.data(), v->wordId.data(), v->weight.data()));
            c.voc_epoch = e;
        }
    }
private:
    mutable std::mutex m_;
    std::vector<std::unique_ptr<Context>> all_;
    std::vector<Context*> free_;
    std::shared_ptr<const Maps> maps_; std::atomic<unsigned> maps_epoch_{0};
    std::shared_ptr<const Voc> voc_; std::atomic<unsigned> voc_epoch_{0};
    std::shared_ptr<const eorb_calib> calib_; std::atomic<unsigned> calib_epoch_{0};
    int (*calib_load_)(eorb_ctx*, const eorb_calib*) = nullptr;      // written under m_ before the epoch's release store
};

// the calling thread's context: borrowed from the pool for the lifetime of the thread
inline Context& thread_context() {
    struct Lease {
        Context* c;
        Lease() : c(ContextPool::instance().acquire()) {}
        ~Lease() { ContextPool::instance().release(c); }
    };
    thread_local Lease lease;
    ContextPool::instance().sync_state(*lease.c);        // (a long-lived thread picks up maps / vocabulary set after it started)
    return *lease.c;
}

// minimal stand-ins for cv::Mat (CV_8UC1 / CV_32FC1) and cv::KeyPoint
template <typename T> struct Mat_ {
    int rows = 0, cols = 0;
    std::vector<T> data;
    Mat_() = default;
    Mat_(int r, int c) : rows(r), cols(c), data((size_t)r * c) {}
    bool empty() const { return rows == 0 || cols == 0; }
    T* ptr(int r = 0) { return data.data() + (size_t)r * cols; }
    const T* ptr(int r = 0) const { return data.data() + (size_t)r * cols; }
};
using Mat8 = Mat_<uint8_t>;
using Mat32f = Mat_<float>;
using KeyPoint = eorb_keypoint;         // same 28-byte layout as cv::KeyPoint
using EventData = eorb_event;           // same 24-byte layout as EORB_SLAM::EventData

}  // namespace eorb_host

namespace EORB_SLAM {

// include/Event/EventConversion.h:45-75: static converters; thread-safe through per-thread contexts
struct EvImConverter {
    // returns the CV_8UC1 image when `normalized` (and, for ev2im, max > min), else the CV_32FC1 image in out32
    static bool ev2im(const std::vector<eorb_host::EventData>& vEvData, unsigned imWidth, unsigned imHeight, bool pol,
                      bool normalized, eorb_host::Mat8& out8, eorb_host::Mat32f& out32) {
        auto& c = eorb_host::thread_context();
        out8 = eorb_host::Mat8((int)imHeight, (int)imWidth); out32 = eorb_host::Mat32f((int)imHeight, (int)imWidth);
        int is_u8 = 0;
        c.check(eorb_ev2im(c.get(), vEvData.data(), vEvData.size(), (int)imWidth, (int)imHeight, pol, normalized,
                           out32.ptr(), out8.ptr(), nullptr, &is_u8));
        return is_u8 != 0;
    }
    static bool ev2im_gauss(const std::vector<eorb_host::EventData>& vEvData, unsigned imWidth, unsigned imHeight,
                            float sigma, bool pol, bool normalized, eorb_host::Mat8& out8, eorb_host::Mat32f& out32) {
        auto& c = eorb_host::thread_context();
        out8 = eorb_host::Mat8((int)imHeight, (int)imWidth); out32 = eorb_host::Mat32f((int)imHeight, (int)imWidth);
        c.check(eorb_ev2im_gauss(c.get(), vEvData.data(), vEvData.size(), (int)imWidth, (int)imHeight, sigma, pol,
                                 normalized, out32.ptr(), out8.ptr(), nullptr));
        return normalized;
    }
    // raw sensor events + MyCalibrator maps (EventLoader.cpp:264-305 fused with ev2im_gauss)
    static void ev2im_gauss_raw(const std::vector<eorb_raw_event>& vRaw, unsigned imWidth, unsigned imHeight, float sigma, bool pol,
                                bool normalized, eorb_host::Mat8& out8, eorb_host::Mat32f& out32) {
        auto& c = eorb_host::thread_context();
        out8 = eorb_host::Mat8((int)imHeight, (int)imWidth); out32 = eorb_host::Mat32f((int)imHeight, (int)imWidth);
        c.check(eorb_ev2im_gauss_raw(c.get(), vRaw.data(), vRaw.size(), (int)imWidth, (int)imHeight, sigma, pol, normalized,
                                     out32.ptr(), out8.ptr(), nullptr));
    }
};

// src/Event/EventLoader.cpp: the parts of EventDataStore the GPU takes over
struct EventDataStore {
    // MyCalibrator::mUndistMapX / mUndistMapY (LH x LW floats each) for this thread's context
    static void setUndistortMaps(const std::vector<float>& mapX, const std::vector<float>& mapY, int LW, int LH, bool checkInImage) {
        eorb_host::ContextPool::instance().set_maps(mapX, mapY, LW, LH, checkInImage);      // every context of the process
    }
    // getline + parseLine + isComment over a text buffer (:80-92); throws eorb_host::Error for a line outside the grammar
    static std::vector<eorb_raw_event> parseText(const std::string& text) {
        auto& c = eorb_host::thread_context();
        size_t lines = 1; for (char ch : text) lines += ch == '\n';
        std::vector<eorb_raw_event> out(lines); size_t n = 0; int64_t bad = -1;
        c.check(eorb_parse_events_text(c.get(), text.data(), text.size(), out.data(), out.size(), &n, &bad));
        out.resize(n);
        return out;
    }
    // the rectification loop of getEventChunkRectified (:264-305)
    static std::vector<eorb_host::EventData> rectify(const std::vector<eorb_raw_event>& raw, int imWidth, int imHeight, double tsFactor) {
        auto& c = eorb_host::thread_context();
        std::vector<eorb_host::EventData> out(raw.size()); size_t n = 0;
        c.check(eorb_undistort_events(c.get(), raw.data(), raw.size(), imWidth, imHeight, tsFactor, out.data(), &n));
        out.resize(n);
        return out;
    }
};

// EORB_SLAM::MyCalibrator (src/Utils/MyCalibrator.cpp): K, distCoefs, R, P as CV_32F values (empty vectors = cv::Mat()); the points go
// through cv::undistortPoints / cv::fisheye::undistortPoints on the device.  The calibration is process-wide state of the pool, like
// the maps: every thread's context loads it before its next call.  P stays as given: the reference's constructor replaces an empty P
// of a pinhole camera by K (:25-27), and so should the caller of this one.
class MyCalibrator {
public:
    MyCalibrator(const float K[9], const std::vector<float>& distCoefs, int imWidth, int imHeight, const std::vector<float>& R = {},
                 const std::vector<float>& P = {}, bool isFishEye = false) : mImWidth(imWidth), mImHeight(imHeight) {
        q_ = eorb_calib{};
        q_.model = isFishEye ? 1 : 0;
        std::memcpy(q_.K, K, sizeof q_.K);
        q_.n_dist = (int)distCoefs.size();
        for (size_t i = 0; i < distCoefs.size() && i < 8; i++) q_.dist[i] = distCoefs[i];
        if (R.size() == 9) { std::memcpy(q_.R, R.data(), sizeof q_.R); q_.has_R = 1; }
        else if (!R.empty()) throw eorb_host::Error(EORB_E_ARG, "MyCalibrator: R must be 3x3");
        if (P.size() == 9 || P.size() == 12) { std::memcpy(q_.P, P.data(), P.size() * sizeof(float)); q_.p_cols = (int)P.size() / 3; }
        else if (!P.empty()) throw eorb_host::Error(EORB_E_ARG, "MyCalibrator: P must be 3x3 or 3x4");
        auto& c = eorb_host::thread_context();
        c.check(eorb_set_calibration(c.get(), &q_));                         // (validates the record before the pool hands it out)
        eorb_host::ContextPool::instance().set_calibration(q_, &eorb_set_calibration);
    }
    const eorb_calib& calibration() const { return q_; }
    // :46-50
    static bool isDistorted(const std::vector<float>& distCoefs) { return distCoefs.size() >= 4 && std::fabs((double)distCoefs[0]) > 1e-9; }
    // :181-283; an empty input leaves vUndistKPts alone (:202-205)
    void undistKeyPoints(const std::vector<eorb_host::KeyPoint>& vDistKPts, std::vector<eorb_host::KeyPoint>& vUndistKPts) const {
        if (vDistKPts.empty()) return;
        auto& c = eorb_host::thread_context();
        std::vector<eorb_host::KeyPoint> out(vDistKPts.size());
        c.check(eorb_undistort_keypoints(c.get(), vDistKPts.data(), (int)vDistKPts.size(), out.data()));
        vUndistKPts.swap(out);
    }
    // :104-156, one point or n points (x, y interleaved)
    void undistPoint(float x, float y, float& ux, float& uy) const {
        const float in[2] = {x, y}; float out[2];
        auto& c = eorb_host::thread_context();
        c.check(eorb_undistort_points(c.get(), in, 1, out));
        ux = out[0]; uy = out[1];
    }
    std::vector<float> undistPoints(const std::vector<float>& xy) const {
        std::vector<float> out(xy.size());
        auto& c = eorb_host::thread_context();
        c.check(eorb_undistort_points(c.get(), xy.data(), (int)(xy.size() / 2), out.data()));
        return out;
    }
    // :52-102: mUndistMapX / mUndistMapY built on the device, installed in this thread's context and recorded in the pool for the others
    void generateUndistMaps(bool checkInImage = true) {
        auto& c = eorb_host::thread_context();
        mUndistMapX.assign((size_t)mImWidth * mImHeight, 0.f); mUndistMapY.assign((size_t)mImWidth * mImHeight, 0.f);
        c.check(eorb_generate_undistort_maps(c.get(), mImWidth, mImHeight, checkInImage, mUndistMapX.data(), mUndistMapY.data()));
        eorb_host::ContextPool::instance().set_maps_built_by(c, mUndistMapX, mUndistMapY, mImWidth, mImHeight, checkInImage);
    }
    std::vector<float> mUndistMapX, mUndistMapY;
private:
    int mImWidth, mImHeight;
    eorb_calib q_;
};

// The data path of EORB_SLAM::EvImBuilder::Track (src/Event/EvImBuilder.cpp:1300-1515) over the one-call seams: per chunk of
// l1ChunkSize events the event image and its frame -- INIT: detect-only ORBextractor + ELK_Tracker::setRefImage (init :568-592);
// TRACKING: ELK_Tracker::trackAndMatchCurrImage (KLT_Tracker.cpp:215-234) + refineTrackedPts (:104-151) -- the window-size rule
// (resolveEvWinSize :209-232) and, on a dispatch, generateMCImage (:1146-1247) + isMcImageGood (:260-267).  The optimisers that hand
// generateMCImage its poses, step()'s two-view refinement (its RANSAC and CheckRT stages: ORB_SLAM3::TwoViewReconstruction below), the
// IMU and the L2 queue stay with the caller, as in the reference.
// (Python twin with the same members: eorb_slam_amd/frontend.py::EvImBuilder; tests/test_gpu_chain.py checks that one against the
// oracle's chain chunk by chunk, tests/test_host_cpp.py checks this one against the separate seams.)
class EvImBuilder {
public:
    enum TrackState { IDLE, INIT, TRACKING };
    struct Params {            // Event.* of Examples/Event/EvETHZ.yaml:178-208
        int imWidth = 240, imHeight = 180; unsigned l1ChunkSize = 2000; int l1NumLoop = 3; bool l1FixedWinSz = false, continTracking = true;
        float maxPixelDisp = 3.f, l1WinOverlap = 0.5f, l1ImSigma = 1.f; double minEvGenRate = 1.0;
        int maxNumPts = 400, fastTh = 0, imMargin = 9; eorb_klt_params klt{23, 1, 10, 0.03, 1e-4f};
    };
    struct MciPoses { const eorb_se3_motion* dp = nullptr; const eorb_se3_motion* ba = nullptr; const float* se2 = nullptr; int nse2 = 3; const eorb_camera* cam = nullptr; };
    struct ChunkResult {
        TrackState state = IDLE; bool dispatched = false; int skipped = 0;
        std::vector<eorb_host::KeyPoint> kps;                          // INIT frame
        std::vector<float> pts; std::vector<uint8_t> status; std::vector<float> err; std::vector<int> matches12;   // TRACKING frame
        unsigned nMatches = 0; float medPxDisp = 0.f; unsigned chunkSize = 0;
        float focus[5] = {-1, -1, -1, -1, -1}; int winner = -1; eorb_host::Mat8 mcImage; std::vector<eorb_host::KeyPoint> l2Kps; bool mcGood = false;
        size_t window = 0, overlap = 0;                                // events of the dispatched window / handed back to the queue (its tail)
    };
    static const int DEF_TH_MIN_KPTS = 100, DEF_TH_MIN_MATCHES = 50;   // include/Event/EventData.h:24-26

    explicit EvImBuilder(const Params& p) : P(p), mL1EvWinSize(p.l1ChunkSize), mInitL1EvWinSize(p.l1ChunkSize) {
        eorb_orb_params q{p.maxNumPts, 1.0f, 1, p.fastTh, 0, p.imMargin, p.imWidth};       // "FAST = ORB with one level": EvBaseTracker.cpp:150-164
        l1_.check(eorb_orb_configure(l1_.get(), &q, p.imWidth, p.imHeight));
        q.nfeatures = 2 * p.maxNumPts;                                  // the L2 tracker's extractor: EvAsynchTracker.cpp:51
        l2_.check(eorb_orb_configure(l2_.get(), &q, p.imWidth, p.imHeight));
        cap1_ = eorb_orb_max_keypoints(l1_.get()); cap2_ = eorb_orb_max_keypoints(l2_.get());
        mnWinOverlap = (unsigned long)(p.l1WinOverlap * (double)(p.l1NumLoop * mL1EvWinSize));      // :40
        reset();
    }
    void resetAll() { mStat = IDLE; mL1EvWinSize = mInitL1EvWinSize; reset(); }                      // :70-93
    unsigned getL1ChunkSize() const { return mL1EvWinSize; }

    // one pass of the loop body for the chunk l1Evs; `poses` = what the resolve*() calls of generateMCImage deliver (absent = failed)
    ChunkResult Track(const std::vector<eorb_host::EventData>& l1Evs, const MciPoses* (*mciPoses)(const std::vector<eorb_host::EventData>&, void*) = nullptr, void* user = nullptr) {
        ChunkResult out;
        if (mStat == IDLE) mStat = INIT;
        if (mStat == INIT) reset();
        if (l1Evs.empty()) return out;
        const double evTspan = l1Evs.back().ts - l1Evs[0].ts;           // calcEventGenRate, src/Event/EventData.cpp:14-19
        const double evGenRate = (double)l1Evs.size() / (evTspan * P.imWidth * P.imHeight);
        out.state = mStat;
        const int rate = checkEvGenRate(evGenRate);
        if (rate != 0) {
            if (rate == -1) mStat = INIT; else mvSharedL2Evs.insert(mvSharedL2Evs.end(), l1Evs.begin(), l1Evs.end());
            out.skipped = rate;
            return out;
        }
        bool sendMCF = false;
        if (mStat == INIT) {
            out.kps.assign(cap1_, eorb_host::KeyPoint{});
            int n = 0, mono = 0;
            l1_.check(eorb_ev_slice_extract(l1_.get(), l1Evs.data(), nullptr, l1Evs.size(), P.l1ImSigma, 0, 1000, 0, out.kps.data(), nullptr, nullptr,
                                            cap1_, &n, &mono, nullptr));
            out.kps.resize(n);
            mRefKPoints = out.kps; mvMatchesCnt.assign(n, 1);
            mLastTrackedPts.resize(2 * (size_t)n);
            for (int i = 0; i < n; i++) { mLastTrackedPts[2 * i] = out.kps[i].x; mLastTrackedPts[2 * i + 1] = out.kps[i].y; }
            if (n > DEF_TH_MIN_KPTS || (P.continTracking && P.l1FixedWinSz)) { updateState(l1Evs); mStat = TRACKING; }
            else mL1EvWinSize = mInitL1EvWinSize;
        } else {
            const int nref = (int)mRefKPoints.size();
            out.status.assign(nref, 0); out.err.assign(nref, 0.f);
            l1_.check(eorb_ev_slice_track(l1_.get(), l1Evs.data(), nullptr, l1Evs.size(), P.l1ImSigma, &P.klt, mLastTrackedPts.data(), out.status.data(),
                                          out.err.data(), nref, nullptr));
            out.pts = mLastTrackedPts;
            out.matches12.assign(nref, -1);
            std::vector<float> vPxDisp;
            for (int i = 0; i < nref; i++) {                            // refineTrackedPts
                const float x = out.pts[2 * i], y = out.pts[2 * i + 1];
                if (out.status[i] == 1 && x >= 0 && x < (float)P.imWidth && y >= 0 && y < (float)P.imHeight) {
                    mvMatchesCnt[i]++; out.matches12[i] = i; out.nMatches++;
                    const float dx = x - mRefKPoints[i].x, dy = y - mRefKPoints[i].y;
                    vPxDisp.push_back(std::sqrt(dx * dx + dy * dy));
                }
            }
            std::sort(vPxDisp.begin(), vPxDisp.end());
            out.medPxDisp = vPxDisp.empty() ? 0.f : vPxDisp[vPxDisp.size() / 2];
            if (out.nMatches < (unsigned)DEF_TH_MIN_MATCHES && !P.continTracking && mCurrIdx < 3) { mL1EvWinSize = mInitL1EvWinSize; mStat = INIT; out.chunkSize = mL1EvWinSize; return out; }
            updateState(l1Evs);
            const bool dispatchMCI = resolveEvWinSize(out.medPxDisp);
            if (dispatchMCI || out.nMatches < (unsigned)DEF_TH_MIN_MATCHES) { mStat = INIT; sendMCF = true; }
        }
        out.chunkSize = mL1EvWinSize;
        if (sendMCF) {
            const MciPoses none; const MciPoses* mp = mciPoses ? mciPoses(mvSharedL2Evs, user) : &none;
            out.mcImage = eorb_host::Mat8(P.imHeight, P.imWidth);
            out.l2Kps.assign(cap2_, eorb_host::KeyPoint{});
            int n = 0;
            l1_.check(eorb_ev_mc_contest(l1_.get(), mvSharedL2Evs.data(), mvSharedL2Evs.size(), mp->cam, mp->dp, mp->ba, mp->se2, mp->nse2, P.imWidth, P.imHeight,
                                         P.l1ImSigma, out.focus, &out.winner, out.mcImage.ptr(), l2_.get(), 0, 1000, out.l2Kps.data(), cap2_, &n));
            out.l2Kps.resize(n);
            out.dispatched = true; out.window = mvSharedL2Evs.size();
            out.mcGood = n > DEF_TH_MIN_KPTS || P.continTracking;
            if (P.continTracking) out.overlap = P.l1FixedWinSz ? mnWinOverlap : (size_t)(mvSharedL2Evs.size() * P.l1WinOverlap);     // :1465-1469
        }
        return out;
    }
    const std::vector<eorb_host::EventData>& accumulatedEvents() const { return mvSharedL2Evs; }

private:
    void reset() { mCurrIdx = 0; mCntLowEvGenRate = 0; mvSharedL2Evs.clear(); mvMatchesCnt.clear(); }          // :95-139
    void updateState(const std::vector<eorb_host::EventData>& ev) { mCurrIdx++; mvSharedL2Evs.insert(mvSharedL2Evs.end(), ev.begin(), ev.end()); }      // :427-435
    int checkEvGenRate(double rate) {                                    // :284-328
        if (rate > P.minEvGenRate) { mCntLowEvGenRate = 0; return 0; }
        if (P.continTracking) return (!P.l1FixedWinSz && mStat == INIT) ? -1 : 0;
        if (mStat == INIT) return -1;
        return ++mCntLowEvGenRate > 3 ? -1 : 1;
    }
    bool resolveEvWinSize(float medPxDisp) {                             // :209-232, calcNewL1ChunkSize :197-201
        if (!P.l1FixedWinSz && medPxDisp > P.maxPixelDisp) { mL1EvWinSize = (unsigned)floorf(((float)(mCurrIdx + 1) / medPxDisp) * ((float)mL1EvWinSize)); return true; }
        return P.l1FixedWinSz && (int)mCurrIdx >= P.l1NumLoop;
    }
    Params P;
    eorb_host::Context l1_, l2_;
    int cap1_ = 0, cap2_ = 0;
    TrackState mStat = IDLE;
    unsigned mCurrIdx = 0, mL1EvWinSize, mInitL1EvWinSize; int mCntLowEvGenRate = 0; unsigned long mnWinOverlap = 0;
    std::vector<eorb_host::EventData> mvSharedL2Evs;
    std::vector<eorb_host::KeyPoint> mRefKPoints; std::vector<float> mLastTrackedPts; std::vector<int> mvMatchesCnt;
};

}  // namespace EORB_SLAM

namespace ORB_SLAM3 {

struct ORBxParams {            // include/ORBextractor.h:33-47
    int nfeatures = 0; float scaleFactor = 1; int nlevels = 1; int iniThFAST = 10; int minThFAST = 7; int edgeTh = 19;
    int imWidth = 0, imHeight = 0;
};

class ORBextractor {           // include/ORBextractor.h:49-139; one instance per thread, like the reference
public:
    explicit ORBextractor(const ORBxParams& p) : p_(p) {
        eorb_orb_params q{p.nfeatures, p.scaleFactor, p.nlevels, p.iniThFAST, p.minThFAST, p.edgeTh, p.imWidth};
        ctx_.check(eorb_orb_configure(ctx_.get(), &q, p.imWidth, p.imHeight));
        cap_ = eorb_orb_max_keypoints(ctx_.get());
        mvScaleFactor.resize(p.nlevels); mvInvScaleFactor.resize(p.nlevels); mnFeaturesPerLevel.resize(p.nlevels);
        ctx_.check(eorb_orb_get_tables(ctx_.get(), mvScaleFactor.data(), mvInvScaleFactor.data(), mnFeaturesPerLevel.data(), &edge_));
    }
    // with descriptors (src/ORBextractor.cc:1092-1176); returns monoIndex, -1 for an empty image
    int operator()(const eorb_host::Mat8& image, std::vector<eorb_host::KeyPoint>& keypoints, eorb_host::Mat8& descriptors,
                   const std::vector<int>& vLappingArea) {
        if (image.empty()) return -1;
        keypoints.assign(cap_, eorb_host::KeyPoint{});
        eorb_host::Mat8 d(cap_, 32);
        int n = 0, mono = 0;
        ctx_.check(eorb_orb_extract(ctx_.get(), image.ptr(), image.cols, image.rows, image.cols, vLappingArea[0], vLappingArea[1], 1,
                                    keypoints.data(), d.ptr(), nullptr, cap_, &n, &mono));
        keypoints.resize(n);
        descriptors = eorb_host::Mat8(n, 32);            // released (0 rows) when n == 0, like _descriptors.release()
        if (n) std::memcpy(descriptors.ptr(), d.ptr(), (size_t)n * 32);
        return mono;
    }
    // detect only (:1178-1238)
    int operator()(const eorb_host::Mat8& image, std::vector<eorb_host::KeyPoint>& keypoints, const std::vector<int>& vLappingArea) {
        if (image.empty()) return -1;
        keypoints.assign(cap_, eorb_host::KeyPoint{});
        int n = 0, mono = 0;
        ctx_.check(eorb_orb_extract(ctx_.get(), image.ptr(), image.cols, image.rows, image.cols, vLappingArea[0], vLappingArea[1], 0,
                                    keypoints.data(), nullptr, nullptr, cap_, &n, &mono));
        keypoints.resize(n);
        return mono;
    }
    // Frame::Frame(imLeft, imRight, ...) (src/Frame.cc:97-152): ExtractORB on both images (:122-125) + ComputeStereoMatches (:869-1048)
    // in one call; mb = baseline (mbf / fx).  Fills what the constructor fills: mvKeys, mDescriptors, mvKeysRight, mDescriptorsRight,
    // mvuRight, mvDepth.  Returns the number of correlated matches before the median cut.
    int ExtractStereo(const eorb_host::Mat8& imLeft, const eorb_host::Mat8& imRight, float mb, float mbf,
                      std::vector<eorb_host::KeyPoint>& mvKeys, eorb_host::Mat8& mDescriptors,
                      std::vector<eorb_host::KeyPoint>& mvKeysRight, eorb_host::Mat8& mDescriptorsRight,
                      std::vector<float>& mvuRight, std::vector<float>& mvDepth) {
        mvKeys.assign(cap_, eorb_host::KeyPoint{}); mvKeysRight.assign(cap_, eorb_host::KeyPoint{});
        eorb_host::Mat8 dl(cap_, 32), dr(cap_, 32);
        mvuRight.assign(cap_, -1.0f); mvDepth.assign(cap_, -1.0f);
        int nl = 0, nr = 0, nm = 0;
        ctx_.check(eorb_frame_stereo(ctx_.get(), imLeft.ptr(), imRight.ptr(), imLeft.cols, imLeft.rows, imLeft.cols, mb, mbf, mvKeys.data(), dl.ptr(), &nl,
                                     mvKeysRight.data(), dr.ptr(), &nr, cap_, mvuRight.data(), mvDepth.data(), &nm));
        mvKeys.resize(nl); mvKeysRight.resize(nr); mvuRight.resize(nl); mvDepth.resize(nl);
        mDescriptors = eorb_host::Mat8(nl, 32); mDescriptorsRight = eorb_host::Mat8(nr, 32);
        if (nl) std::memcpy(mDescriptors.ptr(), dl.ptr(), (size_t)nl * 32);
        if (nr) std::memcpy(mDescriptorsRight.ptr(), dr.ptr(), (size_t)nr * 32);
        return nm;
    }
    // Frame::Frame(imLeft, imRight, ..., pCamera, pCamera2, Tlr) (src/Frame.cc:1101-1208): ExtractORB on both images with each camera's
    // mvLappingArea (:1124-1129) + ComputeStereoFishEyeMatches (:1210-1250) up to TriangulateMatches.  Fills mvKeys, mDescriptors,
    // monoLeft, mvKeysRight, mDescriptorsRight, monoRight and, per left keypoint, the candidate right keypoint (-1 none) that passed
    // Lowe's test; the caller triangulates the candidates (KannalaBrandt8::TriangulateMatches) into mvLeftToRightMatch,
    // mvRightToLeftMatch and mvDepth.  Returns the number of candidates.
    int ComputeStereoFishEyeMatches(const eorb_host::Mat8& imLeft, const eorb_host::Mat8& imRight, const std::vector<int>& vLappingAreaLeft,
                                    const std::vector<int>& vLappingAreaRight, std::vector<eorb_host::KeyPoint>& mvKeys,
                                    eorb_host::Mat8& mDescriptors, int& monoLeft, std::vector<eorb_host::KeyPoint>& mvKeysRight,
                                    eorb_host::Mat8& mDescriptorsRight, int& monoRight, std::vector<int>& vCandRight) {
        mvKeys.assign(cap_, eorb_host::KeyPoint{}); mvKeysRight.assign(cap_, eorb_host::KeyPoint{});
        eorb_host::Mat8 dl(cap_, 32), dr(cap_, 32);
        vCandRight.assign(cap_, -1);
        int nl = 0, nr = 0, nc = 0;
        ctx_.check(eorb_frame_fisheye(ctx_.get(), imLeft.ptr(), imRight.ptr(), imLeft.cols, imLeft.rows, imLeft.cols, vLappingAreaLeft[0],
                                      vLappingAreaLeft[1], vLappingAreaRight[0], vLappingAreaRight[1], mvKeys.data(), dl.ptr(), &nl, &monoLeft,
                                      mvKeysRight.data(), dr.ptr(), &nr, &monoRight, cap_, vCandRight.data(), nullptr, &nc));
        mvKeys.resize(nl); mvKeysRight.resize(nr); vCandRight.resize(nl);
        mDescriptors = eorb_host::Mat8(nl, 32); mDescriptorsRight = eorb_host::Mat8(nr, 32);
        if (nl) std::memcpy(mDescriptors.ptr(), dl.ptr(), (size_t)nl * 32);
        if (nr) std::memcpy(mDescriptorsRight.ptr(), dr.ptr(), (size_t)nr * 32);
        return nc;
    }
    // Frame::Frame(imGray, ...) (src/Frame.cc:229-266): ExtractORB, undistKeyPoints (:246-252) and ComputeImageBounds (:840-867) in one
    // call; calib = MyCalibrator::calibration().  Fills mvKeys, mvKeysUn, mDescriptors and bounds = mnMinX, mnMaxX, mnMinY, mnMaxY;
    // returns monoIndex, -1 for an empty image.
    int ExtractMono(const eorb_host::Mat8& image, const std::vector<int>& vLappingArea, const eorb_calib& calib,
                    std::vector<eorb_host::KeyPoint>& mvKeys, std::vector<eorb_host::KeyPoint>& mvKeysUn, eorb_host::Mat8& mDescriptors,
                    float bounds[4]) {
        if (image.empty()) return -1;
        if (!has_calib_ || std::memcmp(&calib_, &calib, sizeof calib) != 0) {
            ctx_.check(eorb_set_calibration(ctx_.get(), &calib));
            calib_ = calib; has_calib_ = true;
        }
        mvKeys.assign(cap_, eorb_host::KeyPoint{}); mvKeysUn.assign(cap_, eorb_host::KeyPoint{});
        eorb_host::Mat8 d(cap_, 32);
        int n = 0, mono = 0;
        ctx_.check(eorb_frame_mono(ctx_.get(), image.ptr(), image.cols, image.rows, image.cols, vLappingArea[0], vLappingArea[1], 1,
                                   mvKeys.data(), mvKeysUn.data(), d.ptr(), nullptr, cap_, &n, &mono, bounds));
        mvKeys.resize(n); mvKeysUn.resize(n);
        mDescriptors = eorb_host::Mat8(n, 32);
        if (n) std::memcpy(mDescriptors.ptr(), d.ptr(), (size_t)n * 32);
        return mono;
    }
    int GetLevels() const { return p_.nlevels; }
    float GetScaleFactor() const { return p_.scaleFactor; }
    std::vector<float> GetScaleFactors() const { return mvScaleFactor; }
    std::vector<float> GetInverseScaleFactors() const { return mvInvScaleFactor; }
    int GetNumFeatures() const { return p_.nfeatures; }
    int GetEdgeThreshold() const { return edge_; }
    std::vector<float> mvScaleFactor, mvInvScaleFactor;
    std::vector<int> mnFeaturesPerLevel;
private:
    ORBxParams p_;
    eorb_host::Context ctx_;
    int cap_ = 0, edge_ = 0;
    eorb_calib calib_{}; bool has_calib_ = false;
};

// the part of a Frame the matchers read (undistorted keypoints, descriptors, image bounds)
struct FrameView {
    const std::vector<eorb_host::KeyPoint>* kps; const eorb_host::Mat8* desc; eorb_grid_bounds gb;
    FrameView(const std::vector<eorb_host::KeyPoint>& k, const eorb_host::Mat8& d, int W, int H) : kps(&k), desc(&d) {
        gb.minX = 0.f; gb.minY = 0.f; gb.maxX = (float)W; gb.maxY = (float)H;        // Frame.cc:862-866
        gb.invW = 64.f / (gb.maxX - gb.minX); gb.invH = 48.f / (gb.maxY - gb.minY);  // Frame.cc:362-363
    }
    int numAllKPts() const { return (int)kps->size(); }
};

// the pose-dependent part of a Frame that Frame::isInFrustum reads (mRcw, mtcw, mOw, mpCamera, the image bounds, mbf and the ORB
// scale tables): an eorb_view that owns its tables.  The right camera of a two-camera frame is a second FramePose with
// Rrl*mRcw, Rrl*mtcw + trl and mRwc*tlr + mOw (Frame.cc:1257-1263).
struct FramePose {
    eorb_view v{};
    std::vector<float> scaleFactors;
    FramePose(const float Rcw[9], const float tcw[3], const float Ow[3], const eorb_camera& cam, const eorb_grid_bounds& gb, float mbf,
              const std::vector<float>& mvScaleFactor, float logScaleFactor) : scaleFactors(mvScaleFactor) {
        std::memcpy(v.R, Rcw, sizeof(v.R)); std::memcpy(v.t, tcw, sizeof(v.t)); std::memcpy(v.Ow, Ow, sizeof(v.Ow));
        v.cam = cam; v.minX = gb.minX; v.maxX = gb.maxX; v.minY = gb.minY; v.maxY = gb.maxY; v.mbf = mbf;
        v.nlevels = (int)scaleFactors.size(); v.log_scale = logScaleFactor; v.scale_factors = scaleFactors.data();
    }
    FramePose(const FramePose& o) : v(o.v), scaleFactors(o.scaleFactors) { v.scale_factors = scaleFactors.data(); }
    FramePose& operator=(const FramePose&) = delete;
};

// the local map points as Tracking::SearchLocalPoints reads them (Tracking.cc:2390-2408), one entry per MapPoint*: GetWorldPos,
// GetNormal, mfMinDistance / mfMaxDistance, skip = isBad() or already matched in this frame, GetDescriptor, Observations() > 0
struct MapPointsView {
    std::vector<float> worldPos, normal, minDistance, maxDistance;
    std::vector<uint8_t> skip, observed;
    eorb_host::Mat8 descriptors;
    int size() const { return (int)minDistance.size(); }
};

// what Frame::isInFrustum leaves in the map points: mbTrackInView, mTrackProjX/Y, mTrackProjXR, mnTrackScaleLevel, mTrackViewCos,
// mTrackDepth (+ the scale factor of the level and the reject reason of include/eorb_fe.h)
struct TrackedPoints {
    std::vector<uint8_t> inView, reason;
    std::vector<float> projXY, projXR, viewCos, depth, levelScale;
    std::vector<int> level;
    eorb_frustum_out bind(size_t M) {
        inView.assign(M, 0); reason.assign(M, 0); projXY.assign(2 * M, -1.f); projXR.assign(M, 0.f); viewCos.assign(M, 0.f);
        depth.assign(M, 0.f); levelScale.assign(M, 0.f); level.assign(M, -1);
        return eorb_frustum_out{inView.data(), projXY.data(), projXR.data(), level.data(), viewCos.data(), depth.data(), levelScale.data(), reason.data()};
    }
};

// Frame::isInFrustum(pMP, viewingCosLimit) over every local map point (Frame.cc:548-625; two cameras: right != nullptr, :626-636,
// trackedRight receives the *R members).  Returns the number of points in view (nToMatch).
inline int isInFrustum(const FramePose& F, const MapPointsView& mps, float viewingCosLimit, TrackedPoints& tracked,
                       const FramePose* right = nullptr, TrackedPoints* trackedRight = nullptr) {
    auto& c = eorb_host::thread_context();
    const int M = mps.size();
    eorb_view views[2] = {F.v, right ? right->v : F.v};
    eorb_frustum_out out[2] = {tracked.bind((size_t)M), (right && trackedRight) ? trackedRight->bind((size_t)M) : eorb_frustum_out{}};
    int n = 0;
    c.check(eorb_project_frustum(c.get(), views, right ? 2 : 1, M, mps.worldPos.data(), mps.normal.data(), mps.minDistance.data(),
                                 mps.maxDistance.data(), mps.skip.empty() ? nullptr : mps.skip.data(), nullptr, viewingCosLimit, out, &n));
    return n;
}

class ORBmatcher {             // include/ORBmatcher.h:40-116
public:
    // Tracking::SearchLocalPoints (Tracking.cc:2390-2430) in one call: isInFrustum over the local map points, then
    // SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) (:44-219).  frameMP in/out as eorb_search_by_projection_map;
    // uRight = F.mvuRight for a rectified-stereo / RGB-D frame.  tracked: for IncreaseVisible and mmProjectPoints; *nToMatch = points in view.
    int SearchLocalPoints(const FrameView& F, const FramePose& pose, const MapPointsView& mps, std::vector<int>& frameMP, float th,
                          bool bFarPoints, float thFarPoints, TrackedPoints& tracked, int* nToMatch = nullptr,
                          const std::vector<float>* uRight = nullptr, float viewingCosLimit = 0.5f) {
        auto& c = eorb_host::thread_context();
        const int M = mps.size();
        const eorb_frustum_out out = tracked.bind((size_t)M);
        int nm = 0, nv = 0;
        c.check(eorb_search_local_points(c.get(), F.kps->data(), F.numAllKPts(), F.desc->ptr(), F.desc->cols, nullptr, &pose.v, M,
                                         mps.worldPos.data(), mps.normal.data(), mps.minDistance.data(), mps.maxDistance.data(),
                                         mps.skip.empty() ? nullptr : mps.skip.data(), nullptr, viewingCosLimit, mps.descriptors.ptr(),
                                         mps.observed.data(), &F.gb, frameMP.data(), th, mfNNratio, uRight ? uRight->data() : nullptr,
                                         bFarPoints, thFarPoints, &out, &nv, &nm));
        if (nToMatch) *nToMatch = nv;
        return nm;
    }
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
    explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    // vbPrevMatched: (x,y) per F1 keypoint, updated in place; vnMatches12 resized to F1.numAllKPts()
    int SearchForInitialization(const FrameView& F1, const FrameView& F2, std::vector<float>& vbPrevMatched,
                                std::vector<int>& vnMatches12, int windowSize = 10) {
        auto& c = eorb_host::thread_context();
        vnMatches12.assign(F1.numAllKPts(), -1);
        int nm = 0;
        c.check(eorb_search_for_initialization(c.get(), F1.kps->data(), F1.numAllKPts(), F1.desc->ptr(), F1.desc->cols, nullptr,
                                               F2.kps->data(), F2.numAllKPts(), F2.desc->ptr(), F2.desc->cols, nullptr, &F2.gb,
                                               vbPrevMatched.data(), vnMatches12.data(), windowSize, mfNNratio,
                                               mbCheckOrientation, &nm));
        return nm;
    }
    // DBoW2::FeatureVector as CSR (nodes ascending, node_off, idx) -- what ORBVocabulary::transform returns below
    struct FeatureVector { std::vector<uint32_t> nodes; std::vector<int32_t> off{0}, idx; };
    // SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (:276-478): match_f[j] = KeyFrame feature whose map point goes to F's j
    int SearchByBoW(const FrameView& KF, const std::vector<uint8_t>& kfHasMP, const FeatureVector& kfFV, const FrameView& F,
                    const FeatureVector& fFV, std::vector<int>& match_f) {
        auto& c = eorb_host::thread_context();
        match_f.assign(F.numAllKPts(), -1); int nm = 0;
        c.check(eorb_search_by_bow(c.get(), KF.kps->data(), KF.numAllKPts(), KF.desc->ptr(), kfHasMP.data(), kfFV.nodes.data(),
                                   kfFV.off.data(), kfFV.idx.data(), (int)kfFV.nodes.size(), F.kps->data(), F.numAllKPts(), F.desc->ptr(),
                                   fFV.nodes.data(), fFV.off.data(), fFV.idx.data(), (int)fFV.nodes.size(), match_f.data(),
                                   mfNNratio, mbCheckOrientation, &nm));
        return nm;
    }
    // the two-camera frame (numKPtsLeft() != -1): F holds Nleft left keypoints, then the right ones (:276-478)
    int SearchByBoW(const FrameView& KF, const std::vector<uint8_t>& kfHasMP, const FeatureVector& kfFV, const FrameView& F, int Nleft,
                    const FeatureVector& fFV, std::vector<int>& match_f) {
        auto& c = eorb_host::thread_context();
        match_f.assign(F.numAllKPts(), -1); int nm = 0;
        c.check(eorb_search_by_bow_fisheye(c.get(), KF.kps->data(), KF.numAllKPts(), KF.desc->ptr(), kfHasMP.data(), kfFV.nodes.data(),
                                           kfFV.off.data(), kfFV.idx.data(), (int)kfFV.nodes.size(), F.kps->data(), F.numAllKPts(), Nleft,
                                           F.desc->ptr(), fFV.nodes.data(), fFV.off.data(), fFV.idx.data(), (int)fFV.nodes.size(),
                                           match_f.data(), mfNNratio, mbCheckOrientation, &nm));
        return nm;
    }
    // what Frame::isInFrustum leaves in a map point for one camera (mbTrackInView[R], mTrackProjX[R]/Y[R], mnTrackScaleLevel[R],
    // mTrackViewCos[R]) plus getORBScaleFactor(level), per map point
    struct TrackView { std::vector<uint8_t> inView; std::vector<float> projXY, viewCos, levelScale; std::vector<int> level; };
    // SearchByProjection(Frame& F, const vector<MapPoint*>&, th) on a two-camera frame (:44-219): F = Nleft left then right keypoints,
    // l2r / r2l = mvLeftToRightMatch / mvRightToLeftMatch, frameMP in/out as eorb_search_by_projection_map_fisheye
    int SearchByProjection(const FrameView& F, int Nleft, const std::vector<int>& l2r, const std::vector<int>& r2l, const TrackView& left,
                           const TrackView& right, const eorb_host::Mat8& mpDesc, const std::vector<uint8_t>& mpObs,
                           std::vector<int>& frameMP, float th) {
        auto& c = eorb_host::thread_context();
        int nm = 0;
        c.check(eorb_search_by_projection_map_fisheye(c.get(), F.kps->data(), Nleft, F.numAllKPts() - Nleft, F.desc->ptr(), F.desc->cols,
                                                      l2r.data(), r2l.data(), (int)mpObs.size(), left.inView.data(), left.projXY.data(),
                                                      left.level.data(), left.viewCos.data(), left.levelScale.data(), right.inView.data(),
                                                      right.projXY.data(), right.level.data(), right.viewCos.data(), right.levelScale.data(),
                                                      mpDesc.ptr(), mpObs.data(), &F.gb, frameMP.data(), th, mfNNratio, &nm));
        return nm;
    }
    // SearchByProjection(CurrentFrame, LastFrame, th, bMono) on a two-camera frame (:1969-2187): queries = every LastFrame point (its
    // keypoints in index order), uv / uvR = left / right projections, mode 0 / 1 (bForward) / 2 (bBackward); curMP in/out
    int SearchByProjection(const FrameView& Cur, int Nleft, const std::vector<eorb_host::KeyPoint>& lastKps, const std::vector<uint8_t>& valid,
                           const std::vector<float>& uv, const std::vector<float>& uvR, const eorb_host::Mat8& mpDesc,
                           const std::vector<uint8_t>& mpObs, const std::vector<float>& levelScale, std::vector<int>& curMP, float th,
                           int mode) {
        auto& c = eorb_host::thread_context();
        int nm = 0;
        c.check(eorb_search_by_projection_last_fisheye(c.get(), Cur.kps->data(), Nleft, Cur.numAllKPts() - Nleft, Cur.desc->ptr(),
                                                       Cur.desc->cols, lastKps.data(), (int)lastKps.size(), valid.data(), uv.data(),
                                                       uvR.data(), mpDesc.ptr(), mpObs.data(), levelScale.data(), &Cur.gb, curMP.data(),
                                                       th, mode, mbCheckOrientation, &nm));
        return nm;
    }
    // SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (:833-973)
    int SearchByBoW(const FrameView& KF1, const std::vector<uint8_t>& hasMP1, const FeatureVector& FV1, const FrameView& KF2,
                    const std::vector<uint8_t>& hasMP2, const FeatureVector& FV2, std::vector<int>& match12, bool) {
        auto& c = eorb_host::thread_context();
        match12.assign(KF1.numAllKPts(), -1); int nm = 0;
        c.check(eorb_search_by_bow_kf(c.get(), KF1.kps->data(), KF1.numAllKPts(), KF1.desc->ptr(), hasMP1.data(), FV1.nodes.data(),
                                      FV1.off.data(), FV1.idx.data(), (int)FV1.nodes.size(), KF2.kps->data(), KF2.numAllKPts(),
                                      KF2.desc->ptr(), hasMP2.data(), FV2.nodes.data(), FV2.off.data(), FV2.idx.data(),
                                      (int)FV2.nodes.size(), match12.data(), mfNNratio, mbCheckOrientation, &nm));
        return nm;
    }
    // SearchForTriangulation (:975-1214, mono): ep / F12 / level tables from the caller (see include/eorb_fe.h)
    int SearchForTriangulation(const FrameView& KF1, const std::vector<uint8_t>& elig1, const FeatureVector& FV1, const FrameView& KF2,
                               const std::vector<uint8_t>& elig2, const FeatureVector& FV2, const float ep[2], const float F12[9],
                               const std::vector<float>& scale2, const std::vector<float>& sigma2_2,
                               std::vector<std::pair<size_t, size_t>>& vMatchedPairs, bool bCoarse = false) {
        auto& c = eorb_host::thread_context();
        std::vector<int> m12(KF1.numAllKPts(), -1); int nm = 0;
        c.check(eorb_search_for_triangulation(c.get(), KF1.kps->data(), KF1.numAllKPts(), KF1.desc->ptr(), KF1.desc->cols, elig1.data(),
                                              FV1.nodes.data(), FV1.off.data(), FV1.idx.data(), (int)FV1.nodes.size(), KF2.kps->data(),
                                              KF2.numAllKPts(), KF2.desc->ptr(), KF2.desc->cols, elig2.data(), FV2.nodes.data(),
                                              FV2.off.data(), FV2.idx.data(), (int)FV2.nodes.size(), ep, F12, scale2.data(),
                                              sigma2_2.data(), (int)scale2.size(), bCoarse, mbCheckOrientation, m12.data(), &nm));
        vMatchedPairs.clear();
        for (size_t i = 0; i < m12.size(); i++) if (m12[i] >= 0) vMatchedPairs.emplace_back(i, (size_t)m12[i]);     // :1203-1211
        return nm;
    }
    // SearchForTriangulation (:975-1214) with a KannalaBrandt8 pCamera1: nLeft = numAllKPtsLeft() of each keyframe (-1: monocular,
    // Rt[0..11] = R12 | t12; >= 0: two cameras, Rt = ll, lr, rl, rr), cams = {mpCamera, mpCamera2} (see include/eorb_fe.h)
    int SearchForTriangulation(const FrameView& KF1, int nLeft1, const std::vector<uint8_t>& elig1, const FeatureVector& FV1,
                               const FrameView& KF2, int nLeft2, const std::vector<uint8_t>& elig2, const FeatureVector& FV2,
                               const eorb_camera cams1[2], const eorb_camera cams2[2], const float Rt[48], const float ep[2],
                               const std::vector<float>& scale2, const std::vector<float>& sigma2_1, const std::vector<float>& sigma2_2,
                               std::vector<std::pair<size_t, size_t>>& vMatchedPairs, bool bCoarse = false) {
        auto& c = eorb_host::thread_context();
        std::vector<int> m12(KF1.numAllKPts(), -1); int nm = 0;
        c.check(eorb_search_for_triangulation_kb8(c.get(), KF1.kps->data(), KF1.numAllKPts(), nLeft1, KF1.desc->ptr(), KF1.desc->cols,
                                                  elig1.data(), FV1.nodes.data(), FV1.off.data(), FV1.idx.data(), (int)FV1.nodes.size(),
                                                  KF2.kps->data(), KF2.numAllKPts(), nLeft2, KF2.desc->ptr(), KF2.desc->cols, elig2.data(),
                                                  FV2.nodes.data(), FV2.off.data(), FV2.idx.data(), (int)FV2.nodes.size(), cams1, cams2,
                                                  Rt, ep, scale2.data(), sigma2_1.data(), sigma2_2.data(), (int)sigma2_2.size(), bCoarse,
                                                  mbCheckOrientation, m12.data(), &nm));
        vMatchedPairs.clear();
        for (size_t i = 0; i < m12.size(); i++) if (m12[i] >= 0) vMatchedPairs.emplace_back(i, (size_t)m12[i]);     // :1203-1211
        return nm;
    }
    // ---- the same matchers over K keyframes per call (eorb_kf_set and the *_keyframes entry points of include/eorb_fe.h) ----
    // row k of a K x n1 match table -> vMatchedPairs of keyframe k (:1203-1211)
    static void PairsPerKeyFrame(const std::vector<int>& m12, int K, size_t n1, std::vector<std::vector<std::pair<size_t, size_t>>>& vv) {
        vv.assign(K, std::vector<std::pair<size_t, size_t>>());
        for (int k = 0; k < K; k++)
            for (size_t i = 0; i < n1; i++) if (m12[k * n1 + i] >= 0) vv[k].emplace_back(i, (size_t)m12[k * n1 + i]);
    }
    // one keyframe of the list: its view, the flag byte per feature (elig2 / kfHasMP / hasMP2 of the single overloads) and its FeatureVector
    struct KeyFrameNodes { const FrameView* KF; const std::vector<uint8_t>* flag; const FeatureVector* FV; };
    // the list packed into the concatenated arrays an eorb_kf_set points at
    struct KeyFrameSet {
        std::vector<eorb_host::KeyPoint> kps; std::vector<uint8_t> desc, flag; std::vector<int32_t> kfOff{0}, nodeOff{0}, featOff, idx;
        std::vector<uint32_t> nodes; eorb_kf_set set{};
        explicit KeyFrameSet(const std::vector<KeyFrameNodes>& kfs) {
            int stride = 32;
            for (const auto& k : kfs) if (k.KF->numAllKPts() > 0) stride = k.KF->desc->cols;
            for (const auto& k : kfs) {
                const int n = k.KF->numAllKPts();
                if (n > 0 && k.KF->desc->cols != stride) throw eorb_host::Error(EORB_E_ARG, "KeyFrameSet: the keyframes of a set share one descriptor stride");
                kps.insert(kps.end(), k.KF->kps->begin(), k.KF->kps->end());
                if (n > 0) desc.insert(desc.end(), k.KF->desc->ptr(), k.KF->desc->ptr() + (size_t)n * stride);
                flag.insert(flag.end(), k.flag->begin(), k.flag->end());
                kfOff.push_back((int32_t)kps.size());
                nodes.insert(nodes.end(), k.FV->nodes.begin(), k.FV->nodes.end());
                nodeOff.push_back((int32_t)nodes.size());
                if (k.FV->off.empty()) featOff.push_back(0); else featOff.insert(featOff.end(), k.FV->off.begin(), k.FV->off.end());
                idx.insert(idx.end(), k.FV->idx.begin(), k.FV->idx.end());
            }
            set.K = (int)kfs.size(); set.kps = kps.data(); set.desc = desc.data(); set.stride = stride; set.flag = flag.data();
            set.kf_off = kfOff.data(); set.nodes = nodes.data(); set.node_off = nodeOff.data(); set.feat_off = featOff.data(); set.idx = idx.data();
        }
        KeyFrameSet(const KeyFrameSet&) = delete;
        KeyFrameSet& operator=(const KeyFrameSet&) = delete;
    };
    // SearchForTriangulation(pKF1, pKF2_k, F12_k, ...) over the neighbours of LocalMapping::CreateNewMapPoints (LocalMapping.cc:467-511):
    // ep[2K], F12[9K]; vvMatchedPairs[k] = the pairs of neighbour k, searched with elig1 as it stands before the loop.  The caller walks k
    // in the reference's order and drops a pair whose idx1 got a map point from an earlier neighbour (the recipe in include/eorb_fe.h).
    std::vector<int> SearchForTriangulation(const FrameView& KF1, const std::vector<uint8_t>& elig1, const FeatureVector& FV1,
                                            const std::vector<KeyFrameNodes>& KFs, const std::vector<float>& ep, const std::vector<float>& F12,
                                            const std::vector<float>& scale2, const std::vector<float>& sigma2_2,
                                            std::vector<std::vector<std::pair<size_t, size_t>>>& vvMatchedPairs, bool bCoarse = false) {
        auto& c = eorb_host::thread_context();
        const KeyFrameSet S(KFs);
        const size_t n1 = (size_t)KF1.numAllKPts();
        std::vector<int> m12(S.set.K * n1, -1), nm(S.set.K, 0);
        if (ep.size() != 2 * (size_t)S.set.K || F12.size() != 9 * (size_t)S.set.K) throw eorb_host::Error(EORB_E_ARG, "SearchForTriangulation: ep / F12 per keyframe");
        c.check(eorb_search_for_triangulation_keyframes(c.get(), KF1.kps->data(), (int)n1, KF1.desc->ptr(), KF1.desc->cols, elig1.data(),
                                                        FV1.nodes.data(), FV1.off.data(), FV1.idx.data(), (int)FV1.nodes.size(), &S.set, ep.data(),
                                                        F12.data(), scale2.data(), sigma2_2.data(), (int)scale2.size(), bCoarse,
                                                        mbCheckOrientation, m12.data(), nm.data()));
        PairsPerKeyFrame(m12, S.set.K, n1, vvMatchedPairs);
        return nm;
    }
    // the same with a KannalaBrandt8 pCamera1: nLeft2[K]; Rt = 12 floats (monocular) or 48 (two cameras) per neighbour
    std::vector<int> SearchForTriangulation(const FrameView& KF1, int nLeft1, const std::vector<uint8_t>& elig1, const FeatureVector& FV1,
                                            const std::vector<KeyFrameNodes>& KFs, const std::vector<int>& nLeft2, const eorb_camera cams1[2],
                                            const eorb_camera cams2[2], const std::vector<float>& Rt, const std::vector<float>& ep,
                                            const std::vector<float>& scale2, const std::vector<float>& sigma2_1, const std::vector<float>& sigma2_2,
                                            std::vector<std::vector<std::pair<size_t, size_t>>>& vvMatchedPairs, bool bCoarse = false) {
        auto& c = eorb_host::thread_context();
        const KeyFrameSet S(KFs);
        const size_t n1 = (size_t)KF1.numAllKPts(), K = (size_t)S.set.K;
        std::vector<int> m12(K * n1, -1), nm(K, 0);
        if (nLeft2.size() != K || ep.size() != 2 * K || Rt.size() != (nLeft1 >= 0 ? 48 : 12) * K)
            throw eorb_host::Error(EORB_E_ARG, "SearchForTriangulation: nLeft2 / ep / Rt per keyframe");
        c.check(eorb_search_for_triangulation_kb8_keyframes(c.get(), KF1.kps->data(), (int)n1, nLeft1, KF1.desc->ptr(), KF1.desc->cols, elig1.data(),
                                                            FV1.nodes.data(), FV1.off.data(), FV1.idx.data(), (int)FV1.nodes.size(), &S.set,
                                                            nLeft2.data(), cams1, cams2, Rt.data(), ep.data(), scale2.data(), sigma2_1.data(),
                                                            sigma2_2.data(), (int)sigma2_2.size(), bCoarse, mbCheckOrientation, m12.data(), nm.data()));
        PairsPerKeyFrame(m12, S.set.K, n1, vvMatchedPairs);
        return nm;
    }
    // SearchByBoW(pKF_k, F, vvpMapPointMatches[k]) over the candidates of Tracking::Relocalization (Tracking.cc:2674-2689):
    // vvMatchF[k][j] = feature of keyframe k whose map point goes to F's j, or -1
    std::vector<int> SearchByBoW(const std::vector<KeyFrameNodes>& KFs, const FrameView& F, const FeatureVector& fFV,
                                 std::vector<std::vector<int>>& vvMatchF) {
        auto& c = eorb_host::thread_context();
        const KeyFrameSet S(KFs);
        const size_t n = (size_t)F.numAllKPts();
        std::vector<int> m(S.set.K * n, -1), nm(S.set.K, 0);
        c.check(eorb_search_by_bow_keyframes(c.get(), &S.set, F.kps->data(), (int)n, F.desc->ptr(), fFV.nodes.data(), fFV.off.data(), fFV.idx.data(),
                                             (int)fFV.nodes.size(), m.data(), mfNNratio, mbCheckOrientation, nm.data()));
        vvMatchF.assign(S.set.K, std::vector<int>());
        for (int k = 0; k < S.set.K; k++) vvMatchF[k].assign(m.begin() + k * n, m.begin() + (k + 1) * n);
        return nm;
    }
    // SearchByBoW(pKF1, pKF2_k, vvpMatchedMPs[k]) over a candidate and its covisibles (LoopClosing.cc:628-648): vvMatches12[k][i] = index in
    // keyframe k, or -1
    std::vector<int> SearchByBoW(const FrameView& KF1, const std::vector<uint8_t>& hasMP1, const FeatureVector& FV1,
                                 const std::vector<KeyFrameNodes>& KFs, std::vector<std::vector<int>>& vvMatches12) {
        auto& c = eorb_host::thread_context();
        const KeyFrameSet S(KFs);
        const size_t n = (size_t)KF1.numAllKPts();
        std::vector<int> m(S.set.K * n, -1), nm(S.set.K, 0);
        c.check(eorb_search_by_bow_kf_keyframes(c.get(), KF1.kps->data(), (int)n, KF1.desc->ptr(), hasMP1.data(), FV1.nodes.data(), FV1.off.data(),
                                                FV1.idx.data(), (int)FV1.nodes.size(), &S.set, m.data(), mfNNratio, mbCheckOrientation, nm.data()));
        vvMatches12.assign(S.set.K, std::vector<int>());
        for (int k = 0; k < S.set.K; k++) vvMatches12[k].assign(m.begin() + k * n, m.begin() + (k + 1) * n);
        return nm;
    }
    // Fuse(pKF, vpMapPoints, th, bRight = true) (:1407-1578) on a two-camera KeyFrame: the search core over the right block.
    // KFRight = the right keypoints and descriptors (desc + Nleft * stride) with the right grid's bounds; uv / radius / level from
    // the map points projected by mpCamera2 (:1463-1513).  The returned indices are right-camera indices plus nLeft (:1567).
    // The reference reads mvuRight[idx] with the right-camera index (:1541): -1 below Nleft (Frame.cc:1221) and past the vector
    // otherwise; this treats every right keypoint as monocular (the 5.99 gate).
    void FuseRightMatch(const FrameView& KFRight, int nLeft, const std::vector<uint8_t>& valid, const std::vector<float>& uv,
                        const std::vector<float>& radius, const std::vector<int>& level, const eorb_host::Mat8& mpDesc,
                        const std::vector<float>& invSigma2, std::vector<int>& bestIdx, std::vector<int>& bestDist) {
        KeyFrameRadiusMatch(KFRight, valid, uv, radius, level, mpDesc, &invSigma2, nullptr, 0.f, bestIdx, bestDist);
        for (int& i : bestIdx) if (i >= 0) i += nLeft;
    }
    // search core of Fuse / SearchBySim3 / SearchByProjection(KF, Scw): see eorb_kf_radius_match
    void KeyFrameRadiusMatch(const FrameView& KF, const std::vector<uint8_t>& valid, const std::vector<float>& uv,
                             const std::vector<float>& radius, const std::vector<int>& level, const eorb_host::Mat8& mpDesc,
                             const std::vector<float>* invSigma2, std::vector<uint8_t>* taken, float acceptThr,
                             std::vector<int>& bestIdx, std::vector<int>& bestDist) {
        auto& c = eorb_host::thread_context();
        const int M = (int)valid.size();
        bestIdx.assign(M, -1); bestDist.assign(M, 256);
        c.check(eorb_kf_radius_match(c.get(), KF.kps->data(), KF.numAllKPts(), KF.desc->ptr(), KF.desc->cols, &KF.gb, M, valid.data(),
                                     uv.data(), radius.data(), level.data(), mpDesc.ptr(), invSigma2 ? invSigma2->data() : nullptr,
                                     invSigma2 ? (int)invSigma2->size() : 0, taken ? taken->data() : nullptr, acceptThr,
                                     bestIdx.data(), bestDist.data()));
    }
    // Fuse on a rectified-stereo KeyFrame (:1541-1553): uright = pKF->mvuRight, qUr[m] = u - bf * invz of map point m
    void FuseStereoMatch(const FrameView& KF, const std::vector<uint8_t>& valid, const std::vector<float>& uv,
                         const std::vector<float>& radius, const std::vector<int>& level, const eorb_host::Mat8& mpDesc,
                         const std::vector<float>& invSigma2, const std::vector<float>& uright, const std::vector<float>& qUr,
                         std::vector<int>& bestIdx, std::vector<int>& bestDist) {
        auto& c = eorb_host::thread_context();
        const int M = (int)valid.size();
        bestIdx.assign(M, -1); bestDist.assign(M, 256);
        c.check(eorb_kf_radius_match_stereo(c.get(), KF.kps->data(), KF.numAllKPts(), KF.desc->ptr(), KF.desc->cols, &KF.gb, M, valid.data(),
                                            uv.data(), radius.data(), level.data(), mpDesc.ptr(), invSigma2.data(), (int)invSigma2.size(),
                                            uright.data(), qUr.data(), bestIdx.data(), bestDist.data()));
    }
    // ---- the KeyFrame-side matchers with the projection on the device (see include/eorb_fe.h) ----
    // the map points handed to Fuse / SearchByProjection(pKF, Scw): GetWorldPos, GetNormal, mfMinDistance, mfMaxDistance, 3 / 3 / 1 / 1
    // floats per point, and GetDescriptor; skip (optional): !pMP, isBad(), IsInKeyFrame(pKF) / spAlreadyFound
    struct MapPoints { std::vector<float> pos, normal, minDist, maxDist; eorb_host::Mat8 desc; std::vector<uint8_t> skip;
                       int size() const { return (int)minDist.size(); } };
    // what the projection leaves per (keyframe, map point): eorb_kfside_out
    struct SideProjection { std::vector<uint8_t> valid, reason; std::vector<float> uv, radius, qUr, dist3D; std::vector<int> level;
        eorb_kfside_out bind(size_t n) {
            valid.assign(n, 0); reason.assign(n, 0); uv.assign(2 * n, 0.f); radius.assign(n, 0.f); qUr.assign(n, 0.f); dist3D.assign(n, 0.f);
            level.assign(n, 0);
            return eorb_kfside_out{valid.data(), uv.data(), radius.data(), level.data(), qUr.data(), dist3D.data(), reason.data()};
        } };
    // the projection of Fuse / SearchByProjection(pKF, Scw) alone (:1463-1513, :1650-1690, :511-550)
    void ProjectKeyFrameSide(const eorb_view& view, const MapPoints& P, float th, SideProjection& out) {
        auto& c = eorb_host::thread_context();
        const eorb_kfside_out o = out.bind((size_t)P.size());
        c.check(eorb_project_keyframe_side(c.get(), &view, P.size(), P.pos.data(), P.normal.data(), P.minDist.data(), P.maxDist.data(),
                                           P.skip.empty() ? nullptr : P.skip.data(), th, &o));
    }
    // Fuse(pKF, vpMapPoints, th) up to the map update (:1439-1578); invSigma2 == nullptr: Fuse(pKF, Scw, ...) (:1642-1720); uright =
    // pKF->mvuRight or nullptr.  The caller thresholds bestDist with TH_LOW and performs Replace / AddObservation in order.
    void Fuse(const FrameView& KF, const eorb_view& view, const MapPoints& P, const std::vector<float>* invSigma2,
              const std::vector<float>* uright, float th, std::vector<int>& bestIdx, std::vector<int>& bestDist, SideProjection* proj = nullptr) {
        auto& c = eorb_host::thread_context();
        const int M = P.size();
        bestIdx.assign(M, -1); bestDist.assign(M, 256);
        eorb_kfside_out o{};
        if (proj) o = proj->bind((size_t)M);
        c.check(eorb_fuse_pose(c.get(), KF.kps->data(), KF.numAllKPts(), KF.desc->ptr(), KF.desc->cols ? KF.desc->cols : 32, &KF.gb, &view, M,
                               P.pos.data(), P.normal.data(), P.minDist.data(), P.maxDist.data(), P.skip.empty() ? nullptr : P.skip.data(),
                               P.desc.ptr(), invSigma2 ? invSigma2->data() : nullptr, uright ? uright->data() : nullptr, th, bestIdx.data(),
                               bestDist.data(), proj ? &o : nullptr));
    }
    // SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) up to the assignment of vpMatched (:487-590): taken in / out
    void SearchByProjection(const FrameView& KF, const eorb_view& view, const MapPoints& P, std::vector<uint8_t>& taken, float th,
                            float ratioHamming, std::vector<int>& bestIdx, std::vector<int>& bestDist) {
        auto& c = eorb_host::thread_context();
        const int M = P.size();
        bestIdx.assign(M, -1); bestDist.assign(M, 256);
        c.check(eorb_search_by_projection_kf_scw(c.get(), KF.kps->data(), KF.numAllKPts(), KF.desc->ptr(), KF.desc->cols ? KF.desc->cols : 32,
                                                 &KF.gb, &view, M, P.pos.data(), P.normal.data(), P.minDist.data(), P.maxDist.data(),
                                                 P.skip.empty() ? nullptr : P.skip.data(), P.desc.ptr(), th, taken.data(),
                                                 (float)TH_LOW * ratioHamming, bestIdx.data(), bestDist.data(), nullptr));
    }
    // SearchBySim3 (:1743-1967) in one call: P1 / P2 = the map points of the keyframes' keypoint slots (skip: none, bad or already
    // matched), sR12 / t12 / sR21 / t21 as at :1760-1762.  match12[i1] = index in KF2 or -1; returns nFound
    int SearchBySim3(const FrameView& KF1, const eorb_view& view1, const MapPoints& P1, const FrameView& KF2, const eorb_view& view2,
                     const MapPoints& P2, const float sR12[9], const float t12[3], const float sR21[9], const float t21[3], float th,
                     std::vector<int>& match12) {
        auto& c = eorb_host::thread_context();
        match12.assign(KF1.numAllKPts(), -1); int nf = 0;
        c.check(eorb_search_by_sim3(c.get(), KF1.kps->data(), KF1.numAllKPts(), KF1.desc->ptr(), KF1.desc->cols ? KF1.desc->cols : 32, &KF1.gb,
                                    &view1, P1.pos.data(), P1.minDist.data(), P1.maxDist.data(), P1.desc.ptr(),
                                    P1.skip.empty() ? nullptr : P1.skip.data(), KF2.kps->data(), KF2.numAllKPts(), KF2.desc->ptr(),
                                    KF2.desc->cols ? KF2.desc->cols : 32, &KF2.gb, &view2, P2.pos.data(), P2.minDist.data(), P2.maxDist.data(),
                                    P2.desc.ptr(), P2.skip.empty() ? nullptr : P2.skip.data(), sR12, t12, sR21, t21, th, TH_HIGH,
                                    match12.data(), &nf, nullptr, nullptr));
        return nf;
    }
    // Fuse of P into K keyframes at once (SearchInNeighbors, SearchAndFuse): KFs = the keyframes concatenated (keypoints, descriptors,
    // kfOff[K + 1]), P.skip = K x M or empty.  bestIdx / bestDist: K x M, applied by the caller keyframe by keyframe with the re-tests
    // that include/eorb_fe.h lists.
    void FuseKeyFrames(const std::vector<eorb_view>& views, const std::vector<eorb_grid_bounds>& gbs, const std::vector<eorb_host::KeyPoint>& kps,
                       const eorb_host::Mat8& desc, const std::vector<int32_t>& kfOff, const MapPoints& P, const std::vector<float>* invSigma2,
                       const std::vector<float>* uright, float th, std::vector<int>& bestIdx, std::vector<int>& bestDist) {
        auto& c = eorb_host::thread_context();
        const int K = (int)views.size(), M = P.size();
        bestIdx.assign((size_t)K * M, -1); bestDist.assign((size_t)K * M, 256);
        c.check(eorb_fuse_keyframes(c.get(), views.data(), gbs.data(), K, kps.data(), desc.ptr(), desc.cols ? desc.cols : 32,
                                    uright ? uright->data() : nullptr, kfOff.data(), M, P.pos.data(), P.normal.data(), P.minDist.data(),
                                    P.maxDist.data(), P.desc.ptr(), P.skip.empty() ? nullptr : P.skip.data(),
                                    invSigma2 ? invSigma2->data() : nullptr, th, bestIdx.data(), bestDist.data(), nullptr));
    }
    // ---- the same on a MixedKeyFrame: EORB_SLAM::MixedMatcher's KeyFrame-side forms (see the *_mixed entry points of include/eorb_fe.h) ----
    // what a MixedKeyFrame adds: kpIsOrb[i] = pKF->isORBDescValid(i), kpInvSigma2[i] = pKF->getKPtInvLevelSigma2(i) (empty: no
    // reprojection gate), mpIsOrb[m] = vpMapPoints[m]->isORBMapPoint(); an empty vector means "all ORB" on that side
    struct MixedKinds { std::vector<uint8_t> kpIsOrb; std::vector<float> kpInvSigma2; std::vector<uint8_t> mpIsOrb;
        const uint8_t* kp() const { return kpIsOrb.empty() ? nullptr : kpIsOrb.data(); }
        const float* sigma() const { return kpInvSigma2.empty() ? nullptr : kpInvSigma2.data(); }
        const uint8_t* mp() const { return mpIsOrb.empty() ? nullptr : mpIsOrb.data(); } };
    // search loop of MixedMatcher::Fuse / SearchByProjection(pKF, Scw, ...): KeyFrameRadiusMatch and FuseStereoMatch in one
    void KeyFrameRadiusMatchMixed(const FrameView& KF, const MixedKinds& kinds, const std::vector<uint8_t>& valid, const std::vector<float>& uv,
                                  const std::vector<float>& radius, const std::vector<int>& level, const eorb_host::Mat8& mpDesc,
                                  const std::vector<float>* uright, const std::vector<float>* qUr, std::vector<uint8_t>* taken, float acceptThr,
                                  std::vector<int>& bestIdx, std::vector<int>& bestDist) {
        auto& c = eorb_host::thread_context();
        const int M = (int)valid.size();
        bestIdx.assign(M, -1); bestDist.assign(M, 256);
        c.check(eorb_kf_radius_match_mixed(c.get(), KF.kps->data(), KF.numAllKPts(), KF.desc->ptr(), KF.desc->cols ? KF.desc->cols : 32, &KF.gb,
                                           kinds.kp(), kinds.sigma(), uright ? uright->data() : nullptr, M, valid.data(), uv.data(),
                                           radius.data(), level.data(), mpDesc.ptr(), kinds.mp(), qUr ? qUr->data() : nullptr,
                                           taken ? taken->data() : nullptr, acceptThr, bestIdx.data(), bestDist.data()));
    }
    void ProjectKeyFrameSideMixed(const eorb_view& view, const MapPoints& P, const MixedKinds& kinds, float th, SideProjection& out) {
        auto& c = eorb_host::thread_context();
        const eorb_kfside_out o = out.bind((size_t)P.size());
        c.check(eorb_project_keyframe_side_mixed(c.get(), &view, P.size(), P.pos.data(), P.normal.data(), P.minDist.data(), P.maxDist.data(),
                                                 kinds.mp(), P.skip.empty() ? nullptr : P.skip.data(), th, &o));
    }
    // MixedMatcher::Fuse(pKF, vpMapPoints, th, bRight) up to the map update (src/MixedMatcher.cpp:1575-1758); kinds.kpInvSigma2 empty:
    // MixedMatcher::Fuse(pKF, Scw, ...) (:1799-1921)
    void FuseMixed(const FrameView& KF, const eorb_view& view, const MapPoints& P, const MixedKinds& kinds, const std::vector<float>* uright,
                   float th, std::vector<int>& bestIdx, std::vector<int>& bestDist, SideProjection* proj = nullptr) {
        auto& c = eorb_host::thread_context();
        const int M = P.size();
        bestIdx.assign(M, -1); bestDist.assign(M, 256);
        eorb_kfside_out o{};
        if (proj) o = proj->bind((size_t)M);
        c.check(eorb_fuse_pose_mixed(c.get(), KF.kps->data(), KF.numAllKPts(), KF.desc->ptr(), KF.desc->cols ? KF.desc->cols : 32, &KF.gb,
                                     kinds.kp(), kinds.sigma(), uright ? uright->data() : nullptr, &view, M, P.pos.data(), P.normal.data(),
                                     P.minDist.data(), P.maxDist.data(), kinds.mp(), P.skip.empty() ? nullptr : P.skip.data(), P.desc.ptr(), th,
                                     bestIdx.data(), bestDist.data(), proj ? &o : nullptr));
    }
    // both MixedMatcher::SearchByProjection(pKF, Scw, ...) up to the assignment of vpMatched (:1065-1189, :1191-1324): taken in / out
    void SearchByProjectionMixed(const FrameView& KF, const eorb_view& view, const MapPoints& P, const MixedKinds& kinds,
                                 std::vector<uint8_t>& taken, float th, float ratioHamming, std::vector<int>& bestIdx, std::vector<int>& bestDist) {
        auto& c = eorb_host::thread_context();
        const int M = P.size();
        bestIdx.assign(M, -1); bestDist.assign(M, 256);
        c.check(eorb_search_by_projection_kf_scw_mixed(c.get(), KF.kps->data(), KF.numAllKPts(), KF.desc->ptr(), KF.desc->cols ? KF.desc->cols : 32,
                                                       &KF.gb, kinds.kp(), &view, M, P.pos.data(), P.normal.data(), P.minDist.data(),
                                                       P.maxDist.data(), kinds.mp(), P.skip.empty() ? nullptr : P.skip.data(), P.desc.ptr(), th,
                                                       taken.data(), (float)TH_LOW * ratioHamming, bestIdx.data(), bestDist.data(), nullptr));
    }
    // MixedMatcher::Fuse of P into K MixedKeyFrames at once: FuseKeyFrames with kinds.kpIsOrb / kpInvSigma2 concatenated like kps
    void FuseKeyFramesMixed(const std::vector<eorb_view>& views, const std::vector<eorb_grid_bounds>& gbs,
                            const std::vector<eorb_host::KeyPoint>& kps, const eorb_host::Mat8& desc, const std::vector<int32_t>& kfOff,
                            const MapPoints& P, const MixedKinds& kinds, const std::vector<float>* uright, float th, std::vector<int>& bestIdx,
                            std::vector<int>& bestDist) {
        auto& c = eorb_host::thread_context();
        const int K = (int)views.size(), M = P.size();
        bestIdx.assign((size_t)K * M, -1); bestDist.assign((size_t)K * M, 256);
        c.check(eorb_fuse_keyframes_mixed(c.get(), views.data(), gbs.data(), K, kps.data(), desc.ptr(), desc.cols ? desc.cols : 32, kinds.kp(),
                                          kinds.sigma(), uright ? uright->data() : nullptr, kfOff.data(), M, P.pos.data(), P.normal.data(),
                                          P.minDist.data(), P.maxDist.data(), kinds.mp(), P.desc.ptr(), P.skip.empty() ? nullptr : P.skip.data(),
                                          th, bestIdx.data(), bestDist.data(), nullptr));
    }
protected:
    float mfNNratio; bool mbCheckOrientation;
};

// ORBVocabulary (= DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) resident on the device
class ORBVocabulary {
public:
    // m_nodes flattened after loadFromTextFile: node 0 = root (see eorb_bow_set_vocabulary)
    ORBVocabulary(int L, const std::vector<int32_t>& childOff, const std::vector<int32_t>& childIds, const eorb_host::Mat8& nodeDesc,
                  const std::vector<int32_t>& wordId, const std::vector<double>& weight, int weighting = 0, int norm = 1)
        : weighting_(weighting), norm_(norm) {
        eorb_host::ContextPool::Voc v;
        v.L = L; v.childOff = childOff; v.childIds = childIds; v.wordId = wordId; v.weight = weight;
        v.nodeDesc.assign(nodeDesc.ptr(), nodeDesc.ptr() + (size_t)nodeDesc.rows * nodeDesc.cols);
        eorb_host::ContextPool::instance().set_vocabulary(std::move(v));                    // every context of the process
    }
    // transform(vCurrentDesc, mBowVec, mFeatVec, levelsup) (Frame::ComputeBoW)
    void transform(const eorb_host::Mat8& desc, std::vector<std::pair<uint32_t, double>>& bowVec, ORBmatcher::FeatureVector& featVec,
                   int levelsup = 4) const {
        auto& c = eorb_host::thread_context();
        const int n = desc.rows;
        std::vector<uint32_t> bw(n ? n : 1); std::vector<double> bv(n ? n : 1); int nw = 0, nn = 0;
        featVec.nodes.assign(n ? n : 1, 0); featVec.off.assign(n + 1, 0); featVec.idx.assign(n ? n : 1, 0);
        c.check(eorb_bow_transform(c.get(), desc.ptr(), n, desc.cols ? desc.cols : 32, levelsup, weighting_, norm_, bw.data(), bv.data(),
                                   &nw, featVec.nodes.data(), featVec.off.data(), featVec.idx.data(), &nn, nullptr, nullptr));
        bowVec.clear();
        for (int i = 0; i < nw; i++) bowVec.emplace_back(bw[i], bv[i]);
        featVec.nodes.resize(nn); featVec.off.resize(nn + 1); featVec.idx.resize(featVec.off[nn]);
    }
private:
    int weighting_, norm_;
};

// KeyFrameDatabase (src/KeyFrameDatabase.cc) resident on the device.  Keyframes are named by the slots add() returns; the adapter keeps a
// `slot` member per KeyFrame and a vector<KeyFrame*> by slot.  What needs the KeyFrame itself is mirrored per slot here
// and kept current by the adapter: its map (GetMap, an id), isBad(), Map::IsBad() per map id and GetBestCovisibilityKeyFrames(10) as
// slots.  The object owns one context (the database lives in it) and a mutex in the place of mMutex: any thread may call it.
class KeyFrameDatabase {
public:
    typedef std::vector<std::pair<uint32_t, double>> BowVector;      // DBoW2::BowVector in map order: word ids ascending

    explicit KeyFrameDatabase(int device = 0) : ctx_(device) {}

    // add(pKF) :39-45 -> the keyframe's slot (the lowest free one)
    int add(const BowVector& bow, long mapId) {
        std::lock_guard<std::mutex> lock(mMutex);
        std::vector<uint32_t> w; std::vector<double> v;
        split(bow, w, v);
        const int32_t off[2] = {0, (int32_t)w.size()};
        int32_t slot = -1;
        ctx_.check(eorb_kfdb_add(ctx_.get(), 1, off, w.data(), v.data(), &slot));
        if ((size_t)slot >= map_.size()) { map_.resize(slot + 1, -1); bad_.resize(slot + 1, 0); covis_.resize((size_t)(slot + 1) * EORB_KFDB_COVIS, -1); }
        map_[slot] = mapId; bad_[slot] = 0;
        std::fill(covis_.begin() + (size_t)slot * EORB_KFDB_COVIS, covis_.begin() + (size_t)(slot + 1) * EORB_KFDB_COVIS, -1);
        return slot;
    }
    // erase(pKF) :47-66; the slot also leaves every covisibility row
    void erase(int slot) {
        std::lock_guard<std::mutex> lock(mMutex);
        erase_locked(slot);
    }
    // clear() :68-72
    void clear() {
        std::lock_guard<std::mutex> lock(mMutex);
        ctx_.check(eorb_kfdb_clear(ctx_.get()));
        map_.clear(); bad_.clear(); covis_.clear();
    }
    // clearMap(pMap) :74-98: every keyframe of that map leaves the lists
    void clearMap(long mapId) {
        std::lock_guard<std::mutex> lock(mMutex);
        for (size_t s = 0; s < map_.size(); s++) if (map_[s] == mapId) erase_locked((int)s);
    }
    void SetBadFlag(int slot, bool bad = true) { std::lock_guard<std::mutex> lock(mMutex); bad_.at(slot) = bad ? 1 : 0; }      // KeyFrame::isBad()
    void SetMapBad(long mapId, bool bad = true) {                                                                            // Map::IsBad()
        std::lock_guard<std::mutex> lock(mMutex);
        auto it = std::find(badMaps_.begin(), badMaps_.end(), mapId);
        if (bad && it == badMaps_.end()) badMaps_.push_back(mapId);
        if (!bad && it != badMaps_.end()) badMaps_.erase(it);
    }
    // GetBestCovisibilityKeyFrames(10) of the keyframe in `slot`, as slots in their order (keyframes outside the database: left out or -1)
    void SetBestCovisibility(int slot, const std::vector<int>& neighbours) {
        std::lock_guard<std::mutex> lock(mMutex);
        for (int j = 0; j < EORB_KFDB_COVIS; j++) covis_.at((size_t)slot * EORB_KFDB_COVIS + j) = j < (int)neighbours.size() ? neighbours[j] : -1;
    }

    // DetectRelocalizationCandidates(F, pMap) :783-895 -> the slots of vpRelocCandidates
    std::vector<int> DetectRelocalizationCandidates(const BowVector& bow, long mapId) {
        std::lock_guard<std::mutex> lock(mMutex);
        std::vector<uint32_t> w; std::vector<double> v;
        split(bow, w, v);
        const int cap = (int)map_.size(), m = cap ? cap : 1;
        std::vector<int32_t> slot(m), words(m), best(m); std::vector<float> si(m), acc(m); std::vector<uint8_t> keep(m);
        int nl = 0, ns = 0, mc = 0; float ba = 0.f;
        ctx_.check(eorb_kfdb_detect_reloc(ctx_.get(), (int)w.size(), w.data(), v.data(), covis_.data(), cap, slot.data(), si.data(), words.data(),
                                          acc.data(), best.data(), keep.data(), &nl, &ns, &mc, &ba));
        std::vector<int> vpRelocCandidates;
        std::vector<uint8_t> spAlreadyAddedKF(map_.size(), 0);
        for (int i = 0; i < ns; i++) {                           // :878-892
            if (!keep[i]) continue;
            const int pKFi = best[i];
            if (map_[pKFi] != mapId) continue;
            if (!spAlreadyAddedKF[pKFi]) { vpRelocCandidates.push_back(pKFi); spAlreadyAddedKF[pKFi] = 1; }
        }
        return vpRelocCandidates;
    }

    // DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates) :612-780; connected = pKF->GetConnectedKeyFrames() as slots,
    // mapId = pKF->GetMap()
    void DetectNBestCandidates(const BowVector& bow, long mapId, const std::vector<int>& connected, std::vector<int>& vpLoopCand,
                               std::vector<int>& vpMergeCand, int nNumCandidates) {
        std::lock_guard<std::mutex> lock(mMutex);
        std::vector<uint32_t> w; std::vector<double> v;
        split(bow, w, v);
        const int cap = (int)map_.size(), m = cap ? cap : 1;
        std::vector<uint8_t> exclude(m, 0);
        for (int s : connected) if (s >= 0 && s < cap) exclude[s] = 1;
        std::vector<int32_t> slot(m), words(m), best(m), sbest(m); std::vector<float> si(m), acc(m), sacc(m);
        int nl = 0, ns = 0, mc = 0; float ba = 0.f;
        ctx_.check(eorb_kfdb_detect_nbest(ctx_.get(), (int)w.size(), w.data(), v.data(), exclude.data(), covis_.data(), cap, slot.data(), si.data(),
                                          words.data(), acc.data(), best.data(), sacc.data(), sbest.data(), &nl, &ns, &mc, &ba));
        vpLoopCand.clear(); vpMergeCand.clear();
        std::vector<uint8_t> spAlreadyAddedKF(map_.size(), 0);
        // :731-752.  The reference's while loop `continue`s on a bad keyframe without advancing its iterator and never ends; this mirror
        // skips the bad keyframe and advances.
        for (int i = 0; i < ns && ((int)vpLoopCand.size() < nNumCandidates || (int)vpMergeCand.size() < nNumCandidates); i++) {
            const int pKFi = sbest[i];
            if (bad_[pKFi]) continue;
            if (!spAlreadyAddedKF[pKFi]) {
                if (mapId == map_[pKFi] && (int)vpLoopCand.size() < nNumCandidates) vpLoopCand.push_back(pKFi);
                else if (mapId != map_[pKFi] && (int)vpMergeCand.size() < nNumCandidates &&
                         std::find(badMaps_.begin(), badMaps_.end(), map_[pKFi]) == badMaps_.end()) vpMergeCand.push_back(pKFi);
                spAlreadyAddedKF[pKFi] = 1;
            }
        }
    }

private:
    static void split(const BowVector& bow, std::vector<uint32_t>& w, std::vector<double>& v) {
        w.resize(bow.size()); v.resize(bow.size());
        for (size_t i = 0; i < bow.size(); i++) { w[i] = bow[i].first; v[i] = bow[i].second; }
    }
    void erase_locked(int slot) {
        ctx_.check(eorb_kfdb_erase(ctx_.get(), slot));
        map_[slot] = -1; bad_[slot] = 0;
        for (auto& s : covis_) if (s == slot) s = -1;
        std::fill(covis_.begin() + (size_t)slot * EORB_KFDB_COVIS, covis_.begin() + (size_t)(slot + 1) * EORB_KFDB_COVIS, -1);
    }
    eorb_host::Context ctx_;
    std::mutex mMutex;
    std::vector<long> map_;            // per slot: the keyframe's map id (-1: free slot)
    std::vector<uint8_t> bad_;         // per slot: isBad()
    std::vector<int32_t> covis_;       // per slot: ten neighbours as slots
    std::vector<long> badMaps_;
};

// The two stages of TwoViewReconstruction (src/TwoViewReconstruction.cc) whose cost grows with the match count, on the calling thread's
// context.  FindHomographyFundamental = the two threads of Reconstruct (:131-136 / :228-233) in one call; CheckRT = :1242-1352 for every
// pose hypothesis of ReconstructF (4) / ReconstructH (8) in one call.  The set draw (mvSets), SH/(SH+SF) and the H/F choice, K.t()*F21*K,
// DecomposeE, the Faugeras decomposition, resolveReconstStat* and acos stay with an adapter that uses these two; Reconstruct below is the
// whole function in one device call, and only the set draw (mvSets) stays with the adapter.
class TwoViewReconstruction {
public:
    typedef std::pair<int, int> Match;
    struct HF {                            // what FindHomography / FindFundamental leave; best_it < 0: no iteration scored above 0
        float H21[9], F21[9], SH = 0.f, SF = 0.f; int32_t best_it_h = -1, best_it_f = -1;
        std::vector<uint8_t> vbMatchesInliersH, vbMatchesInliersF;
        std::vector<float> it_score_h, it_score_f, it_H, it_F;      // filled when asked for (test aids)
    };
    struct RT {                            // CheckRT per pose: nGood, vbGood / vP3D by first index, vCosParallax[min(mMinTriangulated, size - 1)]
        std::vector<int32_t> nGood; std::vector<uint8_t> vbGood; std::vector<float> vP3D, cosParallax, cosAll;
        double parallax(int pose) const { return nGood[pose] > 0 ? std::acos((double)cosParallax[pose]) * 180 / 3.14159265358979323846 : 0.0; }      // :1346
    };

    explicit TwoViewReconstruction(const float K[9], float sigma = 1.0f, int iterations = 200) : mSigma(sigma), mMaxIterations(iterations) {
        for (int i = 0; i < 9; i++) mK[i] = K[i];
    }
    eorb_tvr_params params{1.0f, 5.991f, 3.841f};        // sigma is set from mSigma at each call
    float mMinParallaxCRT = 0.99998f; int mMinTriangulated = 50;

    // vKeys1 / vKeys2: ALL keys of the two frames; vMatches12: mvMatches12; vSets: mMaxIterations x 8 indices into vMatches12
    HF FindHomographyFundamental(const std::vector<eorb_keypoint>& vKeys1, const std::vector<eorb_keypoint>& vKeys2, const std::vector<Match>& vMatches12,
                                 const std::vector<int32_t>& vSets, bool aids = false) const {
        auto& c = eorb_host::thread_context();
        const int N = (int)vMatches12.size(), it = (int)(vSets.size() / 8);
        const std::vector<int32_t> m = flat(vMatches12);
        HF o;
        o.vbMatchesInliersH.assign(N, 0); o.vbMatchesInliersF.assign(N, 0);
        if (aids) { o.it_score_h.assign(it, 0.f); o.it_score_f.assign(it, 0.f); o.it_H.assign((size_t)it * 9, 0.f); o.it_F.assign((size_t)it * 9, 0.f); }
        eorb_tvr_params p = params; p.sigma = mSigma;
        c.check(eorb_two_view_ransac(c.get(), vKeys1.data(), (int)vKeys1.size(), vKeys2.data(), (int)vKeys2.size(), m.data(), N, vSets.data(), it, &p,
                                     o.H21, &o.SH, &o.best_it_h, o.vbMatchesInliersH.data(), o.F21, &o.SF, &o.best_it_f, o.vbMatchesInliersF.data(),
                                     aids ? o.it_score_h.data() : nullptr, aids ? o.it_score_f.data() : nullptr, aids ? o.it_H.data() : nullptr,
                                     aids ? o.it_F.data() : nullptr));
        return o;
    }
    RT CheckRT(const std::vector<eorb_keypoint>& vKeys1, const std::vector<eorb_keypoint>& vKeys2, const std::vector<Match>& vMatches12,
               const std::vector<uint8_t>& vbMatchesInliers, const std::vector<eorb_tvr_pose>& poses, float th2, bool cosAll = false) const {
        auto& c = eorb_host::thread_context();
        const size_t N = vMatches12.size(), Kp = poses.size(), n1 = vKeys1.size();
        const std::vector<int32_t> m = flat(vMatches12);
        RT o;
        o.nGood.assign(Kp, 0); o.vbGood.assign(Kp * n1, 0); o.vP3D.assign(Kp * n1 * 3, 0.f); o.cosParallax.assign(Kp, 0.f);
        if (cosAll) o.cosAll.assign(Kp * N, 0.f);
        c.check(eorb_two_view_check_rt(c.get(), vKeys1.data(), (int)n1, vKeys2.data(), (int)vKeys2.size(), m.data(), (int)N, vbMatchesInliers.data(), mK,
                                       th2, mMinParallaxCRT, mMinTriangulated, poses.data(), (int)Kp, o.nGood.data(), o.vbGood.data(), o.vP3D.data(),
                                       o.cosParallax.data(), cosAll ? o.cosAll.data() : nullptr));
        return o;
    }

    // ---- Reconstruct as one device call (eorb_two_view_reconstruct), in the reference's two overload shapes with OpenCV-free types:
    // a 3x3 / 3x1 cv::Mat is a Mat33 / Vec3 (row-major), a cv::Point3f a Vec3.  vMatches12 is the reference's argument (per key of frame 1
    // the index of its match in frame 2, or -1; mvMatches12 is built from it as :81-90 does); vSets, the draw of :107-124, is the
    // caller's (mMaxIterations x 8 indices into mvMatches12).  `last` keeps every field of the call's eorb_tvr_recon_result.
    struct Vec3 { float v[3]; };
    struct Mat33 { float m[9]; };
    struct ReconstInfo {                   // include/TwoViewReconstruction.h:62-80, with its initial values
        int mnBestGood = 0, mnMinGood = 0, mnSecondBest = 0; float mBestParallax = -1.f, mSecondBestPar = -1.f; bool isHomography = true;
        float mHScore = 0.f, mFScore = 0.f, mHFRatio = 0.f; unsigned char mnSimilar = 0; std::vector<int> mvnGood = std::vector<int>(8, 0);
    };
    struct Params2VR {                     // the members of Params2VR the decision reads (mThChiSq*, mMinParallaxCRT, mMinTriangulated: above)
        float mThHFRatio = 0.45f, mDefMinParallax = 1.0f, mThMinGoodR = 0.9f, mThMaxGoodR_F = 0.7f, mThMaxGoodR_H = 0.75f, mThRDHomo = (float)1.00001;
    } mParams2VR;
    mutable eorb_tvr_recon_result last{};

    // :67-158.  R21 / t21 / vP3D / vbTriangulated are written when the call returns true; R21 is left empty by the reference otherwise,
    // and here the arguments are left as they were.
    bool Reconstruct(const std::vector<eorb_keypoint>& vKeys1, const std::vector<eorb_keypoint>& vKeys2, const std::vector<int>& vMatches12,
                     const std::vector<int32_t>& vSets, Mat33& R21, Vec3& t21, std::vector<Vec3>& vP3D, std::vector<bool>& vbTriangulated) const {
        Out o = call(vKeys1, vKeys2, vMatches12, vSets, EORB_TVR_FORM_STOCK);
        if (!last.ok) return false;
        const size_t n1 = vKeys1.size();
        std::memcpy(R21.m, o.R21.data(), sizeof R21.m); std::memcpy(t21.v, o.t21.data(), sizeof t21.v);
        vP3D.resize(n1); vbTriangulated.assign(n1, false);
        for (size_t i = 0; i < n1; i++) { std::memcpy(vP3D[i].v, &o.p3d[3 * i], sizeof vP3D[i].v); vbTriangulated[i] = o.tri[i] != 0; }
        return true;
    }
    // :162-262.  The vectors get two entries (best, second best); at the SH+SF == 0 exit only vbTransInliers is written (:237), at the d test
    // of ReconstructH vbTransInliers and the three scores, as the reference does.  Where the reference would read vR[-1] (ReconstructH with
    // fewer than two hypotheses that triangulate anything) the entry is zeros.
    bool Reconstruct(const std::vector<eorb_keypoint>& vKeys1, const std::vector<eorb_keypoint>& vKeys2, const std::vector<int>& vMatches12,
                     const std::vector<int32_t>& vSets, std::vector<Mat33>& R21, std::vector<Vec3>& t21, std::vector<std::vector<Vec3>>& vP3D,
                     std::vector<std::vector<bool>>& vbTriangulated, std::vector<bool>& vbTransInliers, ReconstInfo& reconstInfo) const {
        Out o = call(vKeys1, vKeys2, vMatches12, vSets, EORB_TVR_FORM_INFO);
        vbTransInliers.assign(o.trans.size(), false);
        for (size_t i = 0; i < o.trans.size(); i++) vbTransInliers[i] = o.trans[i] != 0;
        if (last.stage == 0) return false;
        reconstInfo.mHScore = last.SH; reconstInfo.mFScore = last.SF; reconstInfo.mHFRatio = last.RH;
        if (last.stage == 1) return false;
        const size_t n1 = vKeys1.size();
        R21.assign(2, Mat33{}); t21.assign(2, Vec3{}); vP3D.assign(2, std::vector<Vec3>(n1)); vbTriangulated.assign(2, std::vector<bool>(n1, false));
        for (int s = 0; s < 2; s++) {
            std::memcpy(R21[s].m, &o.R21[9 * s], sizeof R21[s].m); std::memcpy(t21[s].v, &o.t21[3 * s], sizeof t21[s].v);
            for (size_t i = 0; i < n1; i++) { std::memcpy(vP3D[s][i].v, &o.p3d[3 * (s * n1 + i)], sizeof vP3D[s][i].v); vbTriangulated[s][i] = o.tri[s * n1 + i] != 0; }
        }
        reconstInfo.mnBestGood = last.best_good; reconstInfo.mBestParallax = last.best_parallax;
        reconstInfo.mnSecondBest = last.second_good; reconstInfo.mSecondBestPar = last.second_parallax;
        if (!last.is_homography) {         // (:972-976, resolveReconstStatF; ReconstructH writes neither isHomography nor these two)
            for (int i = 0; i < 4; i++) reconstInfo.mvnGood[i] = last.info_good[i];
            reconstInfo.isHomography = false;
            reconstInfo.mnMinGood = last.n_min_good; reconstInfo.mnSimilar = (unsigned char)last.n_similar;
        } else
            for (int i = 0; i < 8; i++) reconstInfo.mvnGood[i] = last.info_good[i];
        return last.ok != 0;
    }
private:
    struct Out { std::vector<float> R21, t21, p3d; std::vector<uint8_t> tri, trans; };
    Out call(const std::vector<eorb_keypoint>& vKeys1, const std::vector<eorb_keypoint>& vKeys2, const std::vector<int>& vMatches12,
             const std::vector<int32_t>& vSets, int form) const {
        auto& c = eorb_host::thread_context();
        std::vector<int32_t> m;
        for (size_t i = 0; i < vMatches12.size(); i++) if (vMatches12[i] >= 0) { m.push_back((int32_t)i); m.push_back(vMatches12[i]); }
        const int N = (int)(m.size() / 2), n1 = (int)vKeys1.size();
        eorb_tvr_recon_params p{mSigma, params.th_score, params.th_f, mParams2VR.mThHFRatio, mParams2VR.mDefMinParallax, mMinParallaxCRT,
                                mMinTriangulated, mParams2VR.mThMinGoodR, mParams2VR.mThMaxGoodR_F, mParams2VR.mThMaxGoodR_H, mParams2VR.mThRDHomo, form};
        Out o;
        o.R21.assign(18, 0.f); o.t21.assign(6, 0.f); o.p3d.assign((size_t)6 * n1, 0.f); o.tri.assign((size_t)2 * n1, 0); o.trans.assign((size_t)N, 0);
        c.check(eorb_two_view_reconstruct(c.get(), vKeys1.data(), n1, vKeys2.data(), (int)vKeys2.size(), m.data(), N, vSets.data(), (int)(vSets.size() / 8),
                                          mK, &p, &last, o.R21.data(), o.t21.data(), o.p3d.data(), o.tri.data(), o.trans.data(), nullptr));
        return o;
    }
    static std::vector<int32_t> flat(const std::vector<Match>& v) {
        std::vector<int32_t> m(2 * v.size());
        for (size_t i = 0; i < v.size(); i++) { m[2 * i] = v[i].first; m[2 * i + 1] = v[i].second; }
        return m;
    }
    float mK[9]; float mSigma; int mMaxIterations;
};

namespace detail {
// the tail of both SetRansacParameters: 1 when minInliers == N (exact), else ceil(log(1 - p) / log(1 - epsilon^3)), then
// max(1, min(n, maxIterations)).  "int nIterations = ceil(...)" of a value no int holds converts as the reference's x86 build does
// (INT_MIN -> 1 iteration)
inline int ransac_max_iterations(double probability, float epsilon, bool exact, int maxIterations) {
    int nIterations = 1;
    if (!exact) {
        const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3)));
        nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : (-2147483647 - 1);
    }
    return std::max(1, std::min(nIterations, maxIterations));
}
// the minimal sets of iterations [from_set, to_set), K draws without replacement each, appended to out:
// randomInt(min, max) = DUtils::Random::RandomInt
template <int K, class RandomInt> void draw_minimal_sets(int N, int from_set, int to_set, RandomInt&& randomInt, std::vector<int32_t>& out) {
    std::vector<int32_t> all((size_t)N), avail;
    for (int i = 0; i < N; i++) all[i] = i;
    for (int it = from_set; it < to_set; it++) {
        avail = all;
        for (int i = 0; i < K; i++) {
            const int randi = randomInt(0, (int)avail.size() - 1);
            out.push_back(avail[randi]);
            avail[randi] = avail.back(); avail.pop_back();
        }
    }
}
}  // namespace detail

// Sim3Solver (src/Sim3Solver.cc) on the calling thread's context, over correspondences the adapter has compacted: the constructor's filter
// (:71-91: null, isBad, index < 0) stays with it, and so do the set draw and the g2o::Sim3 composition.  The first
// iterate() / find() makes ONE device call for all mRansacMaxIts iterations; iterate(n, ...) then replays its chunk of the loop from the
// per-iteration counts and transforms, so "while(!bConverge && !bNoMore) iterate(20, ...)" (LoopClosing.cc:698-701) returns what the
// reference returns, chunk by chunk.  GetEstimated* give the state that loop ends in (the reference's mBest* once it has ended).
class Sim3Solver {
public:
    typedef std::vector<float> Mat;        // a 4x4 / 3x3 / 3x1 float matrix, row-major; empty = cv::Mat()

    // Xw1 / Xw2: 3 floats per correspondence (GetWorldPos of both sides); Rt1 / Rt2: Rcw row-major then tcw of pKF1 / pKF2;
    // sigma2_1 / sigma2_2: getKPtLevelSigma2 per correspondence.  vnIndices1 / N1 (optional): mvnIndices1 and mN1, for vbInliers.
    Sim3Solver(const std::vector<float>& Xw1, const std::vector<float>& Xw2, const float Rt1[12], const float Rt2[12], const eorb_camera& cam1,
               const eorb_camera& cam2, const std::vector<float>& sigma2_1, const std::vector<float>& sigma2_2, bool bFixScale = true,
               const std::vector<int>& vnIndices1 = std::vector<int>(), int N1 = -1)
        : mXw1(Xw1), mXw2(Xw2), mSigma1(sigma2_1), mSigma2(sigma2_2), mvnIndices1(vnIndices1), N((int)(Xw1.size() / 3)), mbFixScale(bFixScale) {
        for (int i = 0; i < 12; i++) { mProblem.Rt1[i] = Rt1[i]; mProblem.Rt2[i] = Rt2[i]; }
        mProblem.cam1 = cam1; mProblem.cam2 = cam2;
        if (mvnIndices1.empty()) for (int i = 0; i < N; i++) mvnIndices1.push_back(i);
        mN1 = N1 < 0 ? N : N1;
        SetRansacParameters();
    }
    // :126-150
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacProb = probability; mRansacMinInliers = minInliers;
        mRansacMaxIts = detail::ransac_max_iterations(mRansacProb, (float)mRansacMinInliers / N, mRansacMinInliers == N, maxIterations);
        mnIterations = 0; mnBestInliers = 0; mSolved = false;
    }
    int GetMaxIterations() const { return mRansacMaxIts; }
    // the minimal sets of :178-189 from the adapter's generator: randomInt(min, max) = DUtils::Random::RandomInt
    template <class RandomInt> void DrawSets(RandomInt&& randomInt) {
        mvSets.clear();
        detail::draw_minimal_sets<3>(N, 0, mRansacMaxIts, randomInt, mvSets);
        mSolved = false;
    }
    void SetSets(const std::vector<int32_t>& vSets) { mvSets = vSets; mSolved = false; }      // mRansacMaxIts x 3 indices

    Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {      // :221-297
        bNoMore = false; bConverge = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        if (N < mRansacMinInliers) { bNoMore = true; return Mat(); }
        solve();
        int nCurrentIterations = 0;
        Mat bestSim3;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            const int it = mnIterations;
            nCurrentIterations++; mnIterations++;
            if (mItInliers[it] >= mnBestInliers) {
                mnBestInliers = mItInliers[it];
                const Mat T12(mItT12.begin() + 16 * (size_t)it, mItT12.begin() + 16 * (size_t)it + 16);
                if (mItInliers[it] > mRansacMinInliers) {        // (the device's winner: its flags are this iteration's)
                    nInliers = mItInliers[it];
                    for (int i = 0; i < N; i++) if (mvbBestInliers[i]) vbInliers[mvnIndices1[i]] = true;
                    bConverge = true;
                    return T12;
                }
                bestSim3 = T12;
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return bestSim3;
    }
    Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {                      // :152-219
        bool bConverge;
        const Mat T = iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge);
        return bConverge ? T : Mat();
    }
    Mat find(std::vector<bool>& vbInliers12, int& nInliers) { bool bFlag; return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers); }      // :299-303
    Mat GetEstimatedRotation() const { return Mat(mResult.R12, mResult.R12 + 9); }
    Mat GetEstimatedTranslation() const { return Mat(mResult.t12, mResult.t12 + 3); }
    float GetEstimatedScale() const { return mResult.s12; }
    const eorb_sim3_result& result() { solve(); return mResult; }
    const std::vector<int32_t>& it_inliers() { solve(); return mItInliers; }
    int mnIterations = 0;
private:
    void solve() {
        if (mSolved) return;
        auto& c = eorb_host::thread_context();
        mProblem.N = N; mProblem.iters = (int)(mvSets.size() / 3); mProblem.fix_scale = mbFixScale; mProblem.min_inliers = mRansacMinInliers;
        if (mProblem.iters != mRansacMaxIts) throw eorb_host::Error(EORB_E_ARG, "Sim3Solver: the sets do not cover mRansacMaxIts iterations (DrawSets / SetSets)");
        mvbBestInliers.assign((size_t)N, 0); mItInliers.assign((size_t)mProblem.iters, 0); mItT12.assign((size_t)mProblem.iters * 16, 0.f);
        c.check(eorb_sim3_ransac(c.get(), &mProblem, 1, mXw1.data(), mXw2.data(), mSigma1.data(), mSigma2.data(), mvSets.data(), &mResult,
                                 mvbBestInliers.data(), mItInliers.data(), mItT12.data(), nullptr, nullptr));
        mSolved = true;
    }
    std::vector<float> mXw1, mXw2, mSigma1, mSigma2;
    std::vector<int> mvnIndices1;
    std::vector<int32_t> mvSets, mItInliers;
    std::vector<float> mItT12;
    std::vector<uint8_t> mvbBestInliers;
    eorb_sim3_problem mProblem{}; eorb_sim3_result mResult{};
    int N, mN1 = 0; bool mbFixScale;
    double mRansacProb = 0.99; int mRansacMinInliers = 6, mRansacMaxIts = 300, mnBestInliers = 0; bool mSolved = false;
};

// ORB_SLAM3::MLPnPsolver (src/MLPnPsolver.cpp) over correspondences the adapter has compacted (the constructor's filter :67-96 stays with
// it; vKeyPointIndices / nKeyPoints carry mvKeyPointIndices and mvpMapPointMatches.size() for vbInliers).  Every iterate(n, ...) is one
// device call that walks the iterations this call of the reference's loop covers, resumed from the running best of the calls before it
// (first_it / best_it of eorb_mlpnp_problem), so "iterate(5, ...)" of Tracking.cc:2716-2729 returns what the reference returns, call by call.
class MLPnPsolver {
public:
    typedef std::vector<float> Mat;        // a 4x4 float matrix, row-major; empty = cv::Mat()

    // p2d: 2 floats per correspondence (the undistorted keypoint); Xw: 3 floats (GetWorldPos); sigma2: getKPtLevelSigma2
    MLPnPsolver(const std::vector<float>& p2d, const std::vector<float>& Xw, const std::vector<float>& sigma2, const eorb_camera& cam,
                const std::vector<int>& vKeyPointIndices = std::vector<int>(), int nKeyPoints = -1)
        : mP2D(p2d), mXw(Xw), mSigma2(sigma2), mvKeyPointIndices(vKeyPointIndices), N((int)(Xw.size() / 3)) {
        mProblem.cam = cam;
        if (mvKeyPointIndices.empty()) for (int i = 0; i < N; i++) mvKeyPointIndices.push_back(i);
        mnKeyPoints = nKeyPoints < 0 ? N : nKeyPoints;
        SetRansacParameters();
    }
    // :268-303.  mRansacEpsilon is a float
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 6, float epsilon = 0.4f,
                             float th2 = 5.991f) {
        mRansacProb = probability; mRansacMinInliers = minInliers; mRansacEpsilon = epsilon; mRansacMinSet = minSet;
        int nMinInliers = (int)(N * mRansacEpsilon);
        if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
        if (nMinInliers < minSet) nMinInliers = minSet;
        mRansacMinInliers = nMinInliers;
        if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
        mRansacMaxIts = detail::ransac_max_iterations(mRansacProb, mRansacEpsilon, mRansacMinInliers == N, maxIterations);
        mTh2 = th2;
        mnIterations = 0; mnBestIt = -1;
    }
    int GetMaxIterations() const { return mRansacMaxIts; }
    int GetMinInliers() const { return mRansacMinInliers; }
    // the minimal sets of :176-188 from the adapter's generator, for nSets iterations (at least what the calls of iterate will reach):
    // randomInt(min, max) = DUtils::Random::RandomInt.  Sets already drawn stay; more are appended.
    template <class RandomInt> void DrawSets(RandomInt&& randomInt, int nSets) {
        detail::draw_minimal_sets<6>(N, (int)(mvSets.size() / 6), nSets, randomInt, mvSets);
    }
    void SetSets(const std::vector<int32_t>& vSets) { mvSets = vSets; }      // 6 indices per iteration
    const std::vector<int32_t>& sets() const { return mvSets; }

    Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {      // :149-266
        bNoMore = false; vbInliers.clear(); nInliers = 0;
        if (N < mRansacMinInliers) { bNoMore = true; return Mat(); }
        // while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations): the first call runs to the maximum, later ones n more
        const int end = std::max(mRansacMaxIts, mnIterations + nIterations);
        if ((int)(mvSets.size() / 6) < end) throw eorb_host::Error(EORB_E_ARG, "MLPnPsolver: the sets do not cover the iterations of this call (DrawSets / SetSets)");
        auto& c = eorb_host::thread_context();
        mProblem.N = N; mProblem.iters = end; mProblem.min_inliers = mRansacMinInliers; mProblem.th2 = mTh2;
        mProblem.first_it = mnIterations; mProblem.best_it = mnBestIt;
        std::vector<uint8_t> flags((size_t)N, 0);
        c.check(eorb_mlpnp_ransac(c.get(), &mProblem, 1, mP2D.data(), mXw.data(), mSigma2.data(), mvSets.data(), &mResult, flags.data(),
                                  nullptr, nullptr, nullptr));
        mnIterations = mResult.iterations_used; mnBestIt = mResult.best_it;
        const bool best = !mResult.refined && mResult.n_best >= mRansacMinInliers;
        if (!mResult.refined) bNoMore = true;      // (the walk ran to its end, which is at or beyond mRansacMaxIts)
        if (!mResult.refined && !best) return Mat();
        nInliers = mResult.n_inliers;
        vbInliers = std::vector<bool>((size_t)mnKeyPoints, false);
        for (int i = 0; i < N; i++) if (flags[i]) vbInliers[mvKeyPointIndices[i]] = true;
        return Mat(mResult.Tcw, mResult.Tcw + 16);
    }
    const eorb_mlpnp_result& result() const { return mResult; }
    int mnIterations = 0;
private:
    std::vector<float> mP2D, mXw, mSigma2;
    std::vector<int> mvKeyPointIndices;
    std::vector<int32_t> mvSets;
    eorb_mlpnp_problem mProblem{}; eorb_mlpnp_result mResult{};
    int N, mnKeyPoints = 0, mnBestIt = -1;
    double mRansacProb = 0.99; int mRansacMinInliers = 8, mRansacMaxIts = 300, mRansacMinSet = 6; float mRansacEpsilon = 0.4f, mTh2 = 5.991f;
};

// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:527-784; params.form = EORB_NEWPTS_TRACKING: Tracking::CreateNewMapPoints,
// src/Tracking.cc:3232-3408): the per-match half for the K neighbours whose keypoints are concatenated in kps2 (kfOff[K + 1]), on
// vMatches12 (K * n1) as SearchForTriangulation returned it for every neighbour with the initial eligibility.  The claim of idx1 by an
// earlier neighbour (:775) and the ratioFactor rule of mixed keyframes (:464, :545-546) are resolved in the call.  The adapter then walks
// status in the reference's order and, per EORB_NP_NEW entry, does :770-783 (new MapPoint(x3D), the observations, the two AddMapPoint,
// ComputeDistinctiveDescriptors, UpdateNormalAndDepth, Atlas::AddMapPoint).  params as include/eorb_fe.h documents eorb_newpts_params.
struct NewMapPoints {
    std::vector<uint8_t> status, branch;       // K * n1: EORB_NP_*, EORB_NP_BRANCH_*
    std::vector<float> x3D, cosParallax;       // 3 per entry (zero unless status is EORB_NP_NEW); cosParallaxRays
    std::vector<int32_t> nNew;                 // per neighbour
};
inline NewMapPoints CreateNewMapPoints(const std::vector<eorb_host::KeyPoint>& kps1, const std::vector<eorb_host::KeyPoint>& kps2,
                                       const std::vector<int32_t>& kfOff, const std::vector<int32_t>& vMatches12, const eorb_newpts_params& params) {
    auto& c = eorb_host::thread_context();
    const int K = kfOff.empty() ? 0 : (int)kfOff.size() - 1;
    const size_t n = (size_t)K * kps1.size();
    if (vMatches12.size() != n) throw eorb_host::Error(EORB_E_ARG, "CreateNewMapPoints: vMatches12 holds K * n1 entries");
    NewMapPoints r;
    r.status.resize(n); r.branch.resize(n); r.x3D.resize(3 * n); r.cosParallax.resize(n); r.nNew.resize((size_t)K);
    const eorb_newpts_out out{r.status.data(), r.x3D.data(), r.branch.data(), r.cosParallax.data(), r.nNew.data()};
    c.check(eorb_new_map_points(c.get(), kps1.data(), (int)kps1.size(), kps2.data(), kfOff.data(), K, vMatches12.data(), &params, &out));
    return r;
}

// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:349-423) for a batch of map points (CSR offsets into desc rows)
inline std::vector<int> ComputeDistinctiveDescriptors(const eorb_host::Mat8& desc, const std::vector<int32_t>& offsets) {
    auto& c = eorb_host::thread_context();
    std::vector<int> best(offsets.size() - 1, -1);
    c.check(eorb_distinctive_descriptors(c.get(), desc.ptr(), offsets.data(), (int)offsets.size() - 1, best.data()));
    return best;
}

}  // namespace ORB_SLAM3
