// ORBmatcher.h -- adapter with the surface of /root/reference/include/ORBmatcher.h:36-103 over the C ABI.
//
// The reference matchers take Frame / KeyFrame / MapPoint pointer graphs guarded by mutexes.  The adapter's job
// (see INTEGRATION.md for the Frame-typed overloads a maintainer adds inside the ORB-SLAM3 tree) is to flatten what
// the loops read under the reference's locks, call the kernels, and write the assignments back in reference order.
// This header holds the dependency-free core: same constants, same constructor, DescriptorDistance, and the
// flattened forms of the two SearchByProjection variants and of the stereo matchers.
#ifndef ORBX_ADAPTER_ORBMATCHER_H
#define ORBX_ADAPTER_ORBMATCHER_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <array>
#include <vector>

#include "../../include/orbx.h"

namespace ORB_SLAM3 {

// What the projection matchers read of a Frame (Frame.h: mvKeysUn, mDescriptors, mnMinX.., mvScaleFactors, mvuRight)
struct FrameView {
    const orbx_keypoint *mvKeysUn = nullptr;
    const uint8_t *mDescriptors = nullptr;  // N x 32
    int N = 0;
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
    const float *mvScaleFactors = nullptr;
    int nlevels = 0;
    const float *mvuRight = nullptr;  // NULL for monocular
    orbx_frame_desc c() const { return orbx_frame_desc{mvKeysUn, mDescriptors, N, mnMinX, mnMaxX, mnMinY, mnMaxY, mvScaleFactors, nlevels, mvuRight}; }
};

// The MapPoint scratch fields SearchByProjection reads (MapPoint.h:171-179), one entry per map point
struct MapPointBatch {
    std::vector<float> mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos;
    std::vector<int32_t> mnTrackScaleLevel;
    std::vector<uint8_t> descriptors;  // n x 32 (MapPoint::GetDescriptor)
    std::vector<uint8_t> inView;       // mbTrackInView && !isBad() && !(bFarPoints && mTrackDepth > thFarPoints)
    std::vector<uint8_t> hasObservations;  // Observations() > 0
    int size() const { return (int)mTrackProjX.size(); }
};

class ORBmatcher;
class ORBVocabularyDevice;

// A Frame resident on the device across matcher calls (orbx_frame, include/orbx.h): built once per Frame -- load() after UndistortKeyPoints, or
// loadBatch() from an extractor's resident batch -- and passed to the SearchByProjection / SearchLocalPoints overloads below in place of a
// FrameView.  It belongs to the ORBmatcher it was created with and must not outlive it.
class DeviceFrame {
public:
    DeviceFrame(ORBmatcher &matcher, int cap);
    ~DeviceFrame() { orbx_frame_destroy(f_); }
    DeviceFrame(const DeviceFrame &) = delete;
    DeviceFrame &operator=(const DeviceFrame &) = delete;
    void load(const FrameView &F) {
        orbx_frame_desc fd = F.c();
        check(orbx_frame_load_host(f_, &fd), "orbx_frame_load_host");
    }
    // frame `frame` of the extractor's last batch; bounds4 / scaleFactors NULL = the extractor's
    void loadBatch(orbx_extractor *ex, int frame, const float *bounds4 = nullptr, const float *scaleFactors = nullptr, int nlevels = 0) {
        check(orbx_frame_load_batch(f_, ex, frame, bounds4, scaleFactors, nlevels), "orbx_frame_load_batch");
    }
    // loadBatch plus the frame's mvuRight, mvDepth and raw key points of the (left) extractor's last orbx_stereo_batch_device / orbx_rgbd_batch_device
    // stage, copied on the device in the same launch; refused when no stage has run on the extractor's current batch
    void loadStereoBatch(orbx_extractor *left, int frame, const float *bounds4 = nullptr, const float *scaleFactors = nullptr, int nlevels = 0) {
        check(orbx_frame_load_stereo_batch(f_, left, frame, bounds4, scaleFactors, nlevels), "orbx_frame_load_stereo_batch");
    }
    // load() with F.mvuRight required, mvDepth [N] and the raw mvKeys[i].pt as (x, y) pairs (empty: the undistorted points) in the same upload
    void loadHostStereo(const FrameView &F, const std::vector<float> &mvDepth, const std::vector<float> &keysXY = {}) {
        orbx_frame_desc fd = F.c();
        if ((int)mvDepth.size() != fd.n || (!keysXY.empty() && (int)keysXY.size() != 2 * fd.n)) throw std::runtime_error("loadHostStereo: array sizes");
        check(orbx_frame_load_host_stereo(f_, &fd, mvDepth.data(), keysXY.empty() ? nullptr : keysXY.data()), "orbx_frame_load_host_stereo");
    }
    int count() {
        int n = 0;
        check(orbx_frame_count(f_, &n), "orbx_frame_count");
        return n;
    }
    // a fisheye-stereo frame (Frame::Nleft != -1): left.mvKeysUn = mvKeys, left.N = Nleft, left.mDescriptors = ALL N rows; keysRight = mvKeysRight,
    // l2r / r2l = mvLeftToRightMatch / mvRightToLeftMatch
    void loadFisheye(const FrameView &left, const std::vector<orbx_keypoint> &keysRight, const std::vector<int32_t> &l2r, const std::vector<int32_t> &r2l) {
        orbx_frame_desc fd = left.c();
        check(orbx_frame_load_host_fisheye(f_, &fd, keysRight.data(), (int)keysRight.size(), l2r.data(), r2l.data()), "orbx_frame_load_host_fisheye");
    }
    // frame `frame` of the last fisheye stereo stage on (left, right) (orbx_stereo_fisheye_batch_device); asynchronous
    void loadStereoFisheyeBatch(orbx_extractor *left, orbx_extractor *right, int frame, const float *bounds4 = nullptr, const float *scaleFactors = nullptr,
                                int nlevels = 0) {
        check(orbx_frame_load_stereo_fisheye_batch(f_, left, right, frame, bounds4, scaleFactors, nlevels), "orbx_frame_load_stereo_fisheye_batch");
    }
    // Nleft and N - Nleft (-1 for a monocular / rectified frame)
    void counts(int &nLeft, int &nRight) { check(orbx_frame_counts(f_, &nLeft, &nRight), "orbx_frame_counts"); }
    // Frame::ComputeBoW's transform on the resident descriptors (orbx_frame_compute_bow): the FeatureVector stays here for the SearchByBoW
    // overloads on a DeviceFrame.  wordId / nodeId (optional) receive N ids each -- mBowVec is folded from the word ids on the host.
    inline void ComputeBoW(ORBmatcher &matcher, const ORBVocabularyDevice &voc, int levelsup = 4, std::vector<int32_t> *wordId = nullptr,
                           std::vector<int32_t> *nodeId = nullptr);
    // the same for a fisheye-stereo frame (orbx_frame_compute_bow_fisheye): all N = Nleft + N_right rows, ids in the rig's numbering (features
    // >= Nleft are the right camera's); the FeatureVector stays here for ORBmatcher::SearchByBoWFisheye
    inline void ComputeBoWFisheye(ORBmatcher &matcher, const ORBVocabularyDevice &voc, int levelsup = 4, std::vector<int32_t> *wordId = nullptr,
                                  std::vector<int32_t> *nodeId = nullptr);
    // Frame::mBowVec after ComputeBoW / ComputeBoWFisheye (orbx_frame_bow_vector): ascending word ids and their normalised tf-idf values, built on the
    // device from the kept word ids.  One synchronisation.
    inline void BowVector(ORBmatcher &matcher, std::vector<int32_t> &wordId, std::vector<double> &value);
    orbx_frame *handle() const { return f_; }
    int capacity() const { return cap_; }

private:
    static void check(int st, const char *what) {
        if (st < 0) throw std::runtime_error(std::string(what) + ": " + orbx_status_string(st) + " " + orbx_last_error());
    }
    orbx_frame *f_ = nullptr;
    int cap_ = 0;
};

// An immutable key frame resident on the device (orbx_keyframe): what KeyFrame::KeyFrame(Frame&) (KeyFrame.cc:36-82) copies of the frame.  It belongs
// to no matcher -- every ORBmatcher of the same device may search it, from any thread (ORBmatcher::FuseSearchKeyFrames / FuseMapPoints); destroy it
// only when no call that was handed it is running.
class DeviceKeyFrame {
public:
    // a device-to-device copy of a loaded monocular / rectified DeviceFrame of `matcher` (asynchronous; the frame may be reloaded right away)
    inline DeviceKeyFrame(ORBmatcher &matcher, DeviceFrame &frame, const float *mvInvLevelSigma2);
    // the same object from host arrays (a loaded atlas): one upload
    inline DeviceKeyFrame(ORBmatcher &matcher, const FrameView &KF, const float *mvInvLevelSigma2);
    // a rectified-stereo / RGB-D key frame from host arrays (orbx_keyframe_create_host_stereo): KF.mvuRight required, mvDepth [N], keysXY = the raw
    // mvKeys[i].pt as (x, y) pairs (empty: the undistorted points) -- what ORBmatcher::TriangulatePairsStereo / SearchAndTriangulateStereo decide stereo pairs on
    inline DeviceKeyFrame(ORBmatcher &matcher, const FrameView &KF, const std::vector<float> &mvDepth, const std::vector<float> &keysXY,
                          const float *mvInvLevelSigma2);
    // a fisheye-stereo key frame (KeyFrame::NLeft != -1) -- mvKeys, mvKeysRight, all N descriptor rows, both counts and both grids: a device-to-device
    // copy of a loaded fisheye-stereo DeviceFrame of `matcher` (orbx_keyframe_from_frame_fisheye; asynchronous, also while the counts are still on the
    // device) ...
    struct Fisheye {};
    inline DeviceKeyFrame(Fisheye, ORBmatcher &matcher, DeviceFrame &frame, const float *mvInvLevelSigma2);
    // ... or the same object from host arrays (orbx_keyframe_create_host_fisheye): left.mvKeysUn = mvKeys, left.N = NLeft, left.mDescriptors = ALL N
    // rows, keysRight = mvKeysRight.  mvLeftToRightMatch / mvRightToLeftMatch are not kept: Fuse does not read them.
    inline DeviceKeyFrame(ORBmatcher &matcher, const FrameView &left, const std::vector<orbx_keypoint> &keysRight, const float *mvInvLevelSigma2);
    ~DeviceKeyFrame() { orbx_keyframe_destroy(kf_); }
    DeviceKeyFrame(const DeviceKeyFrame &) = delete;
    DeviceKeyFrame &operator=(const DeviceKeyFrame &) = delete;
    int count() {
        int n = 0;
        const int st = orbx_keyframe_count(kf_, &n);
        if (st < 0) throw std::runtime_error(std::string("orbx_keyframe_count: ") + orbx_status_string(st));
        return n;
    }
    // NLeft and N - NLeft (-1 for a monocular / rectified key frame)
    void counts(int &nLeft, int &nRight) {
        const int st = orbx_keyframe_counts(kf_, &nLeft, &nRight);
        if (st < 0) throw std::runtime_error(std::string("orbx_keyframe_counts: ") + orbx_status_string(st));
    }
    // KeyFrame::NLeft != -1: made by one of the two fisheye-stereo constructors.  ComputeBoW / BowFromFrame and the resident BoW searches of ORBmatcher
    // dispatch on it (orbx_keyframe_*_fisheye); a list that mixes the two kinds throws, as Fuse does.
    bool fisheye() const { return fisheye_; }
    // KeyFrame::ComputeBoW on the resident descriptors (orbx_keyframe_compute_bow[_fisheye]): the key frame keeps mFeatVec for the resident SearchByBoW /
    // SearchForTriangulation overloads of ORBmatcher.  Set once; a second call with the same vocabulary and levelsup only returns the ids.  wordId /
    // nodeId (optional) receive N ids each -- mBowVec is folded from the word ids on the host.  Order this call before any BoW search is handed the
    // key frame (include/orbx.h, SHARING).
    inline void ComputeBoW(ORBmatcher &matcher, const ORBVocabularyDevice &voc, int levelsup = 4, std::vector<int32_t> *wordId = nullptr,
                           std::vector<int32_t> *nodeId = nullptr);
    // the mBowVec(F.mBowVec), mFeatVec(F.mFeatVec) part of KeyFrame::KeyFrame(Frame&) (orbx_keyframe_bow_from_frame): a device-to-device copy from the
    // DeviceFrame this key frame was made from, after its ComputeBoW and before its next load; asynchronous
    inline void BowFromFrame(ORBmatcher &matcher, DeviceFrame &frame);
    // KeyFrame::mBowVec of a key frame that has BoW (orbx_keyframe_bow_vector): ascending word ids and their normalised values
    inline void BowVector(ORBmatcher &matcher, std::vector<int32_t> &wordId, std::vector<double> &value);
    orbx_keyframe *handle() const { return kf_; }

private:
    orbx_keyframe *kf_ = nullptr;
    bool fisheye_ = false;
};

// A device-resident table of map points (orbx_map): what the one-call searches read of a MapPoint -- GetWorldPos(), GetNormal(), mfMinDistance,
// mfMaxDistance, mDescriptor -- in `capacity` slots addressed by ids the caller assigns (one int in MapPoint).  It belongs to no matcher: every
// ORBmatcher of its device may update and read it, and the ...Map overloads of ORBmatcher take (map, ids) where the others take the five arrays.
// What keeps it current: ORBmatcher::RefreshMapPoints writes the descriptor, the normal and both distances of the map points a LocalMapping step
// changed (ComputeDistinctiveDescriptors + UpdateNormalAndDepth, computed on the device; the table overloads of those two names are its halves);
// update() is left for SetWorldPos / a bundle adjustment's write-back and for a slot's first, whole write; erase() at SetBadFlag.  The caller runs
// none of them concurrently with a call that reads the table (Map::mMutexMapUpdate).  Destroy it only when no call that was handed it is running.
class DeviceMap {
public:
    explicit DeviceMap(int capacity, int device = 0) {
        const int st = orbx_map_create(device, capacity, &map_);
        if (st < 0) throw std::runtime_error(std::string("orbx_map_create: ") + orbx_status_string(st) + " " + orbx_last_error());
    }
    ~DeviceMap() { orbx_map_destroy(map_); }
    DeviceMap(const DeviceMap &) = delete;
    DeviceMap &operator=(const DeviceMap &) = delete;
    // row j of the arrays that are given (NULL: that field keeps its value) -> slot ids[j]; a slot's first update gives all five.  Does not wait.
    inline void update(ORBmatcher &matcher, const std::vector<int32_t> &ids, const float *pos, const float *normal, const float *minDistance,
                       const float *maxDistance, const uint8_t *descriptors);
    void erase(const std::vector<int32_t> &ids) {
        const int st = orbx_map_erase(map_, (int)ids.size(), ids.data());
        if (st < 0) throw std::runtime_error(std::string("orbx_map_erase: ") + orbx_status_string(st));
    }
    // slot ids[j] -> row j of the outputs that are given; one synchronisation (tests, serialization, debugging)
    inline void read(ORBmatcher &matcher, const std::vector<int32_t> &ids, float *pos, float *normal, float *minDistance, float *maxDistance,
                     uint8_t *descriptors);
    orbx_map *handle() const { return map_; }

private:
    orbx_map *map_ = nullptr;
};

// The BowVectors of a KeyFrameDatabase's key frames, resident on the device (orbx_keyframe_database): nSlots rows of at most wordsCap words, in slots
// the caller numbers (one int in KeyFrame).  It belongs to no matcher: every ORBmatcher of its device may write and query it.  add() at
// KeyFrameDatabase::add, erase() / clear() at the members of those names; queryFrame() / queryKeyFrame() are the first halves of
// DetectRelocalizationCandidates / DetectNBestCandidates -- the common words and L1 scores of every slot and the slots above minCommonWords -- and the
// covisibility accumulation behind them stays on the host.  The caller does not write while another thread's query is running
// (KeyFrameDatabase::mMutex).  Destroy it only when no call that was handed it is running.
class DeviceKeyFrameDatabase {
public:
    struct Candidates {
        int nCandidates = 0, maxCommonWords = 0;        // nCandidates is the true count; the lists hold at most the capacity asked for
        std::vector<int32_t> slot, commonWords;         // ascending slots with more than int(maxCommonWords * minRatio) common words
        std::vector<double> score;                      // L1Scoring::score(query, slot)
        std::vector<int32_t> nCommon;                   // full arrays (on request): per slot, -1 for an empty or excluded one
        std::vector<double> allScores;
    };
    DeviceKeyFrameDatabase(int nSlots, int wordsCap, int device = 0) : nSlots_(nSlots) {
        check(orbx_keyframe_database_create(device, nSlots, wordsCap, &db_), "orbx_keyframe_database_create");
    }
    ~DeviceKeyFrameDatabase() { orbx_keyframe_database_destroy(db_); }
    DeviceKeyFrameDatabase(const DeviceKeyFrameDatabase &) = delete;
    DeviceKeyFrameDatabase &operator=(const DeviceKeyFrameDatabase &) = delete;
    // the key frame's BowVector into `slot`; does not wait.  The row is a copy: the key frame may be destroyed afterwards
    inline void add(ORBmatcher &matcher, int slot, DeviceKeyFrame &kf);
    inline void erase(ORBmatcher &matcher, int slot);
    inline void clear(ORBmatcher &matcher);
    // exclude: slots left out of the count (spConnectedKF); candCap < 0: nSlots; full: also nCommon / allScores of every slot
    inline Candidates queryFrame(ORBmatcher &matcher, DeviceFrame &frame, const std::vector<int32_t> &exclude = {}, float minRatio = 0.8f, int candCap = -1,
                                 bool full = false);
    inline Candidates queryKeyFrame(ORBmatcher &matcher, DeviceKeyFrame &kf, const std::vector<int32_t> &exclude = {}, float minRatio = 0.8f,
                                    int candCap = -1, bool full = false);
    orbx_keyframe_database *handle() const { return db_; }

private:
    static void check(int st, const char *what) {
        if (st < 0) throw std::runtime_error(std::string(what) + ": " + orbx_status_string(st) + " " + orbx_last_error());
    }
    template <class Fn, class H> Candidates query(Fn fn, const char *what, ORBmatcher &matcher, H *src, const std::vector<int32_t> &exclude, float minRatio,
                                                  int candCap, bool full);
    orbx_keyframe_database *db_ = nullptr;
    int nSlots_ = 0;
};

class ORBmatcher {
public:
    static const int TH_LOW = ORBX_TH_LOW;
    static const int TH_HIGH = ORBX_TH_HIGH;
    static const int HISTO_LENGTH = ORBX_HISTO_LENGTH;

    ORBmatcher(float nnratio = 0.6, bool checkOri = true, int device = 0) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {
        const int st = orbx_matcher_create(device, &m_);
        if (st != ORBX_OK) throw std::runtime_error(std::string("orbx_matcher_create: ") + orbx_status_string(st) + " " + orbx_last_error());
    }
    ~ORBmatcher() { orbx_matcher_destroy(m_); }
    ORBmatcher(const ORBmatcher &) = delete;
    ORBmatcher &operator=(const ORBmatcher &) = delete;

    // ORBmatcher::DescriptorDistance (ORBmatcher.cc:2058-2074); scalar host helper for the adapter's own glue
    static int DescriptorDistance(const uint8_t *a, const uint8_t *b) {
        int dist = 0;
        for (int i = 0; i < 4; i++) {
            uint64_t x, y;
            __builtin_memcpy(&x, a + 8 * i, 8);
            __builtin_memcpy(&y, b + 8 * i, 8);
            dist += __builtin_popcountll(x ^ y);
        }
        return dist;
    }

    // SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th, bFarPoints, thFarPoints)
    // (ORBmatcher.cc:43-213, Nleft == -1).  vpMatch[i] = index into `mps` assigned to feature i, or -1.
    int SearchByProjection(const FrameView &F, const std::vector<uint8_t> &occupied, const MapPointBatch &mps, float th,
                           std::vector<int32_t> &vpMatch) {
        vpMatch.assign(F.N, -1);
        orbx_frame_desc fd = F.c();
        const int r = orbx_search_by_projection_mappoints(
            m_, &fd, occupied.empty() ? nullptr : occupied.data(), mps.size(), mps.mTrackProjX.data(), mps.mTrackProjY.data(),
            mps.mTrackProjXR.empty() ? nullptr : mps.mTrackProjXR.data(), mps.mnTrackScaleLevel.data(), mps.mTrackViewCos.data(),
            mps.descriptors.data(), mps.inView.empty() ? nullptr : mps.inView.data(),
            mps.hasObservations.empty() ? nullptr : mps.hasObservations.data(), th, mfNNratio, vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_search_by_projection_mappoints: ") + orbx_status_string(r));
        return r;
    }

    // SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (ORBmatcher.cc:1676-1887) after the
    // adapter projected LastFrame's map points with CurrentFrame's pose (host float math, unchanged).
    struct ProjectedQueries {
        std::vector<float> u, v, ur, angle;
        std::vector<int32_t> octave;
        std::vector<uint8_t> descriptors, hasObservations;
    };
    int SearchByProjection(const FrameView &Cur, const std::vector<uint8_t> &occupied, const ProjectedQueries &q, float th,
                           bool bForward, bool bBackward, std::vector<int32_t> &vpMatch) {
        vpMatch.assign(Cur.N, -1);
        orbx_frame_desc fd = Cur.c();
        const int mode = bForward ? 1 : (bBackward ? 2 : 0);
        const int r = orbx_search_by_projection_frame(
            m_, &fd, occupied.empty() ? nullptr : occupied.data(), (int)q.u.size(), q.u.data(), q.v.data(),
            q.ur.empty() ? nullptr : q.ur.data(), q.octave.data(), q.angle.data(), q.descriptors.data(),
            q.hasObservations.empty() ? nullptr : q.hasObservations.data(), th, mode, mbCheckOrientation ? 1 : 0, vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_search_by_projection_frame: ") + orbx_status_string(r));
        return r;   // vpMatch[i]: query index, -1 = untouched, -2 = assigned then cleared by the rotation check (slot becomes NULL)
    }

    // The same two matchers on a resident frame (DeviceFrame): nothing of the frame travels, its grid is built already
    int SearchByProjection(DeviceFrame &F, const std::vector<uint8_t> &occupied, const MapPointBatch &mps, float th, std::vector<int32_t> &vpMatch) {
        vpMatch.assign(F.count(), -1);
        const int r = orbx_frame_search_by_projection_mappoints(
            m_, F.handle(), occupied.empty() ? nullptr : occupied.data(), mps.size(), mps.mTrackProjX.data(), mps.mTrackProjY.data(),
            mps.mTrackProjXR.empty() ? nullptr : mps.mTrackProjXR.data(), mps.mnTrackScaleLevel.data(), mps.mTrackViewCos.data(),
            mps.descriptors.data(), mps.inView.empty() ? nullptr : mps.inView.data(),
            mps.hasObservations.empty() ? nullptr : mps.hasObservations.data(), th, mfNNratio, vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_by_projection_mappoints: ") + orbx_status_string(r));
        return r;
    }
    int SearchByProjection(DeviceFrame &Cur, const std::vector<uint8_t> &occupied, const ProjectedQueries &q, float th, bool bForward, bool bBackward,
                           std::vector<int32_t> &vpMatch) {
        vpMatch.assign(Cur.count(), -1);
        const int mode = bForward ? 1 : (bBackward ? 2 : 0);
        const int r = orbx_frame_search_by_projection_frame(
            m_, Cur.handle(), occupied.empty() ? nullptr : occupied.data(), (int)q.u.size(), q.u.data(), q.v.data(),
            q.ur.empty() ? nullptr : q.ur.data(), q.octave.data(), q.angle.data(), q.descriptors.data(),
            q.hasObservations.empty() ? nullptr : q.hasObservations.data(), th, mode, mbCheckOrientation ? 1 : 0, vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_by_projection_frame: ") + orbx_status_string(r));
        return r;
    }

    // Tracking::SearchLocalPoints (Tracking.cc:3339-3413) on a resident frame: isInFrustum of every local map point and
    // SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) in one call.  eligible[j] = !isBad() && mnLastFrameSeen != F.mnId,
    // hasObservations[j] = Observations() > 0 (empty = all).  inView[j] = mbTrackInView (for IncreaseVisible); vpMatch[i] = map point of feature i or -1.
    struct LocalMapPoints {
        std::vector<float> pos, normal;             // 3 floats each: GetWorldPos(), GetNormal()
        std::vector<float> minDistance, maxDistance; // GetMinDistanceInvariance / GetMaxDistanceInvariance inputs (mfMinDistance, mfMaxDistance)
        std::vector<uint8_t> descriptors;            // n x 32
        std::vector<uint8_t> eligible, hasObservations;
        int size() const { return (int)minDistance.size(); }
    };
    int SearchLocalPoints(DeviceFrame &F, const std::vector<uint8_t> &occupied, const orbx_camera &cam, const orbx_frame_pose &pose, float logScaleFactor,
                          float viewingCosLimit, const LocalMapPoints &mps, float th, bool bFarPoints, float thFarPoints, std::vector<uint8_t> &inView,
                          std::vector<int32_t> &vpMatch) {
        inView.assign(mps.size(), 0);
        vpMatch.assign(F.count(), -1);
        const int r = orbx_frame_search_local_points(
            m_, F.handle(), occupied.empty() ? nullptr : occupied.data(), &cam, &pose, logScaleFactor, viewingCosLimit, mps.size(), mps.pos.data(),
            mps.normal.data(), mps.minDistance.data(), mps.maxDistance.data(), mps.descriptors.data(), mps.eligible.empty() ? nullptr : mps.eligible.data(),
            mps.hasObservations.empty() ? nullptr : mps.hasObservations.data(), th, mfNNratio, bFarPoints ? 1 : 0, thFarPoints, inView.data(), vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_local_points: ") + orbx_status_string(r));
        return r;
    }

    // The fisheye-stereo twins on a resident rig frame (DeviceFrame::loadFisheye / loadStereoFisheyeBatch): features [0, Nleft) left, [Nleft, N) right.
    // SearchByProjection(Frame&, vector<MapPoint*>&, th, ...) whole (ORBmatcher.cc:43-213); the *R fields are the right camera's mTrack*R.
    struct FisheyeMapPoints {
        std::vector<uint8_t> inView, inViewR, descriptors, hasObservations;
        std::vector<float> projX, projY, viewCos, projXR, projYR, viewCosR;
        std::vector<int32_t> level, levelR;
        int size() const { return (int)projX.size(); }
    };
    int SearchByProjectionFisheye(DeviceFrame &F, const std::vector<uint8_t> &occupied, const FisheyeMapPoints &mp, float th, std::vector<int32_t> &vpMatch) {
        vpMatch.assign(F.count(), -1);
        const int r = orbx_frame_search_by_projection_mappoints_fisheye(
            m_, F.handle(), occupied.empty() ? nullptr : occupied.data(), mp.size(), mp.inView.data(), mp.projX.data(), mp.projY.data(), mp.level.data(),
            mp.viewCos.data(), mp.inViewR.data(), mp.projXR.data(), mp.projYR.data(), mp.levelR.data(), mp.viewCosR.data(), mp.descriptors.data(),
            mp.hasObservations.empty() ? nullptr : mp.hasObservations.data(), th, mfNNratio, vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_by_projection_mappoints_fisheye: ") + orbx_status_string(r));
        return r;
    }
    // SearchByProjection(Frame &Cur, const Frame &Last, th, bMono) with the twin (:1676-1887, :1794-1863); vr = v of the right-camera projection
    // (q.ur holds its u)
    int SearchByProjectionFisheye(DeviceFrame &Cur, const std::vector<uint8_t> &occupied, const ProjectedQueries &q, const std::vector<float> &vr, float th,
                                  bool bForward, bool bBackward, std::vector<int32_t> &vpMatch) {
        vpMatch.assign(Cur.count(), -1);
        const int mode = bForward ? 1 : (bBackward ? 2 : 0);
        const int r = orbx_frame_search_by_projection_frame_fisheye(
            m_, Cur.handle(), occupied.empty() ? nullptr : occupied.data(), (int)q.u.size(), q.u.data(), q.v.data(), q.ur.data(), vr.data(),
            q.octave.data(), q.angle.data(), q.descriptors.data(), q.hasObservations.empty() ? nullptr : q.hasObservations.data(), th, mode,
            mbCheckOrientation ? 1 : 0, vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_by_projection_frame_fisheye: ") + orbx_status_string(r));
        return r;
    }
    // Tracking::SearchLocalPoints on a rig frame in one call: views[0] / views[1] = left / right camera (isInFrustumChecks), trackDepth = the map
    // points' previous mTrackDepth (read for points only the right camera sees; empty: such a point is never far).  inView [2][n] =
    // mbTrackInView / mbTrackInViewR.
    int SearchLocalPointsFisheye(DeviceFrame &F, const std::vector<uint8_t> &occupied, const orbx_fisheye_view views[2], float logScaleFactor,
                                 float viewingCosLimit, const LocalMapPoints &mps, const std::vector<float> &trackDepth, float th, bool bFarPoints,
                                 float thFarPoints, std::vector<uint8_t> &inView, std::vector<int32_t> &vpMatch) {
        inView.assign(2 * (size_t)mps.size(), 0);
        vpMatch.assign(F.count(), -1);
        const int r = orbx_frame_search_local_points_fisheye(
            m_, F.handle(), occupied.empty() ? nullptr : occupied.data(), views, logScaleFactor, viewingCosLimit, mps.size(), mps.pos.data(),
            mps.normal.data(), mps.minDistance.data(), mps.maxDistance.data(), mps.descriptors.data(), mps.eligible.empty() ? nullptr : mps.eligible.data(),
            mps.hasObservations.empty() ? nullptr : mps.hasObservations.data(), trackDepth.empty() ? nullptr : trackDepth.data(), th, mfNNratio,
            bFarPoints ? 1 : 0, thFarPoints, inView.data(), vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_local_points_fisheye: ") + orbx_status_string(r));
        return r;
    }

    // SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist)
    // (ORBmatcher.cc:1889-2010) and SearchByProjection(KeyFrame*, Sim3f&, vpPoints[, vpPointsKFs], vpMatched[, vpMatchedKF],
    // th, ratioHamming) (ORBmatcher.cc:427-646) share this window form; the adapter projects and fills `q`.
    struct WindowQueries {
        std::vector<float> x, y, r, angle;
        std::vector<int32_t> minLevel, maxLevel;
        std::vector<uint8_t> descriptors;
    };
    int SearchByProjectionWindow(const FrameView &F, const std::vector<uint8_t> &occupied, const WindowQueries &q, float maxDist,
                                 bool checkOrientation, std::vector<int32_t> &vpMatch) {
        vpMatch.assign(F.N, -1);
        orbx_frame_desc fd = F.c();
        const int r = orbx_search_by_projection_window(m_, &fd, occupied.empty() ? nullptr : occupied.data(), (int)q.x.size(), q.x.data(),
                                                       q.y.data(), q.r.data(), q.minLevel.data(), q.maxLevel.data(),
                                                       q.angle.empty() ? nullptr : q.angle.data(), q.descriptors.data(), nullptr, maxDist,
                                                       checkOrientation ? 1 : 0, vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_search_by_projection_window: ") + orbx_status_string(r));
        return r;
    }

    // the same on a resident frame (Relocalization's second stage): vpMatch holds N entries
    int SearchByProjectionWindow(DeviceFrame &F, const std::vector<uint8_t> &occupied, const WindowQueries &q, float maxDist, bool checkOrientation,
                                 std::vector<int32_t> &vpMatch) {
        vpMatch.assign(F.count(), -1);
        const int r = orbx_frame_search_by_projection_window(m_, F.handle(), occupied.empty() ? nullptr : occupied.data(), (int)q.x.size(), q.x.data(),
                                                             q.y.data(), q.r.data(), q.minLevel.data(), q.maxLevel.data(),
                                                             q.angle.empty() ? nullptr : q.angle.data(), q.descriptors.data(), nullptr, maxDist,
                                                             checkOrientation ? 1 : 0, vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_by_projection_window: ") + orbx_status_string(r));
        return r;
    }
    // the same on a resident fisheye-stereo frame (orbx_frame_search_by_projection_window_fisheye): the LEFT camera only (GetFeaturesInArea's
    // default bRight = false); occupied and vpMatch hold N entries, the right camera's entries of vpMatch stay -1
    int SearchByProjectionWindowFisheye(DeviceFrame &F, const std::vector<uint8_t> &occupied, const WindowQueries &q, float maxDist, bool checkOrientation,
                                        std::vector<int32_t> &vpMatch) {
        vpMatch.assign(F.count(), -1);
        const int r = orbx_frame_search_by_projection_window_fisheye(m_, F.handle(), occupied.empty() ? nullptr : occupied.data(), (int)q.x.size(),
                                                                     q.x.data(), q.y.data(), q.r.data(), q.minLevel.data(), q.maxLevel.data(),
                                                                     q.angle.empty() ? nullptr : q.angle.data(), q.descriptors.data(), nullptr, maxDist,
                                                                     checkOrientation ? 1 : 0, vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_by_projection_window_fisheye: ") + orbx_status_string(r));
        return r;
    }

    // SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.cc:648-763)
    int SearchForInitialization(const orbx_keypoint *mvKeysUn1, const uint8_t *mDescriptors1, int N1, const FrameView &F2,
                                std::vector<float> &vbPrevMatchedXY, std::vector<int> &vnMatches12, int windowSize = 10) {
        vnMatches12.assign(N1, -1);
        orbx_frame_desc fd = F2.c();
        const int r = orbx_search_for_initialization(m_, mvKeysUn1, mDescriptors1, N1, &fd, vbPrevMatchedXY.data(), windowSize, mfNNratio,
                                                     mbCheckOrientation ? 1 : 0, vnMatches12.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_search_for_initialization: ") + orbx_status_string(r));
        return r;
    }

    // DBoW2::FeatureVector flattened by the adapter (iterate the std::map in order)
    struct FeatVec {
        std::vector<uint32_t> node_id;
        std::vector<int32_t> node_ptr{0}, index;
        template <class Map> static FeatVec from(const Map &fv) {  // Map = DBoW2::FeatureVector
            FeatVec f;
            for (const auto &kv : fv) {
                f.node_id.push_back((uint32_t)kv.first);
                for (unsigned int i : kv.second) f.index.push_back((int32_t)i);
                f.node_ptr.push_back((int32_t)f.index.size());
            }
            return f;
        }
        orbx_featvec c() const { return orbx_featvec{node_id.data(), node_ptr.data(), index.data(), (int32_t)node_id.size()}; }
    };

    // SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:223-425): vpMatch[iF] = KF feature index or -1
    int SearchByBoW(const uint8_t *descKF, const float *angleKF, const uint8_t *validKF, int nKF, const FeatVec &fvKF,
                    const uint8_t *descF, const float *angleF, int nF, const FeatVec &fvF, std::vector<int32_t> &vpMatch) {
        vpMatch.assign(nF, -1);
        orbx_featvec a = fvKF.c(), b = fvF.c();
        const int r = orbx_search_by_bow_frame(m_, descKF, angleKF, validKF, nKF, &a, descF, angleF, nF, &b, mfNNratio,
                                               mbCheckOrientation ? 1 : 0, vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_search_by_bow_frame: ") + orbx_status_string(r));
        return r;
    }
    // SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) against every key frame of kfs at once on a resident frame after DeviceFrame::ComputeBoW
    // (orbx_frame_search_by_bow): vpMatch[k][iF] = KF feature index or -1, nmatches[k] = the member's return value.  Returns the sum.
    int SearchByBoW(DeviceFrame &F, const std::vector<orbx_bow_keyframe> &kfs, std::vector<int32_t> &nmatches, std::vector<std::vector<int32_t>> &vpMatch) {
        return searchByBoWDevice(F, kfs, nmatches, vpMatch, orbx_frame_search_by_bow, "orbx_frame_search_by_bow");
    }
    // the same for a fisheye-stereo frame after DeviceFrame::ComputeBoWFisheye (orbx_frame_search_by_bow_fisheye, ORBmatcher.cc:283-392):
    // vpMatch[k] holds N entries, a right-camera match at Nleft + j.  kfs[k].angle: mvKeysUn, or mvKeys / mvKeysRight of a fisheye key frame.
    int SearchByBoWFisheye(DeviceFrame &F, const std::vector<orbx_bow_keyframe> &kfs, std::vector<int32_t> &nmatches,
                           std::vector<std::vector<int32_t>> &vpMatch) {
        return searchByBoWDevice(F, kfs, nmatches, vpMatch, orbx_frame_search_by_bow_fisheye, "orbx_frame_search_by_bow_fisheye");
    }
    int searchByBoWDevice(DeviceFrame &F, const std::vector<orbx_bow_keyframe> &kfs, std::vector<int32_t> &nmatches, std::vector<std::vector<int32_t>> &vpMatch,
                          int (*fn)(orbx_matcher *, orbx_frame *, int, const orbx_bow_keyframe *, float, int, int32_t *, int, int32_t *), const char *what) {
        const int nkf = (int)kfs.size();
        const int N = F.count(), stride = std::max(N, 1);
        std::vector<int32_t> rows((size_t)std::max(nkf, 1) * stride, -1);
        nmatches.assign(nkf, 0);
        const int r = fn(m_, F.handle(), nkf, kfs.data(), mfNNratio, mbCheckOrientation ? 1 : 0, rows.data(), stride, nmatches.data());
        if (r < 0) throw std::runtime_error(std::string(what) + ": " + orbx_status_string(r) + " " + orbx_last_error());
        vpMatch.assign(nkf, std::vector<int32_t>());
        int total = 0;
        for (int k = 0; k < nkf; k++) {
            vpMatch[k].assign(rows.begin() + (size_t)k * stride, rows.begin() + (size_t)k * stride + N);
            total += nmatches[k];
        }
        return total;
    }
    // SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:223-425) against resident key frames that carry BoW
    // (orbx_frame_search_by_bow_resident): only valid[k] (GetMapPointMatches()[i] present and !isBad(); an empty vector = all) and one record per
    // key frame are uploaded.  vpMatch[k][iF] = feature of key frame k or -1, nmatches[k] = the member's return value.  Returns the sum.
    int SearchByBoW(DeviceFrame &F, const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<std::vector<uint8_t>> &valid, std::vector<int32_t> &nmatches,
                    std::vector<std::vector<int32_t>> &vpMatch) {
        const size_t K = vpKFs.size();
        if (!valid.empty() && valid.size() != K) throw std::invalid_argument("SearchByBoW: one valid mask per key frame (or none at all)");
        std::vector<orbx_keyframe *> h(K);
        std::vector<const uint8_t *> fl(K, nullptr);
        for (size_t k = 0; k < K; k++) {
            h[k] = vpKFs[k]->handle();
            if (!valid.empty() && !valid[k].empty()) fl[k] = valid[k].data();
        }
        const int N = F.count(), stride = std::max(N, 1);
        std::vector<int32_t> rows(std::max<size_t>(K, 1) * stride, -1);
        nmatches.assign(K, 0);
        // fisheye-stereo key frames go with a fisheye-stereo frame (orbx_frame_search_by_bow_resident_fisheye, ORBmatcher.cc:283-392)
        const auto search = allFisheye(vpKFs, "SearchByBoW") ? orbx_frame_search_by_bow_resident_fisheye : orbx_frame_search_by_bow_resident;
        const int r = search(m_, F.handle(), (int)K, h.data(), fl.data(), mfNNratio, mbCheckOrientation ? 1 : 0, rows.data(), stride, nmatches.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_by_bow_resident: ") + orbx_status_string(r) + " " + orbx_last_error());
        return splitRows(rows, stride, N, nmatches, vpMatch);
    }
    // SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cc:765-905) for KF1 against every key frame of vpKFs2 in one call (orbx_keyframe_search_by_bow;
    // LoopClosing::DetectCommonRegionsFromBoW's loop over a candidate's covisible key frames): vpMatches12[k][i1] = feature of vpKFs2[k] or -1.
    int SearchByBoW(DeviceKeyFrame &KF1, const std::vector<uint8_t> &valid1, const std::vector<DeviceKeyFrame *> &vpKFs2,
                    const std::vector<std::vector<uint8_t>> &valid2, std::vector<int32_t> &nmatches, std::vector<std::vector<int32_t>> &vpMatches12) {
        const size_t K = vpKFs2.size();
        if (!valid2.empty() && valid2.size() != K) throw std::invalid_argument("SearchByBoW: one valid mask per key frame (or none at all)");
        std::vector<orbx_keyframe *> h(K);
        std::vector<const uint8_t *> fl(K, nullptr);
        for (size_t k = 0; k < K; k++) {
            h[k] = vpKFs2[k]->handle();
            if (!valid2.empty() && !valid2[k].empty()) fl[k] = valid2[k].data();
        }
        const int N1 = KF1.count(), stride = std::max(N1, 1);
        std::vector<int32_t> rows(std::max<size_t>(K, 1) * stride, -1);
        nmatches.assign(K, 0);
        // between fisheye-stereo key frames the right camera's features are neither queries nor candidates (:800-802, :820-822)
        std::vector<DeviceKeyFrame *> all(vpKFs2);
        all.push_back(&KF1);
        const auto search = allFisheye(all, "SearchByBoW") ? orbx_keyframe_search_by_bow_fisheye : orbx_keyframe_search_by_bow;
        const int r = search(m_, KF1.handle(), valid1.empty() ? nullptr : valid1.data(), (int)K, h.data(), fl.data(), mfNNratio,
                             mbCheckOrientation ? 1 : 0, rows.data(), stride, nmatches.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_search_by_bow: ") + orbx_status_string(r) + " " + orbx_last_error());
        return splitRows(rows, stride, N1, nmatches, vpMatches12);
    }
    // SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (ORBmatcher.cc:907-1146) between two resident pinhole key frames with both
    // gates on the device (orbx_keyframe_search_for_triangulation): skip1 / skip2 (empty = none) as the host-pointer overloads take them, `gate` = F12,
    // the epipole, bCoarse and pKF2->mvLevelSigma2; everything else is the key frames' own.  One call per neighbour, as CreateNewMapPoints makes them.
    int SearchForTriangulation(DeviceKeyFrame &KF1, DeviceKeyFrame &KF2, const std::vector<uint8_t> &skip1, const std::vector<uint8_t> &skip2,
                               const orbx_keyframe_gate &gate, std::vector<std::pair<size_t, size_t>> &vMatchedPairs) {
        const int n1 = KF1.count();
        std::vector<int32_t> m12((size_t)std::max(n1, 1), -1);
        const int r = orbx_keyframe_search_for_triangulation(m_, KF1.handle(), KF2.handle(), skip1.empty() ? nullptr : skip1.data(),
                                                             skip2.empty() ? nullptr : skip2.data(), mbCheckOrientation ? 1 : 0, &gate, m12.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_search_for_triangulation: ") + orbx_status_string(r) + " " + orbx_last_error());
        vMatchedPairs.clear();
        for (int i = 0; i < n1; i++) if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);  // :1138-1143
        return r;
    }
    // the same member between two resident FISHEYE-STEREO key frames, KannalaBrandt8::epipolarConstrain on the device (:1036-1072;
    // orbx_keyframe_search_for_triangulation_fisheye): `gate` = the level tables, the four cameras' parameters, the four relative poses and bCoarse
    int SearchForTriangulation(DeviceKeyFrame &KF1, DeviceKeyFrame &KF2, const std::vector<uint8_t> &skip1, const std::vector<uint8_t> &skip2,
                               const orbx_keyframe_kb8_gate &gate, std::vector<std::pair<size_t, size_t>> &vMatchedPairs) {
        const int n1 = KF1.count();
        std::vector<int32_t> m12((size_t)std::max(n1, 1), -1);
        const int r = orbx_keyframe_search_for_triangulation_fisheye(m_, KF1.handle(), KF2.handle(), skip1.empty() ? nullptr : skip1.data(),
                                                                     skip2.empty() ? nullptr : skip2.data(), mbCheckOrientation ? 1 : 0, &gate, m12.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_search_for_triangulation_fisheye: ") + orbx_status_string(r) + " " + orbx_last_error());
        vMatchedPairs.clear();
        for (int i = 0; i < n1; i++) if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);  // :1138-1143
        return r;
    }
    // ---- LocalMapping::CreateNewMapPoints' triangulation on the two resident key frames (include/orbx.h restates the member; PARITY UNPINNED).
    // TriangulatePairs: the loop body for the pairs the caller names (orbx_keyframe_triangulate_pairs[_fisheye]; the kind is the view type's).  pos
    // ([n][3]) is resized and only the rows of accepted pairs are written; status [n] = ORBX_NEWPT_*.  Returns the number of accepted pairs.
    int TriangulatePairs(DeviceKeyFrame &KF1, DeviceKeyFrame &KF2, const orbx_new_points_view &view1, const orbx_new_points_view &view2,
                         const orbx_new_points_params &par, const std::vector<int32_t> &idx1, const std::vector<int32_t> &idx2, std::vector<float> &pos,
                         std::vector<uint8_t> &status) {
        const size_t n = NewPointsPairs(idx1, idx2, pos, status);
        int accepted = 0;
        const int r = orbx_keyframe_triangulate_pairs(m_, KF1.handle(), KF2.handle(), &view1, &view2, &par, (int)n, idx1.data(), idx2.data(), pos.data(),
                                                      status.data(), &accepted);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_triangulate_pairs: ") + orbx_status_string(r) + " " + orbx_last_error());
        return accepted;
    }
    int TriangulatePairs(DeviceKeyFrame &KF1, DeviceKeyFrame &KF2, const orbx_fisheye_view views1[2], const orbx_fisheye_view views2[2],
                         const orbx_new_points_params &par, const std::vector<int32_t> &idx1, const std::vector<int32_t> &idx2, std::vector<float> &pos,
                         std::vector<uint8_t> &status) {
        const size_t n = NewPointsPairs(idx1, idx2, pos, status);
        int accepted = 0;
        const int r = orbx_keyframe_triangulate_pairs_fisheye(m_, KF1.handle(), KF2.handle(), views1, views2, &par, (int)n, idx1.data(), idx2.data(),
                                                              pos.data(), status.data(), &accepted);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_triangulate_pairs_fisheye: ") + orbx_status_string(r) + " " + orbx_last_error());
        return accepted;
    }
    // SearchAndTriangulate: SearchForTriangulation(KF1, KF2, ...) above and TriangulatePairs on its matches in ONE call
    // (orbx_keyframe_search_and_triangulate[_fisheye]): one launch more than the search, one synchronisation.  vMatchedPairs as the search fills it;
    // pos [N1][3] / status [N1] are indexed by KF1's feature.  Returns the number of matches; nAccepted the number of ORBX_NEWPT_OK rows.
    int SearchAndTriangulate(DeviceKeyFrame &KF1, DeviceKeyFrame &KF2, const std::vector<uint8_t> &skip1, const std::vector<uint8_t> &skip2,
                             const orbx_keyframe_gate &gate, const orbx_new_points_view &view1, const orbx_new_points_view &view2,
                             const orbx_new_points_params &par, std::vector<std::pair<size_t, size_t>> &vMatchedPairs, std::vector<float> &pos,
                             std::vector<uint8_t> &status, int &nAccepted) {
        const int n1 = KF1.count();
        std::vector<int32_t> m12((size_t)std::max(n1, 1), -1);
        pos.resize(3 * (size_t)std::max(n1, 1)); status.assign((size_t)std::max(n1, 1), (uint8_t)ORBX_NEWPT_NO_MATCH);
        const int r = orbx_keyframe_search_and_triangulate(m_, KF1.handle(), KF2.handle(), skip1.empty() ? nullptr : skip1.data(),
                                                           skip2.empty() ? nullptr : skip2.data(), mbCheckOrientation ? 1 : 0, &gate, &view1, &view2, &par,
                                                           m12.data(), pos.data(), status.data(), &nAccepted);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_search_and_triangulate: ") + orbx_status_string(r) + " " + orbx_last_error());
        vMatchedPairs.clear();
        for (int i = 0; i < n1; i++) if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);  // :1138-1143
        return r;
    }
    int SearchAndTriangulate(DeviceKeyFrame &KF1, DeviceKeyFrame &KF2, const std::vector<uint8_t> &skip1, const std::vector<uint8_t> &skip2,
                             const orbx_keyframe_kb8_gate &gate, const orbx_fisheye_view views1[2], const orbx_fisheye_view views2[2],
                             const orbx_new_points_params &par, std::vector<std::pair<size_t, size_t>> &vMatchedPairs, std::vector<float> &pos,
                             std::vector<uint8_t> &status, int &nAccepted) {
        const int n1 = KF1.count();
        std::vector<int32_t> m12((size_t)std::max(n1, 1), -1);
        pos.resize(3 * (size_t)std::max(n1, 1)); status.assign((size_t)std::max(n1, 1), (uint8_t)ORBX_NEWPT_NO_MATCH);
        const int r = orbx_keyframe_search_and_triangulate_fisheye(m_, KF1.handle(), KF2.handle(), skip1.empty() ? nullptr : skip1.data(),
                                                                   skip2.empty() ? nullptr : skip2.data(), mbCheckOrientation ? 1 : 0, &gate, views1, views2,
                                                                   &par, m12.data(), pos.data(), status.data(), &nAccepted);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_search_and_triangulate_fisheye: ") + orbx_status_string(r) + " " + orbx_last_error());
        vMatchedPairs.clear();
        for (int i = 0; i < n1; i++) if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);  // :1138-1143
        return r;
    }
    // The same two with the member's stereo branches (orbx_keyframe_triangulate_pairs_stereo / orbx_keyframe_search_and_triangulate_stereo; st = mb, mbf of
    // each key frame): a pair with mvuRight >= 0 on a key frame that holds mvDepth (made with DeviceKeyFrame's stereo constructor or from a DeviceFrame
    // with depth) is triangulated or unprojected from its depth on the device; status may be ORBX_NEWPT_UNPROJECT_FAILED.
    int TriangulatePairsStereo(DeviceKeyFrame &KF1, DeviceKeyFrame &KF2, const orbx_new_points_view &view1, const orbx_new_points_view &view2,
                               const orbx_new_points_params &par, const orbx_new_points_stereo &st, const std::vector<int32_t> &idx1,
                               const std::vector<int32_t> &idx2, std::vector<float> &pos, std::vector<uint8_t> &status) {
        const size_t n = NewPointsPairs(idx1, idx2, pos, status);
        int accepted = 0;
        const int r = orbx_keyframe_triangulate_pairs_stereo(m_, KF1.handle(), KF2.handle(), &view1, &view2, &par, &st, (int)n, idx1.data(), idx2.data(),
                                                             pos.data(), status.data(), &accepted);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_triangulate_pairs_stereo: ") + orbx_status_string(r) + " " + orbx_last_error());
        return accepted;
    }
    int SearchAndTriangulateStereo(DeviceKeyFrame &KF1, DeviceKeyFrame &KF2, const std::vector<uint8_t> &skip1, const std::vector<uint8_t> &skip2,
                                   const orbx_keyframe_gate &gate, const orbx_new_points_view &view1, const orbx_new_points_view &view2,
                                   const orbx_new_points_params &par, const orbx_new_points_stereo &st,
                                   std::vector<std::pair<size_t, size_t>> &vMatchedPairs, std::vector<float> &pos, std::vector<uint8_t> &status, int &nAccepted) {
        const int n1 = KF1.count();
        std::vector<int32_t> m12((size_t)std::max(n1, 1), -1);
        pos.resize(3 * (size_t)std::max(n1, 1)); status.assign((size_t)std::max(n1, 1), (uint8_t)ORBX_NEWPT_NO_MATCH);
        const int r = orbx_keyframe_search_and_triangulate_stereo(m_, KF1.handle(), KF2.handle(), skip1.empty() ? nullptr : skip1.data(),
                                                                  skip2.empty() ? nullptr : skip2.data(), mbCheckOrientation ? 1 : 0, &gate, &view1, &view2,
                                                                  &par, &st, m12.data(), pos.data(), status.data(), &nAccepted);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_search_and_triangulate_stereo: ") + orbx_status_string(r) + " " + orbx_last_error());
        vMatchedPairs.clear();
        for (int i = 0; i < n1; i++) if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);  // :1138-1143
        return r;
    }
    static size_t NewPointsPairs(const std::vector<int32_t> &idx1, const std::vector<int32_t> &idx2, std::vector<float> &pos, std::vector<uint8_t> &status) {
        if (idx1.size() != idx2.size()) throw std::invalid_argument("TriangulatePairs: one index of each key frame per pair");
        pos.resize(3 * idx1.size()); status.assign(idx1.size(), (uint8_t)ORBX_NEWPT_NO_MATCH);
        return idx1.size();
    }
    // the kind of a list of resident key frames: all fisheye-stereo or none (a mixed list throws, as Fuse does)
    static bool allFisheye(const std::vector<DeviceKeyFrame *> &kfs, const char *who) {
        size_t n = 0;
        for (const DeviceKeyFrame *kf : kfs) n += kf && kf->fisheye() ? 1 : 0;
        if (n != 0 && n != kfs.size()) throw std::invalid_argument(std::string(who) + ": fisheye-stereo and monocular key frames in one call");
        return n != 0;
    }
    static int splitRows(const std::vector<int32_t> &rows, int stride, int n, const std::vector<int32_t> &nmatches, std::vector<std::vector<int32_t>> &out) {
        out.assign(nmatches.size(), std::vector<int32_t>());
        int total = 0;
        for (size_t k = 0; k < nmatches.size(); k++) {
            out[k].assign(rows.begin() + k * (size_t)stride, rows.begin() + k * (size_t)stride + n);
            total += nmatches[k];
        }
        return total;
    }
    // SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (ORBmatcher.cc:765-905): vpMatches12[i1] = i2 or -1
    int SearchByBoW(const uint8_t *desc1, const float *angle1, const uint8_t *valid1, int n1, const FeatVec &fv1, const uint8_t *desc2,
                    const float *angle2, const uint8_t *valid2, int n2, const FeatVec &fv2, std::vector<int32_t> &vpMatches12) {
        vpMatches12.assign(n1, -1);
        orbx_featvec a = fv1.c(), b = fv2.c();
        const int r = orbx_search_by_bow_keyframes(m_, desc1, angle1, valid1, n1, &a, desc2, angle2, valid2, n2, &b, mfNNratio,
                                                   mbCheckOrientation ? 1 : 0, vpMatches12.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_search_by_bow_keyframes: ") + orbx_status_string(r));
        return r;
    }
    // SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (ORBmatcher.cc:907-1146).  `gate` is a callable
    // bool(size_t idx1, size_t idx2) holding the reference's epipole-distance test and pCamera1->epipolarConstrain(...) (or
    // `return true` for bCoarse) -- unchanged host float math.
    template <class Gate>
    int SearchForTriangulation(const uint8_t *desc1, const float *angle1, const uint8_t *skip1, int n1, const FeatVec &fv1,
                               const uint8_t *desc2, const float *angle2, const uint8_t *skip2, int n2, const FeatVec &fv2, Gate gate,
                               std::vector<std::pair<size_t, size_t>> &vMatchedPairs) {
        std::vector<int32_t> m12(n1, -1);
        orbx_featvec a = fv1.c(), b = fv2.c();
        auto thunk = [](void *user, int i1, int i2) -> int { return (*static_cast<Gate *>(user))((size_t)i1, (size_t)i2) ? 1 : 0; };
        const int r = orbx_search_for_triangulation(m_, desc1, angle1, skip1, n1, &a, desc2, angle2, skip2, n2, &b,
                                                    mbCheckOrientation ? 1 : 0, thunk, &gate, m12.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_search_for_triangulation: ") + orbx_status_string(r));
        vMatchedPairs.clear();
        for (int i = 0; i < n1; i++) if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);  // :1138-1143
        return r;
    }

    // The same for pinhole key frames with both gates on the device (no callback): `gate` carries mvKeysUn / mvuRight of both key frames,
    // pKF2's mvScaleFactors / mvLevelSigma2, the epipole (:919-921) and F12 = K1^-T [t12]x R12 K2^-1 computed by the caller's Eigen as
    // Pinhole::epipolarConstrain (CameraModels/Pinhole.cpp:107-112) does; bCoarse = gate.coarse.
    int SearchForTriangulation(const uint8_t *desc1, const uint8_t *skip1, int n1, const FeatVec &fv1, const uint8_t *desc2,
                               const uint8_t *skip2, int n2, const FeatVec &fv2, const orbx_pinhole_gate &gate,
                               std::vector<std::pair<size_t, size_t>> &vMatchedPairs) {
        std::vector<int32_t> m12(n1, -1);
        orbx_featvec a = fv1.c(), b = fv2.c();
        const int r = orbx_search_for_triangulation_pinhole(m_, desc1, skip1, n1, &a, desc2, skip2, n2, &b, mbCheckOrientation ? 1 : 0, &gate,
                                                            m12.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_search_for_triangulation_pinhole: ") + orbx_status_string(r));
        vMatchedPairs.clear();
        for (int i = 0; i < n1; i++) if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);
        return r;
    }

    // Matching core of Fuse(KeyFrame*, vpMapPoints, th, bRight) (ORBmatcher.cc:1148-1337) and Fuse(KeyFrame*, Sim3f&, vpPoints, th,
    // vpReplacePoint) (:1339-1455).  The caller projects the map points exactly as :1186-1244 / :1376-1403 do (host float math), passes
    // the survivors, and afterwards runs the reference's own tail on (bestIdx[i], bestDist[i] <= TH_LOW): Replace / AddObservation /
    // AddMapPoint (:1309-1330) or vpReplacePoint[iMP] = pMPinKF (:1436-1449).  mvInvLevelSigma2 = nullptr selects the Sim3 overload
    // (no chi2 gate).
    struct FuseQueries {
        std::vector<float> u, v, ur, radius;   // radius = th * pKF->mvScaleFactors[nPredictedLevel]
        std::vector<int32_t> nPredictedLevel;
        std::vector<uint8_t> descriptors;      // 32 B each (pMP->GetDescriptor())
    };
    void FuseSearch(const FrameView &KF, const float *mvInvLevelSigma2, const FuseQueries &q, std::vector<int32_t> &bestIdx,
                    std::vector<int32_t> &bestDist, bool strictFloat = false) {
        const int nq = (int)q.u.size();
        bestIdx.assign(nq, -1); bestDist.assign(nq, 256);
        orbx_frame_desc fd = KF.c();
        const int r = orbx_fuse_search(m_, &fd, mvInvLevelSigma2, nq, q.u.data(), q.v.data(), q.ur.empty() ? nullptr : q.ur.data(),
                                       q.radius.data(), q.nPredictedLevel.data(), q.descriptors.data(), strictFloat ? 1 : 0, bestIdx.data(),
                                       bestDist.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_fuse_search: ") + orbx_status_string(r));
    }

    // FuseSearch for K resident key frames in ONE call (orbx_keyframe_fuse_search): key frame k with its own query set q[k]; useChi2 = the first
    // overload's reprojection gate with the key frames' mvInvLevelSigma2, false = the gate-less form (Fuse with a Sim3, SearchBySim3).
    // bestIdx[k] / bestDist[k] equal FuseSearch on key frame k's host arrays.
    void FuseSearchKeyFrames(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<FuseQueries> &q, bool useChi2,
                             std::vector<std::vector<int32_t>> &bestIdx, std::vector<std::vector<int32_t>> &bestDist, bool strictFloat = false) {
        const size_t K = vpKFs.size();
        if (q.size() != K) throw std::invalid_argument("FuseSearchKeyFrames: one query set per key frame");
        std::vector<orbx_keyframe *> h(K);
        std::vector<orbx_fuse_queries> c(K);
        std::vector<int32_t *> pi(K), pd(K);
        bestIdx.assign(K, {}); bestDist.assign(K, {});
        for (size_t k = 0; k < K; k++) {
            const int nq = (int)q[k].u.size();
            h[k] = vpKFs[k]->handle();
            c[k] = orbx_fuse_queries{nq, q[k].u.data(), q[k].v.data(), q[k].ur.empty() ? nullptr : q[k].ur.data(), q[k].radius.data(),
                                     q[k].nPredictedLevel.data(), q[k].descriptors.data()};
            bestIdx[k].assign(nq, -1); bestDist[k].assign(nq, 256);
            pi[k] = bestIdx[k].data(); pd[k] = bestDist[k].data();
        }
        const int r = orbx_keyframe_fuse_search(m_, (int)K, h.data(), c.data(), useChi2 ? 1 : 0, strictFloat ? 1 : 0, pi.data(), pd.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_fuse_search: ") + orbx_status_string(r));
    }

    // The Fuse loop of LocalMapping::SearchInNeighbors in ONE call, projection included (orbx_keyframe_fuse_map_points): Fuse(pKF, vpMapPoints, th)
    // (ORBmatcher.cc:1148-1337) up to and including the candidate loop for every target key frame.  cams[k] / poses[k] = pKF_k's intrinsics + mbf and
    // GetPose() / GetCameraCenter(); the map points flat and given once (mfMinDistance / mfMaxDistance UNSCALED: the device applies 0.8f / 1.2f);
    // skip [K][n] (empty = none) = !pMP || isBad() || IsInKeyFrame(pKF_k).  bestIdx / bestDist / projected: [K][n], row-major.
    struct FuseMapPointSet {
        std::vector<float> pos, normal;              // 3 floats each: GetWorldPos(), GetNormal()
        std::vector<float> minDistance, maxDistance; // mfMinDistance, mfMaxDistance
        std::vector<uint8_t> descriptors;            // n x 32
        int size() const { return (int)minDistance.size(); }
    };
    void FuseMapPoints(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<orbx_camera> &cams, const std::vector<orbx_frame_pose> &poses,
                       const FuseMapPointSet &mps, const std::vector<uint8_t> &skip, float th, float logScaleFactor, std::vector<int32_t> &bestIdx,
                       std::vector<int32_t> &bestDist, std::vector<uint8_t> *projected = nullptr, bool strictFloat = false) {
        const size_t K = vpKFs.size(), n = (size_t)mps.size();
        if (cams.size() != K || poses.size() != K || (!skip.empty() && skip.size() != K * n))
            throw std::invalid_argument("FuseMapPoints: one camera and pose per key frame, K x n skip flags");
        std::vector<orbx_keyframe *> h(K);
        for (size_t k = 0; k < K; k++) h[k] = vpKFs[k]->handle();
        bestIdx.assign(K * n, -1); bestDist.assign(K * n, 256);
        if (projected) projected->assign(K * n, 0);
        const int r = orbx_keyframe_fuse_map_points(m_, (int)K, h.data(), cams.data(), poses.data(), th, logScaleFactor, strictFloat ? 1 : 0, (int)n,
                                                    mps.pos.data(), mps.normal.data(), mps.minDistance.data(), mps.maxDistance.data(),
                                                    mps.descriptors.data(), skip.empty() ? nullptr : skip.data(), bestIdx.data(), bestDist.data(),
                                                    projected ? projected->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_fuse_map_points: ") + orbx_status_string(r));
    }

    // LoopClosing's Sim3 searches on resident key frames (monocular / rectified, Pinhole).  poses[k] = Tcw = SE3f(Scw.rotationMatrix(),
    // Scw.translation() / Scw.scale()) and Ow = Tcw.inverse().translation(), as the reference evaluates them; the gates run on the device.
    //
    // SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (ORBmatcher.cc:427-532; projectionForm ORBX_SIM3_PROJECT_CAMERA) or its
    // vpPointsKFs overload (:534-646; ORBX_SIM3_PROJECT_INVZ) for K key frames with ONE shared point set in one call
    // (orbx_keyframe_search_by_projection_sim3).  skip [K][n] (empty = none) = isBad() || spAlreadyFound.count(pMP) for key frame k; occupied: empty, or
    // K rows, each empty or N_k flags vpMatched[i] != NULL.  vpMatch[k][i] = the index into the point set assigned to feature i of key frame k, or -1;
    // vnMatches[k] = the member's return value.  The key frames of one call must have equal image bounds (std::runtime_error otherwise: split the list).
    void SearchByProjectionSim3KeyFrames(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<orbx_camera> &cams,
                                         const std::vector<orbx_frame_pose> &poses, const FuseMapPointSet &mps, const std::vector<uint8_t> &skip,
                                         const std::vector<std::vector<uint8_t>> &occupied, float th, float ratioHamming, float logScaleFactor,
                                         int projectionForm, std::vector<std::vector<int32_t>> &vpMatch, std::vector<int> &vnMatches,
                                         std::vector<uint8_t> *projected = nullptr) {
        const size_t K = vpKFs.size(), n = (size_t)mps.size();
        if (cams.size() != K || poses.size() != K || (!skip.empty() && skip.size() != K * n) || (!occupied.empty() && occupied.size() != K))
            throw std::invalid_argument("SearchByProjectionSim3KeyFrames: one camera and pose per key frame, K x n skip flags, K occupancy rows");
        std::vector<orbx_keyframe *> h(K);
        std::vector<const uint8_t *> occ(K, nullptr);
        std::vector<int32_t *> rows(K);
        std::vector<int32_t> nm(K, 0);
        vpMatch.assign(K, {});
        for (size_t k = 0; k < K; k++) {
            h[k] = vpKFs[k]->handle();
            const size_t N = (size_t)vpKFs[k]->count();
            if (!occupied.empty() && !occupied[k].empty()) {
                if (occupied[k].size() != N) throw std::invalid_argument("SearchByProjectionSim3KeyFrames: an occupancy row holds N_k flags");
                occ[k] = occupied[k].data();
            }
            vpMatch[k].assign(N + 1, -1);   // (+ 1: data() of an empty row may be NULL, which the call refuses)
            rows[k] = vpMatch[k].data();
        }
        if (projected) projected->assign(K * n, 0);
        const int r = orbx_keyframe_search_by_projection_sim3(m_, (int)K, h.data(), cams.data(), poses.data(), th, ratioHamming, logScaleFactor,
                                                              projectionForm, (int)n, mps.pos.data(), mps.normal.data(), mps.minDistance.data(),
                                                              mps.maxDistance.data(), mps.descriptors.data(), skip.empty() ? nullptr : skip.data(),
                                                              occupied.empty() ? nullptr : occ.data(), rows.data(), nm.data(),
                                                              projected ? projected->data() : nullptr, nullptr, nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_search_by_projection_sim3: ") + orbx_status_string(r));
        for (size_t k = 0; k < K; k++) vpMatch[k].pop_back();
        vnMatches.assign(nm.begin(), nm.end());
    }

    // The loop of LoopClosing::SearchAndFuse -- Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:1339-1455) per key frame of
    // CorrectedPosesMap -- in ONE call, projection included (orbx_keyframe_fuse_map_points_sim3): the gate-less candidate search, no mvuRight.
    // skip [K][n] (empty = none) = isBad() || pKF_k->GetMapPoints().count(pMP).  bestIdx / bestDist / projected: [K][n], row-major.
    void FuseMapPointsSim3(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<orbx_camera> &cams, const std::vector<orbx_frame_pose> &poses,
                           const FuseMapPointSet &mps, const std::vector<uint8_t> &skip, float th, float logScaleFactor, std::vector<int32_t> &bestIdx,
                           std::vector<int32_t> &bestDist, std::vector<uint8_t> *projected = nullptr) {
        const size_t K = vpKFs.size(), n = (size_t)mps.size();
        if (cams.size() != K || poses.size() != K || (!skip.empty() && skip.size() != K * n))
            throw std::invalid_argument("FuseMapPointsSim3: one camera and pose per key frame, K x n skip flags");
        std::vector<orbx_keyframe *> h(K);
        for (size_t k = 0; k < K; k++) h[k] = vpKFs[k]->handle();
        bestIdx.assign(K * n, -1); bestDist.assign(K * n, 256);
        if (projected) projected->assign(K * n, 0);
        const int r = orbx_keyframe_fuse_map_points_sim3(m_, (int)K, h.data(), cams.data(), poses.data(), th, logScaleFactor, (int)n, mps.pos.data(),
                                                         mps.normal.data(), mps.minDistance.data(), mps.maxDistance.data(), mps.descriptors.data(),
                                                         skip.empty() ? nullptr : skip.data(), bestIdx.data(), bestDist.data(),
                                                         projected ? projected->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_fuse_map_points_sim3: ") + orbx_status_string(r));
    }

    // The two calls above for K FISHEYE-STEREO key frames (orbx_keyframe_search_by_projection_sim3_fisheye / orbx_keyframe_fuse_map_points_sim3_fisheye):
    // the members read the LEFT camera only, so views holds K entries, one per key frame -- R, t = Tcw = SE3f(Scw.rotationMatrix(), Scw.translation() /
    // Scw.scale()), twc = Tcw.inverse().translation(), params = mpCamera's eight (KannalaBrandt8; ORBX_SIM3_PROJECT_INVZ: params[0..3] = pKF->fx, fy,
    // cx, cy).  occupied rows and vpMatch[k] hold N_k = N_left + N_right entries as vpMatched does on a rig; only indices below N_left are read or set.
    void SearchByProjectionSim3KeyFramesFisheye(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<orbx_fisheye_view> &views,
                                                const FuseMapPointSet &mps, const std::vector<uint8_t> &skip,
                                                const std::vector<std::vector<uint8_t>> &occupied, float th, float ratioHamming, float logScaleFactor,
                                                int projectionForm, std::vector<std::vector<int32_t>> &vpMatch, std::vector<int> &vnMatches,
                                                std::vector<uint8_t> *projected = nullptr) {
        const size_t K = vpKFs.size(), n = (size_t)mps.size();
        if (views.size() != K || (!skip.empty() && skip.size() != K * n) || (!occupied.empty() && occupied.size() != K))
            throw std::invalid_argument("SearchByProjectionSim3KeyFramesFisheye: one view per key frame, K x n skip flags, K occupancy rows");
        std::vector<orbx_keyframe *> h(K);
        std::vector<const uint8_t *> occ(K, nullptr);
        std::vector<int32_t *> rows(K);
        std::vector<int32_t> nm(K, 0);
        vpMatch.assign(K, {});
        for (size_t k = 0; k < K; k++) {
            h[k] = vpKFs[k]->handle();
            const size_t N = (size_t)vpKFs[k]->count();
            if (!occupied.empty() && !occupied[k].empty()) {
                if (occupied[k].size() != N) throw std::invalid_argument("SearchByProjectionSim3KeyFramesFisheye: an occupancy row holds N_k flags");
                occ[k] = occupied[k].data();
            }
            vpMatch[k].assign(N + 1, -1);   // (+ 1: data() of an empty row may be NULL, which the call refuses)
            rows[k] = vpMatch[k].data();
        }
        if (projected) projected->assign(K * n, 0);
        const int r = orbx_keyframe_search_by_projection_sim3_fisheye(m_, (int)K, h.data(), views.data(), th, ratioHamming, logScaleFactor, projectionForm,
                                                                      (int)n, mps.pos.data(), mps.normal.data(), mps.minDistance.data(),
                                                                      mps.maxDistance.data(), mps.descriptors.data(), skip.empty() ? nullptr : skip.data(),
                                                                      occupied.empty() ? nullptr : occ.data(), rows.data(), nm.data(),
                                                                      projected ? projected->data() : nullptr, nullptr, nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_search_by_projection_sim3_fisheye: ") + orbx_status_string(r));
        for (size_t k = 0; k < K; k++) vpMatch[k].pop_back();
        vnMatches.assign(nm.begin(), nm.end());
    }
    // bestIdx (always below N_left) / bestDist / projected: [K][n], row-major.
    void FuseMapPointsSim3Fisheye(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<orbx_fisheye_view> &views, const FuseMapPointSet &mps,
                                  const std::vector<uint8_t> &skip, float th, float logScaleFactor, std::vector<int32_t> &bestIdx,
                                  std::vector<int32_t> &bestDist, std::vector<uint8_t> *projected = nullptr) {
        const size_t K = vpKFs.size(), n = (size_t)mps.size();
        if (views.size() != K || (!skip.empty() && skip.size() != K * n))
            throw std::invalid_argument("FuseMapPointsSim3Fisheye: one view per key frame, K x n skip flags");
        std::vector<orbx_keyframe *> h(K);
        for (size_t k = 0; k < K; k++) h[k] = vpKFs[k]->handle();
        bestIdx.assign(K * n, -1); bestDist.assign(K * n, 256);
        if (projected) projected->assign(K * n, 0);
        const int r = orbx_keyframe_fuse_map_points_sim3_fisheye(m_, (int)K, h.data(), views.data(), th, logScaleFactor, (int)n, mps.pos.data(),
                                                                 mps.normal.data(), mps.minDistance.data(), mps.maxDistance.data(),
                                                                 mps.descriptors.data(), skip.empty() ? nullptr : skip.data(), bestIdx.data(),
                                                                 bestDist.data(), projected ? projected->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_fuse_map_points_sim3_fisheye: ") + orbx_status_string(r));
    }

    // FuseSearchKeyFrames for K fisheye-stereo key frames (orbx_keyframe_fuse_search_fisheye): q / bestIdx / bestDist hold 2 K entries, 2 k = key frame
    // k's left-camera set, 2 k + 1 its right-camera set (ur is not read).  A right-camera index is NLeft + j (ORBmatcher.cc:1296).
    void FuseSearchKeyFramesFisheye(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<FuseQueries> &q, bool useChi2,
                                    std::vector<std::vector<int32_t>> &bestIdx, std::vector<std::vector<int32_t>> &bestDist, bool strictFloat = false) {
        const size_t K = vpKFs.size();
        if (q.size() != 2 * K) throw std::invalid_argument("FuseSearchKeyFramesFisheye: a left and a right query set per key frame");
        std::vector<orbx_keyframe *> h(K);
        std::vector<orbx_fuse_queries> c(2 * K);
        std::vector<int32_t *> pi(2 * K), pd(2 * K);
        bestIdx.assign(2 * K, {}); bestDist.assign(2 * K, {});
        for (size_t k = 0; k < K; k++) h[k] = vpKFs[k]->handle();
        for (size_t p = 0; p < 2 * K; p++) {
            const int nq = (int)q[p].u.size();
            c[p] = orbx_fuse_queries{nq, q[p].u.data(), q[p].v.data(), nullptr, q[p].radius.data(), q[p].nPredictedLevel.data(), q[p].descriptors.data()};
            bestIdx[p].assign(nq, -1); bestDist[p].assign(nq, 256);
            pi[p] = bestIdx[p].data(); pd[p] = bestDist[p].data();
        }
        const int r = orbx_keyframe_fuse_search_fisheye(m_, (int)K, h.data(), c.data(), useChi2 ? 1 : 0, strictFloat ? 1 : 0, pi.data(), pd.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_fuse_search_fisheye: ") + orbx_status_string(r));
    }

    // BOTH Fuse calls of LocalMapping::SearchInNeighbors' loop on a rig -- Fuse(pKFi, vpMapPointMatches) and Fuse(pKFi, vpMapPointMatches, true) -- for
    // every target in ONE call, projection included (orbx_keyframe_fuse_map_points_fisheye).  views [K][2]: GetPose() / GetCameraCenter() / mpCamera's
    // parameters, then GetRightPose() / GetRightCameraCenter() / mpCamera2's; skip [K][n] (empty = none), one row per key frame for both cameras.
    // bestIdx (the rig's numbering) / bestDist / projected: [K][2][n], row-major.
    void FuseMapPointsFisheye(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<orbx_fisheye_view> &views, const FuseMapPointSet &mps,
                              const std::vector<uint8_t> &skip, float th, float logScaleFactor, std::vector<int32_t> &bestIdx,
                              std::vector<int32_t> &bestDist, std::vector<uint8_t> *projected = nullptr, bool strictFloat = false) {
        const size_t K = vpKFs.size(), n = (size_t)mps.size();
        if (views.size() != 2 * K || (!skip.empty() && skip.size() != K * n))
            throw std::invalid_argument("FuseMapPointsFisheye: two views per key frame, K x n skip flags");
        std::vector<orbx_keyframe *> h(K);
        for (size_t k = 0; k < K; k++) h[k] = vpKFs[k]->handle();
        bestIdx.assign(2 * K * n, -1); bestDist.assign(2 * K * n, 256);
        if (projected) projected->assign(2 * K * n, 0);
        const int r = orbx_keyframe_fuse_map_points_fisheye(m_, (int)K, h.data(), views.data(), th, logScaleFactor, strictFloat ? 1 : 0, (int)n,
                                                            mps.pos.data(), mps.normal.data(), mps.minDistance.data(), mps.maxDistance.data(),
                                                            mps.descriptors.data(), skip.empty() ? nullptr : skip.data(), bestIdx.data(),
                                                            bestDist.data(), projected ? projected->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_fuse_map_points_fisheye: ") + orbx_status_string(r));
    }

    // SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (ORBmatcher.cc:1457-1674): the two projection searches are gate-less fuse searches
    // (KeyFrame::GetFeaturesInArea, octave gate [l-1,l], first minimum wins, accept bestDist <= TH_HIGH :1569/:1656), followed by the
    // mutual-agreement pass (:1662-1675).  q1 = KF1's map points transformed by S21 and projected into KF2 (one entry per KF1 feature,
    // radius = th * pKF2->mvScaleFactors[level]); q2 = the converse.  use1[i] / use2[i] == 0 drops a slot (no / bad map point,
    // vbAlreadyMatched, failed depth / image / distance gate :1495-1527).  vnMatch12[i1] = KF2 feature index or -1; returns nFound.
    int SearchBySim3(const FrameView &KF1, const FrameView &KF2, const FuseQueries &q1, const std::vector<uint8_t> &use1,
                     const FuseQueries &q2, const std::vector<uint8_t> &use2, std::vector<int32_t> &vnMatch12) {
        std::vector<int32_t> bi1, bd1, bi2, bd2;
        FuseSearch(KF2, nullptr, q1, bi1, bd1);
        FuseSearch(KF1, nullptr, q2, bi2, bd2);
        const int n1 = (int)bi1.size(), n2 = (int)bi2.size();
        vnMatch12.assign(n1, -1);
        int nFound = 0;
        for (int i1 = 0; i1 < n1; i1++) {
            if (!use1[i1] || bd1[i1] > TH_HIGH || bi1[i1] < 0) continue;
            const int idx2 = bi1[i1];
            if (idx2 >= n2 || !use2[idx2] || bd2[idx2] > TH_HIGH) continue;
            if (bi2[idx2] == i1) { vnMatch12[i1] = idx2; nFound++; }
        }
        return nFound;
    }

    // ---- The one-call searches with their map points resident (DeviceMap): ids[j] names the slot of map point j; eligible / hasObservations / skip /
    // trackDepth, inView and projected stay positional (entry j belongs to ids[j]) and every output indexes POSITIONS in ids.  Results as the
    // overloads that take the arrays, given the slots' rows.
    int SearchLocalPoints(DeviceFrame &F, const std::vector<uint8_t> &occupied, const orbx_camera &cam, const orbx_frame_pose &pose, float logScaleFactor,
                          float viewingCosLimit, const DeviceMap &map, const std::vector<int32_t> &ids, const std::vector<uint8_t> &eligible,
                          const std::vector<uint8_t> &hasObservations, float th, bool bFarPoints, float thFarPoints, std::vector<uint8_t> &inView,
                          std::vector<int32_t> &vpMatch) {
        inView.assign(ids.size(), 0);
        vpMatch.assign(F.count(), -1);
        const int r = orbx_frame_search_local_points_map(m_, F.handle(), occupied.empty() ? nullptr : occupied.data(), &cam, &pose, logScaleFactor,
                                                         viewingCosLimit, (int)ids.size(), map.handle(), ids.data(),
                                                         eligible.empty() ? nullptr : eligible.data(), hasObservations.empty() ? nullptr : hasObservations.data(),
                                                         th, mfNNratio, bFarPoints ? 1 : 0, thFarPoints, inView.data(), vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_local_points_map: ") + orbx_status_string(r));
        return r;
    }
    int SearchLocalPointsFisheye(DeviceFrame &F, const std::vector<uint8_t> &occupied, const orbx_fisheye_view views[2], float logScaleFactor,
                                 float viewingCosLimit, const DeviceMap &map, const std::vector<int32_t> &ids, const std::vector<uint8_t> &eligible,
                                 const std::vector<uint8_t> &hasObservations, const std::vector<float> &trackDepth, float th, bool bFarPoints,
                                 float thFarPoints, std::vector<uint8_t> &inView, std::vector<int32_t> &vpMatch) {
        inView.assign(2 * ids.size(), 0);
        vpMatch.assign(F.count(), -1);
        const int r = orbx_frame_search_local_points_fisheye_map(
            m_, F.handle(), occupied.empty() ? nullptr : occupied.data(), views, logScaleFactor, viewingCosLimit, (int)ids.size(), map.handle(), ids.data(),
            eligible.empty() ? nullptr : eligible.data(), hasObservations.empty() ? nullptr : hasObservations.data(),
            trackDepth.empty() ? nullptr : trackDepth.data(), th, mfNNratio, bFarPoints ? 1 : 0, thFarPoints, inView.data(), vpMatch.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_local_points_fisheye_map: ") + orbx_status_string(r));
        return r;
    }
    void FuseMapPoints(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<orbx_camera> &cams, const std::vector<orbx_frame_pose> &poses,
                       const DeviceMap &map, const std::vector<int32_t> &ids, const std::vector<uint8_t> &skip, float th, float logScaleFactor,
                       std::vector<int32_t> &bestIdx, std::vector<int32_t> &bestDist, std::vector<uint8_t> *projected = nullptr, bool strictFloat = false) {
        const size_t K = vpKFs.size(), n = ids.size();
        if (cams.size() != K || poses.size() != K) throw std::invalid_argument("FuseMapPoints: one camera and pose per key frame");
        const std::vector<orbx_keyframe *> h = mapCallHandles(vpKFs, K, n, skip, bestIdx, bestDist, projected);
        const int r = orbx_keyframe_fuse_map_points_map(m_, (int)K, h.data(), cams.data(), poses.data(), th, logScaleFactor, strictFloat ? 1 : 0, (int)n,
                                                        map.handle(), ids.data(), skip.empty() ? nullptr : skip.data(), bestIdx.data(), bestDist.data(),
                                                        projected ? projected->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_fuse_map_points_map: ") + orbx_status_string(r));
    }
    // views: 2 K entries (left, right per key frame); bestIdx / bestDist / projected [K][2][n]
    void FuseMapPointsFisheye(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<orbx_fisheye_view> &views, const DeviceMap &map,
                              const std::vector<int32_t> &ids, const std::vector<uint8_t> &skip, float th, float logScaleFactor,
                              std::vector<int32_t> &bestIdx, std::vector<int32_t> &bestDist, std::vector<uint8_t> *projected = nullptr,
                              bool strictFloat = false) {
        const size_t K = vpKFs.size(), n = ids.size();
        if (views.size() != 2 * K) throw std::invalid_argument("FuseMapPointsFisheye: a left and a right view per key frame");
        const std::vector<orbx_keyframe *> h = mapCallHandles(vpKFs, K, n, skip, bestIdx, bestDist, projected, 2);
        const int r = orbx_keyframe_fuse_map_points_fisheye_map(m_, (int)K, h.data(), views.data(), th, logScaleFactor, strictFloat ? 1 : 0, (int)n,
                                                                map.handle(), ids.data(), skip.empty() ? nullptr : skip.data(), bestIdx.data(),
                                                                bestDist.data(), projected ? projected->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_fuse_map_points_fisheye_map: ") + orbx_status_string(r));
    }
    void FuseMapPointsSim3(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<orbx_camera> &cams, const std::vector<orbx_frame_pose> &poses,
                           const DeviceMap &map, const std::vector<int32_t> &ids, const std::vector<uint8_t> &skip, float th, float logScaleFactor,
                           std::vector<int32_t> &bestIdx, std::vector<int32_t> &bestDist, std::vector<uint8_t> *projected = nullptr) {
        const size_t K = vpKFs.size(), n = ids.size();
        if (cams.size() != K || poses.size() != K) throw std::invalid_argument("FuseMapPointsSim3: one camera and pose per key frame");
        const std::vector<orbx_keyframe *> h = mapCallHandles(vpKFs, K, n, skip, bestIdx, bestDist, projected);
        const int r = orbx_keyframe_fuse_map_points_sim3_map(m_, (int)K, h.data(), cams.data(), poses.data(), th, logScaleFactor, (int)n, map.handle(),
                                                             ids.data(), skip.empty() ? nullptr : skip.data(), bestIdx.data(), bestDist.data(),
                                                             projected ? projected->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_fuse_map_points_sim3_map: ") + orbx_status_string(r));
    }
    void FuseMapPointsSim3Fisheye(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<orbx_fisheye_view> &views, const DeviceMap &map,
                                  const std::vector<int32_t> &ids, const std::vector<uint8_t> &skip, float th, float logScaleFactor,
                                  std::vector<int32_t> &bestIdx, std::vector<int32_t> &bestDist, std::vector<uint8_t> *projected = nullptr) {
        const size_t K = vpKFs.size(), n = ids.size();
        if (views.size() != K) throw std::invalid_argument("FuseMapPointsSim3Fisheye: one (left) view per key frame");
        const std::vector<orbx_keyframe *> h = mapCallHandles(vpKFs, K, n, skip, bestIdx, bestDist, projected);
        const int r = orbx_keyframe_fuse_map_points_sim3_fisheye_map(m_, (int)K, h.data(), views.data(), th, logScaleFactor, (int)n, map.handle(), ids.data(),
                                                                     skip.empty() ? nullptr : skip.data(), bestIdx.data(), bestDist.data(),
                                                                     projected ? projected->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_fuse_map_points_sim3_fisheye_map: ") + orbx_status_string(r));
    }
    // cams / poses [K] of monocular key frames, or (cams empty) views [K] of rig key frames: orbx_keyframe_search_by_projection_sim3[_fisheye]_map
    void SearchByProjectionSim3KeyFrames(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<orbx_camera> &cams,
                                         const std::vector<orbx_frame_pose> &poses, const std::vector<orbx_fisheye_view> &views, const DeviceMap &map,
                                         const std::vector<int32_t> &ids, const std::vector<uint8_t> &skip, const std::vector<std::vector<uint8_t>> &occupied,
                                         float th, float ratioHamming, float logScaleFactor, int projectionForm, std::vector<std::vector<int32_t>> &vpMatch,
                                         std::vector<int> &vnMatches, std::vector<uint8_t> *projected = nullptr) {
        const size_t K = vpKFs.size(), n = ids.size();
        const bool rig = cams.empty() && K > 0;
        if ((rig ? views.size() != K : cams.size() != K || poses.size() != K) || (!skip.empty() && skip.size() != K * n) ||
            (!occupied.empty() && occupied.size() != K))
            throw std::invalid_argument("SearchByProjectionSim3KeyFrames: one camera and pose (or one view) per key frame, K x n skip flags, K occupancy rows");
        std::vector<orbx_keyframe *> h(K);
        std::vector<const uint8_t *> occ(K, nullptr);
        std::vector<int32_t *> rows(K);
        std::vector<int32_t> nm(K, 0);
        vpMatch.assign(K, {});
        for (size_t k = 0; k < K; k++) {
            h[k] = vpKFs[k]->handle();
            const size_t N = (size_t)vpKFs[k]->count();
            if (!occupied.empty() && !occupied[k].empty()) {
                if (occupied[k].size() != N) throw std::invalid_argument("SearchByProjectionSim3KeyFrames: an occupancy row holds N_k flags");
                occ[k] = occupied[k].data();
            }
            vpMatch[k].assign(N + 1, -1);   // (+ 1: data() of an empty row may be NULL, which the call refuses)
            rows[k] = vpMatch[k].data();
        }
        if (projected) projected->assign(K * n, 0);
        const int r = rig ? orbx_keyframe_search_by_projection_sim3_fisheye_map(m_, (int)K, h.data(), views.data(), th, ratioHamming, logScaleFactor,
                                                                                projectionForm, (int)n, map.handle(), ids.data(),
                                                                                skip.empty() ? nullptr : skip.data(), occupied.empty() ? nullptr : occ.data(),
                                                                                rows.data(), nm.data(), projected ? projected->data() : nullptr, nullptr, nullptr)
                          : orbx_keyframe_search_by_projection_sim3_map(m_, (int)K, h.data(), cams.data(), poses.data(), th, ratioHamming, logScaleFactor,
                                                                        projectionForm, (int)n, map.handle(), ids.data(),
                                                                        skip.empty() ? nullptr : skip.data(), occupied.empty() ? nullptr : occ.data(),
                                                                        rows.data(), nm.data(), projected ? projected->data() : nullptr, nullptr, nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_search_by_projection_sim3_map: ") + orbx_status_string(r));
        for (size_t k = 0; k < K; k++) vpMatch[k].pop_back();
        vnMatches.assign(nm.begin(), nm.end());
    }
    // ComputeDistinctiveDescriptors with map point s's winning row written into the descriptor of slot setId[s]
    // (orbx_keyframe_distinctive_descriptors_to_map); a map point without observations keeps its descriptor.  bestObs as the overload above.
    void ComputeDistinctiveDescriptors(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<int32_t> &setPtr, const std::vector<int32_t> &obsKf,
                                       const std::vector<int32_t> &obsIdx, const DeviceMap &map, const std::vector<int32_t> &setId,
                                       std::vector<int32_t> &bestObs) {
        const size_t n = setPtr.empty() ? 0 : setPtr.size() - 1;
        if (obsKf.size() != obsIdx.size() || setId.size() != n || (n > 0 && (setPtr[n] < 0 || (size_t)setPtr[n] > obsKf.size())))
            throw std::invalid_argument("ComputeDistinctiveDescriptors: a key frame number and an index per observation, setPtr inside them, an id per set");
        std::vector<orbx_keyframe *> h(vpKFs.size());
        for (size_t k = 0; k < vpKFs.size(); k++) h[k] = vpKFs[k]->handle();
        bestObs.assign(n, -1);
        const int r = orbx_keyframe_distinctive_descriptors_to_map(m_, (int)h.size(), h.data(), (int)n, setPtr.data(), obsKf.data(), obsIdx.data(), map.handle(),
                                                                   setId.data(), bestObs.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_distinctive_descriptors_to_map: ") + orbx_status_string(r) + " " + orbx_last_error());
    }

    // ---- MapPoint::UpdateNormalAndDepth on resident key frames, over ComputeDistinctiveDescriptors' observation lists.  centers / centersRight:
    // 3 floats per key frame of vpKFs, GetCameraCenter() / GetRightCameraCenter() (centersRight may be empty without rig key frames); refObs[s] = the
    // position inside map point s's observations of the one in mpRefKF (the left one of a rig observation that has both).  The distances come back /
    // are stored UNSCALED, as the member leaves mfMinDistance / mfMaxDistance; a map point without observations keeps what it had.
    // flat (orbx_keyframe_update_normal_and_depth): pos = 3 floats per map point (mWorldPos) in, normal (3 per point), minDistance, maxDistance out
    void UpdateNormalAndDepth(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<float> &centers, const std::vector<float> &centersRight,
                              const std::vector<int32_t> &setPtr, const std::vector<int32_t> &obsKf, const std::vector<int32_t> &obsIdx,
                              const std::vector<int32_t> &refObs, const std::vector<float> &pos, std::vector<float> &normal,
                              std::vector<float> &minDistance, std::vector<float> &maxDistance) {
        const size_t n = NormalDepthSets("UpdateNormalAndDepth", vpKFs, centers, centersRight, setPtr, obsKf, obsIdx, refObs);
        if (pos.size() != 3 * n) throw std::invalid_argument("UpdateNormalAndDepth: three floats of pos per map point");
        normal.resize(3 * n); minDistance.resize(n); maxDistance.resize(n);
        std::vector<orbx_keyframe *> h = KeyFrameHandles(vpKFs);
        const int r = orbx_keyframe_update_normal_and_depth(m_, (int)h.size(), h.data(), centers.data(), centersRight.empty() ? nullptr : centersRight.data(),
                                                            (int)n, setPtr.data(), obsKf.data(), obsIdx.data(), refObs.data(), pos.data(), normal.data(),
                                                            minDistance.data(), maxDistance.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_update_normal_and_depth: ") + orbx_status_string(r) + " " + orbx_last_error());
    }
    // into the table (orbx_keyframe_update_normal_and_depth_to_map): pos is read from slot setId[s], the results are written into it.  normal /
    // minDistance / maxDistance: NULL, or vectors that receive what was written -- without them the host's members go stale.
    void UpdateNormalAndDepth(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<float> &centers, const std::vector<float> &centersRight,
                              const std::vector<int32_t> &setPtr, const std::vector<int32_t> &obsKf, const std::vector<int32_t> &obsIdx,
                              const std::vector<int32_t> &refObs, const DeviceMap &map, const std::vector<int32_t> &setId,
                              std::vector<float> *normal = nullptr, std::vector<float> *minDistance = nullptr, std::vector<float> *maxDistance = nullptr) {
        const size_t n = NormalDepthSets("UpdateNormalAndDepth", vpKFs, centers, centersRight, setPtr, obsKf, obsIdx, refObs);
        if (setId.size() != n) throw std::invalid_argument("UpdateNormalAndDepth: an id per map point");
        if (normal) normal->resize(3 * n);
        if (minDistance) minDistance->resize(n);
        if (maxDistance) maxDistance->resize(n);
        std::vector<orbx_keyframe *> h = KeyFrameHandles(vpKFs);
        const int r = orbx_keyframe_update_normal_and_depth_to_map(m_, (int)h.size(), h.data(), centers.data(),
                                                                   centersRight.empty() ? nullptr : centersRight.data(), (int)n, setPtr.data(), obsKf.data(),
                                                                   obsIdx.data(), refObs.data(), map.handle(), setId.data(), normal ? normal->data() : nullptr,
                                                                   minDistance ? minDistance->data() : nullptr, maxDistance ? maxDistance->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_update_normal_and_depth_to_map: ") + orbx_status_string(r) + " " + orbx_last_error());
    }
    // pMP->ComputeDistinctiveDescriptors(); pMP->UpdateNormalAndDepth(); for a batch of map points in ONE call
    // (orbx_keyframe_refresh_map_points_to_map): the descriptor, the normal and both distances of slot setId[s] are refreshed on the device; bestObs as
    // ComputeDistinctiveDescriptors returns it.  After it only SetWorldPos is left to DeviceMap::update.
    void RefreshMapPoints(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<float> &centers, const std::vector<float> &centersRight,
                          const std::vector<int32_t> &setPtr, const std::vector<int32_t> &obsKf, const std::vector<int32_t> &obsIdx,
                          const std::vector<int32_t> &refObs, const DeviceMap &map, const std::vector<int32_t> &setId, std::vector<int32_t> &bestObs) {
        const size_t n = NormalDepthSets("RefreshMapPoints", vpKFs, centers, centersRight, setPtr, obsKf, obsIdx, refObs);
        if (setId.size() != n) throw std::invalid_argument("RefreshMapPoints: an id per map point");
        bestObs.assign(n, -1);
        std::vector<orbx_keyframe *> h = KeyFrameHandles(vpKFs);
        const int r = orbx_keyframe_refresh_map_points_to_map(m_, (int)h.size(), h.data(), centers.data(), centersRight.empty() ? nullptr : centersRight.data(),
                                                              (int)n, setPtr.data(), obsKf.data(), obsIdx.data(), refObs.data(), map.handle(), setId.data(),
                                                              bestObs.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_refresh_map_points_to_map: ") + orbx_status_string(r) + " " + orbx_last_error());
    }

private:
    static std::vector<orbx_keyframe *> KeyFrameHandles(const std::vector<DeviceKeyFrame *> &vpKFs) {
        std::vector<orbx_keyframe *> h(vpKFs.size());
        for (size_t k = 0; k < vpKFs.size(); k++) h[k] = vpKFs[k]->handle();
        return h;
    }
    // the sizes the three calls above share; returns the number of map points
    static size_t NormalDepthSets(const char *who, const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<float> &centers,
                                  const std::vector<float> &centersRight, const std::vector<int32_t> &setPtr, const std::vector<int32_t> &obsKf,
                                  const std::vector<int32_t> &obsIdx, const std::vector<int32_t> &refObs) {
        const size_t n = setPtr.empty() ? 0 : setPtr.size() - 1;
        if (obsKf.size() != obsIdx.size() || refObs.size() != n || (n > 0 && (setPtr[n] < 0 || (size_t)setPtr[n] > obsKf.size())) ||
            centers.size() != 3 * vpKFs.size() || (!centersRight.empty() && centersRight.size() != 3 * vpKFs.size()))
            throw std::invalid_argument(std::string(who) + ": a key frame number and an index per observation, setPtr inside them, a reference position "
                                                           "per map point, three floats per key frame and centre");
        return n;
    }

public:

    // ---- The Tracking thread's searches whose queries are another frame's map points, from map ids (monocular / rectified frames): ids[i] = the
    // slot of the source's mvpMapPoints[i] or -1; the projection, the gates and the windows run on the device (k_track_project).  vpMatch[j] >= 0 is
    // the SOURCE feature index: CurrentFrame.mvpMapPoints[j] = Source.mvpMapPoints[vpMatch[j]]; -2 = cleared by the rotation check (set it NULL).
    // projected / projU / projV (optional, [ids.size()]): the entries that passed every gate and their projections.
    // SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1676-1887): cam / pose are the CURRENT frame's, ids[i] = -1 also for
    // mvbOutlier[i], hasObservations[i] = Observations() > 0 (empty: all), levelMode 0 / 1 (bForward) / 2 (bBackward).
    int TrackLastFrame(DeviceFrame &Cur, DeviceFrame &Last, const std::vector<uint8_t> &occupied, const orbx_camera &cam, const orbx_frame_pose &pose,
                       const DeviceMap &map, const std::vector<int32_t> &ids, const std::vector<uint8_t> &hasObservations, float th, int levelMode,
                       std::vector<int32_t> &vpMatch, std::vector<uint8_t> *projected = nullptr, std::vector<float> *projU = nullptr,
                       std::vector<float> *projV = nullptr) {
        if (!hasObservations.empty() && hasObservations.size() != ids.size()) throw std::invalid_argument("TrackLastFrame: one flag per id");
        if ((projU == nullptr) != (projV == nullptr)) throw std::invalid_argument("TrackLastFrame: projU and projV together");
        vpMatch.assign(Cur.count(), -1);
        if (projected) projected->assign(ids.size(), 0);
        if (projU) { projU->assign(ids.size(), 0.f); projV->assign(ids.size(), 0.f); }
        const int r = orbx_frame_track_last_frame_map(m_, Cur.handle(), Last.handle(), occupied.empty() ? nullptr : occupied.data(), &cam, &pose, map.handle(),
                                                      (int)ids.size(), ids.data(), hasObservations.empty() ? nullptr : hasObservations.data(), th, levelMode,
                                                      mbCheckOrientation ? 1 : 0, vpMatch.data(), projected ? projected->data() : nullptr,
                                                      projU ? projU->data() : nullptr, projV ? projV->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_track_last_frame_map: ") + orbx_status_string(r));
        return r;
    }
    // SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1889-2010): ids[i] = -1 for no point, isBad() or a point in
    // sAlreadyFound; occupied[j] = CurrentFrame.mvpMapPoints[j] != NULL.
    int SearchByProjection(DeviceFrame &Cur, DeviceKeyFrame &KF, const std::vector<uint8_t> &occupied, const orbx_camera &cam, const orbx_frame_pose &pose,
                           float logScaleFactor, const DeviceMap &map, const std::vector<int32_t> &ids, float th, int ORBdist,
                           std::vector<int32_t> &vpMatch, std::vector<uint8_t> *projected = nullptr, std::vector<float> *projU = nullptr,
                           std::vector<float> *projV = nullptr) {
        if ((projU == nullptr) != (projV == nullptr)) throw std::invalid_argument("SearchByProjection: projU and projV together");
        vpMatch.assign(Cur.count(), -1);
        if (projected) projected->assign(ids.size(), 0);
        if (projU) { projU->assign(ids.size(), 0.f); projV->assign(ids.size(), 0.f); }
        const int r = orbx_frame_search_by_projection_keyframe_map(m_, Cur.handle(), occupied.empty() ? nullptr : occupied.data(), &cam, &pose,
                                                                   logScaleFactor, KF.handle(), map.handle(), (int)ids.size(), ids.data(), th, (float)ORBdist,
                                                                   mbCheckOrientation ? 1 : 0, vpMatch.data(), projected ? projected->data() : nullptr,
                                                                   projU ? projU->data() : nullptr, projV ? projV->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_by_projection_keyframe_map: ") + orbx_status_string(r));
        return r;
    }
    // The same two for a fisheye-stereo rig: view = the CURRENT frame's left camera (Rcw, tcw, Ow, mpCamera's parameters), TrlR / Trlt =
    // GetRelativePoseTrl(); Last / KF are rig handles, ids has N_left + N_right entries, vpMatch N entries (Relocalization's form searches the left
    // camera only: the right camera's entries stay -1).
    int TrackLastFrameFisheye(DeviceFrame &Cur, DeviceFrame &Last, const std::vector<uint8_t> &occupied, const orbx_fisheye_view &view, const float TrlR[9],
                              const float Trlt[3], const DeviceMap &map, const std::vector<int32_t> &ids, const std::vector<uint8_t> &hasObservations,
                              float th, int levelMode, std::vector<int32_t> &vpMatch, std::vector<uint8_t> *projected = nullptr,
                              std::vector<float> *projU = nullptr, std::vector<float> *projV = nullptr) {
        if (!hasObservations.empty() && hasObservations.size() != ids.size()) throw std::invalid_argument("TrackLastFrameFisheye: one flag per id");
        if ((projU == nullptr) != (projV == nullptr)) throw std::invalid_argument("TrackLastFrameFisheye: projU and projV together");
        vpMatch.assign(Cur.count(), -1);
        if (projected) projected->assign(ids.size(), 0);
        if (projU) { projU->assign(ids.size(), 0.f); projV->assign(ids.size(), 0.f); }
        const int r = orbx_frame_track_last_frame_fisheye_map(m_, Cur.handle(), Last.handle(), occupied.empty() ? nullptr : occupied.data(), &view, TrlR, Trlt,
                                                              map.handle(), (int)ids.size(), ids.data(),
                                                              hasObservations.empty() ? nullptr : hasObservations.data(), th, levelMode,
                                                              mbCheckOrientation ? 1 : 0, vpMatch.data(), projected ? projected->data() : nullptr,
                                                              projU ? projU->data() : nullptr, projV ? projV->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_track_last_frame_fisheye_map: ") + orbx_status_string(r));
        return r;
    }
    int SearchByProjectionFisheye(DeviceFrame &Cur, DeviceKeyFrame &KF, const std::vector<uint8_t> &occupied, const orbx_fisheye_view &view,
                                  float logScaleFactor, const DeviceMap &map, const std::vector<int32_t> &ids, float th, int ORBdist,
                                  std::vector<int32_t> &vpMatch, std::vector<uint8_t> *projected = nullptr, std::vector<float> *projU = nullptr,
                                  std::vector<float> *projV = nullptr) {
        if ((projU == nullptr) != (projV == nullptr)) throw std::invalid_argument("SearchByProjectionFisheye: projU and projV together");
        vpMatch.assign(Cur.count(), -1);
        if (projected) projected->assign(ids.size(), 0);
        if (projU) { projU->assign(ids.size(), 0.f); projV->assign(ids.size(), 0.f); }
        const int r = orbx_frame_search_by_projection_keyframe_fisheye_map(m_, Cur.handle(), occupied.empty() ? nullptr : occupied.data(), &view,
                                                                           logScaleFactor, KF.handle(), map.handle(), (int)ids.size(), ids.data(), th,
                                                                           (float)ORBdist, mbCheckOrientation ? 1 : 0, vpMatch.data(),
                                                                           projected ? projected->data() : nullptr, projU ? projU->data() : nullptr,
                                                                           projV ? projV->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_frame_search_by_projection_keyframe_fisheye_map: ") + orbx_status_string(r));
        return r;
    }

    // MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:329-403) for a batch of map points: the observations' descriptors of map
    // point p are rows [setPtr[p], setPtr[p+1]) of `descriptors`; bestIdx[p] is the row offset (within the set) the reference keeps.
    void ComputeDistinctiveDescriptors(const std::vector<uint8_t> &descriptors, const std::vector<int32_t> &setPtr, std::vector<int32_t> &bestIdx) {
        const int n_sets = (int)setPtr.size() - 1;
        bestIdx.assign(n_sets > 0 ? n_sets : 0, -1);
        if (n_sets <= 0) return;
        const int r = orbx_distinctive_descriptors(m_, descriptors.data(), setPtr.data(), n_sets, bestIdx.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_distinctive_descriptors: ") + orbx_status_string(r));
    }
    // The same with the observations named where they are (orbx_keyframe_distinctive_descriptors): observation o of map point p, o in
    // [setPtr[p], setPtr[p+1]), is row obsIdx[o] of mDescriptors of vpKFs[obsKf[o]] (key frames of both kinds may be mixed; a rig's leftIndex, then
    // rightIndex, in its own numbering).  bestObs[p] is the position inside the set the reference keeps, -1 for an empty set; bestDesc, where given,
    // receives the winning rows, [n_sets][32] (zeros for an empty set): mDescriptor without touching a key frame.  No row is uploaded.
    void ComputeDistinctiveDescriptors(const std::vector<DeviceKeyFrame *> &vpKFs, const std::vector<int32_t> &setPtr, const std::vector<int32_t> &obsKf,
                                       const std::vector<int32_t> &obsIdx, std::vector<int32_t> &bestObs, std::vector<uint8_t> *bestDesc = nullptr) {
        const int n_sets = (int)setPtr.size() - 1;
        bestObs.assign(n_sets > 0 ? n_sets : 0, -1);
        if (bestDesc) bestDesc->assign(n_sets > 0 ? 32 * (size_t)n_sets : 0, 0);
        if (n_sets <= 0) return;
        if (obsKf.size() != obsIdx.size() || setPtr[n_sets] < 0 || (size_t)setPtr[n_sets] > obsKf.size())
            throw std::invalid_argument("ComputeDistinctiveDescriptors: a key frame number and an index per observation, setPtr inside them");
        std::vector<orbx_keyframe *> h(vpKFs.size());
        for (size_t k = 0; k < vpKFs.size(); k++) h[k] = vpKFs[k]->handle();
        const int r = orbx_keyframe_distinctive_descriptors(m_, (int)h.size(), h.data(), n_sets, setPtr.data(), obsKf.data(), obsIdx.data(), bestObs.data(),
                                                            bestDesc ? bestDesc->data() : nullptr);
        if (r < 0) throw std::runtime_error(std::string("orbx_keyframe_distinctive_descriptors: ") + orbx_status_string(r));
    }

    // Frame::ComputeStereoFishEyeMatches (Frame.cc:1126-1166) on host vectors: the brute-force kNN-2 of the two lapping-area descriptor
    // tails (BFmatcher.knnMatch, :1144) on the device, Lowe's ratio (:1151) and the bookkeeping (:1157-1162) here.  `triangulate(iLeft,
    // iRight, sigma1, sigma2, p3D) -> depth` is the caller's own KannalaBrandt8::TriangulateMatches (host geometry of the camera objects,
    // not part of the path) on mvKeys[iLeft] / mvKeysRight[iRight]; p3D is a float[3].  Returns nMatches; mvStereo3Dpoints[i] is written
    // for accepted matches only, as in the reference.  The body that replaces the reference's member is in INTEGRATION.md.
    template <class Triangulate>
    int ComputeStereoFishEyeMatches(const orbx_keypoint *mvKeys, const uint8_t *mDescriptors, int Nleft, int monoLeft,
                                    const orbx_keypoint *mvKeysRight, const uint8_t *mDescriptorsRight, int Nright, int monoRight,
                                    const float *mvLevelSigma2, Triangulate &&triangulate, std::vector<int> &mvLeftToRightMatch,
                                    std::vector<int> &mvRightToLeftMatch, std::vector<float> &mvDepth, std::vector<float> &mvuRight,
                                    std::vector<std::array<float, 3>> &mvStereo3Dpoints, int *descMatches = nullptr) {
        mvLeftToRightMatch.assign(Nleft > 0 ? Nleft : 0, -1);
        mvRightToLeftMatch.assign(Nright > 0 ? Nright : 0, -1);
        mvDepth.assign(Nleft > 0 ? Nleft : 0, -1.0f);
        mvuRight.assign(Nleft > 0 ? Nleft : 0, -1.0f);
        mvStereo3Dpoints.assign(Nleft > 0 ? Nleft : 0, std::array<float, 3>{0.f, 0.f, 0.f});
        const int nq = Nleft - monoLeft, nt = Nright - monoRight;
        int nMatches = 0, nDesc = 0;
        if (nq > 0) {
            std::vector<int32_t> idx(2 * (size_t)nq), dist(2 * (size_t)nq);
            const int r = orbx_knn2(m_, mDescriptors + (size_t)monoLeft * 32, nq, mDescriptorsRight + (size_t)monoRight * 32, nt > 0 ? nt : 0,
                                    idx.data(), dist.data());
            if (r < 0) throw std::runtime_error(std::string("orbx_knn2: ") + orbx_status_string(r));
            for (int q = 0; q < nq; q++) {
                if (idx[2 * q + 1] < 0) continue;                                     // fewer than two neighbours
                if (!((float)dist[2 * q] < (float)dist[2 * q + 1] * 0.7)) continue;     // :1151 (float against double)
                nDesc++;
                const int iL = q + monoLeft, iR = idx[2 * q] + monoRight;
                float p3D[3] = {0.f, 0.f, 0.f};
                const float depth = triangulate(iL, iR, mvLevelSigma2[mvKeys[iL].octave], mvLevelSigma2[mvKeysRight[iR].octave], p3D);
                if (depth > 0.0001f) {
                    mvLeftToRightMatch[iL] = iR;
                    mvRightToLeftMatch[iR] = iL;
                    mvStereo3Dpoints[iL] = {p3D[0], p3D[1], p3D[2]};
                    mvDepth[iL] = depth;
                    nMatches++;
                }
            }
        }
        if (descMatches) *descMatches = nDesc;
        return nMatches;
    }

    // The same member whole on the device, no callback: the rig's two KannalaBrandt8 cameras (mpCamera / mpCamera2 mvParameters, mRlr, mtlr) in `rig`,
    // KannalaBrandt8::TriangulateMatches (KannalaBrandt8.cpp:305-368) evaluated by the kernel (orbx_compute_stereo_fisheye_matches).  Same outputs;
    // mvuRight stays -1.  The callback form above remains the route for other camera models.
    int ComputeStereoFishEyeMatches(const orbx_keypoint *mvKeys, const uint8_t *mDescriptors, int Nleft, int monoLeft,
                                    const orbx_keypoint *mvKeysRight, const uint8_t *mDescriptorsRight, int Nright, int monoRight,
                                    const float *mvLevelSigma2, int nlevels, const orbx_kb8_rig &rig, std::vector<int> &mvLeftToRightMatch,
                                    std::vector<int> &mvRightToLeftMatch, std::vector<float> &mvDepth, std::vector<float> &mvuRight,
                                    std::vector<std::array<float, 3>> &mvStereo3Dpoints, int *descMatches = nullptr) {
        const int nl = Nleft > 0 ? Nleft : 0, nr = Nright > 0 ? Nright : 0;
        mvLeftToRightMatch.assign(nl, -1);
        mvRightToLeftMatch.assign(nr, -1);
        mvDepth.assign(nl, -1.0f);
        mvuRight.assign(nl, -1.0f);
        mvStereo3Dpoints.assign(nl, std::array<float, 3>{0.f, 0.f, 0.f});
        static_assert(sizeof(std::array<float, 3>) == 3 * sizeof(float), "mvStereo3Dpoints rows are three packed floats");
        std::vector<int32_t> l2r(nl), r2l(nr);
        int nDesc = 0;
        const int r = orbx_compute_stereo_fisheye_matches(m_, &rig, mvKeys, mDescriptors, Nleft, monoLeft, mvKeysRight, mDescriptorsRight, Nright, monoRight,
                                                          mvLevelSigma2, nlevels, l2r.data(), r2l.data(), mvDepth.data(),
                                                          reinterpret_cast<float *>(mvStereo3Dpoints.data()), &nDesc);
        if (r < 0) throw std::runtime_error(std::string("orbx_compute_stereo_fisheye_matches: ") + orbx_status_string(r));
        for (int i = 0; i < nl; i++) mvLeftToRightMatch[i] = l2r[i];
        for (int i = 0; i < nr; i++) mvRightToLeftMatch[i] = r2l[i];
        if (descMatches) *descMatches = nDesc;
        return r;
    }

    // Frame::ComputeStereoMatches (Frame.cc:811-981) on host vectors: mvuRight / mvDepth out.  pyrLeft/pyrRight[l] are the level ROI
    // origins of the two extractors' mvImagePyramid (host copies, e.g. ORBextractor::GetPyramidLevel).  For the device-resident
    // batched form (no pyramid transfer) use orbx_stereo_batch_device / orbx_stereo_batch_download on the two extractors.
    int ComputeStereoMatches(const orbx_keypoint *mvKeys, const uint8_t *mDescriptors, int N, const orbx_keypoint *mvKeysRight,
                             const uint8_t *mDescriptorsRight, int Nr, const float *mvScaleFactors, const float *mvInvScaleFactors, int nlevels,
                             const uint8_t *const *pyrLeft, const uint8_t *const *pyrRight, const int32_t *pyrW, const int32_t *pyrH,
                             const size_t *pyrStride, float mbf, float mb, std::vector<float> &mvuRight, std::vector<float> &mvDepth) {
        mvuRight.assign(N, -1.0f); mvDepth.assign(N, -1.0f);
        const int r = orbx_compute_stereo_matches(m_, mvKeys, mDescriptors, N, mvKeysRight, mDescriptorsRight, Nr, mvScaleFactors, mvInvScaleFactors,
                                                  nlevels, pyrLeft, pyrRight, pyrW, pyrH, pyrStride, mbf, mb, mvuRight.data(), mvDepth.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_compute_stereo_matches: ") + orbx_status_string(r));
        return r;
    }

    // Frame::UnprojectStereo for every feature of a resident frame that holds mvDepth (DeviceFrame::loadStereoBatch / loadHostStereo;
    // orbx_frame_unproject_stereo): mvuRight / mvDepth get N entries; x3D gets N rows of 3, the point where mvDepth > 0 and zeros elsewhere.
    // Returns the number of features with depth.
    int UnprojectStereo(DeviceFrame &F, const orbx_new_points_view &view, std::vector<float> &mvuRight, std::vector<float> &mvDepth, std::vector<float> &x3D) {
        // (the count may still be on the device: sized by the handle's capacity, trimmed once the call has brought N home)
        const size_t cap = (size_t)F.capacity();
        mvuRight.assign(cap, 0.f); mvDepth.assign(cap, 0.f); x3D.assign(3 * cap, 0.f);
        int with = 0;
        const int st = orbx_frame_unproject_stereo(m_, F.handle(), &view, mvuRight.data(), mvDepth.data(), x3D.data(), &with);
        if (st < 0) throw std::runtime_error(std::string("orbx_frame_unproject_stereo: ") + orbx_status_string(st) + " " + orbx_last_error());
        const size_t n = (size_t)F.count();   // known after the call
        mvuRight.resize(n); mvDepth.resize(n); x3D.resize(3 * n);
        return with;
    }

#ifdef ORBX_WITH_SLAM_TYPES
    // the reference's own signatures (Frame / KeyFrame / MapPoint graphs): see ORBmatcher_slam.inl
#include "ORBmatcher_slam.inl"
#endif

    orbx_matcher *handle() { return m_; }

private:
    // what the key-frame ...Map overloads share: the handles, the skip row count and the output rows (sides per key frame)
    static std::vector<orbx_keyframe *> mapCallHandles(const std::vector<DeviceKeyFrame *> &vpKFs, size_t K, size_t n, const std::vector<uint8_t> &skip,
                                                       std::vector<int32_t> &bestIdx, std::vector<int32_t> &bestDist, std::vector<uint8_t> *projected,
                                                       size_t sides = 1) {
        if (!skip.empty() && skip.size() != K * n) throw std::invalid_argument("a ...Map call takes K x n skip flags");
        std::vector<orbx_keyframe *> h(K);
        for (size_t k = 0; k < K; k++) h[k] = vpKFs[k]->handle();
        bestIdx.assign(K * sides * n, -1); bestDist.assign(K * sides * n, 256);
        if (projected) projected->assign(K * sides * n, 0);
        return h;
    }

protected:
    float mfNNratio;
    bool mbCheckOrientation;
    orbx_matcher *m_ = nullptr;
};

// ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) flattened for the device: the k-ary tree as CSR children, one
// 32-byte descriptor and one word id (-1 for inner nodes) per node.  transform() is the tree descent of
// TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1151-1193)
// as called from Frame::ComputeBoW (Frame.cc:462-470) / KeyFrame::ComputeBoW: per feature the word id and the node id `levelsup`
// levels above the leaf; the caller folds them into BowVector (addWeight) and FeatureVector (addFeature) in feature order.
inline DeviceFrame::DeviceFrame(ORBmatcher &matcher, int cap) : cap_(cap) {
    check(orbx_frame_create(matcher.handle(), cap, &f_), "orbx_frame_create");
}

inline void DeviceMap::update(ORBmatcher &matcher, const std::vector<int32_t> &ids, const float *pos, const float *normal, const float *minDistance,
                              const float *maxDistance, const uint8_t *descriptors) {
    const int st = orbx_map_update(matcher.handle(), map_, (int)ids.size(), ids.data(), pos, normal, minDistance, maxDistance, descriptors);
    if (st < 0) throw std::runtime_error(std::string("orbx_map_update: ") + orbx_status_string(st) + " " + orbx_last_error());
}
inline void DeviceMap::read(ORBmatcher &matcher, const std::vector<int32_t> &ids, float *pos, float *normal, float *minDistance, float *maxDistance,
                            uint8_t *descriptors) {
    const int st = orbx_map_read(matcher.handle(), map_, (int)ids.size(), ids.data(), pos, normal, minDistance, maxDistance, descriptors);
    if (st < 0) throw std::runtime_error(std::string("orbx_map_read: ") + orbx_status_string(st) + " " + orbx_last_error());
}

inline DeviceKeyFrame::DeviceKeyFrame(ORBmatcher &matcher, DeviceFrame &frame, const float *mvInvLevelSigma2) {
    const int st = orbx_keyframe_from_frame(matcher.handle(), frame.handle(), mvInvLevelSigma2, &kf_);
    if (st < 0) throw std::runtime_error(std::string("orbx_keyframe_from_frame: ") + orbx_status_string(st) + " " + orbx_last_error());
}
inline DeviceKeyFrame::DeviceKeyFrame(ORBmatcher &matcher, const FrameView &KF, const float *mvInvLevelSigma2) {
    orbx_frame_desc fd = KF.c();
    const int st = orbx_keyframe_create_host(matcher.handle(), &fd, mvInvLevelSigma2, &kf_);
    if (st < 0) throw std::runtime_error(std::string("orbx_keyframe_create_host: ") + orbx_status_string(st) + " " + orbx_last_error());
}

inline DeviceKeyFrame::DeviceKeyFrame(ORBmatcher &matcher, const FrameView &KF, const std::vector<float> &mvDepth, const std::vector<float> &keysXY,
                                      const float *mvInvLevelSigma2) {
    orbx_frame_desc fd = KF.c();
    if ((int)mvDepth.size() != fd.n || (!keysXY.empty() && (int)keysXY.size() != 2 * fd.n)) throw std::invalid_argument("DeviceKeyFrame: array sizes");
    const int st = orbx_keyframe_create_host_stereo(matcher.handle(), &fd, mvDepth.data(), keysXY.empty() ? nullptr : keysXY.data(), mvInvLevelSigma2, &kf_);
    if (st < 0) throw std::runtime_error(std::string("orbx_keyframe_create_host_stereo: ") + orbx_status_string(st) + " " + orbx_last_error());
}

inline DeviceKeyFrame::DeviceKeyFrame(Fisheye, ORBmatcher &matcher, DeviceFrame &frame, const float *mvInvLevelSigma2) : fisheye_(true) {
    const int st = orbx_keyframe_from_frame_fisheye(matcher.handle(), frame.handle(), mvInvLevelSigma2, &kf_);
    if (st < 0) throw std::runtime_error(std::string("orbx_keyframe_from_frame_fisheye: ") + orbx_status_string(st) + " " + orbx_last_error());
}
inline DeviceKeyFrame::DeviceKeyFrame(ORBmatcher &matcher, const FrameView &left, const std::vector<orbx_keypoint> &keysRight,
                                      const float *mvInvLevelSigma2) : fisheye_(true) {
    orbx_frame_desc fd = left.c();
    const int st = orbx_keyframe_create_host_fisheye(matcher.handle(), &fd, keysRight.data(), (int)keysRight.size(), mvInvLevelSigma2, &kf_);
    if (st < 0) throw std::runtime_error(std::string("orbx_keyframe_create_host_fisheye: ") + orbx_status_string(st) + " " + orbx_last_error());
}

class ORBVocabularyDevice {
public:
    ORBVocabularyDevice(int L, const std::vector<int32_t> &childPtr, const std::vector<int32_t> &childIdx, const std::vector<uint8_t> &nodeDesc,
                        const std::vector<int32_t> &wordId, int device = 0) {
        const int st = orbx_vocabulary_create(device, L, (int)wordId.size(), childPtr.data(), childIdx.data(), nodeDesc.data(), wordId.data(), &v_);
        if (st != ORBX_OK) throw std::runtime_error(std::string("orbx_vocabulary_create: ") + orbx_status_string(st));
    }
    ~ORBVocabularyDevice() { orbx_vocabulary_destroy(v_); }
    ORBVocabularyDevice(const ORBVocabularyDevice &) = delete;
    ORBVocabularyDevice &operator=(const ORBVocabularyDevice &) = delete;
    void transform(ORBmatcher &m, const uint8_t *descriptors, int n, int levelsup, std::vector<int32_t> &wordId, std::vector<int32_t> &nodeId) const {
        wordId.assign(n, -1); nodeId.assign(n, -1);
        if (n == 0) return;
        const int r = orbx_bow_transform(m.handle(), v_, descriptors, n, levelsup, wordId.data(), nodeId.data());
        if (r < 0) throw std::runtime_error(std::string("orbx_bow_transform: ") + orbx_status_string(r));
    }
    // m_words[id]->weight for every word id: words with weight <= 0 are stop words of DeviceFrame::ComputeBoW's FeatureVector
    void setWordWeights(const std::vector<double> &weights) {
        const int r = orbx_vocabulary_set_word_weights(v_, weights.data(), (int)weights.size());
        if (r < 0) throw std::runtime_error(std::string("orbx_vocabulary_set_word_weights: ") + orbx_status_string(r));
    }
    const orbx_vocabulary *handle() const { return v_; }

private:
    orbx_vocabulary *v_ = nullptr;
};

inline void DeviceFrame::ComputeBoW(ORBmatcher &matcher, const ORBVocabularyDevice &voc, int levelsup, std::vector<int32_t> *wordId,
                                    std::vector<int32_t> *nodeId) {
    if (!wordId && !nodeId) {
        check(orbx_frame_compute_bow(matcher.handle(), f_, voc.handle(), levelsup, nullptr, nullptr), "orbx_frame_compute_bow");
        return;
    }
    std::vector<int32_t> w(cap_), nd(cap_);
    check(orbx_frame_compute_bow(matcher.handle(), f_, voc.handle(), levelsup, w.data(), nd.data()), "orbx_frame_compute_bow");
    const int n = count();   // known after the call
    if (wordId) wordId->assign(w.begin(), w.begin() + n);
    if (nodeId) nodeId->assign(nd.begin(), nd.begin() + n);
}

inline void DeviceFrame::ComputeBoWFisheye(ORBmatcher &matcher, const ORBVocabularyDevice &voc, int levelsup, std::vector<int32_t> *wordId,
                                           std::vector<int32_t> *nodeId) {
    if (!wordId && !nodeId) {
        check(orbx_frame_compute_bow_fisheye(matcher.handle(), f_, voc.handle(), levelsup, nullptr, nullptr), "orbx_frame_compute_bow_fisheye");
        return;
    }
    std::vector<int32_t> w(cap_), nd(cap_);
    check(orbx_frame_compute_bow_fisheye(matcher.handle(), f_, voc.handle(), levelsup, w.data(), nd.data()), "orbx_frame_compute_bow_fisheye");
    const int n = count();   // known after the call
    if (wordId) wordId->assign(w.begin(), w.begin() + n);
    if (nodeId) nodeId->assign(nd.begin(), nd.begin() + n);
}

inline void DeviceKeyFrame::ComputeBoW(ORBmatcher &matcher, const ORBVocabularyDevice &voc, int levelsup, std::vector<int32_t> *wordId,
                                       std::vector<int32_t> *nodeId) {
    auto check = [](int st) { if (st < 0) throw std::runtime_error(std::string("orbx_keyframe_compute_bow: ") + orbx_status_string(st) + " " + orbx_last_error()); };
    const auto compute = fisheye_ ? orbx_keyframe_compute_bow_fisheye : orbx_keyframe_compute_bow;   // (a rig: all N = NLeft + NRight rows, left then right)
    if (!wordId && !nodeId) {
        check(compute(matcher.handle(), kf_, voc.handle(), levelsup, nullptr, nullptr));
        return;
    }
    const int n = count();   // (the id buffers hold N entries)
    std::vector<int32_t> w((size_t)std::max(n, 1)), nd((size_t)std::max(n, 1));
    check(compute(matcher.handle(), kf_, voc.handle(), levelsup, w.data(), nd.data()));
    if (wordId) wordId->assign(w.begin(), w.begin() + n);
    if (nodeId) nodeId->assign(nd.begin(), nd.begin() + n);
}

inline void DeviceFrame::BowVector(ORBmatcher &matcher, std::vector<int32_t> &wordId, std::vector<double> &value) {
    wordId.assign((size_t)std::max(cap_, 1), 0); value.assign((size_t)std::max(cap_, 1), 0.0);
    int n = 0;
    check(orbx_frame_bow_vector(matcher.handle(), f_, wordId.data(), value.data(), &n), "orbx_frame_bow_vector");
    wordId.resize((size_t)n); value.resize((size_t)n);
}

inline void DeviceKeyFrame::BowVector(ORBmatcher &matcher, std::vector<int32_t> &wordId, std::vector<double> &value) {
    const size_t cap = (size_t)std::max(count(), 1);   // (the buffers hold N entries)
    wordId.assign(cap, 0); value.assign(cap, 0.0);
    int n = 0;
    const int st = orbx_keyframe_bow_vector(matcher.handle(), kf_, wordId.data(), value.data(), &n);
    if (st < 0) throw std::runtime_error(std::string("orbx_keyframe_bow_vector: ") + orbx_status_string(st) + " " + orbx_last_error());
    wordId.resize((size_t)n); value.resize((size_t)n);
}

inline void DeviceKeyFrameDatabase::add(ORBmatcher &matcher, int slot, DeviceKeyFrame &kf) {
    check(orbx_keyframe_database_add(matcher.handle(), db_, slot, kf.handle()), "orbx_keyframe_database_add");
}
inline void DeviceKeyFrameDatabase::erase(ORBmatcher &matcher, int slot) {
    check(orbx_keyframe_database_erase(matcher.handle(), db_, slot), "orbx_keyframe_database_erase");
}
inline void DeviceKeyFrameDatabase::clear(ORBmatcher &matcher) { check(orbx_keyframe_database_clear(matcher.handle(), db_), "orbx_keyframe_database_clear"); }
template <class Fn, class H>
DeviceKeyFrameDatabase::Candidates DeviceKeyFrameDatabase::query(Fn fn, const char *what, ORBmatcher &matcher, H *src, const std::vector<int32_t> &exclude,
                                                                 float minRatio, int candCap, bool full) {
    Candidates c;
    const int cap = candCap < 0 ? nSlots_ : candCap;
    c.slot.assign((size_t)std::max(cap, 1), 0); c.commonWords.assign((size_t)std::max(cap, 1), 0); c.score.assign((size_t)std::max(cap, 1), 0.0);
    if (full) { c.nCommon.assign((size_t)nSlots_, -1); c.allScores.assign((size_t)nSlots_, 0.0); }
    check(fn(matcher.handle(), db_, src, exclude.empty() ? nullptr : exclude.data(), (int)exclude.size(), minRatio, full ? c.nCommon.data() : nullptr,
             full ? c.allScores.data() : nullptr, c.slot.data(), c.commonWords.data(), c.score.data(), cap, &c.nCandidates, &c.maxCommonWords), what);
    const size_t k = (size_t)std::min(c.nCandidates, cap);
    c.slot.resize(k); c.commonWords.resize(k); c.score.resize(k);
    return c;
}
inline DeviceKeyFrameDatabase::Candidates DeviceKeyFrameDatabase::queryFrame(ORBmatcher &matcher, DeviceFrame &frame, const std::vector<int32_t> &exclude,
                                                                             float minRatio, int candCap, bool full) {
    return query(orbx_keyframe_database_query_frame, "orbx_keyframe_database_query_frame", matcher, frame.handle(), exclude, minRatio, candCap, full);
}
inline DeviceKeyFrameDatabase::Candidates DeviceKeyFrameDatabase::queryKeyFrame(ORBmatcher &matcher, DeviceKeyFrame &kf, const std::vector<int32_t> &exclude,
                                                                                float minRatio, int candCap, bool full) {
    return query(orbx_keyframe_database_query_keyframe, "orbx_keyframe_database_query_keyframe", matcher, kf.handle(), exclude, minRatio, candCap, full);
}

inline void DeviceKeyFrame::BowFromFrame(ORBmatcher &matcher, DeviceFrame &frame) {
    const int st = (fisheye_ ? orbx_keyframe_bow_from_frame_fisheye : orbx_keyframe_bow_from_frame)(matcher.handle(), kf_, frame.handle());
    if (st < 0) throw std::runtime_error(std::string("orbx_keyframe_bow_from_frame: ") + orbx_status_string(st) + " " + orbx_last_error());
}

}  // namespace ORB_SLAM3

#endif
