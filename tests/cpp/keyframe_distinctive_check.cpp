// MapPoint::ComputeDistinctiveDescriptors on resident key frames -- orbx_keyframe_distinctive_descriptors -- with K = 3 key frames (two monocular of
// unequal N, one fisheye-stereo) and sets of 0, 1, 2, 17, 64, 65 and 130 observations: on a FRESH matcher context, then twice on ONE context that
// served a call three times as large first (the arena and the pinned mirror are then larger than the call and hold the larger call's bytes).  All three
// runs must give the same results, and these must equal the reference loop (MapPoint.cc:329-403) written out below; the caller's output arrays are
// heap blocks of exactly the needed size, filled with a sentinel; a refused call and an empty one leave the transfer counters alone.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt) and
// compiled with -fsanitize=address,undefined, as tests/cpp/keyframe_paths_check.cpp.  Prints "keyframe distinctive ok" and returns 0.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kLevels = 8, kK = 3, kSentinel = -7;
const int kRows[kK] = {150, 257, 120 + 90};   // key frame 2 is the rig: 120 left rows, 90 right rows
constexpr int kRigLeft = 120, kRigRight = 90;
const int kSizes[] = {0, 1, 2, 17, 64, 65, 130};
constexpr int kSets = (int)(sizeof(kSizes) / sizeof(kSizes[0]));

#define MUST(expr)                                                                   \
    do {                                                                             \
        const int r_ = (expr);                                                       \
        if (r_ < 0) { printf("%s: %d\n", #expr, r_); return 1; }                     \
    } while (0)
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

struct Scene {
    float scale[kLevels];
    std::vector<orbx_keypoint> kps[kK];
    std::vector<uint8_t> desc[kK];
    std::vector<int32_t> set_ptr, obs_kf, obs_idx;
};

// Every key frame's rows are noisy copies of a handful of base rows, so the medians inside a set differ.  `repeat` copies of the sets.
void make_scene(int repeat, Scene &S) {
    std::mt19937 rng(23);
    for (int l = 0; l < kLevels; l++) S.scale[l] = l ? S.scale[l - 1] * 1.2f : 1.f;
    uint8_t base[4][32];
    for (auto &b : base) for (uint8_t &x : b) x = (uint8_t)rng();
    for (int k = 0; k < kK; k++)
        for (int i = 0; i < kRows[k]; i++) {
            orbx_keypoint kp;
            memset(&kp, 0, sizeof(kp));
            kp.x = 1.f + (float)(rng() % 600); kp.y = 1.f + (float)(rng() % 400); kp.octave = (int)(rng() % kLevels);
            kp.size = 31.f; kp.class_id = -1;
            S.kps[k].push_back(kp);
            const uint8_t *b = base[rng() % 4];
            for (int j = 0; j < 32; j++) S.desc[k].push_back(b[j]);
            for (int f = 0; f < 20; f++) { const unsigned bit = rng() % 256; S.desc[k][S.desc[k].size() - 32 + bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
        }
    S.set_ptr.push_back(0);
    for (int r = 0; r < repeat; r++)
        for (int s = 0; s < kSets; s++) {
            for (int o = 0; o < kSizes[s]; o++) {
                const int k = (int)(rng() % kK);
                // the rig's last left row, first right row and last row are named early in every set
                const int i = k == 2 && o < 6 ? (o % 3 == 0 ? kRigLeft - 1 : o % 3 == 1 ? kRigLeft : kRows[2] - 1) : (int)(rng() % (unsigned)kRows[k]);
                S.obs_kf.push_back(k); S.obs_idx.push_back(i);
            }
            S.set_ptr.push_back((int32_t)S.obs_kf.size());
        }
}

int make_key_frames(orbx_matcher *m, const Scene &S, orbx_keyframe **kfs) {
    for (int k = 0; k < kK; k++) {
        orbx_frame_desc d;
        memset(&d, 0, sizeof(d));
        d.keypoints_un = S.kps[k].data(); d.descriptors = S.desc[k].data(); d.n = k == 2 ? kRigLeft : kRows[k];
        d.min_x = 0.f; d.max_x = 640.f; d.min_y = 0.f; d.max_y = 480.f;
        d.scale_factors = S.scale; d.nlevels = kLevels;
        if (k == 2) MUST(orbx_keyframe_create_host_fisheye(m, &d, S.kps[k].data() + kRigLeft, kRigRight, nullptr, &kfs[k]));
        else MUST(orbx_keyframe_create_host(m, &d, nullptr, &kfs[k]));
    }
    return 0;
}

// MapPoint.cc:358-403 on mDescriptors.row(idx) of every observation
void reference(const Scene &S, std::vector<int32_t> &best, std::vector<uint8_t> &desc) {
    const int n_sets = (int)S.set_ptr.size() - 1;
    best.assign(n_sets, -1); desc.assign(32 * (size_t)n_sets, 0);
    for (int s = 0; s < n_sets; s++) {
        const int b = S.set_ptr[s], N = S.set_ptr[s + 1] - b;
        if (N == 0) continue;
        auto row = [&](int o) { return S.desc[S.obs_kf[b + o]].data() + 32 * (size_t)S.obs_idx[b + o]; };
        int bestMedian = 0x7fffffff, bestIdx = 0;
        for (int i = 0; i < N; i++) {
            std::vector<int> d(N);
            for (int j = 0; j < N; j++) {
                int h = 0;
                for (int q = 0; q < 32; q++) h += __builtin_popcount((unsigned)(row(i)[q] ^ row(j)[q]));
                d[j] = h;
            }
            std::sort(d.begin(), d.end());
            const int median = d[(size_t)(0.5 * (N - 1))];
            if (median < bestMedian) { bestMedian = median; bestIdx = i; }
        }
        best[s] = bestIdx;
        memcpy(desc.data() + 32 * (size_t)s, row(bestIdx), 32);
    }
}

struct Out {
    std::vector<int32_t> best;
    std::vector<uint8_t> desc;
};

// the caller's arrays: heap blocks of exactly the needed size, filled with a sentinel
int call(orbx_matcher *m, orbx_keyframe *const *kfs, const Scene &S, bool want_desc, Out &out) {
    const int n_sets = (int)S.set_ptr.size() - 1;
    std::unique_ptr<int32_t[]> best(new int32_t[n_sets]);
    std::unique_ptr<uint8_t[]> desc(new uint8_t[32 * (size_t)n_sets]);
    std::fill(best.get(), best.get() + n_sets, kSentinel);
    memset(desc.get(), 0xa5, 32 * (size_t)n_sets);
    MUST(orbx_keyframe_distinctive_descriptors(m, kK, kfs, n_sets, S.set_ptr.data(), S.obs_kf.data(), S.obs_idx.data(), best.get(),
                                               want_desc ? desc.get() : nullptr));
    out.best.assign(best.get(), best.get() + n_sets);
    out.desc.assign(desc.get(), desc.get() + 32 * (size_t)n_sets);
    return 0;
}

bool same_counters(orbx_matcher *m, const int64_t *before) {
    int64_t now[6];
    return orbx_matcher_debug_transfers(m, now, 6) >= 0 && memcmp(now, before, sizeof(now)) == 0;
}

}  // namespace

int main() {
    Scene S, S3;
    make_scene(1, S);
    make_scene(3, S3);
    std::vector<int32_t> want;
    std::vector<uint8_t> want_desc;
    reference(S, want, want_desc);
    CHECK(want[0] == -1);
    int moved = 0;
    for (int s = 1; s < kSets; s++) moved += want[s] != 0;
    CHECK(moved >= 3);   // the winner is not always the first row

    orbx_matcher *fresh = nullptr, *used = nullptr;
    MUST(orbx_matcher_create(0, &fresh));
    MUST(orbx_matcher_create(0, &used));
    orbx_keyframe *kfs[kK] = {nullptr, nullptr, nullptr};
    if (make_key_frames(fresh, S, kfs)) return 1;

    Out a, b, c, big, nodesc;
    if (call(fresh, kfs, S, true, a)) return 1;
    if (call(used, kfs, S3, true, big)) return 1;   // three times as large, on the other context
    if (call(used, kfs, S, true, b) || call(used, kfs, S, true, c) || call(used, kfs, S, false, nodesc)) return 1;
    CHECK(a.best == want && a.desc == want_desc);
    CHECK(b.best == a.best && b.desc == a.desc && c.best == a.best && c.desc == a.desc);
    CHECK(nodesc.best == a.best);
    for (uint8_t x : nodesc.desc) CHECK(x == 0xa5);   // best_desc = NULL: nothing is written
    CHECK(std::equal(want.begin(), want.end(), big.best.begin()));   // (the first copy of the larger call's sets names the same observations)

    // a refused call and an empty one leave the transfer counters alone
    int64_t before[6];
    MUST(orbx_matcher_debug_transfers(used, before, 6));
    CHECK(before[0] == 1 && before[1] == 1);
    const int n_sets = (int)S.set_ptr.size() - 1;
    std::vector<int32_t> best(n_sets, kSentinel), bad_idx = S.obs_idx, bad_kf = S.obs_kf;
    bad_idx.back() = 100000; bad_kf[1] = kK;
    for (size_t o = 0; o < S.obs_kf.size(); o++)
        if (S.obs_kf[o] == 2) { bad_idx[o] = kRows[2]; break; }   // the rig's N: one past its last right row
    CHECK(orbx_keyframe_distinctive_descriptors(used, kK, kfs, n_sets, S.set_ptr.data(), S.obs_kf.data(), bad_idx.data(), best.data(), nullptr) == ORBX_E_BAD_ARG);
    CHECK(orbx_keyframe_distinctive_descriptors(used, kK, kfs, n_sets, S.set_ptr.data(), bad_kf.data(), S.obs_idx.data(), best.data(), nullptr) == ORBX_E_BAD_ARG);
    CHECK(orbx_keyframe_distinctive_descriptors(used, kK, kfs, n_sets, S.set_ptr.data(), nullptr, S.obs_idx.data(), best.data(), nullptr) == ORBX_E_BAD_ARG);
    CHECK(orbx_keyframe_distinctive_descriptors(used, ORBX_MAX_DISTINCTIVE_KEYFRAMES + 1, kfs, n_sets, S.set_ptr.data(), S.obs_kf.data(), S.obs_idx.data(),
                                                best.data(), nullptr) == ORBX_E_TOO_LARGE);
    CHECK(orbx_keyframe_distinctive_descriptors(used, kK, kfs, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == ORBX_OK);
    const int32_t empty_ptr[3] = {0, 0, 0};
    int32_t two[2] = {kSentinel, kSentinel};
    CHECK(orbx_keyframe_distinctive_descriptors(used, kK, kfs, 2, empty_ptr, nullptr, nullptr, two, nullptr) == ORBX_OK && two[0] == -1 && two[1] == -1);
    for (int32_t x : best) CHECK(x == kSentinel);
    CHECK(same_counters(used, before));

    for (orbx_keyframe *kf : kfs) orbx_keyframe_destroy(kf);
    orbx_matcher_destroy(fresh);
    orbx_matcher_destroy(used);
    printf("keyframe distinctive ok\n");
    return 0;
}
