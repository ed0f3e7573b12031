// MapPoint::UpdateNormalAndDepth on resident key frames -- orbx_keyframe_update_normal_and_depth (flat) and orbx_keyframe_refresh_map_points_to_map --
// with K = 3 key frames (two monocular of unequal N and different pyramids, one fisheye-stereo) and sets of 0, 1, 2, 17, 64, 65 and 130 observations.
// The flat results must equal the reference loop of MapPoint.cc written out below, bit for bit; the refresh call must leave those values, the winning
// rows of the distinctive reference loop, and untouched pos in the slots of a table whose LAST slot is one of them.  The caller's arrays are heap
// blocks of exactly the needed size, filled with a sentinel; a refused call and an empty one leave the transfer counters alone.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt) and
// compiled with -fsanitize=address,undefined, as tests/cpp/map_check.cpp.  Prints "normal depth ok" and returns 0.  With an argument N it also times
// N runs of the reference loop on the host and prints the mean ("host reference loop": the C++ host cost of the member on this scene, nothing else).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kK = 3, kCapacity = 64;
const int kRows[kK] = {150, 257, 120 + 90};   // key frame 2 is the rig: 120 left rows, 90 right rows
const int kLevels[kK] = {8, 5, 8};
const float kFactor[kK] = {1.2f, 1.1f, 1.2f};
constexpr int kRigLeft = 120, kRigRight = 90;
const int kSizes[] = {0, 1, 2, 17, 64, 65, 130};
constexpr int kSets = (int)(sizeof(kSizes) / sizeof(kSizes[0]));
constexpr float kSentinel = -12345.f;

#define MUST(expr)                                                                   \
    do {                                                                             \
        const int r_ = (expr);                                                       \
        if (r_ < 0) { printf("%s: %d %s\n", #expr, r_, orbx_last_error()); return 1; } \
    } while (0)
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

struct Scene {
    float scale[kK][8];
    std::vector<orbx_keypoint> kps[kK];
    std::vector<uint8_t> desc[kK];
    float centers[kK][3], centers_right[kK][3];
    std::vector<int32_t> set_ptr, obs_kf, obs_idx, ref_obs;
    std::vector<float> pos;
};

void make_scene(Scene &S) {
    std::mt19937 rng(29);
    auto uni = [&](float a, float b) { return a + (b - a) * (float)(rng() % 100000) / 100000.f; };
    uint8_t base[4][32];
    for (auto &b : base) for (uint8_t &x : b) x = (uint8_t)rng();
    for (int k = 0; k < kK; k++) {
        for (int l = 0; l < kLevels[k]; l++) S.scale[k][l] = l ? S.scale[k][l - 1] * kFactor[k] : 1.f;
        for (int i = 0; i < kRows[k]; i++) {
            orbx_keypoint kp;
            memset(&kp, 0, sizeof(kp));
            kp.x = 1.f + (float)(rng() % 600); kp.y = 1.f + (float)(rng() % 400); kp.octave = (int)(rng() % (unsigned)kLevels[k]);
            kp.size = 31.f; kp.class_id = -1;
            S.kps[k].push_back(kp);
            const uint8_t *b = base[rng() % 4];
            for (int j = 0; j < 32; j++) S.desc[k].push_back(b[j]);
            for (int f = 0; f < 20; f++) { const unsigned bit = rng() % 256; S.desc[k][S.desc[k].size() - 32 + bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
        }
        for (int a = 0; a < 3; a++) { S.centers[k][a] = uni(-3.f, 3.f); S.centers_right[k][a] = S.centers[k][a] + uni(-0.1f, 0.1f); }
    }
    S.set_ptr.push_back(0);
    for (int s = 0; s < kSets; s++) {
        for (int o = 0; o < kSizes[s]; o++) {
            const int k = (int)(rng() % kK);
            // the rig's last left row, first right row and last row are named early in every set
            const int i = k == 2 && o < 6 ? (o % 3 == 0 ? kRigLeft - 1 : o % 3 == 1 ? kRigLeft : kRows[2] - 1) : (int)(rng() % (unsigned)kRows[k]);
            S.obs_kf.push_back(k); S.obs_idx.push_back(i);
        }
        S.set_ptr.push_back((int32_t)S.obs_kf.size());
        S.ref_obs.push_back(kSizes[s] ? (int32_t)(rng() % (unsigned)kSizes[s]) : 0);
        for (int a = 0; a < 3; a++) S.pos.push_back(uni(6.f, 12.f));
    }
}

int make_key_frames(orbx_matcher *m, const Scene &S, orbx_keyframe **kfs) {
    for (int k = 0; k < kK; k++) {
        orbx_frame_desc d;
        memset(&d, 0, sizeof(d));
        d.keypoints_un = S.kps[k].data(); d.descriptors = S.desc[k].data(); d.n = k == 2 ? kRigLeft : kRows[k];
        d.min_x = 0.f; d.max_x = 640.f; d.min_y = 0.f; d.max_y = 480.f;
        d.scale_factors = S.scale[k]; d.nlevels = kLevels[k];
        if (k == 2) MUST(orbx_keyframe_create_host_fisheye(m, &d, S.kps[k].data() + kRigLeft, kRigRight, nullptr, &kfs[k]));
        else MUST(orbx_keyframe_create_host(m, &d, nullptr, &kfs[k]));
    }
    return 0;
}

// one rounding per operation whatever the compiler's contraction setting is
inline float dot3(const volatile float *a) {
    volatile float p0 = a[0] * a[0], p1 = a[1] * a[1], p2 = a[2] * a[2];
    volatile float s = 0.f + p0;
    s = s + p1;
    s = s + p2;
    return s;
}

// MapPoint::UpdateNormalAndDepth; entries of empty sets keep what they hold
void reference(const Scene &S, std::vector<float> &normal, std::vector<float> &mn, std::vector<float> &mx) {
    for (int s = 0; s < kSets; s++) {
        const int b = S.set_ptr[s], N = S.set_ptr[s + 1] - b;
        if (N == 0) continue;
        const float *P = S.pos.data() + 3 * (size_t)s;
        volatile float acc[3] = {0.f, 0.f, 0.f};
        for (int o = b; o < b + N; o++) {
            const int k = S.obs_kf[o];
            const float *O = k == 2 && S.obs_idx[o] >= kRigLeft ? S.centers_right[k] : S.centers[k];
            volatile float d[3] = {P[0] - O[0], P[1] - O[1], P[2] - O[2]};
            const float nrm = std::sqrt(dot3(d));
            for (int a = 0; a < 3; a++) { volatile float t = d[a] / nrm; acc[a] = acc[a] + t; }
        }
        for (int a = 0; a < 3; a++) normal[3 * (size_t)s + a] = acc[a] / (float)N;
        const int o = b + S.ref_obs[s], k = S.obs_kf[o];
        volatile float pc[3] = {P[0] - S.centers[k][0], P[1] - S.centers[k][1], P[2] - S.centers[k][2]};
        const float dist = std::sqrt(dot3(pc));
        const int level = S.kps[k][S.obs_idx[o]].octave;
        volatile float m = dist * S.scale[k][level];
        mx[s] = m;
        mn[s] = m / S.scale[k][kLevels[k] - 1];
    }
}

// MapPoint.cc:358-403 on mDescriptors.row(idx) of every observation
void distinctive_reference(const Scene &S, std::vector<int32_t> &best) {
    best.assign(kSets, -1);
    for (int s = 0; s < kSets; s++) {
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
    }
}

bool same_bits(const float *a, const float *b, size_t n) { return memcmp(a, b, 4 * n) == 0; }

bool same_counters(orbx_matcher *m, const int64_t *before) {
    int64_t now[6];
    return orbx_matcher_debug_transfers(m, now, 6) >= 0 && memcmp(now, before, sizeof(now)) == 0;
}

}  // namespace

int main(int argc, char **argv) {
    Scene S;
    make_scene(S);
    std::vector<float> wn(3 * kSets, kSentinel), wmn(kSets, kSentinel), wmx(kSets, kSentinel);
    reference(S, wn, wmn, wmx);
    std::vector<int32_t> wbest;
    distinctive_reference(S, wbest);
    if (argc > 1) {
        const int reps = std::max(1, atoi(argv[1]));
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < reps; r++) reference(S, wn, wmn, wmx);
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
        printf("host reference loop: %.2f us per run of %d sets, %d observations\n", us, kSets, (int)S.obs_kf.size());
    }

    orbx_matcher *m = nullptr;
    MUST(orbx_matcher_create(0, &m));
    orbx_keyframe *kfs[kK] = {nullptr, nullptr, nullptr};
    if (make_key_frames(m, S, kfs)) return 1;

    // ---- the flat form; the caller's arrays are heap blocks of exactly the needed size
    std::unique_ptr<float[]> normal(new float[3 * kSets]), mn(new float[kSets]), mx(new float[kSets]);
    std::fill(normal.get(), normal.get() + 3 * kSets, kSentinel);
    std::fill(mn.get(), mn.get() + kSets, kSentinel);
    std::fill(mx.get(), mx.get() + kSets, kSentinel);
    MUST(orbx_keyframe_update_normal_and_depth(m, kK, kfs, &S.centers[0][0], &S.centers_right[0][0], kSets, S.set_ptr.data(), S.obs_kf.data(),
                                               S.obs_idx.data(), S.ref_obs.data(), S.pos.data(), normal.get(), mn.get(), mx.get()));
    CHECK(same_bits(normal.get(), wn.data(), 3 * kSets));   // (the empty set: the sentinel on both sides)
    CHECK(same_bits(mn.get(), wmn.data(), kSets) && same_bits(mx.get(), wmx.data(), kSets));
    CHECK(normal[0] == kSentinel && mn[0] == kSentinel);
    int64_t t[6];
    MUST(orbx_matcher_debug_transfers(m, t, 6));
    CHECK(t[0] == 1 && t[1] == 1 && t[4] == 0);

    // ---- the refresh call into a table whose last slot is written
    orbx_map *map = nullptr;
    MUST(orbx_map_create(0, kCapacity, &map));
    const int32_t set_id[kSets] = {5, kCapacity - 1, 0, 17, 31, 32, 40};
    std::vector<float> p0(S.pos), n0(3 * kSets, 0.25f), a0(kSets, 0.5f), b0(kSets, 9.f);
    std::vector<uint8_t> d0(32 * kSets, 0x5a);
    MUST(orbx_map_update(m, map, kSets, set_id, p0.data(), n0.data(), a0.data(), b0.data(), d0.data()));
    std::unique_ptr<int32_t[]> best(new int32_t[kSets]);
    std::fill(best.get(), best.get() + kSets, -7);
    MUST(orbx_keyframe_refresh_map_points_to_map(m, kK, kfs, &S.centers[0][0], &S.centers_right[0][0], kSets, S.set_ptr.data(), S.obs_kf.data(),
                                                 S.obs_idx.data(), S.ref_obs.data(), map, set_id, best.get()));
    MUST(orbx_matcher_debug_transfers(m, t, 6));
    CHECK(t[0] == 1 && t[1] == 1 && t[4] == 0);
    CHECK(std::equal(wbest.begin(), wbest.end(), best.get()));
    std::unique_ptr<float[]> rp(new float[3 * kSets]), rn(new float[3 * kSets]), ra(new float[kSets]), rb(new float[kSets]);
    std::unique_ptr<uint8_t[]> rd(new uint8_t[32 * kSets]);
    MUST(orbx_map_read(m, map, kSets, set_id, rp.get(), rn.get(), ra.get(), rb.get(), rd.get()));
    CHECK(same_bits(rp.get(), S.pos.data(), 3 * kSets));
    for (int s = 0; s < kSets; s++) {
        if (kSizes[s] == 0) {   // the member's early return: the slot keeps everything
            CHECK(rn[3 * s] == 0.25f && ra[s] == 0.5f && rb[s] == 9.f && rd[32 * s] == 0x5a);
            continue;
        }
        CHECK(same_bits(rn.get() + 3 * s, wn.data() + 3 * s, 3) && same_bits(ra.get() + s, wmn.data() + s, 1) && same_bits(rb.get() + s, wmx.data() + s, 1));
        const int o = S.set_ptr[s] + wbest[s];
        CHECK(memcmp(rd.get() + 32 * s, S.desc[S.obs_kf[o]].data() + 32 * (size_t)S.obs_idx[o], 32) == 0);
    }

    // ---- refused calls and an empty one leave the transfer counters and the table alone
    int64_t before[6];
    MUST(orbx_matcher_debug_transfers(m, before, 6));
    std::vector<int32_t> bad_idx = S.obs_idx, bad_ref = S.ref_obs;
    for (size_t o = 0; o < S.obs_kf.size(); o++)
        if (S.obs_kf[o] == 2) { bad_idx[o] = kRows[2]; break; }   // the rig's N: one past its last right row
    bad_ref[3] = kSizes[3];
    const int32_t dup_id[kSets] = {5, 5, 0, 17, 31, 32, 40};
#define FLAT(C, CR, IDX, REF, POS, NRM) \
    orbx_keyframe_update_normal_and_depth(m, kK, kfs, C, CR, kSets, S.set_ptr.data(), S.obs_kf.data(), IDX, REF, POS, NRM, mn.get(), mx.get())
#define REFRESH(CR, REF, MAP, ID) \
    orbx_keyframe_refresh_map_points_to_map(m, kK, kfs, &S.centers[0][0], CR, kSets, S.set_ptr.data(), S.obs_kf.data(), S.obs_idx.data(), REF, MAP, ID, best.get())
    const float *c = &S.centers[0][0], *cr = &S.centers_right[0][0];
    CHECK(FLAT(c, cr, bad_idx.data(), S.ref_obs.data(), S.pos.data(), normal.get()) == ORBX_E_BAD_ARG);
    CHECK(FLAT(c, cr, S.obs_idx.data(), bad_ref.data(), S.pos.data(), normal.get()) == ORBX_E_BAD_ARG);
    CHECK(FLAT(nullptr, cr, S.obs_idx.data(), S.ref_obs.data(), S.pos.data(), normal.get()) == ORBX_E_BAD_ARG);
    CHECK(FLAT(c, nullptr, S.obs_idx.data(), S.ref_obs.data(), S.pos.data(), normal.get()) == ORBX_E_BAD_ARG);   // a rig is in kfs
    CHECK(FLAT(c, cr, S.obs_idx.data(), nullptr, S.pos.data(), normal.get()) == ORBX_E_BAD_ARG);
    CHECK(FLAT(c, cr, S.obs_idx.data(), S.ref_obs.data(), nullptr, normal.get()) == ORBX_E_BAD_ARG);
    CHECK(FLAT(c, cr, S.obs_idx.data(), S.ref_obs.data(), S.pos.data(), nullptr) == ORBX_E_BAD_ARG);
    CHECK(REFRESH(nullptr, S.ref_obs.data(), map, set_id) == ORBX_E_BAD_ARG);
    CHECK(REFRESH(cr, bad_ref.data(), map, set_id) == ORBX_E_BAD_ARG);
    CHECK(REFRESH(cr, S.ref_obs.data(), nullptr, set_id) == ORBX_E_BAD_ARG);
    CHECK(REFRESH(cr, S.ref_obs.data(), map, nullptr) == ORBX_E_BAD_ARG);
    CHECK(REFRESH(cr, S.ref_obs.data(), map, dup_id) == ORBX_E_BAD_ARG);
    CHECK(orbx_keyframe_update_normal_and_depth(m, kK, kfs, c, cr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == ORBX_OK);
    CHECK(orbx_keyframe_refresh_map_points_to_map(m, kK, kfs, c, cr, 0, nullptr, nullptr, nullptr, nullptr, map, nullptr, nullptr) == ORBX_OK);
    CHECK(same_counters(m, before));
    std::unique_ptr<float[]> rn2(new float[3 * kSets]);
    MUST(orbx_map_read(m, map, kSets, set_id, nullptr, rn2.get(), nullptr, nullptr, nullptr));
    CHECK(same_bits(rn2.get(), rn.get(), 3 * kSets));

    orbx_map_destroy(map);
    for (orbx_keyframe *kf : kfs) orbx_keyframe_destroy(kf);
    orbx_matcher_destroy(m);
    printf("normal depth ok\n");
    return 0;
}
