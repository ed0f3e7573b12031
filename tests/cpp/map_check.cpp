// The device-resident map-point table (orbx_map): create / update / partial update / erase / read, one orbx_frame_search_local_points_map and one
// orbx_keyframe_fuse_map_points_map, each compared with the flat call on the same rows -- return value and every output array.  A 640 x 480 frame of
// 400 synthetic features, 601 map points (three blocks of the scatter / gather kernels, the last one partial) back-projected from the features under an
// identity pose, held in a table of 2048 slots under shuffled, non-contiguous ids that include 0 and 2047; two key frames for Fuse.  Every caller
// array is a heap block of exactly the needed size, so a copy or a kernel write past one ends the run; refused calls must leave the transfer
// counters and the table alone.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt) and
// compiled with -fsanitize=address,undefined, as tests/cpp/keyframe_distinctive_check.cpp.  Prints "map ok" and returns 0.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kLevels = 8, kFeatures = 400, kPoints = 601, kCapacity = 2048;
constexpr float kW = 640.f, kH = 480.f, kF = 400.f, kCx = 320.f, kCy = 240.f;

#define MUST(expr)                                                                   \
    do {                                                                             \
        const int r_ = (expr);                                                       \
        if (r_ < 0) { printf("%s: %d\n", #expr, r_); return 1; }                     \
    } while (0)
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

struct Points {
    std::vector<float> pos, normal, min_dist, max_dist;
    std::vector<uint8_t> desc;
    void resize(size_t n) { pos.resize(3 * n); normal.resize(3 * n); min_dist.resize(n); max_dist.resize(n); desc.resize(32 * n); }
    bool operator==(const Points &o) const {   // bit for bit
        return pos.size() == o.pos.size() && !memcmp(pos.data(), o.pos.data(), 4 * pos.size()) && !memcmp(normal.data(), o.normal.data(), 4 * normal.size()) &&
               !memcmp(min_dist.data(), o.min_dist.data(), 4 * min_dist.size()) && !memcmp(max_dist.data(), o.max_dist.data(), 4 * max_dist.size()) &&
               desc == o.desc;
    }
};

struct Scene {
    float scale[kLevels], inv_sigma2[kLevels];
    std::vector<orbx_keypoint> kps;
    std::vector<uint8_t> desc;
    Points mp;
    std::vector<uint8_t> eligible, has_obs;
    std::vector<int32_t> ids;
    orbx_frame_desc frame() const {
        orbx_frame_desc d;
        memset(&d, 0, sizeof(d));
        d.keypoints_un = kps.data(); d.descriptors = desc.data(); d.n = kFeatures;
        d.min_x = 0.f; d.max_x = kW; d.min_y = 0.f; d.max_y = kH;
        d.scale_factors = scale; d.nlevels = kLevels;
        return d;
    }
};

void make_scene(Scene &S) {
    std::mt19937 rng(31);
    auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    for (int l = 0; l < kLevels; l++) { S.scale[l] = l ? S.scale[l - 1] * 1.2f : 1.f; S.inv_sigma2[l] = 1.f / (S.scale[l] * S.scale[l]); }
    for (int i = 0; i < kFeatures; i++) {
        orbx_keypoint kp;
        memset(&kp, 0, sizeof(kp));
        kp.x = uni(20.f, kW - 20.f); kp.y = uni(20.f, kH - 20.f); kp.octave = (int)(rng() % kLevels);
        kp.size = 31.f * S.scale[kp.octave]; kp.angle = uni(0.f, 360.f); kp.response = 50.f; kp.class_id = -1;
        S.kps.push_back(kp);
        for (int b = 0; b < 32; b++) S.desc.push_back((uint8_t)rng());
    }
    S.mp.resize(kPoints);
    for (int j = 0; j < kPoints; j++) {
        const orbx_keypoint &kp = S.kps[(size_t)(j % kFeatures)];
        const float z = uni(2.f, 20.f), x = (kp.x + uni(-1.f, 1.f) - kCx) / kF * z, y = (kp.y + uni(-1.f, 1.f) - kCy) / kF * z;
        const float d = std::sqrt(x * x + y * y + z * z);
        const float p[3] = {x, y, j % 17 == 0 ? -z : z};   // some behind the camera
        for (int c = 0; c < 3; c++) { S.mp.pos[3 * (size_t)j + c] = p[c]; S.mp.normal[3 * (size_t)j + c] = p[c] / d; }
        S.mp.max_dist[(size_t)j] = d * S.scale[kp.octave] * 1.05f;
        S.mp.min_dist[(size_t)j] = S.mp.max_dist[(size_t)j] / S.scale[kLevels - 1];
        for (int b = 0; b < 32; b++) S.mp.desc[32 * (size_t)j + b] = S.desc[32 * (size_t)(j % kFeatures) + b];
        for (int f = 0; f < 10; f++) { const unsigned bit = rng() % 256; S.mp.desc[32 * (size_t)j + bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
        S.eligible.push_back(rng() % 10 != 0);
        S.has_obs.push_back(rng() % 12 != 0);
    }
    std::vector<int32_t> all(kCapacity - 2);
    std::iota(all.begin(), all.end(), 1);
    std::shuffle(all.begin(), all.end(), rng);
    S.ids.assign(all.begin(), all.begin() + kPoints - 2);
    S.ids.push_back(0); S.ids.push_back(kCapacity - 1);
    std::shuffle(S.ids.begin(), S.ids.end(), rng);
}

// the rows [b, e) of P as a set of their own
Points rows(const Points &P, size_t b, size_t e) {
    Points R;
    R.pos.assign(P.pos.begin() + 3 * b, P.pos.begin() + 3 * e); R.normal.assign(P.normal.begin() + 3 * b, P.normal.begin() + 3 * e);
    R.min_dist.assign(P.min_dist.begin() + b, P.min_dist.begin() + e); R.max_dist.assign(P.max_dist.begin() + b, P.max_dist.begin() + e);
    R.desc.assign(P.desc.begin() + 32 * b, P.desc.begin() + 32 * e);
    return R;
}

int read_all(orbx_matcher *m, orbx_map *map, const std::vector<int32_t> &ids, Points &out) {
    const size_t n = ids.size();
    // heap blocks of exactly the needed size
    std::unique_ptr<float[]> pos(new float[3 * n]), normal(new float[3 * n]), mn(new float[n]), mx(new float[n]);
    std::unique_ptr<uint8_t[]> desc(new uint8_t[32 * n]);
    MUST(orbx_map_read(m, map, (int)n, ids.data(), pos.get(), normal.get(), mn.get(), mx.get(), desc.get()));
    out.pos.assign(pos.get(), pos.get() + 3 * n); out.normal.assign(normal.get(), normal.get() + 3 * n);
    out.min_dist.assign(mn.get(), mn.get() + n); out.max_dist.assign(mx.get(), mx.get() + n); out.desc.assign(desc.get(), desc.get() + 32 * n);
    return 0;
}

bool same_counters(orbx_matcher *m, const int64_t *before) {
    int64_t now[6];
    return orbx_matcher_debug_transfers(m, now, 6) >= 0 && memcmp(now, before, sizeof(now)) == 0;
}

}  // namespace

int main() {
    Scene S;
    make_scene(S);
    orbx_matcher *m = nullptr, *other = nullptr;
    MUST(orbx_matcher_create(0, &m));
    MUST(orbx_matcher_create(0, &other));
    orbx_map *map = nullptr;
    orbx_map *none = reinterpret_cast<orbx_map *>(&none);
    CHECK(orbx_map_create(0, ORBX_MAX_MAP_POINTS + 1, &none) == ORBX_E_TOO_LARGE && none == nullptr);
    MUST(orbx_map_create(0, kCapacity, &map));

    // ---- the store: written in pieces whose sizes straddle the kernels' 64-point blocks, through two contexts
    Points want = S.mp, got;
    const size_t pieces[] = {1, 63, 64, 65, 255, 153};
    size_t at = 0;
    for (size_t p = 0; p < sizeof(pieces) / sizeof(pieces[0]); p++) {
        const Points R = rows(S.mp, at, at + pieces[p]);
        MUST(orbx_map_update(p % 2 ? other : m, map, (int)pieces[p], S.ids.data() + at, R.pos.data(), R.normal.data(), R.min_dist.data(), R.max_dist.data(),
                             R.desc.data()));
        at += pieces[p];
    }
    CHECK(at == (size_t)kPoints);
    if (read_all(m, map, S.ids, got)) return 1;
    CHECK(got == want);
    // partial updates: the descriptor of rows [100, 357), pos + normal of rows [300, 556): exactly those fields change
    std::mt19937 rng(77);
    for (size_t j = 100; j < 357; j++) for (int b = 0; b < 32; b++) want.desc[32 * j + b] = (uint8_t)rng();
    MUST(orbx_map_update(m, map, 257, S.ids.data() + 100, nullptr, nullptr, nullptr, nullptr, want.desc.data() + 32 * 100));
    for (size_t j = 300; j < 556; j++) for (int c = 0; c < 3; c++) { want.pos[3 * j + c] += 0.25f; want.normal[3 * j + c] = -want.normal[3 * j + c]; }
    MUST(orbx_map_update(other, map, 256, S.ids.data() + 300, want.pos.data() + 3 * 300, want.normal.data() + 3 * 300, nullptr, nullptr, nullptr));
    if (read_all(other, map, S.ids, got)) return 1;
    CHECK(got == want);
    // back to the scene's points for the searches
    MUST(orbx_map_update(m, map, kPoints, S.ids.data(), S.mp.pos.data(), S.mp.normal.data(), nullptr, nullptr, S.mp.desc.data()));
    if (read_all(m, map, S.ids, got)) return 1;
    CHECK(got == S.mp);

    // ---- refusals leave the counters and the table alone
    int64_t before[6];
    MUST(orbx_matcher_debug_transfers(m, before, 6));
    std::vector<int32_t> bad = {S.ids[0], kCapacity}, neg = {-1}, dup = {S.ids[3], S.ids[4], S.ids[3]};
    int32_t unwritten = 1;
    while (std::find(S.ids.begin(), S.ids.end(), unwritten) != S.ids.end()) unwritten++;
    float f3[9] = {0};
    uint8_t d3[96] = {0};
    CHECK(orbx_map_read(m, map, 2, bad.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == ORBX_E_BAD_ARG);
    CHECK(orbx_map_read(m, map, 1, neg.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == ORBX_E_BAD_ARG);
    CHECK(orbx_map_read(m, map, 1, &unwritten, nullptr, nullptr, nullptr, nullptr, nullptr) == ORBX_E_BAD_ARG);
    CHECK(orbx_map_read(m, map, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == ORBX_E_BAD_ARG);
    CHECK(orbx_map_update(m, map, 3, dup.data(), f3, f3, f3, f3, d3) == ORBX_E_BAD_ARG);
    CHECK(orbx_map_update(m, map, 1, &unwritten, f3, f3, f3, nullptr, d3) == ORBX_E_BAD_ARG);   // a first update with a field missing
    CHECK(orbx_map_update(m, map, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == ORBX_OK);
    CHECK(orbx_map_erase(map, 2, bad.data()) == ORBX_E_BAD_ARG);
    CHECK(same_counters(m, before));
    if (read_all(m, map, S.ids, got)) return 1;
    CHECK(got == S.mp);

    // ---- SearchLocalPoints: flat against _map (identity pose)
    const orbx_frame_desc fd = S.frame();
    orbx_frame *F = nullptr;
    MUST(orbx_frame_create(m, kFeatures, &F));
    MUST(orbx_frame_load_host(F, &fd));
    orbx_camera cam;
    memset(&cam, 0, sizeof(cam));
    cam.fx = cam.fy = kF; cam.cx = kCx; cam.cy = kCy;
    orbx_frame_pose pose;
    memset(&pose, 0, sizeof(pose));
    pose.Rcw[0] = pose.Rcw[4] = pose.Rcw[8] = 1.f;
    const float lsf = std::log(1.2f);
    std::unique_ptr<uint8_t[]> iv_a(new uint8_t[kPoints]), iv_b(new uint8_t[kPoints]);
    std::unique_ptr<int32_t[]> fm_a(new int32_t[kFeatures]), fm_b(new int32_t[kFeatures]);
    const int na = orbx_frame_search_local_points(m, F, nullptr, &cam, &pose, lsf, 0.5f, kPoints, S.mp.pos.data(), S.mp.normal.data(), S.mp.min_dist.data(),
                                                  S.mp.max_dist.data(), S.mp.desc.data(), S.eligible.data(), S.has_obs.data(), 3.f, 0.8f, 0, 0.f, iv_a.get(),
                                                  fm_a.get());
    int64_t flat_t[6], map_t[6];
    MUST(orbx_matcher_debug_transfers(m, flat_t, 6));
    const int nb = orbx_frame_search_local_points_map(m, F, nullptr, &cam, &pose, lsf, 0.5f, kPoints, map, S.ids.data(), S.eligible.data(), S.has_obs.data(),
                                                      3.f, 0.8f, 0, 0.f, iv_b.get(), fm_b.get());
    MUST(orbx_matcher_debug_transfers(m, map_t, 6));
    CHECK(na >= 100 && nb == na);
    CHECK(!memcmp(iv_a.get(), iv_b.get(), kPoints) && !memcmp(fm_a.get(), fm_b.get(), 4 * kFeatures));
    CHECK(flat_t[0] == 1 && map_t[0] == 1 && flat_t[1] == map_t[1] && flat_t[5] == map_t[5] && flat_t[4] == 0 && map_t[4] == 0);
    CHECK(std::llabs((flat_t[2] - map_t[2]) - 60ll * kPoints) <= 6 * 256);   // run extents: 60 bytes per point less, to within the alignment of six buffers

    // ---- Fuse into two key frames (the frame itself, twice), with a skip row and `projected`: flat against _map, through the OTHER context
    orbx_keyframe *kfs[2] = {nullptr, nullptr};
    for (orbx_keyframe *&kf : kfs) MUST(orbx_keyframe_create_host(m, &fd, S.inv_sigma2, &kf));
    const orbx_camera cams[2] = {cam, cam};
    const orbx_frame_pose poses[2] = {pose, pose};
    std::vector<uint8_t> skip(2 * (size_t)kPoints);
    for (size_t i = 0; i < skip.size(); i++) skip[i] = i % 9 == 0;
    const size_t total = 2 * (size_t)kPoints;
    std::unique_ptr<int32_t[]> bi_a(new int32_t[total]), bd_a(new int32_t[total]), bi_b(new int32_t[total]), bd_b(new int32_t[total]);
    std::unique_ptr<uint8_t[]> pr_a(new uint8_t[total]), pr_b(new uint8_t[total]);
    MUST(orbx_keyframe_fuse_map_points(other, 2, kfs, cams, poses, 3.f, lsf, 0, kPoints, S.mp.pos.data(), S.mp.normal.data(), S.mp.min_dist.data(),
                                       S.mp.max_dist.data(), S.mp.desc.data(), skip.data(), bi_a.get(), bd_a.get(), pr_a.get()));
    MUST(orbx_keyframe_fuse_map_points_map(other, 2, kfs, cams, poses, 3.f, lsf, 0, kPoints, map, S.ids.data(), skip.data(), bi_b.get(), bd_b.get(),
                                           pr_b.get()));
    CHECK(!memcmp(bi_a.get(), bi_b.get(), 4 * total) && !memcmp(bd_a.get(), bd_b.get(), 4 * total) && !memcmp(pr_a.get(), pr_b.get(), total));
    int found = 0;
    for (size_t i = 0; i < total; i++) found += bi_a[i] >= 0 && bd_a[i] <= ORBX_TH_LOW;
    CHECK(found >= 200);

    // ---- erase: the slot is refused by every call until it is written whole again
    MUST(orbx_matcher_debug_transfers(m, before, 6));
    MUST(orbx_map_erase(map, 1, S.ids.data() + 5));
    CHECK(orbx_frame_search_local_points_map(m, F, nullptr, &cam, &pose, lsf, 0.5f, kPoints, map, S.ids.data(), nullptr, nullptr, 3.f, 0.8f, 0, 0.f,
                                             iv_b.get(), fm_b.get()) == ORBX_E_BAD_ARG);
    CHECK(orbx_map_update(m, map, 1, S.ids.data() + 5, nullptr, nullptr, nullptr, nullptr, S.mp.desc.data()) == ORBX_E_BAD_ARG);
    CHECK(same_counters(m, before));
    const Points R = rows(S.mp, 5, 6);
    MUST(orbx_map_update(m, map, 1, S.ids.data() + 5, R.pos.data(), R.normal.data(), R.min_dist.data(), R.max_dist.data(), R.desc.data()));
    CHECK(orbx_frame_search_local_points_map(m, F, nullptr, &cam, &pose, lsf, 0.5f, kPoints, map, S.ids.data(), S.eligible.data(), S.has_obs.data(), 3.f,
                                             0.8f, 0, 0.f, iv_b.get(), fm_b.get()) == na);
    CHECK(!memcmp(iv_a.get(), iv_b.get(), kPoints) && !memcmp(fm_a.get(), fm_b.get(), 4 * kFeatures));

    for (orbx_keyframe *kf : kfs) orbx_keyframe_destroy(kf);
    orbx_frame_destroy(F);
    orbx_map_destroy(map);
    orbx_matcher_destroy(m);
    orbx_matcher_destroy(other);
    printf("map ok\n");
    return 0;
}
