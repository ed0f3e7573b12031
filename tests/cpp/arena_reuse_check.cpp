// One matcher context, calls of different sizes: every entry point sizes its arena from the buffers it carves, so a call that still FITS the capacity
// an earlier, smaller call left behind must find room for all of its buffers.  Per entry point, on ONE context: a big call, a call about 1.5 times
// as big (inside the arena's 3/2 growth: nothing is re-allocated), a small one; each result must equal the same call on a fresh context.
// Stand-alone: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt) and compiled with -fsanitize=address,undefined,
// which sees a staged upload or a kernel's output running past the arena or its pinned mirror.  Prints "arena reuse ok" and returns 0.
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kFrame = 200, kW = 640, kH = 480, kLevels = 8;
const int kSizes[3] = {2000, 3060, 500};

struct Scene {   // a frame of kFrame features and a pool of queries that look at them
    std::vector<orbx_keypoint> kps;
    std::vector<uint8_t> desc, occupied;
    std::vector<float> u_right, scale, inv_sigma2;
    orbx_frame_desc frame;
    // queries (as many as the largest call takes)
    std::vector<float> qx, qy, qxr, qr, q_angle, view_cos;
    std::vector<int32_t> q_level, q_min, q_max;
    std::vector<uint8_t> q_desc, q_has_obs, q_in_view;
};

Scene make_scene(uint32_t seed, int nq) {
    std::mt19937 rng(seed);
    auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    Scene S;
    S.scale.resize(kLevels); S.inv_sigma2.resize(kLevels);
    for (int l = 0; l < kLevels; l++) { S.scale[l] = l ? S.scale[l - 1] * 1.2f : 1.0f; S.inv_sigma2[l] = 1.0f / (S.scale[l] * S.scale[l]); }
    S.kps.resize(kFrame); S.desc.resize(32 * kFrame); S.occupied.resize(kFrame); S.u_right.resize(kFrame);
    for (int i = 0; i < kFrame; i++) {
        orbx_keypoint &k = S.kps[i];
        memset(&k, 0, sizeof(k));
        k.x = uni(20.f, kW - 20.f); k.y = uni(20.f, kH - 20.f); k.angle = uni(0.f, 359.9f); k.octave = (int)(rng() % kLevels);
        k.size = 31.f * S.scale[k.octave]; k.response = uni(20.f, 100.f); k.class_id = -1;
        for (int b = 0; b < 32; b++) S.desc[32 * i + b] = (uint8_t)rng();
        S.occupied[i] = rng() % 8 == 0;
        S.u_right[i] = rng() % 3 ? k.x - uni(1.f, 30.f) : -1.f;
    }
    memset(&S.frame, 0, sizeof(S.frame));
    S.frame.keypoints_un = S.kps.data(); S.frame.descriptors = S.desc.data(); S.frame.n = kFrame;
    S.frame.min_x = 0.f; S.frame.max_x = (float)kW; S.frame.min_y = 0.f; S.frame.max_y = (float)kH;
    S.frame.scale_factors = S.scale.data(); S.frame.nlevels = kLevels; S.frame.u_right = S.u_right.data();
    S.qx.resize(nq); S.qy.resize(nq); S.qxr.resize(nq); S.qr.resize(nq); S.q_angle.resize(nq); S.view_cos.resize(nq);
    S.q_level.resize(nq); S.q_min.resize(nq); S.q_max.resize(nq);
    S.q_desc.resize(32 * (size_t)nq); S.q_has_obs.resize(nq); S.q_in_view.resize(nq);
    for (int j = 0; j < nq; j++) {   // a noisy copy of feature j % kFrame: many queries compete for one feature
        const int i = j % kFrame;
        const orbx_keypoint &k = S.kps[i];
        S.qx[j] = k.x + uni(-3.f, 3.f); S.qy[j] = k.y + uni(-3.f, 3.f);
        S.qxr[j] = S.u_right[i] >= 0.f ? S.u_right[i] + uni(-1.f, 1.f) : -1.f;
        S.q_level[j] = k.octave; S.q_min[j] = k.octave - 1; S.q_max[j] = k.octave + 1;
        S.qr[j] = 7.f * S.scale[k.octave];
        S.q_angle[j] = k.angle + uni(-4.f, 4.f);
        if (S.q_angle[j] < 0.f) S.q_angle[j] += 360.f;
        if (S.q_angle[j] >= 360.f) S.q_angle[j] -= 360.f;
        S.view_cos[j] = uni(0.9f, 1.0f);
        memcpy(&S.q_desc[32 * (size_t)j], &S.desc[32 * i], 32);
        for (int f = 0; f < 12; f++) { const unsigned b = rng() % 256; S.q_desc[32 * (size_t)j + b / 8] ^= (uint8_t)(1u << (b % 8)); }
        S.q_has_obs[j] = rng() % 4 != 0;
        S.q_in_view[j] = rng() % 10 != 0;
    }
    return S;
}

typedef std::function<int(orbx_matcher *, int, std::vector<int32_t> &)> Call;   // (context, size, result) -> ORBX_* code or a match count

int check(const char *name, const Call &call) {
    orbx_matcher *reused = nullptr;
    if (orbx_matcher_create(0, &reused) != ORBX_OK) { printf("%s: no context\n", name); return 1; }
    int bad = 0;
    for (int size : kSizes) {
        orbx_matcher *fresh = nullptr;
        if (orbx_matcher_create(0, &fresh) != ORBX_OK) { printf("%s: no context\n", name); return 1; }
        std::vector<int32_t> a, b;
        const int ra = call(reused, size, a), rb = call(fresh, size, b);
        orbx_matcher_destroy(fresh);
        if (ra < 0 || ra != rb || a != b) { printf("%s, size %d: %d on the reused context, %d on a fresh one, results %s\n", name, size, ra, rb, a == b ? "equal" : "DIFFER"); bad++; }
        else printf("%s, size %d: %d, %zu values equal\n", name, size, ra, a.size());
    }
    orbx_matcher_destroy(reused);
    return bad;
}

}  // namespace

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const int nq_max = 3060;
    const Scene S = make_scene(20240607u, nq_max);
    int bad = 0;

    bad += check("orbx_search_by_projection_frame", [&](orbx_matcher *m, int nq, std::vector<int32_t> &out) {   // u_right, mask, angles, has_obs
        out.assign(kFrame, -7);
        return orbx_search_by_projection_frame(m, &S.frame, S.occupied.data(), nq, S.qx.data(), S.qy.data(), S.qxr.data(), S.q_level.data(), S.q_angle.data(),
                                               S.q_desc.data(), S.q_has_obs.data(), 7.f, 0, 1, out.data());
    });
    bad += check("orbx_search_by_projection_mappoints", [&](orbx_matcher *m, int nq, std::vector<int32_t> &out) {
        out.assign(kFrame, -7);
        return orbx_search_by_projection_mappoints(m, &S.frame, S.occupied.data(), nq, S.qx.data(), S.qy.data(), S.qxr.data(), S.q_level.data(),
                                                   S.view_cos.data(), S.q_desc.data(), S.q_in_view.data(), S.q_has_obs.data(), 3.f, 0.8f, out.data());
    });
    bad += check("orbx_search_by_projection_window", [&](orbx_matcher *m, int nq, std::vector<int32_t> &out) {
        out.assign(kFrame, -7);
        return orbx_search_by_projection_window(m, &S.frame, S.occupied.data(), nq, S.qx.data(), S.qy.data(), S.qr.data(), S.q_min.data(), S.q_max.data(),
                                                S.q_angle.data(), S.q_desc.data(), S.q_has_obs.data(), 64.f, 1, out.data());
    });
    bad += check("orbx_fuse_search", [&](orbx_matcher *m, int nq, std::vector<int32_t> &out) {
        out.assign(2 * (size_t)nq, -7);
        return orbx_fuse_search(m, &S.frame, S.inv_sigma2.data(), nq, S.qx.data(), S.qy.data(), S.qxr.data(), S.qr.data(), S.q_level.data(), S.q_desc.data(), 0,
                                out.data(), out.data() + nq);
    });
    bad += check("orbx_knn2", [&](orbx_matcher *m, int nq, std::vector<int32_t> &out) {
        out.assign(4 * (size_t)nq, -7);
        return orbx_knn2(m, S.q_desc.data(), nq, S.desc.data(), kFrame, out.data(), out.data() + 2 * (size_t)nq);
    });
    // F1 = the first n1 queries as level-0 keypoints (every one of them is a query of the window search), F2 = the frame
    std::vector<orbx_keypoint> kps1(nq_max);
    for (int j = 0; j < nq_max; j++) { kps1[j] = S.kps[j % kFrame]; kps1[j].x = S.qx[j]; kps1[j].y = S.qy[j]; kps1[j].angle = S.q_angle[j]; kps1[j].octave = 0; }
    bad += check("orbx_search_for_initialization", [&](orbx_matcher *m, int n1, std::vector<int32_t> &out) {
        std::vector<float> prev(2 * (size_t)n1);
        for (int j = 0; j < n1; j++) { prev[2 * j] = S.qx[j]; prev[2 * j + 1] = S.qy[j]; }
        out.assign(3 * (size_t)n1, -7);
        const int r = orbx_search_for_initialization(m, kps1.data(), S.q_desc.data(), n1, &S.frame, prev.data(), 40, 0.9f, 1, out.data());
        memcpy(out.data() + n1, prev.data(), 8 * (size_t)n1);   // vbPrevMatched comes back updated
        return r;
    });
    bad += check("orbx_distinctive_descriptors", [&](orbx_matcher *m, int n_sets, std::vector<int32_t> &out) {
        std::vector<int32_t> ptr((size_t)n_sets + 1);   // set s: 1 + s % 5 consecutive descriptors of the query pool
        ptr[0] = 0;
        for (int s = 0; s < n_sets; s++) ptr[s + 1] = ptr[s] + 1 + s % 5;
        std::vector<uint8_t> d(32 * (size_t)ptr[n_sets]);
        for (size_t k = 0; k < d.size(); k += 32) memcpy(&d[k], &S.q_desc[k % (32 * (size_t)nq_max)], 32);
        out.assign(n_sets, -7);
        return orbx_distinctive_descriptors(m, d.data(), ptr.data(), n_sets, out.data());
    });
    if (bad) { printf("arena reuse FAILED: %d\n", bad); return 1; }
    printf("arena reuse ok\n");
    return 0;
}
