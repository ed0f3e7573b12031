// LoopClosing's Sim3 searches on FISHEYE-STEREO resident key frames -- orbx_keyframe_search_by_projection_sim3_fisheye and
// orbx_keyframe_fuse_map_points_sim3_fisheye -- with K = 2 rig key frames of unequal N_left / N_right and 300 map points, with and without skip /
// occupied / projected (and the projections), both projection forms: every variant on a FRESH matcher context, then all of them again on ONE context
// that served a call three times as large first (the arena and the pinned mirror are then larger than the call and hold the larger call's bytes).
// Both runs must give the same results; every caller array is a heap block of exactly the size the call may write (match / occupied rows: N_left +
// N_right entries), rows the call must not touch keep their sentinel, a match row is -1 from N_left on and a Fuse index is below N_left.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt) and
// compiled with -fsanitize=address,undefined, as tests/cpp/keyframe_sim3_check.cpp.  Prints "keyframe sim3 fisheye ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kW = 512, kH = 512, kLevels = 8, kK = 2, kMapPoints = 300, kSentinel = -7;
constexpr float kDepth = 5.f;
const float kCam[8] = {190.978f, 190.973f, 254.932f, 256.897f, 0.00348f, 0.000715f, -0.00205f, 0.000203f};   // a TUM-VI-like KannalaBrandt8 camera

#define MUST(expr)                                                                   \
    do {                                                                             \
        const int r_ = (expr);                                                       \
        if (r_ < 0) { printf("%s: %d\n", #expr, r_); return 1; }                     \
    } while (0)

struct Scene {
    float scale[kLevels];
    std::vector<orbx_keypoint> left[kK], right[kK];
    std::vector<uint8_t> desc[kK];          // N_left + N_right rows
    orbx_fisheye_view views[2][kK];         // [projection form][key frame]: form 1 carries the pinhole fx, fy, cx, cy alone
    std::vector<float> pos, normal, min_dist, max_dist;
    std::vector<uint8_t> mp_desc;
};

void project(const float *p, float *u, float *v) {   // KannalaBrandt8::project, plainly (the features only have to lie NEAR the device's projections)
    const float th = std::atan2(std::hypot(p[0], p[1]), p[2]), psi = std::atan2(p[1], p[0]), t2 = th * th;
    const float r = th * (1.f + t2 * (kCam[4] + t2 * (kCam[5] + t2 * (kCam[6] + t2 * kCam[7]))));
    *u = kCam[0] * r * std::cos(psi) + kCam[2]; *v = kCam[1] * r * std::sin(psi) + kCam[3];
}

// n_mp map points at depth kDepth in front of key frame 0 (identity pose; key frame 1 is shifted by 5 cm); each key frame's LEFT camera holds a jittered
// feature for two thirds of the points (same octave as the point predicts, a few descriptor bits flipped) and random clutter, its right camera clutter
// only; every third point is a near duplicate of its predecessor, so queries compete for a feature
void make_scene(int n_mp, Scene &S) {
    std::mt19937 rng(11);
    auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    for (int l = 0; l < kLevels; l++) S.scale[l] = l ? S.scale[l - 1] * 1.2f : 1.f;
    std::vector<int> lvl(n_mp);
    for (int i = 0; i < n_mp; i++) {
        const bool dup = i % 3 == 2;
        float p[3] = {dup ? 0.f : uni(-1.6f, 1.6f) * kDepth, dup ? 0.f : uni(-1.6f, 1.6f) * kDepth, kDepth};   // (some outside the image)
        if (dup) for (int c = 0; c < 3; c++) p[c] = S.pos[3 * (size_t)(i - 1) + c] + uni(-0.01f, 0.01f);
        if (i % 17 == 5) p[2] = -p[2];   // behind the cameras
        const float d = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        lvl[i] = dup ? lvl[i - 1] : (int)(rng() % (kLevels - 1));
        for (int c = 0; c < 3; c++) { S.pos.push_back(p[c]); S.normal.push_back(i % 13 == 7 ? -p[c] / d : p[c] / d); }   // (some seen from behind)
        S.max_dist.push_back(d * S.scale[lvl[i]] * 0.97f); S.min_dist.push_back(i % 19 == 3 ? 2.f * d : 0.2f * d);
        for (int b = 0; b < 32; b++) S.mp_desc.push_back(dup ? S.mp_desc[32 * (size_t)(i - 1) + b] : (uint8_t)rng());
        if (dup) for (int f = 0; f < 6; f++) { const unsigned b = rng() % 256; S.mp_desc[32 * (size_t)i + b / 8] ^= (uint8_t)(1u << (b % 8)); }
    }
    auto clutter = [&](std::vector<orbx_keypoint> &kps, std::vector<uint8_t> &desc, int n) {
        for (int j = 0; j < n; j++) {
            orbx_keypoint kp;
            memset(&kp, 0, sizeof(kp));
            kp.x = uni(1.f, kW - 2.f); kp.y = uni(1.f, kH - 2.f); kp.octave = (int)(rng() % kLevels);
            kp.size = 31.f * S.scale[kp.octave]; kp.angle = uni(0.f, 360.f); kp.response = 20.f; kp.class_id = -1;
            kps.push_back(kp);
            for (int b = 0; b < 32; b++) desc.push_back((uint8_t)rng());
        }
    };
    for (int k = 0; k < kK; k++) {
        for (int form = 0; form < 2; form++) {
            orbx_fisheye_view &V = S.views[form][k];
            memset(&V, 0, sizeof(V));
            V.R[0] = V.R[4] = V.R[8] = 1.f;
            V.t[0] = 0.05f * k; V.twc[0] = -0.05f * k;
            for (int c = 0; c < (form ? 4 : 8); c++) V.params[c] = kCam[c];
        }
        for (int i = 0; i < n_mp; i++) {
            if (i % 3 == k || S.pos[3 * (size_t)i + 2] <= 0) continue;
            const float pc[3] = {S.pos[3 * (size_t)i] + 0.05f * k, S.pos[3 * (size_t)i + 1], S.pos[3 * (size_t)i + 2]};
            orbx_keypoint kp;
            memset(&kp, 0, sizeof(kp));
            project(pc, &kp.x, &kp.y);
            kp.x += uni(-1.f, 1.f); kp.y += uni(-1.f, 1.f);
            if (kp.x < 1 || kp.x >= kW - 1 || kp.y < 1 || kp.y >= kH - 1) continue;
            kp.octave = lvl[i] > 0 && rng() % 4 == 0 ? lvl[i] - 1 : lvl[i];
            kp.size = 31.f * S.scale[kp.octave]; kp.angle = uni(0.f, 360.f); kp.response = 50.f; kp.class_id = -1;
            S.left[k].push_back(kp);
            for (int b = 0; b < 32; b++) S.desc[k].push_back(S.mp_desc[32 * (size_t)i + b]);
            for (int f = 0; f < 8; f++) { const unsigned b = rng() % 256; S.desc[k][S.desc[k].size() - 32 + b / 8] ^= (uint8_t)(1u << (b % 8)); }
        }
        clutter(S.left[k], S.desc[k], 40 + 25 * k);        // (and unequal N_left)
        clutter(S.right[k], S.desc[k], 90 - 35 * k);       // the right camera's rows behind the left one's: unequal N_right
    }
}

int make_key_frames(orbx_matcher *m, const Scene &S, orbx_keyframe **kfs) {
    for (int k = 0; k < kK; k++) {
        orbx_frame_desc d;
        memset(&d, 0, sizeof(d));
        d.keypoints_un = S.left[k].data(); d.descriptors = S.desc[k].data(); d.n = (int)S.left[k].size();
        d.min_x = 0.f; d.max_x = (float)kW; d.min_y = 0.f; d.max_y = (float)kH;
        d.scale_factors = S.scale; d.nlevels = kLevels;
        MUST(orbx_keyframe_create_host_fisheye(m, &d, S.right[k].data(), (int)S.right[k].size(), nullptr, &kfs[k]));
    }
    return 0;
}

// every result of the variants of both calls, in call order (heap blocks of exactly the size a call may write)
typedef std::vector<std::vector<int32_t>> Results;

int bytes_to(const std::vector<uint8_t> &b, Results &out) { out.emplace_back(b.begin(), b.end()); return 0; }
int floats_to(const std::vector<float> &f, Results &out) {
    std::vector<int32_t> v(f.size());
    memcpy(v.data(), f.data(), 4 * f.size());
    out.push_back(v);
    return 0;
}

int run_variants(orbx_matcher *m, orbx_keyframe *const *kfs, const Scene &S, int n_mp, Results &out, int *matched, int *fused) {
    const size_t total = (size_t)kK * n_mp;
    const float log_sf = std::log(1.2f);
    int NL[kK], NR[kK], N[kK];
    for (int k = 0; k < kK; k++) {
        MUST(orbx_keyframe_counts(kfs[k], &NL[k], &NR[k]));
        N[k] = NL[k] + NR[k];
        if (NL[k] != (int)S.left[k].size() || NR[k] != (int)S.right[k].size()) { printf("FAILED: counts of key frame %d\n", k); return 1; }
    }
    std::vector<uint8_t> skip(total);
    for (size_t i = 0; i < total; i++) skip[i] = i % 11 == 0;
    std::vector<uint8_t> occ0((size_t)N[0]);
    for (int i = 0; i < N[0]; i++) occ0[(size_t)i] = i % 7 == 0 || i >= NL[0];   // (the right camera's entries are not read)
    const uint8_t *occ_rows[kK] = {occ0.data(), nullptr};
    *matched = *fused = 0;
    for (int variant = 0; variant < 4; variant++) {   // form = variant % 2; flags and optional outputs on the upper two
        const bool full = variant >= 2;
        std::vector<int32_t> row0((size_t)N[0], kSentinel), row1((size_t)N[1], kSentinel), nm(kK, kSentinel);
        int32_t *rows[kK] = {row0.data(), row1.data()};
        std::vector<uint8_t> pr(full ? total : 0, 9);
        std::vector<float> pu(full ? total : 0, -3.f), pv(full ? total : 0, -3.f);
        MUST(orbx_keyframe_search_by_projection_sim3_fisheye(m, kK, kfs, S.views[variant % 2], 8.f, 1.5f, log_sf, variant % 2, n_mp, S.pos.data(),
                                                             S.normal.data(), S.min_dist.data(), S.max_dist.data(), S.mp_desc.data(),
                                                             full ? skip.data() : nullptr, full ? occ_rows : nullptr, rows, nm.data(),
                                                             full ? pr.data() : nullptr, full ? pu.data() : nullptr, full ? pv.data() : nullptr));
        for (int k = 0; k < kK; k++) {
            const std::vector<int32_t> &row = k ? row1 : row0;
            int cnt = 0;
            for (int i = 0; i < N[k]; i++) {
                const int32_t v = row[(size_t)i];
                if (v < -1 || v >= n_mp || (i >= NL[k] && v != -1)) { printf("FAILED: match[%d] = %d of key frame %d\n", i, v, k); return 1; }
                if (full && k == 0 && v >= 0 && occ0[(size_t)i]) { printf("FAILED: an occupied feature was matched\n"); return 1; }
                cnt += v >= 0;
            }
            if (cnt != nm[(size_t)k]) { printf("FAILED: nmatches %d, %d rows set\n", nm[(size_t)k], cnt); return 1; }
            *matched += cnt;
        }
        out.push_back(row0); out.push_back(row1); out.push_back(nm);
        if (full) {
            for (size_t i = 0; i < total; i++)
                if (pr[i] > 1 || (pr[i] && skip[i])) { printf("FAILED: projected[%zu] = %d\n", i, pr[i]); return 1; }
            for (size_t i = 0; i < total; i++) if (!pr[i]) pu[i] = pv[i] = 0.f;   // meaningful where projected == 1
            bytes_to(pr, out); floats_to(pu, out); floats_to(pv, out);
        }
    }
    for (int variant = 0; variant < 2; variant++) {
        const bool full = variant == 1;
        std::vector<int32_t> bi(total, kSentinel), bd(total, kSentinel);
        std::vector<uint8_t> pr(full ? total : 0, 9);
        MUST(orbx_keyframe_fuse_map_points_sim3_fisheye(m, kK, kfs, S.views[0], 3.f, log_sf, n_mp, S.pos.data(), S.normal.data(), S.min_dist.data(),
                                                        S.max_dist.data(), S.mp_desc.data(), full ? skip.data() : nullptr, bi.data(), bd.data(),
                                                        full ? pr.data() : nullptr));
        for (size_t i = 0; i < total; i++) {
            if (bi[i] < -1 || bi[i] >= NL[i / (size_t)n_mp] || bd[i] < 0 || bd[i] > 256 || (bi[i] < 0) != (bd[i] == 256)) { printf("FAILED: fuse row %zu: %d %d\n", i, bi[i], bd[i]); return 1; }
            *fused += bd[i] <= ORBX_TH_LOW;
        }
        out.push_back(bi); out.push_back(bd);
        if (full) bytes_to(pr, out);
    }
    return 0;
}

}  // namespace

int main() {
    Scene S, Big;
    make_scene(kMapPoints, S);
    make_scene(3 * kMapPoints, Big);
    // every variant on a fresh context
    Results fresh;
    int matched = 0, fused = 0;
    {
        orbx_matcher *m = nullptr;
        MUST(orbx_matcher_create(0, &m));
        orbx_keyframe *kfs[kK] = {nullptr, nullptr};
        if (make_key_frames(m, S, kfs)) return 1;
        orbx_matcher_destroy(m);   // the key frames belong to no matcher
        orbx_matcher *f = nullptr;
        MUST(orbx_matcher_create(0, &f));
        if (run_variants(f, kfs, S, kMapPoints, fresh, &matched, &fused)) return 1;
        orbx_matcher_destroy(f);
        // ONE context: a call three times as large first, then the same variants twice
        orbx_matcher *m1 = nullptr;
        MUST(orbx_matcher_create(0, &m1));
        orbx_keyframe *big[kK] = {nullptr, nullptr};
        if (make_key_frames(m1, Big, big)) return 1;
        Results large;
        int mb = 0, fb = 0;
        if (run_variants(m1, big, Big, 3 * kMapPoints, large, &mb, &fb)) return 1;
        printf("large call: %d matches, %d fuse candidates within TH_LOW\n", mb, fb);
        for (int rep = 0; rep < 2; rep++) {
            Results again;
            int ma = 0, fa = 0;
            if (run_variants(m1, kfs, S, kMapPoints, again, &ma, &fa)) return 1;
            if (again != fresh || ma != matched || fa != fused) { printf("FAILED: repetition %d after the larger call differs from the fresh contexts\n", rep); return 1; }
        }
        // a refused call leaves the transfer numbers of the call before, and an empty call is fine
        int64_t t0[6], t1[6];
        orbx_matcher_debug_transfers(m1, t0, 6);
        orbx_keyframe *mixed[kK] = {kfs[0], nullptr};
        std::vector<int32_t> r0(1000, kSentinel), r1(1000, kSentinel), nm(kK, kSentinel), bi(2 * kMapPoints, kSentinel), bd(2 * kMapPoints, kSentinel);
        int32_t *rows[kK] = {r0.data(), r1.data()};
        const int bad = orbx_keyframe_search_by_projection_sim3_fisheye(m1, kK, mixed, S.views[0], 8.f, 1.5f, 0.18f, 0, kMapPoints, S.pos.data(),
                                                                        S.normal.data(), S.min_dist.data(), S.max_dist.data(), S.mp_desc.data(), nullptr,
                                                                        nullptr, rows, nm.data(), nullptr, nullptr, nullptr);
        const int form = orbx_keyframe_search_by_projection_sim3_fisheye(m1, kK, kfs, S.views[0], 8.f, 1.5f, 0.18f, 2, kMapPoints, S.pos.data(),
                                                                         S.normal.data(), S.min_dist.data(), S.max_dist.data(), S.mp_desc.data(), nullptr,
                                                                         nullptr, rows, nm.data(), nullptr, nullptr, nullptr);
        const int fbad = orbx_keyframe_fuse_map_points_sim3_fisheye(m1, kK, mixed, S.views[0], 3.f, 0.18f, kMapPoints, S.pos.data(), S.normal.data(),
                                                                    S.min_dist.data(), S.max_dist.data(), S.mp_desc.data(), nullptr, bi.data(), bd.data(),
                                                                    nullptr);
        MUST(orbx_keyframe_search_by_projection_sim3_fisheye(m1, kK, kfs, S.views[0], 8.f, 1.5f, 0.18f, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                             nullptr, nullptr, rows, nm.data(), nullptr, nullptr, nullptr));
        MUST(orbx_keyframe_fuse_map_points_sim3_fisheye(m1, kK, kfs, S.views[0], 3.f, 0.18f, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                        nullptr, nullptr, nullptr));
        orbx_matcher_debug_transfers(m1, t1, 6);
        const size_t n0 = S.left[0].size() + S.right[0].size();
        if (bad != ORBX_E_BAD_ARG || form != ORBX_E_BAD_ARG || fbad != ORBX_E_BAD_ARG || memcmp(t0, t1, sizeof(t0)) || nm[0] != 0 || nm[1] != 0 ||
            r0[0] != -1 || r0[n0 - 1] != -1 || r0[n0] != kSentinel || bi[0] != kSentinel) {
            printf("FAILED: refusals %d %d %d, nmatches %d %d\n", bad, form, fbad, nm[0], nm[1]);
            return 1;
        }
        for (int k = 0; k < kK; k++) { orbx_keyframe_destroy(kfs[k]); orbx_keyframe_destroy(big[k]); }
        orbx_matcher_destroy(m1);
    }
    printf("%zu result arrays, %d matches, %d fuse candidates within TH_LOW\n", fresh.size(), matched, fused);
    if (matched < 150 || fused < 100) { printf("FAILED: the scene matches too little to show anything\n"); return 1; }
    printf("keyframe sim3 fisheye ok\n");
    return 0;
}
