// BoW on resident FISHEYE-STEREO key frames (orbx_keyframe_compute_bow_fisheye, orbx_keyframe_bow_from_frame_fisheye,
// orbx_frame_search_by_bow_resident_fisheye, orbx_keyframe_search_by_bow_fisheye, orbx_keyframe_search_for_triangulation_fisheye).  The key frame of
// one 320 x 240 rig frame is made four ways: from host arrays (BoW computed on it), from a host-loaded handle (BoW copied from the handle), and twice
// from a batch-loaded handle whose capacity lies above N -- both counts still on the device ("pending") and a gap of rows between the left camera's
// features and the right camera's -- once with BoW computed on the key frame, once copied from the handle.  Per call a FRESH set of the four is made,
// so every call meets the pending ones pending.  All four must return the same value and the same results, end with the extractor's counts, and
// nothing may be written beyond the rows in use (every caller array is a heap block of exactly the needed size, filled with a sentinel).  Per call
// the return value, the counts and a checksum of every result array are printed: the same text for any two builds of the library that behave alike.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt) and
// compiled with -fsanitize=address,undefined, as tests/cpp/keyframe_paths_check.cpp.  Prints "keyframe bow fisheye ok" and returns 0.
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kW = 320, kH = 240, kFrames = 2, kLevels = 8, kSentinel = -7, kLevelsUp = 1;

#define MUST(expr)                                                                   \
    do {                                                                             \
        const int r_ = (expr);                                                       \
        if (r_ < 0) { printf("%s: %d\n", #expr, r_); return 1; }                     \
    } while (0)

// kFrames views (shifted by `dx` + 3 per frame) of one canvas of random rectangles: corners for FAST
std::vector<uint8_t> make_images(int dx) {
    const int cw = kW + 32, ch = kH + 16;
    std::mt19937 rng(5);
    std::vector<int> canvas((size_t)cw * ch, 110);
    for (int k = 0; k < 260; k++) {
        const int x0 = (int)(rng() % cw), y0 = (int)(rng() % ch), w = 6 + (int)(rng() % 40), h = 6 + (int)(rng() % 40), d = (int)(rng() % 120) - 60;
        for (int y = y0; y < std::min(ch, y0 + h); y++)
            for (int x = x0; x < std::min(cw, x0 + w); x++) canvas[(size_t)y * cw + x] += d;
    }
    std::vector<uint8_t> img((size_t)kFrames * kW * kH);
    for (int f = 0; f < kFrames; f++)
        for (int y = 0; y < kH; y++)
            for (int x = 0; x < kW; x++) img[((size_t)f * kH + y) * kW + x] = (uint8_t)std::min(255, std::max(0, canvas[(size_t)(y + 2 * f) * cw + x + dx + 3 * f]));
    return img;
}

int make_extractor(const std::vector<uint8_t> &img, orbx_extractor **ex) {
    const orbx_params prm = {500, 1.2f, kLevels, 20, 7, 0};
    MUST(orbx_create(&prm, 0, kW, kH, kFrames, ex));
    MUST(orbx_extract_batch_host(*ex, img.data(), kFrames, kW, kH, kW, (size_t)kW * kH, 0, 0));
    return 0;
}

struct Features {
    std::vector<orbx_keypoint> kps;
    std::vector<uint8_t> desc;
    int n = 0;
};
int download(orbx_extractor *ex, int frame, int cap, Features &F) {
    F.kps.resize(cap); F.desc.resize(32 * (size_t)cap);
    int mono = 0;
    MUST(orbx_batch_download(ex, frame, F.kps.data(), F.desc.data(), cap, &F.n, &mono));
    F.kps.resize(F.n); F.desc.resize(32 * (size_t)F.n);
    return 0;
}

// a vocabulary of branching 4 and depth 2 whose 20 node descriptors are descriptors of the scene: node 0 the root, 1 .. 4 its children, 5 .. 20 the words
int make_vocabulary(const std::vector<uint8_t> &pool, orbx_vocabulary **voc) {
    std::mt19937 rng(9);
    std::vector<int32_t> cp(22), ci, wid(21, -1);
    for (int i = 0; i < 21; i++) {
        cp[i] = (int32_t)ci.size();
        if (i < 5) for (int c = 0; c < 4; c++) ci.push_back(1 + 4 * i + c);
        else wid[i] = i - 5;
    }
    cp[21] = (int32_t)ci.size();
    std::vector<uint8_t> nd(21 * 32);
    for (int i = 0; i < 21; i++) memcpy(nd.data() + 32 * i, pool.data() + 32 * (size_t)(rng() % (pool.size() / 32)), 32);
    MUST(orbx_vocabulary_create(0, 2, 21, cp.data(), ci.data(), nd.data(), wid.data(), voc));
    return 0;
}

// What a call wrote: heap blocks of exactly the size the call may write; `used` < 0: the whole array is result, else only its first `used` entries
// are and the rest must still hold the sentinel.
struct Result {
    int ret = 0, used = -1;
    std::vector<std::vector<int32_t>> a;
};
// (key frame, the rows its arrays are sized by, result)
typedef std::function<void(orbx_keyframe *, int, Result &)> Call;

struct Scene {
    int n, n_left, n_right, cap;   // the frame's counts as the extractor reported them; the batch-loaded handle's capacity
    std::function<int(int, orbx_keyframe **)> make;   // way 0 .. 3 -> a fresh key frame with BoW
};

int check(const char *name, const Scene &S, const Call &call) {
    printf("%s\n", name);
    static const char *who[4] = {"host arrays", "host-loaded handle", "pending, BoW computed", "pending, BoW copied"};
    int bad = 0;
    Result R[4];
    for (int v = 0; v < 4; v++) {
        orbx_keyframe *kf = nullptr;
        MUST(S.make(v, &kf));
        call(kf, v < 2 ? S.n : S.cap, R[v]);
        int c[3] = {-2, -2, -2};
        MUST(orbx_keyframe_count(kf, &c[0])); MUST(orbx_keyframe_counts(kf, &c[1], &c[2]));
        printf("  %-22s returned %d, counts %d (%d, %d), checksums", who[v], R[v].ret, c[0], c[1], c[2]);
        for (const std::vector<int32_t> &a : R[v].a) {
            const size_t used = R[v].used < 0 ? a.size() : (size_t)R[v].used;
            long long sum = 0;
            for (size_t i = 0; i < a.size(); i++) {
                if (i < used) sum = (sum * 31 + a[i] + 2) % 1000000007LL;
                if (i < used ? a[i] == kSentinel : a[i] != kSentinel) { printf(" [entry %zu of %zu, %zu in use: %d]", i, a.size(), used, a[i]); bad++; break; }
            }
            printf(" %lld", sum);
        }
        printf("\n");
        if (c[0] != S.n || c[1] != S.n_left || c[2] != S.n_right) { printf("  %s: counts %d (%d, %d), the extractor's %d (%d, %d)\n", who[v], c[0], c[1], c[2], S.n, S.n_left, S.n_right); bad++; }
        orbx_keyframe_destroy(kf);
        if (R[v].ret < 0 || R[v].ret != R[0].ret || R[v].a.size() != R[0].a.size()) { printf("  %s: returned %d, %zu arrays\n", who[v], R[v].ret, R[v].a.size()); bad++; continue; }
        for (size_t k = 0; k < R[v].a.size(); k++) {
            const size_t used = R[0].used < 0 ? R[0].a[k].size() : (size_t)R[0].used;
            if (R[v].a[k].size() < used || (R[v].used < 0 && R[v].a[k].size() != used) || (used && memcmp(R[v].a[k].data(), R[0].a[k].data(), 4 * used))) {
                printf("  %s: array %zu differs from the one of the key frame made from host arrays\n", who[v], k);
                bad++;
            }
        }
    }
    if (bad) printf("  FAILED\n");
    return bad;
}

}  // namespace

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const std::vector<uint8_t> img_l = make_images(4), img_r = make_images(1);
    orbx_extractor *exl = nullptr, *exr = nullptr;
    if (make_extractor(img_l, &exl) || make_extractor(img_r, &exr)) return 1;
    const float tumvi[8] = {190.978477f, 190.973307f, 254.931706f, 256.897442f, 0.0034823894f, 0.0007150348f, -0.0020532361f, 0.0002029367f};
    orbx_kb8_rig rig;
    memcpy(rig.cam_left, tumvi, sizeof(tumvi)); memcpy(rig.cam_right, tumvi, sizeof(tumvi));
    const float eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, base[3] = {0.1f, 0.f, 0.f};
    memcpy(rig.R_lr, eye, sizeof(eye)); memcpy(rig.t_lr, base, sizeof(base));
    MUST(orbx_stereo_fisheye_batch_device(exl, exr, &rig));
    orbx_batch_view view_l, view_r;
    MUST(orbx_batch_view_get(exl, &view_l)); MUST(orbx_batch_view_get(exr, &view_r));
    float scale[kLevels], inv_scale[kLevels], sigma2[kLevels], inv_sigma2[kLevels];
    MUST(orbx_get_scale_tables(exl, scale, inv_scale, sigma2, inv_sigma2));
    Features FL[2], FR[2];
    for (int f = 0; f < 2; f++)
        if (download(exl, f, view_l.cap, FL[f]) || download(exr, f, view_r.cap, FR[f])) return 1;
    printf("frame 0: %d + %d features, frame 1: %d + %d features, capacities %d + %d\n", FL[0].n, FR[0].n, FL[1].n, FR[1].n, view_l.cap, view_r.cap);
    if (FL[0].n < 50 || FR[0].n < 50 || FL[1].n < 50 || FR[1].n < 50 || view_l.cap <= FL[0].n) { printf("the scene is too poor\n"); return 1; }

    orbx_matcher *m = nullptr;
    MUST(orbx_matcher_create(0, &m));
    std::vector<uint8_t> rows2[2];   // mDescriptors of the rig: the left camera's rows, then the right camera's
    orbx_frame_desc dl[2];
    for (int f = 0; f < 2; f++) {
        rows2[f] = FL[f].desc;
        rows2[f].insert(rows2[f].end(), FR[f].desc.begin(), FR[f].desc.end());
        memset(&dl[f], 0, sizeof(dl[f]));
        dl[f].keypoints_un = FL[f].kps.data(); dl[f].descriptors = rows2[f].data(); dl[f].n = FL[f].n; dl[f].max_x = (float)kW; dl[f].max_y = (float)kH;
        dl[f].scale_factors = scale; dl[f].nlevels = kLevels;
    }
    orbx_vocabulary *voc = nullptr;
    if (make_vocabulary(rows2[0], &voc)) return 1;
    const float bounds[4] = {0.f, (float)kW, 0.f, (float)kH};
    const int N0 = FL[0].n + FR[0].n, N1 = FL[1].n + FR[1].n, cap_rig = view_l.cap + view_r.cap + 37;
    const std::vector<int32_t> no_partner((size_t)std::max(std::max(FL[0].n, FR[0].n), std::max(FL[1].n, FR[1].n)), -1);

    // the handles: frame 0 loaded from host arrays and from the batch (never counted), frame 1 (the current frame of the frame form) from the batch too
    orbx_frame *fh = nullptr, *fb = nullptr, *cur = nullptr;
    MUST(orbx_frame_create(m, cap_rig, &fh)); MUST(orbx_frame_create(m, cap_rig, &fb)); MUST(orbx_frame_create(m, cap_rig, &cur));
    MUST(orbx_frame_load_host_fisheye(fh, &dl[0], FR[0].kps.data(), FR[0].n, no_partner.data(), no_partner.data()));
    MUST(orbx_frame_compute_bow_fisheye(m, fh, voc, kLevelsUp, nullptr, nullptr));
    MUST(orbx_frame_load_stereo_fisheye_batch(fb, exl, exr, 0, bounds, nullptr, 0));
    MUST(orbx_frame_compute_bow_fisheye(m, fb, voc, kLevelsUp, nullptr, nullptr));
    MUST(orbx_frame_load_stereo_fisheye_batch(cur, exl, exr, 1, bounds, nullptr, 0));
    MUST(orbx_frame_compute_bow_fisheye(m, cur, voc, kLevelsUp, nullptr, nullptr));
    orbx_keyframe *other = nullptr;   // frame 1 as a key frame, from host arrays
    MUST(orbx_keyframe_create_host_fisheye(m, &dl[1], FR[1].kps.data(), FR[1].n, inv_sigma2, &other));
    MUST(orbx_keyframe_compute_bow_fisheye(m, other, voc, kLevelsUp, nullptr, nullptr));

    Scene S;
    S.n = N0; S.n_left = FL[0].n; S.n_right = FR[0].n; S.cap = cap_rig;
    S.make = [&](int way, orbx_keyframe **out) {
        if (way == 0) MUST(orbx_keyframe_create_host_fisheye(m, &dl[0], FR[0].kps.data(), FR[0].n, inv_sigma2, out));
        else MUST(orbx_keyframe_from_frame_fisheye(m, way == 1 ? fh : fb, inv_sigma2, out));
        if (way == 0 || way == 2) MUST(orbx_keyframe_compute_bow_fisheye(m, *out, voc, kLevelsUp, nullptr, nullptr));
        else MUST(orbx_keyframe_bow_from_frame_fisheye(m, *out, way == 1 ? fh : fb));
        return 0;
    };
    std::vector<uint8_t> flags0((size_t)N0), flags1((size_t)N1);
    { std::mt19937 rng(21); for (uint8_t &s : flags0) s = rng() % 5 != 0; for (uint8_t &s : flags1) s = rng() % 5 != 0; }
    std::vector<uint8_t> skip0(flags0), skip1(flags1);
    for (uint8_t &s : skip0) s = !s;
    for (uint8_t &s : skip1) s = !s;
    orbx_keyframe_kb8_gate gate;
    memset(&gate, 0, sizeof(gate));
    gate.level_sigma2_1 = sigma2; gate.level_sigma2_2 = sigma2; gate.nlevels = kLevels;
    for (int c = 0; c < 2; c++) { memcpy(gate.cam1[c], tumvi, sizeof(tumvi)); memcpy(gate.cam2[c], tumvi, sizeof(tumvi)); }
    const float tt[4][3] = {{0.02f, 0.005f, 0.f}, {0.12f, 0.005f, 0.f}, {-0.08f, 0.005f, 0.f}, {0.02f, 0.005f, 0.f}};
    for (int p = 0; p < 4; p++) { memcpy(gate.R12[p], eye, sizeof(eye)); memcpy(gate.t12[p], tt[p], sizeof(tt[p])); }
    int bad = 0, total = 0;

    // ---- orbx_keyframe_compute_bow_fisheye: the ids (a second call on a key frame that has BoW returns what was kept), both buffers or one
    bad += check("orbx_keyframe_compute_bow_fisheye, word and node ids", S, [&](orbx_keyframe *kf, int rows, Result &R) {
        R.a.assign(2, std::vector<int32_t>((size_t)rows, kSentinel));
        R.used = N0;
        R.ret = orbx_keyframe_compute_bow_fisheye(m, kf, voc, kLevelsUp, R.a[0].data(), R.a[1].data());
    });
    bad += check("orbx_keyframe_compute_bow_fisheye, node ids only", S, [&](orbx_keyframe *kf, int rows, Result &R) {
        R.a.assign(1, std::vector<int32_t>((size_t)rows, kSentinel));
        R.used = N0;
        R.ret = orbx_keyframe_compute_bow_fisheye(m, kf, voc, kLevelsUp, nullptr, R.a[0].data());
    });

    // ---- orbx_frame_search_by_bow_resident_fisheye: the batch-loaded frame 1 against {the key frame, frame 1's own key frame}, rows of the handle's capacity
    bad += check("orbx_frame_search_by_bow_resident_fisheye, K = 2", S, [&](orbx_keyframe *kf, int, Result &R) {
        orbx_keyframe *kfs[2] = {kf, other};
        const uint8_t *valid[2] = {nullptr, flags1.data()};
        R.a.assign(3, std::vector<int32_t>());
        R.a[0].assign((size_t)cap_rig, kSentinel); R.a[1].assign((size_t)cap_rig, kSentinel); R.a[2].assign(2, kSentinel);
        std::vector<int32_t> rows(2 * (size_t)cap_rig, kSentinel);
        R.ret = orbx_frame_search_by_bow_resident_fisheye(m, cur, 2, kfs, valid, 0.75f, 1, rows.data(), cap_rig, R.a[2].data());
        for (int k = 0; k < 2; k++) {
            memcpy(R.a[k].data(), rows.data() + (size_t)k * cap_rig, 4 * (size_t)cap_rig);
            for (int i = N1; i < cap_rig; i++) if (R.a[k][i] != kSentinel) R.ret = -100;   // untouched beyond N of the frame
            R.a[k].resize((size_t)N1);
        }
        if (R.ret >= 0) total += R.a[2][0] + R.a[2][1];
    });
    // ---- orbx_keyframe_search_by_bow_fisheye: the key frame as kf1 (a row of its capacity), and among kfs2 with flags of the other side
    bad += check("orbx_keyframe_search_by_bow_fisheye, the key frame first", S, [&](orbx_keyframe *kf, int rows, Result &R) {
        R.a.assign(1, std::vector<int32_t>((size_t)rows, kSentinel));
        R.used = N0;
        int32_t nm = 0;
        R.ret = orbx_keyframe_search_by_bow_fisheye(m, kf, nullptr, 1, &other, nullptr, 0.75f, 1, R.a[0].data(), rows, &nm);
        if (R.ret >= 0) { R.ret = nm; total += nm; }
    });
    bad += check("orbx_keyframe_search_by_bow_fisheye, the key frame among kfs2", S, [&](orbx_keyframe *kf, int, Result &R) {
        orbx_keyframe *kfs[2] = {kf, other};
        R.a.assign(2, std::vector<int32_t>());
        R.a[0].assign(2 * (size_t)N1, kSentinel); R.a[1].assign(2, kSentinel);
        R.ret = orbx_keyframe_search_by_bow_fisheye(m, other, flags1.data(), 2, kfs, nullptr, 0.9f, 0, R.a[0].data(), N1, R.a[1].data());
        if (R.ret >= 0) total += R.a[1][0];
    });
    // ---- orbx_keyframe_search_for_triangulation_fisheye: gated and coarse, the key frame as kf1 (N1 is counted by the call) and as kf2 without flags
    for (int coarse = 0; coarse < 2; coarse++) {
        gate.coarse = coarse;
        char name[128];
        snprintf(name, sizeof(name), "orbx_keyframe_search_for_triangulation_fisheye%s, the key frame first", coarse ? ", coarse" : "");
        bad += check(name, S, [&](orbx_keyframe *kf, int, Result &R) {
            R.a.assign(1, std::vector<int32_t>((size_t)N0, kSentinel));
            R.ret = orbx_keyframe_search_for_triangulation_fisheye(m, kf, other, skip0.data(), skip1.data(), 1, &gate, R.a[0].data());
            if (R.ret >= 0) total += R.ret;
        });
        snprintf(name, sizeof(name), "orbx_keyframe_search_for_triangulation_fisheye%s, the key frame second", coarse ? ", coarse" : "");
        bad += check(name, S, [&](orbx_keyframe *kf, int, Result &R) {
            R.a.assign(1, std::vector<int32_t>((size_t)N1, kSentinel));
            R.ret = orbx_keyframe_search_for_triangulation_fisheye(m, other, kf, skip1.data(), nullptr, 0, &gate, R.a[0].data());
            if (R.ret >= 0) total += R.ret;
        });
    }
    int cl = -1, cr = -1;
    MUST(orbx_frame_counts(cur, &cl, &cr));
    if (cl != FL[1].n || cr != FR[1].n) { printf("the current frame ends with counts (%d, %d), the extractor's (%d, %d) FAILED\n", cl, cr, FL[1].n, FR[1].n); bad++; }
    printf("matches over all calls: %d\n", total);
    if (total < 200) { printf("too few matches for the comparison to mean anything FAILED\n"); bad++; }

    orbx_keyframe_destroy(other);
    for (orbx_frame *f : {fh, fb, cur}) orbx_frame_destroy(f);
    orbx_vocabulary_destroy(voc);
    orbx_matcher_destroy(m);
    orbx_destroy(exl); orbx_destroy(exr);
    if (bad) { printf("keyframe bow fisheye FAILED: %d\n", bad); return 1; }
    printf("keyframe bow fisheye ok\n");
    return 0;
}
