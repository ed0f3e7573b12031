// Resident key frames (orbx_keyframe) of both kinds -- monocular and fisheye-stereo -- are made three ways: from host arrays, from a frame handle
// loaded from host arrays, and from a frame handle loaded from an extractor's batch, whose capacity lies above N and whose count is still on the
// device ("pending").  Per entry point that takes a key frame, four key frames of the SAME frame are searched: the two host-made ones, a pending one
// that orbx_keyframe_counts counted first, and a pending one that is handed over as it is.  All four must return the same value and the same
// results, the pending one must end with the counted one's counts, and nothing may be written beyond the rows in use (every caller array is a heap
// block of exactly the needed size, filled with a sentinel).  Each entry point must refuse the other kind's key frame with ORBX_E_BAD_ARG before it
// enqueues anything (the numbers of orbx_matcher_debug_transfers stay those of the call before).  Per call the return value, the counts, a checksum
// of every result array and the six transfer numbers are printed: the output is the same text for any two builds of the library that behave alike.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt) and
// compiled with -fsanitize=address,undefined, as tests/cpp/frame_pending_count_check.cpp.  Prints "keyframe paths ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kW = 320, kH = 240, kFrames = 2, kLevels = 8, kSentinel = -7, kMapPoints = 300, kLevelsUp = 1;
constexpr float kDepth = 5.f;

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

// nq queries that look at the features of F (a jittered copy of feature j % N each, a few descriptor bits flipped), once as the projected records
// orbx_keyframe_fuse_search takes and once as map points: the back-projection of feature j % N at depth kDepth under an identity pose, through a
// pinhole camera without distortion (fx = fy = 200) or a KannalaBrandt8 camera with k1 .. k4 = 0 (fx = fy = 100)
struct Queries {
    std::vector<float> u, v, r, pos, normal, min_dist, max_dist;
    std::vector<int32_t> level;
    std::vector<uint8_t> desc;
    orbx_fuse_queries set(int n) const { return orbx_fuse_queries{n, u.data(), v.data(), nullptr, r.data(), level.data(), desc.data()}; }
};
Queries make_queries(const Features &F, const float *scale, int nq, uint32_t seed, bool kb8) {
    std::mt19937 rng(seed);
    auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    Queries Q;
    for (int j = 0; j < nq; j++) {
        const int i = j % F.n;
        const orbx_keypoint k = F.kps[i];
        Q.u.push_back(k.x + uni(-2.f, 2.f)); Q.v.push_back(k.y + uni(-2.f, 2.f));
        Q.level.push_back(std::min(k.octave + (int)(rng() % 2), kLevels - 1));   // Fuse takes octaves in [level - 1, level]
        Q.r.push_back(3.f * scale[Q.level[j]]);
        for (int b = 0; b < 32; b++) Q.desc.push_back(F.desc[32 * (size_t)i + b]);
        for (int f = 0; f < 10; f++) { const unsigned b = rng() % 256; Q.desc[32 * (size_t)j + b / 8] ^= (uint8_t)(1u << (b % 8)); }
        float ray[3];
        if (kb8) {
            const float ax = (k.x - 160.f) / 100.f, ay = (k.y - 120.f) / 100.f, theta = std::sqrt(ax * ax + ay * ay), s = theta > 1e-6f ? std::sin(theta) / theta : 1.f;
            ray[0] = s * ax; ray[1] = s * ay; ray[2] = std::cos(theta);
        } else {
            const float px = (k.x - 160.f) / 200.f, py = (k.y - 120.f) / 200.f, pn = std::sqrt(px * px + py * py + 1.f);
            ray[0] = px / pn; ray[1] = py / pn; ray[2] = 1.f / pn;
        }
        const float d = kb8 ? kDepth : kDepth / ray[2];   // pinhole: depth z = kDepth
        for (int c = 0; c < 3; c++) { Q.pos.push_back(d * ray[c]); Q.normal.push_back(ray[c]); }   // (seen head-on)
        Q.max_dist.push_back(d * scale[k.octave] * 1.05f); Q.min_dist.push_back(0.2f * d);
    }
    return Q;
}

// a vocabulary of branching 4 and depth 2: node 0 the root, nodes 1 .. 4 its children, nodes 5 .. 20 the 16 words
int make_vocabulary(orbx_vocabulary **voc) {
    std::mt19937 rng(9);
    std::vector<int32_t> cp(22), ci, wid(21, -1);
    for (int i = 0; i < 21; i++) {
        cp[i] = (int32_t)ci.size();
        if (i < 5) for (int c = 0; c < 4; c++) ci.push_back(1 + 4 * i + c);
        else wid[i] = i - 5;
    }
    cp[21] = (int32_t)ci.size();
    std::vector<uint8_t> nd(21 * 32);
    for (uint8_t &b : nd) b = (uint8_t)rng();
    MUST(orbx_vocabulary_create(0, 2, 21, cp.data(), ci.data(), nd.data(), wid.data(), voc));
    return 0;
}

// What a call wrote.  Every array is a heap block of exactly the size the call may write (int32 rows; byte rows are widened after the call);
// `used` < 0: the whole array is result, else only its first `used` entries are and the rest must still hold the sentinel.
struct Result {
    int ret = 0, used = -1;
    std::vector<std::vector<int32_t>> a;
};
// (key frame, the rows its arrays are sized by, result)
typedef std::function<void(orbx_keyframe *, int, Result &)> Call;

void transfers(const orbx_matcher *m, int64_t *t) {
    for (int i = 0; i < 6; i++) t[i] = 0;
    orbx_matcher_debug_transfers(m, t, 6);
}

// One kind of key frame: the two host-made key frames of the frame, and how to make one more from the batch-loaded handle (count pending)
struct Kind {
    const char *name;
    orbx_matcher *m;
    bool fisheye;
    int n, n_left, n_right, cap;   // the frame's counts as the extractor reported them; the batch-loaded handle's capacity
    orbx_keyframe *host, *handle;
    std::function<int(orbx_keyframe **)> from_batch;
};

int check(const char *name, const Kind &K, const Call &call) {
    printf("%s, %s\n", name, K.name);
    static const char *who[4] = {"host arrays", "host-loaded handle", "counted first", "count pending"};
    orbx_keyframe *kf[4] = {K.host, K.handle, nullptr, nullptr};
    MUST(K.from_batch(&kf[2])); MUST(K.from_batch(&kf[3]));
    int counted[3] = {-2, -2, -2};
    MUST(orbx_keyframe_count(kf[2], &counted[0])); MUST(orbx_keyframe_counts(kf[2], &counted[1], &counted[2]));
    int bad = 0;
    Result R[4];
    for (int v = 0; v < 4; v++) {
        call(kf[v], v < 2 ? K.n : K.cap, R[v]);
        int64_t t[6];
        transfers(K.m, t);
        int c[3] = {-2, -2, -2};
        MUST(orbx_keyframe_count(kf[v], &c[0])); MUST(orbx_keyframe_counts(kf[v], &c[1], &c[2]));
        printf("  %-18s returned %d, counts %d (%d, %d), checksums", who[v], R[v].ret, c[0], c[1], c[2]);
        for (const std::vector<int32_t> &a : R[v].a) {
            const size_t used = R[v].used < 0 ? a.size() : (size_t)R[v].used;
            long long sum = 0;
            for (size_t i = 0; i < a.size(); i++) {
                if (i < used) sum = (sum * 31 + a[i] + 2) % 1000000007LL;
                if (i < used ? a[i] == kSentinel : a[i] != kSentinel) { printf(" [entry %zu of %zu, %zu in use: %d]", i, a.size(), used, a[i]); bad++; break; }
            }
            printf(" %lld", sum);
        }
        printf(", transfers %lld %lld %lld %lld %lld %lld\n", (long long)t[0], (long long)t[1], (long long)t[2], (long long)t[3], (long long)t[4], (long long)t[5]);
        if (c[0] != K.n || c[1] != (K.fisheye ? K.n_left : K.n) || c[2] != (K.fisheye ? K.n_right : -1) || memcmp(c, counted, sizeof(c))) {
            printf("  %s: counts %d (%d, %d), the extractor's %d (%d, %d), the counted copy's %d (%d, %d)\n", who[v], c[0], c[1], c[2], K.n, K.n_left, K.n_right,
                   counted[0], counted[1], counted[2]);
            bad++;
        }
        if (R[v].ret < 0 || R[v].ret != R[0].ret || R[v].a.size() != R[0].a.size()) { printf("  %s: returned %d, %zu arrays\n", who[v], R[v].ret, R[v].a.size()); bad++; continue; }
        for (size_t k = 0; k < R[v].a.size(); k++) {
            const size_t used = R[0].used < 0 ? R[0].a[k].size() : (size_t)R[0].used;
            if (R[v].a[k].size() < used || (R[v].used < 0 && R[v].a[k].size() != used) || (used && memcmp(R[v].a[k].data(), R[0].a[k].data(), 4 * used))) {
                printf("  %s: array %zu differs from the one of the key frame made from host arrays\n", who[v], k);
                bad++;
            }
        }
    }
    orbx_keyframe_destroy(kf[2]); orbx_keyframe_destroy(kf[3]);
    if (bad) printf("  FAILED\n");
    return bad;
}

// a call that must be refused before anything is enqueued: the context's transfer numbers are still those of the call before
int refused(const char *name, const orbx_matcher *m, const std::function<int()> &call) {
    int64_t before[6], after[6];
    transfers(m, before);
    const int r = call();
    transfers(m, after);
    const bool ok = r == ORBX_E_BAD_ARG && !memcmp(before, after, sizeof(before)) && before[0] + before[1] > 0;
    printf("  %s: returned %d, transfers %lld %lld %lld %lld %lld %lld%s\n", name, r, (long long)after[0], (long long)after[1], (long long)after[2],
           (long long)after[3], (long long)after[4], (long long)after[5], ok ? "" : " FAILED");
    return ok ? 0 : 1;
}

std::vector<int32_t> widen(const std::vector<uint8_t> &b) { return std::vector<int32_t>(b.begin(), b.end()); }

}  // namespace

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const std::vector<uint8_t> img = make_images(0), img_l = make_images(4), img_r = make_images(1);
    orbx_extractor *ex = nullptr, *exl = nullptr, *exr = nullptr;
    if (make_extractor(img, &ex) || make_extractor(img_l, &exl) || make_extractor(img_r, &exr)) return 1;
    const float tumvi[8] = {190.978477f, 190.973307f, 254.931706f, 256.897442f, 0.0034823894f, 0.0007150348f, -0.0020532361f, 0.0002029367f};
    orbx_kb8_rig rig;
    memcpy(rig.cam_left, tumvi, sizeof(tumvi)); memcpy(rig.cam_right, tumvi, sizeof(tumvi));
    const float eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, base[3] = {0.1f, 0.f, 0.f};
    memcpy(rig.R_lr, eye, sizeof(eye)); memcpy(rig.t_lr, base, sizeof(base));
    MUST(orbx_stereo_fisheye_batch_device(exl, exr, &rig));
    orbx_batch_view view, view_l, view_r;
    MUST(orbx_batch_view_get(ex, &view)); MUST(orbx_batch_view_get(exl, &view_l)); MUST(orbx_batch_view_get(exr, &view_r));
    float scale[kLevels], inv_scale[kLevels], sigma2[kLevels], inv_sigma2[kLevels];
    MUST(orbx_get_scale_tables(ex, scale, inv_scale, sigma2, inv_sigma2));
    Features F[2], FL[2], FR[2];
    for (int f = 0; f < 2; f++)
        if (download(ex, f, view.cap, F[f]) || download(exl, f, view_l.cap, FL[f]) || download(exr, f, view_r.cap, FR[f])) return 1;
    printf("pinhole frame 0: %d features, fisheye frame 0: %d + %d features\n", F[0].n, FL[0].n, FR[0].n);
    if (F[0].n < 50 || FL[0].n < 50 || FR[0].n < 50) { printf("the scene is too poor\n"); return 1; }

    orbx_matcher *m = nullptr;
    MUST(orbx_matcher_create(0, &m));
    orbx_vocabulary *voc = nullptr;
    if (make_vocabulary(&voc)) return 1;
    const float bounds[4] = {0.f, (float)kW, 0.f, (float)kH};
    auto desc_of = [&](const Features &f, const uint8_t *rows) {
        orbx_frame_desc d;
        memset(&d, 0, sizeof(d));
        d.keypoints_un = f.kps.data(); d.descriptors = rows; d.n = f.n; d.max_x = (float)kW; d.max_y = (float)kH; d.scale_factors = scale; d.nlevels = kLevels;
        return d;
    };

    // ---- the key frames.  Frame 0 three ways per kind; frame 1 from host arrays as the second key frame of the K = 2 calls
    orbx_frame_desc d[2] = {desc_of(F[0], F[0].desc.data()), desc_of(F[1], F[1].desc.data())};
    orbx_keyframe *mono_host = nullptr, *mono_handle = nullptr, *mono_other = nullptr;
    orbx_frame *fh_mono = nullptr, *fb_mono = nullptr;
    const int cap_mono = view.cap + 37;
    MUST(orbx_keyframe_create_host(m, &d[0], inv_sigma2, &mono_host));
    MUST(orbx_keyframe_create_host(m, &d[1], inv_sigma2, &mono_other));
    MUST(orbx_frame_create(m, cap_mono, &fh_mono)); MUST(orbx_frame_create(m, cap_mono, &fb_mono));
    MUST(orbx_frame_load_host(fh_mono, &d[0]));
    MUST(orbx_keyframe_from_frame(m, fh_mono, inv_sigma2, &mono_handle));
    MUST(orbx_frame_load_batch(fb_mono, ex, 0, bounds, nullptr, 0));   // never counted: every key frame made from it starts with its count pending
    const Kind M = {"monocular", m, false, F[0].n, F[0].n, -1, cap_mono, mono_host, mono_handle,
                    [&](orbx_keyframe **out) { return orbx_keyframe_from_frame(m, fb_mono, inv_sigma2, out); }};

    std::vector<uint8_t> rows2[2];   // mDescriptors of the rig: the left camera's rows, then the right camera's
    orbx_frame_desc dl[2];
    for (int f = 0; f < 2; f++) {
        rows2[f] = FL[f].desc;
        rows2[f].insert(rows2[f].end(), FR[f].desc.begin(), FR[f].desc.end());
        dl[f] = desc_of(FL[f], rows2[f].data());
    }
    orbx_keyframe *rig_host = nullptr, *rig_handle = nullptr, *rig_other = nullptr;
    orbx_frame *fh_rig = nullptr, *fb_rig = nullptr;
    const int cap_rig = view_l.cap + view_r.cap + 37;
    MUST(orbx_keyframe_create_host_fisheye(m, &dl[0], FR[0].kps.data(), FR[0].n, inv_sigma2, &rig_host));
    MUST(orbx_keyframe_create_host_fisheye(m, &dl[1], FR[1].kps.data(), FR[1].n, inv_sigma2, &rig_other));
    MUST(orbx_frame_create(m, cap_rig, &fh_rig)); MUST(orbx_frame_create(m, cap_rig, &fb_rig));
    const std::vector<int32_t> no_partner((size_t)std::max(FL[0].n, FR[0].n), -1);   // (a key frame keeps neither mvLeftToRightMatch nor its inverse)
    MUST(orbx_frame_load_host_fisheye(fh_rig, &dl[0], FR[0].kps.data(), FR[0].n, no_partner.data(), no_partner.data()));
    MUST(orbx_keyframe_from_frame_fisheye(m, fh_rig, inv_sigma2, &rig_handle));
    MUST(orbx_frame_load_stereo_fisheye_batch(fb_rig, exl, exr, 0, bounds, nullptr, 0));
    const Kind S = {"fisheye", m, true, FL[0].n + FR[0].n, FL[0].n, FR[0].n, cap_rig, rig_host, rig_handle,
                    [&](orbx_keyframe **out) { return orbx_keyframe_from_frame_fisheye(m, fb_rig, inv_sigma2, out); }};

    const orbx_camera cam2[2] = {{200.f, 200.f, 160.f, 120.f, 0.f, 0.f, 0.f, 0.f, 0.f, 40.f}, {200.f, 200.f, 160.f, 120.f, 0.f, 0.f, 0.f, 0.f, 0.f, 40.f}};
    const orbx_frame_pose pose2[2] = {{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}, {0, 0, 0}}, {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}, {0, 0, 0}}};
    const orbx_fisheye_view left = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}, {0, 0, 0}, {100.f, 100.f, 160.f, 120.f, 0.f, 0.f, 0.f, 0.f}},
                            right = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {-0.02f, 0, 0}, {0.02f, 0, 0}, {100.f, 100.f, 160.f, 120.f, 0.f, 0.f, 0.f, 0.f}};
    const orbx_fisheye_view views4[4] = {left, right, left, right};
    const float log_sf = std::log(1.2f);
    // projected records: of the frame's own features (the rig: per camera) and of frame 1's; map points: of the frame's (left) features
    const Queries Q0 = make_queries(F[0], scale, 400, 11u, false), Q1 = make_queries(F[1], scale, 350, 12u, false);
    const Queries QL0 = make_queries(FL[0], scale, 400, 13u, true), QR0 = make_queries(FR[0], scale, 380, 14u, true), QL1 = make_queries(FL[1], scale, 390, 18u, true),
                  QR1 = make_queries(FR[1], scale, 350, 15u, true);
    const Queries P0 = make_queries(F[0], scale, kMapPoints, 16u, false), PL0 = make_queries(FL[0], scale, kMapPoints, 17u, true);
    std::vector<uint8_t> skip(2 * (size_t)kMapPoints);
    { std::mt19937 rng(21); for (uint8_t &s : skip) s = rng() % 4 == 0; }
    int bad = 0;

    // ---- orbx_keyframe_fuse_search[_fisheye]: K = 1; K = 2; K = 2 with one empty query set
    for (int form = 0; form < 3; form++) {
        const int K = form == 0 ? 1 : 2;
        char name[96];
        snprintf(name, sizeof(name), "orbx_keyframe_fuse_search, K = %d%s", K, form == 2 ? ", one query set empty" : "");
        bad += check(name, M, [&](orbx_keyframe *kf, int, Result &R) {
            orbx_keyframe *kfs[2] = {kf, mono_other};
            const orbx_fuse_queries q[2] = {Q0.set(400), Q1.set(form == 1 ? 350 : 0)};
            R.a.assign(4, std::vector<int32_t>());
            int32_t *bi[2], *bd[2];
            for (int p = 0; p < 2; p++) { R.a[p].assign((size_t)q[p].n, kSentinel); R.a[2 + p].assign((size_t)q[p].n, kSentinel); bi[p] = R.a[p].data(); bd[p] = R.a[2 + p].data(); }
            R.ret = orbx_keyframe_fuse_search(m, K, kfs, q, 1, 0, bi, bd);
        });
        snprintf(name, sizeof(name), "orbx_keyframe_fuse_search_fisheye, K = %d%s", K, form == 2 ? ", one query set empty" : "");
        bad += check(name, S, [&](orbx_keyframe *kf, int, Result &R) {
            orbx_keyframe *kfs[2] = {kf, rig_other};
            const orbx_fuse_queries q[4] = {QL0.set(400), QR0.set(380), QL1.set(form == 1 ? 390 : 0), QR1.set(K == 2 ? 350 : 0)};
            R.a.assign(8, std::vector<int32_t>());
            int32_t *bi[4], *bd[4];
            for (int p = 0; p < 4; p++) { R.a[p].assign((size_t)q[p].n, kSentinel); R.a[4 + p].assign((size_t)q[p].n, kSentinel); bi[p] = R.a[p].data(); bd[p] = R.a[4 + p].data(); }
            R.ret = orbx_keyframe_fuse_search_fisheye(m, K, kfs, q, 1, 0, bi, bd);
        });
    }

    // ---- orbx_keyframe_fuse_map_points[_fisheye]: K = 2, 300 map points, with and without `skip`, with and without `projected`
    for (int form = 0; form < 4; form++) {
        const bool with_skip = form & 1, with_proj = form & 2;
        char name[128];
        snprintf(name, sizeof(name), "orbx_keyframe_fuse_map_points, K = 2%s%s", with_skip ? ", skip" : "", with_proj ? ", projected" : "");
        bad += check(name, M, [&](orbx_keyframe *kf, int, Result &R) {
            orbx_keyframe *kfs[2] = {kf, mono_other};
            const size_t total = 2 * (size_t)kMapPoints;
            R.a.assign(2, std::vector<int32_t>(total, kSentinel));
            std::vector<uint8_t> proj(with_proj ? total : 0, 0xee);
            R.ret = orbx_keyframe_fuse_map_points(m, 2, kfs, cam2, pose2, 3.f, log_sf, 0, kMapPoints, P0.pos.data(), P0.normal.data(), P0.min_dist.data(),
                                                  P0.max_dist.data(), P0.desc.data(), with_skip ? skip.data() : nullptr, R.a[0].data(), R.a[1].data(),
                                                  with_proj ? proj.data() : nullptr);
            if (with_proj) R.a.push_back(widen(proj));
        });
        snprintf(name, sizeof(name), "orbx_keyframe_fuse_map_points_fisheye, K = 2%s%s", with_skip ? ", skip" : "", with_proj ? ", projected" : "");
        bad += check(name, S, [&](orbx_keyframe *kf, int, Result &R) {
            orbx_keyframe *kfs[2] = {kf, rig_other};
            const size_t total = 4 * (size_t)kMapPoints;
            R.a.assign(2, std::vector<int32_t>(total, kSentinel));
            std::vector<uint8_t> proj(with_proj ? total : 0, 0xee);
            R.ret = orbx_keyframe_fuse_map_points_fisheye(m, 2, kfs, views4, 3.f, log_sf, 0, kMapPoints, PL0.pos.data(), PL0.normal.data(), PL0.min_dist.data(),
                                                          PL0.max_dist.data(), PL0.desc.data(), with_skip ? skip.data() : nullptr, R.a[0].data(), R.a[1].data(),
                                                          with_proj ? proj.data() : nullptr);
            if (with_proj) R.a.push_back(widen(proj));
        });
    }

    // ---- orbx_keyframe_compute_bow on a monocular key frame: no id buffers; both id buffers as the first call; no id buffers, then the word ids
    bad += check("orbx_keyframe_compute_bow, no id buffers", M, [&](orbx_keyframe *kf, int, Result &R) {
        R.ret = orbx_keyframe_compute_bow(m, kf, voc, kLevelsUp, nullptr, nullptr);
    });
    bad += check("orbx_keyframe_compute_bow, word and node ids", M, [&](orbx_keyframe *kf, int rows, Result &R) {
        R.a.assign(2, std::vector<int32_t>((size_t)rows, kSentinel));
        R.used = M.n;
        R.ret = orbx_keyframe_compute_bow(m, kf, voc, kLevelsUp, R.a[0].data(), R.a[1].data());
    });
    bad += check("orbx_keyframe_compute_bow, no id buffers, then word ids", M, [&](orbx_keyframe *kf, int rows, Result &R) {
        R.a.assign(1, std::vector<int32_t>((size_t)rows, kSentinel));
        R.used = M.n;
        R.ret = orbx_keyframe_compute_bow(m, kf, voc, kLevelsUp, nullptr, nullptr);
        if (R.ret >= 0) R.ret = orbx_keyframe_compute_bow(m, kf, voc, kLevelsUp, R.a[0].data(), nullptr);
    });

    // ---- every entry point with the other kind's key frame or handle
    printf("the other kind's key frame\n");
    {
        const orbx_fuse_queries q[2] = {Q0.set(400), Q0.set(400)};
        std::vector<int32_t> bi(4 * (size_t)kMapPoints, kSentinel), bd(4 * (size_t)kMapPoints, kSentinel);
        int32_t *pi[2] = {bi.data(), bi.data() + 400}, *pd[2] = {bd.data(), bd.data() + 400};
        orbx_keyframe *out = nullptr;
        bad += refused("orbx_keyframe_fuse_search", m, [&] { return orbx_keyframe_fuse_search(m, 1, &rig_host, q, 1, 0, pi, pd); });
        bad += refused("orbx_keyframe_fuse_search_fisheye", m, [&] { return orbx_keyframe_fuse_search_fisheye(m, 1, &mono_host, q, 1, 0, pi, pd); });
        bad += refused("orbx_keyframe_fuse_map_points", m, [&] {
            return orbx_keyframe_fuse_map_points(m, 1, &rig_host, cam2, pose2, 3.f, log_sf, 0, kMapPoints, P0.pos.data(), P0.normal.data(), P0.min_dist.data(),
                                                 P0.max_dist.data(), P0.desc.data(), nullptr, bi.data(), bd.data(), nullptr);
        });
        bad += refused("orbx_keyframe_fuse_map_points_fisheye", m, [&] {
            return orbx_keyframe_fuse_map_points_fisheye(m, 1, &mono_host, views4, 3.f, log_sf, 0, kMapPoints, PL0.pos.data(), PL0.normal.data(), PL0.min_dist.data(),
                                                         PL0.max_dist.data(), PL0.desc.data(), nullptr, bi.data(), bd.data(), nullptr);
        });
        bad += refused("orbx_keyframe_compute_bow", m, [&] { return orbx_keyframe_compute_bow(m, rig_host, voc, kLevelsUp, nullptr, nullptr); });
        bad += refused("orbx_keyframe_from_frame", m, [&] { return orbx_keyframe_from_frame(m, fb_rig, inv_sigma2, &out); });
        bad += refused("orbx_keyframe_from_frame_fisheye", m, [&] { return orbx_keyframe_from_frame_fisheye(m, fb_mono, inv_sigma2, &out); });
        for (size_t i = 0; i < bi.size(); i++) if (bi[i] != kSentinel || bd[i] != kSentinel || out) { printf("  a refused call wrote its outputs FAILED\n"); bad++; break; }
    }

    for (orbx_keyframe *kf : {mono_host, mono_handle, mono_other, rig_host, rig_handle, rig_other}) orbx_keyframe_destroy(kf);
    for (orbx_frame *f : {fh_mono, fb_mono, fh_rig, fb_rig}) orbx_frame_destroy(f);
    orbx_vocabulary_destroy(voc);
    orbx_matcher_destroy(m);
    orbx_destroy(ex); orbx_destroy(exl); orbx_destroy(exr);
    if (bad) { printf("keyframe paths FAILED: %d\n", bad); return 1; }
    printf("keyframe paths ok\n");
    return 0;
}
