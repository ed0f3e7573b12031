// A frame handle loaded from an extractor's batch does not know its feature count N on the host: the first call that touches it sizes its buffers by
// the handle's capacity and brings N home with its results.  Per entry point that can be that first call, two handles are loaded from the same
// batch frame with a capacity above N: A is counted first (orbx_frame_count), B is not.  The same call on both must return the same value, write the
// same entries [0, N), leave the caller's array untouched beyond N (every array is a heap block of exactly the capacity, filled with a sentinel), and
// leave B with A's count(s).  Per call the six numbers of orbx_matcher_debug_transfers are printed for A and for B.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt, whose
// stand-in runtime takes any host pointer as pinned memory) and compiled with -fsanitize=address,undefined, which sees a copy that runs past an
// array.  Prints "frame pending count ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kW = 320, kH = 240, kFrames = 2, kLevels = 8, kSentinel = -7;
constexpr int kLevelsUp = 1;

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
    std::vector<float> angle;
    int n = 0;
};
int download(orbx_extractor *ex, int frame, int cap, Features &F) {
    F.kps.resize(cap); F.desc.resize(32 * (size_t)cap);
    int mono = 0;
    MUST(orbx_batch_download(ex, frame, F.kps.data(), F.desc.data(), cap, &F.n, &mono));
    F.kps.resize(F.n); F.desc.resize(32 * (size_t)F.n); F.angle.resize(F.n);
    for (int i = 0; i < F.n; i++) F.angle[i] = F.kps[i].angle;
    return 0;
}

// queries that look at the features of F: a jittered copy of feature j % n each, a few descriptor bits flipped
struct Queries {
    int n = 0;
    std::vector<float> x, y, xr, yr, r, angle, view_cos;
    std::vector<int32_t> level, lmin, lmax;
    std::vector<uint8_t> desc, has_obs, in_view;
    // the same as map points in front of a camera at the origin (pinhole: fx = fy = 200; KannalaBrandt8 without distortion: fx = fy = 100)
    std::vector<float> pos, pos_kb8, normal, min_dist, max_dist;
};
Queries make_queries(const Features &F, const float *scale, int nq, uint32_t seed) {
    std::mt19937 rng(seed);
    auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    Queries Q;
    Q.n = nq;
    for (int j = 0; j < nq; j++) {
        const int i = j % std::max(F.n, 1);
        const orbx_keypoint k = F.n ? F.kps[i] : orbx_keypoint{160.f, 120.f, 31.f, 0.f, 50.f, 0, -1};
        Q.x.push_back(k.x + uni(-2.f, 2.f)); Q.y.push_back(k.y + uni(-2.f, 2.f)); Q.xr.push_back(k.x - 2.f + uni(-2.f, 2.f)); Q.yr.push_back(k.y + uni(-2.f, 2.f));
        Q.level.push_back(k.octave); Q.lmin.push_back(k.octave - 1); Q.lmax.push_back(k.octave + 1);
        Q.r.push_back(7.f * scale[k.octave]);
        Q.angle.push_back(k.angle); Q.view_cos.push_back(uni(0.9f, 1.0f));
        for (int b = 0; b < 32; b++) Q.desc.push_back(F.n ? F.desc[32 * (size_t)i + b] : (uint8_t)rng());
        for (int f = 0; f < 10; f++) { const unsigned b = rng() % 256; Q.desc[32 * (size_t)j + b / 8] ^= (uint8_t)(1u << (b % 8)); }
        Q.has_obs.push_back(rng() % 5 != 0); Q.in_view.push_back(rng() % 10 != 0);
        const float d = uni(2.f, 12.f);
        const float px = (Q.x[j] - 160.f) / 200.f, py = (Q.y[j] - 120.f) / 200.f, pn = std::sqrt(px * px + py * py + 1.f);
        Q.pos.insert(Q.pos.end(), {d * px / pn, d * py / pn, d / pn});
        const float ax = (Q.x[j] - 160.f) / 100.f, ay = (Q.y[j] - 120.f) / 100.f, theta = std::sqrt(ax * ax + ay * ay), s = theta > 1e-6f ? std::sin(theta) / theta : 1.f;
        Q.pos_kb8.insert(Q.pos_kb8.end(), {d * s * ax, d * s * ay, d * std::cos(theta)});
        Q.normal.insert(Q.normal.end(), {px / pn, py / pn, 1.f / pn});   // (seen head-on)
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

// a key frame of a BoW search given as host arrays: the features of F and their FeatureVector under the vocabulary
struct HostKeyFrame {
    std::vector<uint32_t> node_id;
    std::vector<int32_t> node_ptr, index;
    orbx_bow_keyframe kf;
};
int make_host_keyframe(orbx_matcher *m, const orbx_vocabulary *voc, const Features &F, HostKeyFrame &K) {
    std::vector<int32_t> word(std::max(F.n, 1)), node(std::max(F.n, 1));
    MUST(orbx_bow_transform(m, voc, F.desc.data(), F.n, kLevelsUp, word.data(), node.data()));
    K.node_ptr.assign(1, 0);
    for (int id = 0; id < 21; id++) {
        const size_t before = K.index.size();
        for (int i = 0; i < F.n; i++) if (node[i] == id) K.index.push_back(i);
        if (K.index.size() > before) { K.node_id.push_back((uint32_t)id); K.node_ptr.push_back((int32_t)K.index.size()); }
    }
    K.kf = orbx_bow_keyframe{F.desc.data(), F.angle.data(), nullptr, F.n, {K.node_id.data(), K.node_ptr.data(), K.index.data(), (int32_t)K.node_id.size()}};
    return 0;
}

typedef std::vector<std::vector<int32_t>> Arrays;   // what a call writes: every array a heap block of its own
// (handle, arrays) -> the call's return value; an array holds rows of the handle's capacity whose first N entries the call writes
typedef std::function<int(orbx_frame *, Arrays &)> Call;

struct Kind {
    orbx_matcher *m;
    int cap;
    bool fisheye;
    std::function<int(orbx_frame *)> load;
};

void print_transfers(const char *who, const orbx_matcher *m) {
    int64_t t[6] = {0, 0, 0, 0, 0, 0};
    orbx_matcher_debug_transfers(m, t, 6);
    printf("  %s: transfers %lld %lld %lld %lld %lld %lld\n", who, (long long)t[0], (long long)t[1], (long long)t[2], (long long)t[3], (long long)t[4], (long long)t[5]);
}

int check(const char *name, const Kind &K, const Call &call) {
    orbx_frame *A = nullptr, *B = nullptr;
    MUST(orbx_frame_create(K.m, K.cap, &A)); MUST(orbx_frame_create(K.m, K.cap, &B));
    MUST(K.load(A)); MUST(K.load(B));
    int n = -1, nl = -1, nr = -1, nb = -1, nlb = -1, nrb = -1;
    MUST(orbx_frame_count(A, &n)); MUST(orbx_frame_counts(A, &nl, &nr));
    Arrays a, b;
    printf("%s\n", name);
    const int ra = call(A, a);
    print_transfers("counted first", K.m);
    const int rb = call(B, b);
    print_transfers("count pending", K.m);
    MUST(orbx_frame_count(B, &nb)); MUST(orbx_frame_counts(B, &nlb, &nrb));
    int bad = 0;
    long long sum = 0;
    if (ra < 0 || ra != rb) { printf("%s: returned %d with the count known, %d with the count pending\n", name, ra, rb); bad++; }
    if (n >= K.cap || n != nb || nl != nlb || nr != nrb) { printf("%s: counts %d (%d, %d) and %d (%d, %d), capacity %d\n", name, n, nl, nr, nb, nlb, nrb, K.cap); bad++; }
    if (a.size() != b.size()) { printf("%s: %zu and %zu arrays\n", name, a.size(), b.size()); bad++; }
    for (size_t k = 0; k < a.size() && !bad; k++) {
        if (a[k].size() != b[k].size() || a[k].size() % (size_t)K.cap) { printf("%s: array %zu of %zu and %zu entries\n", name, k, a[k].size(), b[k].size()); bad++; break; }
        for (size_t i = 0; i < a[k].size(); i++) {
            const bool inside = (int)(i % (size_t)K.cap) < n;
            if (inside ? a[k][i] != b[k][i] || a[k][i] == kSentinel : a[k][i] != kSentinel || b[k][i] != kSentinel) {
                printf("%s: array %zu entry %zu (N = %d): %d with the count known, %d with the count pending\n", name, k, i, n, a[k][i], b[k][i]);
                bad++;
                break;
            }
            if (inside) sum = (sum * 31 + a[k][i] + 2) % 1000000007LL;
        }
    }
    printf("  returned %d, N = %d (%d, %d), %zu arrays, checksum %lld%s\n", ra, n, nl, nr, a.size(), sum, bad ? " FAILED" : "");
    orbx_frame_destroy(A); orbx_frame_destroy(B);
    return bad;
}

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
    Features F0, F1, FL0, FL1;
    if (download(ex, 0, view.cap, F0) || download(ex, 1, view.cap, F1) || download(exl, 0, view_l.cap, FL0) || download(exl, 1, view_l.cap, FL1)) return 1;
    printf("pinhole frame 0: %d features, fisheye frame 0: %d left features\n", F0.n, FL0.n);
    if (F0.n < 50 || FL0.n < 50) { printf("the scene is too poor\n"); return 1; }

    orbx_matcher *m = nullptr;
    MUST(orbx_matcher_create(0, &m));
    orbx_vocabulary *voc = nullptr;
    if (make_vocabulary(&voc)) return 1;
    const float bounds[4] = {0.f, (float)kW, 0.f, (float)kH};
    const Kind P = {m, view.cap + 37, false, [&](orbx_frame *f) { return orbx_frame_load_batch(f, ex, 0, bounds, nullptr, 0); }};
    const Kind S = {m, view_l.cap + view_r.cap + 37, true, [&](orbx_frame *f) { return orbx_frame_load_stereo_fisheye_batch(f, exl, exr, 0, bounds, nullptr, 0); }};
    const Queries Q = make_queries(F0, scale, 700, 11u), QS = make_queries(FL0, scale, 700, 12u);
    HostKeyFrame K0, K1, KS;
    if (make_host_keyframe(m, voc, F1, K0) || make_host_keyframe(m, voc, F0, K1) || make_host_keyframe(m, voc, FL1, KS)) return 1;
    const orbx_bow_keyframe kfs[2] = {K0.kf, K1.kf};
    orbx_frame_desc d1;
    memset(&d1, 0, sizeof(d1));
    d1.keypoints_un = F1.kps.data(); d1.descriptors = F1.desc.data(); d1.n = F1.n; d1.max_x = (float)kW; d1.max_y = (float)kH;
    d1.scale_factors = scale; d1.nlevels = kLevels;
    orbx_keyframe *kf = nullptr;
    MUST(orbx_keyframe_create_host(m, &d1, nullptr, &kf));
    MUST(orbx_keyframe_compute_bow(m, kf, voc, kLevelsUp, nullptr, nullptr));
    const orbx_camera cam = {200.f, 200.f, 160.f, 120.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const orbx_frame_pose pose = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}, {0, 0, 0}};
    const orbx_fisheye_view views[2] = {{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}, {0, 0, 0}, {100.f, 100.f, 160.f, 120.f, 0.f, 0.f, 0.f, 0.f}},
                                        {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {-0.02f, 0, 0}, {0.02f, 0, 0}, {100.f, 100.f, 160.f, 120.f, 0.f, 0.f, 0.f, 0.f}}};
    const float log_sf = std::log(1.2f);
    auto rows = [](Arrays &out, int cap, int n_arrays, int n_rows = 1) { out.assign((size_t)n_arrays, std::vector<int32_t>((size_t)n_rows * cap, kSentinel)); };
    int bad = 0;

    bad += check("orbx_frame_search_by_projection_mappoints", P, [&](orbx_frame *f, Arrays &out) {
        rows(out, P.cap, 1);
        return orbx_frame_search_by_projection_mappoints(m, f, nullptr, Q.n, Q.x.data(), Q.y.data(), nullptr, Q.level.data(), Q.view_cos.data(), Q.desc.data(),
                                                         Q.in_view.data(), Q.has_obs.data(), 3.f, 0.8f, out[0].data());
    });
    bad += check("orbx_frame_search_by_projection_frame", P, [&](orbx_frame *f, Arrays &out) {
        rows(out, P.cap, 1);
        return orbx_frame_search_by_projection_frame(m, f, nullptr, Q.n, Q.x.data(), Q.y.data(), nullptr, Q.level.data(), Q.angle.data(), Q.desc.data(),
                                                     Q.has_obs.data(), 7.f, 0, 1, out[0].data());
    });
    bad += check("orbx_frame_search_by_projection_window", P, [&](orbx_frame *f, Arrays &out) {
        rows(out, P.cap, 1);
        return orbx_frame_search_by_projection_window(m, f, nullptr, Q.n, Q.x.data(), Q.y.data(), Q.r.data(), Q.lmin.data(), Q.lmax.data(), Q.angle.data(),
                                                      Q.desc.data(), Q.has_obs.data(), 64.f, 1, out[0].data());
    });
    bad += check("orbx_frame_search_local_points", P, [&](orbx_frame *f, Arrays &out) {
        rows(out, P.cap, 1);
        std::vector<uint8_t> in_view(Q.n);
        const int r = orbx_frame_search_local_points(m, f, nullptr, &cam, &pose, log_sf, 0.5f, Q.n, Q.pos.data(), Q.normal.data(), Q.min_dist.data(),
                                                     Q.max_dist.data(), Q.desc.data(), nullptr, Q.has_obs.data(), 3.f, 0.8f, 0, 0.f, in_view.data(), out[0].data());
        out.push_back(std::vector<int32_t>(P.cap, kSentinel));   // mbTrackInView, as entries [0, N) of a second array
        int seen = 0;
        for (int j = 0; j < Q.n; j++) seen += in_view[j];
        int n = 0;
        orbx_frame_count(f, &n);
        for (int i = 0; i < n; i++) out[1][i] = seen;
        return r;
    });
    bad += check("orbx_frame_compute_bow", P, [&](orbx_frame *f, Arrays &out) {
        rows(out, P.cap, 2);
        return orbx_frame_compute_bow(m, f, voc, kLevelsUp, out[0].data(), out[1].data());
    });
    bad += check("orbx_frame_compute_bow, word ids only", P, [&](orbx_frame *f, Arrays &out) {
        rows(out, P.cap, 1);
        return orbx_frame_compute_bow(m, f, voc, kLevelsUp, out[0].data(), nullptr);
    });
    bad += check("orbx_frame_search_by_bow", P, [&](orbx_frame *f, Arrays &out) {
        rows(out, P.cap, 2, 2);   // [0]: the two rows at the stride of the capacity, [1]: nmatches
        const int r = orbx_frame_compute_bow(m, f, voc, kLevelsUp, nullptr, nullptr);
        if (r < 0) return r;
        int32_t nm[2] = {0, 0};
        const int r2 = orbx_frame_search_by_bow(m, f, 2, kfs, 0.8f, 1, out[0].data(), P.cap, nm);
        int n = 0;
        orbx_frame_count(f, &n);
        for (int k = 0; k < 2; k++) for (int i = 0; i < n; i++) out[1][(size_t)k * P.cap + i] = nm[k];
        return r2;
    });
    bad += check("orbx_frame_search_by_bow_resident", P, [&](orbx_frame *f, Arrays &out) {
        rows(out, P.cap, 1);
        const int r = orbx_frame_compute_bow(m, f, voc, kLevelsUp, nullptr, nullptr);
        if (r < 0) return r;
        int32_t nm = 0;
        const int r2 = orbx_frame_search_by_bow_resident(m, f, 1, &kf, nullptr, 0.8f, 1, out[0].data(), P.cap, &nm);
        return r2 < 0 ? r2 : nm;
    });

    bad += check("orbx_frame_search_by_projection_mappoints_fisheye", S, [&](orbx_frame *f, Arrays &out) {
        rows(out, S.cap, 1);
        return orbx_frame_search_by_projection_mappoints_fisheye(m, f, nullptr, QS.n, QS.in_view.data(), QS.x.data(), QS.y.data(), QS.level.data(), QS.view_cos.data(),
                                                                 QS.has_obs.data(), QS.xr.data(), QS.yr.data(), QS.level.data(), QS.view_cos.data(), QS.desc.data(),
                                                                 QS.has_obs.data(), 3.f, 0.8f, out[0].data());
    });
    bad += check("orbx_frame_search_by_projection_frame_fisheye", S, [&](orbx_frame *f, Arrays &out) {
        rows(out, S.cap, 1);
        return orbx_frame_search_by_projection_frame_fisheye(m, f, nullptr, QS.n, QS.x.data(), QS.y.data(), QS.xr.data(), QS.yr.data(), QS.level.data(), QS.angle.data(),
                                                             QS.desc.data(), QS.has_obs.data(), 7.f, 0, 1, out[0].data());
    });
    bad += check("orbx_frame_search_by_projection_window_fisheye", S, [&](orbx_frame *f, Arrays &out) {
        rows(out, S.cap, 1);
        return orbx_frame_search_by_projection_window_fisheye(m, f, nullptr, QS.n, QS.x.data(), QS.y.data(), QS.r.data(), QS.lmin.data(), QS.lmax.data(),
                                                              QS.angle.data(), QS.desc.data(), QS.has_obs.data(), 64.f, 1, out[0].data());
    });
    bad += check("orbx_frame_search_local_points_fisheye", S, [&](orbx_frame *f, Arrays &out) {
        rows(out, S.cap, 1);
        std::vector<uint8_t> in_view(2 * (size_t)QS.n);
        return orbx_frame_search_local_points_fisheye(m, f, nullptr, views, log_sf, 0.5f, QS.n, QS.pos_kb8.data(), QS.normal.data(), QS.min_dist.data(),
                                                      QS.max_dist.data(), QS.desc.data(), nullptr, QS.has_obs.data(), nullptr, 3.f, 0.8f, 0, 0.f, in_view.data(),
                                                      out[0].data());
    });
    bad += check("orbx_frame_compute_bow_fisheye", S, [&](orbx_frame *f, Arrays &out) {
        rows(out, S.cap, 2);
        return orbx_frame_compute_bow_fisheye(m, f, voc, kLevelsUp, out[0].data(), out[1].data());
    });
    bad += check("orbx_frame_search_by_bow_fisheye", S, [&](orbx_frame *f, Arrays &out) {
        rows(out, S.cap, 1);
        const int r = orbx_frame_compute_bow_fisheye(m, f, voc, kLevelsUp, nullptr, nullptr);
        if (r < 0) return r;
        int32_t nm = 0;
        const int r2 = orbx_frame_search_by_bow_fisheye(m, f, 1, &KS.kf, 0.8f, 1, out[0].data(), S.cap, &nm);
        return r2 < 0 ? r2 : nm;
    });

    orbx_keyframe_destroy(kf);
    orbx_vocabulary_destroy(voc);
    orbx_matcher_destroy(m);
    orbx_destroy(ex); orbx_destroy(exl); orbx_destroy(exr);
    if (bad) { printf("frame pending count FAILED: %d\n", bad); return 1; }
    printf("frame pending count ok\n");
    return 0;
}
