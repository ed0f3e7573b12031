// A frame handle (orbx_frame) of either kind -- monocular and fisheye-stereo -- is loaded four ways: from host arrays, from an extractor's batch and
// counted first (orbx_frame_count), from the batch with the count(s) left on the device ("pending"), and from the batch, pending, over a handle that
// just held a DIFFERENT frame of the OTHER kind which was loaded, searched and given BoW ("re-used": the case a loader that forgets one of the
// handle's bookkeeping fields breaks).  All handles have one capacity above N.  Per entry point that takes a handle the four handles of the SAME
// frame are reloaded and called: all four must return the same value and the same entries [0, N), the pending ones must end with the counted one's
// counts, and nothing may be written beyond the rows in use (every caller array is a heap block of exactly the needed size, filled with a sentinel).
// After a load each kind's entry points must still refuse the other kind's handle with ORBX_E_BAD_ARG before they enqueue anything (the numbers of
// orbx_matcher_debug_transfers stay those of the call before).  Per load and per call the return value, the counts, a checksum of every result
// array and the six transfer numbers are printed: the output is the same text for any two builds of the library that behave alike.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt) and
// compiled with -fsanitize=address,undefined, as tests/cpp/keyframe_paths_check.cpp.  Prints "frame paths ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kW = 320, kH = 240, kFrames = 2, kLevels = 8, kSentinel = -7, kMapPoints = 300, kLevelsUp = 1;

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
// un: mvKeysUn (what a batch load of a monocular handle copies), else mvKeys (what a batch load of a rig handle copies)
int download(orbx_extractor *ex, int frame, int cap, bool un, Features &F) {
    F.kps.resize(cap); F.desc.resize(32 * (size_t)cap);
    int mono = 0;
    MUST(orbx_batch_download(ex, frame, F.kps.data(), F.desc.data(), cap, &F.n, &mono));
    if (un) MUST(orbx_batch_download_keypoints_un(ex, frame, F.kps.data(), cap, &F.n));
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
        const int i = j % F.n;
        const orbx_keypoint k = F.kps[i];
        Q.x.push_back(k.x + uni(-2.f, 2.f)); Q.y.push_back(k.y + uni(-2.f, 2.f)); Q.xr.push_back(k.x - 2.f + uni(-2.f, 2.f)); Q.yr.push_back(k.y + uni(-2.f, 2.f));
        Q.level.push_back(k.octave); Q.lmin.push_back(k.octave - 1); Q.lmax.push_back(k.octave + 1);
        Q.r.push_back(7.f * scale[k.octave]);
        Q.angle.push_back(k.angle); Q.view_cos.push_back(uni(0.9f, 1.0f));
        for (int b = 0; b < 32; b++) Q.desc.push_back(F.desc[32 * (size_t)i + b]);
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
    std::vector<int32_t> word(F.n), node(F.n);
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

// What a call wrote.  Every array is a heap block of exactly the size the call may write: rows of `row` int32 (byte arrays are widened after the
// call) of which the first `used` are result and the rest must still hold the sentinel; row == 0: the whole array is result.
struct Array {
    std::vector<int32_t> v;
    size_t row = 0, used = 0;
    bool in_use(size_t i) const { return row == 0 || i % row < used; }
};
struct Result {
    int ret = 0;
    std::vector<Array> a;
    // n_rows rows for a handle whose arrays are sized by `rows` features, N of them in use
    int32_t *rows(int rows, int n, int n_rows = 1) {
        a.push_back(Array{std::vector<int32_t>((size_t)n_rows * rows, kSentinel), (size_t)rows, (size_t)n});
        return a.back().v.data();
    }
    template <class T> void whole(const std::vector<T> &x) { a.push_back(Array{std::vector<int32_t>(x.begin(), x.end()), 0, 0}); }
};
// (handle, the features its arrays are sized by, result)
typedef std::function<void(orbx_frame *, int, Result &)> Call;

void transfers(const orbx_matcher *m, int64_t *t) {
    for (int i = 0; i < 6; i++) t[i] = 0;
    orbx_matcher_debug_transfers(m, t, 6);
}
void print_transfers(const orbx_matcher *m) {
    int64_t t[6];
    transfers(m, t);
    printf(", transfers %lld %lld %lld %lld %lld %lld\n", (long long)t[0], (long long)t[1], (long long)t[2], (long long)t[3], (long long)t[4], (long long)t[5]);
}

// One kind of handle: four handles of one capacity, how to load the frame from host arrays and from the batch, and how to give a handle the history
// of the re-used one (another frame of the other kind: loaded, searched, given BoW)
struct Kind {
    const char *name;
    orbx_matcher *m;
    bool fisheye;
    int n, n_left, n_right, cap;   // the frame's counts as the extractor reported them; the handles' capacity
    orbx_frame *h[4];
    std::function<int(orbx_frame *)> load_host, load_batch, other_kind;
};
const char *const kWho[4] = {"host-loaded", "counted first", "count pending", "re-used"};

int load(const Kind &K, int v) {
    if (v == 3) MUST(K.other_kind(K.h[3]));
    const int r = v == 0 ? K.load_host(K.h[v]) : K.load_batch(K.h[v]);
    printf("  load %-14s returned %d", kWho[v], r);
    print_transfers(K.m);
    return r;
}

int check(const char *name, const Kind &K, const Call &call) {
    printf("%s, %s\n", name, K.name);
    int bad = 0, counted[3] = {-2, -2, -2};
    Result R[4];
    for (int v = 0; v < 4; v++) {
        MUST(load(K, v));
        if (v == 1) { MUST(orbx_frame_count(K.h[1], &counted[0])); MUST(orbx_frame_counts(K.h[1], &counted[1], &counted[2])); }
        call(K.h[v], v < 2 ? K.n : K.cap, R[v]);
        printf("  %-19s returned %d", kWho[v], R[v].ret);
        int64_t t[6];
        transfers(K.m, t);
        int c[3] = {-2, -2, -2};
        MUST(orbx_frame_count(K.h[v], &c[0])); MUST(orbx_frame_counts(K.h[v], &c[1], &c[2]));
        printf(", counts %d (%d, %d), checksums", c[0], c[1], c[2]);
        for (const Array &A : R[v].a) {
            long long sum = 0;
            for (size_t i = 0; i < A.v.size(); i++) {
                if (A.in_use(i)) sum = (sum * 31 + A.v[i] + 2) % 1000000007LL;
                if (A.in_use(i) ? A.v[i] == kSentinel : A.v[i] != kSentinel) { printf(" [entry %zu of %zu, rows of %zu, %zu in use: %d]", i, A.v.size(), A.row, A.used, A.v[i]); bad++; break; }
            }
            printf(" %lld", sum);
        }
        printf(", transfers %lld %lld %lld %lld %lld %lld\n", (long long)t[0], (long long)t[1], (long long)t[2], (long long)t[3], (long long)t[4], (long long)t[5]);
        if (c[0] != K.n || c[1] != (K.fisheye ? K.n_left : K.n) || c[2] != (K.fisheye ? K.n_right : -1) || (v >= 1 && memcmp(c, counted, sizeof(c)))) {
            printf("  %s: counts %d (%d, %d), the extractor's %d (%d, %d), the counted handle's %d (%d, %d)\n", kWho[v], c[0], c[1], c[2], K.n, K.n_left, K.n_right,
                   counted[0], counted[1], counted[2]);
            bad++;
        }
        if (R[v].ret < 0 || R[v].ret != R[0].ret || R[v].a.size() != R[0].a.size()) { printf("  %s: returned %d, %zu arrays\n", kWho[v], R[v].ret, R[v].a.size()); bad++; continue; }
        for (size_t k = 0; k < R[v].a.size(); k++) {
            const Array &A = R[v].a[k], &B = R[0].a[k];
            bool same = A.used == B.used && (A.row == 0) == (B.row == 0) && (A.row ? A.v.size() / A.row == B.v.size() / B.row : A.v.size() == B.v.size());
            for (size_t i = 0; same && i < B.v.size(); i++)
                if (B.in_use(i)) same = A.v[B.row ? i / B.row * A.row + i % B.row : i] == B.v[i];
            if (!same) { printf("  %s: array %zu differs from the host-loaded handle's\n", kWho[v], k); bad++; }
        }
    }
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
    std::vector<int32_t> l2r[2], r2l[2];   // mvLeftToRightMatch / mvRightToLeftMatch as the stereo stage left them: what a batch load copies
    for (int f = 0; f < 2; f++) {
        if (download(ex, f, view.cap, true, F[f]) || download(exl, f, view_l.cap, false, FL[f]) || download(exr, f, view_r.cap, false, FR[f])) return 1;
        l2r[f].assign((size_t)view_l.cap, -1); r2l[f].assign((size_t)view_r.cap, -1);
        MUST(orbx_stereo_fisheye_batch_download(exl, f, l2r[f].data(), r2l[f].data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    }
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
    std::vector<uint8_t> rows2[2];   // mDescriptors of the rig: the left camera's rows, then the right camera's
    orbx_frame_desc d[2], dl[2];
    for (int f = 0; f < 2; f++) {
        rows2[f] = FL[f].desc;
        rows2[f].insert(rows2[f].end(), FR[f].desc.begin(), FR[f].desc.end());
        d[f] = desc_of(F[f], F[f].desc.data()); dl[f] = desc_of(FL[f], rows2[f].data());
    }
    const Queries Q = make_queries(F[0], scale, kMapPoints, 11u), QS = make_queries(FL[0], scale, kMapPoints, 12u);
    const Queries Q1 = make_queries(F[1], scale, 40, 13u), QS1 = make_queries(FL[1], scale, 40, 14u);   // what the re-used handles' first frames are searched with
    const int cap = view_l.cap + view_r.cap + 37;   // one capacity for every handle: a rig's batch, and above every N
    if (cap <= view.cap) { printf("capacities\n"); return 1; }
    auto load_mono_host = [&](orbx_frame *f, int fr) { return orbx_frame_load_host(f, &d[fr]); };
    auto load_rig_host = [&](orbx_frame *f, int fr) { return orbx_frame_load_host_fisheye(f, &dl[fr], FR[fr].kps.data(), FR[fr].n, l2r[fr].data(), r2l[fr].data()); };
    std::vector<int32_t> scratch((size_t)cap);
    // frame 1 of a kind on a handle: loaded from host arrays, searched through the window form, given BoW
    auto mono_history = [&](orbx_frame *f) {
        MUST(load_mono_host(f, 1));
        MUST(orbx_frame_search_by_projection_window(m, f, nullptr, Q1.n, Q1.x.data(), Q1.y.data(), Q1.r.data(), Q1.lmin.data(), Q1.lmax.data(), Q1.angle.data(),
                                                    Q1.desc.data(), Q1.has_obs.data(), 64.f, 1, scratch.data()));
        MUST(orbx_frame_compute_bow(m, f, voc, kLevelsUp, nullptr, nullptr));
        return 0;
    };
    auto rig_history = [&](orbx_frame *f) {
        MUST(load_rig_host(f, 1));
        MUST(orbx_frame_search_by_projection_window_fisheye(m, f, nullptr, QS1.n, QS1.x.data(), QS1.y.data(), QS1.r.data(), QS1.lmin.data(), QS1.lmax.data(),
                                                            QS1.angle.data(), QS1.desc.data(), QS1.has_obs.data(), 64.f, 1, scratch.data()));
        MUST(orbx_frame_compute_bow_fisheye(m, f, voc, kLevelsUp, nullptr, nullptr));
        return 0;
    };
    Kind M = {"monocular", m, false, F[0].n, F[0].n, -1, cap, {}, [&](orbx_frame *f) { return load_mono_host(f, 0); },
              [&](orbx_frame *f) { return orbx_frame_load_batch(f, ex, 0, bounds, nullptr, 0); }, rig_history};
    Kind S = {"fisheye", m, true, FL[0].n + FR[0].n, FL[0].n, FR[0].n, cap, {}, [&](orbx_frame *f) { return load_rig_host(f, 0); },
              [&](orbx_frame *f) { return orbx_frame_load_stereo_fisheye_batch(f, exl, exr, 0, bounds, nullptr, 0); }, mono_history};
    for (int v = 0; v < 4; v++) { MUST(orbx_frame_create(m, cap, &M.h[v])); MUST(orbx_frame_create(m, cap, &S.h[v])); }

    HostKeyFrame K0, K1, KS0, KS1;
    if (make_host_keyframe(m, voc, F[1], K0) || make_host_keyframe(m, voc, F[0], K1) || make_host_keyframe(m, voc, FL[1], KS0) || make_host_keyframe(m, voc, FL[0], KS1)) return 1;
    const orbx_bow_keyframe kfs[2] = {K0.kf, K1.kf}, kfs_rig[2] = {KS0.kf, KS1.kf};
    orbx_keyframe *kf = nullptr, *kf_rig = nullptr;
    MUST(orbx_keyframe_create_host(m, &d[1], nullptr, &kf));
    MUST(orbx_keyframe_compute_bow(m, kf, voc, kLevelsUp, nullptr, nullptr));
    MUST(orbx_keyframe_create_host_fisheye(m, &dl[1], FR[1].kps.data(), FR[1].n, nullptr, &kf_rig));
    MUST(orbx_keyframe_compute_bow_fisheye(m, kf_rig, voc, kLevelsUp, nullptr, nullptr));
    const orbx_camera cam = {200.f, 200.f, 160.f, 120.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const orbx_frame_pose pose = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}, {0, 0, 0}};
    const orbx_fisheye_view views[2] = {{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}, {0, 0, 0}, {100.f, 100.f, 160.f, 120.f, 0.f, 0.f, 0.f, 0.f}},
                                        {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {-0.02f, 0, 0}, {0.02f, 0, 0}, {100.f, 100.f, 160.f, 120.f, 0.f, 0.f, 0.f, 0.f}}};
    const float log_sf = std::log(1.2f);
    std::vector<uint8_t> mask_m((size_t)M.n), mask_s((size_t)S.n);   // occupancy masks: N entries
    { std::mt19937 rng(21); for (uint8_t &o : mask_m) o = rng() % 8 == 0; for (uint8_t &o : mask_s) o = rng() % 8 == 0; }
    int bad = 0;
    char name[128];

    // ---- the three projection searches, with and without an occupancy mask
    for (int with_mask = 0; with_mask < 2; with_mask++) {
        const uint8_t *om = with_mask ? mask_m.data() : nullptr, *os = with_mask ? mask_s.data() : nullptr;
        const char *tag = with_mask ? ", mask" : "";
        snprintf(name, sizeof(name), "orbx_frame_search_by_projection_mappoints%s", tag);
        bad += check(name, M, [&](orbx_frame *f, int rows, Result &R) {
            R.ret = orbx_frame_search_by_projection_mappoints(m, f, om, Q.n, Q.x.data(), Q.y.data(), nullptr, Q.level.data(), Q.view_cos.data(), Q.desc.data(),
                                                              Q.in_view.data(), Q.has_obs.data(), 3.f, 0.8f, R.rows(rows, M.n));
        });
        snprintf(name, sizeof(name), "orbx_frame_search_by_projection_frame%s", tag);
        bad += check(name, M, [&](orbx_frame *f, int rows, Result &R) {
            R.ret = orbx_frame_search_by_projection_frame(m, f, om, Q.n, Q.x.data(), Q.y.data(), nullptr, Q.level.data(), Q.angle.data(), Q.desc.data(), Q.has_obs.data(),
                                                          7.f, 0, 1, R.rows(rows, M.n));
        });
        snprintf(name, sizeof(name), "orbx_frame_search_by_projection_window%s", tag);
        bad += check(name, M, [&](orbx_frame *f, int rows, Result &R) {
            R.ret = orbx_frame_search_by_projection_window(m, f, om, Q.n, Q.x.data(), Q.y.data(), Q.r.data(), Q.lmin.data(), Q.lmax.data(), Q.angle.data(), Q.desc.data(),
                                                           Q.has_obs.data(), 64.f, 1, R.rows(rows, M.n));
        });
        snprintf(name, sizeof(name), "orbx_frame_search_by_projection_mappoints_fisheye%s", tag);
        bad += check(name, S, [&](orbx_frame *f, int rows, Result &R) {
            R.ret = orbx_frame_search_by_projection_mappoints_fisheye(m, f, os, QS.n, QS.in_view.data(), QS.x.data(), QS.y.data(), QS.level.data(), QS.view_cos.data(),
                                                                      QS.has_obs.data(), QS.xr.data(), QS.yr.data(), QS.level.data(), QS.view_cos.data(), QS.desc.data(),
                                                                      QS.has_obs.data(), 3.f, 0.8f, R.rows(rows, S.n));
        });
        snprintf(name, sizeof(name), "orbx_frame_search_by_projection_frame_fisheye%s", tag);
        bad += check(name, S, [&](orbx_frame *f, int rows, Result &R) {
            R.ret = orbx_frame_search_by_projection_frame_fisheye(m, f, os, QS.n, QS.x.data(), QS.y.data(), QS.xr.data(), QS.yr.data(), QS.level.data(), QS.angle.data(),
                                                                  QS.desc.data(), QS.has_obs.data(), 7.f, 0, 1, R.rows(rows, S.n));
        });
        snprintf(name, sizeof(name), "orbx_frame_search_by_projection_window_fisheye%s", tag);
        bad += check(name, S, [&](orbx_frame *f, int rows, Result &R) {
            R.ret = orbx_frame_search_by_projection_window_fisheye(m, f, os, QS.n, QS.x.data(), QS.y.data(), QS.r.data(), QS.lmin.data(), QS.lmax.data(), QS.angle.data(),
                                                                   QS.desc.data(), QS.has_obs.data(), 64.f, 1, R.rows(rows, S.n));
        });
    }

    // ---- SearchLocalPoints: 300 map points; with a mask; no map points
    for (int form = 0; form < 3; form++) {
        const int n_mp = form == 2 ? 0 : kMapPoints;
        const char *tag = form == 0 ? "" : form == 1 ? ", mask" : ", no map points";
        snprintf(name, sizeof(name), "orbx_frame_search_local_points%s", tag);
        bad += check(name, M, [&](orbx_frame *f, int rows, Result &R) {
            std::vector<uint8_t> in_view((size_t)n_mp, 0xee);
            R.ret = orbx_frame_search_local_points(m, f, form == 1 ? mask_m.data() : nullptr, &cam, &pose, log_sf, 0.5f, n_mp, Q.pos.data(), Q.normal.data(),
                                                   Q.min_dist.data(), Q.max_dist.data(), Q.desc.data(), nullptr, Q.has_obs.data(), 3.f, 0.8f, 0, 0.f, in_view.data(),
                                                   R.rows(rows, M.n));
            R.whole(in_view);
        });
        snprintf(name, sizeof(name), "orbx_frame_search_local_points_fisheye%s", tag);
        bad += check(name, S, [&](orbx_frame *f, int rows, Result &R) {
            std::vector<uint8_t> in_view(2 * (size_t)n_mp, 0xee);
            R.ret = orbx_frame_search_local_points_fisheye(m, f, form == 1 ? mask_s.data() : nullptr, views, log_sf, 0.5f, n_mp, QS.pos_kb8.data(), QS.normal.data(),
                                                           QS.min_dist.data(), QS.max_dist.data(), QS.desc.data(), nullptr, QS.has_obs.data(), nullptr, 3.f, 0.8f, 0, 0.f,
                                                           in_view.data(), R.rows(rows, S.n));
            R.whole(in_view);
        });
    }

    // ---- ComputeBoW: both id buffers; the word ids only; none
    for (int form = 0; form < 3; form++) {
        const char *tag = form == 0 ? ", word and node ids" : form == 1 ? ", word ids" : ", no id buffers";
        for (const Kind *K : {&M, &S}) {
            snprintf(name, sizeof(name), "orbx_frame_compute_bow%s%s", K->fisheye ? "_fisheye" : "", tag);
            bad += check(name, *K, [&](orbx_frame *f, int rows, Result &R) {
                int32_t *w = form < 2 ? R.rows(rows, K->n) : nullptr, *nd = form < 1 ? R.rows(rows, K->n) : nullptr;
                if (form < 1) w = R.a[0].v.data();   // (the second push_back may have moved the first array's header, never its block)
                R.ret = K->fisheye ? orbx_frame_compute_bow_fisheye(m, f, voc, kLevelsUp, w, nd) : orbx_frame_compute_bow(m, f, voc, kLevelsUp, w, nd);
            });
        }
    }

    // ---- SearchByBoW against two key frames given as host arrays, and against one resident key frame
    for (const Kind *K : {&M, &S}) {
        snprintf(name, sizeof(name), "orbx_frame_search_by_bow%s, K = 2", K->fisheye ? "_fisheye" : "");
        bad += check(name, *K, [&](orbx_frame *f, int rows, Result &R) {
            R.ret = K->fisheye ? orbx_frame_compute_bow_fisheye(m, f, voc, kLevelsUp, nullptr, nullptr) : orbx_frame_compute_bow(m, f, voc, kLevelsUp, nullptr, nullptr);
            if (R.ret < 0) return;
            std::vector<int32_t> nm(2, kSentinel);
            int32_t *match = R.rows(rows, K->n, 2);
            R.ret = K->fisheye ? orbx_frame_search_by_bow_fisheye(m, f, 2, kfs_rig, 0.8f, 1, match, rows, nm.data())
                               : orbx_frame_search_by_bow(m, f, 2, kfs, 0.8f, 1, match, rows, nm.data());
            R.whole(nm);
        });
        snprintf(name, sizeof(name), "orbx_frame_search_by_bow_resident%s, K = 1", K->fisheye ? "_fisheye" : "");
        bad += check(name, *K, [&](orbx_frame *f, int rows, Result &R) {
            R.ret = K->fisheye ? orbx_frame_compute_bow_fisheye(m, f, voc, kLevelsUp, nullptr, nullptr) : orbx_frame_compute_bow(m, f, voc, kLevelsUp, nullptr, nullptr);
            if (R.ret < 0) return;
            std::vector<int32_t> nm(1, kSentinel);
            int32_t *match = R.rows(rows, K->n);
            R.ret = K->fisheye ? orbx_frame_search_by_bow_resident_fisheye(m, f, 1, &kf_rig, nullptr, 0.8f, 1, match, rows, nm.data())
                               : orbx_frame_search_by_bow_resident(m, f, 1, &kf, nullptr, 0.8f, 1, match, rows, nm.data());
            R.whole(nm);
        });
    }

    // ---- an empty frame loaded from host arrays through SearchLocalPoints: returns 0 and writes mbTrackInView
    {
        printf("an empty frame through SearchLocalPoints\n");
        orbx_frame_desc e = d[0], el = dl[0];
        e.n = 0; el.n = 0;
        std::vector<uint8_t> in_view(2 * (size_t)kMapPoints, 0xee);
        std::vector<int32_t> none(1, kSentinel);
        int r = orbx_frame_load_host(M.h[3], &e);
        printf("  load monocular returned %d", r);
        print_transfers(m);
        int r2 = orbx_frame_search_local_points(m, M.h[3], nullptr, &cam, &pose, log_sf, 0.5f, kMapPoints, Q.pos.data(), Q.normal.data(), Q.min_dist.data(),
                                                Q.max_dist.data(), Q.desc.data(), nullptr, Q.has_obs.data(), 3.f, 0.8f, 0, 0.f, in_view.data(), none.data());
        int seen = 0, bytes_bad = 0;
        for (int j = 0; j < kMapPoints; j++) { seen += in_view[j] == 1; bytes_bad += in_view[j] > 1; }
        printf("  monocular returned %d, %d in view", r2, seen);
        print_transfers(m);
        if (r != 0 || r2 != 0 || bytes_bad || seen == 0 || none[0] != kSentinel) { printf("  FAILED\n"); bad++; }
        in_view.assign(in_view.size(), 0xee);
        r = orbx_frame_load_host_fisheye(S.h[3], &el, nullptr, 0, nullptr, nullptr);
        printf("  load fisheye returned %d", r);
        print_transfers(m);
        r2 = orbx_frame_search_local_points_fisheye(m, S.h[3], nullptr, views, log_sf, 0.5f, kMapPoints, QS.pos_kb8.data(), QS.normal.data(), QS.min_dist.data(),
                                                    QS.max_dist.data(), QS.desc.data(), nullptr, QS.has_obs.data(), nullptr, 3.f, 0.8f, 0, 0.f, in_view.data(), none.data());
        seen = 0; bytes_bad = 0;
        for (int j = 0; j < 2 * kMapPoints; j++) { seen += in_view[j] == 1; bytes_bad += in_view[j] > 1; }
        printf("  fisheye returned %d, %d in view", r2, seen);
        print_transfers(m);
        if (r != 0 || r2 != 0 || bytes_bad || seen == 0 || none[0] != kSentinel) { printf("  FAILED\n"); bad++; }
    }

    // ---- every entry point with the other kind's handle, host-loaded and re-used (the re-used monocular handle last held a rig frame and the other way round)
    printf("the other kind's handle\n");
    for (int v : {0, 3}) {
        if (load(M, v) < 0 || load(S, v) < 0) return 1;
        std::vector<int32_t> out(2 * (size_t)cap, kSentinel), nm(2, kSentinel);
        std::vector<uint8_t> in_view(2 * (size_t)kMapPoints, 0xee);
        orbx_frame *fm = M.h[v], *fs = S.h[v];
        MUST(orbx_frame_compute_bow(m, fm, voc, kLevelsUp, nullptr, nullptr));
        MUST(orbx_frame_compute_bow_fisheye(m, fs, voc, kLevelsUp, nullptr, nullptr));
        MUST(orbx_frame_search_by_bow(m, fm, 1, kfs, 0.8f, 1, out.data(), cap, nm.data()));   // (a call with transfers: what the refusals must leave as it is)
        out.assign(out.size(), kSentinel); nm.assign(2, kSentinel);
        bad += refused("orbx_frame_search_by_projection_mappoints", m, [&] {
            return orbx_frame_search_by_projection_mappoints(m, fs, nullptr, Q.n, Q.x.data(), Q.y.data(), nullptr, Q.level.data(), Q.view_cos.data(), Q.desc.data(),
                                                             Q.in_view.data(), Q.has_obs.data(), 3.f, 0.8f, out.data());
        });
        bad += refused("orbx_frame_search_by_projection_frame", m, [&] {
            return orbx_frame_search_by_projection_frame(m, fs, nullptr, Q.n, Q.x.data(), Q.y.data(), nullptr, Q.level.data(), Q.angle.data(), Q.desc.data(), Q.has_obs.data(),
                                                         7.f, 0, 1, out.data());
        });
        bad += refused("orbx_frame_search_by_projection_window", m, [&] {
            return orbx_frame_search_by_projection_window(m, fs, nullptr, Q.n, Q.x.data(), Q.y.data(), Q.r.data(), Q.lmin.data(), Q.lmax.data(), Q.angle.data(), Q.desc.data(),
                                                          Q.has_obs.data(), 64.f, 1, out.data());
        });
        bad += refused("orbx_frame_search_local_points", m, [&] {
            return orbx_frame_search_local_points(m, fs, nullptr, &cam, &pose, log_sf, 0.5f, kMapPoints, Q.pos.data(), Q.normal.data(), Q.min_dist.data(), Q.max_dist.data(),
                                                  Q.desc.data(), nullptr, Q.has_obs.data(), 3.f, 0.8f, 0, 0.f, in_view.data(), out.data());
        });
        bad += refused("orbx_frame_compute_bow", m, [&] { return orbx_frame_compute_bow(m, fs, voc, kLevelsUp, out.data(), nullptr); });
        bad += refused("orbx_frame_search_by_bow", m, [&] { return orbx_frame_search_by_bow(m, fs, 1, kfs, 0.8f, 1, out.data(), cap, nm.data()); });
        bad += refused("orbx_frame_search_by_bow_resident", m, [&] { return orbx_frame_search_by_bow_resident(m, fs, 1, &kf, nullptr, 0.8f, 1, out.data(), cap, nm.data()); });
        bad += refused("orbx_frame_search_by_projection_mappoints_fisheye", m, [&] {
            return orbx_frame_search_by_projection_mappoints_fisheye(m, fm, nullptr, QS.n, QS.in_view.data(), QS.x.data(), QS.y.data(), QS.level.data(), QS.view_cos.data(),
                                                                     QS.has_obs.data(), QS.xr.data(), QS.yr.data(), QS.level.data(), QS.view_cos.data(), QS.desc.data(),
                                                                     QS.has_obs.data(), 3.f, 0.8f, out.data());
        });
        bad += refused("orbx_frame_search_by_projection_frame_fisheye", m, [&] {
            return orbx_frame_search_by_projection_frame_fisheye(m, fm, nullptr, QS.n, QS.x.data(), QS.y.data(), QS.xr.data(), QS.yr.data(), QS.level.data(), QS.angle.data(),
                                                                 QS.desc.data(), QS.has_obs.data(), 7.f, 0, 1, out.data());
        });
        bad += refused("orbx_frame_search_by_projection_window_fisheye", m, [&] {
            return orbx_frame_search_by_projection_window_fisheye(m, fm, nullptr, QS.n, QS.x.data(), QS.y.data(), QS.r.data(), QS.lmin.data(), QS.lmax.data(), QS.angle.data(),
                                                                  QS.desc.data(), QS.has_obs.data(), 64.f, 1, out.data());
        });
        bad += refused("orbx_frame_search_local_points_fisheye", m, [&] {
            return orbx_frame_search_local_points_fisheye(m, fm, nullptr, views, log_sf, 0.5f, kMapPoints, QS.pos_kb8.data(), QS.normal.data(), QS.min_dist.data(),
                                                          QS.max_dist.data(), QS.desc.data(), nullptr, QS.has_obs.data(), nullptr, 3.f, 0.8f, 0, 0.f, in_view.data(), out.data());
        });
        bad += refused("orbx_frame_compute_bow_fisheye", m, [&] { return orbx_frame_compute_bow_fisheye(m, fm, voc, kLevelsUp, out.data(), nullptr); });
        bad += refused("orbx_frame_search_by_bow_fisheye", m, [&] { return orbx_frame_search_by_bow_fisheye(m, fm, 1, kfs_rig, 0.8f, 1, out.data(), cap, nm.data()); });
        bad += refused("orbx_frame_search_by_bow_resident_fisheye", m, [&] {
            return orbx_frame_search_by_bow_resident_fisheye(m, fm, 1, &kf_rig, nullptr, 0.8f, 1, out.data(), cap, nm.data());
        });
        bool wrote = nm[0] != kSentinel || nm[1] != kSentinel;
        for (int32_t o : out) wrote = wrote || o != kSentinel;
        for (uint8_t b : in_view) wrote = wrote || b != 0xee;
        if (wrote) { printf("  a refused call wrote its outputs FAILED\n"); bad++; }
    }

    orbx_keyframe_destroy(kf); orbx_keyframe_destroy(kf_rig);
    for (int v = 0; v < 4; v++) { orbx_frame_destroy(M.h[v]); orbx_frame_destroy(S.h[v]); }
    orbx_vocabulary_destroy(voc);
    orbx_matcher_destroy(m);
    orbx_destroy(ex); orbx_destroy(exl); orbx_destroy(exr);
    if (bad) { printf("frame paths FAILED: %d\n", bad); return 1; }
    printf("frame paths ok\n");
    return 0;
}
