// The synchronous downloads of the extractor and of the stages that run behind an extraction: orbx_batch_download, orbx_batch_download_all,
// orbx_batch_download_keypoints_un, orbx_get_level, orbx_debug_level_keypoints, orbx_stereo_batch_download[_all],
// orbx_stereo_fisheye_batch_download[_all], and the two RGB-D stages (float and 16-bit depth) with an asynchronous download between two batches.
// Every caller buffer is a heap block of exactly the bytes the contract allows the call to write, filled with a sentinel before the call: a copy of
// `cap` entries where `n` are due ends the run, an output written through another output's place in the staging block fails an equality.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt, whose
// stand-in runtime takes any host pointer as device memory) and compiled with -fsanitize=address,undefined.  Prints "staged downloads ok", returns 0.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kW = 320, kH = 240, kFrames = 3, kFlat = 1, kLevels = 8;
constexpr uint8_t kFill = 0xA5;

#define MUST(expr)                                                                   \
    do {                                                                             \
        const int r_ = (expr);                                                       \
        if (r_ < 0) { printf("%s: %d %s\n", #expr, r_, orbx_last_error()); return 1; } \
    } while (0)
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

// a heap block of exactly n elements, every byte the sentinel
template <class T> struct Block {
    std::unique_ptr<T[]> p;
    size_t n;
    explicit Block(size_t n_) : p(new T[n_]), n(n_) { memset((void *)p.get(), kFill, n * sizeof(T)); }
    T *get() const { return p.get(); }
    size_t bytes() const { return n * sizeof(T); }
    bool untouched() const {
        const uint8_t *b = (const uint8_t *)p.get();
        for (size_t i = 0; i < bytes(); i++)
            if (b[i] != kFill) return false;
        return true;
    }
};
template <class T> bool same(const Block<T> &a, const Block<T> &b) { return a.n == b.n && memcmp((const void *)a.get(), (const void *)b.get(), a.bytes()) == 0; }
template <class T> bool same_row(const Block<T> &row, const Block<T> &all, size_t first) {
    return first + row.n <= all.n && memcmp((const void *)row.get(), (const void *)(all.get() + first), row.bytes()) == 0;
}

// kFrames views (shifted by `dx` + 3 per frame) of one canvas of random rectangles: corners for FAST; frame kFlat is one grey value (no feature)
std::vector<uint8_t> make_images(int dx, int seed) {
    const int cw = kW + 32, ch = kH + 16;
    std::mt19937 rng(seed);
    std::vector<int> canvas((size_t)cw * ch, 110);
    for (int k = 0; k < 260; k++) {
        const int x0 = (int)(rng() % cw), y0 = (int)(rng() % ch), w = 6 + (int)(rng() % 40), h = 6 + (int)(rng() % 40), d = (int)(rng() % 120) - 60;
        for (int y = y0; y < std::min(ch, y0 + h); y++)
            for (int x = x0; x < std::min(cw, x0 + w); x++) canvas[(size_t)y * cw + x] += d;
    }
    std::vector<uint8_t> img((size_t)kFrames * kW * kH);
    for (int f = 0; f < kFrames; f++)
        for (int y = 0; y < kH; y++)
            for (int x = 0; x < kW; x++)
                img[((size_t)f * kH + y) * kW + x] = f == kFlat ? 110 : (uint8_t)std::min(255, std::max(0, canvas[(size_t)(y + 2 * f) * cw + x + dx + 3 * f]));
    return img;
}

int extract(orbx_extractor *ex, const std::vector<uint8_t> &img) {
    MUST(orbx_extract_batch_host(ex, img.data(), kFrames, kW, kH, kW, (size_t)kW * kH, 0, kW));
    return 0;
}

int make_extractor(const std::vector<uint8_t> &img, orbx_extractor **ex) {
    const orbx_params prm = {500, 1.2f, kLevels, 20, 7, 0};
    MUST(orbx_create(&prm, 0, kW, kH, kFrames, ex));
    return extract(*ex, img);
}

// ---------------------------------------------------------------------------------------------------------
// the extractor's own downloads
// ---------------------------------------------------------------------------------------------------------
struct BatchAll {
    Block<orbx_keypoint> kps;
    Block<uint8_t> desc;
    Block<int32_t> counts, mono;
    explicit BatchAll(size_t cap) : kps(kFrames * cap), desc(32 * kFrames * cap), counts(kFrames), mono(kFrames) {}
};

int monocular_part(orbx_extractor *ex, const std::vector<uint8_t> &img) {
    const int cap_i = orbx_output_capacity(ex, kW, kH);
    CHECK(cap_i > 0);
    const size_t cap = (size_t)cap_i;
    BatchAll full(cap);
    MUST(orbx_batch_download_all(ex, full.kps.get(), full.desc.get(), full.counts.get(), full.mono.get()));
    {   // every output alone
        BatchAll a(cap), b(cap), c(cap), d(cap);
        MUST(orbx_batch_download_all(ex, a.kps.get(), nullptr, nullptr, nullptr));
        MUST(orbx_batch_download_all(ex, nullptr, b.desc.get(), nullptr, nullptr));
        MUST(orbx_batch_download_all(ex, nullptr, nullptr, c.counts.get(), nullptr));
        MUST(orbx_batch_download_all(ex, nullptr, nullptr, nullptr, d.mono.get()));
        CHECK(same(a.kps, full.kps) && a.desc.untouched() && a.counts.untouched() && a.mono.untouched());
        CHECK(same(b.desc, full.desc) && b.kps.untouched() && b.counts.untouched() && b.mono.untouched());
        CHECK(same(c.counts, full.counts) && c.kps.untouched() && c.desc.untouched() && c.mono.untouched());
        CHECK(same(d.mono, full.mono) && d.kps.untouched() && d.desc.untouched() && d.counts.untouched());
    }
    int total = 0;
    for (int f = 0; f < kFrames; f++) {
        const int n = full.counts.get()[f];
        CHECK(n >= 0 && n <= cap_i && (f == kFlat ? n == 0 : n > 100));
        total += n;
        {   // exactly n rows: the frame's rows of the full download
            Block<orbx_keypoint> kps((size_t)n), kun((size_t)n);
            Block<uint8_t> desc(32 * (size_t)n);
            int got = -1, mono = -1, got_un = -1;
            MUST(orbx_batch_download(ex, f, kps.get(), desc.get(), n, &got, &mono));
            CHECK(got == n && mono == full.mono.get()[f]);
            CHECK(same_row(kps, full.kps, f * cap) && same_row(desc, full.desc, 32 * f * cap));
            MUST(orbx_batch_download_keypoints_un(ex, f, kun.get(), n, &got_un));   // no camera is set: mvKeysUn = mvKeys
            CHECK(got_un == n && same(kun, kps));
        }
        if (n > 0) {   // one row short: refused, the count still reported, nothing written
            Block<orbx_keypoint> kps((size_t)n - 1);
            Block<uint8_t> desc(32 * ((size_t)n - 1));
            int got = -1, mono = -1;
            CHECK(orbx_batch_download(ex, f, kps.get(), desc.get(), n - 1, &got, &mono) == ORBX_E_CAPACITY);
            CHECK(got == n && kps.untouched() && desc.untouched());
        } else {       // the flat frame: room offered, none used
            Block<orbx_keypoint> kps(4);
            Block<uint8_t> desc(32 * 4);
            int got = -1, mono = -1;
            MUST(orbx_batch_download(ex, f, kps.get(), desc.get(), 4, &got, &mono));
            CHECK(got == 0 && kps.untouched() && desc.untouched());
        }
    }
    // orbx_get_level: a destination whose stride is the padded width, so that the last row's block ends at the destination's last byte
    for (int level : {0, kLevels - 1}) {
        int w = 0, h = 0;
        MUST(orbx_level_size(ex, kW, kH, level, &w, &h));
        const size_t pw = (size_t)w + 38, ph = (size_t)h + 38;
        for (int f : {0, kFrames - 1}) {
            Block<uint8_t> tight(pw * ph), wide((pw + 7) * ph);
            MUST(orbx_get_level(ex, f, level, tight.get(), pw));
            MUST(orbx_get_level(ex, f, level, wide.get(), pw + 7));
            for (size_t y = 0; y < ph; y++) {
                CHECK(memcmp(tight.get() + y * pw, wide.get() + y * (pw + 7), pw) == 0);
                for (size_t x = pw; x < pw + 7; x++) CHECK(wide.get()[y * (pw + 7) + x] == kFill);
            }
            if (level == 0)   // level 0 is the frame inside its ring of 19 pixels
                for (int y = 0; y < kH; y++) CHECK(memcmp(tight.get() + ((size_t)y + 19) * pw + 19, &img[((size_t)f * kH + y) * kW], kW) == 0);
        }
    }
    // orbx_debug_level_keypoints: the count whatever room is offered
    int listed = 0;
    for (int level : {0, kLevels - 1}) {
        const int n = orbx_debug_level_keypoints(ex, 0, level, nullptr, 0);
        CHECK(n >= 0);
        Block<orbx_keypoint> out((size_t)n);
        CHECK(orbx_debug_level_keypoints(ex, 0, level, out.get(), n) == n);
        for (int i = 0; i < n; i++) CHECK(out.get()[i].octave == level);
        CHECK(orbx_debug_level_keypoints(ex, kFlat, level, nullptr, 0) == 0);
        listed += n;
    }
    CHECK(listed > 0);
    printf("extractor downloads: %d features on %d frames, capacity %d\n", total, kFrames, cap_i);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// the rectified stage's and the RGB-D stages' results (one set of result buffers on the left extractor)
// ---------------------------------------------------------------------------------------------------------
struct StereoAll {
    Block<float> ur, depth;
    Block<int32_t> nm;
    explicit StereoAll(size_t cap) : ur(kFrames * cap), depth(kFrames * cap), nm(kFrames) {}
};
bool same(const StereoAll &a, const StereoAll &b) { return same(a.ur, b.ur) && same(a.depth, b.depth) && same(a.nm, b.nm); }

int stereo_downloads(orbx_extractor *L, size_t cap, StereoAll &full, int *with_depth) {
    MUST(orbx_stereo_batch_download_all(L, full.ur.get(), full.depth.get(), full.nm.get()));
    StereoAll a(cap), b(cap), c(cap);
    MUST(orbx_stereo_batch_download_all(L, a.ur.get(), nullptr, nullptr));
    MUST(orbx_stereo_batch_download_all(L, nullptr, b.depth.get(), nullptr));
    MUST(orbx_stereo_batch_download_all(L, nullptr, nullptr, c.nm.get()));
    CHECK(same(a.ur, full.ur) && a.depth.untouched() && a.nm.untouched());
    CHECK(same(b.depth, full.depth) && b.ur.untouched() && b.nm.untouched());
    CHECK(same(c.nm, full.nm) && c.ur.untouched() && c.depth.untouched());
    *with_depth = 0;
    for (int f = 0; f < kFrames; f++) {
        int n_left = -1, n_matches = -1;
        MUST(orbx_stereo_batch_download(L, f, nullptr, nullptr, &n_left, &n_matches));
        CHECK(n_left >= 0 && (size_t)n_left <= cap && (f == kFlat) == (n_left == 0) && n_matches == full.nm.get()[f]);
        Block<float> ur((size_t)n_left), depth((size_t)n_left), alone((size_t)n_left);
        int n2 = -1, m2 = -1;
        MUST(orbx_stereo_batch_download(L, f, ur.get(), depth.get(), &n2, &m2));
        CHECK(n2 == n_left && m2 == n_matches && same_row(ur, full.ur, f * cap) && same_row(depth, full.depth, f * cap));
        MUST(orbx_stereo_batch_download(L, f, nullptr, alone.get(), nullptr, nullptr));
        CHECK(same(alone, depth));
        *with_depth += n_matches;
    }
    return 0;
}

int rectified_part(orbx_extractor *L, orbx_extractor *R) {
    const size_t cap = (size_t)orbx_output_capacity(L, kW, kH);
    MUST(orbx_stereo_batch_device(L, R, 40.f, 0.1f));
    StereoAll full(cap);
    int matched = 0;
    if (stereo_downloads(L, cap, full, &matched)) return 1;
    CHECK(matched > 0 && full.nm.get()[kFlat] == 0);
    printf("rectified stage: %d matches\n", matched);
    return 0;
}

int rgbd_part(orbx_extractor *L, const std::vector<uint8_t> &img_a, const std::vector<uint8_t> &img_b) {
    const size_t cap = (size_t)orbx_output_capacity(L, kW, kH);
    // the same depth values as floats and as the sensor's 16-bit integers (factor 1: no rounding), holes of zeros, garbage in the row padding
    const int pf = kW + 5, pu = kW + 3;
    Block<float> df((size_t)kFrames * kH * pf);
    Block<uint16_t> du((size_t)kFrames * kH * pu);
    for (int f = 0; f < kFrames; f++)
        for (int y = 0; y < kH; y++)
            for (int x = 0; x < kW; x++) {
                const uint16_t d = x >= 40 && x < 70 ? 0 : (uint16_t)(1 + (x + 3 * y + 7 * f) % 4000);
                df.get()[((size_t)f * kH + y) * pf + x] = (float)d;
                du.get()[((size_t)f * kH + y) * pu + x] = d;
            }
    const float bf = 40.f;
    auto float_stage = [&] { return orbx_rgbd_batch_device(L, df.get(), 4 * (size_t)pf, 4 * (size_t)pf * kH, bf); };
    auto u16_stage = [&] { return orbx_rgbd_batch_device_u16(L, du.get(), 2 * (size_t)pu, 2 * (size_t)pu * kH, 1.0f, bf); };
    int with_f = 0, with_u = 0;
    StereoAll first_f(cap), first_u(cap);
    MUST(float_stage());
    if (stereo_downloads(L, cap, first_f, &with_f)) return 1;
    MUST(u16_stage());
    if (stereo_downloads(L, cap, first_u, &with_u)) return 1;
    CHECK(with_f > 100 && with_f == with_u && same(first_f, first_u));
    // the results leave asynchronously, a second batch is extracted and its stage overwrites the buffers the copy reads: it waits for the copy
    StereoAll async(cap), second_f(cap), second_u(cap);
    MUST(orbx_stereo_batch_download_async(L, async.ur.get(), async.depth.get(), async.nm.get()));
    if (extract(L, img_b)) return 1;
    MUST(float_stage());
    MUST(orbx_stereo_download_wait(L));
    CHECK(same(async, first_u));
    MUST(orbx_stereo_batch_download_all(L, second_f.ur.get(), second_f.depth.get(), second_f.nm.get()));
    MUST(orbx_stereo_batch_download_async(L, async.ur.get(), async.depth.get(), async.nm.get()));
    MUST(orbx_stereo_download_wait(L));
    CHECK(same(async, second_f));
    MUST(u16_stage());
    MUST(orbx_stereo_batch_download_all(L, second_u.ur.get(), second_u.depth.get(), second_u.nm.get()));
    CHECK(same(second_f, second_u) && !same(second_f.nm, first_f.nm));
    if (extract(L, img_a)) return 1;   // the batch the other parts expect
    printf("rgbd stages: %d features with depth, float and 16-bit forms equal on two batches\n", with_f);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// the fisheye stage's results
// ---------------------------------------------------------------------------------------------------------
struct FisheyeAll {
    Block<int32_t> l2r, r2l;
    Block<float> depth, p3d;
    Block<int32_t> nm, dm;
    FisheyeAll(size_t cl, size_t cr) : l2r(kFrames * cl), r2l(kFrames * cr), depth(kFrames * cl), p3d(3 * kFrames * cl), nm(kFrames), dm(kFrames) {}
    int others_untouched(const void *but) const {
        return (l2r.get() == but || l2r.untouched()) && (r2l.get() == but || r2l.untouched()) && (depth.get() == but || depth.untouched()) &&
               (p3d.get() == but || p3d.untouched()) && (nm.get() == but || nm.untouched()) && (dm.get() == but || dm.untouched());
    }
};

int fisheye_part(orbx_extractor *L, orbx_extractor *R) {
    const size_t cl = (size_t)orbx_output_capacity(L, kW, kH), cr = (size_t)orbx_output_capacity(R, kW, kH);
    const float tumvi[8] = {190.978477f, 190.973307f, 254.931706f, 256.897442f, 0.0034823894f, 0.0007150348f, -0.0020532361f, 0.0002029367f};
    orbx_kb8_rig rig;
    memcpy(rig.cam_left, tumvi, sizeof(tumvi)); memcpy(rig.cam_right, tumvi, sizeof(tumvi));
    const float eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, base[3] = {0.1f, 0.f, 0.f};
    memcpy(rig.R_lr, eye, sizeof(eye)); memcpy(rig.t_lr, base, sizeof(base));
    MUST(orbx_stereo_fisheye_batch_device(L, R, &rig));
    FisheyeAll full(cl, cr);
    MUST(orbx_stereo_fisheye_batch_download_all(L, full.l2r.get(), full.r2l.get(), full.depth.get(), full.p3d.get(), full.nm.get(), full.dm.get()));
    {   // every output alone
        FisheyeAll a(cl, cr), b(cl, cr), c(cl, cr), d(cl, cr), e(cl, cr), g(cl, cr);
        MUST(orbx_stereo_fisheye_batch_download_all(L, a.l2r.get(), nullptr, nullptr, nullptr, nullptr, nullptr));
        MUST(orbx_stereo_fisheye_batch_download_all(L, nullptr, b.r2l.get(), nullptr, nullptr, nullptr, nullptr));
        MUST(orbx_stereo_fisheye_batch_download_all(L, nullptr, nullptr, c.depth.get(), nullptr, nullptr, nullptr));
        MUST(orbx_stereo_fisheye_batch_download_all(L, nullptr, nullptr, nullptr, d.p3d.get(), nullptr, nullptr));
        MUST(orbx_stereo_fisheye_batch_download_all(L, nullptr, nullptr, nullptr, nullptr, e.nm.get(), nullptr));
        MUST(orbx_stereo_fisheye_batch_download_all(L, nullptr, nullptr, nullptr, nullptr, nullptr, g.dm.get()));
        CHECK(same(a.l2r, full.l2r) && a.others_untouched(a.l2r.get()));
        CHECK(same(b.r2l, full.r2l) && b.others_untouched(b.r2l.get()));
        CHECK(same(c.depth, full.depth) && c.others_untouched(c.depth.get()));
        CHECK(same(d.p3d, full.p3d) && d.others_untouched(d.p3d.get()));
        CHECK(same(e.nm, full.nm) && e.others_untouched(e.nm.get()));
        CHECK(same(g.dm, full.dm) && g.others_untouched(g.dm.get()));
    }
    int matched = 0, by_descriptor = 0;
    for (int f = 0; f < kFrames; f++) {
        int nl = -1, nr = -1, nm = -1, dm = -1;
        MUST(orbx_stereo_fisheye_batch_download(L, f, nullptr, nullptr, nullptr, nullptr, &nl, &nr, &nm, &dm));
        CHECK(nl >= 0 && (size_t)nl <= cl && nr >= 0 && (size_t)nr <= cr && (f == kFlat) == (nl == 0) && nm == full.nm.get()[f] && dm == full.dm.get()[f]);
        Block<int32_t> l2r((size_t)nl), r2l((size_t)nr), r2l_alone((size_t)nr);
        Block<float> depth((size_t)nl), p3d(3 * (size_t)nl), p3d_alone(3 * (size_t)nl);
        int nl2 = -1, nr2 = -1;
        MUST(orbx_stereo_fisheye_batch_download(L, f, l2r.get(), r2l.get(), depth.get(), p3d.get(), &nl2, &nr2, nullptr, nullptr));
        CHECK(nl2 == nl && nr2 == nr);
        CHECK(same_row(l2r, full.l2r, f * cl) && same_row(r2l, full.r2l, f * cr) && same_row(depth, full.depth, f * cl) && same_row(p3d, full.p3d, 3 * f * cl));
        MUST(orbx_stereo_fisheye_batch_download(L, f, nullptr, r2l_alone.get(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        MUST(orbx_stereo_fisheye_batch_download(L, f, nullptr, nullptr, nullptr, p3d_alone.get(), nullptr, nullptr, nullptr, nullptr));
        CHECK(same(r2l_alone, r2l) && same(p3d_alone, p3d));
        matched += nm; by_descriptor += dm;
    }
    CHECK(by_descriptor > 0 && matched <= by_descriptor);
    printf("fisheye stage: %d descriptor matches, %d triangulated\n", by_descriptor, matched);
    return 0;
}

}  // namespace

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const std::vector<uint8_t> img = make_images(0, 5), img_l = make_images(4, 5), img_r = make_images(1, 5), img_l2 = make_images(9, 6);
    orbx_extractor *ex = nullptr, *exl = nullptr, *exr = nullptr;
    if (make_extractor(img, &ex) || make_extractor(img_l, &exl) || make_extractor(img_r, &exr)) return 1;
    if (monocular_part(ex, img)) return 1;
    if (rectified_part(exl, exr)) return 1;
    if (rgbd_part(exl, img_l, img_l2)) return 1;
    if (fisheye_part(exl, exr)) return 1;
    orbx_destroy(ex); orbx_destroy(exl); orbx_destroy(exr);
    printf("staged downloads ok\n");
    return 0;
}
