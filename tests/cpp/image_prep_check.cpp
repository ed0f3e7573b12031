// Raw sensor images on the device: orbx_rectify_batch_device against cv::remap(src, dst, map1, map2, INTER_LINEAR) for 8-bit one-channel images as
// include/orbx.h restates it, and orbx_rgbd_batch_device_u16 against convertTo + Frame::ComputeStereoFromRGBD, both written out below.
// Every image buffer is a heap block of exactly the bytes the call may touch: a tap read past the source's last pixel or a dword stored past the
// destination's last byte ends the run.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt, whose
// stand-in runtime takes any host pointer as device memory) and compiled with -fsanitize=address,undefined.  Prints "image prep ok", returns 0.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

#define MUST(expr)                                                                   \
    do {                                                                             \
        const int r_ = (expr);                                                       \
        if (r_ < 0) { printf("%s: %d %s\n", #expr, r_, orbx_last_error()); return 1; } \
    } while (0)
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

// cvRound(v * 32): nearest, ties to even (the default rounding mode), INT_MIN outside int
long long fixed(float v) {
    const double p = (double)v * 32.0;
    if (!(p >= -2147483648.0 && p < 2147483648.0)) return INT_MIN;
    return (long long)std::nearbyint(p);
}
long long saturate_short(long long v) { return std::min(32767LL, std::max(-32768LL, v)); }

uint8_t remap_pixel(const uint8_t *src, int sw, int sh, size_t stride, float mx, float my) {
    const long long sx = fixed(mx), sy = fixed(my);
    const long long a = sx & 31, b = sy & 31, ix = saturate_short(sx >> 5), iy = saturate_short(sy >> 5);
    auto tap = [&](long long x, long long y) -> long long { return x >= 0 && x < sw && y >= 0 && y < sh ? src[(size_t)y * stride + (size_t)x] : 0; };
    const long long sum = tap(ix, iy) * ((32 - a) * (32 - b) * 32) + tap(ix + 1, iy) * (a * (32 - b) * 32) + tap(ix, iy + 1) * ((32 - a) * b * 32) +
                          tap(ix + 1, iy + 1) * (a * b * 32);
    return (uint8_t)((sum + 16384) >> 15);
}

// a distortion field with designed entries sprinkled in: the image's last pixel and its neighbours, the borders, what saturates, what is not finite
void make_maps(int dw, int dh, int sw, int sh, std::vector<float> &mx, std::vector<float> &my) {
    const float special_x[] = {(float)(sw - 1), (float)(sw - 2) + 0.5f, (float)sw - 1.f / 64.f, (float)sw, -1.f, -1.f / 64.f, -0.5f, 40000.f, -40000.f,
                               67108864.f, -67108864.f, 1e12f, -INFINITY, INFINITY, NAN, 0.f};
    const float special_y[] = {(float)(sh - 1), (float)(sh - 2) + 0.75f, (float)sh - 1.f / 64.f, (float)sh, -1.f, -0.25f, NAN, (float)(sh - 1), 3e38f, 0.f};
    mx.assign((size_t)dw * dh, 0.f); my.assign((size_t)dw * dh, 0.f);
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            const int p = y * dw + x;
            const float xn = ((float)x - 0.5f * (float)(dw - 1)) / (0.62f * (float)dw), yn = ((float)y - 0.5f * (float)(dh - 1)) / (0.62f * (float)dw);
            const float r2 = xn * xn + yn * yn, rad = 1.f - 0.28f * r2 + 0.07f * r2 * r2;
            float u = 0.85f * (float)sw * xn * rad + 0.5f * (float)(sw - 1) + 0.3f, v = 0.85f * (float)sw * yn * rad + 0.5f * (float)(sh - 1) - 0.2f;
            if (p % 3 == 1) u = special_x[(p / 3) % 16];
            if (p % 5 == 2) v = special_y[(p / 5) % 10];
            mx[p] = u; my[p] = v;
        }
}

int rectify_part(int dw, int dh, int n, size_t dst_offset) {
    const int sw = 61, sh = 17;
    std::mt19937 rng(7 + dw);
    std::unique_ptr<uint8_t[]> src(new uint8_t[(size_t)n * sw * sh]);   // packed: the last frame's last pixel is the block's last byte
    for (size_t i = 0; i < (size_t)n * sw * sh; i++) src[i] = (uint8_t)(1 + rng() % 255);
    const size_t dst_bytes = dst_offset + (size_t)n * dw * dh;
    std::unique_ptr<uint8_t[]> dst(new uint8_t[dst_bytes]);
    memset(dst.get(), 0xa5, dst_bytes);
    std::vector<float> mx, my;
    make_maps(dw, dh, sw, sh, mx, my);
    orbx_rectifier *r = nullptr;
    MUST(orbx_rectifier_create(0, mx.data(), my.data(), dw, dh, (size_t)dw, &r));
    const orbx_params prm = {500, 1.2f, 8, 20, 7, 0};
    orbx_extractor *ex = nullptr;
    MUST(orbx_create(&prm, 0, 0, 0, 0, &ex));
    CHECK(orbx_rectify_batch_device(r, ex, src.get(), n, sw, sh, (size_t)sw - 1, (size_t)sw * sh, dst.get() + dst_offset, (size_t)dw, (size_t)dw * dh) == ORBX_E_BAD_ARG);
    CHECK(orbx_rectify_batch_device(r, ex, src.get(), n, sw, sh, (size_t)sw, (size_t)sw * sh, src.get() + 5, (size_t)dw, (size_t)dw * dh) == ORBX_E_BAD_ARG);
    CHECK(orbx_rectify_batch_device(r, ex, src.get(), 0, sw, sh, (size_t)sw, (size_t)sw * sh, dst.get() + dst_offset, (size_t)dw, (size_t)dw * dh) == ORBX_E_BAD_ARG);
    for (size_t i = 0; i < dst_bytes; i++) CHECK(dst[i] == 0xa5);
    MUST(orbx_rectify_batch_device(r, ex, src.get(), n, sw, sh, (size_t)sw, (size_t)sw * sh, dst.get() + dst_offset, (size_t)dw, (size_t)dw * dh));
    MUST(orbx_sync(ex));
    int zeros = 0;
    for (size_t i = 0; i < dst_offset; i++) CHECK(dst[i] == 0xa5);
    for (int f = 0; f < n; f++)
        for (int y = 0; y < dh; y++)
            for (int x = 0; x < dw; x++) {
                const uint8_t want = remap_pixel(src.get() + (size_t)f * sw * sh, sw, sh, (size_t)sw, mx[(size_t)y * dw + x], my[(size_t)y * dw + x]);
                const uint8_t got = dst[dst_offset + ((size_t)f * dh + y) * dw + x];
                if (got != want) { printf("FAILED: frame %d (%d, %d): %d, expected %d (map %g, %g)\n", f, x, y, got, want, mx[(size_t)y * dw + x], my[(size_t)y * dw + x]); return 1; }
                zeros += want == 0;
            }
    if (dw >= 64) CHECK(zeros > n * dw * dh / 8 && zeros < n * dw * dh * 3 / 4);   // both kinds of pixel in numbers
    orbx_rectifier_destroy(r);
    orbx_destroy(ex);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// the 16-bit depth image on an extracted batch
// ---------------------------------------------------------------------------------------------------------
constexpr int kW = 320, kH = 240, kFrames = 2;

std::vector<uint8_t> make_images() {
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
            for (int x = 0; x < kW; x++) img[((size_t)f * kH + y) * kW + x] = (uint8_t)std::min(255, std::max(0, canvas[(size_t)(y + 2 * f) * cw + x + 3 * f]));
    return img;
}

int depth_part() {
    const std::vector<uint8_t> img = make_images();
    const orbx_params prm = {500, 1.2f, 8, 20, 7, 0};
    orbx_extractor *ex = nullptr;
    MUST(orbx_create(&prm, 0, kW, kH, kFrames, &ex));
    orbx_camera cam;
    memset(&cam, 0, sizeof(cam));
    cam.fx = 265.f; cam.fy = 262.f; cam.cx = 161.5f; cam.cy = 118.25f; cam.k1 = -0.28f; cam.k2 = 0.07f; cam.bf = 40.f;
    MUST(orbx_set_camera(ex, &cam));
    MUST(orbx_extract_batch_host(ex, img.data(), kFrames, kW, kH, kW, (size_t)kW * kH, 0, 0));
    // rows of exactly kW values (the pitch is the row): the last row's last value is the block's last
    const size_t pitch = 2 * (size_t)kW, frame_stride = pitch * kH;
    std::unique_ptr<uint16_t[]> raw(new uint16_t[(size_t)kFrames * kH * kW]);
    for (int f = 0; f < kFrames; f++)
        for (int y = 0; y < kH; y++)
            for (int x = 0; x < kW; x++) {
                uint16_t d = (uint16_t)(300 + (x * 131 + y * 71 + 1000 * f) % 65000);
                if ((x / 16 + y / 16) % 5 == 0) d = 0;
                else if ((x + y) % 97 == 0) d = 65535;
                else if ((x + y) % 89 == 0) d = 1;
                raw[((size_t)f * kH + y) * kW + x] = d;
            }
    const float bf = 40.f, factor = 1.0f / 5000.0f;
    CHECK(orbx_rgbd_batch_device_u16(ex, raw.get(), pitch - 2, frame_stride, factor, bf) == ORBX_E_BAD_ARG);
    CHECK(orbx_rgbd_batch_device_u16(ex, raw.get(), pitch + 1, frame_stride, factor, bf) == ORBX_E_BAD_ARG);
    CHECK(orbx_rgbd_batch_device_u16(ex, raw.get(), pitch, frame_stride, 0.f, bf) == ORBX_E_BAD_ARG);
    CHECK(orbx_rgbd_batch_device_u16(ex, raw.get(), pitch, frame_stride, INFINITY, bf) == ORBX_E_BAD_ARG);
    CHECK(orbx_rgbd_batch_device_u16(ex, nullptr, pitch, frame_stride, factor, bf) == ORBX_E_BAD_ARG);
    MUST(orbx_rgbd_batch_device_u16(ex, raw.get(), pitch, frame_stride, factor, bf));
    const int cap = orbx_output_capacity(ex, kW, kH);
    CHECK(cap > 0);
    for (int f = 0; f < kFrames; f++) {
        std::vector<orbx_keypoint> kps((size_t)cap), kun((size_t)cap);
        std::vector<uint8_t> desc(32 * (size_t)cap);
        std::vector<float> ur((size_t)cap), dep((size_t)cap);
        int n = 0, mono = 0, n_un = 0, n_left = 0, n_with = 0, want_with = 0;
        MUST(orbx_batch_download(ex, f, kps.data(), desc.data(), cap, &n, &mono));
        MUST(orbx_batch_download_keypoints_un(ex, f, kun.data(), cap, &n_un));
        MUST(orbx_stereo_batch_download(ex, f, ur.data(), dep.data(), &n_left, &n_with));
        CHECK(n > 100 && n_un == n && n_left == n);
        for (int i = 0; i < n; i++) {
            const float d = (float)raw[((size_t)f * kH + (int)kps[i].y) * kW + (int)kps[i].x] * factor;   // convertTo: one rounded product
            const float wd = d > 0 ? d : -1.f, wu = d > 0 ? kun[i].x - bf / d : -1.f;
            CHECK(memcmp(&wd, &dep[i], 4) == 0 && memcmp(&wu, &ur[i], 4) == 0);
            want_with += d > 0;
        }
        CHECK(n_with == want_with && want_with > n / 2 && want_with < n);
    }
    orbx_destroy(ex);
    return 0;
}

}  // namespace

int main() {
    // destination widths around the four-pixel group and a multiple of four, 1, 3 and 5 frames (chunks of four), rows at every alignment
    const int shapes[][4] = {{67, 13, 5, 0}, {67, 13, 3, 1}, {64, 13, 5, 0}, {64, 9, 1, 3}, {1, 13, 3, 0}, {3, 5, 1, 2}, {5, 13, 5, 0}, {65, 4, 3, 0}};
    for (const auto &s : shapes)
        if (rectify_part(s[0], s[1], s[2], (size_t)s[3])) { printf("FAILED: shape %d x %d, %d frames, offset %d\n", s[0], s[1], s[2], s[3]); return 1; }
    if (depth_part()) return 1;
    printf("image prep ok\n");
    return 0;
}
