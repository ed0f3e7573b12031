// Colour, size and contrast of raw frames on the device: orbx_gray_batch_device, orbx_resize_batch_device and orbx_clahe_batch_device against cvtColor,
// cv::resize (INTER_LINEAR) and cv::CLAHE::apply for 8-bit images as include/orbx.h restates them, written out below.
// Every image buffer is a heap block of exactly the bytes the call may touch (packed rows, the last frame's last pixel is the block's last byte, the
// first pixel sits `offset` bytes into its block): a read past a source row's last pixel, a dword stored past the destination's last byte or a
// reflected coordinate outside the image ends the run.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt, whose
// stand-in runtime takes any host pointer as device memory) and compiled with -fsanitize=address,undefined.  Prints "image enhance ok", returns 0.
#include <algorithm>
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

struct Block {   // `offset` bytes of 0xa5, then exactly `bytes` bytes
    std::unique_ptr<uint8_t[]> mem;
    size_t offset, bytes;
    Block(size_t offset_, size_t bytes_) : mem(new uint8_t[offset_ + bytes_]), offset(offset_), bytes(bytes_) { memset(mem.get(), 0xa5, offset + bytes); }
    uint8_t *p() { return mem.get() + offset; }
    bool head_untouched() const { for (size_t i = 0; i < offset; i++) if (mem[i] != 0xa5) return false; return true; }
    bool untouched() const { for (size_t i = 0; i < offset + bytes; i++) if (mem[i] != 0xa5) return false; return true; }
};

int compare(const uint8_t *got, const std::vector<uint8_t> &want, const char *what) {
    for (size_t i = 0; i < want.size(); i++)
        if (got[i] != want[i]) { printf("FAILED: %s byte %zu: %d, expected %d\n", what, i, got[i], want[i]); return 1; }
    return 0;
}

// ---- cvtColor ----
int gray_part(orbx_extractor *ex, int w, int h, int n, int channels, int rgb, size_t s_off, size_t d_off) {
    std::mt19937 rng(3 + w + channels);
    Block src(s_off, (size_t)n * w * h * channels), dst(d_off, (size_t)n * w * h);
    for (size_t i = 0; i < src.bytes; i++) src.p()[i] = (uint8_t)(rng() % 256);
    std::vector<uint8_t> want(dst.bytes);
    for (size_t i = 0; i < want.size(); i++) {
        const uint8_t *px = src.p() + i * channels;
        const int r = rgb ? px[0] : px[2], b = rgb ? px[2] : px[0];
        want[i] = (uint8_t)((r * 9798 + px[1] * 19235 + b * 3735 + 16384) >> 15);
    }
    const size_t srs = (size_t)w * channels, sfs = srs * h, drs = (size_t)w, dfs = drs * h;
    CHECK(orbx_gray_batch_device(ex, src.p(), n, w, h, 2, rgb, srs, sfs, dst.p(), drs, dfs) == ORBX_E_BAD_ARG);
    CHECK(orbx_gray_batch_device(ex, src.p(), n, w, h, channels, rgb, srs - 1, sfs, dst.p(), drs, dfs) == ORBX_E_BAD_ARG);
    CHECK(orbx_gray_batch_device(ex, src.p(), n, w, h, channels, rgb, srs, sfs, src.p() + 1, drs, dfs) == ORBX_E_BAD_ARG);
    CHECK(dst.untouched());
    MUST(orbx_gray_batch_device(ex, src.p(), n, w, h, channels, rgb, srs, sfs, dst.p(), drs, dfs));
    MUST(orbx_sync(ex));
    CHECK(dst.head_untouched());
    return compare(dst.p(), want, "gray");
}

// ---- cv::resize ----
struct Tab { std::vector<int> ofs, c0, c1; };
Tab linear_tab(int ssize, int dsize, bool horizontal) {
    Tab t;
    const double inv_scale = (double)dsize / ssize, scale = 1. / inv_scale;
    for (int d = 0; d < dsize; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= (float)s;
        if (horizontal) {
            if (s < 0) { f = 0; s = 0; }
            if (s >= ssize - 1) { f = 0; s = ssize - 1; }
        }
        t.ofs.push_back(s);
        t.c0.push_back((int)std::min(32767L, std::max(-32768L, std::lrint((1.f - f) * 2048.f))));
        t.c1.push_back((int)std::min(32767L, std::max(-32768L, std::lrint(f * 2048.f))));
    }
    return t;
}
void resize_reference(const uint8_t *src, int sw, int sh, uint8_t *dst, int dw, int dh) {
    if (sw == 2 * dw && sh == 2 * dh) {
        for (int y = 0; y < dh; y++)
            for (int x = 0; x < dw; x++) {
                const uint8_t *p = src + (size_t)(2 * y) * sw + 2 * x;
                dst[(size_t)y * dw + x] = (uint8_t)((p[0] + p[1] + p[sw] + p[sw + 1] + 2) >> 2);
            }
        return;
    }
    const Tab tx = linear_tab(sw, dw, true), ty = linear_tab(sh, dh, false);
    for (int y = 0; y < dh; y++) {
        const int sy0 = std::min(std::max(ty.ofs[y], 0), sh - 1), sy1 = std::min(std::max(ty.ofs[y] + 1, 0), sh - 1);
        for (int x = 0; x < dw; x++) {
            const int sx = tx.ofs[x];
            int r[2];
            for (int k = 0; k < 2; k++) {
                const uint8_t *S = src + (size_t)(k ? sy1 : sy0) * sw;
                r[k] = sx + 1 < sw ? S[sx] * tx.c0[x] + S[sx + 1] * tx.c1[x] : S[sx] * 2048;
            }
            const int v = (((ty.c0[y] * (r[0] >> 4)) >> 16) + ((ty.c1[y] * (r[1] >> 4)) >> 16) + 2) >> 2;
            dst[(size_t)y * dw + x] = (uint8_t)std::min(std::max(v, 0), 255);
        }
    }
}
int resize_part(orbx_extractor *ex, int sw, int sh, int dw, int dh, int n, size_t s_off, size_t d_off) {
    std::mt19937 rng(5 + sw + dw);
    Block src(s_off, (size_t)n * sw * sh), dst(d_off, (size_t)n * dw * dh);
    for (size_t i = 0; i < src.bytes; i++) src.p()[i] = (uint8_t)(rng() % 256);
    std::vector<uint8_t> want(dst.bytes);
    for (int f = 0; f < n; f++) resize_reference(src.p() + (size_t)f * sw * sh, sw, sh, want.data() + (size_t)f * dw * dh, dw, dh);
    CHECK(orbx_resize_batch_device(ex, src.p(), n, sw, sh, (size_t)sw, (size_t)sw * sh, dst.p(), 0, dh, (size_t)dw, (size_t)dw * dh) == ORBX_E_BAD_ARG);
    CHECK(orbx_resize_batch_device(ex, src.p(), n, sw, sh, (size_t)sw, (size_t)sw * sh, dst.p(), dw, dh, (size_t)dw - 1, (size_t)dw * dh) == ORBX_E_BAD_ARG);
    CHECK(dst.untouched());
    MUST(orbx_resize_batch_device(ex, src.p(), n, sw, sh, (size_t)sw, (size_t)sw * sh, dst.p(), dw, dh, (size_t)dw, (size_t)dw * dh));
    MUST(orbx_sync(ex));
    CHECK(dst.head_untouched());
    return compare(dst.p(), want, "resize");
}

// ---- cv::CLAHE::apply ----
int reflect101(int p, int len) { return p < len ? p : 2 * (len - 1) - p; }
void clahe_reference(const uint8_t *src, int w, int h, double clip_limit, int tiles_x, int tiles_y, uint8_t *dst) {
    int pad_x = 0, pad_y = 0;
    if (w % tiles_x != 0 || h % tiles_y != 0) { pad_x = tiles_x - w % tiles_x; pad_y = tiles_y - h % tiles_y; }
    const int tile_w = (w + pad_x) / tiles_x, tile_h = (h + pad_y) / tiles_y, area = tile_w * tile_h;
    const int clip = clip_limit > 0 ? std::max((int)(clip_limit * area / 256), 1) : 0;
    const float lut_scale = 255.0f / (float)area;
    std::vector<uint8_t> lut((size_t)tiles_x * tiles_y * 256);
    for (int ty = 0; ty < tiles_y; ty++)
        for (int tx = 0; tx < tiles_x; tx++) {
            int hist[256] = {0};
            for (int y = ty * tile_h; y < (ty + 1) * tile_h; y++)
                for (int x = tx * tile_w; x < (tx + 1) * tile_w; x++) hist[src[(size_t)reflect101(y, h) * w + reflect101(x, w)]]++;
            if (clip > 0) {
                int clipped = 0;
                for (int i = 0; i < 256; i++)
                    if (hist[i] > clip) { clipped += hist[i] - clip; hist[i] = clip; }
                const int batch = clipped / 256;
                int residual = clipped - batch * 256;
                for (int i = 0; i < 256; i++) hist[i] += batch;
                if (residual != 0) {
                    const int step = std::max(256 / residual, 1);
                    for (int i = 0; i < 256 && residual > 0; i += step, residual--) hist[i]++;
                }
            }
            int sum = 0;
            for (int i = 0; i < 256; i++) {
                sum += hist[i];
                const long v = std::lrint((float)sum * lut_scale);
                lut[((size_t)ty * tiles_x + tx) * 256 + i] = (uint8_t)std::min(255L, std::max(0L, v));
            }
        }
    const float inv_tw = 1.0f / (float)tile_w, inv_th = 1.0f / (float)tile_h;
    for (int y = 0; y < h; y++) {
        const float tyf = (float)y * inv_th - 0.5f;
        int ty1 = (int)std::floor(tyf), ty2 = ty1 + 1;
        const float ya = tyf - (float)ty1, ya1 = 1.0f - ya;
        ty1 = std::max(ty1, 0); ty2 = std::min(ty2, tiles_y - 1);
        for (int x = 0; x < w; x++) {
            const float txf = (float)x * inv_tw - 0.5f;
            int tx1 = (int)std::floor(txf), tx2 = tx1 + 1;
            const float xa = txf - (float)tx1, xa1 = 1.0f - xa;
            tx1 = std::max(tx1, 0); tx2 = std::min(tx2, tiles_x - 1);
            const int v = src[(size_t)y * w + x];
            const float l11 = lut[((size_t)ty1 * tiles_x + tx1) * 256 + v], l12 = lut[((size_t)ty1 * tiles_x + tx2) * 256 + v];
            const float l21 = lut[((size_t)ty2 * tiles_x + tx1) * 256 + v], l22 = lut[((size_t)ty2 * tiles_x + tx2) * 256 + v];
            const float top = l11 * xa1 + l12 * xa, bot = l21 * xa1 + l22 * xa;
            const float res = top * ya1 + bot * ya;
            dst[(size_t)y * w + x] = (uint8_t)std::min(255L, std::max(0L, std::lrint(res)));
        }
    }
}
int clahe_part(orbx_extractor *ex, int w, int h, int tiles_x, int tiles_y, double clip_limit, int n, size_t s_off, size_t d_off) {
    std::mt19937 rng(9 + w + h);
    Block src(s_off, (size_t)n * w * h), dst(d_off, (size_t)n * w * h);
    for (int f = 0; f < n; f++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                int v = 100 + (int)(60 * std::sin(x / 7.0 + f) * std::cos(y / 5.0)) + (int)(rng() % 31);
                if ((x / 9 + y / 7) % 4 == 0) v = 33 + 50 * ((x / 9) % 4);   // flat patches
                if ((x / 9 + y / 7) % 4 == 1) v = (int)(rng() % 256);
                src.p()[((size_t)f * h + y) * w + x] = (uint8_t)std::min(255, std::max(0, v));
            }
    std::vector<uint8_t> want(dst.bytes);
    for (int f = 0; f < n; f++) clahe_reference(src.p() + (size_t)f * w * h, w, h, clip_limit, tiles_x, tiles_y, want.data() + (size_t)f * w * h);
    orbx_clahe *c = nullptr;
    CHECK(orbx_clahe_create(0, clip_limit, 65, tiles_y, &c) == ORBX_E_BAD_ARG && c == nullptr);
    MUST(orbx_clahe_create(0, clip_limit, tiles_x, tiles_y, &c));
    const size_t rs = (size_t)w, fs = rs * h;
    CHECK(orbx_clahe_batch_device(c, ex, src.p(), n, w, h, rs, fs, src.p() + 1, rs, fs) == ORBX_E_BAD_ARG);
    CHECK(orbx_clahe_batch_device(c, ex, src.p(), 0, w, h, rs, fs, dst.p(), rs, fs) == ORBX_E_BAD_ARG);
    CHECK(orbx_clahe_batch_device(c, ex, src.p(), n, w, h, rs - 1, fs, dst.p(), rs, fs) == ORBX_E_BAD_ARG);
    CHECK(dst.untouched());
    MUST(orbx_clahe_batch_device(c, ex, src.p(), n, w, h, rs, fs, dst.p(), rs, fs));
    MUST(orbx_sync(ex));
    CHECK(dst.head_untouched());
    if (compare(dst.p(), want, "clahe")) return 1;
    MUST(orbx_clahe_batch_device(c, ex, src.p(), n, w, h, rs, fs, src.p(), rs, fs));   // apply(im, im)
    MUST(orbx_sync(ex));
    CHECK(src.head_untouched());
    if (compare(src.p(), want, "clahe in place")) return 1;
    orbx_clahe_destroy(c);
    return 0;
}

}  // namespace

int main() {
    const orbx_params prm = {500, 1.2f, 8, 20, 7, 0};
    orbx_extractor *ex = nullptr;
    MUST(orbx_create(&prm, 0, 0, 0, 0, &ex));
    const int widths[] = {1, 3, 5, 64, 65, 67}, frames[] = {1, 3, 5};
    int k = 0;
    for (int w : widths)
        for (int n : frames)
            for (int code = 0; code < 4; code++, k++)
                if (gray_part(ex, w, 5, n, code < 2 ? 3 : 4, code & 1, (size_t)(k % 4), (size_t)((k / 4) % 4))) {
                    printf("FAILED: gray width %d, %d frames, code %d\n", w, n, code);
                    return 1;
                }
    // {src_w, src_h, dst_w, dst_h}: exact halves (whole and part groups), a half in one dimension, enlargement, equal size, widths 1 and 3, reductions
    const int sizes[][4] = {{130, 22, 65, 11}, {10, 6, 5, 3}, {128, 22, 64, 13}, {67, 26, 67, 13}, {41, 9, 67, 14}, {64, 13, 64, 13}, {37, 11, 1, 5},
                            {7, 8, 3, 4}, {94, 60, 65, 41}, {77, 19, 64, 15}, {2, 2, 3, 5}, {2, 2, 1, 1}, {6, 4, 3, 2}};
    for (const auto &s : sizes)
        for (int n : frames) {
            k++;
            if (resize_part(ex, s[0], s[1], s[2], s[3], n, (size_t)(k % 4), (size_t)((k / 4) % 4))) {
                printf("FAILED: resize %d x %d -> %d x %d, %d frames\n", s[0], s[1], s[2], s[3], n);
                return 1;
            }
        }
    // {width, height, tiles_x, tiles_y, clip limit in tenths}
    const int cases[][5] = {{64, 48, 8, 8, 30}, {67, 48, 8, 8, 30}, {64, 45, 8, 8, 30}, {61, 45, 8, 8, 30}, {40, 30, 1, 1, 30}, {40, 30, 2, 3, 30},
                            {40, 30, 3, 8, 30}, {40, 30, 2, 3, 0}, {40, 30, 2, 3, 400}, {9, 9, 8, 8, 30}, {65, 3, 64, 2, 20}};
    for (const auto &c : cases)
        for (int n : frames) {
            k++;
            if (clahe_part(ex, c[0], c[1], c[2], c[3], c[4] / 10.0, n, (size_t)(k % 4), (size_t)((k / 4) % 4))) {
                printf("FAILED: clahe %d x %d, grid %d x %d, limit %g, %d frames\n", c[0], c[1], c[2], c[3], c[4] / 10.0, n);
                return 1;
            }
        }
    orbx_destroy(ex);
    printf("image enhance ok\n");
    return 0;
}
