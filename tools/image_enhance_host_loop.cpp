// cvtColor (to gray), cv::resize (INTER_LINEAR) and cv::CLAHE::apply for 8-bit images as include/orbx.h restates them: plain C++ loops on one core.
// The yardstick of tools/image_enhance_latency.py (g++ -O3 -ffp-contract=off); it is NOT OpenCV's SIMD code, whose speed is not measured anywhere in
// this repository.  Each function runs n_frames packed images `reps` times and returns the fastest repetition in microseconds by its own clock.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {
typedef std::chrono::steady_clock Clock;
double us_since(Clock::time_point t0) { return std::chrono::duration<double, std::micro>(Clock::now() - t0).count(); }

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
inline int reflect101(int p, int len) { return p < len ? p : 2 * (len - 1) - p; }
}  // namespace

extern "C" double gray_host_loop(const uint8_t *src, int n_frames, int w, int h, int channels, int rgb, uint8_t *dst, int reps) {
    double best = 1e300;
    const int c0 = rgb ? 9798 : 3735, c2 = rgb ? 3735 : 9798;
    for (int rep = 0; rep < reps; rep++) {
        const auto t0 = Clock::now();
        const size_t n = (size_t)n_frames * w * h;
        for (size_t i = 0; i < n; i++) {
            const uint8_t *p = src + i * channels;
            dst[i] = (uint8_t)((p[0] * c0 + p[1] * 19235 + p[2] * c2 + 16384) >> 15);
        }
        best = std::min(best, us_since(t0));
    }
    return best;
}

extern "C" double resize_host_loop(const uint8_t *src, int n_frames, int sw, int sh, uint8_t *dst, int dw, int dh, int reps) {
    double best = 1e300;
    std::vector<int> row0(dw), row1(dw);
    for (int rep = 0; rep < reps; rep++) {
        const auto t0 = Clock::now();
        const bool half = sw == 2 * dw && sh == 2 * dh;
        const Tab tx = linear_tab(sw, dw, true), ty = linear_tab(sh, dh, false);   // per call, as cv::resize builds them
        for (int f = 0; f < n_frames; f++) {
            const uint8_t *img = src + (size_t)f * sw * sh;
            uint8_t *out = dst + (size_t)f * dw * dh;
            for (int y = 0; y < dh; y++) {
                if (half) {
                    const uint8_t *p = img + (size_t)(2 * y) * sw;
                    for (int x = 0; x < dw; x++) out[(size_t)y * dw + x] = (uint8_t)((p[2 * x] + p[2 * x + 1] + p[sw + 2 * x] + p[sw + 2 * x + 1] + 2) >> 2);
                    continue;
                }
                const int sy0 = std::min(std::max(ty.ofs[y], 0), sh - 1), sy1 = std::min(std::max(ty.ofs[y] + 1, 0), sh - 1);
                const uint8_t *S0 = img + (size_t)sy0 * sw, *S1 = img + (size_t)sy1 * sw;
                for (int x = 0; x < dw; x++) {
                    const int sx = tx.ofs[x];
                    if (sx + 1 < sw) { row0[x] = S0[sx] * tx.c0[x] + S0[sx + 1] * tx.c1[x]; row1[x] = S1[sx] * tx.c0[x] + S1[sx + 1] * tx.c1[x]; }
                    else { row0[x] = S0[sx] * 2048; row1[x] = S1[sx] * 2048; }
                }
                for (int x = 0; x < dw; x++) {
                    const int v = (((ty.c0[y] * (row0[x] >> 4)) >> 16) + ((ty.c1[y] * (row1[x] >> 4)) >> 16) + 2) >> 2;
                    out[(size_t)y * dw + x] = (uint8_t)std::min(std::max(v, 0), 255);
                }
            }
        }
        best = std::min(best, us_since(t0));
    }
    return best;
}

extern "C" double clahe_host_loop(const uint8_t *src_all, int n_frames, int w, int h, double clip_limit, int tiles_x, int tiles_y, uint8_t *dst_all, int reps) {
    double best = 1e300;
    int pad_x = 0, pad_y = 0;
    if (w % tiles_x != 0 || h % tiles_y != 0) { pad_x = tiles_x - w % tiles_x; pad_y = tiles_y - h % tiles_y; }
    const int tile_w = (w + pad_x) / tiles_x, tile_h = (h + pad_y) / tiles_y, area = tile_w * tile_h;
    const int clip = clip_limit > 0 ? std::max((int)(clip_limit * area / 256), 1) : 0;
    const float lut_scale = 255.0f / (float)area, inv_tw = 1.0f / (float)tile_w, inv_th = 1.0f / (float)tile_h;
    std::vector<uint8_t> lut((size_t)tiles_x * tiles_y * 256);
    for (int rep = 0; rep < reps; rep++) {
        const auto t0 = Clock::now();
        for (int f = 0; f < n_frames; f++) {
            const uint8_t *src = src_all + (size_t)f * w * h;
            uint8_t *dst = dst_all + (size_t)f * w * h;
            for (int ty = 0; ty < tiles_y; ty++)
                for (int tx = 0; tx < tiles_x; tx++) {
                    int hist[256] = {0};
                    for (int y = ty * tile_h; y < (ty + 1) * tile_h; y++) {
                        const uint8_t *row = src + (size_t)reflect101(y, h) * w;
                        for (int x = tx * tile_w; x < (tx + 1) * tile_w; x++) hist[row[reflect101(x, w)]]++;
                    }
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
                    uint8_t *l = &lut[((size_t)ty * tiles_x + tx) * 256];
                    for (int i = 0; i < 256; i++) {
                        sum += hist[i];
                        l[i] = (uint8_t)std::min(255L, std::max(0L, std::lrint((float)sum * lut_scale)));
                    }
                }
            for (int y = 0; y < h; y++) {
                const float tyf = (float)y * inv_th - 0.5f;
                int ty1 = (int)std::floor(tyf), ty2 = ty1 + 1;
                const float ya = tyf - (float)ty1, ya1 = 1.0f - ya;
                ty1 = std::max(ty1, 0); ty2 = std::min(ty2, tiles_y - 1);
                const uint8_t *top = &lut[(size_t)ty1 * tiles_x * 256], *bot = &lut[(size_t)ty2 * tiles_x * 256];
                for (int x = 0; x < w; x++) {
                    const float txf = (float)x * inv_tw - 0.5f;
                    int tx1 = (int)std::floor(txf), tx2 = tx1 + 1;
                    const float xa = txf - (float)tx1, xa1 = 1.0f - xa;
                    tx1 = std::max(tx1, 0); tx2 = std::min(tx2, tiles_x - 1);
                    const int v = src[(size_t)y * w + x];
                    const float a = (float)top[tx1 * 256 + v] * xa1 + (float)top[tx2 * 256 + v] * xa;
                    const float b = (float)bot[tx1 * 256 + v] * xa1 + (float)bot[tx2 * 256 + v] * xa;
                    dst[(size_t)y * w + x] = (uint8_t)std::min(255L, std::max(0L, std::lrint(a * ya1 + b * ya)));
                }
            }
        }
        best = std::min(best, us_since(t0));
    }
    return best;
}
