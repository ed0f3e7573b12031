// cv::remap(src, dst, map1, map2, INTER_LINEAR) for 8-bit one-channel images and two CV_32FC1 maps, BORDER_CONSTANT 0, as include/orbx.h restates it:
// a plain C++ loop on one core, the maps converted to fixed point for every image as remap does for every call.  The yardstick of
// tools/image_prep_latency.py (g++ -O3); it is NOT OpenCV's SIMD code, whose speed is not measured anywhere in this repository.
// remap_host_loop: n_frames images, `reps` repetitions; returns the fastest repetition in microseconds by its own clock.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace {
inline int fixed(float v) {
    const float p = v * 32.f;
    if (!(p >= -2147483648.f && p < 2147483648.f)) return INT_MIN;
    return (int)std::nearbyint(p);
}
inline int saturate_short(int v) { return std::min(32767, std::max(-32768, v)); }
}  // namespace

extern "C" double remap_host_loop(const uint8_t *src, int n_frames, int sw, int sh, const float *map_x, const float *map_y, int dw, int dh, uint8_t *dst, int reps) {
    double best = 1e300;
    for (int rep = 0; rep < reps; rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int f = 0; f < n_frames; f++) {
            const uint8_t *img = src + (size_t)f * sw * sh;
            uint8_t *out = dst + (size_t)f * dw * dh;
            for (int y = 0; y < dh; y++)
                for (int x = 0; x < dw; x++) {
                    const int sx = fixed(map_x[(size_t)y * dw + x]), sy = fixed(map_y[(size_t)y * dw + x]);
                    const int a = sx & 31, b = sy & 31, ix = saturate_short(sx >> 5), iy = saturate_short(sy >> 5);
                    int sum;
                    if ((unsigned)ix < (unsigned)(sw - 1) && (unsigned)iy < (unsigned)(sh - 1)) {   // all four taps inside
                        const uint8_t *p = img + (size_t)iy * sw + ix;
                        sum = p[0] * ((32 - a) * (32 - b) * 32) + p[1] * (a * (32 - b) * 32) + p[sw] * ((32 - a) * b * 32) + p[sw + 1] * (a * b * 32);
                    } else {
                        auto tap = [&](int tx, int ty) -> int { return (unsigned)tx < (unsigned)sw && (unsigned)ty < (unsigned)sh ? img[(size_t)ty * sw + tx] : 0; };
                        sum = tap(ix, iy) * ((32 - a) * (32 - b) * 32) + tap(ix + 1, iy) * (a * (32 - b) * 32) + tap(ix, iy + 1) * ((32 - a) * b * 32) +
                              tap(ix + 1, iy + 1) * (a * b * 32);
                    }
                    out[(size_t)y * dw + x] = (uint8_t)((sum + 16384) >> 15);
                }
        }
        best = std::min(best, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    return best;
}
