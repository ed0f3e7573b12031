// image_prep_kernels.hip.h -- what ORB-SLAM3 does to the sensor's images on the host before the extractor sees them, on the device:
//   k_rectify               cv::remap(src, dst, map1, map2, INTER_LINEAR), 8-bit one channel, BORDER_CONSTANT 0 (System::TrackStereo, System.cc:259-260)
//   k_stereo_from_rgbd_u16  Frame::ComputeStereoFromRGBD on the raw 16-bit depth image (Tracking::GrabImageRGBD's convertTo folded in)
// The arithmetic of both is restated in include/orbx.h (orbx_rectify_batch_device, orbx_rgbd_batch_device_u16).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/orbx.h"

namespace orbx {

// ---------------------------------------------------------------------------------------------------------
// The fixed-point map, converted once from the two CV_32FC1 maps (orbx_rectifier_create, on the host): per destination pixel
//   xy   (uint32)  ix | iy << 16, both saturate_cast<short>(s >> 5) as int16
//   frac (uint16)  a | b << 8,    both s & 31
// in two planes whose rows are padded to a multiple of four entries (padding: ix = iy = -32768, every tap outside), so that a thread's four
// entries are one 16-byte and one 8-byte load.
// ---------------------------------------------------------------------------------------------------------
// cvRound(v * 32) as the x86 conversion gives it: nearest, ties to even; INT_MIN for NaN, infinite and anything outside int.  The product only
// moves the exponent (exact, or infinite); the range is tested BEFORE the conversion, whose result for such values differs between machines.
inline int32_t remap_fixed(float v) {
    const float p = v * 32.f;
    if (!(p >= -2147483648.f && p < 2147483648.f)) return INT_MIN;
    return (int32_t)std::nearbyint(p);   // (the default rounding mode: to nearest even; |p| >= 2^23 is integral already)
}
inline int32_t remap_short(int32_t s) {
    const int32_t i = s >> 5;   // arithmetic
    return i < -32768 ? -32768 : i > 32767 ? 32767 : i;
}
inline void remap_entry(float mx, float my, uint32_t *xy, uint16_t *frac) {
    const int32_t sx = remap_fixed(mx), sy = remap_fixed(my);
    *xy = (uint32_t)(uint16_t)(int16_t)remap_short(sx) | (uint32_t)(uint16_t)(int16_t)remap_short(sy) << 16;
    *frac = (uint16_t)((sx & 31) | (sy & 31) << 8);
}

struct RectifyArgs {
    const uint4 *xy;     // [dst_h][map_w4 / 4] four entries each
    const uint2 *frac;   // [dst_h][map_w4 / 4]
    int groups;          // map_w4 / 4: groups of four destination pixels per row
    int dst_w, dst_h, src_w, src_h, n_frames;
    const uint8_t *src; size_t src_row, src_frame;
    uint8_t *dst; size_t dst_row, dst_frame;
};

// the taps (ix, y) and (ix + 1, y) of one source row as lo | hi << 8; a tap outside [0, src_w) is 0 and its address is never formed
__device__ __forceinline__ uint32_t rectify_pair(const uint8_t *__restrict__ row, int ix, int src_w) {
    if ((unsigned)ix < (unsigned)(src_w - 1)) {   // both inside: two adjacent bytes, at any alignment
        uint16_t v;
        __builtin_memcpy(&v, row + ix, 2);
        return v;
    }
    uint32_t r = 0;
    if ((unsigned)ix < (unsigned)src_w) r = row[ix];
    if ((unsigned)(ix + 1) < (unsigned)src_w) r |= (uint32_t)row[ix + 1] << 8;
    return r;
}

// one destination pixel of one frame: four taps, weights (32-a)(32-b)32, a(32-b)32, (32-a)b 32, ab 32, (sum + 16384) >> 15
__device__ __forceinline__ uint32_t rectify_pixel(const uint8_t *__restrict__ img, size_t src_row, int src_w, int src_h, uint32_t xy, uint32_t frac) {
    const int ix = (int16_t)(xy & 0xffffu), iy = (int16_t)(xy >> 16);
    const int a = (int)(frac & 0xffu), b = (int)(frac >> 8 & 0xffu);
    uint32_t top = 0, bot = 0;
    if ((unsigned)iy < (unsigned)src_h) top = rectify_pair(img + (size_t)iy * src_row, ix, src_w);
    if ((unsigned)(iy + 1) < (unsigned)src_h) bot = rectify_pair(img + (size_t)(iy + 1) * src_row, ix, src_w);
    const int wa = 32 - a, wb = (32 - b) * 32, b32 = b * 32;
    const int sum = (int)(top & 0xffu) * (wa * wb) + (int)(top >> 8) * (a * wb) + (int)(bot & 0xffu) * (wa * b32) + (int)(bot >> 8) * (a * b32);
    return (uint32_t)(sum + 16384) >> 15;
}

// grid (ceil(groups / 64), ceil(dst_h / 4), frame chunks), block 256 = 64 groups x 4 rows.  A thread holds the map entries of four adjacent destination
// pixels of one row and serves them for kRectifyFrames frames per read (and for further chunks when the grid's z is short of them); per frame its four
// bytes leave as one dword where the address is aligned and the row has all four, byte by byte otherwise (odd d_dst / dst_row_stride, the last group).
constexpr int kRectifyFrames = 4;
__global__ __launch_bounds__(256) void k_rectify(const RectifyArgs A) {
    const int g = (int)(blockIdx.x * 64 + (threadIdx.x & 63)), y = (int)(blockIdx.y * 4 + (threadIdx.x >> 6));
    if (g >= A.groups || y >= A.dst_h) return;
    const uint4 xy = A.xy[(size_t)y * A.groups + g];
    const uint2 fr = A.frac[(size_t)y * A.groups + g];
    const uint32_t e[4] = {xy.x, xy.y, xy.z, xy.w};
    const uint32_t q[4] = {fr.x & 0xffffu, fr.x >> 16, fr.y & 0xffffu, fr.y >> 16};
    const int x0 = 4 * g, n_px = min(4, A.dst_w - x0);
    const int chunks = (A.n_frames + kRectifyFrames - 1) / kRectifyFrames;
    for (int c = (int)blockIdx.z; c < chunks; c += (int)gridDim.z) {
        const int f0 = c * kRectifyFrames;
        uint32_t px[kRectifyFrames][4];
        // every frame's taps first (the gathers of all frames in flight together), the stores behind them
#pragma unroll
        for (int j = 0; j < kRectifyFrames; j++) {
            if (f0 + j >= A.n_frames) break;
            const uint8_t *img = A.src + (size_t)(f0 + j) * A.src_frame;
#pragma unroll
            for (int k = 0; k < 4; k++) px[j][k] = rectify_pixel(img, A.src_row, A.src_w, A.src_h, e[k], q[k]);
        }
#pragma unroll
        for (int j = 0; j < kRectifyFrames; j++) {
            if (f0 + j >= A.n_frames) break;
            uint8_t *out = A.dst + (size_t)(f0 + j) * A.dst_frame + (size_t)y * A.dst_row + x0;
            if (n_px == 4 && ((uintptr_t)out & 3u) == 0)
                *reinterpret_cast<uint32_t *>(out) = px[j][0] | px[j][1] << 8 | px[j][2] << 16 | px[j][3] << 24;
            else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (k < n_px) out[k] = (uint8_t)px[j][k];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Frame::ComputeStereoFromRGBD on the sensor's 16-bit depth image: k_stereo_from_rgbd (matcher_kernels.hip.h) with
// d = (float)raw * depth_factor -- one conversion (exact: 16 bits) and one rounded product, Tracking::GrabImageRGBD's
// imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) at the one pixel the feature reads -- in front of the same tail.
// grid (n_frames), block 256
// ---------------------------------------------------------------------------------------------------------
struct RgbdU16Stage {
    const orbx_keypoint *kps, *kps_un;   // [B][cap] mvKeys, mvKeysUn
    const int32_t *count;                // [B]
    const uint8_t *depth;                // B uint16 images, `pitch` bytes per row, `frame_stride` bytes per image
    size_t pitch, frame_stride;
    int cap, width, height;
    float bf, depth_factor;
    float *u_right, *out_depth;          // [B][cap]
    int32_t *nmatches;                   // [B]
};
__global__ __launch_bounds__(256) void k_stereo_from_rgbd_u16(const RgbdU16Stage S) {
    __shared__ int32_t total;
    const int f = blockIdx.x;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const int n = max(0, min(S.count[f], S.cap));
    const uint8_t *img = S.depth + (size_t)f * S.frame_stride;
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const size_t o = (size_t)f * S.cap + i;
        const float u = S.kps[o].x, v = S.kps[o].y;
        float d = -1.f;
        // (int)u lies in [0, width) exactly when -1 < u < width; a NaN coordinate fails the comparison and is never converted
        if (u > -1.f && u < (float)S.width && v > -1.f && v < (float)S.height)
            d = __fmul_rn((float)*reinterpret_cast<const uint16_t *>(img + (size_t)(int)v * S.pitch + 2 * (size_t)(int)u), S.depth_factor);
        const bool has = d > 0.f;
        S.out_depth[o] = has ? d : -1.f;
        S.u_right[o] = has ? __fsub_rn(S.kps_un[o].x, __fdiv_rn(S.bf, d)) : -1.f;
        mine += has ? 1 : 0;
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) S.nmatches[f] = total;
}

}  // namespace orbx
