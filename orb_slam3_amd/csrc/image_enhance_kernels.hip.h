// image_enhance_kernels.hip.h -- the image-sized host steps that sit in front of ORB-SLAM3's extractor besides cv::remap, on the device:
//   k_gray          cvtColor(..., COLOR_{RGB,BGR,RGBA,BGRA}2GRAY), 8-bit (Tracking::GrabImage*, Tracking.cc:1569-1582)
//   k_resize        cv::resize(..., INTER_LINEAR), 8-bit one channel, the generic path (System::Track*, needToResize())
//   k_resize_half   the same for exactly half the size: OpenCV's 2 x 2 area path
//   k_clahe_lut     cv::CLAHE::apply, step 1: one look-up table per (frame, tile)           (the TUM-VI examples)
//   k_clahe_apply   cv::CLAHE::apply, step 2: four tables interpolated per pixel
// The arithmetic of all of them is restated in include/orbx.h (orbx_gray_batch_device, orbx_resize_batch_device, orbx_clahe_batch_device).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/orbx.h"

namespace orbx {

// four adjacent bytes of a row leave as one dword where the address is aligned and the row has all four, byte by byte otherwise
__device__ __forceinline__ void store_px4(uint8_t *out, int n_px, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
    if (n_px == 4 && ((uintptr_t)out & 3u) == 0) {
        *reinterpret_cast<uint32_t *>(out) = p0 | p1 << 8 | p2 << 16 | p3 << 24;
    } else {
        const uint32_t p[4] = {p0, p1, p2, p3};
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n_px) out[k] = (uint8_t)p[k];
    }
}
// n_px (1..4) adjacent bytes of a row as b0 | b1 << 8 | ..: one dword load where the address is aligned and the row has all four; no byte past the
// row's last is read
__device__ __forceinline__ uint32_t load_px4(const uint8_t *in, int n_px) {
    if (n_px == 4 && ((uintptr_t)in & 3u) == 0) return *reinterpret_cast<const uint32_t *>(in);
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (k < n_px) r |= (uint32_t)in[k] << (8 * k);
    return r;
}

// ---------------------------------------------------------------------------------------------------------
// k_gray: gray = (c0 * byte0 + 19235 * byte1 + c2 * byte2 + 16384) >> 15, c0 / c2 = 9798 / 3735 when the first byte is R, the reverse when it is B;
// a fourth byte is skipped.  grid (ceil(groups / 64), ceil(height / 4), n_frames), block 256 = 64 groups of four pixels x 4 rows.
// ---------------------------------------------------------------------------------------------------------
struct GrayArgs {
    const uint8_t *src; size_t src_row, src_frame;
    uint8_t *dst; size_t dst_row, dst_frame;
    int width, height, channels;
    uint32_t c0, c2;
};
__device__ __forceinline__ uint32_t gray_px(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t c0, uint32_t c2) {
    return (b0 * c0 + b1 * 19235u + b2 * c2 + 16384u) >> 15;
}
__global__ __launch_bounds__(256) void k_gray(const GrayArgs A) {
    const int g = (int)(blockIdx.x * 64 + (threadIdx.x & 63)), y = (int)(blockIdx.y * 4 + (threadIdx.x >> 6));
    const int x0 = 4 * g;
    if (x0 >= A.width || y >= A.height) return;
    const int n_px = min(4, A.width - x0);
    const uint8_t *in = A.src + (size_t)blockIdx.z * A.src_frame + (size_t)y * A.src_row + (size_t)x0 * A.channels;
    uint32_t px[4] = {0, 0, 0, 0};
    if (n_px == 4 && ((uintptr_t)in & 3u) == 0) {   // 12 or 16 bytes as dwords
        const uint32_t *q = reinterpret_cast<const uint32_t *>(in);
        if (A.channels == 4) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t d = q[k];
                px[k] = gray_px(d & 0xffu, d >> 8 & 0xffu, d >> 16 & 0xffu, A.c0, A.c2);
            }
        } else {
            const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
            px[0] = gray_px(d0 & 0xffu, d0 >> 8 & 0xffu, d0 >> 16 & 0xffu, A.c0, A.c2);
            px[1] = gray_px(d0 >> 24, d1 & 0xffu, d1 >> 8 & 0xffu, A.c0, A.c2);
            px[2] = gray_px(d1 >> 16 & 0xffu, d1 >> 24, d2 & 0xffu, A.c0, A.c2);
            px[3] = gray_px(d2 >> 8 & 0xffu, d2 >> 16 & 0xffu, d2 >> 24, A.c0, A.c2);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n_px) px[k] = gray_px(in[k * A.channels], in[k * A.channels + 1], in[k * A.channels + 2], A.c0, A.c2);
    }
    store_px4(A.dst + (size_t)blockIdx.z * A.dst_frame + (size_t)y * A.dst_row + x0, n_px, px[0], px[1], px[2], px[3]);
}

// ---------------------------------------------------------------------------------------------------------
// k_resize: cv::resize's generic INTER_LINEAR path for 8-bit one channel (resizeGeneric_<HResizeLinear<uchar,int,short,2048>, VResizeLinear<..>>).
// The tables are built on the host (resize_tab below) in OpenCV's float / double arithmetic; the kernel does the integer part:
//   row(sy)[x] = S[sy][xofs[x]] * c0[x] + S[sy][min(xofs[x] + 1, sw - 1)] * c1[x]      (c1 == 0 wherever xofs + 1 == sw: OpenCV's tail S * 2048)
//   dst[y][x]  = clamp((((b0[y] * (row(sy0)[x] >> 4)) >> 16) + ((b1[y] * (row(sy1)[x] >> 4)) >> 16) + 2) >> 2, 0, 255)
// xtab [groups * 4] {xofs, c0 | c1 << 16} (padding: 0, 0), ytab [dst_h] {sy0, sy1, b0, b1} (rows clamped to the image already).
// grid (ceil(groups / 64), ceil(dst_h / 4), n_frames), block 256 = 64 groups of four destination pixels x 4 rows.
// ---------------------------------------------------------------------------------------------------------
struct ResizeArgs {
    const uint2 *xtab; const uint4 *ytab;
    const uint8_t *src; size_t src_row, src_frame;
    uint8_t *dst; size_t dst_row, dst_frame;
    int src_w, src_h, dst_w, dst_h;
};
__global__ __launch_bounds__(256) void k_resize(const ResizeArgs A) {
    const int g = (int)(blockIdx.x * 64 + (threadIdx.x & 63)), y = (int)(blockIdx.y * 4 + (threadIdx.x >> 6));
    const int x0 = 4 * g;
    if (x0 >= A.dst_w || y >= A.dst_h) return;
    const int n_px = min(4, A.dst_w - x0);
    const uint4 ty = A.ytab[y];
    const int b0 = (int)ty.z, b1 = (int)ty.w;
    const uint8_t *r0 = A.src + (size_t)blockIdx.z * A.src_frame + (size_t)ty.x * A.src_row, *r1 = r0 + ((size_t)ty.y - (size_t)ty.x) * A.src_row;
    uint32_t px[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint2 tx = A.xtab[x0 + k];   // (the table is padded to whole groups)
        const int xa = (int)tx.x, xb = min(xa + 1, A.src_w - 1), c0 = (int16_t)(tx.y & 0xffffu), c1 = (int16_t)(tx.y >> 16);
        const int h0 = (int)r0[xa] * c0 + (int)r0[xb] * c1, h1 = (int)r1[xa] * c0 + (int)r1[xb] * c1;
        const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
        px[k] = (uint32_t)min(max(v, 0), 255);
    }
    store_px4(A.dst + (size_t)blockIdx.z * A.dst_frame + (size_t)y * A.dst_row + x0, n_px, px[0], px[1], px[2], px[3]);
}

// k_resize_half: src == 2 * dst in both dimensions: dst = (a + b + c + d + 2) >> 2 over the 2 x 2 block.  A thread reads two rows of four pairs.
// grid and block as k_resize (ResizeArgs without the tables).
__global__ __launch_bounds__(256) void k_resize_half(const ResizeArgs A) {
    const int g = (int)(blockIdx.x * 64 + (threadIdx.x & 63)), y = (int)(blockIdx.y * 4 + (threadIdx.x >> 6));
    const int x0 = 4 * g;
    if (x0 >= A.dst_w || y >= A.dst_h) return;
    const int n_px = min(4, A.dst_w - x0);
    const uint8_t *r0 = A.src + (size_t)blockIdx.z * A.src_frame + (size_t)(2 * y) * A.src_row + 2 * (size_t)x0, *r1 = r0 + A.src_row;
    // the pairs of pixels 0, 1 and of pixels 2, 3: n_px pixels need 2 * n_px source bytes per row
    const uint32_t t0 = load_px4(r0, min(4, 2 * n_px)), b0 = load_px4(r1, min(4, 2 * n_px));
    uint32_t t1 = 0, b1 = 0;
    if (n_px > 2) { t1 = load_px4(r0 + 4, 2 * n_px - 4); b1 = load_px4(r1 + 4, 2 * n_px - 4); }
    const uint32_t p0 = ((t0 & 0xffu) + (t0 >> 8 & 0xffu) + (b0 & 0xffu) + (b0 >> 8 & 0xffu) + 2u) >> 2;
    const uint32_t p1 = ((t0 >> 16 & 0xffu) + (t0 >> 24) + (b0 >> 16 & 0xffu) + (b0 >> 24) + 2u) >> 2;
    const uint32_t p2 = ((t1 & 0xffu) + (t1 >> 8 & 0xffu) + (b1 & 0xffu) + (b1 >> 8 & 0xffu) + 2u) >> 2;
    const uint32_t p3 = ((t1 >> 16 & 0xffu) + (t1 >> 24) + (b1 >> 16 & 0xffu) + (b1 >> 24) + 2u) >> 2;
    store_px4(A.dst + (size_t)blockIdx.z * A.dst_frame + (size_t)y * A.dst_row + x0, n_px, p0, p1, p2, p3);
}

// The coefficient tables of one dimension as OpenCV builds them: ofs[d] = floor(fx), fx = (float)((d + 0.5) * scale - 0.5) with
// scale = 1 / ((double)dsize / ssize); the fraction fx - ofs; horizontally offset and fraction are reset at both borders, vertically only the rows are
// clamped (by the caller); c0 = saturate_cast<short>((1.f - f) * 2048), c1 = saturate_cast<short>(f * 2048) (cvRound: nearest, ties to even).
inline void resize_tab(int ssize, int dsize, bool horizontal, int d, int *ofs, int *c0, int *c1) {
    const double inv_scale = (double)dsize / ssize, scale = 1. / inv_scale;
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)std::floor(f);
    f -= (float)s;
    if (horizontal) {
        if (s < 0) { f = 0; s = 0; }
        if (s >= ssize - 1) { f = 0; s = ssize - 1; }
    }
    *ofs = s;
    const long a0 = std::lrint((1.f - f) * 2048.f), a1 = std::lrint(f * 2048.f);   // (the default rounding mode: to nearest even)
    *c0 = (int)(a0 < -32768 ? -32768 : a0 > 32767 ? 32767 : a0);
    *c1 = (int)(a1 < -32768 ? -32768 : a1 > 32767 ? 32767 : a1);
}

// ---------------------------------------------------------------------------------------------------------
// CLAHE.  The geometry of one call, computed on the host (clahe_geometry in orbx_extractor.hip) as clahe.cpp computes it.
// ---------------------------------------------------------------------------------------------------------
constexpr int kClaheMaxTiles = 64;
struct ClaheArgs {
    const uint8_t *src; size_t src_row, src_frame;
    uint8_t *dst; size_t dst_row, dst_frame;
    uint8_t *lut;                 // [n_frames][tiles_y][tiles_x][256]
    int width, height, tiles_x, tiles_y, tile_w, tile_h;
    int clip;                     // 0: no clipping
    float lut_scale, inv_tw, inv_th;
    // rows [band[b], band[b + 1]) are the rows y with floor((float)y * inv_th - 0.5f) == b - 1, b = 0 .. tiles_y: between two tile-centre rows
    int band[kClaheMaxTiles + 2];
};

// k_clahe_lut: one workgroup per (tile x, tile y, frame), block 256 = 4 waves.  Each wave counts its rows of the tile into a histogram of its own
// (LDS atomics: a flat tile then contends within a wave only, not across the group); bin i of the sum belongs to thread i from there on: clipping
// (a workgroup sum of the excess), redistribution (the closed form of clahe.cpp's residual loop: bin i gets +1 iff i % step == 0 && i / step < residual,
// because residual * step <= 256 keeps the loop's `i < 256` from ever ending it), the cumulative sum (wave scans plus carries) and
// lut[i] = saturate_cast<uchar>(cvRound((float)sum * lut_scale)); the 256 bytes leave as 64 dwords.
// A tile's pixels past the image's right or bottom edge are the reflected ones (BORDER_REFLECT_101); the extension is never materialised.
__global__ __launch_bounds__(256) void k_clahe_lut(const ClaheArgs A) {
    __shared__ uint32_t s_hist[4][256];
    __shared__ uint32_t s_part[4];
    __shared__ uint32_t s_lut[64];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < 4; k++) s_hist[k][tid] = 0;
    __syncthreads();
    const uint8_t *img = A.src + (size_t)blockIdx.z * A.src_frame;
    const int tx0 = (int)blockIdx.x * A.tile_w, ty0 = (int)blockIdx.y * A.tile_h;
    for (int r = wave; r < A.tile_h; r += 4) {
        int y = ty0 + r;
        if (y >= A.height) y = 2 * (A.height - 1) - y;
        const uint8_t *row = img + (size_t)y * A.src_row;
        for (int c = lane; c < A.tile_w; c += 64) {
            int x = tx0 + c;
            if (x >= A.width) x = 2 * (A.width - 1) - x;
            atomicAdd(&s_hist[wave][row[x]], 1u);
        }
    }
    __syncthreads();
    uint32_t h = s_hist[0][tid] + s_hist[1][tid] + s_hist[2][tid] + s_hist[3][tid];
    if (A.clip > 0) {
        const uint32_t clip = (uint32_t)A.clip;
        uint32_t excess = h > clip ? h - clip : 0u;
        h = min(h, clip);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) excess += __shfl_xor(excess, m);
        if (lane == 0) s_part[wave] = excess;
        __syncthreads();
        const uint32_t clipped = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        const uint32_t batch = clipped >> 8, residual = clipped & 255u;
        h += batch;
        if (residual != 0) {
            const uint32_t step = max(256u / residual, 1u);
            if ((uint32_t)tid % step == 0 && (uint32_t)tid / step < residual) h++;
        }
        __syncthreads();   // s_part is written again below
    }
    uint32_t sum = h;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(sum, (unsigned)d);
        if (lane >= d) sum += up;
    }
    if (lane == 63) s_part[wave] = sum;
    __syncthreads();
    for (int k = 0; k < wave; k++) sum += s_part[k];
    const int v = __float2int_rn(__fmul_rn((float)sum, A.lut_scale));
    reinterpret_cast<uint8_t *>(s_lut)[tid] = (uint8_t)min(max(v, 0), 255);
    __syncthreads();
    if (tid < 64) {
        uint8_t *out = A.lut + (((size_t)blockIdx.z * A.tiles_y + blockIdx.y) * A.tiles_x + blockIdx.x) * 256;
        reinterpret_cast<uint32_t *>(out)[tid] = s_lut[tid];
    }
}

// k_clahe_apply: grid (ceil(longest band / kClaheBandRows), tiles_y + 1 bands, n_frames), block 256 = 4 rows x 64 groups of four pixels, striding over
// the slice's rows and the row's groups.  All rows of a band share ty1 / ty2, so the workgroup stages those two tile rows of tables in LDS
// (dynamic, 2 * tiles_x * 256 bytes) with the two rows interleaved -- entry [tx][v] = top | bottom << 8 as one 16-bit value -- so that a pixel's four
// table bytes are two 16-bit LDS reads (a gather by pixel value: whatever bank conflicts the image's values give are left as they are).  Per pixel
//   txf = (float)x * inv_tw - 0.5f, tx1 = floor(txf), xa = txf - tx1, xa1 = 1.f - xa, THEN tx1 = max(tx1, 0), tx2 = min(tx1 + 1, tiles_x - 1); the same in y;
//   res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya, every operation rounded as written; dst = saturate_cast<uchar>(cvRound(res)).
// A thread reads its four source pixels before it writes them: d_dst == d_src with equal strides is in place.
constexpr int kClaheBandRows = 32;
__global__ __launch_bounds__(256) void k_clahe_apply(const ClaheArgs A) {
    extern __shared__ uint32_t s_tab[];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y;
    const int y_begin = A.band[b] + (int)blockIdx.x * kClaheBandRows, y_end = min(A.band[b + 1], y_begin + kClaheBandRows);
    if (y_begin >= y_end) return;   // (the whole workgroup)
    const int ty1 = max(b - 1, 0), ty2 = min(b, A.tiles_y - 1);
    const uint32_t *top = reinterpret_cast<const uint32_t *>(A.lut + ((size_t)blockIdx.z * A.tiles_y + ty1) * A.tiles_x * 256);
    const uint32_t *bot = reinterpret_cast<const uint32_t *>(A.lut + ((size_t)blockIdx.z * A.tiles_y + ty2) * A.tiles_x * 256);
    for (int i = tid; i < A.tiles_x * 64; i += 256) {   // four values of one tile per step
        const uint32_t t = top[i], u = bot[i];
        s_tab[2 * i] = (t & 0xffu) | (u & 0xffu) << 8 | (t & 0xff00u) << 8 | (u & 0xff00u) << 16;
        s_tab[2 * i + 1] = (t >> 16 & 0xffu) | (u >> 16 & 0xffu) << 8 | (t >> 24) << 16 | (u >> 24) << 24;
    }
    __syncthreads();
    const uint16_t *tab = reinterpret_cast<const uint16_t *>(s_tab);
    const int groups = (A.width + 3) >> 2;
    for (int y = y_begin + (tid >> 6); y < y_end; y += 4) {
        const float tyf = __fsub_rn(__fmul_rn((float)y, A.inv_th), 0.5f);
        const float ya = __fsub_rn(tyf, floorf(tyf)), ya1 = __fsub_rn(1.0f, ya);
        const uint8_t *in = A.src + (size_t)blockIdx.z * A.src_frame + (size_t)y * A.src_row;
        uint8_t *out = A.dst + (size_t)blockIdx.z * A.dst_frame + (size_t)y * A.dst_row;
        for (int g = tid & 63; g < groups; g += 64) {
            const int x0 = 4 * g, n_px = min(4, A.width - x0);
            const uint32_t v4 = load_px4(in + x0, n_px);
            uint32_t px[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float txf = __fsub_rn(__fmul_rn((float)(x0 + k), A.inv_tw), 0.5f);
                const float fl = floorf(txf);
                const float xa = __fsub_rn(txf, fl), xa1 = __fsub_rn(1.0f, xa);
                const int tx1 = min(max((int)fl, 0), A.tiles_x - 1), tx2 = min((int)fl + 1, A.tiles_x - 1);   // (floor(txf) <= tiles_x - 1 always)
                const uint32_t v = v4 >> (8 * k) & 0xffu;
                const uint32_t l1 = tab[tx1 * 256 + (int)v], l2 = tab[tx2 * 256 + (int)v];
                const float top_v = __fadd_rn(__fmul_rn((float)(l1 & 0xffu), xa1), __fmul_rn((float)(l2 & 0xffu), xa));
                const float bot_v = __fadd_rn(__fmul_rn((float)(l1 >> 8), xa1), __fmul_rn((float)(l2 >> 8), xa));
                const int r = __float2int_rn(__fadd_rn(__fmul_rn(top_v, ya1), __fmul_rn(bot_v, ya)));
                px[k] = (uint32_t)min(max(r, 0), 255);
            }
            store_px4(out + x0, n_px, px[0], px[1], px[2], px[3]);
        }
    }
}

}  // namespace orbx
