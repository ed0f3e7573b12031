/*
 * orbx.h -- C ABI of liborbx.so: the MI355X (gfx950) ORB front-end for ORB-SLAM3.
 *
 * This is the drop-in boundary.  The reference has no FFI seam: ORBextractor / ORBmatcher are ordinary C++
 * classes (/root/reference/include/ORBextractor.h:43-109, include/ORBmatcher.h:36-103).  The replacement is
 * a same-named C++ adapter (orb_slam3_amd/cpp/ORBextractor.h, ORBmatcher.h) whose methods forward to the
 * entry points below; INTEGRATION.md shows the binding a maintainer adds.  Plain pointers and sizes only --
 * no C++ types, no OpenCV types, no torch types, no exceptions cross this ABI.
 *
 * All compute entry points run hand-written HIP kernels on the selected GPU.  There is no CPU fallback:
 * if no HIP device is usable the create functions fail with ORBX_E_NO_DEVICE.
 */
#ifndef ORBX_H
#define ORBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_VERSION 100

/* status codes: >= 0 success, < 0 error.  ORBX_E_EMPTY mirrors the reference's "return -1" for an empty
 * image (ORBextractor.cc:1090). */
enum {
    ORBX_OK = 0,
    ORBX_E_EMPTY = -1,
    ORBX_E_BAD_ARG = -2,
    ORBX_E_TOO_SMALL = -3,   /* a pyramid level would have no 35-px FAST cell, or its detection window is narrower than half its
                              * height (nIni = round(w/h) = 0, src/ORBextractor.cc:559-580): the reference divides by zero there */
    ORBX_E_CAPACITY = -4,    /* output capacity too small */
    ORBX_E_NO_DEVICE = -5,
    ORBX_E_HIP = -6,         /* a HIP runtime call failed; see orbx_last_error() */
    ORBX_E_TOO_LARGE = -7,   /* image / batch exceeds the limits given at creation, or a dimension > 4095 px */
    ORBX_E_INTERNAL = -8,    /* device-side consistency check failed; orbx_last_error() names the code: 1 more keypoints than the output
                              * capacity, 2 / 3 quad-tree node pool / level list overflow */
    ORBX_E_STALE = -9        /* level 0 of a batch that was extracted in place was requested after orbx_sync / orbx_download_wait released the
                              * caller's frames (see orbx_get_level) */
};

/* 28-byte POD with the field layout of cv::KeyPoint {Point2f pt; float size, angle, response; int octave,
 * class_id} -- what ORBextractor::operator() fills (ORBextractor.cc:861-869, 884-890). */
typedef struct orbx_keypoint {
    float x, y;
    float size;
    float angle;
    float response;
    int32_t octave;
    int32_t class_id;
} orbx_keypoint;

/* flags in orbx_params.flags */
enum {
    /* Round descriptor sample coordinates with separate multiply and add (strict ISO evaluation of
     * ORBextractor.cc:117-119).  Default (flag clear): the fused form GCC emits for the reference's own
     * build flags (-O3 -march=native, CMakeLists.txt:10-13) on an FMA-capable x86. */
    ORBX_FLAG_DESC_STRICT = 1u,
    /* 7x7 Gaussian taps of OpenCV <= 4.5.0 ([18,34,49,55,49,34,18]/256) instead of >= 4.5.1
     * ([18,34,48,56,48,34,18]/256). */
    ORBX_FLAG_BLUR_OCV440 = 2u,
    /* cv::fastAtan2 (ORBextractor.cc:102) with its polynomial contracted to fused multiply-adds:
     * fma(fma(fma(p7,c2,p5),c2,p3),c2,p1) * c, and 90 - q*c as ONE fnmadd.  That is what the scalar atan_f32 of
     * OpenCV's core/src/mathfuncs.cpp compiles to where FMA is part of the library's BASELINE instruction set and the
     * compiler contracts by default (GCC: -ffp-contract=fast): aarch64 builds (NEON FMA is baseline: Jetson, Apple),
     * and x86 builds configured with CPU_BASELINE >= FMA3 / AVX2 or -march=native.  Default (flag clear): every
     * operation rounded separately -- the stock x86-64 packages (baseline SSE3; FMA only in the dispatched array
     * kernels, which the scalar cv::fastAtan2 does not go through).  The two differ by 1 ulp on a few percent of the
     * angles (up to 3e-5 degrees near 360). */
    ORBX_FLAG_ATAN_FMA = 4u
};

/* ORBextractor constructor arguments (ORBextractor.h:50-51; values from Settings.cc:443-451) */
typedef struct orbx_params {
    int32_t nfeatures;
    float scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
    uint32_t flags;
} orbx_params;

typedef struct orbx_extractor orbx_extractor;

/* ---------------------------------------------------------------------------------------------------
 * Extractor  (replaces ORBextractor, include/ORBextractor.h:43-109)
 * ------------------------------------------------------------------------------------------------- */

/* ORBextractor::ORBextractor (ORBextractor.cc:409-469).  `device` is the HIP device ordinal.  Workspaces are
 * sized lazily for the largest (width, height, batch) seen; max_* are optional pre-allocation hints (0 = lazy). */
int orbx_create(const orbx_params *params, int device, int max_width, int max_height, int max_batch,
                orbx_extractor **out);
void orbx_destroy(orbx_extractor *ex);

/* ORBextractor::operator() (ORBextractor.cc:1086-1168) on a host image (8-bit, 1 channel, `stride` bytes per row).
 * vLappingArea = {lap0, lap1}.  Writes up to `cap` keypoints / 32-byte descriptors; *n_out = number of keypoints,
 * *mono_index = the reference's return value.  Synchronous (H2D, kernels, D2H on the extractor's stream).
 * Returns ORBX_OK, ORBX_E_EMPTY (image NULL or 0-sized: the reference returns -1), or another error. */
int orbx_extract(orbx_extractor *ex, const uint8_t *image, int width, int height, size_t stride, int lap0, int lap1,
                 orbx_keypoint *keypoints, uint8_t *descriptors, int cap, int *n_out, int *mono_index);

/* Batched form over device-resident frames (one camera stream = one extractor = one HIP stream).
 * d_images: device pointer; frame f row y starts at d_images + f*frame_stride + y*row_stride.
 * Enqueues all kernels asynchronously on the extractor's stream; results stay in HBM until downloaded.
 * The extractor's streams are non-blocking: d_images (like every device buffer handed to an orbx_*_device call) must be complete
 * when the call is made, and must stay untouched until orbx_sync / orbx_download_wait. */
int orbx_extract_batch_device(orbx_extractor *ex, const uint8_t *d_images, int n_frames, int width, int height,
                              size_t row_stride, size_t frame_stride, int lap0, int lap1);

/* The same over HOST-resident frames (what the reference hands to operator(): cv::Mat data in host memory, ORBextractor.cc:1086):
 * the frames are copied to the device on the extractor's upload stream into one of two internal input slabs, so the upload
 * of batch i+1 overlaps the kernels of batch i; everything else as orbx_extract_batch_device.  h_images MUST be pinned
 * (hipHostMalloc / hipHostRegister; ORBX_E_BAD_ARG otherwise); it may be reused by the caller as soon as the NEXT call
 * to this function (or orbx_sync) has returned. */
int orbx_extract_batch_host(orbx_extractor *ex, const uint8_t *h_images, int n_frames, int width, int height,
                            size_t row_stride, size_t frame_stride, int lap0, int lap1);

/* ---- raw stereo frames: the rectification in front of the extractor (PARITY UNPINNED) ----
 * System::TrackStereo (System.cc:259-260) runs cv::remap(imLeft, imLeftToFeed, M1l, M2l, cv::INTER_LINEAR) on both images of every frame when
 * settings_->needToRectify() holds; M1 / M2 are the CV_32FC1 maps Settings.cc builds once with initUndistortRectifyMap(..., CV_32F, M1, M2).
 * orbx_rectify_batch_device is that call for 8-bit one-channel images on the device (k_rectify): border mode BORDER_CONSTANT, value 0, the defaults
 * the call in System.cc gets.  Building the maps stays with the caller.  PARITY UNPINNED, as cv::resize and cv::GaussianBlur are: no OpenCV is in
 * the tree, the text below restates OpenCV's imgwarp.cpp (remap, remapBilinear, the float -> fixed-point map conversion), and where an OpenCV at
 * hand disagrees its code wins.  Per destination pixel (x, y):
 *     sx = cvRound(map_x[y][x] * 32),  sy = cvRound(map_y[y][x] * 32)
 *         the product is a float product and exact (the exponent moves); cvRound rounds to nearest, ties to even, and gives INT_MIN when the
 *         product is NaN, infinite or outside int (what the x86 conversion returns; the range is tested here, no conversion is relied on)
 *     a = sx & 31,  b = sy & 31                                            (INTER_BITS = 5)
 *     ix = saturate_cast<short>(sx >> 5),  iy = saturate_cast<short>(sy >> 5)   (arithmetic shifts)
 *     four taps (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1): the source pixel where the tap lies inside [0, src_width) x [0, src_height),
 *         0 otherwise
 *     weights (32 - a)(32 - b) * 32,  a (32 - b) * 32,  (32 - a) b * 32,  a b * 32     (they sum to 32768 = 1 << INTER_REMAP_COEF_BITS)
 *     dst = (sum of tap * weight + 16384) >> 15
 *   - OpenCV's table of `short` weights stores 32767 for a = b = 0 (32768 does not fit) and puts the missing unit elsewhere;
 *     ((32767 p + q + 16384) >> 15) == p for all bytes p, q (checked exhaustively), so the formula above gives the same bytes.
 *   - OpenCV's three border branches (all taps inside, all outside, some outside) all reduce to "a tap outside is 0".
 * orbx_rectifier_create converts the maps to that fixed-point form once (ix, iy, a, b: 6 bytes per destination pixel) and keeps it on `device`.
 * map_x / map_y: HOST float32, dst_height rows of dst_width entries, map_stride floats per row.  Synchronous; the maps are copied and may be freed
 * afterwards.  ORBX_E_BAD_ARG: a NULL pointer, dst_width or dst_height outside [1, 32766], map_stride < dst_width.
 * orbx_rectify_batch_device: n_frames raw images (src_width x src_height, any size; frame f row y at d_src + f*src_frame_stride + y*src_row_stride)
 * -> n_frames rectified images of the maps' size at d_dst, both in DEVICE memory, at any alignment.  One launch on `ex`'s stream, no host wait:
 * orbx_extract_batch_device(ex, d_dst, ...) issued right after it needs no synchronisation in between, whichever route the extraction takes, and
 * neither does anything that batch reads from level 0 later (orbx_stereo_batch_device, orbx_get_level).  d_dst is an input buffer of the extractor in
 * every respect: the rule for d_images above applies to it, and rectifying into it counts as touching it.  d_src must be complete when the call is
 * made and stay untouched until the same wait.  One rectifier may serve several extractors of its device.  ORBX_E_BAD_ARG, before anything is
 * enqueued: a NULL pointer; n_frames < 1; src_width or src_height outside [1, 32766] (above that a saturated `short` would land inside the image);
 * a row stride below its width; for n_frames > 1 a dst_frame_stride below one destination image; a d_dst range that overlaps d_src's; an `ex` on
 * another device than the rectifier's. */
typedef struct orbx_rectifier orbx_rectifier;
int orbx_rectifier_create(int device, const float *map_x, const float *map_y, int dst_width, int dst_height, size_t map_stride, orbx_rectifier **out);
void orbx_rectifier_destroy(orbx_rectifier *r);
int orbx_rectify_batch_device(orbx_rectifier *r, orbx_extractor *ex, const uint8_t *d_src, int n_frames, int src_width, int src_height,
                              size_t src_row_stride, size_t src_frame_stride, uint8_t *d_dst, size_t dst_row_stride, size_t dst_frame_stride);

/* ---- raw frames: colour, size and contrast in front of the extractor (PARITY UNPINNED) ----
 * The other image-sized host steps between the sensor's bytes and ORBextractor::operator():
 *   Tracking::GrabImageMonocular / Stereo / RGBD (Tracking.cc:1569-1582): cvtColor(im, im, COLOR_{RGB,BGR,RGBA,BGRA}2GRAY) for 3 or 4 channels
 *   System::TrackMonocular / Stereo / RGBD: cv::resize(im, im, settings_->newImSize()) when settings_->needToResize() (Camera.newWidth)
 *   the TUM-VI examples: cv::createCLAHE(3.0, cv::Size(8, 8))->apply(im, im) on every frame before System::Track*
 * An integrator chains them in that code's order -- the example's CLAHE, System's resize / remap, Tracking's cvtColor -- or uses any one alone.
 * Each call enqueues its kernels on `ex`'s stream exactly as orbx_rectify_batch_device does: `ex` is passed for the stream and the device only, there is
 * no host wait, orbx_extract_batch_device(ex, d_dst, ...) (or the next of these calls) issued right after needs no synchronisation in between, d_dst is
 * an input buffer of the extractor in every respect (the rule for d_images above), and d_src must be complete when the call is made and stay
 * untouched until the same wait.  Frame f row y lies at d_src + f*src_frame_stride + y*src_row_stride (bytes); source and destination may sit at
 * any alignment.  PARITY UNPINNED, as cv::remap is: no OpenCV is in the tree, the text below restates OpenCV 4.x (color_rgb.simd.hpp, resize.cpp,
 * clahe.cpp), and where an OpenCV at hand disagrees its code wins.
 * ORBX_E_BAD_ARG, before anything is enqueued (d_dst keeps its bytes): a NULL pointer; n_frames < 1; a width or height outside [1, 65535]; a row
 * stride below the row's bytes; for n_frames > 1 a dst_frame_stride below one destination image; a d_dst range that overlaps d_src's (CLAHE's exact
 * in-place form excepted); and what each call adds below.
 *
 * orbx_gray_batch_device (k_gray): channels = 3 or 4 interleaved bytes per pixel (anything else: ORBX_E_BAD_ARG); rgb != 0: the first byte of a pixel
 * is R (Tracking's mbRGB), else B.
 *     gray = (R * 9798 + G * 19235 + B * 3735 + 16384) >> 15
 *   the coefficients sum to 32768; the shift of 15 is OpenCV 4's (ORB-SLAM3 requires OpenCV >= 4.4); a fourth channel is skipped.
 *
 * orbx_resize_batch_device (k_resize, k_resize_half): cv::resize(src, dst, Size(dst_width, dst_height)) with the default INTER_LINEAR, 8-bit one channel.
 *   - exactly src_width == 2 * dst_width && src_height == 2 * dst_height: OpenCV turns INTER_LINEAR into its fast area path,
 *         dst = (a + b + c + d + 2) >> 2 over the 2 x 2 block;
 *   - every other size pair, enlargement and a half in one dimension only included: the generic path.  Per dimension, for destination index d:
 *         f = (float)((d + 0.5) * scale - 0.5), scale = 1. / ((double)dsize / ssize);  s = floor(f);  f -= s
 *         horizontally: s < 0 -> f = 0, s = 0;  s >= ssize - 1 -> f = 0, s = ssize - 1.  Vertically the rows s, s + 1 are clamped to the image, f is kept.
 *         c0 = saturate_cast<short>((1.f - f) * 2048), c1 = saturate_cast<short>(f * 2048)        (cvRound: nearest, ties to even)
 *         row(sy)[x] = S[sy][sx] * c0x + S[sy][sx + 1] * c1x, or S[sy][sx] * 2048 where sx + 1 >= src_width
 *         dst = clamp((((c0y * (row(sy0)[x] >> 4)) >> 16) + ((c1y * (row(sy1)[x] >> 4)) >> 16) + 2) >> 2, 0, 255)
 *     The tables are built on the host and kept on the device per size pair (the last four of an extractor; a new size pair uploads its tables
 *     synchronously, a fifth one waits for the stream first); the kernel does the integer part only.
 *
 * orbx_clahe_batch_device (k_clahe_lut, k_clahe_apply): cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y)) and clahe->apply(src, dst), 8-bit one
 * channel, histSize = 256.  d_dst == d_src with equal strides is allowed (apply(im, im)); any other overlap is refused.
 *   1. If width % tiles_x == 0 && height % tiles_y == 0 the tables are made from the source.  Otherwise from the source extended at the right by
 *      tiles_x - width % tiles_x columns AND at the bottom by tiles_y - height % tiles_y rows with BORDER_REFLECT_101 -- a full extra tiles_y rows when only
 *      the width fails to divide, and the reverse.  (The extension is never materialised: a tile's histogram reads reflected coordinates.)
 *      tile_w, tile_h = the extended size / the tile counts; area = tile_w * tile_h.
 *   2. clip = clip_limit > 0 ? max((int)(clip_limit * area / 256), 1) : 0   (double arithmetic, truncated);  lutScale = 255.0f / area (float).
 *   3. Per tile: the histogram of its `area` pixels.  If clip > 0: clipped = sum of max(hist[i] - clip, 0), those bins set to clip;
 *      batch = clipped / 256, residual = clipped - batch * 256; every bin += batch; if residual != 0: step = max(256 / residual, 1) and
 *      for (i = 0; i < 256 && residual > 0; i += step, residual--) hist[i]++.
 *      lut[i] = saturate_cast<uchar>(cvRound((float)(sum of hist[0..i]) * lutScale))   (one rounded float product; nearest, ties to even)
 *   4. Per source pixel (x, y) of value v: txf = (float)x * (1.0f / tile_w) - 0.5f;  tx1 = floor(txf), tx2 = tx1 + 1;  xa = txf - tx1, xa1 = 1.0f - xa;
 *      THEN tx1 = max(tx1, 0), tx2 = min(tx2, tiles_x - 1); the same in y.
 *      res = (lut[ty1][tx1][v] * xa1 + lut[ty1][tx2][v] * xa) * ya1 + (lut[ty2][tx1][v] * xa1 + lut[ty2][tx2][v] * xa) * ya
 *      in float, every operation rounded as written;  dst = saturate_cast<uchar>(cvRound(res)).
 * orbx_clahe_create: ORBX_E_BAD_ARG for out == NULL, tiles_x or tiles_y outside [1, 64], a NaN clip_limit; clip_limit <= 0 means no clipping.
 * The object owns the tables of the batch in flight (n_frames * tiles_x * tiles_y * 256 bytes), allocated at the first batch and grown when a batch
 * needs more (that call waits for the device).  One object may serve several extractors of its device, PROVIDED TWO BATCHES ARE NEVER IN FLIGHT ON THE
 * SAME OBJECT AT ONCE: batches through one extractor are ordered by its stream; before the object is used with another extractor, wait for the first
 * (orbx_sync / orbx_download_wait).  orbx_clahe_batch_device adds to the refusals: an image in which the padding of step 1 would be at least as wide
 * as the dimension it reflects (pad_x >= width or pad_y >= height); an `ex` on another device than the object's. */
int orbx_gray_batch_device(orbx_extractor *ex, const uint8_t *d_src, int n_frames, int width, int height, int channels, int rgb,
                           size_t src_row_stride, size_t src_frame_stride, uint8_t *d_dst, size_t dst_row_stride, size_t dst_frame_stride);
int orbx_resize_batch_device(orbx_extractor *ex, const uint8_t *d_src, int n_frames, int src_width, int src_height,
                             size_t src_row_stride, size_t src_frame_stride,
                             uint8_t *d_dst, int dst_width, int dst_height, size_t dst_row_stride, size_t dst_frame_stride);
typedef struct orbx_clahe orbx_clahe;
int orbx_clahe_create(int device, double clip_limit, int tiles_x, int tiles_y, orbx_clahe **out);
void orbx_clahe_destroy(orbx_clahe *c);
int orbx_clahe_batch_device(orbx_clahe *c, orbx_extractor *ex, const uint8_t *d_src, int n_frames, int width, int height,
                            size_t src_row_stride, size_t src_frame_stride, uint8_t *d_dst, size_t dst_row_stride, size_t dst_frame_stride);

/* Device-side view of the last batch (valid until the next extract call on this extractor). */
typedef struct orbx_batch_view {
    int32_t n_frames;
    int32_t cap;                    /* per-frame capacity of keypoints / descriptors */
    const orbx_keypoint *d_keypoints; /* [n_frames][cap] */
    const uint8_t *d_descriptors;     /* [n_frames][cap][32] */
    const int32_t *d_count;           /* [n_frames] keypoints per frame */
    const int32_t *d_mono_index;      /* [n_frames] */
    const orbx_keypoint *d_keypoints_un;  /* [n_frames][cap] mvKeysUn: == d_keypoints unless orbx_set_camera gave a distortion model */
} orbx_batch_view;
int orbx_batch_view_get(orbx_extractor *ex, orbx_batch_view *view);

/* Wait for the extractor's stream. */
int orbx_sync(orbx_extractor *ex);
/* D2H of one frame of the last batch (synchronises the stream). */
int orbx_batch_download(orbx_extractor *ex, int frame, orbx_keypoint *keypoints, uint8_t *descriptors, int cap,
                        int *n_out, int *mono_index);
/* D2H of all frames of the last batch into packed host arrays: counts[n_frames], mono[n_frames], keypoints and
 * descriptors laid out [n_frames][cap_per_frame] (cap_per_frame from orbx_output_capacity). Synchronous. */
int orbx_batch_download_all(orbx_extractor *ex, orbx_keypoint *keypoints, uint8_t *descriptors, int32_t *counts,
                            int32_t *mono_index);
int orbx_output_capacity(orbx_extractor *ex, int width, int height);
/* Asynchronous form: the D2H copies run on the extractor's copy stream behind the kernels of the last batch and
 * overlap the kernels of the NEXT batch (which wait for the copy before overwriting the device outputs).
 * Host buffers MUST be pinned (hipHostMalloc / hipHostRegister; ORBX_E_BAD_ARG otherwise).  match / nmatches (optional) receive the internal results of
 * orbx_match_consecutive_device(..., NULL, NULL): [n_frames][cap] / [n_frames].  Up to TWO downloads may be in flight
 * (enqueue batch i+1 before waiting for batch i, so that the matcher of batch i overlaps the pyramid / FAST of batch
 * i+1); orbx_download_wait blocks until the OLDEST one has landed and reports device-side errors. */
int orbx_batch_download_async(orbx_extractor *ex, orbx_keypoint *keypoints, uint8_t *descriptors, int32_t *counts,
                              int32_t *mono_index, int32_t *match, int32_t *nmatches);
int orbx_download_wait(orbx_extractor *ex);

/* mvImagePyramid[level] (public member read by Frame::ComputeStereoMatches, Frame.cc:818,908,923): copies the
 * padded level (19-px REFLECT_101 ring included) of `frame` of the last batch to host memory.
 * dst must hold (h+38) rows of dst_stride >= w+38 bytes; the ROI origin is dst + 19*dst_stride + 19.
 * LEVEL 0 of a batched extraction of ps_min_frames (48) frames or more is not copied into the library's pyramid (its kernels read the caller's
 * frames in place): the first orbx_get_level / orbx_get_level_device of level 0 after such a batch writes the padded level from those frames.
 * After orbx_extract_batch_device that is only possible while the frames are still the library's to read, i.e. BEFORE the orbx_sync /
 * orbx_download_wait that hands them back to the caller (a wait that completes a download issued before the batch does not): afterwards the
 * request fails with ORBX_E_STALE rather than return a level built from whatever the buffer holds by then, and so do orbx_debug_level_blurred,
 * orbx_debug_fused_patches and the extractor's first orbx_stereo_batch_device, which need level 0 too.  The frames of orbx_extract_batch_host live
 * in the library's upload slab, which is kept until the call after the next: level 0 of such a batch can be asked for as long as it is the last
 * batch, also after orbx_sync / orbx_download_wait.  orbx_get_level_device(0) of an in-place batch synchronises the extractor's stream before it
 * returns the pointer; for every other level and batch it is a pure getter. */
int orbx_get_level(orbx_extractor *ex, int frame, int level, uint8_t *dst, size_t dst_stride);
int orbx_level_size(orbx_extractor *ex, int width, int height, int level, int *w, int *h);
/* Device pointer to the padded level (for device-resident consumers such as the stereo matcher). */
int orbx_get_level_device(orbx_extractor *ex, int frame, int level, const uint8_t **d_padded, size_t *pitch);

/* GetLevels / GetScaleFactor(s) / GetInverseScaleFactors / GetScaleSigmaSquares / GetInverseScaleSigmaSquares
 * (ORBextractor.h:62-83).  Arrays hold nlevels floats; any pointer may be NULL. */
int orbx_get_levels(const orbx_extractor *ex);
float orbx_get_scale_factor(const orbx_extractor *ex);
int orbx_get_scale_tables(const orbx_extractor *ex, float *scale, float *inv_scale, float *sigma2, float *inv_sigma2);
/* mnFeaturesPerLevel (nlevels ints) and umax (16 ints) -- for known-answer tests */
int orbx_get_feature_tables(const orbx_extractor *ex, int32_t *features_per_level, int32_t *umax16);

/* Stage introspection of the last batch (parity tests): FAST candidates of a level in reference order
 * (x, y relative to the 16-px border; response = score) and the level's keypoints after the quad-tree cull
 * (level coordinates).  Return the count, or < 0. */
int orbx_debug_level_candidates(orbx_extractor *ex, int frame, int level, orbx_keypoint *out, int cap);
int orbx_debug_level_keypoints(orbx_extractor *ex, int frame, int level, orbx_keypoint *out, int cap);
int orbx_debug_level_blurred(orbx_extractor *ex, int frame, int level, uint8_t *dst, size_t dst_stride);
/* The blur on demand of k_describe_fused (no blurred pyramid exists then): the 37 x 37 blurred pixels around keypoint k of `frame` of the last batch,
 * dst[k][37][37] for the first min(count, cap_keypoints) keypoints in OUTPUT order, centre = the keypoint's level pixel; pixels outside the level are
 * its BORDER_REFLECT_101 extension.  Re-runs the descriptor kernel of the last batch, so it is refused with ORBX_E_STALE once level 0 was read in
 * place from frames that have been released (orbx_get_level).  Returns the number of patches, or < 0 (ORBX_E_BAD_ARG when the extractor uses the
 * blurred slab: orbx_debug_level_blurred). */
int orbx_debug_fused_patches(orbx_extractor *ex, int frame, uint8_t *dst, int cap_keypoints);
/* Which paths the last batch took (bench / stress tests): out[0] = cells that went to the FAST list pass (k_fast_wave_list: corners at iniThFAST
 * that all lost the NMS, or a strip / cell whose candidate queue overflowed), out[1] = cells of the batch, out[2..4] = (frame, level) quad-trees with
 * <= 1792 / <= 4096 / more candidates (the two 256-thread tiers and the single-wave chunked form), out[5] = FAST candidates of the batch,
 * out[6] = the largest candidate count of a level.  Returns the number of entries written (7), or < 0. */
int orbx_debug_stage_stats(orbx_extractor *ex, int64_t *out, int cap);

/* The FAST stage's candidate queues.  k_fast_strip keeps the pixels that pass its pre-tests in per-wave LDS queues sized for sparse scenes (the default
 * leaves seven workgroups on a CU); a strip whose queue overflows is finished by the list pass (k_fast_wave_list) -- the RESULTS never depend on the
 * queue size, only the time does (dense texture: two thirds of the cells take the list pass, the stage is 4 x slower).  This call looks at the LAST batch
 * (it waits for it): mode 0 reports only; mode 1 doubles the queues (up to "every pixel of a wave's band") when more than a tenth of the batch's cells
 * went to the list pass, and halves them again (never below the default) when fewer than 1 in 200 did while the queues are enlarged; mode 2 restores the
 * default.  A caller with unknown imagery runs it after each of its first few batches (orb_slam3_amd.ORBextractor.tune_fast_queues, bench.py --scene
 * texture).  info[0] = cells of the last batch that took the list pass, info[1] = cells of the batch, info[2] / info[3] = group / pixel queue entries per
 * wave now in force.  Returns 1 if the sizes changed, 0 if not, < 0 on error. */
int orbx_tune_fast_queues(orbx_extractor *ex, int mode, int32_t info[4]);

/* Average GPU time (ms) per launch of each extractor kernel over the calls since the last reset, measured with
 * HIP events on the extractor's stream when profiling is enabled.  names/ms arrays of `cap` entries; returns the
 * number of kernels. */
int orbx_profile_enable(orbx_extractor *ex, int enable);
int orbx_profile_read(orbx_extractor *ex, const char **names, double *avg_ms, int64_t *launches, int cap);

/* ---------------------------------------------------------------------------------------------------
 * Matcher  (replaces ORBmatcher, include/ORBmatcher.h:36-103, and the Hamming stages of Frame.cc)
 * One context per host thread (own HIP stream): re-entrant across Tracking / LocalMapping / LoopClosing.
 * ------------------------------------------------------------------------------------------------- */
typedef struct orbx_matcher orbx_matcher;
int orbx_matcher_create(int device, orbx_matcher **out);
void orbx_matcher_destroy(orbx_matcher *m);
/* Transfers of the context's LAST call (test hook; host-pointer entry points): out[0] = host-to-device transfers submitted (one per run of adjacent
 * buffers), out[1] = device-to-host ones, out[2] / out[3] = their bytes; with cap >= 6 also out[4] = how many of them a DMA engine carried
 * (hipMemcpyAsync) and out[5] = k_xfer launches.  A call stages its inputs in a pinned, device-visible mirror of its device arena; runs up to 1 MiB are
 * moved by the lanes of a k_xfer launch in the call's own queue (a projection-matcher call: 1 run up, 1 down, 2 launches, no DMA submission), larger
 * ones by the DMA engine; ORBX_MATCHER_DMA=1 sends everything through the DMA engine (round 5's transport).  Returns the entries written, or < 0. */
int orbx_matcher_debug_transfers(const orbx_matcher *m, int64_t *out, int cap);
/* Test hook: the replay of the context's last orbx_search_for_initialization (k_replay_init_lists): out3[0] = rounds of its chunk loop, out3[1] = queries whose
 * candidate list ran dry and were re-scanned by the whole wave, out3[2] = queries (level-0 keypoints of F1).  Returns 3, or < 0. */
int orbx_matcher_debug_replay_stats(const orbx_matcher *m, int32_t *out3);

/* ORBmatcher::TH_LOW / TH_HIGH / HISTO_LENGTH (ORBmatcher.cc:35-37) */
#define ORBX_TH_LOW 50
#define ORBX_TH_HIGH 100
#define ORBX_HISTO_LENGTH 30

/* ORBmatcher::DescriptorDistance (ORBmatcher.cc:2058-2074) for every candidate of a CSR candidate list:
 * query i is compared with train rows cand[row_ptr[i] .. row_ptr[i+1]); dist_out[k] = Hamming(q_i, t_cand[k]).
 * Host pointers; synchronous.  The caller replays best / second-best / ratio / taken-mask logic in reference order. */
int orbx_hamming_csr(orbx_matcher *m, const uint8_t *q_desc, int n_q, const uint8_t *t_desc, int n_t,
                     const int32_t *row_ptr, const int32_t *cand, uint16_t *dist_out);

/* Best and second-best candidate per query, ties resolved to the EARLIEST candidate position (strict '<' scan,
 * as every matcher except SearchForTriangulation does).  best_pos/second_pos are positions inside the query's
 * candidate list (-1 if none); distances are 256 if none. */
int orbx_hamming_best2_csr(orbx_matcher *m, const uint8_t *q_desc, int n_q, const uint8_t *t_desc, int n_t,
                           const int32_t *row_ptr, const int32_t *cand, int32_t *best_pos, int32_t *best_dist,
                           int32_t *second_pos, int32_t *second_dist);

/* cv::BFMatcher(NORM_HAMMING).knnMatch(query, train, k=2) as used by Frame::ComputeStereoFishEyeMatches
 * (Frame.cc:1144): idx[2*i], idx[2*i+1] = best / second-best train row (lower index wins ties), -1 if absent. */
int orbx_knn2(orbx_matcher *m, const uint8_t *q_desc, int n_q, const uint8_t *t_desc, int n_t, int32_t *idx,
              int32_t *dist);

/* Hamming stage of Frame::ComputeStereoMatches (Frame.cc:849-894): for each left keypoint the best right keypoint
 * among those registered on row (int)yL with |octave difference| <= 1 and uL-maxD <= uR <= uL-minD.
 * best_idx_r = -1 / best_dist = ORBX_TH_HIGH when no candidate is closer than TH_HIGH. */
int orbx_stereo_rowband(orbx_matcher *m, const orbx_keypoint *kp_left, const uint8_t *desc_left, int n_left,
                        const orbx_keypoint *kp_right, const uint8_t *desc_right, int n_right,
                        const float *scale_factors, int nlevels, int n_rows, float min_d, float max_d,
                        int32_t *best_idx_r, int32_t *best_dist);

/* Frame::ComputeStereoMatches complete (Frame.cc:811-981): row-band Hamming + 11x11 SAD sub-pixel refinement on the
 * pyramid levels + median outlier rejection.  pyr_left/right[l] point at the level ROI origin (host memory),
 * as mvImagePyramid[l] does.  Fills u_right[n_left], depth[n_left] (-1 where unmatched); returns #matches. */
int orbx_compute_stereo_matches(orbx_matcher *m, const orbx_keypoint *kp_left, const uint8_t *desc_left, int n_left,
                                const orbx_keypoint *kp_right, const uint8_t *desc_right, int n_right,
                                const float *scale_factors, const float *inv_scale_factors, int nlevels,
                                const uint8_t *const *pyr_left, const uint8_t *const *pyr_right, const int32_t *pyr_w,
                                const int32_t *pyr_h, const size_t *pyr_stride, float bf, float b, float *u_right,
                                float *depth);

/* Frame description for the projection matchers: undistorted keypoints (mvKeysUn), descriptors, image bounds
 * (mnMinX..mnMaxY) from which the 64x48 grid (Frame.h:44-45, Frame.cc:385-416) is built, per-level scale factors,
 * optional right coordinates (mvuRight, NULL for mono).  n <= ORBX_MAX_FRAME_FEATURES for the projection matchers
 * (ORBX_E_TOO_LARGE otherwise, checked before any work is enqueued). */
#define ORBX_MAX_FRAME_FEATURES 16000
typedef struct orbx_frame_desc {
    const orbx_keypoint *keypoints_un;
    const uint8_t *descriptors;
    int32_t n;
    float min_x, max_x, min_y, max_y;
    const float *scale_factors;
    int32_t nlevels;
    const float *u_right;
} orbx_frame_desc;

/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints)
 * (ORBmatcher.cc:43-213), monocular / rectified-stereo form (Nleft == -1).  Map points are passed flattened:
 * the MapPoint scratch fields the loop reads (MapPoint.h:171-179) and a 32-byte descriptor each.
 * mp_in_view[j] != 0  <=> mbTrackInView && !isBad() && !(bFarPoints && mTrackDepth > thFarPoints).
 * frame_occupied[i] != 0 <=> F.mvpMapPoints[i] != NULL with Observations() > 0 on entry (may be NULL).
 * mp_has_obs[j] = Observations() > 0 of map point j (may be NULL = all true).
 * Output frame_match[i] = j if map point j was assigned to feature i, else -1.  Returns nmatches (>= 0). */
int orbx_search_by_projection_mappoints(orbx_matcher *m, const orbx_frame_desc *frame, const uint8_t *frame_occupied,
                                        int n_mp, const float *proj_x, const float *proj_y, const float *proj_xr,
                                        const int32_t *pred_level, const float *view_cos, const uint8_t *mp_desc,
                                        const uint8_t *mp_in_view, const uint8_t *mp_has_obs, float th, float nnratio,
                                        int32_t *frame_match);

/* ORBmatcher::SearchByProjection(Frame& Cur, const Frame& Last, th, bMono) (ORBmatcher.cc:1676-1887) after the
 * adapter has projected the last frame's map points (one query per point that passed the projection gates).
 * level_mode: 0 = [o-1, o+1], 1 = forward [o, inf), 2 = backward [0, o].  Rotation-histogram filter applied when
 * check_orientation != 0.  cur_match[i] = query index, -1 (never assigned: the slot keeps what it held), or -2 (assigned by the
 * loop and then cleared by the rotation check: the reference leaves NULL there, ORBmatcher.cc:1871-1881).  Returns nmatches. */
int orbx_search_by_projection_frame(orbx_matcher *m, const orbx_frame_desc *cur, const uint8_t *cur_occupied, int n_q,
                                    const float *q_u, const float *q_v, const float *q_ur, const int32_t *q_octave,
                                    const float *q_angle, const uint8_t *q_desc, const uint8_t *q_has_obs, float th,
                                    int level_mode, int check_orientation, int32_t *cur_match);

/* General window form of the projection matchers: one query per projected map point with explicit window half-size
 * and level range; accept iff (float)bestDist <= max_dist; a matched feature becomes occupied (q_has_obs NULL = always).
 *   SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)  (ORBmatcher.cc:1889-2010):
 *       r = th*scale[lvl], levels [lvl-1, lvl+1], max_dist = ORBdist, rotation check, occupied = mvpMapPoints[i] != NULL
 *   SearchByProjection(KeyFrame*, Sim3f&, vpPoints[, vpPointsKFs], vpMatched[, vpMatchedKF], th, ratioHamming)
 *       (ORBmatcher.cc:427-532, 534-646): r = th*scale[lvl], levels [lvl-1, lvl], max_dist = TH_LOW*ratioHamming,
 *       no rotation check, occupied = vpMatched[i] != NULL
 * match[i] = query index or -1.  Returns nmatches. */
int orbx_search_by_projection_window(orbx_matcher *m, const orbx_frame_desc *frame, const uint8_t *occupied, int n_q,
                                     const float *q_x, const float *q_y, const float *q_r, const int32_t *q_min_level,
                                     const int32_t *q_max_level, const float *q_angle, const uint8_t *q_desc,
                                     const uint8_t *q_has_obs, float max_dist, int check_orientation, int32_t *match);

/* ---- device-resident frame handle ----
 * In the reference one Frame is built once (ExtractORB -> UndistortKeyPoints -> AssignFeaturesToGrid, Frame.cc:311-367) and then searched by three
 * to five matcher calls (Tracking.cc:2886,2894,3377,3413).  An orbx_frame keeps such a frame on the device across calls: undistorted keypoints,
 * descriptors, optional mvuRight, the count, the scale factors and the 64x48 grid, in buffers of its own for `cap` features.
 * It belongs to the matcher that created it (its device, its stream): every load and every use is ordered on that stream, and a handle passed to
 * another matcher is refused with ORBX_E_BAD_ARG.  Destroy the handles of a matcher before the matcher.
 *   orbx_frame_create: cap <= ORBX_MAX_FRAME_FEATURES (ORBX_E_TOO_LARGE otherwise).  A new handle holds an empty frame.
 *   orbx_frame_load_host: uploads the frame once (desc->n <= cap) and builds the grid.  Returns without waiting for the upload.
 *   orbx_frame_load_batch: frame `frame` of the extractor's last batch (orbx_batch_view: d_keypoints_un, d_descriptors, d_count); bounds4 =
 *     {mnMinX, mnMaxX, mnMinY, mnMaxY} (NULL: the extractor's camera / image rectangle), scale_factors[nlevels] (NULL: the extractor's).
 *     Asynchronous: the matcher's stream waits for the extraction, no host synchronisation, nothing passes through host memory.  The handle
 *     holds a COPY: the extractor's next batch waits for it, and later extract calls do not change what the handle holds.  ORBX_E_BAD_ARG when
 *     the frame index is not one of the batch, `ex` is on another device, or the batch's per-frame capacity exceeds `cap`.  No mvuRight.
 *   orbx_frame_count: N, synchronising the matcher's stream once if the count is still on the device (cached until the next load).
 * A handle holds a monocular / rectified frame (these loads) or a fisheye-stereo frame (orbx_frame_load_host_fisheye,
 * orbx_frame_load_stereo_fisheye_batch, below); each kind's entry points refuse the other kind with ORBX_E_BAD_ARG (the `_fisheye` forms of
 * ComputeBoW, SearchByBoW and the window search: after orbx_frame_search_by_projection_window).
 * Checks that fail return before anything is enqueued. */
typedef struct orbx_frame orbx_frame;
int orbx_frame_create(orbx_matcher *m, int cap, orbx_frame **out);
void orbx_frame_destroy(orbx_frame *f);
int orbx_frame_load_host(orbx_frame *f, const orbx_frame_desc *desc);
int orbx_frame_load_batch(orbx_frame *f, orbx_extractor *ex, int frame, const float *bounds4, const float *scale_factors, int nlevels);
int orbx_frame_count(orbx_frame *f, int *n);
/* Handle forms of the two projection matchers: arguments, outputs and results of orbx_search_by_projection_mappoints /
 * orbx_search_by_projection_frame with the resident frame in place of the orbx_frame_desc; frame_match / cur_match hold N entries.
 * The occupancy mask (N entries, may be NULL) comes from the host on every call.  Results equal the host-pointer forms' bit for bit. */
int orbx_frame_search_by_projection_mappoints(orbx_matcher *m, orbx_frame *frame, const uint8_t *frame_occupied, int n_mp, const float *proj_x,
                                              const float *proj_y, const float *proj_xr, const int32_t *pred_level, const float *view_cos,
                                              const uint8_t *mp_desc, const uint8_t *mp_in_view, const uint8_t *mp_has_obs, float th, float nnratio,
                                              int32_t *frame_match);
int orbx_frame_search_by_projection_frame(orbx_matcher *m, orbx_frame *cur, const uint8_t *cur_occupied, int n_q, const float *q_u, const float *q_v,
                                          const float *q_ur, const int32_t *q_octave, const float *q_angle, const uint8_t *q_desc,
                                          const uint8_t *q_has_obs, float th, int level_mode, int check_orientation, int32_t *cur_match);
/* orbx_frame_search_local_points: below, after orbx_camera / orbx_frame_pose. */

/* ---- fisheye-stereo frames on the handle (Frame::Nleft != -1: KannalaBrandt8 stereo rigs) ----
 * Numbering as the host-pointer fisheye forms (below): features [0, N_left) = left camera, [N_left, N) = right camera; occupancy masks and match
 * arrays hold N entries.  cap covers both cameras.
 *   orbx_frame_load_host_fisheye: left->keypoints_un = mvKeys, left->n = N_left, left->descriptors = ALL N rows; kps_right = mvKeysRight [n_right];
 *     l2r [N_left] = mvLeftToRightMatch, r2l [n_right] = mvRightToLeftMatch (-1 = none).  ORBX_E_BAD_ARG when l2r[i] is not in [-1, n_right) or
 *     r2l[j] not in [-1, N_left); ORBX_E_TOO_LARGE when N > cap.  Returns without waiting for the upload.
 *   orbx_frame_load_stereo_fisheye_batch: frame `frame` of the last orbx_stereo_fisheye_batch_device(left, right, ...): both extractors' RAW
 *     keypoints (mvKeys / mvKeysRight: what the stage triangulated), descriptors and counts, and the stage's l2r / r2l rows -- copied on the device.
 *     bounds4 / scale_factors as orbx_frame_load_batch (NULL: the left extractor's).  Asynchronous, no host synchronisation: the matcher's stream
 *     waits for the stage; both extractors' next batches and the left extractor's next fisheye stage wait for the copy.  The counts stay on the
 *     device until a search returns them (or orbx_frame_counts).  ORBX_E_BAD_ARG when the stage's results are not those of the extractors'
 *     current batches (an extraction since the stage, another right extractor), the frame is not one of the batch, an extractor is on another
 *     device, or cap_left + cap_right > cap.
 *   orbx_frame_counts: N_left and N_right (n_right = -1 for a monocular / rectified frame, as Frame::Nleft == -1); synchronises like orbx_frame_count. */
int orbx_frame_load_host_fisheye(orbx_frame *f, const orbx_frame_desc *left, const orbx_keypoint *kps_right, int n_right, const int32_t *l2r,
                                 const int32_t *r2l);
int orbx_frame_load_stereo_fisheye_batch(orbx_frame *f, orbx_extractor *left, orbx_extractor *right, int frame, const float *bounds4,
                                         const float *scale_factors, int nlevels);
int orbx_frame_counts(orbx_frame *f, int *n_left, int *n_right);
/* Handle forms of orbx_search_by_projection_mappoints_fisheye (M1, ORBmatcher.cc:43-213 whole) and orbx_search_by_projection_frame_fisheye
 * (M2, :1676-1887 with :1794-1863): the same arguments and results with the frame, kps_right, l2r and r2l taken from the handle; frame_match /
 * cur_match hold N entries (the handle's capacity while the counts are still on the device: N comes back with the results).  Bit for bit the
 * host-pointer forms' results. */
int orbx_frame_search_by_projection_mappoints_fisheye(orbx_matcher *m, orbx_frame *f, const uint8_t *frame_occupied, int n_mp, const uint8_t *in_view,
                                                      const float *proj_x, const float *proj_y, const int32_t *pred_level, const float *view_cos,
                                                      const uint8_t *in_view_r, const float *proj_xr, const float *proj_yr, const int32_t *pred_level_r,
                                                      const float *view_cos_r, const uint8_t *mp_desc, const uint8_t *mp_has_obs, float th, float nnratio,
                                                      int32_t *frame_match);
int orbx_frame_search_by_projection_frame_fisheye(orbx_matcher *m, orbx_frame *f, const uint8_t *cur_occupied, int n_q, const float *q_u, const float *q_v,
                                                  const float *q_ur, const float *q_vr, const int32_t *q_octave, const float *q_angle, const uint8_t *q_desc,
                                                  const uint8_t *q_has_obs, float th, int level_mode, int check_orientation, int32_t *cur_match);
/* orbx_frame_search_local_points_fisheye: below, after orbx_fisheye_view. */

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (ORBmatcher.cc:648-763).
 * prev_matched: n1 (x, y) pairs, updated in place (:757-760).  matches12[i1] = index in F2 or -1. */
int orbx_search_for_initialization(orbx_matcher *m, const orbx_keypoint *kps1_un, const uint8_t *desc1, int n1,
                                   const orbx_frame_desc *F2, float *prev_matched, int window_size, float nnratio,
                                   int check_orientation, int32_t *matches12);

/* DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned int>>) flattened: node ids ascending + CSR of indices */
typedef struct orbx_featvec {
    const uint32_t *node_id;
    const int32_t *node_ptr;   /* n_nodes + 1 */
    const int32_t *index;
    int32_t n_nodes;
} orbx_featvec;

/* ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (ORBmatcher.cc:223-425, monocular).
 * kf_valid[i] != 0 <=> KF feature i has a good map point.  f_match[iF] = KF feature index or -1. */
int orbx_search_by_bow_frame(orbx_matcher *m, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_valid,
                             int n_kf, const orbx_featvec *kf_fv, const uint8_t *f_desc, const float *f_angle, int n_f,
                             const orbx_featvec *f_fv, float nnratio, int check_orientation, int32_t *f_match);
/* ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (ORBmatcher.cc:765-905).  match12[i1] = i2 or -1 */
int orbx_search_by_bow_keyframes(orbx_matcher *m, const uint8_t *desc1, const float *angle1, const uint8_t *valid1,
                                 int n1, const orbx_featvec *fv1, const uint8_t *desc2, const float *angle2,
                                 const uint8_t *valid2, int n2, const orbx_featvec *fv2, float nnratio,
                                 int check_orientation, int32_t *match12);
/* ORBmatcher::SearchForTriangulation (ORBmatcher.cc:907-1146).  skipN[i] != 0 <=> feature i already has a map point
 * (or fails bOnlyStereo).  pair_ok(user, idx1, idx2) evaluates the geometric gates of :1026-1072 (epipole distance,
 * epipolarConstrain unless bCoarse) -- host float math that stays in the adapter; NULL = always true.
 * matches12[i1] = idx2 or -1 (vMatchedPairs = the pairs with matches12[i1] >= 0 in i1 order). */
typedef int (*orbx_pair_predicate)(void *user, int idx1, int idx2);
int orbx_search_for_triangulation(orbx_matcher *m, const uint8_t *desc1, const float *angle1, const uint8_t *skip1, int n1,
                                  const orbx_featvec *fv1, const uint8_t *desc2, const float *angle2, const uint8_t *skip2,
                                  int n2, const orbx_featvec *fv2, int check_orientation, orbx_pair_predicate pair_ok,
                                  void *user, int32_t *matches12);

/* SearchForTriangulation for PINHOLE key frames with both geometric gates evaluated on the device -- no callback:
 *  - epipole distance, src/ORBmatcher.cc:1026-1034 (pairs where neither feature is stereo): (ex-x2)^2 + (ey-y2)^2 <
 *    100 * pKF2->mvScaleFactors[kp2.octave] rejects; (ep_x, ep_y) = pKF2->mpCamera->project(T2w * Cw) (:919-921);
 *  - Pinhole::epipolarConstrain, src/CameraModels/Pinhole.cpp:107-129, on the caller's F12 = K1^-T [t12]x R12 K2^-1 (row-major;
 *    the 3x3 algebra stays with the caller's Eigen): dsqr < 3.84 * pKF2->mvLevelSigma2[kp2.octave]; skipped when coarse (bCoarse).
 * strict_fp = 0 applies the FMA contraction GCC -O3 -march=native gives the reference's text, 1 rounds
 * every operation separately.  skip1/skip2, feature vectors, check_orientation, matches12 and the return value as in
 * orbx_search_for_triangulation; rotation uses kps*_un[i].angle (:1086-1094). */
typedef struct orbx_pinhole_gate {
    const orbx_keypoint *kps1_un, *kps2_un; /* pKF1/pKF2->mvKeysUn */
    const float *u_right1, *u_right2;       /* mvuRight, NULL = monocular (all < 0) */
    const float *scale_factors2;            /* pKF2->mvScaleFactors [nlevels] */
    const float *level_sigma2_2;            /* pKF2->mvLevelSigma2 [nlevels] */
    int nlevels;
    float F12[9];
    float ep_x, ep_y;
    int coarse;
    int strict_fp;
} orbx_pinhole_gate;
int orbx_search_for_triangulation_pinhole(orbx_matcher *m, const uint8_t *desc1, const uint8_t *skip1, int n1, const orbx_featvec *fv1,
                                          const uint8_t *desc2, const uint8_t *skip2, int n2, const orbx_featvec *fv2,
                                          int check_orientation, const orbx_pinhole_gate *gate, int32_t *matches12);

/* SearchForTriangulation between two key frames of a FISHEYE rig (pKF1->mpCamera2 && pKF2->mpCamera2) with the geometric gate on the device -- no callback:
 * src/ORBmatcher.cc:1036-1072 picks, per candidate pair, the cameras the two features were seen by (idx < NLeft: left) and the relative pose of that camera pair,
 * then KannalaBrandt8::epipolarConstrain (src/CameraModels/KannalaBrandt8.cpp:216-221 = TriangulateMatches :305-368 > 0.0001: unproject both keypoints,
 * parallax test, Triangulate :387-400 (Eigen::JacobiSVD of the 4x4 system), depth tests, reprojection errors against 5.991 * mvLevelSigma2); skipped when coarse.
 * There is no epipole-distance test for such key frames (:1026).  Float operations round as the reference text writes them; atan2f / tanf are glibc's restated
 * bit for bit, cos / sin evaluate in double as the reference's translation unit does; Eigen's JacobiSVD is restated from its published source (Eigen is not
 * vendored by the reference: that step's parity is UNPINNED -- DESIGN.md section 5).
 * kps1 / kps2: ALL features of the key frame, [0, n_left) = mvKeys, [n_left, N) = mvKeysRight (pt, octave, angle are read).
 * cam1[0] / cam1[1] = mvParameters (fx, fy, cx, cy, k0..k3) of pKF1->mpCamera / mpCamera2, cam2 likewise for pKF2.
 * R12 / t12 [2 * right1 + right2] = Rll tll, Rlr tlr, Rrl trl, Rrr trr of :934-944 (row-major), computed by the caller's Sophus as the reference does. */
typedef struct orbx_kb8_gate {
    const orbx_keypoint *kps1, *kps2;
    int n_left1, n_left2;
    const float *level_sigma2_1, *level_sigma2_2; /* mvLevelSigma2 of pKF1 / pKF2 [nlevels] */
    int nlevels;
    float cam1[2][8], cam2[2][8];
    float R12[4][9], t12[4][3];
    int coarse;
} orbx_kb8_gate;
int orbx_search_for_triangulation_kb8(orbx_matcher *m, const uint8_t *desc1, const uint8_t *skip1, int n1, const orbx_featvec *fv1, const uint8_t *desc2,
                                      const uint8_t *skip2, int n2, const orbx_featvec *fv2, int check_orientation, const orbx_kb8_gate *gate,
                                      int32_t *matches12);

/* Test hook: KannalaBrandt8::epipolarConstrain (src/CameraModels/KannalaBrandt8.cpp:216-221) of n independent keypoint pairs evaluated on the device, one verdict
 * per pair -- the gate of orbx_search_for_triangulation_kb8 on its own.  cam1 / cam2: [2][8] parameters of (mpCamera, mpCamera2); R12 [4][9] / t12 [4][3] as in
 * orbx_kb8_gate; sel[i] = 2 * right1 + right2 picks the cameras and the pose of pair i; sigma1 / sigma2: the two level variances per pair. */
int orbx_debug_kb8_epipolar(orbx_matcher *m, const float *cam1_2x8, const float *cam2_2x8, const float *R12_4x9, const float *t12_4x3, int n, const float *xy1,
                            const float *xy2, const float *sigma1, const float *sigma2, const uint8_t *sel, uint8_t *ok);

/* ---- Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1126-1166) on the device: the rig's two KannalaBrandt8 cameras, no callback ----
 * kNN-2 of the two lapping-area tails (BFmatcher.knnMatch, :1144: ties to the lower train index), Lowe's ratio as :1151 writes it ((float)d0 < (float)d1 * 0.7,
 * float against double; a missing second neighbour fails), then KannalaBrandt8::TriangulateMatches (src/CameraModels/KannalaBrandt8.cpp:305-368) of mvKeys[iL]
 * (cam1 = mpCamera) and mvKeysRight[iR] (cam2 = mpCamera2) with R12 = mRlr, t12 = mtlr and both level variances from the frame's mvLevelSigma2 (:1155).
 * depth > 0.0001f accepts (:1157): mvLeftToRightMatch[iL] = iR, mvRightToLeftMatch[iR] = iL (of two accepted queries on one iR the larger iL, the
 * reference's later one), mvDepth[iL], mvStereo3Dpoints[iL] = x3D.  Every output is initialised over the whole frame as :1134-1138 (l2r / r2l / depth = -1,
 * p3d = 0); mvuRight stays -1 (the caller's).  The same device function as orbx_search_for_triangulation_kb8's gate: atan2f / tanf restated from glibc bit
 * for bit, cos / sin in double, Eigen's JacobiSVD restated from its published source -- that step's parity is UNPINNED (Eigen is not vendored by the
 * reference: DESIGN.md section 5). */
typedef struct orbx_kb8_rig {   /* Frame::mpCamera / mpCamera2 mvParameters (fx, fy, cx, cy, k0..k3), mRlr (row-major), mtlr */
    float cam_left[8], cam_right[8], R_lr[9], t_lr[3];
} orbx_kb8_rig;
/* on host arrays: returns nMatches; l2r / depth [n_left], p3d [n_left][3], r2l [n_right]; *desc_matches = the pairs that passed the ratio test (may be NULL).
 * ORBX_E_BAD_ARG before any device work for mono_left outside [0, n_left], mono_right outside [0, n_right], a NULL array that is needed, or an octave outside
 * [0, nlevels).  One launch chain and one synchronisation in the matcher's queue. */
int orbx_compute_stereo_fisheye_matches(orbx_matcher *m, const orbx_kb8_rig *rig, const orbx_keypoint *kps_left, const uint8_t *desc_left, int n_left,
                                        int mono_left, const orbx_keypoint *kps_right, const uint8_t *desc_right, int n_right, int mono_right,
                                        const float *level_sigma2, int nlevels, int32_t *l2r, int32_t *r2l, float *depth, float *p3d, int *desc_matches);
/* the same for every frame pair of two resident batches (left / right extractor: same n_frames, same nlevels, same device): the extractors' raw keypoints
 * (mvKeys), counts and mono indices, the LEFT extractor's mvLevelSigma2.  Runs on the left extractor's match stream behind both extractions; the next pair
 * of batches may be extracted meanwhile (both extractors' next k_finalize waits for this stage).  Reads no pyramid level.  Results stay valid until the next
 * call of this function on `left`. */
int orbx_stereo_fisheye_batch_device(orbx_extractor *left, orbx_extractor *right, const orbx_kb8_rig *rig);
/* one frame: l2r / depth [n_left], p3d [n_left][3], r2l [n_right], the counts (any pointer may be NULL); synchronous */
int orbx_stereo_fisheye_batch_download(orbx_extractor *left, int frame, int32_t *l2r, int32_t *r2l, float *depth, float *p3d, int *n_left, int *n_right,
                                       int *n_matches, int *desc_matches);
/* all frames: l2r / depth [n_frames][cap_left], p3d [n_frames][cap_left][3], r2l [n_frames][cap_right] (caps = orbx_batch_view_get's cap of each extractor;
 * entries beyond a frame's counts unspecified), n_matches / desc_matches [n_frames]; synchronous */
int orbx_stereo_fisheye_batch_download_all(orbx_extractor *left, int32_t *l2r, int32_t *r2l, float *depth, float *p3d, int32_t *n_matches,
                                           int32_t *desc_matches);

/* ---- fisheye-stereo forms (F.Nleft != -1: KannalaBrandt8 stereo rigs, both cameras' features in one Frame) ----
 * Feature indices follow the reference: [0, n_left) = left camera (F.mvKeys), [n_left, n_left + n_right) = right camera
 * (F.mvKeysRight); `left` describes the left camera (keypoints_un = mvKeys, n = n_left, image bounds, scale factors) and its
 * `descriptors` field points at ALL n_left + n_right rows of F.mDescriptors; occupied / match arrays cover all features.
 *
 * SearchByProjection(Frame&, const vector<MapPoint*>&, th, ...) ORBmatcher.cc:43-213 whole: per map point the left search and then
 * the right-camera twin (:144-210) with mbTrackInViewR / mTrackProjXR,YR / mnTrackScaleLevelR / mTrackViewCosR; an accepted match
 * is also written to the stereo partner's slot (mvLeftToRightMatch / mvRightToLeftMatch, -1 = none) and counts twice. */
int orbx_search_by_projection_mappoints_fisheye(orbx_matcher *m, const orbx_frame_desc *left, const orbx_keypoint *kps_right, int n_right,
                                                const int32_t *left_to_right, const int32_t *right_to_left, const uint8_t *frame_occupied,
                                                int n_mp, const uint8_t *in_view, const float *proj_x, const float *proj_y,
                                                const int32_t *pred_level, const float *view_cos, const uint8_t *in_view_r,
                                                const float *proj_xr, const float *proj_yr, const int32_t *pred_level_r,
                                                const float *view_cos_r, const uint8_t *mp_desc, const uint8_t *mp_has_obs, float th,
                                                float nnratio, int32_t *frame_match);
/* SearchByProjection(Frame& Cur, const Frame& Last, th, bMono) ORBmatcher.cc:1676-1887 incl. the right-camera twin :1794-1863:
 * (q_u, q_v) = projection into the left camera, (q_ur, q_vr) = projection of Trl * x3Dc into the right camera.  cur_match as in
 * orbx_search_by_projection_frame (-2 = assigned, then cleared by the rotation check). */
int orbx_search_by_projection_frame_fisheye(orbx_matcher *m, const orbx_frame_desc *left, const orbx_keypoint *kps_right, int n_right,
                                            const uint8_t *cur_occupied, int n_q, const float *q_u, const float *q_v, const float *q_ur,
                                            const float *q_vr, const int32_t *q_octave, const float *q_angle, const uint8_t *q_desc,
                                            const uint8_t *q_has_obs, float th, int level_mode, int check_orientation, int32_t *cur_match);
/* SearchByBoW(KeyFrame*, Frame&, ...) for a fisheye-stereo frame, ORBmatcher.cc:283-392: frame features >= n_f_left are the right
 * camera's; best / second best are kept per camera, the right match is taken only inside the left `bestDist1 <= TH_LOW` branch and
 * its ratio test is disabled by the reference's `|| true` (:359).  f_angle covers all n_f features (mvKeys then mvKeysRight). */
int orbx_search_by_bow_frame_fisheye(orbx_matcher *m, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_valid, int n_kf,
                                     const orbx_featvec *kf_fv, const uint8_t *f_desc, const float *f_angle, int n_f, int n_f_left,
                                     const orbx_featvec *f_fv, float nnratio, int check_orientation, int32_t *f_match);

/* Device-resident, batched frame-to-frame matcher used by the throughput path: for every frame f >= 1 of the
 * extractor's last batch, the keypoints of frame f-1 (queries, at their own position shifted by (du, dv)) are
 * matched against frame f exactly as orbx_search_by_projection_frame does with level_mode 0, all features free on
 * entry and every query "has observations".  d_match: device int32 [n_frames][cap] (query index in frame f-1 or -1),
 * d_nmatches: device int32 [n_frames]; pass NULL for both to use internal buffers (fetched with
 * orbx_batch_download_async).  There is ONE set of internal buffers per extractor: of the two batched matchers
 * (this one and orbx_search_mappoints_batch_device) only the first to be called on a batch may use them, the other gets
 * ORBX_E_BAD_ARG and has to be given result buffers of its own.  Asynchronous on the extractor's stream. */
int orbx_match_consecutive_device(orbx_extractor *ex, float th, float du, float dv, int check_orientation,
                                  int32_t *d_match, int32_t *d_nmatches);

/* ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th, ...) (ORBmatcher.cc:39-141; called by
 * Tracking::SearchLocalPoints, Tracking.cc:3390-3413) for EVERY frame of the extractor's last batch, device-resident: frame f is
 * searched against n_mp map points whose per-frame projection data (what Frame::isInFrustum stores in the MapPoint: mTrackProjX/Y,
 * mnTrackScaleLevel, mTrackViewCos, mbTrackInView) lie in device arrays [n_frames][n_mp]; d_mp_desc holds the map points'
 * descriptors, frame f's at d_mp_desc + f*desc_frame_stride (0 = one shared set).  Monocular form (Nleft == -1, no mvuRight),
 * all features free on entry, every map point "has observations".  d_match: device int32 [n_frames][cap] (map-point index
 * per feature or -1), d_nmatches [n_frames]; NULL for both = internal buffers (orbx_batch_download_async).  Asynchronous. */
int orbx_search_mappoints_batch_device(orbx_extractor *ex, int n_mp, const float *d_proj_x, const float *d_proj_y,
                                       const int32_t *d_level, const float *d_view_cos, const uint8_t *d_in_view,
                                       const uint8_t *d_mp_desc, size_t desc_frame_stride, float th, float nnratio,
                                       int32_t *d_match, int32_t *d_nmatches);

/* ---- candidate generation for the projection matchers: Frame::UndistortKeyPoints, ComputeImageBounds, isInFrustum ----
 * Pinhole intrinsics (Frame::mK / fx, fy, cx, cy), radial-tangential distortion (Frame::mDistCoef: k1, k2, p1, p2[, k3]) and mbf. */
typedef struct orbx_camera {
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3;
    float bf;
} orbx_camera;
/* Frame::mRcw (row-major), mtcw, mOw */
typedef struct orbx_frame_pose {
    float Rcw[9], tcw[3], Ow[3];
} orbx_frame_pose;

/* Frame::UndistortKeyPoints (Frame.cc:747-780): kps_un[i] = kps[i] with the point run through cv::undistortPoints(K, distCoef, R = I,
 * P = K) (published algorithm: 5 fixed-point iterations of the radial-tangential model in double); a plain copy when k1 == 0. */
int orbx_undistort_keypoints(orbx_matcher *m, const orbx_camera *cam, const orbx_keypoint *kps, int n, orbx_keypoint *kps_un);
/* Frame::ComputeImageBounds (Frame.cc:782-810): bounds4 = {mnMinX, mnMaxX, mnMinY, mnMaxY} (host arithmetic, no device needed) */
int orbx_image_bounds(const orbx_camera *cam, int width, int height, float *bounds4);
/* Frame::isInFrustum(pMP, viewingCosLimit) (Frame.cc:512-575, Nleft == -1) for n_mp map points given flat: world position and normal
 * (3 floats each), mfMinDistance / mfMaxDistance.  Outputs are the MapPoint fields the function writes: in_view (mbTrackInView),
 * proj_x / proj_y (mTrackProjX/Y; -1 unless the projection lies inside the image bounds), and where in_view: proj_xr, depth
 * (mTrackDepth), level (mnTrackScaleLevel = PredictScale, MapPoint.cc:531-546), view_cos.  Every float operation rounds as the
 * reference text writes it. */
int orbx_is_in_frustum(orbx_matcher *m, const orbx_camera *cam, const orbx_frame_pose *pose, const float *bounds4, float log_scale_factor,
                       int nlevels, float viewing_cos_limit, int n_mp, const float *pos, const float *normal, const float *min_dist,
                       const float *max_dist, uint8_t *in_view, float *proj_x, float *proj_y, float *proj_xr, float *depth, int32_t *level,
                       float *view_cos);
/* Tracking::SearchLocalPoints (Tracking.cc:3339-3413) on a resident frame in one call with one synchronisation: Frame::isInFrustum (Frame.cc:512-575,
 * mono or rectified stereo, as orbx_is_in_frustum with the frame's bounds and levels) of every map point, then SearchByProjection(F, vpMapPoints, th,
 * bFarPoints, thFarPoints) (ORBmatcher.cc:43-213, Nleft == -1).  Map points flat: pos / normal (3 floats each), min_dist / max_dist, 32-byte
 * descriptors, eligible[j] = !isBad() && mnLastFrameSeen != F.mnId (NULL = all), has_obs[j] = Observations() > 0 (NULL = all).  A map point is
 * searched iff eligible, in view, its predicted level one of the frame's and not (far_points && depth > th_far_points).  Outputs: in_view[n_mp]
 * (mbTrackInView of the eligible points: the caller's IncreaseVisible), frame_match[N] as orbx_search_by_projection_mappoints.  The projection
 * records never leave the device.  Returns nmatches. */
int orbx_frame_search_local_points(orbx_matcher *m, orbx_frame *f, const uint8_t *frame_occupied, const orbx_camera *cam, const orbx_frame_pose *pose,
                                   float log_scale_factor, float viewing_cos_limit, int n_mp, const float *pos, const float *normal,
                                   const float *min_dist, const float *max_dist, const uint8_t *mp_desc, const uint8_t *eligible,
                                   const uint8_t *has_obs, float th, float nnratio, int far_points, float th_far_points, uint8_t *in_view,
                                   int32_t *frame_match);
/* One camera of a fisheye rig as Frame::isInFrustumChecks (Frame.cc:1168-1240) sees it.  The caller evaluates the reference's expressions (:1172-1186):
 * left camera R = mRcw, t = mtcw, twc = mOw; right camera (bRight) R = Rrl * mRcw, t = Rrl * mtcw + trl, twc = mRwc * mTlr.translation() + mOw.
 * params = KannalaBrandt8::mvParameters (fx, fy, cx, cy, k0 .. k3). */
typedef struct orbx_fisheye_view {
    float R[9], t[3], twc[3];
    float params[8];
} orbx_fisheye_view;
/* Frame::isInFrustumChecks(pMP, viewingCosLimit, bRight) (Frame.cc:1168-1240, called from Frame::isInFrustum :577-590 when Nleft != -1) with
 * KannalaBrandt8::project (CameraModels/KannalaBrandt8.cpp:67-85) for n_mp map points and n_views (1 or 2: left, right) cameras of the rig.
 * Outputs [n_views][n_mp]: in_view (mbTrackInView / mbTrackInViewR) and, where in_view, proj_x / proj_y (mTrackProjX/Y[R]), depth (mTrackDepth[R]),
 * level (mnTrackScaleLevel[R]), view_cos (mTrackViewCos[R]); elsewhere level = -1 (:579-580) and zeros (the reference leaves those fields untouched).
 * atan2f is glibc's, restated bit for bit; cos / sin of the azimuth are evaluated in double as the reference's translation unit does (no float overload
 * in scope): proj_x / proj_y may differ from an x86-64 glibc build in the last float ulp where the double result lies on a rounding boundary. */
int orbx_is_in_frustum_checks(orbx_matcher *m, const orbx_fisheye_view *views, int n_views, const float *bounds4, float log_scale_factor, int nlevels,
                              float viewing_cos_limit, int n_mp, const float *pos, const float *normal, const float *min_dist, const float *max_dist,
                              uint8_t *in_view, float *proj_x, float *proj_y, float *depth, int32_t *level, float *view_cos);
/* Tracking::SearchLocalPoints (Tracking.cc:3339-3413) on a resident FISHEYE-STEREO frame in one call, one synchronisation: Frame::isInFrustum of
 * every map point (isInFrustumChecks of views[0] = left and views[1] = right, with the frame's bounds and levels), the window setup and
 * SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) (ORBmatcher.cc:43-213 whole); the projection records stay on the device.
 * The contract is orbx_frame_search_local_points', per camera: a map point is searched iff eligible[j] (!isBad() && mnLastFrameSeen != F.mnId;
 * NULL = all), in view of either camera, and not (far_points && mTrackDepth > th_far_points).  The left sub-query's radius is
 * RadiusByViewingCos * th (th != 1) * scale, the right one's has no th factor; a level outside the frame's levels drops that camera's sub-query.
 * mTrackDepth: isInFrustumChecks writes it only when the LEFT camera sees the point (Frame.cc:1168-1240).  For a point only the right camera sees,
 * the reference's far-point test reads the MapPoint's PREVIOUS mTrackDepth: pass it in track_depth[n_mp] (read for those points only); NULL means
 * such a point is never far.  Outputs: in_view [2][n_mp] = mbTrackInView / mbTrackInViewR of the eligible points (the caller calls IncreaseVisible
 * when either is set), frame_match [N].  Returns nmatches. */
int orbx_frame_search_local_points_fisheye(orbx_matcher *m, orbx_frame *f, const uint8_t *frame_occupied, const orbx_fisheye_view *views,
                                           float log_scale_factor, float viewing_cos_limit, int n_mp, const float *pos, const float *normal,
                                           const float *min_dist, const float *max_dist, const uint8_t *mp_desc, const uint8_t *eligible,
                                           const uint8_t *has_obs, const float *track_depth, float th, float nnratio, int far_points,
                                           float th_far_points, uint8_t *in_view, int32_t *frame_match);
/* The same for n_frames poses at once on device-resident map-point data (shared by all frames); outputs [n_frames][n_mp] in device
 * memory -- exactly the arrays orbx_search_mappoints_batch_device consumes (Tracking::SearchLocalPoints, Tracking.cc:3339-3413: frustum
 * test, then SearchByProjection).  bounds4 = NULL uses the extractor's camera (orbx_set_camera) or the plain image rectangle.
 * Asynchronous, ordered before a following orbx_search_mappoints_batch_device on the same extractor. */
int orbx_frustum_batch_device(orbx_extractor *ex, const orbx_camera *cam, const orbx_frame_pose *poses, int n_frames, const float *bounds4,
                              float viewing_cos_limit, int n_mp, const float *d_pos, const float *d_normal, const float *d_min_dist,
                              const float *d_max_dist, uint8_t *d_in_view, float *d_proj_x, float *d_proj_y, float *d_proj_xr, float *d_depth,
                              int32_t *d_level, float *d_view_cos);
/* Gives the extractor's batch path a camera: after every batched extraction the keypoints are undistorted on the device (mvKeysUn,
 * orbx_batch_view.d_keypoints_un) and the batched matchers use them together with the undistorted image bounds.  cam = NULL removes
 * it (mvKeysUn = mvKeys, bounds = image rectangle: the distortion-free default). */
int orbx_set_camera(orbx_extractor *ex, const orbx_camera *cam);
/* mvKeysUn of one frame of the last batch (equals the keypoints when no camera is set) */
int orbx_batch_download_keypoints_un(orbx_extractor *ex, int frame, orbx_keypoint *kps_un, int cap, int *n_out);

/* The matching core of ORBmatcher::Fuse(KeyFrame*, vpMapPoints, th, bRight) (ORBmatcher.cc:1148-1337, candidate loop
 * :1246-1306) and Fuse(KeyFrame*, Sim3f&, vpPoints, th, vpReplacePoint) (:1339-1455, loop :1405-1433): for each projected
 * map point (u, v[, ur], radius = th*scale[lvl], predicted level) the best feature of the key frame among
 * KeyFrame::GetFeaturesInArea(u, v, r) with octave in [lvl-1, lvl] and -- when inv_level_sigma2 != NULL (first overload) --
 * reprojection chi2 <= 5.99 (mono) / 7.8 (kf->u_right[idx] >= 0).  Queries do not interact; best_idx = -1 / best_dist = 256
 * when nothing qualifies.  The caller accepts best_dist <= ORBX_TH_LOW and performs Replace / AddObservation / AddMapPoint.
 * strict_fp = 0: e2 summed with the fused multiply-adds GCC emits for the reference's flags; 1: separate mul/add. */
int orbx_fuse_search(orbx_matcher *m, const orbx_frame_desc *kf, const float *inv_level_sigma2, int n_q, const float *q_u,
                     const float *q_v, const float *q_ur, const float *q_r, const int32_t *q_level, const uint8_t *q_desc,
                     int strict_fp, int32_t *best_idx, int32_t *best_dist);

/* ---- device-resident key frames ----
 * KeyFrame::KeyFrame(Frame &F, Map*, KeyFrameDatabase*) (KeyFrame.cc:36-82) copies the frame's mvKeysUn, mDescriptors, mvuRight, mvScaleFactors,
 * mvInvLevelSigma2, the image bounds and mGrid; none of them changes afterwards, and LocalMapping / LoopClosing search the same 10 - 30 covisible key
 * frames again for every new key frame.  An orbx_keyframe is that copy on the device: ONE allocation sized by N (about 66 bytes per feature + 6 KB of
 * grid; sized by the frame handle's capacity only when N of a batch-loaded frame is still on the device), immutable once made.  These entry points take monocular / rectified
 * key frames (NLeft == -1, Pinhole); fisheye-stereo key frames have the `_fisheye` forms further down, and each kind's calls refuse the other kind.
 *   orbx_keyframe_from_frame: a device-to-device copy of a loaded monocular / rectified orbx_frame owned by `m` -- rows, count, scale factors and the grid
 *     AS BUILT (no rebuild) -- plus inv_level_sigma2 [the frame's nlevels] (mvInvLevelSigma2; NULL = none: only the gate-less searches accept the key
 *     frame).  Enqueued on m's stream, no host synchronisation, also while N is still on the device; the frame may be reloaded as soon as the call
 *     returns (stream order protects the copy).  A fisheye handle, a handle that was never loaded or one of another matcher: ORBX_E_BAD_ARG before anything
 *     is enqueued.
 *   orbx_keyframe_create_host: the same object from host arrays (a loaded atlas, tests): one upload, the grid built as orbx_fuse_search builds it, so the
 *     candidate order and every tie are that entry point's.  desc->n <= 65535 (ORBX_E_TOO_LARGE otherwise).  Returns without waiting for the upload.
 *   orbx_keyframe_count: N (one download behind the copy if the key frame was made while N was still on the device; cached).
 * SHARING.  A key frame belongs to no matcher: it records an event when its copy / upload is enqueued, and ANY matcher context of the same device may
 * search it -- the context's stream waits for that event until a call that did so has returned.  (A context of another device: ORBX_E_BAD_ARG.)  The
 * key frame is read-only afterwards, so contexts on different threads may search the same key frames at the same time without a lock.
 * (The one later write is attaching the BoW state, orbx_keyframe_compute_bow / orbx_keyframe_bow_from_frame below: the caller orders that call before any
 * BoW search is handed the key frame -- "SHARING, continued" there.)
 * orbx_keyframe_destroy waits for the copy / upload, then frees the allocation and the event; call it only when no call that was handed the key frame
 * is running (both searches below synchronise before they return, so "running" means: has not returned yet).  A key frame may outlive the matcher and the
 * frame handle it was made from. */
typedef struct orbx_keyframe orbx_keyframe;
int orbx_keyframe_from_frame(orbx_matcher *m, orbx_frame *frame, const float *inv_level_sigma2, orbx_keyframe **out);
int orbx_keyframe_create_host(orbx_matcher *m, const orbx_frame_desc *desc, const float *inv_level_sigma2, orbx_keyframe **out);
int orbx_keyframe_count(orbx_keyframe *kf, int *n);
void orbx_keyframe_destroy(orbx_keyframe *kf);

/* The most key frames one orbx_keyframe_fuse_search / orbx_keyframe_fuse_map_points call takes (ORBX_E_TOO_LARGE beyond). */
#define ORBX_MAX_FUSE_KEYFRAMES 256
/* One query set of orbx_keyframe_fuse_search: the q_* arguments of orbx_fuse_search (ur may be NULL; everything may be NULL when n == 0). */
typedef struct orbx_fuse_queries {
    int32_t n;
    const float *u, *v, *ur, *r;
    const int32_t *level;
    const uint8_t *desc;
} orbx_fuse_queries;
/* orbx_fuse_search (the candidate loops of ORBmatcher::Fuse, ORBmatcher.cc:1246-1306 and :1405-1433; SearchBySim3's two searches, :1457-1674) for n_kf
 * resident key frames in one call, key frame k with its own query set queries[k].  use_chi2 != 0: the reprojection gate with the key frame's
 * mvInvLevelSigma2 (first overload; ORBX_E_BAD_ARG if a key frame has none); 0: the gate-less form (Fuse(pKF, Scw, ...), SearchBySim3).  The gate-less form
 * never reads the key frame's mvuRight, as the reference's (:1405-1433) and the adapter's call of orbx_fuse_search for it (a frame description without
 * u_right) do not.
 * best_idx[k] / best_dist[k] (queries[k].n entries each; may be NULL when that is 0) equal orbx_fuse_search on key frame k's host arrays bit for bit.
 * Key frames of one call may have different image bounds.  One upload run, one launch, one download run, one synchronisation whatever n_kf is;
 * n_kf = 0 and empty query sets are fine.  Argument errors (a NULL row included) are reported before anything is enqueued. */
int orbx_keyframe_fuse_search(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fuse_queries *queries, int use_chi2, int strict_fp,
                              int32_t *const *best_idx, int32_t *const *best_dist);
/* The Fuse loop of LocalMapping::SearchInNeighbors (LocalMapping.cc: one ORBmatcher::Fuse(pKFi, vpMapPointMatches) per target key frame) in one call,
 * projection included: ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th, bRight = false) (ORBmatcher.cc:1148-1337) up to and including the
 * candidate loop, for n_kf target key frames and n_mp map points given once.  cams[k] / poses[k]: the key frame's Pinhole intrinsics and mbf,
 * GetPose() (Rcw row-major, tcw) and GetCameraCenter(); map points flat as orbx_frame_search_local_points takes them (world position and normal, 3 floats
 * each; mfMinDistance / mfMaxDistance; GetDescriptor(), 32 bytes); skip [n_kf][n_mp] (may be NULL) = !pMP || isBad() || IsInKeyFrame(pKF_k) (:1193-1201).
 * Per pair, in the reference's order and rounding (:1186-1244): p3Dc.z < 0 rejects; Pinhole::project and KeyFrame::IsInImage -- x >= mnMinX && x < mnMaxX
 * && y >= mnMinY && y < mnMaxY, strict on the max side, unlike Frame::isInFrustum; ur = u - bf / z; dist3D outside [0.8 mfMinDistance, 1.2 mfMaxDistance]
 * rejects; PO.dot(Pn) < 0.5 * dist3D rejects (compared in double, no division); PredictScale(dist3D, pKF) (MapPoint.cc:531-546) with the key frame's
 * levels and log_scale_factor; radius = th * mvScaleFactors[level]; candidates with octave in [level - 1, level] and chi2 <= 5.99 / 7.8 as
 * orbx_fuse_search (every key frame needs inv_level_sigma2: ORBX_E_BAD_ARG otherwise).
 * Outputs [n_kf][n_mp]: best_idx / best_dist (-1 / 256 when the pair was skipped, failed a gate or found no candidate), projected (may be NULL; 1 = the
 * pair passed every gate above).  The caller accepts best_dist <= ORBX_TH_LOW and runs the reference's tail (:1308-1330) per key frame, re-checking
 * isBad() / IsInKeyFrame on the live graph: the searches of the loop are independent, an earlier Fuse changes only those two for a later one.
 * The map points are uploaded once, the query records never leave the device; the transfers and the launch chain do not grow with n_kf. */
int orbx_keyframe_fuse_map_points(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams, const orbx_frame_pose *poses, float th,
                                  float log_scale_factor, int strict_fp, int n_mp, const float *pos, const float *normal, const float *min_dist,
                                  const float *max_dist, const uint8_t *mp_desc, const uint8_t *skip, int32_t *best_idx, int32_t *best_dist,
                                  uint8_t *projected);

/* ---- fisheye-stereo key frames (KeyFrame::NLeft != -1: KannalaBrandt8 rigs) ----
 * What KeyFrame::KeyFrame(Frame&) copies of a rig frame and Fuse reads: mvKeys (rows [0, N_left)), mvKeysRight (stored at a row offset the host knows
 * before the counts are, as the frame handle's), all N = N_left + N_right descriptor rows, the two counts, mvScaleFactors, mvInvLevelSigma2, the bounds,
 * mGrid and mGridRight (side-local indices).  One allocation, immutable, owned by no matcher; the `ready` event, orbx_keyframe_destroy and SHARING are
 * those of every orbx_keyframe.  NOT kept: mvLeftToRightMatch / mvRightToLeftMatch (Fuse does not read them) and mvuRight (a rig key frame has none that
 * Fuse could use: every candidate of either camera meets the monocular gate, 5.99, as through the adapter's single-target Fuse).
 * Numbering as every fisheye entry point: features [0, N_left) = left camera, [N_left, N) = right camera.
 *   orbx_keyframe_from_frame_fisheye: a device-to-device copy of a loaded fisheye-stereo orbx_frame owned by `m` (orbx_frame_load_host_fisheye or
 *     orbx_frame_load_stereo_fisheye_batch): rows, both counts, scale factors and both grids AS BUILT, plus inv_level_sigma2 (NULL = none).  On m's
 *     stream, no host synchronisation, also while the counts are still on the device (the key frame is searchable without one, too: the counts come
 *     home with the first search's results); the frame may be reloaded as soon as the call returns.  A monocular handle, a handle that was never
 *     loaded or one of another matcher: ORBX_E_BAD_ARG before anything is enqueued.
 *   orbx_keyframe_create_host_fisheye: the same object from host arrays; arguments as orbx_frame_load_host_fisheye without l2r / r2l (left->keypoints_un
 *     = mvKeys, left->n = N_left, left->descriptors = ALL N rows, kps_right = mvKeysRight [n_right]).  One upload; both grids in k_grid_build's order,
 *     so candidate order and ties are orbx_fuse_search's on that camera's arrays.  N <= 65535 (ORBX_E_TOO_LARGE).
 *   orbx_keyframe_counts: N_left and N_right (n_right = -1 for a monocular key frame, as orbx_frame_counts); at most one synchronisation, then cached.
 *     orbx_keyframe_count of a fisheye key frame returns N.
 * Every other key-frame call above and below (orbx_keyframe_fuse_search, orbx_keyframe_fuse_map_points, the BoW calls and searches) refuses a fisheye
 * key frame with ORBX_E_BAD_ARG before anything is enqueued, and the two searches here refuse a monocular one.  Not covered: BoW on fisheye key frames
 * and the KannalaBrandt8 triangulation gate on resident key frames. */
int orbx_keyframe_from_frame_fisheye(orbx_matcher *m, orbx_frame *frame, const float *inv_level_sigma2, orbx_keyframe **out);
int orbx_keyframe_create_host_fisheye(orbx_matcher *m, const orbx_frame_desc *left, const orbx_keypoint *kps_right, int n_right,
                                      const float *inv_level_sigma2, orbx_keyframe **out);
int orbx_keyframe_counts(orbx_keyframe *kf, int *n_left, int *n_right);
/* orbx_keyframe_fuse_search for rig key frames: queries / best_idx / best_dist hold [n_kf][2] entries, index 2 k = key frame k's left-camera query set,
 * 2 k + 1 its right-camera set.  A left-camera problem searches mvKeys with the left grid and descriptor rows [0, N_left), a right-camera problem
 * mvKeysRight with the right grid and rows [N_left, N); a right-camera best_idx comes back in the rig's numbering, N_left + j (ORBmatcher.cc:1296; -1
 * stays -1).  queries[.].ur is ignored and may be NULL: use_chi2 applies the monocular gate (5.99) to every candidate.  Each row equals
 * orbx_fuse_search on that camera's host arrays (right indices + N_left) bit for bit.  Cost shape, limits and errors as orbx_keyframe_fuse_search: one
 * upload run, one launch over 2 n_kf problems, one download run, one synchronisation; n_kf <= ORBX_MAX_FUSE_KEYFRAMES. */
int orbx_keyframe_fuse_search_fisheye(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fuse_queries *queries, int use_chi2, int strict_fp,
                                      int32_t *const *best_idx, int32_t *const *best_dist);
/* BOTH Fuse calls of LocalMapping::SearchInNeighbors' loop on a rig -- matcher.Fuse(pKFi, vpMapPointMatches) and matcher.Fuse(pKFi, vpMapPointMatches,
 * true) -- for n_kf target key frames in one call, projection included (ORBmatcher.cc:1148-1337 with :1150-1163 choosing the camera).
 * views [n_kf][2]: the left camera's R, t = GetPose(), twc = GetCameraCenter(), params = mpCamera's; the right camera's GetRightPose(),
 * GetRightCameraCenter(), mpCamera2's -- evaluated by the caller, as for orbx_is_in_frustum_checks.  Map points flat as orbx_keyframe_fuse_map_points
 * takes them; skip [n_kf][n_mp] (may be NULL): one row per key frame, read by both cameras (the caller's tail re-checks isBad() / IsInKeyFrame per
 * camera).  Per (key frame, camera, map point), in the reference's order (:1186-1244): p3Dc = R p + t; p3Dc.z < 0 rejects; KannalaBrandt8::project
 * (the restatement orbx_is_in_frustum_checks uses, same one-ulp caveat); KeyFrame::IsInImage, strict on the max side; dist3D outside [0.8 mfMinDistance,
 * 1.2 mfMaxDistance] rejects; PO.dot(Pn) < 0.5 * dist3D rejects (in double, no division); PredictScale; radius = th * mvScaleFactors[level]; candidates
 * with octave in [level - 1, level] and chi2 <= 5.99.  Every key frame needs inv_level_sigma2.
 * Outputs [n_kf][2][n_mp]: best_idx (rig numbering) / best_dist, projected (may be NULL).  Four launches whatever n_kf is (upload, projection, search,
 * download), one synchronisation; the map points go up once and the query records never visit the host. */
int orbx_keyframe_fuse_map_points_fisheye(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fisheye_view *views, float th,
                                          float log_scale_factor, int strict_fp, int n_mp, const float *pos, const float *normal, const float *min_dist,
                                          const float *max_dist, const uint8_t *mp_desc, const uint8_t *skip, int32_t *best_idx, int32_t *best_dist,
                                          uint8_t *projected);

/* MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:329-403), batched over map points: set s = the descriptors of the
 * observations of map point s, descriptors[set_ptr[s] .. set_ptr[s+1]) (gathered by the adapter from
 * pKF->mDescriptors.row(leftIndex/rightIndex) in std::map order).  best_idx[s] = index inside the set of the descriptor
 * with the least median Hamming distance to the others (first minimum wins), -1 for an empty set. */
int orbx_distinctive_descriptors(orbx_matcher *m, const uint8_t *descriptors, const int32_t *set_ptr, int n_sets,
                                 int32_t *best_idx);

/* ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> on the device (include/ORBVocabulary.h;
 * Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h).  The tree crosses the ABI flattened: node 0 is the root, the children
 * of node i are child_idx[child_ptr[i] .. child_ptr[i+1]) in m_nodes[i].children order, node_desc = n_nodes x 32 bytes,
 * word_id[i] >= 0 iff node i is a leaf (its WordId).  L = depth (m_L). */
typedef struct orbx_vocabulary orbx_vocabulary;
int orbx_vocabulary_create(int device, int L, int n_nodes, const int32_t *child_ptr, const int32_t *child_idx,
                           const uint8_t *node_desc, const int32_t *word_id, orbx_vocabulary **out);
void orbx_vocabulary_destroy(orbx_vocabulary *voc);
/* TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup) (TemplatedVocabulary.h:1206-1250) for the n
 * descriptors of a frame, as Frame::ComputeBoW needs (Frame.cc:738-745, levelsup = 4): word_id[i] = WordId of the leaf
 * reached, node_id[i] = NodeId at level L - levelsup (the FeatureVector key).  The adapter builds BowVector (weights from
 * its own vocabulary copy, tf-idf + L1 in double) and FeatureVector from these ids. */
int orbx_bow_transform(orbx_matcher *m, const orbx_vocabulary *voc, const uint8_t *descriptors, int n, int levelsup,
                       int32_t *word_id, int32_t *node_id);
/* The stop words of TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) (TemplatedVocabulary.h:1151-1193): a
 * feature enters the FeatureVector only `if (w > 0)`.  weight[id] = m_words[id]->weight for every word id 0 .. n_words - 1 (n_words above the
 * largest word id of the tree, ORBX_E_BAD_ARG otherwise).  The device keeps the sign of every weight for the stop-word test and, beside it, the
 * weights themselves as doubles: the tf-idf values of orbx_frame_bow_vector / orbx_keyframe_bow_vector and the key-frame database (below).  A
 * vocabulary without weights stops no word and has no BowVector.  Takes effect at the next orbx_frame_compute_bow. */
int orbx_vocabulary_set_word_weights(orbx_vocabulary *voc, const double *weight, int n_words);

/* ---- BoW on the device-resident frame: Tracking::TrackReferenceKeyFrame and Tracking::Relocalization ----
 * orbx_frame_compute_bow replaces Frame::ComputeBoW's transform (Frame.cc:738-745: mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4))
 * on the handle's descriptors: nothing of the frame is uploaded.  The frame's FeatureVector (ascending node ids, each with its feature indices in
 * ascending order, stopped features left out: the std::map order of FeatureVector::addFeature) stays in the handle.  Node ids are
 * orbx_bow_transform's (node 0 for a leaf above level L - levelsup).  word_id / node_id (optional, N entries each; N may be unknown to the caller
 * after orbx_frame_load_batch: buffers of the handle's capacity always suffice) return the per-feature ids; mBowVec itself (tf-idf, L1) is built
 * on the device from the kept ids: orbx_frame_bow_vector and the orbx_keyframe_database, below.  Both NULL: asynchronous, nothing waits.  The handle keeps the result, the vocabulary and
 * levelsup until its next load.  ORBX_E_BAD_ARG for a handle of another matcher or a vocabulary on another device, before anything is enqueued. */
int orbx_frame_compute_bow(orbx_matcher *m, orbx_frame *f, const orbx_vocabulary *voc, int levelsup, int32_t *word_id, int32_t *node_id);
/* One key frame of a SearchByBoW batch: mDescriptors (n x 32), mvKeysUn[i].angle, valid[i] = GetMapPointMatches()[i] present and !isBad()
 * (NULL: all), its mFeatVec flattened (node ids strictly ascending, indices < n).  n <= 65535. */
typedef struct orbx_bow_keyframe {
    const uint8_t *descriptors;
    const float *angle;
    const uint8_t *valid;
    int32_t n;
    orbx_featvec fv;
} orbx_bow_keyframe;
#define ORBX_MAX_BOW_KEYFRAMES 1024
/* ORBmatcher(nnratio, check_orientation).SearchByBoW(kfs[k], F, vvpMapPointMatches[k]) (ORBmatcher.cc:223-425) for k = 0 .. n_kf - 1 against the
 * handle's frame (its descriptors, mvKeysUn angles and orbx_frame_compute_bow's FeatureVector): match[k * match_stride + iF] = KF feature index or
 * -1 for iF < N, nmatches[k] = the member's return value.  Row k equals orbx_search_by_bow_frame for key frame k bit for bit.  Relocalization's
 * candidates in one call: one upload run, one launch chain whose length does not depend on n_kf, one download run, one synchronisation.
 * match_stride >= N; while N is still on the device (orbx_frame_load_batch) a stride below the handle's capacity costs one orbx_frame_count first.
 * Monocular / rectified frames only: a fisheye-stereo handle is refused (ORBX_E_BAD_ARG) by this call and orbx_frame_compute_bow (fisheye-stereo
 * handles: orbx_frame_compute_bow_fisheye / orbx_frame_search_by_bow_fisheye, below).  n_kf <= ORBX_MAX_BOW_KEYFRAMES (ORBX_E_TOO_LARGE).
 * Returns ORBX_OK; ORBX_E_BAD_ARG, before anything is enqueued, for a handle of another matcher, a frame without orbx_frame_compute_bow since its
 * last load, or a malformed key frame. */
int orbx_frame_search_by_bow(orbx_matcher *m, orbx_frame *f, int n_kf, const orbx_bow_keyframe *kfs, float nnratio, int check_orientation,
                             int32_t *match, int match_stride, int32_t *nmatches);
/* orbx_search_by_projection_window on the resident frame (ORBmatcher.cc:1889-2010: Relocalization's SearchByProjection(F, pKF, sFound, 10, 100)
 * and (.., 3, 64)); match holds N entries.  Results equal the host-pointer form's bit for bit.  Monocular / rectified frames only (fisheye-stereo
 * handles: orbx_frame_search_by_projection_window_fisheye). */
int orbx_frame_search_by_projection_window(orbx_matcher *m, orbx_frame *f, const uint8_t *occupied, int n_q, const float *q_x, const float *q_y,
                                           const float *q_r, const int32_t *q_min_level, const int32_t *q_max_level, const float *q_angle,
                                           const uint8_t *q_desc, const uint8_t *q_has_obs, float max_dist, int check_orientation, int32_t *match);

/* ---- BoW and the relocalization window search on a fisheye-stereo handle (Frame::Nleft != -1): TrackReferenceKeyFrame and Relocalization of a rig.
 * These refuse a monocular / rectified handle with ORBX_E_BAD_ARG, as the forms above refuse a fisheye-stereo one.  Numbering as everywhere for a
 * rig: features [0, N_left) = left camera, [N_left, N) = right camera.
 * orbx_frame_compute_bow_fisheye: Frame::ComputeBoW of a rig frame (Frame.cc:738-745; mDescriptors holds all N = N_left + N_right rows) on the
 *   handle's rows, after orbx_frame_load_host_fisheye or orbx_frame_load_stereo_fisheye_batch.  The FeatureVector stays in the handle (equal to
 *   TemplatedVocabulary::transform's over the N rows: ascending node ids, ascending feature indices within a node, stopped words dropped).
 *   word_id / node_id: as orbx_frame_compute_bow (optional, N entries each; buffers of the handle's capacity always suffice).  Both NULL:
 *   asynchronous, nothing waits and the counts are not read on the host. */
int orbx_frame_compute_bow_fisheye(orbx_matcher *m, orbx_frame *f, const orbx_vocabulary *voc, int levelsup, int32_t *word_id, int32_t *node_id);
/* orbx_frame_search_by_bow_fisheye: SearchByBoW(kfs[k], F, vvpMapPointMatches[k]) for a rig frame (ORBmatcher.cc:283-392) for k < n_kf; row k
 *   equals orbx_search_by_bow_frame_fisheye for key frame k bit for bit (N entries; a right-camera match sits at N_left + j).  kfs[k].angle: the
 *   key frame's keypoint angles (mvKeysUn, or mvKeys / mvKeysRight of a fisheye key frame).  Arguments, limits, cost shape and errors as
 *   orbx_frame_search_by_bow; the frame needs orbx_frame_compute_bow_fisheye since its last load. */
int orbx_frame_search_by_bow_fisheye(orbx_matcher *m, orbx_frame *f, int n_kf, const orbx_bow_keyframe *kfs, float nnratio, int check_orientation,
                                     int32_t *match, int match_stride, int32_t *nmatches);
/* orbx_frame_search_by_projection_window_fisheye: Relocalization's SearchByProjection(F, pKF, sFound, th, ORBdist) (ORBmatcher.cc:1889-2010) on a
 *   rig frame.  GetFeaturesInArea runs with its default bRight = false, so only the LEFT camera is searched (raw mvKeys, the left grid; N_left is
 *   read on the device).  occupied and match hold all N entries: occupancy is read for [0, N_left) only, the right camera's entries of match
 *   stay -1.  Otherwise as orbx_frame_search_by_projection_window. */
int orbx_frame_search_by_projection_window_fisheye(orbx_matcher *m, orbx_frame *f, const uint8_t *occupied, int n_q, const float *q_x,
                                                   const float *q_y, const float *q_r, const int32_t *q_min_level, const int32_t *q_max_level,
                                                   const float *q_angle, const uint8_t *q_desc, const uint8_t *q_has_obs, float max_dist,
                                                   int check_orientation, int32_t *match);

/* ---- BoW on device-resident key frames: KeyFrame::ComputeBoW and the BoW-guided matchers with BOTH sides resident ----
 * A key frame's BoW state is a second allocation, made when BoW is first attached (key frames without it keep their ~66 bytes per feature): per-feature
 * word and node ids, mvKeysUn[i].angle, and mFeatVec as orbx_frame_compute_bow keeps it (ascending node ids, each with its feature indices in
 * ascending order, stopped words left out: the std::map order of FeatureVector::addFeature), with the vocabulary and levelsup it was made with.
 * It is set ONCE and immutable afterwards.  Key frames of at most 16384 features (ORBX_E_TOO_LARGE beyond: the FeatureVector is sorted in LDS).
 *   orbx_keyframe_compute_bow: KeyFrame::ComputeBoW (KeyFrame.cc: `if (mBowVec.empty() || mFeatVec.empty())` ... transform(vCurrentDesc, mBowVec,
 *     mFeatVec, 4), the transform of Frame.cc:738-745) on the key frame's own descriptors: nothing is uploaded, N is read on the device when the key
 *     frame came from a batch-loaded frame.  word_id / node_id: optional, N entries each (a buffer of the key frame's capacity -- the frame handle's,
 *     if N was unknown when it was made -- always suffices); both NULL: nothing waits.  A second call with the same vocabulary and levelsup does not
 *     compute again, as the reference's guard: it only returns the ids that were kept.  With another vocabulary or levelsup: ORBX_E_BAD_ARG.
 *   orbx_keyframe_bow_from_frame: the mBowVec(F.mBowVec), mFeatVec(F.mFeatVec) part of KeyFrame::KeyFrame(Frame&) (KeyFrame.cc:36-82): a
 *     device-to-device copy of the frame handle's BoW state on the owner's stream, no host synchronisation.  `frame` must be the handle `kf` was
 *     made from by orbx_keyframe_from_frame (ORBX_E_BAD_ARG otherwise), still holding that load (ORBX_E_STALE if it has been loaded since), with an
 *     orbx_frame_compute_bow since that load (ORBX_E_BAD_ARG otherwise).  A key frame that already has BoW: ORBX_E_BAD_ARG.
 * SHARING, continued.  The BoW state is guarded as the rows are: an event behind its creation, every context's stream waits for it until a call that
 * did so has returned.  ORDER: attaching BoW is the one write a key frame sees after its creation, and it takes no lock.  The caller orders the
 * attaching call before any BoW search is handed the key frame (and before a second attaching call), as LocalMapping::ProcessNewKeyFrame computes
 * the BoW before the key frame enters the map; searches that do not read the BoW state (the Fuse forms) may run meanwhile. */
int orbx_keyframe_compute_bow(orbx_matcher *m, orbx_keyframe *kf, const orbx_vocabulary *voc, int levelsup, int32_t *word_id, int32_t *node_id);
int orbx_keyframe_bow_from_frame(orbx_matcher *m, orbx_keyframe *kf, orbx_frame *frame);
/* The three searches below share one driver: flags and one problem record per problem go up in one run, a pairing kernel reads both sides' node counts
 * on the device, then the batched replay and its finish pass, one download run, one synchronisation; the launch chain does not grow with n_kf and
 * nothing waits before the launches.  Refused with ORBX_E_BAD_ARG before anything is enqueued: a key frame without BoW, key frames / a frame whose
 * vocabulary or levelsup differ, a key frame of another device, a NULL key frame or row, a fisheye-stereo handle.  n_kf > ORBX_MAX_BOW_KEYFRAMES:
 * ORBX_E_TOO_LARGE.  Flags are given for all N features of their key frame; if N of that key frame is still on the device only, flags other than
 * NULL cost one orbx_keyframe_count first.
 *
 * orbx_frame_search_by_bow_resident: ORBmatcher(nnratio, check_orientation).SearchByBoW(kfs[k], F, vvpMapPointMatches[k]) (ORBmatcher.cc:223-425)
 *   for k < n_kf -- Tracking::Relocalization's candidates, TrackReferenceKeyFrame with n_kf = 1 -- against the handle's frame (after
 *   orbx_frame_compute_bow).  valid[k][i] != 0 <=> feature i of key frame k has a good map point (valid or valid[k] NULL: all).  match / match_stride
 *   / nmatches as orbx_frame_search_by_bow; row k equals that call's, and orbx_search_by_bow_frame's, for the same key frame given as host arrays,
 *   bit for bit.  Uploaded per key frame: its flags and its record. */
int orbx_frame_search_by_bow_resident(orbx_matcher *m, orbx_frame *f, int n_kf, orbx_keyframe *const *kfs, const uint8_t *const *valid, float nnratio,
                                      int check_orientation, int32_t *match, int match_stride, int32_t *nmatches);
/* orbx_keyframe_search_by_bow: SearchByBoW(pKF1, kfs2[k], vpMatches12) (ORBmatcher.cc:765-905; LoopClosing::DetectCommonRegionsFromBoW runs it for
 *   the current key frame against every candidate's covisible key frames) for k < n_kf.  match12[k * match_stride + i1] = feature of kfs2[k] or -1 for
 *   i1 < N1, nmatches[k] = the member's return value; row k equals orbx_search_by_bow_keyframes(kf1, kfs2[k]) bit for bit.  vbMatched2, the row, the
 *   rotation histogram and the counters are per problem: the same key frame may appear several times in kfs2, and kf1 among them.
 *   match_stride >= N1 (below kf1's capacity while N1 is on the device only: one orbx_keyframe_count first). */
int orbx_keyframe_search_by_bow(orbx_matcher *m, orbx_keyframe *kf1, const uint8_t *valid1, int n_kf, orbx_keyframe *const *kfs2,
                                const uint8_t *const *valid2, float nnratio, int check_orientation, int32_t *match12, int match_stride, int32_t *nmatches);
/* orbx_keyframe_search_for_triangulation: SearchForTriangulation (ORBmatcher.cc:907-1146) between two resident PINHOLE key frames with both gates on
 *   the device: orbx_search_for_triangulation_pinhole with everything the key frames already hold taken from them (mvKeysUn, mvuRight, descriptors,
 *   mFeatVec, pKF2->mvScaleFactors).  The gate carries what is left: F12, the epipole, coarse, strict_fp and pKF2->mvLevelSigma2 [nlevels = the key
 *   frame's] -- the key frame keeps mvInvLevelSigma2 and the reference reads mvLevelSigma2 (Pinhole.cpp:107-129), so the table is sent, not derived by
 *   a division.  skip1 / skip2 (N1 / N2 entries, NULL: none) and matches12 (N1 entries) as orbx_search_for_triangulation_pinhole; returns the number
 *   of matches (>= 0) or an error.  LocalMapping::CreateNewMapPoints calls it once per neighbour: its calls depend on each other through skip1, so
 *   there is no batched form.  Uploads: the two flag rows, the level table and the record. */
typedef struct orbx_keyframe_gate {
    float F12[9];
    float ep_x, ep_y;
    int coarse;
    int strict_fp;
    int nlevels;
    const float *level_sigma2_2;   /* pKF2->mvLevelSigma2 [nlevels] */
} orbx_keyframe_gate;
int orbx_keyframe_search_for_triangulation(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                           int check_orientation, const orbx_keyframe_gate *gate, int32_t *matches12);

/* ---- The same five calls for FISHEYE-STEREO key frames (orbx_keyframe_create_host_fisheye / orbx_keyframe_from_frame_fisheye; KeyFrame::NLeft != -1) ----
 * The calls above refuse such a key frame and these refuse a monocular one (ORBX_E_BAD_ARG before anything is enqueued); a rig frame handle goes with
 * rig key frames.  Everything said above holds -- set once, the event and done-flag rule, one upload run, one download run and one synchronisation
 * whatever n_kf is, nothing waiting before the launches unless flags are given for a side whose N is pending.  All indices the caller sees are in the
 * reference's feature numbering, [0, N_left) the left camera's and [N_left, N) the right camera's; on the device a rig key frame works in ROW space
 * (the right camera's rows from a fixed offset on) and both renumberings run there, with counts that may still be on the device.  The limit of 16384
 * is on the key frame's row extent (a key frame made from a batch-loaded handle keeps the handle's left capacity as that offset).
 *   orbx_keyframe_compute_bow_fisheye: KeyFrame::ComputeBoW over all N = N_left + N_right descriptor rows; word_id / node_id [N], left then right.
 *   orbx_keyframe_bow_from_frame_fisheye: the mBowVec / mFeatVec copy from the fisheye handle the key frame was made from (after its
 *     orbx_frame_compute_bow_fisheye); preconditions and ORBX_E_STALE as orbx_keyframe_bow_from_frame; no host synchronisation.
 *   orbx_frame_search_by_bow_resident_fisheye: SearchByBoW(kfs[k], F, ...) with F.Nleft != -1 (ORBmatcher.cc:283-392) for k < n_kf.  valid[k]: N_k
 *     entries.  match[k * match_stride + iF] = a feature of key frame k in [0, N_k) or -1 for iF in [0, N): row k equals
 *     orbx_frame_search_by_bow_fisheye's for the same key frame given as host arrays.
 *   orbx_keyframe_search_by_bow_fisheye: SearchByBoW(pKF1, kfs2[k], ...) between rig key frames.  The reference skips the right camera's features as
 *     queries and as candidates (:800-802, :820-822): match12 spans kf1's N features, the right camera's entries are always -1, values are below
 *     N_left of kfs2[k]; equal to orbx_search_by_bow_keyframes with every right-camera feature marked as having no map point.
 *   orbx_keyframe_search_for_triangulation_fisheye: SearchForTriangulation between two rig key frames with KannalaBrandt8::epipolarConstrain on the
 *     device (:1036-1072), as orbx_search_for_triangulation_kb8.  The gate carries what the key frames do not hold (see orbx_kb8_gate for the
 *     fields); coarse: no gate at all.  matches12[i1] = a feature of kf2 in [0, N2) or -1, i1 < N1; returns the number of matches.  N1 must be
 *     known (one orbx_keyframe_count otherwise), as in the pinhole form. */
typedef struct orbx_keyframe_kb8_gate {
    const float *level_sigma2_1, *level_sigma2_2; /* mvLevelSigma2 of pKF1 / pKF2 [nlevels = the key frames'] */
    int nlevels;
    float cam1[2][8], cam2[2][8];
    float R12[4][9], t12[4][3];
    int coarse;
} orbx_keyframe_kb8_gate;
int orbx_keyframe_compute_bow_fisheye(orbx_matcher *m, orbx_keyframe *kf, const orbx_vocabulary *voc, int levelsup, int32_t *word_id, int32_t *node_id);
int orbx_keyframe_bow_from_frame_fisheye(orbx_matcher *m, orbx_keyframe *kf, orbx_frame *frame);
int orbx_frame_search_by_bow_resident_fisheye(orbx_matcher *m, orbx_frame *f, int n_kf, orbx_keyframe *const *kfs, const uint8_t *const *valid,
                                              float nnratio, int check_orientation, int32_t *match, int match_stride, int32_t *nmatches);
int orbx_keyframe_search_by_bow_fisheye(orbx_matcher *m, orbx_keyframe *kf1, const uint8_t *valid1, int n_kf, orbx_keyframe *const *kfs2,
                                        const uint8_t *const *valid2, float nnratio, int check_orientation, int32_t *match12, int match_stride,
                                        int32_t *nmatches);
int orbx_keyframe_search_for_triangulation_fisheye(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                                   int check_orientation, const orbx_keyframe_kb8_gate *gate, int32_t *matches12);

/* ---- LocalMapping::CreateNewMapPoints: triangulating a neighbour's matches on the two resident key frames (PARITY UNPINNED) ----
 * What the member does with one matched pair (idx1, idx2) of the current key frame KF1 and a neighbour KF2 -- unproject, parallax test,
 * GeometricTools::Triangulate, depth, reprojection, distance and scale-ratio tests -- runs on the device over the key frames' own rows: key points,
 * octaves, mvuRight and mvScaleFactors never leave it.  PARITY UNPINNED: neither LocalMapping.cc nor GeometricTools.cc is among the units the oracle
 * compiles and the SVD is Eigen-internal; the text below is ORB-SLAM3 v1.0's as restated for this project, and where a reference tree is at hand its
 * text wins (DESIGN section 7p records the differences).  The member, per pair, as the device evaluates it:
 *   kp1 = NLeft == -1 ? mvKeysUn[idx1] : idx1 < NLeft ? mvKeys[idx1] : mvKeysRight[idx1 - NLeft];  bRight1 = NLeft != -1 && idx1 >= NLeft   (kp2, bRight2 alike)
 *   bStereo1 = !KF1.mpCamera2 && mvuRight[idx1] >= 0                                                                           (bStereo2 alike)
 *   rig: (Tcw1, Ow1, camera1) = bRight1 ? (GetRightPose(), GetRightCameraCenter(), mpCamera2) : (GetPose(), GetCameraCenter(), mpCamera); same for 2
 *   Rcw = Tcw.block<3,3>; Rwc = Rcw.transpose(); tcw = translation
 *   xn1 = camera1->unprojectEig(kp1.pt); xn2 alike        Pinhole: ((x - cx) / fx, (y - cy) / fy, 1.f), true divisions; KannalaBrandt8: unproject, 1e-6
 *   ray1 = Rwc1 * xn1; ray2 = Rwc2 * xn2
 *   cosParallaxRays = ray1.dot(ray2) / (ray1.norm() * ray2.norm());  cosParallaxStereo = cosParallaxRays + 1       (no stereo observation)
 *   if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && cosParallaxRays < (mbInertial ? 0.9996 : 0.9998))        compared in double
 *        A.row(0) = xn1(0) * Tcw1.row(2) - Tcw1.row(0);  A.row(1) = xn1(1) * Tcw1.row(2) - Tcw1.row(1);  rows 2, 3 with xn2, Tcw2   (Tcw: 3 x 4)
 *        x3Dh = JacobiSVD<Matrix4f>(A, ComputeFullV).matrixV().col(3);  if (x3Dh(3) == 0) continue;  x3D = x3Dh.head(3) / x3Dh(3)
 *   else continue                                                                                          "no stereo and very low parallax"
 *   z1 = Rcw1.row(2).dot(x3D) + tcw1(2);  if (z1 <= 0) continue;   z2 alike;  if (z2 <= 0) continue
 *   x1 = Rcw1.row(0).dot(x3D) + tcw1(0);  y1 alike;  uv1 = camera1->project((x1, y1, z1));  errX1 = uv1.x - kp1.pt.x;  errY1 alike
 *   if ((errX1 * errX1 + errY1 * errY1) > 5.991 * mvLevelSigma2_1[kp1.octave]) continue           float sum, compared in double; then camera 2
 *   dist1 = (x3D - Ow1).norm();  dist2 = (x3D - Ow2).norm();  if (dist1 == 0 || dist2 == 0) continue
 *   if (mbFarPoints && (dist1 >= mThFarPoints || dist2 >= mThFarPoints)) continue
 *   ratioDist = dist2 / dist1;  ratioOctave = KF1.mvScaleFactors[kp1.octave] / KF2.mvScaleFactors[kp2.octave];  ratioFactor = 1.5f * KF1.mfScaleFactor
 *   if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) continue
 *   new MapPoint(x3D, ...)
 * Every float operation is rounded on its own; matrix-vector products and dot() sum as ((0.f + a0 b0) + a1 b1) + a2 b2, norm() is the correctly
 * rounded square root of that sum; a NaN takes whatever branch the comparisons, as written, give it.
 * status: the first `continue` the member takes, numbered in the member's order.  A pair with bStereo1 || bStereo2 (rectified stereo / RGB-D: the
 * member reads mvDepth, which a resident key frame does not hold) is reported as ORBX_NEWPT_STEREO_LEFT_TO_HOST and nothing is decided for it: the
 * caller runs the member's text for that pair. */
enum {
    ORBX_NEWPT_OK = 0,
    ORBX_NEWPT_NO_MATCH = 1,              /* the match entry is -1 */
    ORBX_NEWPT_LOW_PARALLAX = 2,
    ORBX_NEWPT_TRIANGULATE_FAILED = 3,    /* x3Dh(3) == 0 */
    ORBX_NEWPT_BEHIND_1 = 4,
    ORBX_NEWPT_BEHIND_2 = 5,
    ORBX_NEWPT_REPROJ_1 = 6,
    ORBX_NEWPT_REPROJ_2 = 7,
    ORBX_NEWPT_ZERO_DIST = 8,
    ORBX_NEWPT_FAR = 9,
    ORBX_NEWPT_SCALE_RATIO = 10,
    ORBX_NEWPT_STEREO_LEFT_TO_HOST = 11
};
/* One Pinhole camera of the pair: Rcw / tcw of GetPose(), Ow = GetCameraCenter(), fx, fy, cx, cy.  A rig gives two orbx_fisheye_view per key frame
 * instead, left then right: R / t of GetPose() / GetRightPose(), twc = GetCameraCenter() / GetRightCameraCenter(), params of mpCamera / mpCamera2. */
typedef struct orbx_new_points_view {
    float Rcw[9], tcw[3], Ow[3];
    float fx, fy, cx, cy;
} orbx_new_points_view;
/* What is left of the member's state: ratio_factor = 1.5f * mpCurrentKeyFrame->mfScaleFactor (the caller's product), mbInertial, mbFarPoints,
 * mThFarPoints and the two key frames' mvLevelSigma2 [nlevels_k = key frame k's] -- sent, not derived from the mvInvLevelSigma2 the key frames keep,
 * for the reason given at orbx_keyframe_gate. */
typedef struct orbx_new_points_params {
    float ratio_factor;
    int inertial;
    int far_points;
    float th_far_points;
    int nlevels_1, nlevels_2;
    const float *level_sigma2_1, *level_sigma2_2;
} orbx_new_points_params;
/* orbx_keyframe_triangulate_pairs[_fisheye]: the member's loop body for n_pairs pairs the host knows, idx1[p] in [0, N1) and idx2[p] in [-1, N2) in
 *   the reference's feature numbering (-1: ORBX_NEWPT_NO_MATCH).  status [n_pairs] (uint8, ORBX_NEWPT_*) and pos [n_pairs][3]: row p of pos is written
 *   where status[p] == ORBX_NEWPT_OK and keeps the caller's values otherwise; *n_accepted (may be NULL) = the number of such rows.  One upload run (the
 *   two index arrays, the two level tables, one record), one k_new_points launch, one download run, one synchronisation.  Counts that are still on the
 *   device stay there: an index is checked against the capacity meanwhile and against N by the kernel, and the counts come home with the results.
 * orbx_keyframe_search_and_triangulate[_fisheye]: orbx_keyframe_search_for_triangulation[_fisheye] with the same arguments, and k_new_points launched
 *   behind it on the match row where it lies on the device: matches12 [N1] and the return value are that call's, pos [N1][3] / status [N1] /
 *   *n_accepted as above with pair p = (p, matches12[p]).  One launch more than the search, no synchronisation more; the three results lie side by
 *   side in the arena and come home in the search's download run; the upload run grows by the record and by each level table the search does not
 *   send itself (Pinhole: level_sigma2_1; a rig with coarse: both).
 * Left to the caller per neighbour, as scalar work: the baseline / median-depth test, bCoarse, the skip flags, building MapPoints from the accepted
 * rows -- whose positions then go into the table through orbx_map_update, 12 bytes per new point.
 * Refusals, ORBX_E_BAD_ARG before anything is enqueued or a transfer counter moves: a NULL argument (n_accepted and, with n_pairs = 0, the arrays
 * excepted), the other kind of key frame, a key frame of another device, nlevels_k other than key frame k's, a NULL level table, n_pairs < 0, an
 * index outside its range, and whatever the search refuses.  Found by the kernel -- an index outside [0, N) behind pending counts, a key point whose
 * octave is outside its pyramid: no address is formed from it, a flag comes home, the call returns ORBX_E_BAD_ARG and NONE of the caller's arrays
 * is written.  n_pairs = 0: ORBX_OK, nothing enqueued.  Not covered: stereo pairs (above), a `_to_map` form (it would reserve slots before the
 * outcome is known). */
int orbx_keyframe_triangulate_pairs(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const orbx_new_points_view *view1,
                                    const orbx_new_points_view *view2, const orbx_new_points_params *par, int n_pairs, const int32_t *idx1,
                                    const int32_t *idx2, float *pos, uint8_t *status, int *n_accepted);
int orbx_keyframe_triangulate_pairs_fisheye(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const orbx_fisheye_view *views1,
                                            const orbx_fisheye_view *views2, const orbx_new_points_params *par, int n_pairs, const int32_t *idx1,
                                            const int32_t *idx2, float *pos, uint8_t *status, int *n_accepted);
int orbx_keyframe_search_and_triangulate(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                         int check_orientation, const orbx_keyframe_gate *gate, const orbx_new_points_view *view1,
                                         const orbx_new_points_view *view2, const orbx_new_points_params *par, int32_t *matches12, float *pos,
                                         uint8_t *status, int *n_accepted);
int orbx_keyframe_search_and_triangulate_fisheye(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                                 int check_orientation, const orbx_keyframe_kb8_gate *gate, const orbx_fisheye_view *views1,
                                                 const orbx_fisheye_view *views2, const orbx_new_points_params *par, int32_t *matches12, float *pos,
                                                 uint8_t *status, int *n_accepted);

/* ---- LoopClosing's Sim3 projection searches on resident key frames (monocular / rectified key frames, Pinhole; a fisheye key frame is refused by
 * this pair and served by the _fisheye pair below it) ----
 * The three matcher calls LoopClosing makes with a Sim3 share their projection gates (ORBmatcher.cc:452-487, :569-604, :1369-1399); the two calls below
 * evaluate them on the device for n_kf key frames and ONE shared set of n_mp map points, and feed the search kernels from them: no key frame is uploaded,
 * the map points go up once, the query records never visit the host.  poses[k] = Tcw = SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale())
 * (Rcw row-major, tcw) with Ow = Tcw.inverse().translation(), evaluated by the caller exactly as the reference does (:436-437, :543-544, :1349-1350);
 * cams[k]: the key frame's Pinhole intrinsics (bf is not read).  Map points flat as orbx_keyframe_fuse_map_points takes them (mfMinDistance /
 * mfMaxDistance UNSCALED).  Per pair, in the reference's order, every float operation rounded on its own:
 *   skip; p3Dc = Rcw p + tcw, p3Dc.z < 0 rejects; the projection (below); KeyFrame::IsInImage, strict on the max side; dist = |p - Ow| outside
 *   [0.8f mfMinDistance, 1.2f mfMaxDistance] rejects; PO.dot(Pn) < 0.5 * dist rejects (compared in double, no division); PredictScale(dist, pKF)
 *   (MapPoint.cc:531-546) with the key frame's levels and log_scale_factor; radius = th * mvScaleFactors[level]; candidate octaves [level - 1, level].
 * No mvuRight is read and no ur is produced. */
#define ORBX_SIM3_PROJECT_CAMERA 0   /* pKF->mpCamera->project(p3Dc), Pinhole: u = fx * X / Z + cx  (ORBmatcher.cc:463, :1378) */
#define ORBX_SIM3_PROJECT_INVZ 1     /* invz = 1 / Z; x = X * invz; y = Y * invz; u = fx * x + cx, as written at ORBmatcher.cc:573-578 */
/* orbx_keyframe_search_by_projection_sim3: SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (ORBmatcher.cc:427-532;
 * projection_form = ORBX_SIM3_PROJECT_CAMERA) and its vpPointsKFs / vpMatchedKF overload (:534-646; ORBX_SIM3_PROJECT_INVZ) for n_kf key frames in one
 * call -- the targets of LoopClosing::FindMatchesByProjection / DetectCommonRegionsFromLastKF (LoopClosing.cc:755,777,964), or n_kf = 1 per candidate
 * of DetectCommonRegionsFromBoW.  The search is the window form of orbx_search_by_projection_window: accept iff (float)bestDist <= ORBX_TH_LOW *
 * ratio_hamming, no rotation check, a matched feature becomes occupied -- so the queries of one key frame interact in map-point order as the
 * reference's loop does (:489-528), and the key frames are independent problems.  Query index = map-point index (rejected pairs are switched off, not
 * compacted): match[k][i] names vpPoints directly.
 *   skip [n_kf][n_mp] or NULL: isBad() || spAlreadyFound.count(pMP) for key frame k (:445-449);
 *   occupied: NULL, or n_kf rows, each NULL or N_k entries: vpMatched[i] != NULL on entry (:499);
 *   match: n_kf rows of N_k entries: the map point assigned to feature i, or -1; nmatches [n_kf]: the member's return value per key frame;
 *   projected [n_kf][n_mp] or NULL: 1 = the pair passed every gate; proj_u / proj_v [n_kf][n_mp], both or neither: the projection, meaningful where
 *   projected == 1.
 * N_k is orbx_keyframe_count (the caller sizes the rows by it; a count still pending costs that one download here).
 * LIMITS.  The search kernels take ONE set of grid parameters per launch: the key frames of one call must have bit-equal image bounds (mnMinX, mnMaxX,
 * mnMinY, mnMaxY) -- ORBX_E_BAD_ARG otherwise, callers split the list (key frames of one camera always qualify).  N_k > ORBX_MAX_FRAME_FEATURES or
 * n_kf > ORBX_MAX_FUSE_KEYFRAMES: ORBX_E_TOO_LARGE.  A fisheye key frame, a key frame of another device, a NULL key frame or match row, projection_form
 * not 0 / 1, proj_u without proj_v: ORBX_E_BAD_ARG.  Every check runs before anything is enqueued.  n_kf = 0 or n_mp = 0: ORBX_OK, match rows -1,
 * nmatches 0.  One upload run, one download run, one synchronisation and a launch chain that do not grow with n_kf. */
int orbx_keyframe_search_by_projection_sim3(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams,
                                            const orbx_frame_pose *poses, float th, float ratio_hamming, float log_scale_factor, int projection_form,
                                            int n_mp, const float *pos, const float *normal, const float *min_dist, const float *max_dist,
                                            const uint8_t *mp_desc, const uint8_t *skip, const uint8_t *const *occupied, int32_t *const *match,
                                            int32_t *nmatches, uint8_t *projected, float *proj_u, float *proj_v);
/* orbx_keyframe_fuse_map_points_sim3: the loop of LoopClosing::SearchAndFuse -- Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:1339-1455)
 * per key frame of CorrectedPosesMap -- up to and including the candidate loop, in one call: the gates above with ORBX_SIM3_PROJECT_CAMERA, then the
 * gate-less candidate search of orbx_keyframe_fuse_search(use_chi2 = 0) (:1405-1433: no chi2 test, no mvuRight).  skip [n_kf][n_mp] or NULL = isBad() ||
 * spAlreadyFound.count(pMP) with spAlreadyFound = pKF_k->GetMapPoints() (:1352, :1363).  Outputs [n_kf][n_mp] as orbx_keyframe_fuse_map_points: best_idx /
 * best_dist (-1 / 256 for no result), projected (may be NULL).  Key frames without inv_level_sigma2 are accepted, and the key frames of one call may
 * have different image bounds; n_kf <= ORBX_MAX_FUSE_KEYFRAMES.  The caller accepts best_dist <= ORBX_TH_LOW and runs the tail :1436-1449 per key frame
 * in the reference's order, re-checking isBad() / IsInKeyFrame on the live graph as for orbx_keyframe_fuse_map_points.  Four launches whatever n_kf is.
 * Refusals as above (ORBX_E_BAD_ARG before anything is enqueued); n_kf = 0 or n_mp = 0: ORBX_OK. */
int orbx_keyframe_fuse_map_points_sim3(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams, const orbx_frame_pose *poses,
                                       float th, float log_scale_factor, int n_mp, const float *pos, const float *normal, const float *min_dist,
                                       const float *max_dist, const uint8_t *mp_desc, const uint8_t *skip, int32_t *best_idx, int32_t *best_dist,
                                       uint8_t *projected);
/* The same two calls for FISHEYE-STEREO key frames (KeyFrame::NLeft != -1, KannalaBrandt8; a monocular key frame is refused).  The three members never
 * look at the right camera: GetFeaturesInArea(u, v, radius) with bRight = false, mvKeysUn[idx].octave, pKF->mpCamera -- so a key frame is ONE problem,
 * its left rows, left grid and N_left, and views holds n_kf entries (one per key frame, not two as orbx_keyframe_fuse_map_points_fisheye takes):
 * R, t = SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()), twc = Tcw.inverse().translation(), params = the LEFT camera's eight parameters.
 * The gates are the ones above, in that order and rounding; the projection is
 *   ORBX_SIM3_PROJECT_CAMERA: pKF->mpCamera->project(p3Dc) = KannalaBrandt8::project, the restatement orbx_is_in_frustum_checks uses (same bit contract,
 *     same one-ulp caveat), evaluated for pairs that are not skipped and lie in front of the camera;
 *   ORBX_SIM3_PROJECT_INVZ: the pinhole form as written at ORBmatcher.cc:573-578 with fx, fy, cx, cy = params[0..3] -- the reference writes it whatever
 *     the camera model is, with pKF->fx, fy, cx, cy: the caller puts those there (params[4..7] are not read).
 * orbx_keyframe_search_by_projection_sim3_fisheye: semantics, arguments and limits as orbx_keyframe_search_by_projection_sim3, except that match[k] and
 * occupied[k] hold N_k = N_left + N_right entries (orbx_keyframe_counts), the shape of vpMatched on a rig: occupied[k] is read for [0, N_left) only and
 * match[k][i] is always -1 for i >= N_left.  N_left <= ORBX_MAX_FRAME_FEATURES; bit-equal image bounds within one call; counts still on the device
 * cost that one download (orbx_keyframe_counts' path).
 * orbx_keyframe_fuse_map_points_sim3_fisheye: as orbx_keyframe_fuse_map_points_sim3; outputs [n_kf][n_mp], best_idx always below N_left (no N_left offset
 * is ever added).  Different bounds in one call and key frames without inv_level_sigma2 are accepted; counts still on the device come home with the
 * results and are known afterwards.  Four launches whatever n_kf is.
 * Refusals (ORBX_E_BAD_ARG / ORBX_E_TOO_LARGE before anything is enqueued): a monocular key frame, a key frame of another device, NULL rows,
 * projection_form not 0 / 1, proj_u without proj_v, unequal bounds in the search form, too many key frames or features.  n_kf = 0 or n_mp = 0: ORBX_OK,
 * match rows -1, nmatches 0. */
int orbx_keyframe_search_by_projection_sim3_fisheye(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fisheye_view *views, float th,
                                                    float ratio_hamming, float log_scale_factor, int projection_form, int n_mp, const float *pos,
                                                    const float *normal, const float *min_dist, const float *max_dist, const uint8_t *mp_desc,
                                                    const uint8_t *skip, const uint8_t *const *occupied, int32_t *const *match, int32_t *nmatches,
                                                    uint8_t *projected, float *proj_u, float *proj_v);
int orbx_keyframe_fuse_map_points_sim3_fisheye(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fisheye_view *views, float th,
                                               float log_scale_factor, int n_mp, const float *pos, const float *normal, const float *min_dist,
                                               const float *max_dist, const uint8_t *mp_desc, const uint8_t *skip, int32_t *best_idx, int32_t *best_dist,
                                               uint8_t *projected);

/* MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:329-403) for a batch of map points whose observations are rows of RESIDENT key frames: what
 * LocalMapping::ProcessNewKeyFrame, the "Update points" loop of LocalMapping::SearchInNeighbors, Tracking::CreateNewKeyFrame and the loop-correction
 * and merge code call per map point.  orbx_distinctive_descriptors takes the rows gathered on the host (32 bytes per observation go up); this call
 * takes where they are: set s is the observations [set_ptr[s], set_ptr[s+1]); observation o is row obs_idx[o] of mDescriptors of key frame
 * kfs[obs_kf[o]], in the reference's feature numbering.  The caller lists a map point's observations in std::map order, skips isBad() key frames, and
 * for a rig observation lists leftIndex, then rightIndex, each where it is not -1 (MapPoint.cc:345-356).
 * best_obs[s] = the position inside set s of the row with the least median Hamming distance to the set's rows -- the median is sorted element
 * (int)(0.5 * (N - 1)) of the N distances, the row's distance to itself included; the first minimum wins -- or -1 for an empty set.
 * best_desc: NULL, or [n_sets][32]: the winning row itself (zeros for an empty set) -- mDescriptor, assigned without touching a key frame.
 * Key frames of both kinds may be mixed; only descriptor rows are read.  Of a fisheye-stereo key frame an index i >= N_left names the right
 * camera's row i - N_left; the device translates it with the key frame's own counts, also while these are still on the device (a key frame made from
 * a batch-loaded frame) -- such a call brings the counts home with its results, and they are known afterwards.
 * Refusals, ORBX_E_BAD_ARG before anything is enqueued: an index outside [0, N) of a key frame whose count the host knows (outside [0, capacity) of
 * one whose counts are pending), obs_kf outside [0, n_kf), a decreasing set_ptr or set_ptr[0] < 0, a NULL array that would be read or written, a NULL
 * key frame or one of another device.  An index outside [0, N) of a key frame with pending counts is found by the kernel: no address is formed from
 * it, a flag comes home with the results and the call returns ORBX_E_BAD_ARG (the outputs are unspecified then).  n_kf above
 * ORBX_MAX_DISTINCTIVE_KEYFRAMES: ORBX_E_TOO_LARGE.  The size of a set has no limit (sets of up to 64 rows are held in registers, larger ones are
 * gathered into the call's scratch once).  n_sets = 0: ORBX_OK, nothing enqueued; n_kf = 0 and empty sets are fine.
 * Cost shape: one upload run (set_ptr, obs_kf, obs_idx, one 32-byte record per key frame), one kernel (a second one if a set holds more than 64 rows), one download run, one
 * synchronisation, whatever n_kf and n_sets are.  Sharing as every key-frame call: waits for each key frame's creation unless a call has done so before. */
#define ORBX_MAX_DISTINCTIVE_KEYFRAMES 4096
int orbx_keyframe_distinctive_descriptors(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, int n_sets, const int32_t *set_ptr,
                                          const int32_t *obs_kf, const int32_t *obs_idx, int32_t *best_obs, uint8_t *best_desc);

/* ---- Device-resident map points.  An orbx_map is a table of `capacity` slots on one device, one 64-byte record per slot: what the one-call searches
 * read of a MapPoint -- mWorldPos (pos), mNormalVector (normal), mfMinDistance / mfMaxDistance as GetMinDistanceInvariance() /
 * GetMaxDistanceInvariance() return them (min_dist, max_dist) and mDescriptor (desc, 32 bytes).  The caller addresses a slot by an id in
 * [0, capacity) that it assigns itself (one int in MapPoint).  A table is device-wide like a key frame: every matcher context of its device may write
 * and read it (a context of another device: ORBX_E_BAD_ARG).  The `_map` forms of the eight one-call searches below take (map, ids) where the flat
 * forms take pos, normal, min_dist, max_dist, mp_desc: 4 bytes per point go up instead of 64.
 *   orbx_map_create: capacity in [1, ORBX_MAX_MAP_POINTS] (ORBX_E_TOO_LARGE beyond, ORBX_E_BAD_ARG below 1); ORBX_E_HIP if the allocation fails.  No
 *     slot is live.
 *   orbx_map_update: writes row j of the given arrays into slot ids[j], j < n.  Any of the five field pointers may be NULL: that field of the
 *     slots keeps its value.  The first update of a slot (and the first after orbx_map_erase) must give all five: ORBX_E_BAD_ARG otherwise.  An id may
 *     be named once per call: a duplicate is refused with ORBX_E_BAD_ARG (a parallel scatter has no "last wins").  One upload run in m's arena, one
 *     launch (k_map_scatter); returns WITHOUT waiting.  n = 0: ORBX_OK.
 *   orbx_map_erase: MapPoint::SetBadFlag -- host bookkeeping only: the slots stop being live, and every call that names one is refused until an
 *     update has written it whole again.  All ids are checked first (each in [0, capacity) and live); n = 0: ORBX_OK.
 *   orbx_map_read: slot ids[j] -> row j of the outputs that are not NULL; one gather, one download run, one synchronisation.  For tests,
 *     serialization and debugging.  The same id may appear more than once.
 * Every call that takes ids checks them BEFORE anything is enqueued and before a transfer counter moves: ids not NULL when n > 0, each in
 * [0, capacity), its slot live, the map on m's device; a refused call changes neither the table nor the context (ORBX_E_BAD_ARG).
 * Ordering.  The table holds one event, `written`.  An update (orbx_map_update, orbx_keyframe_distinctive_descriptors_to_map,
 * orbx_keyframe_update_normal_and_depth_to_map, orbx_keyframe_refresh_map_points_to_map) makes its context's
 * stream wait for the previous `written`, launches and records the next one; every call that reads the table makes its stream wait for `written`
 * ahead of its gather, until a reading call that did so has synchronised.  So updates and reads issued one after the other, from any contexts and
 * threads, take effect in the order of the calls, and no host synchronisation is needed between an update and the search that follows it.
 * What the library does NOT order is a write against reads that are still RUNNING: as under the reference's Map::mMutexMapUpdate, the caller does not
 * run orbx_map_update / orbx_map_erase / ..._to_map on a table concurrently with a call that reads that table.  Every reading call ends in a
 * synchronisation, so once it has returned its reads are done.  Destroy a table before the matchers that used it and after every call that names it
 * has returned; orbx_map_destroy waits for `written`. */
typedef struct orbx_map orbx_map;
#define ORBX_MAX_MAP_POINTS (1 << 24)   /* 1 GiB of records */
int orbx_map_create(int device, int capacity, orbx_map **out);
void orbx_map_destroy(orbx_map *map);
int orbx_map_update(orbx_matcher *m, orbx_map *map, int n, const int32_t *ids, const float *pos, const float *normal, const float *min_dist,
                    const float *max_dist, const uint8_t *desc);
int orbx_map_erase(orbx_map *map, int n, const int32_t *ids);
int orbx_map_read(orbx_matcher *m, orbx_map *map, int n, const int32_t *ids, float *pos, float *normal, float *min_dist, float *max_dist,
                  uint8_t *desc);

/* The one-call searches with their map points named by id.  Each takes its flat form's arguments with (pos, normal, min_dist, max_dist, mp_desc)
 * replaced by (map, ids [n_mp]) and returns what the flat form returns for the rows of those slots, bit for bit.  The per-point arrays that are not
 * part of the table stay positional -- eligible, has_obs, skip, track_depth in, in_view, projected, proj_u / proj_v out: entry j belongs to ids[j] --
 * and every output indexes POSITIONS in ids, never ids.  The same id may appear twice: two queries with equal data, as the flat form given one row
 * twice.  Cost shape as the flat form -- one upload run (the ids lead it), one download run, one synchronisation, a launch chain independent of n_kf --
 * plus ONE launch, k_map_gather, which fills the flat form's five device arrays behind the wait for `written`. */
int orbx_frame_search_local_points_map(orbx_matcher *m, orbx_frame *frame, const uint8_t *frame_occupied, const orbx_camera *cam,
                                       const orbx_frame_pose *pose, float log_scale_factor, float viewing_cos_limit, int n_mp, orbx_map *map,
                                       const int32_t *ids, const uint8_t *eligible, const uint8_t *has_obs, float th, float nnratio, int far_points,
                                       float th_far_points, uint8_t *in_view, int32_t *frame_match);
int orbx_frame_search_local_points_fisheye_map(orbx_matcher *m, orbx_frame *frame, const uint8_t *frame_occupied, const orbx_fisheye_view *views,
                                               float log_scale_factor, float viewing_cos_limit, int n_mp, orbx_map *map, const int32_t *ids,
                                               const uint8_t *eligible, const uint8_t *has_obs, const float *track_depth, float th, float nnratio,
                                               int far_points, float th_far_points, uint8_t *in_view, int32_t *frame_match);
int orbx_keyframe_fuse_map_points_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams, const orbx_frame_pose *poses,
                                      float th, float log_scale_factor, int strict_fp, int n_mp, orbx_map *map, const int32_t *ids,
                                      const uint8_t *skip, int32_t *best_idx, int32_t *best_dist, uint8_t *projected);
int orbx_keyframe_fuse_map_points_fisheye_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fisheye_view *views, float th,
                                              float log_scale_factor, int strict_fp, int n_mp, orbx_map *map, const int32_t *ids, const uint8_t *skip,
                                              int32_t *best_idx, int32_t *best_dist, uint8_t *projected);
int orbx_keyframe_fuse_map_points_sim3_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams, const orbx_frame_pose *poses,
                                           float th, float log_scale_factor, int n_mp, orbx_map *map, const int32_t *ids, const uint8_t *skip,
                                           int32_t *best_idx, int32_t *best_dist, uint8_t *projected);
int orbx_keyframe_fuse_map_points_sim3_fisheye_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fisheye_view *views, float th,
                                                   float log_scale_factor, int n_mp, orbx_map *map, const int32_t *ids, const uint8_t *skip,
                                                   int32_t *best_idx, int32_t *best_dist, uint8_t *projected);
int orbx_keyframe_search_by_projection_sim3_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams,
                                                const orbx_frame_pose *poses, float th, float ratio_hamming, float log_scale_factor,
                                                int projection_form, int n_mp, orbx_map *map, const int32_t *ids, const uint8_t *skip,
                                                const uint8_t *const *occupied, int32_t *const *match, int32_t *nmatches, uint8_t *projected,
                                                float *proj_u, float *proj_v);
int orbx_keyframe_search_by_projection_sim3_fisheye_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fisheye_view *views, float th,
                                                        float ratio_hamming, float log_scale_factor, int projection_form, int n_mp, orbx_map *map,
                                                        const int32_t *ids, const uint8_t *skip, const uint8_t *const *occupied,
                                                        int32_t *const *match, int32_t *nmatches, uint8_t *projected, float *proj_u, float *proj_v);

/* The Tracking thread's two searches whose queries are ANOTHER frame's map points, from map ids, on a monocular / rectified resident frame:
 *   orbx_frame_track_last_frame_map               SearchByProjection(CurrentFrame, LastFrame, th, bMono)  (ORBmatcher.cc:1676-1887,
 *                                                 Tracking::TrackWithMotionModel); the source is `last`, a handle of the same matcher and kind
 *   orbx_frame_search_by_projection_keyframe_map  SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)  (:1889-2010,
 *                                                 Tracking::Relocalization); the source is `kf`, read for mvKeysUn[i].angle only
 * Their flat forms (orbx_frame_search_by_projection_frame / _window) take queries the caller projected on the host, about 70 bytes each.  Here
 * ids [n_ids] has one entry per feature of the source, n_ids = its N: the map slot of mvpMapPoints[i], or -1 (track_last_frame: no point or
 * mvbOutlier[i]; keyframe: no point, isBad(), or in sAlreadyFound).  The projection, the gates and the windows are evaluated on the device
 * (k_track_project reads the source's row and the slot's record directly: no k_map_gather, no flat arrays) in the order and rounding of the host
 * loops they replace:
 *   x3Dc = Rcw p + tcw (pose: the CURRENT frame's); track_last_frame: invzc = 1 / z, reject invzc < 0 -- keyframe: NO depth gate
 *   Pinhole::project; reject u < mnMinX || u > mnMaxX, likewise v (both sides inclusive)
 *   track_last_frame: ur = u - bf invzc; r = th * scale[octave of the source's row i], searched iff 0 <= octave < nlevels; levels by level_mode
 *                     (0: [o-1, o+1], 1: bForward, 2: bBackward -- the caller's, from the two poses and mb)
 *   keyframe:         dist3D = |p - Ow| within [0.8f mfMinDistance, 1.2f mfMaxDistance]; PredictScale(dist3D, &CurrentFrame) with
 *                     log_scale_factor; r = th * scale[l]; levels [l-1, l+1]; accepted iff (float)bestDist <= max_dist
 * cur_match / match [N of cur]: as the flat forms write them (-1 never assigned, -2 cleared by the rotation check), but a value >= 0 is the SOURCE
 * FEATURE INDEX i -- the caller writes Cur.mvpMapPoints[j] = Source.mvpMapPoints[match[j]].  has_obs [n_ids] (may be NULL: all true) as q_has_obs.
 * Optional outputs [n_ids]: projected[i] = 1 where entry i passed every gate above, proj_u / proj_v (both or neither) its (u, v).
 * The same id may appear twice.  The calls work while the counts of cur and of the source are still on the device: entries at or beyond the source's
 * count are switched off there.  One upload run (4 bytes per id, a flag byte, the occupancy mask), one download run, one synchronisation; the launches
 * of the flat handle form plus one.  Ordered against orbx_map_update as every reading call.
 * ORBX_E_BAD_ARG before anything is enqueued or a transfer counter moves: a NULL argument, cur or last of another matcher, a fisheye-stereo frame or
 * key frame, cur == last, a map on another device, an id outside {-1} and [0, capacity), an id whose slot is not live, n_ids different from the source's
 * count where the host knows it (above its capacity while it is pending), level_mode outside 0 .. 2; ORBX_E_TOO_LARGE as the flat forms. */
int orbx_frame_track_last_frame_map(orbx_matcher *m, orbx_frame *cur, orbx_frame *last, const uint8_t *cur_occupied, const orbx_camera *cam,
                                    const orbx_frame_pose *pose, orbx_map *map, int n_ids, const int32_t *ids, const uint8_t *has_obs, float th,
                                    int level_mode, int check_orientation, int32_t *cur_match, uint8_t *projected, float *proj_u, float *proj_v);
int orbx_frame_search_by_projection_keyframe_map(orbx_matcher *m, orbx_frame *cur, const uint8_t *occupied, const orbx_camera *cam,
                                                 const orbx_frame_pose *pose, float log_scale_factor, orbx_keyframe *kf, orbx_map *map, int n_ids,
                                                 const int32_t *ids, float th, float max_dist, int check_orientation, int32_t *match,
                                                 uint8_t *projected, float *proj_u, float *proj_v);

/* The same two searches for a fisheye-stereo rig (Frame::Nleft != -1): cur is a fisheye-stereo handle, `view` the LEFT camera's view of the CURRENT
 * frame (R = Rcw, t = tcw, twc = Ow, params = mpCamera's), and the projection is KannalaBrandt8::project (kb8_project) on the device.
 *   track_last_frame_fisheye  ORBmatcher.cc:1676-1887 with the twin :1794-1863.  `last` is a rig handle as well: ids has N = N_left + N_right entries,
 *                             octave / angle of entry i come from mvKeys[i] below N_left and from mvKeysRight[i - N_left] beyond.  Instead of ur the
 *                             point is carried into the right camera, x3Dr = Trl_R x3Dc + Trl_t (GetRelativePoseTrl()), and projected with the LEFT
 *                             parameters as the reference does (:1795-1796); both cameras are searched (k_replay_twin) and cur_match holds N entries.
 *   keyframe_fisheye          ORBmatcher.cc:1889-2010: the LEFT camera only is searched, as orbx_frame_search_by_projection_window_fisheye; kf is a rig
 *                             key frame, angle = mvKeysUn[i].angle below N_left and 0.f beyond; occupied / match hold N entries, the right camera's
 *                             entries of match stay -1.
 * Everything else -- ids, -1, match values, the optional outputs, the checks, the cost shape -- as the two calls above; a monocular / rectified frame or
 * key frame is refused here as a rig is there. */
int orbx_frame_track_last_frame_fisheye_map(orbx_matcher *m, orbx_frame *cur, orbx_frame *last, const uint8_t *cur_occupied,
                                            const orbx_fisheye_view *view, const float *Trl_R9, const float *Trl_t3, orbx_map *map, int n_ids,
                                            const int32_t *ids, const uint8_t *has_obs, float th, int level_mode, int check_orientation,
                                            int32_t *cur_match, uint8_t *projected, float *proj_u, float *proj_v);
int orbx_frame_search_by_projection_keyframe_fisheye_map(orbx_matcher *m, orbx_frame *cur, const uint8_t *occupied, const orbx_fisheye_view *view,
                                                         float log_scale_factor, orbx_keyframe *kf, orbx_map *map, int n_ids, const int32_t *ids,
                                                         float th, float max_dist, int check_orientation, int32_t *match, uint8_t *projected,
                                                         float *proj_u, float *proj_v);

/* orbx_keyframe_distinctive_descriptors with the winning rows written straight into the table: the same sets, the same two kernels and the same
 * result run (best_obs -- mDescriptor's provenance -- still comes home), then k_map_scatter_desc writes set s's winning row into the descriptor of
 * slot set_id[s], ordered as an update.  An empty set (best_obs = -1) leaves its slot untouched.  set_id [n_sets] must name live slots without
 * duplicates (ORBX_E_BAD_ARG before anything is enqueued).  If the kernel finds an index outside [0, N) of a key frame with pending counts, NOTHING
 * is written to the table and the call returns ORBX_E_BAD_ARG as orbx_keyframe_distinctive_descriptors does. */
int orbx_keyframe_distinctive_descriptors_to_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, int n_sets, const int32_t *set_ptr,
                                                 const int32_t *obs_kf, const int32_t *obs_idx, orbx_map *map, const int32_t *set_id,
                                                 int32_t *best_obs);

/* MapPoint::UpdateNormalAndDepth (MapPoint.cc, the member the reference calls right behind ComputeDistinctiveDescriptors in
 * LocalMapping::ProcessNewKeyFrame, the "Update points" loop of SearchInNeighbors, Tracking::CreateNewKeyFrame and the loop-correction and merge
 * code) for a batch of map points whose observations are features of RESIDENT key frames.  The observation list is
 * orbx_keyframe_distinctive_descriptors' (set_ptr, obs_kf, obs_idx: std::map order, leftIndex then rightIndex of a rig observation), and so are the
 * key frames.  In addition:
 *   centers [n_kf][3]        GetCameraCenter() of each key frame
 *   centers_right [n_kf][3]  GetRightCameraCenter(); may be NULL if no key frame of kfs is a fisheye-stereo one (rows of monocular ones are not read)
 *   ref_obs [n_sets]         the position inside set s of the observation in mpRefKF -- on a rig the left one where both exist; ignored for an empty set
 *   pos [n_sets][3]          mWorldPos (flat form); the `_to_map` forms read it from the slots
 * The member as the device evaluates it, every float operation rounded on its own:
 *   for observation o of the set, in the order of the list:
 *       Owi = centers[obs_kf[o]] if obs_idx[o] < N_left or the key frame is monocular, centers_right[obs_kf[o]] otherwise
 *       normali = Pos - Owi                          three subtractions
 *       norm = sqrt(dot3(normali, normali))          ((0 + x x) + y y) + z z, correctly rounded square root     [Eigen-internal, unpinned]
 *       normal = normal + normali / norm             three true divisions, three additions                      [Eigen-internal, unpinned]
 *   mNormalVector = normal / (float)n                three divisions, n = the size of the set
 *   PC = Pos - centers[key frame of ref_obs]         ALWAYS the left centre
 *   dist = sqrt(dot3(PC, PC)); level = the octave of the reference observation's key point (mvKeysUn / mvKeys / mvKeysRight by its index)
 *   mfMaxDistance = dist * mvScaleFactors[level];  mfMinDistance = mfMaxDistance / mvScaleFactors[mnScaleLevels - 1]
 * The two distances are UNSCALED, as the member leaves them and as the table stores them (the device's gates apply 0.8f / 1.2f themselves).  A term
 * with Pos == Owi is 0 / 0 = NaN here as in the reference.  An empty set is the member's early return: its entries of normal, min_dist, max_dist keep
 * the caller's values and its slot is not written.
 *   orbx_keyframe_update_normal_and_depth          flat: pos in; normal [n_sets][3], min_dist, max_dist [n_sets] out (all three required)
 *   orbx_keyframe_update_normal_and_depth_to_map   pos is read from slot set_id[s], and normal, min_dist, max_dist are written into it (pos and the
 *                                                  descriptor keep their bits).  normal / min_dist / max_dist: each NULL or an output as above; with
 *                                                  all three NULL only the flag and any pending counts come home.  The host's mNormalVector /
 *                                                  mfMinDistance / mfMaxDistance go stale unless they are requested.
 *   orbx_keyframe_refresh_map_points_to_map        both members in one call: orbx_keyframe_distinctive_descriptors_to_map followed by
 *                                                  orbx_keyframe_update_normal_and_depth_to_map (normal = min_dist = max_dist = NULL), bit for bit,
 *                                                  with one upload run, one launch chain, one download run (best_obs), one synchronisation.
 * The `_to_map` forms are updates of the table that also read it: they wait for `written`, launch, record `written` anew under the map's mutex -- and,
 * unlike orbx_map_update, end in the call's one synchronisation.  After them only SetWorldPos (a bundle adjustment's write-back) is left to
 * orbx_map_update.
 * Refusals, ORBX_E_BAD_ARG before anything is enqueued or a transfer counter moves: everything orbx_keyframe_distinctive_descriptors[_to_map]
 * refuses; centers NULL; centers_right NULL while a fisheye-stereo key frame is in kfs; ref_obs NULL; ref_obs[s] outside [0, size of set s) for a
 * non-empty set; pos NULL (flat form); an output NULL (flat form); set_id NULL, not live, out of range or named twice; a map on another device.  An
 * index outside [0, N) behind pending counts, or a reference key point whose octave is outside [0, nlevels), is found by the kernel: no address is formed
 * from it, NOTHING is written to the table and the call returns ORBX_E_BAD_ARG (the flat outputs are unspecified then).  n_sets = 0: ORBX_OK, nothing
 * enqueued.
 * Cost shape: one upload run (the distinctive call's, plus ref_obs, one 64-byte record per key frame that holds the two centres, and pos in the flat
 * form), one download run, one synchronisation, and a launch chain independent of n_kf and n_sets: k_normal_depth_kf (one wave per set; a set of
 * more than 64 observations is walked in chunks by the same wave) and, `_to_map`, one k_map_scatter_refresh; the refresh call runs k_distinctive_kf
 * (+ k_distinctive_kf_large) in front of them. */
int orbx_keyframe_update_normal_and_depth(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const float *centers, const float *centers_right,
                                          int n_sets, const int32_t *set_ptr, const int32_t *obs_kf, const int32_t *obs_idx, const int32_t *ref_obs,
                                          const float *pos, float *normal, float *min_dist, float *max_dist);
int orbx_keyframe_update_normal_and_depth_to_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const float *centers,
                                                 const float *centers_right, int n_sets, const int32_t *set_ptr, const int32_t *obs_kf,
                                                 const int32_t *obs_idx, const int32_t *ref_obs, orbx_map *map, const int32_t *set_id, float *normal,
                                                 float *min_dist, float *max_dist);
int orbx_keyframe_refresh_map_points_to_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const float *centers, const float *centers_right,
                                            int n_sets, const int32_t *set_ptr, const int32_t *obs_kf, const int32_t *obs_idx,
                                            const int32_t *ref_obs, orbx_map *map, const int32_t *set_id, int32_t *best_obs);

/* Frame::ComputeStereoMatches (Frame.cc:811-981) for every frame of two resident batches: `left` and `right` must have
 * extracted batches of the same size and image shape (rectified stereo, lapping {0,0}).  Row-band Hamming match, 11x11
 * SAD sub-pixel refinement on the device-resident pyramids and the median outlier rejection all run on the device, on
 * the left extractor's MATCH stream: the next pair of batches may be extracted meanwhile (from the first call on both
 * extractors alternate between two pyramid slabs, and their next k_finalize waits for this stage as for a matcher of
 * their own).  Results (mvuRight, mvDepth; -1 = no match) per frame via orbx_stereo_batch_download[_all | _async]. */
int orbx_stereo_batch_device(orbx_extractor *left, orbx_extractor *right, float bf, float b);
int orbx_stereo_batch_download(orbx_extractor *left, int frame, float *u_right, float *depth, int *n_left, int *n_matches);
/* all frames at once: u_right / depth [n_frames][cap] (entries beyond a frame's keypoint count unspecified), n_matches [n_frames] */
int orbx_stereo_batch_download_all(orbx_extractor *left, float *u_right, float *depth, int32_t *n_matches);
/* the same into PINNED host buffers, asynchronously behind the stereo kernels (at most two such downloads in flight): the next pair of batches
 * can be extracted meanwhile; orbx_stereo_download_wait returns when the buffers of the OLDER one are complete */
int orbx_stereo_batch_download_async(orbx_extractor *left, float *u_right, float *depth, int32_t *n_matches);
int orbx_stereo_download_wait(orbx_extractor *left);

/* ---- rectified-stereo / RGB-D depth on the extractor's batch and on frame handles ----
 * Frame::ComputeStereoFromRGBD for every frame of `ex`'s last batch (k_stereo_from_rgbd).  d_depth: DEVICE memory, one float32 depth image of the
 * extractor's width x height per frame, pitch_bytes per row, frame_stride_bytes per image, already scaled (what GrabImageRGBD hands to Frame
 * after convertTo).  Per feature i:  u = mvKeys[i].pt.x, v = mvKeys[i].pt.y (the RAW key point);  d = imDepth.at<float>(v, u), both coordinates
 * converted to int by truncation;  d > 0: mvDepth[i] = d, mvuRight[i] = mvKeysUn[i].pt.x - bf / d (one true division, one subtraction;
 * mvKeysUn = the rows orbx_set_camera undistorts);  else mvDepth[i] = mvuRight[i] = -1 (a NaN depth therefore gives -1).  A coordinate outside
 * the image forms no address and gives -1.  The results lie where orbx_stereo_batch_device leaves its own -- with n_matches = the features with
 * d > 0 -- so orbx_stereo_batch_download[_all | _async] serve both sources.  Enqueued behind the extraction on the MATCH stream, no host
 * synchronisation: the depth images must stay valid until orbx_sync or a download has returned.  ORBX_E_BAD_ARG, before anything is enqueued:
 * a NULL argument, no batch, pitch_bytes < 4 * width, !(bf > 0), and d_depth, pitch_bytes or frame_stride_bytes not a multiple of 4 (every row is a
 * row of aligned floats).  frame_stride_bytes is otherwise the caller's: images may overlap or repeat.
 * Both stages stamp the (left) extractor with the batch their results belong to; orbx_frame_load_stereo_batch checks the stamp. */
int orbx_rgbd_batch_device(orbx_extractor *ex, const float *d_depth, size_t pitch_bytes, size_t frame_stride_bytes, float bf);
/* The same on the depth image as the sensor delivers it (k_stereo_from_rgbd_u16): d_depth = DEVICE memory, one uint16 image per frame, and
 * depth_factor = the float mDepthMapFactor (1.0f / DepthMapFactor, as Tracking stores it).  Tracking::GrabImageRGBD's
 * imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) happens at the one pixel a feature reads:  d = (float)raw * depth_factor, one rounded float
 * product (what convertTo's float scale path gives with a zero shift; the conversion of 16 bits is exact) -- and from there exactly as above.
 * ORBX_E_BAD_ARG as above with pitch_bytes < 2 * width, d_depth / pitch_bytes / frame_stride_bytes odd, and a depth_factor that is not finite
 * and above 0. */
int orbx_rgbd_batch_device_u16(orbx_extractor *ex, const uint16_t *d_depth, size_t pitch_bytes, size_t frame_stride_bytes, float depth_factor, float bf);
/* A frame WITH depth on the handle: besides orbx_frame_load_batch's / orbx_frame_load_host's rows the handle then holds mvuRight, mvDepth and the raw
 * mvKeys[i].pt, and every handle call treats it as the monocular / rectified frame it is (those that read mvuRight read the resident row).
 *   orbx_frame_load_stereo_batch: orbx_frame_load_batch plus frame `frame`'s mvuRight / mvDepth of `left`'s last orbx_stereo_batch_device or
 *     orbx_rgbd_batch_device and its raw key points, copied on the device in the same launch, behind the stage.  ORBX_E_BAD_ARG when no stage has
 *     run or its results are not those of the extractor's current batch (an extraction since); otherwise orbx_frame_load_batch's refusals.
 *   orbx_frame_load_host_stereo: orbx_frame_load_host with desc->u_right and depth [n] required; keys_xy [n][2] = mvKeys[i].pt (NULL: keypoints_un's).
 * The other loads leave a handle without depth.
 *   orbx_frame_unproject_stereo: Frame::UnprojectStereo for every feature (k_unproject_stereo; view: Rcw, Ow, fx, fy, cx, cy are read):
 *       z = mvDepth[i];  nothing unless z > 0;  u, v = mvKeysUn[i].pt;  x = (u - cx) * z * invfx;  y = (v - cy) * z * invfy   (invfx = 1.0f / fx)
 *       x3D = mRwc * (x, y, z) + mOw                                     (Rwc = Rcw.transpose(); each row a dot() plus one addition)
 *     under the float contract stated at orbx_keyframe_triangulate_pairs.  u_right / depth [N] (the frame's rows), pos [N][3] (written where
 *     depth > 0, the caller's values elsewhere), n_with_depth: each may be NULL.  One launch, one download run, one synchronisation; a pending
 *     count comes home with the results.  ORBX_E_BAD_ARG for a handle without depth, a fisheye handle, another matcher's handle. */
int orbx_frame_load_stereo_batch(orbx_frame *f, orbx_extractor *left, int frame, const float *bounds4, const float *scale_factors, int nlevels);
int orbx_frame_load_host_stereo(orbx_frame *f, const orbx_frame_desc *desc, const float *depth, const float *keys_xy);
int orbx_frame_unproject_stereo(orbx_matcher *m, orbx_frame *f, const orbx_new_points_view *view, float *u_right, float *depth, float *pos,
                                int *n_with_depth);
/* Depth on key frames.  orbx_keyframe_from_frame copies mvDepth and the raw key points when, and only when, the handle holds them (a key frame made
 * from a handle without depth has the size and the contents it always had); orbx_keyframe_create_host_stereo is orbx_keyframe_create_host with
 * desc->u_right and depth [n] required and keys_xy [n][2] = mvKeys[i].pt (NULL: keypoints_un's).  Fisheye key frames hold no depth.
 *
 * The stereo branches of LocalMapping::CreateNewMapPoints: the `_stereo` forms take every argument of orbx_keyframe_triangulate_pairs /
 * orbx_keyframe_search_and_triangulate plus `st` behind `par`, share their implementation (k_new_points_stereo is k_new_points' body with the
 * branches below switched on) and their cost shape; the record they send is 48 bytes longer.  ORBX_NEWPT_STEREO_LEFT_TO_HOST remains for a stereo
 * observation (mvuRight >= 0) on a key frame that holds mvuRight but no mvDepth; ORBX_NEWPT_UNPROJECT_FAILED is UnprojectStereo returning false.
 * A pair without a stereo observation takes the existing forms' path with their bits.  The member's stereo text, ORB-SLAM3 v1.0, restated (PARITY
 * UNPINNED as the text above: no reference tree compiles LocalMapping.cc here, and where one is at hand its text wins):
 *   bStereo1 = !KF1.mpCamera2 && mvuRight1[idx1] >= 0          (bStereo2 alike)
 *   cosParallaxStereo = cosParallaxRays + 1;  cosParallaxStereo1 = cosParallaxStereo2 = cosParallaxStereo
 *   if (bStereo1)      cosParallaxStereo1 = cos(2 * atan2(KF1.mb / 2, KF1.mvDepth[idx1]));
 *   else if (bStereo2) cosParallaxStereo2 = cos(2 * atan2(KF2.mb / 2, KF2.mvDepth[idx2]));     "else if": with bStereo1 the second stays cosParallaxRays + 1
 *   cosParallaxStereo = min(cosParallaxStereo1, cosParallaxStereo2);
 *   if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || cosParallaxRays < (mbInertial ? 0.9996 : 0.9998)))
 *         Triangulate as above (ORBX_NEWPT_TRIANGULATE_FAILED on false)
 *   else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2)  ok = KF1.UnprojectStereo(idx1, x3D)
 *   else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1)  ok = KF2.UnprojectStereo(idx2, x3D)
 *   else continue                                                                              ORBX_NEWPT_LOW_PARALLAX
 *   if (!ok) continue                                                                          ORBX_NEWPT_UNPROJECT_FAILED
 *   KeyFrame::UnprojectStereo(i): z = mvDepth[i]; false unless z > 0; u, v = mvKeys[i].pt (the RAW key point, unlike Frame's member);
 *         x3D = mRwc * ((u - cx) * z * invfx, (v - cy) * z * invfy, z) + Ow
 *   z1, z2 tests as above.  Reprojection in key frame 1 when bStereo1 (key frame 2 alike with its own values):
 *         invz1 = 1.0 / z1;  u1 = fx1 * x1 * invz1 + cx1;  u1_r = u1 - KF1.mbf * invz1;  v1 = fy1 * y1 * invz1 + cy1
 *         errX1 = u1 - kp1.pt.x;  errY1 = v1 - kp1.pt.y;  errX1_r = u1_r - mvuRight1[idx1]
 *         if ((errX1*errX1 + errY1*errY1 + errX1_r*errX1_r) > 7.8 * mvLevelSigma2_1[kp1.octave]) continue          ORBX_NEWPT_REPROJ_1
 *      when !bStereo1: camera->project and 5.991, as above.  The rest of the member as above.
 * As the device evaluates it: LocalMapping.cc is compiled under `using namespace std`, so the float overloads are taken -- mb / 2 a float halving,
 * atan2 glibc's atan2f, the product with 2 exact, cos glibc's cosf (the "fma" variant the oracle's orbo_cosf restates), min(a, b) = b < a ? b : a;
 * invz the correctly rounded float quotient; u1 = ((fx x1) invz1) + cx1, two products, each rounded, and a sum (u1_r, v1 alike); the three squares
 * summed left to right in float and compared in double with 7.8 * (double)sigma2; UnprojectStereo is orbx_frame_unproject_stereo's arithmetic on
 * the key frame's raw (x, y) and mvDepth rows with the view's Rcw and Ow. */
typedef struct orbx_new_points_stereo { float mb1, mbf1, mb2, mbf2; } orbx_new_points_stereo;   /* KeyFrame::mb, mbf of KF1 / KF2 */
/* status 12, behind the enum above: only the `_stereo` forms report it (KeyFrame::UnprojectStereo returned false: mvDepth <= 0), so the enum of the
 * forms that never do stays as it is */
#define ORBX_NEWPT_UNPROJECT_FAILED 12
int orbx_keyframe_create_host_stereo(orbx_matcher *m, const orbx_frame_desc *desc, const float *depth, const float *keys_xy,
                                     const float *inv_level_sigma2, orbx_keyframe **out);
int orbx_keyframe_triangulate_pairs_stereo(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const orbx_new_points_view *view1,
                                           const orbx_new_points_view *view2, const orbx_new_points_params *par, const orbx_new_points_stereo *st,
                                           int n_pairs, const int32_t *idx1, const int32_t *idx2, float *pos, uint8_t *status, int *n_accepted);
int orbx_keyframe_search_and_triangulate_stereo(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                                int check_orientation, const orbx_keyframe_gate *gate, const orbx_new_points_view *view1,
                                                const orbx_new_points_view *view2, const orbx_new_points_params *par,
                                                const orbx_new_points_stereo *st, int32_t *matches12, float *pos, uint8_t *status, int *n_accepted);

/* ---- The BowVector on the device and the key-frame database: KeyFrameDatabase::add / erase / clear and the first halves of
 * DetectRelocalizationCandidates / DetectNBestCandidates (PARITY UNPINNED: DBoW2 and KeyFrameDatabase.cc are not compiled against this library by
 * any test; what follows restates them and the tests compare with that restatement, bit for bit) ----
 * TemplatedVocabulary::transform(features, v, fv, levelsup) with TF_IDF weighting and L1_NORM scoring (TemplatedVocabulary.h:1151-1193), the BowVector
 * half:
 *   for every feature, in feature order:  transform(*fit, id, w, &nid, levelsup);  if (w > 0) v.addWeight(id, w);
 *   BowVector::addWeight(id, w):  a new word is inserted with the value w; a word that is there gets `vit->second += w` -- ONE double addition per
 *         occurrence.  All occurrences of a word add the same w, so the feature order does not matter, but the NUMBER of sequential additions does:
 *         w added five times to w differs from 6.0 * w for about half of all doubles (two to five occurrences are exact).
 *   v.normalize(L1):  norm = 0.0;  for every entry of the std::map, in ascending word id:  norm += fabs(value);  if (norm > 0.0) every value /= norm.
 * L1Scoring::score(v1, v2) (ScoringObject.cc), v1 the query's vector, v2 the key frame's:
 *   score = 0;  over the words both hold, in ascending id:  score += fabs(vi - wi) - fabs(vi) - fabs(wi);   (left to right)
 *   return -score / 2.0;                                    (a pair without a common word scores -0.0)
 * No expression holds a multiply-add, so contraction cannot fork it; the ORDER of the additions is the whole parity question -- a tree or a
 * per-lane partial sum differs from the sequential one in the last bit for most inputs -- and every sum here runs in word order on one accumulator.
 * KeyFrameDatabase::DetectRelocalizationCandidates(F) / DetectNBestCandidates(pKF, ...) (KeyFrameDatabase.cc), first halves:
 *   mnRelocWords / mnPlaceRecognitionWords of a key frame = the words its mBowVec shares with the query's (the inverted-file walk counts them);
 *   DetectNBestCandidates skips the key frames of spConnectedKF before it counts, so they do not enter the maximum;
 *   maxCommonWords = the largest count;  int minCommonWords = maxCommonWords * 0.8f;   (int -> float, a float product, truncation)
 *   every key frame with more than minCommonWords common words gets si = score(query, key frame);  no key frame sharing a word: an empty result.
 * Here the inverted file is replaced by brute force over all slots (sparse-vector arithmetic on resident data).  Left to the host: everything
 * behind these lines -- GetBestCovisibilityKeyFrames, the accumulated scores, 0.75f * bestAccScore, the map filter.
 *
 * orbx_frame_bow_vector / orbx_keyframe_bow_vector: mBowVec of a handle that has BoW (orbx_frame_compute_bow[_fisheye], orbx_keyframe_compute_bow
 *   [_fisheye] / orbx_keyframe_bow_from_frame[_fisheye]): word_id ascending, value normalised, *n_words entries each, built on the device from the
 *   kept per-feature word ids (k_bow_vector).  Handles of both kinds: for a fisheye-stereo handle the rows of both cameras form ONE vector over all
 *   N rows, as Frame::ComputeBoW makes it.  The count may still be on the device only: buffers of the handle's capacity (a key frame's: N, or the
 *   capacity of the handle it was made from) always suffice.  ORBX_E_BAD_ARG: no BoW, a vocabulary without orbx_vocabulary_set_word_weights, a
 *   handle of another matcher / device.  One launch, one download run, one synchronisation.
 * orbx_keyframe_database: n_slots rows of words_cap entries (word id, double value) and each row's word count, owned by the database, on one
 *   device; any matcher context of that device may write and query it (another device: ORBX_E_BAD_ARG).  The caller numbers the slots, as it
 *   numbers an orbx_map's.  n_slots in [1, ORBX_MAX_DATABASE_SLOTS], words_cap in [1, 16384] (ORBX_E_TOO_LARGE beyond, ORBX_E_BAD_ARG below).
 *   _add: the key frame's BowVector is built straight into the row of `slot` (k_bow_vector), replacing what the slot held; stream order, no host
 *     wait.  The row is a COPY: the key frame may be destroyed afterwards.  Refused before anything is enqueued: a key frame without BoW or whose
 *     vocabulary has no weights, a vocabulary or levelsup other than that of the first key frame added (since the last _clear), a key frame or a
 *     database of another device, a slot outside [0, n_slots) (all ORBX_E_BAD_ARG); a key frame whose row bound exceeds words_cap
 *     (ORBX_E_TOO_LARGE; the bound is N where the host knows it, the key frame's capacity otherwise).
 *   _erase: the slot is empty from here on, in stream order (an empty slot: no effect).  _clear: every slot.
 *   _query_frame / _query_keyframe: the query's BowVector is built in the call's arena (the query key frame need not be in the database; it counts
 *     against its own slot if it is), every slot is compared with it (k_bow_score) and the candidates are chosen (k_bow_select).
 *     exclude [n_exclude]: slots that are not counted (spConnectedKF), each in [0, n_slots).  min_ratio in [0, 1]: the reference's 0.8f.
 *     n_common / score (optional, n_slots entries each): the common words of every slot, -1 for an empty or excluded one, and
 *     L1Scoring::score(query, slot) of every counted slot, -0.0 included (0.0 where n_common is -1).
 *     The candidates: the slots with n_common > (int)((float)max_common * min_ratio) and at least one common word, in ascending slot order, with
 *     their counts and scores (cand_common / cand_score optional).  *n_cand is the true count also when it exceeds cand_cap: the list is then cut
 *     and the status stays ORBX_OK.  *max_common = maxCommonWords; 0 gives *n_cand = 0.
 *     Refused before anything is enqueued (ORBX_E_BAD_ARG): a source without BoW or weights, a vocabulary / levelsup other than the database's, an
 *     exclude id out of range, min_ratio outside [0, 1], another device.
 *     Cost shape: one upload run (the exclude list), three launches whatever n_slots is, one download run, one synchronisation.
 * Ordering, as an orbx_map's: the database holds one event, `written`.  _add, _erase and _clear make their context's stream wait for the previous
 * `written`, enqueue and record the next; a query makes its stream wait for `written` ahead of its kernels until a query that did so has
 * synchronised.  So writes and queries issued one after the other, from any contexts and threads, take effect in the order of the calls, with no
 * host synchronisation between an add and the query behind it.  NOT ordered: a write against a query that is still RUNNING -- as under
 * KeyFrameDatabase::mMutex, the caller does not write while another thread's query has not returned.  Destroy a database after every call that names
 * it has returned and before the matchers that used it; orbx_keyframe_database_destroy waits for `written`. */
typedef struct orbx_keyframe_database orbx_keyframe_database;
#define ORBX_MAX_DATABASE_SLOTS (1 << 20)
int orbx_frame_bow_vector(orbx_matcher *m, orbx_frame *f, int32_t *word_id, double *value, int *n_words);
int orbx_keyframe_bow_vector(orbx_matcher *m, orbx_keyframe *kf, int32_t *word_id, double *value, int *n_words);
int orbx_keyframe_database_create(int device, int n_slots, int words_cap, orbx_keyframe_database **out);
void orbx_keyframe_database_destroy(orbx_keyframe_database *db);
int orbx_keyframe_database_add(orbx_matcher *m, orbx_keyframe_database *db, int slot, orbx_keyframe *kf);
int orbx_keyframe_database_erase(orbx_matcher *m, orbx_keyframe_database *db, int slot);
int orbx_keyframe_database_clear(orbx_matcher *m, orbx_keyframe_database *db);
int orbx_keyframe_database_query_frame(orbx_matcher *m, orbx_keyframe_database *db, orbx_frame *f, const int32_t *exclude, int n_exclude,
                                       float min_ratio, int32_t *n_common, double *score, int32_t *cand_slot, int32_t *cand_common,
                                       double *cand_score, int cand_cap, int *n_cand, int *max_common);
int orbx_keyframe_database_query_keyframe(orbx_matcher *m, orbx_keyframe_database *db, orbx_keyframe *kf, const int32_t *exclude, int n_exclude,
                                          float min_ratio, int32_t *n_common, double *score, int32_t *cand_slot, int32_t *cand_common,
                                          double *cand_score, int cand_cap, int *n_cand, int *max_common);

const char *orbx_last_error(void);
const char *orbx_status_string(int status);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H */
