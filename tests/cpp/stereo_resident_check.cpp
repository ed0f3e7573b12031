// Rectified-stereo / RGB-D depth on resident frames and key frames: orbx_rgbd_batch_device, orbx_frame_load_stereo_batch,
// orbx_frame_load_host_stereo, orbx_frame_unproject_stereo, orbx_keyframe_create_host_stereo and the two `_stereo` forms of CreateNewMapPoints'
// triangulation, against Frame::ComputeStereoFromRGBD, Frame::UnprojectStereo and the member's loop with its stereo branches written out below.
// The caller's arrays are heap blocks of exactly the needed size with the last row in use, filled with a sentinel.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt, whose
// stand-in runtime takes any host pointer as device memory) and compiled with -fsanitize=address,undefined.  Prints "stereo resident ok", returns 0.
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

constexpr float kSentinel = -12345.f;
constexpr uint8_t kStatusSentinel = 99;

#define MUST(expr)                                                                   \
    do {                                                                             \
        const int r_ = (expr);                                                       \
        if (r_ < 0) { printf("%s: %d %s\n", #expr, r_, orbx_last_error()); return 1; } \
    } while (0)
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

inline float dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return ((0.f + a0 * b0) + a1 * b1) + a2 * b2; }

// Frame::UnprojectStereo / KeyFrame::UnprojectStereo for one key point (u, v) with depth z > 0
void unproject(const orbx_new_points_view &V, float u, float v, float z, float *X) {
    const float invfx = 1.0f / V.fx, invfy = 1.0f / V.fy;
    const float x = (u - V.cx) * z * invfx, y = (v - V.cy) * z * invfy;
    for (int r = 0; r < 3; r++) X[r] = dot3(V.Rcw[r], V.Rcw[3 + r], V.Rcw[6 + r], x, y, z) + V.Ow[r];   // mRwc * x3Dc + mOw
}

// ---------------------------------------------------------------------------------------------------------
// part 1: the RGB-D stage on an extracted batch, both loads, UnprojectStereo
// ---------------------------------------------------------------------------------------------------------
constexpr int kW = 320, kH = 240, kFrames = 2, kPitchFloats = kW + 5;

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

int frames_part() {
    const std::vector<uint8_t> img = make_images();
    const orbx_params prm = {500, 1.2f, 8, 20, 7, 0};
    orbx_extractor *ex = nullptr;
    MUST(orbx_create(&prm, 0, kW, kH, kFrames, &ex));
    orbx_camera cam;
    memset(&cam, 0, sizeof(cam));
    cam.fx = 265.f; cam.fy = 262.f; cam.cx = 161.5f; cam.cy = 118.25f; cam.k1 = -0.28f; cam.k2 = 0.07f; cam.bf = 40.f;
    MUST(orbx_set_camera(ex, &cam));
    MUST(orbx_extract_batch_host(ex, img.data(), kFrames, kW, kH, kW, (size_t)kW * kH, 0, 0));
    // the depth images: a heap block of exactly kFrames * kH rows of kPitchFloats, a ramp with holes, garbage in the padding
    const size_t pitch = 4 * (size_t)kPitchFloats, frame_stride = pitch * kH;
    std::unique_ptr<float[]> depth_img(new float[(size_t)kFrames * kH * kPitchFloats]);
    for (int f = 0; f < kFrames; f++)
        for (int y = 0; y < kH; y++)
            for (int x = 0; x < kPitchFloats; x++) {
                float d = 0.5f + 0.01f * (float)x + 0.003f * (float)y + (float)f;
                if (x >= kW) d = 777.f;
                else if (x >= 40 && x < 70) d = 0.f;
                else if (x >= 100 && x < 130) d = -1.f;
                else if (x >= 160 && x < 190) d = NAN;
                depth_img[((size_t)f * kH + y) * kPitchFloats + x] = d;
            }
    const float bf = 40.f;
    CHECK(orbx_rgbd_batch_device(ex, depth_img.get(), 4 * (size_t)kW - 4, frame_stride, bf) == ORBX_E_BAD_ARG);
    CHECK(orbx_rgbd_batch_device(ex, depth_img.get(), pitch, frame_stride, 0.f) == ORBX_E_BAD_ARG);
    CHECK(orbx_rgbd_batch_device(ex, nullptr, pitch, frame_stride, bf) == ORBX_E_BAD_ARG);
    orbx_matcher *m = nullptr;
    MUST(orbx_matcher_create(0, &m));
    const int cap = orbx_output_capacity(ex, kW, kH);
    CHECK(cap > 0);
    orbx_frame *A = nullptr, *B = nullptr;
    MUST(orbx_frame_create(m, cap, &A));
    MUST(orbx_frame_create(m, cap, &B));
    CHECK(orbx_frame_load_stereo_batch(A, ex, 0, nullptr, nullptr, 0) == ORBX_E_BAD_ARG);   // no stage has run yet
    MUST(orbx_rgbd_batch_device(ex, depth_img.get(), pitch, frame_stride, bf));
    orbx_new_points_view V;
    const float R[9] = {0.9995f, 0.01f, -0.03f, -0.0097f, 0.9999f, 0.01f, 0.0301f, -0.0097f, 0.9995f};
    memcpy(V.Rcw, R, sizeof(R));
    V.tcw[0] = 0.1f; V.tcw[1] = -0.2f; V.tcw[2] = 0.3f; V.Ow[0] = -0.11f; V.Ow[1] = 0.2f; V.Ow[2] = -0.29f;
    V.fx = cam.fx; V.fy = cam.fy; V.cx = cam.cx; V.cy = cam.cy;
    for (int f = 0; f < kFrames; f++) {
        std::vector<orbx_keypoint> kps((size_t)cap), kun((size_t)cap);
        std::vector<uint8_t> desc(32 * (size_t)cap);
        std::vector<float> ur((size_t)cap, kSentinel), dep((size_t)cap, kSentinel);
        int n = 0, mono = 0, n_un = 0, n_left = 0, n_with = 0;
        MUST(orbx_batch_download(ex, f, kps.data(), desc.data(), cap, &n, &mono));
        MUST(orbx_batch_download_keypoints_un(ex, f, kun.data(), cap, &n_un));
        MUST(orbx_stereo_batch_download(ex, f, ur.data(), dep.data(), &n_left, &n_with));
        CHECK(n > 100 && n_un == n && n_left == n);
        int want_with = 0, moved = 0;
        for (int i = 0; i < n; i++) {   // Frame::ComputeStereoFromRGBD
            const float u = kps[(size_t)i].x, v = kps[(size_t)i].y;
            const float d = depth_img[((size_t)f * kH + (int)v) * kPitchFloats + (int)u];
            float wd = -1.f, wur = -1.f;
            if (d > 0) { wd = d; wur = kun[(size_t)i].x - bf / d; want_with++; }
            moved += kun[(size_t)i].x != u;
            CHECK(memcmp(&wd, &dep[(size_t)i], 4) == 0 && memcmp(&wur, &ur[(size_t)i], 4) == 0);
        }
        CHECK(n_with == want_with && want_with > 20 && want_with < n && moved > 50);
        // handle A: from the batch, its count pending; handle B: from the downloaded arrays
        MUST(orbx_frame_load_stereo_batch(A, ex, f, nullptr, nullptr, 0));
        std::vector<float> xy(2 * (size_t)n);
        for (int i = 0; i < n; i++) { xy[2 * (size_t)i] = kps[(size_t)i].x; xy[2 * (size_t)i + 1] = kps[(size_t)i].y; }
        float sf[8], b4[4];
        for (int l = 0; l < 8; l++) sf[l] = l ? sf[l - 1] * 1.2f : 1.f;
        MUST(orbx_image_bounds(&cam, kW, kH, b4));
        orbx_frame_desc d;
        memset(&d, 0, sizeof(d));
        d.keypoints_un = kun.data(); d.descriptors = desc.data(); d.n = n; d.min_x = b4[0]; d.max_x = b4[1]; d.min_y = b4[2]; d.max_y = b4[3];
        d.scale_factors = sf; d.nlevels = 8; d.u_right = ur.data();
        CHECK(orbx_frame_load_host_stereo(B, &d, nullptr, xy.data()) == ORBX_E_BAD_ARG);
        MUST(orbx_frame_load_host_stereo(B, &d, dep.data(), xy.data()));
        for (orbx_frame *F : {A, B}) {
            std::unique_ptr<float[]> our(new float[(size_t)n]), odep(new float[(size_t)n]), pos(new float[3 * (size_t)n]);   // exactly N rows
            std::fill(pos.get(), pos.get() + 3 * (size_t)n, kSentinel);
            int with = -1;
            MUST(orbx_frame_unproject_stereo(m, F, &V, our.get(), odep.get(), pos.get(), &with));
            CHECK(with == want_with);
            CHECK(memcmp(our.get(), ur.data(), 4 * (size_t)n) == 0 && memcmp(odep.get(), dep.data(), 4 * (size_t)n) == 0);
            for (int i = 0; i < n; i++) {
                float X[3] = {kSentinel, kSentinel, kSentinel};
                if (dep[(size_t)i] > 0) unproject(V, kun[(size_t)i].x, kun[(size_t)i].y, dep[(size_t)i], X);   // the frame's member reads mvKeysUn
                CHECK(memcmp(X, pos.get() + 3 * (size_t)i, 12) == 0);
            }
            int count = -1;
            MUST(orbx_frame_count(F, &count));
            CHECK(count == n);
        }
        MUST(orbx_frame_load_batch(A, ex, f, nullptr, nullptr, 0));                           // a plain load: no depth on the handle
        CHECK(orbx_frame_unproject_stereo(m, A, &V, nullptr, nullptr, nullptr, nullptr) == ORBX_E_BAD_ARG);
    }
    orbx_frame_destroy(A); orbx_frame_destroy(B);
    orbx_matcher_destroy(m);
    orbx_destroy(ex);
    printf("rgbd stage, loads and UnprojectStereo: equal to the members on %d frames\n", kFrames);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// part 2: the stereo branches of CreateNewMapPoints
// ---------------------------------------------------------------------------------------------------------
// Eigen::JacobiSVD<Matrix4f>(A, ComputeFullV).matrixV().col(3): the two-sided Jacobi iteration of Eigen 3.3 / 3.4, restated (PARITY UNPINNED)
void jacobi_svd4_v3(const float A[4][4], float *out) {
    const float fmin_ = 1.17549435e-38f, eps2 = 2.f * 1.1920929e-07f;
    float W[4][4], V[4][4], scale = 0.f;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) scale = fmaxf(scale, fabsf(A[i][j]));
    if (scale == 0.f) scale = 1.f;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) { W[i][j] = A[i][j] / scale; V[i][j] = i == j ? 1.f : 0.f; }
    float maxDiag = 0.f;
    for (int i = 0; i < 4; i++) maxDiag = fmaxf(maxDiag, fabsf(W[i][i]));
    bool finished = false;
    for (int sweep = 0; !finished && sweep < 64; sweep++) {
        finished = true;
        for (int p = 1; p < 4; p++)
            for (int q = 0; q < p; q++) {
                const float threshold = fmaxf(fmin_, eps2 * maxDiag);
                if (!(fabsf(W[p][q]) > threshold || fabsf(W[q][p]) > threshold)) continue;
                finished = false;
                const float m00 = W[p][p], m01 = W[p][q], m10 = W[q][p], m11 = W[q][q];
                const float t = m00 + m11, d = m10 - m01;
                float c1, s1;
                if (fabsf(d) < fmin_) { s1 = 0.f; c1 = 1.f; }
                else { const float u = t / d, tmp = sqrtf(1.f + u * u); s1 = 1.f / tmp; c1 = u / tmp; }
                const float n00 = c1 * m00 + s1 * m10, n01 = c1 * m01 + s1 * m11, n11 = -s1 * m01 + c1 * m11;
                float cr, sr;
                const float deno = 2.f * fabsf(n01);
                if (deno < fmin_) { cr = 1.f; sr = 0.f; }
                else {
                    const float tau = (n00 - n11) / deno, w = sqrtf(tau * tau + 1.f);
                    const float tt = tau > 0.f ? 1.f / (tau + w) : 1.f / (tau - w);
                    const float sign_t = tt > 0.f ? 1.f : -1.f, n = 1.f / sqrtf(tt * tt + 1.f);
                    sr = -sign_t * (n01 / fabsf(n01)) * fabsf(tt) * n;
                    cr = n;
                }
                const float cl = c1 * cr - s1 * (-sr), sl = c1 * (-sr) + s1 * cr;
                if (!(cl == 1.f && sl == 0.f))
                    for (int i = 0; i < 4; i++) { const float xp = W[p][i], xq = W[q][i]; W[p][i] = cl * xp + sl * xq; W[q][i] = -sl * xp + cl * xq; }
                if (!(cr == 1.f && sr == 0.f))
                    for (int i = 0; i < 4; i++) {
                        const float xp = W[i][p], xq = W[i][q]; W[i][p] = cr * xp + (-sr) * xq; W[i][q] = sr * xp + cr * xq;
                        const float vp = V[i][p], vq = V[i][q]; V[i][p] = cr * vp + (-sr) * vq; V[i][q] = sr * vp + cr * vq;
                    }
                maxDiag = fmaxf(maxDiag, fmaxf(fabsf(W[p][p]), fabsf(W[q][q])));
            }
    }
    float sv[4];
    for (int i = 0; i < 4; i++) sv[i] = fabsf(W[i][i]);
    for (int i = 0; i < 3; i++) {   // descending, first maximum, the columns of V swapped along
        int pos = i;
        for (int j = i + 1; j < 4; j++) if (sv[j] > sv[pos]) pos = j;
        if (sv[pos] == 0.f) break;
        if (pos != i) {
            std::swap(sv[i], sv[pos]);
            for (int r = 0; r < 4; r++) std::swap(V[r][i], V[r][pos]);
        }
    }
    for (int i = 0; i < 4; i++) out[i] = V[i][3];
}

struct Side {
    int n, nlevels;
    float scale[8], sigma2[8];
    std::vector<orbx_keypoint> kps;        // mvKeysUn
    std::vector<float> u_right, depth, xy; // mvuRight, mvDepth, mvKeys[i].pt
    std::vector<uint8_t> desc;
    orbx_new_points_view view;
    float mb, mbf;
};
struct Scene {
    Side kf[2];
    orbx_new_points_params par;
    orbx_new_points_stereo st;
    std::vector<int32_t> idx1, idx2;
};
int g_path[4];   // pairs the member decided without a stereo observation, by triangulation, by unprojection from key frame 1 / 2

void camera_point(const orbx_new_points_view &V, const float *P, float *c) {
    for (int r = 0; r < 3; r++) c[r] = dot3(V.Rcw[3 * r], V.Rcw[3 * r + 1], V.Rcw[3 * r + 2], P[0], P[1], P[2]) + V.tcw[r];
}

void make_scene(Scene &S) {
    std::mt19937 rng(47);
    auto uni = [&](float a, float b) { return a + (b - a) * (float)(rng() % 100000) / 100000.f; };
    const int shape[2] = {300, 340}, levels[2] = {8, 5};
    const float factor[2] = {1.2f, 1.1f};
    const double R[2][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0.9995, 0.01, -0.03, -0.0097, 0.9999, 0.01, 0.0301, -0.0097, 0.9995}};
    const double O[2][3] = {{0, 0, 0}, {0.4, 0.1, 0.8}};
    for (int k = 0; k < 2; k++) {
        Side &K = S.kf[k];
        K.n = shape[k]; K.nlevels = levels[k]; K.mb = 0.11f; K.mbf = 0.11f * 500.f;
        for (int l = 0; l < 8; l++) { K.scale[l] = l ? K.scale[l - 1] * factor[k] : 1.f; K.sigma2[l] = K.scale[l] * K.scale[l]; }
        for (int i = 0; i < 9; i++) K.view.Rcw[i] = (float)R[k][i];
        for (int r = 0; r < 3; r++) {
            K.view.tcw[r] = (float)-(R[k][3 * r] * O[k][0] + R[k][3 * r + 1] * O[k][1] + R[k][3 * r + 2] * O[k][2]);
            K.view.Ow[r] = (float)O[k][r];
        }
        K.view.fx = 500.f; K.view.fy = 498.f; K.view.cx = 322.5f; K.view.cy = 238.25f;
        K.kps.resize((size_t)K.n); K.desc.resize(32 * (size_t)K.n);
        for (uint8_t &b : K.desc) b = (uint8_t)rng();
        for (orbx_keypoint &kp : K.kps) {
            memset(&kp, 0, sizeof(kp));
            kp.x = uni(20.f, 620.f); kp.y = uni(20.f, 460.f); kp.octave = (int)(rng() % (unsigned)K.nlevels); kp.size = 31.f; kp.class_id = -1;
            kp.angle = uni(0.f, 359.f);
        }
        K.u_right.assign((size_t)K.n, -1.f); K.depth.assign((size_t)K.n, -1.f);
    }
    S.par.ratio_factor = 1.5f * 1.2f; S.par.inertial = 0; S.par.far_points = 1; S.par.th_far_points = 7.5f;
    S.par.nlevels_1 = levels[0]; S.par.nlevels_2 = levels[1]; S.par.level_sigma2_1 = S.kf[0].sigma2; S.par.level_sigma2_2 = S.kf[1].sigma2;
    S.st.mb1 = S.kf[0].mb; S.st.mbf1 = S.kf[0].mbf; S.st.mb2 = S.kf[1].mb; S.st.mbf2 = S.kf[1].mbf;
    const float axis[3] = {0.4f / 0.9f, 0.1f / 0.9f, 0.8f / 0.9f};
    const int n_designed = S.kf[0].n - 20;
    for (int i = 0; i < n_designed; i++) {
        const int j = S.kf[1].n - 1 - i, kind = i % 16;
        float z = uni(3.f, 7.f);
        if (kind == 9) z = uni(8.5f, 12.f);                  // beyond mThFarPoints
        if (kind == 10 || kind == 5) z = uni(150.f, 400.f);  // no parallax
        float P[3] = {0.2f + uni(-0.45f, 0.45f) * z, 0.05f + uni(-0.35f, 0.35f) * z, 0.4f + z};
        if (kind == 11) { P[0] = uni(-1.f, 1.f); P[1] = uni(-0.7f, 0.7f); P[2] = -uni(2.5f, 5.f); }                  // behind both
        if (kind == 12) { P[0] = 0.2f + uni(-0.1f, 0.1f); P[1] = 0.05f + uni(-0.1f, 0.1f); P[2] = 0.4f; }            // between the centres
        if (kind == 4 || kind == 6 || kind == 2) {           // beyond key frame 2 on the line through both centres: low ray parallax
            const float s = uni(3.f, 6.f);
            for (int a = 0; a < 3; a++) P[a] = (float)O[1][a] + s * axis[a] + uni(-0.04f, 0.04f);
        }
        const int idx[2] = {i, j};
        for (int k = 0; k < 2; k++) {
            Side &K = S.kf[k];
            orbx_keypoint &kp = K.kps[(size_t)idx[k]];
            float c[3];
            camera_point(K.view, P, c);
            const float depth = c[2];
            if (c[2] < 0.f) { c[0] = -c[0]; c[1] = -c[1]; c[2] = -c[2]; }
            kp.x = K.view.fx * c[0] / c[2] + K.view.cx; kp.y = K.view.fy * c[1] / c[2] + K.view.cy;
            const float noise = (kind == 13 && k == 0) || (kind == 14 && k == 1) ? 7.f : 0.3f;
            kp.x += uni(-noise, noise); kp.y += uni(-noise, noise);
            kp.octave = kind == 15 ? (k == 0 ? K.nlevels - 1 : 0) : (int)(rng() % 3u);
            if (kind == 14 && k == 0) kp.octave = K.nlevels - 1;
            // a stereo observation: kinds 1, 3, 4, 13, 15 on key frame 1; 2, 8 on key frame 2; 6, 9 on both; 5 on key frame 1 without a depth
            const bool on = k == 0 ? (kind == 1 || kind == 3 || kind == 4 || kind == 13 || kind == 15 || kind == 6 || kind == 9 || kind == 5)
                                   : (kind == 2 || kind == 8 || kind == 6 || kind == 9);
            if (on && depth > 0.f) {
                K.depth[(size_t)idx[k]] = kind == 5 ? (i % 32 < 16 ? 0.f : -2.f) : depth * (1.f + uni(-0.002f, 0.002f));
                K.u_right[(size_t)idx[k]] = kp.x - K.mbf / depth + (kind == 3 ? 2.6f * K.scale[kp.octave] : uni(-0.3f, 0.3f));
            }
        }
        for (int b = 0; b < 32; b++) S.kf[1].desc[32 * (size_t)j + b] = S.kf[0].desc[32 * (size_t)i + b];
        for (int f = 0; f < 6; f++) { const unsigned bit = rng() % 256; S.kf[1].desc[32 * (size_t)j + bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
        S.idx1.push_back(i); S.idx2.push_back(kind == 7 ? -1 : j);
    }
    for (int k = 0; k < 2; k++) {   // the raw key points: the undistorted ones, moved on every second feature
        Side &K = S.kf[k];
        K.xy.resize(2 * (size_t)K.n);
        for (int i = 0; i < K.n; i++) {
            K.xy[2 * (size_t)i] = K.kps[(size_t)i].x + (i % 2 ? uni(-1.2f, 1.2f) : 0.f);
            K.xy[2 * (size_t)i + 1] = K.kps[(size_t)i].y + (i % 2 ? uni(-1.2f, 1.2f) : 0.f);
        }
    }
}

// the member's loop body for one pair with its stereo branches (include/orbx.h); with_depth[k]: key frame k holds mvDepth
int member(const Scene &S, const bool *with_depth, int i1, int i2, float *x3D) {
    if (i2 < 0) return ORBX_NEWPT_NO_MATCH;
    const Side &K1 = S.kf[0], &K2 = S.kf[1];
    const orbx_keypoint &kp1 = K1.kps[(size_t)i1], &kp2 = K2.kps[(size_t)i2];
    const bool bStereo1 = K1.u_right[(size_t)i1] >= 0, bStereo2 = K2.u_right[(size_t)i2] >= 0;
    if ((bStereo1 && !with_depth[0]) || (bStereo2 && !with_depth[1])) return ORBX_NEWPT_STEREO_LEFT_TO_HOST;
    const orbx_new_points_view &V1 = K1.view, &V2 = K2.view;
    const float *R1 = V1.Rcw, *R2 = V2.Rcw, *t1 = V1.tcw, *t2 = V2.tcw;
    const float xn1[3] = {(kp1.x - V1.cx) / V1.fx, (kp1.y - V1.cy) / V1.fy, 1.f}, xn2[3] = {(kp2.x - V2.cx) / V2.fx, (kp2.y - V2.cy) / V2.fy, 1.f};
    float ray1[3], ray2[3];
    for (int r = 0; r < 3; r++) {   // Rwc = Rcw.transpose()
        ray1[r] = dot3(R1[r], R1[3 + r], R1[6 + r], xn1[0], xn1[1], xn1[2]);
        ray2[r] = dot3(R2[r], R2[3 + r], R2[6 + r], xn2[0], xn2[1], xn2[2]);
    }
    const float n1 = sqrtf(dot3(ray1[0], ray1[1], ray1[2], ray1[0], ray1[1], ray1[2])), n2 = sqrtf(dot3(ray2[0], ray2[1], ray2[2], ray2[0], ray2[1], ray2[2]));
    const float cosParallaxRays = dot3(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]) / (n1 * n2);
    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
    if (bStereo1) cosParallaxStereo1 = cosf(2 * atan2f(K1.mb / 2, K1.depth[(size_t)i1]));
    else if (bStereo2) cosParallaxStereo2 = cosf(2 * atan2f(K2.mb / 2, K2.depth[(size_t)i2]));
    cosParallaxStereo = std::min(cosParallaxStereo1, cosParallaxStereo2);
    float X[3];
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || cosParallaxRays < (S.par.inertial ? 0.9996 : 0.9998))) {
        float A[4][4];
        for (int j = 0; j < 4; j++) {
            const float a[3] = {j < 3 ? R1[j] : t1[0], j < 3 ? R1[3 + j] : t1[1], j < 3 ? R1[6 + j] : t1[2]};
            const float b[3] = {j < 3 ? R2[j] : t2[0], j < 3 ? R2[3 + j] : t2[1], j < 3 ? R2[6 + j] : t2[2]};
            A[0][j] = xn1[0] * a[2] - a[0]; A[1][j] = xn1[1] * a[2] - a[1];
            A[2][j] = xn2[0] * b[2] - b[0]; A[3][j] = xn2[1] * b[2] - b[1];
        }
        float xh[4];
        jacobi_svd4_v3(A, xh);
        if (xh[3] == 0) return ORBX_NEWPT_TRIANGULATE_FAILED;
        for (int a = 0; a < 3; a++) X[a] = xh[a] / xh[3];
        g_path[bStereo1 || bStereo2 ? 1 : 0]++;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        g_path[2]++;
        const float z = K1.depth[(size_t)i1];
        if (!(z > 0)) return ORBX_NEWPT_UNPROJECT_FAILED;
        unproject(V1, K1.xy[2 * (size_t)i1], K1.xy[2 * (size_t)i1 + 1], z, X);   // the RAW key point
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        g_path[3]++;
        const float z = K2.depth[(size_t)i2];
        if (!(z > 0)) return ORBX_NEWPT_UNPROJECT_FAILED;
        unproject(V2, K2.xy[2 * (size_t)i2], K2.xy[2 * (size_t)i2 + 1], z, X);
    } else {
        return ORBX_NEWPT_LOW_PARALLAX;
    }
    const float z1 = dot3(R1[6], R1[7], R1[8], X[0], X[1], X[2]) + t1[2];
    if (z1 <= 0) return ORBX_NEWPT_BEHIND_1;
    const float z2 = dot3(R2[6], R2[7], R2[8], X[0], X[1], X[2]) + t2[2];
    if (z2 <= 0) return ORBX_NEWPT_BEHIND_2;
    const float x1 = dot3(R1[0], R1[1], R1[2], X[0], X[1], X[2]) + t1[0], y1 = dot3(R1[3], R1[4], R1[5], X[0], X[1], X[2]) + t1[1];
    if (!bStereo1) {
        const float u = V1.fx * x1 / z1 + V1.cx, v = V1.fy * y1 / z1 + V1.cy;
        const float errX1 = u - kp1.x, errY1 = v - kp1.y;
        if ((errX1 * errX1 + errY1 * errY1) > 5.991 * K1.sigma2[kp1.octave]) return ORBX_NEWPT_REPROJ_1;
    } else {
        const float invz1 = (float)(1.0 / z1);
        const float u1 = V1.fx * x1 * invz1 + V1.cx, u1_r = u1 - K1.mbf * invz1, v1 = V1.fy * y1 * invz1 + V1.cy;
        const float errX1 = u1 - kp1.x, errY1 = v1 - kp1.y, errX1_r = u1_r - K1.u_right[(size_t)i1];
        if ((errX1 * errX1 + errY1 * errY1 + errX1_r * errX1_r) > 7.8 * K1.sigma2[kp1.octave]) return ORBX_NEWPT_REPROJ_1;
    }
    const float x2 = dot3(R2[0], R2[1], R2[2], X[0], X[1], X[2]) + t2[0], y2 = dot3(R2[3], R2[4], R2[5], X[0], X[1], X[2]) + t2[1];
    if (!bStereo2) {
        const float u = V2.fx * x2 / z2 + V2.cx, v = V2.fy * y2 / z2 + V2.cy;
        const float errX2 = u - kp2.x, errY2 = v - kp2.y;
        if ((errX2 * errX2 + errY2 * errY2) > 5.991 * K2.sigma2[kp2.octave]) return ORBX_NEWPT_REPROJ_2;
    } else {
        const float invz2 = (float)(1.0 / z2);
        const float u2 = V2.fx * x2 * invz2 + V2.cx, u2_r = u2 - K2.mbf * invz2, v2 = V2.fy * y2 * invz2 + V2.cy;
        const float errX2 = u2 - kp2.x, errY2 = v2 - kp2.y, errX2_r = u2_r - K2.u_right[(size_t)i2];
        if ((errX2 * errX2 + errY2 * errY2 + errX2_r * errX2_r) > 7.8 * K2.sigma2[kp2.octave]) return ORBX_NEWPT_REPROJ_2;
    }
    const float a0 = X[0] - V1.Ow[0], a1 = X[1] - V1.Ow[1], a2 = X[2] - V1.Ow[2], b0 = X[0] - V2.Ow[0], b1 = X[1] - V2.Ow[1], b2 = X[2] - V2.Ow[2];
    const float dist1 = sqrtf(dot3(a0, a1, a2, a0, a1, a2)), dist2 = sqrtf(dot3(b0, b1, b2, b0, b1, b2));
    if (dist1 == 0 || dist2 == 0) return ORBX_NEWPT_ZERO_DIST;
    if (S.par.far_points && (dist1 >= S.par.th_far_points || dist2 >= S.par.th_far_points)) return ORBX_NEWPT_FAR;
    const float ratioDist = dist2 / dist1, ratioOctave = K1.scale[kp1.octave] / K2.scale[kp2.octave], ratioFactor = S.par.ratio_factor;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return ORBX_NEWPT_SCALE_RATIO;
    x3D[0] = X[0]; x3D[1] = X[1]; x3D[2] = X[2];
    return ORBX_NEWPT_OK;
}

int make_key_frame(orbx_matcher *m, const Side &K, bool with_depth, orbx_keyframe **out) {
    orbx_frame_desc d;
    memset(&d, 0, sizeof(d));
    d.keypoints_un = K.kps.data(); d.descriptors = K.desc.data(); d.n = K.n;
    d.min_x = 0.f; d.max_x = 640.f; d.min_y = 0.f; d.max_y = 480.f;
    d.scale_factors = K.scale; d.nlevels = K.nlevels; d.u_right = K.u_right.data();
    if (with_depth) MUST(orbx_keyframe_create_host_stereo(m, &d, K.depth.data(), K.xy.data(), nullptr, out));
    else MUST(orbx_keyframe_create_host(m, &d, nullptr, out));
    return 0;
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

int compare(const Scene &S, const bool *with_depth, int n, const int32_t *i1, const int32_t *i2, const float *pos, const uint8_t *st, int acc, int *hist) {
    int bad = 0, accepted = 0;
    for (int p = 0; p < n; p++) {
        float X[3] = {kSentinel, kSentinel, kSentinel};
        const int want = member(S, with_depth, i1[p], i2[p], X);
        hist[want]++;
        accepted += want == ORBX_NEWPT_OK;
        if (st[p] != want || memcmp(pos + 3 * (size_t)p, X, 12) != 0) {
            if (bad++ < 10) printf("pair %d (%d, %d): status %d want %d, pos %a %a %a want %a %a %a\n", p, i1[p], i2[p], st[p], want, pos[3 * p], pos[3 * p + 1],
                                   pos[3 * p + 2], X[0], X[1], X[2]);
        }
    }
    if (acc != accepted) { printf("n_accepted %d, want %d\n", acc, accepted); bad++; }
    return bad;
}

int key_frames_part() {
    Scene S;
    make_scene(S);
    orbx_matcher *m = nullptr;
    MUST(orbx_matcher_create(0, &m));
    const bool both[2] = {true, true}, first_only[2] = {true, false};
    orbx_keyframe *kfs[2] = {nullptr, nullptr}, *plain2 = nullptr;
    if (make_key_frame(m, S.kf[0], true, &kfs[0]) || make_key_frame(m, S.kf[1], true, &kfs[1]) || make_key_frame(m, S.kf[1], false, &plain2)) return 1;
    const int sizes[] = {1, 63, 64, 65, (int)S.idx1.size()};
    int hist[13] = {0};
    for (int n : sizes) {   // heap blocks of exactly the needed size
        std::unique_ptr<int32_t[]> i1(new int32_t[(size_t)n]), i2(new int32_t[(size_t)n]);
        std::unique_ptr<float[]> pos(new float[3 * (size_t)n]);
        std::unique_ptr<uint8_t[]> st(new uint8_t[(size_t)n]);
        const size_t from = S.idx1.size() - (size_t)n;
        memcpy(i1.get(), S.idx1.data() + from, 4 * (size_t)n); memcpy(i2.get(), S.idx2.data() + from, 4 * (size_t)n);
        std::fill(pos.get(), pos.get() + 3 * (size_t)n, kSentinel); std::fill(st.get(), st.get() + n, kStatusSentinel);
        int acc = -1;
        MUST(orbx_keyframe_triangulate_pairs_stereo(m, kfs[0], kfs[1], &S.kf[0].view, &S.kf[1].view, &S.par, &S.st, n, i1.get(), i2.get(), pos.get(), st.get(),
                                                    &acc));
        int h[13] = {0};
        const bool all = n == (int)S.idx1.size();
        if (all) memset(g_path, 0, sizeof(g_path));
        CHECK(compare(S, both, n, i1.get(), i2.get(), pos.get(), st.get(), acc, all ? hist : h) == 0);
        int64_t t[6];
        orbx_matcher_debug_transfers(m, t, 6);
        CHECK(t[0] == 1 && t[1] == 1 && t[4] == 0 && t[5] == 2);
    }
    printf("stereo pairs: status counts");
    for (int s = 0; s < 13; s++) printf(" %d", hist[s]);
    printf("; without a stereo observation %d, triangulated %d, unprojected from key frame 1 / 2: %d / %d\n", g_path[0], g_path[1], g_path[2], g_path[3]);
    CHECK(hist[ORBX_NEWPT_OK] >= 60 && hist[ORBX_NEWPT_UNPROJECT_FAILED] >= 5 && hist[ORBX_NEWPT_STEREO_LEFT_TO_HOST] == 0 && hist[ORBX_NEWPT_REPROJ_1] >= 3);
    CHECK(g_path[0] >= 40 && g_path[1] >= 20 && g_path[2] >= 10 && g_path[3] >= 5);
    {   // key frame 2 without depth: its stereo observations stay with the host
        const int n = (int)S.idx1.size();
        std::unique_ptr<float[]> pos(new float[3 * (size_t)n]);
        std::unique_ptr<uint8_t[]> st(new uint8_t[(size_t)n]);
        std::fill(pos.get(), pos.get() + 3 * (size_t)n, kSentinel); std::fill(st.get(), st.get() + n, kStatusSentinel);
        int acc = -1, h[13] = {0};
        MUST(orbx_keyframe_triangulate_pairs_stereo(m, kfs[0], plain2, &S.kf[0].view, &S.kf[1].view, &S.par, &S.st, n, S.idx1.data(), S.idx2.data(), pos.get(),
                                                    st.get(), &acc));
        CHECK(compare(S, first_only, n, S.idx1.data(), S.idx2.data(), pos.get(), st.get(), acc, h) == 0 && h[ORBX_NEWPT_STEREO_LEFT_TO_HOST] >= 10);
    }
    {   // refusals: nothing enqueued, nothing written
        int64_t before[6], after[6];
        orbx_matcher_debug_transfers(m, before, 6);
        float pos[3] = {kSentinel, kSentinel, kSentinel};
        uint8_t st = kStatusSentinel;
        int acc = -7;
        const int32_t ok1 = 0, ok2 = 0, high1 = S.kf[0].n;
        CHECK(orbx_keyframe_triangulate_pairs_stereo(m, kfs[0], kfs[1], &S.kf[0].view, &S.kf[1].view, &S.par, nullptr, 1, &ok1, &ok2, pos, &st, &acc) == ORBX_E_BAD_ARG);
        CHECK(orbx_keyframe_triangulate_pairs_stereo(m, kfs[0], kfs[1], &S.kf[0].view, &S.kf[1].view, &S.par, &S.st, 1, &high1, &ok2, pos, &st, &acc) == ORBX_E_BAD_ARG);
        CHECK(orbx_keyframe_triangulate_pairs_stereo(m, kfs[0], kfs[1], &S.kf[0].view, &S.kf[1].view, &S.par, &S.st, 1, &ok1, &ok2, nullptr, &st, &acc) == ORBX_E_BAD_ARG);
        CHECK(pos[0] == kSentinel && st == kStatusSentinel && acc == -7);
        CHECK(orbx_keyframe_triangulate_pairs_stereo(m, kfs[0], kfs[1], &S.kf[0].view, &S.kf[1].view, &S.par, &S.st, 0, nullptr, nullptr, nullptr, nullptr, &acc) == ORBX_OK && acc == 0);
        orbx_matcher_debug_transfers(m, after, 6);
        CHECK(memcmp(before, after, sizeof(before)) == 0);
    }
    // the fused form: BoW on both key frames, the search alone, then the search with the stereo triangulation behind it
    orbx_vocabulary *voc = nullptr;
    if (make_vocabulary(&voc)) return 1;
    for (int k = 0; k < 2; k++) MUST(orbx_keyframe_compute_bow(m, kfs[k], voc, 1, nullptr, nullptr));
    const int n1 = S.kf[0].n;
    std::vector<uint8_t> skip1((size_t)n1, 0);
    for (int i = 0; i < n1; i += 7) skip1[(size_t)i] = 1;
    orbx_keyframe_gate g;
    memset(&g, 0, sizeof(g));
    g.coarse = 1; g.strict_fp = 1; g.ep_x = g.ep_y = 1e6f; g.nlevels = S.kf[1].nlevels; g.level_sigma2_2 = S.kf[1].sigma2;
    for (int pass = 0; pass < 2; pass++) {
        const uint8_t *s1 = pass ? skip1.data() : nullptr;
        std::unique_ptr<int32_t[]> plain(new int32_t[(size_t)n1]), m12(new int32_t[(size_t)n1]), own(new int32_t[(size_t)n1]);
        std::unique_ptr<float[]> pos(new float[3 * (size_t)n1]);
        std::unique_ptr<uint8_t[]> st(new uint8_t[(size_t)n1]);
        std::fill(pos.get(), pos.get() + 3 * (size_t)n1, kSentinel); std::fill(st.get(), st.get() + n1, kStatusSentinel);
        const int nm = orbx_keyframe_search_for_triangulation(m, kfs[0], kfs[1], s1, nullptr, 1, &g, plain.get());
        MUST(nm);
        int64_t ts[6], tf[6];
        orbx_matcher_debug_transfers(m, ts, 6);
        int acc = -1;
        const int nf = orbx_keyframe_search_and_triangulate_stereo(m, kfs[0], kfs[1], s1, nullptr, 1, &g, &S.kf[0].view, &S.kf[1].view, &S.par, &S.st, m12.get(),
                                                                   pos.get(), st.get(), &acc);
        MUST(nf);
        orbx_matcher_debug_transfers(m, tf, 6);
        CHECK(nf == nm && memcmp(plain.get(), m12.get(), 4 * (size_t)n1) == 0 && nm >= 40);
        for (int i = 0; i < n1; i++) own[(size_t)i] = i;
        int h[13] = {0};
        CHECK(compare(S, both, n1, own.get(), m12.get(), pos.get(), st.get(), acc, h) == 0);
        CHECK(h[ORBX_NEWPT_OK] >= 20 && h[ORBX_NEWPT_NO_MATCH] >= 20 && h[ORBX_NEWPT_STEREO_LEFT_TO_HOST] == 0);
        CHECK(tf[0] == 1 && tf[1] == 1 && ts[0] == 1 && ts[1] == 1 && tf[5] == ts[5] && tf[4] == 0);     // one run each way, no launch of a transfer more
        printf("fused stereo (%s skip flags): %d matches, %d accepted, upload %lld -> %lld bytes, download %lld -> %lld bytes\n", pass ? "with" : "no", nm, acc,
               (long long)ts[2], (long long)tf[2], (long long)ts[3], (long long)tf[3]);
    }
    orbx_keyframe_destroy(kfs[0]); orbx_keyframe_destroy(kfs[1]); orbx_keyframe_destroy(plain2);
    orbx_vocabulary_destroy(voc);
    orbx_matcher_destroy(m);
    return 0;
}

}  // namespace

int main() {
    if (frames_part() || key_frames_part()) return 1;
    printf("stereo resident ok\n");
    return 0;
}
