// LocalMapping::CreateNewMapPoints' triangulation on resident key frames -- orbx_keyframe_triangulate_pairs[_fisheye] (pairs the host names) and
// orbx_keyframe_search_and_triangulate[_fisheye] (behind SearchForTriangulation, on the row it leaves on the device) -- for a monocular pair of key
// frames (N = 300 / 340, pyramids 8 x 1.2 / 5 x 1.1) and a fisheye-stereo pair (170 + 130 / 180 + 160 features, KannalaBrandt8).  status must equal the
// member's loop written out below (with the host's libm and Eigen's two-sided Jacobi iteration restated: PARITY UNPINNED, as include/orbx.h says) and
// pos equal it bit for bit where a pair is accepted; the rows of rejected pairs keep the sentinel; the fused call's row equals the search's.  The
// caller's arrays are heap blocks of exactly the needed size; refused calls and an empty one leave the transfer counters alone.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt) and
// compiled with -fsanitize=address,undefined, as tests/cpp/normal_depth_check.cpp.  Prints "new points ok" and returns 0.  With an argument N it also
// times N runs of the reference loop over the rig's pairs on the host and prints the mean ("host reference loop": the C++ cost of the member's loop
// body on contiguous arrays, nothing else).
#pragma clang fp contract(off)   // one rounding per operation, as the device code is built
#include <algorithm>
#include <chrono>
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

// ---- the camera models and the SVD, as the reference's translation units evaluate them ----
void kb8_project(const float *p, float X, float Y, float Z, float *u, float *v) {   // KannalaBrandt8.cpp:67-85 (cos / sin of the double overloads)
    const float x2_plus_y2 = X * X + Y * Y;
    const float theta = atan2f(sqrtf(x2_plus_y2), Z);
    const float psi = atan2f(Y, X);
    const float theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
    const float r = theta + p[4] * theta3 + p[5] * theta5 + p[6] * theta7 + p[7] * theta9;
    *u = (float)((double)(p[0] * r) * cos((double)psi) + (double)p[2]);
    *v = (float)((double)(p[1] * r) * sin((double)psi) + (double)p[3]);
}
void kb8_unproject(const float *p, float px, float py, float *rx, float *ry) {   // KannalaBrandt8.cpp:107-142, precision 1e-6
    const float pwx = (px - p[2]) / p[0], pwy = (py - p[3]) / p[1];
    float scale = 1.f;
    float theta_d = sqrtf(pwx * pwx + pwy * pwy);
    theta_d = fminf(fmaxf((float)(-3.1415926535897932384626433832795 / 2.f), theta_d), (float)(3.1415926535897932384626433832795 / 2.f));
    if ((double)theta_d > 1e-8) {
        float theta = theta_d;
        for (int j = 0; j < 10; j++) {
            const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
            const float k0_theta2 = p[4] * theta2, k1_theta4 = p[5] * theta4, k2_theta6 = p[6] * theta6, k3_theta8 = p[7] * theta8;
            const float theta_fix = (theta * (1 + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                                    (1 + 3 * k0_theta2 + 5 * k1_theta4 + 7 * k2_theta6 + 9 * k3_theta8);
            theta = theta - theta_fix;
            if (fabsf(theta_fix) < 1e-6f) break;
        }
        scale = tanf(theta) / theta_d;
    }
    *rx = pwx * scale; *ry = pwy * scale;
}
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
inline float dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return ((0.f + a0 * b0) + a1 * b1) + a2 * b2; }

// ---- a pair of key frames of one kind ----
struct Side {
    int n_left, n_right;                  // n_right < 0: monocular
    int nlevels;
    float scale[8], sigma2[8];
    std::vector<orbx_keypoint> kps;       // reference numbering: left, then right
    std::vector<float> u_right;           // monocular only
    std::vector<uint8_t> desc;
    orbx_fisheye_view view[2];            // R, t, twc, params (Pinhole: fx, fy, cx, cy in params[0..3])
    int n() const { return n_left + std::max(n_right, 0); }
};
struct Scene {
    bool rig;
    Side kf[2];
    orbx_new_points_params par;
    std::vector<int32_t> idx1, idx2;
};

const float kPinhole[8] = {500.f, 498.f, 322.5f, 238.25f, 0, 0, 0, 0};
const float kKb8[2][8] = {{190.97848f, 190.97331f, 254.93171f, 256.89744f, 0.0034823894f, 0.00071503485f, -0.0020532361f, 0.00020293674f},
                          {190.44237f, 190.43444f, 252.5995f, 254.91723f, 0.003400317f, 0.0017662782f, -0.0026631257f, 0.00032995174f}};

void set_view(orbx_fisheye_view &V, const double R[9], const double O[3], const float *p) {
    for (int i = 0; i < 9; i++) V.R[i] = (float)R[i];
    for (int r = 0; r < 3; r++) { V.t[r] = (float)-(R[3 * r] * O[0] + R[3 * r + 1] * O[1] + R[3 * r + 2] * O[2]); V.twc[r] = (float)O[r]; }
    memcpy(V.params, p, sizeof(V.params));
}
void project(bool rig, const orbx_fisheye_view &V, const float *P, float *u, float *v) {   // the key point where the line from the centre to P meets the image
    float c[3];
    for (int r = 0; r < 3; r++) c[r] = dot3(V.R[3 * r], V.R[3 * r + 1], V.R[3 * r + 2], P[0], P[1], P[2]) + V.t[r];
    if (c[2] < 0.f) { c[0] = -c[0]; c[1] = -c[1]; c[2] = -c[2]; }
    if (rig) kb8_project(V.params, c[0], c[1], c[2], u, v);
    else { *u = V.params[0] * c[0] / c[2] + V.params[2]; *v = V.params[1] * c[1] / c[2] + V.params[3]; }
}

void make_scene(Scene &S, bool rig) {
    std::mt19937 rng(rig ? 41 : 43);
    auto uni = [&](float a, float b) { return a + (b - a) * (float)(rng() % 100000) / 100000.f; };
    S.rig = rig;
    const int shape[2][2] = {{rig ? 170 : 300, rig ? 130 : -1}, {rig ? 180 : 340, rig ? 160 : -1}};
    const int levels[2] = {8, rig ? 8 : 5};
    const float factor[2] = {1.2f, rig ? 1.2f : 1.1f};
    const double R[2][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0.9995, 0.01, -0.03, -0.0097, 0.9999, 0.01, 0.0301, -0.0097, 0.9995}};
    const double O[2][3] = {{0, 0, 0}, {0.4, 0.1, 0.8}};
    const float w = rig ? 512.f : 640.f, h = rig ? 512.f : 480.f;
    for (int k = 0; k < 2; k++) {
        Side &K = S.kf[k];
        K.n_left = shape[k][0]; K.n_right = shape[k][1]; K.nlevels = levels[k];
        for (int l = 0; l < 8; l++) { K.scale[l] = l ? K.scale[l - 1] * factor[k] : 1.f; K.sigma2[l] = K.scale[l] * K.scale[l]; }
        const double Or[3] = {O[k][0] + 0.101 * R[k][0], O[k][1] + 0.101 * R[k][1], O[k][2] + 0.101 * R[k][2]};   // the right camera: same rotation, 10 cm along x
        set_view(K.view[0], R[k], O[k], rig ? kKb8[0] : kPinhole);
        set_view(K.view[1], R[k], Or, kKb8[1]);
        K.kps.resize((size_t)K.n());
        K.desc.resize(32 * (size_t)K.n());
        for (uint8_t &b : K.desc) b = (uint8_t)rng();
        for (orbx_keypoint &kp : K.kps) {
            memset(&kp, 0, sizeof(kp));
            kp.x = uni(20.f, w - 20.f); kp.y = uni(20.f, h - 20.f); kp.octave = (int)(rng() % (unsigned)K.nlevels); kp.size = 31.f; kp.class_id = -1;
            kp.angle = uni(0.f, 359.f);
        }
        if (!rig) K.u_right.assign((size_t)K.n(), -1.f);
    }
    S.par.ratio_factor = 1.5f * 1.2f; S.par.inertial = 0; S.par.far_points = 1; S.par.th_far_points = 7.5f;
    S.par.nlevels_1 = levels[0]; S.par.nlevels_2 = levels[1]; S.par.level_sigma2_1 = S.kf[0].sigma2; S.par.level_sigma2_2 = S.kf[1].sigma2;
    // designed pairs: feature i of key frame 1 with feature n2 - 1 - i of key frame 2 (on a rig that crosses the cameras for part of them)
    const int n_designed = std::min(S.kf[0].n(), S.kf[1].n()) - 20;
    for (int i = 0; i < n_designed; i++) {
        const int j = S.kf[1].n() - 1 - i, kind = i % 16;
        float z = uni(3.f, 7.f);
        if (kind == 9) z = uni(8.5f, 12.f);                  // beyond mThFarPoints
        if (kind == 10) z = uni(150.f, 400.f);               // no parallax
        float P[3] = {0.2f + uni(-0.45f, 0.45f) * z, 0.05f + uni(-0.35f, 0.35f) * z, 0.4f + z};
        if (kind == 11) { P[0] = uni(-1.f, 1.f); P[1] = uni(-0.7f, 0.7f); P[2] = -uni(2.5f, 5.f); }                  // behind both
        if (kind == 12) { P[0] = 0.2f + uni(-0.1f, 0.1f); P[1] = 0.05f + uni(-0.1f, 0.1f); P[2] = 0.4f; }            // between the centres: behind key frame 2
        const int idx[2] = {i, j};
        for (int k = 0; k < 2; k++) {
            Side &K = S.kf[k];
            const bool right = rig && idx[k] >= K.n_left;
            orbx_keypoint &kp = K.kps[(size_t)idx[k]];
            project(rig, K.view[right ? 1 : 0], P, &kp.x, &kp.y);
            const float noise = (kind == 13 && k == 0) || (kind == 14 && k == 1) ? 7.f : 0.3f;
            kp.x += uni(-noise, noise); kp.y += uni(-noise, noise);
            kp.octave = kind == 15 ? (k == 0 ? K.nlevels - 1 : 0) : (int)(rng() % 3u);          // kind 15: the scale ratio
            if (kind == 14 && k == 0) kp.octave = K.nlevels - 1;
        }
        if (!rig && kind == 8) S.kf[i % 2].u_right[(size_t)idx[i % 2]] = S.kf[i % 2].kps[(size_t)idx[i % 2]].x - 10.f;   // a stereo observation on one side
        for (int b = 0; b < 32; b++) S.kf[1].desc[32 * (size_t)j + b] = S.kf[0].desc[32 * (size_t)i + b];             // the same point: a near copy
        for (int f = 0; f < 6; f++) { const unsigned bit = rng() % 256; S.kf[1].desc[32 * (size_t)j + bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
        S.idx1.push_back(i); S.idx2.push_back(kind == 7 ? -1 : j);
    }
    if (rig) {   // N_left - 1 and N_left of both key frames, whatever they triangulate to
        S.idx1.push_back(S.kf[0].n_left - 1); S.idx2.push_back(S.kf[1].n_left);
        S.idx1.push_back(S.kf[0].n_left); S.idx2.push_back(S.kf[1].n_left - 1);
    }
}

// the member's loop body for one pair (include/orbx.h); returns the status, x3D where it is ORBX_NEWPT_OK
int member(const Scene &S, int i1, int i2, float *x3D) {
    if (i2 < 0) return ORBX_NEWPT_NO_MATCH;
    const Side &K1 = S.kf[0], &K2 = S.kf[1];
    const orbx_keypoint &kp1 = K1.kps[(size_t)i1], &kp2 = K2.kps[(size_t)i2];
    const bool bRight1 = S.rig && i1 >= K1.n_left, bRight2 = S.rig && i2 >= K2.n_left;
    const bool bStereo1 = !S.rig && K1.u_right[(size_t)i1] >= 0, bStereo2 = !S.rig && K2.u_right[(size_t)i2] >= 0;
    if (bStereo1 || bStereo2) return ORBX_NEWPT_STEREO_LEFT_TO_HOST;
    const orbx_fisheye_view &V1 = K1.view[bRight1 ? 1 : 0], &V2 = K2.view[bRight2 ? 1 : 0];
    const float *R1 = V1.R, *R2 = V2.R, *t1 = V1.t, *t2 = V2.t;
    float xn1[3] = {0, 0, 1.f}, xn2[3] = {0, 0, 1.f};
    if (S.rig) { kb8_unproject(V1.params, kp1.x, kp1.y, &xn1[0], &xn1[1]); kb8_unproject(V2.params, kp2.x, kp2.y, &xn2[0], &xn2[1]); }
    else {
        xn1[0] = (kp1.x - V1.params[2]) / V1.params[0]; xn1[1] = (kp1.y - V1.params[3]) / V1.params[1];
        xn2[0] = (kp2.x - V2.params[2]) / V2.params[0]; xn2[1] = (kp2.y - V2.params[3]) / V2.params[1];
    }
    float ray1[3], ray2[3];
    for (int r = 0; r < 3; r++) {   // Rwc = Rcw.transpose()
        ray1[r] = dot3(R1[r], R1[3 + r], R1[6 + r], xn1[0], xn1[1], xn1[2]);
        ray2[r] = dot3(R2[r], R2[3 + r], R2[6 + r], xn2[0], xn2[1], xn2[2]);
    }
    const float n1 = sqrtf(dot3(ray1[0], ray1[1], ray1[2], ray1[0], ray1[1], ray1[2])), n2 = sqrtf(dot3(ray2[0], ray2[1], ray2[2], ray2[0], ray2[1], ray2[2]));
    const float cosParallaxRays = dot3(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]) / (n1 * n2);
    const float cosParallaxStereo = cosParallaxRays + 1;
    if (!(cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && cosParallaxRays < (S.par.inertial ? 0.9996 : 0.9998))) return ORBX_NEWPT_LOW_PARALLAX;
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
    const float X[3] = {xh[0] / xh[3], xh[1] / xh[3], xh[2] / xh[3]};
    const float z1 = dot3(R1[6], R1[7], R1[8], X[0], X[1], X[2]) + t1[2];
    if (z1 <= 0) return ORBX_NEWPT_BEHIND_1;
    const float z2 = dot3(R2[6], R2[7], R2[8], X[0], X[1], X[2]) + t2[2];
    if (z2 <= 0) return ORBX_NEWPT_BEHIND_2;
    float u, v;
    const float x1 = dot3(R1[0], R1[1], R1[2], X[0], X[1], X[2]) + t1[0], y1 = dot3(R1[3], R1[4], R1[5], X[0], X[1], X[2]) + t1[1];
    if (S.rig) kb8_project(V1.params, x1, y1, z1, &u, &v);
    else { u = V1.params[0] * x1 / z1 + V1.params[2]; v = V1.params[1] * y1 / z1 + V1.params[3]; }
    const float errX1 = u - kp1.x, errY1 = v - kp1.y;
    if ((errX1 * errX1 + errY1 * errY1) > 5.991 * K1.sigma2[kp1.octave]) return ORBX_NEWPT_REPROJ_1;
    const float x2 = dot3(R2[0], R2[1], R2[2], X[0], X[1], X[2]) + t2[0], y2 = dot3(R2[3], R2[4], R2[5], X[0], X[1], X[2]) + t2[1];
    if (S.rig) kb8_project(V2.params, x2, y2, z2, &u, &v);
    else { u = V2.params[0] * x2 / z2 + V2.params[2]; v = V2.params[1] * y2 / z2 + V2.params[3]; }
    const float errX2 = u - kp2.x, errY2 = v - kp2.y;
    if ((errX2 * errX2 + errY2 * errY2) > 5.991 * K2.sigma2[kp2.octave]) return ORBX_NEWPT_REPROJ_2;
    const float a0 = X[0] - V1.twc[0], a1 = X[1] - V1.twc[1], a2 = X[2] - V1.twc[2], b0 = X[0] - V2.twc[0], b1 = X[1] - V2.twc[1], b2 = X[2] - V2.twc[2];
    const float dist1 = sqrtf(dot3(a0, a1, a2, a0, a1, a2)), dist2 = sqrtf(dot3(b0, b1, b2, b0, b1, b2));
    if (dist1 == 0 || dist2 == 0) return ORBX_NEWPT_ZERO_DIST;
    if (S.par.far_points && (dist1 >= S.par.th_far_points || dist2 >= S.par.th_far_points)) return ORBX_NEWPT_FAR;
    const float ratioDist = dist2 / dist1, ratioOctave = K1.scale[kp1.octave] / K2.scale[kp2.octave], ratioFactor = S.par.ratio_factor;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return ORBX_NEWPT_SCALE_RATIO;
    x3D[0] = X[0]; x3D[1] = X[1]; x3D[2] = X[2];
    return ORBX_NEWPT_OK;
}

int make_key_frames(orbx_matcher *m, const Scene &S, orbx_keyframe **kfs) {
    for (int k = 0; k < 2; k++) {
        const Side &K = S.kf[k];
        orbx_frame_desc d;
        memset(&d, 0, sizeof(d));
        d.keypoints_un = K.kps.data(); d.descriptors = K.desc.data(); d.n = K.n_left;
        d.min_x = 0.f; d.max_x = S.rig ? 512.f : 640.f; d.min_y = 0.f; d.max_y = S.rig ? 512.f : 480.f;
        d.scale_factors = K.scale; d.nlevels = K.nlevels;
        d.u_right = S.rig ? nullptr : K.u_right.data();
        if (S.rig) MUST(orbx_keyframe_create_host_fisheye(m, &d, K.kps.data() + K.n_left, K.n_right, nullptr, &kfs[k]));
        else MUST(orbx_keyframe_create_host(m, &d, nullptr, &kfs[k]));
    }
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

void views_of(const Scene &S, orbx_new_points_view *pin) {
    for (int k = 0; k < 2; k++) {
        const orbx_fisheye_view &V = S.kf[k].view[0];
        memcpy(pin[k].Rcw, V.R, sizeof(V.R)); memcpy(pin[k].tcw, V.t, sizeof(V.t)); memcpy(pin[k].Ow, V.twc, sizeof(V.twc));
        pin[k].fx = V.params[0]; pin[k].fy = V.params[1]; pin[k].cx = V.params[2]; pin[k].cy = V.params[3];
    }
}

int pairs_call(orbx_matcher *m, const Scene &S, orbx_keyframe *const *kfs, int n, const int32_t *i1, const int32_t *i2, float *pos, uint8_t *st, int *acc) {
    orbx_new_points_view pin[2];
    views_of(S, pin);
    return S.rig ? orbx_keyframe_triangulate_pairs_fisheye(m, kfs[0], kfs[1], S.kf[0].view, S.kf[1].view, &S.par, n, i1, i2, pos, st, acc)
                 : orbx_keyframe_triangulate_pairs(m, kfs[0], kfs[1], &pin[0], &pin[1], &S.par, n, i1, i2, pos, st, acc);
}

// status and pos of n pairs against the member; returns the number of mismatches (printed)
int compare(const Scene &S, int n, const int32_t *i1, const int32_t *i2, const float *pos, const uint8_t *st, int acc, int *hist) {
    int bad = 0, accepted = 0;
    for (int p = 0; p < n; p++) {
        float X[3] = {kSentinel, kSentinel, kSentinel};
        const int want = member(S, i1[p], i2[p], X);
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

void transfers(const orbx_matcher *m, int64_t *t) { orbx_matcher_debug_transfers(m, t, 6); }

int run(bool rig, int time_runs) {
    Scene S;
    make_scene(S, rig);
    orbx_matcher *m = nullptr;
    MUST(orbx_matcher_create(0, &m));
    orbx_keyframe *kfs[2] = {nullptr, nullptr};
    if (make_key_frames(m, S, kfs)) return 1;
    const int sizes[] = {1, 63, 64, 65, (int)S.idx1.size()};
    int hist[12] = {0};
    for (int n : sizes) {   // heap blocks of exactly the needed size
        std::unique_ptr<int32_t[]> i1(new int32_t[(size_t)n]), i2(new int32_t[(size_t)n]);
        std::unique_ptr<float[]> pos(new float[3 * (size_t)n]);
        std::unique_ptr<uint8_t[]> st(new uint8_t[(size_t)n]);
        const size_t from = S.idx1.size() - (size_t)n;       // (the tail: a rig's edge indices are in every size)
        memcpy(i1.get(), S.idx1.data() + from, 4 * (size_t)n); memcpy(i2.get(), S.idx2.data() + from, 4 * (size_t)n);
        std::fill(pos.get(), pos.get() + 3 * (size_t)n, kSentinel); std::fill(st.get(), st.get() + n, kStatusSentinel);
        int acc = -1;
        MUST(pairs_call(m, S, kfs, n, i1.get(), i2.get(), pos.get(), st.get(), &acc));
        int h[12] = {0};
        CHECK(compare(S, n, i1.get(), i2.get(), pos.get(), st.get(), acc, n == (int)S.idx1.size() ? hist : h) == 0);
        int64_t t[6];
        transfers(m, t);
        CHECK(t[0] == 1 && t[1] == 1 && t[4] == 0 && t[5] == 2);
    }
    printf("%s pairs: status counts", rig ? "rig" : "monocular");
    for (int s = 0; s < 12; s++) printf(" %d", hist[s]);
    printf("\n");
    CHECK(hist[ORBX_NEWPT_OK] * 10 >= (int)S.idx1.size() * 3 && hist[ORBX_NEWPT_NO_MATCH] >= 3 && hist[ORBX_NEWPT_LOW_PARALLAX] >= 3 &&
          hist[ORBX_NEWPT_BEHIND_1] >= 3 && hist[ORBX_NEWPT_REPROJ_1] >= 3 && hist[ORBX_NEWPT_FAR] >= 3 && hist[ORBX_NEWPT_SCALE_RATIO] >= 3);
    CHECK(rig || hist[ORBX_NEWPT_STEREO_LEFT_TO_HOST] >= 3);

    // refusals and the empty call: nothing enqueued, nothing written
    int64_t before[6], after[6];
    transfers(m, before);
    {
        float pos[3] = {kSentinel, kSentinel, kSentinel};
        uint8_t st = kStatusSentinel;
        int acc = -7;
        const int32_t ok1 = 0, ok2 = 0, high1 = S.kf[0].n(), high2 = S.kf[1].n(), low2 = -2;
        CHECK(pairs_call(m, S, kfs, 1, &high1, &ok2, pos, &st, &acc) == ORBX_E_BAD_ARG);
        CHECK(pairs_call(m, S, kfs, 1, &ok1, &high2, pos, &st, &acc) == ORBX_E_BAD_ARG);
        CHECK(pairs_call(m, S, kfs, 1, &ok1, &low2, pos, &st, &acc) == ORBX_E_BAD_ARG);
        CHECK(pairs_call(m, S, kfs, -1, &ok1, &ok2, pos, &st, &acc) == ORBX_E_BAD_ARG);
        CHECK(pairs_call(m, S, kfs, 1, &ok1, &ok2, nullptr, &st, &acc) == ORBX_E_BAD_ARG);
        Scene other = S;
        other.rig = !rig;                                    // the other kind's entry point
        CHECK(pairs_call(m, other, kfs, 1, &ok1, &ok2, pos, &st, &acc) == ORBX_E_BAD_ARG);
        Scene levels = S;
        levels.par.nlevels_2 += 1;
        CHECK(pairs_call(m, levels, kfs, 1, &ok1, &ok2, pos, &st, &acc) == ORBX_E_BAD_ARG);
        CHECK(pos[0] == kSentinel && st == kStatusSentinel && acc == -7);
        CHECK(pairs_call(m, S, kfs, 0, nullptr, nullptr, nullptr, nullptr, &acc) == ORBX_OK && acc == 0);
    }
    transfers(m, after);
    CHECK(memcmp(before, after, sizeof(before)) == 0);

    // the fused form: BoW on both key frames, the search alone, then the search with the triangulation behind it
    orbx_vocabulary *voc = nullptr;
    if (make_vocabulary(&voc)) return 1;
    for (int k = 0; k < 2; k++)
        MUST(rig ? orbx_keyframe_compute_bow_fisheye(m, kfs[k], voc, 1, nullptr, nullptr) : orbx_keyframe_compute_bow(m, kfs[k], voc, 1, nullptr, nullptr));
    const int n1 = S.kf[0].n();
    std::vector<uint8_t> skip1((size_t)n1, 0);
    for (int i = 0; i < n1; i += 7) skip1[(size_t)i] = 1;
    orbx_keyframe_gate g;
    memset(&g, 0, sizeof(g));
    g.coarse = 1; g.strict_fp = 1; g.ep_x = g.ep_y = 1e6f; g.nlevels = S.kf[1].nlevels; g.level_sigma2_2 = S.kf[1].sigma2;
    orbx_keyframe_kb8_gate gk;
    memset(&gk, 0, sizeof(gk));
    gk.coarse = 1; gk.nlevels = S.kf[1].nlevels; gk.level_sigma2_1 = S.kf[0].sigma2; gk.level_sigma2_2 = S.kf[1].sigma2;
    orbx_new_points_view pin[2];
    views_of(S, pin);
    for (int pass = 0; pass < 2; pass++) {
        const uint8_t *s1 = pass ? skip1.data() : nullptr;
        std::unique_ptr<int32_t[]> plain(new int32_t[(size_t)n1]), m12(new int32_t[(size_t)n1]), own(new int32_t[(size_t)n1]);
        std::unique_ptr<float[]> pos(new float[3 * (size_t)n1]);
        std::unique_ptr<uint8_t[]> st(new uint8_t[(size_t)n1]);
        std::fill(pos.get(), pos.get() + 3 * (size_t)n1, kSentinel); std::fill(st.get(), st.get() + n1, kStatusSentinel);
        const int nm = rig ? orbx_keyframe_search_for_triangulation_fisheye(m, kfs[0], kfs[1], s1, nullptr, 1, &gk, plain.get())
                           : orbx_keyframe_search_for_triangulation(m, kfs[0], kfs[1], s1, nullptr, 1, &g, plain.get());
        MUST(nm);
        int64_t ts[6], tf[6];
        transfers(m, ts);
        int acc = -1;
        const int nf = rig ? orbx_keyframe_search_and_triangulate_fisheye(m, kfs[0], kfs[1], s1, nullptr, 1, &gk, S.kf[0].view, S.kf[1].view, &S.par, m12.get(),
                                                                          pos.get(), st.get(), &acc)
                           : orbx_keyframe_search_and_triangulate(m, kfs[0], kfs[1], s1, nullptr, 1, &g, &pin[0], &pin[1], &S.par, m12.get(), pos.get(), st.get(),
                                                                  &acc);
        MUST(nf);
        transfers(m, tf);
        CHECK(nf == nm && memcmp(plain.get(), m12.get(), 4 * (size_t)n1) == 0 && nm >= 40);
        for (int i = 0; i < n1; i++) own[(size_t)i] = i;
        int h[12] = {0};
        CHECK(compare(S, n1, own.get(), m12.get(), pos.get(), st.get(), acc, h) == 0);
        CHECK(h[ORBX_NEWPT_OK] >= 20 && h[ORBX_NEWPT_NO_MATCH] >= 20);
        CHECK(tf[0] == 1 && tf[1] == 1 && ts[0] == 1 && ts[1] == 1 && tf[5] == ts[5] && tf[4] == 0);     // one run each way, no launch of a transfer more
        printf("%s fused (%s skip flags): %d matches, %d accepted, upload %lld -> %lld bytes, download %lld -> %lld bytes\n", rig ? "rig" : "monocular",
               pass ? "with" : "no", nm, acc, (long long)ts[2], (long long)tf[2], (long long)ts[3], (long long)tf[3]);
    }
    if (time_runs > 0) {
        const int n = (int)S.idx1.size();
        float X[3];
        long sink = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < time_runs; r++)
            for (int p = 0; p < n; p++) sink += member(S, S.idx1[(size_t)p], S.idx2[(size_t)p], X);
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / time_runs;
        printf("host reference loop (%s, %d pairs, contiguous arrays): %.1f us per run (%ld)\n", rig ? "rig" : "monocular", n, us, sink);
    }
    orbx_keyframe_destroy(kfs[0]); orbx_keyframe_destroy(kfs[1]);
    orbx_vocabulary_destroy(voc);
    orbx_matcher_destroy(m);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const int time_runs = argc > 1 ? atoi(argv[1]) : 0;
    if (run(false, time_runs) || run(true, time_runs)) return 1;
    printf("new points ok\n");
    return 0;
}
