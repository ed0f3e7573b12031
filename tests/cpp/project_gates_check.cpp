// The gates every map-point projection kernel shares (rigid transform, distance gate, PO . Pn, PredictScale, Pinhole::project: the helpers of
// geometry_kernels.hip.h), through every entry point that runs them, on ONE scene whose verdicts are known by construction.
//   Points: 257 (two blocks of 256, the second with one live lane), built in the camera frame of view A; point i belongs to class i % 10 --
//     0 accepted, 1 skipped (the skip row; an id of -1 where the queries are map ids), 2 behind the camera, 3 .. 6 left / right / above / below the
//     image, 7 nearer than 0.8 min, 8 farther than 1.2 max, 9 seen from behind its normal.  Directions inside the image lie within 0.2 of the axis,
//     those outside at a slope of 10, bounds are missed by factors of 1.6 and more, normals point straight at or away from the camera: every other
//     view is view A moved by centimetres and hundredths of a radian, so no verdict comes near a rounding.  Point 0 predicts a level below 0, point
//     10 one above the last level: both clamp.
//   Views: monocular key frames A (bounds of the image, 8 levels), B (wider bounds, 6 levels) and A2 (A's bounds, 6 levels: the Sim3 members want one
//     set of bounds per call); rig key frames likewise; one monocular and one rig frame for Relocalization's search.
//   Entry points: orbx_is_in_frustum, orbx_is_in_frustum_checks, orbx_keyframe_fuse_map_points[_fisheye] with a skip row per key frame,
//     orbx_keyframe_search_by_projection_sim3[_fisheye] in both projection forms with projected, proj_u and proj_v,
//     orbx_frame_search_by_projection_keyframe[_fisheye]_map.
//   Asserted: in_view / projected equal the designed verdict for every pair; every class has at least 20 pairs per call; where all three accept,
//     isInFrustum, the Sim3 search (ORBX_SIM3_PROJECT_CAMERA) and Relocalization's search hold the same (u, v) bit for bit for the same view and point
//     -- the pinhole trio and the KannalaBrandt8 trio.
//   Printed: a checksum of every output array over all pairs, rejected pairs included.  Two builds of the library that compute the same print the same.
// Every caller array is a heap block of exactly the needed size.  Stand-alone, against include/orbx.h only: linked against the emulator build of the
// library (python tests/simt/build.py --asan --static-rt) and compiled with -fsanitize=address,undefined, as tests/cpp/track_map_check.cpp; or against
// liborbx.so on a GPU.  Prints "project gates ok" and returns 0.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kPoints = 257, kClasses = 10, kCapacity = 512, kRandom = 60;
constexpr float kFx = 400.f, kCx = 320.f, kCy = 240.f, kBf = 40.f, kScale = 1.1f;
const float kKb8[8] = {190.978477f, 190.973307f, 254.931706f, 256.897443f, 0.00348238940f, 0.000715034845f, -0.00205323614f, 0.000202936736f};
enum Class { ACCEPT, SKIP, BEHIND, LEFT, RIGHT, ABOVE, BELOW, NEAR, FAR, BACK };
enum Kind { FRUSTUM, KEYFRAME, RELOC_PINHOLE, RELOC_KB8 };

#define MUST(expr)                                                                   \
    do {                                                                             \
        const int r_ = (expr);                                                       \
        if (r_ < 0) { printf("%s: %d\n", #expr, r_); return 1; }                     \
    } while (0)
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

// the verdict of point i by construction: `skipped` = its entry of the call's skip row (KEYFRAME) or an id of -1 (RELOC_*)
bool verdict(Kind kind, int i, bool skipped) {
    const int c = i % kClasses;
    switch (kind) {
    case FRUSTUM: return c == ACCEPT || c == SKIP;                                  // isInFrustum has no skip argument
    case KEYFRAME: return c == ACCEPT && !skipped;
    case RELOC_PINHOLE: return !skipped && (c == ACCEPT || c == BACK || c == BEHIND);   // no normal gate, no depth gate: (-X, -Y, -Z) projects where (X, Y, Z) does
    case RELOC_KB8: return !skipped && (c == ACCEPT || c == BACK);                  // KannalaBrandt8 sends a point behind the camera far outside the image
    }
    return false;
}

struct View {
    float R[9], t[3], C[3];
    orbx_frame_pose pose() const {
        orbx_frame_pose p;
        memcpy(p.Rcw, R, sizeof(R)); memcpy(p.tcw, t, sizeof(t)); memcpy(p.Ow, C, sizeof(C));
        return p;
    }
    orbx_fisheye_view fisheye() const {
        orbx_fisheye_view v;
        memcpy(v.R, R, sizeof(R)); memcpy(v.t, t, sizeof(t)); memcpy(v.twc, C, sizeof(C)); memcpy(v.params, kKb8, sizeof(kKb8));
        return v;
    }
};
View make_view(double yaw, double pitch, double roll, double tx, double ty, double tz) {
    const double cy = cos(yaw), sy = sin(yaw), cp = cos(pitch), sp = sin(pitch), cr = cos(roll), sr = sin(roll);
    const double R[9] = {cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr, -sp, cp * sr, cp * cr};
    const double t[3] = {tx, ty, tz};
    View v;
    for (int k = 0; k < 9; k++) v.R[k] = (float)R[k];
    for (int k = 0; k < 3; k++) {
        v.t[k] = (float)t[k];
        v.C[k] = (float)-(R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2]);   // -R^T t
    }
    return v;
}

// where a view sees a point, in double: good enough to put a feature within a pixel of it
void project(const View &V, bool kb8, const float *p, double *u, double *v) {
    double c[3];
    for (int r = 0; r < 3; r++) c[r] = (double)V.R[3 * r] * p[0] + (double)V.R[3 * r + 1] * p[1] + (double)V.R[3 * r + 2] * p[2] + V.t[r];
    if (!kb8) { *u = kFx * c[0] / c[2] + kCx; *v = kFx * c[1] / c[2] + kCy; return; }
    const double th = atan2(sqrt(c[0] * c[0] + c[1] * c[1]), c[2]), psi = atan2(c[1], c[0]);
    const double th2 = th * th, r = th * (1 + th2 * (kKb8[4] + th2 * (kKb8[5] + th2 * (kKb8[6] + th2 * kKb8[7]))));
    *u = kKb8[0] * r * cos(psi) + kKb8[2]; *v = kKb8[1] * r * sin(psi) + kKb8[3];
}

struct Scene {
    View A;
    std::vector<float> pos, normal, min_dist, max_dist;
    std::vector<uint8_t> desc;
    std::vector<int> level;   // the level the point is built for
    float scale[8], inv_sigma2[8];
};

void make_scene(Scene &S) {
    std::mt19937 rng(2027);
    auto uni = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); };
    for (int l = 0; l < 8; l++) { S.scale[l] = l ? S.scale[l - 1] * kScale : 1.f; S.inv_sigma2[l] = 1.f / (S.scale[l] * S.scale[l]); }
    S.A = make_view(0.03, -0.02, 0.015, 0.05, -0.03, 0.08);
    S.pos.resize(3 * kPoints); S.normal.resize(3 * kPoints); S.min_dist.resize(kPoints); S.max_dist.resize(kPoints); S.desc.resize(32 * kPoints);
    S.level.resize(kPoints);
    for (uint8_t &b : S.desc) b = (uint8_t)rng();
    for (int i = 0; i < kPoints; i++) {
        const int c = i % kClasses;
        const double z = uni(5., 9.);
        double sx = uni(-0.2, 0.2), sy = uni(-0.2, 0.2);
        if (c == LEFT) sx = -10.;
        if (c == RIGHT) sx = 10.;
        if (c == ABOVE) sy = -10.;
        if (c == BELOW) sy = 10.;
        double pc[3] = {sx * z, sy * z, z};
        if (c == BEHIND) for (double &x : pc) x = -x;
        double w[3], po[3];   // world = R^T (pc - t)
        for (int k = 0; k < 3; k++)
            w[k] = S.A.R[k] * (pc[0] - S.A.t[0]) + S.A.R[3 + k] * (pc[1] - S.A.t[1]) + S.A.R[6 + k] * (pc[2] - S.A.t[2]);
        for (int k = 0; k < 3; k++) { S.pos[3 * i + k] = (float)w[k]; po[k] = w[k] - S.A.C[k]; }
        const double d = sqrt(po[0] * po[0] + po[1] * po[1] + po[2] * po[2]);
        for (int k = 0; k < 3; k++) S.normal[3 * i + k] = (float)((c == BACK ? -1. : 1.) * po[k] / d);
        const int L = (int)(rng() % 5) + 1;
        S.level[i] = L;
        double mx = d * pow((double)kScale, L - 0.5), mn = mx / 16.;   // log(max / dist) / log(scale) = L - 0.5: the level is L
        if (i == 0) { mx = 0.87 * d; mn = mx / 16.; S.level[i] = 0; }             // log(0.87) / log(1.1) = -1.46: ceil gives -1, clamped to 0 (inside 1.2 max)
        if (i == 10) { mx = d * pow((double)kScale, 20.); mn = d / 16.; S.level[i] = 5; }   // level 20, clamped to nlevels - 1
        if (c == NEAR) mn = 2. * d;    // 0.8 min = 1.6 dist
        if (c == FAR) mx = 0.5 * d;    // 1.2 max = 0.6 dist
        if (c == FAR) mn = mx / 16.;
        S.min_dist[i] = (float)mn; S.max_dist[i] = (float)mx;
    }
}

// features of a frame / key frame that sees the scene through V: one near the projection of every point built to be seen, its descriptor 8 bits from the
// point's, its octave at the point's level or one below, then kRandom more anywhere; rows beyond `left` are the right camera's of a rig (through VR)
struct Features {
    std::vector<orbx_keypoint> kps;
    std::vector<uint8_t> desc;
    std::vector<float> ur;
};
void add_feature(Features &F, std::mt19937 &rng, float x, float y, int octave, const uint8_t *d, float ur) {
    orbx_keypoint kp;
    memset(&kp, 0, sizeof(kp));
    kp.x = x; kp.y = y; kp.octave = octave; kp.size = 31.f; kp.angle = (float)(rng() % 360); kp.response = 50.f; kp.class_id = -1;
    F.kps.push_back(kp);
    for (int b = 0; b < 32; b++) F.desc.push_back(d ? d[b] : (uint8_t)rng());
    if (d) for (int k = 0; k < 8; k++) { const unsigned bit = rng() % 256; F.desc[F.desc.size() - 32 + bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
    F.ur.push_back(ur);
}
int add_camera(Features &F, const Scene &S, const View &V, bool kb8, int nlevels, float w, float h, unsigned seed) {
    std::mt19937 rng(seed);
    auto uni = [&](double a, double b) { return (float)std::uniform_real_distribution<double>(a, b)(rng); };
    const size_t before = F.kps.size();
    for (int i = 0; i < kPoints; i++) {
        if (i % kClasses != ACCEPT && i % kClasses != SKIP) continue;
        double u, v;
        project(V, kb8, &S.pos[3 * (size_t)i], &u, &v);
        const int o = std::min(std::max(S.level[(size_t)i] - (int)(rng() % 2), 0), nlevels - 1);
        const float x = (float)u + uni(-0.7, 0.7);
        add_feature(F, rng, x, (float)v + uni(-0.7, 0.7), o, &S.desc[32 * (size_t)i], i % 4 == 0 ? x - kBf / 7.f + uni(-0.5, 0.5) : -1.f);
    }
    for (int j = 0; j < kRandom; j++) add_feature(F, rng, uni(1., w - 1.), uni(1., h - 1.), (int)(rng() % (unsigned)nlevels), nullptr, -1.f);
    return (int)(F.kps.size() - before);
}

uint64_t fnv(const void *p, size_t bytes) {
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < bytes; k++) h = (h ^ ((const uint8_t *)p)[k]) * 1099511628211ull;
    return h;
}
template <class T>
void sum(const char *name, const std::unique_ptr<T[]> &a, size_t n) { printf(" %s=%016llx", name, (unsigned long long)fnv(a.get(), n * sizeof(T))); }

// got[pair] against the designed verdict; at least 20 pairs of every class
bool verdicts_ok(const char *what, Kind kind, int rows, const uint8_t *got, const uint8_t *skip, int skip_div) {
    int per_class[kClasses] = {0};
    for (int r = 0; r < rows; r++)
        for (int i = 0; i < kPoints; i++) {
            const bool sk = skip && skip[(size_t)(r / skip_div) * kPoints + i];
            per_class[i % kClasses]++;
            if ((got[(size_t)r * kPoints + i] != 0) != verdict(kind, i, sk)) {
                printf("FAILED: %s row %d point %d (class %d): got %d\n", what, r, i, i % kClasses, got[(size_t)r * kPoints + i]);
                return false;
            }
        }
    for (int c = 0; c < kClasses; c++)
        if (per_class[c] < 20) { printf("FAILED: %s has %d pairs of class %d\n", what, per_class[c], c); return false; }
    return true;
}

struct Uv { std::vector<float> u, v; std::vector<uint8_t> ok; };   // one view's row of a call, kept for the cross-kernel comparison
Uv keep(const float *u, const float *v, const uint8_t *ok) { return Uv{{u, u + kPoints}, {v, v + kPoints}, {ok, ok + kPoints}}; }
// where all three accept: the same bits
int trio_agrees(const char *what, const Uv &a, const Uv &b, const Uv &c) {
    int n = 0;
    for (int i = 0; i < kPoints; i++) {
        if (!(a.ok[i] && b.ok[i] && c.ok[i])) continue;
        n++;
        if (memcmp(&a.u[i], &b.u[i], 4) || memcmp(&a.u[i], &c.u[i], 4) || memcmp(&a.v[i], &b.v[i], 4) || memcmp(&a.v[i], &c.v[i], 4)) {
            printf("FAILED: %s point %d: (%a %a) (%a %a) (%a %a)\n", what, i, a.u[i], a.v[i], b.u[i], b.v[i], c.u[i], c.v[i]);
            return -1;
        }
    }
    return n;
}

}  // namespace

int main() {
    Scene S;
    make_scene(S);
    const float lsf = std::log(kScale);
    // view B: A moved; the right cameras: 5 cm beside their left ones, turned a little
    const View A = S.A, B = make_view(0.04, -0.012, 0.01, 0.07, -0.02, 0.06);
    const View AR = make_view(0.034, -0.02, 0.012, 0.0, -0.03, 0.08), BR = make_view(0.036, -0.012, 0.012, 0.02, -0.02, 0.06);
    const float boundsA[4] = {0.f, 640.f, 0.f, 480.f}, boundsB[4] = {-12.5f, 655.25f, -9.75f, 492.5f};
    const float rigA[4] = {30.f, 480.f, 30.f, 480.f}, rigB[4] = {20.f, 490.f, 24.f, 486.f};

    orbx_matcher *m = nullptr;
    MUST(orbx_matcher_create(0, &m));
    const size_t np = kPoints;

    // skip rows: class 1 in every row; the second key frame's row also drops every fourth accepted point, so a row read for the wrong key frame shows
    std::unique_ptr<uint8_t[]> skip(new uint8_t[2 * np]);
    for (int k = 0; k < 2; k++)
        for (int i = 0; i < kPoints; i++) skip[(size_t)k * np + i] = i % kClasses == SKIP || (k == 1 && i % 40 == 0);

    // ---- key frames and frames
    auto desc_of = [&](const Features &F, int n, const float *b, int nlevels, bool ur) {
        orbx_frame_desc d;
        memset(&d, 0, sizeof(d));
        d.keypoints_un = F.kps.data(); d.descriptors = F.desc.data(); d.n = n;
        d.min_x = b[0]; d.max_x = b[1]; d.min_y = b[2]; d.max_y = b[3];
        d.scale_factors = S.scale; d.nlevels = nlevels; d.u_right = ur ? F.ur.data() : nullptr;
        return d;
    };
    Features fA, fB, fA2, fRA, fRB, fRA2, fCur, fRig, fSrc, fRigSrc;
    add_camera(fA, S, A, false, 8, 640.f, 480.f, 1); add_camera(fB, S, B, false, 6, 640.f, 480.f, 2); add_camera(fA2, S, B, false, 6, 640.f, 480.f, 3);
    const int nlA = add_camera(fRA, S, A, true, 8, 512.f, 512.f, 4), nrA = add_camera(fRA, S, AR, true, 8, 512.f, 512.f, 5);
    const int nlB = add_camera(fRB, S, B, true, 6, 512.f, 512.f, 6), nrB = add_camera(fRB, S, BR, true, 6, 512.f, 512.f, 7);
    const int nlA2 = add_camera(fRA2, S, B, true, 6, 512.f, 512.f, 8), nrA2 = add_camera(fRA2, S, BR, true, 6, 512.f, 512.f, 9);
    add_camera(fCur, S, A, false, 8, 640.f, 480.f, 10);
    const int nlC = add_camera(fRig, S, A, true, 8, 512.f, 512.f, 11), nrC = add_camera(fRig, S, AR, true, 8, 512.f, 512.f, 12);
    {   // the sources of Relocalization's search: feature i carries point i; only its octave and angle are read
        std::mt19937 rng(13);
        for (int i = 0; i < kPoints; i++) add_feature(fSrc, rng, (float)(1 + rng() % 600), (float)(1 + rng() % 400), (int)(rng() % 8), nullptr, -1.f);
        for (int i = 0; i < kPoints; i++) add_feature(fRigSrc, rng, (float)(1 + rng() % 500), (float)(1 + rng() % 500), (int)(rng() % 8), nullptr, -1.f);
    }
    constexpr int kSrcLeft = 150;
    orbx_keyframe *kfA = nullptr, *kfB = nullptr, *kfA2 = nullptr, *rkA = nullptr, *rkB = nullptr, *rkA2 = nullptr, *src = nullptr, *rsrc = nullptr;
    orbx_frame_desc d = desc_of(fA, (int)fA.kps.size(), boundsA, 8, true);
    MUST(orbx_keyframe_create_host(m, &d, S.inv_sigma2, &kfA));
    d = desc_of(fB, (int)fB.kps.size(), boundsB, 6, true);
    MUST(orbx_keyframe_create_host(m, &d, S.inv_sigma2, &kfB));
    d = desc_of(fA2, (int)fA2.kps.size(), boundsA, 6, false);
    MUST(orbx_keyframe_create_host(m, &d, S.inv_sigma2, &kfA2));
    d = desc_of(fRA, nlA, rigA, 8, false);
    MUST(orbx_keyframe_create_host_fisheye(m, &d, fRA.kps.data() + nlA, nrA, S.inv_sigma2, &rkA));
    d = desc_of(fRB, nlB, rigB, 6, false);
    MUST(orbx_keyframe_create_host_fisheye(m, &d, fRB.kps.data() + nlB, nrB, S.inv_sigma2, &rkB));
    d = desc_of(fRA2, nlA2, rigA, 6, false);
    MUST(orbx_keyframe_create_host_fisheye(m, &d, fRA2.kps.data() + nlA2, nrA2, S.inv_sigma2, &rkA2));
    d = desc_of(fSrc, kPoints, boundsA, 8, false);
    MUST(orbx_keyframe_create_host(m, &d, nullptr, &src));
    d = desc_of(fRigSrc, kSrcLeft, rigA, 8, false);
    MUST(orbx_keyframe_create_host_fisheye(m, &d, fRigSrc.kps.data() + kSrcLeft, kPoints - kSrcLeft, nullptr, &rsrc));
    orbx_frame *cur = nullptr, *rig = nullptr;
    d = desc_of(fCur, (int)fCur.kps.size(), boundsA, 8, false);
    MUST(orbx_frame_create(m, d.n, &cur));
    MUST(orbx_frame_load_host(cur, &d));
    d = desc_of(fRig, nlC, rigA, 8, false);
    std::vector<int32_t> l2r((size_t)nlC, -1), r2l((size_t)nrC, -1);
    MUST(orbx_frame_create(m, nlC + nrC, &rig));
    MUST(orbx_frame_load_host_fisheye(rig, &d, fRig.kps.data() + nlC, nrC, l2r.data(), r2l.data()));

    orbx_camera cam;
    memset(&cam, 0, sizeof(cam));
    cam.fx = cam.fy = kFx; cam.cx = kCx; cam.cy = kCy; cam.bf = kBf;
    const orbx_frame_pose poseA = A.pose(), poseB = B.pose();
    const float *pos = S.pos.data(), *nrm = S.normal.data(), *mn = S.min_dist.data(), *mx = S.max_dist.data();
    Uv frustum_pin, sim3_pin, reloc_pin, frustum_kb8, sim3_kb8, reloc_kb8;

    // ---- Frame::isInFrustum through views A and B
    for (int k = 0; k < 2; k++) {
        std::unique_ptr<uint8_t[]> iv(new uint8_t[np]);
        std::unique_ptr<float[]> px(new float[np]), py(new float[np]), pxr(new float[np]), dep(new float[np]), vc(new float[np]);
        std::unique_ptr<int32_t[]> lvl(new int32_t[np]);
        const int nlevels = k ? 6 : 8;
        const int rc = orbx_is_in_frustum(m, &cam, k ? &poseB : &poseA, k ? boundsB : boundsA, lsf, nlevels, 0.5f, kPoints, pos, nrm, mn, mx, iv.get(), px.get(),
                                          py.get(), pxr.get(), dep.get(), lvl.get(), vc.get());
        MUST(rc);
        printf("is_in_frustum view %d rc=%d", k, rc);
        sum("in_view", iv, np); sum("x", px, np); sum("y", py, np); sum("xr", pxr, np); sum("depth", dep, np); sum("level", lvl, np); sum("cos", vc, np);
        printf("\n");
        CHECK(verdicts_ok("is_in_frustum", FRUSTUM, 1, iv.get(), nullptr, 1));
        CHECK(lvl[0] == 0 && lvl[10] == nlevels - 1);   // the two clamps
        for (int i = 0; i < kPoints; i++)
            if (iv[(size_t)i] && i != 10) CHECK(lvl[(size_t)i] == S.level[(size_t)i]);
        if (k == 0) frustum_pin = keep(px.get(), py.get(), iv.get());
    }
    // ---- Frame::isInFrustumChecks through rig A's two cameras
    {
        const orbx_fisheye_view views[2] = {A.fisheye(), AR.fisheye()};
        std::unique_ptr<uint8_t[]> iv(new uint8_t[2 * np]);
        std::unique_ptr<float[]> px(new float[2 * np]), py(new float[2 * np]), dep(new float[2 * np]), vc(new float[2 * np]);
        std::unique_ptr<int32_t[]> lvl(new int32_t[2 * np]);
        const int rc = orbx_is_in_frustum_checks(m, views, 2, rigA, lsf, 8, 0.5f, kPoints, pos, nrm, mn, mx, iv.get(), px.get(), py.get(), dep.get(), lvl.get(),
                                                 vc.get());
        MUST(rc);
        printf("is_in_frustum_checks rc=%d", rc);
        sum("in_view", iv, 2 * np); sum("x", px, 2 * np); sum("y", py, 2 * np); sum("depth", dep, 2 * np); sum("level", lvl, 2 * np); sum("cos", vc, 2 * np);
        printf("\n");
        CHECK(verdicts_ok("is_in_frustum_checks", FRUSTUM, 2, iv.get(), nullptr, 1));
        CHECK(lvl[0] == 0 && lvl[10] == 7 && lvl[np] == 0 && lvl[np + 10] == 7);
        frustum_kb8 = keep(px.get(), py.get(), iv.get());
    }
    // ---- Fuse(pKF, vpMapPoints): key frames A and B in one call, a skip row each; a rig: two problems per key frame, one skip row per key frame
    for (int fisheye = 0; fisheye < 2; fisheye++) {
        const int sides = fisheye ? 2 : 1;
        const size_t total = 2 * (size_t)sides * np;
        std::unique_ptr<int32_t[]> bi(new int32_t[total]), bd(new int32_t[total]);
        std::unique_ptr<uint8_t[]> pr(new uint8_t[total]);
        int rc;
        if (fisheye) {
            orbx_keyframe *kfs[2] = {rkA, rkB};
            const orbx_fisheye_view views[4] = {A.fisheye(), AR.fisheye(), B.fisheye(), BR.fisheye()};
            rc = orbx_keyframe_fuse_map_points_fisheye(m, 2, kfs, views, 3.f, lsf, 0, kPoints, pos, nrm, mn, mx, S.desc.data(), skip.get(), bi.get(), bd.get(),
                                                       pr.get());
        } else {
            orbx_keyframe *kfs[2] = {kfA, kfB};
            const orbx_camera cams[2] = {cam, cam};
            const orbx_frame_pose poses[2] = {poseA, poseB};
            rc = orbx_keyframe_fuse_map_points(m, 2, kfs, cams, poses, 3.f, lsf, 0, kPoints, pos, nrm, mn, mx, S.desc.data(), skip.get(), bi.get(), bd.get(),
                                               pr.get());
        }
        MUST(rc);
        printf("keyframe_fuse_map_points%s rc=%d", fisheye ? "_fisheye" : "", rc);
        sum("best_idx", bi, total); sum("best_dist", bd, total); sum("projected", pr, total);
        printf("\n");
        CHECK(verdicts_ok("keyframe_fuse_map_points", KEYFRAME, 2 * sides, pr.get(), skip.get(), sides));
        int found = 0;
        for (size_t k = 0; k < total; k++) found += bi[k] >= 0;
        CHECK(found >= 20 * sides);   // the search behind the gates has something to find
    }
    // ---- the Sim3 searches: K = 2 (key frames A and A2, a skip row each) and K = 1 (key frame B), both projection forms
    for (int fisheye = 0; fisheye < 2; fisheye++)
        for (int form : {(int)ORBX_SIM3_PROJECT_CAMERA, (int)ORBX_SIM3_PROJECT_INVZ})
            for (int K = 2; K >= 1; K--) {
                orbx_keyframe *kfs[2] = {fisheye ? (K == 2 ? rkA : rkB) : (K == 2 ? kfA : kfB), fisheye ? rkA2 : kfA2};
                const size_t total = (size_t)K * np;
                int n[2] = {0, 0};
                std::unique_ptr<int32_t[]> match[2];
                int32_t *rows[2] = {nullptr, nullptr};
                for (int k = 0; k < K; k++) {
                    if (fisheye) { int nl = 0, nr = 0; MUST(orbx_keyframe_counts(kfs[k], &nl, &nr)); n[k] = nl + nr; }
                    else MUST(orbx_keyframe_count(kfs[k], &n[k]));
                    match[k].reset(new int32_t[(size_t)n[k]]);
                    rows[k] = match[k].get();
                }
                std::unique_ptr<int32_t[]> nm(new int32_t[(size_t)K]);
                std::unique_ptr<uint8_t[]> pr(new uint8_t[total]);
                std::unique_ptr<float[]> pu(new float[total]), pv(new float[total]);
                const uint8_t *sk = K == 2 ? skip.get() : skip.get() + np;   // K = 1: the second row alone
                int rc;
                if (fisheye) {
                    const orbx_fisheye_view views[2] = {K == 2 ? A.fisheye() : B.fisheye(), B.fisheye()};
                    rc = orbx_keyframe_search_by_projection_sim3_fisheye(m, K, kfs, views, 10.f, 1.f, lsf, form, kPoints, pos, nrm, mn, mx, S.desc.data(), sk, nullptr,
                                                                         rows, nm.get(), pr.get(), pu.get(), pv.get());
                } else {
                    const orbx_camera cams[2] = {cam, cam};
                    const orbx_frame_pose poses[2] = {K == 2 ? poseA : poseB, poseB};
                    rc = orbx_keyframe_search_by_projection_sim3(m, K, kfs, cams, poses, 10.f, 1.f, lsf, form, kPoints, pos, nrm, mn, mx, S.desc.data(), sk, nullptr,
                                                                 rows, nm.get(), pr.get(), pu.get(), pv.get());
                }
                MUST(rc);
                printf("keyframe_search_by_projection_sim3%s form %d K=%d rc=%d", fisheye ? "_fisheye" : "", form, K, rc);
                for (int k = 0; k < K; k++) sum("match", match[k], (size_t)n[k]);
                sum("nmatches", nm, (size_t)K); sum("projected", pr, total); sum("u", pu, total); sum("v", pv, total);
                printf("\n");
                CHECK(verdicts_ok("keyframe_search_by_projection_sim3", KEYFRAME, K, pr.get(), sk, 1));
                CHECK(nm[0] >= 10);
                if (K == 2 && form == ORBX_SIM3_PROJECT_CAMERA) (fisheye ? sim3_kb8 : sim3_pin) = keep(pu.get(), pv.get(), pr.get());
            }
    // ---- Relocalization's search from map ids: the monocular frame through view A, the rig frame through its left camera (view A as well)
    {
        orbx_map *map = nullptr;
        MUST(orbx_map_create(0, kCapacity, &map));
        std::vector<int32_t> slots(np), ids(np);
        for (int i = 0; i < kPoints; i++) slots[(size_t)i] = (i * 7 + 3) % kCapacity;
        MUST(orbx_map_update(m, map, kPoints, slots.data(), pos, nrm, mn, mx, S.desc.data()));
        std::unique_ptr<uint8_t[]> gone(new uint8_t[np]);
        for (int i = 0; i < kPoints; i++) { gone[(size_t)i] = i % kClasses == SKIP; ids[(size_t)i] = gone[(size_t)i] ? -1 : slots[(size_t)i]; }
        for (int fisheye = 0; fisheye < 2; fisheye++) {
            const size_t nf = fisheye ? (size_t)(nlC + nrC) : fCur.kps.size();
            std::unique_ptr<int32_t[]> match(new int32_t[nf]);
            std::unique_ptr<uint8_t[]> pr(new uint8_t[np]);
            std::unique_ptr<float[]> pu(new float[np]), pv(new float[np]);
            const orbx_fisheye_view view = A.fisheye();
            const int rc = fisheye ? orbx_frame_search_by_projection_keyframe_fisheye_map(m, rig, nullptr, &view, lsf, rsrc, map, kPoints, ids.data(), 10.f, 100.f, 1,
                                                                                          match.get(), pr.get(), pu.get(), pv.get())
                                   : orbx_frame_search_by_projection_keyframe_map(m, cur, nullptr, &cam, &poseA, lsf, src, map, kPoints, ids.data(), 10.f, 100.f, 1,
                                                                                  match.get(), pr.get(), pu.get(), pv.get());
            MUST(rc);
            printf("frame_search_by_projection_keyframe%s_map rc=%d", fisheye ? "_fisheye" : "", rc);
            sum("match", match, nf); sum("projected", pr, np); sum("u", pu, np); sum("v", pv, np);
            printf("\n");
            CHECK(verdicts_ok("frame_search_by_projection_keyframe_map", fisheye ? RELOC_KB8 : RELOC_PINHOLE, 1, pr.get(), gone.get(), 1));
            (fisheye ? reloc_kb8 : reloc_pin) = keep(pu.get(), pv.get(), pr.get());
        }
        orbx_map_destroy(map);
    }
    // ---- the cross-kernel contract: one (u, v) per view and point, whichever kernel projected it
    const int n_pin = trio_agrees("pinhole trio", frustum_pin, sim3_pin, reloc_pin), n_kb8 = trio_agrees("KannalaBrandt8 trio", frustum_kb8, sim3_kb8, reloc_kb8);
    CHECK(n_pin >= 20 && n_kb8 >= 20);
    printf("pinhole trio agrees on %d points, KannalaBrandt8 trio on %d\n", n_pin, n_kb8);

    orbx_frame_destroy(rig); orbx_frame_destroy(cur);
    for (orbx_keyframe *k : {kfA, kfB, kfA2, rkA, rkB, rkA2, src, rsrc}) orbx_keyframe_destroy(k);
    orbx_matcher_destroy(m);
    printf("project gates ok\n");
    return 0;
}
