// The Tracking searches that run from map ids (orbx_frame_track_last_frame_map, orbx_frame_search_by_projection_keyframe_map) against the flat handle
// forms fed with queries projected on the host as the adapters project them (orb_slam3_amd/cpp/ORBmatcher_slam.inl): return value, the match row
// (query indices mapped back to source features), projected and proj_u / proj_v bit for bit.  A 640 x 480 current frame of 400 synthetic features with
// mvuRight; a source of 601 features (three blocks of k_track_project, the last one partial) whose map points are back-projected from the current
// frame's features, some behind the camera, some outside the image, some outside their distance bounds, a sixth of the ids -1, a few source octaves out
// of range; the points live in a table of 2048 slots under shuffled ids.  Every caller array is a heap block of exactly the needed size, so a copy or
// a kernel write past one ends the run; refused calls must leave the transfer counters alone.  Then Relocalization's search on a fisheye-stereo rig
// (orbx_frame_search_by_projection_keyframe_fisheye_map) against orbx_frame_search_by_projection_window_fisheye: KannalaBrandt8::project on the host as
// the reference writes it, a rig key frame as the source, the match row padded with -1 beyond N_left.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt) and
// compiled with -fsanitize=address,undefined, as tests/cpp/map_check.cpp.  Prints "track map ok" and returns 0.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kLevels = 8, kFeatures = 400, kSource = 601, kCapacity = 2048;
constexpr float kW = 640.f, kH = 480.f, kF = 400.f, kCx = 320.f, kCy = 240.f, kBf = 40.f;

#define MUST(expr)                                                                   \
    do {                                                                             \
        const int r_ = (expr);                                                       \
        if (r_ < 0) { printf("%s: %d\n", #expr, r_); return 1; }                     \
    } while (0)
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

struct Scene {
    float scale[kLevels];
    std::vector<orbx_keypoint> kps, src;
    std::vector<uint8_t> desc, src_desc, mp_desc, has_obs, occupied;
    std::vector<float> u_right, pos, normal, min_dist, max_dist;
    std::vector<int32_t> ids;
    orbx_frame_pose pose;
    orbx_camera cam;
    orbx_frame_desc frame(bool source) const {
        orbx_frame_desc d;
        memset(&d, 0, sizeof(d));
        d.keypoints_un = source ? src.data() : kps.data(); d.descriptors = source ? src_desc.data() : desc.data(); d.n = source ? kSource : kFeatures;
        d.min_x = 0.f; d.max_x = kW; d.min_y = 0.f; d.max_y = kH;
        d.scale_factors = scale; d.nlevels = kLevels;
        d.u_right = source ? nullptr : u_right.data();
        return d;
    }
};

void make_scene(Scene &S) {
    std::mt19937 rng(57);
    auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    for (int l = 0; l < kLevels; l++) S.scale[l] = l ? S.scale[l - 1] * 1.2f : 1.f;
    memset(&S.pose, 0, sizeof(S.pose));
    S.pose.Rcw[0] = S.pose.Rcw[4] = S.pose.Rcw[8] = 1.f;
    S.pose.tcw[0] = 0.05f; S.pose.tcw[1] = -0.03f; S.pose.tcw[2] = 0.08f;
    for (int c = 0; c < 3; c++) S.pose.Ow[c] = -S.pose.tcw[c];
    memset(&S.cam, 0, sizeof(S.cam));
    S.cam.fx = S.cam.fy = kF; S.cam.cx = kCx; S.cam.cy = kCy; S.cam.bf = kBf;
    for (int i = 0; i < kFeatures; i++) {
        orbx_keypoint kp;
        memset(&kp, 0, sizeof(kp));
        kp.x = uni(20.f, kW - 20.f); kp.y = uni(20.f, kH - 20.f); kp.octave = (int)(rng() % (kLevels - 1));
        kp.size = 31.f * S.scale[kp.octave]; kp.angle = uni(0.f, 360.f); kp.response = 50.f; kp.class_id = -1;
        S.kps.push_back(kp);
        for (int b = 0; b < 32; b++) S.desc.push_back((uint8_t)rng());
        S.occupied.push_back(rng() % 25 == 0);
    }
    S.u_right.assign(kFeatures, -1.f);
    S.pos.resize(3 * (size_t)kSource); S.normal.assign(3 * (size_t)kSource, 0.f); S.min_dist.resize(kSource); S.max_dist.resize(kSource);
    S.mp_desc.resize(32 * (size_t)kSource); S.src_desc.assign(32 * (size_t)kSource, 0);
    for (int j = 0; j < kSource; j++) {
        const int f = j % kFeatures;
        const orbx_keypoint &kp = S.kps[(size_t)f];
        const float z = uni(2.f, 20.f);
        float pc[3] = {(kp.x + uni(-1.f, 1.f) - kCx) / kF * z, (kp.y + uni(-1.f, 1.f) - kCy) / kF * z, z};
        if (j % 17 == 0) for (float &c : pc) c = -c;   // behind the camera, the same (u, v)
        if (j % 23 == 0) pc[0] += 3.f * z;             // outside the image
        for (int c = 0; c < 3; c++) S.pos[3 * (size_t)j + c] = pc[c] - S.pose.tcw[c];
        const float d = std::sqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]);
        S.max_dist[(size_t)j] = j % 29 == 0 ? 0.5f * d : d * S.scale[kp.octave] * 0.98f;
        S.min_dist[(size_t)j] = j % 31 == 0 ? 2.f * S.max_dist[(size_t)j] : S.max_dist[(size_t)j] / S.scale[kLevels - 1];
        if (j < kFeatures && j % 17 != 0) S.u_right[(size_t)f] = (j % 2) ? kp.x - kBf / z + uni(-0.3f, 0.3f) : -1.f;
        for (int b = 0; b < 32; b++) S.mp_desc[32 * (size_t)j + b] = S.desc[32 * (size_t)f + b];
        for (int k = 0; k < 10; k++) { const unsigned bit = rng() % 256; S.mp_desc[32 * (size_t)j + bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
        orbx_keypoint sk = kp;
        sk.x = uni(1.f, kW - 1.f); sk.y = uni(1.f, kH - 1.f);
        sk.angle = std::fmod(kp.angle + (rng() % 10 ? 10.f + uni(-2.f, 2.f) : uni(0.f, 360.f)), 360.f);
        if (j % 41 == 0) sk.octave = (j % 82 == 0) ? -1 : kLevels + 1;   // out of range: projected, never searched
        S.src.push_back(sk);
        S.has_obs.push_back(rng() % 12 != 0);
    }
    std::vector<int32_t> all(kCapacity - 2);
    std::iota(all.begin(), all.end(), 1);
    std::shuffle(all.begin(), all.end(), rng);
    S.ids.assign(all.begin(), all.begin() + kSource - 2);
    S.ids.push_back(0); S.ids.push_back(kCapacity - 1);
    std::shuffle(S.ids.begin(), S.ids.end(), rng);
}

// what the host adapters compute per source feature with a point, one float operation at a time
struct Projection { float u, v, ur, invz, dist; bool inside; };
Projection project(const Scene &S, int j) {
    const float *R = S.pose.Rcw, *t = S.pose.tcw, *P = &S.pos[3 * (size_t)j];
    float pc[3];
    for (int r = 0; r < 3; r++) {
        const volatile float a = R[3 * r] * P[0], b = R[3 * r + 1] * P[1], c = R[3 * r + 2] * P[2];
        const volatile float ab = a + b, abc = ab + c;
        pc[r] = abc + t[r];
    }
    Projection o;
    o.invz = 1.0f / pc[2];
    const volatile float fxX = S.cam.fx * pc[0], fyY = S.cam.fy * pc[1];
    const volatile float qx = fxX / pc[2], qy = fyY / pc[2];
    o.u = qx + S.cam.cx; o.v = qy + S.cam.cy;
    const volatile float shift = S.cam.bf * o.invz;
    o.ur = o.u - shift;
    o.inside = !(o.u < 0.f || o.u > kW) && !(o.v < 0.f || o.v > kH);
    const volatile float d0 = P[0] - S.pose.Ow[0], d1 = P[1] - S.pose.Ow[1], d2 = P[2] - S.pose.Ow[2];
    const volatile float s0 = d0 * d0, s1 = d1 * d1, s2 = d2 * d2;
    const volatile float s01 = s0 + s1, s012 = s01 + s2;
    o.dist = std::sqrt((float)s012);
    return o;
}

// KannalaBrandt8::project (KannalaBrandt8.cpp:67-85): float arithmetic, cos / sin of the azimuth in double
void kb8(const float *p, float X, float Y, float Z, float *u, float *v) {
    const volatile float xx = X * X, yy = Y * Y;
    const volatile float x2y2 = xx + yy;
    const float theta = atan2f(sqrtf(x2y2), Z), psi = atan2f(Y, X);
    const volatile float t2 = theta * theta, t3 = theta * t2, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
    const volatile float a3 = p[4] * t3, a5 = p[5] * t5, a7 = p[6] * t7, a9 = p[7] * t9;
    const volatile float s1 = theta + a3, s2 = s1 + a5, s3 = s2 + a7, r = s3 + a9;
    const volatile float fr = p[0] * r, gr = p[1] * r;
    *u = (float)((double)fr * cos((double)psi) + (double)p[2]);
    *v = (float)((double)gr * sin((double)psi) + (double)p[3]);
}

bool same_counters(orbx_matcher *m, const int64_t *before) {
    int64_t now[6];
    return orbx_matcher_debug_transfers(m, now, 6) >= 0 && memcmp(now, before, sizeof(now)) == 0;
}

// the flat form's match row in query indices, mapped back to source features
bool same_matches(const int32_t *got, const int32_t *flat, const std::vector<int32_t> &sel, int n) {
    for (int i = 0; i < n; i++)
        if (got[i] != (flat[i] >= 0 ? sel[(size_t)flat[i]] : flat[i])) return false;
    return true;
}

}  // namespace

int main() {
    Scene S;
    make_scene(S);
    orbx_matcher *m = nullptr;
    MUST(orbx_matcher_create(0, &m));
    orbx_map *map = nullptr;
    MUST(orbx_map_create(0, kCapacity, &map));
    MUST(orbx_map_update(m, map, kSource, S.ids.data(), S.pos.data(), S.normal.data(), S.min_dist.data(), S.max_dist.data(), S.mp_desc.data()));
    std::vector<int32_t> ids = S.ids;
    for (int j = 0; j < kSource; j++)
        if (j % 6 == 5) ids[(size_t)j] = -1;   // no point / outlier / already found
    const orbx_frame_desc fd = S.frame(false), sd = S.frame(true);
    orbx_frame *cur = nullptr, *last = nullptr;
    MUST(orbx_frame_create(m, kFeatures, &cur));
    MUST(orbx_frame_load_host(cur, &fd));
    MUST(orbx_frame_create(m, kSource, &last));
    MUST(orbx_frame_load_host(last, &sd));
    orbx_keyframe *kf = nullptr;
    MUST(orbx_keyframe_create_host(m, &sd, nullptr, &kf));
    const float lsf = std::log(1.2f);

    // ---- TrackWithMotionModel's search: flat queries as the adapter builds them
    std::vector<int32_t> sel, q_octave;
    std::vector<float> q_u, q_v, q_ur, q_angle;
    std::vector<uint8_t> q_desc, q_obs, want_projected(kSource, 0);
    std::vector<float> want_u(kSource, 0.f), want_v(kSource, 0.f);
    int behind = 0, off_octave = 0;
    for (int j = 0; j < kSource; j++) {
        if (ids[(size_t)j] < 0) continue;
        const Projection p = project(S, j);
        want_u[(size_t)j] = p.u; want_v[(size_t)j] = p.v;
        if (p.invz < 0) { behind++; continue; }
        if (!p.inside) continue;
        want_projected[(size_t)j] = 1;
        const int o = S.src[(size_t)j].octave;
        if (o < 0 || o >= kLevels) { off_octave++; continue; }
        sel.push_back(j);
        q_u.push_back(p.u); q_v.push_back(p.v); q_ur.push_back(p.ur); q_octave.push_back(o); q_angle.push_back(S.src[(size_t)j].angle);
        q_desc.insert(q_desc.end(), S.mp_desc.begin() + 32 * (size_t)j, S.mp_desc.begin() + 32 * (size_t)j + 32);
        q_obs.push_back(S.has_obs[(size_t)j]);
    }
    CHECK(sel.size() > 300 && behind > 10 && off_octave > 3);
    for (int mode = 0; mode < 3; mode++) {
        // heap blocks of exactly the needed size
        std::unique_ptr<int32_t[]> got(new int32_t[kFeatures]), flat(new int32_t[kFeatures]);
        std::unique_ptr<uint8_t[]> pr(new uint8_t[kSource]);
        std::unique_ptr<float[]> pu(new float[kSource]), pv(new float[kSource]);
        const int na = orbx_frame_search_by_projection_frame(m, cur, S.occupied.data(), (int)sel.size(), q_u.data(), q_v.data(), q_ur.data(), q_octave.data(),
                                                             q_angle.data(), q_desc.data(), q_obs.data(), 7.f, mode, 1, flat.get());
        int64_t flat_t[6], new_t[6];
        MUST(orbx_matcher_debug_transfers(m, flat_t, 6));
        const int nb = orbx_frame_track_last_frame_map(m, cur, last, S.occupied.data(), &S.cam, &S.pose, map, kSource, ids.data(), S.has_obs.data(), 7.f, mode,
                                                       1, got.get(), pr.get(), pu.get(), pv.get());
        MUST(orbx_matcher_debug_transfers(m, new_t, 6));
        CHECK(na >= (mode == 0 ? 100 : 30) && nb == na);
        CHECK(same_matches(got.get(), flat.get(), sel, kFeatures));
        CHECK(!memcmp(pr.get(), want_projected.data(), kSource));
        for (int j = 0; j < kSource; j++)
            if (want_projected[(size_t)j]) CHECK(!memcmp(&pu[(size_t)j], &want_u[(size_t)j], 4) && !memcmp(&pv[(size_t)j], &want_v[(size_t)j], 4));
        CHECK(new_t[0] == 1 && new_t[1] == 1 && new_t[4] == 0 && flat_t[0] == 1 && new_t[2] < flat_t[2]);
    }

    // ---- Relocalization's search: no depth gate, the distance bounds, PredictScale
    std::vector<int32_t> sel3, q_min, q_max;
    std::vector<float> q_x, q_y, q_r, q_angle3;
    std::vector<uint8_t> q_desc3, want_projected3(kSource, 0);
    int behind_kept = 0, out_of_bounds = 0;
    for (int j = 0; j < kSource; j++) {
        if (ids[(size_t)j] < 0) continue;
        const Projection p = project(S, j);
        if (!p.inside) continue;
        const volatile float mn = 0.8f * S.min_dist[(size_t)j], mx = 1.2f * S.max_dist[(size_t)j];
        if (p.dist < mn || p.dist > mx) { out_of_bounds++; continue; }
        behind_kept += p.invz < 0;
        want_projected3[(size_t)j] = 1;
        const volatile float ratio = S.max_dist[(size_t)j] / p.dist;
        const volatile float lg = (float)std::log((double)ratio);
        int l = (int)std::ceil((float)(lg / lsf));
        l = l < 0 ? 0 : (l >= kLevels ? kLevels - 1 : l);
        sel3.push_back(j);
        q_x.push_back(p.u); q_y.push_back(p.v); q_r.push_back(10.f * S.scale[l]); q_min.push_back(l - 1); q_max.push_back(l + 1);
        q_angle3.push_back(S.src[(size_t)j].angle);
        q_desc3.insert(q_desc3.end(), S.mp_desc.begin() + 32 * (size_t)j, S.mp_desc.begin() + 32 * (size_t)j + 32);
    }
    CHECK(sel3.size() > 300 && behind_kept > 10 && out_of_bounds > 10);
    {
        orbx_frame *plain = nullptr;   // the flat window form has no right-coordinate gate to switch off: a frame without mvuRight
        orbx_frame_desc pd = fd;
        pd.u_right = nullptr;
        MUST(orbx_frame_create(m, kFeatures, &plain));
        MUST(orbx_frame_load_host(plain, &pd));
        std::unique_ptr<int32_t[]> got(new int32_t[kFeatures]), flat(new int32_t[kFeatures]);
        std::unique_ptr<uint8_t[]> pr(new uint8_t[kSource]);
        const int na = orbx_frame_search_by_projection_window(m, plain, S.occupied.data(), (int)sel3.size(), q_x.data(), q_y.data(), q_r.data(), q_min.data(),
                                                              q_max.data(), q_angle3.data(), q_desc3.data(), nullptr, 100.f, 1, flat.get());
        for (orbx_frame *f : {plain, cur}) {   // mvuRight on the current frame changes nothing
            const int nb = orbx_frame_search_by_projection_keyframe_map(m, f, S.occupied.data(), &S.cam, &S.pose, lsf, kf, map, kSource, ids.data(), 10.f, 100.f,
                                                                        1, got.get(), pr.get(), nullptr, nullptr);
            CHECK(na >= 100 && nb == na);
            CHECK(same_matches(got.get(), flat.get(), sel3, kFeatures));
            CHECK(!memcmp(pr.get(), want_projected3.data(), kSource));
        }
        orbx_frame_destroy(plain);
    }

    // ---- Relocalization's search on a fisheye-stereo rig: a 512 x 512 rig frame of 300 + 120 features, the left ones at the KannalaBrandt8
    // projections of 300 points (some slightly behind the camera on the image diagonal: kept, there is no depth gate); a rig key frame of 350 + 251
    // features as the source; the left camera only is searched and the match row is padded with -1 beyond N_left
    {
        constexpr int kNL = 300, kNR = 120, kSL = 350;
        const float prm[8] = {190.978477f, 190.973307f, 254.931706f, 256.897443f, 0.00348238940f, 0.000715034845f, -0.00205323614f, 0.000202936736f};
        std::mt19937 rng(91);
        auto uni = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
        std::vector<float> pos(3 * (size_t)kSource), nrm(3 * (size_t)kSource, 0.f), mn(kSource), mx(kSource);
        std::vector<uint8_t> mpd(32 * (size_t)kSource), rdesc(32 * (size_t)(kNL + kNR)), occ(kNL + kNR, 0);
        std::vector<orbx_keypoint> kl(kNL), kr(kNR);
        for (uint8_t &b : mpd) b = (uint8_t)rng();
        for (uint8_t &b : rdesc) b = (uint8_t)rng();
        std::vector<int> level(kSource);
        for (int j = 0; j < kSource; j++) {
            const float z = uni(2.f, 12.f);
            float pc[3] = {uni(-1.f, 1.f) * z, uni(-1.f, 1.f) * z, z};
            if (j % 19 == 0) { const float a = uni(2.f, 8.f); pc[0] = a; pc[1] = (j % 38 == 0) ? a : -a; pc[2] = -0.1f * a; }
            if (j % 23 == 0) pc[0] = 5.f * z;
            for (int c = 0; c < 3; c++) pos[3 * (size_t)j + c] = pc[c] - S.pose.tcw[c];
            const float d = std::sqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]);
            level[(size_t)j] = (int)(rng() % (kLevels - 1));
            mx[(size_t)j] = j % 29 == 0 ? 0.5f * d : d * S.scale[level[(size_t)j]] * 0.98f;
            mn[(size_t)j] = j % 31 == 0 ? 2.f * mx[(size_t)j] : mx[(size_t)j] / S.scale[kLevels - 1];
        }
        std::vector<int32_t> rids(S.ids);
        for (int j = 0; j < kSource; j++) rids[(size_t)j] = (S.ids[(size_t)j] + 977) % kCapacity;   // other slots than the first scene's
        std::sort(rids.begin(), rids.end());
        rids.erase(std::unique(rids.begin(), rids.end()), rids.end());
        CHECK((int)rids.size() == kSource);
        std::shuffle(rids.begin(), rids.end(), rng);
        MUST(orbx_map_update(m, map, kSource, rids.data(), pos.data(), nrm.data(), mn.data(), mx.data(), mpd.data()));
        std::vector<int32_t> ids3 = rids;
        for (int j = 0; j < kSource; j++) if (j % 6 == 5) ids3[(size_t)j] = -1;
        // host projection, as relocalizationQueries
        std::vector<int32_t> sel, qmin, qmax;
        std::vector<float> qx, qy, qr, qa;
        std::vector<uint8_t> qd, want_pr(kSource, 0);
        std::vector<float> su(kSource, 0.f), sv(kSource, 0.f);
        std::vector<orbx_keypoint> src = S.src;   // rows [0, kSL) the left camera's, the rest the right camera's
        int kept_behind = 0;
        for (int j = 0; j < kSource; j++) {
            const float *P = &pos[3 * (size_t)j];
            float pc[3];
            for (int r = 0; r < 3; r++) {
                const volatile float a = S.pose.Rcw[3 * r] * P[0], b = S.pose.Rcw[3 * r + 1] * P[1], c = S.pose.Rcw[3 * r + 2] * P[2];
                const volatile float ab = a + b, abc = ab + c;
                pc[r] = abc + S.pose.tcw[r];
            }
            float u, v;
            kb8(prm, pc[0], pc[1], pc[2], &u, &v);
            su[(size_t)j] = u; sv[(size_t)j] = v;
            if (j < kNL) {   // the rig frame's left feature j sits at the projection of point j
                orbx_keypoint kp;
                memset(&kp, 0, sizeof(kp));
                kp.x = std::min(std::max(u + uni(-0.8f, 0.8f), 0.5f), 511.5f); kp.y = std::min(std::max(v + uni(-0.8f, 0.8f), 0.5f), 511.5f);
                kp.octave = level[(size_t)j]; kp.size = 31.f; kp.angle = std::fmod(src[(size_t)j].angle + 350.f, 360.f); kp.response = 50.f; kp.class_id = -1;
                kl[(size_t)j] = kp;
                memcpy(&rdesc[32 * (size_t)j], &mpd[32 * (size_t)j], 32);
                for (int k = 0; k < 10; k++) { const unsigned bit = rng() % 256; rdesc[32 * (size_t)j + bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
                occ[(size_t)j] = rng() % 25 == 0;
            }
            if (ids3[(size_t)j] < 0) { su[(size_t)j] = sv[(size_t)j] = 0.f; continue; }
            if (u < 0.f || u > 512.f || v < 0.f || v > 512.f) continue;
            const volatile float d0 = P[0] - S.pose.Ow[0], d1 = P[1] - S.pose.Ow[1], d2 = P[2] - S.pose.Ow[2];
            const volatile float s0 = d0 * d0, s1 = d1 * d1, s2 = d2 * d2, s01 = s0 + s1, s012 = s01 + s2;
            const float dist = std::sqrt((float)s012);
            const volatile float lo = 0.8f * mn[(size_t)j], hi = 1.2f * mx[(size_t)j];
            if (dist < lo || dist > hi) continue;
            kept_behind += pc[2] < 0.f;
            want_pr[(size_t)j] = 1;
            const volatile float ratio = mx[(size_t)j] / dist;
            const volatile float lg = (float)std::log((double)ratio);
            int l = (int)std::ceil((float)(lg / lsf));
            l = l < 0 ? 0 : (l >= kLevels ? kLevels - 1 : l);
            sel.push_back(j);
            qx.push_back(u); qy.push_back(v); qr.push_back(10.f * S.scale[l]); qmin.push_back(l - 1); qmax.push_back(l + 1);
            qa.push_back(j < kSL ? src[(size_t)j].angle : 0.f);
            qd.insert(qd.end(), mpd.begin() + 32 * (size_t)j, mpd.begin() + 32 * (size_t)j + 32);
        }
        CHECK(sel.size() > 300 && kept_behind >= 5);
        for (int i = 0; i < kNR; i++) {
            orbx_keypoint kp;
            memset(&kp, 0, sizeof(kp));
            kp.x = uni(1.f, 511.f); kp.y = uni(1.f, 511.f); kp.octave = (int)(rng() % kLevels); kp.size = 31.f; kp.response = 50.f; kp.class_id = -1;
            kr[(size_t)i] = kp;
        }
        orbx_frame_desc ld;
        memset(&ld, 0, sizeof(ld));
        ld.keypoints_un = kl.data(); ld.descriptors = rdesc.data(); ld.n = kNL; ld.max_x = 512.f; ld.max_y = 512.f; ld.scale_factors = S.scale; ld.nlevels = kLevels;
        std::vector<int32_t> l2r(kNL, -1), r2l(kNR, -1);
        orbx_frame *rigf = nullptr;
        MUST(orbx_frame_create(m, kNL + kNR, &rigf));
        MUST(orbx_frame_load_host_fisheye(rigf, &ld, kr.data(), kNR, l2r.data(), r2l.data()));
        orbx_frame_desc sd3;
        memset(&sd3, 0, sizeof(sd3));
        sd3.keypoints_un = src.data(); sd3.descriptors = S.src_desc.data(); sd3.n = kSL; sd3.max_x = 512.f; sd3.max_y = 512.f; sd3.scale_factors = S.scale;
        sd3.nlevels = kLevels;
        orbx_keyframe *rkf = nullptr;
        MUST(orbx_keyframe_create_host_fisheye(m, &sd3, src.data() + kSL, kSource - kSL, nullptr, &rkf));
        orbx_fisheye_view view;
        memcpy(view.R, S.pose.Rcw, sizeof(view.R)); memcpy(view.t, S.pose.tcw, sizeof(view.t)); memcpy(view.twc, S.pose.Ow, sizeof(view.twc));
        memcpy(view.params, prm, sizeof(prm));
        // heap blocks of exactly the needed size: N = N_left + N_right entries of match, n_ids of the rest
        std::unique_ptr<int32_t[]> got(new int32_t[kNL + kNR]), flat(new int32_t[kNL + kNR]);
        std::unique_ptr<uint8_t[]> pr(new uint8_t[kSource]);
        std::unique_ptr<float[]> pu(new float[kSource]), pv(new float[kSource]);
        const int na = orbx_frame_search_by_projection_window_fisheye(m, rigf, occ.data(), (int)sel.size(), qx.data(), qy.data(), qr.data(), qmin.data(),
                                                                      qmax.data(), qa.data(), qd.data(), nullptr, 100.f, 1, flat.get());
        const int nb = orbx_frame_search_by_projection_keyframe_fisheye_map(m, rigf, occ.data(), &view, lsf, rkf, map, kSource, ids3.data(), 10.f, 100.f, 1,
                                                                            got.get(), pr.get(), pu.get(), pv.get());
        int64_t t[6];
        MUST(orbx_matcher_debug_transfers(m, t, 6));
        CHECK(na >= 100 && nb == na && t[0] == 1 && t[1] == 1 && t[4] == 0);
        CHECK(same_matches(got.get(), flat.get(), sel, kNL + kNR));
        for (int i = kNL; i < kNL + kNR; i++) CHECK(got[(size_t)i] == -1);
        CHECK(!memcmp(pr.get(), want_pr.data(), kSource));
        for (int j = 0; j < kSource; j++)
            if (want_pr[(size_t)j]) CHECK(!memcmp(&pu[(size_t)j], &su[(size_t)j], 4) && !memcmp(&pv[(size_t)j], &sv[(size_t)j], 4));
        CHECK(orbx_frame_search_by_projection_keyframe_fisheye_map(m, rigf, nullptr, &view, lsf, kf, map, kSource, ids3.data(), 10.f, 100.f, 1, got.get(),
                                                                   nullptr, nullptr, nullptr) == ORBX_E_BAD_ARG);   // a monocular key frame
        CHECK(orbx_frame_search_by_projection_keyframe_map(m, rigf, nullptr, &S.cam, &S.pose, lsf, kf, map, kSource, ids3.data(), 10.f, 100.f, 1, got.get(),
                                                           nullptr, nullptr, nullptr) == ORBX_E_BAD_ARG);           // a rig frame to the monocular form
        orbx_keyframe_destroy(rkf);
        orbx_frame_destroy(rigf);
    }

    // ---- refusals leave the counters alone
    int64_t before[6];
    MUST(orbx_matcher_debug_transfers(m, before, 6));
    std::unique_ptr<int32_t[]> out(new int32_t[kFeatures]);
    std::vector<int32_t> bad = ids;
    bad[0] = kCapacity;
    CHECK(orbx_frame_track_last_frame_map(m, cur, last, nullptr, &S.cam, &S.pose, map, kSource, bad.data(), nullptr, 7.f, 0, 1, out.get(), nullptr, nullptr,
                                          nullptr) == ORBX_E_BAD_ARG);
    bad[0] = -2;
    CHECK(orbx_frame_search_by_projection_keyframe_map(m, cur, nullptr, &S.cam, &S.pose, lsf, kf, map, kSource, bad.data(), 10.f, 100.f, 1, out.get(), nullptr,
                                                       nullptr, nullptr) == ORBX_E_BAD_ARG);
    CHECK(orbx_frame_track_last_frame_map(m, cur, cur, nullptr, &S.cam, &S.pose, map, kFeatures, ids.data(), nullptr, 7.f, 0, 1, out.get(), nullptr, nullptr,
                                          nullptr) == ORBX_E_BAD_ARG);
    CHECK(orbx_frame_track_last_frame_map(m, cur, last, nullptr, &S.cam, &S.pose, map, kSource - 1, ids.data(), nullptr, 7.f, 0, 1, out.get(), nullptr, nullptr,
                                          nullptr) == ORBX_E_BAD_ARG);
    CHECK(same_counters(m, before));

    orbx_keyframe_destroy(kf);
    orbx_frame_destroy(last);
    orbx_frame_destroy(cur);
    orbx_map_destroy(map);
    orbx_matcher_destroy(m);
    printf("track map ok\n");
    return 0;
}
