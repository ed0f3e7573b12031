// orbx_matcher.hip -- host side of the matchers: per-thread context (own HIP stream + grow-on-demand device
// scratch), upload / launch / download for the host-pointer entry points, and the device-resident batched
// frame-to-frame matcher.  See include/orbx.h for the reference functions each entry point replaces.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "matcher_kernels.hip.h"
#include "geometry_kernels.hip.h"
#include "bow_database_kernels.hip.h"
#include "extractor_state.h"
#include "matcher_context.h"

static_assert(sizeof(orbx_keypoint) == 28, "the rows every matcher uploads and the kernels index");
static_assert(sizeof(orbx::FisheyeView) == sizeof(orbx_fisheye_view), "the views every fisheye entry point hands to its kernels as they come");

using namespace orbx;

namespace {

constexpr int kMaxResolveFeatures = ORBX_MAX_FRAME_FEATURES;  // claim (4 B) + angle (4 B) + occ (1 B) + octave (1 B) per feature must fit the 160 KB LDS (16000 x 10 + 200 B)
inline size_t resolve_lds_bytes(int n) { return (size_t)n * 10 + 64; }   // k_greedy_resolve: claim u32 + angle f32 + occ u8 + octave u8 per feature
// The replay of SearchByProjection's query loop.  Single calls and the batched map-point search: k_resolve_wide_t, a workgroup of 4 waves per problem
// (M1 10 000 points 241 -> 197 us per call, M2 132 -> 94, M3 111 -> 85: profiles/r06_h_resolve_ab.txt).  The frame-to-frame matcher of a BATCH keeps the
// one-wave k_greedy_resolve_t: 255 problems side by side, 75 against 83 us serialized, and a quarter of the wave slots beside the next batch's extraction.
// ORBX_RESOLVE_WAVES = 1 / 2 / 4 / 8 forces one form everywhere (A/B).
template <int WAVES, bool BRUTE>
inline int launch_resolve_wide(int np, size_t lds, hipStream_t st, const WindowProblem *dP, const ResolveProblem *dR, const GridParams &g, int cap) {
    if (lds > 64 * 1024) ORBX_HIP(hipFuncSetAttribute((const void *)k_resolve_wide_t<WAVES, BRUTE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_resolve_wide_t<WAVES, BRUTE>), dim3(np), dim3(64 * WAVES), lds, st, dP, dR, g, cap);
    return ORBX_OK;
}
template <bool BRUTE>
inline int launch_resolve(int np, hipStream_t st, const WindowProblem *dP, const ResolveProblem *dR, const GridParams &g, int cap, int nq_max, int default_waves) {
    static const int waves_env = [] { const char *v = getenv("ORBX_RESOLVE_WAVES"); return v ? atoi(v) : 0; }();
    const int waves = nq_max > 65535 ? 1 : waves_env > 0 ? waves_env : default_waves;   // the wide form carries the query index of a rotation entry in 16 bits
    const size_t lds = resolve_lds_bytes(cap);
    if (waves == 2) return launch_resolve_wide<2, BRUTE>(np, lds, st, dP, dR, g, cap);
    if (waves == 8) return launch_resolve_wide<8, BRUTE>(np, lds, st, dP, dR, g, cap);
    if (waves != 1) return launch_resolve_wide<4, BRUTE>(np, lds, st, dP, dR, g, cap);
    if (lds > 64 * 1024) ORBX_HIP(hipFuncSetAttribute((const void *)k_greedy_resolve_t<BRUTE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_greedy_resolve_t<BRUTE>, dim3(np), dim3(64), lds, st, dP, dR, g, cap);
    return ORBX_OK;
}
#define ORBX_LAUNCH_GRID_BUILD(grid, block, lds, stream, ...) hipLaunchKernelGGL(k_grid_build, grid, block, lds, stream, __VA_ARGS__)
// k_window_best2: 8 lanes per query (a window of the bench's matchers holds 1 - 10 candidates: 16 -> 8 lanes, 74 -> 59 us in round 4; 4 like 8).
// nq = queries per problem, np = problems.  From 8 problems on the launch is XCD-aware like the extractor's (extractor_kernels.hip.h, xcd_grid): x = XCD,
// problem = 8 z + x, so that ALL workgroups of a problem -- they share the frame's grid, keypoints and descriptors -- run on one XCD and fetch that frame
// into ONE L2 (round 4 spread a problem's query blocks over the eight XCDs: 134 MB of HBM reads per launch for 35 MB of data).
#define ORBX_LAUNCH_WINDOW_BEST2(nq, np, stream, ...)                                                                                          \
    do {                                                                                                                                       \
        const int np_ = (np), nb_ = ((nq) + 31) / 32;                                                                                          \
        const dim3 grid_ = np_ >= 8 ? dim3(8, (unsigned)nb_, (unsigned)((np_ + 7) / 8)) : dim3(1, (unsigned)nb_, (unsigned)np_);               \
        hipLaunchKernelGGL(k_window_best2_t<8>, grid_, dim3(256), 0, stream, __VA_ARGS__, np_);                                                \
    } while (0)

}  // namespace


// ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>) resident on the device
struct orbx_vocabulary {
    int device = 0, k = 0, L = 0, n_nodes = 0;
    int32_t *child_ptr = nullptr, *child_idx = nullptr, *word_id = nullptr;
    uint8_t *node_desc = nullptr;
    int max_word = -1;                 // the largest word id of the tree
    uint8_t *word_pos = nullptr;       // [n_words] m_words[id]->weight > 0 (orbx_vocabulary_set_word_weights); NULL: no word is stopped
    double *weight = nullptr;          // [n_words] m_words[id]->weight as given (k_bow_vector's tf-idf); NULL with word_pos
    int n_words = 0;
    std::vector<int> depth_nodes;      // nodes at depth d of the tree (root: depth 0), counted once at creation: the host's bound on a FeatureVector's node count
    int node_bound(int levelsup) const {   // node ids of TemplatedVocabulary::transform at level L - levelsup: the nodes of that depth, or node 0 (a leaf above it / a level <= 0)
        const int d = L - levelsup;
        return 1 + ((d > 0 && d < (int)depth_nodes.size()) ? depth_nodes[(size_t)d] : 0);
    }
};

extern "C" {

int orbx_matcher_create(int device, orbx_matcher **out) {
    if (!out) return ORBX_E_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        set_error("no usable HIP device (liborbx has no CPU fallback)");
        return ORBX_E_NO_DEVICE;
    }
    ORBX_HIP(hipSetDevice(device));
    orbx_matcher *m = new orbx_matcher();
    m->device = device;
    hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); delete m; return ORBX_E_HIP; }
    const char *dma = getenv("ORBX_MATCHER_DMA");
    m->kernel_xfer = !(dma && dma[0] == '1');
    const char *br = getenv("ORBX_MATCHER_BRUTE");
    m->brute_windows = !(br && br[0] == '0');
    *out = m;
    return ORBX_OK;
}

int orbx_matcher_debug_transfers(const orbx_matcher *m, int64_t *out, int cap) {
    if (!m || !out || cap < 4) return ORBX_E_BAD_ARG;
    const int n = cap >= 6 ? 6 : 4;
    for (int i = 0; i < n; i++) out[i] = m->xfers[i];
    return n;
}

int orbx_matcher_debug_replay_stats(const orbx_matcher *m, int32_t *out3) {
    if (!m || !out3) return ORBX_E_BAD_ARG;
    for (int k = 0; k < 3; k++) out3[k] = m->replay_stats[k];
    return 3;
}

void orbx_matcher_destroy(orbx_matcher *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->stream) { (void)hipStreamSynchronize(m->stream); (void)hipStreamDestroy(m->stream); }
    if (m->arena.base) (void)hipFree(m->arena.base);
    if (m->stage.base) (void)hipHostFree(m->stage.base);
    if (m->mirror.base) (void)hipHostFree(m->mirror.base);
    delete m;
}


int orbx_hamming_csr(orbx_matcher *m, const uint8_t *q, int nq, const uint8_t *t, int nt, const int32_t *row_ptr,
                     const int32_t *cand, uint16_t *dist_out) {
    if (!m || nq < 0 || nt < 0 || (nq > 0 && (!q || !row_ptr))) return ORBX_E_BAD_ARG;
    if (nq == 0) return ORBX_OK;
    const int nnz = row_ptr[nq];
    if (nnz <= 0) return ORBX_OK;
    if (!t || !cand || !dist_out) return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(m->device));
    uint8_t *dq, *dt;
    int32_t *drp, *dc;
    uint16_t *dd;
    ORBX_TRY(m->carve([&](Carve &A) {
        dq = A.up(q, (size_t)nq * 32); dt = A.up(t, (size_t)nt * 32);
        drp = A.up(row_ptr, (size_t)nq + 1); dc = A.up(cand, (size_t)nnz);
        dd = A.take<uint16_t>(nnz);
    }));
    hipLaunchKernelGGL(k_hamming_csr, dim3((nq + 3) / 4), dim3(256), 0, m->exec(), dq, nq, dt, drp, dc, dd);
    ORBX_TRY(m->d2h(dist_out, dd, 2 * (size_t)nnz));
    ORBX_TRY(m->sync_and_deliver());
    return ORBX_OK;
}

int orbx_hamming_best2_csr(orbx_matcher *m, const uint8_t *q, int nq, const uint8_t *t, int nt, const int32_t *row_ptr,
                           const int32_t *cand, int32_t *best_pos, int32_t *best_dist, int32_t *second_pos,
                           int32_t *second_dist) {
    if (!m || nq < 0 || nt < 0 || (nq > 0 && (!q || !row_ptr))) return ORBX_E_BAD_ARG;
    if (nq == 0) return ORBX_OK;
    const int nnz = row_ptr[nq];
    ORBX_HIP(hipSetDevice(m->device));
    uint8_t *dq, *dt;
    int32_t *drp, *dc, *o[4];
    ORBX_TRY(m->carve([&](Carve &A) {
        dq = A.up(q, (size_t)nq * 32); dt = A.up(t, (size_t)nt * 32, 32);
        drp = A.up(row_ptr, (size_t)nq + 1); dc = A.up(cand, (size_t)nnz, 1);
        for (int k = 0; k < 4; k++) o[k] = A.take<int32_t>(nq);
    }));
    hipLaunchKernelGGL(k_hamming_best2_csr, dim3((nq + 3) / 4), dim3(256), 0, m->exec(), dq, nq, dt, drp, dc, o[0], o[1], o[2], o[3]);
    int32_t *host[4] = {best_pos, best_dist, second_pos, second_dist};
    for (int k = 0; k < 4; k++) if (host[k]) ORBX_TRY(m->d2h(host[k], o[k], 4 * (size_t)nq));
    ORBX_TRY(m->sync_and_deliver());
    return ORBX_OK;
}

int orbx_knn2(orbx_matcher *m, const uint8_t *q, int nq, const uint8_t *t, int nt, int32_t *idx, int32_t *dist) {
    if (!m || nq < 0 || nt < 0 || (nq > 0 && (!q || !idx || !dist))) return ORBX_E_BAD_ARG;
    if (nq == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(m->device));
    uint8_t *dq, *dt;
    int32_t *di, *dd;
    ORBX_TRY(m->carve([&](Carve &A) {
        dq = A.up(q, (size_t)nq * 32); dt = A.up(t, (size_t)nt * 32, 32);
        di = A.take<int32_t>(2 * (size_t)nq); dd = A.take<int32_t>(2 * (size_t)nq);
    }));
    hipLaunchKernelGGL(k_knn2, dim3((nq + 3) / 4), dim3(256), 0, m->exec(), dq, nq, dt, nt, di, dd, KnnFrames{});
    ORBX_TRY(m->d2h(idx, di, 8 * (size_t)nq)); ORBX_TRY(m->d2h(dist, dd, 8 * (size_t)nq));
    ORBX_TRY(m->sync_and_deliver());
    return ORBX_OK;
}

int orbx_stereo_rowband(orbx_matcher *m, const orbx_keypoint *kl, const uint8_t *dl, int nl, const orbx_keypoint *kr,
                        const uint8_t *dr, int nr, const float *scale, int nlevels, int n_rows, float min_d, float max_d,
                        int32_t *best_idx_r, int32_t *best_dist) {
    if (!m || nl < 0 || nr < 0 || nlevels <= 0 || !scale) return ORBX_E_BAD_ARG;
    if (nl == 0) return ORBX_OK;
    if (!kl || !dl || !best_idx_r || !best_dist) return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(m->device));
    orbx_keypoint *dkl, *dkr;
    uint8_t *ddl, *ddr;
    float *dsc;
    int32_t *dbi, *dbd;
    ORBX_TRY(m->carve([&](Carve &A) {
        dkl = A.up(kl, (size_t)nl); dkr = A.up(kr, (size_t)nr, 1);
        ddl = A.up(dl, 32 * (size_t)nl); ddr = A.up(dr, 32 * (size_t)nr, 32);
        dsc = A.up(scale, (size_t)nlevels);
        dbi = A.take<int32_t>(nl); dbd = A.take<int32_t>(nl);
    }));
    hipLaunchKernelGGL(k_stereo_rowband, dim3((nl + 3) / 4), dim3(256), 0, m->exec(), dkl, ddl, nl, dkr, ddr, nr, dsc, n_rows, min_d,
                       max_d, dbi, dbd);
    ORBX_TRY(m->d2h(best_idx_r, dbi, 4 * (size_t)nl)); ORBX_TRY(m->d2h(best_dist, dbd, 4 * (size_t)nl));
    ORBX_TRY(m->sync_and_deliver());
    return ORBX_OK;
}

// StereoBatch's row index parameters for an image of n_rows rows and pyramid scale factors sc[0 .. nl)
static void stereo_index_params(StereoBatch &S, int n_rows, const float *sc, int nl) {
    S.band = (int)ceilf(2.0f * *std::max_element(sc, sc + nl)) + 1;
    S.row_shift = 0;
    while (((n_rows - 1) >> S.row_shift) + 1 > kStereoIndexMaxBuckets) S.row_shift++;
    S.n_buckets = ((n_rows - 1) >> S.row_shift) + 1;
}

// Frame::ComputeStereoMatches (Frame.cc:811-981): device Hamming stage, host SAD refinement on the host-resident
// pyramid (mvImagePyramid is host memory at this boundary), host median rejection.
int orbx_compute_stereo_matches(orbx_matcher *m, const orbx_keypoint *kl, const uint8_t *dl, int N, const orbx_keypoint *kr,
                                const uint8_t *dr, int Nr, const float *scale_factors, const float *inv_scale_factors,
                                int nlevels, const uint8_t *const *pyr_left, const uint8_t *const *pyr_right, const int32_t *pyr_w,
                                const int32_t *pyr_h, const size_t *pyr_stride, float bf, float b, float *u_right, float *depth) {
    if (!m || !u_right || !depth || N < 0 || Nr < 0 || !pyr_h || !pyr_w || !pyr_stride || !pyr_left || !pyr_right || nlevels <= 0 ||
        !scale_factors || !inv_scale_factors || !(b > 0.f))
        return ORBX_E_BAD_ARG;
    for (int i = 0; i < N; i++) { u_right[i] = -1.0f; depth[i] = -1.0f; }
    if (N == 0 || Nr == 0) return 0;
    ORBX_HIP(hipSetDevice(m->device));
    // the same three kernels as the device-resident batch (Hamming row band, SAD + parabola, median rejection) on a batch
    // of one: the two pyramids are uploaded as slabs addressed like the extractor's (level origin = off + kEdge rows + kRoiX)
    const size_t lead = ((size_t)kEdge * 8192 + kRoiX + 255) & ~(size_t)255;
    std::vector<LevelInfo> lv(nlevels);
    size_t slab = lead;
    for (int l = 0; l < nlevels; l++) {
        if (pyr_stride[l] > 8192 || pyr_w[l] <= 0 || pyr_h[l] <= 0) return ORBX_E_BAD_ARG;
        memset(&lv[l], 0, sizeof(LevelInfo));
        lv[l].w = pyr_w[l]; lv[l].h = pyr_h[l]; lv[l].pitch = (int32_t)pyr_stride[l];
        lv[l].off = slab - (size_t)kEdge * pyr_stride[l] - kRoiX;   // so that the kernels' (kEdge + y) * pitch + kRoiX + x lands on (x, y)
        slab += (pyr_stride[l] * (size_t)pyr_h[l] + 255) & ~(size_t)255;
    }
    StereoBatch S;
    memset(&S, 0, sizeof(S));
    stereo_index_params(S, pyr_h[0], scale_factors, nlevels);
    const int32_t cnts[2] = {N, Nr};
    uint8_t *dL, *dR;
    float *dsc;
    int32_t *dcnt, *drp;
    uint4 *den;
    ORBX_TRY(m->carve([&](Carve &A) {
        dL = A.take<uint8_t>(slab); dR = A.take<uint8_t>(slab);
        S.kl = A.up(kl, (size_t)N); S.kr = A.up(kr, (size_t)Nr);
        S.dl = A.up(dl, 32 * (size_t)N); S.dr = A.up(dr, 32 * (size_t)Nr);
        S.lvL = S.lvR = A.up(lv.data(), (size_t)nlevels);
        dsc = A.take<float>(2 * (size_t)nlevels);
        dcnt = A.up(cnts, 2, 2);
        S.best_idx = A.take<int32_t>(N); S.best_dist = A.take<int32_t>(N);
        S.u_right = A.take<float>(N); S.depth = A.take<float>(N); S.nmatches = A.take<int32_t>(4); S.sad = A.take<int32_t>(N);   // the three downloads side by side: one DMA
        drp = A.take<int32_t>((size_t)S.n_buckets + 1);
        den = A.take<uint4>(Nr);
    }));
    for (int l = 0; l < nlevels; l++) {
        const size_t o = lv[l].off + (size_t)kEdge * pyr_stride[l] + kRoiX, bytes = pyr_stride[l] * (size_t)(pyr_h[l] - 1) + pyr_w[l];
        ORBX_TRY(m->h2d(dL + o, pyr_left[l], bytes));
        ORBX_TRY(m->h2d(dR + o, pyr_right[l], bytes));
    }
    ORBX_TRY(m->h2d(dsc, scale_factors, 4 * (size_t)nlevels)); ORBX_TRY(m->h2d(dsc + nlevels, inv_scale_factors, 4 * (size_t)nlevels));
    S.nl = dcnt; S.nr = dcnt + 1; S.capL = N; S.capR = Nr;
    S.pyrL = dL; S.pyrR = dR; S.pyr_frame_L = 0; S.pyr_frame_R = 0;
    S.scale = dsc; S.inv_scale = dsc + nlevels; S.n_rows = pyr_h[0]; S.bf = bf; S.b = b;
    S.row_ptr = drp; S.row_ent = den;
    hipLaunchKernelGGL(k_stereo_row_index, dim3(1), dim3(256), 4 * ((size_t)S.n_buckets + 1) + 1024, m->exec(), S, drp, den);
    hipLaunchKernelGGL(k_stereo_rowband_batch, dim3((N + 15) / 16, 1), dim3(256), 0, m->exec(), S);
    hipLaunchKernelGGL(k_stereo_sad, dim3((N + 15) / 16, 1), dim3(256), 0, m->exec(), S);
    hipLaunchKernelGGL(k_stereo_reject, dim3(1), dim3(256), 0, m->exec(), S);
    ORBX_HIP(hipGetLastError());
    int32_t nm = 0;
    ORBX_TRY(m->d2h(u_right, S.u_right, 4 * (size_t)N)); ORBX_TRY(m->d2h(depth, S.depth, 4 * (size_t)N)); ORBX_TRY(m->d2h(&nm, S.nmatches, 4));
    ORBX_TRY(m->sync_and_deliver());
    return nm;
}

}  // extern "C"

namespace {

// Result rows on their way to the caller of a call on a resident handle (a frame handle, a key frame) whose N may still be on the device only.
// A block: row k = nc int32 at src + k * nc on the device, bound for dst + k * stride (dst NULL: not wanted).  N known (nc = the entries the caller
// gets): each row goes straight to the caller.  N pending (nc = the capacity the rows are sized by): each block comes down whole into `land`, one block
// behind the other, and take() hands the first `count` entries of every row out once the call knows N.  A call names all its blocks at once: `land`
// must not move while a download into it is on its way.
struct Rows { const int32_t *src; int k_rows, nc; int32_t *dst; size_t stride; };
struct PendingRows {
    orbx_matcher *m;
    std::vector<int32_t> &land;
    bool pending;
    int fetch(const Rows *blocks, int n_blocks = 1) {
        size_t total = 0, at = 0;
        for (int b = 0; b < n_blocks; b++) total += (size_t)blocks[b].k_rows * blocks[b].nc;
        if (pending && land.size() < total) land.resize(total);
        for (int b = 0; b < n_blocks; b++) {
            const Rows &r = blocks[b];
            if (pending) ORBX_TRY(m->d2h(land.data() + at, r.src, 4 * (size_t)r.k_rows * r.nc));
            for (int k = 0; !pending && r.dst && k < r.k_rows; k++) ORBX_TRY(m->d2h(r.dst + k * r.stride, r.src + (size_t)k * r.nc, 4 * (size_t)r.nc));
            at += (size_t)r.k_rows * r.nc;
        }
        return ORBX_OK;
    }
    void take(const Rows *blocks, int n_blocks, int count) const {
        size_t at = 0;
        for (int b = 0; b < n_blocks; b++) {
            const Rows &r = blocks[b];
            for (int k = 0; count > 0 && r.dst && k < r.k_rows; k++) memcpy(r.dst + k * r.stride, land.data() + at + (size_t)k * r.nc, 4 * (size_t)count);
            at += (size_t)r.k_rows * r.nc;
        }
    }
};

// What ComputeBoW leaves on a handle, of either kind: word / node id per feature, mvKeysUn[i].angle, the FeatureVector as k_frame_featvec writes it
// (ascending node ids, the CSR and the indices in std::map / addFeature order, stopped words dropped; fv_meta = {node count, features kept}), and
// what it was computed with.
struct BowArrays {
    int32_t *word = nullptr, *node = nullptr; float *angle = nullptr;
    uint32_t *fv_node = nullptr; int32_t *fv_ptr = nullptr, *fv_index = nullptr, *fv_meta = nullptr;
    const orbx_vocabulary *voc = nullptr; int levelsup = 0;
};

// The rows of a handle as one call sees them (orbx_frame::view, orbx_keyframe::view): n / nl / nr = the counts, -1 while they are on the device only;
// a fisheye-stereo handle keeps the right camera's rows from roff on.
struct HandleRows {
    const uint8_t *desc; const orbx_keypoint *kps; const int32_t *count;
    int cap, n; bool fisheye; int roff, nl, nr;
    int feats() const { return n >= 0 ? n : cap; }                                   // features, or their bound
    // Rows the kernels index.  A fisheye-stereo handle is in ROW space; one made from a batch load keeps the gap behind its left rows after its counts
    // are adopted: what a call sizes per row goes by the row EXTENT, roff + N_right, not by N.
    int rows() const { return !fisheye || n < 0 ? feats() : roff + nr; }
};

}  // namespace

// A frame resident on the device across matcher calls (include/orbx.h, orbx_frame): keypoints, descriptors, optional mvuRight, the count, the
// scale factors and the 64x48 grid in buffers of its own -- not in the matcher's per-call arena, which begin() hands out again on every call.
// Every load and every use is enqueued on the owner's stream, so a load is ordered behind the calls that read the previous contents.
struct orbx_frame {
    orbx_matcher *owner = nullptr;
    int cap = 0;
    uint8_t *dev = nullptr;           // one allocation, carved below
    orbx_keypoint *kps = nullptr;
    uint8_t *desc = nullptr;
    float *u_right = nullptr, *scale = nullptr;
    float *depth = nullptr, *keys_xy = nullptr;   // mvDepth [cap], mvKeys[i].pt [cap][2]: valid while has_depth (the `_stereo` loads)
    int32_t *count = nullptr;
    uint16_t *gstart = nullptr, *gorder = nullptr;
    uint8_t *stage = nullptr;         // pinned (device-visible) staging of orbx_frame_load_host: the rows at the device layout's offsets
    size_t stage_bytes = 0;
    int32_t *h_count = nullptr;       // pinned: where the device count(s) land (fetch_count, frame_count) until adopt_count() reads them
    hipEvent_t ev_src = nullptr;      // load_batch: the extractor's stream up to the batch
    hipEvent_t ev_done = nullptr;     // load_batch: the copy has run (the extractor's next batch waits for it); load_host: the staging is free again
    bool stage_busy = false;
    bool loaded = false, has_ur = false, has_depth = false, n_known = false;
    int n = 0, nlevels = 0;
    std::vector<float> scale_h;       // mvScaleFactors on the host (the projection matchers' host-side window setup)
    float bounds[4] = {0, 0, 0, 0};
    std::vector<int32_t> h_match;     // result rows of a call made while N was still on the device (PendingRows: frame_fetch / frame_take)
    size_t off_kps = 0, off_desc = 0, off_ur = 0, off_count = 0, off_scale = 0, off_gstart = 0, off_gorder = 0, off_depth = 0, off_xy = 0;
    BowArrays bow;                    // Frame::ComputeBoW (orbx_frame_compute_bow[_fisheye]); valid until the next load
    bool bow_valid = false;
    uint64_t load_seq = 0;            // loads so far: orbx_keyframe_from_frame remembers (handle, load_seq) for orbx_keyframe_bow_from_frame
    // A fisheye-stereo frame (Frame::Nleft != -1, orbx_frame_load_host_fisheye / orbx_frame_load_stereo_fisheye_batch): features [0, N_left) are the
    // left camera's (rows [0, N_left)), [N_left, N) the right camera's, stored at rows [roff, roff + N_right) -- roff is known on the host before
    // the counts are (a batch load puts them at the left extractor's capacity).  count[0] / count[1] = N_left / N_right on the device; the right
    // camera has a grid of its own; l2r [N_left] / r2l [N_right] = mvLeftToRightMatch / mvRightToLeftMatch.
    bool fisheye = false;
    int roff = 0, n_left = 0, n_right = -1;   // (cached with n_known; a monocular frame: roff = 0, n_left = n, n_right = -1)
    int32_t *l2r = nullptr, *r2l = nullptr;
    uint16_t *gstart_r = nullptr, *gorder_r = nullptr;
    size_t off_l2r = 0, off_r2l = 0;

    // N as the host sees it.  A batch load leaves the count(s) on the device (n_known == false) until a call needs them: host_*() = the count, or -1
    // for "not yet"; rows_*() = the count, or meanwhile the capacity that a call's per-feature buffers are sized by.
    int host_n() const { return n_known ? n : -1; }
    int host_left() const { return n_known ? n_left : -1; }
    int host_right() const { return n_known ? n_right : -1; }
    int rows_n() const { return n_known ? n : cap; }
    int rows_left() const { return n_known ? n_left : roff; }
    int rows_right() const { return n_known ? n_right : cap - roff; }
    HandleRows view() const { return HandleRows{desc, kps, count, cap, host_n(), fisheye, roff, host_left(), host_right()}; }
    // A call that meets the handle with N pending brings N home with its results: fetch_count() among its downloads, adopt_count() behind its
    // synchronisation (frame_fetch / frame_take).  adopt() is the one place that learns N -- from a loader (frame_loaded) or from the device.
    int fetch_count() { return owner->d2h(h_count, count, fisheye ? 8 : 4); }
    void adopt(int c0, int c1 = 0) {
        n_left = std::min(std::max(c0, 0), fisheye ? roff : cap);
        n_right = fisheye ? std::min(std::max(c1, 0), cap - roff) : -1;
        n = n_left + std::max(n_right, 0);
        n_known = true;
    }
    void adopt_count() { adopt(h_count[0], fisheye ? h_count[1] : 0); }
};

namespace {

inline GridParams grid_of(const float *b) {
    GridParams g;
    g.minx = b[0]; g.miny = b[2];
    g.inv_w = 64.0f / (b[1] - b[0]);  // Frame.cc:342-343
    g.inv_h = 48.0f / (b[3] - b[2]);
    return g;
}

// the frame side of k_in_frustum's record
inline FrustumFrame frustum_frame(const orbx_camera *cam, const orbx_frame_pose *pose, const float *b, float log_sf, int nlevels, float cos_limit) {
    FrustumFrame F;
    memcpy(F.Rcw, pose->Rcw, sizeof(F.Rcw)); memcpy(F.tcw, pose->tcw, sizeof(F.tcw)); memcpy(F.Ow, pose->Ow, sizeof(F.Ow));
    F.fx = cam->fx; F.fy = cam->fy; F.cx = cam->cx; F.cy = cam->cy; F.mbf = cam->bf;
    F.minx = b[0]; F.maxx = b[1]; F.miny = b[2]; F.maxy = b[3];
    F.log_scale_factor = log_sf; F.nlevels = nlevels; F.cos_limit = cos_limit;
    return F;
}

// The destination half of a prepare record (FramePrepare / FisheyePrepare), everything else zeroed: the resident buffers of a frame handle or a key frame
// (both name them alike), the scale factors and the level count.  roff: the right camera's first row (FisheyePrepare only).  The source rows, the
// counts and the capacities are the caller's to add.
template <class P, class H> void prepare_dst(P &R, const H *h, int roff, const float *scale_factors, int nlevels) {
    memset(&R, 0, sizeof(R));
    R.kps = h->kps; R.desc = h->desc; R.count = h->count; R.scale = h->scale; R.nlevels = nlevels;
    memcpy(R.scale_host, scale_factors, sizeof(float) * (size_t)nlevels);
    if constexpr (std::is_same<P, FisheyePrepare>::value) {
        R.gstart[0] = h->gstart; R.gorder[0] = h->gorder; R.gstart[1] = h->gstart_r; R.gorder[1] = h->gorder_r; R.roff = roff;
    } else {
        R.gstart = h->gstart; R.gorder = h->gorder;
    }
}

// a load's record, and the handle's bookkeeping: what the host-side window setup reads (scale factors, levels, bounds)
template <class P> void frame_prepare_common(orbx_frame *f, P &R, int roff, const float *scale_factors, int nlevels, const float *bounds4) {
    prepare_dst(R, f, roff, scale_factors, nlevels);
    f->scale_h.assign(scale_factors, scale_factors + nlevels);
    f->nlevels = nlevels;
    memcpy(f->bounds, bounds4, sizeof(f->bounds));
}

// N of a handle: cached, else one download of the device count(s) (and a synchronisation of the owner's stream)
int frame_count(orbx_frame *f, int *n) {
    if (!f->n_known) {
        orbx_matcher *m = f->owner;
        ORBX_HIP(hipSetDevice(m->device));
        ORBX_HIP(hipMemcpyAsync(f->h_count, f->count, f->fisheye ? 8 : 4, hipMemcpyDeviceToHost, m->stream));
        ORBX_HIP(hipStreamSynchronize(m->stream));
        m->dirty = false;
        f->adopt_count();
    }
    *n = f->n;
    return ORBX_OK;
}

// The result tail of every call on a frame handle: frame_fetch() among the call's downloads -- the rows, then the count(s) if N is pending -- and
// frame_take() behind its synchronisation: the count(s) adopted, the first N (left_only: N_left) entries of every row handed out.  Every site calls
// frame_take() unconditionally: it does nothing for a host-pointer call (f NULL) or when N was known, and says whether it adopted the count(s).
int frame_fetch(orbx_frame *f, const Rows *blocks, int n_blocks) {
    ORBX_TRY((PendingRows{f->owner, f->h_match, !f->n_known}.fetch(blocks, n_blocks)));
    return f->n_known ? ORBX_OK : f->fetch_count();   // N comes back with the results (one small copy of the handle's count(s))
}
bool frame_take(orbx_frame *f, const Rows *blocks, int n_blocks, bool left_only = false) {
    if (!f || f->n_known) return false;
    f->adopt_count();
    PendingRows{f->owner, f->h_match, true}.take(blocks, n_blocks, left_only ? f->n_left : f->n);
    return true;
}

// the resident side of a window problem; right: the right camera of a fisheye-stereo frame (rows from roff on, count[1], its own grid)
inline void frame_side(const orbx_frame *f, bool right, WindowProblem &P) {
    const size_t ro = right ? (size_t)f->roff : 0;
    P.kps = f->kps + ro; P.desc = f->desc + 32 * ro; P.n_ptr = f->count + (right ? 1 : 0);
    P.gstart = right ? f->gstart_r : f->gstart; P.gorder = right ? f->gorder_r : f->gorder;
}

// The head of a load from host arrays: the previous load may still read the staging; the transfer statistics of this load start here
// (orbx_matcher_debug_transfers).
int frame_begin_host_load(orbx_frame *f) {
    ORBX_HIP(hipSetDevice(f->owner->device));
    if (f->stage_busy) { ORBX_HIP(hipEventSynchronize(f->ev_done)); f->stage_busy = false; }
    f->owner->begin();
    return ORBX_OK;
}

// The tail of every load, behind its kernel launch: the launch's error, ev_done (a batch load: the copy has run; staged: the staging is free again),
// and ALL of the handle's bookkeeping -- nothing else writes it.  roff: the right camera's first row (monocular: 0); c0, c1: N (, 0) or N_left,
// N_right where the host knows them, c0 < 0 while they are on the device only.  has_depth: the load filled mvDepth and the raw (x, y) rows too.
int frame_loaded(orbx_frame *f, bool fisheye, int roff, int c0, int c1, bool has_ur, bool has_depth, bool staged) {
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipEventRecord(f->ev_done, f->owner->stream));
    if (staged) f->stage_busy = true;
    f->fisheye = fisheye; f->roff = roff; f->has_ur = has_ur; f->has_depth = has_depth;
    f->loaded = true; f->bow_valid = false; f->load_seq++;
    f->n_known = false; f->n = f->n_left = 0; f->n_right = -1;
    if (c0 >= 0) f->adopt(c0, c1);
    return ORBX_OK;
}

// The host-side window setup of the projection matchers, per query.
struct Windows {
    std::vector<float> qr;
    std::vector<int32_t> qmin, qmax;
    std::vector<uint8_t> valid;
    explicit Windows(int n) : qr(n), qmin(n), qmax(n), valid(n) {}
};
// map points: r = RadiusByViewingCos(viewCos) [* th] * scale[level], levels [lvl-1, lvl]  (ORBmatcher.cc:63-72; in_view NULL: every point)
Windows mappoint_windows(const orbx_frame_desc *F, int n, const uint8_t *in_view, const int32_t *level, const float *view_cos, float th) {
    Windows w(n);
    const bool bFactor = th != 1.0;
    for (int i = 0; i < n; i++) {
        const int lvl = level[i];
        w.valid[i] = (!in_view || in_view[i]) && lvl >= 0 && lvl < F->nlevels;
        float r = (view_cos[i] > 0.998) ? 2.5f : 4.0f;
        if (bFactor) r *= th;
        w.qr[i] = w.valid[i] ? r * F->scale_factors[lvl] : 0.f;
        w.qmin[i] = lvl - 1; w.qmax[i] = lvl;
    }
    return w;
}
// the last frame's features: r = th * scale[octave], levels by level_mode  (ORBmatcher.cc:1726-1735)
Windows octave_windows(const orbx_frame_desc *F, int n, const int32_t *octave, float th, int level_mode) {
    Windows w(n);
    for (int i = 0; i < n; i++) {
        const int o = octave[i];
        w.valid[i] = o >= 0 && o < F->nlevels;
        w.qr[i] = w.valid[i] ? th * F->scale_factors[o] : 0.f;  // :1726
        if (level_mode == 1) { w.qmin[i] = o; w.qmax[i] = -1; }          // bForward  :1731
        else if (level_mode == 2) { w.qmin[i] = 0; w.qmax[i] = o; }      // bBackward :1733
        else { w.qmin[i] = o - 1; w.qmax[i] = o + 1; }                   // :1735
    }
    return w;
}

// shared driver of the two projection matchers (host-pointer form)
struct ProjArgs {
    const orbx_frame_desc *frame;
    const uint8_t *occupied;
    int nq;
    const float *qx, *qy, *qr, *qxr;
    const int32_t *qmin, *qmax;
    const uint8_t *qdesc, *qvalid, *q_has_obs;
    const float *q_angle;
    int mode;
    float nnratio;
    int check_orientation;
    int32_t *match_out;
    float max_dist;
    const struct TrackArgs *track = nullptr;
};

// The queries of a handle call that projects on the device (k_track_project) instead of uploading query records: entry i of ids = the map slot of the
// source's feature i or -1, nq = n_ids, q_has_obs [n_ids] the only per-query host array (qx .. q_angle of ProjArgs are NULL).  The source's rows are
// resident (the last frame's handle, a key frame).  orbx_map and orbx_keyframe are defined further down: run_projection reaches the table's records
// and the two waits that order the table and a key-frame source in front of the kernel through the three functions declared here.
struct TrackArgs {
    bool reloc;                                   // k_track_project<RELOC>
    orbx_map *map; const int32_t *ids;
    orbx_keyframe *kf;                            // the source when it is a key frame (waited for through keyframe_wait_ready), else NULL
    const orbx_keypoint *src_kps; const int32_t *src_count;
    const orbx_camera *cam; const orbx_frame_pose *pose;   // a monocular / rectified current frame
    float th, log_scale_factor; int level_mode;
    uint8_t *projected; float *proj_u, *proj_v;   // optional outputs [n_ids]
    // a fisheye-stereo rig (view != NULL; cam and pose are NULL then): the LEFT camera's view, GetRelativePoseTrl() (k_track_project<false, true> only)
    // and the right camera's first row of the source
    const orbx_fisheye_view *view; const float *Trl_R, *Trl_t; int src_roff;
    struct Out { uint64_t seq; bool waited; } *out;   // what map_points_done() is told behind the call; the call got as far as its waits
};
const uint4 *map_records(const orbx_map *map, int *cap);
int map_wait_written(orbx_matcher *m, orbx_map *map, uint64_t *seq);
int keyframe_wait_ready(orbx_matcher *m, orbx_keyframe *kf);

// Everything of k_track_project's record but the arena buffers (the caller's layout has carved those), the two waits, and the launch: between a
// call's uploads and its window scan.
int track_launch(orbx_matcher *m, const TrackArgs &tr, const orbx_frame *fh, int nq, TrackProject &T) {
    T.rec = map_records(tr.map, &T.cap); T.n_ids = nq;
    T.src_kps = tr.src_kps; T.src_count = tr.src_count; T.src_roff = tr.src_roff;
    if (tr.view) {
        memcpy(T.pose.Rcw, tr.view->R, sizeof(T.pose.Rcw)); memcpy(T.pose.tcw, tr.view->t, sizeof(T.pose.tcw)); memcpy(T.pose.Ow, tr.view->twc, sizeof(T.pose.Ow));
        memcpy(T.kb8, tr.view->params, sizeof(T.kb8));
        if (tr.Trl_R) { memcpy(T.Trl_R, tr.Trl_R, sizeof(T.Trl_R)); memcpy(T.Trl_t, tr.Trl_t, sizeof(T.Trl_t)); }
    } else {
        T.pose = *tr.pose;
        T.fx = tr.cam->fx; T.fy = tr.cam->fy; T.cx = tr.cam->cx; T.cy = tr.cam->cy; T.bf = tr.cam->bf;
    }
    T.minx = fh->bounds[0]; T.maxx = fh->bounds[1]; T.miny = fh->bounds[2]; T.maxy = fh->bounds[3];
    T.th = tr.th; T.log_scale_factor = tr.log_scale_factor; T.level_mode = tr.level_mode; T.nlevels = fh->nlevels; T.scale = fh->scale;
    if (tr.kf) ORBX_TRY(keyframe_wait_ready(m, tr.kf));
    ORBX_TRY(map_wait_written(m, tr.map, &tr.out->seq));
    tr.out->waited = true;
    const dim3 grid((unsigned)((nq + 255) / 256));
    if (tr.view && tr.reloc) hipLaunchKernelGGL((k_track_project<true, true>), grid, dim3(256), 0, m->exec(), T);
    else if (tr.view) hipLaunchKernelGGL((k_track_project<false, true>), grid, dim3(256), 0, m->exec(), T);
    else if (tr.reloc) hipLaunchKernelGGL((k_track_project<true, false>), grid, dim3(256), 0, m->exec(), T);
    else hipLaunchKernelGGL((k_track_project<false, false>), grid, dim3(256), 0, m->exec(), T);
    return ORBX_OK;
}
// the optional outputs among a call's downloads
int track_fetch(orbx_matcher *m, const TrackArgs &tr, const TrackProject &T, int nq) {
    if (tr.proj_u) { ORBX_TRY(m->d2h(tr.proj_u, T.qx, 4 * (size_t)nq)); ORBX_TRY(m->d2h(tr.proj_v, T.qy, 4 * (size_t)nq)); }
    if (tr.projected) ORBX_TRY(m->d2h(tr.projected, T.projected, (size_t)nq));
    return ORBX_OK;
}

// fh != NULL: the handle form -- the frame's rows and grid are resident (a.frame is not read); while its N is still on the device (a load_batch
// nobody has counted yet) every per-feature buffer is sized by the handle's capacity and the count comes back with the results.
// left_only: a fisheye-stereo handle searched through its left camera only (rows [0, N_left), the left grid, count[0]); match_out and the
// occupancy mask keep the frame's N entries, the right camera's stay -1.
int run_projection(orbx_matcher *m, const ProjArgs &a, orbx_frame *fh = nullptr, bool left_only = false) {
    const orbx_frame_desc *F = a.frame;
    const int nq = a.nq;
    int n = fh ? -1 : F->n, n_out = n;   // n: the features searched, n_out: the entries of match_out
    if (fh && (fh->n_known || a.occupied || nq == 0)) {   // the mask holds N entries
        const int rc = frame_count(fh, &n);
        if (rc != ORBX_OK) return rc;
        n_out = n;
        if (left_only) n = fh->n_left;
    }
    for (int i = 0; i < n_out; i++) a.match_out[i] = -1;
    if (n == 0 || nq == 0) return 0;
    const int nc = !fh ? n : left_only ? fh->rows_left() : fh->rows_n();   // features the device buffers are sized for
    if (nc > kMaxResolveFeatures) return ORBX_E_TOO_LARGE;  // before anything is enqueued: the resolve pass keeps 10 B per feature in LDS
    ORBX_HIP(hipSetDevice(m->device));
    WindowProblem P;
    memset(&P, 0, sizeof(P));
    ResolveProblem R;
    memset(&R, 0, sizeof(R));
    R.mode = a.mode; R.nnratio = a.nnratio; R.check_orientation = a.check_orientation; R.max_dist = a.max_dist;
    R.cleared_value = -2;
    const bool has_ur = fh ? fh->has_ur : F->u_right != nullptr;
    // a small problem skips the grid: k_window_brute walks all features per query (no k_grid_build launch, whose counting sort this one call would use once);
    // a handle's grid is built already
    const bool brute = !fh && m->brute_windows && (size_t)nq * (size_t)n <= kBruteMaxPairs;
    const int32_t cnts[2] = {n, nq};
    int32_t *dcnt;
    const TrackArgs *tr = a.track;
    TrackProject T;
    memset(&T, 0, sizeof(T));
    WindowProblem *dP;
    ResolveProblem *dR;
    ORBX_TRY(m->carve([&](Carve &A) {
        if (!fh) { P.kps = A.up(F->keypoints_un, (size_t)n); P.desc = A.up(F->descriptors, 32 * (size_t)n); }   // (resident rows: nothing of the frame travels)
        dcnt = A.up(cnts, 2, 2);
        if (fh && has_ur) P.u_right = fh->u_right;
        else if (has_ur) P.u_right = A.up(F->u_right, (size_t)n);
        P.occupied0 = A.up_opt(a.occupied, (size_t)n);
        if (tr) {   // the ids and the flags are all that travels per query; the records are k_track_project's, behind the uploads
            T.ids = A.up(tr->ids, (size_t)nq);
        } else {
            P.qx = A.up(a.qx, (size_t)nq); P.qy = A.up(a.qy, (size_t)nq); P.qr = A.up(a.qr, (size_t)nq);
            P.qmin = A.up(a.qmin, (size_t)nq); P.qmax = A.up(a.qmax, (size_t)nq);
            if (has_ur) P.qxr = A.up_opt(a.qxr, (size_t)nq);
            P.qdesc = A.up(a.qdesc, 32 * (size_t)nq);
            P.qvalid = A.up_opt(a.qvalid, (size_t)nq);
            R.q_angle = A.up_opt(a.q_angle, (size_t)nq);
        }
        R.q_has_obs = A.up_opt(a.q_has_obs, (size_t)nq);
        // everything the call uploads lies in ONE run of the arena (one DMA, orbx_matcher::exec): the two problem records directly behind the inputs,
        // the buffers only the device writes behind them; the downloads (match, nmatches) side by side as well
        dP = A.take<WindowProblem>(1);
        dR = A.take<ResolveProblem>(1);
        if (tr) {
            T.qr = A.take<float>(nq); T.qmin = A.take<int32_t>(nq); T.qmax = A.take<int32_t>(nq);
            if (has_ur && !tr->reloc) T.qxr = A.take<float>(nq);
            T.qdesc = A.take<uint8_t>(32 * (size_t)nq); T.qvalid = A.take<uint8_t>(nq); T.q_angle = A.take<float>(nq);
        }
        P.keys = A.take<u64>((size_t)nq * kTopK); P.meta = A.take<int32_t>(nq);
        if (!fh) { P.gstart = A.take<uint16_t>(kGridCells + 1); P.gorder = A.take<uint16_t>(n); }
        R.entries = A.take<int32_t>(nq);
        if (tr) {   // (u, v) and the gates' verdicts go down with the matches
            T.qx = A.take<float>(nq); T.qy = A.take<float>(nq);
            if (tr->projected) T.projected = A.take<uint8_t>(nq);
        }
        R.match = A.take<int32_t>(nc);
        R.nmatches = A.take<int32_t>(1);
    }));
    if (fh) frame_side(fh, false, P);
    else P.n_ptr = dcnt;
    P.nq_ptr = dcnt + 1;
    if (brute) { P.gstart = nullptr; P.gorder = nullptr; }
    if (tr) {
        P.qx = T.qx; P.qy = T.qy; P.qr = T.qr; P.qmin = T.qmin; P.qmax = T.qmax; P.qxr = T.qxr; P.qdesc = T.qdesc; P.qvalid = T.qvalid;
        R.q_angle = T.q_angle;
        if (tr->reloc) P.u_right = nullptr;   // Relocalization's search never reads mvuRight (ORBmatcher.cc:1955-1966): no right-coordinate gate
    }
    ORBX_TRY(m->h2d(dP, &P, sizeof(P))); ORBX_TRY(m->h2d(dR, &R, sizeof(R)));
    if (tr) ORBX_TRY(track_launch(m, *tr, fh, nq, T));
    const float fb[4] = {fh ? fh->bounds[0] : F->min_x, fh ? fh->bounds[1] : F->max_x, fh ? fh->bounds[2] : F->min_y, fh ? fh->bounds[3] : F->max_y};
    const GridParams g = grid_of(fb);
    if (brute) {
        hipLaunchKernelGGL(k_window_brute, dim3((nq + 3) / 4), dim3(256), 0, m->exec(), dP, g);
    } else {
        if (!fh) ORBX_LAUNCH_GRID_BUILD( dim3(1), dim3(64), 0, m->exec(), dP, g);
        ORBX_LAUNCH_WINDOW_BEST2(nq, 1, m->exec(), dP, g);
    }
    { const int rr = brute ? launch_resolve<true>(1, m->exec(), dP, dR, g, nc, nq, 4) : launch_resolve<false>(1, m->exec(), dP, dR, g, nc, nq, 4); if (rr != ORBX_OK) return rr; }
    int32_t nm = 0;
    const Rows rows = {R.match, 1, nc, a.match_out, 0};
    if (!fh) ORBX_TRY(m->d2h(a.match_out, R.match, 4 * (size_t)n));
    else ORBX_TRY(frame_fetch(fh, &rows, 1));
    ORBX_TRY(m->d2h(&nm, R.nmatches, 4));
    if (tr) ORBX_TRY(track_fetch(m, *tr, T, nq));
    ORBX_TRY(m->sync_and_deliver());
    if (frame_take(fh, &rows, 1, left_only) && left_only)
        for (int i = fh->n_left; i < fh->n; i++) a.match_out[i] = -1;
    return nm;
}

}  // namespace

extern "C" {

static int search_mappoints_impl(orbx_matcher *m, const orbx_frame_desc *frame, orbx_frame *fh, const uint8_t *frame_occupied, int n_mp,
                                 const float *proj_x, const float *proj_y, const float *proj_xr, const int32_t *pred_level, const float *view_cos,
                                 const uint8_t *mp_desc, const uint8_t *mp_in_view, const uint8_t *mp_has_obs, float th, float nnratio,
                                 int32_t *frame_match) {
    if (!m || !frame || frame->n < 0 || (!frame_match && frame->n > 0) || n_mp < 0) return ORBX_E_BAD_ARG;   // empty frames / query sets are legal
    if (n_mp > 0 && (!proj_x || !proj_y || !pred_level || !view_cos || !mp_desc)) return ORBX_E_BAD_ARG;
    const Windows w = mappoint_windows(frame, n_mp, mp_in_view, pred_level, view_cos, th);
    ProjArgs a = {frame, frame_occupied, n_mp, proj_x, proj_y, w.qr.data(), proj_xr, w.qmin.data(), w.qmax.data(), mp_desc, w.valid.data(),
                  mp_has_obs, nullptr, 1, nnratio, 0, frame_match, (float)ORBX_TH_HIGH};
    return run_projection(m, a, fh);
}

int orbx_search_by_projection_mappoints(orbx_matcher *m, const orbx_frame_desc *frame, const uint8_t *frame_occupied, int n_mp,
                                        const float *proj_x, const float *proj_y, const float *proj_xr,
                                        const int32_t *pred_level, const float *view_cos, const uint8_t *mp_desc,
                                        const uint8_t *mp_in_view, const uint8_t *mp_has_obs, float th, float nnratio,
                                        int32_t *frame_match) {
    return search_mappoints_impl(m, frame, nullptr, frame_occupied, n_mp, proj_x, proj_y, proj_xr, pred_level, view_cos, mp_desc, mp_in_view,
                                 mp_has_obs, th, nnratio, frame_match);
}

static int search_frame_impl(orbx_matcher *m, const orbx_frame_desc *cur, orbx_frame *fh, const uint8_t *cur_occupied, int n_q, const float *q_u,
                             const float *q_v, const float *q_ur, const int32_t *q_octave, const float *q_angle, const uint8_t *q_desc,
                             const uint8_t *q_has_obs, float th, int level_mode, int check_orientation, int32_t *cur_match) {
    if (!m || !cur || cur->n < 0 || (!cur_match && cur->n > 0) || n_q < 0) return ORBX_E_BAD_ARG;
    if (n_q > 0 && (!q_u || !q_v || !q_octave || !q_desc || (check_orientation && !q_angle))) return ORBX_E_BAD_ARG;
    const Windows w = octave_windows(cur, n_q, q_octave, th, level_mode);
    ProjArgs a = {cur, cur_occupied, n_q, q_u, q_v, w.qr.data(), q_ur, w.qmin.data(), w.qmax.data(), q_desc, w.valid.data(), q_has_obs,
                  q_angle, 2, 0.f, check_orientation, cur_match, (float)ORBX_TH_HIGH};
    return run_projection(m, a, fh);
}

int orbx_search_by_projection_frame(orbx_matcher *m, const orbx_frame_desc *cur, const uint8_t *cur_occupied, int n_q,
                                    const float *q_u, const float *q_v, const float *q_ur, const int32_t *q_octave,
                                    const float *q_angle, const uint8_t *q_desc, const uint8_t *q_has_obs, float th, int level_mode,
                                    int check_orientation, int32_t *cur_match) {
    return search_frame_impl(m, cur, nullptr, cur_occupied, n_q, q_u, q_v, q_ur, q_octave, q_angle, q_desc, q_has_obs, th, level_mode,
                             check_orientation, cur_match);
}

}  // extern "C"

namespace {

// shared driver of the fisheye-stereo twins of the two frame projection matchers (k_replay_twin)
struct TwinArgs {
    const orbx_frame_desc *left;          // left camera: mvKeys, n_left, image bounds, scale factors; descriptors of ALL n_left + n_right features
    const orbx_keypoint *kps_right; int n_right;
    const int32_t *l2r, *r2l;
    const uint8_t *occupied;              // [n_left + n_right]
    int nq;
    const float *qx[2], *qy[2], *qr[2];   // per side: window centre and half size
    const int32_t *qmin[2], *qmax[2];
    const uint8_t *qvalid[2];
    const uint8_t *qdesc, *q_has_obs;
    const float *q_angle;
    int mode; float nnratio; int check_orientation;
    int32_t *match_out;
    const TrackArgs *track = nullptr;     // a handle call whose queries k_track_project writes (qx .. q_angle are NULL then)
};

// the twin window search of both cameras and the replay; dP = the two problems (uploaded or to be uploaded by the caller), n_alloc >= N
int launch_twin(orbx_matcher *m, const WindowProblem *dP, const TwinProblem &T, const GridParams &g, int n_alloc, int nq) {
    ORBX_LAUNCH_WINDOW_BEST2(nq, 2, m->exec(), dP, g);
    const size_t lds = twin_lds_bytes(n_alloc);
    if (lds > 64 * 1024) ORBX_HIP(hipFuncSetAttribute((const void *)k_replay_twin, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_replay_twin, dim3(1), dim3(kTwinBlock), lds, m->exec(), dP, T, g, n_alloc);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

// fh != NULL: the handle form -- rows, grids, counts and stereo partners are resident (a.left supplies the bounds and scale factors only); while the
// counts are still on the device every per-feature buffer is sized by the handle's capacity and N comes back with the results
int run_projection_twin(orbx_matcher *m, const TwinArgs &a, orbx_frame *fh = nullptr) {
    const orbx_frame_desc *F = a.left;
    const int nq = a.nq;
    int nl = fh ? -1 : F->n, nr = fh ? -1 : a.n_right, N = fh ? -1 : nl + nr;
    if (fh && (fh->n_known || a.occupied || nq == 0)) {   // the mask holds N entries
        const int rc = frame_count(fh, &N);
        if (rc != ORBX_OK) return rc;
        nl = fh->n_left; nr = fh->n_right;
    }
    for (int i = 0; i < N; i++) a.match_out[i] = -1;
    if (N == 0 || nq == 0) return 0;
    const int nc = fh ? fh->rows_n() : N;   // features the device buffers are sized for
    if (nc > 60000) return ORBX_E_TOO_LARGE;   // 16-bit feature indices in the candidate keys; occupancy bytes in LDS
    ORBX_HIP(hipSetDevice(m->device));
    WindowProblem P[2];
    memset(P, 0, sizeof(P));
    TwinProblem T;
    memset(&T, 0, sizeof(T));
    T.mode = a.mode; T.nq = nq; T.nnratio = a.nnratio; T.max_dist = (float)ORBX_TH_HIGH;
    T.check_orientation = a.check_orientation; T.cleared_value = -2;
    const int32_t cnts[3] = {nl, nr, nq};
    int32_t *dcnt;
    orbx_keypoint *dk = nullptr;
    uint8_t *dd = nullptr;
    WindowProblem *dP;
    const TrackArgs *tr = a.track;
    TrackProject K;
    memset(&K, 0, sizeof(K));
    if (tr) ORBX_TRY(m->carve([&](Carve &A) {   // the track form's own layout: ids and flags up in one run, the records k_track_project's
        dcnt = A.up(cnts, 3, 1);
        K.ids = A.up(tr->ids, (size_t)nq);
        T.occupied0 = A.up_opt(a.occupied, (size_t)N);
        T.q_has_obs = A.up_opt(a.q_has_obs, (size_t)nq);
        dP = A.take<WindowProblem>(2);
        K.qr = A.take<float>(nq); K.qmin = A.take<int32_t>(nq); K.qmax = A.take<int32_t>(nq); K.qxr = A.take<float>(nq); K.qyr = A.take<float>(nq);
        K.qdesc = A.take<uint8_t>(32 * (size_t)nq); K.qvalid = A.take<uint8_t>(nq); K.q_angle = A.take<float>(nq);
        for (int s = 0; s < 2; s++) { P[s].keys = A.take<u64>((size_t)nq * kTopK); P[s].meta = A.take<int32_t>(nq); }
        T.entries = A.take<int32_t>(2 * (size_t)nq);
        K.qx = A.take<float>(nq); K.qy = A.take<float>(nq);   // (u, v) and the verdicts go down with the matches
        if (tr->projected) K.projected = A.take<uint8_t>(nq);
        T.match = A.take<int32_t>(nc); T.nmatches = A.take<int32_t>(1);
    }));
    else ORBX_TRY(m->carve([&](Carve &A) {
        dcnt = A.up(cnts, 3, 1);
        if (!fh) {   // (resident rows and grids: nothing of the frame travels)
            dk = A.take<orbx_keypoint>(N);
            dd = A.up(F->descriptors, 32 * (size_t)N);
            for (int s = 0; s < 2; s++) { P[s].gstart = A.take<uint16_t>(kGridCells + 1); P[s].gorder = A.take<uint16_t>(std::max(s ? nr : nl, 1)); }
        }
        const uint8_t *dqd = A.up(a.qdesc, 32 * (size_t)nq);
        for (int s = 0; s < 2; s++) {
            WindowProblem &w = P[s];
            w.qx = A.up(a.qx[s], (size_t)nq); w.qy = A.up(a.qy[s], (size_t)nq); w.qr = A.up(a.qr[s], (size_t)nq);
            w.qmin = A.up(a.qmin[s], (size_t)nq); w.qmax = A.up(a.qmax[s], (size_t)nq);
            w.qvalid = A.up(a.qvalid[s], (size_t)nq);
            w.qdesc = dqd;
            w.keys = A.take<u64>((size_t)nq * kTopK); w.meta = A.take<int32_t>(nq);
        }
        if (fh) { T.l2r = fh->l2r; T.r2l = fh->r2l; }
        else {
            if (nl) T.l2r = A.up_opt(a.l2r, (size_t)nl);
            if (nr) T.r2l = A.up_opt(a.r2l, (size_t)nr);
        }
        T.occupied0 = A.up_opt(a.occupied, (size_t)N);
        T.q_has_obs = A.up_opt(a.q_has_obs, (size_t)nq);
        T.q_angle = A.up_opt(a.q_angle, (size_t)nq);
        T.match = A.take<int32_t>(nc); T.nmatches = A.take<int32_t>(1); T.entries = A.take<int32_t>(2 * (size_t)nq);
        dP = A.take<WindowProblem>(2);
    }));
    if (tr) {   // left: (u, v); right: the projection into the right camera; one radius, level window and validity for both (:1800)
        for (int s = 0; s < 2; s++) {
            WindowProblem &w = P[s];
            w.qx = s ? K.qxr : K.qx; w.qy = s ? K.qyr : K.qy; w.qr = K.qr; w.qmin = K.qmin; w.qmax = K.qmax; w.qvalid = K.qvalid; w.qdesc = K.qdesc;
        }
        T.q_angle = K.q_angle; T.l2r = fh->l2r; T.r2l = fh->r2l;
    }
    if (fh) {
        for (int s = 0; s < 2; s++) frame_side(fh, s == 1, P[s]);
    } else {
        if (nl) ORBX_TRY(m->h2d(dk, F->keypoints_un, 28 * (size_t)nl));
        if (nr) ORBX_TRY(m->h2d(dk + nl, a.kps_right, 28 * (size_t)nr));
        for (int s = 0; s < 2; s++) { P[s].kps = dk + (s ? nl : 0); P[s].desc = dd + (s ? (size_t)nl * 32 : 0); P[s].n_ptr = dcnt + s; }
    }
    P[0].nq_ptr = P[1].nq_ptr = dcnt + 2;
    ORBX_TRY(m->h2d(dP, P, sizeof(P)));
    const float fb[4] = {F->min_x, F->max_x, F->min_y, F->max_y};
    const GridParams g = grid_of(fb);
    if (!fh) ORBX_LAUNCH_GRID_BUILD( dim3(2), dim3(64), 0, m->exec(), dP, g);
    if (tr) ORBX_TRY(track_launch(m, *tr, fh, nq, K));
    ORBX_TRY(launch_twin(m, dP, T, g, nc, nq));
    int32_t nm = 0;
    const Rows rows = {T.match, 1, nc, a.match_out, 0};
    if (!fh) ORBX_TRY(m->d2h(a.match_out, T.match, 4 * (size_t)N));
    else ORBX_TRY(frame_fetch(fh, &rows, 1));
    ORBX_TRY(m->d2h(&nm, T.nmatches, 4));
    if (tr) ORBX_TRY(track_fetch(m, *tr, K, nq));
    ORBX_TRY(m->sync_and_deliver());
    frame_take(fh, &rows, 1);
    return nm;
}

}  // namespace

// SearchByProjection(Frame&, const vector<MapPoint*>&, th, ...) for a fisheye-stereo frame (F.Nleft != -1), ORBmatcher.cc:43-213 whole
// fh != NULL: the handle form (left / kps_right / l2r / r2l: the resident frame's; left supplies the scale factors and levels only)
static int search_mappoints_fisheye_impl(orbx_matcher *m, const orbx_frame_desc *left, orbx_frame *fh, const orbx_keypoint *kps_right, int n_right,
                                         const int32_t *left_to_right, const int32_t *right_to_left, const uint8_t *frame_occupied,
                                         int n_mp, const uint8_t *in_view, const float *proj_x, const float *proj_y,
                                         const int32_t *pred_level, const float *view_cos, const uint8_t *in_view_r,
                                         const float *proj_xr, const float *proj_yr, const int32_t *pred_level_r,
                                         const float *view_cos_r, const uint8_t *mp_desc, const uint8_t *mp_has_obs, float th,
                                         float nnratio, int32_t *frame_match) {
    if (!m || !left || left->n < 0 || n_right < 0 || n_mp < 0 || (!frame_match && left->n + n_right > 0)) return ORBX_E_BAD_ARG;
    if (!fh && ((left->n > 0 && !left_to_right) || (n_right > 0 && (!right_to_left || !kps_right)))) return ORBX_E_BAD_ARG;
    if (n_mp > 0 && (!in_view || !proj_x || !proj_y || !pred_level || !view_cos || !in_view_r || !proj_xr || !proj_yr || !pred_level_r || !view_cos_r || !mp_desc))
        return ORBX_E_BAD_ARG;
    // left search :60-76; right twin :144-152: needs mbTrackInViewR and mnTrackScaleLevelR != -1, RadiusByViewingCos(mTrackViewCosR) WITHOUT the th factor
    const Windows w[2] = {mappoint_windows(left, n_mp, in_view, pred_level, view_cos, th), mappoint_windows(left, n_mp, in_view_r, pred_level_r, view_cos_r, 1.f)};
    TwinArgs a = {left, kps_right, n_right, left_to_right, right_to_left, frame_occupied, n_mp, {proj_x, proj_xr}, {proj_y, proj_yr},
                  {w[0].qr.data(), w[1].qr.data()}, {w[0].qmin.data(), w[1].qmin.data()}, {w[0].qmax.data(), w[1].qmax.data()},
                  {w[0].valid.data(), w[1].valid.data()}, mp_desc, mp_has_obs, nullptr, 1, nnratio, 0, frame_match};
    return run_projection_twin(m, a, fh);
}

extern "C" int orbx_search_by_projection_mappoints_fisheye(orbx_matcher *m, const orbx_frame_desc *left, const orbx_keypoint *kps_right, int n_right,
                                                           const int32_t *left_to_right, const int32_t *right_to_left, const uint8_t *frame_occupied,
                                                           int n_mp, const uint8_t *in_view, const float *proj_x, const float *proj_y,
                                                           const int32_t *pred_level, const float *view_cos, const uint8_t *in_view_r,
                                                           const float *proj_xr, const float *proj_yr, const int32_t *pred_level_r,
                                                           const float *view_cos_r, const uint8_t *mp_desc, const uint8_t *mp_has_obs, float th,
                                                           float nnratio, int32_t *frame_match) {
    return search_mappoints_fisheye_impl(m, left, nullptr, kps_right, n_right, left_to_right, right_to_left, frame_occupied, n_mp, in_view, proj_x, proj_y,
                                         pred_level, view_cos, in_view_r, proj_xr, proj_yr, pred_level_r, view_cos_r, mp_desc, mp_has_obs, th, nnratio,
                                         frame_match);
}

// SearchByProjection(Frame& Cur, const Frame& Last, th, bMono) for a fisheye-stereo current frame, ORBmatcher.cc:1676-1887 with :1794-1863
static int search_frame_fisheye_impl(orbx_matcher *m, const orbx_frame_desc *left, orbx_frame *fh, const orbx_keypoint *kps_right, int n_right,
                                     const uint8_t *cur_occupied, int n_q, const float *q_u, const float *q_v, const float *q_ur,
                                     const float *q_vr, const int32_t *q_octave, const float *q_angle, const uint8_t *q_desc,
                                     const uint8_t *q_has_obs, float th, int level_mode, int check_orientation, int32_t *cur_match) {
    if (!m || !left || left->n < 0 || n_right < 0 || n_q < 0 || (!cur_match && left->n + n_right > 0) || (!fh && n_right > 0 && !kps_right)) return ORBX_E_BAD_ARG;
    if (n_q > 0 && (!q_u || !q_v || !q_ur || !q_vr || !q_octave || !q_desc || (check_orientation && !q_angle))) return ORBX_E_BAD_ARG;
    const Windows w = octave_windows(left, n_q, q_octave, th, level_mode);   // the twin uses the same radius (:1800)
    TwinArgs a = {left, kps_right, n_right, nullptr, nullptr, cur_occupied, n_q, {q_u, q_ur}, {q_v, q_vr}, {w.qr.data(), w.qr.data()},
                  {w.qmin.data(), w.qmin.data()}, {w.qmax.data(), w.qmax.data()}, {w.valid.data(), w.valid.data()}, q_desc, q_has_obs, q_angle, 2, 0.f,
                  check_orientation, cur_match};
    return run_projection_twin(m, a, fh);
}

extern "C" int orbx_search_by_projection_frame_fisheye(orbx_matcher *m, const orbx_frame_desc *left, const orbx_keypoint *kps_right, int n_right,
                                                       const uint8_t *cur_occupied, int n_q, const float *q_u, const float *q_v, const float *q_ur,
                                                       const float *q_vr, const int32_t *q_octave, const float *q_angle, const uint8_t *q_desc,
                                                       const uint8_t *q_has_obs, float th, int level_mode, int check_orientation, int32_t *cur_match) {
    return search_frame_fisheye_impl(m, left, nullptr, kps_right, n_right, cur_occupied, n_q, q_u, q_v, q_ur, q_vr, q_octave, q_angle, q_desc, q_has_obs, th,
                                     level_mode, check_orientation, cur_match);
}

extern "C" int orbx_search_by_projection_window(orbx_matcher *m, const orbx_frame_desc *frame, const uint8_t *occupied, int n_q,
                                                const float *q_x, const float *q_y, const float *q_r, const int32_t *q_min_level,
                                                const int32_t *q_max_level, const float *q_angle, const uint8_t *q_desc,
                                                const uint8_t *q_has_obs, float max_dist, int check_orientation, int32_t *match) {
    if (!m || !frame || frame->n < 0 || (!match && frame->n > 0) || n_q < 0) return ORBX_E_BAD_ARG;
    if (n_q > 0 && (!q_x || !q_y || !q_r || !q_min_level || !q_max_level || !q_desc || (check_orientation && !q_angle))) return ORBX_E_BAD_ARG;
    ProjArgs a = {frame, occupied, n_q, q_x, q_y, q_r, nullptr, q_min_level, q_max_level, q_desc, nullptr, q_has_obs,
                  q_angle, 2, 0.f, check_orientation, match, max_dist};
    return run_projection(m, a);
}

// ---------------------------------------------------------------------------------------------------------
// Device-resident frame handle (include/orbx.h, orbx_frame): ExtractORB -> UndistortKeyPoints -> AssignFeaturesToGrid once per frame, then every
// matcher of that frame reads the resident rows and grids.  Two kinds, monocular / rectified and fisheye-stereo (Frame::Nleft != -1: features
// [0, N_left) are the left camera's, [N_left, N) the right camera's, and every occupancy mask and match array uses that numbering), with ONE path each
// for what they share:
//   loads           the four public loaders describe their source (staged host arrays, an extractor's batch) and launch k_frame_prepare[_fisheye];
//                   one head for the host loads (frame_begin_host_load), one tail that writes ALL the bookkeeping (frame_loaded)
//   pending counts  orbx_frame::host_* / rows_* / adopt -- orbx_frame_count[s] (frame_count) and every call below learn N through adopt()
//   result tail     frame_fetch among a call's downloads, frame_take behind its synchronisation (PendingRows on h_match)
//   projection      the wrappers below hand the handle to run_projection / run_projection_twin, which read its side through frame_side
//   SearchLocalPoints  local_points_head / local_points_up / local_points_tail around each kind's records and kernels
//   BoW             further down (it needs the vocabulary): BowArrays on the handle, frame_compute_bow / frame_bow_ids_down,
//                   frame_search_by_bow_impl (host key frames) and frame_search_by_bow_resident (resident ones, run_bow_resident)
// ---------------------------------------------------------------------------------------------------------
extern "C" {

void orbx_frame_destroy(orbx_frame *f) {
    if (!f) return;
    (void)hipSetDevice(f->owner->device);
    (void)hipStreamSynchronize(f->owner->stream);   // nothing of the owner's may still read or write the buffers
    if (f->dev) (void)hipFree(f->dev);
    if (f->stage) (void)hipHostFree(f->stage);
    if (f->h_count) (void)hipHostFree(f->h_count);
    if (f->ev_src) (void)hipEventDestroy(f->ev_src);
    if (f->ev_done) (void)hipEventDestroy(f->ev_done);
    delete f;
}

int orbx_frame_create(orbx_matcher *m, int cap, orbx_frame **out) {
    if (!m || !out || cap < 1) return ORBX_E_BAD_ARG;
    *out = nullptr;
    if (cap > ORBX_MAX_FRAME_FEATURES) return ORBX_E_TOO_LARGE;
    ORBX_HIP(hipSetDevice(m->device));
    orbx_frame *f = new orbx_frame();
    f->owner = m;
    f->cap = cap;
    Layout L;
    f->off_kps = L.add(28 * (size_t)cap); f->off_desc = L.add(32 * (size_t)cap); f->off_ur = L.add(4 * (size_t)cap);
    f->off_count = L.add(8); f->off_scale = L.add(4 * (size_t)kFrameMaxLevels);
    f->off_gstart = L.add(2 * ((size_t)kGridCells + 1)); f->off_gorder = L.add(2 * (size_t)cap);
    const size_t off_gsr = L.add(2 * ((size_t)kGridCells + 1)), off_gor = L.add(2 * (size_t)cap);
    f->off_l2r = L.add(4 * (size_t)cap); f->off_r2l = L.add(4 * (size_t)cap);
    const size_t off_bw = L.add(4 * (size_t)cap), off_bn = L.add(4 * (size_t)cap), off_fn = L.add(4 * (size_t)cap), off_fp = L.add(4 * ((size_t)cap + 1)),
                 off_fi = L.add(4 * (size_t)cap), off_fm = L.add(16), off_an = L.add(4 * (size_t)cap);
    f->off_depth = L.add(4 * (size_t)cap); f->off_xy = L.add(8 * (size_t)cap);   // behind everything else: the other rows lie where they lay
    f->stage_bytes = L.used;   // the rows (keypoints, descriptors, mvuRight, mvDepth, raw (x, y); a fisheye frame's partners) at the device layout's offsets
    hipError_t e = hipMalloc((void **)&f->dev, L.used);
    if (e == hipSuccess) e = hipHostMalloc((void **)&f->stage, f->stage_bytes, hipHostMallocCoherent);   // read by k_xfer's lanes
    if (e == hipSuccess) e = hipHostMalloc((void **)&f->h_count, 64, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->ev_src, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->ev_done, hipEventDisableTiming);
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); orbx_frame_destroy(f); return ORBX_E_HIP; }
    f->kps = (orbx_keypoint *)(f->dev + f->off_kps); f->desc = f->dev + f->off_desc; f->u_right = (float *)(f->dev + f->off_ur);
    f->count = (int32_t *)(f->dev + f->off_count); f->scale = (float *)(f->dev + f->off_scale);
    f->gstart = (uint16_t *)(f->dev + f->off_gstart); f->gorder = (uint16_t *)(f->dev + f->off_gorder);
    f->bow.word = (int32_t *)(f->dev + off_bw); f->bow.node = (int32_t *)(f->dev + off_bn); f->bow.fv_node = (uint32_t *)(f->dev + off_fn);
    f->bow.fv_ptr = (int32_t *)(f->dev + off_fp); f->bow.fv_index = (int32_t *)(f->dev + off_fi); f->bow.fv_meta = (int32_t *)(f->dev + off_fm);
    f->bow.angle = (float *)(f->dev + off_an);
    f->gstart_r = (uint16_t *)(f->dev + off_gsr); f->gorder_r = (uint16_t *)(f->dev + off_gor);
    f->l2r = (int32_t *)(f->dev + f->off_l2r); f->r2l = (int32_t *)(f->dev + f->off_r2l);
    f->depth = (float *)(f->dev + f->off_depth); f->keys_xy = (float *)(f->dev + f->off_xy);
    f->n_known = true;   // an empty frame until the first load
    *out = f;
    return ORBX_OK;
}


// orbx_frame_load_host and, depth given, orbx_frame_load_host_stereo: the same load, the second with mvuRight required and mvDepth / the raw
// (x, y) rows in the same upload run (keys_xy NULL: the undistorted key points')
static int frame_load_host(orbx_frame *f, const orbx_frame_desc *d, const float *depth, const float *keys_xy) {
    orbx_matcher *m = f->owner;
    ORBX_TRY(frame_begin_host_load(f));
    const int n = d->n;
    const size_t b_kps = 28 * (size_t)n, b_desc = 32 * (size_t)n, b_ur = d->u_right ? 4 * (size_t)n : 0, b_dep = depth ? 4 * (size_t)n : 0;
    memcpy(f->stage + f->off_kps, d->keypoints_un, b_kps);
    memcpy(f->stage + f->off_desc, d->descriptors, b_desc);
    if (b_ur) memcpy(f->stage + f->off_ur, d->u_right, b_ur);
    if (b_dep) {
        memcpy(f->stage + f->off_depth, depth, b_dep);
        float *xy = reinterpret_cast<float *>(f->stage + f->off_xy);
        if (keys_xy) memcpy(xy, keys_xy, 2 * b_dep);
        else for (int i = 0; i < n; i++) { xy[2 * i] = d->keypoints_un[i].x; xy[2 * i + 1] = d->keypoints_un[i].y; }
    }
    // the rows in ONE k_xfer launch in the owner's queue (ORBX_MATCHER_DMA=1: by the DMA engine); count and scale factors travel as k_frame_prepare's arguments
    const orbx_matcher::Span rows[5] = {{f->off_kps, b_kps}, {f->off_desc, b_desc}, {f->off_ur, b_ur}, {f->off_depth, b_dep}, {f->off_xy, 2 * b_dep}};
    ORBX_TRY(m->upload_ranges(f->dev, f->stage, rows, depth ? 5 : 3));
    FramePrepare P;
    const float b[4] = {d->min_x, d->max_x, d->min_y, d->max_y};
    frame_prepare_common(f, P, 0, d->scale_factors, d->nlevels, b);
    P.n_host = n; P.cap = f->cap;
    hipLaunchKernelGGL(k_frame_prepare, dim3(1), dim3(64), 0, m->stream, P, grid_of(f->bounds));
    return frame_loaded(f, false, 0, n, 0, d->u_right != nullptr, depth != nullptr, true);
}

int orbx_frame_load_host(orbx_frame *f, const orbx_frame_desc *d) {
    if (!f || !d || d->n < 0 || (d->n > 0 && (!d->keypoints_un || !d->descriptors)) || !d->scale_factors || d->nlevels < 1 ||
        d->nlevels > kFrameMaxLevels)
        return ORBX_E_BAD_ARG;
    if (d->n > f->cap) return ORBX_E_TOO_LARGE;
    return frame_load_host(f, d, nullptr, nullptr);
}

int orbx_frame_load_host_stereo(orbx_frame *f, const orbx_frame_desc *d, const float *depth, const float *keys_xy) {
    if (!f || !d || d->n < 0 || (d->n > 0 && (!d->keypoints_un || !d->descriptors)) || !d->scale_factors || d->nlevels < 1 ||
        d->nlevels > kFrameMaxLevels || !d->u_right || !depth)
        return ORBX_E_BAD_ARG;
    if (d->n > f->cap) return ORBX_E_TOO_LARGE;
    return frame_load_host(f, d, depth, keys_xy);
}

// orbx_frame_load_batch and, stereo, orbx_frame_load_stereo_batch: the second copies mvuRight / mvDepth of the extractor's stereo / RGB-D stage and the raw
// (x, y) in the same launch, behind the stage
static int frame_load_batch(orbx_frame *f, orbx_extractor *ex, int frame, const float *bounds4, const float *scale_factors, int nlevels, bool stereo) {
    if (!f || !ex) return ORBX_E_BAD_ARG;
    orbx_matcher *m = f->owner;
    if (frame < 0 || frame >= ex->last_batch || ex->device != m->device || ex->cap > f->cap) return ORBX_E_BAD_ARG;
    // the stage's results must be those of the extractor's current batch
    if (stereo && (!ex->d_st_ur.p || !ex->d_st_depth.p || ex->st_seq == 0 || ex->st_seq != ex->batch_seq)) return ORBX_E_BAD_ARG;
    const float *sf = scale_factors ? scale_factors : ex->scale.data();
    const int nl = scale_factors ? nlevels : ex->prm.nlevels;
    if (nl < 1 || nl > kFrameMaxLevels || (!bounds4 && ex->width <= 0)) return ORBX_E_BAD_ARG;
    const float *b = bounds4 ? bounds4 : ex->bounds;   // mnMinX.. of the extractor's camera (orbx_set_camera) or the image rectangle
    ORBX_HIP(hipSetDevice(m->device));
    FramePrepare P;
    frame_prepare_common(f, P, 0, sf, nl, b);
    P.cap = f->cap;
    const size_t cap = (size_t)ex->cap;
    P.src_kps = (const orbx_keypoint *)ex->match_kps() + (size_t)frame * cap;   // mvKeysUn
    P.src_desc = (const uint8_t *)ex->d_desc.p + (size_t)frame * cap * 32;
    P.src_count = (const int32_t *)ex->d_count.p + frame;
    // the owner's stream waits for the extraction, the extractor's stream for the copy: no host synchronisation, and the next batch on `ex`
    // overwrites its outputs only after this frame holds its own copy
    ORBX_HIP(hipEventRecord(f->ev_src, ex->stream));
    ORBX_HIP(hipStreamWaitEvent(m->stream, f->ev_src, 0));
    const dim3 grid(1 + (unsigned)((cap + 255) / 256));
    if (stereo) {
        ORBX_HIP(hipStreamWaitEvent(m->stream, ex->ev_match, 0));   // the stage runs on the match stream
        FrameDepthRows D;
        D.src_ur = (const float *)ex->d_st_ur.p + (size_t)frame * cap; D.src_depth = (const float *)ex->d_st_depth.p + (size_t)frame * cap;
        D.src_raw = (const orbx_keypoint *)ex->d_kps.p + (size_t)frame * cap;   // mvKeys
        D.ur = f->u_right; D.depth = f->depth; D.keys_xy = f->keys_xy;
        hipLaunchKernelGGL(k_frame_prepare_stereo, grid, dim3(64), 0, m->stream, P, D, grid_of(f->bounds));
    } else {
        hipLaunchKernelGGL(k_frame_prepare, grid, dim3(64), 0, m->stream, P, grid_of(f->bounds));
    }
    ORBX_TRY(frame_loaded(f, false, 0, -1, -1, stereo, stereo, false));
    ORBX_HIP(hipStreamWaitEvent(ex->stream, f->ev_done, 0));
    if (stereo && ex->match_stream) ORBX_HIP(hipStreamWaitEvent(ex->match_stream, f->ev_done, 0));   // the next stage overwrites what the copy reads
    return ORBX_OK;
}

int orbx_frame_load_batch(orbx_frame *f, orbx_extractor *ex, int frame, const float *bounds4, const float *scale_factors, int nlevels) {
    return frame_load_batch(f, ex, frame, bounds4, scale_factors, nlevels, false);
}

int orbx_frame_load_stereo_batch(orbx_frame *f, orbx_extractor *left, int frame, const float *bounds4, const float *scale_factors, int nlevels) {
    return frame_load_batch(f, left, frame, bounds4, scale_factors, nlevels, true);
}

int orbx_frame_load_host_fisheye(orbx_frame *f, const orbx_frame_desc *left, const orbx_keypoint *kps_right, int n_right, const int32_t *l2r,
                                 const int32_t *r2l) {
    if (!f || !left || left->n < 0 || n_right < 0 || (left->n > 0 && (!left->keypoints_un || !l2r)) || (n_right > 0 && (!kps_right || !r2l)) ||
        (left->n + n_right > 0 && !left->descriptors) || !left->scale_factors || left->nlevels < 1 || left->nlevels > kFrameMaxLevels)
        return ORBX_E_BAD_ARG;
    const int nl = left->n, nr = n_right, N = nl + nr;
    // the partners index device memory: checked before anything is enqueued
    for (int i = 0; i < nl; i++) if (l2r[i] < -1 || l2r[i] >= nr) return ORBX_E_BAD_ARG;
    for (int j = 0; j < nr; j++) if (r2l[j] < -1 || r2l[j] >= nl) return ORBX_E_BAD_ARG;
    if (N > f->cap) return ORBX_E_TOO_LARGE;
    orbx_matcher *m = f->owner;
    ORBX_TRY(frame_begin_host_load(f));
    // rows in place: left at 0, right at roff = N_left, so the descriptors of all N features are one run
    const size_t b_kl = 28 * (size_t)nl, b_kr = 28 * (size_t)nr, b_desc = 32 * (size_t)N, b_l2r = 4 * (size_t)nl, b_r2l = 4 * (size_t)nr;
    memcpy(f->stage + f->off_kps, left->keypoints_un, b_kl);
    memcpy(f->stage + f->off_kps + b_kl, kps_right, b_kr);
    memcpy(f->stage + f->off_desc, left->descriptors, b_desc);
    memcpy(f->stage + f->off_l2r, l2r, b_l2r);
    memcpy(f->stage + f->off_r2l, r2l, b_r2l);
    const orbx_matcher::Span rows[4] = {{f->off_kps, b_kl + b_kr}, {f->off_desc, b_desc}, {f->off_l2r, b_l2r}, {f->off_r2l, b_r2l}};
    ORBX_TRY(m->upload_ranges(f->dev, f->stage, rows, 4));
    const float b[4] = {left->min_x, left->max_x, left->min_y, left->max_y};
    FisheyePrepare P;
    frame_prepare_common(f, P, nl, left->scale_factors, left->nlevels, b);
    P.n_host[0] = nl; P.n_host[1] = nr; P.cap_side[0] = nl; P.cap_side[1] = nr;
    P.l2r = f->l2r; P.r2l = f->r2l;
    hipLaunchKernelGGL(k_frame_prepare_fisheye, dim3(2), dim3(64), 0, m->stream, P, grid_of(f->bounds));
    return frame_loaded(f, true, nl, nl, nr, false, false, true);
}

int orbx_frame_load_stereo_fisheye_batch(orbx_frame *f, orbx_extractor *L, orbx_extractor *R, int frame, const float *bounds4,
                                         const float *scale_factors, int nlevels) {
    if (!f || !L || !R) return ORBX_E_BAD_ARG;
    orbx_matcher *m = f->owner;
    // the stage's results must be those of the extractors' current batches
    if (L->sf_batch <= 0 || !L->ev_sf || L->sf_right != R || L->sf_seq_l != L->batch_seq || L->sf_seq_r != R->batch_seq) return ORBX_E_BAD_ARG;
    if (frame < 0 || frame >= L->sf_batch || frame >= L->last_batch || L->device != m->device || R->device != m->device) return ORBX_E_BAD_ARG;
    const int capL = L->sf_capL, capR = L->sf_capR;
    if (capL != L->cap || capR != R->cap || (size_t)capL + (size_t)capR > (size_t)f->cap) return ORBX_E_BAD_ARG;
    const float *sf = scale_factors ? scale_factors : L->scale.data();
    const int nl = scale_factors ? nlevels : L->prm.nlevels;
    if (nl < 1 || nl > kFrameMaxLevels || (!bounds4 && L->width <= 0)) return ORBX_E_BAD_ARG;
    const float *b = bounds4 ? bounds4 : L->bounds;
    ORBX_HIP(hipSetDevice(m->device));
    FisheyePrepare P;
    frame_prepare_common(f, P, capL, sf, nl, b);
    const size_t fr = (size_t)frame;
    P.src_kps[0] = (const orbx_keypoint *)L->d_kps.p + fr * capL;   // mvKeys: the raw keypoints k_tri_kb8_stereo read
    P.src_kps[1] = (const orbx_keypoint *)R->d_kps.p + fr * capR;
    P.src_desc[0] = (const uint8_t *)L->d_desc.p + fr * capL * 32;
    P.src_desc[1] = (const uint8_t *)R->d_desc.p + fr * capR * 32;
    P.src_count[0] = (const int32_t *)L->d_count.p + fr;
    P.src_count[1] = (const int32_t *)R->d_count.p + fr;
    P.src_l2r = (const int32_t *)L->d_sf_l2r.p + fr * capL;
    P.src_r2l = (const int32_t *)L->d_sf_r2l.p + fr * capR;
    P.cap_side[0] = capL; P.cap_side[1] = capR;
    P.l2r = f->l2r; P.r2l = f->r2l;
    // the owner's stream waits for the stage (which waited for both extractions); both extractors' next batches and the left extractor's next
    // stage wait for the copy: no host synchronisation
    ORBX_HIP(hipStreamWaitEvent(m->stream, L->ev_sf, 0));
    hipLaunchKernelGGL(k_frame_prepare_fisheye, dim3(2 + (unsigned)((std::max(capL, capR) + 255) / 256)), dim3(64), 0, m->stream, P, grid_of(f->bounds));
    ORBX_TRY(frame_loaded(f, true, capL, -1, -1, false, false, false));
    ORBX_HIP(hipStreamWaitEvent(L->stream, f->ev_done, 0));
    ORBX_HIP(hipStreamWaitEvent(R->stream, f->ev_done, 0));
    if (L->match_stream) ORBX_HIP(hipStreamWaitEvent(L->match_stream, f->ev_done, 0));
    return ORBX_OK;
}

int orbx_frame_count(orbx_frame *f, int *n) {
    if (!f || !n) return ORBX_E_BAD_ARG;
    return frame_count(f, n);
}

int orbx_frame_counts(orbx_frame *f, int *n_left, int *n_right) {
    if (!f) return ORBX_E_BAD_ARG;
    int n = 0;
    const int rc = frame_count(f, &n);
    if (rc != ORBX_OK) return rc;
    if (n_left) *n_left = f->n_left;     // (a monocular frame: N, -1)
    if (n_right) *n_right = f->n_right;
    return ORBX_OK;
}

// Frame::UnprojectStereo for every feature of a frame that holds mvDepth (k_unproject_stereo): one launch, one download run (mvuRight, mvDepth and the
// points side by side in the arena, with N while it is pending), one synchronisation.  pos rows are written where depth > 0 only.
int orbx_frame_unproject_stereo(orbx_matcher *m, orbx_frame *f, const orbx_new_points_view *view, float *u_right, float *depth, float *pos,
                                int *n_with_depth) {
    if (!m || !f || !view || f->owner != m || f->fisheye || !f->loaded || !f->has_depth) return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(m->device));
    const int nr = f->rows_n();
    if (nr == 0) { if (n_with_depth) *n_with_depth = 0; return ORBX_OK; }
    UnprojectStereo U;
    ORBX_TRY(m->carve([&](Carve &A) {
        U.out_ur = A.take<float>((size_t)nr); U.out_depth = A.take<float>((size_t)nr); U.out_pos = A.take<float>(3 * (size_t)nr);
    }));
    U.kps = f->kps; U.u_right = f->u_right; U.depth = f->depth; U.count = f->count; U.cap = nr;
    memcpy(U.Rcw, view->Rcw, sizeof(U.Rcw)); memcpy(U.Ow, view->Ow, sizeof(U.Ow));
    U.fx = view->fx; U.fy = view->fy; U.cx = view->cx; U.cy = view->cy;
    hipLaunchKernelGGL(k_unproject_stereo, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, m->exec(), U);
    ORBX_HIP(hipGetLastError());
    // N known: mvuRight and mvDepth go straight to the caller's arrays where they are given; the points always land here first (only rows with depth
    // are handed out), and so does whatever has no destination yet.  Rows beyond N are never written by the kernel and never read here.
    const bool known = f->n_known;
    const bool ur_direct = known && u_right, dep_direct = known && depth;
    const size_t n_land = (ur_direct ? 0 : (size_t)nr) + (dep_direct ? 0 : (size_t)nr) + 3 * (size_t)nr;
    std::unique_ptr<float[]> land(new float[n_land]);
    float *l_pos = land.get(), *l_ur = ur_direct ? u_right : l_pos + 3 * (size_t)nr, *l_dep = dep_direct ? depth : l_pos + 3 * (size_t)nr + (ur_direct ? 0 : (size_t)nr);
    ORBX_TRY(m->d2h(l_ur, U.out_ur, 4 * (size_t)nr));
    ORBX_TRY(m->d2h(l_dep, U.out_depth, 4 * (size_t)nr));
    ORBX_TRY(m->d2h(l_pos, U.out_pos, 12 * (size_t)nr));
    if (!known) ORBX_TRY(f->fetch_count());
    ORBX_TRY(m->sync_and_deliver());
    if (!known) f->adopt_count();
    const int n = f->n;
    if (u_right && !ur_direct) memcpy(u_right, l_ur, 4 * (size_t)n);
    if (depth && !dep_direct) memcpy(depth, l_dep, 4 * (size_t)n);
    int with = 0;
    for (int i = 0; i < n; i++) {
        if (!(l_dep[i] > 0.f)) continue;
        with++;
        if (pos) memcpy(pos + 3 * (size_t)i, l_pos + 3 * (size_t)i, 12);
    }
    if (n_with_depth) *n_with_depth = with;
    return ORBX_OK;
}

// the orbx_frame_desc the host-side window setup reads (scale factors, levels, bounds); rows are never read from it
static orbx_frame_desc frame_desc_of(const orbx_frame *f) {
    orbx_frame_desc d;
    memset(&d, 0, sizeof(d));
    d.n = f->rows_n();
    d.min_x = f->bounds[0]; d.max_x = f->bounds[1]; d.min_y = f->bounds[2]; d.max_y = f->bounds[3];
    d.scale_factors = f->scale_h.data(); d.nlevels = f->nlevels;
    d.u_right = f->has_ur ? f->u_right : nullptr;
    return d;
}

int orbx_frame_search_by_projection_mappoints(orbx_matcher *m, orbx_frame *frame, const uint8_t *frame_occupied, int n_mp, const float *proj_x,
                                              const float *proj_y, const float *proj_xr, const int32_t *pred_level, const float *view_cos,
                                              const uint8_t *mp_desc, const uint8_t *mp_in_view, const uint8_t *mp_has_obs, float th, float nnratio,
                                              int32_t *frame_match) {
    if (!m || !frame || frame->owner != m || frame->fisheye || !frame_match) return ORBX_E_BAD_ARG;   // (a fisheye frame: the _fisheye forms)
    const orbx_frame_desc d = frame_desc_of(frame);
    return search_mappoints_impl(m, &d, frame, frame_occupied, n_mp, proj_x, proj_y, proj_xr, pred_level, view_cos, mp_desc, mp_in_view, mp_has_obs,
                                 th, nnratio, frame_match);
}

int orbx_frame_search_by_projection_frame(orbx_matcher *m, orbx_frame *cur, const uint8_t *cur_occupied, int n_q, const float *q_u, const float *q_v,
                                          const float *q_ur, const int32_t *q_octave, const float *q_angle, const uint8_t *q_desc,
                                          const uint8_t *q_has_obs, float th, int level_mode, int check_orientation, int32_t *cur_match) {
    if (!m || !cur || cur->owner != m || cur->fisheye || !cur_match) return ORBX_E_BAD_ARG;
    const orbx_frame_desc d = frame_desc_of(cur);
    return search_frame_impl(m, &d, cur, cur_occupied, n_q, q_u, q_v, q_ur, q_octave, q_angle, q_desc, q_has_obs, th, level_mode, check_orientation,
                             cur_match);
}

int orbx_frame_search_by_projection_mappoints_fisheye(orbx_matcher *m, orbx_frame *f, const uint8_t *frame_occupied, int n_mp,
                                                      const uint8_t *in_view, const float *proj_x, const float *proj_y, const int32_t *pred_level,
                                                      const float *view_cos, const uint8_t *in_view_r, const float *proj_xr, const float *proj_yr,
                                                      const int32_t *pred_level_r, const float *view_cos_r, const uint8_t *mp_desc,
                                                      const uint8_t *mp_has_obs, float th, float nnratio, int32_t *frame_match) {
    if (!m || !f || f->owner != m || !f->fisheye || !frame_match) return ORBX_E_BAD_ARG;
    const orbx_frame_desc d = frame_desc_of(f);
    return search_mappoints_fisheye_impl(m, &d, f, nullptr, 0, nullptr, nullptr, frame_occupied, n_mp, in_view, proj_x, proj_y, pred_level, view_cos,
                                         in_view_r, proj_xr, proj_yr, pred_level_r, view_cos_r, mp_desc, mp_has_obs, th, nnratio, frame_match);
}

int orbx_frame_search_by_projection_frame_fisheye(orbx_matcher *m, orbx_frame *f, const uint8_t *cur_occupied, int n_q, const float *q_u,
                                                  const float *q_v, const float *q_ur, const float *q_vr, const int32_t *q_octave,
                                                  const float *q_angle, const uint8_t *q_desc, const uint8_t *q_has_obs, float th, int level_mode,
                                                  int check_orientation, int32_t *cur_match) {
    if (!m || !f || f->owner != m || !f->fisheye || !cur_match) return ORBX_E_BAD_ARG;
    const orbx_frame_desc d = frame_desc_of(f);
    return search_frame_fisheye_impl(m, &d, f, nullptr, 0, cur_occupied, n_q, q_u, q_v, q_ur, q_vr, q_octave, q_angle, q_desc, q_has_obs, th, level_mode,
                                     check_orientation, cur_match);
}

}  // extern "C"

// the same on a resident frame (Tracking::Relocalization's second stage, Tracking.cc:3726,3740): the frame's rows and grid are the handle's
extern "C" int orbx_frame_search_by_projection_window(orbx_matcher *m, orbx_frame *f, const uint8_t *occupied, int n_q, const float *q_x,
                                                      const float *q_y, const float *q_r, const int32_t *q_min_level, const int32_t *q_max_level,
                                                      const float *q_angle, const uint8_t *q_desc, const uint8_t *q_has_obs, float max_dist,
                                                      int check_orientation, int32_t *match) {
    if (!m || !f || f->owner != m || f->fisheye || !match || n_q < 0) return ORBX_E_BAD_ARG;
    if (n_q > 0 && (!q_x || !q_y || !q_r || !q_min_level || !q_max_level || !q_desc || (check_orientation && !q_angle))) return ORBX_E_BAD_ARG;
    const orbx_frame_desc d = frame_desc_of(f);
    ProjArgs a = {&d, occupied, n_q, q_x, q_y, q_r, nullptr, q_min_level, q_max_level, q_desc, nullptr, q_has_obs,
                  q_angle, 2, 0.f, check_orientation, match, max_dist};
    return run_projection(m, a, f);
}

// the same on a resident fisheye-stereo frame: Relocalization's SearchByProjection(F, pKF, sFound, th, ORBdist) calls GetFeaturesInArea with the
// default bRight = false, so only the LEFT camera is searched (raw mvKeys, the left grid, N_left = count[0] on the device); occupied / match cover
// all N features and the right camera's entries of match stay -1
extern "C" int orbx_frame_search_by_projection_window_fisheye(orbx_matcher *m, orbx_frame *f, const uint8_t *occupied, int n_q, const float *q_x,
                                                              const float *q_y, const float *q_r, const int32_t *q_min_level,
                                                              const int32_t *q_max_level, const float *q_angle, const uint8_t *q_desc,
                                                              const uint8_t *q_has_obs, float max_dist, int check_orientation, int32_t *match) {
    if (!m || !f || f->owner != m || !f->fisheye || !match || n_q < 0) return ORBX_E_BAD_ARG;
    if (n_q > 0 && (!q_x || !q_y || !q_r || !q_min_level || !q_max_level || !q_desc || (check_orientation && !q_angle))) return ORBX_E_BAD_ARG;
    const orbx_frame_desc d = frame_desc_of(f);
    ProjArgs a = {&d, occupied, n_q, q_x, q_y, q_r, nullptr, q_min_level, q_max_level, q_desc, nullptr, q_has_obs,
                  q_angle, 2, 0.f, check_orientation, match, max_dist};
    return run_projection(m, a, f, true);
}

// ---------------------------------------------------------------------------------------------------------
// The device-resident map-point table (include/orbx.h, orbx_map) and the ONE map-point source of the eight one-call searches (MapPoints): host
// arrays, uploaded as ever, or (map, ids), gathered into the same five arena buffers by k_map_gather.  Everything behind those buffers is shared.
// ---------------------------------------------------------------------------------------------------------
struct orbx_map {
    int device = 0, capacity = 0;
    uint4 *rec = nullptr;              // [capacity] 64-byte records (matcher_kernels.hip.h, MapRows)
    hipEvent_t written = nullptr;      // recorded behind the newest update, on the updating context's stream
    std::mutex mu;                     // guards everything below and the re-recording of `written`
    uint64_t write_seq = 0;            // updates recorded so far
    uint64_t seen_seq = 0;             // the newest update a reading call has waited for AND synchronised behind: nobody needs to wait for it again
    uint8_t *live = nullptr;           // [capacity] the slot has been written whole since its creation / its erase
    uint32_t *stamp = nullptr;         // [capacity] the last checking pass that named the slot (duplicate detection)
    uint32_t stamp_now = 0;
};

namespace {

// every id in [0, capacity) and live; unique: named once (the stamp array).  Under map->mu.
bool map_ids_ok(orbx_map *map, int n, const int32_t *ids, bool unique, bool none_ok = false) {
    if (unique && ++map->stamp_now == 0) { memset(map->stamp, 0, sizeof(uint32_t) * (size_t)map->capacity); map->stamp_now = 1; }
    for (int j = 0; j < n; j++) {
        const int32_t id = ids[j];
        if (none_ok && id == -1) continue;   // (the per-feature id rows of the track forms: no map point here)
        if (id < 0 || id >= map->capacity || !map->live[id]) return false;
        if (unique) {
            if (map->stamp[id] == map->stamp_now) return false;
            map->stamp[id] = map->stamp_now;
        }
    }
    return true;
}

// The map points of a call: n rows of host arrays, or n slots of a table (map != NULL; the five pointers are NULL then).
struct MapPoints { int n; const float *pos, *normal, *min_dist, *max_dist; const uint8_t *desc; orbx_map *map; const int32_t *ids; };
struct MapPointsDev { float *pos, *normal, *min_dist, *max_dist; uint8_t *desc; int32_t *ids; };

inline MapPoints map_points_of(int n, orbx_map *map, const int32_t *ids) { return MapPoints{n, nullptr, nullptr, nullptr, nullptr, nullptr, map, ids}; }
// a table source needs its table: a `_map` entry point given map = NULL is refused, not read as "flat arrays, all NULL"
inline bool map_form_ok(const orbx_map *map, int n) { return map != nullptr || n <= 0; }

// what a call checks of its n > 0 map points before it enqueues anything: the five arrays, or the table's device and every id
bool map_points_ok(const orbx_matcher *m, const MapPoints &S) {
    if (!S.map) return S.pos && S.normal && S.min_dist && S.max_dist && S.desc;
    if (S.map->device != m->device || !S.ids) return false;
    std::lock_guard<std::mutex> lock(S.map->mu);
    return map_ids_ok(S.map, S.n, S.ids, false);
}
// the five device arrays every projection kernel reads, first in the call's arena: uploaded from the host arrays, or only carved, with the ids behind
// them -- at the head of the call's one upload run
MapPointsDev map_points_up(Carve &A, const MapPoints &S) {
    const size_t q = (size_t)S.n;
    MapPointsDev d;
    d.pos = A.up(S.pos, 3 * q); d.normal = A.up(S.normal, 3 * q); d.min_dist = A.up(S.min_dist, q); d.max_dist = A.up(S.max_dist, q);
    d.desc = A.up(S.desc, 32 * q);
    d.ids = S.map ? A.up(S.ids, q) : nullptr;
    return d;
}
// the order every reader of a table keeps against its updates: the context's stream waits for `written` unless a reader has synchronised behind the
// newest update.  *seq: what map_points_done() reports once the call has synchronised.
int map_wait_written(orbx_matcher *m, orbx_map *map, uint64_t *seq) {
    std::lock_guard<std::mutex> lock(map->mu);
    if (map->seen_seq < map->write_seq) ORBX_HIP(hipStreamWaitEvent(m->stream, map->written, 0));
    *seq = map->write_seq;
    return ORBX_OK;
}
const uint4 *map_records(const orbx_map *map, int *cap) { *cap = map->capacity; return map->rec; }
// a table source: the context's stream waits for `written` (unless a reader has synchronised behind it), then k_map_gather fills the five arrays.
// *seq: what map_points_done() reports once the call has synchronised.  Host arrays: nothing.
int map_points_gather(orbx_matcher *m, const MapPoints &S, const MapPointsDev &D, uint64_t *seq) {
    *seq = 0;
    if (!S.map || S.n <= 0) return ORBX_OK;
    ORBX_TRY(map_wait_written(m, S.map, seq));
    const MapRows G = {S.map->rec, D.ids, S.n, S.map->capacity, D.pos, D.normal, D.min_dist, D.max_dist, D.desc};
    hipLaunchKernelGGL(k_map_gather, dim3((unsigned)((S.n + 63) / 64)), dim3(256), 0, m->exec(), G);
    return ORBX_OK;
}
inline void map_points_done(const MapPoints &S, uint64_t seq) {   // after the call's synchronisation
    if (!S.map || seq == 0) return;
    std::lock_guard<std::mutex> lock(S.map->mu);
    S.map->seen_seq = std::max(S.map->seen_seq, seq);
}

}  // namespace

extern "C" {

int orbx_map_create(int device, int capacity, orbx_map **out) {
    if (!out) return ORBX_E_BAD_ARG;
    *out = nullptr;
    if (capacity < 1) return ORBX_E_BAD_ARG;
    if (capacity > ORBX_MAX_MAP_POINTS) return ORBX_E_TOO_LARGE;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        set_error("no usable HIP device (liborbx has no CPU fallback)");
        return ORBX_E_NO_DEVICE;
    }
    ORBX_HIP(hipSetDevice(device));
    std::unique_ptr<orbx_map> map(new orbx_map());
    map->device = device; map->capacity = capacity;
    map->live = static_cast<uint8_t *>(calloc((size_t)capacity, 1));
    map->stamp = static_cast<uint32_t *>(calloc((size_t)capacity, sizeof(uint32_t)));
    hipError_t e = hipMalloc((void **)&map->rec, 64 * (size_t)capacity);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&map->written, hipEventDisableTiming);
    if (e != hipSuccess || !map->live || !map->stamp) {
        set_error(e != hipSuccess ? hipGetErrorString(e) : "out of host memory");
        orbx_map_destroy(map.release());
        return ORBX_E_HIP;
    }
    *out = map.release();
    return ORBX_OK;
}

void orbx_map_destroy(orbx_map *map) {
    if (!map) return;
    (void)hipSetDevice(map->device);
    if (map->written) { (void)hipEventSynchronize(map->written); (void)hipEventDestroy(map->written); }   // the last update has run; no search is running (the caller's contract)
    if (map->rec) (void)hipFree(map->rec);
    free(map->live);
    free(map->stamp);
    delete map;
}

int orbx_map_update(orbx_matcher *m, orbx_map *map, int n, const int32_t *ids, const float *pos, const float *normal, const float *min_dist,
                    const float *max_dist, const uint8_t *desc) {
    if (!m || !map || n < 0 || map->device != m->device) return ORBX_E_BAD_ARG;
    if (n == 0) return ORBX_OK;
    if (!ids) return ORBX_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(map->mu);
    // everything is checked before anything is enqueued: range, one mention per id, and all five fields for a slot that is not live
    const bool whole = pos && normal && min_dist && max_dist && desc;
    if (++map->stamp_now == 0) { memset(map->stamp, 0, sizeof(uint32_t) * (size_t)map->capacity); map->stamp_now = 1; }
    for (int j = 0; j < n; j++) {
        const int32_t id = ids[j];
        if (id < 0 || id >= map->capacity || map->stamp[id] == map->stamp_now || (!whole && !map->live[id])) return ORBX_E_BAD_ARG;
        map->stamp[id] = map->stamp_now;
    }
    if (!pos && !normal && !min_dist && !max_dist && !desc) return ORBX_OK;   // every field kept
    ORBX_HIP(hipSetDevice(m->device));
    const size_t q = (size_t)n;
    MapRows S;
    memset(&S, 0, sizeof(S));
    S.rec = map->rec; S.n = n; S.cap = map->capacity;
    ORBX_TRY(m->carve([&](Carve &A) {   // one run
        S.ids = A.up(ids, q);
        S.pos = A.up_opt(pos, 3 * q); S.normal = A.up_opt(normal, 3 * q); S.min_dist = A.up_opt(min_dist, q); S.max_dist = A.up_opt(max_dist, q);
        S.desc = A.up_opt(desc, 32 * q);
    }));
    if (map->write_seq > 0) ORBX_HIP(hipStreamWaitEvent(m->stream, map->written, 0));
    hipLaunchKernelGGL(k_map_scatter, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, m->exec(), S);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipEventRecord(map->written, m->stream));
    map->write_seq++;
    for (int j = 0; j < n; j++) map->live[ids[j]] = 1;
    return ORBX_OK;
}

int orbx_map_erase(orbx_map *map, int n, const int32_t *ids) {
    if (!map || n < 0) return ORBX_E_BAD_ARG;
    if (n == 0) return ORBX_OK;
    if (!ids) return ORBX_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(map->mu);
    if (!map_ids_ok(map, n, ids, false)) return ORBX_E_BAD_ARG;
    for (int j = 0; j < n; j++) map->live[ids[j]] = 0;
    return ORBX_OK;
}

int orbx_map_read(orbx_matcher *m, orbx_map *map, int n, const int32_t *ids, float *pos, float *normal, float *min_dist, float *max_dist,
                  uint8_t *desc) {
    if (!m || !map || n < 0) return ORBX_E_BAD_ARG;
    if (n == 0) return map->device == m->device ? ORBX_OK : ORBX_E_BAD_ARG;
    const MapPoints S = map_points_of(n, map, ids);
    if (!map_points_ok(m, S)) return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(m->device));
    MapPointsDev D;
    ORBX_TRY(m->carve([&](Carve &A) { D = map_points_up(A, S); }));
    uint64_t seq = 0;
    ORBX_TRY(map_points_gather(m, S, D, &seq));
    ORBX_HIP(hipGetLastError());
    const size_t q = (size_t)n;
    if (pos) ORBX_TRY(m->d2h(pos, D.pos, 12 * q));
    if (normal) ORBX_TRY(m->d2h(normal, D.normal, 12 * q));
    if (min_dist) ORBX_TRY(m->d2h(min_dist, D.min_dist, 4 * q));
    if (max_dist) ORBX_TRY(m->d2h(max_dist, D.max_dist, 4 * q));
    if (desc) ORBX_TRY(m->d2h(desc, D.desc, 32 * q));
    ORBX_TRY(m->sync_and_deliver());
    map_points_done(S, seq);
    return ORBX_OK;
}

}  // extern "C"

namespace {

// ---- Tracking::SearchLocalPoints on a resident frame of either kind.  The two forms share their head, the upload of the map points and their tail;
// the projection records, the frustum and window kernels and resolve-versus-twin are each kind's own, and each carves its arena in its own order.
struct LocalPoints { MapPoints src; const uint8_t *eligible, *has_obs; const float *track_depth; };   // (track_depth: a rig's only)
struct LocalPointsDev : MapPointsDev { float *track_depth; uint8_t *eligible, *has_obs, *occupied; };

// The head: the argument checks both forms share (have_view: the form's camera arguments are there), N where the call needs it on the host -- *n = -1
// while it stays on the device -- and frame_match's -1 fill.  The caller returns 0 behind it when there are no map points.
int local_points_head(orbx_matcher *m, orbx_frame *f, bool fisheye, bool have_view, const LocalPoints &mp, const uint8_t *occupied, const uint8_t *in_view,
                      int32_t *frame_match, int *n) {
    if (!m || !f || f->owner != m || f->fisheye != fisheye || !have_view || mp.src.n < 0 || !frame_match) return ORBX_E_BAD_ARG;
    if (mp.src.n > 0 && (!in_view || !map_points_ok(m, mp.src))) return ORBX_E_BAD_ARG;
    *n = -1;
    if (f->n_known || occupied || mp.src.n == 0) ORBX_TRY(frame_count(f, n));   // the mask holds N entries
    for (int i = 0; i < *n; i++) frame_match[i] = -1;
    return ORBX_OK;
}
// the first buffers of both arenas: the map points and the occupancy mask, one run of uploads
LocalPointsDev local_points_up(Carve &A, const LocalPoints &mp, const uint8_t *occupied, int n) {
    const size_t q = (size_t)mp.src.n;
    LocalPointsDev d;
    static_cast<MapPointsDev &>(d) = map_points_up(A, mp.src);
    d.eligible = A.up_opt(mp.eligible, q); d.has_obs = A.up_opt(mp.has_obs, q); d.track_depth = A.up_opt(mp.track_depth, q);
    d.occupied = n > 0 ? A.up_opt(occupied, (size_t)n) : nullptr;
    return d;
}
// The tail: mbTrackInView [n_view], then -- unless the frame is empty (match == false: the frustum test only) -- the matches, the count(s) while
// pending and nmatches; one synchronisation.  Returns nmatches.
int local_points_tail(orbx_matcher *m, orbx_frame *f, bool match, uint8_t *in_view, const uint8_t *d_in_view, size_t n_view, const int32_t *d_match, int nc,
                      const int32_t *d_nmatches, int32_t *frame_match) {
    ORBX_HIP(hipGetLastError());
    int32_t nm = 0;
    ORBX_TRY(m->d2h(in_view, d_in_view, n_view));
    const Rows rows = {d_match, 1, nc, frame_match, 0};
    if (match) { ORBX_TRY(frame_fetch(f, &rows, 1)); ORBX_TRY(m->d2h(&nm, d_nmatches, 4)); }
    ORBX_TRY(m->sync_and_deliver());
    frame_take(f, &rows, 1);
    return nm;
}

}  // namespace

// Tracking::SearchLocalPoints on a resident frame (Tracking.cc:3339-3413): Frame::isInFrustum (Frame.cc:512-575) of every local map point, the
// window setup and SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) (ORBmatcher.cc:43-213, Nleft == -1) in one call: the projection
// records stay in the call's arena, one transfer up, one down, one synchronisation.
static int frame_search_local_points_impl(orbx_matcher *m, orbx_frame *f, const uint8_t *frame_occupied, const orbx_camera *cam,
                                          const orbx_frame_pose *pose, float log_scale_factor, float viewing_cos_limit, const MapPoints &src,
                                          const uint8_t *eligible, const uint8_t *has_obs, float th, float nnratio, int far_points,
                                          float th_far_points, uint8_t *in_view, int32_t *frame_match) {
    const LocalPoints mp = {src, eligible, has_obs, nullptr};
    const int n_mp = src.n;
    int n = -1;
    const int rc = local_points_head(m, f, false, cam && pose, mp, frame_occupied, in_view, frame_match, &n);
    if (rc != ORBX_OK || n_mp == 0) return rc;
    const int nc = f->rows_n();
    if (nc > kMaxResolveFeatures) return ORBX_E_TOO_LARGE;
    ORBX_HIP(hipSetDevice(m->device));
    const size_t q = (size_t)n_mp;
    const FrustumFrame FF = frustum_frame(cam, pose, f->bounds, log_scale_factor, f->nlevels, viewing_cos_limit);
    const int32_t cnts[2] = {n, n_mp};
    WindowProblem P;
    memset(&P, 0, sizeof(P));
    ResolveProblem R;
    memset(&R, 0, sizeof(R));
    LocalPointsDev D;
    float *dx, *dy, *dxr, *dd, *dvc, *dqr;
    uint8_t *div, *dvalid, *div_out;
    int32_t *dcnt, *dl, *dqmin, *dqmax;
    FrustumFrame *dF;
    WindowProblem *dP;
    ResolveProblem *dR;
    ORBX_TRY(m->carve([&](Carve &A) {
        // inputs (one run of the arena)
        D = local_points_up(A, mp, frame_occupied, n);
        dF = A.up(&FF, 1);
        dcnt = A.up(cnts, 2, 2);
        dP = A.take<WindowProblem>(1);
        dR = A.take<ResolveProblem>(1);
        // the projection records and the windows: device only
        div = A.take<uint8_t>(q);
        dx = A.take<float>(q); dy = A.take<float>(q); dxr = A.take<float>(q); dd = A.take<float>(q); dvc = A.take<float>(q);
        dl = A.take<int32_t>(q);
        dqr = A.take<float>(q);
        dqmin = A.take<int32_t>(q); dqmax = A.take<int32_t>(q);
        dvalid = A.take<uint8_t>(q);
        P.keys = A.take<u64>(q * kTopK); P.meta = A.take<int32_t>(q);
        R.entries = A.take<int32_t>(q);
        // the downloads side by side: mbTrackInView, the matches, nmatches
        div_out = A.take<uint8_t>(q);
        R.match = A.take<int32_t>(nc);
        R.nmatches = A.take<int32_t>(1);
    }));
    frame_side(f, false, P);
    P.nq_ptr = dcnt + 1; P.occupied0 = D.occupied;
    if (f->has_ur) { P.u_right = f->u_right; P.qxr = dxr; }   // mTrackProjXR against mvuRight (ORBmatcher.cc:92-97)
    P.qx = dx; P.qy = dy; P.qr = dqr; P.qmin = dqmin; P.qmax = dqmax; P.qdesc = D.desc; P.qvalid = dvalid;
    R.q_has_obs = D.has_obs;
    R.mode = 1; R.nnratio = nnratio; R.max_dist = (float)ORBX_TH_HIGH; R.cleared_value = -2;
    ORBX_TRY(m->h2d(dP, &P, sizeof(P))); ORBX_TRY(m->h2d(dR, &R, sizeof(R)));
    uint64_t seq = 0;
    ORBX_TRY(map_points_gather(m, src, D, &seq));
    hipLaunchKernelGGL(k_in_frustum, dim3((n_mp + 255) / 256, 1), dim3(256), 0, m->exec(), (const FrustumFrame *)dF, n_mp, (const float *)D.pos,
                       (const float *)D.normal, (const float *)D.min_dist, (const float *)D.max_dist, div, dx, dy, dxr, dd, dl, dvc);
    hipLaunchKernelGGL(k_local_windows, dim3((n_mp + 255) / 256), dim3(256), 0, m->exec(), n_mp, (const uint8_t *)div, (const uint8_t *)D.eligible,
                       (const int32_t *)dl, (const float *)dvc, (const float *)dd, (const float *)f->scale, f->nlevels, th, far_points ? 1 : 0,
                       th_far_points, dqr, dqmin, dqmax, dvalid, div_out);
    const bool match = n != 0;   // (an empty frame: isInFrustum only)
    if (match) {
        const GridParams g = grid_of(f->bounds);
        ORBX_LAUNCH_WINDOW_BEST2(n_mp, 1, m->exec(), dP, g);
        const int rr = launch_resolve<false>(1, m->exec(), dP, dR, g, nc, n_mp, 4);
        if (rr != ORBX_OK) return rr;
    }
    const int nm = local_points_tail(m, f, match, in_view, div_out, q, R.match, nc, R.nmatches, frame_match);
    if (nm >= 0) map_points_done(src, seq);
    return nm;
}

extern "C" int orbx_frame_search_local_points(orbx_matcher *m, orbx_frame *f, const uint8_t *frame_occupied, const orbx_camera *cam,
                                              const orbx_frame_pose *pose, float log_scale_factor, float viewing_cos_limit, int n_mp, const float *pos,
                                              const float *normal, const float *min_dist, const float *max_dist, const uint8_t *mp_desc,
                                              const uint8_t *eligible, const uint8_t *has_obs, float th, float nnratio, int far_points,
                                              float th_far_points, uint8_t *in_view, int32_t *frame_match) {
    return frame_search_local_points_impl(m, f, frame_occupied, cam, pose, log_scale_factor, viewing_cos_limit,
                                          MapPoints{n_mp, pos, normal, min_dist, max_dist, mp_desc, nullptr, nullptr}, eligible, has_obs, th, nnratio,
                                          far_points, th_far_points, in_view, frame_match);
}
extern "C" int orbx_frame_search_local_points_map(orbx_matcher *m, orbx_frame *f, const uint8_t *frame_occupied, const orbx_camera *cam,
                                                  const orbx_frame_pose *pose, float log_scale_factor, float viewing_cos_limit, int n_mp, orbx_map *map,
                                                  const int32_t *ids, const uint8_t *eligible, const uint8_t *has_obs, float th, float nnratio,
                                                  int far_points, float th_far_points, uint8_t *in_view, int32_t *frame_match) {
    if (!map_form_ok(map, n_mp)) return ORBX_E_BAD_ARG;
    return frame_search_local_points_impl(m, f, frame_occupied, cam, pose, log_scale_factor, viewing_cos_limit, map_points_of(n_mp, map, ids), eligible,
                                          has_obs, th, nnratio, far_points, th_far_points, in_view, frame_match);
}

// Tracking::SearchLocalPoints on a resident fisheye-stereo frame: isInFrustumChecks of both cameras (k_in_frustum_checks), the windows
// (k_local_windows_fisheye), the twin window search and the replay (k_replay_twin) -- the projection records never leave the device.
static int frame_search_local_points_fisheye_impl(orbx_matcher *m, orbx_frame *f, const uint8_t *frame_occupied, const orbx_fisheye_view *views,
                                                  float log_scale_factor, float viewing_cos_limit, const MapPoints &src, const uint8_t *eligible,
                                                  const uint8_t *has_obs, const float *track_depth, float th, float nnratio, int far_points,
                                                  float th_far_points, uint8_t *in_view, int32_t *frame_match) {
    const LocalPoints mp = {src, eligible, has_obs, track_depth};
    const int n_mp = src.n;
    int N = -1;
    const int rc = local_points_head(m, f, true, views != nullptr, mp, frame_occupied, in_view, frame_match, &N);
    if (rc != ORBX_OK || n_mp == 0) return rc;
    const int nc = f->rows_n();
    ORBX_HIP(hipSetDevice(m->device));
    const size_t q = (size_t)n_mp, q2 = 2 * q;
    FrustumChecks FC;
    memset(&FC, 0, sizeof(FC));
    memcpy(FC.view, views, sizeof(FisheyeView) * 2);
    FC.minx = f->bounds[0]; FC.maxx = f->bounds[1]; FC.miny = f->bounds[2]; FC.maxy = f->bounds[3];
    FC.log_scale_factor = log_scale_factor; FC.nlevels = f->nlevels; FC.cos_limit = viewing_cos_limit;
    const int32_t cnts[4] = {n_mp, 0, 0, 0};
    WindowProblem P[2];
    memset(P, 0, sizeof(P));
    TwinProblem T;
    memset(&T, 0, sizeof(T));
    LocalPointsDev D;
    float *dx, *dy, *dd, *dvc, *dqr;
    uint8_t *div, *dvalid, *div_out;
    int32_t *dcnt, *dl, *dqmin, *dqmax;
    FrustumChecks *dF;
    WindowProblem *dP;
    ORBX_TRY(m->carve([&](Carve &A) {
        // inputs (one run of the arena)
        D = local_points_up(A, mp, frame_occupied, N);
        dF = A.up(&FC, 1);
        dcnt = A.up(cnts, 4);
        dP = A.take<WindowProblem>(2);
        // the projection records and the windows: device only, [2][n_mp] (left, right)
        div = A.take<uint8_t>(q2);
        dx = A.take<float>(q2); dy = A.take<float>(q2); dd = A.take<float>(q2); dvc = A.take<float>(q2);
        dl = A.take<int32_t>(q2);
        dqr = A.take<float>(q2);
        dqmin = A.take<int32_t>(q2); dqmax = A.take<int32_t>(q2);
        dvalid = A.take<uint8_t>(q2);
        for (int s = 0; s < 2; s++) { P[s].keys = A.take<u64>(q * kTopK); P[s].meta = A.take<int32_t>(q); }
        T.entries = A.take<int32_t>(q2);
        // the downloads side by side: mbTrackInView / mbTrackInViewR, the matches, nmatches
        div_out = A.take<uint8_t>(q2);
        T.match = A.take<int32_t>(nc);
        T.nmatches = A.take<int32_t>(1);
    }));
    for (int s = 0; s < 2; s++) {
        const size_t o = (size_t)s * q;
        frame_side(f, s == 1, P[s]);
        P[s].nq_ptr = dcnt;
        P[s].qx = dx + o; P[s].qy = dy + o; P[s].qr = dqr + o; P[s].qmin = dqmin + o; P[s].qmax = dqmax + o; P[s].qvalid = dvalid + o; P[s].qdesc = D.desc;
    }
    T.q_has_obs = D.has_obs; T.occupied0 = D.occupied;
    T.mode = 1; T.nq = n_mp; T.nnratio = nnratio; T.max_dist = (float)ORBX_TH_HIGH; T.cleared_value = -2;
    T.l2r = f->l2r; T.r2l = f->r2l;
    ORBX_TRY(m->h2d(dP, P, sizeof(P)));
    uint64_t seq = 0;
    ORBX_TRY(map_points_gather(m, src, D, &seq));
    hipLaunchKernelGGL(k_in_frustum_checks, dim3((n_mp + 255) / 256, 2), dim3(256), 0, m->exec(), (const FrustumChecks *)dF, n_mp, (const float *)D.pos,
                       (const float *)D.normal, (const float *)D.min_dist, (const float *)D.max_dist, div, dx, dy, dd, dl, dvc);
    hipLaunchKernelGGL(k_local_windows_fisheye, dim3((n_mp + 255) / 256), dim3(256), 0, m->exec(), n_mp, (const uint8_t *)div, (const uint8_t *)D.eligible,
                       (const int32_t *)dl, (const float *)dvc, (const float *)dd, (const float *)D.track_depth, (const float *)f->scale, f->nlevels, th,
                       far_points ? 1 : 0, th_far_points, dqr, dqmin, dqmax, dvalid, div_out);
    const bool match = N != 0;   // (an empty frame: isInFrustumChecks only)
    if (match) ORBX_TRY(launch_twin(m, dP, T, grid_of(f->bounds), nc, n_mp));
    const int nm = local_points_tail(m, f, match, in_view, div_out, q2, T.match, nc, T.nmatches, frame_match);
    if (nm >= 0) map_points_done(src, seq);
    return nm;
}

extern "C" int orbx_frame_search_local_points_fisheye(orbx_matcher *m, orbx_frame *f, const uint8_t *frame_occupied, const orbx_fisheye_view *views,
                                                      float log_scale_factor, float viewing_cos_limit, int n_mp, const float *pos, const float *normal,
                                                      const float *min_dist, const float *max_dist, const uint8_t *mp_desc, const uint8_t *eligible,
                                                      const uint8_t *has_obs, const float *track_depth, float th, float nnratio, int far_points,
                                                      float th_far_points, uint8_t *in_view, int32_t *frame_match) {
    return frame_search_local_points_fisheye_impl(m, f, frame_occupied, views, log_scale_factor, viewing_cos_limit,
                                                  MapPoints{n_mp, pos, normal, min_dist, max_dist, mp_desc, nullptr, nullptr}, eligible, has_obs, track_depth,
                                                  th, nnratio, far_points, th_far_points, in_view, frame_match);
}
extern "C" int orbx_frame_search_local_points_fisheye_map(orbx_matcher *m, orbx_frame *f, const uint8_t *frame_occupied, const orbx_fisheye_view *views,
                                                          float log_scale_factor, float viewing_cos_limit, int n_mp, orbx_map *map, const int32_t *ids,
                                                          const uint8_t *eligible, const uint8_t *has_obs, const float *track_depth, float th,
                                                          float nnratio, int far_points, float th_far_points, uint8_t *in_view, int32_t *frame_match) {
    if (!map_form_ok(map, n_mp)) return ORBX_E_BAD_ARG;
    return frame_search_local_points_fisheye_impl(m, f, frame_occupied, views, log_scale_factor, viewing_cos_limit, map_points_of(n_mp, map, ids), eligible,
                                                  has_obs, track_depth, th, nnratio, far_points, th_far_points, in_view, frame_match);
}

// ---------------------------------------------------------------------------------------------------------
// Matchers whose inner loop carries more state than a taken-mask: SearchForInitialization (vMatchedDistance) and the BoW
// merge-joins run entirely on the device (k_replay_init / k_replay_bow, one wave replays the reference's query order).
// SearchForTriangulation with a geometric gate keeps one host piece: the camera model's epipolarConstrain lives in the
// adapter (camera models are out of scope), so the device evaluates every candidate distance of the reference's enumeration
// and the loop calls the gate back exactly where the reference evaluates it.
// ---------------------------------------------------------------------------------------------------------
namespace {

inline int rotation_bin(float a1, float a2) {  // e.g. ORBmatcher.cc:337-343
    float rot = a1 - a2;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)std::round(rot * (1.0f / ORBX_HISTO_LENGTH));
    if (bin == ORBX_HISTO_LENGTH) bin = 0;
    return bin;
}

// ComputeThreeMaxima (ORBmatcher.cc:2012-2053) + removal of the losing bins; entries = (bin, key) in push order
struct RotHist {
    std::vector<std::pair<int, int>> entries;
    void push(int bin, int key) { entries.emplace_back(bin, key); }
    template <class Drop> void filter(Drop drop) const {
        int cnt[ORBX_HISTO_LENGTH] = {0};
        for (auto &e : entries) cnt[e.first]++;
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        for (int i = 0; i < ORBX_HISTO_LENGTH; i++) {
            const int s = cnt[i];
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
            else if (s > max3) { max3 = s; ind3 = i; }
        }
        if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
        for (auto &e : entries)
            if (e.first != ind1 && e.first != ind2 && e.first != ind3) drop(e.second);
    }
};

// merge-join of two flattened DBoW2::FeatureVector maps: equal node ids in ascending order
template <class V> void for_common_nodes(const orbx_featvec *a, const orbx_featvec *b, V visit) {
    int ia = 0, ib = 0;
    while (ia < a->n_nodes && ib < b->n_nodes) {
        const uint32_t na = a->node_id[ia], nb = b->node_id[ib];
        if (na == nb) { visit(ia, ib); ia++; ib++; }
        else if (na < nb) ia++;
        else ib++;
    }
}

// queries = features of A listed in the common nodes (those with qmask clear), candidates = the node's list in B.
// Builds the CSR in the reference's enumeration order and evaluates all distances on the GPU.
struct BowPairs {
    std::vector<int32_t> q_idx, row_ptr, cand;
    std::vector<uint16_t> dist;
};
int bow_distances(orbx_matcher *m, const uint8_t *descA, const uint8_t *skipA, const orbx_featvec *fvA, const uint8_t *descB, int nB,
                  const orbx_featvec *fvB, BowPairs &P) {
    P.row_ptr.assign(1, 0);
    for_common_nodes(fvA, fvB, [&](int ia, int ib) {
        for (int a = fvA->node_ptr[ia]; a < fvA->node_ptr[ia + 1]; a++) {
            const int i = fvA->index[a];
            if (skipA && skipA[i]) continue;
            P.q_idx.push_back(i);
            for (int b = fvB->node_ptr[ib]; b < fvB->node_ptr[ib + 1]; b++) P.cand.push_back(fvB->index[b]);
            P.row_ptr.push_back((int32_t)P.cand.size());
        }
    });
    const int nq = (int)P.q_idx.size();
    P.dist.assign(P.cand.size(), 0);
    if (nq == 0 || P.cand.empty()) return ORBX_OK;
    std::vector<uint8_t> qd((size_t)nq * 32);
    for (int k = 0; k < nq; k++) memcpy(&qd[(size_t)k * 32], descA + (size_t)P.q_idx[k] * 32, 32);
    return orbx_hamming_csr(m, qd.data(), nq, descB, nB, P.row_ptr.data(), P.cand.data(), P.dist.data());
}

}  // namespace

extern "C" {

// ORBmatcher::SearchForInitialization (ORBmatcher.cc:648-763).  Round 6: F2's grid, the candidate lists of every level-0 keypoint of F1 (k_window_best2_t<64>:
// a wave per query, the lists do not depend on the loop's state) and a one-wave replay of the loop over those lists (k_replay_init_lists);
// frames beyond kMaxResolveFeatures keep the single-wave scan k_replay_init (the replay's state no longer fits the LDS).
int orbx_search_for_initialization(orbx_matcher *m, const orbx_keypoint *kps1_un, const uint8_t *desc1, int n1, const orbx_frame_desc *F2,
                                   float *prev_matched, int window_size, float nnratio, int check_orientation, int32_t *matches12) {
    if (!m || !F2 || n1 < 0 || (n1 > 0 && (!matches12 || !kps1_un || !desc1 || !prev_matched))) return ORBX_E_BAD_ARG;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    const int n2 = F2->n;
    if (n1 == 0 || n2 == 0) return 0;
    if (n1 > 65535 || n2 > 65535) return ORBX_E_TOO_LARGE;
    ORBX_HIP(hipSetDevice(m->device));
    const float fb[4] = {F2->min_x, F2->max_x, F2->min_y, F2->max_y};
    const GridParams g = grid_of(fb);
    if (n1 > kMaxResolveFeatures || n2 > kMaxResolveFeatures) {
        InitProblem P;
        memset(&P, 0, sizeof(P));
        P.n1 = n1; P.n2 = n2; P.window = (float)window_size; P.nnratio = nnratio; P.check_orientation = check_orientation ? 1 : 0;
        float *dprev;
        ORBX_TRY(m->carve([&](Carve &A) {
            P.kps1 = A.up(kps1_un, (size_t)n1); P.kps2 = A.up(F2->keypoints_un, (size_t)n2);
            P.desc1 = A.up(desc1, 32 * (size_t)n1); P.desc2 = A.up(F2->descriptors, 32 * (size_t)n2);
            P.prev_matched = dprev = A.up(prev_matched, 2 * (size_t)n1);
            P.matches12 = A.take<int32_t>(n1); P.entries = A.take<int32_t>(n1);
            P.matches21 = A.take<int32_t>(n2); P.matched_dist = A.take<int32_t>(n2);
            P.nmatches = A.take<int32_t>(4);
        }));
        hipLaunchKernelGGL(k_replay_init, dim3(1), dim3(64), 0, m->exec(), P, g);
        int32_t nm = 0;
        ORBX_TRY(m->d2h(matches12, P.matches12, 4 * (size_t)n1));
        ORBX_TRY(m->d2h(prev_matched, dprev, 8 * (size_t)n1));
        ORBX_TRY(m->d2h(&nm, P.nmatches, 4));
        ORBX_TRY(m->sync_and_deliver());
        return nm;
    }
    // the queries: keypoints of F1 on level 0, in index order (:661-666); window = vbPrevMatched[i1] +- windowSize on level [level1, level1] (:668)
    std::vector<int32_t> qidx;
    qidx.reserve(n1);
    for (int i = 0; i < n1; i++)
        if (kps1_un[i].octave <= 0) qidx.push_back(i);
    const int nq = (int)qidx.size();
    if (nq == 0) return 0;
    std::vector<float> qx(nq), qy(nq), qr(nq, (float)window_size);
    std::vector<int32_t> qlv(nq);
    std::vector<uint8_t> qd(32 * (size_t)nq);
    for (int k = 0; k < nq; k++) {
        const int i = qidx[k];
        qx[k] = prev_matched[2 * i]; qy[k] = prev_matched[2 * i + 1]; qlv[k] = kps1_un[i].octave;
        memcpy(&qd[32 * (size_t)k], desc1 + 32 * (size_t)i, 32);
    }
    const size_t lds = 4 * (size_t)n2 + 2 * (size_t)n2 * 2 + 2 * (size_t)n1 + 64;
    // every candidate key of every query for the replay's re-evaluations (WindowProblem::all_keys): up to 512 per query within 8 MB
    const int all_cap = (int)std::min<size_t>(512, std::max<size_t>(64, ((size_t)8 << 20) / (8 * (size_t)nq)));
    WindowProblem P;
    memset(&P, 0, sizeof(P));
    InitReplay R;
    memset(&R, 0, sizeof(R));
    P.all_cap = all_cap;
    R.n1 = n1; R.n2 = n2; R.nq = nq; R.nnratio = nnratio; R.check_orientation = check_orientation ? 1 : 0;
    const int32_t cnts[2] = {n2, nq};
    int32_t *dcnt;
    WindowProblem *dP;
    // every upload in one run of the arena, the problem record directly behind the inputs; device-only buffers behind it; the three downloads side by side
    ORBX_TRY(m->carve([&](Carve &A) {
        R.kps1 = A.up(kps1_un, (size_t)n1); P.kps = A.up(F2->keypoints_un, (size_t)n2);
        P.desc = A.up(F2->descriptors, 32 * (size_t)n2);
        dcnt = A.up(cnts, 2, 2);
        P.qx = A.up(qx.data(), (size_t)nq); P.qy = A.up(qy.data(), (size_t)nq); P.qr = A.up(qr.data(), (size_t)nq);
        P.qmin = P.qmax = A.up(qlv.data(), (size_t)nq); R.q_index = A.up(qidx.data(), (size_t)nq);
        P.qdesc = A.up(qd.data(), 32 * (size_t)nq);
        dP = A.take<WindowProblem>(1);
        P.keys = A.take<u64>((size_t)nq * kTopK); P.meta = A.take<int32_t>(nq);
        P.gstart = A.take<uint16_t>(kGridCells + 1); P.gorder = A.take<uint16_t>(n2);
        P.all_cnt = A.take<int32_t>(nq); P.all_keys = A.take<u64>((size_t)nq * all_cap);
        R.entries = A.take<int32_t>(nq);
        R.matches12 = A.take<int32_t>(n1);
        R.prev_matched = A.up(prev_matched, 2 * (size_t)n1);
        R.nmatches = A.take<int32_t>(4);
    }));
    P.n_ptr = dcnt; P.nq_ptr = dcnt + 1;
    ORBX_TRY(m->h2d(dP, &P, sizeof(P)));
    ORBX_LAUNCH_GRID_BUILD(dim3(1), dim3(64), 0, m->exec(), dP, g);
    hipLaunchKernelGGL(k_window_best2_t<64>, dim3(1, (unsigned)((nq + 3) / 4), 1), dim3(256), 0, m->exec(), dP, g, 1);   // a wave per query (100-px windows: hundreds of candidates)
    if (lds > 64 * 1024) ORBX_HIP(hipFuncSetAttribute((const void *)k_replay_init_lists, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_replay_init_lists, dim3(1), dim3(64), lds, m->exec(), dP, R, g);
    ORBX_HIP(hipGetLastError());
    int32_t nm[4] = {0, 0, 0, 0};
    ORBX_TRY(m->d2h(matches12, R.matches12, 4 * (size_t)n1));
    ORBX_TRY(m->d2h(prev_matched, R.prev_matched, 8 * (size_t)n1));
    ORBX_TRY(m->d2h(nm, R.nmatches, 16));
    ORBX_TRY(m->sync_and_deliver());
    for (int k = 0; k < 3; k++) m->replay_stats[k] = nm[k + 1];
    return nm[0];
}

}  // extern "C"

namespace {
// k_replay_bow on host pointers: mode 0 SearchByBoW(KF, Frame), 1 SearchByBoW(KF, KF), 2 SearchForTriangulation without a gate
int run_bow_replay(orbx_matcher *m, int mode, const uint8_t *desc_a, const float *angle_a, const uint8_t *skip_a, int na, const orbx_featvec *fa,
                   const uint8_t *desc_b, const float *angle_b, const uint8_t *skip_b, int nb, const orbx_featvec *fb, float nnratio,
                   int check_orientation, int32_t *match_out, int n_out, const orbx_pinhole_gate *gate = nullptr, int nb_left = 0,
                   const orbx_kb8_gate *kgate = nullptr) {
    if (na > 65535 || nb > 65535) return ORBX_E_TOO_LARGE;
    ORBX_HIP(hipSetDevice(m->device));
    const size_t ia = (size_t)fa->node_ptr[fa->n_nodes], ib = (size_t)fb->node_ptr[fb->n_nodes];
    if (!desc_a || !desc_b || (check_orientation && (!angle_a || !angle_b))) return ORBX_E_BAD_ARG;
    if (gate && (!gate->kps1_un || !gate->kps2_un || !gate->scale_factors2 || !gate->level_sigma2_2)) return ORBX_E_BAD_ARG;
    const bool kb8_kernel = kgate && !kgate->coarse;   // bCoarse: no gate at all for such key frames (no epipole test either, :1026) = k_replay_bow without a gate
    if (kb8_kernel && (!kgate->kps1 || !kgate->kps2 || !kgate->level_sigma2_1 || !kgate->level_sigma2_2)) return ORBX_E_BAD_ARG;
    BowProblem P;
    memset(&P, 0, sizeof(P));
    P.mode = mode; P.nb_left = nb_left;
    { const char *dbg = getenv("ORBX_BOW_DEBUG"); P.debug_stop = dbg ? atoi(dbg) : 0; }
    P.na = na; P.nb = nb; P.nnratio = nnratio; P.check_orientation = check_orientation ? 1 : 0;
    P.fa.n_nodes = fa->n_nodes; P.fb.n_nodes = fb->n_nodes;
    // the merge-join of the two sorted node-id lists (:246-250, :800-805, :961-965) on the host: node ia of A pairs with node pair_b[ia] of B
    std::vector<int32_t> pair((size_t)fa->n_nodes + 1, -1);
    for_common_nodes(fa, fb, [&](int a_, int b_) { pair[a_] = b_; });
    Kb8Gate K;
    memset(&K, 0, sizeof(K));
    TriGate &G = P.gate;
    if (gate) {  // the pinhole gates of SearchForTriangulation run inside the kernel (mode 2)
        G.enabled = 1; G.coarse = gate->coarse ? 1 : 0; G.strict = gate->strict_fp ? 1 : 0;
        for (int i = 0; i < 9; i++) G.F[i] = gate->F12[i];
        G.ex = gate->ep_x; G.ey = gate->ep_y;
    }
    if (kb8_kernel) {  // fisheye key frames: KannalaBrandt8::epipolarConstrain on the device (k_tri_kb8)
        G.enabled = 1; G.coarse = 0; G.strict = 1;
        K.n_left1 = kgate->n_left1; K.n_left2 = kgate->n_left2;
        memcpy(K.cam[0], kgate->cam1, sizeof(float) * 16);
        memcpy(K.cam[2], kgate->cam2, sizeof(float) * 16);
        memcpy(K.R12, kgate->R12, sizeof(K.R12));
        memcpy(K.t12, kgate->t12, sizeof(K.t12));
    }
    ORBX_TRY(m->carve([&](Carve &A) {
        P.fa.node_id = A.up(fa->node_id, (size_t)fa->n_nodes, 1); P.fa.node_ptr = A.up(fa->node_ptr, (size_t)fa->n_nodes + 1); P.fa.index = A.up(fa->index, ia, 1);
        P.fb.node_id = A.up(fb->node_id, (size_t)fb->n_nodes, 1); P.fb.node_ptr = A.up(fb->node_ptr, (size_t)fb->n_nodes + 1); P.fb.index = A.up(fb->index, ib, 1);
        P.pair_b = A.up(pair.data(), pair.size());
        P.desc_a = A.up(desc_a, 32 * (size_t)na); P.desc_b = A.up(desc_b, 32 * (size_t)nb);
        P.angle_a = A.up_opt(angle_a, (size_t)na); P.angle_b = A.up_opt(angle_b, (size_t)nb);
        P.skip_a = A.up_opt(skip_a, (size_t)na); P.skip_b = A.up_opt(skip_b, (size_t)nb);
        if (gate) {
            G.k1 = A.up(gate->kps1_un, (size_t)na); G.k2 = A.up(gate->kps2_un, (size_t)nb);
            G.ur1 = A.up_opt(gate->u_right1, (size_t)na); G.ur2 = A.up_opt(gate->u_right2, (size_t)nb);
            G.scale2 = A.up(gate->scale_factors2, (size_t)gate->nlevels); G.sigma2_2 = A.up(gate->level_sigma2_2, (size_t)gate->nlevels);
        }
        if (kb8_kernel) {
            G.k1 = A.up(kgate->kps1, (size_t)na); G.k2 = A.up(kgate->kps2, (size_t)nb);
            G.sigma2_2 = A.up(kgate->level_sigma2_2, (size_t)kgate->nlevels);
            K.sigma2_1 = A.up(kgate->level_sigma2_1, (size_t)kgate->nlevels);
            G.kb8 = A.up(&K, 1);   // (behind the level table it points to)
        }
        // the two downloads side by side (one DMA), the two zero-filled buffers side by side (one fill)
        P.match = A.take<int32_t>(n_out); P.nmatches = A.take<int32_t>(4);
        P.taken_b = A.take<uint8_t>(nb);
        P.hist = A.take<int32_t>(ORBX_HISTO_LENGTH + 2);
        P.entries = A.take<int32_t>(2 * (size_t)std::max(na, nb));
    }));
    P.counters = P.hist + ORBX_HISTO_LENGTH;
    ORBX_HIP(m->fill(P.match, 0xff, 4 * (size_t)n_out));     // -1: no match.  Both fills ride in the launch that brings the inputs (orbx_matcher::fill)
    ORBX_HIP(m->fill(P.taken_b, 0, (size_t)((const uint8_t *)(P.hist + ORBX_HISTO_LENGTH + 2) - P.taken_b)));   // taken_b, (padding,) hist + counters
    if (fa->n_nodes > 0) {   // a wave per vocabulary node
        if (kb8_kernel) hipLaunchKernelGGL(k_tri_kb8, dim3((fa->n_nodes + 3) / 4), dim3(256), 0, m->exec(), P);
        else hipLaunchKernelGGL(k_replay_bow, dim3((fa->n_nodes + 3) / 4), dim3(256), 0, m->exec(), P);
    }
    hipLaunchKernelGGL(k_replay_bow_finish, dim3(1), dim3(64), 0, m->exec(), P);
    int32_t nm = 0;
    ORBX_TRY(m->d2h(match_out, P.match, 4 * (size_t)n_out));
    ORBX_TRY(m->d2h(&nm, P.nmatches, 4));
    ORBX_TRY(m->sync_and_deliver());
    return nm;
}
}  // namespace

extern "C" {

// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (ORBmatcher.cc:223-425), monocular form: k_replay_bow mode 0
int orbx_search_by_bow_frame(orbx_matcher *m, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_valid, int n_kf,
                             const orbx_featvec *kf_fv, const uint8_t *f_desc, const float *f_angle, int n_f, const orbx_featvec *f_fv,
                             float nnratio, int check_orientation, int32_t *f_match) {
    if (!m || !kf_fv || !f_fv || (!f_match && n_f > 0) || n_kf < 0 || n_f < 0) return ORBX_E_BAD_ARG;
    for (int i = 0; i < n_f; i++) f_match[i] = -1;
    if (n_kf == 0 || n_f == 0) return 0;
    std::vector<uint8_t> skip(n_kf);
    for (int i = 0; i < n_kf; i++) skip[i] = kf_valid ? !kf_valid[i] : 0;
    return run_bow_replay(m, 0, kf_desc, kf_angle, skip.data(), n_kf, kf_fv, f_desc, f_angle, nullptr, n_f, f_fv, nnratio, check_orientation,
                          f_match, n_f);
}

// the same for a fisheye-stereo frame (F.Nleft != -1, ORBmatcher.cc:283-392): features >= n_f_left belong to the right camera
int orbx_search_by_bow_frame_fisheye(orbx_matcher *m, const uint8_t *kf_desc, const float *kf_angle, const uint8_t *kf_valid, int n_kf,
                                     const orbx_featvec *kf_fv, const uint8_t *f_desc, const float *f_angle, int n_f, int n_f_left,
                                     const orbx_featvec *f_fv, float nnratio, int check_orientation, int32_t *f_match) {
    if (!m || !kf_fv || !f_fv || (!f_match && n_f > 0) || n_kf < 0 || n_f < 0 || n_f_left < 0 || n_f_left > n_f) return ORBX_E_BAD_ARG;
    for (int i = 0; i < n_f; i++) f_match[i] = -1;
    if (n_kf == 0 || n_f == 0) return 0;
    std::vector<uint8_t> skip(n_kf);
    for (int i = 0; i < n_kf; i++) skip[i] = kf_valid ? !kf_valid[i] : 0;
    return run_bow_replay(m, 3, kf_desc, kf_angle, skip.data(), n_kf, kf_fv, f_desc, f_angle, nullptr, n_f, f_fv, nnratio, check_orientation,
                          f_match, n_f, nullptr, n_f_left);
}

// ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (ORBmatcher.cc:765-905): k_replay_bow mode 1
int orbx_search_by_bow_keyframes(orbx_matcher *m, const uint8_t *desc1, const float *angle1, const uint8_t *valid1, int n1,
                                 const orbx_featvec *fv1, const uint8_t *desc2, const float *angle2, const uint8_t *valid2, int n2,
                                 const orbx_featvec *fv2, float nnratio, int check_orientation, int32_t *match12) {
    if (!m || !fv1 || !fv2 || (!match12 && n1 > 0) || n1 < 0 || n2 < 0) return ORBX_E_BAD_ARG;
    for (int i = 0; i < n1; i++) match12[i] = -1;
    if (n1 == 0 || n2 == 0) return 0;
    std::vector<uint8_t> skip1(n1), skip2(n2);
    for (int i = 0; i < n1; i++) skip1[i] = valid1 ? !valid1[i] : 0;
    for (int i = 0; i < n2; i++) skip2[i] = valid2 ? !valid2[i] : 0;
    return run_bow_replay(m, 1, desc1, angle1, skip1.data(), n1, fv1, desc2, angle2, skip2.data(), n2, fv2, nnratio, check_orientation, match12, n1);
}

// ORBmatcher::SearchForTriangulation (ORBmatcher.cc:907-1146)
int orbx_search_for_triangulation(orbx_matcher *m, const uint8_t *desc1, const float *angle1, const uint8_t *skip1, int n1,
                                  const orbx_featvec *fv1, const uint8_t *desc2, const float *angle2, const uint8_t *skip2, int n2,
                                  const orbx_featvec *fv2, int check_orientation, orbx_pair_predicate pair_ok, void *user,
                                  int32_t *matches12) {
    if (!m || !fv1 || !fv2 || (!matches12 && n1 > 0) || n1 < 0 || n2 < 0) return ORBX_E_BAD_ARG;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (n1 == 0 || n2 == 0) return 0;
    // without a geometric gate (bCoarse) nothing but distances decides: the whole loop runs on the device (k_replay_bow mode 2).
    // With a gate, the camera model's epipolarConstrain is host code of the adapter: the device evaluates every candidate
    // distance and the loop below calls the gate exactly where the reference evaluates it.
    if (!pair_ok)
        return run_bow_replay(m, 2, desc1, angle1, skip1, n1, fv1, desc2, angle2, skip2, n2, fv2, 0.f, check_orientation, matches12, n1);
    BowPairs P;
    const int r = bow_distances(m, desc1, skip1, fv1, desc2, n2, fv2, P);
    if (r != ORBX_OK) return r;
    int nmatches = 0;
    RotHist hist;
    for (size_t k = 0; k < P.q_idx.size(); k++) {
        const int i1 = P.q_idx[k];
        int best = ORBX_TH_LOW, best2 = -1;
        for (int c = P.row_ptr[k]; c < P.row_ptr[k + 1]; c++) {
            const int i2 = P.cand[c], d = P.dist[c];
            if (skip2 && skip2[i2]) continue;            // pMP2 (vbMatched2 is never set in v1.0)
            if (d > ORBX_TH_LOW || d > best) continue;     // :1017 -- '>' : a later equal candidate wins
            if (!pair_ok || pair_ok(user, i1, i2)) { best2 = i2; best = d; }  // epipole gate + epipolarConstrain / bCoarse
        }
        if (best2 >= 0) {
            matches12[i1] = best2;
            nmatches++;
            if (check_orientation) hist.push(rotation_bin(angle1[i1], angle2[best2]), i1);
        }
    }
    if (check_orientation) hist.filter([&](int i1) { matches12[i1] = -1; nmatches--; });
    return nmatches;
}

// SearchForTriangulation for pinhole key frames with both geometric gates on the device (k_replay_bow mode 2 + tri_gate): the
// epipole-distance test (ORBmatcher.cc:1026-1034) and Pinhole::epipolarConstrain (CameraModels/Pinhole.cpp:107-129) on the caller's
// F12.  No callback, no host loop.
int orbx_search_for_triangulation_pinhole(orbx_matcher *m, const uint8_t *desc1, const uint8_t *skip1, int n1, const orbx_featvec *fv1,
                                          const uint8_t *desc2, const uint8_t *skip2, int n2, const orbx_featvec *fv2,
                                          int check_orientation, const orbx_pinhole_gate *gate, int32_t *matches12) {
    if (!m || !fv1 || !fv2 || (!matches12 && n1 > 0) || !gate || n1 < 0 || n2 < 0) return ORBX_E_BAD_ARG;
    if (!gate->kps1_un || !gate->kps2_un || !gate->scale_factors2 || !gate->level_sigma2_2 || gate->nlevels <= 0 || gate->nlevels > 64)
        return ORBX_E_BAD_ARG;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (n1 == 0 || n2 == 0) return 0;
    std::vector<float> a1(n1), a2(n2);  // kp.angle of mvKeysUn (:1086-1094)
    for (int i = 0; i < n1; i++) a1[i] = gate->kps1_un[i].angle;
    for (int i = 0; i < n2; i++) a2[i] = gate->kps2_un[i].angle;
    return run_bow_replay(m, 2, desc1, a1.data(), skip1, n1, fv1, desc2, a2.data(), skip2, n2, fv2, 0.f, check_orientation, matches12, n1, gate);
}

// SearchForTriangulation between two key frames of a FISHEYE rig (pKF->mpCamera2 != NULL): the gate of :1036-1072 -- KannalaBrandt8::epipolarConstrain with the
// camera pair and relative pose the two feature indices select -- evaluated by k_tri_kb8 over the node's list of pairs within TH_LOW (until round 6 a host
// callback around a download of every candidate distance); bCoarse: no gate at all, k_replay_bow mode 2
int orbx_search_for_triangulation_kb8(orbx_matcher *m, const uint8_t *desc1, const uint8_t *skip1, int n1, const orbx_featvec *fv1, const uint8_t *desc2,
                                      const uint8_t *skip2, int n2, const orbx_featvec *fv2, int check_orientation, const orbx_kb8_gate *gate,
                                      int32_t *matches12) {
    if (!m || !fv1 || !fv2 || (!matches12 && n1 > 0) || !gate || n1 < 0 || n2 < 0) return ORBX_E_BAD_ARG;
    if (!gate->kps1 || !gate->kps2 || !gate->level_sigma2_1 || !gate->level_sigma2_2 || gate->nlevels <= 0 || gate->nlevels > 64) return ORBX_E_BAD_ARG;
    if (gate->n_left1 < 0 || gate->n_left1 > n1 || gate->n_left2 < 0 || gate->n_left2 > n2) return ORBX_E_BAD_ARG;
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (n1 == 0 || n2 == 0) return 0;
    for (int i = 0; i < n1; i++) if (gate->kps1[i].octave < 0 || gate->kps1[i].octave >= gate->nlevels) return ORBX_E_BAD_ARG;
    for (int i = 0; i < n2; i++) if (gate->kps2[i].octave < 0 || gate->kps2[i].octave >= gate->nlevels) return ORBX_E_BAD_ARG;
    std::vector<float> a1(n1), a2(n2);  // kp.angle (:1086-1094)
    for (int i = 0; i < n1; i++) a1[i] = gate->kps1[i].angle;
    for (int i = 0; i < n2; i++) a2[i] = gate->kps2[i].angle;
    return run_bow_replay(m, 2, desc1, a1.data(), skip1, n1, fv1, desc2, a2.data(), skip2, n2, fv2, 0.f, check_orientation, matches12, n1, nullptr, 0, gate);
}

// Frame::ComputeStereoFishEyeMatches (Frame.cc:1126-1166) whole, on host arrays: k_knn2 over the lapping-area tails, k_tri_kb8_stereo (ratio test,
// KannalaBrandt8::TriangulateMatches, the four output vectors); one launch chain and one synchronisation in the matcher's queue
int orbx_compute_stereo_fisheye_matches(orbx_matcher *m, const orbx_kb8_rig *rig, const orbx_keypoint *kps_left, const uint8_t *desc_left, int n_left,
                                        int mono_left, const orbx_keypoint *kps_right, const uint8_t *desc_right, int n_right, int mono_right,
                                        const float *level_sigma2, int nlevels, int32_t *l2r, int32_t *r2l, float *depth, float *p3d, int *desc_matches) {
    if (!m || !rig || n_left < 0 || n_right < 0 || mono_left < 0 || mono_left > n_left || mono_right < 0 || mono_right > n_right) return ORBX_E_BAD_ARG;
    if (!level_sigma2 || nlevels <= 0 || nlevels > 64) return ORBX_E_BAD_ARG;
    if (n_left > 0 && (!kps_left || !desc_left || !l2r || !depth || !p3d)) return ORBX_E_BAD_ARG;
    if (n_right > 0 && (!kps_right || !desc_right || !r2l)) return ORBX_E_BAD_ARG;
    for (int i = 0; i < n_left; i++) if (kps_left[i].octave < 0 || kps_left[i].octave >= nlevels) return ORBX_E_BAD_ARG;
    for (int i = 0; i < n_right; i++) if (kps_right[i].octave < 0 || kps_right[i].octave >= nlevels) return ORBX_E_BAD_ARG;
    if (n_left == 0) {   // nothing to match; r2l = -1 (:1134-1138)
        for (int i = 0; i < n_right; i++) r2l[i] = -1;
        if (desc_matches) *desc_matches = 0;
        return 0;
    }
    ORBX_HIP(hipSetDevice(m->device));
    const size_t NL = (size_t)n_left, NR = (size_t)n_right, nq = NL - (size_t)mono_left, nt = NR - (size_t)mono_right;
    const int32_t hn[4] = {n_left, mono_left, n_right, mono_right};
    orbx_kb8_rig *drig;
    int32_t *dn, *di, *dd, *dl2r, *dr2l, *dcnt;
    float *ds, *ddep, *dp;
    orbx_keypoint *dkl, *dkr;
    uint8_t *ddl, *ddr;
    ORBX_TRY(m->carve([&](Carve &A) {
        drig = A.up(rig, 1);
        dn = A.up(hn, 4, 12);
        ds = A.up(level_sigma2, (size_t)nlevels);
        dkl = A.up(kps_left, NL); dkr = A.up(kps_right, NR, 1);
        ddl = A.up(desc_left + 32 * (size_t)mono_left, 32 * nq, 32);     // the lapping-area tails (:1128-1132)
        ddr = A.up(desc_right + 32 * (size_t)mono_right, 32 * nt, 32);
        di = A.take<int32_t>(2 * nq + 2); dd = A.take<int32_t>(2 * nq + 2);
        dl2r = A.take<int32_t>(NL);
        ddep = A.take<float>(NL); dp = A.take<float>(3 * NL);
        dr2l = A.take<int32_t>(NR + 1); dcnt = A.take<int32_t>(4);
    }));
    ORBX_HIP(m->fill(dr2l, 0xff, 4 * NR));
    ORBX_HIP(m->fill(dcnt, 0, 16));
    if (nq > 0)
        hipLaunchKernelGGL(k_knn2, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, m->exec(), (const uint8_t *)ddl, (int)nq, (const uint8_t *)ddr, (int)nt, di, dd,
                           KnnFrames{});
    FisheyeStereo S;
    S.rig = drig; S.kl = dkl; S.kr = dkr;
    S.nl = dn; S.ml = dn + 1; S.nr = dn + 2; S.mr = dn + 3;
    S.capL = n_left; S.capR = n_right;
    S.sigma2 = ds; S.knn_idx = di; S.knn_dist = dd;
    S.l2r = dl2r; S.r2l = dr2l; S.depth = ddep; S.p3d = dp; S.counts = dcnt;
    hipLaunchKernelGGL(k_tri_kb8_stereo, dim3((unsigned)((NL + 255) / 256), 1), dim3(256), 0, m->exec(), S);
    ORBX_HIP(hipGetLastError());
    int32_t cnt[4] = {0, 0, 0, 0};
    ORBX_TRY(m->d2h(l2r, dl2r, 4 * NL)); ORBX_TRY(m->d2h(depth, ddep, 4 * NL)); ORBX_TRY(m->d2h(p3d, dp, 12 * NL)); ORBX_TRY(m->d2h(r2l, dr2l, 4 * NR)); ORBX_TRY(m->d2h(cnt, dcnt, 16));
    ORBX_TRY(m->sync_and_deliver());
    if (desc_matches) *desc_matches = cnt[1];
    return cnt[0];
}

// test hook: KannalaBrandt8::epipolarConstrain of n independent pairs on the device (k_debug_kb8_gate); sel[i] = 2 * right1 + right2 picks cam1[right1],
// cam2[right2] and R12 / t12 [sel] as the search does per candidate
int orbx_debug_kb8_epipolar(orbx_matcher *m, const float *cam1_2x8, const float *cam2_2x8, const float *R12_4x9, const float *t12_4x3, int n, const float *xy1,
                            const float *xy2, const float *sigma1, const float *sigma2, const uint8_t *sel, uint8_t *ok) {
    if (!m || !cam1_2x8 || !cam2_2x8 || !R12_4x9 || !t12_4x3 || n < 0 || (n > 0 && (!xy1 || !xy2 || !sigma1 || !sigma2 || !sel || !ok))) return ORBX_E_BAD_ARG;
    if (n == 0) return ORBX_OK;
    for (int i = 0; i < n; i++) if (sel[i] > 3) return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(m->device));
    const size_t N = (size_t)n;
    Kb8Gate K;
    memset(&K, 0, sizeof(K));
    memcpy(K.cam[0], cam1_2x8, sizeof(float) * 16);
    memcpy(K.cam[2], cam2_2x8, sizeof(float) * 16);
    memcpy(K.R12, R12_4x9, sizeof(K.R12));
    memcpy(K.t12, t12_4x3, sizeof(K.t12));
    float *d1, *d2, *s1, *s2;
    uint8_t *dsel, *dok;
    Kb8Gate *dg;
    ORBX_TRY(m->carve([&](Carve &A) {
        d1 = A.up(xy1, 2 * N); d2 = A.up(xy2, 2 * N); s1 = A.up(sigma1, N); s2 = A.up(sigma2, N);
        dsel = A.up(sel, N); dok = A.take<uint8_t>(N);
        dg = A.up(&K, 1);
    }));
    hipLaunchKernelGGL(k_debug_kb8_gate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->exec(), (const Kb8Gate *)dg, n, (const float *)d1, (const float *)d2,
                       (const float *)s1, (const float *)s2, (const uint8_t *)dsel, dok);
    ORBX_HIP(hipGetLastError());
    ORBX_TRY(m->d2h(ok, dok, N));
    ORBX_TRY(m->sync_and_deliver());
    return ORBX_OK;
}

}  // extern "C"

// The internal result buffers (downloaded by orbx_batch_download_async) for one of the two batched matchers of the current batch: owner 1 the
// frame-to-frame matcher, 2 the map-point search (one matcher per batch: orbx.h).
static int claim_internal_match(orbx_extractor *ex, int owner, int32_t **d_match, int32_t **d_nmatches) {
    if (ex->internal_match_owner == 3 - owner) {
        set_error(owner == 1 ? "the internal match buffers hold the map-point search of this batch: download it first, or pass result buffers"
                             : "the internal match buffers hold the frame-to-frame matches of this batch: download them first, or pass result buffers");
        return ORBX_E_BAD_ARG;
    }
    ex->internal_match_owner = owner;
    const size_t mb = 4 * (size_t)ex->cap * ex->batch_cap, nb = 4 * (size_t)ex->batch_cap;
    if (ex->d_match.bytes < mb || ex->d_nmatch.bytes < nb) {
        // growing frees the old buffers: an earlier matcher / download may still be using them
        ORBX_HIP(hipStreamSynchronize(ex->match_stream)); ORBX_HIP(hipStreamSynchronize(ex->copy_stream));
    }
    ORBX_TRY(ex->d_match.ensure(mb));
    ORBX_TRY(ex->d_nmatch.ensure(nb));
    *d_match = (int32_t *)ex->d_match.p;
    *d_nmatches = (int32_t *)ex->d_nmatch.p;
    return ORBX_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Device-resident batched frame-to-frame matcher (throughput path): problem f-1 matches frame f-1 (queries)
// into frame f of the extractor's last batch; everything stays in HBM on the extractor's stream.
// ---------------------------------------------------------------------------------------------------------
extern "C" int orbx_match_consecutive_device(orbx_extractor *ex, float th, float du, float dv, int check_orientation,
                                             int32_t *d_match, int32_t *d_nmatches) {
    RoctxRange rr("orbx:match_consecutive");
    if (!ex) return ORBX_E_BAD_ARG;
    const int n = ex->last_batch;
    if (n < 2) return ORBX_OK;
    if (ex->cap > kMaxResolveFeatures) return ORBX_E_TOO_LARGE;
    ORBX_HIP(hipSetDevice(ex->device));
    const int np = n - 1, cap = ex->cap;
    if (!d_match || !d_nmatches) ORBX_TRY(claim_internal_match(ex, 1, &d_match, &d_nmatches));
    const orbx_keypoint *kps = (const orbx_keypoint *)ex->match_kps();   // mvKeysUn (== mvKeys without a distortion model)
    orbx_extractor::MatchKey key;
    key.n = n; key.cap = cap; key.match = d_match; key.nm = d_nmatches; key.th = th; key.du = du; key.dv = dv;
    key.ori = check_orientation; key.kps = kps;
    if (!(key == ex->mkey)) {  // (re)build the per-pair problem descriptors; steady-state batches reuse them without any host sync
        ORBX_HIP(hipStreamSynchronize(ex->match_stream));   // the scratch below may be in use by the previous batch's matcher
        ORBX_TRY(ex->d_mkey1.ensure(8 * (size_t)kTopK * cap * np));
        ORBX_TRY(ex->d_mkey2.ensure(4 * (size_t)cap * np));
        ORBX_TRY(ex->d_mentries.ensure(4 * (size_t)cap * np));
        ORBX_TRY(ex->d_mgrid.ensure(2 * ((size_t)kGridCells + 1 + 63 + cap) * np));
        ORBX_TRY(ex->d_mprobs.ensure(sizeof(WindowProblem) * (size_t)np));
        ORBX_TRY(ex->d_mres.ensure(sizeof(ResolveProblem) * (size_t)np));
        ORBX_TRY(ex->d_mscale.ensure(sizeof(float) * ex->prm.nlevels));
        std::vector<WindowProblem> P(np);
        std::vector<ResolveProblem> R(np);
        const uint8_t *desc = (const uint8_t *)ex->d_desc.p;
        const int32_t *count = (const int32_t *)ex->d_count.p;
        for (int p = 0; p < np; p++) {
            const int f = p + 1;
            WindowProblem &w = P[p];
            memset(&w, 0, sizeof(w));
            w.kps = kps + (size_t)f * cap; w.desc = desc + (size_t)f * cap * 32; w.n_ptr = count + f;
            w.q_from_kps = kps + (size_t)(f - 1) * cap; w.qdesc = desc + (size_t)(f - 1) * cap * 32; w.nq_ptr = count + (f - 1);
            w.th = th; w.du = du; w.dv = dv;
            w.scale = (const float *)ex->d_mscale.p;  // mvScaleFactors
            w.gstart = (uint16_t *)ex->d_mgrid.p + (size_t)p * (kGridCells + 64 + cap);
            w.gorder = w.gstart + kGridCells + 64;
            w.keys = (u64 *)ex->d_mkey1.p + (size_t)p * cap * kTopK; w.meta = (int32_t *)ex->d_mkey2.p + (size_t)p * cap;
            ResolveProblem &q = R[p];
            memset(&q, 0, sizeof(q));
            q.mode = 2; q.check_orientation = check_orientation; q.max_dist = (float)ORBX_TH_HIGH; q.cleared_value = -1;
            q.match = d_match + (size_t)f * cap; q.nmatches = d_nmatches + f;
            q.entries = (int32_t *)ex->d_mentries.p + (size_t)p * cap;
        }
        ORBX_HIP(hipMemcpyAsync(ex->d_mscale.p, ex->scale.data(), sizeof(float) * ex->prm.nlevels, hipMemcpyHostToDevice, ex->stream));
        ORBX_HIP(hipMemcpyAsync(ex->d_mprobs.p, P.data(), sizeof(WindowProblem) * np, hipMemcpyHostToDevice, ex->stream));
        ORBX_HIP(hipMemcpyAsync(ex->d_mres.p, R.data(), sizeof(ResolveProblem) * np, hipMemcpyHostToDevice, ex->stream));
        ORBX_HIP(hipStreamSynchronize(ex->stream));  // P/R are host temporaries
        ex->mkey = key;
    }
    const GridParams g = grid_of(ex->bounds);  // mnMinX.. of the extractor's camera (image rectangle without one, Frame.cc:804-807)
    // the matcher of batch i runs on its own stream beside the pyramid / FAST / quad-tree of batch i+1
    const hipStream_t ms = stage_stream(ex);
    ORBX_TRY(stage_begin(ms, {ex}));
    hipEvent_t e0 = ex->ev0, e1 = ex->ev1;
    if (ex->profile) (void)hipEventRecord(e0, ms);
    ORBX_LAUNCH_GRID_BUILD( dim3(np), dim3(64), 0, ms, (const WindowProblem *)ex->d_mprobs.p, g);
    ORBX_LAUNCH_WINDOW_BEST2(cap, np, ms, (const WindowProblem *)ex->d_mprobs.p, g);
    if (ex->profile) {
        (void)hipEventRecord(e1, ms); (void)hipEventSynchronize(e1);
        float t = 0; (void)hipEventElapsedTime(&t, e0, e1);
        ex->prof_ms[K_MATCH_SCAN] += t; ex->prof_n[K_MATCH_SCAN]++;
        (void)hipEventRecord(e0, ms);
    }
    { const int rr = launch_resolve<false>(np, ms, (const WindowProblem *)ex->d_mprobs.p, (const ResolveProblem *)ex->d_mres.p, g, cap, cap, 1); if (rr != ORBX_OK) return rr; }
    if (ex->profile) {
        (void)hipEventRecord(e1, ms); (void)hipEventSynchronize(e1);
        float t = 0; (void)hipEventElapsedTime(&t, e0, e1);
        ex->prof_ms[K_MATCH_RESOLVE] += t; ex->prof_n[K_MATCH_RESOLVE]++;
    }
    return stage_end(ms, {ex});
}

// ---------------------------------------------------------------------------------------------------------
// SearchByProjection(Frame&, vector<MapPoint*>&, th, bFarPoints, thFarPoints) (ORBmatcher.cc:39-141; Tracking::SearchLocalPoints,
// Tracking.cc:3390-3413) for every frame of the resident batch against device-resident map-point data: per (frame, map point)
// the projection (mTrackProjX/Y), predicted level and viewing cosine that Frame::isInFrustum left in the MapPoint, plus the
// map points' descriptors.  Monocular / Nleft == -1 form with all features free on entry.
// ---------------------------------------------------------------------------------------------------------
extern "C" int orbx_search_mappoints_batch_device(orbx_extractor *ex, int n_mp, const float *d_proj_x, const float *d_proj_y,
                                                  const int32_t *d_level, const float *d_view_cos, const uint8_t *d_in_view,
                                                  const uint8_t *d_mp_desc, size_t desc_frame_stride, float th, float nnratio,
                                                  int32_t *d_match, int32_t *d_nmatches) {
    RoctxRange rr("orbx:search_mappoints");
    if (!ex || n_mp < 0 || (n_mp > 0 && (!d_proj_x || !d_proj_y || !d_level || !d_view_cos || !d_mp_desc))) return ORBX_E_BAD_ARG;
    const int n = ex->last_batch;
    if (n < 1) return ORBX_E_BAD_ARG;
    if (ex->cap > kMaxResolveFeatures) return ORBX_E_TOO_LARGE;
    ORBX_HIP(hipSetDevice(ex->device));
    const int cap = ex->cap;
    if (!d_match || !d_nmatches) ORBX_TRY(claim_internal_match(ex, 2, &d_match, &d_nmatches));
    const orbx_keypoint *kps = (const orbx_keypoint *)ex->match_kps();
    orbx_extractor::MpKey key;
    key.n = n; key.cap = cap; key.n_mp = n_mp; key.px = d_proj_x; key.py = d_proj_y; key.lvl = d_level; key.vc = d_view_cos; key.iv = d_in_view;
    key.desc = d_mp_desc; key.match = d_match; key.nm = d_nmatches; key.kps = kps; key.dstride = desc_frame_stride; key.th = th; key.ratio = nnratio;
    const size_t nq_all = (size_t)std::max(n_mp, 1) * n;
    if (!(key == ex->mpkey)) {  // (re)build the per-frame problem descriptors; steady-state batches reuse them without a host sync
        ORBX_HIP(hipStreamSynchronize(ex->match_stream));   // the scratch below may be in use by the previous batch's matcher
        ORBX_TRY(ex->d_mp_qr.ensure(4 * nq_all)); ORBX_TRY(ex->d_mp_qmin.ensure(4 * nq_all)); ORBX_TRY(ex->d_mp_qmax.ensure(4 * nq_all)); ORBX_TRY(ex->d_mp_valid.ensure(nq_all));
        ORBX_TRY(ex->d_mp_keys.ensure(8 * (size_t)kTopK * nq_all)); ORBX_TRY(ex->d_mp_meta.ensure(4 * nq_all));
        ORBX_TRY(ex->d_mp_grid.ensure(2 * ((size_t)kGridCells + 1 + 63 + cap) * n));
        ORBX_TRY(ex->d_mp_entries.ensure(4 * nq_all));
        ORBX_TRY(ex->d_mp_probs.ensure(sizeof(WindowProblem) * (size_t)n));
        ORBX_TRY(ex->d_mp_res.ensure(sizeof(ResolveProblem) * (size_t)n));
        ORBX_TRY(ex->d_mp_misc.ensure(256 + sizeof(float) * ex->prm.nlevels));
        std::vector<WindowProblem> P(n);
        std::vector<ResolveProblem> R(n);
        const uint8_t *desc = (const uint8_t *)ex->d_desc.p;
        const int32_t *count = (const int32_t *)ex->d_count.p;
        int32_t *d_nq = (int32_t *)ex->d_mp_misc.p;
        float *d_scale = (float *)((uint8_t *)ex->d_mp_misc.p + 256);
        for (int f = 0; f < n; f++) {
            WindowProblem &w = P[f];
            memset(&w, 0, sizeof(w));
            w.kps = kps + (size_t)f * cap; w.desc = desc + (size_t)f * cap * 32; w.n_ptr = count + f;
            w.qx = d_proj_x + (size_t)f * n_mp; w.qy = d_proj_y + (size_t)f * n_mp;
            w.qr = (const float *)ex->d_mp_qr.p + (size_t)f * n_mp;
            w.qmin = (const int32_t *)ex->d_mp_qmin.p + (size_t)f * n_mp; w.qmax = (const int32_t *)ex->d_mp_qmax.p + (size_t)f * n_mp;
            w.qdesc = d_mp_desc + (size_t)f * desc_frame_stride;
            w.qvalid = (const uint8_t *)ex->d_mp_valid.p + (size_t)f * n_mp;
            w.nq_ptr = d_nq;
            w.gstart = (uint16_t *)ex->d_mp_grid.p + (size_t)f * (kGridCells + 64 + cap);
            w.gorder = w.gstart + kGridCells + 64;
            w.keys = (u64 *)ex->d_mp_keys.p + (size_t)f * n_mp * kTopK; w.meta = (int32_t *)ex->d_mp_meta.p + (size_t)f * n_mp;
            ResolveProblem &q = R[f];
            memset(&q, 0, sizeof(q));
            q.mode = 1; q.nnratio = nnratio; q.max_dist = (float)ORBX_TH_HIGH; q.cleared_value = -1;
            q.match = d_match + (size_t)f * cap; q.nmatches = d_nmatches + f;
            q.entries = (int32_t *)ex->d_mp_entries.p + (size_t)f * n_mp;
        }
        const int32_t nq_host = n_mp;
        ORBX_HIP(hipMemcpyAsync(d_nq, &nq_host, 4, hipMemcpyHostToDevice, ex->stream));
        ORBX_HIP(hipMemcpyAsync(d_scale, ex->scale.data(), sizeof(float) * ex->prm.nlevels, hipMemcpyHostToDevice, ex->stream));
        ORBX_HIP(hipMemcpyAsync(ex->d_mp_probs.p, P.data(), sizeof(WindowProblem) * n, hipMemcpyHostToDevice, ex->stream));
        ORBX_HIP(hipMemcpyAsync(ex->d_mp_res.p, R.data(), sizeof(ResolveProblem) * n, hipMemcpyHostToDevice, ex->stream));
        ORBX_HIP(hipStreamSynchronize(ex->stream));  // P/R are host temporaries
        ex->mpkey = key;
    }
    const GridParams g = grid_of(ex->bounds);  // mnMinX.. of the extractor's camera (image rectangle without one, Frame.cc:804-807)
    const hipStream_t ms = stage_stream(ex);
    ORBX_TRY(stage_begin(ms, {ex}));
    if (n_mp > 0)
        hipLaunchKernelGGL(k_mappoint_windows, dim3((n_mp + 255) / 256, n), dim3(256), 0, ms, n_mp, d_level, d_view_cos, d_in_view,
                           (const float *)((const uint8_t *)ex->d_mp_misc.p + 256), ex->prm.nlevels, th, (float *)ex->d_mp_qr.p,
                           (int32_t *)ex->d_mp_qmin.p, (int32_t *)ex->d_mp_qmax.p, (uint8_t *)ex->d_mp_valid.p);
    ORBX_LAUNCH_GRID_BUILD( dim3(n), dim3(64), 0, ms, (const WindowProblem *)ex->d_mp_probs.p, g);
    if (n_mp > 0)
        ORBX_LAUNCH_WINDOW_BEST2(n_mp, n, ms, (const WindowProblem *)ex->d_mp_probs.p, g);
    { const int rr = launch_resolve<false>(n, ms, (const WindowProblem *)ex->d_mp_probs.p, (const ResolveProblem *)ex->d_mp_res.p, g, cap, 0, 4); if (rr != ORBX_OK) return rr; }
    return stage_end(ms, {ex});
}

// ---------------------------------------------------------------------------------------------------------
// Candidate generation: Frame::UndistortKeyPoints, ComputeImageBounds, isInFrustum
// ---------------------------------------------------------------------------------------------------------
namespace {
inline CameraModel model_of(const orbx_camera *c) { return CameraModel{c->fx, c->fy, c->cx, c->cy, c->k1, c->k2, c->p1, c->p2, c->k3}; }
}  // namespace

extern "C" int orbx_image_bounds(const orbx_camera *cam, int width, int height, float *bounds4) {
    if (!cam || !bounds4 || width <= 0 || height <= 0) return ORBX_E_BAD_ARG;
    image_bounds(model_of(cam), width, height, bounds4);
    return ORBX_OK;
}

extern "C" int orbx_undistort_keypoints(orbx_matcher *m, const orbx_camera *cam, const orbx_keypoint *kps, int n, orbx_keypoint *kps_un) {
    if (!m || !cam || n < 0 || (n > 0 && (!kps || !kps_un))) return ORBX_E_BAD_ARG;
    if (n == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(m->device));
    orbx_keypoint *di, *dou;
    ORBX_TRY(m->carve([&](Carve &A) { di = A.up(kps, (size_t)n); dou = A.take<orbx_keypoint>(n); }));
    hipLaunchKernelGGL(k_undistort, dim3((n + 255) / 256, 1), dim3(256), 0, m->exec(), model_of(cam), (const orbx_keypoint *)di, (const int32_t *)nullptr, n, dou);
    ORBX_TRY(m->d2h(kps_un, dou, sizeof(orbx_keypoint) * (size_t)n));
    ORBX_TRY(m->sync_and_deliver());
    return ORBX_OK;
}

extern "C" int orbx_is_in_frustum(orbx_matcher *m, const orbx_camera *cam, const orbx_frame_pose *pose, const float *bounds4, float log_scale_factor,
                                  int nlevels, float viewing_cos_limit, int n_mp, const float *pos, const float *normal, const float *min_dist,
                                  const float *max_dist, uint8_t *in_view, float *proj_x, float *proj_y, float *proj_xr, float *depth, int32_t *level,
                                  float *view_cos) {
    if (!m || !cam || !pose || !bounds4 || nlevels < 1 || n_mp < 0) return ORBX_E_BAD_ARG;
    if (n_mp > 0 && (!pos || !normal || !min_dist || !max_dist || !in_view || !proj_x || !proj_y || !proj_xr || !depth || !level || !view_cos)) return ORBX_E_BAD_ARG;
    if (n_mp == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(m->device));
    const size_t n = (size_t)n_mp;
    float *dp, *dn, *dmn, *dmx, *dx, *dy, *dxr, *dd, *dvc;
    uint8_t *div;
    int32_t *dl;
    FrustumFrame *dF;
    ORBX_TRY(m->carve([&](Carve &A) {   // (the inputs are staged below: by the kernel itself where it reads the mirror)
        dp = A.take<float>(3 * n); dn = A.take<float>(3 * n); dmn = A.take<float>(n); dmx = A.take<float>(n);
        div = A.take<uint8_t>(n);
        dx = A.take<float>(n); dy = A.take<float>(n); dxr = A.take<float>(n); dd = A.take<float>(n); dvc = A.take<float>(n);
        dl = A.take<int32_t>(n);
        dF = A.take<FrustumFrame>(1);
    }));
    const FrustumFrame F = frustum_frame(cam, pose, bounds4, log_scale_factor, nlevels, viewing_cos_limit);
    if (m->direct_ok(57 * n)) {   // streaming kernel, small call: its lanes read the staged inputs from and write the results into the pinned mirror (one launch)
        m->stage_direct(dF, &F, sizeof(F));
        m->stage_direct(dp, pos, 12 * n); m->stage_direct(dn, normal, 12 * n); m->stage_direct(dmn, min_dist, 4 * n); m->stage_direct(dmx, max_dist, 4 * n);
        hipLaunchKernelGGL(k_in_frustum, dim3((n_mp + 255) / 256, 1), dim3(256), 0, m->exec(), (const FrustumFrame *)m->host_view(dF), n_mp,
                           (const float *)m->host_view(dp), (const float *)m->host_view(dn), (const float *)m->host_view(dmn), (const float *)m->host_view(dmx),
                           m->host_view(div), m->host_view(dx), m->host_view(dy), m->host_view(dxr), m->host_view(dd), m->host_view(dl), m->host_view(dvc));
        m->result_direct(in_view, div, n); m->result_direct(proj_x, dx, 4 * n); m->result_direct(proj_y, dy, 4 * n); m->result_direct(proj_xr, dxr, 4 * n);
        m->result_direct(depth, dd, 4 * n); m->result_direct(level, dl, 4 * n); m->result_direct(view_cos, dvc, 4 * n);
        ORBX_TRY(m->sync_and_deliver());
        return ORBX_OK;
    }
    ORBX_TRY(m->h2d(dF, &F, sizeof(F)));
    ORBX_TRY(m->h2d(dp, pos, 12 * n)); ORBX_TRY(m->h2d(dn, normal, 12 * n)); ORBX_TRY(m->h2d(dmn, min_dist, 4 * n)); ORBX_TRY(m->h2d(dmx, max_dist, 4 * n));
    hipLaunchKernelGGL(k_in_frustum, dim3((n_mp + 255) / 256, 1), dim3(256), 0, m->exec(), (const FrustumFrame *)dF, n_mp, (const float *)dp,
                       (const float *)dn, (const float *)dmn, (const float *)dmx, div, dx, dy, dxr, dd, dl, dvc);
    ORBX_TRY(m->d2h(in_view, div, n)); ORBX_TRY(m->d2h(proj_x, dx, 4 * n)); ORBX_TRY(m->d2h(proj_y, dy, 4 * n)); ORBX_TRY(m->d2h(proj_xr, dxr, 4 * n)); ORBX_TRY(m->d2h(depth, dd, 4 * n));
    ORBX_TRY(m->d2h(level, dl, 4 * n)); ORBX_TRY(m->d2h(view_cos, dvc, 4 * n));
    ORBX_TRY(m->sync_and_deliver());
    return ORBX_OK;
}

extern "C" int orbx_is_in_frustum_checks(orbx_matcher *m, const orbx_fisheye_view *views, int n_views, const float *bounds4, float log_scale_factor,
                                         int nlevels, float viewing_cos_limit, int n_mp, const float *pos, const float *normal, const float *min_dist,
                                         const float *max_dist, uint8_t *in_view, float *proj_x, float *proj_y, float *depth, int32_t *level,
                                         float *view_cos) {
    if (!m || !views || n_views < 1 || n_views > 2 || !bounds4 || nlevels < 1 || n_mp < 0) return ORBX_E_BAD_ARG;
    if (n_mp > 0 && (!pos || !normal || !min_dist || !max_dist || !in_view || !proj_x || !proj_y || !depth || !level || !view_cos)) return ORBX_E_BAD_ARG;
    if (n_mp == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(m->device));
    const size_t n = (size_t)n_mp, no = n * (size_t)n_views;
    FrustumChecks F;
    memset(&F, 0, sizeof(F));
    memcpy(F.view, views, sizeof(FisheyeView) * (size_t)n_views);
    F.minx = bounds4[0]; F.maxx = bounds4[1]; F.miny = bounds4[2]; F.maxy = bounds4[3];
    F.log_scale_factor = log_scale_factor; F.nlevels = nlevels; F.cos_limit = viewing_cos_limit;
    float *dp, *dn, *dmn, *dmx, *dx, *dy, *dd, *dvc;
    uint8_t *div;
    int32_t *dl;
    FrustumChecks *dF;
    ORBX_TRY(m->carve([&](Carve &A) {
        dp = A.up(pos, 3 * n); dn = A.up(normal, 3 * n); dmn = A.up(min_dist, n); dmx = A.up(max_dist, n);
        div = A.take<uint8_t>(no);
        dx = A.take<float>(no); dy = A.take<float>(no); dd = A.take<float>(no); dvc = A.take<float>(no);
        dl = A.take<int32_t>(no);
        dF = A.up(&F, 1);
    }));
    hipLaunchKernelGGL(k_in_frustum_checks, dim3((n_mp + 255) / 256, n_views), dim3(256), 0, m->exec(), (const FrustumChecks *)dF, n_mp, (const float *)dp,
                       (const float *)dn, (const float *)dmn, (const float *)dmx, div, dx, dy, dd, dl, dvc);
    ORBX_TRY(m->d2h(in_view, div, no)); ORBX_TRY(m->d2h(proj_x, dx, 4 * no)); ORBX_TRY(m->d2h(proj_y, dy, 4 * no)); ORBX_TRY(m->d2h(depth, dd, 4 * no)); ORBX_TRY(m->d2h(level, dl, 4 * no)); ORBX_TRY(m->d2h(view_cos, dvc, 4 * no));
    ORBX_TRY(m->sync_and_deliver());
    return ORBX_OK;
}

extern "C" int orbx_frustum_batch_device(orbx_extractor *ex, const orbx_camera *cam, const orbx_frame_pose *poses, int n_frames, const float *bounds4,
                                         float viewing_cos_limit, int n_mp, const float *d_pos, const float *d_normal, const float *d_min_dist,
                                         const float *d_max_dist, uint8_t *d_in_view, float *d_proj_x, float *d_proj_y, float *d_proj_xr,
                                         float *d_depth, int32_t *d_level, float *d_view_cos) {
    if (!ex || !cam || !poses || n_frames < 1 || n_mp < 0) return ORBX_E_BAD_ARG;
    if (n_mp > 0 && (!d_pos || !d_normal || !d_min_dist || !d_max_dist || !d_in_view || !d_proj_x || !d_proj_y || !d_proj_xr || !d_depth || !d_level || !d_view_cos))
        return ORBX_E_BAD_ARG;
    if (n_mp == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(ex->device));
    // On the stage stream, in front of the map-point search it feeds, but no stage of the protocol: k_in_frustum reads the caller's map points and the
    // poses uploaded here (ev_frustum guards their pinned ring), nothing of the extraction -- so it neither waits for ev_describe nor records ev_match.
    const hipStream_t ms = stage_stream(ex);
    if (ex->d_frustum_frames.bytes < sizeof(FrustumFrame) * (size_t)n_frames) ORBX_HIP(hipStreamSynchronize(ms));
    ORBX_TRY(ex->d_frustum_frames.ensure(sizeof(FrustumFrame) * (size_t)n_frames));
    const float *b = bounds4 ? bounds4 : ex->bounds;
    if (!bounds4 && ex->width <= 0) return ORBX_E_BAD_ARG;
    const float log_sf = logf((float)(double)ex->prm.scale_factor);   // Frame::mfLogScaleFactor = log(mfScaleFactor) (Frame.cc:120)
    // the per-batch pose upload goes through a pinned ring of three slots owned by the library (no caller or pageable memory reaches the
    // HIP runtime, and the host never waits for the matcher stream): a slot is reused once the copy out of it has run
    const unsigned slot = ex->frustum_issued % 3u;
    const size_t fbytes = sizeof(FrustumFrame) * (size_t)n_frames;
    if (ex->frustum_used[slot]) ORBX_HIP(hipEventSynchronize(ex->ev_frustum[slot]));
    if (ex->h_frustum_bytes[slot] < fbytes) {
        if (ex->h_frustum[slot]) ORBX_HIP(hipHostFree(ex->h_frustum[slot]));
        ex->h_frustum[slot] = nullptr; ex->h_frustum_bytes[slot] = 0;
        ORBX_HIP(hipHostMalloc(&ex->h_frustum[slot], fbytes, hipHostMallocDefault));
        ex->h_frustum_bytes[slot] = fbytes;
    }
    if (!ex->ev_frustum[slot]) ORBX_HIP(hipEventCreateWithFlags(&ex->ev_frustum[slot], hipEventDisableTiming));
    FrustumFrame *F = (FrustumFrame *)ex->h_frustum[slot];
    for (int f = 0; f < n_frames; f++) F[f] = frustum_frame(cam, poses + f, b, log_sf, ex->prm.nlevels, viewing_cos_limit);
    ORBX_HIP(hipMemcpyAsync(ex->d_frustum_frames.p, F, fbytes, hipMemcpyHostToDevice, ms));
    ORBX_HIP(hipEventRecord(ex->ev_frustum[slot], ms));
    ex->frustum_used[slot] = true;
    ex->frustum_issued++;
    hipLaunchKernelGGL(k_in_frustum, dim3((n_mp + 255) / 256, n_frames), dim3(256), 0, ms, (const FrustumFrame *)ex->d_frustum_frames.p, n_mp, d_pos,
                       d_normal, d_min_dist, d_max_dist, d_in_view, d_proj_x, d_proj_y, d_proj_xr, d_depth, d_level, d_view_cos);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Frame::ComputeStereoMatches (Frame.cc:811-981) for every frame of two resident batches (left / right extractor):
// row-band Hamming, SAD refinement on the device-resident pyramids, median rejection -- nothing leaves HBM until
// the results are downloaded.  Runs on the left extractor's stream behind both extractions.
// ---------------------------------------------------------------------------------------------------------
extern "C" int orbx_stereo_batch_device(orbx_extractor *L, orbx_extractor *R, float bf, float b) {
    RoctxRange rr("orbx:stereo");
    if (!L || !R || !(b > 0.f)) return ORBX_E_BAD_ARG;
    if (L->last_batch <= 0 || L->last_batch != R->last_batch || L->width != R->width || L->height != R->height ||
        L->prm.nlevels != R->prm.nlevels || L->device != R->device)
        return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(L->device));
    const int n = L->last_batch, capL = L->cap, nl = L->prm.nlevels;
    ORBX_TRY(L->d_st_bidx.ensure(4 * (size_t)capL * L->batch_cap));
    ORBX_TRY(L->d_st_bdist.ensure(4 * (size_t)capL * L->batch_cap));
    ORBX_TRY(L->d_st_ur.ensure(4 * (size_t)capL * L->batch_cap));
    ORBX_TRY(L->d_st_depth.ensure(4 * (size_t)capL * L->batch_cap));
    ORBX_TRY(L->d_st_sad.ensure(4 * (size_t)capL * L->batch_cap));
    ORBX_TRY(L->d_st_nm.ensure(4 * (size_t)L->batch_cap));
    ORBX_TRY(L->d_st_scales.ensure(sizeof(float) * 2 * nl));
    StereoBatch S;
    stereo_index_params(S, L->height, L->scale.data(), nl);
    ORBX_TRY(L->d_st_rowptr.ensure(4 * ((size_t)S.n_buckets + 1) * L->batch_cap));
    ORBX_TRY(L->d_st_rowidx.ensure(16 * (size_t)R->cap * L->batch_cap));
    // From now on both extractors alternate between two pyramid slabs: these kernels run on the left extractor's MATCH stream beside the next
    // pair of extractions, and k_stereo_sad reads the pyramids of THIS pair.  (The slab written next is the one the stereo stage before this
    // one read: every extraction waits for the rig's previous stereo stage before its k_finalize -- match_pending -- and the one after it
    // follows on the same stream.)
    for (orbx_extractor *e : {L, R}) {
        // a pair extracted before the rig existed may have read its level 0 in place: the SAD stage needs the padded level in the slab
        ORBX_TRY(orbx_materialize_level0(e));
        if (!e->pyr_double) {
            ORBX_TRY(e->d_pyr2.ensure(e->d_pyr.bytes));
            e->pyr_double = true;   // pyr_slot stays: the current batch lies in the slab it was extracted into
        }
    }
    const hipStream_t st = stage_stream(L);
    ORBX_HIP(hipMemcpyAsync(L->d_st_scales.p, L->scale.data(), sizeof(float) * nl, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync((float *)L->d_st_scales.p + nl, L->inv_scale.data(), sizeof(float) * nl, hipMemcpyHostToDevice, st));
    ORBX_TRY(stage_begin(st, {L, R}, true));
    S.kl = (const orbx_keypoint *)L->d_kps.p; S.kr = (const orbx_keypoint *)R->d_kps.p;
    S.dl = (const uint8_t *)L->d_desc.p; S.dr = (const uint8_t *)R->d_desc.p;
    S.nl = (const int32_t *)L->d_count.p; S.nr = (const int32_t *)R->d_count.p;
    S.capL = capL; S.capR = R->cap;
    S.pyrL = L->pyr_cur(); S.pyrR = R->pyr_cur();
    S.pyr_frame_L = L->pyr_frame; S.pyr_frame_R = R->pyr_frame;
    S.lvL = (const LevelInfo *)L->d_lv.p; S.lvR = (const LevelInfo *)R->d_lv.p;
    S.scale = (const float *)L->d_st_scales.p; S.inv_scale = S.scale + nl;
    S.n_rows = L->height;
    S.bf = bf; S.b = b;
    S.best_idx = (int32_t *)L->d_st_bidx.p; S.best_dist = (int32_t *)L->d_st_bdist.p;
    S.u_right = (float *)L->d_st_ur.p; S.depth = (float *)L->d_st_depth.p;
    S.sad = (int32_t *)L->d_st_sad.p; S.nmatches = (int32_t *)L->d_st_nm.p;
    S.row_ptr = (const int32_t *)L->d_st_rowptr.p; S.row_ent = (const uint4 *)L->d_st_rowidx.p;
    hipLaunchKernelGGL(k_stereo_row_index, dim3(n), dim3(256), 4 * ((size_t)S.n_buckets + 1) + 1024, st, S, (int32_t *)L->d_st_rowptr.p, (uint4 *)L->d_st_rowidx.p);
    hipLaunchKernelGGL(k_stereo_rowband_batch, dim3((capL + 15) / 16, n), dim3(256), 0, st, S);
    hipLaunchKernelGGL(k_stereo_sad, dim3((capL + 15) / 16, n), dim3(256), 0, st, S);
    hipLaunchKernelGGL(k_stereo_reject, dim3(n), dim3(256), 0, st, S);
    ORBX_TRY(stage_end(st, {L, R}));   // the right extractor's next k_finalize waits for it as for a matcher of its own
    L->st_seq = L->batch_seq;   // (orbx_frame_load_stereo_batch: the results are this batch's)
    return ORBX_OK;
}

// Frame::ComputeStereoFromRGBD for every frame of a resident batch, float depth images (k_stereo_from_rgbd): rgbd_stage, extractor_state.h
extern "C" int orbx_rgbd_batch_device(orbx_extractor *ex, const float *d_depth, size_t pitch_bytes, size_t frame_stride_bytes, float bf) {
    RoctxRange rr("orbx:rgbd");
    if (!ex || !d_depth || ex->last_batch <= 0 || ex->width <= 0 || pitch_bytes < 4 * (size_t)ex->width || !(bf > 0.f)) return ORBX_E_BAD_ARG;
    // every row of every image must be a row of aligned floats
    if (((uintptr_t)d_depth | pitch_bytes | frame_stride_bytes) & 3u) return ORBX_E_BAD_ARG;
    return rgbd_stage(ex, RgbdStage{}, k_stereo_from_rgbd, d_depth, pitch_bytes, frame_stride_bytes, bf);
}

extern "C" int orbx_stereo_batch_download(orbx_extractor *L, int frame, float *u_right, float *depth, int *n_left, int *n_matches) {
    if (!L || frame < 0 || frame >= L->last_batch || !L->d_st_ur.p) return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(L->device));
    ORBX_HIP(hipStreamWaitEvent(L->stream, L->ev_match, 0));   // the stereo stage runs on the match stream
    const size_t fb = 4 * (size_t)L->cap;
    const int32_t *count = nullptr, *nm = nullptr;
    const float *ur = nullptr, *dp = nullptr;
    ORBX_TRY(L->download([&](Staged &S) {
        count = S.view<int32_t>((int32_t *)L->d_count.p + frame, 4);
        nm = S.view<int32_t>((int32_t *)L->d_st_nm.p + frame, 4);
        ur = S.view<float>((float *)L->d_st_ur.p + (size_t)frame * L->cap, fb);
        dp = S.view<float>((float *)L->d_st_depth.p + (size_t)frame * L->cap, fb);
    }));
    if (n_left) *n_left = *count;
    if (n_matches) *n_matches = *nm;
    const int nlv = std::min(std::max(*count, 0), L->cap);   // the rows are the frame's capacity on the device, the caller's arrays its count
    if (u_right) memcpy(u_right, ur, 4 * (size_t)nlv);
    if (depth) memcpy(depth, dp, 4 * (size_t)nlv);
    return ORBX_OK;
}

// all frames of the last stereo batch at once: u_right / depth [n_frames][cap] (-1 where unmatched; entries beyond a frame's
// keypoint count are unspecified), n_matches [n_frames]; synchronous on the left extractor's stream.  The destinations may be
// pinned (copied directly would be possible) or pageable: they are always filled from the pinned staging buffer.
extern "C" int orbx_stereo_batch_download_all(orbx_extractor *L, float *u_right, float *depth, int32_t *n_matches) {
    if (!L || L->last_batch <= 0 || !L->d_st_ur.p) return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(L->device));
    ORBX_HIP(hipStreamWaitEvent(L->stream, L->ev_match, 0));   // the stereo stage runs on the match stream
    const size_t n = (size_t)L->last_batch, fb = 4 * n * L->cap;
    return L->download([&](Staged &S) {
        S.out(u_right, L->d_st_ur.p, fb);
        S.out(depth, L->d_st_depth.p, fb);
        S.out(n_matches, L->d_st_nm.p, 4 * n);
    });
}

// the same into PINNED host buffers, asynchronously on the left extractor's copy stream behind the stereo kernels: the pipelined form
// (the next pair of batches is extracted while these results travel).  At most two such downloads in flight; orbx_stereo_download_wait ends the older, and
// the next orbx_stereo_batch_device waits for it on the device before it overwrites the result buffers.
extern "C" int orbx_stereo_batch_download_async(orbx_extractor *L, float *u_right, float *depth, int32_t *n_matches) {
    if (!L || L->last_batch <= 0 || !L->d_st_ur.p) return ORBX_E_BAD_ARG;
    if (L->stereo_copy_issued - L->stereo_copy_waited >= 2) { set_error("two stereo downloads already in flight: call orbx_stereo_download_wait first"); return ORBX_E_BAD_ARG; }
    for (const void *p : {(const void *)u_right, (const void *)depth, (const void *)n_matches})
        if (!is_pinned_host(p)) { set_error("orbx_stereo_batch_download_async needs pinned host buffers (hipHostMalloc / hipHostRegister)"); return ORBX_E_BAD_ARG; }
    ORBX_HIP(hipSetDevice(L->device));
    for (hipEvent_t &ev : L->ev_stereo_copy) if (!ev) ORBX_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    const size_t n = (size_t)L->last_batch, fb = 4 * n * L->cap;
    hipStream_t cs = L->copy_stream;
    ORBX_HIP(hipStreamWaitEvent(cs, L->ev_match, 0));   // recorded behind k_stereo_reject
    if (u_right) ORBX_HIP(hipMemcpyAsync(u_right, L->d_st_ur.p, fb, hipMemcpyDeviceToHost, cs));
    if (depth) ORBX_HIP(hipMemcpyAsync(depth, L->d_st_depth.p, fb, hipMemcpyDeviceToHost, cs));
    if (n_matches) ORBX_HIP(hipMemcpyAsync(n_matches, L->d_st_nm.p, 4 * n, hipMemcpyDeviceToHost, cs));
    ORBX_HIP(hipEventRecord(L->ev_stereo_copy[L->stereo_copy_issued & 1], cs));
    L->stereo_copy_issued++;
    return ORBX_OK;
}

extern "C" int orbx_stereo_download_wait(orbx_extractor *L) {
    if (!L) return ORBX_E_BAD_ARG;
    if (L->stereo_copy_issued == L->stereo_copy_waited) return ORBX_OK;
    ORBX_HIP(hipSetDevice(L->device));
    ORBX_HIP(hipEventSynchronize(L->ev_stereo_copy[L->stereo_copy_waited & 1]));   // the OLDEST one in flight
    L->stereo_copy_waited++;
    return ORBX_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Frame::ComputeStereoFishEyeMatches (Frame.cc:1126-1166) for every frame pair of two resident batches (left / right extractor of a KannalaBrandt8 rig):
// k_knn2 per frame over the two lapping-area tails (the extractors' counts and mono indices on the device), then k_tri_kb8_stereo.  Ordered as
// orbx_stereo_batch_device minus the pyramid part: no pyramid level is read, so level 0 is not materialised and the extractors keep their single slab.
// Raw keypoints (mvKeys: a KB8 frame triangulates the distorted points), the left extractor's mvLevelSigma2, result buffers of its own.
// ---------------------------------------------------------------------------------------------------------
extern "C" int orbx_stereo_fisheye_batch_device(orbx_extractor *L, orbx_extractor *R, const orbx_kb8_rig *rig) {
    RoctxRange rr("orbx:stereo_fisheye");
    if (!L || !R || !rig) return ORBX_E_BAD_ARG;
    if (L->last_batch <= 0 || L->last_batch != R->last_batch || L->prm.nlevels != R->prm.nlevels || L->device != R->device) return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(L->device));
    const int n = L->last_batch, capL = L->cap, capR = R->cap, nl = L->prm.nlevels;
    const size_t NL = (size_t)n * capL, NR = (size_t)n * capR;
    if (NR + 4 * (size_t)n > (size_t)INT_MAX || nl > kMaxLevels || (int)L->sigma2.size() < nl) return ORBX_E_BAD_ARG;
    ORBX_TRY(L->d_sf_idx.ensure(8 * NL));
    ORBX_TRY(L->d_sf_dist.ensure(8 * NL));
    ORBX_TRY(L->d_sf_l2r.ensure(4 * NL));
    ORBX_TRY(L->d_sf_depth.ensure(4 * NL));
    ORBX_TRY(L->d_sf_p3d.ensure(12 * NL));
    ORBX_TRY(L->d_sf_r2l.ensure(4 * NR));
    ORBX_TRY(L->d_sf_cnt.ensure(16 * (size_t)n));
    ORBX_TRY(L->d_sf_sigma.ensure(sizeof(float) * kMaxLevels));
    ORBX_TRY(L->d_sf_rig.ensure(sizeof(orbx_kb8_rig)));
    const hipStream_t st = stage_stream(L);
    ORBX_TRY(stage_begin(st, {L, R}));   // (the downloads of these results are synchronous: none in flight)
    FisheyeStereoInit I;
    memset(&I, 0, sizeof(I));
    I.rig = *rig;
    for (int k = 0; k < nl; k++) I.sigma2[k] = L->sigma2[k];   // mvLevelSigma2: the frame's (left) table for both cameras (:1155)
    I.nlevels = nl;
    I.d_rig = (orbx_kb8_rig *)L->d_sf_rig.p; I.d_sigma2 = (float *)L->d_sf_sigma.p;
    I.r2l = (int32_t *)L->d_sf_r2l.p; I.counts = (int32_t *)L->d_sf_cnt.p;
    I.n_r2l = (int)NR; I.n_counts = 4 * n;
    const size_t n_init = std::max(NR, (size_t)4 * n);
    hipLaunchKernelGGL(k_tri_kb8_stereo_init, dim3((unsigned)((n_init + 255) / 256)), dim3(256), 0, st, I);
    const KnnFrames F{(const int32_t *)L->d_count.p, (const int32_t *)L->d_mono.p, (const int32_t *)R->d_count.p, (const int32_t *)R->d_mono.p, capL, capR};
    hipLaunchKernelGGL(k_knn2, dim3((unsigned)((capL + 3) / 4), (unsigned)n), dim3(256), 0, st, (const uint8_t *)L->d_desc.p, 0, (const uint8_t *)R->d_desc.p, 0,
                       (int32_t *)L->d_sf_idx.p, (int32_t *)L->d_sf_dist.p, F);
    FisheyeStereo S;
    S.rig = (const orbx_kb8_rig *)L->d_sf_rig.p;
    S.kl = (const orbx_keypoint *)L->d_kps.p; S.kr = (const orbx_keypoint *)R->d_kps.p;
    S.nl = (const int32_t *)L->d_count.p; S.ml = (const int32_t *)L->d_mono.p;
    S.nr = (const int32_t *)R->d_count.p; S.mr = (const int32_t *)R->d_mono.p;
    S.capL = capL; S.capR = capR;
    S.sigma2 = (const float *)L->d_sf_sigma.p;
    S.knn_idx = (const int32_t *)L->d_sf_idx.p; S.knn_dist = (const int32_t *)L->d_sf_dist.p;
    S.l2r = (int32_t *)L->d_sf_l2r.p; S.r2l = (int32_t *)L->d_sf_r2l.p;
    S.depth = (float *)L->d_sf_depth.p; S.p3d = (float *)L->d_sf_p3d.p; S.counts = (int32_t *)L->d_sf_cnt.p;
    hipLaunchKernelGGL(k_tri_kb8_stereo, dim3((unsigned)((capL + 255) / 256), (unsigned)n), dim3(256), 0, st, S);
    ORBX_HIP(hipGetLastError());
    L->sf_batch = n; L->sf_capL = capL; L->sf_capR = capR;
    L->sf_seq_l = L->batch_seq; L->sf_seq_r = R->batch_seq; L->sf_right = R;
    if (!L->ev_sf) ORBX_HIP(hipEventCreateWithFlags(&L->ev_sf, hipEventDisableTiming));
    ORBX_HIP(hipEventRecord(L->ev_sf, st));   // (orbx_frame_load_stereo_fisheye_batch waits for it)
    return stage_end(st, {L, R});
}

// one frame of the last fisheye stereo stage: l2r / depth [n_left], p3d [n_left][3], r2l [n_right] (any output may be NULL); synchronous
extern "C" int orbx_stereo_fisheye_batch_download(orbx_extractor *L, int frame, int32_t *l2r, int32_t *r2l, float *depth, float *p3d, int *n_left,
                                                  int *n_right, int *n_matches, int *desc_matches) {
    if (!L || frame < 0 || frame >= L->sf_batch || !L->d_sf_l2r.p) return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(L->device));
    ORBX_HIP(hipStreamWaitEvent(L->stream, L->ev_match, 0));   // the stage runs on the match stream
    const size_t cl = (size_t)L->sf_capL, cr = (size_t)L->sf_capR, f = (size_t)frame;
    const int32_t *h = nullptr, *h_l2r = nullptr, *h_r2l = nullptr;   // h: nMatches, descMatches, n_left, n_right
    const float *h_depth = nullptr, *h_p3d = nullptr;
    ORBX_TRY(L->download([&](Staged &S) {   // the rows are the frame's capacities on the device, the caller's arrays its counts: clamped below
        h = S.view<int32_t>((int32_t *)L->d_sf_cnt.p + 4 * f, 16);
        if (l2r) h_l2r = S.view<int32_t>((int32_t *)L->d_sf_l2r.p + f * cl, 4 * cl);
        if (depth) h_depth = S.view<float>((float *)L->d_sf_depth.p + f * cl, 4 * cl);
        if (p3d) h_p3d = S.view<float>((float *)L->d_sf_p3d.p + 3 * f * cl, 12 * cl);
        if (r2l) h_r2l = S.view<int32_t>((int32_t *)L->d_sf_r2l.p + f * cr, 4 * cr);
    }));
    const size_t nlv = (size_t)std::min(std::max(h[2], 0), L->sf_capL), nrv = (size_t)std::min(std::max(h[3], 0), L->sf_capR);
    if (n_matches) *n_matches = h[0];
    if (desc_matches) *desc_matches = h[1];
    if (n_left) *n_left = (int)nlv;
    if (n_right) *n_right = (int)nrv;
    if (l2r) memcpy(l2r, h_l2r, 4 * nlv);
    if (depth) memcpy(depth, h_depth, 4 * nlv);
    if (p3d) memcpy(p3d, h_p3d, 12 * nlv);
    if (r2l) memcpy(r2l, h_r2l, 4 * nrv);
    return ORBX_OK;
}

// all frames of the last fisheye stereo stage: l2r / depth [n_frames][cap_left], p3d [n_frames][cap_left][3], r2l [n_frames][cap_right] (entries beyond a
// frame's feature counts unspecified), n_matches / desc_matches [n_frames]; any output may be NULL; synchronous on the left extractor's stream
extern "C" int orbx_stereo_fisheye_batch_download_all(orbx_extractor *L, int32_t *l2r, int32_t *r2l, float *depth, float *p3d, int32_t *n_matches,
                                                      int32_t *desc_matches) {
    if (!L || L->sf_batch <= 0 || !L->d_sf_l2r.p) return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(L->device));
    ORBX_HIP(hipStreamWaitEvent(L->stream, L->ev_match, 0));
    const size_t n = (size_t)L->sf_batch, bl = 4 * n * L->sf_capL, br = 4 * n * L->sf_capR;
    const int32_t *c = nullptr;   // [n][4]: nMatches, descMatches, n_left, n_right
    ORBX_TRY(L->download([&](Staged &S) {
        if (n_matches || desc_matches) c = S.view<int32_t>(L->d_sf_cnt.p, 16 * n);
        S.out(depth, L->d_sf_depth.p, bl);
        S.out(l2r, L->d_sf_l2r.p, bl);
        S.out(p3d, L->d_sf_p3d.p, 3 * bl);
        S.out(r2l, L->d_sf_r2l.p, br);
    }));
    for (size_t f = 0; f < n; f++) {
        if (n_matches) n_matches[f] = c[4 * f];
        if (desc_matches) desc_matches[f] = c[4 * f + 1];
    }
    return ORBX_OK;
}

// ---------------------------------------------------------------------------------------------------------
// DBoW2 vocabulary on the device + TemplatedVocabulary::transform for all features of a frame (Frame::ComputeBoW,
// Frame.cc:738-745).  The tf-idf weighting / L1 normalisation of the BowVector (double arithmetic in std::map order)
// stays in the adapter: it needs only the word ids returned here.
// ---------------------------------------------------------------------------------------------------------
extern "C" int orbx_vocabulary_create(int device, int L, int n_nodes, const int32_t *child_ptr, const int32_t *child_idx,
                                      const uint8_t *node_desc, const int32_t *word_id, orbx_vocabulary **out) {
    if (!out || n_nodes <= 0 || !child_ptr || !child_idx || !node_desc || !word_id || L < 1) return ORBX_E_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        set_error("no usable HIP device (liborbx has no CPU fallback)");
        return ORBX_E_NO_DEVICE;
    }
    ORBX_HIP(hipSetDevice(device));
    orbx_vocabulary *v = new orbx_vocabulary();
    v->device = device; v->L = L; v->n_nodes = n_nodes;
    const int nchild = child_ptr[n_nodes];
    ORBX_HIP(hipMalloc((void **)&v->child_ptr, 4 * (size_t)(n_nodes + 1)));
    ORBX_HIP(hipMalloc((void **)&v->child_idx, 4 * (size_t)std::max(nchild, 1)));
    ORBX_HIP(hipMalloc((void **)&v->word_id, 4 * (size_t)n_nodes));
    ORBX_HIP(hipMalloc((void **)&v->node_desc, 32 * (size_t)n_nodes));
    ORBX_HIP(hipMemcpy(v->child_ptr, child_ptr, 4 * (size_t)(n_nodes + 1), hipMemcpyHostToDevice));
    ORBX_HIP(hipMemcpy(v->child_idx, child_idx, 4 * (size_t)nchild, hipMemcpyHostToDevice));
    ORBX_HIP(hipMemcpy(v->word_id, word_id, 4 * (size_t)n_nodes, hipMemcpyHostToDevice));
    ORBX_HIP(hipMemcpy(v->node_desc, node_desc, 32 * (size_t)n_nodes, hipMemcpyHostToDevice));
    for (int i = 0; i < n_nodes; i++) v->max_word = std::max(v->max_word, (int)word_id[i]);
    {   // nodes per depth, breadth first from the root (a malformed tree's cycles end at n_nodes visits)
        std::vector<int> cur{0}, next;
        size_t seen = 0;
        while (!cur.empty() && seen <= (size_t)n_nodes) {
            v->depth_nodes.push_back((int)cur.size());
            seen += cur.size();
            next.clear();
            for (int nd : cur)
                if (nd >= 0 && nd < n_nodes)
                    for (int c = child_ptr[nd]; c < child_ptr[nd + 1] && next.size() <= (size_t)n_nodes; c++) next.push_back(child_idx[c]);
            cur.swap(next);
        }
    }
    *out = v;
    return ORBX_OK;
}

extern "C" void orbx_vocabulary_destroy(orbx_vocabulary *v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    (void)hipFree(v->child_ptr); (void)hipFree(v->child_idx); (void)hipFree(v->word_id); (void)hipFree(v->node_desc);
    if (v->word_pos) (void)hipFree(v->word_pos);
    if (v->weight) (void)hipFree(v->weight);
    delete v;
}

// the stop-word test of TemplatedVocabulary::transform (`if (w > 0)`, TemplatedVocabulary.h:1170) reads the sign of each word's weight (word_pos);
// the weights themselves stay beside it for the BowVector (k_bow_vector)
extern "C" int orbx_vocabulary_set_word_weights(orbx_vocabulary *v, const double *weight, int n_words) {
    if (!v || !weight || n_words <= v->max_word || n_words <= 0) return ORBX_E_BAD_ARG;   // every word id of the tree needs a weight
    std::vector<uint8_t> pos((size_t)n_words);
    for (int i = 0; i < n_words; i++) pos[i] = weight[i] > 0 ? 1 : 0;
    ORBX_HIP(hipSetDevice(v->device));
    uint8_t *d = nullptr;
    double *dw = nullptr;
    ORBX_HIP(hipMalloc((void **)&d, (size_t)n_words));
    hipError_t e = hipMemcpy(d, pos.data(), (size_t)n_words, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&dw, 8 * (size_t)n_words);
    if (e == hipSuccess) e = hipMemcpy(dw, weight, 8 * (size_t)n_words, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); if (dw) (void)hipFree(dw); set_error(hipGetErrorString(e)); return ORBX_E_HIP; }
    if (v->word_pos) (void)hipFree(v->word_pos);
    if (v->weight) (void)hipFree(v->weight);
    v->word_pos = d; v->weight = dw; v->n_words = n_words;
    return ORBX_OK;
}

extern "C" int orbx_bow_transform(orbx_matcher *m, const orbx_vocabulary *v, const uint8_t *desc, int n, int levelsup, int32_t *word_id,
                                  int32_t *node_id) {
    if (!m || !v || n < 0 || (n > 0 && (!desc || !word_id || !node_id)) || m->device != v->device) return ORBX_E_BAD_ARG;
    if (n == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(m->device));
    uint8_t *dd;
    int32_t *dw, *dn;
    ORBX_TRY(m->carve([&](Carve &A) { dd = A.up(desc, 32 * (size_t)n); dw = A.take<int32_t>(n); dn = A.take<int32_t>(n); }));
    hipLaunchKernelGGL(k_bow_transform, dim3((n + 15) / 16), dim3(256), 0, m->exec(), v->child_ptr, v->child_idx, v->node_desc, v->word_id,
                       v->L, levelsup, dd, n, dw, dn);
    ORBX_TRY(m->d2h(word_id, dw, 4 * (size_t)n)); ORBX_TRY(m->d2h(node_id, dn, 4 * (size_t)n));
    ORBX_TRY(m->sync_and_deliver());
    return ORBX_OK;
}

namespace {

// What ComputeBoW reads and writes: the rows of a frame handle or of a key frame (a fisheye-stereo one: the row-space kernel pair), and the seven
// arrays that take the result.
struct BowTarget : HandleRows, BowArrays {};   // (rows() is HandleRows': the row EXTENT; the features the kernels may see are feats())
inline BowTarget bow_target(const HandleRows &r, const BowArrays &b) { return BowTarget{r, b}; }
// The ids of a fisheye-stereo handle as they go down: word ids, then node ids, renumbered from rows into features [0, N) at dids [2 nc]
// (k_frame_rows_to_features on `st`: with N_left still on the device nothing waits for it).
inline void launch_bow_ids_to_features(hipStream_t st, const HandleRows &r, const BowArrays &b, int nc, int32_t *dids) {
    const int32_t *src[2] = {b.word, b.node};
    for (int k = 0; k < 2; k++)
        hipLaunchKernelGGL(k_frame_rows_to_features, dim3((unsigned)((nc + 255) / 256), 1), dim3(256), 0, st, src[k], 0, dids + (size_t)k * nc, nc, r.count, r.nl,
                           r.nr, r.cap, r.roff);
}

// The driver of every ComputeBoW: the transform of the target's descriptors (k_frame_bow_transform[_fisheye]) and the FeatureVector
// (k_frame_featvec[_fisheye]) on m->stream.  Returns the first HIP error; nothing is synchronised.
hipError_t launch_compute_bow(orbx_matcher *m, const orbx_vocabulary *v, int levelsup, const BowTarget &t) {
    const int nc = t.feats();   // features the kernels may see
    int sort_cap = 1;
    while (sort_cap < nc) sort_cap <<= 1;
    const size_t lds = 8 * (size_t)sort_cap;
    if (lds > 64 * 1024) {
        const void *featvec = t.fisheye ? (const void *)k_frame_featvec_fisheye : (const void *)k_frame_featvec;
        const hipError_t e = hipFuncSetAttribute(featvec, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    FrameBow B;
    memset(&B, 0, sizeof(B));
    B.count = t.count; B.n_host = t.n; B.cap = t.cap; B.kps = t.kps; B.word = t.word; B.node = t.node;
    B.word_pos = v->word_pos; B.n_words = v->n_words;
    B.angle = t.angle; B.fv_node = t.fv_node; B.fv_ptr = t.fv_ptr; B.fv_index = t.fv_index; B.fv_meta = t.fv_meta;
    if (t.fisheye) {
        const int nl = t.nl, nr = t.nr, cap_l = t.roff, cap_r = t.cap - t.roff;   // the rows each camera may occupy
        const int side = t.n >= 0 ? std::max(nl, nr) : std::max(cap_l, cap_r);
        if (side > 0)
            hipLaunchKernelGGL(k_frame_bow_transform_fisheye, dim3((unsigned)((side + 15) / 16), 2), dim3(256), 0, m->stream, v->child_ptr, v->child_idx,
                               v->node_desc, v->word_id, v->L, levelsup, t.desc, t.count, nl, nr, cap_l, cap_r, t.roff, t.word, t.node);
        hipLaunchKernelGGL(k_frame_featvec_fisheye, dim3(1), dim3(1024), lds, m->stream, B, sort_cap, nl, nr, t.roff);
    } else {
        if (nc > 0)
            hipLaunchKernelGGL(k_frame_bow_transform, dim3((nc + 15) / 16), dim3(256), 0, m->stream, v->child_ptr, v->child_idx, v->node_desc, v->word_id,
                               v->L, levelsup, t.desc, t.count, t.n, t.cap, t.word, t.node);
        hipLaunchKernelGGL(k_frame_featvec, dim3(1), dim3(1024), lds, m->stream, B, sort_cap);
    }
    return hipGetLastError();
}

// ComputeBoW of a frame handle (either kind), and the tail of both forms: the ids of the features the kernels saw come down from src_word /
// src_node, with N while it is pending.
int frame_compute_bow(orbx_matcher *m, orbx_frame *f, const orbx_vocabulary *v, int levelsup) {
    f->bow_valid = false;
    ORBX_HIP(launch_compute_bow(m, v, levelsup, bow_target(f->view(), f->bow)));
    f->bow_valid = true; f->bow.voc = v; f->bow.levelsup = levelsup;
    return ORBX_OK;
}
int frame_bow_ids_down(orbx_frame *f, const int32_t *src_word, const int32_t *src_node, int32_t *word_id, int32_t *node_id) {
    const Rows ids[2] = {{src_word, 1, f->rows_n(), word_id, 0}, {src_node, 1, f->rows_n(), node_id, 0}};
    ORBX_TRY(frame_fetch(f, ids, 2));
    ORBX_TRY(f->owner->sync_and_deliver());
    frame_take(f, ids, 2);
    return ORBX_OK;
}

}  // namespace

// Frame::ComputeBoW (Frame.cc:738-745) on a resident frame: k_frame_bow_transform over the handle's descriptors, then k_frame_featvec builds the
// FeatureVector in the handle.  Nothing of the frame is uploaded; without downloads nothing waits (the launches are ordered on the owner's stream).
extern "C" int orbx_frame_compute_bow(orbx_matcher *m, orbx_frame *f, const orbx_vocabulary *v, int levelsup, int32_t *word_id, int32_t *node_id) {
    if (!m || !f || !v || f->owner != m || f->fisheye || v->device != m->device) return ORBX_E_BAD_ARG;   // (a fisheye frame: the _fisheye form)
    ORBX_HIP(hipSetDevice(m->device));
    const int nc = f->rows_n();   // features the kernels may see
    ORBX_TRY(m->reserve_staging(8 * (size_t)nc));   // the ids come down through it
    ORBX_TRY(frame_compute_bow(m, f, v, levelsup));
    if ((!word_id && !node_id) || nc == 0) return ORBX_OK;
    return frame_bow_ids_down(f, f->bow.word, f->bow.node, word_id, node_id);
}

// Frame::ComputeBoW of a resident fisheye-stereo frame (Frame.cc:738-745 over all N = N_left + N_right rows of mDescriptors): the handle's rows
// are transformed in place (k_frame_bow_transform_fisheye, the gap rows of a batch load skipped) and k_frame_featvec_fisheye builds the
// FeatureVector in row space.  The downloaded ids are renumbered into features [0, N) on the device (k_frame_rows_to_features): with N_left
// still on the device nothing waits for it.  Without downloads nothing waits at all.
extern "C" int orbx_frame_compute_bow_fisheye(orbx_matcher *m, orbx_frame *f, const orbx_vocabulary *v, int levelsup, int32_t *word_id,
                                              int32_t *node_id) {
    if (!m || !f || !v || f->owner != m || !f->fisheye || v->device != m->device) return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(m->device));
    const int nc = f->rows_n();   // features the kernels may see
    int32_t *dids;   // word ids, then node ids, in features [0, N)
    ORBX_TRY(m->carve([&](Carve &A) { dids = A.take<int32_t>(2 * (size_t)nc); }));
    ORBX_TRY(frame_compute_bow(m, f, v, levelsup));
    if ((!word_id && !node_id) || nc == 0) return ORBX_OK;
    launch_bow_ids_to_features(m->stream, f->view(), f->bow, nc, dids);
    ORBX_HIP(hipGetLastError());
    return frame_bow_ids_down(f, dids, dids + nc, word_id, node_id);
}

// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (ORBmatcher.cc:223-425) of the resident frame against n_kf key frames at once
// (Tracking::Relocalization, Tracking.cc:3670-3700; n_kf = 1: TrackReferenceKeyFrame): one upload run (the key frames and one BowProblem each),
// k_bow_pair_nodes, k_replay_bow_batch and k_replay_bow_finish_batch, one download run, one synchronisation -- whatever n_kf is.
// fisheye (orbx_frame_search_by_bow_fisheye): the frame side is the handle's ROW space -- k_replay_bow mode 3 with nb_left = roff (a row >= roff is
// the right camera's; rows ascend with the reference's feature indices, so every tie is the reference's), then k_frame_rows_to_features renumbers
// the rows into features [0, N) on the device.
static int frame_search_by_bow_impl(orbx_matcher *m, orbx_frame *f, int n_kf, const orbx_bow_keyframe *kfs, float nnratio, int check_orientation,
                                    int32_t *match, int match_stride, int32_t *nmatches, bool fisheye) {
    if (!m || !f || f->owner != m || f->fisheye != fisheye || !f->bow_valid || n_kf < 0) return ORBX_E_BAD_ARG;
    if (n_kf > ORBX_MAX_BOW_KEYFRAMES) return ORBX_E_TOO_LARGE;
    if (n_kf == 0) return ORBX_OK;
    if (!kfs || !match || !nmatches || match_stride < 0) return ORBX_E_BAD_ARG;
    size_t tot_nodes = 0;
    int max_nodes = 0;
    for (int k = 0; k < n_kf; k++) {   // every key frame is checked before anything is enqueued
        const orbx_bow_keyframe &K = kfs[k];
        const orbx_featvec &F = K.fv;
        if (K.n > 65535) return ORBX_E_TOO_LARGE;
        if (K.n < 0 || F.n_nodes < 0 || !F.node_ptr || (F.n_nodes > 0 && !F.node_id) || F.node_ptr[0] != 0) return ORBX_E_BAD_ARG;
        if (K.n > 0 && (!K.descriptors || (check_orientation && !K.angle))) return ORBX_E_BAD_ARG;
        for (int j = 0; j < F.n_nodes; j++)   // a CSR, node ids strictly ascending (std::map order: the pairing is a binary search)
            if (F.node_ptr[j + 1] < F.node_ptr[j] || (j > 0 && F.node_id[j] <= F.node_id[j - 1])) return ORBX_E_BAD_ARG;
        const int ni = F.node_ptr[F.n_nodes];
        if (ni > 0 && !F.index) return ORBX_E_BAD_ARG;
        for (int a = 0; a < ni; a++)
            if (F.index[a] < 0 || F.index[a] >= K.n) return ORBX_E_BAD_ARG;
        tot_nodes += (size_t)F.n_nodes;
        max_nodes = std::max(max_nodes, F.n_nodes);
    }
    int n = f->host_n();
    if (n < 0 && match_stride < f->cap) { const int rc = frame_count(f, &n); if (rc != ORBX_OK) return rc; }   // the rows must fit the stride
    if (n >= 0 && match_stride < n) return ORBX_E_BAD_ARG;
    const int nc = f->rows_n();   // features the device rows are sized for
    const int nrows = !fisheye ? nc : f->roff + f->rows_right();   // the replay's rows (fisheye: left, gap, right)
    for (int k = 0; k < n_kf; k++) {
        nmatches[k] = 0;
        for (int i = 0; i < std::max(n, 0); i++) match[(size_t)k * match_stride + i] = -1;
    }
    if (n == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(m->device));
    const int ne = std::max(nc, 1);
    size_t n_ent = (size_t)n_kf * ne;
    if (fisheye) {   // mode 3: 2 max(na, nb) entries per key frame (BowProblem::entries)
        n_ent = 0;
        for (int k = 0; k < n_kf; k++) n_ent += 2 * (size_t)std::max(std::max(kfs[k].n, nrows), 1);
    }
    std::vector<BowProblem> probs((size_t)n_kf);
    memset(probs.data(), 0, sizeof(BowProblem) * (size_t)n_kf);
    uint32_t *dkn;
    BowProblem *dP;
    int32_t *dpair, *dmatch, *dout, *dnm, *dhist, *dent;
    std::vector<uint8_t *> dskip((size_t)n_kf, nullptr);
    ORBX_TRY(m->carve([&](Carve &A) {
        // the uploads, side by side: per key frame its rows and feature vector, then every node id of the batch, then the problem records
        for (int k = 0; k < n_kf; k++) {
            const orbx_bow_keyframe &K = kfs[k];
            const int nn = K.fv.n_nodes, ni = K.fv.node_ptr[nn];
            BowProblem &P = probs[k];
            P.desc_a = A.up(K.descriptors, 32 * (size_t)K.n);
            if (K.angle && check_orientation) P.angle_a = A.up(K.angle, (size_t)K.n);
            if (K.valid) P.skip_a = dskip[k] = A.take<uint8_t>(K.n);   // (uploaded below, inverted)
            P.fa.node_ptr = A.up(K.fv.node_ptr, (size_t)nn + 1); P.fa.index = A.up(K.fv.index, (size_t)ni, 1); P.fa.n_nodes = nn;
            P.na = K.n;
        }
        dkn = A.take<uint32_t>(tot_nodes + 1);
        dP = A.take<BowProblem>(n_kf);
        // device-only: the pairing, the rows (filled with -1) and match counts side by side (one download run), histograms + counters (zeroed), entries
        dpair = A.take<int32_t>(tot_nodes + 1);
        dmatch = A.take<int32_t>((size_t)n_kf * nrows);
        dout = fisheye ? A.take<int32_t>((size_t)n_kf * nc) : dmatch;   // fisheye: the rows renumbered into features, next to the counts
        dnm = A.take<int32_t>(n_kf);
        dhist = A.take<int32_t>((size_t)n_kf * (ORBX_HISTO_LENGTH + 2));
        dent = A.take<int32_t>(n_ent);
    }));
    {
        std::vector<uint8_t> skip;
        size_t o = 0;
        for (int k = 0; k < n_kf; k++) {
            const orbx_bow_keyframe &K = kfs[k];
            if (K.valid) {
                skip.resize((size_t)K.n);
                for (int i = 0; i < K.n; i++) skip[i] = K.valid[i] ? 0 : 1;
                ORBX_TRY(m->h2d(dskip[k], skip.data(), (size_t)K.n));
            }
            ORBX_TRY(m->h2d(dkn + o, K.fv.node_id, 4 * (size_t)K.fv.n_nodes));
            probs[k].fa.node_id = dkn + o;
            o += (size_t)K.fv.n_nodes;
        }
    }
    {
        size_t o = 0, oe = 0;
        for (int k = 0; k < n_kf; k++) {
            BowProblem &P = probs[k];
            P.mode = fisheye ? 3 : 0; P.nb_left = fisheye ? f->roff : 0;
            P.fb.node_id = f->bow.fv_node; P.fb.node_ptr = f->bow.fv_ptr; P.fb.index = f->bow.fv_index; P.fb.n_nodes = 0;   // (the frame's node count stays on the device)
            P.desc_b = f->desc; P.angle_b = f->bow.angle; P.nb = nrows;
            P.nnratio = nnratio; P.check_orientation = check_orientation ? 1 : 0;
            P.match = dmatch + (size_t)k * nrows; P.nmatches = dnm + k;
            P.hist = dhist + (size_t)k * (ORBX_HISTO_LENGTH + 2); P.counters = P.hist + ORBX_HISTO_LENGTH;
            P.entries = dent + oe;
            oe += fisheye ? 2 * (size_t)std::max(std::max(kfs[k].n, nrows), 1) : (size_t)ne;
            P.pair_b = dpair + o;
            o += (size_t)P.fa.n_nodes;
        }
    }
    ORBX_TRY(m->h2d(dP, probs.data(), sizeof(BowProblem) * (size_t)n_kf));
    ORBX_HIP(m->fill(dmatch, 0xff, 4 * (size_t)n_kf * nrows));
    ORBX_HIP(m->fill(dhist, 0, 4 * (size_t)n_kf * (ORBX_HISTO_LENGTH + 2)));
    if (tot_nodes > 0) {
        hipLaunchKernelGGL(k_bow_pair_nodes, dim3((unsigned)((tot_nodes + 255) / 256)), dim3(256), 0, m->exec(), dkn, (int)tot_nodes, f->bow.fv_node,
                           f->bow.fv_meta, dpair);
        hipLaunchKernelGGL(k_replay_bow_batch, dim3((unsigned)((max_nodes + 3) / 4), (unsigned)n_kf), dim3(256), 0, m->exec(), (const BowProblem *)dP);
    }
    hipLaunchKernelGGL(k_replay_bow_finish_batch, dim3((unsigned)n_kf), dim3(64), 0, m->exec(), (const BowProblem *)dP);
    if (fisheye)
        hipLaunchKernelGGL(k_frame_rows_to_features, dim3((unsigned)((nc + 255) / 256), (unsigned)n_kf), dim3(256), 0, m->exec(), dmatch, nrows, dout, nc,
                           f->count, f->host_left(), f->host_right(), f->cap, f->roff);
    ORBX_HIP(hipGetLastError());
    const Rows rows = {dout, n_kf, nc, match, (size_t)match_stride};
    ORBX_TRY(frame_fetch(f, &rows, 1));
    ORBX_TRY(m->d2h(nmatches, dnm, 4 * (size_t)n_kf));
    ORBX_TRY(m->sync_and_deliver());
    frame_take(f, &rows, 1);
    return ORBX_OK;
}

extern "C" int orbx_frame_search_by_bow(orbx_matcher *m, orbx_frame *f, int n_kf, const orbx_bow_keyframe *kfs, float nnratio, int check_orientation,
                                        int32_t *match, int match_stride, int32_t *nmatches) {
    return frame_search_by_bow_impl(m, f, n_kf, kfs, nnratio, check_orientation, match, match_stride, nmatches, false);
}

// SearchByBoW(KeyFrame*, Frame&) of a resident fisheye-stereo frame (F.Nleft != -1, ORBmatcher.cc:283-392) against n_kf key frames: row k equals
// orbx_search_by_bow_frame_fisheye for key frame k.  The same cost shape as orbx_frame_search_by_bow (one more launch: the renumbering).
extern "C" int orbx_frame_search_by_bow_fisheye(orbx_matcher *m, orbx_frame *f, int n_kf, const orbx_bow_keyframe *kfs, float nnratio,
                                                int check_orientation, int32_t *match, int match_stride, int32_t *nmatches) {
    return frame_search_by_bow_impl(m, f, n_kf, kfs, nnratio, check_orientation, match, match_stride, nmatches, true);
}

// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:329-403) for a batch of map points
extern "C" int orbx_distinctive_descriptors(orbx_matcher *m, const uint8_t *desc, const int32_t *set_ptr, int n_sets, int32_t *best_idx) {
    if (!m || n_sets < 0 || (n_sets > 0 && (!set_ptr || !best_idx))) return ORBX_E_BAD_ARG;
    if (n_sets == 0) return ORBX_OK;
    const int total = set_ptr[n_sets];
    if (total > 0 && !desc) return ORBX_E_BAD_ARG;
    ORBX_HIP(hipSetDevice(m->device));
    uint8_t *dd;
    int32_t *dp, *db;
    ORBX_TRY(m->carve([&](Carve &A) { dd = A.up(desc, 32 * (size_t)total, 32); dp = A.up(set_ptr, (size_t)n_sets + 1); db = A.take<int32_t>(n_sets); }));
    hipLaunchKernelGGL(k_distinctive, dim3((n_sets + 3) / 4), dim3(256), 0, m->exec(), dd, dp, n_sets, db);
    ORBX_TRY(m->d2h(best_idx, db, 4 * (size_t)n_sets));
    ORBX_TRY(m->sync_and_deliver());
    return ORBX_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Candidate loop of ORBmatcher::Fuse x2 (ORBmatcher.cc:1246-1306, 1405-1433): queries do not interact, so the device
// returns the best feature per projected map point; the Replace / AddObservation logic stays in the adapter.
// ---------------------------------------------------------------------------------------------------------
extern "C" int orbx_fuse_search(orbx_matcher *m, const orbx_frame_desc *kf, const float *inv_level_sigma2, int n_q, const float *q_u,
                                const float *q_v, const float *q_ur, const float *q_r, const int32_t *q_level, const uint8_t *q_desc,
                                int strict_fp, int32_t *best_idx, int32_t *best_dist) {
    if (!m || !kf || n_q < 0 || (n_q > 0 && (!q_u || !q_v || !q_r || !q_level || !q_desc || !best_idx || !best_dist))) return ORBX_E_BAD_ARG;
    for (int i = 0; i < n_q; i++) { best_idx[i] = -1; best_dist[i] = 256; }
    const int n = kf->n;
    if (n == 0 || n_q == 0) return ORBX_OK;
    if (n > 65535) return ORBX_E_TOO_LARGE;
    ORBX_HIP(hipSetDevice(m->device));
    const int nl = kf->nlevels;
    WindowProblem P;
    memset(&P, 0, sizeof(P));
    P.chi2_fma = strict_fp ? 0 : 1;
    std::vector<int32_t> qmin(n_q), qmax(n_q);
    for (int i = 0; i < n_q; i++) { qmin[i] = q_level[i] - 1; qmax[i] = q_level[i]; }  // kpLevel<nPredictedLevel-1 || kpLevel>nPredictedLevel
    const int32_t cnts[2] = {n, n_q};
    int32_t *dcnt;
    WindowProblem *dP;
    ORBX_TRY(m->carve([&](Carve &A) {
        P.kps = A.up(kf->keypoints_un, (size_t)n); P.desc = A.up(kf->descriptors, 32 * (size_t)n);
        dcnt = A.up(cnts, 2, 2);
        P.u_right = A.up_opt(kf->u_right, (size_t)n);
        P.inv_sigma2 = A.up_opt(inv_level_sigma2, (size_t)nl);
        P.qx = A.up(q_u, (size_t)n_q); P.qy = A.up(q_v, (size_t)n_q); P.qr = A.up(q_r, (size_t)n_q);
        P.qmin = A.up(qmin.data(), (size_t)n_q); P.qmax = A.up(qmax.data(), (size_t)n_q);
        if (kf->u_right) P.qxr = A.up_opt(q_ur, (size_t)n_q);
        P.qdesc = A.up(q_desc, 32 * (size_t)n_q);
        dP = A.take<WindowProblem>(1);   // directly behind the inputs: the call's uploads are one run of the arena (one DMA)
        P.keys = A.take<u64>((size_t)n_q * kTopK); P.meta = A.take<int32_t>(n_q);
        P.gstart = A.take<uint16_t>(kGridCells + 1); P.gorder = A.take<uint16_t>(n);
    }));
    P.n_ptr = dcnt; P.nq_ptr = dcnt + 1;
    const bool brute = m->brute_windows && (size_t)n_q * (size_t)n <= kBruteMaxPairs;
    if (brute) { P.gstart = nullptr; P.gorder = nullptr; }
    ORBX_TRY(m->h2d(dP, &P, sizeof(P)));
    const float fb[4] = {kf->min_x, kf->max_x, kf->min_y, kf->max_y};
    const GridParams g = grid_of(fb);
    if (brute) {
        hipLaunchKernelGGL(k_window_brute, dim3((n_q + 3) / 4), dim3(256), 0, m->exec(), dP, g);
    } else {
        ORBX_LAUNCH_GRID_BUILD( dim3(1), dim3(64), 0, m->exec(), dP, g);
        ORBX_LAUNCH_WINDOW_BEST2(n_q, 1, m->exec(), dP, g);
    }
    std::vector<u64> keys((size_t)n_q * kTopK);
    ORBX_TRY(m->d2h(keys.data(), P.keys, 8 * (size_t)n_q * kTopK));
    ORBX_TRY(m->sync_and_deliver());
    for (int i = 0; i < n_q; i++) {
        const u64 k = keys[(size_t)i * kTopK];
        if (k != kNoKey) { best_idx[i] = (int32_t)(k & 0xffff); best_dist[i] = (int32_t)(k >> 32); }
    }
    return ORBX_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Device-resident key frames (include/orbx.h, orbx_keyframe): what KeyFrame::KeyFrame(Frame&) copies of the frame -- immutable from then on, in ONE
// allocation of its own, readable by every matcher context of its device -- and ORBmatcher::Fuse for K of them in one call.  Two kinds, monocular /
// rectified and fisheye-stereo (KeyFrame::NLeft != -1), with ONE path each for what they share, the kind being a `bool fisheye` of that path:
//   construction   keyframe_create_host / keyframe_from_frame (the four public constructors are argument checks), one tail: keyframe_publish
//   pending counts orbx_keyframe::host_n / rows_n / adopt -- orbx_keyframe_count, both Fuse drivers and the BoW calls learn N through adopt()
//   Fuse           keyframe_fuse_search_impl (projected queries) and keyframe_fuse_map_points_impl (projection on the device: SearchInNeighbors'
//                  loop, on a rig both Fuse calls per target), with one decode of the keys: keyframe_fuse_results
//                  (sim3: LoopClosing::SearchAndFuse's Fuse through the same driver; LoopClosing's Sim3 SearchByProjection further down)
// ---------------------------------------------------------------------------------------------------------
// The BoW state of a key frame (orbx_keyframe_compute_bow / orbx_keyframe_bow_from_frame): a SECOND allocation, made when BoW is first attached -- key
// frames without it keep their size.  Set once, immutable afterwards; guarded as the rows are (an event behind its creation, a done flag).
struct KeyFrameBow : BowArrays {
    uint8_t *dev = nullptr;            // one allocation, the arrays carved from it
    hipEvent_t ready = nullptr;
    std::atomic<bool> done{false};
};

struct orbx_keyframe {
    int device = 0;
    uint8_t *dev = nullptr;            // one allocation, carved below
    orbx_keypoint *kps = nullptr;
    uint8_t *desc = nullptr;
    float *u_right = nullptr;          // NULL: no mvuRight
    float *depth = nullptr, *keys_xy = nullptr;   // mvDepth [cap], mvKeys[i].pt [cap][2]; NULL: none (made without depth)
    float *inv_sigma2 = nullptr;       // NULL: no mvInvLevelSigma2 given
    float *scale = nullptr;
    int32_t *count = nullptr;
    uint16_t *gstart = nullptr, *gorder = nullptr;
    hipEvent_t ready = nullptr;        // recorded behind the copy / upload + grid build on the creating context's stream
    std::atomic<bool> done{false};     // a call that waited for `ready` has synchronised since: nobody needs to wait again
    std::atomic<int> n{-1};            // N; -1 while it is known on the device only (made from a batch-loaded frame)
    int cap = 0, nlevels = 0;
    float bounds[4] = {0, 0, 0, 0};
    std::atomic<KeyFrameBow *> bow{nullptr};   // NULL: no BoW attached (yet)
    const orbx_frame *src_frame = nullptr;     // orbx_keyframe_from_frame: the handle and its load counter at the copy
    uint64_t src_seq = 0;
    // A fisheye-stereo key frame (KeyFrame::NLeft != -1; orbx_keyframe_from_frame_fisheye / orbx_keyframe_create_host_fisheye): kps = mvKeys at rows
    // [0, N_left) and mvKeysRight at rows [roff, roff + N_right) -- roff is known on the host before the counts are; desc = mDescriptors with the
    // right camera's rows at roff as well; count[0] / count[1] = N_left / N_right; a grid per camera with side-local indices (gorder_r = gorder + roff).
    // n = N_left + N_right.  No mvuRight; mvLeftToRightMatch / mvRightToLeftMatch are not kept (Fuse does not read them).
    bool fisheye = false;
    int roff = 0;
    uint16_t *gstart_r = nullptr, *gorder_r = nullptr;
    std::atomic<int> n_left{-1}, n_right{-1};  // -1 while known on the device only (cached with n)

    // N as the host sees it, as orbx_frame's members of these names.  A key frame made from a batch-loaded handle leaves the count(s) on the device
    // until a call needs them: host_*() = the count, or -1 for "not yet"; rows_n() = N, or meanwhile the capacity a call's per-feature buffers are
    // sized by.
    int host_n() const { return n.load(); }
    int host_left() const { return n_left.load(); }
    int host_right() const { return n_right.load(); }
    int rows_n() const { const int v = n.load(); return v >= 0 ? v : cap; }
    HandleRows view() const { return HandleRows{desc, kps, count, cap, n.load(), fisheye, roff, n_left.load(), n_right.load()}; }
    // The one place that learns the counts: a constructor with what the host knows, or a call that met the key frame with its counts pending and
    // brought count[0] (, count[1]) home with its results.  Clamped as k_keyframe_copy / k_keyframe_copy_fisheye clamp what they write, so a device
    // count comes through unchanged.
    void adopt(int c0, int c1 = 0) {
        if (fisheye) {
            const int nl = std::min(std::max(c0, 0), roff), nr = std::min(std::max(c1, 0), cap - roff);
            n_left.store(nl); n_right.store(nr); n.store(nl + nr);
        } else {
            n.store(std::min(std::max(c0, 0), cap));
        }
    }
};

namespace {

// A key frame under construction: destroyed on every way out but the one that releases it to the caller.
struct KeyFrameDelete { void operator()(orbx_keyframe *kf) const { orbx_keyframe_destroy(kf); } };
typedef std::unique_ptr<orbx_keyframe, KeyFrameDelete> KeyFramePtr;

void keyframe_bow_free(KeyFrameBow *b) {
    if (!b) return;
    if (b->ready) { (void)hipEventSynchronize(b->ready); (void)hipEventDestroy(b->ready); }
    if (b->dev) (void)hipFree(b->dev);
    delete b;
}

// one allocation per key frame: rows for `cap` features (28 + 32 [+ 4] + 2 bytes each), the per-level arrays, the count and the grid's 3073 cell offsets
// (roff >= 0: a fisheye-stereo key frame -- cap = roff + the right camera's rows, a second set of cell offsets; roff < 0: a monocular one)
int keyframe_alloc(int device, int cap, int roff, bool has_ur, bool has_sigma, int nlevels, const float *bounds4, KeyFramePtr &out, bool has_depth = false) {
    out.reset(new orbx_keyframe());
    orbx_keyframe *kf = out.get();
    kf->device = device; kf->cap = cap; kf->nlevels = nlevels;
    kf->fisheye = roff >= 0; kf->roff = std::max(roff, 0);
    memcpy(kf->bounds, bounds4, sizeof(kf->bounds));
    const size_t c = (size_t)std::max(cap, 1);
    Layout L;
    // (rows and inv_sigma2 first: keyframe_create_host uploads them as one run)
    const size_t off_kps = L.add(28 * c), off_desc = L.add(32 * c), off_ur = has_ur ? L.add(4 * c) : 0, off_sg = has_sigma ? L.add(4 * (size_t)kFrameMaxLevels) : 0;
    const size_t off_scale = L.add(4 * (size_t)kFrameMaxLevels), off_count = L.add(8), off_gs = L.add(2 * ((size_t)kGridCells + 1)), off_go = L.add(2 * c);
    const size_t off_gsr = kf->fisheye ? L.add(2 * ((size_t)kGridCells + 1)) : 0;
    // (behind everything else: a key frame without depth has the size and the layout it had)
    const size_t off_dep = has_depth ? L.add(4 * c) : 0, off_xy = has_depth ? L.add(8 * c) : 0;
    hipError_t e = hipMalloc((void **)&kf->dev, L.used);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&kf->ready, hipEventDisableTiming);
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); return ORBX_E_HIP; }
    kf->kps = (orbx_keypoint *)(kf->dev + off_kps); kf->desc = kf->dev + off_desc;
    kf->u_right = has_ur ? (float *)(kf->dev + off_ur) : nullptr;
    kf->inv_sigma2 = has_sigma ? (float *)(kf->dev + off_sg) : nullptr;
    kf->scale = (float *)(kf->dev + off_scale); kf->count = (int32_t *)(kf->dev + off_count);
    kf->gstart = (uint16_t *)(kf->dev + off_gs); kf->gorder = (uint16_t *)(kf->dev + off_go);
    if (kf->fisheye) { kf->gstart_r = (uint16_t *)(kf->dev + off_gsr); kf->gorder_r = kf->gorder + kf->roff; }
    if (has_depth) { kf->depth = (float *)(kf->dev + off_dep); kf->keys_xy = (float *)(kf->dev + off_xy); }
    return ORBX_OK;
}

// the calling context's stream is ordered behind the key frame's creation (until a call that did so has synchronised)
inline int keyframe_acquire(orbx_matcher *m, orbx_keyframe *const *kfs, int n_kf) {
    for (int k = 0; k < n_kf; k++)
        if (!kfs[k]->done.load(std::memory_order_acquire)) ORBX_HIP(hipStreamWaitEvent(m->stream, kfs[k]->ready, 0));
    return ORBX_OK;
}
int keyframe_wait_ready(orbx_matcher *m, orbx_keyframe *kf) { return keyframe_acquire(m, &kf, 1); }
inline void keyframe_release(orbx_keyframe *const *kfs, int n_kf) {   // after the call's synchronisation
    for (int k = 0; k < n_kf; k++) kfs[k]->done.store(true, std::memory_order_release);
}

// the key-frame side of a problem; right: the right camera of a fisheye-stereo key frame (mvKeysRight, its grid, descriptor rows [N_left, N))
inline void keyframe_problem(const orbx_keyframe *kf, bool chi2, int strict_fp, KfProblem *R, bool right = false) {
    memset(R, 0, sizeof(*R));
    const size_t ro = right ? (size_t)kf->roff : 0;
    R->P.kps = kf->kps + ro; R->P.desc = kf->desc + 32 * ro; R->P.n_ptr = kf->count + (right ? 1 : 0);
    R->P.u_right = chi2 ? kf->u_right : nullptr;   // the gate-less form (Fuse with a Sim3, SearchBySim3) never reads mvuRight (ORBmatcher.cc:1405-1433)
    R->P.scale = kf->scale;
    R->P.inv_sigma2 = chi2 ? kf->inv_sigma2 : nullptr;
    R->P.chi2_fma = strict_fp ? 0 : 1;
    R->P.gstart = right ? kf->gstart_r : kf->gstart; R->P.gorder = right ? kf->gorder_r : kf->gorder;
    R->g = grid_of(kf->bounds);
    R->maxx = kf->bounds[1]; R->maxy = kf->bounds[3];
    R->nlevels = kf->nlevels;
}

// Fisheye key frames whose counts are still on the device (made from a batch-loaded handle): a search brings them home among its downloads and adopts
// them behind its synchronisation -- no synchronisation of their own.  pend: [n_kf][2] landing slots (sized before the first download is recorded).
inline int keyframe_fetch_counts(orbx_matcher *m, bool fisheye, int n_kf, orbx_keyframe *const *kfs, std::vector<int32_t> *pend) {
    if (!fisheye) return ORBX_OK;
    pend->assign(2 * (size_t)n_kf, 0);
    for (int k = 0; k < n_kf; k++)
        if (kfs[k]->host_n() < 0) ORBX_TRY(m->d2h(pend->data() + 2 * (size_t)k, kfs[k]->count, 8));
    return ORBX_OK;
}
inline void keyframe_take_counts(bool fisheye, int n_kf, orbx_keyframe *const *kfs, const std::vector<int32_t> &pend) {
    for (int k = 0; fisheye && k < n_kf; k++)
        if (kfs[k]->host_n() < 0) kfs[k]->adopt(pend[2 * (size_t)k], pend[2 * (size_t)k + 1]);
}

inline void launch_window_best1_kf(hipStream_t st, const KfProblem *dR, int nq_max, int np) {   // ORBX_LAUNCH_WINDOW_BEST2's shape: a problem's blocks on one XCD
    const int nb = (nq_max + 31) / 32;
    const dim3 grid = np >= 8 ? dim3(8, (unsigned)nb, (unsigned)((np + 7) / 8)) : dim3(1, (unsigned)nb, (unsigned)np);
    hipLaunchKernelGGL(k_window_best1_kf, grid, dim3(256), 0, st, dR, np);
}

// The n results of problem p (key frame p / sides, camera p % sides) as the caller gets them: -1 / 256 where nothing qualified; a right-camera index in
// the rig's numbering, N_left + j (ORBmatcher.cc:1296) -- behind keyframe_take_counts, so N_left is at home.
inline void keyframe_fuse_results(orbx_keyframe *const *kfs, int sides, int p, const u64 *keys, size_t n, int32_t *best_idx, int32_t *best_dist) {
    const int base = p % sides == 1 ? kfs[p / sides]->host_left() : 0;
    for (size_t i = 0; i < n; i++) {
        best_idx[i] = keys[i] == kNoKey ? -1 : base + (int32_t)(keys[i] & 0xffff);
        best_dist[i] = keys[i] == kNoKey ? 256 : (int32_t)(keys[i] >> 32);
    }
}

// ---- Construction.  Both kinds of key frame are made by the same two functions -- from host arrays, from a frame handle -- with the kind as data;
// they differ in the kernel launched.  A constructor holds the key frame in a KeyFramePtr, and keyframe_publish() is the one way it reaches the caller.

// The tail behind a constructor's launch: the launch's error, the `ready` event, the counts the host knows (c0 < 0: still on the device only), *out.
int keyframe_publish(orbx_matcher *m, KeyFramePtr &kf, int c0, int c1, orbx_keyframe **out) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(kf->ready, m->stream);
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); return ORBX_E_HIP; }
    if (c0 >= 0) kf->adopt(c0, c1);
    *out = kf.release();
    return ORBX_OK;
}

// From host arrays (arguments checked by the caller).  d: mvKeysUn / mDescriptors [d->n] and the optional mvuRight of a monocular key frame; of a rig
// mvKeys [d->n = N_left] and ALL N descriptor rows, with kps_right [n_right] = mvKeysRight (monocular: NULL, 0).
int keyframe_create_host(orbx_matcher *m, bool fisheye, const orbx_frame_desc *d, const orbx_keypoint *kps_right, int n_right,
                         const float *inv_level_sigma2, orbx_keyframe **out, const float *depth = nullptr, const float *keys_xy = nullptr) {
    ORBX_HIP(hipSetDevice(m->device));
    const int nl = d->n, nr = n_right, N = nl + nr, nlv = d->nlevels;
    const float *ur = fisheye ? nullptr : d->u_right;
    const float b[4] = {d->min_x, d->max_x, d->min_y, d->max_y};
    KeyFramePtr kf;
    ORBX_TRY(keyframe_alloc(m->device, N, fisheye ? nl : -1, ur != nullptr, inv_level_sigma2 != nullptr, nlv, b, kf, depth != nullptr));
    // ONE upload: the rows -- a rig's mvKeysRight right behind its mvKeys (roff = N_left) -- mvuRight and inv_sigma2, staged at the allocation's own
    // offsets (pinned; the context's next call waits before it stages over them)
    const size_t up_end = (size_t)((inv_level_sigma2 ? (uint8_t *)(kf->inv_sigma2 + nlv) : ur ? (uint8_t *)(kf->u_right + N) : kf->desc + 32 * (size_t)N) - kf->dev);
    // (with depth: a second range of the same upload, mvDepth and the raw (x, y) rows side by side at the allocation's end)
    const size_t o_dep = depth ? (size_t)((uint8_t *)kf->depth - kf->dev) : 0, dep_end = depth ? (size_t)((uint8_t *)(kf->keys_xy + 2 * (size_t)N) - kf->dev) : 0;
    const size_t st_bytes = std::max(up_end, dep_end);
    ORBX_TRY(m->reserve_staging(st_bytes));   // the rows go up through it
    if (N > 0 || inv_level_sigma2) {
        uint8_t *st = static_cast<uint8_t *>(m->stage.take(st_bytes + 16));
        if (!st) { set_error("staging arena exhausted"); return ORBX_E_INTERNAL; }
        memset(st, 0, st_bytes + 16);
        const size_t o_kps = (size_t)((uint8_t *)kf->kps - kf->dev);
        if (nl) memcpy(st + o_kps, d->keypoints_un, 28 * (size_t)nl);
        if (nr) memcpy(st + o_kps + 28 * (size_t)nl, kps_right, 28 * (size_t)nr);
        if (N) memcpy(st + (kf->desc - kf->dev), d->descriptors, 32 * (size_t)N);
        if (ur) memcpy(st + ((uint8_t *)kf->u_right - kf->dev), ur, 4 * (size_t)N);
        if (inv_level_sigma2) memcpy(st + ((uint8_t *)kf->inv_sigma2 - kf->dev), inv_level_sigma2, 4 * (size_t)nlv);
        if (depth && N) {
            memcpy(st + o_dep, depth, 4 * (size_t)N);
            float *xy = reinterpret_cast<float *>(st + ((uint8_t *)kf->keys_xy - kf->dev));
            if (keys_xy) memcpy(xy, keys_xy, 8 * (size_t)N);
            else for (int i = 0; i < N; i++) { xy[2 * i] = d->keypoints_un[i].x; xy[2 * i + 1] = d->keypoints_un[i].y; }
        }
        m->dirty = true;
        const orbx_matcher::Span run[2] = {{0, up_end}, {o_dep, depth && N ? dep_end - o_dep : 0}};
        ORBX_TRY(m->upload_ranges(kf->dev, st, run, 2));
    }
    // the in-place form of the frame loaders' kernels: count(s), scale factors, grid_build_wave over the uploaded rows (a grid per camera)
    m->dirty = true;
    if (fisheye) {
        FisheyePrepare P;
        prepare_dst(P, kf.get(), nl, d->scale_factors, nlv);
        P.n_host[0] = nl; P.n_host[1] = nr; P.cap_side[0] = nl; P.cap_side[1] = nr;
        hipLaunchKernelGGL(k_frame_prepare_fisheye, dim3(2), dim3(64), 0, m->stream, P, grid_of(kf->bounds));
    } else {
        FramePrepare P;
        prepare_dst(P, kf.get(), 0, d->scale_factors, nlv);
        P.n_host = N; P.cap = N;
        hipLaunchKernelGGL(k_frame_prepare, dim3(1), dim3(64), 0, m->stream, P, grid_of(kf->bounds));
    }
    return keyframe_publish(m, kf, nl, nr, out);
}

// From a loaded frame handle of the same kind, owned by m (checked by the caller): a device-to-device copy on the owner's stream -- behind the frame's
// load, ahead of its next one, no host synchronisation.  Sized by the counts where the host knows them, else by the handle's capacities.
int keyframe_from_frame(orbx_matcher *m, bool fisheye, orbx_frame *f, const float *inv_level_sigma2, orbx_keyframe **out) {
    ORBX_HIP(hipSetDevice(m->device));
    const int cap_l = fisheye ? f->rows_left() : f->rows_n(), cap_r = fisheye ? f->rows_right() : 0;
    KeyFramePtr kf;
    const bool with_depth = !fisheye && f->has_depth;
    ORBX_TRY(keyframe_alloc(m->device, cap_l + cap_r, fisheye ? cap_l : -1, f->has_ur, inv_level_sigma2 != nullptr, f->nlevels, f->bounds, kf, with_depth));
    m->dirty = true;
    if (fisheye) {
        KeyFrameCopyFisheye C;
        memset(&C, 0, sizeof(C));
        C.src_kps = f->kps; C.src_desc = f->desc; C.src_count = f->count; C.src_scale = f->scale;
        C.src_gstart_l = f->gstart; C.src_gorder_l = f->gorder; C.src_gstart_r = f->gstart_r; C.src_gorder_r = f->gorder_r;
        C.kps = kf->kps; C.desc = kf->desc; C.count = kf->count; C.scale = kf->scale; C.inv_sigma2 = kf->inv_sigma2;
        C.gstart_l = kf->gstart; C.gorder_l = kf->gorder; C.gstart_r = kf->gstart_r; C.gorder_r = kf->gorder_r;
        C.src_roff = f->roff; C.roff = cap_l; C.cap_l = cap_l; C.cap_r = cap_r; C.nlevels = f->nlevels;
        if (inv_level_sigma2) memcpy(C.inv_sigma2_host, inv_level_sigma2, sizeof(float) * (size_t)f->nlevels);
        hipLaunchKernelGGL(k_keyframe_copy_fisheye, dim3(2 + (unsigned)((std::max(cap_l, cap_r) + 255) / 256)), dim3(64), 0, m->stream, C);
    } else {
        KeyFrameCopy C;
        memset(&C, 0, sizeof(C));
        C.src_kps = f->kps; C.src_desc = f->desc; C.src_ur = f->has_ur ? f->u_right : nullptr; C.src_count = f->count; C.src_scale = f->scale;
        C.src_gstart = f->gstart; C.src_gorder = f->gorder;
        C.kps = kf->kps; C.desc = kf->desc; C.ur = kf->u_right; C.count = kf->count; C.scale = kf->scale; C.inv_sigma2 = kf->inv_sigma2;
        C.gstart = kf->gstart; C.gorder = kf->gorder; C.cap = cap_l; C.nlevels = f->nlevels;
        if (inv_level_sigma2) memcpy(C.inv_sigma2_host, inv_level_sigma2, sizeof(float) * (size_t)f->nlevels);
        hipLaunchKernelGGL(k_keyframe_copy, dim3(1 + (unsigned)((cap_l + 255) / 256)), dim3(64), 0, m->stream, C);
        // a handle with depth: mvDepth and the raw (x, y) rows follow in a launch of their own (k_keyframe_copy and its record stay what they were)
        if (with_depth && cap_l > 0)   // (an empty frame: nothing to copy, and a grid of no blocks is no launch)
            hipLaunchKernelGGL(k_keyframe_copy_depth, dim3((unsigned)((cap_l + 255) / 256)), dim3(256), 0, m->stream, (const int32_t *)f->count, cap_l,
                               (const float *)f->depth, (const float *)f->keys_xy, kf->depth, kf->keys_xy);
    }
    kf->src_frame = f; kf->src_seq = f->load_seq;
    return keyframe_publish(m, kf, fisheye ? f->host_left() : f->host_n(), f->host_right(), out);
}

}  // namespace

extern "C" {

void orbx_keyframe_destroy(orbx_keyframe *kf) {
    if (!kf) return;
    (void)hipSetDevice(kf->device);
    if (kf->ready) { (void)hipEventSynchronize(kf->ready); (void)hipEventDestroy(kf->ready); }   // the copy / upload has run; no search is running (the caller's contract)
    keyframe_bow_free(kf->bow.load());
    if (kf->dev) (void)hipFree(kf->dev);
    delete kf;
}

int orbx_keyframe_create_host(orbx_matcher *m, const orbx_frame_desc *d, const float *inv_level_sigma2, orbx_keyframe **out) {
    if (out) *out = nullptr;
    if (!m || !out || !d || d->n < 0 || (d->n > 0 && (!d->keypoints_un || !d->descriptors)) || !d->scale_factors || d->nlevels < 1 ||
        d->nlevels > kFrameMaxLevels)
        return ORBX_E_BAD_ARG;
    if (d->n > 65535) return ORBX_E_TOO_LARGE;   // 16-bit grid entries, as orbx_fuse_search
    return keyframe_create_host(m, false, d, nullptr, 0, inv_level_sigma2, out);
}

int orbx_keyframe_create_host_stereo(orbx_matcher *m, const orbx_frame_desc *d, const float *depth, const float *keys_xy, const float *inv_level_sigma2,
                                     orbx_keyframe **out) {
    if (out) *out = nullptr;
    if (!m || !out || !d || d->n < 0 || (d->n > 0 && (!d->keypoints_un || !d->descriptors)) || !d->scale_factors || d->nlevels < 1 ||
        d->nlevels > kFrameMaxLevels || !d->u_right || !depth)
        return ORBX_E_BAD_ARG;
    if (d->n > 65535) return ORBX_E_TOO_LARGE;   // 16-bit grid entries, as orbx_fuse_search
    return keyframe_create_host(m, false, d, nullptr, 0, inv_level_sigma2, out, depth, keys_xy);
}

int orbx_keyframe_create_host_fisheye(orbx_matcher *m, const orbx_frame_desc *left, const orbx_keypoint *kps_right, int n_right,
                                      const float *inv_level_sigma2, orbx_keyframe **out) {
    if (out) *out = nullptr;
    if (!m || !out || !left || left->n < 0 || n_right < 0 || (left->n > 0 && !left->keypoints_un) || (n_right > 0 && !kps_right) ||
        (left->n + n_right > 0 && !left->descriptors) || !left->scale_factors || left->nlevels < 1 || left->nlevels > kFrameMaxLevels)
        return ORBX_E_BAD_ARG;
    if ((int64_t)left->n + n_right > 65535) return ORBX_E_TOO_LARGE;   // 16-bit grid entries, as orbx_fuse_search
    return keyframe_create_host(m, true, left, kps_right, n_right, inv_level_sigma2, out);
}

int orbx_keyframe_from_frame(orbx_matcher *m, orbx_frame *f, const float *inv_level_sigma2, orbx_keyframe **out) {
    if (out) *out = nullptr;
    if (!m || !out || !f || f->owner != m || !f->loaded || f->fisheye) return ORBX_E_BAD_ARG;
    return keyframe_from_frame(m, false, f, inv_level_sigma2, out);
}

int orbx_keyframe_from_frame_fisheye(orbx_matcher *m, orbx_frame *f, const float *inv_level_sigma2, orbx_keyframe **out) {
    if (out) *out = nullptr;
    if (!m || !out || !f || f->owner != m || !f->loaded || !f->fisheye) return ORBX_E_BAD_ARG;
    return keyframe_from_frame(m, true, f, inv_level_sigma2, out);
}

int orbx_keyframe_count(orbx_keyframe *kf, int *n) {
    if (!kf || !n) return ORBX_E_BAD_ARG;
    if (kf->host_n() < 0) {   // made from a batch-loaded frame: one download behind the copy
        ORBX_HIP(hipSetDevice(kf->device));
        ORBX_HIP(hipEventSynchronize(kf->ready));
        int32_t c[2] = {0, 0};
        ORBX_HIP(hipMemcpy(c, kf->count, kf->fisheye ? 8 : 4, hipMemcpyDeviceToHost));
        kf->adopt(c[0], c[1]);
        kf->done.store(true, std::memory_order_release);
    }
    *n = kf->host_n();
    return ORBX_OK;
}

int orbx_keyframe_counts(orbx_keyframe *kf, int *n_left, int *n_right) {
    if (!kf) return ORBX_E_BAD_ARG;
    int n = 0;
    const int rc = orbx_keyframe_count(kf, &n);   // at most one synchronisation, then cached
    if (rc != ORBX_OK) return rc;
    if (n_left) *n_left = kf->fisheye ? kf->host_left() : n;
    if (n_right) *n_right = kf->fisheye ? kf->host_right() : -1;
    return ORBX_OK;
}

// orbx_fuse_search for n_kf resident key frames, each with its own query set, in one call: one upload run, k_window_best1_kf over all problems, one
// download run, one synchronisation.  fisheye: every key frame is two problems (left camera, right camera), queries / rows [n_kf][2]; a right-camera
// index comes back in the rig's numbering (N_left + j, ORBmatcher.cc:1296) -- where N_left is still on the device it comes home with the results.
static int keyframe_fuse_search_impl(orbx_matcher *m, bool fisheye, int n_kf, orbx_keyframe *const *kfs, const orbx_fuse_queries *queries, int use_chi2,
                                     int strict_fp, int32_t *const *best_idx, int32_t *const *best_dist) {
    if (!m || n_kf < 0 || (n_kf > 0 && (!kfs || !queries || !best_idx || !best_dist))) return ORBX_E_BAD_ARG;
    if (n_kf > ORBX_MAX_FUSE_KEYFRAMES) return ORBX_E_TOO_LARGE;
    const int sides = fisheye ? 2 : 1, np = n_kf * sides;   // problem p: key frame p / sides, camera p % sides
    size_t total = 0;
    int nq_max = 0;
    for (int p = 0; p < np; p++) {
        const orbx_fuse_queries &q = queries[p];
        const orbx_keyframe *kf = kfs[p / sides];
        if (!kf || kf->fisheye != fisheye || kf->device != m->device || q.n < 0 || (use_chi2 && !kf->inv_sigma2)) return ORBX_E_BAD_ARG;
        if (q.n > 0 && (!q.u || !q.v || !q.r || !q.level || !q.desc || !best_idx[p] || !best_dist[p])) return ORBX_E_BAD_ARG;
        total += (size_t)q.n;
        nq_max = std::max(nq_max, q.n);
    }
    for (int p = 0; p < np; p++)
        for (int i = 0; i < queries[p].n; i++) { best_idx[p][i] = -1; best_dist[p][i] = 256; }
    if (total == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(m->device));
    std::vector<KfProblem> R((size_t)np);
    std::vector<int32_t> cnts((size_t)np), lv(total);
    std::vector<size_t> off((size_t)np);
    size_t o = 0;
    for (int p = 0; p < np; p++) {
        const orbx_fuse_queries &q = queries[p];
        keyframe_problem(kfs[p / sides], use_chi2 != 0, strict_fp, &R[p], p % sides == 1);
        cnts[p] = q.n; off[p] = o;
        for (int i = 0; i < q.n; i++) lv[o + (size_t)i] = q.level[i] - 1;   // kpLevel<nPredictedLevel-1 || kpLevel>nPredictedLevel
        o += (size_t)q.n;
    }
    int32_t *dcnt;
    KfProblem *dR;
    u64 *dkeys;
    ORBX_TRY(m->carve([&](Carve &A) {
        for (int p = 0; p < np; p++) {   // the inputs of every problem, adjacent in the arena: one upload run
            const orbx_fuse_queries &q = queries[p];
            const size_t nq = (size_t)q.n;
            if (nq == 0) continue;
            WindowProblem &P = R[p].P;
            P.qx = A.up(q.u, nq); P.qy = A.up(q.v, nq); P.qr = A.up(q.r, nq);
            P.qmin = A.up(lv.data() + off[p], nq); P.qmax = A.up(q.level, nq);
            if (P.u_right) P.qxr = A.up_opt(q.ur, nq);
            P.qdesc = A.up(q.desc, 32 * nq);
        }
        dcnt = A.up(cnts.data(), (size_t)np);
        dR = A.take<KfProblem>(np);
        dkeys = A.take<u64>(total);
    }));
    for (int p = 0; p < np; p++) { R[p].P.nq_ptr = dcnt + p; R[p].P.keys = dkeys + off[p]; }
    ORBX_TRY(m->h2d(dR, R.data(), sizeof(KfProblem) * (size_t)np));
    ORBX_TRY(keyframe_acquire(m, kfs, n_kf));
    launch_window_best1_kf(m->exec(), dR, nq_max, np);
    std::vector<u64> keys(total);
    ORBX_TRY(m->d2h(keys.data(), dkeys, 8 * total));
    std::vector<int32_t> pend;   // the counts of fisheye key frames that still have them on the device: home with the results
    ORBX_TRY(keyframe_fetch_counts(m, fisheye, n_kf, kfs, &pend));
    ORBX_TRY(m->sync_and_deliver());
    keyframe_release(kfs, n_kf);
    keyframe_take_counts(fisheye, n_kf, kfs, pend);
    for (int p = 0; p < np; p++) keyframe_fuse_results(kfs, sides, p, keys.data() + off[p], (size_t)queries[p].n, best_idx[p], best_dist[p]);
    return ORBX_OK;
}

int orbx_keyframe_fuse_search(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fuse_queries *queries, int use_chi2, int strict_fp,
                              int32_t *const *best_idx, int32_t *const *best_dist) {
    return keyframe_fuse_search_impl(m, false, n_kf, kfs, queries, use_chi2, strict_fp, best_idx, best_dist);
}

int orbx_keyframe_fuse_search_fisheye(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fuse_queries *queries, int use_chi2, int strict_fp,
                                      int32_t *const *best_idx, int32_t *const *best_dist) {
    return keyframe_fuse_search_impl(m, true, n_kf, kfs, queries, use_chi2, strict_fp, best_idx, best_dist);
}

// k_kf_project over nprob = n_kf * K.sides problems: the one launch of the key-frame projection kernel, the instantiation by the kind of key frame and member
static void launch_kf_project(hipStream_t stream, bool fisheye, bool sim3, int nprob, const KfProject &K) {
    const dim3 grid((unsigned)((K.n_mp + 255) / 256), (unsigned)nprob);
    if (fisheye && sim3) hipLaunchKernelGGL((k_kf_project<true, true>), grid, dim3(256), 0, stream, K);
    else if (fisheye) hipLaunchKernelGGL((k_kf_project<true, false>), grid, dim3(256), 0, stream, K);
    else if (sim3) hipLaunchKernelGGL((k_kf_project<false, true>), grid, dim3(256), 0, stream, K);
    else hipLaunchKernelGGL((k_kf_project<false, false>), grid, dim3(256), 0, stream, K);
}

// LocalMapping::SearchInNeighbors' Fuse loop in one call: k_kf_project writes the query records of every (key frame,
// [camera,] map point) into the arena, k_window_best1_kf searches the sides * n_kf problems -- the records never visit the host, the map points go up
// once.  Monocular: cams / poses [n_kf], one problem per key frame, Fuse(pKFi, vpMapPointMatches).  fisheye: views [n_kf][2] instead, two problems per
// key frame -- Fuse(pKFi, vpMapPointMatches) and Fuse(pKFi, vpMapPointMatches, true) -- and counts that are still on the device come home with the results.
// sim3: LoopClosing::SearchAndFuse's loop instead, Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:1339-1455) -- the records come from
// k_kf_project<., true> (no ur) and the search is the gate-less one: no inv_sigma2 wanted of the key frames, no mvuRight read.  fisheye && sim3: that member
// reads the left camera only -- views [n_kf], ONE problem per key frame (its left side), best_idx below N_left.
static int keyframe_fuse_map_points_impl(orbx_matcher *m, bool fisheye, bool sim3, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams,
                                         const orbx_frame_pose *poses, const orbx_fisheye_view *views, float th, float log_scale_factor, int strict_fp,
                                         const MapPoints &src, const uint8_t *skip, int32_t *best_idx, int32_t *best_dist, uint8_t *projected) {
    const int n_mp = src.n;
    if (!m || n_kf < 0 || n_mp < 0 || (n_kf > 0 && (!kfs || (fisheye ? !views : !cams || !poses)))) return ORBX_E_BAD_ARG;
    if (n_kf > ORBX_MAX_FUSE_KEYFRAMES) return ORBX_E_TOO_LARGE;
    const int sides = fisheye && !sim3 ? 2 : 1, nprob = n_kf * sides;   // problem p: key frame p / sides, camera p % sides (a Sim3 Fuse: the left one only)
    const size_t np = (size_t)n_mp, total = (size_t)nprob * np;
    if (total > 0 && (!best_idx || !best_dist || !map_points_ok(m, src))) return ORBX_E_BAD_ARG;
    for (int k = 0; k < n_kf; k++)
        if (!kfs[k] || kfs[k]->fisheye != fisheye || kfs[k]->device != m->device || (!sim3 && !kfs[k]->inv_sigma2)) return ORBX_E_BAD_ARG;
    if (total == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(m->device));
    const int32_t cnt4[4] = {n_mp, 0, 0, 0};
    float *qx, *qy, *qxr, *qr;
    uint8_t *dskip, *qvalid;
    int32_t *dcnt, *qmin, *qmax;
    orbx_camera *dcam;
    orbx_frame_pose *dpose;
    FisheyeView *dview;
    KfProblem *dR;
    u64 *dkeys;
    MapPointsDev D;
    ORBX_TRY(m->carve([&](Carve &A) {
        // uploads, adjacent in the arena (one run): the map points ONCE, then what grows with n_kf -- cameras and poses (a rig: two views), problem
        // records, one skip row per key frame
        D = map_points_up(A, src);
        dcnt = A.up(cnt4, 4);
        dcam = fisheye ? nullptr : A.up(cams, (size_t)n_kf);
        dpose = fisheye ? nullptr : A.up(poses, (size_t)n_kf);
        dview = fisheye ? A.up(reinterpret_cast<const FisheyeView *>(views), (size_t)nprob) : nullptr;
        dR = A.take<KfProblem>(nprob);
        dskip = A.up_opt(skip, (size_t)n_kf * np);
        // written by the projection kernel, read by k_window_best1_kf (no mvuRight on a rig: no qxr)
        qx = A.take<float>(total); qy = A.take<float>(total); qxr = fisheye || sim3 ? nullptr : A.take<float>(total); qr = A.take<float>(total);
        qmin = A.take<int32_t>(total); qmax = A.take<int32_t>(total);
        qvalid = A.take<uint8_t>(total);
        dkeys = A.take<u64>(total);
    }));
    std::vector<KfProblem> R((size_t)nprob);
    for (int p = 0; p < nprob; p++) {
        keyframe_problem(kfs[p / sides], !sim3, strict_fp, &R[p], p % sides == 1);
        WindowProblem &P = R[p].P;
        const size_t o = (size_t)p * np;
        P.qx = qx + o; P.qy = qy + o; P.qr = qr + o; P.qmin = qmin + o; P.qmax = qmax + o; P.qvalid = qvalid + o;
        if (qxr) P.qxr = qxr + o;
        P.qdesc = D.desc; P.nq_ptr = dcnt; P.keys = dkeys + o;
    }
    ORBX_TRY(m->h2d(dR, R.data(), sizeof(KfProblem) * (size_t)nprob));
    ORBX_TRY(keyframe_acquire(m, kfs, n_kf));
    uint64_t seq = 0;
    ORBX_TRY(map_points_gather(m, src, D, &seq));
    launch_kf_project(m->exec(), fisheye, sim3, nprob,
                      KfProject{dR, dcam, dpose, dview, th, log_scale_factor, ORBX_SIM3_PROJECT_CAMERA, n_mp, sides, D.pos, D.normal, D.min_dist, D.max_dist, dskip,
                                qx, qy, qxr, qr, qmin, qmax, qvalid});
    launch_window_best1_kf(m->exec(), dR, n_mp, nprob);
    std::vector<u64> keys(total);
    if (projected) ORBX_TRY(m->d2h(projected, qvalid, total));   // (adjacent to the keys: one download run)
    ORBX_TRY(m->d2h(keys.data(), dkeys, 8 * total));
    std::vector<int32_t> pend;   // the counts of fisheye key frames that still have them on the device: home with the results
    ORBX_TRY(keyframe_fetch_counts(m, fisheye, n_kf, kfs, &pend));
    ORBX_TRY(m->sync_and_deliver());
    keyframe_release(kfs, n_kf);
    map_points_done(src, seq);
    keyframe_take_counts(fisheye, n_kf, kfs, pend);
    for (int p = 0; p < nprob; p++) keyframe_fuse_results(kfs, sides, p, keys.data() + (size_t)p * np, np, best_idx + (size_t)p * np, best_dist + (size_t)p * np);
    return ORBX_OK;
}

int orbx_keyframe_fuse_map_points(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams, const orbx_frame_pose *poses, float th,
                                  float log_scale_factor, int strict_fp, int n_mp, const float *pos, const float *normal, const float *min_dist,
                                  const float *max_dist, const uint8_t *mp_desc, const uint8_t *skip, int32_t *best_idx, int32_t *best_dist,
                                  uint8_t *projected) {
    return keyframe_fuse_map_points_impl(m, false, false, n_kf, kfs, cams, poses, nullptr, th, log_scale_factor, strict_fp,
                                         MapPoints{n_mp, pos, normal, min_dist, max_dist, mp_desc, nullptr, nullptr}, skip, best_idx, best_dist, projected);
}
int orbx_keyframe_fuse_map_points_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams, const orbx_frame_pose *poses,
                                      float th, float log_scale_factor, int strict_fp, int n_mp, orbx_map *map, const int32_t *ids,
                                      const uint8_t *skip, int32_t *best_idx, int32_t *best_dist, uint8_t *projected) {
    if (!map_form_ok(map, n_mp)) return ORBX_E_BAD_ARG;
    return keyframe_fuse_map_points_impl(m, false, false, n_kf, kfs, cams, poses, nullptr, th, log_scale_factor, strict_fp, map_points_of(n_mp, map, ids), skip,
                                         best_idx, best_dist, projected);
}

int orbx_keyframe_fuse_map_points_fisheye(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fisheye_view *views, float th,
                                          float log_scale_factor, int strict_fp, int n_mp, const float *pos, const float *normal, const float *min_dist,
                                          const float *max_dist, const uint8_t *mp_desc, const uint8_t *skip, int32_t *best_idx, int32_t *best_dist,
                                          uint8_t *projected) {
    return keyframe_fuse_map_points_impl(m, true, false, n_kf, kfs, nullptr, nullptr, views, th, log_scale_factor, strict_fp,
                                         MapPoints{n_mp, pos, normal, min_dist, max_dist, mp_desc, nullptr, nullptr}, skip, best_idx, best_dist, projected);
}
int orbx_keyframe_fuse_map_points_fisheye_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fisheye_view *views, float th,
                                              float log_scale_factor, int strict_fp, int n_mp, orbx_map *map, const int32_t *ids, const uint8_t *skip,
                                              int32_t *best_idx, int32_t *best_dist, uint8_t *projected) {
    if (!map_form_ok(map, n_mp)) return ORBX_E_BAD_ARG;
    return keyframe_fuse_map_points_impl(m, true, false, n_kf, kfs, nullptr, nullptr, views, th, log_scale_factor, strict_fp, map_points_of(n_mp, map, ids),
                                         skip, best_idx, best_dist, projected);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// BoW on resident key frames: KeyFrame::ComputeBoW / the mBowVec, mFeatVec part of KeyFrame::KeyFrame(Frame&), and the three BoW-guided matchers with
// BOTH sides resident -- SearchByBoW(KeyFrame*, Frame&), SearchByBoW(KeyFrame*, KeyFrame*) and SearchForTriangulation (pinhole gates; between
// fisheye-stereo key frames KannalaBrandt8::epipolarConstrain) -- through one driver (run_bow_resident): only flags and problem records go up.
// Both kinds of key frame share every host path here, the kind being a `bool rig` of that path; the public entry points name the kind.
// ---------------------------------------------------------------------------------------------------------
namespace {

static_assert(sizeof(BowProblem) + sizeof(BowPairSrc) <= 512, "the per-problem upload of a resident BoW search (tests/test_gpu_keyframe_bow.py bounds it)");
static_assert(sizeof(BowProblem) + sizeof(BowPairSrc) + sizeof(BowRigRows) <= 512, "the same between fisheye-stereo sides (tests/test_gpu_keyframe_bow_fisheye.py)");
constexpr int kKeyFrameBowMax = 16384;   // k_frame_featvec sorts 8-byte keys in LDS: 128 KB at most

int keyframe_bow_alloc(int cap, KeyFrameBow **out) {
    KeyFrameBow *b = new KeyFrameBow();
    const size_t c = (size_t)std::max(cap, 1);
    Layout L;
    const size_t off_w = L.add(4 * c), off_n = L.add(4 * c), off_a = L.add(4 * c), off_fn = L.add(4 * c), off_fp = L.add(4 * (c + 1)), off_fi = L.add(4 * c),
                 off_m = L.add(8);
    hipError_t e = hipMalloc((void **)&b->dev, L.used);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&b->ready, hipEventDisableTiming);
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); keyframe_bow_free(b); return ORBX_E_HIP; }
    b->word = (int32_t *)(b->dev + off_w); b->node = (int32_t *)(b->dev + off_n); b->angle = (float *)(b->dev + off_a);
    b->fv_node = (uint32_t *)(b->dev + off_fn); b->fv_ptr = (int32_t *)(b->dev + off_fp); b->fv_index = (int32_t *)(b->dev + off_fi);
    b->fv_meta = (int32_t *)(b->dev + off_m);
    *out = b;
    return ORBX_OK;
}

// the calling context's stream behind the key frame's rows AND its BoW state (each until a call that waited has synchronised)
inline int keyframe_bow_acquire(orbx_matcher *m, orbx_keyframe *kf) {
    if (!kf->done.load(std::memory_order_acquire)) ORBX_HIP(hipStreamWaitEvent(m->stream, kf->ready, 0));
    KeyFrameBow *b = kf->bow.load(std::memory_order_acquire);
    if (b && !b->done.load(std::memory_order_acquire)) ORBX_HIP(hipStreamWaitEvent(m->stream, b->ready, 0));
    return ORBX_OK;
}
inline void keyframe_bow_release(orbx_keyframe *kf) {   // after the call's synchronisation
    kf->done.store(true, std::memory_order_release);
    if (KeyFrameBow *b = kf->bow.load(std::memory_order_acquire)) b->done.store(true, std::memory_order_release);
}

// One side of a resident BoW problem: a key frame with BoW, or the frame handle.
// its rows (a fisheye-stereo side in ROW space: the flags, the match row, vbMatched2 and the entries go by HandleRows::rows()) and its BoW arrays.
struct BowSide : BowTarget {
    int bound;   // the host's bound on the FeatureVector's node count
    int flag_n() const { return fisheye ? rows() : n; }                              // entries of the side's flags as they go up
};
inline BowSide bow_side(const HandleRows &r, const BowArrays &b) { return BowSide{bow_target(r, b), std::min(r.feats(), b.voc->node_bound(b.levelsup))}; }
inline BowSide bow_side(const orbx_keyframe *kf) { return bow_side(kf->view(), *kf->bow.load(std::memory_order_acquire)); }

// LocalMapping::CreateNewMapPoints' triangulation (k_new_points, include/orbx.h) as one call sees it: alone over pairs the host names
// (keyframe_triangulate_pairs) or behind SearchForTriangulation on the row it left on the device (run_bow_resident's optional argument).  Both carve the
// same buffers through it: the level tables and the record among the call's uploads, pos / status / the flag (+ the counts as the kernel read them) side
// by side among its downloads.  The results land here and reach the caller's arrays behind the synchronisation, and only if the flag stayed down.
static_assert(sizeof(NewPoints) == 544, "the record a triangulating call uploads (tests/test_gpu_new_points.py states its size)");
static_assert(sizeof(NewPointsStereoRec) == 592, "the record of the `_stereo` forms (tests/test_gpu_stereo_resident.py states its size)");
struct NewPointsCall {
    NewPoints rec;                      // views, key-frame rows and parameters (new_points_prepare); the arena's addresses are filled in by stage()
    bool stereo = false;                // the `_stereo` forms: the record that goes up is a NewPointsStereoRec, rec with what follows
    const float *depth[2] = {nullptr, nullptr}, *keys_xy[2] = {nullptr, nullptr};   // the key frames' mvDepth / raw (x, y) rows (NULL: none)
    float mb[2] = {0, 0}, mbf[2] = {0, 0};
    const float *sigma2[2];             // the caller's mvLevelSigma2 tables
    const float *dsig[2];
    NewPoints *drec; float *dpos; uint8_t *dstatus; int32_t *dflag;
    bool ran = false;
    std::vector<int32_t> matches;       // the fused form's row
    std::vector<float> pos; std::vector<uint8_t> status; int32_t flag[8];
    // have1 / have2: the search sends that table itself (at d1 / d2)
    void carve_up(Carve &C, bool have1, bool have2, const float *d1, const float *d2) {
        dsig[0] = have1 ? d1 : C.up(sigma2[0], (size_t)rec.kf[0].nlevels);
        dsig[1] = have2 ? d2 : C.up(sigma2[1], (size_t)rec.kf[1].nlevels);
        drec = stereo ? &C.take<NewPointsStereoRec>(1)->base : C.take<NewPoints>(1);
    }
    void carve_out(Carve &C, int n) { dpos = C.take<float>(3 * (size_t)n); dstatus = C.take<uint8_t>((size_t)n); dflag = C.take<int32_t>(8); }
    int stage(orbx_matcher *m, const int32_t *didx1, const int32_t *dmatch, int n, bool counts) {
        rec.kf[0].sigma2 = dsig[0]; rec.kf[1].sigma2 = dsig[1];
        rec.idx1 = didx1; rec.match = dmatch; rec.pos = dpos; rec.status = dstatus; rec.flag = dflag; rec.n = n; rec.counts_out = counts ? 1 : 0;
        if (stereo) {
            NewPointsStereoRec E;
            E.base = rec;
            for (int k = 0; k < 2; k++) { E.depth[k] = depth[k]; E.keys_xy[k] = keys_xy[k]; E.mb[k] = mb[k]; E.mbf[k] = mbf[k]; }
            ORBX_TRY(m->h2d(drec, &E, sizeof(E)));
        } else {
            ORBX_TRY(m->h2d(drec, &rec, sizeof(rec)));
        }
        ORBX_HIP(m->fill(dflag, 0, sizeof(flag)));
        return ORBX_OK;
    }
    void launch(orbx_matcher *m, bool rig, int n) {
        const dim3 grid((unsigned)((n + kNewPointsBlock - 1) / kNewPointsBlock)), block(kNewPointsBlock);
        if (stereo) hipLaunchKernelGGL(k_new_points_stereo, grid, block, 0, m->exec(), (const NewPoints *)drec);
        else if (rig) hipLaunchKernelGGL(k_new_points<true>, grid, block, 0, m->exec(), (const NewPoints *)drec);
        else hipLaunchKernelGGL(k_new_points<false>, grid, block, 0, m->exec(), (const NewPoints *)drec);
        ran = true;
    }
    int fetch(orbx_matcher *m, int n) {
        pos.resize(3 * (size_t)n); status.resize((size_t)n);
        ORBX_TRY(m->d2h(pos.data(), dpos, 12 * (size_t)n));
        ORBX_TRY(m->d2h(status.data(), dstatus, (size_t)n));
        return m->d2h(flag, dflag, sizeof(flag));
    }
    // behind the synchronisation: status of every pair, pos of the accepted ones; a raised flag leaves the caller's arrays alone
    int deliver(int n, float *out_pos, uint8_t *out_status, int *n_accepted) const {
        if (ran && flag[0]) { set_error("an index outside [0, N) of its key frame, or a key point whose octave is outside its pyramid"); return ORBX_E_BAD_ARG; }
        int accepted = 0;
        for (int p = 0; p < n; p++) {
            out_status[p] = ran ? status[p] : (uint8_t)ORBX_NEWPT_NO_MATCH;   // (a search that found a side empty launched nothing)
            if (out_status[p] != ORBX_NEWPT_OK) continue;
            memcpy(out_pos + 3 * (size_t)p, pos.data() + 3 * (size_t)p, 12);
            accepted++;
        }
        if (n_accepted) *n_accepted = accepted;
        return ORBX_OK;
    }
};

// the checks both forms share and the host's part of the record; views: orbx_new_points_view (one per key frame) or, rig, orbx_fisheye_view [2] each
int new_points_prepare(const orbx_matcher *m, bool rig, const orbx_keyframe *kf1, const orbx_keyframe *kf2, const void *views1, const void *views2,
                       const orbx_new_points_params *par, const orbx_new_points_stereo *st, bool stereo, NewPointsCall &T) {
    if (!m || !kf1 || !kf2 || !views1 || !views2 || !par || !par->level_sigma2_1 || !par->level_sigma2_2 || (stereo && (!st || rig))) return ORBX_E_BAD_ARG;
    const orbx_keyframe *kfs[2] = {kf1, kf2};
    const void *views[2] = {views1, views2};
    const int nlevels[2] = {par->nlevels_1, par->nlevels_2};
    memset(&T.rec, 0, sizeof(T.rec));
    for (int k = 0; k < 2; k++) {
        if (kfs[k]->fisheye != rig || kfs[k]->device != m->device || nlevels[k] != kfs[k]->nlevels) return ORBX_E_BAD_ARG;
        static_assert(sizeof(orbx_fisheye_view) == sizeof(FisheyeView), "orbx_fisheye_view is FisheyeView");
        if (rig) {
            memcpy(&T.rec.view[2 * k], views[k], 2 * sizeof(FisheyeView));
        } else {
            const orbx_new_points_view *v = static_cast<const orbx_new_points_view *>(views[k]);
            FisheyeView &V = T.rec.view[2 * k];
            memcpy(V.R, v->Rcw, sizeof(V.R)); memcpy(V.t, v->tcw, sizeof(V.t)); memcpy(V.twc, v->Ow, sizeof(V.twc));
            V.p[0] = v->fx; V.p[1] = v->fy; V.p[2] = v->cx; V.p[3] = v->cy;
        }
        NewPointsKf &R = T.rec.kf[k];
        R.kps = kfs[k]->kps; R.scale = kfs[k]->scale; R.u_right = kfs[k]->u_right; R.count = kfs[k]->count;
        R.roff = kfs[k]->roff; R.cap = kfs[k]->cap; R.nlevels = kfs[k]->nlevels;
        if (stereo) { T.depth[k] = kfs[k]->depth; T.keys_xy[k] = kfs[k]->keys_xy; T.mb[k] = k ? st->mb2 : st->mb1; T.mbf[k] = k ? st->mbf2 : st->mbf1; }
    }
    T.stereo = stereo;
    T.sigma2[0] = par->level_sigma2_1; T.sigma2[1] = par->level_sigma2_2;
    T.rec.ratio_factor = par->ratio_factor; T.rec.inertial = par->inertial ? 1 : 0;
    T.rec.far_points = par->far_points ? 1 : 0; T.rec.th_far_points = par->th_far_points;
    return ORBX_OK;
}

// The driver of the resident BoW searches of both kinds of side.  Problem k: A[k] against B[k] in `mode` (BowProblem::mode: 0 / 3 rows indexed by B's
// features, 1 / 2 by A's); flags_a[k] / flags_b[k] (arrays may be NULL, entries may be NULL = no feature is switched off) are `valid` flags when invert, else `skip`
// flags, of A[k].n / B[k].n entries (the callers resolve N before they hand over flags).  The side the rows are indexed by is the same object in
// every problem.  One upload run (flags, the level table of the gate, the records), k_bow_pair_resident, k_replay_bow_batch,
// k_replay_bow_finish_batch, one download run (rows, match counts, the sides' counts), one synchronisation -- whatever np is, and with no host
// synchronisation before the launches.  counts[4 k ..] = the counts of A[k], then of B[k], as read on the device: N and 0, of a rig side N_left and N_right.
// rig: every side is a fisheye-stereo one, in ROW space.  The flags still come in the reference's feature numbering and are laid out by rows here (mode 1
// also switches every right-camera row off on both sides, ORBmatcher.cc:800-802, :820-822 -- roff is on the host, so this needs no count), and
// k_bow_rig_rows hands rows and values back in feature numbering, with both counts of both sides.  kb8 (mode 2, rig): the KannalaBrandt8 gate of
// k_tri_kb8_resident, which then takes k_replay_bow_batch's place; its level table sigma2_1 and the record ride up beside sigma2_2.
// tri (mode 2, np = 1, A's N known): CreateNewMapPoints' triangulation of the row behind the chain (NewPointsCall) -- its record and the level tables the
// gate does not send ride up beside the gate's, k_new_points reads the row where it lies, pos / status / the flag lie between the row and the counts and come home
// in the same download run.  One launch more, nothing else changes; without it every statement here is the one it was.
int run_bow_resident(orbx_matcher *m, int mode, int np, const BowSide *A, const BowSide *B, const uint8_t *const *flags_a, const uint8_t *const *flags_b,
                     bool invert, float nnratio, int check_orientation, const TriGate *gate, const float *sigma2_2, int nlevels, int32_t *match,
                     int match_stride, int32_t *nmatches, std::vector<int32_t> &counts, bool rig = false, const Kb8Gate *kb8 = nullptr,
                     const float *sigma2_1 = nullptr, NewPointsCall *tri = nullptr) {
    const bool to_b = mode == 0 || mode == 3;
    const BowSide &O = to_b ? B[0] : A[0];
    const int nrows = O.rows(), nfeat = O.feats();
    // mode 3 appends up to two entries per query (BowProblem::entries)
    auto entries_of = [&](int k) { return (size_t)(mode == 3 ? 2 : 1) * (size_t)std::max(std::max(A[k].rows(), B[k].rows()), 1); };
    size_t tot_bound = 0, tot_nb = 0, n_ent = 0;
    int max_bound = 1;
    for (int k = 0; k < np; k++) {
        tot_bound += (size_t)A[k].bound; tot_nb += (size_t)B[k].rows(); n_ent += entries_of(k);
        max_bound = std::max(max_bound, A[k].bound);
    }
    std::vector<BowProblem> probs((size_t)np);
    memset(probs.data(), 0, sizeof(BowProblem) * (size_t)np);
    std::vector<BowPairSrc> srcs((size_t)np);
    // the flags of side A and B of problem k at [2 k], [2 k + 1] (NULL / no feature: none): `skip` flags as they are, `valid` flags inverted in `skip` first
    std::vector<const uint8_t *> flags(2 * (size_t)np, nullptr);
    std::vector<uint8_t> skip;
    for (int k = 0; k < np; k++) {
        if (flags_a && A[k].n > 0) flags[2 * (size_t)k] = flags_a[k];
        if (flags_b && B[k].n > 0) flags[2 * (size_t)k + 1] = flags_b[k];
    }
    if (invert || rig) {
        const bool left_only = rig && mode == 1;
        constexpr size_t kNone = ~(size_t)0;
        std::vector<size_t> at(flags.size(), kNone);
        for (size_t s = 0; s < flags.size(); s++) {
            const BowSide &S = s & 1 ? B[s / 2] : A[s / 2];
            if (!flags[s] && !(left_only && S.rows() > S.roff)) continue;
            at[s] = skip.size();
            auto off = [&](size_t i) { return (uint8_t)((flags[s][i] != 0) == invert ? 0 : 1); };
            if (!rig) {
                for (size_t i = 0; i < (size_t)S.n; i++) skip.push_back(off(i));
                continue;
            }
            skip.resize(at[s] + (size_t)S.rows(), 0);
            uint8_t *row = skip.data() + at[s];
            for (int i = 0; flags[s] && i < S.nl; i++) row[i] = off((size_t)i);
            for (int j = 0; flags[s] && j < S.nr; j++) row[S.roff + j] = off((size_t)S.nl + j);
            for (int r = S.roff; left_only && r < S.rows(); r++) row[r] = 1;
        }
        for (size_t s = 0; s < flags.size(); s++)
            flags[s] = at[s] == kNone ? nullptr : skip.data() + at[s];
    }
    const float *dsig = nullptr, *dsig1 = nullptr;
    Kb8Gate *dK = nullptr;
    BowProblem *dP;
    BowPairSrc *dS;
    BowRigRows *dR = nullptr;
    int32_t *dpair, *dmatch, *dout, *dpc = nullptr, *dnm, *dcnt, *dhist, *dent;
    uint8_t *dtaken;
    const size_t cnt_per = rig ? 4 : 2;
    ORBX_TRY(m->carve([&](Carve &C) {
        // the uploads, side by side: the flags, the gate's level table(s) and the rig's gate, the records
        for (int k = 0; k < np; k++) {
            probs[k].skip_a = C.up_opt(flags[2 * (size_t)k], (size_t)A[k].flag_n());
            probs[k].skip_b = C.up_opt(flags[2 * (size_t)k + 1], (size_t)B[k].flag_n());
        }
        if (gate) dsig = C.up(sigma2_2, (size_t)nlevels);
        if (kb8) { dsig1 = C.up(sigma2_1, (size_t)nlevels); dK = C.take<Kb8Gate>(1); }
        if (tri) tri->carve_up(C, kb8 != nullptr, gate != nullptr, dsig1, dsig);
        dP = C.take<BowProblem>(np);
        dS = C.take<BowPairSrc>(np);
        if (rig) dR = C.take<BowRigRows>(np);
        // device-only: the pairing; rows (filled with -1), match counts and the sides' counts side by side (one download run); vbMatched2, histograms +
        // counters (zeroed by one fill); entries.  rig: the rows the caller gets are k_bow_rig_rows' (k_bow_pair_resident's one count per side is not used)
        dpair = C.take<int32_t>(tot_bound + 1);
        dmatch = C.take<int32_t>((size_t)np * nrows);
        if (rig) dpc = C.take<int32_t>(2 * (size_t)np);
        dout = rig ? C.take<int32_t>((size_t)np * nfeat) : dmatch;
        if (tri) tri->carve_out(C, nfeat);   // (between the row and the counts: one download run)
        dnm = C.take<int32_t>(np);
        dcnt = C.take<int32_t>(cnt_per * (size_t)np);
        dtaken = C.take<uint8_t>(tot_nb + 1);
        dhist = C.take<int32_t>((size_t)np * (ORBX_HISTO_LENGTH + 2));
        dent = C.take<int32_t>(n_ent);
    }));
    std::vector<BowRigRows> rigs(rig ? (size_t)np : 0);
    {
        size_t op = 0, ot = 0, oe = 0;
        for (int k = 0; k < np; k++) {
            BowProblem &P = probs[k];
            const BowSide &a = A[k], &b = B[k];
            P.mode = mode;
            if (mode == 3) P.nb_left = b.roff;   // a row >= roff is the right camera's
            if (gate) { P.gate = *gate; P.gate.sigma2_2 = dsig; P.gate.kb8 = dK; }
            P.fa.node_id = a.fv_node; P.fa.node_ptr = a.fv_ptr; P.fa.index = a.fv_index; P.fa.n_nodes = 0;   // (both node counts: k_bow_pair_resident)
            P.fb.node_id = b.fv_node; P.fb.node_ptr = b.fv_ptr; P.fb.index = b.fv_index; P.fb.n_nodes = 0;
            P.desc_a = a.desc; P.angle_a = a.angle; P.na = a.rows();
            P.desc_b = b.desc; P.angle_b = b.angle; P.nb = b.rows();
            P.nnratio = nnratio; P.check_orientation = check_orientation ? 1 : 0;
            P.match = dmatch + (size_t)k * nrows; P.nmatches = dnm + k;
            P.taken_b = dtaken + ot;
            P.hist = dhist + (size_t)k * (ORBX_HISTO_LENGTH + 2); P.counters = P.hist + ORBX_HISTO_LENGTH;
            P.entries = dent + oe;
            P.pair_b = dpair + op;
            BowPairSrc &S = srcs[k];
            memset(&S, 0, sizeof(S));
            S.node_a = a.fv_node; S.node_b = b.fv_node; S.meta_a = a.fv_meta; S.meta_b = b.fv_meta; S.count_a = a.count; S.count_b = b.count;
            S.pair = dpair + op; S.counts_out = (rig ? dpc : dcnt) + 2 * (size_t)k; S.bound_a = a.bound; S.cap_a = a.cap; S.cap_b = b.cap;
            op += (size_t)a.bound; ot += (size_t)b.rows(); oe += entries_of(k);
            if (rig) {
                BowRigRows &R = rigs[k];
                memset(&R, 0, sizeof(R));
                R.in = P.match; R.out = dout + (size_t)k * nfeat; R.counts_out = dcnt + 4 * (size_t)k; R.out_n = nfeat; R.index_side = to_b ? 1 : 0;
                const BowSide *sd[2] = {&a, &b};
                for (int s = 0; s < 2; s++) { R.count[s] = sd[s]->count; R.nl[s] = sd[s]->nl; R.nr[s] = sd[s]->nr; R.cap[s] = sd[s]->cap; R.roff[s] = sd[s]->roff; }
            }
        }
    }
    if (kb8) {
        Kb8Gate K = *kb8;
        K.sigma2_1 = dsig1;
        ORBX_TRY(m->h2d(dK, &K, sizeof(K)));
    }
    ORBX_TRY(m->h2d(dP, probs.data(), sizeof(BowProblem) * (size_t)np));
    ORBX_TRY(m->h2d(dS, srcs.data(), sizeof(BowPairSrc) * (size_t)np));
    if (rig) ORBX_TRY(m->h2d(dR, rigs.data(), sizeof(BowRigRows) * (size_t)np));
    if (tri) ORBX_TRY(tri->stage(m, nullptr, dout, nfeat, false));   // (the row in feature numbering: a rig's is k_bow_rig_rows')
    ORBX_HIP(m->fill(dmatch, 0xff, 4 * (size_t)np * nrows));
    ORBX_HIP(m->fill(dtaken, 0, (size_t)((const uint8_t *)(dhist + (size_t)np * (ORBX_HISTO_LENGTH + 2)) - dtaken)));   // vbMatched2, (padding,) histograms + counters
    hipLaunchKernelGGL(k_bow_pair_resident, dim3((unsigned)((max_bound + 255) / 256), (unsigned)np), dim3(256), 0, m->exec(), dP, (const BowPairSrc *)dS);
    if (kb8) hipLaunchKernelGGL(k_tri_kb8_resident, dim3((unsigned)((max_bound + 3) / 4), (unsigned)np), dim3(256), 0, m->exec(), (const BowProblem *)dP);
    else hipLaunchKernelGGL(k_replay_bow_batch, dim3((unsigned)((max_bound + 3) / 4), (unsigned)np), dim3(256), 0, m->exec(), (const BowProblem *)dP);
    hipLaunchKernelGGL(k_replay_bow_finish_batch, dim3((unsigned)np), dim3(64), 0, m->exec(), (const BowProblem *)dP);
    if (rig) hipLaunchKernelGGL(k_bow_rig_rows, dim3((unsigned)((std::max(nfeat, 1) + 255) / 256), (unsigned)np), dim3(256), 0, m->exec(), (const BowRigRows *)dR);
    if (tri) tri->launch(m, rig, nfeat);
    ORBX_HIP(hipGetLastError());
    std::vector<int32_t> land;
    PendingRows down{m, land, O.n < 0};   // N comes back with the results (the sides' counts, below)
    const Rows rows = {dout, np, rig ? nfeat : nrows, match, (size_t)match_stride};   // (N known: nfeat = nrows = N)
    ORBX_TRY(down.fetch(&rows));
    std::vector<int32_t> got(cnt_per * (size_t)np, 0);
    ORBX_TRY(m->d2h(nmatches, dnm, 4 * (size_t)np));
    ORBX_TRY(m->d2h(got.data(), dcnt, 4 * got.size()));
    if (tri) ORBX_TRY(tri->fetch(m, nfeat));
    ORBX_TRY(m->sync_and_deliver());
    counts.assign(4 * (size_t)np, 0);
    for (size_t k = 0; k < (size_t)np; k++)
        for (size_t s = 0; s < 2; s++) {
            counts[4 * k + 2 * s] = got[cnt_per * k + (rig ? 2 : 1) * s];
            if (rig) counts[4 * k + 2 * s + 1] = got[4 * k + 2 * s + 1];
        }
    if (O.n < 0) {
        const int32_t *c = counts.data() + (to_b ? 2 : 0);
        down.take(&rows, 1, std::min(std::max(c[0] + c[1], 0), O.feats()));
    }
    return ORBX_OK;
}

// a key frame a BoW search of its kind (rig: fisheye-stereo) may take: on this device, with BoW; the vocabulary and levelsup it was made with come back
// for the cross-check
inline bool keyframe_bow_ok(const orbx_matcher *m, bool rig, const orbx_keyframe *kf, const orbx_vocabulary **voc, int *levelsup) {
    if (!kf || kf->fisheye != rig || kf->device != m->device) return false;
    const KeyFrameBow *b = kf->bow.load(std::memory_order_acquire);
    if (!b) return false;
    if (*voc && (*voc != b->voc || *levelsup != b->levelsup)) return false;
    *voc = b->voc; *levelsup = b->levelsup;
    return true;
}
// what a call learnt of a key frame's pending counts (run_bow_resident's counts of that side)
inline void keyframe_adopt(orbx_keyframe *kf, const int32_t *c) {
    if (kf->host_n() < 0) kf->adopt(c[0], c[1]);
}

// ---- The five calls below are one path per protocol for both kinds of key frame (rig: fisheye-stereo); the public entry points name the kind.

// KeyFrame::ComputeBoW on the key frame's own descriptors through launch_compute_bow.  A rig key frame is a fisheye BowTarget in row space; its ids come
// down renumbered into features [0, N) by k_frame_rows_to_features, so pending counts cost no wait.
int keyframe_compute_bow(orbx_matcher *m, bool rig, orbx_keyframe *kf, const orbx_vocabulary *v, int levelsup, int32_t *word_id, int32_t *node_id) {
    if (!m || !kf || !v || kf->fisheye != rig || kf->device != m->device || v->device != m->device) return ORBX_E_BAD_ARG;
    KeyFrameBow *b = kf->bow.load(std::memory_order_acquire);
    const bool down = word_id || node_id;
    if (b) {   // `if (mBowVec.empty() || mFeatVec.empty())`: not computed again
        if (b->voc != v || b->levelsup != levelsup) return ORBX_E_BAD_ARG;
        if (!down) return ORBX_OK;
    }
    const HandleRows rows = kf->view();
    const int n_host = rows.n, nc = rows.feats();   // nc: features the kernels may see
    if (rows.rows() > kKeyFrameBowMax) return ORBX_E_TOO_LARGE;   // (the rows the BoW state may have to index)
    ORBX_HIP(hipSetDevice(m->device));
    int32_t *dids = nullptr;   // rig: word ids, then node ids, in features [0, N)
    ORBX_TRY(m->carve([&](Carve &A) { dids = A.take<int32_t>(2 * (size_t)nc); }));   // (monocular: the room the ids take in the staging)
    if (!b) {
        ORBX_TRY(keyframe_bow_alloc(kf->cap, &b));
        b->voc = v; b->levelsup = levelsup;
        hipError_t e = hipSuccess;
        if (!kf->done.load(std::memory_order_acquire)) e = hipStreamWaitEvent(m->stream, kf->ready, 0);
        if (e == hipSuccess) {
            m->dirty = true;
            e = launch_compute_bow(m, v, levelsup, bow_target(rows, *b));
        }
        if (e == hipSuccess) e = hipEventRecord(b->ready, m->stream);
        if (e != hipSuccess) { set_error(hipGetErrorString(e)); (void)hipStreamSynchronize(m->stream); m->dirty = false; keyframe_bow_free(b); return ORBX_E_HIP; }
        kf->bow.store(b, std::memory_order_release);
    } else {
        ORBX_TRY(keyframe_bow_acquire(m, kf));
    }
    if (!down || nc == 0) return ORBX_OK;
    const int32_t *src_w = b->word, *src_n = b->node;
    if (rig) {
        launch_bow_ids_to_features(m->exec(), rows, *b, nc, dids);
        ORBX_HIP(hipGetLastError());
        src_w = dids; src_n = dids + nc;
    }
    std::vector<int32_t> land;
    PendingRows got{m, land, n_host < 0};
    const Rows ids[2] = {{src_w, 1, nc, word_id, 0}, {src_n, 1, nc, node_id, 0}};
    int32_t cnt[2] = {n_host, 0};
    ORBX_TRY(got.fetch(ids, 2));
    if (n_host < 0) ORBX_TRY(m->d2h(cnt, kf->count, rig ? 8 : 4));   // N comes back with the ids
    ORBX_TRY(m->sync_and_deliver());
    keyframe_bow_release(kf);
    if (n_host < 0) {
        kf->adopt(cnt[0], cnt[1]);
        got.take(ids, 2, kf->host_n());
    }
    return ORBX_OK;
}

// mBowVec(F.mBowVec), mFeatVec(F.mFeatVec) of KeyFrame::KeyFrame(Frame&) (KeyFrame.cc:36-82): k_keyframe_bow_copy[_fisheye] on the owner's stream,
// behind the frame's ComputeBoW and ahead of its next load; no host synchronisation.
int keyframe_bow_from_frame(orbx_matcher *m, bool rig, orbx_keyframe *kf, orbx_frame *f) {
    if (!m || !kf || !f || f->owner != m || f->fisheye != rig || kf->fisheye != rig || kf->device != m->device || kf->src_frame != f) return ORBX_E_BAD_ARG;
    if (kf->bow.load(std::memory_order_acquire)) return ORBX_E_BAD_ARG;   // set once
    if (f->load_seq != kf->src_seq) return ORBX_E_STALE;                  // the handle holds another frame by now
    if (!f->bow_valid) return ORBX_E_BAD_ARG;
    if ((rig ? kf->view().rows() : f->rows_n()) > kKeyFrameBowMax) return ORBX_E_TOO_LARGE;
    ORBX_HIP(hipSetDevice(m->device));
    KeyFrameBow *b = nullptr;
    int r = keyframe_bow_alloc(kf->cap, &b);
    if (r != ORBX_OK) return r;
    const BowArrays &S = f->bow, &D = *b;
    b->voc = S.voc; b->levelsup = S.levelsup;
    KeyFrameBowCopyFisheye Cf;
    memset(&Cf, 0, sizeof(Cf));
    KeyFrameBowCopy &Cp = Cf.c;
    Cp.src_count = f->count; Cp.n_host = f->host_n(); Cp.cap = kf->cap;
    Cp.src_word = S.word; Cp.src_node = S.node; Cp.src_ptr = S.fv_ptr; Cp.src_index = S.fv_index; Cp.src_meta = S.fv_meta; Cp.src_fv_node = S.fv_node; Cp.src_angle = S.angle;
    Cp.word = D.word; Cp.node = D.node; Cp.ptr = D.fv_ptr; Cp.index = D.fv_index; Cp.meta = D.fv_meta; Cp.fv_node = D.fv_node; Cp.angle = D.angle;
    m->dirty = true;
    if (rig) {
        Cf.nl_host = f->host_left(); Cf.nr_host = f->host_right(); Cf.src_roff = f->roff; Cf.src_cap = f->cap; Cf.roff = kf->roff;
        hipLaunchKernelGGL(k_keyframe_bow_copy_fisheye, dim3((unsigned)((kf->cap + 256) / 256)), dim3(256), 0, m->stream, Cf);
    } else {
        hipLaunchKernelGGL(k_keyframe_bow_copy, dim3((unsigned)((kf->cap + 256) / 256)), dim3(256), 0, m->stream, Cp);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(b->ready, m->stream);
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); (void)hipStreamSynchronize(m->stream); m->dirty = false; keyframe_bow_free(b); return ORBX_E_HIP; }
    kf->bow.store(b, std::memory_order_release);
    return ORBX_OK;
}

}  // namespace

extern "C" {

// KeyFrame::ComputeBoW (KeyFrame.cc; the transform of Frame.cc:738-745) on the key frame's own descriptors.  The kernels are the FRAME's
// (k_frame_bow_transform, k_frame_featvec): they take every array as an argument, so they run on the key frame's rows as they are -- no new code object,
// no existing kernel's ISA touched.
int orbx_keyframe_compute_bow(orbx_matcher *m, orbx_keyframe *kf, const orbx_vocabulary *v, int levelsup, int32_t *word_id, int32_t *node_id) {
    return keyframe_compute_bow(m, false, kf, v, levelsup, word_id, node_id);
}
// The same over all N = N_left + N_right descriptor rows of a fisheye-stereo key frame: k_frame_bow_transform_fisheye / k_frame_featvec_fisheye in row
// space; the ids come back in the reference's numbering, left then right.
int orbx_keyframe_compute_bow_fisheye(orbx_matcher *m, orbx_keyframe *kf, const orbx_vocabulary *v, int levelsup, int32_t *word_id, int32_t *node_id) {
    return keyframe_compute_bow(m, true, kf, v, levelsup, word_id, node_id);
}

// mBowVec(F.mBowVec), mFeatVec(F.mFeatVec) of KeyFrame::KeyFrame(Frame&) (KeyFrame.cc:36-82) from the handle the key frame was made from
int orbx_keyframe_bow_from_frame(orbx_matcher *m, orbx_keyframe *kf, orbx_frame *f) { return keyframe_bow_from_frame(m, false, kf, f); }
int orbx_keyframe_bow_from_frame_fisheye(orbx_matcher *m, orbx_keyframe *kf, orbx_frame *f) { return keyframe_bow_from_frame(m, true, kf, f); }

// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:329-403) for a batch of map points whose observations are rows of resident key frames of either
// kind: k_distinctive_kf (sets of up to 64 rows) and k_distinctive_kf_large gather the rows through a record per key frame.  One upload run (set_ptr, the
// two index arrays, the records, the list of large sets), one launch per kernel, one download run (best_obs, the flag, best_desc, the counts of key
// frames that still had them on the device), one synchronisation.
// map != NULL (orbx_keyframe_distinctive_descriptors_to_map): best_desc stays in the arena and k_map_scatter_desc writes its rows into the slots set_id
// names, ordered as an update of the table.
// nd != NULL: MapPoint::UpdateNormalAndDepth over the same observation lists (k_normal_depth_kf), alone (distinct = false:
// orbx_keyframe_update_normal_and_depth[_to_map]) or behind the distinctive kernels (orbx_keyframe_refresh_map_points_to_map); with a table its results
// (and the winning rows) go into the slots through ONE k_map_scatter_refresh.  Same checks, same upload run, same download run, same synchronisation.
struct NormalDepth {
    const float *centers, *centers_right; const int32_t *ref_obs;
    const float *pos;                       // flat form; NULL with a table
    float *normal, *min_dist, *max_dist;    // outputs; each may be NULL with a table
};
static int keyframe_distinctive_impl(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, int n_sets, const int32_t *set_ptr, const int32_t *obs_kf,
                                     const int32_t *obs_idx, int32_t *best_obs, uint8_t *best_desc, orbx_map *map, const int32_t *set_id,
                                     const NormalDepth *nd = nullptr, bool distinct = true) {
    if (!m || n_kf < 0 || n_sets < 0 || (n_kf > 0 && !kfs) || (n_sets > 0 && (!set_ptr || (distinct && !best_obs)))) return ORBX_E_BAD_ARG;
    if (n_kf > ORBX_MAX_DISTINCTIVE_KEYFRAMES) return ORBX_E_TOO_LARGE;
    if (n_sets == 0) return ORBX_OK;
    // everything is checked before anything is enqueued
    if (set_ptr[0] < 0) return ORBX_E_BAD_ARG;
    if (nd && ((n_kf > 0 && !nd->centers) || !nd->ref_obs || (!map && (!nd->pos || !nd->normal || !nd->min_dist || !nd->max_dist)))) return ORBX_E_BAD_ARG;
    std::vector<int32_t> large;   // the sets k_distinctive_kf_large takes
    for (int s = 0; s < n_sets; s++) {
        const int32_t size = set_ptr[s + 1] - set_ptr[s];
        if (size < 0) return ORBX_E_BAD_ARG;
        if (distinct && size > kDistinctRegisterRows) large.push_back(s);
        if (nd && size > 0 && (nd->ref_obs[s] < 0 || nd->ref_obs[s] >= size)) return ORBX_E_BAD_ARG;
    }
    const size_t total = (size_t)set_ptr[n_sets];
    if (total > 0 && (!obs_kf || !obs_idx)) return ORBX_E_BAD_ARG;
    std::unique_lock<std::mutex> map_lock;   // held to the end of an update of the table
    if (map) {
        if (map->device != m->device || !set_id) return ORBX_E_BAD_ARG;
        map_lock = std::unique_lock<std::mutex>(map->mu);
        if (!map_ids_ok(map, n_sets, set_id, true)) return ORBX_E_BAD_ARG;
    }
    bool pending = false;
    for (int k = 0; k < n_kf; k++) {
        if (!kfs[k] || kfs[k]->device != m->device) return ORBX_E_BAD_ARG;
        if (nd && kfs[k]->fisheye && !nd->centers_right) return ORBX_E_BAD_ARG;
        pending |= kfs[k]->host_n() < 0;
    }
    for (size_t o = (size_t)set_ptr[0]; o < total; o++) {
        if (obs_kf[o] < 0 || obs_kf[o] >= n_kf) return ORBX_E_BAD_ARG;
        if (obs_idx[o] < 0 || obs_idx[o] >= kfs[obs_kf[o]]->rows_n()) return ORBX_E_BAD_ARG;   // (counts pending: the capacity; the kernel checks against N)
    }
    if (total == (size_t)set_ptr[0]) {   // empty sets only: nothing to compute, nothing to write
        for (int s = 0; distinct && s < n_sets; s++) best_obs[s] = -1;
        if (best_desc) memset(best_desc, 0, 32 * (size_t)n_sets);
        return ORBX_OK;
    }
    ORBX_HIP(hipSetDevice(m->device));
    std::vector<DistinctKf> recs(distinct ? (size_t)n_kf : 0);
    for (int k = 0; distinct && k < n_kf; k++) recs[k] = DistinctKf{kfs[k]->desc, kfs[k]->count, kfs[k]->roff, kfs[k]->cap, kfs[k]->fisheye ? 1 : 0, 0};
    std::vector<NormalKf> nrecs(nd ? (size_t)n_kf : 0);
    for (int k = 0; nd && k < n_kf; k++) {
        NormalKf &R = nrecs[k];
        memset(&R, 0, sizeof(R));
        R.kps = kfs[k]->kps; R.scale = kfs[k]->scale; R.count = kfs[k]->count;
        R.roff = kfs[k]->roff; R.cap = kfs[k]->cap; R.fisheye = kfs[k]->fisheye ? 1 : 0; R.nlevels = kfs[k]->nlevels;
        memcpy(R.center, nd->centers + 3 * (size_t)k, sizeof(R.center));
        if (kfs[k]->fisheye) memcpy(R.center_right, nd->centers_right + 3 * (size_t)k, sizeof(R.center_right));
    }
    DistinctSets A;
    memset(&A, 0, sizeof(A));
    A.n_kf = n_kf; A.n_sets = n_sets;
    NormalSets B;
    memset(&B, 0, sizeof(B));
    B.n_kf = n_kf; B.n_sets = n_sets;
    const int32_t *dlarge = nullptr, *dset_id = nullptr;
    int32_t *flag = nullptr, *counts_out = nullptr;
    ORBX_TRY(m->carve([&](Carve &C) {
        A.set_ptr = C.up(set_ptr, (size_t)n_sets + 1); A.obs_kf = C.up(obs_kf, total); A.obs_idx = C.up(obs_idx, total);
        if (distinct) A.kf = C.up(recs.data(), (size_t)n_kf);
        if (!large.empty()) dlarge = C.up(large.data(), large.size());
        if (map) dset_id = C.up(set_id, (size_t)n_sets);
        if (nd) {
            B.kf = C.up(nrecs.data(), (size_t)n_kf); B.ref_obs = C.up(nd->ref_obs, (size_t)n_sets);
            if (!map) B.pos = C.up(nd->pos, 3 * (size_t)n_sets);
        }
        if (distinct) A.best_obs = C.take<int32_t>(n_sets);   // (best_obs between the uploads and the flag's fill: one k_xfer launch for both)
        flag = C.take<int32_t>(4);
        if (best_desc) A.best_desc = C.take<uint8_t>(32 * (size_t)n_sets);
        if (pending) counts_out = C.take<int32_t>(2 * (size_t)n_kf);
        if (nd) { B.normal = C.take<float>(3 * (size_t)n_sets); B.min_dist = C.take<float>(n_sets); B.max_dist = C.take<float>(n_sets); }
        if (map && distinct) A.best_desc = C.take<uint8_t>(32 * (size_t)n_sets);   // (not downloaded: behind the result run)
        if (!large.empty()) A.scratch = C.take<uint8_t>(32 * total);
    }));
    A.flag = B.flag = flag;
    (distinct ? A.counts_out : B.counts_out) = counts_out;   // the first compute kernel of the chain brings the pending counts
    B.set_ptr = A.set_ptr; B.obs_kf = A.obs_kf; B.obs_idx = A.obs_idx;
    if (map) { B.rec = map->rec; B.set_id = dset_id; B.map_cap = map->capacity; }
    ORBX_HIP(m->fill(flag, 0, 16));
    ORBX_TRY(keyframe_acquire(m, kfs, n_kf));
    const unsigned grid = (unsigned)std::max((n_sets + 3) / 4, (n_kf + 255) / 256);
    if (distinct) hipLaunchKernelGGL(k_distinctive_kf, dim3(grid), dim3(256), 0, m->exec(), A);
    if (!large.empty()) hipLaunchKernelGGL(k_distinctive_kf_large, dim3((unsigned)large.size()), dim3(64 * kDistinctLargeWaves), 0, m->exec(), A, dlarge);
    if (map && map->write_seq > 0) ORBX_HIP(hipStreamWaitEvent(m->exec(), map->written, 0));   // (k_normal_depth_kf reads pos from the slots)
    if (nd) hipLaunchKernelGGL(k_normal_depth_kf, dim3(grid), dim3(256), 0, m->exec(), B);
    if (map) {
        if (nd)
            hipLaunchKernelGGL(k_map_scatter_refresh, dim3((unsigned)((n_sets + 63) / 64)), dim3(256), 0, m->exec(), map->rec, map->capacity, n_sets, dset_id,
                               A.set_ptr, (const int32_t *)flag, (const float *)B.normal, (const float *)B.min_dist, (const float *)B.max_dist,
                               (const uint8_t *)A.best_desc);
        else
            hipLaunchKernelGGL(k_map_scatter_desc, dim3((unsigned)((n_sets + 127) / 128)), dim3(256), 0, m->exec(), map->rec, map->capacity, n_sets, dset_id,
                               (const int32_t *)A.best_obs, (const int32_t *)flag, (const uint8_t *)A.best_desc);
        ORBX_HIP(hipEventRecord(map->written, m->stream));
        map->write_seq++;
    }
    ORBX_HIP(hipGetLastError());
    int32_t raised = 0;
    std::vector<int32_t> counts(pending ? 2 * (size_t)n_kf : 0);
    // an empty set is the member's early return: its entries of the caller's arrays keep their values (the arena's rows of such a set are never written)
    std::vector<std::pair<int, std::array<float, 5>>> kept;
    for (int s = 0; nd && s < n_sets; s++) {
        if (set_ptr[s + 1] > set_ptr[s]) continue;
        std::array<float, 5> v = {0, 0, 0, 0, 0};
        if (nd->normal) memcpy(v.data(), nd->normal + 3 * (size_t)s, 12);
        if (nd->min_dist) v[3] = nd->min_dist[s];
        if (nd->max_dist) v[4] = nd->max_dist[s];
        kept.emplace_back(s, v);
    }
    if (distinct) ORBX_TRY(m->d2h(best_obs, A.best_obs, 4 * (size_t)n_sets));
    ORBX_TRY(m->d2h(&raised, flag, 4));
    if (best_desc) ORBX_TRY(m->d2h(best_desc, A.best_desc, 32 * (size_t)n_sets));
    if (pending) ORBX_TRY(m->d2h(counts.data(), counts_out, 8 * (size_t)n_kf));
    if (nd && nd->normal) ORBX_TRY(m->d2h(nd->normal, B.normal, 12 * (size_t)n_sets));
    if (nd && nd->min_dist) ORBX_TRY(m->d2h(nd->min_dist, B.min_dist, 4 * (size_t)n_sets));
    if (nd && nd->max_dist) ORBX_TRY(m->d2h(nd->max_dist, B.max_dist, 4 * (size_t)n_sets));
    ORBX_TRY(m->sync_and_deliver());
    for (const auto &kv : kept) {
        if (nd->normal) memcpy(nd->normal + 3 * (size_t)kv.first, kv.second.data(), 12);
        if (nd->min_dist) nd->min_dist[kv.first] = kv.second[3];
        if (nd->max_dist) nd->max_dist[kv.first] = kv.second[4];
    }
    keyframe_release(kfs, n_kf);
    for (int k = 0; pending && k < n_kf; k++)
        if (kfs[k]->host_n() < 0) kfs[k]->adopt(counts[2 * (size_t)k], counts[2 * (size_t)k + 1]);
    if (raised) { set_error("an observation index outside [0, N) of its key frame, or a reference octave outside its pyramid"); return ORBX_E_BAD_ARG; }
    return ORBX_OK;
}

int orbx_keyframe_distinctive_descriptors(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, int n_sets, const int32_t *set_ptr, const int32_t *obs_kf,
                                          const int32_t *obs_idx, int32_t *best_obs, uint8_t *best_desc) {
    return keyframe_distinctive_impl(m, n_kf, kfs, n_sets, set_ptr, obs_kf, obs_idx, best_obs, best_desc, nullptr, nullptr);
}
int orbx_keyframe_distinctive_descriptors_to_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, int n_sets, const int32_t *set_ptr,
                                                 const int32_t *obs_kf, const int32_t *obs_idx, orbx_map *map, const int32_t *set_id, int32_t *best_obs) {
    if (!map) return ORBX_E_BAD_ARG;
    return keyframe_distinctive_impl(m, n_kf, kfs, n_sets, set_ptr, obs_kf, obs_idx, best_obs, nullptr, map, set_id);
}

// MapPoint::UpdateNormalAndDepth on resident key frames, flat / into the table / together with ComputeDistinctiveDescriptors (include/orbx.h)
int orbx_keyframe_update_normal_and_depth(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const float *centers, const float *centers_right,
                                          int n_sets, const int32_t *set_ptr, const int32_t *obs_kf, const int32_t *obs_idx, const int32_t *ref_obs,
                                          const float *pos, float *normal, float *min_dist, float *max_dist) {
    const NormalDepth nd = {centers, centers_right, ref_obs, pos, normal, min_dist, max_dist};
    return keyframe_distinctive_impl(m, n_kf, kfs, n_sets, set_ptr, obs_kf, obs_idx, nullptr, nullptr, nullptr, nullptr, &nd, false);
}
int orbx_keyframe_update_normal_and_depth_to_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const float *centers,
                                                 const float *centers_right, int n_sets, const int32_t *set_ptr, const int32_t *obs_kf,
                                                 const int32_t *obs_idx, const int32_t *ref_obs, orbx_map *map, const int32_t *set_id, float *normal,
                                                 float *min_dist, float *max_dist) {
    if (!map) return ORBX_E_BAD_ARG;
    const NormalDepth nd = {centers, centers_right, ref_obs, nullptr, normal, min_dist, max_dist};
    return keyframe_distinctive_impl(m, n_kf, kfs, n_sets, set_ptr, obs_kf, obs_idx, nullptr, nullptr, map, set_id, &nd, false);
}
int orbx_keyframe_refresh_map_points_to_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const float *centers, const float *centers_right,
                                            int n_sets, const int32_t *set_ptr, const int32_t *obs_kf, const int32_t *obs_idx,
                                            const int32_t *ref_obs, orbx_map *map, const int32_t *set_id, int32_t *best_obs) {
    if (!map) return ORBX_E_BAD_ARG;
    const NormalDepth nd = {centers, centers_right, ref_obs, nullptr, nullptr, nullptr, nullptr};
    return keyframe_distinctive_impl(m, n_kf, kfs, n_sets, set_ptr, obs_kf, obs_idx, best_obs, nullptr, map, set_id, &nd, true);
}

}  // extern "C"

namespace {

// a key frame's N where a call needs it on the host (flags are given per feature; a row of the caller's is sized by it): one orbx_keyframe_count
inline int keyframe_need_count(orbx_keyframe *kf) {
    int n = 0;
    return kf->host_n() < 0 ? orbx_keyframe_count(kf, &n) : ORBX_OK;
}

// SearchByBoW(kfs[k], F, ...) with both sides resident: A = key frame k, B = the frame handle; mode 0, of a rig mode 3 in row space (ORBmatcher.cc:283-392)
int frame_search_by_bow_resident(orbx_matcher *m, bool rig, orbx_frame *f, int n_kf, orbx_keyframe *const *kfs, const uint8_t *const *valid, float nnratio,
                                 int check_orientation, int32_t *match, int match_stride, int32_t *nmatches) {
    if (!m || !f || f->owner != m || f->fisheye != rig || !f->bow_valid || n_kf < 0) return ORBX_E_BAD_ARG;
    if (n_kf > ORBX_MAX_BOW_KEYFRAMES) return ORBX_E_TOO_LARGE;
    if (n_kf == 0) return ORBX_OK;
    if (!kfs || !match || !nmatches || match_stride < 0) return ORBX_E_BAD_ARG;
    const orbx_vocabulary *voc = f->bow.voc;
    int levelsup = f->bow.levelsup;
    for (int k = 0; k < n_kf; k++)   // every key frame is checked before anything is enqueued
        if (!keyframe_bow_ok(m, rig, kfs[k], &voc, &levelsup)) return ORBX_E_BAD_ARG;
    int n = f->host_n();
    if (n < 0 && match_stride < f->cap) { const int rc = frame_count(f, &n); if (rc != ORBX_OK) return rc; }   // the rows must fit the stride
    if (n >= 0 && match_stride < n) return ORBX_E_BAD_ARG;
    for (int k = 0; k < n_kf; k++) {
        if (valid && valid[k]) { const int rc = keyframe_need_count(kfs[k]); if (rc != ORBX_OK) return rc; }   // flags: N entries
        nmatches[k] = 0;
        for (int i = 0; i < std::max(n, 0); i++) match[(size_t)k * match_stride + i] = -1;
    }
    if (n == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(m->device));
    std::vector<BowSide> A((size_t)n_kf), B((size_t)n_kf, bow_side(f->view(), f->bow));
    for (int k = 0; k < n_kf; k++) A[k] = bow_side(kfs[k]);
    for (int k = 0; k < n_kf; k++) { const int rc = keyframe_bow_acquire(m, kfs[k]); if (rc != ORBX_OK) return rc; }
    std::vector<int32_t> counts;
    const int r = run_bow_resident(m, rig ? 3 : 0, n_kf, A.data(), B.data(), valid, nullptr, true, nnratio, check_orientation, nullptr, nullptr, 0, match,
                                   match_stride, nmatches, counts, rig);
    if (r != ORBX_OK) return r;
    for (int k = 0; k < n_kf; k++) {
        keyframe_bow_release(kfs[k]);
        keyframe_adopt(kfs[k], &counts[4 * (size_t)k]);
    }
    if (!f->n_known) f->adopt(counts[2], counts[3]);
    return ORBX_OK;
}

// SearchByBoW(pKF1, kfs2[k], ...) (ORBmatcher.cc:765-905) with both sides resident: mode 1, A = kf1 for every problem, B = kfs2[k].  Between rig key
// frames the reference skips the right camera's features as queries and as candidates (:800-802, :820-822): the same mode on the same kernels with
// those rows switched off (run_bow_resident).
int keyframe_search_by_bow(orbx_matcher *m, bool rig, orbx_keyframe *kf1, const uint8_t *valid1, int n_kf, orbx_keyframe *const *kfs2,
                           const uint8_t *const *valid2, float nnratio, int check_orientation, int32_t *match12, int match_stride, int32_t *nmatches) {
    if (!m || n_kf < 0) return ORBX_E_BAD_ARG;
    const orbx_vocabulary *voc = nullptr;
    int levelsup = 0;
    if (!keyframe_bow_ok(m, rig, kf1, &voc, &levelsup)) return ORBX_E_BAD_ARG;
    if (n_kf > ORBX_MAX_BOW_KEYFRAMES) return ORBX_E_TOO_LARGE;
    if (n_kf == 0) return ORBX_OK;
    if (!kfs2 || !match12 || !nmatches || match_stride < 0) return ORBX_E_BAD_ARG;
    for (int k = 0; k < n_kf; k++)
        if (!keyframe_bow_ok(m, rig, kfs2[k], &voc, &levelsup)) return ORBX_E_BAD_ARG;
    int n1 = kf1->host_n();
    if (n1 < 0 && (match_stride < kf1->cap || valid1)) { const int rc = orbx_keyframe_count(kf1, &n1); if (rc != ORBX_OK) return rc; }
    if (n1 >= 0 && match_stride < n1) return ORBX_E_BAD_ARG;
    for (int k = 0; k < n_kf; k++) {
        if (valid2 && valid2[k]) { const int rc = keyframe_need_count(kfs2[k]); if (rc != ORBX_OK) return rc; }
        nmatches[k] = 0;
        for (int i = 0; i < std::max(n1, 0); i++) match12[(size_t)k * match_stride + i] = -1;
    }
    if (n1 == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(m->device));
    std::vector<BowSide> A((size_t)n_kf, bow_side(kf1)), B((size_t)n_kf);
    std::vector<const uint8_t *> fa((size_t)n_kf, valid1);
    for (int k = 0; k < n_kf; k++) B[k] = bow_side(kfs2[k]);
    int rc = keyframe_bow_acquire(m, kf1);
    for (int k = 0; k < n_kf && rc == ORBX_OK; k++) rc = keyframe_bow_acquire(m, kfs2[k]);
    if (rc != ORBX_OK) return rc;
    std::vector<int32_t> counts;
    const int r = run_bow_resident(m, 1, n_kf, A.data(), B.data(), fa.data(), valid2, true, nnratio, check_orientation, nullptr, nullptr, 0, match12,
                                   match_stride, nmatches, counts, rig);
    if (r != ORBX_OK) return r;
    keyframe_bow_release(kf1);
    keyframe_adopt(kf1, &counts[0]);
    for (int k = 0; k < n_kf; k++) {
        keyframe_bow_release(kfs2[k]);
        keyframe_adopt(kfs2[k], &counts[4 * (size_t)k + 2]);
    }
    return ORBX_OK;
}

// SearchForTriangulation (ORBmatcher.cc:907-1146) between two resident key frames of one kind, mode 2.  Pinhole: the gates of
// orbx_search_for_triangulation_pinhole (G with the key frames' rows filled in here).  A rig: KannalaBrandt8::epipolarConstrain in k_tri_kb8_resident
// (K; NULL = bCoarse: no gate at all, :1026, :1036).  Keypoints and scale factors are the key frames' own rows; the level tables ride up beside the record.
int keyframe_search_for_triangulation(orbx_matcher *m, bool rig, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                      int check_orientation, TriGate *G, Kb8Gate *K, const float *sigma2_1, const float *sigma2_2, int nlevels,
                                      int32_t *matches12, NewPointsCall *tri = nullptr) {
    const orbx_vocabulary *voc = nullptr;
    int levelsup = 0;
    if (!keyframe_bow_ok(m, rig, kf1, &voc, &levelsup) || !keyframe_bow_ok(m, rig, kf2, &voc, &levelsup)) return ORBX_E_BAD_ARG;
    if (nlevels != kf2->nlevels || (K && nlevels != kf1->nlevels)) return ORBX_E_BAD_ARG;
    int n1 = 0, n2 = kf2->host_n();
    int rc = orbx_keyframe_count(kf1, &n1);   // matches12 holds N1 entries: N1 has to be known here
    if (rc == ORBX_OK && skip2 && n2 < 0) rc = orbx_keyframe_count(kf2, &n2);
    if (rc != ORBX_OK) return rc;
    if (n1 > 0 && !matches12) return ORBX_E_BAD_ARG;
    if (tri) { tri->matches.resize((size_t)n1); matches12 = tri->matches.data(); }   // (the caller's row is written with pos and status, or not at all)
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    if (n1 == 0 || n2 == 0) return 0;
    ORBX_HIP(hipSetDevice(m->device));
    if (G) { G->k1 = kf1->kps; G->k2 = kf2->kps; G->ur1 = kf1->u_right; G->ur2 = kf2->u_right; G->scale2 = kf2->scale; }
    if (K) { K->n_left1 = kf1->roff; K->n_left2 = kf2->roff; }   // row space: a row >= roff is the right camera's
    const BowSide A = bow_side(kf1), B = bow_side(kf2);
    if ((rc = keyframe_bow_acquire(m, kf1)) != ORBX_OK || (rc = keyframe_bow_acquire(m, kf2)) != ORBX_OK) return rc;
    std::vector<int32_t> counts;
    int32_t nm = 0;
    const int r = run_bow_resident(m, 2, 1, &A, &B, &skip1, &skip2, false, 0.f, check_orientation, G, sigma2_2, nlevels, matches12, n1, &nm, counts, rig, K,
                                   sigma2_1, tri);
    if (r != ORBX_OK) return r;
    keyframe_bow_release(kf1); keyframe_bow_release(kf2);
    keyframe_adopt(kf2, &counts[2]);
    return nm;
}

// The two public searches' gates, each built once for the plain call and the one that triangulates behind it (tri).
int search_for_triangulation_pinhole(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                     int check_orientation, const orbx_keyframe_gate *gate, int32_t *matches12, NewPointsCall *tri) {
    if (!m || !gate || !gate->level_sigma2_2) return ORBX_E_BAD_ARG;
    TriGate G;
    memset(&G, 0, sizeof(G));
    G.enabled = 1; G.coarse = gate->coarse ? 1 : 0; G.strict = gate->strict_fp ? 1 : 0;
    for (int i = 0; i < 9; i++) G.F[i] = gate->F12[i];
    G.ex = gate->ep_x; G.ey = gate->ep_y;
    return keyframe_search_for_triangulation(m, false, kf1, kf2, skip1, skip2, check_orientation, &G, nullptr, nullptr, gate->level_sigma2_2, gate->nlevels,
                                             matches12, tri);
}
int search_for_triangulation_rig(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                 int check_orientation, const orbx_keyframe_kb8_gate *gate, int32_t *matches12, NewPointsCall *tri) {
    if (!m || !gate) return ORBX_E_BAD_ARG;
    if (gate->coarse)   // bCoarse: no gate at all for such key frames, plain mode 2
        return keyframe_search_for_triangulation(m, true, kf1, kf2, skip1, skip2, check_orientation, nullptr, nullptr, nullptr, nullptr,
                                                 kf2 ? kf2->nlevels : 0, matches12, tri);
    if (!gate->level_sigma2_1 || !gate->level_sigma2_2) return ORBX_E_BAD_ARG;
    TriGate G;
    memset(&G, 0, sizeof(G));
    G.enabled = 1; G.strict = 1;
    Kb8Gate K;
    memset(&K, 0, sizeof(K));
    memcpy(K.cam[0], gate->cam1, sizeof(float) * 16);
    memcpy(K.cam[2], gate->cam2, sizeof(float) * 16);
    memcpy(K.R12, gate->R12, sizeof(K.R12));
    memcpy(K.t12, gate->t12, sizeof(K.t12));
    return keyframe_search_for_triangulation(m, true, kf1, kf2, skip1, skip2, check_orientation, &G, &K, gate->level_sigma2_1, gate->level_sigma2_2,
                                             gate->nlevels, matches12, tri);
}

// orbx_keyframe_search_and_triangulate[_fisheye]: the search with k_new_points behind it (run_bow_resident's tri); gate: the kind's gate struct
int keyframe_search_and_triangulate(orbx_matcher *m, bool rig, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                    int check_orientation, const void *gate, const void *views1, const void *views2, const orbx_new_points_params *par,
                                    const orbx_new_points_stereo *st, bool stereo, int32_t *matches12, float *pos, uint8_t *status, int *n_accepted) {
    if (!matches12 || !pos || !status) return ORBX_E_BAD_ARG;
    NewPointsCall T;
    ORBX_TRY(new_points_prepare(m, rig, kf1, kf2, views1, views2, par, st, stereo, T));
    const int nm = rig ? search_for_triangulation_rig(m, kf1, kf2, skip1, skip2, check_orientation, static_cast<const orbx_keyframe_kb8_gate *>(gate), matches12, &T)
                       : search_for_triangulation_pinhole(m, kf1, kf2, skip1, skip2, check_orientation, static_cast<const orbx_keyframe_gate *>(gate), matches12, &T);
    if (nm < 0) return nm;
    const int n1 = (int)T.matches.size();
    ORBX_TRY(T.deliver(n1, pos, status, n_accepted));
    if (n1 > 0) memcpy(matches12, T.matches.data(), 4 * (size_t)n1);
    return nm;
}

// orbx_keyframe_triangulate_pairs[_fisheye]: k_new_points over pairs the host names.  One upload run (idx1, idx2, the two level tables, the record), one
// launch, one download run (pos, status, the flag and the counts as the kernel read them), one synchronisation.
int keyframe_triangulate_pairs(orbx_matcher *m, bool rig, orbx_keyframe *kf1, orbx_keyframe *kf2, const void *views1, const void *views2,
                               const orbx_new_points_params *par, const orbx_new_points_stereo *st, bool stereo, int n_pairs, const int32_t *idx1,
                               const int32_t *idx2, float *pos, uint8_t *status, int *n_accepted) {
    NewPointsCall T;
    ORBX_TRY(new_points_prepare(m, rig, kf1, kf2, views1, views2, par, st, stereo, T));
    if (n_pairs < 0 || (n_pairs > 0 && (!idx1 || !idx2 || !pos || !status))) return ORBX_E_BAD_ARG;
    const int b1 = kf1->rows_n(), b2 = kf2->rows_n();   // (counts pending: the capacity; the kernel checks against N)
    for (int p = 0; p < n_pairs; p++)
        if (idx1[p] < 0 || idx1[p] >= b1 || idx2[p] < -1 || idx2[p] >= b2) return ORBX_E_BAD_ARG;
    if (n_pairs == 0) { if (n_accepted) *n_accepted = 0; return ORBX_OK; }
    ORBX_HIP(hipSetDevice(m->device));
    const int32_t *d1 = nullptr, *d2 = nullptr;
    ORBX_TRY(m->carve([&](Carve &C) {
        d1 = C.up(idx1, (size_t)n_pairs); d2 = C.up(idx2, (size_t)n_pairs);
        T.carve_up(C, false, false, nullptr, nullptr);
        T.carve_out(C, n_pairs);
    }));
    orbx_keyframe *kfs[2] = {kf1, kf2};
    const bool pending = kf1->host_n() < 0 || kf2->host_n() < 0;
    ORBX_TRY(T.stage(m, d1, d2, n_pairs, pending));
    ORBX_TRY(keyframe_acquire(m, kfs, 2));
    T.launch(m, rig, n_pairs);
    ORBX_HIP(hipGetLastError());
    ORBX_TRY(T.fetch(m, n_pairs));
    ORBX_TRY(m->sync_and_deliver());
    keyframe_release(kfs, 2);
    for (int k = 0; pending && k < 2; k++)
        if (kfs[k]->host_n() < 0) kfs[k]->adopt(T.flag[4 + 2 * k], T.flag[5 + 2 * k]);
    return T.deliver(n_pairs, pos, status, n_accepted);
}

}  // namespace

extern "C" {

int orbx_frame_search_by_bow_resident(orbx_matcher *m, orbx_frame *f, int n_kf, orbx_keyframe *const *kfs, const uint8_t *const *valid, float nnratio,
                                      int check_orientation, int32_t *match, int match_stride, int32_t *nmatches) {
    return frame_search_by_bow_resident(m, false, f, n_kf, kfs, valid, nnratio, check_orientation, match, match_stride, nmatches);
}
int orbx_frame_search_by_bow_resident_fisheye(orbx_matcher *m, orbx_frame *f, int n_kf, orbx_keyframe *const *kfs, const uint8_t *const *valid,
                                              float nnratio, int check_orientation, int32_t *match, int match_stride, int32_t *nmatches) {
    return frame_search_by_bow_resident(m, true, f, n_kf, kfs, valid, nnratio, check_orientation, match, match_stride, nmatches);
}

int orbx_keyframe_search_by_bow(orbx_matcher *m, orbx_keyframe *kf1, const uint8_t *valid1, int n_kf, orbx_keyframe *const *kfs2,
                                const uint8_t *const *valid2, float nnratio, int check_orientation, int32_t *match12, int match_stride, int32_t *nmatches) {
    return keyframe_search_by_bow(m, false, kf1, valid1, n_kf, kfs2, valid2, nnratio, check_orientation, match12, match_stride, nmatches);
}
int orbx_keyframe_search_by_bow_fisheye(orbx_matcher *m, orbx_keyframe *kf1, const uint8_t *valid1, int n_kf, orbx_keyframe *const *kfs2,
                                        const uint8_t *const *valid2, float nnratio, int check_orientation, int32_t *match12, int match_stride,
                                        int32_t *nmatches) {
    return keyframe_search_by_bow(m, true, kf1, valid1, n_kf, kfs2, valid2, nnratio, check_orientation, match12, match_stride, nmatches);
}

int orbx_keyframe_search_for_triangulation(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                           int check_orientation, const orbx_keyframe_gate *gate, int32_t *matches12) {
    return search_for_triangulation_pinhole(m, kf1, kf2, skip1, skip2, check_orientation, gate, matches12, nullptr);
}
int orbx_keyframe_search_for_triangulation_fisheye(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                                   int check_orientation, const orbx_keyframe_kb8_gate *gate, int32_t *matches12) {
    return search_for_triangulation_rig(m, kf1, kf2, skip1, skip2, check_orientation, gate, matches12, nullptr);
}

// LocalMapping::CreateNewMapPoints' triangulation on resident key frames (include/orbx.h), over named pairs or behind the search
int orbx_keyframe_triangulate_pairs(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const orbx_new_points_view *view1,
                                    const orbx_new_points_view *view2, const orbx_new_points_params *par, int n_pairs, const int32_t *idx1,
                                    const int32_t *idx2, float *pos, uint8_t *status, int *n_accepted) {
    return keyframe_triangulate_pairs(m, false, kf1, kf2, view1, view2, par, nullptr, false, n_pairs, idx1, idx2, pos, status, n_accepted);
}
int orbx_keyframe_triangulate_pairs_stereo(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const orbx_new_points_view *view1,
                                           const orbx_new_points_view *view2, const orbx_new_points_params *par, const orbx_new_points_stereo *st,
                                           int n_pairs, const int32_t *idx1, const int32_t *idx2, float *pos, uint8_t *status, int *n_accepted) {
    return keyframe_triangulate_pairs(m, false, kf1, kf2, view1, view2, par, st, true, n_pairs, idx1, idx2, pos, status, n_accepted);
}
int orbx_keyframe_triangulate_pairs_fisheye(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const orbx_fisheye_view *views1,
                                            const orbx_fisheye_view *views2, const orbx_new_points_params *par, int n_pairs, const int32_t *idx1,
                                            const int32_t *idx2, float *pos, uint8_t *status, int *n_accepted) {
    return keyframe_triangulate_pairs(m, true, kf1, kf2, views1, views2, par, nullptr, false, n_pairs, idx1, idx2, pos, status, n_accepted);
}
int orbx_keyframe_search_and_triangulate(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                         int check_orientation, const orbx_keyframe_gate *gate, const orbx_new_points_view *view1,
                                         const orbx_new_points_view *view2, const orbx_new_points_params *par, int32_t *matches12, float *pos,
                                         uint8_t *status, int *n_accepted) {
    return keyframe_search_and_triangulate(m, false, kf1, kf2, skip1, skip2, check_orientation, gate, view1, view2, par, nullptr, false, matches12, pos, status,
                                           n_accepted);
}
int orbx_keyframe_search_and_triangulate_stereo(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                                int check_orientation, const orbx_keyframe_gate *gate, const orbx_new_points_view *view1,
                                                const orbx_new_points_view *view2, const orbx_new_points_params *par, const orbx_new_points_stereo *st,
                                                int32_t *matches12, float *pos, uint8_t *status, int *n_accepted) {
    return keyframe_search_and_triangulate(m, false, kf1, kf2, skip1, skip2, check_orientation, gate, view1, view2, par, st, true, matches12, pos, status,
                                           n_accepted);
}
int orbx_keyframe_search_and_triangulate_fisheye(orbx_matcher *m, orbx_keyframe *kf1, orbx_keyframe *kf2, const uint8_t *skip1, const uint8_t *skip2,
                                                 int check_orientation, const orbx_keyframe_kb8_gate *gate, const orbx_fisheye_view *views1,
                                                 const orbx_fisheye_view *views2, const orbx_new_points_params *par, int32_t *matches12, float *pos,
                                                 uint8_t *status, int *n_accepted) {
    return keyframe_search_and_triangulate(m, true, kf1, kf2, skip1, skip2, check_orientation, gate, views1, views2, par, nullptr, false, matches12, pos, status,
                                           n_accepted);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// LoopClosing's Sim3 projection searches on resident key frames: both SearchByProjection(KeyFrame*, Sim3f&, ...) overloads (ORBmatcher.cc:427-532,
// :534-646) for K key frames with one shared point set, and SearchAndFuse's loop of Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:1339-1455).  The
// gates run on the device (k_kf_project<., true>); the searches are the existing kernels: k_window_best2_t + the replay of the query loop over n_kf problems
// for the first, k_window_best1_kf through keyframe_fuse_map_points_impl for the second.  The _fisheye twins run the same on the LEFT side of rig key
// frames (KannalaBrandt8::project, or the written-out pinhole form of the second overload).
// ---------------------------------------------------------------------------------------------------------
namespace {

// Both kinds of key frame through one body, the kind being `fisheye`: cams + poses [n_kf], or views [n_kf] on
// the LEFT side of a rig key frame (the members read nothing else: GetFeaturesInArea with bRight = false, mvKeysUn[idx], mpCamera) -- the left
// keyframe_problem, N_left features for the replay, while the caller's match / occupied rows span N = N_left + N_right as vpMatched does.
int keyframe_search_by_projection_sim3_impl(orbx_matcher *m, bool fisheye, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams,
                                            const orbx_frame_pose *poses, const orbx_fisheye_view *views, float th, float ratio_hamming,
                                            float log_scale_factor, int projection_form, const MapPoints &src, const uint8_t *skip,
                                            const uint8_t *const *occupied, int32_t *const *match, int32_t *nmatches, uint8_t *projected, float *proj_u,
                                            float *proj_v) {
    const int n_mp = src.n;
    if (!m || n_kf < 0 || n_mp < 0 || (n_kf > 0 && (!kfs || (fisheye ? !views : !cams || !poses) || !match || !nmatches))) return ORBX_E_BAD_ARG;
    if ((projection_form != ORBX_SIM3_PROJECT_CAMERA && projection_form != ORBX_SIM3_PROJECT_INVZ) || (proj_u == nullptr) != (proj_v == nullptr))
        return ORBX_E_BAD_ARG;
    if (n_kf > ORBX_MAX_FUSE_KEYFRAMES) return ORBX_E_TOO_LARGE;
    const size_t np = (size_t)n_mp, total = (size_t)n_kf * np;
    if (total > 0 && !map_points_ok(m, src)) return ORBX_E_BAD_ARG;
    for (int k = 0; k < n_kf; k++) {
        if (!kfs[k] || kfs[k]->fisheye != fisheye || kfs[k]->device != m->device || !match[k]) return ORBX_E_BAD_ARG;
        // k_window_best2_t and the replay take ONE GridParams per launch: the key frames of a call share their image bounds, bit for bit
        if (memcmp(kfs[k]->bounds, kfs[0]->bounds, sizeof(kfs[0]->bounds)) != 0) return ORBX_E_BAD_ARG;
    }
    int nc = 0;   // the rows of match / occupied hold N_k entries: the counts are needed here (cached since the caller sized the rows)
    std::vector<int> ns((size_t)n_kf, 0);   // the features the search sees: N, of a rig N_left (a match row's entries [N_left, N) stay -1)
    for (int k = 0; k < n_kf; k++) {
        const int rc = keyframe_need_count(kfs[k]);
        if (rc != ORBX_OK) return rc;
        ns[(size_t)k] = fisheye ? kfs[k]->host_left() : kfs[k]->host_n();
        nc = std::max(nc, ns[(size_t)k]);
    }
    if (nc > kMaxResolveFeatures) return ORBX_E_TOO_LARGE;   // before anything is enqueued: the replay keeps 10 B per feature in LDS
    for (int k = 0; k < n_kf; k++) {
        for (int i = 0; i < kfs[k]->host_n(); i++) match[k][i] = -1;
        nmatches[k] = 0;
    }
    if (total == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(m->device));
    const int32_t cnt4[4] = {n_mp, 0, 0, 0};
    float *qx, *qy, *qr;
    uint8_t *dskip, *qvalid;
    MapPointsDev D;
    int32_t *dcnt, *qmin, *qmax, *dmeta, *dentries, *dnm;
    orbx_camera *dcam;
    orbx_frame_pose *dpose;
    FisheyeView *dview;
    KfProblem *dK;
    WindowProblem *dP;
    ResolveProblem *dR;
    u64 *dkeys;
    std::vector<const uint8_t *> docc((size_t)n_kf, nullptr);
    std::vector<int32_t *> dmatch((size_t)n_kf, nullptr);
    ORBX_TRY(m->carve([&](Carve &A) {
        // uploads, adjacent in the arena (one run): the map points ONCE, then what grows with n_kf -- cameras, poses, skip and occupancy rows, records
        D = map_points_up(A, src);
        dcnt = A.up(cnt4, 4);
        dcam = fisheye ? nullptr : A.up(cams, (size_t)n_kf); dpose = fisheye ? nullptr : A.up(poses, (size_t)n_kf);
        dview = fisheye ? A.up(reinterpret_cast<const FisheyeView *>(views), (size_t)n_kf) : nullptr;
        dskip = A.up_opt(skip, total);
        for (int k = 0; k < n_kf; k++)
            if (occupied && occupied[k] && ns[(size_t)k] > 0) docc[(size_t)k] = A.up(occupied[k], (size_t)ns[(size_t)k]);
        dK = A.take<KfProblem>(n_kf); dP = A.take<WindowProblem>(n_kf); dR = A.take<ResolveProblem>(n_kf);
        // written by k_kf_project and the window scan, read by the scan and the replay: device only
        qr = A.take<float>(total); qmin = A.take<int32_t>(total); qmax = A.take<int32_t>(total);
        dkeys = A.take<u64>(total * kTopK); dmeta = A.take<int32_t>(total); dentries = A.take<int32_t>(total);
        // the downloads side by side (one run): the projections, the gates' verdicts, the match rows, nmatches
        qx = A.take<float>(total); qy = A.take<float>(total); qvalid = A.take<uint8_t>(total);
        for (int k = 0; k < n_kf; k++) dmatch[(size_t)k] = A.take<int32_t>((size_t)std::max(ns[(size_t)k], 1));
        dnm = A.take<int32_t>(n_kf);
    }));
    std::vector<KfProblem> K((size_t)n_kf);
    std::vector<WindowProblem> P((size_t)n_kf);
    std::vector<ResolveProblem> R((size_t)n_kf);
    for (int k = 0; k < n_kf; k++) {
        const size_t o = (size_t)k * np;
        keyframe_problem(kfs[k], false, 0, &K[(size_t)k]);   // bounds, levels and scale factors for the projection; the window problem of key frame k:
        WindowProblem &W = K[(size_t)k].P;
        W.occupied0 = docc[(size_t)k];
        W.qx = qx + o; W.qy = qy + o; W.qr = qr + o; W.qmin = qmin + o; W.qmax = qmax + o; W.qvalid = qvalid + o;
        W.qdesc = D.desc; W.nq_ptr = dcnt;
        W.keys = dkeys + o * kTopK; W.meta = dmeta + o;
        P[(size_t)k] = W;
        ResolveProblem &Q = R[(size_t)k];
        memset(&Q, 0, sizeof(Q));
        Q.mode = 2; Q.max_dist = (float)ORBX_TH_LOW * ratio_hamming; Q.cleared_value = -2;   // the window form: no ratio test, no rotation check
        Q.match = dmatch[(size_t)k]; Q.nmatches = dnm + k; Q.entries = dentries + o;
    }
    ORBX_TRY(m->h2d(dK, K.data(), sizeof(KfProblem) * (size_t)n_kf));
    ORBX_TRY(m->h2d(dP, P.data(), sizeof(WindowProblem) * (size_t)n_kf));
    ORBX_TRY(m->h2d(dR, R.data(), sizeof(ResolveProblem) * (size_t)n_kf));
    ORBX_TRY(keyframe_acquire(m, kfs, n_kf));
    uint64_t seq = 0;
    ORBX_TRY(map_points_gather(m, src, D, &seq));
    launch_kf_project(m->exec(), fisheye, true, n_kf,
                      KfProject{dK, dcam, dpose, dview, th, log_scale_factor, projection_form, n_mp, 1, D.pos, D.normal, D.min_dist, D.max_dist, dskip, qx, qy,
                                nullptr, qr, qmin, qmax, qvalid});
    const GridParams g = grid_of(kfs[0]->bounds);
    ORBX_LAUNCH_WINDOW_BEST2(n_mp, n_kf, m->exec(), (const WindowProblem *)dP, g);
    { const int rr = launch_resolve<false>(n_kf, m->exec(), dP, dR, g, nc, n_mp, 4); if (rr != ORBX_OK) return rr; }
    ORBX_HIP(hipGetLastError());
    if (proj_u) { ORBX_TRY(m->d2h(proj_u, qx, 4 * total)); ORBX_TRY(m->d2h(proj_v, qy, 4 * total)); }
    if (projected) ORBX_TRY(m->d2h(projected, qvalid, total));
    for (int k = 0; k < n_kf; k++) ORBX_TRY(m->d2h(match[k], dmatch[(size_t)k], 4 * (size_t)ns[(size_t)k]));
    ORBX_TRY(m->d2h(nmatches, dnm, 4 * (size_t)n_kf));
    ORBX_TRY(m->sync_and_deliver());
    keyframe_release(kfs, n_kf);
    map_points_done(src, seq);
    return ORBX_OK;
}

}  // namespace

extern "C" int orbx_keyframe_search_by_projection_sim3(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams,
                                                       const orbx_frame_pose *poses, float th, float ratio_hamming, float log_scale_factor,
                                                       int projection_form, int n_mp, const float *pos, const float *normal, const float *min_dist,
                                                       const float *max_dist, const uint8_t *mp_desc, const uint8_t *skip,
                                                       const uint8_t *const *occupied, int32_t *const *match, int32_t *nmatches, uint8_t *projected,
                                                       float *proj_u, float *proj_v) {
    return keyframe_search_by_projection_sim3_impl(m, false, n_kf, kfs, cams, poses, nullptr, th, ratio_hamming, log_scale_factor, projection_form,
                                                   MapPoints{n_mp, pos, normal, min_dist, max_dist, mp_desc, nullptr, nullptr}, skip, occupied, match, nmatches,
                                                   projected, proj_u, proj_v);
}
extern "C" int orbx_keyframe_search_by_projection_sim3_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams,
                                                           const orbx_frame_pose *poses, float th, float ratio_hamming, float log_scale_factor,
                                                           int projection_form, int n_mp, orbx_map *map, const int32_t *ids, const uint8_t *skip,
                                                           const uint8_t *const *occupied, int32_t *const *match, int32_t *nmatches, uint8_t *projected,
                                                           float *proj_u, float *proj_v) {
    if (!map_form_ok(map, n_mp)) return ORBX_E_BAD_ARG;
    return keyframe_search_by_projection_sim3_impl(m, false, n_kf, kfs, cams, poses, nullptr, th, ratio_hamming, log_scale_factor, projection_form,
                                                   map_points_of(n_mp, map, ids), skip, occupied, match, nmatches, projected, proj_u, proj_v);
}

extern "C" int orbx_keyframe_search_by_projection_sim3_fisheye(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fisheye_view *views,
                                                               float th, float ratio_hamming, float log_scale_factor, int projection_form, int n_mp,
                                                               const float *pos, const float *normal, const float *min_dist, const float *max_dist,
                                                               const uint8_t *mp_desc, const uint8_t *skip, const uint8_t *const *occupied,
                                                               int32_t *const *match, int32_t *nmatches, uint8_t *projected, float *proj_u,
                                                               float *proj_v) {
    return keyframe_search_by_projection_sim3_impl(m, true, n_kf, kfs, nullptr, nullptr, views, th, ratio_hamming, log_scale_factor, projection_form,
                                                   MapPoints{n_mp, pos, normal, min_dist, max_dist, mp_desc, nullptr, nullptr}, skip, occupied, match, nmatches,
                                                   projected, proj_u, proj_v);
}
extern "C" int orbx_keyframe_search_by_projection_sim3_fisheye_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fisheye_view *views,
                                                                   float th, float ratio_hamming, float log_scale_factor, int projection_form, int n_mp,
                                                                   orbx_map *map, const int32_t *ids, const uint8_t *skip,
                                                                   const uint8_t *const *occupied, int32_t *const *match, int32_t *nmatches,
                                                                   uint8_t *projected, float *proj_u, float *proj_v) {
    if (!map_form_ok(map, n_mp)) return ORBX_E_BAD_ARG;
    return keyframe_search_by_projection_sim3_impl(m, true, n_kf, kfs, nullptr, nullptr, views, th, ratio_hamming, log_scale_factor, projection_form,
                                                   map_points_of(n_mp, map, ids), skip, occupied, match, nmatches, projected, proj_u, proj_v);
}

extern "C" int orbx_keyframe_fuse_map_points_sim3_fisheye(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fisheye_view *views, float th,
                                                          float log_scale_factor, int n_mp, const float *pos, const float *normal,
                                                          const float *min_dist, const float *max_dist, const uint8_t *mp_desc, const uint8_t *skip,
                                                          int32_t *best_idx, int32_t *best_dist, uint8_t *projected) {
    return keyframe_fuse_map_points_impl(m, true, true, n_kf, kfs, nullptr, nullptr, views, th, log_scale_factor, 0,
                                         MapPoints{n_mp, pos, normal, min_dist, max_dist, mp_desc, nullptr, nullptr}, skip, best_idx, best_dist, projected);
}
extern "C" int orbx_keyframe_fuse_map_points_sim3_fisheye_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_fisheye_view *views,
                                                              float th, float log_scale_factor, int n_mp, orbx_map *map, const int32_t *ids,
                                                              const uint8_t *skip, int32_t *best_idx, int32_t *best_dist, uint8_t *projected) {
    if (!map_form_ok(map, n_mp)) return ORBX_E_BAD_ARG;
    return keyframe_fuse_map_points_impl(m, true, true, n_kf, kfs, nullptr, nullptr, views, th, log_scale_factor, 0, map_points_of(n_mp, map, ids), skip,
                                         best_idx, best_dist, projected);
}

extern "C" int orbx_keyframe_fuse_map_points_sim3(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams,
                                                  const orbx_frame_pose *poses, float th, float log_scale_factor, int n_mp, const float *pos,
                                                  const float *normal, const float *min_dist, const float *max_dist, const uint8_t *mp_desc,
                                                  const uint8_t *skip, int32_t *best_idx, int32_t *best_dist, uint8_t *projected) {
    return keyframe_fuse_map_points_impl(m, false, true, n_kf, kfs, cams, poses, nullptr, th, log_scale_factor, 0,
                                         MapPoints{n_mp, pos, normal, min_dist, max_dist, mp_desc, nullptr, nullptr}, skip, best_idx, best_dist, projected);
}
extern "C" int orbx_keyframe_fuse_map_points_sim3_map(orbx_matcher *m, int n_kf, orbx_keyframe *const *kfs, const orbx_camera *cams,
                                                      const orbx_frame_pose *poses, float th, float log_scale_factor, int n_mp, orbx_map *map,
                                                      const int32_t *ids, const uint8_t *skip, int32_t *best_idx, int32_t *best_dist,
                                                      uint8_t *projected) {
    if (!map_form_ok(map, n_mp)) return ORBX_E_BAD_ARG;
    return keyframe_fuse_map_points_impl(m, false, true, n_kf, kfs, cams, poses, nullptr, th, log_scale_factor, 0, map_points_of(n_mp, map, ids), skip,
                                         best_idx, best_dist, projected);
}

// ---------------------------------------------------------------------------------------------------------
// The Tracking thread's two searches whose queries are another frame's map points, from map ids: TrackWithMotionModel's SearchByProjection(Cur, Last,
// th, bMono) and Relocalization's SearchByProjection(Cur, pKF, sAlreadyFound, th, ORBdist) on a monocular / rectified resident frame.  ids [n_ids] =
// the map slot of the source's mvpMapPoints[i] or -1; k_track_project evaluates the adapters' host loops on the device and writes the query records
// into the arena of run_projection's handle form, which runs unchanged behind it: the same window scan, the same replay, one launch more.  A match
// value >= 0 is the SOURCE feature index.  Everything is checked before anything is enqueued.
// ---------------------------------------------------------------------------------------------------------
namespace {

// the checks all four forms share; fisheye: the kind of the form (cur must be of it); have_view: the form's camera arguments are there; n_src: the
// source's count where the host knows it (-1: pending), cap_src: its capacity
int track_check(orbx_matcher *m, orbx_frame *cur, bool fisheye, bool have_view, orbx_map *map, int n_ids, const int32_t *ids, int n_src, int cap_src,
                const int32_t *match, const float *proj_u, const float *proj_v) {
    if (!m || !cur || !have_view || !map || !match || n_ids < 0 || (n_ids > 0 && !ids)) return ORBX_E_BAD_ARG;
    if (cur->owner != m || cur->fisheye != fisheye || !cur->loaded || map->device != m->device || (proj_u == nullptr) != (proj_v == nullptr))
        return ORBX_E_BAD_ARG;
    if (n_src >= 0 ? n_ids != n_src : n_ids > cap_src) return ORBX_E_BAD_ARG;   // one entry per feature of the source
    if (cur->rows_n() > kMaxResolveFeatures) return ORBX_E_TOO_LARGE;
    std::lock_guard<std::mutex> lock(map->mu);
    return map_ids_ok(map, n_ids, ids, false, true) ? ORBX_OK : ORBX_E_BAD_ARG;
}

// twin: the rig form of TrackWithMotionModel's search (both cameras, k_replay_twin); left_only: the rig form of Relocalization's (the left camera)
int track_run(orbx_matcher *m, orbx_frame *cur, const uint8_t *occupied, TrackArgs &tr, int n_ids, const uint8_t *has_obs, float max_dist,
              int check_orientation, int32_t *match, bool twin = false, bool left_only = false) {
    if (tr.projected) memset(tr.projected, 0, (size_t)n_ids);
    if (tr.proj_u) { memset(tr.proj_u, 0, 4 * (size_t)n_ids); memset(tr.proj_v, 0, 4 * (size_t)n_ids); }
    TrackArgs::Out out = {0, false};
    tr.out = &out;
    const orbx_frame_desc d = frame_desc_of(cur);
    int nm;
    if (twin) {
        TwinArgs a = {&d, nullptr, 0, nullptr, nullptr, occupied, n_ids, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr},
                      {nullptr, nullptr}, {nullptr, nullptr}, nullptr, has_obs, nullptr, 2, 0.f, check_orientation, match, &tr};
        nm = run_projection_twin(m, a, cur);
    } else {
        ProjArgs a = {&d, occupied, n_ids, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, has_obs, nullptr, 2, 0.f,
                      check_orientation, match, max_dist, &tr};
        nm = run_projection(m, a, cur, left_only);
    }
    if (nm >= 0 && out.waited) {   // the call made its waits and has synchronised behind them
        map_points_done(map_points_of(n_ids, tr.map, tr.ids), out.seq);
        if (tr.kf) keyframe_release(&tr.kf, 1);
    }
    return nm;
}

}  // namespace

extern "C" int orbx_frame_track_last_frame_map(orbx_matcher *m, orbx_frame *cur, orbx_frame *last, const uint8_t *cur_occupied, const orbx_camera *cam,
                                               const orbx_frame_pose *pose, orbx_map *map, int n_ids, const int32_t *ids, const uint8_t *has_obs,
                                               float th, int level_mode, int check_orientation, int32_t *cur_match, uint8_t *projected, float *proj_u,
                                               float *proj_v) {
    if (!last || last == cur || last->owner != m || last->fisheye || !last->loaded || level_mode < 0 || level_mode > 2) return ORBX_E_BAD_ARG;
    const int rc = track_check(m, cur, false, cam && pose, map, n_ids, ids, last->host_n(), last->cap, cur_match, proj_u, proj_v);
    if (rc != ORBX_OK) return rc;
    TrackArgs tr = {false, map, ids, nullptr, last->kps, last->count, cam, pose, th, 0.f, level_mode, projected, proj_u, proj_v, nullptr, nullptr, nullptr,
                    0, nullptr};
    return track_run(m, cur, cur_occupied, tr, n_ids, has_obs, (float)ORBX_TH_HIGH, check_orientation, cur_match);
}

// the same for a fisheye-stereo rig (ORBmatcher.cc:1676-1887 with the twin :1794-1863): view = the LEFT camera's, Trl = GetRelativePoseTrl(); `last` is a
// rig handle as well -- rows [0, N_left) are mvKeys, the others mvKeysRight; cur_match holds N = N_left + N_right entries
extern "C" int orbx_frame_track_last_frame_fisheye_map(orbx_matcher *m, orbx_frame *cur, orbx_frame *last, const uint8_t *cur_occupied,
                                                       const orbx_fisheye_view *view, const float *Trl_R9, const float *Trl_t3, orbx_map *map, int n_ids,
                                                       const int32_t *ids, const uint8_t *has_obs, float th, int level_mode, int check_orientation,
                                                       int32_t *cur_match, uint8_t *projected, float *proj_u, float *proj_v) {
    if (!last || last == cur || last->owner != m || !last->fisheye || !last->loaded || level_mode < 0 || level_mode > 2) return ORBX_E_BAD_ARG;
    const int rc = track_check(m, cur, true, view && Trl_R9 && Trl_t3, map, n_ids, ids, last->host_n(), last->cap, cur_match, proj_u, proj_v);
    if (rc != ORBX_OK) return rc;
    TrackArgs tr = {false, map, ids, nullptr, last->kps, last->count, nullptr, nullptr, th, 0.f, level_mode, projected, proj_u, proj_v, view, Trl_R9, Trl_t3,
                    last->roff, nullptr};
    return track_run(m, cur, cur_occupied, tr, n_ids, has_obs, (float)ORBX_TH_HIGH, check_orientation, cur_match, true);
}

extern "C" int orbx_frame_search_by_projection_keyframe_map(orbx_matcher *m, orbx_frame *cur, const uint8_t *occupied, const orbx_camera *cam,
                                                            const orbx_frame_pose *pose, float log_scale_factor, orbx_keyframe *kf, orbx_map *map,
                                                            int n_ids, const int32_t *ids, float th, float max_dist, int check_orientation,
                                                            int32_t *match, uint8_t *projected, float *proj_u, float *proj_v) {
    if (!m || !kf || kf->fisheye || kf->device != m->device) return ORBX_E_BAD_ARG;
    const int rc = track_check(m, cur, false, cam && pose, map, n_ids, ids, kf->host_n(), kf->cap, match, proj_u, proj_v);
    if (rc != ORBX_OK) return rc;
    TrackArgs tr = {true, map, ids, kf, kf->kps, kf->count, cam, pose, th, log_scale_factor, 0, projected, proj_u, proj_v, nullptr, nullptr, nullptr, 0,
                    nullptr};
    return track_run(m, cur, occupied, tr, n_ids, nullptr, max_dist, check_orientation, match);
}

// the same for a fisheye-stereo rig: the LEFT camera only is searched (GetFeaturesInArea's default bRight = false, as
// orbx_frame_search_by_projection_window_fisheye); kf is a rig key frame, read for mvKeysUn[i].angle below N_left (0.f beyond, :1973); occupied / match
// hold N entries and the right camera's entries of match stay -1
extern "C" int orbx_frame_search_by_projection_keyframe_fisheye_map(orbx_matcher *m, orbx_frame *cur, const uint8_t *occupied,
                                                                    const orbx_fisheye_view *view, float log_scale_factor, orbx_keyframe *kf,
                                                                    orbx_map *map, int n_ids, const int32_t *ids, float th, float max_dist,
                                                                    int check_orientation, int32_t *match, uint8_t *projected, float *proj_u,
                                                                    float *proj_v) {
    if (!m || !kf || !kf->fisheye || kf->device != m->device) return ORBX_E_BAD_ARG;
    const int rc = track_check(m, cur, true, view != nullptr, map, n_ids, ids, kf->host_n(), kf->cap, match, proj_u, proj_v);
    if (rc != ORBX_OK) return rc;
    TrackArgs tr = {true, map, ids, kf, kf->kps, kf->count, nullptr, nullptr, th, log_scale_factor, 0, projected, proj_u, proj_v, view, nullptr, nullptr,
                    kf->roff, nullptr};
    return track_run(m, cur, occupied, tr, n_ids, nullptr, max_dist, check_orientation, match, false, true);
}

// ---------------------------------------------------------------------------------------------------------
// The BowVector of a resident handle and the key-frame database (include/orbx.h, orbx_keyframe_database; PARITY UNPINNED).  A BowVector is
// (ascending word ids, normalised double values, their count) wherever it lies: a row of the database, or arena space for a query and for
// orbx_frame_bow_vector / orbx_keyframe_bow_vector.  One kernel builds it from the word ids a handle keeps (k_bow_vector); a query is that kernel,
// k_bow_score over all slots and k_bow_select -- three launches whatever n_slots is.
// ---------------------------------------------------------------------------------------------------------
struct orbx_keyframe_database {
    int device = 0, n_slots = 0, words_cap = 0;
    uint8_t *dev = nullptr;            // one allocation, carved below
    int32_t *row_n = nullptr;          // [n_slots] words of the slot's vector, -1: empty
    int32_t *row_word = nullptr;       // [n_slots][words_cap]
    double *row_val = nullptr;         // [n_slots][words_cap]
    hipEvent_t written = nullptr;      // recorded behind the newest add / erase / clear, on the writing context's stream
    std::mutex mu;                     // guards everything below and the re-recording of `written`
    uint64_t write_seq = 0;            // writes recorded so far
    uint64_t seen_seq = 0;             // the newest write a query has waited for AND synchronised behind
    const orbx_vocabulary *voc = nullptr;   // of the first key frame added (since the last clear); every other must match, and so must a query
    int levelsup = 0;
};

namespace {

// what a BowVector is built from: the rows and the BoW arrays of a frame handle or of a key frame (kf != NULL: its events are waited for)
struct BowSource { HandleRows rows; const BowArrays *bow; orbx_keyframe *kf; };
struct BowVecDst { int32_t *word; double *val; int32_t *n; int cap; };

// the checks every entry point makes of its source before anything is enqueued
int bow_source_of_frame(const orbx_matcher *m, const orbx_frame *f, BowSource *out) {
    if (!m || !f || f->owner != m || !f->bow_valid) return ORBX_E_BAD_ARG;
    *out = BowSource{f->view(), &f->bow, nullptr};
    return ORBX_OK;
}
int bow_source_of_keyframe(const orbx_matcher *m, orbx_keyframe *kf, BowSource *out) {
    if (!m || !kf || kf->device != m->device) return ORBX_E_BAD_ARG;
    const KeyFrameBow *b = kf->bow.load(std::memory_order_acquire);
    if (!b) return ORBX_E_BAD_ARG;
    *out = BowSource{kf->view(), b, kf};
    return ORBX_OK;
}
int bow_source_ok(const BowSource &s) {
    if (!s.bow->voc || !s.bow->voc->weight) return ORBX_E_BAD_ARG;   // tf-idf needs the weights (orbx_vocabulary_set_word_weights)
    if (s.rows.feats() > kKeyFrameBowMax) return ORBX_E_TOO_LARGE;   // (the word ids are sorted in LDS)
    return ORBX_OK;
}
inline int bow_sort_cap(const BowSource &s) {
    int sort_cap = 1;
    while (sort_cap < s.rows.feats()) sort_cap <<= 1;
    return sort_cap;
}
hipError_t launch_bow_vector(hipStream_t st, const BowSource &s, const BowVecDst &d) {
    const int sort_cap = bow_sort_cap(s);
    const size_t lds = (size_t)kBowVecLdsHead + 4 * (size_t)sort_cap;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)k_bow_vector, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const HandleRows &r = s.rows;
    const orbx_vocabulary *v = s.bow->voc;
    BowVecSrc S;
    memset(&S, 0, sizeof(S));
    S.count = r.count; S.cap = r.cap;
    S.nl_host = r.fisheye ? r.nl : r.n; S.nr_host = r.fisheye ? r.nr : 0; S.roff = r.fisheye ? r.roff : r.cap;
    S.word = s.bow->word; S.word_pos = v->word_pos; S.weight = v->weight; S.n_words = v->n_words;
    S.out_word = d.word; S.out_val = d.val; S.out_n = d.n; S.out_cap = d.cap;
    hipLaunchKernelGGL(k_bow_vector, dim3(1), dim3(1024), lds, st, S, sort_cap);
    return hipGetLastError();
}

// mBowVec of a handle that has BoW, home: built in the call's arena, one download run (the handle's bound on its words), one synchronisation
int bow_vector_home(orbx_matcher *m, const BowSource &s, int32_t *word_id, double *value, int *n_words) {
    if (!word_id || !value || !n_words) return ORBX_E_BAD_ARG;
    ORBX_TRY(bow_source_ok(s));
    ORBX_HIP(hipSetDevice(m->device));
    const size_t cap = (size_t)std::max(s.rows.feats(), 1);
    BowVecDst d;
    ORBX_TRY(m->carve([&](Carve &A) { d.word = A.take<int32_t>(cap); d.val = A.take<double>(cap); d.n = A.take<int32_t>(1); }));
    d.cap = (int)cap;
    if (s.kf) ORBX_TRY(keyframe_bow_acquire(m, s.kf));
    ORBX_HIP(launch_bow_vector(m->exec(), s, d));
    std::vector<int32_t> w(cap);
    std::vector<double> v(cap);
    int32_t n = 0;
    ORBX_TRY(m->d2h(w.data(), d.word, 4 * cap)); ORBX_TRY(m->d2h(v.data(), d.val, 8 * cap)); ORBX_TRY(m->d2h(&n, d.n, 4));
    ORBX_TRY(m->sync_and_deliver());
    if (s.kf) keyframe_bow_release(s.kf);
    n = std::min(std::max(n, 0), (int32_t)cap);
    memcpy(word_id, w.data(), 4 * (size_t)n); memcpy(value, v.data(), 8 * (size_t)n);
    *n_words = n;
    return ORBX_OK;
}

// a write to the database on m's stream, under db->mu: behind the previous write, the next `written` recorded behind it
template <class F> int database_write(orbx_matcher *m, orbx_keyframe_database *db, F &&enqueue) {
    hipError_t e = db->write_seq > 0 ? hipStreamWaitEvent(m->stream, db->written, 0) : hipSuccess;
    m->dirty = true;
    if (e == hipSuccess) e = enqueue();
    if (e == hipSuccess) e = hipEventRecord(db->written, m->stream);
    if (e != hipSuccess) { set_error(hipGetErrorString(e)); return ORBX_E_HIP; }
    db->write_seq++;
    return ORBX_OK;
}

struct DatabaseQueryOut {
    int32_t *n_common; double *score; int32_t *cand_slot, *cand_common; double *cand_score; int cand_cap; int *n_cand, *max_common;
};

// The query: the source's BowVector into the arena, every slot scored against it, the candidates selected.  One upload run (the exclude list), three
// launches, one download run, one synchronisation.
int database_query(orbx_matcher *m, orbx_keyframe_database *db, const BowSource &s, const int32_t *exclude, int n_exclude, float min_ratio,
                   const DatabaseQueryOut &o) {
    if (!db || db->device != m->device || n_exclude < 0 || (n_exclude > 0 && !exclude) || !(min_ratio >= 0.f && min_ratio <= 1.f) || o.cand_cap < 0 ||
        (o.cand_cap > 0 && !o.cand_slot) || !o.n_cand || !o.max_common)
        return ORBX_E_BAD_ARG;
    ORBX_TRY(bow_source_ok(s));
    for (int e = 0; e < n_exclude; e++)
        if (exclude[e] < 0 || exclude[e] >= db->n_slots) return ORBX_E_BAD_ARG;
    uint64_t seq = 0;
    bool wait = false;
    {
        std::lock_guard<std::mutex> lock(db->mu);
        if (db->voc && (db->voc != s.bow->voc || db->levelsup != s.bow->levelsup)) return ORBX_E_BAD_ARG;
        wait = db->seen_seq < db->write_seq;
        seq = db->write_seq;
    }
    ORBX_HIP(hipSetDevice(m->device));
    const size_t qcap = (size_t)std::max(s.rows.feats(), 1), ns = (size_t)db->n_slots, cc = (size_t)std::max(o.cand_cap, 1);
    BowVecDst q;
    BowQuery Q;
    BowSelect S;
    memset(&Q, 0, sizeof(Q)); memset(&S, 0, sizeof(S));
    ORBX_TRY(m->carve([&](Carve &A) {
        Q.exclude = A.up_opt(exclude, (size_t)n_exclude);
        q.word = A.take<int32_t>(qcap); q.val = A.take<double>(qcap); q.n = A.take<int32_t>(1);
        S.meta = A.take<int32_t>(2);   // the downloads side by side: one run
        S.cand_slot = A.take<int32_t>(cc); S.cand_common = A.take<int32_t>(cc); S.cand_score = A.take<double>(cc);
        Q.common = A.take<int32_t>(ns); Q.score = A.take<double>(ns);
    }));
    q.cap = (int)qcap;
    if (s.kf) ORBX_TRY(keyframe_bow_acquire(m, s.kf));
    if (wait) {
        std::lock_guard<std::mutex> lock(db->mu);   // (`written` is re-recorded under the lock)
        ORBX_HIP(hipStreamWaitEvent(m->stream, db->written, 0));
        seq = db->write_seq;
    }
    ORBX_HIP(launch_bow_vector(m->exec(), s, q));
    Q.q_word = q.word; Q.q_val = q.val; Q.q_n = q.n; Q.q_cap = q.cap;
    Q.row_n = db->row_n; Q.row_word = db->row_word; Q.row_val = db->row_val; Q.n_slots = db->n_slots; Q.words_cap = db->words_cap;
    Q.n_exclude = n_exclude;
    hipLaunchKernelGGL(k_bow_score, dim3((unsigned)((db->n_slots + 3) / 4)), dim3(256), 0, m->exec(), Q);
    S.common = Q.common; S.score = Q.score; S.n_slots = db->n_slots; S.min_ratio = min_ratio; S.cand_cap = o.cand_cap;
    hipLaunchKernelGGL(k_bow_select, dim3(1), dim3(1024), 0, m->exec(), S);
    ORBX_HIP(hipGetLastError());
    int32_t meta[2] = {0, 0};
    std::vector<int32_t> c_slot(cc), c_common(cc);
    std::vector<double> c_score(cc);
    ORBX_TRY(m->d2h(meta, S.meta, 8));
    if (o.cand_cap > 0) {
        ORBX_TRY(m->d2h(c_slot.data(), S.cand_slot, 4 * cc)); ORBX_TRY(m->d2h(c_common.data(), S.cand_common, 4 * cc));
        ORBX_TRY(m->d2h(c_score.data(), S.cand_score, 8 * cc));
    }
    if (o.n_common) ORBX_TRY(m->d2h(o.n_common, Q.common, 4 * ns));
    if (o.score) ORBX_TRY(m->d2h(o.score, Q.score, 8 * ns));
    ORBX_TRY(m->sync_and_deliver());
    if (s.kf) keyframe_bow_release(s.kf);
    {
        std::lock_guard<std::mutex> lock(db->mu);
        db->seen_seq = std::max(db->seen_seq, seq);
    }
    const size_t got = (size_t)std::min(std::max(meta[0], 0), o.cand_cap);   // the list is cut at cand_cap; n_cand is the true count
    if (got) {
        memcpy(o.cand_slot, c_slot.data(), 4 * got);
        if (o.cand_common) memcpy(o.cand_common, c_common.data(), 4 * got);
        if (o.cand_score) memcpy(o.cand_score, c_score.data(), 8 * got);
    }
    *o.n_cand = meta[0]; *o.max_common = meta[1];
    return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_frame_bow_vector(orbx_matcher *m, orbx_frame *f, int32_t *word_id, double *value, int *n_words) {
    BowSource s;
    ORBX_TRY(bow_source_of_frame(m, f, &s));
    return bow_vector_home(m, s, word_id, value, n_words);
}

int orbx_keyframe_bow_vector(orbx_matcher *m, orbx_keyframe *kf, int32_t *word_id, double *value, int *n_words) {
    BowSource s;
    ORBX_TRY(bow_source_of_keyframe(m, kf, &s));
    return bow_vector_home(m, s, word_id, value, n_words);
}

int orbx_keyframe_database_create(int device, int n_slots, int words_cap, orbx_keyframe_database **out) {
    if (!out) return ORBX_E_BAD_ARG;
    *out = nullptr;
    if (n_slots < 1 || words_cap < 1) return ORBX_E_BAD_ARG;
    if (n_slots > ORBX_MAX_DATABASE_SLOTS || words_cap > kKeyFrameBowMax) return ORBX_E_TOO_LARGE;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        set_error("no usable HIP device (liborbx has no CPU fallback)");
        return ORBX_E_NO_DEVICE;
    }
    ORBX_HIP(hipSetDevice(device));
    std::unique_ptr<orbx_keyframe_database> db(new orbx_keyframe_database());
    db->device = device; db->n_slots = n_slots; db->words_cap = words_cap;
    const size_t rows = (size_t)n_slots * (size_t)words_cap;
    Layout L;
    const size_t off_n = L.add(4 * (size_t)n_slots), off_w = L.add(4 * rows), off_v = L.add(8 * rows);
    hipError_t e = hipMalloc((void **)&db->dev, L.used);
    if (e == hipSuccess) e = hipMemset(db->dev + off_n, 0xff, 4 * (size_t)n_slots);   // every slot empty
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipEventCreateWithFlags(&db->written, hipEventDisableTiming);
    if (e != hipSuccess) {
        set_error(hipGetErrorString(e));
        orbx_keyframe_database_destroy(db.release());
        return ORBX_E_HIP;
    }
    db->row_n = (int32_t *)(db->dev + off_n); db->row_word = (int32_t *)(db->dev + off_w); db->row_val = (double *)(db->dev + off_v);
    *out = db.release();
    return ORBX_OK;
}

void orbx_keyframe_database_destroy(orbx_keyframe_database *db) {
    if (!db) return;
    (void)hipSetDevice(db->device);
    if (db->written) { (void)hipEventSynchronize(db->written); (void)hipEventDestroy(db->written); }   // the last write has run; no query is running (the caller's contract)
    if (db->dev) (void)hipFree(db->dev);
    delete db;
}

// KeyFrameDatabase::add: the key frame's BowVector straight into the row of `slot`.  Stream order, no host wait; the row is a copy.
int orbx_keyframe_database_add(orbx_matcher *m, orbx_keyframe_database *db, int slot, orbx_keyframe *kf) {
    BowSource s;
    ORBX_TRY(bow_source_of_keyframe(m, kf, &s));
    if (!db || db->device != m->device || slot < 0 || slot >= db->n_slots) return ORBX_E_BAD_ARG;
    ORBX_TRY(bow_source_ok(s));
    std::lock_guard<std::mutex> lock(db->mu);
    if (db->voc && (db->voc != s.bow->voc || db->levelsup != s.bow->levelsup)) return ORBX_E_BAD_ARG;
    if (s.rows.feats() > db->words_cap) return ORBX_E_TOO_LARGE;   // the row's bound: N where the host knows it, the capacity otherwise
    ORBX_HIP(hipSetDevice(m->device));
    ORBX_TRY(keyframe_bow_acquire(m, kf));
    const size_t at = (size_t)slot * (size_t)db->words_cap;
    const BowVecDst d = {db->row_word + at, db->row_val + at, db->row_n + slot, db->words_cap};
    ORBX_TRY(database_write(m, db, [&] { return launch_bow_vector(m->stream, s, d); }));
    db->voc = s.bow->voc; db->levelsup = s.bow->levelsup;
    return ORBX_OK;
}

// KeyFrameDatabase::erase: the slot's count becomes -1 in stream order
int orbx_keyframe_database_erase(orbx_matcher *m, orbx_keyframe_database *db, int slot) {
    if (!m || !db || db->device != m->device || slot < 0 || slot >= db->n_slots) return ORBX_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    ORBX_HIP(hipSetDevice(m->device));
    return database_write(m, db, [&] { return hipMemsetAsync(db->row_n + slot, 0xff, 4, m->stream); });
}

// KeyFrameDatabase::clear: every slot empty; the next add names the vocabulary anew
int orbx_keyframe_database_clear(orbx_matcher *m, orbx_keyframe_database *db) {
    if (!m || !db || db->device != m->device) return ORBX_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(db->mu);
    ORBX_HIP(hipSetDevice(m->device));
    ORBX_TRY(database_write(m, db, [&] { return hipMemsetAsync(db->row_n, 0xff, 4 * (size_t)db->n_slots, m->stream); }));
    db->voc = nullptr; db->levelsup = 0;
    return ORBX_OK;
}

int orbx_keyframe_database_query_frame(orbx_matcher *m, orbx_keyframe_database *db, orbx_frame *f, const int32_t *exclude, int n_exclude,
                                       float min_ratio, int32_t *n_common, double *score, int32_t *cand_slot, int32_t *cand_common,
                                       double *cand_score, int cand_cap, int *n_cand, int *max_common) {
    BowSource s;
    ORBX_TRY(bow_source_of_frame(m, f, &s));
    return database_query(m, db, s, exclude, n_exclude, min_ratio, {n_common, score, cand_slot, cand_common, cand_score, cand_cap, n_cand, max_common});
}

int orbx_keyframe_database_query_keyframe(orbx_matcher *m, orbx_keyframe_database *db, orbx_keyframe *kf, const int32_t *exclude, int n_exclude,
                                          float min_ratio, int32_t *n_common, double *score, int32_t *cand_slot, int32_t *cand_common,
                                          double *cand_score, int cand_cap, int *n_cand, int *max_common) {
    BowSource s;
    ORBX_TRY(bow_source_of_keyframe(m, kf, &s));
    return database_query(m, db, s, exclude, n_exclude, min_ratio, {n_common, score, cand_slot, cand_common, cand_score, cand_cap, n_cand, max_common});
}

}  // extern "C"
