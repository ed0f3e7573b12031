// extractor_state.h -- host-side state of an extractor (shared by orbx_extractor.hip and orbx_matcher.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "orbx_internal.h"

namespace orbx {

extern thread_local std::string g_last_error;
void set_error(const std::string &s);

#define ORBX_HIP(expr)                                                                                 \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            orbx::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                        \
            return ORBX_E_HIP;                                                                         \
        }                                                                                              \
    } while (0)
// a step that returns an ORBX_* code itself
#define ORBX_TRY(expr)                                                                                 \
    do {                                                                                               \
        const int _r = (expr);                                                                         \
        if (_r != ORBX_OK) return _r;                                                                  \
    } while (0)

// Device buffer.  Normal mode: hipMalloc + zero fill (every buffer has defined contents from its first use).
// Guard mode (ORBX_GUARD=1|2, debugging aid, see tools/repro_fault.sh): the buffer is placed through the HIP virtual-memory
// API so that its END (1) or its START (2) touches an unmapped address range, and it is filled with a poison byte: any kernel or copy
// that runs past (before) the buffer, or indexes with a value it never wrote, faults deterministically instead of silently
// touching a neighbouring allocation.
int guard_mode();
int guard_fill();   // ORBX_GUARD_FILL=<byte> (default 0xCB)
// Optional roctx ranges around the host-side phases (the reference instruments the same two spots with its REGISTER_TIMES timers:
// ORB extraction and stereo / projection matching, Tracking.cc).  ORBX_ROCTX=1 resolves libroctx64.so / librocprofiler-sdk-roctx.so at
// run time (no link dependency); rocprofv3 --marker-trace then shows orbx:extract / orbx:match / orbx:download ranges.
struct RoctxRange {
    explicit RoctxRange(const char *name);
    ~RoctxRange();
    bool on;
};

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    // guard-mode bookkeeping
    void *va = nullptr; size_t va_bytes = 0, map_bytes = 0, gran = 0;
    hipMemGenericAllocationHandle_t handle{};
    bool guarded = false;
    int ensure(size_t need) {
        if (need <= bytes) return ORBX_OK;
        release();
        if (guard_mode() == 0) {
            ORBX_HIP(hipMalloc(&p, need));
            bytes = need;
            // the clear must have RUN before anybody uses the buffer: hipMemset may return before the fill executes (it is queued on the
            // null stream), and the library's non-blocking streams do not wait for the null stream -- a copy or kernel enqueued right
            // after ensure() could otherwise be overtaken by the zeros (seen once: the first host-input batch into a fresh slab)
            ORBX_HIP(hipMemset(p, 0, need));
            ORBX_HIP(hipDeviceSynchronize());   // control run without this wait: 5 of 5 short-batch loops differ (profiles/r03_a_open_item_control.log)
            if (getenv("ORBX_DEBUG_ALLOC")) fprintf(stderr, "[orbx alloc] %p .. %p  %zu bytes\n", p, (char *)p + need, need);
            return ORBX_OK;
        }
        int dev = 0;
        ORBX_HIP(hipGetDevice(&dev));
        hipMemAllocationProp prop{};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = dev;
        ORBX_HIP(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum));
        const size_t need16 = (need + 15) & ~(size_t)15;
        map_bytes = (need16 + gran - 1) / gran * gran;
        va_bytes = map_bytes + 2 * gran;
        ORBX_HIP(hipMemAddressReserve(&va, va_bytes, gran, nullptr, 0));
        ORBX_HIP(hipMemCreate(&handle, map_bytes, &prop, 0));
        ORBX_HIP(hipMemMap((char *)va + gran, map_bytes, 0, handle, 0));
        hipMemAccessDesc acc{};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        ORBX_HIP(hipMemSetAccess((char *)va + gran, map_bytes, &acc, 1));
        guarded = true;
        ORBX_HIP(hipMemset((char *)va + gran, guard_fill(), map_bytes));
        ORBX_HIP(hipDeviceSynchronize());   // as above
        p = (char *)va + gran + (guard_mode() == 1 ? map_bytes - need16 : 0);
        bytes = need;
        return ORBX_OK;
    }
    void release() {
        if (guarded) {
            // the address range stays reserved (debug mode; re-using freed ranges crashed hipMemMap in ROCm 7.0's runtime)
            (void)hipMemUnmap((char *)va + gran, map_bytes);
            (void)hipMemRelease(handle);
            guarded = false; va = nullptr;
        } else if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
    }
};

// The layout primitive: buffers of one allocation in the order they are declared, each on a multiple of 256 bytes and owning its size rounded up to 256
// (k_xfer rounds a run up to 16 bytes).  Used for a matcher call's arena (Carve), for the allocations that stay resident (frame handles, key frames)
// and for the extractor's pinned staging block (Staged).
struct Layout {
    size_t used = 0;
    static size_t pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    size_t add(size_t bytes) { const size_t o = used; used += pad(bytes); return o; }
};

// The asynchronous entry points hand the caller's host pointers straight to the copy engine, so they insist on pinned memory
// (hipHostMalloc / hipHostRegister, e.g. torch's pin_memory()): pageable memory would be pinned page by page by the runtime behind
// the caller's back and the copy would not be asynchronous at all.
inline bool is_pinned_host(const void *p) {
    if (!p) return true;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

enum { K_PYR_BASE, K_PYR_RESIZE, K_FAST, K_OCTREE, K_FINALIZE, K_BLUR, K_DESCRIBE, K_MATCH_SCAN, K_MATCH_RESOLVE, K_COUNT };

}  // namespace orbx

extern "C" int orbx_materialize_level0(struct orbx_extractor *ex);   // orbx_extractor.hip (internal: not part of include/orbx.h)

struct orbx_extractor {
    typedef orbx::DevBuf DevBuf;
    typedef orbx::LevelInfo LevelInfo;
    enum { K_COUNT = orbx::K_COUNT };
    orbx_params prm;
    int device = 0;
    hipStream_t stream = nullptr;
    // T1 tables (ORBextractor.cc:414-468)
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    std::vector<int> quota;
    int umax[16];
    // geometry of the current configuration
    int width = 0, height = 0, batch_cap = 0, last_batch = 0;
    std::vector<LevelInfo> lv;
    size_t pyr_frame = 0, blur_frame = 0, cand_frame = 0, lvl_frame = 0;
    int total_cells = 0, cap = 0, max_pool = 0;
    size_t fast_lds = 0;
    bool resize_march_ok[orbx::kMaxLevels] = {};   // every tap pair of a dword column of level l within 8 source bytes (k_pyr_resize_march)
    bool fast_strip = false;    // k_fast_strip applies (cells at most 57 px wide, 63 px high)
    static constexpr int kStripGcap0 = 512, kStripQcap0 = 816;   // the default queue sizes (sparse scenes); orbx_tune_fast_queues
    int strip_gmax = 1024, strip_qmax = 4096;                     // a wave's band in groups / pixels, over the geometry's strips (configure)
    int n_strips = 0, strip_pix_bytes = 0, strip_gcap = kStripGcap0, strip_qcap = kStripQcap0;   // k_fast_strip: strips per frame, tile rows, per-wave group / pixel queue capacities
    int fast_wave_pitch = 64, fast_wave_rows = 0, fast_wave_qfull = 16;   // list pass (fast_wave_cell): LDS tile pitch (48 / 64), max sub-image rows, whole-cell queue
    DevBuf d_fast_ovf;          // [1 + n_fast_tiles * batch] overflow counter + list of k_fast_wave
    bool oct_par = true;        // wave-parallel quad-tree kernel (k_octree_par); false: sequential emulation (k_octree)
    bool oct_single_wave = false;   // diagnostic: levels beyond the LDS tiers on one wave (round 5) instead of the whole workgroup
    bool fast_wave = true;      // every level's cell fits k_fast_wave's fixed LDS pitch
    int n_fast_tiles = 0, n_blur_items = 0;
    int blur_waves = 2048;      // single-wave workgroups of k_blur_stream (measured: 512 / 1024 / 2048 / 4096 -> EuRoC step 1.25 / 1.115 / 1.09 / 1.10 ms)
    // device memory
    DevBuf d_lv, d_xtab, d_ytab, d_xgtab, d_fast_tiles, d_strips, d_blur_items, d_dc;
    // k_pyr_stream (levels 1 .. n-1 in one launch): per-geometry tables; ps_ok false = the geometry does not fit, the per-level launches run
    // one plan per band count (1, 2, 4, 8 bands per frame): the launch takes the one that puts about two workgroups on every CU for the batch at hand
    struct PyrPlanDev { DevBuf cols, steps, tasks, lists; orbx::PyrStreamGeom geom; int bands = 0; size_t lds = 0; bool ok = false; };
    PyrPlanDev ps_plan[4];
    bool ps_ok = false;         // at least one plan exists
    int ps_wg_target = 512;     // workgroups a launch should have (2 per CU): 256 frames -> 2 bands, 128 -> 4 (KITTI 150 -> 104 us, TUM-VI 328 -> 222 us against 2 bands)
    int ps_min_frames = 48;   // batches smaller than ps_min_frames keep the per-level launches (a band is one workgroup: too few to fill the device; measured equal at 16 frames, 3 % slower at 32, 5 % faster at 64, 14 % at 128)
    // Level 0 in place: a batch extracted by k_pyr_stream + k_fast_strip + k_describe_fused reads level 0 from the caller's frames (which orbx.h
    // keeps untouched until orbx_sync / orbx_download_wait; the upload slab for orbx_extract_batch_host) and leaves the slab's level 0 unwritten; the few readers of the padded level 0
    // (orbx_get_level, the stereo rig's SAD stage, the blurred-level debug readout) materialise it first: materialize_level0()
    bool lvl0_inplace = false;
    // level 0 of an in-place batch is written on REQUEST from the frames it was extracted from.  Frames handed to orbx_extract_batch_device
    // (in0_callers) are the caller's to overwrite after orbx_sync / orbx_download_wait (include/orbx.h): those two calls mark them released, and level 0
    // or a re-run of k_describe_fused (orbx_debug_fused_patches) is refused after that (ORBX_E_STALE) instead of answered from whatever the buffer
    // holds by then.  Frames of orbx_extract_batch_host lie in the library's own upload slab, which nothing overwrites while the batch is the last
    // one: they are never released.  in0_copy_seq = downloads issued when the batch was enqueued (a download issued later covers it).
    bool in0_released = false;
    bool in0_callers = false;
    unsigned in0_copy_seq = 0;
    hipEvent_t in0_event = nullptr;   // "input consumed" event of the in-place batch (upload slab of orbx_extract_batch_host): re-recorded behind the materialisation
    const uint8_t *in0_images = nullptr;
    size_t in0_row_stride = 0, in0_frame_stride = 0;
    int n_strips0 = 0;          // level-0 strips of k_fast_strip (the first of a frame)
    // Stereo rig (orbx_stereo_batch_device): the SAD stage reads both extractors' pyramids on the match stream while the NEXT pair of batches is
    // extracted, so an extractor that has been part of a rig alternates between two pyramid slabs (allocated at the first stereo call)
    DevBuf d_pyr2;
    bool pyr_double = false;
    int pyr_slot = 0;
    uint8_t *pyr_cur() const { return (uint8_t *)(pyr_slot ? d_pyr2.p : d_pyr.p); }
    DevBuf d_pyr, d_blur, d_cellcnt, d_cellent, d_keys0, d_keys1, d_nof0, d_nof1, d_lvlkp, d_lvlcnt, d_candtot, d_work;
    DevBuf d_kps, d_desc, d_count, d_mono, d_err;
    DevBuf d_mkey1, d_mkey2, d_mocc, d_mentries, d_mprobs, d_mres, d_mscale, d_mgrid;  // batched frame-to-frame matcher scratch
    // pinned host staging
    void *h_stage = nullptr;
    size_t h_stage_bytes = 0;
    // profiling
    bool profile = false;
    double prof_ms[K_COUNT] = {0};
    int64_t prof_n[K_COUNT] = {0};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // asynchronous result download (copy stream overlaps the next batch's kernels)
    hipStream_t copy_stream = nullptr;
    // concurrent branches of one batch: blur runs beside FAST/quad-tree (aux), the frame-to-frame matcher of batch i
    // runs beside the pyramid/FAST/quad-tree of batch i+1 (match)
    hipStream_t aux_stream = nullptr, match_stream = nullptr;
    // host-resident input (orbx_extract_batch_host): upload stream + two input slabs; slot s may be overwritten once the
    // k_pyr_base that read it has finished (ev_in_free), the extraction may start once the upload has landed (ev_in_ready)
    hipStream_t in_stream = nullptr;
    hipStream_t spare_stream = nullptr;   // never used: spaces the hardware queues of a second extractor (orbx_create)
    DevBuf d_in[2];
    hipEvent_t ev_in_free[2] = {nullptr, nullptr}, ev_in_ready[2] = {nullptr, nullptr};
    bool in_used[2] = {false, false};
    unsigned in_issued = 0;
    hipEvent_t ev_pyr = nullptr, ev_blur = nullptr, ev_describe = nullptr, ev_match = nullptr;
    bool match_pending = false;
    bool copy_covers_match = false;   // the most recent download waited for ev_match on the copy stream: its ev_copy_done implies the matcher is done
    bool side_streams = true;  // the blur pass / the matcher / the downloads on their own streams (profile mode keeps every kernel on the main stream)
    bool fused_blur = false;   // k_describe_fused (the blur on demand around the keypoints) instead of k_blur_stream + k_describe: chosen per geometry in
                               // configure(), ORBX_FUSED_BLUR=0 / 1 forces
    hipEvent_t ev_stereo_copy[2] = {nullptr, nullptr};   // ends of the last two orbx_stereo_batch_download_async
    unsigned stereo_copy_issued = 0, stereo_copy_waited = 0;
    hipEvent_t ev_copy_done[2] = {nullptr, nullptr};  // ring: up to two downloads in flight
    unsigned copy_issued = 0, copy_waited = 0;         // copy_issued - copy_waited = downloads in flight
    bool copy_pending = false;                         // a download was issued since the last (re)configuration
    int32_t *h_err = nullptr;  // pinned, 2 slots
    DevBuf d_st_bidx, d_st_bdist, d_st_ur, d_st_depth, d_st_sad, d_st_nm, d_st_scales, d_st_rowptr, d_st_rowidx;  // device stereo matcher (left extractor)
    // the batch (batch_seq) whose mvuRight / mvDepth lie in d_st_ur / d_st_depth, written by orbx_stereo_batch_device or orbx_rgbd_batch_device
    // (0: no stage has run): orbx_frame_load_stereo_batch copies from them
    uint64_t st_seq = 0;
    // fisheye stereo stage (orbx_stereo_fisheye_batch_device, left extractor): its own result buffers -- kNN-2 rows [B][capL][2], l2r / depth [B][capL],
    // p3d [B][capL][3], r2l [B][capR], counts [B][4] (nMatches, descMatches, n_left, n_right) -- and the shape they were written with (a later extraction
    // may change last_batch / the counts before the download)
    DevBuf d_sf_idx, d_sf_dist, d_sf_l2r, d_sf_r2l, d_sf_depth, d_sf_p3d, d_sf_cnt, d_sf_sigma, d_sf_rig;
    int sf_batch = 0, sf_capL = 0, sf_capR = 0;
    // which batches the stage read (batch_seq of both extractors) and its end on the device: orbx_frame_load_stereo_fisheye_batch copies from it
    uint64_t batch_seq = 0, sf_seq_l = 0, sf_seq_r = 0;
    const orbx_extractor *sf_right = nullptr;
    hipEvent_t ev_sf = nullptr;
    DevBuf d_match, d_nmatch;  // internal match outputs [B][cap], [B] (one matcher per batch: orbx.h)
    int internal_match_owner = 0;   // which batched matcher wrote them for the current batch: 0 none, 1 frame-to-frame, 2 map points
    // cached problem descriptors of orbx_match_consecutive_device
    struct MatchKey {
        int n = 0, cap = 0; const void *match = nullptr, *nm = nullptr; float th = 0, du = 0, dv = 0; int ori = 0; const void *kps = nullptr;
        bool operator==(const MatchKey &o) const {
            return n == o.n && cap == o.cap && match == o.match && nm == o.nm && th == o.th && du == o.du && dv == o.dv && ori == o.ori && kps == o.kps;
        }
    } mkey;

    // batched SearchByProjection(Frame, MapPoints) on the resident batch (orbx_search_mappoints_batch_device)
    DevBuf d_mp_qr, d_mp_qmin, d_mp_qmax, d_mp_valid, d_mp_keys, d_mp_meta, d_mp_grid, d_mp_probs, d_mp_res, d_mp_misc, d_mp_entries;
    struct MpKey { int n = 0, cap = 0, n_mp = 0; const void *px = nullptr, *py = nullptr, *lvl = nullptr, *vc = nullptr, *iv = nullptr, *desc = nullptr,
                   *match = nullptr, *nm = nullptr, *kps = nullptr; size_t dstride = 0; float th = 0, ratio = 0;
        bool operator==(const MpKey &o) const {
            return n == o.n && cap == o.cap && n_mp == o.n_mp && px == o.px && py == o.py && lvl == o.lvl && vc == o.vc && iv == o.iv && desc == o.desc &&
                   match == o.match && nm == o.nm && kps == o.kps && dstride == o.dstride && th == o.th && ratio == o.ratio;
        }
    } mpkey;

    // camera of the batch path (orbx_set_camera): undistorted keypoints + undistorted image bounds for the batched matchers
    bool has_camera = false;
    float cam_params[9] = {0};           // fx fy cx cy k1 k2 p1 p2 k3
    float cam_bf = 0;
    float bounds[4] = {0, 0, 0, 0};      // mnMinX, mnMaxX, mnMinY, mnMaxY of the current geometry
    DevBuf d_kps_un, d_frustum_frames;
    void *h_frustum[3] = {nullptr, nullptr, nullptr};   // pinned ring of orbx_frustum_batch_device's pose uploads
    size_t h_frustum_bytes[3] = {0, 0, 0};
    hipEvent_t ev_frustum[3] = {nullptr, nullptr, nullptr};
    bool frustum_used[3] = {false, false, false};
    unsigned frustum_issued = 0;
    // orbx_resize_batch_device: cv::resize's coefficient tables of the last size pairs (k_resize).  A table is written once, before the first kernel
    // that reads it is enqueued; a fifth size pair waits for the stream before it takes the oldest slot.
    struct ResizeTabDev { int sw = 0, sh = 0, dw = 0, dh = 0; DevBuf x, y; };
    ResizeTabDev rs_tab[4];
    unsigned rs_next = 0;
    const void *match_kps() const { return has_camera ? d_kps_un.p : d_kps.p; }

    // One synchronous download through the pinned staging block (no caller pointer is ever handed to the HIP runtime: see PinnedArena in
    // matcher_context.h).  `copies(S)` names every copy of the call once -- S.view / S.out / S.room (Staged, below) -- and the block's layout, its
    // size and the transfers are those statements, nothing else.  As orbx_matcher::carve it runs twice: a sizing pass (it only adds up; every pointer
    // it hands out is NULL), then the block is sized -- before the first copy is issued: growing it frees the old one -- and the pass that issues the
    // copies on the main stream.  ONE stream synchronisation; then the views may be read and the outputs are in the caller's buffers.
    template <class F> int download(F &&copies);

    int ensure_stage(size_t bytes) {
        if (bytes <= h_stage_bytes) return ORBX_OK;
        if (h_stage) (void)hipHostFree(h_stage);
        h_stage = nullptr; h_stage_bytes = 0;
        // coherent (fine-grained) whatever HIP_HOST_COHERENT says: orbx_extract's kernels read the image from and write the results into this
        // block themselves, and the host reads them right after the stream synchronisation
        ORBX_HIP(hipHostMalloc(&h_stage, bytes, hipHostMallocCoherent));
        h_stage_bytes = bytes;
        return ORBX_OK;
    }
};

// The copies of one orbx_extractor::download, declared in the order they lie in the staging block.
struct Staged {
    orbx_extractor *ex;
    bool sizing;
    orbx::Layout L;
    int err = ORBX_OK;
    struct Out { void *dst; const uint8_t *src; size_t bytes; } outs[8];
    int n_outs = 0;
    // `bytes` from d_src, read by the caller in the block after the synchronisation (headers, counts, rows it unpacks or clamps itself);
    // the pointer holds until the extractor's next download
    template <class T> const T *view(const void *d_src, size_t bytes) {
        const size_t o = L.add(bytes);
        if (sizing) return nullptr;
        uint8_t *h = (uint8_t *)ex->h_stage + o;
        if (bytes && err == ORBX_OK) err = issue(h, d_src, bytes);
        return reinterpret_cast<const T *>(h);
    }
    // `bytes` from d_src delivered to the caller's `dst` after the synchronisation; dst NULL: no copy is issued and nothing is written
    void out(void *dst, const void *d_src, size_t bytes) {
        if (!dst) return;
        const uint8_t *h = view<uint8_t>(d_src, bytes);
        if (sizing) return;
        if (n_outs == (int)(sizeof(outs) / sizeof(outs[0]))) { orbx::set_error("a download declared more outputs than Staged holds"); err = ORBX_E_INTERNAL; return; }
        outs[n_outs++] = Out{dst, h, bytes};
    }
    // room that a later download of the same call will take (a two-phase call sizes the block once, in its first phase)
    void room(size_t bytes) { L.add(bytes); }
    int issue(void *h, const void *d_src, size_t bytes) {
        ORBX_HIP(hipMemcpyAsync(h, d_src, bytes, hipMemcpyDeviceToHost, ex->stream));
        return ORBX_OK;
    }
};

template <class F> int orbx_extractor::download(F &&copies) {
    Staged S{this, true};
    copies(S);
    ORBX_TRY(ensure_stage(S.L.used));
    Staged D{this, false};
    copies(D);
    ORBX_TRY(D.err);
    ORBX_HIP(hipStreamSynchronize(stream));
    for (int i = 0; i < D.n_outs; i++) memcpy(D.outs[i].dst, D.outs[i].src, D.outs[i].bytes);
    return ORBX_OK;
}

// ---------------------------------------------------------------------------------------------------------
// A stage behind an extraction (a batched matcher, a stereo or RGB-D stage): kernels that read the resident batch of one extractor, or of the left /
// right pair of a rig, while the next batch's pyramid / FAST / quad-tree run on the main stream.  Every such entry point is
//     st = stage_stream(first);  stage_begin(st, {participants}, ..);  its launches on st;  stage_end(st, {participants});
// The extractor's side of the protocol: the next k_finalize (enqueue_extract) waits for ev_match while match_pending is set, unless a download issued
// since then has waited for it on the copy stream already (copy_covers_match: stage_results_on).
// ---------------------------------------------------------------------------------------------------------
namespace orbx {

// the stage's stream: the match stream of the first participant; profile mode and side_streams off keep every kernel on the main stream
inline hipStream_t stage_stream(const orbx_extractor *ex) { return !ex->profile && ex->side_streams ? ex->match_stream : ex->stream; }

// Behind every participant's extraction (ev_describe: its k_undistort and a later materialisation of level 0 included) -- except an extraction
// enqueued on `st` itself, where stream order says the same -- and, for a stage that overwrites the first participant's d_st_* results, behind the
// last orbx_stereo_batch_download_async, whose copy may still read them.
inline int stage_begin(hipStream_t st, std::initializer_list<orbx_extractor *> parts, bool overwrites_stereo_results = false) {
    for (orbx_extractor *e : parts)
        if (e->stream != st) ORBX_HIP(hipStreamWaitEvent(st, e->ev_describe, 0));
    orbx_extractor *first = *parts.begin();
    if (overwrites_stereo_results && first->stereo_copy_issued)
        ORBX_HIP(hipStreamWaitEvent(st, first->ev_stereo_copy[(first->stereo_copy_issued - 1) & 1], 0));
    return ORBX_OK;
}

// The stage is enqueued: no participant may overwrite its key points / descriptors / counts / pyramid before the stage is done.  ev_match and the two
// flags change together: the next extraction and the next download read all three.
inline int stage_end(hipStream_t st, std::initializer_list<orbx_extractor *> parts) {
    ORBX_HIP(hipGetLastError());
    for (orbx_extractor *e : parts) {
        ORBX_HIP(hipEventRecord(e->ev_match, st));
        e->match_pending = true; e->copy_covers_match = false;
    }
    return ORBX_OK;
}

// A download on copy stream `cs` that reads a pending stage's results waits for the stage; the download's end then implies the stage's.
inline int stage_results_on(orbx_extractor *ex, hipStream_t cs) {
    if (ex->match_pending) ORBX_HIP(hipStreamWaitEvent(cs, ex->ev_match, 0));
    ex->copy_covers_match = ex->match_pending;
    return ORBX_OK;
}

// Frame::ComputeStereoFromRGBD for every frame of a resident batch, for either form of the depth images: one launch behind the extraction, no host
// synchronisation.  `S` arrives with the form's own fields set and is given the ones both forms share.  mvuRight / mvDepth / the count of features
// with depth land in the rectified stage's result buffers, so the orbx_stereo_batch_download* calls serve both sources.  No pyramid level is read:
// level 0 is not materialised and the extractor keeps its single slab.
template <class Stage> int rgbd_stage(orbx_extractor *ex, Stage S, void (*kernel)(const Stage), const void *d_depth, size_t pitch_bytes,
                                      size_t frame_stride_bytes, float bf) {
    ORBX_HIP(hipSetDevice(ex->device));
    for (DevBuf *b : {&ex->d_st_ur, &ex->d_st_depth}) ORBX_TRY(b->ensure(4 * (size_t)ex->cap * ex->batch_cap));
    ORBX_TRY(ex->d_st_nm.ensure(4 * (size_t)ex->batch_cap));
    const hipStream_t st = stage_stream(ex);
    ORBX_TRY(stage_begin(st, {ex}, true));
    S.kps = (const orbx_keypoint *)ex->d_kps.p; S.kps_un = (const orbx_keypoint *)ex->match_kps();
    S.count = (const int32_t *)ex->d_count.p;
    S.depth = (const uint8_t *)d_depth; S.pitch = pitch_bytes; S.frame_stride = frame_stride_bytes;
    S.cap = ex->cap; S.width = ex->width; S.height = ex->height; S.bf = bf;
    S.u_right = (float *)ex->d_st_ur.p; S.out_depth = (float *)ex->d_st_depth.p; S.nmatches = (int32_t *)ex->d_st_nm.p;
    hipLaunchKernelGGL(kernel, dim3((unsigned)ex->last_batch), dim3(256), 0, st, S);
    ORBX_TRY(stage_end(st, {ex}));
    ex->st_seq = ex->batch_seq;   // (orbx_frame_load_stereo_batch: the results are this batch's)
    return ORBX_OK;
}

}  // namespace orbx

