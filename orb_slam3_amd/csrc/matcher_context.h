// matcher_context.h -- the per-thread matcher context (orbx_matcher): its own HIP stream, the grow-on-demand device arena a call's buffers are carved
// from, the pinned staging and the transfer functions every entry point of orbx_matcher.hip moves its data with.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "matcher_kernels.hip.h"
#include "extractor_state.h"   // orbx::Layout, the layout primitive of the arena (Carve) and of the resident allocations, comes from there

namespace orbx {

struct Arena {  // one device buffer, handed out anew on every call (Carve)
    uint8_t *base = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return ORBX_OK;
        if (base) (void)hipFree(base);
        base = nullptr; cap = 0;
        bytes = (bytes * 3 / 2 + 4095) & ~(size_t)4095;
        ORBX_HIP(hipMalloc((void **)&base, bytes));
        cap = bytes;
        return ORBX_OK;
    }
};

}  // namespace orbx

// Pinned host staging of a matcher context.  No entry point ever hands a CALLER'S (pageable) pointer to the HIP runtime: uploads are
// memcpy'd into this arena first, downloads land here and are memcpy'd out after the stream synchronisation.  (The runtime's
// alternative for pageable memory is to pin the caller's pages on the fly for the duration of the DMA; keeping that machinery out of
// the hot path removes a whole class of lifetime hazards -- stack temporaries, vectors freed right after the call -- and is faster
// for the small transfers these entry points make.)
struct PinnedArena {
    uint8_t *base = nullptr;
    size_t cap = 0, used = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return ORBX_OK;
        if (base) (void)hipHostFree(base);
        base = nullptr; cap = 0;
        bytes = (bytes * 3 / 2 + 4095) & ~(size_t)4095;
        // coherent (fine-grained) whatever HIP_HOST_COHERENT says: k_xfer's lanes read the staged inputs from and write the results into this block
        // themselves, and the host reads them right after the stream synchronisation (as the extractor's h_stage, extractor_state.h)
        ORBX_HIP(hipHostMalloc((void **)&base, bytes, hipHostMallocCoherent));
        cap = bytes;
        return ORBX_OK;
    }
    void reset() { used = 0; }
    void *take(size_t bytes) {
        used = (used + 63) & ~(size_t)63;
        if (used + bytes > cap) return nullptr;
        void *p = base + used;
        used += bytes;
        return p;
    }
};

struct orbx_matcher {
    int device = 0;
    hipStream_t stream = nullptr;
    orbx::Arena arena;
    PinnedArena stage;
    // Transfers of ONE call are coalesced (round 5) and issued as KERNEL work (round 6).  `mirror` is a pinned, device-visible image of the device arena: an
    // upload to arena offset o is staged at mirror offset o and only RECORDED; exec() -- the stream as every launch, fill and download of a call obtains it --
    // first issues the recorded uploads and fills: every run of arena-adjacent buffers (adjacent = nothing but the layout's alignment padding between them, which
    // no buffer owns) is one op of a k_xfer launch whose lanes read the mirror themselves (runs above kKernelXferMax: one hipMemcpyAsync).  Downloads from the
    // arena are recorded the same way and issued as runs by deliver(): a k_xfer launch that writes the mirror.  Round 4: 14 uploads and 2 downloads of
    // 4 B .. 32 KB per projection-matcher call, each a DMA submission (~5 us); round 5: 1 + 1 DMA submissions; now none -- the call's work is one in-order
    // chain of launches in the compute queue, no hand-over to a DMA engine and back.  Transfers whose device side is not in the arena take the direct path.
    PinnedArena mirror;
    struct Span { size_t off, bytes; };
    std::vector<Span> uploads;      // recorded, not yet issued (ascending offsets: the arena is a bump allocator)
    std::vector<Span> issued;       // mirror ranges a transfer issued since the last synchronisation may still read: not staged over (such an upload goes direct)
    struct Fill { size_t off, bytes; uint32_t value; };
    std::vector<Fill> fills;        // recorded fills of arena ranges, issued with the uploads
    struct Pending { void *dst; const void *src; size_t bytes; };
    std::vector<Pending> pending;   // downloads waiting in pinned memory for the stream synchronisation
    struct Down { void *dst; size_t off, bytes; };
    std::vector<Down> downloads;    // recorded downloads from the arena (issued by deliver())
    std::vector<Down> direct;       // results a kernel wrote straight into the mirror (host_view): handed out after the synchronisation, no transfer
    hipError_t xfer_err = hipSuccess;
    int64_t xfers[6] = {0, 0, 0, 0, 0, 0};   // transfer submissions (runs) up / down and their bytes since begin(); [4] of them by a DMA engine, [5] k_xfer launches
    bool kernel_xfer = true;                 // ORBX_MATCHER_DMA=1: every run by hipMemcpyAsync, fills by hipMemsetAsync (round 5's transport, for A/B)
    bool brute_windows = true;               // ORBX_MATCHER_BRUTE=0: small single calls build the grid as large ones do (A/B)
    bool dirty = false;                      // something was enqueued since the last synchronisation
    int32_t replay_stats[3] = {0, 0, 0};     // k_replay_init_lists of the last orbx_search_for_initialization: rounds, whole-wave re-scans, queries
    static constexpr size_t kPadGap = 255;   // Layout::add aligns to 256
    static constexpr size_t kKernelXferMax = (size_t)1 << 20;
    // Fixed slack behind the last buffer of every call (the largest any call's size carried while the sizes were still summed by hand).
    static constexpr size_t kArenaTail = 64 * 256 + 4096;
    // A call's device scratch: `layout(A)` names every buffer of the call once, in arena order -- A.take<T>(n), A.up(src, n) -- and the call's size is
    // the sum of those statements (+ kArenaTail), nothing else.  The layout runs twice: a sizing pass (it only adds up; every pointer it hands out is
    // NULL and nothing is staged), then reserve_all() + begin(), then the pass that hands out the addresses and stages the uploads.  So a layout reads
    // its pointers only to store them, and leaves arithmetic on them to the code behind carve().
    template <class F> int carve(F &&layout);
    // a call without device scratch whose transfers go through the pinned staging (resident buffers on the device side): room for `bytes` of them
    int reserve_staging(size_t bytes);
    // device scratch for one call + staging for everything that call can move in either direction
    int reserve_all(size_t device_bytes) {
        if (dirty) { (void)hipStreamSynchronize(stream); dirty = false; }   // a call that failed between exec() and deliver(): nothing of it may still read what is re-allocated here
        int r = arena.reserve(device_bytes);
        if (r != ORBX_OK) return r;
        r = mirror.reserve(arena.cap);
        if (r != ORBX_OK) return r;
        return stage.reserve(2 * device_bytes + 65536);
    }
    // begin() follows a synchronisation of the previous call: every entry point ends in deliver(); one that returned between exec() and deliver() (a failed
    // launch, an exhausted staging arena) left `dirty` set and is waited for here, before its mirror ranges are staged over
    void begin() {
        if (dirty) { (void)hipStreamSynchronize(stream); dirty = false; }
        stage.reset(); pending.clear(); uploads.clear(); downloads.clear(); direct.clear(); issued.clear(); fills.clear(); xfer_err = hipSuccess;
        for (int64_t &x : xfers) x = 0;
    }
    bool in_arena(const void *p, size_t bytes) const {
        const uint8_t *q = static_cast<const uint8_t *>(p);
        return arena.base && q >= arena.base && q + bytes <= arena.base + arena.cap && arena.cap <= mirror.cap;
    }
    bool stageable(const void *p, size_t bytes) const {   // an upload that may be staged in the mirror
        if (!in_arena(p, bytes)) return false;
        const size_t o = (size_t)(static_cast<const uint8_t *>(p) - arena.base);
        for (const Span &q : issued)
            if (o < q.off + q.bytes && q.off < o + bytes) return false;
        return true;
    }
    void note(hipError_t e) { if (e != hipSuccess && xfer_err == hipSuccess) xfer_err = e; }
    // DIRECT access (round 6): a purely streaming kernel (every input read once, every output written once: k_in_frustum) is handed the MIRROR's addresses
    // of its arena buffers -- its lanes read the staged inputs over the host link and write the results into host memory themselves: one launch per call
    // instead of three (k_xfer, kernel, k_xfer).  host_view(p) = the mirror address of arena buffer p; stage_direct copies an input there without recording an
    // upload; result_direct registers an output for deliver().
    template <class T> T *host_view(T *p) const { return reinterpret_cast<T *>(mirror.base + (reinterpret_cast<const uint8_t *>(p) - arena.base)); }
    bool direct_ok(size_t total_bytes) const { return kernel_xfer && total_bytes <= kKernelXferMax * 2; }
    void stage_direct(void *arena_dst, const void *src, size_t bytes) { memcpy(host_view(static_cast<uint8_t *>(arena_dst)), src, bytes); }
    void result_direct(void *dst, const void *arena_src, size_t bytes) {
        direct.push_back(Down{dst, (size_t)(static_cast<const uint8_t *>(arena_src) - arena.base), bytes});
    }
    void record_upload(size_t o, size_t bytes) {   // staged in the mirror at offset o by the caller
        for (const Fill &f : fills)
            if (o < f.off + f.bytes + 16 && f.off < o + bytes + 16) { flush_uploads(); break; }   // never reorder an upload and a fill of one range
        uploads.push_back(Span{o, bytes});
    }
    void launch_xfer(const orbx::XferOps &X, uint32_t max_units) {
        const uint32_t grid = std::min<uint32_t>(1024u, (max_units + 255u) / 256u);
        hipLaunchKernelGGL(orbx::k_xfer, dim3(grid ? grid : 1), dim3(256), 0, stream, X);
        note(hipGetLastError());
        xfers[5]++;
    }
    // one more op of a k_xfer launch under construction (a full one is launched first); bytes are rounded up to k_xfer's 16-byte units
    void append_op(orbx::XferOps &X, uint32_t &max_units, uint8_t *dst, const uint8_t *src, size_t bytes, uint32_t value) {
        if (X.n == orbx::kMaxXferOps) { launch_xfer(X, max_units); X.n = 0; max_units = 0; }
        const uint32_t units = (uint32_t)((bytes + 15) / 16);
        X.op[X.n++] = orbx::XferOp{dst, src, units, value};
        max_units = std::max(max_units, units);
    }
    // a fill of an arena range, issued with the call's uploads (the device side of the range must not be the target of a recorded upload)
    hipError_t fill(void *dst, int value, size_t bytes) {
        if (bytes == 0) return hipSuccess;
        const size_t o = (size_t)(static_cast<const uint8_t *>(dst) - arena.base);
        if (kernel_xfer && in_arena(dst, bytes) && (o & 15) == 0) {
            for (const Span &u : uploads)
                if (o < u.off + u.bytes + 16 && u.off < o + bytes + 16) { flush_uploads(); break; }   // never reorder a fill and an upload of one range
            fills.push_back(Fill{o, bytes, (uint32_t)(value & 0xff)});
            return hipSuccess;
        }
        dirty = true;
        return hipMemsetAsync(dst, value, bytes, exec());
    }
    void flush_uploads() {
        std::sort(uploads.begin(), uploads.end(), [](const Span &a, const Span &b) { return a.off < b.off; });   // (a record uploaded after its buffers were taken lies between them)
        orbx::XferOps X;
        X.n = 0;
        uint32_t max_units = 0;
        size_t i = 0;
        while (i < uploads.size()) {
            const size_t b = uploads[i].off;
            size_t e = b + uploads[i].bytes, j = i + 1;
            while (j < uploads.size() && uploads[j].off <= e + kPadGap) { e = std::max(e, uploads[j].off + uploads[j].bytes); j++; }
            if (kernel_xfer && e - b <= kKernelXferMax && (b & 15) == 0) {
                append_op(X, max_units, arena.base + b, mirror.base + b, e - b, 0);   // (rounded up to 16 bytes: alignment padding at most, the next buffer starts on a multiple of 256)
            } else {
                note(hipMemcpyAsync(arena.base + b, mirror.base + b, e - b, hipMemcpyHostToDevice, stream));
                xfers[4]++;
            }
            xfers[0]++; xfers[2] += (int64_t)(e - b);
            issued.push_back(Span{b, e - b});
            i = j;
        }
        uploads.clear();
        for (const Fill &f : fills) append_op(X, max_units, arena.base + f.off, nullptr, f.bytes, f.value);
        fills.clear();
        if (X.n) launch_xfer(X, max_units);
        dirty = true;
    }
    // the stream for anything that consumes the call's uploads (kernel launches, memsets, downloads, the synchronisation)
    hipStream_t exec() {
        if (!uploads.empty() || !fills.empty()) flush_uploads();
        dirty = true;
        return stream;
    }
    // issue the recorded downloads (runs of arena-adjacent buffers), wait for the stream, hand the bytes to the caller's buffers
    hipError_t deliver() {
        (void)exec();
        std::sort(downloads.begin(), downloads.end(), [](const Down &a, const Down &b) { return a.off < b.off; });
        orbx::XferOps X;
        X.n = 0;
        uint32_t max_units = 0;
        size_t i = 0;
        while (i < downloads.size()) {
            const size_t b = downloads[i].off;
            size_t e = b + downloads[i].bytes, j = i + 1;
            while (j < downloads.size() && downloads[j].off <= e + kPadGap) { e = std::max(e, downloads[j].off + downloads[j].bytes); j++; }
            if (kernel_xfer && e - b <= kKernelXferMax && (b & 15) == 0) {
                append_op(X, max_units, mirror.base + b, arena.base + b, e - b, 0);
            } else {
                note(hipMemcpyAsync(mirror.base + b, arena.base + b, e - b, hipMemcpyDeviceToHost, stream));
                xfers[4]++;
            }
            xfers[1]++; xfers[3] += (int64_t)(e - b);
            i = j;
        }
        if (X.n) launch_xfer(X, max_units);
        note(hipStreamSynchronize(stream));
        dirty = false;
        if (xfer_err == hipSuccess) {
            for (const Down &d : downloads) memcpy(d.dst, mirror.base + d.off, d.bytes);
            for (const Down &d : direct) memcpy(d.dst, mirror.base + d.off, d.bytes);
            for (const Pending &q : pending) memcpy(q.dst, q.src, q.bytes);
        }
        downloads.clear();
        direct.clear();
        pending.clear();
        issued.clear();
        return xfer_err;
    }
    // host -> device.  Into the arena: staged in the mirror and recorded, issued with its arena neighbours by exec(); anywhere else: a copy of its own
    int h2d(void *dst, const void *src, size_t bytes) {
        if (bytes == 0) return ORBX_OK;
        if (stageable(dst, bytes)) {
            const size_t o = (size_t)(static_cast<const uint8_t *>(dst) - arena.base);
            memcpy(mirror.base + o, src, bytes);
            record_upload(o, bytes);
            return ORBX_OK;
        }
        void *s = stage.take(bytes);
        if (!s) { orbx::set_error("staging arena exhausted"); return ORBX_E_INTERNAL; }
        memcpy(s, src, bytes);
        dirty = true;
        ORBX_HIP(hipMemcpyAsync(dst, s, bytes, hipMemcpyHostToDevice, stream));
        xfers[0]++; xfers[2] += (int64_t)bytes; xfers[4]++;
        return ORBX_OK;
    }
    // device -> host, handed to `dst` by sync_and_deliver().  From the arena: recorded, issued with its arena neighbours by deliver()
    int d2h(void *dst, const void *src, size_t bytes) {
        if (bytes == 0) return ORBX_OK;
        if (in_arena(src, bytes)) {
            downloads.push_back(Down{dst, (size_t)(static_cast<const uint8_t *>(src) - arena.base), bytes});
            return ORBX_OK;
        }
        void *s = stage.take(bytes);
        if (!s) { orbx::set_error("staging arena exhausted"); return ORBX_E_INTERNAL; }
        ORBX_HIP(hipMemcpyAsync(s, src, bytes, hipMemcpyDeviceToHost, exec()));
        xfers[1]++; xfers[3] += (int64_t)bytes; xfers[4]++;
        pending.push_back(Pending{dst, s, bytes});
        return ORBX_OK;
    }
    int sync_and_deliver() {
        ORBX_HIP(deliver());
        return ORBX_OK;
    }
    // Upload staged ranges of a RESIDENT allocation (a frame handle, a key frame: not the arena): range k lies at ranges[k].off of `stage` as of `dev`.
    // One k_xfer launch in this context's queue (ORBX_MATCHER_DMA=1: one copy per range by the DMA engine), one upload run per range in `xfers`.
    int upload_ranges(uint8_t *dev, const uint8_t *staged, const Span *ranges, int n) {
        orbx::XferOps X;
        X.n = 0;
        uint32_t max_units = 0;
        for (int k = 0; k < n; k++) {
            const Span &r = ranges[k];
            if (!r.bytes) continue;
            if (kernel_xfer && r.bytes <= kKernelXferMax) {
                append_op(X, max_units, dev + r.off, staged + r.off, r.bytes, 0);   // (rounded up to 16 bytes: inside the region's 256-byte padding)
            } else {
                note(hipMemcpyAsync(dev + r.off, staged + r.off, r.bytes, hipMemcpyHostToDevice, stream));
                xfers[4]++;
            }
            xfers[0]++; xfers[2] += (int64_t)r.bytes;
        }
        if (X.n) launch_xfer(X, max_units);
        if (xfer_err != hipSuccess) { orbx::set_error(hipGetErrorString(xfer_err)); return ORBX_E_HIP; }
        return ORBX_OK;
    }
};

// The buffers of one call, declared in arena order (orbx_matcher::carve).
struct Carve {
    orbx_matcher *m;
    bool sizing;
    orbx::Layout L;
    int err = ORBX_OK;
    // n elements of T, device only (or uploaded later by orbx_matcher::h2d)
    template <class T> T *take(size_t n) {
        const size_t o = L.add(n * sizeof(T));
        return sizing ? nullptr : reinterpret_cast<T *>(m->arena.base + o);
    }
    // n + extra elements, the first n uploaded from src (src NULL: nothing is uploaded)
    template <class T> T *up(const T *src, size_t n, size_t extra = 0) {
        T *d = take<T>(n + extra);
        if (!sizing && src && err == ORBX_OK) err = m->h2d(d, src, n * sizeof(T));
        return d;
    }
    // an optional input: no buffer at all without src
    template <class T> T *up_opt(const T *src, size_t n) { return src ? up(src, n) : nullptr; }
};

template <class F> int orbx_matcher::carve(F &&layout) {
    Carve S{this, true};
    layout(S);
    const int r = reserve_all(S.L.used + kArenaTail);
    if (r != ORBX_OK) return r;
    begin();
    Carve A{this, false};
    layout(A);
    if (A.L.used != S.L.used) { orbx::set_error("a layout declared different buffers in its two passes"); return ORBX_E_INTERNAL; }
    return A.err;
}

inline int orbx_matcher::reserve_staging(size_t bytes) {   // (the staging is sized by the call's device bytes: reserve_all)
    return carve([&](Carve &A) { A.take<uint8_t>(bytes); });
}
