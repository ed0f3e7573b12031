// pyr_stream.hip.h -- k_pyr_stream: levels 1 .. n-1 of the image pyramid (ORBextractor::ComputePyramid, /root/reference/src/ORBextractor.cc:1170-1195:
// cv::resize(INTER_LINEAR) of the level before + copyMakeBorder(REFLECT_101)) of a batch of frames in ONE launch, no hand-off between workgroups.
//
// Rounds 2-4 ran one launch per level (k_pyr_resize_march x 7): every level was written to HBM and read back by the next launch, each launch
// lasted as long as a wave's two dependent memory round trips, and seven drains sat on the main stream's critical path (252 us of a 944-us
// step for 657 MB: 0.33 of the HBM roofline).  Here a workgroup owns a BAND of a frame (the whole frame, or a half / quarter of its rows) and
// streams down it through all levels at once:
//   * the frame's rows enter an LDS ring ("level 0") through a ninth wave that does nothing else (sixteen bytes per lane and chunk);
//   * level l keeps its most recent rows in an LDS ring; in step s it produces the rows whose two source rows of level l - 1 were complete
//     after step s - 1 (all levels advance in the same step: ONE barrier per step, no barrier between levels);
//   * a row is computed once, stored once to the padded slab in HBM (plus its REFLECT_101 copies in the 19-row ring above / below) and once to
//     the LDS ring the next level reads; nothing is read back from HBM.
// The row schedule is a per-geometry table built on the host (build_pyr_stream, orbx_extractor.hip): the kernel holds no index arithmetic beyond
// "task -> LDS offsets".  A task = one wave x 64 dword columns x one or two output rows of one level (two rows share the horizontal pass of
// their common source row); every worker wave has its own list of them over all steps (PyrWaveList, PyrTask: orbx_internal.h), with the steps'
// barriers counted inside the list, so that the next task's descriptor and column entries can be fetched while this one is computed.  Bands of one frame overlap by the few rows the cascade needs (9 of 480 rows for two bands of a 752x480 frame);
// rows in the overlap are computed by both bands and stored by the one that owns them.
// Arithmetic = k_pyr_resize_march's ([OCV] resize INTER_LINEAR 8U: Q11 taps, horizontal sums >> 4, (b * H) >> 16 per source row, + 2 >> 2), bit for bit.
// grid xcd_grid(bands per frame, B), block 64 x (worker waves + 1: the loader wave), dynamic LDS = PyrStreamGeom::lds_bytes
#pragma once

namespace orbx {

// horizontal pass of one source row for the four pixels of a dword column: sums >> 4 ([OCV] the vertical pass multiplies (sum >> 4)).
// The column's 8 source bytes start at any byte of the row: three ALIGNED dwords + two v_alignbyte (measured: an 8-byte LDS read at an odd address
// costs the kernel 66 of 228 us -- the LDS serves it in pieces).
__device__ __forceinline__ void pyr_hpass(const uint32_t (&d)[3], const uint32_t osh, const uint32_t sel, const uint32_t selr, const uint32_t (&cc)[4], uint32_t (&H)[4]) {
    const uint32_t vx = __builtin_amdgcn_alignbyte(d[1], d[0], osh), vy = __builtin_amdgcn_alignbyte(d[2], d[1], osh);
    constexpr uint32_t kPair[4] = {0x0c040c00u, 0x0c050c01u, 0x0c060c02u, 0x0c070c03u};  // (left tap k, right tap k) as two u16
    const uint32_t l = __builtin_amdgcn_perm(vy, vx, sel), q = __builtin_amdgcn_perm(vy, vx, selr);
#pragma unroll
    for (int j = 0; j < 4; j++) H[j] = __builtin_amdgcn_udot2(as_pk(__builtin_amdgcn_perm(q, l, kPair[j])), as_pk(cc[j]), 0u, false) >> 4;
}
// vertical pass: (b0 * A >> 16) + (b1 * B >> 16) + 2 >> 2 per pixel, four pixels packed (see k_pyr_resize_march)
__device__ __forceinline__ uint32_t pyr_vpass(const uint32_t (&A)[4], const uint32_t (&B)[4], const uint32_t bb) {
    const uint32_t b0 = bb & 0xffffu, b1 = bb >> 16;
    int t[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t p0 = __umul24(A[j], b0) + 0x20000u, p1 = __umul24(B[j], b1);
        t[j] = (int)((p0 >> 16) + (p1 >> 16));
    }
    return ((uint32_t)(uint16_t)__builtin_amdgcn_ashr_pk_u8_i32(t[0], t[1], 2)) | ((uint32_t)(uint16_t)__builtin_amdgcn_ashr_pk_u8_i32(t[2], t[3], 2) << 16);
}
// the three aligned dwords of a source row that hold a column's 8 source bytes
__device__ __forceinline__ void pyr_row_read(const uint8_t *row4, uint32_t (&d)[3]) {
    const uint32_t *p = reinterpret_cast<const uint32_t *>(row4);
    d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
}
// a lane's PyrColumn of a column block (col = PyrTask::next_col: LDS offset of lane 0's entry | (live lanes - 1) << 16)
__device__ __forceinline__ void pyr_col_read(const uint8_t *smem, const uint32_t col, const int lane, uint2 &e0, uint32_t (&cc)[4]) {
    const uint8_t *e = smem + (col & 0xffffu) + (uint32_t)min(lane, (int)(col >> 16)) * 24u;
    e0 = *reinterpret_cast<const uint2 *>(e);
    const uint2 a = *reinterpret_cast<const uint2 *>(e + 8), b = *reinterpret_cast<const uint2 *>(e + 16);
    cc[0] = a.x; cc[1] = a.y; cc[2] = b.x; cc[3] = b.y;
}

// ---- a worker wave's descriptor fetch ----
// The 64 bytes of the NEXT task are requested by hand, at the one place of a task where the request costs nothing: after the task's LDS reads
// have returned and before its arithmetic.  LDS and scalar memory share one counter (lgkmcnt) and scalar loads return out of order, so a wait for
// LDS data with a descriptor in flight is a wait for the descriptor too (a round trip to L2: a band's lists are larger than the scalar cache);
// left to the compiler, the request sinks below the task's last store and its wait stands a dozen instructions later (round 6: 159 us per launch
// against 96 us of VALU issue).  The row dwords pass through the statement, which makes the compiler retire the LDS reads in front of it and keeps
// the arithmetic behind it; pyr_desc_wait() is the only place the descriptor's registers are touched again (tests/test_isa_pyr_stream.py walks
// the emitted code for both properties).
typedef uint32_t PyrDesc __attribute__((ext_vector_type(16)));
static_assert(sizeof(PyrDesc) == sizeof(PyrTask), "one descriptor = one s_load_dwordx16");
#if defined(__AMDGCN__)
#define PYR_ROW(d) "+v"(d[2])
#define PYR_DESC_FETCH(N, p, ra, rb, rc, rd) asm volatile("s_load_dwordx16 %[n], %[a], 0x0" : [n] "=s"(N), PYR_ROW(ra), PYR_ROW(rb), PYR_ROW(rc), PYR_ROW(rd) : [a] "s"(p) : "memory")
__device__ __forceinline__ void pyr_desc_wait(PyrDesc &N) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(N) : : "memory"); }
#else   // the CPU emulation build: a plain load
#define PYR_DESC_FETCH(N, p, ra, rb, rc, rd) N = *(p)
__device__ __forceinline__ void pyr_desc_wait(PyrDesc &) {}
#endif
enum { kPtSrc = 0, kPtB = 4, kPtGoff = 6, kPtMoff = 8, kPtDlds = 10, kPtNextCol = 12, kPtFlags = 13, kPtRoiLo = 14, kPtRoiN = 15 };   // dwords of PyrTask

// One task: C = its descriptor, (e0, cc) = its lanes' PyrColumn entries, both fetched during the wave's task before.  Requests the next task's
// column entries (ne0, ncc: a read-only table, so this may cross a step's barrier) and descriptor (N).
__device__ __forceinline__ void pyr_task(const PyrDesc &C, PyrDesc &N, const PyrDesc *next, const uint2 e0, const uint32_t (&cc)[4], uint2 &ne0, uint32_t (&ncc)[4],
                                         uint8_t *smem, uint8_t *slab, const int lane) {
    const uint32_t f = C[kPtFlags];
    const uint32_t base = e0.x & 0xfffcu, osh = e0.x & 3u, valid = e0.x >> 30, sel = e0.y, selr = e0.y + 0x01010101u;
    // every LDS operand of the task in ONE round trip: its source rows (a one-row task reads its second row three times: no branch in front of the
    // reads) and the next task's column entries
    uint32_t r0[3], r1[3], r2[3], r3[3], H0[4], H1[4], H2[4], H3[4];
    pyr_row_read(smem + C[kPtSrc + 0] + base, r0);
    pyr_row_read(smem + C[kPtSrc + 1] + base, r1);
    pyr_row_read(smem + C[kPtSrc + 2] + base, r2);
    pyr_row_read(smem + C[kPtSrc + 3] + base, r3);
    pyr_col_read(smem, C[kPtNextCol], lane, ne0, ncc);
    PYR_DESC_FETCH(N, next, r0, r1, r2, r3);
    pyr_hpass(r0, osh, sel, selr, cc, H0);
    pyr_hpass(r1, osh, sel, selr, cc, H1);
    uint32_t o0 = pyr_vpass(H0, H1, C[kPtB + 0]), o1 = 0u;
    if (f & kPyrTwoRows) {   // wave-uniform: three source rows (the middle one shared) or four (two independent pairs)
        pyr_hpass(r2, osh, sel, selr, cc, H2);
        if (f & kPyrFourSrc) {
            pyr_hpass(r3, osh, sel, selr, cc, H3);
            o1 = pyr_vpass(H2, H3, C[kPtB + 1]);
        } else {
            o1 = pyr_vpass(H1, H2, C[kPtB + 1]);
        }
    }
    if (valid != 1u) { o0 = 0u; o1 = 0u; }   // a dword past the ring's last pixel
    const bool live = (uint32_t)lane <= ((f >> 8) & 63u);
    const bool in_roi = (uint32_t)lane - C[kPtRoiLo] < C[kPtRoiN];   // this lane's dword belongs to the ROI row the next level reads
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (k == 1 && !(f & kPyrTwoRows)) break;
        const uint32_t o = k ? o1 : o0;
        if (live) {   // slab + (32-bit offset): the store takes the slab as its scalar base
            if (f & (kPyrStoreRow << k)) *reinterpret_cast<uint32_t *>(slab + (size_t)(C[kPtGoff + k] + 4u * (uint32_t)lane)) = o;   // wave-uniform conditions
            if (f & (kPyrStoreCopy << k)) *reinterpret_cast<uint32_t *>(slab + (size_t)(C[kPtMoff + k] + 4u * (uint32_t)lane)) = o;
        }
        if (in_roi) *reinterpret_cast<uint32_t *>(smem + (uint32_t)(C[kPtDlds + k] + 4u * (uint32_t)lane)) = o;
    }
}

__global__ __launch_bounds__(1024) void k_pyr_stream(const PyrStreamGeom G, const uint4 *__restrict__ xg24, const PyrStep *__restrict__ steps,
                                                                   const PyrTask *__restrict__ tasks, const PyrWaveList *__restrict__ lists,
                                                                   const uint8_t *__restrict__ img, size_t row_stride, size_t frame_stride,
                                                                   uint8_t *__restrict__ pyr, size_t pyr_frame_stride, int32_t *__restrict__ zero_word, int n_frames) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int band, f;
    if (!xcd_frame_map(n_frames, &band, &f)) return;   // the bands of a frame stay on one XCD (their overlap rows hit its L2)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NW = (int)G.workers;   // worker waves (the block has one wave more: the loader)
    if (zero_word && band == 0 && f == 0 && tid == 0) *zero_word = 0;   // the FAST stage's overflow counter of this batch (k_pyr_base's side job)
    for (uint32_t i = (uint32_t)tid; i < G.xg_bytes / 16u; i += 64u * (G.workers + 1u)) reinterpret_cast<uint4 *>(smem)[i] = xg24[i];
    const PyrStep *st = steps + (size_t)band * G.steps_per_band;
    __syncthreads();
    if (wave == NW) {
        // ---- the loader wave: the frame rows of every step into the LDS ring, 16 bytes per lane and chunk.  A wave of its own because a wave's
        // memory operations retire in order: a worker that had requested frame rows would have to wait for every store it issued after them
        // (s_waitcnt vmcnt counts both) before it could hand the rows to LDS -- the workers below never wait for memory at all.
        const uint8_t *frame = img + (size_t)f * frame_stride;
        // chunk i of a step = (row i / cpr0, 16-byte chunk i % cpr0); the last chunk of a row is pulled back to end at the row's last pixel
        for (uint32_t s = 0; s < G.steps_per_band; s++) {
            const PyrStep d = st[s];
            const uint32_t y0 = d.y0_rows & 0xffffu, nrows = d.y0_rows >> 16;
            uint4 stg[kPyrStreamStage];
#pragma unroll
            for (int j = 0; j < kPyrStreamStage; j++) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (64u * (uint32_t)j < nrows * G.cpr0) {   // wave-uniform
                    const uint32_t i = (uint32_t)lane + 64u * (uint32_t)j, row = __umulhi(i, G.cpr0_rcp);
                    const uint32_t x = min((i - row * G.cpr0) * 16u, (uint32_t)G.w0 - 16u);
                    __builtin_memcpy(&v, frame + (size_t)(y0 + min(row, nrows - 1u)) * row_stride + x, 16);
                }
                stg[j] = v;
            }
#pragma unroll
            for (int j = 0; j < kPyrStreamStage; j++) {
                const uint32_t i = (uint32_t)lane + 64u * (uint32_t)j, row = __umulhi(i, G.cpr0_rcp);
                if (64u * (uint32_t)j < nrows * G.cpr0 && row < nrows) {
                    const uint32_t x = min((i - row * G.cpr0) * 16u, (uint32_t)G.w0 - 16u);
                    uint32_t slot = d.slot0 + row;
                    if (slot >= G.ring0_rows) slot -= G.ring0_rows;
                    const uint4 v = stg[j];
                    __builtin_memcpy(smem + G.ring0_off + slot * G.ring0_pitch + x, &v, 16);
                }
            }
            __syncthreads();
        }
        return;
    }
    // ---- the worker waves: each works through its own list of tasks (PyrWaveList), two descriptor sets and two sets of column entries in turn:
    // while task t is computed, the descriptor of t + 1 is on its way and the column entries of t + 1 sit in registers ----
    uint8_t *slab = pyr + (size_t)f * pyr_frame_stride;
    const PyrWaveList wl = lists[(size_t)band * G.workers + (uint32_t)wave];
    for (uint32_t b = wl.lead; b; b--) __syncthreads();
    if (wl.n == 0u) return;
    const PyrDesc *p = reinterpret_cast<const PyrDesc *>(tasks) + wl.first;
    PyrDesc A = *p, B;
    uint2 ea, eb;
    uint32_t ca[4], cb[4];
    pyr_col_read(smem, wl.col0, lane, ea, ca);
    for (uint32_t n = wl.n;;) {
        pyr_task(A, B, ++p, ea, ca, eb, cb, smem, slab, lane);
        for (uint32_t b = A[kPtFlags] >> 16; b; b--) __syncthreads();
        pyr_desc_wait(B);
        if (--n == 0u) break;
        pyr_task(B, A, ++p, eb, cb, ea, ca, smem, slab, lane);
        for (uint32_t b = B[kPtFlags] >> 16; b; b--) __syncthreads();
        pyr_desc_wait(A);
        if (--n == 0u) break;
    }
}

}  // namespace orbx
