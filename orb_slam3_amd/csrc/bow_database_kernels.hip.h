// bow_database_kernels.hip.h -- the BowVector of a resident handle and the brute-force query of the key-frame database (gfx950, wave64).
//
//   k_bow_vector   TemplatedVocabulary::transform's BowVector (TF_IDF, L1_NORM) from the per-feature word ids a handle keeps: addWeight per
//                  occurrence, then BowVector::normalize(L1)
//   k_bow_score    common words and L1Scoring::score of the query vector against every slot of an orbx_keyframe_database
//   k_bow_select   the first half of KeyFrameDatabase::DetectRelocalizationCandidates / DetectNBestCandidates: the maximum of the common-word counts,
//                  minCommonWords, and the slots above it in ascending order
//
// PARITY UNPINNED (include/orbx.h): the reference's arithmetic is restated there; what these kernels keep is its ORDER.  Every double sum runs as
// the reference's loop runs it -- one addition per occurrence of a word, the norm and the score in ascending word id on ONE lane's accumulator --
// because a tree or a per-lane partial sum differs from the sequential one in the last bit for most inputs.  No expression holds a multiply-add.
#pragma once

#include "matcher_kernels.hip.h"

namespace orbx {

constexpr uint32_t kNoWord = 0xffffffffu;   // the sort key of a stopped feature: behind every word id
constexpr int kBowVecTile = 4096;           // values of a BowVector that wait in LDS for the one lane that adds up the norm
constexpr int kBowVecLdsHead = 8 * kBowVecTile + 4 * 1024 + 16;   // the tile, the scan's sums, {norm, kept}: what precedes the sort keys (a multiple of 16)
constexpr int kBowQueryLds = 2048;          // words of a query vector k_bow_score stages in LDS (12 bytes each); a longer one is read through L2

// correctly rounded double division: what `/` is on gfx950 (v_div_scale / v_div_fmas / v_div_fixup) and on the host
__device__ __forceinline__ double bow_ddiv_rn(double a, double b) { return a / b; }

// The rows of a handle whose word ids k_bow_vector folds, and where the vector goes.  Features [0, N_left) are rows [0, N_left), features
// [N_left, N) rows [roff, roff + N_right) (a monocular handle: roff = cap, nr_host = 0).  nl_host / nr_host < 0: count[0] / count[1] read here.
struct BowVecSrc {
    const int32_t *count; int nl_host, nr_host, cap, roff;
    const int32_t *word;             // k_frame_bow_transform's word id per ROW
    const uint8_t *word_pos;         // [n_words] weight > 0
    const double *weight;            // [n_words] m_words[id]->weight
    int n_words;
    int32_t *out_word; double *out_val; int32_t *out_n;   // ascending word ids, their normalised values, how many
    int out_cap;                     // entries out_word / out_val hold (the host's bound on the features; nothing is written beyond)
};

// k_bow_vector: ONE workgroup.  The word ids of the unstopped features (an id outside [0, n_words) counts as stopped, as k_frame_featvec treats it)
// are sorted in LDS by a bitonic network; a scan numbers the places where a new word starts.  The thread that owns a start walks the run and adds w
// once per further occurrence (`vit->second += w`: count - 1 additions to w, NOT count * w).  The values pass through LDS a tile at a time, where
// lane 0 adds their magnitudes to the norm in ascending word id (`norm += fabs(value)` over the std::map); then every thread divides the values it
// wrote (`if (norm > 0.0) value /= norm`).  grid 1, block 1024, dynamic LDS kBowVecLdsHead + 4 * sort_cap (sort_cap: a power of two >= the features
// the call may see).
__global__ __launch_bounds__(1024) void k_bow_vector(const BowVecSrc S, int sort_cap) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    double *vals = reinterpret_cast<double *>(lds);
    int32_t *sums = reinterpret_cast<int32_t *>(lds + 8 * kBowVecTile);
    double *norm_s = reinterpret_cast<double *>(lds + 8 * kBowVecTile + 4096);
    int32_t *kept_s = reinterpret_cast<int32_t *>(lds + 8 * kBowVecTile + 4096 + 8);
    uint32_t *keys = reinterpret_cast<uint32_t *>(lds + kBowVecLdsHead);
    const int t = threadIdx.x;
    const int nl = S.nl_host >= 0 ? min(S.nl_host, S.roff) : min(max(S.count[0], 0), S.roff);
    const int nr = S.nr_host >= 0 ? min(S.nr_host, S.cap - S.roff) : min(max(S.count[1], 0), S.cap - S.roff);
    const int n = min(nl + nr, sort_cap);
    int p2 = 1;
    while (p2 < n) p2 <<= 1;
    if (t == 0) *kept_s = 0;
    for (int p = t; p < p2; p += 1024) {
        uint32_t key = kNoWord;
        if (p < n) {
            const int r = p < nl ? p : S.roff + p - nl;   // feature p's row
            const int w = S.word[r];
            if (w >= 0 && w < S.n_words && S.word_pos[w]) key = (uint32_t)w;
        }
        keys[p] = key;
    }
    __syncthreads();
    for (int k = 2; k <= p2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = t; p < p2; p += 1024) {
                const int q = p ^ j;
                if (q > p) {
                    const uint32_t a = keys[p], b = keys[q];
                    if ((a > b) == ((p & k) == 0)) { keys[p] = b; keys[q] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int p = t; p < p2; p += 1024)
        if (keys[p] != kNoWord && (p + 1 == p2 || keys[p + 1] == kNoWord)) *kept_s = p + 1;
    __syncthreads();
    const int kept = *kept_s;
    const int chunk = (p2 + 1023) / 1024, c0 = min(t * chunk, kept), c1 = min(c0 + chunk, kept);
    auto starts = [&](int p) { return p == 0 || keys[p] != keys[p - 1]; };
    int c = 0;
    for (int p = c0; p < c1; p++) c += starts(p) ? 1 : 0;
    sums[t] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {   // inclusive scan of the per-thread word starts
        const int v = t >= off ? sums[t - off] : 0;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    const int n_words_out = sums[1023], first = sums[t] - c;
    double norm = 0.0;   // lane 0's
    for (int base = 0; base < n_words_out; base += kBowVecTile) {
        int slot = first;
        for (int p = c0; p < c1; p++) {
            if (!starts(p)) continue;
            if (slot >= base && slot < base + kBowVecTile) {
                const uint32_t key = keys[p];
                const double w = S.weight[key];
                double v = w;
                for (int q = p + 1; q < kept && keys[q] == key; q++) v = __dadd_rn(v, w);
                vals[slot - base] = v;
                if (slot < S.out_cap) { S.out_word[slot] = (int32_t)key; S.out_val[slot] = v; }
            }
            slot++;
        }
        __syncthreads();
        if (t == 0) {
            const int m = min(n_words_out - base, kBowVecTile);
            for (int i = 0; i < m; i++) norm = __dadd_rn(norm, fabs(vals[i]));
        }
        __syncthreads();   // the next tile overwrites vals
    }
    if (t == 0) { *norm_s = norm; *S.out_n = min(n_words_out, S.out_cap); }
    __syncthreads();
    const double nm = *norm_s;
    if (nm > 0.0) {
        int slot = first;
        for (int p = c0; p < c1; p++) {
            if (!starts(p)) continue;
            if (slot < S.out_cap) S.out_val[slot] = bow_ddiv_rn(S.out_val[slot], nm);   // (this thread's own store above)
            slot++;
        }
    }
}

// The query of a database: the query's BowVector (k_bow_vector's, in the call's arena), the rows of the database, the slots left out.
struct BowQuery {
    const int32_t *q_word; const double *q_val; const int32_t *q_n; int q_cap;
    const int32_t *row_n;            // [n_slots] words of the slot's vector; < 0: the slot is empty
    const int32_t *row_word;         // [n_slots][words_cap] ascending word ids
    const double *row_val;           // [n_slots][words_cap]
    int n_slots, words_cap;
    const int32_t *exclude; int n_exclude;   // slot ids that are not counted (spConnectedKF)
    int32_t *common;                 // out [n_slots]: common words, -1 for an empty or excluded slot
    double *score;                   // out [n_slots]: L1Scoring::score(query, slot); 0 for a slot that is not counted
};

// One wave, one slot.  The lanes stride the slot's words and find each in the query by binary search; per chunk of 64 words the ballot of the
// hits gives the count, and the hits' terms (fabs(vi - wi) - fabs(vi)) - fabs(wi) are added to ONE running double in lane order -- ascending word id,
// the reference's merge order -- by a loop over the set bits that fetches each term with two readlanes.  score = -sum / 2.0, so no hit gives -0.0.
// Every index is bounded here: the slot by n_slots (the caller), the row's count by words_cap, the query's count by q_cap.
__device__ __forceinline__ void bow_score_wave(const BowQuery &Q, const int32_t *qw, const double *qv, int nq, int slot, int lane) {
    int rn = Q.row_n[slot];
    bool left_out = false;
    for (int e = lane; e < Q.n_exclude; e += 64) left_out |= Q.exclude[e] == slot;
    if (__ballot(left_out) != 0ull || rn < 0) {
        if (lane == 0) { Q.common[slot] = -1; Q.score[slot] = 0.0; }
        return;
    }
    rn = min(rn, Q.words_cap);
    const int32_t *rw = Q.row_word + (size_t)slot * (size_t)Q.words_cap;
    const double *rv = Q.row_val + (size_t)slot * (size_t)Q.words_cap;
    int common = 0;
    double sum = 0.0;
    for (int c0 = 0; c0 < rn; c0 += 64) {
        const int i = c0 + lane;
        bool hit = false;
        double term = 0.0;
        if (i < rn) {
            const int32_t w = rw[i];
            int lo = 0, hi = nq;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (qw[mid] < w) lo = mid + 1;
                else hi = mid;
            }
            if (lo < nq && qw[lo] == w) {
                const double vi = qv[lo], wi = rv[i];
                hit = true;
                term = (fabs(vi - wi) - fabs(vi)) - fabs(wi);
            }
        }
        u64 b = __ballot(hit);
        common += __popcll(b);
        const u64 bits = __builtin_bit_cast(u64, term);
        const int t_lo = (int)(uint32_t)bits, t_hi = (int)(uint32_t)(bits >> 32);
        while (b != 0ull) {
            const int l = __ffsll((long long)b) - 1;
            b &= b - 1ull;
            const u64 x = ((u64)(uint32_t)__builtin_amdgcn_readlane(t_hi, l) << 32) | (u64)(uint32_t)__builtin_amdgcn_readlane(t_lo, l);
            sum = __dadd_rn(sum, __builtin_bit_cast(double, x));
        }
    }
    if (lane == 0) { Q.common[slot] = common; Q.score[slot] = bow_ddiv_rn(-sum, 2.0); }
}
// grid ceil(n_slots / 4), block 256: a wave per slot; the query vector is staged in LDS when it has at most kBowQueryLds words
__global__ __launch_bounds__(256) void k_bow_score(const BowQuery Q) {
    __shared__ __attribute__((aligned(16))) double qv_s[kBowQueryLds];
    __shared__ __attribute__((aligned(16))) int32_t qw_s[kBowQueryLds];
    const int t = threadIdx.x, lane = t & 63;
    const int nq = min(max(*Q.q_n, 0), Q.q_cap);
    const bool staged = nq <= kBowQueryLds;
    if (staged)
        for (int i = t; i < nq; i += 256) { qw_s[i] = Q.q_word[i]; qv_s[i] = Q.q_val[i]; }
    __syncthreads();
    const int slot = (int)blockIdx.x * 4 + (t >> 6);
    if (slot >= Q.n_slots) return;
    if (staged) bow_score_wave(Q, qw_s, qv_s, nq, slot, lane);
    else bow_score_wave(Q, Q.q_word, Q.q_val, nq, slot, lane);
}

struct BowSelect {
    const int32_t *common; const double *score; int n_slots;
    float min_ratio;
    int32_t *cand_slot, *cand_common; double *cand_score; int cand_cap;
    int32_t *meta;                   // out [2]: candidates (also beyond cand_cap), maxCommonWords
};
// k_bow_select: ONE workgroup over all slots.  maxCommonWords over the counted slots, `int minCommonWords = maxCommonWords * 0.8f` (an int-to-float
// conversion, a float multiply, truncation), and the slots with more common words than that in ascending slot order, numbered by a workgroup scan: the
// list does not depend on scheduling.  A slot without a common word is never a candidate (the reference only lists key frames that share a word).
// grid 1, block 1024
__global__ __launch_bounds__(1024) void k_bow_select(const BowSelect S) {
    __shared__ int32_t sums[1024];
    const int t = threadIdx.x;
    const int chunk = (S.n_slots + 1023) / 1024, s0 = min(t * chunk, S.n_slots), s1 = min(s0 + chunk, S.n_slots);
    int mx = 0;
    for (int s = s0; s < s1; s++) mx = max(mx, S.common[s]);
    sums[t] = mx;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if (t < off) sums[t] = max(sums[t], sums[t + off]);
        __syncthreads();
    }
    const int max_common = sums[0];
    __syncthreads();
    const int min_common = (int)__fmul_rn((float)max_common, S.min_ratio);
    auto is_cand = [&](int s) { const int c = S.common[s]; return c > 0 && c > min_common; };
    int c = 0;
    for (int s = s0; s < s1; s++) c += is_cand(s) ? 1 : 0;
    sums[t] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = t >= off ? sums[t - off] : 0;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    int at = sums[t] - c;
    for (int s = s0; s < s1; s++) {
        if (!is_cand(s)) continue;
        if (at < S.cand_cap) { S.cand_slot[at] = s; S.cand_common[at] = S.common[s]; S.cand_score[at] = S.score[s]; }
        at++;
    }
    if (t == 1023) { S.meta[0] = sums[1023]; S.meta[1] = max_common; }
}

}  // namespace orbx
