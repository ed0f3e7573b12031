// The BowVector of resident handles and the key-frame database -- orbx_frame_bow_vector, orbx_keyframe_bow_vector, orbx_keyframe_database_create /
// _add / _erase / _clear / _query_frame / _query_keyframe / _destroy -- against DBoW2's BowVector::addWeight + normalize(L1), L1Scoring::score and the
// first half of KeyFrameDatabase::DetectRelocalizationCandidates / DetectNBestCandidates restated below with std::map<unsigned, double> (the
// reference's container: ascending word ids, sequential double sums).  Two vocabularies (27 words, every word many times; 512 words), a monocular
// query frame, monocular key frames and one fisheye-stereo key frame, slots with gaps, an exclude list, a truncated candidate list, erase / re-add /
// clear.  Doubles are compared by their bits.  Every output array is a heap block of exactly the needed size filled with a sentinel; refused calls
// leave them and the transfer counters alone.
// Stand-alone, against include/orbx.h only: linked against the emulator build of the library (python tests/simt/build.py --asan --static-rt) and
// compiled with -fsanitize=address,undefined, as tests/cpp/keyframe_distinctive_check.cpp.  Prints "keyframe database ok" and returns 0.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <vector>

#include "../../include/orbx.h"

namespace {

constexpr int kLevels = 8, kLevelsUp = 2;
bool g_max_moved = false;   // an exclusion lowered maxCommonWords in at least one run

#define MUST(expr)                                                                   \
    do {                                                                             \
        const int r_ = (expr);                                                       \
        if (r_ < 0) { printf("%s: %d %s\n", #expr, r_, orbx_last_error()); return 1; } \
    } while (0)
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

typedef std::map<unsigned, double> BowVector;

// TemplatedVocabulary::transform's BowVector half (TF_IDF, L1_NORM) from the word ids of the features
BowVector bow_vector(const std::vector<int32_t> &words, const std::vector<double> &weight) {
    BowVector v;
    for (int32_t id : words) {
        const double w = weight[(size_t)id];
        if (w > 0) {
            BowVector::iterator vit = v.lower_bound((unsigned)id);                         // BowVector::addWeight
            if (vit != v.end() && !(v.key_comp()((unsigned)id, vit->first))) vit->second += w;
            else v.insert(vit, BowVector::value_type((unsigned)id, w));
        }
    }
    double norm = 0.0;                                                                     // BowVector::normalize(L1)
    for (BowVector::iterator it = v.begin(); it != v.end(); ++it) norm += fabs(it->second);
    if (norm > 0.0)
        for (BowVector::iterator it = v.begin(); it != v.end(); ++it) it->second /= norm;
    return v;
}

// L1Scoring::score(v1, v2), and the words both hold
double l1_score(const BowVector &v1, const BowVector &v2, int *common) {
    BowVector::const_iterator v1_it = v1.begin(), v2_it = v2.begin();
    const BowVector::const_iterator v1_end = v1.end(), v2_end = v2.end();
    double score = 0;
    *common = 0;
    while (v1_it != v1_end && v2_it != v2_end) {
        const double &vi = v1_it->second, &wi = v2_it->second;
        if (v1_it->first == v2_it->first) {
            score += fabs(vi - wi) - fabs(vi) - fabs(wi);
            ++*common; ++v1_it; ++v2_it;
        } else if (v1_it->first < v2_it->first) {
            v1_it = v1.lower_bound(v2_it->first);
        } else {
            v2_it = v2.lower_bound(v1_it->first);
        }
    }
    return -score / 2.0;
}

struct Expected { std::vector<int32_t> common; std::vector<double> score; int max_common = 0; std::vector<int32_t> cand; };

Expected expected(const BowVector &q, const std::map<int, BowVector> &slots, int n_slots, const std::vector<int32_t> &exclude, float min_ratio) {
    Expected e;
    e.common.assign((size_t)n_slots, -1); e.score.assign((size_t)n_slots, 0.0);
    for (const auto &s : slots) {
        if (std::find(exclude.begin(), exclude.end(), s.first) != exclude.end()) continue;
        int c = 0;
        e.score[(size_t)s.first] = l1_score(q, s.second, &c);
        e.common[(size_t)s.first] = c;
        e.max_common = std::max(e.max_common, c);
    }
    const int min_common = e.max_common * min_ratio;   // int minCommonWords = maxCommonWords * 0.8f
    for (int s = 0; s < n_slots; s++)
        if (e.common[(size_t)s] > 0 && e.common[(size_t)s] > min_common) e.cand.push_back(s);
    return e;
}

bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

struct Vocabulary {
    int L = 0;
    std::vector<int32_t> child_ptr, child_idx, word_id;
    std::vector<uint8_t> node_desc;
    std::vector<double> weight;
    orbx_vocabulary *dev = nullptr;
};

// a full k-ary tree of depth L with random node descriptors; a tenth of the words stopped (weight 0 or negative)
int make_vocabulary(std::mt19937 &rng, int k, int L, Vocabulary &V) {
    V.L = L;
    std::vector<int> depth{0};
    V.child_ptr.push_back(0);
    for (size_t i = 0; i < depth.size(); i++) {
        if (depth[i] < L)
            for (int c = 0; c < k; c++) { V.child_idx.push_back((int32_t)depth.size()); depth.push_back(depth[i] + 1); }
        V.child_ptr.push_back((int32_t)V.child_idx.size());
    }
    int words = 0;
    for (size_t i = 0; i < depth.size(); i++) V.word_id.push_back(depth[i] == L ? words++ : -1);
    for (size_t i = 0; i < 32 * depth.size(); i++) V.node_desc.push_back((uint8_t)rng());
    for (int w = 0; w < words; w++) {
        const unsigned r = rng() % 20;
        V.weight.push_back(r == 0 ? 0.0 : r == 1 ? -1.0 : 0.2 + (double)(rng() % 1000000) / 357913.0);
    }
    MUST(orbx_vocabulary_create(0, L, (int)depth.size(), V.child_ptr.data(), V.child_idx.data(), V.node_desc.data(), V.word_id.data(), &V.dev));
    MUST(orbx_vocabulary_set_word_weights(V.dev, V.weight.data(), words));
    return 0;
}

struct Rows { std::vector<orbx_keypoint> kps; std::vector<uint8_t> desc; };

// n features whose descriptors are leaf descriptors of the vocabulary with a few bits flipped
void make_rows(std::mt19937 &rng, const Vocabulary &V, int n, Rows &R) {
    std::vector<int> leaves;
    for (size_t i = 0; i < V.word_id.size(); i++) if (V.word_id[i] >= 0) leaves.push_back((int)i);
    for (int i = 0; i < n; i++) {
        orbx_keypoint kp;
        memset(&kp, 0, sizeof(kp));
        kp.x = 1.f + (float)(rng() % 600); kp.y = 1.f + (float)(rng() % 400); kp.octave = (int)(rng() % kLevels); kp.size = 31.f; kp.class_id = -1;
        R.kps.push_back(kp);
        const uint8_t *b = V.node_desc.data() + 32 * (size_t)leaves[rng() % leaves.size()];
        for (int j = 0; j < 32; j++) R.desc.push_back(b[j]);
        for (int f = 0; f < 12; f++) { const unsigned bit = rng() % 256; R.desc[R.desc.size() - 32 + bit / 8] ^= (uint8_t)(1u << (bit % 8)); }
    }
}

orbx_frame_desc frame_desc(const Rows &R, int n, const float *scale) {
    orbx_frame_desc d;
    memset(&d, 0, sizeof(d));
    d.keypoints_un = R.kps.data(); d.descriptors = R.desc.data(); d.n = n;
    d.min_x = 0.f; d.max_x = 640.f; d.min_y = 0.f; d.max_y = 480.f; d.scale_factors = scale; d.nlevels = kLevels;
    return d;
}

// one BowVector call into heap blocks of exactly `room` entries: the vector equals `want` bit for bit
template <class Call> int check_vector(Call call, size_t room, const BowVector &want) {
    std::unique_ptr<int32_t[]> ids(new int32_t[std::max<size_t>(room, 1)]);
    std::unique_ptr<double[]> val(new double[std::max<size_t>(room, 1)]);
    int n = -5;
    MUST(call(ids.get(), val.get(), &n));
    CHECK(n == (int)want.size());
    int i = 0;
    for (const auto &e : want) { CHECK(ids[i] == (int32_t)e.first); CHECK(same_bits(val[i], e.second)); i++; }
    return 0;
}

// one query into exact-size heap blocks, compared with the restatement
template <class Call> int check_query(Call call, const Expected &e, int n_slots, int cand_cap) {
    const size_t ns = (size_t)n_slots, cc = (size_t)std::max(cand_cap, 1);
    std::unique_ptr<int32_t[]> common(new int32_t[ns]), cs(new int32_t[cc]), ccm(new int32_t[cc]);
    std::unique_ptr<double[]> score(new double[ns]), csc(new double[cc]);
    for (size_t i = 0; i < cc; i++) { cs[i] = -7; ccm[i] = -7; csc[i] = 7.0; }
    int n_cand = -5, max_common = -5;
    MUST(call(common.get(), score.get(), cs.get(), ccm.get(), csc.get(), cand_cap, &n_cand, &max_common));
    CHECK(n_cand == (int)e.cand.size() && max_common == e.max_common);
    for (size_t s = 0; s < ns; s++) { CHECK(common[s] == e.common[s]); CHECK(same_bits(score[s], e.score[s])); }
    for (int i = 0; i < cand_cap; i++) {
        if (i < n_cand) { CHECK(cs[i] == e.cand[(size_t)i] && ccm[i] == e.common[(size_t)cs[i]] && same_bits(csc[i], e.score[(size_t)cs[i]])); }
        else CHECK(cs[i] == -7 && ccm[i] == -7 && csc[i] == 7.0);   // nothing is written behind the list
    }
    return 0;
}

int run(int k, int L, int n_query, unsigned seed) {
    std::mt19937 rng(seed);
    float scale[kLevels];
    for (int l = 0; l < kLevels; l++) scale[l] = l ? scale[l - 1] * 1.2f : 1.f;
    Vocabulary V;
    if (make_vocabulary(rng, k, L, V)) return 1;
    orbx_matcher *m = nullptr;
    MUST(orbx_matcher_create(0, &m));
    // the query frame
    Rows Q;
    make_rows(rng, V, n_query, Q);
    orbx_frame *F = nullptr;
    MUST(orbx_frame_create(m, n_query + 37, &F));
    orbx_frame_desc qd = frame_desc(Q, n_query, scale);
    MUST(orbx_frame_load_host(F, &qd));
    std::vector<int32_t> qw((size_t)n_query + 37), qn((size_t)n_query + 37);
    MUST(orbx_frame_compute_bow(m, F, V.dev, kLevelsUp, qw.data(), qn.data()));
    qw.resize((size_t)n_query);
    const BowVector qv = bow_vector(qw, V.weight);
    CHECK(qv.size() > 10);
    if (check_vector([&](int32_t *i, double *v, int *n) { return orbx_frame_bow_vector(m, F, i, v, n); }, qv.size(), qv)) return 1;
    // key frames: 0 = the query's rows, 1..4 = parts of them and fresh rows, 5 = empty, 6 = a fisheye-stereo key frame of the query's rows (left 60 %)
    const int kKf = 7, n_slots = 17;
    const int slot_of[kKf] = {1, 4, 5, 9, 12, 14, 16};
    orbx_keyframe *kfs[kKf] = {};
    Rows R[kKf];
    std::map<int, BowVector> slots;
    BowVector kv[kKf];
    for (int j = 0; j < kKf; j++) {
        int n = 0, n_left = 0;
        if (j == 0 || j == 6) { R[j] = Q; n = n_query; }
        else if (j < 5) {
            const int take = n_query * j / 5;
            R[j].kps.assign(Q.kps.begin(), Q.kps.begin() + take); R[j].desc.assign(Q.desc.begin(), Q.desc.begin() + 32 * (size_t)take);
            make_rows(rng, V, 40 * j, R[j]);
            n = take + 40 * j;
        }
        std::vector<int32_t> w((size_t)std::max(n, 1)), nd((size_t)std::max(n, 1));
        if (j == 6) {
            n_left = n * 3 / 5;
            orbx_frame_desc d = frame_desc(R[j], n_left, scale);
            MUST(orbx_keyframe_create_host_fisheye(m, &d, R[j].kps.data() + n_left, n - n_left, nullptr, &kfs[j]));
            MUST(orbx_keyframe_compute_bow_fisheye(m, kfs[j], V.dev, kLevelsUp, w.data(), nd.data()));
        } else {
            orbx_frame_desc d = frame_desc(R[j], n, scale);
            MUST(orbx_keyframe_create_host(m, &d, nullptr, &kfs[j]));
            MUST(orbx_keyframe_compute_bow(m, kfs[j], V.dev, kLevelsUp, n ? w.data() : nullptr, n ? nd.data() : nullptr));
        }
        w.resize((size_t)n);
        kv[j] = bow_vector(w, V.weight);
        slots[slot_of[j]] = kv[j];
        if (check_vector([&](int32_t *i, double *v, int *c) { return orbx_keyframe_bow_vector(m, kfs[j], i, v, c); }, kv[j].size(), kv[j])) return 1;
    }
    CHECK(kv[6] == qv && kv[5].empty());
    // the database: adds without a wait, then queries by frame and by key frame, the full arrays and the list
    orbx_keyframe_database *db = nullptr;
    MUST(orbx_keyframe_database_create(0, n_slots, n_query + 160, &db));
    for (int j = 0; j < kKf; j++) MUST(orbx_keyframe_database_add(m, db, slot_of[j], kfs[j]));
    const std::vector<int32_t> none, ex{1, 16, 3};
    for (float ratio : {0.8f, 0.0f, 1.0f})
        for (const std::vector<int32_t> *x : {&none, &ex}) {
            const Expected e = expected(qv, slots, n_slots, *x, ratio);
            for (int cap : {n_slots, 2, 0}) {
                auto by_frame = [&](int32_t *c, double *s, int32_t *cs, int32_t *cc, double *csc, int cap_, int *nc, int *mx) {
                    return orbx_keyframe_database_query_frame(m, db, F, x->empty() ? nullptr : x->data(), (int)x->size(), ratio, c, s, cs, cc, csc, cap_, nc, mx);
                };
                auto by_kf = [&](int32_t *c, double *s, int32_t *cs, int32_t *cc, double *csc, int cap_, int *nc, int *mx) {
                    return orbx_keyframe_database_query_keyframe(m, db, kfs[6], x->empty() ? nullptr : x->data(), (int)x->size(), ratio, c, s, cs, cc, csc, cap_, nc, mx);
                };
                if (check_query(by_frame, e, n_slots, cap)) return 1;
                if (check_query(by_kf, e, n_slots, cap)) return 1;
            }
        }
    {
        const Expected e = expected(qv, slots, n_slots, none, 0.8f);
        CHECK(e.max_common == (int)qv.size() && e.cand.size() >= 2 && e.common[14] == 0 && same_bits(e.score[14], -0.0));
        const Expected x = expected(qv, slots, n_slots, ex, 0.8f);
        CHECK(x.max_common <= e.max_common && x.cand != e.cand);
        g_max_moved |= x.max_common < e.max_common;   // (27 words: every key frame holds them all)
    }
    // a query key frame that is not the query frame; erase, re-add over a longer row, clear
    auto by_kf2 = [&](int32_t *c, double *s, int32_t *cs, int32_t *cc, double *csc, int cap_, int *nc, int *mx) {
        return orbx_keyframe_database_query_keyframe(m, db, kfs[2], nullptr, 0, 0.8f, c, s, cs, cc, csc, cap_, nc, mx);
    };
    if (check_query(by_kf2, expected(kv[2], slots, n_slots, none, 0.8f), n_slots, n_slots)) return 1;
    MUST(orbx_keyframe_database_erase(m, db, 1)); MUST(orbx_keyframe_database_erase(m, db, 2));
    slots.erase(1);
    if (check_query(by_kf2, expected(kv[2], slots, n_slots, none, 0.8f), n_slots, n_slots)) return 1;
    MUST(orbx_keyframe_database_add(m, db, 1, kfs[1])); MUST(orbx_keyframe_database_add(m, db, 16, kfs[5]));   // a shorter and an empty vector over longer rows
    slots[1] = kv[1]; slots[16] = kv[5];
    if (check_query(by_kf2, expected(kv[2], slots, n_slots, none, 0.8f), n_slots, n_slots)) return 1;
    // refusals: nothing is enqueued, no counter moves, no output is written
    {
        int64_t before[6], after[6];
        CHECK(orbx_matcher_debug_transfers(m, before, 6) == 6);
        orbx_keyframe *plain = nullptr;
        orbx_frame_desc d = frame_desc(R[1], 10, scale);
        MUST(orbx_keyframe_create_host(m, &d, nullptr, &plain));
        CHECK(orbx_matcher_debug_transfers(m, before, 6) == 6);
        int32_t i1 = -7; double v1 = 7.0; int n1 = -5;
        CHECK(orbx_keyframe_bow_vector(m, plain, &i1, &v1, &n1) == ORBX_E_BAD_ARG);
        CHECK(orbx_keyframe_database_add(m, db, 0, plain) == ORBX_E_BAD_ARG);
        CHECK(orbx_keyframe_database_add(m, db, n_slots, kfs[1]) == ORBX_E_BAD_ARG && orbx_keyframe_database_add(m, db, -1, kfs[1]) == ORBX_E_BAD_ARG);
        CHECK(orbx_keyframe_database_erase(m, db, n_slots) == ORBX_E_BAD_ARG);
        const int32_t high[1] = {n_slots};
        int nc = -5, mx = -5;
        CHECK(orbx_keyframe_database_query_frame(m, db, F, high, 1, 0.8f, nullptr, nullptr, &i1, nullptr, nullptr, 1, &nc, &mx) == ORBX_E_BAD_ARG);
        CHECK(orbx_keyframe_database_query_keyframe(m, db, plain, nullptr, 0, 0.8f, nullptr, nullptr, &i1, nullptr, nullptr, 1, &nc, &mx) == ORBX_E_BAD_ARG);
        orbx_keyframe_database *tiny = nullptr;
        MUST(orbx_keyframe_database_create(0, 2, 8, &tiny));
        CHECK(orbx_keyframe_database_add(m, tiny, 0, kfs[0]) == ORBX_E_TOO_LARGE);
        orbx_keyframe_database_destroy(tiny);
        CHECK(orbx_matcher_debug_transfers(m, after, 6) == 6 && memcmp(before, after, sizeof(before)) == 0);
        CHECK(i1 == -7 && v1 == 7.0 && n1 == -5 && nc == -5 && mx == -5);
        orbx_keyframe_destroy(plain);
    }
    // the rows are copies: the key frames go first
    for (int j = 0; j < kKf; j++) orbx_keyframe_destroy(kfs[j]);
    auto by_frame = [&](int32_t *c, double *s, int32_t *cs, int32_t *cc, double *csc, int cap_, int *nc, int *mx) {
        return orbx_keyframe_database_query_frame(m, db, F, nullptr, 0, 0.8f, c, s, cs, cc, csc, cap_, nc, mx);
    };
    if (check_query(by_frame, expected(qv, slots, n_slots, none, 0.8f), n_slots, n_slots)) return 1;
    MUST(orbx_keyframe_database_clear(m, db));
    slots.clear();
    const Expected empty = expected(qv, slots, n_slots, none, 0.8f);
    CHECK(empty.cand.empty() && empty.max_common == 0);
    if (check_query(by_frame, empty, n_slots, n_slots)) return 1;
    orbx_keyframe_database_destroy(db);
    orbx_frame_destroy(F);
    orbx_matcher_destroy(m);
    orbx_vocabulary_destroy(V.dev);
    return 0;
}

}  // namespace

int main() {
    if (run(3, 3, 400, 5)) return 1;     // 27 words: every word many times (the sequential additions), one chunk
    if (run(8, 3, 700, 9)) return 1;     // 512 words: rows of several 64-word chunks
    if (!g_max_moved) { printf("FAILED: no exclusion moved the maximum\n"); return 1; }
    printf("keyframe database ok\n");
    return 0;
}
