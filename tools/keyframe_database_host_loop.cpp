// The host route that orbx_keyframe_database replaces, for tools/keyframe_database_latency.py: the adapter's fold of the word ids into mBowVec
// (BowVector::addWeight per feature, normalize(L1)) and the first half of KeyFrameDatabase::DetectRelocalizationCandidates -- the walk of the inverted
// file that counts the common words, maxCommonWords, minCommonWords and L1Scoring::score for the key frames above it -- with the reference's
// containers: std::map BowVectors and a std::vector<std::list<int>> inverted file.  One core.  kfdb_host_query returns the time of the fold and the
// query in microseconds (std::chrono::steady_clock); the candidates are sorted by key frame id behind the clock.
// Built by the tool with g++ -O2 -shared; nothing else uses it.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <vector>

namespace {

typedef std::map<unsigned, double> BowVector;

struct KeyFrame { BowVector bow; long query = -1; int words = 0; };
struct Database {
    std::vector<double> weight;
    std::vector<std::list<int>> inverted;   // mvInvertedFile: word id -> key frames
    std::vector<KeyFrame> kfs;
    long query_id = 0;
};

BowVector fold(const Database &D, const int32_t *words, int n) {
    BowVector v;
    for (int i = 0; i < n; i++) {
        const unsigned id = (unsigned)words[i];
        if (words[i] < 0 || id >= D.weight.size()) continue;
        const double w = D.weight[id];
        if (w > 0) {
            BowVector::iterator vit = v.lower_bound(id);
            if (vit != v.end() && !(v.key_comp()(id, vit->first))) vit->second += w;
            else v.insert(vit, BowVector::value_type(id, w));
        }
    }
    double norm = 0.0;
    for (BowVector::iterator it = v.begin(); it != v.end(); ++it) norm += fabs(it->second);
    if (norm > 0.0)
        for (BowVector::iterator it = v.begin(); it != v.end(); ++it) it->second /= norm;
    return v;
}

double score(const BowVector &v1, const BowVector &v2) {   // L1Scoring::score
    BowVector::const_iterator v1_it = v1.begin(), v2_it = v2.begin();
    const BowVector::const_iterator v1_end = v1.end(), v2_end = v2.end();
    double s = 0;
    while (v1_it != v1_end && v2_it != v2_end) {
        const double &vi = v1_it->second, &wi = v2_it->second;
        if (v1_it->first == v2_it->first) {
            s += fabs(vi - wi) - fabs(vi) - fabs(wi);
            ++v1_it; ++v2_it;
        } else if (v1_it->first < v2_it->first) {
            v1_it = v1.lower_bound(v2_it->first);
        } else {
            v2_it = v2.lower_bound(v1_it->first);
        }
    }
    return -s / 2.0;
}

}  // namespace

extern "C" void *kfdb_host_create(int n_words, const double *weight) {
    Database *D = new Database();
    D->weight.assign(weight, weight + n_words);
    D->inverted.resize((size_t)n_words);
    return D;
}
extern "C" void kfdb_host_destroy(void *h) { delete static_cast<Database *>(h); }

// KeyFrameDatabase::add; returns the key frame's id (its slot)
extern "C" int kfdb_host_add(void *h, const int32_t *words, int n) {
    Database &D = *static_cast<Database *>(h);
    KeyFrame kf;
    kf.bow = fold(D, words, n);
    const int id = (int)D.kfs.size();
    for (BowVector::const_iterator vit = kf.bow.begin(); vit != kf.bow.end(); ++vit) D.inverted[vit->first].push_back(id);
    D.kfs.push_back(kf);
    return id;
}

extern "C" double kfdb_host_query(void *h, const int32_t *words, int n, float min_ratio, int32_t *cand, int32_t *cand_common, double *cand_score, int cap,
                                  int *n_cand, int *max_common) {
    Database &D = *static_cast<Database *>(h);
    const auto t0 = std::chrono::steady_clock::now();
    const BowVector q = fold(D, words, n);
    const long qid = ++D.query_id;
    std::list<int> sharing;   // lKFsSharingWords
    for (BowVector::const_iterator vit = q.begin(); vit != q.end(); ++vit) {
        std::list<int> &lKFs = D.inverted[vit->first];
        for (std::list<int>::iterator lit = lKFs.begin(); lit != lKFs.end(); ++lit) {
            KeyFrame &kf = D.kfs[(size_t)*lit];
            if (kf.query != qid) { kf.words = 0; kf.query = qid; sharing.push_back(*lit); }
            kf.words++;
        }
    }
    int maxCommonWords = 0;
    for (std::list<int>::iterator lit = sharing.begin(); lit != sharing.end(); ++lit) maxCommonWords = std::max(maxCommonWords, D.kfs[(size_t)*lit].words);
    int minCommonWords = maxCommonWords * min_ratio;
    std::vector<std::pair<int, double>> found;   // lScoreAndMatch (the double kept: the reference narrows it to float)
    for (std::list<int>::iterator lit = sharing.begin(); lit != sharing.end(); ++lit) {
        const KeyFrame &kf = D.kfs[(size_t)*lit];
        if (kf.words > minCommonWords) found.push_back(std::make_pair(*lit, score(q, kf.bow)));
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    std::sort(found.begin(), found.end());
    *n_cand = (int)found.size(); *max_common = maxCommonWords;
    for (int i = 0; i < (int)found.size() && i < cap; i++) { cand[i] = found[(size_t)i].first; cand_common[i] = D.kfs[(size_t)found[(size_t)i].first].words; cand_score[i] = found[(size_t)i].second; }
    return us;
}
