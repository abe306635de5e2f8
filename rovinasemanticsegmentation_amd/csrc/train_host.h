// The forest trainer's host-side rules (rvseg_train.hip), free of HIP so that the host compiler and its sanitizers can
// run them alone (tests/cpp/train_host_test.cpp).  Everything here is order-sensitive fp32 or an ordering rule that the
// byte-for-byte contract with oracle/rvseg_oracle_train.c rests on; line references are to the reference's
// third-party/libforest/src/learning.cpp unless they name another file.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/rvseg.h"
#include "forest_model.h"

#if defined(__HIPCC__)
#define RV_TRAIN_HD __host__ __device__
#else
#define RV_TRAIN_HD
#endif

namespace rvseg {

constexpr int TR_CMAX = 16;     // classes per layer the trainer handles (the reference's layers have 8 and 9)

// ---- the shared random source (oracle/rvseg_oracle_train.c, definition 1) -----------------------------------------
RV_TRAIN_HD inline uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
RV_TRAIN_HD inline uint64_t draw64(uint64_t key, uint64_t i) { return mix64(key ^ mix64(i + 0x632BE59BD9B4E019ull)); }
inline uint64_t tree_key(uint64_t seed, int tree) { return mix64(seed ^ mix64(0x74726565ull + (uint64_t)tree)); }
inline uint64_t root_key(uint64_t kt) { return mix64(kt ^ 0x726F6F74ull); }
inline uint64_t child_key(uint64_t parent, int side) { return mix64(parent ^ (side == 0 ? 0x4Cull : 0x52ull)); }

// what a search kernel reports for one (node, sampled feature)
struct CutResult {
    float objective;           // E(left) + E(right) of the best cut; 1e35 when the feature offers no cut
    float left_value, right_value;   // the two adjacent values the cut lies between
    unsigned left_mass, right_mass;
    int valid;
};

// the midpoint of :592 and :607; adjacent floats (it rounds to left) or an overflowing sum (+-inf): `right` keeps
// `x < threshold` separating the two (oracle definition 4)
inline float split_threshold(float left_value, float right_value) {
    float th = left_value + right_value;                                    // :592
    th *= 0.5f;                                                             // :607
    if (!(left_value < th && th <= right_value)) th = right_value;
    return th;
}

struct Split {
    bool split = false;
    int feature = 0;
    float threshold = 0.f;
    unsigned left_mass = 0, right_mass = 0;
};

// One node's decision from its class totals [TR_CMAX] and the K cut records of its sampled features `feats`, in sampled
// order.
inline Split decide_split(const unsigned* totals, const CutResult* cuts, const int* feats, int K, int depth, const rvseg_train_params& tp) {
    Split out;
    unsigned mass = 0;
    int present = 0;
    for (int c = 0; c < TR_CMAX; c++) { mass += totals[c]; present += totals[c] ? 1 : 0; }
    // stop rules of :521-527: too few examples, pure, too deep
    if ((long long)mass < (long long)tp.min_split_examples || present <= 1 || depth > tp.max_depth) return out;
    int best_k = -1;
    float best_obj = 1e35f;
    for (int k = 0; k < K; k++)   // features in sampled order, strict '<' keeps the first best (:589)
        if (cuts[k].valid && cuts[k].objective < best_obj) { best_obj = cuts[k].objective; best_k = k; }
    if (best_k < 0) return out;                                             // bestFeature < 0, :611
    const CutResult& c = cuts[best_k];
    if ((long long)c.left_mass < (long long)tp.min_child_split_examples || (long long)c.right_mass < (long long)tp.min_child_split_examples) return out;
    out.split = true;
    out.feature = feats[best_k];
    out.threshold = split_threshold(c.left_value, c.right_value);
    out.left_mass = c.left_mass;
    out.right_mass = c.right_mass;
    return out;
}

// inverted class frequency (data.h:358-370): size / count in float.  The reference counts with "freq[label]++" on a
// float: exact up to 2^24, where the float stops growing
inline float inverted_frequency(int P, unsigned count) {
    const float n = count <= 16777216u ? (float)count : 16777216.f;
    return P / n;
}

// ---- the class-weighted split objective (include/rvseg.h: rvseg_class_prior, definitions 1 and 2) -------------------
// What is wrong with a prior for C classes, naming the field, or null.  A null prior is RVSEG_PRIOR_NONE.
inline const char* class_prior_error(const rvseg_class_prior* prior, int C) {
    if (C < 2 || C > TR_CMAX) return "C: the class-weighted objective takes 2..16 classes";
    if (!prior) return nullptr;
    if (prior->mode != RVSEG_PRIOR_NONE && prior->mode != RVSEG_PRIOR_INVERSE_FREQUENCY && prior->mode != RVSEG_PRIOR_GIVEN)
        return "prior->mode: not a rvseg_prior_mode";
    if (prior->mode == RVSEG_PRIOR_GIVEN)
        for (int c = 0; c < C; c++)
            if (!(prior->weights[c] > 0.0f) || !(prior->weights[c] <= 3.4028234663852886e38f))
                return "prior->weights: every weight of the first C must be finite and > 0";
    return nullptr;
}

// definition 1: the weights of one tree from the class counts cnt[TR_CMAX] of its data set (after the bootstrap).
// INVERSE_FREQUENCY: (float)Nb / (float)cnt_c (getInvertedClassFrequency on the bootstrapped storage, data.h:346-357,
// :712); GIVEN: the caller's.  A class the set does not hold gets 0: no side holds it either, so it is never read.
inline void class_prior_weights(const rvseg_class_prior& prior, const unsigned* cnt, int C, float* w) {
    unsigned nb = 0;
    for (int c = 0; c < TR_CMAX; c++) nb += cnt[c];
    for (int c = 0; c < TR_CMAX; c++) {
        w[c] = 0.0f;
        if (c >= C || cnt[c] == 0) continue;
        w[c] = prior.mode == RVSEG_PRIOR_GIVEN ? prior.weights[c] : inverted_frequency((int)nb, cnt[c]);
    }
}

// fastlog2 (fastlog.h:47-58) and ENTROPY (:13) on the host, in the operation order of the kernels
inline float fastlog2_host(float x) {
    uint32_t vi, mi;
    std::memcpy(&vi, &x, 4);
    mi = (vi & 0x007FFFFFu) | 0x3f000000u;
    float mx;
    std::memcpy(&mx, &mi, 4);
    float y = (float)vi;
    y = y * 1.1920928955078125e-7f;
    const float a = 1.498030302f * mx;
    const float den = 0.3520887068f + mx;
    const float b = 1.72587999f / den;
    float r = y - 124.22551499f;
    r = r - a;
    r = r - b;
    return r;
}
inline float entropy_term_host(float p) { return (-p) * fastlog2_host(p); }

// definition 2: the objective of one side with integer class counts cnt[TR_CMAX] under the weights w[TR_CMAX]
inline float weighted_hist_entropy(const unsigned* cnt, const float* w) {
    float mass = 0.0f;
    for (int c = 0; c < TR_CMAX; c++) {
        if (cnt[c] == 0) continue;
        mass += w[c] * (float)cnt[c];
    }
    float total = -entropy_term_host(mass);
    for (int c = 0; c < TR_CMAX; c++) {
        if (cnt[c] == 0) continue;
        total += entropy_term_host(w[c] * (float)cnt[c]);
    }
    return total;
}

// One leaf's log histograms (updateMultiHistograms, :960-1012) from its integer counts cnt[layer][TR_CMAX] over ALL
// examples and the inverted class frequencies freq[layer][class].
inline std::vector<std::vector<float>> leaf_histograms(const unsigned* cnt, const std::vector<std::vector<float>>& freq, float smoothing) {
    std::vector<std::vector<float>> out(freq.size());
    for (size_t l = 0; l < freq.size(); l++) {
        const int C = (int)freq[l].size();
        std::vector<float>& h = out[l];
        h.assign(C, 0.f);
        for (int c = 0; c < C; c++) {
            // "hist[l][classlabel] += freq[classlabel]" once per example (:989-991): n additions of the same addend
            const unsigned n = cnt[l * TR_CMAX + c];
            const float f = freq[l][c];
            float acc = 0.f;
            for (unsigned k = 0; k < n; k++) acc += f;
            h[c] = acc;
        }
        float total = 0;
        for (int c = 0; c < C; c++) total += h[c];
        for (int c = 0; c < C; c++) h[c] = std::log((h[c] + smoothing) / (total + C * smoothing));   // :1004-1007
    }
    return out;
}

// The tree in level order while it grows: node 0 is the root, left == 0 marks a leaf, the right child is left + 1.
struct GrowingTree {
    std::vector<int> feat, left, depth;
    std::vector<float> thr;
    std::vector<uint64_t> key;                                  // the node's path key (oracle definition 1)
    std::vector<std::vector<std::vector<float>>> mhist;         // leaves: [layer][class], filled when the tree is grown
    explicit GrowingTree(uint64_t root) : feat(1, 0), left(1, 0), depth(1, 0), thr(1, 0.f), key(1, root) {}
    int size() const { return (int)left.size(); }
    // DecisionTree::splitNode (classifier.cpp:77-95): two leaves are appended; returns the left one
    int split(int node, int f, float th) {
        const int lc = size();
        for (int side = 0; side < 2; side++) {
            feat.push_back(0); thr.push_back(0.f); left.push_back(0); depth.push_back(depth[node] + 1);
            key.push_back(child_key(key[node], side));
        }
        feat[node] = f; thr[node] = th; left[node] = lc;
        return lc;
    }
};

// The reference's node numbering: children are appended when their parent is popped, the right child is popped first
// (:646-655), so the file equals the depth-first learner's.  A single-layer forest's leaves also serve
// classLogPosterior through `hist`.  Consumes the tree: the leaf histograms move over.
inline RawTree renumber_depth_first(GrowingTree&& g) {
    const int n = g.size();
    std::vector<int> new_id(n, -1), stack(1, 0);
    new_id[0] = 0;
    int next = 1;
    while (!stack.empty()) {
        const int v = stack.back();
        stack.pop_back();
        if (g.left[v] == 0) continue;
        new_id[g.left[v]] = next; new_id[g.left[v] + 1] = next + 1;
        next += 2;
        stack.push_back(g.left[v]);
        stack.push_back(g.left[v] + 1);
    }
    RawTree tree;
    tree.feat.assign(n, 0); tree.thr.assign(n, 0.f); tree.left.assign(n, 0);
    tree.hist.assign(n, {}); tree.mhist.assign(n, {});
    for (int v = 0; v < n; v++) {
        const int nv = new_id[v];
        tree.feat[nv] = g.feat[v]; tree.thr[nv] = g.thr[v];
        tree.left[nv] = g.left[v] ? new_id[g.left[v]] : 0;
        if (g.left[v] != 0 || (size_t)v >= g.mhist.size()) continue;
        tree.mhist[nv] = std::move(g.mhist[v]);
        if (tree.mhist[nv].size() == 1) tree.hist[nv] = tree.mhist[nv][0];
    }
    return tree;
}

// ---- boosting (BoostedRandomForestLearner::learn, :1120-1234; rvseg_train.hip lists the build-owned definitions) ----
// definition 1: the round's key, its uniform draws -- 24 random bits, exact in fp32, in [0, 1) -- and its tree's seed
inline uint64_t boost_round_key(uint64_t seed, int round) { return mix64(seed ^ mix64(0x626F6F73ull + (uint64_t)round)); }
RV_TRAIN_HD inline float boost_uniform(uint64_t kb, uint64_t n) { return (float)(draw64(kb, n) >> 40) * 5.9604644775390625e-8f; }
inline uint64_t boost_tree_seed(uint64_t kb) { return draw64(kb, 1ull << 40); }

// What a round does with its tree, from the tree's error on the whole set (definition 4).  alpha is :1197: the first
// logarithm is float, the second takes an int and is double, the sum is narrowed to float; scale is :1207's
// std::exp(alpha), float.
struct BoostRound {
    bool keep_tree = false;   // addTree(tree, alpha)
    bool go_on = false;       // update the weights and run the next round
    float alpha = 0.f, scale = 1.f;
};
inline BoostRound boost_round(float error, int C) {
    BoostRound r;
    if (!(error < 1.0f)) return r;                       // error >= 1 (or NaN): the tree is not added, boosting ends
    r.keep_tree = true;
    r.alpha = (float)(std::log((1 - error) / error) + std::log(C - 1));
    if (error == 0.0f) return r;                         // alpha = +inf: the tree is added, boosting ends
    r.scale = std::exp(r.alpha);
    r.go_on = true;
    return r;
}
// a total the weights can be divided by (definition 4)
inline bool boost_total_ok(float total) { return total > 0.0f && total <= 3.4028234663852886e38f; }

}  // namespace rvseg
