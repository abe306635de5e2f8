// The forest tools' host-side rules (rvseg_forest_tools.hip), free of HIP so that the host compiler and its sanitizers
// can run them alone (tests/cpp/forest_tools_host_test.cpp): the float arithmetic of libforest's tools.cpp on integer
// counts, the order of a tree's leaves in the device tables, and the refit of a model's leaves from counts.
#pragma once
#include <algorithm>
#include <cstdint>
#include <queue>
#include <string>
#include <vector>

#include "forest_model.h"
#include "train_host.h"

namespace rvseg {

constexpr int TOOLS_CHUNK = 65536;   // points of X on the device at a time: scratch is bounded by this, not by P

// The grid of a kernel whose blocks loop over their work: the `want` blocks that would each take one share, capped at
// max_blocks -- a few blocks per compute unit (count_blocks) -- and at least one.
inline int looping_grid(long want, int max_blocks) { return (int)(want < max_blocks ? want : (max_blocks > 0 ? max_blocks : 1)); }

// AccuracyTool::measure (tools.cpp:61-78): 1.0f - error / (float)size, `error` an int -- the off-diagonal total
inline float tools_accuracy(const uint64_t* confusion, int C) {
    uint64_t size = 0, errors = 0;
    for (int t = 0; t < C; t++)
        for (int p = 0; p < C; p++) {
            size += confusion[(size_t)t * C + p];
            if (t != p) errors += confusion[(size_t)t * C + p];
        }
    return 1.0f - (int)errors / static_cast<float>((int)size);
}

// ConfusionMatrixTool::measure (tools.cpp:95-138): the cell is a float grown by "+= 1" -- it stops at 2^24, the idiom
// inverted_frequency (train_host.h) treats the same way -- divided by the row's int count.  A true class without
// examples is 0 / 0 = NaN, as in the reference.
inline void tools_confusion_normalised(const uint64_t* confusion, int C, float* out) {
    for (int t = 0; t < C; t++) {
        uint64_t row = 0;
        for (int p = 0; p < C; p++) row += confusion[(size_t)t * C + p];
        for (int p = 0; p < C; p++) {
            const uint64_t n = confusion[(size_t)t * C + p];
            const float cell = n <= 16777216ull ? (float)n : 16777216.f;
            out[(size_t)t * C + p] = cell / (int)row;
        }
    }
}

// CorrelationTool::measure (tools.cpp:221-230): 1 - hammingDist / (float)size per pair, the distance an int
inline void tools_correlation(const uint64_t* agree, int T, uint64_t P, float* out) {
    for (int t = 0; t < T; t++)
        for (int tt = 0; tt < T; tt++) {
            const float normalizedDistance = (int)(P - agree[(size_t)t * T + tt]) / static_cast<float>((int)P);
            out[(size_t)t * T + tt] = 1 - normalizedDistance;
        }
}

// The stream nodes of a tree's leaves in the order parse_forest numbers its leaf rows (breadth first, forest_model.cpp):
// leaf row (first row of the tree + k) is node result[k].  The tree has been validated by the parser.
inline std::vector<int32_t> leaf_nodes_in_row_order(const RawTree& raw) {
    std::vector<int32_t> leaves;
    std::queue<int32_t> q;
    q.push(0);
    while (!q.empty()) {
        const int32_t node = q.front();
        q.pop();
        const int32_t l = raw.left[(size_t)node];
        if (l == 0) { leaves.push_back(node); continue; }
        q.push(l);
        q.push(l + 1);
    }
    return leaves;
}

// Which heads a refit writes: the model's multi layers from the label layers one to one; a single-label head alone from
// one label layer.  A single-label head beside multi layers is written -- from the same labels -- only in the shape
// rvseg_forest_train writes (one layer, the same class count); beside other layers no labels are its own and it stays
// as loaded.  Label layers that do not match are refused.
inline bool refit_writes_single(const ForestModel& m, int n_layers, const int32_t* class_counts) {
    if (m.single_classes == 0) return false;
    return m.layer_classes.empty() || (n_layers == 1 && m.single_classes == class_counts[0]);
}
inline bool refit_heads_match(const ForestModel& m, int n_layers, const int32_t* class_counts, std::string& err) {
    for (int l = 0; l < n_layers; l++)
        if (class_counts[l] < 1 || class_counts[l] > TR_CMAX) { err = "the refit handles 1..16 classes per layer"; return false; }
    if (!m.layer_classes.empty()) {
        if ((int)m.layer_classes.size() != n_layers) { err = "n_layers does not match the model's multi layers"; return false; }
        for (int l = 0; l < n_layers; l++)
            if (m.layer_classes[(size_t)l] != class_counts[l]) { err = "class_counts do not match the model's multi layers"; return false; }
        return true;
    }
    if (n_layers != 1 || m.single_classes != class_counts[0]) { err = "n_layers / class_counts do not match the model's single-label head"; return false; }
    return true;
}

// updateHistograms / updateMultiHistograms (learning.cpp:918-1012) on the trees of `m` as loaded: features, thresholds
// and child links stay, every leaf's histograms are re-estimated from counts[leaf row][sumC] (layers concatenated) and
// the class totals class_cnt[layer][class] of the same set of P examples.  The heads must match (refit_heads_match).
inline ForestModel refit_model(const ForestModel& m, const uint32_t* counts, const std::vector<std::vector<uint64_t>>& class_cnt, int P,
                               float smoothing) {
    const size_t L = class_cnt.size();
    std::vector<std::vector<float>> freq(L);
    std::vector<int> off(L + 1, 0);
    for (size_t l = 0; l < L; l++) {
        off[l + 1] = off[l] + (int)class_cnt[l].size();
        for (uint64_t n : class_cnt[l]) freq[l].push_back(inverted_frequency(P, (unsigned)n));
    }
    const int sumC = off[L];
    std::vector<int32_t> cc;
    for (size_t l = 0; l < L; l++) cc.push_back((int32_t)class_cnt[l].size());
    const bool single = refit_writes_single(m, (int)L, cc.data());
    ForestModel out;
    out.raw = m.raw;
    size_t row = 0;
    std::vector<unsigned> cnt(L * TR_CMAX);
    for (RawTree& tree : out.raw)
        for (int32_t node : leaf_nodes_in_row_order(tree)) {
            std::fill(cnt.begin(), cnt.end(), 0u);
            for (size_t l = 0; l < L; l++)
                for (int c = 0; c < off[l + 1] - off[l]; c++) cnt[l * TR_CMAX + (size_t)c] = counts[row * (size_t)sumC + (size_t)(off[l] + c)];
            std::vector<std::vector<float>> h = leaf_histograms(cnt.data(), freq, smoothing);
            if (single) tree.hist[(size_t)node] = h[0];
            if (!m.layer_classes.empty()) tree.mhist[(size_t)node] = std::move(h);
            row++;
        }
    return out;
}

// counts_out of rvseg_forest_refit: [tree][node in stream order][sumC], zeros at inner nodes
inline void refit_counts_by_node(const ForestModel& m, const uint32_t* counts, int sumC, uint32_t* out) {
    size_t row = 0, base = 0;
    for (const RawTree& tree : m.raw) {
        std::fill(out + base * (size_t)sumC, out + (base + tree.left.size()) * (size_t)sumC, 0u);
        for (int32_t node : leaf_nodes_in_row_order(tree)) {
            for (int c = 0; c < sumC; c++) out[(base + (size_t)node) * (size_t)sumC + (size_t)c] = counts[row * (size_t)sumC + (size_t)c];
            row++;
        }
        base += tree.left.size();
    }
}

}  // namespace rvseg
