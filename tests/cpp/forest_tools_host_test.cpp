// The forest tools' host rules of csrc/forest_tools_host.h alone, under the host sanitizers
// (tests/test_forest_tools_host_cpp_cpu.py): the three score formulas on counts (a class without examples, a cell above
// 2^24), the leaf order of the device tables, the head rules of the refit and the refit's serialisation -- structure
// bytes kept, leaves from counts, counts by stream node.  No HIP, no library: forest_model.cpp is compiled in.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "forest_tools_host.h"

using namespace rvseg;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// a tree whose stream order is not breadth first: node 0 splits into 1 | 2, node 2 into 3 | 4 and node 1 into 5 | 6,
// appended last, as the depth-first learner numbers them (the right child is popped first)
static RawTree tree_of(int C, int L, bool single) {
    RawTree t;
    t.feat = {0, 1, 2, 0, 0, 0, 0};
    t.thr = {10.f, 20.f, 30.f, 0.f, 0.f, 0.f, 0.f};
    t.left = {1, 5, 3, 0, 0, 0, 0};
    t.hist.assign(7, {});
    t.mhist.assign(7, {});
    for (int v = 3; v < 7; v++) {
        if (single) t.hist[(size_t)v].assign((size_t)C, -1.f - v);
        for (int l = 0; l < L; l++) t.mhist[(size_t)v].push_back(std::vector<float>((size_t)(C + l), -2.f - v));
    }
    return t;
}

static ForestModel parsed(const std::vector<RawTree>& trees) {
    ForestModel raw, m;
    raw.raw = trees;
    const std::vector<uint8_t> bytes = serialize_forest(raw);
    std::string err;
    CHECK(parse_forest(bytes.data(), bytes.size(), 8, m, err));
    return m;
}

int main() {
    // ---- the grid of a looping kernel: what it wants, capped, at least one block ----
    {
        CHECK(looping_grid(1, 1024) == 1 && looping_grid(1023, 1024) == 1023);
        CHECK(looping_grid(1024, 1024) == 1024 && looping_grid(1025, 1024) == 1024 && looping_grid(1L << 40, 1024) == 1024);
        CHECK(looping_grid(5, 0) == 1 && looping_grid(5, -3) == 1 && looping_grid(1L << 40, 0) == 1);
    }
    // ---- scores ----
    {
        const uint64_t big = (1ull << 24) + 3;
        const uint64_t conf[9] = {big, 5, 0, 0, 0, 0, 7, 1, 40};
        float norm[9];
        tools_confusion_normalised(conf, 3, norm);
        CHECK(norm[0] == 16777216.f / (float)(int)(big + 5) && norm[1] == 5.f / (float)(int)(big + 5) && norm[2] == 0.f);
        CHECK(std::isnan(norm[3]) && std::isnan(norm[4]) && std::isnan(norm[5]));
        CHECK(norm[6] == 7.f / 48 && norm[7] == 1.f / 48 && norm[8] == 40.f / 48);
        CHECK(tools_accuracy(conf, 3) == 1.0f - 13 / (float)(int)(big + 53));
        const uint64_t one[1] = {9};
        CHECK(tools_accuracy(one, 1) == 1.0f);
        const uint64_t agree[4] = {1000, 377, 377, 1000};
        float corr[4];
        tools_correlation(agree, 2, 1000, corr);
        CHECK(corr[0] == 1.f && corr[3] == 1.f && corr[1] == corr[2] && corr[1] == 1 - 623 / 1000.f);
    }
    // ---- leaf order: breadth first over the child links, whatever the stream order ----
    const RawTree t1 = tree_of(3, 1, true);
    {
        const std::vector<int32_t> rows = leaf_nodes_in_row_order(t1);
        CHECK(rows.size() == 4 && rows[0] == 5 && rows[1] == 6 && rows[2] == 3 && rows[3] == 4);
        const ForestModel m = parsed({t1});
        CHECK(m.n_leaves == 4);
        for (size_t k = 0; k < 4; k++) CHECK(m.single_hist[k * 3] == -1.f - rows[k]);   // the parser's rows are these nodes
    }
    // ---- head rules ----
    {
        std::string err;
        const int32_t c3[1] = {3}, c4[1] = {4}, c34[2] = {3, 4}, c17[1] = {17};
        const ForestModel both = parsed({t1}), multi2 = parsed({tree_of(3, 2, false)}), single_beside_two = parsed({tree_of(3, 2, true)});
        ForestModel single_only = parsed({tree_of(3, 0, true)});
        CHECK(refit_heads_match(both, 1, c3, err) && refit_writes_single(both, 1, c3));
        CHECK(!refit_heads_match(both, 1, c4, err) && !refit_heads_match(both, 2, c34, err));
        CHECK(refit_heads_match(multi2, 2, c34, err) && !refit_writes_single(multi2, 2, c34) && !refit_heads_match(multi2, 1, c3, err));
        CHECK(refit_heads_match(single_beside_two, 2, c34, err) && !refit_writes_single(single_beside_two, 2, c34));
        CHECK(refit_heads_match(single_only, 1, c3, err) && refit_writes_single(single_only, 1, c3) && !refit_heads_match(single_only, 1, c4, err));
        CHECK(!refit_heads_match(single_only, 1, c17, err) && !err.empty());
    }
    // ---- refit: two trees, one layer of 3 classes written to both heads ----
    {
        const ForestModel m = parsed({t1, t1});
        const int P = 40;
        // counts[leaf row][3]; every example lands in one leaf per tree
        const uint32_t counts[8 * 3] = {10, 0, 0, 0, 5, 5, 3, 3, 4, 0, 0, 10, 40, 0, 0, 0, 0, 0, 0, 20, 0, 0, 0, 20};
        const std::vector<std::vector<uint64_t>> class_cnt = {{13, 8, 19}};
        const ForestModel out = refit_model(m, counts, class_cnt, P, 1.0f);
        const std::vector<uint8_t> before = serialize_forest(m), after = serialize_forest(out);
        CHECK(before.size() == after.size() && before != after);
        std::vector<std::vector<float>> freq = {{inverted_frequency(P, 13), inverted_frequency(P, 8), inverted_frequency(P, 19)}};
        const std::vector<int32_t> rows = leaf_nodes_in_row_order(t1);
        for (size_t t = 0; t < 2; t++) {
            CHECK(out.raw[t].feat == m.raw[t].feat && out.raw[t].left == m.raw[t].left);
            CHECK(std::memcmp(out.raw[t].thr.data(), m.raw[t].thr.data(), 7 * 4) == 0);
            for (size_t k = 0; k < 4; k++) {
                unsigned cnt[TR_CMAX] = {};
                for (int c = 0; c < 3; c++) cnt[c] = counts[(t * 4 + k) * 3 + (size_t)c];
                const std::vector<std::vector<float>> want = leaf_histograms(cnt, freq, 1.0f);
                const size_t node = (size_t)rows[k];
                CHECK(out.raw[t].mhist[node].size() == 1 && out.raw[t].mhist[node][0] == want[0] && out.raw[t].hist[node] == want[0]);
            }
            for (size_t v = 0; v < 3; v++) CHECK(out.raw[t].hist[v].empty() && out.raw[t].mhist[v].empty());   // inner nodes
        }
        // an empty leaf: log(s / (C s)) in every class
        CHECK(out.raw[1].hist[(size_t)rows[1]][0] == std::log(1.0f / 3.0f));
        // the refitted stream parses again and its rows are the new leaves
        ForestModel again;
        std::string err;
        CHECK(parse_forest(after.data(), after.size(), 8, again, err) && again.n_leaves == 8);
        CHECK(again.single_hist[0] == out.raw[0].hist[5][0]);
        // counts by stream node
        std::vector<uint32_t> by_node(14 * 3, 77u);
        refit_counts_by_node(m, counts, 3, by_node.data());
        for (size_t t = 0; t < 2; t++) {
            for (size_t v = 0; v < 3; v++)
                for (size_t c = 0; c < 3; c++) CHECK(by_node[(t * 7 + v) * 3 + c] == 0u);
            for (size_t k = 0; k < 4; k++)
                for (size_t c = 0; c < 3; c++) CHECK(by_node[(t * 7 + (size_t)rows[k]) * 3 + c] == counts[(t * 4 + k) * 3 + c]);
        }
    }
    // ---- a single-label head beside two layers stays as loaded ----
    {
        const ForestModel m = parsed({tree_of(3, 2, true)});
        const uint32_t counts[4 * 7] = {1, 2, 3, 1, 2, 3, 0, 4, 0, 0, 0, 0, 0, 4, 0, 0, 9, 9, 0, 0, 0, 2, 2, 2, 2, 2, 2, 0};
        const ForestModel out = refit_model(m, counts, {{7, 4, 14}, {12, 4, 5, 4}}, 25, 0.5f);
        for (size_t v = 3; v < 7; v++) {
            CHECK(out.raw[0].hist[v] == m.raw[0].hist[v]);
            CHECK(out.raw[0].mhist[v].size() == 2 && out.raw[0].mhist[v][0].size() == 3 && out.raw[0].mhist[v][1].size() == 4);
            CHECK(out.raw[0].mhist[v][0] != m.raw[0].mhist[v][0]);
        }
    }
    // ---- ... and so does one beside a single layer of another class count (4 single-label classes, one layer of 3) ----
    {
        RawTree t = tree_of(3, 1, true);
        for (size_t v = 3; v < 7; v++) t.hist[v].assign(4, -9.f - (float)v);
        const ForestModel m = parsed({t});
        CHECK(m.single_classes == 4 && m.layer_classes.size() == 1 && m.layer_classes[0] == 3);
        std::string err;
        const int32_t c3[1] = {3}, c4[1] = {4};
        CHECK(refit_heads_match(m, 1, c3, err) && !refit_writes_single(m, 1, c3));
        CHECK(!refit_heads_match(m, 1, c4, err));   // the labels are the multi layer's, never the single head's alone
        const uint32_t counts[4 * 3] = {5, 0, 1, 0, 0, 0, 2, 2, 2, 0, 7, 1};
        const ForestModel out = refit_model(m, counts, {{7, 9, 4}}, 20, 1.0f);
        for (size_t v = 3; v < 7; v++) {
            CHECK(out.raw[0].hist[v] == m.raw[0].hist[v] && out.raw[0].hist[v].size() == 4);
            CHECK(out.raw[0].mhist[v].size() == 1 && out.raw[0].mhist[v][0].size() == 3 && out.raw[0].mhist[v][0] != m.raw[0].mhist[v][0]);
        }
        CHECK(serialize_forest(out).size() == serialize_forest(m).size());
    }
    std::printf("forest tools host ok\n");
    return 0;
}
