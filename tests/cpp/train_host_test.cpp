// The forest trainer's host-side rules (csrc/train_host.h) alone: a stand-alone program for the host compiler with
// -fsanitize=address,undefined (tests/test_train_host_cpp_cpu.py).  No HIP, no library.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "train_host.h"

using namespace rvseg;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); g_fail++; } } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static rvseg_train_params params(int min_split, int min_child, int max_depth) {
    rvseg_train_params tp{};
    tp.num_trees = 1; tp.max_depth = max_depth; tp.min_split_examples = min_split; tp.min_child_split_examples = min_child;
    tp.use_bootstrap = 1; tp.smoothing = 1.f; tp.seed = 1;
    return tp;
}
static CutResult cut(float objective, float l, float r, unsigned lm, unsigned rm) { return CutResult{objective, l, r, lm, rm, 1}; }

// definition 1 of oracle/rvseg_oracle_train.c, written out again
static uint64_t mix_longhand(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void test_random_source() {
    for (uint64_t z : {0ull, 1ull, 0x123456789ABCDEFull, ~0ull}) CHECK(mix64(z) == mix_longhand(z));
    const uint64_t key = 0xC0FFEEull;
    for (uint64_t i : {0ull, 1ull, 7ull, 0x100000000ull + 12345ull})
        CHECK(draw64(key, i) == mix_longhand(key ^ mix_longhand(i + 0x632BE59BD9B4E019ull)));
    CHECK(tree_key(5, 3) == mix_longhand(5 ^ mix_longhand(0x74726565ull + 3)));
    CHECK(root_key(9) == mix_longhand(9 ^ 0x726F6F74ull));
    CHECK(child_key(9, 0) == mix_longhand(9 ^ 0x4Cull) && child_key(9, 1) == mix_longhand(9 ^ 0x52ull));
}

static void test_threshold_guard() {
    // an ordinary pair: exactly (l + r) * 0.5f
    CHECK(same_bits(split_threshold(1.25f, 7.5f), (1.25f + 7.5f) * 0.5f));
    CHECK(same_bits(split_threshold(3.f, 4.f), 3.5f));
    // adjacent floats: the midpoint rounds to the left value, so the threshold is the right one
    const float l = 1.0f, r = std::nextafter(1.0f, 2.0f);
    CHECK(same_bits((l + r) * 0.5f, l));
    CHECK(same_bits(split_threshold(l, r), r));
    // finite values whose sum overflows, at both ends
    const float a = 3.0e38f, b = 3.2e38f;
    CHECK(std::isinf(a + b));
    CHECK(std::isfinite(split_threshold(a, b)) && same_bits(split_threshold(a, b), b));
    CHECK(std::isinf(-b + -a));
    CHECK(std::isfinite(split_threshold(-b, -a)) && same_bits(split_threshold(-b, -a), -a));
}

static void test_stop_rules() {
    const int feats[2] = {11, 4};
    const CutResult cuts[2] = {cut(5.f, 1.f, 2.f, 6, 4), cut(7.f, 1.f, 2.f, 5, 5)};
    unsigned totals[TR_CMAX] = {};
    totals[0] = 6; totals[3] = 4;   // mass 10, two classes
    // mass against min_split: 10 < 11 stops, 10 >= 10 splits
    CHECK(!decide_split(totals, cuts, feats, 2, 0, params(11, 1, 30)).split);
    const Split s = decide_split(totals, cuts, feats, 2, 0, params(10, 1, 30));
    CHECK(s.split && s.feature == 11 && same_bits(s.threshold, 1.5f) && s.left_mass == 6 && s.right_mass == 4);
    // one present class
    unsigned pure[TR_CMAX] = {};
    pure[5] = 10;
    CHECK(!decide_split(pure, cuts, feats, 2, 0, params(1, 1, 30)).split);
    // depth == max_depth splits, max_depth + 1 does not (learning.cpp:525 tests depth > maxDepth)
    CHECK(decide_split(totals, cuts, feats, 2, 30, params(1, 1, 30)).split);
    CHECK(!decide_split(totals, cuts, feats, 2, 31, params(1, 1, 30)).split);
    // no feature offers a cut
    CutResult none[2] = {cuts[0], cuts[1]};
    none[0].valid = none[1].valid = 0;
    CHECK(!decide_split(totals, none, feats, 2, 0, params(1, 1, 30)).split);
}

static void test_feature_order_and_child_mass() {
    unsigned totals[TR_CMAX] = {};
    totals[1] = 5; totals[2] = 5;
    const int feats[3] = {8, 2, 6};
    // an exact tie: the first feature in sampled order keeps it; a strictly better later one takes it
    const CutResult tie[3] = {cut(4.f, 0.f, 1.f, 5, 5), cut(4.f, 10.f, 20.f, 5, 5), cut(4.f, 3.f, 5.f, 5, 5)};
    CHECK(decide_split(totals, tie, feats, 3, 0, params(1, 1, 30)).feature == 8);
    const CutResult better[3] = {cut(4.f, 0.f, 1.f, 5, 5), cut(3.5f, 10.f, 20.f, 5, 5), cut(3.5f, 3.f, 5.f, 5, 5)};
    const Split s = decide_split(totals, better, feats, 3, 0, params(1, 1, 30));
    CHECK(s.split && s.feature == 2 && same_bits(s.threshold, 15.f));
    // the child-mass rule looks at the best cut only: one below min_child on either side refuses the split
    const CutResult small_left[1] = {cut(4.f, 0.f, 1.f, 2, 8)}, small_right[1] = {cut(4.f, 0.f, 1.f, 8, 2)};
    CHECK(!decide_split(totals, small_left, feats, 1, 0, params(1, 3, 30)).split);
    CHECK(!decide_split(totals, small_right, feats, 1, 0, params(1, 3, 30)).split);
    CHECK(decide_split(totals, small_left, feats, 1, 0, params(1, 2, 30)).split);
}

static void test_renumbering() {
    // level order:      0            the reference's stack (children appended when the parent is popped, right child
    //                 1   2          popped first): pop 0 -> 1, 2 get ids 1, 2; pop 2 -> 5, 6 get 3, 4; pop 6, pop 5;
    //                3 4 5 6         pop 1 -> 3, 4 get 5, 6
    GrowingTree g(root_key(1));
    CHECK(g.split(0, 10, 0.5f) == 1);
    CHECK(g.split(1, 11, 1.5f) == 3);
    CHECK(g.split(2, 12, 2.5f) == 5);
    CHECK(g.size() == 7 && g.depth[0] == 0 && g.depth[2] == 1 && g.depth[6] == 2);
    CHECK(g.key[4] == child_key(child_key(g.key[0], 0), 1));
    g.mhist.assign(7, {});
    for (int v = 3; v < 7; v++) g.mhist[v] = {{(float)v}};   // one layer: the leaf's marker
    const RawTree t = renumber_depth_first(std::move(g));
    const int want_feat[7] = {10, 11, 12, 0, 0, 0, 0}, want_left[7] = {1, 5, 3, 0, 0, 0, 0};
    const float want_thr[7] = {0.5f, 1.5f, 2.5f, 0.f, 0.f, 0.f, 0.f}, want_leaf[7] = {0, 0, 0, 5, 6, 3, 4};
    CHECK(t.feat.size() == 7 && t.thr.size() == 7 && t.left.size() == 7 && t.hist.size() == 7 && t.mhist.size() == 7);
    for (int v = 0; v < 7; v++) {
        CHECK(t.feat[v] == want_feat[v] && t.left[v] == want_left[v] && same_bits(t.thr[v], want_thr[v]));
        if (want_left[v]) { CHECK(t.mhist[v].empty() && t.hist[v].empty()); continue; }
        CHECK(t.mhist[v].size() == 1 && t.mhist[v][0].size() == 1 && t.mhist[v][0][0] == want_leaf[v]);
        CHECK(t.hist[v] == t.mhist[v][0]);   // a single layer also fills `hist`
    }
}

static void test_leaf_histograms() {
    const unsigned counts[3] = {0, 1, 3};
    const std::vector<std::vector<float>> freq = {{7.f / 3.f, 1.1f, 0.7f}};
    unsigned cnt[TR_CMAX] = {};
    for (int c = 0; c < 3; c++) cnt[c] = counts[c];
    for (float smoothing : {0.f, 1.f}) {
        float h[3], total = 0.f;
        for (int c = 0; c < 3; c++) {
            h[c] = 0.f;
            for (unsigned k = 0; k < counts[c]; k++) h[c] += freq[0][c];
        }
        for (int c = 0; c < 3; c++) total += h[c];
        const std::vector<std::vector<float>> got = leaf_histograms(cnt, freq, smoothing);
        CHECK(got.size() == 1 && got[0].size() == 3);
        for (int c = 0; c < 3; c++) CHECK(same_bits(got[0][c], std::log((h[c] + smoothing) / (total + 3 * smoothing))));
        if (smoothing == 0.f) CHECK(got[0][0] == -std::numeric_limits<float>::infinity());
    }
    // three additions are not one multiplication
    CHECK(same_bits(inverted_frequency(10, 4), 10 / 4.f));
    CHECK(same_bits(inverted_frequency(1 << 25, 1u << 25), (1 << 25) / 16777216.f));   // the float count stalls at 2^24
}

int main() {
    test_random_source();
    test_threshold_guard();
    test_stop_rules();
    test_feature_order_and_child_mass();
    test_renumbering();
    test_leaf_histograms();
    if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
    std::printf("train host ok\n");
    return 0;
}
