// Forest training on the GPU: replaces, for the forests this path evaluates,
//   RandomForestLearner::learn                 third-party/libforest/src/learning.cpp:1031-1073
//   DecisionTreeLearner::learn (multi-layer)   learning.cpp:410-662   (single layer: :663-915, same search)
//   updateMultiHistograms / updateHistograms   learning.cpp:918-1012
//   forest->write                              src/train.cpp:244-249
//   the extraction + augmentation loop         src/train.cpp:115-147  (rvseg_forest_train_frames)
//
// What the reference does per tree: bootstrap N examples; depth-first over an explicit stack, per node pick a
// random label layer, stop if mass < minSplitExamples / pure / depth > maxDepth, otherwise try numFeatures random
// features: sort the node's examples by the feature and take the threshold (midpoint of two adjacent values that
// differ by at least 1e-6) that minimises E(left) + E(right); split unless a child would have fewer than
// minChildSplitExamples.  Finally the leaf histograms are recomputed from ALL examples, each adding the inverted
// class frequency of its label, and stored as log((h + s) / (total + C*s)).
//
// MI355X design: level by level instead of depth-first -- the tree a given set of random choices produces does not
// depend on the visiting order once those choices are keyed by the node's PATH (train_host.h) -- and per level the
// frontier is searched in batches of SLOT_BATCH nodes (kernels_train.hip: histograms for byte-valued features, one sort
// for the others, exactly the reference's candidates), the host applies the stop rules in the reference's order and
// appends children (decide_split), and one pass routes every example with the evaluator's own rule `x[f] < threshold`.
// Nodes are renumbered at the end in the order the reference's stack would have created them (renumber_depth_first), so
// the file equals the depth-first learner's.
//
// This file is the learner: train_core is a loop over class_frequencies, start_tree, grow_level (draw_slots,
// search_batch, decide_split, route_level) and fill_leaves.  The order-sensitive host arithmetic lives in train_host.h.
//
// Boosting (BoostedRandomForestLearner::learn, learning.cpp:1120-1234; classifier.cpp:238-307): boosted_core.  The
// training set is packed once; a round's resample is a multiplicity per example (`mult`, "the tree's data set") plus its
// index list, never a copy of the features.  The tree's bootstrap draws positions of that list; the class frequencies and
// the leaf histograms count example n mult[n] times, which is what the reference's learner sees on its treeData; routing
// moves every example of the whole set, so after fill_leaves node_of is the leaf of every ORIGINAL example and the
// round's error needs no second walk.  Build-owned definitions (the reference draws from std::random_device and has no
// guard for degenerate rounds; tests/boost_restate.py restates them independently):
//   1. Round key kb = mix64(seed ^ mix64(0x626F6F73 + round)).  Draw n is u_n = (float)(draw64(kb, n) >> 40) * 2^-24,
//      exact in fp32, in [0, 1).  The round's tree is learnt with seed_r = draw64(kb, 2^40) as tree 0 of a one-tree
//      forest -- tree_key(seed_r, 0), the node keys above, use_bootstrap on top of the resample -- so it equals the
//      oracle's learner run with num_trees = 1, seed = seed_r on the materialised resample X[idx].
//   2. Index: the first i with !(u > cumsum[i]), by binary search (cumsum does not decrease: the weights are >= 0),
//      clamped to N - 1 -- the reference reads past the array when rounding leaves cumsum[N-1] < u.
//   3. error, total and cumsum are fp32 sums in example order, bit for bit the serial chain.  Before the first round
//      the weights are 1.0f / N and cumsum[n] is the reference's closed form (n + 1) * 1.0f / N (:1140-1141).
//   4. Stops.  error == 0: the tree is added with the reference's alpha = +inf and boosting ends.  error >= 1, or a
//      total that is not positive and finite: the tree is not added and boosting ends.  Otherwise the reference's
//      arithmetic, negative alpha included.  The call reports how many trees it kept.
//   5. A loader stores a tree weight as w + 0.0f (forest_model.cpp), so -0.0 votes like the reference's 0 + (-0.0).
// alpha and exp(alpha) come from the host's libm (train_host.h: boost_round).
//
// The class-frequency-weighted objective (DecisionTreeLearner::setUseClassFrequency, learning.cpp:708-717;
// rvseg_forest_train_prior / rvseg_boosted_train_prior, single-layer): a Learner carries a rvseg_class_prior; unless its
// mode is NONE, grow_tree forms the tree's class weights after start_tree (tree_weights: the class counts of the
// bootstrapped set, class_prior_weights in train_host.h) and search_batch hands them to the two cut launches.  The
// definitions are in include/rvseg.h; everything but the objective of a cut is the learner above.
//
// Oracle: oracle/rvseg_oracle_train.c restates the reference learner depth-first with sorts; tests compare forest.dat
// byte for byte.  Both sides implement the same build-owned definitions, written down in that file's header: random
// choices from a counter-based generator keyed by (seed, tree, node path); the objective evaluated from the class counts
// by the expression of initEntropies (learning.cpp:279-293) with fastlog2 (fastlog.h:47-58), in float, classes in
// ascending order; bootstrap duplicates as multiplicities; the threshold guard (adjacent floats, overflowing sums).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "forest_model.h"
#include "rvseg_internal.h"
#include "rvseg_kernels.h"
#include "rvseg_pipeline.h"
#include "train_device.h"

namespace rvseg {
namespace {

constexpr int SLOT_BATCH = 1024;   // frontier nodes searched at once

// ---- the training set on the device (TrainSetView) and what the host knows about it -------------------------------
struct TrainSet {
    int P = 0, D = 0, L = 0;
    size_t stride = 0;                 // elements per feature row (>= P)
    DevBuf Xb, Xf, lab, nb_index_dev;
    std::vector<int> nb_index;         // [D]: row of the feature in Xf, -1 for a byte feature
    int n_nb = 0;
    std::vector<int> class_counts;
    // built where it is used: P is final only when the set is complete
    TrainSetView view() const { return {P, D, L, stride, Xb.as<uint8_t>(), Xf.as<float>(), lab.as<int>(), nb_index_dev.as<int>()}; }
};

// the rows of the set, once D, L, stride and nb_index are known
rvseg_status reserve_train_set(rvseg_ctx* ctx, TrainSet& T) {
    rvseg_status st;
    if ((st = dev_alloc(ctx, T.Xb, (size_t)T.D * T.stride)) != RVSEG_OK) return st;
    if ((st = dev_alloc(ctx, T.Xf, (size_t)std::max(T.n_nb, 1) * T.stride * sizeof(float))) != RVSEG_OK) return st;
    if ((st = dev_alloc(ctx, T.lab, (size_t)T.L * T.stride * sizeof(int))) != RVSEG_OK) return st;
    if ((st = dev_alloc(ctx, T.nb_index_dev, (size_t)T.D * sizeof(int))) != RVSEG_OK) return st;
    RV_HIP(ctx, hipMemcpyAsync(T.nb_index_dev.p, T.nb_index.data(), (size_t)T.D * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    return RVSEG_OK;
}

// grow-only with head room, for the arrays that follow the tree's node count: a deep tree does not reallocate at every
// level
rvseg_status reserve_grown(rvseg_ctx* ctx, DevBuf& b, size_t bytes) {
    if (b.p && b.bytes >= bytes) return RVSEG_OK;
    const size_t want = std::max<size_t>(bytes, 4096);
    return dev_alloc(ctx, b, want + want / 2);
}

// device memory of one training call; freed on return
struct TrainScratch {
    DevBuf weights, node_of;                    // [P] multiplicity in the tree's examples, node of every example
    DevBuf class_cnt;                           // [L][TR_CMAX]
    DevBuf hist, totals, cuts;                  // one slot batch: [S][K][TR_BINS][TR_CMAX], [S][TR_CMAX], CutResult[S][K]
    DevBuf slot_layer, slot_feat;               // slot tables of the batch
    DevBuf counter;                             // pairs the emit pass wrote
    DevBuf keysA, keysB, valsA, valsB, sort_temp;   // sorted path: at most min(K, n_nb) float features per example
    size_t nb_cap = 0, sort_temp_bytes = 0;
    DevBuf slot_of, split_feat, split_thr, split_left;   // [nodes] of a level (reserve_grown)
    DevBuf leaf_cnt;                            // [nodes][L][TR_CMAX] (reserve_grown)
};

struct Learner {
    rvseg_ctx* ctx;
    const TrainSet& T;
    const rvseg_train_params& tp;
    int K;                                      // features tried per node
    hipStream_t s;
    TrainScratch sc;
    std::vector<std::vector<float>> freq;       // [layer][class] inverted class frequency
    std::vector<CutResult> cuts;                // read-back of a batch
    std::vector<unsigned> totals;
    std::vector<int> perm;
    // a boosting round's data set (null: every example once): multiplicities [P] and the example at each position [P]
    const unsigned* mult = nullptr;
    const int* positions = nullptr;
    // the split objective (rvseg_class_prior; mode NONE: the integer one) and, when it is weighted, the current tree's weights
    rvseg_class_prior prior{};
    ClassWeights cw{};
    const ClassWeights* objective_weights() const { return prior.mode == RVSEG_PRIOR_NONE ? nullptr : &cw; }
};

rvseg_status reserve_scratch(Learner& R) {
    rvseg_ctx* ctx = R.ctx;
    TrainScratch& sc = R.sc;
    const size_t P = (size_t)R.T.P, K = (size_t)R.K;
    sc.nb_cap = R.T.n_nb ? P * (size_t)std::min(R.K, R.T.n_nb) : 0;
    if (sc.nb_cap >= (1ull << 32)) { ctx->err = "training set too large for the sorted feature path"; return RVSEG_ERR_CAPACITY; }
    struct Want { DevBuf& b; size_t bytes; };
    auto alloc_all = [ctx](std::initializer_list<Want> list) {
        for (const Want& w : list) {
            const rvseg_status st = dev_alloc(ctx, w.b, w.bytes);
            if (st != RVSEG_OK) return st;
        }
        return RVSEG_OK;
    };
    rvseg_status st = alloc_all({{sc.weights, P * 4}, {sc.node_of, P * 4}, {sc.class_cnt, (size_t)R.T.L * TR_CMAX * 4},
                                 {sc.hist, (size_t)SLOT_BATCH * K * TR_BINS * TR_CMAX * 4}, {sc.totals, (size_t)SLOT_BATCH * TR_CMAX * 4},
                                 {sc.cuts, (size_t)SLOT_BATCH * K * sizeof(CutResult)}, {sc.slot_layer, (size_t)SLOT_BATCH * 4},
                                 {sc.slot_feat, (size_t)SLOT_BATCH * K * 4}, {sc.counter, 16}});
    if (st != RVSEG_OK) return st;
    if (sc.nb_cap) {   // the set has a float feature
        sc.sort_temp_bytes = train_sort_temp_bytes(sc.nb_cap);
        // (dev_alloc never hands out a null block: a null sort_temp would turn the sort into a size query)
        st = alloc_all({{sc.keysA, sc.nb_cap * 8}, {sc.keysB, sc.nb_cap * 8}, {sc.valsA, sc.nb_cap * 4}, {sc.valsB, sc.nb_cap * 4},
                        {sc.sort_temp, sc.sort_temp_bytes}});
        if (st != RVSEG_OK) return st;
    }
    R.cuts.resize((size_t)SLOT_BATCH * K);
    R.totals.resize((size_t)SLOT_BATCH * TR_CMAX);
    R.perm.resize((size_t)R.T.D);
    return RVSEG_OK;
}

// inverted class frequencies over the tree's data set (data.h:358-370): freq[c] = size / count_c, in float
rvseg_status class_frequencies(Learner& R) {
    rvseg_ctx* ctx = R.ctx;
    const int L = R.T.L;
    std::vector<unsigned> class_cnt((size_t)L * TR_CMAX);
    RV_HIP(ctx, hipMemsetAsync(R.sc.class_cnt.p, 0, class_cnt.size() * 4, R.s));
    launch_train_class_count(R.T.view(), R.mult, R.sc.class_cnt.as<unsigned>(), R.s);
    RV_HIP(ctx, hipMemcpyAsync(class_cnt.data(), R.sc.class_cnt.p, class_cnt.size() * 4, hipMemcpyDeviceToHost, R.s));
    RV_HIP(ctx, hipStreamSynchronize(R.s));
    RV_LAUNCH_OK(ctx);
    R.freq.assign(L, {});
    for (int l = 0; l < L; l++)
        for (int c = 0; c < R.T.class_counts[l]; c++) R.freq[l].push_back(inverted_frequency(R.T.P, class_cnt[(size_t)l * TR_CMAX + c]));
    return RVSEG_OK;
}

// the tree's examples: P bootstrap draws from its data set as multiplicities, or the data set as it is; all at the root
rvseg_status start_tree(Learner& R, uint64_t kt) {
    rvseg_ctx* ctx = R.ctx;
    const size_t P = (size_t)R.T.P;
    if (R.tp.use_bootstrap) {
        RV_HIP(ctx, hipMemsetAsync(R.sc.weights.p, 0, P * 4, R.s));
        launch_train_bootstrap(R.T.P, kt, R.positions, R.sc.weights.as<unsigned>(), R.s);
    } else if (R.mult) {
        RV_HIP(ctx, hipMemcpyAsync(R.sc.weights.p, R.mult, P * 4, hipMemcpyDeviceToDevice, R.s));
    } else {
        RV_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)R.sc.weights.p, 1, P, R.s));
    }
    RV_HIP(ctx, hipMemsetAsync(R.sc.node_of.p, 0, P * 4, R.s));
    return RVSEG_OK;
}

// the tree's class weights (rvseg_class_prior, definition 1) from the class counts of its examples: start_tree's
// multiplicities, i.e. the data set after the bootstrap
rvseg_status tree_weights(Learner& R) {
    rvseg_ctx* ctx = R.ctx;
    unsigned cnt[TR_CMAX];
    RV_HIP(ctx, hipMemsetAsync(R.sc.class_cnt.p, 0, sizeof(cnt), R.s));
    launch_train_class_count(R.T.view(), R.sc.weights.as<unsigned>(), R.sc.class_cnt.as<unsigned>(), R.s);
    RV_HIP(ctx, hipMemcpyAsync(cnt, R.sc.class_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, R.s));
    RV_HIP(ctx, hipStreamSynchronize(R.s));
    RV_LAUNCH_OK(ctx);
    class_prior_weights(R.prior, cnt, R.T.class_counts[0], R.cw.w);
    return RVSEG_OK;
}

// the host's random choices for the nodes of one batch, in the oracle's draw order (definition 1)
struct SlotDraw {
    std::vector<int> layer, feat;   // [S], [S][K]
    bool any_float = false;         // a float feature was sampled: the batch needs the sorted path
};
SlotDraw draw_slots(Learner& R, const GrowingTree& tree, const int* nodes, int S) {
    const int D = R.T.D, K = R.K;
    SlotDraw d;
    d.layer.resize(S);
    d.feat.resize((size_t)S * K);
    for (int q = 0; q < S; q++) {
        const uint64_t key = tree.key[nodes[q]];
        d.layer[q] = (int)(draw64(key, 0) % (uint64_t)R.T.L);                                   // "Pick a random class layer", :483-485
        for (int f = 0; f < D; f++) R.perm[f] = f;                                              // numFeatures without replacement, :537
        for (int k = 0; k < K; k++) {
            const int j = k + (int)(draw64(key, 1 + (uint64_t)k) % (uint64_t)(D - k));
            std::swap(R.perm[k], R.perm[j]);
            d.feat[(size_t)q * K + k] = R.perm[k];
            d.any_float = d.any_float || R.T.nb_index[R.perm[k]] >= 0;
        }
    }
    return d;
}

// float features of a batch: emit -> count read-back -> sort -> scan (learning.cpp:560-604)
rvseg_status search_floats(Learner& R, const TrainSetView& v, const LevelSlots& sl, int S) {
    rvseg_ctx* ctx = R.ctx;
    TrainScratch& sc = R.sc;
    RV_HIP(ctx, hipMemsetAsync(sc.counter.p, 0, 16, R.s));
    launch_train_emit(v, sl, sc.keysA.as<unsigned long long>(), sc.valsA.as<unsigned>(), sc.counter.as<unsigned>(), (unsigned)sc.nb_cap, R.s);
    unsigned n_items = 0;
    RV_HIP(ctx, hipMemcpyAsync(&n_items, sc.counter.p, 4, hipMemcpyDeviceToHost, R.s));
    RV_HIP(ctx, hipStreamSynchronize(R.s));
    RV_LAUNCH_OK(ctx);
    n_items = (unsigned)std::min<size_t>(n_items, sc.nb_cap);
    const DevBuf *keys = &sc.keysA, *vals = &sc.valsA;
    if (n_items > 1) {
        int seg_bits = 1;
        while ((1u << seg_bits) < (unsigned)(S * R.K)) seg_bits++;
        RV_HIP(ctx, launch_train_sort(sc.sort_temp.p, sc.sort_temp_bytes, sc.keysA.as<unsigned long long>(), sc.keysB.as<unsigned long long>(),
                                      sc.valsA.as<unsigned>(), sc.valsB.as<unsigned>(), (size_t)n_items, (unsigned)(32 + seg_bits), R.s));
        keys = &sc.keysB;
        vals = &sc.valsB;
    }
    launch_train_scan(v, sl, S, R.objective_weights(), n_items, keys->as<unsigned long long>(), vals->as<unsigned>(), sc.totals.as<unsigned>(), sc.cuts.as<CutResult>(), R.s);
    return RVSEG_OK;
}

// One batch of slots on the device: slot_of maps every node of the level to its slot in the batch or -1.  Leaves the
// class totals (the node's histogram, learning.cpp:508-516) and the cut records of the batch in R.totals / R.cuts.
rvseg_status search_batch(Learner& R, const std::vector<int>& slot_of, const SlotDraw& d) {
    rvseg_ctx* ctx = R.ctx;
    TrainScratch& sc = R.sc;
    const size_t S = d.layer.size(), K = (size_t)R.K;
    RV_HIP(ctx, hipMemcpyAsync(sc.slot_of.p, slot_of.data(), slot_of.size() * 4, hipMemcpyHostToDevice, R.s));
    RV_HIP(ctx, hipMemcpyAsync(sc.slot_layer.p, d.layer.data(), S * 4, hipMemcpyHostToDevice, R.s));
    RV_HIP(ctx, hipMemcpyAsync(sc.slot_feat.p, d.feat.data(), S * K * 4, hipMemcpyHostToDevice, R.s));
    RV_HIP(ctx, hipMemsetAsync(sc.hist.p, 0, S * K * TR_BINS * TR_CMAX * 4, R.s));
    RV_HIP(ctx, hipMemsetAsync(sc.totals.p, 0, S * TR_CMAX * 4, R.s));
    const TrainSetView v = R.T.view();
    const LevelSlots sl{R.K, sc.node_of.as<int>(), sc.slot_of.as<int>(), sc.weights.as<unsigned>(), sc.slot_layer.as<int>(), sc.slot_feat.as<int>()};
    launch_train_search_bytes(v, sl, (int)S, R.objective_weights(), sc.totals.as<unsigned>(), sc.hist.as<unsigned>(), sc.cuts.as<CutResult>(), R.s);
    if (d.any_float) {
        const rvseg_status st = search_floats(R, v, sl, (int)S);
        if (st != RVSEG_OK) return st;
    }
    RV_HIP(ctx, hipMemcpyAsync(R.cuts.data(), sc.cuts.p, S * K * sizeof(CutResult), hipMemcpyDeviceToHost, R.s));
    RV_HIP(ctx, hipMemcpyAsync(R.totals.data(), sc.totals.p, S * TR_CMAX * 4, hipMemcpyDeviceToHost, R.s));
    RV_HIP(ctx, hipStreamSynchronize(R.s));
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// the nodes of a level that were split, indexed by node: feat < 0 = not split
struct LevelSplits {
    std::vector<int> feat, left;
    std::vector<float> thr;
    explicit LevelSplits(int n_nodes) : feat(n_nodes, -1), left(n_nodes, 0), thr(n_nodes, 0.f) {}
};

// findLeafNode's rule on the freshly split nodes: every example (bootstrap or not) moves to a child
rvseg_status route_level(Learner& R, const LevelSplits& sp) {
    rvseg_ctx* ctx = R.ctx;
    TrainScratch& sc = R.sc;
    const size_t bytes = sp.feat.size() * 4;
    rvseg_status st;
    if ((st = reserve_grown(ctx, sc.split_feat, bytes)) != RVSEG_OK || (st = reserve_grown(ctx, sc.split_thr, bytes)) != RVSEG_OK ||
        (st = reserve_grown(ctx, sc.split_left, bytes)) != RVSEG_OK)
        return st;
    RV_HIP(ctx, hipMemcpyAsync(sc.split_feat.p, sp.feat.data(), bytes, hipMemcpyHostToDevice, R.s));
    RV_HIP(ctx, hipMemcpyAsync(sc.split_thr.p, sp.thr.data(), bytes, hipMemcpyHostToDevice, R.s));
    RV_HIP(ctx, hipMemcpyAsync(sc.split_left.p, sp.left.data(), bytes, hipMemcpyHostToDevice, R.s));
    launch_train_route(R.T.view(), sc.node_of.as<int>(), sc.split_feat.as<int>(), sc.split_thr.as<float>(), sc.split_left.as<int>(), R.s);
    RV_HIP(ctx, hipStreamSynchronize(R.s));   // the caller's host vectors go out of scope
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// One level: searches the frontier in batches, splits what decide_split says, routes the examples; `frontier` becomes the
// next level's.
rvseg_status grow_level(Learner& R, GrowingTree& tree, std::vector<int>& frontier) {
    const int n_nodes = tree.size(), K = R.K;
    rvseg_status st;
    if ((st = reserve_grown(R.ctx, R.sc.slot_of, (size_t)n_nodes * 4)) != RVSEG_OK) return st;
    std::vector<int> slot_of(n_nodes, -1), next_frontier;
    LevelSplits sp(n_nodes);
    for (size_t base = 0; base < frontier.size(); base += SLOT_BATCH) {
        const int S = (int)std::min<size_t>(SLOT_BATCH, frontier.size() - base);
        const int* nodes = frontier.data() + base;
        std::fill(slot_of.begin(), slot_of.end(), -1);
        for (int q = 0; q < S; q++) slot_of[nodes[q]] = q;
        const SlotDraw d = draw_slots(R, tree, nodes, S);
        if ((st = search_batch(R, slot_of, d)) != RVSEG_OK) return st;
        for (int q = 0; q < S; q++) {
            const int node = nodes[q];
            const Split c = decide_split(&R.totals[(size_t)q * TR_CMAX], &R.cuts[(size_t)q * K], &d.feat[(size_t)q * K], K, tree.depth[node], R.tp);
            if (!c.split) continue;
            const int lc = tree.split(node, c.feature, c.threshold);
            sp.feat[node] = c.feature; sp.thr[node] = c.threshold; sp.left[node] = lc;
            next_frontier.push_back(lc);
            next_frontier.push_back(lc + 1);
        }
    }
    if (!next_frontier.empty() && (st = route_level(R, sp)) != RVSEG_OK) return st;
    frontier.swap(next_frontier);
    return RVSEG_OK;
}

// leaf histograms from ALL examples of the tree's data set (updateMultiHistograms, learning.cpp:960-1012): integer counts on the device, the
// float accumulation of leaf_histograms on the host
rvseg_status fill_leaves(Learner& R, GrowingTree& tree) {
    rvseg_ctx* ctx = R.ctx;
    const size_t n_nodes = (size_t)tree.size(), per_node = (size_t)R.T.L * TR_CMAX;
    std::vector<unsigned> cnt(n_nodes * per_node);
    const rvseg_status st = reserve_grown(ctx, R.sc.leaf_cnt, cnt.size() * 4);
    if (st != RVSEG_OK) return st;
    RV_HIP(ctx, hipMemsetAsync(R.sc.leaf_cnt.p, 0, cnt.size() * 4, R.s));
    launch_train_leaf_count(R.T.view(), R.sc.node_of.as<int>(), R.mult, R.sc.leaf_cnt.as<unsigned>(), R.s);
    RV_HIP(ctx, hipMemcpyAsync(cnt.data(), R.sc.leaf_cnt.p, cnt.size() * 4, hipMemcpyDeviceToHost, R.s));
    RV_HIP(ctx, hipStreamSynchronize(R.s));
    RV_LAUNCH_OK(ctx);
    tree.mhist.assign(n_nodes, {});
    for (size_t v = 0; v < n_nodes; v++)
        if (tree.left[v] == 0) tree.mhist[v] = leaf_histograms(&cnt[v * per_node], R.freq, R.tp.smoothing);
    return RVSEG_OK;
}

// one tree over the learner's data set, in level order, leaves filled
rvseg_status grow_tree(Learner& R, uint64_t kt, GrowingTree& tree) {
    rvseg_status st;
    if ((st = start_tree(R, kt)) != RVSEG_OK) return st;
    if (R.objective_weights() && (st = tree_weights(R)) != RVSEG_OK) return st;
    std::vector<int> frontier(1, 0);
    while (!frontier.empty())
        if ((st = grow_level(R, tree, frontier)) != RVSEG_OK) return st;
    return fill_leaves(R, tree);
}

// autoconf, :363-368
int features_per_node(int D, const rvseg_train_params& tp) { return std::min(D, tp.num_features > 0 ? tp.num_features : (int)std::ceil(std::sqrt((double)D))); }

// ---- the learner over a device-resident training set ---------------------------------------------------------------
rvseg_status train_core(rvseg_ctx* ctx, const TrainSet& T, const rvseg_train_params& tp, const rvseg_class_prior& prior,
                        std::vector<uint8_t>& bytes_out) {
    Learner R{ctx, T, tp, features_per_node(T.D, tp), ctx->stream};
    R.prior = prior;
    rvseg_status st;
    if ((st = reserve_scratch(R)) != RVSEG_OK || (st = class_frequencies(R)) != RVSEG_OK) return st;
    ForestModel model;
    model.raw.reserve((size_t)tp.num_trees);
    for (int t = 0; t < tp.num_trees; t++) {
        const uint64_t kt = tree_key(tp.seed, t);
        GrowingTree tree(root_key(kt));
        if ((st = grow_tree(R, kt, tree)) != RVSEG_OK) return st;
        model.raw.push_back(renumber_depth_first(std::move(tree)));
    }
    bytes_out = serialize_forest(model);
    return RVSEG_OK;
}

// ---- boosting --------------------------------------------------------------------------------------------------
// device memory of the boosting rounds; freed on return
struct BoostScratch {
    DevBuf w, cumsum;        // [N] example weights and their running sum
    DevBuf miss;             // [N] bytes
    DevBuf idx, mult;        // [N] the round's resample: example per draw, draws per example
    DevBuf vote;             // [nodes] vote label per node of the growing tree (reserve_grown)
    DevBuf sums;             // error, total
};

rvseg_status reserve_boost(rvseg_ctx* ctx, BoostScratch& b, size_t N) {
    rvseg_status st;
    if ((st = dev_alloc(ctx, b.w, N * 4)) != RVSEG_OK || (st = dev_alloc(ctx, b.cumsum, N * 4)) != RVSEG_OK ||
        (st = dev_alloc(ctx, b.miss, N)) != RVSEG_OK || (st = dev_alloc(ctx, b.idx, N * 4)) != RVSEG_OK ||
        (st = dev_alloc(ctx, b.mult, N * 4)) != RVSEG_OK || (st = dev_alloc(ctx, b.sums, 16)) != RVSEG_OK)
        return st;
    return RVSEG_OK;
}

// the two sums the stop rules need on the host
rvseg_status boost_error(rvseg_ctx* ctx, BoostScratch& b, int N, float* error, hipStream_t s) {
    launch_train_boost_error(b.w.as<float>(), b.miss.as<uint8_t>(), N, b.sums.as<float>(), s);
    RV_HIP(ctx, hipMemcpyAsync(error, b.sums.p, 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}
rvseg_status boost_total(rvseg_ctx* ctx, BoostScratch& b, int N, float scale, float* total, hipStream_t s) {
    launch_train_boost_update_total(b.w.as<float>(), b.miss.as<uint8_t>(), N, scale, b.sums.as<float>() + 1, s);
    RV_HIP(ctx, hipMemcpyAsync(total, b.sums.as<float>() + 1, 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// miss[n] for every example of the whole set from the leaf it was routed to (tree->classify, :1184)
rvseg_status vote_flags(Learner& R, BoostScratch& b, const GrowingTree& tree) {
    rvseg_ctx* ctx = R.ctx;
    std::vector<int> vote((size_t)tree.size(), 0);
    for (int v = 0; v < tree.size(); v++)
        if (tree.left[v] == 0) vote[(size_t)v] = vote_label(tree.mhist[(size_t)v][0].data(), (int)tree.mhist[(size_t)v][0].size());
    const rvseg_status st = reserve_grown(ctx, b.vote, vote.size() * 4);
    if (st != RVSEG_OK) return st;
    RV_HIP(ctx, hipMemcpyAsync(b.vote.p, vote.data(), vote.size() * 4, hipMemcpyHostToDevice, R.s));
    launch_train_vote_flags(R.sc.node_of.as<int>(), b.vote.as<int>(), R.T.lab.as<int>(), R.T.P, b.miss.as<uint8_t>(), R.s);
    RV_HIP(ctx, hipStreamSynchronize(R.s));   // `vote` goes out of scope
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// the rounds; `model` receives the kept trees and their weights, errors / alphas (num_trees each, or null) the rounds'
rvseg_status boosted_core(rvseg_ctx* ctx, const TrainSet& T, const rvseg_train_params& tp, const rvseg_class_prior& prior, int C,
                          ForestModel& model, float* errors, float* alphas) {
    const int N = T.P;
    Learner R{ctx, T, tp, features_per_node(T.D, tp), ctx->stream};
    R.prior = prior;
    BoostScratch b;
    rvseg_status st;
    if ((st = reserve_scratch(R)) != RVSEG_OK || (st = reserve_boost(ctx, b, (size_t)N)) != RVSEG_OK) return st;
    {   // :1138-1143
        std::vector<float> w((size_t)N), cs((size_t)N);
        for (int n = 0; n < N; n++) { w[(size_t)n] = 1.0f / N; cs[(size_t)n] = (n + 1) * 1.0f / N; }
        RV_HIP(ctx, hipMemcpyAsync(b.w.p, w.data(), (size_t)N * 4, hipMemcpyHostToDevice, R.s));
        RV_HIP(ctx, hipMemcpyAsync(b.cumsum.p, cs.data(), (size_t)N * 4, hipMemcpyHostToDevice, R.s));
        RV_HIP(ctx, hipStreamSynchronize(R.s));
    }
    model = ForestModel();
    model.boosted = true;
    model.boosted_order = RVSEG_BOOSTED_WEIGHT_FIRST;
    R.mult = b.mult.as<unsigned>();
    R.positions = b.idx.as<int>();
    for (int round = 0; round < tp.num_trees; round++) {
        const uint64_t kb = boost_round_key(tp.seed, round);
        RV_HIP(ctx, hipMemsetAsync(b.mult.p, 0, (size_t)N * 4, R.s));
        launch_train_boost_resample(b.cumsum.as<float>(), N, kb, b.idx.as<int>(), b.mult.as<unsigned>(), R.s);
        if ((st = class_frequencies(R)) != RVSEG_OK) return st;
        const uint64_t kt = tree_key(boost_tree_seed(kb), 0);
        GrowingTree tree(root_key(kt));
        if ((st = grow_tree(R, kt, tree)) != RVSEG_OK || (st = vote_flags(R, b, tree)) != RVSEG_OK) return st;
        float error = 0.f, total = 0.f;
        if ((st = boost_error(ctx, b, N, &error, R.s)) != RVSEG_OK) return st;
        if (errors) errors[round] = error;
        const BoostRound br = boost_round(error, C);
        if (!br.keep_tree) break;
        if (br.go_on) {
            if ((st = boost_total(ctx, b, N, br.scale, &total, R.s)) != RVSEG_OK) return st;
            if (!boost_total_ok(total)) break;
        }
        if (alphas) alphas[round] = br.alpha;
        model.raw.push_back(renumber_depth_first(std::move(tree)));   // addTree(tree, alpha), :1220
        model.tree_weights.push_back(br.alpha);
        if (!br.go_on) break;
        if (round + 1 < tp.num_trees)   // (nothing reads the weights after the last round)
            launch_train_boost_update_cumsum(b.w.as<float>(), N, b.sums.as<float>() + 1, b.cumsum.as<float>(), R.s);
    }
    RV_HIP(ctx, hipStreamSynchronize(R.s));
    RV_LAUNCH_OK(ctx);
    model.n_trees = (int)model.raw.size();
    return RVSEG_OK;
}

// ---- what the two entry points share -------------------------------------------------------------------------------
rvseg_train_params resolve_params(const rvseg_train_params* tp_in) {
    rvseg_train_params tp;
    if (tp_in) tp = *tp_in; else rvseg_train_params_default(&tp);
    return tp;
}

rvseg_status check_train_args(rvseg_ctx* ctx, int32_t n_layers, const int32_t* class_counts, const rvseg_train_params& tp, int D) {
    if (!class_counts || n_layers < 1 || n_layers > RVSEG_MAX_LAYERS || tp.num_trees < 1 || tp.num_trees > kMaxTrees || tp.max_depth < 1 ||
        tp.min_split_examples < 0 || tp.min_child_split_examples < 0 || tp.num_features < 0 || tp.num_features > D || !(tp.smoothing >= 0.f)) {
        ctx->err = "bad arguments";
        return RVSEG_ERR_INVALID_ARG;
    }
    int sumC = 0;
    for (int l = 0; l < n_layers; l++) {
        if (class_counts[l] < 1 || class_counts[l] > TR_CMAX) { ctx->err = "the trainer handles 1..16 classes per layer"; return RVSEG_ERR_INVALID_ARG; }
        sumC += class_counts[l];
    }
    if (sumC > kMaxClasses) { ctx->err = "more than 64 classes over all layers"; return RVSEG_ERR_INVALID_ARG; }
    return RVSEG_OK;
}

// the label rule: the n labels of one layer, `step` apart, are class indices of that layer
rvseg_status labels_in_range(rvseg_ctx* ctx, const int32_t* lab, size_t n, size_t step, int n_classes) {
    for (size_t i = 0; i < n; i++)
        if (lab[i * step] < 0 || lab[i * step] >= n_classes) { ctx->err = "label outside its layer's class range"; return RVSEG_ERR_INVALID_ARG; }
    return RVSEG_OK;
}

// the model of the last training call on a context (so that a caller whose buffer was too small need not train again)
rvseg_status hand_out(rvseg_ctx* ctx, void* forest_out, size_t out_cap, size_t* size_out) {
    const std::vector<uint8_t>& b = ctx->trained_model;
    if (size_out) *size_out = b.size();
    if (!forest_out) return RVSEG_OK;
    if (out_cap < b.size()) { ctx->err = "output buffer too small (the model is kept: rvseg_forest_train_result)"; return RVSEG_ERR_INVALID_ARG; }
    std::memcpy(forest_out, b.data(), b.size());
    return RVSEG_OK;
}

// the integer objective: what the multi-layer and the frames entry points always run
const rvseg_class_prior kNoPrior{};   // mode RVSEG_PRIOR_NONE

// a prior as the learner takes it: null is NONE; a refused one leaves the context's models as they are
rvseg_status resolve_prior(rvseg_ctx* ctx, const rvseg_class_prior* prior_in, int C, rvseg_class_prior& prior) {
    if (const char* what = class_prior_error(prior_in, C)) { ctx->err = what; return RVSEG_ERR_INVALID_ARG; }
    prior = prior_in ? *prior_in : kNoPrior;
    return RVSEG_OK;
}

// trains on the complete set; only a successful training replaces the context's model
rvseg_status finish_training(rvseg_ctx* ctx, const TrainSet& T, const rvseg_train_params& tp, const rvseg_class_prior& prior, void* forest_out,
                             size_t out_cap, size_t* size_out) {
    const rvseg_status st = train_core(ctx, T, tp, prior, ctx->trained_model);
    if (st != RVSEG_OK) return st;
    return hand_out(ctx, forest_out, out_cap, size_out);
}

// the P x D host matrix and its P x L labels as a packed training set on the device
rvseg_status pack_matrix(rvseg_ctx* ctx, const float* X, int P, int D, const int32_t* labels, int n_layers, const int32_t* class_counts,
                         TrainSet& T) {
    hipStream_t s = ctx->stream;
    rvseg_status st;
    T.P = P; T.D = D; T.L = n_layers; T.stride = (size_t)P;
    T.class_counts.assign(class_counts, class_counts + n_layers);
    // which features are byte-valued is decided by value
    DevBuf dX, dNotByte, dNotFinite;
    if ((st = dev_alloc(ctx, dX, (size_t)P * D * 4)) != RVSEG_OK || (st = dev_alloc(ctx, dNotByte, (size_t)D * 4)) != RVSEG_OK ||
        (st = dev_alloc(ctx, dNotFinite, 16)) != RVSEG_OK)
        return st;
    RV_HIP(ctx, hipMemcpyAsync(dX.p, X, (size_t)P * D * 4, hipMemcpyHostToDevice, s));
    RV_HIP(ctx, hipMemsetAsync(dNotByte.p, 0, (size_t)D * 4, s));
    RV_HIP(ctx, hipMemsetAsync(dNotFinite.p, 0, 16, s));
    launch_train_feature_stats(dX.as<float>(), P, D, dNotByte.as<int>(), dNotFinite.as<int>(), s);
    std::vector<int> not_byte(D);
    int not_finite = 0;
    RV_HIP(ctx, hipMemcpyAsync(not_byte.data(), dNotByte.p, (size_t)D * 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipMemcpyAsync(&not_finite, dNotFinite.p, 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    RV_LAUNCH_OK(ctx);
    if (not_finite) { ctx->err = "non-finite feature value in the training set"; return RVSEG_ERR_INVALID_ARG; }
    T.nb_index.assign(D, -1);
    for (int f = 0; f < D; f++) if (not_byte[f]) T.nb_index[f] = T.n_nb++;
    if ((st = reserve_train_set(ctx, T)) != RVSEG_OK) return st;
    std::vector<int> lab_lm((size_t)P * n_layers);   // layer-major, like the rows of X
    for (int i = 0; i < P; i++)
        for (int l = 0; l < n_layers; l++) lab_lm[(size_t)l * P + i] = labels[(size_t)i * n_layers + l];
    RV_HIP(ctx, hipMemcpyAsync(T.lab.p, lab_lm.data(), lab_lm.size() * 4, hipMemcpyHostToDevice, s));
    launch_train_pack(dX.as<float>(), T.view(), s);
    RV_HIP(ctx, hipStreamSynchronize(s));
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// ---- frames -> training set on the device (src/train.cpp:115-147) -------------------------------------------------
// One variant of a frame on the host: the colour offset `a` and the horizontal flip of colour, depth and labels.
void augment_variant(const FrameGeom& g, int n_layers, const uint8_t* src_rgb, const uint16_t* src_d, const int8_t* src_l, int a, bool flip,
                     uint8_t* rgb, uint16_t* depth, int8_t* lab) {
    const size_t npix = (size_t)g.W * g.H;
    for (int y = 0; y < g.H; y++)
        for (int x = 0; x < g.W; x++) {
            const size_t d = (size_t)y * g.W + x, q = (size_t)y * g.W + (flip ? g.W - 1 - x : x);
            // `color += a` on an 8UC3 cv::Mat: the scalar becomes cv::Scalar(a, 0, 0, 0) -- only channel 0 moves --
            // with saturate_cast<uchar> (OpenCV's scalar rule; train.cpp:122)
            int c0 = (int)src_rgb[q * 3] + a;
            c0 = c0 < 0 ? 0 : (c0 > 255 ? 255 : c0);
            rgb[d * 3] = (uint8_t)c0; rgb[d * 3 + 1] = src_rgb[q * 3 + 1]; rgb[d * 3 + 2] = src_rgb[q * 3 + 2];
            depth[d] = src_d[q];
            for (int l = 0; l < n_layers; l++) lab[(size_t)l * npix + d] = src_l[(size_t)l * npix + q];
        }
}

// staging of the frames entry: one variant on the host, its labels and the compaction of its points on the device
struct FrameStage {
    std::vector<uint8_t> h_rgb;
    std::vector<uint16_t> h_depth;
    std::vector<int8_t> h_lab;
    DevBuf labels, flags, offs, scan_temp;
    size_t scan_bytes = 0;
};

// Appends the labelled points with valid depth of the staged variant to the set at row `base` (FeatureExtractor::extract,
// WITH_POSITIVE_LABEL) and advances it.
rvseg_status append_variant(rvseg_ctx* ctx, Pipeline* im, FrameStage& fs, const float* calib, TrainSet& T, size_t* base) {
    const FrameGeom& g = im->geom;
    const size_t npix = (size_t)g.W * g.H;
    const int Pg = g.lw * g.lh;
    hipStream_t s = ctx->stream;
    rvseg_status st;
    RV_HIP(ctx, hipMemcpyAsync(im->in_rgb.p, fs.h_rgb.data(), npix * 3, hipMemcpyHostToDevice, s));
    RV_HIP(ctx, hipMemcpyAsync(im->in_depth.p, fs.h_depth.data(), npix * 2, hipMemcpyHostToDevice, s));
    RV_HIP(ctx, hipMemcpyAsync(fs.labels.p, fs.h_lab.data(), fs.h_lab.size(), hipMemcpyHostToDevice, s));
    if ((st = upload_calib(ctx, im, calib, 1, s)) != RVSEG_OK) return st;
    if ((st = dump_frame_features(ctx, im, s)) != RVSEG_OK) return st;
    launch_train_frame_flags(g, im->valid.as<uint8_t>(), fs.labels.as<int8_t>(), T.L, fs.flags.as<int>(), s);
    RV_HIP(ctx, launch_train_scan_offsets(fs.scan_temp.p, fs.scan_bytes, fs.flags.as<int>(), fs.offs.as<int>(), (size_t)Pg, s));
    launch_train_frame_scatter(g, fs.flags.as<int>(), fs.offs.as<int>(), im->dump.as<float>(), fs.labels.as<int8_t>(), *base, T.view(), s);
    int last_off = 0, last_flag = 0;
    RV_HIP(ctx, hipMemcpyAsync(&last_off, fs.offs.as<int>() + (Pg - 1), 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipMemcpyAsync(&last_flag, fs.flags.as<int>() + (Pg - 1), 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));   // (also: the host staging vectors are rewritten by the next variant)
    RV_LAUNCH_OK(ctx);
    *base += (size_t)(last_off + last_flag);
    return RVSEG_OK;
}

// the label rule on the device copy of the frames entry: one small read-back per layer
rvseg_status check_device_labels(rvseg_ctx* ctx, const TrainSet& T) {
    std::vector<int32_t> hl((size_t)T.P);
    for (int l = 0; l < T.L; l++) {
        RV_HIP(ctx, hipMemcpyAsync(hl.data(), T.lab.as<int>() + (size_t)l * T.stride, hl.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        RV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const rvseg_status st = labels_in_range(ctx, hl.data(), hl.size(), 1, T.class_counts[l]);
        if (st != RVSEG_OK) return st;
    }
    return RVSEG_OK;
}

// rvseg_forest_train and rvseg_forest_train_prior: the host matrix, packed and learnt with the objective of `prior`
rvseg_status train_matrix(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, const int32_t* labels, int32_t n_layers,
                          const int32_t* class_counts, const rvseg_train_params* tp_in, const rvseg_class_prior& prior, void* forest_out,
                          size_t out_cap, size_t* size_out) {
    const rvseg_train_params tp = resolve_params(tp_in);
    if (!X || !labels || !size_out || P < 1 || D < 1) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    rvseg_status st = check_train_args(ctx, n_layers, class_counts, tp, D);
    if (st != RVSEG_OK) return st;
    for (int l = 0; l < n_layers; l++)
        if ((st = labels_in_range(ctx, labels + l, (size_t)P, (size_t)n_layers, class_counts[l])) != RVSEG_OK) return st;
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    TrainSet T;
    if ((st = pack_matrix(ctx, X, P, D, labels, n_layers, class_counts, T)) != RVSEG_OK) return st;
    return finish_training(ctx, T, tp, prior, forest_out, out_cap, size_out);
}

// rvseg_boosted_train and rvseg_boosted_train_prior: the boosting rounds with the trees' objective of `prior`
rvseg_status boosted_matrix(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, const int32_t* labels, int32_t C,
                            const rvseg_train_params* tp_in, const rvseg_class_prior& prior, void* out, size_t out_cap, size_t* size_out,
                            float* errors_out, float* alphas_out, int32_t* rounds_out) {
    const rvseg_train_params tp = resolve_params(tp_in);
    if (!X || !labels || !size_out || P < 1 || D < 1) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    rvseg_status st = check_train_args(ctx, 1, &C, tp, D);
    if (st != RVSEG_OK) return st;
    if (C < 2) { ctx->err = "boosting needs at least 2 classes (alpha takes log(C - 1))"; return RVSEG_ERR_INVALID_ARG; }
    if ((st = labels_in_range(ctx, labels, (size_t)P, 1, C)) != RVSEG_OK) return st;
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    TrainSet T;
    if ((st = pack_matrix(ctx, X, P, D, labels, 1, &C, T)) != RVSEG_OK) return st;
    const float nan = std::nanf("");
    for (int r = 0; r < tp.num_trees; r++) {
        if (errors_out) errors_out[r] = nan;
        if (alphas_out) alphas_out[r] = nan;
    }
    ForestModel model;
    if ((st = boosted_core(ctx, T, tp, prior, C, model, errors_out, alphas_out)) != RVSEG_OK) return st;
    if (rounds_out) *rounds_out = model.n_trees;
    const std::vector<uint8_t> bytes = serialize_boosted(model, RVSEG_BOOSTED_WEIGHT_FIRST);
    ctx->trained_boosted = std::move(model);   // only a successful training replaces the kept model
    *size_out = bytes.size();
    if (!out) return RVSEG_OK;
    if (out_cap < bytes.size()) { ctx->err = "output buffer too small (the model is kept: rvseg_boosted_train_result)"; return RVSEG_ERR_INVALID_ARG; }
    std::memcpy(out, bytes.data(), bytes.size());
    return RVSEG_OK;
}

}  // namespace
}  // namespace rvseg

using namespace rvseg;

extern "C" {

void rvseg_train_params_default(rvseg_train_params* tp) {
    if (!tp) return;
    std::memset(tp, 0, sizeof(*tp));
    tp->num_trees = 4;                  // resources/config.json:37
    tp->max_depth = 30;                 // :38
    tp->min_split_examples = 50;        // :39
    tp->min_child_split_examples = 1;   // learning.h:116
    tp->num_features = 0;               // ceil(sqrt(D)), DecisionTreeLearner::autoconf (learning.cpp:363-368)
    tp->use_bootstrap = 1;              // train.cpp:226
    tp->smoothing = 1.0f;               // learning.h:117
    tp->seed = 1;
}

rvseg_status rvseg_forest_train_result(rvseg_ctx* ctx, void* forest_out, size_t out_cap, size_t* size_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (ctx->trained_model.empty()) { ctx->err = "no model has been trained on this context"; return RVSEG_ERR_NO_FOREST; }
    return hand_out(ctx, forest_out, out_cap, size_out);
}

rvseg_status rvseg_forest_train(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, const int32_t* labels, int32_t n_layers,
                                const int32_t* class_counts, const rvseg_train_params* tp_in, void* forest_out, size_t out_cap,
                                size_t* size_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    return train_matrix(ctx, X, P, D, labels, n_layers, class_counts, tp_in, kNoPrior, forest_out, out_cap, size_out);
}

rvseg_status rvseg_forest_train_prior(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, const int32_t* labels, int32_t C,
                                      const rvseg_train_params* tp_in, const rvseg_class_prior* prior_in, void* forest_out, size_t out_cap,
                                      size_t* size_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    rvseg_class_prior prior;
    const rvseg_status st = resolve_prior(ctx, prior_in, C, prior);
    if (st != RVSEG_OK) return st;
    return train_matrix(ctx, X, P, D, labels, 1, &C, tp_in, prior, forest_out, out_cap, size_out);
}

rvseg_status rvseg_forest_train_frames(rvseg_ctx* ctx, int32_t n_frames, const uint8_t* rgb, const uint16_t* depth_mm, const float* calib,
                                       const int8_t* labels, int32_t n_layers, const int32_t* class_counts, int32_t augment,
                                       const rvseg_train_params* tp_in, void* forest_out, size_t out_cap, size_t* size_out,
                                       int32_t* n_examples_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    const rvseg_train_params tp = resolve_params(tp_in);
    if (!rgb || !depth_mm || !calib || !labels || !size_out || n_frames < 1) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    rvseg_status st = pipeline_init(ctx);
    if (st != RVSEG_OK) return st;
    Pipeline* im = ctx->impl;
    const FrameGeom& g = im->geom;
    if ((st = check_train_args(ctx, n_layers, class_counts, tp, g.D)) != RVSEG_OK) return st;
    const size_t npix = (size_t)g.W * g.H;
    const int Pg = g.lw * g.lh;
    const int n_var = augment ? 6 : 1;
    const size_t cap = (size_t)n_frames * n_var * Pg;
    if (cap >= (1ull << 31)) { ctx->err = "too many training points"; return RVSEG_ERR_CAPACITY; }
    TrainSet T;
    T.D = g.D; T.L = n_layers; T.stride = cap;
    T.class_counts.assign(class_counts, class_counts + n_layers);
    T.nb_index.assign(g.D, -1);
    for (int f = g.n_patch; f < g.D; f++) T.nb_index[f] = T.n_nb++;   // depth, height, normal: floats; the patch: Lab bytes
    FrameStage fs;
    fs.scan_bytes = train_scan_temp_bytes((size_t)Pg);
    if ((st = reserve_train_set(ctx, T)) != RVSEG_OK || (st = dev_alloc(ctx, fs.labels, (size_t)n_layers * npix)) != RVSEG_OK ||
        (st = dev_alloc(ctx, fs.flags, (size_t)Pg * 4)) != RVSEG_OK || (st = dev_alloc(ctx, fs.offs, ((size_t)Pg + 1) * 4)) != RVSEG_OK ||
        (st = dev_alloc(ctx, fs.scan_temp, fs.scan_bytes)) != RVSEG_OK || (st = dev_reserve(ctx, im->in_rgb, npix * 3)) != RVSEG_OK ||
        (st = dev_reserve(ctx, im->in_depth, npix * 2)) != RVSEG_OK)
        return st;
    fs.h_rgb.resize(npix * 3);
    fs.h_depth.resize(npix);
    fs.h_lab.resize((size_t)n_layers * npix);
    size_t base = 0;
    static const int offsets[3] = {-20, 0, 20};   // train.cpp:115-117
    for (int fr = 0; fr < n_frames; fr++)
        for (int var = 0; var < n_var; var++) {
            // the reference's order: for a in (-20, 0, +20): the frame, then its horizontal flip (train.cpp:119-147)
            augment_variant(g, n_layers, rgb + (size_t)fr * npix * 3, depth_mm + (size_t)fr * npix, labels + (size_t)fr * n_layers * npix,
                            augment ? offsets[var / 2] : 0, augment && (var & 1), fs.h_rgb.data(), fs.h_depth.data(), fs.h_lab.data());
            if ((st = append_variant(ctx, im, fs, calib + (size_t)fr * 21, T, &base)) != RVSEG_OK) return st;
        }
    if (n_examples_out) *n_examples_out = (int32_t)base;
    if (base == 0) { ctx->err = "no labelled point with valid depth in the training frames"; return RVSEG_ERR_INVALID_ARG; }
    T.P = (int)base;
    if ((st = check_device_labels(ctx, T)) != RVSEG_OK) return st;
    return finish_training(ctx, T, tp, kNoPrior, forest_out, out_cap, size_out);
}

rvseg_status rvseg_boosted_train(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, const int32_t* labels, int32_t C,
                                 const rvseg_train_params* tp_in, void* out, size_t out_cap, size_t* size_out, float* errors_out,
                                 float* alphas_out, int32_t* rounds_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    return boosted_matrix(ctx, X, P, D, labels, C, tp_in, kNoPrior, out, out_cap, size_out, errors_out, alphas_out, rounds_out);
}

rvseg_status rvseg_boosted_train_prior(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, const int32_t* labels, int32_t C,
                                       const rvseg_train_params* tp_in, const rvseg_class_prior* prior_in, void* out, size_t out_cap,
                                       size_t* size_out, float* errors_out, float* alphas_out, int32_t* rounds_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    rvseg_class_prior prior;
    const rvseg_status st = resolve_prior(ctx, prior_in, C, prior);
    if (st != RVSEG_OK) return st;
    return boosted_matrix(ctx, X, P, D, labels, C, tp_in, prior, out, out_cap, size_out, errors_out, alphas_out, rounds_out);
}

rvseg_status rvseg_boosted_resample(rvseg_ctx* ctx, const float* weights, const uint8_t* miss, int32_t N, float exp_alpha, uint64_t key,
                                    float* error_out, float* weights_out, float* cumsum_out, int32_t* idx_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (!weights || N < 1) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    for (int32_t n = 0; n < N; n++)
        if (!(weights[n] >= 0.0f) || std::signbit(weights[n])) { ctx->err = "example weights must be >= +0"; return RVSEG_ERR_INVALID_ARG; }
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    hipStream_t s = ctx->stream;
    BoostScratch b;
    rvseg_status st;
    if ((st = reserve_boost(ctx, b, (size_t)N)) != RVSEG_OK) return st;
    RV_HIP(ctx, hipMemcpyAsync(b.w.p, weights, (size_t)N * 4, hipMemcpyHostToDevice, s));
    if (miss) RV_HIP(ctx, hipMemcpyAsync(b.miss.p, miss, (size_t)N, hipMemcpyHostToDevice, s));
    else RV_HIP(ctx, hipMemsetAsync(b.miss.p, 0, (size_t)N, s));
    float error = 0.f, total = 0.f;
    if ((st = boost_error(ctx, b, N, &error, s)) != RVSEG_OK || (st = boost_total(ctx, b, N, exp_alpha, &total, s)) != RVSEG_OK) return st;
    if (error_out) *error_out = error;
    if (!boost_total_ok(total)) { ctx->err = "the example weights do not sum to a positive finite total"; return RVSEG_ERR_INVALID_ARG; }
    launch_train_boost_update_cumsum(b.w.as<float>(), N, b.sums.as<float>() + 1, b.cumsum.as<float>(), s);
    launch_train_boost_resample(b.cumsum.as<float>(), N, key, b.idx.as<int>(), nullptr, s);
    if (weights_out) RV_HIP(ctx, hipMemcpyAsync(weights_out, b.w.p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
    if (cumsum_out) RV_HIP(ctx, hipMemcpyAsync(cumsum_out, b.cumsum.p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
    if (idx_out) RV_HIP(ctx, hipMemcpyAsync(idx_out, b.idx.p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

}  // extern "C"
