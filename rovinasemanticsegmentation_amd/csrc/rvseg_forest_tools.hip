// The loaded forest on a host matrix of points: its posterior sums, libforest's tools.h and its learner's leaf re-estimation.
//   classLogPosterior / multiClassLogPosterior  classifier.cpp:166-208          rvseg_forest_eval
//   Classifier::classify(DataStorage)           classifier.cpp:29-51, 53-62     rvseg_forest_classify
//   DecisionTree::classify per tree             tools.cpp:214-218               rvseg_forest_classify_trees
//   AccuracyTool / ConfusionMatrixTool /
//   CorrelationTool ::measure                   tools.cpp:61-78, 95-138, 192-231 rvseg_forest_measure + rvseg_forest_tools_*
//   updateHistograms / updateMultiHistograms    learning.cpp:918-1012           rvseg_forest_refit
//
// X is processed in chunks of TOOLS_CHUNK points (forest_tools_host.h, for_each_chunk): a chunk is uploaded, walked once
// (forest_eval_kernel: the sums; tools_votes_kernel: leaf rows, per-tree votes, forest labels) and counted (agreement,
// confusion, leaf counts); the integer counters stay on the device over all chunks and are read back once.  The float
// arithmetic on the counts is the reference's own and runs on the host (forest_tools_host.h).
//
// Pinned to the reference: the label rule (vote_label, forest_model.h) and with it every tree's vote and the forest's
// label; the three score formulas.  Build-owned: the chunking, the layout of counts_out, the `layer` argument on a
// multi-layer context (the reference's tools see the single-label head only) and the refusal of labels out of range,
// where the reference indexes out of bounds.
#include <algorithm>
#include <cstring>
#include <vector>

#include "forest_model.h"
#include "forest_tools_host.h"
#include "rvseg_internal.h"
#include "rvseg_kernels.h"

namespace rvseg {

// what every tools call checks first; the order of the refusals is the header's
rvseg_status check_points(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D) {
    if (!ctx->forest_loaded) { ctx->err = "no forest loaded"; return RVSEG_ERR_NO_FOREST; }
    if (P <= 0 || !X) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    if (D != ctx->feature_length) { ctx->err = "D does not match the configured feature length"; return RVSEG_ERR_INVALID_ARG; }
    return RVSEG_OK;
}

rvseg_status layer_of(rvseg_ctx* ctx, int32_t layer, LayerView& v) {
    const DeviceForest& f = ctx->forest;
    if (layer < 0 || layer >= f.n_layers) { ctx->err = "layer outside the layers of the context's active mode"; return RVSEG_ERR_INVALID_ARG; }
    v.off = 0;
    for (int l = 0; l < layer; l++) v.off += f.class_counts[l];
    v.C = f.class_counts[layer];
    return RVSEG_OK;
}

int count_blocks(rvseg_ctx* ctx) {   // grids that loop: a few blocks per compute unit
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->params.device) != hipSuccess || cus < 1) cus = 64;
    return cus * 4;
}

rvseg_status for_each_chunk(rvseg_ctx* ctx, const float* X, int P, int D, const std::function<rvseg_status(int base, int n)>& body) {
    hipStream_t s = ctx->stream;
    rvseg_status st;
    if ((st = dev_reserve(ctx, ctx->tools.X, (size_t)std::min(P, TOOLS_CHUNK) * D * sizeof(float))) != RVSEG_OK) return st;
    for (int base = 0; base < P; base += TOOLS_CHUNK) {
        const int n = std::min(TOOLS_CHUNK, P - base);
        RV_HIP(ctx, hipMemcpyAsync(ctx->tools.X.p, X + (size_t)base * D, (size_t)n * D * sizeof(float), hipMemcpyHostToDevice, s));
        if ((st = body(base, n)) != RVSEG_OK) return st;
        // the chunk's scratch is written again by the next chunk's upload, which a host-staged copy may start early
        RV_HIP(ctx, hipStreamSynchronize(s));
        RV_LAUNCH_OK(ctx);
    }
    return RVSEG_OK;
}

// DecisionTree::classLogPosterior + classify per leaf, from the model's own histograms as the stream holds them (for a
// boosted model the device rows hold the weighted votes, where a non-positive weight hides the label)
rvseg_status upload_vote_table(rvseg_ctx* ctx, int layer, hipStream_t s) {
    const ForestModel& m = ctx->host_forest;
    const bool multi = ctx->params.multi_layer != 0;
    std::vector<uint8_t> table;
    table.reserve((size_t)m.n_leaves);
    for (const RawTree& tree : m.raw)
        for (int32_t node : leaf_nodes_in_row_order(tree)) {
            const std::vector<float>& h = multi ? tree.mhist[(size_t)node][(size_t)layer] : tree.hist[(size_t)node];
            table.push_back((uint8_t)vote_label(h.data(), (int)h.size()));
        }
    rvseg_status st;
    if ((st = dev_reserve(ctx, ctx->tools.vote_table, table.size())) != RVSEG_OK) return st;
    RV_HIP(ctx, hipMemcpyAsync(ctx->tools.vote_table.p, table.data(), table.size(), hipMemcpyHostToDevice, s));
    RV_HIP(ctx, hipStreamSynchronize(s));   // `table` goes out of scope
    return RVSEG_OK;
}

namespace {

// what a pass over X produces; null = not wanted.  Host pointers.
struct ToolsOut {
    int32_t* pred = nullptr;          // [P]
    uint8_t* votes = nullptr;         // [T][P]
    uint64_t* confusion = nullptr;    // [C][C]
    uint64_t* agree = nullptr;        // [T][T]
};

// One pass over X in chunks.  With `labels` (and out.confusion) a label outside [0, C) refuses the call: then nothing of
// `out` has been written.
rvseg_status tools_pass(rvseg_ctx* ctx, const float* X, int P, int D, int layer, const LayerView& lv, const int32_t* labels, const ToolsOut& out) {
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    hipStream_t s = ctx->stream;
    ToolsScratch& sc = ctx->tools;
    const DeviceForest& f = ctx->forest;
    const int T = f.n_trees, C = lv.C;
    const bool want_votes = out.votes || out.agree, want_conf = out.confusion != nullptr, want_pred = out.pred || want_conf;
    const int chunk = std::min(P, TOOLS_CHUNK), stride = (chunk + 3) & ~3;
    const int blocks = count_blocks(ctx);
    rvseg_status st;
    if ((st = dev_reserve(ctx, sc.flag, 16)) != RVSEG_OK) return st;
    if (want_votes && ((st = dev_reserve(ctx, sc.votes, (size_t)T * stride)) != RVSEG_OK || (st = upload_vote_table(ctx, layer, s)) != RVSEG_OK)) return st;
    if (want_pred && (st = dev_reserve(ctx, sc.pred, (size_t)chunk * 4)) != RVSEG_OK) return st;
    if (out.agree && (st = dev_reserve(ctx, sc.agree, (size_t)T * T * 8)) != RVSEG_OK) return st;
    if (want_conf && ((st = dev_reserve(ctx, sc.confusion, (size_t)C * C * 8)) != RVSEG_OK || (st = dev_reserve(ctx, sc.labels, (size_t)chunk * 4)) != RVSEG_OK)) return st;
    RV_HIP(ctx, hipMemsetAsync(sc.flag.p, 0, 16, s));
    if (out.agree) RV_HIP(ctx, hipMemsetAsync(sc.agree.p, 0, (size_t)T * T * 8, s));
    if (want_conf) RV_HIP(ctx, hipMemsetAsync(sc.confusion.p, 0, (size_t)C * C * 8, s));
    // a call that can still be refused keeps its labels back until the flag is known
    std::vector<int32_t> pred_kept;
    int32_t* pred_host = out.pred;
    if (want_conf && out.pred) { pred_kept.resize((size_t)P); pred_host = pred_kept.data(); }
    if ((st = for_each_chunk(ctx, X, P, D, [&](int base, int n) -> rvseg_status {
        launch_tools_votes(f, sc.vote_table.as<uint8_t>(), lv.off, C, sc.X.as<float>(), n, D, stride, nullptr,
                           want_votes ? sc.votes.as<uint8_t>() : nullptr, want_pred ? sc.pred.as<int32_t>() : nullptr, s);
        if (out.agree) launch_tools_agree(sc.votes.as<uint8_t>(), T, n, stride, blocks, sc.agree.as<unsigned long long>(), s);
        if (want_conf) {
            RV_HIP(ctx, hipMemcpyAsync(sc.labels.p, labels + base, (size_t)n * 4, hipMemcpyHostToDevice, s));
            launch_tools_confusion(sc.labels.as<int32_t>(), sc.pred.as<int32_t>(), n, C, blocks, sc.confusion.as<unsigned long long>(), sc.flag.as<int>(), s);
        }
        if (out.votes) RV_HIP(ctx, hipMemcpy2DAsync(out.votes + base, (size_t)P, sc.votes.p, (size_t)stride, (size_t)n, (size_t)T, hipMemcpyDeviceToHost, s));
        if (pred_host) RV_HIP(ctx, hipMemcpyAsync(pred_host + base, sc.pred.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        return RVSEG_OK;
    })) != RVSEG_OK) return st;
    int flag = 0;
    std::vector<uint64_t> conf((size_t)(want_conf ? C * C : 0));
    RV_HIP(ctx, hipMemcpyAsync(&flag, sc.flag.p, 4, hipMemcpyDeviceToHost, s));
    if (want_conf) RV_HIP(ctx, hipMemcpyAsync(conf.data(), sc.confusion.p, conf.size() * 8, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    if (flag) { ctx->err = "label outside the layer's class range"; return RVSEG_ERR_INVALID_ARG; }
    if (out.agree) {
        RV_HIP(ctx, hipMemcpyAsync(out.agree, sc.agree.p, (size_t)T * T * 8, hipMemcpyDeviceToHost, s));
        RV_HIP(ctx, hipStreamSynchronize(s));
    }
    if (want_conf) std::memcpy(out.confusion, conf.data(), conf.size() * 8);
    if (!pred_kept.empty()) std::memcpy(out.pred, pred_kept.data(), pred_kept.size() * 4);
    return RVSEG_OK;
}

// the leaf counts of (X, labels): counts[leaf row][sumC]; a label out of range refuses
rvseg_status refit_counts(rvseg_ctx* ctx, const float* X, int P, int D, const int32_t* labels, const RefitLayers& lay, std::vector<uint32_t>& counts) {
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    hipStream_t s = ctx->stream;
    ToolsScratch& sc = ctx->tools;
    const DeviceForest& f = ctx->forest;
    const int T = f.n_trees, L = lay.n_layers;
    const int chunk = std::min(P, TOOLS_CHUNK), stride = (chunk + 3) & ~3;
    const int blocks = count_blocks(ctx);
    counts.assign((size_t)f.n_leaves * lay.sum_classes, 0u);
    rvseg_status st;
    if ((st = dev_reserve(ctx, sc.flag, 16)) != RVSEG_OK || (st = dev_reserve(ctx, sc.rows, (size_t)T * stride * 4)) != RVSEG_OK ||
        (st = dev_reserve(ctx, sc.labels, (size_t)chunk * L * 4)) != RVSEG_OK || (st = dev_reserve(ctx, sc.leaf_cnt, counts.size() * 4)) != RVSEG_OK)
        return st;
    RV_HIP(ctx, hipMemsetAsync(sc.flag.p, 0, 16, s));
    RV_HIP(ctx, hipMemsetAsync(sc.leaf_cnt.p, 0, counts.size() * 4, s));
    if ((st = for_each_chunk(ctx, X, P, D, [&](int base, int n) -> rvseg_status {
        RV_HIP(ctx, hipMemcpyAsync(sc.labels.p, labels + (size_t)base * L, (size_t)n * L * 4, hipMemcpyHostToDevice, s));
        launch_tools_votes(f, nullptr, 0, 0, sc.X.as<float>(), n, D, stride, sc.rows.as<int32_t>(), nullptr, nullptr, s);
        launch_tools_refit_count(sc.rows.as<int32_t>(), sc.labels.as<int32_t>(), T, n, stride, lay, blocks, sc.leaf_cnt.as<uint32_t>(), sc.flag.as<int>(), s);
        return RVSEG_OK;
    })) != RVSEG_OK) return st;
    int flag = 0;
    RV_HIP(ctx, hipMemcpyAsync(&flag, sc.flag.p, 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipMemcpyAsync(counts.data(), sc.leaf_cnt.p, counts.size() * 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    if (flag) { ctx->err = "label outside its layer's class range"; return RVSEG_ERR_INVALID_ARG; }
    return RVSEG_OK;
}

}  // namespace
}  // namespace rvseg

using namespace rvseg;

extern "C" {

rvseg_status rvseg_forest_eval(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, float* out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (!ctx->forest_loaded) { ctx->err = "no forest loaded"; return RVSEG_ERR_NO_FOREST; }
    if (P < 0 || !out || (!X && P > 0)) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    if (D != ctx->feature_length) { ctx->err = "D does not match the configured feature length"; return RVSEG_ERR_INVALID_ARG; }
    if (P == 0) return RVSEG_OK;
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    DevBuf& sums = ctx->tools.sums;
    const size_t S = (size_t)ctx->forest.sum_classes;
    rvseg_status st;
    if ((st = dev_reserve(ctx, sums, (size_t)std::min(P, TOOLS_CHUNK) * S * sizeof(float))) != RVSEG_OK) return st;
    return for_each_chunk(ctx, X, P, D, [&](int base, int n) -> rvseg_status {
        launch_forest_eval(ctx->forest, ctx->tools.X.as<float>(), n, D, sums.as<float>(), ctx->stream);
        RV_HIP(ctx, hipMemcpyAsync(out + (size_t)base * S, sums.p, (size_t)n * S * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        return RVSEG_OK;
    });
}

rvseg_status rvseg_forest_classify(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, int32_t layer, int32_t* labels_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    rvseg_status st;
    LayerView lv;
    if ((st = check_points(ctx, X, P, D)) != RVSEG_OK || (st = layer_of(ctx, layer, lv)) != RVSEG_OK) return st;
    if (!labels_out) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    ToolsOut out;
    out.pred = labels_out;
    return tools_pass(ctx, X, P, D, layer, lv, nullptr, out);
}

rvseg_status rvseg_forest_classify_trees(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, int32_t layer, uint8_t* votes_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    rvseg_status st;
    LayerView lv;
    if ((st = check_points(ctx, X, P, D)) != RVSEG_OK || (st = layer_of(ctx, layer, lv)) != RVSEG_OK) return st;
    if (!votes_out) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    ToolsOut out;
    out.votes = votes_out;
    return tools_pass(ctx, X, P, D, layer, lv, nullptr, out);
}

rvseg_status rvseg_forest_measure(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, const int32_t* labels, int32_t layer, int32_t* pred_out,
                                  uint64_t* confusion_out, uint64_t* agree_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    rvseg_status st;
    LayerView lv;
    if ((st = check_points(ctx, X, P, D)) != RVSEG_OK || (st = layer_of(ctx, layer, lv)) != RVSEG_OK) return st;
    if (confusion_out && !labels) { ctx->err = "the confusion counts need labels"; return RVSEG_ERR_INVALID_ARG; }
    if (!pred_out && !confusion_out && !agree_out) return RVSEG_OK;
    ToolsOut out;
    out.pred = pred_out;
    out.confusion = confusion_out;
    out.agree = agree_out;
    return tools_pass(ctx, X, P, D, layer, lv, confusion_out ? labels : nullptr, out);
}

rvseg_status rvseg_forest_tools_scores(const uint64_t* confusion, int32_t C, float* accuracy_out, float* confusion_norm_out) {
    if (!confusion || C < 1) return RVSEG_ERR_INVALID_ARG;
    if (accuracy_out) *accuracy_out = tools_accuracy(confusion, C);
    if (confusion_norm_out) tools_confusion_normalised(confusion, C, confusion_norm_out);
    return RVSEG_OK;
}

rvseg_status rvseg_forest_tools_correlation(const uint64_t* agree, int32_t T, uint64_t P, float* corr_out) {
    if (!agree || !corr_out || T < 1 || P < 1) return RVSEG_ERR_INVALID_ARG;
    tools_correlation(agree, T, P, corr_out);
    return RVSEG_OK;
}

rvseg_status rvseg_forest_refit(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, const int32_t* labels, int32_t n_layers,
                                const int32_t* class_counts, float smoothing, void* forest_out, size_t out_cap, size_t* size_out,
                                uint32_t* counts_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (ctx->forest_loaded && ctx->host_forest.boosted) {
        ctx->err = "the context holds a boosted forest: its leaves are not re-estimated (the learner weighs them per round)";
        return RVSEG_ERR_NO_FOREST;
    }
    rvseg_status st;
    if ((st = check_points(ctx, X, P, D)) != RVSEG_OK) return st;
    if (!labels || !class_counts || n_layers < 1 || n_layers > RVSEG_MAX_LAYERS || !(smoothing >= 0.f)) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    const ForestModel& m = ctx->host_forest;
    if (!refit_heads_match(m, n_layers, class_counts, ctx->err)) return RVSEG_ERR_INVALID_ARG;
    if (!forest_out && !counts_out) {   // size query: the refit changes no vector's length
        if (size_out) *size_out = serialize_forest(m).size();
        return RVSEG_OK;
    }
    RefitLayers lay{};
    lay.n_layers = n_layers;
    for (int l = 0; l < n_layers; l++) {
        lay.class_counts[l] = class_counts[l];
        lay.offset[l] = lay.sum_classes;
        lay.sum_classes += class_counts[l];
    }
    std::vector<uint32_t> counts;
    if ((st = refit_counts(ctx, X, P, D, labels, lay, counts)) != RVSEG_OK) return st;
    // the inverted class frequencies of this set (data.h:358-370); every label is in range
    std::vector<std::vector<uint64_t>> class_cnt((size_t)n_layers);
    for (int l = 0; l < n_layers; l++) {
        class_cnt[(size_t)l].assign((size_t)class_counts[l], 0);
        for (int i = 0; i < P; i++) class_cnt[(size_t)l][(size_t)labels[(size_t)i * n_layers + l]]++;
    }
    const std::vector<uint8_t> bytes = serialize_forest(refit_model(m, counts.data(), class_cnt, P, smoothing));
    if (forest_out && out_cap < bytes.size()) {
        if (size_out) *size_out = bytes.size();
        ctx->err = "output buffer too small";
        return RVSEG_ERR_INVALID_ARG;
    }
    if (size_out) *size_out = bytes.size();
    if (forest_out) std::memcpy(forest_out, bytes.data(), bytes.size());
    if (counts_out) refit_counts_by_node(m, counts.data(), lay.sum_classes, counts_out);
    return RVSEG_OK;
}

}  // extern "C"
