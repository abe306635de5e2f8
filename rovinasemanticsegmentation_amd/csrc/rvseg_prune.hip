// Forest pruning on the GPU: libforest's RandomForestPrune::prune (todos.txt:310-350) and the simulated-annealing driver
// it is written against (mcmc.h:147-240), for the loaded RandomForest.
//   PruneEnergy::energy (majority-vote error)   todos.txt:186-226   the chain on the device, one launch per proposal
//   the second PruneEnergy (cover by distance)  todos.txt:245-297   the chain on the host over the T x T agree counts
//   newForest->addTree(forest->getTree(..))     todos.txt:344-348   rvseg_forest_prune_apply
//
// Error energy: the per-tree votes of all P points are made once by the forest tools' walk (launch_tools_votes, a chunk
// of X at a time) into one [T][stride] byte table that stays on the device with the labels for the whole call.  The
// host fills every step's state-independent record ahead of time (prune_steps, prune_host.h: move, draws, temperature,
// logf of the acceptance uniform) and then issues the launches back to back; it waits once, at the end, and reads back
// the best state, its energy, the trace and the step kinds.
//
// Pinned to the reference: the chain, the moves, both energies (prune_host.h).  Build-owned: the draws, the cap of 64
// entries on a state, the refusals, the `layer` argument as for the forest tools.
#include <cstring>
#include <vector>

#include "forest_model.h"
#include "forest_tools_host.h"
#include "prune_host.h"
#include "rvseg_internal.h"
#include "rvseg_kernels.h"

namespace rvseg {
namespace {

// what both entry points check before anything runs; the order of the refusals is the header's
rvseg_status check_prune_call(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, const int32_t* labels, int32_t layer, int32_t energy,
                              const int32_t* state, int32_t n_state, LayerView& lv) {
    if (!ctx->forest_loaded) { ctx->err = "no forest loaded"; return RVSEG_ERR_NO_FOREST; }
    if (ctx->host_forest.boosted) { ctx->err = "the context holds a boosted forest: RandomForestPrune prunes a RandomForest"; return RVSEG_ERR_INVALID_ARG; }
    rvseg_status st;
    if ((st = check_points(ctx, X, P, D)) != RVSEG_OK || (st = layer_of(ctx, layer, lv)) != RVSEG_OK) return st;
    if (energy != RVSEG_PRUNE_ERROR && energy != RVSEG_PRUNE_COVER) { ctx->err = "unknown energy"; return RVSEG_ERR_INVALID_ARG; }
    if (energy == RVSEG_PRUNE_ERROR && !labels) { ctx->err = "the error energy needs labels"; return RVSEG_ERR_INVALID_ARG; }
    if (energy == RVSEG_PRUNE_ERROR && P > 0x7ffffffc) { ctx->err = "too many points: a vote row padded to four must fit an int"; return RVSEG_ERR_INVALID_ARG; }
    if (energy == RVSEG_PRUNE_ERROR && lv.C > PRUNE_CMAX) { ctx->err = "the error energy handles at most 16 classes"; return RVSEG_ERR_INVALID_ARG; }
    if (const char* why = prune_state_refusal(state, n_state, ctx->forest.n_trees)) { ctx->err = why; return RVSEG_ERR_INVALID_ARG; }
    return RVSEG_OK;
}

// every tree's vote on every point -> ctx->prune.votes [T][stride], the labels -> ctx->prune.labels [stride]
rvseg_status votes_resident(rvseg_ctx* ctx, const float* X, int P, int D, const int32_t* labels, int layer, const LayerView& lv, size_t stride) {
    hipStream_t s = ctx->stream;
    ToolsScratch& sc = ctx->tools;
    PruneScratch& pr = ctx->prune;
    const DeviceForest& f = ctx->forest;
    rvseg_status st;
    if ((st = upload_vote_table(ctx, layer, s)) != RVSEG_OK || (st = dev_reserve(ctx, pr.votes, (size_t)f.n_trees * stride)) != RVSEG_OK ||
        (st = dev_reserve(ctx, pr.labels, stride * 4)) != RVSEG_OK)
        return st;
    RV_HIP(ctx, hipMemsetAsync(pr.votes.p, 0, (size_t)f.n_trees * stride, s));   // the rows' tails beyond P are read, four bytes at a time
    RV_HIP(ctx, hipMemsetAsync(pr.labels.p, 0, stride * 4, s));
    RV_HIP(ctx, hipMemcpyAsync(pr.labels.p, labels, (size_t)P * 4, hipMemcpyHostToDevice, s));
    return for_each_chunk(ctx, X, P, D, [&](int base, int n) -> rvseg_status {   // (TOOLS_CHUNK is a multiple of 4: every chunk's rows stay word-aligned)
        launch_tools_votes(f, sc.vote_table.as<uint8_t>(), lv.off, lv.C, sc.X.as<float>(), n, D, stride, nullptr, pr.votes.as<uint8_t>() + base, nullptr, s);
        return RVSEG_OK;
    });
}

// puts `state` into PruneControl::state[0] and runs the init launch: its energy becomes the current and the best one
rvseg_status chain_start(rvseg_ctx* ctx, int P, size_t stride, int grid, const int32_t* state, int n_state) {
    hipStream_t s = ctx->stream;
    PruneScratch& pr = ctx->prune;
    rvseg_status st;
    if ((st = dev_reserve(ctx, pr.control, sizeof(PruneControl))) != RVSEG_OK) return st;
    PruneControl start;
    std::memset(&start, 0, sizeof(start));
    start.n_state[0] = n_state;
    std::memcpy(start.state[0], state, (size_t)n_state * 4);
    RV_HIP(ctx, hipMemcpyAsync(pr.control.p, &start, sizeof(start), hipMemcpyHostToDevice, s));
    RV_HIP(ctx, hipStreamSynchronize(s));   // `start` goes out of scope
    launch_prune_init(pr.votes.as<uint8_t>(), pr.labels.as<int32_t>(), P, stride, grid, pr.control.as<PruneControl>(), s);
    return RVSEG_OK;
}

struct PruneOut {   // host pointers, as rvseg_forest_prune takes them
    int32_t* state;
    int32_t* n_state;
    float* best_energy;
    rvseg_prune_trace_row* trace;
    int32_t trace_cap;
    int32_t* n_trace;
    uint8_t* step_kind;
};

void write_out(const PruneOut& out, const int32_t* best, int n_best, float best_energy, const rvseg_prune_trace_row* trace, int iterations,
               const uint8_t* step_kind, size_t n_steps) {
    std::memcpy(out.state, best, (size_t)n_best * 4);
    *out.n_state = n_best;
    if (out.best_energy) *out.best_energy = best_energy;
    if (out.trace && out.trace_cap > 0 && iterations > 0) std::memcpy(out.trace, trace, (size_t)std::min(out.trace_cap, iterations) * sizeof(rvseg_prune_trace_row));
    if (out.n_trace) *out.n_trace = iterations;
    if (out.step_kind && n_steps) std::memcpy(out.step_kind, step_kind, n_steps);
}

rvseg_status prune_error_chain(rvseg_ctx* ctx, const float* X, int P, int D, const int32_t* labels, int layer, const LayerView& lv,
                               const rvseg_prune_params& pp, const PruneOut& out) {
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    hipStream_t s = ctx->stream;
    PruneScratch& pr = ctx->prune;
    const size_t stride = ((size_t)P + 3) & ~(size_t)3;
    const int grid = prune_grid(P, count_blocks(ctx));
    const int iterations = prune_iterations(pp);
    const std::vector<PruneStep> steps = prune_steps(pp, ctx->forest.n_trees);
    rvseg_status st;
    if ((st = votes_resident(ctx, X, P, D, labels, layer, lv, stride)) != RVSEG_OK) return st;
    if ((st = dev_reserve(ctx, pr.steps, std::max<size_t>(steps.size(), 1) * sizeof(PruneStep))) != RVSEG_OK ||
        (st = dev_reserve(ctx, pr.step_kind, std::max<size_t>(steps.size(), 1))) != RVSEG_OK ||
        (st = dev_reserve(ctx, pr.trace, std::max<size_t>((size_t)iterations, 1) * sizeof(rvseg_prune_trace_row))) != RVSEG_OK)
        return st;
    if (!steps.empty()) RV_HIP(ctx, hipMemcpyAsync(pr.steps.p, steps.data(), steps.size() * sizeof(PruneStep), hipMemcpyHostToDevice, s));
    if ((st = chain_start(ctx, P, stride, grid, out.state, *out.n_state)) != RVSEG_OK) return st;
    launch_prune_steps(pr.votes.as<uint8_t>(), pr.labels.as<int32_t>(), P, stride, grid, pr.steps.as<PruneStep>(), 0, (int)steps.size(),
                       pr.control.as<PruneControl>(), pr.step_kind.as<uint8_t>(), pr.trace.as<rvseg_prune_trace_row>(), s);
    PruneControl end;
    std::vector<rvseg_prune_trace_row> trace((size_t)iterations);
    std::vector<uint8_t> kinds(steps.size());
    RV_HIP(ctx, hipMemcpyAsync(&end, pr.control.p, sizeof(end), hipMemcpyDeviceToHost, s));
    if (iterations) RV_HIP(ctx, hipMemcpyAsync(trace.data(), pr.trace.p, trace.size() * sizeof(rvseg_prune_trace_row), hipMemcpyDeviceToHost, s));
    if (!kinds.empty()) RV_HIP(ctx, hipMemcpyAsync(kinds.data(), pr.step_kind.p, kinds.size(), hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    RV_LAUNCH_OK(ctx);
    write_out(out, end.best, end.n_best, end.best_energy, trace.data(), iterations, kinds.data(), kinds.size());
    return RVSEG_OK;
}

}  // namespace
}  // namespace rvseg

using namespace rvseg;

extern "C" {

void rvseg_prune_params_default(rvseg_prune_params* pp) {
    if (!pp) return;
    std::memset(pp, 0, sizeof(*pp));
    pp->start_temperature = 100.f;   // todos.txt:319
    pp->end_temperature = 1e-5f;     // todos.txt:320
    pp->alpha = 0.95f;               // todos.txt:318
    pp->inner_loops = 250;           // todos.txt:314
    pp->p_exchange = 1.f;            // todos.txt:324-325: the exchange move alone
    pp->energy = RVSEG_PRUNE_ERROR;  // todos.txt:328
}

rvseg_status rvseg_prune_schedule(const rvseg_prune_params* pp, int32_t* iterations_out, int32_t* steps_out) {
    if (!pp || prune_params_refusal(*pp)) return RVSEG_ERR_INVALID_ARG;
    const int iterations = prune_iterations(*pp);
    if (iterations_out) *iterations_out = iterations;
    if (steps_out) *steps_out = iterations * pp->inner_loops;
    return RVSEG_OK;
}

rvseg_status rvseg_forest_prune(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, const int32_t* labels, int32_t layer,
                                const rvseg_prune_params* pp, int32_t* state_inout, int32_t* n_state_inout, float* best_energy_out,
                                rvseg_prune_trace_row* trace_out, int32_t trace_cap, int32_t* n_trace_out, uint8_t* step_kind_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (!pp || !state_inout || !n_state_inout) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    rvseg_status st;
    LayerView lv;
    if ((st = check_prune_call(ctx, X, P, D, labels, layer, pp->energy, state_inout, *n_state_inout, lv)) != RVSEG_OK) return st;
    if (const char* why = prune_params_refusal(*pp)) { ctx->err = why; return RVSEG_ERR_INVALID_ARG; }
    const PruneOut out{state_inout, n_state_inout, best_energy_out, trace_out, trace_cap, n_trace_out, step_kind_out};
    if (pp->energy == RVSEG_PRUNE_ERROR) return prune_error_chain(ctx, X, P, D, labels, layer, lv, *pp, out);
    const int T = ctx->forest.n_trees;
    std::vector<uint64_t> agree((size_t)T * T);
    if ((st = rvseg_forest_measure(ctx, X, P, D, nullptr, layer, nullptr, nullptr, agree.data())) != RVSEG_OK) return st;
    const PruneRun run = prune_chain(*pp, T, state_inout, *n_state_inout,
                                     [&](const int32_t* state, int n) { return prune_cover_energy(agree.data(), T, (uint64_t)P, state, n); });
    write_out(out, run.best.data(), (int)run.best.size(), run.best_energy, run.trace.data(), (int)run.trace.size(), run.step_kind.data(), run.step_kind.size());
    return RVSEG_OK;
}

rvseg_status rvseg_forest_prune_energy(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D, const int32_t* labels, int32_t layer,
                                       int32_t energy, const int32_t* state, int32_t n_state, float* energy_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (!energy_out) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    rvseg_status st;
    LayerView lv;
    if ((st = check_prune_call(ctx, X, P, D, labels, layer, energy, state, n_state, lv)) != RVSEG_OK) return st;
    if (energy == RVSEG_PRUNE_COVER) {
        const int T = ctx->forest.n_trees;
        std::vector<uint64_t> agree((size_t)T * T);
        if ((st = rvseg_forest_measure(ctx, X, P, D, nullptr, layer, nullptr, nullptr, agree.data())) != RVSEG_OK) return st;
        *energy_out = prune_cover_energy(agree.data(), T, (uint64_t)P, state, n_state);
        return RVSEG_OK;
    }
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    const size_t stride = ((size_t)P + 3) & ~(size_t)3;
    if ((st = votes_resident(ctx, X, P, D, labels, layer, lv, stride)) != RVSEG_OK ||
        (st = chain_start(ctx, P, stride, prune_grid(P, count_blocks(ctx)), state, n_state)) != RVSEG_OK)
        return st;
    PruneControl end;
    RV_HIP(ctx, hipMemcpyAsync(&end, ctx->prune.control.p, sizeof(end), hipMemcpyDeviceToHost, ctx->stream));
    RV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RV_LAUNCH_OK(ctx);
    *energy_out = end.cur_energy;
    return RVSEG_OK;
}

rvseg_status rvseg_forest_prune_apply(rvseg_ctx* ctx, const int32_t* state, int32_t n_state) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (!ctx->forest_loaded) { ctx->err = "no forest loaded"; return RVSEG_ERR_NO_FOREST; }
    if (ctx->host_forest.boosted) { ctx->err = "the context holds a boosted forest: RandomForestPrune prunes a RandomForest"; return RVSEG_ERR_INVALID_ARG; }
    if (const char* why = prune_state_refusal(state, n_state, ctx->forest.n_trees, kMaxTrees)) { ctx->err = why; return RVSEG_ERR_INVALID_ARG; }
    ForestModel picked;   // serialize_forest reads the raw trees alone
    for (int i = 0; i < n_state; i++) picked.raw.push_back(ctx->host_forest.raw[(size_t)state[i]]);
    const std::vector<uint8_t> bytes = serialize_forest(picked);
    return rvseg_forest_load_mem(ctx, bytes.data(), bytes.size());   // the ordinary parse and upload
}

}  // extern "C"
