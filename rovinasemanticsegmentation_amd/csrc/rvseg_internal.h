// Internal declarations shared by the C-ABI translation unit and the HIP kernel files.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/rvseg.h"
#include "forest_model.h"

namespace rvseg {

// ---------------------------------------------------------------------------------------------
// The four owning handle types.  Each releases what it holds in its destructor and is move-only (declaring the moves
// deletes the copies; a move leaves the source empty), so a state struct made of them needs no teardown code: a new
// buffer is a new member.  g_live counts the handles that currently hold something, per type
// (rvseg_debug_live_resources).
// ---------------------------------------------------------------------------------------------
enum LiveKind { LIVE_DEVICE, LIVE_PINNED, LIVE_EVENT, LIVE_STREAM };
extern std::atomic<long long> g_live[4];

// device memory: dev_alloc / dev_reserve / dev_free below
struct DevBuf;
void dev_free(DevBuf& b);
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { dev_free(*this); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~DevBuf() { dev_free(*this); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// page-locked host memory, grow-only
struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~PinnedBuf() { release(); }
    rvseg_status reserve(rvseg_ctx* ctx, size_t n);   // a reallocation frees first; the contents are not kept
    void release();
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// an event / a stream: converts to the HIP handle, so it is passed to HIP calls as such.  Created by event_create /
// stream_create where it is first needed; a group that belongs together (a stream and the events that order it) is
// created into locals and moved into the state only when all of it exists.
template <class H, hipError_t (*Destroy)(H), LiveKind K>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
    Handle& operator=(Handle&& o) noexcept { if (this != &o) { release(); h = o.h; o.h = nullptr; } return *this; }
    ~Handle() { release(); }
    void release() { if (h) { (void)Destroy(h); g_live[K]--; } h = nullptr; }
    operator H() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventDestroy, LIVE_EVENT>;
using Stream = Handle<hipStream_t, hipStreamDestroy, LIVE_STREAM>;
hipError_t event_create(Event& e, unsigned flags);
hipError_t stream_create(Stream& s, unsigned flags);
hipError_t stream_create(Stream& s, unsigned flags, int priority);

// ---------------------------------------------------------------------------------------------
// Label layers of a per-pixel distribution image: what the up-sampler, the per-frame CRF and the label rules need to
// know about a provider.  The loaded forest supplies one (DeviceForest), rvseg_external_layers_set the other.
// ---------------------------------------------------------------------------------------------
struct LayerLayout {
    int n_layers = 0;                       // forest: layers of the ACTIVE mode
    int class_counts[RVSEG_MAX_LAYERS] = {}; // per layer
    int sum_classes = 0;                    // S
};

// ---------------------------------------------------------------------------------------------
// device-side forest (breadth-first node array in HBM, leaf histogram table)
// ---------------------------------------------------------------------------------------------
struct DeviceForest : LayerLayout {
    int n_trees = 0;
    int max_depth = 0;
    int n_nodes = 0;
    int n_leaves = 0;
    DevBuf nodes;                           // DeviceNode[n_nodes]
    DevBuf nodes8;                          // the same nodes in 8 bytes each (frame kernel), or empty: see upload_forest
    DevBuf roots;                           // int32[n_trees]
    DevBuf hist;                            // float[n_leaves * S] of the active mode
};

// Lab LUTs (gamma, cube root, 3x3 fixed-point matrix), uploaded once
struct LabTables {
    DevBuf gamma;   // uint16[256]
    DevBuf cbrt;    // uint16[3072]
    int coeffs[9];
};

struct StageTimer {
    std::vector<std::string> names;  // names[i] = stage that starts at events[i]
    std::vector<Event> events;       // pool; events[i] .. events[i+1] bracket stage i
    size_t used = 0;
    std::vector<float> ms;
    // one stage may run on a side stream, overlapped with the stages above (the lattice build of the
    // frame path): its own pair of events, reported under side_name
    Event side0, side1;
    std::string side_name;
    bool side_used = false;
};

// scratch of the forest tools (rvseg_forest_tools.hip), sized by a chunk of points and the loaded model; grow-only
struct ToolsScratch {
    DevBuf X, labels;               // one chunk of points and of their labels
    DevBuf sums;                    // [chunk][S] posterior sums (rvseg_forest_eval)
    DevBuf rows, votes, pred;       // [T][chunk] leaf rows and votes, [chunk] forest labels
    DevBuf vote_table;              // [n_leaves] vote label per leaf row
    DevBuf agree, confusion, flag;  // [T][T] and [C][C] 64-bit counters, the bad-label flag word
    DevBuf leaf_cnt;                // [n_leaves][sum of the refit's classes]
};

// scratch of rvseg_forest_prune (rvseg_prune.hip), sized by the whole point set and the schedule; grow-only
struct PruneScratch {
    DevBuf votes, labels;           // [T][stride] votes and [stride] labels of all P points
    DevBuf steps, control;          // [steps] PruneStep, one PruneControl
    DevBuf step_kind, trace;        // [steps] bytes, [iterations] rows
};

struct Pipeline;    // state of the frame / CRF / fusion pipelines (rvseg_pipeline.h)
struct EvalState;   // colour codings + confusion counters of the scoring calls (kernels_eval.hip)

}  // namespace rvseg

struct rvseg_ctx {
    rvseg_params params{};
    rvseg_schedule sched{};        // rvseg_set_schedule; defaults from rvseg_schedule_default
    int feature_length = 0;
    mutable std::string err;       // (a const call that refuses still says why)
    rvseg::ForestModel host_forest;
    bool forest_loaded = false;
    rvseg::DeviceForest forest;
    rvseg::LayerLayout external;   // rvseg_external_layers_set; n_layers == 0: not set.  Independent of `forest`
    rvseg::LabTables lab;
    rvseg::Stream stream;          // ctx-owned stream for the host entry points
    rvseg::StageTimer timer;
    rvseg::Pipeline* impl = nullptr;  // frame / crf / fusion state: pipeline_of (rvseg_pipeline.hip)
    std::vector<uint8_t> trained_model;   // forest.dat image of the last rvseg_forest_train* call (rvseg_forest_train_result)
    rvseg::ForestModel trained_boosted;   // trees and weights of the last rvseg_boosted_train (rvseg_boosted_train_result)
    void* comm = nullptr;  // RCCL communicator of the local-map gather (rvseg_comm.cpp), or null
    int comm_rank = 0, comm_world = 0;
    rvseg::EvalState* eval = nullptr;     // allocated by the first scoring call; discarded by rvseg_forest_load
    rvseg::ToolsScratch tools;            // rvseg_forest_classify / _measure / _refit
    rvseg::PruneScratch prune;            // rvseg_forest_prune / _prune_energy
};

namespace rvseg {

// Error plumbing: every HIP call goes through this; failures land in ctx->err.
bool hip_ok(rvseg_ctx* ctx, hipError_t e, const char* what);
#define RV_HIP(ctx, call)                                           \
    do {                                                            \
        if (!::rvseg::hip_ok((ctx), (call), #call)) return RVSEG_ERR_HIP; \
    } while (0)

// Kernel launches happen inside void launch_* helpers.  Every launch group ends with RV_LAUNCHED(name): a launch the
// runtime refused (bad grid, too much LDS, ...) is parked per thread with the kernel's name -- the first one wins -- and
// the orchestration turns it into RVSEG_ERR_HIP with launch_error_take(), so no launch fails silently.
void launch_check(const char* what);
rvseg_status launch_error_take(rvseg_ctx* ctx);
#define RV_LAUNCHED(name) ::rvseg::launch_check(name)
#define RV_LAUNCH_OK(ctx)                                               \
    do {                                                                \
        const rvseg_status st__ = ::rvseg::launch_error_take(ctx);      \
        if (st__ != RVSEG_OK) return st__;                              \
    } while (0)

rvseg_status dev_alloc(rvseg_ctx* ctx, DevBuf& b, size_t bytes);
// grow-only allocation: reallocates when the buffer is too small
rvseg_status dev_reserve(rvseg_ctx* ctx, DevBuf& b, size_t bytes);

// the stream of a device entry point: the caller's, or the context's own when the caller passes none
inline hipStream_t stream_of(const rvseg_ctx* ctx, void* hip_stream) { return hip_stream ? (hipStream_t)hip_stream : ctx->stream; }

// ---- rvseg_forest_tools.hip: what every call on a data set checks first, the per-leaf vote labels of a layer
// (ctx->tools.vote_table) that launch_tools_votes reads, and the loop over X -- shared with rvseg_prune.hip ----------
struct LayerView { int off = 0, C = 0; };   // the layer's classes inside a leaf row of the active mode
rvseg_status check_points(rvseg_ctx* ctx, const float* X, int32_t P, int32_t D);
rvseg_status layer_of(rvseg_ctx* ctx, int32_t layer, LayerView& v);
rvseg_status upload_vote_table(rvseg_ctx* ctx, int layer, hipStream_t s);
int count_blocks(rvseg_ctx* ctx);   // grids that loop: a few blocks per compute unit
// X [P][D] through ctx->tools.X in chunks of TOOLS_CHUNK points, on ctx->stream: body(base, n) enqueues what its caller
// does with points base .. base + n - 1, which are on the device; the chunk's work is complete before the next begins
rvseg_status for_each_chunk(rvseg_ctx* ctx, const float* X, int P, int D, const std::function<rvseg_status(int base, int n)>& body);

// ---- kernels_eval.hip: frees the scoring state (waits for its pending work first) -----------------------------
void eval_destroy(rvseg_ctx* ctx);

}  // namespace rvseg
