// State of the frame / CRF pipelines (ctx->impl).
#pragma once
#include "rvseg_internal.h"
#include "rvseg_kernels.h"

namespace rvseg {

struct CrfState;     // rvseg_crf_state.h (rvseg_lattice.hip, rvseg_crf.hip, rvseg_crf_model.hip)

// buffers of the fusion and of the projector that feeds it, owned by the context (no allocation per call once they have
// grown); created by fusion_state, deleted by fusion_state_free (rvseg_fusion.hip)
struct FusionState {
    DevBuf kin, kout, vin, vout, temp, start, end, bad;
    DevBuf idx, post, un;          // staging of the host entry point
    DevBuf map_un, map_feat, map_q, map_lab;   // intermediates of rvseg_process_map_device
    // projector (rvseg_project.hip): the key image of one launch group (at most 32 images x W x H uint64), the index
    // images of rvseg_process_map_poses_device, and the staging of rvseg_project_cloud (cloud in, index + z-buffer out)
    DevBuf proj_keys, proj_idx, proj_xyz, proj_stage_idx, proj_stage_z;
    PinnedBuf h_bad;               // int: pinned copy of the "index beyond cloud_size" flag
    Event bad_ev;
    bool bad_pending = false;
};

// Host-buffer entry point (rvseg_segment_frames, rvseg_segment_external): two slots of pinned staging + device buffers
// per staged channel, so that the H2D copy of chunk k+1 and the D2H copy of chunk k-1 run under the compute of chunk k
// (three streams: in, compute, out).  A channel is one array that crosses the bus -- three inputs (dist: the external
// provider's distributions), three outputs; a call reserves only the channels it uses, and no pinned staging for a
// channel whose caller buffer is page-locked (segment_host).
struct HostStage {
    static constexpr int SLOTS = 2;
    struct Channel { PinnedBuf h[SLOTS]; DevBuf d[SLOTS]; };
    Channel rgb, depth, dist, post, marg, lab;
    Stream s_in, s_out;   // created together with the six events (stage_init): s_in set = all of them exist
    Event ev_in[SLOTS], ev_done[SLOTS], ev_out[SLOTS];
};

struct Pipeline {
    FrameGeom geom{};
    HostStage stage;
    DevBuf resize_rows;
    UpsampleTables up;
    // per-chunk device buffers (grow-only, sized for up to max_batch frames)
    DevBuf calibA, lab, lab2, cloud, change, rect, nfeat, low, post, in_rgb, in_depth, dump, valid;
    // pinned staging for the per-frame A = R*Kinv, t.  The device entry point returns without
    // synchronising, so a slot may only be rewritten once the copy that read it has run: a small ring,
    // each slot guarded by an event recorded behind its H2D copy
    static constexpr int CALIB_RING = 4;
    PinnedBuf h_calibA[CALIB_RING];
    Event calib_ev[CALIB_RING];
    bool calib_ev_live[CALIB_RING] = {};
    int calib_next = 0;
    // raised (by 3 = x8 slots) every time a lattice build overflows its hash table; applies to all later
    // builds of this context (include/rvseg.h, lattice_capacity_log2)
    int cap_boost = 0;
    CrfState* crf = nullptr;        // deleted by crf_state_free
    FusionState* fusion = nullptr;  // deleted by fusion_state_free
    bool bare = false;  // created by a CRF entry point: frame tables not initialised yet
    // the lattice build depends only on the cloud and the colours, not on the forest: it runs on a
    // side stream beside feature extraction + forest evaluation (fork after prep, join before inference)
    // (created together with timer.side0 / side1 by side_init: side set = all of them exist)
    Stream side;
    Event ev_fork, ev_join, ev_entry;   // ev_entry: everything before this chunk on the caller's stream
};

// the context's pipeline state; the first caller creates it bare
Pipeline* pipeline_of(rvseg_ctx* ctx);
rvseg_status pipeline_init(rvseg_ctx* ctx);
// stages the per-frame A = R*Kinv, t of n calibrations (21 floats each) and enqueues their copy to im->calibA
rvseg_status upload_calib(rvseg_ctx* ctx, Pipeline* im, const float* calib, int n, hipStream_t s);
// One frame's feature vectors, materialised: reserves the working buffers and enqueues prep, the normal feature and the
// dump kernel on s.  The frame is in im->in_rgb / im->in_depth and its calibration uploaded (upload_calib); the result
// is im->dump (lh*lw x D floats, stride-grid order) and im->valid (lh*lw mask bytes).
rvseg_status dump_frame_features(rvseg_ctx* ctx, Pipeline* im, hipStream_t s);
void timer_reset(rvseg_ctx* ctx);
void timer_mark(rvseg_ctx* ctx, const char* name, hipStream_t s);

// The two frame entry points behind rvseg_segment_frames[_device] and rvseg_segment_external[_device]: chunking by
// max_batch, the staging ring of the host entry, the overflow contract.  ext == nullptr: features + forest produce the
// posteriors (layout = the forest's).  Otherwise the caller's distributions take their place (layout = ctx->external)
// and nothing of the forest is touched: `dist` is n x S x (H x W, or H/stride x W/stride with dist_stride > 1) floats,
// host memory for segment_host, device memory for segment_device.  Arguments are checked by the callers.
struct ExternalInput {
    const float* dist;
    int dist_stride;   // 1 or params.stride
};
rvseg_status segment_device(rvseg_ctx* ctx, const ExternalInput* ext, int n_frames, const uint8_t* d_rgb, const uint16_t* d_depth_mm,
                            const float* calib, float* d_posteriors_out, float* d_marginals_out, int8_t* d_labels_out, void* hip_stream);
rvseg_status segment_host(rvseg_ctx* ctx, const ExternalInput* ext, int n_frames, const uint8_t* rgb, const uint16_t* depth_mm,
                          const float* calib, float* posteriors_out, float* marginals_out, int8_t* labels_out);

// rvseg_fusion.hip
rvseg_status fusion_state(rvseg_ctx* ctx, FusionState** out);   // the context's fusion state, created by the first call
void fusion_state_free(Pipeline* im);
rvseg_status fusion_status(rvseg_ctx* ctx, Pipeline* im, bool wait);   // like crf_frames_status, for the index-range flag

// rvseg_project.hip: the projector of include/rvseg.h on device buffers, enqueued on s in launch groups of at most 32
// images.  proj: host, n_images x 12.  d_zbuffer may be null.  Arguments are checked by the callers (project_check).
rvseg_status project_check(rvseg_ctx* ctx, int32_t n_images, const float* proj, int32_t N, const void* xyz, const void* index_out);
rvseg_status project_enqueue(rvseg_ctx* ctx, FusionState* fs, int32_t n_images, const float* proj, int32_t N, const float* d_xyz,
                             int32_t* d_index, float* d_zbuffer, hipStream_t s);

// rvseg_crf.hip
void crf_state_free(Pipeline* im);
// DenseCRF on a cloud whose unaries / features live in HBM, for every label layer over ONE lattice:
// d_unaries = layers concatenated, each N x C_l accumulated log-posteriors (energy = -unary,
// src/segmenter.cpp:642); labels (optional) L x N; marginals stay in context memory
rvseg_status crf_cloud_layers(rvseg_ctx* ctx, int N, int n_layers, const int* class_counts, const float* d_unaries,
                              const float* d_features, float potts_w, int iterations, int label_mode, const int* unknown,
                              int8_t* d_labels, hipStream_t s);
// per-frame, per-layer DenseCRF on the frames of one chunk: unary = -(posteriors), features from
// the back-projected cloud and the colours
// part 1 (lattice + normaliser; needs the cloud only) and part 2 (mean field per layer + labels)
rvseg_status crf_frames_build_begin(rvseg_ctx* ctx, Pipeline* im, int n, hipStream_t s);
rvseg_status crf_frames_build(rvseg_ctx* ctx, Pipeline* im, int n, const uint8_t* d_rgb, hipStream_t s);
// Status of the last enqueued frame build (consumes it): RVSEG_OK, RVSEG_NOT_READY (only without `wait`)
// or RVSEG_ERR_CAPACITY after raising im->cap_boost.  RVSEG_OK when nothing is pending.
rvseg_status crf_frames_status(rvseg_ctx* ctx, Pipeline* im, bool wait);
// `layers`: the layout of d_post -- the loaded forest's, or the external provider's
rvseg_status crf_frames_infer(rvseg_ctx* ctx, Pipeline* im, const LayerLayout& layers, int n, const float* d_post, float* d_marg,
                              int8_t* d_labels, hipStream_t s);

}  // namespace rvseg
