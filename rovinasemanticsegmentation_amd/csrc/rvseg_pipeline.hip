// Frame pipeline: host orchestration of the per-frame hot path over batches of key frames
// (replaces the body of Segmenter::processFramesFromQueueInternalRF, src/segmenter.cpp:351-431,
// and -- with use_dense_crf -- the DenseCRF call shape of src/segmenter.cpp:639-657 per frame).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "rvseg_internal.h"
#include "rvseg_kernels.h"
#include "rvseg_pipeline.h"

namespace rvseg {

// ---- cv::resize coefficient rule (OpenCV 2.4 imgwarp.cpp), identical to the oracle's statement
static void resize_coeffs(int ssize, int dsize, bool clamp_weights, std::vector<int>& ofs,
                          std::vector<float>& w0, std::vector<float>& w1) {
    ofs.resize(dsize); w0.resize(dsize); w1.resize(dsize);
    const double inv_scale = (double)dsize / ssize;
    const double scale = 1. / inv_scale;
    for (int d = 0; d < dsize; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= s;
        if (clamp_weights) {
            if (s < 0) { f = 0; s = 0; }
            if (s >= ssize - 1) { f = 0; s = ssize - 1; }
        }
        ofs[d] = s; w0[d] = 1.f - f; w1[d] = f;
    }
}

static rvseg_status upload(rvseg_ctx* ctx, DevBuf& b, const void* src, size_t bytes) {
    rvseg_status st = dev_alloc(ctx, b, bytes);
    if (st != RVSEG_OK) return st;
    RV_HIP(ctx, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return RVSEG_OK;
}

rvseg_status pipeline_init(rvseg_ctx* ctx) {
    if (ctx->impl && !ctx->impl->bare) return RVSEG_OK;
    const rvseg_params& p = ctx->params;
    if (p.width % p.stride != 0 || p.height % p.stride != 0) {
        // the reference would scatter outside its low-res image (segmenter.cpp:357,370)
        ctx->err = "width and height must be multiples of rf_prediction_stride";
        return RVSEG_ERR_INVALID_ARG;
    }
    if (p.patch_size_reduce > 16) { ctx->err = "patch_size_reduce > 16 is not supported"; return RVSEG_ERR_INVALID_ARG; }
    Pipeline* im = pipeline_of(ctx);
    FrameGeom& g = im->geom;
    g.W = p.width; g.H = p.height; g.stride = p.stride;
    g.lw = p.width / p.stride; g.lh = p.height / p.stride;
    g.depth_min = p.depth_min; g.depth_max = p.depth_max;
    g.dmin_mm = (float)(p.depth_min * 1000.0); g.dmax_mm = (float)(p.depth_max * 1000.0);  // feature_extractor.h:43-44
    g.patch_size = p.patch_size; g.r = p.patch_size_reduce;
    g.n_patch = p.feature_color_patch ? g.r * g.r * 3 : 0;
    int pos = g.n_patch;
    g.pos_depth = p.feature_depth ? pos++ : -1;
    g.pos_height = p.feature_height ? pos++ : -1;
    g.pos_normal = p.feature_normal ? pos++ : -1;
    g.D = pos;
    g.fill = p.fill_value;
    g.rt_rows = 0;

    rvseg_status st;
    // 8-bit patch resize tables, one row per ROI half size
    if (p.feature_color_patch) {
        const int max_half = (int)(p.patch_size / (2.0 * p.depth_min));
        std::vector<ResizeRow> rows((size_t)max_half + 1);
        std::vector<int> ofs; std::vector<float> w0, w1;
        for (int half = 0; half <= max_half; half++) {
            const int size = 2 * half + 1;
            ResizeRow& rr = rows[half];
            std::memset(&rr, 0, sizeof(rr));
            resize_coeffs(size, g.r, true, ofs, w0, w1);
            for (int d = 0; d < g.r; d++) {
                rr.x[d].ofs = (int16_t)ofs[d];
                rr.x[d].w0 = (int16_t)std::lrintf(w0[d] * 2048.f);  // saturate_cast<short>: round half to even
                rr.x[d].w1 = (int16_t)std::lrintf(w1[d] * 2048.f);
                rr.x[d].ofs1 = (int16_t)(ofs[d] + 1 < size ? ofs[d] + 1 : ofs[d]);   // second tap, kept inside the ROI
            }
            resize_coeffs(size, g.r, false, ofs, w0, w1);
            for (int d = 0; d < g.r; d++) {
                // rows are clipped to the ROI (the weights are not): both clipped taps are part of the record
                const int s0 = ofs[d] < 0 ? 0 : (ofs[d] >= size ? size - 1 : ofs[d]);
                const int s1 = ofs[d] + 1 < 0 ? 0 : (ofs[d] + 1 >= size ? size - 1 : ofs[d] + 1);
                rr.y[d].ofs = (int16_t)s0;
                rr.y[d].w0 = (int16_t)std::lrintf(w0[d] * 2048.f);
                rr.y[d].w1 = (int16_t)std::lrintf(w1[d] * 2048.f);
                rr.y[d].ofs1 = (int16_t)s1;
            }
        }
        if ((st = upload(ctx, im->resize_rows, rows.data(), rows.size() * sizeof(ResizeRow))) != RVSEG_OK) return st;
        g.rt_rows = (int)rows.size();
    }
    // float up-sampling tables
    {
        std::vector<int> ofs; std::vector<float> w0, w1;
        resize_coeffs(g.lw, g.W, true, ofs, w0, w1);
        if ((st = upload(ctx, im->up.xofs, ofs.data(), ofs.size() * 4)) != RVSEG_OK) return st;
        if ((st = upload(ctx, im->up.ax0, w0.data(), w0.size() * 4)) != RVSEG_OK) return st;
        if ((st = upload(ctx, im->up.ax1, w1.data(), w1.size() * 4)) != RVSEG_OK) return st;
        resize_coeffs(g.lh, g.H, false, ofs, w0, w1);
        if ((st = upload(ctx, im->up.yofs, ofs.data(), ofs.size() * 4)) != RVSEG_OK) return st;
        if ((st = upload(ctx, im->up.ay0, w0.data(), w0.size() * 4)) != RVSEG_OK) return st;
        if ((st = upload(ctx, im->up.ay1, w1.data(), w1.size() * 4)) != RVSEG_OK) return st;
    }
    im->bare = false;
    return RVSEG_OK;
}

Pipeline* pipeline_of(rvseg_ctx* ctx) {
    if (!ctx->impl) {
        ctx->impl = new Pipeline();
        ctx->impl->bare = true;
    }
    return ctx->impl;
}

// A = R*Kinv, Eigen fixed 3x3 product accumulated left to right (feature_extractor.h:223)
static void calib_to_A(const float* calib, float* out12) {
    const float *Kinv = calib, *R = calib + 9, *t = calib + 18;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            out12[i * 3 + j] = (R[i * 3 + 0] * Kinv[0 * 3 + j] + R[i * 3 + 1] * Kinv[1 * 3 + j]) + R[i * 3 + 2] * Kinv[2 * 3 + j];
    out12[9] = t[0]; out12[10] = t[1]; out12[11] = t[2];
}

rvseg_status upload_calib(rvseg_ctx* ctx, Pipeline* im, const float* calib, int n, hipStream_t s) {
    const int slot = im->calib_next;
    im->calib_next = (slot + 1) % Pipeline::CALIB_RING;
    if (!im->calib_ev[slot]) RV_HIP(ctx, event_create(im->calib_ev[slot], hipEventDisableTiming));
    // the copy that last read this slot must have run before the host rewrites (or frees) it
    if (im->calib_ev_live[slot]) { RV_HIP(ctx, hipEventSynchronize(im->calib_ev[slot])); im->calib_ev_live[slot] = false; }
    const size_t bytes = (size_t)n * 12 * sizeof(float);
    rvseg_status st = im->h_calibA[slot].reserve(ctx, bytes);
    if (st != RVSEG_OK) return st;
    float* h = im->h_calibA[slot].as<float>();
    for (int i = 0; i < n; i++) calib_to_A(calib + (size_t)i * 21, h + (size_t)i * 12);
    if ((st = dev_reserve(ctx, im->calibA, bytes)) != RVSEG_OK) return st;   // (a reallocation frees with hipFree, which waits for the device)
    RV_HIP(ctx, hipMemcpyAsync(im->calibA.p, h, bytes, hipMemcpyHostToDevice, s));
    RV_HIP(ctx, hipEventRecord(im->calib_ev[slot], s));
    im->calib_ev_live[slot] = true;
    return RVSEG_OK;
}

// ---- the materialised feature vectors of one frame (rvseg_extract_features, rvseg_forest_train_frames) -----------
rvseg_status dump_frame_features(rvseg_ctx* ctx, Pipeline* im, hipStream_t s) {
    const FrameGeom& g = im->geom;
    const size_t npix = (size_t)g.W * g.H;
    const int P = g.lw * g.lh;
    const bool normal = ctx->params.feature_normal;
    rvseg_status st;
    if ((st = dev_reserve(ctx, im->lab, npix * 4)) != RVSEG_OK || (st = dev_reserve(ctx, im->cloud, npix * 16)) != RVSEG_OK ||
        (st = dev_reserve(ctx, im->rect, npix)) != RVSEG_OK || (st = dev_reserve(ctx, im->change, npix)) != RVSEG_OK ||
        (st = dev_reserve(ctx, im->nfeat, (size_t)P * 4)) != RVSEG_OK || (st = dev_reserve(ctx, im->dump, (size_t)P * g.D * 4)) != RVSEG_OK ||
        (st = dev_reserve(ctx, im->valid, (size_t)P)) != RVSEG_OK) return st;
    launch_prep(g, ctx->lab, im->in_rgb.as<uint8_t>(), im->in_depth.as<uint16_t>(), im->calibA.as<float>(), im->lab.as<uint32_t>(),
                im->cloud.as<float4>(), normal ? im->change.as<uint8_t>() : nullptr, 1, s);
    if (normal) {
        launch_window_map(g, im->cloud.as<float4>(), im->change.as<uint8_t>(), im->rect.as<uint8_t>(), 1, s);
        launch_normal_feature(g, im->cloud.as<float4>(), im->rect.as<uint8_t>(), im->nfeat.as<float>(), 1, s);
    }
    launch_feature_dump(g, im->resize_rows.as<ResizeRow>(), im->lab.as<uint32_t>(), im->in_depth.as<uint16_t>(), im->cloud.as<float4>(),
                        im->nfeat.as<float>(), im->dump.as<float>(), im->valid.as<uint8_t>(), 1, s);
    return RVSEG_OK;
}

// ---- stage timing ----------------------------------------------------------------------------
void timer_reset(rvseg_ctx* ctx) {
    ctx->timer.names.clear();
    ctx->timer.ms.clear();
    ctx->timer.used = 0;
    ctx->timer.side_used = false;
}

void timer_mark(rvseg_ctx* ctx, const char* name, hipStream_t s) {
    StageTimer& t = ctx->timer;
    if (t.used >= t.events.size()) {
        Event e;
        if (event_create(e, hipEventDefault) != hipSuccess) return;
        t.events.push_back(std::move(e));
    }
    (void)hipEventRecord(t.events[t.used++], s);
    t.names.push_back(name);
}

// ---- the frame path for one chunk of at most max_batch frames ----------------------------------
// element counts per frame of the arrays both drivers chunk: pixels, classes over all layers (of the forest, or of the
// external provider's layout), layers, and floats of the provider's distributions
struct FrameSizes { size_t npix, S, L, dist; };
static FrameSizes frame_sizes(const rvseg_ctx* ctx, const FrameGeom& g, const ExternalInput* ext) {
    const LayerLayout& lay = ext ? ctx->external : static_cast<const LayerLayout&>(ctx->forest);
    const size_t npix = (size_t)g.W * g.H, S = (size_t)lay.sum_classes;
    return {npix, S, (size_t)lay.n_layers, ext ? S * (ext->dist_stride > 1 ? (size_t)g.lw * g.lh : npix) : 0};
}

// the device pointers of one chunk
struct ChunkIo {
    const uint8_t* rgb; const uint16_t* depth; const float* calibA;
    const float* dist; int dist_stride;   // the external provider's distributions; null: features + forest make the posteriors
    float *post, *marg; int8_t* labels;   // outputs, each optional (post: forest only)
};

// the build stream and what orders and times it, created by the first chunk that forks the lattice build
static rvseg_status side_init(rvseg_ctx* ctx, Pipeline* im) {
    if (im->side) return RVSEG_OK;
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    // priority of the build stream.  Round 1 (build = the longer branch) measured the highest priority ahead,
    // 13.85 vs 13.98 ms per step; since the feature branch is the longer one (5.2 vs 3.6 ms) the lowest is, by
    // a little: 13.31 / 13.33 vs 13.37 / 13.42 ms (rvseg_schedule.build_priority_high restores the old choice;
    // it is read when the stream is created, i.e. before the first frame call of the context)
    Stream side;
    Event fork, join, entry, side0, side1;
    RV_HIP(ctx, stream_create(side, hipStreamNonBlocking, ctx->sched.build_priority_high ? prio_hi : prio_lo));
    RV_HIP(ctx, event_create(fork, hipEventDisableTiming));
    RV_HIP(ctx, event_create(join, hipEventDisableTiming));
    RV_HIP(ctx, event_create(entry, hipEventDisableTiming));
    RV_HIP(ctx, event_create(side0, hipEventDefault));
    RV_HIP(ctx, event_create(side1, hipEventDefault));
    im->ev_fork = std::move(fork);   // all six exist: hand them over
    im->ev_join = std::move(join);
    im->ev_entry = std::move(entry);
    ctx->timer.side0 = std::move(side0);
    ctx->timer.side1 = std::move(side1);
    im->side = std::move(side);
    return RVSEG_OK;
}

static rvseg_status run_chunk(rvseg_ctx* ctx, Pipeline* im, int n, const ChunkIo& io, hipStream_t s) {
    const FrameGeom& g = im->geom;
    const rvseg_params& p = ctx->params;
    const size_t npix = (size_t)g.W * g.H;
    const LayerLayout& lay = io.dist ? ctx->external : static_cast<const LayerLayout&>(ctx->forest);
    rvseg_status st;
    const float* post;     // the chunk's posteriors, n x S x H x W: each provider's block leaves them here
    bool forked = false;   // the lattice build is already running on the side stream
    if (io.dist) {
        // ---- an external provider: its distributions are the posteriors (segmenter.cpp:445-514).  No Lab image, no
        // change map, no features, no forest.  There is nothing for the lattice build to hide under, so it runs on the
        // caller's stream without the fork.
        post = io.dist;   // full resolution: the wire layout is the posterior layout
        if (io.dist_stride > 1) {
            // the wire layout at low resolution is the up-sampler's `low` layout ([layer][ly][lx][class] per frame): no repack
            if ((st = dev_reserve(ctx, im->post, npix * lay.sum_classes * 4 * n)) != RVSEG_OK) return st;
            timer_mark(ctx, "upsample_pack", s);
            launch_upsample_pack(g, lay, im->up, io.dist, im->post.as<float>(), n, s);
            post = im->post.as<float>();
        }
        if (p.use_dense_crf) {
            if ((st = dev_reserve(ctx, im->cloud, npix * 16 * n)) != RVSEG_OK) return st;
            timer_mark(ctx, "prep", s);
            launch_prep(g, ctx->lab, io.rgb, io.depth, io.calibA, nullptr, im->cloud.as<float4>(), nullptr, n, s);
        }
    } else {
        // ---- features + forest
        const DeviceForest& f = ctx->forest;
        const bool need_cloud = p.feature_height || p.feature_normal || p.use_dense_crf;
        if (p.feature_color_patch && (st = dev_reserve(ctx, im->lab, npix * 4 * n)) != RVSEG_OK) return st;
        const bool use_lab2 = p.feature_color_patch && rf_frames_wants_lab2(f);
        if (use_lab2 && (st = dev_reserve(ctx, im->lab2, npix * 8 * n + 16)) != RVSEG_OK) return st;
        if (need_cloud && (st = dev_reserve(ctx, im->cloud, npix * 16 * n)) != RVSEG_OK) return st;
        if (p.feature_normal) {
            if ((st = dev_reserve(ctx, im->rect, npix * n)) != RVSEG_OK) return st;
            if ((st = dev_reserve(ctx, im->change, npix * n)) != RVSEG_OK) return st;
            if ((st = dev_reserve(ctx, im->nfeat, (size_t)g.lw * g.lh * 4 * n)) != RVSEG_OK) return st;
        }
        if ((st = dev_reserve(ctx, im->low, (size_t)g.lw * g.lh * f.sum_classes * 4 * n)) != RVSEG_OK) return st;
        float* out = io.post;
        if (!out) {
            if ((st = dev_reserve(ctx, im->post, npix * f.sum_classes * 4 * n)) != RVSEG_OK) return st;
            out = im->post.as<float>();
        }
        const bool fork_build = p.use_dense_crf && ctx->sched.overlap_build;
        if (fork_build) {
            // the build stream first: table and list heads of the new lattice are cleared while prep_kernel runs.  The
            // lattice's previous user (the last chunk's mean field, a cloud CRF on this context) ran on the caller's
            // stream: ev_entry, recorded there before anything of this chunk, orders the memsets behind it.
            if ((st = side_init(ctx, im)) != RVSEG_OK) return st;
            RV_HIP(ctx, hipEventRecord(im->ev_entry, s));
            RV_HIP(ctx, hipStreamWaitEvent(im->side, im->ev_entry, 0));
            if ((st = crf_frames_build_begin(ctx, im, n, im->side)) != RVSEG_OK) return st;
        }
        timer_mark(ctx, "prep", s);
        launch_prep(g, ctx->lab, io.rgb, io.depth, io.calibA, p.feature_color_patch ? im->lab.as<uint32_t>() : nullptr,
                    need_cloud ? im->cloud.as<float4>() : nullptr, p.feature_normal ? im->change.as<uint8_t>() : nullptr, n, s,
                    use_lab2 ? im->lab2.as<uint2>() : nullptr);
        if (fork_build) {
            // fork: the lattice build runs on the side stream while this stream extracts features and walks the forest
            RV_HIP(ctx, hipEventRecord(im->ev_fork, s));
            RV_HIP(ctx, hipStreamWaitEvent(im->side, im->ev_fork, 0));
            RV_HIP(ctx, hipEventRecord(ctx->timer.side0, im->side));
            if ((st = crf_frames_build(ctx, im, n, io.rgb, im->side)) != RVSEG_OK) { (void)hipStreamSynchronize(im->side); return st; }
            RV_HIP(ctx, hipEventRecord(ctx->timer.side1, im->side));
            RV_HIP(ctx, hipEventRecord(im->ev_join, im->side));
            ctx->timer.side_name = "lattice_build";
            ctx->timer.side_used = true;
            forked = true;
        }
        if (p.feature_normal) {
            timer_mark(ctx, "window_map", s);
            launch_window_map(g, im->cloud.as<float4>(), im->change.as<uint8_t>(), im->rect.as<uint8_t>(), n, s);
            timer_mark(ctx, "normal_feature", s);
            launch_normal_feature(g, im->cloud.as<float4>(), im->rect.as<uint8_t>(), im->nfeat.as<float>(), n, s);
        }
        timer_mark(ctx, "rf_frames", s);
        launch_rf_frames(g, f, im->resize_rows.as<ResizeRow>(), im->lab.as<uint32_t>(), io.depth, im->cloud.as<float4>(),
                         im->nfeat.as<float>(), im->low.as<float>(), n, s, use_lab2 ? im->lab2.as<uint2>() : nullptr);
        timer_mark(ctx, "upsample_pack", s);
        launch_upsample_pack(g, f, im->up, im->low.as<float>(), out, n, s);
        post = out;
    }
    // ---- both providers: the frame CRF on the posteriors, or their labels
    if (p.use_dense_crf) {
        if (forked) {
            RV_HIP(ctx, hipStreamWaitEvent(s, im->ev_join, 0));   // join
        } else {
            timer_mark(ctx, "lattice_build", s);
            if ((st = crf_frames_build(ctx, im, n, io.rgb, s)) != RVSEG_OK) return st;
        }
        if ((st = crf_frames_infer(ctx, im, lay, n, post, io.marg, io.labels, s)) != RVSEG_OK) return st;
    } else if (io.labels) {
        timer_mark(ctx, "labels", s);
        launch_labels_frames(post, n, (int)npix, lay, p.label_mode, p.unknown_label, io.labels, s);
    }
    timer_mark(ctx, "end", s);
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

rvseg_status segment_device(rvseg_ctx* ctx, const ExternalInput* ext, int n_frames, const uint8_t* d_rgb, const uint16_t* d_depth_mm,
                            const float* calib, float* d_posteriors_out, float* d_marginals_out, int8_t* d_labels_out, void* hip_stream) {
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    rvseg_status st = pipeline_init(ctx);
    if (st != RVSEG_OK) return st;
    Pipeline* im = ctx->impl;
    hipStream_t s = stream_of(ctx, hip_stream);
    timer_reset(ctx);
    if ((st = upload_calib(ctx, im, calib, n_frames, s)) != RVSEG_OK) return st;
    const FrameSizes z = frame_sizes(ctx, im->geom, ext);
    auto from = [](auto* p, size_t off) { return p ? p + off : nullptr; };   // an optional array, `off` elements in
    for (int start = 0; start < n_frames; start += ctx->params.max_batch) {
        const int n = std::min(ctx->params.max_batch, n_frames - start);
        const size_t px = (size_t)start * z.npix;
        const ChunkIo io{d_rgb + px * 3, d_depth_mm + px, im->calibA.as<float>() + (size_t)start * 12,
                         ext ? ext->dist + (size_t)start * z.dist : nullptr, ext ? ext->dist_stride : 0,
                         from(d_posteriors_out, px * z.S), from(d_marginals_out, px * z.S), from(d_labels_out, px * z.L)};
        if ((st = run_chunk(ctx, im, n, io, s)) != RVSEG_OK) return st;
    }
    return RVSEG_OK;
}

}  // namespace rvseg

using namespace rvseg;

extern "C" {

void rvseg_pipeline_destroy(rvseg_ctx* ctx) {
    if (!ctx || !ctx->impl) return;
    Pipeline* im = ctx->impl;
    // the copy that last read a calibration slot must have run before the slot's event and pinned block go
    for (Event& ev : im->calib_ev) if (ev) (void)hipEventSynchronize(ev);
    crf_state_free(im);
    fusion_state_free(im);
    delete im;
    ctx->impl = nullptr;
}

rvseg_status rvseg_segment_frames_device(rvseg_ctx* ctx, int32_t n_frames, const uint8_t* d_rgb,
                                         const uint16_t* d_depth_mm, const float* calib, float* d_posteriors_out,
                                         float* d_marginals_out, int8_t* d_labels_out, void* hip_stream) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (!ctx->forest_loaded) { ctx->err = "no forest loaded"; return RVSEG_ERR_NO_FOREST; }
    if (n_frames < 0 || (n_frames > 0 && (!d_rgb || !d_depth_mm || !calib))) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    if (n_frames == 0) return RVSEG_OK;
    return segment_device(ctx, nullptr, n_frames, d_rgb, d_depth_mm, calib, d_posteriors_out, d_marginals_out, d_labels_out, hip_stream);
}

}  // extern "C"

// ---- host-buffer entry: pinned staging ring, copies of neighbouring chunks under the compute ----
namespace {

// pageable <-> pinned copies; large ones are split over a few host threads (one memcpy stream saturates
// well below the memory bandwidth of the host)
void host_copy(void* dst, const void* src, size_t bytes) {
    const size_t min_part = (size_t)4 << 20;
    unsigned nt = (unsigned)std::min<size_t>(8, bytes / min_part);
    const unsigned hw = std::thread::hardware_concurrency();
    if (hw && nt > hw) nt = hw;
    if (nt <= 1) { std::memcpy(dst, src, bytes); return; }
    std::vector<std::thread> th;
    const size_t part = (bytes / nt + 4095) & ~(size_t)4095;
    for (unsigned t = 0; t < nt; t++) {
        const size_t off = (size_t)t * part;
        if (off >= bytes) break;
        const size_t len = std::min(part, bytes - off);
        th.emplace_back([=] { std::memcpy((char*)dst + off, (const char*)src + off, len); });
    }
    for (auto& x : th) x.join();
}

// is p page-locked host memory (hipHostMalloc / hipHostRegister, e.g. through rvseg_host_register)?  Then the DMA engines
// reach it directly and the pinned staging copy is skipped.
bool is_pinned_host(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // pageable memory is unknown to the runtime
    return at.type == hipMemoryTypeHost;
}

rvseg_status stage_init(rvseg_ctx* ctx, HostStage& hs) {
    if (hs.s_in) return RVSEG_OK;
    Stream s_in, s_out;
    Event in[HostStage::SLOTS], done[HostStage::SLOTS], out[HostStage::SLOTS];
    RV_HIP(ctx, stream_create(s_in, hipStreamNonBlocking));
    RV_HIP(ctx, stream_create(s_out, hipStreamNonBlocking));
    for (int i = 0; i < HostStage::SLOTS; i++) {
        RV_HIP(ctx, event_create(in[i], hipEventDisableTiming));
        RV_HIP(ctx, event_create(done[i], hipEventDisableTiming));
        RV_HIP(ctx, event_create(out[i], hipEventDisableTiming));
    }
    for (int i = 0; i < HostStage::SLOTS; i++) {   // all eight exist: hand them over
        hs.ev_in[i] = std::move(in[i]);
        hs.ev_done[i] = std::move(done[i]);
        hs.ev_out[i] = std::move(out[i]);
    }
    hs.s_out = std::move(s_out);
    hs.s_in = std::move(s_in);
    return RVSEG_OK;
}

// one staged channel of one call
struct Staged {
    HostStage::Channel* ch;
    char* host;           // the caller's array
    size_t frame_bytes;
    bool out;             // direction: false = host -> device on s_in, true = device -> host on s_out
    bool pinned;          // the caller's memory is page-locked: the copy engines reach it directly, no staging copy
    char* caller(size_t frame) const { return host + frame * frame_bytes; }
    // host end of the DMA of the chunk that starts at `frame`
    void* dma(int slot, size_t frame) const { return pinned ? (void*)caller(frame) : ch->h[slot].p; }
};

}  // namespace

rvseg_status rvseg::segment_host(rvseg_ctx* ctx, const ExternalInput* ext, int n_frames, const uint8_t* rgb, const uint16_t* depth_mm,
                                 const float* calib, float* posteriors_out, float* marginals_out, int8_t* labels_out) {
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    rvseg_status st = pipeline_init(ctx);
    if (st != RVSEG_OK) return st;
    Pipeline* im = ctx->impl;
    HostStage& hs = im->stage;
    if ((st = stage_init(ctx, hs)) != RVSEG_OK) return st;
    const FrameSizes z = frame_sizes(ctx, im->geom, ext);
    hipStream_t s = ctx->stream;
    // The channels of this call, inputs first (the order of the copies on s_in and on s_out).  Page-locked caller
    // buffers are read / written by the copy engines directly (no staging copy on the host): the 11 MB of marginals per
    // frame otherwise cross the host memory twice, which bounds the call at ~10 GB/s
    std::vector<Staged> act;
    auto stage = [&](HostStage::Channel& ch, const void* host, size_t frame_bytes, bool out, bool pinned) {
        if (host) act.push_back({&ch, (char*)host, frame_bytes, out, pinned});
    };
    const bool in_pinned = is_pinned_host(rgb) && is_pinned_host(depth_mm);
    const size_t post_bytes = z.npix * z.S * 4;
    stage(hs.rgb, rgb, z.npix * 3, false, in_pinned);
    stage(hs.depth, depth_mm, z.npix * 2, false, in_pinned);
    if (ext) stage(hs.dist, ext->dist, z.dist * 4, false, is_pinned_host(ext->dist));
    stage(hs.post, posteriors_out, post_bytes, true, is_pinned_host(posteriors_out));
    const bool want_marg = marginals_out && ctx->params.use_dense_crf;
    if (want_marg) stage(hs.marg, marginals_out, post_bytes, true, is_pinned_host(marginals_out));
    stage(hs.lab, labels_out, z.npix * z.L, true, is_pinned_host(labels_out));
    // chunk size: at most max_batch, and small enough that a call has a few chunks to overlap
    const int chunk = std::max(1, std::min(ctx->params.max_batch, std::max(8, (n_frames + 3) / 4)));
    const int n_chunks = (n_frames + chunk - 1) / chunk;
    auto chunk_n = [&](int c) { return std::min(chunk, n_frames - c * chunk); };

    // steps 1-4 of chunk c: stage its inputs, copy them in, compute, copy the outputs back.  RVSEG_ERR_CAPACITY: the
    // lattice build of chunk c - 1 (or of an earlier call nobody polled) overflowed its hash table -- its status is read
    // at the start of this chunk's build, and nothing of chunk c has been enqueued past the feature branch
    auto enqueue_chunk = [&](int c) -> rvseg_status {
        const int slot = c % HostStage::SLOTS, n = chunk_n(c);
        const size_t start = (size_t)c * chunk;
        rvseg_status st;
        // staging + device buffers of this slot (grow only; the slot's previous chunk c - 2 has been retired)
        for (const Staged& u : act)
            if ((!u.pinned && (st = u.ch->h[slot].reserve(ctx, u.frame_bytes * n)) != RVSEG_OK) ||
                (st = dev_reserve(ctx, u.ch->d[slot], u.frame_bytes * n)) != RVSEG_OK) return st;
        // 1. caller's pageable buffers -> pinned (host threads; the GPU is busy with chunk c - 1 meanwhile)
        for (const Staged& u : act)
            if (!u.out && !u.pinned) host_copy(u.ch->h[slot].p, u.caller(start), u.frame_bytes * n);
        // 2. H2D on the input stream, after the compute of chunk c - 2 (the last reader of these device buffers)
        if (c >= HostStage::SLOTS) RV_HIP(ctx, hipStreamWaitEvent(hs.s_in, hs.ev_done[slot], 0));
        for (const Staged& u : act)
            if (!u.out) RV_HIP(ctx, hipMemcpyAsync(u.ch->d[slot].p, u.dma(slot, start), u.frame_bytes * n, hipMemcpyHostToDevice, hs.s_in));
        RV_HIP(ctx, hipEventRecord(hs.ev_in[slot], hs.s_in));
        // 3. compute: after its inputs arrived and after the D2H of chunk c - 2 released the output buffers
        RV_HIP(ctx, hipStreamWaitEvent(s, hs.ev_in[slot], 0));
        if (c >= HostStage::SLOTS) RV_HIP(ctx, hipStreamWaitEvent(s, hs.ev_out[slot], 0));
        timer_reset(ctx);
        if ((st = upload_calib(ctx, im, calib + start * 21, n, s)) != RVSEG_OK) return st;
        const ChunkIo io{hs.rgb.d[slot].as<uint8_t>(), hs.depth.d[slot].as<uint16_t>(), im->calibA.as<float>(),
                         ext ? hs.dist.d[slot].as<float>() : nullptr, ext ? ext->dist_stride : 0,
                         posteriors_out ? hs.post.d[slot].as<float>() : nullptr, want_marg ? hs.marg.d[slot].as<float>() : nullptr,
                         labels_out ? hs.lab.d[slot].as<int8_t>() : nullptr};
        if ((st = run_chunk(ctx, im, n, io, s)) != RVSEG_OK) return st;
        RV_HIP(ctx, hipEventRecord(hs.ev_done[slot], s));
        // 4. D2H on the output stream
        RV_HIP(ctx, hipStreamWaitEvent(hs.s_out, hs.ev_done[slot], 0));
        for (const Staged& u : act)
            if (u.out) RV_HIP(ctx, hipMemcpyAsync(u.dma(slot, start), u.ch->d[slot].p, u.frame_bytes * n, hipMemcpyDeviceToHost, hs.s_out));
        RV_HIP(ctx, hipEventRecord(hs.ev_out[slot], hs.s_out));
        return RVSEG_OK;
    };
    // copies the outputs of chunk c from its pinned slot into the caller's buffers (after its D2H has run).  Taking a
    // chunk twice, as after a retry, copies the same bytes again
    auto retire = [&](int c) -> rvseg_status {
        const int slot = c % HostStage::SLOTS, n = chunk_n(c);
        RV_HIP(ctx, hipEventSynchronize(hs.ev_out[slot]));
        for (const Staged& u : act)
            if (u.out && !u.pinned) host_copy(u.caller((size_t)c * chunk), u.ch->h[slot].p, u.frame_bytes * n);
        return RVSEG_OK;
    };
    auto drain = [&]() { (void)hipStreamSynchronize(hs.s_in); (void)hipStreamSynchronize(s); (void)hipStreamSynchronize(hs.s_out); };
    auto fail = [&](rvseg_status e) { drain(); return e; };

    int next = 0, retries = 0;   // next: the chunk to enqueue; every chunk before next - 1 has been retired
    // Capacity overflow reported for the build of chunk k (the context has raised its capacity): drain, and enqueue
    // again from k.  False when st is another status, or the budget of 16 retries per call is spent.
    auto redo_from = [&](rvseg_status st, int k) {
        if (st != RVSEG_ERR_CAPACITY || retries++ >= 16) return false;
        drain();
        next = k;
        return true;
    };
    // the status of the last build is the only one nobody has looked at once all chunks are enqueued
    auto last_build = [&]() -> rvseg_status {
        RV_HIP(ctx, hipStreamSynchronize(s));
        return ctx->params.use_dense_crf ? crf_frames_status(ctx, im, true) : RVSEG_OK;
    };
    do {
        while (next < n_chunks) {
            st = enqueue_chunk(next);   // reports the build of chunk next - 1
            if (redo_from(st, std::max(0, next - 1))) continue;
            if (st != RVSEG_OK) return fail(st);
            // hand chunk next - 1 to the caller while chunk next runs
            if (next >= 1 && (st = retire(next - 1)) != RVSEG_OK) return fail(st);
            next++;
        }
    } while (redo_from(st = last_build(), n_chunks - 1));
    if (st != RVSEG_OK || (st = retire(n_chunks - 1)) != RVSEG_OK) return fail(st);
    return RVSEG_OK;
}

extern "C" {

rvseg_status rvseg_segment_frames(rvseg_ctx* ctx, int32_t n_frames, const uint8_t* rgb, const uint16_t* depth_mm,
                                  const float* calib, float* posteriors_out, float* marginals_out, int8_t* labels_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (!ctx->forest_loaded) { ctx->err = "no forest loaded"; return RVSEG_ERR_NO_FOREST; }
    if (n_frames < 0 || (n_frames > 0 && (!rgb || !depth_mm || !calib))) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    if (n_frames == 0) return RVSEG_OK;
    return segment_host(ctx, nullptr, n_frames, rgb, depth_mm, calib, posteriors_out, marginals_out, labels_out);
}

rvseg_status rvseg_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return RVSEG_ERR_INVALID_ARG;
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); return e == hipErrorHostMemoryAlreadyRegistered ? RVSEG_OK : RVSEG_ERR_HIP; }
    return RVSEG_OK;
}

rvseg_status rvseg_host_unregister(void* p) {
    if (!p) return RVSEG_ERR_INVALID_ARG;
    if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return RVSEG_ERR_HIP; }
    return RVSEG_OK;
}

rvseg_status rvseg_poll_status(rvseg_ctx* ctx, int32_t wait) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (!ctx->impl) return RVSEG_OK;
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    Pipeline* im = ctx->impl;
    const rvseg_status a = crf_frames_status(ctx, im, wait != 0);
    if (a != RVSEG_OK) return a;
    return fusion_status(ctx, im, wait != 0);
}

rvseg_status rvseg_extract_features(rvseg_ctx* ctx, const uint8_t* rgb, const uint16_t* depth_mm, const float* calib,
                                    float* feat_out, int32_t* x_v, int32_t* y_v, int32_t* n_points) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (!rgb || !depth_mm || !calib || !feat_out || !x_v || !y_v || !n_points) { ctx->err = "null argument"; return RVSEG_ERR_INVALID_ARG; }
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    rvseg_status st = pipeline_init(ctx);
    if (st != RVSEG_OK) return st;
    Pipeline* im = ctx->impl;
    const FrameGeom& g = im->geom;
    const size_t npix = (size_t)g.W * g.H;
    const int P = g.lw * g.lh;
    hipStream_t s = ctx->stream;
    if ((st = dev_reserve(ctx, im->in_rgb, npix * 3)) != RVSEG_OK) return st;
    if ((st = dev_reserve(ctx, im->in_depth, npix * 2)) != RVSEG_OK) return st;
    RV_HIP(ctx, hipMemcpyAsync(im->in_rgb.p, rgb, npix * 3, hipMemcpyHostToDevice, s));
    RV_HIP(ctx, hipMemcpyAsync(im->in_depth.p, depth_mm, npix * 2, hipMemcpyHostToDevice, s));
    if ((st = upload_calib(ctx, im, calib, 1, s)) != RVSEG_OK) return st;
    if ((st = dump_frame_features(ctx, im, s)) != RVSEG_OK) return st;
    RV_LAUNCH_OK(ctx);
    std::vector<float> dump((size_t)P * g.D);
    std::vector<uint8_t> valid((size_t)P);
    RV_HIP(ctx, hipMemcpyAsync(dump.data(), im->dump.p, dump.size() * 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipMemcpyAsync(valid.data(), im->valid.p, valid.size(), hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    // compact in the order of the reference's stride-grid scan (feature_extractor.h:56-71)
    int n = 0;
    for (int ly = 0; ly < g.lh; ly++)
        for (int lx = 0; lx < g.lw; lx++) {
            const size_t pi = (size_t)ly * g.lw + lx;
            if (!valid[pi]) continue;
            std::memcpy(feat_out + (size_t)n * g.D, dump.data() + pi * g.D, (size_t)g.D * 4);
            x_v[n] = lx * g.stride;
            y_v[n] = ly * g.stride;
            n++;
        }
    *n_points = n;
    return RVSEG_OK;
}

}  // extern "C"
