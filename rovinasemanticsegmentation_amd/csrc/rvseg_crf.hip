// CRF orchestration: the mean-field loop, the CRF stages of the frame pipeline and of the cloud path, and the C-ABI entry
// points rvseg_crf_infer* / rvseg_crf_logistic_unary*.  The lattice's host side (capacity rules, build, overflow retry,
// rvseg_lattice_*) is in rvseg_lattice.hip, the kept DenseCRF model and learning on it in rvseg_crf_model.hip;
// rvseg_crf_state.h holds what the three files share.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rvseg_crf_state.h"

namespace rvseg {

// the context's CRF state, created by the first call: the pinned counters and their event first, so that a failure
// leaves nothing behind and the next call tries again
static rvseg_status crf_state(rvseg_ctx* ctx, CrfState** out) {
    Pipeline* im = pipeline_of(ctx);
    if (!im->crf) {
        PinnedBuf h;
        Event ev;
        rvseg_status st = h.reserve(ctx, 8 * sizeof(int));
        if (st != RVSEG_OK) return st;
        RV_HIP(ctx, event_create(ev, hipEventDisableTiming));
        std::memset(h.p, 0, 8 * sizeof(int));
        im->crf = new CrfState();
        im->crf->h_counters = std::move(h);
        im->crf->counters_ev = std::move(ev);
    }
    *out = im->crf;
    return RVSEG_OK;
}

void crf_state_free(Pipeline* im) {   // the one delete of a CrfState
    delete im->crf;
    im->crf = nullptr;
}

// Layers that run side by side on two streams share the lattice's csr_nrm table: when any of them takes the unfused
// path (no fused instantiation for its class count) the table is filled on the PARENT stream before the fork, so the
// stream that did not enqueue the fill cannot read it early.
static rvseg_status csr_nrm_before_fork(rvseg_ctx* ctx, CrfState* cs, int n_layers, const int* class_counts, int iterations, hipStream_t s) {
    for (int l = 0; l < n_layers; l++)
        if (!(iterations > 0 && mf_fused_supported(class_counts[l]))) return ensure_csr_nrm(ctx, cs->lat[0], s);
    return RVSEG_OK;
}

// the Potts term of the Segmenter and of rvseg_crf_infer[_multi|_device] (pairwise.cpp:173-178): needs no compatibility table
static TermPlan potts_term(float w) {
    TermPlan t;
    t.w = w;
    return t;
}

// DenseKernel::filter (pairwise.cpp:63-80): the input scaled by the normaliser (SYMMETRIC / BEFORE), the output (SYMMETRIC / AFTER)
bool term_pre(const TermPlan& t) { return t.norm == RVSEG_NORMALIZE_SYMMETRIC || t.norm == RVSEG_NORMALIZE_BEFORE; }
bool term_post(const TermPlan& t) { return t.norm == RVSEG_NORMALIZE_SYMMETRIC || t.norm == RVSEG_NORMALIZE_AFTER; }

// the scratch of the general loop: tmp and the lattice values of the largest term
rvseg_status mf_scratch(rvseg_ctx* ctx, CrfState* cs, const MfRun& r) {
    rvseg_status st = dev_reserve(ctx, cs->scratch[r.slot].tmp, (size_t)r.n_points * r.C * 4);
    if (st != RVSEG_OK) return st;
    long long mb = 0;
    for (size_t k = 0; k < r.plan.size(); k++) mb = std::max<long long>(mb, cs->lat[k].dev.m_bound);
    return values_reserve(ctx, cs, mb, r.C, r.slot);
}

// the general loop scales by the normaliser inside the splat: per-entry copy of norm
rvseg_status mf_entry_norms(rvseg_ctx* ctx, CrfState* cs, const MfRun& r) {
    for (size_t k = 0; k < r.plan.size(); k++) {
        rvseg_status st;
        if (term_pre(r.plan[k]) && (st = ensure_csr_nrm(ctx, cs->lat[k], r.s)) != RVSEG_OK) return st;
    }
    return RVSEG_OK;
}

// Q = expAndNormalize(-U) (densecrf.cpp:120, :178-186) of the general loop (needs mf_scratch)
void mf_start(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, const ValueView& Q) {
    float* tmp = cs->scratch[r.slot].tmp.as<float>();
    if (r.timed) timer_mark(ctx, "softmax", r.s);
    if (!launch_softmax_unary(r.unary, r.unary_is_energy, r.C, r.N, Q, r.n_points, nullptr, r.s)) {
        launch_neg_unary(r.unary, r.unary_is_energy, r.C, r.N, tmp, r.n_points, r.s);
        launch_softmax(tmp, r.C, r.N, Q, r.n_points, r.s);
    }
}

// The entropy and unary parts, and -- when the caller has no blurred values at hand (tap of a step: it has) -- the
// pairwise parts of Q through a splat and blur of their own.  Q: one dense N x C matrix.
void kl_unary_parts(rvseg_ctx* ctx, const MfRun& r, const float* Q, const KlTap& tap) {
    if (r.timed) timer_mark(ctx, "kl", r.s);
    launch_kl_unary(r.unary.base, r.unary_is_energy, Q, r.C, r.n_points, tap.partials, r.s);
}
void kl_term_part(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, int k, const float* blurred, const float* Q, const KlTap& tap) {
    if (r.timed) timer_mark(ctx, "kl", r.s);
    const TermPlan& t = r.plan[k];
    launch_kl_term(cs->lat[k].dev, r.C, r.C <= 2, blurred, term_post(t), t.matrix, r.d_compat + t.off, Q, r.n_points,
                   tap.partials + (size_t)(2 + k) * KL_MAX_BLOCKS, r.s);
}

// One iteration of the general loop (densecrf.cpp:122-128, stepInference :187-201): tmp = -U, per term splat, blur and
// slice + compatibility folded into tmp, then Q = expAndNormalize(tmp).  Needs mf_scratch and mf_entry_norms.
// tap (optional): the KL parts of the incoming Q (a dense N x C matrix then).
void mf_step(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, const ValueView& Q, const KlTap* tap) {
    auto& sc = cs->scratch[r.slot];
    float* tmp = sc.tmp.as<float>();
    const int C = r.C, N = r.N;
    hipStream_t s = r.s;
    const bool seq = C <= 2;   // Permutohedral::compute dispatch, permutohedral.cpp:600-603
    auto mark = [&](const char* name) { if (r.timed) timer_mark(ctx, name, s); };
    mark("softmax");
    launch_neg_unary(r.unary, r.unary_is_energy, C, N, tmp, r.n_points, s);
    if (tap) kl_unary_parts(ctx, r, Q.base, *tap);
    for (int k = 0; k < (int)r.plan.size(); k++) {
        const LatticeBufs& b = cs->lat[k];
        const TermPlan& t = r.plan[k];
        mark("splat");
        launch_splat(b.dev, Q, C, term_pre(t) ? 1 : 0, sc.val_a.as<float>(), s, false, b.resident_on ? &b.resident : nullptr, r.slot);
        mark("blur");
        float* blurred = launch_blur(b.dev, C, seq, false, sc.val_a.as<float>(), sc.val_b.as<float>(), s);
        if (tap) kl_term_part(ctx, cs, r, k, blurred, Q.base, *tap);
        // DenseKernel::filter's output scale + the compatibility folded into tmp (pairwise.cpp:77-80, labelcompatibility.cpp:47-85);
        // which kernel: DESIGN.md section 4, "Learned models"
        mark("slice");
        if (t.uniform && term_post(t)) launch_slice(b.dev, C, seq, 2, blurred, -t.w, tmp, r.n_points, s);
        else launch_term_update(b.dev, C, seq, blurred, term_post(t), t.matrix, r.d_compat + t.off, tmp, r.n_points, s);
    }
    mark("softmax");
    // expAndNormalize(tmp1) with the row in registers where C has an instantiation (same operations, same bits)
    if (!launch_softmax_unary(ValueView{tmp, (size_t)N * C, 0}, false, C, N, Q, r.n_points, nullptr, s)) launch_softmax(tmp, C, N, Q, r.n_points, s);
}

// DenseCRF::inference (densecrf.cpp:115-131) over the terms of `plan`, term k on cs->lat[k]; d_compat: the device copy of
// the terms' compatibilities (may be null when every term is uniform with NORMALIZE_SYMMETRIC)
// `lab` (optional): where the last fused update may write the labels; *labels_done tells whether it did
// slot: which set of scratch buffers (0 / 1; two layers may run side by side on two streams);
// timed: record stage marks (only one of two concurrent loops may: the marks are a sequence on ONE stream)
static rvseg_status mean_field(rvseg_ctx* ctx, CrfState* cs, const std::vector<TermPlan>& plan, const float* d_compat,
                               const ValueView& unary, bool unary_is_energy, int C, int N, long long n_points, int iterations,
                               const ValueView& Q, hipStream_t s, const MfLabels* lab = nullptr, bool* labels_done = nullptr,
                               int slot = 0, bool timed = true) {
    if (labels_done) *labels_done = false;
    rvseg_status st;
    const int n_terms = (int)plan.size();
    DevBuf &b_qn = cs->scratch[slot].qn, &b_va = cs->scratch[slot].val_a, &b_vb = cs->scratch[slot].val_b;
    auto mark = [&](const char* name) { if (timed) timer_mark(ctx, name, s); };
    auto pre = [&](int k) { return term_pre(plan[k]); };
    auto post = [&](int k) { return term_post(plan[k]); };
    const MfRun run{plan, d_compat, unary, unary_is_energy, C, N, n_points, s, slot, timed};
    if ((st = mf_scratch(ctx, cs, run)) != RVSEG_OK) return st;
    const bool seq = C <= 2;   // Permutohedral::compute dispatch, permutohedral.cpp:600-603
    if (n_terms == 1 && iterations > 0 && mf_fused_supported(C)) {
        // Single term with a fused instantiation: splat, blur, then one fused slice + update + softmax pass.  When the
        // term pre-scales, Q holds fl(Q * norm) between iterations, the input of the next splat (pairwise.cpp:66), so
        // the splat is a plain gather; only the last update stores the marginals themselves.
        const LatticeBufs& b = cs->lat[0];
        const TermPlan& t = plan[0];
        // Where the fused loop keeps Q between iterations: Q itself when that is one contiguous
        // [point][C] matrix, else (a layer inside the reference's [layer][y][x][class] frames) a contiguous scratch
        // matrix -- the splat then addresses a row as point * C without splitting the point index per frame, and
        // its gathers stay inside one array.  The last update writes the marginals into Q in either case.
        ValueView Qs = Q;
        if (!(Q.frame_stride == (size_t)N * (size_t)C && Q.layer_off == 0)) {
            if ((st = dev_reserve(ctx, b_qn, (size_t)n_points * C * 4)) != RVSEG_OK) return st;
            Qs = ValueView{b_qn.as<float>(), (size_t)N * (size_t)C, 0};
        }
        const bool potts = t.uniform && t.norm == RVSEG_NORMALIZE_SYMMETRIC;
        const MfTerm term{-t.w, potts ? nullptr : d_compat + t.off, t.matrix, post(0)};
        const MfLabels none{nullptr, 0, 0, 0, 0};
        mark("softmax");
        launch_softmax_unary(unary, unary_is_energy, C, N, Qs, n_points, pre(0) ? b.dev.norm : nullptr, s);
        for (int it = 0; it < iterations; it++) {
            const bool last = it + 1 == iterations;
            mark("splat");
            launch_splat(b.dev, Qs, C, 0, b_va.as<float>(), s, true, b.resident_on ? &b.resident : nullptr, slot);
            mark("blur");
            float* blurred = launch_blur(b.dev, C, seq, false, b_va.as<float>(), b_vb.as<float>(), s);
            mark("mf_update");
            launch_mf_update(b.dev, C, blurred, term, unary, unary_is_energy, last ? Q : Qs, !last && pre(0), last && lab ? *lab : none, s);
        }
        if (lab && labels_done) *labels_done = true;
        RV_LAUNCH_OK(ctx);
        return RVSEG_OK;
    }
    // The general loop: several terms, or a class count without a fused update.
    mf_start(ctx, cs, run, Q);
    if ((st = mf_entry_norms(ctx, cs, run)) != RVSEG_OK) return st;
    for (int it = 0; it < iterations; it++) mf_step(ctx, cs, run, Q);
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// PottsCompatibility / DiagonalCompatibility / MatrixCompatibility (labelcompatibility.cpp:38-100) as diagonals and
// symmetric matrices: W = 0.5 * (m + m^T) elementwise in fp32 when the term is created (:79)
void plan_compat(int C, int compat, const float* params, TermPlan& tp, float* hc /* C, or C x C for a Matrix */) {
    tp.compat = compat;
    tp.uniform = true;
    tp.matrix = false;
    tp.w = 0.f;
    if (compat == RVSEG_COMPAT_MATRIX) {
        tp.uniform = false;
        tp.matrix = true;
        for (int i = 0; i < C; i++)
            for (int j = 0; j < C; j++) {
                const float sum = params[(size_t)i * C + j] + params[(size_t)j * C + i];
                hc[(size_t)i * C + j] = 0.5f * sum;
            }
    } else if (compat == RVSEG_COMPAT_DIAGONAL) {
        for (int c = 0; c < C; c++) {
            hc[c] = params[c];
            if (!(params[c] == params[0] && std::signbit(params[c]) == std::signbit(params[0]))) tp.uniform = false;
        }
        tp.w = -params[0];
    } else {
        tp.w = params[0];
        for (int c = 0; c < C; c++) hc[c] = -tp.w;
    }
}

static void plan_terms(int C, int n_terms, const rvseg_crf_term* terms, std::vector<TermPlan>& plan, std::vector<float>& hc) {
    plan.assign((size_t)n_terms, TermPlan{});
    hc.clear();
    for (int k = 0; k < n_terms; k++) {
        const rvseg_crf_term& t = terms[k];
        TermPlan& tp = plan[k];
        tp.norm = t.normalization;
        tp.off = hc.size();
        hc.resize(hc.size() + (t.compat == RVSEG_COMPAT_MATRIX ? (size_t)C * C : (size_t)C));
        plan_compat(C, t.compat, t.compat_params, tp, hc.data() + tp.off);
    }
}

// The label layers of one lattice are independent mean fields (the reference runs one DenseCRF per layer,
// segmenter.cpp:639-644).  Their splats wait for their longest chains rather than for bandwidth whenever a chunk
// has few frames (a cloud, a 1280x960 chunk), so odd layers run on a second stream beside the even ones.
// li-th layer to enqueue: odd layers (second stream) first when the layers run on two streams
static int layer_enqueue_order(int li, int n_layers, bool two_streams) {
    if (!two_streams) return li;
    const int n_odd = n_layers / 2;
    return li < n_odd ? 2 * li + 1 : 2 * (li - n_odd);
}

static rvseg_status layer_stream_fork(rvseg_ctx* ctx, CrfState* cs, hipStream_t s, int n_layers, hipStream_t* s2) {
    *s2 = s;
    if (n_layers < 2 || !ctx->sched.overlap_layers) return RVSEG_OK;
    rvseg_status st = second_stream(ctx, cs);
    if (st != RVSEG_OK) return st;
    RV_HIP(ctx, hipEventRecord(cs->layer_fork, s));
    RV_HIP(ctx, hipStreamWaitEvent(cs->layer_stream, cs->layer_fork, 0));
    *s2 = cs->layer_stream;
    return RVSEG_OK;
}

static rvseg_status layer_stream_join(rvseg_ctx* ctx, CrfState* cs, hipStream_t s, hipStream_t s2) {
    if (s2 == s) return RVSEG_OK;
    RV_HIP(ctx, hipEventRecord(cs->layer_join, s2));
    RV_HIP(ctx, hipStreamWaitEvent(s, cs->layer_join, 0));
    return RVSEG_OK;
}

// ---------------------------------------------------------------------------------------------
// per-frame CRF stage of the frame pipeline
// ---------------------------------------------------------------------------------------------
rvseg_status crf_frames_status(rvseg_ctx* ctx, Pipeline* im, bool wait) {
    CrfState* cs = im->crf;
    if (!cs || !cs->counters_pending) return RVSEG_OK;
    if (wait) {
        RV_HIP(ctx, hipEventSynchronize(cs->counters_ev));
    } else {
        const hipError_t e = hipEventQuery(cs->counters_ev);
        if (e == hipErrorNotReady) return RVSEG_NOT_READY;
        RV_HIP(ctx, e);
    }
    cs->counters_pending = false;
    const int* h = cs->h_counters.as<int>();
    if (cs->pending_frames > 0 && !h[1]) cs->frame_vertices_seen = h[0] / cs->pending_frames;
    if (cs->info_async) counters_to_info(cs, h);   // no other lattice has been built on this context since
    if (h[1]) return lattice_raise_capacity(ctx, im, im->geom.W * im->geom.H);
    return RVSEG_OK;
}

// First half of crf_frames_build: status of the previous build, buffers, and the memsets of the new one.  None of it
// needs the frames' cloud, so the frame path enqueues it on the build stream BEFORE that stream waits for prep_kernel
// (40 us of a single frame's 2 ms).  `s` must already be ordered behind the previous user of the lattice.
rvseg_status crf_frames_build_begin(rvseg_ctx* ctx, Pipeline* im, int n, hipStream_t s) {
    CrfState* cs;
    rvseg_status st = crf_state(ctx, &cs);
    if (st != RVSEG_OK) return st;
    const FrameGeom& g = im->geom;
    const int N = g.W * g.H;
    // status of the previous asynchronous build (an earlier chunk of this call, or an earlier call whose
    // status nobody polled): its outputs were invalid, so this call must not pass for a clean one
    if ((st = crf_frames_status(ctx, im, true)) != RVSEG_OK) return st;
    cs->entry = "a frame segmentation call (rvseg_segment_frames / rvseg_segment_external)";
    LatticeBufs& lb = lattice_at(cs, 0);
    if ((st = lattice_prepare(ctx, lb, 6, N, n, false, cs->frame_vertices_seen, true)) != RVSEG_OK) return st;
    return lattice_clear(ctx, lb, s);
}

rvseg_status crf_frames_build(rvseg_ctx* ctx, Pipeline* im, int n, const uint8_t* d_rgb, hipStream_t s) {
    CrfState* cs;
    rvseg_status st = crf_state(ctx, &cs);
    if (st != RVSEG_OK) return st;
    const rvseg_params& p = ctx->params;
    if (cs->lat.size() < 1 || !cs->lat[0].cleared) {
        if ((st = crf_frames_build_begin(ctx, im, n, s)) != RVSEG_OK) return st;
    }
    LatticeBufs& lb = cs->lat[0];
    FeatureSource fs{};
    fs.mode = 1; fs.cloud = im->cloud.as<float4>(); fs.rgb = d_rgb;
    fs.xyz_kernel = p.dcrf_xyz_kernel; fs.rgb_kernel = p.dcrf_rgb_kernel;
    if ((st = lattice_build(ctx, cs, lb, fs, s)) != RVSEG_OK) return st;
    if ((st = counters_readback(ctx, cs, lb, 0, s)) != RVSEG_OK) return st;
    RV_HIP(ctx, hipEventRecord(cs->counters_ev, s));
    cs->counters_pending = true;
    cs->pending_frames = n;
    cs->info_async = true;
    return RVSEG_OK;
}

// What the mean field of one label layer reads and writes.  lab.labels == nullptr: no labels wanted; label_here: labels
// that the fused update did not write are taken from Q (one dense N x C matrix) right behind the layer's loop
struct LayerIo { ValueView U, Q; MfLabels lab; bool label_here; };

// The mean fields of the label layers of cs->lat[0], layer l on scratch slot l & 1 and, with two streams, odd layers on
// the second one.  `layer(l, prefix, slot)` gives the LayerIo of layer l, whose classes start at `prefix`: an inlined
// functor, because enqueuing a layer must not allocate (see below).  *all_labelled: every layer's labels are written.
template <class Layer>
static rvseg_status crf_layers(rvseg_ctx* ctx, CrfState* cs, int n_layers, const int* class_counts, int N, long long n_points, float potts_w,
                               int iterations, hipStream_t s, const Layer& layer, bool* all_labelled) {
    const std::vector<TermPlan> plan{potts_term(potts_w)};
    *all_labelled = true;
    hipStream_t s2;
    rvseg_status st = csr_nrm_before_fork(ctx, cs, n_layers, class_counts, iterations, s);
    if (st != RVSEG_OK) return st;
    if ((st = layer_stream_fork(ctx, cs, s, n_layers, &s2)) != RVSEG_OK) return st;
    // With two streams the layers of the SECOND stream are enqueued first: enqueuing a layer's whole loop takes the host
    // a few hundred microseconds, during which the other stream has nothing to run, and the reference's second layer
    // is the one with more classes (8 and 9: the longer loop starts first)
    for (int li = 0; li < n_layers && st == RVSEG_OK; li++) {
        const int l = layer_enqueue_order(li, n_layers, s2 != s);
        size_t prefix = 0;
        for (int k = 0; k < l; k++) prefix += (size_t)class_counts[k];
        const int C = class_counts[l], slot = l & 1;
        hipStream_t sl = slot ? s2 : s;
        const bool timed = slot == 0 || s2 == s;
        const LayerIo io = layer(l, prefix, slot);
        bool done = false;
        st = mean_field(ctx, cs, plan, nullptr, io.U, false, C, N, n_points, iterations, io.Q, sl, io.lab.labels ? &io.lab : nullptr, &done, slot, timed);
        if (st == RVSEG_OK && io.lab.labels && !done && io.label_here) {
            if (timed) timer_mark(ctx, "labels", sl);
            launch_labels(io.Q.base, (size_t)N, C, io.lab.mode, io.lab.unknown, io.lab.labels, sl);
            done = true;
        }
        *all_labelled = *all_labelled && done;
    }
    const rvseg_status stj = layer_stream_join(ctx, cs, s, s2);   // (also behind a failed layer: the second stream rejoins)
    return st != RVSEG_OK ? st : stj;
}

rvseg_status crf_frames_infer(rvseg_ctx* ctx, Pipeline* im, const LayerLayout& f, int n, const float* d_post, float* d_marg,
                              int8_t* d_labels, hipStream_t s) {
    CrfState* cs;
    rvseg_status st = crf_state(ctx, &cs);
    if (st != RVSEG_OK) return st;
    const rvseg_params& p = ctx->params;
    const int N = im->geom.W * im->geom.H;
    const size_t frame_stride = (size_t)N * f.sum_classes;
    float* marg = d_marg;
    if (!marg) {
        if ((st = dev_reserve(ctx, cs->q, frame_stride * 4 * n)) != RVSEG_OK) return st;
        marg = cs->q.as<float>();
    }
    // a layer inside the frames' posteriors and marginals; unary energy = -(log-posterior) (segmenter.cpp:642), so -U is the posterior
    auto layer = [&](int l, size_t prefix, int) {
        return LayerIo{ValueView{const_cast<float*>(d_post), frame_stride, (size_t)N * prefix}, ValueView{marg, frame_stride, (size_t)N * prefix},
                       MfLabels{d_labels, p.label_mode, p.unknown_label[l], f.n_layers, l}, false};
    };
    bool all_labelled;   // the last fused update of every layer wrote its labels
    if ((st = crf_layers(ctx, cs, f.n_layers, f.class_counts, N, (long long)N * n, p.dcrf_kernel_weight, p.dcrf_iterations, s, layer,
                         &all_labelled)) != RVSEG_OK) return st;
    if (d_labels && !all_labelled) {
        timer_mark(ctx, "labels", s);
        launch_labels_frames(marg, n, N, f, p.label_mode, p.unknown_label, d_labels, s);
    }
    return RVSEG_OK;
}

// rvseg_crf_model_set_kernel: term k of the live model rebuilt on cs->lat[k] from the raw features the model keeps, with new
// kernel parameters (host; null: none) -- lattice, normaliser, point ranks and, where the term had one, the per-entry
// normaliser.  A hash overflow rebuilds this term once at the safe capacity (build_lattices).  No other lattice is touched.
rvseg_status term_rebuild(rvseg_ctx* ctx, CrfState* cs, int k, const float* kernel_params, hipStream_t s) {
    CrfModel& m = cs->model;
    const TermPlan& tp = m.plan[k];
    const bool entry_norms = cs->lat[k].has_csr_nrm;
    const TermInput in{tp.d, m.keep[k].feat.as<float>(), false, tp.kernel, kernel_params, tp.norm, &m.keep[k], true};
    const rvseg_status st = build_lattices(ctx, cs, m.N, 1, &in, s, k);
    if (st != RVSEG_OK) { model_replaced(cs); return st; }   // (a lattice half built: the model is gone)
    return entry_norms ? ensure_csr_nrm(ctx, cs->lat[k], s) : RVSEG_OK;
}

// Where a point CRF's unary comes from and where its marginals and labels go.  on_host: caller host memory, staged
// through cs->unary / cs->q / cs->labels, and the call returns with the outputs complete.  Otherwise device memory, read
// and written in place on the caller's stream (Q or map may be null), and the call only enqueues.
struct PointIo { bool on_host; const float* unary; bool unary_is_energy; float* Q; int8_t* map; };

// DenseCRF::inference + map over the lattices cs->lat[0 .. plan.size()) (build_lattices).  Stage timing: a host call
// shows the mean field alone (its labels follow "end"); a device call adds to what its entry has marked, labels included.
static rvseg_status crf_points(rvseg_ctx* ctx, CrfState* cs, int N, int C, const std::vector<TermPlan>& plan, const float* d_compat,
                               const PointIo& io, int iterations, int label_mode, int unknown_label, hipStream_t s) {
    rvseg_status st;
    const size_t tot = (size_t)N * C;
    const float* u = io.unary;
    float* q = io.Q;
    if (io.on_host || !q) {
        if ((st = dev_reserve(ctx, cs->q, tot * 4)) != RVSEG_OK) return st;
        q = cs->q.as<float>();
    }
    if (io.on_host) {
        if ((st = dev_reserve(ctx, cs->unary, tot * 4)) != RVSEG_OK) return st;
        RV_HIP(ctx, hipMemcpyAsync(cs->unary.p, io.unary, tot * 4, hipMemcpyHostToDevice, s));
        u = cs->unary.as<float>();
        timer_reset(ctx);
    }
    const ValueView U{const_cast<float*>(u), tot, 0}, Q{q, tot, 0};
    // a device call lets the last fused update write the labels; a host call labels the marginals it downloads
    const MfLabels lab{io.map, label_mode, unknown_label, 1, 0};
    bool done = false;
    if ((st = mean_field(ctx, cs, plan, d_compat, U, io.unary_is_energy, C, N, N, iterations, Q, s, !io.on_host && io.map ? &lab : nullptr,
                         &done)) != RVSEG_OK) return st;
    int8_t* d_map = io.map;
    if (io.on_host) {
        timer_mark(ctx, "end", s);
        RV_HIP(ctx, hipMemcpyAsync(io.Q, q, tot * 4, hipMemcpyDeviceToHost, s));
        if (io.map && (st = dev_reserve(ctx, cs->labels, (size_t)N)) != RVSEG_OK) return st;
        d_map = cs->labels.as<int8_t>();
    }
    if (io.map && !done) {
        if (!io.on_host) timer_mark(ctx, "labels", s);
        launch_labels(q, (size_t)N, C, label_mode, unknown_label, d_map, s);
    }
    if (!io.on_host) {
        timer_mark(ctx, "end", s);
        RV_LAUNCH_OK(ctx);
        return RVSEG_OK;
    }
    if (io.map) RV_HIP(ctx, hipMemcpyAsync(io.map, d_map, (size_t)N, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    return RVSEG_OK;
}

rvseg_status crf_cloud_layers(rvseg_ctx* ctx, int N, int n_layers, const int* class_counts, const float* d_unaries,
                              const float* d_features, float potts_w, int iterations, int label_mode, const int* unknown,
                              int8_t* d_labels, hipStream_t s) {
    CrfState* cs;
    rvseg_status st = crf_state(ctx, &cs);
    if (st != RVSEG_OK) return st;
    cs->entry = "a local-map call (rvseg_process_map_device / rvseg_process_map_poses_device)";
    timer_mark(ctx, "lattice_build", s);
    const TermInput cloud = potts_input(6, d_features, false);
    if ((st = build_lattices(ctx, cs, N, 1, &cloud, s)) != RVSEG_OK) return st;
    int cmax = 0;
    for (int l = 0; l < n_layers; l++) cmax = std::max(cmax, class_counts[l]);
    // marginals of even / odd layers in two halves of cs->q (the odd layers run on the second stream)
    if ((st = dev_reserve(ctx, cs->q, (size_t)N * cmax * 4 * 2)) != RVSEG_OK) return st;
    // crf.setUnaryEnergy(-unaries[l]) (segmenter.cpp:642): the accumulated posteriors ARE -energy
    auto layer = [&](int l, size_t prefix, int slot) {
        const size_t tot = (size_t)N * class_counts[l];
        return LayerIo{ValueView{const_cast<float*>(d_unaries) + (size_t)N * prefix, tot, 0},
                       ValueView{cs->q.as<float>() + (size_t)slot * N * cmax, tot, 0},
                       MfLabels{d_labels ? d_labels + (size_t)l * N : nullptr, label_mode, unknown[l], 1, 0}, true};
    };
    bool all_labelled;
    if ((st = crf_layers(ctx, cs, n_layers, class_counts, N, N, potts_w, iterations, s, layer, &all_labelled)) != RVSEG_OK) return st;
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// entry of the C-ABI CRF calls: selects the device; they do not need the frame tables (a bare pipeline will do)
// (`entry`: its name, which a kept model that it replaces reports)
rvseg_status crf_enter(rvseg_ctx* ctx, CrfState** cs_out, const char* entry) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    const rvseg_status st = crf_state(ctx, cs_out);
    if (st == RVSEG_OK) (*cs_out)->entry = entry;
    return st;
}

// A learned model's terms (arguments checked by the caller): their plan, their compatibilities in context memory
// (uploaded from CrfState::h_compat, which outlives the copy; also for Potts terms, which do not read them) and their lattices
rvseg_status terms_prepare(rvseg_ctx* ctx, CrfState* cs, int N, int C, int n_terms, const rvseg_crf_term* terms, bool on_host,
                           std::vector<TermPlan>& plan, hipStream_t s, TermKeep* keep) {
    plan_terms(C, n_terms, terms, plan, cs->h_compat);
    for (int k = 0; k < n_terms; k++) { plan[k].kernel = terms[k].kernel_type; plan[k].d = terms[k].d; }
    if (!cs->h_compat.empty()) {
        rvseg_status st = dev_reserve(ctx, cs->compat, cs->h_compat.size() * 4);
        if (st != RVSEG_OK) return st;
        RV_HIP(ctx, hipMemcpyAsync(cs->compat.p, cs->h_compat.data(), cs->h_compat.size() * 4, hipMemcpyHostToDevice, s));
    }
    TermInput in[8];
    for (int k = 0; k < n_terms; k++)
        in[k] = TermInput{terms[k].d, terms[k].features, on_host, terms[k].kernel_type, terms[k].kernel_params, terms[k].normalization,
                          keep ? keep + k : nullptr};
    const rvseg_status st = build_lattices(ctx, cs, N, n_terms, in, s);
    for (int k = 0; keep && st == RVSEG_OK && k < n_terms; k++) {   // what term_rebuild's callers compare new parameters with
        const int np = terms[k].kernel_type == RVSEG_DIAG_KERNEL ? terms[k].d : terms[k].kernel_type == RVSEG_FULL_KERNEL ? terms[k].d * terms[k].d : 0;
        keep[k].has_kparams = np > 0 && terms[k].kernel_params;
        keep[k].kparams.assign(terms[k].kernel_params, terms[k].kernel_params + (keep[k].has_kparams ? np : 0));
    }
    return st;
}

}  // namespace rvseg

using namespace rvseg;

extern "C" {

rvseg_status rvseg_crf_infer_multi(rvseg_ctx* ctx, int32_t N, int32_t C, int32_t n_kernels, const int32_t* ds,
                                   const float* const* features, const float* ws, const float* unary_energy,
                                   int32_t iterations, float* Q_out, int8_t* map_out, int32_t label_mode, int32_t unknown_label) {
    CrfState* cs;
    rvseg_status st = crf_enter(ctx, &cs, __func__);
    if (st != RVSEG_OK) return st;
    if (N <= 0 || C <= 0 || C > 64 || n_kernels < 0 || n_kernels > 8 || iterations < 0 || !unary_energy || !Q_out ||
        (n_kernels > 0 && (!ds || !features || !ws)) || label_mode < 0 || label_mode > 3) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    TermInput in[8];
    std::vector<TermPlan> plan;
    for (int k = 0; k < n_kernels; k++) {
        in[k] = potts_input(ds[k], features[k], true);   // (a bad ds[k] is the build's to report)
        plan.push_back(potts_term(ws[k]));
    }
    if ((st = build_lattices(ctx, cs, N, n_kernels, in, ctx->stream)) != RVSEG_OK) return st;
    return crf_points(ctx, cs, N, C, plan, nullptr, PointIo{true, unary_energy, true, Q_out, map_out}, iterations, label_mode, unknown_label,
                      ctx->stream);
}

rvseg_status rvseg_crf_terms_check(int32_t N, int32_t C, int32_t n_terms, const rvseg_crf_term* terms) {
    if (N <= 0 || C < 1 || C > 64 || n_terms < 0 || n_terms > 8 || (n_terms > 0 && !terms)) return RVSEG_ERR_INVALID_ARG;
    for (int k = 0; k < n_terms; k++) {
        const rvseg_crf_term& t = terms[k];
        if (t.d < 1 || t.d > 7 || !t.features || !t.compat_params) return RVSEG_ERR_INVALID_ARG;
        if (t.compat < RVSEG_COMPAT_POTTS || t.compat > RVSEG_COMPAT_MATRIX) return RVSEG_ERR_INVALID_ARG;
        if (t.kernel_type < RVSEG_CONST_KERNEL || t.kernel_type > RVSEG_FULL_KERNEL) return RVSEG_ERR_INVALID_ARG;
        if (t.normalization < RVSEG_NO_NORMALIZATION || t.normalization > RVSEG_NORMALIZE_SYMMETRIC) return RVSEG_ERR_INVALID_ARG;
    }
    return RVSEG_OK;
}

rvseg_status rvseg_crf_infer_terms(rvseg_ctx* ctx, int32_t N, int32_t C, int32_t n_terms, const rvseg_crf_term* terms,
                                   const float* unary_energy, int32_t iterations, float* Q_out, int8_t* map_out,
                                   int32_t label_mode, int32_t unknown_label) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (rvseg_crf_terms_check(N, C, n_terms, terms) != RVSEG_OK || iterations < 0 || !unary_energy || !Q_out || label_mode < 0 ||
        label_mode > 3) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    CrfState* cs;
    rvseg_status st = crf_enter(ctx, &cs, __func__);
    if (st != RVSEG_OK) return st;
    std::vector<TermPlan> plan;
    if ((st = terms_prepare(ctx, cs, N, C, n_terms, terms, true, plan, ctx->stream)) != RVSEG_OK) return st;
    return crf_points(ctx, cs, N, C, plan, cs->compat.as<float>(), PointIo{true, unary_energy, true, Q_out, map_out}, iterations, label_mode,
                      unknown_label, ctx->stream);
}

rvseg_status rvseg_crf_infer_terms_device(rvseg_ctx* ctx, int32_t N, int32_t C, int32_t n_terms, const rvseg_crf_term* terms,
                                          const float* d_unary, int32_t unary_is_energy, int32_t iterations, float* d_Q_out,
                                          int8_t* d_map_out, int32_t label_mode, int32_t unknown_label, void* hip_stream) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (rvseg_crf_terms_check(N, C, n_terms, terms) != RVSEG_OK || iterations < 0 || !d_unary || (!d_Q_out && !d_map_out) ||
        label_mode < 0 || label_mode > 3) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    CrfState* cs;
    rvseg_status st = crf_enter(ctx, &cs, __func__);
    if (st != RVSEG_OK) return st;
    hipStream_t s = stream_of(ctx, hip_stream);
    timer_reset(ctx);
    timer_mark(ctx, "lattice_build", s);
    std::vector<TermPlan> plan;
    if ((st = terms_prepare(ctx, cs, N, C, n_terms, terms, false, plan, s)) != RVSEG_OK) return st;
    return crf_points(ctx, cs, N, C, plan, cs->compat.as<float>(), PointIo{false, d_unary, unary_is_energy != 0, d_Q_out, d_map_out}, iterations,
                      label_mode, unknown_label, s);
}

static rvseg_status logistic_args(rvseg_ctx* ctx, int32_t N, int32_t C, int32_t K, const float* L, const float* f, const float* U) {
    if (N <= 0 || C < 1 || C > 64 || K < 1 || !L || !f || !U) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    return RVSEG_OK;
}

rvseg_status rvseg_crf_logistic_unary(rvseg_ctx* ctx, int32_t N, int32_t C, int32_t K, const float* L, const float* f, float* U_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    rvseg_status st = logistic_args(ctx, N, C, K, L, f, U_out);
    if (st != RVSEG_OK) return st;
    CrfState* cs;
    if ((st = crf_enter(ctx, &cs, __func__)) != RVSEG_OK) return st;
    hipStream_t s = ctx->stream;
    if ((st = dev_reserve(ctx, cs->lmat, (size_t)C * K * 4)) != RVSEG_OK) return st;
    if ((st = dev_reserve(ctx, cs->feat, (size_t)N * K * 4)) != RVSEG_OK) return st;
    if ((st = dev_reserve(ctx, cs->unary, (size_t)N * C * 4)) != RVSEG_OK) return st;
    RV_HIP(ctx, hipMemcpyAsync(cs->lmat.p, L, (size_t)C * K * 4, hipMemcpyHostToDevice, s));
    RV_HIP(ctx, hipMemcpyAsync(cs->feat.p, f, (size_t)N * K * 4, hipMemcpyHostToDevice, s));
    launch_logistic_unary(cs->lmat.as<float>(), cs->feat.as<float>(), N, C, K, cs->unary.as<float>(), s);
    RV_LAUNCH_OK(ctx);
    RV_HIP(ctx, hipMemcpyAsync(U_out, cs->unary.p, (size_t)N * C * 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    return RVSEG_OK;
}

rvseg_status rvseg_crf_logistic_unary_device(rvseg_ctx* ctx, int32_t N, int32_t C, int32_t K, const float* L, const float* d_f,
                                             float* d_U_out, void* hip_stream) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    rvseg_status st = logistic_args(ctx, N, C, K, L, d_f, d_U_out);
    if (st != RVSEG_OK) return st;
    CrfState* cs;
    if ((st = crf_enter(ctx, &cs, __func__)) != RVSEG_OK) return st;
    hipStream_t s = stream_of(ctx, hip_stream);
    if ((st = dev_reserve(ctx, cs->lmat, (size_t)C * K * 4)) != RVSEG_OK) return st;
    // L is caller memory that may be gone once this returns: its copy is complete before the call returns
    RV_HIP(ctx, hipMemcpyAsync(cs->lmat.p, L, (size_t)C * K * 4, hipMemcpyHostToDevice, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    launch_logistic_unary(cs->lmat.as<float>(), d_f, N, C, K, d_U_out, s);
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

rvseg_status rvseg_crf_infer_device(rvseg_ctx* ctx, int32_t N, int32_t C, int32_t d, const float* d_unary, int32_t unary_is_energy,
                                    const float* d_features, float potts_w, int32_t iterations, float* d_Q_out, int8_t* d_map_out,
                                    int32_t label_mode, int32_t unknown_label, void* hip_stream) {
    CrfState* cs;
    rvseg_status st = crf_enter(ctx, &cs, __func__);
    if (st != RVSEG_OK) return st;
    if (N <= 0 || C <= 0 || C > 64 || d < 1 || d > 7 || iterations < 0 || !d_unary || !d_features || (!d_Q_out && !d_map_out) ||
        label_mode < 0 || label_mode > 3) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    hipStream_t s = stream_of(ctx, hip_stream);
    timer_reset(ctx);
    timer_mark(ctx, "lattice_build", s);
    const TermInput in = potts_input(d, d_features, false);
    if ((st = build_lattices(ctx, cs, N, 1, &in, s)) != RVSEG_OK) return st;
    const std::vector<TermPlan> plan{potts_term(potts_w)};
    return crf_points(ctx, cs, N, C, plan, nullptr, PointIo{false, d_unary, unary_is_energy != 0, d_Q_out, d_map_out}, iterations, label_mode,
                      unknown_label, s);
}

rvseg_status rvseg_crf_infer(rvseg_ctx* ctx, int32_t N, int32_t C, int32_t d, const float* unary_energy,
                             const float* features, float potts_w, int32_t iterations, float* Q_out, int8_t* map_out,
                             int32_t label_mode, int32_t unknown_label) {
    const float* feats[1] = {features};
    return rvseg_crf_infer_multi(ctx, N, C, 1, &d, feats, &potts_w, unary_energy, iterations, Q_out, map_out, label_mode, unknown_label);
}

}  // extern "C"
