// A kept DenseCRF model (rvseg_crf_model_*) and learning on it: the state of the context, valid until its next lattice
// build.  Each call has one body on device pointers (model_*_on) and one entry body (arguments, staging); a ModelIo
// tells the entry body whether it serves the host entry or the _device entry.
#include <algorithm>
#include <atomic>
#include <cassert>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rvseg_crf_state.h"

using namespace rvseg;

#define RV_TRY(call) do { const rvseg_status st_ = (call); if (st_ != RVSEG_OK) return st_; } while (0)
#define RV_MODEL_ARGS(ok) do { if (!(ok)) { io.ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; } } while (0)

// How the arrays of an entry reach the device (what PointIo is to crf_points).  on_host: caller host memory, staged through
// buffers of the context on ctx->stream; the call returns with its outputs complete and records no stage marks.
// Otherwise device memory, used in place on the caller's stream, and the call only enqueues.  in() and out() turn an
// entry's pointer argument into the pointer its kernels use (a null pointer stays null).
namespace {
// what a model call answers without a live model
rvseg_status no_model(rvseg_ctx* ctx, const CrfModel* m) {
    ctx->err = !m || m->replaced_by.empty() ? std::string("no DenseCRF model on this context (rvseg_crf_model_set has not succeeded)")
                                            : "the DenseCRF model of this context was replaced by " + m->replaced_by + ": call rvseg_crf_model_set again";
    return RVSEG_ERR_INVALID_ARG;
}

struct ModelIo {
    rvseg_ctx* ctx;
    bool on_host;
    void* hip_stream;      // of a device entry (null: the context's own)
    const char* entry;     // the public entry's name
    CrfState* cs = nullptr;    // (enter)
    hipStream_t s = nullptr;   // (enter)
    bool timed = false;        // a device entry that records stage marks (time)
    static constexpr int MAX_HOME = 6;
    struct { void* host; const void* dev; size_t bytes; } home[MAX_HOME];   // the downloads of a host entry, in order (done)
    int n_home = 0;

    // the entry's first step: the device, the CRF state and (need_model) its live model, the stream
    rvseg_status enter(bool need_model = true) {
        RV_TRY(crf_enter(ctx, &cs, entry));   // (refuses a null ctx)
        s = on_host ? (hipStream_t)ctx->stream : stream_of(ctx, hip_stream);
        return !need_model || cs->model.valid ? RVSEG_OK : no_model(ctx, &cs->model);
    }
    // the n elements of *p copied into `stage`
    template <class T> rvseg_status in(DevBuf& stage, T** p, size_t n) {
        if (!on_host || !*p) return RVSEG_OK;
        RV_TRY(dev_reserve(ctx, stage, n * sizeof(T)));
        RV_HIP(ctx, hipMemcpyAsync(stage.p, *p, n * sizeof(T), hipMemcpyHostToDevice, s));
        *p = stage.as<T>();
        return RVSEG_OK;
    }
    // the n elements of *p written into `stage` and downloaded by done()
    template <class T> rvseg_status out(DevBuf& stage, T** p, size_t n) {
        if (!on_host || !*p) return RVSEG_OK;
        RV_TRY(dev_reserve(ctx, stage, std::max<size_t>(1, n * sizeof(T))));
        out_at(stage.as<T>(), p, n);
        return RVSEG_OK;
    }
    // the same from device memory `d` that out() did not reserve (at most MAX_HOME downloads per call)
    template <class T> void out_at(T* d, T** p, size_t n) {
        if (!on_host || !*p) return;
        assert(n == 0 || n_home < MAX_HOME);
        if (n) home[n_home++] = {*p, d, n * sizeof(T)};
        *p = d;
    }
    // start, step, kl, trace and gradient record stage marks when they are device entries
    bool time() {
        timed = !on_host;
        if (timed) timer_reset(ctx);
        return timed;
    }
    rvseg_status done() {
        if (timed) timer_mark(ctx, "end", s);
        if (!on_host) return RVSEG_OK;
        for (int i = 0; i < n_home; i++) RV_HIP(ctx, hipMemcpyAsync(home[i].host, home[i].dev, home[i].bytes, hipMemcpyDeviceToHost, s));
        RV_HIP(ctx, hipStreamSynchronize(s));
        return RVSEG_OK;
    }
};
}  // namespace

static ModelIo host_io(rvseg_ctx* ctx, const char* entry) { return ModelIo{ctx, true, nullptr, entry}; }
static ModelIo device_io(rvseg_ctx* ctx, void* hip_stream, const char* entry) { return ModelIo{ctx, false, hip_stream, entry}; }

static MfRun model_run(CrfState* cs, hipStream_t s, bool timed) {
    CrfModel& m = cs->model;
    return MfRun{m.plan, cs->compat.as<float>(), ValueView{m.unary.as<float>(), (size_t)m.N * m.C, 0}, m.unary_is_energy, m.C, m.N, m.N, s, 0, timed};
}

static ValueView model_view(const CrfModel& m, const float* q) { return ValueView{const_cast<float*>(q), (size_t)m.N * m.C, 0}; }

static rvseg_status model_set(ModelIo io, int32_t N, int32_t C, int32_t n_terms, const rvseg_crf_term* terms, const float* unary,
                              int32_t unary_is_energy) {
    rvseg_ctx* ctx = io.ctx;
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    RV_MODEL_ARGS(rvseg_crf_terms_check(N, C, n_terms, terms) == RVSEG_OK && unary);
    RV_TRY(io.enter(false));
    CrfModel& m = io.cs->model;
    model_replaced(io.cs);   // (also a model of no terms, which builds no lattice; a failure below leaves no model)
    m.replaced_by = io.entry;
    const size_t tot = (size_t)N * C;
    RV_TRY(dev_reserve(ctx, m.unary, tot * 4));
    RV_HIP(ctx, hipMemcpyAsync(m.unary.p, unary, tot * 4, io.on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, io.s));
    RV_TRY(terms_prepare(ctx, io.cs, N, C, n_terms, terms, io.on_host, m.plan, io.s, m.keep));
    // every lattice build has waited for the stream; a model without terms waits here: the caller's buffers are free
    if (n_terms == 0) RV_HIP(ctx, hipStreamSynchronize(io.s));
    m.N = N; m.C = C; m.unary_is_energy = unary_is_energy != 0;
    m.K = 0;
    static std::atomic<uint64_t> next_serial{1};   // one for the process: a serial never names two models
    m.serial = next_serial.fetch_add(1, std::memory_order_relaxed);
    m.valid = true;
    return RVSEG_OK;
}

static rvseg_status model_start_on(rvseg_ctx* ctx, CrfState* cs, float* d_Q, hipStream_t s, bool timed) {
    const MfRun run = model_run(cs, s, timed);
    RV_TRY(mf_scratch(ctx, cs, run));
    mf_start(ctx, cs, run, model_view(cs->model, d_Q));
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

static rvseg_status model_step_on(rvseg_ctx* ctx, CrfState* cs, float* d_Q, int n_steps, hipStream_t s, bool timed) {
    const MfRun run = model_run(cs, s, timed);
    RV_TRY(mf_scratch(ctx, cs, run));
    RV_TRY(mf_entry_norms(ctx, cs, run));
    for (int it = 0; it < n_steps; it++) mf_step(ctx, cs, run, model_view(cs->model, d_Q));
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// DenseKernel::filter (pairwise.cpp:63-80) up to its blur: the input scaled where the normalisation says so, splat, blur
// (transpose: the axes in reverse order).  *post: whether the sliced output is scaled.  Needs mf_scratch.
static rvseg_status model_filter_term(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, int k, const float* d_in, bool transpose, float** blurred,
                                      bool* post) {
    LatticeBufs& b = cs->lat[k];
    const TermPlan& t = r.plan[k];
    const bool pre = transpose ? term_post(t) : term_pre(t);
    *post = transpose ? term_pre(t) : term_post(t);
    if (pre) RV_TRY(ensure_csr_nrm(ctx, b, r.s));
    auto& sc = cs->scratch[r.slot];
    if (r.timed) timer_mark(ctx, "splat", r.s);
    launch_splat(b.dev, model_view(cs->model, d_in), r.C, pre ? 1 : 0, sc.val_a.as<float>(), r.s);
    if (r.timed) timer_mark(ctx, "blur", r.s);
    *blurred = launch_blur(b.dev, r.C, r.C <= 2, transpose, sc.val_a.as<float>(), sc.val_b.as<float>(), r.s);
    return RVSEG_OK;
}

// pairwise_[term]->apply(out, Q) / applyTranspose (pairwise.cpp:173-183: the filter + the compatibility): needs mf_scratch
static rvseg_status model_apply_term(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, int k, const float* d_in, float* d_out, bool transpose = false) {
    const TermPlan& t = r.plan[k];
    float* blurred;
    bool post;
    RV_TRY(model_filter_term(ctx, cs, r, k, d_in, transpose, &blurred, &post));
    launch_term_update(cs->lat[k].dev, r.C, r.C <= 2, blurred, post, t.matrix, r.d_compat + t.off, d_out, r.n_points, r.s, true);
    return RVSEG_OK;
}

static rvseg_status model_term_arg(rvseg_ctx* ctx, const CrfModel& m, int term, int lowest) {
    if (term >= lowest && term < (int)m.plan.size()) return RVSEG_OK;
    ctx->err = "no such term in the DenseCRF model";
    return RVSEG_ERR_INVALID_ARG;
}

static rvseg_status model_apply_on(rvseg_ctx* ctx, CrfState* cs, int term, const float* d_in, float* d_out, hipStream_t s, bool transpose) {
    const MfRun run = model_run(cs, s, false);
    RV_TRY(mf_scratch(ctx, cs, run));
    RV_TRY(model_apply_term(ctx, cs, run, term, d_in, d_out, transpose));
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// DenseCRF::unaryEnergy / pairwiseEnergy (densecrf.cpp:141-177); term == -1: the terms' energies added in fp32 from 0.0f, ascending
static rvseg_status model_energy_on(rvseg_ctx* ctx, CrfState* cs, const int8_t* d_labels, int term, float* d_unary_out, float* d_pairwise_out,
                                    hipStream_t s) {
    CrfModel& m = cs->model;
    const MfRun run = model_run(cs, s, false);
    if (d_unary_out) launch_label_gather(m.unary.as<float>(), d_labels, m.N, m.C, m.unary_is_energy ? 1.0f : -1.0f, false, d_unary_out, s);
    if (d_pairwise_out) {
        const size_t tot = (size_t)m.N * m.C;
        RV_TRY(mf_scratch(ctx, cs, run));
        RV_TRY(dev_reserve(ctx, m.onehot, tot * 4));
        RV_TRY(dev_reserve(ctx, m.rows, tot * 4));
        if (term < 0) RV_HIP(ctx, hipMemsetAsync(d_pairwise_out, 0, (size_t)m.N * 4, s));
        launch_onehot(d_labels, m.N, m.C, m.onehot.as<float>(), s);
        for (int k = term < 0 ? 0 : term; k < (term < 0 ? (int)m.plan.size() : term + 1); k++) {
            RV_TRY(model_apply_term(ctx, cs, run, k, m.onehot.as<float>(), m.rows.as<float>()));
            launch_label_gather(m.rows.as<float>(), d_labels, m.N, m.C, -0.5f, term < 0, d_pairwise_out, s);
        }
    }
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// the KL parts of a Q nobody is about to step: a filter per term of their own.  Needs mf_scratch, mf_entry_norms (which
// leaves model_filter_term's ensure_csr_nrm nothing to do) and CrfModel::partials.
static rvseg_status model_kl_parts(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, const float* d_Q, const KlTap& tap) {
    kl_unary_parts(ctx, r, d_Q, tap);
    for (int k = 0; k < (int)r.plan.size(); k++) {
        float* blurred;
        bool post;
        RV_TRY(model_filter_term(ctx, cs, r, k, d_Q, false, &blurred, &post));
        kl_term_part(ctx, cs, r, k, blurred, d_Q, tap);
    }
    return RVSEG_OK;
}

static rvseg_status model_kl_scratch(rvseg_ctx* ctx, CrfState* cs, const MfRun& run) {
    RV_TRY(mf_scratch(ctx, cs, run));
    RV_TRY(mf_entry_norms(ctx, cs, run));
    return dev_reserve(ctx, cs->model.partials, (size_t)10 * KL_MAX_BLOCKS * sizeof(double));
}

static rvseg_status model_kl_on(rvseg_ctx* ctx, CrfState* cs, const float* d_Q, double* d_parts, hipStream_t s, bool timed) {
    CrfModel& m = cs->model;
    const MfRun run = model_run(cs, s, timed);
    RV_TRY(model_kl_scratch(ctx, cs, run));
    const KlTap tap{m.partials.as<double>()};
    RV_TRY(model_kl_parts(ctx, cs, run, d_Q, tap));
    launch_kl_final(tap.partials, kl_blocks(m.C, m.N), 2 + (int)m.plan.size(), d_parts, nullptr, s);
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// inference from the start with the KL divergence after the start and after every iteration: d_kl[0 .. iterations].  The
// KL of the Q an iteration starts from rides on that iteration's splat and blur (KlTap); only the last Q pays for a filter.
static rvseg_status model_trace_on(rvseg_ctx* ctx, CrfState* cs, int iterations, float* d_Q, int8_t* d_map, int label_mode, int unknown_label,
                                   double* d_kl, hipStream_t s, bool timed) {
    CrfModel& m = cs->model;
    const MfRun run = model_run(cs, s, timed);
    RV_TRY(model_kl_scratch(ctx, cs, run));
    const KlTap tap{m.partials.as<double>()};
    const int blocks = kl_blocks(m.C, m.N), parts = 2 + (int)m.plan.size();
    const ValueView Q = model_view(m, d_Q);
    mf_start(ctx, cs, run, Q);
    for (int it = 0; it < iterations; it++) {
        mf_step(ctx, cs, run, Q, &tap);
        launch_kl_final(tap.partials, blocks, parts, nullptr, d_kl + it, s);
    }
    RV_TRY(model_kl_parts(ctx, cs, run, d_Q, tap));
    launch_kl_final(tap.partials, blocks, parts, nullptr, d_kl + iterations, s);
    if (d_map) {
        if (timed) timer_mark(ctx, "labels", s);
        launch_labels(d_Q, (size_t)m.N, m.C, label_mode, unknown_label, d_map, s);
    }
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// ---------------------------------------------------------------------------------------------
// Learning on the kept model (include/rvseg.h, "Learning on the kept model"): objective, backward pass, gradient.
// ---------------------------------------------------------------------------------------------
static size_t term_compat_params(const CrfModel& m, int k) {
    const int kind = m.plan[k].compat;
    return kind == RVSEG_COMPAT_MATRIX ? (size_t)m.C * (m.C + 1) / 2 : kind == RVSEG_COMPAT_DIAGONAL ? (size_t)m.C : 1;
}

// the layout of labelCompatibilityParameters(): the terms concatenated
static size_t model_compat_params(const CrfModel& m, int upto = -1) {
    size_t n = 0;
    const int end = upto < 0 ? (int)m.plan.size() : upto;
    for (int k = 0; k < end; k++) n += term_compat_params(m, k);
    return n;
}

static rvseg_status objective_arg(rvseg_ctx* ctx, const rvseg_crf_objective* obj) {
    if (rvseg_crf_objective_check(obj) == RVSEG_OK) return RVSEG_OK;
    ctx->err = "bad objective (rvseg_crf_objective_check: kind, gt, class_weight for HAMMING, finite robust)";
    return RVSEG_ERR_INVALID_ARG;
}

// obj: device pointers
static rvseg_status model_objective_on(rvseg_ctx* ctx, CrfState* cs, const rvseg_crf_objective& obj, const float* d_Q, double* d_value,
                                       float* d_dq, hipStream_t s) {
    CrfModel& m = cs->model;
    RV_TRY(dev_reserve(ctx, cs->learn_partials, learn_partials_doubles(m.C) * sizeof(double)));
    RV_TRY(dev_reserve(ctx, m.stats, 129 * sizeof(double)));
    launch_objective(obj.kind, obj.gt, obj.robust, obj.class_weight, d_Q, m.C, m.N, d_dq, cs->learn_partials.as<double>(), m.stats.as<double>(),
                     d_value, s);
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// ---------------------------------------------------------------------------------------------
// The kernel-parameter gradient (include/rvseg.h, "Kernel-parameter gradient"): Permutohedral::gradient, DenseKernel::
// featureGradient / gradient, PairwisePotential::kernelGradient.
// ---------------------------------------------------------------------------------------------
static size_t term_kernel_params(const TermPlan& t) {
    return t.kernel == RVSEG_FULL_KERNEL ? (size_t)t.d * t.d : t.kernel == RVSEG_DIAG_KERNEL ? (size_t)t.d : 0;
}

// the layout of kernelParameters(): the terms concatenated
static size_t model_kernel_params(const CrfModel& m, int upto = -1) {
    size_t n = 0;
    const int end = upto < 0 ? (int)m.plan.size() : upto;
    for (int k = 0; k < end; k++) n += term_kernel_params(m.plan[k]);
    return n;
}

// the work memory of model_kernel_gradient_term for term k (beside mf_scratch), by what the term needs: a term without
// normalisation mixes nothing (fg alone), SYMMETRIC scales and filters both matrices, AFTER / BEFORE one of each
static rvseg_status model_kgrad_scratch(rvseg_ctx* ctx, CrfState* cs, int k) {
    CrfModel& m = cs->model;
    const TermPlan& t = m.plan[k];
    const size_t tot = (size_t)m.N * m.C * 4, nd = (size_t)m.N * t.d * 4;
    RV_TRY(dev_reserve(ctx, m.kg_fg, nd));
    if (t.norm != RVSEG_NO_NORMALIZATION) {
        const bool sym = t.norm == RVSEG_NORMALIZE_SYMMETRIC;
        for (DevBuf* b : {&m.kg_x, &m.kg_ones}) RV_TRY(dev_reserve(ctx, *b, tot));
        if (sym || t.norm == RVSEG_NORMALIZE_AFTER) for (DevBuf* b : {&m.kg_an, &m.kg_fb}) RV_TRY(dev_reserve(ctx, *b, tot));
        if (sym || t.norm == RVSEG_NORMALIZE_BEFORE) for (DevBuf* b : {&m.kg_bn, &m.kg_fa}) RV_TRY(dev_reserve(ctx, *b, tot));
        for (DevBuf* b : {&m.kg_g1, &m.kg_g2}) RV_TRY(dev_reserve(ctx, *b, nd));
    }
    if (t.kernel == RVSEG_CONST_KERNEL) return RVSEG_OK;
    RV_TRY(dev_reserve(ctx, m.kg_full, 49 * sizeof(double)));
    return dev_reserve(ctx, cs->learn_partials, learn_partials_doubles(std::max(m.C, 7)) * sizeof(double));
}

// Permutohedral::gradient (permutohedral.cpp:611-695) of term k: per direction the ordered splat of a (dir 0) or b (dir 1),
// the blur of seqCompute's rounding with the axes ascending (dir 0) or descending (dir 1), the slicing gradient weighted
// by the other matrix.  df: N x d.  Needs mf_scratch.
static void model_lattice_gradient_term(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, int k, const float* a, const float* b, float* df) {
    const LatticeDev& L = cs->lat[k].dev;
    auto& sc = cs->scratch[r.slot];
    const unsigned* ranks = cs->model.keep[k].rank.as<unsigned>();
    for (int dir = 0; dir < 2; dir++) {
        launch_splat(L, model_view(cs->model, dir ? b : a), r.C, 0, sc.val_a.as<float>(), r.s);
        const float* blurred = launch_blur(L, r.C, true, dir == 1, sc.val_a.as<float>(), sc.val_b.as<float>(), r.s);
        launch_slice_gradient(L, r.C, blurred, dir ? a : b, ranks, dir, r.n_points, df, r.s);
    }
}

// lattice_.compute(in, transpose): the filter without any normalisation, with the blur apply / apply_transpose use
static void model_plain_filter(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, int k, const float* in, bool transpose, float* out) {
    const LatticeDev& L = cs->lat[k].dev;
    auto& sc = cs->scratch[r.slot];
    launch_splat(L, model_view(cs->model, in), r.C, 0, sc.val_a.as<float>(), r.s);
    const float* blurred = launch_blur(L, r.C, r.C <= 2, transpose, sc.val_a.as<float>(), sc.val_b.as<float>(), r.s);
    launch_slice(L, r.C, r.C <= 2, 0, blurred, 0.f, out, r.n_points, r.s);
}

// DenseKernel::featureGradient (pairwise.cpp:87-114) of term k into fg (N x d).  Needs mf_scratch and model_kgrad_scratch.
// Stage marks of a timed call, each once, where its work starts: "filter" (the scaled matrices, K / K^T and X; normalised
// terms only), then "lattice_gradient" (every G, and their difference).
static void model_feature_gradient_term(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, int k, const float* a, const float* b, float* fg) {
    CrfModel& m = cs->model;
    const TermPlan& t = r.plan[k];
    if (t.norm == RVSEG_NO_NORMALIZATION) {
        if (r.timed) timer_mark(ctx, "lattice_gradient", r.s);
        return model_lattice_gradient_term(ctx, cs, r, k, a, b, fg);
    }
    const long long tot = (long long)m.N * m.C, nd = (long long)m.N * t.d;
    const float* n = cs->lat[k].dev.norm;
    float *an = m.kg_an.as<float>(), *bn = m.kg_bn.as<float>(), *fa = m.kg_fa.as<float>(), *fb = m.kg_fb.as<float>(), *X = m.kg_x.as<float>();
    float *ones = m.kg_ones.as<float>(), *g1 = m.kg_g1.as<float>(), *g2 = m.kg_g2.as<float>();
    const auto mix = [&](int mode, const float* x, const float* y, const float* fx, const float* fy, float* out) {
        launch_kgrad_mix(mode, x, y, fx, fy, n, m.C, tot, out, r.s);
    };
    const float *ga = a, *gb = b;   // the arguments of the first G
    if (r.timed) timer_mark(ctx, "filter", r.s);
    if (t.norm == RVSEG_NORMALIZE_SYMMETRIC) {   // :90-97
        mix(0, a, nullptr, nullptr, nullptr, an);
        mix(0, b, nullptr, nullptr, nullptr, bn);
        model_plain_filter(ctx, cs, r, k, an, true, fa);
        model_plain_filter(ctx, cs, r, k, bn, false, fb);
        mix(1, a, b, fa, fb, X);
        ga = an; gb = bn;
    } else if (t.norm == RVSEG_NORMALIZE_AFTER) {   // :98-105
        model_plain_filter(ctx, cs, r, k, b, false, fb);
        mix(2, a, fb, nullptr, nullptr, X);
        mix(0, a, nullptr, nullptr, nullptr, an);
        ga = an;
    } else {   // NORMALIZE_BEFORE, :106-113
        model_plain_filter(ctx, cs, r, k, a, true, fa);
        mix(2, fa, b, nullptr, nullptr, X);
        mix(0, b, nullptr, nullptr, nullptr, bn);
        gb = bn;
    }
    mix(4, nullptr, nullptr, nullptr, nullptr, ones);
    if (r.timed) timer_mark(ctx, "lattice_gradient", r.s);
    model_lattice_gradient_term(ctx, cs, r, k, ga, gb, g1);
    model_lattice_gradient_term(ctx, cs, r, k, X, ones, g2);
    launch_kgrad_mix(3, g1, g2, nullptr, nullptr, nullptr, t.d, nd, fg, r.s);
}

// DenseKernel::gradient(a, b) (pairwise.cpp:152-163) of term k: the feature gradient into fg (null: work memory), and for
// a DIAG or FULL kernel its product with the raw features ADDED to the term's doubles d_grad (null: none)
static void model_kernel_gradient_term(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, int k, const float* a, const float* b, double* d_grad,
                                       float* fg) {
    CrfModel& m = cs->model;
    const TermPlan& t = r.plan[k];
    if (!fg) fg = m.kg_fg.as<float>();
    model_feature_gradient_term(ctx, cs, r, k, a, b, fg);
    if (!d_grad || t.kernel == RVSEG_CONST_KERNEL) return;
    if (r.timed) timer_mark(ctx, "reduce", r.s);
    launch_logistic_gradient(fg, m.keep[k].feat.as<float>(), m.N, t.d, t.d, cs->learn_partials.as<double>(), m.kg_full.as<double>(), r.s);
    launch_kgrad_accumulate(t.kernel == RVSEG_DIAG_KERNEL, t.d, m.kg_full.as<double>(), d_grad, r.s);
}

static rvseg_status model_lattice_gradient_on(rvseg_ctx* ctx, CrfState* cs, int term, const float* d_a, const float* d_b, float* d_df,
                                              hipStream_t s) {
    const MfRun run = model_run(cs, s, false);
    RV_TRY(mf_scratch(ctx, cs, run));
    model_lattice_gradient_term(ctx, cs, run, term, d_a, d_b, d_df);
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// d_grad (may be null): the term's doubles, assigned
static rvseg_status model_kernel_gradient_on(rvseg_ctx* ctx, CrfState* cs, int term, const float* d_a, const float* d_b, double* d_grad,
                                             float* d_fg, hipStream_t s, bool timed) {
    const MfRun run = model_run(cs, s, timed);
    RV_TRY(mf_scratch(ctx, cs, run));
    RV_TRY(model_kgrad_scratch(ctx, cs, term));
    const size_t n = term_kernel_params(cs->model.plan[term]);
    if (d_grad && n) RV_HIP(ctx, hipMemsetAsync(d_grad, 0, n * sizeof(double), s));
    model_kernel_gradient_term(ctx, cs, run, term, d_a, d_b, d_grad, d_fg);
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// densecrf.cpp:258-296 from d_mul_Q and Q[0 .. n]; d_ug / d_cg / d_kg may be null
static rvseg_status model_backward_on(rvseg_ctx* ctx, CrfState* cs, int iterations, const float* d_Qall, const float* d_dq, float* d_ug,
                                      double* d_cg, double* d_kg, hipStream_t s) {
    CrfModel& m = cs->model;
    const MfRun run = model_run(cs, s, false);
    const size_t tot = (size_t)m.N * m.C;
    const int n_terms = (int)m.plan.size();
    RV_TRY(mf_scratch(ctx, cs, run));
    RV_TRY(dev_reserve(ctx, m.bgrad, tot * 4));
    RV_TRY(dev_reserve(ctx, m.tsum, tot * 4));
    RV_TRY(dev_reserve(ctx, m.tapp, tot * 4));
    RV_TRY(dev_reserve(ctx, cs->learn_partials, learn_partials_doubles(m.C) * sizeof(double)));
    float *b = m.bgrad.as<float>(), *tsum = m.tsum.as<float>(), *tapp = m.tapp.as<float>();
    launch_sum_normalize(d_dq, false, d_Qall + (size_t)iterations * tot, m.C, m.N, b, d_ug, 1, s);
    if (d_cg && model_compat_params(m)) RV_HIP(ctx, hipMemsetAsync(d_cg, 0, model_compat_params(m) * sizeof(double), s));
    if (d_kg && !model_kernel_params(m)) d_kg = nullptr;
    if (d_kg) {   // (a grow-only reserve per term with kernel parameters, before anything of the pass is enqueued)
        RV_TRY(dev_reserve(ctx, m.kg_lbl, tot * 4));
        for (int k = 0; k < n_terms; k++)
            if (m.plan[k].kernel != RVSEG_CONST_KERNEL) RV_TRY(model_kgrad_scratch(ctx, cs, k));
        RV_HIP(ctx, hipMemsetAsync(d_kg, 0, model_kernel_params(m) * sizeof(double), s));
    }
    for (int it = iterations - 1; it >= 0; it--) {
        const float* Qit = d_Qall + (size_t)it * tot;
        if (n_terms == 0) RV_HIP(ctx, hipMemsetAsync(tsum, 0, tot * 4, s));   // tmp1.fill(0), :270
        for (int k = 0; k < n_terms; k++) {
            if (d_cg) {   // pairwise_[k]->gradient(b, Q[it]) (pairwise.cpp:190-195)
                float* blurred;
                bool post;
                RV_TRY(model_filter_term(ctx, cs, run, k, Qit, false, &blurred, &post));
                launch_compat_grad(cs->lat[k].dev, m.C, m.C <= 2, blurred, post, m.plan[k].compat, b, m.N, cs->learn_partials.as<double>(),
                                   d_cg + model_compat_params(m, k), s);
            }
            if (d_kg && m.plan[k].kernel != RVSEG_CONST_KERNEL) {   // pairwise_[k]->kernelGradient(b, Q[it]) (pairwise.cpp:202-207)
                launch_compat_rows(m.C, m.plan[k].matrix, run.d_compat + m.plan[k].off, Qit, m.N, m.kg_lbl.as<float>(), s);
                model_kernel_gradient_term(ctx, cs, run, k, b, m.kg_lbl.as<float>(), d_kg + model_kernel_params(m, k), nullptr);
            }
            RV_TRY(model_apply_term(ctx, cs, run, k, b, tapp, true));
            launch_add_rows(k == 0, tapp, tsum, (long long)tot, s);
        }
        launch_sum_normalize(tsum, true, Qit, m.C, m.N, b, d_ug, 2, s);
    }
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

// the forward pass of DenseCRF::gradient (:240-253) keeping Q[0 .. n] in CrfModel::qs, then objective and backward
static rvseg_status model_gradient_on(rvseg_ctx* ctx, CrfState* cs, int iterations, const rvseg_crf_objective& obj, double* d_value, float* d_ug,
                                      double* d_cg, double* d_kg, float* d_Q_out, hipStream_t s) {
    CrfModel& m = cs->model;
    const MfRun run = model_run(cs, s, false);
    const size_t tot = (size_t)m.N * m.C;
    RV_TRY(dev_reserve(ctx, m.qs, ((size_t)iterations + 1) * tot * 4));
    RV_TRY(dev_reserve(ctx, m.dq, tot * 4));
    RV_TRY(mf_scratch(ctx, cs, run));
    RV_TRY(mf_entry_norms(ctx, cs, run));
    float* qs = m.qs.as<float>();
    mf_start(ctx, cs, run, model_view(m, qs));
    for (int it = 0; it < iterations; it++) {
        float* next = qs + (size_t)(it + 1) * tot;
        RV_HIP(ctx, hipMemcpyAsync(next, qs + (size_t)it * tot, tot * 4, hipMemcpyDeviceToDevice, s));
        mf_step(ctx, cs, run, model_view(m, next));
    }
    RV_LAUNCH_OK(ctx);
    const float* Qn = qs + (size_t)iterations * tot;
    RV_TRY(model_objective_on(ctx, cs, obj, Qn, d_value, m.dq.as<float>(), s));
    RV_TRY(model_backward_on(ctx, cs, iterations, qs, m.dq.as<float>(), d_ug, d_cg, d_kg, s));
    if (d_Q_out) RV_HIP(ctx, hipMemcpyAsync(d_Q_out, Qn, tot * 4, hipMemcpyDeviceToDevice, s));
    return RVSEG_OK;
}

// ---------------------------------------------------------------------------------------------
// The entry bodies: the live model, the arguments, the arrays through `io`, the call on device pointers, io.done().
// ---------------------------------------------------------------------------------------------
static rvseg_status model_start(ModelIo io, float* Q_out) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(Q_out);
    CrfModel& m = io.cs->model;
    RV_TRY(io.out(m.q, &Q_out, (size_t)m.N * m.C));
    RV_TRY(model_start_on(io.ctx, io.cs, Q_out, io.s, io.time()));
    return io.done();
}

static rvseg_status model_step(ModelIo io, float* Q_inout, int32_t n_steps) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(Q_inout && n_steps >= 0);
    CrfModel& m = io.cs->model;
    const float* Q_in = Q_inout;   // in and out through the same buffer
    RV_TRY(io.out(m.q, &Q_inout, (size_t)m.N * m.C));
    RV_TRY(io.in(m.q, &Q_in, (size_t)m.N * m.C));
    RV_TRY(model_step_on(io.ctx, io.cs, Q_inout, n_steps, io.s, io.time()));
    return io.done();
}

static rvseg_status model_apply(ModelIo io, int32_t term, const float* in, float* out, bool transpose) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(in && out);
    CrfModel& m = io.cs->model;
    RV_TRY(model_term_arg(io.ctx, m, term, 0));
    RV_TRY(io.in(m.q, &in, (size_t)m.N * m.C));
    RV_TRY(io.out(m.rows, &out, (size_t)m.N * m.C));
    RV_TRY(model_apply_on(io.ctx, io.cs, term, in, out, io.s, transpose));
    return io.done();
}

static rvseg_status model_energy(ModelIo io, const int8_t* labels, int32_t term, float* unary_out, float* pairwise_out) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(labels && (unary_out || pairwise_out));
    CrfModel& m = io.cs->model;
    if (pairwise_out) RV_TRY(model_term_arg(io.ctx, m, term, -1));
    const size_t N = (size_t)m.N;
    RV_TRY(io.in(m.labels, &labels, N));
    if (io.on_host) {   // both vectors in CrfModel::vec
        RV_TRY(dev_reserve(io.ctx, m.vec, 2 * N * 4));
        io.out_at(m.vec.as<float>(), &unary_out, N);
        io.out_at(m.vec.as<float>() + N, &pairwise_out, N);
    }
    RV_TRY(model_energy_on(io.ctx, io.cs, labels, term, unary_out, pairwise_out, io.s));
    return io.done();
}

static rvseg_status model_kl(ModelIo io, const float* Q, double* parts) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(Q && parts);
    CrfModel& m = io.cs->model;
    RV_TRY(io.in(m.q, &Q, (size_t)m.N * m.C));
    RV_TRY(io.out(m.kl, &parts, 2 + m.plan.size()));
    RV_TRY(model_kl_on(io.ctx, io.cs, Q, parts, io.s, io.time()));
    return io.done();
}

static rvseg_status model_trace(ModelIo io, int32_t iterations, float* Q_out, int8_t* map_out, int32_t label_mode, int32_t unknown_label,
                                double* kl_out) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(iterations >= 0 && Q_out && kl_out && label_mode >= 0 && label_mode <= 3);
    CrfModel& m = io.cs->model;
    RV_TRY(io.out(m.q, &Q_out, (size_t)m.N * m.C));
    RV_TRY(io.out(m.labels, &map_out, (size_t)m.N));
    RV_TRY(io.out(m.kl, &kl_out, (size_t)iterations + 1));   // written on the device, read back once
    RV_TRY(model_trace_on(io.ctx, io.cs, iterations, Q_out, map_out, label_mode, unknown_label, kl_out, io.s, io.time()));
    return io.done();
}

// *obj on device pointers: gt and (HAMMING only) the class weights of a host entry staged.  For the other kinds
// class_weight stays the caller's pointer, host or device: no kernel of theirs reads it (launch_objective).
static rvseg_status model_objective_in(ModelIo& io, CrfModel& m, rvseg_crf_objective* obj) {
    RV_TRY(io.in(m.gt, &obj->gt, (size_t)m.N));
    if (obj->kind == RVSEG_OBJECTIVE_HAMMING) RV_TRY(io.in(m.cw, &obj->class_weight, (size_t)m.C));
    return RVSEG_OK;
}

static rvseg_status model_objective(ModelIo io, const rvseg_crf_objective* obj, const float* Q, double* value_out, float* d_mul_Q_out) {
    RV_TRY(io.enter());
    RV_TRY(objective_arg(io.ctx, obj));
    RV_MODEL_ARGS(Q && value_out && d_mul_Q_out);
    CrfModel& m = io.cs->model;
    rvseg_crf_objective dev = *obj;
    RV_TRY(model_objective_in(io, m, &dev));
    RV_TRY(io.in(m.q, &Q, (size_t)m.N * m.C));
    RV_TRY(dev_reserve(io.ctx, m.stats, 129 * sizeof(double)));
    io.out_at(m.stats.as<double>() + 128, &value_out, 1);   // where a host entry's value lands
    RV_TRY(io.out(m.dq, &d_mul_Q_out, (size_t)m.N * m.C));
    RV_TRY(model_objective_on(io.ctx, io.cs, dev, Q, value_out, d_mul_Q_out, io.s));
    return io.done();
}

// lbl_Q = compatibility(Q) with no filter (pairwise.cpp:203-205)
static rvseg_status model_compat_apply(ModelIo io, int32_t term, const float* Q, float* out) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(Q && out);
    CrfModel& m = io.cs->model;
    RV_TRY(model_term_arg(io.ctx, m, term, 0));
    RV_TRY(io.in(m.kg_a, &Q, (size_t)m.N * m.C));
    RV_TRY(io.out(m.kg_b, &out, (size_t)m.N * m.C));
    launch_compat_rows(m.C, m.plan[term].matrix, io.cs->compat.as<float>() + m.plan[term].off, Q, m.N, out, io.s);
    RV_LAUNCH_OK(io.ctx);
    return io.done();
}

static rvseg_status model_lattice_gradient(ModelIo io, int32_t term, const float* a, const float* b, float* df_out) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(a && b && df_out);
    CrfModel& m = io.cs->model;
    RV_TRY(model_term_arg(io.ctx, m, term, 0));
    const size_t tot = (size_t)m.N * m.C;
    RV_TRY(io.in(m.kg_a, &a, tot));
    RV_TRY(io.in(m.kg_b, &b, tot));
    RV_TRY(io.out(m.kg_out, &df_out, (size_t)m.N * m.plan[term].d));
    RV_TRY(model_lattice_gradient_on(io.ctx, io.cs, term, a, b, df_out, io.s));
    return io.done();
}

static rvseg_status model_kernel_gradient(ModelIo io, int32_t term, const float* a, const float* b, double* grad_out, float* fg_out) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(a && b);
    CrfModel& m = io.cs->model;
    RV_TRY(model_term_arg(io.ctx, m, term, 0));
    const size_t tot = (size_t)m.N * m.C;
    RV_TRY(io.in(m.kg_a, &a, tot));
    RV_TRY(io.in(m.kg_b, &b, tot));
    RV_TRY(io.out(m.kg_grad, &grad_out, term_kernel_params(m.plan[term])));
    RV_TRY(io.out(m.kg_out, &fg_out, (size_t)m.N * m.plan[term].d));
    RV_TRY(model_kernel_gradient_on(io.ctx, io.cs, term, a, b, grad_out, fg_out, io.s, io.time()));
    return io.done();
}

static rvseg_status model_backward(ModelIo io, int32_t iterations, const float* Q_all, const float* d_mul_Q, float* unary_grad_out,
                                   double* compat_grad_out, double* kernel_grad_out) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(iterations >= 0 && Q_all && d_mul_Q);
    CrfModel& m = io.cs->model;
    const size_t tot = (size_t)m.N * m.C;
    RV_TRY(io.in(m.qs, &Q_all, ((size_t)iterations + 1) * tot));
    RV_TRY(io.in(m.dq, &d_mul_Q, tot));
    RV_TRY(io.out(m.ug, &unary_grad_out, tot));
    RV_TRY(io.out(m.cg, &compat_grad_out, model_compat_params(m)));
    RV_TRY(io.out(m.kg_grad, &kernel_grad_out, model_kernel_params(m)));
    RV_TRY(model_backward_on(io.ctx, io.cs, iterations, Q_all, d_mul_Q, unary_grad_out, compat_grad_out, kernel_grad_out, io.s));
    return io.done();
}

static rvseg_status model_set_compat(ModelIo io, int32_t term, const float* params) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(params);
    CrfModel& m = io.cs->model;
    RV_TRY(model_term_arg(io.ctx, m, term, 0));
    TermPlan& t = m.plan[term];
    std::vector<float> hc(t.compat == RVSEG_COMPAT_MATRIX ? (size_t)m.C * m.C : (size_t)m.C);
    plan_compat(m.C, t.compat, params, t, hc.data());
    RV_HIP(io.ctx, hipMemcpyAsync(io.cs->compat.as<float>() + t.off, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, io.s));
    return io.done();   // waits: hc is gone when this returns
}

static rvseg_status model_set_unary(ModelIo io, const float* unary, int32_t unary_is_energy) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(unary);
    CrfModel& m = io.cs->model;
    RV_HIP(io.ctx, hipMemcpyAsync(m.unary.p, unary, (size_t)m.N * m.C * 4, io.on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, io.s));
    RV_TRY(io.done());   // a host entry waits: the caller's array is free when it returns
    m.unary_is_energy = unary_is_energy != 0;
    m.K = 0;   // (a kept logistic unary ends here)
    return RVSEG_OK;
}

// ---------------------------------------------------------------------------------------------
// The learning loop (include/rvseg.h, "The learning loop"): parameters in place, the parameter gradient, CRFEnergy::gradient.
// ---------------------------------------------------------------------------------------------
static rvseg_status model_set_kernel(ModelIo io, int32_t term, const float* params) {
    RV_TRY(io.enter());
    CrfModel& m = io.cs->model;
    RV_TRY(model_term_arg(io.ctx, m, term, 0));
    const size_t np = term_kernel_params(m.plan[term]);
    if (!np) { io.ctx->err = "a CONST_KERNEL term has no kernel parameters"; return RVSEG_ERR_INVALID_ARG; }
    RV_TRY(term_rebuild(io.ctx, io.cs, term, params, io.s));   // (has waited for the stream)
    TermKeep& keep = m.keep[term];
    keep.has_kparams = params != nullptr;
    keep.kparams.assign(params, params + (params ? np : 0));
    return RVSEG_OK;
}

// U = L f from the model's copies of L (host memory, uploaded here) and f
static rvseg_status model_logistic_unary(ModelIo& io, const float* L) {
    CrfModel& m = io.cs->model;
    const size_t bytes = (size_t)m.C * m.K * 4;
    // L is the caller's and may be gone once the entry returns: it is uploaded from a pinned copy of the model's, which the
    // previous upload has left (long ago, as a rule) before it is written again.  A device entry only enqueues.
    if (!m.lmat_ev) RV_HIP(io.ctx, event_create(m.lmat_ev, hipEventDisableTiming));
    else RV_HIP(io.ctx, hipEventSynchronize(m.lmat_ev));
    RV_TRY(m.h_lmat.reserve(io.ctx, bytes));
    std::memcpy(m.h_lmat.p, L, bytes);
    RV_TRY(dev_reserve(io.ctx, m.lmat, bytes));
    RV_HIP(io.ctx, hipMemcpyAsync(m.lmat.p, m.h_lmat.p, bytes, hipMemcpyHostToDevice, io.s));
    RV_HIP(io.ctx, hipEventRecord(m.lmat_ev, io.s));
    launch_logistic_unary(m.lmat.as<float>(), m.lfeat.as<float>(), m.N, m.C, m.K, m.unary.as<float>(), io.s);
    RV_LAUNCH_OK(io.ctx);
    m.unary_is_energy = true;
    return RVSEG_OK;
}

static rvseg_status model_set_logistic(ModelIo io, int32_t K, const float* L, const float* f) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(K >= 1 && L && f);
    CrfModel& m = io.cs->model;
    m.K = 0;   // (a failure below leaves the unary as it was, without a kept f)
    RV_TRY(dev_reserve(io.ctx, m.lfeat, (size_t)m.N * K * 4));
    RV_HIP(io.ctx, hipMemcpyAsync(m.lfeat.p, f, (size_t)m.N * K * 4, io.on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, io.s));
    m.K = K;
    RV_TRY(model_logistic_unary(io, L));
    return io.done();   // a host entry waits: f is free when it returns
}

static rvseg_status model_logistic_arg(rvseg_ctx* ctx, const CrfModel& m) {
    if (m.K > 0) return RVSEG_OK;
    ctx->err = "the DenseCRF model keeps no logistic unary (rvseg_crf_model_set_logistic)";
    return RVSEG_ERR_INVALID_ARG;
}

static rvseg_status model_set_logistic_params(ModelIo io, const float* L) {
    RV_TRY(io.enter());
    RV_MODEL_ARGS(L);
    RV_TRY(model_logistic_arg(io.ctx, io.cs->model));
    RV_TRY(model_logistic_unary(io, L));
    return io.done();
}

// rvseg_crf_model_gradient[_kernel] and _gradient_params.  lgrad_out: the unary gradient stays on the device (CrfModel::ug)
// and leaves as the C K doubles of rvseg_crf_logistic_gradient over the kept f (the callers that pass it pass no
// unary_grad_out and no Q_out)
static rvseg_status model_gradient(ModelIo io, int32_t iterations, const rvseg_crf_objective* obj, double* value_out, float* unary_grad_out,
                                   double* lgrad_out, double* compat_grad_out, double* kernel_grad_out, float* Q_out) {
    RV_TRY(io.enter());
    RV_TRY(objective_arg(io.ctx, obj));
    RV_MODEL_ARGS(iterations >= 0 && value_out);
    CrfModel& m = io.cs->model;
    if (lgrad_out) RV_TRY(model_logistic_arg(io.ctx, m));
    const size_t tot = (size_t)m.N * m.C;
    rvseg_crf_objective dev = *obj;
    RV_TRY(model_objective_in(io, m, &dev));
    RV_TRY(dev_reserve(io.ctx, m.stats, 129 * sizeof(double)));
    io.out_at(m.stats.as<double>() + 128, &value_out, 1);
    RV_TRY(io.out(m.ug, &unary_grad_out, tot));
    RV_TRY(io.out(m.lgrad, &lgrad_out, (size_t)m.C * m.K));
    RV_TRY(io.out(m.cg, &compat_grad_out, model_compat_params(m)));
    RV_TRY(io.out(m.kg_grad, &kernel_grad_out, model_kernel_params(m)));
    if (lgrad_out) {   // (the partials at their largest before anything is enqueued: no later reserve moves them)
        RV_TRY(dev_reserve(io.ctx, m.ug, tot * 4));
        RV_TRY(dev_reserve(io.ctx, io.cs->learn_partials, learn_partials_doubles(64) * sizeof(double)));
        unary_grad_out = m.ug.as<float>();
    }
    io.time();   // (the forward pass itself records no marks)
    // a host entry downloads Q[n] from where the forward pass has left it: no device copy of it
    RV_TRY(model_gradient_on(io.ctx, io.cs, iterations, dev, value_out, unary_grad_out, compat_grad_out, kernel_grad_out,
                             io.on_host ? nullptr : Q_out, io.s));
    io.out_at(m.qs.as<float>() + (size_t)iterations * tot, &Q_out, tot);
    if (lgrad_out) {
        if (io.timed) timer_mark(io.ctx, "logistic_gradient", io.s);
        launch_logistic_gradient(unary_grad_out, m.lfeat.as<float>(), m.N, m.C, m.K, io.cs->learn_partials.as<double>(), lgrad_out, io.s);
        RV_LAUNCH_OK(io.ctx);
    }
    return io.done();
}

// the compatibility parameters of term `t` as rvseg_crf_term.compat_params from their slice of labelCompatibilityParameters()
static void compat_from_x(int C, int compat, const float* v, std::vector<float>& out) {
    if (compat != RVSEG_COMPAT_MATRIX) { out.assign(v, v + (compat == RVSEG_COMPAT_DIAGONAL ? C : 1)); return; }
    out.assign((size_t)C * C, 0.f);
    for (int i = 0, k = 0; i < C; i++)
        for (int j = i; j < C; j++, k++) out[(size_t)i * C + j] = out[(size_t)j * C + i] = v[k];
}

static rvseg_status model_energy_gradient(rvseg_ctx* ctx, const char* entry, int32_t iterations, const rvseg_crf_objective* obj, int32_t mask,
                                          float l2, const float* x, int32_t n, double* value_out, float* dx_out) {
    ModelIo io = host_io(ctx, entry);
    RV_TRY(io.enter());
    RV_TRY(objective_arg(ctx, obj));
    CrfModel& m = io.cs->model;
    RV_MODEL_ARGS(iterations >= 0 && value_out && mask >= 0 && mask <= 7 && n >= 0 && (n == 0 || (x && dx_out)) && std::isfinite(l2));
    const size_t nu = (mask & 1) ? (size_t)m.C * m.K : 0, nc = (mask & 2) ? model_compat_params(m) : 0,
                 nk = (mask & 4) ? model_kernel_params(m) : 0;
    if ((size_t)n != nu + nc + nk) { ctx->err = "n is not the number of learned parameters of the model"; return RVSEG_ERR_INVALID_ARG; }
    const int n_terms = (int)m.plan.size();
    if (nu) {   // unaryParameters(): L column-major
        std::vector<float> L(nu);
        for (int c = 0; c < m.C; c++)
            for (int k = 0; k < m.K; k++) L[(size_t)c * m.K + k] = x[(size_t)k * m.C + c];
        RV_TRY(model_set_logistic_params(host_io(ctx, entry), L.data()));
    }
    if (mask & 2) {
        std::vector<float> cp;
        for (int t = 0; t < n_terms; t++) {
            compat_from_x(m.C, m.plan[t].compat, x + nu + model_compat_params(m, t), cp);
            RV_TRY(model_set_compat(host_io(ctx, entry), t, cp.data()));
        }
    }
    if (mask & 4)
        for (int t = 0; t < n_terms; t++) {
            const size_t np = term_kernel_params(m.plan[t]);
            const float* v = x + nu + nc + model_kernel_params(m, t);
            const TermKeep& keep = m.keep[t];
            if (!np || (keep.has_kparams && std::memcmp(keep.kparams.data(), v, np * sizeof(float)) == 0)) continue;
            RV_TRY(model_set_kernel(host_io(ctx, entry), t, v));
        }
    std::vector<double> g(nu + nc + nk);   // the gradients of the learned groups in the order of x
    double* gu = g.data();
    double* gc = gu + nu;
    double* gk = gc + nc;
    RV_TRY(model_gradient(host_io(ctx, entry), iterations, obj, value_out, nullptr, nu ? gu : nullptr, nc ? gc : nullptr, nk ? gk : nullptr, nullptr));
    for (int i = 0; i < n; i++) {
        dx_out[i] = -(float)g[i];
        if (l2 > 0) { const float reg = l2 * x[i]; dx_out[i] = dx_out[i] + reg; }
    }
    *value_out = -*value_out;
    if (l2 > 0) {
        double sum = 0.0;
        for (int i = 0; i < n; i++) sum += (double)x[i] * (double)x[i];
        *value_out += (0.5 * (double)l2) * sum;
    }
    return RVSEG_OK;
}

// needs no model; a host entry stages through CrfState::unary / feat / lgrad (a live model keeps its own copy of the unary)
static rvseg_status logistic_gradient(ModelIo io, int32_t N, int32_t C, int32_t K, const float* unary_grad, const float* f, double* out) {
    RV_TRY(io.enter(false));
    RV_MODEL_ARGS(N > 0 && C >= 1 && C <= 64 && K >= 1 && unary_grad && f && out);
    CrfState* cs = io.cs;
    RV_TRY(io.in(cs->unary, &unary_grad, (size_t)N * C));
    RV_TRY(io.in(cs->feat, &f, (size_t)N * K));
    RV_TRY(io.out(cs->lgrad, &out, (size_t)C * K));
    RV_TRY(dev_reserve(io.ctx, cs->learn_partials, learn_partials_doubles(64) * sizeof(double)));
    launch_logistic_gradient(unary_grad, f, N, C, K, cs->learn_partials.as<double>(), out, io.s);
    RV_LAUNCH_OK(io.ctx);
    return io.done();
}

extern "C" {

rvseg_status rvseg_crf_model_set(rvseg_ctx* ctx, int32_t N, int32_t C, int32_t n_terms, const rvseg_crf_term* terms, const float* unary,
                                 int32_t unary_is_energy) {
    return model_set(host_io(ctx, __func__), N, C, n_terms, terms, unary, unary_is_energy);
}
rvseg_status rvseg_crf_model_set_device(rvseg_ctx* ctx, int32_t N, int32_t C, int32_t n_terms, const rvseg_crf_term* terms,
                                        const float* d_unary, int32_t unary_is_energy, void* hip_stream) {
    return model_set(device_io(ctx, hip_stream, __func__), N, C, n_terms, terms, d_unary, unary_is_energy);
}

rvseg_status rvseg_crf_model_info(rvseg_ctx* ctx, struct rvseg_crf_model_info* out) {
    if (out) *out = {};
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (!out) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    const CrfModel* m = ctx->impl && ctx->impl->crf ? &ctx->impl->crf->model : nullptr;   // (reads only: no state is made here)
    if (!m || !m->valid) return no_model(ctx, m);
    out->serial = m->serial;
    out->N = m->N; out->C = m->C; out->n_terms = (int32_t)m->plan.size(); out->K = m->K;
    for (int k = 0; k < out->n_terms; k++) {
        out->d[k] = m->plan[k].d;
        out->compat_params[k] = (int32_t)term_compat_params(*m, k);
        out->kernel_params[k] = (int32_t)term_kernel_params(m->plan[k]);
    }
    out->n_compat_params = (int32_t)model_compat_params(*m);
    out->n_kernel_params = (int32_t)model_kernel_params(*m);
    return RVSEG_OK;
}

rvseg_status rvseg_crf_model_start(rvseg_ctx* ctx, float* Q_out) { return model_start(host_io(ctx, __func__), Q_out); }
rvseg_status rvseg_crf_model_start_device(rvseg_ctx* ctx, float* d_Q_out, void* hip_stream) {
    return model_start(device_io(ctx, hip_stream, __func__), d_Q_out);
}

rvseg_status rvseg_crf_model_step(rvseg_ctx* ctx, float* Q_inout, int32_t n_steps) { return model_step(host_io(ctx, __func__), Q_inout, n_steps); }
rvseg_status rvseg_crf_model_step_device(rvseg_ctx* ctx, float* d_Q_inout, int32_t n_steps, void* hip_stream) {
    return model_step(device_io(ctx, hip_stream, __func__), d_Q_inout, n_steps);
}

rvseg_status rvseg_crf_model_apply(rvseg_ctx* ctx, int32_t term, const float* Q_in, float* out) {
    return model_apply(host_io(ctx, __func__), term, Q_in, out, false);
}
rvseg_status rvseg_crf_model_apply_device(rvseg_ctx* ctx, int32_t term, const float* d_Q_in, float* d_out, void* hip_stream) {
    return model_apply(device_io(ctx, hip_stream, __func__), term, d_Q_in, d_out, false);
}
rvseg_status rvseg_crf_model_apply_transpose(rvseg_ctx* ctx, int32_t term, const float* in, float* out) {
    return model_apply(host_io(ctx, __func__), term, in, out, true);
}
rvseg_status rvseg_crf_model_apply_transpose_device(rvseg_ctx* ctx, int32_t term, const float* d_in, float* d_out, void* hip_stream) {
    return model_apply(device_io(ctx, hip_stream, __func__), term, d_in, d_out, true);
}

rvseg_status rvseg_crf_model_energy(rvseg_ctx* ctx, const int8_t* labels, int32_t term, float* unary_out, float* pairwise_out) {
    return model_energy(host_io(ctx, __func__), labels, term, unary_out, pairwise_out);
}
rvseg_status rvseg_crf_model_energy_device(rvseg_ctx* ctx, const int8_t* d_labels, int32_t term, float* d_unary_out, float* d_pairwise_out,
                                           void* hip_stream) {
    return model_energy(device_io(ctx, hip_stream, __func__), d_labels, term, d_unary_out, d_pairwise_out);
}

rvseg_status rvseg_crf_model_kl(rvseg_ctx* ctx, const float* Q, double* parts) { return model_kl(host_io(ctx, __func__), Q, parts); }
rvseg_status rvseg_crf_model_kl_device(rvseg_ctx* ctx, const float* d_Q, double* d_parts, void* hip_stream) {
    return model_kl(device_io(ctx, hip_stream, __func__), d_Q, d_parts);
}

rvseg_status rvseg_crf_model_trace(rvseg_ctx* ctx, int32_t iterations, float* Q_out, int8_t* map_out, int32_t label_mode, int32_t unknown_label,
                                   double* kl_out) {
    return model_trace(host_io(ctx, __func__), iterations, Q_out, map_out, label_mode, unknown_label, kl_out);
}
rvseg_status rvseg_crf_model_trace_device(rvseg_ctx* ctx, int32_t iterations, float* d_Q_out, int8_t* d_map_out, int32_t label_mode,
                                          int32_t unknown_label, double* d_kl_out, void* hip_stream) {
    return model_trace(device_io(ctx, hip_stream, __func__), iterations, d_Q_out, d_map_out, label_mode, unknown_label, d_kl_out);
}

rvseg_status rvseg_crf_objective_check(const rvseg_crf_objective* obj) {
    if (!obj || obj->kind < RVSEG_OBJECTIVE_LOGLIKELIHOOD || obj->kind > RVSEG_OBJECTIVE_IOU || !obj->gt) return RVSEG_ERR_INVALID_ARG;
    if (obj->kind == RVSEG_OBJECTIVE_HAMMING && !obj->class_weight) return RVSEG_ERR_INVALID_ARG;
    if (!std::isfinite(obj->robust)) return RVSEG_ERR_INVALID_ARG;
    return RVSEG_OK;
}

rvseg_status rvseg_crf_model_objective(rvseg_ctx* ctx, const rvseg_crf_objective* obj, const float* Q, double* value_out, float* d_mul_Q_out) {
    return model_objective(host_io(ctx, __func__), obj, Q, value_out, d_mul_Q_out);
}
rvseg_status rvseg_crf_model_objective_device(rvseg_ctx* ctx, const rvseg_crf_objective* obj, const float* d_Q, double* d_value_out,
                                              float* d_d_mul_Q_out, void* hip_stream) {
    return model_objective(device_io(ctx, hip_stream, __func__), obj, d_Q, d_value_out, d_d_mul_Q_out);
}

rvseg_status rvseg_crf_model_backward(rvseg_ctx* ctx, int32_t iterations, const float* Q_all, const float* d_mul_Q, float* unary_grad_out,
                                      double* compat_grad_out) {
    return model_backward(host_io(ctx, __func__), iterations, Q_all, d_mul_Q, unary_grad_out, compat_grad_out, nullptr);
}
rvseg_status rvseg_crf_model_backward_device(rvseg_ctx* ctx, int32_t iterations, const float* d_Q_all, const float* d_d_mul_Q,
                                             float* d_unary_grad_out, double* d_compat_grad_out, void* hip_stream) {
    return model_backward(device_io(ctx, hip_stream, __func__), iterations, d_Q_all, d_d_mul_Q, d_unary_grad_out, d_compat_grad_out, nullptr);
}

rvseg_status rvseg_crf_model_gradient(rvseg_ctx* ctx, int32_t iterations, const rvseg_crf_objective* obj, double* value_out,
                                      float* unary_grad_out, double* compat_grad_out, float* Q_out) {
    return model_gradient(host_io(ctx, __func__), iterations, obj, value_out, unary_grad_out, nullptr, compat_grad_out, nullptr, Q_out);
}
rvseg_status rvseg_crf_model_gradient_device(rvseg_ctx* ctx, int32_t iterations, const rvseg_crf_objective* obj, double* d_value_out,
                                             float* d_unary_grad_out, double* d_compat_grad_out, float* d_Q_out, void* hip_stream) {
    return model_gradient(device_io(ctx, hip_stream, __func__), iterations, obj, d_value_out, d_unary_grad_out, nullptr, d_compat_grad_out, nullptr,
                          d_Q_out);
}

rvseg_status rvseg_crf_model_compat_apply(rvseg_ctx* ctx, int32_t term, const float* Q, float* out) {
    return model_compat_apply(host_io(ctx, __func__), term, Q, out);
}
rvseg_status rvseg_crf_model_compat_apply_device(rvseg_ctx* ctx, int32_t term, const float* d_Q, float* d_out, void* hip_stream) {
    return model_compat_apply(device_io(ctx, hip_stream, __func__), term, d_Q, d_out);
}

rvseg_status rvseg_crf_model_lattice_gradient(rvseg_ctx* ctx, int32_t term, const float* a, const float* b, float* df_out) {
    return model_lattice_gradient(host_io(ctx, __func__), term, a, b, df_out);
}
rvseg_status rvseg_crf_model_lattice_gradient_device(rvseg_ctx* ctx, int32_t term, const float* d_a, const float* d_b, float* d_df_out,
                                                     void* hip_stream) {
    return model_lattice_gradient(device_io(ctx, hip_stream, __func__), term, d_a, d_b, d_df_out);
}

rvseg_status rvseg_crf_model_kernel_gradient(rvseg_ctx* ctx, int32_t term, const float* a, const float* b, double* grad_out, float* fg_out) {
    return model_kernel_gradient(host_io(ctx, __func__), term, a, b, grad_out, fg_out);
}
rvseg_status rvseg_crf_model_kernel_gradient_device(rvseg_ctx* ctx, int32_t term, const float* d_a, const float* d_b, double* d_grad_out,
                                                    float* d_fg_out, void* hip_stream) {
    return model_kernel_gradient(device_io(ctx, hip_stream, __func__), term, d_a, d_b, d_grad_out, d_fg_out);
}

rvseg_status rvseg_crf_model_backward_kernel(rvseg_ctx* ctx, int32_t iterations, const float* Q_all, const float* d_mul_Q, float* unary_grad_out,
                                             double* compat_grad_out, double* kernel_grad_out) {
    return model_backward(host_io(ctx, __func__), iterations, Q_all, d_mul_Q, unary_grad_out, compat_grad_out, kernel_grad_out);
}
rvseg_status rvseg_crf_model_backward_kernel_device(rvseg_ctx* ctx, int32_t iterations, const float* d_Q_all, const float* d_d_mul_Q,
                                                    float* d_unary_grad_out, double* d_compat_grad_out, double* d_kernel_grad_out,
                                                    void* hip_stream) {
    return model_backward(device_io(ctx, hip_stream, __func__), iterations, d_Q_all, d_d_mul_Q, d_unary_grad_out, d_compat_grad_out,
                          d_kernel_grad_out);
}

rvseg_status rvseg_crf_model_gradient_kernel(rvseg_ctx* ctx, int32_t iterations, const rvseg_crf_objective* obj, double* value_out,
                                             float* unary_grad_out, double* compat_grad_out, double* kernel_grad_out, float* Q_out) {
    return model_gradient(host_io(ctx, __func__), iterations, obj, value_out, unary_grad_out, nullptr, compat_grad_out, kernel_grad_out, Q_out);
}
rvseg_status rvseg_crf_model_gradient_kernel_device(rvseg_ctx* ctx, int32_t iterations, const rvseg_crf_objective* obj, double* d_value_out,
                                                    float* d_unary_grad_out, double* d_compat_grad_out, double* d_kernel_grad_out,
                                                    float* d_Q_out, void* hip_stream) {
    return model_gradient(device_io(ctx, hip_stream, __func__), iterations, obj, d_value_out, d_unary_grad_out, nullptr, d_compat_grad_out,
                          d_kernel_grad_out, d_Q_out);
}

rvseg_status rvseg_crf_model_set_compat(rvseg_ctx* ctx, int32_t term, const float* params) {
    return model_set_compat(host_io(ctx, __func__), term, params);
}

rvseg_status rvseg_crf_model_set_unary(rvseg_ctx* ctx, const float* unary, int32_t unary_is_energy) {
    return model_set_unary(host_io(ctx, __func__), unary, unary_is_energy);
}
rvseg_status rvseg_crf_model_set_unary_device(rvseg_ctx* ctx, const float* d_unary, int32_t unary_is_energy, void* hip_stream) {
    return model_set_unary(device_io(ctx, hip_stream, __func__), d_unary, unary_is_energy);
}

rvseg_status rvseg_crf_model_set_kernel(rvseg_ctx* ctx, int32_t term, const float* params) {
    return model_set_kernel(host_io(ctx, __func__), term, params);
}

rvseg_status rvseg_crf_model_set_logistic(rvseg_ctx* ctx, int32_t K, const float* L, const float* f) {
    return model_set_logistic(host_io(ctx, __func__), K, L, f);
}
rvseg_status rvseg_crf_model_set_logistic_device(rvseg_ctx* ctx, int32_t K, const float* L, const float* d_f, void* hip_stream) {
    return model_set_logistic(device_io(ctx, hip_stream, __func__), K, L, d_f);
}
rvseg_status rvseg_crf_model_set_logistic_params(rvseg_ctx* ctx, const float* L) {
    return model_set_logistic_params(host_io(ctx, __func__), L);
}

rvseg_status rvseg_crf_model_gradient_params(rvseg_ctx* ctx, int32_t iterations, const rvseg_crf_objective* obj, double* value_out,
                                             double* unary_grad_out, double* compat_grad_out, double* kernel_grad_out) {
    return model_gradient(host_io(ctx, __func__), iterations, obj, value_out, nullptr, unary_grad_out, compat_grad_out, kernel_grad_out, nullptr);
}
rvseg_status rvseg_crf_model_gradient_params_device(rvseg_ctx* ctx, int32_t iterations, const rvseg_crf_objective* obj, double* d_value_out,
                                                    double* d_unary_grad_out, double* d_compat_grad_out, double* d_kernel_grad_out,
                                                    void* hip_stream) {
    return model_gradient(device_io(ctx, hip_stream, __func__), iterations, obj, d_value_out, nullptr, d_unary_grad_out, d_compat_grad_out,
                          d_kernel_grad_out, nullptr);
}

rvseg_status rvseg_crf_model_energy_gradient(rvseg_ctx* ctx, int32_t iterations, const rvseg_crf_objective* obj, int32_t learn_mask,
                                             float l2_norm, const float* x, int32_t n, double* value_out, float* dx_out) {
    return model_energy_gradient(ctx, __func__, iterations, obj, learn_mask, l2_norm, x, n, value_out, dx_out);
}

rvseg_status rvseg_crf_logistic_gradient(rvseg_ctx* ctx, int32_t N, int32_t C, int32_t K, const float* unary_grad, const float* f, double* out) {
    return logistic_gradient(host_io(ctx, __func__), N, C, K, unary_grad, f, out);
}
rvseg_status rvseg_crf_logistic_gradient_device(rvseg_ctx* ctx, int32_t N, int32_t C, int32_t K, const float* d_unary_grad, const float* d_f,
                                                double* d_out, void* hip_stream) {
    return logistic_gradient(device_io(ctx, hip_stream, __func__), N, C, K, d_unary_grad, d_f, d_out);
}

}  // extern "C"
