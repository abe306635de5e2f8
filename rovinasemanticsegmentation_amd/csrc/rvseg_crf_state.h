// The CRF state of a context and what rvseg_lattice.hip (the lattice's host side), rvseg_crf.hip (mean field, frame and
// cloud paths) and rvseg_crf_model.hip (the kept DenseCRF model) share.  Private to those three files; the functions are
// defined in rvseg_lattice.hip and rvseg_crf.hip.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "rvseg_crf.h"
#include "rvseg_pipeline.h"

namespace rvseg {

struct LatticeBufs {
    DevBuf state, tkeys, slot_to_id, vkeys, offsets, bary, nb1, nb2, csr_pw, csr_nrm, norm;
    DevBuf vstart;   // vstart | vend | counters (lattice_reserve)
    DevBuf keys_in, keys_out, vals_in, vals_out, sort_temp, scan_temp, fstart, vorder, block_hist;
    DevBuf r_desc, r_vl, r_info, r_small, r_verts, r_jb, r_trace;   // resident band schedule of the splat
    SplatResidentDev resident{};
    bool resident_on = false;
    LatticeDev dev{};
    SortBuffers sb{};
    long long n_entries = 0, n_points = 0;
    bool built = false;
    bool cleared = false;       // the build's memsets are already enqueued (crf_frames_build_begin)
    bool has_csr_nrm = false;   // per-entry normaliser (multi-kernel inference only)
};

// One pairwise term as the mean field runs it.  Potts, and a Diagonal whose entries are all equal, are the same term
// (Potts(w) == Diagonal(-w, .., -w) bit for bit).
struct TermPlan {
    int norm = RVSEG_NORMALIZE_SYMMETRIC;
    bool uniform = true;   // Potts or uniform Diagonal: out = fl(-w * t)
    float w = 0.f;
    bool matrix = false;
    size_t off = 0;        // first float of the term's compatibility in CrfState::compat (C, or C x C symmetric)
    int compat = RVSEG_COMPAT_POTTS;   // rvseg_compat_kind: the layout of the term's parameters and of their gradient
    int kernel = RVSEG_CONST_KERNEL;   // rvseg_kernel_kind and the feature dimension: the layout of the kernel parameters'
    int d = 0;                         // gradient (terms_prepare)
};

// What a kept model keeps of a term beside its lattice, for the kernel-parameter gradient: the ranks of every point (3 bits
// each in one word) and, for a DIAG or FULL kernel, the features as the caller passed them (f_, N x d).
// kparams: the kernel parameters the term's lattice was built from (has_kparams false: none, the features as passed).
struct TermKeep { DevBuf rank, feat; std::vector<float> kparams; bool has_kparams = false; };

// The DenseCRF model a context keeps between calls (rvseg_crf_model_*): term k on CrfState::lat[k], the compatibilities in
// CrfState::compat, the unary in memory of its own.  It lives until the next lattice build on the context.
struct CrfModel {
    bool valid = false;
    uint64_t serial = 0;       // names this model among all of the process (model_set); the in-place setters keep it
    int N = 0, C = 0;
    bool unary_is_energy = true;
    std::vector<TermPlan> plan;
    std::string replaced_by;   // the entry whose lattice build ended the model
    DevBuf unary;              // N x C, as the caller passed it
    // staging of the host entries only: an N x C input or in-out matrix, labels, the two energy vectors, KL values,
    // gradients, ground truth, class weights
    DevBuf q, labels, vec, kl, ug, cg, gt, cw;
    // staging of a host entry, the caller's memory in a device entry: an N x C output (work memory of the energies), Q[0 .. n]
    // (work memory of the gradient's forward pass), d_mul_Q (work memory of the gradient)
    DevBuf rows, qs, dq;
    // work memory (never the mean field's tmp): the energies' one-hot rows, the KL partials, the backward pass's b, tmp1, tmp2
    DevBuf onehot, partials, bgrad, tsum, tapp;
    DevBuf stats;              // 128 doubles of IoU sums + the objective's value (of a host entry)
    // the kernel-parameter gradient.  Per term: ranks and raw features.  Staging of the host entries: a, b (N x C), df / fg
    // (N x d), the gradient's doubles.  Work memory: a n, b n, K(b ..), K^T(a ..), X, ones, lbl_Q (N x C each), the two
    // lattice gradients and fg (N x d each), the d x d product
    TermKeep keep[8];
    DevBuf kg_a, kg_b, kg_out, kg_grad;
    DevBuf kg_an, kg_bn, kg_fa, kg_fb, kg_x, kg_ones, kg_lbl, kg_g1, kg_g2, kg_fg, kg_full;
    // a kept logistic unary (rvseg_crf_model_set_logistic): K > 0, f (N x K) and L (C x K) in memory of the model; staging of
    // the parameter gradient's C K doubles
    int K = 0;
    DevBuf lfeat, lmat, lgrad;
    PinnedBuf h_lmat;   // the source of L's asynchronous upload; lmat_ev: that upload has left it
    Event lmat_ev;
};

struct CrfState {
    std::vector<LatticeBufs> lat;  // one per pairwise kernel
    CrfModel model;                // rvseg_crf_model_*
    long long lattice_builds = 0;  // lattice_build calls on this context (rvseg_debug_lattice_builds)
    const char* entry = "";        // the C-ABI entry at work (crf_enter; the frame and cloud paths name themselves): CrfModel::replaced_by
    // two slots of mean-field scratch: a second label layer's mean field runs beside the first on its own stream
    struct { DevBuf val_a, val_b, tmp, qn; } scratch[2];
    DevBuf q, unary, feat, labels;
    // learned-model terms (rvseg_crf_infer_terms*): compatibilities of all terms, transformed features, logistic L
    DevBuf compat, kfeat, lmat;
    DevBuf learn_partials, lgrad;   // partials of the learning reductions; staging of rvseg_crf_logistic_gradient's result
    std::vector<float> h_compat;   // host copy of `compat` (the source of its asynchronous upload)
    Stream layer_stream;   // the second layer's stream; created together with its two events (second_stream)
    Event layer_fork, layer_join;
    // pinned read-back of a build: [0] M, [1] overflow, [2] longest vertex list, [3] frames the splat planner gave up on.
    // Slot 0 (words 0..3) belongs to the asynchronous frame builds (consumed by crf_frames_status), slot 1 (words 4..7)
    // to the synchronous entry points -- a cloud or host CRF call on the same context must not overwrite a frame
    // build's status that nobody has polled yet.
    PinnedBuf h_counters;   // int[8]
    Event counters_ev;
    bool counters_pending = false;
    rvseg_schedule_info info{};    // what the last build ran with (rvseg_last_schedule)
    int frame_vertices_seen = 0;   // vertices per frame of the last frame build whose status was read (0: none yet)
    int pending_frames = 0;        // frames of the build whose status is pending
    bool info_async = false;       // info.vertices / planner_fallback still travel with the pending frame-build status
};

// What one mean field reads and where it runs: the terms (term k on cs->lat[k]) with their compatibilities d_compat (may
// be null when every term is uniform with NORMALIZE_SYMMETRIC), the unary, the shape, the stream and the scratch slot
// (0 / 1; two layers may run side by side on two streams); timed: record stage marks (only one of two concurrent loops
// may: the marks are a sequence on ONE stream)
struct MfRun {
    const std::vector<TermPlan>& plan;
    const float* d_compat;
    ValueView unary;
    bool unary_is_energy;
    int C, N;
    long long n_points;
    hipStream_t s;
    int slot;
    bool timed;
};

// Where a traced step leaves the KL divergence of the Q it starts from: the term passes read the splat and blur the step
// needs anyway.  partials: [2 + n_terms][KL_MAX_BLOCKS] doubles.
struct KlTap { double* partials; };

// One pairwise term's lattice input: N x d features in host or device memory, the kernel parameters that transform them
// (pairwise.cpp:140-152; none for CONST_KERNEL or a null pointer) and the normaliser the term needs (rvseg_norm_kind)
// keep (a kept model's term only): where the point ranks and, for a DIAG or FULL kernel, a copy of the features go
// in_place (term_rebuild): the features ARE keep->feat, and the model the term belongs to stays live
struct TermInput {
    int d; const float* features; bool on_host; int kernel_type; const float* kernel_params; int norm; TermKeep* keep = nullptr;
    bool in_place = false;
};

// the input of a Potts term (the Segmenter's, the clouds', rvseg_crf_infer[_multi|_device], rvseg_lattice_build)
static inline TermInput potts_input(int d, const float* features, bool on_host) {
    return TermInput{d, features, on_host, RVSEG_CONST_KERNEL, nullptr, RVSEG_NORMALIZE_SYMMETRIC, nullptr};
}

// ---- rvseg_lattice.hip (each is described where it is defined); not exported by the library ----
#pragma GCC visibility push(hidden)
LatticeBufs& lattice_at(CrfState* cs, int k);
rvseg_status lattice_raise_capacity(rvseg_ctx* ctx, Pipeline* im, int N);
rvseg_status lattice_prepare(rvseg_ctx* ctx, LatticeBufs& b, int d, int N, int n_frames, bool safe, int vertices_per_frame_seen = 0,
                             bool frame_ids = false);
rvseg_status values_reserve(rvseg_ctx* ctx, CrfState* cs, long long m_bound, int C, int slot = 0);
rvseg_status second_stream(rvseg_ctx* ctx, CrfState* cs);
rvseg_status lattice_clear(rvseg_ctx* ctx, LatticeBufs& b, hipStream_t s);
void model_replaced(CrfState* cs);
rvseg_status lattice_build(rvseg_ctx* ctx, CrfState* cs, LatticeBufs& b, const FeatureSource& fs, hipStream_t s,
                           int norm_kind = RVSEG_NORMALIZE_SYMMETRIC, bool ends_model = true);
rvseg_status counters_readback(rvseg_ctx* ctx, CrfState* cs, const LatticeBufs& b, int slot, hipStream_t s);
void counters_to_info(CrfState* cs, const int* h);
rvseg_status ensure_csr_nrm(rvseg_ctx* ctx, LatticeBufs& b, hipStream_t s);
rvseg_status build_lattices(rvseg_ctx* ctx, CrfState* cs, int N, int n, const TermInput* terms, hipStream_t s, int first = 0,
                            int* vertices = nullptr);
#pragma GCC visibility pop

// ---- rvseg_crf.hip (each is described where it is defined); not exported by the library ----
#pragma GCC visibility push(hidden)
rvseg_status crf_enter(rvseg_ctx* ctx, CrfState** cs_out, const char* entry);
rvseg_status terms_prepare(rvseg_ctx* ctx, CrfState* cs, int N, int C, int n_terms, const rvseg_crf_term* terms, bool on_host,
                           std::vector<TermPlan>& plan, hipStream_t s, TermKeep* keep = nullptr);
rvseg_status term_rebuild(rvseg_ctx* ctx, CrfState* cs, int k, const float* kernel_params, hipStream_t s);
void plan_compat(int C, int compat, const float* params, TermPlan& tp, float* hc /* C, or C x C for a Matrix */);
bool term_pre(const TermPlan& t);
bool term_post(const TermPlan& t);
rvseg_status mf_scratch(rvseg_ctx* ctx, CrfState* cs, const MfRun& r);
rvseg_status mf_entry_norms(rvseg_ctx* ctx, CrfState* cs, const MfRun& r);
void mf_start(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, const ValueView& Q);
void mf_step(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, const ValueView& Q, const KlTap* tap = nullptr);
void kl_unary_parts(rvseg_ctx* ctx, const MfRun& r, const float* Q, const KlTap& tap);
void kl_term_part(rvseg_ctx* ctx, CrfState* cs, const MfRun& r, int k, const float* blurred, const float* Q, const KlTap& tap);
#pragma GCC visibility pop

}  // namespace rvseg
