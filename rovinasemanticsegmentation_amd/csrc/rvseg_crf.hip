// CRF orchestration: lattice construction, normaliser, mean-field loop; the C-ABI entry points rvseg_crf_infer* /
// rvseg_lattice_* and the CRF stages of the frame pipeline and of the cloud path.  The kept DenseCRF model and learning on it
// are in rvseg_crf_model.hip; rvseg_crf_state.h holds what the two files share.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

static int ceil_log2(unsigned long long v) {
    int b = 0;
    while ((1ull << b) < v) b++;
    return b;
}

// the vector of lattices grown to hold lattice k (one per pairwise term; the frame path and the clouds use lattice 0)
static LatticeBufs& lattice_at(CrfState* cs, int k) {
    if ((int)cs->lat.size() <= k) cs->lat.resize((size_t)k + 1);
    return cs->lat[k];
}

// the per-frame capacity the context asks for: params.lattice_capacity_log2 > 0 as given, else 2^12 (the Segmenter
// kernel yields ~300 vertices per synthetic 640x480 frame).  Every overflow seen on this context has raised cap_boost
// by 3 (x8 slots), so a scene that does not fit is paid for once.
static int configured_capacity_log2(const rvseg_ctx* ctx) {
    const int want = ctx->params.lattice_capacity_log2 > 0 ? ctx->params.lattice_capacity_log2 : 12;
    return want + (ctx->impl ? ctx->impl->cap_boost : 0);
}

// per-frame hash capacity: the configured one; params.lattice_capacity_log2 < 0 or `safe` = enough for every point to
// own d+1 private vertices at load factor 1/2, which also bounds the configured one
static int capacity_log2_per_frame(const rvseg_ctx* ctx, int Npad, int d, bool safe) {
    const int safe_log2 = ceil_log2(2ull * (unsigned long long)Npad * (d + 1));
    if (safe || ctx->params.lattice_capacity_log2 < 0) return safe_log2;
    return std::min(configured_capacity_log2(ctx), safe_log2);
}

static bool capacity_is_worst_case(const rvseg_ctx* ctx, int N, int d) {
    const int Npad = (N + 3) / 4 * 4;
    return capacity_log2_per_frame(ctx, Npad, d, false) == capacity_log2_per_frame(ctx, Npad, d, true);
}

// Does the resident band schedule pay for a chunk of this shape?  It wins where the list-major walk is bound by the
// bytes it re-reads (many frames) and loses where a frame's chains set the time (few frames, a cloud) or where its
// planner -- whose work grows with the vertices of a frame -- costs more than the splat saves.  Measured crossovers
// (profiles/r03_schedule_sweep.json, step time of the whole frame path, 640x480 frames with holes): ~360 vertices per
// frame (the flat synthetic scene): between 16 and 32 frames (resident 5.14 / 7.53 / 12.59 ms against 4.85 / 7.94 /
// 13.97 at 16 / 32 / 64 frames); ~2 320 vertices per frame (the deep scene): between 32 and 64 frames (12.35 / 18.70
// against 10.52 / 19.22).  A line through the two crossovers: resident from 5.6 M points + 4 900 points per vertex of a
// frame -- moved to 6.9 M + 4 900 per vertex when the list-major walk got scan blocks for its longest lists (24 flat
// frames: list-major 5.49 ms against 6.04 resident; 32 frames: 7.15 against 7.03).  The vertex count is a MEASURED quantity: that of the context's previous lattice build (read back with its
// status); before any build has been seen, the flat scene's.
static bool resident_pays(int n_frames, int N, int vertices_per_frame_seen) {
    const long long vpf = vertices_per_frame_seen > 0 ? vertices_per_frame_seen : 360;
    return n_frames >= 2 && (long long)n_frames * N >= 6900000ll + 4900ll * vpf;
}

// Sizes of one lattice over n_frames frames of N points, from plain integers: hash slots of all frames, bound of the
// vertex count, points, entries = P (d+1)
struct LatticeLimits { int Npad, cap_f_log2, key_bits; unsigned long long cap, m_bound; long long P, E; };

static rvseg_status lattice_limits(int d, int N, int n_frames, int cap_f_log2, LatticeLimits& m, const char** err) {
    if (n_frames > 1022) { *err = "at most 1022 frames per chunk (lower max_batch)"; return RVSEG_ERR_INVALID_ARG; }   // 10-bit frame field of the launch-order sort key
    m.Npad = (N + 3) / 4 * 4;
    m.cap_f_log2 = cap_f_log2;
    m.cap = (unsigned long long)n_frames << cap_f_log2;
    if (m.cap >= (1ull << 31)) { *err = "lattice hash capacity too large (lower max_batch or lattice_capacity_log2)"; return RVSEG_ERR_CAPACITY; }
    const unsigned long long worst = (unsigned long long)m.Npad * n_frames * (d + 1);
    m.m_bound = std::min<unsigned long long>(m.cap / 2 + 2, worst);
    m.P = (long long)N * n_frames;
    m.E = m.P * (d + 1);
    if (m.E >= (1ll << 32) || m.m_bound >= (1ull << 31)) { *err = "too many lattice entries for 32-bit indices"; return RVSEG_ERR_CAPACITY; }
    m.key_bits = std::max(1, ceil_log2(m.m_bound));
    return RVSEG_OK;
}

#define RV_RES(buf, bytes) do { const rvseg_status st_ = dev_reserve(ctx, buf, (size_t)(bytes)); if (st_ != RVSEG_OK) return st_; } while (0)

// the lattice's buffers (all but block_hist and the resident schedule's, whose sizes follow from the filled LatticeDev)
static rvseg_status lattice_reserve(rvseg_ctx* ctx, LatticeBufs& b, const LatticeLimits& m, int d, int n_frames) {
    const unsigned long long cap = m.cap, m_bound = m.m_bound, E = (unsigned long long)m.E;
    RV_RES(b.state, cap * 4);
    RV_RES(b.tkeys, cap * 16);
    RV_RES(b.slot_to_id, cap * 4);
    RV_RES(b.fstart, ((size_t)n_frames + 1) * 4);
    RV_RES(b.vkeys, m_bound * 16);
    RV_RES(b.offsets, E * 4);   // (the 16-bit form uses half of it: a context that leaves the counting-sort path needs nothing new)
    RV_RES(b.bary, E * 4);
    RV_RES(b.nb1, m_bound * (d + 1) * 4);
    RV_RES(b.nb2, m_bound * (d + 1) * 4);
    RV_RES(b.csr_pw, E * 8);
    RV_RES(b.vstart, (2 * m_bound + 4) * 4);   // vstart | vend | counters: one allocation, zeroed by ONE memset per build
    RV_RES(b.vorder, m_bound * 4);
    RV_RES(b.norm, m.P * 4);
    const unsigned long long SE = std::max(E, m_bound);  // also sorts the vertex order
    RV_RES(b.keys_in, SE * 4);
    RV_RES(b.keys_out, SE * 4);
    RV_RES(b.vals_in, SE * 4);
    RV_RES(b.vals_out, SE * 4);
    b.sb.temp_bytes = std::max(sort_temp_bytes(m.E, m.key_bits), sort_temp_bytes((long long)m_bound, 32));
    RV_RES(b.sort_temp, b.sb.temp_bytes);
    b.sb.scan_temp_bytes = scan_temp_bytes((unsigned)cap);
    RV_RES(b.scan_temp, b.sb.scan_temp_bytes);
    return RVSEG_OK;
}

// LatticeDev / SortBuffers over the reserved buffers, and the CSR path: block_hist where the counting sort serves
// frame_ids: the frame path's lattice (d = 6, table partitioned by frame) may keep 16-bit frame-local ids (LatticeDev::ids16)
static rvseg_status lattice_fill(rvseg_ctx* ctx, LatticeBufs& b, const LatticeLimits& m, int d, int N, int n_frames, bool frame_ids) {
    LatticeDev& L = b.dev;
    L.d = d; L.N = N; L.Npad = m.Npad; L.n_frames = n_frames;
    L.cap_f_log2 = (unsigned)m.cap_f_log2;
    L.cap_f_mask = (1u << m.cap_f_log2) - 1u;
    L.cap_total = (unsigned)m.cap;
    L.m_bound = (int)m.m_bound;
    // diagonal of E (permutohedral.cpp:177-182): float inv_std_dev; scale = 1/sqrt((i+2)(i+1)) * inv_std_dev
    const float inv_std_dev = (float)(std::sqrt(2.0 / 3.0) * (d + 1));
    for (int i = 0; i < 8; i++) L.scale[i] = i < d ? (float)(1.0 / std::sqrt((double)((i + 2) * (i + 1))) * inv_std_dev) : 0.f;
    L.state = b.state.as<int>(); L.tkeys = b.tkeys.as<unsigned long long>(); L.slot_to_id = b.slot_to_id.as<int>();
    L.fstart = b.fstart.as<int>(); L.vkeys = b.vkeys.as<unsigned long long>();
    L.offsets = b.offsets.as<int>(); L.bary = b.bary.as<float>();
    L.nb1 = b.nb1.as<int>(); L.nb2 = b.nb2.as<int>();
    L.csr_pw = b.csr_pw.as<uint2>(); L.csr_nrm = nullptr;
    b.has_csr_nrm = false;
    L.vstart = b.vstart.as<unsigned>(); L.vend = L.vstart + m.m_bound; L.counters = reinterpret_cast<int*>(L.vend + m.m_bound);
    L.vorder = b.vorder.as<unsigned>(); L.norm = b.norm.as<float>();
    L.n_groups = n_frames >= 8 ? 8 : 1;
    b.sb.keys_in = b.keys_in.as<unsigned>(); b.sb.keys_out = b.keys_out.as<unsigned>();
    b.sb.vals_in = b.vals_in.as<unsigned>(); b.sb.vals_out = b.vals_out.as<unsigned>();
    b.sb.temp = b.sort_temp.p; b.sb.key_bits = m.key_bits;   // (temp_bytes / scan_temp_bytes: lattice_reserve)
    b.sb.scan_temp = b.scan_temp.p;
    b.sb.block_hist = nullptr;
    L.bh = nullptr; L.wbpf = 0;
    L.group_vertices = ctx->sched.group_vertices;
    L.ordered_sum_scan = ctx->sched.serial_chains ? 0 : 1;
    L.heavy_from = 0;
    L.scan_ranks = 0;
    // Wave-blocks of the counting sort.  Its [wave-block][vertex] count matrix is written once and read three times, and
    // its size is points / cs_pix x vertices: 1024-point blocks cut a 64-frame step by 0.15 ms (deep scene: 1.3 ms; 32
    // frames 0.16, 16 frames 0.11), but a single frame then has only 300 waves to sort with (+0.07 ms) and 8 frames
    // gain nothing, so small launches keep 256 (sweep of 256 .. 4096 over 8 - 64 frames: scratch-style script in
    // DESIGN.md section 4; results are identical for every size)
    L.cs_pix = ctx->sched.csr_block > 0 ? ctx->sched.csr_block : (n_frames <= 8 ? 256 : 1024);
    L.ids16 = 0;
    if (csr_fast_path(L)) {
        RV_RES(b.block_hist, csr_fast_bytes(L));
        b.sb.block_hist = b.block_hist.as<unsigned>();
        L.bh = b.sb.block_hist;
        L.wbpf = (N + L.cs_pix - 1) / L.cs_pix;
        // at most 8192 slots and 4096 vertices per frame: frame-local slots and ids fit 16 bits
        L.ids16 = frame_ids && d == 6 ? 1 : 0;
    }
    b.n_entries = m.E; b.n_points = m.P;
    b.built = false;
    b.cleared = false;
    return RVSEG_OK;
}

// Resident band schedule of the mean-field splat: chunks of many frames, whose splat is
// bound by the bytes the list-major walk re-reads.  All n_frames x B blocks have to be on the chip together.
static rvseg_status resident_prepare(rvseg_ctx* ctx, LatticeBufs& b, int vertices_per_frame_seen) {
    const LatticeDev& L = b.dev;
    const int d = L.d, N = L.N, n_frames = L.n_frames;
    const rvseg_schedule& sc = ctx->sched;
    b.resident_on = false;
    // Worth it where the list-major walk is bound by the bytes it re-reads rather than by its longest chain
    // ("where it pays"): see resident_pays().  sched.splat = 2 forces it, 1 forbids it.
    const bool wanted = sc.splat == 2 || (sc.splat == 0 && resident_pays(n_frames, N, vertices_per_frame_seen));
    const int chunk = sc.resident_chunk == 64 ? 64 : 128;
    const int capacity = resident_block_capacity(chunk);
    // one block per CU measured best (the tile loop is bound by its own barrier-coupled latencies, a second block on
    // the CU slows both): B = CUs / frames, at least 2, at most 12
    int B = sc.resident_blocks > 0 ? sc.resident_blocks : (n_frames > 0 ? resident_cu_count() / n_frames : 0);
    if (sc.resident_blocks <= 0) B = B < 2 ? 2 : (B > 12 ? 12 : B);
    B = B > RES_MAXB ? RES_MAXB : B;
    if (!(wanted && L.bh && d == 6 && B >= 2 && (long long)n_frames * B <= capacity &&
          7ll * N < (1ll << 24) && (long long)L.wbpf * L.cs_pix <= 8192ll * RES_MAX_BANDS && L.cs_pix <= 4096)) return RVSEG_OK;   // (bands stay under 16 384 points: chunk counts fit 8 bits)
    SplatResidentDev& R = b.resident;
    R.B = B;
    R.band_wb = sc.resident_band < 1 ? 1 : (sc.resident_band > 32 ? 32 : sc.resident_band);
    R.band_wb = std::max(1, R.band_wb * 256 / L.cs_pix);   // rvseg_schedule.resident_band counts 256 points
    R.n_bands = (L.wbpf + R.band_wb - 1) / R.band_wb;
    while (R.n_bands > RES_MAX_BANDS) { R.band_wb *= 2; R.n_bands = (L.wbpf + R.band_wb - 1) / R.band_wb; }
    R.window = sc.resident_window;
    R.chunk_log2 = chunk == 128 ? 7 : 6;
    R.cap_tiles = (unsigned)(N / 8 + 1024);
    if (sc.resident_cap_tiles > 0 && (unsigned)sc.resident_cap_tiles < R.cap_tiles) R.cap_tiles = (unsigned)sc.resident_cap_tiles;
    const size_t small = (16 + (size_t)n_frames * (RES_MAXB + 1) + (size_t)n_frames * RES_MAXB + 2 * (size_t)n_frames * RES_MAXB) * 4;
    RV_RES(b.r_desc, (size_t)n_frames * 7 * R.cap_tiles * 4);
    RV_RES(b.r_vl, (size_t)n_frames * 7 * R.cap_tiles * 2);
    RV_RES(b.r_info, (size_t)n_frames * R.cap_tiles * 4);
    RV_RES(b.r_small, small);
    RV_RES(b.r_verts, (size_t)n_frames * RES_MAXB * RES_MAX_OWNV * 2);
    RV_RES(b.r_jb, (size_t)n_frames * RES_MAXB * (R.n_bands + 1) * 4);
    R.tdesc = b.r_desc.as<unsigned>(); R.tvl = b.r_vl.as<unsigned short>(); R.tinfo = b.r_info.as<unsigned>();
    unsigned* sm = b.r_small.as<unsigned>();
    R.flags = reinterpret_cast<int*>(sm); sm += 16;
    R.blk_tile0 = sm; sm += (size_t)n_frames * (RES_MAXB + 1);
    R.blk_nown = sm; sm += (size_t)n_frames * RES_MAXB;
    R.prog = sm;
    R.blk_verts = b.r_verts.as<unsigned short>();
    R.jb_tile = b.r_jb.as<unsigned>();
    R.trace = nullptr;
    if (sc.trace) {
        RV_RES(b.r_trace, (size_t)n_frames * RES_MAXB * 64);
        R.trace = b.r_trace.as<unsigned long long>();
    }
    b.resident_on = true;
    return RVSEG_OK;
}
#undef RV_RES

// limits, buffers, LatticeDev and the splat's schedule of a lattice of n_frames x N points; `safe`: at the capacity that
// cannot overflow.  vertices_per_frame_seen / frame_ids: the frame path's (resident_pays, LatticeDev::ids16)
static rvseg_status lattice_prepare(rvseg_ctx* ctx, LatticeBufs& b, int d, int N, int n_frames, bool safe, int vertices_per_frame_seen = 0,
                                    bool frame_ids = false) {
    if (d < 1 || d > 7) { ctx->err = "feature dimension must be in [1,7]"; return RVSEG_ERR_INVALID_ARG; }
    LatticeLimits m;
    const char* err = nullptr;
    rvseg_status st = lattice_limits(d, N, n_frames, capacity_log2_per_frame(ctx, (N + 3) / 4 * 4, d, safe), m, &err);
    if (st != RVSEG_OK) { ctx->err = err; return st; }
    if ((st = lattice_reserve(ctx, b, m, d, n_frames)) != RVSEG_OK) return st;
    if ((st = lattice_fill(ctx, b, m, d, N, n_frames, frame_ids)) != RVSEG_OK) return st;
    return resident_prepare(ctx, b, vertices_per_frame_seen);
}

static rvseg_status values_reserve(rvseg_ctx* ctx, CrfState* cs, long long m_bound, int C, int slot = 0) {
    rvseg_status st;
    if ((st = dev_reserve(ctx, cs->scratch[slot].val_a, (size_t)m_bound * C * 4)) != RVSEG_OK) return st;
    if ((st = dev_reserve(ctx, cs->scratch[slot].val_b, (size_t)m_bound * C * 4)) != RVSEG_OK) return st;
    return RVSEG_OK;
}

// the context's second CRF stream (the second label layer's mean field; the splat planner beside the normaliser)
static rvseg_status second_stream(rvseg_ctx* ctx, CrfState* cs) {
    if (cs->layer_stream) return RVSEG_OK;
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    Stream stream;
    Event fork, join;
    RV_HIP(ctx, stream_create(stream, hipStreamNonBlocking, prio_hi));
    RV_HIP(ctx, event_create(fork, hipEventDisableTiming));
    RV_HIP(ctx, event_create(join, hipEventDisableTiming));
    cs->layer_stream = std::move(stream);
    cs->layer_fork = std::move(fork);
    cs->layer_join = std::move(join);
    return RVSEG_OK;
}

// Permutohedral::init + the normaliser of DenseKernel::initLattice (pairwise.cpp:40-56)
static rvseg_status lattice_clear(rvseg_ctx* ctx, LatticeBufs& b, hipStream_t s) {
    const LatticeDev& L = b.dev;
    RV_HIP(ctx, hipMemsetAsync(L.state, 0xFF, (size_t)L.cap_total * 4, s));
    RV_HIP(ctx, hipMemsetAsync(L.vstart, 0, (2 * (size_t)L.m_bound + 4) * 4, s));   // vstart, vend, counters
    b.cleared = true;
    return RVSEG_OK;
}

void model_replaced(CrfState* cs) {
    if (!cs->model.valid) return;
    cs->model.valid = false;
    cs->model.replaced_by = cs->entry;
}

// norm_kind: the normaliser the term needs (rvseg_norm_kind): SYMMETRIC 1/sqrt(n + 1e-20), BEFORE / AFTER 1/(n + 1e-20),
// NONE none at all (pairwise.cpp:40-56; the mean norm NO_NORMALIZATION computes is never read in inference)
// ends_model: false only for the rebuild of a kept model's own term in place (term_rebuild)
static rvseg_status lattice_build(rvseg_ctx* ctx, CrfState* cs, LatticeBufs& b, const FeatureSource& fs, hipStream_t s,
                                  int norm_kind = RVSEG_NORMALIZE_SYMMETRIC, bool ends_model = true) {
    const LatticeDev& L = b.dev;
    cs->lattice_builds++;
    if (ends_model) model_replaced(cs);   // a kept DenseCRF model ends with any other lattice build on its context
    if (!b.cleared) { rvseg_status stc = lattice_clear(ctx, b, s); if (stc != RVSEG_OK) return stc; }
    b.cleared = false;
    const bool trace = ctx->sched.trace >= 2;
    auto tr = [&](const char* what) {
        if (!trace) return;
        hipError_t e = hipStreamSynchronize(s);
        std::fprintf(stderr, "[rvseg] %s: %s (N=%d d=%d cap_f=%u m_bound=%d)\n", what, hipGetErrorString(e), L.N, L.d, L.cap_f_mask + 1, L.m_bound);
    };
    tr("memsets");
    launch_lattice_points(L, fs, s);
    tr("points");
    // the splat's band schedule needs the lists' bounds (count / scan) and the launch order, not the lists themselves: it
    // is planned beside the scatter and the normaliser
    launch_lattice_finish(L, b.sb, b.n_entries, s, /*defer_scatter=*/b.resident_on);
    tr("finish");
    rvseg_status st;
    bool plan_forked = false;
    if (b.resident_on) {
        if ((st = second_stream(ctx, cs)) != RVSEG_OK) return st;
        RV_HIP(ctx, hipEventRecord(cs->layer_fork, s));
        RV_HIP(ctx, hipStreamWaitEvent(cs->layer_stream, cs->layer_fork, 0));
        RV_HIP(ctx, hipMemsetAsync(b.resident.prog, 0, 2 * (size_t)L.n_frames * RES_MAXB * 4, cs->layer_stream));
        launch_resident_plan(L, b.resident, cs->layer_stream);
        RV_HIP(ctx, hipEventRecord(cs->layer_join, cs->layer_stream));
        plan_forked = true;
        tr("resident plan");
        launch_csr_scatter(L, b.sb, s);
    }
    st = values_reserve(ctx, cs, L.m_bound, 1);
    if (st != RVSEG_OK) { if (plan_forked) (void)hipStreamWaitEvent(s, cs->layer_join, 0); return st; }
    // norm = lattice.compute(ones) through seqCompute (1 row), then 1/sqrt(norm + 1e-20) (or 1/(norm + 1e-20))
    if (norm_kind != RVSEG_NO_NORMALIZATION) {
        ValueView none{nullptr, 0, 0};
        launch_splat(L, none, 1, 2, cs->scratch[0].val_a.as<float>(), s);
        float* blurred = launch_blur(L, 1, true, false, cs->scratch[0].val_a.as<float>(), cs->scratch[0].val_b.as<float>(), s, true);
        launch_slice(L, 1, true, norm_kind == RVSEG_NORMALIZE_SYMMETRIC ? 1 : 3, blurred, 0.f, L.norm, b.n_points, s);
        tr("normaliser");
    }
    if (plan_forked) RV_HIP(ctx, hipStreamWaitEvent(s, cs->layer_join, 0));
    RV_LAUNCH_OK(ctx);
    b.built = true;
    rvseg_schedule_info& inf = cs->info;
    inf.splat = b.resident_on ? 2 : 1;
    inf.planner_fallback = -1;
    inf.csr_path = L.bh ? 1 : 2;
    inf.n_frames = L.n_frames;
    inf.points_per_frame = L.N;
    inf.vertices = -1;
    inf.longest_list = -1;
    inf.resident_blocks = b.resident_on ? b.resident.B : 0;
    inf.resident_band = b.resident_on ? b.resident.band_wb : 0;
    inf.resident_chunk = b.resident_on ? (1 << b.resident.chunk_log2) : 0;
    inf.capacity_log2 = (int)L.cap_f_log2;
    return RVSEG_OK;
}

// enqueues the read-back of a build's counters (+ the planner's flag) into pinned slot `slot` (0: async frame builds,
// 1: synchronous entry points)
static rvseg_status counters_readback(rvseg_ctx* ctx, CrfState* cs, const LatticeBufs& b, int slot, hipStream_t s) {
    int* h = cs->h_counters.as<int>() + 4 * slot;
    RV_HIP(ctx, hipMemcpyAsync(h, b.dev.counters, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipMemcpyAsync(h + 2, b.dev.counters + 3, sizeof(int), hipMemcpyDeviceToHost, s));
    if (b.resident_on) RV_HIP(ctx, hipMemcpyAsync(h + 3, b.resident.flags, sizeof(int), hipMemcpyDeviceToHost, s));
    else h[3] = 0;   // (host write; no copy of this build touches the word)
    return RVSEG_OK;
}

// what a read-back slot tells rvseg_last_schedule about the build cs->info describes
static void counters_to_info(CrfState* cs, const int* h) {
    cs->info.vertices = h[0];
    cs->info.longest_list = h[2];
    cs->info.planner_fallback = h[3];
    cs->info_async = false;
}

// synchronous read of the build counters (host entry points): out = M, overflow, longest vertex list
static rvseg_status lattice_counters(rvseg_ctx* ctx, CrfState* cs, const LatticeBufs& b, hipStream_t s, int out[3]) {
    rvseg_status st = counters_readback(ctx, cs, b, 1, s);
    if (st != RVSEG_OK) return st;
    RV_HIP(ctx, hipStreamSynchronize(s));
    const int* h = cs->h_counters.as<int>() + 4;
    out[0] = h[0]; out[1] = h[1]; out[2] = h[2];
    counters_to_info(cs, h);
    return RVSEG_OK;
}

// per-entry copy of the normaliser for the unfused splat (MODE 1); filled once per lattice
rvseg_status ensure_csr_nrm(rvseg_ctx* ctx, LatticeBufs& b, hipStream_t s) {
    if (b.has_csr_nrm) return RVSEG_OK;
    rvseg_status st = dev_reserve(ctx, b.csr_nrm, (size_t)b.n_entries * 4);
    if (st != RVSEG_OK) return st;
    b.dev.csr_nrm = b.csr_nrm.as<float>();
    launch_csr_norm(b.dev, b.n_entries, s);
    b.has_csr_nrm = true;
    return RVSEG_OK;
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
    if (h[1]) {
        const FrameGeom& g = im->geom;
        const bool was_worst = capacity_is_worst_case(ctx, g.W * g.H, 6);
        // x8 slots per step, but stop at 2^13 on the way up: the largest capacity the counting-sort CSR path serves
        // (real scenes with a deep range have ~2 000 vertices per frame; beyond it the radix-sort path takes over)
        const int cur = configured_capacity_log2(ctx);
        im->cap_boost += cur < 13 ? std::min(3, 13 - cur) : 3;
        ctx->err = was_worst ? "lattice hash table overflowed at its worst-case capacity (internal error)"
                             : "lattice hash table overflowed: the outputs of that call are invalid; the context has raised its "
                               "capacity (x8 slots per frame), repeat the call (or set params.lattice_capacity_log2 = -1)";
        return RVSEG_ERR_CAPACITY;
    }
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

// One pairwise term's lattice input: N x d features in host or device memory, the kernel parameters that transform them
// (pairwise.cpp:140-152; none for CONST_KERNEL or a null pointer) and the normaliser the term needs (rvseg_norm_kind)
// keep (a kept model's term only): where the point ranks and, for a DIAG or FULL kernel, a copy of the features go
// in_place (term_rebuild): the features ARE keep->feat, and the model the term belongs to stays live
struct TermInput {
    int d; const float* features; bool on_host; int kernel_type; const float* kernel_params; int norm; TermKeep* keep = nullptr;
    bool in_place = false;
};

static TermInput potts_input(int d, const float* features, bool on_host) {
    return TermInput{d, features, on_host, RVSEG_CONST_KERNEL, nullptr, RVSEG_NORMALIZE_SYMMETRIC, nullptr};
}

// Permutohedral::init + normaliser of term `t` on lattice `lb` (host features are copied into cs->feat, kernel
// parameters applied into cs->kfeat), then the counters, read back with one stream synchronisation
static rvseg_status build_lattice(rvseg_ctx* ctx, CrfState* cs, LatticeBufs& lb, int N, const TermInput& t, bool safe, hipStream_t s, int cnt[3]) {
    rvseg_status st;
    if ((st = lattice_prepare(ctx, lb, t.d, N, 1, safe)) != RVSEG_OK) return st;
    const float* f = t.features;
    if (t.on_host) {
        if ((st = dev_reserve(ctx, cs->feat, (size_t)N * t.d * 4)) != RVSEG_OK) return st;
        RV_HIP(ctx, hipMemcpyAsync(cs->feat.p, t.features, (size_t)N * t.d * 4, hipMemcpyHostToDevice, s));
        f = cs->feat.as<float>();
    }
    if (t.keep && t.kernel_type != RVSEG_CONST_KERNEL && !t.in_place) {   // f_ of the kernel-parameter gradient
        if ((st = dev_reserve(ctx, t.keep->feat, (size_t)N * t.d * 4)) != RVSEG_OK) return st;
        RV_HIP(ctx, hipMemcpyAsync(t.keep->feat.p, f, (size_t)N * t.d * 4, hipMemcpyDeviceToDevice, s));
    }
    if (t.kernel_params && t.kernel_type != RVSEG_CONST_KERNEL) {
        KernelParams kp{};
        const int np = t.kernel_type == RVSEG_DIAG_KERNEL ? t.d : t.d * t.d;
        for (int i = 0; i < np; i++) kp.p[i] = t.kernel_params[i];
        if ((st = dev_reserve(ctx, cs->kfeat, (size_t)N * t.d * 4)) != RVSEG_OK) return st;
        launch_kernel_params(f, N, t.d, t.kernel_type, kp, cs->kfeat.as<float>(), s);
        f = cs->kfeat.as<float>();
    }
    FeatureSource fs{};
    fs.feat = f;   // (mode 0)
    if ((st = lattice_build(ctx, cs, lb, fs, s, t.norm, !t.in_place)) != RVSEG_OK) return st;
    if (t.keep) {   // the ranks, from the features the lattice was built from
        if ((st = dev_reserve(ctx, t.keep->rank, (size_t)N * 4)) != RVSEG_OK) return st;
        launch_point_ranks(lb.dev, f, t.keep->rank.as<unsigned>(), s);
        RV_LAUNCH_OK(ctx);
    }
    return lattice_counters(ctx, cs, lb, s, cnt);
}

// The lattices of n terms over N points, term k on cs->lat[k], with the overflow retry of the synchronous entry points:
// a hash overflow of any term stops the attempt, and ALL terms are rebuilt once at the safe capacity, which cannot
// overflow.  cnt (optional): the counters of the last lattice (M, overflow, longest list).
static rvseg_status build_lattices(rvseg_ctx* ctx, CrfState* cs, int N, int n, const TermInput* terms, hipStream_t s, int* cnt = nullptr) {
    if (n > 0) lattice_at(cs, n - 1);
    int c[3] = {0, 0, 0};
    for (int attempt = 0; attempt < 2; attempt++) {
        c[1] = 0;
        for (int k = 0; k < n && !c[1]; k++) {
            rvseg_status st = build_lattice(ctx, cs, cs->lat[k], N, terms[k], attempt == 1, s, c);
            if (st != RVSEG_OK) return st;
        }
        if (cnt) std::memcpy(cnt, c, sizeof(c));
        if (!c[1]) return RVSEG_OK;
    }
    ctx->err = "lattice hash table overflow";
    return RVSEG_ERR_CAPACITY;
}

// rvseg_crf_model_set_kernel: term k of the live model rebuilt on cs->lat[k] from the raw features the model keeps, with new
// kernel parameters (host; null: none) -- lattice, normaliser, point ranks and, where the term had one, the per-entry
// normaliser.  A hash overflow rebuilds this term once at the safe capacity.  No other lattice is touched.
rvseg_status term_rebuild(rvseg_ctx* ctx, CrfState* cs, int k, const float* kernel_params, hipStream_t s) {
    CrfModel& m = cs->model;
    const TermPlan& tp = m.plan[k];
    LatticeBufs& lb = cs->lat[k];
    const bool entry_norms = lb.has_csr_nrm;
    TermInput in{tp.d, m.keep[k].feat.as<float>(), false, tp.kernel, kernel_params, tp.norm, &m.keep[k], true};
    int c[3] = {0, 0, 0};
    for (int attempt = 0; attempt < 2; attempt++) {
        rvseg_status st = build_lattice(ctx, cs, lb, m.N, in, attempt == 1, s, c);
        if (st != RVSEG_OK) { model_replaced(cs); return st; }   // (a lattice half built: the model is gone)
        if (!c[1]) return entry_norms ? ensure_csr_nrm(ctx, lb, s) : RVSEG_OK;
    }
    model_replaced(cs);
    ctx->err = "lattice hash table overflow";
    return RVSEG_ERR_CAPACITY;
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

rvseg_status rvseg_lattice_build(rvseg_ctx* ctx, const float* features, int32_t N, int32_t d, int32_t* offsets_out,
                                 float* bary_out, int16_t* keys_out, int32_t keys_capacity, int32_t* M_out) {
    CrfState* cs;
    rvseg_status st = crf_enter(ctx, &cs, __func__);
    if (st != RVSEG_OK) return st;
    if (!features || N <= 0 || !M_out) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    hipStream_t s = ctx->stream;
    int cnt[3] = {0, 0, 0};
    const TermInput in = potts_input(d, features, true);
    if ((st = build_lattices(ctx, cs, N, 1, &in, s, cnt)) != RVSEG_OK) return st;
    const LatticeBufs& lb = cs->lat[0];
    const int M = cnt[0];
    *M_out = M;
    const size_t E = (size_t)N * (d + 1);
    if (offsets_out) RV_HIP(ctx, hipMemcpyAsync(offsets_out, lb.dev.offsets, E * 4, hipMemcpyDeviceToHost, s));
    if (bary_out) RV_HIP(ctx, hipMemcpyAsync(bary_out, lb.dev.bary, E * 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    if (keys_out) {
        if (keys_capacity < M) { ctx->err = "keys_out too small"; return RVSEG_ERR_INVALID_ARG; }
        std::vector<int16_t> k8((size_t)M * 8);
        RV_HIP(ctx, hipMemcpy(k8.data(), lb.dev.vkeys, (size_t)M * 16, hipMemcpyDeviceToHost));
        for (int i = 0; i < M; i++)
            for (int k = 0; k < d; k++) keys_out[(size_t)i * d + k] = k8[(size_t)i * 8 + k];
    }
    return RVSEG_OK;
}

rvseg_status rvseg_lattice_neighbours(rvseg_ctx* ctx, int32_t* n1_out, int32_t* n2_out, uint32_t* csr_point,
                                      uint32_t* vstart, uint32_t* vend) {
    CrfState* cs;
    rvseg_status st = crf_enter(ctx, &cs, __func__);
    if (st != RVSEG_OK) return st;
    if (cs->lat.empty() || !cs->lat[0].built || cs->lat[0].dev.n_frames != 1) { ctx->err = "no lattice built on this context"; return RVSEG_ERR_INVALID_ARG; }
    LatticeBufs& lb = cs->lat[0];
    int cnt[3];
    if ((st = lattice_counters(ctx, cs, lb, ctx->stream, cnt)) != RVSEG_OK) return st;
    const int M = cnt[0], d = lb.dev.d;
    for (int j = 0; j <= d; j++) {
        if (n1_out) RV_HIP(ctx, hipMemcpy(n1_out + (size_t)j * M, lb.dev.nb1 + (size_t)j * lb.dev.m_bound, (size_t)M * 4, hipMemcpyDeviceToHost));
        if (n2_out) RV_HIP(ctx, hipMemcpy(n2_out + (size_t)j * M, lb.dev.nb2 + (size_t)j * lb.dev.m_bound, (size_t)M * 4, hipMemcpyDeviceToHost));
    }
    if (csr_point) {
        std::vector<uint2> pw((size_t)lb.n_entries);
        RV_HIP(ctx, hipMemcpy(pw.data(), lb.dev.csr_pw, (size_t)lb.n_entries * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < pw.size(); i++) csr_point[i] = pw[i].x;
    }
    if (vstart) RV_HIP(ctx, hipMemcpy(vstart, lb.dev.vstart, (size_t)M * 4, hipMemcpyDeviceToHost));
    if (vend) RV_HIP(ctx, hipMemcpy(vend, lb.dev.vend, (size_t)M * 4, hipMemcpyDeviceToHost));
    return RVSEG_OK;
}

// debug (not in rvseg.h): per-block trace of the last resident splat of the frame path's lattice, and the tile ranges
extern "C" rvseg_status rvseg_debug_resident(rvseg_ctx* ctx, void* trace_out, size_t trace_cap, unsigned* tile0_out, size_t tile0_cap, int meta[6]) {
    if (!ctx || !ctx->impl) return RVSEG_ERR_INVALID_ARG;
    Pipeline* im = ctx->impl;
    if (!im->crf || im->crf->lat.empty() || !im->crf->lat[0].resident_on) return RVSEG_ERR_INVALID_ARG;
    LatticeBufs& b = im->crf->lat[0];
    RV_HIP(ctx, hipDeviceSynchronize());
    const int nf = b.dev.n_frames;
    meta[0] = b.resident.B; meta[1] = b.resident.band_wb; meta[2] = b.resident.n_bands; meta[3] = nf; meta[4] = RES_MAXB;
    int fl[2] = {0, 0};
    RV_HIP(ctx, hipMemcpy(fl, b.resident.flags, 8, hipMemcpyDeviceToHost));
    meta[5] = fl[1];
    if (trace_out && b.resident.trace && trace_cap >= (size_t)nf * RES_MAXB * 64)
        RV_HIP(ctx, hipMemcpy(trace_out, b.resident.trace, (size_t)nf * RES_MAXB * 64, hipMemcpyDeviceToHost));
    if (tile0_out && tile0_cap >= (size_t)nf * (RES_MAXB + 1) * 4)
        RV_HIP(ctx, hipMemcpy(tile0_out, b.resident.blk_tile0, (size_t)nf * (RES_MAXB + 1) * 4, hipMemcpyDeviceToHost));
    return RVSEG_OK;
}

// debug (not in rvseg.h): how many lattices have been built on this context, overflow retries included
extern "C" rvseg_status rvseg_debug_lattice_builds(rvseg_ctx* ctx, long long* out) {
    if (!ctx || !out) return RVSEG_ERR_INVALID_ARG;
    *out = ctx->impl && ctx->impl->crf ? ctx->impl->crf->lattice_builds : 0;
    return RVSEG_OK;
}

rvseg_status rvseg_last_schedule(rvseg_ctx* ctx, rvseg_schedule_info* out) {
    if (!ctx || !out) return RVSEG_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof(*out));
    out->planner_fallback = -1;
    out->vertices = -1;
    out->longest_list = -1;
    if (!ctx->impl) return RVSEG_OK;
    Pipeline* im = ctx->impl;
    if (im->crf) *out = im->crf->info;
    return RVSEG_OK;
}

rvseg_status rvseg_lattice_filter(rvseg_ctx* ctx, const float* in, int32_t C, float* out) {
    CrfState* cs;
    rvseg_status st = crf_enter(ctx, &cs, __func__);
    if (st != RVSEG_OK) return st;
    if (cs->lat.empty() || !cs->lat[0].built || cs->lat[0].dev.n_frames != 1) { ctx->err = "no lattice built on this context"; return RVSEG_ERR_INVALID_ARG; }
    if (!in || !out || C <= 0 || C > 64) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    LatticeBufs& lb = cs->lat[0];
    const int N = lb.dev.N;
    hipStream_t s = ctx->stream;
    const size_t tot = (size_t)N * C;
    if ((st = dev_reserve(ctx, cs->q, tot * 4)) != RVSEG_OK) return st;
    if ((st = dev_reserve(ctx, cs->scratch[0].tmp, tot * 4)) != RVSEG_OK) return st;
    if ((st = values_reserve(ctx, cs, lb.dev.m_bound, C)) != RVSEG_OK) return st;
    RV_HIP(ctx, hipMemcpyAsync(cs->q.p, in, tot * 4, hipMemcpyHostToDevice, s));
    const bool seq = C <= 2;
    ValueView V{cs->q.as<float>(), tot, 0};
    auto& sc = cs->scratch[0];
    launch_splat(lb.dev, V, C, 0, sc.val_a.as<float>(), s);
    float* blurred = launch_blur(lb.dev, C, seq, false, sc.val_a.as<float>(), sc.val_b.as<float>(), s);
    launch_slice(lb.dev, C, seq, 0, blurred, 0.f, sc.tmp.as<float>(), N, s);
    RV_LAUNCH_OK(ctx);
    RV_HIP(ctx, hipMemcpyAsync(out, sc.tmp.p, tot * 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    return RVSEG_OK;
}

}  // extern "C"
