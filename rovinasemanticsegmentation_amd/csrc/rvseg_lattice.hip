// The host side of the permutohedral lattice: the capacity rules of its hash table, its buffers, the enqueue of
// Permutohedral::init (permutohedral.cpp) and of the normaliser of DenseKernel::initLattice (pairwise.cpp:40-56), the
// read-back of a build's counters, and the one retry after a hash overflow (build_lattices).  Three callers build
// lattices: the frame path (crf_frames_build*, asynchronous, its status polled by crf_frames_status), the point path
// (rvseg_crf_infer*, crf_cloud_layers) and the kept model (terms_prepare, term_rebuild) -- all in rvseg_crf.hip and
// rvseg_crf_model.hip, which see this file through rvseg_crf_state.h.  The C-ABI entries at the end build and inspect a
// lattice on its own (rvseg_lattice_*, rvseg_last_schedule, rvseg_debug_*).  The kernels are in kernels_lattice.hip,
// kernels_splat.hip and kernels_resident.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rvseg_crf_state.h"

namespace rvseg {

static int ceil_log2(unsigned long long v) {
    int b = 0;
    while ((1ull << b) < v) b++;
    return b;
}

// the vector of lattices grown to hold lattice k (one per pairwise term; the frame path and the clouds use lattice 0)
LatticeBufs& lattice_at(CrfState* cs, int k) {
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

// What the context does about a frame build (d = 6, N points per frame) whose hash table overflowed: it raises
// cap_boost for the calls that follow and reports the overflow (crf_frames_status)
rvseg_status lattice_raise_capacity(rvseg_ctx* ctx, Pipeline* im, int N) {
    const bool was_worst = capacity_is_worst_case(ctx, N, 6);
    // x8 slots per step, but stop at 2^13 on the way up: the largest capacity the counting-sort CSR path serves
    // (real scenes with a deep range have ~2 000 vertices per frame; beyond it the radix-sort path takes over)
    const int cur = configured_capacity_log2(ctx);
    im->cap_boost += cur < 13 ? std::min(3, 13 - cur) : 3;
    ctx->err = was_worst ? "lattice hash table overflowed at its worst-case capacity (internal error)"
                         : "lattice hash table overflowed: the outputs of that call are invalid; the context has raised its "
                           "capacity (x8 slots per frame), repeat the call (or set params.lattice_capacity_log2 = -1)";
    return RVSEG_ERR_CAPACITY;
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
rvseg_status lattice_prepare(rvseg_ctx* ctx, LatticeBufs& b, int d, int N, int n_frames, bool safe, int vertices_per_frame_seen,
                             bool frame_ids) {
    if (d < 1 || d > 7) { ctx->err = "feature dimension must be in [1,7]"; return RVSEG_ERR_INVALID_ARG; }
    LatticeLimits m;
    const char* err = nullptr;
    rvseg_status st = lattice_limits(d, N, n_frames, capacity_log2_per_frame(ctx, (N + 3) / 4 * 4, d, safe), m, &err);
    if (st != RVSEG_OK) { ctx->err = err; return st; }
    if ((st = lattice_reserve(ctx, b, m, d, n_frames)) != RVSEG_OK) return st;
    if ((st = lattice_fill(ctx, b, m, d, N, n_frames, frame_ids)) != RVSEG_OK) return st;
    return resident_prepare(ctx, b, vertices_per_frame_seen);
}

rvseg_status values_reserve(rvseg_ctx* ctx, CrfState* cs, long long m_bound, int C, int slot) {
    rvseg_status st;
    if ((st = dev_reserve(ctx, cs->scratch[slot].val_a, (size_t)m_bound * C * 4)) != RVSEG_OK) return st;
    if ((st = dev_reserve(ctx, cs->scratch[slot].val_b, (size_t)m_bound * C * 4)) != RVSEG_OK) return st;
    return RVSEG_OK;
}

// the context's second CRF stream (the second label layer's mean field; the splat planner beside the normaliser)
rvseg_status second_stream(rvseg_ctx* ctx, CrfState* cs) {
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
rvseg_status lattice_clear(rvseg_ctx* ctx, LatticeBufs& b, hipStream_t s) {
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
rvseg_status lattice_build(rvseg_ctx* ctx, CrfState* cs, LatticeBufs& b, const FeatureSource& fs, hipStream_t s, int norm_kind,
                           bool ends_model) {
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
rvseg_status counters_readback(rvseg_ctx* ctx, CrfState* cs, const LatticeBufs& b, int slot, hipStream_t s) {
    int* h = cs->h_counters.as<int>() + 4 * slot;
    RV_HIP(ctx, hipMemcpyAsync(h, b.dev.counters, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipMemcpyAsync(h + 2, b.dev.counters + 3, sizeof(int), hipMemcpyDeviceToHost, s));
    if (b.resident_on) RV_HIP(ctx, hipMemcpyAsync(h + 3, b.resident.flags, sizeof(int), hipMemcpyDeviceToHost, s));
    else h[3] = 0;   // (host write; no copy of this build touches the word)
    return RVSEG_OK;
}

// what a read-back slot tells rvseg_last_schedule about the build cs->info describes
void counters_to_info(CrfState* cs, const int* h) {
    cs->info.vertices = h[0];
    cs->info.longest_list = h[2];
    cs->info.planner_fallback = h[3];
    cs->info_async = false;
}

// synchronous read of the build counters (host entry points): out = M, overflow
static rvseg_status lattice_counters(rvseg_ctx* ctx, CrfState* cs, const LatticeBufs& b, hipStream_t s, int out[2]) {
    rvseg_status st = counters_readback(ctx, cs, b, 1, s);
    if (st != RVSEG_OK) return st;
    RV_HIP(ctx, hipStreamSynchronize(s));
    const int* h = cs->h_counters.as<int>() + 4;
    out[0] = h[0]; out[1] = h[1];
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

// Permutohedral::init + normaliser of term `t` on lattice `lb` (host features are copied into cs->feat, kernel
// parameters applied into cs->kfeat), then the counters, read back with one stream synchronisation
static rvseg_status build_lattice(rvseg_ctx* ctx, CrfState* cs, LatticeBufs& lb, int N, const TermInput& t, bool safe, hipStream_t s, int cnt[2]) {
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

// The lattices of n terms over N points, term k on cs->lat[first + k], with THE overflow retry of every synchronous
// caller (the point entries, a kept model's terms, term_rebuild's one term, rvseg_lattice_build): a hash overflow of any
// term stops the attempt, and ALL n terms are rebuilt once at the safe capacity, which cannot overflow.
// vertices (optional): the vertex count M of the last lattice.
rvseg_status build_lattices(rvseg_ctx* ctx, CrfState* cs, int N, int n, const TermInput* terms, hipStream_t s, int first, int* vertices) {
    if (n > 0) lattice_at(cs, first + n - 1);
    int c[2] = {0, 0};   // M, overflow
    for (int attempt = 0; attempt < 2; attempt++) {
        c[1] = 0;
        for (int k = 0; k < n && !c[1]; k++) {
            rvseg_status st = build_lattice(ctx, cs, cs->lat[first + k], N, terms[k], attempt == 1, s, c);
            if (st != RVSEG_OK) return st;
        }
        if (vertices) *vertices = c[0];
        if (!c[1]) return RVSEG_OK;
    }
    ctx->err = "lattice hash table overflow";
    return RVSEG_ERR_CAPACITY;
}

}  // namespace rvseg

using namespace rvseg;

extern "C" {

rvseg_status rvseg_lattice_build(rvseg_ctx* ctx, const float* features, int32_t N, int32_t d, int32_t* offsets_out,
                                 float* bary_out, int16_t* keys_out, int32_t keys_capacity, int32_t* M_out) {
    CrfState* cs;
    rvseg_status st = crf_enter(ctx, &cs, __func__);
    if (st != RVSEG_OK) return st;
    if (!features || N <= 0 || !M_out) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    hipStream_t s = ctx->stream;
    int M = 0;
    const TermInput in = potts_input(d, features, true);
    if ((st = build_lattices(ctx, cs, N, 1, &in, s, 0, &M)) != RVSEG_OK) return st;
    const LatticeBufs& lb = cs->lat[0];
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
    int cnt[2];
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
