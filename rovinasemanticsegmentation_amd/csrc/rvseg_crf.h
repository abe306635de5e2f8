// Device-side views and launch interface of the lattice / splat / mean-field kernels
// (kernels_lattice.hip, kernels_splat.hip, kernels_resident.hip, kernels_meanfield.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "rvseg_internal.h"

namespace rvseg {

// Everything a lattice kernel needs, passed by value.
struct LatticeDev {
    int d;          // feature dimension (<= 7)
    int N;          // points per frame
    int Npad;       // N rounded up to a multiple of 4 (SSE block padding, permutohedral.cpp:196)
    int n_frames;
    unsigned cap_f_mask;   // per-frame hash capacity - 1 (power of two)
    unsigned cap_f_log2;
    unsigned cap_total;    // n_frames * per-frame capacity
    int m_bound;        // capacity of the per-vertex arrays
    float scale[8];     // diagonal of E, permutohedral.cpp:177-182
    int* state;                  // per slot: EMPTY / LOCKED / FILLED
    unsigned long long* tkeys;   // per slot: 8 x int16 key (d coordinates .. frame)
    int* slot_to_id;
    int* counters;               // [0] vertices M, [1] overflow flag, [2] (unused), [3] entries of the longest vertex list
    int* fstart;                 // n_frames + 1: first vertex id of each frame (ids are frame-contiguous)
    unsigned long long* vkeys;   // per vertex id: key
    int* offsets;                // P x (d+1): slot, later vertex id.  ids16: the same rows as uint16_t, frame-local
    int ids16;                   // 1: `offsets` holds 16-bit frame-local values -- slot - frame * cap_f, later vertex id -
                                 // fstart[frame] -- in rows of d+1 without padding (frame path on the counting-sort
                                 // path, d = 6: both are below 2^13); 0: 32-bit global values
    float* bary;                 // P x (d+1)
    int *nb1, *nb2;              // (d+1) x m_bound blur neighbours (-1 = none)
    uint2* csr_pw;               // entries sorted by vertex, ascending point index inside a vertex:
                                 // {point index, barycentric weight bits}
    float* csr_nrm;              // norm[point] per entry (multi-kernel path only, built on demand)
    unsigned *vstart, *vend;     // per vertex [start, end) into the csr arrays
    unsigned* vorder;            // vorder[fstart[f] + k] = k-th longest vertex of frame f (splat launch order)
    int n_groups;                // 8 when the chunk has >= 8 frames, else 1
    int group_vertices;          // list-major walk, C = 8 / 9: vertices per block (0 = by the chunk's shape, 6, 7)
    int ordered_sum_scan;        // normaliser: exact wave-scan sums (1) or the serial chain (0); same bits either way
    int cs_pix;                  // counting sort: points per wave-block (256 for launches of <= 8 frames, else 1024)
    unsigned heavy_from;         // list-major walk: lists of this many entries and more belong to scan blocks (0 = none) ...
    unsigned scan_ranks;         // ... if they are among the scan_ranks longest of their frame
    // counting-sort path: after the scan, bh[wave-block][vertex] is the position of the vertex's first entry at or
    // after that wave-block, i.e. the vertex-major lists can be cut at any multiple of CS_PIX points without
    // another sort (the resident band schedule does)
    const unsigned* bh;          // per frame a dense [wbpf][M_f] matrix starting at wbpf * fstart[frame]; null on the radix path
    int wbpf;                    // wave-blocks per frame
    float* norm;                 // per point, pairwise.cpp:55-56
};

// The one statement of which dimensions are instantiated: calls f with d as a compile-time constant.  The API entry
// points take no other d (RVSEG_ERR_INVALID_ARG), so a LatticeDev never carries one: for a d outside 1 .. 7 every launcher
// that goes through here launches nothing.
template <class F>
void with_dimension(int d, F&& f) {
    switch (d) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 5: f(std::integral_constant<int, 5>()); break;
        case 6: f(std::integral_constant<int, 6>()); break;
        case 7: f(std::integral_constant<int, 7>()); break;
        default: break;   // rejected at the API
    }
}

// the constant every slice multiplies by (permutohedral.cpp:512 / :571; the slicing gradient, :628, divides it by d + 1)
inline float lattice_alpha(int d) { return 1.0f / (1 + powf(2, (float)-d)); }

// Vertex ids [x, y) of a frame, each clamped to `bound`: the per-vertex arrays' capacity or the vertices that exist.  (The
// clamp only binds after a flagged hash overflow; it keeps every access in bounds.)
__device__ __forceinline__ int2 lattice_frame_range(const LatticeDev& L, int frame, int bound) {
    const int f0 = L.fstart[frame], f1 = L.fstart[frame + 1];
    return make_int2(f0 < bound ? f0 : bound, f1 < bound ? f1 : bound);
}

// The kernels that are not specialised on the id form read `offsets` through this (L.ids16 is uniform).
typedef unsigned short lattice_id16 __attribute__((may_alias));
// global vertex id of vertex j of point p (after the count pass); stored as such, or with ids16 local to the frame
__device__ __forceinline__ int lattice_vertex(const LatticeDev& L, long long p, int dp1, int j) {
    const long long e = p * dp1 + j;
    return L.ids16 ? (int)reinterpret_cast<const lattice_id16*>(L.offsets)[e] + L.fstart[p / L.N] : L.offsets[e];
}

// Band-interleaved resident schedule of the ordered splat ("resident bands").  A frame's
// vertices are dealt to B blocks that all stay on the chip for the whole launch; a block walks ITS vertices band after
// band of `band_wb` wave-blocks of points, so the d+1 readers of a point's row pass within a few bands of each other
// and meet in the XCD's L2, while every chain stays inside one block (sums never travel between blocks: no hand-off,
// no dependency -- the pacing is a hint, not a condition of correctness).  The walk is a list of tiles built once per
// lattice.  A tile is one step of the block: seven slots, each up to 64 (or 128) consecutive entries of one vertex.  Inside a
// band the chunks of the block's vertices are packed into the fewest tiles that keep a vertex's chunks in
// different tiles, in order (wrap-around rule: tiles = max(longest vertex, chunks / 7)); which vertex a slot serves
// changes from tile to tile, so the running sums live in LDS and a slot swaps its sum when its vertex changes.
constexpr int RES_MAXB = 16;          // blocks per frame at most
constexpr int RES_MAX_OWNV = 640;     // vertices a block can own (their running sums live in LDS): a 2 048-vertex frame on 4 blocks
constexpr int RES_MAX_VERTS = 4096;   // vertices of a frame the planner handles (= the counting-sort path's limit, CS_MCAP)
constexpr int RES_MAX_BANDS = 512;
struct SplatResidentDev {
    unsigned* tdesc;             // [n_frames][7][cap_tiles]: (first entry - frame's first entry) << 8 | entries (0..128)
    unsigned short* tvl;         // [n_frames][7][cap_tiles]: block-local vertex of the slot (n_own = nobody: entries is 0)
    unsigned* tinfo;             // [n_frames][cap_tiles]: band << 16 | most entries of a slot
    unsigned* blk_tile0;         // [n_frames][RES_MAXB + 1]: block j walks tiles [blk_tile0[j], blk_tile0[j + 1]) of its frame
    unsigned short* blk_verts;   // [n_frames][RES_MAXB][RES_MAX_OWNV]: frame-local vertex of each block-local one
    unsigned* blk_nown;          // [n_frames][RES_MAXB]
    unsigned* jb_tile;           // [n_frames][RES_MAXB][n_bands + 1]: first tile of (block, band), relative to the frame
    unsigned* prog;              // [2 scratch slots][n_frames][RES_MAXB]: launch tag << 16 | band reached
    int* flags;                  // [0] frames the planner could not handle, [1] = 1: schedule valid
    unsigned long long* trace;   // optional (rvseg_schedule.trace): per (frame, block) 8 words: start, end, tiles, ticks spent waiting for the pace (10 ns ticks), shader clocks
    int B, band_wb, n_bands, window;
    int chunk_log2;              // entries per slot and tile: 2^6 or 2^7
    unsigned cap_tiles;
};

// Where the lattice features come from.
struct FeatureSource {
    int mode;            // 0: feat array P x d; 1: frame mode (cloud + colours, d = 6)
    const float* feat;
    const float4* cloud;
    const uint8_t* rgb;
    float xyz_kernel, rgb_kernel;
};

// N x C values addressed either densely or inside the per-frame posterior layout
// (frame stride sumC*N floats, layer offset N*prefixC).
struct ValueView {
    float* base;
    size_t frame_stride;
    size_t layer_off;
    __host__ __device__ __forceinline__ size_t index(unsigned p, int c, int C, int N) const {
        const unsigned frame = p / (unsigned)N;
        const unsigned i = p - frame * (unsigned)N;
        return (size_t)frame * frame_stride + layer_off + (size_t)i * C + c;
    }
    __device__ __forceinline__ float at(unsigned p, int c, int C, int N) const { return base[index(p, c, C, N)]; }
    __device__ __forceinline__ float& ref(unsigned p, int c, int C, int N) const { return base[index(p, c, C, N)]; }
};

struct SortBuffers {
    unsigned *keys_in, *keys_out, *vals_in, *vals_out;
    void* temp;
    size_t temp_bytes;
    int key_bits;
    void* scan_temp;
    size_t scan_temp_bytes;
    unsigned* block_hist;   // counting-sort fast path: n_frames x wave-blocks x (cap_f/2), or null
};

void launch_fill_int(int* p, int v, long long n, hipStream_t s);
void launch_lattice_points(const LatticeDev& L, const FeatureSource& fs, hipStream_t s);
// defer_scatter: leaves the counting-sort path's scatter to a later launch_csr_scatter (which the radix-sort path ignores)
void launch_lattice_finish(const LatticeDev& L, SortBuffers& sb, long long n_entries, hipStream_t s, bool defer_scatter);
void launch_csr_scatter(const LatticeDev& L, SortBuffers& sb, hipStream_t s);
size_t sort_temp_bytes(long long n_entries, int key_bits);
size_t scan_temp_bytes(unsigned cap);
bool csr_fast_path(const LatticeDev& L);
size_t csr_fast_bytes(const LatticeDev& L);
int csr_pix_min();
void launch_csr_norm(const LatticeDev& L, long long n_entries, hipStream_t s);
// mode 0: in = src; 1: in = fl(src * norm); 2: in = 1
// own_q: src is the mean-field loop's own Q * norm (finite, non-negative): enables the select-free producer
void launch_splat(const LatticeDev& L, const ValueView& src, int C, int mode, float* values, hipStream_t s, bool own_q = false,
                  const SplatResidentDev* resident = nullptr, int slot = 0);
// blocks ("items") of the list-major walk with `per_item` vertices each
unsigned splat_walk_items(const LatticeDev& L, int per_item);
// builds the resident band schedule from the counting-sort table (after launch_lattice_finish)
void launch_resident_plan(const LatticeDev& L, const SplatResidentDev& r, hipStream_t s);
// how many blocks of the resident splat kernel fit on the device at once (0: unknown)
int resident_block_capacity(int chunk);
int resident_cu_count();
// the splat of C = 8 / 9 classes over the resident schedule; false: the kernel could not be set up or launched, the
// caller walks the lists the list-major way
bool launch_splat_resident(const LatticeDev& L, const SplatResidentDev& R, int C, const float* src, float* values, int slot,
                           hipStream_t s);
float* launch_blur(const LatticeDev& L, int C, bool seq, bool reverse, float* a, float* b, hipStream_t s, bool small_blocks = false);
// out_mode 0: plain, 1: normaliser, 2: inference update (tmp -= (-w) * (sliced * norm)),
// 3: normaliser 1/(sliced + 1e-20) (NORMALIZE_BEFORE / NORMALIZE_AFTER)
void launch_slice(const LatticeDev& L, int C, bool seq, int out_mode, const float* values, float neg_w, float* out,
                  long long n_points, hipStream_t s);
// labels of the final marginals straight from the last update (the values are in registers there):
// labels[(frame * n_layers + layer) * N + point]; labels == nullptr: none
struct MfLabels {
    int8_t* labels;
    int mode, unknown, n_layers, layer;
};
// The compatibility of the one term of a fused update.  compat == nullptr: Potts / uniform Diagonal with
// NORMALIZE_SYMMETRIC, out = fl(neg_w * (sliced * norm)) (the Segmenter's term).  Else a Diagonal (C floats) or symmetric
// Matrix (C x C) read from `compat`, the sliced values scaled by norm first when `post`.
struct MfTerm {
    float neg_w;
    const float* compat;
    bool matrix, post;
};
bool mf_fused_supported(int C);
// fused slice + compatibility + unary + softmax for a single pairwise term; false if C is not instantiated
bool launch_mf_update(const LatticeDev& L, int C, const float* values, const MfTerm& term, const ValueView& unary, bool negate,
                      const ValueView& Q, bool scale_out, const MfLabels& lab, hipStream_t s);
void launch_neg_unary(const ValueView& unary, bool negate, int C, int N, float* tmp, long long n_points, hipStream_t s);
bool launch_softmax_unary(const ValueView& unary, bool negate, int C, int N, const ValueView& q, long long n_points,
                          const float* scale, hipStream_t s);
void launch_softmax(const float* tmp, int C, int N, const ValueView& q, long long n_points, hipStream_t s);
// one general pairwise term: slice, optional post-scale by L.norm, Diagonal (compat: C floats) or symmetric Matrix (C x C)
// compatibility, tmp -= result (assign: tmp = result, the term's apply on its own)
void launch_term_update(const LatticeDev& L, int C, bool seq, const float* values, bool post, bool matrix, const float* compat,
                        float* tmp, long long n_points, hipStream_t s, bool assign = false);
// kernel parameters of a term: kind 1 DIAG (d values), 2 FULL (d x d column-major)
struct KernelParams { float p[49]; };
void launch_kernel_params(const float* f, int N, int d, int kind, const KernelParams& kp, float* out, hipStream_t s);
// U (N x C) = f (N x K) times L^T (L: C x K row-major, device)
void launch_logistic_unary(const float* Lm, const float* f, int N, int C, int K, float* U, hipStream_t s);


// ---- kernels_crf_model.hip: energies and KL divergence of a kept model -----------------------------------------------
// rows[i][c] = 1.0f where c == labels[i], else 0 (a label outside [0, C) gives a zero row: densecrf.cpp:165-169)
void launch_onehot(const int8_t* labels, long long n, int C, float* rows, hipStream_t s);
// v = fl(scale * rows[i][labels[i]]), 0 for a label outside [0, C); out[i] = v, or fl(out[i] + v) when accumulate
void launch_label_gather(const float* rows, const int8_t* labels, long long n, int C, float scale, bool accumulate, float* out, hipStream_t s);
// The KL passes share one thread layout (256 / C points per block step) and one grid: kl_blocks(C, n) blocks, each of
// which leaves ONE double per part in partials[part * KL_MAX_BLOCKS + block].
constexpr int KL_MAX_BLOCKS = 512;
constexpr int KL_FINAL_THREADS = 256;
int kl_blocks(int C, long long n_points);
// parts 0 (entropy, q log max(q, 1e-20f)) and 1 (unary, U q; U = unary_is_energy ? unary : -unary)
void launch_kl_unary(const float* unary, bool unary_is_energy, const float* Q, int C, long long n_points, double* partials, hipStream_t s);
// one pairwise part: sum q * a with a the fp32 value of the term's apply, sliced from the term's blurred `values`
void launch_kl_term(const LatticeDev& L, int C, bool seq, const float* values, bool post, bool matrix, const float* compat,
                    const float* Q, long long n_points, double* partial, hipStream_t s);
// adds each part's partials, index ascending; parts_out (n_parts) / sum_out (1, the parts added in order) may be null
void launch_kl_final(const double* partials, int n_blocks, int n_parts, double* parts_out, double* sum_out, hipStream_t s);


// ---- kernels_crf_learn.hip: objectives, backward pass and parameter gradients of a kept model ------------------------------
// doubles of scratch the learning reductions of C classes need at most (partials of one launch)
size_t learn_partials_doubles(int C);
// rvseg_crf_objective on device pointers: d_mul_Q (N x C, zero where nothing is written) and *value; stats: 128 doubles (IoU)
void launch_objective(int kind, const int16_t* gt, float robust, const float* class_weight, const float* Q, int C, long long n_points,
                      float* d_mul_Q, double* partials, double* stats, double* value, hipStream_t s);
// b = sumAndNormalize(mul ? fl(in * q) : in, q); ug (may be null): ug_mode 1 ug = b, 2 ug += b
void launch_sum_normalize(const float* in, bool mul, const float* q, int C, long long n_points, float* b, float* ug, int ug_mode, hipStream_t s);
// acc = (first ? 0.0f : acc) + t
void launch_add_rows(bool first, const float* t, float* acc, long long total, hipStream_t s);
// out (the term's slots of compat_grad) += the gradient of one term from b and the blurred `values` of its kernel apply
void launch_compat_grad(const LatticeDev& L, int C, bool seq, const float* values, bool post, int compat, const float* b, long long n_points,
                        double* partials, double* out, hipStream_t s);
// out[k * C + m] = sum_i g[i][m] f[i][k]; partials: learn_partials_doubles(64)
void launch_logistic_gradient(const float* g, const float* f, long long n_points, int C, int K, double* partials, double* out, hipStream_t s);


// ---- kernels_crf_kgrad.hip: the kernel-parameter gradient of a kept model ------------------------------------------------
// ranks[i]: the d+1 ranks of point i of the lattice's one frame (0 .. d, 3 bits each, rank[0] lowest), from the features
// the lattice was built from
void launch_point_ranks(const LatticeDev& L, const float* feat, unsigned* ranks, hipStream_t s);
// one direction of Permutohedral::gradient's slicing gradient: values = the blurred table (M x C), x = the weighting
// matrix (N x C); df (N x d) assigned (dir 0) or added to (dir 1).  Grid: kl_blocks(C, n_points)
void launch_slice_gradient(const LatticeDev& L, int C, const float* values, const float* x, const unsigned* ranks, int dir, long long n_points,
                           float* df, hipStream_t s);
// out = compatibility(Q) without a filter; compat: the term's C (Diagonal / Potts) or C x C (Matrix) floats
void launch_compat_rows(int C, bool matrix, const float* compat, const float* Q, long long n_points, float* out, hipStream_t s);
// element-wise steps of featureGradient over `total` elements in rows of C (n: per row): mode 0 a n; 1 the SYMMETRIC X;
// 2 fl(a b) fl(n n); 3 a - b; 4 ones
void launch_kgrad_mix(int mode, const float* a, const float* b, const float* fa, const float* fb, const float* n, int C, long long total,
                      float* out, hipStream_t s);
// out += the d x d column-major `full` (FULL) or its diagonal (DIAG)
void launch_kgrad_accumulate(bool diag, int d, const double* full, double* out, hipStream_t s);

}  // namespace rvseg
