// Ordered splat of the DenseCRF filter for gfx950: list-major walk, the normaliser's exact ordered sums, scan blocks
// and launch_splat, which picks between them and the resident band schedule (kernels_resident.hip).
//
// Reference semantics (third-party/densecrf/src):
//   sseCompute / seqCompute           permutohedral.cpp:476-589   (the splat part)
//   DenseKernel::initLattice/filter   pairwise.cpp:40-80          (symmetric normalisation)
//
// MI355X design notes
//   * The reference splats sequentially over points, so a vertex's fp32 sum is ordered by point
//     index.  To stay bit-exact the splat is a GATHER: entries are stably sorted by vertex and each
//     (vertex, class) chain adds its contributions in ascending point order.  No float atomics.
#include <algorithm>

#include "splat_device.h"

namespace rvseg {

template <int MODE, int CC, bool FULL, int GV = SplatGroup<CC>::G, bool FAST = false, int NH = 1>   // FULL: all CC classes exist (n_store == CC): rows are fetched with wide loads
__global__ void __launch_bounds__((GV + 1) * 64)
splat_group_kernel(LatticeDev L, ValueView src, int C, int c0, int n_store, float* __restrict__ values) {
    __shared__ __attribute__((aligned(16))) float prod[2][GV][CC][64 * NH + 4];  // 16-B aligned rows, 4-bank skew
    if (L.counters[1]) return;   // hash overflow (flagged): the CSR arrays are incomplete, touch nothing
    splat_group_item<MODE, CC, FULL, GV, FAST, NH>(L, src, C, c0, n_store, values, blockIdx.x, prod);
}

// the list-major walk's grid, per XCD group: (frames of the group) x (blocks of `per_item` vertices a frame can have at most)
static unsigned walk_frames_per_group(const LatticeDev& L) { return ((unsigned)L.n_frames + (unsigned)L.n_groups - 1u) / (unsigned)L.n_groups; }
static unsigned long long walk_max_vertices(const LatticeDev& L) {
    return std::min<unsigned long long>(((unsigned long long)L.cap_f_mask + 1) / 2 + 1, (unsigned long long)L.m_bound);
}
unsigned splat_walk_items(const LatticeDev& L, int per_item) {
    return walk_frames_per_group(L) * (unsigned)((walk_max_vertices(L) + per_item - 1) / per_item) * (unsigned)L.n_groups;
}

template <int MODE, int CC, int GV, bool FAST, int NH = 1>
static void splat_group_launch_g(const LatticeDev& L, const ValueView& src, int C, int c0, int n, float* values, hipStream_t s) {
    const dim3 grid(splat_walk_items(L, GV)), block((GV + 1) * 64);
    if (n == CC) splat_group_kernel<MODE, CC, true, GV, FAST, NH><<<grid, block, 0, s>>>(L, src, C, c0, n, values);
    else splat_group_kernel<MODE, CC, false, GV, false><<<grid, block, 0, s>>>(L, src, C, c0, n, values);
    RV_LAUNCHED("splat_group_kernel");
}

template <int MODE, int CC>
static void splat_group_launch(const LatticeDev& L, const ValueView& src, int C, int c0, int n, float* values, hipStream_t s) {
    splat_group_launch_g<MODE, CC, SplatGroup<CC>::G, false>(L, src, C, c0, n, values, s);
}

template <int MODE>
static void splat_group_pass(const LatticeDev& L, const ValueView& src, int C, int c0, int n, float* values, hipStream_t s) {
    if (n == 1) splat_group_launch<MODE, 1>(L, src, C, c0, n, values, s);
    else if (n == 2) splat_group_launch<MODE, 2>(L, src, C, c0, n, values, s);
    else if (n <= 4) splat_group_launch<MODE, 4>(L, src, C, c0, n, values, s);
    else if (n <= 8) splat_group_launch<MODE, 8>(L, src, C, c0, n, values, s);
    else if (n == 9) splat_group_launch<MODE, 9>(L, src, C, c0, n, values, s);
    else splat_group_launch<MODE, 16>(L, src, C, c0, n, values, s);
}


// ---------------------------------------------------------------------------------------------
// The normaliser's splat (C = 1: a vertex's value is the fp32 sum of its entries' barycentric weights, added in list
// order from +0) without the serial chain.  The ordered sum only LOOKS sequential: while the running sum s stays in one
// binade [2^E, 2^(E+1)) every partial sum is a multiple of u = 2^(E-23), and adding w >= 0 to it rounds s + w to the
// nearest multiple of u -- in units of u: n + k  ->  n + rne(k), k = w / u, unless k lies exactly half-way between two
// integers (then the direction depends on the parity of n).  So, as long as no addend of a tile is negative or such a
// tie and the tile does not leave the binade,
//       s_after = (n + sum_i rne(k_i)) * u ,
// a sum of integers below 2^24 -- exact in fp32 in ANY order.  A wave adds a tile of 128 or 256 addends (two or four
// per lane) with a few additions per lane and six DPP steps instead of that many dependent additions; a tile that breaks
// a condition (the first one, ~17 binade crossings and a few dozen ties per long list: 4-5 % of the 64-entry tiles of a
// bench frame's heaviest lists) is tried again in two halves, and a half that breaks one is added the reference's way,
// one addend after the other.  The result is bit-identical to the sequential sum by construction and is tested
// against it (tests/test_gpu_crf.py: test_normaliser_ordered_sums_...).
// The same idea does not pay for the C-class splats: there the serial adder already runs 54 chains in its 64 lanes.
// ---------------------------------------------------------------------------------------------
// One attempt at the lanes `mine` (K addends per lane, lane l holding entries K l .. K l + K - 1 of the tile): true and
// s advanced if the conditions above hold for them, false and s untouched otherwise.
template <int K>
__device__ __forceinline__ bool ordered_try(float& s, const float (&w)[K], bool mine) {
    const unsigned sb = __float_as_uint(s);
    const unsigned e = (sb >> 23) & 0xffu;                              // biased exponent of the running sum
    const bool s_ok = ((int)sb > 0) & (e >= 24u) & (e <= 253u);        // positive, normal, scale factors representable
    const float scale = __uint_as_float((277u - (s_ok ? e : 127u)) << 23);      // 2^(23 - E) = 1 / u
    const float unscale = __uint_as_float(((s_ok ? e : 127u) - 23u) << 23);     // u
    float rs = 0.0f;
    bool bad = false;
#pragma unroll
    for (int h = 0; h < K; h++) {
        const float k = w[h] * scale;                 // exact (a power of two)
        const float r = __builtin_rintf(k);           // round half to even, like the addition itself
        bad |= !(w[h] >= 0.0f) | !(k < 16777216.0f) | (__builtin_fabsf(k - r) == 0.5f);
        rs += r;
    }
    rs = mine ? rs : 0.0f;
    bad &= mine;
    // (sums of integers: exact while below 2^24, and not below 2^24 once the true sum is not -- rounding is monotone)
    const float total = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_total_lane63(rs)), 63));
    const float S = s * scale + total;
    const bool ok = s_ok & (__builtin_amdgcn_ballot_w64(bad) == 0ull) & (S < 16777216.0f);
    if (ok) s = S * unscale;
    return ok;
}
// the reference's way for lanes [LO, HI): one addition per addend, in list order
template <int K, int LO, int HI>
__device__ __forceinline__ float ordered_serial(float s, const float (&w)[K]) {
#pragma unroll
    for (int i = LO; i < HI; i++)
#pragma unroll
        for (int h = 0; h < K; h++) s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w[h]), i));
    return s;
}
// s + (a tile of 64 K addends), rounded after every addition like the sequential loop: the whole tile at once if it can
// be, else its two halves, each at once or serially
template <int K>
__device__ __forceinline__ float ordered_tile_sum(float s, const float (&w)[K]) {
    if (ordered_try<K>(s, w, true)) return s;
    const bool low = (threadIdx.x & 63) < 32;
    if (!ordered_try<K>(s, w, low)) s = ordered_serial<K, 0, 32>(s, w);
    if (!ordered_try<K>(s, w, !low)) s = ordered_serial<K, 32, 64>(s, w);
    return s;
}

// Two kernels share the vertices of a frame (`vorder`: longest list first).
//  * Lists of NS_HEAVY entries and more -- the chains that set the time of a launch with few frames: one block per
//    vertex; wave 0 sums, waves 1..3 bring the list's weights into LDS three batches ahead of it (a single wave cannot
//    keep enough loads in flight for itself: it sums 128 entries in ~0.1 us, a load takes 1-3 us to come back, and a
//    register ring deep enough for that defeated the compiler's wait counting -- every variant ended in s_waitcnt
//    vmcnt(0) or (1) per tile and ran at the speed of the serial chain).  One barrier per batch of 2 048 entries.
//  * The short lists, thousands of them: one wave per vertex straight from global memory; their loads' latency is
//    hidden by the other waves.
constexpr int NS_HEAVY = 8192;                 // entries from which a list gets a block of its own
constexpr int NS_BATCH = 2048;                 // entries per batch
constexpr int NS_RING = 4;                     // batches of floats in LDS (32 KB): one being summed, three on their way
constexpr int NS_K = 4;                        // entries per lane and tile on the heavy path: tiles of 256
constexpr int NS_SEGS = NS_BATCH / (64 * NS_K);   // tiles of a batch: one ordered_tile_sum each
constexpr int NS_PROD = 3;                     // producer waves
constexpr int NS_PER = (NS_SEGS + NS_PROD - 1) / NS_PROD;

struct NormItem { unsigned frame, r; int fs0; unsigned n_vert; bool ok; };
// item -> (rank r, frame) as in splat_group_item: every frame's heaviest vertices are dispatched first
__device__ __forceinline__ NormItem norm_item(const LatticeDev& L, unsigned item) {
    NormItem it{0u, 0u, 0, 0u, false};
    const unsigned g = item % (unsigned)L.n_groups, j = item / (unsigned)L.n_groups;
    const unsigned nfg = ((unsigned)L.n_frames - g + (unsigned)L.n_groups - 1u) / (unsigned)L.n_groups;
    if (nfg == 0) return it;
    it.r = j / nfg;
    it.frame = g + (j - it.r * nfg) * (unsigned)L.n_groups;
    const int Mtot = L.counters[0] < L.m_bound ? L.counters[0] : L.m_bound;
    const int2 fr = lattice_frame_range(L, (int)it.frame, Mtot);
    it.fs0 = fr.x;
    it.n_vert = (unsigned)(fr.y - fr.x);
    it.ok = true;
    return it;
}

__device__ __forceinline__ void norm_sum_heavy(const LatticeDev& L, float* __restrict__ values, unsigned item, float (*buf)[NS_BATCH]) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const NormItem it = norm_item(L, item);
    if (!it.ok || it.r >= it.n_vert) return;
    const unsigned v = L.vorder[(unsigned)it.fs0 + it.r];
    const unsigned k0 = L.vstart[v], k1 = L.vend[v];
    const unsigned len = k1 - k0;
    if (len < (unsigned)NS_HEAVY) return;   // (whole block) a light block's
    const unsigned n_batch = (len + NS_BATCH - 1u) / NS_BATCH;
    const float* wgt = reinterpret_cast<const float*>(L.csr_pw) + 1;   // the weight of entry k is wgt[2 k]
    // producer wave: its share of batch q -- issue (loads, all in flight together) and, an iteration or two later, commit
    auto issue = [&](unsigned q, float (&x)[NS_PER][NS_K]) {
        const unsigned base = k0 + q * NS_BATCH + (unsigned)(NS_K * lane);
#pragma unroll
        for (int i = 0; i < NS_PER; i++) {
            const unsigned e = base + (unsigned)(64 * NS_K) * (unsigned)((wave - 1) + NS_PROD * i);
#pragma unroll
            for (int h = 0; h < NS_K; h++) x[i][h] = wgt[2 * (size_t)__builtin_elementwise_min(e + h, k1 - 1u)];
        }
    };
    auto commit = [&](unsigned q, const float (&x)[NS_PER][NS_K]) {
        const unsigned base = k0 + q * NS_BATCH + (unsigned)(NS_K * lane);
#pragma unroll
        for (int i = 0; i < NS_PER; i++) {
            const int seg = (wave - 1) + NS_PROD * i;
            const unsigned e = base + (unsigned)(64 * NS_K) * (unsigned)seg;
            if (seg < NS_SEGS)   // +0 past the end of the list: the identity of the sum
                *reinterpret_cast<float4*>(&buf[q % NS_RING][seg * 64 * NS_K + NS_K * lane]) =
                    make_float4(e < k1 ? x[i][0] : 0.0f, e + 1u < k1 ? x[i][1] : 0.0f, e + 2u < k1 ? x[i][2] : 0.0f, e + 3u < k1 ? x[i][3] : 0.0f);
        }
    };
    // batches q + 1 and q + 2 travel in registers (xa: odd, xb: even batch numbers) while batch q is summed
    static_assert(NS_K == 4, "the LDS tiles are float4 per lane");
    float xa[NS_PER][NS_K], xb[NS_PER][NS_K];
    float s = 0.0f;
    if (wave > 0) {
        issue(0, xb); commit(0, xb);
        issue(1, xa); issue(2, xb);
    }
    __syncthreads();
    for (unsigned q = 0; q < n_batch; q += 2) {
        // even iteration: batch q is summed, q + 1 (xa) is committed, q + 3 issued into xa
        if (wave > 0) { commit(q + 1u, xa); issue(q + 3u, xa); }
        else {
            const unsigned here = len - q * NS_BATCH < (unsigned)NS_BATCH ? len - q * NS_BATCH : (unsigned)NS_BATCH;
            const float4* pb = reinterpret_cast<const float4*>(buf[q % NS_RING]) + lane;
            const unsigned n_seg = (here + (unsigned)(64 * NS_K - 1)) / (unsigned)(64 * NS_K);
            float4 w = pb[0];
            for (unsigned sg = 0; sg < n_seg; sg++) {   // the next tile's LDS read travels during this tile's sum
                const float4 wn = pb[64u * (sg + 1u < (unsigned)NS_SEGS ? sg + 1u : sg)];
                const float wk[NS_K] = {w.x, w.y, w.z, w.w};
                s = ordered_tile_sum<NS_K>(s, wk);
                w = wn;
            }
        }
        __syncthreads();
        if (q + 1u >= n_batch) break;
        // odd iteration: batch q + 1 is summed, q + 2 (xb) is committed, q + 4 issued into xb
        if (wave > 0) { commit(q + 2u, xb); issue(q + 4u, xb); }
        else {
            const unsigned q1 = q + 1u;
            const unsigned here = len - q1 * NS_BATCH < (unsigned)NS_BATCH ? len - q1 * NS_BATCH : (unsigned)NS_BATCH;
            const float4* pb = reinterpret_cast<const float4*>(buf[q1 % NS_RING]) + lane;
            const unsigned n_seg = (here + (unsigned)(64 * NS_K - 1)) / (unsigned)(64 * NS_K);
            float4 w = pb[0];
            for (unsigned sg = 0; sg < n_seg; sg++) {   // the next tile's LDS read travels during this tile's sum
                const float4 wn = pb[64u * (sg + 1u < (unsigned)NS_SEGS ? sg + 1u : sg)];
                const float wk[NS_K] = {w.x, w.y, w.z, w.w};
                s = ordered_tile_sum<NS_K>(s, wk);
                w = wn;
            }
        }
        __syncthreads();
    }
    if (wave == 0 && lane == 0) values[v] = s;
}

constexpr int NS_WAVES = NS_PROD + 1;   // vertices (waves) per light block

__device__ __forceinline__ void norm_sum_light(const LatticeDev& L, float* __restrict__ values, unsigned item, bool heavy_elsewhere) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const NormItem it = norm_item(L, item);
    if (!it.ok) return;
    const unsigned idx = it.r * NS_WAVES + (unsigned)wave;
    if (idx >= it.n_vert) return;   // whole wave; no block-wide barrier on this path
    const unsigned v = L.vorder[(unsigned)it.fs0 + idx];
    const unsigned k0 = L.vstart[v], k1 = L.vend[v];
    if (heavy_elsewhere && k1 - k0 >= (unsigned)NS_HEAVY) return;   // a heavy block's
    float s = 0.0f;
    const float* wgt = reinterpret_cast<const float*>(L.csr_pw) + 1;
    for (unsigned kb = k0; kb < k1; kb += 512u) {   // four tiles of 128 per step
        float x[4][2];
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const unsigned e = kb + 128u * t + 2u * (unsigned)lane + h;
                const float y = wgt[2 * (size_t)__builtin_elementwise_min(e, k1 - 1u)];
                x[t][h] = e < k1 ? y : 0.0f;   // +0 past the end: the identity of the sum
            }
#pragma unroll
        for (int t = 0; t < 4; t++)
            if (kb + 128u * t < k1) s = ordered_tile_sum<2>(s, x[t]);
    }
    if (lane == 0) values[v] = s;
}

// blocks [0, n_heavy_items): one long list each; the rest: NS_WAVES short lists each.  ONE launch, so that the short
// lists are summed beside the long ones
__global__ void __launch_bounds__(NS_WAVES * 64)
norm_sum_kernel(LatticeDev L, float* __restrict__ values, unsigned n_heavy_items) {
    __shared__ __attribute__((aligned(16))) float buf[NS_RING][NS_BATCH];
    if (L.counters[1]) return;   // hash overflow (flagged): the CSR arrays are incomplete, touch nothing
    if (blockIdx.x < n_heavy_items) norm_sum_heavy(L, values, blockIdx.x, buf);
    else norm_sum_light(L, values, blockIdx.x - n_heavy_items, n_heavy_items != 0u);
}
// the same without the LDS ring (chunks of many frames: no heavy blocks -- see launch_norm_sum)
__global__ void __launch_bounds__(NS_WAVES * 64)
norm_sum_light_kernel(LatticeDev L, float* __restrict__ values) {
    if (L.counters[1]) return;
    norm_sum_light(L, values, blockIdx.x, false);
}

static void launch_norm_sum(const LatticeDev& L, float* values, hipStream_t s) {
    const unsigned nfg = ((unsigned)L.n_frames + (unsigned)L.n_groups - 1u) / (unsigned)L.n_groups;
    const unsigned long long max_mf = std::min<unsigned long long>(((unsigned long long)L.cap_f_mask + 1) / 2 + 1, (unsigned long long)L.m_bound);
    const unsigned n_light = nfg * (unsigned)((max_mf + NS_WAVES - 1) / NS_WAVES) * (unsigned)L.n_groups;
    // A block (and 32 KB of LDS) per long list pays where the launch waits for its longest chains: a frame or two, a
    // cloud.  In a chunk of many frames the lists are summed beside the feature kernels, which need the LDS and the
    // wave slots more (measured at 64 frames: step 11.85 -> 12.2 ms with heavy blocks), and no single chain matters.
    if (L.n_frames <= 4) {
        // a frame of N points has at most 7 N / NS_HEAVY lists that long
        const unsigned long long max_heavy = std::min<unsigned long long>(max_mf, (unsigned long long)(L.d + 1) * L.N / NS_HEAVY + 1);
        const unsigned n_heavy_items = nfg * (unsigned)max_heavy * (unsigned)L.n_groups;
        norm_sum_kernel<<<dim3(n_heavy_items + n_light), dim3(NS_WAVES * 64), 0, s>>>(L, values, n_heavy_items);
    } else {
        norm_sum_light_kernel<<<dim3(n_light), dim3(NS_WAVES * 64), 0, s>>>(L, values);
    }
    RV_LAUNCHED("norm_sum_kernel");
}

// ---------------------------------------------------------------------------------------------
// Scan blocks of the list-major walk: the long lists of launches that wait for their longest chains (a frame or two, a
// cloud).  One vertex per block: two producer waves like those of splat_group_item (128-entry tiles of products into a
// double-buffered LDS tile, register rings of entries and rows; the tiles alternate between the two, so each has two
// steps per tile and its row gathers a lead of six steps -- with one producer the 0.2 us steps outran its rings), and CC
// waves that add one class each with ordered_tile_sum: a wave scan per tile where the serial adder spends 128
// dependent additions per class.  Mode 0 on
// the loop's own contiguous Q * norm only (the FAST producer: padding lanes have weight 0, the rows are finite).
// The same launch carries the regular blocks for the shorter lists (LatticeDev::heavy_from tells them which to leave).
// ---------------------------------------------------------------------------------------------
constexpr unsigned SPLAT_HEAVY = 16384;   // entries from which a list gets a scan block

constexpr int SCAN_PROD = 2;   // producer waves of a scan block (tiles alternate between them)
constexpr int SCAN_NH = 4;     // entries per producer lane and tile: tiles of 256 (the adders' lanes take four addends each)
constexpr int SCAN_TE = 64 * SCAN_NH;

// producer PI of a scan block: tiles PI, PI + 2, ... -- tile k goes into buffer k & 1 between barriers k - 1 and k
template <int CC, int CB, int PI>
__device__ __forceinline__ void splat_scan_producer(const LatticeDev& L, const ValueView& src, unsigned my_k0, unsigned my_k1, unsigned n_steps,
                                                    int c0, float (*prod)[CB][SCAN_TE + 4]) {
    constexpr int NH = SCAN_NH, TE = SCAN_TE, RE_ = 8, RR_ = 4;
    constexpr int LW = CB <= 2 ? 2 : 4;              // floats fetched per row: one load instruction
    static_assert(CB <= 4 && LW <= CC, "class part");
    const int lane = threadIdx.x & 63;
    const int ls = c0 + LW <= CC ? c0 : CC - LW;     // the load stays inside the row; the part starts at x[..][c0 - ls]
    const int xo = c0 - ls;
    float x[RR_][NH][LW];
    float w[RE_][NH];
    unsigned pix[RE_][NH];
#pragma unroll
    for (int r = 0; r < RE_; r++)
#pragma unroll
        for (int h = 0; h < NH; h++) { w[r][h] = 0.f; pix[r][h] = 0u; }
    // loads are unconditional (indices clamped into the list): no divergent branch, counted waits.  `j` counts this
    // producer's own tiles: tile 2 j + PI
    auto load_entries = [&](unsigned j, int slot) {
#pragma unroll
        for (int h = 0; h < NH; h++) {
            unsigned k = my_k0 + (2u * j + PI) * (unsigned)TE + (unsigned)lane + 64u * h;
            k = k < my_k1 ? k : my_k1 - 1u;
            const uint2 pw = L.csr_pw[k];
            w[slot][h] = __uint_as_float(pw.y);
            pix[slot][h] = pw.x;
        }
    };
    auto gather_rows = [&](int eslot, int rslot) {
#pragma unroll
        for (int h = 0; h < NH; h++) load_row<LW>(src.base + (size_t)pix[eslot][h] * (unsigned)CC + (unsigned)ls, x[rslot][h]);
    };
#pragma unroll
    for (int i = 0; i < RE_ - 1; i++) load_entries((unsigned)i, i);
#pragma unroll
    for (int i = 0; i < RR_ - 1; i++) gather_rows(i, i);
    // stage j: barriers 2 j and 2 j + 1 of the block (n_steps + 1 in all), this producer's tile before its own one
    auto stage = [&](unsigned j, auto S) -> bool {
        constexpr int s = decltype(S)::value;
        const unsigned t = 2u * j + PI;
        if (2u * j > n_steps) return false;
        if (PI == 1) {
            __syncthreads();                       // barrier 2 j
            if (t > n_steps) return false;
        }
        if (t < n_steps) {
            const unsigned base = my_k0 + t * (unsigned)TE;
            const unsigned n_valid = my_k1 - base < (unsigned)TE ? my_k1 - base : (unsigned)TE;
            float (*pb)[TE + 4] = prod[t & 1u];
#pragma unroll
            for (int h = 0; h < NH; h++) {
                const bool in = (unsigned)lane + 64u * h < n_valid;
                const float wl = in ? w[s][h] : 0.0f;   // +0 past the list: the product is +0, the identity of the sum
#pragma unroll
                for (int c = 0; c < CB; c++) {
                    // class c0 + c sits at x[c + xo], xo = 0 or 1: a select between two registers, no indexed access
                    const float xv = xo ? x[s % RR_][h][c + 1 < LW ? c + 1 : c] : x[s % RR_][h][c];
                    pb[c][lane + 64 * h] = wl * xv;
                }
            }
        }
        load_entries(j + RE_ - 1, (s + RE_ - 1) % RE_);
        gather_rows((s + RR_ - 1) % RE_, (s + RR_ - 1) % RR_);
        __syncthreads();                           // barrier t
        if (PI == 0) {
            if (t + 1u > n_steps) return false;
            __syncthreads();                       // barrier 2 j + 1
        }
        return true;
    };
    for (unsigned j0 = 0;; j0 += RE_) {
        if (!ring_stages(j0, stage, std::make_integer_sequence<int, RE_>())) break;
    }
}

// classes per scan block: the CC classes of a vertex are split over ceil(CC / CB) blocks -- nine adder waves on one CU
// were bound by instruction issue (0.35 us per 128-entry step); three per block leave a wave per SIMD
template <int CC> struct ScanPart { static constexpr int CB = CC == 9 ? 3 : 4; static constexpr int NP = (CC + CB - 1) / CB; };

template <int CC>
__device__ __forceinline__ void splat_scan_item(const LatticeDev& L, const ValueView& src, float* __restrict__ values, unsigned item,
                                                float (*prod)[ScanPart<CC>::CB][SCAN_TE + 4]) {
    constexpr int TE = SCAN_TE, CB = ScanPart<CC>::CB, NP = ScanPart<CC>::NP;
    static_assert(SCAN_NH == 4, "the adders read float4");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave >= CB + SCAN_PROD) return;
    const NormItem it = norm_item(L, item / NP);
    if (!it.ok || it.r >= it.n_vert || it.r >= L.scan_ranks) return;
    const unsigned v = L.vorder[(unsigned)it.fs0 + it.r];
    const unsigned my_k0 = L.vstart[v], my_k1 = L.vend[v];
    if (my_k1 - my_k0 < L.heavy_from) return;   // (whole block) a regular block's
    const unsigned n_steps = (my_k1 - my_k0 + (unsigned)TE - 1u) / (unsigned)TE;
    const int c0 = (int)(item % NP) * CB;       // this block's classes: c0 .. min(c0 + CB, CC) - 1
    // every wave passes barriers 0 .. n_steps: tile t is complete at barrier t and is summed between barriers t and t + 1
    if (wave == 0) {
        __builtin_amdgcn_s_setprio(1);
        splat_scan_producer<CC, CB, 0>(L, src, my_k0, my_k1, n_steps, c0, prod);
    } else if (wave == 1) {
        __builtin_amdgcn_s_setprio(1);
        splat_scan_producer<CC, CB, 1>(L, src, my_k0, my_k1, n_steps, c0, prod);
    } else {
        // ---- adder of class c: entries 4 l .. 4 l + 3 of a tile in lane l
        __builtin_amdgcn_s_setprio(3);
        const int ci = wave - SCAN_PROD, c = c0 + ci;
        float acc = 0.0f;
        __syncthreads();
        for (unsigned t = 0; t < n_steps; t++) {
            const float4 q = *reinterpret_cast<const float4*>(&prod[t & 1u][ci][4 * lane]);
            const float wk[4] = {q.x, q.y, q.z, q.w};
            acc = ordered_tile_sum<4>(acc, wk);
            __syncthreads();
        }
        if (lane == 0 && c < CC) values[(size_t)v * CC + c] = acc;
    }
}

// blocks [0, n_scan_items): scan blocks; the rest: regular blocks of GV vertices (their waves beyond GV + 1 leave at once)
template <int CC, int GV>
__global__ void __launch_bounds__((GV + 1) * 64)
splat_mixed_kernel(LatticeDev L, ValueView src, float* __restrict__ values, unsigned n_scan_items) {
    static_assert(ScanPart<CC>::CB + SCAN_PROD <= GV + 1 && 2 * ScanPart<CC>::CB * (SCAN_TE + 4) <= 2 * GV * CC * (64 * 2 + 4), "block size, LDS");
    __shared__ __attribute__((aligned(16))) float prod[2][GV][CC][64 * 2 + 4];
    if (L.counters[1]) return;   // hash overflow (flagged): the CSR arrays are incomplete, touch nothing
    if (blockIdx.x < n_scan_items) {
        splat_scan_item<CC>(L, src, values, blockIdx.x, reinterpret_cast<float (*)[ScanPart<CC>::CB][SCAN_TE + 4]>(&prod[0][0][0][0]));
    } else {
        splat_group_item<0, CC, true, GV, true, 2>(L, src, CC, 0, CC, values, blockIdx.x - n_scan_items, prod);
    }
}

template <int CC, int GV>
static void splat_mixed_launch(const LatticeDev& L0, const ValueView& src, float* values, hipStream_t s) {
    LatticeDev L = L0;
    L.heavy_from = SPLAT_HEAVY;
    const unsigned nfg = walk_frames_per_group(L);
    const unsigned long long max_mf = walk_max_vertices(L);
    // a frame of N points has at most 7 N / SPLAT_HEAVY lists that long; and only as many ranks per frame as give every
    // scan block a CU of its own -- they are there to shorten the launch's longest chains, and cost ~60 instructions
    // per tile and class where the serial adder costs ~10, so a second round of them is a loss (measured: 8 - 16 frames
    // with a scan block for EVERY long list ran 4 - 28 % slower than without any)
    const unsigned long long max_heavy = std::min<unsigned long long>(max_mf, (unsigned long long)(L.d + 1) * L.N / SPLAT_HEAVY + 1);
    const unsigned ranks_by_cus = (unsigned)resident_cu_count() / ((unsigned)ScanPart<CC>::NP * (unsigned)std::max(1, L.n_frames));
    L.scan_ranks = (unsigned)std::min<unsigned long long>(max_heavy, std::max(1u, ranks_by_cus));
    const unsigned n_scan = nfg * L.scan_ranks * (unsigned)L.n_groups * (unsigned)ScanPart<CC>::NP;
    const unsigned n_regular = splat_walk_items(L, GV);
    splat_mixed_kernel<CC, GV><<<dim3(n_scan + n_regular), dim3((GV + 1) * 64), 0, s>>>(L, src, values, n_scan);
    RV_LAUNCHED("splat_mixed_kernel");
}

// vertices per block of the list-major walk for C = 8, 9 (rvseg_schedule.group_vertices: 0 = by the chunk's shape)
static int splat_gv_choice(const LatticeDev& L) {
    if (L.group_vertices == 6 || L.group_vertices == 7) return L.group_vertices;
    // few frames: the launch waits for its longest chains (steps x step time), so the shorter step wins;
    // many frames: the launch is bound by the bytes it moves, the block count only adds overhead
    // (with scan blocks for the longest lists the six-vertex shape wins up to 24 frames: 20 frames 5.12 vs 5.48 ms per
    // step, 24 frames 5.49 vs 5.98; 32 frames 7.15 vs 7.37 -- but there the resident bands take 7.03)
    return L.n_frames <= 24 ? 6 : 7;
}


void launch_splat(const LatticeDev& L, const ValueView& src, int C, int mode, float* values, hipStream_t s, bool own_q,
                  const SplatResidentDev* resident, int slot) {
    if (mode == 2) {
        if (L.ordered_sum_scan) launch_norm_sum(L, values, s);
        else splat_group_launch<2, 1>(L, src, 1, 0, 1, values, s);
        return;
    }
    const bool contig = src.frame_stride == (size_t)L.N * (size_t)C && src.layer_off == 0;
    if (mode == 0 && own_q && contig && (C == 9 || C == 8) && resident) {
        // resident band schedule (the kernel walks the lists the list-major way itself should the planner have given up)
        if (launch_splat_resident(L, *resident, C, src.base, values, slot, s)) return;
    }
    if (mode == 0 && own_q && contig && (C == 9 || C == 8)) {
        // the mean-field loop's own input (Q * norm written by the previous update): the fast producer, and the
        // block shape chosen for the chunk
        const int gv = splat_gv_choice(L);
        const auto launch = [&](auto cc) {
            constexpr int CC = decltype(cc)::value;
            // six vertices per block go with 128-entry tiles: both serve launches whose time is their longest chain
            // launches of <= 16 frames wait for their longest chains: those get scan blocks, as many as there are CUs
            if (gv == 6 && L.ordered_sum_scan) splat_mixed_launch<CC, 6>(L, src, values, s);
            else if (gv == 6) splat_group_launch_g<0, CC, 6, true, 2>(L, src, C, 0, CC, values, s);
            else splat_group_launch_g<0, CC, SplatGroup<CC>::G, true>(L, src, C, 0, CC, values, s);
        };
        if (C == 9) launch(std::integral_constant<int, 9>());
        else launch(std::integral_constant<int, 8>());
        return;
    }
    for (int c0 = 0; c0 < C; c0 += 16) {
        const int n = C - c0 < 16 ? C - c0 : 16;
        if (mode == 0) splat_group_pass<0>(L, src, C, c0, n, values, s);
        else splat_group_pass<1>(L, src, C, c0, n, values, s);
    }
}

}  // namespace rvseg
