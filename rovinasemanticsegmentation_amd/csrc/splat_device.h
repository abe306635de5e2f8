// Device code private to kernels_splat.hip and kernels_resident.hip: DPP wave reductions, block shape, the unrolled
// stage walk and one item of the list-major walk.  (rvseg_crf.h is the host-side launch interface.)
#pragma once
#include <type_traits>
#include <utility>

#include "device_math.h"
#include "rvseg_crf.h"

namespace rvseg {

// wave reductions over DPP (the normaliser's ordered sums, the resident planner)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_term(float v) {   // the DPP-selected lane's v, +0 where the pattern selects none
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, true));
}
// sum over the wave, valid in lane 63 (inclusive row scans, then the row totals travel up)
__device__ __forceinline__ float wave_total_lane63(float v) {
    v += dpp_term<0x111, 0xf>(v);   // row_shr:1
    v += dpp_term<0x112, 0xf>(v);   // row_shr:2
    v += dpp_term<0x114, 0xf>(v);   // row_shr:4
    v += dpp_term<0x118, 0xf>(v);   // row_shr:8
    v += dpp_term<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
    v += dpp_term<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
    return v;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_term_u(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, true);
}
// sum over the wave, the same value in every lane
__device__ __forceinline__ unsigned wave_total_u32(unsigned v) {
    v += dpp_term_u<0x111, 0xf>(v);
    v += dpp_term_u<0x112, 0xf>(v);
    v += dpp_term_u<0x114, 0xf>(v);
    v += dpp_term_u<0x118, 0xf>(v);
    v += dpp_term_u<0x142, 0xa>(v);
    v += dpp_term_u<0x143, 0xc>(v);
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_term_keep(unsigned v) {   // the DPP-selected lane's v, ~0 where the pattern selects none
    return (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROW_MASK, 0xf, false);
}
// minimum over the wave, the same value in every lane
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
    unsigned t;
    t = dpp_term_keep<0x111, 0xf>(v); v = t < v ? t : v;
    t = dpp_term_keep<0x112, 0xf>(v); v = t < v ? t : v;
    t = dpp_term_keep<0x114, 0xf>(v); v = t < v ? t : v;
    t = dpp_term_keep<0x118, 0xf>(v); v = t < v ? t : v;
    t = dpp_term_keep<0x142, 0xa>(v); v = t < v ? t : v;
    t = dpp_term_keep<0x143, 0xc>(v); v = t < v ? t : v;
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// ---------------------------------------------------------------------------------------------
// splat as an ordered gather: one lane per (vertex, class) chain.
//   values[v][c] = sum over the vertex's entries, ascending point index, of fl(w * in[p][c])
//   with in[p][c] = fl(Q[p][c] * norm[p]) when `scaled` (DenseKernel::filter, pairwise.cpp:66)
// Per tile of 64 list entries the lanes of a producer wave form the 64 x C products in parallel
// (coalesced reads of the CSR pairs, one gathered Q row per lane) and park them in LDS; a lane
// (vertex, class) of the adder wave then adds the tile's products in list order -- the only part
// that has to be sequential.
// MODE 0: in = src[p*C+c]; 1: in = fl(src*norm) (per-entry normaliser csr_nrm); 2: in = 1 (normaliser pass).
// CC = classes handled by a pass (compile time, so the body is branch-free and the compiler keeps
// counted vmcnt waits); classes [c0, c0 + n_store) are stored, n_store <= CC.
// ---------------------------------------------------------------------------------------------
// The first version ran one wave per vertex (products and adds in the same wave).  PMC showed it
// issue bound: of ~150 instructions per 64-entry tile, 64 adds + 16 LDS reads run with only C of 64
// lanes busy.  Here a block owns G = 64 / CC vertices of similar list length (neighbours in
// `vorder`): wave i < G forms the products of vertex i's tile t exactly as above, and ONE extra
// wave adds them for all G vertices at once -- lane (i, c) walks vertex i's class-c products in
// list order -- so the sequential phase costs 64 adds per G tiles.  Products are double buffered:
// the adder works on tile t while the producers write tile t + 1; one barrier per tile.
template <int CC> struct SplatGroup { static constexpr int G = 64 / CC > 8 ? 8 : 64 / CC; };
// A vertex's chain advances one tile per barrier, so the loads of a tile have to be in flight for
// many tiles: {point, weight} pairs are fetched SPLAT_RE - 1 tiles ahead and the Q rows they point at
// SPLAT_RR - 1 tiles ahead (a ring of 3 / 2 tiles stalled a memory round trip per tile).
constexpr int SPLAT_RE = 16, SPLAT_RR = 8;   // RR must divide RE
static_assert(SPLAT_RE % SPLAT_RR == 0, "ring positions are compile-time: the row ring has to divide the entry ring");
// The unrolled walk of a producer's rings: stages 0 .. RE - 1 of tiles t0 .., each handed its ring position as a
// compile-time constant (the rings live in registers).  Stops at the first stage that returns false, so no stage is
// reachable past a skipped one and the compiler keeps counted vmcnt waits; false tells the caller to leave its loop.
template <class Stage, int... I>
__device__ __forceinline__ bool ring_stages(unsigned t0, Stage& stage, std::integer_sequence<int, I...>) {
    return (stage(t0 + I, std::integral_constant<int, I>()) && ...);
}

// GV = vertices per block (<= G).  With GV = G the block is G producer waves + the adder as the last wave.  A block
// with fewer vertices (GV = 6 for C = 9: 7 waves) puts the adder at wave 3: a workgroup's waves go to the four SIMDs
// in cyclic order (MI355X_MICROARCH.md, LDS section), so waves w and w + 4 share a SIMD and wave 3 of a 7-wave block
// has one to itself -- its 64 dependent adds per step no longer compete with a producer for issue slots.  That
// shortens a step (the critical path of launches with few, long chains: a single frame, a 1280x960 chunk, a cloud)
// at the price of 7/6 as many block-steps; chunks with many frames are bandwidth bound and keep GV = G.
// FAST: the input is this library's own Q * norm (finite, >= 0) in one contiguous [point][C] matrix: a padding lane's
// product is 0 * x = +0 by itself (no select), and the row address needs no per-frame split.
// One item of the list-major walk: G vertices of one frame, whole lists.  splat_group_kernel runs one item per block; the
// resident kernel falls back to a loop over these items when its planner gave up.
// NH = entries per producer lane and tile: 1 (64-entry tiles, rings of 16 / 8 tiles) or 2 (128-entry tiles, rings of 8 / 4:
// the same look-ahead in time).  A launch whose time is its longest chain (a single frame, a cloud, chunks of <= 16
// frames) pays the per-tile costs -- barrier, table reads, the wait for the first product row -- per 128 dependent adds
// instead of per 64 with NH = 2.
template <int MODE, int CC, bool FULL, int GV, bool FAST, int NH = 1>
__device__ __forceinline__ void splat_group_item(const LatticeDev& L, const ValueView& src, int C, int c0, int n_store, float* __restrict__ values,
                                                 unsigned item, float (*prod)[GV][CC][64 * NH + 4]) {
    constexpr int G = GV;
    constexpr int TE = 64 * NH;                       // entries per tile
    constexpr int RE_ = NH == 2 ? 8 : SPLAT_RE, RR_ = NH == 2 ? 4 : SPLAT_RR;
    static_assert(NH == 1 || NH == 2, "entries per lane");
    constexpr int AW = (GV < SplatGroup<CC>::G && GV >= 4) ? 3 : GV;   // the adder's wave index
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // item b -> XCD group b % n_groups (the dispatcher deals blocks round-robin over the 8 XCDs), item
    // b / n_groups inside it.  A group owns the frames f = g, g + n_groups, ...: all readers of a
    // frame's Q rows share one L2.  Item j = (rank r, frame slot q): the r-th heaviest G vertices of
    // that frame -- every frame's heaviest vertices are dispatched first.
    const unsigned g = item % (unsigned)L.n_groups, j = item / (unsigned)L.n_groups;
    const unsigned nfg = ((unsigned)L.n_frames - g + (unsigned)L.n_groups - 1u) / (unsigned)L.n_groups;   // frames of this group
    if (nfg == 0) return;
    const unsigned r = j / nfg, frame = g + (j - r * nfg) * (unsigned)L.n_groups;
    const int Mtot = L.counters[0] < L.m_bound ? L.counters[0] : L.m_bound;
    const int2 fr = lattice_frame_range(L, (int)frame, Mtot);
    const unsigned n_vert = (unsigned)(fr.y - fr.x), gstart = (unsigned)fr.x;
    if (r * G >= n_vert) return;
    const bool contig = FAST || (src.frame_stride == (size_t)L.N * (size_t)C && src.layer_off == 0);
    const int pw = wave < AW ? wave : wave - 1;   // producer index of this wave (unused by the adder)
    {
        // every wave reads the group's G list ranges itself (uniform): no broadcast step
        unsigned n_steps = 0, my_k0 = 0, my_k1 = 0;
        for (int i = 0; i < G; i++) {
            const unsigned idx = r * G + i;
            if (idx < n_vert) {
                const unsigned v = L.vorder[gstart + idx];
                const unsigned k0 = L.vstart[v], k1 = L.vend[v];
                if (idx < L.scan_ranks && k1 - k0 >= L.heavy_from) continue;   // a scan block's (splat_scan_item)
                const unsigned nt = (k1 - k0 + (unsigned)TE - 1u) / (unsigned)TE;
                n_steps = nt > n_steps ? nt : n_steps;
                if (i == pw && wave != AW) { my_k0 = k0; my_k1 = k1; }
            }
        }
        // the adder's 64 dependent adds are the critical path of every step: it wins issue arbitration
        // against the producers (which run a tile ahead and have slack)
        if (wave == AW) __builtin_amdgcn_s_setprio(3);
        else if (n_steps > 256u) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
        if (wave != AW) {
            // ---- producer of vertex `wave`: barriers 0 .. n_steps - 1 close its tiles, one more ends the item
            const bool has = my_k1 > my_k0;
            const unsigned kc0 = has ? my_k0 : 0u, kc1 = has ? my_k1 : 1u;   // clamp range of the loads (entry 0 exists)
            const unsigned n_tiles = has ? (my_k1 - my_k0 + (unsigned)TE - 1u) / (unsigned)TE : 0u;
            float x[RR_][NH][CC];
            float w[RE_][NH], nrm[RE_][NH];
            unsigned pix[RE_][NH];
#pragma unroll
            for (int r = 0; r < RE_; r++)
#pragma unroll
                for (int h = 0; h < NH; h++) { w[r][h] = 0.f; nrm[r][h] = 1.f; pix[r][h] = 0u; }
            // loads are unconditional (indices clamped into the list): no divergent branch, counted waits
            auto load_entries = [&](unsigned tile, int slot) {
#pragma unroll
                for (int h = 0; h < NH; h++) {
                    unsigned k = kc0 + tile * (unsigned)TE + (unsigned)lane + 64u * h;
                    k = k < kc1 ? k : kc1 - 1u;
                    const uint2 pw = L.csr_pw[k];
                    w[slot][h] = __uint_as_float(pw.y);
                    pix[slot][h] = pw.x;
                    if (MODE == 1) nrm[slot][h] = L.csr_nrm[k];
                }
            };
            auto gather_rows = [&](int eslot, int rslot) {
                if (MODE == 2) return;
#pragma unroll
                for (int h = 0; h < NH; h++) {
                    // one frame-contiguous [point][C] matrix (the single-layer case): no division by N
                    const size_t row = contig ? (size_t)pix[eslot][h] * (unsigned)C + (unsigned)c0 : src.index(pix[eslot][h], c0, C, L.N);
                    if (FULL) {
                        load_row<CC>(src.base + row, x[rslot][h]);
                    } else {
#pragma unroll
                        for (int c = 0; c < CC; c++) x[rslot][h][c] = src.base[row + (c < n_store ? c : n_store - 1)];
                    }
                }
            };
#pragma unroll
            for (int i = 0; i < RE_ - 1; i++) load_entries((unsigned)i, i);
#pragma unroll
            for (int i = 0; i < RR_ - 1; i++) gather_rows(i, i);
            // one tile: products -> LDS, refill the two rings, barrier.  `S` is its ring position (ring_stages)
            auto stage = [&](unsigned t, auto S) -> bool {
                constexpr int s = decltype(S)::value;
                if (t >= n_steps) return false;
                const unsigned base = my_k0 + t * (unsigned)TE;
                const unsigned n_valid = t < n_tiles ? (my_k1 - base < (unsigned)TE ? my_k1 - base : (unsigned)TE) : 0u;
                float (*pb)[TE + 4] = prod[t & 1u][pw];
#pragma unroll
                for (int h = 0; h < NH; h++) {
                    const bool in = (unsigned)lane + 64u * h < n_valid;
                    const float wl = in ? w[s][h] : 0.0f;
#pragma unroll
                    for (int c = 0; c < CC; c++) {
                        float xin = MODE == 2 ? 1.0f : x[s % RR_][h][c];
                        if (MODE == 1) xin = xin * nrm[s][h];
                        const float pr = wl * xin;
                        // +0 past the list: identity of the sum (FAST: wl is 0 there and the row is finite, so pr is +0 already)
                        pb[c][lane + 64 * h] = (FAST || in) ? pr : 0.0f;
                    }
                }
                load_entries(t + RE_ - 1, (s + RE_ - 1) % RE_);
                gather_rows((s + RR_ - 1) % RE_, (s + RR_ - 1) % RR_);
                __syncthreads();
                return true;
            };
            for (unsigned t0 = 0;; t0 += RE_) {
                if (!ring_stages(t0, stage, std::make_integer_sequence<int, RE_>())) break;
            }
            __syncthreads();
        } else {
            // ---- adder: lane (i, c) owns the chain of vertex i, class c
            const int gi = lane < G * CC ? lane / CC : 0, c = lane < G * CC ? lane % CC : 0;
            const unsigned idx = r * G + gi;
            bool mine = lane < G * CC && idx < n_vert && c < n_store;
            const unsigned cv = mine ? L.vorder[gstart + idx] : 0u;
            if (mine && idx < L.scan_ranks && L.vend[cv] - L.vstart[cv] >= L.heavy_from) mine = false;   // a scan block's
            float acc = 0.0f;
            __syncthreads();
            for (unsigned t = 0; t < n_steps; t++) {
                const float* pr = prod[t & 1u][gi][c];
                float4 q[16 * NH];
#pragma unroll
                for (int i = 0; i < 16 * NH; i++) q[i] = reinterpret_cast<const float4*>(pr)[i];
#pragma unroll
                for (int i = 0; i < 16 * NH; i++) { acc += q[i].x; acc += q[i].y; acc += q[i].z; acc += q[i].w; }
                __syncthreads();
            }
            if (mine) values[(size_t)cv * C + c0 + c] = acc;
        }
    }
}

}  // namespace rvseg
