// Resident band schedule of the ordered splat for gfx950: planner, seal and fill kernels, the kernel that walks the
// schedule (fallback: the list-major walk, splat_group_item) and its per-device set-up caches.
#include <atomic>

#include "splat_device.h"

namespace rvseg {

// ---------------------------------------------------------------------------------------------
// Resident band schedule of the ordered splat (SplatResidentDev, rvseg_crf.h).
// ---------------------------------------------------------------------------------------------
// piece of frame-local vertex lv inside band b: [k0, k1) of its list
__device__ __forceinline__ void resident_piece(const LatticeDev& L, int band_wb, int f0, int Mf, int lv, int b, unsigned& k0, unsigned& k1) {
    const unsigned* fb = L.bh + (size_t)L.wbpf * f0 + lv;
    const int w0 = b * band_wb, w1 = w0 + band_wb;
    k0 = fb[(size_t)w0 * Mf];
    k1 = w1 < L.wbpf ? fb[(size_t)w1 * Mf] : L.vend[f0 + lv];
}

// One block per frame: deals the frame's vertices to the B blocks and numbers the tiles.  A block's tile count is
// sum over bands of max(chunks of its longest vertex there, all its chunks there / 7), so the heavy vertices are placed
// one at a time, longest first, each into the block whose count ends up smallest -- evaluated exactly, band by band,
// by the whole workgroup (`profiles/analysis`: 1 111 tiles for the fullest block of a bench frame, which is the chain
// of its heaviest vertex, against 1 346 when the blocks are balanced by chunk totals).  The many short vertices
// that follow go to the block with the fewest tiles so far, priced at chunks / 7.
constexpr int RES_PLAN_THREADS = 1024;
constexpr int RES_HEAVY_MAX = 160;   // vertices placed exactly at most (numpy on a bench frame: 96 reach the result of 200; other frames need more)
// dynamic LDS: T[B][nb] words, then the heavy table [heavy_cap][nb] bytes
__global__ void __launch_bounds__(RES_PLAN_THREADS)
resident_plan_kernel(LatticeDev L, SplatResidentDev R, int heavy_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned plan_lds[];
    __shared__ unsigned chv[RES_MAX_VERTS];
    __shared__ unsigned short own[RES_MAXB][RES_MAX_OWNV];
    __shared__ unsigned nown[RES_MAXB], nheavy[RES_MAXB];
    __shared__ unsigned short lvo[RES_MAX_VERTS];   // the frame's vertices, longest list first (`vorder`, frame-local)
    __shared__ unsigned cur[RES_MAXB];
    __shared__ unsigned blk0[RES_MAXB + 1];
    __shared__ int bad, choice;
    if (L.counters[1]) return;
    const int frame = blockIdx.x;
    const int Mtot = L.counters[0] < L.m_bound ? L.counters[0] : L.m_bound;
    const int2 fr = lattice_frame_range(L, frame, Mtot);
    const int f0 = fr.x, Mf = fr.y - fr.x, nb = R.n_bands, B = R.B;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned clog = (unsigned)R.chunk_log2, cmask = (1u << clog) - 1u;   // entries per chunk: 64 or 128
    unsigned* T = plan_lds;                                               // [B][nb]: greedy: (sum of chunks) << 8 | longest; then tiles, then their scan
    unsigned char* hc = reinterpret_cast<unsigned char*>(plan_lds + B * nb);   // [heavy_cap][nb]
    if (tid == 0) { bad = 0; choice = 0; }
    if (tid < RES_MAXB) { nown[tid] = 0; nheavy[tid] = 0; cur[tid] = 0; }
    for (int i = tid; i < B * nb; i += RES_PLAN_THREADS) T[i] = 0;
    for (int lv = tid; lv < RES_MAX_VERTS; lv += RES_PLAN_THREADS) chv[lv] = 0;
    __syncthreads();
    if (Mf > RES_MAX_VERTS) {
        if (tid == 0) atomicAdd(&R.flags[0], 1);
        return;
    }
    for (int k = tid; k < Mf; k += RES_PLAN_THREADS) {
        const int lv = (int)L.vorder[f0 + k] - f0;
        lvo[k] = (unsigned short)(lv < 0 ? 0 : (lv >= Mf ? Mf - 1 : lv));
    }
    // 64-entry chunks of every vertex, summed over the bands: one (vertex, band) piece per thread and step
    for (int i = tid; i < Mf * nb; i += RES_PLAN_THREADS) {
        const int b = i / Mf, lv = i - b * Mf;   // consecutive threads: consecutive vertices of one band (the table's row)
        unsigned k0, k1;
        resident_piece(L, R.band_wb, f0, Mf, lv, b, k0, k1);
        const unsigned ch = (k1 - k0 + cmask) >> clog;
        if (ch) atomicAdd(&chv[lv], ch);
    }
    __syncthreads();
    // heavy = at least 12 chunks; `vorder` is sorted by length, so they are (about) a prefix of it: its length is counted
    if (tid < heavy_cap && tid < Mf && chv[lvo[tid]] >= (12u >> (clog - 6))) atomicAdd(&choice, 1);
    __syncthreads();
    const int n_heavy = choice;
    __syncthreads();
    // their chunks per band, once, in LDS: the placement loop below touches no global memory
    for (int i = tid; i < n_heavy * nb; i += RES_PLAN_THREADS) {
        const int k = i / nb, b = i - k * nb;
        unsigned k0, k1;
        resident_piece(L, R.band_wb, f0, Mf, lvo[k], b, k0, k1);
        hc[i] = (unsigned char)((k1 - k0 + cmask) >> clog);
    }
    __syncthreads();
    // ---- the heavy vertices, exactly, by ONE wave (lane = band): the loop is a chain of up to 160 dependent decisions,
    // and with the whole workgroup on it every decision cost three block-wide barriers and an LDS round trip through
    // thread 0 (0.45 ms per launch, 88 % of the wave cycles waiting); a single wave needs no barrier at all, the tile
    // counts of the B candidate blocks are B independent DPP reductions
    if (wave == 0) {
        for (int k = 0; k < n_heavy; k++) {
            const unsigned char* cb = hc + (size_t)k * nb;
            int best = -1; unsigned best_t = 0, best_inc = 0;
            for (int j = 0; j < B; j++) {
                unsigned sum = 0;
                for (int b = lane; b < nb; b += 64) {
                    const unsigned pk = T[j * nb + b], c = cb[b];
                    const unsigned mx = (pk & 255u) > c ? (pk & 255u) : c, t7 = ((pk >> 8) + c + 6u) / 7u;
                    sum += mx > t7 ? mx : t7;
                }
                const unsigned t = wave_total_u32(sum);
                if (nown[j] >= (unsigned)RES_MAX_OWNV) continue;
                const unsigned inc = t - cur[j];
                if (best < 0 || t < best_t || (t == best_t && inc < best_inc)) { best = j; best_t = t; best_inc = inc; }
            }
            if (best < 0) { if (lane == 0) bad = 1; break; }
            for (int b = lane; b < nb; b += 64) {
                const unsigned pk = T[best * nb + b], c = cb[b];
                T[best * nb + b] = (((pk >> 8) + c) << 8) | ((pk & 255u) > c ? (pk & 255u) : c);
            }
            if (lane == 0) { cur[best] = best_t; own[best][nown[best]] = lvo[k]; nown[best] = nown[best] + 1u; }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // one wave: LDS in program order; keeps the compiler from caching T / cur / nown
        }
    }
    __syncthreads();
    if (bad) { if (tid == 0) atomicAdd(&R.flags[0], 1); return; }
    // ---- the rest: fewest tiles so far, a vertex priced at chunks / 7 (sevenths of a tile).  One wave, lane j = block j:
    // the running prices live in registers and the cheapest block is a DPP minimum (until round 3 thread 0 walked a
    // private array -- scratch memory -- through this loop: 0.6 ms of the deep scene's 2.8 ms planner, 2 159 light vertices)
    if (wave == 0) {
        const bool blk = lane < B;
        unsigned price = blk ? cur[lane] * 7u : 0xFFFFFFFFu;
        unsigned cnt = blk ? nown[lane] : 0u;
        if (blk) nheavy[lane] = cnt;
        for (int k = n_heavy; k < Mf; k++) {
            const int lv = lvo[k];
            const bool room = blk && cnt < (unsigned)RES_MAX_OWNV;
            const unsigned cand = room ? price : 0xFFFFFFFFu;
            const unsigned best_price = wave_min_u32(cand);
            const unsigned long long at = __ballot(room && cand == best_price);
            if (!at || lv < 0 || lv >= Mf) { if (lane == 0) bad = 1; break; }
            const int best = __ffsll((long long)at) - 1;      // the lowest block among equals, as the serial loop chose
            if (lane == best) {
                price += chv[lv] + 1u;
                own[best][cnt] = (unsigned short)lv;
                cnt++;
            }
        }
        if (blk) nown[lane] = cnt;
    }
    __syncthreads();
    if (bad) { if (tid == 0) atomicAdd(&R.flags[0], 1); return; }
    // tiles of every (block, band): the light vertices' chunks join the packed sums, a wave per (block, band)
    for (int idx = wave; idx < B * nb; idx += RES_PLAN_THREADS / 64) {
        const int j = idx / nb, b = idx - j * nb;
        unsigned sum = 0, mx = 0;
        for (unsigned u = nheavy[j] + lane; u < nown[j]; u += 64) {
            unsigned k0, k1;
            resident_piece(L, R.band_wb, f0, Mf, own[j][u], b, k0, k1);
            const unsigned ch = (k1 - k0 + cmask) >> clog;
            sum += ch;
            mx = ch > mx ? ch : mx;
        }
        for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o, 64); const unsigned m2 = __shfl_xor(mx, o, 64); mx = m2 > mx ? m2 : mx; }
        if (lane == 0) {
            const unsigned pk = T[idx];
            sum += pk >> 8; mx = (pk & 255u) > mx ? (pk & 255u) : mx;
            const unsigned t = (sum + 6u) / 7u;
            T[idx] = t > mx ? t : mx;
        }
    }
    __syncthreads();
    if (tid < B) {
        unsigned run = 0;
        for (int b = 0; b < nb; b++) { const unsigned t = T[tid * nb + b]; T[tid * nb + b] = run; run += t; }
        blk0[tid + 1] = run;
    }
    __syncthreads();
    if (tid == 0) {
        blk0[0] = 0;
        for (int j = 0; j < B; j++) blk0[j + 1] += blk0[j];
        if (blk0[B] > R.cap_tiles) bad = 1;
    }
    __syncthreads();
    if (bad) { if (tid == 0) atomicAdd(&R.flags[0], 1); return; }
    unsigned* jb = R.jb_tile + (size_t)frame * RES_MAXB * (nb + 1);
    for (int idx = tid; idx < B * (nb + 1); idx += RES_PLAN_THREADS) {
        const int j = idx / (nb + 1), b = idx - j * (nb + 1);
        jb[idx] = b < nb ? blk0[j] + T[j * nb + b] : blk0[j + 1];
    }
    for (int j = tid; j <= B; j += RES_PLAN_THREADS) R.blk_tile0[(size_t)frame * (RES_MAXB + 1) + j] = blk0[j];
    for (int j = tid; j < B; j += RES_PLAN_THREADS) R.blk_nown[(size_t)frame * RES_MAXB + j] = nown[j];
    for (int idx = tid; idx < B * RES_MAX_OWNV; idx += RES_PLAN_THREADS) {
        const int j = idx / RES_MAX_OWNV, u = idx - j * RES_MAX_OWNV;
        R.blk_verts[((size_t)frame * RES_MAXB + j) * RES_MAX_OWNV + u] = (unsigned)u < nown[j] ? own[j][u] : (unsigned short)0;
    }
}

__global__ void resident_seal_kernel(LatticeDev L, SplatResidentDev R) {
    R.flags[1] = (R.flags[0] == 0 && L.counters[1] == 0) ? 1 : 0;
}

// One wave per (block, band): packs the chunks of the block's vertices into the band's T tiles x 7 slots by the
// wrap-around rule.  The cells are numbered slot after slot; a vertex takes the next `chunks` cells (a prefix sum over
// the block's vertices, kept in LDS), and when its cells run over the end of a slot it continues at the top of the next
// one.  Because a vertex has at most T chunks the two parts never share a tile, and its chunks are numbered by tile,
// so they are summed in list order whatever slot they sit in.  The cells are then written lane = cell (coalesced
// stores), each lane finding its vertex by bisection of the prefix sums.
__global__ void __launch_bounds__(256)
resident_fill_kernel(LatticeDev L, SplatResidentDev R) {
    __shared__ unsigned s_pre[4][RES_MAX_OWNV + 1], s_k0[4][RES_MAX_OWNV], s_len[4][RES_MAX_OWNV];
    if (!R.flags[1]) return;
    const int frame = blockIdx.y;
    const int nb = R.n_bands, B = R.B;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int idx = blockIdx.x * 4 + wv;
    if (idx >= B * nb) return;
    const int j = idx / nb, b = idx - j * nb;
    const int Mtot = L.counters[0] < L.m_bound ? L.counters[0] : L.m_bound;
    const int2 fr = lattice_frame_range(L, frame, Mtot);
    const int f0 = fr.x, Mf = fr.y - fr.x;
    const unsigned* jb = R.jb_tile + ((size_t)frame * RES_MAXB + j) * (nb + 1);
    const unsigned t0 = jb[b], T = jb[b + 1] - t0;
    if (!T) return;
    const unsigned n_own = R.blk_nown[(size_t)frame * RES_MAXB + j];
    const unsigned short* verts = R.blk_verts + ((size_t)frame * RES_MAXB + j) * RES_MAX_OWNV;
    const unsigned base = (unsigned)frame * (unsigned)L.N * 7u;   // the frame's first entry (csr_scan_kernel)
    unsigned* pre = s_pre[wv]; unsigned* k0s = s_k0[wv]; unsigned* lens = s_len[wv];
    const unsigned clog = (unsigned)R.chunk_log2, cmask = (1u << clog) - 1u, CH = 1u << clog;
    unsigned run = 0, hmax = 0;
    unsigned any_k0 = 0xFFFFFFFFu;    // an entry of this band: what an unused cell points at (weight 0)
    for (unsigned u0 = 0; u0 < n_own; u0 += 64) {
        const unsigned u = u0 + lane;
        unsigned k0 = 0, len = 0;
        if (u < n_own) { unsigned k1; resident_piece(L, R.band_wb, f0, Mf, verts[u], b, k0, k1); len = k1 - k0; }
        const unsigned ch = (len + cmask) >> clog;
        unsigned incl = ch;
        for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
        if (u < n_own) { pre[u] = run + incl - ch; k0s[u] = k0; lens[u] = len; }
        hmax = len > hmax ? len : hmax;
        const unsigned long long has = __ballot(ch != 0u);
        if (any_k0 == 0xFFFFFFFFu && has) any_k0 = __shfl(k0, __ffsll((long long)has) - 1, 64);
        run += __shfl(incl, 63, 64);
    }
    if (lane == 0) pre[n_own] = run;
    for (int o = 32; o > 0; o >>= 1) { const unsigned m2 = __shfl_xor(hmax, o, 64); hmax = m2 > hmax ? m2 : hmax; }
    hmax = hmax > CH ? CH : hmax;   // height of the band's tiles for the adder (16 / 32 / 64 / 128 adds)
    __builtin_amdgcn_wave_barrier();   // (one wave: its LDS writes are in order before the reads below)
    unsigned* info = R.tinfo + (size_t)frame * R.cap_tiles + t0;
    for (unsigned t = lane; t < T; t += 64) info[t] = ((unsigned)b << 16) | hmax;
    for (unsigned q = lane; q < 7u * T; q += 64) {
        unsigned u = n_own, at = any_k0, n = 0;
        if (q < run) {
            unsigned lo = 0, hi = n_own;   // the vertex with pre[u] <= q < pre[u + 1]
            while (hi - lo > 1u) { const unsigned mid = (lo + hi) >> 1; if (pre[mid] <= q) lo = mid; else hi = mid; }
            u = lo;
            const unsigned p = pre[u], ch = pre[u + 1] - p, i = q - p;
            const unsigned room = T - p % T;                       // cells left in the slot where the vertex starts
            const unsigned wrap = ch > room ? ch - room : 0u;      // chunks at the top of the next slot: the FIRST ones (lower tiles)
            const unsigned chunk = i < room ? wrap + i : i - room;
            const unsigned len = lens[u];
            n = len - CH * chunk < CH ? len - CH * chunk : CH;
            at = k0s[u] + CH * chunk;
        }
        const unsigned s = q / T, t = q - s * T;
        R.tdesc[((size_t)frame * 7 + s) * R.cap_tiles + t0 + t] = ((at - base) << 8) | n;
        R.tvl[((size_t)frame * 7 + s) * R.cap_tiles + t0 + t] = (unsigned short)u;
    }
}

void launch_resident_plan(const LatticeDev& L, const SplatResidentDev& R, hipStream_t s) {
    (void)hipMemsetAsync(R.flags, 0, 2 * sizeof(int), s);
    // dynamic LDS of the planner: tile sums [B][n_bands] words + the heavy table, inside the 64 KB a block gets by default
    const size_t t_bytes = (size_t)R.B * R.n_bands * 4;
    const size_t fixed = (size_t)RES_MAX_VERTS * 4 + (size_t)RES_MAX_VERTS * 2 + RES_MAXB * RES_MAX_OWNV * 2 + 1024;
    int heavy_cap = RES_HEAVY_MAX;
    while (heavy_cap > 8 && fixed + t_bytes + (size_t)heavy_cap * R.n_bands > 60000) heavy_cap -= 8;
    const size_t dyn = t_bytes + (size_t)heavy_cap * R.n_bands + 16;
    resident_plan_kernel<<<dim3((unsigned)L.n_frames), dim3(RES_PLAN_THREADS), dyn, s>>>(L, R, heavy_cap);
    resident_seal_kernel<<<dim3(1), dim3(1), 0, s>>>(L, R);
    resident_fill_kernel<<<dim3((unsigned)((R.B * R.n_bands + 3) / 4), (unsigned)L.n_frames), dim3(256), 0, s>>>(L, R);
    RV_LAUNCHED("resident_plan_kernel / resident_seal_kernel / resident_fill_kernel");
}

// The splat over the schedule.  Block (frame, j): 7 producer waves + the adder, as in splat_group_kernel; the tile
// list replaces the walk down seven whole lists.  Producer i reads the descriptor stream of slot i 64 tiles at a time
// into one register (lane = tile), refreshed once per unrolled group of stages with an unconditional load, so the
// stage bodies index it with compile-time lanes and the loads of entries (RE - 1 tiles ahead) and rows (RR - 1 tiles
// ahead) run on across vertices and bands without a bubble.  The adder's lane (i, c) serves whatever vertex slot i
// holds in the tile: the running sums of the block's vertices sit in LDS, and a lane swaps its sum when the slot's
// vertex changes (store, then load: one wave, so a chain that moves to another slot in the next tile is handed over
// in order).  Pacing: at the first tile of a band the adder publishes the band and holds the block (by arriving late
// at the tile's barrier) while any block of its frame is more than `window` bands behind; the check uses the progress
// words fetched one band earlier, so it costs no round trip unless it waits, and the wait is bounded -- blocks never
// depend on each other for their results.
template <int CC, int RE, int RR, int TH>   // TH: entries per slot and tile (64 or 128)
__global__ void __launch_bounds__(512)
splat_resident_kernel(LatticeDev L, SplatResidentDev R, ValueView srcv, float* __restrict__ values, unsigned tag, int slot, unsigned n_items) {
    constexpr int G = 7, C = CC;
    static_assert(CC * G <= 64 && (RE == 16 || RE == 8) && RE % RR == 0 && (TH == 64 || TH == 128), "block shape");
    constexpr int NH = TH / 64;        // entries per lane and tile
    constexpr int ROW = TH + 4;        // product row: 16-B aligned, 4-bank skew
    // dynamic LDS (more than 64 KB for TH = 128): products [2][G][CC][ROW], running sums, the adder's table
    extern __shared__ __attribute__((aligned(16))) float res_lds[];
    float (*prod)[G][CC][ROW] = reinterpret_cast<float (*)[G][CC][ROW]>(res_lds);
    float* accs = res_lds + 2 * G * CC * ROW;
    unsigned (*ainfo)[64][8] = reinterpret_cast<unsigned (*)[64][8]>(accs + (RES_MAX_OWNV + 1) * CC);   // per tile and slot: vertex | height << 10 | band << 18
    if (L.counters[1]) return;
    if (!R.flags[1]) {
        // the planner gave up on some frame (more vertices or tiles than its tables hold): this grid walks the lists
        // the list-major way, G vertices per item
        for (unsigned item = blockIdx.x; item < n_items; item += gridDim.x) {
            splat_group_item<0, CC, true, G, true>(L, srcv, CC, 0, CC, values, item, reinterpret_cast<float (*)[G][CC][68]>(res_lds));
            __syncthreads();
        }
        return;
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // block b -> XCD b % NG; all B blocks of a frame on one XCD (frame f lives on XCD f % NG)
    const unsigned NG = (unsigned)L.n_groups, B = (unsigned)R.B;
    const unsigned x = blockIdx.x % NG, jj = blockIdx.x / NG;
    const unsigned j = jj % B, frame = (jj / B) * NG + x;
    if (frame >= (unsigned)L.n_frames) return;
    const int Mtot = L.counters[0] < L.m_bound ? L.counters[0] : L.m_bound;
    const int f0 = lattice_frame_range(L, (int)frame, Mtot).x;
    const unsigned tb = R.blk_tile0[(size_t)frame * (RES_MAXB + 1) + j], te = R.blk_tile0[(size_t)frame * (RES_MAXB + 1) + j + 1];
    const unsigned n_t = te - tb;
    const unsigned n_own = R.blk_nown[(size_t)frame * RES_MAXB + j];
    for (unsigned e = threadIdx.x; e < (n_own + 1u) * CC; e += 512) accs[e] = 0.0f;
    unsigned* prog = R.prog + ((size_t)slot * L.n_frames + frame) * RES_MAXB;
    const unsigned long long t_start = R.trace ? __builtin_amdgcn_s_memrealtime() : 0ull;
    const unsigned long long c_start = R.trace ? __builtin_amdgcn_s_memtime() : 0ull;
    unsigned long long t_spin = 0;
    if (wave == G) __builtin_amdgcn_s_setprio(3);
    else if (n_t > 256u) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
    if (wave < G) {
        if (n_t) {
            const unsigned* D = R.tdesc + ((size_t)frame * 7 + wave) * R.cap_tiles + tb;
            const unsigned base = frame * (unsigned)L.N * 7u;   // the frame's first entry (csr_scan_kernel: every point has d + 1 entries)
            const unsigned klast = base + (unsigned)L.N * 7u - 1u;
            float xr[RR][NH][CC];
            float w[RE][NH];
            unsigned pix[RE][NH];
#pragma unroll
            for (int r = 0; r < RE; r++)
#pragma unroll
                for (int h = 0; h < NH; h++) { w[r][h] = 0.f; pix[r][h] = 0u; }
            auto load_desc = [&](unsigned first) -> unsigned {
                const unsigned t = first + (unsigned)lane;
                return D[t < n_t ? t : n_t - 1u];
            };
            unsigned dcur = load_desc(0u), dnxt = dcur;
            auto load_entries = [&](unsigned d, int slot_e) {
                const unsigned n = d & 255u, last = n ? n - 1u : 0u;
#pragma unroll
                for (int h = 0; h < NH; h++) {
                    const unsigned i = (unsigned)lane + 64u * h;
                    unsigned k = base + (d >> 8) + (i < last ? i : last);
                    k = k < klast ? k : klast;
                    const uint2 e = L.csr_pw[k];
                    w[slot_e][h] = __uint_as_float(e.y);
                    pix[slot_e][h] = e.x;
                }
            };
            // (the rows come through a plain pointer: a const __restrict__ kernel argument makes the gathers invariant loads,
            // which the compiler then sinks to their use -- the whole prefetch distance lost)
            auto gather_rows = [&](int eslot, int rslot) {
#pragma unroll
                for (int h = 0; h < NH; h++) load_row<CC>(srcv.base + (size_t)pix[eslot][h] * (unsigned)C, xr[rslot][h]);
            };
#pragma unroll
            for (int i = 0; i < RE - 1; i++) load_entries(__builtin_amdgcn_readlane(dcur, i), i);
#pragma unroll
            for (int i = 0; i < RR - 1; i++) gather_rows(i, i);
            auto stage = [&](unsigned t, auto S) -> bool {
                constexpr int s = decltype(S)::value;
                if (t >= n_t) return false;
                const unsigned n = __builtin_amdgcn_readlane(dcur, s) & 255u;
                float (*pb)[ROW] = prod[t & 1u][wave];
#pragma unroll
                for (int h = 0; h < NH; h++) {
                    const float wl = (unsigned)lane + 64u * h < n ? w[s][h] : 0.0f;
#pragma unroll
                    for (int c = 0; c < CC; c++) pb[c][lane + 64 * h] = wl * xr[s % RR][h][c];   // +0 past the chunk (rows are finite)
                }
                load_entries(__builtin_amdgcn_readlane(dcur, s + RE - 1), (s + RE - 1) % RE);
                gather_rows((s + RR - 1) % RE, (s + RR - 1) % RR);
                __syncthreads();
                return true;
            };
            for (unsigned t0 = 0;; t0 += RE) {
                dnxt = load_desc(t0 + RE);   // lanes 0 .. 2 RE - 2 of the next group's register
                if (!ring_stages(t0, stage, std::make_integer_sequence<int, RE>())) break;
                dcur = dnxt;
            }
        }
        __syncthreads();
    } else {
        const bool live = lane < G * CC;
        const int gi = live ? lane / CC : 0;
        const int c = live ? lane % CC : 0;
        const unsigned* I = R.tinfo + (size_t)frame * R.cap_tiles + tb;
        const unsigned short* V = R.tvl + (size_t)frame * 7 * R.cap_tiles + tb;
        // What a tile needs besides its products -- height and band (uniform) and the vertex of the lane's slot -- comes
        // from an LDS table of 2 x 64 tiles x 8 words {info, vertex of slot 0 .. 6}.  The adder refills it 64 tiles at a
        // time: lane = tile, eight global loads that stay in flight for 64 tiles and are stored when their half of the
        // table comes up.  Per tile that leaves two LDS reads, issued a tile ahead: the loop's critical path is the 64
        // dependent adds and the barrier, nothing else may wait on it (no load per tile, no register shuffling).
        unsigned pend[8];
        auto batch_load = [&](unsigned first) {
            const unsigned t = first + (unsigned)lane;
            const unsigned tc = n_t ? (t < n_t ? t : n_t - 1u) : 0u;
            pend[0] = n_t ? I[tc] : 0u;
#pragma unroll
            for (int i = 0; i < G; i++) pend[1 + i] = n_t ? (unsigned)V[(size_t)i * R.cap_tiles + tc] : n_own;
        };
        auto batch_store = [&](unsigned first) {
            const bool in = first + (unsigned)lane < n_t;
            unsigned* row = &ainfo[(first >> 6) & 1u][lane][0];
            // one word per slot: vertex | height << 10 | band << 18 (a lane reads ONE word per tile)
            const unsigned hb = ((pend[0] & 255u) << 10) | ((pend[0] >> 16) << 18);
#pragma unroll
            for (int i = 0; i < G; i++) row[i] = (in ? pend[1 + i] : n_own) | hb;
        };
        auto poll = [&]() -> unsigned { return __hip_atomic_load(&prog[(unsigned)lane < B ? lane : 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
        const unsigned tagv = tag << 16;
        if (lane == 0) __hip_atomic_store(&prog[j], n_t ? tagv : (tagv | 0xFFFFu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        batch_load(0u);
        batch_store(0u);
        batch_load(64u);
        unsigned polled = R.window >= 0 ? poll() : 0u;
        unsigned cur_vl = n_own, cur_band = 0u;
        bool pacing = R.window >= 0;
        float acc = 0.0f;
        unsigned w_n = n_own;
        // issues the table read of tile t (used after the next barrier)
        auto prep = [&](unsigned t) {
            if (t >= n_t) return;
            if ((t & 63u) == 0u && t) { batch_store(t); batch_load(t + 64u); }
            w_n = ainfo[(t >> 6) & 1u][t & 63u][gi];
        };
        auto pace = [&](unsigned band) {
            cur_band = band;
            if (lane == 0) __hip_atomic_store(&prog[j], tagv | band, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!pacing) return;
            auto behind = [&](unsigned pv) -> bool {
                // a word of another launch: that block has not started yet
                return (unsigned)lane < B && ((pv >> 16) != tag || (pv & 0xFFFFu) + (unsigned)R.window < band);
            };
            if (__ballot(behind(polled))) {
                const unsigned long long ts = R.trace ? __builtin_amdgcn_s_memrealtime() : 0ull;
                unsigned spins = 0;
                for (;;) {
                    polled = poll();
                    if (!__ballot(behind(polled))) break;
                    if (++spins > 256u) { pacing = false; break; }   // some block is not running: stop waiting for good
                    __builtin_amdgcn_s_sleep(8);
                }
                if (R.trace) t_spin += __builtin_amdgcn_s_memrealtime() - ts;
            }
            polled = poll();   // consumed at the next band
        };
        prep(0u);
        if (n_t) { const unsigned b0 = __builtin_amdgcn_readfirstlane(w_n) >> 18; if (b0 != cur_band) pace(b0); }
        __syncthreads();
        for (unsigned t = 0; t < n_t; t++) {
            const unsigned nmax = (__builtin_amdgcn_readfirstlane(w_n) >> 10) & 255u;
            const unsigned v_n = live ? (w_n & 1023u) : n_own;
            // the slot's vertex changed: park the sum, fetch the other one.  Store before load, one wave: a chain that
            // moved here from another slot of the previous tile is handed over in order.
            if (v_n != cur_vl) { accs[cur_vl * CC + c] = acc; acc = accs[v_n * CC + c]; cur_vl = v_n; }
            const float* pr = prod[t & 1u][gi][c];
            bool done = false;
            if constexpr (TH == 128) {
                if (nmax > 64u) {
                    float4 q[16], q2[16];
#pragma unroll
                    for (int i = 0; i < 16; i++) q[i] = reinterpret_cast<const float4*>(pr)[i];
#pragma unroll
                    for (int i = 0; i < 16; i++) q2[i] = reinterpret_cast<const float4*>(pr)[16 + i];
                    prep(t + 1u);
#pragma unroll
                    for (int i = 0; i < 16; i++) { acc += q[i].x; acc += q[i].y; acc += q[i].z; acc += q[i].w; }
#pragma unroll
                    for (int i = 0; i < 16; i++) { acc += q2[i].x; acc += q2[i].y; acc += q2[i].z; acc += q2[i].w; }
                    done = true;
                }
            }
            if (done) {
            } else if (nmax > 32u) {
                float4 q[16];
#pragma unroll
                for (int i = 0; i < 16; i++) q[i] = reinterpret_cast<const float4*>(pr)[i];
                prep(t + 1u);
#pragma unroll
                for (int i = 0; i < 16; i++) { acc += q[i].x; acc += q[i].y; acc += q[i].z; acc += q[i].w; }
            } else if (nmax > 16u) {
                float4 q[8];
#pragma unroll
                for (int i = 0; i < 8; i++) q[i] = reinterpret_cast<const float4*>(pr)[i];
                prep(t + 1u);
#pragma unroll
                for (int i = 0; i < 8; i++) { acc += q[i].x; acc += q[i].y; acc += q[i].z; acc += q[i].w; }
            } else {
                float4 q[4];
#pragma unroll
                for (int i = 0; i < 4; i++) q[i] = reinterpret_cast<const float4*>(pr)[i];
                prep(t + 1u);
#pragma unroll
                for (int i = 0; i < 4; i++) { acc += q[i].x; acc += q[i].y; acc += q[i].z; acc += q[i].w; }
            }
            if (t + 1u < n_t) { const unsigned bn = __builtin_amdgcn_readfirstlane(w_n) >> 18; if (bn != cur_band) pace(bn); }
            __syncthreads();
        }
        accs[cur_vl * CC + c] = acc;
        if (lane == 0) __hip_atomic_store(&prog[j], tagv | 0xFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (R.trace && lane == 0) {
            unsigned long long* tr = R.trace + ((size_t)frame * RES_MAXB + j) * 8;
            tr[0] = t_start; tr[1] = __builtin_amdgcn_s_memrealtime(); tr[2] = ((unsigned long long)n_own << 32) | n_t; tr[3] = t_spin;
            tr[4] = __builtin_amdgcn_s_memtime() - c_start;   // shader clocks
        }
    }
    __syncthreads();
    // every vertex of the frame belongs to one block: all sums are written, empty lists as 0
    const unsigned short* verts = R.blk_verts + ((size_t)frame * RES_MAXB + j) * RES_MAX_OWNV;
    for (unsigned e = threadIdx.x; e < n_own * CC; e += 512) values[((size_t)f0 + verts[e / CC]) * C + e % CC] = accs[e];
}

static std::atomic<unsigned> g_resident_tag{0};   // launch tags of the pacing words (any two concurrent launches just need different ones)

static size_t resident_lds_bytes(int CC, int TH) {
    return ((size_t)2 * 7 * CC * (TH + 4) + (size_t)(RES_MAX_OWNV + 1) * CC) * sizeof(float) + 2 * 64 * 8 * sizeof(unsigned);
}

// more than 64 KB of dynamic LDS has to be asked for, once per instantiation AND device (one process may drive
// several GPUs, one context each: rvseg_comm.cpp)
constexpr int RES_MAX_DEVICES = 64;
template <int CC, int TH>
static bool resident_setup() {
    static std::atomic<int> state[RES_MAX_DEVICES];   // 0 = not tried, 1 = ok, 2 = refused
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= RES_MAX_DEVICES) return false;
    int st = state[dev].load();
    if (st == 0) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(splat_resident_kernel<CC, 8, 4, TH>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)resident_lds_bytes(CC, TH));
        if (e != hipSuccess) (void)hipGetLastError();   // refused: the caller walks the lists the list-major way
        st = e == hipSuccess ? 1 : 2;
        state[dev].store(st);
    }
    return st == 1;
}

// blocks of the resident kernel that fit on the current device at once, and its CU count (cached per device)
static bool resident_device_info(int chunk, int* capacity, int* cus) {
    static std::atomic<int> cap[RES_MAX_DEVICES][2], ncu[RES_MAX_DEVICES];   // 0 = not known yet, -1 = failed
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= RES_MAX_DEVICES) return false;
    const int which = chunk == 128 ? 1 : 0;
    if (cap[dev][which].load() == 0) {
        int per_cu = 0;
        hipDeviceProp_t pr;
        hipError_t e = hipGetDeviceProperties(&pr, dev);
        if (e == hipSuccess) {
            if (which) e = resident_setup<9, 128>() ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, splat_resident_kernel<9, 8, 4, 128>, 512, resident_lds_bytes(9, 128)) : hipErrorUnknown;
            else e = resident_setup<9, 64>() ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, splat_resident_kernel<9, 8, 4, 64>, 512, resident_lds_bytes(9, 64)) : hipErrorUnknown;
        }
        if (e != hipSuccess) (void)hipGetLastError();
        ncu[dev].store(e == hipSuccess ? pr.multiProcessorCount : -1);
        cap[dev][which].store(e == hipSuccess && per_cu > 0 ? per_cu * pr.multiProcessorCount : -1);
    }
    const int c = cap[dev][which].load(), n = ncu[dev].load();
    if (capacity) *capacity = c > 0 ? c : 0;
    if (cus) *cus = n > 0 ? n : 0;
    return c > 0;
}

int resident_cu_count() { int n = 0; (void)resident_device_info(128, nullptr, &n); return n; }
int resident_block_capacity(int chunk) { int c = 0; (void)resident_device_info(chunk, &c, nullptr); return c; }

// false: the kernel could not be set up or launched (its dynamic LDS was refused): the caller walks the lists the
// list-major way
template <int CC>
static bool splat_resident_launch(const LatticeDev& L, const SplatResidentDev& R, const float* src, float* values, int slot, hipStream_t s) {
    const unsigned NG = (unsigned)L.n_groups;
    const unsigned rounds = ((unsigned)L.n_frames + NG - 1u) / NG;
    const unsigned tag = (g_resident_tag.fetch_add(1u) % 0x7FFFu) + 1u;
    const ValueView sv{const_cast<float*>(src), (size_t)L.N * (unsigned)CC, 0};
    const unsigned n_items = splat_walk_items(L, 7);   // should the planner have given up (splat_group_launch_g's grid)
    const dim3 grid(rounds * (unsigned)R.B * NG), block(512);
    if (R.chunk_log2 == 7) {
        if (!resident_setup<CC, 128>()) return false;
        splat_resident_kernel<CC, 8, 4, 128><<<grid, block, resident_lds_bytes(CC, 128), s>>>(L, R, sv, values, tag, slot, n_items);
    } else {
        if (!resident_setup<CC, 64>()) return false;
        splat_resident_kernel<CC, 8, 4, 64><<<grid, block, resident_lds_bytes(CC, 64), s>>>(L, R, sv, values, tag, slot, n_items);
    }
    return hipGetLastError() == hipSuccess;   // a refused launch is a refused set-up: fall back
}

bool launch_splat_resident(const LatticeDev& L, const SplatResidentDev& R, int C, const float* src, float* values, int slot, hipStream_t s) {
    return C == 9 ? splat_resident_launch<9>(L, R, src, values, slot, s) : splat_resident_launch<8>(L, R, src, values, slot, s);
}

}  // namespace rvseg
