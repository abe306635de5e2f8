// Permutohedral lattice build for gfx950: hash table, per-point simplex, compaction, blur neighbours, vertex-major CSR.
//
// Reference semantics (third-party/densecrf/src):
//   Permutohedral::init  SSE branch   permutohedral.cpp:140-321   (elevate, round-half-even,
//                                     rank, barycentric, d+1 vertex keys per point, blur neighbours)
//
// MI355X design notes
//   * One open-addressing hash table in HBM holds the lattice vertices of ALL frames of a chunk
//     (the frame index is an extra key coordinate), so every later kernel is a flat launch over
//     global vertex / point indices with no per-frame loop.
//   * Vertex numbering is whatever the atomics produce; no result depends on it.
//   * The splat (kernels_splat.hip) adds a vertex's contributions in ascending point order: the sort by vertex is STABLE.
#include <string.h>   // rocprim's texture iterator calls the host memset without including it

#include <type_traits>

#include <rocprim/rocprim.hpp>

#include "device_math.h"
#include "rvseg_crf.h"

namespace rvseg {

// ---------------------------------------------------------------------------------------------
// hash table
// ---------------------------------------------------------------------------------------------
constexpr int ST_EMPTY = -1, ST_LOCKED = -2, ST_FILLED = 0;

// d coordinates, then the frame index at k[7]; unused = 0.  A union so that the short / word /
// quad-word views alias legally (plain reinterpret_casts let the compiler drop the short stores).
struct Key8 {
    union {
        short k[8];
        unsigned w[4];
        unsigned long long q[2];
    };
};

__device__ __forceinline__ unsigned hash_key(const Key8& key) {
    unsigned h = 0x9E3779B9u;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        h ^= key.w[i];
        h *= 0x85EBCA6Bu;
        h ^= h >> 15;
    }
    return h;
}

__device__ __forceinline__ bool key_equal_at(const unsigned long long* tkeys, unsigned slot, const Key8& key) {
    const unsigned long long* mine = key.q;
    // agent-scope loads: another CU may have written the key after this CU cached the line
    const unsigned long long a = __hip_atomic_load(tkeys + 2 * (size_t)slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long b = __hip_atomic_load(tkeys + 2 * (size_t)slot + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return a == mine[0] && b == mine[1];
}

// The table is partitioned by frame: frame f owns slots [f*cap_f, (f+1)*cap_f).  Slot order is
// therefore frame-major, and the scan-based compaction below numbers a frame's vertices
// contiguously (the fused update kernel stages one frame's vertex values in LDS).
// find-or-create; returns the global slot.  On overflow sets counters[1] and returns the region base.
__device__ __forceinline__ unsigned hash_insert(int* state, unsigned long long* tkeys, unsigned base, unsigned mask,
                                                int* counters, const Key8& key) {
    unsigned hl = hash_key(key) & mask;
    for (unsigned probes = 0; probes <= mask; ) {
        const unsigned h = base + hl;
        int st = __hip_atomic_load(state + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (st == ST_EMPTY) {
            int expected = ST_EMPTY;
            if (__hip_atomic_compare_exchange_strong(state + h, &expected, ST_LOCKED, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                const unsigned long long* mine = key.q;
                __hip_atomic_store(tkeys + 2 * (size_t)h, mine[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(tkeys + 2 * (size_t)h + 1, mine[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(state + h, ST_FILLED, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                return h;
            }
            continue;  // lost the race: look at the same slot again
        }
        if (st == ST_LOCKED) continue;  // the owner publishes within its own loop iteration
        if (key_equal_at(tkeys, h, key)) return h;
        hl = (hl + 1) & mask;
        probes++;
    }
    counters[1] = 1;
    return base;
}

// read-only lookup (table complete, written by earlier kernels)
__device__ __forceinline__ int hash_lookup(const int* state, const unsigned long long* tkeys, unsigned base, unsigned mask,
                                           const Key8& key) {
    unsigned hl = hash_key(key) & mask;
    const unsigned long long* mine = key.q;
    for (unsigned probes = 0; probes <= mask; probes++) {
        const unsigned h = base + hl;
        if (state[h] == ST_EMPTY) return -1;
        if (tkeys[2 * (size_t)h] == mine[0] && tkeys[2 * (size_t)h + 1] == mine[1]) return (int)h;
        hl = (hl + 1) & mask;
    }
    return -1;
}

// ---------------------------------------------------------------------------------------------
// Permutohedral::init per point (SSE branch semantics, fp32, no contraction)
// ---------------------------------------------------------------------------------------------
constexpr int LP_SET = 512;        // block-local vertex set (LP_CHUNKS x 256 points x (d+1) keys, few distinct)
constexpr int LP_MAX_PROBE = 24;
constexpr int LP_CHUNKS = 8;       // consecutive 256-point chunks per block (at most): the set (and its global slots) carries over

// NARROW (LatticeDev::ids16, D == 6): the row holds the frame-local slots as uint16_t
template <int D, bool NARROW = false>
__global__ void __launch_bounds__(256)
lattice_points_kernel(LatticeDev L, FeatureSource fs, int n_chunks) {
    // block-local vertex set: tag (EMPTY / LOCKED / FILLED), key, global slot; `lnew` lists the set
    // entries in creation order, so each chunk resolves only the entries it added
    __shared__ int ltag[LP_SET];
    __shared__ unsigned long long lkey[LP_SET][2];
    __shared__ unsigned lslot[LP_SET];
    __shared__ unsigned short lnew[LP_SET];
    __shared__ unsigned n_new;
    for (int t = threadIdx.x; t < LP_SET; t += 256) ltag[t] = ST_EMPTY;
    if (threadIdx.x == 0) n_new = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned resolved = 0;   // set entries [0, resolved) of lnew already have their global slot
    const long long per_frame = L.Npad;

  for (int chunk = 0; chunk < n_chunks; chunk++) {
    const long long gid0 = ((long long)blockIdx.x * n_chunks + chunk) * 256 + threadIdx.x;
    const bool active = gid0 < per_frame * L.n_frames;   // all threads stay for the barriers
    const long long gid = active ? gid0 : 0;
    const int frame = (int)(gid / per_frame);
    const int i = (int)(gid - (long long)frame * per_frame);
    const bool real = active && i < L.N;
    const long long gp = (long long)frame * L.N + i;  // global point index (valid when real)

    float f[D];
    if (!real) {
#pragma unroll
        for (int k = 0; k < D; k++) f[k] = 0.0f;  // padded lanes carry zero features (permutohedral.cpp:196)
    } else if (fs.mode == 0) {
#pragma unroll
        for (int k = 0; k < D; k++) f[k] = fs.feat[gp * D + k];
    } else {
        // frame mode (D == 6): segmenter.cpp:629-637 on the frame's own points
        const float4 c = fs.cloud[gp];
        float x = c.x, y = c.y, z = c.z;
        if (!(finite_f(x) && finite_f(y) && finite_f(z))) x = y = z = 0.0f;
        const uint8_t* px = fs.rgb + gp * 3;
        const float v[6] = {x * fs.xyz_kernel, y * fs.xyz_kernel, z * fs.xyz_kernel,
                            ((float)px[0] / 255.0f) * fs.rgb_kernel, ((float)px[1] / 255.0f) * fs.rgb_kernel,
                            ((float)px[2] / 255.0f) * fs.rgb_kernel};
#pragma unroll
        for (int k = 0; k < D; k++) f[k] = v[k < 6 ? k : 0];
    }

    const float invdplus1 = 1.0f / (D + 1), dplus1 = (float)(D + 1);
    float el[D + 1], rem0[D + 1], rank[D + 1];
    // elevate (permutohedral.cpp:201-207)
    float sm = 0.0f;
#pragma unroll
    for (int j = D; j > 0; j--) {
        const float cf = f[j - 1] * L.scale[j - 1];
        el[j] = sm - (float)j * cf;
        sm += cf;
    }
    el[0] = sm;
    // closest 0-coloured simplex (:210-220), cvtps_epi32 = round half to even
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k <= D; k++) {
        float v = invdplus1 * el[k];
        v = rintf(v);
        rem0[k] = v * dplus1;
        sum += v;
    }
    // rank (:223-233)
#pragma unroll
    for (int k = 0; k <= D; k++) rank[k] = 0.0f;
#pragma unroll
    for (int a = 0; a < D; a++) {
        const float di = el[a] - rem0[a];
#pragma unroll
        for (int b = a + 1; b <= D; b++) {
            const float dj = el[b] - rem0[b];
            const float c = di < dj ? 1.0f : 0.0f;
            rank[a] += c;
            rank[b] += 1.0f - c;
        }
    }
    // back onto the plane (:236-242)
#pragma unroll
    for (int k = 0; k <= D; k++) {
        rank[k] += sum;
        const float add = rank[k] < 0.0f ? dplus1 : 0.0f;
        const float sub = rank[k] >= dplus1 ? dplus1 : 0.0f;
        rank[k] += add - sub;
        rem0[k] += add - sub;
    }
    // barycentric (:245-263); the scatter index D - rank is data dependent, so walk it with
    // compile-time indices to keep the array in registers
    float bary[D + 2];
#pragma unroll
    for (int k = 0; k < D + 2; k++) bary[k] = 0.0f;
#pragma unroll
    for (int k = 0; k <= D; k++) {
        const float v = (el[k] - rem0[k]) * invdplus1;
        const int p = D - (int)rank[k];
#pragma unroll
        for (int q = 0; q <= D; q++) {
            if (q == p) { bary[q] += v; bary[q + 1] -= v; }
        }
    }
    bary[0] += 1.0f + bary[D + 1];
    // vertices (:266-275).  Neighbouring points share almost all their vertices, so the block first
    // collects its distinct keys in an LDS set (phase 1), then one lane per distinct key does the
    // global find-or-create -- all global round trips of a block overlap (phase 2) -- and finally
    // every point reads the global slots of its d+1 vertices back from LDS (phase 3).
    int lidx[D + 1];   // index into the LDS set, or -1 - (global slot) when the set was too full
#pragma unroll
    for (int r = 0; r <= D; r++) {
        Key8 key;
#pragma unroll
        for (int k = 0; k < 8; k++) key.k[k] = 0;
#pragma unroll
        for (int k = 0; k < D; k++) {
            const int rk = (int)rank[k];
            const int canon = rk <= D - r ? r : r - (D + 1);
            key.k[k] = (short)(rem0[k] + (float)canon);
        }
        key.k[7] = (short)frame;
        // equal keys inside the wave first (neighbouring points share most vertices): one lane per
        // distinct key goes to the LDS set, the others take its answer
        int leader_of = lane;
        {
            bool pending = active;
            for (;;) {
                const unsigned long long todo = __ballot(pending);
                if (!todo) break;
                const int ld = __ffsll((long long)todo) - 1;
                const unsigned a0 = __builtin_amdgcn_readlane(key.w[0], ld), a1 = __builtin_amdgcn_readlane(key.w[1], ld);
                const unsigned a2 = __builtin_amdgcn_readlane(key.w[2], ld), a3 = __builtin_amdgcn_readlane(key.w[3], ld);
                const bool same = pending && key.w[0] == a0 && key.w[1] == a1 && key.w[2] == a2 && key.w[3] == a3;
                if (same) leader_of = ld;
                pending = pending && !same;
            }
        }
        int found = 0;
        if (active && leader_of == lane) {
            unsigned h = (hash_key(key) >> 7) & (LP_SET - 1);
            found = -1;
            for (int probes = 0; probes < LP_MAX_PROBE; ) {
                const int t = __hip_atomic_load(&ltag[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (t == ST_EMPTY) {
                    int expected = ST_EMPTY;
                    if (__hip_atomic_compare_exchange_strong(&ltag[h], &expected, ST_LOCKED, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_WORKGROUP)) {
                        __hip_atomic_store(&lkey[h][0], key.q[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_store(&lkey[h][1], key.q[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_store(&ltag[h], ST_FILLED, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                        lnew[atomicAdd(&n_new, 1u)] = (unsigned short)h;   // at most LP_SET entries are ever created
                        found = (int)h;
                        break;
                    }
                    continue;
                }
                if (t == ST_LOCKED) continue;
                const unsigned long long a = __hip_atomic_load(&lkey[h][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const unsigned long long b = __hip_atomic_load(&lkey[h][1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (a == key.q[0] && b == key.q[1]) { found = (int)h; break; }
                h = (h + 1) & (LP_SET - 1);
                probes++;
            }
            if (found < 0)  // set too crowded around this key: go to the global table directly
                found = -1 - (int)hash_insert(L.state, L.tkeys, (unsigned)frame << L.cap_f_log2, L.cap_f_mask, L.counters, key);
        }
        lidx[r] = __shfl(found, leader_of, 64);
    }
    __syncthreads();
    const unsigned created = n_new;   // stable until the next chunk's phase 1, which starts after the barrier below
    for (unsigned t = resolved + threadIdx.x; t < created; t += 256) {
        const unsigned h = lnew[t];
        Key8 key;
        key.q[0] = lkey[h][0];
        key.q[1] = lkey[h][1];
        const unsigned fr = (unsigned)(unsigned short)key.k[7];
        lslot[h] = hash_insert(L.state, L.tkeys, fr << L.cap_f_log2, L.cap_f_mask, L.counters, key);
    }
    resolved = created;
    __syncthreads();
    if (real) {
        int so[D + 1];
#pragma unroll
        for (int r = 0; r <= D; r++) {
            const int li = lidx[r];
            so[r] = li >= 0 ? (int)lslot[li] : -1 - li;
            if (NARROW) so[r] &= (int)L.cap_f_mask;   // slot = frame * cap_f + h
        }
        if constexpr (NARROW) store_ids16(L.offsets, (size_t)gp, so);
        else store_row<D + 1>(L.offsets + gp * (D + 1), so);
        store_row<D + 1>(L.bary + gp * (D + 1), bary);
    }
  }
}

void launch_lattice_points(const LatticeDev& L, const FeatureSource& fs, hipStream_t s) {
    const long long total = (long long)L.Npad * L.n_frames;
    // chunks per block: as many as leave >= 1024 blocks (a single frame or a cloud is a latency case: 150 blocks of
    // 8 chunks kept three quarters of the chip idle for 106 us)
    int n_chunks = LP_CHUNKS;
    while (n_chunks > 1 && (total + 255) / 256 / n_chunks < 1024) n_chunks >>= 1;
    const long long per_block = 256ll * n_chunks;
    const dim3 grid((unsigned)((total + per_block - 1) / per_block)), block(256);
    with_dimension(L.d, [&](auto dim) {
        constexpr int D = decltype(dim)::value;
        if constexpr (D == 6) {   // the only dimension with a 16-bit form
            if (L.ids16) { lattice_points_kernel<6, true><<<grid, block, 0, s>>>(L, fs, n_chunks); return; }
        }
        lattice_points_kernel<D><<<grid, block, 0, s>>>(L, fs, n_chunks);
    });
    RV_LAUNCHED("lattice_points_kernel");
}

// ---------------------------------------------------------------------------------------------
// compaction: an exclusive scan over the slot occupancy numbers the vertices in slot order, i.e.
// deterministically and frame by frame
// ---------------------------------------------------------------------------------------------
struct SlotFilled {
    __device__ __forceinline__ int operator()(int st) const { return st == ST_FILLED ? 1 : 0; }
};

__global__ void __launch_bounds__(256)
lattice_compact_kernel(LatticeDev L) {
    const unsigned slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= L.cap_total) return;
    const bool filled = L.state[slot] == ST_FILLED;
    const int id = L.slot_to_id[slot];
    if (filled && (unsigned)id < (unsigned)L.m_bound) {
        L.vkeys[2 * (size_t)id] = L.tkeys[2 * (size_t)slot];
        L.vkeys[2 * (size_t)id + 1] = L.tkeys[2 * (size_t)slot + 1];
    }
    const unsigned cap_f = L.cap_f_mask + 1;
    if ((slot & L.cap_f_mask) == 0) L.fstart[slot >> L.cap_f_log2] = id;   // first vertex id of the frame
    if (slot == L.cap_total - 1) {
        const int M = id + (filled ? 1 : 0);
        L.counters[0] = M;
        L.fstart[L.n_frames] = M;
        if (M > L.m_bound) L.counters[1] = 1;
    }
    // load factor above 1/2 in a frame's region counts as overflow (checked at the region's last slot)
    if ((slot & L.cap_f_mask) == L.cap_f_mask) {
        const int first = L.slot_to_id[slot - L.cap_f_mask];
        const int Mf = id + (filled ? 1 : 0) - first;
        if ((unsigned)Mf > cap_f / 2) L.counters[1] = 1;
    }
}

// offsets: slot -> vertex id; sort keys / payloads for the stable vertex-major ordering
__global__ void __launch_bounds__(256)
lattice_remap_kernel(LatticeDev L, unsigned* __restrict__ sort_keys, unsigned* __restrict__ sort_vals, long long n_entries) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) return;
    int id = L.slot_to_id[L.offsets[e]];
    id = id < L.m_bound ? id : L.m_bound - 1;   // only after a (flagged) hash overflow
    L.offsets[e] = id;
    sort_keys[e] = (unsigned)id;
    sort_vals[e] = (unsigned)e;
}

// blur neighbours (permutohedral.cpp:296-318).  For axis j == d the +-d write of the reference
// lands on the coordinate that the d-length key ignores.
__global__ void __launch_bounds__(256)
lattice_neighbours_kernel(LatticeDev L) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int M = L.counters[0] < L.m_bound ? L.counters[0] : L.m_bound;
    const int d = L.d;
    if (gid >= (long long)M * (d + 1)) return;
    const int j = (int)(gid / M);
    const int id = (int)(gid - (long long)j * M);
    Key8 key;
    const unsigned long long* src = L.vkeys + 2 * (size_t)id;
    key.q[0] = src[0];
    key.q[1] = src[1];
    Key8 n1 = key, n2 = key;
    for (int k = 0; k < d; k++) { n1.k[k] = (short)(key.k[k] - 1); n2.k[k] = (short)(key.k[k] + 1); }
    if (j < d) { n1.k[j] = (short)(key.k[j] + d); n2.k[j] = (short)(key.k[j] - d); }
    const unsigned fbase = (unsigned)(unsigned short)key.k[7] << L.cap_f_log2;
    const int s1 = hash_lookup(L.state, L.tkeys, fbase, L.cap_f_mask, n1);
    const int s2 = hash_lookup(L.state, L.tkeys, fbase, L.cap_f_mask, n2);
    L.nb1[(size_t)j * L.m_bound + id] = s1 < 0 ? -1 : L.slot_to_id[s1];
    L.nb2[(size_t)j * L.m_bound + id] = s2 < 0 ? -1 : L.slot_to_id[s2];
}

// CSR over the sorted entries: point index, barycentric weight, per-vertex [start, end)
__global__ void __launch_bounds__(256)
lattice_csr_kernel(LatticeDev L, const unsigned* __restrict__ keys_sorted, const unsigned* __restrict__ vals_sorted,
                   long long n_entries) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_entries) return;
    const unsigned e = vals_sorted[k];
    const unsigned key = keys_sorted[k];
    L.csr_pw[k] = make_uint2(e / (unsigned)(L.d + 1), __float_as_uint(L.bary[e]));
    if (k == 0 || keys_sorted[k - 1] != key) L.vstart[key] = (unsigned)k;
    if (k == n_entries - 1 || keys_sorted[k + 1] != key) L.vend[key] = (unsigned)(k + 1);
}

void launch_vertex_order(const LatticeDev& L, SortBuffers& sb, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Vertex-major ordering by a counting sort (fast path, used when a frame has at most CS_MCAP
// vertices -- the Segmenter kernel has ~300).  The entries of a frame are cut into wave-blocks of
// cs_pix points, one wave each; the scatter walks its block in order, 64 points at a time, and ranks
// equal vertex ids inside the chunk with ballots, so the order inside a vertex stays ascending in
// the point index without any comparison sort:
//   pass 1 (count)   per wave-block histogram over the frame's vertices (LDS) + slot -> id remap
//   scan             per frame: vertex start offsets and per-(wave-block, vertex) bases
//   pass 2 (scatter) entries land at base + rank
// ---------------------------------------------------------------------------------------------
constexpr int CS_PIX_MIN = 256;   // points per wave-block (LatticeDev::cs_pix): 256 .. 4096, a power of two
constexpr int CS_MCAP = 4096;   // 4 waves x 4096 counters = 64 KB of LDS at the largest fast-path capacity (2^13 slots per frame)

// Launch shape of the count and scatter passes: one wave per wave-block, four to a block, each with a row of mcap
// counters in LDS (mcap = the vertices a frame can have at this capacity).  The device side is CsWaveBlock.
struct CsLaunch {
    int mcap, wbpf;   // wbpf: wave-blocks per frame
    dim3 grid, block;
    size_t lds;
};
static CsLaunch cs_launch(const LatticeDev& L) {
    CsLaunch c;
    c.mcap = (int)((L.cap_f_mask + 1) / 2);
    c.wbpf = (L.N + L.cs_pix - 1) / L.cs_pix;
    c.grid = dim3((unsigned)(((long long)c.wbpf * L.n_frames + 3) / 4));
    c.block = dim3(256);
    c.lds = (size_t)4 * c.mcap * sizeof(unsigned);
    return c;
}

// {first vertex id f0, vertex count Mf} of a frame as the counting sort sees them (the clamps only matter after a
// flagged hash overflow; they keep every access in bounds)
__device__ __forceinline__ int2 cs_frame_vertices(const LatticeDev& L, int frame, int mcap) {
    const int2 fr = lattice_frame_range(L, frame, L.m_bound);
    return make_int2(fr.x, fr.y - fr.x < mcap ? fr.y - fr.x : mcap);
}

// What a wave of the count / scatter pass works on.  bh holds, per frame, a dense [wave-block][vertex] matrix with row
// stride Mf; the frame's matrix starts at wbpf * fstart[frame] (so the whole array needs wbpf * M_total words).
struct CsWaveBlock {
    bool outside;           // past the last frame (the grid is rounded up to 4 waves): the whole wave leaves
    int lane, frame, wb;
    int f0, Mf;             // the frame's first vertex id and its vertices
    long long p0, p1;       // the wave-block's points [p0, p1) of the frame ...
    long long ebeg, eend;   // ... and their entries, counted over all frames
    unsigned* my;           // this wave's counters in LDS: [Mf]
    size_t row;             // this wave-block's row of bh: bh[row + vertex]
};
__device__ __forceinline__ CsWaveBlock cs_wave_block(const LatticeDev& L, int wbpf, int mcap) {
    extern __shared__ unsigned cs_cnt[];   // [4 waves][mcap]
    CsWaveBlock B{};
    const int wave = threadIdx.x >> 6;
    const long long gwb = (long long)blockIdx.x * 4 + wave;
    B.lane = threadIdx.x & 63;
    B.frame = (int)(gwb / wbpf);
    B.outside = B.frame >= L.n_frames;
    if (B.outside) return B;
    B.wb = (int)(gwb - (long long)B.frame * wbpf);
    const int2 fv = cs_frame_vertices(L, B.frame, mcap);
    B.f0 = fv.x;
    B.Mf = fv.y;
    B.p0 = (long long)B.wb * L.cs_pix;
    B.p1 = B.p0 + L.cs_pix < L.N ? B.p0 + L.cs_pix : L.N;
    B.ebeg = ((long long)B.frame * L.N + B.p0) * (L.d + 1);
    B.eend = ((long long)B.frame * L.N + B.p1) * (L.d + 1);
    B.my = cs_cnt + (size_t)wave * mcap;
    B.row = (size_t)wbpf * B.f0 + (size_t)B.wb * B.Mf;
    return B;
}

// a unit of the count pass: W consecutive ids in one 16-byte access
__device__ __forceinline__ void load_unit(const int* p, int (&v)[4]) { load_row<4>(p, v); }
__device__ __forceinline__ void store_unit(int* p, const int (&v)[4]) { store_row<4>(p, v); }
__device__ __forceinline__ void load_unit(const u16_ids* p, int (&v)[8]) {
    const u16x8_ids t = *reinterpret_cast<const u16x8_ids*>(p);
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = t[k];
}
__device__ __forceinline__ void store_unit(u16_ids* p, const int (&v)[8]) {
    u16x8_ids t;
#pragma unroll
    for (int k = 0; k < 8; k++) t[k] = (unsigned short)v[k];
    *reinterpret_cast<u16x8_ids*>(p) = t;
}

// Count pass, a unit of W entries per lane and step.  Walking a wave-block one entry per lane means two DEPENDENT loads
// per step (slot, then slot -> vertex id): PMC showed such waves waiting 91 % of their cycles.  Counting needs no order, so
// a lane takes W consecutive entries at once -- one 16-byte load, W id gathers in flight together, one 16-byte store of the
// remapped ids -- and adds into the counters with LDS atomics (same-address lanes serialise in hardware, still an order
// of magnitude cheaper than ranking with ballots).
//   32-bit global ids: W = 4, units start at the wave-block's first entry (4-byte aligned accesses).
//   NARROW (LatticeDev::ids16), 16-bit frame-local values: W = 8, and a wave-block walks the ALIGNED 16-byte units that
//   hold its entries, although a frame's first entry (frame * N * (d+1)) need not be a multiple of eight.  The slot -> id
//   gather adds the frame's region base, and the stored id is local to the frame's id range, clamped like the counter index.
// A unit that lies wholly inside the wave-block is one wide load and one wide store; the others -- the tail, and with
// NARROW the unit shared with the neighbouring frame (a wave-block has a multiple of 256 points, so only there) -- are
// read and written element by element, each wave its own entries.
template <bool NARROW>
__global__ void __launch_bounds__(256)
csr_count_kernel(LatticeDev L, unsigned* __restrict__ bh, int wbpf, int mcap) {
    constexpr int W = NARROW ? 8 : 4;
    typedef typename std::conditional<NARROW, u16_ids, int>::type id_t;
    const CsWaveBlock B = cs_wave_block(L, wbpf, mcap);
    if (B.outside) return;   // no block-wide barrier below
    const int lane = B.lane, f0 = B.f0, Mf = B.Mf;
    const long long ebeg = B.ebeg, eend = B.eend;
    unsigned* my = B.my;
    for (int lv = lane; lv < Mf; lv += 64) my[lv] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const long long ubeg = NARROW ? ebeg & ~7ll : ebeg;   // first unit; every unit [e, e + W) below has e + W > ebeg
    id_t* ids = reinterpret_cast<id_t*>(L.offsets);
    const int* s2i = L.slot_to_id + (NARROW ? (size_t)B.frame << L.cap_f_log2 : (size_t)0);   // NARROW: a slot is below cap_f
    auto mine = [&](long long e) { return (!NARROW || e >= ebeg) && e < eend; };          // entry e is this wave-block's
    auto whole = [&](long long e) { return (!NARROW || e >= ebeg) && e + W <= eend; };    // and so is all of unit e
    auto fetch = [&](long long e, int (&sl)[W]) {   // slots of the unit at e; 0 outside the wave-block
        if (whole(e)) {
            load_unit(ids + e, sl);
        } else {
#pragma unroll
            for (int k = 0; k < W; k++) sl[k] = mine(e + k) ? (int)ids[e + k] : 0;
        }
    };
    int sl_n[W];
    fetch(ubeg + W * lane < eend ? ubeg + W * lane : ubeg, sl_n);
    for (long long base = ubeg; base < eend; base += 64 * W) {
        const long long e = base + W * lane;
        int sl[W], id[W], lv[W];
#pragma unroll
        for (int k = 0; k < W; k++) sl[k] = sl_n[k];
        const bool any = e < eend;
        if (any) {
#pragma unroll
            for (int k = 0; k < W; k++) id[k] = s2i[sl[k]];   // W gathers in flight
        }
        const long long en = e + 64 * W;
        fetch(en < eend ? en : ubeg, sl_n);                    // the next step's slots travel meanwhile
        if (!any) continue;
#pragma unroll
        for (int k = 0; k < W; k++) {
            // ids beyond the per-vertex arrays only occur after a (flagged) hash overflow: clamp so that every later
            // kernel stays in bounds; the host discards the result
            id[k] = id[k] < L.m_bound ? id[k] : L.m_bound - 1;
            lv[k] = id[k] - f0;
            lv[k] = lv[k] < Mf ? lv[k] : Mf - 1;
            lv[k] = lv[k] < 0 ? 0 : lv[k];
        }
        const int (&out)[W] = NARROW ? lv : id;                // slot -> vertex id, in place
        if (whole(e)) {
            store_unit(ids + e, out);
        } else {
#pragma unroll
            for (int k = 0; k < W; k++) if (mine(e + k)) ids[e + k] = (id_t)out[k];
        }
#pragma unroll
        for (int k = 0; k < W; k++) {
            if (mine(e + k) && Mf > 0) atomicAdd(&my[lv[k]], 1u);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    unsigned* row = bh + B.row;
    for (int lv = lane; lv < Mf; lv += 64) row[lv] = my[lv];
}

// Scatter pass with one lane per POINT.  A chunk is 64 consecutive points x DP1 entries.  For every distinct vertex k
// of the chunk the lanes that hold k -- in any of their DP1 slots, at most one per lane since a point's vertices are
// distinct -- are found with DP1 ballots; their union, masked to the lower lanes, is the rank of a point among the
// chunk's entries of k, i.e. ascending point order again.  Neighbouring points share their simplex, so a chunk has
// ~12-20 distinct vertices for 448 entries.  (One lane per ENTRY ranks ~10 distinct vertices per 64 entries; PMC: 438
// vector instructions per 64 entries.)
// Ranks and totals depend on the chunk's ids alone, not on the counters, so a chunk is done in two steps:
//   rank     the loop over the distinct vertices leaves, per slot j of a lane, the rank of its entry (bits 0-7 of rt[j])
//            and, in the slot with which the lane led its vertex, the vertex's total in the chunk (bits 8-15; 1 .. 64,
//            0 elsewhere).  Ballots and registers only: neither LDS nor global memory is on this serial path.
//   place    DP1 independent LDS reads of the counters my[lv[j]], DP1 stores at counter + rank, then every leader adds
//            its total to its counter.  A vertex has exactly one leader per chunk, so no two lanes write one counter.
// The LDS reads of a wave are issued before its LDS writes and the wave fence at the end of a chunk orders those writes
// before the next chunk's reads.  The ids and weights of chunk c + 1 are loaded before chunk c is ranked, so a wave
// waits for one memory round trip per wave-block, not per chunk; lanes past the wave-block's last point, and every lane
// behind the last chunk, load the last point again (in bounds, unused).
// NARROW (LatticeDev::ids16, DP1 == 7): the rows hold frame-local ids as uint16_t.
template <int DP1, bool NARROW = false>
__global__ void __launch_bounds__(256)
csr_scatter_kernel(LatticeDev L, const unsigned* __restrict__ bh, int wbpf, int mcap) {
    constexpr int RW = NARROW ? 4 : DP1;   // dwords of a row of ids as loaded
    const CsWaveBlock B = cs_wave_block(L, wbpf, mcap);
    if (B.outside) return;   // no block-wide barrier below
    const int lane = B.lane, frame = B.frame, f0 = B.f0, Mf = B.Mf;
    const unsigned n_entries_total = (unsigned)((long long)L.n_frames * L.N * DP1);
    unsigned* my = B.my;
    const unsigned* row = bh + B.row;
    for (int lv = lane; lv < Mf; lv += 64) my[lv] = row[lv];
    if (Mf == 0 && lane == 0) my[0] = 0xFFFFFFFFu;   // no vertices (overflow only): positions fail the bound check
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const int p0 = (int)B.p0, p1 = (int)B.p1;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    auto point = [&](int pc) {   // this lane's point of the chunk at pc, clamped to the wave-block's last
        const int p = pc + lane;
        return (unsigned)frame * (unsigned)L.N + (unsigned)(p < p1 ? p : p1 - 1);   // below n_frames * N, like the entries' unsigned positions
    };
    auto fetch = [&](size_t gp, unsigned (&raw)[RW], float (&w)[DP1]) {
        if constexpr (NARROW) load_ids16(L.offsets, gp, raw);
        else load_row<DP1>(reinterpret_cast<const unsigned*>(L.offsets) + gp * DP1, raw);
        load_row<DP1>(L.bary + gp * DP1, w);
    };
    unsigned raw_n[RW];
    float w_n[DP1];
    unsigned gp_n = point(p0);
    fetch(gp_n, raw_n, w_n);
    for (int pc = p0; pc < p1; pc += 64) {
        const bool valid = pc + lane < p1;
        const unsigned gp = gp_n;
        int lv[DP1];
        float w[DP1];
        if constexpr (NARROW) {
            unpack_ids16(raw_n, gp, lv);
        } else {
#pragma unroll
            for (int j = 0; j < DP1; j++) lv[j] = (int)raw_n[j];
        }
#pragma unroll
        for (int j = 0; j < DP1; j++) w[j] = w_n[j];
        gp_n = point(pc + 64);
        fetch(gp_n, raw_n, w_n);   // the next chunk travels while this one is ranked
#pragma unroll
        for (int j = 0; j < DP1; j++) {
            if (!NARROW) lv[j] -= f0;
            lv[j] = lv[j] < Mf ? lv[j] : Mf - 1;   // overflow case (flagged elsewhere): stay in bounds
            lv[j] = lv[j] < 0 ? 0 : lv[j];
        }
        unsigned rt[DP1];
#pragma unroll
        for (int j = 0; j < DP1; j++) rt[j] = 0u;
        unsigned pend = valid ? (1u << DP1) - 1u : 0u;
#pragma unroll
        for (int j = 0; j < DP1; j++) {
            for (;;) {
                const unsigned long long todo = __ballot((pend >> j) & 1u);
                if (!todo) break;
                const int leader = __ffsll((long long)todo) - 1;
                const int k = __builtin_amdgcn_readlane(lv[j], leader);
                // slots below j are already empty for every lane; a vertex handled in an earlier pass
                // was removed from all slots then, so it cannot come up again in this chunk
                unsigned long long all = 0ull;
                unsigned hit = 0u;
#pragma unroll
                for (int jj = j; jj < DP1; jj++) {
                    const bool same = ((pend >> jj) & 1u) && lv[jj] == k;
                    all |= __ballot(same);
                    if (same) hit |= 1u << jj;
                }
                const unsigned r = (unsigned)__popcll(all & lt);
#pragma unroll
                for (int jj = j; jj < DP1; jj++) {
                    if ((hit >> jj) & 1u) rt[jj] = r;
                }
                pend &= ~hit;
                if (lane == leader) rt[j] |= (unsigned)__popcll(all) << 8;
            }
        }
        unsigned base[DP1];
#pragma unroll
        for (int j = 0; j < DP1; j++) base[j] = my[lv[j]];
        if (valid) {
#pragma unroll
            for (int j = 0; j < DP1; j++) {
                const unsigned pos = base[j] + (rt[j] & 0xFFu);
                if (pos < n_entries_total) L.csr_pw[pos] = make_uint2(gp, __float_as_uint(w[j]));
            }
        }
#pragma unroll
        for (int j = 0; j < DP1; j++) {
            const unsigned total = rt[j] >> 8;
            if (total) my[lv[j]] = base[j] + total;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
}

// Scatter pass with one lane per ENTRY, for d = 1, 3, 4 and 7 (clouds only, 32-bit ids): csr_scatter_kernel is
// instantiated for d = 2, 5 and 6 alone, and nobody has timed it against this kernel at the other dimensions.  A wave
// walks its block 64 entries at a time and ranks equal vertex ids inside the chunk with ballots, so the order inside a
// vertex is ascending in the point index here too.
__global__ void __launch_bounds__(256)
csr_scatter_entries_kernel(LatticeDev L, const unsigned* __restrict__ bh, int wbpf, int mcap) {
    const CsWaveBlock B = cs_wave_block(L, wbpf, mcap);
    if (B.outside) return;   // no block-wide barrier below
    const int lane = B.lane, f0 = B.f0, Mf = B.Mf, dp1 = L.d + 1;
    const long long ebeg = B.ebeg, eend = B.eend;
    const unsigned n_entries_total = (unsigned)((long long)L.n_frames * L.N * dp1);
    unsigned* my = B.my;
    const unsigned* row = bh + B.row;
    for (int lv = lane; lv < Mf; lv += 64) my[lv] = row[lv];
    if (Mf == 0 && lane == 0) my[0] = 0xFFFFFFFFu;   // no vertices (overflow only): positions fail the bound check
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    // software pipeline: the next chunk's loads are in flight while the current chunk is ranked
    auto fetch = [&](long long e, int& id, float& wgt) {
        id = 0; wgt = 0.f;
        if (e < eend) { id = L.offsets[e]; wgt = L.bary[e]; }
    };
    int id_n; float w_n;
    fetch(ebeg + lane, id_n, w_n);
    for (long long base = ebeg; base < eend; base += 64) {
        const long long e = base + lane;
        const bool valid = e < eend;
        const int id = id_n;
        const float wgt = w_n;
        fetch(e + 64, id_n, w_n);
        int lv = valid ? id - f0 : -1;
        if (lv >= Mf) lv = Mf - 1;                   // overflow case (flagged elsewhere): stay in bounds
        if (valid && lv < 0) lv = 0;
        bool pending = valid;
        // distinct vertex ids of a chunk touch distinct counters, so the loop needs no ordering
        // inside a chunk; one fence per chunk orders the counters between chunks
        for (;;) {
            const unsigned long long todo = __ballot(pending);
            if (!todo) break;
            const int leader = __ffsll((long long)todo) - 1;
            const int k = __shfl(lv, leader, 64);
            const bool same = pending && lv == k;
            const unsigned long long m = __ballot(same);
            const unsigned b = my[k];
            if (same) {
                const unsigned pos = b + (unsigned)__popcll(m & lt);
                if (pos < n_entries_total) L.csr_pw[pos] = make_uint2((unsigned)(e / dp1), __float_as_uint(wgt));   // one 8-byte store
            }
            if (lane == leader) my[k] = b + (unsigned)__popcll(m);
            pending = pending && !same;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
}

// per frame: bh[wb][lv] (counts) -> absolute base of (wave-block, vertex) in the csr arrays; vstart / vend per vertex.
// Two launches over (frame, group of 64 vertices) blocks of 1024 threads = 16 wave-block segments x 64 vertices: the
// first adds up the columns (per segment and whole), the second turns them into running bases.  The only thing a group
// needs from the others is the number of entries of the vertices before it, which it adds up itself from the column
// totals -- so the groups of a frame run side by side.  (Until round 3 one block per frame walked its groups one after
// the other: 139 us for a single 640x480 frame, 461 us for a 1.1 M-point cloud, on the critical path of both.)
constexpr int CS_SEGS = 16;
__device__ __forceinline__ size_t csr_aux_offset(const LatticeDev& L, int wbpf) { return (size_t)wbpf * ((size_t)L.m_bound + 64); }

__global__ void __launch_bounds__(1024)
csr_total_kernel(LatticeDev L, unsigned* __restrict__ bh, int wbpf, int mcap, int n_groups) {
    __shared__ unsigned sseg[CS_SEGS][64];
    const int frame = blockIdx.x / n_groups, grp = blockIdx.x - frame * n_groups;
    const int2 fv = cs_frame_vertices(L, frame, mcap);
    const int f0 = fv.x, Mf = fv.y;
    const int lv0 = grp * 64;
    if (lv0 >= Mf) return;                   // whole block
    const int lvl = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int sw = (wbpf + CS_SEGS - 1) / CS_SEGS;
    const int w0 = seg * sw, w1 = (w0 + sw < wbpf) ? w0 + sw : wbpf;
    const unsigned* fb = bh + (size_t)wbpf * f0;   // dense [wave-block][vertex] matrix, row stride Mf
    unsigned* vtot = bh + csr_aux_offset(L, wbpf);
    unsigned* segsum = vtot + L.m_bound;
    const int lv = lv0 + lvl;
    const bool ok = lv < Mf;
    unsigned sum = 0;
    if (ok) for (int w = w0; w < w1; w++) sum += fb[(size_t)w * Mf + lv];
    sseg[seg][lvl] = sum;
    if (ok) segsum[(size_t)(f0 + lv) * CS_SEGS + seg] = sum;
    __syncthreads();
    if (seg == 0 && ok) {
        unsigned total = 0;
#pragma unroll
        for (int q = 0; q < CS_SEGS; q++) total += sseg[q][lvl];
        vtot[f0 + lv] = total;
    }
}

__global__ void __launch_bounds__(1024)
csr_scan_kernel(LatticeDev L, unsigned* __restrict__ bh, int wbpf, int mcap, int n_groups) {
    __shared__ unsigned red[16];
    __shared__ unsigned vbase[64];
    const int frame = blockIdx.x / n_groups, grp = blockIdx.x - frame * n_groups;
    const int2 fv = cs_frame_vertices(L, frame, mcap);
    const int f0 = fv.x, Mf = fv.y;
    const int lv0 = grp * 64;
    if (lv0 >= Mf) return;                   // whole block
    const int lvl = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int sw = (wbpf + CS_SEGS - 1) / CS_SEGS;
    const int w0 = seg * sw, w1 = (w0 + sw < wbpf) ? w0 + sw : wbpf;
    unsigned* fb = bh + (size_t)wbpf * f0;
    const unsigned* vtot = bh + csr_aux_offset(L, wbpf);
    const unsigned* segsum = vtot + L.m_bound;
    const unsigned frame_base = (unsigned)((long long)frame * L.N * (L.d + 1));
    // entries of the frame's vertices before this group
    unsigned part = 0;
    for (int v = threadIdx.x; v < lv0; v += 1024) part += vtot[f0 + v];
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    if (lvl == 0) red[seg] = part;
    __syncthreads();
    unsigned carry = 0;
#pragma unroll
    for (int q = 0; q < 16; q++) carry += red[q];
    const int lv = lv0 + lvl;
    const bool ok = lv < Mf;
    if (seg == 0) {
        const unsigned total = ok ? vtot[f0 + lv] : 0u;
        unsigned incl = total;                // inclusive scan of the 64 column totals (one wave)
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned t = __shfl_up(incl, off, 64);
            if (lvl >= off) incl += t;
        }
        vbase[lvl] = carry + incl - total;
        if (ok) {
            L.vstart[f0 + lv] = frame_base + carry + incl - total;
            L.vend[f0 + lv] = frame_base + carry + incl;
        }
    }
    __syncthreads();
    if (ok) {
        unsigned run = frame_base + vbase[lvl];
        for (int q = 0; q < seg; q++) run += segsum[(size_t)(f0 + lv) * CS_SEGS + q];
        for (int w = w0; w < w1; w++) {
            const unsigned t = fb[(size_t)w * Mf + lv];
            fb[(size_t)w * Mf + lv] = run;
            run += t;
        }
    }
}

bool csr_fast_path(const LatticeDev& L) { return ((L.cap_f_mask + 1) / 2) <= (unsigned)CS_MCAP; }
size_t csr_fast_bytes(const LatticeDev& L) {
    const size_t wbpf = (size_t)cs_launch(L).wbpf;
    // the [wave-block][vertex] matrices of all frames, then per vertex its column total and CS_SEGS segment sums
    return (wbpf * ((size_t)L.m_bound + 64) + (size_t)L.m_bound * (1 + CS_SEGS)) * sizeof(unsigned);
}

// The scatter of the counting-sort path, the last step of its CSR build (nothing to do on the radix-sort path).
void launch_csr_scatter(const LatticeDev& L, SortBuffers& sb, hipStream_t s) {
    if (!(csr_fast_path(L) && sb.block_hist)) return;
    const CsLaunch c = cs_launch(L);
    with_dimension(L.d, [&](auto dim) {
        constexpr int DP1 = decltype(dim)::value + 1;
        if constexpr (DP1 == 7) {   // the only dimension with a 16-bit form
            if (L.ids16) { csr_scatter_kernel<7, true><<<c.grid, c.block, c.lds, s>>>(L, sb.block_hist, c.wbpf, c.mcap); return; }
        }
        if constexpr (DP1 == 3 || DP1 == 6 || DP1 == 7)   // d = 2, 5, 6: the only instantiations of the per-point scatter
            csr_scatter_kernel<DP1><<<c.grid, c.block, c.lds, s>>>(L, sb.block_hist, c.wbpf, c.mcap);
        else
            csr_scatter_entries_kernel<<<c.grid, c.block, c.lds, s>>>(L, sb.block_hist, c.wbpf, c.mcap);
    });
    RV_LAUNCHED("csr_scatter_kernel");
}

// Vertex numbering, neighbours, the CSR and the splat's launch order.  defer_scatter: everything but the scatter of the
// counting-sort path -- counts, list bounds and launch order are all the splat planner needs; the caller launches
// launch_csr_scatter beside it.  (The radix-sort path has no separate scatter and does it all here.)
void launch_lattice_finish(const LatticeDev& L, SortBuffers& sb, long long n_entries, hipStream_t s, bool defer_scatter) {
    const unsigned cap = L.cap_total;
    {
        size_t temp = sb.scan_temp_bytes;
        auto in = rocprim::make_transform_iterator(L.state, SlotFilled());
        (void)rocprim::exclusive_scan(sb.scan_temp, temp, in, L.slot_to_id, 0, (size_t)cap, rocprim::plus<int>(), s);
    }
    lattice_compact_kernel<<<dim3((cap + 255) / 256), dim3(256), 0, s>>>(L);
    const long long nb_threads = (long long)L.m_bound * (L.d + 1);
    lattice_neighbours_kernel<<<dim3((unsigned)((nb_threads + 255) / 256)), dim3(256), 0, s>>>(L);
    RV_LAUNCHED("lattice_compact_kernel / lattice_neighbours_kernel");
    if (csr_fast_path(L) && sb.block_hist) {
        const CsLaunch c = cs_launch(L);
        if (L.ids16) csr_count_kernel<true><<<c.grid, c.block, c.lds, s>>>(L, sb.block_hist, c.wbpf, c.mcap);
        else csr_count_kernel<false><<<c.grid, c.block, c.lds, s>>>(L, sb.block_hist, c.wbpf, c.mcap);
        const int n_groups = (c.mcap + 63) / 64;
        csr_total_kernel<<<dim3((unsigned)(L.n_frames * n_groups)), dim3(1024), 0, s>>>(L, sb.block_hist, c.wbpf, c.mcap, n_groups);
        csr_scan_kernel<<<dim3((unsigned)(L.n_frames * n_groups)), dim3(1024), 0, s>>>(L, sb.block_hist, c.wbpf, c.mcap, n_groups);
        RV_LAUNCHED("csr_count_kernel / csr_total_kernel / csr_scan_kernel");
        if (!defer_scatter) launch_csr_scatter(L, sb, s);
    } else {
        lattice_remap_kernel<<<dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, s>>>(L, sb.keys_in, sb.vals_in, n_entries);
        // stable radix sort by vertex id: equal keys keep ascending entry (= point) order
        size_t temp = sb.temp_bytes;
        (void)rocprim::radix_sort_pairs(sb.temp, temp, sb.keys_in, sb.keys_out, sb.vals_in, sb.vals_out, (size_t)n_entries, 0,
                                        (unsigned)sb.key_bits, s);
        lattice_csr_kernel<<<dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, s>>>(L, sb.keys_out, sb.vals_out, n_entries);
        RV_LAUNCHED("lattice_remap_kernel / radix sort / lattice_csr_kernel");
    }
    launch_vertex_order(L, sb, s);
}

// Launch order of the vertices for the splat: per frame, longest list first.  vorder[fstart[f] + k]
// is the k-th longest vertex of frame f (ids are frame-contiguous, so a sort by (frame, -length)
// keeps every frame in its own id range).  The splat forms its groups of G vertices inside a frame
// and starts all frames' heaviest groups first (LPT: the serial chains of the heaviest vertices
// start at t = 0).
__global__ void __launch_bounds__(256)
vertex_len_kernel(LatticeDev L, unsigned* __restrict__ key, unsigned* __restrict__ ids, int len_shift) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= L.m_bound) return;
    const int M = L.counters[0] < L.m_bound ? L.counters[0] : L.m_bound;
    unsigned k = 0xFFFFFFFFu;  // unused ids sort to the end
    if (v < M) {
        atomicMax(&L.counters[3], (int)(L.vend[v] - L.vstart[v]));   // the longest chain of the chunk (rvseg_last_schedule)
        const unsigned len = (L.vend[v] - L.vstart[v]) >> len_shift;
        const unsigned frame = (unsigned)(unsigned short)(L.vkeys[2 * (size_t)v + 1] >> 48);
        k = ((frame < 1023u ? frame : 1022u) << 22) | (0x3FFFFFu - (len < 0x3FFFFFu ? len : 0x3FFFFFu));
    }
    key[v] = k;
    ids[v] = (unsigned)v;
}

void launch_vertex_order(const LatticeDev& L, SortBuffers& sb, hipStream_t s) {
    int len_shift = 0;   // a list has at most N entries
    while (((long long)L.N >> len_shift) >= (1 << 22)) len_shift++;
    vertex_len_kernel<<<dim3((unsigned)((L.m_bound + 255) / 256)), dim3(256), 0, s>>>(L, sb.keys_in, sb.vals_in, len_shift);
    size_t temp = sb.temp_bytes;
    (void)rocprim::radix_sort_pairs(sb.temp, temp, sb.keys_in, sb.keys_out, sb.vals_in, L.vorder, (size_t)L.m_bound, 0, 32, s);
    RV_LAUNCHED("vertex_len_kernel / radix sort");
}

size_t scan_temp_bytes(unsigned cap) {
    size_t temp = 0;
    int* nul = nullptr;
    auto in = rocprim::make_transform_iterator(nul, SlotFilled());
    (void)rocprim::exclusive_scan(nullptr, temp, in, nul, 0, (size_t)cap, rocprim::plus<int>(), (hipStream_t)0);
    return temp;
}

size_t sort_temp_bytes(long long n_entries, int key_bits) {
    size_t temp = 0;
    unsigned* nul = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, temp, nul, nul, nul, nul, (size_t)n_entries, 0, (unsigned)key_bits, (hipStream_t)0);
    return temp;
}

// norm values gathered into CSR order once the normaliser exists
__global__ void __launch_bounds__(256)
csr_norm_kernel(const uint2* __restrict__ csr_pw, const float* __restrict__ norm, float* __restrict__ csr_nrm, long long n_entries,
                const int* __restrict__ counters) {
    if (counters[1]) return;   // hash overflow (flagged): the csr arrays are incomplete
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_entries) csr_nrm[k] = norm[csr_pw[k].x];
}

void launch_csr_norm(const LatticeDev& L, long long n_entries, hipStream_t s) {
    csr_norm_kernel<<<dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, s>>>(L.csr_pw, L.norm, L.csr_nrm, n_entries, L.counters);
    RV_LAUNCHED("csr_norm_kernel");
}
int csr_pix_min() { return CS_PIX_MIN; }

}  // namespace rvseg
