// Kernels of the forest trainer (rvseg_train.hip holds the learner and describes the design; train_device.h the
// interface).  Per level of a tree:
//   * byte-valued features: one pass adds every bootstrap example into its node's (feature, value, class) histogram with
//     global atomics; one block per (node, feature) prefix-sums the 256 values in LDS and evaluates every cut between two
//     occupied values;
//   * other features: the (node, feature, value) triples of the level are sorted once (64-bit radix sort), one wave per
//     (node, feature) segment walks its values in ascending order with running class counts (wave scans) and evaluates
//     every cut between two values at least 1e-6 apart (learning.cpp:578-585);
//   * one pass routes every example with the evaluator's own rule `x[f] < threshold`.
// Per boosting round (BoostedRandomForestLearner::learn, learning.cpp:1162-1217): the weighted resample as a binary search
// per draw, the misclassification flags, and the three fp32 sums the reference accumulates in example order -- error, the
// weights' total, their running sum -- each by one wave that adds a tile of 256 values at once where that is exact
// (ordered_tile) and one after the other where it is not, so the result is the serial chain's bit for bit.
// The objective is the oracle's definition 2 (oracle/rvseg_oracle_train.c), in its operation order, or -- in the weighted
// instantiation of the two cut kernels -- definition 2 of rvseg_class_prior (include/rvseg.h).
#include <cstring>   // rocPRIM's headers call memset without including it

#include <rocprim/rocprim.hpp>

#include "rvseg_internal.h"
#include "train_device.h"

namespace rvseg {
namespace {

// order-preserving map float -> uint (sort keys)
__device__ __forceinline__ unsigned f2ord(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f_dev(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// fastlog2 (fastlog.h:47-58) and ENTROPY(p) = -(p) * fastlog2(p) (learning.cpp:13), in the oracle's operation order
__device__ __forceinline__ float fastlog2_dev(float x) {
    const unsigned vi = __float_as_uint(x);
    const float mx = __uint_as_float((vi & 0x007FFFFFu) | 0x3f000000u);
    float y = (float)vi;
    y = y * 1.1920928955078125e-7f;
    const float a = 1.498030302f * mx;
    const float den = 0.3520887068f + mx;
    const float b = 1.72587999f / den;
    float r = y - 124.22551499f;
    r = r - a;
    r = r - b;
    return r;
}
__device__ __forceinline__ float entropy_term(float p) { return (-p) * fastlog2_dev(p); }

// initEntropies (learning.cpp:279-293) from integer counts: -ENTROPY(mass) + sum of ENTROPY(count) over the classes
// with a non-zero count, ascending
__device__ __forceinline__ float hist_entropy(const unsigned (&cnt)[TR_CMAX]) {
    unsigned mass = 0;
#pragma unroll
    for (int c = 0; c < TR_CMAX; c++) mass += cnt[c];
    float total = -entropy_term((float)mass);
#pragma unroll
    for (int c = 0; c < TR_CMAX; c++) {
        if (cnt[c] == 0) continue;
        total += entropy_term((float)cnt[c]);
    }
    return total;
}

// The class-weighted objective of one side (include/rvseg.h, rvseg_class_prior, definition 2): the weighted mass and
// the weighted counts are w_c * (float)n_c, each product rounded before it is added, over the classes with n_c > 0 in
// ascending order.  The weight of a class the side does not hold is never read.
__device__ __forceinline__ float hist_entropy_weighted(const unsigned (&cnt)[TR_CMAX], const ClassWeights& cw) {
    float mass = 0.0f;
#pragma unroll
    for (int c = 0; c < TR_CMAX; c++) {
        if (cnt[c] == 0) continue;
        mass += cw.w[c] * (float)cnt[c];
    }
    float total = -entropy_term(mass);
#pragma unroll
    for (int c = 0; c < TR_CMAX; c++) {
        if (cnt[c] == 0) continue;
        total += entropy_term(cw.w[c] * (float)cnt[c]);
    }
    return total;
}

// The two cut kernels end in a parameter pack `cw`: empty, they are the kernels of the integer objective as they always
// were; holding a ClassWeights, they are the weighted instantiation.
__device__ __forceinline__ float side_entropy(const unsigned (&cnt)[TR_CMAX]) { return hist_entropy(cnt); }
__device__ __forceinline__ float side_entropy(const unsigned (&cnt)[TR_CMAX], const ClassWeights& cw) { return hist_entropy_weighted(cnt, cw); }

// ---- the rules every kernel shares ----------------------------------------------------------------------------
// a feature's value lives in Xb when it is byte-valued, else in its row of Xf
__device__ __forceinline__ float feature_value(const TrainSetView& v, int f, size_t i) {
    const int nb = v.nb_index[f];
    return nb < 0 ? (float)v.Xb[(size_t)f * v.stride + i] : v.Xf[(size_t)nb * v.stride + i];
}
__device__ __forceinline__ void store_feature(const TrainSetView& v, int f, size_t i, float x) {
    const int nb = v.nb_index[f];
    if (nb < 0) v.Xb[(size_t)f * v.stride + i] = (uint8_t)(int)x;
    else v.Xf[(size_t)nb * v.stride + i] = x;
}
// the slot that example i is searched in and its multiplicity; -1 when i is past the set, was not drawn by the bootstrap
// or sits in a node outside the batch
__device__ __forceinline__ int slot_of_example(const TrainSetView& v, const LevelSlots& sl, int i, unsigned* weight) {
    if (i >= v.P) return -1;
    *weight = sl.w[i];
    if (!*weight) return -1;
    return sl.slot_of[sl.node_of[i]];
}

// ---- data set construction ------------------------------------------------------------------------------------
// per feature: is every value an integer in [0, 255]?
__global__ void __launch_bounds__(256)
train_feature_stats_kernel(const float* __restrict__ X, int P, int D, int* __restrict__ not_byte, int* __restrict__ not_finite) {
    const int f = blockIdx.x;
    int bad = 0, inf = 0;
    for (int i = threadIdx.x; i < P; i += 256) {
        const float v = X[(size_t)i * D + f];
        if (!(v >= 0.f && v <= 255.f && v == floorf(v))) bad = 1;
        if (!(fabsf(v) <= 3.4e38f)) inf = 1;
    }
    if (bad) not_byte[f] = 1;
    if (inf) not_finite[0] = 1;
}

__global__ void __launch_bounds__(256)
train_pack_kernel(const float* __restrict__ X, TrainSetView v) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)v.P * v.D) return;
    const int f = (int)(gid / v.P), i = (int)(gid - (long long)f * v.P);
    store_feature(v, f, (size_t)i, X[(size_t)i * v.D + f]);
}

// frames -> training set (src/train.cpp:115-147): flags[p] = the stride-grid point has valid depth (extract's mask) and
// every label layer is >= 0 there (ExtractType::WITH_POSITIVE_LABEL, feature_extractor.h:93-121)
__global__ void __launch_bounds__(256)
train_frame_flags_kernel(FrameGeom g, const uint8_t* __restrict__ valid, const int8_t* __restrict__ labels, int L, int* __restrict__ flags) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= g.lw * g.lh) return;
    const int ly = p / g.lw, lx = p - ly * g.lw;
    const size_t px = (size_t)(ly * g.stride) * g.W + (size_t)lx * g.stride;
    int ok = valid[p] ? 1 : 0;
    for (int l = 0; l < L; l++) ok = ok && labels[(size_t)l * g.W * g.H + px] >= 0;
    flags[p] = ok;
}

__global__ void __launch_bounds__(256)
train_frame_scatter_kernel(FrameGeom g, const int* __restrict__ flags, const int* __restrict__ offs, const float* __restrict__ dump,
                           const int8_t* __restrict__ labels, size_t base, TrainSetView v) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int Pg = g.lw * g.lh;
    if (gid >= (long long)Pg * (g.D + v.L)) return;
    const int col = (int)(gid / Pg), p = (int)(gid - (long long)col * Pg);
    if (!flags[p]) return;
    const size_t dst = base + (size_t)offs[p];
    if (col < g.D) {
        store_feature(v, col, dst, dump[(size_t)p * g.D + col]);
    } else {
        const int l = col - g.D;
        const int ly = p / g.lw, lx = p - ly * g.lw;
        v.lab[(size_t)l * v.stride + dst] = labels[(size_t)l * g.W * g.H + (size_t)(ly * g.stride) * g.W + (size_t)lx * g.stride];
    }
}

// mult: how often the tree's data set holds example i (a boosting round's resample), or null: once
__global__ void __launch_bounds__(256)
train_class_count_kernel(TrainSetView v, const unsigned* __restrict__ mult, unsigned* __restrict__ cnt) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)v.P * v.L) return;
    const int l = (int)(gid / v.P), i = (int)(gid - (long long)l * v.P);
    const unsigned m = mult ? mult[i] : 1u;
    if (m) atomicAdd(&cnt[l * TR_CMAX + v.lab[(size_t)l * v.stride + i]], m);
}

// ---- per tree -------------------------------------------------------------------------------------------------
// bootstrap: P draws with replacement as multiplicities (DataStorage::bootstrapmulti, data.cpp:325-349)
// (positions: the examples at the P positions of a resampled data set, or null: position n is example n)
__global__ void __launch_bounds__(256)
train_bootstrap_kernel(int P, uint64_t kt, const int* __restrict__ positions, unsigned* __restrict__ w) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= P) return;
    const uint64_t pos = draw64(kt, 0x100000000ull + (uint64_t)n) % (uint64_t)P;
    atomicAdd(&w[positions ? (uint64_t)positions[pos] : pos], 1u);
}

// class totals of every slot (the node's histogram, learning.cpp:508-516)
__global__ void __launch_bounds__(256)
train_slot_totals_kernel(TrainSetView v, LevelSlots sl, unsigned* __restrict__ totals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned wi;
    const int slot = slot_of_example(v, sl, i, &wi);
    if (slot < 0) return;
    atomicAdd(&totals[slot * TR_CMAX + v.lab[(size_t)sl.slot_layer[slot] * v.stride + i]], wi);
}

// hist[slot][k][value][class] += multiplicity, byte features of the slot only
__global__ void __launch_bounds__(256)
train_hist_kernel(TrainSetView v, LevelSlots sl, unsigned* __restrict__ hist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned wi;
    const int slot = slot_of_example(v, sl, i, &wi);
    if (slot < 0) return;
    const int c = v.lab[(size_t)sl.slot_layer[slot] * v.stride + i];
    for (int k = 0; k < sl.K; k++) {
        const int f = sl.slot_feat[slot * sl.K + k];
        if (v.nb_index[f] >= 0) continue;
        const int b = v.Xb[(size_t)f * v.stride + i];
        atomicAdd(&hist[(((size_t)slot * sl.K + k) * TR_BINS + b) * TR_CMAX + c], wi);
    }
}

// byte features: one block per (slot, feature), one thread per value
template <class... WEIGHTS>
__global__ void __launch_bounds__(TR_BINS)
train_best_cut_kernel(TrainSetView ts, LevelSlots sl, const unsigned* __restrict__ hist, CutResult* __restrict__ out, WEIGHTS... cw) {
    __shared__ unsigned h[TR_CMAX][TR_BINS + 1];   // inclusive prefix over the values, per class
    __shared__ unsigned occ[TR_BINS];
    __shared__ float best_obj[TR_BINS];
    __shared__ int best_bin[TR_BINS];
    if (ts.nb_index[sl.slot_feat[blockIdx.x]] >= 0) return;   // a float feature: the sorted path writes this record
    const int b = threadIdx.x;
    const unsigned* src = hist + ((size_t)blockIdx.x * TR_BINS + b) * TR_CMAX;
    unsigned row = 0;
#pragma unroll
    for (int c = 0; c < TR_CMAX; c++) { const unsigned v = src[c]; h[c][b] = v; row += v; }
    occ[b] = row;
    __syncthreads();
    for (int off = 1; off < TR_BINS; off <<= 1) {   // inclusive scan over the 256 values, all classes at once
        unsigned add[TR_CMAX];
#pragma unroll
        for (int c = 0; c < TR_CMAX; c++) add[c] = b >= off ? h[c][b - off] : 0u;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < TR_CMAX; c++) h[c][b] += add[c];
        __syncthreads();
    }
    int nb = -1;   // next occupied value above b
    if (row) for (int q = b + 1; q < TR_BINS; q++) if (occ[q]) { nb = q; break; }
    float obj = 1e35f;
    unsigned lm = 0, rm = 0;
    if (nb >= 0) {
        unsigned l[TR_CMAX], r[TR_CMAX];
#pragma unroll
        for (int c = 0; c < TR_CMAX; c++) { l[c] = h[c][b]; r[c] = h[c][TR_BINS - 1] - l[c]; lm += l[c]; rm += r[c]; }
        const float el = side_entropy(l, cw...), er = side_entropy(r, cw...);
        obj = el + er;
    }
    best_obj[b] = obj;
    best_bin[b] = nb >= 0 ? b : TR_BINS;
    __syncthreads();
    for (int s = TR_BINS / 2; s > 0; s >>= 1) {   // arg min; the lower value wins a tie (strict '<' in ascending order, :589)
        if (b < s) {
            const float o2 = best_obj[b + s];
            const int b2 = best_bin[b + s];
            if (o2 < best_obj[b] || (o2 == best_obj[b] && b2 < best_bin[b])) { best_obj[b] = o2; best_bin[b] = b2; }
        }
        __syncthreads();
    }
    if (best_bin[0] == TR_BINS) {
        if (b == 0) { CutResult r{}; r.objective = 1e35f; r.valid = 0; out[blockIdx.x] = r; }
        return;
    }
    if (b == best_bin[0]) {
        CutResult r;
        r.objective = obj;
        r.left_value = (float)b;
        r.right_value = (float)nb;
        r.left_mass = lm;
        r.right_mass = rm;
        r.valid = 1;
        out[blockIdx.x] = r;
    }
}

// float features: (segment << 32 | ordered value, example) for every (bootstrap example, sampled float feature of its node)
__global__ void __launch_bounds__(256)
train_nb_emit_kernel(TrainSetView v, LevelSlots sl, unsigned long long* __restrict__ keys, unsigned* __restrict__ vals,
                     unsigned* __restrict__ counter, unsigned capacity) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned wi;
    const int slot = slot_of_example(v, sl, i, &wi);
    if (slot < 0) return;
    for (int k = 0; k < sl.K; k++) {
        const int nb = v.nb_index[sl.slot_feat[slot * sl.K + k]];
        if (nb < 0) continue;
        const unsigned pos = atomicAdd(counter, 1u);
        if (pos >= capacity) continue;   // cannot happen: capacity = P * min(K, n_nb)
        keys[pos] = ((unsigned long long)(unsigned)(slot * sl.K + k) << 32) | f2ord(v.Xf[(size_t)nb * v.stride + i]);
        vals[pos] = (unsigned)i;
    }
}

// one wave per (slot, feature) segment of the sorted triples: ascending values, running class counts, every cut between
// two values at least 1e-6 apart (learning.cpp:560-604)
template <class... WEIGHTS>
__global__ void __launch_bounds__(64)
train_nb_scan_kernel(TrainSetView ts, LevelSlots sl, unsigned n_items, const unsigned long long* __restrict__ keys,
                     const unsigned* __restrict__ vals, const unsigned* __restrict__ totals, CutResult* __restrict__ out, WEIGHTS... cw) {
    const unsigned seg = blockIdx.x;
    if (ts.nb_index[sl.slot_feat[seg]] < 0) return;   // a byte feature: the histogram path writes this record
    const int lane = threadIdx.x;
    const int slot = (int)(seg / (unsigned)sl.K);
    // the segment's range in the sorted array (keys are unique per segment in their high word)
    auto lower = [&](unsigned long long key) {
        unsigned lo = 0, hi = n_items;
        while (lo < hi) { const unsigned mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
        return lo;
    };
    const unsigned beg = lower((unsigned long long)seg << 32), end = lower((unsigned long long)(seg + 1u) << 32);
    unsigned tot[TR_CMAX], run[TR_CMAX];
    unsigned mass = 0;
#pragma unroll
    for (int c = 0; c < TR_CMAX; c++) { tot[c] = totals[slot * TR_CMAX + c]; run[c] = 0; mass += tot[c]; }
    const int* labl = ts.lab + (size_t)sl.slot_layer[slot] * ts.stride;
    float best_obj = 1e35f, best_lv = 0.f, best_rv = 0.f;
    unsigned best_lm = 0;
    float prev_last = 0.f;   // value of the last element of the previous chunk
    for (unsigned base = beg; base < end; base += 64) {
        const unsigned m = base + (unsigned)lane;
        const bool in = m < end;
        float v = 0.f;
        int cls = -1;
        unsigned wt = 0;
        if (in) {
            v = ord2f_dev((unsigned)(keys[m] & 0xFFFFFFFFull));
            const unsigned e = vals[m];
            cls = labl[e];
            wt = sl.w[e];
        }
        float vprev = __shfl_up(v, 1, 64);
        if (lane == 0) vprev = prev_last;
        // class counts of the elements before this lane's element
        unsigned left[TR_CMAX];
        unsigned lm = 0;
#pragma unroll
        for (int c = 0; c < TR_CMAX; c++) {
            const unsigned x = cls == c ? wt : 0u;
            unsigned incl = x;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned t = __shfl_up(incl, off, 64);
                if (lane >= off) incl += t;
            }
            left[c] = run[c] + incl - x;
            lm += left[c];
            run[c] += __shfl(incl, 63, 64);
        }
        float obj = 1e35f;
        if (in && m > beg && !((v - vprev) < 1e-6f)) {
            unsigned right[TR_CMAX];
#pragma unroll
            for (int c = 0; c < TR_CMAX; c++) right[c] = tot[c] - left[c];
            const float el = side_entropy(left, cw...), er = side_entropy(right, cw...);
            obj = el + er;
        }
        // the chunk's minimum, lowest position first; strict '<' against the running best
        float o = obj;
        int who = lane;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float o2 = __shfl_xor(o, off, 64);
            const int w2 = __shfl_xor(who, off, 64);
            if (o2 < o || (o2 == o && w2 < who)) { o = o2; who = w2; }
        }
        if (o < best_obj) {
            best_obj = o;
            best_lv = __shfl(vprev, who, 64);
            best_rv = __shfl(v, who, 64);
            best_lm = __shfl(lm, who, 64);
        }
        const unsigned last = (end - base < 64u ? end - base : 64u) - 1u;
        prev_last = __shfl(v, (int)last, 64);
    }
    if (lane == 0) {
        CutResult r;
        r.objective = best_obj;
        r.left_value = best_lv;
        r.right_value = best_rv;
        r.left_mass = best_lm;
        r.right_mass = mass - best_lm;
        r.valid = best_obj < 1e35f ? 1 : 0;
        out[seg] = r;
    }
}

// findLeafNode's rule on the freshly split nodes: every example (bootstrap or not) moves to a child
__global__ void __launch_bounds__(256)
train_route_kernel(TrainSetView v, int* __restrict__ node_of, const int* __restrict__ split_feat, const float* __restrict__ split_thr,
                   const int* __restrict__ split_left) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= v.P) return;
    const int node = node_of[i];
    const int f = split_feat[node];
    if (f < 0) return;
    node_of[i] = feature_value(v, f, (size_t)i) < split_thr[node] ? split_left[node] : split_left[node] + 1;   // classifier.cpp:105
}

// integer leaf counts over ALL examples: cnt[node][layer][class]
__global__ void __launch_bounds__(256)
train_leaf_count_kernel(TrainSetView v, const int* __restrict__ node_of, const unsigned* __restrict__ mult, unsigned* __restrict__ cnt) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)v.P * v.L) return;
    const int l = (int)(gid / v.P), i = (int)(gid - (long long)l * v.P);
    const unsigned m = mult ? mult[i] : 1u;
    if (m) atomicAdd(&cnt[((size_t)node_of[i] * v.L + l) * TR_CMAX + v.lab[(size_t)l * v.stride + i]], m);
}

// ---- per boosting round ---------------------------------------------------------------------------------------
// the weighted resample (learning.cpp:1166-1175): draw n picks the first index with !(u > cumsum[index]).  cumsum does
// not decrease (the weights are >= 0), so the binary search finds what the reference's linear scan finds; the index is
// clamped to N - 1, where the reference reads past the array when rounding leaves cumsum[N-1] < u.
__global__ void __launch_bounds__(256)
train_boost_resample_kernel(const float* __restrict__ cumsum, int N, uint64_t kb, int* __restrict__ idx, unsigned* __restrict__ mult) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float u = boost_uniform(kb, (uint64_t)n);
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (u > cumsum[mid]) lo = mid + 1; else hi = mid;
    }
    if (lo > N - 1) lo = N - 1;
    idx[n] = lo;
    if (mult) atomicAdd(&mult[lo], 1u);
}

// miss[n] = the tree's vote for example n of the whole set is not its label (:1182-1194); vote_label: per node of the
// growing tree, the label its leaf histogram votes for
__global__ void __launch_bounds__(256)
train_vote_flags_kernel(const int* __restrict__ node_of, const int* __restrict__ vote_label, const int* __restrict__ label, int N,
                        uint8_t* __restrict__ miss) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    miss[n] = vote_label[node_of[n]] != label[n] ? 1 : 0;
}

// The ordered sums, without the serial chain (the idea of the normaliser's splat, kernels_splat.hip / DESIGN section 4,
// restated here with the running sums kept).  The chain only LOOKS sequential: while the running sum s stays in one
// binade [2^E, 2^(E+1)) every partial sum is a multiple of u = 2^(E-23), and adding w >= 0 rounds s + w to the nearest
// multiple of u -- in units of u: n -> n + rne(w / u), unless w / u lies exactly half-way between two integers (then the
// direction depends on the parity of n).  So for a tile of addends none of which is negative or such a tie, and which
// does not leave the binade,
//       s after addend i = (n + sum_{j <= i} rne(w_j / u)) * u,
// sums of integers below 2^24: exact in fp32 in ANY order, so a wave prefix sum gives all of them at once.  One wave
// takes a tile of 256 addends, lane l the addends 4 l .. 4 l + 3; a tile that breaks a condition (s not yet a positive
// normal number, a binade crossing, a tie) is added the reference's way, one addend after the other.  Either way the
// result is the serial chain's bit for bit.  Addends past the end and examples that are not misses count as +0.0, which
// leaves the sum as it is: s starts at +0.0 and only takes addends >= +0, so it is never -0.0.
constexpr int SUM_K = 4;        // addends per lane and tile
constexpr int SUM_DEPTH = 8;    // tiles in flight: the next 8 load while these are added

__device__ __forceinline__ float wave_inclusive_sum(float v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// s + (the tile), rounded after every addition; KEEP: out[h] = the running sum after this lane's addend h
template <bool KEEP>
__device__ __forceinline__ void ordered_tile(float& s, const float (&w)[SUM_K], float (&out)[SUM_K], int lane) {
    bool any = false;
#pragma unroll
    for (int h = 0; h < SUM_K; h++) any |= w[h] != 0.0f;
    if (__builtin_amdgcn_ballot_w64(any) == 0ull) {      // nothing to add (x + 0.0 = x)
#pragma unroll
        for (int h = 0; h < SUM_K; h++) out[h] = s;
        return;
    }
    const unsigned sb = __float_as_uint(s);
    const unsigned e = (sb >> 23) & 0xffu;                              // biased exponent of the running sum
    const bool s_ok = ((int)sb > 0) & (e >= 24u) & (e <= 253u);        // positive, normal, scale factors representable
    const float scale = __uint_as_float((277u - (s_ok ? e : 127u)) << 23);      // 2^(23 - E) = 1 / u
    const float unscale = __uint_as_float(((s_ok ? e : 127u) - 23u) << 23);     // u
    float pre[SUM_K];
    float rs = 0.0f;
    bool bad = false;
#pragma unroll
    for (int h = 0; h < SUM_K; h++) {
        const float k = w[h] * scale;                 // exact (a power of two), or +inf
        const float r = __builtin_rintf(k);           // round half to even, like the addition itself
        bad |= !(w[h] >= 0.0f) | !(k < 16777216.0f) | (__builtin_fabsf(k - r) == 0.5f);
        rs += r;                                      // (sums of integers: exact while below 2^24; rounding is monotone)
        pre[h] = rs;
    }
    const float incl = wave_inclusive_sum(rs, lane);
    const float n0 = s * scale;
    const float total = __shfl(incl, 63, 64);
    if (s_ok & (__builtin_amdgcn_ballot_w64(bad) == 0ull) & (n0 + total < 16777216.0f)) {
        const float before = n0 + (incl - rs);
#pragma unroll
        for (int h = 0; h < SUM_K; h++) out[h] = (before + pre[h]) * unscale;
        s = (n0 + total) * unscale;
        return;
    }
#pragma unroll 1
    for (int i = 0; i < 64; i++)                      // the reference's way
#pragma unroll
        for (int h = 0; h < SUM_K; h++) {
            s = s + __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(w[h]), i));
            if (KEEP && lane == i) out[h] = s;
        }
}

// MODE 0: error = sum of w[n] over the misses (:1181-1194)
// MODE 1: w[n] *= scale for the misses, total = sum of w[n] (:1202-1210)
// MODE 2: w[n] /= total, cumsum[n] = w[n] + cumsum[n-1] (:1211-1217)
template <int MODE>
__global__ void __launch_bounds__(64)
train_boost_sum_kernel(float* __restrict__ w, const uint8_t* __restrict__ miss, long long N, float scale, float* __restrict__ sum,
                       float* __restrict__ cumsum) {
    const int lane = threadIdx.x;
    const float total = MODE == 2 ? *sum : 0.f;
    // this lane's 4 addends of the tile that starts at n0 (a multiple of 256), with the mode's update of w written back
    auto load = [&](long long n0, float (&x)[SUM_K]) {
        const long long n = n0 + (long long)lane * SUM_K;
        unsigned char m[SUM_K] = {0, 0, 0, 0};
        if (n + SUM_K <= N) {
            const float4 v = *reinterpret_cast<const float4*>(w + n);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
            if (MODE != 2) {
                const unsigned mm = *reinterpret_cast<const unsigned*>(miss + n);
#pragma unroll
                for (int h = 0; h < SUM_K; h++) m[h] = (unsigned char)((mm >> (8 * h)) & 0xffu);
            }
        } else {
#pragma unroll
            for (int h = 0; h < SUM_K; h++) {
                x[h] = n + h < N ? w[n + h] : 0.f;
                if (MODE != 2) m[h] = n + h < N ? miss[n + h] : (unsigned char)0;
            }
        }
#pragma unroll
        for (int h = 0; h < SUM_K; h++) {
            if (MODE == 0) x[h] = m[h] ? x[h] : 0.f;
            if (MODE == 1) x[h] = m[h] ? x[h] * scale : x[h];
            if (MODE == 2) x[h] = n + h < N ? x[h] / total : 0.f;
        }
        if (MODE != 0) {
            if (n + SUM_K <= N) {
                *reinterpret_cast<float4*>(w + n) = make_float4(x[0], x[1], x[2], x[3]);
            } else {
#pragma unroll
                for (int h = 0; h < SUM_K; h++) if (n + h < N) w[n + h] = x[h];
            }
        }
    };
    constexpr long long TILE = 64 * SUM_K;
    float cur[SUM_DEPTH][SUM_K], next[SUM_DEPTH][SUM_K];
#pragma unroll
    for (int j = 0; j < SUM_DEPTH; j++) load((long long)j * TILE, cur[j]);
    float run = 0.f;
    for (long long base = 0; base < N; base += SUM_DEPTH * TILE) {
#pragma unroll
        for (int j = 0; j < SUM_DEPTH; j++) load(base + (long long)(SUM_DEPTH + j) * TILE, next[j]);
#pragma unroll
        for (int j = 0; j < SUM_DEPTH; j++) {
            float out[SUM_K];
            ordered_tile<MODE == 2>(run, cur[j], out, lane);
            if (MODE == 2) {
                const long long n = base + (long long)j * TILE + (long long)lane * SUM_K;
                if (n + SUM_K <= N) {
                    *reinterpret_cast<float4*>(cumsum + n) = make_float4(out[0], out[1], out[2], out[3]);
                } else {
#pragma unroll
                    for (int h = 0; h < SUM_K; h++) if (n + h < N) cumsum[n + h] = out[h];
                }
            }
#pragma unroll
            for (int h = 0; h < SUM_K; h++) cur[j][h] = next[j][h];
        }
    }
    if (MODE != 2 && lane == 0) *sum = run;
}

inline dim3 blocks_of(long long threads) { return dim3((unsigned)((threads + 255) / 256)); }

// Which objective a cut launch uses, stated once: no weights (RVSEG_PRIOR_NONE) is the integer expression of today's
// kernels, never the weighted one run with ones -- (float)(sum of n_c) and the sum of (float)n_c differ above 2^24.
inline bool use_weighted_objective(const ClassWeights* cw) { return cw != nullptr; }

}  // namespace

void launch_train_feature_stats(const float* X, int P, int D, int* not_byte, int* not_finite, hipStream_t s) {
    train_feature_stats_kernel<<<dim3((unsigned)D), dim3(256), 0, s>>>(X, P, D, not_byte, not_finite);
    RV_LAUNCHED("train_feature_stats_kernel");
}

void launch_train_pack(const float* X, const TrainSetView& v, hipStream_t s) {
    train_pack_kernel<<<blocks_of((long long)v.P * v.D), dim3(256), 0, s>>>(X, v);
    RV_LAUNCHED("train_pack_kernel");
}

void launch_train_frame_flags(const FrameGeom& g, const uint8_t* valid, const int8_t* labels, int L, int* flags, hipStream_t s) {
    train_frame_flags_kernel<<<blocks_of(g.lw * g.lh), dim3(256), 0, s>>>(g, valid, labels, L, flags);
    RV_LAUNCHED("train_frame_flags_kernel");
}

void launch_train_frame_scatter(const FrameGeom& g, const int* flags, const int* offs, const float* dump, const int8_t* labels, size_t base,
                                const TrainSetView& v, hipStream_t s) {
    train_frame_scatter_kernel<<<blocks_of((long long)g.lw * g.lh * (g.D + v.L)), dim3(256), 0, s>>>(g, flags, offs, dump, labels, base, v);
    RV_LAUNCHED("train_frame_scatter_kernel");
}

size_t train_scan_temp_bytes(size_t n) {
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (const int*)nullptr, (int*)nullptr, 0, n, rocprim::plus<int>());
    return bytes;
}

hipError_t launch_train_scan_offsets(void* temp, size_t temp_bytes, const int* flags, int* offs, size_t n, hipStream_t s) {
    return rocprim::exclusive_scan(temp, temp_bytes, flags, offs, 0, n, rocprim::plus<int>(), s);
}

void launch_train_class_count(const TrainSetView& v, const unsigned* mult, unsigned* cnt, hipStream_t s) {
    train_class_count_kernel<<<blocks_of((long long)v.P * v.L), dim3(256), 0, s>>>(v, mult, cnt);
    RV_LAUNCHED("train_class_count_kernel");
}

void launch_train_bootstrap(int P, uint64_t kt, const int* positions, unsigned* w, hipStream_t s) {
    train_bootstrap_kernel<<<blocks_of(P), dim3(256), 0, s>>>(P, kt, positions, w);
    RV_LAUNCHED("train_bootstrap_kernel");
}

void launch_train_search_bytes(const TrainSetView& v, const LevelSlots& sl, int S, const ClassWeights* cw, unsigned* totals, unsigned* hist,
                               CutResult* cuts, hipStream_t s) {
    train_slot_totals_kernel<<<blocks_of(v.P), dim3(256), 0, s>>>(v, sl, totals);
    RV_LAUNCHED("train_slot_totals_kernel");
    train_hist_kernel<<<blocks_of(v.P), dim3(256), 0, s>>>(v, sl, hist);
    RV_LAUNCHED("train_hist_kernel");
    if (use_weighted_objective(cw)) {
        train_best_cut_kernel<<<dim3((unsigned)(S * sl.K)), dim3(TR_BINS), 0, s>>>(v, sl, hist, cuts, *cw);
        RV_LAUNCHED("train_best_cut_kernel<weighted>");
    } else {
        train_best_cut_kernel<<<dim3((unsigned)(S * sl.K)), dim3(TR_BINS), 0, s>>>(v, sl, hist, cuts);
        RV_LAUNCHED("train_best_cut_kernel");
    }
}

void launch_train_emit(const TrainSetView& v, const LevelSlots& sl, unsigned long long* keys, unsigned* vals, unsigned* counter,
                       unsigned capacity, hipStream_t s) {
    train_nb_emit_kernel<<<blocks_of(v.P), dim3(256), 0, s>>>(v, sl, keys, vals, counter, capacity);
    RV_LAUNCHED("train_nb_emit_kernel");
}

size_t train_sort_temp_bytes(size_t n) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned*)nullptr,
                                    (unsigned*)nullptr, n, 0, 64);
    return bytes;
}

hipError_t launch_train_sort(void* temp, size_t temp_bytes, unsigned long long* keys_in, unsigned long long* keys_out, unsigned* vals_in,
                             unsigned* vals_out, size_t n, unsigned end_bit, hipStream_t s) {
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0, end_bit, s);
}

void launch_train_scan(const TrainSetView& v, const LevelSlots& sl, int S, const ClassWeights* cw, unsigned n_items, const unsigned long long* keys,
                       const unsigned* vals, const unsigned* totals, CutResult* cuts, hipStream_t s) {
    if (use_weighted_objective(cw)) {
        train_nb_scan_kernel<<<dim3((unsigned)(S * sl.K)), dim3(64), 0, s>>>(v, sl, n_items, keys, vals, totals, cuts, *cw);
        RV_LAUNCHED("train_nb_scan_kernel<weighted>");
    } else {
        train_nb_scan_kernel<<<dim3((unsigned)(S * sl.K)), dim3(64), 0, s>>>(v, sl, n_items, keys, vals, totals, cuts);
        RV_LAUNCHED("train_nb_scan_kernel");
    }
}

void launch_train_route(const TrainSetView& v, int* node_of, const int* split_feat, const float* split_thr, const int* split_left,
                        hipStream_t s) {
    train_route_kernel<<<blocks_of(v.P), dim3(256), 0, s>>>(v, node_of, split_feat, split_thr, split_left);
    RV_LAUNCHED("train_route_kernel");
}

void launch_train_leaf_count(const TrainSetView& v, const int* node_of, const unsigned* mult, unsigned* cnt, hipStream_t s) {
    train_leaf_count_kernel<<<blocks_of((long long)v.P * v.L), dim3(256), 0, s>>>(v, node_of, mult, cnt);
    RV_LAUNCHED("train_leaf_count_kernel");
}

void launch_train_boost_resample(const float* cumsum, int N, uint64_t kb, int* idx, unsigned* mult, hipStream_t s) {
    train_boost_resample_kernel<<<blocks_of(N), dim3(256), 0, s>>>(cumsum, N, kb, idx, mult);
    RV_LAUNCHED("train_boost_resample_kernel");
}

void launch_train_vote_flags(const int* node_of, const int* vote_label, const int* label, int N, uint8_t* miss, hipStream_t s) {
    train_vote_flags_kernel<<<blocks_of(N), dim3(256), 0, s>>>(node_of, vote_label, label, N, miss);
    RV_LAUNCHED("train_vote_flags_kernel");
}

void launch_train_boost_error(const float* w, const uint8_t* miss, int N, float* error, hipStream_t s) {
    train_boost_sum_kernel<0><<<dim3(1), dim3(64), 0, s>>>(const_cast<float*>(w), miss, N, 1.f, error, nullptr);
    RV_LAUNCHED("train_boost_sum_kernel<error>");
}

void launch_train_boost_update_total(float* w, const uint8_t* miss, int N, float scale, float* total, hipStream_t s) {
    train_boost_sum_kernel<1><<<dim3(1), dim3(64), 0, s>>>(w, miss, N, scale, total, nullptr);
    RV_LAUNCHED("train_boost_sum_kernel<total>");
}

void launch_train_boost_update_cumsum(float* w, int N, const float* total, float* cumsum, hipStream_t s) {
    train_boost_sum_kernel<2><<<dim3(1), dim3(64), 0, s>>>(w, nullptr, N, 1.f, const_cast<float*>(total), cumsum);
    RV_LAUNCHED("train_boost_sum_kernel<cumsum>");
}

}  // namespace rvseg
