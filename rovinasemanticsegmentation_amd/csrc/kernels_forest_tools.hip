// The kernels over a chunk of points with materialised features for gfx950 (rvseg_forest_tools.hip): the forest's
// posterior sums (rvseg_forest_eval) and the device side of libforest's tools.h.
//
// Reference semantics:
//   findLeafNode                 classifier.cpp:97-117    node = x[feature] < threshold ? left : left + 1   (strict '<', fp32)
//   Classifier::classify         classifier.cpp:29-51     label 0, then index i wins iff post[i] > prob (vote_label)
//   RandomForest posterior       classifier.cpp:166-208   tree 0's leaf row, then += trees 1..T-1 IN ORDER (fp32)
//   DecisionTree::classify       tools.cpp:214-218        the label rule on the tree's own leaf histogram
//   ConfusionMatrixTool          tools.cpp:121-128        counts [true][predicted]
//   CorrelationTool              tools.cpp:221-230        per tree pair, the points on which the two trees agree
//   updateMultiHistograms        learning.cpp:960-1012    per leaf and (layer, class): the examples that land there
// Every counter is an integer added with ordinary atomics, so the results do not depend on scheduling.
#include <type_traits>

#include "device_math.h"
#include "forest_tools_host.h"
#include "rvseg_internal.h"
#include "rvseg_kernels.h"

namespace rvseg {

// forest_eval and tools_votes give a point TPP = 2^LOG2_TPP lanes of one wave, so that the dependent walks of its trees
// are in flight together: lane `sub` of the point walks trees sub, sub + TPP, ... and keeps their leaf rows, and the
// lanes of the point then add, class by class, the leaf rows of all trees in tree order.  Their three shared pieces:

// findLeafNode over the 16-byte nodes (one dwordx4 load per visited node): the leaf row of x in the tree at `root`
__device__ __forceinline__ int walk_to_leaf_row(const int4* __restrict__ nodes, int root, const float* __restrict__ x) {
    int4 nd = nodes[root];
    while (nd.z != 0) {
        const float v = x[nd.x];
        nd = nodes[(v < __int_as_float(nd.y)) ? nd.z : nd.z + 1];
    }
    return nd.w;
}

// The leaf rows of a lane's trees: slot k is tree sub + k * TPP (kMaxTrees = 64 trees at most).  Written and read by
// unrolled selects, so that the list stays in registers: a dynamically indexed array would go to scratch memory.
template <int TPP>
struct LeafRows {
    static constexpr int SLOTS = 64 / TPP;
    int row[SLOTS] = {};
    __device__ __forceinline__ void put(int slot, int r) {
#pragma unroll
        for (int q = 0; q < SLOTS; q++) if (q == slot) row[q] = r;
    }
    __device__ __forceinline__ int get(int slot) const {
        int r = 0;
#pragma unroll
        for (int q = 0; q < SLOTS; q++) if (q == slot) r = row[q];
        return r;
    }
};

// Column `col` of the leaf rows of the lane's point, summed over trees 0..T-1 in the reference's order: tree t's row is
// in slot t / TPP of lane t % TPP of the point's lanes, which start at lane_base.  Every lane of the wave takes part in
// the shuffle (the slot is uniform over the wave); a lane without a column (`live` false) loads nothing.
template <int LOG2_TPP>
__device__ __forceinline__ float tree_order_sum(const LeafRows<(1 << LOG2_TPP)>& rows, int n_trees, int lane_base,
                                                const float* __restrict__ hist, int S, int col, bool live) {
    constexpr int TPP = 1 << LOG2_TPP;
    float acc = 0.f;
    for (int t = 0; t < n_trees; t++) {
        const int row = __shfl(rows.get(t >> LOG2_TPP), lane_base + (t & (TPP - 1)), 64);
        if (live) {
            const float h = hist[(size_t)row * S + col];
            acc = (t == 0) ? h : acc + h;
        }
    }
    return acc;
}

constexpr int POINTS_BLOCK = 256;

// 4 lanes per point up to four trees, 16 from five: launch(LOG2_TPP as an integral constant, the grid of n points)
template <class Launch>
void launch_lanes_per_point(int n_trees, int n, Launch launch) {
    const auto grid = [n](int log2_tpp) { return dim3((unsigned)((((long)n << log2_tpp) + POINTS_BLOCK - 1) / POINTS_BLOCK)); };
    if (n_trees <= 4) launch(std::integral_constant<int, 2>(), grid(2));
    else launch(std::integral_constant<int, 4>(), grid(4));
}

// ---------------------------------------------------------------------------------------------
// forest_eval: the P x S posterior sums of P points (rvseg_forest_eval): class c of a point is summed by lane c % TPP.
// ---------------------------------------------------------------------------------------------
template <int LOG2_TPP>
__global__ void __launch_bounds__(POINTS_BLOCK)
forest_eval_kernel(const DeviceNode* __restrict__ nodes, const int32_t* __restrict__ roots, const float* __restrict__ hist, int n_trees,
                   int S, const float* __restrict__ X, int P, int D, float* __restrict__ out) {
    constexpr int TPP = 1 << LOG2_TPP;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int point = gid >> LOG2_TPP;
    const int sub = gid & (TPP - 1);
    const bool active = point < P;
    const float* x = X + (size_t)(active ? point : 0) * D;
    const int4* np = reinterpret_cast<const int4*>(nodes);
    LeafRows<TPP> rows;
    int n_mine = 0;
    for (int t = sub; t < n_trees; t += TPP) rows.put(n_mine++, active ? walk_to_leaf_row(np, roots[t], x) : 0);
    const int lane_base = (threadIdx.x & 63) & ~(TPP - 1);
    for (int c0 = 0; c0 < S; c0 += TPP) {
        const int c = c0 + sub;
        const float acc = tree_order_sum<LOG2_TPP>(rows, n_trees, lane_base, hist, S, c, c < S);
        if (active && c < S) out[(size_t)point * S + c] = acc;
    }
}

void launch_forest_eval(const DeviceForest& f, const float* d_X, int P, int D, float* d_out, hipStream_t s) {
    if (P <= 0) return;
    launch_lanes_per_point(f.n_trees, P, [&](auto log2_tpp, dim3 grid) {
        forest_eval_kernel<decltype(log2_tpp)::value><<<grid, dim3(POINTS_BLOCK), 0, s>>>(
            f.nodes.as<DeviceNode>(), f.roots.as<int32_t>(), f.hist.as<float>(), f.n_trees, f.sum_classes, d_X, P, D, d_out);
    });
    RV_LAUNCHED("forest_eval_kernel");
}

// ---------------------------------------------------------------------------------------------
// tools_votes: the lane that walked tree t writes the point's leaf row and, through the per-leaf vote table, the tree's
// vote; the lanes of a point then reduce the sums of the layer's classes with the label rule.
// ---------------------------------------------------------------------------------------------
template <int LOG2_TPP>
__global__ void __launch_bounds__(POINTS_BLOCK)
tools_votes_kernel(const DeviceNode* __restrict__ nodes, const int32_t* __restrict__ roots, const float* __restrict__ hist,
                   const uint8_t* __restrict__ vote_table, int n_trees, int S, int layer_off, int C,
                   const float* __restrict__ X, int n, int D, size_t stride,
                   int32_t* __restrict__ rows_out, uint8_t* __restrict__ votes_out, int32_t* __restrict__ pred_out) {
    constexpr int TPP = 1 << LOG2_TPP;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int point = gid >> LOG2_TPP;
    const int sub = gid & (TPP - 1);
    const bool active = point < n;
    const float* x = X + (size_t)(active ? point : 0) * D;
    const int4* np = reinterpret_cast<const int4*>(nodes);
    LeafRows<TPP> rows;
    int n_mine = 0;
    for (int t = sub; t < n_trees; t += TPP) {
        int row = 0;
        if (active) {
            row = walk_to_leaf_row(np, roots[t], x);
            if (rows_out) rows_out[t * stride + point] = row;
            if (votes_out) votes_out[t * stride + point] = vote_table[row];
        }
        rows.put(n_mine++, row);
    }
    if (!pred_out) return;   // (uniform over the grid)
    // class c of the layer is summed by lane c % TPP; the lane keeps the first strictly greatest of its classes.  A NaN
    // never wins: it is ranked as -inf, which a non-NaN class 0 ties or beats at the lower index; a NaN in class 0 is
    // never beaten (nan0).
    const int lane_base = (threadIdx.x & 63) & ~(TPP - 1);
    float best = -__builtin_inff();
    int best_c = 0x7fffffff;
    int nan0 = 0;
    for (int c0 = 0; c0 < C; c0 += TPP) {
        const int c = c0 + sub;
        const float acc = tree_order_sum<LOG2_TPP>(rows, n_trees, lane_base, hist, S, layer_off + c, c < C);
        if (c < C) {
            const bool is_nan = acc != acc;
            if (c == 0 && is_nan) nan0 = 1;
            const float v = is_nan ? -__builtin_inff() : acc;
            if (best_c == 0x7fffffff || v > best) { best = v; best_c = c; }
        }
    }
#pragma unroll
    for (int m = 1; m < TPP; m <<= 1) {
        const float ov = __shfl_xor(best, m, 64);
        const int oc = __shfl_xor(best_c, m, 64);
        if (ov > best || (ov == best && oc < best_c)) { best = ov; best_c = oc; }
    }
    nan0 = __shfl(nan0, lane_base, 64);
    if (active && sub == 0) pred_out[point] = nan0 ? 0 : best_c;
}

void launch_tools_votes(const DeviceForest& f, const uint8_t* d_vote_table, int layer_off, int C, const float* d_X, int n, int D,
                        size_t stride, int32_t* d_rows, uint8_t* d_votes, int32_t* d_pred, hipStream_t s) {
    if (n <= 0) return;
    launch_lanes_per_point(f.n_trees, n, [&](auto log2_tpp, dim3 grid) {
        tools_votes_kernel<decltype(log2_tpp)::value><<<grid, dim3(POINTS_BLOCK), 0, s>>>(
            f.nodes.as<DeviceNode>(), f.roots.as<int32_t>(), f.hist.as<float>(), d_vote_table, f.n_trees, f.sum_classes, layer_off, C,
            d_X, n, D, stride, d_rows, d_votes, d_pred);
    });
    RV_LAUNCHED("tools_votes_kernel");
}

// ---------------------------------------------------------------------------------------------
// tools_agree: the votes of a tile of points, [T][AGREE_TILE] bytes, in LDS (rows padded by one word: the lanes of a
// wave read the same word of different rows); thread k of the block owns the pairs k, k + 256, ... of the T (T + 1) / 2
// pairs (t, tt >= t) and counts, four packed votes at a time, where the two rows are equal.  Blocks loop over the
// tiles; a pair's count stays in a register until the block adds it, once, to the pair's 64-bit counter.  The tail of
// the last tile is padded with equal bytes in every row and taken off again.  The grid gives a block
// AGREE_TILES_PER_BLOCK tiles to loop over (a full chunk is 32 blocks of 4 tiles), so that its two atomic adds per pair
// are shared by 2048 points, and is capped at what the device holds.
// ---------------------------------------------------------------------------------------------
constexpr int AGREE_TILE = 512;                    // points per tile
constexpr int AGREE_ROW = AGREE_TILE / 4 + 1;      // words per LDS row
constexpr int AGREE_TILES_PER_BLOCK = 4;
constexpr int AGREE_PAIRS = (kMaxTrees * (kMaxTrees + 1) / 2 + 255) / 256;   // pairs per thread, at most

__global__ void __launch_bounds__(256)
tools_agree_kernel(const uint8_t* __restrict__ votes, int n_trees, int n, int stride, int n_tiles,
                   unsigned long long* __restrict__ agree) {
    extern __shared__ __attribute__((aligned(16))) uint32_t agree_tile[];   // [n_trees][AGREE_ROW]
    const int n_pairs = n_trees * (n_trees + 1) / 2;
    int pair_tt[AGREE_PAIRS];   // t | tt << 8, or -1
    unsigned acc[AGREE_PAIRS];
#pragma unroll
    for (int k = 0; k < AGREE_PAIRS; k++) {
        acc[k] = 0u;
        int rem = (int)threadIdx.x + k * 256, t = 0;
        if (rem < n_pairs) {
            while (rem >= n_trees - t) { rem -= n_trees - t; t++; }
            pair_tt[k] = t | ((t + rem) << 8);
        } else {
            pair_tt[k] = -1;
        }
    }
    unsigned padded = 0u;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int first = tile * AGREE_TILE;
        __syncthreads();   // the previous tile has been read
        for (int i = threadIdx.x; i < n_trees * (AGREE_TILE / 4); i += 256) {
            const int t = i / (AGREE_TILE / 4), w = i - t * (AGREE_TILE / 4);
            const int p = first + 4 * w;
            uint32_t v = 0u;
            if (p + 3 < n) {
                v = *reinterpret_cast<const uint32_t*>(votes + (size_t)t * stride + p);   // stride and first are multiples of 4
            } else {
                for (int b = 0; b < 4; b++)
                    if (p + b < n) v |= (uint32_t)votes[(size_t)t * stride + p + b] << (8 * b);
            }
            agree_tile[t * AGREE_ROW + w] = v;
        }
        __syncthreads();
        if (first + AGREE_TILE > n) padded += (unsigned)(first + AGREE_TILE - n);
#pragma unroll
        for (int k = 0; k < AGREE_PAIRS; k++) {
            if (pair_tt[k] < 0) continue;
            const uint32_t* a = agree_tile + (pair_tt[k] & 255) * AGREE_ROW;
            const uint32_t* b = agree_tile + (pair_tt[k] >> 8) * AGREE_ROW;
            unsigned differ = 0u;
            for (int w = 0; w < AGREE_TILE / 4; w++) {
                uint32_t m = a[w] ^ b[w];   // bit 0 of every byte <- any bit of the byte
                m |= m >> 1; m |= m >> 2; m |= m >> 4;
                differ += __popc(m & 0x01010101u);
            }
            acc[k] += (unsigned)AGREE_TILE - differ;
        }
    }
#pragma unroll
    for (int k = 0; k < AGREE_PAIRS; k++) {
        if (pair_tt[k] < 0) continue;
        const unsigned long long cnt = (unsigned long long)(acc[k] - padded);
        if (cnt == 0ull) continue;
        const int t = pair_tt[k] & 255, tt = pair_tt[k] >> 8;
        atomicAdd(&agree[(size_t)t * n_trees + tt], cnt);
        if (tt != t) atomicAdd(&agree[(size_t)tt * n_trees + t], cnt);
    }
}

void launch_tools_agree(const uint8_t* d_votes, int n_trees, int n, int stride, int max_blocks, unsigned long long* d_agree, hipStream_t s) {
    if (n <= 0) return;
    const int n_tiles = (n + AGREE_TILE - 1) / AGREE_TILE;
    const int want = (n_tiles + AGREE_TILES_PER_BLOCK - 1) / AGREE_TILES_PER_BLOCK;
    const int grid = looping_grid(want, max_blocks);
    tools_agree_kernel<<<dim3((unsigned)grid), dim3(256), (size_t)n_trees * AGREE_ROW * sizeof(uint32_t), s>>>(d_votes, n_trees, n, stride,
                                                                                                            n_tiles, d_agree);
    RV_LAUNCHED("tools_agree_kernel");
}

// ---------------------------------------------------------------------------------------------
// tools_confusion: C x C 32-bit counters in LDS per block (C <= 64 by the loader's limit), flushed once to the 64-bit
// counters.  A label outside [0, C) raises the flag word and is not counted.  A block loops over CONF_ROUNDS groups of
// 256 points, so that its flush of up to C x C atomics is shared by 2048 points.
// ---------------------------------------------------------------------------------------------
constexpr int CONF_ROUNDS = 8;

__global__ void __launch_bounds__(256)
tools_confusion_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ pred, int n, int C,
                       unsigned long long* __restrict__ confusion, int* __restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) uint32_t conf_lds[];   // [C][C]
    for (int i = threadIdx.x; i < C * C; i += 256) conf_lds[i] = 0u;
    __syncthreads();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int t = labels[i], p = pred[i];
        if (t < 0 || t >= C) { atomicOr(flag, 1); continue; }
        atomicAdd(&conf_lds[t * C + p], 1u);   // (p is the kernel's own label of the layer: in range)
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += 256)
        if (conf_lds[i]) atomicAdd(&confusion[i], (unsigned long long)conf_lds[i]);
}

void launch_tools_confusion(const int32_t* d_labels, const int32_t* d_pred, int n, int C, int max_blocks, unsigned long long* d_confusion,
                            int* d_flag, hipStream_t s) {
    if (n <= 0) return;
    const int want = (n + 256 * CONF_ROUNDS - 1) / (256 * CONF_ROUNDS);
    const int grid = looping_grid(want, max_blocks);
    tools_confusion_kernel<<<dim3((unsigned)grid), dim3(256), (size_t)C * C * sizeof(uint32_t), s>>>(d_labels, d_pred, n, C, d_confusion, d_flag);
    RV_LAUNCHED("tools_confusion_kernel");
}

// ---------------------------------------------------------------------------------------------
// tools_refit_count: one thread per (tree, point): counts[leaf row][class offset of layer + label] += 1 for every
// label layer of the example.  A label outside its layer's range raises the flag word and is not counted.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
tools_refit_count_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ labels, int n_trees, int n, int stride,
                         RefitLayers lay, uint32_t* __restrict__ counts, int* __restrict__ flag) {
    const long total = (long)n_trees * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int t = (int)(i / n), p = (int)(i - (long)t * n);
        const int row = rows[(size_t)t * stride + p];
        for (int l = 0; l < lay.n_layers; l++) {
            const int lab = labels[(size_t)p * lay.n_layers + l];
            if (lab < 0 || lab >= lay.class_counts[l]) { atomicOr(flag, 1); continue; }
            atomicAdd(&counts[(size_t)row * lay.sum_classes + lay.offset[l] + lab], 1u);
        }
    }
}

void launch_tools_refit_count(const int32_t* d_rows, const int32_t* d_labels, int n_trees, int n, int stride, const RefitLayers& lay,
                              int max_blocks, uint32_t* d_counts, int* d_flag, hipStream_t s) {
    if (n <= 0) return;
    const long want = ((long)n_trees * n + 255) / 256;
    const int grid = looping_grid(want, max_blocks);
    tools_refit_count_kernel<<<dim3((unsigned)grid), dim3(256), 0, s>>>(d_rows, d_labels, n_trees, n, stride, lay, d_counts, d_flag);
    RV_LAUNCHED("tools_refit_count_kernel");
}

}  // namespace rvseg
