// DenseCRF mean-field kernels for gfx950: blur, slice, softmax, fused update, general terms, kernel parameters, logistic unary.
//
// Reference semantics (third-party/densecrf/src):
//   sseCompute / seqCompute           permutohedral.cpp:476-589   (blur over d+1 axes, slice)
//   DenseKernel::initLattice/filter   pairwise.cpp:40-80          (symmetric normalisation)
//   PottsCompatibility::apply         labelcompatibility.cpp:46-48
//   expAndNormalize, inference        densecrf.cpp:98-131
#include <type_traits>

#include "device_math.h"
#include "rvseg_crf.h"
#include "term_device.h"

namespace rvseg {

// ---------------------------------------------------------------------------------------------
// blur along one lattice axis (permutohedral.cpp:556-569 / :496-510)
// ---------------------------------------------------------------------------------------------
template <bool SEQ>
__global__ void __launch_bounds__(256)
blur_kernel(LatticeDev L, int axis, int C, const float* __restrict__ old_v, float* __restrict__ new_v) {
    if (L.counters[1]) return;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int M = L.counters[0] < L.m_bound ? L.counters[0] : L.m_bound;
    if (gid >= (long long)M * C) return;
    const int v = (int)(gid / C), c = (int)(gid - (long long)v * C);
    const int n1 = L.nb1[(size_t)axis * L.m_bound + v], n2 = L.nb2[(size_t)axis * L.m_bound + v];
    const float a = n1 >= 0 ? old_v[(size_t)n1 * C + c] : 0.0f;
    const float b = n2 >= 0 ? old_v[(size_t)n2 * C + c] : 0.0f;
    const float o = old_v[gid];
    if (SEQ) {
        new_v[gid] = (float)((double)o + 0.5 * (double)(a + b));  // seqCompute :505
    } else {
        const float sum = a + b;
        const float h = 0.5f * sum;
        new_v[gid] = o + h;                                        // sseCompute :566
    }
}

// All d+1 axis passes of one frame in one block: the frame's vertex values (M_f x C, ~10 KB for the
// Segmenter kernel) ping-pong between two LDS tables, so a filter costs one launch instead of d+1
// launch-latency-bound ones.  Frames whose values do not fit go through global memory, still inside
// the block (a vertex's neighbours belong to its own frame).  The result lands in `b`.
constexpr int BLUR_LDS_FLOATS = 6144;   // per table

template <bool SEQ>
__global__ void __launch_bounds__(1024)
blur_frames_kernel(LatticeDev L, int C, int reverse, float* __restrict__ a, float* __restrict__ b) {
    __shared__ float tab[2][BLUR_LDS_FLOATS];
    if (L.counters[1]) return;
    const int frame = blockIdx.x;
    const int M = L.counters[0] < L.m_bound ? L.counters[0] : L.m_bound;
    const int2 fr = lattice_frame_range(L, frame, M);
    const int f0 = fr.x, n = (fr.y - fr.x) * C;
    const bool lds = n <= BLUR_LDS_FLOATS;
    float* ga = a + (size_t)f0 * C;
    float* gb = b + (size_t)f0 * C;
    if (lds) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) tab[0][i] = ga[i];
        __syncthreads();
    }
    int cur = 0;
    for (int t = 0; t <= L.d; t++) {
        const int axis = reverse ? L.d - t : t;
        const int* n1p = L.nb1 + (size_t)axis * L.m_bound + f0;
        const int* n2p = L.nb2 + (size_t)axis * L.m_bound + f0;
        const float* old_v = lds ? tab[cur] : (cur ? gb : ga);
        float* new_v = lds ? tab[cur ^ 1] : (cur ? ga : gb);
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int v = i / C, c = i - v * C;
            const int n1 = n1p[v], n2 = n2p[v];
            const float x = n1 >= 0 ? old_v[(n1 - f0) * C + c] : 0.0f;
            const float y = n2 >= 0 ? old_v[(n2 - f0) * C + c] : 0.0f;
            const float o = old_v[i];
            if (SEQ) {
                new_v[i] = (float)((double)o + 0.5 * (double)(x + y));  // seqCompute :505
            } else {
                const float sum = x + y;
                const float h = 0.5f * sum;
                new_v[i] = o + h;                                        // sseCompute :566
            }
        }
        __syncthreads();   // block-wide: also orders the global-memory path (one block owns the frame)
        cur ^= 1;
    }
    if (lds) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) gb[i] = tab[cur][i];
    } else if (cur == 0) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) gb[i] = ga[i];
    }
}

// runs the d+1 axis passes; returns the buffer that holds the result
float* launch_blur(const LatticeDev& L, int C, bool seq, bool reverse, float* a, float* b, hipStream_t s, bool small_blocks) {
    // small_blocks: the pass runs beside the feature kernels (lattice build on the side stream) and a
    // 1024-thread block would wait for a whole free CU
    if (L.cap_f_mask + 1 <= 8192u) {   // at most 4096 vertices per frame: one block per frame is enough
        if (seq) blur_frames_kernel<true><<<dim3((unsigned)L.n_frames), dim3(small_blocks ? 256 : 1024), 0, s>>>(L, C, reverse ? 1 : 0, a, b);
        else blur_frames_kernel<false><<<dim3((unsigned)L.n_frames), dim3(small_blocks ? 256 : 1024), 0, s>>>(L, C, reverse ? 1 : 0, a, b);
        RV_LAUNCHED("blur_frames_kernel");
        return b;
    }
    const long long total = (long long)L.m_bound * C;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    float *cur = a, *nxt = b;
    for (int t = 0; t <= L.d; t++) {
        const int axis = reverse ? L.d - t : t;
        if (seq) blur_kernel<true><<<grid, block, 0, s>>>(L, axis, C, cur, nxt);
        else blur_kernel<false><<<grid, block, 0, s>>>(L, axis, C, cur, nxt);
        float* tmp = cur; cur = nxt; nxt = tmp;
    }
    RV_LAUNCHED("blur_kernel");
    return cur;
}

// ---------------------------------------------------------------------------------------------
// slice (permutohedral.cpp:574-584 / :515-524), one thread per (point, class)
//   OUT_MODE 0: out[p][c] = sliced                      (plain filter, rvseg_lattice_filter)
//   OUT_MODE 1: norm[p]   = 1/sqrt(sliced + 1e-20)      (normaliser, pairwise.cpp:55-56; C == 1)
//   OUT_MODE 2: tmp[p][c] = tmp[p][c] - (-w) * (sliced * norm[p])   (filter + Potts + inference)
//   OUT_MODE 3: norm[p]   = 1/(sliced + 1e-20)          (NORMALIZE_BEFORE / _AFTER normaliser, pairwise.cpp:51-53; C == 1)
// ---------------------------------------------------------------------------------------------
template <bool SEQ, int OUT_MODE>
__global__ void __launch_bounds__(256)
slice_kernel(LatticeDev L, int C, const float* __restrict__ values, float alpha, float neg_w, float* __restrict__ out,
             long long n_points) {
    if (L.counters[1]) return;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_points * C) return;
    const long long p = gid / C;
    const int c = (int)(gid - p * C);
    const float acc = term_slice<SEQ>(L, C, values, alpha, p, c);
    if (OUT_MODE == 0) {
        out[gid] = acc;
    } else if (OUT_MODE == 1) {
        out[gid] = (float)(1.0 / sqrt((double)acc + 1e-20));
    } else if (OUT_MODE == 3) {
        out[gid] = (float)(1.0 / ((double)acc + 1e-20));
    } else {
        const float t = acc * L.norm[p];   // out = out*norm_.asDiagonal(), pairwise.cpp:79
        const float m = neg_w * t;         // out = -w_*Q, labelcompatibility.cpp:47
        out[gid] = out[gid] - m;           // tmp1 -= tmp2, densecrf.cpp:126
    }
}

// The normaliser's slice (C == 1, seqCompute rounding, OUT_MODE 1; RECIP: OUT_MODE 3) with the d+1 offsets and weights
// of a point fetched as two wide rows.
// NARROW (LatticeDev::ids16, DP1 == 7): 16-bit ids local to the point's frame.
template <int DP1, bool RECIP = false, bool NARROW = false>
__global__ void __launch_bounds__(256)
slice_norm_kernel(LatticeDev L, const float* __restrict__ values, float alpha, float* __restrict__ out, long long n_points) {
    if (L.counters[1]) return;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_points) return;
    int offs[DP1];
    float wts[DP1];
    if constexpr (NARROW) {
        unsigned raw[4];
        load_ids16(L.offsets, (size_t)p, raw);
        values += L.fstart[p / L.N];
        unpack_ids16(raw, (size_t)p, offs);
    } else {
        load_row<DP1>(L.offsets + p * DP1, offs);
    }
    load_row<DP1>(L.bary + p * DP1, wts);
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < DP1; j++) {
        const float t = wts[j] * values[offs[j]];
        const float u = t * alpha;   // seqCompute :520
        acc += u;
    }
    if (RECIP) out[p] = (float)(1.0 / ((double)acc + 1e-20));   // pairwise.cpp:51-53
    else out[p] = (float)(1.0 / sqrt((double)acc + 1e-20));      // pairwise.cpp:55-56
}

void launch_slice(const LatticeDev& L, int C, bool seq, int out_mode, const float* values, float neg_w, float* out,
                  long long n_points, hipStream_t s) {
    const float alpha = lattice_alpha(L.d);  // permutohedral.cpp:571
    if (seq && (out_mode == 1 || out_mode == 3) && C == 1 && (L.d == 6 || L.d == 5 || L.d == 2)) {
        const dim3 g1((unsigned)((n_points + 255) / 256)), b1(256);
        auto norm = [&](auto recip) {
            constexpr bool RECIP = decltype(recip)::value;
            if (L.d == 6 && L.ids16) slice_norm_kernel<7, RECIP, true><<<g1, b1, 0, s>>>(L, values, alpha, out, n_points);
            else if (L.d == 6) slice_norm_kernel<7, RECIP><<<g1, b1, 0, s>>>(L, values, alpha, out, n_points);
            else if (L.d == 5) slice_norm_kernel<6, RECIP><<<g1, b1, 0, s>>>(L, values, alpha, out, n_points);
            else slice_norm_kernel<3, RECIP><<<g1, b1, 0, s>>>(L, values, alpha, out, n_points);
        };
        if (out_mode == 3) norm(std::bool_constant<true>()); else norm(std::bool_constant<false>());
        RV_LAUNCHED("slice_norm_kernel");
        return;
    }
    const long long total = n_points * C;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    auto slice = [&](auto seq_c) {
        constexpr bool SEQ = decltype(seq_c)::value;
        auto mode = [&](auto om) { slice_kernel<SEQ, decltype(om)::value><<<grid, block, 0, s>>>(L, C, values, alpha, neg_w, out, n_points); };
        switch (out_mode) {
            case 0: mode(std::integral_constant<int, 0>()); break;
            case 1: mode(std::integral_constant<int, 1>()); break;
            case 3: mode(std::integral_constant<int, 3>()); break;
            default: mode(std::integral_constant<int, 2>()); break;
        }
    };
    if (seq) slice(std::bool_constant<true>()); else slice(std::bool_constant<false>());
    RV_LAUNCHED("slice_kernel");
}

// ---------------------------------------------------------------------------------------------
// tmp = -U (densecrf.cpp:123) and expAndNormalize (densecrf.cpp:98-106)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
neg_unary_kernel(ValueView unary, int negate, int C, int N, float* __restrict__ tmp, long long n_points) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_points * C) return;
    const long long p = gid / C;
    const int c = (int)(gid - p * C);
    const float u = unary.at((unsigned)p, c, C, N);
    tmp[gid] = negate ? -u : u;
}

void launch_neg_unary(const ValueView& unary, bool negate, int C, int N, float* tmp, long long n_points, hipStream_t s) {
    const long long total = n_points * C;
    neg_unary_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(unary, negate ? 1 : 0, C, N, tmp, n_points);
    RV_LAUNCHED("neg_unary_kernel");
}

__global__ void __launch_bounds__(256)
softmax_kernel(const float* __restrict__ tmp, int C, int N, ValueView q, long long n_points) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_points) return;
    const float* b = tmp + p * C;
    float mx = b[0];
    for (int c = 1; c < C; c++) { const float v = b[c]; if (v > mx) mx = v; }
    float sum = 0.0f;
    for (int c = 0; c < C; c++) {
        const float e = exp_f32_dev(b[c] - mx);
        q.ref((unsigned)p, c, C, N) = e;
        sum += e;
    }
    for (int c = 0; c < C; c++) {
        float& r = q.ref((unsigned)p, c, C, N);
        r = r / sum;
    }
}

void launch_softmax(const float* tmp, int C, int N, const ValueView& q, long long n_points, hipStream_t s) {
    softmax_kernel<<<dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, s>>>(tmp, C, N, q, n_points);
    RV_LAUNCHED("softmax_kernel");
}

// ---------------------------------------------------------------------------------------------
// Fused mean-field update for ONE Potts kernel (the Segmenter's case, segmenter.cpp:641-644):
//   slice (permutohedral.cpp:574-584) -> * norm (pairwise.cpp:79) -> * -w (labelcompatibility.cpp:47)
//   -> tmp1 = -U - tmp2 (densecrf.cpp:123-126) -> expAndNormalize (densecrf.cpp:98-106)
// One thread per point, all C classes in registers.  Vertex ids are frame-contiguous, so a block
// (256 points of one frame) stages that frame's blurred vertex values in LDS when they fit and
// slices from there; otherwise it gathers from HBM/L2.  Same operation order as the unfused
// kernels, so the result is bit-identical.
// ---------------------------------------------------------------------------------------------
constexpr int MF_LDS_BYTES = 24 * 1024;   // frames with more vertices than fit read `values` from L2
constexpr int MF_PTS = 512;               // points per block (2 per thread; 256 / 1024 / 2048 / 4096 measured +0.16 / +0.05 / +0.11 / +0.17 ms per 64-frame step)

// inputs of one point of the update: fetched one point ahead of their use.  NARROW (LatticeDev::ids16, DP1 == 7): the
// ids are the four raw dwords around the point's row of 16-bit frame-local ids, unpacked where they are used
template <int C, int DP1, bool NARROW>
struct MfIn {
    int offs[NARROW ? 4 : (DP1 > 0 ? DP1 : 1)];
    float wts[DP1 > 0 ? DP1 : 1];
    float ur[C];
    float nrm;
};

template <int C, int DP1, bool NARROW>
__device__ __forceinline__ void mf_load(const LatticeDev& L, const ValueView& unary, int f0, size_t p, MfIn<C, DP1, NARROW>& in) {
    if constexpr (NARROW) {
        unsigned raw[4];
        load_ids16(L.offsets, p, raw);
#pragma unroll
        for (int k = 0; k < 4; k++) in.offs[k] = (int)raw[k];
        load_row<DP1>(L.bary + p * DP1, in.wts);
    } else if (DP1 > 0) {
        load_row<(DP1 > 0 ? DP1 : 1)>(L.offsets + p * DP1, in.offs);
        load_row<(DP1 > 0 ? DP1 : 1)>(L.bary + p * DP1, in.wts);
    }
    in.nrm = L.norm[p];
    load_row<C>(unary.base + unary.index((unsigned)p, 0, C, L.N), in.ur);
}

// TERM 0: Potts, t = sliced * norm, out = fl(-w * t) (the Segmenter's update).  TERM 1 / 2 (learned single-term models):
// t = sliced, times norm when `post` (block-uniform); out = Diagonal fl(v[c] * t[c]) / Matrix sum_c' W[c][c'] t[c'] from
// c' = 0 up, with v / W read from `compat` at compile-time offsets (uniform loads).  TERM 0 never reads compat / post,
// TERM 1 / 2 never neg_w.
template <bool SEQ, int C, int DP1, bool USE_LDS, int TERM, bool NARROW>
__device__ __forceinline__ void mf_points(const LatticeDev& L, const float* __restrict__ values, const float* tab, float alpha,
                                          float neg_w, const ValueView& unary, int negate, const ValueView& Q, int scale_out,
                                          const MfLabels& lab, int frame, int f0, int i0,
                                          const float* __restrict__ compat, int post) {
    constexpr int CP = (C + 3) / 4 * 4;
    constexpr int PER_THREAD = MF_PTS / 256;
    const int dp1 = DP1 > 0 ? DP1 : L.d + 1;
    MfIn<C, DP1, NARROW> cur, nxt;
    if (i0 < L.N) mf_load<C, DP1, NARROW>(L, unary, f0, (size_t)frame * L.N + i0, cur);
#pragma unroll
    for (int k = 0; k < PER_THREAD; k++) {   // the staged table serves MF_PTS points
        const int i = i0 + 256 * k;
        if (i >= L.N) break;
        const size_t p = (size_t)frame * L.N + i;
        if (k + 1 < PER_THREAD && i + 256 < L.N) mf_load<C, DP1, NARROW>(L, unary, f0, p + 256, nxt);   // next point's rows travel now
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = 0.0f;
        int loc[7];   // NARROW: the point's frame-local ids
        if constexpr (NARROW) {
            unsigned raw[4];
#pragma unroll
            for (int k = 0; k < 4; k++) raw[k] = (unsigned)cur.offs[k];
            unpack_ids16(raw, p, loc);
        }
#pragma unroll
        for (int j = 0; j < (DP1 > 0 ? DP1 : 8); j++) {
            if (DP1 == 0 && j >= dp1) break;
            // the vertex's row in the staged table, and its global id (the runtime-d form reads either id form)
            const int o = NARROW ? loc[j < 7 ? j : 0] + (USE_LDS ? 0 : f0) : DP1 > 0 ? cur.offs[j] : lattice_vertex(L, (long long)p, dp1, j);
            const float bw = DP1 > 0 ? cur.wts[j] : L.bary[p * dp1 + j];
            float val[C];
            if (USE_LDS) {
                const float* row = tab + (NARROW ? o : o - f0) * CP;
#pragma unroll
                for (int c = 0; c < C; c++) val[c] = row[c];
            } else {
                load_row<C>(values + (size_t)o * C, val);
            }
            if (SEQ) {
#pragma unroll
                for (int c = 0; c < C; c++) { const float t = bw * val[c]; const float u = t * alpha; acc[c] += u; }
            } else {
                const float w = bw * alpha;
#pragma unroll
                for (int c = 0; c < C; c++) { const float prod = w * val[c]; acc[c] += prod; }
            }
        }
        const float nrm = cur.nrm;
        float b[C];
        if (TERM == 0) {
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float t = acc[c] * nrm;
                const float m = neg_w * t;
                const float u = cur.ur[c];
                b[c] = (negate ? -u : u) - m;
            }
        } else {
            float t[C];
#pragma unroll
            for (int c = 0; c < C; c++) t[c] = post ? acc[c] * nrm : acc[c];
#pragma unroll
            for (int c = 0; c < C; c++) {
                float o;
                if (TERM == 1) {
                    o = compat[c] * t[c];
                } else {
                    o = compat[c * C] * t[0];
#pragma unroll
                    for (int k = 1; k < C; k++) {
                        const float m = compat[c * C + k] * t[k];
                        o = o + m;
                    }
                }
                const float u = cur.ur[c];
                b[c] = (negate ? -u : u) - o;
            }
        }
        float mx = b[0];
#pragma unroll
        for (int c = 1; c < C; c++) if (b[c] > mx) mx = b[c];
        float sum = 0.0f;
#pragma unroll
        for (int c = 0; c < C; c++) { b[c] = exp_f32_dev(b[c] - mx); sum += b[c]; }
        const size_t qrow = Q.index((unsigned)p, 0, C, L.N);
#pragma unroll
        for (int c = 0; c < C; c++) b[c] = b[c] / sum;
        if (lab.labels) lab.labels[((size_t)frame * lab.n_layers + lab.layer) * L.N + i] = (int8_t)label_rule(b, C, lab.mode, lab.unknown);
        if (scale_out) {   // not the last iteration: hand the next splat its input Q * norm directly
#pragma unroll
            for (int c = 0; c < C; c++) b[c] = b[c] * nrm;
        }
        store_row<C>(Q.base + qrow, b);
        cur = nxt;
    }
}

// DP1 = d+1 at compile time (wide offset / weight loads), 0 = runtime d.  TERM 0 is the Segmenter's update; the fused
// update of ONE learned term is TERM 1 (Diagonal; Potts with a normalisation other than SYMMETRIC is Diagonal(-w, .., -w))
// or TERM 2 (Matrix), at runtime d.  post: scale the sliced values by norm (SYMMETRIC / AFTER); scale_out: hand the
// next splat Q * norm (SYMMETRIC / BEFORE, not the last iteration).
// NARROW: 16-bit frame-local ids (LatticeDev::ids16; DP1 == 7).
template <bool SEQ, int C, int DP1, int TERM = 0, bool NARROW = false>
__global__ void __launch_bounds__(256)
mf_update_kernel(LatticeDev L, const float* __restrict__ values, float alpha, float neg_w, ValueView unary, int negate,
                 ValueView Q, int scale_out, MfLabels lab, const float* __restrict__ compat, int post) {
    extern __shared__ __attribute__((aligned(16))) float tab[];
    if (L.counters[1]) return;   // uniform: hash overflow (flagged)
    constexpr int CP = (C + 3) / 4 * 4;
    const int bpf = (L.N + MF_PTS - 1) / MF_PTS;
    const int frame = blockIdx.x / bpf;
    const int i0 = (blockIdx.x - frame * bpf) * MF_PTS + threadIdx.x;
    const int f0 = L.fstart[frame], f1 = L.fstart[frame + 1];
    const int Mf = f1 - f0;
    const bool use_lds = (size_t)Mf * CP * sizeof(float) <= (size_t)MF_LDS_BYTES;   // block-uniform
    if (use_lds) {
        for (int idx = threadIdx.x; idx < Mf * C; idx += 256) {
            const int r = idx / C, c = idx - r * C;
            tab[r * CP + c] = values[(size_t)(f0 + r) * C + c];
        }
        __syncthreads();
        mf_points<SEQ, C, DP1, true, TERM, NARROW>(L, values, tab, alpha, neg_w, unary, negate, Q, scale_out, lab, frame, f0, i0, compat, post);
    } else {
        mf_points<SEQ, C, DP1, false, TERM, NARROW>(L, values, tab, alpha, neg_w, unary, negate, Q, scale_out, lab, frame, f0, i0, compat, post);
    }
}

// The class counts with a fused softmax_unary / mf_update instantiation, spelled once: calls
// f(std::integral_constant<int, C>) and returns true for one of them, returns false for any other C.
template <typename F>
static bool with_fused_class_count(int C, F&& f) {
    switch (C) {
        case 2: f(std::integral_constant<int, 2>{}); return true;
        case 3: f(std::integral_constant<int, 3>{}); return true;
        case 4: f(std::integral_constant<int, 4>{}); return true;
        case 5: f(std::integral_constant<int, 5>{}); return true;
        case 6: f(std::integral_constant<int, 6>{}); return true;
        case 7: f(std::integral_constant<int, 7>{}); return true;
        case 8: f(std::integral_constant<int, 8>{}); return true;
        case 9: f(std::integral_constant<int, 9>{}); return true;
        case 10: f(std::integral_constant<int, 10>{}); return true;
        case 12: f(std::integral_constant<int, 12>{}); return true;
        case 16: f(std::integral_constant<int, 16>{}); return true;
        case 21: f(std::integral_constant<int, 21>{}); return true;
        default: return false;
    }
}

bool mf_fused_supported(int C) { return with_fused_class_count(C, [](auto) {}); }

// returns false when C has no fused instantiation (the caller then runs the unfused kernels)
bool launch_mf_update(const LatticeDev& L, int C, const float* values, const MfTerm& term, const ValueView& unary, bool negate,
                      const ValueView& Q, bool scale_out, const MfLabels& lab, hipStream_t s) {
    const float alpha = lattice_alpha(L.d);
    const int bpf = (L.N + MF_PTS - 1) / MF_PTS;
    const dim3 grid((unsigned)(bpf * L.n_frames)), block(256);
    const int neg = negate ? 1 : 0, so = scale_out ? 1 : 0;
    const int post = term.post ? 1 : 0;
    return with_fused_class_count(C, [&](auto cc) {
        constexpr int CC = decltype(cc)::value;
        constexpr bool SEQ = CC <= 2;   // Permutohedral::compute dispatch, permutohedral.cpp:600-603
        if (!term.compat && L.d == 6 && L.ids16) mf_update_kernel<SEQ, CC, 7, 0, true><<<grid, block, MF_LDS_BYTES, s>>>(L, values, alpha, term.neg_w, unary, neg, Q, so, lab, term.compat, post);
        else if (!term.compat && L.d == 6) mf_update_kernel<SEQ, CC, 7><<<grid, block, MF_LDS_BYTES, s>>>(L, values, alpha, term.neg_w, unary, neg, Q, so, lab, term.compat, post);
        else if (!term.compat) mf_update_kernel<SEQ, CC, 0><<<grid, block, MF_LDS_BYTES, s>>>(L, values, alpha, term.neg_w, unary, neg, Q, so, lab, term.compat, post);
        else if (term.matrix) mf_update_kernel<SEQ, CC, 0, 2><<<grid, block, MF_LDS_BYTES, s>>>(L, values, alpha, term.neg_w, unary, neg, Q, so, lab, term.compat, post);
        else mf_update_kernel<SEQ, CC, 0, 1><<<grid, block, MF_LDS_BYTES, s>>>(L, values, alpha, term.neg_w, unary, neg, Q, so, lab, term.compat, post);
        RV_LAUNCHED("mf_update_kernel");
    });
}

// Q0 = expAndNormalize(-U) straight from the unary (densecrf.cpp:120), one thread per point
// scale != nullptr: store fl(Q * scale[p]) instead of Q -- the input of the next splat
// (DenseKernel::filter, pairwise.cpp:66), so the splat needs no per-entry normaliser
template <int C>
__global__ void __launch_bounds__(256)
softmax_unary_kernel(ValueView unary, int negate, int N, ValueView q, long long n_points, const float* __restrict__ scale) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_points) return;
    const size_t urow = unary.index((unsigned)p, 0, C, N);
    float b[C];
    load_row<C>(unary.base + urow, b);
#pragma unroll
    for (int c = 0; c < C; c++) b[c] = negate ? -b[c] : b[c];
    float mx = b[0];
#pragma unroll
    for (int c = 1; c < C; c++) if (b[c] > mx) mx = b[c];
    float sum = 0.0f;
#pragma unroll
    for (int c = 0; c < C; c++) { b[c] = exp_f32_dev(b[c] - mx); sum += b[c]; }
    const size_t qrow = q.index((unsigned)p, 0, C, N);
#pragma unroll
    for (int c = 0; c < C; c++) b[c] = b[c] / sum;
    if (scale) {
        const float sc = scale[p];
#pragma unroll
        for (int c = 0; c < C; c++) b[c] = b[c] * sc;
    }
    store_row<C>(q.base + qrow, b);
}

bool launch_softmax_unary(const ValueView& unary, bool negate, int C, int N, const ValueView& q, long long n_points,
                          const float* scale, hipStream_t s) {
    const dim3 grid((unsigned)((n_points + 255) / 256)), block(256);
    return with_fused_class_count(C, [&](auto cc) {
        softmax_unary_kernel<decltype(cc)::value><<<grid, block, 0, s>>>(unary, negate ? 1 : 0, N, q, n_points, scale);
        RV_LAUNCHED("softmax_unary_kernel");
    });
}

__global__ void __launch_bounds__(256)
fill_int_kernel(int* p, int v, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

void launch_fill_int(int* p, int v, long long n, hipStream_t s) {
    if (n <= 0) return;
    fill_int_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(p, v, n);
    RV_LAUNCHED("fill_int_kernel");
}

// ---------------------------------------------------------------------------------------------
// General pairwise term of DenseCRF::inference (densecrf.cpp:123-126) for any compatibility and normalisation:
//   t      = sliced (permutohedral.cpp:574-584 / :515-524), times norm[p] when `post` (DenseKernel::filter, pairwise.cpp:77-79)
//   out[c] = Diagonal: fl(v[c] * t[c])      (labelcompatibility.cpp:66; Potts(w) is Diagonal(-w, .., -w), :47)
//            Matrix:   sum_c' W[c][c'] * t[c'], from c' = 0 up, separately rounded (:85; W symmetric, :79)
//   tmp[p][c] -= out[c]                      (densecrf.cpp:126); ASSIGN: tmp[p][c] = out[c] (DenseKernel::apply alone)
// A block stages the compatibility once (C x C floats at most: 16 KB) and walks groups of PB = 256 / C points; thread
// (lp, c) slices class c of point lp.  A Matrix needs all C sliced values of a point: they meet in an LDS row.  W is
// read as W[c'][c] (= W[c][c'], symmetric), so the lanes of a wave read consecutive LDS banks.
// ---------------------------------------------------------------------------------------------
constexpr int TERM_THREADS = 256;

template <bool SEQ, bool ASSIGN>
__global__ void __launch_bounds__(TERM_THREADS)
term_update_kernel(LatticeDev L, int C, const float* __restrict__ values, float alpha, int post, int matrix,
                   const float* __restrict__ compat, float* __restrict__ tmp, long long n_points) {
    __shared__ float wt[64 * 64];
    __shared__ float rows[TERM_THREADS];
    if (L.counters[1]) return;   // uniform: hash overflow (flagged)
    const int n_w = matrix ? C * C : C;
    for (int i = threadIdx.x; i < n_w; i += TERM_THREADS) wt[i] = compat[i];
    __syncthreads();
    const int PB = TERM_THREADS / C;
    const int lp = threadIdx.x / C, c = threadIdx.x - lp * C;
    for (long long p0 = (long long)blockIdx.x * PB; p0 < n_points; p0 += (long long)gridDim.x * PB) {   // block-uniform
        const long long p = p0 + lp;
        const bool live = lp < PB && p < n_points;
        float t = 0.0f;
        if (live) {
            const float acc = term_slice<SEQ>(L, C, values, alpha, p, c);
            t = post ? acc * L.norm[p] : acc;
        }
        if (matrix) {
            rows[threadIdx.x] = t;
            __syncthreads();
        }
        if (live) {
            const float out = term_compat(matrix != 0, wt, rows + lp * C, C, c, t);
            const size_t g = (size_t)p * C + c;
            tmp[g] = ASSIGN ? out : tmp[g] - out;
        }
        if (matrix) __syncthreads();   // the row is rewritten by the next group
    }
}

void launch_term_update(const LatticeDev& L, int C, bool seq, const float* values, bool post, bool matrix, const float* compat,
                        float* tmp, long long n_points, hipStream_t s, bool assign) {
    const float alpha = lattice_alpha(L.d);
    const int PB = TERM_THREADS / C;
    long long blocks = (n_points + PB - 1) / PB;
    if (blocks > 4096) blocks = 4096;   // each block loads the compatibility once
    const dim3 grid((unsigned)blocks), block(TERM_THREADS);
#define RV_TERM(SEQ, ASSIGN) term_update_kernel<SEQ, ASSIGN><<<grid, block, 0, s>>>(L, C, values, alpha, post ? 1 : 0, matrix ? 1 : 0, compat, tmp, n_points)
    if (seq) { if (assign) RV_TERM(true, true); else RV_TERM(true, false); }
    else { if (assign) RV_TERM(false, true); else RV_TERM(false, false); }
#undef RV_TERM
    RV_LAUNCHED("term_update_kernel");
}

// ---------------------------------------------------------------------------------------------
// Kernel parameters of a term (DenseKernel::setParameters, pairwise.cpp:140-152), one point per thread, d <= 7:
//   kind 1 (DIAG): f'[j] = fl(p[j] * f[j])
//   kind 2 (FULL): f'[a] = sum_b P[a][b] * f[b], b from 0 up; P column-major: P[a][b] = p[b * d + a] (the resize of :147)
// ---------------------------------------------------------------------------------------------
template <int D>   // feature dimension at compile time: the row stays in registers
__global__ void __launch_bounds__(256)
kernel_params_kernel(const float* __restrict__ f, int N, int kind, KernelParams kp, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float x[D], y[D];
#pragma unroll
    for (int j = 0; j < D; j++) x[j] = f[i * D + j];
#pragma unroll
    for (int a = 0; a < D; a++) {
        if (kind == 1) {
            y[a] = kp.p[a] * x[a];
        } else {
            float r = kp.p[a] * x[0];
#pragma unroll
            for (int b = 1; b < D; b++) {
                const float m = kp.p[b * D + a] * x[b];
                r = r + m;
            }
            y[a] = r;
        }
    }
#pragma unroll
    for (int a = 0; a < D; a++) out[i * D + a] = y[a];
}

void launch_kernel_params(const float* f, int N, int d, int kind, const KernelParams& kp, float* out, hipStream_t s) {
    const dim3 grid((unsigned)((N + 255) / 256)), block(256);
    with_dimension(d, [&](auto dim) { kernel_params_kernel<decltype(dim)::value><<<grid, block, 0, s>>>(f, N, kind, kp, out); });
    RV_LAUNCHED("kernel_params_kernel");
}

// ---------------------------------------------------------------------------------------------
// LogisticUnaryEnergy::get (unary.cpp:50-52): U[i][m] = sum_k L[m][k] * f[i][k], k from 0 up, one point per thread.
// L (C x K row-major) is the same for every lane: uniform loads.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
logistic_unary_kernel(const float* __restrict__ Lm, const float* __restrict__ f, int N, int C, int K, float* __restrict__ U) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float* fi = f + i * K;
    for (int m = 0; m < C; m++) {
        const float* lr = Lm + (size_t)m * K;
        float acc = lr[0] * fi[0];
        for (int k = 1; k < K; k++) {
            const float prod = lr[k] * fi[k];
            acc = acc + prod;
        }
        U[i * C + m] = acc;
    }
}

void launch_logistic_unary(const float* Lm, const float* f, int N, int C, int K, float* U, hipStream_t s) {
    logistic_unary_kernel<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s>>>(Lm, f, N, C, K, U);
    RV_LAUNCHED("logistic_unary_kernel");
}

}  // namespace rvseg
