// Device functions of one pairwise term at one (point, class): the slice of the blurred lattice values and the label
// compatibility.  Shared by the mean field's slice / term update (kernels_meanfield.hip) and by the model kernels
// (kernels_crf_model.hip, kernels_crf_learn.hip), so that all of them round alike.  Also the block sum of their double
// reductions.
#pragma once
#include "rvseg_crf.h"

namespace rvseg {

// slice (permutohedral.cpp:574-584 sseCompute / :515-524 seqCompute) of class c at point p
template <bool SEQ>
__device__ __forceinline__ float term_slice(const LatticeDev& L, int C, const float* __restrict__ values, float alpha, long long p, int c) {
    const int dp1 = L.d + 1;
    float acc = 0.0f;
    for (int j = 0; j < dp1; j++) {
        const int o = lattice_vertex(L, p, dp1, j);
        const float bw = L.bary[p * dp1 + j];
        const float val = values[(size_t)o * C + c];
        if (SEQ) {
            const float t = bw * val;
            const float u = t * alpha;
            acc += u;
        } else {
            const float w = bw * alpha;
            const float prod = w * val;
            acc += prod;
        }
    }
    return acc;
}

// Diagonal fl(v[c] * t) (labelcompatibility.cpp:66; Potts(w) is Diagonal(-w, .., -w), :47) or symmetric Matrix
// sum_c' W[c'][c] * r[c'] from c' = 0 up, separately rounded (:85); wt: the compatibility, r: the point's C filtered values
__device__ __forceinline__ float term_compat(bool matrix, const float* wt, const float* r, int C, int c, float t) {
    if (!matrix) return wt[c] * t;
    float out = wt[c] * r[0];
    for (int k = 1; k < C; k++) {
        const float m = wt[k * C + c] * r[k];
        out = out + m;
    }
    return out;
}

// ---- fixed-order double reductions of the model kernels (kernels_crf_model.hip, kernels_crf_learn.hip) ----
constexpr int KL_THREADS = 256;

// the 64 lanes of a wave, in the fixed order of the xor butterfly (every lane ends with the same sum)
__device__ __forceinline__ double kl_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// block sum of one double per thread into *out (thread 0 writes): waves 0..3 added in order
__device__ __forceinline__ void kl_block_sum(double v, double* sh /* 4 */, double* out) {
    const double w = kl_wave_sum(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();   // sh may still be read by the previous part's thread 0
    if ((threadIdx.x & 63) == 0) sh[wave] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = sh[0];
        for (int k = 1; k < KL_THREADS / 64; k++) r = r + sh[k];
        *out = r;
    }
}

}  // namespace rvseg
