// Device functions of one pairwise term at one (point, class): the slice of the blurred lattice values and the label
// compatibility.  Shared by the mean field's slice / term update (kernels_meanfield.hip) and by the model kernels
// (kernels_crf_model.hip), so that all of them round alike.
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

}  // namespace rvseg
