// Kernels of a kept DenseCRF model (rvseg_crf_model_*) for gfx950: one-hot beliefs and per-point energies
// (DenseCRF::unaryEnergy / pairwiseEnergy, densecrf.cpp:141-177) and the KL divergence (densecrf.cpp:214-235).
//
// KL, per element and in double from fp32 inputs:
//   entropy  e   = q * log(max(q, 1e-20f))
//   unary    u   = U * q                       (U: the energy)
//   term k   p_k = q * a_k                     (a_k: the fp32 value of the term's apply, never stored)
// Reduction: a thread keeps one double per part; a wave adds its 64 lanes in a fixed butterfly order; a block adds its four
// waves in order and writes ONE partial per part; kl_final_kernel (one block) adds the partials, index ascending.  No
// atomics: the same input gives the same 64 bits on every call.
#include "device_math.h"
#include "rvseg_crf.h"
#include "term_device.h"

namespace rvseg {

__global__ void __launch_bounds__(256)
onehot_kernel(const int8_t* __restrict__ labels, long long n, int C, float* __restrict__ rows) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n * C) return;
    const long long i = gid / C;
    const int c = (int)(gid - i * C);
    rows[gid] = (int)labels[i] == c ? 1.0f : 0.0f;
}

void launch_onehot(const int8_t* labels, long long n, int C, float* rows, hipStream_t s) {
    onehot_kernel<<<dim3((unsigned)((n * C + 255) / 256)), dim3(256), 0, s>>>(labels, n, C, rows);
    RV_LAUNCHED("onehot_kernel");
}

__global__ void __launch_bounds__(256)
label_gather_kernel(const float* __restrict__ rows, const int8_t* __restrict__ labels, long long n, int C, float scale, int accumulate,
                    float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int l = (int)labels[i];
    const float v = (l >= 0 && l < C) ? scale * rows[(size_t)i * C + l] : 0.0f;
    out[i] = accumulate ? out[i] + v : v;
}

void launch_label_gather(const float* rows, const int8_t* labels, long long n, int C, float scale, bool accumulate, float* out, hipStream_t s) {
    label_gather_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(rows, labels, n, C, scale, accumulate ? 1 : 0, out);
    RV_LAUNCHED("label_gather_kernel");
}

// ---------------------------------------------------------------------------------------------
// KL passes.  Thread (lp, c) of a block serves class c of point p0 + lp, PB = 256 / C points per step, like the term
// update whose device functions it shares.
// ---------------------------------------------------------------------------------------------
int kl_blocks(int C, long long n_points) {
    const int PB = KL_THREADS / C;
    const long long blocks = (n_points + PB - 1) / PB;
    return (int)(blocks > KL_MAX_BLOCKS ? KL_MAX_BLOCKS : blocks);
}

__global__ void __launch_bounds__(KL_THREADS)
kl_unary_kernel(const float* __restrict__ unary, int unary_is_energy, const float* __restrict__ Q, int C, long long n_points,
                double* __restrict__ partials) {
    __shared__ double sh[KL_THREADS / 64];
    const int PB = KL_THREADS / C;
    const int lp = threadIdx.x / C, c = threadIdx.x - lp * C;
    double e = 0.0, u = 0.0;
    for (long long p0 = (long long)blockIdx.x * PB; p0 < n_points; p0 += (long long)gridDim.x * PB) {
        const long long p = p0 + lp;
        if (lp < PB && p < n_points) {
            const size_t g = (size_t)p * C + c;
            const float q = Q[g];
            const float x = unary[g];
            const float U = unary_is_energy ? x : -x;
            const float qc = q > 1e-20f ? q : 1e-20f;   // std::max(Q, 1e-20f), densecrf.cpp:219
            const double et = (double)q * log((double)qc);
            const double ut = (double)U * (double)q;
            e = e + et;
            u = u + ut;
        }
    }
    kl_block_sum(e, sh, partials + blockIdx.x);
    kl_block_sum(u, sh, partials + KL_MAX_BLOCKS + blockIdx.x);
}

void launch_kl_unary(const float* unary, bool unary_is_energy, const float* Q, int C, long long n_points, double* partials, hipStream_t s) {
    kl_unary_kernel<<<dim3((unsigned)kl_blocks(C, n_points)), dim3(KL_THREADS), 0, s>>>(unary, unary_is_energy ? 1 : 0, Q, C, n_points, partials);
    RV_LAUNCHED("kl_unary_kernel");
}

template <bool SEQ>
__global__ void __launch_bounds__(KL_THREADS)
kl_term_kernel(LatticeDev L, int C, const float* __restrict__ values, float alpha, int post, int matrix,
               const float* __restrict__ compat, const float* __restrict__ Q, long long n_points, double* __restrict__ partial) {
    __shared__ float wt[64 * 64];
    __shared__ float rows[KL_THREADS];
    __shared__ double sh[KL_THREADS / 64];
    if (L.counters[1]) {   // uniform: hash overflow (flagged) -- the part is defined, the caller reports the overflow
        if (threadIdx.x == 0) partial[blockIdx.x] = 0.0;
        return;
    }
    const int n_w = matrix ? C * C : C;
    for (int i = threadIdx.x; i < n_w; i += KL_THREADS) wt[i] = compat[i];
    __syncthreads();
    const int PB = KL_THREADS / C;
    const int lp = threadIdx.x / C, c = threadIdx.x - lp * C;
    double acc = 0.0;
    for (long long p0 = (long long)blockIdx.x * PB; p0 < n_points; p0 += (long long)gridDim.x * PB) {   // block-uniform
        const long long p = p0 + lp;
        const bool live = lp < PB && p < n_points;
        float t = 0.0f;
        if (live) {
            const float sl = term_slice<SEQ>(L, C, values, alpha, p, c);
            t = post ? sl * L.norm[p] : sl;
        }
        if (matrix) {
            rows[threadIdx.x] = t;
            __syncthreads();
        }
        if (live) {
            const float a = term_compat(matrix != 0, wt, rows + lp * C, C, c, t);
            const double pt = (double)Q[(size_t)p * C + c] * (double)a;
            acc = acc + pt;
        }
        if (matrix) __syncthreads();   // the row is rewritten by the next group
    }
    kl_block_sum(acc, sh, partial + blockIdx.x);
}

void launch_kl_term(const LatticeDev& L, int C, bool seq, const float* values, bool post, bool matrix, const float* compat,
                    const float* Q, long long n_points, double* partial, hipStream_t s) {
    const float alpha = lattice_alpha(L.d);
    const dim3 grid((unsigned)kl_blocks(C, n_points)), block(KL_THREADS);
    if (seq) kl_term_kernel<true><<<grid, block, 0, s>>>(L, C, values, alpha, post ? 1 : 0, matrix ? 1 : 0, compat, Q, n_points, partial);
    else kl_term_kernel<false><<<grid, block, 0, s>>>(L, C, values, alpha, post ? 1 : 0, matrix ? 1 : 0, compat, Q, n_points, partial);
    RV_LAUNCHED("kl_term_kernel");
}

// One block: the partials of all parts staged in LDS (at most 10 x 512 doubles), then thread `part` adds its part's
// partials from index 0 up, and thread 0 adds the parts in order.
__global__ void __launch_bounds__(KL_FINAL_THREADS)
kl_final_kernel(const double* __restrict__ partials, int n_blocks, int n_parts, double* __restrict__ parts_out, double* __restrict__ sum_out) {
    __shared__ double sh[10 * KL_MAX_BLOCKS];
    __shared__ double part[10];
    for (int i = threadIdx.x; i < n_parts * n_blocks; i += KL_FINAL_THREADS) {
        const int k = i / n_blocks, b = i - k * n_blocks;
        sh[k * KL_MAX_BLOCKS + b] = partials[(size_t)k * KL_MAX_BLOCKS + b];
    }
    __syncthreads();
    if ((int)threadIdx.x < n_parts) {
        const double* row = sh + threadIdx.x * KL_MAX_BLOCKS;
        double r = row[0];
        for (int b = 1; b < n_blocks; b++) r = r + row[b];
        part[threadIdx.x] = r;
        if (parts_out) parts_out[threadIdx.x] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0 && sum_out) {
        double r = part[0];
        for (int k = 1; k < n_parts; k++) r = r + part[k];
        *sum_out = r;
    }
}

void launch_kl_final(const double* partials, int n_blocks, int n_parts, double* parts_out, double* sum_out, hipStream_t s) {
    kl_final_kernel<<<dim3(1), dim3(KL_FINAL_THREADS), 0, s>>>(partials, n_blocks, n_parts, parts_out, sum_out);
    RV_LAUNCHED("kl_final_kernel");
}

}  // namespace rvseg
