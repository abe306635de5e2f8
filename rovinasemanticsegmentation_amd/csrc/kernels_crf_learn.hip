// Learning kernels of a kept DenseCRF model (rvseg_crf_model_objective / _backward / _gradient, rvseg_crf_logistic_gradient)
// for gfx950: the objectives of objective.cpp:35-108, the sumAndNormalize step of DenseCRF::gradient (densecrf.cpp:107-114,
// :258-296) and the reductions of the parameter gradients (labelcompatibility.cpp:57-61, :76-78, :101-108; unary.cpp:64-68).
//
// Every fp32 value follows the pinned orders of include/rvseg.h.  Every double sum follows the KL pattern
// (kernels_crf_model.hip): a thread adds its own elements in the order it meets them, a block adds its threads in a fixed
// order and writes ONE partial per sum, and a single block adds the partials, index ascending.  No atomics: the same input
// gives the same 64 bits on every call.
#include "device_math.h"
#include "rvseg_crf.h"
#include "term_device.h"

namespace rvseg {

// sum over the point groups of a block, per class: thread (lp, c) holds v; thread c < C adds lp = 0 .. PB-1 in order
__device__ __forceinline__ double learn_class_sum(double v, double* sh /* KL_THREADS */, int C, int PB) {
    __syncthreads();   // sh may still be read from the previous sum
    sh[threadIdx.x] = v;
    __syncthreads();
    double r = 0.0;
    if ((int)threadIdx.x < C) {
        r = sh[threadIdx.x];
        for (int lp = 1; lp < PB; lp++) r = r + sh[lp * C + threadIdx.x];
    }
    return r;
}

// ---------------------------------------------------------------------------------------------
// LogLikelihood / Hamming (objective.cpp:37-50, :66-79): one element per thread step, thread (lp, c) as in the KL passes.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(KL_THREADS)
objective_point_kernel(int kind, const int16_t* __restrict__ gt, float robust, const float* __restrict__ class_weight,
                       const float* __restrict__ Q, int C, long long n_points, float* __restrict__ d_mul_Q, double* __restrict__ partials) {
    __shared__ double sh[KL_THREADS / 64];
    const int PB = KL_THREADS / C;
    const int lp = threadIdx.x / C, c = threadIdx.x - lp * C;
    const float fn = (float)n_points;
    const double dn = (double)n_points;
    double acc = 0.0;
    for (long long p0 = (long long)blockIdx.x * PB; p0 < n_points; p0 += (long long)gridDim.x * PB) {
        const long long p = p0 + lp;
        if (lp < PB && p < n_points) {
            const size_t g = (size_t)p * C + c;
            const int l = (int)gt[p];
            float out = 0.0f;
            if (l == c) {   // (c is in 0 .. C-1: a label outside it matches no thread)
                const float q = Q[g];
                if (kind == RVSEG_OBJECTIVE_LOGLIKELIHOOD) {
                    const float sum = q + robust;
                    const float QQ = sum < 1e-20f ? 1e-20f : sum;   // std::max(Q + robust, 1e-20f), objective.cpp:44
                    const float r = q / QQ;
                    out = r / fn;
                    const double t = log((double)QQ) / dn;
                    acc = acc + t;
                } else {
                    const float t = class_weight[l] * q;
                    out = t;
                    acc = acc + (double)t;
                }
            }
            d_mul_Q[g] = out;
        }
    }
    kl_block_sum(acc, sh, partials + blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// IntersectionOverUnion (objective.cpp:82-108) in two passes.  Pass 1: per class the sums in[l] and un[l]; a block leaves
// partials[block][l] (in) and partials[block][C + l] (un).  iou_stats_kernel adds them over the blocks and gives the value.
// Pass 2: d_mul_Q from the finished sums.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(KL_THREADS)
iou_sums_kernel(const int16_t* __restrict__ gt, const float* __restrict__ Q, int C, long long n_points, double* __restrict__ partials) {
    __shared__ double sh[KL_THREADS];
    const int PB = KL_THREADS / C;
    const int lp = threadIdx.x / C, c = threadIdx.x - lp * C;
    double in = 0.0, un = 0.0;
    for (long long p0 = (long long)blockIdx.x * PB; p0 < n_points; p0 += (long long)gridDim.x * PB) {
        const long long p = p0 + lp;
        if (lp < PB && p < n_points) {
            const int l = (int)gt[p];
            if (l >= 0 && l < C) {
                const double q = (double)Q[(size_t)p * C + c];
                if (l == c) {
                    in = in + q;
                    un = un + 1.0;
                } else {
                    un = un + q;
                }
            }
        }
    }
    const double bi = learn_class_sum(in, sh, C, PB);
    const double bu = learn_class_sum(un, sh, C, PB);
    if ((int)threadIdx.x < C) {
        partials[(size_t)blockIdx.x * 2 * C + threadIdx.x] = bi;
        partials[(size_t)blockIdx.x * 2 * C + C + threadIdx.x] = bu;
    }
}

// one block of 128 threads: stats[l] = in[l], stats[64 + l] = un[l] (un starts at 1e-20); value = (sum in / un) / C
__global__ void __launch_bounds__(128)
iou_stats_kernel(const double* __restrict__ partials, int n_blocks, int C, double* __restrict__ stats, double* __restrict__ value) {
    __shared__ double sh[128];
    const int t = threadIdx.x;
    const int is_un = t >= 64, l = t & 63;
    if (l < C) {
        const double* col = partials + (is_un ? C : 0) + l;
        double r = is_un ? 1e-20 : 0.0;
        for (int b = 0; b < n_blocks; b++) r = r + col[(size_t)b * 2 * C];
        sh[t] = r;
        stats[t] = r;
    }
    __syncthreads();
    if (t == 0) {
        double r = 0.0;
        for (int k = 0; k < C; k++) {
            const double ratio = sh[k] / sh[64 + k];
            r = r + ratio;
        }
        *value = r / (double)C;
    }
}

__global__ void __launch_bounds__(256)
iou_grad_kernel(const int16_t* __restrict__ gt, const float* __restrict__ Q, int C, long long n_points, const double* __restrict__ stats,
                float* __restrict__ d_mul_Q) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_points * C) return;
    const long long p = gid / C;
    const int c = (int)(gid - p * C);
    const int l = (int)gt[p];
    float out = 0.0f;
    if (l >= 0 && l < C) {
        const double q = (double)Q[gid];
        const double in = stats[c], un = stats[64 + c], M = (double)C;
        if (l == c) {
            out = (float)(q / (un * M));                      // objective.cpp:103
        } else {
            const double num = (-q) * in;
            const double den = (un * un) * M;
            out = (float)(num / den);                          // :105
        }
    }
    d_mul_Q[gid] = out;
}

// ---------------------------------------------------------------------------------------------
// sumAndNormalize (densecrf.cpp:107-114) with what surrounds it in DenseCRF::gradient:
//   x[c]  = mul ? fl(in[c] * q[c]) : in[c]          (tmp1.array() * Q[it].array(), :290)
//   s     = x[0] + x[1] + ..                        (ascending)
//   b[c]  = fl(s * q[c]) - x[c]
//   ug[c] = ug_mode 1: b[c]; 2: ug[c] + b[c]         (the unary gradient, :262, :294; 0: none)
// Thread (lp, c); a point's x row meets in LDS and every thread of the point adds it in the same order.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(KL_THREADS)
sum_normalize_kernel(const float* __restrict__ in, int mul, const float* __restrict__ q, int C, long long n_points, float* __restrict__ b,
                     float* __restrict__ ug, int ug_mode) {
    __shared__ float rows[KL_THREADS];
    const int PB = KL_THREADS / C;
    const int lp = threadIdx.x / C, c = threadIdx.x - lp * C;
    const long long p = (long long)blockIdx.x * PB + lp;
    const bool live = lp < PB && p < n_points;
    const size_t g = (size_t)p * C + c;
    float x = 0.0f, qc = 0.0f;
    if (live) {
        qc = q[g];
        const float v = in[g];
        x = mul ? v * qc : v;
    }
    rows[threadIdx.x] = x;
    __syncthreads();
    if (!live) return;
    const float* r = rows + lp * C;
    float s = r[0];
    for (int k = 1; k < C; k++) s = s + r[k];
    const float sq = s * qc;
    const float out = sq - x;
    b[g] = out;
    if (ug_mode == 1) ug[g] = out;
    else if (ug_mode == 2) ug[g] = ug[g] + out;
}

// tmp1 += tmp2 of densecrf.cpp:288: acc = (first ? 0.0f : acc) + t
__global__ void __launch_bounds__(256)
add_rows_kernel(int first, const float* __restrict__ t, float* __restrict__ acc, long long total) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const float a = first ? 0.0f : acc[gid];
    acc[gid] = a + t[gid];
}

// ---------------------------------------------------------------------------------------------
// Potts / Diagonal gradient (labelcompatibility.cpp:57-61, :76-78): per class the sum over the points of b[i][c] * F[i][c],
// F the term's kernel apply of Q[it] sliced here from the blurred lattice values (times norm when `post`), as the forward
// path slices it.  A block leaves partials[block][c].
// ---------------------------------------------------------------------------------------------
template <bool SEQ>
__global__ void __launch_bounds__(KL_THREADS)
class_dot_kernel(LatticeDev L, int C, const float* __restrict__ values, float alpha, int post, const float* __restrict__ b,
                 long long n_points, double* __restrict__ partials) {
    __shared__ double sh[KL_THREADS];
    if (L.counters[1]) {   // uniform: hash overflow (flagged) -- defined partials, the caller reports the overflow
        if ((int)threadIdx.x < C) partials[(size_t)blockIdx.x * C + threadIdx.x] = 0.0;
        return;
    }
    const int PB = KL_THREADS / C;
    const int lp = threadIdx.x / C, c = threadIdx.x - lp * C;
    double acc = 0.0;
    for (long long p0 = (long long)blockIdx.x * PB; p0 < n_points; p0 += (long long)gridDim.x * PB) {
        const long long p = p0 + lp;
        if (lp < PB && p < n_points) {
            const float sl = term_slice<SEQ>(L, C, values, alpha, p, c);
            const float F = post ? sl * L.norm[p] : sl;
            const double t = (double)b[(size_t)p * C + c] * (double)F;
            acc = acc + t;
        }
    }
    const double r = learn_class_sum(acc, sh, C, PB);
    if ((int)threadIdx.x < C) partials[(size_t)blockIdx.x * C + threadIdx.x] = r;
}

// ---------------------------------------------------------------------------------------------
// g = A^T B over the points (Matrix gradient: A = b, B = F sliced here, labelcompatibility.cpp:102; logistic gradient:
// A = the unary gradient, B = a block of at most 64 feature columns, unary.cpp:65).  A: n x Ca (row stride lda), B: n x Cb
// (row stride ldb), Ca, Cb <= 64.  A block stages a tile of PAIR_TILE / max(Ca, Cb) points' rows of A and B in LDS; thread t
// owns the pairs e = t, t + 256, .. (e = i * Cb + j) -- at most 16 doubles of state for 64 x 64 -- and adds the tile's points
// in order.  Blocks walk the tiles grid-stride and leave partials[block][e].
// ---------------------------------------------------------------------------------------------
constexpr int PAIR_THREADS = 256;
constexpr int PAIR_TILE = 1024;        // floats per staged matrix
constexpr int PAIR_MAX_BLOCKS = 128;
constexpr int PAIR_PER_THREAD = 64 * 64 / PAIR_THREADS;

template <bool SLICE, bool SEQ>
__global__ void __launch_bounds__(PAIR_THREADS)
pair_sums_kernel(LatticeDev L, const float* __restrict__ values, float alpha, int post, const float* __restrict__ A, int lda, int Ca,
                 const float* __restrict__ B, int ldb, int Cb, long long n_points, double* __restrict__ partials) {
    __shared__ float sa[PAIR_TILE];
    __shared__ float sb[PAIR_TILE];
    const int n_e = Ca * Cb;
    if (SLICE && L.counters[1]) {   // uniform: hash overflow (flagged)
        for (int e = threadIdx.x; e < n_e; e += PAIR_THREADS) partials[(size_t)blockIdx.x * n_e + e] = 0.0;
        return;
    }
    const int T = PAIR_TILE / (Ca > Cb ? Ca : Cb);
    double acc[PAIR_PER_THREAD];
#pragma unroll
    for (int m = 0; m < PAIR_PER_THREAD; m++) acc[m] = 0.0;
    for (long long p0 = (long long)blockIdx.x * T; p0 < n_points; p0 += (long long)gridDim.x * T) {   // block-uniform
        const long long left = n_points - p0;
        const int tl = left < T ? (int)left : T;
        __syncthreads();   // the previous tile is still being read
        for (int e = threadIdx.x; e < tl * Ca; e += PAIR_THREADS) {
            const int t = e / Ca, i = e - t * Ca;
            sa[e] = A[(size_t)(p0 + t) * lda + i];
        }
        for (int e = threadIdx.x; e < tl * Cb; e += PAIR_THREADS) {
            const int t = e / Cb, j = e - t * Cb;
            const long long p = p0 + t;
            if (SLICE) {
                const float sl = term_slice<SEQ>(L, Cb, values, alpha, p, j);
                sb[e] = post ? sl * L.norm[p] : sl;
            } else {
                sb[e] = B[(size_t)p * ldb + j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < PAIR_PER_THREAD; m++) {
            const int e = threadIdx.x + m * PAIR_THREADS;
            if (e < n_e) {
                const int i = e / Cb, j = e - i * Cb;
                double r = acc[m];
                for (int t = 0; t < tl; t++) {
                    const double prod = (double)sa[t * Ca + i] * (double)sb[t * Cb + j];
                    r = r + prod;
                }
                acc[m] = r;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < PAIR_PER_THREAD; m++) {
        const int e = threadIdx.x + m * PAIR_THREADS;
        if (e < n_e) partials[(size_t)blockIdx.x * n_e + e] = acc[m];
    }
}

// One block: G[e] = the partials of e added over the blocks, index ascending, then by `mode`
//   0 POTTS     out[0] += -(G[0] + G[1] + ..)                               (n_e = C)
//   1 DIAGONAL  out[c] += G[c]
//   2 MATRIX    out[k] += G(i,j) + (i != j ? G(j,i) : 0) for j >= i, row by row  (Ca = Cb = C)
//   3 LOGISTIC  out[j * Ca + i] = G(i,j)                                     (column-major, assigned)
__global__ void __launch_bounds__(256)
grad_final_kernel(int mode, int Ca, int Cb, const double* __restrict__ partials, int n_blocks, double* __restrict__ out) {
    __shared__ double G[64 * 64];
    const int n_e = Ca * Cb;
    for (int e = threadIdx.x; e < n_e; e += 256) {
        double r = partials[e];
        for (int b = 1; b < n_blocks; b++) r = r + partials[(size_t)b * n_e + e];
        G[e] = r;
    }
    __syncthreads();
    if (mode == 0) {
        if (threadIdx.x == 0) {
            double r = G[0];
            for (int c = 1; c < n_e; c++) r = r + G[c];
            out[0] = out[0] + (-r);
        }
    } else if (mode == 1) {
        for (int e = threadIdx.x; e < n_e; e += 256) out[e] = out[e] + G[e];
    } else if (mode == 2) {
        const int C = Ca;
        for (int i = threadIdx.x; i < C; i += 256) {
            const int off = i * C - i * (i - 1) / 2 - i;   // packed index of (i, i) minus i
            for (int j = i; j < C; j++) {
                const double v = i != j ? G[i * C + j] + G[j * C + i] : G[i * C + j];
                out[off + j] = out[off + j] + v;
            }
        }
    } else {
        for (int e = threadIdx.x; e < n_e; e += 256) {
            const int i = e / Cb, j = e - i * Cb;
            out[(size_t)j * Ca + i] = G[e];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
int learn_pair_blocks(int Ca, int Cb, long long n_points) {
    const int T = PAIR_TILE / (Ca > Cb ? Ca : Cb);
    const long long blocks = (n_points + T - 1) / T;
    return (int)(blocks > PAIR_MAX_BLOCKS ? PAIR_MAX_BLOCKS : blocks);
}

size_t learn_partials_doubles(int C) {
    const size_t pair = (size_t)PAIR_MAX_BLOCKS * C * C, cls = (size_t)KL_MAX_BLOCKS * 2 * C;
    return pair > cls ? pair : cls;
}

void launch_objective(int kind, const int16_t* gt, float robust, const float* class_weight, const float* Q, int C, long long n_points,
                      float* d_mul_Q, double* partials, double* stats, double* value, hipStream_t s) {
    const int blocks = kl_blocks(C, n_points);
    if (kind == RVSEG_OBJECTIVE_IOU) {
        iou_sums_kernel<<<dim3((unsigned)blocks), dim3(KL_THREADS), 0, s>>>(gt, Q, C, n_points, partials);
        iou_stats_kernel<<<dim3(1), dim3(128), 0, s>>>(partials, blocks, C, stats, value);
        iou_grad_kernel<<<dim3((unsigned)((n_points * C + 255) / 256)), dim3(256), 0, s>>>(gt, Q, C, n_points, stats, d_mul_Q);
        RV_LAUNCHED("iou kernels");
        return;
    }
    objective_point_kernel<<<dim3((unsigned)blocks), dim3(KL_THREADS), 0, s>>>(kind, gt, robust, class_weight, Q, C, n_points, d_mul_Q, partials);
    RV_LAUNCHED("objective_point_kernel");
    launch_kl_final(partials, blocks, 1, nullptr, value, s);
}

void launch_sum_normalize(const float* in, bool mul, const float* q, int C, long long n_points, float* b, float* ug, int ug_mode, hipStream_t s) {
    const int PB = KL_THREADS / C;
    sum_normalize_kernel<<<dim3((unsigned)((n_points + PB - 1) / PB)), dim3(KL_THREADS), 0, s>>>(in, mul ? 1 : 0, q, C, n_points, b, ug,
                                                                                                 ug ? ug_mode : 0);
    RV_LAUNCHED("sum_normalize_kernel");
}

void launch_add_rows(bool first, const float* t, float* acc, long long total, hipStream_t s) {
    add_rows_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(first ? 1 : 0, t, acc, total);
    RV_LAUNCHED("add_rows_kernel");
}

void launch_compat_grad(const LatticeDev& L, int C, bool seq, const float* values, bool post, int compat, const float* b, long long n_points,
                        double* partials, double* out, hipStream_t s) {
    const float alpha = lattice_alpha(L.d);
    const int po = post ? 1 : 0;
    if (compat == RVSEG_COMPAT_MATRIX) {
        const int blocks = learn_pair_blocks(C, C, n_points);
        const dim3 grid((unsigned)blocks), block(PAIR_THREADS);
        if (seq) pair_sums_kernel<true, true><<<grid, block, 0, s>>>(L, values, alpha, po, b, C, C, nullptr, 0, C, n_points, partials);
        else pair_sums_kernel<true, false><<<grid, block, 0, s>>>(L, values, alpha, po, b, C, C, nullptr, 0, C, n_points, partials);
        RV_LAUNCHED("pair_sums_kernel");
        grad_final_kernel<<<dim3(1), dim3(256), 0, s>>>(2, C, C, partials, blocks, out);
    } else {
        const int blocks = kl_blocks(C, n_points);
        const dim3 grid((unsigned)blocks), block(KL_THREADS);
        if (seq) class_dot_kernel<true><<<grid, block, 0, s>>>(L, C, values, alpha, po, b, n_points, partials);
        else class_dot_kernel<false><<<grid, block, 0, s>>>(L, C, values, alpha, po, b, n_points, partials);
        RV_LAUNCHED("class_dot_kernel");
        grad_final_kernel<<<dim3(1), dim3(256), 0, s>>>(compat == RVSEG_COMPAT_POTTS ? 0 : 1, 1, C, partials, blocks, out);
    }
    RV_LAUNCHED("grad_final_kernel");
}

void launch_logistic_gradient(const float* g, const float* f, long long n_points, int C, int K, double* partials, double* out, hipStream_t s) {
    const LatticeDev none{};
    for (int k0 = 0; k0 < K; k0 += 64) {   // feature columns in blocks of 64: at most 64 x 64 pairs per launch
        const int kb = K - k0 < 64 ? K - k0 : 64;
        const int blocks = learn_pair_blocks(C, kb, n_points);
        pair_sums_kernel<false, false><<<dim3((unsigned)blocks), dim3(PAIR_THREADS), 0, s>>>(none, nullptr, 0.f, 0, g, C, C, f + k0, K, kb, n_points,
                                                                                            partials);
        grad_final_kernel<<<dim3(1), dim3(256), 0, s>>>(3, C, kb, partials, blocks, out + (size_t)k0 * C);
    }
    RV_LAUNCHED("logistic gradient kernels");
}

}  // namespace rvseg
