// Kernel-parameter gradient of a kept DenseCRF model (rvseg_crf_model_lattice_gradient / _kernel_gradient / _backward_kernel
// / _gradient_kernel) for gfx950: the per-point ranks the model keeps, the slicing gradient of Permutohedral::gradient
// (permutohedral.cpp:660-691) and the element-wise steps of DenseKernel::featureGradient (pairwise.cpp:87-114) and
// PairwisePotential::kernelGradient (:202-207).
//
// Every fp32 value follows the orders of include/rvseg.h ("Kernel-parameter gradient"): one operation, one rounding, in
// the order written here.  No atomics.
#include "device_math.h"
#include "rvseg_crf.h"
#include "term_device.h"

namespace rvseg {

// ---------------------------------------------------------------------------------------------
// The d+1 ranks of a point (permutohedral.cpp:201-242), with the fp32 arithmetic of lattice_points_kernel: elevate, round
// half to even, the rank comparisons, back onto the plane.  rank[j] in 0 .. d, 3 bits each, j = 0 in the lowest bits.
// ---------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(256)
point_rank_kernel(LatticeDev L, const float* __restrict__ feat, unsigned* __restrict__ ranks) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L.N) return;
    const float invdplus1 = 1.0f / (D + 1), dplus1 = (float)(D + 1);
    float el[D + 1], rem0[D + 1], rank[D + 1];
    float sm = 0.0f;
#pragma unroll
    for (int j = D; j > 0; j--) {
        const float cf = feat[(size_t)i * D + j - 1] * L.scale[j - 1];
        el[j] = sm - (float)j * cf;
        sm += cf;
    }
    el[0] = sm;
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k <= D; k++) {
        float v = invdplus1 * el[k];
        v = rintf(v);
        rem0[k] = v * dplus1;
        sum += v;
    }
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
    unsigned packed = 0;
#pragma unroll
    for (int k = 0; k <= D; k++) {
        rank[k] += sum;
        const float add = rank[k] < 0.0f ? dplus1 : 0.0f;
        const float sub = rank[k] >= dplus1 ? dplus1 : 0.0f;
        rank[k] += add - sub;
        int r = (int)rank[k];
        r = r < 0 ? 0 : (r > D ? D : r);   // (only features that are not finite leave 0 .. d; the index stays in the point's row)
        packed |= (unsigned)r << (3 * k);
    }
    ranks[i] = packed;
}

void launch_point_ranks(const LatticeDev& L, const float* feat, unsigned* ranks, hipStream_t s) {
    const dim3 grid((unsigned)((L.N + 255) / 256)), block(256);
    with_dimension(L.d, [&](auto dim) { point_rank_kernel<decltype(dim)::value><<<grid, block, 0, s>>>(L, feat, ranks); });
    RV_LAUNCHED("point_rank_kernel");
}

// ---------------------------------------------------------------------------------------------
// The slicing gradient of one direction (permutohedral.cpp:660-691).  Thread (lp, k) of a block serves channel k of point
// p0 + lp, PB = 256 / C points per step, like the KL passes: the C threads of a point read a vertex row side by side.
//   V(r)     = fl(alpha * values[o(r)][k]),  o(r) the point's vertex of remainder r
//   ra[j]    = (0.0f + V(r0)) - V(r1),  r0 = d - rank[j], r1 = r0 + 1 > d ? 0 : r0 + 1
//   sm       = ra[0];  for j = 1 .. d:  v = fl(sf[j-1] * fl(sm - fl((float)j * ra[j])));  prod[j][k] = fl(x[i][k] * v);  sm += ra[j]
// The products meet in LDS (7 x 256 floats); thread (lp, j) then adds its chain over k = 0 .. C-1 from 0.0f in order and
// writes df[i][j-1] (dir 0) or fl(df[i][j-1] + grad) (dir 1).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(KL_THREADS)
slice_gradient_kernel(LatticeDev L, int C, const float* __restrict__ values, float alpha, const float* __restrict__ x,
                      const unsigned* __restrict__ ranks, int dir, long long n_points, float* __restrict__ df) {
    __shared__ float prod[7 * KL_THREADS];
    const int d = L.d, dp1 = d + 1;
    const int PB = KL_THREADS / C;
    if (L.counters[1]) {   // uniform: hash overflow (flagged) -- a defined result, the caller reports the overflow
        if (dir == 0)
            for (long long e = (long long)blockIdx.x * KL_THREADS + threadIdx.x; e < n_points * d; e += (long long)gridDim.x * KL_THREADS) df[e] = 0.0f;
        return;
    }
    const int lp = threadIdx.x / C, k = threadIdx.x - lp * C;
    for (long long p0 = (long long)blockIdx.x * PB; p0 < n_points; p0 += (long long)gridDim.x * PB) {   // block-uniform
        const long long p = p0 + lp;
        if (lp < PB && p < n_points) {
            const unsigned rk = ranks[p];
            const float xv = x[(size_t)p * C + k];
            float sm = 0.0f;
            for (int j = 0; j <= d; j++) {
                const int r0 = d - (int)((rk >> (3 * j)) & 7u);
                const int r1 = r0 + 1 > d ? 0 : r0 + 1;
                const float v0 = alpha * values[(size_t)lattice_vertex(L, p, dp1, r0) * C + k];
                const float v1 = alpha * values[(size_t)lattice_vertex(L, p, dp1, r1) * C + k];
                const float t = 0.0f + v0;
                const float ra = t - v1;
                if (j == 0) {
                    sm = ra;
                } else {
                    const float jr = (float)j * ra;
                    const float e = sm - jr;
                    const float v = L.scale[j - 1] * e;
                    prod[(j - 1) * KL_THREADS + threadIdx.x] = xv * v;
                    sm = sm + ra;
                }
            }
        }
        __syncthreads();
        const long long left = n_points - p0;
        const int live = left < PB ? (int)left : PB;   // points of this step
        for (int t = threadIdx.x; t < live * d; t += KL_THREADS) {
            const int q = t / d, j = t - q * d;
            const float* row = prod + j * KL_THREADS + q * C;
            float grad = 0.0f;
            for (int c = 0; c < C; c++) grad = grad + row[c];
            const size_t o = (size_t)(p0 + q) * d + j;
            df[o] = dir ? df[o] + grad : grad;
        }
        __syncthreads();   // the products are rewritten by the next step
    }
}

void launch_slice_gradient(const LatticeDev& L, int C, const float* values, const float* x, const unsigned* ranks, int dir, long long n_points,
                           float* df, hipStream_t s) {
    const float alpha = lattice_alpha(L.d) / (L.d + 1);   // permutohedral.cpp:628
    slice_gradient_kernel<<<dim3((unsigned)kl_blocks(C, n_points)), dim3(KL_THREADS), 0, s>>>(L, C, values, alpha, x, ranks, dir, n_points, df);
    RV_LAUNCHED("slice_gradient_kernel");
}

// ---------------------------------------------------------------------------------------------
// lbl_Q = compatibility(Q) without a filter (pairwise.cpp:203-205), thread (lp, c): term_compat on the point's own row
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(KL_THREADS)
compat_rows_kernel(int C, int matrix, const float* __restrict__ compat, const float* __restrict__ Q, long long n_points, float* __restrict__ out) {
    __shared__ float wt[64 * 64];
    __shared__ float rows[KL_THREADS];
    const int n_w = matrix ? C * C : C;
    for (int i = threadIdx.x; i < n_w; i += KL_THREADS) wt[i] = compat[i];
    const int PB = KL_THREADS / C;
    const int lp = threadIdx.x / C, c = threadIdx.x - lp * C;
    const long long p = (long long)blockIdx.x * PB + lp;
    const bool live = lp < PB && p < n_points;
    const float q = live ? Q[(size_t)p * C + c] : 0.0f;
    rows[threadIdx.x] = q;
    __syncthreads();
    if (live) out[(size_t)p * C + c] = term_compat(matrix != 0, wt, rows + lp * C, C, c, q);
}

void launch_compat_rows(int C, bool matrix, const float* compat, const float* Q, long long n_points, float* out, hipStream_t s) {
    const int PB = KL_THREADS / C;
    compat_rows_kernel<<<dim3((unsigned)((n_points + PB - 1) / PB)), dim3(KL_THREADS), 0, s>>>(C, matrix ? 1 : 0, compat, Q, n_points, out);
    RV_LAUNCHED("compat_rows_kernel");
}

// ---------------------------------------------------------------------------------------------
// The element-wise steps of featureGradient, one thread per element
//   mode 0  out = fl(a * n)                                                          (x * norm_.asDiagonal())
//   mode 1  out = fl(fl(0.5f * fl(fl(a * fb) + fl(fa * b))) * fl(fl(n * n) * n))     (SYMMETRIC, pairwise.cpp:94-95)
//   mode 2  out = fl(fl(a * b) * fl(n * n))                                          (AFTER: a, fb; BEFORE: fa, b; :102-103, :110-111)
//   mode 3  out = fl(a - b)                                                          (-r + kernelGradient(..); n unused, C = d)
//   mode 4  out = 1.0f
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
kgrad_mix_kernel(int mode, const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ fa, const float* __restrict__ fb,
                 const float* __restrict__ n, int C, long long total, float* __restrict__ out) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    float r;
    if (mode == 0) {
        r = a[gid] * n[gid / C];
    } else if (mode == 1) {
        const float nn = n[gid / C];
        const float afb = a[gid] * fb[gid];
        const float fab = fa[gid] * b[gid];
        const float sum = afb + fab;
        const float half = 0.5f * sum;
        const float n2 = nn * nn;
        const float n3 = n2 * nn;
        r = half * n3;
    } else if (mode == 2) {
        const float nn = n[gid / C];
        const float ab = a[gid] * b[gid];
        const float n2 = nn * nn;
        r = ab * n2;
    } else if (mode == 3) {
        r = a[gid] - b[gid];
    } else {
        r = 1.0f;
    }
    out[gid] = r;
}

void launch_kgrad_mix(int mode, const float* a, const float* b, const float* fa, const float* fb, const float* n, int C, long long total,
                      float* out, hipStream_t s) {
    kgrad_mix_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s>>>(mode, a, b, fa, fb, n, C, total, out);
    RV_LAUNCHED("kgrad_mix_kernel");
}

// out[a] += full[a * d + a] (DIAG) or out[e] += full[e] (FULL), full = the d x d column-major product of launch_logistic_gradient
__global__ void __launch_bounds__(64)
kgrad_accumulate_kernel(int diag, int d, const double* __restrict__ full, double* __restrict__ out) {
    const int e = threadIdx.x;
    if (e >= (diag ? d : d * d)) return;
    out[e] = out[e] + full[diag ? e * d + e : e];
}

void launch_kgrad_accumulate(bool diag, int d, const double* full, double* out, hipStream_t s) {
    kgrad_accumulate_kernel<<<dim3(1), dim3(64), 0, s>>>(diag ? 1 : 0, d, full, out);
    RV_LAUNCHED("kgrad_accumulate_kernel");
}

}  // namespace rvseg
