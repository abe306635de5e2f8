"""Expected values of the kernel-parameter gradient of a kept DenseCRF model (rvseg_crf_model_lattice_gradient /
_kernel_gradient / _backward_kernel / _gradient_kernel), restated in numpy from include/rvseg.h ("Kernel-parameter
gradient").  Test infrastructure only.

Follows Permutohedral::gradient (permutohedral.cpp:611-695), DenseKernel::kernelGradient / featureGradient / gradient
(pairwise.cpp:82-114, :152-163) and PairwisePotential::kernelGradient (:202-207) line by line.

The lattice and the number type are parameters.  In float32 the lattice is the CPU oracle's (offset, barycentric,
blur_n1 / n2, and rank read through ctypes from its handle), the splat adds separately rounded products in ascending
point order, the blur is (float)((double)o + 0.5 * (double)(n1 + n2)): compared bit for bit with the GPU.  In float64 the
lattice is NumpyLattice below (init, splat, blur, slice in plain numpy), which test_crf_kgrad_cases_cpu.py checks against
finite differences.

Double sums: an entry of a kernel gradient adds N products per (iteration, term); the bound KL_BOUND of crf_model_cases.py
holds for N <= 2^17 as crf_learn_cases.py explains."""
import math

import numpy as np

import crf_learn_cases as LC
import crf_restate as R
from crf_model_cases import KL_BOUND  # noqa: F401  (the tests read it from here)

f32, f64 = np.float32, np.float64


def scale_factors(d, dt):
    """permutohedral.cpp:623-625 (a float inv_std_dev, the product in double)."""
    if dt is f32:
        inv = f32(math.sqrt(2.0 / 3.0) * (d + 1))
        return np.array([f32(1.0 / math.sqrt(float((i + 2) * (i + 1))) * float(inv)) for i in range(d)], f32)
    inv = math.sqrt(2.0 / 3.0) * (d + 1)
    return np.array([1.0 / math.sqrt(float((i + 2) * (i + 1))) * inv for i in range(d)], f64)


class OracleView:
    """The arrays of an oracle.Lattice that the gradient reads, rank included (N x (d+1) floats behind lat.h.contents.rank)."""

    def __init__(self, lat):
        self.lat = lat
        self.N, self.d, self.M = lat.N, lat.d, lat.M
        self.offset, self.barycentric = lat.offset, lat.barycentric
        self.blur_n1, self.blur_n2 = lat.blur_n1, lat.blur_n2
        n = self.N * (self.d + 1)
        self.rank = np.ctypeslib.as_array(lat.h.contents.rank, (n,)).reshape(self.N, self.d + 1).astype(np.int64)
        self.scale = scale_factors(self.d, f32)

    def compute(self, x, reverse=False):
        return self.lat.compute(np.ascontiguousarray(x, f32), reverse=reverse)


class NumpyLattice:
    """Permutohedral::init (permutohedral.cpp:140-321) in float64 without the SSE padding, with compute() = splat, blur,
    slice (:476-530)."""

    def __init__(self, feature):
        feature = np.asarray(feature, f64)
        self.N, self.d = N, d = feature.shape
        self.scale = scale_factors(d, f64)
        self.offset = np.zeros((N, d + 1), np.int64)
        self.barycentric = np.zeros((N, d + 1), f64)
        self.rank = np.zeros((N, d + 1), np.int64)
        keys = {}
        canonical = np.zeros((d + 1, d + 1), np.int64)
        for i in range(d + 1):
            canonical[i, :d - i + 1] = i
            canonical[i, d - i + 1:] = i - (d + 1)
        for k in range(N):
            el = np.zeros(d + 1)
            sm = 0.0
            for j in range(d, 0, -1):
                cf = feature[k, j - 1] * self.scale[j - 1]
                el[j] = sm - j * cf
                sm += cf
            el[0] = sm
            v = np.rint(el / (d + 1))
            rem0 = v * (d + 1)
            s = int(v.sum())
            rank = np.zeros(d + 1, np.int64)
            for i in range(d):
                for j in range(i + 1, d + 1):
                    if el[i] - rem0[i] < el[j] - rem0[j]:
                        rank[i] += 1
                    else:
                        rank[j] += 1
            rank += s
            for i in range(d + 1):
                if rank[i] < 0:
                    rank[i] += d + 1
                    rem0[i] += d + 1
                elif rank[i] > d:
                    rank[i] -= d + 1
                    rem0[i] -= d + 1
            bary = np.zeros(d + 2)
            for i in range(d + 1):
                t = (el[i] - rem0[i]) / (d + 1)
                bary[d - rank[i]] += t
                bary[d - rank[i] + 1] -= t
            bary[0] += 1.0 + bary[d + 1]
            for r in range(d + 1):
                key = tuple(int(rem0[i]) + int(canonical[r, rank[i]]) for i in range(d))
                self.offset[k, r] = keys.setdefault(key, len(keys))
            self.rank[k] = rank
            self.barycentric[k] = bary[:d + 1]
        self.M = M = len(keys)
        self.blur_n1 = np.full((d + 1, M), -1, np.int64)
        self.blur_n2 = np.full((d + 1, M), -1, np.int64)
        for key, i in keys.items():
            for j in range(d + 1):
                n1 = [c - 1 for c in key]
                n2 = [c + 1 for c in key]
                if j < d:
                    n1[j], n2[j] = key[j] + d, key[j] - d
                self.blur_n1[j, i] = keys.get(tuple(n1), -1)
                self.blur_n2[j, i] = keys.get(tuple(n2), -1)

    def compute(self, x, reverse=False):
        x = np.asarray(x, f64)
        vals = blur(self, splat(self, x, f64), reverse, f64)
        alpha = 1.0 / (1.0 + 2.0 ** -self.d)
        out = np.zeros_like(x)
        for j in range(self.d + 1):
            out += (self.barycentric[:, j] * alpha)[:, None] * vals[self.offset[:, j]]
        return out


def splat(lat, x, dt):
    """permutohedral.cpp:635-642: points ascending, every product rounded before it is added."""
    vals = np.zeros((lat.M, x.shape[1]), dt)
    bary = lat.barycentric.astype(dt)
    for i in range(lat.N):
        for j in range(lat.d + 1):
            o = lat.offset[i, j]
            vals[o] = (vals[o] + (bary[i, j] * x[i]).astype(dt)).astype(dt)
    return vals


def blur(lat, vals, reverse, dt):
    """permutohedral.cpp:645-658: new = old + 0.5 * (n1 + n2), the sum n1 + n2 in dt, the rest in double, rounded to dt."""
    for j in (range(lat.d, -1, -1) if reverse else range(lat.d + 1)):
        n1, n2 = lat.blur_n1[j], lat.blur_n2[j]
        a = np.where((n1 >= 0)[:, None], vals[np.maximum(n1, 0)], dt(0))
        b = np.where((n2 >= 0)[:, None], vals[np.maximum(n2, 0)], dt(0))
        vals = (vals.astype(f64) + 0.5 * (a + b).astype(dt).astype(f64)).astype(dt)
    return vals


def alpha_of(d, dt):
    """float alpha = 1.0f / (1 + powf(2, -d)) / (d + 1), :628."""
    return dt(dt(dt(1) / dt(dt(1) + dt(2.0 ** -d))) / dt(d + 1))


def slice_gradient(lat, vals, x, dirn, df, dt):
    """permutohedral.cpp:660-691 for one direction, all points at once."""
    d = lat.d
    alpha = alpha_of(d, dt)
    r0 = d - lat.rank
    r1 = np.where(r0 + 1 > d, 0, r0 + 1)
    o0 = np.take_along_axis(lat.offset, r0, 1)
    o1 = np.take_along_axis(lat.offset, r1, 1)
    ra = [((dt(0) + (alpha * vals[o0[:, j]]).astype(dt)).astype(dt) - (alpha * vals[o1[:, j]]).astype(dt)).astype(dt) for j in range(d + 1)]
    sm = ra[0].copy()
    for j in range(1, d + 1):
        v = (lat.scale[j - 1] * (sm - (dt(j) * ra[j]).astype(dt)).astype(dt)).astype(dt)
        prod = (x * v).astype(dt)
        grad = np.zeros(lat.N, dt)
        for k in range(x.shape[1]):
            grad = (grad + prod[:, k]).astype(dt)
        df[:, j - 1] = (df[:, j - 1] + grad).astype(dt) if dirn else grad
        sm = (sm + ra[j]).astype(dt)


def lattice_gradient(lat, a, b, dt):
    """Permutohedral::gradient(a, b): df (N x d), the exact derivative of b^T K a = a^T K^T b (of a^T K b only for d = 1)."""
    a, b = np.ascontiguousarray(a, dt), np.ascontiguousarray(b, dt)
    df = np.zeros((lat.N, lat.d), dt)
    for dirn in range(2):
        vals = blur(lat, splat(lat, b if dirn else a, dt), dirn == 1, dt)
        slice_gradient(lat, vals, a if dirn else b, dirn, df, dt)
    return df


def feature_gradient(lat, nrm, nt, a, b, dt):
    """DenseKernel::featureGradient (pairwise.cpp:87-114); lat.compute is lattice_.compute."""
    a, b = np.ascontiguousarray(a, dt), np.ascontiguousarray(b, dt)
    G = lambda x, y: lattice_gradient(lat, x, y, dt)   # noqa: E731
    if nt == R.NO_NORMALIZATION:
        return G(a, b)
    n = np.asarray(nrm, dt)[:, None]
    K = lambda x, rev=False: np.asarray(lat.compute(x, reverse=rev), dt)   # noqa: E731
    ones = np.ones_like(a)
    n2 = (n * n).astype(dt)
    if nt == R.NORMALIZE_SYMMETRIC:
        an, bn = (a * n).astype(dt), (b * n).astype(dt)
        fa, fb = K(an, True), K(bn)
        n3 = (n2 * n).astype(dt)
        X = ((dt(0.5) * ((a * fb).astype(dt) + (fa * b).astype(dt)).astype(dt)).astype(dt) * n3).astype(dt)
        return (G(an, bn) - G(X, ones)).astype(dt)
    if nt == R.NORMALIZE_AFTER:
        fb = K(b)
        X = ((a * fb).astype(dt) * n2).astype(dt)
        return (G((a * n).astype(dt), b) - G(X, ones)).astype(dt)
    fa = K(a, True)
    X = ((fa * b).astype(dt) * n2).astype(dt)
    return (G(a, (b * n).astype(dt)) - G(X, ones)).astype(dt)


def n_kernel_params(kt, d):
    return {R.CONST_KERNEL: 0, R.DIAG_KERNEL: d, R.FULL_KERNEL: d * d}[kt]


def kernel_reduce(fg, f, kt):
    """(grad, S) of DenseKernel::gradient from fg and the raw features f, float64: FULL grad[b*d + a] = sum_i fg[i][a] f[i][b],
    DIAG its diagonal, CONST nothing."""
    d = fg.shape[1]
    if kt == R.CONST_KERNEL:
        return np.zeros(0), np.zeros(0)
    fg64, f64_ = np.asarray(fg, f64), np.asarray(f, f64)
    full = np.array([[math.fsum(fg64[:, a] * f64_[:, b]) for a in range(d)] for b in range(d)])
    S = np.array([[math.fsum(np.abs(fg64[:, a] * f64_[:, b])) for a in range(d)] for b in range(d)])
    if kt == R.DIAG_KERNEL:
        return np.diag(full).copy(), np.diag(S).copy()
    return full.reshape(-1), S.reshape(-1)


class KernelLearn:
    """The kernel-parameter gradient beside a crf_learn_cases.Learn `lr` on the same model.  views: one OracleView (or
    NumpyLattice) per term; terms: the crf_restate tuples (features, compat, params, kernel_type, normalization, kernel_params)."""

    def __init__(self, lr, views, terms):
        self.lr, self.views, self.terms, self.dt = lr, views, terms, lr.dt

    def feature_gradient(self, k, a, b):
        return feature_gradient(self.views[k], self.lr.built[k][1], self.terms[k][4], a, b, self.dt)

    def kernel_gradient(self, k, a, b):
        """(grad, S, fg)."""
        fg = self.feature_gradient(k, a, b)
        g, S = kernel_reduce(fg, self.terms[k][0], self.terms[k][3])
        return g, S, fg

    def lbl_Q(self, k, Q):
        return LC.compat_apply(self.terms[k][1], self.terms[k][2], np.ascontiguousarray(Q, self.dt), self.dt)

    def sizes(self):
        return [n_kernel_params(t[3], np.shape(t[0])[1]) for t in self.terms]

    def backward(self, Qs, dq):
        """(kernel_grad, S): the kernel_grad of densecrf.cpp:258-296, from the b of crf_learn_cases.Learn.backward."""
        lr, dt = self.lr, self.dt
        n = len(Qs) - 1
        sizes = self.sizes()
        kg, S = np.zeros(sum(sizes)), np.zeros(sum(sizes))
        b = LC.sum_and_normalize(np.ascontiguousarray(dq, dt), np.asarray(Qs[n], dt), dt)
        for it in range(n - 1, -1, -1):
            Q = np.asarray(Qs[it], dt)
            tmp1 = np.zeros((lr.N, lr.C), dt)
            off = 0
            for k in range(len(self.terms)):
                if sizes[k]:
                    g, s, _ = self.kernel_gradient(k, b, self.lbl_Q(k, Q))
                    kg[off:off + sizes[k]] += g
                    S[off:off + sizes[k]] += s
                off += sizes[k]
                tmp1 = (tmp1 + lr.apply_transpose(k, b)).astype(dt)
            b = LC.sum_and_normalize((tmp1 * Q).astype(dt), Q, dt)
        return kg, S
