"""Expected values of learning on a kept DenseCRF model (rvseg_crf_model_apply_transpose / _objective / _backward /
_gradient, rvseg_crf_logistic_gradient), restated in numpy from include/rvseg.h ("Learning on the kept model").  Test
infrastructure only.

Restates PairwisePotential::applyTranspose (pairwise.cpp:63-80, :179-183), the objectives of objective.cpp:35-108,
sumAndNormalize and the backward pass of DenseCRF::gradient (densecrf.cpp:107-114, :258-296), the compatibility gradients
(labelcompatibility.cpp:57-61, :76-78, :101-108) and LogisticUnaryEnergy::gradient (unary.cpp:64-68).

The filter object and the number type are parameters.  With the CPU oracle's lattice (compute(x, reverse=...)) and float32
the restatement follows the library's pinned orders and is compared bit for bit where the header says so.  With a dense
matrix as the filter and float64 it is the same mathematics without rounding to speak of, which
test_crf_learn_cases_cpu.py checks against finite differences.

Double sums.  A value or gradient entry is a sum of n double terms (n <= N for a value: one term per point, IoU per class; n <= N per
iteration for a gradient entry).  The library adds them in an order of its own: off by at most n 2^-53 S, S the sum of the absolute terms.
The sums here are math.fsum (correctly rounded) or numpy's float64 dot products (off by at most n 2^-53 S again).  For
n <= 2^17 both together stay below 2 * 2^17 * 2^-53 S = 2.9e-11 S, a 2-ulp log adds 4.4e-16 S: the bound KL_BOUND = 1e-10 of
crf_model_cases.py holds for every count up to LEARN_MAX_TERMS."""
import math

import numpy as np

import crf_restate as R
from crf_model_cases import KL_BOUND  # noqa: F401  (the tests read it from here)

f32 = np.float32
LOGLIKELIHOOD, HAMMING, IOU = range(3)
LEARN_MAX_TERMS = 1 << 17


def pre_post(nt, transpose):
    """DenseKernel::filter (pairwise.cpp:65, :78): is the input / the output scaled by norm?"""
    pre = nt == R.NORMALIZE_SYMMETRIC or nt == (R.NORMALIZE_AFTER if transpose else R.NORMALIZE_BEFORE)
    post = nt == R.NORMALIZE_SYMMETRIC or nt == (R.NORMALIZE_BEFORE if transpose else R.NORMALIZE_AFTER)
    return pre, post


def compat_apply(compat, cp, t, dt):
    """crf_restate.compat_apply in the number type dt (the same operations in the same order)."""
    C = t.shape[1]
    cp = np.asarray(cp, dt).reshape(-1)
    if compat == R.POTTS:
        return (dt(-cp[0]) * t).astype(dt)
    if compat == R.DIAGONAL:
        return (cp[None, :] * t).astype(dt)
    m = cp.reshape(C, C)
    W = (dt(0.5) * (m + m.T)).astype(dt)
    acc = (W[:, 0][None, :] * t[:, 0:1]).astype(dt)
    for k in range(1, C):
        acc = (acc + (W[:, k][None, :] * t[:, k:k + 1]).astype(dt)).astype(dt)
    return acc


def n_compat_params(compat, C):
    return {R.POTTS: 1, R.DIAGONAL: C, R.MATRIX: C * (C + 1) // 2}[compat]


def sum_and_normalize(x, q, dt):
    s = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        s = (s + x[:, c]).astype(dt)
    return ((s[:, None] * q).astype(dt) - x).astype(dt)


def softmax(x):
    """expAndNormalize (densecrf.cpp:97-106) in float64."""
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


class DenseFilter:
    """A lattice stand-in: an explicit N x N matrix (compute = K x, reverse = K^T x)."""

    def __init__(self, K):
        self.K = np.asarray(K, np.float64)
        self.N = self.K.shape[0]

    def compute(self, x, reverse=False):
        return (self.K.T if reverse else self.K) @ np.asarray(x, np.float64)


def norm_of(filt, nt, dt):
    """pairwise.cpp:40-56 (crf_restate.norm_of for the oracle lattice)."""
    if nt == R.NO_NORMALIZATION:
        return None
    if dt is f32:
        return R.norm_of(filt, nt)
    n = filt.compute(np.ones((filt.N, 1)))[:, 0]
    return 1.0 / np.sqrt(n + 1e-20) if nt == R.NORMALIZE_SYMMETRIC else 1.0 / (n + 1e-20)


class Learn:
    """built: [(filter, norm or None, compat, compat_params, normalization)] -- crf_model_cases.Model(...).built for the
    oracle lattice.  dt: np.float32 (pinned orders, start = the oracle's exp_and_normalize) or np.float64."""

    def __init__(self, U, built, dt=f32, exp_and_normalize=None):
        self.dt = dt
        self.U = np.ascontiguousarray(U, dt)
        self.N, self.C = self.U.shape
        self.built = list(built)
        self.softmax = exp_and_normalize if exp_and_normalize is not None else softmax

    @classmethod
    def of_model(cls, model):
        return cls(model.U, model.built, f32, model.oracle.exp_and_normalize)

    # ---- the filter with its normalisation, forward and transposed ----
    def filter(self, k, x, transpose=False):
        filt, nrm, _, _, nt = self.built[k]
        dt = self.dt
        pre, post = pre_post(nt, transpose)
        x = np.ascontiguousarray(x, dt)
        if pre:
            x = (x * nrm[:, None]).astype(dt)
        t = np.asarray(filt.compute(x, reverse=transpose), dt)
        if post:
            t = (t * nrm[:, None]).astype(dt)
        return t

    def apply(self, k, Q):
        _, _, compat, cp, _ = self.built[k]
        return compat_apply(compat, cp, self.filter(k, Q), self.dt)

    def apply_transpose(self, k, b):
        _, _, compat, cp, _ = self.built[k]
        return compat_apply(compat, cp, self.filter(k, b, True), self.dt)

    def forward(self, n):
        """Q[0 .. n] of DenseCRF::gradient's forward pass (densecrf.cpp:240-253)."""
        dt = self.dt
        Qs = [np.asarray(self.softmax(-self.U), dt)]
        for _ in range(n):
            tmp = -self.U
            for k in range(len(self.built)):
                tmp = (tmp - self.apply(k, Qs[-1])).astype(dt)
            Qs.append(np.asarray(self.softmax(tmp), dt))
        return Qs

    # ---- objectives: (value, d_mul_Q, S) with S the sum of the value's absolute terms ----
    def objective(self, obj, Q):
        kind, gt, robust, cw = obj
        dt, N, C = self.dt, self.N, self.C
        Q = np.ascontiguousarray(Q, dt)
        gt = np.asarray(gt, np.int64)
        ok = (gt >= 0) & (gt < C)
        idx = np.nonzero(ok)[0]
        l = gt[idx]
        dq = np.zeros((N, C), dt)
        q = Q[idx, l]
        if kind == LOGLIKELIHOOD:
            QQ = np.maximum((q + dt(robust)).astype(dt), dt(1e-20))
            dq[idx, l] = ((q / QQ).astype(dt) / dt(N)).astype(dt)
            terms = np.log(QQ.astype(np.float64)) / float(N)
        elif kind == HAMMING:
            t = (np.asarray(cw, dt)[l] * q).astype(dt)
            dq[idx, l] = t
            terms = t.astype(np.float64)
        else:
            q64 = Q.astype(np.float64)
            onehot = np.zeros((N, C), bool)
            onehot[idx, l] = True
            inn = np.array([math.fsum(q64[onehot[:, c], c]) for c in range(C)])
            un = np.array([math.fsum([1e-20] + [1.0] * int(onehot[:, c].sum()) + list(q64[ok & ~onehot[:, c], c])) for c in range(C)])
            own = q64 / (un * C)
            other = (-q64 * inn) / ((un * un) * C)
            d = np.where(onehot, own, other)
            d[~ok] = 0.0
            dq = d.astype(dt)
            terms = inn / un
            value = math.fsum(terms) / C
            return value, dq, math.fsum(np.abs(terms)) / C
        return math.fsum(terms), dq, math.fsum(np.abs(terms))

    # ---- the backward pass ----
    def compat_terms(self, k, b, Q):
        """(gradient, S) of term k's compatibility parameters from b and Q[it]: float64 sums of float64 products."""
        _, _, compat, _, _ = self.built[k]
        C = self.C
        b64 = np.asarray(b, np.float64)
        F = self.filter(k, Q).astype(np.float64)
        if compat == R.MATRIX:
            g, S = b64.T @ F, np.abs(b64).T @ np.abs(F)
            iu = [(i, j) for i in range(C) for j in range(i, C)]
            return (np.array([g[i, j] + (g[j, i] if i != j else 0.0) for i, j in iu]),
                    np.array([S[i, j] + (S[j, i] if i != j else 0.0) for i, j in iu]))
        e = b64 * F
        if compat == R.DIAGONAL:
            return (np.array([math.fsum(e[:, c]) for c in range(C)]), np.array([math.fsum(np.abs(e[:, c])) for c in range(C)]))
        return np.array([-math.fsum(e.ravel())]), np.array([math.fsum(np.abs(e).ravel())])

    def backward(self, Qs, dq):
        """(unary_grad, compat_grad, S): densecrf.cpp:258-296 from d_mul_Q and Q[0 .. n]; compat_grad float64, the terms
        concatenated, with S the sum of every entry's absolute element terms."""
        dt = self.dt
        n = len(Qs) - 1
        b = sum_and_normalize(np.ascontiguousarray(dq, dt), np.asarray(Qs[n], dt), dt)
        ug = b.copy()
        sizes = [n_compat_params(t[2], self.C) for t in self.built]
        cg, S = np.zeros(sum(sizes)), np.zeros(sum(sizes))
        for it in range(n - 1, -1, -1):
            Q = np.asarray(Qs[it], dt)
            tmp1 = np.zeros((self.N, self.C), dt)
            off = 0
            for k in range(len(self.built)):
                g, s = self.compat_terms(k, b, Q)
                cg[off:off + sizes[k]] += g
                S[off:off + sizes[k]] += s
                off += sizes[k]
                tmp1 = (tmp1 + self.apply_transpose(k, b)).astype(dt)
            b = sum_and_normalize((tmp1 * Q).astype(dt), Q, dt)
            ug = (ug + b).astype(dt)
        return ug, cg, S

    def gradient(self, n, obj):
        """(value, unary_grad, compat_grad, Q[n], value S, compat S)."""
        Qs = self.forward(n)
        value, dq, vS = self.objective(obj, Qs[n])
        ug, cg, S = self.backward(Qs, dq)
        return value, ug, cg, Qs[n], vS, S


def logistic_gradient(ug, f):
    """(out, S): out[k*C + m] = sum_i g[i][m] f[i][k] in float64 (unary.cpp:64-68, column-major like unaryParameters())."""
    g64, f64 = np.asarray(ug, np.float64), np.asarray(f, np.float64)
    return (f64.T @ g64).reshape(-1), (np.abs(f64).T @ np.abs(g64)).reshape(-1)


def invalid_gt(N, C):
    """A ground truth without one valid label: -1, other negatives and labels >= C mixed."""
    gt = np.full(N, -1, np.int16)
    gt[1::2] = C
    gt[2::5] = C + 3
    gt[3::7] = -7
    return gt


def gt_without_class(rng, N, C, absent):
    """Labels of every class but `absent` (each occurs when N >= 2 C), with a skipped point of either kind when N > 5."""
    gt = rng.integers(0, C - 1, N)
    gt[:C - 1] = np.arange(C - 1)
    gt[gt >= absent] += 1
    if N > 5:
        gt[C], gt[C + 1] = -1, C
    return gt.astype(np.int16)


def hamming_weights(gt, class_weight_pow):
    """Hamming::Hamming(gt, class_weight_pow), objective.cpp:51-63, in float32."""
    gt = np.asarray(gt, np.int64)
    M = max(0, int(gt.max()) + 1)
    cnt = np.bincount(gt[gt >= 0], minlength=M).astype(f32)
    w = cnt / cnt.sum(dtype=f32)
    w = np.power(w, f32(-class_weight_pow)).astype(f32)
    return (w / (cnt * w).sum(dtype=f32)).astype(f32)
