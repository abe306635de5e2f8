"""Expected values of a kept DenseCRF model (rvseg_crf_model_*): apply, one step, the energies and the KL parts, restated
from the CPU oracle's lattice and crf_restate's float32 operations.  Test infrastructure only.

Restates DenseCRF::startInference / stepInference (densecrf.cpp:178-201), unaryEnergy / pairwiseEnergy (:141-177) and
klDivergence (:214-235).  Everything float32 follows the library's pinned orders and is compared bit for bit; the KL parts
are float64 sums (math.fsum, correctly rounded) of per-element float64 terms, compared within KL_BOUND times the sum of
the absolute element terms."""
import math

import numpy as np

import crf_restate as R

f32 = np.float32

# |GPU part - restated part| <= KL_BOUND * S, S = the sum of the part's absolute element terms, for N * C <= 2^17: any-order
# double summation of N * C terms is off by at most N * C * 2^-53 * S ~= 1.5e-11 * S, a 2-ulp log adds 2 * 2^-52 * S
KL_BOUND = 1e-10
KL_MAX_ELEMENTS = 1 << 17


def compat_params(rng, compat, C):
    if compat == R.POTTS:
        return np.array([rng.uniform(0.5, 4.0)], f32)
    if compat == R.DIAGONAL:
        return (-rng.uniform(0.2, 4.0, C)).astype(f32)
    return rng.uniform(-2.0, 2.0, (C, C)).astype(f32)


def compat_object(rv, compat, cp, C):
    if compat == R.POTTS:
        return rv.PottsCompatibility(cp[0])
    if compat == R.DIAGONAL:
        return rv.DiagonalCompatibility(cp)
    return rv.MatrixCompatibility(cp.reshape(C, C))


def api_terms(rv, terms, C):
    """crf_restate term tuples -> the tuples Context.crf_infer_terms / crf_model_set take."""
    return [(f, compat_object(rv, c, np.asarray(p, f32), C), kt, nt, kp) for f, c, p, kt, nt, kp in terms]


def random_model(seed, N, C, specs):
    """U and terms [(features, compat, params, kernel_type, normalization, kernel_params)] for specs [(d, compat, norm)]."""
    rng = np.random.default_rng(seed)
    U = (rng.random((N, C)) * 3).astype(f32)
    terms = []
    for d, compat, norm in specs:
        F = (rng.random((N, d)) * 6).astype(f32)
        terms.append((F, compat, compat_params(rng, compat, C), R.DIAG_KERNEL, norm, None))
    return rng, U, terms


def clamp_q(rng, N, C):
    """Rows for klDivergence's max(Q, 1e-20f) (densecrf.cpp:219): exact zeros, values in (0, 1e-20), the clamp's own value,
    the first float above it, and one exactly one-hot row (N >= 12, C >= 3).  Everything else is a positive marginal."""
    assert N >= 12 and C >= 3
    e = rng.random((N, C)) + 0.05
    Q = (e / e.sum(1, keepdims=True)).astype(f32)
    Q[::3, 0] = 0.0
    Q[1::5, C - 1] = f32(1e-30)
    Q[2::7, 1] = f32(9.9e-21)
    Q[4::11, 1] = f32(1e-20)
    Q[5::11, 2] = np.nextafter(f32(1e-20), f32(1))
    Q[N // 2] = 0.0
    Q[N // 2, C // 2] = 1.0
    return Q


class Model:
    def __init__(self, oracle, U, terms):
        self.oracle = oracle
        self.U = np.ascontiguousarray(U, f32)
        self.N, self.C = self.U.shape
        self.built = []
        for f, compat, cp, kt, nt, kp in terms:
            lat = oracle.Lattice(R.kernel_features(f, kt, kp))
            nrm = R.norm_of(lat, nt) if nt != R.NO_NORMALIZATION else None
            self.built.append((lat, nrm, compat, cp, nt))

    def apply(self, k, Q):
        """pairwise_[k]->apply(out, Q): normalisation scale, lattice filter, compatibility."""
        lat, nrm, compat, cp, nt = self.built[k]
        Q = np.ascontiguousarray(Q, f32)
        inp = (Q * nrm[:, None]).astype(f32) if nt in (R.NORMALIZE_SYMMETRIC, R.NORMALIZE_BEFORE) else Q
        t = lat.compute(inp)
        if nt in (R.NORMALIZE_SYMMETRIC, R.NORMALIZE_AFTER):
            t = (t * nrm[:, None]).astype(f32)
        return R.compat_apply(compat, cp, t)

    def start(self):
        return self.oracle.exp_and_normalize(-self.U)

    def step(self, Q):
        tmp = -self.U
        for k in range(len(self.built)):
            tmp = (tmp - self.apply(k, Q)).astype(f32)
        return self.oracle.exp_and_normalize(tmp)

    def unary_energy(self, labels):
        l = np.asarray(labels, np.int64)
        ok = (l >= 0) & (l < self.C)
        r = np.zeros(self.N, f32)
        r[ok] = self.U[np.nonzero(ok)[0], l[ok]]
        return r

    def pairwise_energy(self, labels, term=-1):
        if term == -1:
            r = np.zeros(self.N, f32)
            for k in range(len(self.built)):
                r = (r + self.pairwise_energy(labels, k)).astype(f32)
            return r
        l = np.asarray(labels, np.int64)
        ok = (l >= 0) & (l < self.C)
        onehot = (l[:, None] == np.arange(self.C)[None, :]).astype(f32)
        a = self.apply(term, onehot)
        r = np.zeros(self.N, f32)
        r[ok] = (f32(-0.5) * a[np.nonzero(ok)[0], l[ok]]).astype(f32)
        return r

    def kl_parts(self, Q):
        """(parts, S): entropy, unary and one part per term as float64, and the sum of each part's absolute element terms."""
        Q = np.ascontiguousarray(Q, f32)
        assert Q.size <= KL_MAX_ELEMENTS
        q = Q.astype(np.float64)
        elems = [q * np.log(np.maximum(Q, f32(1e-20)).astype(np.float64)), self.U.astype(np.float64) * q]
        for k in range(len(self.built)):
            elems.append(q * self.apply(k, Q).astype(np.float64))
        parts = np.array([math.fsum(e.ravel()) for e in elems], np.float64)
        S = np.array([math.fsum(np.abs(e).ravel()) for e in elems], np.float64)
        return parts, S


def kl_sum(parts):
    """The KL divergence: the parts added in order, in double."""
    kl = 0.0
    for v in parts:
        kl += float(v)
    return kl
