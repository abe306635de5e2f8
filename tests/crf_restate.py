"""Expected values of the learned-model DenseCRF (rvseg_crf_infer_terms), composed from the CPU oracle's lattice
(oracle.Lattice.compute, oracle.exp_and_normalize) and float32 numpy operations in the library's pinned orders:
every sum starts at its index-0 product and the index ascends, each product and add rounded on its own.

Restates DenseCRF::inference (densecrf.cpp:115-131) with DenseKernel::filter (pairwise.cpp:40-80, apply only), the
three label compatibilities (labelcompatibility.cpp:43-100), DenseKernel::setParameters (pairwise.cpp:140-152) and
LogisticUnaryEnergy::get (unary.cpp:50-52).  Test infrastructure only."""
import numpy as np

NO_NORMALIZATION, NORMALIZE_BEFORE, NORMALIZE_AFTER, NORMALIZE_SYMMETRIC = range(4)
CONST_KERNEL, DIAG_KERNEL, FULL_KERNEL = range(3)
POTTS, DIAGONAL, MATRIX = range(3)

f32 = np.float32


def ordered_sum(coeffs, cols):
    """sum_k coeffs[k] * cols[k] from k = 0 up, each product and add rounded to float32."""
    acc = f32(coeffs[0]) * cols[0]
    for k in range(1, len(coeffs)):
        acc = acc + f32(coeffs[k]) * cols[k]
    return acc.astype(f32)


def kernel_features(f, kernel_type, kernel_params):
    """The features a term's lattice is built on: DIAG f'[j] = p[j] f[j]; FULL f'[a] = sum_b P[a][b] f[b] with
    P[a][b] = p[b*d + a]; no parameters (or CONST): f as passed."""
    f = np.ascontiguousarray(f, f32)
    if kernel_params is None or kernel_type == CONST_KERNEL:
        return f
    p = np.asarray(kernel_params, f32).reshape(-1)
    d = f.shape[1]
    if kernel_type == DIAG_KERNEL:
        return (f * p[None, :]).astype(f32)
    out = np.empty_like(f)
    for a in range(d):
        out[:, a] = ordered_sum([p[b * d + a] for b in range(d)], [f[:, b] for b in range(d)])
    return out


def norm_of(lat, normalization):
    """pairwise.cpp:40-56: n = lattice.compute(ones); SYMMETRIC 1/sqrt(n + 1e-20), BEFORE / AFTER 1/(n + 1e-20), in double."""
    n = lat.compute(np.ones((lat.N, 1), f32))[:, 0].astype(np.float64)
    if normalization == NORMALIZE_SYMMETRIC:
        return (1.0 / np.sqrt(n + 1e-20)).astype(f32)
    return (1.0 / (n + 1e-20)).astype(f32)


def symmetrised(m):
    m = np.asarray(m, f32)
    return (f32(0.5) * (m + m.T)).astype(f32)


def compat_apply(compat, params, t):
    """out (N x C) of the compatibility on the filtered t."""
    C = t.shape[1]
    params = np.asarray(params, f32).reshape(-1)
    if compat == POTTS:
        return (f32(-params[0]) * t).astype(f32)
    if compat == DIAGONAL:
        return (params[None, :] * t).astype(f32)
    W = symmetrised(params.reshape(C, C))
    return ordered_sum([W[:, k][None, :] for k in range(C)], [t[:, k:k + 1] for k in range(C)])


def logistic_unary(L, f):
    """U[i][m] = sum_k L[m][k] f[i][k] (L: C x K, f: N x K)."""
    L = np.asarray(L, f32)
    f = np.asarray(f, f32)
    return np.stack([ordered_sum(list(L[m]), [f[:, k] for k in range(L.shape[1])]) for m in range(L.shape[0])], 1)


def crf_terms(oracle, U, terms, iterations):
    """Marginals of the mean field.  terms: [(features, compat, compat_params, kernel_type, normalization, kernel_params)]."""
    U = np.ascontiguousarray(U, f32)
    built = []
    for f, compat, cp, kt, nt, kp in terms:
        lat = oracle.Lattice(kernel_features(f, kt, kp))
        nrm = norm_of(lat, nt) if nt != NO_NORMALIZATION else None
        built.append((lat, nrm, compat, cp, nt))
    Q = oracle.exp_and_normalize(-U)
    for _ in range(iterations):
        tmp = -U
        for lat, nrm, compat, cp, nt in built:
            inp = (Q * nrm[:, None]).astype(f32) if nt in (NORMALIZE_SYMMETRIC, NORMALIZE_BEFORE) else Q
            t = lat.compute(inp)
            if nt in (NORMALIZE_SYMMETRIC, NORMALIZE_AFTER):
                t = (t * nrm[:, None]).astype(f32)
            tmp = (tmp - compat_apply(compat, cp, t)).astype(f32)
        Q = oracle.exp_and_normalize(tmp)
    return Q
