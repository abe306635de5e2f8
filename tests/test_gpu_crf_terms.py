"""Learned DenseCRF models on the GPU (rvseg_crf_infer_terms[_device], rvseg_crf_logistic_unary[_device], Python
DenseCRF): every compatibility x normalisation, kernel parameters, the logistic unary and the dense_learning recipe,
each compared bit for bit with the restatement in crf_restate.py."""
import os

import numpy as np
import pytest

import crf_restate as R

pytestmark = pytest.mark.gpu

CLASS_COUNTS = [2, 3, 9, 12, 21, 11, 33, 64]   # fused class counts (2: the seqCompute path), then unfused ones
NORMS = [R.NO_NORMALIZATION, R.NORMALIZE_BEFORE, R.NORMALIZE_AFTER, R.NORMALIZE_SYMMETRIC]
COMPATS = [R.POTTS, R.DIAGONAL, R.MATRIX]
DS = [2, 5, 6]


def _compat_params(rng, compat, C):
    if compat == R.POTTS:
        return np.array([rng.uniform(0.5, 4.0)], np.float32)
    if compat == R.DIAGONAL:
        return (-rng.uniform(0.2, 4.0, C)).astype(np.float32)
    return (rng.uniform(-2.0, 2.0, (C, C))).astype(np.float32)   # not symmetric: the library symmetrises it


def _compat_obj(rv, compat, cp, C):
    if compat == R.POTTS:
        return rv.PottsCompatibility(cp[0])
    if compat == R.DIAGONAL:
        return rv.DiagonalCompatibility(cp)
    return rv.MatrixCompatibility(cp.reshape(C, C))


def _inputs(seed, N, C, d):
    rng = np.random.default_rng(seed)
    U = (rng.random((N, C)) * 3).astype(np.float32)
    F = (rng.random((N, d)) * 6).astype(np.float32)
    return rng, U, F


def _check(oracle, Q, mp, want, C, mode, unknown):
    assert np.array_equal(Q, want)
    assert np.array_equal(mp, oracle.labels(want, C, mode, unknown=unknown))


@pytest.mark.parametrize("C", CLASS_COUNTS)
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("compat", COMPATS)
def test_compat_x_normalisation(gpu_ctx_factory, oracle, compat, norm, C):
    import rovinasemanticsegmentation_amd as rv
    idx = COMPATS.index(compat) * 4 + norm
    d = DS[(idx + C) % 3]
    rng, U, F = _inputs(1000 + 37 * idx + C, 900, C, d)
    cp = _compat_params(rng, compat, C)
    mode, unknown = (idx + C) % 4, C - 1
    ctx = gpu_ctx_factory()
    Q, mp = ctx.crf_infer_terms(U, [(F, _compat_obj(rv, compat, cp, C), rv.DIAG_KERNEL, norm, None)], 5, mode, unknown)
    want = R.crf_terms(oracle, U, [(F, compat, cp, R.DIAG_KERNEL, norm, None)], 5)
    _check(oracle, Q, mp, want, C, mode, unknown)


@pytest.mark.parametrize("C", [2, 9, 33])
@pytest.mark.parametrize("iterations", [0, 1])
@pytest.mark.parametrize("compat", COMPATS)
def test_few_iterations_and_two_terms(gpu_ctx_factory, oracle, compat, iterations, C):
    import rovinasemanticsegmentation_amd as rv
    rng, U, F = _inputs(2000 + C + 7 * iterations + 13 * compat, 800, C, 5)
    F2 = (rng.random((800, 2)) * 9).astype(np.float32)
    cp = _compat_params(rng, compat, C)
    norm = NORMS[(C + iterations) % 4]
    ctx = gpu_ctx_factory()
    for terms in ([(F, compat, cp, R.DIAG_KERNEL, norm, None)],
                  [(F2, R.POTTS, np.array([1.5], np.float32), R.DIAG_KERNEL, R.NORMALIZE_AFTER, None),
                   (F, compat, cp, R.DIAG_KERNEL, norm, None)]):
        Q, mp = ctx.crf_infer_terms(U, [(f, _compat_obj(rv, c, p, C), kt, nt, kp) for f, c, p, kt, nt, kp in terms], iterations,
                                    1, 0)
        _check(oracle, Q, mp, R.crf_terms(oracle, U, terms, iterations), C, 1, 0)


@pytest.mark.parametrize("C", [9, 11, 21])
def test_potts_symmetric_is_unchanged(gpu_ctx_factory, oracle, C):
    """Potts + NORMALIZE_SYMMETRIC through the new entry is rvseg_crf_infer / rvseg_crf_infer_multi bit for bit, and
    Diagonal(-w, .., -w) is Potts(w) -- alone, and beside a Matrix term (the general loop)."""
    import rovinasemanticsegmentation_amd as rv
    rng, U, F = _inputs(3000 + C, 1200, C, 6)
    F2 = (rng.random((1200, 2)) * 9).astype(np.float32)
    ctx = gpu_ctx_factory()
    S = rv.NORMALIZE_SYMMETRIC
    Q1, m1 = ctx.crf_infer(U, F, 3.0, 5)
    Qt, mt = ctx.crf_infer_terms(U, [(F, 3.0, rv.DIAG_KERNEL, S, None)], 5)
    assert np.array_equal(Q1, Qt) and np.array_equal(m1, mt)
    Qd, _ = ctx.crf_infer_terms(U, [(F, rv.DiagonalCompatibility(np.full(C, -3.0)), rv.DIAG_KERNEL, S, None)], 5)
    assert np.array_equal(Q1, Qd)
    Qm, mm = ctx.crf_infer_multi(U, [F, F2], [3.0, 10.0], 5)
    Qt2, mt2 = ctx.crf_infer_terms(U, [(F, rv.PottsCompatibility(3.0), rv.DIAG_KERNEL, S, None), (F2, 10.0, rv.CONST_KERNEL, S, None)], 5)
    assert np.array_equal(Qm, Qt2) and np.array_equal(mm, mt2)
    assert np.array_equal(Qm, oracle.crf_inference_multi(U, [F, F2], [3.0, 10.0], 5))
    W = rng.uniform(-1, 1, (C, C)).astype(np.float32)
    a, _ = ctx.crf_infer_terms(U, [(F, rv.PottsCompatibility(3.0), rv.DIAG_KERNEL, S, None),
                                   (F2, rv.MatrixCompatibility(W), rv.DIAG_KERNEL, S, None)], 5)
    b, _ = ctx.crf_infer_terms(U, [(F, rv.DiagonalCompatibility(np.full(C, -3.0)), rv.DIAG_KERNEL, S, None),
                                   (F2, rv.MatrixCompatibility(W), rv.DIAG_KERNEL, S, None)], 5)
    assert np.array_equal(a, b)
    want = R.crf_terms(oracle, U, [(F, R.POTTS, [3.0], R.DIAG_KERNEL, S, None), (F2, R.MATRIX, W, R.DIAG_KERNEL, S, None)], 5)
    assert np.array_equal(a, want)


@pytest.mark.parametrize("unary_is_energy", [0, 1])
@pytest.mark.parametrize("C", [9, 33])
def test_device_entry_on_a_caller_stream(gpu_ctx_factory, oracle, unary_is_energy, C):
    """rvseg_crf_infer_terms_device on torch buffers and a torch stream; the second context's tiny hash capacity forces
    the overflow retry at the safe capacity."""
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    dev = torch.device("cuda", 0)
    rng, U, F = _inputs(4000 + C + unary_is_energy, 1500, C, 6)
    F2 = (rng.random((1500, 5)) * 5).astype(np.float32)
    cp = _compat_params(rng, R.MATRIX, C)
    kp = np.array([0.5, 2.0, 1.0, 1.5, 0.75], np.float32)
    terms = [(F, R.MATRIX, cp, R.DIAG_KERNEL, R.NORMALIZE_AFTER, None),
             (F2, R.DIAGONAL, _compat_params(rng, R.DIAGONAL, C), R.DIAG_KERNEL, R.NORMALIZE_BEFORE, kp)]
    want = R.crf_terms(oracle, U, terms, 4)
    stream = torch.cuda.Stream(dev)
    for ctx in (gpu_ctx_factory(), gpu_ctx_factory(lattice_capacity_log2=4)):
        d_U = torch.from_numpy(U if unary_is_energy else -U).to(dev)
        d_F = [torch.from_numpy(f).to(dev) for f in (F, F2)]
        d_Q = torch.zeros((1500, C), dtype=torch.float32, device=dev)
        d_map = torch.full((1500,), -99, dtype=torch.int8, device=dev)
        torch.cuda.synchronize(dev)
        dterms = [((t.data_ptr(), f.shape[1]), _compat_obj(rv, c, p, C), kt, nt, k)
                  for t, (f, c, p, kt, nt, k) in zip(d_F, terms)]
        ctx.crf_infer_terms_device(1500, C, dterms, d_U.data_ptr(), unary_is_energy, 4, d_Q.data_ptr(), d_map.data_ptr(),
                                   3, 0, stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(d_Q.cpu().numpy(), want)
        assert np.array_equal(d_map.cpu().numpy(), oracle.labels(want, C, 3))
        # labels only
        d_map2 = torch.full((1500,), -99, dtype=torch.int8, device=dev)
        ctx.crf_infer_terms_device(1500, C, dterms, d_U.data_ptr(), unary_is_energy, 4, 0, d_map2.data_ptr(), 1, C - 1,
                                   stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(d_map2.cpu().numpy(), oracle.labels(want, C, 1, unknown=C - 1))


@pytest.mark.parametrize("kernel_type", [R.DIAG_KERNEL, R.FULL_KERNEL])
@pytest.mark.parametrize("d", [2, 5, 6])
def test_kernel_parameters(gpu_ctx_factory, oracle, kernel_type, d):
    import rovinasemanticsegmentation_amd as rv
    C = 9
    rng, U, F = _inputs(5000 + d + 10 * kernel_type, 1000, C, d)
    if kernel_type == R.DIAG_KERNEL:
        kp = rng.uniform(0.3, 2.0, d).astype(np.float32)
    else:
        kp = (np.eye(d) + rng.uniform(-0.3, 0.3, (d, d))).astype(np.float32).reshape(-1)
    cp = _compat_params(rng, R.MATRIX, C)
    ctx = gpu_ctx_factory()
    crf = rv.DenseCRF(ctx, 1000, C)
    crf.setUnaryEnergy(U)
    crf.addPairwiseEnergy(F, rv.MatrixCompatibility(cp), kernel_type)
    crf.setKernelParameters(kp)
    Q, mp = crf.inference(3)
    want = R.crf_terms(oracle, U, [(F, R.MATRIX, cp, kernel_type, R.NORMALIZE_SYMMETRIC, kp)], 3)
    _check(oracle, Q, mp, want, C, 3, 0)
    # a Potts term with kernel parameters leaves the Potts-only path but computes the same as the transformed features
    Qp, _ = ctx.crf_infer_terms(U, [(F, rv.PottsCompatibility(2.0), kernel_type, rv.NORMALIZE_SYMMETRIC, kp)], 3)
    assert np.array_equal(Qp, oracle.crf_inference(U, R.kernel_features(F, kernel_type, kp), 2.0, 3))


def test_logistic_unary(gpu_ctx_factory):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(6000)
    N, C, K = 5000, 21, 4
    L = rng.uniform(-1, 1, (C, K)).astype(np.float32)
    f = rng.random((N, K)).astype(np.float32)
    ctx = gpu_ctx_factory()
    want = R.logistic_unary(L, f)
    assert np.array_equal(ctx.crf_logistic_unary(L, f), want)
    dev = torch.device("cuda", 0)
    d_f = torch.from_numpy(f).to(dev)
    d_U = torch.zeros((N, C), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.crf_logistic_unary_device(N, L, d_f.data_ptr(), d_U.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_U.cpu().numpy(), want)


def dense_learning_inputs(golden_dir, M=5):
    """The model of examples/dense_learning.cpp:113-133 with fixed parameters in place of the learnt ones: logistic unary on
    (r, g, b) / 255 and a constant 1, a Gaussian Potts(1) term and a bilateral Matrix term with DIAG kernel parameters."""
    from test_oracle_crf import read_ppm
    im = read_ppm(os.path.join(golden_dir, "im2.ppm"))
    H, W, _ = im.shape
    N = W * H
    rng = np.random.default_rng(2013)
    feat = np.ones((N, 4), np.float32)
    feat[:, :3] = (im.reshape(N, 3) / 255.).astype(np.float32)
    L = (0.5 * (1 - 2 * rng.random((M, 4)))).astype(np.float32)
    m = (np.eye(M) * -1.0 + 0.25 * (np.ones((M, M)) - np.eye(M))).astype(np.float32)
    m[0, 1] = m[1, 0] = 0.8   # symmetric, not the identity
    kp_bil = np.array([1.2, 0.8, 1.1, 0.9, 1.3], np.float32)
    return im, W, H, N, L, feat, m, kp_bil


def test_dense_learning_recipe_through_python(gpu_ctx_factory, oracle, golden_dir):
    import rovinasemanticsegmentation_amd as rv
    im, W, H, N, L, feat, m, kp_bil = dense_learning_inputs(golden_dir)
    M = L.shape[0]
    ctx = gpu_ctx_factory()
    crf = rv.DenseCRF(ctx, N, M)
    crf.setUnaryEnergy(L, feat)
    crf.addPairwiseGaussian(W, H, 3, 3, rv.PottsCompatibility(1))
    crf.addPairwiseBilateral(W, H, 80, 80, 13, 13, 13, im, rv.MatrixCompatibility(m))
    # the three lines dense_learning.cpp:177-179 prints, pasted back in
    crf.setUnaryParameters(crf.unaryParameters())
    crf.setLabelCompatibilityParameters(crf.labelCompatibilityParameters())
    crf.setKernelParameters(np.concatenate([np.ones(2, np.float32), kp_bil]))
    mp = crf.map(5)
    U = R.logistic_unary(L, feat)
    fg = rv.capi.crf_features_gaussian(W, H, 3, 3)
    fb = rv.capi.crf_features_bilateral(W, H, 80, 80, 13, 13, 13, im)
    want = R.crf_terms(oracle, U, [(fg, R.POTTS, [1.0], R.DIAG_KERNEL, R.NORMALIZE_SYMMETRIC, np.ones(2, np.float32)),
                                   (fb, R.MATRIX, m, R.DIAG_KERNEL, R.NORMALIZE_SYMMETRIC, kp_bil)], 5)
    assert np.array_equal(mp, oracle.labels(want, M, 3))
    Q, _ = crf.inference(5)
    assert np.array_equal(Q, want)
    assert len(np.unique(mp)) > 1


class _RawMatrix:
    """A Matrix compatibility handed to the C ABI as it is (MatrixCompatibility symmetrises on the Python side already)."""
    kind = R.MATRIX

    def __init__(self, m):
        self.m = np.ascontiguousarray(m, np.float32)

    def array(self, M):
        return self.m


@pytest.mark.parametrize("C", [9, 33])
def test_library_symmetrises_a_raw_matrix(gpu_ctx_factory, oracle, C):
    """rvseg_crf_term.compat_params of a Matrix term is m itself; the library uses W = 0.5 (m + m^T)."""
    import rovinasemanticsegmentation_amd as rv
    rng, U, F = _inputs(7000 + C, 900, C, 5)
    m = rng.uniform(-2.0, 2.0, (C, C)).astype(np.float32)
    assert not np.array_equal(m, m.T)
    ctx = gpu_ctx_factory()
    Q, _ = ctx.crf_infer_terms(U, [(F, _RawMatrix(m), rv.DIAG_KERNEL, rv.NORMALIZE_SYMMETRIC, None)], 3)
    assert np.array_equal(Q, R.crf_terms(oracle, U, [(F, R.MATRIX, m, R.DIAG_KERNEL, R.NORMALIZE_SYMMETRIC, None)], 3))
    Qs, _ = ctx.crf_infer_terms(U, [(F, rv.MatrixCompatibility(m), rv.DIAG_KERNEL, rv.NORMALIZE_SYMMETRIC, None)], 3)
    assert np.array_equal(Q, Qs)


@pytest.mark.parametrize("d", [1, 3, 4, 7])
@pytest.mark.parametrize("C", [9, 11])
def test_generic_dimensions(gpu_ctx_factory, oracle, d, C):
    """Feature dimensions without a dedicated normaliser slice (the generic reciprocal form of NORMALIZE_BEFORE / _AFTER)
    and FULL / DIAG kernel parameters at d = 1, 3, 4, 7; C = 9 takes the fused single-term update, C = 11 the general loop."""
    import rovinasemanticsegmentation_amd as rv
    rng, U, F = _inputs(8000 + 10 * d + C, 1000, C, d)
    full = (np.eye(d) + rng.uniform(-0.3, 0.3, (d, d))).astype(np.float32).reshape(-1)
    diag = rng.uniform(0.5, 1.5, d).astype(np.float32)
    cp = _compat_params(rng, R.MATRIX, C)
    ctx = gpu_ctx_factory()
    for norm, kt, kp in ((R.NORMALIZE_BEFORE, R.FULL_KERNEL, full), (R.NORMALIZE_AFTER, R.DIAG_KERNEL, diag)):
        Q, mp = ctx.crf_infer_terms(U, [(F, rv.MatrixCompatibility(cp), kt, norm, kp)], 4, 3, 0)
        want = R.crf_terms(oracle, U, [(F, R.MATRIX, cp, kt, norm, kp)], 4)
        _check(oracle, Q, mp, want, C, 3, 0)
