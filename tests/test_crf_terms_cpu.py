"""CPU checks of the learned-model DenseCRF (rvseg_crf_infer_terms): the restatement in crf_restate.py against the
oracle, the parameter packings of the reference's loops, rvseg_crf_terms_check and the ctypes mirror of
rvseg_crf_term.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crf_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from rovinasemanticsegmentation_amd import _capi as capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return capi


def _features(rng, N, d, scale):
    return (rng.random((N, d)) * scale).astype(np.float32)


@pytest.mark.parametrize("C", [2, 9, 21])
@pytest.mark.parametrize("n_terms", [1, 2])
def test_restatement_equals_oracle_for_potts_symmetric(oracle, C, n_terms):
    """Potts + NORMALIZE_SYMMETRIC composed from the oracle's lattice is the oracle's own mean field, bit for bit."""
    rng = np.random.default_rng(100 + C * 3 + n_terms)
    N = 700
    U = (rng.random((N, C)) * 3).astype(np.float32)
    feats = [_features(rng, N, 2, 12.0), _features(rng, N, 5, 6.0)][:n_terms]
    ws = [3.0, 10.0][:n_terms]
    want = oracle.crf_inference_multi(U, feats, ws, 3)
    got = R.crf_terms(oracle, U, [(f, R.POTTS, [w], R.DIAG_KERNEL, R.NORMALIZE_SYMMETRIC, None) for f, w in zip(feats, ws)], 3)
    assert np.array_equal(got, want)
    # Diagonal(-w, .., -w) is Potts(w)
    got_d = R.crf_terms(oracle, U, [(f, R.DIAGONAL, np.full(C, -w, np.float32), R.DIAG_KERNEL, R.NORMALIZE_SYMMETRIC, None)
                                    for f, w in zip(feats, ws)], 3)
    assert np.array_equal(got_d, want)


def test_restatement_normaliser_forms(oracle):
    rng = np.random.default_rng(5)
    F = _features(rng, 500, 3, 8.0)
    lat = oracle.Lattice(F)
    assert np.array_equal(R.norm_of(lat, R.NORMALIZE_SYMMETRIC), lat.norm())
    n = lat.compute(np.ones((500, 1), np.float32))[:, 0]
    before = R.norm_of(lat, R.NORMALIZE_BEFORE)
    assert before.dtype == np.float32
    assert np.array_equal(before, np.array([np.float32(1.0 / (float(x) + 1e-20)) for x in n], np.float32))


def test_matrix_compatibility_packing_by_hand():
    import rovinasemanticsegmentation_amd as rv
    m = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.float32)
    mc = rv.MatrixCompatibility(m)
    # w_ = 0.5 * (m + m^T) (labelcompatibility.cpp:79); parameters: for i, for j >= i: w_(i, j) (:88-93)
    assert np.array_equal(mc.W, np.array([[1, 3, 5], [3, 5, 7], [5, 7, 9]], np.float32))
    assert mc.parameters().tolist() == [1, 3, 5, 5, 7, 9]
    mc.setParameters([10, 11, 12, 13, 14, 15])   # :95-100: w_(j, i) = w_(i, j) = v[k]
    assert mc.W.tolist() == [[10, 11, 12], [11, 13, 14], [12, 14, 15]]
    assert R.symmetrised(mc.W).tolist() == mc.W.tolist()


def test_kernel_and_unary_packings_by_hand(oracle):
    import rovinasemanticsegmentation_amd as rv
    # FULL kernel: parameters_ is d x d, resized column-major (pairwise.cpp:145-149): P[a][b] = p[b*d + a]
    f = np.array([[1, 10], [2, 20]], np.float32)
    got = R.kernel_features(f, R.FULL_KERNEL, [1, 2, 3, 4])      # P = [[1, 3], [2, 4]]
    assert got.tolist() == [[1 * 1 + 3 * 10, 2 * 1 + 4 * 10], [1 * 2 + 3 * 20, 2 * 2 + 4 * 20]]
    assert R.kernel_features(f, R.DIAG_KERNEL, [2, 0.5]).tolist() == [[2, 5], [4, 10]]
    assert R.kernel_features(f, R.CONST_KERNEL, [2, 0.5]) is not None
    assert np.array_equal(R.kernel_features(f, R.CONST_KERNEL, [2, 0.5]), f)
    # logistic: L_ resized column-major (unary.cpp:53-63): v[k*M + m] = L[m][k]
    crf = rv.DenseCRF(None, 2, 2)
    L = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    crf.setUnaryEnergy(L, np.ones((2, 3), np.float32))
    assert crf.unaryParameters().tolist() == [1, 4, 2, 5, 3, 6]
    crf.setUnaryParameters([6, 5, 4, 3, 2, 1])
    assert crf.logistic[0].tolist() == [[6, 4, 2], [5, 3, 1]]
    assert R.logistic_unary(L, np.array([[1, 1, 1], [1, 0, 2]], np.float32)).tolist() == [[6, 15], [7, 16]]


def test_term_concatenation_order():
    """labelCompatibilityParameters / kernelParameters concatenate the terms in the order they were added
    (densecrf.cpp:307-360); DIAG defaults to ones, FULL to the identity, CONST has none."""
    import rovinasemanticsegmentation_amd as rv
    W, H = 4, 3
    im = np.arange(W * H * 3, dtype=np.uint8).reshape(H, W, 3)
    crf = rv.DenseCRF(None, W * H, 3)
    crf.addPairwiseGaussian(W, H, 3, 3, rv.PottsCompatibility(1))
    crf.addPairwiseBilateral(W, H, 80, 80, 13, 13, 13, im, rv.MatrixCompatibility(np.eye(3) * 2), rv.FULL_KERNEL)
    crf.addPairwiseEnergy(np.zeros((W * H, 1), np.float32), rv.DiagonalCompatibility([1, 2, 3]), rv.CONST_KERNEL)
    assert crf.labelCompatibilityParameters().tolist() == [1, 2, 0, 0, 2, 0, 2, 1, 2, 3]
    kp = crf.kernelParameters()
    assert kp.tolist() == [1, 1] + np.eye(5).reshape(-1).tolist()
    v = np.arange(2 + 25, dtype=np.float32)
    crf.setKernelParameters(v)
    assert crf.kernels[0][4].tolist() == [0, 1]
    assert crf.kernels[1][4].tolist() == list(range(2, 27))
    assert crf.kernels[2][4] is None
    assert np.array_equal(crf.kernelParameters(), v)
    crf.setLabelCompatibilityParameters(np.arange(10, dtype=np.float32))
    assert crf.kernels[0][1].w == 0
    assert crf.kernels[1][1].W.tolist() == [[1, 2, 3], [2, 4, 5], [3, 5, 6]]
    assert crf.kernels[2][1].v.tolist() == [7, 8, 9]


_BUF = np.zeros(64 * 64, np.float32)


def _term(d=2, compat=0, kernel_type=1, normalization=3, features=True, compat_params=True, kernel_params=False):
    capi = _lib()
    buf = _BUF
    t = capi.RvsegCrfTerm()
    t.d, t.compat, t.kernel_type, t.normalization = d, compat, kernel_type, normalization
    t.features = buf.ctypes.data if features else None
    t.compat_params = buf.ctypes.data if compat_params else None
    t.kernel_params = buf.ctypes.data if kernel_params else None
    return t


def test_terms_check_refuses_each_bad_field():
    capi = _lib()
    ok = capi.OK
    bad = capi.ERR_INVALID_ARG
    assert capi.crf_terms_check(10, 9, [_term()]) == ok
    assert capi.crf_terms_check(10, 9, []) == ok
    assert capi.crf_terms_check(10, 64, [_term(d=7, compat=2, kernel_type=2, normalization=0, kernel_params=True)]) == ok
    assert capi.crf_terms_check(10, 1, [_term(d=1, compat=1, kernel_type=0, normalization=1)]) == ok
    assert capi.crf_terms_check(10, 9, [_term()] * 8) == ok
    assert capi.crf_terms_check(10, 9, [_term()] * 9) == bad
    assert capi.crf_terms_check(0, 9, [_term()]) == bad
    assert capi.crf_terms_check(10, 0, [_term()]) == bad
    assert capi.crf_terms_check(10, 65, [_term()]) == bad
    for kw in (dict(d=0), dict(d=8), dict(compat=-1), dict(compat=3), dict(kernel_type=-1), dict(kernel_type=3),
               dict(normalization=-1), dict(normalization=4), dict(features=False), dict(compat_params=False)):
        assert capi.crf_terms_check(10, 9, [_term(), _term(**kw)]) == bad, kw
    assert capi.lib().rvseg_crf_terms_check(10, 9, 1, None) == bad
    assert capi.lib().rvseg_crf_terms_check(10, 9, -1, None) == bad


def test_term_struct_mirrors_the_header_field_by_field():
    capi = _lib()
    hdr = open(os.path.join(ROOT, "include", "rvseg.h")).read()
    body = re.search(r"typedef struct rvseg_crf_term \{(.*?)\} rvseg_crf_term;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(int32_t|const float \*)\s*([^;]+);", body):
        for n in names.split(","):
            n = n.strip().lstrip("*").strip()
            fields.append((n, C.c_int32 if typ == "int32_t" else C.c_void_p))
    assert [f[0] for f in capi.RvsegCrfTerm._fields_] == [f[0] for f in fields]
    assert [f[1] for f in capi.RvsegCrfTerm._fields_] == [f[1] for f in fields]
    assert C.sizeof(capi.RvsegCrfTerm) == 16 + 3 * C.sizeof(C.c_void_p)
    for enum, names in (("rvseg_norm_kind", ["NO_NORMALIZATION", "NORMALIZE_BEFORE", "NORMALIZE_AFTER", "NORMALIZE_SYMMETRIC"]),
                        ("rvseg_kernel_kind", ["CONST_KERNEL", "DIAG_KERNEL", "FULL_KERNEL"]),
                        ("rvseg_compat_kind", ["COMPAT_POTTS", "COMPAT_DIAGONAL", "COMPAT_MATRIX"])):
        ebody = re.search(r"typedef enum %s \{(.*?)\} %s;" % (enum, enum), hdr, re.S).group(1)
        vals = dict((k, int(v)) for k, v in re.findall(r"RVSEG_(\w+)\s*=\s*(\d+)", ebody))
        assert vals == {n: getattr(capi, n) for n in names}
    import rovinasemanticsegmentation_amd as rv
    assert (rv.NO_NORMALIZATION, rv.NORMALIZE_BEFORE, rv.NORMALIZE_AFTER, rv.NORMALIZE_SYMMETRIC) == (0, 1, 2, 3)
    assert (rv.CONST_KERNEL, rv.DIAG_KERNEL, rv.FULL_KERNEL) == (0, 1, 2)
