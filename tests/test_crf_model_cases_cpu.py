"""The restatement behind the kept-model tests (crf_model_cases.py) against crf_restate and against values worked out by
hand, and the library's exports.  No GPU."""
import ctypes
import math
import os

import numpy as np
import pytest

import crf_model_cases as M
import crf_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODEL_SYMBOLS = ["rvseg_crf_model_" + n + sfx for n in ("set", "start", "step", "apply", "energy", "kl", "trace") for sfx in ("", "_device")] + ["rvseg_crf_model_info"]


@pytest.mark.parametrize("specs", [
    [],
    [(5, R.MATRIX, R.NORMALIZE_SYMMETRIC)],
    [(2, R.POTTS, R.NORMALIZE_AFTER), (6, R.DIAGONAL, R.NORMALIZE_BEFORE), (3, R.MATRIX, R.NO_NORMALIZATION)],
])
def test_steps_are_the_inference(oracle, specs):
    _, U, terms = M.random_model(11 + len(specs), 300, 5, specs)
    model = M.Model(oracle, U, terms)
    Q = model.start()
    for n in range(4):
        assert np.array_equal(Q, R.crf_terms(oracle, U, terms, n))
        Q = model.step(Q)


def test_three_points_by_hand(oracle):
    """Three points with the SAME feature meet in one simplex with the same weights, so the normalised filter
    (NORMALIZE_SYMMETRIC) is the mean over the points: n_i = 3 K, norm = 1 / sqrt(3 K), filter(x)_i = K sum_j x_j / (3 K).
    Potts(2): apply(Q)_i[c] = -2 mean_j Q_j[c].  The filter rounds in fp32 (a few dozen operations): 1e-5 relative."""
    F = np.tile(np.array([[0.3, 0.7]], np.float32), (3, 1))
    U = np.array([[0.5, 1.5], [2.0, 0.25], [1.0, 3.0]], np.float32)
    model = M.Model(oracle, U, [(F, R.POTTS, [2.0], R.DIAG_KERNEL, R.NORMALIZE_SYMMETRIC, None)])
    labels = np.array([0, 1, -1], np.int8)   # one-hot rows (1, 0), (0, 1), (0, 0): mean (1/3, 1/3), apply = -2/3 everywhere
    assert np.array_equal(model.unary_energy(labels), np.array([0.5, 0.25, 0.0], np.float32))
    assert model.pairwise_energy(labels, 0) == pytest.approx([1 / 3, 1 / 3, 0.0], rel=1e-5)   # -0.5 * -2/3; label -1: 0
    assert np.array_equal(model.pairwise_energy(labels, -1), (np.float32(0) + model.pairwise_energy(labels, 0)).astype(np.float32))
    assert np.array_equal(model.pairwise_energy(np.array([2, 2, 2], np.int8), 0), np.zeros(3, np.float32))   # label C: 0
    Q = np.array([[0.5, 0.5], [0.25, 0.75], [1.0, 0.0]], np.float32)
    parts, S = model.kl_parts(Q)
    entropy = math.log(0.5) + 0.25 * math.log(0.25) + 0.75 * math.log(0.75)   # 1 log 1 = 0 and 0 log 1e-20 = 0
    unary = 0.5 * 0.5 + 1.5 * 0.5 + 2.0 * 0.25 + 0.25 * 0.75 + 1.0 * 1.0
    pair = -2 * (1.75 ** 2 + 1.25 ** 2) / 3   # sum_c (sum_i q_ic) * (-2 * sum_j q_jc / 3)
    assert parts[0] == pytest.approx(entropy, rel=1e-14)
    assert parts[1] == pytest.approx(unary, rel=1e-14)
    assert parts[2] == pytest.approx(pair, rel=1e-5)
    assert S[0] == pytest.approx(-entropy, rel=1e-14) and S[2] == pytest.approx(-pair, rel=1e-5)
    assert M.kl_sum(parts) == (parts[0] + parts[1]) + parts[2]


def test_library_exports_the_model_calls():
    lib = ctypes.CDLL(os.path.join(ROOT, "rovinasemanticsegmentation_amd", "librvseg.so"))
    for name in MODEL_SYMBOLS:
        assert hasattr(lib, name), name
    from rovinasemanticsegmentation_amd import _capi as capi
    assert set(MODEL_SYMBOLS) <= set(capi.SYMBOLS)


def test_model_calls_without_a_context_are_refused():
    from rovinasemanticsegmentation_amd import _capi as capi
    L = capi.lib()
    assert L.rvseg_crf_model_start(None, None) == capi.ERR_INVALID_ARG
    assert L.rvseg_crf_model_set(None, 1, 1, 0, None, None, 1) == capi.ERR_INVALID_ARG
    assert L.rvseg_crf_model_kl_device(None, None, None, None) == capi.ERR_INVALID_ARG
    info = capi.RvsegCrfModelInfo(serial=7, N=7)
    assert L.rvseg_crf_model_info(None, ctypes.byref(info)) == capi.ERR_INVALID_ARG and (info.serial, info.N) == (0, 0)   # zeroed first


def test_kl_entropy_at_the_clamp_by_hand(oracle):
    """clamp_q's rows: q = 0 adds 0 log 1e-20f = 0, q <= 1e-20f adds q log 1e-20f, the one-hot row adds 1 log 1 = 0; every
    element term is finite and the entropy is the plain sum of q log max(q, 1e-20f)."""
    N, C = 40, 5
    rng, U, terms = M.random_model(21, N, C, [(2, R.POTTS, R.NORMALIZE_SYMMETRIC)])
    Q = M.clamp_q(rng, N, C)
    lo = float(np.float32(1e-20))
    assert (Q == 0).sum() >= N // 3 and (Q == np.float32(1e-30)).sum() >= N // 5 and (Q == np.float32(1e-20)).any()
    assert (Q[N // 2] == np.eye(C, dtype=np.float32)[C // 2]).all()
    above = np.nextafter(np.float32(1e-20), np.float32(1))
    assert (Q == above).any() and float(above) > lo
    terms_by_hand = [float(q) * math.log(max(float(q), lo)) for q in Q.ravel()]
    assert all(math.isfinite(t) and t <= 0.0 for t in terms_by_hand)
    assert terms_by_hand[(N // 2) * C + C // 2] == 0.0 and terms_by_hand[0] == 0.0
    assert terms_by_hand[1 * C + C - 1] == pytest.approx(1e-30 * math.log(1e-20), rel=1e-7)   # (fp32 roundings of 1e-30, 1e-20)
    parts, S = M.Model(oracle, U, terms).kl_parts(Q)
    assert parts[0] == math.fsum(terms_by_hand) and S[0] == -parts[0] and np.isfinite(parts).all()


def test_energy_of_labels_at_the_edges_by_hand(oracle):
    """C = 64: label 63 reads the last column; 64, -1 and -128 are out of range and give 0 in both energies."""
    N, C = 8, 64
    _, U, terms = M.random_model(22, N, C, [(2, R.POTTS, R.NORMALIZE_SYMMETRIC)])
    model = M.Model(oracle, U, terms)
    labels = np.array([63, 64, -1, -128, 0, 63, 127, 5], np.int8)
    u, p = model.unary_energy(labels), model.pairwise_energy(labels, -1)
    assert np.array_equal(u, np.array([U[0, 63], 0, 0, 0, U[4, 0], U[5, 63], 0, U[7, 5]], np.float32))
    assert not p[[1, 2, 3, 6]].any() and p[[0, 4, 5, 7]].all()
    onehot = np.zeros((N, C), np.float32)
    onehot[[0, 4, 5, 7], [63, 0, 63, 5]] = 1.0
    assert p[5] == np.float32(-0.5) * model.apply(0, onehot)[5, 63]


def test_one_class_and_ten_parts(oracle):
    """C = 1: the marginals are all one, the entropy has no term (S = 0) and the unary part is the sum of U.  Eight terms:
    ten parts, added in order by kl_sum."""
    N = 30
    _, U, terms = M.random_model(23, N, 1, [(2, R.MATRIX, R.NORMALIZE_SYMMETRIC), (3, R.POTTS, R.NORMALIZE_AFTER)])
    model = M.Model(oracle, U, terms)
    Q = model.step(model.start())
    assert np.array_equal(Q, np.ones((N, 1), np.float32))
    parts, S = model.kl_parts(Q)
    assert parts[0] == 0.0 and S[0] == 0.0 and parts[1] == math.fsum(U.astype(np.float64).ravel())
    assert parts[3] == math.fsum(model.apply(1, Q).astype(np.float64).ravel()) and parts[3] < 0   # q = 1: the Potts apply itself
    specs = [(1 + k % 3, [R.POTTS, R.DIAGONAL, R.MATRIX][k % 3], k % 4) for k in range(8)]
    rng, U, terms = M.random_model(24, 50, 3, specs)
    parts, S = M.Model(oracle, U, terms).kl_parts(M.clamp_q(rng, 50, 3))
    assert parts.shape == S.shape == (10,) and (S > 0).all()
    kl = parts[0]
    for v in parts[1:]:
        kl = kl + v
    assert M.kl_sum(parts) == kl
