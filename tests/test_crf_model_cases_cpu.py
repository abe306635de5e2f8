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

MODEL_SYMBOLS = ["rvseg_crf_model_" + n + sfx for n in ("set", "start", "step", "apply", "energy", "kl", "trace") for sfx in ("", "_device")]


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
