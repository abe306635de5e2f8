"""Host-only scoring (rvseg_eval_scores_from_counts) against a line-by-line transcription of the reference's score block,
src/test.cpp:203-228 (test_multi.cpp:243-268): np.float32 for its `float` accumulators and casts, Python floats for its
double expressions.  Bit-for-bit equality, no GPU."""
import math

import numpy as np
import pytest


def reference_scores(counts):
    """test.cpp:203-228 restated.  counts: C x C (row = ground truth); the reference's class_count / vote_count /
    total are the row sums, column sums and grand total of label_count (:187-193)."""
    C = counts.shape[0]
    label_count = [int(v) for v in counts.ravel()]
    class_count = [sum(label_count[i * C:(i + 1) * C]) for i in range(C)]
    vote_count = [sum(label_count[j::C]) for j in range(C)]
    total = sum(label_count)
    total_acc = 0
    avg_acc = np.float32(0)
    iou = np.float32(0)
    row_pct = []
    l = 0
    for i in range(C):
        for j in range(C):
            if i == j:
                total_acc += label_count[l]
                # float += double: the double sum, rounded to float
                avg_acc = np.float32(float(avg_acc) + 100.0 * float(np.float32(label_count[l])) / float(class_count[i] if class_count[i] else 1))
                x = class_count[i] + vote_count[i] - label_count[l]
                iou = np.float32(float(iou) + 100.0 * float(np.float32(label_count[l])) / float(x if x else 1))
            row_pct.append(100.0 * float(np.float32(label_count[l])) / float(class_count[i] if class_count[i] else 1))
            l += 1
    glob = 100.0 * float(np.float32(total_acc)) / total if total else math.nan   # 0.0 / 0 in C++: NaN
    return glob, np.float32(avg_acc / np.float32(C)), np.float32(iou / np.float32(C)), np.array(row_pct).reshape(C, C)


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _check(counts):
    from rovinasemanticsegmentation_amd import _capi as capi
    got = capi.eval_scores_from_counts(counts)
    g, a, u, row = reference_scores(np.asarray(counts, np.uint64))
    assert _same(got["global_acc"], g), (got["global_acc"], g)
    assert np.float32(got["class_avg_acc"]).tobytes() == a.tobytes()
    assert np.float32(got["iou"]).tobytes() == u.tobytes()
    assert got["row_pct"].tobytes() == row.tobytes()


@pytest.mark.parametrize("C", [1, 8, 9, 64])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_scores_equal_the_reference_formulas(C, seed):
    rng = np.random.default_rng(seed * 100 + C)
    counts = rng.integers(0, 100000, size=(C, C)).astype(np.uint64)
    counts[np.diag_indices(C)] += rng.integers(0, 10 ** 6, size=C).astype(np.uint64)    # mostly on the diagonal
    _check(counts)


@pytest.mark.parametrize("C", [8, 9, 64])
def test_empty_classes(C):
    rng = np.random.default_rng(C)
    counts = rng.integers(0, 5000, size=(C, C)).astype(np.uint64)
    counts[1] = 0                 # a class never in the ground truth
    counts[:, 2] = 0              # a class never predicted
    counts[3] = 0
    counts[:, 3] = 0              # neither
    _check(counts)


@pytest.mark.parametrize("C", [1, 9])
def test_empty_matrix_gives_nan_global_accuracy(C):
    from rovinasemanticsegmentation_amd import _capi as capi
    counts = np.zeros((C, C), np.uint64)
    _check(counts)
    s = capi.eval_scores_from_counts(counts)
    assert math.isnan(s["global_acc"]) and s["class_avg_acc"] == 0.0 and s["iou"] == 0.0


@pytest.mark.parametrize("C", [2, 9, 64])
def test_counts_above_2_pow_31(C):
    rng = np.random.default_rng(31 + C)
    counts = rng.integers(0, 1 << 33, size=(C, C), dtype=np.uint64)
    counts[np.diag_indices(C)] += np.uint64(1 << 40) + rng.integers(0, 1 << 20, size=C).astype(np.uint64)
    _check(counts)


def test_scores_of_a_known_matrix():
    from rovinasemanticsegmentation_amd import _capi as capi
    s = capi.eval_scores_from_counts(np.array([[3, 1], [0, 4]], np.uint64))
    assert s["global_acc"] == 100.0 * 7 / 8
    assert s["class_avg_acc"] == np.float32((np.float32(75.0) + 100.0) / 2)
    assert s["iou"] == np.float32((np.float32(75.0) + 80.0) / 2)     # class 0: 3 / (4 + 3 - 3), class 1: 4 / (4 + 5 - 4)


def test_bad_arguments():
    import ctypes as C
    from rovinasemanticsegmentation_amd import _capi as capi
    assert capi.lib().rvseg_eval_scores_from_counts(None, 3, None, None, None, None) == capi.ERR_INVALID_ARG
    z = np.zeros(4, np.uint64)
    assert capi.lib().rvseg_eval_scores_from_counts(z.ctypes.data_as(C.c_void_p), 0, None, None, None, None) == capi.ERR_INVALID_ARG
