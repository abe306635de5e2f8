"""The forest tools on the GPU at the limits of their kernels (csrc/kernels_forest_tools.hip, rvseg_forest_tools.hip): forests
of distinct trees at every tree count and class sum of the lane arithmetic, the tie and NaN rule across class passes and
across lanes, the agreement counts at every pair count and tile edge, the confusion counts from 1 to 64 classes, and the
refit counts across a chunk and through the grid-stride loop.  The recipes and the restated values come from
tests/limits_tools_cases.py and are pinned to their edges in tests/test_limits_tools_cases_cpu.py.  Every comparison is
exact."""
import numpy as np
import pytest

import frame_cases as fc
import limits_tools_cases as lc
import tools_cases as tc
import train_cases as trc

pytestmark = pytest.mark.gpu

F32 = np.float32
_loaded = {}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx6(gpu_ctx_factory):
    ctx = gpu_ctx_factory(**lc.CTX_D6)
    assert ctx.feature_length == fc.EVAL_D
    return ctx


def _load(ctx6, T, S):
    """The distinct forest of (T, S) on the one 6-feature context (loaded again only when another was in between)."""
    if _loaded.get("now") != (T, S):
        ctx6.forest_load(lc.distinct(T, S))
        _loaded["now"] = (T, S)
        info = ctx6.forest_info()
        assert info["n_trees"] == T and info["class_counts"] == [S]
    return ctx6


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- votes and classify ------------------------------------------------------------------------------------------------
def _votes_case(ctx, X, want, layer=0):
    got = ctx.forest_classify(X, layer)
    assert got.dtype == np.int32 and np.array_equal(got, want["pred"])
    votes = ctx.forest_classify_trees(X, layer)
    assert votes.dtype == np.uint8 and votes.shape == want["votes"].shape and np.array_equal(votes, want["votes"])
    assert np.array_equal(ctx.forest_measure(X, layer=layer, want=("pred",))["pred"], want["pred"])


@pytest.mark.parametrize("T,S", lc.VOTE_CASES)
def test_votes_and_labels_of_distinct_trees(ctx6, T, S):
    _votes_case(_load(ctx6, T, S), lc.points(lc.VOTE_P), lc.restated(T, S, lc.VOTE_P))


@pytest.mark.parametrize("T,S", lc.POINT_COUNT_FORESTS)
def test_votes_and_labels_at_every_point_count(ctx6, T, S):
    ctx = _load(ctx6, T, S)
    for P in fc.POINT_COUNTS:
        _votes_case(ctx, lc.points(P), lc.restated(T, S, P))


def test_votes_and_labels_of_both_layers_of_a_two_layer_forest(gpu_ctx_factory):
    ctx = gpu_ctx_factory(multi_layer=1)
    ctx.forest_load(lc.two_layer_forest())
    assert ctx.forest_info()["class_counts"] == list(lc.TWO_LAYERS) and ctx.forest_info()["n_trees"] == 17
    for layer in (0, 1):
        _votes_case(ctx, tc.points(366, lc.VOTE_P), lc.two_layer_restated(layer), layer)


# ---- the tie and NaN rule on the wide paths ----------------------------------------------------------------------------
@pytest.mark.parametrize("T", [3, 6])
def test_tie_and_nan_rule_across_class_passes_and_lanes(gpu_ctx_factory, T):
    fo = lc.tie_forest(T)
    ctx = gpu_ctx_factory(**fo["ctx"])
    ctx.forest_load(fo["blob"])
    assert ctx.forest_info()["class_counts"] == [lc.TIE_C] and ctx.forest_info()["n_trees"] == T
    X, want = tc.points(4, lc.TIE_P), lc.tie_restated(T)
    _votes_case(ctx, X, want)
    pred = ctx.forest_classify(X)
    out = lc.tie_outcomes(lc.tie_sums(T))
    for name, label in lc.TIE_LABELS.items():       # outcome by outcome, so that a failure names the rule
        assert out[name].any() and (pred[out[name]] == label).all(), name
    assert not (pred[out["nan_at_16_only"]] == 16).any()
    assert np.array_equal(ctx.forest_eval(X), lc.tie_sums(T), equal_nan=True)   # the sums the outcomes are read from


# ---- agreement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,P", lc.AGREE_CASES)
def test_agreement_counts(ctx6, T, P):
    S = lc.agree_classes(T)
    ctx = _load(ctx6, T, S)
    want = tc.agreement_counts(lc.restated(T, S, P)["votes"])
    got = ctx.forest_measure(lc.points(P), want=("agree",))["agree"]
    assert got.dtype == np.uint64 and got.shape == (T, T) and np.array_equal(got, want)
    assert np.array_equal(got, got.T) and (np.diag(got) == P).all()


# ---- confusion ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", lc.CONFUSION_POINTS)
@pytest.mark.parametrize("C", lc.CONFUSION_CLASSES)
def test_confusion_counts(ctx6, C, P):
    ctx = _load(ctx6, lc.CONFUSION_T, C)
    want = lc.restated(lc.CONFUSION_T, C, P)
    labels = lc.confusion_labels(want["pred"], C)
    got = ctx.forest_measure(lc.points(P), labels, want=("pred", "confusion"))
    assert np.array_equal(got["pred"], want["pred"])
    assert got["confusion"].dtype == np.uint64 and got["confusion"].shape == (C, C)
    assert np.array_equal(got["confusion"], tc.confusion_counts(labels, want["pred"], C)) and got["confusion"].sum() == P


@pytest.mark.parametrize("P", lc.CONFUSION_POINTS)
def test_a_label_outside_64_classes_is_refused_and_nothing_written(ctx6, P):
    import rovinasemanticsegmentation_amd as rv
    T, C = lc.CONFUSION_T, 64
    ctx = _load(ctx6, T, C)
    X = lc.points(P)
    good = lc.confusion_labels(lc.restated(T, C, P)["pred"], C)
    for bad_value in (64, -1):
        bad = good.copy()
        bad[-1] = bad_value
        pred, conf, agree = np.full(P, -7, np.int32), np.full((C, C), 99, np.uint64), np.full((T, T), 99, np.uint64)
        st = ctx.L.rvseg_forest_measure(ctx.h, X.ctypes.data, P, fc.EVAL_D, bad.ctypes.data, 0, pred.ctypes.data, conf.ctypes.data, agree.ctypes.data)
        assert st == rv.capi.ERR_INVALID_ARG and b"label" in ctx.L.rvseg_last_error(ctx.h)
        assert (pred == -7).all() and (conf == 99).all() and (agree == 99).all(), bad_value
    assert np.array_equal(ctx.forest_measure(X, good)["confusion"], tc.confusion_counts(good, lc.restated(T, C, P)["pred"], C))


# ---- refit counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,S,P", lc.REFIT_CASES)
def test_refit_counts_across_a_chunk_and_through_the_grid_stride_loop(ctx6, T, S, P):
    assert T * min(P, 65536) > 4 * _cus() * 256, "this device's count grid does not loop over this case: the case needs more (tree, point) pairs"
    ctx = _load(ctx6, T, S)
    blob, X, labels = lc.distinct(T, S), lc.points(P), lc.refit_labels(P, S)
    refit, counts = ctx.forest_refit(X, labels, [S], smoothing=0.5, return_counts=True)
    assert counts.dtype == np.uint32 and np.array_equal(counts, tc._walk_counts(blob, X, labels, [S])) and counts.sum() == P * T
    assert ctx.forest_write() == blob                # the loaded model stays
    if P > 5000:
        return
    row = 0                                         # the small case: every leaf, recomputed in Python
    for tb, ta in zip(trc.parse(blob), trc.parse(refit)):
        assert all(np.array_equal(tb[k], ta[k]) for k in ("feat", "thr", "left"))
        for v in np.flatnonzero(ta["left"] == 0):
            want = tc._leaves_from_counts(counts[row + v], labels, [S], 0.5)
            assert len(ta["mhist"][v]) == 1 and np.array_equal(_bits(ta["mhist"][v][0]), _bits(want[0])), (row, v)
        row += len(ta["left"])
