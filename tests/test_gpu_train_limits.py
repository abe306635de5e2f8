"""The forest trainer (csrc/rvseg_train.hip: rvseg_forest_train, rvseg_forest_train_frames) at every limit the code
switches path at, against the CPU oracle's learner BYTE FOR BYTE.  The recipes live in tests/train_cases.py; that each
one really crosses its edge is pinned on the CPU, from the oracle's file alone, by tests/test_train_cases_cpu.py.

  slot batches        levels wider than SLOT_BATCH = 1024 and than 2048 frontier nodes (two and three batches per level)
  layouts             1, 2, 9, 15, 16 classes per layer, 1..8 layers, 64 classes in all; 17 classes, 9 layers, 65 refused
  feature kinds       only byte features, only float features (num_features = D), D = 1, the edges of byte detection
  scan seams          segments of 1, 2, 63, 64, 65, 128, 129, 4097 values, best cut / tie run / near-tie run on a chunk seam
  thresholds          adjacent floats (the guard), negative values and the -2 sentinel, sums that overflow
  parameters          max_depth 1, min_split_examples 0, min_child_split_examples 0 and above P / 2, num_features 1 and D,
                      num_trees 1 and 64 (65 refused), smoothing 0
  degenerate sets     P = 1, P = 2, constant features, pure labels, an absent class, identical rows
  > 2^24 of a class   the stalled float counter of the inverted class frequency
  frames              augment off, no colour patch, no normal, stride 1 and 4, per-frame calibrations, an empty frame
  ABI                 buffer too small + rvseg_forest_train_result, result before training, NaN / inf, labels out of range

What the trainer does where the reference is silent, stated and tested here:
  * smoothing = 0 writes log(0) = -inf for the classes a leaf does not hold; rvseg_forest_check and the loader accept it;
  * finite values near +-3e38 whose sum overflows: the threshold is the right value (the guard of definition 4), never
    +-inf; the file is valid and loads.
"""
import ctypes as C

import numpy as np
import pytest

import train_cases as tc

pytestmark = pytest.mark.gpu

CTX = dict(width=160, height=120)


def _first_difference(got, want):
    tg, tw = tc.parse(got), tc.parse(want)
    assert len(tg) == len(tw), ("tree counts", len(tg), len(tw))
    for k, (a, b) in enumerate(zip(tg, tw)):
        assert len(a["left"]) == len(b["left"]), ("tree %d: node counts" % k, len(a["left"]), len(b["left"]))
        for name in ("left", "feat", "thr"):
            bad = np.flatnonzero(a[name].view(np.int32) != b[name].view(np.int32))
            assert bad.size == 0, ("tree %d: %s differs first at node %d" % (k, name, bad[0]), a[name][bad[0]], b[name][bad[0]])
    return "leaf histograms differ"


def _compare(ctx, oracle, c):
    import rovinasemanticsegmentation_amd as rv
    got = tc.train(ctx, c)
    want = tc.train(oracle, c)
    if got != want:
        raise AssertionError(_first_difference(got, want))
    st, msg, info = rv.capi.forest_check(got, c["X"].shape[1])
    assert st == rv.capi.OK, msg
    return got


@pytest.mark.parametrize("recipe", ["slot_batches", "slot_batches_three"])
def test_levels_wider_than_one_slot_batch(gpu_ctx_factory, oracle, recipe):
    """Each batch of a level re-uploads slot_of, zeroes the histograms again and reuses the cut records."""
    c = getattr(tc, recipe)()
    got = _compare(gpu_ctx_factory(**CTX), oracle, c)
    assert tc.level_widths(tc.parse(got)[0]).max() > (1 if recipe == "slot_batches" else 2) * tc.SLOT_BATCH


@pytest.mark.parametrize("name", list(tc.all_cases()))
def test_trainer_equals_the_oracle_on(gpu_ctx_factory, oracle, name):
    _compare(gpu_ctx_factory(**CTX), oracle, tc.all_cases()[name]())


def test_many_cases_on_one_context_in_both_orders(gpu_ctx_factory, oracle):
    """The trainer keeps nothing between calls but the last model: a wide case, a degenerate one, a float-only one and
    back, on one context."""
    ctx = gpu_ctx_factory(**CTX)
    cases = tc.all_cases()
    names = ["layout_16_16_16_16", "degenerate_P1_plain", "all_floats", "seam_P65_cut64", "layout_8_8_8_8_8_8_8_8", "all_bytes",
             "adjacent_16_cut5", "layout_16_16_16_16"]
    for name in names:
        _compare(ctx, oracle, cases[name]())


def test_loaded_models_with_infinite_histograms_and_huge_thresholds(gpu_ctx_factory, oracle):
    """smoothing = 0 and the +-3e38 case: the files load into a context (the loader accepts -inf histograms and huge
    finite thresholds) and come back unchanged from rvseg_forest_write_mem."""
    for c in (tc.params("smoothing_0"), tc.huge_values(1), tc.huge_values(-1)):
        ctx = gpu_ctx_factory(**CTX)
        blob = _compare(ctx, oracle, c)
        trees = tc.parse(blob)
        assert all(np.isfinite(t["thr"]).all() for t in trees)
        ctx.forest_load(blob)
        assert ctx.forest_write() == blob


def test_more_than_2_pow_24_examples_of_one_class(gpu_ctx_factory, oracle):
    """The `cn <= 16777216u` branch: the reference counts the class sizes with ++ on a float."""
    _compare(gpu_ctx_factory(**CTX), oracle, tc.many_examples())


# ---- refusals and the ABI ------------------------------------------------------------------------------------------
def _raw_train(ctx, X, labels, cc, out_cap=None, **kw):
    """rvseg_forest_train with a caller buffer of out_cap bytes (None: size query only): (status, size_out, bytes)."""
    X = np.ascontiguousarray(X, np.float32)
    labels = np.ascontiguousarray(np.asarray(labels, np.int32).reshape(X.shape[0], -1))
    tp = ctx._train_params(kw)
    ccv = (C.c_int32 * len(cc))(*cc)
    size = C.c_size_t(0)
    buf = C.create_string_buffer(max(out_cap or 0, 1)) if out_cap is not None else None
    st = ctx.L.rvseg_forest_train(ctx.h, X.ctypes.data_as(C.c_void_p), X.shape[0], X.shape[1], labels.ctypes.data_as(C.c_void_p),
                                  labels.shape[1], ccv, C.byref(tp), buf, out_cap or 0, C.byref(size))
    return st, size.value, (buf.raw[:out_cap] if buf is not None else None)


def _result(ctx, cap):
    buf = C.create_string_buffer(max(cap, 1))
    got = C.c_size_t(0)
    st = ctx.L.rvseg_forest_train_result(ctx.h, buf, cap, C.byref(got))
    return st, got.value, buf.raw[:cap]


def test_result_before_any_training_is_no_forest(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    ctx = gpu_ctx_factory(**CTX)
    st, _, _ = _result(ctx, 16)
    assert st == rv.capi.ERR_NO_FOREST
    size = C.c_size_t(0)
    assert ctx.L.rvseg_forest_train_result(ctx.h, None, 0, C.byref(size)) == rv.capi.ERR_NO_FOREST


def test_refused_layouts_and_parameters_keep_the_previous_model(gpu_ctx_factory, oracle):
    import rovinasemanticsegmentation_amd as rv
    ctx = gpu_ctx_factory(**CTX)
    c = tc.params("num_trees_1")
    before = tc.train(ctx, c)
    assert before == tc.train(oracle, c)
    P = c["X"].shape[0]
    for cc in tc.REFUSED_LAYOUTS:
        st, _, _ = _raw_train(ctx, c["X"], np.zeros((P, len(cc)), np.int32), cc)
        assert st == rv.capi.ERR_INVALID_ARG, cc
        st, size, blob = _result(ctx, len(before))
        assert st == rv.capi.OK and size == len(before) and blob == before, cc
    bad = [dict(num_trees=65), dict(num_trees=0), dict(max_depth=0), dict(min_split_examples=-1), dict(min_child_split_examples=-1),
           dict(num_features=-1), dict(num_features=c["X"].shape[1] + 1), dict(smoothing=-1.0), dict(smoothing=float("nan"))]
    for kw in bad:
        st, _, _ = _raw_train(ctx, c["X"], c["labels"], c["cc"], **kw)
        assert st == rv.capi.ERR_INVALID_ARG, kw
    st, size, blob = _result(ctx, len(before))
    assert st == rv.capi.OK and blob == before


def test_buffer_one_byte_too_small_keeps_the_model_for_train_result(gpu_ctx_factory, oracle):
    import rovinasemanticsegmentation_amd as rv
    c = tc.params("num_features_D")
    want = tc.train(oracle, c)
    ctx = gpu_ctx_factory(**CTX)
    st, size, _ = _raw_train(ctx, c["X"], c["labels"], c["cc"], out_cap=len(want) - 1, **c["kw"])
    assert st == rv.capi.ERR_INVALID_ARG and size == len(want)
    st, size, blob = _result(ctx, len(want) - 1)                  # still too small: refused, the size is reported again
    assert st == rv.capi.ERR_INVALID_ARG and size == len(want)
    st, size, blob = _result(ctx, len(want))
    assert st == rv.capi.OK and size == len(want) and blob == want
    st, size, blob = _raw_train(gpu_ctx_factory(**CTX), c["X"], c["labels"], c["cc"], out_cap=len(want), **c["kw"])   # a fresh call
    assert st == rv.capi.OK and size == len(want) and blob == want
    st, size, blob = _raw_train(ctx, c["X"], c["labels"], c["cc"], out_cap=len(want) + 5, **c["kw"])
    assert st == rv.capi.OK and size == len(want) and blob[:size] == want


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_features_are_refused(gpu_ctx_factory, value):
    import rovinasemanticsegmentation_amd as rv
    c = tc.params("num_trees_1")
    ctx = gpu_ctx_factory(**CTX)
    for row, col in ((0, 0), (c["X"].shape[0] - 1, c["X"].shape[1] - 1), (257, 2)):     # a byte column, the float column, mid-block
        X = c["X"].copy()
        X[row, col] = value
        st, _, _ = _raw_train(ctx, X, c["labels"], c["cc"], **c["kw"])
        assert st == rv.capi.ERR_INVALID_ARG, (row, col)
    st, _, _ = _result(ctx, 16)
    assert st == rv.capi.ERR_NO_FOREST                              # nothing was trained on the way


def test_labels_out_of_range_are_refused(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    c = tc.layout([2, 9, 15])
    ctx = gpu_ctx_factory(**CTX)
    for row, layer, value in ((0, 0, 2), (17, 1, 9), (c["X"].shape[0] - 1, 2, 15), (3, 1, -1), (3, 0, 2 ** 31 - 1), (3, 2, -2 ** 31)):
        lab = c["labels"].copy()
        lab[row, layer] = value
        st, _, _ = _raw_train(ctx, c["X"], lab, c["cc"], **c["kw"])
        assert st == rv.capi.ERR_INVALID_ARG, (row, layer, value)


# ---- training from frames ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.FRAME_CONFIGS))
def test_training_from_frames_equals_the_oracle(gpu_ctx_factory, oracle, name):
    """rvseg_forest_train_frames against the oracle's extraction followed by the oracle's learner, n_examples included."""
    import rovinasemanticsegmentation_amd as rv
    fr = tc.frames(name)
    ctx = gpu_ctx_factory(**fr["ctx_kw"])
    got, n_ex = ctx.forest_train_frames(fr["rgb"], fr["depth"], fr["calib"], fr["lab"], fr["cc"], augment=fr["augment"], **fr["kw"])
    X, Y, per_frame = tc.frames_dataset(oracle, fr)
    assert n_ex == X.shape[0]
    want = oracle.forest_train(X, Y, fr["cc"], **fr["kw"])
    if got != want:
        raise AssertionError(_first_difference(got, want))
    st, msg, _ = rv.capi.forest_check(got, X.shape[1])
    assert st == rv.capi.OK, msg
    assert max(len(t["left"]) for t in tc.parse(got)) > 20


def _raw_train_frames(ctx, fr, lab):
    tp = ctx._train_params(fr["kw"])
    ccv = (C.c_int32 * len(fr["cc"]))(*fr["cc"])
    size, n_ex = C.c_size_t(0), C.c_int32(-7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rgb, depth, calib, lab = (np.ascontiguousarray(a) for a in (fr["rgb"], fr["depth"], fr["calib"], lab))
    st = ctx.L.rvseg_forest_train_frames(ctx.h, rgb.shape[0], p(rgb), p(depth), p(calib), p(lab), len(fr["cc"]), ccv, 0, C.byref(tp),
                                         None, 0, C.byref(size), C.byref(n_ex))
    return st, n_ex.value


def test_frames_without_a_labelled_point_or_with_a_label_too_large_are_refused(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    fr = tc.frames("plain")
    ctx = gpu_ctx_factory(**fr["ctx_kw"])
    st, n_ex = _raw_train_frames(ctx, fr, np.full_like(fr["lab"], -1))
    assert st == rv.capi.ERR_INVALID_ARG and n_ex == 0
    lab = fr["lab"].copy()
    lab[:, 0][lab[:, 0] == 2] = 3                      # a label equal to its layer's class count
    st, n_ex = _raw_train_frames(ctx, fr, lab)
    assert st == rv.capi.ERR_INVALID_ARG and n_ex > 0
    st, _, _ = _result(ctx, 16)
    assert st == rv.capi.ERR_NO_FOREST
    st, n_ex = _raw_train_frames(ctx, fr, fr["lab"])   # and the context still trains
    assert st == rv.capi.OK and n_ex > 0
