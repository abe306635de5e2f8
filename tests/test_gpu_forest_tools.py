"""The forest tools on the GPU (rvseg_forest_classify / _classify_trees / _measure / _refit and the Python tool classes)
against the numpy restatement of tests/tools_cases.py and, where it is built, the reference's compiled evaluator.  Every
comparison is exact.  The recipes are pinned on the CPU in tests/test_tools_cases_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import boost_restate as br
import tools_cases as tc
import train_cases as trc
from tools_cases import _leaves_from_counts, _walk_counts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libforest_ref")
F32 = np.float32
_ctxs = {}

HEADS = [(name, layer) for name in tc.FORESTS for layer in tc.forest(name)["layers"]]


def _ctx(gpu_ctx_factory, name):
    """One context per forest of the recipes, with the forest loaded."""
    if name not in _ctxs:
        fo = tc.forest(name)
        ctx = gpu_ctx_factory(**fo["ctx"])
        ctx.forest_load(fo["blob"])
        _ctxs[name] = ctx
    return _ctxs[name]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- classify and votes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layer", HEADS)
def test_classify_and_tree_votes_equal_the_restatement(gpu_ctx_factory, name, layer):
    ctx = _ctx(gpu_ctx_factory, name)
    D = tc.forest(name)["D"]
    T = ctx.forest_info()["n_trees"]
    for P in tc.POINT_COUNTS + ((tc.CHUNK_TAIL,) if name == "tiny" else ()):   # tiny: also one chunk and a ragged tail
        X, want = tc.points(D, P), tc.restate(name, P, layer)
        got = ctx.forest_classify(X, layer)
        assert got.dtype == np.int32 and np.array_equal(got, want["pred"]), P
        votes = ctx.forest_classify_trees(X, layer)
        assert votes.shape == (T, P) and np.array_equal(votes, want["votes"]), P
    # ... and the label rule on the evaluator's own output
    X = tc.points(D, 1000)
    cc = ctx.forest_info()["class_counts"]
    off = int(np.sum(cc[:layer]))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(ctx.forest_classify(X, layer), br.first_strict_max(ctx.forest_eval(X)[:, off:off + cc[layer]]))


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference's evaluator is not built here")
@pytest.mark.parametrize("name", ["tiny", "single"])
def test_tree_votes_equal_the_reference_evaluator(gpu_ctx_factory, tmp_path, name):
    fo = tc.forest(name)
    X = tc.points(fo["D"], 1000)
    got = _ctx(gpu_ctx_factory, name).forest_classify_trees(X)
    (tmp_path / "x.f32").write_bytes(np.ascontiguousarray(X, F32).tobytes())
    for t, tree in enumerate(br.split_trees(fo["blob"])):
        (tmp_path / "t.dat").write_bytes(br.one_tree_forest(tree))
        subprocess.check_call([REF, "eval", str(tmp_path / "t.dat"), str(tmp_path / "x.f32"), str(fo["D"]), "single", str(tmp_path / "o.f32")],
                              timeout=120)
        assert np.array_equal(got[t], br.first_strict_max(np.fromfile(tmp_path / "o.f32", F32).reshape(1000, -1))), t


# ---- measure ---------------------------------------------------------------------------------------------------------
def _measure_case(gpu_ctx_factory, name, layer, P):
    ctx = _ctx(gpu_ctx_factory, name)
    X, want = tc.points(tc.forest(name)["D"], P), tc.restate(name, P, layer)
    labels = tc.labels_for(want["pred"], want["C"])
    got = ctx.forest_measure(X, labels, layer)
    conf, agree = tc.confusion_counts(labels, want["pred"], want["C"]), tc.agreement_counts(want["votes"])
    assert np.array_equal(got["pred"], want["pred"])
    assert got["confusion"].dtype == np.uint64 and np.array_equal(got["confusion"], conf)
    assert got["agree"].dtype == np.uint64 and np.array_equal(got["agree"], agree)
    assert np.array_equal(got["agree"], got["agree"].T) and (np.diag(got["agree"]) == P).all()
    return ctx, X, labels, conf, agree


@pytest.mark.parametrize("name,layer", HEADS)
@pytest.mark.parametrize("P", [1, 17, 65, 1000])
def test_measure_counts_equal_the_restatement(gpu_ctx_factory, name, layer, P):
    _measure_case(gpu_ctx_factory, name, layer, P)


def test_measure_accumulates_over_chunks(gpu_ctx_factory):
    _measure_case(gpu_ctx_factory, "tiny", 0, tc.CHUNK_TAIL)
    _measure_case(gpu_ctx_factory, "nan_tie6", 0, tc.CHUNK_TAIL)
    _measure_case(gpu_ctx_factory, "tiny", 0, 65536)


def test_measure_outputs_are_optional(gpu_ctx_factory):
    ctx = _ctx(gpu_ctx_factory, "single")
    X, want = tc.points(366, 65), tc.restate("single", 65)
    agree = np.zeros((4, 4), np.uint64)
    assert ctx.L.rvseg_forest_measure(ctx.h, X.ctypes.data, 65, 366, None, 0, None, None, agree.ctypes.data) == 0
    assert np.array_equal(agree, tc.agreement_counts(want["votes"]))
    pred = np.zeros(65, np.int32)
    assert ctx.L.rvseg_forest_measure(ctx.h, X.ctypes.data, 65, 366, None, 0, pred.ctypes.data, None, None) == 0
    assert np.array_equal(pred, want["pred"])
    assert ctx.forest_measure(X)["confusion"] is None
    only = ctx.forest_measure(X, tc.labels_for(want["pred"], 9), want=("confusion",))
    assert only["pred"] is None and only["agree"] is None
    assert np.array_equal(only["confusion"], tc.confusion_counts(tc.labels_for(want["pred"], 9), want["pred"], 9))


@pytest.mark.parametrize("name,layer", [("tiny", 0), ("multi", 1), ("ensemble64", 0)])
def test_tool_classes_return_the_restated_floats(gpu_ctx_factory, name, layer):
    import rovinasemanticsegmentation_amd as rv
    ctx, X, labels, conf, agree = _measure_case(gpu_ctx_factory, name, layer, 1000)
    forest = rv.RandomForest(ctx)
    acc = rv.AccuracyTool().measure(forest, X, labels, layer)
    assert _bits(acc) == _bits(tc.accuracy(conf)) and 0 < acc < 1
    norm = rv.ConfusionMatrixTool().measure(forest, X, labels, layer)
    assert np.array_equal(_bits(norm), _bits(tc.confusion_normalised(conf)))
    corr = rv.CorrelationTool().measure(forest, X, layer)
    assert np.array_equal(_bits(corr), _bits(tc.correlation(agree, 1000))) and (np.diag(corr) == 1).all()
    assert np.array_equal(forest.classify(X, layer), tc.restate(name, 1000, layer)["pred"])
    assert rv.AccuracyTool().format(acc) == "Accuracy: %2.2f%% (Error: %2.2f%%)\n" % (acc * 100, (1 - acc) * 100)
    assert rv.ConfusionMatrixTool().format(norm).count("\n") == 2 * len(norm) + 2
    assert rv.CorrelationTool().format(corr).splitlines()[2].startswith("       0 | 100.00% |")


# ---- boosted model -----------------------------------------------------------------------------------------------------
def test_boosted_model_votes_with_its_trees_own_labels(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    trees = br.split_trees(tc.forest("single")["blob"])
    w = np.asarray((1.5, np.inf, -0.25, -0.0), F32)
    ctx = gpu_ctx_factory(multi_layer=0)
    ctx.boosted_load(br.boosted_stream(trees, w))
    X, want = tc.points(366, 1000), tc.restate("single", 1000)
    votes = ctx.forest_classify_trees(X)
    assert np.array_equal(votes, want["votes"])            # the -0.25 and -0.0 trees still vote their labels
    assert len(np.unique(votes[2])) > 1
    pred = ctx.forest_classify(X)
    assert np.array_equal(pred, rv.BoostedRandomForest(ctx).classify(X))
    got = ctx.forest_measure(X, tc.labels_for(pred, 9))
    assert np.array_equal(got["pred"], pred) and np.array_equal(got["agree"], tc.agreement_counts(want["votes"]))
    assert np.array_equal(got["confusion"], tc.confusion_counts(tc.labels_for(pred, 9), pred, 9))
    size = C.c_size_t(77)
    y = np.zeros((1000, 1), np.int32)
    cc = (C.c_int32 * 1)(9)
    st = ctx.L.rvseg_forest_refit(ctx.h, X.ctypes.data, 1000, 366, y.ctypes.data, 1, cc, 1.0, None, 0, C.byref(size), None)
    assert st == rv.capi.ERR_NO_FOREST and size.value == 77 and b"boosted" in ctx.L.rvseg_last_error(ctx.h)


# ---- refused calls -----------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    ctx = _ctx(gpu_ctx_factory, "single")
    P = 300
    X = tc.points(366, P)
    good = tc.labels_for(tc.restate("single", 1000)["pred"][:P], 9)
    pred, votes = np.full(P, -7, np.int32), np.full((4, P), 201, np.uint8)
    conf, agree = np.full((9, 9), 99, np.uint64), np.full((4, 4), 99, np.uint64)
    L, h = ctx.L, ctx.h

    def untouched():
        return (pred == -7).all() and (votes == 201).all() and (conf == 99).all() and (agree == 99).all()
    for layer in (-1, 1, 8):
        assert L.rvseg_forest_classify(h, X.ctypes.data, P, 366, layer, pred.ctypes.data) == rv.capi.ERR_INVALID_ARG
        assert L.rvseg_forest_classify_trees(h, X.ctypes.data, P, 366, layer, votes.ctypes.data) == rv.capi.ERR_INVALID_ARG
        assert L.rvseg_forest_measure(h, X.ctypes.data, P, 366, good.ctypes.data, layer, pred.ctypes.data, conf.ctypes.data,
                                      agree.ctypes.data) == rv.capi.ERR_INVALID_ARG
    assert untouched()
    for bad_value, where in ((9, 0), (-1, P - 1), (9, 150)):
        bad = good.copy()
        bad[where] = bad_value
        assert L.rvseg_forest_measure(h, X.ctypes.data, P, 366, bad.ctypes.data, 0, pred.ctypes.data, conf.ctypes.data,
                                      agree.ctypes.data) == rv.capi.ERR_INVALID_ARG
        assert b"label" in L.rvseg_last_error(h) and untouched()
    assert L.rvseg_forest_classify(h, X.ctypes.data, 0, 366, 0, pred.ctypes.data) == rv.capi.ERR_INVALID_ARG      # P <= 0
    assert L.rvseg_forest_classify(h, X.ctypes.data, P, 365, 0, pred.ctypes.data) == rv.capi.ERR_INVALID_ARG      # D
    assert untouched()
    # refit: a label out of range, heads that do not match
    size, out, counts = C.c_size_t(77), C.create_string_buffer(b"\x55" * 64, 1 << 20), np.full((764, 9), 5, np.uint32)
    for lab, cc in ((np.full((P, 1), 9, np.int32), [9]), (np.zeros((P, 1), np.int32), [8]), (np.zeros((P, 2), np.int32), [9, 9])):
        cca = (C.c_int32 * len(cc))(*cc)
        st = L.rvseg_forest_refit(h, X.ctypes.data, P, 366, lab.ctypes.data, len(cc), cca, 1.0, out, 1 << 20, C.byref(size), counts.ctypes.data)
        assert st == rv.capi.ERR_INVALID_ARG and size.value == 77 and out.raw[:64] == b"\x55" * 64 and (counts == 5).all()
    # no model loaded
    fresh = gpu_ctx_factory(multi_layer=0)
    for st in (fresh.L.rvseg_forest_classify(fresh.h, X.ctypes.data, P, 366, 0, pred.ctypes.data),
               fresh.L.rvseg_forest_classify_trees(fresh.h, X.ctypes.data, P, 366, 0, votes.ctypes.data),
               fresh.L.rvseg_forest_measure(fresh.h, X.ctypes.data, P, 366, good.ctypes.data, 0, pred.ctypes.data, conf.ctypes.data, agree.ctypes.data),
               fresh.L.rvseg_forest_refit(fresh.h, X.ctypes.data, P, 366, good.ctypes.data, 1, (C.c_int32 * 1)(9), 1.0, out, 1 << 20,
                                          C.byref(size), counts.ctypes.data)):
        assert st == rv.capi.ERR_NO_FOREST
    assert untouched() and size.value == 77 and (counts == 5).all()
    # and the model still answers
    assert np.array_equal(ctx.forest_classify(X), tc.restate("single", 1000)["pred"][:P])


# ---- refit -------------------------------------------------------------------------------------------------------------
CTX_D12 = dict(multi_layer=1, patch_size_reduce=2, feature_depth=0, feature_height=0, feature_normal=0)   # train_cases.layout
CTX_D6 = dict(multi_layer=1, patch_size_reduce=1)                                                          # train_cases.params


def _structure(tree):
    return tree["feat"].tobytes() + tree["thr"].tobytes() + tree["left"].tobytes()


@pytest.mark.parametrize("which", ["three_layers", "one_layer"])
def test_refit_on_the_training_set_returns_the_trained_bytes(gpu_ctx_factory, which):
    c = trc.layout([2, 9, 15]) if which == "three_layers" else trc.params("num_features_D")
    kw = dict(c["kw"], use_bootstrap=1)
    ctx = gpu_ctx_factory(**(CTX_D12 if which == "three_layers" else CTX_D6))
    X = c["X"]
    trained = ctx.forest_train(X, c["labels"], c["cc"], **kw)
    ctx.forest_load(trained)
    assert sum(len(t["left"]) for t in trc.parse(trained)) > 20
    assert ctx.forest_refit(X, c["labels"], c["cc"], smoothing=kw.get("smoothing", 1.0)) == trained
    assert ctx.forest_write() == trained                     # the loaded model is not replaced


def test_refit_on_other_labels_re_estimates_the_leaves_only(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    c = trc.layout([2, 9, 15])
    ctx = gpu_ctx_factory(**CTX_D12)
    X = c["X"]
    trained = ctx.forest_train(X, c["labels"], c["cc"], **dict(c["kw"], use_bootstrap=1))
    ctx.forest_load(trained)
    rng = np.random.default_rng(3)
    X2 = rng.integers(0, 256, (777, c["X"].shape[1])).astype(F32)
    lab2 = np.stack([rng.integers(0, n, 777) for n in c["cc"]], 1).astype(np.int32)
    lab2[:, 0] = 1                                                      # a class without examples: an infinite frequency
    refit, counts = ctx.forest_refit(X2, lab2, c["cc"], smoothing=0.5, return_counts=True)
    assert np.array_equal(counts, _walk_counts(trained, X2, lab2, c["cc"])) and counts.sum() == 777 * 3 * len(trc.parse(trained))
    before, after = trc.parse(trained), trc.parse(refit)
    row = 0
    for tb, ta in zip(before, after):
        assert _structure(tb) == _structure(ta)
        for v in range(len(ta["left"])):
            if ta["left"][v] == 0:                                      # every leaf, recomputed in Python
                want = _leaves_from_counts(counts[row + v], lab2, c["cc"], 0.5)
                assert len(ta["mhist"][v]) == 3 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ta["mhist"][v], want)), (row, v)
            if ta["left"][v] != 0:
                assert len(ta["mhist"][v]) == 0 and len(ta["hist"][v]) == 0 and not counts[row + v].any()
        row += len(ta["left"])
    assert rv.RandomForest(ctx).updateHistograms(X2, lab2, c["cc"], 0.5) == refit
    old = ctx.forest_eval(X2)
    ctx.forest_load(refit)
    new = ctx.forest_eval(X2)
    assert old.shape == new.shape and not np.array_equal(old, new)


def test_refit_of_the_golden_multi_forest_covers_both_layers(gpu_ctx_factory):
    ctx = _ctx(gpu_ctx_factory, "multi")
    blob = tc.forest("multi")["blob"]
    X = tc.points(366, 1000)
    labels = np.stack([tc.labels_for(tc.restate("multi", 1000, l)["pred"], n) for l, n in enumerate((8, 9))], 1).astype(np.int32)
    refit, counts = ctx.forest_refit(X, labels, [8, 9], return_counts=True)
    assert len(refit) == len(blob) and refit != blob
    assert np.array_equal(counts, _walk_counts(blob, X, labels, [8, 9]))
    row = 0
    for tb, ta in zip(trc.parse(blob), trc.parse(refit)):
        assert _structure(tb) == _structure(ta)
        leaves = np.flatnonzero(ta["left"] == 0)
        for v in leaves:
            want = _leaves_from_counts(counts[row + v], labels, [8, 9], 1.0)
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ta["mhist"][v], want))
            assert np.array_equal(ta["hist"][v], tb["hist"][v])       # the single-label head beside two layers stays as loaded
        row += len(ta["left"])
    assert ctx.forest_write() == blob
