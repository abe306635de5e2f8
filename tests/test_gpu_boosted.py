"""The boosted forest on the GPU (rvseg_boosted_load / _write / _weights / _train): evaluation against the restatement's
vote sums (tests/boost_restate.py) and, where it is built, the reference's own compiled evaluator; training against the
restatement's bytes.  Every comparison is bit for bit.  The recipes are pinned on the CPU in tests/test_boost_cases_cpu.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

import boost_cases as bc
import boost_restate as br

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libforest_ref")
F32 = np.float32
_cache = {}


def _golden_trees(golden_dir):
    if "trees" not in _cache:
        with open(os.path.join(golden_dir, "forest_single.dat"), "rb") as fh:
            _cache["trees"] = br.split_trees(fh.read())
    return _cache["trees"]


def _points():
    from rovinasemanticsegmentation_amd import synthetic
    if "X" not in _cache:
        _cache["X"] = synthetic.random_points(5, 1000)
    return _cache["X"]


def _tree_labels(trees, X, tmp_path):
    """Per tree its vote for every row of X: from the reference's compiled evaluator on one-tree files where it is built,
    else from the restatement."""
    if "labels" in _cache:
        return _cache["labels"]
    if os.path.exists(REF):
        (tmp_path / "x.f32").write_bytes(np.ascontiguousarray(X, F32).tobytes())
        labels = []
        for t, tree in enumerate(trees):
            (tmp_path / ("t%d.dat" % t)).write_bytes(br.one_tree_forest(tree))
            out = tmp_path / ("t%d.f32" % t)
            subprocess.check_call([REF, "eval", str(tmp_path / ("t%d.dat" % t)), str(tmp_path / "x.f32"), str(X.shape[1]), "single", str(out)],
                                  timeout=120)
            labels.append(br.first_strict_max(np.fromfile(out, F32).reshape(X.shape[0], -1)))
    else:
        labels = [br.tree_votes(tree, X) for tree in trees]
    _cache["labels"] = labels
    return labels


@pytest.mark.parametrize("order", [br.WEIGHT_FIRST, br.TREE_FIRST])
@pytest.mark.parametrize("weights", [(0.5, 1.25, 0.75, 2.0), (1.5, np.inf, -0.25, -0.0)])
def test_loaded_model_returns_the_reference_vote_sums(gpu_ctx_factory, golden_dir, tmp_path, order, weights):
    trees, X = _golden_trees(golden_dir), _points()
    w = np.asarray(weights, F32)
    blob = br.boosted_stream(trees, w, order)
    ctx = gpu_ctx_factory(multi_layer=0)
    ctx.boosted_load(blob, order)
    info = ctx.forest_info()
    C = info["class_counts"][0]
    assert info["n_trees"] == len(trees) and len(info["class_counts"]) == 1
    got = ctx.forest_eval(X)
    labels = _tree_labels(trees, X, tmp_path)
    want = br.vote_sums(trees, w, X, C, labels=labels)
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(np.signbit(got), np.signbit(want))                     # a -0.0 weight votes +0.0, like 0 + (-0.0)
    assert len({tuple(l) for l in map(tuple, labels)}) > 1                       # the trees do not all vote alike
    assert np.array_equal(br.vote_sums(trees, w, X, C), want, equal_nan=True)    # (restatement == compiled evaluator)
    assert np.array_equal(ctx.boosted_weights().view(np.uint32), w.view(np.uint32))
    # the writers: RandomForest::write is refused, the boosted one returns the bytes it read, or the other order
    import rovinasemanticsegmentation_amd as rv
    with pytest.raises(rv.capi.RvsegError) as e:
        ctx.forest_write()
    assert e.value.status == rv.capi.ERR_INVALID_ARG and "rvseg_boosted_write" in str(e.value)
    with pytest.raises(rv.capi.RvsegError):
        ctx.forest_write(str(tmp_path / "no.dat"))
    assert ctx.boosted_write() == blob
    assert ctx.boosted_write(order=1 - order) == br.boosted_stream(trees, w, 1 - order)
    ctx.boosted_write(str(tmp_path / "b.dat"))
    assert (tmp_path / "b.dat").read_bytes() == blob
    f = rv.BoostedRandomForest(ctx)
    assert f.getSize() == len(trees) and np.array_equal(f.classify(X[:50]), br.first_strict_max(want[:50]))
    # a stream named in the wrong order is refused and the model stays
    with pytest.raises(rv.capi.RvsegError):
        ctx.boosted_load(blob, 1 - order)
    assert np.array_equal(ctx.forest_eval(X[:10]), want[:10], equal_nan=True)


def test_multi_layer_context_refuses_a_boosted_model_and_keeps_its_own(gpu_ctx_factory, golden_dir):
    import rovinasemanticsegmentation_amd as rv
    with open(os.path.join(golden_dir, "forest_multi.dat"), "rb") as fh:
        multi = fh.read()
    ctx = gpu_ctx_factory(multi_layer=1)
    ctx.forest_load(multi)
    before = ctx.forest_eval(_points()[:64])
    blob = br.boosted_stream(_golden_trees(golden_dir), np.ones(4, F32))
    with pytest.raises(rv.capi.RvsegError) as e:
        ctx.boosted_load(blob)
    assert e.value.status == rv.capi.ERR_INVALID_ARG
    assert ctx.forest_write() == multi and np.array_equal(ctx.forest_eval(_points()[:64]), before)
    with pytest.raises(rv.capi.RvsegError) as e:
        ctx.boosted_write()
    assert e.value.status == rv.capi.ERR_NO_FOREST
    # and an ordinary forest replaces a boosted one on a single-layer context
    single = gpu_ctx_factory(multi_layer=0)
    single.boosted_load(blob)
    with open(os.path.join(golden_dir, "forest_single.dat"), "rb") as fh:
        plain = fh.read()
    single.forest_load(plain)
    assert single.forest_write() == plain


def test_boosted_model_runs_through_the_single_layer_frame_path(gpu_ctx_factory, oracle):
    """One 32 x 24 frame, single layer, no CRF: the frame path on the boosted model equals the oracle's frame path on the
    same model written as an ordinary forest.dat with one-hot leaves."""
    from rovinasemanticsegmentation_amd import synthetic
    W, H = 32, 24
    kw = dict(width=W, height=H, patch_size=9, patch_size_reduce=3)
    rgb, depth = synthetic.make_batch(1, W, H, holes=True)
    calib = synthetic.make_calib(W, H)
    trees = br.split_trees(synthetic.make_forest_bytes(seed=12, n_trees=5, leaves_per_tree=24, max_depth=6, D=30, single_classes=4,
                                                       layer_classes=(2, 3)))
    w = np.array([0.5, 1.75, -0.5, 0.25, 1.0], F32)
    ctx = gpu_ctx_factory(multi_layer=0, use_dense_crf=0, **kw)
    ctx.boosted_load(br.boosted_stream(trees, w, br.TREE_FIRST), br.TREE_FIRST)
    out = ctx.segment_frames(rgb, depth, calib)
    forest = oracle.Forest(br.one_hot_forest(trees, w, 4))
    want, n_points = oracle.rf_frame(oracle.default_params(**kw), forest, 0, rgb[0], depth[0], calib)
    assert n_points > 50
    assert np.array_equal(out["posteriors"][0], want)
    assert len(np.unique(want)) > 3


# ---- training --------------------------------------------------------------------------------------------------------
def _restated(name, *args):
    key = (name,) + args
    if key not in _cache:
        c = getattr(bc, name)(*args)
        _cache[key] = (c, br.boosted_train(c["X"], c["y"], c["n_classes"], c["rounds"], c["seed"], **c["params"]))
    return _cache[key]


def _train(ctx, c, **over):
    kw = dict(c["params"], num_trees=c["rounds"], seed=c["seed"])
    kw.update(over)
    return ctx.boosted_train(c["X"], c["y"], c["n_classes"], **kw)


def _same(got, want):
    assert got["rounds"] == want["rounds"]
    assert np.array_equal(got["errors"].view(np.uint32), want["errors"].view(np.uint32)), (got["errors"], want["errors"])
    assert np.array_equal(got["alphas"].view(np.uint32), want["alphas"].view(np.uint32)), (got["alphas"], want["alphas"])
    if got["model"] != want["model"] and got["rounds"]:   # say which tree parts
        (T,) = struct.unpack_from("<i", got["model"], 0)
        assert T == want["rounds"]
        pos = 4
        for t, tree in enumerate(want["trees"]):
            assert got["model"][pos:pos + 4] == want["weights"][t:t + 1].tobytes(), ("weight of tree %d" % t)
            assert got["model"][pos + 4:pos + 4 + len(tree)] == tree, ("tree %d" % t)
            pos += 4 + len(tree)
    assert got["model"] == want["model"]


@pytest.mark.parametrize("kind,use_bootstrap", [("byte", 0), ("byte", 1), ("float", 0), ("float", 1)])
def test_boosted_training_equals_the_restatement_byte_for_byte(gpu_ctx_factory, kind, use_bootstrap):
    c, want = _restated("main_case", kind, use_bootstrap)
    ctx = gpu_ctx_factory(width=160, height=120, multi_layer=0)
    got = _train(ctx, c)
    _same(got, want)
    assert got["rounds"] == 4
    import rovinasemanticsegmentation_amd as rv
    with pytest.raises(rv.capi.RvsegError) as e:   # a trained model is not a loaded one
        ctx.boosted_write()
    assert e.value.status == rv.capi.ERR_NO_FOREST
    if kind == "byte" and use_bootstrap:   # equal seeds give equal bytes, different seeds do not
        assert _train(ctx, c)["model"] == got["model"]
        assert _train(ctx, c, seed=c["seed"] + 1)["model"] != got["model"]


def test_training_on_a_context_that_holds_a_loaded_boosted_model_returns_the_trained_one(gpu_ctx_factory, golden_dir):
    """The loaded model and the trained one are kept apart: training hands out what it trained, the loaded model stays the
    context's forest, and a buffer that is too small is answered by rvseg_boosted_train_result, in either order."""
    import ctypes as C
    import rovinasemanticsegmentation_amd as rv
    c, want = _restated("main_case", "byte", 0)
    ctx = gpu_ctx_factory(multi_layer=0)
    loaded = br.boosted_stream(_golden_trees(golden_dir), np.array([0.5, 1.5, 2.5, 3.5], F32), br.TREE_FIRST)
    ctx.boosted_load(loaded, br.TREE_FIRST)
    votes = ctx.forest_eval(_points()[:32])
    got = _train(ctx, c)
    _same(got, want)
    assert got["model"] != loaded
    assert ctx.boosted_write() == loaded and np.array_equal(ctx.forest_eval(_points()[:32]), votes)
    assert rv.BoostedRandomForest(ctx).getSize() == 4 and np.array_equal(ctx.boosted_weights(), [0.5, 1.5, 2.5, 3.5])
    # the C path with a buffer that is too small: the size comes back, the model is fetched without training again
    X = np.ascontiguousarray(c["X"], F32)
    y = np.ascontiguousarray(c["y"], np.int32)
    tp = ctx._train_params(dict(c["params"], num_trees=c["rounds"], seed=c["seed"]))
    small, size = C.create_string_buffer(16), C.c_size_t()
    st = ctx.L.rvseg_boosted_train(ctx.h, X.ctypes.data, X.shape[0], X.shape[1], y.ctypes.data, c["n_classes"], C.byref(tp), small, 16,
                                   C.byref(size), None, None, None)
    assert st == rv.capi.ERR_INVALID_ARG and size.value == len(want["model"])
    assert b"rvseg_boosted_train_result" in ctx.L.rvseg_last_error(ctx.h)
    for order in (br.WEIGHT_FIRST, br.TREE_FIRST):
        buf = C.create_string_buffer(size.value)
        assert ctx.L.rvseg_boosted_train_result(ctx.h, order, buf, size.value, C.byref(size)) == rv.capi.OK
        assert buf.raw[:size.value] == br.boosted_stream(want["trees"], want["weights"], order)
    fresh = gpu_ctx_factory(multi_layer=0)
    assert fresh.L.rvseg_boosted_train_result(fresh.h, 0, None, 0, C.byref(size)) == rv.capi.ERR_NO_FOREST


def test_negative_alpha_is_followed(gpu_ctx_factory):
    c, want = _restated("negative_alpha_case")
    got = _train(gpu_ctx_factory(width=160, height=120, multi_layer=0), c)
    _same(got, want)
    assert (got["alphas"] < 0).any()


@pytest.mark.parametrize("name,rounds", [("separable_case", 1), ("all_wrong_case", 0), ("single_example_case", 1)])
def test_stop_rules_and_a_single_example(gpu_ctx_factory, name, rounds):
    c, want = _restated(name)
    got = _train(gpu_ctx_factory(width=160, height=120, multi_layer=0), c)
    _same(got, want)
    assert got["rounds"] == rounds
    if name == "separable_case":
        assert np.isposinf(got["alphas"][0])
    if name == "all_wrong_case":
        assert got["errors"][0] == 1 and got["model"] == b"\0\0\0\0"


def test_trained_model_loads_and_votes_like_the_restatement(gpu_ctx_factory):
    """The trained stream on a context of the default feature length: its 8 features are the first of 366."""
    c, want = _restated("main_case", "float", 1)
    ctx = gpu_ctx_factory(multi_layer=0)
    X = np.zeros((len(c["y"]), ctx.feature_length), F32)
    X[:, :c["X"].shape[1]] = c["X"]
    ctx.boosted_load(want["model"])
    votes = ctx.forest_eval(X)
    assert np.array_equal(votes, br.vote_sums(want["trees"], want["weights"], c["X"], c["n_classes"]))
    assert (br.first_strict_max(votes) == c["y"]).mean() > 0.6      # and the ensemble has learnt the rule


def test_plain_forest_training_is_untouched_by_a_boosted_run(gpu_ctx_factory, oracle):
    c, _ = _restated("main_case", "float", 1)
    ctx = gpu_ctx_factory(width=160, height=120, multi_layer=0)
    kw = dict(num_trees=2, max_depth=6, min_split_examples=10, seed=3)
    labels = np.stack([c["y"], (c["X"][:, 1] > 99).astype(np.int32)], 1)
    before = ctx.forest_train(c["X"], labels, [3, 2], **kw)
    assert before == oracle.forest_train(c["X"], labels, [3, 2], **kw)
    _train(ctx, c)
    assert ctx.forest_train(c["X"], labels, [3, 2], **kw) == before
