"""Scoring on the GPU (kernels_eval.hip): colour-coded labels (RgbLabelConversion, include/rgb_label_conversion.h), the
confusion matrix of src/test.cpp:186-195 / test_multi.cpp:222-233 and the scores of test.cpp:203-228, against numpy
restatements of the reference: a dict lookup with its std::map defaults, np.bincount, and the score transcription of
tests/test_eval_cpu.py.  Also the device chain segment_frames_device -> eval_accumulate_device against the oracle, a
train -> score round trip, and the C++ facade."""
import json
import os
import subprocess

import numpy as np
import pytest

from rovinasemanticsegmentation_amd import synthetic
from test_eval_cpu import reference_scores

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def codings(golden_dir):
    with open(os.path.join(golden_dir, "color_codings.json")) as f:
        return [c["coding"] for c in json.load(f)["color_codings"]]


def np_decode(rgb, coding, missing=0):
    """rgbToLabel (:86-88): std::map keyed by colour, later entries overwrite, operator[] of a missing colour -> 0."""
    table = {}
    for e in coding:
        table[tuple(int(v) for v in e["color"])] = int(np.int64(e["label"]).astype(np.int8))
    keys = rgb[..., 0].astype(np.int64) << 16 | rgb[..., 1].astype(np.int64) << 8 | rgb[..., 2]
    lut_k = np.array([r << 16 | g << 8 | b for (r, g, b) in table], np.int64)
    lut_v = np.array(list(table.values()), np.int8)
    out = np.full(keys.shape, missing, np.int8)
    if len(lut_k):
        order = np.argsort(lut_k)
        pos = np.clip(np.searchsorted(lut_k[order], keys), 0, len(lut_k) - 1)
        hit = lut_k[order][pos] == keys
        out[hit] = lut_v[order][pos][hit]
    return out


def np_encode(labels, coding):
    """labelToRgb (:80-84): later entries overwrite, a label not in the table -> (0, 0, 0)."""
    lut = np.zeros((256, 3), np.uint8)
    for e in coding:
        lut[int(np.int64(e["label"]).astype(np.int8)) & 255] = [int(v) for v in e["color"]]
    return lut[labels.astype(np.int8).view(np.uint8)]


def np_confusion(pred, gt, C):
    p = pred.astype(np.int64).ravel()
    g = gt.astype(np.int64).ravel()
    both = (p >= 0) & (g >= 0)
    oor = both & ((p >= C) | (g >= C))
    ok = both & ~oor
    return np.bincount(g[ok] * C + p[ok], minlength=C * C).reshape(C, C).astype(np.uint64), int(oor.sum())


def _ctx(factory, layer_classes, W, H, **kw):
    ctx = factory(width=W, height=H, patch_size=9, patch_size_reduce=3, **kw)
    ctx.forest_load(synthetic.make_forest_bytes(seed=3, n_trees=1, leaves_per_tree=4, max_depth=3, D=30,
                                                layer_classes=tuple(layer_classes)))
    return ctx


def _adversarial_coding(rng):
    """256 entries: duplicate colours (the later one wins), colours one channel step apart, duplicate labels."""
    base = rng.integers(0, 256, size=(200, 3))
    near = base[:28] + np.array([0, 0, 1])
    near[:, 2] %= 256
    dup = base[100:128]                                  # repeated colours with other labels
    cols = np.concatenate([base, near, dup])
    labs = rng.integers(-128, 128, size=len(cols))
    return [{"name": "c%d" % i, "color": [int(v) for v in c], "label": int(l)} for i, (c, l) in enumerate(zip(cols, labs))]


def _rgb_images(rng, coding, shape, p_unknown=0.2):
    """Blocky images of the coding's colours plus unknown colours (and colours one step off a known one)."""
    cols = np.array([e["color"] for e in coding], np.uint8)
    idx = rng.integers(0, len(cols), size=shape)
    img = cols[idx]
    unk = rng.random(shape) < p_unknown
    img[unk] = rng.integers(0, 256, size=(int(unk.sum()), 3))
    off = rng.random(shape) < 0.05
    img[off, 1] ^= 1
    return img


# ---- decode / encode --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(640, 480), (161, 97)])
@pytest.mark.parametrize("n", [1, 3, 64])
def test_decode_reference_codings(gpu_ctx_factory, codings, W, H, n):
    ctx = _ctx(gpu_ctx_factory, (8, 9), W, H, max_batch=8)
    rng = np.random.default_rng(n * 7 + W)
    for l in range(2):
        ctx.color_coding_set(l, codings[l])
    rgb = np.empty((n, 2, H, W, 3), np.uint8)
    for l in range(2):
        rgb[:, l] = _rgb_images(rng, codings[l], (n, H, W))
    got = ctx.labels_from_rgb(rgb)                       # every layer, n x L planes
    for l in range(2):
        assert np.array_equal(got[:, l], np_decode(rgb[:, l], codings[l])), l
    # one layer's images only
    got1 = ctx.labels_from_rgb(rgb[:, 1].copy(), layer=1)
    assert np.array_equal(got1, np_decode(rgb[:, 1], codings[1]))
    # missing_label = -1: unknown colours are left unscored instead of becoming class 0
    ctx.color_coding_set(0, codings[0], missing_label=-1)
    got0 = ctx.labels_from_rgb(rgb[:, 0].copy(), layer=0)
    assert np.array_equal(got0, np_decode(rgb[:, 0], codings[0], missing=-1))
    assert (got0 == -1).sum() > (np_decode(rgb[:, 0], codings[0]) == -1).sum()


@pytest.mark.parametrize("W,H,n", [(640, 480, 3), (161, 97, 64), (161, 97, 1)])
def test_decode_adversarial_table(gpu_ctx_factory, W, H, n):
    rng = np.random.default_rng(W + n)
    coding = _adversarial_coding(rng)
    assert len(coding) == 256
    ctx = _ctx(gpu_ctx_factory, (8,), W, H)
    ctx.color_coding_set(0, coding)
    rgb = _rgb_images(rng, coding, (n, H, W))
    assert np.array_equal(ctx.labels_from_rgb(rgb, layer=0), np_decode(rgb, coding))
    ctx.color_coding_set(0, coding, missing_label=-1)
    assert np.array_equal(ctx.labels_from_rgb(rgb, layer=0), np_decode(rgb, coding, missing=-1))


def test_capacity_and_argument_errors(gpu_ctx_factory, codings):
    import rovinasemanticsegmentation_amd as rv
    rng = np.random.default_rng(5)
    ctx = gpu_ctx_factory(width=64, height=48, patch_size=9, patch_size_reduce=3)
    with pytest.raises(rv.capi.RvsegError) as e:           # no model yet: layers and classes are unknown
        ctx.color_coding_set(0, codings[0])
    assert e.value.status == rv.capi.ERR_INVALID_ARG and "forest" in str(e.value)
    ctx = _ctx(gpu_ctx_factory, (8, 9), 64, 48)
    coding = _adversarial_coding(rng) + [{"name": "x", "color": [1, 2, 3], "label": 1}]
    with pytest.raises(rv.capi.RvsegError) as e:
        ctx.color_coding_set(0, coding)
    assert e.value.status == rv.capi.ERR_CAPACITY
    with pytest.raises(rv.capi.RvsegError) as e:           # layer without a coding
        ctx.labels_from_rgb(np.zeros((1, 48, 64, 3), np.uint8), layer=1)
    assert e.value.status == rv.capi.ERR_INVALID_ARG
    with pytest.raises(rv.capi.RvsegError) as e:
        ctx.color_coding_set(2, codings[0])
    assert e.value.status == rv.capi.ERR_INVALID_ARG
    # a forest load discards codings
    ctx.color_coding_set(0, codings[0])
    ctx.labels_to_rgb(np.zeros((1, 48, 64), np.int8), layer=0)
    ctx.forest_load(synthetic.make_forest_bytes(seed=4, n_trees=1, leaves_per_tree=4, max_depth=3, D=30, layer_classes=(8, 9)))
    with pytest.raises(rv.capi.RvsegError):
        ctx.labels_to_rgb(np.zeros((1, 48, 64), np.int8), layer=0)


@pytest.mark.parametrize("W,H,n", [(640, 480, 3), (161, 97, 5)])
def test_encode_round_trip_and_defaults(gpu_ctx_factory, codings, W, H, n):
    rng = np.random.default_rng(n)
    ctx = _ctx(gpu_ctx_factory, (8, 9), W, H)
    for l in range(2):
        ctx.color_coding_set(l, codings[l])
    # labels that are in the tables: decode(encode(x)) == x, and the bytes are the coding's colours
    lab = np.empty((n, 2, H, W), np.int8)
    for l in range(2):
        vals = np.array([e["label"] for e in codings[l]], np.int8)
        lab[:, l] = vals[rng.integers(0, len(vals), size=(n, H, W))]
    rgb = ctx.labels_to_rgb(lab)
    for l in range(2):
        assert np.array_equal(rgb[:, l], np_encode(lab[:, l], codings[l]))
    assert np.array_equal(ctx.labels_from_rgb(rgb), lab)
    # labels not in the table -> black
    odd = rng.integers(9, 128, size=(n, H, W)).astype(np.int8)
    assert not ctx.labels_to_rgb(odd, layer=0).any()
    # duplicate labels: the later colour
    coding = [{"name": "a", "color": [1, 2, 3], "label": 4}, {"name": "b", "color": [9, 8, 7], "label": 4},
              {"name": "c", "color": [5, 5, 5], "label": -1}]
    ctx.color_coding_set(0, coding)
    out = ctx.labels_to_rgb(np.full((1, H, W), 4, np.int8), layer=0)
    assert (out.reshape(-1, 3) == [9, 8, 7]).all()
    out = ctx.labels_to_rgb(np.full((1, H, W), -1, np.int8), layer=0)
    assert (out.reshape(-1, 3) == [5, 5, 5]).all()


def test_rgb_label_conversion_facade(gpu_ctx_factory, codings):
    import rovinasemanticsegmentation_amd as rv
    ctx = _ctx(gpu_ctx_factory, (8, 9), 161, 97)
    conv = rv.RgbLabelConversion(ctx, codings[1], layer=1)
    assert conv.getValidLabelCount() == 9
    assert conv.getLabelNumber("Void") == -1 and conv.getLabelNumber("Floor") == 3 and conv.getLabelNumber("nope") == 0
    assert conv.getLabelName(7) == "Wall" and conv.getLabelName(-2) == "Other" and conv.getLabelName(40) == ""
    img = _rgb_images(np.random.default_rng(1), codings[1], (97, 161))
    lab = conv.rgbToLabel(img)
    assert lab.shape == (97, 161) and np.array_equal(lab, np_decode(img, codings[1]))
    assert np.array_equal(conv.labelToRgb(lab), np_encode(lab, codings[1]))


# ---- confusion ----------------------------------------------------------------------------------------------------
def _random_pairs(rng, n, L, H, W, C):
    """Predictions and ground truth with negative values and values >= C, spatially blocky like real label images."""
    def field():
        coarse = rng.integers(-3, C + 3, size=(n, L, H // 4 + 1, W // 4 + 1)).astype(np.int8)
        f = np.repeat(np.repeat(coarse, 4, axis=2), 4, axis=3)[:, :, :H, :W]
        noise = rng.random(f.shape) < 0.1
        f[noise] = rng.integers(-3, C + 3, size=int(noise.sum()))
        return np.ascontiguousarray(f)
    return field(), field()


@pytest.mark.parametrize("classes", [(2,), (8, 9), (9,), (21, 21), (64,), (2, 2)])
def test_confusion_against_bincount(gpu_ctx_factory, classes):
    import rovinasemanticsegmentation_amd as rv
    L = len(classes)
    W, H, n = 161, 97, 5
    rng = np.random.default_rng(sum(classes))
    ctx = _ctx(gpu_ctx_factory, classes, W, H, max_batch=2)
    pred, gt = _random_pairs(rng, n, L, H, W, max(classes))
    ctx.eval_reset()
    ctx.eval_accumulate(pred, gt, rv.capi.GT_LABELS)
    for l, C in enumerate(classes):
        want, woor = np_confusion(pred[:, l], gt[:, l], C)
        got, oor = ctx.eval_confusion(l)
        assert np.array_equal(got, want), l
        assert oor == woor
    # RGB ground truth through a coding that covers every label value used: identical counts
    coding = [{"name": "v%d" % v, "color": [(v * 37) & 255, (v * 11 + 3) & 255, 200], "label": v} for v in range(-3, max(classes) + 3)]
    for l in range(L):
        ctx.color_coding_set(l, coding)
    gt_rgb = ctx.labels_to_rgb(gt)
    ctx.eval_reset()
    ctx.eval_accumulate(pred, gt_rgb, rv.capi.GT_RGB)
    for l, C in enumerate(classes):
        got, oor = ctx.eval_confusion(l)
        assert np.array_equal(got, np_confusion(pred[:, l], gt[:, l], C)[0]), l
    # k calls add up to one call over the concatenation; reset clears
    ctx.eval_reset()
    for i0 in (0, 1, 3):
        i1 = {0: 1, 1: 3, 3: 5}[i0]
        ctx.eval_accumulate(pred[i0:i1], gt[i0:i1])
    for l, C in enumerate(classes):
        assert np.array_equal(ctx.eval_confusion(l)[0], np_confusion(pred[:, l], gt[:, l], C)[0])
    ctx.eval_reset()
    for l in range(L):
        got, oor = ctx.eval_confusion(l)
        assert not got.any() and oor == 0


@pytest.mark.parametrize("rgb_gt", [False, True])
def test_single_bin_frames_count_exactly(gpu_ctx_factory, rgb_gt):
    import rovinasemanticsegmentation_amd as rv
    W, H, n = 640, 480, 8
    ctx = _ctx(gpu_ctx_factory, (8, 9), W, H, max_batch=8)
    pred = np.full((n, 2, H, W), 3, np.int8)
    gt = np.full((n, 2, H, W), 5, np.int8)
    if rgb_gt:
        coding = [{"name": "five", "color": [10, 20, 30], "label": 5}]
        ctx.color_coding_set(0, coding)
        ctx.color_coding_set(1, coding)
        gt = ctx.labels_to_rgb(gt)
    ctx.eval_reset()
    ctx.eval_accumulate(pred, gt, rv.capi.GT_RGB if rgb_gt else rv.capi.GT_LABELS)
    for l, C in enumerate((8, 9)):
        got, oor = ctx.eval_confusion(l)
        want = np.zeros((C, C), np.uint64)
        want[5, 3] = n * H * W
        assert np.array_equal(got, want) and oor == 0


def test_counts_pass_2_pow_32(gpu_ctx_factory):
    """64 VGA frames of one (gt, pred) pair per call, repeated until one bin passes 2^32: exact uint64 counts."""
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    W, H, n = 640, 480, 64
    dev = torch.device("cuda", 0)
    ctx = _ctx(gpu_ctx_factory, (2,), W, H)
    d_pred = torch.full((n, 1, H, W), 1, dtype=torch.int8, device=dev)
    d_gt = torch.zeros((n, 1, H, W), dtype=torch.int8, device=dev)
    d_gt[:, :, :, :8] = 1                                 # a few pixels on the diagonal as well
    s = torch.cuda.current_stream(dev).cuda_stream
    ctx.eval_reset()
    calls = (1 << 32) // (n * H * (W - 8)) + 1
    for _ in range(calls):
        ctx.eval_accumulate_device(n, d_pred.data_ptr(), d_gt.data_ptr(), rv.capi.GT_LABELS, s)
    got, oor = ctx.eval_confusion(0)
    assert int(got[0, 1]) == calls * n * H * (W - 8) and int(got[0, 1]) > (1 << 32)
    assert int(got[1, 1]) == calls * n * H * 8
    assert got[0, 0] == 0 and got[1, 0] == 0 and oor == 0
    s_ = reference_scores(got)
    sc = rv.capi.eval_scores_from_counts(got)
    assert sc["global_acc"] == s_[0] and np.float32(sc["iou"]) == s_[2]


# ---- end to end: segment -> accumulate on one stream, against the oracle -------------------------------------------
def _oracle_labels(oracle, forest, blob_multi, p_kw, rgb, depth, calib, crf, multi, classes):
    p = oracle.default_params(**p_kw)
    N = p.width * p.height
    out = []
    for i in range(rgb.shape[0]):
        if crf:
            _, _, lab = oracle.segment_frame(p, forest, multi, rgb[i], depth[i], calib, label_mode=1, unknown=[c - 1 for c in classes])
            out.append(lab.reshape(len(classes), N))
        else:
            post, _ = oracle.rf_frame(p, forest, multi, rgb[i], depth[i], calib)
            off, ls = 0, []
            for C in classes:
                ls.append(oracle.labels(post[off:off + N * C], C, 0))
                off += N * C
            out.append(np.stack(ls))
    return np.stack(out)


@pytest.mark.parametrize("crf", [False, True])
@pytest.mark.parametrize("n", [1, 4])
def test_device_chain_against_oracle(gpu_ctx_factory, oracle, codings, golden_dir, crf, n):
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    W, H = 160, 120
    dev = torch.device("cuda", 0)
    blob = open(os.path.join(golden_dir, "forest_multi.dat"), "rb").read()
    classes = (8, 9)
    # the per-frame CRF recipe is the node's (zero-filled low-res image, segmenter.cpp:358-362); the eval rule is test_multi's
    fill = 0.0 if crf else -1000.0
    kw = dict(width=W, height=H, fill_value=fill, use_dense_crf=1 if crf else 0, dcrf_iterations=3,
              label_mode=rv.capi.LABEL_CRF if crf else rv.capi.LABEL_EVAL, unknown_label=[7, 8], max_batch=4)
    ctx = gpu_ctx_factory(**kw)
    ctx.forest_load(blob)
    ev = rv.Evaluator(ctx, codings)
    rgb, depth = synthetic.make_batch(n, W, H, holes=True, start=2)
    calib = synthetic.make_calib(W, H)
    rng = np.random.default_rng(n + 10 * crf)
    gt = np.empty((n, 2, H, W), np.int8)
    for l in range(2):
        vals = np.array([e["label"] for e in codings[l]], np.int8)
        coarse = vals[rng.integers(0, len(vals), size=(n, H // 8, W // 8))]
        gt[:, l] = np.repeat(np.repeat(coarse, 8, 1), 8, 2)
    gt_rgb = np.stack([np_encode(gt[:, l], codings[l]) for l in range(2)], 1)
    d_rgb = torch.from_numpy(rgb).to(dev)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(dev)
    d_gt = torch.from_numpy(gt_rgb).to(dev)
    d_lab = torch.empty((n, 2, H, W), dtype=torch.int8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    ctx.segment_frames_device(n, d_rgb.data_ptr(), d_depth.data_ptr(), calib, 0, 0, d_lab.data_ptr(), s)
    ev.add_device(n, d_lab.data_ptr(), d_gt.data_ptr(), rv.capi.GT_RGB, s)   # no synchronisation in between
    got = [ev.confusion(l) for l in range(2)]                               # waits for the accumulate
    want_lab = _oracle_labels(oracle, oracle.Forest(blob), blob, dict(width=W, height=H, fill_value=fill, dcrf_iterations=3),
                              rgb, depth, calib, crf, 1, classes)
    for l, C in enumerate(classes):
        want, _ = np_confusion(want_lab[:, l], gt[:, l], C)
        assert np.array_equal(got[l], want), l
        assert want.sum() > 0
    # the host entry point on the same predictions gives the same counts
    ev.reset()
    ev.add(want_lab.reshape(n, 2, H, W), gt_rgb)
    for l in range(2):
        assert np.array_equal(ev.confusion(l), got[l])


def test_test_cpp_recipe_single_layer(gpu_ctx_factory, oracle, codings, golden_dir):
    """src/test.cpp: classLogPosterior (multi_layer = 0), fill -1000, the eval rule, stride 2, int8 ground truth."""
    import rovinasemanticsegmentation_amd as rv
    W, H, n = 160, 120, 3
    blob = open(os.path.join(golden_dir, "forest_multi.dat"), "rb").read()
    forest = oracle.Forest(blob)
    C = forest.classes(0)[0]
    ctx = gpu_ctx_factory(width=W, height=H, multi_layer=0, fill_value=-1000.0, label_mode=rv.capi.LABEL_EVAL, stride=2)
    ctx.forest_load(blob)
    rgb, depth = synthetic.make_batch(n, W, H, holes=True)
    calib = synthetic.make_calib(W, H)
    out = ctx.segment_frames(rgb, depth, calib, want_posteriors=False)
    gt = np.random.default_rng(3).integers(-2, C, size=(n, 1, H, W)).astype(np.int8)
    ev = rv.Evaluator(ctx, [None])
    ev.add(out["labels"], gt)
    want_lab = _oracle_labels(oracle, forest, blob, dict(width=W, height=H, fill_value=-1000.0), rgb, depth, calib, False, 0, (C,))
    want, _ = np_confusion(want_lab, gt, C)
    assert np.array_equal(ev.confusion(0), want)
    g, a, u, row = reference_scores(want)
    sc = ev.scores(0)
    assert sc["global_acc"] == g and np.float32(sc["class_avg_acc"]) == a and np.float32(sc["iou"]) == u


# ---- train -> score -----------------------------------------------------------------------------------------------
def test_train_then_score(gpu_ctx_factory, codings):
    """Colour-coded ground truth for a learnable rule (material: depth bands, object: image rows; Void over missing
    depth), decoded on the GPU, 8 frames trained with rvseg_forest_train_frames, 8 held-out frames scored."""
    import rovinasemanticsegmentation_amd as rv
    W, H = 160, 120
    rgb, depth = synthetic.make_batch(16, W, H, holes=True, start=1)
    calib = synthetic.make_calib(W, H)
    yy = np.mgrid[0:H, 0:W][0]
    lab = np.empty((16, 2, H, W), np.int8)
    lab[:, 0] = np.clip((depth.astype(np.int32) - 1500) // 400, 0, 7)
    lab[:, 1] = np.broadcast_to((yy * 9) // H, (16, H, W))
    lab[:, 0][depth == 0] = -1
    lab[:, 1][depth == 0] = -1
    gt_rgb = np.stack([np_encode(lab[:, l], codings[l]) for l in range(2)], 1)
    kw = dict(width=W, height=H, patch_size=9, patch_size_reduce=3, fill_value=-1000.0, label_mode=rv.capi.LABEL_EVAL)
    ctx = gpu_ctx_factory(**kw)
    ctx.forest_load(synthetic.make_forest_bytes(seed=3, n_trees=1, leaves_per_tree=4, max_depth=3, D=30, layer_classes=(8, 9)))
    for l in range(2):
        ctx.color_coding_set(l, codings[l])
    decoded = ctx.labels_from_rgb(gt_rgb)
    assert np.array_equal(decoded, lab)
    model, n_ex = ctx.forest_train_frames(rgb[:8], depth[:8], calib, decoded[:8], [8, 9], num_trees=4, max_depth=14,
                                          min_split_examples=10, seed=5)
    assert n_ex > 0
    ctx.forest_load(model)
    ev = rv.Evaluator(ctx, codings)
    out = ctx.segment_frames(rgb[8:], depth[8:], calib, want_posteriors=False)
    ev.add(out["labels"], gt_rgb[8:])
    accs = []
    for l, C in enumerate((8, 9)):
        want, _ = np_confusion(out["labels"][:, l], lab[8:, l], C)
        assert np.array_equal(ev.confusion(l), want)
        g, a, u, row = reference_scores(want)
        sc = ev.scores(l)
        assert sc["global_acc"] == g and np.float32(sc["class_avg_acc"]) == a and np.float32(sc["iou"]) == u
        assert sc["row_pct"].tobytes() == row.tobytes()
        accs.append(sc["global_acc"])
    print("train -> score global accuracy per layer:", accs)
    rep = ev.report(1)
    lines = rep.splitlines()
    assert lines[0] == "confusion:" and lines[1].startswith("Arch           ") and "out of" in lines[1]
    assert lines[-3].startswith("Global accuracy:         ") and lines[-1].startswith("Intersection over union: ")
    assert len(lines) == 1 + 9 + 3
    # bound picked from one MI355X run, with a margin: that run gave 97.85 (material) and 83.24 (object)
    assert min(accs) > 70.0


# ---- C++ facade ---------------------------------------------------------------------------------------------------
def test_cpp_evaluator_facade(tmp_path, codings, golden_dir):
    exe = str(tmp_path / "evaluator")
    lib_dir = os.path.join(ROOT, "rovinasemanticsegmentation_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "evaluator_test.cpp"), "-o", exe,
                           "-L", lib_dir, "-lrvseg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    W, H, n = 160, 120, 3
    rng = np.random.default_rng(8)
    pred, gt = _random_pairs(rng, n, 2, H, W, 9)
    (tmp_path / "pred.i8").write_bytes(pred.tobytes())
    (tmp_path / "gt.i8").write_bytes(gt.tobytes())
    out = str(tmp_path / "out.bin")
    r = subprocess.run([exe, os.path.join(golden_dir, "forest_multi.dat"), str(tmp_path / "pred.i8"), str(tmp_path / "gt.i8"),
                        str(n), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    N = n * 2 * H * W
    decoded = np.frombuffer(raw[:N], np.int8).reshape(n, 2, H, W)
    pos = N
    for l, C in enumerate((8, 9)):
        want_dec = np_decode(np_encode(gt[:, l], codings[l]), codings[l])
        assert np.array_equal(decoded[:, l], want_dec), l
        counts = np.frombuffer(raw[pos:pos + 8 * C * C], np.uint64).reshape(C, C); pos += 8 * C * C
        oor = int(np.frombuffer(raw[pos:pos + 8], np.uint64)[0]); pos += 8
        g = float(np.frombuffer(raw[pos:pos + 8], np.float64)[0]); pos += 8
        a, u = np.frombuffer(raw[pos:pos + 8], np.float32); pos += 8
        want, woor = np_confusion(pred[:, l], want_dec, C)
        assert np.array_equal(counts, want) and oor == woor
        rg, ra, ru, _ = reference_scores(want)
        assert g == rg and a == ra and u == ru
    rep = raw[pos:].decode()
    assert rep.startswith("confusion:\nArch           ") and "Class averge accuracy:" in rep
