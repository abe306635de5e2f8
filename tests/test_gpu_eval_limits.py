"""The scoring kernels (csrc/kernels_eval.hip) at every limit of their code: the whole-chunk scalar
path behind pointers that are not 16-byte aligned, hash chains across the wrap from slot 511 to slot 0 and a miss that
walks a full cluster, eight layers, the single-layer form on a high layer, C = 1, 63 and 64 with every bin hit, the
skip and out-of-range rules at the int8 extremes, the per-lane caches across a lane's chunks, the per-stream events,
and planes of 16, 20 and 25 pixels.  The recipes come from eval_cases.py and are pinned to their edges by
test_eval_cases_cpu.py.  Every comparison is exact: np.array_equal, or bytes, against the dict, the 256-entry table and
np.bincount of eval_cases."""
import numpy as np
import pytest

import eval_cases as ec
from rovinasemanticsegmentation_amd import synthetic

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
ALIGNMENTS = ((0, 0), (1, 0), (0, 1), (1, 1))      # byte offsets of (input, output) or (pred, gt) from a 16-byte boundary


def _torch():
    torch = pytest.importorskip("torch")
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def contexts(gpu_ctx_factory):
    """One context per (class counts, size, max_batch), kept for the module: scoring needs a loaded model, and runs no
    feature kernel (feature_color_patch=0 lets rvseg_create take 4 x 4)."""
    made = {}

    def get(classes, W, H, max_batch=67):
        key = (tuple(classes), W, H, max_batch)
        if key not in made:
            ctx = gpu_ctx_factory(width=W, height=H, stride=1, feature_color_patch=0, max_batch=max_batch)
            ctx.forest_load(synthetic.make_forest_bytes(seed=3, n_trees=1, leaves_per_tree=4, max_depth=3, D=ctx.feature_length,
                                                        layer_classes=tuple(classes)))
            assert ctx.forest_info()["class_counts"] == list(classes)
            made[key] = ctx
        return made[key]
    return get


@pytest.fixture(scope="module")
def side():
    torch, dev = _torch()
    return torch.cuda.Stream(dev), torch.cuda.Stream(dev)


@pytest.fixture(scope="module")
def wrap():
    return ec.wrap_cluster()


@pytest.fixture(scope="module")
def l8():
    return ec.layers8()


# ---- device buffers with a sentinel around them ---------------------------------------------------------------------------
def _upload(torch, dev, arr, off):
    """The bytes of `arr` on the device, `off` bytes past a 16-byte boundary; returns (tensor, address)"""
    raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
    buf = torch.full((16 + raw.size + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[off:off + raw.size] = torch.from_numpy(raw.copy()).to(dev)
    return buf, buf.data_ptr() + off


def _output(torch, dev, nbytes, off):
    buf = torch.full((16 + nbytes + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + off


def _check_output(buf, off, want, what):
    host = buf.cpu().numpy()
    raw = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    assert (host[:off] == SENTINEL).all() and (host[off + raw.size:] == SENTINEL).all(), "%s: bytes outside the output changed" % (what,)
    diff = host[off:off + raw.size] != raw
    assert not diff.any(), "%s: %d of %d bytes differ, first at %d" % (what, diff.sum(), diff.size, np.flatnonzero(diff)[:1])


def convert_all_ways(ctx, side, to_rgb, layer, inp, want, what):
    """The host entry, then the device entry on a side stream with aligned buffers and with the input, the output and
    both one byte off"""
    torch, dev = _torch()
    n = len(inp)
    got = ctx.labels_to_rgb(inp, layer) if to_rgb else ctx.labels_from_rgb(inp, layer)
    assert got.dtype == want.dtype and np.array_equal(got, want), "%s: host entry" % (what,)
    s = side[0]
    for off_in, off_out in ALIGNMENTS:
        d_in, p_in = _upload(torch, dev, inp, off_in)
        d_out, p_out = _output(torch, dev, want.size * want.itemsize, off_out)
        torch.cuda.synchronize(dev)
        if to_rgb:
            ctx.labels_to_rgb_device(n, p_in, p_out, layer, s.cuda_stream)
        else:
            ctx.labels_from_rgb_device(n, p_in, p_out, layer, s.cuda_stream)
        s.synchronize()
        _check_output(d_out, off_out, want, "%s: device entry, offsets %d / %d" % (what, off_in, off_out))
        _check_output(d_in, off_in, inp, "%s: the input" % (what,))


def check_confusion(ctx, want, what):
    """Every layer's counts and out-of-range counter in one go; want[l] = ref_confusion of layer l"""
    got = [ctx.eval_confusion(l) for l in range(len(want))]
    for l, ((counts, oor), (w_counts, w_oor, _)) in enumerate(zip(got, want)):
        assert counts.dtype == np.uint64 and np.array_equal(counts, w_counts), "%s: counts of layer %d" % (what, l)
        assert oor == w_oor, "%s: out of range of layer %d: %d, expected %d" % (what, l, oor, w_oor)


def confusion_device_all_ways(ctx, side, pred, gt, gt_format, want, what):
    torch, dev = _torch()
    s = side[0]
    for off_p, off_g in ALIGNMENTS:
        d_p, p_p = _upload(torch, dev, pred, off_p)
        d_g, p_g = _upload(torch, dev, gt, off_g)
        torch.cuda.synchronize(dev)
        ctx.eval_reset()
        ctx.eval_accumulate_device(len(pred), p_p, p_g, gt_format, s.cuda_stream)
        check_confusion(ctx, want, "%s: device entry, offsets %d / %d" % (what, off_p, off_g))
        _check_output(d_p, off_p, pred, "%s: pred" % (what,))
        _check_output(d_g, off_g, gt, "%s: gt" % (what,))


def _size_id(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# ---- decode and encode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ec.SIZES, ids=_size_id)
def test_wrap_cluster_decode(contexts, side, wrap, size):
    """Chains that cross slot 511 -> 0, the colour 255 probes from its home, unknown colours that walk the whole
    cluster, land inside it or in the empty half, black, white and one-step neighbours; every missing_label"""
    W, H = size
    ctx = contexts((2,), W, H)
    for i, n in enumerate(ec.FRAME_COUNTS):
        rgb = ec.frames([ec.colors_of(ec.wrap_stream(wrap, n * W * H, seed=i))], n, W, H)[:, 0]
        for missing in ec.MISSING_LABELS:
            ctx.color_coding_set(0, wrap["coding"], missing_label=missing)
            want = ec.ref_decode(rgb, wrap["coding"], missing)
            assert (want == missing).any()
            convert_all_ways(ctx, side, False, 0, rgb, want, "n %d, missing %d" % (n, missing))


@pytest.mark.parametrize("size", ec.SIZES, ids=_size_id)
def test_wrap_cluster_encode(contexts, side, wrap, size):
    """Every int8 label through a 256-entry coding with repeated labels: the last colour of a label, else black"""
    W, H = size
    ctx = contexts((2,), W, H)
    ctx.color_coding_set(0, wrap["coding"])
    for i, n in enumerate(ec.FRAME_COUNTS):
        lab = ec.frames([ec.label_stream(n * W * H, seed=i)], n, W, H)[:, 0]
        want = ec.ref_encode(lab, wrap["coding"])
        assert want.any() and not want.reshape(-1, 3).any(1).all()
        convert_all_ways(ctx, side, True, 0, lab, want, "n %d" % n)


@pytest.mark.parametrize("size", ec.SIZES, ids=_size_id)
def test_alternating_decode(contexts, side, size):
    """Two colours of hash 511 (slots 511 and 0) alternate pixel by pixel; runs of 4096 + 7 pixels where they fit"""
    W, H = size
    ctx = contexts((2,), W, H)
    for n in ec.FRAME_COUNTS:
        a = ec.alternating(n * W * H, 2)
        ctx.color_coding_set(0, a["coding"], missing_label=-128)
        rgb = ec.frames([ec.colors_of(a["keys"])], n, W, H)[:, 0]
        want = ec.ref_decode(rgb, a["coding"], -128)
        convert_all_ways(ctx, side, False, 0, rgb, want, "n %d" % n)
        convert_all_ways(ctx, side, True, 0, want, ec.ref_encode(want, a["coding"]), "n %d, back to colours" % n)


@pytest.mark.parametrize("size", ec.SIZES, ids=_size_id)
def test_layers8_decode_and_encode(contexts, side, l8, size):
    """Eight layers, each with its own coding; the same bytes decode differently per layer.  The all-layers call, and
    the single-layer call on layers 0, 3 and 7."""
    W, H = size
    ctx = contexts(ec.LAYERS8, W, H)
    missing = (0, -1, -128, 127, 5, -7, 64, 1)
    for l in range(8):
        ctx.color_coding_set(l, l8["codings"][l], missing_label=missing[l])
    for i, n in enumerate(ec.FRAME_COUNTS):
        total = n * W * H
        rgb = ec.frames([ec.colors_of(s) for s in ec.layers8_streams(l8, total, seed=i)], n, W, H)
        want = np.stack([ec.ref_decode(rgb[:, l], l8["codings"][l], missing[l]) for l in range(8)], 1)
        assert len({want[:, l].tobytes() for l in range(8)}) == 8
        convert_all_ways(ctx, side, False, -1, rgb, want, "decode n %d, all layers" % n)
        lab = ec.frames([ec.label_stream(total, seed=i + l) for l in range(8)], n, W, H)
        want_rgb = np.stack([ec.ref_encode(lab[:, l], l8["codings"][l]) for l in range(8)], 1)
        convert_all_ways(ctx, side, True, -1, lab, want_rgb, "encode n %d, all layers" % n)
        for l in (0, 3, 7):
            convert_all_ways(ctx, side, False, l, np.ascontiguousarray(rgb[:, l]), np.ascontiguousarray(want[:, l]), "decode n %d, layer %d" % (n, l))
            convert_all_ways(ctx, side, True, l, np.ascontiguousarray(lab[:, l]), np.ascontiguousarray(want_rgb[:, l]), "encode n %d, layer %d" % (n, l))


@pytest.mark.parametrize("size", ec.SIZES, ids=_size_id)
def test_layers8_encode_then_decode(contexts, l8, size):
    """Labels of the tables come back; labels outside them encode to black, and black decodes to `missing`"""
    W, H = size
    ctx = contexts(ec.LAYERS8, W, H)
    for l in range(8):
        ctx.color_coding_set(l, l8["codings"][l], missing_label=-5)
    n = 3
    lab = ec.frames([ec.table_labels_stream(l8["codings"][l], n * W * H, l) for l in range(8)], n, W, H)
    rgb = ctx.labels_to_rgb(lab)
    assert np.array_equal(rgb, np.stack([ec.ref_encode(lab[:, l], l8["codings"][l]) for l in range(8)], 1))
    assert np.array_equal(ctx.labels_from_rgb(rgb), lab)
    outside = np.empty_like(lab)
    for l in range(8):
        used = sorted({int(np.int64(e["label"]).astype(np.int8)) for e in l8["codings"][l]})
        free = np.array([v for v in range(-128, 128) if v not in used], np.int8)
        outside[:, l] = free[np.arange(n * W * H) % len(free)].reshape(n, H, W)
    black = ctx.labels_to_rgb(outside)
    assert not black.any()
    assert (ctx.labels_from_rgb(black) == -5).all()


# ---- confusion --------------------------------------------------------------------------------------------------------------
def _gt_formats():
    import rovinasemanticsegmentation_amd as rv
    return rv.capi.GT_LABELS, rv.capi.GT_RGB


@pytest.mark.parametrize("case", ec.bins_cases(), ids=_size_id)
def test_bins_confusion(contexts, side, case):
    """Every one of the C * C bins, the 36 pairs of the int8 extremes, a plane without runs and a plane whose runs are
    cut by a skipped and by an out-of-range pixel; through the host entry with max_batch 1, 2 and n, and through the
    device entry at the four alignments"""
    C, W, H, n = case
    GT_LABELS, GT_RGB = _gt_formats()
    b = ec.bins(C)
    pred = ec.frames([ec.fit(b["pred"], n * W * H)], n, W, H)
    gt = ec.frames([ec.fit(b["gt"], n * W * H)], n, W, H)
    want = [ec.ref_confusion(pred, gt, C)]
    assert (want[0][0] >= 2).all() and want[0][1] > 0 and want[0][2] > 0
    for max_batch in sorted({1, 2, n}):
        ctx = contexts((C,), W, H, max_batch)
        ctx.eval_reset()
        ctx.eval_accumulate(pred, gt, GT_LABELS)
        check_confusion(ctx, want, "host entry, max_batch %d" % max_batch)
    confusion_device_all_ways(contexts((C,), W, H, n), side, pred, gt, GT_LABELS, want, "int8 gt")


@pytest.mark.parametrize("case", ec.bins_cases(), ids=_size_id)
def test_rgb_gt_confusion(contexts, side, case):
    """The same pairs with the ground truth as colours, some of them not in the table: scored as missing_label -1
    (skipped), 0 and C (out of range)"""
    C, W, H, n = case
    GT_LABELS, GT_RGB = _gt_formats()
    r = ec.rgb_gt(C)
    pred = ec.frames([ec.fit(r["pred"], n * W * H)], n, W, H)
    gt_rgb = ec.frames([ec.fit(r["gt_rgb"], n * W * H)], n, W, H)
    for missing in r["missing"]:
        want = [ec.ref_confusion(pred, ec.ref_decode(gt_rgb, r["coding"], missing), C)]
        for max_batch in sorted({1, 2, n}):
            ctx = contexts((C,), W, H, max_batch)
            ctx.color_coding_set(0, r["coding"], missing_label=missing)
            ctx.eval_reset()
            ctx.eval_accumulate(pred, gt_rgb, GT_RGB)
            check_confusion(ctx, want, "missing %d, host entry, max_batch %d" % (missing, max_batch))
        confusion_device_all_ways(contexts((C,), W, H, n), side, pred, gt_rgb, GT_RGB, want, "missing %d, rgb gt" % missing)
    # the same images through the conversions (the coding of the last round is still set)
    gt = ec.ref_decode(gt_rgb[:, 0], r["coding"], missing)
    convert_all_ways(ctx, side, False, 0, np.ascontiguousarray(gt_rgb[:, 0]), gt, "decode")
    convert_all_ways(ctx, side, True, 0, gt, ec.ref_encode(gt, r["coding"]), "encode")


def _layers8_gt_coding(l):
    """Twenty colours, the same in every layer, for the labels -2 .. 17 rotated by the layer"""
    cols = [[10 + 3 * j, 200 - j, (j * 29) & 255] for j in range(20)]
    return ec.entries([cols[(v + 2 + l) % 20] for v in range(-2, 18)], list(range(-2, 18)))


@pytest.mark.parametrize("size", ec.SIZES, ids=_size_id)
def test_layers8_confusion(contexts, side, size):
    """All eight layers' counts and out-of-range counters from one call: the LayerClasses pack, the layer * 64 * 64
    offset, the counter slot behind the counts, tables + layer"""
    W, H = size
    GT_LABELS, GT_RGB = _gt_formats()
    codings = [_layers8_gt_coding(l) for l in range(8)]
    for i, n in enumerate(ec.FRAME_COUNTS):
        p, g = ec.layers8_labels(n * W * H, seed=i)
        pred, gt = ec.frames(p, n, W, H), ec.frames(g, n, W, H)
        gt_rgb = np.stack([ec.ref_encode(gt[:, l], codings[l]) for l in range(8)], 1)
        want = [ec.ref_confusion(pred[:, l], gt[:, l], C) for l, C in enumerate(ec.LAYERS8)]
        want_rgb = [ec.ref_confusion(pred[:, l], ec.ref_decode(gt_rgb[:, l], codings[l], -1), C) for l, C in enumerate(ec.LAYERS8)]
        assert all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(want, want_rgb))
        for max_batch in sorted({1, 2, n}):
            ctx = contexts(ec.LAYERS8, W, H, max_batch)
            for l in range(8):
                ctx.color_coding_set(l, codings[l], missing_label=-1)
            for fmt, data in ((GT_LABELS, gt), (GT_RGB, gt_rgb)):
                ctx.eval_reset()
                ctx.eval_accumulate(pred, data, fmt)
                check_confusion(ctx, want, "n %d, host entry, max_batch %d, format %d" % (n, max_batch, fmt))
        ctx = contexts(ec.LAYERS8, W, H, n)
        confusion_device_all_ways(ctx, side, pred, gt, GT_LABELS, want, "n %d, int8 gt" % n)
        confusion_device_all_ways(ctx, side, pred, gt_rgb, GT_RGB, want, "n %d, rgb gt" % n)


def test_smaller_model_counts_its_own_layers_only(contexts, side):
    """The first three layers of the eight-layer data on a model of three layers: the same counts per layer, and no
    layer beyond the model's can be asked for (the counters of layers >= L are not readable through the API; the
    eight-layer comparison holds every slot of the counter array)"""
    import rovinasemanticsegmentation_amd as rv
    W, H, n = 17, 5, 3
    GT_LABELS, GT_RGB = _gt_formats()
    p, g = ec.layers8_labels(n * W * H)
    pred, gt = ec.frames(p[:3], n, W, H), ec.frames(g[:3], n, W, H)
    want = [ec.ref_confusion(pred[:, l], gt[:, l], C) for l, C in enumerate(ec.LAYERS8[:3])]
    ctx = contexts(ec.LAYERS8[:3], W, H, n)
    ctx.eval_reset()
    ctx.eval_accumulate(pred, gt, GT_LABELS)
    check_confusion(ctx, want, "three layers")
    for layer in (3, 7, 8, -1):
        with pytest.raises(rv.capi.RvsegError) as e:
            ctx.eval_confusion(layer)
        assert e.value.status == rv.capi.ERR_INVALID_ARG
    check_confusion(ctx, want, "three layers, after the refused call")


# ---- grid stride: a lane's second chunk -------------------------------------------------------------------------------------
def test_grid_stride_eight_layers_vga(contexts, side):
    """Eight layers of 640 x 480 and enough frames that a lane takes a second chunk: a run of one colour (and one
    (pred, gt) pair) reaches from a lane's first chunk into its next and ends inside it, so last_key / last_label and
    run_key / run_n are carried from one chunk to the next"""
    torch, dev = _torch()
    GT_LABELS, GT_RGB = _gt_formats()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    n, layers = ec.grid_stride_case(cus)
    W, H = ec.GRID_W, ec.GRID_H
    chunks = n * (W * H // ec.CHUNK)
    print("grid stride: %d CUs, %d frames, %d chunks per layer, %d lanes per grid row" % (cus, n, chunks, ec.THREADS * ec.launch_blocks(cus, 8)))
    assert chunks > ec.THREADS * ec.launch_blocks(cus, 8)                       # the conversions: 8 blocks per CU over 8 rows
    assert chunks > ec.THREADS * ec.launch_blocks(cus, 8, max(ec.LAYERS8))      # the confusion at C = 16
    for a in layers:
        (start, length, key), = a["runs"]
        assert length == ec.THREADS * ec.launch_blocks(cus, 8) * ec.CHUNK + 7 and (start + length) // ec.CHUNK < chunks
    ctx = contexts(ec.LAYERS8, W, H, n)
    for l, a in enumerate(layers):
        ctx.color_coding_set(l, a["coding"], missing_label=-1)
    rgb = ec.frames([ec.colors_of(a["keys"]) for a in layers], n, W, H)
    pred = ec.frames([a["pred"] for a in layers], n, W, H)
    lab = np.stack([ec.ref_decode(rgb[:, l], a["coding"], -1) for l, a in enumerate(layers)], 1)
    convert_all_ways(ctx, side, False, -1, rgb, lab, "decode")
    convert_all_ways(ctx, side, True, -1, lab, np.stack([ec.ref_encode(lab[:, l], a["coding"]) for l, a in enumerate(layers)], 1), "encode")
    convert_all_ways(ctx, side, False, 7, np.ascontiguousarray(rgb[:, 7]), np.ascontiguousarray(lab[:, 7]), "decode, layer 7")
    want = [ec.ref_confusion(pred[:, l], lab[:, l], C) for l, C in enumerate(ec.LAYERS8)]
    assert all(w[0].sum() > (1 << 20) for w in want[1:])
    for fmt, gt in ((GT_LABELS, lab), (GT_RGB, rgb)):
        ctx.eval_reset()
        ctx.eval_accumulate(pred, gt, fmt)
        check_confusion(ctx, want, "host entry, format %d" % fmt)
        confusion_device_all_ways(ctx, side, pred, gt, fmt, want, "format %d" % fmt)


# ---- streams ----------------------------------------------------------------------------------------------------------------
def _keep_busy(torch, dev, stream, scratch):
    """Some milliseconds of device work on `stream`, so that what is enqueued behind it has not run when the host goes on"""
    with torch.cuda.stream(stream):
        for _ in range(40):
            scratch.add_(1)


@pytest.fixture(scope="module")
def scratch():
    torch, dev = _torch()
    return torch.zeros(1 << 27, dtype=torch.uint8, device=dev)


def test_confusion_waits_for_every_stream_and_reset_clears(contexts, side, scratch):
    """Three disjoint parts of one recipe accumulated on two torch streams and the context's own, no host
    synchronisation: rvseg_eval_confusion gives the counts of the whole; rvseg_eval_reset straight after enqueued work
    gives zeros"""
    torch, dev = _torch()
    GT_LABELS, GT_RGB = _gt_formats()
    C, W, H, n = 64, 161, 97, 3
    r = ec.rgb_gt(C)
    pred = ec.frames([ec.fit(np.roll(r["pred"], 100), n * W * H)], n, W, H)
    gt = ec.frames([ec.fit(r["gt"], n * W * H)], n, W, H)
    gt_rgb = ec.frames([ec.fit(r["gt_rgb"], n * W * H)], n, W, H)
    ctx = contexts((C,), W, H, n)
    ctx.color_coding_set(0, r["coding"], missing_label=0)
    d_p, p_p = _upload(torch, dev, pred, 0)
    d_g, p_g = _upload(torch, dev, gt, 0)
    d_c, p_c = _upload(torch, dev, gt_rgb, 0)
    torch.cuda.synchronize(dev)
    P = W * H
    streams = (side[0].cuda_stream, side[1].cuda_stream, 0)                  # 0: the context's own stream
    for fmt, p_gt, b, host_gt in ((GT_LABELS, p_g, 1, gt), (GT_RGB, p_c, 3, ec.ref_decode(gt_rgb, r["coding"], 0))):
        want = [ec.ref_confusion(pred, host_gt, C)]
        ctx.eval_reset()
        _keep_busy(torch, dev, side[0], scratch)
        _keep_busy(torch, dev, side[1], scratch)
        for f, s in enumerate(streams):
            ctx.eval_accumulate_device(1, p_p + f * P, p_gt + f * P * b, fmt, s)
        check_confusion(ctx, want, "three streams, format %d" % fmt)
        # a second round on top, then a reset while it is still enqueued
        _keep_busy(torch, dev, side[0], scratch)
        for f, s in enumerate(streams):
            ctx.eval_accumulate_device(1, p_p + f * P, p_gt + f * P * b, fmt, s)
        ctx.eval_reset()
        zero = [(np.zeros((C, C), np.uint64), 0, 0)]
        check_confusion(ctx, zero, "after reset")
        torch.cuda.synchronize(dev)
        check_confusion(ctx, zero, "after reset and a device synchronise")
        ctx.eval_accumulate_device(n, p_p, p_gt, fmt, side[1].cuda_stream)
        check_confusion(ctx, want, "one pass after the reset")
    ctx.eval_reset()


def test_color_coding_set_waits_for_a_conversion_on_a_side_stream(contexts, side, scratch, wrap):
    """A conversion enqueued on a side stream reads the table it was enqueued under, the next one the new table"""
    torch, dev = _torch()
    W, H, n = 161, 97, 3
    ctx = contexts((2,), W, H)
    old = wrap["coding"]
    new = ec.entries([e["color"] for e in old[:200]], [(e["label"] + 1 + 128) % 256 - 128 for e in old[:200]])
    rgb = ec.frames([ec.colors_of(ec.wrap_stream(wrap, n * W * H, seed=2))], n, W, H)[:, 0]
    want_old, want_new = ec.ref_decode(rgb, old, -1), ec.ref_decode(rgb, new, 3)
    assert (want_old != want_new).mean() > 0.5
    d_in, p_in = _upload(torch, dev, rgb, 0)
    d_1, p_1 = _output(torch, dev, want_old.size, 0)
    d_2, p_2 = _output(torch, dev, want_new.size, 0)
    torch.cuda.synchronize(dev)
    ctx.color_coding_set(0, old, missing_label=-1)
    _keep_busy(torch, dev, side[0], scratch)
    ctx.labels_from_rgb_device(n, p_in, p_1, 0, side[0].cuda_stream)
    ctx.color_coding_set(0, new, missing_label=3)
    ctx.labels_from_rgb_device(n, p_in, p_2, 0, side[0].cuda_stream)
    side[0].synchronize()
    _check_output(d_1, 0, want_old, "the conversion enqueued before the new table")
    _check_output(d_2, 0, want_new, "the conversion enqueued after it")
