"""Nothing leaks: the four live-resource counters of the library (device buffers, pinned host buffers, events, streams;
capi.debug_live_resources) return to their values from before the context after a context that has driven every family
of calls that allocates state is closed -- twice in a row in one process.

The counters are process-wide and count the owning handle types of csrc/rvseg_internal.h, so they see every hipMalloc /
hipHostMalloc / event / stream the library makes, but not a `new` without a `delete` (the three state structs have one
delete each: crf_state_free, fusion_state_free, eval_destroy)."""
import gc

import numpy as np
import pytest

from rovinasemanticsegmentation_amd import synthetic

pytestmark = pytest.mark.gpu

W, H = 160, 120
KINDS = ("device_buffers", "pinned_buffers", "events", "streams")


def _drive(rv, torch, ctx):
    """Every family of entry points that allocates context state; returns the counters while all of it is alive."""
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    N = W * H
    ctx.forest_load(synthetic.make_forest_bytes(seed=1, n_trees=2, leaves_per_tree=64, max_depth=8))
    cc = ctx.forest_info()["class_counts"]
    assert len(cc) == 2   # two label layers: the second CRF stream
    S = sum(cc)
    rgb, depth = synthetic.make_batch(4, W, H, holes=True)
    calib = synthetic.make_calib(W, H)

    # frame path, host entry: 4 frames with max_batch = 2 are two chunks, one per HostStage slot; pageable, then pinned
    out = ctx.segment_frames(rgb, depth, calib)
    bufs = ctx.host_buffers(4)
    bufs["rgb"][:] = rgb
    bufs["depth"][:] = depth
    ctx.segment_frames(bufs["rgb"], bufs["depth"], calib, out=bufs)
    assert np.array_equal(bufs["labels"], out["labels"])
    ctx.release_host_buffers(bufs)

    # frame path, device entry
    d_rgb = torch.from_numpy(rgb).to(dev)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(dev)
    d_post = torch.empty((4, S * N), dtype=torch.float32, device=dev)
    d_lab = torch.empty((4, 2, H, W), dtype=torch.int8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    ctx.segment_frames_device(4, d_rgb.data_ptr(), d_depth.data_ptr(), calib, d_post.data_ptr(), 0, d_lab.data_ptr(), s)
    torch.cuda.synchronize()
    ctx.poll_status(True)
    assert np.array_equal(d_lab.cpu().numpy(), out["labels"])

    # CRF entry points
    P, C = 600, 4
    U = rng.random((P, C), dtype=np.float32)
    f2 = (rng.random((P, 2), dtype=np.float32) * 20).astype(np.float32)
    f5 = (rng.random((P, 5), dtype=np.float32) * 20).astype(np.float32)
    ctx.crf_infer_multi(U, [f2, f5], [3.0, 5.0], 2)
    m = rng.random((C, C), dtype=np.float32)
    ctx.crf_infer_terms(U, [(f5, rv.MatrixCompatibility(m), rv.DIAG_KERNEL, rv.NORMALIZE_SYMMETRIC, None)], 2)
    ctx.crf_logistic_unary(rng.random((C, 3), dtype=np.float32), rng.random((P, 3), dtype=np.float32))
    ctx.lattice_build(f5)
    ctx.lattice_filter(U)

    # local-map fusion and the cloud CRF
    cloud = 500
    idx = rng.integers(-1, cloud, (4, H, W)).astype(np.int32)
    d_idx = torch.from_numpy(idx).to(dev)
    d_xyz = torch.from_numpy(rng.random((cloud, 3), dtype=np.float32)).to(dev)
    d_crgb = torch.from_numpy(rng.random((cloud, 3), dtype=np.float32)).to(dev)
    d_maplab = torch.empty((2, cloud), dtype=torch.int8, device=dev)
    ctx.process_map_device(4, d_idx.data_ptr(), d_post.data_ptr(), cloud, d_xyz.data_ptr(), d_crgb.data_ptr(), d_maplab.data_ptr(), 0, s)
    torch.cuda.synchronize()
    ctx.poll_status(True)
    ctx.fuse_posteriors(idx, out["posteriors"], cc, cloud)

    # forest evaluation, labelling, training
    X = synthetic.random_points(3, 300)
    ctx.forest_eval(X)
    ctx.label_values(U, rv.capi.LABEL_ARGMAX)
    ctx.forest_train(X[:, :16], rng.integers(0, 3, (300, 1)), [3], num_trees=1, max_depth=3)

    # scoring on two caller streams
    for l in range(2):
        ctx.color_coding_set(l, [{"name": str(k), "color": [k, 2 * k, 255 - k], "label": k} for k in range(cc[l])])
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    ctx.eval_reset()
    for st in streams:
        ctx.eval_accumulate_device(4, d_lab.data_ptr(), d_lab.data_ptr(), rv.capi.GT_LABELS, st.cuda_stream)
    counts, out_of_range = ctx.eval_confusion(0)
    assert int(counts.sum()) + out_of_range == 2 * 4 * N   # both streams' accumulates arrived

    open_counts = rv.capi.debug_live_resources()
    # a second model over the first (the scoring state is discarded with the first)
    ctx.forest_load(synthetic.make_forest_bytes(seed=2, n_trees=3, leaves_per_tree=32, max_depth=6, layer_classes=(5, 6, 7)))
    ctx.segment_frames(rgb[:1], depth[:1], calib)
    return open_counts


def test_context_releases_every_resource():
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    gc.collect()   # contexts of earlier tests that are garbage go now, not in the middle of the rounds
    before = rv.capi.debug_live_resources()
    after_round = []
    for _ in range(2):
        ctx = rv.Context(width=W, height=H, use_dense_crf=1, dcrf_iterations=2, label_mode=1, max_batch=2)
        try:
            open_counts = _drive(rv, torch, ctx)
        finally:
            ctx.close()
        after = rv.capi.debug_live_resources()
        print("live resources: before", before, "open", open_counts, "after close", after)
        for k in KINDS:
            assert open_counts[k] > before[k], k     # the counters see the handles these calls really use
            assert after[k] == before[k], k
        after_round.append(after)
    for k in KINDS:
        assert after_round[1][k] <= after_round[0][k], k
