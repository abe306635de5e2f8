"""The external-semantics path on the GPU (include/rvseg.h "external semantics"; replaces
Segmenter::processFramesFromQueueExternal, src/segmenter.cpp:445-514) against the oracle composition of
tests/external_cases.py.  The bar is the project's own: max|diff| <= 1e-4 first, then equal float32 bit patterns;
labels equal.  No test here loads a forest unless it says so."""
import ctypes as C

import numpy as np
import pytest

import external_cases as X
from frame_cases import bits

pytestmark = pytest.mark.gpu


def same_floats(got, want, what=""):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    both_nan = np.isnan(got) & np.isnan(want)
    diff = np.where(both_nan, 0, np.abs(got.astype(np.float64) - want.astype(np.float64)))
    assert not np.isnan(diff).any(), (what, "NaN on one side only")
    assert diff.max() <= 1e-4, (what, diff.max())
    assert np.array_equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).sum()))


def _torch():
    torch = pytest.importorskip("torch")
    return torch, torch.device("cuda", 0)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(torch, dev, a):
    """A device copy of a (possibly read-only) numpy array; uint16 travels as int16"""
    a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


# ---- rectify ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(160, 120), (5, 5)])
def test_rectify_depth_equals_the_oracle_cloud(gpu_ctx_factory, W, H):
    """rvseg_create accepts 4 x 4 upwards (no colour patch): 5 x 5 is the smallest size whose W * H is no multiple of
    four.  With three frames the 75 pixels leave a scalar tail of three, groups of four straddle row ends AND frame
    ends, and W is odd."""
    torch, dev = _torch()
    n = 3
    depth, cal = X.rectify_depths(n, W, H), X.calibs(n, W, H)
    ctx = gpu_ctx_factory(width=W, height=H, stride=1, feature_color_patch=0, depth_min=X.OWN_LIMITS[0], depth_max=X.OWN_LIMITS[1])
    d_depth = _dev(torch, dev, depth)
    s = torch.cuda.current_stream(dev).cuda_stream
    for dmin, dmax in ((0.5, 15.0), (ctx.params.depth_min, ctx.params.depth_max)):
        want = X.expected_xyz(depth, cal, W, H, dmin, dmax)
        assert np.isnan(want).any() and np.isfinite(want).any()
        host = ctx.rectify_depth(depth, cal, dmin, dmax)
        same_floats(host, want, (W, H, dmin))
        d_xyz = torch.full((n, H, W, 3), -7.0, dtype=torch.float32, device=dev)
        ctx.rectify_depth_device(n, d_depth.data_ptr(), cal, d_xyz.data_ptr(), dmin, dmax, s)
        torch.cuda.synchronize(dev)
        assert d_xyz.cpu().numpy().tobytes() == host.tobytes()
    # the facade's defaults are the reference's hard-coded 0.5 / 15.0
    assert ctx.rectify_depth(depth, cal).tobytes() == ctx.rectify_depth(depth, cal, 0.5, 15.0).tobytes()


def test_rectify_depth_with_unaligned_device_pointers(gpu_ctx_factory):
    """Pointers that are not aligned for the 8-byte load / 16-byte stores take the one-pixel path: same bytes"""
    torch, dev = _torch()
    W, H, n = 160, 120, 2
    depth, cal = X.rectify_depths(n, W, H), X.calibs(n, W, H)
    ctx = gpu_ctx_factory(width=W, height=H, stride=1, feature_color_patch=0)
    want = X.expected_xyz(depth, cal, W, H, 0.5, 15.0)
    buf_d = torch.zeros(n * W * H + 1, dtype=torch.int16, device=dev)
    buf_d[1:] = _dev(torch, dev, depth).ravel()
    buf_x = torch.zeros(n * W * H * 3 + 1, dtype=torch.float32, device=dev)
    ctx.rectify_depth_device(n, buf_d.data_ptr() + 2, cal, buf_x.data_ptr() + 4, 0.5, 15.0, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = buf_x.cpu().numpy()
    assert got[0] == 0.0
    same_floats(got[1:].reshape(want.shape), want)


# ---- the frame path -----------------------------------------------------------------------------------------------------------
FULL = dict(W=160, H=120, layers=(8, 9), n=3, unknown=(7, 8))


def _full_case():
    c = FULL
    rgb, depth = X.frames(c["n"], c["W"], c["H"])
    return rgb, depth, X.calibs(c["n"], c["W"], c["H"]), X.log_softmax_distributions(11, c["n"], c["layers"], c["H"], c["W"])


@pytest.mark.parametrize("mode", [X.LABEL_EVAL, X.LABEL_CRF, X.LABEL_NOCRF, X.LABEL_ARGMAX])
def test_full_resolution_host_and_device_entry(gpu_ctx_factory, mode):
    """160 x 120, layers (8, 9), three frames in chunks of 2 + 1, no forest on the context"""
    torch, dev = _torch()
    import rovinasemanticsegmentation_amd as rv
    c = FULL
    W, H, layers, n = c["W"], c["H"], c["layers"], c["n"]
    rgb, depth, cal, dist = _full_case()
    want_marg, want_lab = X.expected_cached(("full", mode), rgb, depth, cal, dist, layers, W, H, mode, c["unknown"])
    ctx = gpu_ctx_factory(width=W, height=H, use_dense_crf=1, dcrf_iterations=3, label_mode=mode, max_batch=2, unknown_label=c["unknown"])
    with pytest.raises(rv.capi.RvsegError) as e:
        ctx.forest_info()
    assert e.value.status == rv.capi.ERR_NO_FOREST
    ctx.external_layers_set(layers)
    out = ctx.segment_external(rgb, depth, cal, dist)
    same_floats(out["marginals"], want_marg, "host marginals")
    assert np.array_equal(out["labels"].reshape(want_lab.shape), want_lab)
    assert ctx.last_schedule()["n_frames"] == 1 and "lattice_build" in ctx.last_timing()   # the last chunk: one frame

    N, S = W * H, sum(layers)
    d_rgb = _dev(torch, dev, rgb)
    d_depth = _dev(torch, dev, depth)
    d_dist = _dev(torch, dev, dist)
    d_marg = torch.zeros((n, S * N), dtype=torch.float32, device=dev)
    d_lab = torch.zeros((n, len(layers), N), dtype=torch.int8, device=dev)
    ctx.segment_external_device(n, d_rgb.data_ptr(), d_depth.data_ptr(), cal, d_dist.data_ptr(), 1, d_marg.data_ptr(), d_lab.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream)
    assert ctx.poll_status(wait=True) == rv.capi.OK
    torch.cuda.synchronize(dev)
    assert d_marg.cpu().numpy().tobytes() == out["marginals"].tobytes()
    assert np.array_equal(d_lab.cpu().numpy(), want_lab)
    assert d_dist.cpu().numpy().tobytes() == dist.tobytes(), "the distributions are read in place, never written"


@pytest.mark.parametrize("layers", [(1,), (2, 21, 22), (8,) * 8], ids=["1", "2-21-22", "8x8"])
def test_layer_layouts(gpu_ctx_factory, layers):
    """One class; class counts with and without a fused update, three layers on two streams; 8 layers summing to 64"""
    W, H, n = 160, 120, 2
    rgb, depth = X.frames(n, W, H)
    cal = X.calibs(n, W, H)
    dist = X.log_softmax_distributions(17, n, layers, H, W)
    unknown = tuple(c - 1 for c in layers)
    want_marg, want_lab = X.expected(rgb, depth, cal, dist, layers, W, H, X.LABEL_CRF, unknown)
    ctx = gpu_ctx_factory(width=W, height=H, use_dense_crf=1, dcrf_iterations=3, label_mode=X.LABEL_CRF, max_batch=2, unknown_label=unknown)
    ctx.external_layers_set(layers)
    out = ctx.segment_external(rgb, depth, cal, dist)
    same_floats(out["marginals"], want_marg)
    assert np.array_equal(out["labels"].reshape(want_lab.shape), want_lab)
    only_labels = ctx.segment_external(rgb, depth, cal, dist, want_marginals=False)
    assert only_labels["marginals"] is None and np.array_equal(only_labels["labels"], out["labels"])


@pytest.mark.parametrize("W,H,layers", [(192, 128, (8, 9)), (160, 120, (3, 11))], ids=["tiled", "perC-generic"])
def test_low_resolution_distributions(gpu_ctx_factory, W, H, layers):
    """stride 4, dist_stride 4: 192 x 128 with (8, 9) is eligible for the tiled up-sampler, 160 x 120 with (3, 11) takes
    the per-class-count kernel (3) and the generic one (11)"""
    torch, dev = _torch()
    n, s = 2, 4
    rgb, depth = X.frames(n, W, H)
    cal = X.calibs(n, W, H)
    dist = X.log_softmax_distributions(13, n, layers, H // s, W // s)
    unknown = tuple(c - 1 for c in layers)
    want_marg, want_lab = X.expected(rgb, depth, cal, dist, layers, W, H, X.LABEL_CRF, unknown, dist_stride=s)
    kw = dict(width=W, height=H, stride=s, use_dense_crf=1, dcrf_iterations=3, label_mode=X.LABEL_CRF, max_batch=2, unknown_label=unknown)
    ctx = gpu_ctx_factory(**kw)
    ctx.external_layers_set(layers)
    out = ctx.segment_external(rgb, depth, cal, dist, dist_stride=s)
    same_floats(out["marginals"], want_marg)
    assert np.array_equal(out["labels"].reshape(want_lab.shape), want_lab)
    # without the CRF the labels are those of the up-sampled image itself
    plain = gpu_ctx_factory(**dict(kw, use_dense_crf=0, label_mode=X.LABEL_NOCRF))
    plain.external_layers_set(layers)
    _, want_plain = X.expected(rgb, depth, cal, dist, layers, W, H, X.LABEL_NOCRF, unknown, crf=False, dist_stride=s)
    assert np.array_equal(plain.segment_external(rgb, depth, cal, dist, dist_stride=s)["labels"].reshape(want_plain.shape), want_plain)
    # device entry: same bytes
    N, S = W * H, sum(layers)
    d_rgb = _dev(torch, dev, rgb)
    d_depth = _dev(torch, dev, depth)
    d_dist = _dev(torch, dev, dist)
    d_marg = torch.zeros((n, S * N), dtype=torch.float32, device=dev)
    ctx.segment_external_device(n, d_rgb.data_ptr(), d_depth.data_ptr(), cal, d_dist.data_ptr(), s, d_marg.data_ptr(), 0,
                                torch.cuda.current_stream(dev).cuda_stream)
    ctx.poll_status(wait=True)
    torch.cuda.synchronize(dev)
    assert d_marg.cpu().numpy().tobytes() == out["marginals"].tobytes()


@pytest.mark.parametrize("mode", [X.LABEL_NOCRF, X.LABEL_EVAL])
def test_without_dense_crf_the_distributions_are_labelled(gpu_ctx_factory, mode):
    c = FULL
    W, H, layers = c["W"], c["H"], c["layers"]
    rgb, depth, cal, dist = _full_case()
    _, want_lab = X.expected(rgb, depth, cal, dist, layers, W, H, mode, c["unknown"], crf=False)
    ctx = gpu_ctx_factory(width=W, height=H, use_dense_crf=0, label_mode=mode, max_batch=2, unknown_label=c["unknown"])
    ctx.external_layers_set(layers)
    out = ctx.segment_external(rgb, depth, cal, dist)
    assert out["marginals"] is None
    assert np.array_equal(out["labels"].reshape(want_lab.shape), want_lab)
    # marginals_out is ignored without the CRF, as rvseg_segment_frames ignores it
    marg = np.full((c["n"], sum(layers) * W * H), 5.0, np.float32)
    lab = np.empty((c["n"], len(layers), H, W), np.int8)
    calib = np.ascontiguousarray(cal, np.float32)
    st = ctx.L.rvseg_segment_external(ctx.h, c["n"], _ptr(rgb), _ptr(depth), _ptr(calib), _ptr(dist), 1, _ptr(marg), _ptr(lab))
    assert st == 0 and (marg == 5.0).all() and np.array_equal(lab, out["labels"])


def test_forest_and_external_layout_are_independent(gpu_ctx_factory, oracle):
    from rovinasemanticsegmentation_amd import synthetic
    W, H, n, layers = 160, 120, 2, (3, 5)
    blob = synthetic.make_forest_bytes(seed=1, n_trees=4, leaves_per_tree=256, max_depth=12)
    rgb, depth = X.frames(n, W, H)
    cal = X.calibs(n, W, H)
    dist = X.log_softmax_distributions(19, n, layers, H, W)
    want_marg, want_lab = X.expected(rgb, depth, cal, dist, layers, W, H, X.LABEL_CRF, (7, 8))
    ctx = gpu_ctx_factory(width=W, height=H, use_dense_crf=1, dcrf_iterations=3, label_mode=X.LABEL_CRF, max_batch=2)
    ctx.external_layers_set(layers)
    ctx.forest_load(blob)                       # after the layout: the layout stays
    assert ctx.forest_info()["class_counts"] == [8, 9]
    first = ctx.segment_frames(rgb, depth, cal)
    ext = ctx.segment_external(rgb, depth, cal, dist)
    second = ctx.segment_frames(rgb, depth, cal)
    for k in ("posteriors", "marginals", "labels"):
        assert first[k].tobytes() == second[k].tobytes(), k
    same_floats(ext["marginals"], want_marg)
    assert np.array_equal(ext["labels"].reshape(want_lab.shape), want_lab)
    # the forest path is the oracle's still
    p = oracle.default_params(width=W, height=H, dcrf_iterations=3)
    post, marg, lab = oracle.segment_frame(p, oracle.Forest(blob), 1, rgb[0], depth[0], cal[0], label_mode=1, unknown=[7, 8])
    assert np.array_equal(first["posteriors"][0], post) and np.array_equal(first["marginals"][0], marg)
    ctx.external_layers_set((8, 9))             # and a new layout leaves the forest alone
    assert ctx.segment_frames(rgb, depth, cal)["marginals"].tobytes() == first["marginals"].tobytes()


# ---- overflow contract ------------------------------------------------------------------------------------------------------
def test_host_entry_recovers_from_hash_overflow(gpu_ctx_factory):
    """2^4 slots per frame cannot hold a frame's lattice: a handled status.  The host entry redoes the chunk."""
    c = FULL
    W, H, layers = c["W"], c["H"], c["layers"]
    rgb, depth, cal, dist = _full_case()
    want_marg, want_lab = X.expected_cached(("full", X.LABEL_CRF), rgb, depth, cal, dist, layers, W, H, X.LABEL_CRF, c["unknown"])
    ctx = gpu_ctx_factory(width=W, height=H, use_dense_crf=1, dcrf_iterations=3, label_mode=X.LABEL_CRF, max_batch=2,
                          lattice_capacity_log2=4, unknown_label=c["unknown"])
    ctx.external_layers_set(layers)
    out = ctx.segment_external(rgb, depth, cal, dist)
    same_floats(out["marginals"], want_marg)
    assert np.array_equal(out["labels"].reshape(want_lab.shape), want_lab)
    assert ctx.last_schedule()["capacity_log2"] > 4


def test_device_entry_reports_overflow_through_poll_status(gpu_ctx_factory):
    torch, dev = _torch()
    import rovinasemanticsegmentation_amd as rv
    c = FULL
    W, H, layers, n = c["W"], c["H"], c["layers"], 2
    rgb, depth, cal, dist = _full_case()
    want_marg, want_lab = X.expected_cached(("full", X.LABEL_CRF), rgb, depth, cal, dist, layers, W, H, X.LABEL_CRF, c["unknown"])
    ctx = gpu_ctx_factory(width=W, height=H, use_dense_crf=1, dcrf_iterations=3, label_mode=X.LABEL_CRF, max_batch=2,
                          lattice_capacity_log2=4, unknown_label=c["unknown"])
    ctx.external_layers_set(layers)
    N, S = W * H, sum(layers)
    d_rgb = _dev(torch, dev, rgb[:n])
    d_depth = _dev(torch, dev, depth[:n])
    d_dist = _dev(torch, dev, dist[:n])
    d_marg = torch.zeros((n, S * N), dtype=torch.float32, device=dev)
    d_lab = torch.zeros((n, len(layers), N), dtype=torch.int8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream

    def call():
        ctx.segment_external_device(n, d_rgb.data_ptr(), d_depth.data_ptr(), cal[:n], d_dist.data_ptr(), 1, d_marg.data_ptr(), d_lab.data_ptr(), s)

    call()
    seen = 0
    for _ in range(8):   # 2^4 -> 2^7 -> 2^10 ...: each report raises the capacity eightfold
        try:
            assert ctx.poll_status(wait=True) == rv.capi.OK
            break
        except rv.capi.RvsegError as e:
            assert e.status == rv.capi.ERR_CAPACITY
            seen += 1
            call()
    assert seen >= 1, "2^4 slots per frame cannot have been enough"
    assert ctx.poll_status(wait=False) == rv.capi.OK
    torch.cuda.synchronize(dev)
    same_floats(d_marg.cpu().numpy(), want_marg[:n])
    assert np.array_equal(d_lab.cpu().numpy(), want_lab[:n])


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    capi = rv.capi
    W, H, layers, n = 160, 120, (3, 5), 1
    rgb, depth = X.frames(2, W, H)
    rgb, depth = rgb[:n], depth[:n]
    cal = np.ascontiguousarray(X.calibs(n, W, H))
    dist = X.log_softmax_distributions(23, n, layers, H, W)
    low = X.log_softmax_distributions(23, n, layers, H // 4, W // 4)
    ctx = gpu_ctx_factory(width=W, height=H, stride=4, use_dense_crf=1, dcrf_iterations=3, label_mode=X.LABEL_CRF, unknown_label=(2, 4))
    L, h = ctx.L, ctx.h
    lab = np.empty((n, len(layers), H, W), np.int8)

    def refused(st):
        assert st == capi.ERR_INVALID_ARG, st
        assert L.rvseg_last_error(h), "a message in rvseg_last_error"

    def segment(rgb_=rgb, depth_=depth, cal_=cal, dist_=dist, ds=1):
        p = lambda a: _ptr(a) if a is not None else None
        return L.rvseg_segment_external(h, n, p(rgb_), p(depth_), p(cal_), p(dist_), ds, None, _ptr(lab))

    refused(segment())                                           # no layout set
    refused(L.rvseg_segment_external_device(h, n, None, None, _ptr(cal), None, 1, None, None, None))
    for counts in ((), (1,) * 9, (3, 0, 2), (-1,), (32, 33), (65,)):   # 0 and 9 layers, a zero / negative count, sum 65
        arr = (C.c_int32 * max(1, len(counts)))(*counts)
        refused(L.rvseg_external_layers_set(h, len(counts), arr))
    refused(L.rvseg_external_layers_set(h, 2, None))
    refused(segment())                                           # ... and none of them left a layout behind
    ctx.external_layers_set(layers)
    refused(L.rvseg_external_layers_set(h, 9, (C.c_int32 * 9)(*([1] * 9))))   # a refused call keeps the previous layout
    refused(segment(ds=2))                                       # dist_stride 2 on a stride-4 context
    refused(segment(ds=0))
    for missing in ("rgb_", "depth_", "cal_", "dist_"):
        refused(segment(**{missing: None}))
    refused(L.rvseg_segment_external_device(h, n, None, None, _ptr(cal), None, 1, None, None, None))
    refused(L.rvseg_rectify_depth(h, n, None, _ptr(cal), C.c_float(0.5), C.c_float(15.0), None))
    refused(L.rvseg_rectify_depth(h, -1, _ptr(depth), _ptr(cal), C.c_float(0.5), C.c_float(15.0), None))
    refused(L.rvseg_rectify_depth_device(h, n, None, _ptr(cal), C.c_float(0.5), C.c_float(15.0), None, None))
    # the context still works, at both resolutions
    unknown = (2, 4)
    for d, ds in ((dist, 1), (low, 4)):
        want_marg, want_lab = X.expected(rgb, depth, cal, d, layers, W, H, X.LABEL_CRF, unknown, dist_stride=ds)
        out = ctx.segment_external(rgb, depth, cal, d, dist_stride=ds)
        same_floats(out["marginals"], want_marg)
        assert np.array_equal(out["labels"].reshape(want_lab.shape), want_lab)
    assert L.rvseg_segment_external(h, 0, None, None, None, None, 1, None, None) == capi.OK   # no frames: nothing to do


# ---- facade -------------------------------------------------------------------------------------------------------------------
def test_segmenter_facade_with_a_provider(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    W, H, n = 160, 120, 2
    rgb, depth = X.frames(n, W, H)
    cal = X.calibs(n, W, H)
    layers = [{"name": "structure", "classes": [("floor", (0, 0, 255)), ("wall", (0, 255, 0)), ("ceiling", (255, 0, 0))]}]
    seg = rv.Segmenter(forest=None, layers=layers, external_semantics=True, width=W, height=H, use_dense_crf=1, dcrf_iterations=3,
                       label_mode=X.LABEL_CRF, unknown_label=(1,))
    try:
        req = seg.externalRequest(rgb, depth, cal)
        assert req["rgb"].dtype == np.uint8 and req["rgb"].shape == (n, H, W, 3)
        same_floats(req["depth"], X.expected_xyz(depth, cal, W, H, 0.5, 15.0))
        dist = X.height_provider(req)
        want_marg, want_lab = X.expected(rgb, depth, cal, dist, X.HEIGHT_LAYERS, W, H, X.LABEL_CRF, (1,))
        out = seg.processFrames(rgb, depth, cal, provider=X.height_provider)
        assert np.array_equal(out["labels"].reshape(want_lab.shape), want_lab)
        same_floats(out["marginals"], want_marg)
        assert set(np.unique(out["labels"]).tolist()) == {0, 1, 2}
        again = seg.processFrames(rgb, depth, cal, label_distribution=dist)
        assert again["labels"].tobytes() == out["labels"].tobytes()
        assert seg.srvSegmentationInformation()["class_counts"] == [3]

        def broken(request):
            raise ValueError("the network is down")

        with pytest.raises(RuntimeError, match="Calling the segmentation service failed"):
            seg.processFrames(rgb, depth, cal, provider=broken)
        assert seg.processFrames(rgb, depth, cal, label_distribution=dist)["labels"].tobytes() == out["labels"].tobytes()
    finally:
        seg.close()
    with pytest.raises(RuntimeError):
        rv.Segmenter(forest=None, width=W, height=H)     # no forest and no external semantics
