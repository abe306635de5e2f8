"""Local-map fusion (csrc/rvseg_fusion.hip: rvseg_fuse_posteriors, rvseg_fuse_posteriors_device, the fusion leg of
rvseg_process_map_device) at its limits, against the oracle BIT FOR BIT (uint32 views):

  cloud sizes    1, 2, 2^k - 1, 2^k, 2^k + 1 for k = 8 and 16: the radix sort's key width (`key_bits`) must also hold the
                 "no point" key, which is cloud_size itself
  layouts        [1], [64], [8] * 8, [64] * 8 (S = 512), [1, 64, 2]
  run lengths    one point hit by every pixel of every image (a chain of 115 200 ordered additions), n = 1 and n = 33
  values         +-inf, NaN, -0.0, denormals, sums that overflow
  indices        -2 and INT_MIN are "no point"; cloud_size and INT_MAX are errors (through poll_status on the device entry)
  many calls     one context, large then small, the layout changing, host and device entries interleaved, a caller stream
"""
import ctypes as C

import numpy as np
import pytest

import fusion_cases as fc

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    g, w = _bits(got), _bits(want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)                       # NaN: the positions, not the payload
    bad = np.flatnonzero((g != w) & ~nan)
    assert bad.size == 0, (bad[:5], np.asarray(got)[bad[:5]], np.asarray(want)[bad[:5]])


def _device_fuse(ctx, idx, post, cc, cloud_size, stream=None):
    """rvseg_fuse_posteriors_device on torch buffers; returns the unaries.  The call only enqueues, on the context's own
    stream or the caller's: the caller polls the status (which waits for the fusion) before reading them."""
    import torch
    import rovinasemanticsegmentation_amd as rv
    dev = torch.device("cuda", 0)
    S = sum(cc)
    d_idx = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(dev)
    d_post = torch.from_numpy(np.ascontiguousarray(post, np.float32)).to(dev)
    d_un = torch.full((max(cloud_size * S, 1),), 123.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ccv = (C.c_int32 * len(cc))(*cc)
    st = ctx.L.rvseg_fuse_posteriors_device(ctx.h, idx.shape[0], C.c_void_p(d_idx.data_ptr()), C.c_void_p(d_post.data_ptr()), len(cc), ccv,
                                            cloud_size, C.c_void_p(d_un.data_ptr()), C.c_void_p(stream) if stream else None)
    assert st == rv.capi.OK
    return d_un


@pytest.mark.parametrize("cloud_size", [1, 2, 255, 256, 257, 65535, 65536, 65537])
def test_cloud_sizes_around_powers_of_two(gpu_ctx_factory, oracle, cloud_size):
    W, H, n, cc = 160, 120, 3, [3, 2]
    ctx = gpu_ctx_factory(width=W, height=H)
    rng = np.random.default_rng(cloud_size)
    idx = fc.sparse_indices(rng, n, W, H, cloud_size)
    assert (idx == -1).mean() > 0.9 and (idx == 0).any() and (idx == cloud_size - 1).any()
    post = fc.wide_values(rng, (n, sum(cc) * W * H))
    want = oracle.fuse_posteriors(idx, post, cc, cloud_size)
    assert np.count_nonzero(want) > 0
    _same(ctx.fuse_posteriors(idx, post, cc, cloud_size), want)
    # every pixel a hit, the last point the busiest
    idx2 = rng.integers(0, cloud_size, (n, H, W)).astype(np.int32)
    idx2[:, ::2, ::3] = cloud_size - 1
    _same(ctx.fuse_posteriors(idx2, post, cc, cloud_size), oracle.fuse_posteriors(idx2, post, cc, cloud_size))


@pytest.mark.parametrize("cc", [[1], [64], [8] * 8, [64] * 8, [1, 64, 2]], ids=lambda cc: "_".join(map(str, cc)))
def test_layouts(gpu_ctx_factory, oracle, cc):
    W, H, n, P = 160, 120, 2, 300
    ctx = gpu_ctx_factory(width=W, height=H)
    rng = np.random.default_rng(len(cc) * 100 + cc[0])
    idx = rng.integers(-1, P, (n, H, W)).astype(np.int32)
    post = fc.wide_values(rng, (n, sum(cc) * W * H))
    _same(ctx.fuse_posteriors(idx, post, cc, P), oracle.fuse_posteriors(idx, post, cc, P))


def test_layouts_beyond_the_limits_are_refused(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    ctx = gpu_ctx_factory(width=160, height=120)
    idx = np.zeros((1, 120, 160), np.int32)
    for cc in ([65], [0], [3, 0], [1] * 9, []):
        with pytest.raises(rv.capi.RvsegError) as e:
            ctx.fuse_posteriors(idx, np.zeros((1, sum(cc) * 160 * 120), np.float32), cc, 4)
        assert e.value.status == rv.capi.ERR_INVALID_ARG, cc


def test_one_point_hit_by_every_pixel_of_every_image(gpu_ctx_factory, oracle):
    """A chain of 6 * 160 * 120 = 115 200 additions per class, walked front to back by one thread (that another order
    gives other bits for this input is pinned in test_oracle_fusion.py)."""
    idx, post, cc, P = fc.chain()
    ctx = gpu_ctx_factory(width=160, height=120)
    want = oracle.fuse_posteriors(idx, post, cc, P)
    _same(ctx.fuse_posteriors(idx, post, cc, P), want)
    assert np.all(want.reshape(P, -1)[[0, 2]] == 0)


@pytest.mark.parametrize("n", [1, 33])
def test_image_counts(gpu_ctx_factory, oracle, n):
    W, H, cc, P = 160, 120, [4, 3], 37
    ctx = gpu_ctx_factory(width=W, height=H)
    rng = np.random.default_rng(n)
    idx = rng.integers(-1, P, (n, H, W)).astype(np.int32)        # about n * 500 hits per point
    post = fc.wide_values(rng, (n, sum(cc) * W * H))
    _same(ctx.fuse_posteriors(idx, post, cc, P), oracle.fuse_posteriors(idx, post, cc, P))


def test_special_values(gpu_ctx_factory, oracle):
    """+-inf, NaN, -0.0, denormals and overflowing sums go through the additions like any float.  A point hit only by
    -0.0 reads +0.0 (the accumulator starts at +0.0); denormals are NOT flushed (a flushed sum would differ below)."""
    W, H, n, cc, P = 160, 120, 3, [3], 40
    ctx = gpu_ctx_factory(width=W, height=H)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 20, (n, H, W)).astype(np.int32)
    post = fc.wide_values(rng, (n, 3 * W * H)).reshape(n, H * W, 3)
    flat = idx.reshape(n, -1)
    tiny = np.float32(1e-45)
    specials = {20: [np.inf], 21: [-np.inf], 22: [np.inf, -np.inf], 23: [np.nan], 24: [-0.0], 25: [-0.0, -0.0, -0.0],
                26: [tiny, tiny, tiny], 27: [3e38, 3e38, -3e38], 28: [-3e38, np.inf, 1.0, -3e38], 29: [1e-39, -2e-39, 3e-40],
                30: [1.17549435e-38, -1e-45], 31: [-0.0, 0.0], 32: [np.inf, np.nan, 1.0]}
    pix = 0
    for point, vals in specials.items():
        for k, v in enumerate(vals):
            flat[k % n, pix] = point
            post[k % n, pix, :] = v
            pix += 1
    post = post.reshape(n, -1)
    want = oracle.fuse_posteriors(idx, post, cc, P).reshape(P, 3)
    got = ctx.fuse_posteriors(idx, post, cc, P)
    _same(got, want.ravel())
    got = got.reshape(P, 3)
    assert np.all(_bits(got[24]) == 0) and np.all(_bits(got[25]) == 0) and np.all(_bits(got[31]) == 0)      # +0.0
    assert np.all(got[26] == np.float32(3) * tiny) and np.all(got[26] != 0)                               # denormal sums survive
    assert np.all(got[29] != 0) and np.all(np.abs(got[29]) < 1.2e-38)
    assert np.all(np.isnan(got[22])) and np.all(np.isnan(got[23])) and np.all(np.isnan(got[32]))
    assert np.all(got[27] == np.inf) and np.all(np.isnan(got[28]))              # 3e38 + 3e38 = inf stays inf; (-3e38 - 3e38) + inf = NaN
    assert np.all(got[20] == np.inf) and np.all(got[21] == -np.inf)
    d_un = _device_fuse(ctx, idx, post, cc, P)
    ctx.poll_status(wait=True)                                      # the library's own stream: wait before reading
    _same(d_un.cpu().numpy(), want.ravel())


def test_negative_indices_are_no_point_and_large_ones_are_errors(gpu_ctx_factory, oracle):
    import rovinasemanticsegmentation_amd as rv
    W, H, n, cc, P = 160, 120, 2, [4], 256
    ctx = gpu_ctx_factory(width=W, height=H)
    rng = np.random.default_rng(9)
    idx = rng.integers(-1, P, (n, H, W)).astype(np.int32)
    idx[0, 0, :8] = [-2, fc.INT_MIN, -3, fc.INT_MIN + 1, -256, -257, -65536, -2 ** 30]
    post = fc.wide_values(rng, (n, 4 * W * H))
    want = oracle.fuse_posteriors(np.where(idx < 0, -1, idx), post, cc, P)
    _same(ctx.fuse_posteriors(idx, post, cc, P), want)                                   # no error either
    d_un = _device_fuse(ctx, idx, post, cc, P)
    assert ctx.poll_status(wait=True) == rv.capi.OK
    _same(d_un.cpu().numpy(), want)
    for bad_value in (P, P + 1, 2 * P, fc.INT_MAX):
        bad = idx.copy()
        bad[1, 5, 5] = bad_value
        bad[0, 9, 0] = bad_value
        skipped = oracle.fuse_posteriors(np.where((bad < 0) | (bad >= P), -1, bad), post, cc, P)
        with pytest.raises(rv.capi.RvsegError) as e:
            ctx.fuse_posteriors(bad, post, cc, P)
        assert e.value.status == rv.capi.ERR_INVALID_ARG, bad_value
        d_un = _device_fuse(ctx, bad, post, cc, P)                                       # the device entry enqueues ...
        with pytest.raises(rv.capi.RvsegError) as e:
            ctx.poll_status(wait=True)                                                   # ... and reports here
        assert e.value.status == rv.capi.ERR_INVALID_ARG, bad_value
        _same(d_un.cpu().numpy(), skipped)                                               # every other hit was added as usual
        assert ctx.poll_status(wait=True) == rv.capi.OK                                  # reported once
    _same(ctx.fuse_posteriors(idx, post, cc, P), want)                                   # and the context goes on


def test_one_context_many_calls_large_then_small(gpu_ctx_factory, oracle):
    """The context's buffers only grow: a small call after a large one runs on buffers that still hold the large
    call's runs (`start`, `end`), keys and unaries.  Layouts [8, 9] -> [3] -> [64], host and device entries interleaved,
    the device entry on a caller's stream."""
    import torch
    import rovinasemanticsegmentation_amd as rv
    W, H = 160, 120
    ctx = gpu_ctx_factory(width=W, height=H)
    rng = np.random.default_rng(21)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    calls = [([8, 9], 5, 70000, "host"), ([3], 1, 7, "device"), ([64], 2, 300, "host"), ([3], 1, 7, "host"), ([8, 9], 5, 70000, "device"),
             ([64], 1, 1, "device"), ([3], 4, 65536, "stream"), ([8, 9], 1, 2, "stream"), ([3], 1, 7, "host")]
    for cc, n, P, how in calls:
        idx = rng.integers(-1, P, (n, H, W)).astype(np.int32)
        idx[0, 0, 0], idx[0, 0, 1] = 0, P - 1
        post = fc.wide_values(rng, (n, sum(cc) * W * H))
        want = oracle.fuse_posteriors(idx, post, cc, P)
        if how == "host":
            got = ctx.fuse_posteriors(idx, post, cc, P)
        else:
            d_un = _device_fuse(ctx, idx, post, cc, P, stream=stream.cuda_stream if how == "stream" else None)
            assert ctx.poll_status(wait=True) == rv.capi.OK
            if how == "stream":
                stream.synchronize()
            got = d_un.cpu().numpy()
        _same(got, want)


def test_process_map_device_without_unaries_without_points_without_images(gpu_ctx_factory, oracle):
    """rvseg_process_map_device: d_unaries_out = NULL (the unaries stay in the context), cloud_size = 0 (nothing is
    written), n_images = 0 (every point unseen: the "Unknown" label of the no-CRF rule)."""
    import torch
    import rovinasemanticsegmentation_amd as rv
    from rovinasemanticsegmentation_amd import synthetic
    dev = torch.device("cuda", 0)
    W, H, n, P = 160, 120, 2, 500
    blob = synthetic.make_forest_bytes(seed=5, n_trees=2, leaves_per_tree=64, max_depth=10)
    ctx = gpu_ctx_factory(width=W, height=H, multi_layer=1, use_dense_crf=0, unknown_label=[7, 8])
    ctx.forest_load(blob)
    cc = ctx.forest_info()["class_counts"]
    S = sum(cc)
    rng = np.random.default_rng(2)
    idx = rng.integers(-1, P, (n, H, W)).astype(np.int32)
    idx[idx == 17] = -1                                            # point 17 is never seen
    post = rng.standard_normal((n, S * W * H)).astype(np.float32)
    d_idx, d_post = torch.from_numpy(idx).to(dev), torch.from_numpy(post).to(dev)
    want_un = oracle.fuse_posteriors(idx, post, cc, P)

    def want_labels(un, size):
        out, off = [], 0
        for l, c in enumerate(cc):
            out.append(oracle.labels(un[off:off + c * size].reshape(size, c), c, 2, [7, 8][l]))
            off += c * size
        return np.stack(out)

    d_lab = torch.full((len(cc), P), -99, dtype=torch.int8, device=dev)
    d_un = torch.empty(P * S, dtype=torch.float32, device=dev)
    ctx.process_map_device(n, d_idx.data_ptr(), d_post.data_ptr(), P, 0, 0, d_lab.data_ptr(), d_un.data_ptr())
    assert ctx.poll_status(wait=True) == rv.capi.OK
    torch.cuda.synchronize(dev)
    _same(d_un.cpu().numpy(), want_un)
    assert np.array_equal(d_lab.cpu().numpy(), want_labels(want_un, P))
    assert np.all(d_lab.cpu().numpy()[:, 17] == [7, 8])
    # without the unaries
    d_lab2 = torch.full((len(cc), P), -99, dtype=torch.int8, device=dev)
    ctx.process_map_device(n, d_idx.data_ptr(), d_post.data_ptr(), P, 0, 0, d_lab2.data_ptr(), 0)
    assert ctx.poll_status(wait=True) == rv.capi.OK
    torch.cuda.synchronize(dev)
    assert torch.equal(d_lab, d_lab2)
    # no points: nothing is touched
    d_lab2.fill_(-99)
    ctx.process_map_device(n, d_idx.data_ptr(), d_post.data_ptr(), 0, 0, 0, d_lab2.data_ptr(), d_un.data_ptr())
    assert ctx.poll_status(wait=True) == rv.capi.OK
    torch.cuda.synchronize(dev)
    assert bool((d_lab2 == -99).all())
    _same(d_un.cpu().numpy(), want_un)
    # no images: zero unaries, every point "Unknown"
    ctx.process_map_device(0, 0, 0, P, 0, 0, d_lab2.data_ptr(), d_un.data_ptr())
    assert ctx.poll_status(wait=True) == rv.capi.OK
    torch.cuda.synchronize(dev)
    assert np.all(_bits(d_un.cpu().numpy()) == 0)
    assert np.array_equal(d_lab2.cpu().numpy(), want_labels(np.zeros(P * S, np.float32), P))
    assert np.all(d_lab2.cpu().numpy() == np.array([[7], [8]]))
    # the host entry with no images and with no points
    _same(ctx.fuse_posteriors(idx[:0], post[:0], cc, P), np.zeros(P * S, np.float32))
    assert ctx.fuse_posteriors(idx, post, cc, 0).size == 0
