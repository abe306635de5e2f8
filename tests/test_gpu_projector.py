"""GPU: the projector (rvseg_project_cloud[_device], rvseg_process_map_poses_device; src/segmenter.cpp:234-240, 576-578)
against the numpy restatement of its definition (tests/projector_cases.py), BIT FOR BIT: the index images as int32, the
z-buffers as uint32, through both the host and the device entry.  The recipes' own conditions (crowding, ties, the one
pixel) are asserted on the restatement in tests/test_projector_cases_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import projector_cases as PC
from rovinasemanticsegmentation_amd import synthetic
import rovinasemanticsegmentation_amd as rv

pytestmark = pytest.mark.gpu
W, H = PC.W, PC.H
INVALID = rv.capi.ERR_INVALID_ARG


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory(width=W, height=H)


@pytest.fixture(scope="module")
def crowded_want():
    """The crowded cloud under 33 views, computed once: (xyz, Ps, index, zbuffer)"""
    xyz, Ps = PC.crowded(), PC.views(33)
    idx, zb = PC.project(xyz, Ps)
    idx.setflags(write=False)
    zb.setflags(write=False)
    return xyz, Ps, idx, zb


def _device(ctx, Ps, xyz, want_z=True):
    import torch
    dev = torch.device("cuda", 0)
    n = np.asarray(Ps).reshape(-1, 12).shape[0]
    d_xyz = torch.from_numpy(np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)).to(dev)
    d_idx = torch.full((n, H, W), -77, dtype=torch.int32, device=dev)
    d_z = torch.full((n, H, W), -77.0, dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    ctx.project_cloud_device(Ps, d_xyz.shape[0], d_xyz.data_ptr() if d_xyz.shape[0] else 0, d_idx.data_ptr(), d_z.data_ptr() if want_z else 0, s)
    torch.cuda.synchronize(dev)
    return d_idx.cpu().numpy(), d_z.cpu().numpy()


def _check_both(ctx, Ps, xyz, want=None):
    """host and device entry against the restatement; returns the expected (index, zbuffer)"""
    want_idx, want_z = want if want is not None else PC.project(xyz, Ps)
    for idx, z in (ctx.project_cloud(Ps, xyz), _device(ctx, Ps, xyz)):
        assert idx.dtype == np.int32 and z.dtype == np.float32
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(z.view(np.uint32), want_z.view(np.uint32))
    return want_idx, want_z


@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 255, 256, 257, 20000])
def test_cloud_sizes(ctx, crowded_want, n_points):
    xyz, Ps, idx, zb = crowded_want
    # points well inside the first view come first, so that even one point lands
    order = np.argsort(~np.isin(np.arange(xyz.shape[0]), PC.kept(xyz, Ps[0])[0]), kind="stable")
    pts = xyz[order][:n_points]
    want_idx, _ = _check_both(ctx, Ps[:2], pts)
    assert (want_idx[0] >= 0).sum() >= 1


@pytest.mark.parametrize("n_images", [1, 2, 32, 33])
def test_image_counts(ctx, crowded_want, n_images):
    xyz, Ps, idx, zb = crowded_want
    _check_both(ctx, Ps[:n_images], xyz, (idx[:n_images], zb[:n_images]))
    if n_images == 33:
        assert (idx[32] >= 0).sum() >= W * H // 4      # the image behind the launch-group border is a full one


def test_device_entry_without_zbuffer(ctx, crowded_want):
    xyz, Ps, idx, zb = crowded_want
    got, z = _device(ctx, Ps[:2], xyz, want_z=False)
    assert np.array_equal(got, idx[:2]) and np.all(z == -77.0)
    got, z = ctx.project_cloud(Ps[:2], xyz, want_zbuffer=False)
    assert np.array_equal(got, idx[:2]) and z is None


def test_image_that_no_point_reaches(ctx, crowded_want):
    xyz, Ps, _, _ = crowded_want
    away = Ps[:2].copy()
    away[1, 2] = -away[1, 2]                 # the second view looks the other way: every w is negative
    idx, zb = _check_both(ctx, away, xyz)
    assert np.all(idx[1] == -1) and np.all(np.isposinf(zb[1])) and (idx[0] >= 0).any()


def test_no_points_and_no_images(ctx):
    idx, zb = _check_both(ctx, PC.views(2), np.zeros((0, 3), np.float32))
    assert np.all(idx == -1) and np.all(np.isposinf(zb))
    idx, zb = ctx.project_cloud(np.zeros((0, 3, 4), np.float32), PC.crowded()[:10])
    assert idx.shape == (0, H, W)
    _device(ctx, np.zeros((0, 3, 4), np.float32), PC.crowded()[:10])


def test_limits_of_the_keep_rule(ctx):
    xyz, cases = PC.limits()
    idx, zb = _check_both(ctx, PC.PLAIN[None], xyz)
    for name, (k, pixel) in cases.items():
        if pixel is None:
            assert not np.any(idx == k), name
        else:
            assert idx[0][pixel] == k, name
    assert zb[0][3, 10] == PC.DEPTH_MIN and zb[0][3, 14] == PC.DEPTH_MAX
    # every case alone as well: a one-point cloud takes no other path, but nothing can hide behind a neighbour
    for name, (k, pixel) in cases.items():
        got, _ = ctx.project_cloud(PC.PLAIN[None], xyz[k:k + 1], want_zbuffer=False)
        assert (got >= 0).sum() == (pixel is not None), name
        if pixel is not None:
            assert got[0][pixel] == 0, name


def test_depth_ties_lowest_index_wins(ctx):
    xyz = PC.ties()
    idx, _ = _check_both(ctx, PC.PLAIN[None], xyz)
    i, pix, pw = PC.kept(xyz, PC.PLAIN)
    for p in np.unique(pix):
        sel = pix == p
        assert idx[0].ravel()[p] == i[sel][pw[sel] == pw[sel].min()].min()


def test_contention_on_one_pixel(ctx):
    xyz, P = PC.one_pixel()
    idx, zb = _check_both(ctx, P, xyz)
    assert idx[0, H // 2, W // 2] == 123 and zb[0, H // 2, W // 2] == np.float32(0.75) and (idx >= 0).sum() == 1


def test_context_reuse_leaves_no_stale_key(crowded_want):
    xyz, Ps, idx, zb = crowded_want
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    start = rv.capi.debug_live_resources()
    own = rv.Context(width=W, height=H)
    try:
        _check_both(own, Ps, xyz, (idx, zb))                       # 33 images, 20 000 points: two launch groups
        one = xyz[PC.kept(xyz, Ps[0])[0][:1]]
        want = _check_both(own, Ps[:1], one)                       # 1 image, 1 point on the same context
        assert (want[0] >= 0).sum() == 1
        a = own.project_cloud(Ps[:3], xyz)
        b = own.project_cloud(Ps[:3], xyz)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        assert np.array_equal(a[0], idx[:3])
    finally:
        own.close()
    assert rv.capi.debug_live_resources() == start


def _call_device(ctx, n_images, proj, N, xyz, index, z=None):
    return ctx.L.rvseg_project_cloud_device(ctx.h, n_images, proj, N, xyz, index, z, None)


def test_argument_errors_leave_the_context_usable(ctx, crowded_want):
    import torch
    dev = torch.device("cuda", 0)
    xyz, Ps, idx, zb = crowded_want
    P = np.ascontiguousarray(Ps[:1]).reshape(-1)
    pp = P.ctypes.data_as(C.c_void_p)
    d_xyz = torch.from_numpy(xyz).to(dev)
    d_idx = torch.empty((1, H, W), dtype=torch.int32, device=dev)
    x, o = C.c_void_p(d_xyz.data_ptr()), C.c_void_p(d_idx.data_ptr())
    h_idx = np.empty((1, H, W), np.int32)
    hx, ho = xyz.ctypes.data_as(C.c_void_p), h_idx.ctypes.data_as(C.c_void_p)
    L = ctx.L
    assert _call_device(ctx, 1, None, 10, x, o) == INVALID
    assert _call_device(ctx, 1, pp, 10, None, o) == INVALID
    assert _call_device(ctx, 1, pp, 10, x, None) == INVALID
    assert _call_device(ctx, -1, pp, 10, x, o) == INVALID
    assert _call_device(ctx, 1, pp, -1, x, o) == INVALID
    assert L.rvseg_project_cloud_device(None, 1, pp, 10, x, o, None, None) == INVALID
    assert L.rvseg_project_cloud(ctx.h, 1, None, 10, hx, ho, None) == INVALID
    assert L.rvseg_project_cloud(ctx.h, 1, pp, 10, None, ho, None) == INVALID
    assert L.rvseg_project_cloud(ctx.h, 1, pp, 10, hx, None, None) == INVALID
    assert L.rvseg_project_cloud(ctx.h, -1, pp, 10, hx, ho, None) == INVALID
    assert L.rvseg_project_cloud(ctx.h, 1, pp, -1, hx, ho, None) == INVALID
    assert L.rvseg_last_error(ctx.h)
    assert L.rvseg_projection_matrix(None, pp, pp, pp) == INVALID
    # the pixel limit: n_images x W x H must stay below 2^32 - 1 (checked before any memory is touched)
    many = (2 ** 32) // (W * H) + 1
    assert _call_device(ctx, many, pp, 10, x, o) == INVALID
    # depth_min = 0: refused with RVSEG_ERR_INVALID_ARG -- already by rvseg_create, which accepts no depth_min <= 0, so no
    # context with such a range exists for the projector's own check to meet
    with pytest.raises(rv.capi.RvsegError) as e:
        rv.Context(width=W, height=H, depth_min=0.0)
    assert e.value.status == INVALID
    # the process-map entry: no forest, then bad arguments
    lab = C.c_void_p(d_idx.data_ptr())
    assert L.rvseg_process_map_poses_device(ctx.h, 1, pp, x, 10, x, x, lab, None, None, None) == rv.capi.ERR_NO_FOREST
    _check_both(ctx, Ps[:2], xyz, (idx[:2], zb[:2]))               # still usable


@pytest.fixture(scope="module")
def local_map(gpu_ctx_factory):
    """synthetic.make_local_map(3, 160, 120), the frames' posteriors in HBM, the views' matrices, the expected index"""
    import torch
    dev = torch.device("cuda", 0)
    blob = synthetic.make_forest_bytes(seed=5, n_trees=2, leaves_per_tree=64, max_depth=8)
    rgb, depth, calib, xyz, crgb, _ = synthetic.make_local_map(3, W=W, H=H)
    frames = gpu_ctx_factory(width=W, height=H, multi_layer=1, use_dense_crf=0, max_batch=4)
    frames.forest_load(blob)
    cc = frames.forest_info()["class_counts"]
    d_post = torch.empty((3, sum(cc) * W * H), dtype=torch.float32, device=dev)
    d_rgb = torch.from_numpy(rgb).to(dev)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(dev)
    frames.segment_frames_device(3, d_rgb.data_ptr(), d_depth.data_ptr(), calib, d_post.data_ptr(), 0, 0, 0)
    frames.poll_status(wait=True)
    torch.cuda.synchronize(dev)
    Ps = PC.local_map_projections(calib, 3)
    want_idx, _ = PC.project(xyz, Ps)
    return blob, cc, d_post, xyz, crgb, Ps, want_idx


@pytest.mark.parametrize("use_crf", [0, 1])
def test_process_map_poses_device(gpu_ctx_factory, local_map, use_crf):
    import torch
    dev = torch.device("cuda", 0)
    blob, cc, d_post, xyz, crgb, Ps, want_idx = local_map
    P, S = xyz.shape[0], sum(cc)
    assert (want_idx >= 0).sum() >= 1500
    cmap = gpu_ctx_factory(width=W, height=H, multi_layer=1, use_dense_crf=use_crf, dcrf_iterations=3, unknown_label=[7, 8])
    cmap.forest_load(blob)
    d_xyz, d_crgb = torch.from_numpy(xyz).to(dev), torch.from_numpy(crgb).to(dev)
    s = torch.cuda.current_stream(dev).cuda_stream

    def outputs():
        return (torch.full((len(cc), P), -99, dtype=torch.int8, device=dev), torch.full((P * S,), -99.0, dtype=torch.float32, device=dev))

    lab_a, un_a = outputs()
    d_idx = torch.full((3, H, W), -77, dtype=torch.int32, device=dev)
    cmap.process_map_poses_device(Ps, d_post.data_ptr(), P, d_xyz.data_ptr(), d_crgb.data_ptr(), lab_a.data_ptr(), un_a.data_ptr(),
                                  d_idx.data_ptr(), s)
    assert cmap.poll_status(wait=True) == rv.capi.OK
    torch.cuda.synchronize(dev)
    assert "project" in cmap.last_timing() and "fusion" in cmap.last_timing()
    assert np.array_equal(d_idx.cpu().numpy(), want_idx)
    # without d_index_out the index images stay in context memory: the same labels and unaries
    lab_b, un_b = outputs()
    cmap.process_map_poses_device(Ps, d_post.data_ptr(), P, d_xyz.data_ptr(), d_crgb.data_ptr(), lab_b.data_ptr(), un_b.data_ptr(), 0, s)
    # the parent's interface fed with those index images
    lab_c, un_c = outputs()
    d_want = torch.from_numpy(want_idx).to(dev)
    cmap.process_map_device(3, d_want.data_ptr(), d_post.data_ptr(), P, d_xyz.data_ptr(), d_crgb.data_ptr(), lab_c.data_ptr(),
                            un_c.data_ptr(), s)
    assert cmap.poll_status(wait=True) == rv.capi.OK
    torch.cuda.synchronize(dev)
    for lab, un in ((lab_a, un_a), (lab_b, un_b)):
        assert lab.cpu().numpy().tobytes() == lab_c.cpu().numpy().tobytes()
        assert un.cpu().numpy().tobytes() == un_c.cpu().numpy().tobytes()
    assert not np.any(lab_c.cpu().numpy() == -99) and np.any(un_c.cpu().numpy() != 0)


def test_segmenter_process_map_takes_projections(local_map):
    blob, cc, d_post, xyz, crgb, Ps, want_idx = local_map
    post = d_post.cpu().numpy()
    seg = rv.Segmenter(blob, width=W, height=H, multi_layer=1, use_dense_crf=0, unknown_label=[7, 8])
    try:
        lab_p, un_p = seg.processMap(posteriors=post, cloud_xyz=xyz, cloud_rgb=crgb, projections=Ps)
        lab_i, un_i = seg.processMap(want_idx, post, xyz, crgb)
        for a, b in zip(lab_p + un_p, lab_i + un_i):
            assert a.tobytes() == b.tobytes()
        with pytest.raises(RuntimeError):
            seg.processMap(want_idx, post, xyz, crgb, projections=Ps)
        with pytest.raises(RuntimeError):
            seg.processMap(posteriors=post, cloud_xyz=xyz, cloud_rgb=crgb)
    finally:
        seg.close()
