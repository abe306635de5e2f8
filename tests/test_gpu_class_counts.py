"""The DenseCRF and the frame path at every class count and layer count, against the CPU oracle bit for bit (after the
1e-4 marginal bar, so that a failure says how far off it was).

Most kernels of the frame path pick their code by the class count C of a label layer, and the layer loop picks scratch
buffers and streams by the layer index.  Coverage of each switch, and the test that reaches each side of it:

  launch_upsample_pack        tiled kernel (C = 8 / 9, W % 64 = 0, H % 4 = 0): test_frame_path_every_layer_layout at
  (kernels_rf.hip)            192 x 128 with (8, 9, 8, 9) and (2, .., 9), beside the per-C kernel of the other layers.
                              upsample_pack_kernel<C> for C = 2-10, 12, 16: the same test, both shapes (160 x 120 is
                              never tiled).  Generic kernel: C = 1, 21, 22 there, 11 and 17 in
                              test_layer_schedules_agree.
  launch_softmax_unary,       fused C (2-10, 12, 16, 21) with DP1 = 7 (d = 6) and runtime d (d = 5), and unfused C (1,
  launch_mf_update            11, 13-15, 17, 20, 24, 25, 32, 33, 48, 64): test_crf_infer_every_class_count.  In the
  (kernels_meanfield.hip)     frame path: every C of the layouts of test_frame_path_every_layer_layout, the fused (21)
                              and unfused (22) layer side by side in (21, 22).
  seq = C <= 2                double-precision blur and sequential slice: C = 1, 2 in test_crf_infer_every_class_count,
                              (2,), (1, 9), (2, .., 9) and single 2 in the frame path, (2,) and (1, 9) in the cloud path.
  splat_group_pass            the classes of a pass (16 at most) by bucket, FULL where n fills it: n = 1, 2, 3 and 4 (FULL),
  (kernels_splat.hip)         5-7 and 8 (FULL, 24 = 16 + 8), 9 (FULL, 25 = 16 + 9), 10-15 and 16 (FULL); 2, 3 and 4 passes
                              (C = 17-32, 33-48, 64), fused (mode 0) and unfused (mode 1) counts:
                              test_crf_infer_every_class_count; crf_infer_multi (mode 1 for every C):
                              test_crf_infer_multi_class_counts.
  MF_LDS_BYTES = 24 KB        one launch with a frame on each side of the update's edge for C = 4, 12, 16 and 21:
                              test_lds_edges_per_class_count (bands lds_c4, lds_c12, lds_c16, mf_lds_c21).
  BLUR_LDS_FLOATS = 6 144     one launch with a frame on each side of Mf x C = 6 144 for C = 4, 12, 16 (the same bands:
                              the two edges coincide) and 21 (blur_lds_c21).
  layer scheduling            1-8 layers, default (two streams, slot = l & 1, layer_enqueue_order) and overlap_layers = 0:
  (rvseg_crf.hip)             test_frame_path_every_layer_layout, test_layer_schedules_agree; fused and unfused layers
                              mixed (csr_nrm_before_fork, launch_labels_frames fall-back) in (21, 22), (1, 9) and the
                              5-layer layout.  64 classes over 4 layers and 44 over 8.  Per-slot scratch sized by an
                              earlier, smaller layout: test_one_context_across_forest_layouts.
  crf_cloud_layers            test_cloud_path_every_layer_layout: (2,), (5, 12, 21), (1, 9), CRF on and off, through
                              rvseg_process_map_device and Segmenter.processMap.
  limits (64 classes,         test_refused_forests_leave_no_model (and the host-only check in test_capi_cpu.py).
  8 layers)
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import rovinasemanticsegmentation_amd as rv
from rovinasemanticsegmentation_amd import synthetic
from test_oracle_crf import LDS_BANDS, band_params, lds_edges

pytestmark = pytest.mark.gpu

TOL = 1e-4
_POOL = max(1, min(os.cpu_count() or 1, 16))
# kernels_meanfield.hip: mf_fused_supported -- class counts with a fused softmax_unary / mf_update instantiation
FUSED = frozenset([2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 21])


@pytest.fixture(scope="module")
def hip_runtime():
    """torch (if present) is imported before librvseg so both share one HIP runtime (conftest.gpu_ctx_factory does the
    same); the tests here open and close their contexts themselves."""
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def _assert_marginals(got, want, what):
    err = float(np.abs(got - want).max()) if got.size else 0.0
    assert err <= TOL, (what, err)
    assert np.array_equal(got, want), (what, err)


def _unknown(l, C):
    """Each layer's own unknown label: never C - 1 (where C > 1), different between neighbouring layers."""
    return (5 * l + 1) % (C - 1) if C > 1 else 0


# ---- 1. crf_infer and crf_infer_multi at every class count --------------------------------------------------------------
CRF_CLASSES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 20, 21, 24, 25, 32, 33, 48, 64]


def _crf_case(C, d, N=3001):
    rng = np.random.default_rng(1000 + 7 * C + d)
    F = (rng.random((N, d)) * 3.0 - 1.0).astype(np.float32)
    U = (rng.random((N, C)) * 3.0).astype(np.float32)
    U[::3] *= np.float32(0.02)          # near-flat rows: marginals below 2 / C, the unknown label of LABEL_CRF
    return U, F


@pytest.mark.parametrize("d", [6, 5])
@pytest.mark.parametrize("C", CRF_CLASSES)
def test_crf_infer_every_class_count(gpu_ctx_factory, oracle, C, d):
    """rvseg_crf_infer over a random cloud: fused class counts with d = 6 (DP1 = 7) and runtime d = 5, unfused ones, the
    C <= 2 sequential path and up to four 16-class splat passes.  Every label rule, with an unknown label that is not
    C - 1."""
    U, F = _crf_case(C, d)
    want = oracle.crf_inference(U, F, 1.0, 3)
    unknown = C // 2 if C > 2 else C + 3
    ctx = gpu_ctx_factory()
    for mode in (rv.capi.LABEL_EVAL, rv.capi.LABEL_CRF, rv.capi.LABEL_NOCRF, rv.capi.LABEL_ARGMAX):
        Q, mp = ctx.crf_infer(U, F, 1.0, 3, label_mode=mode, unknown_label=unknown)
        _assert_marginals(Q, want, (C, d, mode))
        wl = oracle.labels(want, C, mode, unknown)
        assert np.array_equal(mp, wl), (C, d, mode)
        if mode == rv.capi.LABEL_CRF:
            assert (wl == unknown).any() and (C <= 2 or (wl != unknown).any()), C


@pytest.mark.parametrize("C", [2, 5, 16, 33])
def test_crf_infer_multi_class_counts(gpu_ctx_factory, oracle, C):
    """rvseg_crf_infer_multi with a Gaussian (d = 2) and a bilateral (d = 5) kernel: the unfused loop, one filter per
    kernel into the same energy."""
    W, H = 48, 40
    rng = np.random.default_rng(50 + C)
    im = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    im[:, : W // 2] //= 4
    g = rv.capi.crf_features_gaussian(W, H, 3.0, 3.0)
    b = rv.capi.crf_features_bilateral(W, H, 20.0, 20.0, 13.0, 13.0, 13.0, im)
    U = (rng.random((W * H, C)) * 3.0).astype(np.float32)
    U[::4] *= np.float32(0.02)
    want = oracle.crf_inference_multi(U, [g, b], [3.0, 10.0], 3)
    ctx = gpu_ctx_factory()
    for mode in (rv.capi.LABEL_CRF, rv.capi.LABEL_ARGMAX):
        Q, mp = ctx.crf_infer_multi(U, [g, b], [3.0, 10.0], 3, label_mode=mode, unknown_label=C // 2)
        _assert_marginals(Q, want, (C, mode))
        assert np.array_equal(mp, oracle.labels(want, C, mode, C // 2)), (C, mode)


# ---- 2. the frame path at every layer layout ----------------------------------------------------------------------------
# (multi_layer, classes): classes is the layer_classes of a multi-layer forest, or (single_classes,)
LAYOUTS = [(1, (2,)), (1, (1, 9)), (1, (3, 5)), (1, (4, 6, 7)), (1, (10, 12)), (1, (16,)), (1, (21,)), (1, (21, 22)),
           (1, (8, 9, 8, 9)), (1, (2, 3, 4, 5, 6, 7, 8, 9)), (1, (16, 16, 16, 16)), (0, (2,)), (0, (12,)), (0, (21,))]
SHAPES = [(192, 128), (160, 120)]    # the tiled up-sampler takes the first (W % 64 = 0, H % 4 = 0), not the second
N_FRAMES, MAX_BATCH = 5, 2           # chunks of 2, 2 and 1 frames
_forests = {}
_oracle_cache = {}


def _forest(multi, classes):
    key = (multi, classes)
    if key not in _forests:
        seed = 60 + sum(classes) + 7 * len(classes) + 3 * multi
        if multi:
            _forests[key] = synthetic.make_forest_bytes(seed=seed, n_trees=3, leaves_per_tree=128, max_depth=10,
                                                        single_classes=0, layer_classes=tuple(classes))
        else:
            _forests[key] = synthetic.make_forest_bytes(seed=seed, n_trees=3, leaves_per_tree=128, max_depth=10,
                                                        single_classes=classes[0], layer_classes=None)
    return _forests[key]


def _oracle_frames(oracle, blob, multi, kw, rgb, depth, calib, label_mode, unknown):
    """Oracle (posteriors, marginals, labels) of every frame, cached across the tests of the module."""
    key = (blob, multi, tuple(sorted(kw.items())), rgb.shape, label_mode, tuple(unknown))
    if key not in _oracle_cache:
        forest = oracle.Forest(blob)
        p = oracle.default_params(**kw)

        def one(i):
            return oracle.segment_frame(p, forest, multi, rgb[i], depth[i], calib, label_mode=label_mode, unknown=unknown)

        with ThreadPoolExecutor(_POOL) as ex:
            _oracle_cache[key] = list(ex.map(one, range(rgb.shape[0])))
    return _oracle_cache[key]


def _check_frames(out, want, posteriors=True, marginals=True, what=""):
    for i, (post, marg, lab) in enumerate(want):
        if posteriors:
            assert np.array_equal(out["posteriors"][i], post), (what, i)
        if marginals:
            _assert_marginals(out["marginals"][i], marg, (what, i))
        assert np.array_equal(out["labels"][i].ravel(), lab), (what, i)


def _segment(blob, multi, classes, W, H, label_mode, schedule=None, max_batch=MAX_BATCH, **call):
    unknown = [_unknown(l, c) for l, c in enumerate(classes)]
    with rv.Context(schedule=schedule, width=W, height=H, use_dense_crf=1, dcrf_iterations=2, multi_layer=multi,
                    label_mode=label_mode, unknown_label=unknown, max_batch=max_batch) as ctx:
        ctx.forest_load(blob)
        rgb, depth = synthetic.make_batch(N_FRAMES, W, H, holes=True)
        out = ctx.segment_frames(rgb, depth, synthetic.make_calib(W, H), **call)
        return out, ctx.last_timing(), unknown


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("multi,classes", LAYOUTS)
def test_frame_path_every_layer_layout(hip_runtime, oracle, multi, classes, W, H):
    """segment_frames with the DenseCRF for forests of 1 - 8 layers and 1 - 64 classes, 5 frames in chunks of 2, 2 and
    1, under every label rule; each layer has its own unknown label.  Then one labels-only call (the marginals
    stay in the context's scratch buffer)."""
    blob = _forest(multi, classes)
    rgb, depth = synthetic.make_batch(N_FRAMES, W, H, holes=True)
    calib = synthetic.make_calib(W, H)
    kw = dict(width=W, height=H, dcrf_iterations=2)
    for mode in (rv.capi.LABEL_CRF, rv.capi.LABEL_NOCRF, rv.capi.LABEL_EVAL, rv.capi.LABEL_ARGMAX):
        out, _, unknown = _segment(blob, multi, classes, W, H, mode)
        assert out["class_counts"] == list(classes)
        want = _oracle_frames(oracle, blob, multi, kw, rgb, depth, calib, mode, unknown)
        _check_frames(out, want, what=(classes, mode))
        if mode == rv.capi.LABEL_CRF:
            only, _, _ = _segment(blob, multi, classes, W, H, mode, want_posteriors=False, want_marginals=False)
            assert only["posteriors"] is None and only["marginals"] is None
            _check_frames(only, want, posteriors=False, marginals=False, what=(classes, "labels only"))


# ---- 3. the LDS edges of the update and the blur per class count --------------------------------------------------------
@pytest.mark.parametrize("band", sorted(LDS_BANDS))
def test_lds_edges_per_class_count(hip_runtime, oracle, band):
    """One launch with a frame on each side of the update's MF_LDS_BYTES edge and / or the blur's BLUR_LDS_FLOATS edge
    of a class count (bands of synthetic.LATTICE_BANDS, pinned by test_oracle_crf.py), a single-layer C-class forest."""
    C, which = LDS_BANDS[band]
    scene, _, W, H, frames = synthetic.lattice_band(band)
    kw = dict(band_params(oracle, band), dcrf_iterations=2)
    rgb = np.empty((len(frames), H, W, 3), np.uint8)
    depth = np.empty((len(frames), H, W), np.uint16)
    for k, i in enumerate(frames):
        rgb[k], depth[k] = synthetic.make_frame(i, W, H, holes=True, scene=scene)
    calib = synthetic.make_calib(W, H)
    p = oracle.default_params(**kw)
    counts = [oracle.Lattice(oracle.frame_crf_features(p, rgb[k], oracle.cloud(p, depth[k], calib))).M for k in range(len(frames))]
    mf, blur = lds_edges(C)
    for e in {"both": (mf, blur), "update": (mf,), "blur": (blur,)}[which]:
        assert counts[0] <= e < counts[1], (band, counts, e)
    blob = _forest(0, (C,))
    unknown = [_unknown(0, C)]
    want = _oracle_frames(oracle, blob, 0, kw, rgb, depth, calib, rv.capi.LABEL_CRF, unknown)
    with rv.Context(use_dense_crf=1, multi_layer=0, label_mode=rv.capi.LABEL_CRF, unknown_label=unknown,
                    max_batch=len(frames), **kw) as ctx:
        ctx.forest_load(blob)
        out = ctx.segment_frames(rgb, depth, calib)
        info = ctx.last_schedule()
    assert info["n_frames"] == len(frames) and info["vertices"] == sum(counts), info
    _check_frames(out, want, what=band)


# ---- 4. layer scheduling and context reuse ------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [(4, 6, 7), (3, 11, 6, 17, 2), (2, 3, 4, 5, 6, 7, 8, 9)])
def test_layer_schedules_agree(hip_runtime, oracle, classes):
    """3, 5 and 8 layers with the layers on two streams (default) and on one (overlap_layers = 0): identical outputs,
    equal to the oracle's.  On one stream every layer records its stages: the fused update (mf_update) runs iff some layer
    has a fused instantiation, the unfused slice and the labels fall-back iff some layer has none."""
    W, H = 160, 120
    blob = _forest(1, classes)
    rgb, depth = synthetic.make_batch(N_FRAMES, W, H, holes=True)
    calib = synthetic.make_calib(W, H)
    mode = rv.capi.LABEL_CRF
    two, _, unknown = _segment(blob, 1, classes, W, H, mode)
    one, names, _ = _segment(blob, 1, classes, W, H, mode, schedule=dict(overlap_layers=0))
    for k in ("posteriors", "marginals", "labels"):
        assert np.array_equal(one[k], two[k]), k
    want = _oracle_frames(oracle, blob, 1, dict(width=W, height=H, dcrf_iterations=2), rgb, depth, calib, mode, unknown)
    _check_frames(one, want, what=classes)
    fused = [c in FUSED for c in classes]
    assert ("mf_update" in names) == any(fused), (classes, sorted(names))
    assert ("slice" in names) == (not all(fused)), (classes, sorted(names))
    assert ("labels" in names) == (not all(fused)), (classes, sorted(names))


def test_one_context_across_forest_layouts(hip_runtime, oracle):
    """One context loads (2, 3), then (21, 22, 16), then (2, 3) again and segments after each load: its scratch (per-slot
    buffers, the marginals of a labels-only call, lattice tables) was sized by an earlier layout.  Each result equals a
    fresh context's and the oracle's."""
    W, H = 160, 120
    unknown = [0, 1, 11]
    kw = dict(width=W, height=H, use_dense_crf=1, dcrf_iterations=2, multi_layer=1, label_mode=rv.capi.LABEL_CRF,
              unknown_label=unknown, max_batch=MAX_BATCH)
    rgb, depth = synthetic.make_batch(N_FRAMES, W, H, holes=True)
    calib = synthetic.make_calib(W, H)
    with rv.Context(**kw) as ctx:
        for classes in ((2, 3), (21, 22, 16), (2, 3)):
            blob = _forest(1, classes)
            ctx.forest_load(blob)
            only = ctx.segment_frames(rgb, depth, calib, want_posteriors=False, want_marginals=False)
            out = ctx.segment_frames(rgb, depth, calib)
            with rv.Context(**kw) as fresh:
                fresh.forest_load(blob)
                ref = fresh.segment_frames(rgb, depth, calib)
            for k in ("posteriors", "marginals", "labels"):
                assert np.array_equal(out[k], ref[k]), (classes, k)
            assert np.array_equal(only["labels"], ref["labels"]), classes
            want = _oracle_frames(oracle, blob, 1, dict(width=W, height=H, dcrf_iterations=2), rgb, depth, calib,
                                  rv.capi.LABEL_CRF, unknown[:len(classes)])
            _check_frames(out, want, what=classes)


# ---- 5. the cloud path --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [(2,), (5, 12, 21), (1, 9)])
def test_cloud_path_every_layer_layout(hip_runtime, oracle, classes):
    """processMap for forests of 1 - 3 layers (seq, fused and unfused class counts), CRF on and off: through
    Segmenter.processMap (one crf_infer per layer) and rvseg_process_map_device (one cloud lattice for every layer, the
    layers on two streams), against oracle.fuse_posteriors + crf_inference + labels."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    W, H, n = 160, 120, 3
    blob = _forest(1, classes)
    rgb, depth, calib, xyz, crgb, idx = synthetic.make_local_map(n, W, H, step=2)
    P = xyz.shape[0]
    unknown = [_unknown(l, c) for l, c in enumerate(classes)]
    with rv.Context(width=W, height=H, multi_layer=1, use_dense_crf=0, max_batch=n) as fctx:
        fctx.forest_load(blob)
        post = fctx.segment_frames(rgb, depth, calib, want_labels=False)["posteriors"]
    want_un = oracle.fuse_posteriors(idx, post, list(classes), P)
    pairwise = np.concatenate([xyz * np.float32(0.5), crgb * np.float32(4.0)], 1)
    S = sum(classes)
    for use_crf in (0, 1):
        wl = []
        off = 0
        for l, c in enumerate(classes):
            U = want_un[off:off + c * P].reshape(P, c)
            off += c * P
            if use_crf:
                wl.append(oracle.labels(oracle.crf_inference(-U, pairwise, 10.0, 3), c, 1, unknown[l]))
            else:
                wl.append(oracle.labels(U, c, 2, unknown[l]))
        params = dict(width=W, height=H, multi_layer=1, use_dense_crf=use_crf, dcrf_iterations=3, unknown_label=unknown)
        seg = rv.Segmenter(blob, **params)
        try:
            labels, unaries = seg.processMap(idx, post, xyz, crgb)
        finally:
            seg.close()
        assert np.array_equal(np.concatenate([u.ravel() for u in unaries]), want_un), use_crf
        for l in range(len(classes)):
            assert np.array_equal(labels[l], wl[l].astype(np.uint8)), (classes, use_crf, l)
        with rv.Context(**params) as cmap:
            cmap.forest_load(blob)
            d_idx = torch.from_numpy(idx).to(dev)
            d_post = torch.from_numpy(post).to(dev)
            d_xyz = torch.from_numpy(xyz).to(dev)
            d_crgb = torch.from_numpy(crgb).to(dev)
            d_lab = torch.full((len(classes), P), -99, dtype=torch.int8, device=dev)
            d_un = torch.empty(P * S, dtype=torch.float32, device=dev)
            s = torch.cuda.current_stream(dev).cuda_stream
            cmap.process_map_device(n, d_idx.data_ptr(), d_post.data_ptr(), P, d_xyz.data_ptr(), d_crgb.data_ptr(),
                                    d_lab.data_ptr(), d_un.data_ptr(), s)
            assert cmap.poll_status(wait=True) == rv.capi.OK
            torch.cuda.synchronize(dev)
            assert np.array_equal(d_un.cpu().numpy(), want_un), use_crf
            lab = d_lab.cpu().numpy()
        for l in range(len(classes)):
            assert np.array_equal(lab[l], wl[l]), (classes, use_crf, l, "device")


# ---- 6. refusals at the limits ------------------------------------------------------------------------------------------
def refused_forests():
    """Forests past the limits of a context (64 classes over all layers, 8 layers): (multi_layer, bytes, what)."""
    return [(1, synthetic.make_forest_bytes(seed=71, n_trees=2, leaves_per_tree=16, max_depth=6, single_classes=0,
                                            layer_classes=(16, 16, 16, 17)), "65 classes over 4 layers"),
            (1, synthetic.make_forest_bytes(seed=72, n_trees=2, leaves_per_tree=16, max_depth=6, single_classes=0,
                                            layer_classes=(2,) * 9), "9 layers"),
            (0, synthetic.make_forest_bytes(seed=73, n_trees=2, leaves_per_tree=16, max_depth=6, single_classes=65,
                                            layer_classes=None), "65 single-layer classes")]


def test_refused_forests_leave_no_model(hip_runtime, oracle, tmp_path):
    """A forest past the limits is refused with ERR_FORMAT, and the context is left with no model: segment_frames,
    forest_write, forest_info and processMap (device and Segmenter) raise ERR_NO_FOREST.  A valid load afterwards gives
    bit-exact outputs again."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    W, H = 160, 120
    rgb, depth = synthetic.make_batch(3, W, H, holes=True)
    calib = synthetic.make_calib(W, H)
    d_idx = torch.full((1, H, W), -1, dtype=torch.int32, device=dev)
    d_post = torch.zeros((1, 64 * W * H), dtype=torch.float32, device=dev)
    d_xyz = torch.zeros((4, 3), dtype=torch.float32, device=dev)
    d_lab = torch.zeros((8, 4), dtype=torch.int8, device=dev)
    kw = dict(width=W, height=H, dcrf_iterations=2)
    for multi, bad, what in refused_forests():
        classes = (3, 5) if multi else (12,)
        good = _forest(multi, classes)
        unknown = [_unknown(l, c) for l, c in enumerate(classes)]
        params = dict(use_dense_crf=1, multi_layer=multi, label_mode=rv.capi.LABEL_CRF, unknown_label=unknown,
                      max_batch=2, **kw)
        want = _oracle_frames(oracle, good, multi, kw, rgb, depth, calib, rv.capi.LABEL_CRF, unknown)
        seg = rv.Segmenter(good, **params)
        try:
            ctx = seg.ctx
            _check_frames(ctx.segment_frames(rgb, depth, calib), want, what=(what, "before"))
            with pytest.raises(rv.capi.RvsegError) as e:
                ctx.forest_load(bad)
            assert e.value.status == rv.capi.ERR_FORMAT, what
            for call in (lambda: ctx.segment_frames(rgb, depth, calib),
                         lambda: ctx.forest_write(),
                         lambda: ctx.forest_write(str(tmp_path / "f.dat")),
                         lambda: ctx.forest_info(),
                         lambda: ctx.process_map_device(1, d_idx.data_ptr(), d_post.data_ptr(), 4, d_xyz.data_ptr(),
                                                        d_xyz.data_ptr(), d_lab.data_ptr(), 0, 0),
                         lambda: seg.processMap(np.full((1, H, W), -1, np.int32), np.zeros((1, sum(classes) * W * H), np.float32),
                                                np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32))):
                with pytest.raises(rv.capi.RvsegError) as e:
                    call()
                assert e.value.status == rv.capi.ERR_NO_FOREST, what
            assert not os.path.exists(tmp_path / "f.dat")
            ctx.forest_load(good)
            _check_frames(ctx.segment_frames(rgb, depth, calib), want, what=(what, "after"))
            assert ctx.forest_write() == rv.capi.forest_rewrite(good)
        finally:
            seg.close()
