"""CPU pins of the external-semantics recipes (tests/external_cases.py): numpy and the oracle alone show that every
recipe reaches what it claims, so that the GPU comparisons of test_gpu_external.py cannot pass on inputs that miss the
edge they are about.  Plus the new C-ABI symbols and the host-only argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

import external_cases as X
from frame_cases import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECTIFY_SIZES = ((160, 120), (5, 5))

NEW_SYMBOLS = ("rvseg_rectify_depth", "rvseg_rectify_depth_device", "rvseg_external_layers_set", "rvseg_segment_external",
               "rvseg_segment_external_device")


def test_library_exports_the_external_entry_points():
    from rovinasemanticsegmentation_amd import _capi as capi
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
        assert hasattr(L, name), name
    header = open(os.path.join(ROOT, "include", "rvseg.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name


def test_null_context_is_refused_without_a_device():
    """The only argument check that needs no context (and so no GPU): a null context"""
    from rovinasemanticsegmentation_amd import _capi as capi
    L = capi.lib()
    cc = (C.c_int32 * 2)(8, 9)
    assert L.rvseg_external_layers_set(None, 2, cc) == capi.ERR_INVALID_ARG
    assert L.rvseg_rectify_depth(None, 1, None, None, C.c_float(0.5), C.c_float(15.0), None) == capi.ERR_INVALID_ARG
    assert L.rvseg_rectify_depth_device(None, 1, None, None, C.c_float(0.5), C.c_float(15.0), None, None) == capi.ERR_INVALID_ARG
    assert L.rvseg_segment_external(None, 1, None, None, None, None, 1, None, None) == capi.ERR_INVALID_ARG
    assert L.rvseg_segment_external_device(None, 1, None, None, None, None, 1, None, None, None) == capi.ERR_INVALID_ARG


@pytest.mark.parametrize("W,H", RECTIFY_SIZES)
def test_rectify_inputs_lie_on_both_sides_of_every_edge(W, H):
    n = 3
    depth = X.rectify_depths(n, W, H)
    cal = X.calibs(n, W, H)
    for limits, edges, finite in (((0.5, 15.0), X.EDGE_DEPTHS, X.EDGE_FINITE), (X.OWN_LIMITS, X.OWN_EDGE_DEPTHS, X.OWN_EDGE_FINITE)):
        xyz = X.expected_xyz(depth, cal, W, H, *limits)
        nan = np.isnan(xyz)
        assert (nan.all(-1) == nan.any(-1)).all(), "a pixel is NaN in all three channels or in none"
        for d in edges:
            at = depth == d
            assert at.any(), (d, "missing from the recipe")
            assert (~nan[at].any(-1)).all() == finite[d] and nan[at].all(-1).all() == (not finite[d]), d
    # the float rule itself: d = mm / 1000.0f compared against the float limits
    for d, fin in list(X.EDGE_FINITE.items()):
        m = np.float32(d) / np.float32(1000.0)
        assert (not (m < np.float32(0.5) or m > np.float32(15.0))) == fin, d
    # the edges sit where the kernel's paths differ: in the last pixels (the scalar tail when n * W * H % 4 != 0) and
    # in a group of four that crosses the end of row 0
    flat = depth.reshape(n, -1)
    edge_set = set(X.EDGE_DEPTHS + X.OWN_EDGE_DEPTHS)
    assert all(int(v) in edge_set for v in flat[:, -2:].ravel())
    assert all(int(v) in edge_set for v in flat[:, W - 2:W + 2].ravel())
    if (W, H) == (5, 5):
        assert (W * H) % 4 != 0 and (n * W * H) % 4 != 0


def test_calibrations_differ_and_are_not_trivial():
    cal = X.calibs(3, 160, 120)
    for i in range(3):
        assert not np.allclose(cal[i, 9:18].reshape(3, 3), np.eye(3)) and np.abs(cal[i, 18:21]).min() > 0
        for j in range(i):
            assert not np.array_equal(cal[i], cal[j])


def test_height_provider_produces_all_three_classes():
    W, H = 160, 120
    rgb, depth = X.frames(2, W, H)
    cal = X.calibs(2, W, H)
    req = {"rgb": rgb, "depth": X.expected_xyz(depth, cal, W, H, 0.5, 15.0)}
    cls = X.height_classes(req)
    dist = X.height_provider(req).reshape(2, H * W, 3)
    for i in range(2):
        assert set(np.unique(cls[i]).tolist()) == {-1, 0, 1, 2}, "floor, wall, ceiling and pixels without depth"
        known = cls[i].ravel() >= 0
        assert np.array_equal(dist[i].argmax(1)[known], cls[i].ravel()[known])
        assert np.allclose(np.exp(dist[i]).sum(1), 1.0, atol=1e-6)


def test_label_crf_cases_have_unknown_and_known_labels():
    """LABEL_CRF: the best class where its marginal exceeds 2 / C, else "Unknown".  Both outcomes, per layer, with a
    known label that is not the unknown one."""
    W, H, layers = 160, 120, (8, 9)
    rgb, depth = X.frames(3, W, H)
    cal = X.calibs(3, W, H)
    dist = X.log_softmax_distributions(11, 3, layers, H, W)
    marg, lab = X.expected_cached(("full", X.LABEL_CRF), rgb, depth, cal, dist, layers, W, H, X.LABEL_CRF, (7, 8))
    off, N = 0, W * H
    for l, Cn in enumerate(layers):
        best = marg[:, off:off + N * Cn].reshape(3, N, Cn).max(-1)
        conf = best > np.float32(2.0) / np.float32(Cn)
        assert conf.any() and (~conf).any()
        assert (lab[:, l][~conf] == Cn - 1).all()
        assert (lab[:, l][conf] != Cn - 1).any()
        off += N * Cn


@pytest.mark.parametrize("W,H,layers", [(192, 128, (8, 9)), (160, 120, (3, 11))])
def test_low_resolution_recipe_is_not_nearest_neighbour(W, H, layers):
    s = 4
    dist = X.log_softmax_distributions(13, 1, layers, H // s, W // s)
    up = X.upsampled(dist[0], layers, W // s, H // s, W, H)
    nn = X.nearest(dist[0], layers, W // s, H // s, s)
    assert up.shape == nn.shape == (sum(layers) * W * H,)
    assert (bits(up) != bits(nn)).mean() > 0.5
    # an interpolated row is no log-softmax row any more, but lies between its neighbours
    assert up.max() <= dist.max() and up.min() >= dist.min()
