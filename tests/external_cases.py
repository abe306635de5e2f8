"""Data recipes and the expected results of the external-semantics path (csrc/rvseg_external.hip; rvseg_rectify_depth,
rvseg_external_layers_set, rvseg_segment_external) -- a plain helper module like frame_cases.py: the CPU pins
(test_external_cases_cpu.py: numpy and the oracle alone show that a recipe reaches what it claims) and the GPU
comparisons (test_gpu_external.py: GPU == oracle, float32 bit patterns) draw the same bytes from here.

The expected result is composed from the oracle's existing bindings only, the way src/segmenter.cpp composes the
stages: oracle.cloud -> oracle.frame_crf_features -> per layer oracle.crf_inference(-post_l, feat, w, iters) ->
oracle.labels; low-resolution distributions go through oracle.resize_linear per layer first (cv::resize, :380-382).
"""
import functools

import numpy as np

from oracle import oracle as O
from rovinasemanticsegmentation_amd import synthetic

LABEL_EVAL, LABEL_CRF, LABEL_NOCRF, LABEL_ARGMAX = range(4)

# depths (mm) on both sides of the request's limits 0.5 / 15.0 m (segmenter.cpp:472), and the ends of uint16
EDGE_DEPTHS = (0, 499, 500, 501, 14999, 15000, 15001, 65535)
EDGE_FINITE = {0: False, 499: False, 500: True, 501: True, 14999: True, 15000: True, 15001: False, 65535: False}
# a second pair of limits, passed as arguments (they need not be the reference's), with their own edges
OWN_LIMITS = (0.7, 1.3)
OWN_EDGE_DEPTHS = (699, 700, 701, 1299, 1300, 1301)
OWN_EDGE_FINITE = {699: False, 700: True, 701: True, 1299: True, 1300: True, 1301: False}


def calibs(n, W, H):
    """n different calibrations: the stock one turned about the vertical by 0.2 rad per frame and moved -- R is no
    identity and t is not zero in any of them."""
    base = synthetic.make_calib(W, H)
    out = np.empty((n, 21), np.float32)
    for i in range(n):
        a = 0.2 * (i + 1)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        out[i] = base
        out[i, 9:18] = (Rz @ base[9:18].reshape(3, 3).astype(np.float64)).astype(np.float32).ravel()
        out[i, 18:21] = base[18:21] + np.array([0.4 * i - 0.3, 0.25 * (i + 1), 0.1 * i], np.float32)
    return out


def rectify_depths(n, W, H, seed=7):
    """Depth images for rvseg_rectify_depth: a ramp over the whole uint16 range with every edge depth planted at the
    start of each frame, at its end (the last pixels: the scalar tail when W * H is no multiple of four) and across the
    end of the first row (a group of four pixels that straddles a row end)."""
    rng = np.random.default_rng(seed)
    depth = rng.integers(300, 16000, (n, H * W)).astype(np.uint16)
    edges = np.array(EDGE_DEPTHS + OWN_EDGE_DEPTHS, np.uint16)
    k = min(len(edges), H * W // 2)
    for i in range(n):
        e = np.roll(edges, 5 * i)[:k]
        depth[i, :k] = e
        depth[i, H * W - k:] = e[::-1]
        depth[i, W - 2:W - 2 + min(k, 4)] = e[:min(k, 4)]   # the last two pixels of row 0 and the first two of row 1
    return depth.reshape(n, H, W)


def oracle_params(W, H, stride=1, iters=3, depth_min=0.5, depth_max=15.0):
    return O.default_params(width=W, height=H, stride=stride, dcrf_iterations=iters, depth_min=depth_min, depth_max=depth_max)


def expected_xyz(depth, cal, W, H, depth_min, depth_max):
    p = oracle_params(W, H, depth_min=depth_min, depth_max=depth_max)
    return np.stack([O.cloud(p, depth[i], cal[i]) for i in range(depth.shape[0])])


@functools.lru_cache(maxsize=None)
def frames(n, W, H):
    rgb, depth = synthetic.make_batch(n, W, H, holes=True)
    rgb.setflags(write=False)
    depth.setflags(write=False)
    return rgb, depth


@functools.lru_cache(maxsize=None)
def log_softmax_distributions(seed, n, layers, h, w):
    """(n, S * h * w) float32: per frame the layers concatenated, each [y][x][class] -- the wire layout of
    label_distribution; every row the log-softmax of standard normal logits."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        parts = []
        for C in layers:
            lg = rng.normal(size=(h * w, C))
            parts.append((lg - np.log(np.exp(lg).sum(1, keepdims=True))).astype(np.float32).ravel())
        out.append(np.concatenate(parts))
    out = np.stack(out)
    out.setflags(write=False)
    return out


# ---- the provider written for these tests: floor / wall / ceiling by the height of the rectified image -------------------
HEIGHT_LAYERS = (3,)
FLOOR_BELOW, CEILING_ABOVE = 0.0, 1.2      # metres of z in the frame the calibration maps to


def height_provider(request):
    """A SingleFrameSegmentation provider: request = {"rgb": (n, H, W, 3) uint8, "depth": (n, H, W, 3) float32 xyz};
    returns label_distribution (n, 3 * H * W): log-probabilities 0.8 / 0.1 / 0.1 for floor (z < 0), wall, ceiling
    (z > 1.2), uniform where the pixel has no depth (NaN)."""
    z = np.asarray(request["depth"], np.float32)[..., 2]
    n = z.shape[0]
    cls = np.where(z < FLOOR_BELOW, 0, np.where(z > CEILING_ABOVE, 2, 1))
    prob = np.full(z.shape + (3,), 0.1, np.float32)
    np.put_along_axis(prob, cls[..., None], np.float32(0.8), axis=-1)
    prob[np.isnan(z)] = np.float32(1.0 / 3.0)
    return np.log(prob).astype(np.float32).reshape(n, -1)


def height_classes(request):
    z = np.asarray(request["depth"], np.float32)[..., 2]
    return np.where(np.isnan(z), -1, np.where(z < FLOOR_BELOW, 0, np.where(z > CEILING_ABOVE, 2, 1)))


# ---- the expected result --------------------------------------------------------------------------------------------------
def upsampled(dist_i, layers, lw, lh, W, H):
    """One frame's low-resolution distributions -> full resolution, per layer through cv::resize INTER_LINEAR"""
    parts, off = [], 0
    for C in layers:
        low = dist_i[off:off + lw * lh * C].reshape(lh, lw, C)
        parts.append(O.resize_linear(low, W, H).ravel())
        off += lw * lh * C
    return np.concatenate(parts)


def nearest(dist_i, layers, lw, lh, stride):
    """The same by nearest-neighbour replication: what the up-sampler must NOT compute"""
    parts, off = [], 0
    for C in layers:
        low = dist_i[off:off + lw * lh * C].reshape(lh, lw, C)
        parts.append(np.repeat(np.repeat(low, stride, 0), stride, 1).ravel())
        off += lw * lh * C
    return np.concatenate(parts)


def expected(rgb, depth, cal, dist, layers, W, H, label_mode, unknown, crf=True, dist_stride=1, iters=3, weight=10.0):
    """Marginals (n, S * N; None without CRF) and labels (n, L, N) of the external path"""
    n, N = rgb.shape[0], W * H
    p = oracle_params(W, H, iters=iters)
    p.dcrf_kernel_weight = weight
    marg, labels = [], []
    for i in range(n):
        post = dist[i] if dist_stride == 1 else upsampled(dist[i], layers, W // dist_stride, H // dist_stride, W, H)
        feat = O.frame_crf_features(p, rgb[i], O.cloud(p, depth[i], cal[i])) if crf else None
        m, lab, off = [], [], 0
        for l, C in enumerate(layers):
            v = post[off:off + N * C].reshape(N, C)
            if crf:
                v = O.crf_inference(-v, feat, weight, iters)      # unary energy = -value (segmenter.cpp:642)
                m.append(v.ravel())
            lab.append(O.labels(v, C, label_mode, unknown[l]))
            off += N * C
        marg.append(np.concatenate(m) if crf else None)
        labels.append(np.stack(lab))
    return (np.stack(marg) if crf else None), np.stack(labels)


_EXPECTED = {}


def expected_cached(key, *a, **kw):
    """expected() once per key (a reference is computed once and shared among the tests that need it)"""
    if key not in _EXPECTED:
        _EXPECTED[key] = expected(*a, **kw)
    return _EXPECTED[key]
