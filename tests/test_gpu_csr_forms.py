"""The counting-sort CSR build (csrc/kernels_lattice.hip: count, total, scan, scatter) in both of its id forms, against
the CPU oracle bit for bit.  The CSR order is the splat's summation order, so an entry ranked or placed wrongly changes
bits of the filter output; every comparison here is exact.

Cloud form (32-bit global ids, one frame): every dimension d = 1 .. 7, i.e. every instantiation of the scatter, with
N = 4003 points: N is odd; N (d+1) mod 4 = 2, 1, 0, 3, 2, 1, 0 for d = 1 .. 7, so the count pass's last 4-wide unit holds
1, 2, 3 or 4 entries; and at the default wave-block of 256 points the last of the 16 wave-blocks holds 163 points.  With
csr_block = 4096 (d = 3, and d = 6 at the narrower spread below) the cloud is a single wave-block shorter than the block
size.

The counting-sort path holds at most CS_MCAP = 4096 vertices per frame (2^13 slots).  Features spread over 4 units give
7, 40, 204, 859 and 3 131 vertices for d = 1 .. 5 but 9 300 and 20 003 for d = 6 and 7: those two clouds overflow 2^13
slots and are rebuilt on the radix-sort path, which is what their cases then assert (the expected path follows from the
oracle's vertex count, as in test_gpu_lattice_limits.py).  So that the d = 6 and d = 7 scatters run as well, both
dimensions also come with a narrower spread (3.0: 3 767 vertices, 2.2: 3 434) that stays on the counting-sort path.

Frame form (16-bit frame-local ids): the 3-frame 33 x 21 case of test_gpu_narrow_ids.py at csr_block = 1024: each
693-point frame is one wave-block of 4 851 entries, not a multiple of 8, so both its first and its last 16-byte unit of
the id array are shared with the neighbouring frame.
"""
import numpy as np
import pytest

from rovinasemanticsegmentation_amd import synthetic
from test_gpu_narrow_ids import SMALL_KW, ITERS, _check, _forest, _want

pytestmark = pytest.mark.gpu

CS_MCAP = 4096
N = 4003
_clouds = {}


def _cloud(oracle, d, spread):
    """Features, oracle lattice, and the oracle's filter and 2-iteration CRF of the cloud, computed once per (d, spread)."""
    if (d, spread) not in _clouds:
        rng = np.random.default_rng(600 + N)
        F = (rng.random((N, d)) * spread - spread / 3).astype(np.float32)
        V = np.random.default_rng(d).random((N, 3)).astype(np.float32)
        U = (np.random.default_rng(d + 1).random((N, 5)) * 4).astype(np.float32)
        lat = oracle.Lattice(F)
        Q = oracle.crf_inference(U, F, 3.0, 2)
        _clouds[(d, spread)] = (F, V, U, lat, lat.compute(V), Q, oracle.labels(Q, 5, 3))
    return _clouds[(d, spread)]


@pytest.mark.parametrize("d,spread,csr_block", [
    (1, 4.0, 0), (2, 4.0, 0), (3, 4.0, 0), (4, 4.0, 0), (5, 4.0, 0), (6, 4.0, 0), (7, 4.0, 0),
    (6, 3.0, 0), (7, 2.2, 0),
    (3, 4.0, 4096), (6, 3.0, 4096)])
def test_cloud_form_every_dimension(gpu_ctx_factory, oracle, d, spread, csr_block):
    """Structure, a 3-channel filter and a 2-iteration 5-class CRF of a 4003-point cloud at 2^13 slots."""
    F, V, U, lat, want_filter, want_Q, want_labels = _cloud(oracle, d, spread)
    assert (N * (d + 1)) % 4 == (2, 1, 0, 3, 2, 1, 0)[d - 1] and N % 256 == 163
    fits = lat.M <= CS_MCAP
    assert fits == ((d, spread) not in ((6, 4.0), (7, 4.0))), lat.M
    ctx = gpu_ctx_factory(lattice_capacity_log2=13)
    if csr_block:
        ctx.set_schedule(csr_block=csr_block)
    off, bary, keys, M = ctx.lattice_build(F)
    assert ctx.last_schedule()["csr_path"] == (1 if fits else 2), ctx.last_schedule()
    assert off.dtype == np.int32 and off.shape == (N, d + 1)
    assert M == lat.M and 0 <= off.min() and off.max() == M - 1
    assert np.array_equal(bary, lat.barycentric)
    assert np.array_equal(keys[off], lat.keys[lat.offset])
    assert sorted(map(tuple, keys.tolist())) == sorted(map(tuple, lat.keys.tolist()))
    assert np.array_equal(ctx.lattice_filter(V), want_filter)
    Q, mp = ctx.crf_infer(U, F, 3.0, 2)
    assert ctx.last_schedule()["csr_path"] == (1 if fits else 2), ctx.last_schedule()
    assert np.array_equal(Q, want_Q)
    assert np.array_equal(mp, want_labels)


def test_frame_form_one_wave_block_per_frame(gpu_ctx_factory, oracle):
    """3 frames of 33 x 21 with csr_block = 1024: posteriors, marginals and labels of every frame."""
    W, H = 33, 21
    kw = dict(width=W, height=H, dcrf_iterations=ITERS, **SMALL_KW)
    rgb, depth = synthetic.make_batch(3, W, H, holes=True)
    calib = synthetic.make_calib(W, H)
    assert W * H <= 1024 and (W * H * 7) % 8 != 0 and (2 * W * H * 7) % 8 != 0
    blob = _forest(D=30)
    want = _want(oracle, "odd", blob, 1, kw, rgb, depth, calib, [7, 8])
    ctx = gpu_ctx_factory(use_dense_crf=1, multi_layer=1, label_mode=1, unknown_label=[7, 8], max_batch=3,
                          lattice_capacity_log2=13, schedule=dict(csr_block=1024), **kw)
    ctx.forest_load(blob)
    out = ctx.segment_frames(rgb, depth, calib)
    info = ctx.last_schedule()
    assert info["csr_path"] == 1 and info["capacity_log2"] == 13, info
    _check(out, want, "33x21, csr_block 1024")
