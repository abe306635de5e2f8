"""bench.py --dump-outputs on CPU tensors laid out as the hot path writes them (include/rvseg.h): marginals per frame
[y][x][class] float32, labels per frame H x W int8.  Every value encodes its own (frame, pixel, class), so a row of
marginals.npy must hold exactly the classes of the pixel named in pixel_index.npy, and labels.npy the same pixel."""
import os

import numpy as np


def test_dump_outputs_rows_are_the_pixels_of_pixel_index(tmp_path):
    import torch
    import bench
    n, N, C = 3, bench.W * bench.H, bench.C_CLASSES
    flat = torch.arange(n * N, dtype=torch.int64)                        # frame * N + pixel
    marg = (flat.view(n, N, 1) * 16 + torch.arange(C).view(1, 1, C)).to(torch.float32).view(n, N * C)
    assert float(marg.max()) < 2 ** 24                                   # every code exact in float32
    labels = (flat.view(n, N) % 127).to(torch.int8)
    fused = ((flat.view(n, N) * 3) % 127).to(torch.int8)
    bench.dump_outputs(str(tmp_path / "a"), n, marg, labels, fused)
    bench.dump_outputs(str(tmp_path / "b"), n, marg, labels, fused)

    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["fused_labels.npy", "labels.npy", "marginals.npy", "pixel_index.npy"]
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    for f in files:                                                      # seeded: the same sample every run
        assert np.array_equal(got[f[:-4]], np.load(tmp_path / "b" / f)), f

    idx = got["pixel_index"]
    k = min(bench.DUMP_PIXELS, n * N)
    assert idx.shape == (k,) and np.array_equal(idx, np.floor(idx)) and idx.min() >= 0 and idx.max() < n * N
    assert np.all(np.diff(idx) > 0)
    assert np.unique(idx.astype(np.int64) // N).size == n               # the sample spans every frame
    ii = idx.astype(np.int64)
    assert got["marginals"].shape == (k, C)
    assert np.array_equal(got["marginals"], (ii[:, None] * 16 + np.arange(C)[None, :]).astype(np.float32))
    assert np.array_equal(got["labels"], (ii % 127).astype(np.float32))
    assert np.array_equal(got["fused_labels"], ((ii * 3) % 127).astype(np.float32))
