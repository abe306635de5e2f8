"""Data recipes for the local-map fusion's limits (plain helper module): shared by the CPU pins in
test_oracle_fusion.py and the GPU comparisons in test_gpu_fusion_limits.py."""
import numpy as np

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def wide_values(rng, shape):
    """Mixed signs over ten decades: sums whose fp32 result depends on the order of the additions."""
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 8, shape)).astype(np.float32)


def chain(n=6, W=160, H=120, cc=(2,), seed=11):
    """Every pixel of every image maps to point 1 of 3: one ordered chain of n * W * H additions per class."""
    rng = np.random.default_rng(seed)
    idx = np.ones((n, H, W), np.int32)
    post = wide_values(rng, (n, sum(cc) * W * H))
    return idx, post, list(cc), 3


def sparse_indices(rng, n, W, H, cloud_size, hits=400):
    """Mostly -1; the hits include points 0 and cloud_size - 1, several pixels on some points, in several images."""
    idx = np.full((n, H, W), -1, np.int32)
    flat = idx.reshape(-1)
    where = rng.choice(flat.size, size=min(hits, flat.size // 2), replace=False)
    flat[where] = rng.integers(0, cloud_size, where.size)
    flat[where[:4]] = [0, cloud_size - 1, 0, cloud_size - 1]
    return idx
