"""The recipes of the boosted-forest tests (tests/test_gpu_boosted.py, tests/test_gpu_boosted_resample.py).  What each one
claims -- a round with 0 < error < 1, a negative alpha, a stop, a draw that needs the clamp -- is pinned from the
restatement alone in tests/test_boost_cases_cpu.py, so the GPU tests compare bytes on cases known to reach those paths."""
import numpy as np

F32 = np.float32


def _features(rng, N, D, kind):
    X = rng.integers(0, 256, (N, D)).astype(F32)
    if kind == "float":   # half the columns leave the byte path
        X[:, D // 2:] = (rng.standard_normal((N, D - D // 2)) * 3).astype(F32)
    return X


def main_case(kind, use_bootstrap):
    """C = 3, N = 600, D = 8, 4 rounds: labels from two features plus noise, trees too shallow to fit them."""
    rng = np.random.default_rng(11)
    X = _features(rng, 600, 8, kind)
    y = ((X[:, 0] > 100).astype(np.int32) + (X[:, 5] > (0 if kind == "float" else 128)).astype(np.int32))
    flip = rng.random(600) < 0.2
    y[flip] = rng.integers(0, 3, int(flip.sum()))
    return dict(X=X, y=y.astype(np.int32), n_classes=3, rounds=4, seed=21,
                params=dict(max_depth=3, min_split_examples=20, use_bootstrap=use_bootstrap))


def negative_alpha_case():
    """C = 2 with labels that are mostly noise: some round's error passes 1/2 and its alpha is negative."""
    rng = np.random.default_rng(5)
    X = _features(rng, 300, 6, "byte")
    y = (X[:, 1] > 128).astype(np.int32)
    flip = rng.random(300) < 0.45
    y[flip] = 1 - y[flip]
    return dict(X=X, y=y, n_classes=2, rounds=6, seed=NEGATIVE_ALPHA_SEED, params=dict(max_depth=1, min_split_examples=40, use_bootstrap=0))


NEGATIVE_ALPHA_SEED = 1   # searched on the CPU (test_boost_cases_cpu.py pins that it still does what it claims)


def separable_case():
    """Two clusters far apart: the first tree classifies the whole set, error == 0, alpha = +inf, boosting ends."""
    rng = np.random.default_rng(2)
    y = (np.arange(200) % 2).astype(np.int32)
    X = _features(rng, 200, 4, "byte")
    X[:, 2] = np.where(y == 1, 200, 10) + rng.integers(0, 20, 200)
    return dict(X=X.astype(F32), y=y, n_classes=2, rounds=3, seed=4, params=dict(max_depth=4, min_split_examples=2, num_features=4, use_bootstrap=1))


def all_wrong_case():
    """Every label is 1 and the smoothing swallows the histogram (h + 1e30 == 1e30 in fp32): both classes tie, the vote is
    class 0, every example is misclassified and error = 64 * (1/64) = 1: the tree is not added, no tree is kept."""
    rng = np.random.default_rng(3)
    return dict(X=_features(rng, 64, 4, "byte"), y=np.ones(64, np.int32), n_classes=2, rounds=3, seed=9,
                params=dict(max_depth=4, min_split_examples=2, smoothing=1e30, use_bootstrap=0))


def single_example_case():
    return dict(X=np.array([[3, 200, 7]], F32), y=np.array([1], np.int32), n_classes=3, rounds=2, seed=1,
                params=dict(max_depth=4, min_split_examples=2, use_bootstrap=1))


# ---- weight patterns of the resample kernels -------------------------------------------------------------------------
RESAMPLE_SIZES = (1, 63, 64, 65, 129, 255, 256, 257, 2047, 2048, 2049, 4097, 100003)   # 256: a tile, 2 048: a batch of the sums
RESAMPLE_PATTERNS = ("uniform", "first", "last", "middle", "denormal", "binade_inside", "binade_seam", "binade_tile_seam", "miss_all", "miss_alternating")


def resample_case(pattern, N):
    """(weights, miss or None, exp_alpha, key) of one pattern at one size."""
    rng = np.random.default_rng(N * 31 + len(pattern))
    w = np.full(N, F32(1) / F32(N), F32)
    miss, scale = None, F32(1)
    if pattern in ("first", "last", "middle"):       # long runs of zeros: equal cumsum values, the first index must win
        w = np.zeros(N, F32)
        w[{"first": 0, "last": N - 1, "middle": N // 2}[pattern]] = F32(0.75)
    elif pattern == "denormal":                      # denormal weights beside one large one
        w = np.full(N, F32(1e-41), F32)
        w[N // 3] = F32(2.5)
    elif pattern == "binade_inside":                 # the running sum crosses a power of two inside a 64-block ...
        w = rng.random(N).astype(F32) + F32(0.01)
        w[:min(N, 40)] = F32(2.0 ** -7)
    elif pattern == "binade_seam":                   # ... and exactly between two blocks
        w = rng.random(N).astype(F32) * F32(0.001)
        w[:min(N, 64)] = F32(1.0 / 64)
    elif pattern == "binade_tile_seam":              # ... and between two 256-value tiles of the sums
        w = rng.random(N).astype(F32) * F32(0.001)
        w[:min(N, 256)] = F32(1.0 / 256)
    elif pattern == "miss_all":
        w = rng.random(N).astype(F32)
        miss, scale = np.ones(N, bool), F32(1.75)
    elif pattern == "miss_alternating":
        w = rng.random(N).astype(F32)
        miss, scale = (np.arange(N) % 2).astype(bool), F32(0.3)
    return w, miss, scale, 0xB0057 + N


def clamp_case():
    """Rounding leaves cumsum[N-1] well below 1: after the one large weight every addend 1.5 * 2^-24 rounds UP in the
    total (1 + 1.5 * 2^-24 -> 1 + 2^-23) but, once the weights are divided by that inflated total, adds up to about its
    true share.  CLAMP_KEY has a draw above cumsum[N-1], which the reference would answer by reading past the array."""
    w = np.full(4097, F32(1.5 * 2.0 ** -24), F32)
    w[0] = F32(1)
    return w, None, F32(1), CLAMP_KEY


CLAMP_KEY = 1   # searched on the CPU
