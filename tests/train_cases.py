"""Data recipes for the forest trainer's limits (plain helper module, like crf_restate.py): the CPU pins
(test_train_cases_cpu.py: the oracle alone shows that a recipe crosses its edge) and the GPU comparisons
(test_gpu_train_limits.py: trainer == oracle byte for byte) draw the same bytes from here.

A case is a dict: X (P, D) float32, labels (P, L) int32, cc (class counts), kw (training parameters) and, where a
pin needs them, extra facts about how the data was built (`cut`, `sorted`, ...).

The switches of the trainer (csrc/rvseg_train.hip, train_host.h, kernels_train.hip) the recipes are built around:
  SLOT_BATCH = 1024   frontier nodes per batch of a level;  TR_CMAX = 16 classes per layer;  RVSEG_MAX_LAYERS = 8,
  at most 64 classes over all layers;  byte features (integers in [0, 255]: histograms) against float features
  (sorted, scanned by one wave in chunks of 64);  the 1e-6 cut rule;  the adjacent-floats threshold guard.
"""
import struct

import numpy as np

SLOT_BATCH = 1024
TR_CMAX = 16
MAX_LAYERS = 8
CHUNK = 64


# ---- forest.dat ----------------------------------------------------------------------------------------------------
def parse(blob):
    """forest.dat -> list of trees: dict(feat, thr, left, hist[list], mhist[list of list])"""
    pos = 0
    T = struct.unpack_from("<i", blob, pos)[0]; pos += 4
    trees = []
    for _ in range(T):
        n = struct.unpack_from("<i", blob, pos)[0]
        feat = np.frombuffer(blob, np.int32, n, pos + 4); pos += 4 + 4 * n
        thr = np.frombuffer(blob, np.float32, n, pos + 4); pos += 4 + 4 * n
        left = np.frombuffer(blob, np.int32, n, pos + 4); pos += 4 + 4 * n
        cnt = struct.unpack_from("<i", blob, pos)[0]; pos += 4
        hist = []
        for _i in range(cnt):
            m = struct.unpack_from("<i", blob, pos)[0]; pos += 4
            hist.append(np.frombuffer(blob, np.float32, m, pos).copy()); pos += 4 * m
        cnt = struct.unpack_from("<i", blob, pos)[0]; pos += 4
        mhist = []
        for _i in range(cnt):
            m = struct.unpack_from("<i", blob, pos)[0]; pos += 4
            layers = []
            for _l in range(m):
                c = struct.unpack_from("<i", blob, pos)[0]; pos += 4
                layers.append(np.frombuffer(blob, np.float32, c, pos).copy()); pos += 4 * c
            mhist.append(layers)
        trees.append(dict(feat=feat, thr=thr, left=left, hist=hist, mhist=mhist))
    assert pos == len(blob)
    return trees


def node_depths(tree):
    left = tree["left"]
    depth = np.zeros(len(left), np.int64)
    for v in range(len(left)):          # children are appended after their parent in the file's order
        if left[v] != 0:
            assert left[v] > v
            depth[left[v]] = depth[left[v] + 1] = depth[v] + 1
    return depth


def level_widths(tree):
    """Nodes per depth: the frontier sizes the level-wise trainer meets (a level of w nodes takes ceil(w / 1024) batches)."""
    return np.bincount(node_depths(tree))


def route(tree, X):
    """findLeafNode for every row (classifier.cpp:97-117)."""
    node = np.zeros(X.shape[0], np.int64)
    while True:
        l = tree["left"][node]
        go = l != 0
        if not go.any():
            return node
        v = X[np.arange(X.shape[0]), tree["feat"][node]]
        node = np.where(go, np.where(v < tree["thr"][node], l, l + 1), node)


def case(X, labels, cc, **extra):
    kw = extra.pop("kw")
    X = np.ascontiguousarray(X, np.float32)
    labels = np.ascontiguousarray(np.asarray(labels, np.int32).reshape(X.shape[0], -1))
    assert labels.shape[1] == len(cc)
    return dict(X=X, labels=labels, cc=list(cc), kw=kw, **extra)


# ---- 1. slot batches -----------------------------------------------------------------------------------------------
def slot_batches(P=60000, max_depth=20, rng_seed=5):
    """One deep tree on noise labels.  The oracle's tree has 11 621 nodes; its levels 17 to 21 are 1206, 1272, 1310, 1304
    and 1356 nodes wide: five levels of two batches each."""
    rng = np.random.default_rng(rng_seed)
    X = np.empty((P, 10), np.float32)
    X[:, :8] = rng.integers(0, 256, (P, 8))
    X[:, 8] = rng.uniform(0, 20, P)
    X[:, 9] = rng.normal(0, 1, P)
    labels = rng.integers(0, 16, (P, 4))
    return case(X, labels, [16] * 4, kw=dict(num_trees=1, max_depth=max_depth, min_split_examples=8, min_child_split_examples=1,
                                           use_bootstrap=1, seed=2))


def slot_batches_three(P=120000, max_depth=22):
    """The same recipe with twice the examples and two more levels: levels wider than 2048, three batches (the oracle
    takes under 2 s for it)."""
    return slot_batches(P=P, max_depth=max_depth, rng_seed=6)


# ---- 2. class and layer layouts ------------------------------------------------------------------------------------
LAYOUTS = [[1], [2], [9], [15], [16], [16, 1], [1, 16], [2, 9, 15], [16, 16, 16, 16], [8] * 8, [1, 2, 9, 15, 16],
           [15, 16, 2, 9, 1, 2], [9, 1, 2, 15, 16, 1, 2], [16, 15, 9, 2, 1, 1, 2, 9]]
REFUSED_LAYOUTS = [[17], [3, 17], [1] * 9, [16, 16, 16, 16, 1]]


def layout(cc, P=2500, seed=0):
    """Every layer's label is a learnable function of one column (byte columns and float columns in turn) that reaches
    the layer's last class, plus 3 % noise drawn over all classes."""
    rng = np.random.default_rng(1000 + seed)
    D = 12
    X = rng.integers(0, 256, (P, D)).astype(np.float32)
    X[:, 10] = rng.uniform(0, 255.999, P)
    X[:, 11] = rng.uniform(0, 255.999, P)
    labels = np.zeros((P, len(cc)), np.int32)
    for l, C in enumerate(cc):
        col = (10, 3, 11, 7, 0, 5, 9, 1)[l]
        lab = np.minimum((X[:, col] * np.float32(C / 256.0)).astype(np.int32), C - 1)
        noise = rng.random(P) < 0.03
        labels[:, l] = np.where(noise, rng.integers(0, C, P), lab)
        labels[0, l] = C - 1                                     # the last class occurs whatever the draw
    return case(X, labels, cc, kw=dict(num_trees=3, max_depth=12, min_split_examples=10, min_child_split_examples=1, seed=3 + seed))


# ---- 3. feature kinds ----------------------------------------------------------------------------------------------
def _isolating(X, y, cc, **kw):
    base = dict(num_trees=1, max_depth=30, min_split_examples=2, min_child_split_examples=1, num_features=X.shape[1], use_bootstrap=0, seed=1)
    base.update(kw)
    return base


def all_bytes(P=2000, D=9):
    rng = np.random.default_rng(31)
    X = rng.integers(0, 256, (P, D)).astype(np.float32)
    y = (X[:, 2] < 77).astype(np.int32) + 2 * (X[:, 5] >= 200).astype(np.int32)
    y = np.where(rng.random(P) < 0.05, rng.integers(0, 4, P), y)
    return case(X, y, [4], kw=dict(num_trees=2, max_depth=10, min_split_examples=6, seed=4))


def all_floats(P=2000, D=4):
    """No byte feature at all, every feature sampled at every node (num_features = D)."""
    rng = np.random.default_rng(32)
    X = rng.normal(0, 3, (P, D)).astype(np.float32)
    y = (X[:, 0] < 0.5).astype(np.int32) + 2 * (X[:, 3] < -1).astype(np.int32)
    y = np.where(rng.random(P) < 0.05, rng.integers(0, 4, P), y)
    return case(X, y, [4], kw=dict(num_trees=2, max_depth=10, min_split_examples=6, num_features=D, seed=4))


def single_feature(kind, P=1500):
    rng = np.random.default_rng(33)
    X = rng.integers(0, 256, (P, 1)).astype(np.float32) if kind == "byte" else rng.uniform(-4, 4, (P, 1)).astype(np.float32)
    t = 100 if kind == "byte" else 0.7
    y = (X[:, 0] < t).astype(np.int32)
    y = np.where(rng.random(P) < 0.1, 1 - y, y)
    return case(X, y, [2], kw=dict(num_trees=2, max_depth=8, min_split_examples=4, seed=6))


def byte_edge(kind):
    """Column 0 carries the edge of byte detection and the label hangs on it, so the oracle's tree must cut there:
         "255.5"  integers in [0, 255] and one 255.5 (cut 255 | 255.5 at 255.25)      -> a float column
         "256"    integers in [0, 256]            (cut 255 | 256 at 255.5)            -> a float column
         "-1"     integers in [-1, 255]           (cut -1 | 0 at -0.5)                -> a float column
         "0_255"  only the values 0 and 255       (cut at 127.5)                      -> a byte column, first and last bin
         "-0.0"   only -0.0 and +0.0              (no cut: the two are equal)         -> a byte column, one bin
       Column 1 is a plain byte column, column 2 a plain float column; every node looks at all three."""
    rng = np.random.default_rng(34)
    P = 600
    X = np.zeros((P, 3), np.float32)
    X[:, 0] = rng.integers(0, 256, P)
    X[:, 1] = rng.integers(0, 256, P)
    X[:, 2] = rng.uniform(-1, 1, P)
    X[:40, 0] = 255                         # enough mass right below the edge
    if kind == "255.5":
        X[7, 0] = 255.5
        y = (X[:, 0] > 255.25).astype(np.int32)
    elif kind == "256":
        X[40:60, 0] = 256
        y = (X[:, 0] > 255.5).astype(np.int32)
    elif kind == "-1":
        X[40:60, 0] = -1
        X[60:80, 0] = 0
        y = (X[:, 0] < -0.5).astype(np.int32)
    elif kind == "0_255":
        X[:, 0] = np.where(rng.random(P) < 0.5, 0, 255)
        y = (X[:, 0] > 127).astype(np.int32)
    elif kind == "-0.0":
        X[:, 0] = np.where(rng.random(P) < 0.5, -0.0, 0.0)
        assert np.signbit(X[:, 0]).any() and not np.signbit(X[:, 0]).all()
        y = (X[:, 1] < 90).astype(np.int32)
    else:
        raise KeyError(kind)
    y[1::97] ^= 1                            # a little noise: the tree goes on below the edge cut
    return case(X, y, [2], kw=_isolating(X, y, [2]), kind=kind)


BYTE_EDGES = {"255.5": 255.25, "256": 255.5, "-1": -0.5, "0_255": 127.5, "-0.0": None}


# ---- 4. scan seams -------------------------------------------------------------------------------------------------
def _one_float(values_sorted, y_sorted, seed, **extra):
    """One float column given in ascending order; rows are shuffled so that the sort has work to do."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(values_sorted))
    X = np.asarray(values_sorted, np.float32)[perm][:, None]
    y = np.asarray(y_sorted, np.int32)[perm]
    kw = dict(num_trees=1, max_depth=30, min_split_examples=1, min_child_split_examples=1, num_features=1, use_bootstrap=0, seed=1)
    return case(X, y, [2], kw=kw, sorted=np.asarray(values_sorted, np.float32), **extra)


# (P, position of the best cut): the root's sorted segment has P elements and its labels flip once, at `cut`, so the
# best cut lies between sorted positions cut - 1 | cut.  Seams of the scan are at multiples of 64.
SEAM_SPLITS = [(1, None), (2, 1), (63, 31), (63, 62), (64, 32), (64, 63), (65, 64), (65, 1), (128, 64), (129, 128), (129, 64),
               (200, 64), (200, 128), (4097, 4096), (4097, 2048), (4097, 1)]


def seam_split(P, cut):
    v = np.sort(np.random.default_rng(40 + P).uniform(0.5, 9.0, P).astype(np.float32))
    assert P == 1 or np.diff(v).min() >= 1e-6 or P > 4000
    if P > 4000:                              # dense enough for near-ties: spread them out exactly
        v = (0.5 + np.arange(P) * 2e-3).astype(np.float32)
    y = (np.arange(P) >= cut).astype(np.int32) if cut is not None else np.zeros(P, np.int32)
    return _one_float(v, y, P, cut=cut)


def seam_run(kind, seam=64, P=200):
    """A run of eleven equal ("tie") or less-than-1e-6-apart ("near") values over sorted positions seam - 4 .. seam + 6,
    labels flipping AT the seam, inside the run: no cut is allowed inside the run, so the best one is at an end of it."""
    v = (0.5 + np.arange(P) * 0.01).astype(np.float32)
    lo, hi = seam - 4, seam + 7               # the run is [lo, hi)
    if kind == "tie":
        v[lo:hi] = v[lo]
    else:
        one = np.float32(1.0)
        v[lo:hi] = one + np.arange(hi - lo).astype(np.float32) * np.float32(2.0 ** -22)    # 2 ulps = 2.4e-7 apart, 2.4e-6 end to end
        v[:lo] = np.linspace(0.1, 0.9, lo).astype(np.float32)
        v[hi:] = (1.5 + np.arange(P - hi) * 0.01).astype(np.float32)
    assert np.all(np.diff(v) >= 0)
    y = (np.arange(P) >= seam).astype(np.int32)
    return _one_float(v, y, 7, run=(lo, hi), seam=seam)


def seam_noise(P=4097):
    """Coin-flip labels on distinct values: the tree grows until every leaf is pure, so segments of every small length
    (1, 2, 3, ...) and every alignment pass through the scan."""
    rng = np.random.default_rng(44)
    v = (np.arange(P) * 0.25 - 300).astype(np.float32)
    return _one_float(v, rng.integers(0, 2, P), 8)


# ---- 5. threshold rules --------------------------------------------------------------------------------------------
def adjacent_floats(start, k, n=8):
    """n consecutive floats from `start` away from zero (|values| >= 16, so one ulp is above the 1e-6 cut rule), in
    ascending order, labels flipping between sorted positions k - 1 | k.  `guard` says whether (left + right) * 0.5f
    rounds to `left` in float arithmetic -- then only the guard of the oracle's definition 4 keeps `x < threshold`
    separating the two; otherwise the midpoint rounds to `right` by itself."""
    v = np.empty(n, np.float32)
    v[0] = start
    for i in range(1, n):
        v[i] = np.nextafter(v[i - 1], np.float32(np.inf if start > 0 else -np.inf))
    v = np.sort(v)
    left, right = v[k - 1], v[k]
    mid = np.float32(np.float32(left + right) * np.float32(0.5))
    y = (np.arange(n) >= k).astype(np.int32)
    return _one_float(v, y, 3, cut=k, guard=bool(mid == left), left=left, right=right)


ADJACENT = [(16.0, 3), (16.0, 4), (16.0, 5), (-16.0, 3), (-16.0, 4), (1024.5, 2), (1024.5, 3), (-1024.5, 4), (-1024.5, 5), (3.0e7, 4),
            (3.0e7, 5)]


def sentinel_and_negatives(P=3000):
    """The normal feature's shape: -2 where there is no normal, otherwise an angle; a second column all negative; the
    labels hang on both, one of them on `value == -2`."""
    rng = np.random.default_rng(52)
    X = np.zeros((P, 3), np.float32)
    X[:, 0] = np.where(rng.random(P) < 0.15, -2.0, rng.uniform(0, np.pi / 2, P))
    X[:, 1] = -rng.uniform(1e-3, 50.0, P)
    X[:, 2] = rng.integers(0, 256, P)
    y0 = (X[:, 0] < -1).astype(np.int32) + 2 * (X[:, 1] < -20).astype(np.int32)
    y0 = np.where(rng.random(P) < 0.03, rng.integers(0, 4, P), y0)
    return case(X, y0, [4], kw=dict(num_trees=2, max_depth=10, min_split_examples=6, num_features=3, seed=8))


def huge_values(sign):
    """Finite values whose pairwise sum overflows float: left + right = +-inf, where (left + right) * 0.5f is no
    midpoint any more.  Definition 4: the threshold is then `right`."""
    big = np.array([2.6e38, 2.7e38, 2.8e38, 2.9e38, 3.0e38, 3.1e38, 3.2e38, 3.3e38], np.float32)
    v = big if sign > 0 else -big[::-1]
    if sign == 0:
        v = np.concatenate([-big[::-1], big])             # the cut -2.6e38 | 2.6e38 sums to 0: an ordinary midpoint
    y = (np.arange(len(v)) >= len(v) // 2).astype(np.int32)
    if sign != 0:
        y[1] ^= 1                                          # a second cut among the huge values
    return _one_float(v, y, 5, cut=len(v) // 2)


# ---- 6. stop rules and parameters ----------------------------------------------------------------------------------
def _mixed(P, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (P, D)).astype(np.float32)
    X[:, D - 1] = rng.uniform(0.5, 15.0, P)
    y = (X[:, 0] < 100).astype(np.int32) + (X[:, D - 1] < 6.0).astype(np.int32)
    y = np.where(rng.random(P) < 0.1, rng.integers(0, 3, P), y)
    return X, y


PARAMS = {
    "max_depth_1": dict(max_depth=1),
    "max_depth_2": dict(max_depth=2),
    "min_split_0": dict(min_split_examples=0, max_depth=8),
    "min_split_1_no_bootstrap": dict(min_split_examples=1, use_bootstrap=0, max_depth=30),
    "min_child_0": dict(min_child_split_examples=0, min_split_examples=4, max_depth=8),
    "min_child_above_half": dict(min_child_split_examples=401, min_split_examples=4),
    "min_child_half": dict(min_child_split_examples=150, min_split_examples=4, use_bootstrap=0),
    "num_features_1": dict(num_features=1, min_split_examples=10, max_depth=10),
    "num_features_D": dict(num_features=6, min_split_examples=10, max_depth=10),
    "num_trees_1": dict(num_trees=1, min_split_examples=10, max_depth=10),
    "num_trees_64": dict(num_trees=64, min_split_examples=40, max_depth=6),
    "smoothing_0": dict(smoothing=0.0, min_split_examples=2, max_depth=30),
    "smoothing_small": dict(smoothing=1e-30, min_split_examples=10, max_depth=10),
    "seed_0": dict(seed=0, min_split_examples=10, max_depth=10),
    "seed_max": dict(seed=2 ** 64 - 1, min_split_examples=10, max_depth=10),
}


def params(name):
    X, y = _mixed(800, 6, 61)
    kw = dict(num_trees=2, seed=5)
    kw.update(PARAMS[name])
    return case(X, y, [3], kw=kw)


# ---- 7. degenerate sets --------------------------------------------------------------------------------------------
DEGENERATE = ["P1", "P2_same_label", "P2_two_labels", "constant_features", "pure_labels", "absent_class", "identical_rows",
              "identical_rows_two_labels"]


def degenerate(name, bootstrap):
    rng = np.random.default_rng(71)
    P, D = 300, 5
    X = rng.integers(0, 256, (P, D)).astype(np.float32)
    X[:, 4] = rng.uniform(-3, 3, P)
    y = (X[:, 1] < 128).astype(np.int32)
    cc = [2]
    if name == "P1":
        X, y = X[:1], y[:1]
    elif name == "P2_same_label":
        X, y = X[:2], np.array([1, 1], np.int32)
    elif name == "P2_two_labels":
        X, y = X[:2], np.array([0, 1], np.int32)
    elif name == "constant_features":
        X = np.tile(np.array([[7, 0, 255, 31, 2.5]], np.float32), (P, 1))
    elif name == "pure_labels":
        y = np.ones(P, np.int32)
    elif name == "absent_class":
        y = 2 * y                                # classes 0 and 2 of 4; 1 and 3 never occur: freq = P / 0
        cc = [4]
    elif name == "identical_rows":
        X = np.tile(X[:1], (P, 1))
        y = np.zeros(P, np.int32)
    elif name == "identical_rows_two_labels":
        X = np.tile(X[:1], (P, 1))
    else:
        raise KeyError(name)
    return case(X, y, cc, kw=dict(num_trees=3, max_depth=10, min_split_examples=1, min_child_split_examples=1, num_features=D,
                                  use_bootstrap=bootstrap, seed=9))


# ---- 8. more than 2^24 examples of one class -----------------------------------------------------------------------
def many_examples():
    """2^25 + 39 examples of class 0 and 25 of class 1 in one float column: the float counter behind the inverted class
    frequency (data.h:358-370 counts with `freq[label]++` on a float) stops growing at 2^24, so class 0 weighs
    P / 2^24 = 2.0 per example, not P / count = 1.0.  The oracle takes about 4 s for it."""
    P = (1 << 25) + 64
    X = np.full((P, 1), 0.25, np.float32)
    y = np.zeros(P, np.int32)
    X[-25:, 0] = 0.75
    y[-25:] = 1
    X[5, 0] = 0.75                               # one class-0 example on the other side: the right child is not pure
    return case(X, y, [2], kw=dict(num_trees=1, max_depth=1, min_split_examples=2, min_child_split_examples=1, num_features=1,
                                   use_bootstrap=0, seed=1))


# ---- 9. training from frames ---------------------------------------------------------------------------------------
W, H = 160, 120
FRAME_CONFIGS = {
    # name: (context / extraction parameters, number of frames, augment)
    "plain": (dict(patch_size=9, patch_size_reduce=3), 2, False),
    "no_colour_patch": (dict(patch_size=9, patch_size_reduce=3, feature_color_patch=0), 2, False),
    "no_normal": (dict(patch_size=9, patch_size_reduce=3, feature_normal=0), 2, False),
    "stride_1": (dict(patch_size=9, patch_size_reduce=3, stride=1, feature_color_patch=0), 1, False),
    "stride_4": (dict(patch_size=9, patch_size_reduce=3, stride=4), 2, True),
    "two_calibrations": (dict(patch_size=9, patch_size_reduce=3), 2, False),
    "empty_frame_between": (dict(patch_size=9, patch_size_reduce=3), 3, False),
}


def frames(name):
    """rgb, depth, calib (n, 21), labels (n, 2, H, W) int8, class counts, context parameters, augment."""
    from rovinasemanticsegmentation_amd import synthetic
    ctx_kw, n, augment = FRAME_CONFIGS[name]
    rgb, depth = synthetic.make_batch(n, W, H, holes=True, start=2)
    calib = np.tile(np.asarray(synthetic.make_calib(W, H), np.float32).reshape(1, 21), (n, 1))
    if name == "two_calibrations":
        calib[1, :4] *= np.float32(1.25)       # another focal length / centre for the second frame
        calib[1, 4:] += np.float32(0.01)
    if name == "empty_frame_between":
        depth[1] = 0
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.empty((n, 2, H, W), np.int8)
    for i in range(n):
        lab[i, 0] = ((xx // 40) + i) % 3
        lab[i, 1] = ((yy // 30) + (xx // 80)) % 4
        lab[i, 0][(xx + 2 * yy) % 13 == 0] = -1
        lab[i, 1][yy < 5] = -3
    return dict(rgb=rgb, depth=depth, calib=calib, lab=lab, cc=[3, 4], ctx_kw=dict(width=W, height=H, **ctx_kw), augment=augment,
                kw=dict(num_trees=2, max_depth=8, min_split_examples=10, seed=9))


def frames_dataset(oracle, fr):
    """The P x D matrix the reference's DataStorage would hold (src/train.cpp:115-147, WITH_POSITIVE_LABEL), from the
    oracle's extraction; also the number of examples each frame contributes."""
    p = oracle.default_params(**fr["ctx_kw"])
    Xs, Ys, per_frame = [], [], []
    rgb, depth, lab = fr["rgb"], fr["depth"], fr["lab"]
    for i in range(rgb.shape[0]):
        count = 0
        for a in ((-20, 0, 20) if fr["augment"] else (0,)):
            col = rgb[i].astype(np.int32)
            col[:, :, 0] = np.clip(col[:, :, 0] + a, 0, 255)
            col = col.astype(np.uint8)
            for flip in ((False, True) if fr["augment"] else (False,)):
                c2 = col[:, ::-1].copy() if flip else col
                d2 = depth[i][:, ::-1].copy() if flip else depth[i]
                l2 = lab[i][:, :, ::-1] if flip else lab[i]
                feats, xs, ys = oracle.extract(p, c2, d2, fr["calib"][i])
                keep = (l2[0][ys, xs] >= 0) & (l2[1][ys, xs] >= 0)
                Xs.append(feats[keep])
                Ys.append(np.stack([l2[0][ys, xs][keep], l2[1][ys, xs][keep]], 1).astype(np.int32))
                count += int(keep.sum())
        per_frame.append(count)
    return np.concatenate(Xs), np.concatenate(Ys), per_frame


# ---- every matrix case under one name ------------------------------------------------------------------------------
def all_cases():
    """name -> zero-argument recipe, for everything that is compared through ctx.forest_train (cases 2-7)."""
    out = {}
    for i, cc in enumerate(LAYOUTS):
        out["layout_" + "_".join(map(str, cc))] = (lambda cc=cc, i=i: layout(cc, seed=i))
    out["all_bytes"] = all_bytes
    out["all_floats"] = all_floats
    out["single_byte_feature"] = lambda: single_feature("byte")
    out["single_float_feature"] = lambda: single_feature("float")
    for k in BYTE_EDGES:
        out["byte_edge_" + k] = (lambda k=k: byte_edge(k))
    for P, cut in SEAM_SPLITS:
        out["seam_P%d_cut%s" % (P, cut)] = (lambda P=P, cut=cut: seam_split(P, cut))
    for kind in ("tie", "near"):
        for seam in (64, 128):
            out["seam_run_%s_%d" % (kind, seam)] = (lambda kind=kind, seam=seam: seam_run(kind, seam))
    out["seam_noise"] = seam_noise
    for start, k in ADJACENT:
        out["adjacent_%g_cut%d" % (start, k)] = (lambda start=start, k=k: adjacent_floats(start, k))
    out["sentinel_and_negatives"] = sentinel_and_negatives
    for sign, nm in ((1, "pos"), (-1, "neg"), (0, "both")):
        out["huge_" + nm] = (lambda sign=sign: huge_values(sign))
    for name in PARAMS:
        out["params_" + name] = (lambda name=name: params(name))
    for name in DEGENERATE:
        for b in (0, 1):
            out["degenerate_%s_%s" % (name, "bootstrap" if b else "plain")] = (lambda name=name, b=b: degenerate(name, b))
    return out


def train(oracle_or_ctx, c):
    return oracle_or_ctx.forest_train(c["X"], c["labels"], c["cc"], **c["kw"])
