"""TEST INFRASTRUCTURE ONLY -- a Python restatement of the boosted forest (libf::BoostedRandomForest and
BoostedRandomForestLearner, libforest classifier.cpp:238-307 and learning.cpp:1120-1234), written from those lines and from
the build-owned definitions in csrc/rvseg_train.hip, independently of the HIP code.

Per round the tree comes from the CPU oracle's learner (oracle.forest_train) on the materialised resample X[idx] with
num_trees = 1 and the round's seed; trees vote through orc_forest_eval and the first-strict-maximum rule; the fp32 chains
are np.float32 loops; alpha and exp(alpha) come from libm's logf / log / expf through ctypes.  The boosted stream is
written here, byte by byte."""
import ctypes as C
import ctypes.util
import struct

import numpy as np

from oracle import oracle as O

WEIGHT_FIRST, TREE_FIRST = 0, 1
_M = (1 << 64) - 1
F32 = np.float32

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]
_libm.log.restype = C.c_double
_libm.log.argtypes = [C.c_double]


# ---- the shared random source (definition 1) ---------------------------------------------------------------------------
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def draw64(key, i):
    return mix64(key ^ mix64((i + 0x632BE59BD9B4E019) & _M))


def _mix64_np(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def round_key(seed, rnd):
    return mix64(seed ^ mix64(0x626F6F73 + rnd))


def tree_seed(kb):
    return draw64(kb, 1 << 40)


def uniforms(kb, N):
    """u_n = (float)(draw64(kb, n) >> 40) * 2^-24 for n < N: 24 random bits, exact in fp32, in [0, 1)."""
    n = np.arange(N, dtype=np.uint64)
    with np.errstate(over="ignore"):
        d = _mix64_np(np.uint64(kb) ^ _mix64_np(n + np.uint64(0x632BE59BD9B4E019)))
    return (d >> np.uint64(40)).astype(F32) * F32(2.0 ** -24)


def pick(cumsum, u):
    """Definition 2: the first index with !(u > cumsum[index]), clamped to N - 1 (cumsum must not decrease)."""
    idx = np.searchsorted(cumsum, u, side="left")
    return np.minimum(idx, len(cumsum) - 1).astype(np.int32)


def pick_linear(cumsum, u):
    """The reference's own scan (learning.cpp:1169-1173) with the clamp, for the tests of pick()."""
    out = np.empty(len(u), np.int32)
    for k, x in enumerate(u):
        i = 0
        while i < len(cumsum) - 1 and x > cumsum[i]:
            i += 1
        out[k] = i
    return out


# ---- the fp32 chains (definition 3) --------------------------------------------------------------------------------------
def serial_sum(values):
    acc = F32(0)
    for v in values:
        acc = F32(acc + v)
    return acc


def serial_cumsum(values):
    out = np.empty(len(values), F32)
    acc = F32(0)
    for i, v in enumerate(values):
        acc = F32(acc + v) if i else F32(v)     # cumsum[0] = w[0] (:1212)
        out[i] = acc
    return out


def weight_round(w, miss, scale):
    """One round's arithmetic on the weights (:1181-1217): returns (error, total, weights, cumsum); weights and cumsum
    are None when the total is not positive and finite."""
    w = np.asarray(w, F32).copy()
    miss = np.asarray(miss, bool)
    error = serial_sum(w[miss])
    w[miss] = w[miss] * F32(scale)
    total = serial_sum(w)
    if not (total > 0 and np.isfinite(total)):
        return error, total, None, None
    w = w / total
    return error, total, w, serial_cumsum(w)


def alpha_of(error, n_classes):
    """:1197 -- logf of a float, log of an int (double), the sum narrowed to float."""
    error = F32(error)
    with np.errstate(divide="ignore"):
        ratio = F32(F32(1) - error) / error
    first = _libm.logf(C.c_float(float(ratio)))
    return F32(float(first) + _libm.log(C.c_double(float(n_classes - 1))))


def exp_of(alpha):
    return F32(_libm.expf(C.c_float(float(alpha))))


# ---- trees, votes, streams -------------------------------------------------------------------------------------------
def first_strict_max(post):
    """Classifier::classify (classifier.cpp:29-51) per row."""
    post = np.asarray(post, F32)
    label = np.zeros(post.shape[0], np.int32)
    best = post[:, 0].copy()
    for c in range(1, post.shape[1]):
        win = post[:, c] > best
        label[win] = c
        best[win] = post[win, c]
    return label


def split_trees(blob):
    """The trees of a forest.dat image (int32 T, then T trees), each as its own bytes."""
    (T,) = struct.unpack_from("<i", blob, 0)
    pos = 4
    trees = []

    def vec(pos, depth):
        (n,) = struct.unpack_from("<i", blob, pos)
        pos += 4
        if depth == 0:
            return pos + 4 * n
        for _ in range(n):
            pos = vec(pos, depth - 1)
        return pos
    for _ in range(T):
        start = pos
        for depth in (0, 0, 0, 1, 2):   # splitFeatures, thresholds, leftChild, histograms, multi_histograms
            pos = vec(pos, depth)
        trees.append(blob[start:pos])
    assert pos == len(blob)
    return trees


def one_tree_forest(tree):
    return struct.pack("<i", 1) + tree


def boosted_stream(trees, weights, order=WEIGHT_FIRST):
    """BoostedRandomForest::write (:250-262, the weight first) or the layout ::read expects (:264-280, the tree first)."""
    out = [struct.pack("<i", len(trees))]
    for t, w in zip(trees, weights):
        wb = np.asarray(w, F32).tobytes()
        out += [wb, t] if order == WEIGHT_FIRST else [t, wb]
    return b"".join(out)


def tree_votes(tree, X):
    return first_strict_max(O.Forest(one_tree_forest(tree)).eval(X, False))


def vote_sums(trees, weights, X, n_classes, labels=None):
    """BoostedRandomForest::classLogPosterior (:283-302): C zeros, then out[label_t] += weight_t in tree order.  labels:
    per tree, the votes to use in the place of this module's (the reference's compiled evaluator's)."""
    X = np.ascontiguousarray(X, F32)
    out = np.zeros((X.shape[0], n_classes), F32)
    rows = np.arange(X.shape[0])
    for t, (tree, w) in enumerate(zip(trees, weights)):
        lab = tree_votes(tree, X) if labels is None else labels[t]
        with np.errstate(invalid="ignore"):
            out[rows, lab] = out[rows, lab] + F32(w)
    return out


def one_hot_forest(trees, weights, n_classes):
    """The boosted model as an ordinary forest.dat: every leaf's single-label histogram becomes weight + 0.0 at its vote
    label and +0.0 elsewhere; no multi-layer histograms."""
    out = [struct.pack("<i", len(trees))]
    for tree, w in zip(trees, weights):
        pos = 0
        parts = []
        for _ in range(3):
            (n,) = struct.unpack_from("<i", tree, pos)
            parts.append(tree[pos:pos + 4 + 4 * n])
            pos += 4 + 4 * n
        left = np.frombuffer(parts[2][4:], np.int32)
        (n,) = struct.unpack_from("<i", tree, pos)
        pos += 4
        hist = [struct.pack("<i", n)]
        for v in range(n):
            (c,) = struct.unpack_from("<i", tree, pos)
            h = np.frombuffer(tree, F32, c, pos + 4)
            pos += 4 + 4 * c
            if left[v] == 0:
                row = np.zeros(n_classes, F32)
                row[first_strict_max(h[None, :])[0]] = F32(w) + F32(0)
                hist.append(struct.pack("<i", n_classes) + row.tobytes())
            else:
                hist.append(struct.pack("<i", c) + h.tobytes())
        mh = struct.pack("<i", n) + struct.pack("<i", 0) * n
        out += parts + hist + [mh]
    return b"".join(out)


# ---- the learner -----------------------------------------------------------------------------------------------------
def boosted_train(X, y, n_classes, rounds, seed, **tree_params):
    """BoostedRandomForestLearner::learn with the build-owned definitions.  Returns dict(model, trees, weights, rounds,
    errors, alphas, draws = per round the index list, history = per round the weights it started from)."""
    X = np.ascontiguousarray(X, F32)
    y = np.asarray(y, np.int32).reshape(-1)
    N = X.shape[0]
    w = np.full(N, F32(1) / F32(N), F32)                                       # :1140
    cumsum = (np.arange(1, N + 1).astype(F32) * F32(1)) / F32(N)               # :1141
    trees, weights, draws, history = [], [], [], []
    errors = np.full(rounds, np.nan, F32)
    alphas = np.full(rounds, np.nan, F32)
    for r in range(rounds):
        kb = round_key(seed, r)
        idx = pick(cumsum, uniforms(kb, N))
        draws.append(idx)
        history.append(w.copy())
        forest = O.forest_train(X[idx], y[idx], [n_classes], num_trees=1, seed=tree_seed(kb), **tree_params)
        (tree,) = split_trees(forest)
        miss = tree_votes(tree, X) != y
        error = serial_sum(w[miss])
        errors[r] = error
        if not error < 1:                                                      # definition 4: the tree is not added
            break
        alpha = alpha_of(error, n_classes)
        if error == 0:                                                         # alpha = +inf: added, boosting ends
            alphas[r] = alpha
            trees.append(tree)
            weights.append(alpha)
            break
        _, total, w2, cumsum2 = weight_round(w, miss, exp_of(alpha))
        if w2 is None:                                                         # the tree is not added
            break
        alphas[r] = alpha
        trees.append(tree)
        weights.append(alpha)
        w, cumsum = w2, cumsum2
    return {"model": boosted_stream(trees, weights), "trees": trees, "weights": np.asarray(weights, F32), "rounds": len(trees),
            "errors": errors, "alphas": alphas, "draws": draws, "history": history}
