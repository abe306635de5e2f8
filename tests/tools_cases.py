"""TEST INFRASTRUCTURE ONLY -- the recipes of the forest-tools tests (tests/test_gpu_forest_tools.py) and a numpy
restatement of libforest's tools.h (AccuracyTool, ConfusionMatrixTool, CorrelationTool; tools.cpp:61-231) written from
those lines, independently of the HIP code: trees vote through the CPU oracle's evaluator on one-tree files and the
first-strict-maximum rule of boost_restate, the counts are numpy sums and the three score formulas are np.float32
expressions.  What each case claims -- scores that are not trivial -- is pinned in tests/test_tools_cases_cpu.py."""
import ctypes as C
import os
import struct

import numpy as np

import boost_restate as br
import train_cases as trc
from oracle import oracle as O

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENSEMBLE_SIZES = (1, 4, 5, 16, 17, 64)          # the 4-lane / 16-lane switch at 4 | 5, looped trees from 17
POINT_COUNTS = (1, 15, 16, 17, 63, 64, 65, 1000)
CHUNK_TAIL = 65536 + 257                        # one chunk of the tools and a ragged tail
TINY_CTX = dict(patch_size_reduce=1, feature_height=0, feature_normal=0)   # a context whose feature length is 4
LABEL_SEED = 7                                  # (test_tools_cases_cpu.py pins that the scores stay non-trivial)
_cache = {}


def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as fh:
        return fh.read()


def _tree(feat, thr, left, hist):
    n = len(feat)
    out = [struct.pack("<i", n), np.asarray(feat, np.int32).tobytes(), struct.pack("<i", n), np.asarray(thr, F32).tobytes(),
           struct.pack("<i", n), np.asarray(left, np.int32).tobytes(), struct.pack("<i", n)]
    for h in hist:
        out.append(struct.pack("<i", len(h)) + np.asarray(h, F32).tobytes())
    out.append(struct.pack("<i", n) + struct.pack("<i", 0) * n)
    return b"".join(out)


def nan_tie_trees():
    """Three stumps over D = 4 with 4 single-label classes whose leaves hold an all-equal row, a NaN at class 0, a NaN
    at a later class and -inf beside a NaN: the sums tie, carry a NaN at 0 or elsewhere, or are -inf but at one class."""
    nan, inf = np.nan, np.inf
    return [_tree([0, 0, 0], [128, 0, 0], [1, 0, 0], [[], [nan, 1, 2, 3], [1, 1, 1, 1]]),
            _tree([1, 0, 0], [100, 0, 0], [1, 0, 0], [[], [0, 1.5, 2.5, 0], [0.25, nan, 0.25, 0.5]]),
            _tree([3, 0, 0], [60.5, 0, 0], [1, 0, 0], [[], [-inf, -inf, nan, -inf], [2, 2, 1, 2]])]


def forest_of(trees):
    return struct.pack("<i", len(trees)) + b"".join(trees)


def forest(name):
    """name -> dict(blob, ctx = context parameters, D, layers = the (multi_layer, layer) heads the tests walk)."""
    if name == "tiny":
        return dict(blob=_golden("forest_tiny.dat"), ctx=dict(TINY_CTX, multi_layer=0), D=4, layers=[0])
    if name == "multi":
        return dict(blob=_golden("forest_multi.dat"), ctx=dict(multi_layer=1), D=366, layers=[0, 1])
    if name == "single":
        return dict(blob=_golden("forest_single.dat"), ctx=dict(multi_layer=0), D=366, layers=[0])
    if name.startswith("ensemble"):   # the four trees of forest_single.dat, cycled
        T = int(name[len("ensemble"):])
        trees = br.split_trees(_golden("forest_single.dat"))
        return dict(blob=forest_of([trees[t % 4] for t in range(T)]), ctx=dict(multi_layer=0), D=366, layers=[0])
    if name.startswith("nan_tie"):    # 3 trees, or 6: C = 4 classes on the 16-lane path
        T = int(name[len("nan_tie"):])
        trees = nan_tie_trees()
        return dict(blob=forest_of([trees[t % 3] for t in range(T)]), ctx=dict(TINY_CTX, multi_layer=0), D=4, layers=[0])
    raise KeyError(name)


FORESTS = ["tiny", "multi", "single"] + ["ensemble%d" % T for T in ENSEMBLE_SIZES] + ["nan_tie3", "nan_tie6"]


def points(D, P):
    from rovinasemanticsegmentation_amd import synthetic
    if (D, P) not in _cache:
        _cache[(D, P)] = synthetic.random_points(5, P, D)
    return _cache[(D, P)]


# ---- the restatement --------------------------------------------------------------------------------------------------
def _layer_slice(f, multi, layer):
    cc = f.classes(multi)
    off = int(np.sum(cc[:layer]))
    return slice(off, off + cc[layer])


def restate_blob(blob, X, multi, layer=0):
    """dict(pred (P,), votes (T, P) uint8, C) of any forest.dat image on the points X: Classifier::classify on the forest
    posterior and on every tree's own, through the CPU oracle on the whole forest and on one-tree files."""
    whole = O.Forest(blob)
    sl = _layer_slice(whole, multi, layer)
    with np.errstate(invalid="ignore"):
        pred = br.first_strict_max(whole.eval(X, multi)[:, sl])
        by_tree, votes = {}, []
        for tree in br.split_trees(blob):
            if tree not in by_tree:
                by_tree[tree] = br.first_strict_max(O.Forest(br.one_tree_forest(tree)).eval(X, multi)[:, sl]).astype(np.uint8)
            votes.append(by_tree[tree])
    return dict(pred=pred, votes=np.stack(votes), C=sl.stop - sl.start)


def restate(name, P, layer=0):
    """restate_blob of a named forest of this module on its own points, computed once."""
    key = ("restate", name, P, layer)
    if key not in _cache:
        fo = forest(name)
        _cache[key] = restate_blob(fo["blob"], points(fo["D"], P), bool(fo["ctx"]["multi_layer"]), layer)
    return _cache[key]


def labels_for(pred, C, seed=LABEL_SEED):
    """The restated forest label with ~30 % replaced by another class."""
    rng = np.random.default_rng(seed)
    lab = np.asarray(pred, np.int32).copy()
    flip = rng.random(lab.shape[0]) < 0.3
    lab[flip] = (lab[flip] + rng.integers(1, C, int(flip.sum()))) % C
    return lab


def confusion_counts(labels, pred, C):
    out = np.zeros((C, C), np.uint64)
    np.add.at(out, (labels, pred), 1)
    return out


def agreement_counts(votes):
    T = votes.shape[0]
    out = np.zeros((T, T), np.uint64)
    for t in range(T):
        out[t] = (votes == votes[t]).sum(1)
    return out


def accuracy(conf):
    """tools.cpp:77 -- 1.0f - error / (float)size, error an int."""
    conf = np.asarray(conf, np.uint64)
    size = int(conf.sum())
    errors = size - int(np.trace(conf))
    return F32(F32(1.0) - F32(errors) / F32(size))


def confusion_normalised(conf):
    """tools.cpp:126-135 -- a float cell grown by += 1 (it stops at 2^24) over the row's int count; 0 / 0 stays NaN."""
    conf = np.asarray(conf, np.uint64)
    cell = np.minimum(conf, np.uint64(1 << 24)).astype(F32)
    rows = conf.sum(1).astype(np.int64).astype(F32)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (cell / rows).astype(F32)


def correlation(agree, P):
    """tools.cpp:226-228 -- 1 - hammingDist / (float)size per pair."""
    dist = (np.int64(P) - np.asarray(agree, np.uint64).astype(np.int64)).astype(F32)
    return (1 - (dist / F32(P)).astype(F32)).astype(F32)


# ---- the refit: leaf counts and leaves, recomputed ---------------------------------------------------------------------
def _walk_counts(blob, X, labels, cc):
    """[node over all trees][sumC]: the examples per leaf and (layer, class), zeros at inner nodes."""
    offs = np.concatenate([[0], np.cumsum(cc)])
    rows = []
    for tree in trc.parse(blob):
        cnt = np.zeros((len(tree["left"]), offs[-1]), np.uint32)
        node = trc.route(tree, X)
        for l in range(len(cc)):
            np.add.at(cnt, (node, offs[l] + labels[:, l]), 1)
        rows.append(cnt)
    return np.concatenate(rows)


def _leaves_from_counts(cnt, labels, cc, smoothing):
    """updateMultiHistograms from integer counts, as tests/test_gpu_train.py recomputes the trainer's leaves: n additions of
    the inverted class frequency, then log((h + s) / (total + C s)), all fp32."""
    offs = np.concatenate([[0], np.cumsum(cc)])
    P = labels.shape[0]
    out = []
    for l, Cn in enumerate(cc):
        class_cnt = np.bincount(labels[:, l], minlength=Cn)
        with np.errstate(divide="ignore"):
            freq = (F32(P) / class_cnt.astype(F32)).astype(F32)
        h = np.zeros(Cn, F32)
        for c in range(Cn):
            acc = F32(0)
            for _ in range(int(cnt[offs[l] + c])):
                acc = F32(acc + freq[c])
            h[c] = acc
        total = F32(0)
        for c in range(Cn):
            total = F32(total + h[c])
        s = F32(smoothing)
        arg = ((h + s) / F32(total + F32(Cn) * s)).astype(F32)
        out.append(np.array([br._libm.logf(C.c_float(float(a))) for a in arg], F32))   # the host's own logf
    return out
