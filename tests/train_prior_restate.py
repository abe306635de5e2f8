"""TEST INFRASTRUCTURE ONLY -- a Python restatement of the single-layer depth-first learner with the class-weighted split
objective (libforest DecisionTreeLearner::learn, learning.cpp:664-916), written in numpy float32 from those lines, from
definitions 1-4 in the header of oracle/rvseg_oracle_train.c and from the definitions of rvseg_class_prior in
include/rvseg.h, independently of the HIP code.  oracle/ is frozen, so the weighted objective has no C oracle: in mode NONE
this file must reproduce orc_forest_train's bytes (tests/test_train_prior_cases_cpu.py), after which the two differ in the
objective alone.

Every fp32 operation is one numpy float32 operation, so each product and sum is rounded on its own (no FMA).  logf comes
from libm through ctypes, as in boost_restate.py.  The forest.dat stream is written here, byte by byte."""
import ctypes as C
import struct

import numpy as np

import boost_restate as B
from boost_restate import draw64, mix64

F32 = np.float32
NONE, INVERSE_FREQUENCY, GIVEN = 0, 1, 2


# ---- the objective ---------------------------------------------------------------------------------------------------
def fastlog2(x):
    """fastlog.h:47-58 on a float32 array, in the oracle's operation order."""
    x = np.ascontiguousarray(x, F32)
    vi = x.view(np.uint32)
    mx = ((vi & np.uint32(0x007FFFFF)) | np.uint32(0x3F000000)).view(F32)
    y = vi.astype(F32)
    y = y * F32(1.1920928955078125e-7)
    a = F32(1.498030302) * mx
    den = F32(0.3520887068) + mx
    b = F32(1.72587999) / den
    r = y - F32(124.22551499)
    r = r - a
    r = r - b
    return r


def entropy_term(p):
    """ENTROPY(p) = -(p) * fastlog2(p), learning.cpp:13"""
    p = np.ascontiguousarray(p, F32)
    return (-p) * fastlog2(p)


def side_entropy(counts, weights):
    """E of one side for every row of the integer matrix counts [n, C].  weights None: oracle definition 2 (the integer
    expression); else rvseg_class_prior definition 2.  A weight is read only where the count is not zero."""
    counts = np.asarray(counts, np.int64)
    n, Cn = counts.shape
    if weights is None:
        total = -entropy_term(counts.sum(axis=1).astype(F32))
        for c in range(Cn):
            has = counts[:, c] > 0
            total[has] = total[has] + entropy_term(counts[has, c].astype(F32))
        return total
    mass = np.zeros(n, F32)
    for c in range(Cn):
        has = counts[:, c] > 0
        mass[has] = mass[has] + weights[c] * counts[has, c].astype(F32)
    total = -entropy_term(mass)
    for c in range(Cn):
        has = counts[:, c] > 0
        total[has] = total[has] + entropy_term(weights[c] * counts[has, c].astype(F32))
    return total


def tree_weights(mode, given, cnt):
    """definition 1: the weights of a tree from the class counts of its data set after the bootstrap.  A class the set
    does not hold gets NaN here, so that reading it would show in the objective."""
    if mode == NONE:
        return None
    cnt = np.asarray(cnt, np.int64)
    w = np.full(len(cnt), np.nan, F32)
    has = cnt > 0
    if mode == GIVEN:
        w[has] = np.asarray(given, F32)[has]
    else:
        w[has] = F32(cnt.sum()) / cnt[has].astype(F32)
    return w


# ---- one tree ----------------------------------------------------------------------------------------------------------
def _logf(x):
    return F32(B._libm.logf(C.c_float(float(x))))


def _grow(X, y, Cn, mult, key_root, K, max_depth, min_split, min_child, weights, refused):
    """Depth-first over an explicit stack (:664-916).  Returns (feat, thr, left) in the reference's node numbering.
    refused receives, per best cut the child-mass rule turned down, (left counts, right counts)."""
    P, D = X.shape
    feat, thr, left, depth, keys = [0], [F32(0)], [0], [0], [key_root]
    examples = {0: np.nonzero(mult)[0]}
    stack = [0]
    while stack:
        node = stack.pop()
        ex = examples.pop(node)
        key = keys[node]
        hist = np.bincount(y[ex], weights=mult[ex], minlength=Cn).astype(np.int64)
        mass = int(hist.sum())
        if mass < min_split or np.count_nonzero(hist) <= 1 or depth[node] > max_depth:     # :773 and its neighbours
            continue
        perm = list(range(D))
        for k in range(min(K, D)):
            j = k + draw64(key, 1 + k) % (D - k)
            perm[k], perm[j] = perm[j], perm[k]
        best = (F32(1e35), -1, F32(0), F32(0), None)  # objective, feature, left value, right value, left counts
        for k in range(min(K, D)):
            f = perm[k]
            order = np.lexsort((ex, X[ex, f]))
            idx = ex[order]
            v = X[idx, f]
            if len(idx) < 2:
                continue
            onehot = np.zeros((len(idx), Cn), np.int64)
            onehot[np.arange(len(idx)), y[idx]] = mult[idx]
            lh = np.cumsum(onehot, axis=0)[:-1]          # the counts left of position m = 1 .. n-1
            rh = hist[None, :] - lh
            cand = ~((v[1:] - v[:-1]) < F32(1e-6))        # :578-585
            if not cand.any():
                continue
            obj = np.full(len(idx) - 1, F32(1e35), F32)
            obj[cand] = side_entropy(lh[cand], weights) + side_entropy(rh[cand], weights)
            m = int(np.argmin(obj))                       # the first minimum: strict '<' in ascending order
            if obj[m] < best[0]:
                best = (obj[m], f, v[m], v[m + 1], lh[m].copy())
        obj, f, lv, rv, lcounts = best
        if f < 0:
            continue
        lm = int(lcounts.sum())
        th = F32(F32(lv + rv) * F32(0.5))
        if not (lv < th and th <= rv):
            th = rv
        if lm < min_child or mass - lm < min_child:       # the unweighted masses, :842-843
            refused.append((lcounts, hist - lcounts))
            continue
        lc = len(feat)
        for side in (0x4C, 0x52):
            feat.append(0)
            thr.append(F32(0))
            left.append(0)
            depth.append(depth[node] + 1)
            keys.append(mix64(key ^ side))
        goes_left = X[ex, f] < th
        examples[lc], examples[lc + 1] = ex[goes_left], ex[~goes_left]
        feat[node], thr[node], left[node] = f, th, lc
        stack += [lc, lc + 1]
    return np.asarray(feat, np.int32), np.asarray(thr, F32), np.asarray(left, np.int32)


def _leaf_rows(X, y, Cn, feat, thr, left, smoothing):
    """updateHistograms (:918-958 / :960-1012) over ALL examples: per leaf log((h + s) / (total + C s))."""
    P = X.shape[0]
    node = np.zeros(P, np.int64)
    while True:
        inner = left[node] != 0
        if not inner.any():
            break
        i = np.nonzero(inner)[0]
        go_left = X[i, feat[node[i]]] < thr[node[i]]
        node[i] = np.where(go_left, left[node[i]], left[node[i]] + 1)
    with np.errstate(divide="ignore"):
        freq = F32(P) / np.bincount(y, minlength=Cn).astype(F32)
    rows = {}
    for v in np.nonzero(left == 0)[0]:
        cnt = np.bincount(y[node == v], minlength=Cn)
        h = np.zeros(Cn, F32)
        for c in range(Cn):
            acc = F32(0)
            for _ in range(int(cnt[c])):
                acc = F32(acc + freq[c])
            h[c] = acc
        total = F32(0)
        for c in range(Cn):
            total = F32(total + h[c])
        den = F32(total + F32(F32(Cn) * F32(smoothing)))
        with np.errstate(divide="ignore"):
            rows[int(v)] = np.asarray([_logf(F32(F32(h[c] + F32(smoothing)) / den)) for c in range(Cn)], F32)
    return rows


def forest_train(X, y, n_classes, mode=NONE, given=None, num_trees=4, max_depth=30, min_split_examples=50,
                 min_child_split_examples=1, num_features=0, use_bootstrap=1, smoothing=1.0, seed=1, book=None):
    """The single-layer forest.dat bytes.  book (a list, optional) receives per tree dict(cnt = class counts after the
    bootstrap, weights, root = (feature, threshold) or None, refused = the cuts the child-mass rule turned down)."""
    X = np.ascontiguousarray(X, F32)
    y = np.asarray(y, np.int64).reshape(-1)
    P, D = X.shape
    K = num_features if num_features > 0 else int(np.ceil(np.sqrt(float(D))))
    out = [struct.pack("<i", num_trees)]
    for t in range(num_trees):
        kt = mix64(seed ^ mix64(0x74726565 + t))
        if use_bootstrap:
            mult = np.zeros(P, np.int64)
            for n in range(P):
                mult[draw64(kt, 0x100000000 + n) % P] += 1
        else:
            mult = np.ones(P, np.int64)
        cnt = np.bincount(y, weights=mult, minlength=n_classes).astype(np.int64)
        weights = tree_weights(mode, given, cnt)
        refused = []
        feat, thr, left = _grow(X, y, n_classes, mult, mix64(kt ^ 0x726F6F74), K, max_depth, min_split_examples,
                                min_child_split_examples, weights, refused)
        if book is not None:
            book.append({"cnt": cnt, "weights": weights, "root": (int(feat[0]), thr[0]) if left[0] else None, "refused": refused})
        rows = _leaf_rows(X, y, n_classes, feat, thr, left, smoothing)
        nn = len(feat)
        out += [struct.pack("<i", nn), feat.tobytes(), struct.pack("<i", nn), thr.tobytes(), struct.pack("<i", nn), left.tobytes()]
        for multi in (False, True):                    # `histograms`, then `multi_histograms` with its one layer
            out.append(struct.pack("<i", nn))
            for v in range(nn):
                if left[v] != 0:
                    out.append(struct.pack("<i", 0))
                    continue
                if multi:
                    out.append(struct.pack("<i", 1))
                out += [struct.pack("<i", n_classes), rows[v].tobytes()]
    return b"".join(out)


# ---- boosting rounds over that learner (boost_restate.boosted_train with the tree learner exchanged) ---------------
def boosted_train(X, y, n_classes, rounds, seed, mode=NONE, given=None, book=None, **tree_params):
    X = np.ascontiguousarray(X, F32)
    y = np.asarray(y, np.int32).reshape(-1)
    N = X.shape[0]
    w = np.full(N, F32(1) / F32(N), F32)
    cumsum = (np.arange(1, N + 1).astype(F32) * F32(1)) / F32(N)
    trees, weights = [], []
    errors = np.full(rounds, np.nan, F32)
    alphas = np.full(rounds, np.nan, F32)
    for r in range(rounds):
        kb = B.round_key(seed, r)
        idx = B.pick(cumsum, B.uniforms(kb, N))
        forest = forest_train(X[idx], y[idx], n_classes, mode=mode, given=given, num_trees=1, seed=B.tree_seed(kb), book=book,
                              **tree_params)
        (tree,) = B.split_trees(forest)
        miss = B.tree_votes(tree, X) != y
        error = B.serial_sum(w[miss])
        errors[r] = error
        if not error < 1:
            break
        alpha = B.alpha_of(error, n_classes)
        if error == 0:
            alphas[r] = alpha
            trees.append(tree)
            weights.append(alpha)
            break
        _, total, w2, cumsum2 = B.weight_round(w, miss, B.exp_of(alpha))
        if w2 is None:
            break
        alphas[r] = alpha
        trees.append(tree)
        weights.append(alpha)
        w, cumsum = w2, cumsum2
    return {"model": B.boosted_stream(trees, weights), "rounds": len(trees), "errors": errors, "alphas": alphas}
