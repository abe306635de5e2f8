"""TEST INFRASTRUCTURE ONLY -- the recipes of the limit tests of the forest tools, the pruning and the boosted models
(tests/test_gpu_tools_limits.py, test_gpu_prune_limits.py, test_gpu_boosted_limits.py) and their restated values.  What
each recipe claims -- the edge it sits on -- is pinned from the restatement alone in tests/test_limits_tools_cases_cpu.py.

The switches of the code the recipes are built around (csrc/kernels_forest_tools.hip, kernels_prune.hip,
rvseg_forest_tools.hip, rvseg_prune.hip):
  tools_votes_kernel   4 lanes per point up to 4 trees, 16 from 5; tree t in lane t % lanes, slot t / lanes; class c summed
                       by lane c % lanes in pass c / lanes, then a cross-lane reduction that prefers the lower class
  tools_agree_kernel   tiles of 512 points, four tiles per block, the T (T + 1) / 2 pairs decoded per thread
  tools_confusion      C x C counters in LDS, C <= 64
  tools_refit_count    a grid of 4 blocks of 256 per compute unit that loops over the T x n (tree, point) pairs
  prune_step_kernel    1024 points per block, four of a lane per 32-bit load, a grid of 4 blocks per compute unit
  TOOLS_CHUNK          65536 points of X on the device at a time
Trees of the distinct forests differ in every split and every leaf row, so that no tree stands in for another."""
import numpy as np

import boost_restate as br
import frame_cases as fc
import prune_cases as pc
import prune_restate as pr
import tools_cases as tc
from oracle import oracle as O

F32 = np.float32
CHUNK_TAIL = tc.CHUNK_TAIL                      # one chunk and a ragged tail
CTX_D6 = dict(width=64, height=48, patch_size=9, patch_size_reduce=1)      # the 6-feature context of test_gpu_forest_limits
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- forests of distinct trees ---------------------------------------------------------------------------------------
_SEED_STEPS = {(3, 17): 3, (5, 17): 1}          # 24 or 40 leaves over 17 classes: the first seeds whose forests predict class 16


def _seed(T, S):
    """7 T + S, or the first of 7 T + S + 1000 k under which the forest reaches what its case is for (pinned on the CPU)."""
    return 7 * T + S + 1000 * _SEED_STEPS.get((T, S), 0)


def distinct(T, S):
    """The forest.dat image of T distinct complete trees of 8 leaves, one layer of S classes, over 6 features."""
    return _once(("distinct", T, S), lambda: fc.small_forest(_seed(T, S), T, S, fc.EVAL_D)[1])


def points(P, seed=11):
    """Byte-valued points; a shorter set is a prefix of a longer one of the same seed."""
    return fc.eval_points(seed, P) if P > CHUNK_TAIL else _once(("points", seed), lambda: fc.eval_points(seed, CHUNK_TAIL))[:P]


def restated(T, S, P):
    """tools_cases.restate_blob of distinct(T, S) on points(P): dict(pred, votes, C)."""
    return _once(("restated", T, S, P), lambda: tc.restate_blob(distinct(T, S), points(P), True))


VOTE_CASES = sorted({(T, 5) for T in fc.EVAL_TREES} | {(T, S) for S in fc.CLASS_SUMS for T in (3, 5, 17)} | {(4, 17), (17, 17)})
POINT_COUNT_FORESTS = ((4, 17), (17, 17))       # every P of frame_cases.POINT_COUNTS
VOTE_P = 257

TWO_LAYERS = (5, 17)


def two_layer_forest():
    """17 trees with two label layers of 5 and 17 classes over the default 366 features."""
    from rovinasemanticsegmentation_amd import synthetic
    return _once("two_layer", lambda: synthetic.make_forest_bytes(n_trees=17, leaves_per_tree=8, max_depth=4, single_classes=0,
                                                                  layer_classes=TWO_LAYERS))


def two_layer_restated(layer, P=VOTE_P):
    return _once(("two_layer", layer, P), lambda: tc.restate_blob(two_layer_forest(), tc.points(366, P), True, layer))


# ---- agreement -------------------------------------------------------------------------------------------------------
AGREE_TREES = (1, 2, 5, 16, 17, 23, 64)         # at P = 513
AGREE_POINTS = (1, 3, 4, 5, 511, 512, 513, 2047, 2048, 2049)    # at T = 17: the word and the 512-point tile edges
AGREE_CASES = sorted({(T, 513) for T in AGREE_TREES} | {(17, P) for P in AGREE_POINTS} | {(64, 2049), (17, CHUNK_TAIL)})


def agree_classes(T):
    """The class count of the agreement forest of T trees."""
    return 64 if T == 64 else 17


# ---- confusion -------------------------------------------------------------------------------------------------------
CONFUSION_CLASSES = (1, 2, 16, 17, 63, 64)
CONFUSION_POINTS = (1, 2049)
CONFUSION_T = 3


def confusion_labels(pred, C):
    """tools_cases.labels_for with class 0 at the first and class C - 1 at the last point."""
    lab = tc.labels_for(pred, C) if C > 1 else np.zeros(len(pred), np.int32)
    lab[0] = 0
    lab[-1] = C - 1
    return lab


# ---- refit -----------------------------------------------------------------------------------------------------------
REFIT_CASES = ((5, 3, CHUNK_TAIL), (64, 3, 4097))      # (T, S, P): T * min(P, 65536) > 4 * 256 * 256 on a 256-CU device


def refit_labels(P, S, seed=13):
    return np.random.default_rng(seed).integers(0, S, (P, 1)).astype(np.int32)


# ---- the tie and NaN rule on the wide paths ----------------------------------------------------------------------------
TIE_C = 20
TIE_P = 1000


def _row(base=0.0, **at):
    row = np.full(TIE_C, base, F32)
    for k, v in at.items():
        row[int(k[1:])] = v
    return row


def _tie_trees(features):
    """Three hand-written trees over D = 4 with 20 single-label classes, splitting on `features` = (A's root, A's second
    level, B, C).  A has four leaves, B and C are stumps; every tree's leaves sum with the others' to

      A0 + B0 + C0   3 and 19 tie at 2 (1.5 + 0.5 = 0.5 + 1.5), 5 and 18 stay below: 3 wins
      A1 + B0 + C0   5 and 18 tie at 2, 3 and 19 stay below: 5 wins
      A2 + B0 + C0   a NaN at class 0 under finite classes: label 0
      A. + B0 + C1   the same with a NaN at class 16 alone, which never wins
      A0..2 + B1     every class -inf (with the NaNs of A2 and C1 where they are): all equal, label 0
      A3 + B1        +inf - inf at class 7: every class -inf except a NaN, label 0
      A3 + B0        +inf at class 7: 7 wins

    (Three stumps have eight sums, and a leaf of -inf takes half of them: A needs its four leaves.)"""
    nan, inf = np.nan, np.inf
    fa, fa2, fb, fc_ = features
    a = tc._tree([fa, fa2, fa2, 0, 0, 0, 0], [128, 100, 150, 0, 0, 0, 0], [1, 3, 5, 0, 0, 0, 0],
                 [[], [], [], _row(c3=1.5, c19=0.5), _row(c5=1.5, c18=0.5), _row(c0=nan), _row(c7=inf)])
    b = tc._tree([fb, 0, 0], [160, 0, 0], [1, 0, 0], [[], _row(c3=0.5, c19=1.5, c5=0.5, c18=1.5), _row(-inf)])
    c = tc._tree([fc_, 0, 0], [200.5, 0, 0], [1, 0, 0], [[], _row(), _row(c16=nan)])
    return [a, b, c]


def tie_forest(T):
    """T = 3: the 4-lane path, five class passes.  T = 6: the 16-lane path, two passes; trees 3..5 carry the same leaf
    rows behind other split features, so all six route the points differently."""
    assert T in (3, 6)
    trees = _tie_trees((0, 1, 2, 3)) + (_tie_trees((3, 2, 0, 1)) if T == 6 else [])
    return dict(blob=tc.forest_of(trees), ctx=dict(tc.TINY_CTX, multi_layer=0), D=4)


def tie_sums(T, P=TIE_P):
    """The forest's posterior sums (P, 20) on tools_cases.points(4, P), from the CPU oracle."""
    return _once(("tie_sums", T, P), lambda: O.Forest(tie_forest(T)["blob"]).eval(tc.points(4, P), False))


def tie_restated(T, P=TIE_P):
    return _once(("tie", T, P), lambda: tc.restate_blob(tie_forest(T)["blob"], tc.points(4, P), False))


def tie_outcomes(sums):
    """name -> the points (a mask) on which the sums show the named outcome."""
    nans = np.isnan(sums)
    with np.errstate(invalid="ignore"):
        top = np.nanmax(np.where(nans, -np.inf, sums), 1, keepdims=True)
        at_top = (sums == top) & ~nans
        clean = ~nans.any(1)
        finite_top = np.isfinite(top[:, 0])

        def tie(lo, hi):
            return clean & finite_top & at_top[:, lo] & at_top[:, hi] & (at_top.sum(1) == 2)
        others_neg_inf = (np.where(nans, -np.inf, sums) == -np.inf).all(1)
        return dict(tie_3_19=tie(3, 19), tie_5_18=tie(5, 18),
                    nan_at_0=nans[:, 0] & finite_top,
                    nan_at_16_only=nans[:, 16] & (nans.sum(1) == 1) & finite_top,
                    neg_inf_but_a_nan=others_neg_inf & nans.any(1) & ~nans[:, 0],
                    all_equal=clean & (at_top.sum(1) == TIE_C))


TIE_LABELS = dict(tie_3_19=3, tie_5_18=5, nan_at_0=0, neg_inf_but_a_nan=0, all_equal=0)   # (nan_at_16_only: any but 16)


# ---- pruning ---------------------------------------------------------------------------------------------------------
PRUNE_SMALL_POINTS = (1, 2, 3, 4, 5, 1023, 1024, 1025)      # a lane's four points, a block's 1024
PRUNE_CHAIN_POINTS = (1, 3, 1025)
PRUNE_T, PRUNE_C = 6, 4
_CHAIN_SEEDS = {1: 2, 3: 1, 1025: 3, CHUNK_TAIL: 3}     # (test_limits_tools_cases_cpu.py: every step kind, every move)


def prune_forest():
    return _once("prune_forest", lambda: pc._forest(1, [PRUNE_C], PRUNE_T))


def prune_points(P, seed=21):
    """(X (P, 4), labels (P,)): a prefix of one set, so that the votes of a longer set hold those of a shorter."""
    X, labels = _once(("prune_points", seed), lambda: pc._points(seed, CHUNK_TAIL, [PRUNE_C]))
    return X[:P], np.ascontiguousarray(labels[:P, 0])


def _votes_of(blob, X, multi=False):
    return np.stack([br.first_strict_max(O.Forest(br.one_tree_forest(tree)).eval(X, multi)).astype(np.uint8) for tree in br.split_trees(blob)])


def prune_votes(P):
    return _once("prune_votes", lambda: _votes_of(prune_forest(), prune_points(CHUNK_TAIL)[0]))[:, :P]


def prune_states(T):
    return [[0], [T - 1], list(range(T)), [(5 * k + 3) % T for k in range(64)]]


def prune_label_sets(P):
    """The labels as they are, with -1 and with C at the last point."""
    labels = prune_points(P)[1]
    out = [labels]
    for bad in (-1, PRUNE_C):
        lab = labels.copy()
        lab[-1] = bad
        out.append(lab)
    return out


def prune_chain(P):
    """dict(X, labels, state, params, T, votes) of the SHORT chain at P points on the 6-tree forest; the labels carry a -1
    and a C where there is room."""
    X, labels = prune_points(P)
    labels = labels.copy()
    if P > 4:
        labels[P // 2] = -1
        labels[-1] = PRUNE_C
    return dict(X=X, labels=labels, state=[0, 1, 2], T=PRUNE_T, votes=prune_votes(P),
                params=dict(pc.SHORT, p_exchange=0.5, p_remove=0.25, p_add=0.25, seed=_CHAIN_SEEDS[P]))


WIDE_T, WIDE_C, WIDE_P = 64, 16, 257
WIDE_STATE = [63, 16, 0, 5, 17, 31, 32, 33, 47, 48, 2, 9, 20, 40, 62]
COVER_P = 2049


def wide_forest():
    """64 distinct trees of depth 3 on 16 classes, trained by the CPU oracle on bootstrap samples."""
    return _once("wide_forest", lambda: pc._forest(3, [WIDE_C], WIDE_T, depth=3))


def wide_points(P):
    X, labels = _once("wide_points", lambda: pc._points(23, COVER_P, [WIDE_C]))
    return X[:P], np.ascontiguousarray(labels[:P, 0])


def wide_votes(P):
    return _once("wide_votes", lambda: _votes_of(wide_forest(), wide_points(COVER_P)[0]))[:, :P]


def wide_chain():
    X, labels = wide_points(WIDE_P)
    return dict(X=X, labels=labels, state=list(WIDE_STATE), T=WIDE_T, votes=wide_votes(WIDE_P),
                params=dict(pc.SHORT, p_exchange=0.25, p_remove=0.25, p_add=0.5, seed=2))


def error_energy(votes, labels, state, n_classes=16):
    """prune_restate.error_energy with counters for the classes the votes can name alone (it keeps 256 per point)."""
    errors = int((pr.predictions(votes, state, n_classes=n_classes) != np.asarray(labels, np.int64)).sum())
    return F32(F32(min(errors, 1 << 24)) / F32(np.asarray(votes).shape[1]))


def chain_restated(c):
    return pr.run(c["params"], c["T"], c["state"], lambda state: error_energy(c["votes"], c["labels"], state))


def added_trees(c, run):
    """The tree index of every `add` move of the run that had room to add."""
    key = pr.prune_key(c["params"]["seed"])
    return [pr.draw(key, s, 1) % c["T"] for s, (kind, n) in enumerate(run["moves"]) if kind == pr.ADD and n < pr.MAX_STATE]


# the grid-stride loop of prune_step_kernel: more than 4 x CUs x 1024 points
STRIDE_T, STRIDE_C = 3, 4
STRIDE_BLOCK = 4099                              # no multiple of 4: every tile starts at another byte of a vote word
STRIDE_STATES = ([0], [2, 1], [1, 0, 2, 1])


def stride_point_count(cus):
    return 4 * cus * 1024 + 1029


def stride_forest():
    return _once("stride_forest", lambda: pc._forest(5, [STRIDE_C], STRIDE_T, depth=2))


def stride_case(cus):
    """dict(X (P, 4), labels (P,), energy = state -> the restated energy): X tiles a block of 4099 points, so the restated
    votes are the block's, tiled; the labels are drawn over all P points and do not repeat."""
    P = stride_point_count(cus)
    Xb, lb = pc._points(29, STRIDE_BLOCK, [STRIDE_C])
    votes = _votes_of(stride_forest(), Xb)
    rng = np.random.default_rng(31)
    labels = np.resize(lb[:, 0], P).astype(np.int32)
    flip = rng.random(P) < 0.2
    labels[flip] = rng.integers(0, STRIDE_C, int(flip.sum()))
    labels[-1] = STRIDE_C                          # and a label out of range at the very end
    X = np.ascontiguousarray(np.resize(Xb, (P, 4)))

    def energy(state):
        pred = np.resize(pr.predictions(votes, state, n_classes=STRIDE_C), P)
        return F32(F32(min(int((pred != labels).sum()), 1 << 24)) / F32(P))
    return dict(X=X, labels=labels, energy=energy, P=P, votes=votes)


# ---- boosted models ----------------------------------------------------------------------------------------------------
BOOSTED_CASES = ((1, 2), (5, 17), (17, 64), (64, 16))      # (T, C)
BOOSTED_WEIGHTS = ("ones", "rising", "mixed")
BOOSTED_P = 257
CTX_D6_SINGLE = dict(CTX_D6, multi_layer=0)


def boosted_trees(T, Cn):
    """The trees of a distinct forest with their leaf rows as single-label histograms, each as its own bytes."""
    def make():
        out = []
        for t in fc.small_forest(_seed(T, Cn), T, Cn, fc.EVAL_D)[0]:
            rows = iter(t["rows"])
            out.append(tc._tree(t["feat"], t["thr"], t["left"], [next(rows) if l == 0 else [] for l in t["left"]]))
        return out
    return _once(("boosted_trees", T, Cn), make)


def boosted_weights(which, T):
    if which == "ones":                             # every vote counts alike: ties wherever two labels have as many votes
        return np.ones(T, F32)
    if which == "rising":
        return (F32(0.25) * np.arange(1, T + 1)).astype(F32)
    mixed = (np.inf, -0.25, -0.0, 1.5, 0.75, -2.0, 3.0)
    return np.asarray([mixed[t % len(mixed)] for t in range(T)], F32)


def boosted_restated(T, Cn, which, P=BOOSTED_P):
    """dict(stream, sums (P, C), pred (P,), votes (T, P)) of the boosted model of boosted_trees(T, C) under the weights."""
    def make():
        trees, w, X = boosted_trees(T, Cn), boosted_weights(which, T), points(P)
        votes = _once(("boosted_votes", T, Cn, P), lambda: [br.tree_votes(tree, X) for tree in trees])
        sums = br.vote_sums(trees, w, X, Cn, labels=votes)
        with np.errstate(invalid="ignore"):
            pred = br.first_strict_max(sums)
        return dict(stream=br.boosted_stream(trees, w), sums=sums, pred=pred, votes=np.stack(votes).astype(np.uint8), weights=w)
    return _once(("boosted", T, Cn, which, P), make)
