"""TEST INFRASTRUCTURE ONLY -- the recipes of the pruning tests (tests/test_gpu_prune.py): small forests trained by the
CPU oracle on noisy labels (shallow trees, so that they disagree), a point set, an initial state and a schedule per case,
and the restated trajectory (prune_restate) each case is compared with.  What each case claims -- the edge it crosses --
is pinned from the restatement alone in tests/test_prune_cases_cpu.py."""
import numpy as np

import boost_restate as br
import prune_restate as pr
from oracle import oracle as O

F32 = np.float32
CTX_D4 = dict(patch_size_reduce=1, feature_height=0, feature_normal=0)   # a context whose feature length is 4
SHORT = dict(start_temperature=1.0, end_temperature=0.5, alpha=0.8, inner_loops=8)   # 4 temperatures x 8 proposals
_cache = {}


def _points(seed, P, cc, noise=0.35):
    """P points of 4 byte-valued features and, per layer, a label that depends on them and is wrong `noise` of the time."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (P, 4)).astype(F32)
    labels = []
    for l, Cn in enumerate(cc):
        clean = ((X[:, l % 4] // 37).astype(np.int64) + 2 * (X[:, (l + 1) % 4] > 128) + 3 * (X[:, (l + 2) % 4] > 70)) % Cn
        flip = rng.random(P) < noise
        labels.append(np.where(flip, rng.integers(0, Cn, P), clean))
    return X, np.stack(labels, 1).astype(np.int32)


def _forest(seed, cc, T, depth=3, P_train=300):
    X, labels = _points(1000 + seed, P_train, cc, noise=0.45)
    return O.forest_train(X, labels, cc, num_trees=T, max_depth=depth, min_split_examples=8, num_features=2, use_bootstrap=1, seed=seed)


def _case(cc, T, P, state, params, forest_seed=1, point_seed=2, layer=0, multi=0, depth=3):
    X, labels = _points(point_seed, P, cc)
    return dict(blob=_forest(forest_seed, cc, T, depth), ctx=dict(CTX_D4, multi_layer=multi), multi=multi, layer=layer, C=cc[layer], T=T, X=X,
                labels=np.ascontiguousarray(labels[:, layer]), state=list(state), params=dict(params))


def case(name):
    """name -> dict(blob, ctx, multi, layer, C, T, X (P, 4), labels (P,), state, params = fields of rvseg_prune_params)."""
    if name in _cache:
        return _cache[name]
    if name == "main":            # each step kind, a step with improvement == 0, a best state that is not the first
        c = _case([4], 8, 4097, [0, 1, 2], dict(SHORT, seed=3), depth=2)
    elif name == "moves":         # all three moves from a one-tree state: remove meets its floor
        c = _case([4], 6, 65, [2], dict(SHORT, p_exchange=0.5, p_remove=0.25, p_add=0.25, seed=2))
    elif name == "cap":           # 63 entries: add meets the cap of 64
        c = _case([3], 7, 64, [t % 7 for t in range(63)], dict(SHORT, p_exchange=0.25, p_remove=0.25, p_add=0.5, seed=1))
    elif name == "duplicates":
        c = _case([4], 6, 63, [0, 0, 3, 3, 5], dict(SHORT, seed=2))
    elif name == "bad_labels":    # labels of -1 and C are errors whatever the vote
        c = _case([4], 6, 1000, [0, 1, 2, 3], dict(SHORT, seed=4))
        c["labels"][::7] = -1
        c["labels"][3::11] = 4
    elif name == "layer1":        # layer 1 of a two-layer forest on a multi_layer context
        c = _case([3, 5], 6, 1000, [0, 1, 2], dict(SHORT, seed=5), layer=1, multi=1)
    elif name == "single_class":
        c = _case([1], 6, 65, [0, 1], dict(SHORT, seed=6))
    elif name == "c16_state64":   # 16 byte counters, each able to reach 64
        c = _case([16], 8, 65, [t % 8 for t in range(64)], dict(SHORT, seed=7), depth=5)
    elif name == "tie":           # an even state: two labels tie and the first to reach the maximum wins
        c = _case([4], 8, 1000, [5, 1, 6, 2], dict(SHORT, seed=8), depth=2)
    elif name == "no_iterations":   # start <= end: the initial state comes back with its energy
        c = _case([4], 6, 64, [1, 4], dict(SHORT, start_temperature=0.5, seed=9))
    elif name == "cover":
        c = _case([4], 8, 1000, [0, 1], dict(SHORT, p_exchange=0.5, p_remove=0.25, p_add=0.25, energy=pr.COVER, seed=10))
    else:
        raise KeyError(name)
    _cache[name] = c
    return c


CASES = ["main", "moves", "cap", "duplicates", "bad_labels", "layer1", "single_class", "c16_state64", "tie", "no_iterations", "cover"]


def votes(name):
    """(T, P) uint8: every tree's own label of the case's layer, through the CPU oracle's evaluator on one-tree files."""
    key = ("votes", name)
    if key not in _cache:
        c = case(name)
        whole = O.Forest(c["blob"])
        cc = whole.classes(bool(c["multi"]))
        off = int(np.sum(cc[:c["layer"]]))
        assert cc[c["layer"]] == c["C"]
        _cache[key] = np.stack([br.first_strict_max(O.Forest(br.one_tree_forest(tree)).eval(c["X"], bool(c["multi"]))[:, off:off + c["C"]]).astype(np.uint8)
                                for tree in br.split_trees(c["blob"])])
        assert _cache[key].shape == (c["T"], c["X"].shape[0])
    return _cache[key]


def agreement(name):
    v = votes(name)
    return np.stack([(v == v[t]).sum(1) for t in range(v.shape[0])]).astype(np.uint64)


def energy_of(name):
    """The case's energy as a function of a state."""
    c, v = case(name), votes(name)
    if c["params"].get("energy", pr.ERROR) == pr.COVER:
        agree = agreement(name)
        return lambda state: pr.cover_energy(agree, v.shape[1], state)
    return lambda state: pr.error_energy(v, c["labels"], state)


def restated(name):
    """The restated run of the case, computed once."""
    key = ("run", name)
    if key not in _cache:
        c = case(name)
        _cache[key] = pr.run(c["params"], c["T"], c["state"], energy_of(name))
    return _cache[key]
