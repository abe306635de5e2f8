"""The recipes of the class-weighted trainer's tests (tests/test_gpu_train_prior.py).  What each one claims -- that the
weighted objective chooses other trees than the unweighted one, that a class is absent from a tree's bootstrap, that the
child-mass rule refuses a split the weighted masses would allow -- is pinned from the restatement alone in
tests/test_train_prior_cases_cpu.py, so the GPU tests compare bytes on cases known to reach those paths.

A recipe is dict(X, y, n_classes, mode, given, boosted, params); `params` are rvseg_train_params fields (for a boosted
recipe num_trees is the number of rounds)."""
import functools

import numpy as np

import boost_restate as br
import train_prior_restate as tr

F32 = np.float32


def _imbalanced_labels(rng, N, C, X, col):
    """Class 0 about nine times as frequent as each other class, tied loosely to one feature so that trees have
    something to find."""
    p = np.ones(C)
    p[0] = 9.0
    y = rng.choice(C, N, p=p / p.sum())
    rare = np.nonzero(y > 0)[0]
    X[rare, col] = X[rare, col] * F32(0.5) + F32(y[rare] % 4) * F32(30)
    return y.astype(np.int32)


def _bytes(C, N, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (N, 6)).astype(F32)
    y = _imbalanced_labels(rng, N, C, X, 2)
    X = np.floor(X)
    return dict(X=X, y=y, n_classes=C, mode=tr.INVERSE_FREQUENCY, given=None, boosted=False,
                params=dict(num_trees=2, max_depth=6, min_split_examples=10, seed=3 + C))


def _floats(N):
    """Float features only, no bootstrap: the root's segment has N elements, so the running weighted counts cross a
    64-lane chunk seam at N = 65 and 129, end on it at 64 and stop short of it at 63.  Feature 0 holds a run of equal
    values over sorted positions 61..66, on the seam."""
    rng = np.random.default_rng(100 + N)
    X = (rng.standard_normal((N, 2)) * 3).astype(F32)
    y = rng.choice(3, N, p=[0.8, 0.12, 0.08]).astype(np.int32)     # overlapping classes: the weighting moves the cuts
    X[:, 1] += (y * F32(2.5)).astype(F32)
    X[:, 0] -= ((y == 2) * F32(2)).astype(F32)
    order = np.argsort(X[:, 0], kind="stable")
    X[order[61:min(N, 67)], 0] = X[order[min(N, 67) - 1], 0]
    return dict(X=X, y=y, n_classes=3, mode=tr.INVERSE_FREQUENCY, given=None, boosted=False,
                params=dict(num_trees=1, max_depth=6, min_split_examples=4, num_features=2, use_bootstrap=0, seed=N))


def _mixed(mode, given, C, seed, **params):
    rng = np.random.default_rng(seed)
    N, D = 300, 8
    X = rng.integers(0, 256, (N, D)).astype(F32)
    X[:, D // 2:] = (rng.standard_normal((N, D - D // 2)) * 3).astype(F32)
    y = _imbalanced_labels(rng, N, C, X, 5)
    X[:, :D // 2] = np.floor(X[:, :D // 2])
    p = dict(num_trees=2, max_depth=6, min_split_examples=10, num_features=3, seed=seed)
    p.update(params)
    return dict(X=X, y=y, n_classes=C, mode=mode, given=given, boosted=False, params=p)


def _absent():
    """40 examples, class 2 has one: ABSENT_SEED's bootstraps leave it out of at least one tree, whose weight for it does
    not exist and must never be read."""
    rng = np.random.default_rng(7)
    X = rng.integers(0, 256, (40, 4)).astype(F32)
    X[:, 3] = (rng.standard_normal(40) * 2).astype(F32)
    y = (rng.random(40) < 0.3).astype(np.int32)
    y[17] = 2
    return dict(X=X, y=y, n_classes=3, mode=tr.INVERSE_FREQUENCY, given=None, boosted=False,
                params=dict(num_trees=4, max_depth=5, min_split_examples=4, num_features=2, seed=ABSENT_SEED))


ABSENT_SEED = 1   # searched on the CPU (test_train_prior_cases_cpu.py pins that it still does what it claims)


def _example_shape():
    """libforest's example (example/main.cpp:92-104): a boosted forest, no bootstrap, depth 5, the learner's defaults --
    useClassFrequency among them."""
    rng = np.random.default_rng(13)
    N, D = 300, 6
    X = rng.integers(0, 256, (N, D)).astype(F32)
    X[:, 4:] = (rng.standard_normal((N, 2)) * 3).astype(F32)
    y = _imbalanced_labels(rng, N, 3, X, 1)
    X[:, :4] = np.floor(X[:, :4])
    flip = rng.random(N) < 0.15
    y[flip] = rng.integers(0, 3, int(flip.sum()))
    return dict(X=X, y=y.astype(np.int32), n_classes=3, mode=tr.INVERSE_FREQUENCY, given=None, boosted=True,
                params=dict(num_trees=3, max_depth=5, min_split_examples=20, use_bootstrap=0, seed=17))


RECIPES = {
    "bytes_c2": lambda: _bytes(2, 300, 1),
    "bytes_c16": lambda: _bytes(16, 400, 2),
    "floats_63": lambda: _floats(63),
    "floats_64": lambda: _floats(64),
    "floats_65": lambda: _floats(65),
    "floats_129": lambda: _floats(129),
    "mixed": lambda: _mixed(tr.INVERSE_FREQUENCY, None, 4, 21),
    "absent_class": _absent,
    "given_ones": lambda: _mixed(tr.GIVEN, [1.0] * 3, 3, 22),
    "given_inexact": lambda: _mixed(tr.GIVEN, [0.1, 3.7, 1e-3], 3, 23),
    "example_shape": _example_shape,
    "min_child": lambda: _mixed(tr.INVERSE_FREQUENCY, None, 3, 24, min_child_split_examples=8, min_split_examples=4),
}
NAMES = tuple(RECIPES)


@functools.lru_cache(maxsize=None)
def recipe(name):
    return RECIPES[name]()


@functools.lru_cache(maxsize=None)
def restated(name, mode=None):
    """The restatement's result for a recipe in its own mode, or in `mode`; computed once and shared -- treat as read-only.
    dict(model = the stream, book = per tree the restatement's bookkeeping, and for a boosted recipe rounds, errors,
    alphas)."""
    r = recipe(name)
    mode = r["mode"] if mode is None else mode
    book = []
    if r["boosted"]:
        p = dict(r["params"])
        out = tr.boosted_train(r["X"], r["y"], r["n_classes"], p.pop("num_trees"), p.pop("seed"), mode=mode, given=r["given"], book=book, **p)
        out["book"] = book
        return out
    return {"model": tr.forest_train(r["X"], r["y"], r["n_classes"], mode=mode, given=r["given"], book=book, **r["params"]), "book": book}


def oracle_model(name):
    """The frozen CPU oracle's bytes for a recipe (it knows the unweighted objective only)."""
    from oracle import oracle as O
    r = recipe(name)
    if r["boosted"]:
        p = dict(r["params"])
        return br.boosted_train(r["X"], r["y"], r["n_classes"], p.pop("num_trees"), p.pop("seed"), **p)["model"]
    return O.forest_train(r["X"], r["y"], [r["n_classes"]], **r["params"])
