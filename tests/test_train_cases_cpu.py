"""CPU pins of the trainer recipes (tests/train_cases.py): the oracle learner ALONE, run on every recipe, must show
that the recipe crosses the edge it was built for -- level widths for the slot batches, the root threshold for seams
and the threshold guard, node counts for the degenerate sets -- so that test_gpu_train_limits.py compares trees that
really exercise those paths.  The evidence is read from the oracle's forest.dat, never from the code under test; the
only product code used here is the host-side validator rvseg_forest_check and nothing needs a GPU."""
import numpy as np
import pytest

import train_cases as tc


def _checked(oracle, c):
    import rovinasemanticsegmentation_amd as rv
    blob = tc.train(oracle, c)
    st, msg, info = rv.capi.forest_check(blob, c["X"].shape[1])
    assert st == rv.capi.OK, msg
    oracle.Forest(blob)                       # the oracle's own loader reads it as well
    return tc.parse(blob)


def test_every_recipe_trains_to_a_valid_file(oracle):
    for name, make in tc.all_cases().items():
        c = make()
        trees = _checked(oracle, c)
        assert len(trees) == c["kw"].get("num_trees", 4), name
        for t in trees:
            for n in np.flatnonzero(t["left"] == 0):
                assert [len(h) for h in t["mhist"][n]] == c["cc"], name


def test_slot_batch_recipes_cross_1024_and_2048(oracle):
    t = _checked(oracle, tc.slot_batches())[0]
    w = tc.level_widths(t)
    assert w.max() > tc.SLOT_BATCH and (w > tc.SLOT_BATCH).sum() >= 3, w.tolist()
    assert w.max() <= 2 * tc.SLOT_BATCH                      # two batches, the three-batch recipe is the next one
    t = _checked(oracle, tc.slot_batches_three())[0]
    w = tc.level_widths(t)
    assert w.max() > 2 * tc.SLOT_BATCH and (w > 2 * tc.SLOT_BATCH).sum() >= 3, w.tolist()
    # below the edge: the same recipe, shallower, stays inside one batch
    w = tc.level_widths(_checked(oracle, tc.slot_batches(P=20000, max_depth=12))[0])
    assert w.max() <= tc.SLOT_BATCH


@pytest.mark.parametrize("cc", tc.LAYOUTS, ids=lambda cc: "_".join(map(str, cc)))
def test_layout_recipes_reach_the_last_class(oracle, cc):
    assert 1 <= len(cc) <= tc.MAX_LAYERS and max(cc) <= tc.TR_CMAX and sum(cc) <= 64
    c = tc.layout(cc, seed=tc.LAYOUTS.index(cc))
    for l, C in enumerate(cc):
        assert c["labels"][:, l].max() == C - 1 and c["labels"][:, l].min() == 0
    trees = _checked(oracle, c)
    if cc != [1]:
        assert max(len(t["left"]) for t in trees) > 1
    # an absent class holds the smallest value of its histogram in every leaf: the last class must beat it somewhere
    for l, C in enumerate(cc):
        if C == 1:
            continue
        assert any(t["mhist"][n][l][C - 1] > t["mhist"][n][l].min() for t in trees for n in np.flatnonzero(t["left"] == 0)), l


def test_layout_list_covers_the_limits():
    flat = [C for cc in tc.LAYOUTS for C in cc]
    assert {1, 2, 9, 15, 16} <= set(flat)
    assert {len(cc) for cc in tc.LAYOUTS} == set(range(1, 9))
    assert [16] * 4 in tc.LAYOUTS and [8] * 8 in tc.LAYOUTS
    assert max(sum(cc) for cc in tc.LAYOUTS) == 64
    for cc in tc.REFUSED_LAYOUTS:
        assert max(cc) > tc.TR_CMAX or len(cc) > tc.MAX_LAYERS or sum(cc) > 64


def _is_byte_column(x):
    return bool(np.all((x >= 0) & (x <= 255) & (x == np.floor(x))))


def test_feature_kind_recipes(oracle):
    c = tc.all_bytes()
    assert all(_is_byte_column(c["X"][:, f]) for f in range(c["X"].shape[1]))
    assert len(_checked(oracle, c)[0]["left"]) > 100
    c = tc.all_floats()
    assert not any(_is_byte_column(c["X"][:, f]) for f in range(c["X"].shape[1])) and c["kw"]["num_features"] == c["X"].shape[1]
    t = _checked(oracle, c)[0]
    assert len(t["left"]) > 100 and len(set(t["feat"][t["left"] != 0])) > 1
    for kind in ("byte", "float"):
        c = tc.single_feature(kind)
        assert c["X"].shape[1] == 1 and _is_byte_column(c["X"][:, 0]) == (kind == "byte")
        assert len(_checked(oracle, c)[0]["left"]) > 50


@pytest.mark.parametrize("kind", list(tc.BYTE_EDGES))
def test_byte_detection_edges_are_where_the_oracle_cuts(oracle, kind):
    c = tc.byte_edge(kind)
    x = c["X"][:, 0]
    assert _is_byte_column(x) == (kind in ("0_255", "-0.0"))          # what the trainer's detection must conclude
    assert _is_byte_column(c["X"][:, 1]) and not _is_byte_column(c["X"][:, 2])
    t = _checked(oracle, c)[0]
    inner = t["left"] != 0
    want = tc.BYTE_EDGES[kind]
    if want is None:     # -0.0 == 0.0: nothing to cut, however the zeros are signed
        assert len(t["left"]) > 1 and not np.any(t["feat"][inner] == 0)
    else:
        assert np.any((t["feat"] == 0) & inner & (t["thr"] == np.float32(want))), (t["feat"][:8], t["thr"][:8])
    if kind == "0_255":
        assert set(np.unique(x)) == {0.0, 255.0}


@pytest.mark.parametrize("P,cut", tc.SEAM_SPLITS)
def test_seam_recipes_cut_where_they_say(oracle, P, cut):
    c = tc.seam_split(P, cut)
    t = _checked(oracle, c)[0]
    if cut is None:
        assert len(t["left"]) == 1
        return
    v = c["sorted"]
    assert np.all(np.diff(v) >= 1e-6)
    assert len(t["left"]) == 3
    mid = np.float32(np.float32(v[cut - 1] + v[cut]) * np.float32(0.5))
    assert t["thr"][0] == mid and v[cut - 1] < mid <= v[cut]


def test_seam_list_covers_the_chunk_boundaries():
    Ps = {P for P, _ in tc.SEAM_SPLITS}
    assert {1, 2, 63, 64, 65, 128, 129, 4097} <= Ps
    cuts = {(P, cut) for P, cut in tc.SEAM_SPLITS if cut and cut % tc.CHUNK == 0}
    assert {cut for _, cut in cuts} >= {64, 128, 4096}      # the best cut's right value is lane 0 of a later chunk
    assert (64, 63) in tc.SEAM_SPLITS and (65, 64) in tc.SEAM_SPLITS


@pytest.mark.parametrize("kind", ["tie", "near"])
@pytest.mark.parametrize("seam", [64, 128])
def test_runs_across_a_seam_are_not_cut(oracle, kind, seam):
    c = tc.seam_run(kind, seam)
    v = c["sorted"]
    lo, hi = c["run"]
    assert lo < seam < hi and seam % tc.CHUNK == 0
    d = np.diff(v[lo:hi])
    assert np.all(d == 0) if kind == "tie" else np.all((d > 0) & (d < 1e-6))
    assert v[lo] - v[lo - 1] >= 1e-6 and v[hi] - v[hi - 1] >= 1e-6
    t = _checked(oracle, c)[0]
    inner = t["left"] != 0
    ends = {np.float32(np.float32(v[lo - 1] + v[lo]) * np.float32(0.5)), np.float32(np.float32(v[hi - 1] + v[hi]) * np.float32(0.5))}
    assert t["thr"][0] in ends
    assert not np.any(inner & (t["thr"] > v[lo]) & (t["thr"] <= v[hi - 1]))          # no threshold inside the run
    assert len(t["left"]) == 5            # the run stays together in one impure leaf


def test_seam_noise_recipe_reaches_every_small_segment(oracle):
    c = tc.seam_noise()
    t = _checked(oracle, c)[0]
    assert len(t["left"]) > 1000
    sizes = np.bincount(tc.route(t, c["X"]))
    assert {1, 2, 3, 4, 5} <= set(sizes.tolist())


@pytest.mark.parametrize("start,k", tc.ADJACENT)
def test_adjacent_floats_take_the_right_value(oracle, start, k):
    c = tc.adjacent_floats(start, k)
    v = c["sorted"]
    assert np.all(np.diff(v) >= 1e-6) and np.all(np.diff(v.view(np.int32)) != 0)
    assert np.all(np.abs(np.diff(v.view(np.int32))) == 1)                             # adjacent floats indeed
    t = _checked(oracle, c)[0]
    assert len(t["left"]) == 3 and t["thr"][0] == c["right"]
    sides = v < t["thr"][0]
    assert sides.sum() == k                                                          # `x < threshold` separates the two


def test_adjacent_list_has_cases_only_the_guard_saves():
    flags = [tc.adjacent_floats(s, k)["guard"] for s, k in tc.ADJACENT]
    assert flags.count(True) >= 4 and flags.count(False) >= 4
    assert tc.adjacent_floats(16.0, 5)["guard"] and tc.adjacent_floats(-16.0, 4)["guard"]


def test_overflowing_midpoints_take_the_right_value(oracle):
    """left + right = +-inf for finite values near 3e38.  Definition 4 of the oracle: the threshold is then `right`
    (an infinite one would send every example to one child and the same node would be split again and again until
    max_depth)."""
    for sign in (1, -1):
        c = tc.huge_values(sign)
        v = c["sorted"]
        with np.errstate(over="ignore"):
            assert np.isinf(np.float32(v[3] + v[4]))
        t = _checked(oracle, c)[0]
        assert np.all(np.isfinite(t["thr"])) and t["thr"][0] == v[4]
        assert len(t["left"]) == 7                                                   # three cuts isolate the three label runs
        leaf = tc.route(t, c["X"])
        for n in np.unique(leaf):
            assert len(set(c["labels"][leaf == n, 0])) == 1
    c = tc.huge_values(0)
    t = _checked(oracle, c)[0]
    assert len(t["left"]) == 3 and t["thr"][0] == 0.0                                # -2.6e38 | 2.6e38: an ordinary midpoint


def test_sentinel_recipe_cuts_between_the_sentinel_and_the_angles(oracle):
    c = tc.sentinel_and_negatives()
    t = _checked(oracle, c)[0]
    inner = t["left"] != 0
    assert np.any(inner & (t["feat"] == 0) & (t["thr"] > -2) & (t["thr"] < 0))
    assert np.any(inner & (t["feat"] == 1) & (t["thr"] < 0))


def test_parameter_recipes(oracle):
    got = {name: _checked(oracle, tc.params(name)) for name in tc.PARAMS}
    depth = lambda t: int(tc.node_depths(t).max())
    assert all(depth(t) == 2 for t in got["max_depth_1"])            # `depth > max_depth` stops: max_depth + 1 edges
    assert all(depth(t) == 3 for t in got["max_depth_2"])
    assert all(len(t["left"]) == 1 for t in got["min_child_above_half"])
    assert all(1 < len(t["left"]) <= 5 for t in got["min_child_half"])
    assert len(got["num_trees_1"]) == 1 and len(got["num_trees_64"]) == 64
    assert all(len(t["left"]) > 20 for name in ("min_split_0", "min_child_0", "num_features_1", "num_features_D") for t in got[name])
    # one feature per node against all six: the sampled subsets really differ
    assert any(not np.array_equal(a["feat"], b["feat"]) for a, b in zip(got["num_features_1"], got["num_features_D"]))
    # smoothing = 0: log(0) = -inf for the classes a leaf does not hold; the file still validates and loads (above)
    h = np.concatenate([x for t in got["smoothing_0"] for n in np.flatnonzero(t["left"] == 0) for x in t["mhist"][n]])
    assert np.isneginf(h).any() and not np.isnan(h).any() and not np.isposinf(h).any()
    h = np.concatenate([x for t in got["smoothing_small"] for n in np.flatnonzero(t["left"] == 0) for x in t["mhist"][n]])
    assert np.isfinite(h).all() and h.min() < -60


@pytest.mark.parametrize("bootstrap", [0, 1])
def test_degenerate_recipes(oracle, bootstrap):
    sizes = {}
    for name in tc.DEGENERATE:
        c = tc.degenerate(name, bootstrap)
        trees = _checked(oracle, c)
        sizes[name] = [len(t["left"]) for t in trees]
        for t in trees:
            for n in np.flatnonzero(t["left"] == 0):
                assert np.all(np.isfinite(np.concatenate(t["mhist"][n]))), name    # also with freq = P / 0 for an absent class
    for name in ("P1", "P2_same_label", "constant_features", "pure_labels", "identical_rows", "identical_rows_two_labels"):
        assert sizes[name] == [1, 1, 1], (name, sizes[name])
    assert sizes["absent_class"] == [3, 3, 3]
    assert max(sizes["P2_two_labels"]) == 3 and (bootstrap or sizes["P2_two_labels"] == [3, 3, 3])
    c = tc.degenerate("absent_class", bootstrap)
    assert set(np.unique(c["labels"])) == {0, 2} and c["cc"] == [4]


def test_many_examples_recipe_weighs_class_0_with_the_stalled_counter(oracle):
    c = tc.many_examples()
    P = c["X"].shape[0]
    n0 = int((c["labels"][:, 0] == 0).sum())
    assert n0 > (1 << 24)
    t = _checked(oracle, c)[0]
    assert len(t["left"]) == 3 and t["thr"][0] == 0.5
    right = t["mhist"][2][0]                   # one class-0 example, 25 of class 1
    f1 = P / 25.0
    stalled = np.log((P / float(1 << 24) + 1) / (P / float(1 << 24) + 25 * f1 + 2))
    exact = np.log((P / float(n0) + 1) / (P / float(n0) + 25 * f1 + 2))
    assert abs(stalled - exact) > 0.3
    assert abs(right[0] - stalled) < 1e-3, (right, stalled, exact)


@pytest.mark.parametrize("name", list(tc.FRAME_CONFIGS))
def test_frame_recipes(oracle, name):
    fr = tc.frames(name)
    X, Y, per_frame = tc.frames_dataset(oracle, fr)
    p = oracle.default_params(**fr["ctx_kw"])
    assert X.shape[1] == oracle.feature_length(p) and X.shape[0] == sum(per_frame) > 0
    byte_cols = [_is_byte_column(X[:, f]) for f in range(X.shape[1])]
    if name in ("no_colour_patch", "stride_1"):
        assert X.shape[1] == 3 and not any(byte_cols)                 # depth, height, normal: every feature a float
    else:
        assert sum(byte_cols) >= 27
    if name == "no_normal":
        assert X.shape[1] == 27 + 2
    if name == "empty_frame_between":
        assert per_frame[1] == 0 and per_frame[0] > 0 and per_frame[2] > 0
    if name == "stride_1":
        assert per_frame[0] > 10000
    if name == "two_calibrations":
        assert not np.array_equal(fr["calib"][0], fr["calib"][1])
        same = dict(fr, calib=np.tile(fr["calib"][:1], (2, 1)))
        assert not np.array_equal(tc.frames_dataset(oracle, same)[0], X)      # the second calibration changes the features
    assert Y.min() >= 0 and Y[:, 0].max() == 2 and Y[:, 1].max() == 3
    assert (fr["lab"] < 0).any()
