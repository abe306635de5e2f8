"""The boosted stream on the host (rvseg_boosted_check / rvseg_boosted_rewrite, no GPU): both orders -- what
BoostedRandomForest::write emits (weight, tree) and what ::read expects (tree, weight), libforest classifier.cpp:250-280 --
built by splicing weights between the trees of the reference-written tests/golden/forest_single.dat."""
import os
import struct

import numpy as np
import pytest

import boost_restate as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = np.array([0.5, -1.25, np.inf, 3.0], np.float32)


def _capi():
    from rovinasemanticsegmentation_amd import _capi as capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return capi


@pytest.fixture(scope="module")
def trees():
    with open(os.path.join(ROOT, "tests", "golden", "forest_single.dat"), "rb") as fh:
        t = br.split_trees(fh.read())
    assert len(t) == len(WEIGHTS)
    return t


def _streams(trees):
    return {o: br.boosted_stream(trees, WEIGHTS, o) for o in (br.WEIGHT_FIRST, br.TREE_FIRST)}


def test_check_accepts_each_order_as_named_and_refuses_the_other(trees):
    capi = _capi()
    assert (capi.BOOSTED_WEIGHT_FIRST, capi.BOOSTED_TREE_FIRST) == (br.WEIGHT_FIRST, br.TREE_FIRST)
    s = _streams(trees)
    assert s[br.WEIGHT_FIRST] != s[br.TREE_FIRST] and len(s[br.WEIGHT_FIRST]) == len(s[br.TREE_FIRST])
    plain = capi.forest_check(struct.pack("<i", len(trees)) + b"".join(trees), 366)[2]
    for order in (br.WEIGHT_FIRST, br.TREE_FIRST):
        st, msg, info = capi.boosted_check(s[order], order, 366)
        assert st == capi.OK, msg
        assert info == plain
        st, msg, _ = capi.boosted_check(s[order], 1 - order, 366)
        assert st == capi.ERR_FORMAT, (order, msg)
    assert capi.boosted_check(s[br.WEIGHT_FIRST], 7)[0] == capi.ERR_INVALID_ARG          # no such order


def test_check_refuses_bad_streams(trees):
    capi = _capi()
    s = _streams(trees)
    for order in (br.WEIGHT_FIRST, br.TREE_FIRST):
        blob = s[order]
        assert capi.boosted_check(blob[:len(blob) // 2], order)[0] == capi.ERR_FORMAT     # truncated
        assert capi.boosted_check(blob[:-1], order)[0] == capi.ERR_FORMAT
        assert capi.boosted_check(blob + b"\0", order)[0] == capi.ERR_FORMAT              # bytes after the last tree
        st, msg, _ = capi.boosted_check(blob, order, 3)                                    # D = 3: split feature >= D
        assert st == capi.ERR_FORMAT and "mismatch" in msg
    assert capi.boosted_check(b"\0\0\0\0", br.WEIGHT_FIRST)[0] == capi.ERR_NO_FOREST
    # 65 trees
    many = br.boosted_stream([trees[0]] * 65, np.ones(65, np.float32))
    st, msg, _ = capi.boosted_check(many, br.WEIGHT_FIRST, 366)
    assert st == capi.ERR_CAPACITY and "65 trees" in msg
    assert capi.boosted_check(br.boosted_stream([trees[0]] * 64, np.ones(64, np.float32)), br.WEIGHT_FIRST, 366)[0] == capi.OK


def _single_leaf_tree(hist):
    one = struct.pack("<ii", 1, 0)
    return (one + struct.pack("<if", 1, 0.0) + one + struct.pack("<ii", 1, len(hist)) + np.asarray(hist, np.float32).tobytes() +
            struct.pack("<ii", 1, 0))


def test_check_refuses_empty_and_unequal_leaf_histograms():
    capi = _capi()
    ok = br.boosted_stream([_single_leaf_tree([0.1, 0.2]), _single_leaf_tree([0.3, 0.1])], [1.0, 2.0])
    assert capi.boosted_check(ok)[0] == capi.OK
    empty = br.boosted_stream([_single_leaf_tree([])], [1.0])
    st, msg, _ = capi.boosted_check(empty)
    assert st == capi.ERR_FORMAT and "empty leaf histogram" in msg
    st, msg, _ = capi.boosted_check(br.boosted_stream([_single_leaf_tree([0.1, 0.2]), _single_leaf_tree([])], [1.0, 1.0]))
    assert st == capi.ERR_FORMAT
    st, msg, _ = capi.boosted_check(br.boosted_stream([_single_leaf_tree([0.1, 0.2]), _single_leaf_tree([0.1, 0.2, 0.3])], [1.0, 1.0]))
    assert st == capi.ERR_FORMAT and "differ" in msg


def test_rewrite_returns_each_stream_and_converts_between_the_orders(trees):
    capi = _capi()
    s = _streams(trees)
    for order in (br.WEIGHT_FIRST, br.TREE_FIRST):
        assert capi.boosted_rewrite(s[order], order) == s[order]
        assert capi.boosted_rewrite(s[order], order, 1 - order) == s[1 - order]
        with pytest.raises(capi.RvsegError):
            capi.boosted_rewrite(s[order], 1 - order)
    # weights travel bit for bit: -0.0, NaN payloads, infinities
    odd = np.array([-0.0, np.inf, -np.inf, 1e-45], np.float32)
    blob = br.boosted_stream(trees, odd)
    assert capi.boosted_rewrite(capi.boosted_rewrite(blob, br.WEIGHT_FIRST, br.TREE_FIRST), br.TREE_FIRST, br.WEIGHT_FIRST) == blob
