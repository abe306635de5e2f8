"""Boosted models of distinct trees on the GPU, from 1 to 64 trees and 2 to 64 classes (rvseg_boosted_load, then the
evaluator and the forest tools on the weighted one-hot leaf rows): the vote sums by bits, the forest's label by the
first-strict-maximum rule -- under equal weights a tie wherever two labels have as many votes -- and every tree's own,
unweighted vote.  The recipes come from tests/limits_tools_cases.py and are pinned in tests/test_limits_tools_cases_cpu.py."""
import numpy as np
import pytest

import boost_restate as br
import limits_tools_cases as lc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", lc.BOOSTED_WEIGHTS)
@pytest.mark.parametrize("T,C", lc.BOOSTED_CASES)
def test_boosted_models_of_distinct_trees(gpu_ctx_factory, T, C, which):
    want = lc.boosted_restated(T, C, which)
    ctx = gpu_ctx_factory(**lc.CTX_D6_SINGLE)
    try:
        ctx.boosted_load(want["stream"])
        info = ctx.forest_info()
        assert info["n_trees"] == T and info["class_counts"] == [C]
        assert np.array_equal(ctx.boosted_weights().view(np.uint32), want["weights"].view(np.uint32))
        X = lc.points(lc.BOOSTED_P)
        got = ctx.forest_eval(X)
        assert got.shape == want["sums"].shape and np.array_equal(got, want["sums"], equal_nan=True)
        assert np.array_equal(np.signbit(got), np.signbit(want["sums"]))
        pred = ctx.forest_classify(X)
        assert np.array_equal(pred, want["pred"])
        with np.errstate(invalid="ignore"):
            assert np.array_equal(pred, br.first_strict_max(got))
        votes = ctx.forest_classify_trees(X)
        assert votes.shape == (T, lc.BOOSTED_P) and np.array_equal(votes, want["votes"])
    finally:
        ctx.close()
