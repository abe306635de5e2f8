"""Forest pruning on the GPU at the limits of its kernels (csrc/kernels_prune.hip, rvseg_prune.hip): fewer points than a
lane's four, the 1024-point block edges, a 64-tree forest, a vote table written in two chunks, the grid-stride loop of the
walk, and the cover energy on the agreement counts of 64 trees.  The recipes come from tests/limits_tools_cases.py (pinned
in tests/test_limits_tools_cases_cpu.py), the chain from tests/prune_restate.py.  Every comparison is exact: states, step
kinds, and every float by its bits."""
import numpy as np
import pytest

import limits_tools_cases as lc
import prune_cases as pc
import prune_restate as pr
import tools_cases as tc

pytestmark = pytest.mark.gpu

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def small_ctx(gpu_ctx_factory):
    ctx = gpu_ctx_factory(**dict(pc.CTX_D4, multi_layer=0))
    ctx.forest_load(lc.prune_forest())
    assert ctx.forest_info()["n_trees"] == lc.PRUNE_T and ctx.forest_info()["class_counts"] == [lc.PRUNE_C]
    return ctx


@pytest.fixture(scope="module")
def wide_ctx(gpu_ctx_factory):
    ctx = gpu_ctx_factory(**dict(pc.CTX_D4, multi_layer=0))
    ctx.forest_load(lc.wide_forest())
    assert ctx.forest_info()["n_trees"] == lc.WIDE_T and ctx.forest_info()["class_counts"] == [lc.WIDE_C]
    return ctx


def _same_run(got, want):
    assert got["state"].dtype == np.int32 and np.array_equal(got["state"], want["state"])
    assert _bits(got["best_energy"]) == _bits(want["best_energy"])
    assert np.array_equal(got["step_kind"], want["step_kind"])
    trace = pr.trace_array(want["trace"])
    assert len(got["trace"]) == len(trace)
    for field in ("iteration", "state_size"):
        assert np.array_equal(got["trace"][field], trace[field]), field
    for field in ("temperature", "energy", "best_energy"):
        assert np.array_equal(_bits(got["trace"][field]), _bits(trace[field])), field


# ---- small and block-edge point counts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("P", lc.PRUNE_SMALL_POINTS)
def test_energy_at_small_and_block_edge_point_counts(small_ctx, P):
    X, votes = lc.prune_points(P)[0], lc.prune_votes(P)
    assert np.array_equal(small_ctx.forest_classify_trees(X), votes)
    for labels in lc.prune_label_sets(P):
        for state in lc.prune_states(lc.PRUNE_T):
            got = small_ctx.forest_prune_energy(X, labels, state)
            assert _bits(got) == _bits(lc.error_energy(votes, labels, state)), (int(labels[-1]), state)


@pytest.mark.parametrize("P", lc.PRUNE_CHAIN_POINTS)
def test_chain_at_small_and_block_edge_point_counts(small_ctx, P):
    c = lc.prune_chain(P)
    _same_run(small_ctx.forest_prune(c["X"], c["labels"], 0, c["state"], **c["params"]), lc.chain_restated(c))


# ---- wide forest -------------------------------------------------------------------------------------------------------
def test_chain_over_64_distinct_trees(wide_ctx):
    c = lc.wide_chain()
    assert np.array_equal(wide_ctx.forest_classify_trees(c["X"]), c["votes"])
    want = lc.chain_restated(c)
    _same_run(wide_ctx.forest_prune(c["X"], c["labels"], 0, c["state"], **c["params"]), want)
    for state in ([63], [16, 63], list(range(63, -1, -1)), want["final"].tolist()):
        assert _bits(wide_ctx.forest_prune_energy(c["X"], c["labels"], state)) == _bits(lc.error_energy(c["votes"], c["labels"], state)), state


def test_cover_energy_over_64_distinct_trees(wide_ctx):
    P = lc.COVER_P
    X, votes = lc.wide_points(P)[0], lc.wide_votes(P)
    agree = tc.agreement_counts(votes)
    assert np.array_equal(wide_ctx.forest_measure(X, want=("agree",))["agree"], agree)
    for state in ([63], [16, 63], lc.WIDE_STATE, list(range(64))):
        assert _bits(wide_ctx.forest_prune_energy(X, None, state, 0, pr.COVER)) == _bits(pr.cover_energy(agree, P, state)), state


# ---- across a chunk ----------------------------------------------------------------------------------------------------
def test_chain_and_votes_across_a_chunk(small_ctx):
    c = lc.prune_chain(lc.CHUNK_TAIL)
    assert c["X"].shape[0] == 65536 + 257
    assert np.array_equal(small_ctx.forest_classify_trees(c["X"]), c["votes"])
    _same_run(small_ctx.forest_prune(c["X"], c["labels"], 0, c["state"], **c["params"]), lc.chain_restated(c))


# ---- the grid-stride loop of the walk ----------------------------------------------------------------------------------
def test_energy_through_the_grid_stride_loop(gpu_ctx_factory):
    cus = _cus()
    c = lc.stride_case(cus)
    assert c["P"] == 4 * cus * 1024 + 1029 and c["X"].shape == (c["P"], 4)
    ctx = gpu_ctx_factory(**dict(pc.CTX_D4, multi_layer=0))
    ctx.forest_load(lc.stride_forest())
    for state in lc.STRIDE_STATES:
        assert _bits(ctx.forest_prune_energy(c["X"], c["labels"], state)) == _bits(c["energy"](state)), state
