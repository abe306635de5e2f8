"""The recipes of tests/limits_tools_cases.py sit on the edges they are named for -- shown from the restatement alone (the
CPU oracle's evaluator, boost_restate, prune_restate), without a GPU.  These are conditions on the recipes, not
measurements of the library."""
import numpy as np
import pytest

import frame_cases as fc
import limits_tools_cases as lc
import prune_restate as pr
import tools_cases as tc

F32 = np.float32


def _distinct_rows(votes):
    return len({v.tobytes() for v in votes}) == len(votes)


def _off_diagonal_values(votes):
    agree = tc.agreement_counts(votes)
    return np.unique(agree[~np.eye(len(agree), dtype=bool)])


# ---- forests of distinct trees ---------------------------------------------------------------------------------------
def test_the_vote_cases_are_the_tree_counts_class_sums_and_point_counts_of_the_forest_walk():
    assert {(T, 5) for T in fc.EVAL_TREES} <= set(lc.VOTE_CASES)
    assert {(T, S) for S in fc.CLASS_SUMS for T in (3, 5, 17)} <= set(lc.VOTE_CASES)
    assert set(lc.POINT_COUNT_FORESTS) == {(4, 17), (17, 17)} <= set(lc.VOTE_CASES)
    assert {1, 4, 5, 16, 17, 64} <= {T for T, _ in lc.VOTE_CASES} and {1, 16, 17, 64} <= {S for _, S in lc.VOTE_CASES}


@pytest.mark.parametrize("T,S", [c for c in lc.VOTE_CASES if c[0] > 1 and c[1] > 1])
def test_no_two_trees_of_a_vote_forest_vote_alike(T, S):
    """(With one class every tree votes 0: S = 1 is the one class sum without distinct rows.)"""
    r = lc.restated(T, S, lc.VOTE_P)
    assert r["votes"].shape == (T, lc.VOTE_P) and r["C"] == S and _distinct_rows(r["votes"])
    assert len(np.unique(r["pred"])) > 1


@pytest.mark.parametrize("T,S", lc.POINT_COUNT_FORESTS)
def test_no_two_trees_vote_alike_from_15_points_on(T, S):
    for P in fc.POINT_COUNTS:
        if P >= 15:
            assert _distinct_rows(lc.restated(T, S, P)["votes"]), P


@pytest.mark.parametrize("T,S", [c for c in lc.VOTE_CASES if c[1] >= 17])
def test_wide_class_counts_reach_the_later_class_passes(T, S):
    r = lc.restated(T, S, lc.VOTE_P)
    assert (r["pred"] >= 16).any() and (r["votes"] >= 16).any()
    if S >= 63 and T >= 3:                          # and the passes c0 = 32 and c0 = 48
        assert (r["votes"] >= 48).any() and ((r["votes"] >= 32) & (r["votes"] < 48)).any()


def test_two_layer_forest_votes_differ_per_layer_and_tree():
    a, b = lc.two_layer_restated(0), lc.two_layer_restated(1)
    assert (a["C"], b["C"]) == lc.TWO_LAYERS and a["votes"].shape == b["votes"].shape == (17, lc.VOTE_P)
    assert _distinct_rows(a["votes"]) and _distinct_rows(b["votes"])
    assert (b["pred"] >= 16).any() and (b["votes"] >= 16).any() and not np.array_equal(a["pred"], b["pred"])


# ---- agreement -------------------------------------------------------------------------------------------------------
def test_agreement_cases_cover_the_pair_counts_and_the_tile_edges():
    assert {T for T, P in lc.AGREE_CASES if P == 513} == {1, 2, 5, 16, 17, 23, 64}
    assert {P for T, P in lc.AGREE_CASES if T == 17} == {1, 3, 4, 5, 511, 512, 513, 2047, 2048, 2049, 65536 + 257}
    assert (64, 2049) in lc.AGREE_CASES
    assert 64 * 65 // 2 > 8 * 256 and 23 * 24 // 2 > 256 > 17 * 18 // 2      # pairs per thread: 9, 2 and 1


@pytest.mark.parametrize("T", [17, 64])
def test_many_tree_agreement_has_many_distinct_pair_values(T):
    r = lc.restated(T, lc.agree_classes(T), 2049)
    assert _distinct_rows(r["votes"])
    assert len(_off_diagonal_values(r["votes"])) >= 50


@pytest.mark.parametrize("T", [t for t in lc.AGREE_TREES if t > 1])
def test_no_two_trees_of_an_agreement_forest_vote_alike(T):
    votes = lc.restated(T, lc.agree_classes(T), 513)["votes"]
    assert _distinct_rows(votes)
    off = _off_diagonal_values(votes)
    assert off.max() < 513 and (T < 16 or len(off) >= T)      # many pairs have a count of their own


# ---- confusion -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", lc.CONFUSION_CLASSES)
def test_confusion_labels_hold_the_first_and_the_last_class(C):
    for P in lc.CONFUSION_POINTS:
        r = lc.restated(lc.CONFUSION_T, C, P)
        lab = lc.confusion_labels(r["pred"], C)
        assert lab[0] == (0 if P > 1 else C - 1) and lab[-1] == C - 1 and lab.min() >= 0 and lab.max() == C - 1
        if P > 1 and C > 1:
            conf = tc.confusion_counts(lab, r["pred"], C)
            assert (conf - np.diag(np.diag(conf))).any() and np.trace(conf) > 0
            assert C <= 16 or (np.flatnonzero(conf.sum(0)) >= 16).any()          # a predicted class past the first 16
    assert 64 * 64 * 4 == 16384                     # C = 64: 4096 words of LDS


# ---- refit -----------------------------------------------------------------------------------------------------------
def test_refit_cases_loop_the_count_grid_of_a_256_cu_device():
    for T, S, P in lc.REFIT_CASES:
        assert T * min(P, 65536) > 4 * 256 * 256
        lab = lc.refit_labels(P, S)
        assert lab.shape == (P, 1) and set(np.unique(lab)) == set(range(S))
    assert lc.REFIT_CASES[0][2] > 65536 and (min(lc.REFIT_CASES[0][2], 65536) + 3) // 4 * 4 != lc.REFIT_CASES[0][2] - 65536   # stride != n in the tail
    # the labels of the second chunk differ from the first's: a lost offset changes the counts
    lab = lc.refit_labels(lc.CHUNK_TAIL, 3)
    assert not np.array_equal(lab[:257], lab[65536:])


# ---- the tie and NaN rule ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [3, 6])
def test_tie_forest_produces_every_named_outcome(T):
    sums, r = lc.tie_sums(T), lc.tie_restated(T)
    assert sums.shape == (lc.TIE_P, lc.TIE_C) and r["C"] == 20 and r["votes"].shape[0] == T
    out = lc.tie_outcomes(sums)
    for name, where in out.items():
        assert where.sum() >= 5, name
    for name, label in lc.TIE_LABELS.items():
        assert (r["pred"][out[name]] == label).all(), name
    assert not (r["pred"] == 16).any() and not (r["pred"] == 19).any()
    assert len(set(tc.br.split_trees(lc.tie_forest(T)["blob"]))) == T       # distinct trees, not copies
    assert (r["pred"] == 7).any()                                              # and +inf wins where nothing cancels it
    # 3 and 19 share a lane on both paths (3 = 19 mod 4 = 19 mod 16); 5 and 18 never do
    assert 3 % 4 == 19 % 4 and 3 % 16 == 19 % 16 and 5 % 4 != 18 % 4 and 5 % 16 != 18 % 16 and 18 % 16 == 2


# ---- pruning -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", lc.PRUNE_CHAIN_POINTS + (lc.CHUNK_TAIL,))
def test_prune_chains_contain_every_step_kind_and_every_move(P):
    c = lc.prune_chain(P)
    run = lc.chain_restated(c)
    assert set(run["step_kind"].tolist()) == {0, 1, 2} and {k for k, _ in run["moves"]} == {pr.EXCHANGE, pr.REMOVE, pr.ADD}
    assert len(run["step_kind"]) == 32 and len(run["trace"]) == 4 and c["votes"].shape == (lc.PRUNE_T, P)
    if P > 4:
        assert (c["labels"] == -1).any() and (c["labels"] == lc.PRUNE_C).any()


def test_prune_energies_differ_between_the_states_and_the_label_sets():
    assert set(lc.PRUNE_SMALL_POINTS) == {1, 2, 3, 4, 5, 1023, 1024, 1025}
    states = lc.prune_states(lc.PRUNE_T)
    assert states[:3] == [[0], [5], [0, 1, 2, 3, 4, 5]] and len(states[3]) == 64 and set(states[3]) == set(range(6))
    votes = lc.prune_votes(1025)
    assert _distinct_rows(votes)
    sets = lc.prune_label_sets(1025)
    assert sets[1][-1] == -1 and sets[2][-1] == lc.PRUNE_C and 0 <= sets[0][-1] < lc.PRUNE_C
    energies = {float(lc.error_energy(votes, sets[0], s)) for s in states}
    assert len(energies) >= 3 and all(0 < e < 1 for e in energies)
    # the last point is right under some state, so that its bad label costs an error
    assert any(lc.error_energy(votes, sets[1], s) > lc.error_energy(votes, sets[0], s) for s in states)


def test_wide_chain_adds_a_tree_past_the_first_sixteen():
    c = lc.wide_chain()
    assert len(c["state"]) == 15 and {63, 16} <= set(c["state"]) and c["params"]["p_add"] == 0.5
    assert c["votes"].shape == (64, 257) and _distinct_rows(c["votes"]) and c["votes"].max() < 16
    run = lc.chain_restated(c)
    assert set(run["step_kind"].tolist()) == {0, 1, 2}
    assert max(lc.added_trees(c, run)) >= 16 and max(run["state"]) >= 16
    assert _distinct_rows(lc.wide_votes(lc.COVER_P)) and len(_off_diagonal_values(lc.wide_votes(lc.COVER_P))) >= 50


def test_stride_case_tiles_its_block_and_keeps_the_cpu_work_small():
    assert lc.stride_point_count(256) == 4 * 256 * 1024 + 1029 and lc.STRIDE_BLOCK % 4 != 0
    c = lc.stride_case(2)                           # the same recipe on a device of two compute units
    P = c["P"]
    assert c["X"].shape == (P, 4) and np.array_equal(c["X"][lc.STRIDE_BLOCK:2 * lc.STRIDE_BLOCK], c["X"][:lc.STRIDE_BLOCK])
    assert c["votes"].shape == (3, lc.STRIDE_BLOCK) and _distinct_rows(c["votes"]) and c["labels"][-1] == lc.STRIDE_C
    assert not np.array_equal(c["labels"][lc.STRIDE_BLOCK:2 * lc.STRIDE_BLOCK], c["labels"][:lc.STRIDE_BLOCK])
    energies = [c["energy"](s) for s in lc.STRIDE_STATES]
    assert len({float(e) for e in energies}) == 3 and all(0 < e < 1 for e in energies)
    # the tiled restatement is the plain one on the votes written out
    whole = np.resize(c["votes"].T, (P, 3)).T
    for s, e in zip(lc.STRIDE_STATES, energies):
        assert e == lc.error_energy(whole, c["labels"], s)


# ---- boosted models ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C", lc.BOOSTED_CASES)
def test_boosted_models_tie_under_equal_weights_and_not_under_rising_ones(T, C):
    ones, rising, mixed = (lc.boosted_restated(T, C, w) for w in lc.BOOSTED_WEIGHTS)
    assert ones["votes"].shape == (T, lc.BOOSTED_P) and (T == 1 or _distinct_rows(ones["votes"]))
    top = (ones["sums"] == ones["sums"].max(1, keepdims=True)).sum(1)
    if T > 1:
        assert (top > 1).mean() > 0.25              # two labels with as many votes: the first wins
        assert not np.array_equal(ones["pred"], rising["pred"]) and not np.array_equal(ones["pred"], mixed["pred"])
    if C > 16:
        assert (ones["votes"] >= 16).any() and (ones["pred"] >= 16).any()
        tied = top > 1
        assert (np.argmax(ones["sums"][tied][:, ::-1] == ones["sums"][tied].max(1, keepdims=True), 1) < C - 16).any()   # a tie that reaches past class 15
    w = lc.boosted_weights("mixed", T)
    assert np.isinf(w[0]) and (T < 3 or ((w < 0).any() and np.signbit(w[2]) and w[2] == 0))
