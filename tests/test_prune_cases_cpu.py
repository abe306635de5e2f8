"""The recipes of tests/prune_cases.py cross the edges they are named for -- shown from the restatement alone
(tests/prune_restate.py), without a GPU.  These are conditions on the recipes, not measurements of the library."""
import numpy as np
import pytest

import prune_cases as pc
import prune_restate as pr

F32 = np.float32


def test_the_default_schedule_is_the_references():
    temps = pr.temperatures(100.0, 1e-5, 0.95)
    assert len(temps) == 315 and temps[0] == F32(F32(100) * F32(0.95)) and temps[-1] <= F32(1e-5) < temps[-2]
    assert len(pr.temperatures(1.0, 0.5, 0.8)) == 4 and pr.temperatures(0.5, 0.5, 0.8) == [] and pr.temperatures(0.4, 0.5, 0.8) == []


def test_move_choice_follows_the_prob_sum_scan():
    moves = pr.registered_moves(dict(p_exchange=0.5, p_remove=0.0, p_add=0.25))
    assert [k for k, _ in moves] == [pr.EXCHANGE, pr.ADD]                       # probability 0 is not registered
    assert [pr.choose_move(moves, F32(u)) for u in (0.0, 0.49, 0.5, 0.74, 0.75, 0.99)] == [0, 0, 2, 2, 2, 2]   # 0.75 and up: the last
    assert pr.propose(pr.REMOVE, [4], 1, 1, 6) == [4] and pr.propose(pr.REMOVE, [4, 5, 3], 1, 7, 6) == [4, 3]
    assert pr.propose(pr.ADD, [1] * 64, 3, 0, 6) == [1] * 64 and pr.propose(pr.ADD, [1] * 63, 9, 0, 6) == [1] * 63 + [3]
    assert pr.propose(pr.EXCHANGE, [0, 1, 2], 11, 5, 6) == [0, 1, 5]


def test_main_case_takes_every_branch_of_the_acceptance_test():
    run = pc.restated("main")
    assert len(run["step_kind"]) == 32 and len(run["trace"]) == 4
    assert set(run["step_kind"].tolist()) == {0, 1, 2}
    assert (run["improvement"] == 0).any() and (run["improvement"] < 0).any()
    assert run["state"].tolist() != pc.case("main")["state"]
    assert run["best_energy"] < pc.energy_of("main")(pc.case("main")["state"])
    assert pc.case("main")["X"].shape[0] > 4 * 1024                                # more than one block's worth of points per pass


def test_floor_and_cap_cases_draw_the_blocked_move():
    moves = pc.restated("moves")["moves"]
    assert (pr.REMOVE, 1) in moves and {k for k, _ in moves} == {pr.EXCHANGE, pr.REMOVE, pr.ADD}
    assert max(n for _, n in moves) >= 3
    cap = pc.restated("cap")["moves"]
    assert cap[0][1] == 63 and (pr.ADD, 64) in cap and max(n for _, n in cap) == 64


def test_tie_case_depends_on_the_first_to_reach_rule():
    c, v = pc.case("tie"), pc.votes("tie")
    first, lowest = pr.predictions(v, c["state"]), pr.predictions(v, c["state"], rule="lowest")
    assert (first != lowest).sum() > 20
    assert pr.error_count(v, c["labels"], c["state"]) != pr.error_count(v, c["labels"], c["state"], rule="lowest")


def test_the_other_cases_are_what_they_say():
    dup = pc.case("duplicates")["state"]
    assert len(set(dup)) < len(dup)
    bad = pc.case("bad_labels")
    assert (bad["labels"] == -1).any() and (bad["labels"] == bad["C"]).any()
    wrong = (bad["labels"] < 0) | (bad["labels"] >= bad["C"])
    assert pc.restated("bad_labels")["best_energy"] >= F32(wrong.sum()) / F32(len(wrong))
    lay = pc.case("layer1")
    assert lay["multi"] == 1 and lay["layer"] == 1 and lay["C"] == 5 and len(np.unique(pc.votes("layer1"))) == 5
    one = pc.case("single_class")
    assert one["C"] == 1 and not pc.votes("single_class").any() and pc.restated("single_class")["best_energy"] == 0
    wide = pc.case("c16_state64")
    assert wide["C"] == 16 and len(wide["state"]) == 64 and pc.votes("c16_state64").max() >= 12
    assert max(np.bincount(pc.votes("c16_state64")[wide["state"], n]).max() for n in range(65)) >= 32   # a counter well past one nibble
    none = pc.restated("no_iterations")
    assert len(none["trace"]) == 0 and len(none["step_kind"]) == 0 and none["state"].tolist() == pc.case("no_iterations")["state"]
    cover = pc.restated("cover")
    assert pc.case("cover")["params"]["energy"] == pr.COVER and cover["best_energy"] < pc.energy_of("cover")(pc.case("cover")["state"])
    assert set(cover["step_kind"].tolist()) >= {0, 1} and len({n for _, n in cover["moves"]}) > 2


@pytest.mark.parametrize("name", pc.CASES)
def test_point_counts_cover_the_word_and_block_edges(name):
    assert pc.case(name)["X"].shape[0] in (63, 64, 65, 1000, 4097)
    assert {pc.case(n)["X"].shape[0] for n in pc.CASES} == {63, 64, 65, 1000, 4097}
