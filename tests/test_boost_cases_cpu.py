"""The recipes of tests/boost_cases.py do what they claim, shown from the restatement alone (tests/boost_restate.py: the
CPU oracle's tree learner, np.float32 chains, libm through ctypes) -- no GPU, no library."""
import functools

import numpy as np
import pytest

import boost_cases as bc
import boost_restate as br

F32 = np.float32


@functools.lru_cache(maxsize=None)
def _run(name, *args):
    c = getattr(bc, name)(*args)
    return c, br.boosted_train(c["X"], c["y"], c["n_classes"], c["rounds"], c["seed"], **c["params"])


@pytest.mark.parametrize("kind,use_bootstrap", [("byte", 0), ("byte", 1), ("float", 0), ("float", 1)])
def test_main_cases_boost_through_every_round(kind, use_bootstrap):
    c, r = _run("main_case", kind, use_bootstrap)
    assert r["rounds"] == c["rounds"] == 4
    assert np.all((r["errors"] > 0) & (r["errors"] < 1)) and np.all(np.isfinite(r["alphas"]))
    N = len(c["y"])
    for k, idx in enumerate(r["draws"]):
        mult = np.bincount(idx, minlength=N)
        assert mult.sum() == N and (mult >= 2).any() and (mult == 0).any(), k
    for before, after in zip(r["history"], r["history"][1:]):   # at least one weight changed in every round
        assert not np.array_equal(before, after)
    assert len({bytes(t) for t in r["trees"]}) > 1                # the rounds do not repeat one tree
    assert np.array_equal(r["weights"], r["alphas"])
    if kind == "float":
        assert not np.all(c["X"] == np.floor(c["X"]))


def test_negative_alpha_case_has_a_round_with_error_above_one_half():
    c, r = _run("negative_alpha_case")
    assert r["rounds"] == c["rounds"] and (r["alphas"] < 0).any() and (r["errors"] > 0.5).any()
    assert np.all((r["errors"] > 0) & (r["errors"] < 1))


def test_separable_case_stops_with_an_infinite_alpha():
    c, r = _run("separable_case")
    assert r["rounds"] == 1 and r["errors"][0] == 0 and np.isposinf(r["alphas"][0]) and np.isnan(r["errors"][1:]).all()
    assert np.isposinf(r["weights"][0])


def test_all_wrong_case_stops_without_a_tree():
    c, r = _run("all_wrong_case")
    assert r["rounds"] == 0 and r["errors"][0] == 1 and np.isnan(r["alphas"]).all() and r["model"] == b"\0\0\0\0"


def test_single_example_case_is_one_leaf_and_stops():
    c, r = _run("single_example_case")
    assert r["rounds"] == 1 and r["errors"][0] == 0 and np.array_equal(r["draws"][0], [0])


def test_alpha_follows_the_mixed_precision_of_the_reference():
    # C = 2: log(1) = 0, alpha = logf((1 - e) / e); C = 9: the double log(8) is added before the narrowing
    e = F32(0.3)
    a2, a9 = br.alpha_of(e, 2), br.alpha_of(e, 9)
    ratio = F32(F32(1) - e) / e
    assert a2 == F32(np.log(ratio)) or abs(float(a2) - np.log(float(ratio))) < 1e-6
    assert a9 == F32(float(a2) + np.log(8.0))
    assert np.isposinf(br.alpha_of(F32(0), 3)) and br.alpha_of(F32(0.75), 2) < 0


def test_binary_search_equals_the_linear_scan():
    rng = np.random.default_rng(0)
    for N in (1, 2, 65, 300):
        for pattern in ("uniform", "first", "last", "middle", "denormal"):
            w, miss, scale, key = bc.resample_case(pattern, N)
            _, _, _, cs = br.weight_round(w, np.zeros(N, bool) if miss is None else miss, scale)
            u = np.concatenate([br.uniforms(key, 200), cs[rng.integers(0, N, 20)], [F32(0)]]).astype(F32)
            assert np.array_equal(br.pick(cs, u), br.pick_linear(cs, u)), (N, pattern)


def test_resample_patterns_reach_what_they_name():
    w, _, _, _ = bc.resample_case("denormal", 129)
    assert 0 < w[0] < np.finfo(F32).tiny
    for pattern, at in (("binade_inside", 32), ("binade_seam", 64), ("binade_tile_seam", 256)):   # the running sum passes a power of two there
        w, miss, scale, _ = bc.resample_case(pattern, 4097)
        run = np.array([br.serial_sum(w[:k + 1]) for k in range(at - 1, at + 1)])
        assert np.floor(np.log2(run[0] * (1 - 1e-7))) < np.floor(np.log2(run[1])), (pattern, run)
    w, miss, _, _ = bc.resample_case("first", 129)
    _, _, _, cs = br.weight_round(w, np.zeros(129, bool), 1)
    assert np.all(cs == cs[0]) and np.all(br.pick(cs, br.uniforms(3, 50)) == 0)      # equal cumsum values: the first wins
    w, _, _, _ = bc.resample_case("last", 129)
    _, _, _, cs = br.weight_round(w, np.zeros(129, bool), 1)
    assert np.all(br.pick(cs, br.uniforms(3, 50)[1:]) == 128)


def test_clamp_case_has_a_draw_past_the_last_cumsum():
    w, _, scale, key = bc.clamp_case()
    _, total, w2, cs = br.weight_round(w, np.zeros(len(w), bool), scale)
    assert cs[-1] < F32(1) - F32(2.0 ** -24)
    u = br.uniforms(key, len(w))
    past = u > cs[-1]
    assert past.any()
    assert np.all(np.searchsorted(cs, u[past], side="left") == len(w))   # the unclamped index is N
    assert np.all(br.pick(cs, u)[past] == len(w) - 1)
