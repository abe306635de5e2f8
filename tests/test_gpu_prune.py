"""Forest pruning on the GPU (rvseg_forest_prune / _prune_energy / _prune_apply and rv.RandomForestPrune) against the Python
restatement of tests/prune_restate.py on the recipes of tests/prune_cases.py.  Every comparison is exact: states, step
kinds, and every float by its bits.  The recipes are pinned on the CPU in tests/test_prune_cases_cpu.py; no test runs the
reference's default schedule (78 750 proposals)."""
import ctypes as C
import struct

import numpy as np
import pytest

import boost_restate as br
import prune_cases as pc
import prune_restate as pr
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
_ctxs = {}


def _ctx(gpu_ctx_factory, name):
    """One context per recipe, with the recipe's forest loaded."""
    if name not in _ctxs:
        c = pc.case(name)
        ctx = gpu_ctx_factory(**c["ctx"])
        ctx.forest_load(c["blob"])
        _ctxs[name] = ctx
    return _ctxs[name]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("name", pc.CASES)
def test_trajectory_equals_the_restatement(gpu_ctx_factory, name):
    c, want = pc.case(name), pc.restated(name)
    ctx = _ctx(gpu_ctx_factory, name)
    assert np.array_equal(ctx.forest_classify_trees(c["X"], c["layer"]), pc.votes(name))     # the votes the chain walks
    got = ctx.forest_prune(c["X"], c["labels"], c["layer"], c["state"], **c["params"])
    assert got["state"].dtype == np.int32 and np.array_equal(got["state"], want["state"])
    assert _bits(got["best_energy"]) == _bits(want["best_energy"])
    assert np.array_equal(got["step_kind"], want["step_kind"])
    trace = pr.trace_array(want["trace"])
    assert len(got["trace"]) == len(trace)
    for field in ("iteration", "state_size"):
        assert np.array_equal(got["trace"][field], trace[field]), field
    for field in ("temperature", "energy", "best_energy"):
        assert np.array_equal(_bits(got["trace"][field]), _bits(trace[field])), field


def test_a_second_run_and_another_seed(gpu_ctx_factory):
    """The chain leaves nothing behind on the context (counter and ticket are back at zero), and the seed is all that
    separates two runs."""
    c = pc.case("main")
    ctx = _ctx(gpu_ctx_factory, "main")
    a = ctx.forest_prune(c["X"], c["labels"], 0, c["state"], **c["params"])
    b = ctx.forest_prune(c["X"], c["labels"], 0, c["state"], **c["params"])
    assert np.array_equal(a["step_kind"], b["step_kind"]) and np.array_equal(a["state"], b["state"]) and a["trace"].tobytes() == b["trace"].tobytes()
    other = dict(c["params"], seed=c["params"]["seed"] + 1)
    want = pr.run(other, c["T"], c["state"], pc.energy_of("main"))
    got = ctx.forest_prune(c["X"], c["labels"], 0, c["state"], **other)
    assert np.array_equal(got["step_kind"], want["step_kind"]) and np.array_equal(got["state"], want["state"])
    assert not np.array_equal(got["step_kind"], a["step_kind"])


def test_trace_capacity_and_optional_outputs(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    c, want = pc.case("main"), pc.restated("main")
    ctx = _ctx(gpu_ctx_factory, "main")
    pp = rv.capi.prune_params(**c["params"])
    assert rv.capi.prune_schedule(pp) == (4, 32)
    state = np.zeros(64, np.int32)
    state[:3] = c["state"]
    n, n_trace = C.c_int32(3), C.c_int32(-1)
    trace = np.full(2 * 5, -7, np.int32)                                   # room for two rows of five words
    st = ctx.L.rvseg_forest_prune(ctx.h, c["X"].ctypes.data, 4097, 4, c["labels"].ctypes.data, 0, C.byref(pp), state.ctypes.data, C.byref(n), None,
                                  trace.ctypes.data, 2, C.byref(n_trace), None)
    assert st == 0 and n_trace.value == 4 and np.array_equal(state[:n.value], want["state"])
    assert trace.tobytes() == pr.trace_array(want["trace"])[:2].tobytes()


@pytest.mark.parametrize("name", ["main", "bad_labels", "layer1", "c16_state64", "tie", "cover"])
def test_energy_of_hand_picked_states(gpu_ctx_factory, name):
    c = pc.case(name)
    ctx = _ctx(gpu_ctx_factory, name)
    energy = pc.energy_of(name)
    kind = c["params"].get("energy", pr.ERROR)
    T = c["T"]
    for state in ([0], [T - 1], [0, 0], list(range(T)), list(range(T - 1, -1, -1)), [1, 0, 1, 0, 2], [t % T for t in range(64)], c["state"]):
        got = ctx.forest_prune_energy(c["X"], c["labels"], state, c["layer"], kind)
        assert _bits(got) == _bits(energy(state)), state
    if name == "tie":       # the order of a state matters: first to reach the maximum
        assert ctx.forest_prune_energy(c["X"], c["labels"], c["state"]) != ctx.forest_prune_energy(c["X"], c["labels"], c["state"][::-1])


def test_apply_writes_the_chosen_trees_and_evaluates_like_the_oracle(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    c = pc.case("layer1")
    ctx = gpu_ctx_factory(**c["ctx"])
    ctx.forest_load(c["blob"])
    trees = br.split_trees(c["blob"])
    for state in ([4, 1, 1, 3], [2], list(range(6)) * 10 + [5, 5, 5, 5]):
        ctx.forest_load(c["blob"])
        ctx.forest_prune_apply(state)
        stream = struct.pack("<i", len(state)) + b"".join(trees[t] for t in state)       # the original file's byte ranges
        assert ctx.forest_write() == stream
        assert ctx.forest_info()["n_trees"] == len(state)
        assert np.array_equal(ctx.forest_eval(c["X"]), O.Forest(stream).eval(c["X"], True))
    # the facade: prune, then the forest is the best state's trees
    ctx.forest_load(c["blob"])
    forest = rv.RandomForest(ctx)
    pruner = rv.RandomForestPrune(**c["params"])
    assert pruner.prune(forest, c["X"], c["labels"], c["layer"], c["state"]) is forest
    best = pc.restated("layer1")["state"]
    assert np.array_equal(pruner.state, best) and forest.write() == struct.pack("<i", len(best)) + b"".join(trees[t] for t in best)
    assert pruner.format().count("\n") == 4 and pruner.format().startswith("iteration: 1 energy: ")


def test_default_state_is_the_first_fifteen_trees(gpu_ctx_factory):
    c = pc.case("main")                                                     # 8 trees: min(15, T) = 8
    ctx = _ctx(gpu_ctx_factory, "main")
    want = pr.run(c["params"], c["T"], list(range(8)), pc.energy_of("main"))
    got = ctx.forest_prune(c["X"], c["labels"], **c["params"])
    assert np.array_equal(got["state"], want["state"]) and np.array_equal(got["step_kind"], want["step_kind"])


def test_refused_calls_leave_the_model_and_the_outputs(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    c = pc.case("main")
    ctx = gpu_ctx_factory(**c["ctx"])
    ctx.forest_load(c["blob"])
    L, h, X, lab = ctx.L, ctx.h, c["X"], c["labels"]
    P = X.shape[0]
    before = ctx.forest_write()
    state = np.full(70, 1, np.int32)
    n, best, n_trace = C.c_int32(3), C.c_float(-7.0), C.c_int32(-7)
    trace, kinds = np.full(5 * 8, -7, np.int32), np.full(64, 201, np.uint8)

    def prune(pp, n_state=3, layer=0, first=1, D=4, points=P):
        state[:] = 1
        state[0] = first
        n.value = n_state
        return L.rvseg_forest_prune(h, X.ctypes.data, points, D, lab.ctypes.data, layer, C.byref(pp), state.ctypes.data, C.byref(n), C.byref(best),
                                    trace.ctypes.data, 8, C.byref(n_trace), kinds.ctypes.data)

    def untouched(n_state=3, first=1):
        return (ctx.forest_write() == before and state[0] == first and (state[1:] == 1).all() and n.value == n_state and best.value == -7.0 and
                n_trace.value == -7 and (trace == -7).all() and (kinds == 201).all())
    good = dict(c["params"])
    for bad in (dict(alpha=0.0), dict(alpha=1.0), dict(alpha=float("nan")), dict(inner_loops=0), dict(p_exchange=0.0), dict(p_remove=-0.5),
                dict(energy=2), dict(start_temperature=100.0, end_temperature=1e-5, alpha=0.95, inner_loops=(1 << 22) // 315 + 1),
                dict(start_temperature=float("inf"))):
        assert prune(rv.capi.prune_params(**dict(good, **bad))) == rv.capi.ERR_INVALID_ARG and untouched(), bad
        with pytest.raises(rv.capi.RvsegError):
            rv.capi.prune_schedule(rv.capi.prune_params(**dict(good, **bad)))
    pp = rv.capi.prune_params(**good)
    for kw in (dict(n_state=0), dict(n_state=65), dict(n_state=-1), dict(first=8), dict(first=-1), dict(layer=1), dict(layer=-1), dict(D=3), dict(points=0)):
        assert prune(pp, **kw) == rv.capi.ERR_INVALID_ARG and untouched(kw.get("n_state", 3), kw.get("first", 1)), kw
    out = C.c_float(-7.0)
    for st_, n_ in ((np.asarray([8], np.int32), 1), (np.asarray([0], np.int32), 0), (np.zeros(65, np.int32), 65)):
        assert L.rvseg_forest_prune_energy(h, X.ctypes.data, P, 4, lab.ctypes.data, 0, 0, st_.ctypes.data, n_, C.byref(out)) == rv.capi.ERR_INVALID_ARG
        assert L.rvseg_forest_prune_apply(h, st_.ctypes.data, n_) == rv.capi.ERR_INVALID_ARG
    assert L.rvseg_forest_prune_energy(h, X.ctypes.data, P, 4, None, 0, 0, state.ctypes.data, 3, C.byref(out)) == rv.capi.ERR_INVALID_ARG   # no labels
    assert out.value == -7.0 and ctx.forest_write() == before
    # more than 16 classes: the error energy is refused, the cover energy is not
    wide = gpu_ctx_factory(multi_layer=0)
    wide.forest_load(rv.synthetic.make_forest_bytes(seed=5, n_trees=3, leaves_per_tree=8, max_depth=4, single_classes=17))
    Xw = rv.synthetic.random_points(5, 64, 366)
    wide_before = wide.forest_write()
    with pytest.raises(rv.capi.RvsegError, match="16 classes"):
        wide.forest_prune(Xw, np.zeros(64, np.int32), state=[0, 1], **good)
    assert wide.forest_prune(Xw, None, state=[0, 1], **dict(good, energy=pr.COVER))["trace"].shape == (4,) and wide.forest_write() == wide_before
    # a boosted model, and no model at all
    boosted = gpu_ctx_factory(**c["ctx"])
    stream = br.boosted_stream(br.split_trees(pc.case("main")["blob"]), np.ones(8, F32))
    boosted.boosted_load(stream)
    state[:] = 1
    n.value = 3
    assert L.rvseg_forest_prune(boosted.h, X.ctypes.data, P, 4, lab.ctypes.data, 0, C.byref(pp), state.ctypes.data, C.byref(n), C.byref(best),
                                trace.ctypes.data, 8, C.byref(n_trace), kinds.ctypes.data) == rv.capi.ERR_INVALID_ARG
    assert L.rvseg_forest_prune_apply(boosted.h, state.ctypes.data, 3) == rv.capi.ERR_INVALID_ARG
    assert L.rvseg_forest_prune_energy(boosted.h, X.ctypes.data, P, 4, lab.ctypes.data, 0, 0, state.ctypes.data, 3, C.byref(out)) == rv.capi.ERR_INVALID_ARG
    assert boosted.boosted_write() == stream and b"boosted" in L.rvseg_last_error(boosted.h)
    fresh = gpu_ctx_factory(**c["ctx"])
    assert L.rvseg_forest_prune(fresh.h, X.ctypes.data, P, 4, lab.ctypes.data, 0, C.byref(pp), state.ctypes.data, C.byref(n), C.byref(best),
                                trace.ctypes.data, 8, C.byref(n_trace), kinds.ctypes.data) == rv.capi.ERR_NO_FOREST
    assert L.rvseg_forest_prune_apply(fresh.h, state.ctypes.data, 3) == rv.capi.ERR_NO_FOREST
    assert L.rvseg_forest_prune_energy(fresh.h, X.ctypes.data, P, 4, lab.ctypes.data, 0, 0, state.ctypes.data, 3, C.byref(out)) == rv.capi.ERR_NO_FOREST
    assert untouched() and out.value == -7.0
    # and the model still prunes
    assert np.array_equal(ctx.forest_prune(X, lab, 0, c["state"], **good)["state"], pc.restated("main")["state"])
