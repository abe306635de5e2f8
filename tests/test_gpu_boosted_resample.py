"""The boosting round's weight kernels on caller-supplied weights (rvseg_boosted_resample) against the numpy serial chains
and search of tests/boost_restate.py, bit for bit: sizes around the 256-value tile and the 2 048-value batch of the ordered
sums, one large size, and weight patterns a short training never produces (tests/boost_cases.py).  The multiplicities the resample
kernel also counts are not an output of this entry: the training tests of tests/test_gpu_boosted.py cover them, where a
wrong count changes the tree."""
import numpy as np
import pytest

import boost_cases as bc
import boost_restate as br

pytestmark = pytest.mark.gpu

_want = {}


def _reference(case_key, w, miss, scale, key):
    """The restated round, computed once per case."""
    if case_key not in _want:
        m = np.zeros(len(w), bool) if miss is None else miss
        error, total, w2, cs = br.weight_round(w, m, scale)
        _want[case_key] = (error, w2, cs, br.pick(cs, br.uniforms(key, len(w))))
    return _want[case_key]


def _check(ctx, case_key, w, miss, scale, key):
    error, w2, cs, idx = _reference(case_key, w, miss, scale, key)
    got = ctx.boosted_resample(w, miss, scale, key)
    u32 = lambda a: np.asarray(a, np.float32).view(np.uint32)
    assert u32(got["error"]) == u32(error), (got["error"], error)
    assert np.array_equal(u32(got["weights"]), u32(w2))
    bad = np.flatnonzero(u32(got["cumsum"]) != u32(cs))
    assert bad.size == 0, ("cumsum differs first at", bad[0], got["cumsum"][bad[0]], cs[bad[0]])
    assert np.array_equal(got["idx"], idx)
    assert got["idx"].min() >= 0 and got["idx"].max() < len(w)
    return got


@pytest.mark.parametrize("N", bc.RESAMPLE_SIZES)
@pytest.mark.parametrize("pattern", bc.RESAMPLE_PATTERNS)
def test_round_kernels_equal_the_serial_chain(gpu_ctx_factory, pattern, N):
    ctx = gpu_ctx_factory(width=160, height=120)
    w, miss, scale, key = bc.resample_case(pattern, N)
    got = _check(ctx, (pattern, N), w, miss, scale, key)
    if pattern == "first":
        assert np.all(got["idx"] == 0)                      # equal cumsum values: the first index wins
    if pattern == "middle" and N > 1:
        assert np.all(got["idx"][br.uniforms(key, N) > 0] == N // 2)
    if miss is None:
        assert got["error"] == 0


def test_miss_none_equals_an_all_clear_miss_vector(gpu_ctx_factory):
    ctx = gpu_ctx_factory(width=160, height=120)
    w, _, _, key = bc.resample_case("binade_inside", 129)
    a, b = ctx.boosted_resample(w, None, 3.0, key), ctx.boosted_resample(w, np.zeros(129, bool), 3.0, key)
    assert all(np.array_equal(a[k], b[k]) for k in ("weights", "cumsum", "idx")) and a["error"] == b["error"] == 0


def test_a_draw_past_the_last_cumsum_is_clamped(gpu_ctx_factory):
    ctx = gpu_ctx_factory(width=160, height=120)
    w, miss, scale, key = bc.clamp_case()
    got = _check(ctx, "clamp", w, miss, scale, key)
    past = br.uniforms(key, len(w)) > got["cumsum"][-1]
    assert past.any() and np.all(got["idx"][past] == len(w) - 1)


def test_weights_without_a_usable_total_are_refused(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    ctx = gpu_ctx_factory(width=160, height=120)
    for w in (np.zeros(70, np.float32), np.array([1, -1, 2], np.float32), np.array([1, np.nan], np.float32), np.array([-0.0, 1], np.float32),
              np.full(3, 3e38, np.float32)):
        with pytest.raises(rv.capi.RvsegError) as e:
            ctx.boosted_resample(w)
        assert e.value.status == rv.capi.ERR_INVALID_ARG
