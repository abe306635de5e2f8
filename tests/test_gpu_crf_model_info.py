"""Which model a context keeps is the library's to say (rvseg_crf_model_info): the struct and the serial, DenseCRF objects
that share a context, a model set behind an object's back, and library errors that reach the caller as themselves.  One model
shape throughout: N = 300, C = 3, a CONST / Potts term (d = 2), a DIAG / Diagonal term (d = 2), a FULL / Matrix term (d = 3).
Every comparison is bit for bit against the same object alone on a context of its own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
N, C, NIT = 300, 3, 2


@pytest.fixture(scope="module")
def rv():
    import rovinasemanticsegmentation_amd as rv
    return rv


def _model(rv, seed):
    rng = np.random.default_rng(seed)
    U = rng.random((N, C)).astype(f32)
    W = (np.eye(C) + rng.uniform(-0.2, 0.2, (C, C))).astype(f32)
    terms = [((rng.random((N, 2)) * 5).astype(f32), 0.7, rv.CONST_KERNEL, rv.NORMALIZE_SYMMETRIC, None),
             ((rng.random((N, 2)) * 5).astype(f32), rv.DiagonalCompatibility(rng.uniform(0.05, 0.2, C)), rv.DIAG_KERNEL, rv.NORMALIZE_AFTER, None),
             ((rng.random((N, 3)) * 5).astype(f32), rv.MatrixCompatibility(W), rv.FULL_KERNEL, rv.NORMALIZE_SYMMETRIC, None)]
    return rng, U, terms


def _objective(rv, rng):
    gt = rng.integers(0, C, N).astype(np.int16)
    gt[::7] = -1
    return rv.IntersectionOverUnion(gt)


def _crf(rv, ctx, U, terms, logistic=None):
    crf = rv.DenseCRF(ctx, N, C)
    if logistic is None:
        crf.setUnaryEnergy(U)
    else:
        crf.setUnaryEnergy(*logistic)
    for F, comp, kt, nt, _ in terms:
        crf.addPairwiseEnergy(F, comp, kt, nt)
    return crf


def _bytes(x):
    """A result of a DenseCRF call (an array, a float or a tuple of them) as bytes."""
    if isinstance(x, tuple):
        return b"|".join(_bytes(v) for v in x)
    return np.ascontiguousarray(np.float64(x) if isinstance(x, float) else x).tobytes()


def test_info(rv, gpu_ctx_factory):
    torch = pytest.importorskip("torch")
    capi = rv.capi
    rng, U, terms = _model(rv, 1)
    ctx, other = gpu_ctx_factory(), gpu_ctx_factory()
    assert ctx.crf_model_serial() == 0   # a fresh context: no model, and asking makes none
    serial = ctx.crf_model_set(U, terms)
    m = ctx._crf_model()
    assert serial != 0 and m.serial == serial == ctx.crf_model_serial()
    assert (m.N, m.C, m.n_terms, m.K) == (300, 3, 3, 0)
    assert (list(m.d), list(m.compat_params), list(m.kernel_params)) == ([2, 2, 3] + [0] * 5, [1, 3, 6] + [0] * 5, [0, 2, 9] + [0] * 5)
    assert (m.n_compat_params, m.n_kernel_params) == (10, 11)
    # the in-place setters: the same model with new parameters
    L, f = rng.uniform(-1, 1, (C, 4)).astype(f32), rng.random((N, 4)).astype(f32)
    ctx.crf_model_set_logistic(L, f)
    assert ctx._crf_model().K == 4 and ctx.crf_model_serial() == serial
    ctx.crf_model_set_logistic_params((L * f32(0.5)).astype(f32))
    assert ctx._crf_model().K == 4 and ctx.crf_model_serial() == serial
    ctx.crf_model_set_unary(U)
    assert ctx._crf_model().K == 0 and ctx.crf_model_serial() == serial
    ctx.crf_model_set_compat(1, rv.DiagonalCompatibility(np.full(C, 0.3)))
    ctx.crf_model_set_kernel(1, np.array([0.8, 1.2], f32))
    m2 = ctx._crf_model()
    assert bytes(m2) == bytes(m)   # nothing of the struct moved
    # every model_set of the process names a new model
    seen = {serial}
    for new in (ctx.crf_model_set(U, terms), other.crf_model_set(U, terms)):
        assert new != 0 and new not in seen
        seen.add(new)
    assert ctx.crf_model_serial() != other.crf_model_serial()
    d_U = torch.from_numpy(U).cuda()
    d_F = [torch.from_numpy(t[0]).cuda() for t in terms]
    torch.cuda.synchronize()
    new = ctx.crf_model_set_device(N, C, [((d.data_ptr(), t[0].shape[1]),) + tuple(t[1:]) for d, t in zip(d_F, terms)], d_U.data_ptr())
    assert new not in seen and new == ctx.crf_model_serial() and bytes(ctx._crf_model())[8:] == bytes(m)[8:]
    # any other lattice build on the context ends the model, and the library says which
    for name, call in (("rvseg_crf_infer", lambda: ctx.crf_infer(U, terms[0][0], 3.0, 1)), ("rvseg_lattice_build", lambda: ctx.lattice_build(terms[0][0]))):
        ctx.crf_model_set(U, terms)
        assert ctx.crf_model_serial() != 0
        call()
        assert ctx.crf_model_serial() == 0
        with pytest.raises(capi.RvsegError) as e:
            ctx._crf_model()
        assert e.value.status == capi.ERR_INVALID_ARG and name in str(e.value)
    assert other.crf_model_serial() in seen   # the other context's model is untouched


def test_two_objects_take_turns(rv, gpu_ctx_factory):
    """Two DenseCRF objects with different models called alternately on one context: each result is that of the same object
    alone on its own context, a hand-over builds the lattices of the model that takes over once, and consecutive calls of one
    object build none."""
    shared, alone_a, alone_b = gpu_ctx_factory(), gpu_ctx_factory(), gpu_ctx_factory()
    rng, Ua, terms_a = _model(rv, 2)
    _, Ub, terms_b = _model(rv, 3)
    terms_b = terms_b[1:]   # two terms
    obj = _objective(rv, rng)
    a, b = _crf(rv, shared, Ua, terms_a), _crf(rv, shared, Ub, terms_b)
    a1, b1 = _crf(rv, alone_a, Ua, terms_a), _crf(rv, alone_b, Ub, terms_b)
    Q = {x: x.startInference() for x in (a1, b1)}   # the arguments of the calls below, from the objects alone
    Q[a], Q[b] = Q[a1], Q[b1]
    calls = [lambda x: x.startInference(), lambda x: x.stepInference(Q[x]), lambda x: x.klDivergence(Q[x], parts=True),
             lambda x: x.gradient(NIT, obj, energy_grad=True, kernel=True)]
    for call in calls:
        for x, x1, n_terms in ((a, a1, 3), (b, b1, 2)):
            builds = shared.debug_lattice_builds()
            got = call(x)
            assert shared.debug_lattice_builds() - builds == n_terms   # the hand-over
            assert _bytes(got) == _bytes(call(x1))
    for call in calls:   # b again and again: its model stays
        builds = shared.debug_lattice_builds()
        assert _bytes(call(b)) == _bytes(call(b1))
        assert shared.debug_lattice_builds() == builds


def test_a_foreign_model(rv, gpu_ctx_factory):
    """A model that somebody sets on the context directly between two calls of an object is not the object's: its next call
    sets its own again."""
    ctx, alone = gpu_ctx_factory(), gpu_ctx_factory()
    _, U, terms = _model(rv, 4)
    _, U2, terms2 = _model(rv, 5)
    crf, crf1 = _crf(rv, ctx, U, terms), _crf(rv, alone, U, terms)
    Q = crf.startInference()
    assert Q.tobytes() == crf1.startInference().tobytes()
    foreign = ctx.crf_model_set(U2, terms2)   # the same shape, other values
    want = crf1.stepInference(Q)
    assert crf.stepInference(Q).tobytes() == want.tobytes()
    assert ctx.crf_model_serial() != foreign
    assert ctx.crf_model_step(Q).tobytes() == want.tobytes()   # the context keeps the object's model again


def test_errors_are_themselves(rv, gpu_ctx_factory):
    """A refusal of the library that is not about a replaced model reaches the caller at once: nothing is set again first."""
    capi = rv.capi
    ctx = gpu_ctx_factory()
    rng, U, terms = _model(rv, 6)
    obj = _objective(rv, rng)
    L, f = rng.uniform(-1, 1, (C, 4)).astype(f32), rng.random((N, 4)).astype(f32)
    crf = _crf(rv, ctx, U, terms, logistic=(L, f))
    Q = crf.startInference()
    value = crf.gradient(NIT, obj, unary=True)[0]
    builds, serial = ctx.debug_lattice_builds(), ctx.crf_model_serial()
    with pytest.raises(capi.RvsegError) as e:
        crf.applyTranspose(5, Q)
    assert e.value.status == capi.ERR_INVALID_ARG and "no such term" in str(e.value)
    assert (ctx.debug_lattice_builds(), ctx.crf_model_serial()) == (builds, serial)
    ctx.crf_model_set_unary(U)   # drops the kept logistic unary behind the object's back: the model is still the object's
    with pytest.raises(capi.RvsegError) as e:
        crf.gradient(NIT, obj, unary=True)
    assert e.value.status == capi.ERR_INVALID_ARG and "keeps no logistic unary" in str(e.value)
    assert (ctx.debug_lattice_builds(), ctx.crf_model_serial()) == (builds, serial)
    crf.setUnaryEnergy(L, f)   # in place on the live model: the object is whole again, still without a build
    assert crf.gradient(NIT, obj, unary=True)[0] == value
    assert ctx.debug_lattice_builds() == builds
