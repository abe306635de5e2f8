"""Parameters of a kept DenseCRF model changed in place (rvseg.h, "The learning loop"): rvseg_crf_model_set_kernel,
_set_logistic / _set_logistic_params, _gradient_params and _energy_gradient.  The reference of every comparison is the path
that existed before them, on the same GPU: a fresh rvseg_crf_model_set with the same parameters and the call-by-call
composition.  The bar is bit equality (arrays compared as bytes, doubles included), so there is no tolerance."""
import numpy as np
import pytest

from crf_loop_cases import ParentPath

pytestmark = pytest.mark.gpu
f32 = np.float32
NIT = 3


@pytest.fixture(scope="module")
def rv():
    import rovinasemanticsegmentation_amd as rv
    return rv


@pytest.fixture(scope="module")
def ctxs(gpu_ctx_factory):
    """(the context whose model is changed in place, the context of the fresh models)"""
    return gpu_ctx_factory(), gpu_ctx_factory()


def _features(rng, N, d):
    """Duplicate rows and an all-zero row."""
    F = (rng.random((N, d)) * 5).astype(f32)
    if N > 4:
        F[N // 2] = F[1]
        F[N - 1] = F[1]
        F[3] = 0.0
    return F


def _kparams(rv, rng, kt, d):
    if kt == rv.DIAG_KERNEL:
        return rng.uniform(0.6, 1.6, d).astype(f32)
    return (np.eye(d) + rng.uniform(-0.3, 0.3, (d, d))).astype(f32).reshape(-1)


def _objective(rv, rng, N, C):
    gt = rng.integers(0, C, N).astype(np.int16)
    gt[::7] = -1
    return rv.IntersectionOverUnion(gt)


def _snapshot(ctx, obj, dims, A, B, apply_terms=()):
    """Everything the issue compares, as bytes: trace (Q, map, KL doubles), gradient_kernel (value, three gradients, Q[n]),
    lattice_gradient of every term, and apply of the given terms."""
    Q, mp, kl = ctx.crf_model_trace(NIT)
    val, ug, cg, kg, Qn = ctx.crf_model_gradient_kernel(NIT, obj, want_Q=True)
    out = {"Q": Q, "map": mp, "kl": kl, "value": np.float64(val), "ug": ug, "cg": cg, "kg": kg, "Qn": Qn}
    for t in range(len(dims)):
        out["lattice_gradient %d" % t] = ctx.crf_model_lattice_gradient(t, A, B)
    for t in apply_terms:
        out["apply %d" % t] = ctx.crf_model_apply(t, A)
    return {k: np.ascontiguousarray(v).tobytes() for k, v in out.items()}


def _same(got, want, what):
    assert got.keys() == want.keys()
    diff = [k for k in want if got[k] != want[k]]
    assert not diff, "%s: %s differ from a fresh model" % (what, diff)


def _with(terms, t, kp):
    terms = [list(x) for x in terms]
    terms[t][4] = kp
    return [tuple(x) for x in terms]


def _case(rv, seed, N, C, d, kt, norm):
    """A CONST Potts term and the term under test (Matrix compatibility), built with parameters p0; p1 is what it is set to."""
    rng = np.random.default_rng(seed)
    U = rng.random((N, C)).astype(f32)
    W = (np.eye(C) + rng.uniform(-0.2, 0.2, (C, C))).astype(f32)
    terms = [(_features(rng, N, 2), 0.7, rv.CONST_KERNEL, rv.NORMALIZE_SYMMETRIC, None),
             (_features(rng, N, d), rv.MatrixCompatibility(W), kt, norm, _kparams(rv, rng, kt, d))]
    return rng, U, terms, _kparams(rv, rng, kt, d), _objective(rv, rng, N, C), rng.random((N, C)).astype(f32), rng.random((N, C)).astype(f32)


def _check_set_kernel(rv, ctxs, seed, N, C, d, kt, norm):
    live, fresh = ctxs
    rng, U, terms, p1, obj, A, B = _case(rv, seed, N, C, d, kt, norm)
    live.crf_model_set(U, terms)
    live.crf_model_set_kernel(1, p1)
    fresh.crf_model_set(U, _with(terms, 1, p1))
    _same(_snapshot(live, obj, [2, d], A, B), _snapshot(fresh, obj, [2, d], A, B), "d=%d kernel=%d C=%d norm=%d" % (d, kt, C, norm))


KERNEL_CASES = [(1, d) for d in range(1, 8)] + [(2, d) for d in (1, 3, 7)]   # (DIAG | FULL, d)


@pytest.mark.parametrize("norm", [0, 1, 2, 3])
@pytest.mark.parametrize("kt,d", KERNEL_CASES)
def test_set_kernel_equals_a_fresh_model(rv, ctxs, kt, d, norm):
    _check_set_kernel(rv, ctxs, 100 + 10 * d + kt, 257, 3, d, kt, norm)


@pytest.mark.parametrize("C", [1, 2, 3, 21, 64])
@pytest.mark.parametrize("kt,d", [(1, 2), (2, 3)])
def test_set_kernel_at_every_class_count(rv, ctxs, kt, d, C):
    _check_set_kernel(rv, ctxs, 300 + C, 257, C, d, kt, rv.NORMALIZE_SYMMETRIC)


def test_set_kernel_touches_no_other_term(rv, ctxs):
    """Eight terms at (400, 5), two CONST terms between the others: the third and the last are set; apply of every other term
    keeps its bits, and the whole model equals a fresh one."""
    live, fresh = ctxs
    N, C = 400, 5
    rng = np.random.default_rng(7)
    U = rng.random((N, C)).astype(f32)
    kinds = [rv.DIAG_KERNEL, rv.CONST_KERNEL, rv.FULL_KERNEL, rv.DIAG_KERNEL, rv.CONST_KERNEL, rv.FULL_KERNEL, rv.DIAG_KERNEL, rv.DIAG_KERNEL]
    dims = [2, 3, 3, 5, 1, 2, 4, 3]
    norms = [3, 2, 1, 0, 3, 3, 2, 1]
    terms = [(_features(rng, N, d), rv.DiagonalCompatibility(rng.uniform(0.05, 0.2, C)), kt, nt, None if kt == rv.CONST_KERNEL else _kparams(rv, rng, kt, d))
             for kt, d, nt in zip(kinds, dims, norms)]
    obj = _objective(rv, rng, N, C)
    A, B = rng.random((N, C)).astype(f32), rng.random((N, C)).astype(f32)
    live.crf_model_set(U, terms)
    live.crf_model_kl(A)   # (the per-entry normalisers of the terms that scale their input exist before the rebuild)
    others = [t for t in range(8) if t not in (2, 7)]
    before = {t: live.crf_model_apply(t, A).tobytes() for t in range(8)}
    p2, p7 = _kparams(rv, rng, kinds[2], dims[2]), _kparams(rv, rng, kinds[7], dims[7])
    live.crf_model_set_kernel(2, p2)
    live.crf_model_set_kernel(7, p7)
    after = {t: live.crf_model_apply(t, A).tobytes() for t in range(8)}
    assert all(after[t] == before[t] for t in others)
    assert after[2] != before[2] and after[7] != before[7]
    fresh.crf_model_set(U, _with(_with(terms, 2, p2), 7, p7))
    _same(_snapshot(live, obj, dims, A, B, range(8)), _snapshot(fresh, obj, dims, A, B, range(8)), "eight terms")


def test_set_kernel_shrinks_and_grows_the_lattice_in_place(rv, ctxs):
    """All-zero parameters collapse the features onto one lattice simplex, x 50 spreads them to about one vertex per point;
    then the same parameters twice, and NULL back to the features as passed."""
    live, fresh = ctxs
    rng, U, terms, p1, obj, A, B = _case(rv, 11, 257, 4, 3, rv.DIAG_KERNEL, rv.NORMALIZE_SYMMETRIC)
    live.crf_model_set(U, terms)
    for what, p in (("zeros", np.zeros(3, f32)), ("x 50", np.full(3, 50, f32)), ("zeros again", np.zeros(3, f32)), ("p1", p1), ("p1 twice", p1),
                    ("NULL", None)):
        live.crf_model_set_kernel(1, p)
        fresh.crf_model_set(U, _with(terms, 1, p))
        vertices = fresh.last_schedule()["vertices"]
        print(what, "vertices", vertices, live.last_schedule()["vertices"])
        assert live.last_schedule()["vertices"] == vertices
        _same(_snapshot(live, obj, [2, 3], A, B), _snapshot(fresh, obj, [2, 3], A, B), what)


def test_set_kernel_retries_at_the_safe_capacity(rv, gpu_ctx_factory):
    """lattice_capacity_log2 = 4: sixteen hash slots cannot hold the spread lattice, so the first attempt overflows and the term
    is built again at the capacity that cannot; a fresh model_set on a context of the same kind does the same for all terms."""
    live, fresh = gpu_ctx_factory(lattice_capacity_log2=4), gpu_ctx_factory(lattice_capacity_log2=4)
    N, C = 257, 3
    rng = np.random.default_rng(13)
    U = rng.random((N, C)).astype(f32)
    F = _features(rng, N, 3)
    small = np.zeros(3, f32)   # one simplex: four vertices fit sixteen slots
    terms = [(F, rv.PottsCompatibility(0.8), rv.DIAG_KERNEL, rv.NORMALIZE_SYMMETRIC, small)]
    obj = _objective(rv, rng, N, C)
    A, B = rng.random((N, C)).astype(f32), rng.random((N, C)).astype(f32)
    live.crf_model_set(U, terms)
    spread = np.full(3, 50, f32)
    live.crf_model_set_kernel(0, spread)
    assert live.last_schedule()["capacity_log2"] > 4 and live.last_schedule()["vertices"] > 8
    fresh.crf_model_set(U, _with(terms, 0, spread))
    _same(_snapshot(live, obj, [3], A, B), _snapshot(fresh, obj, [3], A, B), "safe-capacity retry")
    live.crf_model_set_kernel(0, small)   # and back down
    fresh.crf_model_set(U, terms)
    _same(_snapshot(live, obj, [3], A, B), _snapshot(fresh, obj, [3], A, B), "back at the configured capacity")


def test_set_kernel_refuses_what_it_cannot_set(rv, gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    capi = rv.capi
    rng, U, terms, p1, obj, A, B = _case(rv, 17, 64, 3, 2, rv.DIAG_KERNEL, rv.NORMALIZE_SYMMETRIC)
    with pytest.raises(capi.RvsegError) as e:   # no model yet
        ctx.crf_model_set_kernel(1, p1)
    assert e.value.status == capi.ERR_INVALID_ARG
    ctx.crf_model_set(U, terms)
    want = _snapshot(ctx, obj, [2, 2], A, B)
    for term, p in ((0, None), (-1, None), (2, None)):   # a CONST term, out of range twice
        with pytest.raises(capi.RvsegError) as e:
            ctx.crf_model_set_kernel(term, p)
        assert e.value.status == capi.ERR_INVALID_ARG
        _same(_snapshot(ctx, obj, [2, 2], A, B), want, "after a refused call")
    ctx.lattice_build(terms[0][0])   # any other lattice build ends the model
    with pytest.raises(capi.RvsegError) as e:
        ctx.crf_model_set_kernel(1, p1)
    assert e.value.status == capi.ERR_INVALID_ARG and "rvseg_lattice_build" in str(e.value)


# ---- the kept logistic unary and the parameter gradient --------------------------------------------------------------------------
def _logistic_case(rv, seed, N, C, K):
    rng = np.random.default_rng(seed)
    f = rng.random((N, K)).astype(f32)
    L0, L1 = rng.uniform(-1, 1, (C, K)).astype(f32), rng.uniform(-1, 1, (C, K)).astype(f32)
    terms = [(_features(rng, N, 2), rv.MatrixCompatibility(np.eye(C, dtype=f32)), rv.DIAG_KERNEL, rv.NORMALIZE_SYMMETRIC, _kparams(rv, rng, 1, 2))]
    return rng, f, L0, L1, terms, _objective(rv, rng, N, C)


def _composed(ctx, obj, f):
    """gradient_kernel followed by logistic_gradient: what gradient_params replaces."""
    val, ug, cg, kg, _ = ctx.crf_model_gradient_kernel(NIT, obj)
    return {"value": np.float64(val).tobytes(), "ug": ctx.crf_logistic_gradient(ug, f).tobytes(), "cg": cg.tobytes(), "kg": kg.tobytes()}


@pytest.mark.parametrize("C", [1, 3, 64])
@pytest.mark.parametrize("N", [1, 5, 257])
@pytest.mark.parametrize("K", [1, 4, 9])
def test_kept_logistic_unary_and_gradient_params(rv, ctxs, K, N, C):
    live, fresh = ctxs
    rng, f, L0, L1, terms, obj = _logistic_case(rv, 1000 + 100 * K + 10 * N + C, N, C, K)
    live.crf_model_set(np.zeros((N, C), f32), terms)
    live.crf_model_set_logistic(L0, f)
    for L in (L0, L1):
        if L is L1:
            live.crf_model_set_logistic_params(L1)
        fresh.crf_model_set(np.zeros((N, C), f32), terms)
        fresh.crf_model_set_unary(fresh.crf_logistic_unary(L, f))
        assert live.crf_model_trace(NIT)[0].tobytes() == fresh.crf_model_trace(NIT)[0].tobytes()
        assert live.crf_model_kl(live.crf_model_start()).tobytes() == fresh.crf_model_kl(fresh.crf_model_start()).tobytes()
        val, ug, cg, kg = live.crf_model_gradient_params(NIT, obj)
        got = {"value": np.float64(val).tobytes(), "ug": ug.tobytes(), "cg": cg.tobytes(), "kg": kg.tobytes()}
        assert ug.shape == (C * K,)
        _same(got, _composed(fresh, obj, f), "gradient_params")
    # the parts not asked for stay away; the value does not depend on them
    val2, ug2, cg2, kg2 = live.crf_model_gradient_params(NIT, obj, True, False, False)
    assert (val2, ug2.tobytes(), cg2, kg2) == (val, ug.tobytes(), None, None)
    assert live.crf_model_gradient_params(NIT, obj, False, True, True)[2].tobytes() == cg.tobytes()


def test_kept_logistic_unary_from_device_memory(rv, ctxs):
    torch = pytest.importorskip("torch")
    live, fresh = ctxs
    N, C, K = 257, 3, 4
    rng, f, L0, L1, terms, obj = _logistic_case(rv, 23, N, C, K)
    d_f = torch.from_numpy(f).cuda()
    d_gt = torch.from_numpy(obj.gt).cuda()
    d_out = torch.zeros(1 + C * K + C * (C + 1) // 2 + 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    live.crf_model_set(np.zeros((N, C), f32), terms)
    live.crf_model_set_logistic_device(L1, d_f.data_ptr())
    fresh.crf_model_set(fresh.crf_logistic_unary(L1, f), terms)
    assert live.crf_model_trace(NIT)[0].tobytes() == fresh.crf_model_trace(NIT)[0].tobytes()
    rec, keep = obj.record(N, C, d_gt=d_gt.data_ptr())
    base, n_ug, n_cg = d_out.data_ptr(), C * K, C * (C + 1) // 2
    live.crf_model_call_device("gradient_params", NIT, rec, base, base + 8, base + 8 * (1 + n_ug), base + 8 * (1 + n_ug + n_cg))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    want = _composed(fresh, obj, f)
    got = {"value": out[:1].tobytes(), "ug": out[1:1 + n_ug].tobytes(), "cg": out[1 + n_ug:1 + n_ug + n_cg].tobytes(), "kg": out[1 + n_ug + n_cg:].tobytes()}
    _same(got, want, "gradient_params_device")


def test_set_unary_drops_the_kept_logistic_unary(rv, ctxs):
    live, _ = ctxs
    capi = rv.capi
    N, C, K = 64, 3, 4
    rng, f, L0, L1, terms, obj = _logistic_case(rv, 29, N, C, K)
    live.crf_model_set(np.zeros((N, C), f32), terms)
    with pytest.raises(capi.RvsegError) as e:   # nothing kept yet
        live.crf_model_set_logistic_params(L0)
    assert e.value.status == capi.ERR_INVALID_ARG
    live.crf_model_set_logistic(L0, f)
    live.crf_model_gradient_params(NIT, obj)
    live.crf_model_set_unary(rng.random((N, C)).astype(f32))
    for call in (lambda: live.crf_model_gradient_params(NIT, obj), lambda: live.crf_model_set_logistic_params(L1)):
        with pytest.raises(capi.RvsegError) as e:
            call()
        assert e.value.status == capi.ERR_INVALID_ARG and "logistic" in str(e.value)
    val, ug, cg, kg = live.crf_model_gradient_params(NIT, obj, unary=False)   # the model itself stays usable
    assert ug is None and np.isfinite(val)
    with pytest.raises(capi.RvsegError) as e:
        live.crf_model_set_logistic(L0[:, :0], f[:, :0])   # K = 0
    assert e.value.status == capi.ERR_INVALID_ARG


# ---- rvseg_crf_model_energy_gradient -----------------------------------------------------------------------------------------
def _energy_case(rv, seed=31, N=257, C=4, K=4):
    rng = np.random.default_rng(seed)
    f = rng.random((N, K)).astype(f32)
    f[:, -1] = 1
    L = rng.uniform(-0.5, 0.5, (C, K)).astype(f32)
    pos = np.stack([np.arange(N) % 20, np.arange(N) // 20], 1).astype(f32)
    gauss = (pos / f32(3)).astype(f32)
    bil = np.concatenate([pos / f32(8), rng.random((N, 3)).astype(f32) * f32(4)], 1).astype(f32)
    gt = ((np.arange(N) // 20) * C // 13).astype(np.int16)
    gt[::5] = -1

    def terms():
        return [(gauss, rv.PottsCompatibility(1.0), rv.DIAG_KERNEL, rv.NORMALIZE_SYMMETRIC, None),
                (bil, rv.MatrixCompatibility(np.eye(C, dtype=f32)), rv.FULL_KERNEL, rv.NORMALIZE_SYMMETRIC, None)]
    return rng, f, L, terms, gt


def _dense_crf(rv, ctx, N, C, L, f, terms):
    crf = rv.DenseCRF(ctx, N, C)
    crf.setUnaryEnergy(L, f)
    for F, comp, kt, nt, _ in terms:
        crf.addPairwiseEnergy(F, comp, kt, nt)
    return crf


@pytest.mark.parametrize("mask", range(1, 8))
def test_energy_gradient_equals_the_composition(rv, ctxs, mask):
    live, fresh = ctxs
    N, C = 257, 4
    rng, f, L, terms, gt = _energy_case(rv)
    obj = rv.IntersectionOverUnion(gt)
    flags = (bool(mask & 1), bool(mask & 2), bool(mask & 4))
    crf = _dense_crf(rv, live, N, C, L, f, terms())
    energy = rv.CRFKernelEnergy(crf, obj, NIT, *flags)
    parent = ParentPath(rv, fresh, L, f, terms(), obj, NIT)
    x0 = energy.initialValue()
    assert x0.shape == ((16 if flags[0] else 0) + (11 if flags[1] else 0) + (27 if flags[2] else 0),)
    x1 = (x0 * f32(1.1) + f32(0.01)).astype(f32)
    x2 = x1.copy()
    x2[0] += f32(0.25)   # one value of the first learned group
    for l2 in (0.0, 1e-3):
        energy.setL2Norm(l2)
        for what, x in (("x0", x0), ("x1", x1), ("x1 again", x1), ("x2", x2), ("x0 again", x0)):
            builds = live.debug_lattice_builds()
            value, dx = energy.gradient(x)
            built = live.debug_lattice_builds() - builds
            if what == "x1":
                first_value, first_dx = value, dx.tobytes()
            if what == "x1 again":   # the same x: the same 64 bits, and no lattice is built
                assert value == first_value and dx.tobytes() == first_dx and built == 0
            elif what in ("x2", "x0 again") or (what == "x1" and l2 == 0.0):
                # x2 moves one value of the first learned group, the others move every value: a lattice per term whose kernel
                # parameters changed and no other (both terms have some; no build overflows at the default capacity)
                assert built == (0 if not flags[2] else 1 if what == "x2" and mask == 4 else 0 if what == "x2" else 2), (what, built)
            want_value, want_dx = parent.gradient(x, *flags, l2)
            print(mask, l2, what, value, want_value)
            assert dx.dtype == f32 and dx.tobytes() == want_dx.tobytes(), (what, l2)
            assert value == want_value, (what, l2)
            # this object's parameters are x now, as after the setters
            got = np.concatenate([p for on, p in zip(flags, (crf.unaryParameters(), crf.labelCompatibilityParameters(), crf.kernelParameters())) if on])
            assert got.tobytes() == x.tobytes()
    # the learned model serves the other calls: the kept model equals a fresh one with the same parameters
    assert crf.inference_trace(NIT)[0].tobytes() == fresh.crf_model_trace(NIT)[0].tobytes()


def test_energy_gradient_arguments(rv, ctxs):
    live, _ = ctxs
    capi = rv.capi
    N, C = 257, 4
    rng, f, L, terms, gt = _energy_case(rv)
    obj = rv.LogLikelihood(gt, 0.01)
    live.crf_model_set(np.zeros((N, C), f32), terms())
    live.crf_model_set_logistic(L, f)
    x = np.zeros(16 + 11 + 27 + 4, f32)
    for m, n in ((7, 53), (7, 55), (1, 15), (2, 12), (4, 26), (8, 0), (-1, 0)):
        with pytest.raises(capi.RvsegError) as e:
            live.crf_model_energy_gradient(NIT, obj, m, 0.0, x[:n])
        assert e.value.status == capi.ERR_INVALID_ARG, (m, n)
    value, dx = live.crf_model_energy_gradient(NIT, obj, 0, 0.0, x[:0])   # nothing learned: the value alone
    assert dx.shape == (0,) and value == -live.crf_model_gradient_params(NIT, obj, False, False, False)[0]
    live.crf_model_set_unary(np.zeros((N, C), f32))   # without a kept logistic unary the unary group is empty
    v = np.concatenate([np.ones(1, f32), np.eye(C, dtype=f32)[np.triu_indices(C)]])
    value, dx = live.crf_model_energy_gradient(NIT, obj, 3, 0.0, v)
    assert dx.shape == (11,)
