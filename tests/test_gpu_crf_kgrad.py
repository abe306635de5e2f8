"""The kernel-parameter gradient of a kept DenseCRF model on the GPU (rvseg_crf_model_lattice_gradient / _kernel_gradient /
_backward_kernel / _gradient_kernel) against the float32 restatement in crf_kgrad_cases.py on the CPU oracle's lattice:
df and fg bit for bit, every double within KL_BOUND of the sum of its absolute terms (N C <= 2^17 everywhere) and
identical in all 64 bits on a second call."""
import os
import re

import numpy as np
import pytest

import crf_kgrad_cases as KG
import crf_learn_cases as LC
import crf_model_cases as M
import crf_restate as R

pytestmark = pytest.mark.gpu

NORMS = [R.NO_NORMALIZATION, R.NORMALIZE_BEFORE, R.NORMALIZE_AFTER, R.NORMALIZE_SYMMETRIC]
COMPATS = [R.POTTS, R.DIAGONAL, R.MATRIX]
KERNELS = [R.CONST_KERNEL, R.DIAG_KERNEL, R.FULL_KERNEL]
f32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rovinasemanticsegmentation_amd", "csrc")


def _constant(header, name):
    with open(os.path.join(CSRC, header)) as fh:
        return int(re.search(r"constexpr int %s = (\d+);" % name, fh.read()).group(1))


def _set(ctx, rv, U, terms):
    ctx.crf_model_set(U, M.api_terms(rv, terms, U.shape[1]))


def _within(got, want, S, what):
    got, want, S = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(S)
    assert got.shape == want.shape, what
    assert (S > 0).all(), what + ": an entry without terms checks nothing"
    err = np.abs(got - want)
    print("%s: max error / S = %.3g (bound %.1g)" % (what, (err / S).max(), LC.KL_BOUND))
    assert (err <= LC.KL_BOUND * S).all(), what


def _kernel_params(rng, kt, d):
    """DIAG: non-unit values; FULL: a non-symmetric matrix, column-major."""
    if kt == R.CONST_KERNEL:
        return None
    if kt == R.DIAG_KERNEL:
        return rng.uniform(0.6, 1.6, d).astype(f32)
    return (np.eye(d) + rng.uniform(-0.3, 0.3, (d, d))).astype(f32).reshape(-1)


def _model(seed, N, C, specs, compat_scale=1.0):
    """specs: [(d, compat, norm, kernel_type)] -> rng, U, terms (crf_restate tuples).  compat_scale: on the compatibility
    parameters (many strong terms drive the marginals to one-hot rows, whose gradients are all zero)."""
    rng, U, terms = M.random_model(seed, N, C, [s[:3] for s in specs])
    terms = [(f, c, (p * f32(compat_scale)).astype(f32), s[3], nt, _kernel_params(rng, s[3], s[0]))
             for (f, c, p, _, nt, _), s in zip(terms, specs)]
    return rng, U, terms


def _restated(oracle, U, terms):
    model = M.Model(oracle, U, terms)
    lr = LC.Learn.of_model(model)
    return lr, KG.KernelLearn(lr, [KG.OracleView(b[0]) for b in model.built], terms)


def _features(rng, N, d):
    """Duplicate rows, an all-zero row (every rank comparison ties) and rows on lattice points."""
    F = (rng.random((N, d)) * 5).astype(f32)
    if N > 4:
        F[N // 2] = F[1]
        F[N - 1] = F[1]
        F[3] = 0.0
    return F


def _lattice_gradient_case(ctx, rv, oracle, seed, N, C, d):
    rng = np.random.default_rng(seed)
    U = rng.random((N, C)).astype(f32)
    F = _features(rng, N, d)
    terms = [(F, R.POTTS, np.array([1.0], f32), R.CONST_KERNEL, R.NO_NORMALIZATION, None)]
    _set(ctx, rv, U, terms)
    a, b = rng.normal(size=(N, C)).astype(f32), rng.random((N, C)).astype(f32)
    got = ctx.crf_model_lattice_gradient(0, a, b)
    want = KG.lattice_gradient(KG.OracleView(oracle.Lattice(F)), a, b, f32)
    assert got.shape == (N, d) and np.abs(want).max() > 0
    assert np.array_equal(got, want), (N, C, d, np.abs(got - want).max())


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7])
def test_lattice_gradient_ranks(gpu_ctx_factory, oracle, d):
    """The ranks the model keeps, through lattice_gradient: d = 1 .. 7 at N = 257 (no multiple of 4) with duplicate and
    all-zero rows, bit for bit."""
    import rovinasemanticsegmentation_amd as rv
    _lattice_gradient_case(gpu_ctx_factory(), rv, oracle, 4000 + d, 257, 3, d)


@pytest.mark.parametrize("N,C", [(257, 1), (257, 2), (257, 21), (257, 64), (1, 3), (2, 3), (5, 3), (2600, 43), (3600, 33)])
def test_lattice_gradient_shapes(gpu_ctx_factory, oracle, N, C):
    """C = 1, 2 (the filters' double blur elsewhere), 21, 64 (4 points per block step); N = 1, 2, 5; and (2600, 43), (3600, 33),
    which need more blocks than the grid cap: the grid-stride loop."""
    import rovinasemanticsegmentation_amd as rv
    assert N * C <= M.KL_MAX_ELEMENTS
    if N > 2000:
        PB = 256 // C
        assert (N + PB - 1) // PB > _constant("rvseg_crf.h", "KL_MAX_BLOCKS")
    _lattice_gradient_case(gpu_ctx_factory(), rv, oracle, 4100 + N + C, N, C, 3)


def _kernel_gradient_case(ctx, rv, oracle, seed, N, C, d, compat, norm, kt):
    rng, U, terms = _model(seed, N, C, [(d, compat, norm, kt)])
    _set(ctx, rv, U, terms)
    lr, kl = _restated(oracle, U, terms)
    a, b = rng.normal(size=(N, C)).astype(f32), rng.random((N, C)).astype(f32)
    grad, fg = ctx.crf_model_kernel_gradient(0, a, b, want_fg=True)
    want, S, wfg = kl.kernel_gradient(0, a, b)
    assert np.array_equal(fg, wfg), (norm, kt, np.abs(fg - wfg).max())
    assert grad.shape == (KG.n_kernel_params(kt, d),)
    if kt != R.CONST_KERNEL:
        _within(grad, want, S, "kernel gradient norm %d kernel %d" % (norm, kt))
        again = ctx.crf_model_kernel_gradient(0, a, b)
        assert again.tobytes() == grad.tobytes()
        assert np.array_equal(ctx.crf_model_lattice_gradient(0, a, b), KG.lattice_gradient(kl.views[0], a, b, f32))


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("compat", COMPATS)
def test_kernel_gradient(gpu_ctx_factory, oracle, compat, norm):
    """4 normalisations x 3 compatibilities x {CONST, DIAG with non-unit parameters, FULL with a non-symmetric matrix} at
    (300, 7, d = 3)."""
    import rovinasemanticsegmentation_amd as rv
    ctx = gpu_ctx_factory()
    for kt in KERNELS:
        _kernel_gradient_case(ctx, rv, oracle, 4200 + 16 * norm + 4 * compat + kt, 300, 7, 3, compat, norm, kt)


def test_kernel_gradient_d7(gpu_ctx_factory, oracle):
    import rovinasemanticsegmentation_amd as rv
    _kernel_gradient_case(gpu_ctx_factory(), rv, oracle, 4300, 300, 7, 7, R.MATRIX, R.NORMALIZE_SYMMETRIC, R.FULL_KERNEL)


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("norm", [R.NORMALIZE_BEFORE, R.NORMALIZE_AFTER, R.NORMALIZE_SYMMETRIC])
def test_kernel_gradient_few_classes(gpu_ctx_factory, oracle, norm, C):
    """C <= 2: K and K^T of the normalised mixes take the double-precision blur and the seq slice, like apply."""
    import rovinasemanticsegmentation_amd as rv
    _kernel_gradient_case(gpu_ctx_factory(), rv, oracle, 4350 + 4 * norm + C, 300, C, 3, R.DIAGONAL, norm, R.FULL_KERNEL)


EIGHT_TERMS = [(2, R.POTTS, R.NORMALIZE_SYMMETRIC, R.DIAG_KERNEL), (3, R.DIAGONAL, R.NORMALIZE_BEFORE, R.FULL_KERNEL),
               (1, R.MATRIX, R.NORMALIZE_AFTER, R.DIAG_KERNEL), (2, R.POTTS, R.NO_NORMALIZATION, R.CONST_KERNEL),
               (4, R.MATRIX, R.NORMALIZE_SYMMETRIC, R.FULL_KERNEL), (2, R.DIAGONAL, R.NO_NORMALIZATION, R.FULL_KERNEL),
               (5, R.POTTS, R.NORMALIZE_AFTER, R.DIAG_KERNEL), (3, R.DIAGONAL, R.NORMALIZE_BEFORE, R.CONST_KERNEL)]


def test_backward_and_gradient_kernel(gpu_ctx_factory, oracle):
    """Two iterations of the eight-term model at (400, 5): gradient_kernel is the three-call composition bit for bit; with
    no kernel gradient asked for the calls equal the old entries bit for bit; the old entries equal the existing
    restatement; the kernel gradient follows its own restatement."""
    import rovinasemanticsegmentation_amd as rv
    N, C, n = 400, 5, 2
    rng, U, terms = _model(4400, N, C, EIGHT_TERMS, compat_scale=0.05)
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    lr, kl = _restated(oracle, U, terms)
    gt = rng.integers(0, C, N).astype(np.int16)
    gt[::7] = -1
    obj = rv.LogLikelihood(gt, 0.01)
    value, ug, cg, kg, Qn = ctx.crf_model_gradient_kernel(n, obj, want_Q=True)
    assert kg.shape == (sum(kl.sizes()),) and kg.shape[0] == 2 + 9 + 1 + 0 + 16 + 4 + 5 + 0
    # the old entries, and the new ones without a kernel gradient
    value0, ug0, cg0, Q0 = ctx.crf_model_gradient(n, obj, want_Q=True)
    value1, ug1, cg1, none, Q1 = ctx.crf_model_gradient_kernel(n, obj, kernel=False, want_Q=True)
    assert none is None
    for x, y, z in ((ug, ug0, ug1), (cg, cg0, cg1), (Qn, Q0, Q1), (np.float64(value), np.float64(value0), np.float64(value1))):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    # the three-call composition
    Qs = [ctx.crf_model_start()]
    for _ in range(n):
        Qs.append(ctx.crf_model_step(Qs[-1]))
    v2, dq = ctx.crf_model_objective(obj, Qs[n])
    ug2, cg2, kg2 = ctx.crf_model_backward_kernel(np.stack(Qs), dq)
    assert np.float64(v2).tobytes() == np.float64(value).tobytes()
    assert ug2.tobytes() == ug.tobytes() and cg2.tobytes() == cg.tobytes() and kg2.tobytes() == kg.tobytes()
    ug3, cg3 = ctx.crf_model_backward(np.stack(Qs), dq)
    ug4, cg4, none = ctx.crf_model_backward_kernel(np.stack(Qs), dq, kernel=False)
    assert ug3.tobytes() == ug4.tobytes() == ug.tobytes() and cg3.tobytes() == cg4.tobytes() == cg.tobytes()
    # the restatements
    wvalue, wug, wcg, wQ, vS, cS = lr.gradient(n, (LC.LOGLIKELIHOOD, gt, 0.01, None))
    assert np.array_equal(Qn, wQ) and np.array_equal(ug, wug)
    _within(value, wvalue, vS, "value")
    _within(cg, wcg, cS, "compat gradient")
    wQs = lr.forward(n)
    wkg, kS = kl.backward(wQs, lr.objective((LC.LOGLIKELIHOOD, gt, 0.01, None), wQs[n])[1])
    _within(kg, wkg, kS, "kernel gradient")
    # zero iterations: zeros
    _, _, _, kg0, _ = ctx.crf_model_gradient_kernel(0, obj)
    assert kg0.shape == kg.shape and not kg0.any()


def test_python_facade(gpu_ctx_factory, oracle):
    """DenseCRF.kernelGradient and gradient(kernel=True): the C ABI's doubles rounded to fp32."""
    import rovinasemanticsegmentation_amd as rv
    N, C, n = 300, 4, 2
    specs = [(2, R.DIAGONAL, R.NORMALIZE_SYMMETRIC, R.FULL_KERNEL), (3, R.POTTS, R.NORMALIZE_AFTER, R.DIAG_KERNEL),
             (2, R.MATRIX, R.NORMALIZE_BEFORE, R.DIAG_KERNEL)]
    rng, U, terms = _model(4500, N, C, specs, compat_scale=0.2)
    ctx = gpu_ctx_factory()
    crf = rv.DenseCRF(ctx, N, C)
    crf.setUnaryEnergy(U)
    for f, c, p, kt, nt, kp in terms:
        crf.addPairwiseEnergy(f, M.compat_object(rv, c, np.asarray(p, f32), C), kt, nt)
    crf.setKernelParameters(np.concatenate([t[5] for t in terms]))
    gt = rng.integers(0, C, N).astype(np.int16)
    obj = rv.IntersectionOverUnion(gt)
    value, du, dl, dk = crf.gradient(n, obj, kernel=True)
    _set(ctx, rv, U, terms)
    v, ug, cg, kg, _ = ctx.crf_model_gradient_kernel(n, obj)
    assert value == v and dk.dtype == f32 and np.array_equal(dk, kg.astype(f32)) and np.array_equal(dl, cg.astype(f32))
    b, Q = rng.normal(size=(N, C)).astype(f32), ctx.crf_model_start()
    lr, kl = _restated(oracle, U, terms)
    for k in range(3):   # Diagonal, Potts, Matrix: lbl_Q is the library's own (compat_apply), bit for bit the restated one
        assert np.array_equal(ctx.crf_model_compat_apply(k, Q), kl.lbl_Q(k, Q)), k
        want = ctx.crf_model_kernel_gradient(k, b, kl.lbl_Q(k, Q))
        assert want.any() and np.array_equal(crf.kernelGradient(k, b, Q), want.astype(f32)), k


def test_refusals(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    from rovinasemanticsegmentation_amd import capi
    N, C = 64, 3
    rng, U, terms = _model(4600, N, C, [(2, R.POTTS, R.NORMALIZE_SYMMETRIC, R.DIAG_KERNEL)])
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    a = rng.random((N, C)).astype(f32)
    for term in (-1, 1):
        for call in (lambda: ctx.crf_model_lattice_gradient(term, a, a), lambda: ctx.crf_model_kernel_gradient(term, a, a)):
            with pytest.raises(capi.RvsegError) as e:
                call()
            assert e.value.status == capi.ERR_INVALID_ARG and "term" in str(e.value)
    df = np.empty((N, 2), f32)
    p = lambda x: x.ctypes.data   # noqa: E731
    for args in ((0, None, p(a), p(df)), (0, p(a), None, p(df)), (0, p(a), p(a), None)):
        assert ctx.L.rvseg_crf_model_lattice_gradient(ctx.h, *args) == capi.ERR_INVALID_ARG
    for args in ((0, None, p(a), None, p(df)), (0, p(a), None, None, p(df))):
        assert ctx.L.rvseg_crf_model_kernel_gradient(ctx.h, *args) == capi.ERR_INVALID_ARG
    ctx.crf_infer(U, terms[0][0], 1.0, 1)   # builds a lattice: the model is gone
    gt = np.zeros(N, np.int16)
    for call in (lambda: ctx.crf_model_lattice_gradient(0, a, a), lambda: ctx.crf_model_kernel_gradient(0, a, a),
                 lambda: ctx.crf_model_gradient_kernel(1, rv.LogLikelihood(gt)),
                 lambda: ctx.crf_model_backward_kernel(np.stack([a, a]), a)):
        with pytest.raises(capi.RvsegError) as e:
            call()
        assert e.value.status == capi.ERR_INVALID_ARG and "rvseg_crf_infer" in str(e.value)


def test_device_twins(gpu_ctx_factory):
    """The _device entries on torch buffers and a torch stream give the bits of the host entries."""
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    dev = torch.device("cuda", 0)
    N, C, d, n = 300, 5, 3, 2
    rng, U, terms = _model(4700, N, C, [(d, R.MATRIX, R.NORMALIZE_SYMMETRIC, R.FULL_KERNEL), (2, R.POTTS, R.NORMALIZE_BEFORE, R.DIAG_KERNEL)])
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    a, b = rng.normal(size=(N, C)).astype(f32), rng.random((N, C)).astype(f32)
    df = ctx.crf_model_lattice_gradient(0, a, b)
    grad, fg = ctx.crf_model_kernel_gradient(0, a, b, want_fg=True)
    Qs = [ctx.crf_model_start()]
    for _ in range(n):
        Qs.append(ctx.crf_model_step(Qs[-1]))
    ug, cg, kg = ctx.crf_model_backward_kernel(np.stack(Qs), a)
    gt = rng.integers(0, C, N).astype(np.int16)
    obj = rv.LogLikelihood(gt, 0.01)
    gv, gug, gcg, gkg, gQ = ctx.crf_model_gradient_kernel(n, obj, want_Q=True)
    lbl = ctx.crf_model_compat_apply(0, b)
    stream = torch.cuda.Stream(dev)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_a, d_b, d_Qs = up(a), up(b), up(np.stack(Qs))
    d_df = torch.zeros((N, d), dtype=torch.float32, device=dev)
    d_fg = torch.zeros((N, d), dtype=torch.float32, device=dev)
    d_grad = torch.ones(d * d, dtype=torch.float64, device=dev)
    d_ug = torch.zeros((N, C), dtype=torch.float32, device=dev)
    d_cg = torch.ones(cg.shape[0], dtype=torch.float64, device=dev)
    d_kg = torch.ones(kg.shape[0], dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    s = stream.cuda_stream
    ctx.crf_model_call_device("lattice_gradient", 0, d_a.data_ptr(), d_b.data_ptr(), d_df.data_ptr(), stream=s)
    ctx.crf_model_call_device("kernel_gradient", 0, d_a.data_ptr(), d_b.data_ptr(), d_grad.data_ptr(), d_fg.data_ptr(), stream=s)
    ctx.crf_model_call_device("backward_kernel", n, d_Qs.data_ptr(), d_a.data_ptr(), d_ug.data_ptr(), d_cg.data_ptr(), d_kg.data_ptr(), stream=s)
    # gradient_kernel_device: five distinct outputs, so a slip in the argument order cannot pass
    import ctypes
    d_gt = up(gt)
    rec, keep = obj.record(N, C, d_gt=d_gt.data_ptr())
    d_val = torch.zeros(1, dtype=torch.float64, device=dev)
    d_gug = torch.zeros((N, C), dtype=torch.float32, device=dev)
    d_gcg = torch.ones(cg.shape[0], dtype=torch.float64, device=dev)
    d_gkg = torch.ones(kg.shape[0], dtype=torch.float64, device=dev)
    d_gQ = torch.zeros((N, C), dtype=torch.float32, device=dev)
    d_lbl = torch.zeros((N, C), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.crf_model_call_device("gradient_kernel", n, ctypes.byref(rec), d_val.data_ptr(), d_gug.data_ptr(), d_gcg.data_ptr(), d_gkg.data_ptr(),
                              d_gQ.data_ptr(), stream=s)
    ctx.crf_model_call_device("compat_apply", 0, d_b.data_ptr(), d_lbl.data_ptr(), stream=s)
    stream.synchronize()
    del keep
    assert d_val.cpu().numpy().tobytes() == np.float64(gv).tobytes()
    assert np.array_equal(d_gug.cpu().numpy(), gug) and np.array_equal(d_gQ.cpu().numpy(), gQ) and np.array_equal(d_lbl.cpu().numpy(), lbl)
    assert d_gcg.cpu().numpy().tobytes() == gcg.tobytes() and d_gkg.cpu().numpy().tobytes() == gkg.tobytes() and gkg.any()
    assert np.array_equal(d_df.cpu().numpy(), df) and np.array_equal(d_fg.cpu().numpy(), fg)
    assert d_grad.cpu().numpy().tobytes() == grad.tobytes()
    assert np.array_equal(d_ug.cpu().numpy(), ug) and d_cg.cpu().numpy().tobytes() == cg.tobytes() and d_kg.cpu().numpy().tobytes() == kg.tobytes()


def test_growing_model_equals_a_fresh_context(gpu_ctx_factory):
    """Models (300, 4) -> (900, 21) -> (300, 4) on one context: every buffer grows and is reused; each equals a fresh context
    bit for bit."""
    import rovinasemanticsegmentation_amd as rv
    ctx = gpu_ctx_factory()
    for N, C in ((300, 4), (900, 21), (300, 4)):
        rng, U, terms = _model(4800 + N, N, C, [(3, R.DIAGONAL, R.NORMALIZE_SYMMETRIC, R.FULL_KERNEL), (5, R.POTTS, R.NORMALIZE_AFTER, R.DIAG_KERNEL)])
        gt = rng.integers(0, C, N).astype(np.int16)
        a, b = rng.normal(size=(N, C)).astype(f32), rng.random((N, C)).astype(f32)
        got = []
        for c in (ctx, gpu_ctx_factory()):
            _set(c, rv, U, terms)
            g, fg = c.crf_model_kernel_gradient(1, a, b, want_fg=True)
            _, ug, cg, kg, _ = c.crf_model_gradient_kernel(2, rv.LogLikelihood(gt))
            got.append((g, fg, ug, cg, kg))
        for x, y in zip(*got):
            assert x.tobytes() == y.tobytes(), (N, C)
