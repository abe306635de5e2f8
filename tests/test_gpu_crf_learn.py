"""Learning on a kept DenseCRF model on the GPU (rvseg_crf_model_apply_transpose / _objective / _backward / _gradient /
_set_compat / _set_unary, rvseg_crf_logistic_gradient, Python DenseCRF.gradient and CRFEnergy) against the restatement in
crf_learn_cases.py on the CPU oracle's lattice.  Everything fp32 is compared bit for bit (IoU's d_mul_Q within one ulp);
every double within crf_learn_cases.KL_BOUND of the sum of its absolute terms."""
import os

import numpy as np
import pytest

import crf_learn_cases as LC
import crf_model_cases as M
import crf_restate as R

pytestmark = pytest.mark.gpu

NORMS = [R.NO_NORMALIZATION, R.NORMALIZE_BEFORE, R.NORMALIZE_AFTER, R.NORMALIZE_SYMMETRIC]
COMPATS = [R.POTTS, R.DIAGONAL, R.MATRIX]
f32 = np.float32


def _set(ctx, rv, U, terms):
    ctx.crf_model_set(U, M.api_terms(rv, terms, U.shape[1]))


def _objective(rv, obj):
    kind, gt, robust, cw = obj
    if kind == LC.LOGLIKELIHOOD:
        return rv.LogLikelihood(gt, robust)
    return rv.Hamming(gt, cw) if kind == LC.HAMMING else rv.IntersectionOverUnion(gt)


def _gt(rng, N, C):
    gt = rng.integers(0, C, N).astype(np.int16)
    gt[::7] = -1
    gt[3::11] = C + 2
    return gt


def _objectives(rng, N, C):
    gt = _gt(rng, N, C)
    return {"loglikelihood": (LC.LOGLIKELIHOOD, gt, 0.0, None), "loglikelihood robust": (LC.LOGLIKELIHOOD, gt, 0.01, None),
            "hamming": (LC.HAMMING, gt, 0.0, rng.uniform(0.1, 1.0, C).astype(f32)), "iou": (LC.IOU, gt, 0.0, None)}


def _within(got, want, S, what):
    got, want, S = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(S)
    assert (S > 0).all(), what + ": an entry without terms checks nothing"
    err = np.abs(got - want)
    print("%s: max error / S = %.3g (bound %.1g)" % (what, (err / S).max(), LC.KL_BOUND))
    assert (err <= LC.KL_BOUND * S).all(), what


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("compat", COMPATS)
def test_apply_transpose(gpu_ctx_factory, oracle, compat, norm):
    """C = 2 (the double-precision blur), 3, 9, 21 x d = 2, 5 at N = 997 (no multiple of 4 or of 256 / C), bit for bit."""
    import rovinasemanticsegmentation_amd as rv
    ctx = gpu_ctx_factory()
    N = 997
    for C in (2, 3, 9, 21):
        for d in (2, 5):
            rng, U, terms = M.random_model(1300 + 31 * C + d + 7 * norm + compat, N, C, [(d, compat, norm)])
            x = rng.normal(size=(N, C)).astype(f32)
            _set(ctx, rv, U, terms)
            lr = LC.Learn.of_model(M.Model(oracle, U, terms))
            assert np.array_equal(ctx.crf_model_apply_transpose(0, x), lr.apply_transpose(0, x)), (C, d)


def test_apply_transpose_swaps_before_and_after(gpu_ctx_factory, oracle):
    """Transposed, NORMALIZE_BEFORE scales the output and NORMALIZE_AFTER the input (pairwise.cpp:65, :78), and the blur runs
    its axes backwards: neither equals apply."""
    import rovinasemanticsegmentation_amd as rv
    N, C, d = 997, 3, 5
    rng, U, terms = M.random_model(1400, N, C, [(d, R.POTTS, R.NORMALIZE_BEFORE), (d, R.POTTS, R.NORMALIZE_AFTER)])
    terms[1] = (terms[0][0],) + terms[1][1:]   # the same features: the same lattice and norm
    terms[1] = terms[1][:2] + (terms[0][2],) + terms[1][3:]
    x = rng.normal(size=(N, C)).astype(f32)
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    model = M.Model(oracle, U, terms)
    lat, nrm = model.built[0][0], model.built[0][1]
    w = f32(-terms[0][2][0])
    tb, ta = ctx.crf_model_apply_transpose(0, x), ctx.crf_model_apply_transpose(1, x)
    assert np.array_equal(tb, (w * (lat.compute(x, reverse=True) * nrm[:, None]).astype(f32)).astype(f32))
    assert np.array_equal(ta, (w * lat.compute((x * nrm[:, None]).astype(f32), reverse=True)).astype(f32))
    for k, t in ((0, tb), (1, ta)):
        assert not np.array_equal(t, ctx.crf_model_apply(k, x))
    assert not np.array_equal(tb, ctx.crf_model_apply(1, x)) and not np.array_equal(ta, ctx.crf_model_apply(0, x))


# (N, C): one block, idle threads (C = 9), C = 64, and more points than 512 blocks of 256 / C take in one step
@pytest.mark.parametrize("N,C", [(1000, 9), (300, 64), (4100, 32)])
def test_objectives(gpu_ctx_factory, oracle, N, C):
    """Every sum of a value has at most N <= LEARN_MAX_TERMS terms (one per point; IoU: per class)."""
    import rovinasemanticsegmentation_amd as rv
    assert N <= LC.LEARN_MAX_TERMS
    rng, U, terms = M.random_model(1500 + N, N, C, [(2, R.POTTS, R.NORMALIZE_SYMMETRIC)])
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    lr = LC.Learn.of_model(M.Model(oracle, U, terms))
    Q = oracle.exp_and_normalize((rng.random((N, C)) * 4).astype(f32))
    Q[::5, 0] = 0.0   # exact zeros: max(q + robust, 1e-20f)
    for name, obj in _objectives(rng, N, C).items():
        value, dq = ctx.crf_model_objective(_objective(rv, obj), Q)
        again, dq2 = ctx.crf_model_objective(_objective(rv, obj), Q)
        assert np.float64(value).tobytes() == np.float64(again).tobytes() and np.array_equal(dq, dq2)
        want, wdq, S = lr.objective(obj, Q)
        _within(value, want, S, name)
        gt = obj[1]
        assert not dq[(gt < 0) | (gt >= C)].any()
        if obj[0] == LC.IOU:
            assert (np.abs(dq.astype(np.float64) - wdq.astype(np.float64)) <= np.spacing(np.maximum(np.abs(dq), np.abs(wdq)))).all()
            assert (dq != 0).sum() > N
        else:
            assert np.array_equal(dq, wdq), name
            assert np.count_nonzero(dq) <= N


BACKWARD_CASES = {
    # name: (N, C, [(d, compat, norm)], iterations, K of the logistic features)
    "no iteration": (600, 5, [(2, R.POTTS, R.NORMALIZE_SYMMETRIC), (5, R.MATRIX, R.NORMALIZE_SYMMETRIC)], 0, 4),
    "one term, one iteration": (600, 9, [(3, R.DIAGONAL, R.NORMALIZE_BEFORE)], 1, 4),
    "two classes": (500, 2, [(2, R.MATRIX, R.NORMALIZE_SYMMETRIC), (4, R.POTTS, R.NORMALIZE_AFTER)], 3, 3),
    "three terms": (700, 7, [(2, R.POTTS, R.NO_NORMALIZATION), (5, R.MATRIX, R.NORMALIZE_AFTER), (3, R.DIAGONAL, R.NORMALIZE_SYMMETRIC)], 3, 70),
    "64 classes": (300, 64, [(5, R.MATRIX, R.NORMALIZE_SYMMETRIC)], 1, 5),
    # more points than any reduction's blocks take in one step: 512 x (256 / 32) = 4096 (class sums, objective),
    # 128 tiles x (1024 / 32) = 4096 (pair sums)
    "past every block cap": (4100, 32, [(2, R.POTTS, R.NORMALIZE_SYMMETRIC), (3, R.DIAGONAL, R.NORMALIZE_BEFORE), (5, R.MATRIX, R.NORMALIZE_SYMMETRIC)],
                             1, 33),
    "no term": (400, 4, [], 2, 2),
}


@pytest.mark.parametrize("case", list(BACKWARD_CASES))
def test_backward(gpu_ctx_factory, oracle, case):
    """A caller's random d_mul_Q: unary_grad bit for bit; every compat_grad and logistic entry within KL_BOUND x the sum of
    its absolute terms (at most N terms per iteration and entry, N <= LEARN_MAX_TERMS)."""
    import rovinasemanticsegmentation_amd as rv
    N, C, specs, n, K = BACKWARD_CASES[case]
    assert N * (n + 1) <= LC.LEARN_MAX_TERMS
    rng, U, terms = M.random_model(1600 + N + C, N, C, specs)
    terms = [t[:2] + ((t[2] * f32(0.25)).astype(f32),) + t[3:] for t in terms]   # keeps three iterations away from one-hot marginals
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    lr = LC.Learn.of_model(M.Model(oracle, U, terms))
    Qs = lr.forward(n)
    dq = (rng.normal(size=(N, C)) * 0.1).astype(f32)
    ug, cg = ctx.crf_model_backward(np.stack(Qs), dq)
    wug, wcg, S = lr.backward(Qs, dq)
    assert np.array_equal(ug, wug)
    assert cg.shape == wcg.shape == (sum(LC.n_compat_params(c, C) for _, c, _ in specs),)
    if n > 0 and specs:
        _within(cg, wcg, S, "compat_grad")
    else:
        assert not cg.any()
    ug2, cg2 = ctx.crf_model_backward(np.stack(Qs), dq)
    assert np.array_equal(ug, ug2) and cg.tobytes() == cg2.tobytes()
    assert ctx.crf_model_backward(np.stack(Qs), dq, lbl_cmp=False)[1] is None
    assert np.array_equal(ctx.crf_model_backward(np.stack(Qs), dq, unary=False)[1], cg)
    f = rng.uniform(-1.0, 1.0, (N, K)).astype(f32)
    lg = ctx.crf_logistic_gradient(ug, f)
    wlg, lS = LC.logistic_gradient(ug, f)
    _within(lg, wlg, lS, "logistic_gradient")
    assert lg.tobytes() == ctx.crf_logistic_gradient(ug, f).tobytes()


def test_gradient_is_the_composition(gpu_ctx_factory, oracle):
    import rovinasemanticsegmentation_amd as rv
    N, C, n = 700, 5, 3
    rng, U, terms = M.random_model(1700, N, C, [(2, R.POTTS, R.NORMALIZE_SYMMETRIC), (5, R.MATRIX, R.NORMALIZE_BEFORE)])
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    lr = LC.Learn.of_model(M.Model(oracle, U, terms))
    for name, obj in _objectives(rng, N, C).items():
        o = _objective(rv, obj)
        value, ug, cg, Q = ctx.crf_model_gradient(n, o, want_Q=True)
        Qs = [ctx.crf_model_start()]
        for _ in range(n):
            Qs.append(ctx.crf_model_step(Qs[-1]))
        v2, dq = ctx.crf_model_objective(o, Qs[n])
        ug2, cg2 = ctx.crf_model_backward(np.stack(Qs), dq)
        assert np.array_equal(Q, Qs[n]) and np.float64(value).tobytes() == np.float64(v2).tobytes(), name
        assert np.array_equal(ug, ug2) and cg.tobytes() == cg2.tobytes(), name
        again = ctx.crf_model_gradient(n, o, want_Q=True)
        assert np.float64(again[0]).tobytes() == np.float64(value).tobytes() and np.array_equal(again[1], ug)
        assert again[2].tobytes() == cg.tobytes() and np.array_equal(again[3], Q)
        wv, wug, wcg, wQ, vS, S = lr.gradient(n, obj)
        assert np.array_equal(Q, wQ)
        _within(value, wv, vS, name + " value")
        if obj[0] != LC.IOU:   # (IoU's d_mul_Q may differ from the restated one by an ulp, which the backward pass carries on)
            assert np.array_equal(ug, wug)
            _within(cg, wcg, S, name + " compat_grad")
    v0, ug0, cg0, Q0 = ctx.crf_model_gradient(0, _objective(rv, obj), want_Q=True)
    assert np.array_equal(Q0, ctx.crf_model_start()) and not cg0.any()
    assert ctx.crf_model_gradient(1, o, unary=False, lbl_cmp=False)[1:] == (None, None, None)


def test_set_compat_and_set_unary_equal_a_fresh_model(gpu_ctx_factory, oracle):
    """After the in-place updates, step, apply and gradient give the bits of a model set afresh with the new values, and
    nothing was built: the context's schedule record (rewritten by every lattice build) has not changed, and the Python
    DenseCRF has not called crf_model_set again."""
    import rovinasemanticsegmentation_amd as rv
    N, C = 600, 6
    specs = [(2, R.POTTS, R.NORMALIZE_SYMMETRIC), (5, R.MATRIX, R.NORMALIZE_AFTER), (3, R.DIAGONAL, R.NORMALIZE_SYMMETRIC)]
    rng, U, terms = M.random_model(1800, N, C, specs)
    new = [(f, c, M.compat_params(rng, c, C), kt, nt, kp) for f, c, p, kt, nt, kp in terms]
    new[2] = new[2][:2] + (np.full(C, -1.5, f32),) + new[2][3:]   # a Diagonal that has become uniform: the Potts path
    U2 = (rng.random((N, C)) * 2).astype(f32)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    _set(a, rv, U, terms)
    before = a.last_schedule()
    for k, t in enumerate(M.api_terms(rv, new, C)):
        a.crf_model_set_compat(k, t[1])
    a.crf_model_set_unary(-U2, unary_is_energy=False)
    assert a.last_schedule() == before
    _set(b, rv, U2, new)
    obj = rv.LogLikelihood(_gt(rng, N, C), 0.01)
    x = rng.normal(size=(N, C)).astype(f32)
    assert np.array_equal(a.crf_model_step(a.crf_model_start(), 2), b.crf_model_step(b.crf_model_start(), 2))
    for k in range(3):
        assert np.array_equal(a.crf_model_apply(k, x), b.crf_model_apply(k, x))
        assert np.array_equal(a.crf_model_apply_transpose(k, x), b.crf_model_apply_transpose(k, x))
    ga, gb = a.crf_model_gradient(2, obj, want_Q=True), b.crf_model_gradient(2, obj, want_Q=True)
    assert ga[0] == gb[0] and np.array_equal(ga[1], gb[1]) and ga[2].tobytes() == gb[2].tobytes() and np.array_equal(ga[3], gb[3])
    assert not np.array_equal(b.crf_model_start(), M.Model(oracle, U, terms).start())
    # the Python facade: parameter changes on its own live model go in place
    crf = rv.DenseCRF(a, N, C)
    crf.setUnaryEnergy(U)
    for f, c, p, kt, nt, kp in terms:
        crf.addPairwiseEnergy(f, M.compat_object(rv, c, p, C), kt, nt)
    calls = []
    real = a.crf_model_set
    a.crf_model_set = lambda *args, **kw: (calls.append(1), real(*args, **kw))[1]
    Q1 = crf.stepInference(crf.startInference())
    assert len(calls) == 1
    crf.setLabelCompatibilityParameters(np.concatenate([rv.PottsCompatibility(new[0][2][0]).parameters(),
                                                        rv.MatrixCompatibility(new[1][2].reshape(C, C)).parameters(), new[2][2]]))
    Q2 = crf.stepInference(crf.startInference())
    assert len(calls) == 1 and not np.array_equal(Q1, Q2)
    _set(b, rv, U, new)
    assert np.array_equal(Q2, b.crf_model_step(b.crf_model_start()))


def test_refusals(gpu_ctx_factory, oracle):
    import rovinasemanticsegmentation_amd as rv
    from rovinasemanticsegmentation_amd import _capi as capi
    N, C = 300, 4
    rng, U, terms = M.random_model(1900, N, C, [(2, R.POTTS, R.NORMALIZE_SYMMETRIC), (3, R.DIAGONAL, R.NORMALIZE_SYMMETRIC)])
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    Q = ctx.crf_model_start()
    gt = _gt(rng, N, C)
    obj = rv.IntersectionOverUnion(gt)

    def refused(call, word):
        with pytest.raises(capi.RvsegError) as e:
            call()
        assert e.value.status == capi.ERR_INVALID_ARG and word in str(e.value), str(e.value)

    for call in (lambda: ctx.crf_model_apply_transpose(2, Q), lambda: ctx.crf_model_apply_transpose(-1, Q),
                 lambda: ctx.crf_model_set_compat(2, 1.0)):
        refused(call, "no such term")

    class Bad(rv.IntersectionOverUnion):
        kind = 7

    class NoWeights(rv.Hamming):
        def weights(self, M):
            return None
    for bad in (Bad(gt), NoWeights(gt, 0.0), rv.LogLikelihood(gt, float("nan"))):
        refused(lambda: ctx.crf_model_objective(bad, Q), "objective")
        refused(lambda: ctx.crf_model_gradient(1, bad), "objective")
    refused(lambda: ctx.crf_model_gradient(-1, obj), "bad arguments")
    assert np.array_equal(ctx.crf_model_start(), Q)   # the refused calls left the model alone
    ctx.lattice_build(terms[0][0])                    # ends the model
    for call in (lambda: ctx.crf_model_apply_transpose(0, Q), lambda: ctx.crf_model_objective(obj, Q),
                 lambda: ctx.crf_model_backward(Q[None], Q), lambda: ctx.crf_model_gradient(1, obj),
                 lambda: ctx.crf_model_set_compat(0, 1.0), lambda: ctx.crf_model_set_unary(U)):
        refused(call, "rvseg_lattice_build")
    assert ctx.crf_logistic_gradient(Q, U).shape == (C * C,)   # needs no model


def test_device_entries(gpu_ctx_factory, oracle):
    """Every _device twin on torch buffers and a torch stream gives the bits of its host entry."""
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    dev = torch.device("cuda", 0)
    N, C, n, K = 700, 6, 2, 3
    rng, U, terms = M.random_model(2000, N, C, [(3, R.DIAGONAL, R.NORMALIZE_BEFORE), (5, R.MATRIX, R.NORMALIZE_SYMMETRIC)])
    host, ctx = gpu_ctx_factory(), gpu_ctx_factory()
    _set(host, rv, U, terms)
    _set(ctx, rv, (U * f32(0.5)).astype(f32), terms)
    gt = _gt(rng, N, C)
    hobj = rv.Hamming(gt, rng.uniform(0.1, 1.0, C).astype(f32))
    x = rng.normal(size=(N, C)).astype(f32)
    f = rng.uniform(-1, 1, (N, K)).astype(f32)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_U, d_x, d_f, d_gt, d_w = t(U), t(x), t(f), t(gt), t(hobj.weights(C))
    d_out = torch.zeros((N, C), dtype=torch.float32, device=dev)
    d_Q = torch.zeros((N, C), dtype=torch.float32, device=dev)
    d_dq = torch.zeros((N, C), dtype=torch.float32, device=dev)
    d_ug = torch.zeros((N, C), dtype=torch.float32, device=dev)
    d_ug2 = torch.zeros((N, C), dtype=torch.float32, device=dev)
    n_cg = C + C * (C + 1) // 2
    d_cg = torch.ones(n_cg, dtype=torch.float64, device=dev)
    d_cg2 = torch.ones(n_cg, dtype=torch.float64, device=dev)
    d_val = torch.zeros(2, dtype=torch.float64, device=dev)
    d_lg = torch.zeros(C * K, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    rec, keep = hobj.record(N, C, d_gt.data_ptr(), d_w.data_ptr())
    import ctypes
    ctx.crf_model_call_device("set_unary", d_U.data_ptr(), 1, stream=s)
    ctx.crf_model_call_device("apply_transpose", 1, d_x.data_ptr(), d_out.data_ptr(), stream=s)
    ctx.crf_model_call_device("gradient", n, ctypes.byref(rec), d_val.data_ptr(), d_ug.data_ptr(), d_cg.data_ptr(), d_Q.data_ptr(), stream=s)
    ctx.crf_model_call_device("objective", ctypes.byref(rec), d_Q.data_ptr(), d_val.data_ptr() + 8, d_dq.data_ptr(), stream=s)
    ctx.crf_logistic_gradient_device(N, C, K, d_ug.data_ptr(), d_f.data_ptr(), d_lg.data_ptr(), stream=s)
    stream.synchronize()
    value, ug, cg, Q = host.crf_model_gradient(n, hobj, want_Q=True)
    assert np.array_equal(d_out.cpu().numpy(), host.crf_model_apply_transpose(1, x))
    assert d_val.cpu().numpy()[0] == value and np.array_equal(d_ug.cpu().numpy(), ug) and np.array_equal(d_Q.cpu().numpy(), Q)
    assert d_cg.cpu().numpy().tobytes() == cg.tobytes()
    v2, dq = host.crf_model_objective(hobj, Q)
    assert d_val.cpu().numpy()[1] == v2 == value and np.array_equal(d_dq.cpu().numpy(), dq)
    assert d_lg.cpu().numpy().tobytes() == host.crf_logistic_gradient(ug, f).tobytes()
    Qs = [host.crf_model_start()]
    for _ in range(n):
        Qs.append(host.crf_model_step(Qs[-1]))
    d_Qall = t(np.stack(Qs))
    torch.cuda.synchronize(dev)
    ctx.crf_model_call_device("backward", n, d_Qall.data_ptr(), d_dq.data_ptr(), d_ug2.data_ptr(), d_cg2.data_ptr(), stream=s)
    stream.synchronize()
    assert np.array_equal(d_ug2.cpu().numpy(), ug) and d_cg2.cpu().numpy().tobytes() == cg.tobytes()
    del keep


def _same_bits(a, b):
    a, b = (v if isinstance(v, tuple) else (v,) for v in (a, b))
    return len(a) == len(b) and all((p is None) == (q is None) and (p is None or np.asarray(p).tobytes() == np.asarray(q).tobytes())
                                    for p, q in zip(a, b))


@pytest.mark.parametrize("C", [2, 11])   # C = 2: the sequential blur
def test_entries_leave_each_other_alone(gpu_ctx_factory, C):
    """The host entries share the model's staging and work memory.  On one context with a two-term model every host entry
    runs once, then all run again in reverse order with a _device step and a _device backward on a torch stream among
    them: every output must equal its first value bit for bit, and that of the same call as the only one on a fresh
    context.  The inputs are the same arrays throughout, none of them an output of another entry."""
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    N, n = 300, 2
    rng, U, terms = M.random_model(2100 + C, N, C, [(3, R.DIAGONAL, R.NORMALIZE_BEFORE), (5, R.MATRIX, R.NORMALIZE_SYMMETRIC)])

    def marginals(*shape):
        e = np.exp(rng.normal(size=shape + (C,)))
        return np.ascontiguousarray(e / e.sum(-1, keepdims=True), f32)
    Q, Q_all = marginals(N), marginals(n + 1, N)
    x = rng.normal(size=(N, C)).astype(f32)
    dq = (rng.normal(size=(N, C)) * 0.1).astype(f32)
    labels = rng.integers(0, C, N).astype(np.int8)
    obj = rv.Hamming(_gt(rng, N, C), rng.uniform(0.1, 1.0, C).astype(f32))
    entries = [
        ("start", lambda c: c.crf_model_start()),
        ("step", lambda c: c.crf_model_step(Q, 2)),
        ("apply", lambda c: c.crf_model_apply(1, x)),
        ("apply_transpose", lambda c: c.crf_model_apply_transpose(0, x)),
        ("energy, unary only", lambda c: c.crf_model_energy(labels, pairwise=False)),
        ("energy, pairwise only", lambda c: c.crf_model_energy(labels, term=1, unary=False)),
        ("energy", lambda c: c.crf_model_energy(labels)),
        ("kl", lambda c: c.crf_model_kl(Q)),
        ("trace", lambda c: c.crf_model_trace(n, label_mode=3, unknown_label=C)),
        ("objective", lambda c: c.crf_model_objective(obj, Q)),
        ("backward, no unary_grad", lambda c: c.crf_model_backward(Q_all, dq, unary=False)),
        ("backward, no compat_grad", lambda c: c.crf_model_backward(Q_all, dq, lbl_cmp=False)),
        ("backward", lambda c: c.crf_model_backward(Q_all, dq)),
        ("gradient with Q", lambda c: c.crf_model_gradient(n, obj, want_Q=True)),
        ("gradient", lambda c: c.crf_model_gradient(n, obj)),
    ]
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    first = {name: call(ctx) for name, call in entries}
    assert first["backward, no unary_grad"][0] is None and first["backward, no compat_grad"][1] is None and first["gradient"][3] is None
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    d_Q, d_Qall, d_dq = (torch.from_numpy(a).to(dev) for a in (Q, Q_all, dq))
    d_ug = torch.zeros((N, C), dtype=torch.float32, device=dev)
    d_cg = torch.ones(C + C * (C + 1) // 2, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    for k, (name, call) in enumerate(reversed(entries)):
        if k == len(entries) // 2:
            ctx.crf_model_call_device("step", d_Q.data_ptr(), 2, stream=stream.cuda_stream)
            ctx.crf_model_call_device("backward", n, d_Qall.data_ptr(), d_dq.data_ptr(), d_ug.data_ptr(), d_cg.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
        assert _same_bits(call(ctx), first[name]), name + " after the others"
    assert _same_bits(d_Q.cpu().numpy(), first["step"]) and _same_bits((d_ug.cpu().numpy(), d_cg.cpu().numpy()), first["backward"])
    for name, call in entries:
        fresh = gpu_ctx_factory()
        _set(fresh, rv, U, terms)
        assert _same_bits(call(fresh), first[name]), name + " on a fresh context"
        fresh.close()


def _labeling(anno, M):
    """getLabeling (examples/common.cpp:49-66): colours in order of appearance, black = unlabelled (-1)."""
    col = anno[:, 0].astype(np.int64) | (anno[:, 1].astype(np.int64) << 8) | (anno[:, 2].astype(np.int64) << 16)
    colors, out = [], np.empty(col.shape[0], np.int16)
    for k, c in enumerate(col):
        if c and c not in colors and len(colors) < M:
            colors.append(c)
        out[k] = colors.index(c) if c in colors else -1
    return out


def test_learning_smoke(gpu_ctx_factory, oracle, golden_dir):
    """The model of examples/dense_learning.cpp:116-134 on a 64 x 48 crop of im2.ppm / anno2.ppm, M = 4: ten plain
    gradient-descent steps on CRFEnergy over the pairwise parameters.  The energy must end below its start, and every
    step's (value, dx) must match the restatement: the value within KL_BOUND x the sum of its absolute terms, dx -- the
    library's double rounded to fp32 once by the facade -- within KL_BOUND x S + 2^-24 |dx| of the restated double."""
    import rovinasemanticsegmentation_amd as rv
    from test_oracle_crf import read_ppm
    W, H, Mc, x0 = 64, 48, 4, 32
    im = np.ascontiguousarray(read_ppm(os.path.join(golden_dir, "im2.ppm"))[:H, x0:x0 + W])
    anno = np.ascontiguousarray(read_ppm(os.path.join(golden_dir, "anno2.ppm"))[:H, x0:x0 + W])
    N = W * H
    gt = _labeling(anno.reshape(N, 3), Mc)
    assert len(set(gt[gt >= 0])) >= 2
    feat = np.ones((N, 4), f32)
    feat[:, :3] = (im.reshape(N, 3) / 255.).astype(f32)
    L = (0.01 * (1 - 2 * np.random.default_rng(2013).random((Mc, 4)))).astype(f32)
    ctx = gpu_ctx_factory()
    crf = rv.DenseCRF(ctx, N, Mc)
    crf.setUnaryEnergy(L, feat)
    crf.addPairwiseGaussian(W, H, 3, 3, rv.PottsCompatibility(1))
    crf.addPairwiseBilateral(W, H, 80, 80, 13, 13, 13, im, rv.MatrixCompatibility(np.eye(Mc, dtype=f32)))
    objective = rv.LogLikelihood(gt, 0.01)
    obj = (LC.LOGLIKELIHOOD, gt, 0.01, None)
    energy = rv.CRFEnergy(crf, objective, 5, unary=False, pairwise=True)
    # the restatement: lattices and norms once, the compatibilities of the step's x
    U = R.logistic_unary(L, feat)
    assert np.array_equal(U, ctx.crf_logistic_unary(L, feat))
    fg, fb = rv.capi.crf_features_gaussian(W, H, 3, 3), rv.capi.crf_features_bilateral(W, H, 80, 80, 13, 13, 13, im)
    model = M.Model(oracle, U, [(fg, R.POTTS, [1.0], R.DIAG_KERNEL, R.NORMALIZE_SYMMETRIC, None),
                                (fb, R.MATRIX, np.eye(Mc, dtype=f32), R.DIAG_KERNEL, R.NORMALIZE_SYMMETRIC, None)])
    x = energy.initialValue()
    assert x.shape == (1 + Mc * (Mc + 1) // 2,)
    values = []
    for step in range(11):
        value, dx = energy.gradient(x)
        W_ = rv.MatrixCompatibility(np.eye(Mc, dtype=f32))
        W_.setParameters(x[1:])
        built = [model.built[0][:3] + ([x[0]],) + model.built[0][4:], model.built[1][:3] + (W_.W.copy(),) + model.built[1][4:]]
        wv, _, wcg, _, vS, S = LC.Learn(U, built, f32, oracle.exp_and_normalize).gradient(5, obj)
        _within(-value, wv, vS, "step %d value" % step)
        assert (S > 0).all()
        err = np.abs(dx.astype(np.float64) + wcg)
        assert (err <= LC.KL_BOUND * S + 2.0 ** -24 * np.abs(wcg)).all(), step
        values.append(value)
        x = (x - f32(2.0) * dx).astype(f32)
    print("energy per step:", values)
    assert values[10] < values[0]
