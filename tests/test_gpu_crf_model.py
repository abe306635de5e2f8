"""A kept DenseCRF model on the GPU (rvseg_crf_model_*[_device], Python DenseCRF): stepwise inference, apply, energies,
KL divergence, the traced inference and the model's lifetime, against the restatement in crf_model_cases.py.  Everything
fp32 is compared bit for bit; the KL parts (double) within crf_model_cases.KL_BOUND of the sum of their absolute terms."""
import numpy as np
import pytest

import crf_model_cases as M
import crf_restate as R

pytestmark = pytest.mark.gpu

NORMS = [R.NO_NORMALIZATION, R.NORMALIZE_BEFORE, R.NORMALIZE_AFTER, R.NORMALIZE_SYMMETRIC]
COMPATS = [R.POTTS, R.DIAGONAL, R.MATRIX]
EIGHT = [(1 + k % 7, COMPATS[k % 3], NORMS[k % 4]) for k in range(8)]
STEP_CASES = {
    "one term, fused C": (9, [(5, R.MATRIX, R.NORMALIZE_SYMMETRIC)]),
    "one term, unfused C": (11, [(5, R.DIAGONAL, R.NORMALIZE_BEFORE)]),
    "one Potts term, fused C": (12, [(6, R.POTTS, R.NORMALIZE_SYMMETRIC)]),
    "two terms": (9, [(2, R.POTTS, R.NORMALIZE_AFTER), (6, R.MATRIX, R.NORMALIZE_SYMMETRIC)]),
    "eight terms": (5, EIGHT),
    "no term": (7, []),
}


def _set(ctx, rv, U, terms):
    ctx.crf_model_set(U, M.api_terms(rv, terms, U.shape[1]))


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_start_and_steps_are_infer_terms(gpu_ctx_factory, oracle, case):
    import rovinasemanticsegmentation_amd as rv
    C, specs = STEP_CASES[case]
    _, U, terms = M.random_model(100 + C + len(specs), 700, C, specs)
    ctx, other = gpu_ctx_factory(), gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    Q = ctx.crf_model_start()
    for k in (0, 1, 2, 3):
        if k != 2:
            want, _ = other.crf_infer_terms(U, M.api_terms(rv, terms, C), k)   # on another context: the model stays
            assert np.array_equal(Q, want), k
        Q = ctx.crf_model_step(Q)
    assert np.array_equal(ctx.crf_model_step(ctx.crf_model_start(), 3), other.crf_infer_terms(U, M.api_terms(rv, terms, C), 3)[0])
    assert np.array_equal(ctx.crf_model_start(), R.crf_terms(oracle, U, terms, 0))
    assert np.array_equal(ctx.crf_model_step(ctx.crf_model_start(), 0), ctx.crf_model_start())


@pytest.mark.parametrize("case", ["one term, fused C", "two terms", "eight terms"])
def test_step_on_a_callers_q(gpu_ctx_factory, oracle, case):
    import rovinasemanticsegmentation_amd as rv
    C, specs = STEP_CASES[case]
    rng, U, terms = M.random_model(200 + C + len(specs), 500, C, specs)
    Q = (rng.random((500, C)) * 2).astype(np.float32)   # rows that do not sum to one
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    model = M.Model(oracle, U, terms)
    assert np.array_equal(ctx.crf_model_step(Q), model.step(Q))


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("compat", COMPATS)
def test_apply(gpu_ctx_factory, oracle, compat, norm):
    """C = 1, 2 (the sequential blur dispatch), 3, 64 x d = 1, 7, the point counts 1, 63, 64, 65, 1000 dealt over them."""
    import rovinasemanticsegmentation_amd as rv
    ctx = gpu_ctx_factory()
    Ns = [1, 63, 64, 65, 1000]
    i = COMPATS.index(compat) * 4 + norm
    for C in (1, 2, 3, 64):
        for d in (1, 7):
            N = Ns[i % 5]
            i += 1
            rng, U, terms = M.random_model(300 + 17 * i + C, N, C, [(d, compat, norm)])
            Q = (rng.random((N, C)) * 2).astype(np.float32)
            _set(ctx, rv, U, terms)
            assert np.array_equal(ctx.crf_model_apply(0, Q), M.Model(oracle, U, terms).apply(0, Q)), (C, d, N)


@pytest.mark.parametrize("case", ["one term, unfused C", "two terms", "eight terms", "no term"])
def test_energy(gpu_ctx_factory, oracle, case):
    import rovinasemanticsegmentation_amd as rv
    C, specs = STEP_CASES[case]
    N = 600
    rng, U, terms = M.random_model(400 + C + len(specs), N, C, specs)
    labels = rng.integers(0, C, N).astype(np.int8)
    labels[::7] = -1
    labels[3::11] = C
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    model = M.Model(oracle, U, terms)
    u, p = ctx.crf_model_energy(labels)
    assert np.array_equal(u, model.unary_energy(labels))
    assert np.array_equal(p, model.pairwise_energy(labels, -1))
    assert not u[::7].any() and not p[::7].any() and not u[3::11].any() and not p[3::11].any()
    acc = np.zeros(N, np.float32)
    for k in range(len(terms)):
        pk = ctx.crf_model_energy(labels, k, unary=False)[1]
        assert np.array_equal(pk, model.pairwise_energy(labels, k))
        acc = (acc + pk).astype(np.float32)
    assert np.array_equal(p, acc)
    # the map of an inference goes straight in
    Q, mp, _ = ctx.crf_model_trace(2)
    u2, p2 = ctx.crf_model_energy(mp)
    assert np.array_equal(u2, model.unary_energy(mp)) and np.array_equal(p2, model.pairwise_energy(mp, -1))


# (N, C): 256 / C points per block step -- exactly one block, two blocks, and 500 partials per part (the second stage
# has 256 threads); C = 3 leaves idle threads in a block
KL_SHAPES = [(4, 64), (5, 64), (2000, 64), (85, 3), (86, 3), (1000, 9)]


@pytest.mark.parametrize("N,C", KL_SHAPES)
def test_kl(gpu_ctx_factory, oracle, N, C):
    import rovinasemanticsegmentation_amd as rv
    specs = [(2, R.POTTS, R.NORMALIZE_SYMMETRIC), (5, R.MATRIX, R.NORMALIZE_AFTER)]
    rng, U, terms = M.random_model(500 + N + C, N, C, specs)
    Q = oracle.exp_and_normalize((rng.random((N, C)) * 4).astype(np.float32))
    Q[::3, 0] = 0.0   # exact zeros: q log max(q, 1e-20f) = 0
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    parts = ctx.crf_model_kl(Q)
    again = ctx.crf_model_kl(Q)
    assert parts.tobytes() == again.tobytes()
    want, S = M.Model(oracle, U, terms).kl_parts(Q)
    err = np.abs(parts - want)
    print("kl parts", parts, "restated", want, "error / S", err / S)
    assert (err <= M.KL_BOUND * S).all()
    assert np.isfinite(parts).all()


def test_trace(gpu_ctx_factory, oracle):
    """The traced inference runs the kernels of the general loop and of rvseg_crf_model_kl, so kl_out[it] is bit for bit
    rvseg_crf_model_kl of the stepped Q, and Q_out / map_out are rvseg_crf_infer_terms bit for bit (fused and general)."""
    import rovinasemanticsegmentation_amd as rv
    for case in ("one term, fused C", "two terms", "no term"):
        C, specs = STEP_CASES[case]
        _, U, terms = M.random_model(600 + C, 800, C, specs)
        ctx, other = gpu_ctx_factory(), gpu_ctx_factory()
        _set(ctx, rv, U, terms)
        Q, mp, kl = ctx.crf_model_trace(3, 1, C - 1)
        wantQ, wantm = other.crf_infer_terms(U, M.api_terms(rv, terms, C), 3, 1, C - 1)
        assert np.array_equal(Q, wantQ) and np.array_equal(mp, wantm)
        Qs = ctx.crf_model_start()
        for it in range(4):
            assert kl[it] == M.kl_sum(ctx.crf_model_kl(Qs)), (case, it)
            Qs = ctx.crf_model_step(Qs)
        assert ctx.crf_model_trace(0)[2].shape == (1,)


def test_lifetime(gpu_ctx_factory, oracle):
    import rovinasemanticsegmentation_amd as rv
    from rovinasemanticsegmentation_amd import _capi as capi
    C, specs = STEP_CASES["two terms"]
    rng, U, terms = M.random_model(700, 400, C, specs)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    with pytest.raises(capi.RvsegError) as e:
        a.crf_model_start()
    assert e.value.status == capi.ERR_INVALID_ARG and "rvseg_crf_model_set" in str(e.value)
    _set(a, rv, U, terms)
    _set(b, rv, U, terms)
    want = b.crf_model_step(b.crf_model_start(), 2)
    F = terms[1][0]
    replacers = [("rvseg_crf_infer", lambda: a.crf_infer(U, F, 3.0, 1)),
                 ("rvseg_lattice_build", lambda: a.lattice_build(F))]
    for name, call in replacers:
        call()
        for model_call in (a.crf_model_start, lambda: a.crf_model_step(want), lambda: a.crf_model_apply(0, want),
                           lambda: a.crf_model_energy(np.zeros(400, np.int8)), lambda: a.crf_model_kl(want), lambda: a.crf_model_trace(1)):
            with pytest.raises(capi.RvsegError) as e:
                model_call()
            assert e.value.status == capi.ERR_INVALID_ARG and name in str(e.value)
        assert np.array_equal(b.crf_model_step(b.crf_model_start(), 2), want)   # the other context's model is untouched
        _set(a, rv, U, terms)
        assert np.array_equal(a.crf_model_step(a.crf_model_start(), 2), want)
    # the refusals of rvseg_crf_terms_check reach model_set unchanged; argument refusals of the model calls
    for bad in ([(F, 3.0, rv.DIAG_KERNEL, 7, None)], [(F, 3.0, 5, rv.NORMALIZE_SYMMETRIC, None)],
                [(F, 3.0, rv.DIAG_KERNEL, rv.NORMALIZE_SYMMETRIC, None)] * 9):
        with pytest.raises(capi.RvsegError) as e:
            a.crf_model_set(U, bad)
        assert e.value.status == capi.ERR_INVALID_ARG
    assert np.array_equal(a.crf_model_step(a.crf_model_start(), 2), want)   # a refused model_set touched nothing
    for bad_call in (lambda: a.crf_model_apply(2, want), lambda: a.crf_model_apply(-1, want),
                     lambda: a.crf_model_energy(np.zeros(400, np.int8), 2), lambda: a.crf_model_step(want, -1)):
        with pytest.raises(capi.RvsegError) as e:
            bad_call()
        assert e.value.status == capi.ERR_INVALID_ARG
    assert np.array_equal(a.crf_model_step(a.crf_model_start(), 2), want)


def test_lifetime_after_a_frame_call(gpu_ctx_factory, oracle):
    import rovinasemanticsegmentation_amd as rv
    from rovinasemanticsegmentation_amd import _capi as capi, synthetic
    W, H = 160, 120
    ctx = gpu_ctx_factory(width=W, height=H, use_dense_crf=1, dcrf_iterations=1)
    ctx.forest_load(synthetic.make_forest_bytes(seed=1, n_trees=4, leaves_per_tree=256, max_depth=12))
    _, U, terms = M.random_model(800, 300, 4, [(3, R.POTTS, R.NORMALIZE_SYMMETRIC)])
    _set(ctx, rv, U, terms)
    Q = ctx.crf_model_start()
    rgb, depth = synthetic.make_batch(1, W, H, holes=True)
    ctx.segment_frames(rgb, depth, synthetic.make_calib(W, H))
    with pytest.raises(capi.RvsegError) as e:
        ctx.crf_model_step(Q)
    assert e.value.status == capi.ERR_INVALID_ARG and "rvseg_segment_frames" in str(e.value)


def test_python_densecrf(gpu_ctx_factory, oracle):
    import rovinasemanticsegmentation_amd as rv
    C, N = 9, 900
    rng, U, terms = M.random_model(900, N, C, [(2, R.POTTS, R.NORMALIZE_SYMMETRIC), (5, R.MATRIX, R.NORMALIZE_SYMMETRIC)])
    ctx = gpu_ctx_factory()
    crf = rv.DenseCRF(ctx, N, C)
    crf.setUnaryEnergy(U)
    for f, c, p, kt, nt, kp in terms:
        crf.addPairwiseEnergy(f, M.compat_object(rv, c, p, C), kt, nt)
    model = M.Model(oracle, U, terms)
    Q = crf.startInference()
    assert np.array_equal(Q, model.start())
    Q = crf.stepInference(Q)
    assert np.array_equal(Q, model.step(model.start()))
    Q3, mp = crf.inference(3)            # replaces the context's model; the next call sets it again
    assert np.array_equal(crf.stepInference(crf.stepInference(Q)), Q3)
    assert np.array_equal(crf.currentMap(Q3), mp)
    assert np.array_equal(crf.unaryEnergy(mp), model.unary_energy(mp))
    assert np.array_equal(crf.pairwiseEnergy(mp), model.pairwise_energy(mp, -1))
    assert np.array_equal(crf.pairwiseEnergy(mp, 1), model.pairwise_energy(mp, 1))
    kl, parts = crf.klDivergence(Q3, parts=True)
    want, S = model.kl_parts(Q3)
    assert (np.abs(parts - want) <= M.KL_BOUND * S).all()
    assert kl == M.kl_sum(parts) == crf.klDivergence(Q3)
    Qt, trace = crf.inference_trace(3)
    assert np.array_equal(Qt, Q3) and trace[3] == kl and trace.shape == (4,)
    # a parameter change sets the model again
    crf.setLabelCompatibilityParameters(crf.labelCompatibilityParameters() * np.float32(0.5))
    terms2 = [(f, c, k[1].array(C), kt, nt, kp) for (f, c, p, kt, nt, kp), k in zip(terms, crf.kernels)]   # (W is symmetric already)
    assert not np.array_equal(crf.stepInference(crf.startInference()), model.step(model.start()))
    assert np.array_equal(crf.stepInference(crf.startInference()), M.Model(oracle, U, terms2).step(model.start()))


def test_device_entries(gpu_ctx_factory, oracle):
    """The _device twins on torch buffers and a torch stream give the bits of the host entries."""
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    dev = torch.device("cuda", 0)
    C, N = 11, 700
    rng, U, terms = M.random_model(1000, N, C, [(3, R.DIAGONAL, R.NORMALIZE_BEFORE), (6, R.MATRIX, R.NORMALIZE_SYMMETRIC)])
    host, ctx = gpu_ctx_factory(), gpu_ctx_factory()
    _set(host, rv, U, terms)
    stream = torch.cuda.Stream(dev)
    d_U = torch.from_numpy(-U).to(dev)   # passed as -energy (unary_is_energy = 0)
    d_F = [torch.from_numpy(t[0]).to(dev) for t in terms]
    torch.cuda.synchronize(dev)
    dterms = [((t.data_ptr(), f.shape[1]), M.compat_object(rv, c, p, C), kt, nt, kp) for t, (f, c, p, kt, nt, kp) in zip(d_F, terms)]
    ctx.crf_model_set_device(N, C, dterms, d_U.data_ptr(), False, stream=stream.cuda_stream)
    d_U.zero_()
    for t in d_F:
        t.zero_()   # the caller's buffers are free once model_set has returned
    s = stream.cuda_stream
    d_Q = torch.zeros((N, C), dtype=torch.float32, device=dev)
    d_out = torch.zeros((N, C), dtype=torch.float32, device=dev)
    d_map = torch.zeros(N, dtype=torch.int8, device=dev)
    d_u = torch.zeros(N, dtype=torch.float32, device=dev)
    d_p = torch.zeros(N, dtype=torch.float32, device=dev)
    d_parts = torch.zeros(4, dtype=torch.float64, device=dev)
    d_kl = torch.zeros(3, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    ctx.crf_model_call_device("start", d_Q.data_ptr(), stream=s)
    ctx.crf_model_call_device("step", d_Q.data_ptr(), 2, stream=s)
    ctx.crf_model_call_device("apply", 1, d_Q.data_ptr(), d_out.data_ptr(), stream=s)
    ctx.crf_model_call_device("kl", d_Q.data_ptr(), d_parts.data_ptr(), stream=s)
    stream.synchronize()
    Q2 = host.crf_model_step(host.crf_model_start(), 2)
    assert np.array_equal(d_Q.cpu().numpy(), Q2)
    assert np.array_equal(d_out.cpu().numpy(), host.crf_model_apply(1, Q2))
    assert d_parts.cpu().numpy().tobytes() == host.crf_model_kl(Q2).tobytes()
    ctx.crf_model_call_device("trace", 2, d_Q.data_ptr(), d_map.data_ptr(), 3, 0, d_kl.data_ptr(), stream=s)
    ctx.crf_model_call_device("energy", d_map.data_ptr(), -1, d_u.data_ptr(), d_p.data_ptr(), stream=s)
    stream.synchronize()
    Qh, mh, klh = host.crf_model_trace(2)
    assert np.array_equal(d_Q.cpu().numpy(), Qh) and np.array_equal(d_map.cpu().numpy(), mh)
    assert d_kl.cpu().numpy().tobytes() == klh.tobytes()
    uh, ph = host.crf_model_energy(mh)
    assert np.array_equal(d_u.cpu().numpy(), uh) and np.array_equal(d_p.cpu().numpy(), ph)
    assert "kl" in ctx.last_timing()   # the traced inference marks its KL passes
