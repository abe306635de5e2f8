"""The kept DenseCRF model (rvseg_crf_model_*) and learning on it at the limits of their kernels: the capped grids of the KL
passes, ten KL parts, the sequential blur and C = 1, every compatibility x normalisation, the clamps, labels at the edge of
int8 and of C, N below one block step, eight terms in the backward pass, the 64-column blocks of the logistic gradient,
degenerate ground truths and regrown model buffers.

The acceptance rule is that of test_gpu_crf_model.py / test_gpu_crf_learn.py: everything fp32 bit for bit with the
restatement (crf_model_cases.py / crf_learn_cases.py on the CPU oracle's lattice), IoU's d_mul_Q within one ulp, every
double within KL_BOUND x the sum of its absolute terms -- and every double identical in all 64 bits on a second call."""
import os
import re

import numpy as np
import pytest

import crf_learn_cases as LC
import crf_model_cases as M
import crf_restate as R
from test_gpu_crf_learn import _objective, _same_bits, _within
from test_gpu_crf_model import COMPATS, EIGHT, NORMS

pytestmark = pytest.mark.gpu

f32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rovinasemanticsegmentation_amd", "csrc")
TWO = [(2, R.POTTS, R.NORMALIZE_SYMMETRIC), (5, R.MATRIX, R.NORMALIZE_AFTER)]


def _constant(header, name):
    """`constexpr int name = value;` of a kernel header: the tests state their premises in the kernels' own numbers."""
    with open(os.path.join(CSRC, header)) as fh:
        return int(re.search(r"constexpr int %s = (\d+);" % name, fh.read()).group(1))


def _uncapped_kl_blocks(N, C):
    return -(-N // (_constant("term_device.h", "KL_THREADS") // C))


def _set(ctx, rv, U, terms):
    ctx.crf_model_set(U, M.api_terms(rv, terms, U.shape[1]))


def _quarter(terms):
    """Compatibilities scaled by 1/4: keeps a few iterations away from one-hot marginals (as test_backward does)."""
    return [t[:2] + ((t[2] * f32(0.25)).astype(f32),) + t[3:] for t in terms]


def _bits(v):
    return np.asarray(v, np.float64).tobytes()


def _kl(ctx, model, Q, what):
    """crf_model_kl twice (64 equal bits), every part within KL_BOUND x S of the restatement; prints error / S per part."""
    assert Q.size <= M.KL_MAX_ELEMENTS
    parts = ctx.crf_model_kl(Q)
    assert _bits(parts) == _bits(ctx.crf_model_kl(Q)), what
    want, S = model.kl_parts(Q)
    assert parts.shape == want.shape == (2 + len(model.built),)
    err = np.abs(parts - want)
    print("%s: kl parts %s error / S %s (bound %.1g)" % (what, parts, err / np.where(S > 0, S, 1.0), M.KL_BOUND))
    assert np.isfinite(parts).all(), what
    assert (err <= M.KL_BOUND * S).all(), what
    return parts


def _trace(ctx, model, n, what):
    """crf_model_trace(n): Q bit for bit the restated steps, kl[it] bit for bit kl_sum(crf_model_kl(Q_it)), the parts of the
    last Q within the bound of the restatement."""
    Q, mp, kl = ctx.crf_model_trace(n)
    assert _bits(kl) == _bits(ctx.crf_model_trace(n)[2]), what
    assert kl.shape == (n + 1,)
    Qs = model.start()
    for it in range(n + 1):
        assert np.array_equal(ctx.crf_model_step(ctx.crf_model_start(), it), Qs), (what, it)
        assert kl[it] == M.kl_sum(ctx.crf_model_kl(Qs)), (what, it)
        if it < n:
            Qs = model.step(Qs)
    assert np.array_equal(Q, Qs) and np.array_equal(mp, Qs.argmax(1).astype(np.int8)), what
    parts = _kl(ctx, model, Qs, what + ", the traced Q")
    assert kl[n] == M.kl_sum(parts)


@pytest.fixture(scope="module")
def shared_ctx(gpu_ctx_factory):
    """One context for the small cases that only set a model and read it."""
    return gpu_ctx_factory()


# ---------------------------------------------------------------------------------------------
# KL and trace
# ---------------------------------------------------------------------------------------------
# C does not divide 256: PB = 256 / C = 5 (7) points per block step, 512 blocks take 2560 (3584) points per sweep, so blocks
# 0 .. 7 (0 .. 2) take a second trip of the grid-stride loop and the others do not
@pytest.mark.parametrize("N,C", [(2600, 43), (3600, 33)])
def test_kl_past_the_block_cap(gpu_ctx_factory, oracle, N, C):
    import rovinasemanticsegmentation_amd as rv
    cap = _constant("rvseg_crf.h", "KL_MAX_BLOCKS")
    assert cap < _uncapped_kl_blocks(N, C) < 2 * cap and N * C <= M.KL_MAX_ELEMENTS
    rng, U, terms = M.random_model(3000 + N + C, N, C, TWO)
    Q = oracle.exp_and_normalize((rng.random((N, C)) * 4).astype(f32))
    Q[::3, 0] = 0.0
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    _kl(ctx, M.Model(oracle, U, terms), Q, "capped grid (%d, %d)" % (N, C))


def test_trace_past_the_block_cap(gpu_ctx_factory, oracle):
    import rovinasemanticsegmentation_amd as rv
    N, C = 2600, 43
    assert _uncapped_kl_blocks(N, C) > _constant("rvseg_crf.h", "KL_MAX_BLOCKS") and N * C <= M.KL_MAX_ELEMENTS
    _, U, terms = M.random_model(3100, N, C, TWO)
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    _trace(ctx, M.Model(oracle, U, terms), 2, "capped grid trace (%d, %d)" % (N, C))


# kl_final_kernel at its stated size: 2 + 8 parts, and 10 parts x 512 partials.  The eight terms keep the features of EIGHT
# (d = 1 .. 7) at both shapes: the oracle builds its eight lattices of 2600 points in a tenth of a second.
@pytest.mark.parametrize("N,C", [(500, 5), (2600, 43)])
def test_kl_of_ten_parts(gpu_ctx_factory, oracle, N, C):
    import rovinasemanticsegmentation_amd as rv
    assert N * C <= M.KL_MAX_ELEMENTS and len(EIGHT) == 8
    assert {c for _, c, _ in EIGHT} == set(COMPATS) and {n for _, _, n in EIGHT} == set(NORMS)
    if N > 500:
        assert _uncapped_kl_blocks(N, C) > _constant("rvseg_crf.h", "KL_MAX_BLOCKS")
    rng, U, terms = M.random_model(3200 + N, N, C, EIGHT)
    Q = oracle.exp_and_normalize((rng.random((N, C)) * 4).astype(f32))
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    parts = _kl(ctx, M.Model(oracle, U, terms), Q, "ten parts (%d, %d)" % (N, C))
    assert parts.shape == (10,) and parts[2:].all()


# C <= 2: kl_term_kernel<SEQ = true> behind the double-precision blur.  C = 2: PB = 128, two block steps with one live point
# in the second; C = 1: PB = 256, the same.  A Q whose rows do not sum to one keeps the entropy of C = 1 away from 1 log 1.
@pytest.mark.parametrize("N,C", [(129, 2), (257, 1)])
def test_kl_and_trace_of_the_sequential_blur(gpu_ctx_factory, oracle, N, C):
    import rovinasemanticsegmentation_amd as rv
    assert _uncapped_kl_blocks(N, C) == 2 and N % (256 // C) == 1
    rng, U, terms = M.random_model(3300 + C, N, C, [(3, R.MATRIX, R.NORMALIZE_SYMMETRIC), (2, R.POTTS, R.NORMALIZE_AFTER)])
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    model = M.Model(oracle, U, terms)
    Q = (rng.random((N, C)) * 0.9 + 0.05).astype(f32)
    parts = _kl(ctx, model, Q, "sequential blur, C = %d" % C)
    assert parts.all()
    _trace(ctx, model, 2, "sequential blur trace, C = %d" % C)


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("compat", COMPATS)
def test_kl_of_one_term(shared_ctx, oracle, compat, norm):
    """post = false (NO_NORMALIZATION, BEFORE) and a Diagonal's per-class weights in kl_term_kernel."""
    import rovinasemanticsegmentation_amd as rv
    N, C, d = 300, 7, 3
    rng, U, terms = M.random_model(3400 + 4 * compat + norm, N, C, [(d, compat, norm)])
    if compat == R.DIAGONAL:
        assert len(set(terms[0][2].tolist())) == C   # no uniform Diagonal, which would run as Potts
    Q = oracle.exp_and_normalize((rng.random((N, C)) * 4).astype(f32))
    _set(shared_ctx, rv, U, terms)
    parts = _kl(shared_ctx, M.Model(oracle, U, terms), Q, "one term, compat %d, normalisation %d" % (compat, norm))
    assert parts[2] != 0.0


def test_kl_at_the_clamp(shared_ctx, oracle):
    """q = 0, q in (0, 1e-20], the first float above 1e-20f and a one-hot row: the entropy is finite and within the bound."""
    import rovinasemanticsegmentation_amd as rv
    N, C = 300, 7
    rng, U, terms = M.random_model(3500, N, C, TWO)
    Q = M.clamp_q(rng, N, C)
    assert (Q == 0).sum() >= N // 3 and ((Q > 0) & (Q < f32(1e-20))).sum() >= N // 5 and (Q == 1).sum() == 1
    _set(shared_ctx, rv, U, terms)
    parts = _kl(shared_ctx, M.Model(oracle, U, terms), Q, "clamp")
    assert np.isfinite(parts[0]) and parts[0] < 0


def test_energy_of_labels_at_the_edges(shared_ctx, oracle):
    """C = 64 with the labels 63 (the last class), 64 (the first one out of range), -1 and -128 at N = 65."""
    import rovinasemanticsegmentation_amd as rv
    N, C = 65, 64
    rng, U, terms = M.random_model(3600, N, C, TWO)
    labels = rng.integers(0, C, N).astype(np.int8)
    labels[[0, 64]], labels[[1, 33]], labels[[2, 63]], labels[[3, 34]] = 63, 64, -1, -128
    out = (labels < 0) | (labels >= C)
    assert out.sum() == 6
    _set(shared_ctx, rv, U, terms)
    model = M.Model(oracle, U, terms)
    u, p = shared_ctx.crf_model_energy(labels)
    assert np.array_equal(u, model.unary_energy(labels)) and np.array_equal(p, model.pairwise_energy(labels, -1))
    assert not u[out].any() and not p[out].any() and u[~out].all() and p[~out].all()
    assert u[0] == U[0, 63] and u[64] == U[64, 63]
    for k in range(len(terms)):
        pk = shared_ctx.crf_model_energy(labels, k, unary=False)[1]
        assert np.array_equal(pk, model.pairwise_energy(labels, k)) and not pk[out].any()


# ---------------------------------------------------------------------------------------------
# Learning
# ---------------------------------------------------------------------------------------------
def _objective_check(ctx, rv, lr, obj, Q, what):
    value, dq = ctx.crf_model_objective(_objective(rv, obj), Q)
    again, dq2 = ctx.crf_model_objective(_objective(rv, obj), Q)
    assert _bits(value) == _bits(again) and np.array_equal(dq, dq2), what
    want, wdq, S = lr.objective(obj, Q)
    _within(value, want, S, what)
    if obj[0] == LC.IOU:
        assert (np.abs(dq.astype(np.float64) - wdq.astype(np.float64)) <= np.spacing(np.maximum(np.abs(dq), np.abs(wdq)))).all(), what
    else:
        assert np.array_equal(dq, wdq), what
    return value, dq


@pytest.mark.parametrize("C", [3, 64])
@pytest.mark.parametrize("N", [1, 2, 5])
def test_learning_on_a_few_points(gpu_ctx_factory, oracle, N, C):
    """N below one block step of every kernel (fn = (float)N = 1 for N = 1; pair_sums_kernel's only tile is partial): the
    objectives, the backward pass over two iterations and the logistic gradient.  No entry of Q or d_mul_Q is zero, so
    every sum has terms (_within's S > 0)."""
    import rovinasemanticsegmentation_amd as rv
    n, K = 2, 3
    assert N * (n + 1) <= LC.LEARN_MAX_TERMS
    rng, U, terms = M.random_model(4000 + 10 * N + C, N, C, [(3, R.MATRIX, R.NORMALIZE_SYMMETRIC)])
    terms = _quarter(terms)
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    lr = LC.Learn.of_model(M.Model(oracle, U, terms))
    Q = oracle.exp_and_normalize((rng.random((N, C)) * 2).astype(f32))
    assert Q.all()
    gt = rng.integers(0, C, N).astype(np.int16)
    if N == 5:
        gt[3] = -1
    objectives = {"loglikelihood": (LC.LOGLIKELIHOOD, gt, 0.01, None), "hamming": (LC.HAMMING, gt, 0.0, rng.uniform(0.1, 1.0, C).astype(f32)),
                  "iou": (LC.IOU, gt, 0.0, None)}
    for name, obj in objectives.items():
        _objective_check(ctx, rv, lr, obj, Q, "%s, N = %d, C = %d" % (name, N, C))
    Qs = lr.forward(n)
    dq = (rng.uniform(0.05, 0.2, (N, C)) * rng.choice([-1.0, 1.0], (N, C))).astype(f32)
    ug, cg = ctx.crf_model_backward(np.stack(Qs), dq)
    wug, wcg, S = lr.backward(Qs, dq)
    assert np.array_equal(ug, wug)
    assert cg.shape == wcg.shape == (C * (C + 1) // 2,)
    _within(cg, wcg, S, "compat_grad, N = %d, C = %d" % (N, C))
    ug2, cg2 = ctx.crf_model_backward(np.stack(Qs), dq)
    assert np.array_equal(ug, ug2) and _bits(cg) == _bits(cg2)
    f = (rng.uniform(0.1, 1.0, (N, K)) * rng.choice([-1.0, 1.0], (N, K))).astype(f32)
    lg = ctx.crf_logistic_gradient(ug, f)
    wlg, lS = LC.logistic_gradient(ug, f)
    _within(lg, wlg, lS, "logistic_gradient, N = %d, C = %d" % (N, C))
    assert _bits(lg) == _bits(ctx.crf_logistic_gradient(ug, f))
    # the whole gradient on the few points
    obj = objectives["loglikelihood"]
    value, gug, gcg, gQ = ctx.crf_model_gradient(n, _objective(rv, obj), want_Q=True)
    wv, wug, wcg, wQ, vS, S = lr.gradient(n, obj)
    assert np.array_equal(gQ, wQ) and np.array_equal(gug, wug)
    _within(value, wv, vS, "gradient value, N = %d, C = %d" % (N, C))
    _within(gcg, wcg, S, "gradient compat_grad, N = %d, C = %d" % (N, C))


def test_backward_over_eight_terms(gpu_ctx_factory, oracle):
    """The d_cg + model_compat_params(m, k) offsets over eight terms of every compatibility kind."""
    import rovinasemanticsegmentation_amd as rv
    N, C, n = 400, 5, 2
    assert N * (n + 1) <= LC.LEARN_MAX_TERMS
    rng, U, terms = M.random_model(4100, N, C, EIGHT)
    terms = _quarter(terms)
    sizes = [LC.n_compat_params(c, C) for _, c, _ in EIGHT]
    assert sorted(set(sizes)) == [1, C, C * (C + 1) // 2]
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    lr = LC.Learn.of_model(M.Model(oracle, U, terms))
    Qs = lr.forward(n)
    dq = (rng.normal(size=(N, C)) * 0.1).astype(f32)
    ug, cg = ctx.crf_model_backward(np.stack(Qs), dq)
    wug, wcg, S = lr.backward(Qs, dq)
    assert np.array_equal(ug, wug)
    assert cg.shape == wcg.shape == (sum(sizes),)
    _within(cg, wcg, S, "eight terms, backward compat_grad")
    ug2, cg2 = ctx.crf_model_backward(np.stack(Qs), dq)
    assert np.array_equal(ug, ug2) and _bits(cg) == _bits(cg2)
    gt = rng.integers(0, C, N).astype(np.int16)
    gt[::7], gt[3::11] = -1, C + 2
    obj = (LC.LOGLIKELIHOOD, gt, 0.01, None)
    value, ug, cg, Q = ctx.crf_model_gradient(n, _objective(rv, obj), want_Q=True)
    wv, wug, wcg, wQ, vS, S = lr.gradient(n, obj)
    assert np.array_equal(Q, wQ) and np.array_equal(ug, wug) and cg.shape == (sum(sizes),)
    _within(value, wv, vS, "eight terms, gradient value")
    _within(cg, wcg, S, "eight terms, gradient compat_grad")
    again = ctx.crf_model_gradient(n, _objective(rv, obj), want_Q=True)
    assert _bits(again[0]) == _bits(value) and np.array_equal(again[1], ug) and _bits(again[2]) == _bits(cg) and np.array_equal(again[3], Q)


# K at the 64-column blocks of launch_logistic_gradient: one full block; a full block and one column (ldb = 65 != Cb); two
# full blocks; two full blocks and one column.  With C = 64 the pair state is the full 64 x 64.  A tile holds
# 1024 / max(C, columns of the block) points: 16 for a full block, 341 for the one-column remainder at C = 3, where the last
# of the four tiles of N = 1100 holds 77 points.
LOGISTIC_SHAPES = [(300, 64, 64), (300, 64, 65), (300, 5, 128), (1100, 3, 129)]


@pytest.mark.parametrize("N,C,K", LOGISTIC_SHAPES)
def test_logistic_gradient_at_the_column_blocks(shared_ctx, N, C, K):
    assert N <= LC.LEARN_MAX_TERMS
    rng = np.random.default_rng(4200 + K + C)
    ug = rng.normal(size=(N, C)).astype(f32)
    f = rng.uniform(-1.0, 1.0, (N, K)).astype(f32)
    lg = shared_ctx.crf_logistic_gradient(ug, f)
    wlg, S = LC.logistic_gradient(ug, f)
    assert lg.shape == (C * K,)
    _within(lg, wlg, S, "logistic_gradient (%d, %d, %d)" % (N, C, K))
    assert _bits(lg) == _bits(shared_ctx.crf_logistic_gradient(ug, f))


def test_logistic_gradient_device_twin(gpu_ctx_factory):
    torch = pytest.importorskip("torch")
    N, C, K = LOGISTIC_SHAPES[1]
    rng = np.random.default_rng(4300)
    ug = rng.normal(size=(N, C)).astype(f32)
    f = rng.uniform(-1.0, 1.0, (N, K)).astype(f32)
    host, ctx = gpu_ctx_factory(), gpu_ctx_factory()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    d_ug, d_f = torch.from_numpy(ug).to(dev), torch.from_numpy(f).to(dev)
    d_out = torch.zeros(C * K, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    ctx.crf_logistic_gradient_device(N, C, K, d_ug.data_ptr(), d_f.data_ptr(), d_out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert _bits(d_out.cpu().numpy()) == _bits(host.crf_logistic_gradient(ug, f))


def test_ground_truth_without_a_valid_label(gpu_ctx_factory, oracle):
    """Every point skipped: the value is exactly 0.0 (IoU: 0 / 1e-20 per class), d_mul_Q and both gradients are zeros.
    Exact comparisons: a sum without terms has S = 0."""
    import rovinasemanticsegmentation_amd as rv
    N, C, n = 300, 4, 2
    rng, U, terms = M.random_model(4400, N, C, TWO)
    terms = _quarter(terms)
    gt = LC.invalid_gt(N, C)
    assert not ((gt >= 0) & (gt < C)).any() and (gt < 0).any() and (gt >= C).any()
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    lr = LC.Learn.of_model(M.Model(oracle, U, terms))
    Q = lr.forward(1)[1]
    for name, obj in (("loglikelihood", (LC.LOGLIKELIHOOD, gt, 0.01, None)), ("hamming", (LC.HAMMING, gt, 0.0, rng.uniform(0.1, 1.0, C).astype(f32))),
                      ("iou", (LC.IOU, gt, 0.0, None))):
        for _ in range(2):
            value, dq = ctx.crf_model_objective(_objective(rv, obj), Q)
            assert value == 0.0 and not dq.any(), name
        want, wdq, S = lr.objective(obj, Q)
        assert want == 0.0 and not wdq.any() and S == 0.0, name
        value, ug, cg, Qn = ctx.crf_model_gradient(n, _objective(rv, obj), want_Q=True)
        assert value == 0.0 and not ug.any() and not cg.any(), name
        assert cg.shape == (1 + C * (C + 1) // 2,) and np.array_equal(Qn, lr.forward(n)[n]), name


def test_iou_of_a_class_that_never_occurs(gpu_ctx_factory, oracle):
    """One class without a labelled point: its in is 0 and its un 1e-20 + the sum of its q over the labelled points, so it
    adds 0 to the value and nothing but zeros to its column of d_mul_Q."""
    import rovinasemanticsegmentation_amd as rv
    N, C, absent = 300, 4, 2
    rng, U, terms = M.random_model(4500, N, C, TWO)
    gt = LC.gt_without_class(rng, N, C, absent)
    assert set(gt[(gt >= 0) & (gt < C)].tolist()) == set(range(C)) - {absent} and (gt < 0).any() and (gt >= C).any()
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    lr = LC.Learn.of_model(M.Model(oracle, U, terms))
    Q = oracle.exp_and_normalize((rng.random((N, C)) * 4).astype(f32))
    value, dq = _objective_check(ctx, rv, lr, (LC.IOU, gt, 0.0, None), Q, "iou without class %d" % absent)
    assert not dq[:, absent].any()
    ok = (gt >= 0) & (gt < C)
    assert dq[ok][:, [c for c in range(C) if c != absent]].all() and not dq[~ok].any()
    assert 0.0 < value < (C - 1) / C


def test_loglikelihood_below_the_clamp(gpu_ctx_factory, oracle):
    """robust = -0.3: where q + robust < 1e-20f the term is log(1e-20f) / N and d_mul_Q is q / 1e-20f / N, of the order 1e17."""
    import rovinasemanticsegmentation_amd as rv
    N, C, robust = 500, 4, -0.3
    rng, U, terms = M.random_model(4600, N, C, TWO)
    gt = rng.integers(0, C, N).astype(np.int16)
    gt[::7], gt[3::11] = -1, C + 2
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    lr = LC.Learn.of_model(M.Model(oracle, U, terms))
    Q = oracle.exp_and_normalize((rng.random((N, C)) * 4).astype(f32))
    Q[5] = (f32(0.3), f32(0.7), 0, 0)   # q + robust = 0 and q + robust > 0, whichever the label
    gt[5] = 0
    obj = (LC.LOGLIKELIHOOD, gt, robust, None)
    _, wdq, _ = lr.objective(obj, Q)
    assert np.isfinite(wdq).all()
    ok = (gt >= 0) & (gt < C)
    qgt = Q[ok, gt[ok]]
    below = (qgt + f32(robust)).astype(f32) < f32(1e-20)
    assert below.sum() > 50 and (~below).sum() > 50
    value, dq = _objective_check(ctx, rv, lr, obj, Q, "loglikelihood, robust = %g" % robust)
    assert np.isfinite(dq).all() and dq.max() > 1e16
    # the gradient carries the large entries through the backward pass: fp32 bit for bit, doubles within the bound
    terms_q = _quarter(terms)
    _set(ctx, rv, U, terms_q)
    lrq = LC.Learn.of_model(M.Model(oracle, U, terms_q))
    value, ug, cg, Qn = ctx.crf_model_gradient(1, _objective(rv, obj), want_Q=True)
    wv, wug, wcg, wQ, vS, S = lrq.gradient(1, obj)
    assert np.isfinite(wug).all() and np.isfinite(wcg).all()
    assert np.array_equal(Qn, wQ) and np.array_equal(ug, wug)
    _within(value, wv, vS, "gradient value, robust = %g" % robust)
    _within(cg, wcg, S, "gradient compat_grad, robust = %g" % robust)


# ---------------------------------------------------------------------------------------------
# Regrown buffers
# ---------------------------------------------------------------------------------------------
def test_learning_buffers_regrow_under_one_model(gpu_ctx_factory, oracle):
    """CrfModel::qs holds Q[0 .. n]: it grows from gradient(1) to gradient(6), is reused by gradient(2), grows again for a
    caller's Q[0 .. 7] and is reused by gradient(6).  Every result is that of the same call as the only one on a fresh context."""
    import rovinasemanticsegmentation_amd as rv
    N, C = 300, 5
    rng, U, terms = M.random_model(4700, N, C, TWO)
    terms = _quarter(terms)
    gt = rng.integers(0, C, N).astype(np.int16)
    gt[::7], gt[3::11] = -1, C + 2
    obj = rv.LogLikelihood(gt, 0.01)
    lr = LC.Learn.of_model(M.Model(oracle, U, terms))
    Q_all = np.stack(lr.forward(7))
    dq = (rng.normal(size=(N, C)) * 0.1).astype(f32)
    calls = [("gradient(1)", lambda c: c.crf_model_gradient(1, obj, want_Q=True)),
             ("gradient(6)", lambda c: c.crf_model_gradient(6, obj, want_Q=True)),
             ("gradient(2)", lambda c: c.crf_model_gradient(2, obj, want_Q=True)),
             ("backward over Q[0 .. 7]", lambda c: c.crf_model_backward(Q_all, dq)),
             ("gradient(6) again", lambda c: c.crf_model_gradient(6, obj, want_Q=True))]
    ctx = gpu_ctx_factory()
    _set(ctx, rv, U, terms)
    got = [(name, call(ctx)) for name, call in calls]
    assert _same_bits(got[1][1], got[4][1])
    for (name, call), (_, result) in zip(calls, got):
        fresh = gpu_ctx_factory()
        _set(fresh, rv, U, terms)
        assert _same_bits(call(fresh), result), name
        fresh.close()
    # and the restatement, once: the backward pass over the caller's eight matrices
    wug, wcg, S = lr.backward(list(Q_all), dq)
    assert np.array_equal(got[3][1][0], wug)
    _within(got[3][1][1], wcg, S, "backward over Q[0 .. 7]")


RESET_MODELS = [(300, 4, [(2, R.POTTS, R.NORMALIZE_SYMMETRIC)]), (900, 21, TWO), (200, 64, [(5, R.MATRIX, R.NORMALIZE_AFTER)]),
                (300, 4, [(2, R.POTTS, R.NORMALIZE_SYMMETRIC)])]


def test_buffers_regrow_from_model_to_model(gpu_ctx_factory, oracle):
    """Models of growing N, C and parameter count set one after another on one context (then the first again): the learning
    partials, IoU's sums, the staged weights and gradients are regrown or reused.  After each set the IoU objective, a
    Hamming gradient, KL, the energies and the logistic gradient equal a fresh context bit for bit, and the restatement."""
    import rovinasemanticsegmentation_amd as rv
    ctx = gpu_ctx_factory()
    n, K = 2, 3
    for i, (N, C, specs) in enumerate(RESET_MODELS):
        what = "model %d (%d, %d)" % (i, N, C)
        assert N * C <= M.KL_MAX_ELEMENTS and N * (n + 1) <= LC.LEARN_MAX_TERMS
        rng, U, terms = M.random_model(4800 + N + C, N, C, specs)
        terms = _quarter(terms)
        gt = rng.integers(0, C, N).astype(np.int16)
        gt[::7], gt[3::11] = -1, C + 2
        iou = (LC.IOU, gt, 0.0, None)
        ham = (LC.HAMMING, gt, 0.0, rng.uniform(0.1, 1.0, C).astype(f32))
        Q = oracle.exp_and_normalize((rng.random((N, C)) * 4).astype(f32))
        labels = rng.integers(-1, C + 1, N).astype(np.int8)
        f = rng.uniform(-1.0, 1.0, (N, K)).astype(f32)
        x = rng.normal(size=(N, C)).astype(f32)
        calls = [("objective", lambda c: c.crf_model_objective(_objective(rv, iou), Q)),
                 ("gradient", lambda c: c.crf_model_gradient(n, _objective(rv, ham), want_Q=True)),
                 ("kl", lambda c: c.crf_model_kl(Q)),
                 ("energy", lambda c: c.crf_model_energy(labels)),
                 ("logistic_gradient", lambda c: c.crf_logistic_gradient(x, f))]
        _set(ctx, rv, U, terms)
        got = {name: call(ctx) for name, call in calls}
        fresh = gpu_ctx_factory()
        _set(fresh, rv, U, terms)
        for name, call in calls:
            assert _same_bits(call(fresh), got[name]), (what, name)
        fresh.close()
        model = M.Model(oracle, U, terms)
        lr = LC.Learn.of_model(model)
        _objective_check(ctx, rv, lr, iou, Q, what + " iou")
        value, ug, cg, Qn = got["gradient"]
        wv, wug, wcg, wQ, vS, S = lr.gradient(n, ham)
        assert np.array_equal(Qn, wQ) and np.array_equal(ug, wug), what
        _within(value, wv, vS, what + " gradient value")
        _within(cg, wcg, S, what + " compat_grad")
        parts = _kl(ctx, model, Q, what)
        assert _bits(parts) == _bits(got["kl"])
        assert np.array_equal(got["energy"][0], model.unary_energy(labels)) and np.array_equal(got["energy"][1], model.pairwise_energy(labels, -1))
        wlg, lS = LC.logistic_gradient(x, f)
        _within(got["logistic_gradient"], wlg, lS, what + " logistic_gradient")
