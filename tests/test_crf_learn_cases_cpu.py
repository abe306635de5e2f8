"""The learning restatement (crf_learn_cases.py) against central finite differences, in float64 on an explicit dense
filter matrix: this guards the mathematics of the yardstick the GPU tests compare with.  Also the host-only
rvseg_crf_objective_check and CRFEnergy's signs and L2 term.  No GPU."""
import math

import numpy as np
import pytest

import crf_learn_cases as LC
import crf_restate as R

NORMS = [R.NO_NORMALIZATION, R.NORMALIZE_BEFORE, R.NORMALIZE_AFTER, R.NORMALIZE_SYMMETRIC]
COMPATS = [R.POTTS, R.DIAGONAL, R.MATRIX]
N, C, K, NIT, H = 12, 3, 4, 3, 1e-5
# relative to the gradient's norm.  Central differences in float64: O(h^2) truncation ~1e-10 and ~1e-16 / h = 1e-11 rounding
# of values of order 1, against gradient norms of 1e-2 .. 1 -- observed maximum over all cases: 4.4e-10
TOL = 1e-5


def _params(rng, compat):
    if compat == R.POTTS:
        return rng.uniform(0.5, 2.0, 1)
    if compat == R.DIAGONAL:
        return -rng.uniform(0.2, 2.0, C)
    m = rng.uniform(-1.0, 1.0, (C, C))
    return (0.5 * (m + m.T)).reshape(-1)


def _unpack(compat, v):
    """labelCompatibilityParameters() layout -> the compat_params a term is built from."""
    if compat != R.MATRIX:
        return np.asarray(v, np.float64)
    W = np.zeros((C, C))
    k = 0
    for i in range(C):
        for j in range(i, C):
            W[i, j] = W[j, i] = v[k]
            k += 1
    return W.reshape(-1)


def _pack(compat, cp):
    if compat != R.MATRIX:
        return np.asarray(cp, np.float64).copy()
    W = np.asarray(cp).reshape(C, C)
    return np.array([W[i, j] for i in range(C) for j in range(i, C)])


class Case:
    def __init__(self, seed, specs, n=N, gt=None):
        """n points (below six: every one labelled); gt: a ground truth in place of the random one."""
        rng = np.random.default_rng(seed)
        self.L = rng.uniform(-1.0, 1.0, (C, K))
        self.f = rng.uniform(0.0, 1.0, (n, K))
        self.specs = specs
        self.filters = [LC.DenseFilter(rng.uniform(0.0, 1.0, (n, n)) * rng.uniform(0.5, 1.5) / n) for _ in specs]
        self.params = [_pack(c, _params(rng, c)) for c, _ in specs]
        if gt is None:
            gt = rng.integers(0, C, n)
            if n > 5:
                gt[1], gt[5] = -1, C   # skipped points
        assert len(gt) == n
        self.gt = gt
        self.objectives = {
            "loglikelihood": (LC.LOGLIKELIHOOD, gt, 0.0, None),
            "loglikelihood robust": (LC.LOGLIKELIHOOD, gt, 0.01, None),
            "hamming": (LC.HAMMING, gt, 0.0, rng.uniform(0.1, 1.0, C)),
            "iou": (LC.IOU, gt, 0.0, None),
        }

    def learn(self, U=None, params=None, L=None):
        L = self.L if L is None else L
        U = self.f @ L.T if U is None else U   # LogisticUnaryEnergy::get
        params = self.params if params is None else params
        built = [(flt, LC.norm_of(flt, nt, np.float64), c, _unpack(c, p), nt) for flt, (c, nt), p in zip(self.filters, self.specs, params)]
        return LC.Learn(U, built, np.float64)

    def value(self, obj, **kw):
        lr = self.learn(**kw)
        return lr.objective(obj, lr.forward(NIT)[NIT])[0]


def _fd(fun, x):
    x = np.asarray(x, np.float64)
    g = np.zeros(x.size)
    for i in range(x.size):
        e = np.zeros(x.size)
        e[i] = H
        g[i] = (fun((x.ravel() + e).reshape(x.shape)) - fun((x.ravel() - e).reshape(x.shape))) / (2 * H)
    return g


def _close(got, fd, what):
    err = np.abs(np.ravel(got) - fd).max()
    scale = np.linalg.norm(fd)
    print("%s: max error %.3g, gradient norm %.3g, relative %.3g" % (what, err, scale, err / scale))
    assert scale > 0
    assert err <= TOL * scale, what


# two terms per case; the six cases hold every normalisation and every compatibility
SPECS = [[(COMPATS[(i + j) % 3], NORMS[(i + 2 * j) % 4]) for j in range(2)] for i in range(6)]


def test_specs_cover_every_normalisation_and_compatibility():
    assert {c for spec in SPECS for c, _ in spec} == set(COMPATS) and {n for spec in SPECS for _, n in spec} == set(NORMS)


def _gradients_match_central_differences(case, obj):
    lr = case.learn()
    value, ug, cg, Qn, _, _ = lr.gradient(NIT, obj)
    assert value == case.value(obj)
    # unary energy
    _close(ug, _fd(lambda U: case.value(obj, U=U), lr.U), "unary")
    # compatibility parameters, in the layout of labelCompatibilityParameters()
    sizes = [p.size for p in case.params]
    flat = np.concatenate(case.params)

    def with_params(v):
        return case.value(obj, params=np.split(v, np.cumsum(sizes)[:-1]))
    _close(cg, _fd(with_params, flat), "compatibility")
    # logistic L, column-major like unaryParameters()
    lg, _ = LC.logistic_gradient(ug, case.f)
    _close(lg, _fd(lambda v: case.value(obj, L=v.reshape(K, C).T), case.L.T.reshape(-1)), "logistic")


@pytest.mark.parametrize("name", ["loglikelihood", "loglikelihood robust", "hamming", "iou"])
@pytest.mark.parametrize("i", range(len(SPECS)))
def test_gradients_match_central_differences(i, name):
    case = Case(40 + i, SPECS[i])
    _gradients_match_central_differences(case, case.objectives[name])


@pytest.mark.parametrize("name", ["loglikelihood robust", "hamming", "iou"])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("i", [1, 2])   # (Diagonal, Matrix) and (Matrix, Potts), three normalisations
def test_gradients_of_one_and_two_points(i, n, name):
    """N = 1: the filter is one number, IoU's union is 1e-20 + 1 + the other classes' q of the one point."""
    case = Case(140 + 10 * i + n, SPECS[i], n=n)
    assert ((case.gt >= 0) & (case.gt < C)).all()
    _gradients_match_central_differences(case, case.objectives[name])


@pytest.mark.parametrize("i", range(0, len(SPECS), 2))
def test_gradients_of_a_negative_robust(i):
    """LogLikelihood with robust < 0 where every labelled q + robust stays above the 1e-20 clamp (by a margin the finite
    differences' steps cannot cross): there the objective is differentiable and d_mul_Q = q / (q + robust) / N its derivative."""
    case = Case(240 + i, SPECS[i])
    lr = case.learn()
    Qn = lr.forward(NIT)[NIT]
    ok = (case.gt >= 0) & (case.gt < C)
    qmin = Qn[ok, case.gt[ok]].min()
    robust = -0.5 * qmin
    assert robust < -1e-3 and qmin + robust > 1e3 * H
    obj = (LC.LOGLIKELIHOOD, case.gt, robust, None)
    value, dq, _ = lr.objective(obj, Qn)
    assert value < lr.objective((LC.LOGLIKELIHOOD, case.gt, 0.0, None), Qn)[0] and (dq[ok, case.gt[ok]] > 1.0 / N).all()
    _gradients_match_central_differences(case, obj)


def test_negative_robust_below_the_clamp_by_hand():
    """Below the clamp the term is log(1e-20) / N and d_mul_Q is q / 1e-20 / N (objective.cpp:44-46), whatever q + robust is."""
    Q = np.array([[0.25, 0.75], [0.5, 0.5], [0.9, 0.1]])
    lr = LC.Learn(np.zeros((3, 2)), [], np.float64)
    value, dq, S = lr.objective((LC.LOGLIKELIHOOD, np.array([0, 0, 0]), -0.5, None), Q)
    want = (2 * math.log(1e-20) + math.log(0.9 - 0.5)) / 3
    assert value == pytest.approx(want, rel=1e-15) and S == pytest.approx(-want, rel=1e-15)
    assert dq[:, 0] == pytest.approx([0.25 / 1e-20 / 3, 0.5 / 1e-20 / 3, 0.9 / (0.9 - 0.5) / 3], rel=1e-15) and not dq[:, 1].any()
    # in float32 the same entries are finite, of the order 1e19
    lr32 = LC.Learn(np.zeros((3, 2), np.float32), [], np.float32)
    _, dq32, _ = lr32.objective((LC.LOGLIKELIHOOD, np.array([0, 0, 0]), -0.5, None), Q.astype(np.float32))
    assert dq32.dtype == np.float32 and np.isfinite(dq32).all() and dq32[1, 0] == np.float32(np.float32(np.float32(0.5) / np.float32(1e-20)) / np.float32(3))


@pytest.mark.parametrize("absent", range(C))
def test_iou_gradients_without_one_class(absent):
    rng = np.random.default_rng(340 + absent)
    gt = LC.gt_without_class(rng, N, C, absent)
    assert set(gt[(gt >= 0) & (gt < C)].tolist()) == set(range(C)) - {absent} and (gt < 0).any() and (gt >= C).any()
    case = Case(340 + absent, SPECS[absent], gt=gt)
    _gradients_match_central_differences(case, (LC.IOU, gt, 0.0, None))


def test_iou_without_one_class_by_hand():
    """Class 1 never occurs: in = 0 and un = 1e-20 + its q over the labelled points, so its ratio and its column of
    d_mul_Q are zero; class 0: in = q00 + q10, un = 1e-20 + 2; the skipped point counts nowhere."""
    Q = np.array([[0.25, 0.75], [0.5, 0.5], [0.9, 0.1]])
    lr = LC.Learn(np.zeros((3, 2)), [], np.float64)
    value, dq, S = lr.objective((LC.IOU, np.array([0, 0, -1]), 0.0, None), Q)
    inn, un = 0.75, 1e-20 + 2.0
    assert value == pytest.approx((inn / un + 0.0 / (1e-20 + 1.25)) / 2, rel=1e-15) and S == pytest.approx(value, rel=1e-15)
    assert dq[:2, 0] == pytest.approx([0.25 / (un * 2), 0.5 / (un * 2)], rel=1e-15)
    assert not dq[:, 1].any() and not dq[2].any()


@pytest.mark.parametrize("i", range(0, len(SPECS), 2))
def test_a_ground_truth_without_a_valid_label_gives_zeros(i):
    """Closed form: no point counts, so every value is 0 (IoU: C times 0 / 1e-20) and so is every gradient."""
    gt = LC.invalid_gt(N, C)
    assert not ((gt >= 0) & (gt < C)).any() and (gt < 0).any() and (gt >= C).any()
    case = Case(440 + i, SPECS[i], gt=gt)
    lr = case.learn()
    for obj in ((LC.LOGLIKELIHOOD, gt, 0.01, None), (LC.LOGLIKELIHOOD, gt, -0.3, None), (LC.HAMMING, gt, 0.0, np.ones(C)), (LC.IOU, gt, 0.0, None)):
        value, dq, S = lr.objective(obj, lr.forward(NIT)[NIT])
        assert value == 0.0 and S == 0.0 and not dq.any()
        value, ug, cg, _, vS, cS = lr.gradient(NIT, obj)
        assert value == 0.0 and vS == 0.0 and not ug.any() and not cg.any() and not cS.any()
        assert cg.shape == (sum(p.size for p in case.params),)
        assert not LC.logistic_gradient(ug, case.f)[0].any()


def test_apply_transpose_is_the_adjoint_of_the_kernel_apply():
    """<a, filter(b)> == <filter^T(a), b> for every normalisation (pairwise.cpp:63-80), and BEFORE / AFTER swap roles."""
    rng = np.random.default_rng(7)
    K = LC.DenseFilter(rng.uniform(0, 1, (N, N)))
    a, b = rng.normal(size=(N, C)), rng.normal(size=(N, C))
    for nt in NORMS:
        lr = LC.Learn(np.zeros((N, C)), [(K, LC.norm_of(K, nt, np.float64), R.POTTS, [1.0], nt)], np.float64)
        lhs, rhs = (a * lr.filter(0, b)).sum(), (lr.filter(0, a, True) * b).sum()
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs), nt
    assert LC.pre_post(R.NORMALIZE_BEFORE, True) == LC.pre_post(R.NORMALIZE_AFTER, False) == (False, True)
    assert LC.pre_post(R.NORMALIZE_AFTER, True) == LC.pre_post(R.NORMALIZE_BEFORE, False) == (True, False)


def test_objective_check_failure_paths():
    from rovinasemanticsegmentation_amd import _capi as capi
    gt = np.zeros(4, np.int16)
    w = np.ones(3, np.float32)
    g, wp = gt.ctypes.data, w.ctypes.data
    ok = [capi.RvsegCrfObjective(capi.OBJECTIVE_LOGLIKELIHOOD, g, 0.01, None), capi.RvsegCrfObjective(capi.OBJECTIVE_HAMMING, g, 0.0, wp),
          capi.RvsegCrfObjective(capi.OBJECTIVE_IOU, g, 0.0, None)]
    for o in ok:
        assert capi.crf_objective_check(o) == capi.OK
    bad = [None, capi.RvsegCrfObjective(-1, g, 0.0, wp), capi.RvsegCrfObjective(3, g, 0.0, wp),
           capi.RvsegCrfObjective(capi.OBJECTIVE_IOU, None, 0.0, None), capi.RvsegCrfObjective(capi.OBJECTIVE_HAMMING, g, 0.0, None),
           capi.RvsegCrfObjective(capi.OBJECTIVE_LOGLIKELIHOOD, g, float("nan"), None),
           capi.RvsegCrfObjective(capi.OBJECTIVE_LOGLIKELIHOOD, g, float("inf"), None)]
    for o in bad:
        assert capi.crf_objective_check(o) == capi.ERR_INVALID_ARG


def test_hamming_weights_follow_the_reference_constructor():
    import rovinasemanticsegmentation_amd as rv
    gt = np.array([0, 1, 1, 2, 2, 2, -1, 1], np.int16)
    for p in (0.0, 0.2, 1.0):
        h = rv.Hamming(gt, p)
        assert np.array_equal(h.class_weight, LC.hamming_weights(gt, p))
        # (cnt * w).sum() == 1: the weights of the labelled points add up to one
        assert abs(float((np.bincount(gt[gt >= 0]) * h.class_weight).sum()) - 1.0) < 1e-6
    assert np.array_equal(rv.Hamming(gt, [0.5, 0.25]).weights(3), np.array([0.5, 0.25, 0.0], np.float32))
    assert rv.Hamming(gt, 0.0).record(8, 3)[0].kind == rv.capi.OBJECTIVE_HAMMING


class _FakeCRF:
    """The part of DenseCRF that CRFEnergy drives, over the float64 restatement."""

    def __init__(self, case):
        self.case, self.Lm, self.params = case, case.L.copy(), [p.copy() for p in case.params]
        self.calls = []

    def unaryParameters(self):
        return self.Lm.T.reshape(-1).astype(np.float32)

    def labelCompatibilityParameters(self):
        return np.concatenate(self.params).astype(np.float32)

    def setUnaryParameters(self, v):
        self.calls.append("unary")
        self.Lm = np.asarray(v, np.float64).reshape(K, C).T

    def setLabelCompatibilityParameters(self, v):
        self.calls.append("lbl")
        self.params = np.split(np.asarray(v, np.float64), np.cumsum([p.size for p in self.params])[:-1])

    def gradient(self, n, objective, unary=True, lbl_cmp=True):
        lr = self.case.learn(L=self.Lm, params=self.params)
        value, ug, cg, _, _, _ = lr.gradient(n, objective)
        return value, (LC.logistic_gradient(ug, self.case.f)[0].astype(np.float32) if unary else None), (cg.astype(np.float32) if lbl_cmp else None)


@pytest.mark.parametrize("unary,pairwise", [(True, True), (False, True), (True, False)])
def test_crf_energy_negates_and_regularises(unary, pairwise):
    """dense_learning.cpp:60-84: dx = -(du, dl) + l2 x, r = -r + 0.5 l2 x.x; only the chosen parameter groups move."""
    import rovinasemanticsegmentation_amd as rv
    case = Case(90, SPECS[2])
    obj = case.objectives["iou"]
    crf = _FakeCRF(case)
    energy = rv.CRFEnergy(crf, obj, NIT, unary, pairwise)
    x0 = energy.initialValue()
    want0 = np.concatenate(([crf.unaryParameters()] if unary else []) + ([crf.labelCompatibilityParameters()] if pairwise else []))
    assert np.array_equal(x0, want0) and x0.dtype == np.float32
    x = (x0 * np.float32(1.25) + np.float32(0.01)).astype(np.float32)
    value, dx = energy.gradient(x)
    assert crf.calls == (["unary"] if unary else []) + (["lbl"] if pairwise else [])
    r, du, dl = crf.gradient(NIT, obj, unary, pairwise)   # the parameters are x now
    g = np.concatenate(([du] if unary else []) + ([dl] if pairwise else []))
    assert value == -r and np.array_equal(dx, -g)
    energy.setL2Norm(1e-3)
    value2, dx2 = energy.gradient(x)
    l2 = np.float32(1e-3)
    assert np.array_equal(dx2, (-g + l2 * x).astype(np.float32))
    assert value2 == -r + 0.5 * float(l2) * float(np.dot(x, x))
    assert value2 > value
    with pytest.raises(NotImplementedError) as e:
        rv.CRFEnergy(crf, obj, NIT, True, True, kernel=True)
    assert "kernel" in str(e.value)
