"""rvseg_minimize_lbfgs (include/rvseg.h, "The minimiser") through ctypes, without a context or a GPU: three problems whose
minimisers are known, the iteration limit, an energy that stops being finite, and the restart loop of minimizeLBFGS
(optimization.cpp:87-94)."""
import ctypes as C
import math
import os

import numpy as np
import pytest


def _capi():
    from rovinasemanticsegmentation_amd import _capi as capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    capi.lib()
    return capi


# diagonal convex quadratic, n = 10, condition number 1e3
_D = np.logspace(0, 3, 10)
_B = np.linspace(-1.0, 2.0, 10)


def quadratic(x):
    r = x - _B
    return 0.5 * float(np.dot(_D * r, r)), _D * r


def rosenbrock(x):
    a, b = x
    return (1 - a) ** 2 + 100 * (b - a * a) ** 2, np.array([-2 * (1 - a) - 400 * a * (b - a * a), 200 * (b - a * a)])


def scalar(x):   # n = 1: cosh(x - 3), minimum 1 at 3
    return math.cosh(x[0] - 3.0), np.array([math.sinh(x[0] - 3.0)])


PROBLEMS = {"quadratic": (quadratic, np.full(10, 5.0), _B, {}),
            "rosenbrock": (rosenbrock, np.array([-1.2, 1.0]), np.ones(2), {"max_iterations": 500}),
            "scalar": (scalar, np.array([-1.0]), np.array([3.0]), {})}


def test_defaults_are_the_documented_ones():
    capi = _capi()
    p = capi.RvsegLbfgsParams()
    capi.lib().rvseg_lbfgs_params_default(C.byref(p))
    assert (p.m, p.epsilon, p.max_iterations, p.max_linesearch, p.ftol, p.min_step, p.max_step) == (6, 1e-5, 0, 20, 1e-4, 1e-20, 1e20)
    for name in ("rvseg_minimize_lbfgs", "rvseg_lbfgs_params_default", "rvseg_crf_model_set_kernel", "rvseg_crf_model_set_logistic",
                 "rvseg_crf_model_set_logistic_device", "rvseg_crf_model_set_logistic_params", "rvseg_crf_model_gradient_params",
                 "rvseg_crf_model_gradient_params_device", "rvseg_crf_model_energy_gradient", "rvseg_crf_model_info"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_converges(name):
    capi = _capi()
    fun, x0, xmin, params = PROBLEMS[name]
    seen = []
    x, fx, rep = capi.minimize_lbfgs(fun, x0, lambda x, g, fx, xn, gn, step, k, ls: seen.append((k, fx, ls, step)), **params)
    print(name, rep, fx, x)
    assert rep["rvseg_status"] == capi.OK and rep["status"] == capi.LBFGS_CONVERGED
    f, g = fun(x)
    assert f == fx
    assert np.linalg.norm(g) / max(1.0, np.linalg.norm(x)) < 1e-5   # epsilon's default, recomputed here
    assert rep["gnorm"] == math.sqrt(float(np.dot(g, g))) or abs(rep["gnorm"] - np.linalg.norm(g)) <= 1e-12 * np.linalg.norm(g)
    values = [fun(x0)[0]] + [s[1] for s in seen]
    assert all(b <= a for a, b in zip(values, values[1:])), values   # Armijo: never up between iterations
    assert [s[0] for s in seen] == list(range(1, rep["iterations"] + 1))
    assert rep["evaluations"] == 1 + sum(s[2] for s in seen)
    assert all(1 <= s[2] <= 20 for s in seen)
    assert np.abs(x - xmin).max() < 1e-3


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_iteration_limit(name):
    capi = _capi()
    fun, x0, _, _ = PROBLEMS[name]
    x, fx, rep = capi.minimize_lbfgs(fun, x0, max_iterations=3)
    assert rep["rvseg_status"] == capi.OK and rep["status"] == capi.LBFGS_MAX_ITERATIONS and rep["iterations"] == 3
    assert fx <= fun(x0)[0] and fx == fun(x)[0]


def test_start_at_the_minimum_takes_no_step():
    capi = _capi()
    x, fx, rep = capi.minimize_lbfgs(quadratic, _B)
    assert rep["status"] == capi.LBFGS_CONVERGED and rep["iterations"] == 0 and rep["evaluations"] == 1
    assert np.array_equal(x, _B) and fx == 0.0


def test_energy_that_stops_being_finite():
    """NaN from the third evaluation on: an error status, x the best finite point, its value in fx."""
    capi = _capi()
    calls = []

    def fun(x):
        f, g = quadratic(x)
        calls.append((x.copy(), f))
        return (float("nan"), g) if len(calls) >= 3 else (f, g)
    x0 = np.full(10, 5.0)
    x, fx, rep = capi.minimize_lbfgs(fun, x0)
    assert rep["rvseg_status"] == capi.ERR_INVALID_ARG and rep["status"] == capi.LBFGS_NOT_FINITE
    finite = calls[:2]
    best = min(finite, key=lambda c: c[1])
    assert fx == best[1] and np.array_equal(x, best[0]) and fx <= finite[0][1]
    # not finite at the start: x stays
    x, fx, rep = capi.minimize_lbfgs(lambda x: (float("inf"), np.zeros(10)), x0)
    assert rep["rvseg_status"] == capi.ERR_INVALID_ARG and rep["status"] == capi.LBFGS_NOT_FINITE and np.array_equal(x, x0)
    # a gradient that is not finite counts too
    x, fx, rep = capi.minimize_lbfgs(lambda x: (1.0, np.full(10, float("nan"))), x0)
    assert rep["status"] == capi.LBFGS_NOT_FINITE and np.array_equal(x, x0)


def test_failed_line_search_keeps_the_start():
    """A gradient with the wrong sign: no step can satisfy the Armijo condition, and the start comes back."""
    capi = _capi()
    x0 = np.array([2.0])
    x, fx, rep = capi.minimize_lbfgs(lambda x: (float(x[0] ** 2), np.array([-2 * x[0]])), x0)
    assert rep["rvseg_status"] == capi.OK and rep["status"] == capi.LBFGS_LINESEARCH_FAILED
    assert rep["iterations"] == 0 and rep["evaluations"] == 21 and fx <= 4.0 and fx == float(x[0] ** 2)


def test_bad_arguments_and_callbacks():
    capi = _capi()
    L = capi.lib()
    x = np.zeros(2)
    rep = capi.RvsegLbfgsReport()
    fn = capi.ENERGY_FN(lambda u, xp, gp, n: 0.0)
    none = C.cast(None, capi.PROGRESS_FN)
    assert L.rvseg_minimize_lbfgs(0, x.ctypes.data_as(C.c_void_p), None, fn, none, None, None, C.byref(rep)) == capi.ERR_INVALID_ARG
    assert rep.status == capi.LBFGS_BAD_ARGUMENTS
    assert L.rvseg_minimize_lbfgs(2, None, None, fn, none, None, None, None) == capi.ERR_INVALID_ARG
    assert L.rvseg_minimize_lbfgs(2, x.ctypes.data_as(C.c_void_p), None, C.cast(None, capi.ENERGY_FN), none, None, None, None) == capi.ERR_INVALID_ARG
    with pytest.raises(TypeError):
        capi.minimize_lbfgs(quadratic, _B, no_such_parameter=1)
    # a progress callback that returns non-zero stops after that iteration; an exception of the energy comes out as itself
    x, fx, rep = capi.minimize_lbfgs(quadratic, np.full(10, 5.0), lambda *a: 1)
    assert rep["status"] == capi.LBFGS_STOPPED and rep["iterations"] == 1 and fx < quadratic(np.full(10, 5.0))[0]
    with pytest.raises(ZeroDivisionError):
        capi.minimize_lbfgs(lambda x: (1 / 0, x), _B)


class _Energy:
    """An EnergyFunction over the quadratic whose value is overridden run by run: value_of_run[r] is added to run r."""

    def __init__(self, offsets, flat=False):
        self.offsets, self.run, self.flat = offsets, -1, flat

    def initialValue(self):
        return np.full(10, 5.0, np.float32)

    def gradient(self, x):
        assert x.dtype == np.float32
        f, g = quadratic(x.astype(np.float64))
        if self.flat:   # converged wherever it is
            return self.offsets[self.run], np.zeros(10, np.float32)
        return f + self.offsets[self.run], g.astype(np.float32)


def test_restart_loop_stops_when_the_value_no_longer_falls():
    """optimization.cpp:85-94: up to restart + 1 runs, each from where the last ended; the loop ends after the first run whose
    value is not below the lowest so far."""
    import rovinasemanticsegmentation_amd as rv
    from rovinasemanticsegmentation_amd import _capi as capi
    _capi()
    real = capi.minimize_lbfgs
    runs = []

    def spy(fun, x0, progress=None, **params):
        e.run += 1
        runs.append((np.array(x0), dict(params)))
        return real(fun, x0, progress, **params)
    # (the quadratic's own value, below 1e5 from this start, falls from run to run: the offsets decide)
    for offsets, restart, want_runs, flat in (((0.0, -1e6, -2e6, -3e6), 2, 3, False),   # falls every time: all restart + 1 runs
                                              ((0.0, -1e6, 5e6, -9e6), 3, 3, False),    # the third run is higher: it is the last
                                              ((0.0, 0.0, -1.0), 2, 2, True),           # equal is not lower
                                              ((0.0,), 0, 1, False)):
        e = _Energy(offsets, flat)
        del runs[:]
        capi.minimize_lbfgs = spy
        try:
            rep = []
            x = rv.minimizeLBFGS(e, restart, max_iterations=2, report=rep)
        finally:
            capi.minimize_lbfgs = real
        assert len(runs) == want_runs == len(rep), (offsets, len(runs))
        assert x.dtype == np.float32 and x.shape == (10,)
        assert all(r[1]["max_iterations"] == 2 and r[1]["epsilon"] == 1e-6 for r in runs)
        assert np.array_equal(runs[0][0], e.initialValue().astype(np.float64))
        for a, b in zip(rep, runs[1:]):
            assert a["iterations"] == (0 if flat else 2) and b[0].dtype == np.float64   # each run starts from the last one's double result
    # defaults of the reference's call: epsilon 1e-6, at most 50 iterations
    e = _Energy((0.0,))
    e.run = 0
    rep = []
    x = rv.minimizeLBFGS(e, report=rep)
    assert rep[0]["status"] == capi.LBFGS_MAX_ITERATIONS and rep[0]["iterations"] == 50   # (this start needs about 150)
    assert rep[0]["fx"] < quadratic(np.full(10, 5.0))[0]   # 50 accepted Armijo steps: lower than the start


def test_numeric_gradient_and_grad_check():
    import rovinasemanticsegmentation_amd as rv
    _capi()
    e = _Energy((0.0,))
    e.run = 0
    x = np.linspace(0, 1, 10).astype(np.float32)
    ng = rv.numericGradient(e, x, 1e-2)
    assert ng.dtype == np.float32 and np.allclose(ng, quadratic(x.astype(np.float64))[1], rtol=1e-3, atol=1e-2)
    assert rv.gradCheck(e, x, 1e-2) < 0.5
