// rvseg_minimize_lbfgs over rvseg_lbfgs.cpp alone: a stand-alone program for the host compiler with
// -fsanitize=address,undefined (tests/test_lbfgs_cpp_cpu.py).  The three problems of tests/test_lbfgs_cpu.py.
#include <cmath>
#include <cstdio>
#include <vector>

#include "rvseg.h"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); g_fail++; } } while (0)

static double quadratic(void*, const double* x, double* g, int32_t n) {
    double f = 0.0;
    for (int i = 0; i < n; i++) {
        const double d = std::pow(10.0, 3.0 * i / (n - 1)), r = x[i] - (-1.0 + 3.0 * i / (n - 1));
        f += 0.5 * d * r * r;
        g[i] = d * r;
    }
    return f;
}
static double rosenbrock(void*, const double* x, double* g, int32_t) {
    const double a = x[0], b = x[1];
    g[0] = -2 * (1 - a) - 400 * a * (b - a * a);
    g[1] = 200 * (b - a * a);
    return (1 - a) * (1 - a) + 100 * (b - a * a) * (b - a * a);
}
static double scalar(void*, const double* x, double* g, int32_t) {
    g[0] = std::sinh(x[0] - 3.0);
    return std::cosh(x[0] - 3.0);
}
struct Seen { double last; int n; bool rose; };
static int32_t progress(void* user, const double*, const double*, double fx, double, double, double, int32_t, int32_t k, int32_t) {
    Seen* s = static_cast<Seen*>(user);
    if (fx > s->last) s->rose = true;
    s->last = fx;
    s->n = k;
    return 0;
}
struct Nan { int calls; };
static double nan_after_two(void* user, const double* x, double* g, int32_t n) {
    Nan* s = static_cast<Nan*>(user);
    const double f = quadratic(nullptr, x, g, n);
    return ++s->calls >= 3 ? std::nan("") : f;
}

static void run(const char* name, rvseg_energy_fn fn, std::vector<double> x0, int max_iterations) {
    const int n = (int)x0.size();
    std::vector<double> g(x0.size()), x = x0;
    const double f0 = fn(nullptr, x0.data(), g.data(), n);
    rvseg_lbfgs_params p;
    rvseg_lbfgs_params_default(&p);
    p.max_iterations = max_iterations;
    rvseg_lbfgs_report rep;
    Seen seen{f0, 0, false};
    double fx = 0.0;
    // (progress gets `seen` as user, so the energies above ignore theirs)
    CHECK(rvseg_minimize_lbfgs(n, x.data(), &fx, fn, progress, &seen, &p, &rep) == RVSEG_OK);
    CHECK(rep.status == RVSEG_LBFGS_CONVERGED);
    const double f = fn(nullptr, x.data(), g.data(), n);
    double gn = 0.0, xn = 0.0;
    for (int i = 0; i < n; i++) { gn += g[i] * g[i]; xn += x[i] * x[i]; }
    CHECK(f == fx && std::sqrt(gn) / std::fmax(1.0, std::sqrt(xn)) < p.epsilon);
    CHECK(!seen.rose && seen.n == rep.iterations && fx <= f0);
    std::printf("%s: %d iterations, %d evaluations, fx = %.3g\n", name, rep.iterations, rep.evaluations, fx);
    x = x0;
    p.max_iterations = 3;
    CHECK(rvseg_minimize_lbfgs(n, x.data(), &fx, fn, nullptr, nullptr, &p, &rep) == RVSEG_OK);
    CHECK(rep.status == RVSEG_LBFGS_MAX_ITERATIONS && rep.iterations == 3 && fx <= f0);
}

int main() {
    run("quadratic", quadratic, std::vector<double>(10, 5.0), 0);
    run("rosenbrock", rosenbrock, {-1.2, 1.0}, 500);
    run("scalar", scalar, {-1.0}, 0);
    std::vector<double> x(10, 5.0);
    Nan st{0};
    rvseg_lbfgs_report rep;
    double fx = 0.0;
    CHECK(rvseg_minimize_lbfgs(10, x.data(), &fx, nan_after_two, nullptr, &st, nullptr, &rep) == RVSEG_ERR_INVALID_ARG);
    CHECK(rep.status == RVSEG_LBFGS_NOT_FINITE && std::isfinite(fx));
    CHECK(rvseg_minimize_lbfgs(0, x.data(), &fx, quadratic, nullptr, nullptr, nullptr, nullptr) == RVSEG_ERR_INVALID_ARG);
    if (g_fail) return 1;
    std::printf("lbfgs ok\n");
    return 0;
}
