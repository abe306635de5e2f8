// rvseg_minimize_lbfgs (include/rvseg.h, "The minimiser"): limited-memory BFGS with a backtracking Armijo line search, in
// double on the host.  The project's own, written from the algorithm (Nocedal & Wright, Numerical Optimization, algorithms
// 7.4 and 7.5); no HIP, no context.
#include <cmath>
#include <vector>

#include "rvseg.h"

namespace {

double dot(const std::vector<double>& a, const std::vector<double>& b) {
    double s = 0.0;
    for (size_t i = 0; i < a.size(); i++) s += a[i] * b[i];
    return s;
}

bool finite_all(double f, const std::vector<double>& g) {
    if (!std::isfinite(f)) return false;
    for (double v : g) if (!std::isfinite(v)) return false;
    return true;
}

struct Pair { std::vector<double> s, y; double rho; };

}  // namespace

extern "C" {

void rvseg_lbfgs_params_default(rvseg_lbfgs_params* p) {
    if (!p) return;
    p->m = 6;
    p->max_iterations = 0;
    p->max_linesearch = 20;
    p->reserved = 0;
    p->epsilon = 1e-5;
    p->ftol = 1e-4;
    p->min_step = 1e-20;
    p->max_step = 1e20;
}

rvseg_status rvseg_minimize_lbfgs(int32_t n, double* x_io, double* fx_out, rvseg_energy_fn energy, rvseg_progress_fn progress, void* user,
                                  const rvseg_lbfgs_params* params, rvseg_lbfgs_report* out) {
    rvseg_lbfgs_params p;
    rvseg_lbfgs_params_default(&p);
    if (params) p = *params;
    rvseg_lbfgs_report rep{RVSEG_LBFGS_BAD_ARGUMENTS, 0, 0, 0, 0.0, 0.0};
    if (out) *out = rep;
    if (n <= 0 || !x_io || !energy || p.m < 1 || !(p.epsilon >= 0.0) || p.max_iterations < 0 || p.max_linesearch < 1 ||
        !(p.ftol > 0.0 && p.ftol < 1.0) || !(p.min_step > 0.0) || !(p.max_step >= p.min_step)) return RVSEG_ERR_INVALID_ARG;

    const size_t N = (size_t)n;
    std::vector<double> x(x_io, x_io + N), g(N), xn(N), gn(N), d(N), best(x);
    std::vector<Pair> hist;   // oldest first, at most m
    std::vector<double> alpha;
    double fx = energy(user, x.data(), g.data(), n);
    rep.evaluations = 1;
    double fbest = fx;
    // the end of every path: the point returned, its value, the report
    const auto finish = [&](int status, const std::vector<double>& at, double f, double gnorm, rvseg_status st) {
        for (size_t i = 0; i < N; i++) x_io[i] = at[i];
        if (fx_out) *fx_out = f;
        rep.status = status;
        rep.gnorm = gnorm;
        rep.xnorm = std::sqrt(dot(at, at));
        if (out) *out = rep;
        return st;
    };
    if (!finite_all(fx, g)) return finish(RVSEG_LBFGS_NOT_FINITE, x, fx, 0.0, RVSEG_ERR_INVALID_ARG);   // (x as given)
    double gnorm = std::sqrt(dot(g, g)), xnorm = std::sqrt(dot(x, x));
    if (gnorm / std::fmax(1.0, xnorm) < p.epsilon) return finish(RVSEG_LBFGS_CONVERGED, x, fx, gnorm, RVSEG_OK);
    for (size_t i = 0; i < N; i++) d[i] = -g[i];
    double step = 1.0 / gnorm;

    for (int k = 1;; k++) {
        double dg = dot(g, d);
        if (!(dg < 0.0)) {   // not a descent direction (rounding in the recursion): steepest descent without history
            hist.clear();
            for (size_t i = 0; i < N; i++) d[i] = -g[i];
            dg = -gnorm * gnorm;
            step = 1.0 / gnorm;
        }
        // backtracking: halve t until f(x + t d) <= f(x) + ftol t g.d
        double t = std::fmin(std::fmax(step, p.min_step), p.max_step), fn = 0.0;
        int ls = 0;
        bool accepted = false;
        while (ls < p.max_linesearch && t >= p.min_step) {
            for (size_t i = 0; i < N; i++) xn[i] = x[i] + t * d[i];
            fn = energy(user, xn.data(), gn.data(), n);
            ls++;
            rep.evaluations++;
            if (!finite_all(fn, gn)) return finish(RVSEG_LBFGS_NOT_FINITE, best, fbest, gnorm, RVSEG_ERR_INVALID_ARG);
            if (fn < fbest) { fbest = fn; best = xn; }
            if (fn <= fx + p.ftol * t * dg) { accepted = true; break; }
            t *= 0.5;
        }
        if (!accepted) {
            const bool at_x = !(fbest < fx);   // (the gradient norm reported is that of the last accepted point)
            return finish(RVSEG_LBFGS_LINESEARCH_FAILED, at_x ? x : best, at_x ? fx : fbest, gnorm, RVSEG_OK);
        }
        Pair pr;
        pr.s.resize(N);
        pr.y.resize(N);
        for (size_t i = 0; i < N; i++) { pr.s[i] = xn[i] - x[i]; pr.y[i] = gn[i] - g[i]; }
        x.swap(xn);
        g.swap(gn);
        fx = fn;
        if (!(fbest < fx)) { fbest = fx; best = x; }
        rep.iterations = k;
        gnorm = std::sqrt(dot(g, g));
        xnorm = std::sqrt(dot(x, x));
        if (progress && progress(user, x.data(), g.data(), fx, xnorm, gnorm, t, n, k, ls))
            return finish(RVSEG_LBFGS_STOPPED, x, fx, gnorm, RVSEG_OK);
        if (gnorm / std::fmax(1.0, xnorm) < p.epsilon) return finish(RVSEG_LBFGS_CONVERGED, x, fx, gnorm, RVSEG_OK);
        if (p.max_iterations > 0 && k >= p.max_iterations) return finish(RVSEG_LBFGS_MAX_ITERATIONS, x, fx, gnorm, RVSEG_OK);
        // a pair without positive curvature (the Armijo condition alone does not ensure it) would break H > 0: left out
        const double ys = dot(pr.y, pr.s), yy = dot(pr.y, pr.y);
        if (ys > 1e-300 && yy > 0.0 && std::isfinite(1.0 / ys)) {
            pr.rho = 1.0 / ys;
            if ((int)hist.size() == p.m) hist.erase(hist.begin());
            hist.push_back(std::move(pr));
        }
        // two-loop recursion: d = -H g, H0 = (s.y / y.y) I of the newest pair
        for (size_t i = 0; i < N; i++) d[i] = -g[i];
        alpha.assign(hist.size(), 0.0);
        for (size_t j = hist.size(); j-- > 0;) {
            alpha[j] = hist[j].rho * dot(hist[j].s, d);
            for (size_t i = 0; i < N; i++) d[i] -= alpha[j] * hist[j].y[i];
        }
        if (!hist.empty()) {
            const Pair& last = hist.back();
            const double gamma = 1.0 / (last.rho * dot(last.y, last.y));
            for (size_t i = 0; i < N; i++) d[i] *= gamma;
        }
        for (size_t j = 0; j < hist.size(); j++) {
            const double beta = hist[j].rho * dot(hist[j].y, d);
            for (size_t i = 0; i < N; i++) d[i] += (alpha[j] - beta) * hist[j].s[i];
        }
        step = hist.empty() ? 1.0 / gnorm : 1.0;
    }
}

}  // extern "C"
