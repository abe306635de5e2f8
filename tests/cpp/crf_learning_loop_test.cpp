// The recipe of examples/dense_learning.cpp:126-182 through the C++ facade (include/rvseg_segmenter.hpp): DenseCRF2D with a
// logistic unary, three phases of minimizeLBFGS(CRFEnergy) with setL2Norm(1e-3), then map().  argv[1]: a directory with the
// scene (im.bin, gt.bin, f.bin, L.bin) and want.bin, the parameters the same loop learns over the evaluation path that sets a
// fresh model for every evaluation (tests/test_gpu_cpp_crf_learning_loop.py writes them).  The learned parameters must be
// those bit for bit, and the kept model must label like a fresh one.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "rvseg_segmenter.hpp"

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); g_fail++; } } while (0)

template <class T> static std::vector<T> load(const std::string& dir, const char* name, size_t n) {
    std::vector<T> v(n);
    std::ifstream in(dir + "/" + name, std::ios::binary);
    in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
    if (!in || in.peek() != EOF) { std::printf("%s: not %zu values\n", name, n); std::exit(2); }
    return v;
}

// an EnergyFunction that is not a CRF: minimizeLBFGS alone (restart loop, a gradient of the wrong size)
struct Bowl : rvseg::EnergyFunction {
    int calls = 0, short_from = -1;
    std::vector<float> initialValue() override { return {5.f, -3.f}; }
    double gradient(const std::vector<float>& x, std::vector<float>& dx) override {
        dx = {2 * (x[0] - 1), 8 * (x[1] - 2)};
        if (short_from >= 0 && calls >= short_from) dx.pop_back();
        calls++;
        return (double)(x[0] - 1) * (x[0] - 1) + 4.0 * (x[1] - 2) * (x[1] - 2);
    }
};

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const int W = 48, H = 32, M = 4, K = 4, NIT = 5, N = W * H;
    const auto im = load<unsigned char>(dir, "im.bin", (size_t)N * 3);
    const auto gt = load<int16_t>(dir, "gt.bin", (size_t)N);
    const auto f = load<float>(dir, "f.bin", (size_t)N * K);
    const auto L = load<float>(dir, "L.bin", (size_t)M * K);
    const auto want = load<float>(dir, "want.bin", (size_t)M * K + 1 + M * (M + 1) / 2 + 2 + 5);

    Bowl bowl;
    const std::vector<float> pb = rvseg::minimizeLBFGS(bowl, 2, false);
    CHECK(std::fabs(pb[0] - 1) < 1e-3 && std::fabs(pb[1] - 2) < 1e-3);
    Bowl bad;
    bad.short_from = 2;
    bool threw = false;
    try { rvseg::minimizeLBFGS(bad, 2, false); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw && bad.calls == 3);   // no restart after the failed run

    rvseg_params p;
    rvseg_params_default(&p);
    rvseg_ctx *ctx = nullptr, *ctx2 = nullptr;
    if (rvseg_create(&p, &ctx) != RVSEG_OK || rvseg_create(&p, &ctx2) != RVSEG_OK) { std::printf("no context: %s\n", rvseg_last_error(nullptr)); return 2; }
    std::vector<float> eye((size_t)M * M, 0.f);
    for (int i = 0; i < M; i++) eye[(size_t)i * M + i] = 1.f;
    const auto build = [&](rvseg::DenseCRF2D& crf) {
        crf.setUnaryEnergy(L.data(), f.data(), K);
        crf.addPairwiseGaussian(3, 3, rvseg::PottsCompatibility(1));
        crf.addPairwiseBilateral(80, 80, 13, 13, 13, im.data(), rvseg::MatrixCompatibility(eye.data(), M));
    };
    std::vector<float> learned;
    std::vector<int8_t> map_kept;
    try {
        rvseg::DenseCRF2D crf(ctx, W, H, M);
        build(crf);
        std::unique_ptr<rvseg::ObjectiveFunction> objective;
        if (std::string(argv[2]) == "iou") objective.reset(new rvseg::IntersectionOverUnion(gt));
        else objective.reset(new rvseg::LogLikelihood(gt, 0.01f));
        rvseg_lbfgs_params lp;
        rvseg_lbfgs_params_default(&lp);
        lp.epsilon = 1e-6;
        lp.max_iterations = 8;   // (the recipe's 50 would take long)
        const bool phases[3][3] = {{true, false, false}, {true, true, false}, {true, true, true}};
        for (const auto& ph : phases) {
            rvseg::CRFEnergy energy(crf, *objective, NIT, ph[0], ph[1], ph[2]);
            energy.setL2Norm(1e-3f);
            std::vector<float> dx;
            const double start = energy.gradient(energy.initialValue(), dx);
            const std::vector<float> x = rvseg::minimizeLBFGS(energy, 2, false, &lp);
            const double end = energy.gradient(x, dx);
            std::printf("phase %d%d%d: %.9g -> %.9g\n", ph[0], ph[1], ph[2], start, end);
            CHECK(end <= start);
            size_t id = 0;   // "save the values", dense_learning.cpp:163-174
            if (ph[0]) { const size_t n = crf.unaryParameters().size(); crf.setUnaryParameters({x.begin() + id, x.begin() + id + n}); id += n; }
            if (ph[1]) { const size_t n = crf.labelCompatibilityParameters().size(); crf.setLabelCompatibilityParameters({x.begin() + id, x.begin() + id + n}); id += n; }
            if (ph[2]) crf.setKernelParameters({x.begin() + id, x.end()});
        }
        for (const auto& part : {crf.unaryParameters(), crf.labelCompatibilityParameters(), crf.kernelParameters()}) learned.insert(learned.end(), part.begin(), part.end());
        CHECK(learned.size() == want.size());
        CHECK(learned.size() == want.size() && std::memcmp(learned.data(), want.data(), want.size() * sizeof(float)) == 0);
        for (size_t i = 0; i < learned.size() && i < want.size(); i++)
            if (std::memcmp(&learned[i], &want[i], 4)) std::printf("  parameter %zu: %.9g, want %.9g\n", i, learned[i], want[i]);
        std::vector<double> kl;
        const std::vector<float> Q_kept = crf.inferenceTrace(NIT, kl, &map_kept);   // the model changed in place all along
        // a fresh DenseCRF given the learned parameters
        rvseg::DenseCRF2D other(ctx2, W, H, M);
        build(other);
        other.setUnaryParameters(crf.unaryParameters());
        other.setLabelCompatibilityParameters(crf.labelCompatibilityParameters());
        other.setKernelParameters(crf.kernelParameters());
        std::vector<int8_t> map_fresh;
        const std::vector<float> Q = other.inference(NIT, &map_fresh);
        CHECK(map_kept == map_fresh);
        CHECK(Q.size() == Q_kept.size() && std::memcmp(Q.data(), Q_kept.data(), Q.size() * sizeof(float)) == 0);
    } catch (const std::exception& e) {
        std::printf("FAILED: %s\n", e.what());
        g_fail++;
    }
    rvseg_destroy(ctx);
    rvseg_destroy(ctx2);
    if (g_fail) return 1;
    std::printf("crf learning loop ok\n");
    return 0;
}
