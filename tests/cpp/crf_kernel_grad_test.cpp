// The kernel-parameter gradient through the C++ facade (rvseg::DenseCRF::gradient(.., &kernel_grad) and kernelGradient in
// include/rvseg_segmenter.hpp) against the C ABI on a second context: a 3-class model with a CONST Potts term, a DIAG Matrix
// term and a FULL Diagonal term with non-unit kernel parameters.  No arguments; prints "crf kernel grad ok".
#include <cstdio>
#include <cstring>
#include <vector>

#include "rvseg_segmenter.hpp"

static uint32_t lcg_state = 2468u;
static float uniform01() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return (float)(lcg_state >> 8) / 16777216.0f;
}

static void ok(rvseg_ctx* ctx, rvseg_status st) {
    if (st != RVSEG_OK) throw std::runtime_error(std::string("C ABI: ") + rvseg_last_error(ctx));
}

template <class T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0; }

int main() {
    try {
        const int N = 400, C = 3, d0 = 2, d1 = 3, d2 = 2, NIT = 2;
        std::vector<float> U((size_t)N * C), F0((size_t)N * d0), F1((size_t)N * d1), F2((size_t)N * d2), m((size_t)C * C), v(C), x((size_t)N * C);
        for (auto& e : U) e = 3.f * uniform01();
        for (auto& e : F0) e = 6.f * uniform01();
        for (auto& e : F1) e = 6.f * uniform01();
        for (auto& e : F2) e = 6.f * uniform01();
        for (auto& e : m) e = 0.2f * (uniform01() - 0.5f);
        for (auto& e : v) e = -0.1f - 0.2f * uniform01();
        for (auto& e : x) e = uniform01() - 0.5f;
        std::vector<int16_t> gt((size_t)N);
        for (int i = 0; i < N; i++) gt[i] = (int16_t)((int)(uniform01() * (C + 2)) - 1);   // -1 .. C: some points are skipped
        // kernel parameters in the layout of kernelParameters(): CONST none, DIAG d1, FULL d2 x d2 column-major (not symmetric)
        const std::vector<float> kp = {1.2f, 0.8f, 1.1f, 1.1f, 0.2f, -0.1f, 0.9f};
        rvseg_params p;
        rvseg_params_default(&p);
        rvseg_ctx *ctx = nullptr, *abi = nullptr;
        if (rvseg_create(&p, &ctx) != RVSEG_OK || rvseg_create(&p, &abi) != RVSEG_OK) throw std::runtime_error("rvseg_create failed");
        {
            rvseg::DenseCRF crf(ctx, N, C);
            crf.setUnaryEnergy(U.data());
            crf.addPairwiseEnergy(F0.data(), d0, rvseg::PottsCompatibility(0.3f), RVSEG_CONST_KERNEL, RVSEG_NORMALIZE_SYMMETRIC);
            crf.addPairwiseEnergy(F1.data(), d1, rvseg::MatrixCompatibility(m.data(), C), RVSEG_DIAG_KERNEL, RVSEG_NORMALIZE_BEFORE);
            crf.addPairwiseEnergy(F2.data(), d2, rvseg::DiagonalCompatibility(v), RVSEG_FULL_KERNEL, RVSEG_NORMALIZE_AFTER);
            crf.setKernelParameters(kp);
            if (crf.kernelParameters() != kp) throw std::runtime_error("kernelParameters() does not return what was set");
            // the same model through the C ABI
            const rvseg::MatrixCompatibility W(m.data(), C);
            const float w = 0.3f;
            rvseg_crf_term terms[3] = {{d0, RVSEG_COMPAT_POTTS, RVSEG_CONST_KERNEL, RVSEG_NORMALIZE_SYMMETRIC, F0.data(), &w, nullptr},
                                       {d1, RVSEG_COMPAT_MATRIX, RVSEG_DIAG_KERNEL, RVSEG_NORMALIZE_BEFORE, F1.data(), W.params.data(), kp.data()},
                                       {d2, RVSEG_COMPAT_DIAGONAL, RVSEG_FULL_KERNEL, RVSEG_NORMALIZE_AFTER, F2.data(), v.data(), kp.data() + d1}};
            ok(abi, rvseg_crf_model_set(abi, N, C, 3, terms, U.data(), 1));
            const rvseg::LogLikelihood ll(gt, 0.01f);
            const rvseg_crf_objective rec = ll.record();
            const size_t n_cg = 1 + (size_t)C * (C + 1) / 2 + C, n_kg = kp.size();
            std::vector<float> dl, dU, dk;
            const double r = crf.gradient(NIT, ll, nullptr, &dl, &dU, &dk);
            double r2 = 0;
            std::vector<float> ug((size_t)N * C);
            std::vector<double> cg(n_cg), kg(n_kg);
            ok(abi, rvseg_crf_model_gradient_kernel(abi, NIT, &rec, &r2, ug.data(), cg.data(), kg.data(), nullptr));
            const std::vector<float> cg32(cg.begin(), cg.end()), kg32(kg.begin(), kg.end());
            if (std::memcmp(&r, &r2, 8) != 0 || !same_bits(dU, ug) || !same_bits(dl, cg32)) throw std::runtime_error("DenseCRF::gradient differs from the C ABI");
            if (!same_bits(dk, kg32)) throw std::runtime_error("kernel_grad differs from the C ABI's doubles rounded to fp32");
            if (dk.size() != crf.kernelParameters().size()) throw std::runtime_error("kernel_grad's layout differs from kernelParameters()");
            bool any = false;
            for (float e : dk) any = any || e != 0.f;
            if (!any) throw std::runtime_error("the kernel gradient is all zero");
            // without kernel_grad: the same value and gradients
            std::vector<float> dl2, dU2;
            const double r3 = crf.gradient(NIT, ll, nullptr, &dl2, &dU2);
            if (std::memcmp(&r, &r3, 8) != 0 || !same_bits(dl, dl2) || !same_bits(dU, dU2)) throw std::runtime_error("gradient changes with kernel_grad");
            // kernelGradient(term, b, Q) = kernel_gradient(b, compat_apply(Q)) of the C ABI, per term
            std::vector<float> Q((size_t)N * C), lbl((size_t)N * C);
            ok(abi, rvseg_crf_model_start(abi, Q.data()));
            const int sizes[3] = {0, d1, d2 * d2};
            for (int t = 0; t < 3; t++) {
                const std::vector<float> g = crf.kernelGradient(t, x, Q);
                std::vector<double> g64((size_t)sizes[t] + 1);
                ok(abi, rvseg_crf_model_compat_apply(abi, t, Q.data(), lbl.data()));
                ok(abi, rvseg_crf_model_kernel_gradient(abi, t, x.data(), lbl.data(), g64.data(), nullptr));
                if (!same_bits(g, std::vector<float>(g64.begin(), g64.end() - 1))) throw std::runtime_error("kernelGradient differs from the C ABI");
            }
        }
        rvseg_destroy(ctx);
        rvseg_destroy(abi);
        std::printf("crf kernel grad ok\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
