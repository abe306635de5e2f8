// Learning through the C++ facade (rvseg::DenseCRF::gradient / applyTranspose and the objective structs in
// include/rvseg_segmenter.hpp) against the C ABI on a second context: a 3-class model with a Potts and a Matrix term and a
// logistic unary.  No arguments; prints "crf learn ok".
#include <cstdio>
#include <cstring>
#include <vector>

#include "rvseg_segmenter.hpp"

static uint32_t lcg_state = 12345u;
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
        const int N = 500, C = 3, K = 4, d0 = 2, d1 = 3, NIT = 3;
        std::vector<float> L((size_t)C * K), f((size_t)N * K), F0((size_t)N * d0), F1((size_t)N * d1), m((size_t)C * C), x((size_t)N * C);
        for (auto& v : L) v = uniform01() - 0.5f;
        for (auto& v : f) v = uniform01();
        for (auto& v : F0) v = 6.f * uniform01();
        for (auto& v : F1) v = 6.f * uniform01();
        for (auto& v : m) v = uniform01() - 0.5f;
        for (auto& v : x) v = uniform01() - 0.5f;
        std::vector<int16_t> gt((size_t)N);
        for (int i = 0; i < N; i++) gt[i] = (int16_t)((int)(uniform01() * (C + 2)) - 1);   // -1 .. C: some points are skipped
        rvseg_params p;
        rvseg_params_default(&p);
        rvseg_ctx *ctx = nullptr, *abi = nullptr;
        if (rvseg_create(&p, &ctx) != RVSEG_OK || rvseg_create(&p, &abi) != RVSEG_OK) throw std::runtime_error("rvseg_create failed");
        {
            rvseg::DenseCRF crf(ctx, N, C);
            crf.setUnaryEnergy(L.data(), f.data(), K);
            crf.addPairwiseEnergy(F0.data(), d0, rvseg::PottsCompatibility(1.5f));
            crf.addPairwiseEnergy(F1.data(), d1, rvseg::MatrixCompatibility(m.data(), C), RVSEG_DIAG_KERNEL, RVSEG_NORMALIZE_BEFORE);
            // the same model through the C ABI
            const rvseg::MatrixCompatibility W(m.data(), C);
            const float w = 1.5f;
            rvseg_crf_term terms[2] = {{d0, RVSEG_COMPAT_POTTS, RVSEG_DIAG_KERNEL, RVSEG_NORMALIZE_SYMMETRIC, F0.data(), &w, nullptr},
                                       {d1, RVSEG_COMPAT_MATRIX, RVSEG_DIAG_KERNEL, RVSEG_NORMALIZE_BEFORE, F1.data(), W.params.data(), nullptr}};
            std::vector<float> U((size_t)N * C);
            ok(abi, rvseg_crf_logistic_unary(abi, N, C, K, L.data(), f.data(), U.data()));
            ok(abi, rvseg_crf_model_set(abi, N, C, 2, terms, U.data(), 1));
            const std::vector<float> weights = {0.5f, 0.25f, 0.25f};
            const rvseg::LogLikelihood ll(gt, 0.01f);
            const rvseg::Hamming ham(gt, weights);
            const rvseg::IntersectionOverUnion iou(gt);
            const rvseg::ObjectiveFunction* objectives[3] = {&ll, &ham, &iou};
            const size_t n_cg = 1 + (size_t)C * (C + 1) / 2;
            for (const rvseg::ObjectiveFunction* o : objectives) {
                std::vector<float> du, dl, dU;
                const double r = crf.gradient(NIT, *o, &du, &dl, &dU);
                const rvseg_crf_objective rec = o->record();
                double r2 = 0;
                std::vector<float> ug((size_t)N * C);
                std::vector<double> cg(n_cg), lg((size_t)C * K);
                ok(abi, rvseg_crf_model_gradient(abi, NIT, &rec, &r2, ug.data(), cg.data(), nullptr));
                ok(abi, rvseg_crf_logistic_gradient(abi, N, C, K, ug.data(), f.data(), lg.data()));
                const std::vector<float> cg32(cg.begin(), cg.end()), lg32(lg.begin(), lg.end());
                if (std::memcmp(&r, &r2, 8) != 0 || !same_bits(dU, ug) || !same_bits(dl, cg32) || !same_bits(du, lg32))
                    throw std::runtime_error("DenseCRF::gradient differs from the C ABI");
                if (dl.size() != crf.labelCompatibilityParameters().size() || du.size() != crf.unaryParameters().size())
                    throw std::runtime_error("gradient layouts differ from the parameter layouts");
                bool any = false;
                for (float v : dl) any = any || v != 0.f;
                if (!any) throw std::runtime_error("the compatibility gradient is all zero");
            }
            // applyTranspose on a d = 3 lattice without normalisation: the blur runs its axes backwards, so it differs from
            // apply, and it equals the C ABI
            rvseg::DenseCRF plain(ctx, N, C);
            std::vector<float> zeros((size_t)N * C, 0.f);
            plain.setUnaryEnergy(zeros.data());
            plain.addPairwiseEnergy(F1.data(), d1, rvseg::PottsCompatibility(1.f), RVSEG_DIAG_KERNEL, RVSEG_NO_NORMALIZATION);
            const std::vector<float> t = plain.applyTranspose(0, x);
            const float one = 1.f;
            rvseg_crf_term pt = {d1, RVSEG_COMPAT_POTTS, RVSEG_DIAG_KERNEL, RVSEG_NO_NORMALIZATION, F1.data(), &one, nullptr};
            ok(abi, rvseg_crf_model_set(abi, N, C, 1, &pt, zeros.data(), 1));
            std::vector<float> t_abi((size_t)N * C), a_abi((size_t)N * C);
            ok(abi, rvseg_crf_model_apply_transpose(abi, 0, x.data(), t_abi.data()));
            ok(abi, rvseg_crf_model_apply(abi, 0, x.data(), a_abi.data()));
            if (!same_bits(t, t_abi)) throw std::runtime_error("applyTranspose differs from the C ABI");
            if (same_bits(t, a_abi)) throw std::runtime_error("applyTranspose equals apply: the blur order was not reversed");
        }
        rvseg_destroy(ctx);
        rvseg_destroy(abi);
        std::printf("crf learn ok\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
