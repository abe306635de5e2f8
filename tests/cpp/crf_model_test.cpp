// Stepwise inference, energies and KL divergence through the C++ facade (rvseg::DenseCRF in include/rvseg_segmenter.hpp):
// a model with a Potts term and a Matrix term.  argv: in.bin out.bin.  in.bin: int32 N, C, d0, d1, then U (N x C), F0
// (N x d0), F1 (N x d1), m (C x C) as float32 and N int8 labels.  out.bin: Q after start + 1 step, Q after 3 steps,
// currentMap of it (N int8), unary and pairwise energy of the labels (N float32 each), then as float64 the KL divergence
// of the 3-step Q, its 4 parts and the 4 values of inferenceTrace(3), then the traced Q.
#include <cstdio>
#include <fstream>
#include <vector>

#include "rvseg_segmenter.hpp"

template <class T>
static void put(std::ofstream& out, const std::vector<T>& v) { out.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T))); }

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        int32_t h[4];
        in.read(reinterpret_cast<char*>(h), 16);
        const int N = h[0], C = h[1], d0 = h[2], d1 = h[3];
        std::vector<float> U((size_t)N * C), F0((size_t)N * d0), F1((size_t)N * d1), m((size_t)C * C);
        std::vector<int8_t> labels((size_t)N);
        in.read(reinterpret_cast<char*>(U.data()), (std::streamsize)U.size() * 4);
        in.read(reinterpret_cast<char*>(F0.data()), (std::streamsize)F0.size() * 4);
        in.read(reinterpret_cast<char*>(F1.data()), (std::streamsize)F1.size() * 4);
        in.read(reinterpret_cast<char*>(m.data()), (std::streamsize)m.size() * 4);
        in.read(reinterpret_cast<char*>(labels.data()), N);
        if (!in) throw std::runtime_error("bad input file");
        rvseg_params p;
        rvseg_params_default(&p);
        rvseg_ctx* ctx = nullptr;
        if (rvseg_create(&p, &ctx) != RVSEG_OK) throw std::runtime_error("rvseg_create failed");
        {
            rvseg::DenseCRF crf(ctx, N, C);
            crf.setUnaryEnergy(U.data());
            crf.addPairwiseEnergy(F0.data(), d0, rvseg::PottsCompatibility(2.5f), RVSEG_DIAG_KERNEL, RVSEG_NORMALIZE_AFTER);
            crf.addPairwiseEnergy(F1.data(), d1, rvseg::MatrixCompatibility(m.data(), C));
            std::vector<float> Q = crf.startInference();
            crf.stepInference(Q);
            const std::vector<float> Q1 = Q;
            const std::vector<float> Qi = crf.inference(3);   // replaces the context's model: the next call sets it again
            crf.stepInference(Q, 2);
            if (Q != Qi) throw std::runtime_error("start + 3 steps differ from inference(3)");
            const std::vector<int8_t> map = crf.currentMap(Q);
            if (map != crf.map(3)) throw std::runtime_error("currentMap differs from map(3)");
            const std::vector<float> ue = crf.unaryEnergy(labels), pe = crf.pairwiseEnergy(labels);
            std::vector<double> parts, trace;
            const double kl = crf.klDivergence(Q, &parts);
            if (parts.size() != 4 || kl != ((parts[0] + parts[1]) + parts[2]) + parts[3]) throw std::runtime_error("KL is not the sum of its parts");
            const std::vector<float> Qt = crf.inferenceTrace(3, trace);
            if (trace.size() != 4 || trace[3] != kl) throw std::runtime_error("the trace's last KL differs from klDivergence");
            // a second object on the same context takes the model over, and the first one takes it back
            rvseg::DenseCRF other(ctx, N, C);
            other.setUnaryEnergy(U.data());
            if (other.startInference() == Q1) throw std::runtime_error("a model without terms stepped like one with terms");
            std::vector<float> Q2 = crf.startInference();
            crf.stepInference(Q2);
            if (Q2 != Q1) throw std::runtime_error("the first object did not set its model again");
            // a model that somebody sets on the context directly is not the object's either
            if (rvseg_crf_model_set(ctx, N, C, 0, nullptr, U.data(), 1) != RVSEG_OK) throw std::runtime_error("rvseg_crf_model_set failed");
            Q2 = crf.startInference();
            crf.stepInference(Q2);
            if (Q2 != Q1) throw std::runtime_error("the object computed on a model set behind its back");
            std::ofstream out(argv[2], std::ios::binary);
            put(out, Q1); put(out, Q); put(out, map); put(out, ue); put(out, pe);
            put(out, std::vector<double>{kl}); put(out, parts); put(out, trace); put(out, Qt);
            if (!out) throw std::runtime_error("cannot write the output");
        }
        rvseg_destroy(ctx);
        std::printf("crf model ok\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "crf_model_test: %s\n", e.what());
        return 1;
    }
}
