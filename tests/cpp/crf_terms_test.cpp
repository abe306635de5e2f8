// The dense_learning recipe (examples/dense_learning.cpp:113-182) through the C++ facade: rvseg::DenseCRF2D with a
// logistic unary, a Gaussian Potts term and a bilateral MatrixCompatibility term, the three parameter vectors read
// back and set again, DIAG kernel parameters, then map(5); the same model once more as a plain rvseg::DenseCRF over the
// feature matrices.  argv: image.ppm params.bin out.bin.  params.bin: int32 M, then L (M x 4), m (M x M) and the five
// bilateral kernel parameters as float32.  out.bin: Q (N x M float32), then the map (N int8).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <vector>

#include "rvseg_segmenter.hpp"

static std::vector<unsigned char> read_ppm(const char* path, int& W, int& H) {
    std::ifstream in(path, std::ios::binary);
    std::string magic;
    int maxv = 0;
    in >> magic >> W >> H >> maxv;
    in.get();
    std::vector<unsigned char> im((size_t)W * H * 3);
    in.read(reinterpret_cast<char*>(im.data()), (std::streamsize)im.size());
    if (magic != "P6" || maxv != 255 || !in) throw std::runtime_error("bad ppm");
    return im;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::fprintf(stderr, "usage: %s image.ppm params.bin out.bin\n", argv[0]); return 2; }
    try {
        int W = 0, H = 0;
        const auto im = read_ppm(argv[1], W, H);
        const int N = W * H;
        std::ifstream pin(argv[2], std::ios::binary);
        int32_t M = 0;
        pin.read(reinterpret_cast<char*>(&M), 4);
        std::vector<float> L((size_t)M * 4), m((size_t)M * M), kp(5);
        pin.read(reinterpret_cast<char*>(L.data()), (std::streamsize)L.size() * 4);
        pin.read(reinterpret_cast<char*>(m.data()), (std::streamsize)m.size() * 4);
        pin.read(reinterpret_cast<char*>(kp.data()), 20);
        if (!pin) throw std::runtime_error("bad params file");
        // logistic_feature(k, i) = im[3i + k] / 255., row 3 = 1 (dense_learning.cpp:115-119), point-major here
        std::vector<float> feat((size_t)N * 4, 1.f);
        for (int i = 0; i < N; i++)
            for (int k = 0; k < 3; k++) feat[(size_t)i * 4 + k] = (float)(im[3 * (size_t)i + k] / 255.);
        rvseg_params p;
        rvseg_params_default(&p);
        rvseg_ctx* ctx = nullptr;
        if (rvseg_create(&p, &ctx) != RVSEG_OK) throw std::runtime_error("rvseg_create failed");
        std::vector<float> kparams = {1.f, 1.f};
        kparams.insert(kparams.end(), kp.begin(), kp.end());

        rvseg::DenseCRF2D crf(ctx, W, H, M);
        crf.setUnaryEnergy(L.data(), feat.data(), 4);
        crf.addPairwiseGaussian(3, 3, rvseg::PottsCompatibility(1));
        crf.addPairwiseBilateral(80, 80, 13, 13, 13, im.data(), rvseg::MatrixCompatibility(m.data(), M));
        // the three vectors dense_learning.cpp:177-179 prints, pasted back in
        crf.setUnaryParameters(crf.unaryParameters());
        crf.setLabelCompatibilityParameters(crf.labelCompatibilityParameters());
        if (crf.kernelParameters().size() != kparams.size()) throw std::runtime_error("kernel parameter count");
        crf.setKernelParameters(kparams);
        std::vector<int8_t> map;
        const std::vector<float> Q = crf.inference(5, &map);
        if (crf.map(5) != map) throw std::runtime_error("map() differs from inference()");

        // the same model as a plain DenseCRF over feature matrices built by the caller
        std::vector<float> fg((size_t)N * 2), fb((size_t)N * 5);
        if (rvseg_crf_features_gaussian(W, H, 3, 3, fg.data()) != RVSEG_OK ||
            rvseg_crf_features_bilateral(W, H, 80, 80, 13, 13, 13, im.data(), fb.data()) != RVSEG_OK) throw std::runtime_error("features");
        rvseg::DenseCRF plain(ctx, N, M);
        plain.setUnaryEnergy(L.data(), feat.data(), 4);
        plain.addPairwiseEnergy(fg.data(), 2, rvseg::PottsCompatibility(1));
        plain.addPairwiseEnergy(fb.data(), 5, rvseg::MatrixCompatibility(m.data(), M), RVSEG_DIAG_KERNEL, RVSEG_NORMALIZE_SYMMETRIC);
        plain.setKernelParameters(kparams);
        if (plain.inference(5) != Q) throw std::runtime_error("DenseCRF and DenseCRF2D differ");

        std::ofstream out(argv[3], std::ios::binary);
        out.write(reinterpret_cast<const char*>(Q.data()), (std::streamsize)Q.size() * 4);
        out.write(reinterpret_cast<const char*>(map.data()), (std::streamsize)map.size());
        rvseg_destroy(ctx);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    std::printf("crf terms ok\n");
    return 0;
}
