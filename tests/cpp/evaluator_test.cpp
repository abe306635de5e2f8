// Exercises the scoring facade (include/rvseg_segmenter.hpp: RgbLabelConversion, Evaluator) the way src/test_multi.cpp
// drives the reference objects: decode colour-coded ground truth, count predictions against it, print the scores.
// usage: evaluator_test <forest.dat> <pred.i8> <gt.i8> <n_frames> <out.bin>
//   pred / gt: n x 2 x 120 x 160 int8 (the model has two layers: 8 and 9 classes)
//   out.bin:   decoded labels (n x 2 x H x W int8), then per layer C*C uint64 counts, 1 uint64 out-of-range count,
//              double global, float class average, float IoU; then the report text of layer 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "rvseg_segmenter.hpp"

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    std::fseek(f, 0, SEEK_END);
    long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> b((size_t)n);
    if (std::fread(b.data(), 1, b.size(), f) != b.size()) throw std::runtime_error("short read");
    std::fclose(f);
    return b;
}

int main(int argc, char** argv) {
    if (argc < 6) { std::fprintf(stderr, "usage\n"); return 2; }
    try {
        const int W = 160, H = 120, n = std::atoi(argv[4]);
        // resources/config.json color_codings (material, object), entry order kept
        const std::vector<rvseg::ColorCodingEntry> material = {
            {"Marble", {255, 0, 255}, 0}, {"New bricks", {0, 255, 0}, 1}, {"Plaster", {255, 153, 153}, 2},
            {"Rubble", {0, 255, 255}, 3}, {"Tufa irregular", {0, 0, 255}, 4}, {"Tufa regular", {255, 0, 0}, 5},
            {"Tufa wall", {255, 255, 0}, 6}, {"Unknown", {50, 50, 50}, 7}, {"Other", {255, 255, 255}, -2},
            {"Void", {0, 0, 0}, -1}};
        const std::vector<rvseg::ColorCodingEntry> object = {
            {"Arch", {255, 0, 255}, 0}, {"Ceiling", {255, 0, 0}, 1}, {"Epigraph", {255, 153, 153}, 2},
            {"Floor", {0, 0, 255}, 3}, {"Fresco", {255, 153, 0}, 4}, {"Niche", {0, 255, 255}, 5},
            {"Pillar", {0, 255, 0}, 6}, {"Wall", {255, 255, 0}, 7}, {"Unknown", {50, 50, 50}, 8},
            {"Other", {255, 255, 255}, -2}, {"Void", {0, 0, 0}, -1}};

        rvseg_params p;
        rvseg_params_default(&p);
        p.width = W; p.height = H;
        rvseg_ctx* ctx = nullptr;
        if (rvseg_create(&p, &ctx) != RVSEG_OK) throw std::runtime_error(rvseg_last_error(nullptr));
        if (rvseg_forest_load(ctx, argv[1]) != RVSEG_OK) throw std::runtime_error(rvseg_last_error(ctx));

        // before any coding is set, a conversion is refused with a message
        {
            std::vector<int8_t> l((size_t)W * H);
            std::vector<uint8_t> c((size_t)W * H * 3);
            if (rvseg_labels_to_rgb(ctx, 0, 1, l.data(), c.data()) != RVSEG_ERR_INVALID_ARG) { std::fprintf(stderr, "no coding accepted\n"); return 1; }
        }
        rvseg::Evaluator ev(ctx, {material, object});
        rvseg::RgbLabelConversion& mat = *ev.conversion(0);
        if (mat.getValidLabelCount() != 8 || mat.getLabelNumber("Void") != -1 || mat.getLabelName(3) != "Rubble" ||
            mat.getLabelNumber("nothing") != 0 || !mat.getLabelName(42).empty()) { std::fprintf(stderr, "name lookups\n"); return 1; }

        const size_t N = (size_t)W * H;
        const std::vector<uint8_t> pred = slurp(argv[2]);
        const std::vector<uint8_t> gt = slurp(argv[3]);
        if (pred.size() != (size_t)n * 2 * N || gt.size() != pred.size()) { std::fprintf(stderr, "bad input sizes\n"); return 1; }
        // ground truth as the reference reads it: colour-coded images, one per layer and frame
        std::vector<uint8_t> rgb(gt.size() * 3);
        std::vector<int8_t> decoded(gt.size());
        for (int f = 0; f < n; f++)
            for (int l = 0; l < 2; l++) {
                const size_t off = ((size_t)f * 2 + l) * N;
                ev.conversion(l)->labelToRgb(reinterpret_cast<const int8_t*>(gt.data()) + off, rgb.data() + off * 3);
                ev.conversion(l)->rgbToLabel(rgb.data() + off * 3, decoded.data() + off);
            }
        ev.add(n, reinterpret_cast<const int8_t*>(pred.data()), rgb.data(), RVSEG_GT_RGB);

        FILE* out = std::fopen(argv[5], "wb");
        if (!out) return 1;
        std::fwrite(decoded.data(), 1, decoded.size(), out);
        for (int l = 0; l < 2; l++) {
            uint64_t oor = 0;
            const std::vector<uint64_t> c = ev.confusion(l, &oor);
            const rvseg::EvalScores s = ev.scores(l);
            std::fwrite(c.data(), 8, c.size(), out);
            std::fwrite(&oor, 8, 1, out);
            std::fwrite(&s.global_acc, 8, 1, out);
            std::fwrite(&s.class_avg_acc, 4, 1, out);
            std::fwrite(&s.iou, 4, 1, out);
        }
        const std::string rep = ev.report(1);
        std::fwrite(rep.data(), 1, rep.size(), out);
        std::fclose(out);
        rvseg_destroy(ctx);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
