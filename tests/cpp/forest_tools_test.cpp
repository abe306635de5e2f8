// The C++ forest tools of include/rvseg_segmenter.hpp (rvseg::AccuracyTool, ConfusionMatrixTool, CorrelationTool, refit)
// on the golden forest_tiny.dat (D 4, 2 trees, 2 single-label classes): their floats against counts made here by a plain
// loop over the labels and votes of rvseg_forest_classify / _classify_trees (tests/test_gpu_forest_tools.py pins those to
// the restatement), with the reference's three divisions written out.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "rvseg_segmenter.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main(int argc, char** argv) {
    CHECK(argc == 2);
    rvseg_params p;
    rvseg_params_default(&p);
    p.multi_layer = 0;
    p.patch_size_reduce = 1;
    p.feature_height = 0;
    p.feature_normal = 0;
    rvseg_ctx* ctx = nullptr;
    CHECK(rvseg_create(&p, &ctx) == RVSEG_OK);
    const int D = rvseg_feature_length(ctx), P = 777;
    CHECK(D == 4);
    CHECK(rvseg_forest_load(ctx, argv[1]) == RVSEG_OK);
    int32_t T = 0, n_layers = 0, cc[RVSEG_MAX_LAYERS];
    CHECK(rvseg_forest_info(ctx, &T, nullptr, nullptr, &n_layers, cc) == RVSEG_OK && T == 2 && n_layers == 1 && cc[0] == 2);
    const int C = cc[0];

    std::vector<float> X((size_t)P * D);
    uint32_t s = 12345u;
    for (float& v : X) { s = s * 1664525u + 1013904223u; v = (float)((s >> 16) & 255u); }
    std::vector<int32_t> pred((size_t)P), labels((size_t)P);
    std::vector<uint8_t> votes((size_t)T * P);
    CHECK(rvseg_forest_classify(ctx, X.data(), P, D, 0, pred.data()) == RVSEG_OK);
    CHECK(rvseg_forest_classify_trees(ctx, X.data(), P, D, 0, votes.data()) == RVSEG_OK);
    for (int i = 0; i < P; i++) labels[(size_t)i] = (pred[(size_t)i] + (i % 3 == 0 ? 1 : 0)) % C;

    // the reference's loops (tools.cpp:68-77, 121-135, 221-229)
    int error = 0;
    std::vector<std::vector<float>> conf((size_t)C, std::vector<float>((size_t)C, 0.f));
    std::vector<int> classCounts((size_t)C, 0);
    for (int n = 0; n < P; n++) {
        if (pred[(size_t)n] != labels[(size_t)n]) error++;
        conf[(size_t)labels[(size_t)n]][(size_t)pred[(size_t)n]] += 1;
        classCounts[(size_t)labels[(size_t)n]] += 1;
    }
    for (int c = 0; c < C; c++)
        for (int k = 0; k < C; k++) conf[(size_t)c][(size_t)k] /= classCounts[(size_t)c];
    const float accuracy = 1.0f - error / static_cast<float>(P);
    CHECK(error > 0 && error < P);

    CHECK(rvseg::AccuracyTool().measure(ctx, X.data(), P, D, labels.data()) == accuracy);
    const std::vector<std::vector<float>> got_conf = rvseg::ConfusionMatrixTool().measure(ctx, X.data(), P, D, labels.data());
    CHECK(got_conf == conf);
    const std::vector<std::vector<float>> corr = rvseg::CorrelationTool().measure(ctx, X.data(), P, D);
    CHECK((int)corr.size() == T);
    bool between = false;
    for (int t = 0; t < T; t++)
        for (int tt = t; tt < T; tt++) {
            int dist = 0;
            for (int n = 0; n < P; n++) dist += votes[(size_t)t * P + n] != votes[(size_t)tt * P + n];
            const float normalizedDistance = dist / static_cast<float>(P);
            CHECK(corr[(size_t)t][(size_t)tt] == 1 - normalizedDistance && corr[(size_t)tt][(size_t)t] == 1 - normalizedDistance);
            between = between || (dist > 0 && dist < P);
        }
    CHECK(between && corr[0][0] == 1.f && corr[1][1] == 1.f);
    rvseg::AccuracyTool().print(accuracy);
    rvseg::ConfusionMatrixTool().print(got_conf);
    rvseg::CorrelationTool().print(corr);

    // a label out of range is refused with the library's message
    labels[5] = C;
    bool thrown = false;
    try { rvseg::AccuracyTool().measure(ctx, X.data(), P, D, labels.data()); } catch (const std::runtime_error& e) { thrown = std::string(e.what()).find("label") != std::string::npos; }
    CHECK(thrown);
    labels[5] = 0;

    // refit: forest_tiny carries a single-label head beside two layers (3 | 2): the layers are re-estimated, the structure stays
    std::vector<int32_t> two((size_t)P * 2);
    for (int i = 0; i < P; i++) { two[(size_t)i * 2] = i % 3; two[(size_t)i * 2 + 1] = labels[(size_t)i]; }
    std::ifstream is(argv[1], std::ios::binary);
    const std::vector<uint8_t> loaded((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
    const std::vector<uint8_t> refitted = rvseg::refit(ctx, X.data(), P, D, two.data(), {3, 2});
    CHECK(refitted.size() == loaded.size() && refitted != loaded);
    int32_t t2 = 0, nodes2 = 0;
    CHECK(rvseg_forest_check(refitted.data(), refitted.size(), D, &t2, &nodes2, nullptr, nullptr, 0) == RVSEG_OK && t2 == 2);
    bool refused = false;
    try { rvseg::refit(ctx, X.data(), P, D, two.data(), {3, 3}); } catch (const std::runtime_error&) { refused = true; }
    CHECK(refused);

    rvseg_destroy(ctx);
    std::printf("forest tools ok\n");
    return 0;
}
