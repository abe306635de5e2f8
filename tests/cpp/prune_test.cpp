// The C++ pruner of include/rvseg_segmenter.hpp (rvseg::RandomForestPrune) on the golden forest_single.dat (D 366, 4 trees,
// 9 classes): the chain's claims that need no second implementation -- the best energy is the energy of the best state
// (rvseg_forest_prune_energy), no trace row lies below it, a second run repeats the first -- and prune() leaves the
// context with the best state's trees.  The trajectory itself is pinned in tests/test_gpu_prune.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rvseg_segmenter.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main(int argc, char** argv) {
    CHECK(argc == 2);
    rvseg_params p;
    rvseg_params_default(&p);
    p.multi_layer = 0;
    rvseg_ctx* ctx = nullptr;
    CHECK(rvseg_create(&p, &ctx) == RVSEG_OK);
    const int D = rvseg_feature_length(ctx), P = 777;
    CHECK(rvseg_forest_load(ctx, argv[1]) == RVSEG_OK);
    int32_t T = 0, n_layers = 0, cc[RVSEG_MAX_LAYERS];
    CHECK(rvseg_forest_info(ctx, &T, nullptr, nullptr, &n_layers, cc) == RVSEG_OK && T == 4 && n_layers == 1 && cc[0] == 9);

    std::vector<float> X((size_t)P * D);
    uint32_t s = 12345u;
    for (float& v : X) { s = s * 1664525u + 1013904223u; v = (float)((s >> 16) & 255u); }
    std::vector<int32_t> labels((size_t)P);
    CHECK(rvseg_forest_classify(ctx, X.data(), P, D, 0, labels.data()) == RVSEG_OK);
    for (int i = 0; i < P; i += 3) labels[(size_t)i] = (labels[(size_t)i] + 1) % cc[0];

    rvseg::RandomForestPrune pruner;
    CHECK(pruner.params.start_temperature == 100.f && pruner.params.end_temperature == 1e-5f && pruner.params.alpha == 0.95f &&
          pruner.params.inner_loops == 250 && pruner.params.p_exchange == 1.f && pruner.params.p_remove == 0.f && pruner.params.p_add == 0.f &&
          pruner.params.energy == RVSEG_PRUNE_ERROR);
    int32_t iterations = 0, steps = 0;
    CHECK(rvseg_prune_schedule(&pruner.params, &iterations, &steps) == RVSEG_OK && iterations == 315 && steps == 78750);
    pruner.params.start_temperature = 1.f;
    pruner.params.end_temperature = 0.05f;
    pruner.params.alpha = 0.7f;
    pruner.params.inner_loops = 10;
    pruner.params.p_remove = 0.5f;
    pruner.params.p_add = 0.5f;
    pruner.params.seed = 4;
    CHECK(rvseg_prune_schedule(&pruner.params, &iterations, &steps) == RVSEG_OK && iterations == 9 && steps == 90);

    float best = -1.f, energy = -2.f, first = -3.f;
    const std::vector<int32_t> start = {0, 1};
    const std::vector<int32_t> state = pruner.optimize(ctx, X.data(), P, D, labels.data(), 0, start, &best);
    CHECK(!state.empty() && (int)pruner.trace.size() == iterations);
    CHECK(rvseg_forest_prune_energy(ctx, X.data(), P, D, labels.data(), 0, RVSEG_PRUNE_ERROR, state.data(), (int32_t)state.size(), &energy) == RVSEG_OK);
    CHECK(rvseg_forest_prune_energy(ctx, X.data(), P, D, labels.data(), 0, RVSEG_PRUNE_ERROR, start.data(), 2, &first) == RVSEG_OK);
    CHECK(energy == best && best <= first && best > 0.f && best < 1.f);
    for (size_t i = 0; i < pruner.trace.size(); i++) {
        const rvseg_prune_trace_row& r = pruner.trace[i];
        CHECK(r.iteration == (int)i + 1 && r.best_energy <= r.energy && r.best_energy >= best && r.state_size >= 1 && r.state_size <= RVSEG_PRUNE_MAX_STATE);
        CHECK(i == 0 || (r.temperature < pruner.trace[i - 1].temperature && r.best_energy <= pruner.trace[i - 1].best_energy));
    }
    CHECK(pruner.trace.back().best_energy == best);
    pruner.print();
    const std::vector<rvseg_prune_trace_row> kept = pruner.trace;
    const std::vector<int32_t> again = pruner.prune(ctx, X.data(), P, D, labels.data(), 0, start);
    CHECK(again == state && kept.size() == pruner.trace.size());
    for (size_t i = 0; i < kept.size(); i++) CHECK(kept[i].energy == pruner.trace[i].energy && kept[i].state_size == pruner.trace[i].state_size);
    CHECK(rvseg_forest_info(ctx, &T, nullptr, nullptr, nullptr, nullptr) == RVSEG_OK && T == (int32_t)state.size());

    // a refused schedule throws with the library's reason and keeps the model
    pruner.params.alpha = 1.f;
    bool thrown = false;
    try { pruner.prune(ctx, X.data(), P, D, labels.data()); } catch (const std::runtime_error& e) { thrown = std::string(e.what()).find("alpha") != std::string::npos; }
    CHECK(thrown);
    int32_t after = 0;
    CHECK(rvseg_forest_info(ctx, &after, nullptr, nullptr, nullptr, nullptr) == RVSEG_OK && after == T);

    rvseg_destroy(ctx);
    std::printf("prune ok\n");
    return 0;
}
