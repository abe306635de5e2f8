// The host chain of csrc/prune_host.h alone on one core, for the one CPU figure of DESIGN.md's pruning section: the
// reference's 315 temperatures with 25 proposals each (a tenth of its 78 750 steps) and the error energy, on the votes and
// labels that profiles/scripts/prune_time.py --dump wrote.
//   g++ -O3 -std=c++17 -ffp-contract=off -I rovinasemanticsegmentation_amd/csrc profiles/analysis/prune_host_time.cpp -o prune_host_time
//   ./prune_host_time votes.u8 labels.i32 16 8
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "prune_host.h"

int main(int argc, char** argv) {
    if (argc != 5) { std::printf("usage: %s votes.u8 labels.i32 T C\n", argv[0]); return 2; }
    std::ifstream fv(argv[1], std::ios::binary), fl(argv[2], std::ios::binary);
    const std::vector<char> votes((std::istreambuf_iterator<char>(fv)), std::istreambuf_iterator<char>());
    const std::vector<char> lab((std::istreambuf_iterator<char>(fl)), std::istreambuf_iterator<char>());
    const int T = std::atoi(argv[3]), C = std::atoi(argv[4]), P = (int)(lab.size() / 4);
    if (P < 1 || votes.size() != (size_t)T * P) { std::printf("sizes do not match\n"); return 2; }
    const uint8_t* v = reinterpret_cast<const uint8_t*>(votes.data());
    const int32_t* labels = reinterpret_cast<const int32_t*>(lab.data());
    rvseg_prune_params p;
    p.start_temperature = 100.f; p.end_temperature = 1e-5f; p.alpha = 0.95f; p.inner_loops = 25;
    p.p_exchange = 1.f; p.p_remove = 0.f; p.p_add = 0.f; p.energy = RVSEG_PRUNE_ERROR; p.seed = 1;
    std::vector<int32_t> state;
    for (int i = 0; i < 15 && i < T; i++) state.push_back(i);
    const auto t0 = std::chrono::steady_clock::now();
    const rvseg::PruneRun run = rvseg::prune_chain(p, T, state.data(), (int)state.size(), [&](const int32_t* s, int n) {
        return rvseg::prune_error_energy(rvseg::prune_error_count(v, (size_t)P, P, labels, C, s, n), P);
    });
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("{\"points\": %d, \"steps\": %zu, \"seconds\": %.3f, \"ms_per_step\": %.3f, \"best_energy\": %.9g}\n", P, run.step_kind.size(), dt,
                1e3 * dt / (double)run.step_kind.size(), (double)run.best_energy);
    return 0;
}
