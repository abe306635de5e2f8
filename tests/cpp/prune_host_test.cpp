// The forest pruner's host rules (csrc/prune_host.h) alone, built with the host compiler and its sanitizers: the
// schedule's step count, the refusals, the move rules, and a full chain with both energies on the vote matrix below.
// The trajectories are printed with their floats as bits; tests/test_prune_host_cpp_cpu.py runs the Python restatement
// (tests/prune_restate.py) on the same votes and compares every line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "prune_host.h"

using namespace rvseg;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

namespace {

constexpr int T = 5, P = 12, C = 3;
const uint8_t kVotes[T][P] = {{0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2},
                              {0, 0, 1, 1, 2, 2, 0, 0, 1, 1, 2, 2},
                              {2, 1, 0, 2, 1, 0, 1, 1, 1, 0, 0, 2},
                              {1, 1, 1, 0, 2, 2, 0, 2, 2, 1, 1, 0},
                              {0, 2, 2, 1, 1, 2, 0, 1, 0, 0, 2, 2}};
const int32_t kLabels[P] = {0, 1, 2, 1, 1, 2, 0, 3, -1, 0, 2, 2};   // 3 and -1: outside [0, C)

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

rvseg_prune_params params(float start, float end, float alpha, int inner, float pe, float pr, float pa, int energy, uint64_t seed) {
    rvseg_prune_params p;
    std::memset(&p, 0, sizeof(p));
    p.start_temperature = start; p.end_temperature = end; p.alpha = alpha; p.inner_loops = inner;
    p.p_exchange = pe; p.p_remove = pr; p.p_add = pa; p.energy = energy; p.seed = seed;
    return p;
}

void dump(const char* name, const rvseg_prune_params& p, const std::vector<int32_t>& initial, const PruneRun& run) {
    std::printf("run %s energy %d seed %llu start %08x end %08x alpha %08x inner %d moves %08x %08x %08x\n", name, p.energy, (unsigned long long)p.seed,
                bits(p.start_temperature), bits(p.end_temperature), bits(p.alpha), p.inner_loops, bits(p.p_exchange), bits(p.p_remove), bits(p.p_add));
    std::printf("initial");
    for (int32_t t : initial) std::printf(" %d", t);
    std::printf("\nkinds");
    for (uint8_t k : run.step_kind) std::printf(" %d", (int)k);
    std::printf("\n");
    for (const rvseg_prune_trace_row& r : run.trace)
        std::printf("trace %d %08x %08x %08x %d\n", r.iteration, bits(r.temperature), bits(r.energy), bits(r.best_energy), r.state_size);
    std::printf("best %08x", bits(run.best_energy));
    for (int32_t t : run.best) std::printf(" %d", t);
    std::printf("\n");
}

}  // namespace

int main() {
    // ---- the schedule's step count: the fp32 loop itself ----------------------------------------------------------------
    rvseg_prune_params def = params(100.f, 1e-5f, 0.95f, 250, 1.f, 0.f, 0.f, RVSEG_PRUNE_ERROR, 0);
    CHECK(prune_iterations(def) == 315 && prune_params_refusal(def) == nullptr);
    CHECK(prune_steps(def, T).size() == 315u * 250u);
    CHECK(prune_iterations(params(1.f, 0.5f, 0.8f, 8, 1, 0, 0, 0, 0)) == 4);
    CHECK(prune_iterations(params(0.5f, 0.5f, 0.8f, 8, 1, 0, 0, 0, 0)) == 0 && prune_iterations(params(0.25f, 0.5f, 0.8f, 8, 1, 0, 0, 0, 0)) == 0);
    CHECK(prune_iterations(params(std::nanf(""), 0.5f, 0.8f, 8, 1, 0, 0, 0, 0)) == 0);

    // ---- the refusals -----------------------------------------------------------------------------------------------------
    const float inf = std::numeric_limits<float>::infinity();
    for (float alpha : {0.f, 1.f, -0.5f, 1.5f, std::nanf("")}) CHECK(prune_params_refusal(params(1.f, 0.5f, alpha, 8, 1, 0, 0, 0, 0)) != nullptr);
    CHECK(prune_params_refusal(params(1.f, 0.5f, 0.8f, 0, 1, 0, 0, 0, 0)) != nullptr);
    CHECK(prune_params_refusal(params(1.f, 0.5f, 0.8f, 8, 0, 0, 0, 0, 0)) != nullptr);            // all zero
    CHECK(prune_params_refusal(params(1.f, 0.5f, 0.8f, 8, 1, -0.25f, 0, 0, 0)) != nullptr);       // negative
    CHECK(prune_params_refusal(params(1.f, 0.5f, 0.8f, 8, 1, std::nanf(""), 0, 0, 0)) != nullptr);
    CHECK(prune_params_refusal(params(1.f, 0.5f, 0.8f, 8, 1, 0, 0, 2, 0)) != nullptr);            // unknown energy
    CHECK(prune_params_refusal(params(100.f, 1e-5f, 0.95f, PRUNE_MAX_STEPS / 315 + 1, 1, 0, 0, 0, 0)) != nullptr);   // 2^22 + a few steps
    CHECK(prune_params_refusal(params(100.f, 1e-5f, 0.95f, PRUNE_MAX_STEPS / 315, 1, 0, 0, 0, 0)) == nullptr);
    CHECK(prune_params_refusal(params(inf, 0.5f, 0.8f, 1, 1, 0, 0, 0, 0)) != nullptr);            // never cools
    CHECK(prune_params_refusal(params(1.f, -1.f, 0.8f, 1, 1, 0, 0, 0, 0)) != nullptr);            // never gets below the end
    CHECK(prune_params_refusal(params(1.f, 0.5f, 0.99999994f, 1, 1, 0, 0, 0, 0)) != nullptr);     // 2^22 steps of 2^-24 each do not halve it
    const int32_t ok_state[3] = {0, 4, 4}, low[1] = {-1}, high[2] = {0, T};
    std::vector<int32_t> longest(65, 1);
    CHECK(prune_state_refusal(ok_state, 3, T) == nullptr && prune_state_refusal(longest.data(), 64, T) == nullptr);
    CHECK(prune_state_refusal(ok_state, 0, T) && prune_state_refusal(nullptr, 1, T) && prune_state_refusal(low, 1, T) && prune_state_refusal(high, 2, T));
    CHECK(prune_state_refusal(longest.data(), 65, T) != nullptr);

    // ---- choosing and making moves ----------------------------------------------------------------------------------------
    PruneMoves m;
    CHECK(prune_moves(params(1, 0.5f, 0.8f, 8, 0.5f, 0.f, 0.25f, 0, 0), m) && m.n == 2 && m.kind[0] == PRUNE_EXCHANGE && m.kind[1] == PRUNE_ADD);
    CHECK(prune_choose_move(m, 0.f) == PRUNE_EXCHANGE && prune_choose_move(m, 0.49f) == PRUNE_EXCHANGE && prune_choose_move(m, 0.5f) == PRUNE_ADD);
    CHECK(prune_choose_move(m, 0.74f) == PRUNE_ADD && prune_choose_move(m, 0.75f) == PRUNE_ADD && prune_choose_move(m, 0.99f) == PRUNE_ADD);   // the fallback
    int32_t out[RVSEG_PRUNE_MAX_STATE];
    const std::vector<int32_t> three = {4, 0, 3}, one = {2};
    CHECK(prune_propose(PRUNE_EXCHANGE, 1, 7ull, three, 3, out) == 3 && out[0] == 4 && out[1] == 1 && out[2] == 3);
    CHECK(prune_propose(PRUNE_EXCHANGE, 4, 0ull, three, 3, out) == 3 && out[0] == 4 && out[1] == 0 && out[2] == 3);       // a duplicate is kept
    CHECK(prune_propose(PRUNE_REMOVE, 1, 0xffffffffffffffffull, three, 3, out) == 2 && out[0] == 0 && out[1] == 3);        // 2^64 - 1 = 0 mod 3
    CHECK(prune_propose(PRUNE_REMOVE, 1, 5ull, one, 1, out) == 1 && out[0] == 2);                                         // the floor
    CHECK(prune_propose(PRUNE_ADD, 1, 5ull, three, 3, out) == 4 && out[3] == 1 && out[2] == 3);
    std::vector<int32_t> full(64, 3), almost(63, 3);
    CHECK(prune_propose(PRUNE_ADD, 1, 5ull, almost, 63, out) == 64 && out[63] == 1 && out[62] == 3);
    CHECK(prune_propose(PRUNE_ADD, 1, 5ull, full, 64, out) == 64 && out[63] == 3);                                        // the cap
    CHECK(prune_uniform(0xffffffffffffffffull) < 1.f && prune_uniform(0ull) == 0.f && prune_uniform(1ull << 63) == 0.5f);
    CHECK(std::log(prune_uniform(0ull)) == -inf && prune_accept_host(0.5f, 0.25f, -inf, 1.f) == 2);

    // ---- the energies on the matrix above -----------------------------------------------------------------------------------
    const int32_t s012[3] = {0, 1, 2}, s31[2] = {3, 1};
    // state {0, 1, 2}: point 2 votes 2, 1, 0 -> every count 1, the first vote keeps the maximum: label 2
    CHECK(prune_error_count(&kVotes[0][0], P, P, kLabels, C, s012, 3) == 4);   // points 3, 7, 8 and 10
    CHECK(prune_error_energy(4, P) == 4.f / 12.f && prune_error_energy(1ull << 30, 1 << 24) == 1.f);
    std::vector<uint64_t> agree((size_t)T * T);
    for (int a = 0; a < T; a++)
        for (int b = 0; b < T; b++)
            for (int n = 0; n < P; n++) agree[(size_t)a * T + b] += kVotes[a][n] == kVotes[b][n];
    uint64_t want = 0;
    for (int j = 0; j < T; j++) want += std::min(P - agree[3 * T + j], P - agree[1 * T + j]);
    CHECK(prune_cover_energy(agree.data(), T, P, s31, 2) == (float)want / 2.f && want > 0);

    // ---- full chains ------------------------------------------------------------------------------------------------------------
    auto error = [&](const int32_t* state, int n) { return prune_error_energy(prune_error_count(&kVotes[0][0], P, P, kLabels, C, state, n), P); };
    auto cover = [&](const int32_t* state, int n) { return prune_cover_energy(agree.data(), T, P, state, n); };
    const std::vector<int32_t> first = {0, 1};
    const rvseg_prune_params pe = params(1.f, 0.1f, 0.7f, 16, 0.5f, 0.25f, 0.25f, RVSEG_PRUNE_ERROR, 11);
    const PruneRun re = prune_chain(pe, T, first.data(), 2, error);
    CHECK(re.step_kind.size() == (size_t)prune_iterations(pe) * 16 && re.trace.size() == (size_t)prune_iterations(pe));
    CHECK(re.best_energy <= error(first.data(), 2) && re.best_energy == error(re.best.data(), (int)re.best.size()));
    CHECK(re.trace.back().best_energy == re.best_energy && re.trace.front().iteration == 1);
    dump("error", pe, first, re);
    const rvseg_prune_params pc = params(2.f, 0.2f, 0.6f, 12, 0.25f, 0.25f, 0.5f, RVSEG_PRUNE_COVER, 5);
    const PruneRun rc = prune_chain(pc, T, first.data(), 2, cover);
    CHECK(rc.best_energy <= cover(first.data(), 2) && rc.best_energy == cover(rc.best.data(), (int)rc.best.size()));
    dump("cover", pc, first, rc);
    const rvseg_prune_params pz = params(0.5f, 0.5f, 0.8f, 8, 1, 0, 0, RVSEG_PRUNE_ERROR, 1);
    const PruneRun rz = prune_chain(pz, T, first.data(), 2, error);
    CHECK(rz.step_kind.empty() && rz.trace.empty() && rz.best == first && rz.best_energy == error(first.data(), 2));
    dump("none", pz, first, rz);

    std::printf("votes");
    for (int t = 0; t < T; t++)
        for (int n = 0; n < P; n++) std::printf(" %d", (int)kVotes[t][n]);
    std::printf("\nlabels");
    for (int n = 0; n < P; n++) std::printf(" %d", kLabels[n]);
    std::printf("\nprune host ok\n");
    return 0;
}
