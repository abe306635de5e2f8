// The forest pruner's host-side rules (rvseg_prune.hip), free of HIP so that the host compiler and its sanitizers can run
// them alone (tests/cpp/prune_host_test.cpp).  Everything order-sensitive that the device chain (kernels_prune.hip) and
// the host chain share is stated here once: the schedule, the draws, the moves, the acceptance test and the two energies.
// Line references are to the reference's third-party/libforest/src/mcmc.h and todos.txt.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "train_host.h"

namespace rvseg {

constexpr int PRUNE_MAX_STEPS = 1 << 22;   // proposals per call: the step records are filled ahead of the chain
constexpr int PRUNE_CMAX = 16;             // classes of the error energy: 16 byte counters in four registers
enum PruneMove : uint32_t { PRUNE_EXCHANGE = 0, PRUNE_REMOVE = 1, PRUNE_ADD = 2 };

// ---- the draws: the reference seeds std::mt19937 from std::random_device (mcmc.h:152, todos.txt:53,105,136); here every
// draw is a pure function of (seed, step, slot), so nothing depends on how steps are batched ---------------------------
enum PruneSlot { SLOT_MOVE = 0, SLOT_TREE = 1, SLOT_POSITION = 2, SLOT_ACCEPT = 3 };
RV_TRAIN_HD inline uint64_t prune_key(uint64_t seed) { return mix64(seed ^ mix64(0x7072756Eull)); }
RV_TRAIN_HD inline uint64_t prune_draw(uint64_t key, uint64_t step, int slot) { return draw64(key, 4ull * step + (uint64_t)slot); }
RV_TRAIN_HD inline float prune_uniform(uint64_t d) { return (float)(d >> 40) * 5.9604644775390625e-8f; }   // 24 bits, in [0, 1)

// ---- the argument rules of rvseg_forest_prune ---------------------------------------------------------------------------
// SimulatedAnnealing::addMove in the order exchange, remove, add (todos.txt:324-325 registers the first alone); a move
// of probability 0 is not registered, so the fallback of mcmc.h:194-198 is the last move that can be drawn at all
struct PruneMoves {
    int n = 0;
    uint32_t kind[3] = {};
    float prob[3] = {};
};
inline bool prune_moves(const rvseg_prune_params& p, PruneMoves& m) {
    const float prob[3] = {p.p_exchange, p.p_remove, p.p_add};
    m = PruneMoves();
    for (int k = 0; k < 3; k++) {
        if (!(prob[k] >= 0.f)) return false;
        if (prob[k] > 0.f) { m.kind[m.n] = (uint32_t)k; m.prob[m.n] = prob[k]; m.n++; }
    }
    return m.n > 0;
}

// the temperature iterations of `while (temperature > end) { iteration++; temperature = temperature * alpha; ... }`
// (mcmc.h:170-173, :312-315), counted by running the fp32 loop; -1 once iterations x inner_loops passes PRUNE_MAX_STEPS
// (a schedule that never ends -- an infinite start, an alpha that rounds the product back -- stops there too)
inline int prune_iterations(const rvseg_prune_params& p) {
    float temperature = p.start_temperature;
    long iterations = 0;
    while (temperature > p.end_temperature) {
        iterations++;
        if (iterations * (long)p.inner_loops > (long)PRUNE_MAX_STEPS) return -1;
        temperature = temperature * p.alpha;
    }
    return (int)iterations;
}

inline const char* prune_params_refusal(const rvseg_prune_params& p) {
    PruneMoves m;
    if (!(p.alpha > 0.f && p.alpha < 1.f)) return "alpha outside (0, 1)";
    if (p.inner_loops < 1) return "inner_loops < 1";
    if (p.inner_loops > PRUNE_MAX_STEPS) return "a schedule of more than 2^22 proposals";
    if (!prune_moves(p, m)) return "a negative or all-zero move probability";
    if (p.energy != RVSEG_PRUNE_ERROR && p.energy != RVSEG_PRUNE_COVER) return "unknown energy";
    if (prune_iterations(p) < 0) return "a schedule of more than 2^22 proposals";
    return nullptr;
}
inline const char* prune_state_refusal(const int32_t* state, int n_state, int T, int cap = RVSEG_PRUNE_MAX_STATE) {
    if (!state || n_state < 1) return "empty state";
    if (n_state > cap) return "state longer than 64 entries";
    for (int i = 0; i < n_state; i++)
        if (state[i] < 0 || state[i] >= T) return "tree index outside [0, T)";
    return nullptr;
}

// ---- choosing and making a move -----------------------------------------------------------------------------------------
// the probSum scan of mcmc.h:178-198 on fp32
inline uint32_t prune_choose_move(const PruneMoves& m, float u) {
    float probSum = 0;
    for (int i = 0; i < m.n; i++) {
        if (probSum <= u && u < probSum + m.prob[i]) return m.kind[i];
        probSum += m.prob[i];
    }
    return m.kind[m.n - 1];
}

// The proposal from `state` (n entries), integer arithmetic only; `out` holds RVSEG_PRUNE_MAX_STATE entries.  Returns
// the proposal's length.  add_tree = d_1 % T, pos_draw = d_2.
//   exchange  todos.txt:141-155  newState[replaceTree] = addTree (duplicates are not avoided)
//   remove    todos.txt:58-87    a state of one tree is copied
//   add       todos.txt:110-118  a state already at RVSEG_PRUNE_MAX_STATE is copied: this build's own rule (the
//                                reference's vector grows without bound; the device keeps 64 votes in a byte counter)
template <class State>
RV_TRAIN_HD inline int prune_propose(uint32_t move, int add_tree, uint64_t pos_draw, const State& state, int n, int32_t* out) {
    if (move == PRUNE_REMOVE && n >= 2) {
        const int removeTree = (int)(pos_draw % (uint64_t)n);
        for (int i = 0, k = 0; i < n; i++)
            if (i != removeTree) out[k++] = state[i];
        return n - 1;
    }
    for (int i = 0; i < n; i++) out[i] = state[i];
    if (move == PRUNE_EXCHANGE) out[(int)(pos_draw % (uint64_t)n)] = add_tree;
    if (move == PRUNE_ADD && n < RVSEG_PRUNE_MAX_STATE) { out[n] = add_tree; return n + 1; }
    return n;
}

// What a step needs that does not depend on the state, filled ahead of the chain: the move, the tree to add, the raw
// position draw (its modulus is the state's length), the temperature of the step's iteration, logf of the acceptance
// uniform (libm's; never evaluated on the device) and, for the last step of an iteration, the iteration (else 0).
struct PruneStep {
    uint32_t move;
    int32_t add_tree;
    uint64_t pos_draw;
    float temperature;
    float log_u;
    int32_t trace_iteration;
    int32_t pad;
};
static_assert(sizeof(PruneStep) == 32, "PruneStep is read by the device as two 16-byte words");

inline std::vector<PruneStep> prune_steps(const rvseg_prune_params& p, int T) {
    PruneMoves moves;
    prune_moves(p, moves);
    const int iterations = prune_iterations(p);
    const uint64_t key = prune_key(p.seed);
    std::vector<PruneStep> steps((size_t)iterations * (size_t)p.inner_loops);
    float temperature = p.start_temperature;
    size_t s = 0;
    for (int iteration = 1; iteration <= iterations; iteration++) {
        temperature = temperature * p.alpha;
        for (int inner = 0; inner < p.inner_loops; inner++, s++) {
            PruneStep& st = steps[s];
            st.move = prune_choose_move(moves, prune_uniform(prune_draw(key, s, SLOT_MOVE)));
            st.add_tree = (int32_t)(prune_draw(key, s, SLOT_TREE) % (uint64_t)T);
            st.pos_draw = prune_draw(key, s, SLOT_POSITION);
            st.temperature = temperature;
            st.log_u = std::log(prune_uniform(prune_draw(key, s, SLOT_ACCEPT)));   // float overload: logf; logf(0) = -inf accepts
            st.trace_iteration = inner == p.inner_loops - 1 ? iteration : 0;
            st.pad = 0;
        }
    }
    return steps;
}

// mcmc.h:205-225: 0 rejected, 1 accepted with improvement <= 0, 2 accepted uphill.  The divide is fp32, correctly
// rounded, on both sides (kernels_prune.hip uses __fdiv_rn).
inline int prune_accept_host(float newE, float curE, float log_u, float temperature) {
    const float improvement = newE - curE;
    if (improvement <= 0) return 1;
    return log_u <= -improvement / temperature ? 2 : 0;
}

// ---- the two energies ---------------------------------------------------------------------------------------------------
// PruneEnergy::energy (todos.txt:186-226) on votes[t * stride + n]: the integer error count of a state
inline uint64_t prune_error_count(const uint8_t* votes, size_t stride, int P, const int32_t* labels, int C, const int32_t* state, int n) {
    uint64_t errors = 0;
    int count[256];   // (a vote is a label of the layer: below C)
    for (int p = 0; p < P; p++) {
        std::fill(count, count + C, 0);
        int maxLabel = 0, maxVotes = 0;
        for (int j = 0; j < n; j++) {
            const int vote = votes[(size_t)state[j] * stride + (size_t)p];
            count[vote]++;
            if (count[vote] > maxVotes) { maxVotes = count[vote]; maxLabel = vote; }
        }
        const int label = labels[p];
        if (label < 0 || label >= C || maxLabel != label) errors++;
    }
    return errors;
}
// `error += 1` on a float stops at 2^24 (:220); error / storage->getSize() (:225)
inline float prune_error_energy(uint64_t errors, int P) {
    return (float)std::min<uint64_t>(errors, 16777216ull) / (float)P;
}
// the second PruneEnergy (todos.txt:281-297) on dist[i][j] = P - agree[i][j]; res is an int there, 64 bits here
inline float prune_cover_energy(const uint64_t* agree, int T, uint64_t P, const int32_t* state, int n) {
    uint64_t res = 0;
    for (int j = 0; j < T; j++) {
        uint64_t min = P - agree[(size_t)state[0] * T + j];
        for (int i = 0; i < n; i++) min = std::min(min, P - agree[(size_t)state[i] * T + j]);
        res += min;
    }
    return (float)res / (float)n;
}

// ---- the chain (mcmc.h:147-240) on the host, for any energy: what kernels_prune.hip runs one launch per step ----------
struct PruneRun {
    std::vector<int32_t> best;                      // the result: `state = bestState` (:239)
    float best_energy = 0.f;
    std::vector<rvseg_prune_trace_row> trace;       // one row per iteration (:234-237)
    std::vector<uint8_t> step_kind;
};
template <class Energy>   // float energy(const int32_t* state, int n)
inline PruneRun prune_chain(const rvseg_prune_params& p, int T, const int32_t* initial, int n_initial, Energy energy) {
    const std::vector<PruneStep> steps = prune_steps(p, T);
    std::vector<int32_t> state(initial, initial + n_initial), proposal((size_t)RVSEG_PRUNE_MAX_STATE);
    float currentEnergy = energy(state.data(), (int)state.size());
    PruneRun run;
    run.best = state;
    run.best_energy = currentEnergy;
    run.step_kind.reserve(steps.size());
    for (const PruneStep& st : steps) {
        const int n_new = prune_propose(st.move, st.add_tree, st.pos_draw, state, (int)state.size(), proposal.data());
        const float newError = energy(proposal.data(), n_new);
        const int kind = prune_accept_host(newError, currentEnergy, st.log_u, st.temperature);
        if (kind) {
            currentEnergy = newError;
            state.assign(proposal.begin(), proposal.begin() + n_new);
        }
        if (currentEnergy < run.best_energy) {
            run.best_energy = currentEnergy;
            run.best = state;
        }
        run.step_kind.push_back((uint8_t)kind);
        if (st.trace_iteration) run.trace.push_back({st.trace_iteration, st.temperature, currentEnergy, run.best_energy, (int32_t)state.size()});
    }
    return run;
}

}  // namespace rvseg
