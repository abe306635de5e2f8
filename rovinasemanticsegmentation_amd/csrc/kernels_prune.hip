// Forest pruning kernels for gfx950 (rvseg_prune.hip): one proposal of the simulated-annealing chain per launch, the
// launches issued back to back on one stream.  The rules are those of prune_host.h; line references are to the
// reference's third-party/libforest/src/mcmc.h and todos.txt.
//
// A launch of step s:
//   every block  reads the current state (PruneControl::state[s & 1], written by the launch before), forms the proposal
//                in LDS with prune_propose (integers only), walks its points through the proposal's trees -- votes[t][n]
//                bytes, four points of a lane per 32-bit load, coalesced across the lanes -- counts the points whose
//                majority label (todos.txt:200-221) differs from theirs and adds the count to PruneControl::errors;
//   the block that takes the last ticket (atomic ticket behind __threadfence(); no block waits for another) forms the
//                energy with correctly rounded fp32 divides, applies the acceptance test of mcmc.h:205-225 with the
//                step's temperature and logf(u) as the host filled them in, writes the next state to state[(s + 1) & 1],
//                the current and best energy, the best state, the step's kind and, at the end of a temperature, the
//                trace row, and takes the counter and the ticket back to zero for the next launch.
// The two state buffers alternate, so no block reads what another writes in the same launch; what a launch wrote reaches
// the next one through the kernel boundary.
//
// The walk keeps a point's (at most 16) class counters of (at most 64) votes as bytes in four registers and updates
// them with selects: a dynamically indexed array would live in scratch.
#include "device_math.h"
#include "forest_tools_host.h"
#include "prune_host.h"
#include "rvseg_internal.h"
#include "rvseg_kernels.h"

namespace rvseg {

constexpr int PRUNE_BLOCK = 256;
constexpr int PRUNE_POINTS_PER_LANE = 4;   // one 32-bit load of a vote row

// todos.txt:204-214 for one vote of one point: votes[vote]++, and the label follows the first count above the maximum
__device__ __forceinline__ void cast_vote(uint32_t vote, uint32_t (&cnt)[4], uint32_t& maxVotes, uint32_t& maxLabel) {
    const uint32_t word = vote >> 2, shift = (vote & 3u) * 8u, one = 1u << shift;
    cnt[0] += word == 0u ? one : 0u;
    cnt[1] += word == 1u ? one : 0u;
    cnt[2] += word == 2u ? one : 0u;
    cnt[3] += word == 3u ? one : 0u;
    const uint32_t sel = word == 0u ? cnt[0] : (word == 1u ? cnt[1] : (word == 2u ? cnt[2] : cnt[3]));
    const uint32_t mine = (sel >> shift) & 255u;
    if (mine > maxVotes) { maxVotes = mine; maxLabel = vote; }
}

// votes: [T][stride] bytes, labels: [stride] (stride a multiple of 4, the tail beyond P zero).  INIT: no step -- the
// "proposal" is state[0] itself and the deciding block makes it the current and the best state (mcmc.h:162-166).
template <bool INIT>
__global__ void __launch_bounds__(PRUNE_BLOCK)
prune_step_kernel(const uint8_t* __restrict__ votes, const int32_t* __restrict__ labels, int P, size_t stride,
                  const PruneStep* __restrict__ steps, int s, PruneControl* __restrict__ ctl,
                  uint8_t* __restrict__ step_kind, rvseg_prune_trace_row* __restrict__ trace) {
    __shared__ int32_t proposal[RVSEG_PRUNE_MAX_STATE];
    __shared__ int n_proposal;
    __shared__ unsigned wave_errors[PRUNE_BLOCK / 64];
    __shared__ int decision;   // -1: another block decides; else the step's kind
    __shared__ int better;
    const int tid = (int)threadIdx.x;
    const int cur = INIT ? 0 : (s & 1);
    const int32_t* state = ctl->state[cur];
    const int n_state = ctl->n_state[cur];
    PruneStep st = {};
    if (!INIT) st = steps[s];
    if (tid == 0) n_proposal = INIT ? prune_propose(PRUNE_ADD + 1u, 0, 0ull, state, n_state, proposal)   // (no move: a copy)
                                    : prune_propose(st.move, st.add_tree, st.pos_draw, state, n_state, proposal);
    __syncthreads();
    const int n = n_proposal;

    unsigned errors = 0;
    for (long first = ((long)blockIdx.x * PRUNE_BLOCK + tid) * PRUNE_POINTS_PER_LANE; first < P;
         first += (long)gridDim.x * PRUNE_BLOCK * PRUNE_POINTS_PER_LANE) {
        uint32_t cnt[PRUNE_POINTS_PER_LANE][4] = {};
        uint32_t maxVotes[PRUNE_POINTS_PER_LANE] = {}, maxLabel[PRUNE_POINTS_PER_LANE] = {};
        for (int j = 0; j < n; j++) {
            const uint32_t four = *reinterpret_cast<const uint32_t*>(votes + (size_t)proposal[j] * stride + (size_t)first);
#pragma unroll
            for (int k = 0; k < PRUNE_POINTS_PER_LANE; k++) cast_vote((four >> (8 * k)) & 255u, cnt[k], maxVotes[k], maxLabel[k]);
        }
        const int4 lab = *reinterpret_cast<const int4*>(labels + first);
        const int label[PRUNE_POINTS_PER_LANE] = {lab.x, lab.y, lab.z, lab.w};
#pragma unroll
        for (int k = 0; k < PRUNE_POINTS_PER_LANE; k++)   // a label outside [0, C) equals no vote: always an error
            errors += (first + k < P && (int)maxLabel[k] != label[k]) ? 1u : 0u;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) errors += __shfl_xor(errors, m, 64);
    if ((tid & 63) == 0) wave_errors[tid >> 6] = errors;
    __syncthreads();

    if (tid == 0) {
        unsigned block_errors = 0;
        for (int w = 0; w < PRUNE_BLOCK / 64; w++) block_errors += wave_errors[w];
        if (block_errors) atomicAdd(&ctl->errors, block_errors);
        __threadfence();
        const unsigned ticket = atomicAdd(&ctl->ticket, 1u);
        int kind = -1;
        if (ticket == gridDim.x - 1) {
            __threadfence();
            const unsigned total = atomicExch(&ctl->errors, 0u);   // every block's add is before its ticket
            atomicExch(&ctl->ticket, 0u);
            const float newE = __fdiv_rn((float)min(total, 16777216u), (float)P);   // prune_error_energy
            float curE = ctl->cur_energy;
            if (INIT) {
                kind = 1;
                curE = newE;
                ctl->best_energy = newE;
                better = 1;
            } else {
                const float improvement = newE - curE;
                kind = improvement <= 0 ? 1 : (st.log_u <= __fdiv_rn(-improvement, st.temperature) ? 2 : 0);   // prune_accept_host
                if (kind) curE = newE;
                const float bestE = ctl->best_energy;
                better = curE < bestE ? 1 : 0;
                if (better) ctl->best_energy = curE;
                step_kind[s] = (uint8_t)kind;
                if (st.trace_iteration) {
                    rvseg_prune_trace_row row;
                    row.iteration = st.trace_iteration;
                    row.temperature = st.temperature;
                    row.energy = curE;
                    row.best_energy = better ? curE : bestE;
                    row.state_size = kind ? n : n_state;
                    trace[st.trace_iteration - 1] = row;
                }
            }
            ctl->cur_energy = curE;
        }
        decision = kind;
    }
    __syncthreads();
    if (decision < 0) return;
    const int nxt = INIT ? 0 : (cur ^ 1);
    const int n_next = decision ? n : n_state;
    if (tid < n_next) {
        const int32_t tree = decision ? proposal[tid] : state[tid];
        if (!INIT) ctl->state[nxt][tid] = tree;
        if (better) ctl->best[tid] = tree;
    }
    if (tid == 0) {
        ctl->n_state[nxt] = n_next;
        if (better) ctl->n_best = n_next;
    }
}

int prune_grid(int P, int max_blocks) {
    const long want = ((long)P + PRUNE_BLOCK * PRUNE_POINTS_PER_LANE - 1) / (PRUNE_BLOCK * PRUNE_POINTS_PER_LANE);
    return looping_grid(want, max_blocks);
}

void launch_prune_init(const uint8_t* d_votes, const int32_t* d_labels, int P, size_t stride, int grid, PruneControl* d_ctl, hipStream_t s) {
    prune_step_kernel<true><<<dim3((unsigned)grid), dim3(PRUNE_BLOCK), 0, s>>>(d_votes, d_labels, P, stride, nullptr, 0, d_ctl, nullptr, nullptr);
    RV_LAUNCHED("prune_step_kernel<init>");
}

void launch_prune_steps(const uint8_t* d_votes, const int32_t* d_labels, int P, size_t stride, int grid, const PruneStep* d_steps,
                        int first_step, int n_steps, PruneControl* d_ctl, uint8_t* d_step_kind, rvseg_prune_trace_row* d_trace, hipStream_t s) {
    for (int k = first_step; k < first_step + n_steps; k++)
        prune_step_kernel<false><<<dim3((unsigned)grid), dim3(PRUNE_BLOCK), 0, s>>>(d_votes, d_labels, P, stride, d_steps, k, d_ctl, d_step_kind, d_trace);
    RV_LAUNCHED("prune_step_kernel");
}

}  // namespace rvseg
