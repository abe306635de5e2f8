// Host-only restatement of one wave of csr_scatter_kernel (csrc/kernels_lattice.hip): a wave-block of points, DP1 vertex
// ids per point, walked in chunks of 64 "lanes" with ballots as 64-bit masks and the kernel's leader order.  Two ways of
// emitting the entries of a chunk are compared:
//   old   per distinct vertex: read its counter, store the entries at counter + rank, leader writes counter + total
//   new   all ranks and totals first (no counter touched), then per lane its DP1 counter reads, its DP1 stores, and the
//         leaders' additions
// Both must write the same (point, slot) to the same positions and leave the same counters -- over random id rows, rows
// of one simplex per chunk, rows with nearly all vertices distinct, rows in which a vertex sits in different slots of
// different lanes, rows with the same id twice in one lane (what the overflow clamp produces), and a partial last chunk.
// No GPU, no library: c++ -std=c++17 tests/cpp/csr_scatter_rank_test.cpp && ./a.out
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

namespace {

constexpr int LANES = 64;
struct Entry {
    uint32_t point, slot;
    bool operator==(const Entry& o) const { return point == o.point && slot == o.slot; }
};
const Entry EMPTY{0xFFFFFFFFu, 0xFFFFFFFFu};

struct Result {
    std::vector<Entry> csr;
    std::vector<uint32_t> counters;
};

inline int popc(uint64_t m) { return __builtin_popcountll(m); }
inline uint64_t below(int lane) { return lane == 0 ? 0ull : (~0ull >> (64 - lane)); }

// one ranking step of the kernel: the vertex of the first lane with slot j pending; who holds it, in which slot
struct Step {
    int leader, k;
    uint64_t all;
    uint32_t hit[LANES];   // per lane: mask of its slots that hold k
};
template <int DP1>
bool next_vertex(const int (*lv)[DP1], uint32_t* pend, int j, Step& s) {
    uint64_t todo = 0;
    for (int l = 0; l < LANES; l++) todo |= (uint64_t)((pend[l] >> j) & 1u) << l;
    if (!todo) return false;
    s.leader = __builtin_ctzll(todo);
    s.k = lv[s.leader][j];
    s.all = 0;
    for (int l = 0; l < LANES; l++) s.hit[l] = 0;
    for (int jj = j; jj < DP1; jj++)
        for (int l = 0; l < LANES; l++)
            if (((pend[l] >> jj) & 1u) && lv[l][jj] == s.k) { s.all |= 1ull << l; s.hit[l] |= 1u << jj; }
    for (int l = 0; l < LANES; l++) pend[l] &= ~s.hit[l];
    return true;
}

template <int DP1>
void load_chunk(const std::vector<int>& ids, int n_points, int pc, int Mf, int (*lv)[DP1], uint32_t* pend, uint32_t* gp) {
    for (int l = 0; l < LANES; l++) {
        const int p = pc + l;
        const bool valid = p < n_points;
        gp[l] = (uint32_t)(valid ? p : n_points - 1);   // the kernel's clamp of the last partial chunk
        for (int j = 0; j < DP1; j++) {
            int v = ids[(size_t)gp[l] * DP1 + j];
            v = v < Mf ? v : Mf - 1;
            v = v < 0 ? 0 : v;
            lv[l][j] = v;
        }
        pend[l] = valid ? (1u << DP1) - 1u : 0u;
    }
}

template <int DP1>
Result scatter_old(const std::vector<int>& ids, int n_points, int Mf, const std::vector<uint32_t>& start) {
    Result r{std::vector<Entry>((size_t)n_points * DP1, EMPTY), start};
    int lv[LANES][DP1];
    uint32_t pend[LANES], gp[LANES];
    for (int pc = 0; pc < n_points; pc += LANES) {
        load_chunk<DP1>(ids, n_points, pc, Mf, lv, pend, gp);
        for (int j = 0; j < DP1; j++) {
            Step s;
            while (next_vertex<DP1>(lv, pend, j, s)) {
                const uint32_t b = r.counters[s.k];
                for (int l = 0; l < LANES; l++) {
                    if (!s.hit[l]) continue;
                    const uint32_t pos = b + (uint32_t)popc(s.all & below(l));
                    const uint32_t slot = 31 - __builtin_clz(s.hit[l]);   // the last matching slot's weight wins
                    if (pos < r.csr.size()) r.csr[pos] = Entry{gp[l], slot};
                }
                r.counters[s.k] = b + (uint32_t)popc(s.all);
            }
        }
    }
    return r;
}

template <int DP1>
Result scatter_new(const std::vector<int>& ids, int n_points, int Mf, const std::vector<uint32_t>& start) {
    Result r{std::vector<Entry>((size_t)n_points * DP1, EMPTY), start};
    int lv[LANES][DP1];
    uint32_t pend[LANES], gp[LANES];
    uint32_t rt[LANES][DP1], base[LANES][DP1];
    for (int pc = 0; pc < n_points; pc += LANES) {
        load_chunk<DP1>(ids, n_points, pc, Mf, lv, pend, gp);
        bool valid[LANES];
        for (int l = 0; l < LANES; l++) {
            valid[l] = pend[l] != 0;
            for (int j = 0; j < DP1; j++) rt[l][j] = 0;
        }
        for (int j = 0; j < DP1; j++) {   // rank: registers only
            Step s;
            while (next_vertex<DP1>(lv, pend, j, s)) {
                for (int l = 0; l < LANES; l++)
                    for (int jj = j; jj < DP1; jj++)
                        if ((s.hit[l] >> jj) & 1u) rt[l][jj] = (uint32_t)popc(s.all & below(l));
                rt[s.leader][j] |= (uint32_t)popc(s.all) << 8;
            }
        }
        for (int l = 0; l < LANES; l++)   // place: every read of the chunk before any of its writes
            for (int j = 0; j < DP1; j++) base[l][j] = r.counters[lv[l][j]];
        for (int l = 0; l < LANES; l++) {
            if (!valid[l]) continue;
            for (int j = 0; j < DP1; j++) {
                const uint32_t pos = base[l][j] + (rt[l][j] & 0xFFu);
                if (pos < r.csr.size()) r.csr[pos] = Entry{gp[l], (uint32_t)j};
            }
        }
        for (int l = 0; l < LANES; l++)
            for (int j = 0; j < DP1; j++)
                if (rt[l][j] >> 8) r.counters[lv[l][j]] = base[l][j] + (rt[l][j] >> 8);
    }
    return r;
}

// counters as the scan leaves them: the start of every vertex's list; with duplicates in a lane a list is shorter than
// its count, which both forms must treat alike
std::vector<uint32_t> starts(const std::vector<int>& ids, int Mf) {
    std::vector<uint32_t> cnt(Mf > 0 ? Mf : 1, 0u), st(Mf > 0 ? Mf : 1, 0u);
    for (int v : ids) cnt[v < 0 ? 0 : (v < Mf ? v : Mf - 1)]++;
    uint32_t run = 0;
    for (int k = 0; k < Mf; k++) { st[k] = run; run += cnt[k]; }
    return st;
}

int failures = 0;

template <int DP1>
void check(const char* what, const std::vector<int>& ids, int n_points, int Mf, bool a_permutation) {
    const std::vector<uint32_t> st = starts(ids, Mf);
    const Result a = scatter_old<DP1>(ids, n_points, Mf, st), b = scatter_new<DP1>(ids, n_points, Mf, st);
    bool ok = a.csr == b.csr && a.counters == b.counters;
    if (ok && a_permutation) {   // distinct ids per point: every entry placed once, ascending points inside a vertex
        for (const Entry& e : a.csr) ok = ok && !(e == EMPTY);
        for (int k = 0; ok && k < Mf; k++)
            for (uint32_t q = st[k] + 1; q < a.counters[k]; q++) ok = ok && a.csr[q - 1].point < a.csr[q].point;
    }
    std::printf("%-44s DP1 %d  %6d points  %5d vertices  %s\n", what, DP1, n_points, Mf, ok ? "ok" : "DIFFERENT");
    if (!ok) failures++;
}

template <int DP1>
void run(std::mt19937& rng) {
    const int sizes[] = {1, 63, 64, 65, 1024, 2664};   // 2664 = 41 chunks + 40 points
    for (int n : sizes) {
        std::vector<int> ids((size_t)n * DP1);
        // random rows, distinct inside a point, any vertex in any slot (so slots differ between lanes)
        for (int Mf : {DP1, 24, 300, 4096}) {
            for (int p = 0; p < n; p++)
                for (int j = 0; j < DP1; j++) {
                    int v;
                    bool again;
                    do {
                        v = (int)(rng() % (unsigned)Mf);
                        again = false;
                        for (int q = 0; q < j; q++) again = again || ids[(size_t)p * DP1 + q] == v;
                    } while (again);
                    ids[(size_t)p * DP1 + j] = v;
                }
            check<DP1>("random rows, vertices in any slot", ids, n, Mf, true);
        }
        // one simplex per chunk: totals of 64, rank = lane
        for (int p = 0; p < n; p++)
            for (int j = 0; j < DP1; j++) ids[(size_t)p * DP1 + j] = (p / 64 % 3) * DP1 + j;
        check<DP1>("one simplex per chunk", ids, n, 3 * DP1, true);
        // (nearly) all vertices of a chunk distinct
        for (int p = 0; p < n; p++)
            for (int j = 0; j < DP1; j++) ids[(size_t)p * DP1 + j] = (p % 61) * DP1 + j;
        check<DP1>("61 simplices per chunk", ids, n, 61 * DP1, true);
        // neighbouring simplices: a vertex moves one slot from lane to lane
        for (int p = 0; p < n; p++)
            for (int j = 0; j < DP1; j++) ids[(size_t)p * DP1 + j] = (p + j) % (DP1 + 5);
        check<DP1>("a vertex in another slot of every lane", ids, n, DP1 + 5, true);
        // ids past the vertex range and negative ones: the clamp puts one id into several slots of a lane
        for (int p = 0; p < n; p++)
            for (int j = 0; j < DP1; j++) ids[(size_t)p * DP1 + j] = (int)(rng() % 40u) - 8;
        check<DP1>("clamped rows, an id twice in a lane", ids, n, 20, false);
    }
}

}  // namespace

int main() {
    std::mt19937 rng(20261019u);
    run<3>(rng);
    run<6>(rng);
    run<7>(rng);
    if (failures) { std::printf("%d cases differ\n", failures); return 1; }
    std::printf("csr scatter rank ok\n");
    return 0;
}
