// The boosting rules of csrc/train_host.h and the vote rule of csrc/forest_model.h alone, under the host sanitizers
// (tests/test_boost_host_cpp_cpu.py): alpha's mixed precision for C = 2 and C = 9, the stop rules, the round keys, the
// vote label with ties, -inf entries, NaN and a single class.  No HIP, no library.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "train_host.h"

using namespace rvseg;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // alpha (learning.cpp:1197): float log + double log, narrowed
    for (float e : {0.01f, 0.3f, 0.5f, 0.75f, 0.999f}) {
        const BoostRound r2 = boost_round(e, 2), r9 = boost_round(e, 9);
        const float first = std::log((1 - e) / e);
        CHECK(r2.keep_tree && r2.go_on && r9.keep_tree && r9.go_on);
        CHECK(r2.alpha == (float)((double)first + std::log(1.0)));
        CHECK(r2.alpha == first);
        CHECK(r9.alpha == (float)((double)first + std::log(8.0)));
        CHECK(r2.scale == std::exp(r2.alpha) && r9.scale == std::exp(r9.alpha));
    }
    CHECK(boost_round(0.75f, 2).alpha < 0.f && boost_round(0.75f, 2).scale < 1.f);   // negative alpha is followed
    CHECK(boost_round(0.5f, 2).alpha == 0.f && boost_round(0.5f, 2).scale == 1.f);
    // stops
    const BoostRound zero = boost_round(0.f, 3);
    CHECK(zero.keep_tree && !zero.go_on && zero.alpha == inf);
    for (float e : {1.0f, 1.0000001f, 2.f, inf, nan}) {
        const BoostRound r = boost_round(e, 3);
        CHECK(!r.keep_tree && !r.go_on);
    }
    CHECK(boost_round(0.99999994f, 3).keep_tree);
    CHECK(boost_total_ok(1.f) && boost_total_ok(1e-45f) && boost_total_ok(3.4028234663852886e38f));
    CHECK(!boost_total_ok(0.f) && !boost_total_ok(-0.f) && !boost_total_ok(-1.f) && !boost_total_ok(inf) && !boost_total_ok(nan));
    // keys and draws (definition 1)
    CHECK(boost_round_key(7, 0) == mix64(7ull ^ mix64(0x626F6F73ull)) && boost_round_key(7, 0) != boost_round_key(7, 1));
    CHECK(boost_tree_seed(5) == draw64(5, 1ull << 40));
    for (uint64_t n = 0; n < 100000; n++) {
        const float u = boost_uniform(0xABCDEFull, n);
        CHECK(u >= 0.f && u < 1.f && u * 16777216.f == std::floor(u * 16777216.f));
    }
    // the vote label (classifier.cpp:29-51)
    { const float h[] = {-1.f, -0.5f, -0.5f, -2.f}; CHECK(vote_label(h, 4) == 1); }        // a tie: the first wins
    { const float h[] = {-0.5f, -0.5f}; CHECK(vote_label(h, 2) == 0); }
    { const float h[] = {-inf, -inf, -3.f}; CHECK(vote_label(h, 3) == 2); }
    { const float h[] = {-inf, -inf}; CHECK(vote_label(h, 2) == 0); }
    { const float h[] = {nan, 5.f}; CHECK(vote_label(h, 2) == 0); }                          // nothing beats a NaN in h[0]
    { const float h[] = {1.f, nan, 2.f}; CHECK(vote_label(h, 3) == 2); }                     // a NaN never wins
    { const float h[] = {-7.f}; CHECK(vote_label(h, 1) == 0); }                              // a single class
    std::printf("boost host ok\n");
    return 0;
}
