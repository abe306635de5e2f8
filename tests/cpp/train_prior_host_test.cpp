// The class-weighted split objective's host-side rules (csrc/train_host.h) alone: a stand-alone program for the host
// compiler with -fsanitize=address,undefined (tests/test_train_prior_host_cpp_cpu.py).  No HIP, no library.
// The expected bit patterns were worked out in fp32 by the numpy restatement (tests/train_prior_restate.py), one rounded
// operation at a time.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "train_host.h"

using namespace rvseg;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); g_fail++; } } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }
static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

static rvseg_class_prior prior_of(int mode, std::initializer_list<float> w = {}) {
    rvseg_class_prior p{};
    p.mode = mode;
    int c = 0;
    for (float x : w) p.weights[c++] = x;
    return p;
}

static void test_weight_formula() {
    // INVERSE_FREQUENCY: (float)Nb / (float)cnt_c over the counts after the bootstrap; an absent class gets 0 and is never read
    unsigned cnt[TR_CMAX] = {};
    cnt[0] = 36; cnt[2] = 4;
    float w[TR_CMAX];
    for (float& x : w) x = -1.f;
    class_prior_weights(prior_of(RVSEG_PRIOR_INVERSE_FREQUENCY), cnt, 3, w);
    CHECK(same_bits(w[0], from_bits(0x3f8e38e4u)) && same_bits(w[0], 40.f / 36.f));
    CHECK(same_bits(w[1], 0.f));
    CHECK(same_bits(w[2], 10.f));
    for (int c = 3; c < TR_CMAX; c++) CHECK(same_bits(w[c], 0.f));
    // the weights are the tree's: other counts, other weights, and Nb is their sum, not the set's size
    cnt[1] = 10;
    class_prior_weights(prior_of(RVSEG_PRIOR_INVERSE_FREQUENCY), cnt, 3, w);
    CHECK(same_bits(w[0], 50.f / 36.f) && same_bits(w[1], 5.f) && same_bits(w[2], 12.5f));
    // GIVEN: the caller's, whatever the counts; still nothing for an absent class or past C
    cnt[1] = 0;
    const rvseg_class_prior given = prior_of(RVSEG_PRIOR_GIVEN, {0.1f, 3.7f, 1e-3f, 9.f});
    class_prior_weights(given, cnt, 3, w);
    CHECK(same_bits(w[0], 0.1f) && same_bits(w[1], 0.f) && same_bits(w[2], 1e-3f) && same_bits(w[3], 0.f));
}

static void test_weighted_entropy() {
    CHECK(same_bits(fastlog2_host(10.f), from_bits(0x4054996eu)));
    const float nan = std::numeric_limits<float>::quiet_NaN();
    {   // counts (3, 0, 5), weights (0.1, unread, 3.7)
        unsigned cnt[TR_CMAX] = {3, 0, 5};
        float w[TR_CMAX] = {0.1f, nan, 3.7f};
        for (int c = 3; c < TR_CMAX; c++) w[c] = nan;   // a weight whose count is zero is never read
        CHECK(same_bits(weighted_hist_entropy(cnt, w), from_bits(0x400e1c40u)));
        // the same by hand: products first, each rounded, then the sums in class order
        const float p0 = 0.1f * 3.f, p2 = 3.7f * 5.f;
        float mass = 0.0f;
        mass += p0;
        mass += p2;
        float e = -entropy_term_host(mass);
        e += entropy_term_host(p0);
        e += entropy_term_host(p2);
        CHECK(same_bits(weighted_hist_entropy(cnt, w), e));
    }
    {   // counts (7, 1, 0), weights (0.1, 3.7, 1e-3)
        unsigned cnt[TR_CMAX] = {7, 1, 0};
        float w[TR_CMAX] = {0.1f, 3.7f, 1e-3f};
        CHECK(same_bits(weighted_hist_entropy(cnt, w), from_bits(0x40320034u)));
    }
    {   // ones: here the value of the integer expression, -ENTROPY(8) + ENTROPY(3) + ENTROPY(5)
        unsigned cnt[TR_CMAX] = {3, 0, 5};
        float w[TR_CMAX];
        for (float& x : w) x = 1.f;
        CHECK(same_bits(weighted_hist_entropy(cnt, w), from_bits(0x40f4587cu)));
        CHECK(same_bits(weighted_hist_entropy(cnt, w), -entropy_term_host(8.f) + entropy_term_host(3.f) + entropy_term_host(5.f)));
    }
    {   // all 16 classes, counts 1..16, weights 136 / count: every weighted count is about 136
        unsigned cnt[TR_CMAX];
        float w[TR_CMAX];
        for (int c = 0; c < TR_CMAX; c++) cnt[c] = (unsigned)c + 1u;
        rvseg_class_prior inv = prior_of(RVSEG_PRIOR_INVERSE_FREQUENCY);
        class_prior_weights(inv, cnt, TR_CMAX, w);
        CHECK(same_bits(w[2], 136.f / 3.f) && same_bits(w[15], 8.5f));
        CHECK(same_bits(weighted_hist_entropy(cnt, w), from_bits(0x4607fffcu)));
    }
}

static void test_refusals() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // no prior and NONE are fine for 2..16 classes; C outside is refused whatever the prior
    const rvseg_class_prior none = prior_of(RVSEG_PRIOR_NONE), inv = prior_of(RVSEG_PRIOR_INVERSE_FREQUENCY);
    for (int C : {2, 9, 16}) { CHECK(!class_prior_error(nullptr, C)); CHECK(!class_prior_error(&none, C)); CHECK(!class_prior_error(&inv, C)); }
    for (int C : {-1, 0, 1, 17}) {
        const char* e = class_prior_error(&inv, C);
        CHECK(e && std::strstr(e, "C:"));
        CHECK(class_prior_error(nullptr, C) != nullptr);
    }
    // an unknown mode
    for (int mode : {-1, 3, 1 << 20}) {
        const rvseg_class_prior p = prior_of(mode);
        const char* e = class_prior_error(&p, 3);
        CHECK(e && std::strstr(e, "mode"));
    }
    // NONE and INVERSE_FREQUENCY do not read the weights
    const rvseg_class_prior junk = prior_of(RVSEG_PRIOR_INVERSE_FREQUENCY, {nan, -1.f, inf});
    CHECK(!class_prior_error(&junk, 3));
    // GIVEN: each of the first C finite and > 0; past C anything goes
    const rvseg_class_prior ok = prior_of(RVSEG_PRIOR_GIVEN, {1.f, 1e-38f, 3.4e38f, nan});
    CHECK(!class_prior_error(&ok, 3));
    CHECK(class_prior_error(&ok, 4) != nullptr);
    for (float bad : {0.f, -0.f, -1.f, inf, -inf, nan}) {
        for (int at = 0; at < 3; at++) {
            rvseg_class_prior p = prior_of(RVSEG_PRIOR_GIVEN, {1.f, 2.f, 3.f});
            p.weights[at] = bad;
            const char* e = class_prior_error(&p, 3);
            CHECK(e && std::strstr(e, "weights"));
        }
    }
}

int main() {
    test_weight_formula();
    test_weighted_entropy();
    test_refusals();
    if (g_fail) { std::printf("%d check(s) failed\n", g_fail); return 1; }
    std::printf("train prior host ok\n");
    return 0;
}
