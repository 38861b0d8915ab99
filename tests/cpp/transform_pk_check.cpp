// transform_pk_check.cpp -- TEST PROGRAM (tests/test_transform_pk.py, no GPU): the integer
// arithmetic of the packed LIMITED transform (libbicos_amd/csrc/transform_pk.hpp, which
// transform_limited_pk_kernel runs on the GPU), checked on the CPU. Links nothing but that header.
//
//   transform_pk_check   one "<what> ok <count>" line per property, exit status 1 and
//                        "FAIL ..." lines on a violation:
//     compare     less() for every x, y in 0..510 in one field with independent pairs
//                 (extremes and pseudo-random ones) in the other, either field
//     threshold   ceil_div against the division and against the reference's float mean
//     split       even_pixels / odd_pixels on every byte in every place
//     descriptor  pair_descriptor + pair_words against a plain one-pixel restatement of the
//                 reference's LIMITED descriptor (float mean, sequential bit writer), for
//                 n = 2 3 4 5 9 12 17 24 33 40 48 65 over random, constant, 0/255 alternating
//                 and neighbour-extremes inputs
#include "transform_pk.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace bicos_hip::tpk;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures++ < 20) {                        \
                std::printf("FAIL %s: ", #cond);          \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd() {  // xorshift32
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

// -------------------------------------------------------------------------------- compare
static long check_compare() {
    long count = 0;
    for (uint32_t x = 0; x <= 510; ++x)
        for (uint32_t y = 0; y <= 510; ++y) {
            // the other field: the extremes (every borrow / carry it could send or take), its
            // own equal and off-by-one cases, and pseudo-random pairs
            uint32_t other[12][2] = {{0, 0}, {0, 510}, {510, 0}, {510, 510}, {x, y}, {y, x},
                                     {255, 256}, {256, 255}};
            for (int i = 8; i < 12; ++i) {
                other[i][0] = rnd() % 511;
                other[i][1] = rnd() % 511;
            }
            for (auto& o : other) {
                const uint32_t u = o[0], v = o[1];
                const uint32_t d0 = less(left(x | u << 16), y | v << 16);
                CHECK(((d0 >> 15) & 1) == (x < y) && (d0 >> 31) == (u < v), "lo %u<%u hi %u<%u: %08x",
                      x, y, u, v, d0);
                const uint32_t d1 = less(left(u | x << 16), v | y << 16);
                CHECK(((d1 >> 15) & 1) == (u < v) && (d1 >> 31) == (x < y), "lo %u<%u hi %u<%u: %08x",
                      u, v, x, y, d1);
                count += 2;
            }
        }
    return count;
}

// ------------------------------------------------------------------------------ threshold
static long check_threshold() {
    long count = 0;
    for (uint32_t n = 2; n <= 65; ++n) {
        const uint32_t magic = (uint32_t)((0x100000000ull + n - 1) / n);
        for (uint32_t sum = 0; sum <= n * 255; ++sum) {
            const uint32_t thr = ceil_div(sum, n, magic);
            CHECK(thr == (sum + n - 1) / n, "n %u sum %u: %u", n, sum, thr);
            // a < thr is the reference's (float)a < (float)sum / (float)n for every sample a
            const float av = (float)sum / (float)n;
            for (uint32_t a = thr > 2 ? thr - 2 : 0; a <= thr + 1 && a <= 255; ++a)
                CHECK((a < thr) == ((float)a < av), "n %u sum %u a %u", n, sum, a);
            ++count;
        }
    }
    return count;
}

// ---------------------------------------------------------------------------------- split
static long check_split() {
    long count = 0;
    for (uint32_t b = 0; b < 256; ++b)
        for (int place = 0; place < 4; ++place) {
            const uint32_t fill = rnd();
            const uint32_t d = (fill & ~(0xFFu << (8 * place))) | b << (8 * place);
            const uint32_t px[4] = {d & 0xFF, (d >> 8) & 0xFF, (d >> 16) & 0xFF, d >> 24};
            CHECK(even_pixels(d) == (px[0] | px[2] << 16), "%08x", d);
            CHECK(odd_pixels(d) == (px[1] | px[3] << 16), "%08x", d);
            ++count;
        }
    return count;
}

// ----------------------------------------------------------------------------- descriptor
// One pixel's LIMITED descriptor as the reference computes it (descriptor_transform.hpp:31-73):
// float mean, bits in sequence, LSB first.
static std::vector<uint32_t> scalar_descriptor(const uint8_t* p, int n, int words) {
    std::vector<uint32_t> w(words, 0u);
    int k = 0;
    auto set = [&](bool v) {
        if (v) w[k / 32] |= 1u << (k % 32);
        ++k;
    };
    float sum = 0.f;
    for (int t = 0; t < n; ++t) sum += (float)p[t];
    const float av = sum / (float)n;
    int pm1 = -1, pm2 = -1;
    uint32_t a = p[0], b = p[1];
    for (int t = 0; t < n - 2; ++t) {
        const uint32_t c = p[t + 2];
        set(a < b);
        set(a < c);
        set((float)a < av);
        const int cur = (int)(a + b);
        if (t >= 2) set(pm2 < cur);
        pm2 = pm1;
        pm1 = cur;
        a = b;
        b = c;
    }
    set(a < b);
    set((float)a < av);
    set((float)b < av);
    set(pm2 < (int)(a + b));
    return w;
}

template <int N>
static long check_pair(const uint8_t* lo, const uint8_t* hi, const char* what) {
    constexpr int WORDS = limited_words(N);
    static_assert(WORDS > 0, "no descriptor holds this stack size");
    uint32_t X[N];
    for (int t = 0; t < N; ++t) X[t] = lo[t] | (uint32_t)hi[t] << 16;
    uint32_t acc[accumulators(N)];
    pair_descriptor<N>([&](int t) { return X[t]; }, (uint32_t)((0x100000000ull + N - 1) / N), acc);
    uint32_t wl[WORDS], wh[WORDS];
    pair_words<WORDS>(acc, wl, wh);
    const std::vector<uint32_t> rl = scalar_descriptor(lo, N, WORDS), rh = scalar_descriptor(hi, N, WORDS);
    CHECK(std::memcmp(wl, rl.data(), 4 * WORDS) == 0, "n %d %s: low pixel, word0 %08x vs %08x", N,
          what, wl[0], rl[0]);
    CHECK(std::memcmp(wh, rh.data(), 4 * WORDS) == 0, "n %d %s: high pixel, word0 %08x vs %08x", N,
          what, wh[0], rh[0]);
    return 2;
}

template <int N>
static long check_descriptor() {
    long count = 0;
    uint8_t lo[N], hi[N];
    for (int trial = 0; trial < 4000; ++trial) {  // random: full range, then close to each other
        const int spread = trial < 2000 ? 256 : 1 + trial % 7;
        const int base_lo = (int)(rnd() % (257 - spread)), base_hi = (int)(rnd() % (257 - spread));
        for (int t = 0; t < N; ++t) {
            lo[t] = (uint8_t)(base_lo + (int)(rnd() % spread));
            hi[t] = (uint8_t)(base_hi + (int)(rnd() % spread));
        }
        count += check_pair<N>(lo, hi, "random");
    }
    for (int c = 0; c < 256; ++c) {  // constant: no comparison is true, whatever the neighbour
        std::memset(lo, c, N);
        std::memset(hi, 255 - c, N);
        count += check_pair<N>(lo, hi, "constant");
        count += check_pair<N>(lo, lo, "constant");
    }
    for (int phase = 0; phase < 2; ++phase) {  // 0 / 255 alternating, in and out of step
        for (int t = 0; t < N; ++t) {
            lo[t] = (t + phase) % 2 ? 255 : 0;
            hi[t] = t % 2 ? 255 : 0;
        }
        count += check_pair<N>(lo, hi, "alternating");
    }
    // neighbour extremes: one pixel rises as fast as u8 allows from 0 with a spike at the end
    // (every sample, pair-sum and mean comparison true where the data can make it so), the
    // other falls (every comparison false), in either field: a leak between the fields shows
    for (int swap = 0; swap < 2; ++swap) {
        for (int t = 0; t < N; ++t) {
            const int up = t == N - 1 ? 255 : t * 3, down = t == N - 1 ? 0 : 255 - t * 3;
            lo[t] = (uint8_t)(swap ? down : up);
            hi[t] = (uint8_t)(swap ? up : down);
        }
        count += check_pair<N>(lo, hi, "neighbour extremes");
        for (int t = 0; t < N; ++t) {  // and every sample of one at 0, of the other at 255
            lo[t] = swap ? 255 : 0;
            hi[t] = swap ? 0 : 255;
        }
        count += check_pair<N>(lo, hi, "neighbour extremes");
    }
    return count;
}

int main() {
    std::printf("compare ok %ld\n", check_compare());
    std::printf("threshold ok %ld\n", check_threshold());
    std::printf("split ok %ld\n", check_split());
    long d = 0;
    d += check_descriptor<2>();
    d += check_descriptor<3>();
    d += check_descriptor<4>();
    d += check_descriptor<5>();
    d += check_descriptor<9>();
    d += check_descriptor<12>();
    d += check_descriptor<17>();
    d += check_descriptor<24>();
    d += check_descriptor<33>();
    d += check_descriptor<40>();
    d += check_descriptor<48>();
    d += check_descriptor<65>();
    std::printf("descriptor ok %ld\n", d);
    if (failures) std::printf("%d violations\n", failures);
    return failures ? 1 : 0;
}
