// transform_pk.hpp -- the LIMITED descriptor (transform.hpp limited_descriptor; reference
// include/impl/cpu/descriptor_transform.hpp:31-73) of TWO pixels at once, as 16-bit fields of
// 32-bit registers, in plain integer C++ that compiles for the host as well:
// transform_limited_pk_kernel (kernels.hip) runs exactly these functions on the GPU, and
// tests/cpp/transform_pk_check.cpp checks them on the CPU against a scalar restatement of the
// descriptor (tests/test_transform_pk.py).
//
// Every LIMITED bit is x < y with x, y <= 510: u8 samples, the mean threshold
// thr = ceil(sum / n) <= 255, and sums of two samples. With X = x_lo | x_hi << 16 and Y
// likewise, D = (0x7FFF7FFF - X) + Y holds 0x7FFF + (y - x) in each field: within
// [0x7FFF - 510, 0x7FFF + 510], so nothing borrows or carries across bit 16, and bit 15 /
// bit 31 is set exactly where x_lo < y_lo / x_hi < y_hi. 0x7FFF7FFF - X is taken once per
// left operand (a sample is the left operand of three comparisons, a pair sum of one), which
// leaves per comparison of two pixels: one add, one and with 0x80008000, one shift to the
// bit's place in its 16-bit accumulator field, one or -- all two-operand integer ops, which
// issue at full rate on gfx950 (the v_cmp into an SGPR mask + v_addc of the one-pixel kernel
// are two half-rate ops per pixel and bit; profiles/valu_rates_r04.jsonl).
//
// Accumulator j holds descriptor bits 16 j .. 16 j + 15 of the low-field pixel in bits 0..15
// and of the high-field pixel in bits 16..31, each bit at its final LSB-first place, so a
// pixel's word m is two half-words of accumulators 2 m and 2 m + 1 (pair_words).
#pragma once

#include <stdint.h>

#if defined(__HIP__)
#define BICOS_TPK_FN __host__ __device__ inline
#else
#define BICOS_TPK_FN inline
#endif
// On the GPU the steps are emitted in their order: left to itself the instruction scheduler
// moves every step's sample and pair-sum arithmetic to the front and holds two to three
// registers per plane.
// Likewise an accumulator takes each bit as it comes (an empty asm makes it opaque): hipcc
// otherwise re-associates an accumulator's ors into trees at the end and keeps every masked
// bit in a register of its own until then (152 VGPRs for two pairs at n = 33 against 55).
#if defined(__HIP_DEVICE_COMPILE__)
#define BICOS_TPK_STEP_DONE() __builtin_amdgcn_sched_barrier(0)
#define BICOS_TPK_KEEP(x) asm("" : "+v"(x))
#else
#define BICOS_TPK_STEP_DONE() ((void)0)
#define BICOS_TPK_KEEP(x) ((void)0)
#endif

namespace bicos_hip {
namespace tpk {

constexpr uint32_t BIAS = 0x7FFF7FFFu;  // per field: the largest value below the sign bit
constexpr uint32_t SIGN = 0x80008000u;

// bits of the LIMITED descriptor of an n-image stack, and the bits its per-t loop emits
// before the four tail bits (transform.hpp limited_descriptor `nl`)
constexpr int loop_bits(int n) { return n >= 4 ? 6 + 4 * (n - 4) : 3 * (n - 2); }
constexpr int limited_bits(int n) { return loop_bits(n) + 4; }
constexpr int accumulators(int n) { return (limited_bits(n) + 15) / 16; }
// the narrowest descriptor (32-bit words: 1, 2, 4, 8) that holds them; 0: none does
constexpr int limited_words(int n) {
    return n < 2 ? 0 : limited_bits(n) <= 32 ? 1 : limited_bits(n) <= 64 ? 2
         : limited_bits(n) <= 128 ? 4 : limited_bits(n) <= 256 ? 8 : 0;
}
// the stack sizes the packed kernel is built for: the exact sizes of the one-pixel kernel's
// buckets (kernels.hip launch_transform_w), each at its narrowest descriptor
constexpr bool built(int n) {
    return n == 9 || n == 12 || n == 17 || n == 24 || n == 33 || n == 40 || n == 48 || n == 65;
}

// the left operand's form: 0x7FFF - x per field
BICOS_TPK_FN uint32_t left(uint32_t X) { return BIAS - X; }
// bit 15 / bit 31 set exactly where x_lo < y_lo / x_hi < y_hi (nx = left(X)); the other bits
// are not zero
BICOS_TPK_FN uint32_t less(uint32_t nx, uint32_t Y) { return nx + Y; }

// comparison -> descriptor bit K of both pixels
template <int K, int ACC>
BICOS_TPK_FN void put(uint32_t (&acc)[ACC], uint32_t nx, uint32_t Y) {
    static_assert(K >= 0 && K / 16 < ACC, "bit outside the accumulators");
    const uint32_t d = less(nx, Y) & SIGN;
    acc[K / 16] |= d >> (15 - K % 16);
    BICOS_TPK_KEEP(acc[K / 16]);
}

// ceil(sum / n) for sum < 2^24, n <= 65, magic = ceil(2^32 / n): floor((sum + n - 1) / n) by
// the high half of a product, exact because the reciprocal's error sum * n / 2^32 < 2^-8 < 1/n
BICOS_TPK_FN uint32_t ceil_div(uint32_t sum, uint32_t n, uint32_t magic) {
    return (uint32_t)(((uint64_t)(sum + n - 1) * magic) >> 32);
}

// The sum of the samples X(0) .. X(N - 1), per field (<= 65 * 255 < 2^16), and the mean
// threshold ceil(sum / N) of both fields, magic = ceil(2^32 / N)
template <int N, class Sample>
BICOS_TPK_FN uint32_t pair_sum(const Sample& X) {
    uint32_t sum = 0;
#pragma unroll
    for (int t = 0; t < N; ++t) sum += X(t);
    return sum;
}
BICOS_TPK_FN uint32_t pair_threshold(uint32_t sum, uint32_t n, uint32_t magic) {
    return ceil_div(sum & 0xFFFFu, n, magic) | ceil_div(sum >> 16, n, magic) << 16;
}

// The loop's step T (transform.hpp limited_steps): a<b, a<c, a<thr, and from T = 2 on
// ps[T-2] < ps[T], at bits 3 T (T < 2) or 6 + 4 (T - 2); then the tail
// (descriptor_transform.hpp:63-68): p[n-2]<p[n-1], p[n-2]<av, p[n-1]<av, ps[n-4]<ps[n-2] --
// which without a ps[n-4] (n < 4) compares -1 and is set. One sample is fetched per step and
// the window goes along: a = X(T), b = X(T + 1), ps2 = ps[T - 2], ps1 = ps[T - 1], where
// ps[t] = X(t) + X(t + 1) (fields <= 510).
template <int T, int N, int ACC, class Sample>
BICOS_TPK_FN void steps(const Sample& X, uint32_t a, uint32_t b, uint32_t ps2, uint32_t ps1,
                        uint32_t thr, uint32_t (&acc)[ACC]) {
    const uint32_t na = left(a);
    const uint32_t cur = a + b;  // ps[T]
    if constexpr (T < N - 2) {
        constexpr int pos = T < 2 ? 3 * T : 6 + 4 * (T - 2);
        const uint32_t c = X(T + 2);
        put<pos>(acc, na, b);
        put<pos + 1>(acc, na, c);
        put<pos + 2>(acc, na, thr);
        if constexpr (T >= 2) put<pos + 3>(acc, left(ps2), cur);
        BICOS_TPK_STEP_DONE();
        steps<T + 1, N, ACC>(X, b, c, ps1, cur, thr, acc);
    } else {
        constexpr int nl = loop_bits(N);
        put<nl>(acc, na, b);
        put<nl + 1>(acc, na, thr);
        put<nl + 2>(acc, left(b), thr);
        if constexpr (N >= 4)
            put<nl + 3>(acc, left(ps2), cur);
        else
            acc[(nl + 3) / 16] |= 0x00010001u << ((nl + 3) % 16);
    }
}

// The descriptor bits of two pixels from their samples and threshold: X(t) = sample t of the
// low-field pixel | sample t of the high-field pixel << 16 (u8 samples), t a constant.
template <int N, class Sample>
BICOS_TPK_FN void pair_bits(const Sample& X, uint32_t thr, uint32_t (&acc)[accumulators(N)]) {
    static_assert(N >= 2 && N <= 65, "fields hold sums of at most 65 u8 samples");
#pragma unroll
    for (int j = 0; j < accumulators(N); ++j) acc[j] = 0;
    steps<0, N, accumulators(N)>(X, X(0), X(1), 0u, 0u, thr, acc);
}

// ... and the whole of it: the sum, the threshold, the bits
template <int N, class Sample>
BICOS_TPK_FN void pair_descriptor(const Sample& X, uint32_t magic, uint32_t (&acc)[accumulators(N)]) {
    pair_bits<N>(X, pair_threshold(pair_sum<N>(X), N, magic), acc);
}

// word m of the low-field pixel (lo) and of the high-field pixel (hi), m < WORDS; words past
// the accumulators are zero
template <int WORDS, int ACC>
BICOS_TPK_FN void pair_words(const uint32_t (&acc)[ACC], uint32_t (&lo)[WORDS], uint32_t (&hi)[WORDS]) {
    static_assert(ACC <= 2 * WORDS, "descriptor too narrow");
#pragma unroll
    for (int m = 0; m < WORDS; ++m) {
        const uint32_t a = 2 * m < ACC ? acc[2 * m] : 0u;
        const uint32_t b = 2 * m + 1 < ACC ? acc[2 * m + 1] : 0u;
        lo[m] = (a & 0xFFFFu) | b << 16;
        hi[m] = a >> 16 | (b & 0xFFFF0000u);
    }
}

// four adjacent u8 pixels of one plane, as loaded in one dword (pixel i in byte i), to the
// packed samples of pixels (0, 2) and of pixels (1, 3)
BICOS_TPK_FN uint32_t even_pixels(uint32_t dword) { return dword & 0x00FF00FFu; }
BICOS_TPK_FN uint32_t odd_pixels(uint32_t dword) { return dword >> 8 & 0x00FF00FFu; }

}  // namespace tpk
}  // namespace bicos_hip
