// search_mx_common.hpp -- device helpers shared by the matrix-core searches (search_mx.hip,
// search_range.hip): the FP4 expansion of descriptor bits, the unscaled FP4 x FP4 MFMA, the
// float argmin keys riding in the accumulator (search_mx.hip's header comment) and their
// 16-register min / max trees.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicos_hip {

namespace {

constexpr int16_t INVALID_I16 = -32768;

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr float KEY_BIAS = 256.f;
constexpr float KEY_EPS = 1.f / 32768.f;  // col1 * 2^-15
constexpr float KEY_PAD = 1.0e30f;        // C of columns beyond the image (A = 0 there)

// 32 descriptor bits -> 32 FP4 elements through a byte table: byte q of dword m holds bits
// 8q + 2m (low nibble) and 8q + 2m + 1 (high nibble), i.e. dword m = v_perm of the 4-entry
// table `lut` (one byte per bit pair) selected by the pairs (x >> 2m) & 3 of every byte.
// The order of the bits along K does not matter as long as both operands use the same
// one; 4 v_perm + 7 shift/and per word instead of ~28 shift/or/and.
constexpr uint32_t LUT_A = 0x22200200u;  // right (A): bit 1 -> 1.0 (0x2), 0 -> 0
constexpr uint32_t LUT_B = 0xAAA22A22u;  // left (B): bit 1 -> -1.0 (0xA), 0 -> +1.0 (0x2)
__device__ __forceinline__ v4i expand_bits(uint32_t x, uint32_t lut) {
    v4i r;
#pragma unroll
    for (int m = 0; m < 4; ++m)
        r[m] = (int)__builtin_amdgcn_perm(lut, lut, (x >> (2 * m)) & 0x03030303u);
    return r;
}

__device__ __forceinline__ uint32_t umin3(uint32_t a, uint32_t b, uint32_t c) {
    return min(min(a, b), c);
}
__device__ __forceinline__ uint32_t umax3(uint32_t a, uint32_t b, uint32_t c) {
    return max(max(a, b), c);
}

__device__ __forceinline__ uint32_t fbits(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ __forceinline__ float bitsf(uint32_t u) { return __builtin_bit_cast(float, u); }

constexpr uint32_t KEY_NONE = 0x7F000000u;  // above every key

// min over the 16 keys of a D tile (bits ^ flip) and m; depth-3 tree of v_min3_u32. (The
// keys are positive floats, so v_min3_f32 would do too; measured: it issues at the same half
// rate as v_min3_u32 on gfx950 -- profiles/valu_rates_r02.jsonl -- and the search ran the
// same, cfg2 0.400 vs 0.400 ms, cfg4 0.87 vs 0.86 ms.)
__device__ __forceinline__ uint32_t min16(const v16f& d, uint32_t m, uint32_t flip) {
    // (element copied first: __builtin_bit_cast of a vector-element lvalue reads element 0)
    auto k = [&](int r) { return fbits(d[r]) ^ flip; };
    const uint32_t a0 = umin3(k(0), k(1), k(2)), a1 = umin3(k(3), k(4), k(5));
    const uint32_t a2 = umin3(k(6), k(7), k(8)), a3 = umin3(k(9), k(10), k(11));
    const uint32_t a4 = umin3(k(12), k(13), k(14));
    return umin3(m, umin3(a0, a1, a2), umin3(a3, a4, k(15)));
}
__device__ __forceinline__ uint32_t max16(const v16f& d, uint32_t m) {
    auto k = [&](int r) { return fbits(d[r]); };
    const uint32_t a0 = umax3(k(0), k(1), k(2)), a1 = umax3(k(3), k(4), k(5));
    const uint32_t a2 = umax3(k(6), k(7), k(8)), a3 = umax3(k(9), k(10), k(11));
    const uint32_t a4 = umax3(k(12), k(13), k(14));
    return umax3(m, umax3(a0, a1, a2), umax3(a3, a4, k(15)));
}

__device__ __forceinline__ v16f mfma_fp4(v4i a, v4i b, v16f c) {
    const v8i a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0};
    const v8i b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
    // cbsz = blgp = 4: both operands FP4 e2m1; zero scales = the unscaled instruction
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, 0, 0, 0);
}

constexpr uint32_t XK_INF = 0x7F000000u;  // "no key yet"; stays huge under the shifts
// KEYS 3 (float keys, no C matrix): where the descriptors leave the upper lane half of the
// last 64-bit K-step free (e.g. 256-bit words with <= 160 transform bits, cfg4's 154), that
// half carries the column: the right operand holds the binary digits of col1 % 32 there
// (FP4 1, 2, 4, 4+4, 4+4+4+4 in nine elements), the left operand is +1.0 (its descriptor bits
// are 0), and the MFMA scales that half of the right operand by 2^-12. So D = x + (col1 %
// 32) * 2^-12 with C = 0 (an inline constant): 16 VGPRs freer than the XK keys. The running
// minimum is kept relative to the current block base B, D = x + (col1 - B) * 2^-12, moved by
// -32 * 2^-12 per (ascending) block with one float subtract; |col1 - B| < 2048 keeps the
// column term inside (-0.5, 0.5), so floats order by x first and then by col1 (the first
// minimum, v_min3_f32), rint(D) = x, and (D - x) * 4096 = col1 - B exactly (|D| < 256 ->
// ulp 2^-16). NoDuplicates keeps the XK keys (the last minimum needs the bit trick).
constexpr float FK_EPS = 1.f / 4096.f;
constexpr int FK_SCALE_E8M0 = 127 - 12;  // 2^-12

// FK column digits of r = col1 % 32 as one lane's 32 FP4 elements (element k = nibble k):
// 1.0 * bit0, 2.0 * bit1, 4.0 * bit2, 4.0 * bit3 (twice), 4.0 * bit4 (four times)
__device__ __forceinline__ v4i fk_digits(int r) {
    uint32_t w0 = 0, w1 = 0;
    w0 |= (r & 1) ? 0x2u : 0u;
    w0 |= (r & 2) ? 0x40u : 0u;
    w0 |= (r & 4) ? 0x600u : 0u;
    w0 |= (r & 8) ? 0x66000u : 0u;
    w0 |= (r & 16) ? 0x66600000u : 0u;
    w1 |= (r & 16) ? 0x6u : 0u;
    return v4i{(int)w0, (int)w1, 0, 0};
}

__device__ __forceinline__ float fmin3(float a, float b, float c) {
    return __builtin_fminf(__builtin_fminf(a, b), c);
}
// min over the 16 float keys of a D tile and m (v_min3_f32 tree)
__device__ __forceinline__ float fmin16(const v16f& d, float m) {
    const float a0 = fmin3(d[0], d[1], d[2]), a1 = fmin3(d[3], d[4], d[5]);
    const float a2 = fmin3(d[6], d[7], d[8]), a3 = fmin3(d[9], d[10], d[11]);
    const float a4 = fmin3(d[12], d[13], d[14]);
    return fmin3(m, fmin3(a0, a1, a2), fmin3(a3, a4, d[15]));
}

// the same with E8M0 scales: sa for this lane's block of the right operand (A), 2^0 for B
__device__ __forceinline__ v16f mfma_fp4_sa(v4i a, v4i b, v16f c, int sa) {
    const v8i a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0};
    const v8i b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, sa, 0, 127);
}

// col1 encoded in a key (D1 or D2 bits): key - 256 = +-x + col1 * 2^-15, x integer
__device__ __forceinline__ int key_col(uint32_t key) {
    const float v = bitsf(key) - KEY_BIAS;  // exact
    return (int)((v - floorf(v)) * 32768.f);
}

}  // namespace

}  // namespace bicos_hip
