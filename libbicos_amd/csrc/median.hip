// median.hip -- the median filter of a disparity map (median.hpp; the definition is
// include/bicos_c.h, "median filter"): per pixel the lower median of the VALID values of its
// 3x3 or 5x5 window, clipped at the image border, optionally written into invalid pixels
// (holes) whose window holds at least fill_min valid values. One launch.
//
// KEYS. Both map types become unsigned 32-bit keys whose unsigned order is the order of the
// definition, with 0 free to mean "invalid or outside the image":
//     float   k = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000). k = 0 and k = 0xFFFFFFFF are
//             the keys of the NaN patterns 0xFFFFFFFF and 0x7FFFFFFF; no valid float has them.
//     int16   k = v + 32768: 1 .. 65535 for a valid v, and 0 for -32768 by itself.
// Both maps are bijections on the valid values, so the selected key turns back into the bits
// of one definite input pixel, and "output bits differ from input bits" is a key comparison.
//
// ONE NETWORK FOR EVERY m. A window has N = ksize^2 slots of which i are invalid or outside.
// Visiting the slots in row-major order, the j-th such slot becomes the pad 0 (below every
// valid key) for even j and 0xFFFFFFFF (above every valid key) for odd j: ceil(i/2) low and
// floor(i/2) high pads. The element of rank (N-1)/2 of the padded N keys is then the element
// of rank floor((m-1)/2) of the m = N - i valid ones, because
//     ceil(i/2) + floor((N-i-1)/2) = (N-1)/2     for odd N
// (i even: i/2 + (N-1-i)/2; i odd: (i+1)/2 + (N-i-2)/2 with N-i even, floor takes the half
// away). It is a pad exactly when m = 0, and then nothing is written from it. So a fixed,
// branch-free selection network serves clipped and holed windows alike; the cost is one
// toggle word per lane.
//
// SELECTION. Exchange networks of unsigned min / max on named registers (never indexed at
// run time): the 19-exchange median of 9 and the 99-exchange median of 25 of Paeth, "Median
// finding on a 3x3 grid", Graphics Gems (1990), and N. Devillard, "Fast median search: an
// ANSI C implementation" (1998). tests/test_median_api.py reads the CX lists below and
// proves both by the 0-1 principle over all 2^9 and 2^25 inputs.
//
// COUNTS. Ballots per wave kept in a wave-uniform register over all of the workgroup's tiles,
// summed over the waves in LDS, then one atomic instruction per workgroup; at most
// MEDIAN_MAX_BLOCKS workgroups stride over the tiles. Integer sums: the order is irrelevant.
// No workgroup reads what another writes: there is no flag, wait or protocol between them.
#include "median.hpp"

#include "../../include/bicos_c.h"

namespace bicos_hip {
namespace {

constexpr int WAVE = 64;
constexpr int TR = MEDIAN_TILE_ROWS, TC = MEDIAN_TILE_COLS;
constexpr int WAVES = MEDIAN_THREADS / WAVE;
constexpr int ROWS_PER_WAVE = TR / WAVES;
constexpr uint32_t PAD_LOW = 0u;  // its complement 0xFFFFFFFF is the high pad
static_assert(TC == WAVE, "a wave owns a tile row");
static_assert(MEDIAN_THREADS % WAVE == 0 && TR % WAVES == 0, "whole waves, whole rows");

// the key of a pixel, 0 where it is invalid
__device__ __forceinline__ uint32_t pixel_key(int16_t v, int) { return (uint32_t)((int)v + 32768); }
__device__ __forceinline__ uint32_t pixel_key(float v, int flags) {
    const uint32_t bits = __float_as_uint(v);
    const bool invalid = v != v || ((flags & BICOS_MEDIAN_F32_SENTINEL) && bits == 0xC7000000u);
    return invalid ? 0u : bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
// the pixel of a valid key
template <typename T>
__device__ __forceinline__ T key_pixel(uint32_t k);
template <>
__device__ __forceinline__ int16_t key_pixel<int16_t>(uint32_t k) {
    return (int16_t)((int)k - 32768);
}
template <>
__device__ __forceinline__ float key_pixel<float>(uint32_t k) {
    return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k);
}

#define CX(i, j)                                          \
    {                                                     \
        const uint32_t lo_ = v[i] < v[j] ? v[i] : v[j];   \
        v[j] = v[i] < v[j] ? v[j] : v[i];                 \
        v[i] = lo_;                                       \
    }

// the element of rank 4 of v[0..9)
__device__ __forceinline__ uint32_t select9(uint32_t (&v)[9]) {
    // NETWORK 9
    CX(1, 2) CX(4, 5) CX(7, 8) CX(0, 1) CX(3, 4) CX(6, 7) CX(1, 2) CX(4, 5) CX(7, 8) CX(0, 3)
    CX(5, 8) CX(4, 7) CX(3, 6) CX(1, 4) CX(2, 5) CX(4, 7) CX(4, 2) CX(6, 4) CX(4, 2)
    // END
    return v[4];
}

// the element of rank 12 of v[0..25)
__device__ __forceinline__ uint32_t select25(uint32_t (&v)[25]) {
    // NETWORK 25
    CX(0, 1) CX(3, 4) CX(2, 4) CX(2, 3) CX(6, 7) CX(5, 7) CX(5, 6) CX(9, 10) CX(8, 10)
    CX(8, 9) CX(12, 13) CX(11, 13) CX(11, 12) CX(15, 16) CX(14, 16) CX(14, 15) CX(18, 19)
    CX(17, 19) CX(17, 18) CX(21, 22) CX(20, 22) CX(20, 21) CX(23, 24) CX(2, 5) CX(3, 6)
    CX(0, 6) CX(0, 3) CX(4, 7) CX(1, 7) CX(1, 4) CX(11, 14) CX(8, 14) CX(8, 11) CX(12, 15)
    CX(9, 15) CX(9, 12) CX(13, 16) CX(10, 16) CX(10, 13) CX(20, 23) CX(17, 23) CX(17, 20)
    CX(21, 24) CX(18, 24) CX(18, 21) CX(19, 22) CX(8, 17) CX(9, 18) CX(0, 18) CX(0, 9)
    CX(10, 19) CX(1, 19) CX(1, 10) CX(11, 20) CX(2, 20) CX(2, 11) CX(12, 21) CX(3, 21)
    CX(3, 12) CX(13, 22) CX(4, 22) CX(4, 13) CX(14, 23) CX(5, 23) CX(5, 14) CX(15, 24)
    CX(6, 24) CX(6, 15) CX(7, 16) CX(7, 19) CX(13, 21) CX(15, 23) CX(7, 13) CX(7, 15)
    CX(1, 9) CX(3, 11) CX(5, 17) CX(11, 17) CX(9, 17) CX(4, 10) CX(6, 12) CX(7, 14) CX(4, 6)
    CX(4, 7) CX(12, 14) CX(10, 14) CX(6, 7) CX(10, 12) CX(6, 10) CX(6, 17) CX(12, 17)
    CX(7, 17) CX(7, 10) CX(12, 18) CX(7, 12) CX(10, 18) CX(12, 20) CX(10, 20) CX(10, 12)
    // END
    return v[12];
}

#undef CX

template <int N>
__device__ __forceinline__ uint32_t select(uint32_t (&v)[N]) {
    if constexpr (N == 9)
        return select9(v);
    else
        return select25(v);
}

template <typename T, int K>
__global__ __launch_bounds__(MEDIAN_THREADS) void median_kernel(MedianArgs a, uint32_t tiles_c,
                                                               uint32_t tiles) {
    constexpr int H = K / 2, LR = TR + 2 * H, LC = TC + 2 * H, N = K * K;
    __shared__ uint32_t key[LR * LC];
    __shared__ uint32_t wave_counts[WAVES][4];
    const T* in = (const T*)a.disp;
    T* out = (T*)a.out;
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    uint32_t n[4] = {0, 0, 0, 0};  // unchanged, changed, filled, invalid (wave-uniform)

    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // workgroup-uniform
        const int row0 = (int)(tile / tiles_c) * TR, col0 = (int)(tile % tiles_c) * TC;
        // the tile and its halo as keys; 0 outside the image
        for (int s = threadIdx.x; s < LR * LC; s += MEDIAN_THREADS) {
            const int r = row0 - H + s / LC, c = col0 - H + s % LC;
            const bool inside = r >= 0 && r < a.rows && c >= 0 && c < a.cols;
            key[s] = inside ? pixel_key(in[(size_t)r * a.cols + c], a.flags) : 0u;
        }
        __syncthreads();

#pragma unroll 1
        for (int k = 0; k < ROWS_PER_WAVE; ++k) {
            const int r = wave + k * WAVES, gr = row0 + r, gc = col0 + lane;
            const bool inside = gr < a.rows && gc < a.cols;
            // the window, row-major; its invalid slots padded low, high, low, ... in that order.
            // In vector arithmetic alone (a compare and a select per slot go through a lane mask
            // in scalar registers and its wait states: 5-6 % slower): a hole's
            // key is 0, so it only needs the pad's bits or-ed in.
            uint32_t v[N];
            uint32_t pad = PAD_LOW, valid = 0;
#pragma unroll
            for (int dy = 0; dy < K; ++dy) {
#pragma unroll
                for (int dx = 0; dx < K; ++dx) {
                    const uint32_t x = key[(r + dy) * LC + lane + dx];
                    const uint32_t one = x < 1u ? x : 1u;  // 0 for a hole, else 1
                    const uint32_t hole = one - 1u;        // all ones for a hole, else 0
                    v[dy * K + dx] = x | (pad & hole);
                    pad ^= hole;
                    valid += one;
                }
            }
            const uint32_t centre = key[(r + H) * LC + lane + H];
            const uint32_t med = select<N>(v);
            const bool was_valid = centre != 0u;
            const bool fill = !was_valid && a.fill_min > 0 && valid >= (uint32_t)a.fill_min;
            if (inside) {
                const size_t p = (size_t)gr * a.cols + gc;
                // (an invalid pixel that stays one keeps its own bits, a NaN's payload included)
                out[p] = (was_valid || fill) ? key_pixel<T>(med) : in[p];
            }
            n[0] += (uint32_t)__popcll(__ballot(inside && was_valid && med == centre));
            n[1] += (uint32_t)__popcll(__ballot(inside && was_valid && med != centre));
            n[2] += (uint32_t)__popcll(__ballot(inside && fill));
            n[3] += (uint32_t)__popcll(__ballot(inside && !was_valid && !fill));
        }
        __syncthreads();  // the next tile overwrites the keys
    }
    if (!a.counts) return;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) wave_counts[wave][c] = n[c];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += wave_counts[w][threadIdx.x];
        if (s) atomicAdd(&a.counts[threadIdx.x], s);
    }
}

template <typename T, int K>
hipError_t launch(const MedianArgs& a, hipStream_t st) {
    const uint32_t tiles_r = ((uint32_t)a.rows + TR - 1) / TR, tiles_c = ((uint32_t)a.cols + TC - 1) / TC;
    const uint32_t tiles = tiles_r * tiles_c;  // <= rows * cols < 2^31
    if (a.counts) {
        const hipError_t e = hipMemsetAsync(a.counts, 0, 4 * sizeof(uint32_t), st);
        if (e != hipSuccess) return e;
    }
    // every workgroup the same number of tiles but the last few, which take one fewer
    const uint32_t per = (tiles + MEDIAN_MAX_BLOCKS - 1) / MEDIAN_MAX_BLOCKS;
    const uint32_t blocks = (tiles + per - 1) / per;
    hipLaunchKernelGGL((median_kernel<T, K>), dim3(blocks), dim3(MEDIAN_THREADS), 0, st, a, tiles_c,
                       tiles);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_median(const MedianArgs& a, bool f32, int ksize, hipStream_t st) {
    if (ksize == 3) return f32 ? launch<float, 3>(a, st) : launch<int16_t, 3>(a, st);
    if (ksize == 5) return f32 ? launch<float, 5>(a, st) : launch<int16_t, 5>(a, st);
    return hipErrorInvalidValue;
}

}  // namespace bicos_hip
