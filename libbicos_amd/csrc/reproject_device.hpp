// reproject_device.hpp -- the device code of the ordered point list, shared by reproject.hip and
// mesh.hip (whose vertices are that list): the pixel's class and point, the segment count, the
// scan of the segments, and the ranked write. Device code only, with internal linkage: include it
// from a .hip file, never from host code.
#pragma once

#include "reproject.hpp"

#include "../../include/bicos_c.h"

namespace bicos_hip {
namespace {

constexpr int WAVE = 64;
constexpr int WAVES = REPROJECT_THREADS / WAVE;
constexpr int SCAN_WAVES = REPROJECT_SCAN_THREADS / WAVE;
static_assert(REPROJECT_THREADS % WAVE == 0 && REPROJECT_SCAN_THREADS % WAVE == 0, "whole waves");

// the classes in the order of the counts
enum : int { KEPT = 0, INVALID = 1, NONFINITE = 2, NEGATIVE_Z = 3, OUTSIDE = 4 };

struct Point {
    float x, y, z;
};

__device__ __forceinline__ bool invalid_disparity(int16_t v, int) { return v == INT16_MIN; }
__device__ __forceinline__ bool invalid_disparity(float v, int flags) {
    return v != v || ((flags & BICOS_REPROJECT_F32_SENTINEL) && v == -32768.0f);
}

// The class of pixel idx and, where it is KEPT, its point (three NaNs otherwise).
template <typename T>
__device__ __forceinline__ int reproject_pixel(const ReprojectArgs& a, uint32_t idx, Point& p) {
#pragma clang fp contract(off)
    const float nan = __builtin_nanf("");
    p = Point{nan, nan, nan};
    if (idx >= a.pixels) return OUTSIDE;
    const T v = ((const T*)a.disp)[idx];
    if (invalid_disparity(v, a.flags)) return INVALID;
    const uint32_t row = idx / (uint32_t)a.cols;
    const double x = (double)(idx - row * (uint32_t)a.cols), y = (double)row, d = (double)v;
    const double* Q = a.Q.q;
    double o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        o[i] = ((Q[4 * i] * x + Q[4 * i + 1] * y) + Q[4 * i + 2] * d) + Q[4 * i + 3];
    const double iw = 1.0 / o[3];
    const float X = (float)(o[0] * iw), Y = (float)(o[1] * iw), Z = (float)(o[2] * iw);
    if (!__builtin_isfinite(X) || !__builtin_isfinite(Y) || !__builtin_isfinite(Z))
        return NONFINITE;
    if (!(a.flags & BICOS_REPROJECT_ALLOW_NEGATIVE_Z) && Z < 0.0f) return NEGATIVE_Z;
    p = Point{X, Y, Z};
    return KEPT;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

template <typename T>
__global__ __launch_bounds__(REPROJECT_THREADS) void reproject_count_kernel(ReprojectArgs a) {
    __shared__ uint32_t wave_counts[WAVES][4];
    const uint32_t first = blockIdx.x * (uint32_t)REPROJECT_SEGMENT + threadIdx.x;
    uint32_t n[4] = {0, 0, 0, 0};  // wave-uniform
#pragma unroll
    for (int k = 0; k < REPROJECT_PER_LANE; ++k) {
        Point p;
        const int cls = reproject_pixel<T>(a, first + k * REPROJECT_THREADS, p);
#pragma unroll
        for (int c = 0; c < 4; ++c) n[c] += (uint32_t)__popcll(__ballot(cls == c));
    }
    if (threadIdx.x % WAVE == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) wave_counts[threadIdx.x / WAVE][c] = n[c];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += wave_counts[w][threadIdx.x];
        a.seg_counts[(size_t)blockIdx.x * 4 + threadIdx.x] = s;
    }
}

// One workgroup over all segments, REPROJECT_SCAN_THREADS at a time with a running carry: the
// exclusive scan of the segments' first counts into seg_offsets, and the four totals into counts.
__global__ __launch_bounds__(REPROJECT_SCAN_THREADS) void reproject_scan_kernel(
    const uint32_t* __restrict__ seg_counts, uint32_t* __restrict__ seg_offsets, uint32_t segments,
    uint32_t* __restrict__ counts) {
    __shared__ uint32_t wave_total[SCAN_WAVES];
    __shared__ uint32_t wave_others[SCAN_WAVES][3];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    uint32_t carry = 0;               // kept points of the chunks before this one
    uint32_t others[3] = {0, 0, 0};   // this lane's share of invalid, nonfinite, negative_z
    for (uint32_t base = 0; base < segments; base += REPROJECT_SCAN_THREADS) {
        const uint32_t i = base + threadIdx.x;
        uint4 c = make_uint4(0, 0, 0, 0);
        if (i < segments) c = ((const uint4*)seg_counts)[i];
        others[0] += c.y;
        others[1] += c.z;
        others[2] += c.w;
        uint32_t incl = c.x;  // inclusive scan within the wave
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == WAVE - 1) wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SCAN_WAVES; ++w) {
            const uint32_t t = wave_total[w];
            if (w < wave) before += t;
            total += t;
        }
        if (i < segments) seg_offsets[i] = carry + before + incl - c.x;
        carry += total;
        __syncthreads();  // wave_total is rewritten by the next chunk
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int d = WAVE / 2; d > 0; d >>= 1) others[k] += __shfl_down(others[k], d);
        if (lane == 0) wave_others[wave][k] = others[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t s = carry;
        if (threadIdx.x > 0) {
            s = 0;
            for (int w = 0; w < SCAN_WAVES; ++w) s += wave_others[w][threadIdx.x - 1];
        }
        counts[threadIdx.x] = s;
    }
}

// DENSE: the [pixels][3] map. LIST: the compacted points (and their pixel indices). RANK (with
// LIST): every pixel's position in the full list, or -1 where it is not kept, into rank[pixels]:
// one dense store per pixel.
template <typename T, bool LIST, bool DENSE, bool RANK = false>
__global__ __launch_bounds__(REPROJECT_THREADS) void reproject_write_kernel(ReprojectArgs a,
                                                                            int32_t* rank) {
    static_assert(LIST || !RANK, "ranks are positions in the list");
    __shared__ uint32_t wave_kept[REPROJECT_PER_LANE][WAVES];
    const uint32_t first = blockIdx.x * (uint32_t)REPROJECT_SEGMENT + threadIdx.x;
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    Point p[REPROJECT_PER_LANE];
    uint64_t kept[REPROJECT_PER_LANE];  // the wave's kept lanes of each step (uniform)
#pragma unroll
    for (int k = 0; k < REPROJECT_PER_LANE; ++k) {
        const uint32_t idx = first + k * REPROJECT_THREADS;
        const int cls = reproject_pixel<T>(a, idx, p[k]);
        if (DENSE && cls != OUTSIDE) ((Point*)a.xyz_map)[idx] = p[k];
        if (LIST) {
            kept[k] = __ballot(cls == KEPT);
            if (lane == 0) wave_kept[k][wave] = (uint32_t)__popcll(kept[k]);
        }
    }
    if (!LIST) return;
    __syncthreads();
    // pixel order within the segment: step k, then wave, then lane
    uint32_t at = a.seg_offsets[blockIdx.x];
#pragma unroll
    for (int k = 0; k < REPROJECT_PER_LANE; ++k) {
        uint32_t mine = at;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t t = wave_kept[k][w];
            if (w < wave) mine += t;
            at += t;
        }
        const uint32_t idx = first + k * REPROJECT_THREADS;
        const uint32_t pos = mine + lanes_below(kept[k]);
        const bool is_kept = (kept[k] >> lane) & 1;
        if (is_kept && pos < a.capacity) {
            ((Point*)a.points)[pos] = p[k];
            if (a.index) a.index[pos] = (int32_t)idx;
        }
        if (RANK && idx < a.pixels) rank[idx] = is_kept ? (int32_t)pos : -1;
    }
}

}  // namespace
}  // namespace bicos_hip
