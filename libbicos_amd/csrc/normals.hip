// normals.hip -- unit surface normals from a disparity map and Q (normals.hpp; the definition
// is include/bicos_c.h, "surface normals"): per pixel the least-squares plane
// e = a*du + b*dv + c of the disparity differences over a (2*radius+1)^2 window in (column,
// row, disparity), three points of it carried through Q, their cross product turned towards
// the origin and normalised. The arithmetic is the definition's, operation for operation in
// IEEE double without contraction (-ffp-contract=off), so the float32 normals are those of a
// float64 CPU evaluation bit for bit.
//
// STAGING. Both map types become float32 with NaN for an invalid pixel (int16 -32768; float NaN,
// and -32768.0f under the sentinel flag) and for a pixel outside the image: int16 -> float32 ->
// double is exact, and a NaN fails the membership test fabsf(dq - dp) <= max_diff by itself, so
// "valid and linked" is one float subtraction and one compare.
//
// NON-MEMBERS ADD ZERO. The double sums run over the whole window without a branch: a
// non-member's e is replaced by +0.0. That leaves the bits of the definition's sums, which
// skip it: a sum that starts at +0.0 is never -0.0 (x + y is -0.0 only for x = y = -0.0 under
// round-to-nearest), and s + (+-0.0) = s for every other s, NaN and infinities included.
//
// Dense map: one launch; the tile and its halo in LDS, a lane per pixel. List: one launch, a
// lane per entry, the window through the cache.
//
// COUNTS. As median.hip: ballots per wave in wave-uniform registers over all of the workgroup's
// tiles, summed over the waves in LDS, one atomic instruction per class and workgroup. Integer
// sums; no workgroup reads what another writes.
#include "normals.hpp"

#include "../../include/bicos_c.h"

namespace bicos_hip {
namespace {

constexpr int WAVE = 64;
constexpr int TR = NORMALS_TILE_ROWS, TC = NORMALS_TILE_COLS;
constexpr int WAVES = NORMALS_THREADS / WAVE;
constexpr int ROWS_PER_WAVE = TR / WAVES;
static_assert(TC == WAVE, "a wave owns a tile row");
static_assert(NORMALS_THREADS % WAVE == 0 && TR % WAVES == 0, "whole waves, whole rows");

// the classes in the order of the counts
enum : int { NORMAL = 0, NO_POINT = 1, SPARSE = 2, DEGENERATE = 3 };

struct Vec3f {
    float x, y, z;
};

// the staged value of a pixel: its disparity, NaN where it is invalid
__device__ __forceinline__ float staged(int16_t v, int) {
    return v == INT16_MIN ? __builtin_nanf("") : (float)v;
}
__device__ __forceinline__ float staged(float v, int flags) {
    return ((flags & BICOS_NORMALS_F32_SENTINEL) && v == -32768.0f) ? __builtin_nanf("") : v;
}

// reproj of the definition: (x, y, d) through Q, divided by the fourth row
__device__ __forceinline__ void reproj(const double* Q, double x, double y, double d,
                                       double (&p)[3]) {
#pragma clang fp contract(off)
    double o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        o[i] = ((Q[4 * i] * x + Q[4 * i + 1] * y) + Q[4 * i + 2] * d) + Q[4 * i + 3];
    const double iw = 1.0 / o[3];
    p[0] = o[0] * iw;
    p[1] = o[1] * iw;
    p[2] = o[2] * iw;
}

// The class of pixel (row y, column x) and, where it is NORMAL, its normal (three NaNs
// otherwise). fetch(dv, du) is the staged value of pixel (y + dv, x + du), NaN outside the image.
template <int R, typename Fetch>
__device__ __forceinline__ int normal_pixel(const NormalsArgs& a, int x, int y, Fetch fetch,
                                            Vec3f& n) {
#pragma clang fp contract(off)
    const float nan = __builtin_nanf("");
    n = Vec3f{nan, nan, nan};
    const double* Q = a.Q.q;
    // 1. the pixel's own point, as reproject keeps or drops it
    const float fp = fetch(0, 0);
    if (fp != fp) return NO_POINT;
    const double xd = (double)x, yd = (double)y, dp = (double)fp;
    {
        double P[3];
        reproj(Q, xd, yd, dp, P);
        const float X = (float)P[0], Y = (float)P[1], Z = (float)P[2];
        if (!__builtin_isfinite(X) || !__builtin_isfinite(Y) || !__builtin_isfinite(Z))
            return NO_POINT;
        if (!(a.flags & BICOS_NORMALS_ALLOW_NEGATIVE_Z) && Z < 0.0f) return NO_POINT;
    }
    // 2., 3. members and sums, in row-major window order
    int m = 0, Su = 0, Sv = 0, Suu = 0, Suv = 0, Svv = 0;
    double Sd = 0.0, Sud = 0.0, Svd = 0.0;
#pragma unroll
    for (int dv = -R; dv <= R; ++dv) {
#pragma unroll
        for (int du = -R; du <= R; ++du) {
            const float fq = fetch(dv, du);
            const bool member = __builtin_fabsf(fq - fp) <= a.max_diff;  // false for NaN
            const int k = member ? 1 : 0;
            m += k;
            Su += k * du;
            Sv += k * dv;
            Suu += k * (du * du);
            Suv += k * (du * dv);
            Svv += k * (dv * dv);
            const double e = member ? (double)fq - dp : 0.0;
            Sd = Sd + e;
            Sud = Sud + (double)du * e;
            Svd = Svd + (double)dv * e;
        }
    }
    // 4. sparse
    if (m < a.min_points) return SPARSE;
    // 5. the adjugate and determinant of the normal equations, in integers (all below 2^31)
    const int C00 = Svv * m - Sv * Sv;
    const int C01 = Su * Sv - Suv * m;
    const int C02 = Suv * Sv - Svv * Su;
    const int C11 = Suu * m - Su * Su;
    const int C12 = Suv * Su - Suu * Sv;
    const int C22 = Suu * Svv - Suv * Suv;
    const int det = Suu * C00 + Suv * C01 + Su * C02;
    if (det == 0) return DEGENERATE;
    // 6. the plane
    const double c00 = (double)C00, c01 = (double)C01, c02 = (double)C02, c11 = (double)C11,
                 c12 = (double)C12, c22 = (double)C22, dt = (double)det;
    const double pa = ((c00 * Sud + c01 * Svd) + c02 * Sd) / dt;
    const double pb = ((c01 * Sud + c11 * Svd) + c12 * Sd) / dt;
    const double pc = ((c02 * Sud + c12 * Svd) + c22 * Sd) / dt;
    // 7. three points of it in 3-D, and their cross product turned towards the origin
    const double d0 = dp + pc;
    double P0[3], P1[3], P2[3];
    reproj(Q, xd, yd, d0, P0);
    reproj(Q, xd + 1.0, yd, d0 + pa, P1);
    reproj(Q, xd, yd + 1.0, d0 + pb, P2);
    const double Ux = P1[0] - P0[0], Uy = P1[1] - P0[1], Uz = P1[2] - P0[2];
    const double Vx = P2[0] - P0[0], Vy = P2[1] - P0[1], Vz = P2[2] - P0[2];
    double Nx = Uy * Vz - Uz * Vy, Ny = Uz * Vx - Ux * Vz, Nz = Ux * Vy - Uy * Vx;
    if ((Nx * P0[0] + Ny * P0[1]) + Nz * P0[2] > 0) {
        Nx = -Nx;
        Ny = -Ny;
        Nz = -Nz;
    }
    // 8., 9. its length and the unit normal
    const double L = __builtin_sqrt((Nx * Nx + Ny * Ny) + Nz * Nz);
    if (L == 0 || !__builtin_isfinite(L)) return DEGENERATE;
    n = Vec3f{(float)(Nx / L), (float)(Ny / L), (float)(Nz / L)};
    return NORMAL;
}

template <typename T, int R>
__global__ __launch_bounds__(NORMALS_THREADS) void normals_map_kernel(NormalsArgs a,
                                                                      uint32_t tiles_c,
                                                                      uint32_t tiles) {
    constexpr int LR = TR + 2 * R, LC = TC + 2 * R;
    __shared__ float val[LR * LC];
    __shared__ uint32_t wave_counts[WAVES][4];
    const T* in = (const T*)a.disp;
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    uint32_t n[4] = {0, 0, 0, 0};  // normal, no_point, sparse, degenerate (wave-uniform)

    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // workgroup-uniform
        const int row0 = (int)(tile / tiles_c) * TR, col0 = (int)(tile % tiles_c) * TC;
        // the tile and its halo as staged values; NaN outside the image
        for (int s = threadIdx.x; s < LR * LC; s += NORMALS_THREADS) {
            const int r = row0 - R + s / LC, c = col0 - R + s % LC;
            const bool inside = r >= 0 && r < a.rows && c >= 0 && c < a.cols;
            val[s] = inside ? staged(in[(size_t)r * a.cols + c], a.flags) : __builtin_nanf("");
        }
        __syncthreads();

#pragma unroll 1
        for (int k = 0; k < ROWS_PER_WAVE; ++k) {
            const int r = wave + k * WAVES, gr = row0 + r, gc = col0 + lane;
            const bool inside = gr < a.rows && gc < a.cols;
            const float* centre = &val[(r + R) * LC + lane + R];
            Vec3f nv;
            // (a pixel outside the image has a NaN centre: NO_POINT at once, counted nowhere)
            const int cls = normal_pixel<R>(
                a, gc, gr, [centre](int dv, int du) { return centre[dv * LC + du]; }, nv);
            if (inside) ((Vec3f*)a.normal_map)[(size_t)gr * a.cols + gc] = nv;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                n[c] += (uint32_t)__popcll(__ballot(inside && cls == c));
        }
        __syncthreads();  // the next tile overwrites the staged values
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

template <typename T, int R>
__global__ __launch_bounds__(NORMALS_LIST_THREADS) void normals_list_kernel(NormalsArgs a) {
    const T* in = (const T*)a.disp;
    const uint32_t pixels = (uint32_t)a.rows * (uint32_t)a.cols;
    const size_t stride = (size_t)gridDim.x * NORMALS_LIST_THREADS;
    for (size_t i = (size_t)blockIdx.x * NORMALS_LIST_THREADS + threadIdx.x; i < a.count;
         i += stride) {
        const int32_t idx = a.index[i];
        const float nan = __builtin_nanf("");
        Vec3f nv{nan, nan, nan};
        if (idx >= 0 && (uint32_t)idx < pixels) {  // anything else reads nothing
            const int y = (int)((uint32_t)idx / (uint32_t)a.cols), x = idx - y * a.cols;
            normal_pixel<R>(
                a, x, y,
                [&](int dv, int du) {
                    const int r = y + dv, c = x + du;
                    const bool inside = r >= 0 && r < a.rows && c >= 0 && c < a.cols;
                    return inside ? staged(in[(size_t)r * a.cols + c], a.flags) : nan;
                },
                nv);
        }
        ((Vec3f*)a.normals)[i] = nv;
    }
}

template <typename T, int R>
hipError_t launch_map(const NormalsArgs& a, hipStream_t st) {
    const uint32_t tiles_r = ((uint32_t)a.rows + TR - 1) / TR, tiles_c = ((uint32_t)a.cols + TC - 1) / TC;
    const uint32_t tiles = tiles_r * tiles_c;  // <= rows * cols < 2^31
    if (a.counts) {
        const hipError_t e = hipMemsetAsync(a.counts, 0, 4 * sizeof(uint32_t), st);
        if (e != hipSuccess) return e;
    }
    // every workgroup the same number of tiles but the last few, which take one fewer
    const uint32_t per = (tiles + NORMALS_MAX_BLOCKS - 1) / NORMALS_MAX_BLOCKS;
    const uint32_t blocks = (tiles + per - 1) / per;
    hipLaunchKernelGGL((normals_map_kernel<T, R>), dim3(blocks), dim3(NORMALS_THREADS), 0, st, a,
                       tiles_c, tiles);
    return hipGetLastError();
}

template <typename T, int R>
hipError_t launch_list(const NormalsArgs& a, hipStream_t st) {
    const size_t want = (a.count + NORMALS_LIST_THREADS - 1) / NORMALS_LIST_THREADS;
    const uint32_t blocks = (uint32_t)(want < (size_t)NORMALS_LIST_MAX_BLOCKS
                                           ? want
                                           : (size_t)NORMALS_LIST_MAX_BLOCKS);
    hipLaunchKernelGGL((normals_list_kernel<T, R>), dim3(blocks), dim3(NORMALS_LIST_THREADS), 0,
                       st, a);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_map_r(const NormalsArgs& a, hipStream_t st) {
    switch (a.radius) {
        case 1: return launch_map<T, 1>(a, st);
        case 2: return launch_map<T, 2>(a, st);
        case 3: return launch_map<T, 3>(a, st);
        case 4: return launch_map<T, 4>(a, st);
    }
    return hipErrorInvalidValue;
}

template <typename T>
hipError_t launch_list_r(const NormalsArgs& a, hipStream_t st) {
    switch (a.radius) {
        case 1: return launch_list<T, 1>(a, st);
        case 2: return launch_list<T, 2>(a, st);
        case 3: return launch_list<T, 3>(a, st);
        case 4: return launch_list<T, 4>(a, st);
    }
    return hipErrorInvalidValue;
}
static_assert(NORMALS_MAX_RADIUS == 4, "the radius switches above");

}  // namespace

hipError_t launch_normals_map(const NormalsArgs& a, bool f32, hipStream_t st) {
    return f32 ? launch_map_r<float>(a, st) : launch_map_r<int16_t>(a, st);
}

hipError_t launch_normals_list(const NormalsArgs& a, bool f32, hipStream_t st) {
    return f32 ? launch_list_r<float>(a, st) : launch_list_r<int16_t>(a, st);
}

}  // namespace bicos_hip
