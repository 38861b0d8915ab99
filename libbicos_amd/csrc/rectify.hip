// rectify.hip -- raw image stacks -> rectified stacks (rectify.hpp; the definition is
// include/bicos_c.h, "rectification", restated in numpy by tests/rectify_ref.py).
//
//   rectify_maps_kernel  a lane per output pixel: the camera model in IEEE double, operation for
//                        operation as the header writes it (no contraction: -ffp-contract=off and
//                        the pragma below). Runs once per rig.
//   rectify_kernel<T>    the remap of a stack through one pair of maps. Everything that depends
//                        on the maps alone -- the four clamped tap offsets, the two fractions, the
//                        taps' in-image bits, valid -- is computed once per pixel and kept in
//                        registers; the loop over the n planes then only loads the taps from a
//                        wave-uniform plane base, blends and stores. The kernel is bound by the
//                        number of gather instructions, not by bytes, so the two
//                        taps of a source row come in ONE unaligned load (PAIR; 2 bytes for u8, 4
//                        for u16) and are picked apart by per-pixel shifts: two loads per pixel
//                        and plane instead of four. PAIR = false, four single loads, remains for
//                        sources of one column.
//
// Memory safety of the remap: every tap address is y*row_pitch + x with 0 <= x < src_cols and
// 0 <= y < src_rows after the clamps below (a pair starts at x <= src_cols - 2), whatever the
// maps hold (NaN, infinities and huge values are "not inside" and address element 0); the loads
// are unguarded, the border is selected afterwards. Stores go to (v, u) with v < rows and
// u < cols only.
#include "rectify.hpp"

namespace bicos_hip {
namespace {

constexpr int PX = RECTIFY_PER_LANE;
constexpr int LANES_X = RECTIFY_TILE_COLS / PX;
static_assert(RECTIFY_TILE_ROWS * LANES_X == RECTIFY_THREADS, "one lane per pixel group");
static_assert(PX == 4, "the vector stores below are four pixels wide");

__device__ __forceinline__ void store4(uint8_t* p, const uint32_t (&r)[PX]) {
    *(uint32_t*)p = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
}
__device__ __forceinline__ void store4(uint16_t* p, const uint32_t (&r)[PX]) {
    *(uint2*)p = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
}

// The two taps of one source row in one load: 2 bytes at any address (u8), 4 bytes at an even one
// (u16). gfx950 serves unaligned global loads in hardware.
typedef uint16_t __attribute__((aligned(1))) pair_u8;
typedef uint32_t __attribute__((aligned(2))) pair_u16;
__device__ __forceinline__ uint32_t load_pair(const uint8_t* p) { return *(const pair_u8*)p; }
__device__ __forceinline__ uint32_t load_pair(const uint16_t* p) { return *(const pair_u16*)p; }

template <typename T, bool PAIR>
__global__ __launch_bounds__(RECTIFY_THREADS) void rectify_kernel(RectifyArgs a) {
#pragma clang fp contract(off)
    const uint32_t tiles_x = ((uint32_t)a.cols + RECTIFY_TILE_COLS - 1) / RECTIFY_TILE_COLS;
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int u0 = (int)(tile_x * RECTIFY_TILE_COLS + (threadIdx.x % LANES_X) * PX);
    const int v = (int)(tile_y * RECTIFY_TILE_ROWS + threadIdx.x / LANES_X);
    if (v >= a.rows || u0 >= a.cols) return;
    const bool full = u0 + PX <= a.cols;

    float fx[PX], fy[PX];
    uint32_t o00[PX], o01[PX], o10[PX], o11[PX];
    uint32_t in[PX];  // bit 0..3: tap 00, 01, 10, 11 lies in the image
    uint32_t ok[PX];  // valid
    uint32_t sh[PX];  // PAIR: the bit offsets of tap x0 (bits 0..7) and x0 + 1 (8..15) in a pair
    constexpr uint32_t BITS = 8 * sizeof(T);
    const float* mx = a.map_x + (size_t)v * a.map_pitch;
    const float* my = a.map_y + (size_t)v * a.map_pitch;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        float x = __builtin_nanf(""), y = x;  // a pixel past the row's end: not inside
        if (u0 + k < a.cols) {
            x = mx[u0 + k];
            y = my[u0 + k];
        }
        const bool inside =
            x > -1.0f && x < (float)a.src_cols && y > -1.0f && y < (float)a.src_rows;
        const float xs = inside ? x : 0.0f, ys = inside ? y : 0.0f;
        const float xf = floorf(xs), yf = floorf(ys);
        fx[k] = xs - xf;
        fy[k] = ys - yf;
        const int x0 = (int)xf, y0 = (int)yf, x1 = x0 + 1, y1 = y0 + 1;  // x0, y0 >= -1
        const bool cx0 = x0 >= 0 && x0 < a.src_cols, cx1 = x1 < a.src_cols;
        const bool ry0 = y0 >= 0 && y0 < a.src_rows, ry1 = y1 < a.src_rows;
        in[k] = inside ? ((ry0 && cx0) ? 1u : 0u) | ((ry0 && cx1) ? 2u : 0u) |
                             ((ry1 && cx0) ? 4u : 0u) | ((ry1 && cx1) ? 8u : 0u)
                       : 0u;
        ok[k] = (inside && cx0 && ry0 && (fx[k] == 0.0f || cx1) && (fy[k] == 0.0f || ry1)) ? 1u : 0u;
        const uint32_t xa = (uint32_t)min(max(x0, 0), a.src_cols - 1);
        const uint32_t xb = (uint32_t)min(max(x1, 0), a.src_cols - 1);
        const uint32_t ya = (uint32_t)min(max(y0, 0), a.src_rows - 1) * a.src_row_pitch;
        const uint32_t yb = (uint32_t)min(max(y1, 0), a.src_rows - 1) * a.src_row_pitch;
        if (PAIR) {
            // the pair starts at xp with xp, xp + 1 both in the row (src_cols >= 2); a tap that
            // is not in the pair (x0 = -1, x0 + 1 = src_cols) is not in the image either
            const int xp = min(max(x0, 0), a.src_cols - 2);
            sh[k] = (x0 > xp ? BITS : 0u) | ((x0 < xp ? 0u : BITS) << 8);
            o00[k] = ya + (uint32_t)xp;
            o10[k] = yb + (uint32_t)xp;
            continue;
        }
        o00[k] = ya + xa;
        o01[k] = ya + xb;
        o10[k] = yb + xa;
        o11[k] = yb + xb;
    }
    if (a.valid) {
        uint8_t* vp = a.valid + (size_t)v * (uint32_t)a.cols + u0;
        if (full && a.valid_vector) {
            store4(vp, ok);
        } else {
#pragma unroll
            for (int k = 0; k < PX; ++k)
                if (u0 + k < a.cols) vp[k] = (uint8_t)ok[k];
        }
    }

    const float border = (float)a.border;
    const float top_level = sizeof(T) == 1 ? 255.0f : 65535.0f;
    const T* sp = (const T*)a.src;  // wave-uniform
    T* dp = (T*)a.dst + (size_t)v * a.dst_row_pitch + u0;
    const bool vec = full && a.dst_vector;
    for (int t = 0; t < a.n; ++t, sp += a.src_plane_pitch, dp += a.dst_plane_pitch) {
        uint32_t r[PX];
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            float l00, l01, l10, l11;
            if (PAIR) {
                constexpr uint32_t MASK = (1u << BITS) - 1;
                const uint32_t w0 = load_pair(sp + o00[k]), w1 = load_pair(sp + o10[k]);
                const uint32_t s0 = sh[k] & 0xFFu, s1 = sh[k] >> 8;
                l00 = (float)((w0 >> s0) & MASK);
                l01 = (float)((w0 >> s1) & MASK);
                l10 = (float)((w1 >> s0) & MASK);
                l11 = (float)((w1 >> s1) & MASK);
            } else {
                l00 = (float)sp[o00[k]];
                l01 = (float)sp[o01[k]];
                l10 = (float)sp[o10[k]];
                l11 = (float)sp[o11[k]];
            }
            const float p00 = (in[k] & 1u) ? l00 : border, p01 = (in[k] & 2u) ? l01 : border;
            const float p10 = (in[k] & 4u) ? l10 : border, p11 = (in[k] & 8u) ? l11 : border;
            const float top = p00 + fx[k] * (p01 - p00);
            const float bot = p10 + fx[k] * (p11 - p10);
            const float val = top + fy[k] * (bot - top);
            r[k] = (uint32_t)fminf(fmaxf(rintf(val), 0.0f), top_level);
        }
        if (vec) {
            store4(dp, r);
        } else {
#pragma unroll
            for (int k = 0; k < PX; ++k)
                if (u0 + k < a.cols) dp[k] = (T)r[k];
        }
    }
}

__global__ __launch_bounds__(RECTIFY_MAPS_THREADS) void rectify_maps_kernel(
    RectifyCamera c, int cols, uint32_t pixels, float* __restrict__ map_x,
    float* __restrict__ map_y) {
#pragma clang fp contract(off)
    const uint32_t idx = blockIdx.x * (uint32_t)RECTIFY_MAPS_THREADS + threadIdx.x;
    if (idx >= pixels) return;
    const uint32_t row = idx / (uint32_t)cols;
    const double u = (double)(idx - row * (uint32_t)cols), v = (double)row;
    const double X = (c.iM[0] * u + c.iM[1] * v) + c.iM[2];
    const double Y = (c.iM[3] * u + c.iM[4] * v) + c.iM[5];
    const double W = (c.iM[6] * u + c.iM[7] * v) + c.iM[8];
    const double x = X / W, y = Y / W;
    const double r2 = x * x + y * y;
    const double kr = (1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2) /
                      (1.0 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2);
    const double xd = (x * kr + c.p1 * ((2.0 * x) * y)) + c.p2 * (r2 + (2.0 * x) * x);
    const double yd = (y * kr + c.p1 * (r2 + (2.0 * y) * y)) + c.p2 * ((2.0 * x) * y);
    map_x[idx] = (float)(c.fx * xd + c.cx);
    map_y[idx] = (float)(c.fy * yd + c.cy);
}

}  // namespace

hipError_t launch_rectify(const RectifyArgs& a, int depth, hipStream_t st) {
    const uint32_t tiles_x = ((uint32_t)a.cols + RECTIFY_TILE_COLS - 1) / RECTIFY_TILE_COLS;
    const uint32_t tiles_y = ((uint32_t)a.rows + RECTIFY_TILE_ROWS - 1) / RECTIFY_TILE_ROWS;
    const dim3 grid(tiles_x * tiles_y), block(RECTIFY_THREADS);
    const bool pair = a.src_cols >= 2;  // a source of one column has no pair to load
    if (depth == 1) {
        if (pair)
            hipLaunchKernelGGL((rectify_kernel<uint8_t, true>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((rectify_kernel<uint8_t, false>), grid, block, 0, st, a);
    } else {
        if (pair)
            hipLaunchKernelGGL((rectify_kernel<uint16_t, true>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((rectify_kernel<uint16_t, false>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_rectify_maps(const RectifyCamera& c, int rows, int cols, float* map_x,
                               float* map_y, hipStream_t st) {
    const uint32_t pixels = (uint32_t)rows * (uint32_t)cols;
    const uint32_t blocks = (pixels + RECTIFY_MAPS_THREADS - 1) / RECTIFY_MAPS_THREADS;
    hipLaunchKernelGGL(rectify_maps_kernel, dim3(blocks), dim3(RECTIFY_MAPS_THREADS), 0, st, c,
                       cols, pixels, map_x, map_y);
    return hipGetLastError();
}

}  // namespace bicos_hip
