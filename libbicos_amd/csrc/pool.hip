// pool.hip -- an image stack pooled by an integer factor (pool.hpp; the definition is
// include/bicos_c.h, "stack pooling", restated in numpy by tests/test_pool_api.py).
//
//   pool_kernel<T, S, WIDE>  a lane per four consecutive output pixels of one row of one plane.
//                        The stage reads every source byte once and writes 1 / S^2 of them, so it
//                        is bound by HBM: what matters is that a wave's loads are few, wide and
//                        contiguous. WIDE (the source view dword-aligned, pool_wide()): the lane's
//                        4 S source elements of a row come as S (u8) or 2 S (u16) dword loads from
//                        one dword-aligned address -- the compiler merges them up to dwordx4, which
//                        gfx950 serves from any dword boundary. u8 sums add the bytes of a masked
//                        dword with one v_sad_u8 against zero; u16 sums add the two halves. The
//                        four pixels go out as one dword (u8) or two (u16) where the output view
//                        is dword-aligned too (PoolArgs::dst_vector, the same in every lane), else
//                        as four elements: 1 / S^2 of the traffic, so no kernel of its own. Lanes
//                        that straddle the right edge, and every lane of WIDE = false, load and
//                        store element by element.
//                        S is a template parameter: the block is unrolled and the division by
//                        S * S is a multiply and a shift. All sums are uint32 and exact.
//
// Memory safety: a lane that passes the guard owns output pixels (R, C .. C+3) with R < prows and
// C < pcols. The WIDE body runs only for C + 4 <= pcols and then reads source rows S R .. S R+S-1
// (<= rows - 1, as prows = rows / S) and columns S C .. S C + 4 S - 1 (<= S pcols - 1 <= cols - 1),
// the per-element body reads the S x S block of each pixel with C + k < pcols: never a remainder
// row or column, never a byte between rows or planes. Stores go to pixels < (prows, pcols) only.
// In-plane offsets are 32-bit: the entries refuse a plane that spans more than 2^32 - 1 elements.
#include "pool.hpp"

namespace bicos_hip {
namespace {

constexpr int PX = POOL_PER_LANE;
constexpr int LANES_X = POOL_TILE_COLS / PX;
static_assert(POOL_TILE_ROWS * LANES_X == POOL_THREADS, "one lane per pixel group");
static_assert(PX == 4, "the vector stores below are four pixels wide");

// Of dword d of a lane's 4 S source bytes (u8), the bytes that belong to output pixel k: byte j
// of the run belongs to pixel j / S
constexpr uint32_t byte_mask(int S, int d, int k) {
    uint32_t m = 0;
    for (int b = 0; b < 4; ++b)
        if ((4 * d + b) / S == k) m |= 0xFFu << (8 * b);
    return m;
}

// One source row of the lane, DW dwords, added to the four sums
template <int S, int DW>
__device__ __forceinline__ void add_row(const uint8_t*, const uint32_t (&w)[DW], uint32_t (&acc)[PX]) {
#pragma unroll
    for (int d = 0; d < DW; ++d)
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const uint32_t m = byte_mask(S, d, k);
            if (m) acc[k] = __builtin_amdgcn_sad_u8(m == 0xFFFFFFFFu ? w[d] : (w[d] & m), 0u, acc[k]);
        }
}
template <int S, int DW>
__device__ __forceinline__ void add_row(const uint16_t*, const uint32_t (&w)[DW], uint32_t (&acc)[PX]) {
#pragma unroll
    for (int d = 0; d < DW; ++d) {
        acc[(2 * d) / S] += w[d] & 0xFFFFu;
        acc[(2 * d + 1) / S] += w[d] >> 16;
    }
}

__device__ __forceinline__ void store4(uint8_t* p, const uint32_t (&r)[PX]) {
    *(uint32_t*)p = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
}
__device__ __forceinline__ void store4(uint16_t* p, const uint32_t (&r)[PX]) {  // dword-aligned
    ((uint32_t*)p)[0] = r[0] | (r[1] << 16);
    ((uint32_t*)p)[1] = r[2] | (r[3] << 16);
}

template <typename T, int S, bool WIDE>
__global__ __launch_bounds__(POOL_THREADS) void pool_kernel(PoolArgs a) {
    constexpr int DW = PX * S * (int)sizeof(T) / 4;  // dwords of a lane's run of a source row
    constexpr uint32_t AREA = S * S;
    // the tile and the plane are the workgroup's: scalar arithmetic, a scalar plane base
    const uint32_t tiles_x = ((uint32_t)a.pcols + POOL_TILE_COLS - 1) / POOL_TILE_COLS;
    const uint32_t tiles_y = ((uint32_t)a.prows + POOL_TILE_ROWS - 1) / POOL_TILE_ROWS;
    const uint32_t plane = blockIdx.x / (tiles_x * tiles_y);
    const uint32_t tile = blockIdx.x - plane * (tiles_x * tiles_y);
    const uint32_t tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const T* src = (const T*)a.src + (size_t)plane * a.src_plane_pitch;
    T* dst = (T*)a.dst + (size_t)plane * a.dst_plane_pitch;

    const uint32_t C = tile_x * POOL_TILE_COLS + (threadIdx.x % LANES_X) * PX;
    const uint32_t R = tile_y * POOL_TILE_ROWS + threadIdx.x / LANES_X;
    if (R >= (uint32_t)a.prows || C >= (uint32_t)a.pcols) return;
    const uint32_t so = R * S * a.src_row_pitch + C * S;
    T* out = dst + (R * a.dst_row_pitch + C);

    if (WIDE && C + PX <= (uint32_t)a.pcols) {
        uint32_t acc[PX] = {0, 0, 0, 0};
        uint32_t w[S][DW];
#pragma unroll
        for (int y = 0; y < S; ++y) {
            const uint32_t* p = (const uint32_t*)(src + (so + (uint32_t)y * a.src_row_pitch));
#pragma unroll
            for (int d = 0; d < DW; ++d) w[y][d] = p[d];
        }
#pragma unroll
        for (int y = 0; y < S; ++y) add_row<S, DW>((const T*)nullptr, w[y], acc);
#pragma unroll
        for (int k = 0; k < PX; ++k) acc[k] = (acc[k] + AREA / 2) / AREA;
        if (a.dst_vector) {
            store4(out, acc);
        } else {
#pragma unroll
            for (int k = 0; k < PX; ++k) out[k] = (T)acc[k];
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        if (C + k >= (uint32_t)a.pcols) break;
        uint32_t sum = 0;
#pragma unroll
        for (int y = 0; y < S; ++y)
#pragma unroll
            for (int x = 0; x < S; ++x) sum += src[so + (uint32_t)y * a.src_row_pitch + k * S + x];
        out[k] = (T)((sum + AREA / 2) / AREA);
    }
}

template <typename T, int S>
void launch_scale(const PoolArgs& a, bool wide, dim3 grid, hipStream_t st) {
    if (wide)
        hipLaunchKernelGGL((pool_kernel<T, S, true>), grid, dim3(POOL_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((pool_kernel<T, S, false>), grid, dim3(POOL_THREADS), 0, st, a);
}

template <typename T>
void launch_depth(const PoolArgs& a, int scale, bool wide, dim3 grid, hipStream_t st) {
    switch (scale) {
        case 2: return launch_scale<T, 2>(a, wide, grid, st);
        case 3: return launch_scale<T, 3>(a, wide, grid, st);
        case 4: return launch_scale<T, 4>(a, wide, grid, st);
        case 5: return launch_scale<T, 5>(a, wide, grid, st);
        case 6: return launch_scale<T, 6>(a, wide, grid, st);
        case 7: return launch_scale<T, 7>(a, wide, grid, st);
        case 8: return launch_scale<T, 8>(a, wide, grid, st);
    }
}

}  // namespace

bool pool_wide(const PoolArgs& a, int depth) {
    const size_t d = (size_t)depth;
    return ((uintptr_t)a.src | (a.src_row_pitch * d) | (a.src_plane_pitch * d)) % 4 == 0;
}

bool pool_dst_vector(const PoolArgs& a, int depth) {
    const size_t d = (size_t)depth;
    return ((uintptr_t)a.dst | (a.dst_row_pitch * d) | (a.dst_plane_pitch * d)) % 4 == 0;
}

uint64_t pool_blocks(const PoolArgs& a) {
    const uint64_t tiles_x = ((uint64_t)a.pcols + POOL_TILE_COLS - 1) / POOL_TILE_COLS;
    const uint64_t tiles_y = ((uint64_t)a.prows + POOL_TILE_ROWS - 1) / POOL_TILE_ROWS;
    return tiles_x * tiles_y * (uint64_t)a.n;
}

hipError_t launch_pool(const PoolArgs& args, int depth, int scale, hipStream_t st) {
    if (scale < POOL_MIN_SCALE || scale > POOL_MAX_SCALE || (depth != 1 && depth != 2))
        return hipErrorInvalidValue;
    PoolArgs a = args;
    a.dst_vector = pool_dst_vector(a, depth);
    const dim3 grid((uint32_t)pool_blocks(a));
    if (depth == 1)
        launch_depth<uint8_t>(a, scale, pool_wide(a, depth), grid, st);
    else
        launch_depth<uint16_t>(a, scale, pool_wide(a, depth), grid, st);
    return hipGetLastError();
}

}  // namespace bicos_hip
