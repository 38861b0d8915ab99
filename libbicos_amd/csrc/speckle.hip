// speckle.hip -- the speckle filter of a disparity map (speckle.hpp; the definition is
// include/bicos_c.h, "speckle filter"): connected-component labelling by union-find over the
// whole frame, the component sizes, and the removal of every component of at most max_size
// pixels. Four launches on one stream; what one needs from another crosses a kernel boundary.
//
//   speckle_tile_kernel     one workgroup per 32 x 64 tile, in LDS. A wave owns a row: the
//                           row's runs of linked pixels come from one ballot, every pixel
//                           starts with its run's first pixel as label, and only the down
//                           links that are not implied by the pair to their left are united
//                           (LDS atomicMin union-find). Out: label[p] = the tile-local root as
//                           a global index (-1 for an invalid pixel), sizes[p] = the tile-local
//                           component size at a tile-local root and 0 elsewhere (counted in
//                           LDS, one LDS add per run).
//   speckle_border_kernel   a lane per link that crosses a tile border, united on the global
//                           label array. A crossing link is skipped where the same crossing one
//                           pixel before it along the border, in the same tile, is linked and
//                           the two links that close the square hold: those two lie inside
//                           tiles (united by the first launch) and the earlier crossing is
//                           united here or skipped by the same rule, so by induction along the
//                           border the connectivity is unchanged. (The rule never looks across
//                           a tile corner, where two skips could rely on each other.)
//   speckle_resolve_kernel  every tile-local root (sizes > 0) finds its global root, stores it
//                           as its label and, if it is not that root, adds its size to the
//                           root's: the workgroup's (root, size) pairs are gathered in LDS and
//                           summed per root within a wave first, so a frame-sized component
//                           costs one add per workgroup, not one per tile.
//   speckle_apply_kernel    per pixel: root (two hops: its tile-local root's label, which
//                           the resolve launch made the global root), size, verdict; out,
//                           labels, counts (ballots per wave, LDS per workgroup, one atomic
//                           instruction per workgroup).
//
// EXACT AND DETERMINISTIC. A label is only ever replaced by a smaller index of a pixel that
// is linked to it through united links (atomicMin(&L[a], b) with a, b roots of two linked
// pixels' trees), so at every moment L[x] <= x, the trees are forests inside the components,
// and when the launches are done each component is one tree whose root is the only pixel
// with L[x] == x: the component's smallest index, whatever order the atomics arrived in
// (the standard argument for atomicMin union-find, e.g. Komura 2015; Playne and Hawick 2018).
// Sizes are sums of integers, each tile-local size added exactly once to its global root
// (a global root is the smallest index of its component, hence of its tile-local component,
// hence a tile-local root, so only slots with sizes > 0 ever receive an add and "sizes > 0"
// names the tile-local roots throughout the resolve launch). Integer addition commutes.
// The map is copied bits or the invalid value. Nothing depends on arrival order.
//
// NO LOOP CAN HANG. find(x) replaces x by L[x] while L[x] != x; L[x] <= x always (labels start
// at or below their own index and atomicMin / the resolve store only lower them), so x
// decreases strictly and is bounded by 0. A stale or racing read returns a former value of
// L[x], still < x or == x. union(a, b) carries max(a, b): after the finds a' <= a, b' <= b;
// it ends if they are equal; else with a' > b' it runs old = atomicMin(&L[a'], b'), ends if
// old == a' and continues with (old, b') where old < a' (old is a value of L[a'], not a'), so
// the maximum has decreased strictly. No loop waits for another lane, wave or workgroup:
// there are no flags, no spin-waits and no protocol inside a launch.
//
// VISIBILITY. The per-XCD L2s are not coherent and a plain load may be served stale within a
// launch, so in the border launch the label array is touched only by agent-scope atomic
// loads and atomic mins. In the resolve launch a plain load that races with another lane's
// store of a root reads the old parent or the new one, both ancestors: the find ends at the
// same root, which no one writes. In the apply launch a lane writes only its own pixel's
// label, with the value a tile-local root already holds.
#include "speckle.hpp"

#include "../../include/bicos_c.h"

namespace bicos_hip {
namespace {

constexpr int WAVE = 64;
constexpr int TR = SPECKLE_TILE_ROWS, TC = SPECKLE_TILE_COLS;
constexpr int WAVES = SPECKLE_THREADS / WAVE;
constexpr int ROWS_PER_WAVE = TR / WAVES;
constexpr int BLOCK_ITEMS = SPECKLE_THREADS * SPECKLE_PER_LANE;
// the resolve launch: pixels per workgroup (more than a row of tiles' roots of a wide frame), the
// (root, size) pairs it gathers in LDS, and the distinct roots a wave sums before it adds
constexpr int RESOLVE_PER_LANE = 16;
constexpr int RESOLVE_ITEMS = SPECKLE_THREADS * RESOLVE_PER_LANE;
constexpr int RESOLVE_LIST = 1024;
constexpr int RESOLVE_LEADERS = 4;
constexpr int APPLY_MAX_BLOCKS = 1024;
static_assert(TC == WAVE, "a wave owns a tile row");
static_assert(SPECKLE_THREADS % WAVE == 0 && TR % WAVES == 0, "whole waves, whole rows");

// the pixel as a float, NaN where it is invalid: a link then fails on its own
__device__ __forceinline__ float pixel_value(int16_t v, int) {
    return v == INT16_MIN ? __builtin_nanf("") : (float)v;
}
__device__ __forceinline__ float pixel_value(float v, int flags) {
    return ((flags & BICOS_SPECKLE_F32_SENTINEL) && v == -32768.0f) ? __builtin_nanf("") : v;
}
__device__ __forceinline__ int16_t removed_value(int16_t, int) { return INT16_MIN; }
__device__ __forceinline__ float removed_value(float, int flags) {
    return (flags & BICOS_SPECKLE_F32_SENTINEL) ? -32768.0f : __builtin_nanf("");
}

// one IEEE subtraction; false when either is NaN (invalid) or the difference is (inf - inf)
__device__ __forceinline__ bool linked(float a, float b, float max_diff) {
    return __builtin_fabsf(a - b) <= max_diff;
}

template <typename T>
__device__ __forceinline__ float load_value(const SpeckleArgs& a, int row, int col) {
    return pixel_value(((const T*)a.disp)[(size_t)row * a.cols + col], a.flags);
}

// ------------------------------------------------------------------ LDS union-find
__device__ __forceinline__ int lds_find(int* L, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) return x;
        x = p;  // p < x
    }
}

__device__ __forceinline__ void lds_union(int* L, int a, int b) {
    for (;;) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(&L[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;
        a = old;  // old < a: max(a, b) has decreased
    }
}

template <typename T>
__global__ __launch_bounds__(SPECKLE_THREADS) void speckle_tile_kernel(SpeckleArgs a) {
    __shared__ float val[TR * TC];
    __shared__ int lab[TR * TC];
    __shared__ uint32_t cnt[TR * TC];
    __shared__ uint64_t starts[TR];  // per row: the lanes that begin a run
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const int row0 = blockIdx.y * TR, col0 = blockIdx.x * TC;
    const int gc = col0 + lane;

    float v[ROWS_PER_WAVE];
    uint64_t mask[ROWS_PER_WAVE];
#pragma unroll
    for (int k = 0; k < ROWS_PER_WAVE; ++k) {
        const int r = wave + k * WAVES, gr = row0 + r;
        const float nan = __builtin_nanf("");
        v[k] = (gr < a.rows && gc < a.cols) ? load_value<T>(a, gr, gc) : nan;
        const float left = __shfl_up(v[k], 1);
        const bool link_left = lane > 0 && linked(v[k], left, a.max_diff);
        mask[k] = __ballot(!link_left);  // bit 0 is always set
        const uint64_t below = mask[k] & (~0ull >> (63 - lane));
        const int start = 63 - __builtin_clzll(below);
        val[r * TC + lane] = v[k];
        lab[r * TC + lane] = r * TC + start;
        cnt[r * TC + lane] = 0;
        if (lane == 0) starts[r] = mask[k];
    }
    __syncthreads();

    // down links; the one at lane l is implied where lane l-1 has one too and both rows link
    // l-1 to l
#pragma unroll
    for (int k = 0; k < ROWS_PER_WAVE; ++k) {
        const int r = wave + k * WAVES;
        if (r + 1 >= TR) continue;  // wave-uniform
        const bool down = linked(v[k], val[(r + 1) * TC + lane], a.max_diff);
        const uint64_t dmask = __ballot(down);
        const uint64_t next_starts = starts[r + 1];
        const bool implied = lane > 0 && !((mask[k] >> lane) & 1) && !((next_starts >> lane) & 1) &&
                             ((dmask >> (lane - 1)) & 1);
        if (down && !implied) lds_union(lab, lab[r * TC + lane], lab[(r + 1) * TC + lane]);
    }
    __syncthreads();

    int root[ROWS_PER_WAVE];
#pragma unroll
    for (int k = 0; k < ROWS_PER_WAVE; ++k) {
        const int r = wave + k * WAVES;
        const bool valid = v[k] == v[k];
        const int start = 63 - __builtin_clzll(mask[k] & (~0ull >> (63 - lane)));
        root[k] = valid ? lds_find(lab, r * TC + start) : -1;
        if (valid && ((mask[k] >> lane) & 1)) {  // the run's first lane adds its length
            const uint64_t above = lane == 63 ? 0ull : mask[k] & (~0ull << (lane + 1));
            const int next = above ? __builtin_ctzll(above) : WAVE;
            atomicAdd(&cnt[root[k]], (uint32_t)(next - lane));
        }
    }
    __syncthreads();

#pragma unroll
    for (int k = 0; k < ROWS_PER_WAVE; ++k) {
        const int r = wave + k * WAVES, gr = row0 + r;
        if (gr >= a.rows || gc >= a.cols) continue;
        const size_t p = (size_t)gr * a.cols + gc;
        const int rt = root[k];
        a.labels[p] = rt < 0 ? -1 : (row0 + rt / TC) * a.cols + col0 + rt % TC;
        a.sizes[p] = rt == r * TC + lane ? cnt[rt] : 0u;
    }
}

// ---------------------------------------------------------------- global union-find
__device__ __forceinline__ int agent_find(int32_t* L, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;  // p < x
    }
}

__device__ __forceinline__ void agent_union(int32_t* L, int a, int b) {
    for (;;) {
        a = agent_find(L, a);
        b = agent_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(&L[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;  // old < a: max(a, b) has decreased
    }
}

// items [0, n_vert): the link (r, c)-(r, c+1) with c the last column of a tile column,
//                    item = border * rows + r
// items [n_vert, n_vert + n_horz): the link (r, c)-(r+1, c) with r the last row of a tile row,
//                    item - n_vert = border * cols + c
template <typename T>
__global__ __launch_bounds__(SPECKLE_THREADS) void speckle_border_kernel(SpeckleArgs a,
                                                                        uint32_t n_vert,
                                                                        uint32_t n_horz) {
    const uint32_t first = blockIdx.x * (uint32_t)BLOCK_ITEMS + threadIdx.x;
#pragma unroll
    for (int k = 0; k < SPECKLE_PER_LANE; ++k) {
        const uint32_t item = first + k * SPECKLE_THREADS;
        if (item >= n_vert + n_horz) continue;
        int r, c, r2, c2;
        bool implied = false;
        float v, w;
        if (item < n_vert) {
            const uint32_t border = item / (uint32_t)a.rows;
            r = r2 = (int)(item - border * (uint32_t)a.rows);
            c = (int)(border + 1) * TC - 1;
            c2 = c + 1;
            v = load_value<T>(a, r, c);
            w = load_value<T>(a, r2, c2);
            if (r % TR != 0) {
                const float pv = load_value<T>(a, r - 1, c), pw = load_value<T>(a, r - 1, c2);
                implied = linked(pv, pw, a.max_diff) && linked(pv, v, a.max_diff) &&
                          linked(pw, w, a.max_diff);
            }
        } else {
            const uint32_t j = item - n_vert, border = j / (uint32_t)a.cols;
            c = c2 = (int)(j - border * (uint32_t)a.cols);
            r = (int)(border + 1) * TR - 1;
            r2 = r + 1;
            v = load_value<T>(a, r, c);
            w = load_value<T>(a, r2, c2);
            if (c % TC != 0) {
                const float pv = load_value<T>(a, r, c - 1), pw = load_value<T>(a, r2, c - 1);
                implied = linked(pv, pw, a.max_diff) && linked(pv, v, a.max_diff) &&
                          linked(pw, w, a.max_diff);
            }
        }
        if (linked(v, w, a.max_diff) && !implied)
            agent_union(a.labels, r * a.cols + c, r2 * a.cols + c2);
    }
}

__device__ __forceinline__ int plain_find(const int32_t* L, int x) {
    for (;;) {
        const int p = L[x];
        if (p == x) return x;
        x = p;  // p < x
    }
}

// Adds to one address are served one after another by the memory side (about 10 ns each,
// measured), and the frame's surface is ONE component with a tile-local root in every tile. So a
// workgroup first gathers its (root, size) pairs in LDS and each wave sums the pairs of up to
// RESOLVE_LEADERS distinct roots among its 64 before it adds: one add per workgroup and
// large component where it was one per tile. A pair that finds the list full is added directly.
__global__ __launch_bounds__(SPECKLE_THREADS) void speckle_resolve_kernel(SpeckleArgs a,
                                                                         uint32_t pixels) {
    __shared__ int list_root[RESOLVE_LIST];
    __shared__ uint32_t list_size[RESOLVE_LIST];
    __shared__ uint32_t list_n;
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    if (threadIdx.x == 0) list_n = 0;
    __syncthreads();
    const uint32_t first = blockIdx.x * (uint32_t)RESOLVE_ITEMS + threadIdx.x;
    uint32_t s[RESOLVE_PER_LANE];  // all loads first: they do not wait for one another
#pragma unroll
    for (int k = 0; k < RESOLVE_PER_LANE; ++k) {
        const uint32_t p = first + k * SPECKLE_THREADS;
        s[k] = p < pixels ? a.sizes[p] : 0u;
    }
#pragma unroll
    for (int k = 0; k < RESOLVE_PER_LANE; ++k) {
        const uint32_t p = first + k * SPECKLE_THREADS;
        if (s[k] == 0) continue;  // not a tile-local root
        const int g = plain_find(a.labels, (int)p);
        if (g == (int)p) continue;  // the global root: its slot receives the others' sizes
        a.labels[p] = g;
        const uint32_t at = atomicAdd(&list_n, 1u);
        if (at < (uint32_t)RESOLVE_LIST) {
            list_root[at] = g;
            list_size[at] = s[k];
        } else {
            atomicAdd(&a.sizes[g], s[k]);
        }
    }
    __syncthreads();
    const uint32_t n = list_n < (uint32_t)RESOLVE_LIST ? list_n : (uint32_t)RESOLVE_LIST;
    for (uint32_t base = wave * WAVE; base < n; base += SPECKLE_THREADS) {  // wave-uniform
        const uint32_t i = base + lane;
        int g = i < n ? list_root[i] : -1;
        const uint32_t size = i < n ? list_size[i] : 0u;
        for (int t = 0; t < RESOLVE_LEADERS; ++t) {
            const uint64_t open = __ballot(g >= 0);
            if (!open) break;
            const int leader = __builtin_ctzll(open);
            const int root = __shfl(g, leader);
            const bool mine = g == root;
            uint32_t sum = mine ? size : 0u;
#pragma unroll
            for (int d = WAVE / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
            if (lane == leader) atomicAdd(&a.sizes[root], sum);
            if (mine) g = -1;
        }
        if (g >= 0) atomicAdd(&a.sizes[g], size);
    }
}

template <typename T>
__global__ __launch_bounds__(SPECKLE_THREADS) void speckle_apply_kernel(SpeckleArgs a,
                                                                       uint32_t pixels) {
    __shared__ uint32_t wave_counts[WAVES][4];
    const T* in = (const T*)a.disp;  // may be `out`: a lane reads its pixel before it writes it
    T* out = (T*)a.out;
    uint32_t n[4] = {0, 0, 0, 0};  // kept, removed, invalid, removed_components (wave-uniform)
    // At most APPLY_MAX_BLOCKS workgroups stride over the map: the counts are four addresses,
    // and the adds to one address are served one after another.
    for (uint32_t base = blockIdx.x * (uint32_t)BLOCK_ITEMS; base < pixels;
         base += gridDim.x * (uint32_t)BLOCK_ITEMS) {
        const uint32_t first = base + threadIdx.x;
        // Three dependent loads per pixel -- its label t (a tile-local root, or -1), t's label g
        // (the global root: the resolve launch stored it, and L[g] == g) and g's size -- each
        // issued for all of the lane's pixels before the next, so they overlap.
        T v[SPECKLE_PER_LANE];
        int t[SPECKLE_PER_LANE], g[SPECKLE_PER_LANE];
        uint32_t size[SPECKLE_PER_LANE];
#pragma unroll
        for (int k = 0; k < SPECKLE_PER_LANE; ++k) {
            const uint32_t p = first + k * SPECKLE_THREADS;
            v[k] = p < pixels ? in[p] : T(0);
            t[k] = p < pixels ? a.labels[p] : -1;
        }
#pragma unroll
        for (int k = 0; k < SPECKLE_PER_LANE; ++k) g[k] = t[k] >= 0 ? a.labels[t[k]] : -1;
#pragma unroll
        for (int k = 0; k < SPECKLE_PER_LANE; ++k) size[k] = g[k] >= 0 ? a.sizes[g[k]] : 0u;
#pragma unroll
        for (int k = 0; k < SPECKLE_PER_LANE; ++k) {
            const uint32_t p = first + k * SPECKLE_THREADS;
            const bool inside = p < pixels, invalid = inside && t[k] < 0;
            const bool removed = inside && !invalid && size[k] <= a.max_size;
            const bool removed_root = removed && g[k] == (int)p;
            if (inside) {
                out[p] = removed ? removed_value(v[k], a.flags) : v[k];
                if (a.final_labels && !invalid) a.labels[p] = g[k];
            }
            n[0] += (uint32_t)__popcll(__ballot(inside && !invalid && !removed));
            n[1] += (uint32_t)__popcll(__ballot(removed));
            n[2] += (uint32_t)__popcll(__ballot(invalid));
            n[3] += (uint32_t)__popcll(__ballot(removed_root));
        }
    }
    if (!a.counts) return;
    if (threadIdx.x % WAVE == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) wave_counts[threadIdx.x / WAVE][c] = n[c];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += wave_counts[w][threadIdx.x];
        if (s) atomicAdd(&a.counts[threadIdx.x], s);
    }
}

inline uint32_t blocks_for(uint32_t items) { return (items + BLOCK_ITEMS - 1) / BLOCK_ITEMS; }

template <typename T>
hipError_t launch(const SpeckleArgs& a, hipStream_t st) {
    const uint32_t pixels = (uint32_t)a.rows * (uint32_t)a.cols;
    const uint32_t tiles_r = (a.rows + TR - 1) / TR, tiles_c = (a.cols + TC - 1) / TC;
    if (a.counts) {
        const hipError_t e = hipMemsetAsync(a.counts, 0, 4 * sizeof(uint32_t), st);
        if (e != hipSuccess) return e;
    }
    // (tile rows in grid y: at most 65535, i.e. 2 097 120 rows)
    if (tiles_r > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(speckle_tile_kernel<T>, dim3(tiles_c, tiles_r), dim3(SPECKLE_THREADS), 0, st, a);
    const uint32_t n_vert = (tiles_c - 1) * (uint32_t)a.rows, n_horz = (tiles_r - 1) * (uint32_t)a.cols;
    if (n_vert + n_horz)
        hipLaunchKernelGGL(speckle_border_kernel<T>, dim3(blocks_for(n_vert + n_horz)),
                           dim3(SPECKLE_THREADS), 0, st, a, n_vert, n_horz);
    hipLaunchKernelGGL(speckle_resolve_kernel, dim3((pixels + RESOLVE_ITEMS - 1) / RESOLVE_ITEMS),
                       dim3(SPECKLE_THREADS), 0, st, a, pixels);
    const uint32_t apply_blocks = blocks_for(pixels);
    hipLaunchKernelGGL(speckle_apply_kernel<T>,
                       dim3(apply_blocks < (uint32_t)APPLY_MAX_BLOCKS ? apply_blocks : APPLY_MAX_BLOCKS),
                       dim3(SPECKLE_THREADS), 0, st, a, pixels);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_speckle(const SpeckleArgs& a, bool f32, hipStream_t st) {
    return f32 ? launch<float>(a, st) : launch<int16_t>(a, st);
}

}  // namespace bicos_hip
