// project.hip -- a point list projected into another camera (project.hpp; the definition is
// include/bicos_c.h, "projection", restated in numpy by tests/project_ref.py).
//
// A lane owns a point. The camera model runs in IEEE double, operation for operation as the
// header writes it (no contraction: -ffp-contract=off and the pragma below), by ONE device
// function that both point kernels call: the resolve computes a point's (uf, vf, zf) again from
// its 12 bytes instead of reading 13 bytes that the splat would have had to write, so the stage
// needs no per-point workspace and the splat writes nothing but its offers.
//   (memset)                the keys [img_rows][img_cols] to all ones, the counts to zero
//   project_splat_kernel    every inside point offers (bits(zf) << 32) | i to the pixels of its
//                           splat, clipped to the image: atomicMin on unsigned long long at agent
//                           scope (the HIP default; the XCDs' L2s are not coherent with each other,
//                           a narrower scope would be wrong), behind a plain load that skips the
//                           offers that cannot win. Keys only fall and the minimum does not
//                           depend on the order of arrival: deterministic.
//   project_resolve_kernel  class from the key at the point's own pixel, uv / depth / cls, the
//                           bilinear gather of visible points, the counts: one ballot per class
//                           and step, summed per workgroup in LDS, at most five atomics per
//                           workgroup. Without a z-buffer (ZBUF = false) this is the only launch.
//   project_maps_kernel     only where a map is asked for: the keys unpacked per pixel.
// The launch boundary is the only ordering between the atomics and their readers: no flags, no
// workgroup waits on another.
//
// Memory safety: points are read at i < count only. A key is addressed at (y, x) with
// 0 <= y < img_rows and 0 <= x < img_cols: the own pixel by the float compares of "outside"
// (which NaN and infinities fail), the splat by the clamps. Image taps are clamped to the image
// and loaded for visible points only, which lie inside a non-empty image. Every store goes to
// position i < count of a per-point output or to a pixel below img_rows * img_cols.
#include "project.hpp"

namespace bicos_hip {
namespace {

constexpr int WAVE = 64;
constexpr int WAVES = PROJECT_THREADS / WAVE;
constexpr int CLASSES = 5;
constexpr uint32_t POINTS_PER_GROUP = PROJECT_THREADS * PROJECT_PER_LANE;
constexpr unsigned long long EMPTY_KEY = ~0ull;

enum : int { VISIBLE = 0, OCCLUDED = 1, OUTSIDE = 2, BEHIND = 3, INVALID = 4, NO_POINT = 5 };

struct Projected {
    int cls;  // VISIBLE (inside; the z-buffer has the last word), OUTSIDE, BEHIND or INVALID
    float uf, vf, zf;
    int px, py;  // the own pixel, where cls == VISIBLE
};

// Steps 1 to 4 of the definition for point i.
__device__ __forceinline__ Projected project_point(const ProjectCamera& c, const float* points,
                                                   uint32_t i, int img_rows, int img_cols) {
#pragma clang fp contract(off)
    const float nan = __builtin_nanf("");
    Projected r{INVALID, nan, nan, nan, 0, 0};
    const float* p = points + (size_t)i * 3;
    const float Xf = p[0], Yf = p[1], Zf = p[2];
    if (!(__builtin_isfinite(Xf) && __builtin_isfinite(Yf) && __builtin_isfinite(Zf))) return r;
    const double X = (double)Xf, Y = (double)Yf, Z = (double)Zf;
    const double Xc = ((c.R[0] * X + c.R[1] * Y) + c.R[2] * Z) + c.t[0];
    const double Yc = ((c.R[3] * X + c.R[4] * Y) + c.R[5] * Z) + c.t[1];
    const double Zc = ((c.R[6] * X + c.R[7] * Y) + c.R[8] * Z) + c.t[2];
    if (!(Zc > 0.0)) {
        r.cls = BEHIND;
        return r;
    }
    const double x = Xc / Zc, y = Yc / Zc;
    const double r2 = x * x + y * y;
    const double kr = (1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2) /
                      (1.0 + ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2);
    const double xd = (x * kr + c.p1 * ((2.0 * x) * y)) + c.p2 * (r2 + (2.0 * x) * x);
    const double yd = (y * kr + c.p1 * (r2 + (2.0 * y) * y)) + c.p2 * ((2.0 * x) * y);
    r.uf = (float)(c.fx * xd + c.cx);
    r.vf = (float)(c.fy * yd + c.cy);
    r.zf = (float)Zc;
    const float pxf = floorf(r.uf + 0.5f), pyf = floorf(r.vf + 0.5f);
    const bool inside = __builtin_isfinite(r.uf) && __builtin_isfinite(r.vf) && pxf >= 0.0f &&
                        pxf < (float)img_cols && pyf >= 0.0f && pyf < (float)img_rows;
    r.cls = inside ? VISIBLE : OUTSIDE;
    if (inside) {
        r.px = (int)pxf;
        r.py = (int)pyf;
    }
    return r;
}

__global__ __launch_bounds__(PROJECT_THREADS) void project_splat_kernel(ProjectArgs a) {
    const uint32_t first = blockIdx.x * POINTS_PER_GROUP + threadIdx.x;
#pragma unroll
    for (int k = 0; k < PROJECT_PER_LANE; ++k) {
        const uint32_t i = first + k * PROJECT_THREADS;
        if (i >= a.count) continue;
        const Projected p = project_point(a.cam, a.points, i, a.img_rows, a.img_cols);
        if (p.cls != VISIBLE) continue;
        // zf is a non-negative float: its bits order as its value does
        const unsigned long long key = ((unsigned long long)__float_as_uint(p.zf) << 32) | i;
        const int y0 = max(p.py - a.splat, 0), y1 = min(p.py + a.splat, a.img_rows - 1);
        const int x0 = max(p.px - a.splat, 0), x1 = min(p.px + a.splat, a.img_cols - 1);
        for (int y = y0; y <= y1; ++y) {
            unsigned long long* row = a.keys + (uint32_t)y * (uint32_t)a.img_cols;
            for (int x = x0; x <= x1; ++x) {
                // a plain load first: an offer that cannot win is not made. Keys only fall
                // during the launch, so a stale value (another XCD's L2, this CU's cache) is
                // never below the current one: it can cost an unneeded atomic, never skip a
                // winner. Measured: 1.7x at splat 1, 2.7x at splat 2
                if (row[x] <= key) continue;
                atomicMin(row + x, key);
            }
        }
    }
}

// One channel of the remap's blend, the edge replicated; every operation a float32 rounding
template <typename T>
__device__ __forceinline__ T blend(const T* r0, const T* r1, uint32_t xa, uint32_t xb, float fx,
                                   float fy) {
#pragma clang fp contract(off)
    const float p00 = (float)r0[xa], p01 = (float)r0[xb];
    const float p10 = (float)r1[xa], p11 = (float)r1[xb];
    const float top = p00 + fx * (p01 - p00);
    const float bot = p10 + fx * (p11 - p10);
    const float val = top + fy * (bot - top);
    const float top_level = sizeof(T) == 1 ? 255.0f : 65535.0f;
    return (T)fminf(fmaxf(rintf(val), 0.0f), top_level);
}

template <bool ZBUF, typename T, int CH>
__global__ __launch_bounds__(PROJECT_THREADS) void project_resolve_kernel(ProjectArgs a) {
#pragma clang fp contract(off)
    __shared__ uint32_t wave_counts[WAVES][CLASSES];
    const uint32_t first = blockIdx.x * POINTS_PER_GROUP + threadIdx.x;
    uint32_t n[CLASSES] = {0, 0, 0, 0, 0};  // wave-uniform
#pragma unroll
    for (int k = 0; k < PROJECT_PER_LANE; ++k) {
        const uint32_t i = first + k * PROJECT_THREADS;
        int cls = NO_POINT;
        if (i < a.count) {
            const Projected p = project_point(a.cam, a.points, i, a.img_rows, a.img_cols);
            cls = p.cls;
            if (ZBUF && cls == VISIBLE) {
                const unsigned long long key =
                    a.keys[(uint32_t)p.py * (uint32_t)a.img_cols + (uint32_t)p.px];
                const float zmin = __uint_as_float((uint32_t)(key >> 32));
                if (!(p.zf <= zmin + a.tol)) cls = OCCLUDED;
            }
            if (a.uv) {  // (two stores: the caller's array is only 4-byte aligned)
                a.uv[2 * (size_t)i] = p.uf;
                a.uv[2 * (size_t)i + 1] = p.vf;
            }
            if (a.zdepth) a.zdepth[i] = p.zf;
            if (a.cls) a.cls[i] = (uint8_t)cls;
            if (a.tex) {
                T* out = (T*)a.tex + (size_t)i * CH;
                if (cls == VISIBLE) {
                    // uf in [-0.5, img_cols - 0.5), vf likewise: the conversions are exact
                    const float x0f = floorf(p.uf), y0f = floorf(p.vf);
                    const float fx = p.uf - x0f, fy = p.vf - y0f;
                    const int x0 = (int)x0f, y0 = (int)y0f;
                    const uint32_t xa = (uint32_t)min(max(x0, 0), a.img_cols - 1) * CH;
                    const uint32_t xb = (uint32_t)min(max(x0 + 1, 0), a.img_cols - 1) * CH;
                    const T* r0 = (const T*)a.image +
                                  (size_t)min(max(y0, 0), a.img_rows - 1) * a.img_pitch;
                    const T* r1 = (const T*)a.image +
                                  (size_t)min(max(y0 + 1, 0), a.img_rows - 1) * a.img_pitch;
#pragma unroll
                    for (int ch = 0; ch < CH; ++ch)
                        out[ch] = blend<T>(r0 + ch, r1 + ch, xa, xb, fx, fy);
                } else {
#pragma unroll
                    for (int ch = 0; ch < CH; ++ch) out[ch] = (T)a.fill;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CLASSES; ++c) n[c] += (uint32_t)__popcll(__ballot(cls == c));
    }
    if (!a.counts) return;  // (uniform)
    if (threadIdx.x % WAVE == 0) {
#pragma unroll
        for (int c = 0; c < CLASSES; ++c) wave_counts[threadIdx.x / WAVE][c] = n[c];
    }
    __syncthreads();
    if (threadIdx.x < CLASSES) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += wave_counts[w][threadIdx.x];
        if (s) atomicAdd(a.counts + threadIdx.x, s);
    }
}

__global__ __launch_bounds__(PROJECT_THREADS) void project_maps_kernel(
    const unsigned long long* __restrict__ keys, uint32_t pixels, float* __restrict__ depth_map,
    int32_t* __restrict__ index_map) {
    const uint32_t idx = blockIdx.x * (uint32_t)PROJECT_THREADS + threadIdx.x;
    if (idx >= pixels) return;
    const unsigned long long key = keys[idx];
    const bool empty = key == EMPTY_KEY;  // (no point's key: its high word would be a NaN's bits)
    if (depth_map)
        depth_map[idx] = empty ? __builtin_nanf("") : __uint_as_float((uint32_t)(key >> 32));
    if (index_map) index_map[idx] = empty ? -1 : (int32_t)(uint32_t)key;
}

template <bool ZBUF>
void launch_resolve(const ProjectArgs& a, dim3 grid, hipStream_t st) {
    const dim3 block(PROJECT_THREADS);
    const bool three = a.tex && a.channels == 3;
    if (a.tex && a.depth == 2) {
        if (three)
            hipLaunchKernelGGL((project_resolve_kernel<ZBUF, uint16_t, 3>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((project_resolve_kernel<ZBUF, uint16_t, 1>), grid, block, 0, st, a);
    } else {
        if (three)
            hipLaunchKernelGGL((project_resolve_kernel<ZBUF, uint8_t, 3>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((project_resolve_kernel<ZBUF, uint8_t, 1>), grid, block, 0, st, a);
    }
}

}  // namespace

hipError_t launch_project(const ProjectArgs& a, hipStream_t st) {
    const uint32_t pixels = (uint32_t)a.img_rows * (uint32_t)a.img_cols;
    const dim3 grid((a.count + POINTS_PER_GROUP - 1) / POINTS_PER_GROUP);
    if (a.counts)
        if (hipError_t rc = hipMemsetAsync(a.counts, 0, CLASSES * sizeof(uint32_t), st)) return rc;
    if (a.keys && pixels) {
        if (hipError_t rc = hipMemsetAsync(a.keys, 0xFF, (size_t)pixels * sizeof(*a.keys), st))
            return rc;
        if (a.count)
            hipLaunchKernelGGL(project_splat_kernel, grid, dim3(PROJECT_THREADS), 0, st, a);
    }
    if (a.count && (a.uv || a.zdepth || a.cls || a.tex || a.counts)) {
        if (a.keys)
            launch_resolve<true>(a, grid, st);
        else
            launch_resolve<false>(a, grid, st);
    }
    if (a.keys && pixels && (a.depth_map || a.index_map))
        hipLaunchKernelGGL(project_maps_kernel, dim3((pixels + PROJECT_THREADS - 1) / PROJECT_THREADS),
                           dim3(PROJECT_THREADS), 0, st, a.keys, pixels, a.depth_map, a.index_map);
    return hipGetLastError();
}

}  // namespace bicos_hip
