// mesh.hip -- disparity map -> triangle mesh over the reprojection's ordered point list (mesh.hpp;
// the definition is include/bicos_c.h, "mesh").
//
// A disparity map is an organised grid: every 2x2 block of pixels is a quad of at most two
// triangles, so there is no neighbour search. Everything runs over the reprojection's fixed
// segments of the linear pixel index, one workgroup each, no workgroup waiting on another and no
// atomics. Six launches:
//   reproject_count_kernel  } the vertex list, by reproject_device.hpp's code: the write also
//   reproject_scan_kernel   } stores every pixel's rank in the full list, or -1, into the rank
//   reproject_write_kernel  } array (one dense 4-byte store per pixel, no memset, no scatter)
//   mesh_count_kernel       a lane owns the quad whose corner A is its pixel: four ranks, four
//                           disparities, float32 compares only; per segment the triangles and the
//                           quads with 2, 1 and 0 of them, from two ballots
//   reproject_scan_kernel   the same scan over those: triangle offsets and the four mesh_counts
//   mesh_write_kernel       the quads again; a triangle's position is the segment's offset plus
//                           the mbcnt ranks of the two ballots, in pixel order and T0 before T1,
//                           below tri_capacity only: 12-byte stores
#include "mesh.hpp"

#include "reproject_device.hpp"

namespace bicos_hip {
namespace {

struct Triangle {
    int32_t a, b, c;
};

// The triangles of one quad in the order of the definition, as vertex numbers: n of them, t0
// first. `quad`: the pixel is the corner A of a quad at all.
struct Quad {
    int n;
    bool quad;
    Triangle t0, t1;
};

// The quad whose corner A is pixel idx.
template <typename T>
__device__ __forceinline__ Quad quad_triangles(const MeshArgs& a, uint32_t idx) {
    const uint32_t cols = (uint32_t)a.v.cols;
    Quad q{0, false, Triangle{-1, -1, -1}, Triangle{-1, -1, -1}};
    if (idx >= a.v.pixels) return q;
    const uint32_t row = idx / cols, col = idx - row * cols;
    if (col + 1 >= cols || row + 1 >= (uint32_t)a.rows) return q;
    q.quad = true;
    // (the farthest corner, idx + cols + 1, is at most pixels - 1 here)
    const int32_t rA = a.rank[idx], rB = a.rank[idx + 1];
    const int32_t rC = a.rank[idx + cols], rD = a.rank[idx + cols + 1];
    const bool kA = rA >= 0, kB = rB >= 0, kC = rC >= 0, kD = rD >= 0;
    if ((int)kA + (int)kB + (int)kC + (int)kD < 3) return q;
    const T* d = (const T*)a.v.disp;
    const float dA = (float)d[idx], dB = (float)d[idx + 1];
    const float dC = (float)d[idx + cols], dD = (float)d[idx + cols + 1];
    // a link needs both ends kept; one float32 subtraction each
    const float md = a.max_diff;
    const float ad = __builtin_fabsf(dA - dD), bc = __builtin_fabsf(dB - dC);
    const bool lAB = kA && kB && __builtin_fabsf(dA - dB) <= md;
    const bool lAC = kA && kC && __builtin_fabsf(dA - dC) <= md;
    const bool lBD = kB && kD && __builtin_fabsf(dB - dD) <= md;
    const bool lCD = kC && kD && __builtin_fabsf(dC - dD) <= md;
    const bool lAD = kA && kD && ad <= md;
    const bool lBC = kB && kC && bc <= md;
    // all four kept: the diagonal with the smaller step, a tie takes AD. Three kept: the
    // diagonal whose two ends are there (B or C missing: AD; A or D missing: BC); the triangle
    // with the missing corner then has a broken link by itself.
    const bool all = kA && kB && kC && kD;
    const bool use_ad = all ? ad <= bc : (kA && kD);
    const bool e0 = use_ad ? (lAC && lCD && lAD) : (lAC && lBC && lAB);
    const bool e1 = use_ad ? (lAD && lBD && lAB) : (lBC && lCD && lBD);
    const Triangle t0 = use_ad ? Triangle{rA, rC, rD} : Triangle{rA, rC, rB};
    const Triangle t1 = use_ad ? Triangle{rA, rD, rB} : Triangle{rB, rC, rD};
    q.n = (int)e0 + (int)e1;
    q.t0 = e0 ? t0 : t1;
    q.t1 = t1;
    return q;
}

template <typename T>
__global__ __launch_bounds__(REPROJECT_THREADS) void mesh_count_kernel(MeshArgs a) {
    __shared__ uint32_t wave_counts[WAVES][3];
    const uint32_t first = blockIdx.x * (uint32_t)REPROJECT_SEGMENT + threadIdx.x;
    uint32_t n2 = 0, n1 = 0, n0 = 0;  // wave-uniform: quads with 2, 1 and 0 triangles
#pragma unroll
    for (int k = 0; k < REPROJECT_PER_LANE; ++k) {
        const Quad q = quad_triangles<T>(a, first + k * REPROJECT_THREADS);
        n2 += (uint32_t)__popcll(__ballot(q.n == 2));
        n1 += (uint32_t)__popcll(__ballot(q.n == 1));
        n0 += (uint32_t)__popcll(__ballot(q.quad && q.n == 0));
    }
    if (threadIdx.x % WAVE == 0) {
        wave_counts[threadIdx.x / WAVE][0] = n2;
        wave_counts[threadIdx.x / WAVE][1] = n1;
        wave_counts[threadIdx.x / WAVE][2] = n0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s2 = 0, s1 = 0, s0 = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            s2 += wave_counts[w][0];
            s1 += wave_counts[w][1];
            s0 += wave_counts[w][2];
        }
        ((uint4*)a.tri_counts)[blockIdx.x] = make_uint4(2 * s2 + s1, s2, s1, s0);
    }
}

template <typename T>
__global__ __launch_bounds__(REPROJECT_THREADS) void mesh_write_kernel(MeshArgs a) {
    __shared__ uint32_t wave_tris[REPROJECT_PER_LANE][WAVES];
    const uint32_t first = blockIdx.x * (uint32_t)REPROJECT_SEGMENT + threadIdx.x;
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    Quad q[REPROJECT_PER_LANE];
    uint64_t has1[REPROJECT_PER_LANE], has2[REPROJECT_PER_LANE];  // (uniform)
#pragma unroll
    for (int k = 0; k < REPROJECT_PER_LANE; ++k) {
        q[k] = quad_triangles<T>(a, first + k * REPROJECT_THREADS);
        has1[k] = __ballot(q[k].n >= 1);
        has2[k] = __ballot(q[k].n == 2);
        if (lane == 0) wave_tris[k][wave] = (uint32_t)(__popcll(has1[k]) + __popcll(has2[k]));
    }
    __syncthreads();
    // pixel order within the segment: step k, then wave, then lane; within a quad T0, then T1
    uint32_t at = a.tri_offsets[blockIdx.x];
#pragma unroll
    for (int k = 0; k < REPROJECT_PER_LANE; ++k) {
        uint32_t mine = at;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t c = wave_tris[k][w];
            if (w < wave) mine += c;
            at += c;
        }
        const uint32_t pos = mine + lanes_below(has1[k]) + lanes_below(has2[k]);
        if (q[k].n >= 1 && pos < a.tri_capacity) ((Triangle*)a.triangles)[pos] = q[k].t0;
        if (q[k].n == 2 && pos + 1 < a.tri_capacity) ((Triangle*)a.triangles)[pos + 1] = q[k].t1;
    }
}

template <typename T>
hipError_t launch(const MeshArgs& a, hipStream_t st) {
    const uint32_t segments = reproject_segments(a.v.pixels);
    const dim3 grid(segments), block(REPROJECT_THREADS);
    hipLaunchKernelGGL(reproject_count_kernel<T>, grid, block, 0, st, a.v);
    hipLaunchKernelGGL(reproject_scan_kernel, dim3(1), dim3(REPROJECT_SCAN_THREADS), 0, st,
                       (const uint32_t*)a.v.seg_counts, a.v.seg_offsets, segments, a.v.counts);
    hipLaunchKernelGGL((reproject_write_kernel<T, true, false, true>), grid, block, 0, st, a.v,
                       a.rank);
    hipLaunchKernelGGL(mesh_count_kernel<T>, grid, block, 0, st, a);
    hipLaunchKernelGGL(reproject_scan_kernel, dim3(1), dim3(REPROJECT_SCAN_THREADS), 0, st,
                       (const uint32_t*)a.tri_counts, a.tri_offsets, segments, a.mesh_counts);
    hipLaunchKernelGGL(mesh_write_kernel<T>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_mesh(const MeshArgs& a, bool f32, hipStream_t st) {
    return f32 ? launch<float>(a, st) : launch<int16_t>(a, st);
}

}  // namespace bicos_hip
