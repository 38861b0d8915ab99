// search_guided.hip -- the windowed matrix-core search of search_range.hip with one disparity
// window PER LEFT PIXEL (include/bicos_c.h, "disparity guide"), and the kernel that derives
// such windows from a prior disparity map.
//
// search_guided_kernel is search_range_kernel (whose header comment derives the scheme: one
// row x waves * T * 32 col0 per workgroup, the left fragments in registers, the right row
// staged into LDS as FP4 fragments in fills of `chunk` columns, absolute float keys, a signed
// last-minimum tree for NoDuplicates, the "no candidate" test before the key is decoded) with
// the window read per lane instead of from two kernel arguments:
//
//  * Bounds. Lane j of tile t owns col0 = c0_t + j and loads its guide dword {lo, hi} (an empty
//    window past the row's end). dlo = max(dmin, lo, col0 - (cols - 1)) and dhi = min(dmax, hi,
//    col0) are the disparities whose col1 lie in the row; the window is empty iff dlo > dhi.
//  * Block skipping. The col1 a tile can need are [min (col0 - dhi), max (col0 - dlo)] over
//    its lanes with a window, a wave's the union over its tiles, the workgroup's staged columns
//    the union over its waves (one LDS word pair per wave behind one barrier). All of these are
//    reduced once, in the prologue, and kept wave-uniform (SGPRs). A wave or a workgroup
//    without any candidate multiplies nothing, but joins every barrier and writes its pixels
//    as invalid.
//  * Masking. The pair (tile, block B) needs no mask iff every lane's 32 pairs lie inside that
//    lane's window: col0 - B - 31 >= dlo and col0 - B <= dhi for all j, i.e. c0_t - B - 31 >=
//    max_j (dlo_j - j) and c0_t - B <= min_j (dhi_j - j) -- the tile's intersection window,
//    taken relative to the lane so that the test is exact (for a constant guide it is
//    search_range_kernel's cut_lo / cut_hi, the image's right edge included). Otherwise the
//    element mask compares against the lane's own dlo and dhi, against one of them where the
//    other edge does not cut the pair. A lane with an empty window fails either compare for
//    every pair, so it ends at "no candidate".
//
// guide_kernel: one output pixel per lane, the minimum and maximum of the valid prior values
// of the clipped (2 spread + 1)^2 window around the pixel's prior position, one dword store.
#include "guide.hpp"
#include "search_dev.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace bicos_hip {

namespace {

__device__ __forceinline__ int imax3(int a, int b, int c) { return max(max(a, b), c); }
// signed max over the 16 keys of a negated-product tile and m (v_max3_i32 tree)
__device__ __forceinline__ int imax16(const v16f& d, int m) {
    auto k = [&](int r) { return (int)fbits(d[r]); };
    const int a0 = imax3(k(0), k(1), k(2)), a1 = imax3(k(3), k(4), k(5));
    const int a2 = imax3(k(6), k(7), k(8)), a3 = imax3(k(9), k(10), k(11));
    const int a4 = imax3(k(12), k(13), k(14));
    return imax3(m, imax3(a0, a1, a2), imax3(a3, a4, k(15)));
}

// min / max over the 32 lanes of a wave half (both halves hold the same values here), made
// wave-uniform: four DPP steps inside each row of 16 lanes (quad_perm [1,0,3,2] and [2,3,0,1],
// row_half_mirror, row_mirror -- every lane of a row then holds the row's result), and rows
// 0 and 1 joined on the scalar side. (Through __shfl_xor the 16 reductions of a 4-tile wave
// were 80 dependent ds_bpermute round trips ahead of the first LDS fill.)
template <int CTRL>
__device__ __forceinline__ int dpp_lane(int v) {
    return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ int half_min(int v) {
    v = min(v, dpp_lane<0xB1>(v));
    v = min(v, dpp_lane<0x4E>(v));
    v = min(v, dpp_lane<0x141>(v));
    v = min(v, dpp_lane<0x140>(v));
    return min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16));
}
__device__ __forceinline__ int half_max(int v) {
    v = max(v, dpp_lane<0xB1>(v));
    v = max(v, dpp_lane<0x4E>(v));
    v = max(v, dpp_lane<0x141>(v));
    v = max(v, dpp_lane<0x140>(v));
    return max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16));
}

constexpr int SPAN_NONE_LO = 1 << 20;  // an empty col1 span: lo above every column, hi = -1
constexpr int WIN_ALL = 1 << 20;       // beyond every disparity (|d| < 32768) and lane offset

// A workgroup = one row x the col0 range [tile * waves * T * 32, + waves * T * 32); a.chunk
// col1 per LDS fill (multiple of 32), fills start at the first 32-col1 block of the
// workgroup's span. ka.dmin / ka.dmax within [-cols, cols] (launch_search_guided).
// (The 128-bit NoDuplicates kernel of 4 tiles, the headline shape's, must stay within 128
// VGPRs: its LDS stage lets two workgroups share a CU only if the registers do, and left
// alone the allocator ends at 133, search_range_kernel's 127 plus the upper bounds. Asked
// for 4 waves per SIMD it fits without scratch; the other instantiations stay as they
// come.)
template <int WORDS, int KS, bool NODUPES, int T>
__global__ __launch_bounds__(512)
__attribute__((amdgpu_waves_per_eu(WORDS == 4 && KS == 2 && NODUPES && T == 4 ? 4 : 1)))
void search_guided_kernel(SearchGuidedArgs ka) {
    const SearchArgs& a = ka.s;
    static_assert(KS >= 1 && 2 * KS <= (WORDS >= 2 ? WORDS : 2), "K-steps exceed the descriptor");
    constexpr int WL = 2 * KS;  // LDS word slots per col1 (W=1: 1 pad)
    extern __shared__ __attribute__((aligned(16))) v4i lds_gd[];  // [WL][chunk]
    __shared__ int wave_span[2 * 8];  // {lo1, hi1} of each wave

    int row, tile;
    xcd_row_tile(a.tiles_per_row, row, tile);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int h = lane >> 5;
    const int j = lane & 31;
    const int cols = a.cols;
    const int chunk = a.chunk;
    const int waves = blockDim.x >> 6;
    const int dmin = ka.dmin, dmax = ka.dmax;
    const int wg_c0 = tile * waves * T * 32;
    const int c0_wave = wg_c0 + wave * (T * 32);

    const uint32_t* __restrict__ row0 = a.desc0 + (size_t)row * a.desc_pitch;
    const uint32_t* __restrict__ row1 = a.desc1 + (size_t)row * a.desc_pitch;
    const uint32_t* __restrict__ grow =
        reinterpret_cast<const uint32_t*>(ka.guide) + (size_t)row * ka.guide_pitch;

    // B fragments: +1 (0x2) where the left bit is 0, -1 (0xA) where it is 1
    v4i bf[T][KS];
    // this lane's window of disparities whose col1 lie in the row, dlo in the low and dhi in
    // the high half of one register (both fit int16; empty: dlo > dhi). Two registers per
    // tile took the 128-bit NoDuplicates kernel of 4 tiles past 128 VGPRs, one workgroup per
    // CU instead of two.
    uint32_t win_lane[T];
    // per tile, wave-uniform: the col1 its lanes can need, and its intersection window
    // relative to the lane (max (dlo - j), min (dhi - j))
    int t_lo1[T], t_hi1[T], t_ilo[T], t_ihi[T];
    int wv_lo1 = SPAN_NONE_LO, wv_hi1 = -1;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int c0 = c0_wave + 32 * t + j;
        const bool in = c0 < cols;
        int lo = 1, hi = 0;
        if (in) {
            const uint32_t g = grow[c0];
            lo = (int)(int16_t)(g & 0xFFFFu);
            hi = (int)(int16_t)(g >> 16);
        }
        const int dlo = in ? max(max(dmin, lo), c0 - (cols - 1)) : 1;
        const int dhi = in ? min(min(dmax, hi), c0) : 0;
        win_lane[t] = ((uint32_t)dlo & 0xFFFFu) | ((uint32_t)dhi << 16);
        const bool has = dlo <= dhi;
        t_lo1[t] = half_min(has ? c0 - dhi : SPAN_NONE_LO);
        t_hi1[t] = half_max(has ? c0 - dlo : -1);
        // (lanes past the row's end hold no pixel: they do not narrow the intersection)
        t_ilo[t] = half_max(in ? dlo - j : -WIN_ALL);
        t_ihi[t] = half_min(in ? dhi - j : WIN_ALL);
        wv_lo1 = min(wv_lo1, t_lo1[t]);
        wv_hi1 = max(wv_hi1, t_hi1[t]);
#pragma unroll
        for (int s = 0; s < KS; ++s) bf[t][s] = expand_bits(desc_word<WORDS, KS>(row0, c0, 2 * s + h, in), LUT_B);
    }

    uint32_t m1[T];
    int m2[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        m1[t] = KEY_NONE;
        m2[t] = 0;
    }
    // row offset of accumulator register r in this lane half
    auto rrow = [&](int r) { return (r & 3) + 8 * (r >> 2) + 4 * h; };

    // the workgroup's staged span: the union of its waves' (inclusive; empty when lo > hi)
    if (lane == 0) {
        wave_span[2 * wave] = wv_lo1;
        wave_span[2 * wave + 1] = wv_hi1;
    }
    __syncthreads();
    int wg_lo1 = SPAN_NONE_LO, wg_hi1 = -1;
    for (int w = 0; w < waves; ++w) {
        wg_lo1 = min(wg_lo1, wave_span[2 * w]);
        wg_hi1 = max(wg_hi1, wave_span[2 * w + 1]);
    }
    wg_lo1 = __builtin_amdgcn_readfirstlane(wg_lo1);
    wg_hi1 = __builtin_amdgcn_readfirstlane(wg_hi1);
    const bool idle = wv_hi1 < wv_lo1;  // wave-uniform; still joins the barriers
    const int stage0 = wg_lo1 & ~31;    // first staged column
    const int nchunks = wg_hi1 >= wg_lo1 ? (wg_hi1 - stage0) / chunk + 1 : 0;

    // C of the block being multiplied: BIAS + col1 * EPS, advanced by 32 * EPS per block
    // (exact: col1 < 32768 keeps 256 + col1 * 2^-15 within 24 bits)
    int bc = idle ? 0 : wv_lo1 & ~31;  // the block base cc stands at
    v16f cc;
#pragma unroll
    for (int r = 0; r < 16; ++r) cc[r] = KEY_BIAS + (float)(bc + rrow(r)) * KEY_EPS;

    for (int k = 0; k < nchunks; ++k) {
        const int base = stage0 + k * chunk;
        // columns of this fill the workgroup needs: up to the end of its span's last block
        const int ncols = min(chunk, ((wg_hi1 | 31) + 1) - base);
        if (k) __syncthreads();
        // expand the fill's right descriptors: one col1 per thread, all its words
        for (int c = threadIdx.x; c < ncols; c += blockDim.x) {
            const int c1 = base + c;
#pragma unroll
            for (int w = 0; w < WL; ++w) {
                lds_gd[w * chunk + c] = expand_bits(desc_word<WORDS, KS>(row1, c1, w, c1 < cols), LUT_A);
            }
        }
        __syncthreads();
        if (idle) continue;

        // this wave's blocks of the fill (wave-uniform bounds)
        const int b_lo = max(wv_lo1, base) >> 5;
        const int b_hi = min(wv_hi1, base + ncols - 1) >> 5;
        for (int bi = b_lo; bi <= b_hi; ++bi) {
            const int B = 32 * bi;
            if (B != bc) {
#pragma unroll
                for (int r = 0; r < 16; ++r) cc[r] += (float)(B - bc) * KEY_EPS;  // exact
                bc = B;
            }
            v4i af[KS], an[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) af[s] = lds_gd[(2 * s + h) * chunk + (B - base) + j];
            if constexpr (NODUPES) {
#pragma unroll
                for (int s = 0; s < KS; ++s)
#pragma unroll
                    for (int q = 0; q < 4; ++q) an[s][q] = af[s][q] | (af[s][q] << 2);  // 1.0 -> -1.0
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int c0_t = c0_wave + 32 * t;
                // outside the col1 any lane of the tile can need
                if (B + 31 < t_lo1[t] || B > t_hi1[t]) continue;
                // which edges of some lane's window cut through the pair (wave-uniform): a
                // lower one (or the image's right edge), an upper one; neither = wholly inside
                const bool cut_lo = c0_t - B - 31 < t_ilo[t];
                const bool cut_hi = c0_t - B > t_ihi[t];
                v16f c1 = cc, c2 = cc;
                if (cut_lo || cut_hi) {
                    // register r's pair has disparity dl - off(r), off(r) = (r & 3) + 8 (r >> 2)
                    // a constant: inside iff off(r) <= dl - dlo and off(r) >= dl - dhi
                    const int dl = c0_t + j - B - 4 * h;
                    const int off_max = dl - (int)(int16_t)(win_lane[t] & 0xFFFFu);
                    const int off_min = dl - ((int)win_lane[t] >> 16);
                    auto mask = [&](auto in) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const bool k = in((r & 3) + 8 * (r >> 2));
                            c1[r] = k ? cc[r] : KEY_PAD;
                            c2[r] = k ? cc[r] : -KEY_PAD;
                        }
                    };
                    if (!cut_hi)
                        mask([&](int off) { return off <= off_max; });
                    else if (!cut_lo)
                        mask([&](int off) { return off >= off_min; });
                    else
                        mask([&](int off) { return off <= off_max && off >= off_min; });
                }
                v16f d = mfma_fp4(af[0], bf[t][0], c1);
#pragma unroll
                for (int s = 1; s < KS; ++s) d = mfma_fp4(af[s], bf[t][s], d);
                m1[t] = min16(d, m1[t], 0u);
                if constexpr (NODUPES) {
                    v16f e = mfma_fp4(an[0], bf[t][0], c2);
#pragma unroll
                    for (int s = 1; s < KS; ++s) e = mfma_fp4(an[s], bf[t][s], e);
                    m2[t] = imax16(e, m2[t]);
                }
            }
        }
    }
    if (c0_wave >= cols) return;

    // the two lane halves hold the even / odd 4-row groups of every block
#pragma unroll
    for (int t = 0; t < T; ++t) {
        m1[t] = min(m1[t], (uint32_t)__shfl_xor((int)m1[t], 32));
        if constexpr (NODUPES) m2[t] = max(m2[t], __shfl_xor(m2[t], 32));
    }
    int16_t* out = a.out + (size_t)row * a.out_pitch;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (T > 1 && (t & 1) != h) continue;  // half 0 writes even tiles, half 1 odd tiles
        if (T == 1 && h) continue;
        const int c0 = c0_wave + 32 * t + j;
        if (c0 >= cols) continue;
        // no candidate in the window: the running minimum was never lowered below the pad
        const bool none = m1[t] >= fbits(KEY_PAD);
        const int best = key_col(m1[t]);
        bool ok = !none;
        if constexpr (NODUPES) ok = ok && key_col((uint32_t)m2[t]) == best;
        int16_t v;
        if (a.out_mode == 0)
            v = ok ? (int16_t)(c0 - best) : INVALID_I16;
        else
            v = ok ? (int16_t)best : (int16_t)-1;
        out[c0] = v;
    }
}

constexpr size_t GUIDED_STATIC_LDS = 2 * 8 * sizeof(int);  // wave_span

template <int WORDS, int KS, bool NODUPES, int T>
hipError_t launch_guided_grid(const SearchGuidedArgs& ka, int waves, hipStream_t st) {
    const size_t lds = (size_t)2 * KS * ka.s.chunk * 16;
    const auto kern = search_guided_kernel<WORDS, KS, NODUPES, T>;
    if (lds + GUIDED_STATIC_LDS > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern,
                       dim3(ka.s.rows * ka.s.tiles_per_row), dim3(64 * waves), lds, st, ka);
    return hipGetLastError();
}

template <int WORDS, int KS>
hipError_t launch_guided_w(const SearchGuidedArgs& ka, int T, int waves, bool nodupes,
                           hipStream_t st) {
    if (T == 4)
        return nodupes ? launch_guided_grid<WORDS, KS, true, 4>(ka, waves, st)
                       : launch_guided_grid<WORDS, KS, false, 4>(ka, waves, st);
    return nodupes ? launch_guided_grid<WORDS, KS, true, 2>(ka, waves, st)
                   : launch_guided_grid<WORDS, KS, false, 2>(ka, waves, st);
}

// ------------------------------------------------------------------ the builder

__device__ __forceinline__ float prior_value(const int16_t* p, size_t i, bool, bool& valid) {
    const int16_t v = p[i];
    valid = v != INVALID_I16;
    return (float)v;
}
__device__ __forceinline__ float prior_value(const float* p, size_t i, bool sentinel, bool& valid) {
    const float v = p[i];
    valid = !(v != v) && !(sentinel && v == -32768.0f);
    return v;
}

// one output pixel per lane; block = 64 x GUIDE_BLOCK_ROWS (a wave = 64 pixels of one row)
template <class P>
__global__ __launch_bounds__(64 * GUIDE_BLOCK_ROWS) void guide_kernel(GuideArgs a) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    const int r = blockIdx.y * GUIDE_BLOCK_ROWS + threadIdx.y;
    const bool in = c < a.cols && r < a.rows;
    bool from_prior = false;
    if (in) {
        const P* prior = static_cast<const P*>(a.prior);
        const int pr = min(r / a.scale, a.prows - 1), pc = min(c / a.scale, a.pcols - 1);
        const int r_lo = max(pr - a.spread, 0), r_hi = min(pr + a.spread, a.prows - 1);
        const int c_lo = max(pc - a.spread, 0), c_hi = min(pc + a.spread, a.pcols - 1);
        float vmin = 0.f, vmax = 0.f;
        for (int y = r_lo; y <= r_hi; ++y)
            for (int x = c_lo; x <= c_hi; ++x) {
                bool valid;
                const float v = prior_value(prior, (size_t)y * a.pcols + x, a.sentinel != 0, valid);
                if (!valid) continue;
                vmin = from_prior ? fminf(vmin, v) : v;
                vmax = from_prior ? fmaxf(vmax, v) : v;
                from_prior = true;
            }
        int lo = a.fallback_lo, hi = a.fallback_hi;
        if (from_prior) {
            // floor / ceil in float, clamped to +-32767 before the conversion (infinities too)
            const int fl = (int)fminf(fmaxf(floorf(vmin), -32767.f), 32767.f);
            const int ce = (int)fminf(fmaxf(ceilf(vmax), -32767.f), 32767.f);
            lo = min(max(a.scale * fl - a.radius, -32767), 32767);
            hi = min(max(a.scale * ce + (a.scale - 1) + a.radius, -32767), 32767);
        }
        reinterpret_cast<uint32_t*>(a.guide)[(size_t)r * a.guide_pitch + c] =
            ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
    }
    if (a.counts) {  // one add per wave and count
        const int np = __popcll(__builtin_amdgcn_ballot_w64(in && from_prior));
        const int nf = __popcll(__builtin_amdgcn_ballot_w64(in && !from_prior));
        if (threadIdx.x == 0) {
            if (np) atomicAdd(&a.counts[0], (uint32_t)np);
            if (nf) atomicAdd(&a.counts[1], (uint32_t)nf);
        }
    }
}

}  // namespace

hipError_t launch_search_guided(SearchArgs a, int dmin, int dmax, const int16_t* guide,
                                size_t guide_pitch, int words, bool nodupes, int bits, int cus,
                                hipStream_t st, int tiles, int waves_wg) {
    if (dmin > dmax || !guide) return hipErrorInvalidValue;
    if (a.rows <= 0 || a.cols <= 0) return hipSuccess;
    if (a.cols > 32767 || a.keep || a.row_valid || guide_pitch < (size_t)a.cols)
        return hipErrorInvalidValue;
    const int cols = a.cols;
    // the global window clamped as launch_search_range's: to the disparities a row can hold,
    // one wholly beyond them stays empty (lo > hi), within [-cols, cols]
    SearchGuidedArgs ka;
    ka.dmin = std::min(std::max(dmin, -(cols - 1)), cols);
    ka.dmax = std::max(std::min(dmax, cols - 1), -cols);
    ka.guide = guide;
    ka.guide_pitch = guide_pitch;
    // K-steps, tiles and waves: launch_search_range's rules (search_range.hip)
    int ks = words >= 2 ? words / 2 : 1;
    if (words == 8 && bits > 0 && bits <= 192) ks = 3;
    int T = 2;
    if (tiles) {
        T = tiles >= 4 ? 4 : 2;
    } else {
        for (int t = ks >= 4 ? 2 : 4; t >= 2; t /= 2) {
            const long per_wg = 32L * 8 * t;
            if ((long)a.rows * ((cols + per_wg - 1) / per_wg) >= 2L * (cus > 0 ? cus : 256)) {
                T = t;
                break;
            }
        }
    }
    const int max_waves = waves_wg >= 1 && waves_wg <= 8 ? waves_wg : 8;
    const int waves = std::min(max_waves, (cols + 32 * T - 1) / (32 * T));
    const int per_wg = 32 * waves * T;
    a.tiles_per_row = (cols + per_wg - 1) / per_wg;
    a.tail_T = 0;
    a.tail_col0 = cols;
    // LDS fill: launch_search_range's rule over the GLOBAL window, the one bound on a
    // workgroup's columns the host knows (the kernel stages only the columns its pixels'
    // windows reach): one fill where that fits 80 KiB, else fills of 64 KiB
    long span = std::min<long>(cols, (long)per_wg + ((long)ka.dmax - ka.dmin) + 64);
    span = (std::max<long>(span, 1) + 31) & ~31L;  // whole 32-column blocks
    const int per_col = 2 * ks * 16;
    int chunk = (64 * 1024 / per_col) & ~31;
    if (span < chunk || span <= ((80 * 1024 / per_col) & ~31)) chunk = (int)span;
    if (chunk < 32) chunk = 32;
    a.chunk = chunk;
    ka.s = a;
    switch (words) {
        case 1: return launch_guided_w<1, 1>(ka, T, waves, nodupes, st);
        case 2: return launch_guided_w<2, 1>(ka, T, waves, nodupes, st);
        case 4: return launch_guided_w<4, 2>(ka, T, waves, nodupes, st);
        case 8:
            if (ks == 3) return launch_guided_w<8, 3>(ka, T, waves, nodupes, st);
            return launch_guided_w<8, 4>(ka, T, waves, nodupes, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_guide(const GuideArgs& a, bool f32, hipStream_t st) {
    if (a.rows <= 0 || a.cols <= 0) return hipSuccess;
    if (a.counts) {
        const hipError_t e = hipMemsetAsync(a.counts, 0, 2 * sizeof(uint32_t), st);
        if (e != hipSuccess) return e;
    }
    const dim3 block(64, GUIDE_BLOCK_ROWS);
    const dim3 grid((a.cols + 63) / 64, (a.rows + GUIDE_BLOCK_ROWS - 1) / GUIDE_BLOCK_ROWS);
    if (f32)
        hipLaunchKernelGGL(guide_kernel<float>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(guide_kernel<int16_t>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace bicos_hip
