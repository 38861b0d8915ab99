// search_range.hip -- the bicos Hamming search over a disparity window on the gfx950 matrix
// cores: for the left pixel col0 only the right pixels col1 with dmin <= col0 - col1 <= dmax
// are candidates (reference include/impl/cpu/bicos.hpp:50-76 run over that set, in ascending
// col1). Same FP4 Hamming products, workgroup layout and LDS staging as search_mx_kernel
// (search_mx.hip, whose header comment derives the scheme); what differs:
//
//  * Block skipping. A wave's T tiles cover col0 [c0_lo, c0_hi]; it multiplies only the
//    32-col1 blocks that intersect [c0_lo - dmax, c0_hi - dmin] (clipped to the image), and
//    the workgroup stages only the columns of the union of its waves' spans. All bounds are
//    wave-uniform (SGPRs).
//  * Masking. A (tile, block) pair whose 32 x 32 pairs all lie inside the window uses the
//    plain key matrix C; one that straddles an edge of the window (or of the image) sets
//    C = KEY_PAD for the first-minimum product and C = -KEY_PAD for the negated one wherever
//    the pair is outside, element by element (lane l: col0 = c0_tile + (l & 31); register r:
//    col1 = B + (r & 3) + 8 (r >> 2) + 4 (l >> 5)); pairs fully outside are skipped. Unlike
//    the columns past the image that search_mx_kernel's partial block pads (A = 0 there), a
//    masked pair inside the image still has its product +-x in the accumulator, so the
//    negated key of a masked pair is -x - 1e30 < 0 and the last-minimum reduction is a
//    SIGNED integer maximum (positive floats order like their bits as signed integers too,
//    negative ones fall below all of them).
//  * Keys. The absolute float keys of search_mx_kernel's KEYS 0: C = 256 + col1 * 2^-15 and,
//    for NoDuplicates, a second product with the right operand negated. They do not depend
//    on the block order and hold for every cols <= 32767.
//  * No candidate. A pixel whose window holds no column leaves its running minimum at its
//    initial value (or at KEY_PAD, from masked pairs): tested before the key is decoded.
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

// A workgroup = one row x the col0 range [tile * waves * T * 32, + waves * T * 32); a.chunk
// col1 per LDS fill (multiple of 32), fills start at the first 32-col1 block of the
// workgroup's span. ka.dmin / ka.dmax within [-cols, cols] (launch_search_range).
template <int WORDS, int KS, bool NODUPES, int T>
__global__ __launch_bounds__(512) void search_range_kernel(SearchRangeArgs ka) {
    const SearchArgs& a = ka.s;
    static_assert(KS >= 1 && 2 * KS <= (WORDS >= 2 ? WORDS : 2), "K-steps exceed the descriptor");
    constexpr int WL = 2 * KS;  // LDS word slots per col1 (W=1: 1 pad)
    extern __shared__ __attribute__((aligned(16))) v4i lds_rg[];  // [WL][chunk]

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

    // B fragments: +1 (0x2) where the left bit is 0, -1 (0xA) where it is 1
    v4i bf[T][KS];
    // lowest disparity of this lane's col0 that stays inside the image on the right
    // (col1 <= cols - 1), joined with dmin: the mask's lower bound
    int dlo_lane[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int c0 = c0_wave + 32 * t + j;
        dlo_lane[t] = max(dmin, c0 - (cols - 1));
#pragma unroll
        for (int s = 0; s < KS; ++s) bf[t][s] = expand_bits(desc_word<WORDS, KS>(row0, c0, 2 * s + h, c0 < cols), LUT_B);
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

    // col1 spans (inclusive, clipped to the image; empty when lo > hi): the workgroup's
    // and this wave's
    const int wg_hi0 = min(cols, wg_c0 + waves * T * 32) - 1;
    const int wg_lo1 = max(0, wg_c0 - dmax), wg_hi1 = min(cols - 1, wg_hi0 - dmin);
    const bool idle = c0_wave >= cols;  // wave-uniform; still joins the barriers
    const int wv_hi0 = min(cols, c0_wave + T * 32) - 1;
    const int wv_lo1 = max(0, c0_wave - dmax), wv_hi1 = min(cols - 1, wv_hi0 - dmin);
    const int stage0 = wg_lo1 & ~31;  // first staged column
    const int nchunks = wg_hi1 >= wg_lo1 ? (wg_hi1 - stage0) / chunk + 1 : 0;

    // C of the block being multiplied: BIAS + col1 * EPS, advanced by 32 * EPS per block
    // (exact: col1 < 32768 keeps 256 + col1 * 2^-15 within 24 bits)
    v16f cc;
#pragma unroll
    for (int r = 0; r < 16; ++r) cc[r] = KEY_BIAS + (float)((wv_lo1 & ~31) + rrow(r)) * KEY_EPS;
    int bc = wv_lo1 & ~31;  // the block base cc stands at

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
                lds_rg[w * chunk + c] = expand_bits(desc_word<WORDS, KS>(row1, c1, w, c1 < cols), LUT_A);
            }
        }
        __syncthreads();
        if (idle || wv_hi1 < wv_lo1) continue;

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
            for (int s = 0; s < KS; ++s) af[s] = lds_rg[(2 * s + h) * chunk + (B - base) + j];
            if constexpr (NODUPES) {
#pragma unroll
                for (int s = 0; s < KS; ++s)
#pragma unroll
                    for (int q = 0; q < 4; ++q) an[s][q] = af[s][q] | (af[s][q] << 2);  // 1.0 -> -1.0
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int c0_t = c0_wave + 32 * t;
                // disparities of the tile's pairs with this block: [c0_t - B - 31, c0_t - B + 31]
                const int d_lo = c0_t - B - 31, d_hi = c0_t - B + 31;
                if (c0_t >= cols || d_hi < dmin || d_lo > dmax) continue;  // fully outside
                // which edges of the window cut through the pair (wave-uniform): the lower
                // one (or the image's right edge), the upper one; neither = wholly inside
                const bool cut_lo = d_lo < dmin || B + 32 > cols;
                const bool cut_hi = d_hi > dmax;
                v16f c1 = cc, c2 = cc;
                if (cut_lo || cut_hi) {
                    // register r's pair has disparity dl - off(r), off(r) = (r & 3) + 8 (r >> 2)
                    // a constant: inside iff off(r) <= dl - lower bound and off(r) >= dl - dmax.
                    // A pair cut by one edge only (every window of >= 63 disparities) pays
                    // one compare per element.
                    const int dl = c0_t + j - B - 4 * h;
                    const int off_max = dl - dlo_lane[t], off_min = dl - dmax;
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
    if (idle) return;

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

template <int WORDS, int KS, bool NODUPES, int T>
hipError_t launch_range_grid(const SearchRangeArgs& ka, int waves, hipStream_t st) {
    const size_t lds = (size_t)2 * KS * ka.s.chunk * 16;
    const auto kern = search_range_kernel<WORDS, KS, NODUPES, T>;
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern,
                       dim3(ka.s.rows * ka.s.tiles_per_row), dim3(64 * waves), lds, st, ka);
    return hipGetLastError();
}

template <int WORDS, int KS>
hipError_t launch_range_w(const SearchRangeArgs& ka, int T, int waves, bool nodupes,
                          hipStream_t st) {
    if (T == 4)
        return nodupes ? launch_range_grid<WORDS, KS, true, 4>(ka, waves, st)
                       : launch_range_grid<WORDS, KS, false, 4>(ka, waves, st);
    return nodupes ? launch_range_grid<WORDS, KS, true, 2>(ka, waves, st)
                   : launch_range_grid<WORDS, KS, false, 2>(ka, waves, st);
}

}  // namespace

hipError_t launch_search_range(SearchArgs a, int dmin, int dmax, int words, bool nodupes,
                               int bits, int cus, hipStream_t st, int tiles, int waves_wg) {
    if (dmin > dmax) return hipErrorInvalidValue;
    if (a.rows <= 0 || a.cols <= 0) return hipSuccess;
    if (a.cols > 32767 || a.keep || a.row_valid) return hipErrorInvalidValue;
    const int cols = a.cols;
    // the window clamped to the disparities a row can hold, [-(cols-1), cols-1]; one that
    // lies wholly beyond them stays empty (lo > hi), within [-cols, cols]
    SearchRangeArgs ka;
    ka.dmin = std::min(std::max(dmin, -(cols - 1)), cols);
    ka.dmax = std::max(std::min(dmax, cols - 1), -cols);
    // 64-bit K-steps: all of the descriptor unless the bits past `bits` are known zero
    int ks = words >= 2 ? words / 2 : 1;
    if (words == 8 && bits > 0 && bits <= 192) ks = 3;
    // 8 waves x 4 tiles (2 for 4-step 256-bit descriptors: 4 tiles take 175 VGPRs with
    // NoDuplicates, two waves per SIMD), fewer tiles when the grid would not give every CU
    // about two workgroups, fewer waves for rows narrower than a workgroup
    // (tiles / waves_wg != 0: the caller's choice, as bicos_engine_tune's for the full-row
    // search -- 2 or 4 tiles, up to 8 waves)
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
    // LDS fill: the columns one workgroup can need (its col0 range widened by the window,
    // plus the partial blocks at both ends) in ONE fill where they fit 80 KiB of expanded
    // descriptors (two workgroups per CU; cfg2 with a 128-wide window: 1216 columns, 76 KiB --
    // a second fill makes every wave wait at its barriers for columns only the last wave
    // reads), else fills of 64 KiB
    long span = std::min<long>(cols, (long)per_wg + ((long)ka.dmax - ka.dmin) + 64);
    span = (std::max<long>(span, 1) + 31) & ~31L;  // whole 32-column blocks
    const int per_col = 2 * ks * 16;
    int chunk = (64 * 1024 / per_col) & ~31;
    if (span < chunk || span <= ((80 * 1024 / per_col) & ~31)) chunk = (int)span;
    if (chunk < 32) chunk = 32;
    a.chunk = chunk;
    ka.s = a;
    switch (words) {
        case 1: return launch_range_w<1, 1>(ka, T, waves, nodupes, st);
        case 2: return launch_range_w<2, 1>(ka, T, waves, nodupes, st);
        case 4: return launch_range_w<4, 2>(ka, T, waves, nodupes, st);
        case 8:
            if (ks == 3) return launch_range_w<8, 3>(ka, T, waves, nodupes, st);
            return launch_range_w<8, 4>(ka, T, waves, nodupes, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace bicos_hip
