// search_dev.hpp -- device pieces shared by the matrix-core search kernels (search_mx.hip,
// search_pk.hip, search_range.hip): the workgroup -> (row, tile) mappings, the compacted (LIST)
// col0 prologue and the dense-row fast path, the descriptor words behind the MFMA fragments
// and the fused agree epilogue.
#pragma once

#include "kernels.hpp"
#include "nxc.hpp"
#include "search_mx_common.hpp"
#include "search_plan.hpp"
#include "stack.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace bicos_hip {

namespace {

// (row, tile) of a workgroup of an uncompacted launch of rows x tiles_per_row workgroups, in
// XCD-aware order: the tiles of one row on one XCD (shared right row in its L2)
__device__ __forceinline__ void xcd_row_tile(int tiles_per_row, int& row, int& tile) {
    const int nwg = gridDim.x;
    const int bid = blockIdx.x;
    const int per_xcd = (nwg + 7) / 8;
    int logical = (bid % 8) * per_xcd + bid / 8;
    if (nwg % 8 != 0) logical = bid;
    row = logical / tiles_per_row;
    tile = logical % tiles_per_row;
}

// Word w of the descriptor of column c of `row` (WORDS words each), 0 where !in or w is past
// the descriptor (a K-step's pad slot). Bit 255 of a 256-bit descriptor multiplied in all 4
// K-steps is masked on both sides: the keys' |x| <= 255 needs it, and transform descriptors
// use at most 254 bits.
template <int WORDS, int KS>
__device__ __forceinline__ uint32_t desc_word(const uint32_t* __restrict__ row, int c, int w, bool in) {
    uint32_t x = 0;
    if (in && w < WORDS) x = row[(size_t)c * WORDS + w];
    if (WORDS == 8 && KS == 4 && w == 7) x &= 0x7FFFFFFFu;
    return x;
}
// LIST: the col0 of row r are the distinct col1 >= 0 of row r of a.keep (Consistency's reverse
// search over the col1 its forward search kept, engine.cpp reverse_search), in ascending
// order: entry i is the i-th of them. The workgroup finds its own entries in a prologue
// (list_prologue); a workgroup's col0 ranges then run over i, workgroups past the row's count exit,
// and the block order starts REV_AHEAD columns above the wave's highest entry (a reverse
// match lies at col0 = col1 + d, d >= 0 in a rectified pair). The tail split is the full
// search's, in entry space: the main launch takes entries below tail_col0, the tail launch
// the rest (a dense row then costs what it does uncompacted: without the tail, the 4th
// workgroup of a 3300-column row ran 228 entries for a whole-row scan, planted stereo
// NODUPES|CONSISTENCY 2.38 vs 2.24 ms).

// Consistency's compacted reverse search, the reference's rule (bicos.hpp:94-101,
// bicos.cuh:114,124-131: the reverse search runs only where the forward one found a valid
// match), computed by each workgroup for its own row: the distinct col1 >= 0 of the forward
// result `f` (cols entries) marked in an LDS bitmap, a scan of the words' popcounts, and the
// columns of entries [e0, e0 + ne) written into `ent` by the threads owning their words.
// Returns the row's entry count (workgroup-uniform). Every thread of the workgroup must call
// it (barriers). Run as a separate kernel writing a list to HBM first it cost 18 us per cfg4
// frame; here it overlaps the other resident workgroup's matrix-core work.
[[maybe_unused]] __device__ int list_prologue(const int16_t* __restrict__ f, int cols,
                                              uint32_t* scratch, int16_t* ent, int e0, int ne) {
    const int tid = threadIdx.x, bs = blockDim.x;
    const int nw = (cols + 31) >> 5;
    uint32_t* bits = scratch;
    int* wsum = (int*)(scratch + 1024);
    for (int w = tid; w < nw; w += bs) bits[w] = 0u;
    for (int i = tid; i < ne; i += bs) ent[i] = 0;  // entries past the row's count
    __syncthreads();
    // mark: 8 forward results per thread and 16-byte load where the row is aligned (it is
    // when cols % 8 == 0); a run of results in one bitmap word is one LDS atomic (a stereo
    // row's col1 ascend with col0, so most threads issue one or two)
    auto mark8 = [&](const int (&v)[8]) {
        int cw = -1;
        uint32_t m = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (v[k] < 0) continue;
            const int w = v[k] >> 5;
            if (w != cw) {
                if (cw >= 0) atomicOr(&bits[cw], m);
                cw = w;
                m = 0u;
            }
            m |= 1u << (v[k] & 31);
        }
        if (cw >= 0) atomicOr(&bits[cw], m);
    };
    if ((reinterpret_cast<uintptr_t>(f) & 15u) == 0) {
        for (int c = 8 * tid; c < cols; c += 8 * bs) {
            int v[8];
            if (c + 8 <= cols) {
                const v4i x = *reinterpret_cast<const v4i*>(f + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[2 * k] = (int)(int16_t)(x[k] & 0xFFFF);
                    v[2 * k + 1] = (int)(int16_t)((uint32_t)x[k] >> 16);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = c + k < cols ? (int)f[c + k] : -1;
            }
            mark8(v);
        }
    } else {
        for (int c = 8 * tid; c < cols; c += 8 * bs) {
            int v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = c + k < cols ? (int)f[c + k] : -1;
            mark8(v);
        }
    }
    __syncthreads();
    // thread t owns words [t q, t q + q): popcounts, a wave scan and the wave sums give its
    // first entry index; it writes the columns of its set bits that fall in [e0, e0 + ne)
    const int q = (nw + bs - 1) / bs;
    int mine = 0;
    for (int k = 0; k < q; ++k) {
        const int w = tid * q + k;
        mine += w < nw ? __popc(bits[w]) : 0;
    }
    const int lane = tid & 63, wave = tid >> 6, nwaves = bs >> 6;
    int incl = mine;
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const int y = __shfl_up(incl, sh);
        if (lane >= sh) incl += y;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < nwaves; ++w) {
        const int v = wsum[w];
        before += w < wave ? v : 0;
        total += v;
    }
    int e = before + incl - mine;
    if (e < e0 + ne && e + mine > e0) {
        for (int k = 0; k < q; ++k) {
            const int w = tid * q + k;
            uint32_t x = w < nw ? bits[w] : 0u;
            while (x) {
                const int b = __builtin_ctz(x);
                x &= x - 1u;
                if (e >= e0 && e < e0 + ne) ent[e - e0] = (int16_t)(32 * w + b);
                ++e;
            }
        }
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(total);
}
// (row, tile) of a compacted (LIST) launch: grid = 8 x ceil(R8 / G) G x tiles_per_row, R8 =
// ceil(rows / 8), G = LIST_GROUP rows. XCD x = bid % 8 owns rows [x R8, (x + 1) R8), and
// within the XCD the order is tile-major per group of G rows: the group's tile 0 workgroups,
// then its tile 1 workgroups, ... Row-major order put the workgroups past a row's count --
// which exit at once -- in a fixed pattern (tiles 2 and 3 of every row at 52 % kept), and the
// dispatcher then ran the live ones on a fixed subset of the CUs: a 52 % list took as long
// as the whole row (random u128, profiles/reverse_search_r05.jsonl). Tile-major over all of
// the XCD's rows fixed that but put a row's workgroups hundreds of workgroups apart, past
// the XCD's L2 (cfg4's reverse search +4.5 %); a group of G = 32 rows x 2 tiles is what an
// XCD holds at once (32 CUs x 2 workgroups), so a row's workgroups run together again.
// Rows past the XCD's range (or past rows) exit.
__device__ __forceinline__ void list_row_tile(int tiles_per_row, int rows, int& row, int& tile) {
    const int r8 = (rows + 7) / 8;
    const int j = blockIdx.x / 8;
    const int per_group = LIST_GROUP * tiles_per_row;
    const int g = j / per_group, w = j % per_group;
    tile = w / LIST_GROUP;
    const int r = g * LIST_GROUP + w % LIST_GROUP;  // row within the XCD's range
    row = r < r8 ? (blockIdx.x % 8) * r8 + r : rows;
}
// Consistency's dense-row fast path (SearchArgs.row_valid): the compacted reverse search's
// workgroup sums its row's per-tile valid counts, written by the forward search's epilogue
// (tile_valid_store), in every wave -- a workgroup-uniform answer without a barrier. A row
// whose forward search kept >= 7/8 of its col0 skips list_prologue (one dependent read of
// the whole forward row, an LDS bitmap and a scan: ~9 us per cfg4 frame, where 98 % of the
// columns are kept) and searches its col0 in order -- every rev the check could read is
// then computed, plus a few it does not read.
__device__ __forceinline__ bool dense_row(const SearchArgs& a, int row) {
    const uint8_t* v = a.row_valid + (size_t)row * a.valid_pitch;
    const int nt = (a.cols + 31) >> 5;
    const int lane = threadIdx.x & 63;
    int sum = 0;
    for (int i = lane; i < nt; i += 64) sum += v[i];
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) sum += __shfl_xor(sum, sh);
    return __builtin_amdgcn_readfirstlane(sum) * 8 >= 7 * a.cols;
}
// forward search epilogue, dense-row fast path: the valid results of one 32-col0 tile (the
// 32 lanes of this lane's half-wave, lane & 31 = col0 % 32) whose col1 `best` lies above the
// previous col0's (a rectified stereo row's matches ascend with col0, so the count stands for
// the DISTINCT col1 the reverse search needs; random descriptors, whose every col0 may be
// valid, count about half), counted into row_valid[row][c0_tile / 32] by the half's writer
__device__ __forceinline__ void tile_valid_store(const SearchArgs& a, int row, int c0_tile,
                                                 bool valid, int best, bool writer) {
    const int v = valid ? best : -1;
    const int prev = __shfl_up(v, 1, 32);  // (the half's first lane: its own value)
    const bool first = (threadIdx.x & 31) == 0;
    const uint64_t bal = __builtin_amdgcn_ballot_w64(valid && (first || v > prev));
    const uint32_t half = (threadIdx.x & 32) ? (uint32_t)(bal >> 32) : (uint32_t)bal;
    if (writer && c0_tile < a.cols)
        a.row_valid[(size_t)row * a.valid_pitch + (c0_tile >> 5)] = (uint8_t)__popc(half);
}

// LIST block order: a wave's blocks start REV_AHEAD columns above its highest entry, a
// workgroup's chunks at the chunk of its highest entry, with no columns ahead. Starting the
// chunks 64 columns up as well sent every wave through the chunk above first, where only the
// top few entries have their matches: dense rows (planted / low-texture NODUPES|CONSISTENCY
// at 3300 columns) 2.37 / 2.38 ms vs 2.30 / 2.25 (REV_AHEAD 0 / 32: planted 2.35 / 2.32;
// profiles/reverse_search_r05.jsonl)
#ifndef BICOS_REV_AHEAD
#define BICOS_REV_AHEAD 64
#endif
constexpr int REV_AHEAD = BICOS_REV_AHEAD;

// The agree stage (kernels.hip agree_reg_kernel, reference agree.hpp:53-93: NXC of the n left
// samples at col and the n right ones at col - d, invalid below the threshold) for the cnt
// col0 from c0 of one row whose integer disparities the workgroup holds in LDS, u8 stacks,
// float, n = N exactly: the search_mx_kernel AG epilogue. Same arithmetic, order and outputs
// as agree_reg_kernel<uint8_t, float, N, true>, so the two are interchangeable bit for bit.
// (Staging the left samples in LDS with dword loads and gathering two pixels' right samples
// per thread before either's arithmetic, as agree_lds_kernel does, measured slower here:
// the fused launch 351 vs 345 us at cfg2, profiles/fused_agree_r05.jsonl.)
template <int N>
__device__ __forceinline__ void fused_agree(const AgreeArgs& g, int row, int c0, int cnt,
                                            const int16_t* raw) {
    const StackReader<uint8_t> rd0(g.stack0, g.stack_bytes), rd1(g.stack1, g.stack_bytes);
    const uint32_t rowoff = (uint32_t)row * (uint32_t)g.row_pitch;
    const uint32_t pp = (uint32_t)g.plane_pitch;
    const int cols = g.cols;
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
        const int col = c0 + i;
        int d = raw[i];
        const int idx1 = col - d;
        const bool inb = d != INVALID_I16 && idx1 >= 0 && idx1 < cols;
        uint32_t l[N], r[N];
        uint32_t sl = 0, sr = 0;
#pragma unroll
        for (int t = 0; t < N; ++t) l[t] = rd0((uint32_t)col, rowoff + (uint32_t)t * pp);
        const uint32_t c1 = inb ? (uint32_t)idx1 : (uint32_t)col;
#pragma unroll
        for (int t = 0; t < N; ++t) r[t] = rd1(c1, rowoff + (uint32_t)t * pp);
#pragma unroll
        for (int t = 0; t < N; ++t) {
            sl += l[t];
            sr += r[t];
        }
        float corr = __builtin_nanf("");
        if (inb) {
            const float m0 = nxc::div_p((float)sl, (float)N);
            const float m1 = nxc::div_p((float)sr, (float)N);
            float cov = 0.f, v0 = 0.f, v1 = 0.f;
#pragma unroll
            for (int t = 0; t < N; ++t) {
                const float x0 = (float)l[t] - m0;
                const float x1 = (float)r[t] - m1;
                cov = nxc::fma_p(x0, x1, cov);
                v0 = nxc::fma_p(x0, x0, v0);
                v1 = nxc::fma_p(x1, x1, v1);
            }
            if (g.has_minvar && (v0 < g.minvar || v1 < g.minvar))
                corr = -1.f;
            else
                corr = nxc::div_p(cov, nxc::sqrt_p(v0 * v1));
            if (corr < g.threshold) d = INVALID_I16;  // NaN passes, as in the reference
        } else {
            d = INVALID_I16;
        }
        const size_t o = (size_t)row * cols + col;
        if (g.out_f32)
            ((float*)g.out)[o] = (float)d;
        else
            ((int16_t*)g.out)[o] = (int16_t)d;
        if (g.corrmap) ((float*)g.corrmap)[o] = corr;
    }
}
// kernel arguments: SearchArgs, plus the agree's for the fused (AG) instantiations only
template <bool AG> struct SearchKArgs { using type = SearchArgs; };
template <> struct SearchKArgs<true> { using type = SearchAgreeArgs; };
__device__ __forceinline__ const SearchArgs& search_part(const SearchArgs& k) { return k; }
__device__ __forceinline__ const SearchArgs& search_part(const SearchAgreeArgs& k) { return k.s; }
// kernel arguments of a launch: the search's, plus the agree's for AG
template <bool AG>
typename SearchKArgs<AG>::type kernel_args(const SearchArgs& a, const AgreeArgs* ag) {
    if constexpr (AG)
        return SearchAgreeArgs{a, *ag};
    else
        return a;
}

// A runtime value to a template argument: calls f(std::integral_constant<T, X>{}) for the X
// among Xs that equals v; hipErrorInvalidValue when v is none of them.
template <class T, T... Xs, class F>
hipError_t pick(T v, F&& f) {
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Xs ? (e = f(std::integral_constant<T, Xs>{}), true) : false) || ...);
    return e;
}

// Launches `kern` as planned: l's grid, block and dynamic LDS (raised past 64 KiB where
// needed), the search's arguments plus the agree's for an AG instantiation.
template <bool AG, class K>
hipError_t launch_planned(K kern, const SearchLaunch& l, const SearchArgs& a, const AgreeArgs* ag,
                          hipStream_t st) {
    if (l.lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kern,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.block), l.lds, st, kernel_args<AG>(a, ag));
    return hipGetLastError();
}

}  // namespace

}  // namespace bicos_hip
