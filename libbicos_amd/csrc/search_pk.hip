// search_pk.hip -- the bicos Hamming search (reference include/impl/cpu/bicos.hpp:50-113) on the
// gfx950 matrix cores with packed keys: NoDuplicates, descriptors with <= 127 used bits in
// 32/64/128-bit words. Same FP4 products, workgroup layout and LDS staging as search_mx_kernel
// (search_mx.hip, whose header comment derives the scheme); what differs is the key.
//
// The one-product search spends most of its VALU issue on the first-minimum trees: one v_min3_u32
// per two keys, one key per accumulator register. Here every accumulator register carries
// TWO Hamming distances, and the tree runs on gfx950's v_pk_minimum3_f16 (half rate, four
// keys per instruction; profiles/valu_rates_r03.jsonl), so the reduction per pair halves.
// The keys carry no column: per col0 a wave keeps the running minimum, a tie marker and the
// block that holds the minimum, and finds the column inside that block.
//
// The map -- each scheme is described once, at the function that implements it:
//   mfma_pk                 packed keys and operands: what one product leaves in an accumulator
//   pk_tree, pk_row_keys    the block's minimum; (distance, row) keys of the drop branch
//   pk_bfrags, pk_cb, pk_rrow, pk_pad, pk_product
//                           the prologue and the full product of a block, for both kernels
//   lazy_drop               the pair step: block minimum against running minimum; lazy drops
//   pk_rescan, pk_copy_row, pk_result, pk_agree, pk_end_of_row
//                           the end of a row, for both kernels
//   search_pk_kernel        1/2/4 words, 1/2/4 wide tiles, tail and list launches, the drop
//                           branch (pair_step) or lazy drops
//   pkp_mix                 which 32 descriptor bits each product of the pruned search holds
//   search_pkp_kernel       the pruned 128-bit search: ST at its staging (raw_col), pruning and
//                           the fallback at block_pr, EOR at pair_update and its end of row
//   launch_pk_variant       the instantiations that are built
#include "search_dev.hpp"

#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace bicos_hip {

namespace {

constexpr uint32_t LUT_PA = 0xAAA22A22u;  // right: bit 0 -> +1.0 (0x2), 1 -> -1.0 (0xA)
constexpr uint32_t LUT_PB = 0x11199199u;  // left: bit 0 -> -0.5 (0x9), 1 -> +0.5 (0x1)
constexpr int PK_SCALE_HI = 127 + 16;     // E8M0 2^16 for the K-half-0 (col0 P) lanes
constexpr uint32_t PK_PAD = 0x7BFF7BFFu;  // the largest finite f16 in both fields
// search_pkp_kernel's reach test: thr = R + 33 per field, so that the saturated thr - lb is 0
// exactly where ham_lo lies above the running minimum (a probe of products 0 and 1, that is of
// words 0 and 1); R + 49 where the probe is product 0 alone
constexpr uint32_t PKP_THR = 0x00210021u;
constexpr uint32_t PKP_THR1 = 0x00310031u;
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));

// v_pk_minimum3_f16 on two packed positive f16 keys per register
__device__ __forceinline__ uint32_t pkmin3(uint32_t a, uint32_t b, uint32_t c) {
    const h2 x = __builtin_bit_cast(h2, a), y = __builtin_bit_cast(h2, b), z = __builtin_bit_cast(h2, c);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_minimum(__builtin_elementwise_minimum(x, y), z));
}
__device__ __forceinline__ uint32_t pkminu(uint32_t a, uint32_t b) {  // v_pk_min_u16
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a),
                                                                  __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pksub(uint32_t a, uint32_t b) {  // v_pk_sub_u16 (wraps)
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ uint32_t pksubsat(uint32_t a, uint32_t b) {  // v_pk_sub_u16 clamp: max(a - b, 0)
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a),
                                                                      __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pksign(uint32_t a) {  // 0xFFFF per field with its top bit set
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(i16x2, a) >> (short)15);
}
__device__ __forceinline__ uint32_t bfi(uint32_t mask, uint32_t a, uint32_t b) {
    return (a & mask) | (b & ~mask);
}

// Packed keys and operands. Right A = 1 - 2b in {+1, -1}, left B = -(1 - 2a) / 2 in {-0.5,
// +0.5} (both exact FP4 e2m1), so one K position contributes -(1 - 2a)(1 - 2b) / 2 and K
// positions sum to ham - K / 2 (K = 32 WORDS, the zero bits past the used ones included: they
// add the same -1/2 to every pair). One MFMA multiplies the 32 bits of ONE product -- in
// search_pk_kernel descriptor word w, in search_pkp_kernel the 32 bits pkp_mix gives product w;
// any fixed 32 of the descriptor's bit positions do, the same in both operands: the B lanes of
// K-half 0 hold them of col0 P, those of K-half 1 of col0 Q = P + 32, and the E8M0
// scale sb of the K-half-0 lanes is 2^16. With C = 2^23 + 2^16 (K/2) + 0x4B00 + K/2 (pk_cb)
// every D is an integer in [2^23, 2^24) (ulp 1), so
//     bits(D) = 0x4B000000 + 2^16 ham(P, col1) + 0x4B00 + ham(Q, col1)
// exactly: the high half is 0x4B00 + ham_P, the low half 0x4B00 + ham_Q, both positive normal
// f16 values whose order is the order of the distances (ham <= 127 keeps each in 7 bits; the
// partial sums of the first products stay inside [0, 127] too). WORDS MFMAs cover 32 col1 x 64
// col0 pairs: the same matrix-core work per pair as the one-product keys.
__device__ __forceinline__ v16f mfma_pk(v4i a, v4i b, v16f c, int sb) {
    const v8i a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0};
    const v8i b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, 127, 0, sb);
}

// minimum over the 16 packed keys of a D tile (v_pk_minimum3_f16 tree, 8 instructions)
__device__ __forceinline__ uint32_t pk_tree(const v16f& d) {
    auto k = [&](int r) { return fbits(d[r]); };
    const uint32_t a0 = pkmin3(k(0), k(1), k(2)), a1 = pkmin3(k(3), k(4), k(5));
    const uint32_t a2 = pkmin3(k(6), k(7), k(8)), a3 = pkmin3(k(9), k(10), k(11));
    const uint32_t a4 = pkmin3(k(12), k(13), k(14));
    return pkminu(pkmin3(a0, a1, a2), pkmin3(a3, a4, k(15)));
}
// (distance, row) keys of ONE distance field of a D tile, minimum over this lane half's
// rows: low half distance * 256 + row, high half distance * 256 + (31 - row), row = (r & 3)
// + 8 (r >> 2) (the lane half's 4h is added by the caller) -- the first and the LAST row
// at the minimum distance in one v_pk_min_u16 tree. SEL picks the distance byte of D
// (byte 2: ham_P, byte 0: ham_Q).
template <uint32_t SEL>
__device__ __forceinline__ uint32_t pk_row_keys(const v16f& d) {
    uint32_t k[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t row = (uint32_t)((r & 3) + 8 * (r >> 2));
        // bytes: [row, ham, 31 - row, ham]
        k[r] = __builtin_amdgcn_perm(fbits(d[r]), row | ((31u - row) << 8), SEL);
    }
#pragma unroll
    for (int s = 1; s < 16; s *= 2)
#pragma unroll
        for (int r = 0; r < 16; r += 2 * s) k[r] = pkminu(k[r], k[r + s]);
    return k[0];
}
constexpr uint32_t PK_SEL_P = 0x06010600u;
constexpr uint32_t PK_SEL_Q = 0x04010400u;

// ---- the prologue and the full product of a block

// B fragments: wide tile t, word w; this lane's col0 is entry c0_wave + 64 t + lane of the
// row's lcols, column lcol(entry) (K-half h: P = lanes 0-31, Q = lanes 32-63)
template <int WORDS, int T, class LCOL>
__device__ __forceinline__ void pk_bfrags(v4i (&bf)[T][WORDS], const uint32_t* __restrict__ row0,
                                          int c0_wave, int lane, int lcols, LCOL lcol) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int c0 = c0_wave + 64 * t + lane;
        const int cl = c0 < lcols ? lcol(c0) : 0;
#pragma unroll
        for (int w = 0; w < WORDS; ++w) {
            const uint32_t x = c0 < lcols ? row0[(size_t)cl * WORDS + w] : 0u;
            bf[t][w] = expand_bits(x, LUT_PB);
        }
    }
}
// the products' C (see mfma_pk), in all 16 accumulator registers
template <int WORDS>
constexpr float PK_CBIAS = 8388608.f + 65536.f * (16 * WORDS) + (float)(0x4B00 + 16 * WORDS);
template <int WORDS>
__device__ __forceinline__ v16f pk_cb() {
    v16f cb;
#pragma unroll
    for (int r = 0; r < 16; ++r) cb[r] = PK_CBIAS<WORDS>;
    return cb;
}
// the block row (col1 offset in the block) of accumulator register r in lane half h: half 0
// owns rows 0-3, 8-11, 16-19, 24-27 of the block, half 1 the others: bit 2 of the row. (As
// an OR: with "+ 4 h" the compiler folds the sum into pk_pad's compare, and the registers of
// all but a few instantiations move, next_free_vgpr 80 -> 96 for <2, 2, *, *, false, true>.)
__device__ __forceinline__ int pk_rrow(int r, int h) { return ((r & 3) + 8 * (r >> 2)) | (4 * h); }
// Columns beyond the image in the partial block (block bi of a step with ncols columns) are set
// to 0x7BFF (the largest finite f16) before the tree.
__device__ __forceinline__ void pk_pad(v16f& dx, v16f& dy, int bi, int ncols, int h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const bool in = 32 * bi + pk_rrow(r, h) < ncols;
        dx[r] = in ? dx[r] : bitsf(PK_PAD);
        dy[r] = in ? dy[r] : bitsf(PK_PAD);
    }
}
// the full product of one block (its fragments af) for a pair of wide tiles x / y: WORDS
// MFMAs per tile (TWO false: one tile, dy = dx)
template <int WORDS, bool TWO>
__device__ __forceinline__ void pk_product(const v4i (&af)[WORDS], const v4i (&bx)[WORDS],
                                           const v4i (&by)[WORDS], const v16f& cb, int sb, v16f& dx,
                                           v16f& dy) {
    dx = mfma_pk(af[0], bx[0], cb, sb);
    dy = dx;
    if constexpr (TWO) dy = mfma_pk(af[0], by[0], cb, sb);
#pragma unroll
    for (int w = 1; w < WORDS; ++w) {
        dx = mfma_pk(af[w], bx[w], dx, sb);
        if constexpr (TWO) dy = mfma_pk(af[w], by[w], dy, sb);
    }
}

// ---- the pair step

// Per wide tile (64 col0) and block (32 col1) the tree gives the block's minimum distance per
// col0 (both lane halves combined by one v_permlane32_swap per two tiles, as in pair_reduce):
// comb, and diff = comb - R against the running minimum R (packed, per col0):
//   block > R: nothing;  block == R: a second column at the running minimum -> duplicate
//   (tracked as M = min over blocks of (block - R), packed; 0 = tie); block < R: a new
//   minimum, a strict drop, which resets M. Any block order gives the same result (a tie with
//   a later-improved minimum is forgotten on the improvement, exactly as the reference's
//   strict '<' scan would).
// Lazy drops (round 6). A strict drop of the running minimum used to branch into (distance,
// row) key trees that found its first row and whether the block holds it twice (the drop
// branch of search_pk_kernel's pair_step) -- one wave-uniform branch whenever any of the
// wave's 128 col0 dropped, ~150 VALU; on random descriptors most blocks of a scan take it. A
// lazy drop only records the block base B in C and clears the tie marker, branch-free, and
// each col0 rescans its final block once after the scan, from the right row's raw words staged
// in LDS: 32 popcounts of WORDS words, the first col1 at the minimum and whether it occurs
// twice (pk_rescan). The plan chooses per shape (PK_LAZY_MIN_COLS, search_plan.hpp).
__device__ __forceinline__ void lazy_drop(uint32_t& M, uint32_t& R, uint32_t& C, uint32_t comb,
                                          uint32_t diff, int B) {
    const uint32_t mi = pksign(diff);
    M = pkminu(M, diff) | mi;  // a drop: no tie seen since
    // (bfi(mi, comb, R) as the one v_bitop3_b32 it should be: from bfi()'s and/or form the
    // compiler rebuilt the per-field select here from two compares, two cndmasks and a v_perm,
    // and from the xor form it kept a v_xor_b32 beside the v_bitop3_b32 in the 4-tile loops)
    R = __builtin_amdgcn_bitop3_b32(comb, R, mi, 0xe4);
    // (one v_bfi_b32 with the block base as an SGPR operand: left alone, the compiler rebuilt
    // this select the same way)
    asm("v_bfi_b32 %0, %1, %2, %0" : "+v"(C) : "v"(mi), "s"((uint32_t)B * 0x10001u));
}

// ---- the end of a row

// a wave's place in its row, as the end of row needs it: image row; lane half, lane within it;
// first col0 (LIST: entry) of the wave / of the workgroup, the row's count of them; no col0 in
// this wave (wave-uniform); the row's left / right descriptors
struct PkWave {
    int row, h, j, c0_wave, wg_c0, lcols;
    bool idle;
    const uint32_t* __restrict__ row0;
    const uint32_t* __restrict__ row1;
};
// bytes of the chunk region ahead of the staged raw right row: the workgroup's int16 results
__device__ __forceinline__ int pk_row_off(int waves, int T) { return (waves * T * 64 * 2 + 15) & ~15; }

// col0 c's final block (base Bb, minimum distance hm) rescanned by popcounts -- the first col1
// at hm, and whether it occurs twice there; src = the right row's words, staged or in HBM.
// (row0 without __restrict__: with it the two calls' loads of the left descriptor differ in
// their alias scopes, the compiler no longer hoists them above the staged / unstaged branch,
// and every rescan starts by waiting for its own load: random 32-bit NoDuplicates +1 %)
template <int WORDS>
__device__ __forceinline__ void pk_rescan(const uint32_t* src, const uint32_t* row0, int cols,
                                          int c, int Bb, uint32_t hm, int& best, bool& uniq) {
    uint32_t aw[WORDS];
#pragma unroll
    for (int w = 0; w < WORDS; ++w) aw[w] = row0[(size_t)c * WORDS + w];
    uint32_t eq = 0;
#pragma unroll 4
    for (int r = 0; r < 32; ++r) {
        const int c1 = Bb + r;
        const int cc = min(c1, cols - 1);  // (past the row: never counted, read in bounds)
        uint32_t hsum = 0;
#pragma unroll
        for (int w = 0; w < WORDS; ++w) hsum = __popc(aw[w] ^ src[(size_t)cc * WORDS + w]) + hsum;
        eq |= (c1 < cols && hsum == hm) ? (1u << r) : 0u;
    }
    best = Bb + (int)__builtin_ctz(eq | 0x80000000u);
    uniq = __popc(eq) == 1;
}
// the right row's nw raw words into LDS: one coalesced copy per workgroup, L2-resident
// (WORDS == 4: nw is a multiple of 4 and the tail loop is empty)
__device__ __forceinline__ void pk_copy_row(uint32_t* row_lds, const uint32_t* __restrict__ row1, int nw) {
    if ((reinterpret_cast<uintptr_t>(row1) & 15u) == 0) {
        for (int i = threadIdx.x; i < nw / 4; i += blockDim.x)
            reinterpret_cast<v4i*>(row_lds)[i] = reinterpret_cast<const v4i*>(row1)[i];
        for (int i = nw / 4 * 4 + threadIdx.x; i < nw; i += blockDim.x) row_lds[i] = row1[i];
    } else {
        for (int i = threadIdx.x; i < nw; i += blockDim.x) row_lds[i] = row1[i];
    }
}
// one col0's result, column c0 of the 32-col0 tile at c0_tile: col1 `best` where ok. The dense-row
// fast path's valid count of the tile (every lane of the half joins), then the disparity or
// the column to the output row, or (AG) to the workgroup's results in LDS
template <bool LIST, bool AG>
__device__ __forceinline__ void pk_result(const SearchArgs& a, int row, int c0_tile, int c0, bool live,
                                          bool ok, int best, bool writer, int16_t* raw_lds, int wg_c0) {
    if constexpr (!LIST && !AG) {
        if (a.row_valid) tile_valid_store(a, row, c0_tile, live && ok, best, writer);
    }
    if (!live) return;
    int16_t v;
    if (a.out_mode == 0)
        v = ok ? (int16_t)(c0 - best) : INVALID_I16;
    else
        v = ok ? (int16_t)best : (int16_t)-1;
    if constexpr (AG)
        raw_lds[c0 - wg_c0] = v;
    else
        (a.out + (size_t)row * a.out_pitch)[c0] = v;
}
// AG: the fused agree over the workgroup's wg_cols col0 from wg_c0, whose integer results
// raw_lds holds (n = 8 with 32-bit descriptors, cfg1; n = 33 with 128-bit, cfg2 / cfg5)
template <int WORDS, bool AG, class KA>
__device__ __forceinline__ void pk_agree(const KA& ka, int row, int wg_c0, int wg_cols, const int16_t* raw_lds) {
    if constexpr (AG) {
        __syncthreads();
        fused_agree<WORDS == 1 ? FUSED_AGREE_N_PK : FUSED_AGREE_N>(
            ka.ag, row, wg_c0, min(wg_cols, search_part(ka).cols - wg_c0), raw_lds);
    }
}
// The end of a row behind the block loops, from the pairs' R, M and C (NP of each). AG: the
// workgroup's integer results go through LDS to the fused agree (as in search_mx_kernel); the
// chunk region is reused once every wave is done with its blocks. LAZY: each col0 without a
// tie since its last drop counts its final block's minima (pk_rescan), from the right row's
// raw words copied past those results (staged: they fit the chunk region), else from HBM.
template <int WORDS, int T, bool LIST, bool AG, bool LAZY, class KA, class LCOL>
__device__ __forceinline__ void pk_end_of_row(const KA& ka, const PkWave& w, v4i* lds_mx, bool staged,
                                              const uint32_t* R, const uint32_t* M, const uint32_t* C,
                                              LCOL lcol) {
    constexpr int NP = T == 1 ? 1 : T / 2;
    const SearchArgs& a = search_part(ka);
    const int cols = a.cols;
    const int waves = blockDim.x >> 6;
    int16_t* raw_lds = reinterpret_cast<int16_t*>(lds_mx);
    uint32_t* row_lds = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds_mx) + pk_row_off(waves, T));
    if (!AG && !staged && w.idle) return;
    if (AG || staged) __syncthreads();
    if (staged) {
        pk_copy_row(row_lds, w.row1, cols * WORDS);
        __syncthreads();
        if (!AG && w.idle) return;
    }
    int jo = w.j;
    asm volatile("" : "+v"(jo));
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if (T == 1 && w.h) continue;  // one tile: lanes 0-31 hold it
        const int t = T == 1 ? 0 : 2 * p + w.h;
#pragma unroll
        for (int f = 0; f < 2; ++f) {  // f = 0: high field (col0 P), 1: low field (Q = P + 32)
            const int c0i = w.c0_wave + 64 * t + 32 * f + jo;
            const int sh = f ? 0 : 16;
            const bool live = !w.idle && c0i < w.lcols;
            int best = (int)((C[p] >> sh) & 0xFFFFu);
            bool ok = ((M[p] >> sh) & 0xFFFFu) != 0u;
            if constexpr (LAZY) {
                if (live && ok) {
                    const uint32_t hm = ((R[p] >> sh) & 0xFFFFu) - 0x4B00u;
                    if (staged)
                        pk_rescan<WORDS>(row_lds, w.row0, cols, lcol(c0i), best, hm, best, ok);
                    else
                        pk_rescan<WORDS>(w.row1, w.row0, cols, lcol(c0i), best, hm, best, ok);
                }
            }
            pk_result<LIST, AG>(a, w.row, w.c0_wave + 64 * t + 32 * f, live ? lcol(c0i) : 0, live, ok, best,
                                jo == 0, raw_lds, w.wg_c0);
        }
    }
    pk_agree<WORDS, AG>(ka, w.row, w.wg_c0, waves * T * 64, raw_lds);
}

// T wide tiles (64 col0 each) per wave; T = 1 or an even count (tiles reduced in pairs);
// TAIL: the col0 range starts at a.tail_col0 (the tail launch, as search_mx_kernel's);
// LIST: compacted col0 entries (as search_mx_kernel's); LAZY: lazy drops (lazy_drop)
template <int WORDS, int T, bool TAIL, bool LIST, bool AG, bool LAZY>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4)))
void search_pk_kernel(typename SearchKArgs<AG>::type ka) {
    const SearchArgs& a = search_part(ka);
    static_assert(T == 1 || T % 2 == 0, "wide tiles: 1 or pairs");
    static_assert(!AG || (!TAIL && !LIST), "the fused agree: main launch, every col0");
    static_assert(!AG || WORDS == 1 || WORDS == 4, "the fused agree: cfg1's and cfg2's widths");
    constexpr int NP = T == 1 ? 1 : T / 2;
    extern __shared__ __attribute__((aligned(16))) v4i lds_mx[];  // [WORDS][chunk]

    int row, tile;
    if constexpr (LIST) {
        list_row_tile(a.tiles_per_row, a.rows, row, tile);
        if (row >= a.rows) return;
    } else {
        xcd_row_tile(a.tiles_per_row, row, tile);
    }

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int h = lane >> 5;
    const int j = lane & 31;
    const int cols = a.cols;
    const int chunk = a.chunk;
    const int waves = blockDim.x >> 6;
    const int c0_base = TAIL ? a.tail_col0 : 0;
    const int c0_wave = c0_base + (tile * waves + wave) * (T * 64);
    int lcols = cols;
    const int e0 = c0_base + tile * waves * T * 64;
    int16_t* ent = nullptr;
    bool dense = false;  // (as search_mx_kernel's)
    if constexpr (LIST) {
        ent = (int16_t*)((char*)lds_mx + list_ent_offset(WORDS * chunk * 16));
        dense = a.row_valid != nullptr && dense_row(a, row);
        if (!dense)
            lcols = list_prologue(a.keep + (size_t)row * a.keep_pitch, cols, (uint32_t*)lds_mx, ent,
                                  e0, waves * T * 64);
        if (!TAIL) lcols = min(lcols, a.tail_col0);  // the tail launch takes the entries past it
        if (e0 >= lcols) return;  // the whole workgroup, past the prologue's barriers
    }
    auto lcol = [&](int i) { return LIST && !dense ? (int)ent[i - e0] : i; };
    auto start_col = [&](int e, int ahead) {
        return LIST ? min(cols - 1, lcol(min(e, lcols) - 1) + ahead) : min(cols - 1, e - 1);
    };

    const uint32_t* __restrict__ row0 = a.desc0 + (size_t)row * a.desc_pitch;
    const uint32_t* __restrict__ row1 = a.desc1 + (size_t)row * a.desc_pitch;

    v4i bf[T][WORDS];
    pk_bfrags<WORDS, T>(bf, row0, c0_wave, lane, lcols, lcol);
    const int sb = h ? 127 : PK_SCALE_HI;
    v16f cb = pk_cb<WORDS>();

    // per pair p (lanes 0-31: tile 2p, lanes 32-63: tile 2p+1; T = 1: all lanes tile 0):
    // running minimum, tie marker, first column of the minimum
    uint32_t R[NP], M[NP], C[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        R[p] = PK_PAD;
        M[p] = 0xFFFFFFFFu;
        C[p] = 0u;
    }

    // one pair's block minima x (tile 2p) / y (tile 2p+1) at block base B (see lazy_drop)
    auto pair_step = [&](int p, int B, const v16f& dx, const v16f& dy) {
        const uint32_t x = pk_tree(dx);
        const uint32_t y = T == 1 ? x : pk_tree(dy);
        const auto sw = __builtin_amdgcn_permlane32_swap(x, y, false, false);
        const uint32_t comb = pkminu(sw[0], sw[1]);
        const uint32_t diff = pksub(comb, R[p]);
        if constexpr (LAZY) {
            lazy_drop(M[p], R[p], C[p], comb, diff, B);
            return;
        }
        M[p] = pkminu(M[p], diff);
        const bool imp = (diff & 0x80008000u) != 0u;
        if (__builtin_amdgcn_ballot_w64(imp)) {
            // a new running minimum somewhere in the pair: per (tile, distance field) that
            // holds one, the first row at it and whether the block holds it twice ((distance,
            // row) keys through v_perm + v_pk_min_u16, first and reversed rows)
            const uint32_t mi = pksign(diff);
            const uint32_t hoff = h ? 0xFFFC0004u : 0u;  // rows + 4h (low), 31 - rows - 4h (high)
            auto field = [&](auto sel_tag, uint32_t top, int sh) {
                constexpr uint32_t SEL = decltype(sel_tag)::value;
                const uint64_t bal = __builtin_amdgcn_ballot_w64((diff & top) != 0u);
                uint32_t lo = (uint32_t)bal, hi = (uint32_t)(bal >> 32);
                asm volatile("" : "+s"(lo), "+s"(hi));
                if (T == 1) hi = 0;  // (one tile: both halves hold it)
                if (!(lo | hi)) return;
                uint32_t kx = 0, ky = 0;
                if (lo) kx = pk_row_keys<SEL>(dx) + hoff;
                if constexpr (T != 1) {
                    if (hi) ky = pk_row_keys<SEL>(dy) + hoff;
                }
                if (!lo) kx = ky;
                if (!hi) ky = kx;
                const auto sk = __builtin_amdgcn_permlane32_swap(kx, ky, false, false);
                const uint32_t res = pkminu(sk[0], sk[1]);
                const uint32_t first = res & 0x1Fu;
                const uint32_t uniq = first + ((res >> 16) & 0x1Fu) == 31u ? 0xFFFFu : 0u;
                const uint32_t fm = mi & (0xFFFFu << sh);
                R[p] = bfi(fm, comb, R[p]);
                C[p] = bfi(fm, ((uint32_t)B + first) << sh, C[p]);
                M[p] = bfi(fm, uniq << sh, M[p]);
            };
            field(std::integral_constant<uint32_t, PK_SEL_P>{}, 0x80000000u, 16);
            field(std::integral_constant<uint32_t, PK_SEL_Q>{}, 0x00008000u, 0);
        }
    };

    const bool idle = c0_wave >= lcols;  // wave-uniform; still joins the barriers
    const int nchunks = (cols + chunk - 1) / chunk;
    // chunks downwards from the one holding the workgroup's highest col0, blocks downwards
    // from the wave's highest col0 (stereo matches lie at col1 <= col0 within a few blocks,
    // so the running minimum is found early and later blocks rarely take the branch)
    const int cstart = start_col(c0_base + (tile + 1) * waves * T * 64, 0) / chunk;
    for (int k = 0; k < nchunks; ++k) {
        int ci = cstart - k;
        if (ci < 0) ci += nchunks;
        const int base = ci * chunk;
        const int ncols = min(chunk, cols - base);
        if (k) __syncthreads();
        for (int c = threadIdx.x; c < chunk; c += blockDim.x) {
            const int c1 = base + c;
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                const uint32_t x = c1 < cols ? row1[(size_t)c1 * WORDS + w] : 0u;
                lds_mx[w * chunk + c] = expand_bits(x, LUT_PA);
            }
        }
        __syncthreads();
        if (idle) continue;

        const int nfull = ncols / 32;
        auto block = [&](int b, bool pad) {
            const int B = base + 32 * b;
            // (C kept in VGPRs: left alone the compiler re-copies it from SGPRs every block)
            asm volatile("" : "+v"(cb));
            v4i af[WORDS];
#pragma unroll
            for (int w = 0; w < WORDS; ++w) af[w] = lds_mx[w * chunk + 32 * b + j];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int tx = T == 1 ? 0 : 2 * p, ty = T == 1 ? 0 : 2 * p + 1;
                v16f dx, dy;
                pk_product<WORDS, T != 1>(af, bf[tx], bf[ty], cb, sb, dx, dy);
                if (pad) pk_pad(dx, dy, b, ncols, h);
                pair_step(p, B, dx, dy);
            }
        };
        if ((ncols & 31) != 0) block(nfull, true);
        const int sb0 = max(0, min(nfull - 1, (start_col(c0_wave + 64 * T, REV_AHEAD) - base) / 32));
        for (int i = 0; i < nfull; ++i) {
            int b = sb0 - i;
            if (b < 0) b += nfull;
            block(b, false);
        }
    }
    const bool staged =
        LAZY && (size_t)WORDS * chunk * 16 >= (size_t)pk_row_off(waves, T) + (size_t)cols * WORDS * 4;
    if constexpr (AG && WORDS == 4 && T == 1) {
        // pk_end_of_row written out for the fused one-tile 128-bit instantiations (BICOS_PK128,
        // narrow bands): through the function the same statements leave fused_agree scheduled
        // with more loads in flight, next_free_vgpr 96 -> 104 (branch) and 83 -> 102 (lazy),
        // 5 -> 4 waves per SIMD by the compiler's count
        int16_t* raw_lds = reinterpret_cast<int16_t*>(lds_mx);
        uint32_t* row_lds = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds_mx) + pk_row_off(waves, T));
        __syncthreads();
        if (staged) {
            pk_copy_row(row_lds, row1, cols * WORDS);
            __syncthreads();
        }
        int jo = j;
        asm volatile("" : "+v"(jo));
#pragma unroll
        for (int f = 0; f < 2; ++f) {  // lanes 0-31 hold the tile; f as in pk_end_of_row
            if (h) continue;
            const int c0 = c0_wave + 32 * f + jo;
            const int sh = f ? 0 : 16;
            const bool live = !idle && c0 < lcols;
            int best = (int)((C[0] >> sh) & 0xFFFFu);
            bool ok = ((M[0] >> sh) & 0xFFFFu) != 0u;
            if constexpr (LAZY) {
                if (live && ok) {
                    const uint32_t hm = ((R[0] >> sh) & 0xFFFFu) - 0x4B00u;
                    if (staged)
                        pk_rescan<WORDS>(row_lds, row0, cols, c0, best, hm, best, ok);
                    else
                        pk_rescan<WORDS>(row1, row0, cols, c0, best, hm, best, ok);
                }
            }
            pk_result<LIST, AG>(a, row, c0_wave + 32 * f, c0, live, ok, best, jo == 0, raw_lds, e0);
        }
        pk_agree<WORDS, AG>(ka, row, e0, waves * T * 64, raw_lds);
    } else {
        const PkWave pw{row, h, j, c0_wave, e0, lcols, idle, row0, row1};
        pk_end_of_row<WORDS, T, LIST, AG, LAZY>(ka, pw, lds_mx, staged, R, M, C, lcol);
    }
}

// The pruned search's four products: e holds the expansions of a descriptor's four words on entry
// and the operands of its four products on return. Dword m of an expansion holds the bits p of
// its word with (p mod 8) div 2 == m (expand_bits), and products 0 and 1 take words 0 and 1 by
// alternate dwords (search_plan.hpp pkp_dword_word): product 0 is {E(w0)[0], E(w1)[1], E(w0)[2],
// E(w1)[3]}, product 1 {E(w1)[0], E(w0)[1], E(w1)[2], E(w0)[3]}, products 2 and 3 words 2 and 3.
// Every dword of an expansion is a shift, mask and v_perm of its own, so this chooses which
// word feeds which dword and adds no instruction. The search is exact for any fixed assignment of
// descriptor bits to K positions that both operands share (expand_bits); this one is chosen for
// the one-word probe (block_pr). The bits of a LIMITED word are those of about 8 consecutive
// image steps and share samples (a < b, a < c, a < mean, the pair sums of steps t and t + 1),
// so the distance of unrelated pixels over one WORD has a fat lower tail and blocks reach that 32
// less correlated bits rule out: on the cfg2 frame 18.0 % of wide-tile-blocks with word 0, 11.9 %
// with this product 0, 11.4 % with the two-word probe (tools/prune_sim.py --mix).
// Products 0 and 1 together are still exactly words 0 and 1. (The price: rows of slightly noisy
// descriptors, 2 % of the bits flipped, reach with this product in 68 % of the blocks where word 0
// reached in 99 %; the window rule keeps such waves at depth 1, and they are slower than they
// were -- DESIGN.md s5.1, round 17.)
__device__ __forceinline__ void pkp_mix(v4i (&e)[4]) {
    v4i o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int m = 0; m < 4; ++m) o[k][m] = e[pkp_dword_word(k, m)][m];
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = o[k];
}

// The pruned 128-bit search: WORDS = 4, one pair of wide tiles per wave, lazy drops, every
// col0 of the row (no tail, no list), main launches only; the 128 descriptor bits go to four
// products of 32 bits each (pkp_mix), a block is probed with product 0, or with products 0
// and 1, and the other products are multiplied only where they can matter (block_pr). ST: the
// right row streamed (raw_col); EOR: a shorter end of row (pair_update, and the end of the
// kernel). Prologue but for pkp_mix, lazy step and, without EOR, the end of row are
// search_pk_kernel<4, 2, false, false, AG, true>'s.
template <bool AG, bool ST, bool EOR>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4)))
void search_pkp_kernel(typename SearchKArgs<AG>::type ka) {
    const SearchArgs& a = search_part(ka);
    constexpr int WORDS = 4, T = 2;
    extern __shared__ __attribute__((aligned(16))) v4i lds_mx[];  // [WORDS][chunk]

    int row, tile;
    xcd_row_tile(a.tiles_per_row, row, tile);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int h = lane >> 5;
    const int j = lane & 31;
    const int cols = a.cols;
    // ST: the chunk is PKP_ST_CHUNK (search_plan.hpp: the default geometry's, 8 waves over a 64
    // KiB stage), a constant of those instantiations so that a block's products 1-3 are read at
    // immediate offsets (16, 32, 48 KiB: the ds_read offset field has 16 bits) from the address
    // of its product-0 fragment. plan_mx (search_plan.cpp) streams the packed search at that
    // geometry only; launch_pk_variant refuses a streamed launch with any other.
    const int chunk = ST ? PKP_ST_CHUNK : a.chunk;
    const int waves = blockDim.x >> 6;
    const int c0_wave = (tile * waves + wave) * (T * 64);

    const uint32_t* __restrict__ row0 = a.desc0 + (size_t)row * a.desc_pitch;
    const uint32_t* __restrict__ row1 = a.desc1 + (size_t)row * a.desc_pitch;

    // The block loops name a block by the LDS address of the lane's product-0 fragment of it and
    // step that address by a scalar delta (-512 bytes, or back up to the step's last full block
    // at the wrap); products 1-3 lie 16 chunk bytes apart. frag: the fragment of product w of the
    // block whose product-0 fragment this lane reads at LDS address ad (ST: at an immediate
    // offset). LDS addresses as integers, lds0 the chunk region's: with the region's pointer in
    // the sum the compiler adds its address, 0, to ad at every read.
    typedef const __attribute__((address_space(3))) v4i* lds_frag_ptr;
    const uint32_t lds0 = (uint32_t) reinterpret_cast<uintptr_t>((lds_frag_ptr)lds_mx);
    auto frag = [&](uint32_t ad, int w) {
        return *reinterpret_cast<lds_frag_ptr>(ad + (uint32_t)(w * chunk * 16));
    };

    // ST (the plan guarantees chunk = 2 * blockDim.x = PKP_ST_CHUNK and cols > chunk -- a tuned
    // geometry with another chunk takes the chunk loop): the right row streamed exactly as
    // search_mx_kernel ST does -- the workgroup's own chunk expanded whole, the rest of the row
    // in stages of half a chunk alternating between the two halves of the chunk region, the
    // next stage's raw descriptor held in four VGPRs across the block loop, one barrier per
    // stage. Same LDS layout; only the expansion table differs.
    // raw_col: the raw right descriptor of col1 (zero past the image); the own chunk's two
    // columns of this thread are requested ahead of the B-fragment loads below
    auto raw_col = [&](int c1) {
        v4i x = {0, 0, 0, 0};
        if (c1 < cols) {
#pragma unroll
            for (int w = 0; w < WORDS; ++w) x[w] = (int)row1[(size_t)c1 * WORDS + w];
        }
        return x;
    };
    auto put_col = [&](int c, const v4i& x) {  // LDS column c of the chunk region, by products
        v4i e[WORDS];
#pragma unroll
        for (int w = 0; w < WORDS; ++w) e[w] = expand_bits((uint32_t)x[w], LUT_PA);
        pkp_mix(e);
#pragma unroll
        for (int w = 0; w < WORDS; ++w) lds_mx[w * chunk + c] = e[w];
    };
    const int half = chunk >> 1;
    const int nchunks = (cols + chunk - 1) / chunk;
    // chunks downwards from the one holding the workgroup's highest col0 (as search_pk_kernel)
    const int cstart = min(cols - 1, (tile + 1) * waves * T * 64 - 1) / chunk;
    v4i raw = {0, 0, 0, 0}, raw_hi = {0, 0, 0, 0};
    if constexpr (ST) {
        raw = raw_col(cstart * chunk + (int)threadIdx.x);
        raw_hi = raw_col(cstart * chunk + half + (int)threadIdx.x);
    }

    v4i bf[T][WORDS];
    pk_bfrags<WORDS, T>(bf, row0, c0_wave, lane, cols, [](int i) { return i; });
#pragma unroll
    for (int t = 0; t < T; ++t) pkp_mix(bf[t]);  // by products, as put_col's
    const int sb = h ? 127 : PK_SCALE_HI;
    v16f cb = pk_cb<WORDS>();
    // (C kept in VGPRs: left alone the compiler re-copies it from SGPRs every block. Made opaque
    // once, here: done in every block, each of the three block loops carries a copy of its own)
    asm volatile("" : "+v"(cb));

    // lanes 0-31: tile 0, lanes 32-63: tile 1 -- running minimum, tie marker, block base of
    // the last drop; the reach test's threshold R + thr_off per field (49 at probe depth 1, 33
    // at depth 2); the fallback's state (wave-uniform): the probe depth in products,
    // from the launch (a.split: 1 or 2), 1 -> 2 -> 0 (the unpruned loop), never back up
    uint32_t R = PK_PAD, M = 0xFFFFFFFFu, C = 0u;
    int depth = a.split == 1 ? 1 : 2;
    uint32_t thr_off = depth == 1 ? PKP_THR1 : PKP_THR;
    uint32_t thr = PK_PAD + thr_off;
    int wblocks = 0, wreach = 0;

    // the lazy pair step from the two trees' results x (tile 0) / y (tile 1) in this lane half
    // at block base B (a pruned tile passes its partial one); renews thr.
    // EOR: a lazy drop also records WHICH LANE HALF of the block holds the new minimum. sw[0] /
    // sw[1] are the block minima of the lane's tile over the rows of lane half 0 / 1 (pk_rrow).
    // On a strict drop of a field:
    //   sw[0] != sw[1]: every column of the block at the new minimum lies in the half with the
    //     smaller value; bit 15 of the field of C (block bases stay below 2^15) takes the sign of
    //     sw[1] - sw[0], and M takes sw[0] ^ sw[1], some value != 0: "no tie seen since".
    //   sw[0] == sw[1]: the block holds the new minimum in two rows of different halves, that is
    //     in two different columns -- exactly what a tie in a later block would have meant. M
    //     takes sw[0] ^ sw[1] = 0, the tie marker, and no rescan is needed for this col0.
    // (Why that is exact: at the EOR end of row below.)
    auto pair_update = [&](int B, uint32_t x, uint32_t y) {
        const auto sw = __builtin_amdgcn_permlane32_swap(x, y, false, false);
        const uint32_t comb = pkminu(sw[0], sw[1]);
        const uint32_t diff = pksub(comb, R);
        if constexpr (EOR) {
            const uint32_t mi = pksign(diff);
            // a drop: the tie marker restarts from the two halves' minima (0: the block holds
            // the new minimum in both), and bit 15 of C's field says which half holds it
            // (v_bfi_b32 by hand, as in lazy_drop: left alone the compiler selects per field)
            uint32_t m = pkminu(M, diff);
            asm("v_bfi_b32 %0, %1, %2, %0" : "+v"(m) : "v"(mi), "v"(sw[0] ^ sw[1]));
            M = m;
            R = bfi(mi, comb, R);
            uint32_t bh = pksub(sw[1], sw[0]);
            asm("v_bfi_b32 %0, %1, %2, %0" : "+v"(bh) : "v"(0x7FFF7FFFu), "s"((uint32_t)B * 0x10001u));
            asm("v_bfi_b32 %0, %1, %2, %0" : "+v"(C) : "v"(mi), "v"(bh));
        } else {
            lazy_drop(M, R, C, comb, diff, B);
        }
        thr = R + thr_off;
    };

    const bool idle = c0_wave >= cols;  // wave-uniform; still joins the barriers
    // ST: streamed stage s (after the own chunk) starts at col1 stage_base(s) and lives in
    // half s & 1 of the chunk region; 2 (nchunks - 1) of them, the last chunk's possibly
    // short or empty (they still take their barrier: workgroup-uniform)
    auto stage_base = [&](int s) {
        int ci = cstart - 1 - (s >> 1);
        if (ci < 0) ci += nchunks;
        return ci * chunk + ((s & 1) ? 0 : half);
    };
    const int nstages = ST ? 2 * (nchunks - 1) : 0;
    const int nsteps = ST ? 1 + nstages : nchunks;
    if constexpr (ST) {
        put_col((int)threadIdx.x, raw);
        put_col(half + (int)threadIdx.x, raw_hi);
    }
    for (int k = 0; k < nsteps; ++k) {
        // this step's columns: col1 base + c for LDS column c, from LDS block b0, ncols of them
        int base, ncols, b0 = 0;
        if constexpr (ST) {
            if (k == 0) {
                base = cstart * chunk;
                ncols = min(chunk, cols - base);
            } else {
                const int sbase = stage_base(k - 1);
                b0 = ((k - 1) & 1) ? half >> 5 : 0;
                base = sbase - 32 * b0;
                ncols = max(0, min(half, cols - sbase));
            }
            if (k == 1) __syncthreads();  // every wave is done with the own chunk
            if (k >= 1) put_col(32 * b0 + (int)threadIdx.x, raw);
            if (k < nstages) raw = raw_col(stage_base(k) + (int)threadIdx.x);  // the next stage's
            __syncthreads();
        } else {
            int ci = cstart - k;
            if (ci < 0) ci += nchunks;
            base = ci * chunk;
            ncols = min(chunk, cols - base);
            if (k) __syncthreads();
            for (int c = threadIdx.x; c < chunk; c += blockDim.x) put_col(c, raw_col(base + c));
            __syncthreads();
        }
        if (idle) continue;

        const int nfull = ncols / 32;
        // (block indices: LDS blocks of the chunk region, the step's first one b0; the loops
        // name block b by ad, the LDS address of this lane's product-0 fragment of it: lds0 +
        // 16 (32 b + j))
        // a block in full, at col1 B, the step's block bi: the partial last block (pad) and the
        // fallback's loop
        auto block = [&](uint32_t ad, int B, int bi, bool pad) {
            v4i af[WORDS];
#pragma unroll
            for (int w = 0; w < WORDS; ++w) af[w] = frag(ad, w);
            v16f dx, dy;
            pk_product<WORDS, true>(af, bf[0], bf[1], cb, sb, dx, dy);
            if (pad) pk_pad(dx, dy, bi, ncols, h);
            pair_update(B, pk_tree(dx), pk_tree(dy));
        };
        // A full block, at col1 B, with products 2 and 3 only for the wide tiles that can reach.
        // The four products partition the 128 bit positions into groups of 32 (pkp_mix); ham'_k
        // is the distance over product k's bits, each in [0, 32], ham = ham'_0 + ham'_1 + ham'_2
        // + ham'_3, and ham_lo = ham'_0 + ham'_1 is the distance over words 0 and 1, whichever 32
        // of their bits product 0 holds. Nothing below depends on which bits a product holds.
        // After the MFMAs of products 0 and 1 both fields of every accumulator hold 0x4B00 + 32 +
        // ham_lo (C carries + 64, each product adds ham'_k - 16), and the final field is 0x4B00 +
        // ham with ham >= ham_lo. The packed tree of these partial keys, combined over the lane
        // halves as in the pair step, is tested per field against thr = R + 0x00210021 as
        // UNSIGNED 16-BIT INTEGERS (not f16: PK_PAD + 0x21 is a NaN pattern) by one saturating
        // subtraction, thr - key != 0 (v_pk_sub_u16 clamp; neither field of thr wraps: R <=
        // 0x7BFF): reach is ham_lo <= running minimum, "<=" because a tie must never be pruned
        // (NoDuplicates needs it). The decision is per wide tile (the ballot's halves): a tile
        // none of whose 64 col0 reaches skips its MFMAs of products 2 and 3 and its tree; it
        // enters the pair step, if the other tile takes one, with its partial keys. That is
        // safe under lazy drops: a pruned tile-block has block minimum > R for every col0, and
        // R only falls, so the block is neither a drop nor a tie now or later; its partial keys
        // lie above R too, so all they can give M is a positive value, which never decides
        // anything -- `ok` tests M == 0 only, and a later drop resets M. thr is renewed only
        // where R may have changed. The partial last block never prunes. Fallback as
        // search_mx_kernel's: over windows of PRUNE_WINDOW visited blocks a wave counts its
        // reaching wide-tile-blocks (wreach) from the branch's own ballots; >= 7/8 of them (14
        // of 16) send it to the unpruned loop for the rest of the row. (Lazy drops stay under
        // pruning: with the drop branch in the reaching blocks instead of the rescans the fused
        // cfg2 launch took 313.8 instead of 276.2 us.)
        // Probe depth 1 (D = 1): one scaled MFMA multiplies the 32 bits of exactly one product,
        // so the block can be tested after product 0 alone. After that MFMA both fields of every
        // accumulator hold 0x4B00 + 48 + ham'_0 (C carries + 64, product 0 adds ham'_0 - 16),
        // and the final field is 0x4B00 + ham with ham >= ham_lo >= ham'_0. The packed tree of
        // these keys, combined over the lane halves, is tested per field against thr = R +
        // 0x00310031 as unsigned 16-bit integers by the same saturating subtraction, thr - key !=
        // 0 (neither field of thr wraps: R <= 0x7BFF, and 0x7BFF + 0x31 < 2^16): reach is ham'_0
        // <= running minimum, "<=" because a tie must never be pruned. A tile none of whose 64
        // col0 reaches skips its MFMAs of products 1, 2 and 3 and its second tree, and enters the
        // pair step, if the other tile takes one, with its product-0 keys. That is safe under
        // lazy drops for the same reason: a tile-block pruned at depth 1 has ham >= ham'_0 > R
        // for every col0 and every column of the block, and R only falls, so the block is
        // neither a drop nor a tie now or later; its product-0 keys, 0x4B00 + 48 + ham'_0, lie
        // above R in every field too, so all they can give M is a positive value, which never
        // decides anything. A tile that reaches takes products 1-3 at once and the full tree.
        // Which 32 bits product 0 holds decides only how often a block reaches: with 16 bits of
        // each of words 0 and 1 (pkp_mix) a one-product probe prunes nearly like the two-word
        // one. The window rule is the same at both depths: at depth 1 a wave 14 of whose 16
        // wide-tile-blocks reach goes on at depth 2 (thr = R + 33) for the rest of the row, and
        // from depth 2 to the unpruned loop; it never goes back up. Depth 2 tests words 0 and
        // 1 whole, so its decisions, BICOS_PKP_PROBE=2 and the windows at depth 2 are bit for bit
        // what they were before the products were mixed. Noisy rows so pay one window more than
        // they did.
        // af0 holds the block's product-0 fragment on entry and the next block's on return, read
        // once the probe products are issued; the other words' fragments are read here, at the
        // top of the block, and ad then steps by d bytes to the next block.
        auto block_pr = [&](auto depth_tag, int B, uint32_t& ad, v4i& af0, int d) {
            constexpr int D = decltype(depth_tag)::value;  // the probe's products
            // (the products behind the probe read here too: 2 and 3 read only in the blocks
            // that reach, the fused cfg2 launch took 275.9 instead of 273.5 us at depth 2)
            v4i af[WORDS];
            af[0] = af0;
#pragma unroll
            for (int w = 1; w < WORDS; ++w) af[w] = frag(ad, w);
            // (one v_add_u32 with the scalar step: kept a value of its own, or the compiler
            // rebuilds the address of every word from the scalar block offset)
            ad += (uint32_t)d;
            asm volatile("" : "+v"(ad));
            v16f dx = mfma_pk(af[0], bf[0][0], cb, sb);
            v16f dy = mfma_pk(af[0], bf[1][0], cb, sb);
#pragma unroll
            for (int w = 1; w < D; ++w) {
                dx = mfma_pk(af[w], bf[0][w], dx, sb);
                dy = mfma_pk(af[w], bf[1][w], dy, sb);
            }
            // (both tiles' probe products go out before the first key is read)
            __builtin_amdgcn_sched_barrier(0);
            af0 = frag(ad, 0);
            uint32_t x = pk_tree(dx), y = pk_tree(dy);
            const auto sw = __builtin_amdgcn_permlane32_swap(x, y, false, false);
            // the probe's distance <= running minimum in either field, as u16 ("<=": a tie
            // reaches): thr is R + 49 / R + 33, so the saturated thr - lb is 0 exactly where lb
            // > R + 48 / R + 32
            const uint64_t bal = __builtin_amdgcn_ballot_w64(pksubsat(thr, pkminu(sw[0], sw[1])) != 0u);
            if (bal) {
                uint32_t lo = (uint32_t)bal, hi = (uint32_t)(bal >> 32);
                asm volatile("" : "+s"(lo), "+s"(hi));
                if (lo) {
#pragma unroll
                    for (int w = D; w < WORDS; ++w) dx = mfma_pk(af[w], bf[0][w], dx, sb);
                    x = pk_tree(dx);
                    ++wreach;
                }
                if (hi) {
#pragma unroll
                    for (int w = D; w < WORDS; ++w) dy = mfma_pk(af[w], bf[1][w], dy, sb);
                    y = pk_tree(dy);
                    ++wreach;
                }
                pair_update(B, x, y);
            }
        };
        const int Bs = base + 32 * b0;  // col1 of the step's first block
        if ((ncols & 31) != 0)
            block(lds0 + 16u * (uint32_t)(32 * (b0 + nfull) + j), Bs + 32 * nfull, nfull, true);
        // full blocks downwards from the one holding the wave's highest col0 (clamped)
        const int sb0 = max(0, min(nfull - 1, (min(cols - 1, c0_wave + 64 * T - 1) - base - 32 * b0) / 32));
        // The visiting order as one carried address: so = 512 x the step's block index (a
        // block's product-0 fragments are 512 bytes), stepped by -512, or from block 0 back up to
        // the last full block; ad follows it by the same scalar step. A read never leaves
        // the step's nfull blocks.
        int so = 512 * sb0;
        const int wrap = 512 * (nfull - 1);
        uint32_t ad = lds0 + 16u * (uint32_t)(32 * b0 + j) + (uint32_t)so;
        // The pruned loop over the first i0 blocks of the visiting order -- all of them unless
        // a window sends the wave to the unpruned loop below for the rest of the row. Shaped
        // as search_mx_kernel's: an inner run of blocks up to the window's end that only steps
        // the (wrapping) block offset, the next block's product-0 fragment read unconditionally
        // (behind the last block: the wrapped offset, a block nobody uses). The run is at the
        // wave's probe depth; a window that falls at depth 1 goes on here at depth 2
        int i0 = 0;
        if (depth && nfull > 0) {
            v4i af0 = frag(ad, 0);
            while (i0 < nfull) {
                int n = min(nfull - i0, PRUNE_WINDOW - wblocks);
                i0 += n;
                wblocks += n;
                if (depth == 1) {
                    for (; n > 0; --n) {
                        const int d = so > 0 ? -512 : wrap;
                        block_pr(std::integral_constant<int, 1>{}, Bs + (so >> 4), ad, af0, d);
                        so += d;
                    }
                } else {
                    for (; n > 0; --n) {
                        const int d = so > 0 ? -512 : wrap;
                        block_pr(std::integral_constant<int, 2>{}, Bs + (so >> 4), ad, af0, d);
                        so += d;
                    }
                }
                if (wblocks == PRUNE_WINDOW) {
                    const bool fall = 8 * wreach >= 7 * PRUNE_WINDOW * T;
                    wblocks = wreach = 0;
                    if (fall) {
                        if (depth == 2) {
                            depth = 0;
                            break;
                        }
                        depth = 2;
                        thr_off = PKP_THR;
                        thr = R + thr_off;
                    }
                }
            }
        }
        for (int i = i0; i < nfull; ++i) {
            const int d = so > 0 ? -512 : wrap;
            block(ad, Bs + (so >> 4), 0, false);
            ad += (uint32_t)d;
            so += d;
        }
    }
    // The workgroup's integer results (AG) and the right row's raw words for the rescans go
    // into the chunk region once every wave is done with its blocks (the plan guarantees that
    // the row fits: packed_search, search_plan.cpp)
    const int wg_c0 = tile * waves * T * 64;
    if constexpr (EOR) {
        // EOR: a shorter end of row, from the lane half that pair_update recorded with every
        // drop. Why that is exact: R ends as the row's minimum distance hm, and reaches it by a
        // strict drop in the first visited block whose minimum is hm; C holds that block and
        // half. If M ends 0, either a later block had minimum hm too (as without EOR) or both
        // halves of C's block did: a second column at hm either way, invalid. A later strict
        // drop overwrites M and C as a whole, so a duplicate of a minimum that was improved on
        // is forgotten, as before. If M ends != 0, every column at hm lies in the recorded half
        // of C's block, and the rescan of its 16 rows counts them and finds the first: the same
        // answer as the rescan of all 32. A pruned tile's partial keys lie above R in every
        // field, so they never take the drop's side of any of this.
        int16_t* raw_lds = reinterpret_cast<int16_t*>(lds_mx);
        uint32_t* row_lds = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(lds_mx) + pk_row_off(waves, T));
        // The raw row's first EARLY * blockDim columns (one dwordx4 each) and this lane's two
        // left descriptors are requested here, behind the wave's own last block; they arrive
        // while the barrier waits for the workgroup's slowest wave, and the row is written to
        // LDS behind it. (k * blockDim < cols is workgroup-uniform: a scalar branch around each
        // load, none waits for another.)
        constexpr int EARLY = 8;
        const bool al16 = (reinterpret_cast<uintptr_t>(row1) & 15u) == 0;
        const int bd = (int)blockDim.x;
        v4i early[EARLY];
        if (al16) {
#pragma unroll
            for (int k = 0; k < EARLY; ++k) {
                early[k] = v4i{0, 0, 0, 0};
                if (k * bd < cols)
                    early[k] = reinterpret_cast<const v4i*>(row1)[min(k * bd + (int)threadIdx.x, cols - 1)];
            }
        }
        v4i aw[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int c = min(c0_wave + 64 * h + 32 * f + j, cols - 1);
#pragma unroll
            for (int w = 0; w < WORDS; ++w) aw[f][w] = (int)row0[(size_t)c * WORDS + w];
        }
        __syncthreads();
        if (al16) {
#pragma unroll
            for (int k = 0; k < EARLY; ++k) {
                const int i = k * bd + (int)threadIdx.x;
                if (i < cols) reinterpret_cast<v4i*>(row_lds)[i] = early[k];
            }
            for (int i = EARLY * bd + (int)threadIdx.x; i < cols; i += bd)
                reinterpret_cast<v4i*>(row_lds)[i] = reinterpret_cast<const v4i*>(row1)[i];
        } else {
            for (int i = threadIdx.x; i < cols * WORDS; i += bd) row_lds[i] = row1[i];
        }
        __syncthreads();
        if (!AG && idle) return;

        // col0's final block rescanned in the recorded half only (16 rows from col1 B0 = block
        // base + 4 half, at (k & 3) + 8 (k >> 2)), in two levels: ham_lo (words 0 and 1) of the
        // 16 rows against hm, then the full distance of the candidates only (ham >= ham_lo, so
        // a column at hm is always a candidate), one per lane and trip of a loop that runs the
        // wave's largest candidate count. Masks are indexed by the row's offset from B0. CLAMP:
        // the block may reach past the row (the partial last block) -- those rows are read in
        // bounds and never counted.
        auto rescan = [&](auto clamp_tag, const v4i& x, int B0, uint32_t hm, int& best, bool& uniq) {
            constexpr bool CLAMP = decltype(clamp_tag)::value;
            uint32_t cand = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int r = (k & 3) + 8 * (k >> 2);
                const int cc = CLAMP ? min(B0 + r, cols - 1) : B0 + r;
                const v2u w = *reinterpret_cast<const v2u*>(row_lds + (size_t)cc * WORDS);
                const uint32_t lo = __popc((uint32_t)x[0] ^ w[0]) + __popc((uint32_t)x[1] ^ w[1]);
                cand |= lo <= hm ? (1u << r) : 0u;
            }
            if constexpr (CLAMP) {
                const int n = cols - B0;  // (>= 1: the recorded half holds a column of the row)
                cand &= n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u;
            }
            uint32_t eq = 0;
            while (__builtin_amdgcn_ballot_w64(cand != 0u)) {
                const bool act = cand != 0u;
                const int r = act ? (int)__builtin_ctz(cand | 0x80000000u) : 0;
                cand &= cand - 1u;
                const v4i w = *reinterpret_cast<const v4i*>(row_lds + (size_t)(B0 + r) * WORDS);
                uint32_t hsum = 0;
#pragma unroll
                for (int q = 0; q < WORDS; ++q) hsum = __popc((uint32_t)(x[q] ^ w[q])) + hsum;
                eq |= (act && hsum == hm) ? (1u << r) : 0u;
            }
            best = B0 + (int)__builtin_ctz(eq | 0x80000000u);
            uniq = __popc(eq) == 1;
        };

        int jo = j;
        asm volatile("" : "+v"(jo));
        // (wave-uniform: does any rescan of this wave touch the partial last block)
        bool need[2];
        bool part = false;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int sh = f ? 0 : 16;
            need[f] = !idle && c0_wave + 64 * h + 32 * f + jo < cols && ((M >> sh) & 0xFFFFu) != 0u;
            part = part || (need[f] && (int)((C >> sh) & 0x7FE0u) + 32 > cols);
        }
        const bool anypart = __builtin_amdgcn_ballot_w64(part) != 0;
#pragma unroll
        for (int f = 0; f < 2; ++f) {  // f = 0: high field (col0 P), 1: low field (Q = P + 32)
            const int c0 = c0_wave + 64 * h + 32 * f + jo;
            const int sh = f ? 0 : 16;
            const bool live = !idle && c0 < cols;
            const uint32_t cf = (C >> sh) & 0xFFFFu;
            int best = (int)(cf & 0x7FFFu);
            bool ok = need[f];
            if (ok) {
                const int B0 = best + (int)((cf >> 15) << 2);
                const uint32_t hm = ((R >> sh) & 0xFFFFu) - 0x4B00u;
                if (anypart)
                    rescan(std::true_type{}, aw[f], B0, hm, best, ok);
                else
                    rescan(std::false_type{}, aw[f], B0, hm, best, ok);
            }
            pk_result<false, AG>(a, row, c0_wave + 64 * h + 32 * f, c0, live, ok, best, jo == 0, raw_lds, wg_c0);
        }
        pk_agree<WORDS, AG>(ka, row, wg_c0, waves * T * 64, raw_lds);
    } else {
        const PkWave pw{row, h, j, c0_wave, wg_c0, cols, idle, row0, row1};
        pk_end_of_row<WORDS, T, false, AG, true>(ka, pw, lds_mx, true, &R, &M, &C, [](int i) { return i; });
    }
}

// search_pkp_kernel's shorter end of row (EOR; BICOS_PKP_EOR=0: the instantiations without it,
// the rescans of all 32 rows and the row copy behind the barrier; read once)
bool pkp_eor() {
    static const bool on = [] {
        const char* v = std::getenv("BICOS_PKP_EOR");
        return !(v && !std::strcmp(v, "0"));
    }();
    return on;
}
// search_pkp_kernel's probe depth at the start of a row, in products (block_pr): 1, or with
// BICOS_PKP_PROBE=2 the two-product probe, words 0 and 1, from the first block on (read once)
int pkp_probe() {
    static const int depth = [] {
        const char* v = std::getenv("BICOS_PKP_PROBE");
        return v && !std::strcmp(v, "2") ? 2 : 1;
    }();
    return depth;
}

}  // namespace

// The instantiations that are built: 1, 2 or (32/64-bit descriptors) 4 wide tiles per wave, whole
// rows or compacted, the drop branch or lazy drops; tails of one wide tile; the fused agree
// for cfg1's and cfg2's widths with 1 or (128-bit) 2 wide tiles. And search_pkp_kernel, with and
// without the fused agree, the streamed row and the shorter end of row.
hipError_t launch_pk_variant(const SearchLaunch& l, const SearchArgs& a, const AgreeArgs* ag,
                             hipStream_t st) {
    const SearchVariant& v = l.v;
    if (v.prune || v.stream) {  // search_pkp_kernel: the pruned 128-bit lazy search, streamed or not
        if (!v.prune || !v.lazy || v.words != 4 || v.T != 2 || v.tail || v.list) return hipErrorInvalidValue;
        // (the streamed instantiations are built for one chunk: two columns per thread)
        if (v.stream && (a.chunk != PKP_ST_CHUNK || l.block * 2 != PKP_ST_CHUNK)) return hipErrorInvalidValue;
        // (the start depth travels in `split`, which only the VALU search's launch reads: a field
        // of its own would move the agree's arguments in every fused kernel)
        SearchArgs ap = a;
        ap.split = pkp_probe();
        // clang-format off
        return pick<bool, false, true>(v.agree, [&](auto agree) {
        return pick<bool, false, true>(v.stream, [&](auto stream) {
        return pick<bool, false, true>(pkp_eor(), [&](auto eor) {
            return launch_planned<agree.value>(search_pkp_kernel<agree.value, stream.value, eor.value>, l, ap, ag, st);
        }); }); });
        // clang-format on
    }
    // clang-format off
    return pick<int, 1, 2, 4>(v.words, [&](auto words) {
    return pick<int, 1, 2, 4>(v.T, [&](auto T) {
    return pick<bool, false, true>(v.tail, [&](auto tail) {
    return pick<bool, false, true>(v.list, [&](auto list) {
    return pick<bool, false, true>(v.agree, [&](auto agree) {
    return pick<bool, false, true>(v.lazy, [&](auto lazy) {
        constexpr int W = words.value, TW = T.value;
        constexpr bool built = agree.value ? !tail.value && !list.value && (W == 1 ? TW == 1 : W == 4 && TW <= 2)
                               : tail.value ? TW == 1 : TW <= 2 || W <= 2;
        if constexpr (built)
            return launch_planned<agree.value>(
                search_pk_kernel<W, TW, tail.value, list.value, agree.value, lazy.value>, l, a, ag, st);
        else
            return hipErrorInvalidValue;
    }); }); }); }); }); });
    // clang-format on
}

}  // namespace bicos_hip
