// search_mx.hip -- the bicos Hamming search (reference include/impl/cpu/bicos.hpp:50-113) on
// the gfx950 matrix cores.
//
// Why a matrix core can do an exact Hamming search. With a = bits of the left (col0)
// descriptor and b = bits of the right (col1) descriptor,
//     ham(a, b) = sum_k a_k + b_k - 2 a_k b_k = |a| + sum_k b_k (1 - 2 a_k).
// |a| is constant over a row scan, so argmin_col1 ham = argmin_col1 x with
//     x(col0, col1) = sum_k B[k][col0] * A[col1][k],  A = b in {0, 1},  B = 1 - 2a in {+1, -1},
// a plain matrix product with K = descriptor bits. Both operands are exact FP4 (e2m1: 0, 1.0,
// -1.0), so one v_mfma_f32_32x32x64_f8f6f4 (FP4 x FP4 -> f32, 32 cycles per SIMD) evaluates
// 32 x 32 pairs x 64 bits; partial sums are small integers, exact in f32.
//
// The argmin key rides in the accumulator input: C[col1][col0] = 256 + col1 * 2^-15, so
//     D1 = A * B + C = 256 + x + col1 * 2^-15
// exactly (|x| <= 255, col1 < 32768: 24 significant bits at most; bit 255 of 256-bit
// descriptors is masked on both sides, as in the VALU search -- transform descriptors use
// at most 254 bits). D1 is positive, so its bit
// pattern orders like the float; min over col1 of bits(D1) picks the smallest x and, among
// equal x, the lowest col1 -- the reference's strict '<' scan (bicos.hpp:56-66). For
// NoDuplicates the same MFMA with the A operand negated gives D2 = 256 - x + col1 * 2^-15,
// whose maximum is the HIGHEST col1 at the minimum cost; the minimum is duplicated iff the
// two columns differ (bicos.hpp:58-73). Per pair the VALU does half a v_min3_u32 (and half a
// v_max3_u32): the xor / popcount work is gone from the vector pipe.
//
// Layout: a workgroup = one row x a range of WAVES*T*32 col0; each wave
// keeps T tiles of 32 left descriptors as B fragments in registers (lane l: col0 = 32t +
// (l & 31), descriptor word 2s + (l >> 5) of K-step s, one bit per FP4 nibble). The right
// row is expanded chunk by chunk into LDS as [word][col1] 16-byte FP4 fragments (one bit
// per nibble, 0 or 1.0), so the A fragment of (block, K-step) is ONE conflict-free
// ds_read_b128 per lane. Accumulator map (32x32 shapes): lane l, register r holds row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5) (= col1 in the block) and column l & 31 (= col0).
#include "search_dev.hpp"

#include <type_traits>

namespace bicos_hip {

namespace {

// One-product keys (XK): C = 768 + col1 * 2^-14 keeps every D1 = 768 + x + col1 * 2^-14 in
// the binade [512, 1024) (|x| <= 255), where the ulp is 2^-14: the low 14 mantissa bits of
// D1 ARE col1 and the bits above are x + 256. So bits(D1) ^ 0x3FFF orders by x, then by
// DEScending col1, and its minimum is the last minimum: NoDuplicates costs one v_xor per
// pair instead of a second (negated) product. Needs cols <= 16384.
constexpr float XK_BIAS = 768.f;
constexpr float XK_EPS = 1.f / 16384.f;
constexpr uint32_t XK_COL = 0x3FFFu;
// XK keys are block-relative: C is the same for every block, C = 768 + (XK_K0 + col1 % 32)
// * 2^-14, and the running minima are kept relative to the base col1 B of the block being
// reduced -- their col1 field is col1 - B + XK_K0 (first minimum) and 31 - (col1 - B) (last
// minimum, key ^ 0x3FFF), moved by -32 / +32 per block with ONE integer add each. Both
// fields stay inside [0, 16383] for B <= 16352 (cols <= 16384). This replaces the 16 float
// adds per block that advanced C (which the compiler packed into v_pk_add_f32, expensive
// beside MFMAs) and keeps C in registers that never change.
constexpr int XK_K0 = 16352;
// KEYS 2 (any block order): the relative col1 fields span +-cols, so C carries a
// mid-range offset instead -- first-minimum field col1 - B + 8160, last-minimum field
// 8223 - (col1 - B) -- which keeps both in [0, 16383] for cols <= 8160.
constexpr int XKF_K0 = 8160;
// KEYS: 0 = float keys (col1 * 2^-15 in C per block; NoDuplicates by a second, negated
//           product), any width;
//       1 = XK keys, blocks in ascending col1 order (cols <= 16384);
//       2 = XK keys in any block order with the last-minimum work skipped where it cannot
//           matter (NoDuplicates, cols <= 8160; see below);
//       3 = FK float keys, column in the free K half, ascending, no NoDuplicates
//           (cols <= 2048, see FK_EPS).
//
// KEYS 2. NoDuplicates needs the LAST column at the minimum cost only to compare it with
// the first; a block none of whose keys reaches the running minimum cost cannot hold it. So
// each tile's block minimum is combined over the two lane halves (tiles in pairs: one
// v_permlane32_swap of two tiles' minima, see pair_reduce) and tested against the tile's
// running first minimum (<= in cost), and the xor + min tree of the last minimum runs only
// for a tile some lane of which passes (one wave-uniform branch per pair). Blocks
// are visited from the wave's own col0 downwards (chunks from the workgroup's, wrapping):
// a stereo match lies at col1 <= col0 within a few blocks, the running minimum reaches it
// early, and the rest of the row skips that half of the VALU work (cfg2 synthetic: ~6 % of
// blocks still do it). The result is exact whatever the data: the order only changes speed.
// Keys stay relative to the base B of the block being reduced (shifts by the signed
// B - B_prev); C = 768 + (8160 + col1 % 32) * 2^-14 keeps both fields in [0, 16383].
//
// A workgroup scans one row for the col0 range [c0_base + tile * waves * T * 32, + waves * T *
// 32), c0_base = a.tail_col0 for the tail launch (search_plan.cpp tail_launch), else 0.
//
// ST (streamed right row; KEYS 2, 128-bit descriptors in 2 K-steps, every col0 of the row, no
// tail; the plan guarantees chunk = 2 * blockDim.x and cols > chunk). The workgroup's own
// chunk is expanded whole, as without ST, and every wave scans it from its own col0. The rest
// of the row then comes in stages of half a chunk = one col1 per thread, alternating between
// the two halves of the chunk region:
//  * the raw descriptor of a thread's column of the NEXT stage is requested before the block
//    loop over the current one and held in four VGPRs, so its latency runs under that loop
//    (the own chunk's loads go out ahead of the left B-fragment loads);
//  * a wave that is done with stage s expands its columns of stage s + 1 into the other half
//    at once -- every wave left that half's previous stage before the barrier that published
//    s -- and ONE barrier then publishes s + 1 and retires s. Only the step from the own chunk
//    (which fills both halves) to the first stage takes two.
// Without ST every chunk costs barrier -> loads -> expansion -> barrier with no wave of the
// workgroup multiplying. The stages run downwards from the own chunk (wrapping), upper half
// first; any order gives the same minima (KEYS 2).
//
// PRUNE (KEYS 2, 128-bit descriptors in 2 K-steps, tiles in pairs, main launches): the second
// K-step only where it can matter. The key carries x = ham - |a| = x_lo + x_hi, the sums over
// the two 64-bit K-steps, and x_hi = sum_k b_k (1 - 2 a_k) >= -|a_hi|, |a_hi| = the popcount
// of the left descriptor's words 2 and 3. So x >= x_lo - |a_hi|: if, after the FIRST K-step of
// a tile pair, every col0's block minimum of x_lo - |a_hi| lies strictly above that col0's
// running minimum cost, the block holds neither a new first minimum nor a tie (the last
// minimum), and its second K-step, its key reduction and its update of mp / m2 change
// nothing: they are skipped (block_pr; one wave-uniform branch per pair, both tiles taken
// when either reaches). The test is exact in the key's integer cost field (bits 14 and up
// of D = 768 + x + col * 2^-14, i.e. x + 256): it runs as x_lo <= running x + |a_hi|, the
// bits of D_lo against thr = (running minimum | column field) + (|a_hi| << 14). x_lo in
// [-64, 64] keeps D_lo in [704, 832]; the running x in [-128, 128] and |a_hi| <= 64 (62 for
// transform output) keep thr's cost field in [128, 448]: positive, and D stays in the binade
// [512, 1024), where adding to the bits IS the float addition. The comparison is "<=": a tie
// is never pruned (NoDuplicates needs it). A pruned pair skips its update, so mp[p] keeps
// its own previous base bpp[p], as m2[t] has b2[t].
// Fallback: where true matches are poor (costs above ~10 of 126 bits) or absent, every
// block reaches and the test is pure overhead. A wave counts its reaching pair-blocks (SALU,
// from the ballots the branch takes anyway) over windows of PRUNE_WINDOW visited blocks, all
// through the scan; a window in which >= 7/8 of them reached sends the wave to the unpruned
// loop for the rest of the row (PRUNE_WINDOW: search_plan.hpp, shared with
// search_pk.hip's pruned kernel).

// Diagnostic builds (tools/build_diag.sh, -DBICOS_MX_DIAG=1..5; results are WRONG, timing only):
// 1 = MFMA skeleton, one key per tile; 2 = + the first-minimum tree only; 3 = the real kernel
// with only the first chunk of each row expanded; 4 = the last-minimum path never taken (its
// branch kept); 5 = no last-minimum branch at all. 0: the search.
#ifndef BICOS_MX_DIAG
#define BICOS_MX_DIAG 0
#endif
constexpr int MX_DIAG = BICOS_MX_DIAG;

// One instantiation of search_mx_kernel: what the launch plan sets (SearchVariant's fields of
// the same names, search_plan.hpp) and everything the kernel derives from it.
template <int WORDS_, int KSTEPS_, bool NODUPES_, int T_, int KEYS_, bool TAIL_, bool LIST_, bool AGREE_,
          bool STREAM_, bool PRUNE_>
struct MxVariant {
    static constexpr int WORDS = WORDS_;       // 32-bit words per descriptor
    // 64-bit K-steps: KS <= WORDS / 2 -- the steps past the highest descriptor bit the
    // transform writes are all zero on both sides and contribute nothing (n = 40 LIMITED:
    // 154 of 256 bits -> 3 steps, not 4)
    static constexpr int KS = KSTEPS_;
    static constexpr bool NODUPES = NODUPES_;
    static constexpr int T = T_;               // 32-col0 tiles per wave
    static constexpr int KEYS = KEYS_;         // key scheme, see above
    static constexpr bool TAIL = TAIL_;        // the col0 from a.tail_col0 on
    static constexpr bool LIST = LIST_;        // compacted col0
    static constexpr bool AG = AGREE_;         // the fused agree epilogue
    static constexpr bool STREAM = STREAM_;    // ST
    static constexpr bool PRUNE = PRUNE_;

    static constexpr int WL = 2 * KS;          // LDS word slots per col1 (W=1: 1 pad)
    static constexpr bool FK = KEYS == 3;
    static constexpr bool XK = KEYS == 1 || KEYS == 2;
    static constexpr bool FREE = KEYS == 2;    // any block order
    static constexpr int K0 = FREE ? XKF_K0 : XK_K0;
    // PAIRS (KEYS 2): the running first minima of tiles 2p / 2p+1 share register mp[p]
    // (lanes 0-31 / 32-63: the halves that write those tiles), see pair_reduce
    // (diagnostic floors 1 and 2 reduce per tile: m1[] must stay live)
    static constexpr bool PAIRS = FREE && T % 2 == 0 && MX_DIAG != 1 && MX_DIAG != 2;
    // one pair per wave: the block loop is software-pipelined (see the FREE chunk loop)
    static constexpr bool PIPE = PAIRS && T == 2 && KS <= 3;
    static constexpr bool PR = PRUNE && PAIRS;
    // XK full blocks: the next block's A fragments are read while this one is reduced.
    // Only where the registers allow (paired NoDuplicates tiles, <= 2 K-steps): cfg2 -1.5 %,
    // cfg5 -1 %; with 3 K-steps the extra live fragments spill inside the loop (cfg4 2.3x
    // slower)
    // (FK at 3 K-steps: 25 registers spill even with the C matrix gone)
    static constexpr bool PREFETCH = XK && PAIRS && KS <= 2;
    static constexpr int NP = T / 2 > 0 ? T / 2 : 1;  // tile pairs (at least one slot)

    static_assert(!PRUNE || (KEYS == 2 && T % 2 == 0 && WORDS == 4 && KS == 2 && !TAIL && !LIST),
                  "PRUNE: the 128-bit any-order NoDuplicates search's main launches");
    static_assert(!STREAM || (KEYS == 2 && T % 2 == 0 && WORDS == 4 && KS == 2 && !TAIL && !LIST),
                  "ST: the 128-bit any-order NoDuplicates search over every col0");
    static_assert(!FK || !NODUPES, "FK keys: first minimum only");
    static_assert(!FREE || NODUPES, "KEYS 2 is the NoDuplicates search");
    static_assert(KS >= 1 && 2 * KS <= (WORDS >= 2 ? WORDS : 2), "K-steps exceed the descriptor");
};

template <class V>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(V::KS >= 4 ? 3 : 4)))
void search_mx_kernel(typename SearchKArgs<V::AG>::type ka) {
    const SearchArgs& a = search_part(ka);
    constexpr int WORDS = V::WORDS, KS = V::KS, T = V::T, WL = V::WL, K0 = V::K0;
    constexpr bool NODUPES = V::NODUPES, TAIL = V::TAIL, LIST = V::LIST, AG = V::AG, STREAM = V::STREAM;
    constexpr bool FK = V::FK, XK = V::XK, FREE = V::FREE;
    constexpr bool PAIRS = V::PAIRS, PIPE = V::PIPE, PR = V::PR, PREFETCH = V::PREFETCH;
    extern __shared__ __attribute__((aligned(16))) v4i lds_mx[];  // [WL][chunk]

    const int nwg = gridDim.x;
    const int bid = blockIdx.x;
    // XCD-aware order (as xcd_row_tile, search_dev.hpp; written out here: through the helper
    // the streamed and fused 128-bit instantiations, at 128 VGPRs, schedule differently)
    const int per_xcd = (nwg + 7) / 8;
    int logical = (bid % 8) * per_xcd + bid / 8;
    if (nwg % 8 != 0) logical = bid;
    int row = logical / a.tiles_per_row;
    int tile = logical % a.tiles_per_row;
    if constexpr (LIST) {
        list_row_tile(a.tiles_per_row, a.rows, row, tile);
        if (row >= a.rows) return;
    }
    const int c0_base = TAIL ? a.tail_col0 : 0;

    const int lane = threadIdx.x & 63;
    // wave-uniform, so the block loop's indices and addresses live in SGPRs (the SALU
    // computes them; the VALU issue slots beside the MFMAs are the scarce resource)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int h = lane >> 5;
    const int j = lane & 31;
    const int cols = a.cols;
    const int chunk = a.chunk;
    const int waves = blockDim.x >> 6;
    const int c0_wave = c0_base + (tile * waves + wave) * (T * 32);
    // col0 entries of this row (LIST: the compacted count, found by the prologue; the
    // workgroup's entry columns in LDS past the chunk region)
    int lcols = cols;
    const int e0 = c0_base + tile * waves * T * 32;
    int16_t* ent = nullptr;
    // LIST, dense row (row_valid): identity entries, no prologue
    bool dense = false;
    if constexpr (LIST) {
        ent = (int16_t*)((char*)lds_mx + list_ent_offset(WL * chunk * 16));
        dense = a.row_valid != nullptr && dense_row(a, row);
        if (!dense)
            lcols = list_prologue(a.keep + (size_t)row * a.keep_pitch, cols, (uint32_t*)lds_mx, ent,
                                  e0, waves * T * 32);
        if (!TAIL) lcols = min(lcols, a.tail_col0);  // the tail launch takes the entries past it
        if (e0 >= lcols) return;  // the whole workgroup, past the prologue's barriers
    }
    // LIST: the column of entry i (ascending in i); the block order's start for entries < e
    auto lcol = [&](int i) { return LIST && !dense ? (int)ent[i - e0] : i; };
    auto start_col = [&](int e, int ahead) {
        return LIST ? min(cols - 1, lcol(min(e, lcols) - 1) + ahead) : min(cols - 1, e - 1);
    };

    const uint32_t* __restrict__ row0 = a.desc0 + (size_t)row * a.desc_pitch;
    const uint32_t* __restrict__ row1 = a.desc1 + (size_t)row * a.desc_pitch;

    // ST: the raw right descriptor of col1 (zero past the image), and the own chunk's two
    // columns of this thread, requested ahead of the B-fragment loads below
    auto raw_col = [&](int c1) {
        v4i x = {0, 0, 0, 0};
        if (c1 < cols) {
#pragma unroll
            for (int w = 0; w < 4; ++w) x[w] = (int)row1[(size_t)c1 * WORDS + w];
        }
        return x;
    };
    auto put_col = [&](int c, const v4i& x) {  // LDS column c of the chunk region
#pragma unroll
        for (int w = 0; w < 4; ++w) lds_mx[w * chunk + c] = expand_bits((uint32_t)x[w], LUT_A);
    };
    // this thread's index, recomputed where it is used (a register less across the block loops)
    auto thread_index = [&]() {
        int l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return 64 * wave + l;
    };
    const int half = chunk >> 1;
    const int own_chunk = (min(cols, c0_base + (tile + 1) * waves * T * 32) - 1) / chunk;
    v4i raw = {0, 0, 0, 0}, raw_hi = {0, 0, 0, 0};
    if constexpr (STREAM) {
        raw = raw_col(own_chunk * chunk + (int)threadIdx.x);
        raw_hi = raw_col(own_chunk * chunk + half + (int)threadIdx.x);
    }

    // B fragments: +1 (0x2) where the left bit is 0, -1 (0xA) where it is 1
    v4i bf[T][KS];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int c0 = c0_wave + 32 * t + j;
        const int cl = c0 < lcols ? lcol(c0) : 0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int w = 2 * s + h;
            uint32_t x = 0;
            if (c0 < lcols && w < WORDS) x = row0[(size_t)cl * WORDS + w];
            if (WORDS == 8 && KS == 4 && w == 7) x &= 0x7FFFFFFFu;  // bit 255 masked (as desc_word)
            bf[t][s] = expand_bits(x, LUT_B);
        }
    }

    uint32_t m1[T], m2[T], mp[V::NP];
    int b2[T];  // KEYS 2: the base m2[t] is relative to (wave-uniform)
#pragma unroll
    for (int t = 0; t < T; ++t) {
        m1[t] = XK || FK ? XK_INF : KEY_NONE;  // (FK: a huge positive float)
        m2[t] = XK ? XK_INF : 0u;
        b2[t] = 0;
    }
#pragma unroll
    for (int p = 0; p < V::NP; ++p) mp[p] = XK_INF;
    // PRUNE: |a_hi| of the col0 whose running minimum this lane homes (tile 2p in lanes 0-31,
    // tile 2p+1 in lanes 32-63), in the key's cost field; the base mp[p] is relative to; the
    // fallback's state (wave-uniform)
    uint32_t ah[V::NP];
    // ... and the test's threshold: the running minimum's cost raised by |a_hi|, its column
    // field all ones (the same in every block's frame), renewed where mp[p] changes
    uint32_t thr[V::NP];
    int bpp[V::NP];
    bool prune_on = PR;
    int wblocks = 0, wreach = 0;
#pragma unroll
    for (int p = 0; p < V::NP; ++p) {
        ah[p] = 0u;
        bpp[p] = 0;
        if constexpr (PR) {
            const int c0 = c0_wave + 32 * (2 * p + h) + j;
            if (c0 < lcols) {
                const uint32_t* q = row0 + (size_t)lcol(c0) * WORDS;
                ah[p] = (uint32_t)(__popc(q[2]) + __popc(q[3])) << 14;
            }
        }
        thr[p] = (XK_INF | XK_COL) + ah[p];
    }

    // row offset of accumulator register r in this lane half
    auto rrow = [&](int r) { return (r & 3) + 8 * (r >> 2) + 4 * h; };

    v16f d[T], e[T];
    // products of tile `tile` into accumulator slot `slot`
    const int fk_sa = h ? FK_SCALE_E8M0 : 127;  // FK: the column half of the last step x 2^-12
    auto products = [&](int slot, const v4i* af, const v4i* an, const v16f& c1, const v16f& c2,
                        int tile) {
        if constexpr (FK && KS == 1) {
            d[slot] = mfma_fp4_sa(af[0], bf[tile][0], c1, fk_sa);
        } else {
            d[slot] = mfma_fp4(af[0], bf[tile][0], c1);
        }
#pragma unroll
        for (int s = 1; s < KS; ++s) {
            if (FK && s == KS - 1)
                d[slot] = mfma_fp4_sa(af[s], bf[tile][s], d[slot], fk_sa);
            else
                d[slot] = mfma_fp4(af[s], bf[tile][s], d[slot]);
        }
        if constexpr (NODUPES && !XK) {
            e[slot] = mfma_fp4(an[0], bf[tile][0], c2);
#pragma unroll
            for (int s = 1; s < KS; ++s) e[slot] = mfma_fp4(an[s], bf[tile][s], e[slot]);
        }
    };
    // block at base B, the previous one at base bp (XK: the running minima move from bp's
    // frame to B's first)
    auto reduce = [&](int t, int B, int bp) {
        if constexpr (MX_DIAG == 1) {  // MFMA skeleton: one key per tile
            m1[t] = min(m1[t], fbits(d[t][0]));
        } else if constexpr (MX_DIAG == 2) {  // + the first-minimum tree only
            m1[t] = min16(d[t], m1[t], 0u);
        } else if constexpr (FREE) {
            const uint32_t m1s = m1[t] - (uint32_t)(B - bp);
            const uint32_t bm = min16(d[t], KEY_NONE, 0u);      // this half's block minimum
            // cost <= running minimum cost (MX_DIAG 4: never)
            const bool reach = bm <= (m1s | XK_COL) && (MX_DIAG != 4 || bm == 0u);
            const auto sw = __builtin_amdgcn_permlane32_swap(bm, bm, false, false);
            m1[t] = umin3(m1s, sw[0], sw[1]);                  // both halves' minimum
            if (MX_DIAG != 5 && __builtin_amdgcn_ballot_w64(reach)) {
                m2[t] = min16(d[t], m2[t] + (uint32_t)(B - b2[t]), XK_COL);
                b2[t] = B;
            }
        } else if constexpr (FK) {
            m1[t] = fbits(fmin16(d[t], bitsf(m1[t]) - 32.f * FK_EPS));
        } else if constexpr (XK) {
            m1[t] = min16(d[t], m1[t] - 32u, 0u);
            if constexpr (NODUPES) m2[t] = min16(d[t], m2[t] + 32u, XK_COL);
        } else {
            m1[t] = min16(d[t], m1[t], 0u);
            if constexpr (NODUPES) m2[t] = max16(e[t], m2[t]);
        }
    };
    int bprev = (XK || FK) && !FREE ? -32 : 0;  // base of the previously reduced block
    // KEYS 2, tiles in pairs (2p, 2p+1) for block base B (accumulators dx, dy): ONE
    // v_permlane32_swap of the two block minima leaves tile 2p's both-halves minimum in
    // lanes 0-31 and tile 2p+1's in lanes 32-63 (swap: vdst lanes 32-63 <-> src lanes 0-31),
    // where the pair's running first minima mp[p] live; one wave-uniform branch per pair,
    // then a scalar test per tile of the ballot's halves. The caller sets bprev = B after.
    auto pair_reduce = [&](int p, int B, const v16f& dx, const v16f& dy) {
        const uint32_t x = min16(dx, KEY_NONE, 0u);
        const uint32_t y = min16(dy, KEY_NONE, 0u);
        const auto sw = __builtin_amdgcn_permlane32_swap(x, y, false, false);
        const uint32_t comb = min((uint32_t)sw[0], (uint32_t)sw[1]);
        const uint32_t ms = mp[p] - (uint32_t)(B - (PR ? bpp[p] : bprev));
        if constexpr (PR) bpp[p] = B;
        // cost <= running minimum cost (MX_DIAG 4: never)
        const bool reach = comb <= (ms | XK_COL) && (MX_DIAG != 4 || comb == 0u);
        mp[p] = min(ms, comb);
        if constexpr (MX_DIAG == 5) {  // no last-minimum branch at all
            if (reach) m2[2 * p] ^= 0u;
            return;
        }
        const uint64_t bal = __builtin_amdgcn_ballot_w64(reach);
        // (halves as opaque SGPRs: left alone the compiler tests the upper one with a 64-bit
        // VALU compare)
        uint32_t lo = (uint32_t)bal, hi = (uint32_t)(bal >> 32);
        asm volatile("" : "+s"(lo), "+s"(hi));
        if (lo) {
            m2[2 * p] = min16(dx, m2[2 * p] + (uint32_t)(B - b2[2 * p]), XK_COL);
            b2[2 * p] = B;
        }
        if (hi) {
            m2[2 * p + 1] = min16(dy, m2[2 * p + 1] + (uint32_t)(B - b2[2 * p + 1]), XK_COL);
            b2[2 * p + 1] = B;
        }
    };
    // XK: the C of every block (col1 % 32 only)
    v16f cx;
#pragma unroll
    for (int r = 0; r < 16; ++r) cx[r] = XK_BIAS + (float)(K0 + rrow(r)) * XK_EPS;

    const bool idle = c0_wave >= lcols;  // wave-uniform; still joins the barriers
    const int nchunks = (cols + chunk - 1) / chunk;
    // FREE: chunks downwards from the one holding the workgroup's highest col0
    int cstart = 0;
    if constexpr (FREE) cstart = start_col(c0_base + (tile + 1) * waves * T * 32, 0) / chunk;
    // ST: streamed stage s (after the own chunk) starts at col1 stage_base(s) and lives in
    // half s & 1 of the chunk region; 2 (nchunks - 1) of them, the last chunk's possibly
    // short or empty (they still take their barrier: workgroup-uniform)
    auto stage_base = [&](int s) {
        int ci = own_chunk - 1 - (s >> 1);
        if (ci < 0) ci += nchunks;
        return ci * chunk + ((s & 1) ? 0 : half);
    };
    const int nstages = STREAM ? 2 * (nchunks - 1) : 0;
    const int nsteps = STREAM ? 1 + nstages : nchunks;
    if constexpr (STREAM) {
        put_col((int)threadIdx.x, raw);
        put_col(half + (int)threadIdx.x, raw_hi);
    }
    for (int k = 0; k < nsteps; ++k) {
        // this step's columns: col1 base + c for LDS column c, from LDS block b0, ncols of them
        int base, ncols, b0 = 0;
        const bool expand = MX_DIAG != 3 || k == 0;  // (MX_DIAG 3: the first chunk only)
        if constexpr (STREAM) {
            if (k == 0) {
                base = own_chunk * chunk;
                ncols = min(chunk, cols - base);
            } else {
                const int sbase = stage_base(k - 1);
                b0 = ((k - 1) & 1) ? half >> 5 : 0;
                base = sbase - 32 * b0;
                ncols = max(0, min(half, cols - sbase));
            }
            if (expand) {
                if (k == 1) __syncthreads();  // every wave is done with the own chunk
                const int tid = thread_index();
                if (k >= 1) put_col(32 * b0 + tid, raw);
                if (k < nstages) raw = raw_col(stage_base(k) + tid);  // the next stage's
                __syncthreads();
            }
        } else {
            int ci = FREE ? cstart - k : k;
            if (ci < 0) ci += nchunks;
            base = ci * chunk;
            ncols = min(chunk, cols - base);
            if (k && expand) __syncthreads();
            // expand the chunk's right descriptors: one col1 per thread, all its words
            for (int c = threadIdx.x; expand && c < chunk; c += blockDim.x) {
                const int c1 = base + c;
#pragma unroll
                for (int w = 0; w < WL; ++w) {
                    const uint32_t x = desc_word<WORDS, KS>(row1, c1, w, c1 < cols);
                    if (FK && w == WL - 1)  // (the descriptors leave this slot 0: host check)
                        lds_mx[w * chunk + c] = fk_digits(c1 & 31);
                    else
                        lds_mx[w * chunk + c] = expand_bits(x, LUT_A);
                }
            }
            if (expand) __syncthreads();
        }
        if (idle) continue;

        const int nfull = ncols / 32;
        const bool partial = (ncols & 31) != 0;
        v16f cc;  // C of the current block: BIAS + col1 * EPS (XK: cx, the same for all)
        if constexpr (FK) {
#pragma unroll
            for (int r = 0; r < 16; ++r) cc[r] = 0.f;  // C = 0: an inline constant
        } else if constexpr (XK) {
            cc = cx;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) cc[r] = KEY_BIAS + (float)(base + rrow(r)) * KEY_EPS;
        }
        auto block = [&](int b, const v16f& c1, const v16f& c2) {
            const int B = base + 32 * b;
            v4i af[KS], an[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) af[s] = lds_mx[(2 * s + h) * chunk + 32 * b + j];
            if constexpr (FREE && PAIRS) {
#pragma unroll
                for (int p = 0; p < T / 2; ++p) {
                    products(0, af, an, c1, c2, 2 * p);
                    products(1, af, an, c1, c2, 2 * p + 1);
                    pair_reduce(p, B, d[0], d[1]);
                }
                bprev = B;
                return;
            }
            if constexpr (NODUPES && !XK) {
#pragma unroll
                for (int s = 0; s < KS; ++s)
#pragma unroll
                    for (int q = 0; q < 4; ++q) an[s][q] = af[s][q] | (af[s][q] << 2);  // 1.0 -> -1.0
            }
            // tile t+1's products are issued before tile t's keys are reduced, so the MFMAs
            // overlap the reduction (and its branch) within the wave
            products(0, af, an, c1, c2, 0);
#pragma unroll
            for (int t = 0; t < T; ++t) {
                if (t + 1 < T) products(t + 1, af, an, c1, c2, t + 1);
                reduce(t, B, bprev);
            }
            bprev = B;
        };
        // XK full blocks with the A fragments of the next block prefetched: `af` holds block
        // b's fragments on entry; right after the last products that read them are issued,
        // the ds_reads of block `nb` (if >= 0) go out into the same registers, so their
        // latency runs under this block's remaining key reductions
        auto load_af = [&](v4i* af, int b) {
#pragma unroll
            for (int s = 0; s < KS; ++s) af[s] = lds_mx[(2 * s + h) * chunk + 32 * b + j];
        };
        auto block_pf = [&](int b, v4i* af, int nb) {
            const int B = base + 32 * b;
            v4i an[KS];
            if constexpr (FREE && PAIRS) {
#pragma unroll
                for (int p = 0; p < T / 2; ++p) {
                    products(0, af, an, cc, cc, 2 * p);
                    products(1, af, an, cc, cc, 2 * p + 1);
                    if (p + 1 == T / 2 && nb >= 0) load_af(af, nb);
                    pair_reduce(p, B, d[0], d[1]);
                }
            } else {
                products(0, af, an, cc, cc, 0);
                if (T == 1 && nb >= 0) load_af(af, nb);
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    if (t + 1 < T) {
                        products(t + 1, af, an, cc, cc, t + 1);
                        if (t + 2 == T && nb >= 0) load_af(af, nb);
                    }
                    reduce(t, B, bprev);
                }
            }
            bprev = B;
        };
        // PRUNE: a full block with the second K-step only for the pairs that can reach (see
        // the kernel's header). af0 holds the block's K-step 0 fragment on entry and block
        // nb's (the next one) on return, read once the last K-step 0 products are
        // issued; the K-step 1 fragment is read here, ahead of the first test. Counts the
        // reaching pairs into wreach.
        auto block_pr = [&](int b, v4i& af0, int nb) {
            const int B = base + 32 * b;
            if constexpr (PR) {
                const v4i af1 = lds_mx[(2 + h) * chunk + 32 * b + j];
#pragma unroll
                for (int p = 0; p < T / 2; ++p) {
                    d[0] = mfma_fp4(af0, bf[2 * p][0], cc);
                    d[1] = mfma_fp4(af0, bf[2 * p + 1][0], cc);
                    // (both products go out before the first key is read: left alone the
                    // scheduler may put tile 2p's whole tree ahead of tile 2p+1's product)
                    __builtin_amdgcn_sched_barrier(0);
                    if (p + 1 == T / 2) af0 = lds_mx[h * chunk + 32 * nb + j];
                    // the first half of pair_reduce on the partial keys
                    const uint32_t x = min16(d[0], KEY_NONE, 0u);
                    const uint32_t y = min16(d[1], KEY_NONE, 0u);
                    const auto sw = __builtin_amdgcn_permlane32_swap(x, y, false, false);
                    // x_lo - |a_hi| <= running x as x_lo <= thr; "<=": a tie reaches
                    const uint32_t lb = min((uint32_t)sw[0], (uint32_t)sw[1]);
                    if (__builtin_amdgcn_ballot_w64(lb <= thr[p])) {
                        d[0] = mfma_fp4(af1, bf[2 * p][1], d[0]);
                        d[1] = mfma_fp4(af1, bf[2 * p + 1][1], d[1]);
                        __builtin_amdgcn_sched_barrier(0);
                        pair_reduce(p, B, d[0], d[1]);
                        thr[p] = (mp[p] | XK_COL) + ah[p];
                        ++wreach;
                    }
                }
            }
            bprev = B;
        };
        // the block reaching past the image (last chunk): A = 0 there, so D1 = KEY_PAD,
        // D2 = 0 never win. Ascending orders take it last, FREE first.
        auto partial_block = [&](const v16f& cb) {
            if constexpr ((STREAM || PR) && PAIRS) {
                // (no second C matrix, whose 16 registers would spill beside `raw` or the
                // pruned loop's state: the rows past the image are set to KEY_PAD after the
                // products -- the same D)
                const int b = b0 + nfull, B = base + 32 * b;
                v4i af[KS];
#pragma unroll
                for (int s = 0; s < KS; ++s) af[s] = lds_mx[(2 * s + h) * chunk + 32 * b + j];
#pragma unroll
                for (int p = 0; p < T / 2; ++p) {
                    products(0, af, af, cb, cb, 2 * p);
                    products(1, af, af, cb, cb, 2 * p + 1);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool in = 32 * nfull + rrow(r) < ncols;
                        d[0][r] = in ? d[0][r] : KEY_PAD;
                        d[1][r] = in ? d[1][r] : KEY_PAD;
                    }
                    pair_reduce(p, B, d[0], d[1]);
                    if constexpr (PR) thr[p] = (mp[p] | XK_COL) + ah[p];
                }
                bprev = B;
                return;
            }
            v16f c1, c2;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool in = 32 * nfull + rrow(r) < ncols;
                c1[r] = in ? cb[r] : KEY_PAD;
                c2[r] = in ? cb[r] : 0.f;
            }
            block(b0 + nfull, c1, c2);
        };
        if constexpr (FREE) {
            if (partial) partial_block(cc);
            // full blocks downwards from the one holding the wave's highest col0 (clamped)
            // (block indices below are relative to the step's first LDS block b0)
            const int sb = max(0, min(nfull - 1, (start_col(c0_wave + 32 * T, REV_AHEAD) - base - 32 * b0) / 32));
            // PRUNE: the pruned loop over the first i0 blocks of the visiting order -- all of
            // them unless a window of PRUNE_WINDOW blocks had >= 7/8 of its pair-blocks reach,
            // which sends the wave to the loops below for the rest of the row
            int i0 = 0;
            if constexpr (PR) {
                if (prune_on && nfull > 0) {
                    // The scalar unit's instructions take issue slots of the wave like the
                    // VALU's, so the loop carries little of them: the blocks
                    // up to the end of the fallback's window run in an inner loop that only
                    // steps the block index (wrapping) and counts down -- the window is looked
                    // at between two such runs -- and the next block's fragment is read
                    // unconditionally (behind the row's last block: the wrapped index, a block
                    // of this step that nobody uses).
                    int b = sb;
                    v4i af0 = lds_mx[h * chunk + 32 * (b0 + b) + j];
                    while (i0 < nfull) {
                        int n = min(nfull - i0, PRUNE_WINDOW - wblocks);
                        i0 += n;
                        wblocks += n;
                        for (; n > 0; --n) {
                            const int nb = b > 0 ? b - 1 : nfull - 1;
                            block_pr(b0 + b, af0, b0 + nb);
                            b = nb;
                        }
                        if (wblocks == PRUNE_WINDOW) {
                            const bool fall = 8 * wreach >= 7 * PRUNE_WINDOW * (T / 2);
                            wblocks = wreach = 0;
                            if (fall) {
                                prune_on = false;
                                break;
                            }
                        }
                    }
                }
            }
            if constexpr (PIPE) {
                // software pipeline over the blocks (one tile pair per wave): the products of
                // block i+1 are issued before block i is reduced, so the wave's MFMAs stay in
                // flight during its own key reduction (accumulator sets A / B alternate)
                v16f dA[2], dB[2];
                int BA = 0, BB = 0;
                auto issue = [&](int i, v16f* dd) {
                    int b = sb - i;
                    if (b < 0) b += nfull;
                    b += b0;
                    v4i af[KS];
#pragma unroll
                    for (int s = 0; s < KS; ++s) af[s] = lds_mx[(2 * s + h) * chunk + 32 * b + j];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        dd[u] = mfma_fp4(af[0], bf[u][0], cc);
#pragma unroll
                        for (int s = 1; s < KS; ++s) dd[u] = mfma_fp4(af[s], bf[u][s], dd[u]);
                    }
                    return base + 32 * b;
                };
                auto finish = [&](int B, const v16f* dd) {
                    pair_reduce(0, B, dd[0], dd[1]);
                    bprev = B;
                };
                if (i0 < nfull) {
                    BA = issue(i0, dA);
                    for (int i = i0;;) {
                        if (i + 1 < nfull) BB = issue(i + 1, dB);
                        finish(BA, dA);
                        if (++i >= nfull) break;
                        if (i + 1 < nfull) BA = issue(i + 1, dA);
                        finish(BB, dB);
                        if (++i >= nfull) break;
                    }
                }
            } else if constexpr (PREFETCH) {
                auto bidx = [&](int i) {
                    int b = sb - i;
                    return b0 + (b < 0 ? b + nfull : b);
                };
                v4i af[KS];
                if (i0 < nfull) load_af(af, bidx(i0));
                for (int i = i0; i < nfull; ++i) block_pf(bidx(i), af, i + 1 < nfull ? bidx(i + 1) : -1);
            } else {
                for (int i = 0; i < nfull; ++i) {
                    int b = sb - i;
                    if (b < 0) b += nfull;
                    block(b0 + b, cc, cc);
                }
            }
        } else if constexpr ((XK || FK) && PREFETCH) {
            v4i af[KS];
            if (nfull > 0) load_af(af, 0);
            for (int b = 0; b < nfull; ++b) block_pf(b, af, b + 1 < nfull ? b + 1 : -1);
            if (partial) partial_block(cc);
        } else {
            for (int b = 0; b < nfull; ++b) {
                if constexpr (!XK && !FK) {
                    if (b) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) cc[r] += 32.f * KEY_EPS;  // exact (same binade)
                    }
                }
                block(b, cc, cc);
            }
            if (partial) {
                if constexpr (!XK && !FK) {
                    if (nfull) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) cc[r] += 32.f * KEY_EPS;
                    }
                }
                partial_block(cc);
            }
        }
    }
    if (!AG && idle) return;
    // AG: the workgroup's integer results go through LDS to the fused agree below; the chunk
    // region is reused once every wave is done with its blocks
    int16_t* raw_lds = reinterpret_cast<int16_t*>(lds_mx);
    const int wg_c0 = c0_base + tile * waves * T * 32;
    if constexpr (AG) __syncthreads();

    // the two lane halves hold the even / odd 4-row groups of every block
    if constexpr (PR) {
#pragma unroll
        for (int p = 0; p < T / 2; ++p) mp[p] -= (uint32_t)(bprev - bpp[p]);  // as m2 below
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if constexpr (FREE) m2[t] += (uint32_t)(bprev - b2[t]);  // into the last block's frame
        if constexpr (PAIRS)  // already merged; valid in the half that writes tile t
            m1[t] = mp[t / 2];
        else if constexpr (FK)
            m1[t] = fbits(__builtin_fminf(bitsf(m1[t]), bitsf((uint32_t)__shfl_xor((int)m1[t], 32))));
        else
            m1[t] = min(m1[t], (uint32_t)__shfl_xor((int)m1[t], 32));
        if constexpr (NODUPES && XK) m2[t] = min(m2[t], (uint32_t)__shfl_xor((int)m2[t], 32));
        else if constexpr (NODUPES) m2[t] = max(m2[t], (uint32_t)__shfl_xor((int)m2[t], 32));
    }
    // best col1 of tile t, and whether it is the only column at the minimum cost
    // (XK: the minima are relative to the base of the last block reduced)
    auto best_of = [&](int t) {
        if constexpr (FK) {
            const float v = bitsf(m1[t]);
            return bprev + (int)((v - __builtin_rintf(v)) * 4096.f);  // exact (see FK_EPS)
        }
        return XK ? (int)(m1[t] & XK_COL) - K0 + bprev : key_col(m1[t]);
    };
    auto unique_of = [&](int t, int best) {
        if constexpr (NODUPES && XK)
            return (int)(XK_COL - K0) - (int)(m2[t] & XK_COL) + bprev == best;
        else if constexpr (NODUPES) return key_col(m2[t]) == best;
        return true;
    };
    int16_t* out = a.out + (size_t)row * a.out_pitch;
    // (lane index made opaque: otherwise the compiler hoists these addresses into the
    // prologue, where they share c0 with the B-fragment loads, and spills them to scratch
    // across the whole search -- 68 MB of scratch writes per cfg2 launch)
    int jo = j;
    asm volatile("" : "+v"(jo));
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if ((t & 1) != h) continue;  // half 0 writes even tiles, half 1 odd tiles
        const int c0i = c0_wave + 32 * t + jo;
        if constexpr (!LIST && !AG) {  // dense-row fast path: this tile's valid count
            if (a.row_valid)
                tile_valid_store(a, row, c0_wave + 32 * t,
                                 c0i < lcols && unique_of(t, best_of(t)), best_of(t), jo == 0);
        }
        if (idle || c0i >= lcols) continue;
        const int c0 = lcol(c0i);
        const int best = best_of(t);
        const bool ok = unique_of(t, best);
        int16_t v;
        if (a.out_mode == 0)
            v = ok ? (int16_t)(c0 - best) : INVALID_I16;
        else
            v = ok ? (int16_t)best : (int16_t)-1;
        // (AG: only the agree reads the integer map, from LDS -- no HBM copy)
        if constexpr (AG)
            raw_lds[c0 - wg_c0] = v;
        else
            out[c0] = v;
    }
    if constexpr (AG) {
        __syncthreads();
        fused_agree<FUSED_AGREE_N>(ka.ag, row, wg_c0, min(waves * T * 32, cols - wg_c0), raw_lds);
    }
}

// The instantiations that are built (the launch plan, search_plan.cpp, asks for no other):
// every width in its K-steps; main launches of 2 or 4 tiles per wave, or 8 where they fit,
// with the key schemes of their search (first minimum: 0, 1, 3; NoDuplicates: 0, 1, 2), whole
// rows or compacted; KEYS 2 tails of 1 or 2 tiles; and the 128-bit KEYS 2 search over every
// col0 with any of the fused agree, the streamed row and the pruned second K-step.
constexpr bool mx_built(const SearchVariant& v) {
    const bool width = (v.words == 1 && v.ksteps == 1) || (v.words == 2 && v.ksteps == 1) ||
                       (v.words == 4 && v.ksteps == 2) || (v.words == 8 && (v.ksteps == 3 || v.ksteps == 4));
    const bool keys = v.keys == 0 || v.keys == 1 || v.keys == (v.nodupes ? 2 : 3);
    if (!width || !keys) return false;
    if (v.agree || v.stream || v.prune)
        return v.words == 4 && v.nodupes && v.keys == 2 && (v.T == 2 || v.T == 4) && !v.tail && !v.list;
    if (v.tail) return v.keys == 2 && (v.T == 1 || v.T == 2);
    return v.T == 2 || v.T == 4 || (v.T == 8 && mx_tiles_fit(v.words, v.nodupes, v.keys, 8));
}

}  // namespace

hipError_t launch_mx_variant(const SearchLaunch& l, const SearchArgs& a, const AgreeArgs* ag,
                             hipStream_t st) {
    const SearchVariant& v = l.v;
    if (v.packed) {
        // the same geometry on packed keys (search_pk.hip search_pkp_kernel): two 32-col0 tiles are one
        // wide tile, the drops lazy
        SearchLaunch pl = l;
        pl.v.family = SearchFamily::pk;
        pl.v.T = v.T / 2;
        pl.v.lazy = true;
        return launch_pk_variant(pl, a, ag, st);
    }
    // clang-format off
    return pick<int, 1, 2, 4, 8>(v.words, [&](auto words) {
    return pick<int, 1, 2, 3, 4>(v.ksteps, [&](auto ksteps) {
        if constexpr (!mx_built(SearchVariant{SearchFamily::mx, words.value, ksteps.value, false, 2}))
            return hipErrorInvalidValue;  // (no such width: nothing below it is built)
        else
    return pick<bool, false, true>(v.nodupes, [&](auto nodupes) {
    return pick<int, 1, 2, 4, 8>(v.T, [&](auto T) {
    return pick<int, 0, 1, 2, 3>(v.keys, [&](auto keys) {
    return pick<bool, false, true>(v.tail, [&](auto tail) {
        if constexpr (!mx_built(SearchVariant{SearchFamily::mx, words.value, ksteps.value, nodupes.value,
                                              T.value, keys.value, tail.value}))
            return hipErrorInvalidValue;  // (not built over whole rows: nor in any other form)
        else
    return pick<bool, false, true>(v.list, [&](auto list) {
    return pick<bool, false, true>(v.agree, [&](auto agree) {
    return pick<bool, false, true>(v.stream, [&](auto stream) {
    return pick<bool, false, true>(v.prune, [&](auto prune) {
        constexpr SearchVariant cv{SearchFamily::mx, words.value, ksteps.value, nodupes.value, T.value,
                                   keys.value, tail.value, list.value, agree.value, stream.value,
                                   prune.value};
        if constexpr (mx_built(cv)) {
            using V = MxVariant<cv.words, cv.ksteps, cv.nodupes, cv.T, cv.keys, cv.tail, cv.list, cv.agree,
                                cv.stream, cv.prune>;
            return launch_planned<cv.agree>(search_mx_kernel<V>, l, a, ag, st);
        } else {
            return hipErrorInvalidValue;
        }
    }); }); }); }); }); }); }); }); }); });
    // clang-format on
}

// a's launch fields as the plan sets them
static SearchArgs planned_args(SearchArgs a, const SearchLaunch& l) {
    a.chunk = l.chunk;
    a.tiles_per_row = l.tiles_per_row;
    a.tail_col0 = l.tail_col0;
    a.tail_T = l.tail_T;
    return a;
}

static hipError_t launch_plan(const SearchLaunchPlan& p, const SearchArgs& a, const AgreeArgs* ag,
                              hipStream_t st) {
    if (!p.ok) return hipErrorInvalidValue;
    for (int i = 0; i < p.n; ++i) {
        const SearchLaunch& l = p.launch[i];
        const hipError_t e = l.v.family == SearchFamily::pk ? launch_pk_variant(l, planned_args(a, l), ag, st)
                                                            : launch_mx_variant(l, planned_args(a, l), ag, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_search_mx(SearchArgs a, const MxGeometry& g, int words, bool nodupes,
                            hipStream_t st) {
    return launch_plan(plan_search_mx(a, g, words, nodupes), a, nullptr, st);
}

hipError_t launch_search_mx_agree(SearchArgs a, const AgreeArgs& ag, const MxGeometry& g, int words,
                                  hipStream_t st) {
    return launch_plan(plan_search_mx(a, g, words, true, &ag), a, &ag, st);
}

}  // namespace bicos_hip
