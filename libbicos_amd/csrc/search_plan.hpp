// search_plan.hpp -- which kernel for which shape: the launch plan of the matrix-core searches
// (search_plan.cpp, host only) and the limits it shares with the kernels (search_mx.hip,
// search_pk.hip, search_lr.hip). The plan is the one place that decides; a kernel file only
// maps a planned variant to its instantiation.
#pragma once

#include "kernels.hpp"

#include <stddef.h>

namespace bicos_hip {

// ---- limits of the key schemes (derived where the kernels define the keys)
constexpr int XK_MAX_COLS = 16384;   // search_mx.hip KEYS 1: 14 column bits
constexpr int XKF_MAX_COLS = 8160;   // KEYS 2
constexpr int FK_MAX_COLS = 2048;    // KEYS 3 (see FK_EPS)
constexpr int PK_MAX_BITS = 127;     // search_pk.hip: a distance in 7 bits
constexpr int PK_MAX_COLS = 32767;
constexpr int LR_MAX_COLS = FK_MAX_COLS;  // search_lr.hip
constexpr int LR_FREE_BITS = 38;     // 32 upper-half + 6 lower-half K elements
constexpr int LR_KSTEPS = 3;
// The pruned 128-bit searches' fallback (search_mx.hip PRUNE, search_pk.hip search_pkp_kernel): visited
// blocks per window
constexpr int PRUNE_WINDOW = 8;
// The one chunk search_pkp_kernel's streamed instantiations are built for (search_pk.hip: words
// 1-3 of a block at immediate offsets from its word-0 fragment): the default geometry's, 8
// waves over a 64 KiB stage. mx_streamable alone allows any chunk of two columns per thread
// (a tuned engine: 512 with 4 waves over 32 KiB); plan_mx gives the packed search of such a
// geometry the chunk loop, and launch_pk_variant refuses what it did not plan.
constexpr int PKP_ST_CHUNK = 1024;
// Which 32 descriptor bits each of search_pkp_kernel's four products holds (search_pk.hip
// pkp_mix, block_pr). expand_bits puts the bits p of a word with (p mod 8) div 2 == m into dword
// m of its expansion; dword m of product k's operands is dword m of the expansion of word
// pkp_dword_word(k, m): products 0 and 1 take words 0 and 1 by alternate dwords (16 bits of
// each), products 2 and 3 are words 2 and 3. The one-word probe, product 0, so holds bits of
// twice as many image steps as a descriptor word does. pkp_bit_product: the product that
// descriptor bit 0-127 is multiplied in (bicos_search_packed_product, bicos_c.h).
constexpr int pkp_dword_word(int k, int m) { return k < 2 ? k ^ (m & 1) : k; }
constexpr int pkp_bit_product(int bit) {
    const int w = bit >> 5, m = (bit & 7) >> 1;
    for (int k = 0; k < 4; ++k)
        if (pkp_dword_word(k, m) == w) return k;
    return -1;
}

// Lazy drops of the packed-key search (search_pk.hip lazy_drop). They pay a fixed rescan per
// col0 (~32 popcounts of WORDS words); the drop branch pays per drop. Narrow rows (few blocks,
// few drops on stereo input) keep the branch: cfg1 (640 columns) 13391 vs 12478-12791 Mpix/s;
// 3208-3300-column rows take the lazy form: random 32-bit NoDuplicates 0.66 vs 1.12-1.14 ms,
// FULL n = 6 +5 % (FULL n = 8 -1.7 %); profiles/pk_lazy_r06.jsonl
constexpr int PK_LAZY_MIN_COLS = 1024;

// The tail launch's shape: one workgroup per row with only the waves its columns need and a
// small LDS chunk, so several tail workgroups stay resident per CU (the main launch's 64 KiB
// chunks allow two) -- the tail rows then run in < 2 rounds of workgroups instead of 4
// (BICOS_TAIL_CHUNK = 0 keeps the main launch's shape; 512 vs 256 vs 0:
// profiles/search_tail_shape_r04.jsonl).
#ifndef BICOS_TAIL_CHUNK
#define BICOS_TAIL_CHUNK 512
#endif

// ---- compacted (LIST) launches: grid and LDS layout
// (row, tile) of a compacted launch: grid = 8 x ceil(R8 / G) G x tiles_per_row, R8 =
// ceil(rows / 8), G = LIST_GROUP rows (search_dev.hpp list_row_tile has the order's reasons)
constexpr int LIST_GROUP = 32;
constexpr int list_grid(int rows, int tiles_per_row) {
    return 8 * (((rows + 7) / 8 + LIST_GROUP - 1) / LIST_GROUP) * LIST_GROUP * tiles_per_row;
}
// LIST prologue scratch at the start of the dynamic LDS (before the first chunk is staged):
// the row's kept-column bitmap (<= 1024 words: cols <= 32767) and 8 wave sums; the
// workgroup's entry columns live after the chunk region
constexpr int LIST_SCRATCH_BYTES = (1024 + 8) * 4;
static_assert(LIST_SCRATCH_BYTES % 16 == 0, "scratch size");
// byte offset of the LIST entry columns in the dynamic LDS: past the chunk region and the
// prologue scratch
constexpr int list_ent_offset(int chunk_bytes) {
    return chunk_bytes > LIST_SCRATCH_BYTES ? (chunk_bytes + 15) / 16 * 16 : LIST_SCRATCH_BYTES;
}

// ---- the plan
enum class SearchFamily { mx, pk, lr };  // search_mx_kernel, search_pk_kernel, search_lr_kernel

// A kernel instantiation by its named fields (the families read the ones they have).
struct SearchVariant {
    SearchFamily family = SearchFamily::mx;
    int words = 0;         // 32-bit words per descriptor
    int ksteps = 0;        // mx, lr: 64-bit K-steps multiplied
    bool nodupes = false;  // mx (pk: always)
    int T = 0;             // tiles per wave (mx, lr: 32 col0; pk: 64 col0)
    int keys = 0;          // mx: key scheme 0..3 (search_mx.hip)
    bool tail = false;     // the col0 from tail_col0 on, one workgroup per row
    bool list = false;     // compacted col0 (SearchArgs.keep)
    bool agree = false;    // the fused agree epilogue
    bool stream = false;   // mx: the right row streamed in half-chunk stages (ST)
    bool prune = false;    // mx: the second K-step only where it can matter (PRUNE)
    bool lazy = false;     // pk: lazy drops
    // mx, pruned main launches of 4 tiles per wave: run by search_pkp_kernel on packed
    // keys in the same geometry (launch_mx_variant forwards it); the plan's packed_search
    bool packed = false;
};

struct SearchLaunch {
    SearchVariant v;
    int grid = 0, block = 0;  // workgroups, threads per workgroup
    size_t lds = 0;           // dynamic LDS bytes
    // patched into the launch's SearchArgs
    int chunk = 0, tiles_per_row = 0, tail_col0 = 0, tail_T = 0;
};

struct SearchLaunchPlan {
    bool ok = true;  // false: no kernel for this request (hipErrorInvalidValue), nothing launches
    int n = 0;       // launches, in order: the main one, then the tail's
    SearchLaunch launch[2];
};

// Tile counts of the one-product search whose registers fit (checked with
// -Rpass-analysis=kernel-resource-usage): 8 tiles only for 32/64-bit descriptors with one key
// product. The plan falls back to 4 tiles; search_mx.hip builds only what fits.
constexpr bool mx_tiles_fit(int words, bool nodupes, int keys, int t) {
    return t <= 4 || (words == 1 && (keys != 0 || !nodupes)) || (words == 2 && !nodupes);
}

// Shapes whose agree stage runs inside the search launch: search_mx_agree_fusable and the
// plan of a fused launch both read this table.
struct FusedAgreeShape {
    int words, n;         // descriptor words, stack depth (u8, float NXC)
    SearchFamily family;
    int tiles[2];         // tiles per wave (mx: T, pk: wide tiles)
};
constexpr FusedAgreeShape FUSED_AGREE_SHAPES[] = {
    {1, 8, SearchFamily::pk, {1, 1}},   // cfg1
    {4, 33, SearchFamily::pk, {1, 2}},  // cfg2 / cfg5 under BICOS_PK128 or variant 68
    {4, 33, SearchFamily::mx, {2, 4}},  // cfg2, cfg5, readme; 2 tiles: their narrow row bands
};
constexpr int FUSED_AGREE_N = 33;    // search_mx_kernel AG: 128-bit descriptors (cfg2, cfg5)
constexpr int FUSED_AGREE_N_PK = 8;  // search_pk_kernel AG: 32-bit descriptors (cfg1)

// The launches of launch_search_mx (ag == nullptr) or launch_search_mx_agree (ag: the fused
// agree's arguments) for `a` under geometry g. Pure: no HIP call, reads only its arguments.
SearchLaunchPlan plan_search_mx(const SearchArgs& a, const MxGeometry& g, int words, bool nodupes,
                                const AgreeArgs* ag = nullptr);
// The launch of launch_search_lr (BICOS_LR_T=2, read per call: two tiles per wave, A/B).
SearchLaunchPlan plan_search_lr(const SearchArgs& a, int words, int bits);

// the families' launchers: a planned variant to its instantiation; one that is not built
// returns hipErrorInvalidValue (`a`: the plan's chunk / tiles_per_row / tail fields set)
hipError_t launch_mx_variant(const SearchLaunch& l, const SearchArgs& a, const AgreeArgs* ag,
                             hipStream_t st);
hipError_t launch_pk_variant(const SearchLaunch& l, const SearchArgs& a, const AgreeArgs* ag,
                             hipStream_t st);

}  // namespace bicos_hip
