// search_plan.cpp -- the host side of the matrix-core searches: the geometry of a shape and
// the launch plan, i.e. which kernel instantiations run it, with which grid, LDS and
// arguments. Host only: no kernel, no HIP call; the kernel files launch what is planned here.
#include "search_plan.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace bicos_hip {

namespace {

// The one-product search's key scheme for a shape (search_mx.hip KEYS): one-product XK keys by
// default -- with NoDuplicates in any block order up to 8160 columns (2), ascending up to
// 16384 (1), float keys with the column in the free K half where the geometry allows them (3)
// -- and the two-product float keys (0) beyond that, or when tuned (variant 66)
int mx_keys(const MxGeometry& g, bool nodupes, int cols) {
    if (g.keys != 1) return 0;
    if (!nodupes && g.fk) return 3;
    if (nodupes && cols <= XKF_MAX_COLS) return 2;
    return cols <= XK_MAX_COLS ? 1 : 0;
}

// Whether a main launch takes the streamed kernel (search_mx_kernel ST): asked for
// (MxGeometry.stream), more than one chunk per row, and a stage of half a chunk = one col1
// per thread (1024-column chunks under 8 waves: cfg2, cfg5, readme and their row bands)
bool mx_streamable(int cols, int chunk, int waves, bool stream) {
    return stream && cols > chunk && chunk == 2 * 64 * waves;
}

// Whether a pruned main launch runs on packed keys (search_pk.hip search_pkp_kernel): asked
// for (MxGeometry.packed: 128-bit descriptors whose used bits the caller states, <=
// PK_MAX_BITS), 4 tiles = 2 wide tiles per wave, and the raw right row fits the LDS stage
// behind the workgroup's results for the lazy rescans (8 waves: 3968 columns). The geometry
// is the one-product kernel's: the same workgroups, threads, chunk and LDS bytes.
bool packed_search(const MxGeometry& g, const SearchVariant& v, int cols) {
    if (!g.packed || !v.prune || v.T != 4 || v.words != 4 || v.keys != 2 || v.list) return false;
    const long row_off = (64L * g.waves * v.T + 15) & ~15L;  // the results: int16 per col0
    return (long)g.chunk * v.words * 16 >= row_off + (long)cols * v.words * 4;
}

int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

const FusedAgreeShape* fused_agree_shape(int words, int n, SearchFamily family, int tiles) {
    for (const FusedAgreeShape& s : FUSED_AGREE_SHAPES)
        if (s.words == words && s.n == n && s.family == family &&
            (s.tiles[0] == tiles || s.tiles[1] == tiles))
            return &s;
    return nullptr;
}

SearchLaunchPlan invalid() {
    SearchLaunchPlan p;
    p.ok = false;
    return p;
}

// One launch of `v` with `waves` waves: col_tile col0 per tile (mx 32, pk 64), word_slots
// 16-byte LDS slots per col1; compacted launches add the prologue scratch and the entries.
SearchLaunch make_launch(const SearchVariant& v, int rows, int waves, int col_tile, int word_slots,
                         int chunk, int tiles_per_row, int tail_col0, int tail_T) {
    SearchLaunch l;
    l.v = v;
    l.grid = v.list ? list_grid(rows, tiles_per_row) : rows * tiles_per_row;
    l.block = 64 * waves;
    l.lds = (size_t)word_slots * chunk * 16;
    if (v.list) l.lds = list_ent_offset((int)l.lds) + (size_t)waves * v.T * col_tile * 2;
    l.chunk = chunk;
    l.tiles_per_row = tiles_per_row;
    l.tail_col0 = tail_col0;
    l.tail_T = tail_T;
    return l;
}

// The tail launch after `main`: one workgroup per row of tail_tiles tiles per wave over
// [tail_col0, cols), shaped by BICOS_TAIL_CHUNK (search_plan.hpp). A tail workgroup scans the
// whole row like the others but with fewer tiles, so the remainder no longer costs a full
// T-tile scan: 3208 columns are 3 x 1024 + 136, and the 4th workgroup of every row ran 2 of
// its 8 waves for a full-length scan. (One heterogeneous launch would also fill the main
// launch's last round, but hosting both tile counts in one kernel made the main path spill.)
// Compacted col0 split the same way in entry space: the main workgroups take the row's entries
// below tail_col0, the tail workgroup the entries from tail_col0 on, if the row has any.
SearchLaunch tail_launch(const SearchLaunch& main, int rows, int cols, int tail_tiles, int col_tile,
                         int word_slots) {
    SearchVariant v = main.v;
    v.T = tail_tiles;
    v.tail = true;
    v.agree = v.stream = v.prune = v.packed = false;
    int waves = main.block / 64, chunk = main.chunk;
    if (BICOS_TAIL_CHUNK > 0) {
        const int per_wave = col_tile * tail_tiles, rem = cols - main.tail_col0;
        waves = std::max(1, std::min(waves, (rem + per_wave - 1) / per_wave));
        chunk = std::min(chunk, (int)BICOS_TAIL_CHUNK);
    }
    return make_launch(v, rows, waves, col_tile, word_slots, chunk, 1, main.tail_col0, main.tail_T);
}

// packed keys (search_pk.hip): main launch over [0, pk_tail_col0), then the tail of one wide
// tile per wave when the geometry asked for one
SearchLaunchPlan plan_pk(const SearchArgs& a, const MxGeometry& g, int words, bool agree) {
    if (a.cols > PK_MAX_COLS || g.pk_chunk < 32 || (g.pk_chunk & 31)) return invalid();
    const int T = g.pk_T;
    // (4 wide tiles only for 32/64-bit descriptors: the B fragments of more do not fit)
    if ((words != 1 && words != 2 && words != 4) || !(T == 1 || T == 2 || (T == 4 && words <= 2)))
        return invalid();
    SearchVariant v;
    v.family = SearchFamily::pk;
    v.words = words;
    v.nodupes = true;
    v.T = T;
    v.list = a.keep != nullptr;
    v.agree = agree;
    v.lazy = a.cols >= PK_LAZY_MIN_COLS;
    SearchLaunchPlan p;
    p.launch[p.n++] = make_launch(v, a.rows, g.waves, 64, words, g.pk_chunk, g.pk_tiles_per_row,
                                  agree ? a.cols : g.pk_tail_col0, 0);
    if (T > 1 && g.pk_tail_col0 < a.cols) p.launch[p.n++] = tail_launch(p.launch[0], a.rows, a.cols, 1, 64, words);
    return p;
}

// one-product keys (search_mx.hip): rows x tiles_per_row workgroups of T tiles per wave over
// [0, tail_col0); then, when the row's last workgroup would hold only a few col0 (tail_col0 <
// cols), one workgroup per row with fewer tiles per wave over [tail_col0, cols)
SearchLaunchPlan plan_mx(const SearchArgs& a, const MxGeometry& g, int words, bool nodupes, bool agree) {
    SearchVariant v;
    v.family = SearchFamily::mx;
    v.words = words;
    switch (words) {
        case 1: case 2: v.ksteps = 1; break;
        case 4: v.ksteps = 2; break;
        case 8: v.ksteps = g.ksteps == 3 ? 3 : 4; break;
        default: return invalid();
    }
    v.nodupes = nodupes;
    v.keys = mx_keys(g, nodupes, a.cols);
    v.list = a.keep != nullptr;
    v.agree = agree;
    int tiles_per_row = g.tiles_per_row, tail_T = g.tail_T, tail_col0 = g.tail_col0;
    v.T = g.T;
    if (v.T != 2 && v.T != 4 && v.T != 8) return invalid();
    if (v.T == 8 && !mx_tiles_fit(words, nodupes, v.keys, 8)) {
        v.T = 4;     // does not fit: 4 tiles per wave, twice the workgroups per row
        tail_T = 0;  // (the tail was sized for 8 tiles)
    }
    // tail tiles: 1 or 2, and fewer than the main workgroups'; KEYS 2 only -- the any-order
    // NoDuplicates search, whose block order starts at each wave's own col0
    const bool tail = !agree && v.keys == 2 && tail_col0 < a.cols &&
                      ((tail_T == 1 && v.T >= 2) || (tail_T == 2 && v.T >= 4));
    if (!tail) {  // the main workgroups cover every col0
        tiles_per_row = ceil_div(a.cols, 32L * g.waves * v.T);
        tail_T = 0;
        tail_col0 = a.cols;
    }
    // the 128-bit any-order NoDuplicates search over every col0: streamed and / or pruned
    if (!v.list && words == 4 && v.ksteps == 2 && v.keys == 2 && (v.T == 2 || v.T == 4)) {
        v.stream = mx_streamable(a.cols, g.chunk, g.waves, g.stream != 0);
        v.prune = g.prune != 0;
        v.packed = packed_search(g, v, a.cols);
        // (the packed kernel streams at one chunk only; at any other it runs its chunk loop)
        if (v.packed && (g.chunk != PKP_ST_CHUNK || 128 * g.waves != PKP_ST_CHUNK)) v.stream = false;
    }
    SearchLaunchPlan p;
    p.launch[p.n++] = make_launch(v, a.rows, g.waves, 32, 2 * v.ksteps, g.chunk, tiles_per_row, tail_col0, tail_T);
    if (tail) p.launch[p.n++] = tail_launch(p.launch[0], a.rows, a.cols, tail_T, 32, 2 * v.ksteps);
    return p;
}

// tiles per wave of the one-pass Consistency search (BICOS_LR_T=2: two, A/B)
int lr_tiles() {
    const char* v = std::getenv("BICOS_LR_T");
    return v && std::atoi(v) == 2 ? 2 : 4;
}

}  // namespace

MxGeometry search_mx_geometry(int rows, int cols, int words, int lds_bytes, int T, int waves,
                              int cus, int keys, int bits) {
    MxGeometry g;
    g.stream = 1;
    g.prune = 1;
    g.packed = words == 4 && bits > 0 && bits <= PK_MAX_BITS;
    g.keys = keys == 2 ? 2 : 1;
    // 64-bit K-steps the products need: all of the descriptor unless the caller knows that
    // the bits past `bits` are zero (transform output); only 256-bit descriptors have a
    // step to drop (129..192 used bits)
    g.ksteps = words >= 2 ? words / 2 : 1;
    if (words == 8 && bits > 0 && bits <= 192) g.ksteps = 3;
    // keys 3 (engine tuned to variant 67): XK keys for the first-minimum searches too (A/B)
    g.fk = keys != 3 && g.keys == 1 && bits > 0 && bits <= 64 * g.ksteps - 32 && cols <= FK_MAX_COLS;
    const int wl = 2 * g.ksteps;
    // LDS chunk of expanded right descriptors (16 B per word per col1), multiple of 32
    int chunk = lds_bytes / (wl * 16);
    chunk &= ~31;
    if (chunk < 32) chunk = 32;
    const int cols32 = (cols + 31) & ~31;
    g.chunk = cols32 < chunk ? cols32 : chunk;
    g.waves = waves ? waves : 8;
    if (T) {
        g.T = T;
    } else {
        // 4 tiles per wave (2 for 4-step 256-bit descriptors, whose 4-tile B fragments
        // spill: cfg4 1.47 -> 1.09 ms, cfg4f 1.53 -> 0.64 ms; at 3 steps 4 tiles win: cfg4
        // 0.92 -> 0.82 ms; 8 spill for most widths), 2 when the grid would not give every
        // CU about two workgroups (narrow row bands)
        g.T = 2;
        for (int t = g.ksteps >= 4 ? 2 : 4; t >= 2; t /= 2) {
            const long per_wg = 32L * g.waves * t;
            const long nwg = (long)rows * ((cols + per_wg - 1) / per_wg);
            if (nwg >= 2L * (cus > 0 ? cus : 256)) {
                g.T = t;
                break;
            }
        }
    }
    const long per_wg = 32L * g.waves * g.T;
    g.tiles_per_row = (int)((cols + per_wg - 1) / per_wg);
    // a short remainder of the row (<= 8 waves x 2 tiles, and at most half of a workgroup)
    // goes to one tail workgroup per row with 1 or 2 tiles per wave (tail_launch), for
    // 4-tile main workgroups: 3208 columns readme 1.127 vs 1.254 ms, FULL n = 12 1.127 vs
    // 1.255; behind 2-tile ones (4-K-step 256-bit, FULL n = 16) it measured slower, 2.15 vs
    // 2.08 ms (profiles/search_tail_r04.jsonl)
    g.tail_T = 0;
    g.tail_col0 = cols;
    const long rem = cols % per_wg;
    if (g.T >= 4 && rem > 0 && cols > per_wg && 2 * rem <= per_wg) {
        const int tt = rem <= 32L * g.waves ? 1 : 2;
        if (tt < g.T && rem <= 32L * g.waves * tt) {
            g.tail_T = tt;
            g.tiles_per_row = (int)(cols / per_wg);
            g.tail_col0 = (int)(cols - rem);
        }
    }
    // packed keys: the default NoDuplicates search for 32/64-bit descriptors (one K-step,
    // where the key reduction, not the matrix products, bounds the one-product search: FULL
    // n = 6 0.63 vs 1.43 ms, n = 8 0.78 vs 0.97 ms at 3208x2200, profiles/search_integ_r04.jsonl),
    // or wherever variant 68 (or BICOS_PK128=1, for 128-bit descriptors with <= 127 used bits)
    // asks for it. With lazy drops (round 6) the 128-bit packed search is faster back to back
    // (cfg2 0.334 vs 0.349 ms, random descriptors 0.382 vs 0.481; profiles/pk128_r06.jsonl), but
    // in the bench's frames it only ties or loses where it matters: cfg2 7889 / 7847 vs 7858 /
    // 7913 Mpix/s, readme -1.2 %, cfg2's 192-row bands of the 8-GPU run -11 % (one wide tile per
    // wave), cfg5 +2.4 % -- so the one-product search stays the 128-bit default.
    // Same workgroup shape, a wide tile = two 32-col0 tiles; the LDS stage holds one expanded
    // word per descriptor word
    // (32/64-bit words need no used-bits hint: a distance is at most 64 <= PK_MAX_BITS)
    static const bool pk128 = [] {
        const char* v = std::getenv("BICOS_PK128");
        return v && !std::strcmp(v, "1");
    }();
    g.pk = (keys == 4 || (keys == 0 && (words <= 2 || (words == 4 && pk128)))) &&
           (words <= 2 || (bits > 0 && bits <= PK_MAX_BITS)) && bits <= 32 * words &&
           (words == 1 || words == 2 || words == 4) && cols <= PK_MAX_COLS;
    g.pk_T = g.T >= 2 ? g.T / 2 : 1;
    if (words == 4 && g.pk_T > 2) g.pk_T = 2;  // (4 wide tiles' B fragments do not fit)
    int pchunk = (lds_bytes / (words * 16)) & ~31;
    if (pchunk < 32) pchunk = 32;
    g.pk_chunk = cols32 < pchunk ? cols32 : pchunk;
    const long pk_wg = 64L * g.waves * g.pk_T;
    g.pk_tiles_per_row = (int)((cols + pk_wg - 1) / pk_wg);
    // the packed search's tail: one workgroup per row of one wide tile per wave (FULL n = 6 at
    // 3208 columns: 0.575 vs 0.66 ms, profiles/search_tail_r04.jsonl)
    g.pk_tail_col0 = cols;
    const long pk_rem = cols % pk_wg;
    if (g.pk_T > 1 && pk_rem > 0 && cols > pk_wg && 2 * pk_rem <= pk_wg &&
        pk_rem <= 64L * g.waves) {
        g.pk_tiles_per_row = (int)(cols / pk_wg);
        g.pk_tail_col0 = (int)(cols - pk_rem);
    }
    return g;
}

bool search_mx_agree_fusable(const MxGeometry& g, int words, bool nodupes, int cols, int n,
                             int depth, bool dbl) {
    if (!nodupes || depth != 1 || dbl) return false;
    if (!fused_agree_shape(words, n, g.pk ? SearchFamily::pk : SearchFamily::mx, g.pk ? g.pk_T : g.T))
        return false;
    // no tail; the raw results in the LDS stage (16 B per col1 and word): packed keys 64
    // int16 per wave and wide tile, one-product keys 32 per wave and tile
    if (g.pk)
        return g.pk_tail_col0 == cols && cols <= PK_MAX_COLS &&
               (long)g.pk_chunk * words * 16 >= 128L * g.waves * g.pk_T;
    return g.ksteps == 2 && mx_keys(g, true, cols) == 2 && g.tail_T == 0 &&
           g.chunk * 4 * 16 >= 2 * 32 * g.T * g.waves;
}

SearchLaunchPlan plan_search_mx(const SearchArgs& a, const MxGeometry& g, int words, bool nodupes,
                                const AgreeArgs* ag) {
    if (a.rows <= 0 || a.cols <= 0) return SearchLaunchPlan{};
    if (a.cols > 32767 || g.waves < 1 || g.waves > 8) return invalid();
    if (ag) {  // one launch over every col0 of a shape of FUSED_AGREE_SHAPES
        if (a.keep || a.out_mode != 0 || !search_mx_agree_fusable(g, words, true, a.cols, ag->n, 1, false))
            return invalid();
        if (g.pk) return plan_pk(a, g, words, true);
    }
    if (g.chunk < 32 || (g.chunk & 31)) return invalid();
    if (!ag && g.pk && nodupes) return plan_pk(a, g, words, false);
    return plan_mx(a, g, words, ag ? true : nodupes, ag != nullptr);
}

bool search_mx_packed(const MxGeometry& g, int rows, int cols, int words, int n) {
    SearchArgs a{};
    a.rows = rows;
    a.cols = cols;
    AgreeArgs ag{};
    ag.n = n;
    if (n && !search_mx_agree_fusable(g, words, true, cols, n, 1, false)) return false;
    const SearchLaunchPlan p = plan_search_mx(a, g, words, true, n ? &ag : nullptr);
    return p.ok && p.n > 0 && p.launch[0].v.packed;
}

bool search_lr_eligible(int words, int bits, int cols) {
    return words == 8 && bits > 128 && bits <= LR_KSTEPS * 64 - LR_FREE_BITS && cols >= 1 &&
           cols <= LR_MAX_COLS;
}

SearchLaunchPlan plan_search_lr(const SearchArgs& a, int words, int bits) {
    if (a.rows <= 0 || a.cols <= 0) return SearchLaunchPlan{};
    if (!search_lr_eligible(words, bits, a.cols) || a.keep || a.out_mode != 0) return invalid();
    constexpr int WL = 2 * LR_KSTEPS;
    // 8 waves of T x 32 col0 per pass (fewer for narrow rows); the LDS stage as the KEYS 3
    // search's (64 KiB) plus the row's reverse keys and forward results
    SearchLaunch l;
    l.v.family = SearchFamily::lr;
    l.v.words = words;
    l.v.ksteps = LR_KSTEPS;
    l.v.T = lr_tiles();
    const int waves = std::min(8, (a.cols + 32 * l.v.T - 1) / (32 * l.v.T));
    const int cols32 = (a.cols + 31) & ~31;
    // two workgroups per CU: <= 80 KiB each for the stage, the row's keys and results and (4
    // tiles) the B fragments of the last K-step; cfg4: 384-column chunks
    const size_t fixed = (size_t)cols32 * 6 + (l.v.T == 4 ? (size_t)waves * l.v.T * 64 * 16 : 0);
    l.chunk = std::min((int)((80 * 1024 - fixed) / (WL * 16)) & ~31, cols32);
    if (l.chunk < 32) return invalid();
    l.grid = a.rows;
    l.block = 64 * waves;
    l.lds = (size_t)WL * l.chunk * 16 + fixed;
    SearchLaunchPlan p;
    p.launch[p.n++] = l;
    return p;
}

}  // namespace bicos_hip
