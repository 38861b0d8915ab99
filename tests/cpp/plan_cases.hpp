// plan_cases.hpp -- the table of shapes behind tests/golden/search_plan.json and the line
// format of a planned launch (plan_dump.cpp; tests/test_search_plan.py). The table straddles
// every threshold the launch plan tests: descriptor widths, used bits around the packed-key /
// K-step / float-key / one-pass limits, columns around the chunk, key-scheme and tile limits,
// rows around the two-workgroups-per-CU rule.
#pragma once

#include <cstdio>

namespace plan_cases {

struct Case {
    char kind;  // 'S' launch_search_mx, 'A' launch_search_mx_agree, 'L' launch_search_lr
    int words, bits, cols, rows;
    int nodupes, keep, row_valid;
    int keys, T, waves, stream, prune;
    int n;  // 'A': the agree's stack depth
};

inline void print_case(const Case& c) {
    std::printf("%c %d %d %d %d %d %d %d %d %d %d %d %d %d:", c.kind, c.words, c.bits, c.cols, c.rows,
                c.nodupes, c.keep, c.row_valid, c.keys, c.T, c.waves, c.stream, c.prune, c.n);
}

// one launch: family (mx | pk | lr), the variant by field, @grid x block + LDS bytes, and
// what the launch patches into SearchArgs (chunk/tiles_per_row/tail_col0/tail_T)
inline void print_launch(const char* family, int words, int ksteps, int nodupes, int T, int keys,
                         int tail, int list, int agree, int stream, int prune, int lazy, int grid,
                         int block, long lds, int chunk, int tiles_per_row, int tail_col0, int tail_T) {
    std::printf(" %s %d %d %d %d %d %d %d %d %d %d %d @%dx%d+%ld %d/%d/%d/%d;", family, words, ksteps,
                nodupes, T, keys, tail, list, agree, stream, prune, lazy, grid, block, lds, chunk,
                tiles_per_row, tail_col0, tail_T);
}

template <class F>
void for_each_case(F f) {
    const int W[] = {1, 2, 4, 8};
    const int BITS[] = {0, 64, 126, 127, 128, 154, 155, 192, 193, 254};
    const int COLS[] = {31,   32,   33,   640,  1023, 1024,  1025,  2048,  2049,
                        3208, 3300, 8160, 8161, 16384, 16385, 32767};
    // every width x used bits x columns, NoDuplicates on and off, the engine's defaults
    for (int w : W)
        for (int b : BITS)
            for (int c : COLS)
                for (int nd = 0; nd < 2; ++nd) f(Case{'S', w, b, c, 2200, nd, 0, 0, 0, 0, 0, 1, 1, 0});
    // one switch at a time (and the pairs that meet in one ladder) on a smaller grid
    const int BITS2[] = {0, 126, 154};
    const int COLS2[] = {640, 2049, 3208, 8161};
    for (int w : W)
        for (int b : BITS2)
            for (int c : COLS2)
                for (int nd = 0; nd < 2; ++nd) {
                    const Case d{'S', w, b, c, 2200, nd, 0, 0, 0, 0, 0, 1, 1, 0};
                    Case x;
                    for (int rows : {1, 192}) { x = d; x.rows = rows; f(x); }
                    for (int kr = 1; kr < 4; ++kr) {  // keep / row_valid, also on a narrow band
                        x = d; x.keep = kr & 1; x.row_valid = kr >> 1; f(x);
                        if (kr == 1) { x.rows = 192; f(x); }
                    }
                    for (int keys = 1; keys <= 4; ++keys) {
                        x = d; x.keys = keys; f(x);
                        x.keep = 1; f(x);
                    }
                    for (int T : {2, 4, 8}) {
                        x = d; x.T = T; f(x);
                        x.keep = 1; f(x);
                        x.keep = 0; x.waves = 4; f(x);
                    }
                    for (int waves : {4, 8}) { x = d; x.waves = waves; f(x); }
                    for (int sp = 0; sp < 3; ++sp) {
                        x = d; x.stream = sp & 1; x.prune = sp >> 1; f(x);
                        x.rows = 192; f(x);
                    }
                }
    // the fused agree: the shapes of its table, their neighbours, the packed 128-bit search
    for (int wn = 0; wn < 2; ++wn)
        for (int b : {0, 126, 127})
            for (int c : {640, 1025, 2048, 3208, 8160, 8161})
                for (int rows : {192, 2200})
                    for (int keys : {0, 4})
                        for (int T : {0, 2, 4})
                            for (int sp = 0; sp < 4; ++sp)
                                f(Case{'A', wn ? 4 : 1, b, c, rows, 1, 0, 0, keys, T, 0, sp & 1, sp >> 1,
                                       wn ? 33 : 8});
    // one-pass Consistency
    for (int b : {128, 129, 154, 155})
        for (int c : {31, 32, 33, 640, 1023, 1024, 1025, 2048, 2049})
            for (int rows : {1, 2200}) f(Case{'L', 8, b, c, rows, 0, 0, 0, 0, 0, 0, 0, 0, 0});
}

}  // namespace plan_cases
