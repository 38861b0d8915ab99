// TEST PROGRAM: the main launch the plan (libbicos_amd/csrc/search_plan.cpp, linked alone: no
// kernel, no GPU) gives the 128-bit NoDuplicates search for a geometry as a tuned engine makes
// it (engine.cpp mx_geometry: tiles per wave, waves, LDS stage bytes, variant 64), one line per
// argument "rows,cols,T,waves,lds_kib,bits":
//   rows cols T waves lds_kib bits: ok stream prune packed chunk block lds
// "sweep" instead prints how many geometries of a grid plan the packed search streamed, and
// how many of those with another chunk than PKP_ST_CHUNK or another workgroup than half of it
// (tests/test_pkp_block_loop.py).
#include "search_plan.hpp"

#include <cstdio>
#include <cstring>

using namespace bicos_hip;

static SearchLaunchPlan plan(int rows, int cols, int T, int waves, int lds_kib, int bits) {
    SearchArgs a{};
    a.rows = rows;
    a.cols = cols;
    const MxGeometry g = search_mx_geometry(rows, cols, 4, lds_kib * 1024, T, waves, 256, 0, bits);
    return plan_search_mx(a, g, 4, true);
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        int streamed = 0, other = 0, packed = 0;
        for (int rows : {128, 256, 512, 1024, 2048})
            for (int cols = 256; cols <= 4096; cols += 124)
                for (int T : {0, 2, 4})
                    for (int waves : {0, 2, 4, 8})
                        for (int kib : {16, 32, 48, 64}) {
                            const SearchLaunchPlan p = plan(rows, cols, T, waves, kib, 125);
                            if (!p.ok || !p.launch[0].v.packed) continue;
                            ++packed;
                            if (!p.launch[0].v.stream) continue;
                            ++streamed;
                            other += p.launch[0].chunk != PKP_ST_CHUNK || 2 * p.launch[0].block != PKP_ST_CHUNK;
                        }
        std::printf("packed %d streamed %d other %d\n", packed, streamed, other);
        return 0;
    }
    for (int i = 1; i < argc; ++i) {
        int rows, cols, T, waves, kib, bits;
        if (std::sscanf(argv[i], "%d,%d,%d,%d,%d,%d", &rows, &cols, &T, &waves, &kib, &bits) != 6) return 2;
        const SearchLaunchPlan p = plan(rows, cols, T, waves, kib, bits);
        const SearchLaunch& l = p.launch[0];
        std::printf("%d %d %d %d %d %d: %d %d %d %d %d %d %ld\n", rows, cols, T, waves, kib, bits, (int)p.ok,
                    (int)l.v.stream, (int)l.v.prune, (int)l.v.packed, l.chunk, l.block, (long)l.lds);
    }
    return 0;
}
