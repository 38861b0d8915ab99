// median.hpp -- launcher of median.hip: the 3x3 / 5x5 median filter of a dense disparity map
// that knows the map's invalid values and can fill small holes (include/bicos_c.h, "median
// filter").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicos_hip {

// One workgroup stages a MEDIAN_TILE_ROWS x MEDIAN_TILE_COLS output tile plus its halo in LDS
// as 32-bit keys; a wave owns a tile row at a time (the tile is one wave wide). 512 threads:
// the workgroups are capped (below), so the waves per SIMD come from the workgroup's size
// (DESIGN.md 5.8).
constexpr int MEDIAN_TILE_ROWS = 32;
constexpr int MEDIAN_TILE_COLS = 64;
constexpr int MEDIAN_THREADS = 512;
// At most this many workgroups stride over the tiles: the counts are four addresses, and adds
// to one address are served one after another.
constexpr int MEDIAN_MAX_BLOCKS = 1024;

struct MedianArgs {
    const void* disp;  // int16 or float32, dense rows x cols
    void* out;         // same type and shape; does not overlap disp
    int rows, cols;    // rows * cols > 0
    int fill_min;      // 0 .. ksize * ksize
    int flags;         // BICOS_MEDIAN_*
    uint32_t* counts;  // device uint32[4] {unchanged, changed, filled, invalid} or nullptr
};

// One launch on `st`, after a hipMemsetAsync of counts where they are asked for. ksize is 3 or 5.
hipError_t launch_median(const MedianArgs& a, bool f32, int ksize, hipStream_t st);

}  // namespace bicos_hip
