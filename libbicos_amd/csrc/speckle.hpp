// speckle.hpp -- launchers of speckle.hip: the speckle filter of a dense disparity map
// (include/bicos_c.h, "speckle filter"): connected components of similar disparity under
// 4-connectivity, every component of at most max_size pixels removed.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicos_hip {

// One workgroup labels a SPECKLE_TILE_ROWS x SPECKLE_TILE_COLS tile in LDS: a wave per row
// (the tile is one wave wide, so a row's runs come from one ballot), SPECKLE_THREADS / 64 rows
// at a time.
constexpr int SPECKLE_TILE_ROWS = 32;
constexpr int SPECKLE_TILE_COLS = 64;
constexpr int SPECKLE_THREADS = 256;
// the border, resolve and apply launches: a lane per item, SPECKLE_PER_LANE items a block apart
constexpr int SPECKLE_PER_LANE = 4;

struct SpeckleArgs {
    const void* disp;  // int16 or float32, dense rows x cols
    void* out;         // same type and shape; may be disp itself
    int rows, cols;    // rows * cols > 0
    uint32_t max_size;
    float max_diff;  // >= 0, may be +inf
    int flags;       // BICOS_SPECKLE_*
    int32_t* labels;  // [rows*cols]: the caller's optional output or workspace
    uint32_t* sizes;  // [rows*cols] workspace
    uint32_t* counts;  // device uint32[4] {kept, removed, invalid, removed_components} or nullptr
    bool final_labels;  // labels is the caller's: apply writes every valid pixel's root
};

// tile, border (where the map has more than one tile), resolve, apply -- on `st`, after a
// hipMemsetAsync of counts where they are asked for.
hipError_t launch_speckle(const SpeckleArgs& a, bool f32, hipStream_t st);

}  // namespace bicos_hip
