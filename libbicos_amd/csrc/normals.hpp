// normals.hpp -- launchers of normals.hip: unit surface normals from a dense disparity map and
// the rig's 4x4 Q matrix, by a least-squares plane in (column, row, disparity) over a small
// window (include/bicos_c.h, "surface normals").
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace bicos_hip {

// Dense map: one workgroup stages a NORMALS_TILE_ROWS x NORMALS_TILE_COLS tile plus its radius
// halo in LDS as float32 (NaN = invalid or outside the image); a wave owns a tile row at a
// time (the tile is one wave wide), a lane a pixel.
constexpr int NORMALS_TILE_ROWS = 32;
constexpr int NORMALS_TILE_COLS = 64;
constexpr int NORMALS_THREADS = 512;
// At most this many workgroups stride over the tiles: the counts are four addresses, and adds
// to one address are served one after another (median.hpp).
constexpr int NORMALS_MAX_BLOCKS = 1024;
// List form: a lane per entry, the lanes striding over the list.
constexpr int NORMALS_LIST_THREADS = 256;
constexpr int NORMALS_LIST_MAX_BLOCKS = 1 << 16;
constexpr int NORMALS_MAX_RADIUS = 4;

struct NormalsQ {
    double q[16];  // row-major
};

struct NormalsArgs {
    const void* disp;  // int16 or float32, dense rows x cols (not read where rows * cols == 0)
    int rows, cols;
    int flags;  // BICOS_NORMALS_*
    int radius;  // 1 .. NORMALS_MAX_RADIUS
    float max_diff;
    int min_points;
    NormalsQ Q;
    float* normal_map;     // [rows][cols][3] or nullptr
    uint32_t* counts;      // device uint32[4] {normal, no_point, sparse, degenerate} or nullptr
    const int32_t* index;  // [count] or nullptr
    float* normals;        // [count][3] or nullptr
    size_t count;
};

// The dense map: one launch on `st`, after a hipMemsetAsync of counts where they are asked for.
// rows * cols > 0.
hipError_t launch_normals_map(const NormalsArgs& a, bool f32, hipStream_t st);
// The list: one launch on `st`. count > 0; rows * cols may be 0 (every entry is then outside).
hipError_t launch_normals_list(const NormalsArgs& a, bool f32, hipStream_t st);

}  // namespace bicos_hip
