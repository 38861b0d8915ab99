// rectify.hpp -- launchers of rectify.hip: the lookup maps of one camera from its calibration
// and the bilinear remap of a whole image stack through one pair of maps (include/bicos_c.h,
// "rectification"; the numpy restatement is tests/rectify_ref.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicos_hip {

// One workgroup remaps a RECTIFY_TILE_ROWS x RECTIFY_TILE_COLS tile of output pixels: a lane
// owns RECTIFY_PER_LANE consecutive pixels of one row (one dword of u8, two of u16), a wave two
// rows of the tile, so a wave's stores are two runs of 128 (u8) or 256 (u16) bytes.
constexpr int RECTIFY_THREADS = 256;
constexpr int RECTIFY_PER_LANE = 4;
constexpr int RECTIFY_TILE_COLS = 128;
constexpr int RECTIFY_TILE_ROWS = RECTIFY_THREADS * RECTIFY_PER_LANE / RECTIFY_TILE_COLS;

struct RectifyArgs {
    const void* src;  // n planes, u8 or u16
    void* dst;        // n planes, same depth
    const float* map_x;
    const float* map_y;
    uint8_t* valid;  // [rows][cols] dense, or nullptr
    int n, src_rows, src_cols, rows, cols;
    // elements; a plane spans less than 2^32 elements (32-bit in-plane offsets)
    uint32_t src_row_pitch, dst_row_pitch;
    size_t src_plane_pitch, dst_plane_pitch;
    uint32_t map_pitch;  // floats
    uint32_t border;
    // a lane's four pixels may go out as one aligned store: the stack's / the valid map's
    bool dst_vector, valid_vector;
};
hipError_t launch_rectify(const RectifyArgs& a, int depth, hipStream_t st);

// The calibration as the maps kernel takes it: iM = inverse(P[:, :3] * R), computed by the host
struct RectifyCamera {
    double iM[9];
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3, k4, k5, k6;
};
constexpr int RECTIFY_MAPS_THREADS = 256;
// dense float32 [rows][cols] maps
hipError_t launch_rectify_maps(const RectifyCamera& c, int rows, int cols, float* map_x,
                               float* map_y, hipStream_t st);

}  // namespace bicos_hip
