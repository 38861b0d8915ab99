// reproject.hpp -- launchers of reproject.hip: a dense disparity map through the rig's 4x4 Q
// matrix to 3-D points (include/bicos_c.h, "reprojection"; the CPU restatement is
// bicos_cli::write_xyz, libbicos_amd/cli/imageio.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicos_hip {

// The point list is built over fixed segments of the linear pixel index, one workgroup each:
// REPROJECT_THREADS lanes, each REPROJECT_PER_LANE pixels a block apart (so a wave's loads and
// its 12-byte stores stay contiguous).
constexpr int REPROJECT_THREADS = 256;
constexpr int REPROJECT_PER_LANE = 8;
constexpr int REPROJECT_SEGMENT = REPROJECT_THREADS * REPROJECT_PER_LANE;
constexpr int REPROJECT_SCAN_THREADS = 1024;

inline uint32_t reproject_segments(uint32_t pixels) {
    return (pixels + REPROJECT_SEGMENT - 1) / REPROJECT_SEGMENT;
}

struct ReprojectQ {
    double q[16];  // row-major
};

struct ReprojectArgs {
    const void* disp;  // int16 or float32, dense rows x cols
    int cols;
    uint32_t pixels;  // rows * cols (> 0)
    int flags;        // BICOS_REPROJECT_*
    ReprojectQ Q;
    float* xyz_map;     // [pixels][3] or nullptr
    float* points;      // [capacity][3] or nullptr
    int32_t* index;     // [capacity] or nullptr
    uint32_t capacity;  // points / index never written at or past it
    uint32_t* counts;   // device uint32[4]: kept, invalid, nonfinite, negative_z
    // workspace of the list path: 4 class counts per segment, then the kept offsets
    uint32_t* seg_counts;   // [segments][4]
    uint32_t* seg_offsets;  // [segments]
};

// The dense map alone: one launch.
hipError_t launch_reproject_map(const ReprojectArgs& a, bool f32, hipStream_t st);
// The ordered list (and the dense map with it when a.xyz_map is set): count, scan, write.
hipError_t launch_reproject_points(const ReprojectArgs& a, bool f32, hipStream_t st);

}  // namespace bicos_hip
