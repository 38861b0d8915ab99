// guide.hpp -- launcher of search_guided.hip's guide_kernel: per-pixel disparity windows
// {lo, hi} for the guided search from a prior disparity map (include/bicos_c.h, "disparity
// guide").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicos_hip {

constexpr int GUIDE_BLOCK_ROWS = 4;  // a workgroup = 64 x 4 output pixels, one per lane

struct GuideArgs {
    const void* prior;  // int16 or float32, dense prows x pcols
    int prows, pcols;   // > 0
    int16_t* guide;     // rows x cols pairs {lo, hi}, 4-byte aligned
    size_t guide_pitch; // pixels (dwords) per guide row, >= cols
    int rows, cols;
    int scale;          // 1..8: output pixels per prior pixel, and the factor of its values
    int radius;         // 0..32767
    int spread;         // 0..7: the prior window is (2 spread + 1)^2
    int fallback_lo, fallback_hi;  // the pair where the window holds no valid value
    int sentinel;       // float32: -32768.0 is invalid too (NaN always is)
    uint32_t* counts;   // device uint32[2] {from_prior, fallback} or nullptr
};

// One launch on `st`, after a hipMemsetAsync of counts where they are asked for.
hipError_t launch_guide(const GuideArgs& a, bool f32, hipStream_t st);

}  // namespace bicos_hip
