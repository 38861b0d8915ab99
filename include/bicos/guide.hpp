// bicos/guide.hpp -- BICOS::guide_from_disparity: per-pixel disparity windows for the guided
// match (the BICOS::match overload of bicos/match.hpp that takes a guide) from a prior
// disparity map -- the previous frame's map, the match of a downsampled stack, a neighbouring
// view. The reference has no such step.
//
// A guide of a rows x cols frame is an S16 image of rows x 2 cols: the pairs {lo, hi} of the
// pixels of a row side by side (include/bicos_c.h, "disparity guide", which also states the
// builder's arithmetic: pr = min(r / scale, prows - 1), the (2 spread + 1)^2 window of valid
// prior values, lo = scale * floor(min) - radius, hi = scale * ceil(max) + scale - 1 + radius,
// the fallback pair where the window holds no valid value). The prior is a dense S16 or F32
// image in host or device memory; the guide is created in the same memory. Errors throw
// BICOS::Exception.
#pragma once

#include <cstdint>

#include "types.hpp"

namespace BICOS {

enum GuideFlags : int {
    GUIDE_F32_SENTINEL = 1,  // a float -32768.0f is invalid too (NaN always is)
};

struct GuideParams {
    int radius = 0;  // 0 .. 32767
    int spread = 0;  // 0 .. 7
    int scale = 1;   // 1 .. 8
    // the window where the prior knows nothing; lo > hi: do not search there
    int fallback_lo = -32767, fallback_hi = 32767;
    int flags = 0;
};

// from_prior + fallback = rows * cols
struct GuideStats {
    uint32_t from_prior = 0, fallback = 0;
};

// `guide` becomes the rows x cols guide (an S16 image of rows x 2 cols) in the memory of
// `prior`. Synchronous: the statistics come back with the call.
GuideStats guide_from_disparity(const HipImage& prior, HipImage& guide, int rows, int cols,
                                const GuideParams& params = GuideParams{});

// For a device prior, asynchronous on `stream`: counts (uint32[2] = {from_prior, fallback}) is
// a device buffer or nullptr.
void guide_from_disparity(const HipImage& prior, HipImage& guide, int rows, int cols,
                          const GuideParams& params, uint32_t* counts,
                          hipStream_t stream = nullptr);

}  // namespace BICOS
