// bicos/speckle.hpp -- BICOS::filter_speckles: the speckle filter of a disparity map on the
// GPU (what cv::filterSpeckles does on a CPU). The reference has no such step, so the
// reference-named headers (include/BICOS/) do not gain it.
//
// The map is a dense S16 or F32 image in host or device memory. Valid pixels, links,
// components, labels and the removal rule are those of include/bicos_c.h ("speckle filter"):
// every 4-connected component of pixels whose neighbours differ by at most max_diff and that
// has at most max_size pixels becomes invalid; every other pixel is copied bit for bit.
// Errors throw BICOS::Exception.
#pragma once

#include <cstdint>
#include <vector>

#include "types.hpp"

namespace BICOS {

enum SpeckleFlags : int {
    SPECKLE_F32_SENTINEL = 1,  // a float -32768.0f is invalid too, and is what removal writes
};

// kept + removed + invalid = rows * cols
struct SpeckleStats {
    uint32_t kept = 0, removed = 0, invalid = 0, removed_components = 0;
};

// `out` becomes the filtered map in the memory of `disparity` (it may be `disparity` itself:
// in place); `labels`, when given, every pixel's component label (the smallest row * cols + col
// of its component, -1 where the pixel was invalid), in host memory. Synchronous for maps in
// either memory: the statistics come back with the call.
SpeckleStats filter_speckles(const HipImage& disparity, HipImage& out, int max_size,
                             float max_diff = 1.0f, int flags = 0,
                             std::vector<int32_t>* labels = nullptr);

// For a device map, asynchronous on `stream`: labels (int32 [rows*cols]) and counts
// (uint32[4] = {kept, removed, invalid, removed_components}) are device buffers or nullptr.
void filter_speckles(const HipImage& disparity, HipImage& out, int max_size, float max_diff,
                     int flags, int32_t* labels, uint32_t* counts, hipStream_t stream = nullptr);

}  // namespace BICOS
