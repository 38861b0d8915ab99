// bicos/median.hpp -- BICOS::median_filter: the 3x3 / 5x5 median filter of a disparity map on
// the GPU (what cv::medianBlur does on a CPU), which knows the map's invalid values and can
// fill small holes. The reference has no such step, so the reference-named headers
// (include/BICOS/) do not gain it.
//
// The map is a dense S16 or F32 image in host or device memory. Valid pixels, the clipped
// window, the order, the lower median and the fill rule are those of include/bicos_c.h
// ("median filter"): a valid pixel becomes the median of the valid values of its window; an
// invalid one becomes it too where fill_min > 0 and the window holds at least fill_min valid
// values; every other pixel is copied bit for bit. Errors throw BICOS::Exception.
#pragma once

#include <cstdint>

#include "types.hpp"

namespace BICOS {

enum MedianFlags : int {
    MEDIAN_F32_SENTINEL = 1,  // a float -32768.0f is invalid too
};

// unchanged + changed + filled + invalid = rows * cols
struct MedianStats {
    uint32_t unchanged = 0, changed = 0, filled = 0, invalid = 0;
};

// `out` becomes the filtered map in the memory of `disparity`. For a host map it may be
// `disparity` itself; for a device map it must be another image (the filter reads neighbours).
// Synchronous for maps in either memory: the statistics come back with the call.
MedianStats median_filter(const HipImage& disparity, HipImage& out, int ksize = 3,
                          int fill_min = 0, int flags = 0);

// For a device map, asynchronous on `stream`: counts (uint32[4] = {unchanged, changed, filled,
// invalid}) is a device buffer or nullptr.
void median_filter(const HipImage& disparity, HipImage& out, int ksize, int fill_min, int flags,
                   uint32_t* counts, hipStream_t stream = nullptr);

}  // namespace BICOS
