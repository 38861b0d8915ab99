// bicos/pool.hpp -- BICOS::pool_stack and BICOS::match_pyramid: an image stack pooled by an
// integer factor on the GPU, and the coarse-to-fine match built on it in one call (pool both
// stacks, match them over the scaled window, turn that map into a guide, run the guided match).
// The reference has neither.
//
// The pooling is that of include/bicos_c.h ("stack pooling"): out = (sum of the scale x scale
// block + scale*scale/2) / (scale*scale) in integers, the mean rounded half up; the output is
// rows / scale x cols / scale and the remainder rows and columns are not read. The pyramid match
// is, byte for byte, the four calls that "pyramid match" there lists. Errors throw
// BICOS::Exception.
#pragma once

#include <cstdint>
#include <vector>

#include "types.hpp"

namespace BICOS {

// The n images of `stack` (U8 or U16, one size, one memory) pooled by `scale` (2 .. 8) into
// out_stack: n images of rows / scale x cols / scale of the stack's type in the same memory
// (images of out_stack that already have that shape are written in place, like cv::Mat::create;
// an out_stack none of whose images has it becomes, in device memory, n row ranges of ONE planar
// allocation). Device memory: asynchronous on `stream`; ONE launch for all n images when the
// stack and out_stack are each one planar buffer (equal steps, images equally spaced, as match()
// reads them zero-copy -- a fresh out_stack is), else one launch per image. Host memory:
// synchronous (upload, one launch, download); the images of each stack must share one step.
void pool_stack(const std::vector<HipImage>& stack, int scale, std::vector<HipImage>& out_stack,
                hipStream_t stream = nullptr);

struct PyramidParams {
    int scale = 2;   // 2 .. 8: the pooling factor of the coarse level
    int radius = 2;  // 0 .. 32767: the guide's margin around the scaled coarse disparity
    int spread = 1;  // 0 .. 7: the guide looks at (2 spread + 1)^2 coarse pixels
    // where the coarse map knows nothing: the global window (clamped to +-32767), or the pair
    // below (lo > hi: do not search there)
    bool fallback_window = true;
    int fallback_lo = 0, fallback_hi = 0;
};

// The pyramid match. cfg.disparity_range is required: it is the global window of the fine match
// and, divided by the scale, of the coarse one. Outputs as BICOS::match's, in the memory of the
// stacks; besides, where given: `coarse` becomes the coarse map (rows / scale x cols / scale,
// F32 with an nxcorr_threshold, else S16), `guide` the guide (S16, rows x 2 cols; bicos/guide.hpp)
// and counts[2] = {from_prior, fallback} of the guide -- a device buffer for device stacks
// (asynchronous on `stream`), a host buffer for host stacks (synchronous).
void match_pyramid(const std::vector<HipImage>& stack0, const std::vector<HipImage>& stack1,
                   HipImage& disparity, Config cfg, const PyramidParams& params = PyramidParams{},
                   HipImage* corrmap = nullptr, HipImage* coarse = nullptr,
                   HipImage* guide = nullptr, uint32_t* counts = nullptr,
                   hipStream_t stream = nullptr);

}  // namespace BICOS
