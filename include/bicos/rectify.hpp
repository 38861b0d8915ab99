// bicos/rectify.hpp -- BICOS::rectify_maps and BICOS::rectify: the stage before match(), raw
// camera frames to rectified stacks on the GPU (what cv::initUndistortRectifyMap and cv::remap
// with INTER_LINEAR do on a CPU, image by image). The reference starts at rectified imagery, so
// the reference-named headers (include/BICOS/) do not gain it.
//
// The camera model, the bilinear blend, the border and the valid map are those of
// include/bicos_c.h ("rectification"). Errors throw BICOS::Exception.
#pragma once

#include <vector>

#include "types.hpp"

namespace BICOS {

// One camera's calibration as cv::stereoRectify and cv::calibrateCamera hand it over, row-major.
struct RectifyCamera {
    double K[9];               // intrinsics; the skew K[1] is ignored
    std::vector<double> D;     // 0, 4, 5 or 8 coefficients k1 k2 p1 p2 [k3 [k4 k5 k6]]
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // rectifying rotation
    std::vector<double> P;     // new projection matrix, 3x3 (9) or 3x4 (12); left 3x3 used
};

// map_x / map_y become dense F32 rows x cols images in `mem`: the absolute source coordinates
// of every output pixel. Device maps: asynchronous on `stream`. Host maps: synchronous.
void rectify_maps(const RectifyCamera& camera, int rows, int cols, HipImage& map_x, HipImage& map_y,
                  Memory mem = Memory::Device, hipStream_t stream = nullptr);

// The n images of `stack` (U8 or U16, one size, all in the memory of the maps) through one pair
// of maps into out_stack: n images of the maps' size and the stack's type in the same memory
// (images of out_stack that already have that shape are written in place, like cv::Mat::create).
// valid, when given, becomes a U8 image: 1 where every contributing tap lies in the source.
// Device memory: asynchronous on `stream`; ONE launch for all n images when the stack and
// out_stack are each one planar buffer (equal steps, images equally spaced, as match() reads
// them zero-copy), else one launch per image. Host memory: synchronous (upload, one launch,
// download); the images of each stack must share one step.
void rectify(const std::vector<HipImage>& stack, const HipImage& map_x, const HipImage& map_y,
             std::vector<HipImage>& out_stack, int border = 0, HipImage* valid = nullptr,
             hipStream_t stream = nullptr);

}  // namespace BICOS
