// bicos/reproject.hpp -- BICOS::reproject: a disparity map through the rig's 4x4 Q matrix to
// 3-D points on the GPU. The reference does this step in its command-line tool only
// (cv::reprojectImageTo3D + save_pointcloud, src/cli.cpp:238, include/fileutils.hpp:44-89);
// its library has no such call, so the reference-named headers (include/BICOS/) do not gain it.
//
// The map is a dense S16 or F32 image in host or device memory. The arithmetic, the pixel
// classes and the flags are those of include/bicos_c.h ("reprojection"); the float32 results
// are bit for bit what that double-precision formula gives on a CPU.
// Errors throw BICOS::Exception.
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "types.hpp"

namespace BICOS {

enum ReprojectFlags : int {
    REPROJECT_ALLOW_NEGATIVE_Z = 1,  // keep points with Z < 0
    REPROJECT_F32_SENTINEL = 2,      // a float -32768.0f is invalid too (NXC without subpixel)
};

// every pixel is in exactly one class: the four sum to rows * cols
struct ReprojectStats {
    uint32_t kept = 0, invalid = 0, nonfinite = 0, negative_z = 0;
};

using Matx44d = std::array<double, 16>;  // row-major

// Dense map: xyz becomes an F32 image of rows x 3*cols (X, Y, Z interleaved) in the memory of
// `disparity`, the point where the pixel is kept and three NaNs elsewhere. With a device map
// the call is asynchronous on `stream`; with a host map it is synchronous.
void reproject(const HipImage& disparity, const Matx44d& Q, HipImage& xyz, int flags = 0,
               hipStream_t stream = nullptr);

// Point list: `points` becomes the kept points (X, Y, Z each) in row-major pixel order, and
// `index`, when given, each point's pixel row * cols + col. Synchronous for maps in either
// memory (a device map's points are downloaded).
ReprojectStats reproject(const HipImage& disparity, const Matx44d& Q, std::vector<float>& points,
                         int flags = 0, std::vector<int32_t>* index = nullptr);

// Point list into device buffers, for a device map: points float32 [capacity][3], index int32
// [capacity] or nullptr, counts uint32[4] = {kept, invalid, nonfinite, negative_z}. No more
// than `capacity` points are written; counts[0] is the full number. Asynchronous on `stream`.
void reproject(const HipImage& disparity, const Matx44d& Q, float* points, int32_t* index,
               size_t capacity, uint32_t* counts, int flags = 0, hipStream_t stream = nullptr);

}  // namespace BICOS
