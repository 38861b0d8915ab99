// bicos/normals.hpp -- BICOS::normals: one unit surface normal per pixel of a disparity map,
// oriented towards the camera, on the GPU: the least-squares plane of the disparities over a
// (2*radius+1)^2 window in (column, row, disparity), carried through the rig's 4x4 Q matrix.
// The reference has no such call, so the reference-named headers (include/BICOS/) do not gain it.
//
// The map is a dense S16 or F32 image in host or device memory. The stage is for SUBPIXEL maps:
// integer disparities stair-step (include/bicos_c.h, "surface normals", which also holds the
// arithmetic, the pixel classes and the flags); the float32 results are bit for bit what that
// double-precision text gives on a CPU. Errors throw BICOS::Exception.
#pragma once

#include <cstdint>
#include <vector>

#include "reproject.hpp"
#include "types.hpp"

namespace BICOS {

enum NormalsFlags : int {
    NORMALS_ALLOW_NEGATIVE_Z = 1,  // as REPROJECT_ALLOW_NEGATIVE_Z
    NORMALS_F32_SENTINEL = 2,      // as REPROJECT_F32_SENTINEL
};

struct NormalsParams {
    int radius = 2;        // 1 .. 4
    float max_diff = 1.f;  // a window pixel takes part if its disparity is within this of the centre's
    int min_points = 3;    // 3 .. (2*radius+1)^2
    int flags = 0;         // NormalsFlags
};

// every pixel is in exactly one class: the four sum to rows * cols
struct NormalStats {
    uint32_t normal = 0, no_point = 0, sparse = 0, degenerate = 0;
};

// Dense map: normal_map becomes an F32 image of rows x 3*cols (NX, NY, NZ interleaved) in the
// memory of `disparity`, the unit normal where the pixel has one and three NaNs elsewhere. With a
// device map the call is asynchronous on `stream`; with a host map it is synchronous.
void normals(const HipImage& disparity, const Matx44d& Q, HipImage& normal_map,
             const NormalsParams& params = {}, hipStream_t stream = nullptr);

// List: normals_out becomes the normal (NX, NY, NZ each) of every pixel of `index`, as
// BICOS::reproject writes it, three NaNs where the pixel has none or the entry lies outside the
// map. With normal_map the dense map is produced by the same call, and the returned stats
// count its classes (all zero without it). Synchronous for maps in either memory.
NormalStats normals(const HipImage& disparity, const Matx44d& Q, const std::vector<int32_t>& index,
                    std::vector<float>& normals_out, const NormalsParams& params = {},
                    HipImage* normal_map = nullptr);

// Raw device buffers, for a device map: normal_map float32 [rows][cols][3] or nullptr; index
// int32 [count] with normals float32 [count][3], or both nullptr; counts uint32[4] = {normal,
// no_point, sparse, degenerate} or nullptr (only with normal_map). Asynchronous on `stream`.
void normals(const HipImage& disparity, const Matx44d& Q, float* normal_map, const int32_t* index,
             size_t count, float* normals_out, uint32_t* counts, const NormalsParams& params = {},
             hipStream_t stream = nullptr);

}  // namespace BICOS
