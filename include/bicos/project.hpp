// bicos/project.hpp -- BICOS::project: a point list projected into another camera on the GPU: a
// pixel position, a depth and a class per point, that camera's image sampled at the point (a
// texture), and the scan as that camera sees it, a depth image and an index image on its pixel
// grid, through a z-buffer that tells which points a nearer surface hides. The reference has no
// such step, so the reference-named headers (include/BICOS/) do not gain it.
//
// The points are float32 triples in the frame of Q: the list of BICOS::reproject or BICOS::mesh,
// or a dense xyz image taken as a list. The arithmetic, the classes and the z-buffer are those of
// include/bicos_c.h ("projection"); the results are bit for bit what that definition gives in
// float64 on a CPU. Errors throw BICOS::Exception.
#pragma once

#include <array>
#include <cstdint>
#include <limits>
#include <vector>

#include "types.hpp"

namespace BICOS {

// Pc = R*P + T, then the rectification's model: K row-major (the skew ignored), D with 0, 4, 5 or
// 8 coefficients k1 k2 p1 p2 [k3 [k4 k5 k6]], an image of rows x cols pixels.
struct Camera {
    std::array<double, 9> K{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    std::vector<double> D;
    std::array<double, 9> R{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    std::array<double, 3> T{{0, 0, 0}};
    int rows = 0, cols = 0;
};

enum ProjectClass : uint8_t {
    PROJECT_VISIBLE = 0,
    PROJECT_OCCLUDED = 1,
    PROJECT_OUTSIDE = 2,
    PROJECT_BEHIND = 3,
    PROJECT_INVALID = 4,
};

struct ProjectParams {
    int splat = 0;  // a point covers (2*splat+1)^2 pixels of the z-buffer; 0 .. 3
    float tol = std::numeric_limits<float>::infinity();  // occluded: !(z <= zmin + tol)
    int fill = 0;  // the texture value of a point that is not visible
};

// every point is in exactly one class: the five sum to the number of points
struct ProjectStats {
    uint32_t visible = 0, occluded = 0, outside = 0, behind = 0, invalid = 0;
};

// The texture source: a U8 or U16 image of cam.rows x channels*cam.cols values, channels in
// {1, 3} interleaved, any row step.
struct ProjectImage {
    const HipImage* image = nullptr;
    int channels = 1;
};

// What to compute; every pointer may be null, one at least is not. Host vectors are resized:
// uv 2 per point, depth and cls 1, tex `channels` VALUES per point as bytes of the image's type
// (a U16 texture takes 2 bytes per value), the maps cam.rows * cam.cols.
struct ProjectHostOutputs {
    std::vector<float>* uv = nullptr;
    std::vector<float>* depth = nullptr;
    std::vector<uint8_t>* cls = nullptr;
    std::vector<uint8_t>* tex = nullptr;
    std::vector<float>* depth_map = nullptr;
    std::vector<int32_t>* index_map = nullptr;
};

// Host memory: `points` (3 * count floats) and the image, if any, are in host memory.
// Synchronous.
ProjectStats project(const float* points, size_t count, const Camera& cam,
                     const ProjectHostOutputs& out, const ProjectParams& params = {},
                     const ProjectImage& image = {});

// Device memory: the points, the image and every output, as bicos_project_device takes them
// (counts uint32[5] = {visible, occluded, outside, behind, invalid}). Asynchronous on `stream`.
struct ProjectDeviceOutputs {
    float* uv = nullptr;
    float* depth = nullptr;
    uint8_t* cls = nullptr;
    void* tex = nullptr;
    float* depth_map = nullptr;
    int32_t* index_map = nullptr;
    uint32_t* counts = nullptr;
};
void project(const float* points, size_t count, const Camera& cam, const ProjectDeviceOutputs& out,
             const ProjectParams& params = {}, const ProjectImage& image = {},
             hipStream_t stream = nullptr);

}  // namespace BICOS
