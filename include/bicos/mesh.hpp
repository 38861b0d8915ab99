// bicos/mesh.hpp -- BICOS::mesh: a disparity map triangulated on the GPU, the vertices being the
// ordered point list of BICOS::reproject. The reference has no such step, so the reference-named
// headers (include/BICOS/) do not gain it.
//
// The map is a dense S16 or F32 image in host or device memory. Every 2x2 block of pixels is a
// quad of at most two triangles; a triangle is emitted where its three corners are kept points
// and its three edges join disparities that differ by at most max_diff. The definition, the
// order of the triangles and the flags are those of include/bicos_c.h ("mesh").
// Errors throw BICOS::Exception.
#pragma once

#include <cstdint>
#include <vector>

#include "reproject.hpp"

namespace BICOS {

enum MeshFlags : int {
    MESH_ALLOW_NEGATIVE_Z = REPROJECT_ALLOW_NEGATIVE_Z,  // keep points with Z < 0
    MESH_F32_SENTINEL = REPROJECT_F32_SENTINEL,          // a float -32768.0f is invalid too
};

// vertices: the four classes of the reprojection, summing to rows * cols. triangles is
// 2 * quads_full + quads_half; the three quad counts sum to (rows - 1) * (cols - 1).
struct MeshStats {
    ReprojectStats vertices;
    uint32_t triangles = 0, quads_full = 0, quads_half = 0, quads_empty = 0;
};

// Host vectors, for a map in either memory: `points` becomes the kept points (X, Y, Z each) in
// row-major pixel order, `triangles` three vertex numbers each, and `index`, when given, each
// vertex's pixel row * cols + col (what BICOS::normals takes). Synchronous (a device map's
// results are downloaded, the counts first).
MeshStats mesh(const HipImage& disparity, const Matx44d& Q, std::vector<float>& points,
               std::vector<int32_t>& triangles, float max_diff = 1.0f, int flags = 0,
               std::vector<int32_t>* index = nullptr);

// Device buffers, for a device map: points float32 [vertex_capacity][3], index int32
// [vertex_capacity] or nullptr, counts uint32[4], triangles int32 [tri_capacity][3], mesh_counts
// uint32[4] = {triangles, quads with 2, with 1, with 0}, vertex_map int32 [rows][cols] or
// nullptr. Nothing is written past a capacity; the counts are the full numbers. Asynchronous on
// `stream`.
void mesh(const HipImage& disparity, const Matx44d& Q, float* points, int32_t* index,
          size_t vertex_capacity, uint32_t* counts, int32_t* triangles, size_t tri_capacity,
          uint32_t* mesh_counts, float max_diff = 1.0f, int flags = 0,
          int32_t* vertex_map = nullptr, hipStream_t stream = nullptr);

}  // namespace BICOS
