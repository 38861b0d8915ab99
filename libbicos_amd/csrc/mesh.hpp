// mesh.hpp -- launchers of mesh.hip: a dense disparity map to a triangle mesh over the ordered
// point list of the reprojection (include/bicos_c.h, "mesh"; the CPU restatement is
// tests/mesh_ref.py).
#pragma once

#include "reproject.hpp"

namespace bicos_hip {

// The mesh runs over the reprojection's segments of the linear pixel index, one workgroup each.
struct MeshArgs {
    ReprojectArgs v;       // the vertex list: disp, cols, pixels, flags, Q, points, index, capacity,
                           // counts, seg_counts, seg_offsets (xyz_map unused)
    int rows;
    float max_diff;        // the link: fabsf(d_p - d_q) <= max_diff
    int32_t* rank;         // [pixels]: the pixel's vertex number or -1 (the caller's vertex_map or
                           // workspace)
    int32_t* triangles;    // [tri_capacity][3]
    uint32_t tri_capacity; // triangles never written at or past it
    uint32_t* mesh_counts; // device uint32[4]: triangles, quads with 2, with 1, with 0
    // workspace: per segment {triangles, quads with 2, with 1, with 0}, then the triangle offsets
    uint32_t* tri_counts;   // [segments][4]
    uint32_t* tri_offsets;  // [segments]
};

// Vertex count, scan and write (with the ranks), triangle count, scan and write: six launches.
hipError_t launch_mesh(const MeshArgs& a, bool f32, hipStream_t st);

}  // namespace bicos_hip
