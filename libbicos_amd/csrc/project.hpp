// project.hpp -- launchers of project.hip: a point list projected into another camera, with a
// z-buffer for visibility, a texture value per point and the registered depth / index images
// (include/bicos_c.h, "projection"; the numpy restatement is tests/project_ref.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicos_hip {

// A workgroup of PROJECT_THREADS lanes owns PROJECT_PER_LANE * PROJECT_THREADS consecutive points;
// a lane's points lie PROJECT_THREADS apart, so a wave reads and writes runs.
constexpr int PROJECT_THREADS = 256;
constexpr int PROJECT_PER_LANE = 4;
constexpr int PROJECT_MAX_SPLAT = 3;

// The camera as the kernels take it: Pc = R*P + t, then bicos_c.h's rectification model
struct ProjectCamera {
    double R[9], t[3];
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3, k4, k5, k6;
};

struct ProjectArgs {
    ProjectCamera cam;
    const float* points;  // [count][3]
    uint32_t count;
    int img_rows, img_cols;
    int splat;
    float tol;
    // the texture source, or nullptr: u8 / u16 (depth 1 / 2), channels 1 / 3, pitch in elements
    const void* image;
    int depth, channels;
    size_t img_pitch;
    uint32_t fill;
    // outputs, each may be nullptr
    float* uv;           // [count][2]
    float* zdepth;       // [count]
    uint8_t* cls;        // [count]
    void* tex;           // [count][channels]
    float* depth_map;    // [img_rows][img_cols]
    int32_t* index_map;  // [img_rows][img_cols]
    uint32_t* counts;    // device uint32[5], zeroed by the launcher
    // workspace: the z-buffer's keys [img_rows][img_cols], or nullptr for no z-buffer (every
    // inside point is then visible and no map can be asked for)
    unsigned long long* keys;
};

// No z-buffer: the counts' memset and one launch. With one: the keys' memset, the splat, the
// resolve of the points (skipped when no per-point output and no counts are asked for) and,
// where a map is asked for, the resolve of the maps.
hipError_t launch_project(const ProjectArgs& a, hipStream_t st);

}  // namespace bicos_hip
