// reproject.hip -- disparity map -> 3-D points through the rig's Q matrix (reproject.hpp).
//
// The arithmetic is bicos_cli::write_xyz's (libbicos_amd/cli/imageio.cpp; the reference runs
// cv::reprojectImageTo3D and save_pointcloud, src/cli.cpp:238, include/fileutils.hpp:44-89),
// operation for operation in IEEE double without contraction (-ffp-contract=off), so the
// float32 points are the CPU's bit for bit.
//
// Dense map: one launch, a lane per pixel and REPROJECT_PER_LANE pixels a block apart per lane.
// Ordered point list: three launches, no workgroup waiting on another and no atomics --
//   reproject_count_kernel  the four class counts of each segment of the linear pixel index
//   reproject_scan_kernel   one workgroup: exclusive scan of the segments' kept counts and the
//                           four totals into the caller's counts
//   reproject_write_kernel  the points again, placed by ballot / mbcnt ranks and wave totals
//                           in LDS on top of the segment's offset, below `capacity` only
#include "reproject_device.hpp"

namespace bicos_hip {
namespace {

// (the kernels are reproject_device.hpp's: mesh.hip builds its vertex list from the same code)

template <typename T>
hipError_t launch_points(const ReprojectArgs& a, hipStream_t st) {
    const uint32_t segments = reproject_segments(a.pixels);
    hipLaunchKernelGGL(reproject_count_kernel<T>, dim3(segments), dim3(REPROJECT_THREADS), 0, st, a);
    hipLaunchKernelGGL(reproject_scan_kernel, dim3(1), dim3(REPROJECT_SCAN_THREADS), 0, st,
                       (const uint32_t*)a.seg_counts, a.seg_offsets, segments, a.counts);
    if (a.xyz_map)
        hipLaunchKernelGGL((reproject_write_kernel<T, true, true>), dim3(segments),
                           dim3(REPROJECT_THREADS), 0, st, a, (int32_t*)nullptr);
    else
        hipLaunchKernelGGL((reproject_write_kernel<T, true, false>), dim3(segments),
                           dim3(REPROJECT_THREADS), 0, st, a, (int32_t*)nullptr);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_map(const ReprojectArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((reproject_write_kernel<T, false, true>), dim3(reproject_segments(a.pixels)),
                       dim3(REPROJECT_THREADS), 0, st, a, (int32_t*)nullptr);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_reproject_map(const ReprojectArgs& a, bool f32, hipStream_t st) {
    return f32 ? launch_map<float>(a, st) : launch_map<int16_t>(a, st);
}

hipError_t launch_reproject_points(const ReprojectArgs& a, bool f32, hipStream_t st) {
    return f32 ? launch_points<float>(a, st) : launch_points<int16_t>(a, st);
}

}  // namespace bicos_hip
