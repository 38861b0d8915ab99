// pool.hpp -- launcher of pool.hip: an image stack pooled by an integer factor, the mean of
// every scale x scale block rounded half up in integer arithmetic (include/bicos_c.h, "stack
// pooling"; the numpy restatement is tests/test_pool_api.py).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicos_hip {

// One workgroup pools a POOL_TILE_ROWS x POOL_TILE_COLS tile of OUTPUT pixels of one plane: a
// lane owns POOL_PER_LANE consecutive output pixels of one row (one dword of u8, two of u16), so
// it reads scale rows of POOL_PER_LANE * scale contiguous source elements, and a wave covers two
// output rows: per source row two runs of 128 * scale (u8) or 256 * scale (u16) bytes.
constexpr int POOL_THREADS = 256;
constexpr int POOL_PER_LANE = 4;
constexpr int POOL_TILE_COLS = 128;
constexpr int POOL_TILE_ROWS = POOL_THREADS * POOL_PER_LANE / POOL_TILE_COLS;
constexpr int POOL_MIN_SCALE = 2, POOL_MAX_SCALE = 8;

struct PoolArgs {
    const void* src;  // n planes of rows x cols, u8 or u16
    void* dst;        // n planes of prows x pcols, same depth
    int n, prows, pcols;  // the OUTPUT size: rows / scale, cols / scale
    // elements; a plane spans less than 2^32 elements (32-bit in-plane offsets)
    uint32_t src_row_pitch, dst_row_pitch;
    size_t src_plane_pitch, dst_plane_pitch;
    bool dst_vector;  // set by launch_pool: pool_dst_vector()
};

// Whether the dword-load kernel serves this source: its base and its two pitches, in bytes, are
// multiples of 4. Every other source runs the per-element kernel. The results are the same.
bool pool_wide(const PoolArgs& a, int depth);
// Whether that kernel stores a lane's four pixels as one vector: the output's base and its two
// pitches, in bytes, are multiples of 4 (else four element stores)
bool pool_dst_vector(const PoolArgs& a, int depth);
// Workgroups of the launch (the entries refuse more than INT32_MAX: one grid dimension)
uint64_t pool_blocks(const PoolArgs& a);
// One launch on `st`. scale in POOL_MIN_SCALE .. POOL_MAX_SCALE, depth 1 or 2.
hipError_t launch_pool(const PoolArgs& a, int depth, int scale, hipStream_t st);

}  // namespace bicos_hip
