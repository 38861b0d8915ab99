// host_plan.hpp -- the arithmetic of the banded host-buffer pipeline (host.cpp match_host):
// which rows form a band, how a band's upload is split over the copy streams, which bytes of
// a landed band each pool task delivers. Plain integers in and out, no HIP header: host.cpp
// issues exactly the copies these functions name, and tests/cpp/host_plan_check.cpp checks
// them exhaustively on the CPU (tests/test_host_plan.py).
#pragma once

#include <algorithm>
#include <cstddef>

namespace bicos_impl {
namespace host_plan {

// a byte range [offset, offset + length)
struct Span {
    size_t offset = 0, length = 0;
};

// Row bands (every stage is row-local): upload of band b+1 overlaps the match
// of band b; ~8 bands keep the pipeline tail short without starving the search.
struct BandPlan {
    int rows = 0;
    int band_rows = 0;  // rows of every band but the last
    int B = 0;          // bands
    int K = 0;          // pinned slots in flight: band b uses slot b % K
    int first_row(int b) const { return b * band_rows; }
    int height(int b) const { return std::min(band_rows, rows - b * band_rows); }
};

inline BandPlan plan_bands(int rows) {
    BandPlan p;
    p.rows = rows;
    const int want = rows >= 1024 ? 8 : rows >= 256 ? 4 : rows >= 64 ? 2 : 1;
    p.band_rows = (rows + want - 1) / want;
    p.B = (rows + p.band_rows - 1) / p.band_rows;
    p.K = p.B > 1 ? 3 : 1;
    return p;
}

// The upload of a band of `up` bytes over `streams` (1 or 2) copy streams: the first stream
// takes [0, first), the second [first, up). With two streams the cut is the middle rounded up
// to a page of 4096 bytes; a band of at most one page is one copy on the first stream (the
// rounded middle would lie past its end).
inline size_t upload_first(size_t up, int streams) {
    if (streams != 2 || up <= 4096) return up;
    return (up / 2 + 4095) / 4096 * 4096;
}

// ... as the copies to issue: part[0] on the first stream, part[1] (when 2 is returned) on the
// second; offsets within the band, the same in the pinned slot and on the device.
inline int upload_parts(size_t up, int streams, Span part[2]) {
    const size_t first = upload_first(up, streams);
    part[0] = Span{0, first};
    part[1] = Span{first, up - first};
    return first < up ? 2 : 1;
}

// Rows [r0, r0 + br) of a dense map of `cols` elements of `esz` bytes: what band b's download
// copies, at the same offset on the device and in the pinned map.
inline Span map_rows(int r0, int br, int cols, size_t esz) {
    return Span{(size_t)r0 * cols * esz, (size_t)br * cols * esz};
}

// deliver_band: a landed band's `bytes` of one map go to the caller in `parts` chunks of a
// multiple of 64 bytes (the last one shorter, trailing ones empty); chunk i is this range of
// the band's bytes. The chunk is the share rounded UP: rounded down, a band of 8 * 64 k + r
// bytes (0 < r < 8) had its last r bytes in no chunk.
constexpr int DELIVER_PARTS = 8;  // per map and band (host.cpp deliver_band)
inline Span deliver_part(size_t bytes, int parts, int i) {
    const size_t chunk = ((bytes + parts - 1) / parts + 63) / 64 * 64;
    const size_t o = (size_t)i * chunk;
    if (o >= bytes) return Span{bytes, 0};
    return Span{o, std::min(chunk, bytes - o)};
}

}  // namespace host_plan
}  // namespace bicos_impl
