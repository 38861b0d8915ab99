// host_plan_check.cpp -- TEST PROGRAM (tests/test_host_plan.py, no GPU): the arithmetic of the
// banded host-buffer pipeline (libbicos_amd/csrc/host_plan.hpp, which host.cpp's match_host
// calls for every copy it issues), checked exhaustively on the CPU.
//
//   host_plan_check [align]   bands, split, delivery and stage layout; one "<what> ok <count>"
//                             line each, or "FAIL ..." lines and exit status 1. align: the
//                             stage's sub-buffer alignment (engine.hpp ALIGN, default 256).
//   host_plan_check parent    the split properties on the formula match_host used before
//                             upload_first (below, the thing being rejected): one line per
//                             stream count, "split streams=<s> violations <lo>..<hi> ..." or
//                             "... violations none"; then the delivery's tiling on the chunk
//                             deliver_band used before deliver_part; exit status 0.
//   host_plan_check frames    the stage-layout table: "n rows cols depth" per line.
#include "host_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace bicos_impl::host_plan;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures++ < 20) {                        \
                std::printf("FAIL %s: ", #cond);          \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

// ---------------------------------------------------------------------------------- bands
static int check_bands() {
    for (int rows = 1; rows <= 20000; ++rows) {
        const BandPlan p = plan_bands(rows);
        CHECK(p.rows == rows && p.band_rows >= 1, "rows %d", rows);
        CHECK(p.B >= 1 && p.B <= 8, "rows %d: B %d", rows, p.B);
        CHECK(p.K >= 1 && p.K <= 3, "rows %d: K %d", rows, p.K);
        CHECK((p.K == 1) == (p.B == 1), "rows %d: B %d K %d", rows, p.B, p.K);
        int next = 0;  // the bands tile [0, rows) once and in order
        for (int b = 0; b < p.B; ++b) {
            CHECK(p.first_row(b) == next, "rows %d band %d starts at %d, not %d", rows, b,
                  p.first_row(b), next);
            CHECK(p.height(b) >= 1 && p.height(b) <= p.band_rows, "rows %d band %d height %d", rows,
                  b, p.height(b));
            next += p.height(b);
        }
        CHECK(next == rows, "rows %d: bands end at %d", rows, next);
    }
    return 20000;
}

// ---------------------------------------------------------------------------------- split
// What match_host computed before upload_first: the middle rounded up to a page, whatever the
// band's size. Written out here as the thing the properties must reject.
static size_t parent_first(size_t up, int streams) {
    return streams == 2 ? (up / 2 + 4095) / 4096 * 4096 : up;
}

static std::vector<size_t> split_sizes() {
    std::vector<size_t> v;
    for (size_t up = 0; up <= 70000; ++up) v.push_back(up);
    const size_t G = (size_t)1 << 30;
    for (size_t up : {(size_t)1 << 20, ((size_t)1 << 20) + 1, 2 * G - 1, 2 * G, 2 * G + 4097,
                      4 * G - 1, 4 * G, 4 * G + 1, 8 * G - 4096, 8 * G - 1, 8 * G})
        v.push_back(up);
    return v;
}

// The properties of one split: the copies are [0, first) on the first stream and [first, up)
// on the second, as match_host issues them. The name of the first one violated, or nullptr.
static const char* split_violation(size_t up, int streams, size_t first) {
    if (first > up) return "first <= up";
    const Span a{0, first}, b{first, up - first};  // (first <= up: no wrap)
    if (a.offset != 0 || a.offset + a.length != b.offset || b.offset + b.length != up)
        return "the two parts tile [0, up)";
    if (streams == 1 && first != up) return "one stream: first == up";
    if (streams == 2 && first % 4096 != 0 && first != up)
        return "two streams: first is a multiple of 4096 or equals up";
    // the first stream's event is the one every band records and waits on: it carries bytes
    if (up > 0 && first == 0) return "first > 0 where up > 0";
    return nullptr;
}

static int check_split() {
    int count = 0;
    for (int streams = 1; streams <= 2; ++streams)
        for (size_t up : split_sizes()) {
            const size_t first = upload_first(up, streams);
            const char* bad = split_violation(up, streams, first);
            CHECK(!bad, "up %zu streams %d first %zu: %s", up, streams, first, bad ? bad : "");
            Span part[2];
            const int copies = upload_parts(up, streams, part);  // ... and as the copies themselves
            CHECK(part[0].offset == 0 && part[0].length == first && part[1].offset == first &&
                      part[1].length == up - first && copies == (first < up ? 2 : 1),
                  "up %zu streams %d: upload_parts disagrees with upload_first", up, streams);
            ++count;
        }
    return count;
}

static void report_parent() {
    for (int streams = 1; streams <= 2; ++streams) {
        std::string line;
        bool open = false;
        size_t lo = 0, prev = 0;
        auto close = [&] {
            if (open) line += " " + std::to_string(lo) + ".." + std::to_string(prev);
            open = false;
        };
        for (size_t up : split_sizes()) {
            const bool bad = split_violation(up, streams, parent_first(up, streams)) != nullptr;
            if (bad && open && up == prev + 1) {
                prev = up;
            } else if (bad) {
                close();
                open = true;
                lo = prev = up;
            } else {
                close();
            }
        }
        close();
        std::printf("split streams=%d violations%s\n", streams, line.empty() ? " none" : line.c_str());
    }
}

// ------------------------------------------------------------------------------- delivery
// the parts of `bytes` tile [0, bytes): in order, none overlapping, none past the end
static void check_delivery_of(size_t bytes, int parts) {
    size_t cursor = 0;
    for (int i = 0; i < parts; ++i) {
        const Span s = deliver_part(bytes, parts, i);
        CHECK(s.offset <= bytes && s.length <= bytes - s.offset, "bytes %zu part %d: [%zu, +%zu)",
              bytes, i, s.offset, s.length);
        if (!s.length) continue;
        CHECK(s.offset == cursor, "bytes %zu part %d starts at %zu, not %zu", bytes, i, s.offset,
              cursor);
        cursor = s.offset + s.length;
    }
    CHECK(cursor == bytes, "bytes %zu: the parts end at %zu", bytes, cursor);
}

// What deliver_band computed before deliver_part: the share rounded down, then up to 64.
static Span parent_part(size_t bytes, int parts, int i) {
    const size_t chunk = (bytes / parts + 63) / 64 * 64, o = (size_t)i * chunk;
    if (o >= bytes) return Span{bytes, 0};
    return Span{o, std::min(chunk, bytes - o)};
}

// ... on which the tiling must fail for exactly bytes = 512 k + r, 0 < r < 8: there the 8
// chunks of 64 k bytes end r bytes short
static void report_parent_delivery() {
    int bad = 0, unexpected = 0;
    for (size_t bytes = 0; bytes <= 20000; ++bytes) {
        size_t cursor = 0;
        for (int i = 0; i < DELIVER_PARTS; ++i) {
            const Span s = parent_part(bytes, DELIVER_PARTS, i);
            if (s.length && s.offset == cursor) cursor += s.length;
        }
        const bool short_of = cursor != bytes, expected = bytes % 512 >= 1 && bytes % 512 <= 7;
        bad += short_of;
        unexpected += short_of != expected;
    }
    std::printf("delivery violations %d, %d not of the form 512 k + 1..7\n", bad, unexpected);
}

static int check_delivery() {
    int count = 0;
    for (size_t bytes = 0; bytes <= 20000; ++bytes, ++count) check_delivery_of(bytes, DELIVER_PARTS);
    const size_t G = (size_t)1 << 30;
    for (size_t bytes : {(size_t)519, 64 * G + 1, 2 * G - 1, 2 * G + 2, 4 * G + 4, 4 * G + 6,
                         8 * G - 2, 8 * G + 516, 8 * G * 8 + 7}) {
        check_delivery_of(bytes, DELIVER_PARTS);
        ++count;
    }
    return count;
}

// --------------------------------------------------------------------------- stage layout
struct Frame {
    int n, rows, cols, depth;
};
// every frame of tests/test_host_small_gpu.py, and those of tests/test_host_path.py's band test
static const Frame FRAMES[] = {
    {4, 8, 8, 1},     {8, 5, 51, 1},    {8, 4, 64, 1},    {10, 5, 41, 1},   {12, 9, 19, 1},
    {17, 1, 241, 1},  {6, 64, 10, 1},   {6, 64, 5, 2},    {6, 256, 5, 1},   {6, 257, 5, 1},
    {5, 1030, 3, 1},  {6, 1030, 2, 1},  {12, 301, 256, 1}, {12, 1100, 256, 1}, {12, 63, 256, 1},
    {12, 301, 256, 2}, {4, 43, 3, 1},   {4, 86, 3, 1},    {12, 1, 257, 1},  {12, 300, 99, 1},
    {12, 1, 256, 1},  {12, 64, 256, 1}, {8, 2, 64, 1},    {33, 1536, 2048, 1},
};

static size_t g_align = 256;
static size_t align_up(size_t x) { return (x + g_align - 1) / g_align * g_align; }

static bool inside(size_t begin, const Span& s, size_t lo, size_t hi) {
    return begin + s.offset >= lo && begin + s.offset + s.length <= hi;  // (far from 2^64)
}

static void check_layout_of(const Frame& f, bool nxcorr, bool dbl, int streams) {
    const BandPlan p = plan_bands(f.rows);
    const size_t row_bytes = (size_t)f.cols * f.depth;
    const size_t band_bytes = 2 * (size_t)f.n * p.band_rows * row_bytes;
    const size_t dsz = nxcorr ? 4 : 2, csz = dbl ? 8 : 4;
    const size_t disp_bytes = (size_t)f.rows * f.cols * dsz;
    const size_t corr_bytes = nxcorr ? (size_t)f.rows * f.cols * csz : 0;
    // the stage as carve() takes it: bands | disparity | corrmap, each aligned
    const size_t bands_end = (size_t)p.B * band_bytes;
    const size_t disp_at = align_up(bands_end);
    const size_t corr_at = disp_at + align_up(disp_bytes);
    const size_t pinned = (size_t)p.K * band_bytes;  // the K slots
    size_t d_next = 0, c_next = 0;
    for (int b = 0; b < p.B; ++b) {
        const size_t up = 2 * (size_t)f.n * p.height(b) * row_bytes;
        const size_t dev_at = (size_t)b * band_bytes, slot_at = (size_t)(b % p.K) * band_bytes;
        CHECK(up <= band_bytes && dev_at + up <= bands_end && bands_end <= disp_at &&
                  slot_at + up <= pinned,
              "%dx%dx%d band %d: %zu bytes do not fit their band", f.n, f.rows, f.cols, b, up);
        Span part[2];
        const int copies = upload_parts(up, streams, part);
        for (int i = 0; i < copies; ++i) {
            CHECK(inside(dev_at, part[i], dev_at, dev_at + up),
                  "%dx%dx%d d%d band %d copy %d: device [%zu, +%zu) leaves [%zu, %zu)", f.n, f.rows,
                  f.cols, f.depth, b, i, dev_at + part[i].offset, part[i].length, dev_at,
                  dev_at + up);
            CHECK(inside(slot_at, part[i], slot_at, slot_at + up),
                  "%dx%dx%d d%d band %d copy %d: host [%zu, +%zu) leaves its slot [%zu, %zu)", f.n,
                  f.rows, f.cols, f.depth, b, i, slot_at + part[i].offset, part[i].length, slot_at,
                  slot_at + up);
        }
        // the downloads: band by band, or the whole map at once -- the bands tile each map
        const Span d = map_rows(p.first_row(b), p.height(b), f.cols, dsz);
        CHECK(d.offset == d_next && inside(disp_at, d, disp_at, disp_at + disp_bytes),
              "%dx%dx%d band %d: disparity rows [%zu, +%zu) of %zu", f.n, f.rows, f.cols, b,
              d.offset, d.length, disp_bytes);
        d_next = d.offset + d.length;
        for (int i = 0; i < DELIVER_PARTS; ++i) {
            const Span s = deliver_part(d.length, DELIVER_PARTS, i);
            CHECK(inside(d.offset, s, d.offset, d.offset + d.length), "%dx%dx%d band %d part %d",
                  f.n, f.rows, f.cols, b, i);
        }
        if (!nxcorr) continue;
        const Span c = map_rows(p.first_row(b), p.height(b), f.cols, csz);
        CHECK(c.offset == c_next && inside(corr_at, c, corr_at, corr_at + corr_bytes),
              "%dx%dx%d band %d: corrmap rows [%zu, +%zu) of %zu", f.n, f.rows, f.cols, b,
              c.offset, c.length, corr_bytes);
        c_next = c.offset + c.length;
        for (int i = 0; i < DELIVER_PARTS; ++i) {
            const Span s = deliver_part(c.length, DELIVER_PARTS, i);
            CHECK(inside(c.offset, s, c.offset, c.offset + c.length), "%dx%dx%d band %d part %d",
                  f.n, f.rows, f.cols, b, i);
        }
    }
    CHECK(d_next == disp_bytes && c_next == corr_bytes, "%dx%dx%d: the bands' rows end at %zu / %zu",
          f.n, f.rows, f.cols, d_next, c_next);
}

static int check_layout() {
    int count = 0;
    for (const Frame& f : FRAMES)
        for (int streams = 1; streams <= 2; ++streams) {
            check_layout_of(f, false, false, streams);
            check_layout_of(f, true, false, streams);
            check_layout_of(f, true, true, streams);
            count += 3;
        }
    return count;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "parent")) {
        report_parent();
        report_parent_delivery();
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "frames")) {
        for (const Frame& f : FRAMES) std::printf("%d %d %d %d\n", f.n, f.rows, f.cols, f.depth);
        return 0;
    }
    if (argc > 1) g_align = std::strtoull(argv[1], nullptr, 10);
    if (g_align == 0) return 2;
    int k = check_bands();
    if (!failures) std::printf("bands ok %d\n", k);
    k = check_split();
    if (!failures) std::printf("split ok %d\n", k);
    k = check_delivery();
    if (!failures) std::printf("delivery ok %d\n", k);
    k = check_layout();
    if (!failures) std::printf("layout ok %d\n", k);
    if (failures) std::printf("%d checks failed\n", failures);
    return failures ? 1 : 0;
}
