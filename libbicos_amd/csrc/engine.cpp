// engine.cpp -- host orchestration of the gfx950 BICOS hot path.
//
//   bicos_impl::match_device   <- reference match_impl (src/impl/cpu.cpp:35-98)
//
// The host-buffer pipeline is host.cpp, the C-ABI entries entries.cpp / multi.cpp, the C++
// API cxxapi.cpp (engine.hpp).
#include "engine.hpp"
#include "reproject.hpp"
#include "speckle.hpp"
#include "median.hpp"
#include "normals.hpp"
#include "mesh.hpp"
#include "project.hpp"
#include "guide.hpp"
#include "pool.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>

namespace bicos_impl {

namespace {
thread_local std::string g_last_error;
}  // namespace

void set_error(int code, const std::string& msg) {
    (void)code;
    g_last_error = msg;
}

int fail(int code, const std::string& msg) {
    set_error(code, msg);
    return code;
}

int check_hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return BICOS_OK;
    std::ostringstream os;
    os << what << ": " << hipGetErrorName(e) << " (" << hipGetErrorString(e) << ")";
    return fail(BICOS_E_HIP, os.str());
}

const char* last_error() { return g_last_error.c_str(); }

int check_stack_shape(int n, int depth, int rows, int cols) {
    if (n < 2) return fail(BICOS_E_ARG, "need at least two images");
    if (depth != 1 && depth != 2)
        return fail(BICOS_E_ARG, "bad input depths, only CV_8UC1 and CV_16UC1 are supported");
    if (rows < 0 || cols < 0) return fail(BICOS_E_ARG, "negative image size");
    return BICOS_OK;
}

int reserve(void*& buf, size_t& have, size_t bytes, int device, hipStream_t st,
            hipEvent_t ready) {
    if (bytes <= have && buf) return BICOS_OK;
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != device) (void)hipSetDevice(device);
    int rc = BICOS_OK;
    if (buf) {
        // Stream-ordered: every earlier use of the old buffer, on any stream, is ordered
        // before `ready` (recorded after each use), so `st` waits for it and frees the old
        // buffer in its own order -- no device-wide synchronisation, nothing else stalls.
        rc = check_hip(hipStreamWaitEvent(st, ready, 0), "hipStreamWaitEvent");
        if (!rc) rc = check_hip(hipFreeAsync(buf, st), "hipFreeAsync(workspace)");
        buf = nullptr;
        have = 0;
    }
    const size_t want = bytes + bytes / 8;  // headroom for slightly larger calls
    if (!rc) rc = check_hip(hipMallocAsync(&buf, want, st), "hipMallocAsync(workspace)");
    if (cur != device) (void)hipSetDevice(cur);
    if (rc != BICOS_OK) {
        buf = nullptr;
        return rc;
    }
    have = want;
    return BICOS_OK;
}

int Lease::acquire() {
    int rc = reserve(buf_, have_, off_, e_->device, st_, e_->ws_ready);
    // order against earlier users of the buffer on other streams
    if (!rc) rc = check_hip(hipStreamWaitEvent(st_, e_->ws_ready, 0), "hipStreamWaitEvent");
    if (rc) return rc;
    held_ = true;
    off_ = 0;
    return BICOS_OK;
}

void Lease::release() {
    if (held_) (void)hipEventRecord(e_->ws_ready, st_);
    held_ = false;
}

// ------------------------------------------------------------ engine resources

int grow_pinned(PinnedBuf& b, size_t bytes, const char* what) {
    if (b.bytes >= bytes) return BICOS_OK;
    if (b.p) (void)hipHostFree(b.p);
    b = PinnedBuf{};
    const int rc = check_hip(hipHostMalloc(&b.p, bytes, hipHostMallocDefault), what);
    if (rc)
        b.p = nullptr;
    else
        b.bytes = bytes;
    return rc;
}

int grow_events(std::vector<hipEvent_t>& v, int count) {
    while ((int)v.size() < count) {
        hipEvent_t ev;
        if (int rc = check_hip(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate"))
            return rc;
        v.push_back(ev);
    }
    return BICOS_OK;
}

int ensure_stream(hipStream_t& s) {
    if (s) return BICOS_OK;
    return check_hip(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
}

void free_resources(bicos_engine* e) {
    for (PinnedBuf* b : {&e->pinned, &e->gather_pinned, &e->pinned_out})
        if (b->p) (void)hipHostFree(b->p);
    for (auto* v : {&e->events, &e->gather_events, &e->dl_events, &e->events2})
        for (hipEvent_t ev : *v) (void)hipEventDestroy(ev);
    e->pool.reset();
    for (hipStream_t s : {e->dl_stream, e->copy_stream2, e->own_stream, e->copy_stream})
        if (s) (void)hipStreamDestroy(s);
    if (e->ws_ready) (void)hipEventDestroy(e->ws_ready);
}

// ------------------------------------------------------- shapes and geometries

// reference src/impl/cpu.cpp:122-156
int descriptor_words(int n, int mode) {
    const long bits = mode ? (long)n * n - 2L * n + 3 : 4L * n - 7;
    if (bits <= 32) return 1;
    if (bits <= 64) return 2;
    if (bits <= 128) return 4;
    if (bits <= 256) return 8;
    return BICOS_E_BITS;
}

static bicos_hip::SearchGeometry geometry(const bicos_engine* e, int rows, int cols, int words) {
    int max_lds = e ? e->max_lds : 64 * 1024;
    // Row stage budget per workgroup (BICOS_SEARCH_STAGE_KIB, default 40; 0 = whole rows up
    // to 64 KiB): wider rows are split into equal chunks under it, so 4 workgroups (8 waves
    // per SIMD) stay resident per CU. Measured: 3840-column rows (cfg5) search -2.6 %,
    // 256-bit 2048-column rows -1.3 %; rows that fit (cfg2: 32 KiB) are unchanged.
    static const int stage_kib = [] {
        const char* v = std::getenv("BICOS_SEARCH_STAGE_KIB");
        return v ? std::atoi(v) : 40;
    }();
    if (stage_kib > 0) {
        const int budget = stage_kib * 1024;
        const int bytes = cols * words * 4;
        if (bytes > budget) {
            const int chunks = (bytes + budget - 1) / budget;
            const int chunk = (cols + chunks - 1) / chunks;
            max_lds = std::min(max_lds, chunk * words * 4);
        }
    }
    // (an engine tuned for the matrix-core search runs VALU kernels untuned)
    if (!e || e->tune_variant >= 64) return bicos_hip::search_geometry(rows, cols, words, max_lds);
    return bicos_hip::search_geometry(rows, cols, words, max_lds, e->tune_variant, e->tune_R,
                                      e->tune_waves, e->tune_split, e->cus);
}

// a switch that is on unless the environment sets it to "0"; read where it is called
static bool env_on(const char* name) {
    const char* v = std::getenv(name);
    return !(v && !std::strcmp(v, "0"));
}

// The agree inside the search launch for the shape search_mx_agree_fusable accepts
// (BICOS_FUSE_AGREE=0: the separate agree launch; read once)
static bool fuse_agree() {
    static const bool on = env_on("BICOS_FUSE_AGREE");
    return on;
}
// The right row streamed through LDS in half-chunk stages by the 128-bit NoDuplicates search
// (search_mx.hip search_mx_kernel ST; BICOS_MX_STREAM=0: the chunk loop; read once)
static bool stream_search() {
    static const bool on = env_on("BICOS_MX_STREAM");
    return on;
}
// The second K-step of the same search only for the blocks that can hold a minimum
// (search_mx.hip search_mx_kernel PRUNE; BICOS_MX_PRUNE=0: every block in full; read once)
static bool prune_search() {
    static const bool on = env_on("BICOS_MX_PRUNE");
    return on;
}
// That search's pruned main launch of 4 tiles per wave on packed keys where the descriptors'
// used bits allow (search_pk.hip search_pkp_kernel; BICOS_MX_PACKED=0: the one-product kernel;
// read once)
static bool packed_search() {
    static const bool on = env_on("BICOS_MX_PACKED");
    return on;
}
// Consistency's left-right check inside the agree launch (kernels.hip agree_lds_kernel CONS;
// BICOS_FUSE_CONS=0: consistency_kernel + the agree; read once)
static bool fuse_consistency() {
    static const bool on = env_on("BICOS_FUSE_CONS");
    return on;
}

// Search implementation: the matrix-core search (search_mx.hip) unless the engine is tuned
// to the VALU search (bicos_engine_tune variant 16) or BICOS_SEARCH=valu;
// BICOS_SEARCH=mx forces it. Results are identical either way. Neither switch applies to a
// call with a disparity range: the windowed search exists on the matrix cores only
// (search_range.hip).
bool use_mx(const bicos_engine* e) {
    static const int env = [] {
        const char* v = std::getenv("BICOS_SEARCH");
        if (!v) return 0;
        if (!std::strcmp(v, "valu")) return 1;
        if (!std::strcmp(v, "mx")) return 2;
        return 0;
    }();
    if (e && e->tune_variant >= 64) return true;
    if (e && e->tune_variant != 0) return false;
    return env != 1;
}

// Highest descriptor bit the transform writes + 1 (an upper bound: LIMITED writes 4n-6 bits
// for n >= 4, 7 for n = 3 and 4 for n = 2 -- the closing four comparisons alone,
// descriptor_transform.hpp:62-68 --, FULL n^2-2n+3; descriptor_transform.hpp:31-123). The
// search multiplies only the 64-bit K-steps that hold them.
int used_bits(int n, int mode) { return mode ? n * n - 2 * n + 3 : std::max(4 * n - 5, 4); }

static bicos_hip::MxGeometry mx_geometry(const bicos_engine* e, int rows, int cols, int words,
                                         int bits) {
    const bool tuned = e && e->tune_variant >= 64;
    // tuned: split = LDS stage KiB (0 = 64)
    const int lds = tuned && e->tune_split > 0 ? e->tune_split * 1024 : 64 * 1024;
    bicos_hip::MxGeometry g = bicos_hip::search_mx_geometry(
        rows, cols, words, lds, tuned ? e->tune_R : 0, tuned ? e->tune_waves : 0, e ? e->cus : 256,
        tuned ? e->tune_variant - 64 : 0, bits);
    g.stream = stream_search() ? 1 : 0;
    g.prune = prune_search() ? 1 : 0;
    if (!packed_search()) g.packed = 0;
    return g;
}

// Whether the NoDuplicates search of rows x cols descriptors of `words` words with `bits` used
// bits (0: unknown) -- fused: inside the fused search + agree launch of a stack of n images --
// runs its main launch on packed keys (bicos_search_packed, bicos_c.h)
bool search_runs_packed(const bicos_engine* e, int rows, int cols, int words, int bits, int n,
                        bool fused) {
    if (rows <= 0 || cols <= 0 || !use_mx(e)) return false;
    const bicos_hip::MxGeometry g = mx_geometry(e, rows, cols, words, bits);
    if (fused && !fuse_agree()) return false;
    return bicos_hip::search_mx_packed(g, rows, cols, words, fused ? n : 0);
}

// Number of x the reference's subpixel loop visits: for (float x = -1.f; x <= 1.f; x += step)
// (agree.hpp:122 / agree.cuh:213), accumulated in float exactly as there. 0 when the loop
// would exceed MAX_SUBPIXEL_STEPS (or never end: x + step == x), which the reference would
// run for hours on a CPU and which on a GPU is a hung device; such steps are rejected.
constexpr int MAX_SUBPIXEL_STEPS = 65536;
int subpixel_steps(float step) {
    int count = 0;
    for (float x = -1.f; x <= 1.f; x += step)
        if (++count > MAX_SUBPIXEL_STEPS) return 0;
    return count;
}

int check_range(int min_disparity, int max_disparity) {
    if (min_disparity <= max_disparity) return BICOS_OK;
    std::ostringstream os;
    os << "disparity range: min_disparity " << min_disparity << " exceeds max_disparity "
       << max_disparity;
    return fail(BICOS_E_ARG, os.str());
}

int check_guide(const void* guide, size_t guide_pitch, int cols, int min_disparity,
                int max_disparity) {
    if (int rc0 = check_range(min_disparity, max_disparity)) return rc0;
    if (!guide) return fail(BICOS_E_ARG, "disparity guide: null guide");
    if (cols > 0 && guide_pitch < (size_t)cols) {
        std::ostringstream os;
        os << "disparity guide: guide_pitch " << guide_pitch << " is smaller than cols " << cols;
        return fail(BICOS_E_ARG, os.str());
    }
    if ((uintptr_t)guide & 3u)
        return fail(BICOS_E_ARG, "disparity guide: the guide's base is not 4-byte aligned");
    return BICOS_OK;
}

static int required_bits(int n, int mode) { return mode ? n * n - 2 * n + 3 : 4 * n - 7; }

// Consistency's reverse search (reference bicos.hpp:94-106, bicos.cuh:110-135): rev[col1] is
// read only for the col1 a valid forward match chose, so the matrix-core search runs only
// over those -- per row the distinct valid fwd[col0] in ascending order, which each
// workgroup of the compacted search finds itself (search_dev.hpp list_prologue); rev
// elsewhere is left unwritten and never read. Periodic inputs whose forward search keeps
// nothing skip the reverse pass almost entirely. BICOS_REV_FULL=1 (A/B) and the VALU search
// run the full reverse pass (run_search: keep = nullptr).
static bool reverse_compacted(bool mx) {
    static const bool full = [] {
        const char* v = std::getenv("BICOS_REV_FULL");
        return v && std::atoi(v) != 0;
    }();
    return mx && !full;
}

// Consistency's dense-row fast path (SearchArgs.row_valid, search_dev.hpp dense_row): the
// forward search counts its valid col0 per 32-column tile and the compacted reverse search
// skips its entry prologue on rows that kept >= 7/8 of them. BICOS_DENSE_ROWS=0: off (A/B).
static bool dense_rows() {
    static const bool on = env_on("BICOS_DENSE_ROWS");
    return on;
}
// Consistency without NoDuplicates in one launch where the descriptors allow it (search_lr.hip
// search_lr_kernel: the forward and reverse searches share their matrix products, the check
// runs in the same workgroup). BICOS_LR_ONE_PASS=0: the two searches + the check (A/B; read
// per call, so one process can compare the two forms).
static bool lr_one_pass() { return env_on("BICOS_LR_ONE_PASS"); }
// Descriptor bits the transform writes, exactly (descriptor_transform.hpp:31-123; used_bits
// is an upper bound): LIMITED 4n-6 for n >= 4 (7 for n = 3, 4 for n = 2), FULL n^2-2n+3
static int written_bits(int n, int mode) {
    if (mode) return n * n - 2 * n + 3;
    return n >= 4 ? 4 * n - 6 : (n == 3 ? 7 : 4);
}
// bytes per row of the per-tile valid counts
static size_t valid_pitch(int cols) { return ((size_t)(cols + 31) / 32 + 15) / 16 * 16; }

int stack_span(int n, int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
               uint32_t* out) {
    if (rows <= 0 || cols <= 0) {
        *out = 0;
        return BICOS_OK;
    }
    const unsigned long long span =
        ((unsigned long long)(n - 1) * plane_pitch + (unsigned long long)(rows - 1) * row_pitch +
         (unsigned long long)cols) * (unsigned long long)depth;
    if (span > 0xFFFFFFFFull) return fail(BICOS_E_ARG, "image stack spans more than 4 GiB");
    *out = (uint32_t)span;
    return BICOS_OK;
}

// ------------------------------------------------------------------- the plans

SearchPlan search_plan(const bicos_engine* e, int rows, int cols, int words, int used_bits,
                       int written_bits, bool nodupes, bool consistency, bool ranged) {
    SearchPlan p;
    p.two_pass = consistency;
    if (ranged) {
        // the windowed search (search_range.hip) and separate launches: the fused and
        // compacted plans are specialised to the full-row kernels' shapes
        p.bits = BICOS_PLAN_MATRIX_CORES;
        return p;
    }
    const bool mx = use_mx(e);
    if (mx) {
        p.bits |= BICOS_PLAN_MATRIX_CORES;
        p.mx = mx_geometry(e, rows, cols, words, used_bits);
        if (p.mx.pk && nodupes) p.bits |= BICOS_PLAN_PACKED_KEYS;
    }
    if (consistency && mx && !nodupes && lr_one_pass() &&
        bicos_hip::search_lr_eligible(words, written_bits, cols)) {
        p.bits |= BICOS_PLAN_CONSISTENCY_ONE_PASS;
        p.two_pass = false;
    } else if (consistency && reverse_compacted(mx)) {
        p.bits |= BICOS_PLAN_REVERSE_COMPACTED;
        if (dense_rows()) p.bits |= BICOS_PLAN_DENSE_ROWS;
    }
    return p;
}

// What match_device runs for a shape and config (bicos_match_plan's bits, bicos_c.h): the
// kernels after the transform. Valid configurations only (match_device validates first).
MatchPlan match_plan(const bicos_engine* e, int n, int rows, int cols, size_t row_pitch,
                     size_t plane_pitch, int depth, const BicosConfig& cfg, bool has_nxcorr,
                     const void* s0, const void* s1, bool ranged) {
    MatchPlan plan;
    const int mode = cfg.mode == 0 ? 0 : 1;
    const int words = descriptor_words(n, mode);
    if (words < 0 || rows <= 0 || cols <= 0) return plan;
    const bool consistency = cfg.variant_type != 0;
    const bool nodupes = consistency ? cfg.no_dupes != 0 : true;
    plan.search = search_plan(e, rows, cols, words, used_bits(n, mode), written_bits(n, mode),
                              nodupes, consistency, ranged);
    // the agree's part: both fusions need the plain NXC stage over stacks the LDS-staged
    // agree kernels can read with dword loads
    const bool aligned4 = ((row_pitch * depth | plane_pitch * depth) & 3) == 0 &&
                          (((uintptr_t)s0 | (uintptr_t)s1) & 3) == 0;
    if (!has_nxcorr || cfg.subpixel_step >= 0 || !aligned4) return plan;
    if (!consistency && !ranged && (plan.search.bits & BICOS_PLAN_MATRIX_CORES) && fuse_agree() &&
        bicos_hip::search_mx_agree_fusable(plan.search.mx, words, true, cols, n, depth,
                                           cfg.precision != 0))
        plan.agree |= BICOS_PLAN_AGREE_IN_SEARCH;
    if (plan.search.two_pass && n <= 65 && fuse_consistency())
        plan.agree |= BICOS_PLAN_CONSISTENCY_IN_AGREE;
    return plan;
}

// ----------------------------------------------------------- the search stage

SearchBuffers search_buffers(Lease& ws, const SearchPlan& p, int rows, int cols) {
    SearchBuffers b;
    if (!p.two_pass) return b;
    b.fwd = ws.take<int16_t>((size_t)rows * cols);
    b.rev = ws.take<int16_t>((size_t)rows * cols);
    if (p.bits & BICOS_PLAN_DENSE_ROWS) b.valid = ws.take<uint8_t>((size_t)rows * valid_pitch(cols));
    return b;
}

// bicos search (cpu.cpp:68-75): NoDuplicates in one search; Consistency as the forward and
// the reverse search (the same search with the stacks swapped, bicos.hpp:96) over only the
// col1 the forward search kept (reverse_compacted), then the left-right check -- or all of
// it in one launch (lr_one_pass)
int run_search(const bicos_engine* e, const SearchPlan& p, const SearchBuffers& b,
               const SearchJob& j, int16_t* out, hipStream_t st,
               const bicos_hip::AgreeArgs* fused_agree) {
    const int rows = j.rows, cols = j.cols, words = j.words;
    auto args = [&](const uint32_t* a0, const uint32_t* a1, int16_t* o, int out_mode) {
        return bicos_hip::SearchArgs{a0, a1, o, rows, cols, bicos_desc_pitch(cols, words),
                                     (size_t)cols, out_mode, 0, 0, 0};
    };
    // the headline shape runs the agree inside the search's workgroups (one launch,
    // search_dev.hpp fused_agree; BICOS_FUSE_AGREE=0 keeps the two launches)
    if (fused_agree)
        return check_hip(bicos_hip::launch_search_mx_agree(args(j.d0, j.d1, out, 0), *fused_agree,
                                                           p.mx, words, st),
                         "search + agree launch");
    if (p.bits & BICOS_PLAN_CONSISTENCY_ONE_PASS)
        return check_hip(bicos_hip::launch_search_lr(args(j.d0, j.d1, out, 0), words,
                                                     j.written_bits, j.max_lr_diff, st),
                         "consistency search launch");
    // the window: bounds beyond +-cols are equivalent to +-cols (and safe to negate); the
    // reverse search swaps the roles of the columns: its window is [-max, -min]
    const int lo = j.range ? std::min(std::max(j.range->min, -cols), cols) : 0;
    const int hi = j.range ? std::min(std::max(j.range->max, -cols), cols) : 0;
    const bool tuned = e && e->tune_variant >= 64;
    auto search = [&](const bicos_hip::SearchArgs& sa, bool reverse, const char* what) {
        // the guide holds windows of the LEFT pixels: the forward search alone reads it
        if (j.range && j.range->guide && !reverse)
            return check_hip(bicos_hip::launch_search_guided(
                                 sa, lo, hi, j.range->guide, j.range->guide_pitch, words,
                                 j.nodupes, j.used_bits, e ? e->cus : 256, st,
                                 tuned ? e->tune_R : 0, tuned ? e->tune_waves : 0),
                             what);
        if (j.range)
            return check_hip(bicos_hip::launch_search_range(
                                 sa, reverse ? -hi : lo, reverse ? -lo : hi, words, j.nodupes,
                                 j.used_bits, e ? e->cus : 256, st, tuned ? e->tune_R : 0,
                                 tuned ? e->tune_waves : 0),
                             what);
        if (p.bits & BICOS_PLAN_MATRIX_CORES)
            return check_hip(bicos_hip::launch_search_mx(sa, p.mx, words, j.nodupes, st), what);
        return check_hip(bicos_hip::launch_search(sa, geometry(e, rows, cols, words), words,
                                                  j.nodupes, st),
                         what);
    };
    if (!p.two_pass) return search(args(j.d0, j.d1, out, 0), false, "search launch");

    bicos_hip::SearchArgs fa = args(j.d0, j.d1, b.fwd, 1), ra = args(j.d1, j.d0, b.rev, 1);
    fa.row_valid = ra.row_valid = b.valid;  // dense-row fast path
    fa.valid_pitch = ra.valid_pitch = valid_pitch(cols);
    if (p.bits & BICOS_PLAN_REVERSE_COMPACTED) {
        ra.keep = b.fwd;
        ra.keep_pitch = (size_t)cols;
    }
    int rc = search(fa, false, "search launch");
    if (!rc) rc = search(ra, true, "reverse search launch");
    if (rc || !out) return rc;
    bicos_hip::ConsistencyArgs ca{b.fwd, b.rev, out, rows, cols, (size_t)cols, j.max_lr_diff};
    return check_hip(bicos_hip::launch_consistency(ca, st), "consistency launch");
}

bicos_hip::AgreeArgs agree_args(const int16_t* raw, const void* s0, const void* s1, int n,
                                int rows, int cols, size_t row_pitch, size_t plane_pitch,
                                uint32_t span, float threshold, float step, int nsteps,
                                int has_minvar, float minvar_scaled, void* out, bool out_f32,
                                void* corr) {
    // (kernels.hpp AgreeArgs in its order; fwd / rev / max_lr_diff stay null / 0)
    return bicos_hip::AgreeArgs{raw, (size_t)cols, s0, s1, n, rows, cols, row_pitch, plane_pitch,
                                threshold, step, nsteps, has_minvar, minvar_scaled, out,
                                out_f32 ? 1 : 0, corr, span};
}

int check_match(const void* s0, const void* s1, int n, int rows, int cols, size_t row_pitch,
                size_t plane_pitch, int depth, const BicosConfig& cfg, bool has_nxcorr,
                const void* disp, bool disp_i16, MatchShape* out) {
    *out = MatchShape{};
    if (int rc0 = check_stack_shape(n, depth, rows, cols)) return rc0;
    if (cols > 32767)
        return fail(BICOS_E_ARG, "image width exceeds the int16 disparity range (32767)");
    const int mode = cfg.mode == 0 ? 0 : 1;
    const int words = descriptor_words(n, mode);
    if (words < 0) {
        std::ostringstream os;
        os << "input stacks too large, would require " << required_bits(n, mode) << " bits";
        return fail(BICOS_E_BITS, os.str());
    }
    const bool has_step = has_nxcorr && cfg.subpixel_step >= 0;
    if (has_step && !(cfg.subpixel_step > 0 && std::isfinite(cfg.subpixel_step)))
        return fail(BICOS_E_ARG, "subpixel_step must be a positive finite number");
    const int nsteps = has_step ? subpixel_steps(cfg.subpixel_step) : 0;
    if (has_step && !nsteps)
        return fail(BICOS_E_ARG, "subpixel_step too small (more than 65536 interpolation steps)");
    if (disp_i16 && has_step)
        return fail(BICOS_E_ARG, "an int16 disparity map cannot hold subpixel disparities");
    *out = MatchShape{mode, words, has_step, nsteps, 0};
    if (rows == 0 || cols == 0) return BICOS_OK;
    if (!s0 || !s1 || !disp) return fail(BICOS_E_ARG, "null buffer");
    if (row_pitch < (size_t)cols || plane_pitch < (size_t)rows * row_pitch)
        return fail(BICOS_E_ARG, "row/plane pitch smaller than the image");
    return stack_span(n, rows, cols, row_pitch, plane_pitch, depth, &out->span);
}

int match_device(bicos_engine* e, const void* s0, const void* s1, int n, int rows, int cols,
                 size_t row_pitch, size_t plane_pitch, int depth, const BicosConfig& cfg,
                 bool has_nxcorr, float threshold, void* disp, void* corr, hipStream_t st,
                 bool disp_i16, const uint32_t* ext_d0, const uint32_t* ext_d1,
                 const DispRange* range) {
    if (range)
        if (int rc0 = check_range(range->min, range->max)) return rc0;
    if (range && range->guide)
        if (int rc0 = check_guide(range->guide, range->guide_pitch, cols, range->min, range->max))
            return rc0;
    if (!e) return fail(BICOS_E_ARG, "null engine");
    MatchShape shape;
    if (int rc0 = check_match(s0, s1, n, rows, cols, row_pitch, plane_pitch, depth, cfg, has_nxcorr,
                              disp, disp_i16, &shape))
        return rc0;
    if (rows == 0 || cols == 0) return BICOS_OK;
    const int mode = shape.mode, words = shape.words, nsteps = shape.nsteps;
    const bool has_step = shape.has_step;
    const uint32_t span = shape.span;

    const bool consistency = cfg.variant_type != 0;
    const bool dbl = cfg.precision != 0;
    const MatchPlan plan = match_plan(e, n, rows, cols, row_pitch, plane_pitch, depth, cfg,
                                      has_nxcorr, s0, s1, range != nullptr);
    const bool ext = ext_d0 != nullptr;
    if (ext != (ext_d1 != nullptr)) return fail(BICOS_E_ARG, "need both descriptor buffers");

    // workspace: desc0 | desc1 | raw int16 | the search's maps (Consistency); the descriptors
    // are the caller's when given (bicos_search_agree_device: the match past its transform)
    const size_t dpitch = bicos_desc_pitch(cols, words);
    const uint32_t *d0 = ext_d0, *d1 = ext_d1;
    int16_t* raw = (int16_t*)disp;
    SearchBuffers maps;
    Lease ws(e, e->ws, e->ws_bytes, st);
    auto carve = [&] {
        if (!ext) {
            d0 = ws.take<uint32_t>((size_t)rows * dpitch);
            d1 = ws.take<uint32_t>((size_t)rows * dpitch);
        }
        if (has_nxcorr) raw = ws.take<int16_t>((size_t)rows * cols);
        maps = search_buffers(ws, plan.search, rows, cols);
    };
    carve();
    int rc = ws.acquire();
    if (rc) return rc;
    carve();

    // 1. descriptor_transform, both stacks in one launch (cpu.cpp:50-59)
    if (!ext) {
        bicos_hip::TransformArgs ta{s0, s1, (uint32_t*)d0, (uint32_t*)d1, n, rows, cols,
                                    row_pitch, plane_pitch, dpitch, 0, span};
        rc = check_hip(bicos_hip::launch_transform(ta, depth, mode, words, st), "transform launch");
        if (rc) return rc;
    }

    // 2. the search (run_search); 3. agree / agree_subpixel (cpu.cpp:77-95), inside the
    // search launch or with Consistency's check inside it where the plan says so
    bicos_hip::AgreeArgs aa = agree_args(
        raw, s0, s1, n, rows, cols, row_pitch, plane_pitch, span, threshold,
        has_step ? cfg.subpixel_step : 0.f, nsteps, cfg.min_variance >= 0,
        cfg.min_variance >= 0 ? cfg.min_variance * (float)n : 0.f, disp, !disp_i16, corr);
    const bool check_in_agree = (plan.agree & BICOS_PLAN_CONSISTENCY_IN_AGREE) != 0;
    const SearchJob job{d0, d1, rows, cols, words, used_bits(n, mode), written_bits(n, mode),
                        consistency ? cfg.no_dupes != 0 : true, cfg.max_lr_diff, range};
    const bool fused = (plan.agree & BICOS_PLAN_AGREE_IN_SEARCH) != 0;
    rc = run_search(e, plan.search, maps, job, check_in_agree ? nullptr : raw, st,
                    fused ? &aa : nullptr);
    if (rc || fused || !has_nxcorr) return rc;
    if (check_in_agree) {
        // the left-right check runs inside the agree (kernels.hip agree_lds_kernel CONS)
        aa.fwd = maps.fwd;
        aa.rev = maps.rev;
        aa.max_lr_diff = cfg.max_lr_diff;
        return check_hip(bicos_hip::launch_agree(aa, depth, dbl, st), "consistency + agree launch");
    }
    if (has_step) return check_hip(bicos_hip::launch_subpixel(aa, depth, dbl, st), "subpixel launch");
    return check_hip(bicos_hip::launch_agree(aa, depth, dbl, st), "agree launch");
}

// ------------------------------------------- what the map stages check alike

namespace {
// "<stage>: the <what> must be CV_16S or CV_32F"
int check_map_type(const char* stage, int type, const char* what = "disparity map") {
    if (type == BICOS_CV_16S || type == BICOS_CV_32F) return BICOS_OK;
    return fail(BICOS_E_ARG, std::string(stage) + ": the " + what + " must be CV_16S or CV_32F");
}

// "<stage>: negative image size", then "<stage>: rows * cols exceeds int32"
int check_map_size(const char* stage, int rows, int cols) {
    if (rows < 0 || cols < 0)
        return fail(BICOS_E_ARG, std::string(stage) + ": negative image size");
    if ((int64_t)rows * cols > INT32_MAX)
        return fail(BICOS_E_ARG, std::string(stage) + ": rows * cols exceeds int32");
    return BICOS_OK;
}

// whether [p, p + n) and [q, q + m) share a byte; a null pointer or an empty span shares none
bool overlaps(const void* p, uintptr_t n, const void* q, uintptr_t m) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a && b && n && m && a < b + m && b < a + n;
}

// no pixels, nothing to launch: the `n` counts (if asked for) are all zero
int zero_counts(uint32_t* counts, size_t n, hipStream_t st,
                const char* what = "hipMemsetAsync(counts)") {
    return counts ? check_hip(hipMemsetAsync(counts, 0, n * sizeof(uint32_t), st), what)
                  : (int)BICOS_OK;
}
}  // namespace

// -------------------------------------------------------------- reprojection

int check_reproject(const ReprojectJob& j, const bicos_engine* e, bool needs_engine) {
    if (int rc0 = check_map_type("reproject", j.disp_type)) return rc0;
    if (int rc0 = check_map_size("reproject", j.rows, j.cols)) return rc0;
    if (j.flags & ~(BICOS_REPROJECT_ALLOW_NEGATIVE_Z | BICOS_REPROJECT_F32_SENTINEL))
        return fail(BICOS_E_ARG, "reproject: unknown flag bits");
    if (!j.xyz_map && !j.points)
        return fail(BICOS_E_ARG, "reproject: no output (xyz_map and points both null)");
    if (j.points && !j.counts) return fail(BICOS_E_ARG, "reproject: points need counts");
    if (j.index && !j.points) return fail(BICOS_E_ARG, "reproject: index without points");
    if (j.points && needs_engine && !e)
        return fail(BICOS_E_ARG, "reproject: points need an engine workspace");
    if (!j.Q) return fail(BICOS_E_ARG, "reproject: null Q");
    if (j.rows > 0 && j.cols > 0 && !j.disp) return fail(BICOS_E_ARG, "reproject: null disparity map");
    return BICOS_OK;
}

int reproject_device(bicos_engine* e, const ReprojectJob& j, hipStream_t st) {
    const uint32_t pixels = (uint32_t)j.rows * (uint32_t)j.cols;
    if (pixels == 0) return zero_counts(j.points ? j.counts : nullptr, 4, st);
    bicos_hip::ReprojectArgs a{};
    a.disp = j.disp;
    a.cols = j.cols;
    a.pixels = pixels;
    a.flags = j.flags;
    std::copy(j.Q, j.Q + 16, a.Q.q);
    a.xyz_map = j.xyz_map;
    a.points = j.points;
    a.index = j.index;
    a.capacity = (uint32_t)std::min<size_t>(j.capacity, pixels);
    a.counts = j.counts;
    const bool f32 = j.disp_type == BICOS_CV_32F;
    if (!j.points)
        return check_hip(bicos_hip::launch_reproject_map(a, f32, st), "reproject launch");
    const uint32_t segments = bicos_hip::reproject_segments(pixels);
    Lease ws(e, e->ws, e->ws_bytes, st);
    auto carve = [&] {
        a.seg_counts = ws.take<uint32_t>((size_t)segments * 4);
        a.seg_offsets = ws.take<uint32_t>(segments);
    };
    carve();
    if (int rc = ws.acquire()) return rc;
    carve();
    return check_hip(bicos_hip::launch_reproject_points(a, f32, st), "reproject launches");
}

// ------------------------------------------------------------ speckle filter

int check_speckle(const SpeckleJob& j, const bicos_engine* e, bool needs_engine) {
    if (int rc0 = check_map_type("speckle", j.disp_type)) return rc0;
    if (int rc0 = check_map_size("speckle", j.rows, j.cols)) return rc0;
    if (j.flags & ~BICOS_SPECKLE_F32_SENTINEL)
        return fail(BICOS_E_ARG, "speckle: unknown flag bits");
    if (!(j.max_diff >= 0.0f))
        return fail(BICOS_E_ARG, "speckle: max_diff must be >= 0 and not NaN");
    if (j.max_size < 0) return fail(BICOS_E_ARG, "speckle: negative max_size");
    if (needs_engine && !e) return fail(BICOS_E_ARG, "speckle: null engine (workspace)");
    if (j.rows > 0 && j.cols > 0) {
        if (!j.disp) return fail(BICOS_E_ARG, "speckle: null disparity map");
        if (!j.out) return fail(BICOS_E_ARG, "speckle: null out");
        const uintptr_t bytes = (uintptr_t)j.rows * j.cols * (j.disp_type == BICOS_CV_32F ? 4 : 2);
        if (j.out != j.disp && overlaps(j.out, bytes, j.disp, bytes))
            return fail(BICOS_E_ARG, "speckle: out overlaps the map partially (in place: out == map)");
    }
    return BICOS_OK;
}

int speckle_device(bicos_engine* e, const SpeckleJob& j, hipStream_t st) {
    const size_t pixels = (size_t)j.rows * j.cols;
    if (pixels == 0) return zero_counts(j.counts, 4, st);
    bicos_hip::SpeckleArgs a{};
    a.disp = j.disp;
    a.out = j.out;
    a.rows = j.rows;
    a.cols = j.cols;
    a.max_size = (uint32_t)j.max_size;
    a.max_diff = j.max_diff;
    a.flags = j.flags;
    a.counts = j.counts;
    a.final_labels = j.labels != nullptr;
    Lease ws(e, e->ws, e->ws_bytes, st);
    auto carve = [&] {
        a.sizes = ws.take<uint32_t>(pixels);
        a.labels = j.labels ? j.labels : ws.take<int32_t>(pixels);
    };
    carve();
    if (int rc = ws.acquire()) return rc;
    carve();
    return check_hip(bicos_hip::launch_speckle(a, j.disp_type == BICOS_CV_32F, st),
                     "speckle launches");
}

// ------------------------------------------------------------- median filter

int check_median(const MedianJob& j, bool device) {
    if (int rc0 = check_map_type("median", j.disp_type)) return rc0;
    if (j.ksize != 3 && j.ksize != 5) return fail(BICOS_E_ARG, "median: ksize must be 3 or 5");
    if (j.fill_min < 0 || j.fill_min > j.ksize * j.ksize)
        return fail(BICOS_E_ARG, "median: fill_min must lie in 0 .. ksize * ksize");
    if (j.flags & ~BICOS_MEDIAN_F32_SENTINEL)
        return fail(BICOS_E_ARG, "median: unknown flag bits");
    if (int rc0 = check_map_size("median", j.rows, j.cols)) return rc0;
    if (j.rows > 0 && j.cols > 0) {
        if (!j.disp) return fail(BICOS_E_ARG, "median: null disparity map");
        if (!j.out) return fail(BICOS_E_ARG, "median: null out");
        const uintptr_t bytes = (uintptr_t)j.rows * j.cols * (j.disp_type == BICOS_CV_32F ? 4 : 2);
        if (device && overlaps(j.out, bytes, j.disp, bytes))
            return fail(BICOS_E_ARG, "median: out overlaps the map (the filter reads neighbours)");
    }
    return BICOS_OK;
}

int median_device(const MedianJob& j, hipStream_t st) {
    if ((size_t)j.rows * j.cols == 0) return zero_counts(j.counts, 4, st);
    bicos_hip::MedianArgs a{};
    a.disp = j.disp;
    a.out = j.out;
    a.rows = j.rows;
    a.cols = j.cols;
    a.fill_min = j.fill_min;
    a.flags = j.flags;
    a.counts = j.counts;
    return check_hip(bicos_hip::launch_median(a, j.disp_type == BICOS_CV_32F, j.ksize, st),
                     "median launch");
}

// ----------------------------------------------------------- surface normals

int check_normals(const NormalsJob& j) {
    if (int rc0 = check_map_type("normals", j.disp_type)) return rc0;
    if (j.flags & ~(BICOS_NORMALS_ALLOW_NEGATIVE_Z | BICOS_NORMALS_F32_SENTINEL))
        return fail(BICOS_E_ARG, "normals: unknown flag bits");
    if (j.radius < 1 || j.radius > bicos_hip::NORMALS_MAX_RADIUS)
        return fail(BICOS_E_ARG, "normals: radius must lie in 1 .. 4");
    if (!(j.max_diff >= 0.0f))
        return fail(BICOS_E_ARG, "normals: max_diff must be >= 0 and not NaN");
    if (j.min_points < 3 || j.min_points > (2 * j.radius + 1) * (2 * j.radius + 1))
        return fail(BICOS_E_ARG, "normals: min_points must lie in 3 .. (2 * radius + 1)^2");
    if (int rc0 = check_map_size("normals", j.rows, j.cols)) return rc0;
    if (!j.normal_map && !j.normals && !j.index)
        return fail(BICOS_E_ARG, "normals: no output (normal_map and normals both null)");
    if (j.normals && !j.index) return fail(BICOS_E_ARG, "normals: normals without index");
    if (j.index && !j.normals) return fail(BICOS_E_ARG, "normals: index without normals");
    if (j.counts && !j.normal_map)
        return fail(BICOS_E_ARG, "normals: counts need normal_map (they count over the map)");
    if (j.rows > 0 && j.cols > 0) {
        if (!j.disp) return fail(BICOS_E_ARG, "normals: null disparity map");
        if (!j.Q) return fail(BICOS_E_ARG, "normals: null Q");
        const uintptr_t pixels = (uintptr_t)j.rows * j.cols;
        const uintptr_t bytes = pixels * (j.disp_type == BICOS_CV_32F ? 4 : 2);
        if (overlaps(j.normal_map, pixels * 12, j.disp, bytes))
            return fail(BICOS_E_ARG, "normals: normal_map overlaps the map");
        if (overlaps(j.normals, (uintptr_t)j.count * 12, j.disp, bytes))
            return fail(BICOS_E_ARG, "normals: normals overlaps the map");
        if (overlaps(j.counts, 4 * sizeof(uint32_t), j.disp, bytes))
            return fail(BICOS_E_ARG, "normals: counts overlaps the map");
    }
    return BICOS_OK;
}

int normals_device(const NormalsJob& j, hipStream_t st) {
    const size_t pixels = (size_t)j.rows * j.cols;
    bicos_hip::NormalsArgs a{};
    a.disp = j.disp;
    a.rows = j.rows;
    a.cols = j.cols;
    a.flags = j.flags;
    a.radius = j.radius;
    a.max_diff = j.max_diff;
    a.min_points = j.min_points;
    if (j.Q) std::copy(j.Q, j.Q + 16, a.Q.q);  // (may be null for an empty map: nothing reads it)
    a.normal_map = j.normal_map;
    a.counts = j.counts;
    a.index = j.index;
    a.normals = j.normals;
    a.count = j.count;
    const bool f32 = j.disp_type == BICOS_CV_32F;
    if (j.normal_map) {
        if (pixels == 0) {  // no map to launch
            if (int rc = zero_counts(j.counts, 4, st)) return rc;
        } else if (int rc = check_hip(bicos_hip::launch_normals_map(a, f32, st),
                                      "normals map launch")) {
            return rc;
        }
    }
    if (j.normals && j.count > 0)
        return check_hip(bicos_hip::launch_normals_list(a, f32, st), "normals list launch");
    return BICOS_OK;
}

// ---------------------------------------------------------------------- mesh

namespace {
// quads of a rows x cols map: (rows-1) * (cols-1), 0 for a map without a second row or column
size_t mesh_quads(int rows, int cols) {
    return rows < 2 || cols < 2 ? 0 : (size_t)(rows - 1) * (size_t)(cols - 1);
}
}  // namespace

int check_mesh(const MeshJob& j, const bicos_engine* e, bool needs_engine) {
    if (int rc0 = check_map_type("mesh", j.disp_type)) return rc0;
    if (j.flags & ~(BICOS_MESH_ALLOW_NEGATIVE_Z | BICOS_MESH_F32_SENTINEL))
        return fail(BICOS_E_ARG, "mesh: unknown flag bits");
    if (!(j.max_diff >= 0.0f)) return fail(BICOS_E_ARG, "mesh: max_diff must be >= 0 and not NaN");
    if (int rc0 = check_map_size("mesh", j.rows, j.cols)) return rc0;
    if (needs_engine && !e) return fail(BICOS_E_ARG, "mesh: null engine (workspace)");
    if (j.rows == 0 || j.cols == 0) return BICOS_OK;
    if (!j.disp) return fail(BICOS_E_ARG, "mesh: null disparity map");
    if (!j.Q) return fail(BICOS_E_ARG, "mesh: null Q");
    if (!j.points) return fail(BICOS_E_ARG, "mesh: null points");
    if (!j.triangles) return fail(BICOS_E_ARG, "mesh: null triangles");
    if (!j.counts) return fail(BICOS_E_ARG, "mesh: null counts");
    if (!j.mesh_counts) return fail(BICOS_E_ARG, "mesh: null mesh_counts");
    // the map, then every output with the bytes the call may write
    const uintptr_t pixels = (uintptr_t)j.rows * j.cols;
    const uintptr_t verts = (uintptr_t)std::min<size_t>(j.vertex_capacity, pixels);
    const uintptr_t tris =
        (uintptr_t)std::min<size_t>(j.tri_capacity, 2 * mesh_quads(j.rows, j.cols));
    const struct {
        const void* p;
        uintptr_t bytes;
        const char* name;
    } span[] = {{j.disp, pixels * (j.disp_type == BICOS_CV_32F ? 4 : 2), "the map"},
                {j.points, verts * 12, "points"},
                {j.index, verts * 4, "index"},
                {j.counts, 16, "counts"},
                {j.triangles, tris * 12, "triangles"},
                {j.mesh_counts, 16, "mesh_counts"},
                {j.vertex_map, pixels * 4, "vertex_map"}};
    const int n = (int)(sizeof span / sizeof span[0]);
    for (int i = 1; i < n; ++i)
        for (int k = 0; k < i; ++k)
            if (overlaps(span[i].p, span[i].bytes, span[k].p, span[k].bytes))
                return fail(BICOS_E_ARG, std::string("mesh: ") + span[i].name + " overlaps " +
                                             span[k].name);
    return BICOS_OK;
}

int mesh_device(bicos_engine* e, const MeshJob& j, hipStream_t st) {
    const uint32_t pixels = (uint32_t)j.rows * (uint32_t)j.cols;
    if (pixels == 0) {
        if (int rc = zero_counts(j.counts, 4, st)) return rc;
        return zero_counts(j.mesh_counts, 4, st, "hipMemsetAsync(mesh_counts)");
    }
    bicos_hip::MeshArgs a{};
    a.v.disp = j.disp;
    a.v.cols = j.cols;
    a.v.pixels = pixels;
    a.v.flags = j.flags;  // (the BICOS_MESH_* flags are the BICOS_REPROJECT_* flags)
    std::copy(j.Q, j.Q + 16, a.v.Q.q);
    a.v.points = j.points;
    a.v.index = j.index;
    a.v.capacity = (uint32_t)std::min<size_t>(j.vertex_capacity, pixels);
    a.v.counts = j.counts;
    a.rows = j.rows;
    a.max_diff = j.max_diff;
    a.triangles = j.triangles;
    a.tri_capacity = (uint32_t)std::min<size_t>(j.tri_capacity, 2 * mesh_quads(j.rows, j.cols));
    a.mesh_counts = j.mesh_counts;
    const uint32_t segments = bicos_hip::reproject_segments(pixels);
    Lease ws(e, e->ws, e->ws_bytes, st);
    auto carve = [&] {
        a.v.seg_counts = ws.take<uint32_t>((size_t)segments * 4);
        a.v.seg_offsets = ws.take<uint32_t>(segments);
        a.tri_counts = ws.take<uint32_t>((size_t)segments * 4);
        a.tri_offsets = ws.take<uint32_t>(segments);
        a.rank = j.vertex_map ? j.vertex_map : ws.take<int32_t>(pixels);
    };
    carve();
    if (int rc = ws.acquire()) return rc;
    carve();
    return check_hip(bicos_hip::launch_mesh(a, j.disp_type == BICOS_CV_32F, st), "mesh launches");
}

// ---------------------------------------------------------------- projection

int check_project(const ProjectJob& j, const bicos_engine* e, bool needs_engine) {
    if (!j.uv && !j.depth && !j.cls && !j.tex && !j.depth_map && !j.index_map && !j.counts)
        return fail(BICOS_E_ARG, "project: no output");
    if (j.tex && !j.image) return fail(BICOS_E_ARG, "project: tex without image");
    if (j.image) {
        if (j.channels != 1 && j.channels != 3)
            return fail(BICOS_E_ARG, "project: channels must be 1 or 3");
        if (j.img_depth != 1 && j.img_depth != 2)
            return fail(BICOS_E_ARG, "project: img_depth must be 1 (u8) or 2 (u16)");
    }
    if (j.nd != 0 && j.nd != 4 && j.nd != 5 && j.nd != 8)
        return fail(BICOS_E_ARG, "project: nd must be 0, 4, 5 or 8");
    if (j.splat < 0 || j.splat > BICOS_PROJECT_MAX_SPLAT)
        return fail(BICOS_E_ARG, "project: splat must be 0 .. 3");
    if (!(j.tol >= 0.0f)) return fail(BICOS_E_ARG, "project: tol must be >= 0 and not NaN");
    if (j.image && (j.fill < 0 || j.fill > (j.img_depth == 1 ? 255 : 65535)))
        return fail(BICOS_E_ARG, "project: fill out of the image type's range");
    if (int rc0 = check_map_size("project", j.img_rows, j.img_cols)) return rc0;
    if (j.image && j.img_pitch < (size_t)j.img_cols * j.channels)
        return fail(BICOS_E_ARG, "project: img_pitch is shorter than a row");
    if (j.count > (size_t)INT32_MAX) return fail(BICOS_E_ARG, "project: count exceeds int32");
    if (j.count > 0 && !j.points) return fail(BICOS_E_ARG, "project: null points");
    if (j.count > 0 && !j.K) return fail(BICOS_E_ARG, "project: null K");
    if (j.nd > 0 && !j.D) return fail(BICOS_E_ARG, "project: null D");
    bool finite = true;
    for (int i = 0; j.K && i < 9; ++i) finite = finite && std::isfinite(j.K[i]);
    for (int i = 0; i < j.nd; ++i) finite = finite && std::isfinite(j.D[i]);
    for (int i = 0; j.R && i < 9; ++i) finite = finite && std::isfinite(j.R[i]);
    for (int i = 0; j.t && i < 3; ++i) finite = finite && std::isfinite(j.t[i]);
    if (!finite) return fail(BICOS_E_ARG, "project: a camera value is not finite");
    // the inputs, then every output with the bytes the call may write
    const uintptr_t n = (uintptr_t)j.count, pixels = (uintptr_t)j.img_rows * j.img_cols;
    const uintptr_t esz = (uintptr_t)j.img_depth, ch = (uintptr_t)j.channels;
    const uintptr_t img_bytes =
        j.image && pixels ? ((uintptr_t)(j.img_rows - 1) * j.img_pitch + j.img_cols * ch) * esz : 0;
    const struct {
        const void* p;
        uintptr_t bytes;
        const char* name;
    } span[] = {{j.points, n * 12, "points"},
                {j.image, img_bytes, "image"},
                {j.uv, n * 8, "uv"},
                {j.depth, n * 4, "depth"},
                {j.cls, n, "cls"},
                {j.tex, j.image ? n * ch * esz : 0, "tex"},
                {j.depth_map, pixels * 4, "depth_map"},
                {j.index_map, pixels * 4, "index_map"},
                {j.counts, 5 * sizeof(uint32_t), "counts"}};
    const int spans = (int)(sizeof span / sizeof span[0]);
    for (int i = 2; i < spans; ++i)
        for (int k = 0; k < i; ++k)
            if (overlaps(span[i].p, span[i].bytes, span[k].p, span[k].bytes))
                return fail(BICOS_E_ARG, std::string("project: ") + span[i].name + " overlaps " +
                                             span[k].name);
    if (needs_engine && !e && j.zbuffer())
        return fail(BICOS_E_ARG, "project: null engine (the z-buffer's workspace)");
    return BICOS_OK;
}

int project_device(bicos_engine* e, const ProjectJob& j, hipStream_t st) {
    bicos_hip::ProjectArgs a{};
    static const double identity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::copy(j.R ? j.R : identity, (j.R ? j.R : identity) + 9, a.cam.R);
    for (int i = 0; i < 3; ++i) a.cam.t[i] = j.t ? j.t[i] : 0.0;
    if (j.K) {  // (NULL only with count == 0: no point kernel runs)
        a.cam.fx = j.K[0];
        a.cam.cx = j.K[2];
        a.cam.fy = j.K[4];
        a.cam.cy = j.K[5];
    }
    const auto d = [&](int i) { return i < j.nd ? j.D[i] : 0.0; };
    a.cam.k1 = d(0);
    a.cam.k2 = d(1);
    a.cam.p1 = d(2);
    a.cam.p2 = d(3);
    a.cam.k3 = d(4);
    a.cam.k4 = d(5);
    a.cam.k5 = d(6);
    a.cam.k6 = d(7);
    a.points = j.points;
    a.count = (uint32_t)j.count;
    a.img_rows = j.img_rows;
    a.img_cols = j.img_cols;
    a.splat = j.splat;
    a.tol = j.tol;
    a.image = j.image;
    a.depth = j.img_depth;
    a.channels = j.channels;
    a.img_pitch = j.img_pitch;
    a.fill = (uint32_t)j.fill;
    a.uv = j.uv;
    a.zdepth = j.depth;
    a.cls = j.cls;
    a.tex = j.tex;
    a.depth_map = j.depth_map;
    a.index_map = j.index_map;
    a.counts = j.counts;
    if (!j.zbuffer())
        return check_hip(bicos_hip::launch_project(a, st), "project launches");
    const size_t pixels = (size_t)j.img_rows * j.img_cols;
    Lease ws(e, e->ws, e->ws_bytes, st);
    auto carve = [&] { a.keys = ws.take<unsigned long long>(std::max<size_t>(pixels, 1)); };
    carve();
    if (int rc = ws.acquire()) return rc;
    carve();
    return check_hip(bicos_hip::launch_project(a, st), "project launches");
}

// ------------------------------------------------------------ disparity guide

int check_guide_params(const GuideJob& j) {
    if (j.scale < 1 || j.scale > 8) return fail(BICOS_E_ARG, "guide: scale must lie in 1 .. 8");
    if (j.radius < 0 || j.radius > 32767)
        return fail(BICOS_E_ARG, "guide: radius must lie in 0 .. 32767");
    if (j.spread < 0 || j.spread > 7) return fail(BICOS_E_ARG, "guide: spread must lie in 0 .. 7");
    if (j.fallback_lo < -32768 || j.fallback_lo > 32767 || j.fallback_hi < -32768 ||
        j.fallback_hi > 32767)
        return fail(BICOS_E_ARG, "guide: the fallback pair must fit int16");
    if (j.flags & ~BICOS_GUIDE_F32_SENTINEL) return fail(BICOS_E_ARG, "guide: unknown flag bits");
    return BICOS_OK;
}

int check_guide_job(const GuideJob& j) {
    if (int rc0 = check_map_type("guide", j.prior_type, "prior map")) return rc0;
    if (int rc0 = check_guide_params(j)) return rc0;
    if (j.rows < 0 || j.cols < 0 || j.prows < 0 || j.pcols < 0)
        return fail(BICOS_E_ARG, "guide: negative image size");
    if ((int64_t)j.rows * j.cols > INT32_MAX || (int64_t)j.prows * j.pcols > INT32_MAX)
        return fail(BICOS_E_ARG, "guide: rows * cols exceeds int32");
    if (j.guide_pitch && j.guide_pitch < (size_t)j.cols)
        return fail(BICOS_E_ARG, "guide: guide_pitch is smaller than cols");
    if (j.rows > 0 && j.cols > 0) {
        if (j.prows == 0 || j.pcols == 0) return fail(BICOS_E_ARG, "guide: empty prior map");
        if (!j.prior) return fail(BICOS_E_ARG, "guide: null prior map");
        if (!j.guide) return fail(BICOS_E_ARG, "guide: null guide");
        if ((uintptr_t)j.guide & 3u)
            return fail(BICOS_E_ARG, "guide: the guide's base is not 4-byte aligned");
    }
    return BICOS_OK;
}

int guide_device(const GuideJob& j, hipStream_t st) {
    if ((size_t)j.rows * j.cols == 0) return zero_counts(j.counts, 2, st);
    bicos_hip::GuideArgs a{};
    a.prior = j.prior;
    a.prows = j.prows;
    a.pcols = j.pcols;
    a.guide = j.guide;
    a.guide_pitch = j.guide_pitch ? j.guide_pitch : (size_t)j.cols;
    a.rows = j.rows;
    a.cols = j.cols;
    a.scale = j.scale;
    a.radius = j.radius;
    a.spread = j.spread;
    a.fallback_lo = j.fallback_lo;
    a.fallback_hi = j.fallback_hi;
    a.sentinel = (j.flags & BICOS_GUIDE_F32_SENTINEL) != 0;
    a.counts = j.counts;
    return check_hip(bicos_hip::launch_guide(a, j.prior_type == BICOS_CV_32F, st), "guide launch");
}

// ------------------------------------------------------------- stack pooling

static bicos_hip::PoolArgs pool_args(const PoolJob& j) {
    bicos_hip::PoolArgs a{};
    a.src = j.src;
    a.dst = j.dst;
    a.n = j.n;
    a.prows = j.rows / j.scale;
    a.pcols = j.cols / j.scale;
    a.src_row_pitch = (uint32_t)j.src_row_pitch;
    a.dst_row_pitch = (uint32_t)j.dst_row_pitch;
    a.src_plane_pitch = j.src_plane_pitch;
    a.dst_plane_pitch = j.dst_plane_pitch;
    return a;
}

int check_pool(const PoolJob& j, bool with_dst) {
    if (j.n < 1) return fail(BICOS_E_ARG, "pool: need at least one image");
    if (j.depth != 1 && j.depth != 2)
        return fail(BICOS_E_ARG, "pool: depth must be 1 (u8) or 2 (u16)");
    if (j.scale < bicos_hip::POOL_MIN_SCALE || j.scale > bicos_hip::POOL_MAX_SCALE)
        return fail(BICOS_E_ARG, "pool: scale must lie in 2 .. 8");
    if (j.rows < j.scale || j.cols < j.scale)
        return fail(BICOS_E_ARG, "pool: the image is smaller than scale x scale");
    const int prows = j.rows / j.scale, pcols = j.cols / j.scale;
    if (j.src_row_pitch < (size_t)j.cols || j.src_plane_pitch < (size_t)j.cols)
        return fail(BICOS_E_ARG, "pool: a source pitch is smaller than a row");
    if (with_dst && (j.dst_row_pitch < (size_t)pcols || j.dst_plane_pitch < (size_t)pcols))
        return fail(BICOS_E_ARG, "pool: an output pitch is smaller than a row");
    if (!j.src) return fail(BICOS_E_ARG, "pool: null source stack");
    if (with_dst && !j.dst) return fail(BICOS_E_ARG, "pool: null output stack");
    if (((uintptr_t)j.src | (with_dst ? (uintptr_t)j.dst : 0)) % (uintptr_t)j.depth)
        return fail(BICOS_E_ARG, "pool: a u16 stack's base is not 2-byte aligned");
    // 32-bit offsets within a plane
    const unsigned long long lim = 0xFFFFFFFFull;
    const unsigned long long src_plane =
        (unsigned long long)(j.rows - 1) * j.src_row_pitch + (unsigned long long)j.cols;
    const unsigned long long dst_plane =
        with_dst ? (unsigned long long)(prows - 1) * j.dst_row_pitch + (unsigned long long)pcols : 0;
    if (src_plane > lim || dst_plane > lim)
        return fail(BICOS_E_ARG, "pool: a plane spans more than 2^32 - 1 elements");
    if (bicos_hip::pool_blocks(pool_args(j)) > (uint64_t)INT32_MAX)
        return fail(BICOS_E_ARG, "pool: more tiles than one launch holds");
    if (with_dst) {
        const unsigned long long d = (unsigned long long)j.depth;
        const unsigned long long a = (uintptr_t)j.src, b = (uintptr_t)j.dst;
        const unsigned long long a_bytes = ((unsigned long long)(j.n - 1) * j.src_plane_pitch + src_plane) * d;
        const unsigned long long b_bytes = ((unsigned long long)(j.n - 1) * j.dst_plane_pitch + dst_plane) * d;
        if (a < b + b_bytes && b < a + a_bytes)
            return fail(BICOS_E_ARG, "pool: the output overlaps the source");
    }
    return BICOS_OK;
}

int pool_device(const PoolJob& j, hipStream_t st) {
    return check_hip(bicos_hip::launch_pool(pool_args(j), j.depth, j.scale, st), "pool launch");
}

// ------------------------------------------------------------- pyramid match

void pyramid_window(int min_disparity, int max_disparity, int scale, int* lo, int* hi) {
    const int64_t s = scale, a = min_disparity, b = max_disparity;
    // floor and ceil of the quotients (C++ division truncates toward zero)
    *lo = (int)(a / s - (a % s < 0 ? 1 : 0));
    *hi = (int)(b / s + (b % s > 0 ? 1 : 0));
}

int check_pyramid(const void* s0, const void* s1, int n, int rows, int cols, size_t row_pitch,
                  size_t plane_pitch, int depth, const BicosConfig& cfg, bool has_nxcorr,
                  const DispRange& range, const PyramidJob& j, const void* disp) {
    if (int rc0 = check_range(range.min, range.max)) return rc0;
    for (const void* s : {s0, s1}) {
        const PoolJob pj{s, n, rows, cols, row_pitch, plane_pitch, depth, j.scale, nullptr, 0, 0};
        if (int rc0 = check_pool(pj, false)) return rc0;
    }
    GuideJob gj{};
    gj.scale = j.scale;
    gj.radius = j.radius;
    gj.spread = j.spread;
    gj.fallback_lo = j.fallback_lo;
    gj.fallback_hi = j.fallback_hi;
    gj.flags = BICOS_GUIDE_F32_SENTINEL;
    if (int rc0 = check_guide_params(gj)) return rc0;
    MatchShape shape;
    if (int rc0 = check_match(s0, s1, n, rows, cols, row_pitch, plane_pitch, depth, cfg, has_nxcorr,
                              disp, false, &shape))
        return rc0;
    if ((int64_t)rows * cols > INT32_MAX)
        return fail(BICOS_E_ARG, "guide: rows * cols exceeds int32");
    if ((uintptr_t)j.guide & 3u)
        return fail(BICOS_E_ARG, "guide: the guide's base is not 4-byte aligned");
    return BICOS_OK;
}

int match_pyramid_device(bicos_engine* e, const void* s0, const void* s1, int n, int rows,
                         int cols, size_t row_pitch, size_t plane_pitch, int depth,
                         const BicosConfig& cfg, bool has_nxcorr, float threshold,
                         const DispRange& range, const PyramidJob& j, void* disp, void* corr,
                         hipStream_t st) {
    if (!e) return fail(BICOS_E_ARG, "null engine");
    const int prows = rows / j.scale, pcols = cols / j.scale;
    const size_t ppix = (size_t)prows * pcols, pix = (size_t)rows * cols;
    const int coarse_type = has_nxcorr ? BICOS_CV_32F : BICOS_CV_16S;
    // pooled stack 0 | pooled stack 1 | the coarse map | the guide, the last two only where the
    // caller does not keep them. Held over all four steps; the inner matches lease ws on the
    // same stream, which only re-records ws_ready.
    void *q0 = nullptr, *q1 = nullptr, *coarse = nullptr;
    int16_t* guide = nullptr;
    Lease pyr(e, e->pyr, e->pyr_bytes, st);
    auto carve = [&] {
        q0 = pyr.take(ppix * n * depth);
        q1 = pyr.take(ppix * n * depth);
        coarse = j.coarse ? j.coarse : pyr.take(ppix * (has_nxcorr ? 4 : 2));
        guide = j.guide ? j.guide : pyr.take<int16_t>(2 * pix);
    };
    carve();
    int rc = pyr.acquire();
    if (rc) return rc;
    carve();

    // 1. both stacks pooled into dense prows x pcols planes
    PoolJob pj{s0, n, rows, cols, row_pitch, plane_pitch, depth, j.scale, q0, (size_t)pcols, ppix};
    rc = pool_device(pj, st);
    pj.src = s1;
    pj.dst = q1;
    if (!rc) rc = pool_device(pj, st);
    if (rc) return rc;
    // 2. the coarse match over the scaled window, without subpixel interpolation
    BicosConfig coarse_cfg = cfg;
    coarse_cfg.subpixel_step = -1;
    DispRange coarse_range{0, 0};
    pyramid_window(range.min, range.max, j.scale, &coarse_range.min, &coarse_range.max);
    rc = match_device(e, q0, q1, n, prows, pcols, (size_t)pcols, ppix, depth, coarse_cfg,
                      has_nxcorr, threshold, coarse, nullptr, st, false, nullptr, nullptr,
                      &coarse_range);
    if (rc) return rc;
    // 3. its map as the prior of a full-size guide
    const GuideJob gj{coarse, coarse_type, prows, pcols, rows, cols, j.scale, j.radius, j.spread,
                      j.fallback_lo, j.fallback_hi, BICOS_GUIDE_F32_SENTINEL, guide, (size_t)cols,
                      j.counts};
    rc = guide_device(gj, st);
    if (rc) return rc;
    // 4. the guided match of the full stacks
    const DispRange fine{range.min, range.max, guide, (size_t)cols};
    rc = match_device(e, s0, s1, n, rows, cols, row_pitch, plane_pitch, depth, cfg, has_nxcorr,
                      threshold, disp, corr, st, false, nullptr, nullptr, &fine);
    // match_device's last act on `st` is the release of its ws lease (engine.hpp): ws_ready
    // stands behind its last launch, the last use of the guide, so a second record would only
    // put one more marker into the queue. BICOS_PYRAMID_SINGLE_RECORD=0 records it all the same
    // (A/B, read per call: tools/pool_bench.py measures both in one process).
    if (!rc && env_on("BICOS_PYRAMID_SINGLE_RECORD")) pyr.dismiss();
    return rc;
}

// ------------------------------------------------------------- rectification

int check_rectify(const RectifyJob& j) {
    if (j.n < 1) return fail(BICOS_E_ARG, "rectify: need at least one image");
    if (j.src_rows < 1 || j.src_cols < 1)
        return fail(BICOS_E_ARG, "rectify: the source size must be positive");
    if (j.rows < 1 || j.cols < 1)
        return fail(BICOS_E_ARG, "rectify: the output size must be positive");
    if (j.depth != 1 && j.depth != 2)
        return fail(BICOS_E_ARG, "rectify: depth must be 1 (u8) or 2 (u16)");
    if (j.src_row_pitch < (size_t)j.src_cols || j.src_plane_pitch < (size_t)j.src_cols)
        return fail(BICOS_E_ARG, "rectify: a source pitch is smaller than a row");
    if (j.dst_row_pitch < (size_t)j.cols || j.dst_plane_pitch < (size_t)j.cols)
        return fail(BICOS_E_ARG, "rectify: an output pitch is smaller than a row");
    if (j.map_pitch % sizeof(float))
        return fail(BICOS_E_ARG, "rectify: map_pitch must be a multiple of 4 bytes");
    if (j.map_pitch && j.map_pitch < (size_t)j.cols * sizeof(float))
        return fail(BICOS_E_ARG, "rectify: map_pitch is smaller than a row");
    if (j.border < 0 || j.border > (j.depth == 1 ? 255 : 65535))
        return fail(BICOS_E_ARG, "rectify: border is outside the range of the depth");
    if (!j.src) return fail(BICOS_E_ARG, "rectify: null source stack");
    if (!j.dst) return fail(BICOS_E_ARG, "rectify: null output stack");
    if (!j.map_x || !j.map_y) return fail(BICOS_E_ARG, "rectify: null map");
    if (j.dst == j.src) return fail(BICOS_E_ARG, "rectify: the output must not be the source");
    // 32-bit offsets within a plane, 32-bit linear index of the dense valid map
    const unsigned long long lim = 0xFFFFFFFFull;
    if ((unsigned long long)(j.src_rows - 1) * j.src_row_pitch + (unsigned long long)j.src_cols > lim ||
        (unsigned long long)(j.rows - 1) * j.dst_row_pitch + (unsigned long long)j.cols > lim ||
        (unsigned long long)j.rows * (j.map_pitch ? j.map_pitch / sizeof(float) : (size_t)j.cols) > lim ||
        (unsigned long long)j.rows * (unsigned long long)j.cols > (unsigned long long)INT32_MAX)
        return fail(BICOS_E_ARG, "rectify: a plane spans more than 2^32 - 1 elements");
    return BICOS_OK;
}

int rectify_device(const RectifyJob& j, hipStream_t st) {
    bicos_hip::RectifyArgs a{};
    a.src = j.src;
    a.dst = j.dst;
    a.map_x = j.map_x;
    a.map_y = j.map_y;
    a.valid = j.valid;
    a.n = j.n;
    a.src_rows = j.src_rows;
    a.src_cols = j.src_cols;
    a.rows = j.rows;
    a.cols = j.cols;
    a.src_row_pitch = (uint32_t)j.src_row_pitch;
    a.dst_row_pitch = (uint32_t)j.dst_row_pitch;
    a.src_plane_pitch = j.src_plane_pitch;
    a.dst_plane_pitch = j.dst_plane_pitch;
    a.map_pitch = (uint32_t)(j.map_pitch ? j.map_pitch / sizeof(float) : (size_t)j.cols);
    a.border = (uint32_t)j.border;
    // a lane's four pixels start at a column that is a multiple of four
    const size_t vec_bytes = (size_t)bicos_hip::RECTIFY_PER_LANE * j.depth;
    a.dst_vector = (uintptr_t)j.dst % vec_bytes == 0 &&
                   j.dst_row_pitch % bicos_hip::RECTIFY_PER_LANE == 0 &&
                   j.dst_plane_pitch % bicos_hip::RECTIFY_PER_LANE == 0;
    a.valid_vector = (uintptr_t)j.valid % 4 == 0 && j.cols % 4 == 0;
    return check_hip(bicos_hip::launch_rectify(a, j.depth, st), "rectify launch");
}

int check_rectify_maps(const RectifyMapsJob& j, bicos_hip::RectifyCamera* cam) {
    if (j.nd != 0 && j.nd != 4 && j.nd != 5 && j.nd != 8)
        return fail(BICOS_E_ARG, "rectify_maps: nd must be 0, 4, 5 or 8");
    if (j.p_cols != 3 && j.p_cols != 4)
        return fail(BICOS_E_ARG, "rectify_maps: p_cols must be 3 or 4");
    if (j.rows < 1 || j.cols < 1)
        return fail(BICOS_E_ARG, "rectify_maps: the output size must be positive");
    if ((int64_t)j.rows * j.cols > INT32_MAX)
        return fail(BICOS_E_ARG, "rectify_maps: rows * cols exceeds int32");
    if (!j.K || !j.P || (j.nd > 0 && !j.D))
        return fail(BICOS_E_ARG, "rectify_maps: null K, D or P");
    if (!j.map_x || !j.map_y) return fail(BICOS_E_ARG, "rectify_maps: null map");
    bool finite = true;
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(j.K[i]);
    for (int i = 0; i < j.nd; ++i) finite = finite && std::isfinite(j.D[i]);
    for (int i = 0; j.R && i < 9; ++i) finite = finite && std::isfinite(j.R[i]);
    for (int i = 0; i < 3 * j.p_cols; ++i) finite = finite && std::isfinite(j.P[i]);
    if (!finite) return fail(BICOS_E_ARG, "rectify_maps: a calibration value is not finite");
    static const double identity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double* R = j.R ? j.R : identity;
    double m[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double* p = j.P + r * j.p_cols;
            m[r][c] = ((p[0] * R[c] + p[1] * R[3 + c]) + p[2] * R[6 + c]);
        }
    const double det = (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) -
                        m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])) +
                       m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    if (det == 0.0 || !std::isfinite(det))
        return fail(BICOS_E_ARG, "rectify_maps: P[:, :3] * R is singular");
    bicos_hip::RectifyCamera c{};
    c.iM[0] = (m[1][1] * m[2][2] - m[1][2] * m[2][1]) / det;
    c.iM[1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det;
    c.iM[2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
    c.iM[3] = (m[1][2] * m[2][0] - m[1][0] * m[2][2]) / det;
    c.iM[4] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det;
    c.iM[5] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
    c.iM[6] = (m[1][0] * m[2][1] - m[1][1] * m[2][0]) / det;
    c.iM[7] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det;
    c.iM[8] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
    c.fx = j.K[0];
    c.cx = j.K[2];
    c.fy = j.K[4];
    c.cy = j.K[5];
    const auto d = [&](int i) { return i < j.nd ? j.D[i] : 0.0; };
    c.k1 = d(0);
    c.k2 = d(1);
    c.p1 = d(2);
    c.p2 = d(3);
    c.k3 = d(4);
    c.k4 = d(5);
    c.k5 = d(6);
    c.k6 = d(7);
    *cam = c;
    return BICOS_OK;
}

int rectify_maps_device(const RectifyMapsJob& j, const bicos_hip::RectifyCamera& cam,
                        hipStream_t st) {
    return check_hip(bicos_hip::launch_rectify_maps(cam, j.rows, j.cols, j.map_x, j.map_y, st),
                     "rectify_maps launch");
}

// ------------------------------------------------------- process-wide engines

namespace {
std::mutex g_engines_lock;
std::map<int, bicos_engine*> g_engines;
}  // namespace

bicos_engine* default_engine(int device) {
    std::lock_guard<std::mutex> g(g_engines_lock);
    auto it = g_engines.find(device);
    if (it != g_engines.end()) return it->second;
    bicos_engine* e = nullptr;
    if (bicos_engine_create(device, &e) != BICOS_OK) return nullptr;
    g_engines[device] = e;
    return e;
}

bool is_default_engine(const bicos_engine* e) {
    std::lock_guard<std::mutex> g(g_engines_lock);
    for (const auto& kv : g_engines)
        if (kv.second == e) return true;
    return false;
}

}  // namespace bicos_impl
