// engine.hpp -- host-side orchestration of the BICOS hot path (internal).
//
// Plays the role of the reference's match_impl (src/impl/cpu.cpp:35-98,
// src/impl/cuda.cu:56-463): transform both stacks, search, optional consistency,
// optional agree / subpixel. All launches are asynchronous on one HIP stream.
//
//   engine.cpp  errors, the workspace lease, engine resources, the plans, the search driver
//               and match_device; reproject_device (disparity map -> 3-D points);
//               speckle_device (the speckle filter of a disparity map); rectify_device and
//               rectify_maps_device (raw stacks -> rectified stacks); median_device (the
//               median filter of a disparity map); normals_device (a disparity map -> unit
//               surface normals); mesh_device (a disparity map -> a triangle mesh over the
//               reprojection's point list); project_device (a point list -> another camera's
//               pixels, visibility, texture and registered depth); guide_device (a prior
//               disparity map -> per-pixel search windows); pool_device (a stack pooled by an integer factor);
//               match_pyramid_device (pool, coarse ranged match, guide, guided match)
//   host.cpp    the banded host-buffer pipeline (HostPool, match_host); the staged host call
//               (Staging) and the eleven paths on it: reproject_host; speckle_host; rectify_host,
//               rectify_maps_host; median_host; normals_host; mesh_host; project_host; guide_host;
//               pool_host; match_pyramid_host
//   entries.cpp the bicos_* extern "C" entries (bicos_c.h) but the multi-GPU ones
//   multi.cpp   bicos_match_host_multi, bicos_match_bands_device
//   cxxapi.cpp  namespace BICOS (HipImage, match, reproject, filter_speckles, median_filter,
//               normals, mesh, project, guide_from_disparity, pool_stack, match_pyramid)
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <condition_variable>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bicos_c.h"
#include "kernels.hpp"
#include "rectify.hpp"

namespace bicos_impl {
// Small persistent pool for the host-side copies of the host-buffer pipeline: run(k, f)
// calls f(0..k-1), the caller taking part, and returns when all have finished.
class HostPool {
  public:
    explicit HostPool(int threads);
    ~HostPool();
    int size() const { return (int)workers_.size() + 1; }
    void run(int tasks, const std::function<void(int)>& f);

  private:
    void loop();
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* job_ = nullptr;
    int tasks_ = 0, next_ = 0, active_ = 0;
    unsigned gen_ = 0;
    bool stop_ = false;
};

// pinned host memory, grown on demand (grow_pinned)
struct PinnedBuf {
    void* p = nullptr;
    size_t bytes = 0;
};
}  // namespace bicos_impl

struct bicos_engine {
    int device = 0;
    int max_lds = 64 * 1024;           // search row stage budget (>= 2 workgroups per CU)
    int lds_limit = 64 * 1024;         // device limit per workgroup
    int cus = 256;                     // compute units (workgroup geometry)
    // search kernel tuning (0 = automatic): see bicos_engine_tune
    int tune_variant = 0, tune_R = 0, tune_waves = 0, tune_split = 0;
    hipStream_t own_stream = nullptr;  // used by the host-buffer APIs
    std::mutex lock;                   // serialises host-buffer calls on this engine

    // workspace (grown on demand, never shrunk). ws_ready is recorded after every use of
    // ws / stage on the caller's stream and waited on before the next: calls on different
    // streams are ordered, never racing on the shared buffers (bicos_impl::Lease).
    hipEvent_t ws_ready = nullptr;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    // host-API staging (device): band-major stacks + dense output maps
    void* stage = nullptr;
    size_t stage_bytes = 0;
    // the pyramid match's own buffers (match_pyramid_device): the pooled stacks, and the coarse
    // map and the guide where the caller keeps neither. Beside ws, not inside it: the inner
    // matches lease ws themselves. Ordered by ws_ready like the other two.
    void* pyr = nullptr;
    size_t pyr_bytes = 0;
    // host-buffer pipeline (match_host): copy stream, pinned band slots, band events
    hipStream_t copy_stream = nullptr;
    bicos_impl::PinnedBuf pinned;  // K input band slots
    std::vector<hipEvent_t> events;
    std::unique_ptr<bicos_impl::HostPool> pool;
    // host-staged multi-GPU gather (multi.cpp bicos_match_bands_device): its own pinned
    // buffer and events, grown only (sharing match_host's slots reallocated the
    // pinned memory whenever the two paths alternated)
    bicos_impl::PinnedBuf gather_pinned;
    std::vector<hipEvent_t> gather_events;
    // host-buffer pipeline, maps downloaded band by band on their own stream (so a copy
    // engine other than the uploads' can take them: PCIe is full duplex) into pinned memory,
    // then copied into the caller's buffers by the pool; 2 events per band (matched, landed)
    hipStream_t dl_stream = nullptr;
    // a second upload stream: each band's upload split in two halves (BICOS_HOST_UPLOAD_STREAMS)
    hipStream_t copy_stream2 = nullptr;
    std::vector<hipEvent_t> events2;
    bicos_impl::PinnedBuf pinned_out;
    std::vector<hipEvent_t> dl_events;
};

namespace bicos_impl {

void set_error(int code, const std::string& msg);
int fail(int code, const std::string& msg);
const char* last_error();  // this thread's last message
int check_hip(hipError_t e, const char* what);

// The boundary of every extern "C" entry: f's code, or BICOS_E_INTERNAL for what it throws
template <class F>
int guarded(F&& f) {
    try {
        return f();
    } catch (const std::exception& ex) {
        return fail(BICOS_E_INTERNAL, ex.what());
    } catch (...) {
        return fail(BICOS_E_INTERNAL, "unknown exception");
    }
}

// n >= 2 images of depth 1 or 2 bytes, no negative size: BICOS_OK or BICOS_E_ARG
int check_stack_shape(int n, int depth, int rows, int cols);

// reference src/pybicos_c.cpp:59-61: a negative threshold keeps the default 0.5
inline float nxc_threshold(const BicosConfig& cfg) {
    return cfg.nxcorr_threshold >= 0 ? cfg.nxcorr_threshold : 0.5f;
}

// Reserve `bytes` of engine workspace (device), stream-ordered on `st`: a buffer that
// must grow is freed on `st` after `ready` (every earlier use) and the new one allocated
// there (hipFreeAsync / hipMallocAsync). Returns BICOS_OK or an error code.
int reserve(void*& buf, size_t& have, size_t bytes, int device, hipStream_t st, hipEvent_t ready);

constexpr size_t ALIGN = 256;
inline size_t align_up(size_t x) { return (x + ALIGN - 1) / ALIGN * ALIGN; }

// One use of an engine buffer (ws, stage or pyr) on one stream, and the rule that keeps two
// streams from racing on it: acquire() reserves the bytes, makes `st` wait for ws_ready
// (every earlier use, on any stream), and from then on release() -- at the latest the
// destructor, on every exit path -- records ws_ready on `st`.
// The layout is a sequence of take() calls that the user walks twice with the same code:
// before acquire() the calls only add up the bytes (and return nullptr), after it they hand
// out the 256-byte aligned sub-buffers in the same order, so a size cannot disagree with
// its layout.
class Lease {
  public:
    Lease(bicos_engine* e, void*& buf, size_t& have, hipStream_t st)
        : e_(e), buf_(buf), have_(have), st_(st) {}
    Lease(const Lease&) = delete;
    ~Lease() { release(); }

    template <class T = char>
    T* take(size_t count) {
        const size_t at = off_;
        off_ += align_up(count * sizeof(T));
        return held_ ? (T*)((char*)buf_ + at) : nullptr;
    }
    int acquire();
    void release();
    // release() without the record, for a holder whose last step on `st` was another lease's
    // release(): ws_ready already stands behind every use of this buffer
    void dismiss() { held_ = false; }
    char* base() const { return (char*)buf_; }
    size_t needed() const { return off_; }  // bytes taken so far

  private:
    bicos_engine* e_;
    void*& buf_;
    size_t& have_;
    hipStream_t st_;
    size_t off_ = 0;
    bool held_ = false;
};

// One staged host call (host.cpp; every *_host path but match_host's banded pipeline): a lease
// on e->stage over e->own_stream whose buffers are declared once each -- size, host side,
// direction, the name check_hip reports, where the device pointer goes -- so that a buffer's
// size is written once for its layout, its upload and its download.
//     Staging s(e);  declarations;  int rc = s.begin();  if (!rc) rc = ..._device(.., s.stream());
//     return s.finish(rc);
// begin() leases the sum, hands out the 256-byte aligned pointers and issues the uploads in
// declaration order; finish(rc) issues the downloads in declaration order if nothing failed,
// then synchronises in any case and returns the first error, else the synchronisation's. The
// lease is released (ws_ready recorded) by the destructor, on every exit path.
// e is not null and its lock is held: the entries (entries.cpp) find the engine.
class Staging {
  public:
    explicit Staging(bicos_engine* e)
        : lease_(e, e->stage, e->stage_bytes, e->own_stream), st_(e->own_stream) {}
    hipStream_t stream() const { return st_; }

    // A device-only buffer of `bytes` -> its number, for up() / down() into parts of it
    template <class T>
    int buffer(T*& dev, size_t bytes) {
        bufs_.push_back({bytes, &dev, [](void* slot, char* p) { *(T**)slot = (T*)p; }});
        return (int)bufs_.size() - 1;
    }
    // ... one that is uploaded from / downloaded into `host` whole. A null host is an absent
    // optional buffer: no bytes, a null device pointer, no copy.
    template <class T>
    void in(T*& dev, const void* host, size_t bytes, const char* what) {
        if (!host) return (void)(dev = nullptr);
        up(buffer(dev, bytes), 0, host, bytes, what);
    }
    template <class T>
    void out(T*& dev, void* host, size_t bytes, const char* what) {
        if (!host) return (void)(dev = nullptr);
        down(buffer(dev, bytes), 0, host, bytes, what);
    }
    // Copies between `host` and byte `at` of buffer `buf`: dense (hipMemcpyAsync), or `rows` rows
    // of `row_bytes`, `host_pitch` bytes apart on the host and dense in the buffer
    // (hipMemcpy2DAsync)
    void up(int buf, size_t at, const void* host, size_t bytes, const char* what) {
        copies_.push_back({buf, at, (void*)host, 0, bytes, 0, true, what});
    }
    void down(int buf, size_t at, void* host, size_t bytes, const char* what) {
        copies_.push_back({buf, at, host, 0, bytes, 0, false, what});
    }
    void up2d(int buf, size_t at, const void* host, size_t host_pitch, size_t row_bytes,
              size_t rows, const char* what) {
        copies_.push_back({buf, at, (void*)host, host_pitch, row_bytes, rows, true, what});
    }
    void down2d(int buf, size_t at, void* host, size_t host_pitch, size_t row_bytes, size_t rows,
                const char* what) {
        copies_.push_back({buf, at, host, host_pitch, row_bytes, rows, false, what});
    }

    int begin();
    // For a download whose length an earlier one decides (reproject_host, mesh_host), between the
    // device call and finish(): both do nothing but return the first error once there is one.
    int download(void* host, const void* dev, size_t bytes, const char* what);
    int sync();
    int finish(int rc);

  private:
    struct Buf {
        size_t bytes;
        void* slot;
        void (*set)(void* slot, char* p);
        char* dev = nullptr;
    };
    struct Copy {
        int buf;
        size_t at;
        void* host;
        size_t host_pitch, row_bytes, rows;  // rows 0: dense, row_bytes in all
        bool upload;
        const char* what;
    };
    int issue(bool upload);
    Lease lease_;
    hipStream_t st_;
    std::vector<Buf> bufs_;
    std::vector<Copy> copies_;
    int rc_ = BICOS_OK;
};

// Engine resources, each grown on demand and freed by free_resources (bicos_engine_destroy)
int grow_pinned(PinnedBuf& b, size_t bytes, const char* what);  // failure: null, 0 bytes
int grow_events(std::vector<hipEvent_t>& v, int count);
int ensure_stream(hipStream_t& s);  // a non-blocking stream, created on first use
void free_resources(bicos_engine* e);  // streams, events, pinned buffers; not ws / stage / pyr

int descriptor_words(int n, int mode);

// An inclusive disparity window min <= col0 - col1 <= max (bicos_c.h, the *_range entries)
// guide != nullptr (the *_guided entries): besides, one window per left pixel for the forward
// search, guide[row * guide_pitch + col] = {lo, hi} in device memory (4-byte aligned,
// guide_pitch in pixels)
struct DispRange {
    int min, max;
    const int16_t* guide = nullptr;
    size_t guide_pitch = 0;
};

// What the search stage runs (the search's BICOS_PLAN_* bits: MATRIX_CORES, PACKED_KEYS,
// CONSISTENCY_ONE_PASS, REVERSE_COMPACTED, DENSE_ROWS) and what it runs it with
struct SearchPlan {
    int bits = 0;
    bool two_pass = false;       // Consistency as forward search, reverse search and a check:
                                 // the one form that needs workspace (SearchBuffers)
    bicos_hip::MxGeometry mx{};  // of the full-row matrix-core search (MATRIX_CORES, no range)
};
// e may be NULL (256 CUs, untuned). used_bits: the K-step hint, written_bits: the exact count
// one-pass Consistency is eligible by (0 = unknown); a stage entry has one hint for both.
SearchPlan search_plan(const bicos_engine* e, int rows, int cols, int words, int used_bits,
                       int written_bits, bool nodupes, bool consistency, bool ranged);

// the maps of a two-pass Consistency search, taken from a lease in this order
struct SearchBuffers {
    int16_t* fwd = nullptr;
    int16_t* rev = nullptr;
    uint8_t* valid = nullptr;  // per-tile valid counts (DENSE_ROWS)
};
SearchBuffers search_buffers(Lease& ws, const SearchPlan& p, int rows, int cols);

struct SearchJob {
    const uint32_t* d0;  // descriptors (bicos_desc_pitch rows) of the matched side
    const uint32_t* d1;  // ... and of the searched side
    int rows, cols, words;
    int used_bits, written_bits;  // as search_plan's
    bool nodupes;
    int max_lr_diff;
    const DispRange* range;  // nullptr: the whole row
};
// The search stage of `p` on `st`: the final int16 map into `out`; with out == nullptr
// (two-pass Consistency whose check runs inside the agree) only b.fwd and b.rev.
// fused_agree (BICOS_PLAN_AGREE_IN_SEARCH): the agree to run inside the search launch.
int run_search(const bicos_engine* e, const SearchPlan& p, const SearchBuffers& b,
               const SearchJob& j, int16_t* out, hipStream_t st,
               const bicos_hip::AgreeArgs* fused_agree = nullptr);

// Bytes the kernels may address from a stack base (32-bit buffer offsets): BICOS_E_ARG past 4 GiB
int stack_span(int n, int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
               uint32_t* out);
int subpixel_steps(float step);  // 0: more than the kernels accept

// The agree / subpixel launch arguments; minvar_scaled: min_variance * n (cpu.cpp:127)
bicos_hip::AgreeArgs agree_args(const int16_t* raw, const void* s0, const void* s1, int n,
                                int rows, int cols, size_t row_pitch, size_t plane_pitch,
                                uint32_t span, float threshold, float step, int nsteps,
                                int has_minvar, float minvar_scaled, void* out, bool out_f32,
                                void* corr);

// Full match on device buffers (validated arguments). corr may be null. disp_i16: the
// disparity map is int16 even with the NXC stage (no subpixel; bicos_match_device_i16).
// ext_d0 / ext_d1: the two stacks' descriptors (transform output, bicos_desc_pitch rows)
// already computed -- the match then runs from its search on (bicos_search_agree_device).
// range: the search's disparity window (nullptr: the whole row) -- the windowed matrix-core
// search (search_range.hip), none of the fused or compacted plans.
// Postcondition that match_pyramid_device relies on: a call that returns BICOS_OK for a
// non-empty image has leased ws, and the last thing it put on `st` is that lease's record of
// ws_ready, behind all its launches.
int match_device(bicos_engine* e, const void* s0, const void* s1, int n, int rows, int cols,
                 size_t row_pitch, size_t plane_pitch, int depth, const BicosConfig& cfg,
                 bool has_nxcorr, float threshold, void* disp, void* corr, hipStream_t st,
                 bool disp_i16 = false, const uint32_t* ext_d0 = nullptr,
                 const uint32_t* ext_d1 = nullptr, const DispRange* range = nullptr);

// What match_device refuses, in its order, and what it derives on the way: BICOS_E_ARG /
// BICOS_E_BITS (with a message); no HIP call. An empty image (rows or cols 0) passes without
// its buffers and pitches being looked at.
struct MatchShape {
    int mode, words;
    bool has_step;
    int nsteps;
    uint32_t span;
};
int check_match(const void* s0, const void* s1, int n, int rows, int cols, size_t row_pitch,
                size_t plane_pitch, int depth, const BicosConfig& cfg, bool has_nxcorr,
                const void* disp, bool disp_i16, MatchShape* out);

// What match_device runs after the transform (bicos_match_plan: bits()): the search's part
// and the agree's (BICOS_PLAN_AGREE_IN_SEARCH, BICOS_PLAN_CONSISTENCY_IN_AGREE)
struct MatchPlan {
    SearchPlan search;
    int agree = 0;
    int bits() const { return search.bits | agree; }
};
MatchPlan match_plan(const bicos_engine* e, int n, int rows, int cols, size_t row_pitch,
                     size_t plane_pitch, int depth, const BicosConfig& cfg, bool has_nxcorr,
                     const void* s0, const void* s1, bool ranged = false);

// bicos_search_packed (bicos_c.h): whether this NoDuplicates search's main launch runs on packed
// keys (search_pk.hip search_pkp_kernel)
bool search_runs_packed(const bicos_engine* e, int rows, int cols, int words, int bits, int n,
                        bool fused);

// Host buffers in and out (the reference's cv::Mat path, src/impl/cpu.cpp:100-159): the
// stacks are uploaded in row bands through pinned slots on a copy stream while earlier
// bands match on the compute stream; the maps are downloaded into `disp` / `corr` (dense
// rows x cols). p0/p1: n plane pointers each, steps0/steps1: bytes per row of each plane.
// Synchronous.
int match_host(bicos_engine* e, const void* const* p0, const size_t* steps0,
               const void* const* p1, const size_t* steps1, int n, int rows, int cols,
               int depth, const BicosConfig& cfg, bool has_nxcorr, float threshold, void* disp,
               void* corr, const DispRange* range = nullptr);
// (range->guide, if any, is in HOST memory here: uploaded whole before the first band)

// BICOS_E_ARG (with a message) for a window whose min exceeds its max; no HIP call
int check_range(int min_disparity, int max_disparity);
// ... and for what the *_guided entries refuse besides: a null guide, a pitch below cols, a
// base that is not 4-byte aligned
int check_guide(const void* guide, size_t guide_pitch, int cols, int min_disparity,
                int max_disparity);

// One guide build (bicos_c.h "disparity guide"): the arguments of bicos_guide_device /
// bicos_guide_host, the pointers all in device or all in host memory.
struct GuideJob {
    const void* prior;
    int prior_type, prows, pcols;
    int rows, cols;
    int scale, radius, spread;
    int fallback_lo, fallback_hi;
    int flags;
    int16_t* guide;
    size_t guide_pitch;  // pixels; 0 = cols
    uint32_t* counts;
};
int check_guide_job(const GuideJob& j);  // BICOS_E_ARG (with a message); no HIP call
// ... its part that looks at scale, radius, spread, the fallback pair and the flags alone
int check_guide_params(const GuideJob& j);
int guide_device(const GuideJob& j, hipStream_t st);
int guide_host(bicos_engine* e, const GuideJob& j);

// One pooling of a stack (bicos_c.h "stack pooling"): the arguments of bicos_pool_device, the
// pointers in device memory, the pitches in elements.
struct PoolJob {
    const void* src;
    int n, rows, cols;
    size_t src_row_pitch, src_plane_pitch;
    int depth, scale;
    void* dst;
    size_t dst_row_pitch, dst_plane_pitch;
};
// BICOS_E_ARG (with a message) for what the entries refuse; no HIP call. with_dst = false: the
// source side alone (the pyramid match, whose pooled stacks are its own).
int check_pool(const PoolJob& j, bool with_dst = true);
// The one launch on `st` (validated arguments); no workspace, no engine.
int pool_device(const PoolJob& j, hipStream_t st);
// Host buffers: n plane pointers in and out with their steps in bytes, staged through the
// engine, the same launch on its own stream. Synchronous.
int pool_host(bicos_engine* e, const void* const* src, size_t src_step, void* const* dst,
              size_t dst_step, const PoolJob& j);

// The pyramid match (bicos_c.h "pyramid match"): what it takes besides a ranged match's
// arguments. coarse, guide and counts are optional outputs, in device memory for
// match_pyramid_device and in host memory for match_pyramid_host.
struct PyramidJob {
    int scale, radius, spread;
    int fallback_lo, fallback_hi;
    void* coarse;
    int16_t* guide;
    uint32_t* counts;
};
// The coarse match's window: [floor(min / scale), ceil(max / scale)]
void pyramid_window(int min_disparity, int max_disparity, int scale, int* lo, int* hi);
// BICOS_E_ARG / BICOS_E_BITS (with a message) for what any of the four steps would refuse; no
// HIP call. s0 / s1: the stacks' bases, device memory or (host entry) any non-null placeholder.
int check_pyramid(const void* s0, const void* s1, int n, int rows, int cols, size_t row_pitch,
                  size_t plane_pitch, int depth, const BicosConfig& cfg, bool has_nxcorr,
                  const DispRange& range, const PyramidJob& j, const void* disp);
// pool both stacks, match them over the coarse window, build the guide, run the guided match:
// enqueued on `st`, the pooled stacks (and the coarse map / the guide the caller does not keep)
// in e->pyr. Validated arguments (check_pyramid); the caller holds e->lock.
int match_pyramid_device(bicos_engine* e, const void* s0, const void* s1, int n, int rows,
                         int cols, size_t row_pitch, size_t plane_pitch, int depth,
                         const BicosConfig& cfg, bool has_nxcorr, float threshold,
                         const DispRange& range, const PyramidJob& j, void* disp, void* corr,
                         hipStream_t st);
// Host buffers: each stack uploaded once, whole, into the engine's staging; the device pyramid
// on the engine's own stream; the maps and the optional outputs downloaded. Synchronous.
int match_pyramid_host(bicos_engine* e, const void* const* p0, const void* const* p1, size_t step,
                       int n, int rows, int cols, int depth, const BicosConfig& cfg,
                       bool has_nxcorr, float threshold, const DispRange& range,
                       const PyramidJob& j, void* disp, void* corr);

// One reprojection (bicos_c.h "reprojection"): the arguments of bicos_reproject_device /
// bicos_reproject_host, the pointers all in device or all in host memory.
struct ReprojectJob {
    const void* disp;
    int disp_type, rows, cols;
    const double* Q;
    int flags;
    float* xyz_map;
    float* points;
    int32_t* index;
    size_t capacity;
    uint32_t* counts;
};
// BICOS_E_ARG (with a message) for what the entries refuse; no HIP call. needs_engine: points
// without an engine are an error (the device entry; the host entry has a default engine).
int check_reproject(const ReprojectJob& j, const bicos_engine* e, bool needs_engine);
// The launches on `st` (validated arguments): the dense map alone, or count / scan / write
// with the segment counts in the engine's workspace.
int reproject_device(bicos_engine* e, const ReprojectJob& j, hipStream_t st);
// Host buffers: the map uploaded into the engine's staging, the same launches on the engine's
// own stream, the counts and then min(kept, capacity) points downloaded. Synchronous.
int reproject_host(bicos_engine* e, const ReprojectJob& j);

// One speckle filter (bicos_c.h "speckle filter"): the arguments of bicos_speckle_device /
// bicos_speckle_host, the pointers all in device or all in host memory.
struct SpeckleJob {
    const void* disp;
    int disp_type, rows, cols;
    int max_size;
    float max_diff;
    int flags;
    void* out;
    int32_t* labels;
    uint32_t* counts;
};
// BICOS_E_ARG (with a message) for what the entries refuse; no HIP call. needs_engine: a NULL
// engine is an error (the device entry; the host entry has a default engine).
int check_speckle(const SpeckleJob& j, const bicos_engine* e, bool needs_engine);
// The launches on `st` (validated arguments): tile, border, resolve, apply, with the label
// array (unless j.labels is given) and the size array in the engine's workspace.
int speckle_device(bicos_engine* e, const SpeckleJob& j, hipStream_t st);
// Host buffers: the map uploaded into the engine's staging, the same launches on the engine's
// own stream, the map, the counts and the labels downloaded. Synchronous.
int speckle_host(bicos_engine* e, const SpeckleJob& j);

// One median filter (bicos_c.h "median filter"): the arguments of bicos_median_device /
// bicos_median_host, the pointers all in device or all in host memory.
struct MedianJob {
    const void* disp;
    int disp_type, rows, cols;
    int ksize, fill_min, flags;
    void* out;
    uint32_t* counts;
};
// BICOS_E_ARG (with a message) for what the entries refuse; no HIP call. device: any overlap
// of map and out is an error (the host entry stages both, so its out may be the map).
int check_median(const MedianJob& j, bool device);
// The launch on `st` (validated arguments). It needs nothing of an engine.
int median_device(const MedianJob& j, hipStream_t st);
// Host buffers: the map uploaded into the engine's staging, the same launch on the engine's
// own stream, the map and the counts downloaded. Synchronous.
int median_host(bicos_engine* e, const MedianJob& j);

// One normal estimation (bicos_c.h "surface normals"): the arguments of bicos_normals_device /
// bicos_normals_host, the pointers all in device or all in host memory.
struct NormalsJob {
    const void* disp;
    int disp_type, rows, cols;
    const double* Q;
    int flags, radius;
    float max_diff;
    int min_points;
    float* normal_map;
    const int32_t* index;
    size_t count;
    float* normals;
    uint32_t* counts;
};
// BICOS_E_ARG (with a message) for what the entries refuse; no HIP call.
int check_normals(const NormalsJob& j);
// The launches on `st` (validated arguments): the dense map, the list, or both. They need
// nothing of an engine.
int normals_device(const NormalsJob& j, hipStream_t st);
// Host buffers: the map and the index uploaded into the engine's staging, the same launches on
// the engine's own stream, the map, the list and the counts downloaded as asked. Synchronous.
// rows * cols > 0 (bicos_normals_host answers an empty map itself, without an engine).
int normals_host(bicos_engine* e, const NormalsJob& j);

// One triangulation (bicos_c.h "mesh"): the arguments of bicos_mesh_device / bicos_mesh_host,
// the pointers all in device or all in host memory.
struct MeshJob {
    const void* disp;
    int disp_type, rows, cols;
    const double* Q;
    int flags;
    float max_diff;
    float* points;
    int32_t* index;
    size_t vertex_capacity;
    uint32_t* counts;
    int32_t* triangles;
    size_t tri_capacity;
    uint32_t* mesh_counts;
    int32_t* vertex_map;
};
// BICOS_E_ARG (with a message) for what the entries refuse; no HIP call. needs_engine: a NULL
// engine is an error (the device entry; the host entry has a default engine).
int check_mesh(const MeshJob& j, const bicos_engine* e, bool needs_engine);
// The six launches on `st` (validated arguments), with the segment counts and (unless
// j.vertex_map is given) the rank array in the engine's workspace.
int mesh_device(bicos_engine* e, const MeshJob& j, hipStream_t st);
// Host buffers: the map uploaded into the engine's staging, the same launches on the engine's
// own stream, both counts downloaded and then min(kept, vertex_capacity) points and
// min(triangles, tri_capacity) triangles. Synchronous.
// rows * cols > 0 (bicos_mesh_host answers an empty map itself, without an engine).
int mesh_host(bicos_engine* e, const MeshJob& j);

// One projection (bicos_c.h "projection"): the arguments of bicos_project_device /
// bicos_project_host, the pointers all in device or all in host memory (the camera always in
// host memory).
struct ProjectJob {
    const float* points;
    size_t count;
    const double* R;
    const double* t;
    const double* K;
    const double* D;
    int nd, img_rows, img_cols, splat;
    float tol;
    const void* image;
    int img_depth, channels;
    size_t img_pitch;
    int fill;
    float* uv;
    float* depth;
    uint8_t* cls;
    void* tex;
    float* depth_map;
    int32_t* index_map;
    uint32_t* counts;
    // the z-buffer is needed: tol is finite or a map is asked for
    bool zbuffer() const { return tol < INFINITY || depth_map || index_map; }
};
// BICOS_E_ARG (with a message) for what the entries refuse; no HIP call. needs_engine: a NULL
// engine is an error where the z-buffer is needed (the device entry; the host entry has a
// default engine).
int check_project(const ProjectJob& j, const bicos_engine* e, bool needs_engine);
// The launches on `st` (validated arguments), the z-buffer's keys in the engine's workspace; e
// may be NULL where no z-buffer is needed.
int project_device(bicos_engine* e, const ProjectJob& j, hipStream_t st);
// Host buffers: the points and the image (its rows made dense) uploaded into the engine's
// staging, the same launches on the engine's own stream, every output asked for downloaded.
// Synchronous.
int project_host(bicos_engine* e, const ProjectJob& j);

// One remap of a stack (bicos_c.h "rectification"): the arguments of bicos_rectify_device, the
// pointers all in device memory, the stack pitches in elements, map_pitch in bytes (0 = dense).
struct RectifyJob {
    const void* src;
    int n, src_rows, src_cols;
    size_t src_row_pitch, src_plane_pitch;
    int depth;
    const float* map_x;
    const float* map_y;
    size_t map_pitch;
    int rows, cols;
    void* dst;
    size_t dst_row_pitch, dst_plane_pitch;
    int border;
    uint8_t* valid;
};
// BICOS_E_ARG (with a message) for what the entries refuse; no HIP call.
int check_rectify(const RectifyJob& j);
// The one launch on `st` (validated arguments); no workspace, no engine.
int rectify_device(const RectifyJob& j, hipStream_t st);
// Host buffers: n plane pointers in and out with their steps in bytes (0 = dense), the maps and
// valid in host memory; staged through the engine, the same launch on its own stream. Synchronous.
int rectify_host(bicos_engine* e, const void* const* src, size_t src_step, void* const* dst,
                 size_t dst_step, const RectifyJob& j);

// The maps of one camera (bicos_c.h "rectification"): the calibration as the entries take it.
struct RectifyMapsJob {
    const double* K;
    const double* D;
    int nd;
    const double* R;
    const double* P;
    int p_cols, rows, cols;
    float* map_x;
    float* map_y;
};
// BICOS_E_ARG (with a message) for what the entries refuse, else the camera with the inverse of
// P[:, :3] * R as the kernel takes it (plain double arithmetic on the host); no HIP call.
int check_rectify_maps(const RectifyMapsJob& j, bicos_hip::RectifyCamera* cam);
int rectify_maps_device(const RectifyMapsJob& j, const bicos_hip::RectifyCamera& cam,
                        hipStream_t st);
// Host maps: computed in the engine's staging on its own stream and downloaded. Synchronous.
int rectify_maps_host(bicos_engine* e, const RectifyMapsJob& j, const bicos_hip::RectifyCamera& cam);

// Process-wide engine for `device` (created on first use).
bicos_engine* default_engine(int device);
bool is_default_engine(const bicos_engine* e);

}  // namespace bicos_impl
