// entries.cpp -- the bicos_* extern "C" entries of include/bicos_c.h over bicos_impl
// (engine.hpp); the multi-GPU entries are multi.cpp, the reference's ctypes ABI capi.cpp.
#include "engine.hpp"
#include "reproject.hpp"
#include "speckle.hpp"
#include "median.hpp"
#include "normals.hpp"
#include "project.hpp"
#include "guide.hpp"
#include "pool.hpp"
#include "search_plan.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

using namespace bicos_impl;

namespace {

int check_words(int words) {
    if (words == 1 || words == 2 || words == 4 || words == 8) return BICOS_OK;
    return fail(BICOS_E_ARG, "words must be 1, 2, 4 or 8");
}

// The one way from an entry to its engine: f(e) under `guarded` with e's lock held. The
// engine's workspace and staging may be shared with other threads (the default engine's are):
// enqueueing is serialised per engine, the GPU work is ordered through ws_ready.
// e is not NULL (the device entries, which refuse a NULL engine among their argument errors).
template <class F>
int with_engine(bicos_engine* e, F&& f) {
    return guarded([&]() -> int {
        std::lock_guard<std::mutex> g(e->lock);
        return f(e);
    });
}

// ... and with a NULL e replaced by the current device's default engine (the host entries)
template <class F>
int with_default_engine(bicos_engine* e, F&& f) {
    return guarded([&]() -> int {
        if (!e) {
            int dev = 0;
            if (int rc = check_hip(hipGetDevice(&dev), "hipGetDevice")) return rc;
            e = default_engine(dev);
            if (!e) return (int)BICOS_E_HIP;  // bicos_last_error says why
        }
        std::lock_guard<std::mutex> g(e->lock);
        return f(e);
    });
}

int match_device_entry(bicos_engine* e, const void* stack0, const void* stack1, int n, int rows,
                       int cols, size_t row_pitch, size_t plane_pitch, int depth,
                       const BicosConfig* cfg, int has_nxcorr, void* disparity, void* corrmap,
                       void* stream, bool disp_i16, const DispRange* range = nullptr,
                       const uint32_t* desc0 = nullptr, const uint32_t* desc1 = nullptr) {
    if (range)
        if (int rc0 = check_range(range->min, range->max)) return rc0;
    if (!cfg) return fail(BICOS_E_ARG, "null config");
    if (!e) return fail(BICOS_E_ARG, "null engine");
    return with_engine(e, [&](bicos_engine* e) -> int {
        return match_device(e, stack0, stack1, n, rows, cols, row_pitch, plane_pitch, depth, *cfg,
                            has_nxcorr != 0, nxc_threshold(*cfg), disparity, corrmap,
                            (hipStream_t)stream, disp_i16, desc0, desc1, range);
    });
}

int match_host_entry(bicos_engine* e, const void* const* stack0, const void* const* stack1, int n,
                     int rows, int cols, size_t step, int depth, const BicosConfig* cfg,
                     int has_nxcorr, void* disparity, void* corrmap, const DispRange* range) {
    if (range)
        if (int rc0 = check_range(range->min, range->max)) return rc0;
    if (!cfg) return fail(BICOS_E_ARG, "null config");
    if (n < 0) return fail(BICOS_E_ARG, "negative stack size");
    return with_default_engine(e, [&](bicos_engine* e) -> int {
        const std::vector<size_t> steps((size_t)n, step ? step : (size_t)(cols > 0 ? cols : 0) * depth);
        return match_host(e, stack0, steps.data(), stack1, steps.data(), n, rows, cols, depth, *cfg,
                          has_nxcorr != 0, nxc_threshold(*cfg), disparity, corrmap, range);
    });
}

// bicos_search_device[_range]: the search stage of a match (search_plan, run_search) over the
// caller's descriptors. Only two-pass Consistency needs the engine, for its two maps.
int search_entry(bicos_engine* e, const uint32_t* desc0, const uint32_t* desc1, int rows, int cols,
                 int words, int flags, int max_lr_diff, const DispRange* range, int16_t* out,
                 void* stream) {
    if (int rc0 = check_words(words)) return rc0;
    if (cols > 32767) return fail(BICOS_E_ARG, "image width exceeds 32767");
    const bool empty = rows <= 0 || cols <= 0;
    if (empty && !range) return BICOS_OK;
    const int bits = (flags >> 16) & 0x1FF;  // 0 = all descriptor bits may be set
    const SearchPlan plan = search_plan(e, rows, cols, words, bits, bits, (flags & 1) != 0,
                                        (flags & 2) != 0, range != nullptr);
    if (plan.two_pass && !e)
        return fail(BICOS_E_ARG, "consistency search needs an engine workspace");
    if (empty) return BICOS_OK;
    hipStream_t st = (hipStream_t)stream;
    const SearchJob job{desc0, desc1, rows, cols, words, bits, bits, (flags & 1) != 0,
                        max_lr_diff, range};
    if (!plan.two_pass) return run_search(e, plan, SearchBuffers{}, job, out, st);
    std::lock_guard<std::mutex> lk(e->lock);  // the workspace may be shared (default engine)
    Lease ws(e, e->ws, e->ws_bytes, st);
    search_buffers(ws, plan, rows, cols);
    if (int rc = ws.acquire()) return rc;
    return run_search(e, plan, search_buffers(ws, plan, rows, cols), job, out, st);
}

int agree_common(bool sub, const int16_t* raw, const void* stack0, const void* stack1, int n,
                 int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
                 float threshold, float step, int has_minvar, float minvar_scaled, float* out,
                 void* corrmap, void* stream, bool dbl = false) {
    if (n > 65 && sub) return fail(BICOS_E_ARG, "subpixel supports n <= 65");
    if (int rc0 = check_stack_shape(n, depth, 0, 0)) return rc0;
    if (sub && !(step > 0 && std::isfinite(step)))
        return fail(BICOS_E_ARG, "subpixel_step must be a positive finite number");
    const int nsteps = sub ? subpixel_steps(step) : 0;
    if (sub && !nsteps)
        return fail(BICOS_E_ARG, "subpixel_step too small (more than 65536 interpolation steps)");
    uint32_t span = 0;
    if (int rc0 = stack_span(n, rows, cols, row_pitch, plane_pitch, depth, &span)) return rc0;
    const bicos_hip::AgreeArgs aa =
        agree_args(raw, stack0, stack1, n, rows, cols, row_pitch, plane_pitch, span, threshold,
                   step, nsteps, has_minvar, minvar_scaled, out, true, corrmap);
    hipStream_t st = (hipStream_t)stream;
    return sub ? check_hip(bicos_hip::launch_subpixel(aa, depth, dbl, st), "subpixel launch")
               : check_hip(bicos_hip::launch_agree(aa, depth, dbl, st), "agree launch");
}

}  // namespace

extern "C" {

const char* bicos_last_error(void) { return bicos_impl::last_error(); }

int bicos_engine_create(int device, bicos_engine** out) {
    if (!out) return fail(BICOS_E_ARG, "null out");
    *out = nullptr;
    int count = 0;
    int rc = check_hip(hipGetDeviceCount(&count), "hipGetDeviceCount");
    if (rc) return rc;
    if (device < 0 || device >= count) return fail(BICOS_E_ARG, "no such HIP device");
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(device);
    auto* e = new bicos_engine();
    e->device = device;
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) ==
            hipSuccess &&
        lds > 0) {
        // keep the per-workgroup right-row stage <= 64 KiB so >= 2 workgroups fit per CU
        e->max_lds = lds < 64 * 1024 ? lds : 64 * 1024;
        e->lds_limit = lds;
    }
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
        cus > 0)
        e->cus = cus;
    rc = ensure_stream(e->own_stream);
    if (!rc) rc = ensure_stream(e->copy_stream);
    if (!rc)
        rc = check_hip(hipEventCreateWithFlags(&e->ws_ready, hipEventDisableTiming),
                       "hipEventCreate");
    (void)hipSetDevice(cur);
    if (rc) {
        free_resources(e);
        delete e;
        return rc;
    }
    *out = e;
    return BICOS_OK;
}

bicos_engine* bicos_engine_default(int device) { return default_engine(device); }

void bicos_engine_destroy(bicos_engine* e) {
    if (!e) return;
    if (is_default_engine(e)) return;  // the process-wide engines live until exit
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    // workspaces come from the stream-ordered allocator (reserve)
    if (e->ws) (void)hipFreeAsync(e->ws, e->own_stream);
    if (e->stage) (void)hipFreeAsync(e->stage, e->own_stream);
    if (e->pyr) (void)hipFreeAsync(e->pyr, e->own_stream);
    (void)hipStreamSynchronize(e->own_stream);
    free_resources(e);
    (void)hipSetDevice(cur);
    delete e;
}

int bicos_engine_tune(bicos_engine* e, int variant, int col0_per_lane, int waves, int split) {
    if (!e) return fail(BICOS_E_ARG, "null engine");
    if (variant >= 64 && variant <= 68) {
        // matrix-core search (64 auto keys, 65 one product + xor keys, 66 two products, 67
        // xor keys for first-minimum searches too, no FK keys, 68 packed keys where they
        // apply -- the automatic choice);
        // col0_per_lane = 32-column tiles per wave
        if (col0_per_lane != 0 && col0_per_lane != 2 && col0_per_lane != 4 && col0_per_lane != 8)
            return fail(BICOS_E_ARG, "variant 64-68: tiles per wave 2|4|8");
        if (waves < 0 || waves > 8) return fail(BICOS_E_ARG, "waves 1..8");
        if (split < 0 || split > 160) return fail(BICOS_E_ARG, "variant 64-68: split = LDS KiB 0..160");
    } else {
        if (variant != 0 && variant != 16) return fail(BICOS_E_ARG, "variant 0|16|64..68");
        if (col0_per_lane != 0 && col0_per_lane != 2 && col0_per_lane != 4)
            return fail(BICOS_E_ARG, "col0_per_lane: 2|4 (variant 16)");
        if (waves < 0 || waves > 8) return fail(BICOS_E_ARG, "waves 1..8");
        if (split != 0 && split != 1 && split != 2 && split != 4 && split != 8)
            return fail(BICOS_E_ARG, "split 1|2|4|8");
        if (split > 1 && (waves ? waves : 8) % split)
            return fail(BICOS_E_ARG, "split needs waves divisible by split");
    }
    e->tune_variant = variant;
    e->tune_R = col0_per_lane;
    e->tune_waves = waves;
    e->tune_split = split;
    return BICOS_OK;
}

int bicos_descriptor_words(int n, int mode) {
    if (n < 2) return fail(BICOS_E_ARG, "need at least two images");
    const int w = descriptor_words(n, mode ? 1 : 0);
    if (w < 0) return fail(BICOS_E_BITS, "input stacks too large");
    return w;
}

int bicos_output_type(const BicosConfig* cfg, int has_nxcorr) {
    (void)cfg;
    return has_nxcorr ? BICOS_CV_32F : BICOS_CV_16S;
}

size_t bicos_desc_pitch(int cols, int words) {
    return ((size_t)cols * words + 3) / 4 * 4;
}

int bicos_match_device(bicos_engine* e, const void* stack0, const void* stack1, int n, int rows,
                       int cols, size_t row_pitch, size_t plane_pitch, int depth,
                       const BicosConfig* cfg, int has_nxcorr, void* disparity, void* corrmap,
                       void* stream) {
    return match_device_entry(e, stack0, stack1, n, rows, cols, row_pitch, plane_pitch, depth, cfg,
                              has_nxcorr, disparity, corrmap, stream, false);
}

int bicos_match_device_range(bicos_engine* e, const void* stack0, const void* stack1, int n,
                             int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
                             const BicosConfig* cfg, int has_nxcorr, int min_disparity,
                             int max_disparity, void* disparity, void* corrmap, void* stream) {
    const DispRange range{min_disparity, max_disparity};
    return match_device_entry(e, stack0, stack1, n, rows, cols, row_pitch, plane_pitch, depth, cfg,
                              has_nxcorr, disparity, corrmap, stream, false, &range);
}

int bicos_match_device_i16(bicos_engine* e, const void* stack0, const void* stack1, int n, int rows,
                           int cols, size_t row_pitch, size_t plane_pitch, int depth,
                           const BicosConfig* cfg, int has_nxcorr, void* disparity, void* corrmap,
                           void* stream) {
    return match_device_entry(e, stack0, stack1, n, rows, cols, row_pitch, plane_pitch, depth, cfg,
                              has_nxcorr, disparity, corrmap, stream, true);
}

int bicos_match_plan(bicos_engine* e, const void* stack0, const void* stack1, int n, int rows,
                     int cols, size_t row_pitch, size_t plane_pitch, int depth,
                     const BicosConfig* cfg, int has_nxcorr) {
    if (!cfg) return fail(BICOS_E_ARG, "null config");
    if (int rc0 = check_stack_shape(n, depth, 0, 0)) return rc0;  // (any rows / cols plan)
    if (descriptor_words(n, cfg->mode ? 1 : 0) < 0) return fail(BICOS_E_BITS, "input stacks too large");
    return match_plan(e, n, rows, cols, row_pitch, plane_pitch, depth, *cfg, has_nxcorr != 0,
                      stack0, stack1).bits();
}

int bicos_search_packed(bicos_engine* e, int rows, int cols, int words, int bits, int n, int fused) {
    return search_runs_packed(e, rows, cols, words, bits, n, fused != 0) ? 1 : 0;
}

int bicos_search_packed_product(int bit) {
    return bit >= 0 && bit < 128 ? bicos_hip::pkp_bit_product(bit) : -1;
}

int bicos_agree_kernel(const void* stack0, const void* stack1, int n, size_t row_pitch,
                       size_t plane_pitch, int depth) {
    if (int rc0 = check_stack_shape(n, depth, 0, 0)) return rc0;
    bicos_hip::AgreeArgs aa{};
    aa.stack0 = stack0;
    aa.stack1 = stack1;
    aa.n = n;
    aa.row_pitch = row_pitch;
    aa.plane_pitch = plane_pitch;
    return bicos_hip::agree_kernel_kind(aa, depth);
}

int bicos_transform_kernel(const void* stack0, const void* stack1, int n, int rows, int cols,
                           size_t row_pitch, size_t plane_pitch, int depth, int mode, int words) {
    if (int rc0 = check_stack_shape(n, depth, 0, 0)) return rc0;
    if (int rc0 = check_words(words)) return rc0;
    uint32_t span = 0;
    if (int rc0 = stack_span(n, rows, cols, row_pitch, plane_pitch, depth, &span)) return rc0;
    bicos_hip::TransformArgs ta{};
    ta.stack0 = stack0;
    ta.stack1 = stack1;
    ta.n = n;
    ta.rows = rows;
    ta.cols = cols;
    ta.row_pitch = row_pitch;
    ta.plane_pitch = plane_pitch;
    ta.stack_bytes = span;
    return bicos_hip::transform_kernel_kind(ta, depth, mode ? 1 : 0, words);
}

int bicos_search_agree_device(bicos_engine* e, const uint32_t* desc0, const uint32_t* desc1,
                              const void* stack0, const void* stack1, int n, int rows, int cols,
                              size_t row_pitch, size_t plane_pitch, int depth,
                              const BicosConfig* cfg, int has_nxcorr, void* disparity,
                              void* corrmap, void* stream) {
    if (!cfg) return fail(BICOS_E_ARG, "null config");
    if (!e) return fail(BICOS_E_ARG, "null engine");
    if (rows > 0 && cols > 0 && (!desc0 || !desc1)) return fail(BICOS_E_ARG, "null descriptors");
    return match_device_entry(e, stack0, stack1, n, rows, cols, row_pitch, plane_pitch, depth, cfg,
                              has_nxcorr, disparity, corrmap, stream, false, nullptr, desc0, desc1);
}

int bicos_match_host(bicos_engine* e, const void* const* stack0, const void* const* stack1, int n,
                     int rows, int cols, size_t step, int depth, const BicosConfig* cfg,
                     int has_nxcorr, void* disparity, void* corrmap) {
    return match_host_entry(e, stack0, stack1, n, rows, cols, step, depth, cfg, has_nxcorr,
                            disparity, corrmap, nullptr);
}

int bicos_match_host_range(bicos_engine* e, const void* const* stack0, const void* const* stack1,
                           int n, int rows, int cols, size_t step, int depth,
                           const BicosConfig* cfg, int has_nxcorr, int min_disparity,
                           int max_disparity, void* disparity, void* corrmap) {
    const DispRange range{min_disparity, max_disparity};
    return match_host_entry(e, stack0, stack1, n, rows, cols, step, depth, cfg, has_nxcorr,
                            disparity, corrmap, &range);
}

int bicos_transform_device(const void* stack, int n, int rows, int cols, size_t row_pitch,
                           size_t plane_pitch, int depth, int mode, int words, uint32_t* desc,
                           void* stream) {
    if (int rc0 = check_stack_shape(n, depth, 0, 0)) return rc0;
    if (int rc0 = check_words(words)) return rc0;
    const int need = descriptor_words(n, mode ? 1 : 0);
    if (need < 0 || need > words) return fail(BICOS_E_BITS, "descriptor too narrow for n");
    uint32_t span = 0;
    if (int rc0 = stack_span(n, rows, cols, row_pitch, plane_pitch, depth, &span)) return rc0;
    bicos_hip::TransformArgs ta{stack, nullptr, desc, nullptr, n, rows, cols,
                                row_pitch, plane_pitch, bicos_desc_pitch(cols, words), 0, span};
    return check_hip(bicos_hip::launch_transform(ta, depth, mode ? 1 : 0, words, (hipStream_t)stream),
                     "transform launch");
}

int bicos_search_device(bicos_engine* e, const uint32_t* desc0, const uint32_t* desc1, int rows,
                        int cols, int words, int flags, int max_lr_diff, int16_t* out,
                        void* stream) {
    return search_entry(e, desc0, desc1, rows, cols, words, flags, max_lr_diff, nullptr, out,
                        stream);
}

int bicos_search_device_range(bicos_engine* e, const uint32_t* desc0, const uint32_t* desc1,
                              int rows, int cols, int words, int flags, int max_lr_diff,
                              int min_disparity, int max_disparity, int16_t* out, void* stream) {
    if (int rc0 = check_range(min_disparity, max_disparity)) return rc0;
    const DispRange range{min_disparity, max_disparity};
    return search_entry(e, desc0, desc1, rows, cols, words, flags, max_lr_diff, &range, out,
                        stream);
}

int bicos_search_device_guided(bicos_engine* e, const uint32_t* desc0, const uint32_t* desc1,
                               int rows, int cols, int words, int flags, int max_lr_diff,
                               int min_disparity, int max_disparity, const int16_t* guide,
                               size_t guide_pitch, int16_t* out, void* stream) {
    if (int rc0 = check_guide(guide, guide_pitch, cols, min_disparity, max_disparity)) return rc0;
    const DispRange range{min_disparity, max_disparity, guide, guide_pitch};
    return search_entry(e, desc0, desc1, rows, cols, words, flags, max_lr_diff, &range, out,
                        stream);
}

int bicos_match_device_guided(bicos_engine* e, const void* stack0, const void* stack1, int n,
                              int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
                              const BicosConfig* cfg, int has_nxcorr, int min_disparity,
                              int max_disparity, const int16_t* guide, size_t guide_pitch,
                              void* disparity, void* corrmap, void* stream) {
    if (int rc0 = check_guide(guide, guide_pitch, cols, min_disparity, max_disparity)) return rc0;
    const DispRange range{min_disparity, max_disparity, guide, guide_pitch};
    return match_device_entry(e, stack0, stack1, n, rows, cols, row_pitch, plane_pitch, depth, cfg,
                              has_nxcorr, disparity, corrmap, stream, false, &range);
}

int bicos_match_host_guided(bicos_engine* e, const void* const* stack0, const void* const* stack1,
                            int n, int rows, int cols, size_t step, int depth,
                            const BicosConfig* cfg, int has_nxcorr, int min_disparity,
                            int max_disparity, const int16_t* guide, size_t guide_pitch,
                            void* disparity, void* corrmap) {
    if (int rc0 = check_guide(guide, guide_pitch, cols, min_disparity, max_disparity)) return rc0;
    const DispRange range{min_disparity, max_disparity, guide, guide_pitch};
    return match_host_entry(e, stack0, stack1, n, rows, cols, step, depth, cfg, has_nxcorr,
                            disparity, corrmap, &range);
}

int bicos_guide_device(bicos_engine* e, const void* prior, int prior_type, int prows, int pcols,
                       int rows, int cols, int scale, int radius, int spread, int fallback_lo,
                       int fallback_hi, int flags, int16_t* guide, size_t guide_pitch,
                       uint32_t* counts, void* stream) {
    const GuideJob job{prior, prior_type, prows, pcols, rows, cols, scale, radius, spread,
                       fallback_lo, fallback_hi, flags, guide, guide_pitch, counts};
    if (int rc0 = check_guide_job(job)) return rc0;
    (void)e;  // no workspace: nothing of the engine is used, so it may be NULL and is not locked
    return guarded([&]() -> int { return guide_device(job, (hipStream_t)stream); });
}

int bicos_guide_host(bicos_engine* e, const void* prior, int prior_type, int prows, int pcols,
                     int rows, int cols, int scale, int radius, int spread, int fallback_lo,
                     int fallback_hi, int flags, int16_t* guide, size_t guide_pitch,
                     uint32_t counts[2]) {
    const GuideJob job{prior, prior_type, prows, pcols, rows, cols, scale, radius, spread,
                       fallback_lo, fallback_hi, flags, guide, guide_pitch, counts};
    if (int rc0 = check_guide_job(job)) return rc0;
    return with_default_engine(e, [&](bicos_engine* e) { return guide_host(e, job); });
}

int bicos_agree_stage_device(const int16_t* raw, const void* stack0, const void* stack1, int n,
                             int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
                             float threshold, float step, int has_minvar, float minvar_scaled,
                             int precision, float* out, void* corrmap, void* stream) {
    return agree_common(step > 0, raw, stack0, stack1, n, rows, cols, row_pitch, plane_pitch,
                        depth, threshold, step, has_minvar, minvar_scaled, out, corrmap, stream,
                        precision != 0);
}

int bicos_agree_device(const int16_t* raw, const void* stack0, const void* stack1, int n, int rows,
                       int cols, size_t row_pitch, size_t plane_pitch, int depth, float threshold,
                       int has_minvar, float minvar_scaled, float* out, float* corrmap,
                       void* stream) {
    return agree_common(false, raw, stack0, stack1, n, rows, cols, row_pitch, plane_pitch, depth,
                        threshold, 0.f, has_minvar, minvar_scaled, out, corrmap, stream);
}

int bicos_subpixel_device(const int16_t* raw, const void* stack0, const void* stack1, int n,
                          int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
                          float threshold, float step, int has_minvar, float minvar_scaled,
                          float* out, float* corrmap, void* stream) {
    return agree_common(true, raw, stack0, stack1, n, rows, cols, row_pitch, plane_pitch, depth,
                        threshold, step, has_minvar, minvar_scaled, out, corrmap, stream);
}

int bicos_reproject_device(bicos_engine* e, const void* disparity, int disp_type, int rows,
                           int cols, const double Q[16], int flags, float* xyz_map,
                           float* points, int32_t* index, size_t capacity, uint32_t* counts,
                           void* stream) {
    const ReprojectJob job{disparity, disp_type, rows, cols, Q, flags, xyz_map, points, index,
                           capacity, counts};
    if (int rc0 = check_reproject(job, e, true)) return rc0;
    hipStream_t st = (hipStream_t)stream;
    if (!points)  // no workspace: nothing of the engine is used, so it is not locked
        return guarded([&]() -> int { return reproject_device(e, job, st); });
    return with_engine(e, [&](bicos_engine* e) { return reproject_device(e, job, st); });
}

int bicos_reproject_host(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                         const double Q[16], int flags, float* xyz_map, float* points,
                         int32_t* index, size_t capacity, uint32_t counts[4]) {
    const ReprojectJob job{disparity, disp_type, rows, cols, Q, flags, xyz_map, points, index,
                           capacity, counts};
    if (int rc0 = check_reproject(job, e, false)) return rc0;
    return with_default_engine(e, [&](bicos_engine* e) { return reproject_host(e, job); });
}

int bicos_reproject_segment(void) { return bicos_hip::REPROJECT_SEGMENT; }

int bicos_mesh_device(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                      const double Q[16], int flags, float max_diff, float* points, int32_t* index,
                      size_t vertex_capacity, uint32_t* counts, int32_t* triangles,
                      size_t tri_capacity, uint32_t* mesh_counts, int32_t* vertex_map,
                      void* stream) {
    const MeshJob job{disparity, disp_type, rows, cols, Q, flags, max_diff, points, index,
                      vertex_capacity, counts, triangles, tri_capacity, mesh_counts, vertex_map};
    if (int rc0 = check_mesh(job, e, true)) return rc0;
    return with_engine(e, [&](bicos_engine* e) -> int {
        return mesh_device(e, job, (hipStream_t)stream);
    });
}

int bicos_mesh_host(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                    const double Q[16], int flags, float max_diff, float* points, int32_t* index,
                    size_t vertex_capacity, uint32_t counts[4], int32_t* triangles,
                    size_t tri_capacity, uint32_t mesh_counts[4], int32_t* vertex_map) {
    const MeshJob job{disparity, disp_type, rows, cols, Q, flags, max_diff, points, index,
                      vertex_capacity, counts, triangles, tri_capacity, mesh_counts, vertex_map};
    if (int rc0 = check_mesh(job, e, false)) return rc0;
    if (rows == 0 || cols == 0) {  // all counts zero, without an engine or a HIP call
        if (counts) std::fill(counts, counts + 4, 0u);
        if (mesh_counts) std::fill(mesh_counts, mesh_counts + 4, 0u);
        return BICOS_OK;
    }
    return with_default_engine(e, [&](bicos_engine* e) { return mesh_host(e, job); });
}

int bicos_mesh_segment(void) { return bicos_hip::REPROJECT_SEGMENT; }

int bicos_project_device(bicos_engine* e, const float* points, size_t count, const double* R,
                         const double* t, const double K[9], const double* D, int nd, int img_rows,
                         int img_cols, int splat, float tol, const void* image, int img_depth,
                         int channels, size_t img_pitch, int fill, float* uv, float* depth,
                         uint8_t* cls, void* tex, float* depth_map, int32_t* index_map,
                         uint32_t* counts, void* stream) {
    const ProjectJob job{points, count, R, t, K, D, nd, img_rows, img_cols, splat, tol, image,
                         img_depth, channels, img_pitch, fill, uv, depth, cls, tex, depth_map,
                         index_map, counts};
    if (int rc0 = check_project(job, e, true)) return rc0;
    hipStream_t st = (hipStream_t)stream;
    // (no z-buffer: one launch, no workspace, nothing of an engine)
    if (!e) return guarded([&]() -> int { return project_device(nullptr, job, st); });
    return with_engine(e, [&](bicos_engine* e) { return project_device(e, job, st); });
}

int bicos_project_host(bicos_engine* e, const float* points, size_t count, const double* R,
                       const double* t, const double K[9], const double* D, int nd, int img_rows,
                       int img_cols, int splat, float tol, const void* image, int img_depth,
                       int channels, size_t img_pitch, int fill, float* uv, float* depth,
                       uint8_t* cls, void* tex, float* depth_map, int32_t* index_map,
                       uint32_t counts[5]) {
    const ProjectJob job{points, count, R, t, K, D, nd, img_rows, img_cols, splat, tol, image,
                         img_depth, channels, img_pitch, fill, uv, depth, cls, tex, depth_map,
                         index_map, counts};
    if (int rc0 = check_project(job, e, false)) return rc0;
    return with_default_engine(e, [&](bicos_engine* e) { return project_host(e, job); });
}

int bicos_project_group(void) {
    return bicos_hip::PROJECT_THREADS * bicos_hip::PROJECT_PER_LANE;
}

int bicos_speckle_device(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                         int max_size, float max_diff, int flags, void* out, int32_t* labels,
                         uint32_t* counts, void* stream) {
    const SpeckleJob job{disparity, disp_type, rows, cols, max_size, max_diff, flags, out, labels,
                         counts};
    if (int rc0 = check_speckle(job, e, true)) return rc0;
    return with_engine(e, [&](bicos_engine* e) -> int {
        return speckle_device(e, job, (hipStream_t)stream);
    });
}

int bicos_speckle_host(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                       int max_size, float max_diff, int flags, void* out, int32_t* labels,
                       uint32_t counts[4]) {
    const SpeckleJob job{disparity, disp_type, rows, cols, max_size, max_diff, flags, out, labels,
                         counts};
    if (int rc0 = check_speckle(job, e, false)) return rc0;
    return with_default_engine(e, [&](bicos_engine* e) { return speckle_host(e, job); });
}

int bicos_speckle_tile(int* rows, int* cols) {
    if (rows) *rows = bicos_hip::SPECKLE_TILE_ROWS;
    if (cols) *cols = bicos_hip::SPECKLE_TILE_COLS;
    return BICOS_OK;
}

int bicos_rectify_maps_device(const double K[9], const double* D, int nd, const double* R,
                              const double* P, int p_cols, int rows, int cols, float* map_x,
                              float* map_y, void* stream) {
    const RectifyMapsJob job{K, D, nd, R, P, p_cols, rows, cols, map_x, map_y};
    bicos_hip::RectifyCamera cam;
    if (int rc0 = check_rectify_maps(job, &cam)) return rc0;
    return guarded([&]() -> int { return rectify_maps_device(job, cam, (hipStream_t)stream); });
}

int bicos_rectify_maps_host(const double K[9], const double* D, int nd, const double* R,
                            const double* P, int p_cols, int rows, int cols, float* map_x,
                            float* map_y) {
    const RectifyMapsJob job{K, D, nd, R, P, p_cols, rows, cols, map_x, map_y};
    bicos_hip::RectifyCamera cam;
    if (int rc0 = check_rectify_maps(job, &cam)) return rc0;
    return with_default_engine(nullptr,
                               [&](bicos_engine* e) { return rectify_maps_host(e, job, cam); });
}

int bicos_rectify_device(bicos_engine* e, const void* src, int n, int src_rows, int src_cols,
                         size_t src_row_pitch, size_t src_plane_pitch, int depth,
                         const float* map_x, const float* map_y, size_t map_pitch, int rows,
                         int cols, void* dst, size_t dst_row_pitch, size_t dst_plane_pitch,
                         int border, uint8_t* valid, void* stream) {
    (void)e;  // no workspace: one launch on the caller's stream
    const RectifyJob job{src, n, src_rows, src_cols, src_row_pitch, src_plane_pitch, depth,
                         map_x, map_y, map_pitch, rows, cols, dst, dst_row_pitch,
                         dst_plane_pitch, border, valid};
    if (int rc0 = check_rectify(job)) return rc0;
    return guarded([&]() -> int { return rectify_device(job, (hipStream_t)stream); });
}

int bicos_rectify_host(bicos_engine* e, const void* const* src, int n, int src_rows, int src_cols,
                       size_t src_step, int depth, const float* map_x, const float* map_y,
                       size_t map_pitch, int rows, int cols, void* const* dst, size_t dst_step,
                       int border, uint8_t* valid) {
    if (n < 1) return fail(BICOS_E_ARG, "rectify: need at least one image");
    if (depth != 1 && depth != 2)
        return fail(BICOS_E_ARG, "rectify: depth must be 1 (u8) or 2 (u16)");
    if (!src || !dst) return fail(BICOS_E_ARG, "rectify: null image list");
    if (src_step % (size_t)depth || dst_step % (size_t)depth)
        return fail(BICOS_E_ARG, "rectify: a step is not a multiple of the depth");
    const size_t sstep = src_step ? src_step : (size_t)(src_cols > 0 ? src_cols : 0) * depth;
    const size_t dstep = dst_step ? dst_step : (size_t)(cols > 0 ? cols : 0) * depth;
    for (int t = 0; t < n; ++t) {
        // every image through the device entry's checks, as a one-plane stack of its step
        const RectifyJob one{src[t], 1, src_rows, src_cols, sstep / depth, sstep / depth, depth,
                             map_x, map_y, map_pitch, rows, cols, dst[t], dstep / depth,
                             dstep / depth, border, valid};
        if (int rc0 = check_rectify(one)) return rc0;
    }
    const RectifyJob job{src[0], n, src_rows, src_cols, 0, 0, depth, map_x, map_y, map_pitch,
                         rows, cols, dst[0], 0, 0, border, valid};
    return with_default_engine(e, [&](bicos_engine* e) -> int {
        return rectify_host(e, src, sstep, dst, dstep, job);
    });
}

int bicos_rectify_tile(int* rows, int* cols) {
    if (rows) *rows = bicos_hip::RECTIFY_TILE_ROWS;
    if (cols) *cols = bicos_hip::RECTIFY_TILE_COLS;
    return BICOS_OK;
}

int bicos_median_device(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                        int ksize, int fill_min, int flags, void* out, uint32_t* counts,
                        void* stream) {
    const MedianJob job{disparity, disp_type, rows, cols, ksize, fill_min, flags, out, counts};
    if (int rc0 = check_median(job, true)) return rc0;
    (void)e;  // no workspace: nothing of the engine is used, so it may be NULL and is not locked
    return guarded([&]() -> int { return median_device(job, (hipStream_t)stream); });
}

int bicos_median_host(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                      int ksize, int fill_min, int flags, void* out, uint32_t counts[4]) {
    const MedianJob job{disparity, disp_type, rows, cols, ksize, fill_min, flags, out, counts};
    if (int rc0 = check_median(job, false)) return rc0;
    return with_default_engine(e, [&](bicos_engine* e) { return median_host(e, job); });
}

int bicos_median_tile(int* rows, int* cols) {
    if (rows) *rows = bicos_hip::MEDIAN_TILE_ROWS;
    if (cols) *cols = bicos_hip::MEDIAN_TILE_COLS;
    return BICOS_OK;
}

int bicos_normals_device(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                         const double Q[16], int flags, int radius, float max_diff, int min_points,
                         float* normal_map, const int32_t* index, size_t count, float* normals,
                         uint32_t* counts, void* stream) {
    const NormalsJob job{disparity, disp_type, rows, cols, Q, flags, radius, max_diff, min_points,
                         normal_map, index, count, normals, counts};
    if (int rc0 = check_normals(job)) return rc0;
    (void)e;  // no workspace: nothing of the engine is used, so it may be NULL and is not locked
    return guarded([&]() -> int { return normals_device(job, (hipStream_t)stream); });
}

int bicos_normals_host(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                       const double Q[16], int flags, int radius, float max_diff, int min_points,
                       float* normal_map, const int32_t* index, size_t count, float* normals,
                       uint32_t counts[4]) {
    const NormalsJob job{disparity, disp_type, rows, cols, Q, flags, radius, max_diff, min_points,
                         normal_map, index, count, normals, counts};
    if (int rc0 = check_normals(job)) return rc0;
    if (rows == 0 || cols == 0) {
        // no map, and every list entry lies outside it: nothing to run, no engine to find
        if (counts) std::fill(counts, counts + 4, 0u);
        if (normals) std::fill(normals, normals + count * 3, std::numeric_limits<float>::quiet_NaN());
        return BICOS_OK;
    }
    return with_default_engine(e, [&](bicos_engine* e) { return normals_host(e, job); });
}

int bicos_normals_tile(int* rows, int* cols) {
    if (rows) *rows = bicos_hip::NORMALS_TILE_ROWS;
    if (cols) *cols = bicos_hip::NORMALS_TILE_COLS;
    return BICOS_OK;
}

int bicos_pool_device(bicos_engine* e, const void* src, int n, int rows, int cols,
                      size_t src_row_pitch, size_t src_plane_pitch, int depth, int scale,
                      void* dst, size_t dst_row_pitch, size_t dst_plane_pitch, void* stream) {
    (void)e;  // no workspace: one launch on the caller's stream
    const PoolJob job{src, n, rows, cols, src_row_pitch, src_plane_pitch, depth, scale,
                      dst, dst_row_pitch, dst_plane_pitch};
    if (int rc0 = check_pool(job)) return rc0;
    return guarded([&]() -> int { return pool_device(job, (hipStream_t)stream); });
}

int bicos_pool_host(bicos_engine* e, const void* const* src, int n, int rows, int cols,
                    size_t src_step, int depth, int scale, void* const* dst, size_t dst_step) {
    if (n < 1) return fail(BICOS_E_ARG, "pool: need at least one image");
    if (depth != 1 && depth != 2) return fail(BICOS_E_ARG, "pool: depth must be 1 (u8) or 2 (u16)");
    if (!src || !dst) return fail(BICOS_E_ARG, "pool: null image list");
    if (src_step % (size_t)depth || dst_step % (size_t)depth)
        return fail(BICOS_E_ARG, "pool: a step is not a multiple of the depth");
    const int pcols = scale >= 1 && cols > 0 ? cols / scale : 0;
    const size_t sstep = src_step ? src_step : (size_t)(cols > 0 ? cols : 0) * depth;
    const size_t dstep = dst_step ? dst_step : (size_t)pcols * depth;
    for (int t = 0; t < n; ++t) {
        // every image through the device entry's checks but the overlap (both sides are staged),
        // as a one-plane stack of its step
        const PoolJob one{src[t], 1, rows, cols, sstep / depth, sstep / depth, depth, scale,
                          nullptr, 0, 0};
        if (int rc0 = check_pool(one, false)) return rc0;
        if (dstep / depth < (size_t)pcols)
            return fail(BICOS_E_ARG, "pool: an output pitch is smaller than a row");
        if (!dst[t]) return fail(BICOS_E_ARG, "pool: null output stack");
    }
    const PoolJob job{src[0], n, rows, cols, 0, 0, depth, scale, dst[0], 0, 0};
    return with_default_engine(e, [&](bicos_engine* e) -> int {
        return pool_host(e, src, sstep, dst, dstep, job);
    });
}

int bicos_pool_tile(int* rows, int* cols) {
    if (rows) *rows = bicos_hip::POOL_TILE_ROWS;
    if (cols) *cols = bicos_hip::POOL_TILE_COLS;
    return BICOS_OK;
}

int bicos_pool_kernel(const void* src, size_t src_row_pitch, size_t src_plane_pitch, int depth,
                      const void* dst, size_t dst_row_pitch, size_t dst_plane_pitch) {
    if (depth != 1 && depth != 2) return fail(BICOS_E_ARG, "pool: depth must be 1 (u8) or 2 (u16)");
    bicos_hip::PoolArgs a{};
    a.src = src;
    a.dst = (void*)dst;
    a.src_row_pitch = (uint32_t)src_row_pitch;
    a.dst_row_pitch = (uint32_t)dst_row_pitch;
    a.src_plane_pitch = src_plane_pitch;
    a.dst_plane_pitch = dst_plane_pitch;
    return (bicos_hip::pool_wide(a, depth) ? 1 : 0) | (bicos_hip::pool_dst_vector(a, depth) ? 2 : 0);
}

int bicos_pyramid_window(int min_disparity, int max_disparity, int scale, int* lo, int* hi) {
    if (scale < bicos_hip::POOL_MIN_SCALE || scale > bicos_hip::POOL_MAX_SCALE)
        return fail(BICOS_E_ARG, "pool: scale must lie in 2 .. 8");
    if (!lo || !hi) return fail(BICOS_E_ARG, "null out");
    pyramid_window(min_disparity, max_disparity, scale, lo, hi);
    return BICOS_OK;
}

int bicos_match_device_pyramid(bicos_engine* e, const void* stack0, const void* stack1, int n,
                               int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
                               const BicosConfig* cfg, int has_nxcorr, int min_disparity,
                               int max_disparity, int scale, int radius, int spread,
                               int fallback_lo, int fallback_hi, void* disparity, void* corrmap,
                               void* coarse, int16_t* guide, uint32_t* counts, void* stream) {
    if (!cfg) return fail(BICOS_E_ARG, "null config");
    const DispRange range{min_disparity, max_disparity};
    const PyramidJob job{scale, radius, spread, fallback_lo, fallback_hi, coarse, guide, counts};
    if (int rc0 = check_pyramid(stack0, stack1, n, rows, cols, row_pitch, plane_pitch, depth, *cfg,
                                has_nxcorr != 0, range, job, disparity))
        return rc0;
    if (!e) return fail(BICOS_E_ARG, "null engine");
    return with_engine(e, [&](bicos_engine* e) -> int {
        return match_pyramid_device(e, stack0, stack1, n, rows, cols, row_pitch, plane_pitch,
                                    depth, *cfg, has_nxcorr != 0, nxc_threshold(*cfg), range, job,
                                    disparity, corrmap, (hipStream_t)stream);
    });
}

int bicos_match_host_pyramid(bicos_engine* e, const void* const* stack0, const void* const* stack1,
                             int n, int rows, int cols, size_t step, int depth,
                             const BicosConfig* cfg, int has_nxcorr, int min_disparity,
                             int max_disparity, int scale, int radius, int spread, int fallback_lo,
                             int fallback_hi, void* disparity, void* corrmap, void* coarse,
                             int16_t* guide, uint32_t counts[2]) {
    if (!cfg) return fail(BICOS_E_ARG, "null config");
    if (n < 1) return fail(BICOS_E_ARG, "pool: need at least one image");
    if (depth != 1 && depth != 2)
        return fail(BICOS_E_ARG, "bad input depths, only CV_8UC1 and CV_16UC1 are supported");
    if (!stack0 || !stack1) return fail(BICOS_E_ARG, "null buffer");
    if (step % (size_t)depth) return fail(BICOS_E_ARG, "image step is not a multiple of the depth");
    const size_t row = step ? step : (size_t)(cols > 0 ? cols : 0) * depth;
    const DispRange range{min_disparity, max_disparity};
    const PyramidJob job{scale, radius, spread, fallback_lo, fallback_hi, coarse, guide, counts};
    for (int t = 0; t < n; ++t) {
        if (!stack0[t] || !stack1[t]) return fail(BICOS_E_ARG, "null image");
        if (row < (size_t)(cols > 0 ? cols : 0) * depth)
            return fail(BICOS_E_ARG, "image step smaller than a row");
    }
    // the device entry's checks on the stacks as they will lie in the staging: dense
    if (int rc0 = check_pyramid(stack0[0], stack1[0], n, rows, cols, (size_t)(cols > 0 ? cols : 0),
                                (size_t)(rows > 0 ? rows : 0) * (size_t)(cols > 0 ? cols : 0),
                                depth, *cfg, has_nxcorr != 0, range, job, disparity))
        return rc0;
    return with_default_engine(e, [&](bicos_engine* e) -> int {
        return match_pyramid_host(e, stack0, stack1, row, n, rows, cols, depth, *cfg,
                                  has_nxcorr != 0, nxc_threshold(*cfg), range, job, disparity,
                                  corrmap);
    });
}

const char* bicos_build_info(void) {
    return "libbicos_amd: gfx950 HIP kernels (transform, mx search: FP4 MFMA Hamming products "
           "with argmin keys in the accumulator [default], LDS-broadcast popcount/argmin VALU "
           "search, NXC agree/subpixel), -O3 -ffp-contract=off";
}

}  // extern "C"
