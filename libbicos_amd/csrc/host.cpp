// host.cpp -- the banded host-buffer pipeline: bicos_impl::match_host and its thread pool
// (the reference's cv::Mat path, src/impl/cpu.cpp:100-159).
#include "engine.hpp"
#include "host_plan.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace bicos_impl {

HostPool::HostPool(int threads) {
    for (int i = 1; i < threads; ++i) workers_.emplace_back([this] { loop(); });
}

HostPool::~HostPool() {
    {
        std::lock_guard<std::mutex> g(m_);
        stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
}

void HostPool::loop() {
    unsigned seen = 0;
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
        cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen_;
        ++active_;
        while (next_ < tasks_) {
            const int i = next_++;
            const std::function<void(int)>* f = job_;
            lk.unlock();
            (*f)(i);
            lk.lock();
        }
        if (--active_ == 0) done_.notify_all();
    }
}

void HostPool::run(int tasks, const std::function<void(int)>& f) {
    std::unique_lock<std::mutex> lk(m_);
    job_ = &f;
    tasks_ = tasks;
    next_ = 0;
    ++gen_;
    cv_.notify_all();
    ++active_;
    while (next_ < tasks_) {
        const int i = next_++;
        lk.unlock();
        f(i);
        lk.lock();
    }
    --active_;
    done_.wait(lk, [&] { return active_ == 0; });
    job_ = nullptr;
    tasks_ = 0;
}

namespace {

// Transfers (measured, tools/host_bench.py): a thread pool gathers each band of the
// caller's images into a pinned slot and one DMA per band uploads it (5-7 ms per cfg2
// match, PCIe-bound: 207 MB at 35-42 GB/s while the gathers run; pageable
// hipMemcpy2DAsync per band and plane: ~11 ms).
// Round 6 (profiles/host_path_r06.jsonl, host_trace_r06*.txt): each band's
// upload is split over two copy streams, and the maps come down band by band on a third
// stream into pinned memory as each band's match ends, then into the caller's buffers by
// the pool -- 4.40-4.52 ms per cfg2 match against 5.45-5.79 with one upload stream and one
// download at the end (two rounds interleaved on one box; either change alone was not
// consistent: 4.86-7.29 / 4.98-5.41 ms). BICOS_HOST_UPLOAD_STREAMS=1 / BICOS_HOST_DL=once:
// the round-5 pipeline.
bool download_by_band() {
    static const bool on = [] {
        const char* v = std::getenv("BICOS_HOST_DL");
        return !(v && !std::strcmp(v, "once"));
    }();
    return on;
}
int upload_streams() {
    static const int k = [] {
        const char* v = std::getenv("BICOS_HOST_UPLOAD_STREAMS");
        return v && std::atoi(v) == 1 ? 1 : 2;
    }();
    return k;
}
bool host_trace() {
    static const bool on = std::getenv("BICOS_HOST_TRACE") != nullptr;
    return on;
}

// One match_host call: its arguments, the band plan, the buffers, and the steps in the
// order match_host runs them.
struct HostMatch {
    bicos_engine* e;
    const void* const* p0;
    const size_t* steps0;
    const void* const* p1;
    const size_t* steps1;
    int n, rows, cols, depth;
    const BicosConfig& cfg;
    bool has_nxcorr;
    float threshold;
    void* disp;
    void* corr;
    const DispRange* range;

    hipStream_t cs, ks;  // compute, copy
    const bool dl_bands = download_by_band();
    const int up_streams = upload_streams();
    // the band plan (plan_bands; the arithmetic is host_plan.hpp's)
    host_plan::BandPlan bands;
    size_t row_bytes = 0, band_bytes = 0, dsz = 0, csz = 0, disp_bytes = 0, corr_bytes = 0;
    int band_rows = 0, B = 0, K = 0;
    // the stage: band-major stacks | disparity | corrmap (carve)
    char *dev = nullptr, *dev_disp = nullptr, *dev_corr = nullptr;
    char *hout_d = nullptr, *hout_c = nullptr;  // pinned maps (dl_bands)
    int16_t* dev_guide = nullptr;  // the whole guide, dense (range->guide set)

    // BICOS_HOST_TRACE=1: per-phase host timestamps on stderr (tools/host_bench.py)
    const bool trace = host_trace();
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    std::vector<std::pair<hipEvent_t, hipEvent_t>> dma_ev;
    void stamp(const char* what, int b) const {
        if (!trace) return;
        const double us = std::chrono::duration<double, std::micro>(
                              std::chrono::steady_clock::now() - t_start).count();
        std::fprintf(stderr, "[bicos host] %8.1f us  %s %d\n", us, what, b);
    }

    void plan_bands() {
        bands = host_plan::plan_bands(rows);
        band_rows = bands.band_rows;
        B = bands.B;
        K = bands.K;  // pinned slots in flight
        row_bytes = (size_t)cols * depth;
        band_bytes = 2 * (size_t)n * band_rows * row_bytes;
        dsz = has_nxcorr ? 4 : 2;
        csz = cfg.precision ? 8 : 4;
        disp_bytes = (size_t)rows * cols * dsz;
        corr_bytes = corr ? (size_t)rows * cols * csz : 0;
    }
    int band_height(int b) const { return bands.height(b); }
    // band b's bytes in its slot and on the device, and whether its upload has a second part
    // (on copy_stream2, with events2[b] recorded behind it)
    size_t band_upload(int b) const { return 2 * (size_t)n * band_height(b) * row_bytes; }
    bool upload_is_split(int b) const {
        const size_t up = band_upload(b);
        return host_plan::upload_first(up, up_streams) < up;
    }

    void carve(Lease& stage) {
        dev = stage.take((size_t)B * band_bytes);
        dev_disp = stage.take(disp_bytes);
        dev_corr = corr ? stage.take(corr_bytes) : nullptr;
        dev_guide = range && range->guide ? stage.take<int16_t>(2 * (size_t)rows * cols) : nullptr;
    }

    // the guide, whole, on the copy stream ahead of the first band's stacks (4 bytes per
    // pixel against the stacks' 2 n: not worth a banded overlap)
    int upload_guide() {
        if (!dev_guide) return BICOS_OK;
        return check_hip(hipMemcpy2DAsync(dev_guide, (size_t)cols * 4, range->guide,
                                          range->guide_pitch * 4, (size_t)cols * 4, (size_t)rows,
                                          hipMemcpyHostToDevice, ks), "guide upload");
    }

    // pinned slots, events, streams and the pool, each on first use / grown only
    int ensure_resources() {
        int rc = grow_pinned(e->pinned, (size_t)K * band_bytes, "hipHostMalloc(staging)");
        if (!rc) rc = grow_events(e->events, B);
        if (rc) return rc;
        if (!e->pool) {
            // gather threads (BICOS_HOST_THREADS, default 8): the gathers compete with the DMA
            // for host memory bandwidth; 16 threads measured slower than 3-8 (tools/host_bench.py)
            const unsigned hw = std::thread::hardware_concurrency();
            const char* th = std::getenv("BICOS_HOST_THREADS");
            const unsigned cap = th ? (unsigned)std::max(1, std::atoi(th)) : 8u;
            e->pool.reset(new HostPool((int)std::max(1u, std::min(cap, hw ? hw : 1u))));
        }
        if (up_streams == 2) {
            rc = ensure_stream(e->copy_stream2);
            if (!rc) rc = grow_events(e->events2, B);
            // earlier calls (possibly on other streams) may still read the stage / workspace
            if (!rc)
                rc = check_hip(hipStreamWaitEvent(e->copy_stream2, e->ws_ready, 0),
                               "hipStreamWaitEvent");
            if (rc) return rc;
        }
        if (dl_bands) {
            rc = ensure_stream(e->dl_stream);
            if (!rc)
                rc = grow_pinned(e->pinned_out, align_up(disp_bytes) + corr_bytes,
                                 "hipHostMalloc(map staging)");
            if (!rc) rc = grow_events(e->dl_events, 2 * B);
            if (rc) return rc;
            hout_d = (char*)e->pinned_out.p;
            hout_c = corr ? hout_d + align_up(disp_bytes) : nullptr;
        }
        return BICOS_OK;
    }

    // band b: gather its 2n planes into a pinned slot, upload the slot, match it
    int upload_and_match(int b) {
        const int r0 = b * band_rows, br = band_height(b);
        const size_t plane = (size_t)br * row_bytes;
        char* slot = (char*)e->pinned.p + (size_t)(b % K) * band_bytes;
        int rc = BICOS_OK;
        if (b >= K) {
            rc = check_hip(hipEventSynchronize(e->events[b - K]), "hipEventSynchronize");
            if (!rc && upload_is_split(b - K))
                rc = check_hip(hipEventSynchronize(e->events2[b - K]), "hipEventSynchronize");
            if (rc) return rc;
        }
        char* band = dev + (size_t)b * band_bytes;
        // 2n planes -> slot [2n][br][cols], dense
        const std::function<void(int)> copy = [&](int i) {
            const bool right = i >= n;
            const int t = right ? i - n : i;
            const size_t step = right ? (steps1 ? steps1[t] : row_bytes)
                                      : (steps0 ? steps0[t] : row_bytes);
            const char* src = (const char*)(right ? p1[t] : p0[t]) + (size_t)r0 * step;
            char* dst = slot + (size_t)i * plane;
            if (step == row_bytes) {
                std::memcpy(dst, src, plane);
            } else {
                for (int r = 0; r < br; ++r)
                    std::memcpy(dst + (size_t)r * row_bytes, src + (size_t)r * step, row_bytes);
            }
        };
        stamp("slot free", b);
        e->pool->run(2 * n, copy);
        stamp("gathered", b);
        hipEvent_t t0 = nullptr, t1 = nullptr;
        if (trace) {
            (void)hipEventCreate(&t0);
            (void)hipEventCreate(&t1);
            (void)hipEventRecord(t0, ks);
        }
        // one copy, or two on two streams: never past the band's own bytes (a band of under
        // 4096 bytes once had a first part of 4096, host_plan.hpp upload_first)
        host_plan::Span part[2];
        const int copies = host_plan::upload_parts(band_upload(b), up_streams, part);
        rc = check_hip(hipMemcpyAsync(band + part[0].offset, slot + part[0].offset, part[0].length,
                                      hipMemcpyHostToDevice, ks), "stack upload");
        if (!rc && copies == 2) {
            rc = check_hip(hipMemcpyAsync(band + part[1].offset, slot + part[1].offset,
                                          part[1].length, hipMemcpyHostToDevice, e->copy_stream2),
                           "stack upload");
            if (!rc) rc = check_hip(hipEventRecord(e->events2[b], e->copy_stream2), "hipEventRecord");
            if (!rc) rc = check_hip(hipStreamWaitEvent(cs, e->events2[b], 0), "hipStreamWaitEvent");
        }
        if (trace) {
            (void)hipEventRecord(t1, ks);
            dma_ev.push_back({t0, t1});
        }
        if (!rc) rc = check_hip(hipEventRecord(e->events[b], ks), "hipEventRecord");
        if (!rc) rc = check_hip(hipStreamWaitEvent(cs, e->events[b], 0), "hipStreamWaitEvent");
        if (rc) return rc;
        // the band's window: the call's, with the band's rows of the uploaded guide
        DispRange band_range = range ? *range : DispRange{0, 0};
        if (dev_guide) {
            band_range.guide = dev_guide + 2 * (size_t)r0 * cols;
            band_range.guide_pitch = (size_t)cols;
        }
        return match_device(e, band, band + (size_t)n * plane, n, br, cols, (size_t)cols,
                            (size_t)br * cols, depth, cfg, has_nxcorr, threshold,
                            dev_disp + (size_t)r0 * cols * dsz,
                            dev_corr ? dev_corr + (size_t)r0 * cols * csz : nullptr, cs, false,
                            nullptr, nullptr, range ? &band_range : nullptr);
    }

    // band b's rows of the maps into pinned memory, as soon as they are matched (dl_bands)
    int download_band(int b) {
        const int r0 = b * band_rows, br = band_height(b);
        hipStream_t ds = e->dl_stream;
        const host_plan::Span d = host_plan::map_rows(r0, br, cols, dsz);
        const host_plan::Span c = host_plan::map_rows(r0, br, cols, csz);
        int rc = check_hip(hipEventRecord(e->dl_events[2 * b], cs), "hipEventRecord");
        if (!rc) rc = check_hip(hipStreamWaitEvent(ds, e->dl_events[2 * b], 0), "hipStreamWaitEvent");
        if (!rc)
            rc = check_hip(hipMemcpyAsync(hout_d + d.offset, dev_disp + d.offset, d.length,
                                          hipMemcpyDeviceToHost, ds), "download");
        if (!rc && corr)
            rc = check_hip(hipMemcpyAsync(hout_c + c.offset, dev_corr + c.offset, c.length,
                                          hipMemcpyDeviceToHost, ds), "download");
        if (!rc) rc = check_hip(hipEventRecord(e->dl_events[2 * b + 1], ds), "hipEventRecord");
        return rc;
    }

    // band b from pinned memory into the caller's buffers once it has landed (the pool: row
    // chunks of both maps)
    int deliver_band(int b) {
        int rc = check_hip(hipEventSynchronize(e->dl_events[2 * b + 1]), "hipEventSynchronize");
        if (rc) return rc;
        const int r0 = b * band_rows, br = band_height(b);
        const int parts = host_plan::DELIVER_PARTS;
        const std::function<void(int)> out = [&](int i) {
            const bool c = i >= parts;
            if (c && !corr) return;
            const host_plan::Span band = host_plan::map_rows(r0, br, cols, c ? csz : dsz);
            const host_plan::Span part = host_plan::deliver_part(band.length, parts, i % parts);
            if (!part.length) return;
            const size_t base = band.offset + part.offset;
            std::memcpy((char*)(c ? corr : disp) + base, (c ? hout_c : hout_d) + base, part.length);
        };
        e->pool->run(2 * parts, out);
        return BICOS_OK;
    }

    // both maps in one copy each at the end (BICOS_HOST_DL=once)
    int download_once() {
        int rc = check_hip(hipMemcpyAsync(disp, dev_disp, disp_bytes, hipMemcpyDeviceToHost, cs),
                           "download");
        if (!rc && corr)
            rc = check_hip(hipMemcpyAsync(corr, dev_corr, corr_bytes, hipMemcpyDeviceToHost, cs),
                           "download");
        return rc;
    }

    // drain every stream whatever happened: the slots and the stage are reused next call
    int drain(int rc) {
        const int r1 = check_hip(hipStreamSynchronize(ks), "hipStreamSynchronize");
        if (up_streams == 2) (void)hipStreamSynchronize(e->copy_stream2);
        const int r2 = check_hip(hipStreamSynchronize(cs), "hipStreamSynchronize");
        const int r3 = dl_bands ? check_hip(hipStreamSynchronize(e->dl_stream), "hipStreamSynchronize")
                                : BICOS_OK;
        stamp("downloaded", B);
        for (size_t i = 0; i < dma_ev.size(); ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, dma_ev[i].first, dma_ev[i].second);
            std::fprintf(stderr, "[bicos host] dma %zu: %.3f ms = %.1f GB/s\n", i, ms,
                         band_bytes / (ms * 1e6));
            (void)hipEventDestroy(dma_ev[i].first);
            (void)hipEventDestroy(dma_ev[i].second);
        }
        return rc ? rc : (r1 ? r1 : (r2 ? r2 : r3));
    }
};

}  // namespace

int match_host(bicos_engine* e, const void* const* p0, const size_t* steps0,
               const void* const* p1, const size_t* steps1, int n, int rows, int cols,
               int depth, const BicosConfig& cfg, bool has_nxcorr, float threshold, void* disp,
               void* corr, const DispRange* range) {
    if (range)
        if (int rc0 = check_range(range->min, range->max)) return rc0;
    if (range && range->guide)
        if (int rc0 = check_guide(range->guide, range->guide_pitch, cols, range->min, range->max))
            return rc0;
    if (!e) return fail(BICOS_E_ARG, "null engine");
    if (int rc0 = check_stack_shape(n, depth, rows, cols)) return rc0;
    if (rows == 0 || cols == 0) {  // validates the configuration, no work
        const DispRange window = range ? DispRange{range->min, range->max} : DispRange{0, 0};
        return match_device(e, nullptr, nullptr, n, rows, cols, (size_t)cols,
                            (size_t)rows * cols, depth, cfg, has_nxcorr, threshold, disp, corr,
                            e->own_stream, false, nullptr, nullptr, range ? &window : nullptr);
    }
    if (!p0 || !p1 || !disp) return fail(BICOS_E_ARG, "null buffer");
    for (int t = 0; t < n; ++t) {
        if (!p0[t] || !p1[t]) return fail(BICOS_E_ARG, "null image");
        if ((steps0 && steps0[t] < (size_t)cols * depth) || (steps1 && steps1[t] < (size_t)cols * depth))
            return fail(BICOS_E_ARG, "image step smaller than a row");
    }
    // (the compute stream is the engine's own, the first upload stream its copy stream)
    HostMatch m{e, p0, steps0, p1, steps1, n, rows, cols, depth, cfg, has_nxcorr, threshold,
                disp, corr, range, e->own_stream, e->copy_stream};
    m.plan_bands();
    Lease stage(e, e->stage, e->stage_bytes, m.ks);
    m.carve(stage);
    int rc = stage.acquire();
    if (!rc) rc = m.ensure_resources();
    if (rc) return rc;
    m.carve(stage);
    rc = m.upload_guide();
    for (int b = 0; b < m.B && !rc; ++b) {
        rc = m.upload_and_match(b);
        if (!rc && m.dl_bands) rc = m.download_band(b);
    }
    m.stamp("bands queued", m.B);
    if (m.trace) {
        (void)hipStreamSynchronize(m.cs);
        m.stamp("bands matched", m.B);
    }
    for (int b = 0; b < m.B && !rc && m.dl_bands; ++b) rc = m.deliver_band(b);
    if (!rc && !m.dl_bands) rc = m.download_once();
    return m.drain(rc);
}

int reproject_host(bicos_engine* e, const ReprojectJob& j) {
    if (!e) return fail(BICOS_E_ARG, "null engine");
    if (int rc0 = check_reproject(j, e, false)) return rc0;
    const size_t pixels = (size_t)j.rows * j.cols;
    if (pixels == 0) {
        if (j.counts) std::fill(j.counts, j.counts + 4, 0u);
        return BICOS_OK;
    }
    hipStream_t st = e->own_stream;
    const size_t esz = j.disp_type == BICOS_CV_32F ? 4 : 2;
    const size_t cap = std::min(j.capacity, pixels);
    ReprojectJob d = j;  // the same job on staged device buffers
    Lease stage(e, e->stage, e->stage_bytes, st);
    auto carve = [&] {
        d.disp = stage.take(pixels * esz);
        d.xyz_map = j.xyz_map ? stage.take<float>(3 * pixels) : nullptr;
        d.points = j.points ? stage.take<float>(3 * cap + 1) : nullptr;  // (non-null at cap 0)
        d.index = j.index ? stage.take<int32_t>(cap + 1) : nullptr;
        d.counts = j.points ? stage.take<uint32_t>(4) : nullptr;
    };
    carve();
    int rc = stage.acquire();
    if (rc) return rc;
    carve();
    d.capacity = cap;
    rc = check_hip(hipMemcpyAsync((void*)d.disp, j.disp, pixels * esz, hipMemcpyHostToDevice, st),
                   "disparity upload");
    if (!rc) rc = reproject_device(e, d, st);
    if (!rc && j.points) {
        rc = check_hip(hipMemcpyAsync(j.counts, d.counts, 4 * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, st), "counts download");
        if (!rc) rc = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
        const size_t got = rc ? 0 : std::min<size_t>(j.counts[0], cap);
        if (!rc && got)
            rc = check_hip(hipMemcpyAsync(j.points, d.points, got * 3 * sizeof(float),
                                          hipMemcpyDeviceToHost, st), "points download");
        if (!rc && got && j.index)
            rc = check_hip(hipMemcpyAsync(j.index, d.index, got * sizeof(int32_t),
                                          hipMemcpyDeviceToHost, st), "index download");
    }
    if (!rc && j.xyz_map)
        rc = check_hip(hipMemcpyAsync(j.xyz_map, d.xyz_map, pixels * 3 * sizeof(float),
                                      hipMemcpyDeviceToHost, st), "xyz map download");
    const int rc2 = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    return rc ? rc : rc2;
}

int mesh_host(bicos_engine* e, const MeshJob& j) {
    if (!e) return fail(BICOS_E_ARG, "null engine");
    if (int rc0 = check_mesh(j, e, false)) return rc0;
    const size_t pixels = (size_t)j.rows * j.cols;
    if (pixels == 0) {
        if (j.counts) std::fill(j.counts, j.counts + 4, 0u);
        if (j.mesh_counts) std::fill(j.mesh_counts, j.mesh_counts + 4, 0u);
        return BICOS_OK;
    }
    hipStream_t st = e->own_stream;
    const size_t esz = j.disp_type == BICOS_CV_32F ? 4 : 2;
    const size_t quads = j.rows < 2 || j.cols < 2 ? 0 : (size_t)(j.rows - 1) * (j.cols - 1);
    const size_t vcap = std::min(j.vertex_capacity, pixels);
    const size_t tcap = std::min(j.tri_capacity, 2 * quads);
    MeshJob d = j;  // the same job on staged device buffers
    Lease stage(e, e->stage, e->stage_bytes, st);
    auto carve = [&] {
        d.disp = stage.take(pixels * esz);
        d.points = stage.take<float>(3 * vcap + 1);  // (non-null at capacity 0)
        d.index = j.index ? stage.take<int32_t>(vcap + 1) : nullptr;
        d.counts = stage.take<uint32_t>(4);
        d.triangles = stage.take<int32_t>(3 * tcap + 1);
        d.mesh_counts = stage.take<uint32_t>(4);
        d.vertex_map = j.vertex_map ? stage.take<int32_t>(pixels) : nullptr;
    };
    carve();
    int rc = stage.acquire();
    if (rc) return rc;
    carve();
    d.vertex_capacity = vcap;
    d.tri_capacity = tcap;
    rc = check_hip(hipMemcpyAsync((void*)d.disp, j.disp, pixels * esz, hipMemcpyHostToDevice, st),
                   "disparity upload");
    if (!rc) rc = mesh_device(e, d, st);
    if (!rc)
        rc = check_hip(hipMemcpyAsync(j.counts, d.counts, 4 * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, st), "counts download");
    if (!rc)
        rc = check_hip(hipMemcpyAsync(j.mesh_counts, d.mesh_counts, 4 * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, st), "mesh_counts download");
    if (!rc) rc = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    const size_t verts = rc ? 0 : std::min<size_t>(j.counts[0], vcap);
    const size_t tris = rc ? 0 : std::min<size_t>(j.mesh_counts[0], tcap);
    if (!rc && verts)
        rc = check_hip(hipMemcpyAsync(j.points, d.points, verts * 3 * sizeof(float),
                                      hipMemcpyDeviceToHost, st), "points download");
    if (!rc && verts && j.index)
        rc = check_hip(hipMemcpyAsync(j.index, d.index, verts * sizeof(int32_t),
                                      hipMemcpyDeviceToHost, st), "index download");
    if (!rc && tris)
        rc = check_hip(hipMemcpyAsync(j.triangles, d.triangles, tris * 3 * sizeof(int32_t),
                                      hipMemcpyDeviceToHost, st), "triangles download");
    if (!rc && j.vertex_map)
        rc = check_hip(hipMemcpyAsync(j.vertex_map, d.vertex_map, pixels * sizeof(int32_t),
                                      hipMemcpyDeviceToHost, st), "vertex_map download");
    const int rc2 = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    return rc ? rc : rc2;
}

int speckle_host(bicos_engine* e, const SpeckleJob& j) {
    if (!e) return fail(BICOS_E_ARG, "null engine");
    if (int rc0 = check_speckle(j, e, false)) return rc0;
    const size_t pixels = (size_t)j.rows * j.cols;
    if (pixels == 0) {
        if (j.counts) std::fill(j.counts, j.counts + 4, 0u);
        return BICOS_OK;
    }
    hipStream_t st = e->own_stream;
    const size_t esz = j.disp_type == BICOS_CV_32F ? 4 : 2;
    SpeckleJob d = j;  // the same job on staged device buffers, filtered in place
    Lease stage(e, e->stage, e->stage_bytes, st);
    auto carve = [&] {
        d.out = stage.take(pixels * esz);
        d.disp = d.out;
        d.labels = j.labels ? stage.take<int32_t>(pixels) : nullptr;
        d.counts = j.counts ? stage.take<uint32_t>(4) : nullptr;
    };
    carve();
    int rc = stage.acquire();
    if (rc) return rc;
    carve();
    rc = check_hip(hipMemcpyAsync(d.out, j.disp, pixels * esz, hipMemcpyHostToDevice, st),
                   "disparity upload");
    if (!rc) rc = speckle_device(e, d, st);
    if (!rc)
        rc = check_hip(hipMemcpyAsync(j.out, d.out, pixels * esz, hipMemcpyDeviceToHost, st),
                       "filtered map download");
    if (!rc && j.labels)
        rc = check_hip(hipMemcpyAsync(j.labels, d.labels, pixels * sizeof(int32_t),
                                      hipMemcpyDeviceToHost, st), "labels download");
    if (!rc && j.counts)
        rc = check_hip(hipMemcpyAsync(j.counts, d.counts, 4 * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, st), "counts download");
    const int rc2 = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    return rc ? rc : rc2;
}

// --------------------------------------------------------------- rectification

int rectify_host(bicos_engine* e, const void* const* src, size_t src_step, void* const* dst,
                 size_t dst_step, const RectifyJob& j) {
    if (!e) return fail(BICOS_E_ARG, "null engine");
    hipStream_t st = e->own_stream;
    const size_t d = (size_t)j.depth;
    const size_t src_row = (size_t)j.src_cols * d, dst_row = (size_t)j.cols * d;
    const size_t map_row = (size_t)j.cols * sizeof(float);
    const size_t src_plane = src_row * j.src_rows, dst_plane = dst_row * j.rows;
    RectifyJob dj = j;  // the same job on dense staged device buffers
    dj.src_row_pitch = (size_t)j.src_cols;
    dj.src_plane_pitch = (size_t)j.src_cols * j.src_rows;
    dj.dst_row_pitch = (size_t)j.cols;
    dj.dst_plane_pitch = (size_t)j.cols * j.rows;
    dj.map_pitch = 0;
    Lease stage(e, e->stage, e->stage_bytes, st);
    char *s = nullptr, *o = nullptr;
    auto carve = [&] {
        s = stage.take(src_plane * j.n);
        o = stage.take(dst_plane * j.n);
        dj.map_x = stage.take<float>((size_t)j.rows * j.cols);
        dj.map_y = stage.take<float>((size_t)j.rows * j.cols);
        dj.valid = j.valid ? stage.take<uint8_t>((size_t)j.rows * j.cols) : nullptr;
    };
    carve();
    int rc = stage.acquire();
    if (rc) return rc;
    carve();
    dj.src = s;
    dj.dst = o;
    for (int t = 0; t < j.n && !rc; ++t)
        rc = check_hip(hipMemcpy2DAsync(s + t * src_plane, src_row, src[t], src_step, src_row,
                                        (size_t)j.src_rows, hipMemcpyHostToDevice, st),
                       "stack upload");
    const size_t mp = j.map_pitch ? j.map_pitch : map_row;
    if (!rc)
        rc = check_hip(hipMemcpy2DAsync((void*)dj.map_x, map_row, j.map_x, mp, map_row,
                                        (size_t)j.rows, hipMemcpyHostToDevice, st), "map upload");
    if (!rc)
        rc = check_hip(hipMemcpy2DAsync((void*)dj.map_y, map_row, j.map_y, mp, map_row,
                                        (size_t)j.rows, hipMemcpyHostToDevice, st), "map upload");
    if (!rc) rc = rectify_device(dj, st);
    for (int t = 0; t < j.n && !rc; ++t)
        rc = check_hip(hipMemcpy2DAsync(dst[t], dst_step, o + t * dst_plane, dst_row, dst_row,
                                        (size_t)j.rows, hipMemcpyDeviceToHost, st),
                       "stack download");
    if (!rc && j.valid)
        rc = check_hip(hipMemcpyAsync(j.valid, dj.valid, (size_t)j.rows * j.cols,
                                      hipMemcpyDeviceToHost, st), "valid download");
    const int rc2 = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    return rc ? rc : rc2;
}

int rectify_maps_host(bicos_engine* e, const RectifyMapsJob& j,
                      const bicos_hip::RectifyCamera& cam) {
    if (!e) return fail(BICOS_E_ARG, "null engine");
    hipStream_t st = e->own_stream;
    const size_t pixels = (size_t)j.rows * j.cols;
    RectifyMapsJob dj = j;
    Lease stage(e, e->stage, e->stage_bytes, st);
    auto carve = [&] {
        dj.map_x = stage.take<float>(pixels);
        dj.map_y = stage.take<float>(pixels);
    };
    carve();
    int rc = stage.acquire();
    if (rc) return rc;
    carve();
    rc = rectify_maps_device(dj, cam, st);
    if (!rc)
        rc = check_hip(hipMemcpyAsync(j.map_x, dj.map_x, pixels * sizeof(float),
                                      hipMemcpyDeviceToHost, st), "map download");
    if (!rc)
        rc = check_hip(hipMemcpyAsync(j.map_y, dj.map_y, pixels * sizeof(float),
                                      hipMemcpyDeviceToHost, st), "map download");
    const int rc2 = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    return rc ? rc : rc2;
}

int median_host(bicos_engine* e, const MedianJob& j) {
    if (!e) return fail(BICOS_E_ARG, "null engine");
    if (int rc0 = check_median(j, false)) return rc0;
    const size_t pixels = (size_t)j.rows * j.cols;
    if (pixels == 0) {
        if (j.counts) std::fill(j.counts, j.counts + 4, 0u);
        return BICOS_OK;
    }
    hipStream_t st = e->own_stream;
    const size_t esz = j.disp_type == BICOS_CV_32F ? 4 : 2;
    // the same job on staged device buffers: two of them, because the launch reads
    // neighbours (which is why the caller's out may be its map)
    MedianJob d = j;
    Lease stage(e, e->stage, e->stage_bytes, st);
    void* map = nullptr;
    auto carve = [&] {
        map = stage.take(pixels * esz);
        d.disp = map;
        d.out = stage.take(pixels * esz);
        d.counts = j.counts ? stage.take<uint32_t>(4) : nullptr;
    };
    carve();
    int rc = stage.acquire();
    if (rc) return rc;
    carve();
    rc = check_hip(hipMemcpyAsync(map, j.disp, pixels * esz, hipMemcpyHostToDevice, st),
                   "disparity upload");
    if (!rc) rc = median_device(d, st);
    if (!rc)
        rc = check_hip(hipMemcpyAsync(j.out, d.out, pixels * esz, hipMemcpyDeviceToHost, st),
                       "filtered map download");
    if (!rc && j.counts)
        rc = check_hip(hipMemcpyAsync(j.counts, d.counts, 4 * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, st), "counts download");
    const int rc2 = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    return rc ? rc : rc2;
}

int normals_host(bicos_engine* e, const NormalsJob& j) {
    if (!e) return fail(BICOS_E_ARG, "null engine");
    if (int rc0 = check_normals(j)) return rc0;
    const size_t pixels = (size_t)j.rows * j.cols;
    const size_t count = j.normals ? j.count : 0;
    if (pixels == 0) return fail(BICOS_E_ARG, "normals: empty map (the entry answers it)");
    hipStream_t st = e->own_stream;
    const size_t esz = j.disp_type == BICOS_CV_32F ? 4 : 2;
    NormalsJob d = j;  // the same job on staged device buffers
    Lease stage(e, e->stage, e->stage_bytes, st);
    void* map = nullptr;
    int32_t* index = nullptr;
    auto carve = [&] {
        map = stage.take(pixels * esz);
        d.disp = map;
        d.normal_map = j.normal_map ? stage.take<float>(pixels * 3) : nullptr;
        index = count ? stage.take<int32_t>(count) : nullptr;
        d.index = index;
        d.normals = count ? stage.take<float>(count * 3) : nullptr;
        d.count = count;
        d.counts = j.counts ? stage.take<uint32_t>(4) : nullptr;
    };
    carve();
    int rc = stage.acquire();
    if (rc) return rc;
    carve();
    rc = check_hip(hipMemcpyAsync(map, j.disp, pixels * esz, hipMemcpyHostToDevice, st),
                   "disparity upload");
    if (!rc && count)
        rc = check_hip(hipMemcpyAsync(index, j.index, count * sizeof(int32_t),
                                      hipMemcpyHostToDevice, st), "index upload");
    if (!rc) rc = normals_device(d, st);
    if (!rc && j.normal_map)
        rc = check_hip(hipMemcpyAsync(j.normal_map, d.normal_map, pixels * 3 * sizeof(float),
                                      hipMemcpyDeviceToHost, st), "normal map download");
    if (!rc && count)
        rc = check_hip(hipMemcpyAsync(j.normals, d.normals, count * 3 * sizeof(float),
                                      hipMemcpyDeviceToHost, st), "normals download");
    if (!rc && j.counts)
        rc = check_hip(hipMemcpyAsync(j.counts, d.counts, 4 * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, st), "counts download");
    const int rc2 = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    return rc ? rc : rc2;
}

int guide_host(bicos_engine* e, const GuideJob& j) {
    if (!e) return fail(BICOS_E_ARG, "null engine");
    if (int rc0 = check_guide_job(j)) return rc0;
    const size_t pixels = (size_t)j.rows * j.cols;
    if (pixels == 0) {
        if (j.counts) std::fill(j.counts, j.counts + 2, 0u);
        return BICOS_OK;
    }
    hipStream_t st = e->own_stream;
    const size_t prior_bytes = (size_t)j.prows * j.pcols * (j.prior_type == BICOS_CV_32F ? 4 : 2);
    const size_t pitch = j.guide_pitch ? j.guide_pitch : (size_t)j.cols;
    GuideJob d = j;  // the same job on staged device buffers, the guide dense
    d.guide_pitch = (size_t)j.cols;
    Lease stage(e, e->stage, e->stage_bytes, st);
    auto carve = [&] {
        d.prior = stage.take(prior_bytes);
        d.guide = stage.take<int16_t>(2 * pixels);
        d.counts = j.counts ? stage.take<uint32_t>(2) : nullptr;
    };
    carve();
    int rc = stage.acquire();
    if (rc) return rc;
    carve();
    rc = check_hip(hipMemcpyAsync((void*)d.prior, j.prior, prior_bytes, hipMemcpyHostToDevice, st),
                   "prior upload");
    if (!rc) rc = guide_device(d, st);
    if (!rc)
        rc = check_hip(hipMemcpy2DAsync(j.guide, pitch * 4, d.guide, (size_t)j.cols * 4,
                                        (size_t)j.cols * 4, (size_t)j.rows, hipMemcpyDeviceToHost,
                                        st), "guide download");
    if (!rc && j.counts)
        rc = check_hip(hipMemcpyAsync(j.counts, d.counts, 2 * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, st), "counts download");
    const int rc2 = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    return rc ? rc : rc2;
}

// --------------------------------------------------------------- stack pooling

int pool_host(bicos_engine* e, const void* const* src, size_t src_step, void* const* dst,
              size_t dst_step, const PoolJob& j) {
    if (!e) return fail(BICOS_E_ARG, "null engine");
    hipStream_t st = e->own_stream;
    const size_t d = (size_t)j.depth;
    const int prows = j.rows / j.scale, pcols = j.cols / j.scale;
    // only what the launch reads is uploaded: the remainder rows and columns stay on the host
    const size_t src_row = (size_t)pcols * j.scale * d, dst_row = (size_t)pcols * d;
    const size_t src_plane = src_row * prows * j.scale, dst_plane = dst_row * prows;
    PoolJob dj = j;  // the same job on dense staged device buffers
    dj.rows = prows * j.scale;
    dj.cols = pcols * j.scale;
    dj.src_row_pitch = (size_t)dj.cols;
    dj.src_plane_pitch = (size_t)dj.cols * dj.rows;
    dj.dst_row_pitch = (size_t)pcols;
    dj.dst_plane_pitch = (size_t)pcols * prows;
    Lease stage(e, e->stage, e->stage_bytes, st);
    char *s = nullptr, *o = nullptr;
    auto carve = [&] {
        s = stage.take(src_plane * j.n);
        o = stage.take(dst_plane * j.n);
    };
    carve();
    int rc = stage.acquire();
    if (rc) return rc;
    carve();
    dj.src = s;
    dj.dst = o;
    for (int t = 0; t < j.n && !rc; ++t)
        rc = check_hip(hipMemcpy2DAsync(s + t * src_plane, src_row, src[t], src_step, src_row,
                                        (size_t)dj.rows, hipMemcpyHostToDevice, st),
                       "stack upload");
    if (!rc) rc = pool_device(dj, st);
    for (int t = 0; t < j.n && !rc; ++t)
        rc = check_hip(hipMemcpy2DAsync(dst[t], dst_step, o + t * dst_plane, dst_row, dst_row,
                                        (size_t)prows, hipMemcpyDeviceToHost, st),
                       "stack download");
    const int rc2 = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    return rc ? rc : rc2;
}

// --------------------------------------------------------------- pyramid match

int match_pyramid_host(bicos_engine* e, const void* const* p0, const void* const* p1, size_t step,
                       int n, int rows, int cols, int depth, const BicosConfig& cfg,
                       bool has_nxcorr, float threshold, const DispRange& range,
                       const PyramidJob& j, void* disp, void* corr) {
    if (!e) return fail(BICOS_E_ARG, "null engine");
    hipStream_t st = e->own_stream;
    const size_t row = (size_t)cols * depth, plane = row * rows;
    const size_t pix = (size_t)rows * cols;
    const size_t ppix = (size_t)(rows / j.scale) * (size_t)(cols / j.scale);
    const bool f32 = has_nxcorr;  // bicos_output_type: of the fine map and of the coarse one
    const size_t esz = f32 ? 4 : 2;
    const size_t csz = cfg.precision != 0 ? sizeof(double) : sizeof(float);  // of the corrmap
    PyramidJob dj = j;  // the same job on staged device buffers
    char *s0 = nullptr, *s1 = nullptr;
    void *d_disp = nullptr, *d_corr = nullptr;
    Lease stage(e, e->stage, e->stage_bytes, st);
    auto carve = [&] {
        s0 = stage.take(plane * n);
        s1 = stage.take(plane * n);
        d_disp = stage.take(pix * esz);
        d_corr = corr && has_nxcorr ? stage.take(pix * csz) : nullptr;
        dj.coarse = j.coarse ? stage.take(ppix * esz) : nullptr;
        dj.guide = j.guide ? stage.take<int16_t>(2 * pix) : nullptr;
        dj.counts = j.counts ? stage.take<uint32_t>(2) : nullptr;
    };
    carve();
    int rc = stage.acquire();
    if (rc) return rc;
    carve();
    for (int t = 0; t < n && !rc; ++t) {
        rc = check_hip(hipMemcpy2DAsync(s0 + t * plane, row, p0[t], step, row, (size_t)rows,
                                        hipMemcpyHostToDevice, st), "stack upload");
        if (!rc)
            rc = check_hip(hipMemcpy2DAsync(s1 + t * plane, row, p1[t], step, row, (size_t)rows,
                                            hipMemcpyHostToDevice, st), "stack upload");
    }
    if (!rc)
        rc = match_pyramid_device(e, s0, s1, n, rows, cols, (size_t)cols, pix, depth, cfg,
                                  has_nxcorr, threshold, range, dj, d_disp, d_corr, st);
    if (!rc)
        rc = check_hip(hipMemcpyAsync(disp, d_disp, pix * esz, hipMemcpyDeviceToHost, st),
                       "disparity download");
    if (!rc && d_corr)
        rc = check_hip(hipMemcpyAsync(corr, d_corr, pix * csz, hipMemcpyDeviceToHost, st),
                       "corrmap download");
    if (!rc && j.coarse)
        rc = check_hip(hipMemcpyAsync(j.coarse, dj.coarse, ppix * esz, hipMemcpyDeviceToHost, st),
                       "coarse map download");
    if (!rc && j.guide)
        rc = check_hip(hipMemcpyAsync(j.guide, dj.guide, pix * 4, hipMemcpyDeviceToHost, st),
                       "guide download");
    if (!rc && j.counts)
        rc = check_hip(hipMemcpyAsync(j.counts, dj.counts, 2 * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, st), "counts download");
    const int rc2 = check_hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    return rc ? rc : rc2;
}

}  // namespace bicos_impl
