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

// -------------------------------------------------------- the staged host call

int Staging::begin() {
    for (const Buf& b : bufs_) lease_.take(b.bytes);
    rc_ = lease_.acquire();
    if (rc_) return rc_;
    for (Buf& b : bufs_) {
        b.dev = lease_.take(b.bytes);
        b.set(b.slot, b.dev);
    }
    return issue(true);
}

// the declared copies of one direction, in their order; none after an error
int Staging::issue(bool upload) {
    const hipMemcpyKind kind = upload ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    for (const Copy& c : copies_) {
        if (c.upload != upload || rc_) continue;
        char* dev = bufs_[c.buf].dev + c.at;
        void* dst = upload ? dev : c.host;
        const void* src = upload ? c.host : dev;
        rc_ = check_hip(c.rows ? hipMemcpy2DAsync(dst, upload ? c.row_bytes : c.host_pitch, src,
                                                  upload ? c.host_pitch : c.row_bytes,
                                                  c.row_bytes, c.rows, kind, st_)
                               : hipMemcpyAsync(dst, src, c.row_bytes, kind, st_),
                        c.what);
    }
    return rc_;
}

int Staging::download(void* host, const void* dev, size_t bytes, const char* what) {
    if (!rc_) rc_ = check_hip(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st_), what);
    return rc_;
}

int Staging::sync() {
    if (!rc_) rc_ = check_hip(hipStreamSynchronize(st_), "hipStreamSynchronize");
    return rc_;
}

int Staging::finish(int rc) {
    if (!rc_) rc_ = rc;
    issue(false);
    const int synced = check_hip(hipStreamSynchronize(st_), "hipStreamSynchronize");
    return rc_ ? rc_ : synced;
}

// --------------------------------------------------- the stages on host buffers
// Each takes a job its entry has validated (entries.cpp), copies it and points the copy at
// staged device buffers.

int reproject_host(bicos_engine* e, const ReprojectJob& j) {
    const size_t pixels = (size_t)j.rows * j.cols;
    if (pixels == 0) {
        if (j.counts) std::fill(j.counts, j.counts + 4, 0u);
        return BICOS_OK;
    }
    const size_t esz = j.disp_type == BICOS_CV_32F ? 4 : 2;
    const size_t cap = std::min(j.capacity, pixels);
    ReprojectJob d = j;
    d.capacity = cap;
    d.counts = nullptr;
    Staging s(e);
    s.in(d.disp, j.disp, pixels * esz, "disparity upload");
    s.out(d.xyz_map, j.xyz_map, pixels * 3 * sizeof(float), "xyz map download");
    if (j.points) {  // the list comes down by hand: the counts, then as much as they say
        s.buffer(d.points, (3 * cap + 1) * sizeof(float));  // (non-null at cap 0)
        if (j.index) s.buffer(d.index, (cap + 1) * sizeof(int32_t));
        s.buffer(d.counts, 4 * sizeof(uint32_t));
    }
    int rc = s.begin();
    if (!rc) rc = reproject_device(e, d, s.stream());
    if (!rc && j.points) {
        s.download(j.counts, d.counts, 4 * sizeof(uint32_t), "counts download");
        rc = s.sync();
        const size_t got = rc ? 0 : std::min<size_t>(j.counts[0], cap);
        if (got) rc = s.download(j.points, d.points, got * 3 * sizeof(float), "points download");
        if (got && j.index)
            rc = s.download(j.index, d.index, got * sizeof(int32_t), "index download");
    }
    return s.finish(rc);
}

// rows * cols > 0 (bicos_mesh_host answers an empty map itself, without an engine)
int mesh_host(bicos_engine* e, const MeshJob& j) {
    const size_t pixels = (size_t)j.rows * j.cols;
    const size_t esz = j.disp_type == BICOS_CV_32F ? 4 : 2;
    const size_t quads = j.rows < 2 || j.cols < 2 ? 0 : (size_t)(j.rows - 1) * (j.cols - 1);
    const size_t vcap = std::min(j.vertex_capacity, pixels);
    const size_t tcap = std::min(j.tri_capacity, 2 * quads);
    MeshJob d = j;
    d.vertex_capacity = vcap;
    d.tri_capacity = tcap;
    Staging s(e);
    s.in(d.disp, j.disp, pixels * esz, "disparity upload");
    // the lists come down by hand: both counts, then as much as they say
    s.buffer(d.points, (3 * vcap + 1) * sizeof(float));  // (non-null at capacity 0)
    if (j.index) s.buffer(d.index, (vcap + 1) * sizeof(int32_t));
    s.buffer(d.counts, 4 * sizeof(uint32_t));
    s.buffer(d.triangles, (3 * tcap + 1) * sizeof(int32_t));
    s.buffer(d.mesh_counts, 4 * sizeof(uint32_t));
    s.out(d.vertex_map, j.vertex_map, pixels * sizeof(int32_t), "vertex_map download");
    int rc = s.begin();
    if (!rc) rc = mesh_device(e, d, s.stream());
    if (!rc) {
        s.download(j.counts, d.counts, 4 * sizeof(uint32_t), "counts download");
        s.download(j.mesh_counts, d.mesh_counts, 4 * sizeof(uint32_t), "mesh_counts download");
        rc = s.sync();
        const size_t verts = rc ? 0 : std::min<size_t>(j.counts[0], vcap);
        const size_t tris = rc ? 0 : std::min<size_t>(j.mesh_counts[0], tcap);
        if (verts)
            rc = s.download(j.points, d.points, verts * 3 * sizeof(float), "points download");
        if (verts && j.index)
            rc = s.download(j.index, d.index, verts * sizeof(int32_t), "index download");
        if (tris)
            rc = s.download(j.triangles, d.triangles, tris * 3 * sizeof(int32_t),
                            "triangles download");
    }
    return s.finish(rc);
}

int project_host(bicos_engine* e, const ProjectJob& j) {
    const size_t n = j.count, pixels = (size_t)j.img_rows * j.img_cols;
    ProjectJob d = j;
    Staging s(e);
    // (a zero-length list still gets a buffer of its own: the launches take pointers)
    const int pts = s.buffer(d.points, std::max<size_t>(n * 12, 4));
    if (n) s.up(pts, 0, j.points, n * 12, "points upload");
    if (j.image) {  // the rows made dense
        const size_t esz = (size_t)j.img_depth, row = (size_t)j.img_cols * j.channels * esz;
        const int img = s.buffer(d.image, std::max<size_t>(pixels * j.channels * esz, 4));
        if (pixels)
            s.up2d(img, 0, j.image, j.img_pitch * esz, row, (size_t)j.img_rows, "image upload");
        d.img_pitch = (size_t)j.img_cols * j.channels;
        s.out(d.tex, j.tex, n * j.channels * esz, "tex download");
    }
    s.out(d.uv, j.uv, n * 8, "uv download");
    s.out(d.depth, j.depth, n * 4, "depth download");
    s.out(d.cls, j.cls, n, "cls download");
    s.out(d.depth_map, j.depth_map, pixels * 4, "depth_map download");
    s.out(d.index_map, j.index_map, pixels * 4, "index_map download");
    s.out(d.counts, j.counts, 5 * sizeof(uint32_t), "counts download");
    int rc = s.begin();
    if (!rc) rc = project_device(e, d, s.stream());
    return s.finish(rc);
}

int speckle_host(bicos_engine* e, const SpeckleJob& j) {
    const size_t pixels = (size_t)j.rows * j.cols;
    if (pixels == 0) {
        if (j.counts) std::fill(j.counts, j.counts + 4, 0u);
        return BICOS_OK;
    }
    const size_t bytes = pixels * (j.disp_type == BICOS_CV_32F ? 4 : 2);
    SpeckleJob d = j;
    Staging s(e);
    const int map = s.buffer(d.out, bytes);  // filtered in place
    s.up(map, 0, j.disp, bytes, "disparity upload");
    s.down(map, 0, j.out, bytes, "filtered map download");
    s.out(d.labels, j.labels, pixels * sizeof(int32_t), "labels download");
    s.out(d.counts, j.counts, 4 * sizeof(uint32_t), "counts download");
    int rc = s.begin();
    d.disp = d.out;
    if (!rc) rc = speckle_device(e, d, s.stream());
    return s.finish(rc);
}

int median_host(bicos_engine* e, const MedianJob& j) {
    const size_t pixels = (size_t)j.rows * j.cols;
    if (pixels == 0) {
        if (j.counts) std::fill(j.counts, j.counts + 4, 0u);
        return BICOS_OK;
    }
    const size_t bytes = pixels * (j.disp_type == BICOS_CV_32F ? 4 : 2);
    MedianJob d = j;
    Staging s(e);
    // two buffers, because the launch reads neighbours (which is why the caller's out may be
    // its map)
    s.in(d.disp, j.disp, bytes, "disparity upload");
    s.out(d.out, j.out, bytes, "filtered map download");
    s.out(d.counts, j.counts, 4 * sizeof(uint32_t), "counts download");
    int rc = s.begin();
    if (!rc) rc = median_device(d, s.stream());
    return s.finish(rc);
}

// rows * cols > 0 (bicos_normals_host answers an empty map itself, without an engine)
int normals_host(bicos_engine* e, const NormalsJob& j) {
    const size_t pixels = (size_t)j.rows * j.cols;
    const size_t count = j.normals ? j.count : 0;
    const size_t esz = j.disp_type == BICOS_CV_32F ? 4 : 2;
    NormalsJob d = j;
    d.count = count;
    Staging s(e);
    s.in(d.disp, j.disp, pixels * esz, "disparity upload");
    s.out(d.normal_map, j.normal_map, pixels * 3 * sizeof(float), "normal map download");
    s.in(d.index, count ? j.index : nullptr, count * sizeof(int32_t), "index upload");
    s.out(d.normals, count ? j.normals : nullptr, count * 3 * sizeof(float), "normals download");
    s.out(d.counts, j.counts, 4 * sizeof(uint32_t), "counts download");
    int rc = s.begin();
    if (!rc) rc = normals_device(d, s.stream());
    return s.finish(rc);
}

int guide_host(bicos_engine* e, const GuideJob& j) {
    const size_t pixels = (size_t)j.rows * j.cols;
    if (pixels == 0) {
        if (j.counts) std::fill(j.counts, j.counts + 2, 0u);
        return BICOS_OK;
    }
    const size_t prior_bytes = (size_t)j.prows * j.pcols * (j.prior_type == BICOS_CV_32F ? 4 : 2);
    const size_t pitch = j.guide_pitch ? j.guide_pitch : (size_t)j.cols;
    GuideJob d = j;
    d.guide_pitch = (size_t)j.cols;  // the staged guide is dense
    Staging s(e);
    s.in(d.prior, j.prior, prior_bytes, "prior upload");
    s.down2d(s.buffer(d.guide, pixels * 4), 0, j.guide, pitch * 4, (size_t)j.cols * 4,
             (size_t)j.rows, "guide download");
    s.out(d.counts, j.counts, 2 * sizeof(uint32_t), "counts download");
    int rc = s.begin();
    if (!rc) rc = guide_device(d, s.stream());
    return s.finish(rc);
}

// --------------------------------------------------------------- rectification

int rectify_host(bicos_engine* e, const void* const* src, size_t src_step, void* const* dst,
                 size_t dst_step, const RectifyJob& j) {
    const size_t d = (size_t)j.depth;
    const size_t src_row = (size_t)j.src_cols * d, dst_row = (size_t)j.cols * d;
    const size_t map_row = (size_t)j.cols * sizeof(float);
    const size_t src_plane = src_row * j.src_rows, dst_plane = dst_row * j.rows;
    RectifyJob dj = j;  // dense
    dj.src_row_pitch = (size_t)j.src_cols;
    dj.src_plane_pitch = (size_t)j.src_cols * j.src_rows;
    dj.dst_row_pitch = (size_t)j.cols;
    dj.dst_plane_pitch = (size_t)j.cols * j.rows;
    dj.map_pitch = 0;
    const size_t mp = j.map_pitch ? j.map_pitch : map_row;
    Staging s(e);
    const int in = s.buffer(dj.src, src_plane * j.n), out = s.buffer(dj.dst, dst_plane * j.n);
    for (int t = 0; t < j.n; ++t)
        s.up2d(in, t * src_plane, src[t], src_step, src_row, (size_t)j.src_rows, "stack upload");
    s.up2d(s.buffer(dj.map_x, map_row * j.rows), 0, j.map_x, mp, map_row, (size_t)j.rows,
           "map upload");
    s.up2d(s.buffer(dj.map_y, map_row * j.rows), 0, j.map_y, mp, map_row, (size_t)j.rows,
           "map upload");
    for (int t = 0; t < j.n; ++t)
        s.down2d(out, t * dst_plane, dst[t], dst_step, dst_row, (size_t)j.rows, "stack download");
    s.out(dj.valid, j.valid, (size_t)j.rows * j.cols, "valid download");
    int rc = s.begin();
    if (!rc) rc = rectify_device(dj, s.stream());
    return s.finish(rc);
}

int rectify_maps_host(bicos_engine* e, const RectifyMapsJob& j,
                      const bicos_hip::RectifyCamera& cam) {
    const size_t bytes = (size_t)j.rows * j.cols * sizeof(float);
    RectifyMapsJob dj = j;
    Staging s(e);
    s.out(dj.map_x, j.map_x, bytes, "map download");
    s.out(dj.map_y, j.map_y, bytes, "map download");
    int rc = s.begin();
    if (!rc) rc = rectify_maps_device(dj, cam, s.stream());
    return s.finish(rc);
}

// --------------------------------------------------------------- stack pooling

int pool_host(bicos_engine* e, const void* const* src, size_t src_step, void* const* dst,
              size_t dst_step, const PoolJob& j) {
    const size_t d = (size_t)j.depth;
    const int prows = j.rows / j.scale, pcols = j.cols / j.scale;
    // only what the launch reads is uploaded: the remainder rows and columns stay on the host
    const size_t src_row = (size_t)pcols * j.scale * d, dst_row = (size_t)pcols * d;
    const size_t src_plane = src_row * prows * j.scale, dst_plane = dst_row * prows;
    PoolJob dj = j;  // dense
    dj.rows = prows * j.scale;
    dj.cols = pcols * j.scale;
    dj.src_row_pitch = (size_t)dj.cols;
    dj.src_plane_pitch = (size_t)dj.cols * dj.rows;
    dj.dst_row_pitch = (size_t)pcols;
    dj.dst_plane_pitch = (size_t)pcols * prows;
    Staging s(e);
    const int in = s.buffer(dj.src, src_plane * j.n), out = s.buffer(dj.dst, dst_plane * j.n);
    for (int t = 0; t < j.n; ++t)
        s.up2d(in, t * src_plane, src[t], src_step, src_row, (size_t)dj.rows, "stack upload");
    for (int t = 0; t < j.n; ++t)
        s.down2d(out, t * dst_plane, dst[t], dst_step, dst_row, (size_t)prows, "stack download");
    int rc = s.begin();
    if (!rc) rc = pool_device(dj, s.stream());
    return s.finish(rc);
}

// --------------------------------------------------------------- pyramid match

int match_pyramid_host(bicos_engine* e, const void* const* p0, const void* const* p1, size_t step,
                       int n, int rows, int cols, int depth, const BicosConfig& cfg,
                       bool has_nxcorr, float threshold, const DispRange& range,
                       const PyramidJob& j, void* disp, void* corr) {
    const size_t row = (size_t)cols * depth, plane = row * rows;
    const size_t pix = (size_t)rows * cols;
    const size_t ppix = (size_t)(rows / j.scale) * (size_t)(cols / j.scale);
    const size_t esz = has_nxcorr ? 4 : 2;  // bicos_output_type: of the fine map and the coarse one
    const size_t csz = cfg.precision != 0 ? sizeof(double) : sizeof(float);  // of the corrmap
    PyramidJob dj = j;
    const void *s0 = nullptr, *s1 = nullptr;
    void *d_disp = nullptr, *d_corr = nullptr;
    Staging s(e);
    const int b0 = s.buffer(s0, plane * n), b1 = s.buffer(s1, plane * n);
    for (int t = 0; t < n; ++t) {
        s.up2d(b0, t * plane, p0[t], step, row, (size_t)rows, "stack upload");
        s.up2d(b1, t * plane, p1[t], step, row, (size_t)rows, "stack upload");
    }
    s.out(d_disp, disp, pix * esz, "disparity download");
    s.out(d_corr, has_nxcorr ? corr : nullptr, pix * csz, "corrmap download");
    s.out(dj.coarse, j.coarse, ppix * esz, "coarse map download");
    s.out(dj.guide, j.guide, pix * 4, "guide download");
    s.out(dj.counts, j.counts, 2 * sizeof(uint32_t), "counts download");
    int rc = s.begin();
    if (!rc)
        rc = match_pyramid_device(e, s0, s1, n, rows, cols, (size_t)cols, pix, depth, cfg,
                                  has_nxcorr, threshold, range, dj, d_disp, d_corr, s.stream());
    return s.finish(rc);
}

}  // namespace bicos_impl

