// cxxapi.cpp -- the C++ API (include/bicos/*.hpp) over bicos_impl (engine.hpp):
//
//   BICOS::match   <- reference BICOS::match (src/lib.cpp:31-49) and the backend entry
//                     impl::cpu::match (src/impl/cpu.cpp:100-159)
//   BICOS::reproject  (bicos/reproject.hpp; no reference counterpart in its library)
//   BICOS::filter_speckles  (bicos/speckle.hpp; no reference counterpart)
//   BICOS::rectify_maps, BICOS::rectify  (bicos/rectify.hpp; no reference counterpart)
//   BICOS::median_filter  (bicos/median.hpp; no reference counterpart)
//   BICOS::normals  (bicos/normals.hpp; no reference counterpart)
//   BICOS::mesh  (bicos/mesh.hpp; likewise)
//   BICOS::project  (bicos/project.hpp; likewise)
//   BICOS::guide_from_disparity, the guided BICOS::match  (bicos/guide.hpp; likewise)
//   BICOS::pool_stack, BICOS::match_pyramid  (bicos/pool.hpp; likewise)
#include "engine.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../include/bicos/common.hpp"
#include "../../include/bicos/match.hpp"
#include "../../include/bicos/hip.hpp"
#include "../../include/bicos/reproject.hpp"
#include "../../include/bicos/speckle.hpp"
#include "../../include/bicos/rectify.hpp"
#include "../../include/bicos/median.hpp"
#include "../../include/bicos/normals.hpp"
#include "../../include/bicos/mesh.hpp"
#include "../../include/bicos/project.hpp"
#include "../../include/bicos/guide.hpp"
#include "../../include/bicos/pool.hpp"

using bicos_impl::check_hip;

namespace BICOS {

size_t HipImage::elem_size(int type) {
    switch (type) {
        case U8: return 1;
        case U16:
        case S16: return 2;
        case F32: return 4;
        case F64: return 8;
    }
    throw Exception("unsupported image type " + std::to_string(type));
}

HipImage::HipImage(int rows, int cols, int type, void* data, size_t step, Memory mem)
    : _data(data), _rows(rows), _cols(cols), _type(type), _mem(mem) {
    _step = step ? step : (size_t)cols * elem_size(type);
}

void HipImage::create(int rows, int cols, int type, Memory mem) {
    // like cv::Mat::create: a no-op when the header already describes a dense buffer of this
    // size and type (owned or a view of the caller's memory), so results can be written
    // straight into caller-provided buffers
    if (_data && _rows == rows && _cols == cols && _type == type && _mem == mem &&
        _step == (size_t)cols * elem_size(type))
        return;
    const size_t step = (size_t)cols * elem_size(type);
    const size_t bytes = step * rows;
    void* p = nullptr;
    if (mem == Memory::Host) {
        p = std::malloc(bytes ? bytes : 1);
        if (!p) throw Exception("out of host memory");
        _owner = std::shared_ptr<void>(p, [](void* q) { std::free(q); });
    } else {
        if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) throw Exception("hipMalloc failed");
        _owner = std::shared_ptr<void>(p, [](void* q) { (void)hipFree(q); });
    }
    _data = p;
    _rows = rows;
    _cols = cols;
    _type = type;
    _step = step;
    _mem = mem;
}

HipImage HipImage::download() const {
    if (_mem == Memory::Host) return *this;
    Image h = allocate(_rows, _cols, _type, Memory::Host);
    if (!empty() &&
        hipMemcpy2D(h._data, h._step, _data, _step, (size_t)_cols * elemSize(), _rows,
                    hipMemcpyDeviceToHost) != hipSuccess)
        throw Exception("download failed");
    return h;
}

static void throw_rc(int rc) {
    if (rc != BICOS_OK) throw Exception(bicos_impl::last_error());
}

// reference src/impl/cpu.cpp:100-159 (validation, dispatch) + src/lib.cpp:31-49
void match(const std::vector<Image>& stack0, const std::vector<Image>& stack1, Image& disparity,
           Config cfg, Image* corrmap, hipStream_t stream) {
    impl::hip::match(stack0, stack1, disparity, cfg, corrmap, stream);
}

// what match_pyramid adds to a match: its parameters and its optional outputs
struct PyramidCall {
    PyramidParams params;
    Image* coarse;
    Image* guide;
    uint32_t* counts;
};

static void match_stacks(const std::vector<Image>& stack0, const std::vector<Image>& stack1,
                         const Image* guide, Image& disparity, Config cfg, Image* corrmap,
                         hipStream_t stream, const PyramidCall* pyr = nullptr);

// the backend seam (bicos/hip.hpp; reference include/cpu.hpp:27-33, include/cuda.hpp:27-34)
void impl::hip::match(const std::vector<Image>& stack0, const std::vector<Image>& stack1,
                      Image& disparity, Config cfg, Image* corrmap, hipStream_t stream) {
    match_stacks(stack0, stack1, nullptr, disparity, cfg, corrmap, stream);
}

// the guided match (bicos/match.hpp): cfg.disparity_range is the global window beside the guide
void match(const std::vector<Image>& stack0, const std::vector<Image>& stack1, const Image& guide,
           Image& disparity, Config cfg, Image* corrmap, hipStream_t stream) {
    match_stacks(stack0, stack1, &guide, disparity, cfg, corrmap, stream);
}

// the pyramid match (bicos/pool.hpp): cfg.disparity_range is the global window of both levels
void match_pyramid(const std::vector<Image>& stack0, const std::vector<Image>& stack1,
                   Image& disparity, Config cfg, const PyramidParams& params, Image* corrmap,
                   Image* coarse, Image* guide, uint32_t* counts, hipStream_t stream) {
    if (!cfg.disparity_range) throw Exception("match_pyramid: cfg.disparity_range is required");
    const PyramidCall call{params, coarse, guide, counts};
    match_stacks(stack0, stack1, nullptr, disparity, cfg, corrmap, stream, &call);
}

static void match_stacks(const std::vector<Image>& stack0, const std::vector<Image>& stack1,
                         const Image* guide, Image& disparity, Config cfg, Image* corrmap,
                         hipStream_t stream, const PyramidCall* pyr) {
    const size_t n = stack0.size();
    if (n < 2) throw Exception("need at least two images");
    if (stack1.size() != n) throw Exception("stacks differ in length");
    const Image& f = stack0.front();
    if (f.type() != U8 && f.type() != U16)
        throw Exception("bad input depths, only CV_8UC1 and CV_16UC1 are supported");
    const Memory mem = f.memory();
    for (const auto* s : {&stack0, &stack1})
        for (const Image& im : *s)
            if (im.rows() != f.rows() || im.cols() != f.cols() || im.type() != f.type() ||
                im.memory() != mem)
                throw Exception("all images must share size, type and memory");
    const int rows = f.rows(), cols = f.cols();
    const int depth = (int)f.elemSize();

    BicosConfig c{};
    const bool has_nxcorr = cfg.nxcorr_threshold.has_value();
    c.nxcorr_threshold = has_nxcorr ? *cfg.nxcorr_threshold : 0.5f;
    c.subpixel_step = cfg.subpixel_step ? *cfg.subpixel_step : -1.f;
    c.min_variance = cfg.min_variance ? *cfg.min_variance : -1.f;
    c.mode = cfg.mode == TransformMode::FULL ? 1 : 0;
    c.precision = cfg.precision == Precision::DOUBLE ? 1 : 0;
    if (auto* cons = std::get_if<Variant::Consistency>(&cfg.variant)) {
        c.variant_type = 1;
        c.max_lr_diff = cons->max_lr_diff;
        c.no_dupes = cons->no_dupes;
    }
    if (cfg.subpixel_step && !(*cfg.subpixel_step > 0))
        throw Exception("subpixel_step must be a positive finite number");
    bicos_impl::DispRange range{0, 0};
    if (cfg.disparity_range) {
        range = {cfg.disparity_range->min, cfg.disparity_range->max};
        throw_rc(bicos_impl::check_range(range.min, range.max));
    }
    if (guide) {
        // pairs {lo, hi} side by side: S16, rows x 2 cols, rows a whole number of dwords apart
        if (guide->type() != S16 || guide->rows() != rows || guide->cols() != 2 * cols)
            throw Exception("guide: need an S16 image of rows x 2 cols");
        if (guide->memory() != mem) throw Exception("guide: must be in the memory of the stacks");
        if (guide->step() % 4) throw Exception("guide: the row step must be a multiple of 4 bytes");
        if (!cfg.disparity_range) range = {INT32_MIN, INT32_MAX};
        range.guide = (const int16_t*)guide->data();
        range.guide_pitch = guide->step() / 4;
        if (rows > 0 && cols > 0)
            throw_rc(bicos_impl::check_guide(range.guide, range.guide_pitch, cols, range.min,
                                             range.max));
    }
    const bicos_impl::DispRange* rg = cfg.disparity_range || guide ? &range : nullptr;
    if (cfg.min_variance && *cfg.min_variance < 0) c.min_variance = -1.f;
    bicos_impl::PyramidJob pj{};
    if (pyr) {
        const PyramidParams& p = pyr->params;
        pj.scale = p.scale;
        pj.radius = p.radius;
        pj.spread = p.spread;
        pj.fallback_lo = p.fallback_window ? std::max(range.min, -32767) : p.fallback_lo;
        pj.fallback_hi = p.fallback_window ? std::min(range.max, 32767) : p.fallback_hi;
        // the argument errors of all four steps before an output is created (any non-null
        // placeholder stands for the buffers that do not exist yet)
        const void* some = &pj;
        throw_rc(bicos_impl::check_pyramid(some, some, (int)n, rows, cols, (size_t)cols,
                                           (size_t)rows * cols, depth, c, has_nxcorr, range, pj,
                                           some));
    }

    int dev = 0;
    (void)hipGetDevice(&dev);
    bicos_engine* e = bicos_impl::default_engine(dev);
    if (!e) throw Exception(bicos_impl::last_error());
    std::lock_guard<std::mutex> g(e->lock);
    hipStream_t st = mem == Memory::Host ? e->own_stream : stream;
    const int dtype = has_nxcorr ? F32 : S16;
    const bool dbl = c.precision != 0;
    const bool want_corr = corrmap && has_nxcorr;

    if (mem == Memory::Host) {
        // banded, pipelined upload -> match -> download (bicos_impl::match_host)
        std::vector<const void*> p0(n), p1(n);
        std::vector<size_t> st0(n), st1(n);
        for (size_t t = 0; t < n; ++t) {
            p0[t] = stack0[t].data();
            p1[t] = stack1[t].data();
            st0[t] = stack0[t].step();
            st1[t] = stack1[t].step();
        }
        disparity.create(rows, cols, dtype, Memory::Host);
        if (want_corr) corrmap->create(rows, cols, dbl ? F64 : F32, Memory::Host);
        if (pyr) {
            for (size_t t = 0; t < n; ++t)
                if (st0[t] != st0[0] || st1[t] != st0[0])
                    throw Exception("match_pyramid: host images must share one step");
            if (pyr->coarse) pyr->coarse->create(rows / pj.scale, cols / pj.scale, dtype, Memory::Host);
            if (pyr->guide) pyr->guide->create(rows, 2 * cols, S16, Memory::Host);
            pj.coarse = pyr->coarse ? pyr->coarse->data() : nullptr;
            pj.guide = pyr->guide ? (int16_t*)pyr->guide->data() : nullptr;
            pj.counts = pyr->counts;
            throw_rc(bicos_impl::match_pyramid_host(
                e, p0.data(), p1.data(), st0[0], (int)n, rows, cols, depth, c, has_nxcorr,
                c.nxcorr_threshold, range, pj, disparity.data(),
                want_corr ? corrmap->data() : nullptr));
            return;
        }
        throw_rc(bicos_impl::match_host(e, p0.data(), st0.data(), p1.data(), st1.data(), (int)n,
                                        rows, cols, depth, c, has_nxcorr, c.nxcorr_threshold,
                                        disparity.data(), want_corr ? corrmap->data() : nullptr,
                                        rg));
        return;
    }

    // the planar device stacks the kernels read
    const size_t elem = (size_t)depth;
    const void* s0 = nullptr;
    const void* s1 = nullptr;
    size_t row_pitch = (size_t)cols, plane_pitch = (size_t)rows * cols;
    auto uniform = [&](const std::vector<Image>& s, size_t& rp, size_t& pp) {
        // zero-copy when the images already form one planar buffer with a common pitch
        if (s[0].step() % elem) return false;
        rp = s[0].step() / elem;
        const char* b = (const char*)s[0].data();
        if (n < 2) return false;
        const ptrdiff_t d = (const char*)s[1].data() - b;
        if (d <= 0 || d % (ptrdiff_t)elem) return false;
        for (size_t t = 0; t < n; ++t)
            if (s[t].step() != s[0].step() || (const char*)s[t].data() != b + (ptrdiff_t)t * d)
                return false;
        pp = (size_t)d / elem;
        return pp >= (size_t)rows * rp;
    };
    size_t rp0 = 0, pp0 = 0, rp1 = 0, pp1 = 0;
    // staged rows start 64-byte aligned: no two copies share a dword and the pitches suit
    // the aligned (LDS-staged) agree kernel
    const size_t stage_row = ((size_t)cols * elem + 63) & ~(size_t)63;
    const size_t plane_bytes = (size_t)rows * stage_row;
    bicos_impl::Lease stage(e, e->stage, e->stage_bytes, st);  // held until the match is queued
    if (uniform(stack0, rp0, pp0) && uniform(stack1, rp1, pp1) && rp0 == rp1 && pp0 == pp1) {
        s0 = stack0[0].data();
        s1 = stack1[0].data();
        row_pitch = rp0;
        plane_pitch = pp0;
    } else if (rows > 0 && cols > 0) {
        stage.take(2 * n * plane_bytes);
        throw_rc(stage.acquire());
        char* dst = stage.take(2 * n * plane_bytes);
        const hipMemcpyKind kind = hipMemcpyDeviceToDevice;
        for (size_t t = 0; t < n; ++t) {
            throw_rc(check_hip(hipMemcpy2DAsync(dst + t * plane_bytes, stage_row,
                                                stack0[t].data(), stack0[t].step(), cols * elem,
                                                rows, kind, st),
                               "stack upload"));
            throw_rc(check_hip(hipMemcpy2DAsync(dst + (n + t) * plane_bytes, stage_row,
                                                stack1[t].data(), stack1[t].step(), cols * elem,
                                                rows, kind, st),
                               "stack upload"));
        }
        s0 = dst;
        s1 = dst + n * plane_bytes;
        row_pitch = stage_row / elem;
        plane_pitch = plane_bytes / elem;
    }

    disparity.create(rows, cols, dtype, Memory::Device);
    if (want_corr) corrmap->create(rows, cols, dbl ? F64 : F32, Memory::Device);
    if (pyr) {
        if (pyr->coarse) pyr->coarse->create(rows / pj.scale, cols / pj.scale, dtype, Memory::Device);
        if (pyr->guide) pyr->guide->create(rows, 2 * cols, S16, Memory::Device);
        pj.coarse = pyr->coarse ? pyr->coarse->data() : nullptr;
        pj.guide = pyr->guide ? (int16_t*)pyr->guide->data() : nullptr;
        pj.counts = pyr->counts;
        throw_rc(bicos_impl::match_pyramid_device(
            e, s0, s1, (int)n, rows, cols, row_pitch, plane_pitch, depth, c, has_nxcorr,
            c.nxcorr_threshold, range, pj, disparity.data(),
            want_corr ? corrmap->data() : nullptr, st));
        return;
    }
    throw_rc(bicos_impl::match_device(e, s0, s1, (int)n, rows, cols, row_pitch, plane_pitch, depth,
                                      c, has_nxcorr, c.nxcorr_threshold, disparity.data(),
                                      want_corr ? corrmap->data() : nullptr, st, false, nullptr,
                                      nullptr, rg));
}

// ---------------------------------------------------------------- BICOS::reproject
// over the C entries (entries.cpp), which validate, lock the engine and launch

namespace {

// What every map stage asks of its map, `name` being the function's in the messages: S16 or
// F32, dense and, where the stage writes an image of `channels` values per pixel, narrow enough
// for that image's width to fit an int
void check_map(const std::string& name, const Image& map, int channels = 0,
               const char* what = "disparity") {
    if (map.type() != S16 && map.type() != F32)
        throw Exception(name + ": the " + what + " map must be S16 or F32");
    if (map.step() != (size_t)map.cols() * map.elemSize() && map.rows() > 1)
        throw Exception(name + ": the " + what + " map must be dense");
    if ((int64_t)map.cols() * channels > INT32_MAX) throw Exception(name + ": map too wide");
}

// One device allocation sliced into counts | a | b (32-bit words each), for the overloads that
// run a device entry on buffers of their own and bring down the counts, then what they call for
class DeviceBlock {
  public:
    DeviceBlock(const char* what, size_t counts, size_t a = 0, size_t b = 0) : n_(counts), a_(a) {
        void* raw = nullptr;
        throw_rc(check_hip(hipMalloc(&raw, (counts + a + b) * 4), what));
        own_.reset(raw, [](void* q) { (void)hipFree(q); });
    }
    uint32_t* counts() const { return (uint32_t*)own_.get(); }
    template <class T>
    T* a() const { return (T*)(counts() + n_); }
    template <class T>
    T* b() const { return (T*)(counts() + n_ + a_); }
    void counts_down(uint32_t* host) const { down(host, counts(), n_ * 4, "counts download"); }
    static void down(void* host, const void* dev, size_t bytes, const char* what) {
        throw_rc(check_hip(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost), what));
    }

  private:
    std::shared_ptr<void> own_;
    size_t n_, a_;
};

bicos_engine* current_engine() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    bicos_engine* e = bicos_impl::default_engine(dev);
    if (!e) throw Exception(bicos_impl::last_error());
    return e;
}

}  // namespace

void reproject(const Image& disparity, const Matx44d& Q, Image& xyz, int flags,
               hipStream_t stream) {
    check_map("reproject", disparity, 3);
    const int rows = disparity.rows(), cols = disparity.cols();
    xyz.create(rows, 3 * cols, F32, disparity.memory());
    if (disparity.memory() == Memory::Host)
        throw_rc(bicos_reproject_host(nullptr, disparity.data(), disparity.type(), rows, cols,
                                      Q.data(), flags, (float*)xyz.data(), nullptr, nullptr, 0,
                                      nullptr));
    else
        throw_rc(bicos_reproject_device(nullptr, disparity.data(), disparity.type(), rows, cols,
                                        Q.data(), flags, (float*)xyz.data(), nullptr, nullptr, 0,
                                        nullptr, stream));
}

void reproject(const Image& disparity, const Matx44d& Q, float* points, int32_t* index,
               size_t capacity, uint32_t* counts, int flags, hipStream_t stream) {
    check_map("reproject", disparity);
    if (disparity.memory() != Memory::Device)
        throw Exception("reproject: device buffers need a device map");
    if (!points) throw Exception("reproject: null points");
    throw_rc(bicos_reproject_device(current_engine(), disparity.data(), disparity.type(),
                                    disparity.rows(), disparity.cols(), Q.data(), flags, nullptr,
                                    points, index, capacity, counts, stream));
}

ReprojectStats reproject(const Image& disparity, const Matx44d& Q, std::vector<float>& points,
                         int flags, std::vector<int32_t>* index) {
    check_map("reproject", disparity);
    const int rows = disparity.rows(), cols = disparity.cols();
    const size_t pixels = (size_t)(rows > 0 ? rows : 0) * (size_t)(cols > 0 ? cols : 0);
    uint32_t counts[4] = {0, 0, 0, 0};
    points.resize(3 * pixels + 1);  // (+1: never a null pointer)
    if (index) index->resize(pixels + 1);
    if (disparity.memory() == Memory::Host) {
        throw_rc(bicos_reproject_host(nullptr, disparity.data(), disparity.type(), rows, cols,
                                      Q.data(), flags, nullptr, points.data(),
                                      index ? index->data() : nullptr, pixels, counts));
    } else {
        // device buffers for every pixel, then only the kept points come down
        // counts | points | index in one allocation
        const DeviceBlock d("hipMalloc(points)", 4, 3 * pixels, index ? pixels : 0);
        float* d_points = d.a<float>();
        int32_t* d_index = index ? d.b<int32_t>() : nullptr;
        throw_rc(bicos_reproject_device(current_engine(), disparity.data(), disparity.type(), rows,
                                        cols, Q.data(), flags, nullptr, d_points, d_index, pixels,
                                        d.counts(), nullptr));
        d.counts_down(counts);
        const size_t kept = counts[0];
        if (kept) d.down(points.data(), d_points, kept * 3 * sizeof(float), "points download");
        if (kept && index)
            d.down(index->data(), d_index, kept * sizeof(int32_t), "index download");
    }
    points.resize(3 * (size_t)counts[0]);
    if (index) index->resize(counts[0]);
    return ReprojectStats{counts[0], counts[1], counts[2], counts[3]};
}

// ---------------------------------------------------------- BICOS::filter_speckles
// over the C entries (entries.cpp), which validate, lock the engine and launch

void filter_speckles(const Image& disparity, Image& out, int max_size, float max_diff, int flags,
                     int32_t* labels, uint32_t* counts, hipStream_t stream) {
    check_map("filter_speckles", disparity);
    if (disparity.memory() != Memory::Device)
        throw Exception("filter_speckles: device buffers need a device map");
    const void* map = disparity.data();  // (out may be the same header)
    const int rows = disparity.rows(), cols = disparity.cols(), type = disparity.type();
    out.create(rows, cols, type, Memory::Device);
    throw_rc(bicos_speckle_device(current_engine(), map, type, rows, cols, max_size, max_diff,
                                  flags, out.data(), labels, counts, stream));
}

SpeckleStats filter_speckles(const Image& disparity, Image& out, int max_size, float max_diff,
                             int flags, std::vector<int32_t>* labels) {
    check_map("filter_speckles", disparity);
    const void* map = disparity.data();
    const int rows = disparity.rows(), cols = disparity.cols(), type = disparity.type();
    const Memory mem = disparity.memory();
    const size_t pixels = (size_t)(rows > 0 ? rows : 0) * (size_t)(cols > 0 ? cols : 0);
    uint32_t counts[4] = {0, 0, 0, 0};
    out.create(rows, cols, type, mem);
    if (labels) labels->resize(pixels);
    if (mem == Memory::Host) {
        throw_rc(bicos_speckle_host(nullptr, map, type, rows, cols, max_size, max_diff, flags,
                                    out.data(), labels ? labels->data() : nullptr, counts));
    } else {
        // counts | labels in one device allocation, downloaded after the launches
        const DeviceBlock d("hipMalloc(labels)", 4, labels ? pixels : 0);
        int32_t* d_labels = labels ? d.a<int32_t>() : nullptr;
        throw_rc(bicos_speckle_device(current_engine(), map, type, rows, cols, max_size, max_diff,
                                      flags, out.data(), d_labels, d.counts(), nullptr));
        d.counts_down(counts);
        if (labels && pixels)
            d.down(labels->data(), d_labels, pixels * sizeof(int32_t), "labels download");
    }
    return SpeckleStats{counts[0], counts[1], counts[2], counts[3]};
}

// ------------------------------------------------------------ BICOS::median_filter
// over the C entries (entries.cpp), which validate and launch

void median_filter(const Image& disparity, Image& out, int ksize, int fill_min, int flags,
                   uint32_t* counts, hipStream_t stream) {
    check_map("median_filter", disparity);
    if (disparity.memory() != Memory::Device)
        throw Exception("median_filter: device buffers need a device map");
    if (&out == &disparity)
        throw Exception("median_filter: a device map cannot be filtered in place");
    const int rows = disparity.rows(), cols = disparity.cols(), type = disparity.type();
    out.create(rows, cols, type, Memory::Device);
    throw_rc(bicos_median_device(current_engine(), disparity.data(), type, rows, cols, ksize,
                                 fill_min, flags, out.data(), counts, stream));
}

MedianStats median_filter(const Image& disparity, Image& out, int ksize, int fill_min, int flags) {
    check_map("median_filter", disparity);
    const void* map = disparity.data();  // (a host out may be the same header)
    const int rows = disparity.rows(), cols = disparity.cols(), type = disparity.type();
    const Memory mem = disparity.memory();
    uint32_t counts[4] = {0, 0, 0, 0};
    if (mem == Memory::Host) {
        out.create(rows, cols, type, mem);
        throw_rc(bicos_median_host(nullptr, map, type, rows, cols, ksize, fill_min, flags,
                                   out.data(), counts));
    } else {
        if (&out == &disparity)
            throw Exception("median_filter: a device map cannot be filtered in place");
        out.create(rows, cols, type, mem);
        const DeviceBlock d("hipMalloc(counts)", 4);
        throw_rc(bicos_median_device(current_engine(), map, type, rows, cols, ksize, fill_min,
                                     flags, out.data(), d.counts(), nullptr));
        d.counts_down(counts);
    }
    return MedianStats{counts[0], counts[1], counts[2], counts[3]};
}

// ------------------------------------------------------------------ BICOS::normals
// over the C entries (entries.cpp), which validate and launch

void normals(const Image& disparity, const Matx44d& Q, Image& normal_map,
             const NormalsParams& p, hipStream_t stream) {
    check_map("normals", disparity, 3);
    const int rows = disparity.rows(), cols = disparity.cols();
    normal_map.create(rows, 3 * cols, F32, disparity.memory());
    if (disparity.memory() == Memory::Host)
        throw_rc(bicos_normals_host(nullptr, disparity.data(), disparity.type(), rows, cols,
                                    Q.data(), p.flags, p.radius, p.max_diff, p.min_points,
                                    (float*)normal_map.data(), nullptr, 0, nullptr, nullptr));
    else
        throw_rc(bicos_normals_device(nullptr, disparity.data(), disparity.type(), rows, cols,
                                      Q.data(), p.flags, p.radius, p.max_diff, p.min_points,
                                      (float*)normal_map.data(), nullptr, 0, nullptr, nullptr,
                                      stream));
}

void normals(const Image& disparity, const Matx44d& Q, float* normal_map, const int32_t* index,
             size_t count, float* normals_out, uint32_t* counts, const NormalsParams& p,
             hipStream_t stream) {
    check_map("normals", disparity, 3);
    if (disparity.memory() != Memory::Device)
        throw Exception("normals: device buffers need a device map");
    throw_rc(bicos_normals_device(nullptr, disparity.data(), disparity.type(), disparity.rows(),
                                  disparity.cols(), Q.data(), p.flags, p.radius, p.max_diff,
                                  p.min_points, normal_map, index, count, normals_out, counts,
                                  stream));
}

NormalStats normals(const Image& disparity, const Matx44d& Q, const std::vector<int32_t>& index,
                    std::vector<float>& normals_out, const NormalsParams& p, Image* normal_map) {
    check_map("normals", disparity, 3);
    const int rows = disparity.rows(), cols = disparity.cols();
    const size_t count = index.size();
    uint32_t counts[4] = {0, 0, 0, 0};
    if (normal_map) normal_map->create(rows, 3 * cols, F32, disparity.memory());
    float* map = normal_map ? (float*)normal_map->data() : nullptr;
    std::vector<float> list(3 * count + 1);  // (+1: never a null pointer)
    std::vector<int32_t> idx(index);
    idx.push_back(0);  // (likewise)
    if (disparity.memory() == Memory::Host) {
        throw_rc(bicos_normals_host(nullptr, disparity.data(), disparity.type(), rows, cols,
                                    Q.data(), p.flags, p.radius, p.max_diff, p.min_points, map,
                                    idx.data(), count, list.data(), normal_map ? counts : nullptr));
    } else {
        // counts | normals | index in one allocation
        const DeviceBlock d("hipMalloc(normals)", 4, 3 * count, count);
        float* d_list = d.a<float>();
        int32_t* d_index = d.b<int32_t>();
        if (count)
            throw_rc(check_hip(hipMemcpy(d_index, index.data(), count * sizeof(int32_t),
                                         hipMemcpyHostToDevice), "index upload"));
        throw_rc(bicos_normals_device(nullptr, disparity.data(), disparity.type(), rows, cols,
                                      Q.data(), p.flags, p.radius, p.max_diff, p.min_points, map,
                                      d_index, count, d_list, normal_map ? d.counts() : nullptr,
                                      nullptr));
        if (normal_map) d.counts_down(counts);
        if (count)
            d.down(list.data(), d_list, count * 3 * sizeof(float), "normals download");
        else
            throw_rc(check_hip(hipStreamSynchronize(nullptr), "hipStreamSynchronize"));
    }
    list.resize(3 * count);
    normals_out.swap(list);
    return NormalStats{counts[0], counts[1], counts[2], counts[3]};
}

// --------------------------------------------------------------------- BICOS::mesh
// over the C entries (entries.cpp), which validate, lock the engine and launch

void mesh(const Image& disparity, const Matx44d& Q, float* points, int32_t* index,
          size_t vertex_capacity, uint32_t* counts, int32_t* triangles, size_t tri_capacity,
          uint32_t* mesh_counts, float max_diff, int flags, int32_t* vertex_map,
          hipStream_t stream) {
    check_map("mesh", disparity);
    if (disparity.memory() != Memory::Device)
        throw Exception("mesh: device buffers need a device map");
    throw_rc(bicos_mesh_device(current_engine(), disparity.data(), disparity.type(),
                               disparity.rows(), disparity.cols(), Q.data(), flags, max_diff,
                               points, index, vertex_capacity, counts, triangles, tri_capacity,
                               mesh_counts, vertex_map, stream));
}

MeshStats mesh(const Image& disparity, const Matx44d& Q, std::vector<float>& points,
               std::vector<int32_t>& triangles, float max_diff, int flags,
               std::vector<int32_t>* index) {
    check_map("mesh", disparity);
    const int rows = disparity.rows(), cols = disparity.cols();
    const size_t pixels = (size_t)(rows > 0 ? rows : 0) * (size_t)(cols > 0 ? cols : 0);
    const size_t tris = rows < 2 || cols < 2 ? 0 : 2 * (size_t)(rows - 1) * (size_t)(cols - 1);
    uint32_t counts[4] = {0, 0, 0, 0}, mesh_counts[4] = {0, 0, 0, 0};
    if (disparity.memory() == Memory::Host) {
        points.resize(3 * pixels + 1);  // (+1: never a null pointer)
        triangles.resize(3 * tris + 1);
        if (index) index->resize(pixels + 1);
        throw_rc(bicos_mesh_host(nullptr, disparity.data(), disparity.type(), rows, cols, Q.data(),
                                 flags, max_diff, points.data(), index ? index->data() : nullptr,
                                 pixels, counts, triangles.data(), tris, mesh_counts, nullptr));
    } else {
        // device buffers for every pixel and quad, then only what was kept and emitted comes
        // down: counts | mesh_counts | points | triangles | index in one allocation
        const DeviceBlock d("hipMalloc(mesh)", 8, 3 * pixels, 3 * tris + (index ? pixels : 0));
        uint32_t* d_counts = d.counts();
        float* d_points = d.a<float>();
        int32_t* d_tris = d.b<int32_t>();
        int32_t* d_index = index ? d_tris + 3 * tris : nullptr;
        // (a map without pixels launches nothing and needs no buffers: the entry zeroes the counts)
        throw_rc(bicos_mesh_device(current_engine(), disparity.data(), disparity.type(), rows,
                                   cols, Q.data(), flags, max_diff, d_points, d_index, pixels,
                                   d_counts, d_tris, tris, d_counts + 4, nullptr, nullptr));
        uint32_t both[8];
        d.counts_down(both);
        std::copy(both, both + 4, counts);
        std::copy(both + 4, both + 8, mesh_counts);
        points.resize(3 * (size_t)counts[0]);
        triangles.resize(3 * (size_t)mesh_counts[0]);
        if (index) index->resize(counts[0]);
        if (counts[0])
            d.down(points.data(), d_points, points.size() * sizeof(float), "points download");
        if (counts[0] && index)
            d.down(index->data(), d_index, index->size() * sizeof(int32_t), "index download");
        if (mesh_counts[0])
            d.down(triangles.data(), d_tris, triangles.size() * sizeof(int32_t),
                   "triangles download");
    }
    points.resize(3 * (size_t)counts[0]);
    triangles.resize(3 * (size_t)mesh_counts[0]);
    if (index) index->resize(counts[0]);
    MeshStats s;
    s.vertices = ReprojectStats{counts[0], counts[1], counts[2], counts[3]};
    s.triangles = mesh_counts[0];
    s.quads_full = mesh_counts[1];
    s.quads_half = mesh_counts[2];
    s.quads_empty = mesh_counts[3];
    return s;
}

// ------------------------------------------------------------------ BICOS::project
// over the C entries (entries.cpp), which validate, lock the engine and launch

namespace {
// The texture source as the entries take it: depth in bytes, pitch in elements
struct ImageArgs {
    const void* data = nullptr;
    int depth = 1, channels = 1;
    size_t pitch = 0;
};
ImageArgs image_args(const ProjectImage& image, const Camera& cam, Memory mem) {
    ImageArgs a;
    if (!image.image) return a;
    const Image& im = *image.image;
    if (im.type() != U8 && im.type() != U16) throw Exception("project: the image must be U8 or U16");
    if (image.channels != 1 && image.channels != 3)
        throw Exception("project: channels must be 1 or 3");
    if (im.rows() != cam.rows || (int64_t)im.cols() != (int64_t)cam.cols * image.channels)
        throw Exception("project: the image must be cam.rows x channels * cam.cols");
    if (im.memory() != mem)
        throw Exception("project: the image must be in the memory of the points");
    if (im.step() % im.elemSize()) throw Exception("project: the image's step splits an element");
    a.data = im.data();
    a.depth = (int)im.elemSize();
    a.channels = image.channels;
    a.pitch = im.step() / im.elemSize();
    return a;
}
void check_camera(const Camera& cam) {
    const size_t nd = cam.D.size();
    if (nd != 0 && nd != 4 && nd != 5 && nd != 8)
        throw Exception("project: D must hold 0, 4, 5 or 8 coefficients");
}
}  // namespace

void project(const float* points, size_t count, const Camera& cam, const ProjectDeviceOutputs& out,
             const ProjectParams& params, const ProjectImage& image, hipStream_t stream) {
    check_camera(cam);
    const ImageArgs im = image_args(image, cam, Memory::Device);
    throw_rc(bicos_project_device(
        current_engine(), points, count, cam.R.data(), cam.T.data(), cam.K.data(),
        cam.D.empty() ? nullptr : cam.D.data(), (int)cam.D.size(), cam.rows, cam.cols, params.splat,
        params.tol, im.data, im.depth, im.channels, im.pitch, params.fill, out.uv, out.depth,
        out.cls, out.tex, out.depth_map, out.index_map, out.counts, stream));
}

ProjectStats project(const float* points, size_t count, const Camera& cam,
                     const ProjectHostOutputs& out, const ProjectParams& params,
                     const ProjectImage& image) {
    check_camera(cam);
    const ImageArgs im = image_args(image, cam, Memory::Host);
    if (out.tex && !im.data) throw Exception("project: tex without image");
    const size_t pixels = (size_t)(cam.rows > 0 ? cam.rows : 0) * (size_t)(cam.cols > 0 ? cam.cols : 0);
    // (+1: never a null pointer)
    if (out.uv) out.uv->resize(2 * count + 1);
    if (out.depth) out.depth->resize(count + 1);
    if (out.cls) out.cls->resize(count + 1);
    if (out.tex) out.tex->resize(count * im.channels * im.depth + 1);
    if (out.depth_map) out.depth_map->resize(pixels + 1);
    if (out.index_map) out.index_map->resize(pixels + 1);
    uint32_t counts[5] = {0, 0, 0, 0, 0};
    const int rc = bicos_project_host(
        nullptr, points, count, cam.R.data(), cam.T.data(), cam.K.data(),
        cam.D.empty() ? nullptr : cam.D.data(), (int)cam.D.size(), cam.rows, cam.cols, params.splat,
        params.tol, im.data, im.depth, im.channels, im.pitch, params.fill,
        out.uv ? out.uv->data() : nullptr, out.depth ? out.depth->data() : nullptr,
        out.cls ? out.cls->data() : nullptr, out.tex ? (void*)out.tex->data() : nullptr,
        out.depth_map ? out.depth_map->data() : nullptr,
        out.index_map ? out.index_map->data() : nullptr, counts);
    if (out.uv) out.uv->resize(2 * count);
    if (out.depth) out.depth->resize(count);
    if (out.cls) out.cls->resize(count);
    if (out.tex) out.tex->resize(count * im.channels * im.depth);
    if (out.depth_map) out.depth_map->resize(pixels);
    if (out.index_map) out.index_map->resize(pixels);
    throw_rc(rc);
    return ProjectStats{counts[0], counts[1], counts[2], counts[3], counts[4]};
}

// ------------------------------------------------------ BICOS::guide_from_disparity
// over the C entries (entries.cpp), which validate and launch

void guide_from_disparity(const Image& prior, Image& guide, int rows, int cols,
                          const GuideParams& p, uint32_t* counts, hipStream_t stream) {
    check_map("guide_from_disparity", prior, 2, "prior");
    if (prior.memory() != Memory::Device)
        throw Exception("guide_from_disparity: device buffers need a device map");
    if (rows < 0 || cols < 0 || cols > INT32_MAX / 2)
        throw Exception("guide_from_disparity: bad guide size");
    guide.create(rows, 2 * cols, S16, Memory::Device);
    throw_rc(bicos_guide_device(nullptr, prior.data(), prior.type(), prior.rows(), prior.cols(),
                                rows, cols, p.scale, p.radius, p.spread, p.fallback_lo,
                                p.fallback_hi, p.flags, (int16_t*)guide.data(), guide.step() / 4,
                                counts, stream));
}

GuideStats guide_from_disparity(const Image& prior, Image& guide, int rows, int cols,
                                const GuideParams& p) {
    check_map("guide_from_disparity", prior, 2, "prior");
    if (rows < 0 || cols < 0 || cols > INT32_MAX / 2)
        throw Exception("guide_from_disparity: bad guide size");
    uint32_t counts[2] = {0, 0};
    if (prior.memory() == Memory::Host) {
        guide.create(rows, 2 * cols, S16, Memory::Host);
        throw_rc(bicos_guide_host(nullptr, prior.data(), prior.type(), prior.rows(), prior.cols(),
                                  rows, cols, p.scale, p.radius, p.spread, p.fallback_lo,
                                  p.fallback_hi, p.flags, (int16_t*)guide.data(),
                                  guide.step() / 4, counts));
    } else {
        const DeviceBlock d("hipMalloc(counts)", 2);
        guide_from_disparity(prior, guide, rows, cols, p, d.counts(), nullptr);
        d.counts_down(counts);
    }
    return GuideStats{counts[0], counts[1]};
}

// ------------------------------------------------- BICOS::rectify_maps, BICOS::rectify
// over the C entries (entries.cpp), which validate and launch

void rectify_maps(const RectifyCamera& camera, int rows, int cols, Image& map_x, Image& map_y,
                  Memory mem, hipStream_t stream) {
    const size_t np = camera.P.size();
    if (np != 9 && np != 12) throw Exception("rectify_maps: P must hold 3x3 or 3x4 values");
    if (rows < 1 || cols < 1) throw Exception("rectify_maps: the output size must be positive");
    map_x.create(rows, cols, F32, mem);
    map_y.create(rows, cols, F32, mem);
    const double* D = camera.D.empty() ? nullptr : camera.D.data();
    if (mem == Memory::Host)
        throw_rc(bicos_rectify_maps_host(camera.K, D, (int)camera.D.size(), camera.R,
                                         camera.P.data(), (int)np / 3, rows, cols,
                                         (float*)map_x.data(), (float*)map_y.data()));
    else
        throw_rc(bicos_rectify_maps_device(camera.K, D, (int)camera.D.size(), camera.R,
                                           camera.P.data(), (int)np / 3, rows, cols,
                                           (float*)map_x.data(), (float*)map_y.data(), stream));
}

namespace {

// The distance in bytes between the images when they form one planar buffer (one step, equally
// spaced, ascending), 0 when they do not; a single image is planar with any distance.
size_t planar_pitch(const std::vector<Image>& s) {
    const size_t row = (size_t)s[0].cols() * s[0].elemSize();
    if (s.size() == 1) return s[0].step() * (size_t)s[0].rows() + row;
    const char* base = (const char*)s[0].data();
    if ((const char*)s[1].data() <= base) return 0;
    const size_t pitch = (size_t)((const char*)s[1].data() - base);
    if (pitch % s[0].elemSize() || pitch < row) return 0;
    for (size_t t = 0; t < s.size(); ++t)
        if (s[t].step() != s[0].step() || (const char*)s[t].data() != base + t * pitch) return 0;
    return pitch;
}

}  // namespace

void rectify(const std::vector<Image>& stack, const Image& map_x, const Image& map_y,
             std::vector<Image>& out_stack, int border, Image* valid, hipStream_t stream) {
    if (stack.empty()) throw Exception("rectify: empty image stack");
    const Image& f = stack[0];
    const int type = f.type(), rows = map_x.rows(), cols = map_x.cols();
    if (type != U8 && type != U16) throw Exception("rectify: the images must be U8 or U16");
    const Memory mem = f.memory();
    for (const Image& im : stack)
        if (im.rows() != f.rows() || im.cols() != f.cols() || im.type() != type ||
            im.memory() != mem || !im.data())
            throw Exception("rectify: all images must share size, type and memory");
    if (map_x.type() != F32 || map_y.type() != F32 || map_y.rows() != rows || map_y.cols() != cols ||
        map_x.step() != map_y.step() || map_x.memory() != mem || map_y.memory() != mem)
        throw Exception("rectify: the maps must be F32 images of one shape and step in the "
                        "memory of the stack");
    if (rows < 1 || cols < 1) throw Exception("rectify: empty maps");
    if (&out_stack == &stack) throw Exception("rectify: the output must not be the source");
    const size_t n = stack.size(), depth = f.elemSize();
    out_stack.resize(n);
    for (Image& o : out_stack) o.create(rows, cols, type, mem);
    if (valid) valid->create(rows, cols, U8, mem);
    uint8_t* vp = valid ? (uint8_t*)valid->data() : nullptr;
    const float* mx = (const float*)map_x.data();
    const float* my = (const float*)map_y.data();
    if (mem == Memory::Host) {
        std::vector<const void*> src(n);
        std::vector<void*> dst(n);
        for (size_t t = 0; t < n; ++t) {
            if (stack[t].step() != f.step() || out_stack[t].step() != out_stack[0].step())
                throw Exception("rectify: host images of one stack must share one step");
            src[t] = stack[t].data();
            dst[t] = out_stack[t].data();
        }
        throw_rc(bicos_rectify_host(nullptr, src.data(), (int)n, f.rows(), f.cols(), f.step(),
                                    (int)depth, mx, my, map_x.step(), rows, cols, dst.data(),
                                    out_stack[0].step(), border, vp));
        return;
    }
    if (f.step() % depth || out_stack[0].step() % depth)
        throw Exception("rectify: an image step is not a multiple of the pixel size");
    const size_t sp = planar_pitch(stack), dp = planar_pitch(out_stack);
    if (sp && dp) {
        throw_rc(bicos_rectify_device(current_engine(), f.data(), (int)n, f.rows(), f.cols(),
                                      f.step() / depth, sp / depth, (int)depth, mx, my,
                                      map_x.step(), rows, cols, out_stack[0].data(),
                                      out_stack[0].step() / depth, dp / depth, border, vp, stream));
        return;
    }
    for (size_t t = 0; t < n; ++t) {
        const Image &s = stack[t], &o = out_stack[t];
        if (s.step() % depth || o.step() % depth)
            throw Exception("rectify: an image step is not a multiple of the pixel size");
        throw_rc(bicos_rectify_device(current_engine(), s.data(), 1, s.rows(), s.cols(),
                                      s.step() / depth, s.step() / depth * s.rows(), (int)depth, mx,
                                      my, map_x.step(), rows, cols, o.data(), o.step() / depth,
                                      o.step() / depth * o.rows(), border, t ? nullptr : vp, stream));
    }
}

// ---------------------------------------------------------------- BICOS::pool_stack
// over the C entries (entries.cpp), which validate and launch

void pool_stack(const std::vector<Image>& stack, int scale, std::vector<Image>& out_stack,
                hipStream_t stream) {
    if (stack.empty()) throw Exception("pool_stack: empty image stack");
    const Image& f = stack[0];
    const int type = f.type();
    if (type != U8 && type != U16) throw Exception("pool_stack: the images must be U8 or U16");
    if (scale < 2 || scale > 8) throw Exception("pool_stack: scale must lie in 2 .. 8");
    if (f.rows() < scale || f.cols() < scale)
        throw Exception("pool_stack: the images are smaller than scale x scale");
    const Memory mem = f.memory();
    for (const Image& im : stack)
        if (im.rows() != f.rows() || im.cols() != f.cols() || im.type() != type ||
            im.memory() != mem || !im.data())
            throw Exception("pool_stack: all images must share size, type and memory");
    if (&out_stack == &stack) throw Exception("pool_stack: the output must not be the source");
    const size_t n = stack.size(), depth = f.elemSize();
    const int prows = f.rows() / scale, pcols = f.cols() / scale;
    out_stack.resize(n);
    const bool fresh = std::none_of(out_stack.begin(), out_stack.end(), [&](const Image& o) {
        return o.data() && o.rows() == prows && o.cols() == pcols && o.type() == type &&
               o.memory() == mem;
    });
    if (fresh && mem == Memory::Device) {
        // one planar allocation for the n outputs: the one-launch path below, and a stack that
        // match() reads zero-copy
        const Image planar = Image::allocate((int)n * prows, pcols, type, mem);
        for (size_t t = 0; t < n; ++t)
            out_stack[t] = planar.rowRange((int)t * prows, (int)(t + 1) * prows);
    } else {
        for (Image& o : out_stack) o.create(prows, pcols, type, mem);
    }
    if (mem == Memory::Host) {
        std::vector<const void*> src(n);
        std::vector<void*> dst(n);
        for (size_t t = 0; t < n; ++t) {
            if (stack[t].step() != f.step() || out_stack[t].step() != out_stack[0].step())
                throw Exception("pool_stack: host images of one stack must share one step");
            src[t] = stack[t].data();
            dst[t] = out_stack[t].data();
        }
        throw_rc(bicos_pool_host(nullptr, src.data(), (int)n, f.rows(), f.cols(), f.step(),
                                 (int)depth, scale, dst.data(), out_stack[0].step()));
        return;
    }
    if (f.step() % depth || out_stack[0].step() % depth)
        throw Exception("pool_stack: an image step is not a multiple of the pixel size");
    const size_t sp = planar_pitch(stack), dp = planar_pitch(out_stack);
    if (sp && dp) {
        throw_rc(bicos_pool_device(nullptr, f.data(), (int)n, f.rows(), f.cols(), f.step() / depth,
                                   sp / depth, (int)depth, scale, out_stack[0].data(),
                                   out_stack[0].step() / depth, dp / depth, stream));
        return;
    }
    for (size_t t = 0; t < n; ++t) {
        const Image &s = stack[t], &o = out_stack[t];
        if (s.step() % depth || o.step() % depth)
            throw Exception("pool_stack: an image step is not a multiple of the pixel size");
        throw_rc(bicos_pool_device(nullptr, s.data(), 1, s.rows(), s.cols(), s.step() / depth,
                                   s.step() / depth * s.rows(), (int)depth, scale, o.data(),
                                   o.step() / depth, o.step() / depth * o.rows(), stream));
    }
}

}  // namespace BICOS
