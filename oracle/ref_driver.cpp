/*
 * ref_driver.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * extern "C" entry points over the reference's own CPU functions, for the parity
 * tests (tests/test_reference_parity.py through oracle/reference.py). The reference's
 * headers and src/impl/cpu.cpp are reached from the reference tree at build time
 * (oracle/Makefile, target `ref`) and compiled unchanged; cv:: is the stand-in in
 * oracle/ref_shim. Nothing of the reference is copied into this file.
 *
 * The call signatures follow oracle/bicos_oracle.h: planar stacks (plane t at
 * stack + t*rows*cols elements), descriptors as uint32 words with bit i at word
 * i/32, bit i%32. Descriptor objects are taken apart by shifting or indexing.
 */
#include <bitset>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <optional>
#include <stdexcept>
#include <vector>

#include "cpu.hpp"
#include "impl/cpu/agree.hpp"
#include "impl/cpu/bicos.hpp"
#include "impl/cpu/descriptor_transform.hpp"

namespace {

using namespace BICOS;
using namespace BICOS::impl;
using namespace BICOS::impl::cpu;

struct ref_config { /* = bicos_oracle_config */
    int has_nxcorr;
    float nxcorr_threshold;
    int has_step;
    float subpixel_step;
    int has_minvar;
    float min_variance;
    int mode, variant, max_lr_diff, no_dupes;
};

enum { ERR_BICOS = -1, ERR_INVALID_ARGUMENT = -3, ERR_OTHER = -9 };

void say(char* err, int errlen, const char* what) {
    if (err && errlen > 0)
        std::snprintf(err, (size_t)errlen, "%s", what);
}

int cv_depth(int depth) {
    return depth == 1 ? CV_8U : CV_16U;
}

/* n single-channel views, one per plane of a caller's planar stack */
std::vector<cv::Mat> planes(const void* stack, int n, int rows, int cols, int depth) {
    std::vector<cv::Mat> v;
    for (int t = 0; t < n; ++t)
        v.emplace_back(
            rows,
            cols,
            CV_MAKETYPE(cv_depth(depth), 1),
            (unsigned char*)stack + (size_t)t * rows * cols * depth
        );
    return v;
}

cv::Mat merged(const void* stack, int n, int rows, int cols, int depth) {
    cv::Mat m;
    cv::merge(planes(stack, n, rows, cols, depth), m);
    return m;
}

/* ---- descriptor objects <-> uint32 words */

void to_words(uint32_t d, uint32_t* w) {
    w[0] = d;
}
void to_words(uint64_t d, uint32_t* w) {
    for (int k = 0; k < 2; ++k)
        w[k] = (uint32_t)(d >> (32 * k));
}
void to_words(uint128_t d, uint32_t* w) {
    for (int k = 0; k < 4; ++k)
        w[k] = (uint32_t)(d >> (32 * k));
}
void to_words(const std::bitset<256>& d, uint32_t* w) {
    for (int k = 0; k < 8; ++k) {
        uint32_t x = 0;
        for (int b = 0; b < 32; ++b)
            x |= (uint32_t)d[(size_t)(32 * k + b)] << b;
        w[k] = x;
    }
}

void from_words(const uint32_t* w, uint32_t& d) {
    d = w[0];
}
void from_words(const uint32_t* w, uint64_t& d) {
    d = 0;
    for (int k = 0; k < 2; ++k)
        d |= (uint64_t)w[k] << (32 * k);
}
void from_words(const uint32_t* w, uint128_t& d) {
    d = 0;
    for (int k = 0; k < 4; ++k)
        d |= (uint128_t)w[k] << (32 * k);
}
void from_words(const uint32_t* w, std::bitset<256>& d) {
    d.reset();
    for (int i = 0; i < 256; ++i)
        if ((w[i / 32] >> (i % 32)) & 1u)
            d.set((size_t)i);
}

template<typename T>
constexpr int words_of() {
    return (int)(sizeof(T) / 4);
}

/* ---- stages */

template<typename TInput, typename TDesc>
void run_transform(const cv::Mat& stack, cv::Size sz, int n, int mode, uint32_t* out) {
    std::unique_ptr<StepBuf<TDesc>> d = mode == 1
        ? descriptor_transform<TInput, TDesc, transform_full>(stack, sz, (size_t)n)
        : descriptor_transform<TInput, TDesc, transform_limited>(stack, sz, (size_t)n);
    const int words = words_of<TDesc>();
    for (int r = 0; r < sz.height; ++r)
        for (int c = 0; c < sz.width; ++c)
            to_words(d->row(r)[c], out + ((size_t)r * sz.width + c) * words);
}

template<typename TDesc>
void run_search(
    const uint32_t* w0,
    const uint32_t* w1,
    cv::Size sz,
    int flags,
    int max_lr_diff,
    int16_t* out
) {
    const int words = words_of<TDesc>();
    auto d0 = std::make_unique<StepBuf<TDesc>>(sz), d1 = std::make_unique<StepBuf<TDesc>>(sz);
    for (int r = 0; r < sz.height; ++r)
        for (int c = 0; c < sz.width; ++c) {
            const size_t i = ((size_t)r * sz.width + c) * words;
            from_words(w0 + i, d0->row(r)[c]);
            from_words(w1 + i, d1->row(r)[c]);
        }
    cv::Mat disp(sz.height, sz.width, CV_16S, out); /* bicos() keeps a fitting Mat */
    switch (flags) {
        case BICOSFLAGS_NODUPES:
            bicos<TDesc, BICOSFLAGS_NODUPES>(d0, d1, max_lr_diff, sz, disp);
            break;
        case BICOSFLAGS_CONSISTENCY:
            bicos<TDesc, BICOSFLAGS_CONSISTENCY>(d0, d1, max_lr_diff, sz, disp);
            break;
        case BICOSFLAGS_NODUPES | BICOSFLAGS_CONSISTENCY:
            bicos<TDesc, BICOSFLAGS_NODUPES | BICOSFLAGS_CONSISTENCY>(d0, d1, max_lr_diff, sz, disp);
            break;
        default:
            throw std::logic_error("ref_driver: flags must be 1, 2 or 3");
    }
    if (disp.ptr<int16_t>(0) != out) /* it did not: copy */
        for (int r = 0; r < sz.height; ++r)
            std::memcpy(out + (size_t)r * sz.width, disp.ptr<int16_t>(r), sizeof(int16_t) * sz.width);
}

template<typename F>
int guarded(char* err, int errlen, F f) {
    try {
        return f();
    } catch (const BICOS::Exception& e) {
        say(err, errlen, e.what());
        return ERR_BICOS;
    } catch (const std::invalid_argument& e) {
        say(err, errlen, e.what());
        return ERR_INVALID_ARGUMENT;
    } catch (const std::exception& e) {
        say(err, errlen, e.what());
        return ERR_OTHER;
    }
}

std::optional<float> opt(int has, float v) {
    return has ? std::optional<float>(v) : std::nullopt;
}

} // namespace

extern "C" {

/* BICOS::impl::cpu::match. disp_out holds rows*cols 4-byte elements (an int16 result
 * fills the first half). Returns 0 (int16 map), 1 (float32 map and corrmap) -- read off
 * the Mats the reference returned -- or a negative error with its message in err. */
int bicos_ref_match(
    const void* stack0,
    const void* stack1,
    int n,
    int rows,
    int cols,
    int depth,
    const ref_config* c,
    void* disp_out,
    float* corrmap,
    int nthreads,
    char* err,
    int errlen
) {
    cv::ref_shim_threads = nthreads;
    return guarded(err, errlen, [&]() -> int {
        Config cfg;
        cfg.nxcorr_threshold = opt(c->has_nxcorr, c->nxcorr_threshold);
        cfg.subpixel_step = opt(c->has_step, c->subpixel_step);
        cfg.min_variance = opt(c->has_minvar, c->min_variance);
        cfg.mode = c->mode == 1 ? TransformMode::FULL : TransformMode::LIMITED;
        if (c->variant == 1) {
            Variant::Consistency v;
            v.max_lr_diff = c->max_lr_diff;
            v.no_dupes = c->no_dupes != 0;
            cfg.variant = v;
        } else
            cfg.variant = Variant::NoDuplicates {};

        cv::Mat disp, corr;
        match(planes(stack0, n, rows, cols, depth), planes(stack1, n, rows, cols, depth), disp, cfg, &corr);

        if (disp.rows != rows || disp.cols != cols)
            throw std::logic_error("ref_driver: disparity map has another size");
        int kind;
        size_t es;
        if (disp.type() == CV_16S)
            kind = 0, es = 2;
        else if (disp.type() == CV_32F)
            kind = 1, es = 4;
        else
            throw std::logic_error("ref_driver: disparity map has an unexpected type");
        for (int r = 0; r < rows; ++r)
            std::memcpy((char*)disp_out + (size_t)r * cols * es, disp.ptr<unsigned char>(r), (size_t)cols * es);
        if (corr.rows) {
            if (corr.type() != CV_32F || corr.rows != rows || corr.cols != cols)
                throw std::logic_error("ref_driver: corrmap has an unexpected type or size");
            for (int r = 0; r < rows; ++r)
                std::memcpy(corrmap + (size_t)r * cols, corr.ptr<float>(r), sizeof(float) * cols);
        } else if (kind == 1)
            throw std::logic_error("ref_driver: float result without a corrmap");
        return kind;
    });
}

/* descriptor_transform<TInput, TDescriptor, transform_limited | transform_full>, the
 * descriptor type chosen by `words` (1, 2, 4, 8) */
int bicos_ref_transform(
    const void* stack,
    int n,
    int rows,
    int cols,
    int depth,
    int mode,
    int words,
    uint32_t* desc,
    int nthreads,
    char* err,
    int errlen
) {
    cv::ref_shim_threads = nthreads;
    return guarded(err, errlen, [&]() -> int {
        /* bits the transform writes: LIMITED 3 per triple, one per pair sum that has a
         * predecessor, 4 at the end; FULL n^2-2n+3. Shifting past the descriptor is undefined. */
        const int bits = mode == 1 ? n * n - 2 * n + 3 : 3 * (n - 2) + (n > 4 ? n - 4 : 0) + 4;
        if (n < 2 || bits > 32 * words)
            throw std::logic_error("ref_driver: descriptor too narrow for this stack");
        const cv::Mat s = merged(stack, n, rows, cols, depth);
        const cv::Size sz(cols, rows);
#define RUN(W, T)                                                   \
    case W:                                                         \
        if (depth == 1)                                             \
            run_transform<uint8_t, T>(s, sz, n, mode, desc);        \
        else                                                        \
            run_transform<uint16_t, T>(s, sz, n, mode, desc);       \
        break;
        switch (words) {
            RUN(1, uint32_t)
            RUN(2, uint64_t)
            RUN(4, uint128_t)
            RUN(8, std::bitset<256>)
            default:
                throw std::logic_error("ref_driver: words must be 1, 2, 4 or 8");
        }
#undef RUN
        return 0;
    });
}

/* bicos<TDescriptor, FLAGS> on caller-given descriptors */
int bicos_ref_search(
    const uint32_t* desc0,
    const uint32_t* desc1,
    int rows,
    int cols,
    int words,
    int flags,
    int max_lr_diff,
    int16_t* disp,
    int nthreads,
    char* err,
    int errlen
) {
    cv::ref_shim_threads = nthreads;
    return guarded(err, errlen, [&]() -> int {
        const cv::Size sz(cols, rows);
        switch (words) {
            case 1:
                run_search<uint32_t>(desc0, desc1, sz, flags, max_lr_diff, disp);
                break;
            case 2:
                run_search<uint64_t>(desc0, desc1, sz, flags, max_lr_diff, disp);
                break;
            case 4:
                run_search<uint128_t>(desc0, desc1, sz, flags, max_lr_diff, disp);
                break;
            case 8:
                run_search<std::bitset<256>>(desc0, desc1, sz, flags, max_lr_diff, disp);
                break;
            default:
                throw std::logic_error("ref_driver: words must be 1, 2, 4 or 8");
        }
        return 0;
    });
}

/* agree<TInput>: disp (int16) is updated in place, corrmap written where the reference
 * writes it. minvar_scaled is what match() would pass: min_variance * n. */
int bicos_ref_agree(
    int16_t* disp,
    const void* stack0,
    const void* stack1,
    int n,
    int rows,
    int cols,
    int depth,
    float threshold,
    int has_minvar,
    float minvar_scaled,
    float* corrmap,
    int nthreads,
    char* err,
    int errlen
) {
    cv::ref_shim_threads = nthreads;
    return guarded(err, errlen, [&]() -> int {
        const cv::Mat s0 = merged(stack0, n, rows, cols, depth), s1 = merged(stack1, n, rows, cols, depth);
        cv::Mat raw(rows, cols, CV_16S, disp), corr(rows, cols, CV_32F, corrmap);
        if (depth == 1)
            agree<uint8_t>(raw, s0, s1, (size_t)n, threshold, opt(has_minvar, minvar_scaled), corrmap ? &corr : nullptr);
        else
            agree<uint16_t>(raw, s0, s1, (size_t)n, threshold, opt(has_minvar, minvar_scaled), corrmap ? &corr : nullptr);
        return 0;
    });
}

/* agree_subpixel<TInput> */
int bicos_ref_agree_subpixel(
    const int16_t* disp,
    const void* stack0,
    const void* stack1,
    int n,
    int rows,
    int cols,
    int depth,
    float threshold,
    float step,
    int has_minvar,
    float minvar_scaled,
    float* out,
    float* corrmap,
    int nthreads,
    char* err,
    int errlen
) {
    cv::ref_shim_threads = nthreads;
    return guarded(err, errlen, [&]() -> int {
        const cv::Mat s0 = merged(stack0, n, rows, cols, depth), s1 = merged(stack1, n, rows, cols, depth);
        const cv::Mat1s raw(cv::Mat(rows, cols, CV_16S, (void*)disp));
        cv::Mat ret, corr(rows, cols, CV_32F, corrmap);
        if (depth == 1)
            agree_subpixel<uint8_t>(raw, s0, s1, (size_t)n, threshold, step, opt(has_minvar, minvar_scaled), ret, corrmap ? &corr : nullptr);
        else
            agree_subpixel<uint16_t>(raw, s0, s1, (size_t)n, threshold, step, opt(has_minvar, minvar_scaled), ret, corrmap ? &corr : nullptr);
        if (ret.type() != CV_32F || ret.rows != rows || ret.cols != cols)
            throw std::logic_error("ref_driver: subpixel map has an unexpected type or size");
        for (int r = 0; r < rows; ++r)
            std::memcpy(out + (size_t)r * cols, ret.ptr<float>(r), sizeof(float) * cols);
        return 0;
    });
}

/* Checks of the stand-in itself (oracle/ref_shim). Returns 0, or the number of the first
 * check that failed:
 *   1x merge: plane k of pixel (r, c) is ptr<T>(r, c)[k], u8 (11) and u16 (12)
 *   2x views over caller memory honour the row stride
 *   3x row(), at and ptr alias the same storage; copies share it; create keeps a fit
 *   4x convertTo maps int16 to the same float, -32768 included
 *   5x setTo(NaN) fills a float Mat; setTo casts to int16
 *   6x parallel_for_ covers the range exactly once */
int bicos_ref_shim_selfcheck(void) {
    try {
        { /* merge */
            const int n = 5, rows = 3, cols = 4;
            std::vector<uint8_t> a((size_t)n * rows * cols);
            std::vector<uint16_t> b((size_t)n * rows * cols);
            for (size_t i = 0; i < a.size(); ++i) {
                a[i] = (uint8_t)(i * 7 + 1);
                b[i] = (uint16_t)(i * 1031 + 40000);
            }
            const cv::Mat ma = merged(a.data(), n, rows, cols, 1), mb = merged(b.data(), n, rows, cols, 2);
            if (ma.channels() != n || ma.depth() != CV_8U || ma.rows != rows || ma.cols != cols)
                return 11;
            if (mb.channels() != n || mb.depth() != CV_16U || mb.type() != CV_MAKETYPE(CV_16U, n))
                return 12;
            for (int k = 0; k < n; ++k)
                for (int r = 0; r < rows; ++r)
                    for (int c = 0; c < cols; ++c) {
                        const size_t i = ((size_t)k * rows + r) * cols + c;
                        if (ma.ptr<uint8_t>(r, c)[k] != a[i])
                            return 11;
                        if (mb.ptr<uint16_t>(r, c)[k] != b[i])
                            return 12;
                    }
        }
        { /* strided view: 3 rows of 4 int16 inside rows of 7 */
            int16_t buf[3 * 7];
            for (int i = 0; i < 21; ++i)
                buf[i] = (int16_t)(100 + i);
            cv::Mat v(3, 4, CV_16S, buf, 7 * sizeof(int16_t));
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c)
                    if (v.at<int16_t>(r, c) != 100 + 7 * r + c || v.ptr<int16_t>(r) != buf + 7 * r)
                        return 21;
            v.row(1).setTo(-5);
            for (int i = 0; i < 21; ++i)
                if (buf[i] != ((i >= 7 && i < 11) ? -5 : 100 + i))
                    return 22;
            /* a merged Mat of strided planes */
            std::vector<cv::Mat> pl;
            for (int k = 0; k < 2; ++k)
                pl.emplace_back(3, 2, CV_16S, buf + 2 * k, 7 * sizeof(int16_t));
            cv::Mat m;
            cv::merge(pl, m);
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 2; ++c)
                    for (int k = 0; k < 2; ++k)
                        if (m.ptr<int16_t>(r, c)[k] != buf[7 * r + 2 * k + c])
                            return 23;
        }
        { /* aliasing */
            cv::Mat m;
            m.create(cv::Size(5, 4), CV_32F);
            if (m.rows != 4 || m.cols != 5 || m.size().width != 5 || m.size().height != 4 || m.size().area() != 20)
                return 31;
            m.setTo(0.f);
            cv::Mat row = m.row(2);
            if (row.rows != 1 || row.cols != 5)
                return 31;
            row.at<float>(3) = 7.f;
            if (m.at<float>(2, 3) != 7.f || m.ptr<float>(2)[3] != 7.f || *m.ptr<float>(2, 3) != 7.f)
                return 32;
            if (&row.at<float>(3) != &m.at<float>(2, 3) || m.ptr<float>(2, 3) != m.ptr<float>(2) + 3)
                return 32;
            cv::Mat copy = m;
            copy.at<float>(0, 0) = 3.f;
            if (m.at<float>(0, 0) != 3.f)
                return 33;
            cv::Mat_<float> typed = m;
            if (typed.ptr<float>(0) != m.ptr<float>(0))
                return 33;
            const float* before = m.ptr<float>(0);
            m.create(cv::Size(5, 4), CV_32F);
            if (m.ptr<float>(0) != before)
                return 34;
            m.create(cv::Size(5, 4), CV_16S);
            if (m.type() != CV_16S || (const void*)m.ptr<int16_t>(0) == (const void*)before)
                return 34;
            if (copy.type() != CV_32F || copy.at<float>(2, 3) != 7.f)
                return 34;
        }
        { /* convertTo */
            int16_t v[6] = {-32768, -1, 0, 1, 255, 32767};
            cv::Mat s(2, 3, CV_16S, v), d;
            s.convertTo(d, CV_32F);
            if (d.type() != CV_32F || d.rows != 2 || d.cols != 3)
                return 41;
            for (int i = 0; i < 6; ++i)
                if (d.at<float>(i / 3, i % 3) != (float)v[i])
                    return 42;
            if (d.at<float>(0, 0) != -32768.0f)
                return 42;
        }
        { /* setTo */
            cv::Mat f;
            f.create(cv::Size(3, 2), cv::DataType<float>::type);
            f.setTo(0.f);
            f.setTo(std::numeric_limits<float>::quiet_NaN());
            for (int r = 0; r < 2; ++r)
                for (int c = 0; c < 3; ++c)
                    if (f.at<float>(r, c) == f.at<float>(r, c))
                        return 51;
            cv::Mat s;
            s.create(cv::Size(3, 2), cv::DataType<int16_t>::type);
            s.setTo(std::numeric_limits<int16_t>::lowest());
            for (int r = 0; r < 2; ++r)
                for (int c = 0; c < 3; ++c)
                    if (s.at<int16_t>(r, c) != -32768)
                        return 52;
        }
        { /* parallel_for_ */
            for (int threads: {0, 1, 3, 16, 64})
                for (int len: {0, 1, 2, 17, 100}) {
                    cv::ref_shim_threads = threads;
                    std::vector<int> hits((size_t)len + 2, 0);
                    cv::parallel_for_(cv::Range(1, 1 + len), [&](const cv::Range& r) {
                        for (int i = r.start; i < r.end; ++i)
                            hits[(size_t)i]++;
                    });
                    cv::ref_shim_threads = 0;
                    for (int i = 0; i < len + 2; ++i)
                        if (hits[(size_t)i] != (i >= 1 && i <= len ? 1 : 0))
                            return 61;
                }
        }
    } catch (const std::exception&) {
        return 99;
    }
    return 0;
}

} // extern "C"
