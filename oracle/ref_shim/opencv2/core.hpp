/*
 * THIS IS NOT OPENCV. TEST INFRASTRUCTURE ONLY.
 *
 * A stand-in for <opencv2/core.hpp> that lets the reference's CPU path
 * (src/impl/cpu.cpp and the headers of include/impl/cpu/) compile unchanged into the
 * parity library oracle/_ref/libbicos_ref.so (see oracle/ref_driver.cpp and the
 * `ref` target of oracle/Makefile). It supplies what that code takes from cv::
 * and nothing else: containers and indexing. All of the reference's arithmetic
 * stays in the reference's own headers. The only value conversions here are
 * convertTo for int16 -> float and setTo, which casts its argument to the
 * element type.
 *
 * The reference relies on OpenCV's header pulling in <climits>, <cmath>,
 * <string> and alloca(); so does this one. ref_driver.cpp checks this file's
 * own behaviour (bicos_ref_shim_selfcheck, tests/test_reference_parity.py).
 */
#pragma once

#include <alloca.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#define CV_8U 0
#define CV_16U 2
#define CV_16S 3
#define CV_32F 5
#define CV_64F 6
#define CV_MAKETYPE(depth, cn) ((depth) + (((cn) - 1) << 3))
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_16UC1 CV_MAKETYPE(CV_16U, 1)

namespace cv {

/* Worker threads of parallel_for_: 0 = up to 16, bounded by the hardware. Not an
 * OpenCV name; set by ref_driver.cpp only. */
inline int ref_shim_threads = 0;

struct Size {
    int width = 0, height = 0;
    Size() = default;
    Size(int w, int h): width(w), height(h) {}
    size_t area() const {
        return (size_t)width * (size_t)height;
    }
};

struct Range {
    int start = 0, end = 0;
    Range() = default;
    Range(int s, int e): start(s), end(e) {}
};

template<typename T>
struct DataType;
template<>
struct DataType<uint8_t> {
    static constexpr int type = CV_8U;
};
template<>
struct DataType<uint16_t> {
    static constexpr int type = CV_16U;
};
template<>
struct DataType<int16_t> {
    static constexpr int type = CV_16S;
};
template<>
struct DataType<float> {
    static constexpr int type = CV_32F;
};
template<>
struct DataType<double> {
    static constexpr int type = CV_64F;
};

/* rows x cols pixels of channels() elements each, row r at data + r * step bytes.
 * Either owns a shared buffer (create) or views caller memory (the data constructor).
 * Copies share storage, as row() does. */
class Mat {
public:
    int rows = 0, cols = 0;

    Mat() = default;
    /* view over caller memory; step in bytes, 0 = rows are contiguous */
    Mat(int r, int c, int type, void* data, size_t step = 0):
        rows(r),
        cols(c),
        _type(type),
        _data((unsigned char*)data) {
        _step = step ? step : (size_t)c * elem_size();
    }

    int type() const {
        return _type;
    }
    int depth() const {
        return _type & 7;
    }
    int channels() const {
        return (_type >> 3) + 1;
    }
    Size size() const {
        return Size(cols, rows);
    }

    /* keeps the storage when size and type already match, as OpenCV's does */
    void create(Size sz, int type) {
        if (_data && rows == sz.height && cols == sz.width && _type == type)
            return;
        rows = sz.height;
        cols = sz.width;
        _type = type;
        _step = (size_t)cols * elem_size();
        const size_t bytes = _step * (size_t)rows;
        _owner = std::shared_ptr<unsigned char>(
            new unsigned char[bytes ? bytes : 1],
            std::default_delete<unsigned char[]>()
        );
        _data = _owner.get();
    }

    Mat row(int i) const {
        Mat m(*this);
        m.rows = 1;
        m._data = _data + (size_t)i * _step;
        return m;
    }

    template<typename T>
    T* ptr(int r = 0) {
        return (T*)(_data + (size_t)r * _step);
    }
    template<typename T>
    const T* ptr(int r = 0) const {
        return (const T*)(_data + (size_t)r * _step);
    }
    /* the channel vector of pixel (r, c) */
    template<typename T>
    T* ptr(int r, int c) {
        return (T*)(_data + (size_t)r * _step + (size_t)c * elem_size());
    }
    template<typename T>
    const T* ptr(int r, int c) const {
        return (const T*)(_data + (size_t)r * _step + (size_t)c * elem_size());
    }

    template<typename T>
    T& at(int r, int c) {
        return *ptr<T>(r, c);
    }
    template<typename T>
    const T& at(int r, int c) const {
        return *ptr<T>(r, c);
    }
    /* element i of a one-row Mat */
    template<typename T>
    T& at(int i) {
        return *ptr<T>(0, i);
    }
    template<typename T>
    const T& at(int i) const {
        return *ptr<T>(0, i);
    }

    /* every element := (element type)v */
    template<typename S>
    Mat& setTo(S v) {
        switch (depth()) {
            case CV_8U:
                fill<uint8_t>(v);
                break;
            case CV_16U:
                fill<uint16_t>(v);
                break;
            case CV_16S:
                fill<int16_t>(v);
                break;
            case CV_32F:
                fill<float>(v);
                break;
            case CV_64F:
                fill<double>(v);
                break;
            default:
                throw std::logic_error("ref_shim: setTo on an unknown depth");
        }
        return *this;
    }

    /* int16 -> float only: the one conversion the reference asks for (cpu.cpp) */
    void convertTo(Mat& dst, int rtype) const {
        if (_type != CV_16S || rtype != CV_32F)
            throw std::logic_error("ref_shim: convertTo supports CV_16S -> CV_32F only");
        Mat out;
        out.create(size(), CV_32F);
        for (int r = 0; r < rows; ++r) {
            const int16_t* s = ptr<int16_t>(r);
            float* d = out.ptr<float>(r);
            for (int c = 0; c < cols; ++c)
                d[c] = (float)s[c];
        }
        dst = out;
    }

    size_t elem_size1() const {
        switch (depth()) {
            case CV_8U:
                return 1;
            case CV_16U:
            case CV_16S:
                return 2;
            case CV_32F:
                return 4;
            default:
                return 8;
        }
    }
    size_t elem_size() const {
        return elem_size1() * (size_t)channels();
    }

private:
    template<typename T, typename S>
    void fill(S v) {
        const size_t per_row = (size_t)cols * (size_t)channels();
        for (int r = 0; r < rows; ++r) {
            T* p = ptr<T>(r);
            for (size_t i = 0; i < per_row; ++i)
                p[i] = (T)v;
        }
    }

    int _type = 0;
    size_t _step = 0;
    unsigned char* _data = nullptr;
    std::shared_ptr<unsigned char> _owner;
};

/* A Mat known to hold single-channel T. The reference only ever converts between Mats
 * of the same type, so a mismatch is an error here, not a conversion. */
template<typename T>
class Mat_: public Mat {
public:
    Mat_() = default;
    Mat_(const Mat& m): Mat(m) {
        if (m.rows && m.type() != DataType<T>::type)
            throw std::logic_error("ref_shim: Mat_ built from a Mat of another type");
    }
};

using Mat1s = Mat_<int16_t>;

/* dst(r, c)[k] = planes[k](r, c) */
inline void merge(const std::vector<Mat>& planes, Mat& dst) {
    const int n = (int)planes.size();
    const Mat& first = planes.front();
    const size_t es = first.elem_size1();
    Mat out;
    out.create(first.size(), CV_MAKETYPE(first.depth(), n));
    for (int k = 0; k < n; ++k) {
        const Mat& p = planes[k];
        if (p.type() != first.type() || p.rows != first.rows || p.cols != first.cols
            || p.channels() != 1)
            throw std::logic_error("ref_shim: merge needs equal single-channel planes");
        for (int r = 0; r < out.rows; ++r) {
            const unsigned char* s = p.ptr<unsigned char>(r);
            unsigned char* d = out.ptr<unsigned char>(r) + (size_t)k * es;
            for (int c = 0; c < out.cols; ++c)
                std::memcpy(d + (size_t)c * n * es, s + (size_t)c * es, es);
        }
    }
    dst = out;
}

/* body(Range) over disjoint sub-ranges that cover `range`; at most 16 threads */
template<typename Body>
void parallel_for_(const Range& range, const Body& body) {
    const int len = range.end - range.start;
    int nt = ref_shim_threads > 0 ? ref_shim_threads : (int)std::thread::hardware_concurrency();
    nt = std::max(1, std::min(std::min(nt, 16), len));
    if (nt == 1) {
        if (len > 0)
            body(range);
        return;
    }
    std::vector<std::thread> workers;
    workers.reserve(nt);
    for (int i = 0; i < nt; ++i) {
        const Range part(
            range.start + (int)((long long)len * i / nt),
            range.start + (int)((long long)len * (i + 1) / nt)
        );
        workers.emplace_back([&body, part] { body(part); });
    }
    for (auto& w: workers)
        w.join();
}

} // namespace cv
