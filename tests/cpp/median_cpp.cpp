// median_cpp.cpp -- TEST PROGRAM (tests/test_median_gpu.py, -m gpu): drives
// BICOS::median_filter (bicos/median.hpp) through each of its forms on one map, in host and in
// device memory, and writes the results for the Python test to compare with its restatement:
//   <out>.host.map / .dev.map     the filtered maps of the synchronous form
//   <out>.hostinplace.map         a host map filtered in place
//   <out>.buf.map                 the asynchronous device-buffer form
//
//   median_cpp <map.raw> <rows> <cols> <type 3|5> <flags> <ksize> <fill_min> <out_prefix>
// One line per form on stdout: "<form> unchanged changed filled invalid".
#include <bicos/common.hpp>
#include <bicos/median.hpp>
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace BICOS;

static void hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        std::fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e));
        std::exit(3);
    }
}

static void dump(const std::string& path, const void* p, size_t bytes) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) std::exit(4);
    std::fwrite(p, 1, bytes, f);
    std::fclose(f);
}

static void line(const char* form, const MedianStats& s) {
    std::printf("%s %u %u %u %u\n", form, s.unchanged, s.changed, s.filled, s.invalid);
}

int main(int argc, char** argv) {
    if (argc != 9) {
        std::fprintf(stderr, "usage: see header\n");
        return 2;
    }
    try {
        const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), type = std::atoi(argv[4]);
        const int flags = std::atoi(argv[5]), ksize = std::atoi(argv[6]);
        const int fill_min = std::atoi(argv[7]);
        const std::string out = argv[8];
        const size_t pixels = (size_t)rows * cols, bytes = pixels * Image::elem_size(type);
        std::vector<unsigned char> raw(bytes);
        FILE* f = std::fopen(argv[1], "rb");
        if (!f || std::fread(raw.data(), 1, bytes, f) != bytes) return 2;
        std::fclose(f);

        const Image host(rows, cols, type, raw.data(), 0, Memory::Host);
        Image dev = Image::allocate(rows, cols, type, Memory::Device);
        hip_ok(hipMemcpy(dev.data(), raw.data(), bytes, hipMemcpyHostToDevice), "upload");

        const struct {
            const char* name;
            const Image* map;
        } forms[] = {{"host", &host}, {"dev", &dev}};
        for (const auto& fm : forms) {
            Image filtered;
            const MedianStats s = median_filter(*fm.map, filtered, ksize, fill_min, flags);
            if (filtered.memory() != fm.map->memory() || filtered.rows() != rows ||
                filtered.cols() != cols || filtered.type() != type)
                return 5;
            if (filtered.data() == fm.map->data()) return 5;  // out of place
            const Image h = filtered.download();
            dump(out + "." + fm.name + ".map", h.data(), bytes);
            line(fm.name, s);
        }

        // a host map in place
        {
            Image own = Image::allocate(rows, cols, type, Memory::Host);
            std::memcpy(own.data(), raw.data(), bytes);
            const void* before = own.data();
            const MedianStats s = median_filter(own, own, ksize, fill_min, flags);
            if (own.data() != before) return 5;
            dump(out + ".hostinplace.map", own.data(), bytes);
            line("hostinplace", s);
        }

        // the asynchronous form on a stream of its own
        {
            void* buf = nullptr;
            hip_ok(hipMalloc(&buf, 16), "hipMalloc");
            hipStream_t st = nullptr;
            hip_ok(hipStreamCreate(&st), "hipStreamCreate");
            Image filtered;
            median_filter(dev, filtered, ksize, fill_min, flags, (uint32_t*)buf, st);
            hip_ok(hipStreamSynchronize(st), "sync");
            hip_ok(hipStreamDestroy(st), "hipStreamDestroy");
            uint32_t c[4];
            hip_ok(hipMemcpy(c, buf, sizeof c, hipMemcpyDeviceToHost), "download");
            hip_ok(hipFree(buf), "hipFree");
            const Image h = filtered.download();
            dump(out + ".buf.map", h.data(), bytes);
            line("buf", MedianStats{c[0], c[1], c[2], c[3]});
        }

        // the device map is as it was
        {
            const Image h = dev.download();
            if (std::memcmp(h.data(), raw.data(), bytes) != 0) return 7;
        }

        // errors are BICOS::Exception
        try {
            const Image bad(rows, cols, U8, raw.data(), 0, Memory::Host);
            Image o;
            median_filter(bad, o, 3);
            return 6;
        } catch (const Exception&) {
        }
        try {
            Image o;
            median_filter(host, o, 4);
            return 6;
        } catch (const Exception&) {
        }
        try {
            Image o;
            median_filter(host, o, 3, 10);
            return 6;
        } catch (const Exception&) {
        }
        try {
            median_filter(dev, dev, 3);  // a device map in place
            return 6;
        } catch (const Exception&) {
        }
        try {
            Image o;
            median_filter(host, o, 3, 0, 0, nullptr, nullptr);  // device buffers, host map
            return 6;
        } catch (const Exception&) {
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
