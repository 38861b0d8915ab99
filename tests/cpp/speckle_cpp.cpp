// speckle_cpp.cpp -- TEST PROGRAM (tests/test_speckle_gpu.py, -m gpu): drives
// BICOS::filter_speckles (bicos/speckle.hpp) through each of its forms on one map, in host and
// in device memory, and writes the results for the Python test to compare with its restatement:
//   <out>.host.map / .dev.map     the filtered maps, <out>.host.lab / .dev.lab their labels
//   <out>.inplace.map             a device map filtered in place
//   <out>.buf.map / .buf.lab      the asynchronous device-buffer form
//
//   speckle_cpp <map.raw> <rows> <cols> <type 3|5> <flags> <max_size> <max_diff> <out_prefix>
// One line per form on stdout: "<form> kept removed invalid removed_components".
#include <bicos/common.hpp>
#include <bicos/speckle.hpp>
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
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

static void line(const char* form, const SpeckleStats& s) {
    std::printf("%s %u %u %u %u\n", form, s.kept, s.removed, s.invalid, s.removed_components);
}

int main(int argc, char** argv) {
    if (argc != 9) {
        std::fprintf(stderr, "usage: see header\n");
        return 2;
    }
    try {
        const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), type = std::atoi(argv[4]);
        const int flags = std::atoi(argv[5]), max_size = std::atoi(argv[6]);
        const float max_diff = std::strtof(argv[7], nullptr);
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
            std::vector<int32_t> labels;
            const SpeckleStats s = filter_speckles(*fm.map, filtered, max_size, max_diff, flags, &labels);
            if (filtered.memory() != fm.map->memory() || filtered.rows() != rows ||
                filtered.cols() != cols || filtered.type() != type || labels.size() != pixels)
                return 5;
            if (filtered.data() == fm.map->data()) return 5;  // out of place
            const Image h = filtered.download();
            dump(out + "." + fm.name + ".map", h.data(), bytes);
            dump(out + "." + fm.name + ".lab", labels.data(), pixels * 4);
            line(fm.name, s);
        }

        // the asynchronous form: labels | counts in one device buffer
        {
            void* buf = nullptr;
            hip_ok(hipMalloc(&buf, pixels * 4 + 16), "hipMalloc");
            int32_t* d_labels = (int32_t*)buf;
            uint32_t* d_counts = (uint32_t*)buf + pixels;
            hipStream_t st = nullptr;
            hip_ok(hipStreamCreate(&st), "hipStreamCreate");
            Image filtered;
            filter_speckles(dev, filtered, max_size, max_diff, flags, d_labels, d_counts, st);
            hip_ok(hipStreamSynchronize(st), "sync");
            hip_ok(hipStreamDestroy(st), "hipStreamDestroy");
            std::vector<uint32_t> back(pixels + 4);
            hip_ok(hipMemcpy(back.data(), buf, back.size() * 4, hipMemcpyDeviceToHost), "download");
            hip_ok(hipFree(buf), "hipFree");
            const Image h = filtered.download();
            dump(out + ".buf.map", h.data(), bytes);
            dump(out + ".buf.lab", back.data(), pixels * 4);
            const uint32_t* c = back.data() + pixels;
            line("buf", SpeckleStats{c[0], c[1], c[2], c[3]});
        }

        // in place, last: `dev` is the filtered map afterwards
        {
            const void* before = dev.data();
            const SpeckleStats s = filter_speckles(dev, dev, max_size, max_diff, flags);
            if (dev.data() != before) return 5;
            const Image h = dev.download();
            dump(out + ".inplace.map", h.data(), bytes);
            line("inplace", s);
        }

        // errors are BICOS::Exception
        try {
            const Image bad(rows, cols, U8, raw.data(), 0, Memory::Host);
            Image o;
            filter_speckles(bad, o, 1);
            return 6;
        } catch (const Exception&) {
        }
        try {
            Image o;
            filter_speckles(host, o, 1, -1.0f);
            return 6;
        } catch (const Exception&) {
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
