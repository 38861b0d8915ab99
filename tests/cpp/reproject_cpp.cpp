// reproject_cpp.cpp -- TEST PROGRAM (tests/test_reproject_gpu.py, -m gpu): drives
// BICOS::reproject (bicos/reproject.hpp) through each of its forms on one map, in host and in
// device memory, and writes the results for the Python test to compare with its restatement:
//   <out>.host.map / .dev.map      the dense maps (rows x 3*cols float32)
//   <out>.host.pts / .dev.pts      the point lists (float32 x 3), <out>.*.idx their pixels
//   <out>.buf.pts / .buf.idx       the device-buffer form with capacity = rows*cols
//
//   reproject_cpp <map.raw> <rows> <cols> <type 3|5> <flags> <out_prefix> <16 numbers of Q>
// One line per form on stdout: "<form> kept invalid nonfinite negative_z".
#include <bicos/common.hpp>
#include <bicos/reproject.hpp>
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

static void line(const char* form, const ReprojectStats& s) {
    std::printf("%s %u %u %u %u\n", form, s.kept, s.invalid, s.nonfinite, s.negative_z);
}

int main(int argc, char** argv) {
    if (argc != 7 + 16) {
        std::fprintf(stderr, "usage: see header\n");
        return 2;
    }
    try {
        const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), type = std::atoi(argv[4]);
        const int flags = std::atoi(argv[5]);
        const std::string out = argv[6];
        Matx44d Q;
        for (int i = 0; i < 16; ++i) Q[i] = std::strtod(argv[7 + i], nullptr);
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
            Image xyz;
            reproject(*fm.map, Q, xyz, flags);
            hip_ok(hipDeviceSynchronize(), "sync");
            if (xyz.memory() != fm.map->memory() || xyz.rows() != rows || xyz.cols() != 3 * cols ||
                xyz.type() != F32)
                return 5;
            const Image h = xyz.download();
            dump(out + "." + fm.name + ".map", h.data(), pixels * 12);
            std::vector<float> pts;
            std::vector<int32_t> idx;
            const ReprojectStats s = reproject(*fm.map, Q, pts, flags, &idx);
            if (pts.size() != 3 * (size_t)s.kept || idx.size() != s.kept) return 5;
            dump(out + "." + fm.name + ".pts", pts.data(), pts.size() * 4);
            dump(out + "." + fm.name + ".idx", idx.data(), idx.size() * 4);
            line(fm.name, s);
        }

        // device buffers: counts | points | index
        void* buf = nullptr;
        hip_ok(hipMalloc(&buf, 16 + pixels * 16), "hipMalloc");
        uint32_t* d_counts = (uint32_t*)buf;
        float* d_pts = (float*)buf + 4;
        int32_t* d_idx = (int32_t*)buf + 4 + 3 * pixels;
        reproject(dev, Q, d_pts, d_idx, pixels, d_counts, flags);
        std::vector<uint32_t> back(4 + 4 * pixels);
        hip_ok(hipMemcpy(back.data(), buf, back.size() * 4, hipMemcpyDeviceToHost), "download");
        hip_ok(hipFree(buf), "hipFree");
        dump(out + ".buf.pts", back.data() + 4, (size_t)back[0] * 12);
        dump(out + ".buf.idx", back.data() + 4 + 3 * pixels, (size_t)back[0] * 4);
        line("buf", ReprojectStats{back[0], back[1], back[2], back[3]});

        // errors are BICOS::Exception
        try {
            const Image bad(rows, cols, U8, raw.data(), 0, Memory::Host);
            std::vector<float> pts;
            reproject(bad, Q, pts);
            return 6;
        } catch (const Exception&) {
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
