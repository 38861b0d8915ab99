// normals_cpp.cpp -- TEST PROGRAM (tests/test_normals_cpp.py, -m gpu): drives BICOS::normals
// (bicos/normals.hpp) through each of its forms on one map, in host and in device memory, and
// writes the results for the Python test to compare with its restatement:
//   <out>.host.map / .dev.map      the dense form
//   <out>.host.list / .dev.list    the list form alone
//   <out>.hostboth.map / .list, <out>.devboth.map / .list   the list form with the map
//   <out>.buf.map / .list          the raw device-buffer form on a stream of its own
//
//   normals_cpp <map.raw> <rows> <cols> <type 3|5> <Q.raw> <index.raw> <count> <flags> <radius>
//               <max_diff> <min_points> <out_prefix>
// One line per form that counts on stdout: "<form> normal no_point sparse degenerate".
#include <bicos/common.hpp>
#include <bicos/normals.hpp>
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

static bool slurp(const char* path, void* p, size_t bytes) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = std::fread(p, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

static void line(const std::string& form, const NormalStats& s) {
    std::printf("%s %u %u %u %u\n", form.c_str(), s.normal, s.no_point, s.sparse, s.degenerate);
}

int main(int argc, char** argv) {
    if (argc != 13) {
        std::fprintf(stderr, "usage: see header\n");
        return 2;
    }
    try {
        const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), type = std::atoi(argv[4]);
        const size_t count = (size_t)std::atoll(argv[7]);
        NormalsParams p;
        p.flags = std::atoi(argv[8]);
        p.radius = std::atoi(argv[9]);
        p.max_diff = (float)std::atof(argv[10]);
        p.min_points = std::atoi(argv[11]);
        const std::string out = argv[12];
        const size_t pixels = (size_t)rows * cols, bytes = pixels * Image::elem_size(type);
        const size_t map_bytes = pixels * 3 * sizeof(float), list_bytes = count * 3 * sizeof(float);
        std::vector<unsigned char> raw(bytes);
        Matx44d Q;
        std::vector<int32_t> index(count);
        if (!slurp(argv[1], raw.data(), bytes) || !slurp(argv[5], Q.data(), sizeof(double) * 16) ||
            !slurp(argv[6], index.data(), count * sizeof(int32_t)))
            return 2;

        const Image host(rows, cols, type, raw.data(), 0, Memory::Host);
        Image dev = Image::allocate(rows, cols, type, Memory::Device);
        hip_ok(hipMemcpy(dev.data(), raw.data(), bytes, hipMemcpyHostToDevice), "upload");

        const struct {
            const char* name;
            const Image* map;
        } forms[] = {{"host", &host}, {"dev", &dev}};
        for (const auto& fm : forms) {
            const std::string name = fm.name;
            // the dense form (a device map: asynchronous on the null stream; download() waits)
            Image nmap;
            normals(*fm.map, Q, nmap, p);
            if (nmap.memory() != fm.map->memory() || nmap.rows() != rows ||
                nmap.cols() != 3 * cols || nmap.type() != F32)
                return 5;
            dump(out + "." + name + ".map", nmap.download().data(), map_bytes);
            // the list alone: no map, no counts
            std::vector<float> list(7, 1.f);
            const NormalStats none = normals(*fm.map, Q, index, list, p);
            if (list.size() != 3 * count) return 5;
            if (none.normal || none.no_point || none.sparse || none.degenerate) return 5;
            dump(out + "." + name + ".list", list.data(), list_bytes);
            // the list with the map
            Image both;
            std::vector<float> list2;
            const NormalStats s = normals(*fm.map, Q, index, list2, p, &both);
            if (both.memory() != fm.map->memory() || list2.size() != 3 * count) return 5;
            dump(out + "." + name + "both.map", both.download().data(), map_bytes);
            dump(out + "." + name + "both.list", list2.data(), list_bytes);
            line(name + "both", s);
        }

        // the raw device-buffer form on a stream of its own
        {
            float *d_map = nullptr, *d_list = nullptr;
            int32_t* d_index = nullptr;
            uint32_t* d_counts = nullptr;
            hip_ok(hipMalloc((void**)&d_map, map_bytes + 4), "hipMalloc");
            hip_ok(hipMalloc((void**)&d_list, list_bytes + 4), "hipMalloc");
            hip_ok(hipMalloc((void**)&d_index, count * 4 + 4), "hipMalloc");
            hip_ok(hipMalloc((void**)&d_counts, 16), "hipMalloc");
            hip_ok(hipMemcpy(d_index, index.data(), count * 4, hipMemcpyHostToDevice), "upload");
            hipStream_t st = nullptr;
            hip_ok(hipStreamCreate(&st), "hipStreamCreate");
            normals(dev, Q, d_map, d_index, count, d_list, d_counts, p, st);
            hip_ok(hipStreamSynchronize(st), "sync");
            hip_ok(hipStreamDestroy(st), "hipStreamDestroy");
            std::vector<float> m(pixels * 3 + 1), l(count * 3 + 1);
            uint32_t c[4];
            hip_ok(hipMemcpy(m.data(), d_map, map_bytes, hipMemcpyDeviceToHost), "download");
            hip_ok(hipMemcpy(l.data(), d_list, list_bytes, hipMemcpyDeviceToHost), "download");
            hip_ok(hipMemcpy(c, d_counts, sizeof c, hipMemcpyDeviceToHost), "download");
            dump(out + ".buf.map", m.data(), map_bytes);
            dump(out + ".buf.list", l.data(), list_bytes);
            line("buf", NormalStats{c[0], c[1], c[2], c[3]});
            hip_ok(hipFree(d_map), "hipFree");
            hip_ok(hipFree(d_list), "hipFree");
            hip_ok(hipFree(d_index), "hipFree");
            hip_ok(hipFree(d_counts), "hipFree");
        }

        // the device map is as it was
        if (std::memcmp(dev.download().data(), raw.data(), bytes) != 0) return 7;

        // errors are BICOS::Exception
        try {
            const Image bad(rows, cols, U8, raw.data(), 0, Memory::Host);
            Image o;
            normals(bad, Q, o, p);
            return 6;
        } catch (const Exception&) {
        }
        for (int which = 0; which < 4; ++which) {
            NormalsParams q = p;
            if (which == 0) q.radius = 5;
            if (which == 1) q.max_diff = -1.f;
            if (which == 2) q.min_points = 2;
            if (which == 3) q.flags = 4;
            try {
                Image o;
                normals(host, Q, o, q);
                return 6;
            } catch (const Exception&) {
            }
        }
        try {
            float one[3];
            normals(host, Q, one, nullptr, 0, nullptr, nullptr, p);  // device buffers, host map
            return 6;
        } catch (const Exception&) {
        }
        try {
            normals(dev, Q, nullptr, nullptr, 0, nullptr, nullptr, p);  // no output
            return 6;
        } catch (const Exception&) {
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
