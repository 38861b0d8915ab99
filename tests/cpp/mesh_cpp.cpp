// mesh_cpp.cpp -- TEST PROGRAM (tests/test_mesh_cpp.py, -m gpu): drives BICOS::mesh
// (bicos/mesh.hpp) through each of its forms on one map, in host and in device memory, and
// writes the results for the Python test to compare with its restatement:
//   <out>.host.pts / .tri / .idx     the host-vector form, map in host memory
//   <out>.dev.pts / .tri / .idx      the host-vector form, map in device memory
//   <out>.buf.pts / .tri / .idx / .vmap   the raw device-buffer form on a stream of its own
//
//   mesh_cpp <map.raw> <rows> <cols> <type 3|5> <Q.raw> <flags> <max_diff> <out_prefix>
// One line per form on stdout:
//   "<form> kept invalid nonfinite negative_z triangles quads_full quads_half quads_empty".
#include <bicos/common.hpp>
#include <bicos/mesh.hpp>
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

static void line(const std::string& form, const MeshStats& s) {
    std::printf("%s %u %u %u %u %u %u %u %u\n", form.c_str(), s.vertices.kept, s.vertices.invalid,
                s.vertices.nonfinite, s.vertices.negative_z, s.triangles, s.quads_full,
                s.quads_half, s.quads_empty);
}

int main(int argc, char** argv) {
    if (argc != 9) {
        std::fprintf(stderr, "usage: see header\n");
        return 2;
    }
    try {
        const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), type = std::atoi(argv[4]);
        const int flags = std::atoi(argv[6]);
        const float max_diff = (float)std::atof(argv[7]);
        const std::string out = argv[8];
        const size_t pixels = (size_t)rows * cols, bytes = pixels * Image::elem_size(type);
        const size_t tris = rows < 2 || cols < 2 ? 0 : 2 * (size_t)(rows - 1) * (cols - 1);
        std::vector<unsigned char> raw(bytes);
        Matx44d Q;
        if (!slurp(argv[1], raw.data(), bytes) || !slurp(argv[5], Q.data(), sizeof(double) * 16))
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
            std::vector<float> points(5, 1.f);
            std::vector<int32_t> triangles(7, 1), index(3, 1);
            const MeshStats s = mesh(*fm.map, Q, points, triangles, max_diff, flags, &index);
            if (points.size() != 3 * (size_t)s.vertices.kept || index.size() != s.vertices.kept ||
                triangles.size() != 3 * (size_t)s.triangles)
                return 5;
            dump(out + "." + name + ".pts", points.data(), points.size() * sizeof(float));
            dump(out + "." + name + ".tri", triangles.data(), triangles.size() * sizeof(int32_t));
            dump(out + "." + name + ".idx", index.data(), index.size() * sizeof(int32_t));
            line(name, s);
            // without the index: the same points and triangles
            std::vector<float> points2;
            std::vector<int32_t> triangles2;
            const MeshStats s2 = mesh(*fm.map, Q, points2, triangles2, max_diff, flags);
            if (points2 != points || triangles2 != triangles || s2.triangles != s.triangles)
                return 5;
        }

        // the raw device-buffer form on a stream of its own
        {
            float* d_points = nullptr;
            int32_t *d_index = nullptr, *d_tris = nullptr, *d_vmap = nullptr;
            uint32_t* d_counts = nullptr;
            hip_ok(hipMalloc((void**)&d_points, pixels * 12 + 4), "hipMalloc");
            hip_ok(hipMalloc((void**)&d_index, pixels * 4 + 4), "hipMalloc");
            hip_ok(hipMalloc((void**)&d_tris, tris * 12 + 4), "hipMalloc");
            hip_ok(hipMalloc((void**)&d_vmap, pixels * 4 + 4), "hipMalloc");
            hip_ok(hipMalloc((void**)&d_counts, 32), "hipMalloc");
            hipStream_t st = nullptr;
            hip_ok(hipStreamCreate(&st), "hipStreamCreate");
            mesh(dev, Q, d_points, d_index, pixels, d_counts, d_tris, tris, d_counts + 4, max_diff,
                 flags, d_vmap, st);
            hip_ok(hipStreamSynchronize(st), "sync");
            hip_ok(hipStreamDestroy(st), "hipStreamDestroy");
            uint32_t c[8];
            hip_ok(hipMemcpy(c, d_counts, sizeof c, hipMemcpyDeviceToHost), "download");
            std::vector<float> p(3 * (size_t)c[0] + 1);
            std::vector<int32_t> i((size_t)c[0] + 1), t(3 * (size_t)c[4] + 1), v(pixels + 1);
            hip_ok(hipMemcpy(p.data(), d_points, (size_t)c[0] * 12, hipMemcpyDeviceToHost), "download");
            hip_ok(hipMemcpy(i.data(), d_index, (size_t)c[0] * 4, hipMemcpyDeviceToHost), "download");
            hip_ok(hipMemcpy(t.data(), d_tris, (size_t)c[4] * 12, hipMemcpyDeviceToHost), "download");
            hip_ok(hipMemcpy(v.data(), d_vmap, pixels * 4, hipMemcpyDeviceToHost), "download");
            dump(out + ".buf.pts", p.data(), (size_t)c[0] * 12);
            dump(out + ".buf.idx", i.data(), (size_t)c[0] * 4);
            dump(out + ".buf.tri", t.data(), (size_t)c[4] * 12);
            dump(out + ".buf.vmap", v.data(), pixels * 4);
            MeshStats s;
            s.vertices = ReprojectStats{c[0], c[1], c[2], c[3]};
            s.triangles = c[4];
            s.quads_full = c[5];
            s.quads_half = c[6];
            s.quads_empty = c[7];
            line("buf", s);
            hip_ok(hipFree(d_points), "hipFree");
            hip_ok(hipFree(d_index), "hipFree");
            hip_ok(hipFree(d_tris), "hipFree");
            hip_ok(hipFree(d_vmap), "hipFree");
            hip_ok(hipFree(d_counts), "hipFree");
        }

        // the device map is as it was
        if (std::memcmp(dev.download().data(), raw.data(), bytes) != 0) return 7;

        // errors are BICOS::Exception
        std::vector<float> points;
        std::vector<int32_t> triangles;
        try {
            const Image bad(rows, cols, U8, raw.data(), 0, Memory::Host);
            mesh(bad, Q, points, triangles);
            return 6;
        } catch (const Exception&) {
        }
        for (const auto& fm : forms) {
            const Image* m = fm.map;
            try {
                mesh(*m, Q, points, triangles, -1.f);  // a negative max_diff
                return 6;
            } catch (const Exception&) {
            }
            try {
                mesh(*m, Q, points, triangles, 1.f, 4);  // an unknown flag
                return 6;
            } catch (const Exception&) {
            }
        }
        try {
            float one[3];
            int32_t tri[3];
            uint32_t c[8];
            mesh(host, Q, one, nullptr, 1, c, tri, 1, c + 4);  // device buffers, host map
            return 6;
        } catch (const Exception&) {
        }
        try {
            mesh(dev, Q, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr);  // no outputs
            return 6;
        } catch (const Exception&) {
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
