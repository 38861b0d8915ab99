// ply_check.cpp -- TEST PROGRAM (tests/test_mesh_api.py): bicos_cli::write_ply
// (libbicos_amd/cli/imageio.cpp) alone, from raw files, so that the Python test can compare the
// .ply with its own packing of the header and the records. Needs no GPU.
//
//   ply_check <points.raw> <vertices> <triangles.raw> <faces> <out.ply>
// points.raw: float32 [vertices][3]; triangles.raw: int32 [faces][3].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include "../../libbicos_amd/cli/imageio.hpp"

static bool slurp(const char* path, void* p, size_t bytes) {
    if (!bytes) return true;
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = std::fread(p, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: ply_check points.raw vertices triangles.raw faces out.ply\n");
        return 2;
    }
    try {
        const size_t vertices = (size_t)std::atoll(argv[2]), faces = (size_t)std::atoll(argv[4]);
        std::vector<float> points(3 * vertices + 1);
        std::vector<int32_t> triangles(3 * faces + 1);
        if (!slurp(argv[1], points.data(), vertices * 12) ||
            !slurp(argv[3], triangles.data(), faces * 12))
            return 2;
        bicos_cli::write_ply(argv[5], points.data(), vertices, triangles.data(), faces);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
