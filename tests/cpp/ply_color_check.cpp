// ply_color_check.cpp -- TEST PROGRAM (tests/test_project_api.py): bicos_cli::write_ply_colored
// (libbicos_amd/cli/imageio.cpp) alone, from raw files, so that the Python test can compare the
// .ply with its own packing of the header and the records. Needs no GPU.
//
//   ply_color_check <points.raw> <rgb.raw> <vertices> <triangles.raw> <faces> <out.ply>
// points.raw: float32 [vertices][3]; rgb.raw: uint8 [vertices][3]; triangles.raw: int32 [faces][3].
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
    if (argc != 7) {
        std::fprintf(stderr, "usage: ply_color_check points.raw rgb.raw vertices triangles.raw "
                             "faces out.ply\n");
        return 2;
    }
    try {
        const size_t vertices = (size_t)std::atoll(argv[3]), faces = (size_t)std::atoll(argv[5]);
        std::vector<float> points(3 * vertices + 1);
        std::vector<uint8_t> rgb(3 * vertices + 1);
        std::vector<int32_t> triangles(3 * faces + 1);
        if (!slurp(argv[1], points.data(), vertices * 12) ||
            !slurp(argv[2], rgb.data(), vertices * 3) ||
            !slurp(argv[4], triangles.data(), faces * 12))
            return 2;
        bicos_cli::write_ply_colored(argv[6], points.data(), rgb.data(), vertices,
                                     triangles.data(), faces);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
