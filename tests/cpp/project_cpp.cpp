// project_cpp.cpp -- TEST PROGRAM (tests/test_project_cpp.py, -m gpu): drives BICOS::project
// (bicos/project.hpp) through both of its forms on one point list and writes the results for the
// Python test to compare with its restatement:
//   <out>.host.uv / .depth / .cls / .tex / .dmap / .imap   host vectors, everything in host memory
//   <out>.dev.uv  / ...                                     device buffers on a stream of its own
//
//   project_cpp <points.raw> <count> <camera.raw> <nd> <rows> <cols> <image.raw> <channels>
//               <depth 1|2> <pad> <splat> <tol> <fill> <out_prefix>
// camera.raw: float64 K[9] R[9] T[3] D[nd]; image.raw: rows x (cols*channels + pad) elements of
// `depth` bytes. One line per form on stdout: "<form> visible occluded outside behind invalid".
// It also checks that the error cases throw BICOS::Exception.
#include <bicos/common.hpp>
#include <bicos/project.hpp>
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
    if (bytes) std::fwrite(p, 1, bytes, f);
    std::fclose(f);
}

static bool slurp(const char* path, void* p, size_t bytes) {
    if (!bytes) return true;
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = std::fread(p, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

template <class F>
static bool throws(F&& f) {
    try {
        f();
    } catch (const Exception&) {
        return true;
    }
    return false;
}

int main(int argc, char** argv) {
    if (argc != 15) {
        std::fprintf(stderr, "usage: see header\n");
        return 2;
    }
    try {
        const size_t count = (size_t)std::atoll(argv[2]);
        const int nd = std::atoi(argv[4]), rows = std::atoi(argv[5]), cols = std::atoi(argv[6]);
        const int channels = std::atoi(argv[8]), depth = std::atoi(argv[9]);
        const int pad = std::atoi(argv[10]);
        ProjectParams params;
        params.splat = std::atoi(argv[11]);
        params.tol = (float)std::atof(argv[12]);
        params.fill = std::atoi(argv[13]);
        const std::string out = argv[14];

        std::vector<float> points(3 * count + 1);
        std::vector<double> c(21 + nd);
        const size_t pitch = (size_t)cols * channels + pad;
        std::vector<uint8_t> pixels(rows * pitch * depth + 1);
        if (!slurp(argv[1], points.data(), count * 12) || !slurp(argv[3], c.data(), c.size() * 8) ||
            !slurp(argv[7], pixels.data(), rows * pitch * depth))
            return 2;
        Camera cam;
        std::copy(c.begin(), c.begin() + 9, cam.K.begin());
        std::copy(c.begin() + 9, c.begin() + 18, cam.R.begin());
        std::copy(c.begin() + 18, c.begin() + 21, cam.T.begin());
        cam.D.assign(c.begin() + 21, c.end());
        cam.rows = rows;
        cam.cols = cols;
        const size_t npix = (size_t)rows * cols, texb = count * channels * depth;
        const int type = depth == 1 ? U8 : U16;

        // host vectors, a pitched host image
        {
            const Image img(rows, cols * channels, type, pixels.data(), pitch * depth, Memory::Host);
            std::vector<float> uv, z, dmap;
            std::vector<uint8_t> cls, tex;
            std::vector<int32_t> imap;
            ProjectHostOutputs o;
            o.uv = &uv, o.depth = &z, o.cls = &cls, o.tex = &tex, o.depth_map = &dmap;
            o.index_map = &imap;
            const ProjectStats s = project(points.data(), count, cam, o, params, {&img, channels});
            if (uv.size() != 2 * count || z.size() != count || cls.size() != count ||
                tex.size() != texb || dmap.size() != npix || imap.size() != npix)
                return 5;
            std::printf("host %u %u %u %u %u\n", s.visible, s.occluded, s.outside, s.behind,
                        s.invalid);
            dump(out + ".host.uv", uv.data(), uv.size() * 4);
            dump(out + ".host.depth", z.data(), z.size() * 4);
            dump(out + ".host.cls", cls.data(), cls.size());
            dump(out + ".host.tex", tex.data(), tex.size());
            dump(out + ".host.dmap", dmap.data(), dmap.size() * 4);
            dump(out + ".host.imap", imap.data(), imap.size() * 4);

            // what the layer refuses itself, and what the library refuses for it
            Camera bad = cam;
            bad.D.assign(3, 0.0);
            ProjectHostOutputs only_tex;
            only_tex.tex = &tex;
            ProjectParams wide = params;
            wide.splat = 4;
            const Image f32(rows, cols * channels, F32, pixels.data(), 0, Memory::Host);
            if (!throws([&] { project(points.data(), count, bad, o, params, {&img, channels}); }) ||
                !throws([&] { project(points.data(), count, cam, only_tex, params); }) ||
                !throws([&] { project(points.data(), count, cam, o, wide, {&img, channels}); }) ||
                !throws([&] { project(points.data(), count, cam, o, params, {&f32, channels}); }) ||
                !throws([&] { project(points.data(), count, cam, o, params, {&img, 2}); }) ||
                !throws([&] {
                    project(points.data(), count, cam, ProjectDeviceOutputs{}, params);
                })) {
                std::fprintf(stderr, "an error case did not throw\n");
                return 6;
            }
        }

        // device buffers on a stream of its own, a dense device image
        {
            Image img = Image::allocate(rows, cols * channels, type, Memory::Device);
            if (npix)
                hip_ok(hipMemcpy2D(img.data(), img.step(), pixels.data(), pitch * depth,
                                   (size_t)cols * channels * depth, rows, hipMemcpyHostToDevice),
                       "image upload");
            char* d = nullptr;
            const size_t at_uv = 0, at_z = at_uv + 8 * count, at_dm = at_z + 4 * count;
            const size_t at_im = at_dm + 4 * npix, at_cnt = at_im + 4 * npix, at_p = at_cnt + 32;
            const size_t at_tex = at_p + 12 * count, at_cls = at_tex + ((texb + 3) & ~(size_t)3);
            const size_t total = at_cls + count + 4;
            hip_ok(hipMalloc((void**)&d, total), "hipMalloc");
            hip_ok(hipMemcpy(d + at_p, points.data(), 12 * count, hipMemcpyHostToDevice), "points");
            hipStream_t st = nullptr;
            hip_ok(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "stream");
            ProjectDeviceOutputs o;
            o.uv = (float*)(d + at_uv), o.depth = (float*)(d + at_z), o.cls = (uint8_t*)(d + at_cls);
            o.tex = d + at_tex, o.depth_map = (float*)(d + at_dm), o.index_map = (int32_t*)(d + at_im);
            o.counts = (uint32_t*)(d + at_cnt);
            project((const float*)(d + at_p), count, cam, o, params, {&img, channels}, st);
            hip_ok(hipStreamSynchronize(st), "sync");
            std::vector<char> h(total);
            hip_ok(hipMemcpy(h.data(), d, total, hipMemcpyDeviceToHost), "download");
            const uint32_t* s = (const uint32_t*)(h.data() + at_cnt);
            std::printf("dev %u %u %u %u %u\n", s[0], s[1], s[2], s[3], s[4]);
            dump(out + ".dev.uv", h.data() + at_uv, 8 * count);
            dump(out + ".dev.depth", h.data() + at_z, 4 * count);
            dump(out + ".dev.cls", h.data() + at_cls, count);
            dump(out + ".dev.tex", h.data() + at_tex, texb);
            dump(out + ".dev.dmap", h.data() + at_dm, 4 * npix);
            dump(out + ".dev.imap", h.data() + at_im, 4 * npix);
            hip_ok(hipStreamDestroy(st), "stream destroy");
            hip_ok(hipFree(d), "hipFree");
        }
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
