// rectify_cpp.cpp -- TEST PROGRAM (tests/test_rectify_gpu.py, -m gpu): drives BICOS::rectify and
// BICOS::rectify_maps (bicos/rectify.hpp) through each of their forms and writes the results for
// the Python test to compare with its restatement:
//   <out>.host.stack / .host.valid          host images in and out
//   <out>.planar.stack / .planar.valid      device views of one planar buffer in and out
//   <out>.separate.stack / .separate.valid  device images allocated one by one
//   <out>.maps.host / .maps.dev             map_x then map_y of the camera in <cam.raw>
//
//   rectify_cpp <stack.raw> <n> <src_rows> <src_cols> <type 0|2> <map_x.raw> <map_y.raw> <rows>
//               <cols> <border> <cam.raw> <out_prefix>
// cam.raw: 38 doubles K[9] D[8] R[9] P[12].
#include <bicos/common.hpp>
#include <bicos/rectify.hpp>
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

static std::vector<unsigned char> slurp(const char* path, size_t bytes) {
    std::vector<unsigned char> v(bytes);
    FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), 1, bytes, f) != bytes) {
        std::fprintf(stderr, "cannot read %zu bytes of %s\n", bytes, path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

static void dump(const std::string& path, const std::vector<unsigned char>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) std::exit(4);
    std::fwrite(v.data(), 1, v.size(), f);
    std::fclose(f);
}

// the dense bytes of the images, one after another
static std::vector<unsigned char> gather(const std::vector<Image>& s) {
    std::vector<unsigned char> v;
    for (const Image& im : s) {
        const Image h = im.download();
        const size_t row = (size_t)h.cols() * h.elemSize();
        for (int y = 0; y < h.rows(); ++y) {
            const unsigned char* p = h.ptr<unsigned char>(y);
            v.insert(v.end(), p, p + row);
        }
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 13) {
        std::fprintf(stderr, "usage: see header\n");
        return 2;
    }
    try {
        const int n = std::atoi(argv[2]), sr = std::atoi(argv[3]), sc = std::atoi(argv[4]);
        const int type = std::atoi(argv[5]), rows = std::atoi(argv[8]), cols = std::atoi(argv[9]);
        const int border = std::atoi(argv[10]);
        const std::string out = argv[12];
        const size_t depth = Image::elem_size(type), plane = (size_t)sr * sc * depth;
        const size_t oplane = (size_t)rows * cols * depth, mbytes = (size_t)rows * cols * 4;
        std::vector<unsigned char> raw = slurp(argv[1], plane * n);
        std::vector<unsigned char> mx = slurp(argv[6], mbytes), my = slurp(argv[7], mbytes);

        // host
        {
            std::vector<Image> stack, result;
            for (int t = 0; t < n; ++t)
                stack.emplace_back(sr, sc, type, raw.data() + t * plane, 0, Memory::Host);
            const Image hx(rows, cols, F32, mx.data(), 0, Memory::Host);
            const Image hy(rows, cols, F32, my.data(), 0, Memory::Host);
            Image valid;
            rectify(stack, hx, hy, result, border, &valid);
            if ((int)result.size() != n || result[0].memory() != Memory::Host ||
                result[0].rows() != rows || result[0].cols() != cols || result[0].type() != type)
                return 5;
            dump(out + ".host.stack", gather(result));
            dump(out + ".host.valid", gather({valid}));
        }

        // device: everything in one allocation, the stacks as views of planar buffers
        void* buf = nullptr;
        hip_ok(hipMalloc(&buf, plane * n + oplane * n + 2 * mbytes + 1024), "hipMalloc");
        unsigned char* d_src = (unsigned char*)buf;
        unsigned char* d_mx = d_src + (plane * n + 255) / 256 * 256;
        unsigned char* d_my = d_mx + mbytes;
        unsigned char* d_dst = d_my + (mbytes + 255) / 256 * 256;
        hip_ok(hipMemcpy(d_src, raw.data(), plane * n, hipMemcpyHostToDevice), "upload");
        hip_ok(hipMemcpy(d_mx, mx.data(), mbytes, hipMemcpyHostToDevice), "upload");
        hip_ok(hipMemcpy(d_my, my.data(), mbytes, hipMemcpyHostToDevice), "upload");
        const Image dx(rows, cols, F32, d_mx, 0, Memory::Device);
        const Image dy(rows, cols, F32, d_my, 0, Memory::Device);
        {
            std::vector<Image> stack, result;
            for (int t = 0; t < n; ++t) {
                stack.emplace_back(sr, sc, type, d_src + t * plane, 0, Memory::Device);
                result.emplace_back(rows, cols, type, d_dst + t * oplane, 0, Memory::Device);
            }
            hipStream_t st = nullptr;
            hip_ok(hipStreamCreate(&st), "hipStreamCreate");
            Image valid;
            rectify(stack, dx, dy, result, border, &valid, st);
            hip_ok(hipStreamSynchronize(st), "sync");
            hip_ok(hipStreamDestroy(st), "hipStreamDestroy");
            for (int t = 0; t < n; ++t)
                if (result[t].data() != d_dst + t * oplane) return 5;  // written in place
            dump(out + ".planar.stack", gather(result));
            dump(out + ".planar.valid", gather({valid}));
        }
        {
            std::vector<Image> stack, result;
            for (int t = 0; t < n; ++t) {
                stack.push_back(Image::allocate(sr, sc, type, Memory::Device));
                hip_ok(hipMemcpy(stack[t].data(), raw.data() + t * plane, plane,
                                 hipMemcpyHostToDevice), "upload");
            }
            Image valid;
            rectify(stack, dx, dy, result, border, &valid);
            hip_ok(hipDeviceSynchronize(), "sync");
            if ((int)result.size() != n || result[0].memory() != Memory::Device) return 5;
            dump(out + ".separate.stack", gather(result));
            dump(out + ".separate.valid", gather({valid}));
        }

        // the maps of a camera, in both memories
        {
            const std::vector<unsigned char> cam = slurp(argv[11], 38 * sizeof(double));
            const double* c = (const double*)cam.data();
            RectifyCamera rc;
            std::memcpy(rc.K, c, sizeof rc.K);
            rc.D.assign(c + 9, c + 17);
            std::memcpy(rc.R, c + 17, sizeof rc.R);
            rc.P.assign(c + 26, c + 38);
            for (const Memory mem : {Memory::Host, Memory::Device}) {
                Image ax, ay;
                rectify_maps(rc, rows, cols, ax, ay, mem);
                hip_ok(hipDeviceSynchronize(), "sync");
                if (ax.memory() != mem || ax.type() != F32 || ay.rows() != rows) return 5;
                dump(out + (mem == Memory::Host ? ".maps.host" : ".maps.dev"), gather({ax, ay}));
            }
            // errors are BICOS::Exception
            try {
                rc.P.assign(12, 0.0);
                Image ax, ay;
                rectify_maps(rc, rows, cols, ax, ay);
                return 6;
            } catch (const Exception&) {
            }
        }
        try {
            std::vector<Image> stack{Image(sr, sc, type, d_src, 0, Memory::Device)}, result;
            rectify(stack, dx, dy, result, 70000);
            return 6;
        } catch (const Exception&) {
        }
        try {
            std::vector<Image> stack{Image(sr, sc, F32, d_src, 0, Memory::Device)}, result;
            rectify(stack, dx, dy, result);
            return 6;
        } catch (const Exception&) {
        }
        hip_ok(hipFree(buf), "hipFree");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
