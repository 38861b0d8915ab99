// pool_cpp.cpp -- TEST PROGRAM (tests/test_pool_cpp.py, -m gpu): drives BICOS::pool_stack and
// BICOS::match_pyramid (bicos/pool.hpp) on the stacks the Python test wrote, in host and in
// device memory, and writes the results for it to compare with the Python device path:
//   <out>.host.pool / .dev.pool      the pooled left stack (planar, dense)
//   <out>.host.disp / .dev.disp      the pyramid's disparity maps (float32)
//   <out>.host.corr / .dev.corr      their corrmaps (float32)
//   <out>.host.coarse / .dev.coarse  the coarse maps (float32)
//   <out>.host.guide / .dev.guide    the guides (int16 pairs, dense)
//
//   pool_cpp <in.bin> <scale> <radius> <spread> <min_disparity> <max_disparity> <out_prefix>
// in.bin: int32 {n, rows, cols, depth}, then the left and the right stack, planar and dense.
// One line per form on stdout: "<form> from_prior fallback". A window with min_disparity >
// max_disparity must throw: "exception: <message>" on stdout, exit status 5.
#include <bicos/common.hpp>
#include <bicos/pool.hpp>
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

static void dump(FILE* f, const Image& img) {
    const Image h = img.download();
    const size_t row = (size_t)h.cols() * h.elemSize();
    for (int r = 0; r < h.rows(); ++r)
        std::fwrite((const char*)h.data() + (size_t)r * h.step(), 1, row, f);
}

static void dump(const std::string& path, const std::vector<Image>& imgs) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) std::exit(4);
    for (const Image& im : imgs) dump(f, im);
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: see header\n");
        return 2;
    }
    try {
        PyramidParams pp;
        pp.scale = std::atoi(argv[2]);
        pp.radius = std::atoi(argv[3]);
        pp.spread = std::atoi(argv[4]);
        const int dmin = std::atoi(argv[5]), dmax = std::atoi(argv[6]);
        const std::string out = argv[7];

        FILE* f = std::fopen(argv[1], "rb");
        int32_t hdr[4];
        if (!f || std::fread(hdr, sizeof hdr, 1, f) != 1) return 2;
        const int n = hdr[0], rows = hdr[1], cols = hdr[2], depth = hdr[3];
        const int type = depth == 2 ? U16 : U8;
        const size_t plane = (size_t)rows * cols * depth;
        std::vector<unsigned char> stacks(2 * n * plane);
        if (std::fread(stacks.data(), 1, stacks.size(), f) != stacks.size()) return 2;
        std::fclose(f);

        void* dstacks = nullptr;
        hip_ok(hipMalloc(&dstacks, stacks.size()), "hipMalloc");
        hip_ok(hipMemcpy(dstacks, stacks.data(), stacks.size(), hipMemcpyHostToDevice), "upload");
        void* dcounts = nullptr;
        hip_ok(hipMalloc(&dcounts, 8), "hipMalloc");

        Config cfg;
        cfg.nxcorr_threshold = 0.9f;
        cfg.disparity_range = DisparityRange{dmin, dmax};

        const struct {
            const char* name;
            unsigned char* base;
            Memory mem;
        } forms[] = {{"host", stacks.data(), Memory::Host},
                     {"dev", (unsigned char*)dstacks, Memory::Device}};
        for (const auto& fm : forms) {
            std::vector<Image> s0, s1;
            for (int t = 0; t < n; ++t) {
                s0.emplace_back(rows, cols, type, fm.base + (size_t)t * plane, 0, fm.mem);
                s1.emplace_back(rows, cols, type, fm.base + (size_t)(n + t) * plane, 0, fm.mem);
            }
            std::vector<Image> pooled;
            pool_stack(s0, pp.scale, pooled);
            if (fm.mem == Memory::Device) hip_ok(hipDeviceSynchronize(), "sync");
            if ((int)pooled.size() != n || pooled[0].rows() != rows / pp.scale ||
                pooled[0].cols() != cols / pp.scale || pooled[0].type() != type ||
                pooled[0].memory() != fm.mem)
                return 5;
            // a fresh device out_stack is one planar buffer (the one-launch path)
            if (fm.mem == Memory::Device)
                for (int t = 1; t < n; ++t)
                    if ((const char*)pooled[t].data() !=
                        (const char*)pooled[0].data() + (size_t)t * pooled[0].rows() * pooled[0].step())
                        return 7;
            dump(out + "." + fm.name + ".pool", pooled);

            Image disp, corr, coarse, guide;
            uint32_t c[2] = {0, 0};
            try {
                match_pyramid(s0, s1, disp, cfg, pp, &corr, &coarse, &guide,
                              fm.mem == Memory::Host ? c : (uint32_t*)dcounts);
            } catch (const Exception& e) {
                std::printf("exception: %s\n", e.what());
                return 5;
            }
            if (fm.mem == Memory::Device) {
                hip_ok(hipDeviceSynchronize(), "sync");
                hip_ok(hipMemcpy(c, dcounts, sizeof c, hipMemcpyDeviceToHost), "download");
            }
            if (disp.memory() != fm.mem || disp.type() != F32 || corr.type() != F32 ||
                coarse.type() != F32 || coarse.rows() != rows / pp.scale ||
                coarse.cols() != cols / pp.scale || guide.type() != S16 || guide.rows() != rows ||
                guide.cols() != 2 * cols)
                return 5;
            std::printf("%s %u %u\n", fm.name, c[0], c[1]);
            dump(out + "." + fm.name + ".disp", {disp});
            dump(out + "." + fm.name + ".corr", {corr});
            dump(out + "." + fm.name + ".coarse", {coarse});
            dump(out + "." + fm.name + ".guide", {guide});
        }

        // errors are BICOS::Exception
        std::vector<Image> s0, s1;
        for (int t = 0; t < n; ++t) {
            s0.emplace_back(rows, cols, type, stacks.data() + (size_t)t * plane, 0, Memory::Host);
            s1.emplace_back(rows, cols, type, stacks.data() + (size_t)(n + t) * plane, 0,
                            Memory::Host);
        }
        try {
            std::vector<Image> p;
            pool_stack(s0, 9, p);
            return 6;
        } catch (const Exception&) {
        }
        try {  // no global window
            Image d;
            match_pyramid(s0, s1, d, Config{}, pp);
            return 6;
        } catch (const Exception&) {
        }
        try {
            PyramidParams bad = pp;
            bad.spread = 8;
            Image d;
            match_pyramid(s0, s1, d, cfg, bad);
            return 6;
        } catch (const Exception&) {
        }
        hip_ok(hipFree(dcounts), "hipFree");
        hip_ok(hipFree(dstacks), "hipFree");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
