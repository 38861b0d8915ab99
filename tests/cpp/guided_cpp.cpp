// guided_cpp.cpp -- TEST PROGRAM (tests/test_guided_cpp.py, -m gpu): drives
// BICOS::guide_from_disparity (bicos/guide.hpp) and the guided BICOS::match overload
// (bicos/match.hpp) on the stacks and the prior map the Python test wrote, in host and in
// device memory, and writes the results for it to compare with its restatements:
//   <out>.host.guide / .dev.guide / .buf.guide   the guides (int16 pairs, dense)
//   <out>.host.disp / .dev.disp                  the guided disparity maps (float32)
//   <out>.host.corr / .dev.corr                  their corrmaps (float32)
//
//   guided_cpp <in.bin> <prior.raw> <prows> <pcols> <type 3|5> <radius> <spread> <scale>
//              <fallback_lo> <fallback_hi> <min_disparity> <max_disparity> <out_prefix>
// in.bin: int32 {n, rows, cols, depth}, then the left and the right stack, planar and dense.
// One line per guide on stdout: "<form> from_prior fallback". A window with min_disparity >
// max_disparity must throw: "exception: <message>" on stdout, exit status 5.
#include <bicos/common.hpp>
#include <bicos/guide.hpp>
#include <bicos/match.hpp>
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

static void dump(const std::string& path, const Image& img) {
    const Image h = img.download();
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) std::exit(4);
    const size_t row = (size_t)h.cols() * h.elemSize();
    for (int r = 0; r < h.rows(); ++r)
        std::fwrite((const char*)h.data() + (size_t)r * h.step(), 1, row, f);
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 14) {
        std::fprintf(stderr, "usage: see header\n");
        return 2;
    }
    try {
        const int prows = std::atoi(argv[3]), pcols = std::atoi(argv[4]), ptype = std::atoi(argv[5]);
        GuideParams gp;
        gp.radius = std::atoi(argv[6]);
        gp.spread = std::atoi(argv[7]);
        gp.scale = std::atoi(argv[8]);
        gp.fallback_lo = std::atoi(argv[9]);
        gp.fallback_hi = std::atoi(argv[10]);
        gp.flags = GUIDE_F32_SENTINEL;
        const int dmin = std::atoi(argv[11]), dmax = std::atoi(argv[12]);
        const std::string out = argv[13];

        FILE* f = std::fopen(argv[1], "rb");
        int32_t hdr[4];
        if (!f || std::fread(hdr, sizeof hdr, 1, f) != 1) return 2;
        const int n = hdr[0], rows = hdr[1], cols = hdr[2], depth = hdr[3];
        const int type = depth == 2 ? U16 : U8;
        const size_t plane = (size_t)rows * cols * depth;
        std::vector<unsigned char> stacks(2 * n * plane);
        if (std::fread(stacks.data(), 1, stacks.size(), f) != stacks.size()) return 2;
        std::fclose(f);
        const size_t pbytes = (size_t)prows * pcols * Image::elem_size(ptype);
        std::vector<unsigned char> praw(pbytes);
        f = std::fopen(argv[2], "rb");
        if (!f || std::fread(praw.data(), 1, pbytes, f) != pbytes) return 2;
        std::fclose(f);

        void* dstacks = nullptr;
        hip_ok(hipMalloc(&dstacks, stacks.size()), "hipMalloc");
        hip_ok(hipMemcpy(dstacks, stacks.data(), stacks.size(), hipMemcpyHostToDevice), "upload");
        const Image hprior(prows, pcols, ptype, praw.data(), 0, Memory::Host);
        Image dprior = Image::allocate(prows, pcols, ptype, Memory::Device);
        hip_ok(hipMemcpy(dprior.data(), praw.data(), pbytes, hipMemcpyHostToDevice), "upload");

        Config cfg;
        cfg.nxcorr_threshold = 0.9f;
        cfg.disparity_range = DisparityRange{dmin, dmax};

        const struct {
            const char* name;
            const Image* prior;
            unsigned char* base;
            Memory mem;
        } forms[] = {{"host", &hprior, stacks.data(), Memory::Host},
                     {"dev", &dprior, (unsigned char*)dstacks, Memory::Device}};
        for (const auto& fm : forms) {
            Image guide;
            const GuideStats s = guide_from_disparity(*fm.prior, guide, rows, cols, gp);
            if (guide.memory() != fm.mem || guide.rows() != rows || guide.cols() != 2 * cols ||
                guide.type() != S16)
                return 5;
            std::printf("%s %u %u\n", fm.name, s.from_prior, s.fallback);
            dump(out + "." + fm.name + ".guide", guide);

            std::vector<Image> s0, s1;
            for (int t = 0; t < n; ++t) {
                s0.emplace_back(rows, cols, type, fm.base + (size_t)t * plane, 0, fm.mem);
                s1.emplace_back(rows, cols, type, fm.base + (size_t)(n + t) * plane, 0, fm.mem);
            }
            Image disp, corr;
            try {
                match(s0, s1, guide, disp, cfg, &corr);
            } catch (const Exception& e) {
                std::printf("exception: %s\n", e.what());
                return 5;
            }
            if (fm.mem == Memory::Device) hip_ok(hipDeviceSynchronize(), "sync");
            if (disp.memory() != fm.mem || disp.type() != F32 || corr.type() != F32) return 5;
            dump(out + "." + fm.name + ".disp", disp);
            dump(out + "." + fm.name + ".corr", corr);
        }

        // the asynchronous builder on a stream of its own
        {
            void* buf = nullptr;
            hip_ok(hipMalloc(&buf, 8), "hipMalloc");
            hipStream_t st = nullptr;
            hip_ok(hipStreamCreate(&st), "hipStreamCreate");
            Image guide;
            guide_from_disparity(dprior, guide, rows, cols, gp, (uint32_t*)buf, st);
            hip_ok(hipStreamSynchronize(st), "sync");
            hip_ok(hipStreamDestroy(st), "hipStreamDestroy");
            uint32_t c[2];
            hip_ok(hipMemcpy(c, buf, sizeof c, hipMemcpyDeviceToHost), "download");
            hip_ok(hipFree(buf), "hipFree");
            std::printf("buf %u %u\n", c[0], c[1]);
            dump(out + ".buf.guide", guide);
        }

        // errors are BICOS::Exception
        try {
            const Image bad(prows, pcols, U8, praw.data(), 0, Memory::Host);
            Image g;
            guide_from_disparity(bad, g, rows, cols, gp);
            return 6;
        } catch (const Exception&) {
        }
        try {
            GuideParams p = gp;
            p.scale = 9;
            Image g;
            guide_from_disparity(hprior, g, rows, cols, p);
            return 6;
        } catch (const Exception&) {
        }
        try {  // a guide of the wrong shape
            std::vector<Image> s0, s1;
            for (int t = 0; t < n; ++t) {
                s0.emplace_back(rows, cols, type, stacks.data() + (size_t)t * plane, 0, Memory::Host);
                s1.emplace_back(rows, cols, type, stacks.data() + (size_t)(n + t) * plane, 0,
                                Memory::Host);
            }
            Image g = Image::allocate(rows, cols, S16, Memory::Host), d;
            match(s0, s1, g, d, cfg);
            return 6;
        } catch (const Exception&) {
        }
        hip_ok(hipFree(dstacks), "hipFree");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
