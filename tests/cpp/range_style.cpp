// range_style.cpp -- TEST PROGRAM (tests/test_range_gpu.py): a C++ caller that sets
// BICOS::Config::disparity_range and runs BICOS::match twice on the same host stacks -- the
// cv::Mat overload (<BICOS/match.hpp>, cv::Mat from tests/cpp/cvmat_double) and the native
// HipImage overload (<bicos/match.hpp>) -- built against the installed tree like
// ref_style.cpp (tests/cpp/range_consumer/CMakeLists.txt).
//
//   range_style <in.bin> <out_prefix> <nxcorr|-1> <subpixel|-1> <minvar|-1> <consistency 0/1>
//               <max_lr_diff> <no_dupes> <min_disparity> <max_disparity>
// in.bin: int32 n, rows, cols, depth, then stack0 and stack1 as dense planes (match_cpp's
// format). Writes <out_prefix>.{mat,native}.disp / .corr and one summary line. A range
// with min > max must throw BICOS::Exception: printed as "exception: ...", exit code 5.
#include <BICOS/match.hpp>
#include <bicos/match.hpp>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static void dump(const std::string& path, const void* data, size_t step, int rows) {
    FILE* o = std::fopen(path.c_str(), "wb");
    if (!o) std::exit(4);
    std::fwrite(data, step, rows, o);
    std::fclose(o);
}

int main(int argc, char** argv) {
    if (argc != 11) {
        std::fprintf(stderr, "usage: range_style in.bin out_prefix nxcorr subpix minvar "
                             "consistency max_lr_diff no_dupes min_disparity max_disparity\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    int hdr[4];
    if (!f || std::fread(hdr, sizeof(int), 4, f) != 4) return 2;
    const int n = hdr[0], rows = hdr[1], cols = hdr[2], depth = hdr[3];
    const int type = depth == 1 ? CV_8UC1 : CV_16UC1;
    std::vector<cv::Mat> stack0, stack1;
    for (int s = 0; s < 2; ++s)
        for (int t = 0; t < n; ++t) {
            cv::Mat m(rows, cols, type);
            if (std::fread(m.data, (size_t)depth * cols, rows, f) != (size_t)rows) return 2;
            (s ? stack1 : stack0).push_back(m);
        }
    std::fclose(f);

    BICOS::Config cfg;
    const float nxc = std::atof(argv[3]), sp = std::atof(argv[4]), mv = std::atof(argv[5]);
    cfg.nxcorr_threshold = nxc < 0 ? std::nullopt : std::optional<float>(nxc);
    if (sp > 0) cfg.subpixel_step = sp;
    if (mv >= 0) cfg.min_variance = mv;
    if (std::atoi(argv[6]))
        cfg.variant = BICOS::Variant::Consistency{std::atoi(argv[7]), std::atoi(argv[8]) != 0};
    cfg.disparity_range = BICOS::DisparityRange{std::atoi(argv[9]), std::atoi(argv[10])};

    const std::string out = argv[2];
    try {
        cv::Mat disparity, corrmap;
        BICOS::match(stack0, stack1, disparity, cfg, &corrmap);
        dump(out + ".mat.disp", disparity.data, disparity.step[0], disparity.rows);
        if (!corrmap.empty()) dump(out + ".mat.corr", corrmap.data, corrmap.step[0], corrmap.rows);

        std::vector<BICOS::HipImage> h0, h1;
        for (const cv::Mat& m : stack0) h0.push_back(BICOS::image_view(m));
        for (const cv::Mat& m : stack1) h1.push_back(BICOS::image_view(m));
        BICOS::HipImage d, c;
        BICOS::match(h0, h1, d, cfg, &c);
        dump(out + ".native.disp", d.data(), d.step(), d.rows());
        if (!c.empty()) dump(out + ".native.corr", c.data(), c.step(), c.rows());
        std::printf("range_style type=%d corr=%d\n", disparity.type(), corrmap.empty() ? 0 : 1);
    } catch (const BICOS::Exception& e) {
        std::printf("exception: %s\n", e.what());
        return 5;
    }
    return 0;
}
