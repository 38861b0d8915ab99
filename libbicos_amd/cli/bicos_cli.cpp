// bicos-cli -- the reference's command-line front end (reference src/cli.cpp:55-253) on the
// gfx950 engine, without OpenCV, cxxopts or fmt: a folder of numbered images in (PNG or
// binary PGM), the disparity out as a colourised PNG plus the raw map as TIFF, optionally
// the correlation map and a point cloud (.xyz) through a stereo Q matrix.
//
//   bicos-cli folder0 [folder1] [-t 0.75] [-v VAR] [-s STEP] [-o bicosdisp.png] [-n N]
//             [-q Q.yml] [--allow-negative-z] [-m MAXDIFF] [--double] [--limited]
//             [--corrmap] [--no-dupes] [-h]
// and, beyond the reference: --speckle-size / --speckle-diff, --median / --median-fill,
// --rectify, --normals / --normals-diff / --normals-min, --mesh / --mesh-diff, --texture /
// --texture-camera / --texture-tol / --texture-splat (see USAGE below).
//
// Same options, defaults and semantics as the reference (FULL transform unless --limited;
// --threshold <= 0 disables the NXC filter; --corrmap without a threshold computes with
// threshold -1; the variance filter only when -v is given and > 0; --lr-maxdiff selects
// the Consistency variant, --no-dupes then adds duplicate rejection). Divergence: the
// reference declares --allow-negative-z but reads "allow-behind" (cli.cpp:233), so its flag
// never takes effect; here it does.
#include <bicos/common.hpp>
#include <bicos/match.hpp>
#include <bicos_c.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <iostream>
#include <limits>
#include <map>
#include <optional>
#include <string>
#include <unistd.h>
#include <vector>

#include "imageio.hpp"

using namespace BICOS;
namespace fs = std::filesystem;

namespace {

const char* USAGE =
    "bicos-cli: process multi-shot stereo images with BICOS (libbicos_amd, gfx950)\n"
    "usage: bicos-cli folder0 [folder1] [options]\n"
    "  folder0                 first folder with numbered input images\n"
    "  folder1                 optional second folder; then names are 0.png, 1.png...\n"
    "                          else folder0 holds 0_left.png, 0_right.png, 1_left.png...\n"
    "  -t, --threshold F       minimum normalized cross correlation of a match (0.75;\n"
    "                          0.0 disables)\n"
    "  -v, --variance F        minimum intensity variance (only with --threshold)\n"
    "  -s, --step F            subpixel interpolation step (only with --threshold)\n"
    "  -o, --out FILE          output file for the disparity image (bicosdisp.png)\n"
    "  -n, --stacksize N       number of images to process (default: all found)\n"
    "  -q, --qmatrix FILE      OpenCV FileStorage (YAML/XML) with a 4x4 matrix \"Q\":\n"
    "                          also write a point cloud (.xyz)\n"
    "      --allow-negative-z  keep points with negative Z in the point cloud\n"
    "      --speckle-size N    speckle filter: invalidate every 4-connected region of similar\n"
    "                          disparity with at most N pixels, before the disparity is\n"
    "                          saved and reprojected (default: off)\n"
    "      --speckle-diff F    largest disparity difference of two neighbours in one region\n"
    "                          (1; only with --speckle-size)\n"
    "      --median K          median filter: K x K (3 or 5) median over the valid disparities\n"
    "                          of each pixel's window, after --speckle-size and before the\n"
    "                          disparity is saved and reprojected (default: off)\n"
    "      --median-fill M     also fill an invalid pixel whose window holds at least M valid\n"
    "                          disparities (K*K/2 + 1: only surrounded holes; 0: none; only\n"
    "                          with --median)\n"
    "      --normals R         with a Q matrix: also estimate a unit surface normal per point,\n"
    "                          towards the camera, from the plane fitted to the disparities of\n"
    "                          the (2R+1) x (2R+1) window (R in 1..4); each .xyz line becomes\n"
    "                          X Y Z NX NY NZ, with 0 0 0 where a point has no normal. Meant\n"
    "                          for subpixel maps (--step): integer disparities stair-step\n"
    "      --normals-diff F    a window pixel takes part if its disparity lies within F of the\n"
    "                          centre's (1; only with --normals)\n"
    "      --normals-min M     least number of window pixels for a normal (3; only with\n"
    "                          --normals)\n"
    "      --mesh              with a Q matrix: also triangulate the disparity map and write\n"
    "                          <out>.ply beside the .xyz (binary little-endian): its vertices\n"
    "                          are the .xyz points, and every 2x2 block of pixels gives at most\n"
    "                          two triangles\n"
    "      --mesh-diff F       a triangle's edge may join disparities that differ by at most F\n"
    "                          (1; only with --mesh)\n"
    "      --texture IMAGE     with --mesh: colour every vertex with the grey value that IMAGE\n"
    "                          (PNG or PGM, the picture of the camera of --texture-camera) has\n"
    "                          where the vertex projects to; the .ply gains red, green and blue\n"
    "                          per vertex, 0 for a vertex that camera does not see\n"
    "      --texture-camera FILE  OpenCV FileStorage (YAML/XML) with the 3x3 \"K\" of that camera\n"
    "                          and optionally \"D\" (0, 4, 5 or 8 coefficients), \"R\" (3x3) and\n"
    "                          \"T\" (3 values) from the rectified left camera to it; for the\n"
    "                          rectified left camera itself K is the left 3x3 of P1\n"
    "      --texture-tol F     also test occlusion: a vertex is not seen where a nearer one lies\n"
    "                          more than F in depth in front of it on its pixel (default: no\n"
    "                          test)\n"
    "      --texture-splat S   each vertex covers (2S+1) x (2S+1) pixels in that test (1; 0..3;\n"
    "                          only with --texture-tol)\n"
    "      --rectify FILE      the inputs are raw frames: OpenCV FileStorage (YAML/XML) with\n"
    "                          the matrices M1 D1 R1 P1 M2 D2 R2 P2 of cv::stereoRectify;\n"
    "                          both stacks are rectified to their own size before the match.\n"
    "                          A \"Q\" in FILE is used when -q is not given\n"
    "  -m, --lr-maxdiff N      maximum left-right disparity difference (Consistency\n"
    "                          variant; disables duplicate filtering)\n"
    "      --double            double precision correlation\n"
    "      --limited           LIMITED transform mode (allows more images)\n"
    "      --corrmap           also write the map of correlation values\n"
    "      --no-dupes          duplicate filtering (the default without --lr-maxdiff)\n"
    "  -h, --help              this message\n";

struct Args {
    std::vector<std::string> pos;
    std::map<std::string, std::string> val;  // option -> value ("" for flags)
    bool has(const std::string& k) const { return val.count(k) != 0; }
};

Args parse(int argc, char** argv) {
    static const std::map<std::string, std::string> shorts = {
        {"t", "threshold"}, {"v", "variance"}, {"s", "step"}, {"o", "out"},
        {"n", "stacksize"}, {"q", "qmatrix"}, {"m", "lr-maxdiff"}, {"h", "help"}};
    static const std::map<std::string, bool> takes = {
        {"threshold", true}, {"variance", true}, {"step", true}, {"out", true},
        {"stacksize", true}, {"qmatrix", true}, {"lr-maxdiff", true}, {"help", false},
        {"allow-negative-z", false}, {"double", false}, {"limited", false},
        {"corrmap", false}, {"no-dupes", false}, {"speckle-size", true}, {"speckle-diff", true},
        {"rectify", true}, {"median", true}, {"median-fill", true}, {"normals", true},
        {"normals-diff", true}, {"normals-min", true}, {"mesh", false}, {"mesh-diff", true},
        {"texture", true}, {"texture-camera", true}, {"texture-tol", true},
        {"texture-splat", true}};
    Args a;
    for (int i = 1; i < argc; ++i) {
        std::string s = argv[i];
        if (s.size() < 2 || s[0] != '-') {
            a.pos.push_back(s);
            continue;
        }
        std::string name, value;
        bool inline_value = false;
        if (s[1] == '-') {
            name = s.substr(2);
            const size_t eq = name.find('=');
            if (eq != std::string::npos) {
                value = name.substr(eq + 1);
                name = name.substr(0, eq);
                inline_value = true;
            }
        } else {
            const auto it = shorts.find(s.substr(1, 1));
            if (it == shorts.end()) throw std::invalid_argument("unknown option " + s);
            name = it->second;
            if (s.size() > 2) value = s.substr(2), inline_value = true;
        }
        const auto t = takes.find(name);
        if (t == takes.end()) throw std::invalid_argument("unknown option --" + name);
        if (t->second && !inline_value) {
            if (i + 1 >= argc) throw std::invalid_argument("option --" + name + " needs a value");
            value = argv[++i];
        }
        a.val[name] = value;
    }
    return a;
}

float as_float(const Args& a, const std::string& k) {
    size_t used = 0;
    const float v = std::stof(a.val.at(k), &used);
    if (used != a.val.at(k).size()) throw std::invalid_argument("--" + k + ": not a number");
    return v;
}

unsigned as_uint(const Args& a, const std::string& k) {
    const std::string& s = a.val.at(k);
    if (s.empty() || s.find_first_not_of("0123456789") != std::string::npos)
        throw std::invalid_argument("--" + k + ": not an unsigned integer");
    return (unsigned)std::stoul(s);
}

double ms_since(std::chrono::high_resolution_clock::time_point t) {
    return std::chrono::duration_cast<std::chrono::microseconds>(
               std::chrono::high_resolution_clock::now() - t).count() / 1000.0;
}

// reference save_image (src/fileutils.cpp:30-58): colourised PNG and raw TIFF
void save_image(const Image& img, fs::path out, bicos_cli::Colormap cmap) {
    const std::vector<uint8_t> rgb = bicos_cli::colorize(img, cmap);
    bicos_cli::write_png_rgb(out.replace_extension("png").string(), img.rows(), img.cols(), rgb);
    std::cout << "Saved colorized disparity to\t\t" << out << std::endl;
    bicos_cli::write_tiff(out.replace_extension("tiff").string(), img);
    std::cout << "Saved floating-point disparity to\t" << out << std::endl;
}

// --rectify: the images of one camera (side "1" or "2": M, D, R, P of that name in `file`, as
// OpenCV's stereo calibration sample writes them) remapped in place to their own size
void rectify_stack(const std::string& file, const std::string& side, std::vector<bicos_cli::Gray>& stack) {
    const std::vector<double> M = bicos_cli::read_filestorage_matrix(file, "M" + side, 3, 3);
    const std::vector<double> R = bicos_cli::read_filestorage_matrix(file, "R" + side, 3, 3);
    const auto D = bicos_cli::find_filestorage_matrix(file, "D" + side);
    const auto P = bicos_cli::find_filestorage_matrix(file, "P" + side);
    if (!D) throw std::runtime_error(file + ": no matrix \"D" + side + "\"");
    if (!P || P->rows != 3) throw std::runtime_error(file + ": no 3-row matrix \"P" + side + "\"");
    const int rows = stack.front().rows, cols = stack.front().cols, type = stack.front().type;
    const size_t pixels = (size_t)rows * cols;
    std::vector<float> map_x(pixels), map_y(pixels);
    if (bicos_rectify_maps_host(M.data(), D->data.empty() ? nullptr : D->data.data(),
                                (int)D->data.size(), R.data(), P->data.data(), P->cols, rows, cols,
                                map_x.data(), map_y.data()) != BICOS_OK)
        throw std::runtime_error(std::string("rectification maps failed: ") + bicos_last_error());
    std::vector<bicos_cli::Gray> out(stack.size());
    std::vector<const void*> src;
    std::vector<void*> dst;
    for (size_t t = 0; t < stack.size(); ++t) {
        if (stack[t].rows != rows || stack[t].cols != cols || stack[t].type != type)
            throw std::runtime_error("--rectify: all images must share size and type");
        out[t].rows = rows;
        out[t].cols = cols;
        out[t].type = type;
        out[t].pixels.resize(stack[t].pixels.size());
        src.push_back(stack[t].pixels.data());
        dst.push_back(out[t].pixels.data());
    }
    if (bicos_rectify_host(nullptr, src.data(), (int)stack.size(), rows, cols, 0, type == U16 ? 2 : 1,
                           map_x.data(), map_y.data(), 0, rows, cols, dst.data(), 0, 0,
                           nullptr) != BICOS_OK)
        throw std::runtime_error(std::string("rectification failed: ") + bicos_last_error());
    stack.swap(out);
}

// --texture: one grey value per vertex from the picture of another camera (K, D, R, T in `file`),
// on the GPU (bicos_project_host), as the rgb triples of write_ply_colored
std::vector<uint8_t> texture_vertices(const Args& args, const float* points, size_t count) {
    const std::string file = args.val.at("texture-camera");
    if (!fs::exists(file)) throw std::invalid_argument("'" + file + "' does not exist");
    bicos_cli::Gray img = bicos_cli::read_gray(args.val.at("texture"), false);
    const std::vector<double> K = bicos_cli::read_filestorage_matrix(file, "K", 3, 3);
    const auto D = bicos_cli::find_filestorage_matrix(file, "D");
    const auto R = bicos_cli::find_filestorage_matrix(file, "R");
    const auto T = bicos_cli::find_filestorage_matrix(file, "T");
    if (R && (R->rows != 3 || R->cols != 3)) throw std::runtime_error(file + ": \"R\" is not 3x3");
    if (T && T->data.size() != 3) throw std::runtime_error(file + ": \"T\" has not 3 values");
    const bool test = args.has("texture-tol");
    const float tol = test ? as_float(args, "texture-tol") : std::numeric_limits<float>::infinity();
    const unsigned splat = args.has("texture-splat") ? as_uint(args, "texture-splat") : 1u;
    if (splat > BICOS_PROJECT_MAX_SPLAT) throw std::invalid_argument("--texture-splat: S must lie in 0 .. 3");
    if (!test && args.has("texture-splat"))
        std::cerr << "'texture-splat' has no effect without 'texture-tol'.\n";
    std::vector<uint8_t> grey(count + 1);
    uint32_t counts[5] = {0, 0, 0, 0, 0};  // visible, occluded, outside, behind, invalid
    if (bicos_project_host(nullptr, points, count, R ? R->data.data() : nullptr,
                           T ? T->data.data() : nullptr, K.data(),
                           D && !D->data.empty() ? D->data.data() : nullptr,
                           D ? (int)D->data.size() : 0, img.rows, img.cols, (int)splat, tol,
                           img.pixels.data(), 1, 1, (size_t)img.cols, 0, nullptr, nullptr, nullptr,
                           grey.data(), nullptr, nullptr, counts) != BICOS_OK)
        throw std::runtime_error(std::string("texture failed: ") + bicos_last_error());
    std::cout << "Texture:\t" << counts[0] << " vertices seen, " << counts[1] << " occluded, "
              << counts[2] + counts[3] << " out of view" << std::endl;
    std::vector<uint8_t> rgb(3 * count + 1);
    for (size_t i = 0; i < count; ++i) rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = grey[i];
    return rgb;
}

int run(int argc, char** argv) {
    const Args args = parse(argc, argv);
    if (args.has("help") || args.pos.empty()) {
        std::cout << USAGE;
        return args.has("help") ? 0 : 2;
    }
    if (args.pos.size() > 2) throw std::invalid_argument("at most two input folders");
    std::cout << "bicos-cli (libbicos_amd: BICOS on the MI355X)\n" << std::endl;
    if (!isatty(STDOUT_FILENO)) std::cerr << "Danger: bicos-cli does not have a stable CLI interface\n";
    if (args.has("no-dupes") && !args.has("lr-maxdiff"))
        std::cerr << "'no-dupes' is the default when 'lr-maxdiff' is not set.\n";

    if (args.has("texture") != args.has("texture-camera"))
        throw std::invalid_argument("--texture and --texture-camera go together");
    if (args.has("texture") && !fs::exists(args.val.at("texture")))
        throw std::invalid_argument("'" + args.val.at("texture") + "' does not exist");

    const std::string folder0 = args.pos[0];
    const fs::path outfile = args.has("out") ? args.val.at("out") : "bicosdisp.png";
    std::optional<std::string> folder1;
    if (args.pos.size() == 2) folder1 = args.pos[1];
    std::optional<std::string> q_store;
    if (args.has("qmatrix")) {
        q_store = args.val.at("qmatrix");
        if (!fs::exists(*q_store)) throw std::invalid_argument("'" + *q_store + "' does not exist");
    }

    std::vector<bicos_cli::Gray> left, right;
    bicos_cli::read_stacks(folder0, folder1, left, right);
    if (args.has("stacksize")) {
        const unsigned n = as_uint(args, "stacksize");
        if (n < left.size()) {
            left.resize(n);
            right.resize(n);
        }
    }
    if (left.empty()) throw std::invalid_argument("no input images");
    std::cout << "Loaded " << left.size() + right.size() << " "
              << (left.front().type == U16 ? 16 : 8) << "-bit images in total" << std::endl;

    if (args.has("rectify")) {
        // raw frames: both stacks through their camera's maps, on the GPU, to the input size
        const std::string file = args.val.at("rectify");
        if (!fs::exists(file)) throw std::invalid_argument("'" + file + "' does not exist");
        const auto tick = std::chrono::high_resolution_clock::now();
        rectify_stack(file, "1", left);
        rectify_stack(file, "2", right);
        std::cout << "Rectified:\t" << ms_since(tick) << "ms" << std::endl;
        if (!q_store && bicos_cli::find_filestorage_matrix(file, "Q")) q_store = file;
    }

    Config c;
    c.nxcorr_threshold = args.has("threshold") ? as_float(args, "threshold") : 0.75f;
    c.mode = TransformMode::FULL;
    if (*c.nxcorr_threshold <= 0.0f) c.nxcorr_threshold = std::nullopt;
    const bool need_corrmap = args.has("corrmap");
    if (need_corrmap && !c.nxcorr_threshold) {
        c.nxcorr_threshold = -1.0f;
        std::cerr << "Computing with nxcorr-threshold of -1 because 'corrmap' is set\n";
    }
    if (args.has("step")) c.subpixel_step = as_float(args, "step");
    if (args.has("limited")) c.mode = TransformMode::LIMITED;
    if (args.has("variance"))
        if (const float mv = as_float(args, "variance"); mv > 0.0f) c.min_variance = mv;
    if (args.has("double")) c.precision = Precision::DOUBLE;
    if (args.has("lr-maxdiff"))
        c.variant = Variant::Consistency{(int)as_uint(args, "lr-maxdiff"), args.has("no-dupes")};

    std::vector<Image> s0, s1;
    for (auto& g : left) s0.push_back(g.view());
    for (auto& g : right) s1.push_back(g.view());
    Image disp, corrmap;
    const auto tick = std::chrono::high_resolution_clock::now();
    BICOS::match(s0, s1, disp, c, need_corrmap ? &corrmap : nullptr);
    std::cout << "Latency:\t" << ms_since(tick) << "ms" << std::endl;

    if (args.has("speckle-size")) {
        // on the GPU, in place; the flags are those of the reprojection call below (a float
        // -32768.0 is a number like any other); the corrmap is left alone
        const unsigned max_size = as_uint(args, "speckle-size");
        if (max_size > (unsigned)INT32_MAX) throw std::invalid_argument("--speckle-size: too large");
        const float max_diff = args.has("speckle-diff") ? as_float(args, "speckle-diff") : 1.0f;
        uint32_t counts[4] = {0, 0, 0, 0};  // kept, removed, invalid, removed_components
        if (bicos_speckle_host(nullptr, disp.data(), disp.type(), disp.rows(), disp.cols(),
                               (int)max_size, max_diff, 0, disp.data(), nullptr, counts) != BICOS_OK)
            throw std::runtime_error(std::string("speckle filter failed: ") + bicos_last_error());
        std::cout << "Speckle filter:\tremoved " << counts[1] << " pixels in " << counts[3]
                  << " regions" << std::endl;
    } else if (args.has("speckle-diff")) {
        std::cerr << "'speckle-diff' has no effect without 'speckle-size'.\n";
    }

    if (args.has("median")) {
        // on the GPU, after the speckle filter (islands are gone before anything can be filled
        // from them), with the flags of that call and of the reprojection below
        const unsigned ksize = as_uint(args, "median");
        const unsigned fill_min = args.has("median-fill") ? as_uint(args, "median-fill") : 0u;
        if (ksize != 3 && ksize != 5) throw std::invalid_argument("--median: K must be 3 or 5");
        if (fill_min > ksize * ksize)
            throw std::invalid_argument("--median-fill: M must lie in 0 .. K * K");
        uint32_t counts[4] = {0, 0, 0, 0};  // unchanged, changed, filled, invalid
        if (bicos_median_host(nullptr, disp.data(), disp.type(), disp.rows(), disp.cols(),
                              (int)ksize, (int)fill_min, 0, disp.data(), counts) != BICOS_OK)
            throw std::runtime_error(std::string("median filter failed: ") + bicos_last_error());
        std::cout << "Median filter:\tchanged " << counts[1] << " pixels, filled " << counts[2]
                  << std::endl;
    } else if (args.has("median-fill")) {
        std::cerr << "'median-fill' has no effect without 'median'.\n";
    }

    save_image(disp, outfile, bicos_cli::Colormap::Turbo);
    if (need_corrmap)
        save_image(corrmap,
                   outfile.parent_path() /
                       (outfile.stem().string() + "-corrmap" + outfile.extension().string()),
                   bicos_cli::Colormap::Viridis);

    if (q_store) {
        const auto Q = bicos_cli::read_filestorage_matrix(*q_store, "Q");
        fs::path xyz = outfile;
        xyz.replace_extension("xyz");
        // the points come from the GPU (bicos_reproject_host: bicos_cli::write_xyz's arithmetic
        // bit for bit); only the text is made here
        const size_t pixels = (size_t)disp.rows() * disp.cols();
        const bool with_normals = args.has("normals");
        std::vector<float> points(3 * pixels + 1);
        std::vector<int32_t> index(with_normals ? pixels + 1 : 0);
        uint32_t counts[4] = {0, 0, 0, 0};  // kept, invalid, nonfinite, negative_z
        const int flags = args.has("allow-negative-z") ? BICOS_REPROJECT_ALLOW_NEGATIVE_Z : 0;
        if (args.has("mesh")) {
            // the mesh's vertices are the reprojection's list (same flags: the two flag sets
            // share their values), so this one call gives the points, the index and the faces
            const float max_diff = args.has("mesh-diff") ? as_float(args, "mesh-diff") : 1.0f;
            const size_t quads = disp.rows() < 2 || disp.cols() < 2
                                     ? 0
                                     : (size_t)(disp.rows() - 1) * (disp.cols() - 1);
            std::vector<int32_t> triangles(3 * 2 * quads + 1);
            uint32_t mesh_counts[4] = {0, 0, 0, 0};  // triangles, quads with 2, 1, 0
            if (bicos_mesh_host(nullptr, disp.data(), disp.type(), disp.rows(), disp.cols(),
                                Q.data(), flags, max_diff, points.data(),
                                with_normals ? index.data() : nullptr, pixels, counts,
                                triangles.data(), 2 * quads, mesh_counts, nullptr) != BICOS_OK)
                throw std::runtime_error(std::string("mesh failed: ") + bicos_last_error());
            fs::path ply = outfile;
            ply.replace_extension("ply");
            if (args.has("texture")) {
                const std::vector<uint8_t> rgb = texture_vertices(args, points.data(), counts[0]);
                bicos_cli::write_ply_colored(ply.string(), points.data(), rgb.data(), counts[0],
                                             triangles.data(), mesh_counts[0]);
            } else {
                bicos_cli::write_ply(ply.string(), points.data(), counts[0], triangles.data(),
                                     mesh_counts[0]);
            }
            std::cout << "Saved mesh (" << counts[0] << " vertices, " << mesh_counts[0]
                      << " triangles) to\t" << ply << std::endl;
        } else if (bicos_reproject_host(nullptr, disp.data(), disp.type(), disp.rows(),
                                        disp.cols(), Q.data(), flags, nullptr, points.data(),
                                        with_normals ? index.data() : nullptr, pixels,
                                        counts) != BICOS_OK) {
            throw std::runtime_error(std::string("reprojection failed: ") + bicos_last_error());
        }
        if (with_normals) {
            // one normal per point of the list, on the same map with the same flags (the two
            // flag sets share their values)
            const unsigned radius = as_uint(args, "normals");
            const float max_diff = args.has("normals-diff") ? as_float(args, "normals-diff") : 1.0f;
            const unsigned min_points = args.has("normals-min") ? as_uint(args, "normals-min") : 3u;
            if (radius < 1 || radius > 4) throw std::invalid_argument("--normals: R must lie in 1 .. 4");
            if (min_points < 3 || min_points > (2 * radius + 1) * (2 * radius + 1))
                throw std::invalid_argument("--normals-min: M must lie in 3 .. (2R+1)^2");
            std::vector<float> normals(3 * pixels + 1);
            if (bicos_normals_host(nullptr, disp.data(), disp.type(), disp.rows(), disp.cols(),
                                   Q.data(), flags, (int)radius, max_diff, (int)min_points, nullptr,
                                   index.data(), counts[0], normals.data(), nullptr) != BICOS_OK)
                throw std::runtime_error(std::string("normals failed: ") + bicos_last_error());
            size_t have = 0;
            for (size_t i = 0; i < counts[0]; ++i) have += normals[3 * i] == normals[3 * i];
            bicos_cli::write_xyz_points_normals(xyz.string(), points.data(), normals.data(), counts[0]);
            std::cout << "Normals:\t" << have << " of " << counts[0] << " points" << std::endl;
        } else {
            bicos_cli::write_xyz_points(xyz.string(), points.data(), counts[0]);
        }
        std::cout << "Saved pointcloud in ascii-format to\t" << xyz << std::endl;
        if (counts[2]) std::cerr << "Skipped " << counts[2] << " points with non-finite fp values" << std::endl;
        if (counts[3]) std::cerr << "Skipped " << counts[3] << " points with negative Z values" << std::endl;
    }
    if (!q_store)
        for (const char* k : {"normals", "normals-diff", "normals-min", "mesh", "mesh-diff"})
            if (args.has(k)) std::cerr << "'" << k << "' has no effect without a Q matrix.\n";
    if (q_store && !args.has("normals"))
        for (const char* k : {"normals-diff", "normals-min"})
            if (args.has(k)) std::cerr << "'" << k << "' has no effect without 'normals'.\n";
    if (q_store && !args.has("mesh") && args.has("mesh-diff"))
        std::cerr << "'mesh-diff' has no effect without 'mesh'.\n";
    if (!(q_store && args.has("mesh")))
        for (const char* k : {"texture", "texture-tol", "texture-splat"})
            if (args.has(k)) std::cerr << "'" << k << "' has no effect without 'mesh'.\n";
    if (q_store && args.has("mesh") && !args.has("texture"))
        for (const char* k : {"texture-tol", "texture-splat"})
            if (args.has(k)) std::cerr << "'" << k << "' has no effect without 'texture'.\n";
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        return run(argc, argv);
    } catch (const std::exception& e) {
        std::cerr << "bicos-cli: " << e.what() << std::endl;
        return 1;
    }
}
