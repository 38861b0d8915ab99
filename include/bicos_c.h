/*
 * bicos_c.h -- C-ABI of libbicos_amd.so, the MI355X (gfx950) BICOS engine.
 *
 * Two layers, both plain C (pointers, sizes, ints; no C++ or torch types):
 *
 * 1. The reference's ctypes ABI, symbol for symbol (drop-in for pybicos_c.so):
 *      BicosConfig / BicosResult          reference src/pybicos_c.cpp:30-53
 *      BICOS_CreateDefaultConfig           reference src/pybicos_c.cpp:92-108
 *      BICOS_FreeConfig                    reference src/pybicos_c.cpp:111-113
 *      BICOS_FreeResult                    reference src/pybicos_c.cpp:116-118
 *      BICOS_Match                         reference src/pybicos_c.cpp:131-200
 *      BICOS_InvalidDisparityFloat/Int16   reference src/pybicos_c.cpp:203-209
 *    Host buffers in, malloc'd host copies out -- exactly the reference contract,
 *    with three documented fixes:
 *      - BicosConfig ALWAYS carries `precision` (the reference's Python wrapper,
 *        pybicos/__init__.py:41-51, always lays it out; the reference's CPU build
 *        omitted it and silently shifted the struct);
 *      - BICOS_FreeResult frees the data buffers too (the reference leaked them);
 *      - every exception is caught at the boundary (NULL result), not only
 *        BICOS::Exception; bicos_last_error() says why.
 *
 * 2. The device-resident hot path (bicos_hip_*): device pointers to planar image
 *    stacks already in HBM, results written to caller-provided device buffers,
 *    asynchronous on the caller's HIP stream. This is the entry point the
 *    reference's CUDA build exposes through BICOS::match(GpuMat...) with a
 *    cv::cuda::Stream (reference include/match.hpp:31-41, src/impl/cuda.cu:465-524),
 *    restated without OpenCV types.
 *
 * Error convention: int-returning functions return BICOS_OK (0) or a negative
 * BICOS_E_* code; bicos_last_error() returns a thread-local message.
 */
#ifndef BICOS_C_H
#define BICOS_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* OpenCV type codes used across the ABI (CV_MAKETYPE(depth, 1)) */
#define BICOS_CV_8U 0
#define BICOS_CV_16U 2
#define BICOS_CV_16S 3
#define BICOS_CV_32F 5
#define BICOS_CV_64F 6

/* reference src/pybicos_c.cpp:30-41 (with `precision` unconditionally present) */
typedef struct {
    float nxcorr_threshold; /* < 0: keep the default 0.5 (reference :59-61) */
    float subpixel_step;    /* < 0: no subpixel refinement */
    float min_variance;     /* < 0: no minimum variance */
    int mode;               /* 0 = LIMITED, 1 = FULL */
    int precision;          /* 0 = SINGLE, 1 = DOUBLE */
    int variant_type;       /* 0 = NoDuplicates, 1 = Consistency */
    int max_lr_diff;        /* Consistency only */
    int no_dupes;           /* Consistency only */
} BicosConfig;

/* reference src/pybicos_c.cpp:44-53 */
typedef struct {
    void* disparity_data;
    int disparity_rows;
    int disparity_cols;
    int disparity_type;
    void* corrmap_data;
    int corrmap_rows;
    int corrmap_cols;
    int corrmap_type;
} BicosResult;

BicosConfig* BICOS_CreateDefaultConfig(void);
void BICOS_FreeConfig(BicosConfig* config);
void BICOS_FreeResult(BicosResult* result);
BicosResult* BICOS_Match(void** stack0_data, int* stack0_rows, int* stack0_cols, int* stack0_types,
                         int stack0_size, void** stack1_data, int* stack1_rows, int* stack1_cols,
                         int* stack1_types, int stack1_size, BicosConfig* config);
float BICOS_InvalidDisparityFloat(void);
int16_t BICOS_InvalidDisparityInt16(void);

/* ------------------------------------------------------------------ errors */
enum {
    BICOS_OK = 0,
    BICOS_E_ARG = -1,       /* invalid argument (BICOS::Exception in the reference) */
    BICOS_E_BITS = -2,      /* stacks need > 256 descriptor bits (std::invalid_argument) */
    BICOS_E_HIP = -3,       /* HIP runtime error */
    BICOS_E_INTERNAL = -4
};
const char* bicos_last_error(void);

/* --------------------------------------------------- device-resident API */

/* Opaque per-device engine: owns a workspace (descriptor buffers, temporaries)
 * that grows on demand (stream-ordered: hipFreeAsync / hipMallocAsync on the calling
 * stream, never a device-wide synchronisation) and is reused across calls. Calls on one
 * handle from several host threads are serialised by the engine's lock; the GPU work of
 * calls on different streams is ordered through the engine's workspace event. */
typedef struct bicos_engine bicos_engine;

int bicos_engine_create(int device, bicos_engine** out);
/* The process-wide engine of `device` that BICOS_Match, bicos_match_host(NULL, ...) and
 * BICOS::match use (created on first use; bicos_engine_destroy ignores it). NULL on error. */
bicos_engine* bicos_engine_default(int device);
void bicos_engine_destroy(bicos_engine* e);

/* Search-kernel tuning for this engine (0 = automatic for each argument):
 *   variant        16 = the VALU search (packed 16-bit keys)
 *   col0_per_lane  left pixels held in registers per lane (2|4)
 *   waves          waves per workgroup (1..8)
 *   split          waves that share one col0 group and split its col1 scan (1|2|4|8)
 * Matrix-core search (search_mx.hip, the default): variant 64 (automatic keys), 65 (one FP4
 * product per pair + xor keys; rows <= 16384), 66 (two products: first / last minimum), 67
 * (xor keys for first-minimum searches too, instead of the float keys that carry the column
 * in a free K half);
 * col0_per_lane = 32-column tiles per wave (2|4|8; 8 falls back to 4 where the registers do
 * not fit), waves 1..8, split = LDS stage KiB (0 = 64).
 * Results are identical for every setting; only speed changes. */
int bicos_engine_tune(bicos_engine* e, int variant, int col0_per_lane, int waves, int split);

/* Descriptor width in 32-bit words for n images in `mode` (reference dispatch
 * src/impl/cpu.cpp:122-156); BICOS_E_BITS when more than 256 bits are needed. */
int bicos_descriptor_words(int n, int mode);

/* Output element type BICOS_Match / bicos_match_device produce for a config:
 * BICOS_CV_16S without a correlation threshold, else BICOS_CV_32F
 * (BICOS_CV_64F corrmap for precision DOUBLE). */
int bicos_output_type(const BicosConfig* cfg, int has_nxcorr);

/*
 * Full match on device-resident planar stacks.
 *   stack0/stack1 : n planes each; element (t, y, x) at
 *                   base[t*plane_pitch + y*row_pitch + x], u8 (depth 1) or u16 (depth 2).
 *                   Pitches are in ELEMENTS and may be anything >= a row / the rows of a plane;
 *                   the base needs only the element's own alignment (any byte for u8, 2 bytes
 *                   for u16): a region of interest cut out of a pitched frame is passed as it
 *                   lies. Bytes between rows, between planes and around the view are never
 *                   taken for pixels and never written. Alignment only selects kernels
 *                   (bicos_match_plan, bicos_agree_kernel), never results: every stage is
 *                   tested at every base residue and pitch residue mod 4
 *                   (tests/test_stack_views_gpu.py).
 *   has_nxcorr    : 0 disables the NXC stage (Config::nxcorr_threshold = nullopt, only
 *                   reachable from C++ in the reference); disparity is then int16
 *   disparity     : device, rows*cols dense, int16 or float32 per bicos_output_type
 *   corrmap       : device, rows*cols dense float32 (float64 for DOUBLE), or NULL
 *   stream        : hipStream_t (NULL = default stream); the call only enqueues work
 */
int bicos_match_device(bicos_engine* e, const void* stack0, const void* stack1, int n, int rows,
                       int cols, size_t row_pitch, size_t plane_pitch, int depth,
                       const BicosConfig* cfg, int has_nxcorr, void* disparity, void* corrmap,
                       void* stream);

/*
 * bicos_match_device with the disparity map always int16, also with the NXC stage: the
 * integer disparity, -32768 where invalid or below the threshold, so that
 * (float)disparity is exactly the float32 map bicos_match_device writes (the reference's
 * float map is the int16 one converted, src/impl/cpu.cpp:77-95). Half the bytes of the
 * float map -- what a row band ships to the gathering GPU (bench.py). A subpixel config
 * is rejected (BICOS_E_ARG): its disparities are not integers. No reference counterpart.
 */
int bicos_match_device_i16(bicos_engine* e, const void* stack0, const void* stack1, int n,
                           int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
                           const BicosConfig* cfg, int has_nxcorr, void* disparity, void* corrmap,
                           void* stream);

/*
 * Full match on host buffers (the reference's cv::Mat path; what BICOS_Match and
 * pybicos.match run). Synchronous.
 *   e             : engine, or NULL for the current device's default engine
 *   stack0/stack1 : n host image pointers each (any addresses), rows x cols, `step` bytes
 *                   per row (0 = dense), u8 (depth 1) or u16 (depth 2)
 *   disparity     : host, rows*cols dense, int16 or float32 per bicos_output_type
 *   corrmap       : host, rows*cols dense float32 (float64 for DOUBLE), or NULL
 * The stacks are uploaded in row bands through pinned staging on a copy stream while the
 * bands already uploaded are matched; the maps are written straight into the buffers.
 */
int bicos_match_host(bicos_engine* e, const void* const* stack0, const void* const* stack1, int n,
                     int rows, int cols, size_t step, int depth, const BicosConfig* cfg,
                     int has_nxcorr, void* disparity, void* corrmap);

/* ------------------------------------------------------- disparity range */
/* The search restricted to a disparity window (no reference counterpart; BicosConfig is the
 * reference's ctypes layout and does not grow, so the window is two extra arguments):
 * min_disparity <= max_disparity, inclusive, disparity = col0 - col1 (left column minus
 * right column, the sign of the maps). Any pair of ints with min <= max is legal, negative
 * values included; the window is clamped to the disparities a row holds, [-(cols-1), cols-1],
 * and one that no pixel can satisfy yields an all-invalid map, not an error. min > max is
 * BICOS_E_ARG, detected before any HIP call.
 *   candidates  of the left pixel col0: C(col0) = { col1 : 0 <= col1 < cols and
 *               min_disparity <= col0 - col1 <= max_disparity }
 *   search      the reference's bicos_search (include/impl/cpu/bicos.hpp:50-76) over C(col0)
 *               in ascending col1: the first minimum wins; NoDuplicates invalidates the
 *               pixel if the minimum cost occurs more than once WITHIN C(col0); an empty
 *               C(col0) gives an invalid pixel
 *   consistency the reverse search for col1 runs over { col0 : min_disparity <= col0 - col1
 *               <= max_disparity } in ascending col0 (the same search with the descriptor
 *               sets swapped and the window [-max_disparity, -min_disparity]); the
 *               max_lr_diff check and (col0 + reverse_col0) / 2 - best_col1 are unchanged
 *               (bicos.hpp:94-106)
 * The agree / subpixel / min-variance / corrmap stages consume the integer map as always. A
 * window covering [-(cols-1), cols-1] gives the unrestricted call's maps byte for byte.
 * These calls always run the windowed matrix-core search (search_range.hip) followed by
 * separate consistency / agree launches: BICOS_SEARCH=valu and the fused or compacted plans
 * of bicos_match_plan do not apply to them. Otherwise exactly their unranged twins. */
int bicos_match_device_range(bicos_engine* e, const void* stack0, const void* stack1, int n,
                             int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
                             const BicosConfig* cfg, int has_nxcorr, int min_disparity,
                             int max_disparity, void* disparity, void* corrmap, void* stream);
int bicos_match_host_range(bicos_engine* e, const void* const* stack0, const void* const* stack1,
                           int n, int rows, int cols, size_t step, int depth,
                           const BicosConfig* cfg, int has_nxcorr, int min_disparity,
                           int max_disparity, void* disparity, void* corrmap);

/* ------------------------------------------------ single-process multi-GPU */
/* One frame matched on several GPUs from one process (the reference has
 * no multi-GPU API -- these extend bicos_match_host / bicos_match_device, whose conventions
 * they keep). The frame's rows are split into contiguous bands, band b on devices[b] with
 * that device's default engine. Every stage of the match is row-local, so the maps are
 * byte-identical to the one-GPU call. devices may repeat (bands on one GPU then run one
 * after another on its engine). Both calls are synchronous. */

/* Host buffers, bicos_match_host's arguments: the rows are split into min(ndev, rows)
 * bands whose heights differ by at most one (the first rows % ndev bands get the extra
 * row); one host thread per band runs the banded upload -> match -> download pipeline of
 * its GPU over that GPU's own PCIe link and writes its rows of the maps straight into
 * `disparity` / `corrmap`. */
int bicos_match_host_multi(const int* devices, int ndev, const void* const* stack0,
                           const void* const* stack1, int n, int rows, int cols, size_t step,
                           int depth, const BicosConfig* cfg, int has_nxcorr, void* disparity,
                           void* corrmap);

/* Device-resident bands: band b (band_rows[b] rows, in frame order) lives on devices[b] as
 * planar stacks stack0[b] / stack1[b] with row_pitch[b] / plane_pitch[b] (elements, as in
 * bicos_match_device). Each GPU matches its band; the maps are gathered into `disparity` /
 * `corrmap` on devices[0] (dense, sum(band_rows) x cols; corrmap may be NULL) by peer
 * copies over xGMI -- band 0 is written in place. */
int bicos_match_bands_device(const int* devices, int ndev, const void* const* stack0,
                             const void* const* stack1, const int* band_rows,
                             const size_t* row_pitch, const size_t* plane_pitch, int n, int cols,
                             int depth, const BicosConfig* cfg, int has_nxcorr, void* disparity,
                             void* corrmap);

/* Stage entry points (tests, benchmarks, custom pipelines). Same conventions.
 * desc buffers: rows x desc_pitch uint32 with desc_pitch = bicos_desc_pitch(cols, words), dense.
 * Descriptors that are READ (the search entries, bicos_search_agree_device) need 4-byte
 * alignment only (they are uint32_t*); 16 bytes, which the engine's own buffers have, only
 * lets a few copies use wider loads. Results are the same at every word offset, and desc0 and
 * desc1 may differ in it (tests/test_desc_views_gpu.py). bicos_transform_device WRITES whole
 * 16-byte vectors: its desc must be 16-byte aligned. Output maps are dense and need their
 * element's alignment only (tested 2, 4 and 8 bytes past a 16-byte boundary). */
size_t bicos_desc_pitch(int cols, int words);
int bicos_transform_device(const void* stack, int n, int rows, int cols, size_t row_pitch,
                           size_t plane_pitch, int depth, int mode, int words, uint32_t* desc,
                           void* stream);
/* flags: 1 = NODUPES, 2 = CONSISTENCY (reference impl/common.hpp:46-47); out is int16 rows x
 * cols (dense). The engine may be NULL (the search is then planned for 256 compute units,
 * untuned) wherever the search needs no workspace: without CONSISTENCY, and for CONSISTENCY
 * without NODUPES in its one-launch form (BICOS_PLAN_CONSISTENCY_ONE_PASS: 256-bit
 * descriptors with 129..154 used bits given in B below, at most 2048 columns, the
 * matrix-core search, BICOS_LR_ONE_PASS not 0). Every other CONSISTENCY search runs as two
 * searches and a check and needs the engine's workspace for its two maps (NULL: BICOS_E_ARG).
 * flags bits 16-24 (optional): B = (flags >> 16) & 0x1FF, the number of low descriptor bits
 * that may be set (0 = all). The caller promises bits B..32*words-1 are zero in both
 * descriptor sets (true of transform output with B >= the transform's bit count: LIMITED
 * 4n-6, FULL n^2-2n+3); the matrix-core search then skips the 64-bit K-steps above B
 * (256-bit descriptors with B <= 192: 3 steps instead of 4). Results are unchanged.
 * 256-bit descriptors (words = 8): bit 255 is ignored (masked on both sides). Every
 * descriptor the transform produces leaves it zero -- LIMITED uses at most 4*65-6 = 254
 * bits, FULL at most 16*16-2*16+3 = 227 -- so results on transform output are exact; a
 * caller passing hand-made descriptors must keep bit 255 clear. */
int bicos_search_device(bicos_engine* e, const uint32_t* desc0, const uint32_t* desc1, int rows,
                        int cols, int words, int flags, int max_lr_diff, int16_t* out,
                        void* stream);
/* bicos_search_device over a disparity window (see "disparity range" above): the same flags,
 * the used-bits hint in bits 16-24 included. With flags & 2 it needs an engine for the two
 * maps (NULL: BICOS_E_ARG). */
int bicos_search_device_range(bicos_engine* e, const uint32_t* desc0, const uint32_t* desc1,
                              int rows, int cols, int words, int flags, int max_lr_diff,
                              int min_disparity, int max_disparity, int16_t* out, void* stream);
/* agree: raw int16 disparity -> float32 disparity (+ corrmap); minvar already x n */
int bicos_agree_device(const int16_t* raw, const void* stack0, const void* stack1, int n, int rows,
                       int cols, size_t row_pitch, size_t plane_pitch, int depth, float threshold,
                       int has_minvar, float minvar_scaled, float* out, float* corrmap,
                       void* stream);
int bicos_subpixel_device(const int16_t* raw, const void* stack0, const void* stack1, int n,
                          int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
                          float threshold, float step, int has_minvar, float minvar_scaled,
                          float* out, float* corrmap, void* stream);
/* agree (step <= 0) or subpixel (step > 0) in either precision: precision 1 = the CUDA
 * build's Precision::DOUBLE NXC (corrmap is then double*); the reference kernel-bench shapes
 * (bench/cuda.cu:99-180) time these with double precision. */
int bicos_agree_stage_device(const int16_t* raw, const void* stack0, const void* stack1, int n,
                             int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
                             float threshold, float step, int has_minvar, float minvar_scaled,
                             int precision, float* out, void* corrmap, void* stream);

/* What bicos_match_device runs for a shape and config past the descriptor transform
 * (tests, benchmarks): a mask of BICOS_PLAN_* bits, or a negative BICOS_E_* code for an
 * invalid configuration. stack0 / stack1 are only inspected for their alignment. No
 * reference counterpart (its kernels are fixed per build). */
#define BICOS_PLAN_MATRIX_CORES 1           /* the FP4 MFMA search (search_mx.hip) */
#define BICOS_PLAN_PACKED_KEYS 2            /* its packed-key form (search_pk_kernel) */
#define BICOS_PLAN_AGREE_IN_SEARCH 4        /* the NXC agree inside the search launch */
#define BICOS_PLAN_REVERSE_COMPACTED 8      /* Consistency: reverse search over kept col1 */
#define BICOS_PLAN_CONSISTENCY_IN_AGREE 16  /* Consistency: left-right check in the agree */
#define BICOS_PLAN_DENSE_ROWS 32            /* ... rows kept >= 7/8 skip the entry prologue */
#define BICOS_PLAN_CONSISTENCY_ONE_PASS 64  /* Consistency: both searches + the check, one launch */
int bicos_match_plan(bicos_engine* e, const void* stack0, const void* stack1, int n, int rows,
                     int cols, size_t row_pitch, size_t plane_pitch, int depth,
                     const BicosConfig* cfg, int has_nxcorr);
/* Whether the NoDuplicates search of rows x cols descriptors of `words` 32-bit words, `bits`
 * of them used (0: unknown, as bicos_search_device's flags), runs its main launch as the
 * pruned packed-key kernel (search_pkp_kernel) instead of the one-product one: 1 or 0.
 * fused != 0: the search inside the fused search + agree launch of stacks of n u8 images
 * (0 where that launch is not planned); else n is ignored. For tests; no HIP call, e may be
 * NULL. */
int bicos_search_packed(bicos_engine* e, int rows, int cols, int words, int bits, int n, int fused);
/* Which of its four matrix products (0-3, 32 bits each) the pruned packed-key search multiplies
 * bit `bit` (0-127: bit b % 32 of descriptor word b / 32) of a 128-bit descriptor in; -1 for any
 * other bit. Product 0 is what that search probes a block with, products 0 and 1 together are
 * words 0 and 1, products 2 and 3 are words 2 and 3. Results do not depend on the map. For tests
 * and tools; no HIP call. */
int bicos_search_packed_product(int bit);
/* Which kernel the agree stage (bicos_agree_device, bicos_agree_stage_device without a step, the
 * agree launch of a match) runs for these stacks: 2 = the left tile staged through LDS with
 * dword loads (stack0's base and both pitches, in bytes, multiples of 4; stack1's base is
 * free), 1 = every sample by byte / short loads into registers (any other view), 0 = the
 * generic kernel (n > 65, stage entries only). Results are identical. The pointers are only
 * inspected for their alignment. For tests; no HIP call. */
int bicos_agree_kernel(const void* stack0, const void* stack1, int n, size_t row_pitch,
                       size_t plane_pitch, int depth);
/* Which kernel the transform (bicos_transform_device with stack1 NULL, the transform launch of
 * a match over both stacks) runs for these stacks: 1 = two pixels per 32-bit register from
 * dword loads (u8 stacks, LIMITED, n one of 9 12 17 24 33 40 48 65 with words =
 * bicos_descriptor_words(n, 0), every base and both pitches multiples of 4 bytes, the stacks
 * within 256 MiB together, and the environment's BICOS_TRANSFORM_PK, read once, not 0),
 * 0 = one pixel per lane from byte / short loads (anything else). Results are identical. The
 * pointers are only inspected for their alignment. For tests; no HIP call. */
int bicos_transform_kernel(const void* stack0, const void* stack1, int n, int rows, int cols,
                           size_t row_pitch, size_t plane_pitch, int depth, int mode, int words);

/* bicos_match_device from its search on: desc0 / desc1 are the two stacks' descriptors as
 * bicos_transform_device writes them (rows x bicos_desc_pitch(cols, words) uint32, words =
 * bicos_descriptor_words(n, cfg->mode)); the stacks are still read by the agree / subpixel
 * stage. Exactly the launches the match issues after its transform (bicos_match_plan), so
 * benchmarks can time them in isolation; same outputs as bicos_match_device. */
int bicos_search_agree_device(bicos_engine* e, const uint32_t* desc0, const uint32_t* desc1,
                              const void* stack0, const void* stack1, int n, int rows, int cols,
                              size_t row_pitch, size_t plane_pitch, int depth,
                              const BicosConfig* cfg, int has_nxcorr, void* disparity,
                              void* corrmap, void* stream);

/* ---------------------------------------------------------- reprojection */
/* A dense rows x cols disparity map (BICOS_CV_16S or BICOS_CV_32F) through the rig's 4x4 matrix
 * Q (16 doubles, row-major) to 3-D points: what the reference's command-line tool does with
 * cv::reprojectImageTo3D and save_pointcloud (src/cli.cpp:238, include/fileutils.hpp:44-89).
 * For pixel (x = col, y = row) with d = (double)disparity, in IEEE double without contraction:
 *     o[i] = ((Q[4i]*x + Q[4i+1]*y) + Q[4i+2]*d) + Q[4i+3]      i = 0..3
 *     iw   = 1.0 / o[3]
 *     X, Y, Z = (float)(o[0]*iw), (float)(o[1]*iw), (float)(o[2]*iw)
 * Every pixel falls into exactly one class, tested in this order:
 *     invalid     int16 -32768; float NaN; with BICOS_REPROJECT_F32_SENTINEL also the float
 *                 -32768.0f (what a match with the NXC stage and no subpixel step writes for
 *                 a rejected pixel; without the flag it is reprojected like any number)
 *     nonfinite   X, Y or Z is not finite
 *     negative_z  Z < 0.0f, unless BICOS_REPROJECT_ALLOW_NEGATIVE_Z
 *     kept
 * Outputs, either alone or both:
 *     xyz_map  float32 [rows][cols][3]: the point where the pixel is kept, three NaNs elsewhere
 *     points   float32 [capacity][3]: the kept points in row-major pixel order (deterministic);
 *              index, optional, int32 [capacity]: each point's pixel row*cols + col;
 *              counts, uint32[4]: {kept, invalid, nonfinite, negative_z}, summing to rows*cols.
 *              With kept > capacity the first `capacity` points are written and nothing past
 *              them; counts[0] is still the full number. counts is written only with points.
 * rows*cols must fit int32. rows == 0 or cols == 0 is legal (counts all zero). Argument errors
 * (a type other than 16S / 32F, a negative size, too many pixels, no output, points without
 * counts, index without points, unknown flag bits, a NULL map or Q) are BICOS_E_ARG before any
 * HIP call. No reference counterpart in its library. */
#define BICOS_REPROJECT_ALLOW_NEGATIVE_Z 1
#define BICOS_REPROJECT_F32_SENTINEL 2
/* device: asynchronous on `stream`; xyz_map and points may each be NULL (not both);
 * index may be NULL; counts (device uint32[4]) is required with points. e is needed
 * for points (workspace); the dense map alone works with e == NULL. */
int bicos_reproject_device(bicos_engine* e, const void* disparity, int disp_type, int rows,
                           int cols, const double Q[16], int flags, float* xyz_map,
                           float* points, int32_t* index, size_t capacity, uint32_t* counts,
                           void* stream);
/* host buffers, synchronous, e NULL = default engine: uploads the map, runs the same
 * launches, downloads counts and then only the first min(kept, capacity) points. */
int bicos_reproject_host(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                         const double Q[16], int flags, float* xyz_map, float* points,
                         int32_t* index, size_t capacity, uint32_t counts[4]);
/* Pixels per segment of the point list's count / scan / write launches (tests). */
int bicos_reproject_segment(void);

/* -------------------------------------------------------- speckle filter */
/* Removes the small islands of disparities that disagree with their surroundings from a dense
 * rows x cols map (BICOS_CV_16S or BICOS_CV_32F), on the GPU. The reference has no such step.
 *     valid pixel  an int16 that is not -32768; a float that is not NaN and, with
 *                  BICOS_SPECKLE_F32_SENTINEL, not -32768.0f either (the notion of
 *                  BICOS_REPROJECT_F32_SENTINEL). Infinities are valid numbers.
 *     link         two 4-neighbours p, q are linked iff both are valid and
 *                      fabsf((float)d_p - (float)d_q) <= max_diff
 *                  with one IEEE float subtraction: exact for int16, symmetric, and false when
 *                  the difference is NaN (inf - inf).
 *     component    a connected component of the valid pixels under links. Its label is the
 *                  smallest linear index row*cols + col in it: canonical, independent of any
 *                  execution order.
 *     removal      a component with size <= max_size is removed: its pixels become int16
 *                  -32768, float NaN, or float -32768.0f under the sentinel flag (a sentinel
 *                  map stays one). Every other pixel, invalid ones included, is copied bit for
 *                  bit. max_size = 0 removes nothing.
 * max_diff must be >= 0 and not NaN; +inf is legal. max_size must not be negative.
 * Outputs:
 *     out     same type and shape as the map; may be the map itself (in place). Any other
 *             overlap of the two is an argument error.
 *     labels  optional, int32 [rows][cols]: the component label of every pixel that was valid
 *             on input, removed ones included, and -1 where the pixel was invalid.
 *     counts  optional, uint32[4]: {kept, removed, invalid, removed_components}; the first
 *             three sum to rows*cols.
 * The results are exact and deterministic: integers and copied bits.
 * rows*cols must fit int32. rows == 0 or cols == 0 is legal (counts all zero, nothing launched).
 * Argument errors (a type other than 16S / 32F, a negative size, too many pixels, unknown flag
 * bits, a negative or NaN max_diff, a negative max_size, a NULL map or out on a non-empty map,
 * a partial overlap of map and out, a NULL engine on the device entry) are BICOS_E_ARG before
 * any HIP call.
 * For int16 maps and an integral max_diff this is cv::filterSpeckles(img, newVal = -32768,
 * maxSpeckleSize = max_size, maxDiff = max_diff) on a map whose invalid pixels already hold
 * newVal -- a statement from reading that function's definition (regions of pixels != newVal
 * grown over 4-neighbours with |difference| <= maxDiff, filled with newVal when their pixel
 * count is <= maxSpeckleSize), not from a test against it. */
#define BICOS_SPECKLE_F32_SENTINEL 1
/* device: asynchronous on `stream`. The label and size arrays live in e's workspace (labels,
 * when given, is used directly as the label array). */
int bicos_speckle_device(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                         int max_size, float max_diff, int flags, void* out, int32_t* labels,
                         uint32_t* counts, void* stream);
/* host buffers, synchronous, e NULL = default engine: uploads the map, runs the same launches,
 * downloads the map, and the counts and the labels where asked. */
int bicos_speckle_host(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                       int max_size, float max_diff, int flags, void* out, int32_t* labels,
                       uint32_t counts[4]);
/* The tile (rows, cols) one workgroup labels in LDS (tests). Returns BICOS_OK. */
int bicos_speckle_tile(int* rows, int* cols);

/* --------------------------------------------------------- rectification */
/* The stage before match(): raw camera frames -> row-aligned (rectified) stacks, on the GPU. Two
 * operations: the lookup maps of one camera from its calibration, and the bilinear remap of a
 * whole stack through one pair of maps. The reference starts at rectified imagery and has neither.
 *
 * MAPS FROM CALIBRATION: cv::initUndistortRectifyMap's camera model with CV_32FC1 maps (a
 * statement from reading that function's definition, not from a test against it).
 *     K   9 doubles, row-major: fx = K[0], cx = K[2], fy = K[4], cy = K[5]. The skew K[1] is
 *         ignored, as OpenCV ignores it.
 *     D   nd in {0, 4, 5, 8} doubles k1 k2 p1 p2 [k3 [k4 k5 k6]]; missing coefficients are 0
 *         (D may be NULL with nd = 0).
 *     R   9 doubles, row-major, or NULL for the identity.
 *     P   3 rows of p_cols in {3, 4} doubles, row-major; only the left 3x3 is used.
 * On the host, in IEEE double without contraction:
 *     M[i][j] = ((P[i][0]*R[0][j] + P[i][1]*R[1][j]) + P[i][2]*R[2][j])
 *     det = (M00*(M11*M22 - M12*M21) - M01*(M10*M22 - M12*M20)) + M02*(M10*M21 - M11*M20)
 *     iM  = inverse(M) by cofactors, each element its cofactor divided by det:
 *         iM00 = (M11*M22 - M12*M21)/det  iM01 = (M02*M21 - M01*M22)/det  iM02 = (M01*M12 - M02*M11)/det
 *         iM10 = (M12*M20 - M10*M22)/det  iM11 = (M00*M22 - M02*M20)/det  iM12 = (M02*M10 - M00*M12)/det
 *         iM20 = (M10*M21 - M11*M20)/det  iM21 = (M01*M20 - M00*M21)/det  iM22 = (M00*M11 - M01*M10)/det
 * On the device, for output pixel (row v, column u), u and v converted to double, all in IEEE
 * double without contraction:
 *     X = (iM00*u + iM01*v) + iM02     Y = (iM10*u + iM11*v) + iM12     W = (iM20*u + iM21*v) + iM22
 *     x = X/W   y = Y/W   r2 = x*x + y*y
 *     kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2)
 *     xd = (x*kr + p1*((2*x)*y)) + p2*(r2 + (2*x)*x)
 *     yd = (y*kr + p1*(r2 + (2*y)*y)) + p2*((2*x)*y)
 *     map_x = (float)(fx*xd + cx)      map_y = (float)(fy*yd + cy)
 * Nonfinite results are stored as they come; the remap treats them as outside. The maps are dense
 * float32 [rows][cols]. A determinant that is 0 or not finite, any nonfinite input, an nd or p_cols
 * outside its set, a size < 1 or a NULL K, P, map (or D with nd > 0) is BICOS_E_ARG before any HIP
 * call.
 *
 * REMAP OF A STACK:
 *     src    n planes of src_rows x src_cols, u8 (depth 1) or u16 (depth 2), element (t, y, x) at
 *            base[t*src_plane_pitch + y*src_row_pitch + x]: pitches in ELEMENTS, exactly as
 *            bicos_match_device takes them
 *     map_x, map_y   float32 [rows][cols], absolute source coordinates (column, row); map_pitch is
 *            the BYTES between their rows (0 = dense, else a multiple of 4 and >= 4*cols)
 *     border 0 <= border <= 255 (u8) or 65535 (u16)
 *     dst    n planes of rows x cols of the same depth with pitches of its own (elements)
 *     valid  optional, uint8 [rows][cols] dense
 * Per output pixel, with x = map_x and y = map_y as float32:
 *     inside = x > -1 && x < src_cols && y > -1 && y < src_rows      (false for NaN; float32
 *            comparisons, the sizes converted to float32)
 *     not inside: every plane gets `border`, valid = 0. Otherwise
 *     x0 = floorf(x), fx = x - x0 (one float32 subtraction); y0, fy likewise
 *     p00 p01 p10 p11 = the taps at (y0, x0) (y0, x0+1) (y0+1, x0) (y0+1, x0+1), converted to
 *            float32; a tap outside the image has the value (float)border
 *     top = p00 + fx*(p01 - p00)   bot = p10 + fx*(p11 - p10)   v = top + fy*(bot - top)
 *            every operation rounded to float32 on its own, no fma
 *     out = (T)min(max(rintf(v), 0), max of the depth)               (ties to even)
 *     valid = 1 iff every tap with a nonzero weight lies in the image: column x0 and row y0
 *            always count, column x0+1 only if fx != 0, row y0+1 only if fy != 0
 * An identity map therefore reproduces the image byte for byte with valid all ones. The fractions
 * are full float32: finer than cv::remap's INTER_LINEAR, which quantises them to 1/32 pixel, so
 * the two differ in the last level here and there. Nothing here is tested against OpenCV.
 * Argument errors are BICOS_E_ARG (bicos_last_error says which) before any HIP call: n < 1; a
 * size < 1; depth not 1 or 2; a pitch smaller than a row; a map_pitch or host step that is not a
 * multiple of its element size; border out of range; a NULL src, dst or map; dst == src; a plane
 * that spans more than 2^32 - 1 elements. */
/* device: asynchronous on `stream`, no workspace, nothing allocated. */
int bicos_rectify_maps_device(const double K[9], const double* D, int nd, const double* R,
                              const double* P, int p_cols, int rows, int cols, float* map_x,
                              float* map_y, void* stream);
/* host maps, synchronous, through the current device's default engine. */
int bicos_rectify_maps_host(const double K[9], const double* D, int nd, const double* R,
                            const double* P, int p_cols, int rows, int cols, float* map_x,
                            float* map_y);
/* device: asynchronous on `stream`, one launch, no workspace: e may be NULL. */
int bicos_rectify_device(bicos_engine* e, const void* src, int n, int src_rows, int src_cols,
                         size_t src_row_pitch, size_t src_plane_pitch, int depth,
                         const float* map_x, const float* map_y, size_t map_pitch, int rows,
                         int cols, void* dst, size_t dst_row_pitch, size_t dst_plane_pitch,
                         int border, uint8_t* valid, void* stream);
/* host buffers, synchronous, e NULL = default engine: n image pointers in (src_rows x src_cols,
 * src_step BYTES per row, 0 = dense) and n out (rows x cols, dst_step likewise); the maps
 * (map_pitch as above) and valid in host memory. Uploads, runs the same launch, downloads. */
int bicos_rectify_host(bicos_engine* e, const void* const* src, int n, int src_rows, int src_cols,
                       size_t src_step, int depth, const float* map_x, const float* map_y,
                       size_t map_pitch, int rows, int cols, void* const* dst, size_t dst_step,
                       int border, uint8_t* valid);
/* The tile (rows, cols) of output pixels one workgroup remaps (tests). Returns BICOS_OK. */
int bicos_rectify_tile(int* rows, int* cols);

/* ---------------------------------------------------------- median filter */
/* The 3x3 or 5x5 median of a dense rows x cols disparity map (BICOS_CV_16S or BICOS_CV_32F), on
 * the GPU, that knows the map's invalid values and can fill small holes. The reference has no
 * such step. Parameters: ksize in {3, 5}, fill_min, flags.
 *     valid pixel  as in the speckle filter: an int16 that is not -32768; a float that is not
 *                  NaN and, with BICOS_MEDIAN_F32_SENTINEL, not -32768.0f either. Infinities
 *                  are valid.
 *     window of p  the ksize x ksize pixels centred on p that lie inside the image. There is no
 *                  border replication: a clipped window is simply smaller. V(p) is the multiset
 *                  of the valid values in the window, m = |V(p)|.
 *     order        int16 values as integers; floats by the integer key
 *                      k = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000)
 *                  compared unsigned: numeric order with -0.0 before +0.0, a total order on
 *                  every valid float. So the result is one definite element of V, whose bits
 *                  are copied.
 *     median(p)    the element of rank floor((m - 1) / 2), 0-based, of V sorted in that order:
 *                  the lower median, and the median for odd m.
 *     output       p valid on input: out(p) = median(p) (m >= 1: p is in its own window).
 *                  p invalid on input, fill_min > 0 and m >= fill_min: out(p) = median(p); the
 *                  hole is filled.
 *                  Otherwise p is copied bit for bit. The filter never creates an invalid pixel
 *                  and never changes one that it does not fill.
 *     fill_min     0: no filling; else 1 .. ksize*ksize. ksize*ksize/2 + 1 fills only holes
 *                  that valid pixels surround.
 * Outputs:
 *     out     same type and shape as the map. On the device entry it must not overlap the map
 *             (the filter reads neighbours): any overlap is an argument error. On the host
 *             entry out may be the input buffer.
 *     counts  optional, uint32[4]: {unchanged, changed, filled, invalid} = valid on input and
 *             the output bits equal the input bits; valid on input and they differ; invalid on
 *             input and valid on output; invalid on input and copied. They sum to rows*cols.
 * The results are exact and deterministic: integers and copied bits.
 * rows*cols must fit int32. rows == 0 or cols == 0 is legal (counts all zero, nothing launched).
 * Argument errors (a type other than 16S / 32F, a ksize other than 3 or 5, a fill_min outside
 * 0 .. ksize*ksize, unknown flag bits, a negative size, too many pixels, a NULL map or out on a
 * non-empty map, an overlap of map and out on the device entry) are BICOS_E_ARG before any HIP
 * call.
 * Where every pixel of a window is valid and inside the image, the result is that pixel of
 * cv::medianBlur(map, ksize) -- a statement from reading that function's definition (the
 * median of the ksize x ksize neighbourhood; for 16-bit and float images it offers exactly
 * the apertures 3 and 5), not from a test against it. At the border cv::medianBlur replicates
 * pixels where this filter clips the window. */
#define BICOS_MEDIAN_F32_SENTINEL 1
/* device: asynchronous on `stream`. Needs no workspace: e may be NULL. */
int bicos_median_device(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                        int ksize, int fill_min, int flags, void* out, uint32_t* counts, void* stream);
/* host buffers, synchronous, e NULL = default engine: uploads the map, runs the same launch,
 * downloads the map and the counts. */
int bicos_median_host(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                      int ksize, int fill_min, int flags, void* out, uint32_t counts[4]);
/* The output tile (rows, cols) of one workgroup (tests). Returns BICOS_OK. */
int bicos_median_tile(int* rows, int* cols);

/* --------------------------------------------------------- surface normals */
/* One unit normal per pixel of a dense rows x cols disparity map (BICOS_CV_16S or BICOS_CV_32F),
 * oriented towards the camera, on the GPU: the least-squares plane of the disparities over a
 * small window in (column, row, disparity), carried through Q. A plane there is a plane in 3-D
 * because Q is projective, and disparity noise is homogeneous there, where the noise of the 3-D
 * points grows with Z^2 along the ray. The reference has no such step.
 * The stage is for SUBPIXEL maps. On integer disparities a surface that moves less than one
 * level per window fits as a fronto-parallel stair step, whatever its tilt: this is no
 * alternative to the subpixel step of the match.
 * Inputs: the map; Q, 16 doubles, row-major; flags; radius in 1 .. 4; max_diff, a float >= 0 and
 * not NaN (+inf is legal); min_points in 3 .. (2*radius+1)^2.
 * Flags: BICOS_NORMALS_ALLOW_NEGATIVE_Z and BICOS_NORMALS_F32_SENTINEL have the meanings and
 * values of BICOS_REPROJECT_ALLOW_NEGATIVE_Z and BICOS_REPROJECT_F32_SENTINEL.
 * Arithmetic: everything below is IEEE double, one rounding per written operation and no
 * contraction, unless it says float32.
 *     reproj(x, y, d)   o[i] = ((Q[4i]*x + Q[4i+1]*y) + Q[4i+2]*d) + Q[4i+3], iw = 1.0/o[3],
 *                       returning (o[0]*iw, o[1]*iw, o[2]*iw) as doubles: the formula of
 *                       "reprojection" without the final cast.
 * For pixel p = (row y, column x) with disparity dp:
 *     1. own point   if bicos_reproject_* with the same map, Q and flags does not keep p, the
 *                    class is no_point (its classes invalid, nonfinite and negative_z).
 *     2. members     the window pixels q within `radius` of p in both axes, clipped to the image
 *                    without replication, that are valid in the sense of step 1's invalid test
 *                    and satisfy fabsf((float)dq - (float)dp) <= max_diff: one float32
 *                    subtraction, the speckle filter's link. p itself is always a member.
 *     3. sums        over the members in row-major window order, with du = col_q - x,
 *                    dv = row_q - y and e = (double)dq - (double)dp (one subtraction):
 *                    integers, exact: m (the member count), Su, Sv, Suu, Suv, Svv;
 *                    doubles, starting at 0.0: Sd = Sd + e; Sud = Sud + (double)du*e;
 *                    Svd = Svd + (double)dv*e, each a product and then an add. (For int16 maps
 *                    every one of these is an exact integer in any order.)
 *     4. sparse      m < min_points: the class is sparse.
 *     5. determinant in integers (every value is below 2^31):
 *                        C00 = Svv*m - Sv*Sv    C01 = Su*Sv - Suv*m     C02 = Suv*Sv - Svv*Su
 *                        C11 = Suu*m - Su*Su    C12 = Suv*Su - Suu*Sv   C22 = Suu*Svv - Suv*Suv
 *                        det = Suu*C00 + Suv*C01 + Su*C02
 *                    det == 0 (collinear members): the class is degenerate.
 *     6. plane       with the C's and det converted to double:
 *                        a = ((C00*Sud + C01*Svd) + C02*Sd) / det
 *                        b = ((C01*Sud + C11*Svd) + C12*Sd) / det
 *                        c = ((C02*Sud + C12*Svd) + C22*Sd) / det
 *                    the plane e ~ a*du + b*dv + c.
 *     7. vectors     d0 = (double)dp + c; P0 = reproj(x, y, d0); P1 = reproj(x + 1.0, y, d0 + a);
 *                    P2 = reproj(x, y + 1.0, d0 + b); U = P1 - P0; V = P2 - P0;
 *                    N = (Uy*Vz - Uz*Vy, Uz*Vx - Ux*Vz, Ux*Vy - Uy*Vx).
 *                    If (Nx*P0x + Ny*P0y) + Nz*P0z > 0, N is negated: the normal then faces the
 *                    origin of Q's frame.
 *     8. length      L = sqrt((Nx*Nx + Ny*Ny) + Nz*Nz); L zero or not finite: degenerate.
 *     9. result      otherwise the class is normal and the result is
 *                    ((float)(Nx/L), (float)(Ny/L), (float)(Nz/L)).
 * A pixel of any class but normal gets three NaNs (0x7FC00000).
 * Outputs, either alone or both:
 *     normal_map  float32 [rows][cols][3].
 *     normals     float32 [count][3], with index (int32 [count], as bicos_reproject_* writes
 *                 it): normals[i] is the normal of pixel index[i], bit for bit the map's. An
 *                 index outside 0 .. rows*cols-1 gives three NaNs and reads nothing.
 *     counts      optional, uint32[4] = {normal, no_point, sparse, degenerate} over the whole
 *                 map; they sum to rows*cols. Allowed only together with normal_map.
 * rows*cols must fit int32. rows == 0 or cols == 0 is legal: the counts are all zero and no map
 * is launched (a list then holds NaNs alone).
 * Argument errors are BICOS_E_ARG before any HIP call, and bicos_last_error says which: a type
 * other than 16S / 32F; unknown flag bits; radius, max_diff or min_points out of range; a
 * negative size or too many pixels for int32; a NULL map or Q on a non-empty map; no output at
 * all; normals without index or index without normals; counts without normal_map; an output
 * overlapping the map.
 * The results are deterministic, and equal to a float64 CPU evaluation of the text above bit for
 * bit. */
#define BICOS_NORMALS_ALLOW_NEGATIVE_Z 1
#define BICOS_NORMALS_F32_SENTINEL 2
/* device: asynchronous on `stream`. Needs no workspace: e may be NULL. */
int bicos_normals_device(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                         const double Q[16], int flags, int radius, float max_diff, int min_points,
                         float* normal_map, const int32_t* index, size_t count, float* normals,
                         uint32_t* counts, void* stream);
/* host buffers, synchronous, e NULL = default engine: uploads the map (and index), runs the same
 * launches, downloads what was asked for. */
int bicos_normals_host(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                       const double Q[16], int flags, int radius, float max_diff, int min_points,
                       float* normal_map, const int32_t* index, size_t count, float* normals,
                       uint32_t counts[4]);
/* The tile (rows, cols) of the dense map one workgroup stages (tests). Returns BICOS_OK. */
int bicos_normals_tile(int* rows, int* cols);

/* -------------------------------------------------------------------- mesh */
/* A dense rows x cols disparity map triangulated on the GPU. The map is an organised grid, so
 * every 2x2 block of pixels is a quad of at most two triangles and no neighbour search is
 * needed. The reference has no such step.
 * Inputs: the map, BICOS_CV_16S or BICOS_CV_32F; Q, 16 doubles, row-major; flags,
 * BICOS_MESH_ALLOW_NEGATIVE_Z and BICOS_MESH_F32_SENTINEL with the values and meanings of the
 * BICOS_REPROJECT_* flags; max_diff, a float >= 0 and not NaN (+inf is legal).
 * Vertices: exactly the ordered point list of bicos_reproject_* for the same map, Q and flags:
 *     the kept points in row-major pixel order, the same optional index, the same counts[4] =
 *     {kept, invalid, nonfinite, negative_z}. Vertex number v is position v in that list. Kept
 *     points that no triangle uses stay in the list, so normals[i] of bicos_normals_* with the
 *     same index is the normal of vertex i.
 * Link: two pixels p, q are linked iff fabsf((float)d_p - (float)d_q) <= max_diff, with one
 *     float32 subtraction: the speckle filter's link. It is only ever evaluated between kept
 *     pixels, so both values are finite numbers.
 * Quads: one for every (r, c) with 0 <= r < rows-1 and 0 <= c < cols-1, with the corners
 *     A = (r, c), B = (r, c+1), C = (r+1, c), D = (r+1, c+1). Its candidate triangles:
 *         kept corners   condition                                        T0         T1
 *         all four       fabsf((float)dA-(float)dD) <= fabsf((float)dB-(float)dC)
 *                        (diagonal AD; a tie takes AD)                    (A,C,D)    (A,D,B)
 *         all four       otherwise (diagonal BC)                          (A,C,B)    (B,C,D)
 *         three, D missing                                                (A,C,B)    -
 *         three, A missing                                                (B,C,D)    -
 *         three, B missing                                                (A,C,D)    -
 *         three, C missing                                                (A,D,B)    -
 *         fewer than three                                                none       none
 *     A candidate is emitted iff all three of its edges are linked. Every triangle therefore
 *     turns the same way in the image: with x to the right and y down, (p1-p0) x (p2-p0) has a
 *     negative z.
 * Outputs:
 *     points, index, counts   the vertices, as bicos_reproject_* writes them; vertex_capacity
 *                 behaves as its capacity does. index may be NULL.
 *     triangles   int32 [tri_capacity][3]: the vertex numbers of each triangle's corners in the
 *                 order written above. Quads come in row-major order, and within a quad T0 comes
 *                 before T1. Integers only: the output is deterministic. With more triangles
 *                 than tri_capacity the first tri_capacity are written and nothing past them.
 *     mesh_counts uint32[4] = {triangles, quads with 2 triangles, quads with 1, quads with 0}.
 *                 The last three sum to (rows-1)*(cols-1), which is 0 when rows < 2 or cols < 2;
 *                 the first is 2*q2 + q1, the full number whatever tri_capacity is.
 *     vertex_map  optional, int32 [rows][cols]: the pixel's vertex number, or -1 where the pixel
 *                 is not kept. When given, the stage uses it as its rank array; otherwise that
 *                 array lives in the engine's workspace (as the speckle filter's labels do).
 *     Triangle entries and vertex_map always use the numbering of the full list, also when
 *     kept > vertex_capacity; the caller sees that in counts[0].
 * rows*cols must fit int32. rows == 0 or cols == 0 is legal: all counts are zero and nothing is
 * launched. rows == 1 or cols == 1 gives vertices and no triangles.
 * Argument errors are BICOS_E_ARG before any HIP call, and bicos_last_error says which: a type
 * other than 16S / 32F; unknown flag bits; a negative or NaN max_diff; a negative size; too many
 * pixels for int32; a NULL map, Q, points, triangles, counts or mesh_counts on a non-empty map; a
 * NULL engine on the device entry; any output overlapping the map or another output. */
#define BICOS_MESH_ALLOW_NEGATIVE_Z 1
#define BICOS_MESH_F32_SENTINEL 2
/* device: asynchronous on `stream`; e is required (workspace). */
int bicos_mesh_device(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                      const double Q[16], int flags, float max_diff, float* points, int32_t* index,
                      size_t vertex_capacity, uint32_t* counts, int32_t* triangles,
                      size_t tri_capacity, uint32_t* mesh_counts, int32_t* vertex_map, void* stream);
/* host buffers, synchronous, e NULL = default engine: uploads the map, runs the same launches,
 * downloads the counts first, then only the first min(kept, vertex_capacity) points and
 * min(triangles, tri_capacity) triangles (and vertex_map whole, where given). */
int bicos_mesh_host(bicos_engine* e, const void* disparity, int disp_type, int rows, int cols,
                    const double Q[16], int flags, float max_diff, float* points, int32_t* index,
                    size_t vertex_capacity, uint32_t counts[4], int32_t* triangles,
                    size_t tri_capacity, uint32_t mesh_counts[4], int32_t* vertex_map);
/* Pixels per segment of the mesh's launches: bicos_reproject_segment's (tests). */
int bicos_mesh_segment(void);

/* -------------------------------------------------------------- projection */
/* A point list projected into another camera on the GPU: a pixel position, a depth and a class
 * per point, the value of that camera's image at the point (a texture), and the scan as that
 * camera sees it: a depth image and an index image registered to its pixel grid, through a
 * z-buffer that also tells which points a nearer surface hides. The reference has no such step.
 * Inputs:
 *     points  float32 [count][3] in the frame of Q (the rectified left camera): the list of
 *             bicos_reproject_* or bicos_mesh_*, or a dense xyz_map taken as a list, whose NaN
 *             triples are simply of class invalid. count must fit int32; count == 0 is legal.
 *     R, t    9 doubles, row-major (NULL = identity) and 3 doubles (NULL = zero): Pc = R*P + t.
 *     K, D, nd   the rectification section's model and coefficient order: fx = K[0], cx = K[2],
 *             fy = K[4], cy = K[5], the skew K[1] ignored; nd in {0, 4, 5, 8} doubles
 *             k1 k2 p1 p2 [k3 [k4 k5 k6]], missing coefficients 0 (D may be NULL with nd = 0).
 *     img_rows x img_cols   the camera's image size; img_rows*img_cols must fit int32. An empty
 *             image is legal: every point in front of the camera is then outside.
 *     splat   0 .. 3: in the z-buffer a point covers the (2*splat+1)^2 pixels around its own,
 *             clipped to the image.
 *     tol     a float32 >= 0 and not NaN; +inf is legal and means no occlusion test.
 *     image   optional, the texture source: u8 (img_depth 1) or u16 (img_depth 2), channels in
 *             {1, 3} interleaved, element (y, x, k) at base[y*img_pitch + x*channels + k] with
 *             img_pitch in ELEMENTS, >= img_cols*channels. fill, 0 <= fill <= 255 or 65535: the
 *             value of every channel of a point that is not visible. With image == NULL,
 *             img_depth, channels, img_pitch and fill are not looked at.
 * Per point i. All arithmetic is IEEE double, one rounding per written operation and no
 * contraction, unless it says float32:
 *     1. invalid: X, Y or Z is not finite.
 *     2. Xc = ((R00*X + R01*Y) + R02*Z) + t0, likewise Yc (row 1) and Zc (row 2), X Y Z converted
 *        to double. behind: !(Zc > 0).
 *     3. x = Xc/Zc, y = Yc/Zc, then r2, kr, xd, yd exactly as the rectification section writes
 *        them; u = fx*xd + cx, v = fy*yd + cy; uf = (float)u, vf = (float)v, zf = (float)Zc.
 *     4. pxf = floorf(uf + 0.5f), pyf = floorf(vf + 0.5f), one float32 addition each: the point's
 *        own pixel. outside: unless uf and vf are finite and 0 <= pxf < img_cols and
 *        0 <= pyf < img_rows (float32 compares, the sizes converted to float32). So uf = -0.5 is
 *        inside and uf = img_cols - 0.5 is outside.
 *     5. z-buffer: every point that is none of the above offers the key
 *        ((uint64)bits(zf) << 32) | (uint32)i to each pixel of its splat; a pixel keeps the
 *        smallest key. zf is a non-negative float, so its bits order as its value does: the
 *        nearest point wins and equal depths go to the smaller i. The result does not depend on
 *        the order of arrival: it is deterministic.
 *     6. zmin = the depth kept at the point's own pixel (which its own splat always covers).
 *        occluded: !(zf <= zmin + tol), one float32 addition. Otherwise visible.
 *     7. texture of a visible point, per channel, the remap's arithmetic with the edge replicated:
 *        x0 = floorf(uf), fx = uf - x0 (one float32 subtraction), the taps at the columns
 *        clamp(x0, 0, img_cols-1) and clamp(x0+1, 0, img_cols-1); y0, fy and the rows likewise;
 *        top = p00 + fx*(p01 - p00)   bot = p10 + fx*(p11 - p10)   v = top + fy*(bot - top)
 *        every operation rounded to float32 on its own, no fma;
 *        out = (T)min(max(rintf(v), 0), max of the depth)            (ties to even)
 *        Every other class gets fill in every channel.
 * Outputs, each optional, at least one required:
 *     uv         float32 [count][2]: two NaNs for invalid and behind, (uf, vf) for every other
 *                class, outside included.
 *     depth      float32 [count]: zf, or NaN for invalid and behind.
 *     cls        uint8 [count]: BICOS_PROJECT_VISIBLE 0, _OCCLUDED 1, _OUTSIDE 2, _BEHIND 3,
 *                _INVALID 4.
 *     tex        [count][channels] of the image's type; requires image.
 *     depth_map  float32 [img_rows][img_cols]: the kept depth, NaN where no splat fell.
 *     index_map  int32 [img_rows][img_cols]: the list position of the point that won the pixel,
 *                -1 where none.
 *     counts     uint32[5] = {visible, occluded, outside, behind, invalid}, summing to count.
 *     Every NaN the stage writes is the quiet NaN 0x7FC00000.
 * The z-buffer is needed only when tol is finite or a map is asked for; its keys, 8 bytes per
 * pixel, live in the engine's workspace. Otherwise the stage is one launch with no workspace, and
 * e may be NULL. A point's (uf, vf, zf) is computed again by the launch that needs it, not kept:
 * the stage has no per-point workspace.
 * Argument errors are BICOS_E_ARG before any HIP call, and bicos_last_error says which: no
 * output; tex without image; channels, img_depth, nd, splat, tol or fill out of range; a pitch
 * shorter than a row; a negative size; count or img_rows*img_cols beyond int32; a nonfinite
 * camera entry; a NULL points or K with count > 0 (a NULL D with nd > 0); an output overlapping
 * an input or another output; a NULL engine where the z-buffer is needed. */
#define BICOS_PROJECT_VISIBLE 0
#define BICOS_PROJECT_OCCLUDED 1
#define BICOS_PROJECT_OUTSIDE 2
#define BICOS_PROJECT_BEHIND 3
#define BICOS_PROJECT_INVALID 4
#define BICOS_PROJECT_MAX_SPLAT 3
/* device: asynchronous on `stream`. */
int bicos_project_device(bicos_engine* e, const float* points, size_t count, const double* R,
                         const double* t, const double K[9], const double* D, int nd, int img_rows,
                         int img_cols, int splat, float tol, const void* image, int img_depth,
                         int channels, size_t img_pitch, int fill, float* uv, float* depth,
                         uint8_t* cls, void* tex, float* depth_map, int32_t* index_map,
                         uint32_t* counts, void* stream);
/* host buffers, synchronous, e NULL = default engine: uploads the points and the image, runs the
 * same launches, downloads what was asked for. */
int bicos_project_host(bicos_engine* e, const float* points, size_t count, const double* R,
                       const double* t, const double K[9], const double* D, int nd, int img_rows,
                       int img_cols, int splat, float tol, const void* image, int img_depth,
                       int channels, size_t img_pitch, int fill, float* uv, float* depth,
                       uint8_t* cls, void* tex, float* depth_map, int32_t* index_map,
                       uint32_t counts[5]);
/* Points per workgroup of the point launches (tests). */
int bicos_project_group(void);

/* --------------------------------------------------------- disparity guide */
/* The search restricted to one disparity window PER LEFT PIXEL, from a prior: the previous
 * frame's map of a continuous scan, the match of a downsampled stack, a CAD pose, a
 * neighbouring view (no reference counterpart).
 *   guide       int16 pairs, guide[row * guide_pitch + col] = {lo, hi}: one dword per pixel, lo
 *               in its low half. guide_pitch is counted in PIXELS (dwords) and is >= cols; the
 *               base is 4-byte aligned. Device memory for the *_device entries, host memory
 *               for bicos_match_host_guided.
 *   window      every guided call also takes the global window min_disparity <= max_disparity
 *               with the meaning and clamping of the *_range calls ("disparity range" above);
 *               (INT_MIN, INT_MAX) is allowed and means no global bound.
 *   candidates  of the left pixel (row, col0): C(row, col0) = { col1 : 0 <= col1 < cols and
 *               max(min_disparity, lo) <= col0 - col1 <= min(max_disparity, hi) }
 *   search      the reference's bicos_search over C in ascending col1: the first minimum wins;
 *               NoDuplicates rejects a minimum that occurs more than once WITHIN C; a pixel
 *               with an empty C is invalid. lo > hi is legal and gives an empty C ("do not
 *               search here"); so does a window wholly outside the image.
 *   consistency the right view has no prior, so its pixels have no guide: the reverse search
 *               is exactly that of the *_range call with the same global window,
 *               [-max_disparity, -min_disparity] with the descriptor sets swapped, run by the
 *               same kernel. The max_lr_diff check and the output formula are unchanged. A
 *               TIGHT GLOBAL WINDOW is therefore what keeps the reverse search fast: pass the
 *               bounding window of the guide, not (INT_MIN, INT_MAX), where one is known. A
 *               transposed per-pixel mask for the reverse search is left for a later change.
 * Identities, byte for byte: a guide whose every pixel is (min_disparity, max_disparity) gives
 * the *_range call's maps; a guide and a global window that both cover [-(cols-1), cols-1]
 * give the unrestricted call's maps.
 * Restrictions, those of the *_range calls: the guided search runs on the matrix cores only
 * (search_guided.hip) with separate consistency / agree launches; bicos_match_plan reports
 * nothing new; the multi-GPU entries (bicos_match_host_multi, bicos_match_bands_device) take
 * no guide.
 * A NULL guide, guide_pitch < cols, a base that is not 4-byte aligned and min_disparity >
 * max_disparity are BICOS_E_ARG before any HIP call; bicos_last_error names the cause. */
int bicos_search_device_guided(bicos_engine* e, const uint32_t* desc0, const uint32_t* desc1,
                               int rows, int cols, int words, int flags, int max_lr_diff,
                               int min_disparity, int max_disparity, const int16_t* guide,
                               size_t guide_pitch, int16_t* out, void* stream);
int bicos_match_device_guided(bicos_engine* e, const void* stack0, const void* stack1, int n,
                              int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
                              const BicosConfig* cfg, int has_nxcorr, int min_disparity,
                              int max_disparity, const int16_t* guide, size_t guide_pitch,
                              void* disparity, void* corrmap, void* stream);
/* host buffers (the guide too; uploaded whole before the first band), synchronous */
int bicos_match_host_guided(bicos_engine* e, const void* const* stack0, const void* const* stack1,
                            int n, int rows, int cols, size_t step, int depth,
                            const BicosConfig* cfg, int has_nxcorr, int min_disparity,
                            int max_disparity, const int16_t* guide, size_t guide_pitch,
                            void* disparity, void* corrmap);

/* The guide builder: a rows x cols guide from a prior disparity map of its own size prows x
 * pcols (dense). prior_type BICOS_CV_16S (invalid: -32768) or BICOS_CV_32F (invalid: NaN, and
 * -32768.0f with BICOS_GUIDE_F32_SENTINEL). scale 1..8 (output pixels per prior pixel, and the
 * factor of its disparities), radius 0..32767, spread 0..7, and the fallback pair, any two
 * int16 values (lo > hi: "do not search here"). For the output pixel (r, c):
 *   pr = min(r / scale, prows - 1), pc = min(c / scale, pcols - 1)
 *   N  = the valid prior values in the (2 spread + 1)^2 window around (pr, pc), clipped to the
 *        prior map
 *   N empty:  {lo, hi} = {fallback_lo, fallback_hi}
 *   else:     lo = scale * floor(min N) - radius
 *             hi = scale * ceil(max N) + (scale - 1) + radius
 * floor and ceil are taken in float and clamped to +-32767 before the conversion to int; lo
 * and hi are computed in int32 and clamped to [-32767, 32767]: integer-exact throughout.
 * counts, if not NULL: uint32[2] {from_prior, fallback}, which add up to rows * cols.
 * guide_pitch in pixels, 0 = cols. One launch, no workspace. Out-of-range parameters, a null
 * or misaligned guide and a null or empty prior for a non-empty guide are BICOS_E_ARG before
 * any HIP call. */
#define BICOS_GUIDE_F32_SENTINEL 1
/* device: asynchronous on `stream`. Needs no workspace: e may be NULL. */
int bicos_guide_device(bicos_engine* e, const void* prior, int prior_type, int prows, int pcols,
                       int rows, int cols, int scale, int radius, int spread, int fallback_lo,
                       int fallback_hi, int flags, int16_t* guide, size_t guide_pitch,
                       uint32_t* counts, void* stream);
/* host buffers, synchronous, e NULL = default engine */
int bicos_guide_host(bicos_engine* e, const void* prior, int prior_type, int prows, int pcols,
                     int rows, int cols, int scale, int radius, int spread, int fallback_lo,
                     int fallback_hi, int flags, int16_t* guide, size_t guide_pitch,
                     uint32_t counts[2]);

/* ---------------------------------------------------------- stack pooling */
/* An image stack pooled by an integer factor, on the GPU: the first level of a coarse-to-fine
 * match (the pyramid match below), defined in integers so that every caller gets the same
 * pooled stack. The reference has no such step.
 *     src    n planes of rows x cols, u8 (depth 1) or u16 (depth 2), element (t, y, x) at
 *            base[t*src_plane_pitch + y*src_row_pitch + x]: pitches in ELEMENTS, exactly as
 *            bicos_match_device takes them. Any base with the element's alignment and any
 *            pitch >= a row are accepted: views of larger buffers are passed as they lie.
 *     scale  s in 2 .. 8
 *     dst    n planes of prows x pcols of the same depth with pitches of its own (elements),
 *            prows = rows / s, pcols = cols / s (integer division). This is the size
 *            bicos_guide_device expects of a prior at `scale` s: pr = min(r / s, prows - 1).
 * For each plane t and output pixel (R, C):
 *     sum = the s*s source elements of rows s*R .. s*R + s-1 and columns s*C .. s*C + s-1,
 *           added in uint32 (at most 64 * 65535)
 *     out = (sum + s*s/2) / (s*s)       integer division: the mean, rounded half up
 * The result is exact, never above the depth's maximum, and there is no float anywhere. The
 * trailing rows % s rows and cols % s columns are not read; nor is any byte between rows,
 * between planes or around either view, and no byte outside the prows x pcols pixels of each
 * output plane is written. (A numpy mean through float64 with .astype truncates instead of
 * rounding: it is NOT this stage.)
 * Alignment selects kernels, never results: a source whose base and two pitches are multiples
 * of 4 BYTES is read by the dword-load kernel, every other source by the per-element kernel; the
 * dword-load kernel stores four pixels at once where the output's base and two pitches are
 * multiples of 4 bytes too, else element by element (bicos_pool_kernel says which).
 * Argument errors are BICOS_E_ARG (bicos_last_error says which) before any HIP call: n < 1;
 * depth not 1 or 2; scale outside 2 .. 8; rows < scale or cols < scale; a pitch smaller than a
 * row; a NULL pointer; a u16 base that is not 2-byte aligned; a host step that is not a multiple
 * of the element size; dst overlapping src on the device entry; a plane that spans more than
 * 2^32 - 1 elements. A pitch is only held to be >= a row, so that interleaved layouts pass: an
 * output whose own rows or planes overlap each other (dst_plane_pitch below (prows - 1) *
 * dst_row_pitch + pcols without interleaving) is the caller's error, is not detected, and leaves
 * the overlapping pixels undefined. */
/* device: asynchronous on `stream`, one launch, no workspace: e may be NULL. */
int bicos_pool_device(bicos_engine* e, const void* src, int n, int rows, int cols,
                      size_t src_row_pitch, size_t src_plane_pitch, int depth, int scale,
                      void* dst, size_t dst_row_pitch, size_t dst_plane_pitch, void* stream);
/* host buffers, synchronous, e NULL = default engine: n image pointers in (rows x cols, src_step
 * BYTES per row, 0 = dense) and n out (prows x pcols, dst_step likewise). Uploads what the
 * launch reads, runs the same launch, downloads. */
int bicos_pool_host(bicos_engine* e, const void* const* src, int n, int rows, int cols,
                    size_t src_step, int depth, int scale, void* const* dst, size_t dst_step);
/* The tile (rows, cols) of OUTPUT pixels one workgroup pools (tests). Returns BICOS_OK. */
int bicos_pool_tile(int* rows, int* cols);
/* Which kernel bicos_pool_device runs on these views (tests): bit 0 set: the dword-load kernel,
 * clear: the per-element kernel; bit 1 set: the output is aligned for vector stores (used by
 * the dword-load kernel alone). Pitches in elements. No launch. */
int bicos_pool_kernel(const void* src, size_t src_row_pitch, size_t src_plane_pitch, int depth,
                      const void* dst, size_t dst_row_pitch, size_t dst_plane_pitch);

/* ---------------------------------------------------------- pyramid match */
/* The coarse-to-fine match in one call: for scenes whose disparity range is too wide for one
 * window. DEFINITION: the maps are byte for byte those of these four calls in this order on
 * the same stream, with prows = rows / scale, pcols = cols / scale:
 *   1. bicos_pool_device of both stacks with `scale` into dense prows x pcols stacks;
 *   2. bicos_match_device_range of the pooled stacks with cfg' and the window
 *      [floor(min_disparity / scale), ceil(max_disparity / scale)] (mathematical rounding, in
 *      int64; bicos_pyramid_window), corrmap NULL. cfg' is cfg with subpixel_step = -1 and
 *      nothing else changed; has_nxcorr is passed on. The coarse map's type is
 *      bicos_output_type(cfg', has_nxcorr): float32 with the NXC stage, else int16;
 *   3. bicos_guide_device of that map (prior_type its type) with prows, pcols, rows, cols,
 *      scale, radius, spread, fallback_lo, fallback_hi, the flag BICOS_GUIDE_F32_SENTINEL,
 *      guide_pitch = cols, and `counts`;
 *   4. bicos_match_device_guided of the full stacks with cfg, the window [min_disparity,
 *      max_disparity] and that guide.
 * Optional outputs, each NULL or a buffer the call fills: `coarse`, the coarse map, dense
 * prows x pcols; `guide`, dense rows x cols int16 pairs, 4-byte aligned (it can serve as the
 * next frame's prior input); `counts`, uint32[2] {from_prior, fallback} of step 3. What the
 * caller does not keep, and the pooled stacks always, lives in a buffer of the engine.
 * The device entry only enqueues: no host synchronisation, and no allocation but the
 * stream-ordered growth of the engine's buffers.
 * Errors: whatever any of the four calls refuses, each detected before any HIP call.
 * Restrictions, those of the guided entries: the searches run on the matrix cores only
 * (search_range.hip, search_guided.hip) with separate consistency / agree launches; the
 * multi-GPU entries have no pyramid form; there is no int16-out form (bicos_match_device_i16).
 * The host entry uploads each stack once, whole, runs the device pyramid on the engine's own
 * stream and downloads the maps and what else is asked for; it does not overlap upload and
 * match band by band as bicos_match_host does. */
int bicos_match_device_pyramid(bicos_engine* e, const void* stack0, const void* stack1, int n,
                               int rows, int cols, size_t row_pitch, size_t plane_pitch, int depth,
                               const BicosConfig* cfg, int has_nxcorr, int min_disparity,
                               int max_disparity, int scale, int radius, int spread,
                               int fallback_lo, int fallback_hi, void* disparity, void* corrmap,
                               void* coarse, int16_t* guide, uint32_t* counts, void* stream);
/* host buffers (coarse, guide and counts too), `step` BYTES per image row (0 = dense),
 * synchronous, e NULL = default engine */
int bicos_match_host_pyramid(bicos_engine* e, const void* const* stack0, const void* const* stack1,
                             int n, int rows, int cols, size_t step, int depth,
                             const BicosConfig* cfg, int has_nxcorr, int min_disparity,
                             int max_disparity, int scale, int radius, int spread, int fallback_lo,
                             int fallback_hi, void* disparity, void* corrmap, void* coarse,
                             int16_t* guide, uint32_t counts[2]);
/* The coarse window of step 2 (scale 2 .. 8, else BICOS_E_ARG). */
int bicos_pyramid_window(int min_disparity, int max_disparity, int scale, int* lo, int* hi);

/* Build identification (arch, flags) for reports. */
const char* bicos_build_info(void);

#ifdef __cplusplus
}
#endif

#endif /* BICOS_C_H */
