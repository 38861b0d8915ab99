"""ctypes binding of libbicos_amd.so (include/bicos_c.h).

The product path has exactly one implementation: the gfx950 HIP engine in this
shared library. There is no CPU fallback -- if the library is missing or fails
to load, importing the package's compute entry points raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbicos_amd.so")
CSRC = os.path.join(_HERE, "csrc")

BICOS_OK = 0
BICOS_E_ARG = -1
BICOS_E_BITS = -2
BICOS_E_HIP = -3
BICOS_E_INTERNAL = -4

CV_8U, CV_16U, CV_16S, CV_32F, CV_64F = 0, 2, 3, 5, 6


class BicosConfig(ctypes.Structure):
    """reference src/pybicos_c.cpp:30-41, with `precision` always present."""
    _fields_ = [
        ("nxcorr_threshold", ctypes.c_float),
        ("subpixel_step", ctypes.c_float),
        ("min_variance", ctypes.c_float),
        ("mode", ctypes.c_int),
        ("precision", ctypes.c_int),
        ("variant_type", ctypes.c_int),
        ("max_lr_diff", ctypes.c_int),
        ("no_dupes", ctypes.c_int),
    ]


class BicosResult(ctypes.Structure):
    """reference src/pybicos_c.cpp:44-53."""
    _fields_ = [
        ("disparity_data", ctypes.c_void_p),
        ("disparity_rows", ctypes.c_int),
        ("disparity_cols", ctypes.c_int),
        ("disparity_type", ctypes.c_int),
        ("corrmap_data", ctypes.c_void_p),
        ("corrmap_rows", ctypes.c_int),
        ("corrmap_cols", ctypes.c_int),
        ("corrmap_type", ctypes.c_int),
    ]


# every symbol include/bicos_c.h declares (tests check the .so exports them all)
EXPORTS = (
    "BICOS_CreateDefaultConfig", "BICOS_FreeConfig", "BICOS_FreeResult", "BICOS_Match",
    "BICOS_InvalidDisparityFloat", "BICOS_InvalidDisparityInt16", "bicos_last_error",
    "bicos_engine_create", "bicos_engine_default", "bicos_engine_destroy", "bicos_engine_tune", "bicos_descriptor_words", "bicos_output_type",
    "bicos_match_device", "bicos_match_device_i16", "bicos_match_host", "bicos_match_host_multi", "bicos_match_bands_device",
    "bicos_desc_pitch", "bicos_transform_device", "bicos_search_device",
    "bicos_agree_device", "bicos_subpixel_device", "bicos_agree_stage_device", "bicos_build_info",
    "bicos_match_plan", "bicos_search_agree_device", "bicos_search_packed", "bicos_search_packed_product",
    "bicos_agree_kernel",
    "bicos_transform_kernel",
    "bicos_match_device_range", "bicos_match_host_range", "bicos_search_device_range",
    "bicos_reproject_device", "bicos_reproject_host", "bicos_reproject_segment",
    "bicos_speckle_device", "bicos_speckle_host", "bicos_speckle_tile",
    "bicos_rectify_maps_device", "bicos_rectify_maps_host", "bicos_rectify_device",
    "bicos_rectify_host", "bicos_rectify_tile",
    "bicos_median_device", "bicos_median_host", "bicos_median_tile",
    "bicos_normals_device", "bicos_normals_host", "bicos_normals_tile",
    "bicos_mesh_device", "bicos_mesh_host", "bicos_mesh_segment",
    "bicos_project_device", "bicos_project_host", "bicos_project_group",
    "bicos_search_device_guided", "bicos_match_device_guided", "bicos_match_host_guided",
    "bicos_guide_device", "bicos_guide_host",
    "bicos_pool_device", "bicos_pool_host", "bicos_pool_tile", "bicos_pool_kernel",
    "bicos_match_device_pyramid", "bicos_match_host_pyramid", "bicos_pyramid_window",
)

# bicos_match_plan bits (include/bicos_c.h)
PLAN_MATRIX_CORES = 1
PLAN_PACKED_KEYS = 2
PLAN_AGREE_IN_SEARCH = 4
PLAN_REVERSE_COMPACTED = 8
PLAN_CONSISTENCY_IN_AGREE = 16
PLAN_DENSE_ROWS = 32
PLAN_CONSISTENCY_ONE_PASS = 64

# bicos_reproject_* flags (include/bicos_c.h)
REPROJECT_ALLOW_NEGATIVE_Z = 1
REPROJECT_F32_SENTINEL = 2

# bicos_speckle_* flag (include/bicos_c.h)
SPECKLE_F32_SENTINEL = 1

# bicos_median_* flag (include/bicos_c.h)
MEDIAN_F32_SENTINEL = 1

# bicos_normals_* flags (include/bicos_c.h): the values of the bicos_reproject_* flags
NORMALS_ALLOW_NEGATIVE_Z = 1
NORMALS_F32_SENTINEL = 2
NORMALS_MAX_RADIUS = 4

# bicos_mesh_* flags (include/bicos_c.h): the values of the bicos_reproject_* flags
MESH_ALLOW_NEGATIVE_Z = 1
MESH_F32_SENTINEL = 2

# bicos_project_* classes and the largest splat (include/bicos_c.h)
PROJECT_VISIBLE, PROJECT_OCCLUDED, PROJECT_OUTSIDE, PROJECT_BEHIND, PROJECT_INVALID = range(5)
PROJECT_CLASSES = ("visible", "occluded", "outside", "behind", "invalid")
PROJECT_MAX_SPLAT = 3

# bicos_guide_* flag (include/bicos_c.h)
GUIDE_F32_SENTINEL = 1

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def build(verbose: bool = False, jobs: int = 4) -> str:
    """Compile libbicos_amd.so for gfx950 with hipcc (in-tree)."""
    out = subprocess.run(["make", "-C", CSRC, "-j%d" % jobs, "all"], capture_output=True,
                         text=True)
    if verbose:
        print(out.stdout, out.stderr)
    if out.returncode != 0:
        raise RuntimeError("libbicos_amd build failed:\n" + out.stdout[-4000:] + out.stderr[-4000:])
    return LIB_PATH


_lib = None


class BicosError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libbicos_amd.so not built at %s -- run libbicos_amd._lib.build() "
                          "(hipcc, gfx950)" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    P, I, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    PI = ctypes.POINTER(ctypes.c_int)
    PP = ctypes.POINTER(ctypes.c_void_p)
    L.BICOS_CreateDefaultConfig.restype = ctypes.POINTER(BicosConfig)
    L.BICOS_CreateDefaultConfig.argtypes = []
    L.BICOS_FreeConfig.argtypes = [ctypes.POINTER(BicosConfig)]
    L.BICOS_FreeConfig.restype = None
    L.BICOS_FreeResult.argtypes = [ctypes.POINTER(BicosResult)]
    L.BICOS_FreeResult.restype = None
    L.BICOS_Match.argtypes = [PP, PI, PI, PI, I, PP, PI, PI, PI, I, ctypes.POINTER(BicosConfig)]
    L.BICOS_Match.restype = ctypes.POINTER(BicosResult)
    L.BICOS_InvalidDisparityFloat.restype = F
    L.BICOS_InvalidDisparityFloat.argtypes = []
    L.BICOS_InvalidDisparityInt16.restype = ctypes.c_int16
    L.BICOS_InvalidDisparityInt16.argtypes = []
    L.bicos_last_error.restype = ctypes.c_char_p
    L.bicos_last_error.argtypes = []
    L.bicos_engine_create.argtypes = [I, ctypes.POINTER(P)]
    L.bicos_engine_create.restype = I
    L.bicos_engine_default.argtypes = [I]
    L.bicos_engine_default.restype = P
    L.bicos_engine_destroy.argtypes = [P]
    L.bicos_engine_destroy.restype = None
    L.bicos_engine_tune.argtypes = [P, I, I, I, I]
    L.bicos_engine_tune.restype = I
    L.bicos_descriptor_words.argtypes = [I, I]
    L.bicos_descriptor_words.restype = I
    L.bicos_output_type.argtypes = [ctypes.POINTER(BicosConfig), I]
    L.bicos_output_type.restype = I
    L.bicos_match_device.argtypes = [P, P, P, I, I, I, Z, Z, I, ctypes.POINTER(BicosConfig), I,
                                     P, P, P]
    L.bicos_match_device.restype = I
    L.bicos_match_device_i16.argtypes = L.bicos_match_device.argtypes
    L.bicos_match_device_i16.restype = I
    L.bicos_match_host.argtypes = [P, PP, PP, I, I, I, Z, I, ctypes.POINTER(BicosConfig), I, P, P]
    L.bicos_match_host.restype = I
    PZ = ctypes.POINTER(ctypes.c_size_t)
    L.bicos_match_host_multi.argtypes = [PI, I, PP, PP, I, I, I, Z, I,
                                         ctypes.POINTER(BicosConfig), I, P, P]
    L.bicos_match_host_multi.restype = I
    L.bicos_match_bands_device.argtypes = [PI, I, PP, PP, PI, PZ, PZ, I, I, I,
                                           ctypes.POINTER(BicosConfig), I, P, P]
    L.bicos_match_bands_device.restype = I
    L.bicos_desc_pitch.argtypes = [I, I]
    L.bicos_desc_pitch.restype = Z
    L.bicos_transform_device.argtypes = [P, I, I, I, Z, Z, I, I, I, P, P]
    L.bicos_transform_device.restype = I
    L.bicos_search_device.argtypes = [P, P, P, I, I, I, I, I, P, P]
    L.bicos_search_device.restype = I
    L.bicos_agree_device.argtypes = [P, P, P, I, I, I, Z, Z, I, F, I, F, P, P, P]
    L.bicos_agree_device.restype = I
    L.bicos_subpixel_device.argtypes = [P, P, P, I, I, I, Z, Z, I, F, F, I, F, P, P, P]
    L.bicos_subpixel_device.restype = I
    L.bicos_agree_stage_device.argtypes = [P, P, P, I, I, I, Z, Z, I, F, F, I, F, I, P, P, P]
    L.bicos_agree_stage_device.restype = I
    L.bicos_match_plan.argtypes = [P, P, P, I, I, I, Z, Z, I, ctypes.POINTER(BicosConfig), I]
    L.bicos_match_plan.restype = I
    L.bicos_search_packed.argtypes = [P, I, I, I, I, I, I]
    L.bicos_search_packed.restype = I
    L.bicos_search_packed_product.argtypes = [I]
    L.bicos_search_packed_product.restype = I
    L.bicos_agree_kernel.argtypes = [P, P, I, Z, Z, I]
    L.bicos_agree_kernel.restype = I
    L.bicos_transform_kernel.argtypes = [P, P, I, I, I, Z, Z, I, I, I]
    L.bicos_transform_kernel.restype = I
    L.bicos_search_agree_device.argtypes = [P, P, P, P, P, I, I, I, Z, Z, I,
                                            ctypes.POINTER(BicosConfig), I, P, P, P]
    L.bicos_search_agree_device.restype = I
    L.bicos_match_device_range.argtypes = [P, P, P, I, I, I, Z, Z, I, ctypes.POINTER(BicosConfig),
                                           I, I, I, P, P, P]
    L.bicos_match_device_range.restype = I
    L.bicos_match_host_range.argtypes = [P, PP, PP, I, I, I, Z, I, ctypes.POINTER(BicosConfig), I,
                                         I, I, P, P]
    L.bicos_match_host_range.restype = I
    L.bicos_search_device_range.argtypes = [P, P, P, I, I, I, I, I, I, I, P, P]
    L.bicos_search_device_range.restype = I
    PD = ctypes.POINTER(ctypes.c_double)
    L.bicos_reproject_device.argtypes = [P, P, I, I, I, PD, I, P, P, P, Z, P, P]
    L.bicos_reproject_device.restype = I
    L.bicos_reproject_host.argtypes = [P, P, I, I, I, PD, I, P, P, P, Z, P]
    L.bicos_reproject_host.restype = I
    L.bicos_reproject_segment.argtypes = []
    L.bicos_reproject_segment.restype = I
    L.bicos_speckle_device.argtypes = [P, P, I, I, I, I, F, I, P, P, P, P]
    L.bicos_speckle_device.restype = I
    L.bicos_speckle_host.argtypes = [P, P, I, I, I, I, F, I, P, P, P]
    L.bicos_speckle_host.restype = I
    L.bicos_speckle_tile.argtypes = [PI, PI]
    L.bicos_speckle_tile.restype = I
    L.bicos_rectify_maps_device.argtypes = [PD, PD, I, PD, PD, I, I, I, P, P, P]
    L.bicos_rectify_maps_device.restype = I
    L.bicos_rectify_maps_host.argtypes = [PD, PD, I, PD, PD, I, I, I, P, P]
    L.bicos_rectify_maps_host.restype = I
    L.bicos_rectify_device.argtypes = [P, P, I, I, I, Z, Z, I, P, P, Z, I, I, P, Z, Z, I, P, P]
    L.bicos_rectify_device.restype = I
    L.bicos_rectify_host.argtypes = [P, PP, I, I, I, Z, I, P, P, Z, I, I, PP, Z, I, P]
    L.bicos_rectify_host.restype = I
    L.bicos_rectify_tile.argtypes = [PI, PI]
    L.bicos_rectify_tile.restype = I
    L.bicos_median_device.argtypes = [P, P, I, I, I, I, I, I, P, P, P]
    L.bicos_median_device.restype = I
    L.bicos_median_host.argtypes = [P, P, I, I, I, I, I, I, P, P]
    L.bicos_median_host.restype = I
    L.bicos_median_tile.argtypes = [PI, PI]
    L.bicos_median_tile.restype = I
    L.bicos_normals_device.argtypes = [P, P, I, I, I, PD, I, I, F, I, P, P, Z, P, P, P]
    L.bicos_normals_device.restype = I
    L.bicos_normals_host.argtypes = [P, P, I, I, I, PD, I, I, F, I, P, P, Z, P, P]
    L.bicos_normals_host.restype = I
    L.bicos_normals_tile.argtypes = [PI, PI]
    L.bicos_normals_tile.restype = I
    L.bicos_mesh_device.argtypes = [P, P, I, I, I, PD, I, F, P, P, Z, P, P, Z, P, P, P]
    L.bicos_mesh_device.restype = I
    L.bicos_mesh_host.argtypes = [P, P, I, I, I, PD, I, F, P, P, Z, P, P, Z, P, P]
    L.bicos_mesh_host.restype = I
    L.bicos_mesh_segment.argtypes = []
    L.bicos_mesh_segment.restype = I
    project_args = [P, P, Z, PD, PD, PD, PD, I, I, I, I, F, P, I, I, Z, I, P, P, P, P, P, P, P]
    L.bicos_project_device.argtypes = project_args + [P]
    L.bicos_project_device.restype = I
    L.bicos_project_host.argtypes = project_args
    L.bicos_project_host.restype = I
    L.bicos_project_group.argtypes = []
    L.bicos_project_group.restype = I
    L.bicos_search_device_guided.argtypes = [P, P, P, I, I, I, I, I, I, I, P, Z, P, P]
    L.bicos_search_device_guided.restype = I
    L.bicos_match_device_guided.argtypes = [P, P, P, I, I, I, Z, Z, I,
                                            ctypes.POINTER(BicosConfig), I, I, I, P, Z, P, P, P]
    L.bicos_match_device_guided.restype = I
    L.bicos_match_host_guided.argtypes = [P, PP, PP, I, I, I, Z, I, ctypes.POINTER(BicosConfig), I,
                                          I, I, P, Z, P, P]
    L.bicos_match_host_guided.restype = I
    L.bicos_guide_device.argtypes = [P, P, I, I, I, I, I, I, I, I, I, I, I, P, Z, P, P]
    L.bicos_guide_device.restype = I
    L.bicos_guide_host.argtypes = [P, P, I, I, I, I, I, I, I, I, I, I, I, P, Z, P]
    L.bicos_guide_host.restype = I
    L.bicos_pool_device.argtypes = [P, P, I, I, I, Z, Z, I, I, P, Z, Z, P]
    L.bicos_pool_device.restype = I
    L.bicos_pool_host.argtypes = [P, PP, I, I, I, Z, I, I, PP, Z]
    L.bicos_pool_host.restype = I
    L.bicos_pool_tile.argtypes = [PI, PI]
    L.bicos_pool_tile.restype = I
    L.bicos_pool_kernel.argtypes = [P, Z, Z, I, P, Z, Z]
    L.bicos_pool_kernel.restype = I
    L.bicos_match_device_pyramid.argtypes = [P, P, P, I, I, I, Z, Z, I,
                                             ctypes.POINTER(BicosConfig), I, I, I, I, I, I, I, I,
                                             P, P, P, P, P, P]
    L.bicos_match_device_pyramid.restype = I
    L.bicos_match_host_pyramid.argtypes = [P, PP, PP, I, I, I, Z, I, ctypes.POINTER(BicosConfig),
                                           I, I, I, I, I, I, I, I, P, P, P, P, P]
    L.bicos_match_host_pyramid.restype = I
    L.bicos_pyramid_window.argtypes = [I, I, I, PI, PI]
    L.bicos_pyramid_window.restype = I
    L.bicos_build_info.restype = ctypes.c_char_p
    L.bicos_build_info.argtypes = []
    _lib = L
    return L


def check_disparity_range(rng):
    """None, or (lo, hi) as two ints with lo <= hi (ValueError otherwise): the inclusive
    disparity window of the *_range entry points (include/bicos_c.h)."""
    if rng is None:
        return None
    try:
        lo, hi = rng
    except (TypeError, ValueError):
        raise ValueError("disparity_range must be None or a pair (lo, hi)") from None
    for v in (lo, hi):
        if isinstance(v, bool) or not hasattr(v, "__index__"):
            raise ValueError("disparity_range bounds must be integers, got %r" % (v,))
    lo, hi = int(lo), int(hi)
    if lo > hi:
        raise ValueError("disparity_range: lo %d exceeds hi %d" % (lo, hi))
    if not (-2 ** 31 <= lo and hi < 2 ** 31):
        raise ValueError("disparity_range bounds must fit a C int")
    return lo, hi


def check_guide_shape(shape, rows, cols):
    """A guide's shape must be (rows, cols, 2) (ValueError otherwise): one int16 pair (lo, hi)
    per left pixel (include/bicos_c.h "disparity guide")."""
    if tuple(shape) != (rows, cols, 2):
        raise ValueError("guide must have shape (%d, %d, 2): one (lo, hi) pair per pixel, got %s"
                         % (rows, cols, tuple(shape)))


def guide_window(rng):
    """The global window of a guided call: check_disparity_range's pair, or no global bound
    (INT_MIN, INT_MAX) for None."""
    rng = check_disparity_range(rng)
    return (INT_MIN, INT_MAX) if rng is None else rng


def guide_params(radius, spread=0, scale=1, fallback=None):
    """(radius, spread, scale, fallback_lo, fallback_hi) as the bicos_guide_* entries take them
    (ValueError for what they would refuse): radius 0..32767, spread 0..7, scale 1..8, fallback
    None (every disparity, (-32767, 32767)) or a pair of int16 values -- lo > hi is legal and
    means "do not search here"."""
    def integer(v, name, lo, hi):
        if isinstance(v, bool) or not hasattr(v, "__index__"):
            raise ValueError("%s must be an integer, got %r" % (name, v))
        v = int(v)
        if not lo <= v <= hi:
            raise ValueError("%s must lie in [%d, %d], got %d" % (name, lo, hi, v))
        return v

    r = integer(radius, "radius", 0, 32767)
    sp = integer(spread, "spread", 0, 7)
    sc = integer(scale, "scale", 1, 8)
    if fallback is None:
        fallback = (-32767, 32767)
    try:
        flo, fhi = fallback
    except (TypeError, ValueError):
        raise ValueError("fallback must be None or a pair (lo, hi)") from None
    return r, sp, sc, integer(flo, "fallback lo", -32768, 32767), \
        integer(fhi, "fallback hi", -32768, 32767)


def guide_shape(shape, prior_shape, scale):
    """(rows, cols) of the guide to build: `shape`, or the prior's size times scale."""
    if shape is None:
        return int(prior_shape[0]) * scale, int(prior_shape[1]) * scale
    try:
        rows, cols = shape
        rows, cols = int(rows), int(cols)
    except (TypeError, ValueError):
        raise ValueError("shape must be None or a pair (rows, cols)") from None
    if rows < 0 or cols < 0 or rows * cols >= 2 ** 31:
        raise ValueError("shape must be non-negative with fewer than 2^31 pixels, got %r" % (shape,))
    return rows, cols


def pool_scale(scale):
    """The pooling factor as the bicos_pool_* entries take it: an integer in 2..8 (ValueError
    otherwise)."""
    if isinstance(scale, bool) or not hasattr(scale, "__index__"):
        raise ValueError("scale must be an integer, got %r" % (scale,))
    scale = int(scale)
    if not 2 <= scale <= 8:
        raise ValueError("scale must lie in [2, 8], got %d" % scale)
    return scale


def pool_shape(rows, cols, scale):
    """(prows, pcols) = (rows // scale, cols // scale) of a pooled image (ValueError for an
    image smaller than scale x scale)."""
    if rows < scale or cols < scale:
        raise ValueError("a %d x %d image is smaller than scale x scale (%d)" % (rows, cols, scale))
    return rows // scale, cols // scale


def pool_tile():
    """(rows, cols) of the output tile one workgroup pools (bicos_pool_tile)."""
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    lib().bicos_pool_tile(ctypes.byref(r), ctypes.byref(c))
    return r.value, c.value


def pyramid_window(rng, scale):
    """The coarse match's window of a pyramid match: (floor(lo / scale), ceil(hi / scale))
    (include/bicos_c.h "pyramid match")."""
    lo, hi = rng
    return lo // scale, -((-hi) // scale)


def pyramid_params(disparity_range, scale=2, radius=2, spread=1, fallback=None):
    """((lo, hi), scale, radius, spread, fallback_lo, fallback_hi) as the *_pyramid entries take
    them (ValueError for what they would refuse): disparity_range is required, scale 2..8,
    radius and spread as guide_params; fallback None is the global window clamped to +-32767."""
    rng = check_disparity_range(disparity_range)
    if rng is None:
        raise ValueError("match_pyramid needs cfg.disparity_range: the global window of both levels")
    sc = pool_scale(scale)
    if fallback is None:
        fallback = (max(rng[0], -32767), min(rng[1], 32767))
    r, sp, _, flo, fhi = guide_params(radius, spread, sc, fallback)
    return rng, sc, r, sp, flo, fhi


def reproject_q(Q):
    """The 16 doubles of a 4x4 matrix (anything numpy reads as one), row-major, as the
    ctypes array the bicos_reproject_* entries take (ValueError otherwise)."""
    import numpy as np
    q = np.asarray(Q, dtype=np.float64)
    if q.shape != (4, 4):
        raise ValueError("Q must be a 4x4 matrix, got shape %s" % (q.shape,))
    return (ctypes.c_double * 16)(*q.ravel().tolist())


def reproject_flags(allow_negative_z: bool, sentinel: bool) -> int:
    return (REPROJECT_ALLOW_NEGATIVE_Z if allow_negative_z else 0) | \
        (REPROJECT_F32_SENTINEL if sentinel else 0)


def speckle_params(max_size, max_diff):
    """(int max_size, float max_diff) as the bicos_speckle_* entries take them (ValueError for
    what they would refuse: a negative max_size, a negative or NaN max_diff)."""
    size, diff = int(max_size), float(max_diff)
    if size != max_size or size < 0 or size > 2 ** 31 - 1:
        raise ValueError("max_size must be an integer in [0, 2^31 - 1], got %r" % (max_size,))
    if not diff >= 0:
        raise ValueError("max_diff must be >= 0 and not NaN, got %r" % (max_diff,))
    return size, diff


def speckle_tile():
    """(rows, cols) of the tile one workgroup labels (bicos_speckle_tile)."""
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    lib().bicos_speckle_tile(ctypes.byref(r), ctypes.byref(c))
    return r.value, c.value


def median_params(ksize, fill_min):
    """(int ksize, int fill_min) as the bicos_median_* entries take them (ValueError for what
    they would refuse: a ksize other than 3 or 5, a fill_min outside 0 .. ksize * ksize)."""
    try:
        k, f = int(ksize), int(fill_min)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("ksize and fill_min must be integers, got %r, %r" % (ksize, fill_min))
    if k != ksize or k not in (3, 5):
        raise ValueError("ksize must be 3 or 5, got %r" % (ksize,))
    if f != fill_min or f < 0 or f > k * k:
        raise ValueError("fill_min must be an integer in [0, %d], got %r" % (k * k, fill_min))
    return k, f


def median_tile():
    """(rows, cols) of the output tile of one workgroup (bicos_median_tile)."""
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    lib().bicos_median_tile(ctypes.byref(r), ctypes.byref(c))
    return r.value, c.value


def normals_flags(allow_negative_z: bool, sentinel: bool) -> int:
    return (NORMALS_ALLOW_NEGATIVE_Z if allow_negative_z else 0) | \
        (NORMALS_F32_SENTINEL if sentinel else 0)


def mesh_flags(allow_negative_z: bool, sentinel: bool) -> int:
    return (MESH_ALLOW_NEGATIVE_Z if allow_negative_z else 0) | \
        (MESH_F32_SENTINEL if sentinel else 0)


def mesh_max_diff(max_diff) -> float:
    """float max_diff as the bicos_mesh_* entries take it (ValueError for what they would
    refuse: a negative or NaN value, or no number at all)."""
    try:
        diff = float(max_diff)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("max_diff must be a number, got %r" % (max_diff,))
    if not diff >= 0:
        raise ValueError("max_diff must be >= 0 and not NaN, got %r" % (max_diff,))
    return diff


def mesh_quads(rows: int, cols: int) -> int:
    """(rows - 1) * (cols - 1): the quads of a map, 0 without a second row or column"""
    return 0 if rows < 2 or cols < 2 else (rows - 1) * (cols - 1)


def project_camera(K, D=None, R=None, t=None):
    """One camera as the bicos_project_* entries take it: (R, t, K, D, nd) with ctypes double
    arrays (R, t and D None for the identity, zero and no distortion). K is 3x3, D None or 0, 4,
    5 or 8 coefficients, R None or 3x3, t None or 3 values. ValueError for other shapes; the
    values are checked by the library."""
    import numpy as np

    def arr(a, name, size, shape=None):
        a = np.asarray(a, dtype=np.float64)
        if a.size != size or (shape is not None and a.shape != shape):
            raise ValueError("%s must have %s, got shape %s"
                             % (name, "shape %s" % (shape,) if shape else "%d values" % size,
                                a.shape))
        return (ctypes.c_double * size)(*a.ravel().tolist())

    k = arr(K, "K", 9, (3, 3))
    d = np.zeros(0) if D is None else np.asarray(D, dtype=np.float64).ravel()
    if d.size not in (0, 4, 5, 8):
        raise ValueError("D must hold 0, 4, 5 or 8 coefficients, got %d" % d.size)
    dd = (ctypes.c_double * d.size)(*d.tolist()) if d.size else None
    r = None if R is None else arr(R, "R", 9, (3, 3))
    tt = None if t is None else arr(t, "t", 3)
    return r, tt, k, dd, int(d.size)


def project_params(size, splat, tol, fill):
    """(int rows, int cols, int splat, float tol, int fill) as the bicos_project_* entries take
    them (ValueError for what they would refuse but a fill beyond the image type, which the
    library sees)."""
    try:
        rows, cols = size
        rows, cols = int(rows), int(cols)
    except (TypeError, ValueError):
        raise ValueError("size must be a pair (rows, cols)") from None
    if rows < 0 or cols < 0 or rows * cols >= 2 ** 31:
        raise ValueError("size must not be negative, with fewer than 2^31 pixels, got %r"
                         % (size,))
    try:
        s, f, tl = int(splat), int(fill), float(tol)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("splat, tol and fill must be numbers, got %r, %r, %r"
                         % (splat, tol, fill)) from None
    if s != splat or not 0 <= s <= PROJECT_MAX_SPLAT:
        raise ValueError("splat must be an integer 0 .. %d, got %r" % (PROJECT_MAX_SPLAT, splat))
    if not tl >= 0:
        raise ValueError("tol must be >= 0 and not NaN, got %r" % (tol,))
    if f != fill or f < 0:
        raise ValueError("fill must be a non-negative integer, got %r" % (fill,))
    return rows, cols, s, tl, f


def project_group() -> int:
    """points per workgroup of the projection's point launches"""
    return int(lib().bicos_project_group())


def normals_params(radius, max_diff, min_points):
    """(int radius, float max_diff, int min_points) as the bicos_normals_* entries take them
    (ValueError for what they would refuse: a radius outside 1 .. 4, a negative or NaN
    max_diff, a min_points outside 3 .. (2 * radius + 1)^2)."""
    try:
        r, m, diff = int(radius), int(min_points), float(max_diff)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("radius and min_points must be integers and max_diff a number, got "
                         "%r, %r, %r" % (radius, min_points, max_diff))
    if r != radius or r < 1 or r > NORMALS_MAX_RADIUS:
        raise ValueError("radius must be an integer in [1, %d], got %r"
                         % (NORMALS_MAX_RADIUS, radius))
    if not diff >= 0:
        raise ValueError("max_diff must be >= 0 and not NaN, got %r" % (max_diff,))
    if m != min_points or m < 3 or m > (2 * r + 1) ** 2:
        raise ValueError("min_points must be an integer in [3, %d], got %r"
                         % ((2 * r + 1) ** 2, min_points))
    return r, diff, m


def normals_tile():
    """(rows, cols) of the tile of the dense map one workgroup stages (bicos_normals_tile)."""
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    lib().bicos_normals_tile(ctypes.byref(r), ctypes.byref(c))
    return r.value, c.value


def rectify_tile():
    """(rows, cols) of the output tile one workgroup remaps (bicos_rectify_tile)."""
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    lib().bicos_rectify_tile(ctypes.byref(r), ctypes.byref(c))
    return r.value, c.value


def rectify_camera(K, D, R, P, size):
    """The calibration of one camera as the bicos_rectify_maps_* entries take it: (K, D, nd, R,
    P, p_cols, rows, cols) with ctypes double arrays (R None for the identity). K is 3x3, D
    None or 0, 4, 5 or 8 coefficients, R None or 3x3, P 3x3 or 3x4, size (rows, cols).
    ValueError for other shapes; the values are checked by the library."""
    import numpy as np

    def arr(a, name, shapes):
        a = np.asarray(a, dtype=np.float64)
        if a.shape not in shapes:
            raise ValueError("%s must have shape %s, got %s"
                             % (name, " or ".join(str(s) for s in shapes), a.shape))
        return (ctypes.c_double * a.size)(*a.ravel().tolist())

    k = arr(K, "K", ((3, 3),))
    d = np.zeros(0) if D is None else np.asarray(D, dtype=np.float64).ravel()
    if d.size not in (0, 4, 5, 8):
        raise ValueError("D must hold 0, 4, 5 or 8 coefficients, got %d" % d.size)
    dd = (ctypes.c_double * d.size)(*d.tolist()) if d.size else None
    r = None if R is None else arr(R, "R", ((3, 3),))
    p = np.asarray(P, dtype=np.float64)
    pp = arr(p, "P", ((3, 3), (3, 4)))
    try:
        rows, cols = size
        rows, cols = int(rows), int(cols)
    except (TypeError, ValueError):
        raise ValueError("size must be a pair (rows, cols)") from None
    if rows < 1 or cols < 1 or rows * cols >= 2 ** 31:
        raise ValueError("size must be positive with fewer than 2^31 pixels, got %r" % (size,))
    return k, dd, int(d.size), r, pp, int(p.shape[1]), rows, cols


def check(rc: int, what: str = "bicos") -> None:
    if rc != BICOS_OK:
        msg = lib().bicos_last_error().decode(errors="replace")
        raise BicosError("%s failed (%d): %s" % (what, rc, msg))
