"""pybicos -- drop-in for the reference's Python API (pybicos/__init__.py:1-252).

Same names, argument meaning, return dtypes and error behaviour:
  Config() with nxcorr_threshold / subpixel_step / min_variance / mode /
  precision properties, variant (read-only), set_no_duplicates(),
  set_consistency(max_lr_diff=1, no_dupes=False);
  match(stack0, stack1, cfg=None) -> (disparity, corrmap) numpy copies;
  invalid_disparity(dtype).
Backed by libbicos_amd.so's BICOS_Match (host buffers in, host copies out),
which runs on the gfx950 HIP engine.
"""
from __future__ import annotations

import ctypes
from enum import Enum

import numpy as np

from . import _lib
from ._lib import BicosConfig, BicosResult  # noqa: F401  (re-exported like the reference)

CV_8U, CV_16U, CV_16S, CV_32F, CV_64F = 0, 2, 3, 5, 6


class TransformMode(Enum):
    LIMITED = 0
    FULL = 1


class Precision(Enum):
    SINGLE = 0
    DOUBLE = 1


class VariantType(Enum):
    NO_DUPLICATES = 0
    CONSISTENCY = 1


def _get_cv_type(dtype):
    # reference pybicos/__init__.py:85-97
    if dtype == np.uint8:
        return CV_8U
    elif dtype == np.uint16:
        return CV_16U
    elif dtype == np.int16:
        return CV_16S
    elif dtype == np.float32:
        return CV_32F
    elif dtype == np.float64:
        return CV_64F
    raise ValueError(f"Unsupported numpy dtype: {dtype}")


def _get_np_dtype(cv_type):
    # reference pybicos/__init__.py:99-107
    if cv_type == CV_16S or cv_type == (CV_16S | (1 << 3)):
        return np.int16
    elif cv_type == CV_32F or cv_type == (CV_32F | (1 << 3)):
        return np.float32
    elif cv_type == CV_64F or cv_type == (CV_64F | (1 << 3)):
        return np.float64
    raise ValueError(f"Unsupported OpenCV type: {cv_type}")


class Config:
    """reference pybicos/__init__.py:110-196."""

    def __init__(self):
        self._L = _lib.lib()
        self._c_config = self._L.BICOS_CreateDefaultConfig()
        self._disparity_range = None

    def __del__(self):
        if getattr(self, "_c_config", None):
            self._L.BICOS_FreeConfig(self._c_config)
            self._c_config = None

    @property
    def nxcorr_threshold(self):
        return self._c_config.contents.nxcorr_threshold

    @nxcorr_threshold.setter
    def nxcorr_threshold(self, value):
        self._c_config.contents.nxcorr_threshold = value

    @property
    def subpixel_step(self):
        val = self._c_config.contents.subpixel_step
        return None if val < 0 else val

    @subpixel_step.setter
    def subpixel_step(self, value):
        self._c_config.contents.subpixel_step = -1.0 if value is None else value

    @property
    def min_variance(self):
        val = self._c_config.contents.min_variance
        return None if val < 0 else val

    @min_variance.setter
    def min_variance(self, value):
        self._c_config.contents.min_variance = -1.0 if value is None else value

    @property
    def mode(self):
        return TransformMode(self._c_config.contents.mode)

    @mode.setter
    def mode(self, value):
        self._c_config.contents.mode = value.value if isinstance(value, TransformMode) else value

    @property
    def precision(self):
        return Precision(self._c_config.contents.precision)

    @precision.setter
    def precision(self, value):
        self._c_config.contents.precision = value.value if isinstance(value, Precision) else value

    @property
    def disparity_range(self):
        """An extension (the reference scans whole rows): None, or (lo, hi) -- search only the
        right columns with lo <= left column - right column <= hi, inclusive (include/bicos_c.h
        "disparity range"). Kept beside the C struct, whose layout is the reference's."""
        return self._disparity_range

    @disparity_range.setter
    def disparity_range(self, value):
        self._disparity_range = _lib.check_disparity_range(value)

    @property
    def variant(self):
        if self._c_config.contents.variant_type == VariantType.NO_DUPLICATES.value:
            return "NoDuplicates"
        return {
            "type": "Consistency",
            "max_lr_diff": self._c_config.contents.max_lr_diff,
            "no_dupes": bool(self._c_config.contents.no_dupes),
        }

    def set_no_duplicates(self):
        self._c_config.contents.variant_type = VariantType.NO_DUPLICATES.value

    def set_consistency(self, max_lr_diff=1, no_dupes=False):
        self._c_config.contents.variant_type = VariantType.CONSISTENCY.value
        self._c_config.contents.max_lr_diff = max_lr_diff
        self._c_config.contents.no_dupes = 1 if no_dupes else 0

    def __repr__(self):
        parts = [
            "Config(",
            f"  nxcorr_threshold={self.nxcorr_threshold}",
            f"  subpixel_step={self.subpixel_step}",
            f"  min_variance={self.min_variance}",
            f"  mode={self.mode.name}",
            f"  precision={self.precision.name}",
            f"  variant={self.variant}",
        ] + ([f"  disparity_range={self.disparity_range}"] if self.disparity_range else []) + [
            ")",
        ]
        return "\n".join(parts)


def _marshal(stack):
    k = len(stack)
    data = (ctypes.c_void_p * k)()
    rows = (ctypes.c_int * k)()
    cols = (ctypes.c_int * k)()
    types = (ctypes.c_int * k)()
    keep = []
    for i, img in enumerate(stack):
        img = np.asarray(img)
        if not img.flags["C_CONTIGUOUS"]:
            img = np.ascontiguousarray(img)
        if img.ndim != 2:
            raise ValueError("images must be 2-D (single channel)")
        keep.append(img)
        data[i] = img.ctypes.data_as(ctypes.c_void_p)
        rows[i] = img.shape[0]
        cols[i] = img.shape[1]
        types[i] = _get_cv_type(img.dtype)
    return data, rows, cols, types, keep


def _guide_array(guide, rows, cols):
    """the guide as the host entry reads it: a C-contiguous int16 [rows, cols, 2] array"""
    g = np.asarray(guide)
    if g.dtype != np.int16:
        raise ValueError(f"guide must be an int16 array, got {g.dtype}")
    _lib.check_guide_shape(g.shape, rows, cols)
    return np.ascontiguousarray(g)


def match(stack0, stack1, cfg=None, devices=None, guide=None):
    """reference pybicos/__init__.py:199-244 -> (disparity, corrmap).

    guide (an extension): an int16 array [rows, cols, 2], one disparity window (lo, hi) per
    left pixel (guide_from_disparity builds one from a prior map; include/bicos_c.h "disparity
    guide"); cfg.disparity_range is the global window beside it.

    devices (an extension; the reference is single-GPU): a sequence of GPU indices to split
    the frame's rows over from this process (bicos_match_host_multi: one band per device,
    each uploaded over its own GPU's link); the maps are byte-identical to the one-GPU call.

    Same inputs, outputs, dtypes and errors as the reference wrapper (which goes through
    BICOS_Match: NXC always on, so float32 disparity; corrmap float32, or float64 with
    Precision.DOUBLE). Runs bicos_match_host, which writes the maps straight into the
    returned arrays (no result struct, no extra copies) and overlaps the upload of the
    stacks with the match (include/bicos_c.h)."""
    if stack0 is None or stack1 is None or len(stack0) == 0 or len(stack1) == 0:
        raise ValueError("Empty image stacks")
    if cfg is None:
        cfg = Config()
    L = _lib.lib()
    d0, r0, c0, t0, k0 = _marshal(stack0)
    d1, r1, c1, t1, k1 = _marshal(stack1)
    f = k0[0]
    if len(k0) != len(k1) or any(a.shape != f.shape or a.dtype != f.dtype for a in k0 + k1):
        raise RuntimeError("BICOS matching failed: all images must share size and type "
                           "(and both stacks the same length)")
    rows, cols = f.shape
    ddtype = _get_np_dtype(L.bicos_output_type(cfg._c_config, 1))
    cdtype = np.float64 if cfg._c_config.contents.precision else np.float32
    disparity = np.empty((rows, cols), ddtype)
    corrmap = np.empty((rows, cols), cdtype)
    rng = getattr(cfg, "disparity_range", None)
    if guide is not None:
        if devices is not None and len(list(devices)) > 1:
            raise ValueError("a disparity guide is not supported with several GPUs yet")
        if devices is not None:
            raise ValueError("a guided match runs on the current device: leave devices unset")
        g = _guide_array(guide, rows, cols)
        lo, hi = _lib.guide_window(rng)
        rc = 0
        if rows * cols:
            rc = L.bicos_match_host_guided(None, d0, d1, len(k0), rows, cols, 0, f.dtype.itemsize,
                                           cfg._c_config, 1, lo, hi, g.ctypes.data, cols,
                                           disparity.ctypes.data, corrmap.ctypes.data)
        del k0, k1
        if rc != 0:
            raise RuntimeError("BICOS matching failed: " +
                               L.bicos_last_error().decode(errors="replace"))
        return disparity, corrmap
    if rng is not None and devices is not None and len(list(devices)) > 1:
        raise ValueError("disparity_range is not supported with several GPUs yet")
    if rng is not None:
        if devices is not None and len(list(devices)) == 1:
            raise ValueError("disparity_range runs on the current device: leave devices unset")
        rc = L.bicos_match_host_range(None, d0, d1, len(k0), rows, cols, 0, f.dtype.itemsize,
                                      cfg._c_config, 1, rng[0], rng[1], disparity.ctypes.data,
                                      corrmap.ctypes.data)
    elif devices is None:
        rc = L.bicos_match_host(None, d0, d1, len(k0), rows, cols, 0, f.dtype.itemsize,
                                cfg._c_config, 1, disparity.ctypes.data, corrmap.ctypes.data)
    else:
        devs = [int(d) for d in devices]
        if not devs:
            raise ValueError("devices must name at least one GPU")
        rc = L.bicos_match_host_multi((ctypes.c_int * len(devs))(*devs), len(devs), d0, d1,
                                      len(k0), rows, cols, 0, f.dtype.itemsize, cfg._c_config, 1,
                                      disparity.ctypes.data, corrmap.ctypes.data)
    del k0, k1
    if rc != 0:
        raise RuntimeError("BICOS matching failed: " + L.bicos_last_error().decode(errors="replace"))
    return disparity, corrmap


def reproject(disparity, Q, allow_negative_z=False, sentinel=True):
    """An extension (the reference reprojects in its command-line tool only, src/cli.cpp:238):
    a disparity map from match() -- int16 or float32, [rows, cols] -- through the rig's 4x4
    matrix Q to the kept 3-D points, a float32 [kept, 3] array in row-major pixel order
    (bicos_reproject_host, include/bicos_c.h "reprojection": on the GPU, bit for bit the
    double-precision formula). Invalid pixels (int16 -32768, NaN, and with `sentinel` the
    float -32768.0 of a match without subpixel step), points that are not finite and, unless
    allow_negative_z, points with Z < 0 are left out."""
    d = np.ascontiguousarray(disparity)
    if d.ndim != 2:
        raise ValueError("disparity map must be 2-D")
    if d.dtype != np.int16 and d.dtype != np.float32:
        raise ValueError(f"Unsupported disparity dtype: {d.dtype}")
    rows, cols = d.shape
    q = _lib.reproject_q(Q)
    points = np.empty((max(rows * cols, 1), 3), np.float32)
    counts = (ctypes.c_uint32 * 4)()
    L = _lib.lib()
    rc = L.bicos_reproject_host(None, d.ctypes.data, _get_cv_type(d.dtype), rows, cols, q,
                                _lib.reproject_flags(allow_negative_z, sentinel), None,
                                points.ctypes.data, None, rows * cols, counts)
    if rc != 0:
        raise RuntimeError("BICOS reprojection failed: " +
                           L.bicos_last_error().decode(errors="replace"))
    return points[:counts[0]].copy()


def normals(disparity, Q, radius=2, max_diff=1.0, min_points=3, allow_negative_z=False,
            sentinel=True, index=None):
    """An extension (the reference has no such step): one unit surface normal per pixel of a
    disparity map from match() -- int16 or float32, [rows, cols] --, oriented towards the
    camera: the least-squares plane of the disparities over the (2 * radius + 1)^2 window in
    (column, row, disparity), carried through the rig's 4x4 matrix Q (bicos_normals_host,
    include/bicos_c.h "surface normals": on the GPU, bit for bit the double-precision text). A
    window pixel takes part if it is valid and within max_diff of the centre's disparity.
    Returns the float32 [rows, cols, 3] map, or with `index` (int32 pixel indices row * cols +
    col, as the reprojection orders its points) the float32 [len(index), 3] list. Three NaNs
    where reproject() with the same flags keeps no point, where fewer than min_points pixels
    take part or where they are collinear. Meant for subpixel (float32) maps: integer
    disparities stair-step."""
    d = np.ascontiguousarray(disparity)
    if d.ndim != 2:
        raise ValueError("disparity map must be 2-D")
    if d.dtype != np.int16 and d.dtype != np.float32:
        raise ValueError(f"Unsupported disparity dtype: {d.dtype}")
    rows, cols = d.shape
    q = _lib.reproject_q(Q)
    r, diff, m = _lib.normals_params(radius, max_diff, min_points)
    flags = _lib.normals_flags(allow_negative_z, sentinel)
    L = _lib.lib()
    if index is None:
        out = np.empty((rows, cols, 3), np.float32)
        if rows * cols == 0:
            return out
        rc = L.bicos_normals_host(None, d.ctypes.data, _get_cv_type(d.dtype), rows, cols, q,
                                  flags, r, diff, m, out.ctypes.data, None, 0, None, None)
    else:
        idx = np.ascontiguousarray(index, dtype=np.int32)
        if idx.ndim != 1:
            raise ValueError("index must be 1-D")
        out = np.full((idx.shape[0], 3), np.nan, np.float32)
        if rows * cols == 0 or idx.shape[0] == 0:
            return out
        rc = L.bicos_normals_host(None, d.ctypes.data, _get_cv_type(d.dtype), rows, cols, q,
                                  flags, r, diff, m, None, idx.ctypes.data, idx.shape[0],
                                  out.ctypes.data, None)
    if rc != 0:
        raise RuntimeError("BICOS normals failed: " +
                           L.bicos_last_error().decode(errors="replace"))
    return out


def mesh(disparity, Q, max_diff=1.0, allow_negative_z=False, sentinel=True):
    """An extension (the reference has no such step): a disparity map from match() -- int16 or
    float32, [rows, cols] -- triangulated (bicos_mesh_host, include/bicos_c.h "mesh": on the
    GPU, exact). Returns (points, triangles): the float32 [kept, 3] points of reproject() with
    the same flags, and int32 [T, 3] vertex numbers into them. Every 2x2 block of pixels gives
    at most two triangles, split along the diagonal with the smaller disparity step; a triangle
    is emitted where its three corners are kept points and every edge joins disparities that
    differ by at most max_diff."""
    d = np.ascontiguousarray(disparity)
    if d.ndim != 2:
        raise ValueError("disparity map must be 2-D")
    if d.dtype != np.int16 and d.dtype != np.float32:
        raise ValueError(f"Unsupported disparity dtype: {d.dtype}")
    rows, cols = d.shape
    q = _lib.reproject_q(Q)
    diff = _lib.mesh_max_diff(max_diff)
    tcap = 2 * _lib.mesh_quads(rows, cols)
    points = np.empty((max(rows * cols, 1), 3), np.float32)
    triangles = np.empty((max(tcap, 1), 3), np.int32)
    counts = (ctypes.c_uint32 * 4)()
    mesh_counts = (ctypes.c_uint32 * 4)()
    L = _lib.lib()
    rc = L.bicos_mesh_host(None, d.ctypes.data, _get_cv_type(d.dtype), rows, cols, q,
                           _lib.mesh_flags(allow_negative_z, sentinel), diff, points.ctypes.data,
                           None, rows * cols, counts, triangles.ctypes.data, tcap, mesh_counts,
                           None)
    if rc != 0:
        raise RuntimeError("BICOS mesh failed: " + L.bicos_last_error().decode(errors="replace"))
    return points[:counts[0]].copy(), triangles[:mesh_counts[0]].copy()


PROJECT_OUTPUTS = ("uv", "depth", "cls", "tex", "depth_map", "index_map", "counts")


def project(points, K, size=None, D=None, R=None, t=None, splat=0, tol=float("inf"), image=None,
            fill=0, outputs=None):
    """An extension (the reference has no such step): float32 points [count, 3] in the frame of
    Q -- reproject()'s or mesh()'s list, or an xyz map reshaped to one -- projected into the
    camera Pc = R*P + t, K, D with an image of size = (rows, cols) (bicos_project_host,
    include/bicos_c.h "projection": on the GPU, exact). Returns a dict of the `outputs` asked
    for among uv [count, 2] float32, depth [count] float32, cls [count] uint8 (0 visible,
    1 occluded, 2 outside, 3 behind, 4 invalid), tex [count, channels] of the image's dtype,
    depth_map / index_map [rows, cols] float32 / int32 and counts uint32 [5]; the default is
    uv, depth, cls, counts and, with an image, tex. `image`: uint8 or uint16, [rows, cols] or
    [rows, cols, 3]; `size` defaults to its shape. A point covers (2*splat+1)^2 pixels of the
    z-buffer and is occluded where !(depth <= nearest depth at its pixel + tol)."""
    pts = np.ascontiguousarray(points)
    if pts.dtype != np.float32 or pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be a float32 array [count, 3]")
    count = pts.shape[0]
    img, depth, channels, pitch = None, 1, 1, 0
    if image is not None:
        img = np.ascontiguousarray(image)
        if img.dtype != np.uint8 and img.dtype != np.uint16:
            raise ValueError(f"Unsupported image dtype: {img.dtype}")
        if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3)):
            raise ValueError("image must be [rows, cols] or [rows, cols, 3]")
        channels = img.shape[2] if img.ndim == 3 else 1
        if size is None:
            size = img.shape[:2]
        if tuple(img.shape[:2]) != tuple(size):
            raise ValueError("image must have the camera's size %s" % (tuple(size),))
        depth, pitch = img.itemsize, img.shape[1] * channels
    if size is None:
        raise ValueError("size = (rows, cols) is required without an image")
    rows, cols, splat, tol, fill = _lib.project_params(size, splat, tol, fill)
    r, tt, k, d, nd = _lib.project_camera(K, D, R, t)
    if outputs is None:
        outputs = ("uv", "depth", "cls", "counts") + (("tex",) if img is not None else ())
    unknown = [n for n in outputs if n not in PROJECT_OUTPUTS]
    if unknown:
        raise ValueError("unknown outputs %r (of %r)" % (unknown, PROJECT_OUTPUTS))
    if "tex" in outputs and img is None:
        raise ValueError("tex requires an image")
    spec = {"uv": ((count, 2), np.float32), "depth": ((count,), np.float32),
            "cls": ((count,), np.uint8),
            "tex": ((count, channels), img.dtype if img is not None else np.uint8),
            "depth_map": ((rows, cols), np.float32), "index_map": ((rows, cols), np.int32),
            "counts": ((5,), np.uint32)}
    res = {n: np.empty(*spec[n]) for n in PROJECT_OUTPUTS if n in outputs}
    if not res:
        raise ValueError("at least one output is required")
    args = [res[n].ctypes.data if n in res and res[n].size else None for n in PROJECT_OUTPUTS]
    if all(a is None for a in args):  # nothing but empty outputs: nothing to do
        return res
    L = _lib.lib()
    rc = L.bicos_project_host(None, pts.ctypes.data if count else None, count, r, tt, k, d, nd,
                              rows, cols, splat, tol,
                              img.ctypes.data if img is not None and img.size else None, depth,
                              channels, pitch, fill, *args)
    if rc != 0:
        raise RuntimeError("BICOS project failed: " + L.bicos_last_error().decode(errors="replace"))
    return res


def filter_speckles(disparity, max_size, max_diff=1.0, sentinel=True):
    """An extension (the reference has no such step; cv2.filterSpeckles is the CPU
    counterpart): removes from a disparity map of match() -- int16 or float32, [rows, cols] --
    every 4-connected component of similar disparity (neighbours differing by at most
    max_diff) that has at most max_size pixels (bicos_speckle_host, include/bicos_c.h "speckle
    filter": on the GPU, exact). Removed pixels become invalid: int16 -32768, float NaN, or
    with `sentinel` the float -32768.0 of a match without subpixel step, which is then also
    invalid on input. Returns (filtered, stats) with stats = dict(kept, removed, invalid,
    removed_components); the input is left as it is."""
    d = np.ascontiguousarray(disparity)
    if d.ndim != 2:
        raise ValueError("disparity map must be 2-D")
    if d.dtype != np.int16 and d.dtype != np.float32:
        raise ValueError(f"Unsupported disparity dtype: {d.dtype}")
    size, diff = _lib.speckle_params(max_size, max_diff)
    rows, cols = d.shape
    out = np.empty_like(d)
    counts = (ctypes.c_uint32 * 4)()
    L = _lib.lib()
    rc = L.bicos_speckle_host(None, d.ctypes.data, _get_cv_type(d.dtype), rows, cols, size, diff,
                              _lib.SPECKLE_F32_SENTINEL if sentinel else 0, out.ctypes.data,
                              None, counts)
    if rc != 0:
        raise RuntimeError("BICOS speckle filter failed: " +
                           L.bicos_last_error().decode(errors="replace"))
    return out, dict(kept=counts[0], removed=counts[1], invalid=counts[2],
                     removed_components=counts[3])


def rectify_maps(K, D, R, P, size):
    """An extension (the reference starts at rectified imagery): the float32 lookup maps
    (map_x, map_y), each [rows, cols] for size = (rows, cols), of one camera from its
    calibration -- K 3x3, D None or 4, 5 or 8 coefficients, R None or 3x3, P 3x3 or 3x4, what
    cv2.stereoRectify returns -- in the model of cv2.initUndistortRectifyMap
    (bicos_rectify_maps_host, include/bicos_c.h "rectification": on the GPU, in double)."""
    k, d, nd, r, p, p_cols, rows, cols = _lib.rectify_camera(K, D, R, P, size)
    map_x = np.empty((rows, cols), np.float32)
    map_y = np.empty((rows, cols), np.float32)
    L = _lib.lib()
    rc = L.bicos_rectify_maps_host(k, d, nd, r, p, p_cols, rows, cols, map_x.ctypes.data,
                                   map_y.ctypes.data)
    if rc != 0:
        raise RuntimeError("BICOS rectification maps failed: " +
                           L.bicos_last_error().decode(errors="replace"))
    return map_x, map_y


def rectify(stack, map_x, map_y, border=0):
    """An extension: the images of `stack` -- a list of 2-D uint8 or uint16 arrays of one size,
    or one [n, rows, cols] array -- remapped bilinearly through the float32 maps of absolute
    source coordinates (rectify_maps) to the maps' size; pixels that fall outside the source
    get `border` (bicos_rectify_host, include/bicos_c.h "rectification": on the GPU, all images
    through one computation of the taps). Returns (rectified, valid): an [n, rows, cols] array of
    the input dtype, ready for match(), and a uint8 [rows, cols] array that is 1 where every
    contributing tap lies in the source."""
    imgs = [np.ascontiguousarray(im) for im in stack]
    if not imgs:
        raise ValueError("Empty image stack")
    f = imgs[0]
    if f.ndim != 2 or f.dtype not in (np.uint8, np.uint16):
        raise ValueError("images must be 2-D uint8 or uint16 arrays")
    if any(im.shape != f.shape or im.dtype != f.dtype for im in imgs):
        raise ValueError("all images must share size and type")
    mx = np.ascontiguousarray(map_x, dtype=np.float32)
    my = np.ascontiguousarray(map_y, dtype=np.float32)
    if mx.ndim != 2 or mx.shape != my.shape or mx.size == 0:
        raise ValueError("map_x and map_y must be non-empty 2-D arrays of one shape")
    n = len(imgs)
    rows, cols = mx.shape
    out = np.empty((n, rows, cols), f.dtype)
    valid = np.empty((rows, cols), np.uint8)
    src = (ctypes.c_void_p * n)(*[im.ctypes.data for im in imgs])
    dst = (ctypes.c_void_p * n)(*[out[t].ctypes.data for t in range(n)])
    L = _lib.lib()
    rc = L.bicos_rectify_host(None, src, n, f.shape[0], f.shape[1], 0, f.dtype.itemsize,
                              mx.ctypes.data, my.ctypes.data, 0, rows, cols, dst, 0, int(border),
                              valid.ctypes.data)
    if rc != 0:
        raise RuntimeError("BICOS rectification failed: " +
                           L.bicos_last_error().decode(errors="replace"))
    return out, valid


def median_filter(disparity, ksize=3, fill_min=0, sentinel=True):
    """An extension (the reference has no such step; cv2.medianBlur is the CPU counterpart,
    which knows nothing of invalid pixels): the ksize x ksize (3 or 5) median filter of a
    disparity map of match() -- int16 or float32, [rows, cols] -- over the valid values of each
    pixel's window, clipped at the border (bicos_median_host, include/bicos_c.h "median
    filter": on the GPU, exact). Invalid pixels (int16 -32768, float NaN, and with `sentinel`
    the float -32768.0 of a match without subpixel step) never enter a median; one whose
    window holds at least fill_min > 0 valid values is filled with their median, every other
    one keeps its bits. Returns (filtered, stats) with stats = dict(unchanged, changed, filled,
    invalid); the input is left as it is."""
    d = np.ascontiguousarray(disparity)
    if d.ndim != 2:
        raise ValueError("disparity map must be 2-D")
    if d.dtype != np.int16 and d.dtype != np.float32:
        raise ValueError(f"Unsupported disparity dtype: {d.dtype}")
    k, fill = _lib.median_params(ksize, fill_min)
    rows, cols = d.shape
    out = np.empty_like(d)
    counts = (ctypes.c_uint32 * 4)()
    L = _lib.lib()
    rc = L.bicos_median_host(None, d.ctypes.data, _get_cv_type(d.dtype), rows, cols, k, fill,
                             _lib.MEDIAN_F32_SENTINEL if sentinel else 0, out.ctypes.data, counts)
    if rc != 0:
        raise RuntimeError("BICOS median filter failed: " +
                           L.bicos_last_error().decode(errors="replace"))
    return out, dict(unchanged=counts[0], changed=counts[1], filled=counts[2], invalid=counts[3])


def guide_from_disparity(prior, radius, spread=0, scale=1, fallback=None, shape=None,
                         sentinel=True):
    """An extension: the guide of match(guide=) -- an int16 array [rows, cols, 2] of disparity
    windows (lo, hi) -- from a prior disparity map, int16 or float32 [prows, pcols], e.g. the
    map of a stack pooled by 2 with scale=2 (bicos_guide_host, include/bicos_c.h "disparity
    guide": on the GPU, integer-exact). The output pixel (r, c) looks at the valid prior values
    of the (2 spread + 1)^2 window around (r // scale, c // scale): lo = scale * floor(min) -
    radius, hi = scale * ceil(max) + scale - 1 + radius; where there is none, `fallback` (None:
    every disparity; lo > hi: do not search there). shape: (rows, cols), default the prior's
    size times scale. Returns (guide, stats) with stats = dict(from_prior, fallback)."""
    d = np.ascontiguousarray(prior)
    if d.ndim != 2:
        raise ValueError("prior map must be 2-D")
    if d.dtype != np.int16 and d.dtype != np.float32:
        raise ValueError(f"Unsupported prior dtype: {d.dtype}")
    r, sp, sc, flo, fhi = _lib.guide_params(radius, spread, scale, fallback)
    rows, cols = _lib.guide_shape(shape, d.shape, sc)
    out = np.empty((rows, cols, 2), np.int16)
    counts = (ctypes.c_uint32 * 2)()
    if rows * cols == 0:
        return out, dict(from_prior=0, fallback=0)
    if d.size == 0:
        raise ValueError("prior map is empty")
    L = _lib.lib()
    rc = L.bicos_guide_host(None, d.ctypes.data, _get_cv_type(d.dtype), d.shape[0], d.shape[1],
                            rows, cols, sc, r, sp, flo, fhi,
                            _lib.GUIDE_F32_SENTINEL if sentinel else 0, out.ctypes.data, cols,
                            counts)
    if rc != 0:
        raise RuntimeError("BICOS guide failed: " + L.bicos_last_error().decode(errors="replace"))
    return out, dict(from_prior=counts[0], fallback=counts[1])


def _host_stack(stack):
    """the images of a host stack as C-contiguous 2-D uint8 / uint16 arrays of one size"""
    imgs = [np.ascontiguousarray(im) for im in stack] if stack is not None else []
    if not imgs:
        raise ValueError("Empty image stack")
    f = imgs[0]
    if f.ndim != 2 or f.dtype not in (np.uint8, np.uint16):
        raise ValueError("images must be 2-D uint8 or uint16 arrays")
    if any(im.shape != f.shape or im.dtype != f.dtype for im in imgs):
        raise ValueError("all images must share size and type")
    return imgs


def pool_stack(stack, scale):
    """An extension: the images of `stack` -- a list of 2-D uint8 or uint16 arrays of one size,
    or one [n, rows, cols] array -- pooled by `scale` in 2..8 on the GPU (bicos_pool_host,
    include/bicos_c.h "stack pooling"): each output pixel is (sum of its scale x scale block +
    scale*scale // 2) // (scale*scale), the mean rounded half up, in integers. Returns an [n,
    rows // scale, cols // scale] array of the input dtype, ready for match(); the rows % scale
    last rows and cols % scale last columns are not read. (A numpy .mean().astype() truncates
    instead: it is not this function.)"""
    sc = _lib.pool_scale(scale)
    imgs = _host_stack(stack)
    f = imgs[0]
    n = len(imgs)
    prows, pcols = _lib.pool_shape(f.shape[0], f.shape[1], sc)
    out = np.empty((n, prows, pcols), f.dtype)
    src = (ctypes.c_void_p * n)(*[im.ctypes.data for im in imgs])
    dst = (ctypes.c_void_p * n)(*[out[t].ctypes.data for t in range(n)])
    L = _lib.lib()
    rc = L.bicos_pool_host(None, src, n, f.shape[0], f.shape[1], 0, f.dtype.itemsize, sc, dst, 0)
    if rc != 0:
        raise RuntimeError("BICOS pooling failed: " + L.bicos_last_error().decode(errors="replace"))
    return out


def match_pyramid(stack0, stack1, cfg, scale=2, radius=2, spread=1, fallback=None):
    """An extension: the coarse-to-fine match in one call, for disparity windows too wide for
    one search (bicos_match_host_pyramid, include/bicos_c.h "pyramid match"). Byte for byte:
    pool_stack of both stacks by `scale`; match() of the pooled stacks without a subpixel step
    over cfg.disparity_range divided by scale (floor, ceil); guide_from_disparity(coarse,
    radius, spread, scale, fallback, shape=(rows, cols)); match(guide=) of the full stacks.
    cfg.disparity_range is required. fallback None: the global window clamped to +-32767; a
    pair with lo > hi: do not search where the coarse map knows nothing. Each stack is uploaded
    once. Returns (disparity, corrmap, stats) with stats = dict(from_prior, fallback)."""
    if cfg is None:
        raise ValueError("match_pyramid needs a Config with a disparity_range")
    rng, sc, r, sp, flo, fhi = _lib.pyramid_params(getattr(cfg, "disparity_range", None), scale,
                                                   radius, spread, fallback)
    im0, im1 = _host_stack(stack0), _host_stack(stack1)
    f = im0[0]
    if len(im0) != len(im1) or im1[0].shape != f.shape or im1[0].dtype != f.dtype:
        raise ValueError("both stacks must share length, size and type")
    rows, cols = f.shape
    _lib.pool_shape(rows, cols, sc)
    n = len(im0)
    L = _lib.lib()
    ddtype = _get_np_dtype(L.bicos_output_type(cfg._c_config, 1))
    cdtype = np.float64 if cfg._c_config.contents.precision else np.float32
    disparity = np.empty((rows, cols), ddtype)
    corrmap = np.empty((rows, cols), cdtype)
    counts = (ctypes.c_uint32 * 2)()
    d0 = (ctypes.c_void_p * n)(*[im.ctypes.data for im in im0])
    d1 = (ctypes.c_void_p * n)(*[im.ctypes.data for im in im1])
    rc = L.bicos_match_host_pyramid(None, d0, d1, n, rows, cols, 0, f.dtype.itemsize,
                                    cfg._c_config, 1, rng[0], rng[1], sc, r, sp, flo, fhi,
                                    disparity.ctypes.data, corrmap.ctypes.data, None, None, counts)
    if rc != 0:
        raise RuntimeError("BICOS matching failed: " + L.bicos_last_error().decode(errors="replace"))
    return disparity, corrmap, dict(from_prior=counts[0], fallback=counts[1])


def invalid_disparity(dtype):
    """reference pybicos/__init__.py:246-252."""
    L = _lib.lib()
    if dtype == np.float32:
        return L.BICOS_InvalidDisparityFloat()
    elif dtype == np.int16:
        return L.BICOS_InvalidDisparityInt16()
    raise ValueError(f"Unsupported dtype for invalid_disparity: {dtype}")
