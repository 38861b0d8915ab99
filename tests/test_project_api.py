"""The projection interface without a GPU (include/bicos_c.h, "projection"): the C-ABI symbols
and their argument checks (BICOS_E_ARG before any HIP call), the Python plumbing, the coloured
.ply writer of the command-line tool, and a self-check of the numpy restatement
(tests/project_ref.py) that the GPU tests compare the kernels against: it must equal a plain
Python loop over points and splat pixels, give the hand-worked answers on small cases, and put
every reprojected pixel of a rig back onto itself.
"""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import project_ref as ref
from tests.normals_ref import rig_q
from tests.project_ref import F32, F64, bits
from tests.test_reproject_api import restate as restate_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLY_COLOR_CHECK = os.path.join(ROOT, "tests", "cpp", "ply_color_check")
SYMBOLS = ("bicos_project_device", "bicos_project_host", "bicos_project_group")
NAN, INF = float("nan"), float("inf")
V, O, OUT, B, I = ref.VISIBLE, ref.OCCLUDED, ref.OUTSIDE, ref.BEHIND, ref.INVALID


# ------------------------------------------------------- the restatement, checked
def f32bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def loop_project(points, c, size, splat, tol, image, fill):
    """the definition, point by point and splat pixel by splat pixel, on numpy scalars"""
    rows, cols = size
    n = len(points)
    R, t = c["R"], c["t"]
    rec = []
    keys = {}
    with np.errstate(all="ignore"):
        for i in range(n):
            X, Y, Z = (F64(v) for v in points[i])
            if not all(math.isfinite(v) for v in (X, Y, Z)):
                rec.append((I, NAN, NAN, NAN, 0, 0))
                continue
            Xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]
            Yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]
            Zc = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]
            if not Zc > 0:
                rec.append((B, NAN, NAN, NAN, 0, 0))
                continue
            x, y = Xc / Zc, Yc / Zc
            r2 = x * x + y * y
            kr = (1.0 + ((c["k3"] * r2 + c["k2"]) * r2 + c["k1"]) * r2) / \
                 (1.0 + ((c["k6"] * r2 + c["k5"]) * r2 + c["k4"]) * r2)
            xd = (x * kr + c["p1"] * ((2.0 * x) * y)) + c["p2"] * (r2 + (2.0 * x) * x)
            yd = (y * kr + c["p1"] * (r2 + (2.0 * y) * y)) + c["p2"] * ((2.0 * x) * y)
            uf, vf, zf = F32(c["fx"] * xd + c["cx"]), F32(c["fy"] * yd + c["cy"]), F32(Zc)
            pxf, pyf = np.floor(uf + F32(0.5)), np.floor(vf + F32(0.5))
            inside = math.isfinite(uf) and math.isfinite(vf) and F32(0) <= pxf < F32(cols) and \
                F32(0) <= pyf < F32(rows)
            if not inside:
                rec.append((OUT, uf, vf, zf, 0, 0))
                continue
            px, py = int(pxf), int(pyf)
            rec.append((V, uf, vf, zf, px, py))
            key = (f32bits(zf) << 32) | i
            for yy in range(max(py - splat, 0), min(py + splat, rows - 1) + 1):
                for xx in range(max(px - splat, 0), min(px + splat, cols - 1) + 1):
                    keys[yy, xx] = min(keys.get((yy, xx), key), key)
        cls = np.zeros(n, np.uint8)
        uv = np.zeros((n, 2), F32)
        depth = np.zeros(n, F32)
        for i, (k, uf, vf, zf, px, py) in enumerate(rec):
            if k == V:
                zmin = np.array([keys[py, px] >> 32], np.uint32).view(F32)[0]
                if not zf <= zmin + F32(tol):
                    k = O
            cls[i], uv[i], depth[i] = k, (uf, vf), zf
    depth_map = np.full((rows, cols), NAN, F32)
    index_map = np.full((rows, cols), -1, np.int32)
    for (yy, xx), key in keys.items():
        depth_map[yy, xx] = np.array([key >> 32], np.uint32).view(F32)[0]
        index_map[yy, xx] = key & 0xFFFFFFFF
    out = dict(uv=uv, depth=depth, cls=cls, depth_map=depth_map, index_map=index_map,
               counts=np.bincount(cls, minlength=5).astype(np.uint32))
    if image is not None:
        img = image.reshape(rows, cols, -1)
        top = 255 if img.dtype == np.uint8 else 65535
        tex = np.full((n, img.shape[2]), fill, img.dtype)
        for i in np.flatnonzero(cls == V):
            uf, vf = uv[i]
            x0, y0 = np.floor(uf), np.floor(vf)
            fx, fy = uf - x0, vf - y0
            xa, xb = (min(max(int(x0) + k, 0), cols - 1) for k in (0, 1))
            ya, yb = (min(max(int(y0) + k, 0), rows - 1) for k in (0, 1))
            for k in range(img.shape[2]):
                p00, p01, p10, p11 = (F32(img[a, b, k]) for a, b in
                                      ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
                tp = p00 + fx * (p01 - p00)
                bt = p10 + fx * (p11 - p10)
                val = tp + fy * (bt - tp)
                assert type(val) is F32
                tex[i, k] = int(min(max(np.rint(val), F32(0)), F32(top)))
        out["tex"] = tex
    return out


@pytest.mark.parametrize("nd,moved,splat,tol,channels,dtype",
                         [(0, False, 0, 0.0, 1, np.uint8), (4, True, 1, 0.5, 3, np.uint8),
                          (5, True, 3, INF, 1, np.uint16), (8, True, 1, 0.0, 3, np.uint16)])
def test_restatement_is_the_loop(nd, moved, splat, tol, channels, dtype):
    rows, cols, n = 11, 17, 600
    K, D, R, t = ref.rig(rows, cols, nd, moved)
    pts = ref.cloud(n, rows, cols, K)
    img = ref.picture(rows, cols, channels, dtype)
    c = ref.camera(K, D, R, t)
    want = ref.restate(pts, c, (rows, cols), splat, tol, img, 7)
    got = loop_project(pts, c, (rows, cols), splat, tol, img, 7)
    assert (want["counts"] > 0).sum() >= 4 and int(want["counts"].sum()) == n
    for o in ref.OUTPUTS:
        if want[o].dtype == F32:
            assert np.array_equal(bits(want[o]), bits(got[o])), o
        else:
            assert np.array_equal(want[o], got[o]), o


# ------------------------------------------------------------- hand-worked cases
# K = identity-like: fx = fy = 1, cx = cy = 0, so a point (u*Z, v*Z, Z) lands on (u, v) exactly
# for the dyadic values used here; every number below is an integer or a dyadic fraction.
UNIT = ref.camera(np.eye(3))


def at(u, v, z=1.0):
    return [u * z, v * z, z]


def hand(points, size, **kw):
    return ref.restate(np.array(points, F32), UNIT, size, **kw)


def test_equal_depths_go_to_the_smaller_index():
    w = hand([at(2, 1, 4.0), at(2, 1, 4.0), at(2, 1, 8.0)], (3, 4), tol=0.0)
    assert w["index_map"][1, 2] == 0 and w["depth_map"][1, 2] == 4.0
    assert (w["index_map"] >= 0).sum() == 1
    # equal depth is not occluded (zf <= zmin + 0); the farther point is
    assert w["cls"].tolist() == [V, V, O] and w["counts"].tolist() == [2, 1, 0, 0, 0]
    w = hand([at(2, 1, 8.0), at(2, 1, 4.0), at(2, 1, 4.0)], (3, 4), tol=0.0)
    assert w["index_map"][1, 2] == 1 and w["cls"].tolist() == [O, V, V]


def test_half_a_pixel_beyond_the_first_is_inside_and_beyond_the_last_is_not():
    rows, cols = 3, 4
    w = hand([at(-0.5, 0), at(cols - 0.5, 0), at(0, -0.5), at(0, rows - 0.5), at(-0.75, 0),
              at(cols - 0.75, rows - 0.75)], (rows, cols))
    assert w["cls"].tolist() == [V, OUT, V, OUT, OUT, V]
    assert w["uv"][0].tolist() == [-0.5, 0.0] and w["uv"][1].tolist() == [cols - 0.5, 0.0]
    assert w["index_map"][0, 0] == 0  # (the first of the two points on pixel (0, 0))
    assert w["index_map"][rows - 1, cols - 1] == 5


def test_behind_and_invalid():
    w = hand([[1, 1, 0], [1, 1, -2], [NAN, 0, 1], [0, INF, 1], [0, 0, -INF], [1, 1, 1]], (3, 4))
    assert w["cls"].tolist() == [B, B, I, I, I, V]
    assert w["counts"].tolist() == [1, 0, 0, 2, 3]
    assert np.isnan(w["uv"][:5]).all() and np.isnan(w["depth"][:5]).all()
    assert (bits(w["uv"][:5]) == 0x7FC00000).all()
    assert w["uv"][5].tolist() == [1.0, 1.0] and w["depth"][5] == 1.0
    # a shifted camera: Zc = Z + t2
    c = ref.camera(np.eye(3), t=[0, 0, -1.0])
    w = ref.restate(np.array([[0, 0, 1], [0, 0, 0.5], [0, 0, 2]], F32), c, (1, 1))
    assert w["cls"].tolist() == [B, B, V]


def test_tolerance():
    pts = [at(1, 1, 2.0), at(1, 1, 2.5), at(1, 1, 3.0)]
    assert hand(pts, (3, 3), tol=0.0)["cls"].tolist() == [V, O, O]
    assert hand(pts, (3, 3), tol=0.5)["cls"].tolist() == [V, V, O]
    assert hand(pts, (3, 3), tol=1.0)["cls"].tolist() == [V, V, V]
    assert hand(pts, (3, 3), tol=INF)["cls"].tolist() == [V, V, V]
    # the maps do not depend on tol
    assert hand(pts, (3, 3), tol=INF)["index_map"][1, 1] == 0


def test_a_near_plane_hides_the_far_one_only_through_its_splat():
    """a far plane on every pixel of 8 x 8, a near plane on every second pixel of its left half:
    with splat = 1 the near points close their gaps and hide the far points between them, with
    splat = 0 the far plane shows through the holes"""
    far = [at(x, y, 4.0) for y in range(8) for x in range(8)]
    near = [at(x, y, 2.0) for y in range(0, 8, 2) for x in range(0, 4, 2)]
    w0 = hand(far + near, (8, 8), splat=0, tol=0.0)
    w1 = hand(far + near, (8, 8), splat=1, tol=0.0)
    f0, f1 = w0["cls"][:64].reshape(8, 8), w1["cls"][:64].reshape(8, 8)
    assert (w0["cls"][64:] == V).all() and (w1["cls"][64:] == V).all()
    # splat 0: only the far points exactly under a near point are hidden
    under = np.zeros((8, 8), bool)
    under[0:8:2, 0:4:2] = True
    assert np.array_equal(f0 == O, under)
    # splat 1: near points at columns 0, 2 and rows 0, 2, 4, 6 cover columns 0..3, rows 0..7
    covered = np.zeros((8, 8), bool)
    covered[:, 0:4] = True
    assert np.array_equal(f1 == O, covered)
    assert w0["counts"].tolist() == [64 - 8 + 8, 8, 0, 0, 0]
    assert w1["counts"].tolist() == [64 - 32 + 8, 32, 0, 0, 0]
    assert (w1["depth_map"][:, :4] == 2.0).all() and (w1["depth_map"][:, 4:] == 4.0).all()


def test_edges_are_replicated_at_all_four_borders():
    img = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)
    pts = [at(-0.5, 1), at(2.25, 1), at(1, -0.5), at(1, 2.25), at(-0.5, -0.5), at(2.25, 2.25),
           at(0.5, 0.5), at(5, 5)]
    w = hand(pts, (3, 3), image=img, fill=99)
    # left: taps (clamp(-1), 0) = (40, 40); right: x0 = 2, taps (60, 60); likewise rows
    assert w["tex"][:, 0].tolist() == [40, 60, 20, 80, 10, 90, 30, 99]
    assert w["cls"].tolist() == [V] * 7 + [OUT]


def test_rintf_ties_go_to_even_and_levels_saturate():
    img = np.array([[0, 1, 2, 5, 255, 255]], np.uint8)
    # halfway between 0 and 1 -> 0.5 -> 0; between 1 and 2 -> 1.5 -> 2; 2 and 5 -> 3.5 -> 4
    w = hand([at(0.5, 0), at(1.5, 0), at(2.5, 0), at(4.5, 0)], (1, 6), image=img)
    assert w["tex"][:, 0].tolist() == [0, 2, 4, 255]
    img16 = np.array([[65535, 65535, 0, 1]], np.uint16)
    w = hand([at(0.25, 0), at(2.5, 0), at(9, 0)], (1, 4), image=img16, fill=65535)
    assert w["tex"][:, 0].tolist() == [65535, 0, 65535] and w["tex"].dtype == np.uint16


def test_three_channels_are_interleaved():
    img = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) * 10
    w = hand([at(1, 0), at(1.5, 0.5)], (2, 3), image=img)
    assert w["tex"][0].tolist() == [30, 40, 50]
    # the mean of pixels (0,1) (0,2) (1,1) (1,2), per channel: 30, 60, 120, 150 -> 90
    assert w["tex"][1].tolist() == [90, 100, 110]


# ------------------------------------------------------------- round trip on a rig
def rig_points(rows, cols, seed=0):
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[0:rows, 0:cols]
    d = (30 + 0.01 * c - 0.005 * r + rng.random((rows, cols)) * 4).astype(F32)
    d[rng.random((rows, cols)) < 0.05] = np.nan
    f = 2000.0
    v = restate_points(d, rig_q(rows, cols, f))
    K = np.array([[f, 0, (cols - 1) / 2.0], [0, f, (rows - 1) / 2.0], [0, 0, 1]])
    return v, K


@pytest.mark.parametrize("rows,cols", [(48, 64), (97, 131), (2200, 3208)])
def test_reprojected_points_land_on_their_own_pixel(rows, cols):
    """float32 points carry 2^-24 relative error and uf below 4096 has an ulp of 2^-12: the
    projection of a reprojected pixel is within 2^-10 of the pixel, so it rounds to it"""
    v, K = rig_points(rows, cols)
    p = ref.pinhole(ref.camera(K), v["points"])
    row, col = np.divmod(v["index"].astype(np.int64), cols)
    assert not p["invalid"].any() and not p["behind"].any() and len(row) > 0.9 * rows * cols
    assert np.array_equal(p["pxf"], col.astype(F32)) and np.array_equal(p["pyf"], row.astype(F32))
    du, dv = np.abs(p["uf"] - col).max(), np.abs(p["vf"] - row).max()
    print("largest deviation at %dx%d: %.3g %.3g" % (cols, rows, du, dv))
    assert du <= 2.0 ** -10 and dv <= 2.0 ** -10


@pytest.mark.parametrize("rows,cols", [(48, 64), (97, 131)])
def test_index_map_inverts_index(rows, cols):
    v, K = rig_points(rows, cols)
    w = ref.restate(v["points"], ref.camera(K), (rows, cols), tol=0.0)
    n = len(v["index"])
    assert w["counts"].tolist() == [n, 0, 0, 0, 0]
    inverse = np.full(rows * cols, -1, np.int32)
    inverse[v["index"]] = np.arange(n, dtype=np.int32)
    assert np.array_equal(w["index_map"].ravel(), inverse)
    assert np.array_equal(np.isnan(w["depth_map"]), ~v["kept"])


# --------------------------------------------------------------- the C interface
def test_symbols_and_constants(blib):
    for s in SYMBOLS:
        assert hasattr(blib, s) and s in _lib.EXPORTS
    assert blib.bicos_project_group() == 1024
    header = open(os.path.join(ROOT, "include", "bicos_c.h")).read()
    for name, value in (("VISIBLE", 0), ("OCCLUDED", 1), ("OUTSIDE", 2), ("BEHIND", 3),
                        ("INVALID", 4), ("MAX_SPLAT", 3)):
        assert "#define BICOS_PROJECT_%s %d\n" % (name, value) in header
        assert getattr(_lib, "PROJECT_" + name) == value


_BUF = ctypes.create_string_buffer(16384)
_P = ctypes.addressof(_BUF)  # never dereferenced: every case fails before any HIP call
_PTS = _P                    # 32 points of 12 bytes
_IMG = _P + 1024             # 4 x 8 x 3 bytes at a pitch of 24
_UV = _P + 2048              # 32 x 8
_Z = _P + 3072               # 32 x 4
_CLS = _P + 4096             # 32
_TEX = _P + 5120             # 32 x 3
_DM = _P + 6144              # 4 x 8 x 4
_IM = _P + 7168
_CNT = _P + 8192             # 20
_E = 0x1000                  # a non-NULL "engine", never dereferenced either


def _d(*v):
    return (ctypes.c_double * len(v))(*v)


_K = _d(100, 0, 4, 0, 100, 2, 0, 0, 1)
_D8 = _d(*ref.DISTORTION)
NAMES = ("points", "count", "R", "t", "K", "D", "nd", "rows", "cols", "splat", "tol", "image",
         "depth", "channels", "pitch", "fill", "uv", "zdepth", "cls", "tex", "depth_map",
         "index_map", "counts")
OK = (_PTS, 32, None, None, _K, _D8, 8, 4, 8, 1, 0.5, _IMG, 1, 3, 24, 0, _UV, _Z, _CLS, _TEX,
      _DM, _IM, _CNT)


def _case(**kw):
    assert set(kw) <= set(NAMES)
    return tuple(kw.get(n, v) for n, v in zip(NAMES, OK))


_NONE = dict(uv=None, zdepth=None, cls=None, tex=None, depth_map=None, index_map=None,
             counts=None)
ARG_ERRORS = [
    ("no_output", _case(**_NONE), "no output"),
    ("tex_without_image", _case(image=None), "tex without image"),
    ("channels_2", _case(channels=2), "channels"),
    ("channels_0", _case(channels=0), "channels"),
    ("depth_4", _case(depth=4), "img_depth"),
    ("depth_0", _case(depth=0), "img_depth"),
    ("nd_3", _case(nd=3), "nd must be"),
    ("nd_negative", _case(nd=-1), "nd must be"),
    ("splat_4", _case(splat=4), "splat"),
    ("splat_negative", _case(splat=-1), "splat"),
    ("tol_negative", _case(tol=-0.5), "tol"),
    ("tol_nan", _case(tol=NAN), "tol"),
    ("fill_256_u8", _case(fill=256), "fill"),
    ("fill_negative", _case(fill=-1), "fill"),
    ("fill_65536_u16", _case(depth=2, fill=65536), "fill"),
    ("pitch_short", _case(pitch=23), "img_pitch"),
    ("negative_rows", _case(rows=-1), "negative image size"),
    ("negative_cols", _case(cols=-8), "negative image size"),
    ("too_many_pixels", _case(rows=65536, cols=32768, image=None, tex=None), "int32"),
    ("too_many_points", _case(count=2 ** 31), "count exceeds int32"),
    ("k_nan", _case(K=_d(100, 0, NAN, 0, 100, 2, 0, 0, 1)), "not finite"),
    ("k_inf", _case(K=_d(INF, 0, 4, 0, 100, 2, 0, 0, 1)), "not finite"),
    ("d_nan", _case(D=_d(0, 0, 0, 0, 0, 0, 0, NAN)), "not finite"),
    ("r_inf", _case(R=_d(1, 0, 0, 0, -INF, 0, 0, 0, 1)), "not finite"),
    ("t_nan", _case(t=_d(0, NAN, 0)), "not finite"),
    ("null_points", _case(points=None), "null points"),
    ("null_k", _case(K=None), "null K"),
    ("null_d", _case(D=None), "null D"),
    ("uv_overlaps_points", _case(uv=_PTS + 380), "uv overlaps points"),
    ("uv_overlaps_points_last_byte", _case(uv=_PTS + 383), "uv overlaps points"),
    ("depth_overlaps_image", _case(zdepth=_IMG + 24 * 3 + 23), "depth overlaps image"),
    ("cls_overlaps_uv", _case(cls=_UV + 255), "cls overlaps uv"),
    ("tex_overlaps_cls", _case(tex=_CLS - 95), "tex overlaps cls"),
    ("depth_map_overlaps_depth", _case(depth_map=_Z + 64), "depth_map overlaps depth"),
    ("index_map_is_depth_map", _case(index_map=_DM), "index_map overlaps depth_map"),
    ("counts_overlap_index_map", _case(counts=_IM + 124), "counts overlaps index_map"),
    ("counts_overlap_points", _case(counts=_PTS - 19), "counts overlaps points"),
]


def call(blib, entry, handle, args):
    f = getattr(blib, "bicos_project_" + entry)
    return f(handle, *args, *((None,) if entry == "device" else ()))


@pytest.mark.parametrize("case", ARG_ERRORS, ids=lambda c: c[0])
def test_project_argument_errors(blib, case):
    _, args, word = case
    for entry, handle in (("device", _E), ("host", None)):
        assert call(blib, entry, handle, args) == _lib.BICOS_E_ARG
        assert word in blib.bicos_last_error().decode()


def test_untouched_neighbours_do_not_overlap(blib):
    """(the negatives of the overlap cases: the byte after a span is free. The engine is checked
    last of all, so that message says every overlap check has passed)"""
    for kw in (dict(uv=_PTS + 384), dict(zdepth=_IMG + 24 * 3 + 24), dict(counts=_PTS - 20),
               dict(cls=_UV + 256), dict(tex=_CLS - 96)):
        assert call(blib, "device", None, _case(**kw)) == _lib.BICOS_E_ARG
        assert "null engine" in blib.bicos_last_error().decode()


def test_the_z_buffer_needs_an_engine_on_the_device(blib):
    for kw in (dict(), dict(tol=INF), dict(tol=INF, depth_map=None),
               dict(tol=0.0, depth_map=None, index_map=None)):
        assert call(blib, "device", None, _case(**kw)) == _lib.BICOS_E_ARG
        assert "null engine" in blib.bicos_last_error().decode()


def test_image_parameters_are_not_looked_at_without_an_image(blib):
    args = _case(image=None, tex=None, channels=7, depth=9, pitch=0, fill=-3)
    assert call(blib, "device", None, args) == _lib.BICOS_E_ARG
    assert "null engine" in blib.bicos_last_error().decode()


# --------------------------------------------------------------- the Python layers
def test_pybicos_project_checks_its_arguments():
    import pybicos
    pts = np.zeros((4, 3), np.float32)
    K = np.eye(3)
    with pytest.raises(ValueError, match="points"):
        pybicos.project(np.zeros((4, 3), np.float64), K, (4, 8))
    with pytest.raises(ValueError, match="points"):
        pybicos.project(np.zeros((4, 2), np.float32), K, (4, 8))
    with pytest.raises(ValueError, match="size"):
        pybicos.project(pts, K)
    with pytest.raises(ValueError, match="size"):
        pybicos.project(pts, K, (-1, 8))
    with pytest.raises(ValueError, match="K must"):
        pybicos.project(pts, np.eye(4), (4, 8))
    with pytest.raises(ValueError, match="D must"):
        pybicos.project(pts, K, (4, 8), D=[0, 0, 0])
    with pytest.raises(ValueError, match="R must"):
        pybicos.project(pts, K, (4, 8), R=np.eye(2))
    with pytest.raises(ValueError, match="t must"):
        pybicos.project(pts, K, (4, 8), t=[0, 0])
    with pytest.raises(ValueError, match="splat"):
        pybicos.project(pts, K, (4, 8), splat=4)
    with pytest.raises(ValueError, match="splat"):
        pybicos.project(pts, K, (4, 8), splat=0.5)
    with pytest.raises(ValueError, match="tol"):
        pybicos.project(pts, K, (4, 8), tol=-1)
    with pytest.raises(ValueError, match="tol"):
        pybicos.project(pts, K, (4, 8), tol=NAN)
    with pytest.raises(ValueError, match="fill"):
        pybicos.project(pts, K, (4, 8), fill=-1)
    with pytest.raises(ValueError, match="dtype"):
        pybicos.project(pts, K, image=np.zeros((4, 8), np.float32))
    with pytest.raises(ValueError, match="image must be"):
        pybicos.project(pts, K, image=np.zeros((4, 8, 2), np.uint8))
    with pytest.raises(ValueError, match="camera's size"):
        pybicos.project(pts, K, (4, 9), image=np.zeros((4, 8), np.uint8))
    with pytest.raises(ValueError, match="tex requires"):
        pybicos.project(pts, K, (4, 8), outputs=("tex",))
    with pytest.raises(ValueError, match="unknown outputs"):
        pybicos.project(pts, K, (4, 8), outputs=("uv", "normals"))
    with pytest.raises(ValueError, match="at least one"):
        pybicos.project(pts, K, (4, 8), outputs=())
    # the library's own refusal comes through as its message
    with pytest.raises(RuntimeError, match="fill"):
        pybicos.project(pts, K, image=np.zeros((4, 8), np.uint8), fill=256)
    # nothing but empty outputs never reaches the GPU
    got = pybicos.project(np.zeros((0, 3), np.float32), K, (4, 8), outputs=("uv", "cls"))
    assert got["uv"].shape == (0, 2) and got["cls"].shape == (0,)


def test_project_camera_and_params():
    r, t, k, d, nd = _lib.project_camera(np.eye(3) * 2, [1, 2, 3, 4, 5])
    assert r is None and t is None and list(k) == [2, 0, 0, 0, 2, 0, 0, 0, 2]
    assert list(d) == [1, 2, 3, 4, 5] and nd == 5
    r, t, k, d, nd = _lib.project_camera(np.eye(3), None, np.eye(3), [[1], [2], [3]])
    assert list(r) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(t) == [1, 2, 3] and d is None and nd == 0
    assert _lib.project_params((4, 8), 2, 0.5, 3) == (4, 8, 2, 0.5, 3)
    assert _lib.project_params((0, 8), 0, INF, 0) == (0, 8, 0, INF, 0)
    with pytest.raises(ValueError):
        _lib.project_params((65536, 32768), 0, 0.0, 0)


# ------------------------------------------------------- the coloured .ply writer
def ply_colored_bytes(points, rgb, triangles):
    """the file of the definition: the header's lines, then the records, with struct"""
    head = ["ply", "format binary_little_endian 1.0", "comment bicos-cli",
            "element vertex %d" % len(points), "property float x", "property float y",
            "property float z", "property uchar red", "property uchar green",
            "property uchar blue", "element face %d" % len(triangles),
            "property list uchar int vertex_indices", "end_header"]
    out = "".join(ln + "\n" for ln in head).encode("ascii")
    out += b"".join(struct.pack("<3f3B", *(float(v) for v in p), *(int(v) for v in c))
                    for p, c in zip(points, rgb))
    out += b"".join(struct.pack("<B3i", 3, *(int(v) for v in t)) for t in triangles)
    return out


@pytest.mark.parametrize("vertices,faces", [(5, 0), (0, 0), (300, 517), (5000, 3), (3, 5000)],
                         ids=["no_faces", "nothing", "hundreds", "vertex_chunks", "face_chunks"])
def test_colored_ply_writer(blib, tmp_path, vertices, faces):
    if not os.path.exists(PLY_COLOR_CHECK):  # (links the library: blib has built it)
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "ply_color.mk"],
                       check=True, capture_output=True)
    rng = np.random.default_rng(vertices + faces)
    pts = (rng.standard_normal((vertices, 3)) * 100).astype(np.float32)
    rgb = rng.integers(0, 256, (vertices, 3)).astype(np.uint8)
    if vertices:
        pts[0], rgb[0] = [0.0, -0.0, 1e-30], [0, 255, 10]
    tri = rng.integers(0, max(vertices, 1), (faces, 3)).astype(np.int32)
    (tmp_path / "p.raw").write_bytes(pts.tobytes())
    (tmp_path / "c.raw").write_bytes(rgb.tobytes())
    (tmp_path / "t.raw").write_bytes(tri.tobytes())
    out = tmp_path / "m.ply"
    r = subprocess.run([PLY_COLOR_CHECK, str(tmp_path / "p.raw"), str(tmp_path / "c.raw"),
                        str(vertices), str(tmp_path / "t.raw"), str(faces), str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == ply_colored_bytes(pts, rgb, tri)
