"""Rectification without a GPU (include/bicos_c.h, "rectification"): the numpy restatement of
tests/rectify_ref.py against answers derived by hand and against independent float64
computations, the C-ABI symbols and their argument checks (BICOS_E_ARG before any HIP call),
and the Python plumbing.
"""
import ctypes
import inspect
import os

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import rectify_ref as ref

SYMBOLS = ("bicos_rectify_maps_device", "bicos_rectify_maps_host", "bicos_rectify_device",
           "bicos_rectify_host", "bicos_rectify_tile")
DTYPES = [np.uint8, np.uint16]


# ------------------------------------------------------------- the remap restatement
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16"])
def test_identity_map_reproduces_the_image(dtype):
    s = ref.images(3, 13, 17, dtype)
    mx, my = ref.identity_maps(13, 17)
    out, valid = ref.remap(s, mx, my, border=7)
    assert out.dtype == dtype and np.array_equal(out, s)
    assert valid.dtype == np.uint8 and valid.all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16"])
@pytest.mark.parametrize("dy,dx", [(0, 3), (2, 0), (-4, 5), (1, -2), (20, 0)])
def test_integer_shift(dtype, dy, dx):
    """out(v, u) = src(v + dy, u + dx), `border` where that leaves the frame"""
    s = ref.images(2, 11, 14, dtype, seed=1)
    mx, my = ref.identity_maps(11, 14)
    out, valid = ref.remap(s, mx + np.float32(dx), my + np.float32(dy), border=9)
    want = np.full_like(s, 9)
    ok = np.zeros((11, 14), bool)
    for v in range(11):
        for u in range(14):
            if 0 <= v + dy < 11 and 0 <= u + dx < 14:
                want[:, v, u] = s[:, v + dy, u + dx]
                ok[v, u] = True
    assert np.array_equal(out, want)
    assert np.array_equal(valid.astype(bool), ok)


def test_ties_round_to_even():
    s = np.array([[[1, 2, 3]]], np.uint8)
    my = np.zeros((1, 2), np.float32)
    out, valid = ref.remap(s, np.array([[0.5, 1.5]], np.float32), my)
    assert out.tolist() == [[[2, 2]]]  # 1.5 -> 2, 2.5 -> 2
    assert valid.tolist() == [[1, 1]]
    # the same ties down a column
    out, _ = ref.remap(s.reshape(1, 3, 1), np.zeros((2, 1), np.float32),
                       np.array([[0.5], [1.5]], np.float32))
    assert out.ravel().tolist() == [2, 2]


def test_borders_and_valid_by_hand():
    s = np.array([[[10, 20], [30, 40]]], np.uint16)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    #        in, half out left, exactly -1, last column, half out right, == cols, NaN, inf, huge
    xs = [0.0, -0.5, -1.0, 1.0, 1.5, 2.0, nan, inf, -1e30]
    mx = np.array([xs], np.float32)
    my = np.zeros_like(mx)
    out, valid = ref.remap(s, mx, my, border=4)
    assert out[0, 0].tolist() == [10, 7, 4, 20, 12, 4, 4, 4, 4]  # (4+10)/2 = 7, (20+4)/2 = 12
    assert valid[0].tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0]
    # the same values as rows
    out, valid = ref.remap(s, np.zeros((1, 9), np.float32), mx, border=4)
    assert out[0, 0].tolist() == [10, 7, 4, 30, 17, 4, 4, 4, 4]
    assert valid[0].tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0]
    # -1e-9 rounds the fraction to 1.0f: the tap at x0 + 1 = 0 alone, but x0 = -1 counts
    out, valid = ref.remap(s, np.array([[-1e-9]], np.float32), np.zeros((1, 1), np.float32), 4)
    assert out.ravel().tolist() == [10] and valid.ravel().tolist() == [0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16"])
def test_against_scipy_float64_bilinear(dtype):
    """|out - s| <= 0.5 + 2^-5 at every inside pixel: half a level for the final rounding plus
    the float32 rounding of the two fractions and five blend operations on values below 2^16,
    each at most 2^-9 (include/bicos_c.h)."""
    from scipy import ndimage
    rows, cols = 40, 56
    s = ref.images(2, rows, cols, dtype, seed=3)
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64),
                       indexing="ij")
    # affine plus quadratic, leaving the frame on two sides
    mx = (0.97 * u + 0.05 * v - 2.3 + 4e-4 * (u - 20) ** 2)
    my = (-0.04 * u + 1.02 * v + 1.7 + 3e-4 * (v - 10) * (u - 5))
    mx32, my32 = mx.astype(np.float32), my.astype(np.float32)
    out, valid = ref.remap(s, mx32, my32, border=11)
    inside = (mx32 > -1) & (mx32 < cols) & (my32 > -1) & (my32 < rows)
    assert inside.mean() > 0.5 and not inside.all() and valid.sum() > 0
    coords = np.stack([my32.astype(np.float64), mx32.astype(np.float64)])
    for t in range(s.shape[0]):
        want = ndimage.map_coordinates(s[t].astype(np.float64), coords, order=1,
                                       mode="grid-constant", cval=11.0)
        err = np.abs(out[t].astype(np.float64) - want)[inside]
        print("max |out - scipy| =", err.max())
        assert err.max() <= 0.5 + 2.0 ** -5


# -------------------------------------------------------------- the maps restatement
def _ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


@pytest.mark.parametrize("nd", [0, 4, 5, 8])
@pytest.mark.parametrize("p_cols", [3, 4])
def test_maps_against_numpy_inverse(nd, p_cols):
    """the same formula with np.linalg.inv: both are double results whose error is far below a
    float32 ulp, so only the final rounding can differ -- at most 1 ulp of the coordinate"""
    rows, cols = 37, 70
    K, D, R, P = ref.camera(rows, cols)
    D, P = D[:nd], P[:, :p_cols]
    mx, my = ref.maps(K, D, R, P, rows, cols)
    assert mx.dtype == np.float32 and mx.shape == (rows, cols)
    inv = np.linalg.inv(P[:, :3] @ R)
    wx, wy = ref.distort([float(v) for v in inv.ravel()], K, D, rows, cols)
    for got, want in ((mx, wx), (my, wy)):
        assert np.isfinite(got).all()
        assert (np.abs(got.astype(np.float64) - want) <= _ulp32(got)).all()
    # the maps are not trivially the identity
    iu, iv = ref.identity_maps(rows, cols)
    assert np.abs(mx - iu).max() > 1 and np.abs(my - iv).max() > 1


def test_maps_of_an_ideal_camera_are_the_identity_grid():
    """D = 0, R = I, P[:, :3] = K (no skew): the identity grid to 1 float32 ulp of the
    coordinate. Column 0 and row 0, whose coordinate is exactly 0, have no ulp to measure by:
    there fx*x + cx cancels two numbers of magnitude cx <= 2^6 in double, so 2^-40 bounds it."""
    rows, cols = 23, 31
    K = ref.camera(rows, cols)[0].copy()
    K[0, 1] = 0
    for R in (None, np.eye(3)):
        mx, my = ref.maps(K, None, R, K, rows, cols)
        iu, iv = ref.identity_maps(rows, cols)
        for got, want in ((mx, iu), (my, iv)):
            bound = np.where(want == 0, 2.0 ** -40, _ulp32(want))
            assert (np.abs(got.astype(np.float64) - want) <= bound).all()


def test_skew_is_ignored():
    rows, cols = 9, 11
    K, D, R, P = ref.camera(rows, cols)
    K0 = K.copy()
    K0[0, 1] = 0
    assert K[0, 1] != 0
    a, b = ref.maps(K, D, R, P, rows, cols), ref.maps(K0, D, R, P, rows, cols)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_cofactor_inverse_by_hand():
    iM, det = ref.inverse3([[2, 0, 0], [0, 4, 0], [0, 0, 8]])
    assert det == 64 and iM == [0.5, 0, 0, 0, 0.25, 0, 0, 0, 0.125]
    iM, det = ref.inverse3([[1, 2, 3], [0, 1, 4], [5, 6, 0]])
    assert det == 1 and iM == [-24, 18, 5, 20, -15, -4, -5, 4, 1]


# --------------------------------------------------------------------------- C-ABI
def test_rectify_symbols_are_exported_and_declared(blib):
    header = open(os.path.join(_lib._HERE, "..", "include", "bicos_c.h")).read()
    for s in SYMBOLS:
        assert hasattr(blib, s), s
        assert s in _lib.EXPORTS, s
        assert ("int %s(" % s) in header, s
    P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    PD, PP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_void_p)
    assert blib.bicos_rectify_maps_device.argtypes == [PD, PD, I, PD, PD, I, I, I, P, P, P]
    assert blib.bicos_rectify_maps_host.argtypes == [PD, PD, I, PD, PD, I, I, I, P, P]
    assert blib.bicos_rectify_device.argtypes == [P, P, I, I, I, Z, Z, I, P, P, Z, I, I, P, Z, Z,
                                                  I, P, P]
    assert blib.bicos_rectify_host.argtypes == [P, PP, I, I, I, Z, I, P, P, Z, I, I, PP, Z, I, P]
    tr, tc = _lib.rectify_tile()
    assert tr > 0 and tc > 0 and (tr * tc) % 64 == 0


_BUF = (ctypes.c_uint32 * 256)()
_P = ctypes.addressof(_BUF)  # never dereferenced: every case fails before any HIP call
_Q = _P + 512


def _remap_args(**kw):
    a = dict(src=_P, n=2, src_rows=4, src_cols=8, srp=8, spp=32, depth=1, map_x=_P, map_y=_P,
             map_pitch=0, rows=4, cols=8, dst=_Q, drp=8, dpp=32, border=0, valid=None)
    a.update(kw)
    return a


REMAP_ERRORS = [
    ("n_zero", dict(n=0), "at least one image"),
    ("src_rows_zero", dict(src_rows=0), "source size"),
    ("src_cols_negative", dict(src_cols=-8), "source size"),
    ("rows_zero", dict(rows=0), "output size"),
    ("cols_zero", dict(cols=0), "output size"),
    ("depth_4", dict(depth=4), "depth"),
    ("depth_0", dict(depth=0), "depth"),
    ("src_row_pitch_small", dict(srp=7), "source pitch"),
    ("src_plane_pitch_small", dict(spp=7), "source pitch"),
    ("dst_row_pitch_small", dict(drp=7), "output pitch"),
    ("dst_plane_pitch_small", dict(dpp=3), "output pitch"),
    ("map_pitch_not_multiple", dict(map_pitch=34), "multiple of 4"),
    ("map_pitch_small", dict(map_pitch=28), "map_pitch"),
    ("border_negative", dict(border=-1), "border"),
    ("border_256_u8", dict(border=256), "border"),
    ("border_65536_u16", dict(depth=2, border=65536), "border"),
    ("null_src", dict(src=None), "null source"),
    ("null_dst", dict(dst=None), "null output"),
    ("null_map_x", dict(map_x=None), "null map"),
    ("null_map_y", dict(map_y=None), "null map"),
    ("dst_is_src", dict(dst=_P), "must not be the source"),
    ("plane_too_large", dict(src_rows=70000, srp=70000), "2^32"),
]


@pytest.mark.parametrize("case", REMAP_ERRORS, ids=lambda c: c[0])
def test_rectify_argument_errors(blib, case):
    _, kw, word = case
    a = _remap_args(**kw)
    for engine in (None, 0x1000):  # never dereferenced
        rc = blib.bicos_rectify_device(engine, a["src"], a["n"], a["src_rows"], a["src_cols"],
                                       a["srp"], a["spp"], a["depth"], a["map_x"], a["map_y"],
                                       a["map_pitch"], a["rows"], a["cols"], a["dst"], a["drp"],
                                       a["dpp"], a["border"], a["valid"], None)
        assert rc == _lib.BICOS_E_ARG
        assert word in blib.bicos_last_error().decode()


HOST_ERRORS = [
    ("n_zero", dict(n=0), {}, "at least one image"),
    ("depth_3", dict(depth=3), {}, "depth"),
    ("src_step_small", dict(), dict(src_step=7), "source pitch"),
    ("dst_step_small", dict(), dict(dst_step=5), "output pitch"),
    ("src_step_odd_u16", dict(depth=2), dict(src_step=17), "multiple of the depth"),
    ("dst_step_odd_u16", dict(depth=2), dict(dst_step=19), "multiple of the depth"),
    ("border", dict(border=300), {}, "border"),
    ("rows_zero", dict(rows=0), {}, "output size"),
    ("null_map", dict(map_x=None), {}, "null map"),
    ("null_lists", dict(), dict(null_lists=True), "null image list"),
    ("null_image", dict(), dict(null_image=True), "null source"),
    ("dst_is_src", dict(), dict(same=True), "must not be the source"),
]


@pytest.mark.parametrize("case", HOST_ERRORS, ids=lambda c: c[0])
def test_rectify_host_argument_errors(blib, case):
    _, kw, h, word = case
    a = _remap_args(**kw)
    n = max(a["n"], 1)
    src = (ctypes.c_void_p * n)(*[_P + 64 * t for t in range(n)])
    dst = (ctypes.c_void_p * n)(*[_Q + 64 * t for t in range(n)])
    if h.get("null_image"):
        src[n - 1] = None
    if h.get("same"):
        dst[n - 1] = src[n - 1]
    if h.get("null_lists"):
        src = dst = None
    rc = blib.bicos_rectify_host(None, src, a["n"], a["src_rows"], a["src_cols"],
                                 h.get("src_step", 0), a["depth"], a["map_x"], a["map_y"],
                                 a["map_pitch"], a["rows"], a["cols"], dst, h.get("dst_step", 0),
                                 a["border"], None)
    assert rc == _lib.BICOS_E_ARG
    assert word in blib.bicos_last_error().decode()


def _cam(**kw):
    K, D, R, P = ref.camera(8, 12)
    a = dict(K=K, D=D, nd=8, R=R, P=P, p_cols=4, rows=8, cols=12, map_x=_P, map_y=_Q)
    a.update(kw)
    return a


_K, _D, _R, _PM = ref.camera(8, 12)
_NANK = _K.copy()
_NANK[1, 1] = np.nan
_INFD = _D.copy()
_INFD[3] = np.inf
_NANR = _R.copy()
_NANR[2, 0] = np.nan
_INFP = _PM.copy()
_INFP[0, 3] = -np.inf  # even the unused column
_SING = _PM.copy()
_SING[2, :] = 0
MAPS_ERRORS = [
    ("nd_3", dict(nd=3), "nd must be"),
    ("nd_12", dict(nd=12), "nd must be"),
    ("nd_negative", dict(nd=-1), "nd must be"),
    ("p_cols_2", dict(p_cols=2), "p_cols"),
    ("p_cols_5", dict(p_cols=5), "p_cols"),
    ("rows_zero", dict(rows=0), "output size"),
    ("cols_negative", dict(cols=-1), "output size"),
    ("too_many_pixels", dict(rows=65536, cols=32768), "int32"),
    ("null_K", dict(K=None), "null K"),
    ("null_P", dict(P=None), "null K"),
    ("null_D", dict(D=None), "null K"),
    ("null_map_x", dict(map_x=None), "null map"),
    ("null_map_y", dict(map_y=None), "null map"),
    ("nan_K", dict(K=_NANK), "not finite"),
    ("inf_D", dict(D=_INFD), "not finite"),
    ("nan_R", dict(R=_NANR), "not finite"),
    ("inf_P", dict(P=_INFP), "not finite"),
    ("singular", dict(P=_SING), "singular"),
]


@pytest.mark.parametrize("case", MAPS_ERRORS, ids=lambda c: c[0])
def test_rectify_maps_argument_errors(blib, case):
    _, kw, word = case
    a = _cam(**kw)

    def dbl(m):
        if m is None:
            return None
        m = np.asarray(m, np.float64).ravel()
        return (ctypes.c_double * m.size)(*m.tolist())

    args = (dbl(a["K"]), dbl(a["D"]), a["nd"], dbl(a["R"]), dbl(a["P"]), a["p_cols"], a["rows"],
            a["cols"], a["map_x"], a["map_y"])
    rc = blib.bicos_rectify_maps_device(*args, None)
    assert rc == _lib.BICOS_E_ARG
    assert word in blib.bicos_last_error().decode()
    rc = blib.bicos_rectify_maps_host(*args)
    assert rc == _lib.BICOS_E_ARG
    assert word in blib.bicos_last_error().decode()


# -------------------------------------------------------------------------- Python
def test_rectify_camera_marshalling():
    K, D, R, P = ref.camera(8, 12)
    k, d, nd, r, p, p_cols, rows, cols = _lib.rectify_camera(K, D[:5], None, P, (8, 12))
    assert list(k) == K.ravel().tolist() and list(d) == D[:5].tolist() and nd == 5
    assert r is None and list(p) == P.ravel().tolist() and p_cols == 4 and (rows, cols) == (8, 12)
    k, d, nd, r, p, p_cols, _, _ = _lib.rectify_camera(K.tolist(), None, R, P[:, :3], (1, 1))
    assert d is None and nd == 0 and list(r) == R.ravel().tolist() and p_cols == 3
    for bad in (dict(K=np.eye(4)), dict(D=np.zeros(3)), dict(R=np.eye(2)), dict(P=np.eye(4)),
                dict(size=(0, 4)), dict(size=5), dict(size=(65536, 32768))):
        a = dict(K=K, D=D, R=R, P=P, size=(8, 12))
        a.update(bad)
        with pytest.raises(ValueError):
            _lib.rectify_camera(a["K"], a["D"], a["R"], a["P"], a["size"])


def test_engine_methods_and_their_defaults(blib):
    from libbicos_amd import device
    p = inspect.signature(device.Engine.rectify).parameters
    assert list(p)[:4] == ["self", "stack", "map_x", "map_y"]
    for k in ("border", "out", "valid", "stream"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert p["border"].default == 0 and p["out"].default is None
    assert p["valid"].default is False and p["stream"].default is None
    assert "NEVER synchronises" in device.Engine.rectify.__doc__
    m = inspect.signature(device.Engine.rectify_maps).parameters
    assert list(m)[:6] == ["self", "K", "D", "R", "P", "size"]


def test_pybicos_rectify_validates_before_the_gpu(blib):
    from libbicos_amd import pybicos
    assert list(inspect.signature(pybicos.rectify).parameters) == ["stack", "map_x", "map_y",
                                                                   "border"]
    assert list(inspect.signature(pybicos.rectify_maps).parameters) == ["K", "D", "R", "P", "size"]
    mx, my = ref.identity_maps(4, 8)
    with pytest.raises(ValueError, match="Empty"):
        pybicos.rectify([], mx, my)
    with pytest.raises(ValueError, match="uint8 or uint16"):
        pybicos.rectify(np.zeros((2, 4, 8), np.float32), mx, my)
    with pytest.raises(ValueError, match="share size"):
        pybicos.rectify([np.zeros((4, 8), np.uint8), np.zeros((4, 9), np.uint8)], mx, my)
    with pytest.raises(ValueError, match="one shape"):
        pybicos.rectify(np.zeros((2, 4, 8), np.uint8), mx, my[:3])
    with pytest.raises(RuntimeError, match="border"):
        pybicos.rectify(np.zeros((2, 4, 8), np.uint8), mx, my, border=256)
    K, D, R, P = ref.camera(8, 12)
    with pytest.raises(ValueError, match="D must hold"):
        pybicos.rectify_maps(K, D[:6], R, P, (8, 12))
    with pytest.raises(RuntimeError, match="singular"):
        pybicos.rectify_maps(K, D, R, np.zeros((3, 4)), (8, 12))
