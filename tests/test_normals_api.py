"""The surface-normal stage without a GPU: the two restatements of its definition
(tests/normals_ref.py) against each other and against answers derived by hand, the C entries
and their argument checks (BICOS_E_ARG before any HIP call), and the Python plumbing.
"""
import ctypes
import inspect
import os

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import normals_ref as ref

bits = ref.bits
DTYPES = {"int16": np.int16, "float32": np.float32}
SYMBOLS = ("bicos_normals_device", "bicos_normals_host", "bicos_normals_tile")


# ---------------------------------------------------------------- the restatements
@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 6), (5, 1), (2, 2), (3, 3), (4, 7), (9, 11)])
def test_the_two_restatements_agree(shape, dtype):
    seen = np.zeros(4, np.int64)
    for name, d, q in ref.patterns(*shape, DTYPES[dtype]):
        for flags, radius, max_diff, min_points in ((0, 1, 1.0, 3), (2, 2, 0.0, 3), (1, 2, np.inf, 25),
                                                    (3, 4, 1.0, 5), (0, 4, np.inf, 81)):
            a = ref.restate(d, q, flags, radius, max_diff, min_points)
            b = ref.restate_loops(d, q, flags, radius, max_diff, min_points)
            assert np.array_equal(a["cls"], b["cls"]), (name, flags, radius)
            assert np.array_equal(bits(a["map"]), bits(b["map"])), (name, flags, radius)
            assert a["counts"].tolist() == b["counts"].tolist()
            assert int(a["counts"].sum()) == d.size
            nan = np.isnan(a["map"]).all(axis=-1)
            assert np.array_equal(nan, a["cls"] != ref.NORMAL)
            assert (bits(a["map"])[nan] == 0x7FC00000).all()
            unit = np.linalg.norm(a["map"][~nan].astype(np.float64), axis=-1)
            assert np.all(np.abs(unit - 1) < 1e-6)
            seen += a["counts"]
    if shape == (9, 11):
        assert seen.all()  # the cases exercise every class


def test_the_patterns_hold_what_they_are_for():
    pats = {n: (d, q) for n, d, q in ref.patterns(9, 11, np.float32)}
    assert set(pats) == {"exact", "tilted", "rounded", "random-holes", "special", "step",
                         "all-invalid", "odd-q"}
    assert set(n for n, _, _ in ref.patterns(9, 11, np.int16)) == set(pats) - {"tilted"}
    sp = pats["special"][0]
    assert np.isnan(sp).any() and (sp == -32768.0).any() and np.isposinf(sp).any() and np.isneginf(sp).any()
    st = pats["step"][0]
    assert np.abs(np.diff(st, axis=1)).max() > 1 and np.abs(np.diff(st, axis=0)).max() > 1
    assert not ref.valid_mask(pats["all-invalid"][0], ref.F32_SENTINEL).any()
    d, q = pats["odd-q"]
    w = q[3, 2] * d.astype(np.float64) + q[3, 3]
    assert (w == 0).any() and (w < 0).any() and (w > 0).any()
    assert (pats["rounded"][0] == np.rint(pats["rounded"][0])).all()
    assert (pats["tilted"][0] != np.rint(pats["tilted"][0])).all()


# ------------------------------------------------------------- answers by hand
def test_class_order_and_flag_values():
    assert (ref.NORMAL, ref.NO_POINT, ref.SPARSE, ref.DEGENERATE) == (0, 1, 2, 3)
    assert (ref.ALLOW_NEGATIVE_Z, ref.F32_SENTINEL) == (1, 2)
    assert (_lib.NORMALS_ALLOW_NEGATIVE_Z, _lib.NORMALS_F32_SENTINEL) == \
        (_lib.REPROJECT_ALLOW_NEGATIVE_Z, _lib.REPROJECT_F32_SENTINEL)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_a_constant_map_faces_the_camera_exactly(dtype):
    """U = (ux, 0, 0) and V = (0, vy, 0) exactly, so N = (0, 0, ux * vy) and |N| is its magnitude"""
    q = ref.rig_q(6, 7)
    for value, flags, want in ((12, 0, -1.0), (-12, ref.ALLOW_NEGATIVE_Z, 1.0)):
        d = np.full((6, 7), value, DTYPES[dtype])
        for fn in (ref.restate, ref.restate_loops):
            got = fn(d, q, flags, 2, 1.0, 3)
            assert got["counts"].tolist() == [42, 0, 0, 0]
            assert np.array_equal(got["map"], np.broadcast_to(np.float32([0, 0, want]), (6, 7, 3)))
    # Z < 0 without the flag: no point, as reproject drops it
    got = ref.restate(np.full((6, 7), -12, DTYPES[dtype]), q, 0)
    assert got["counts"].tolist() == [0, 42, 0, 0]


@pytest.mark.parametrize("shape", [(1, 9), (9, 1), (1, 1)])
def test_a_line_of_pixels_is_degenerate(shape):
    d = (20 + np.arange(shape[0] * shape[1])).reshape(shape).astype(np.float32)
    for fn in (ref.restate, ref.restate_loops):
        got = fn(d, ref.rig_q(*shape), 0, 2, np.inf, 3 if max(shape) > 2 else 3)
        n = d.size
        if shape == (1, 1):
            assert got["counts"].tolist() == [0, 0, 1, 0]  # one member < min_points
        else:
            # the two ends see 3 collinear members, the inner pixels more: det = 0 everywhere
            assert got["counts"].tolist() == [0, 0, 0, n]


def test_min_points_above_the_population_is_sparse():
    d = np.full((5, 5), 30, np.int16)
    q = ref.rig_q(5, 5)
    got = ref.restate(d, q, 0, 1, 1.0, 9)
    # only the 3 x 3 interior sees a full 3 x 3 window; the border windows are clipped
    want = np.full((5, 5), ref.SPARSE)
    want[1:4, 1:4] = ref.NORMAL
    assert np.array_equal(got["cls"], want) and got["counts"].tolist() == [9, 0, 16, 0]
    assert ref.restate(d, q, 0, 1, 1.0, 4)["counts"].tolist() == [25, 0, 0, 0]  # a corner holds 4
    # a step edge taller than max_diff cuts the window: 2 of 3 columns remain beside it
    d[:, 3:] += 5
    cls = ref.restate(d, q, 0, 1, 1.0, 9)["cls"]
    assert (cls[1:4, 1] == ref.NORMAL).all() and (cls[1:4, 2:4] == ref.SPARSE).all()
    assert (ref.restate(d, q, 0, 1, np.inf, 9)["cls"][1:4, 1:4] == ref.NORMAL).all()


@pytest.mark.parametrize("radius", [1, 2, 4])
def test_the_exact_plane_gives_the_analytic_normal(radius):
    """d = d00 + a x + b y under rig_q is the 3-D plane a X + b Y + (d0c / f) Z = B with
    d0c = d00 + a cx + b cy; N . P = B > 0 points away from the origin, so the normal is its
    negative. 1e-5 is a sanity bound, not a measurement: float32 output rounding is 2^-24, and
    the double cancellation in U, V for this Q is many orders below that."""
    rows, cols = 9, 11
    name, d, q = ref.patterns(rows, cols, np.float32)[0]
    assert name == "exact"
    a, b, d00 = 0.25, -0.5, 16.0
    f, cx, cy = q[2, 3], -q[0, 3], -q[1, 3]
    n = -np.array([a, b, (d00 + a * cx + b * cy) / f])
    n /= np.linalg.norm(n)
    got = ref.restate(d, q, 0, radius, np.inf, 3)
    assert got["counts"].tolist() == [rows * cols, 0, 0, 0]
    assert np.abs(got["map"].astype(np.float64) - n).max() <= 1e-5
    # max_diff = 1 keeps at least the centre's row and its neighbours: the same plane
    assert np.abs(ref.restate(d, q, 0, radius, 1.0, 3)["map"].astype(np.float64) - n).max() <= 1e-5


def test_integer_maps_stair_step():
    """the caveat of the documentation: the rounded plane steps every 1 / 0.137 = 7.3 columns
    and 1 / 0.071 = 14 rows, so about (3.3 / 7.3) * (10 / 14) = 0.3 of the 5 x 5 windows see
    no step at all and fit a fronto-parallel plane exactly; 0.1 leaves room for the borders"""
    name, d, q = [p for p in ref.patterns(24, 80, np.float32) if p[0] == "rounded"][0]
    flat = ref.restate(d, q, 0, 2, 1.0, 3)["map"]
    assert (flat[..., 2] == -1).mean() > 0.1
    name, d, q = [p for p in ref.patterns(24, 80, np.float32) if p[0] == "tilted"][0]
    assert (ref.restate(d, q, 0, 2, 1.0, 3)["map"][..., 2] == -1).sum() == 0


def test_gather_is_the_list_form():
    m = np.arange(2 * 3 * 3, dtype=np.float32).reshape(2, 3, 3)
    got = ref.gather(m, [5, 0, 0, -1, 6, 2 ** 31 - 1])
    assert np.array_equal(got[:3], m.reshape(-1, 3)[[5, 0, 0]])
    assert (bits(got[3:]) == 0x7FC00000).all()


# --------------------------------------------------------------------- C-ABI
def test_normals_symbols_are_exported_and_declared(blib):
    header = open(os.path.join(_lib._HERE, "..", "include", "bicos_c.h")).read()
    for s in SYMBOLS:
        assert hasattr(blib, s), s
        assert s in _lib.EXPORTS, s
        assert ("int %s(" % s) in header, s
    assert len(blib.bicos_normals_device.argtypes) == 16
    assert len(blib.bicos_normals_host.argtypes) == 15
    assert "#define BICOS_NORMALS_ALLOW_NEGATIVE_Z 1" in header
    assert "#define BICOS_NORMALS_F32_SENTINEL 2" in header
    assert "surface normals */" in header and "SUBPIXEL" in header
    tr, tc = _lib.normals_tile()
    assert tr > 0 and tc > 0 and (tr * tc) % 64 == 0  # whole waves


_BUF = (ctypes.c_uint32 * 1024)()
_P = ctypes.addressof(_BUF)  # never dereferenced: every case fails before any HIP call
_M = _P + 1024               # a normal map of 4 x 8 x 3 floats that does not overlap the map
_I = _P + 2048               # an index of 8 entries
_N = _P + 2560               # their normals
_C = _P + 3072               # counts
_E = 0x1000                  # a non-NULL "engine", never dereferenced either
_Q = (ctypes.c_double * 16)(*ref.rig_q(4, 8).ravel().tolist())
NAN, INF = float("nan"), float("inf")
# (type, rows, cols, Q, flags, radius, max_diff, min_points, map, normal_map, index, count,
#  normals, counts) -> word of the message
OK = (5, 4, 8, _Q, 0, 2, 1.0, 3, _P, _M, _I, 8, _N, _C)


def _case(**kw):
    names = ("typ", "rows", "cols", "Q", "flags", "radius", "max_diff", "min_points", "map",
             "normal_map", "index", "count", "normals", "counts")
    assert set(kw) <= set(names)
    return tuple(kw.get(n, v) for n, v in zip(names, OK))


ARG_ERRORS = [
    ("bad_type", _case(typ=0), "CV_16S"),
    ("f64_type", _case(typ=6), "CV_16S"),
    ("unknown_flags", _case(flags=4), "flag"),
    ("radius_0", _case(radius=0), "radius"),
    ("radius_5", _case(radius=5, min_points=3), "radius"),
    ("radius_negative", _case(radius=-1), "radius"),
    ("max_diff_negative", _case(max_diff=-0.5), "max_diff"),
    ("max_diff_nan", _case(max_diff=NAN), "max_diff"),
    ("min_points_2", _case(min_points=2), "min_points"),
    ("min_points_10_of_9", _case(radius=1, min_points=10), "min_points"),
    ("min_points_82_of_81", _case(radius=4, min_points=82), "min_points"),
    ("negative_rows", _case(rows=-1), "negative image size"),
    ("negative_cols", _case(cols=-8), "negative image size"),
    ("too_many_pixels", _case(rows=65536, cols=32768), "int32"),
    ("null_map", _case(map=None), "null disparity"),
    ("null_q", _case(Q=None), "null Q"),
    ("no_output", _case(normal_map=None, index=None, normals=None, counts=None, count=0), "no output"),
    ("normals_without_index", _case(index=None), "without index"),
    ("index_without_normals", _case(normals=None), "without normals"),
    ("counts_without_map", _case(normal_map=None), "counts need normal_map"),
    ("map_overlaps", _case(normal_map=_P), "normal_map overlaps"),
    ("map_overlaps_last_byte", _case(normal_map=_P + 127), "normal_map overlaps"),
    ("map_overlaps_from_below", _case(map=_P + 380, normal_map=_P), "normal_map overlaps"),
    ("normals_overlap", _case(normals=_P + 64), "normals overlaps"),
    ("counts_overlap", _case(counts=_P + 124), "counts overlaps"),
]


@pytest.mark.parametrize("case", ARG_ERRORS, ids=lambda c: c[0])
def test_normals_argument_errors(blib, case):
    name, (typ, rows, cols, q, flags, radius, max_diff, min_points, m, nmap, index, count,
           normals, counts), word = case
    for e in (_E, None):
        rc = blib.bicos_normals_device(e, m, typ, rows, cols, q, flags, radius, max_diff,
                                       min_points, nmap, index, count, normals, counts, None)
        assert rc == _lib.BICOS_E_ARG
        assert word in blib.bicos_last_error().decode()
    rc = blib.bicos_normals_host(None, m, typ, rows, cols, q, flags, radius, max_diff, min_points,
                                 nmap, index, count, normals, counts)
    assert rc == _lib.BICOS_E_ARG
    assert word in blib.bicos_last_error().decode()


def test_legal_edges_pass_the_checks(blib):
    """+inf max_diff, the full window, adjacent buffers and an empty map with NULL map and Q are
    not argument errors (the empty host call needs no GPU: nothing is launched)"""
    counts = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    out = np.zeros((2, 3), np.float32)
    idx = np.array([0, 5], np.int32)
    for rows, cols in ((0, 5), (5, 0), (0, 0)):
        rc = blib.bicos_normals_host(None, None, 3, rows, cols, None, 3, 4, INF, 81, _M,
                                     idx.ctypes.data, 2, out.ctypes.data, counts)
        assert rc == 0, blib.bicos_last_error()
        assert list(counts) == [0, 0, 0, 0]
        assert (bits(out) == 0x7FC00000).all()


# -------------------------------------------------------------------- Python
def test_normals_params_marshalling():
    assert _lib.normals_params(2, 1.0, 3) == (2, 1.0, 3)
    assert _lib.normals_params(np.int64(4), np.float32(0), np.int32(81)) == (4, 0.0, 81)
    assert _lib.normals_params(1, INF, 9) == (1, INF, 9)
    for bad in ((0, 1, 3), (5, 1, 3), (-1, 1, 3), (1.5, 1, 3), (2, -1, 3), (2, NAN, 3), (2, 1, 2),
                (1, 1, 10), (4, 1, 82), (2, 1, 3.5), ("x", 1, 3), (2, None, 3), (2, 1, None)):
        with pytest.raises(ValueError):
            _lib.normals_params(*bad)
    assert _lib.normals_flags(False, False) == 0 and _lib.normals_flags(True, True) == 3
    assert _lib.normals_flags(True, False) == 1 and _lib.normals_flags(False, True) == 2


def test_engine_methods_and_their_defaults():
    from libbicos_amd import device
    p = inspect.signature(device.Engine.normals_map).parameters
    assert list(p) == ["self", "disp", "Q", "radius", "max_diff", "min_points", "allow_negative_z",
                       "sentinel", "out", "counts", "stream"]
    assert (p["radius"].default, p["max_diff"].default, p["min_points"].default) == (2, 1.0, 3)
    assert p["allow_negative_z"].default is False and p["sentinel"].default is False
    for k in list(p)[3:]:
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    p = inspect.signature(device.Engine.normals_points).parameters
    assert list(p)[:4] == ["self", "disp", "Q", "index"]
    assert (p["radius"].default, p["max_diff"].default, p["min_points"].default) == (2, 1.0, 3)
    for k in list(p)[4:]:
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    for fn in (device.Engine.normals_map, device.Engine.normals_points):
        assert "NEVER synchronises" in fn.__doc__


def test_pybicos_normals_validates_before_the_gpu(blib):
    import pybicos as alias
    from libbicos_amd import pybicos
    assert alias.normals is pybicos.normals
    sig = inspect.signature(pybicos.normals).parameters
    assert list(sig) == ["disparity", "Q", "radius", "max_diff", "min_points", "allow_negative_z",
                         "sentinel", "index"]
    assert (sig["radius"].default, sig["max_diff"].default, sig["min_points"].default) == (2, 1.0, 3)
    assert sig["allow_negative_z"].default is False and sig["sentinel"].default is True
    assert sig["index"].default is None
    q = ref.rig_q(4, 8)
    d = np.zeros((4, 8), np.float32)
    with pytest.raises(ValueError, match="2-D"):
        pybicos.normals(np.zeros((2, 4, 8), np.float32), q)
    with pytest.raises(ValueError, match="dtype"):
        pybicos.normals(np.zeros((4, 8), np.float64), q)
    with pytest.raises(ValueError, match="4x4"):
        pybicos.normals(d, np.eye(3))
    with pytest.raises(ValueError, match="radius"):
        pybicos.normals(d, q, radius=5)
    with pytest.raises(ValueError, match="max_diff"):
        pybicos.normals(d, q, max_diff=-1)
    with pytest.raises(ValueError, match="min_points"):
        pybicos.normals(d, q, radius=1, min_points=10)
    with pytest.raises(ValueError, match="1-D"):
        pybicos.normals(d, q, index=np.zeros((2, 2), np.int32))
    # empty maps and lists never reach the GPU
    assert pybicos.normals(np.zeros((0, 8), np.int16), q).shape == (0, 8, 3)
    got = pybicos.normals(np.zeros((0, 8), np.int16), q, index=[0, 3])
    assert got.shape == (2, 3) and (bits(got) == 0x7FC00000).all()
    assert pybicos.normals(d, q, index=[]).shape == (0, 3)
