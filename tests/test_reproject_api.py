"""The reprojection interface without a GPU (include/bicos_c.h, "reprojection"): the C-ABI
symbols and their argument checks (BICOS_E_ARG before any HIP call), the Python plumbing, and
a self-check of the numpy restatement that tests/test_reproject_gpu.py compares the kernels
against -- its points, formatted as the .xyz writer formats them, must be the bytes that the
project's CPU writer (bicos_cli::write_xyz through tests/cpp/imageio_check) produces.
"""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from libbicos_amd import _lib
from tests.test_cli import CHECK, Q, YAML, _built

REPROJECT_SYMBOLS = ("bicos_reproject_device", "bicos_reproject_host", "bicos_reproject_segment")
ALLOW_NEGATIVE_Z, F32_SENTINEL = 1, 2


# ---------------------------------------------------------------- the restatement
def restate(d, q, flags=0):
    """The definition in include/bicos_c.h, vectorised: elementwise float64 in the header's
    parenthesised order (numpy's ufuncs do not contract), then float32, then the classes.
    -> dict(map [rows, cols, 3], points [kept, 3], index [kept], counts uint32[4], kept mask)"""
    d = np.asarray(d)
    assert d.dtype in (np.int16, np.float32) and d.ndim == 2
    rows, cols = d.shape
    q = np.asarray(q, np.float64).reshape(16)
    y, x = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64),
                       indexing="ij")
    if d.dtype == np.int16:
        invalid = d == -32768
    else:
        invalid = np.isnan(d)
        if flags & F32_SENTINEL:
            invalid |= d == np.float32(-32768.0)
    dd = d.astype(np.float64)
    with np.errstate(all="ignore"):
        o = [((q[4 * i] * x + q[4 * i + 1] * y) + q[4 * i + 2] * dd) + q[4 * i + 3]
             for i in range(4)]
        iw = 1.0 / o[3]
        p = np.stack([(o[k] * iw).astype(np.float32) for k in range(3)], axis=-1)
        nonfinite = ~invalid & ~np.isfinite(p).all(axis=-1)
        negative = ~invalid & ~nonfinite & (p[..., 2] < 0)
    if flags & ALLOW_NEGATIVE_Z:
        negative[:] = False
    kept = ~invalid & ~nonfinite & ~negative
    xyz = np.where(kept[..., None], p, np.float32(np.nan)).astype(np.float32)
    counts = np.array([kept.sum(), invalid.sum(), nonfinite.sum(), negative.sum()], np.uint32)
    assert int(counts.astype(np.int64).sum()) == rows * cols
    return dict(map=xyz, points=np.ascontiguousarray(p[kept]),
                index=np.flatnonzero(kept.ravel()).astype(np.int32), counts=counts, kept=kept)


def xyz_text(points):
    """The .xyz writer's lines (an ostream's default float format is printf's %g)."""
    return "".join("%g %g %g\n" % (float(a), float(b), float(c)) for a, b, c in points).encode()


def make_map(rows, cols, dtype, seed, invalid=0.05, fractional=True, sentinels=True):
    """Integers -5..59 (under tests/test_cli.py's Q about 8 % give negative z and 1.5 % W = 0),
    planted invalids; float maps: fractional parts on half the pixels and, with `sentinels`,
    some -32768.0 too. The first pixel is always one that is kept."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-5, 60, size=(rows, cols)).astype(dtype)
    if dtype == np.float32:
        if fractional:
            frac = rng.integers(0, 16, size=(rows, cols)).astype(np.float32) / np.float32(16)
            d = np.where(rng.random((rows, cols)) < 0.5, d + frac, d).astype(np.float32)
        d[rng.random((rows, cols)) < invalid] = np.nan
        if sentinels:
            d[rng.random((rows, cols)) < 0.03] = -32768.0
    else:
        d[rng.random((rows, cols)) < invalid] = -32768
    d.flat[0] = 30
    return d


@pytest.mark.parametrize("dt,typ", [(np.int16, 3), (np.float32, 5)])
@pytest.mark.parametrize("allow", [0, 1])
def test_restatement_is_the_cpu_writer(tmp_path, dt, typ, allow):
    """37 x 211, 20 % invalid: the restatement's points as text are write_xyz's file, byte for
    byte, and its classes are write_xyz's counts"""
    _built()
    d = make_map(37, 211, dt, seed=typ, invalid=0.2, sentinels=False)
    raw = tmp_path / "d.raw"
    raw.write_bytes(d.tobytes())
    qf = tmp_path / "q.yml"
    qf.write_text(YAML.format(", ".join(repr(float(v)) for v in Q.ravel())))
    out = tmp_path / "p.xyz"
    r = subprocess.run([CHECK, "xyz", str(raw), "37", "211", str(typ), str(qf), str(allow), str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = restate(d, Q, ALLOW_NEGATIVE_Z if allow else 0)
    assert want["counts"][0] > 0.3 * d.size
    assert [int(v) for v in r.stdout.split()] == [int(want["counts"][k]) for k in (0, 2, 3)]
    assert out.read_bytes() == xyz_text(want["points"])


def test_restatement_classes_and_sentinel():
    d = np.array([[30, 0, -3, np.nan, -32768.0, 30.5]], np.float32)
    r = restate(d, Q, 0)  # the sentinel is a number like any other: far behind the camera
    assert r["counts"].tolist() == [2, 1, 1, 2] and r["index"].tolist() == [0, 5]
    r = restate(d, Q, F32_SENTINEL)
    assert r["counts"].tolist() == [2, 2, 1, 1]
    r = restate(d, Q, F32_SENTINEL | ALLOW_NEGATIVE_Z)
    assert r["counts"].tolist() == [3, 2, 1, 0] and r["index"].tolist() == [0, 2, 5]
    assert np.isnan(r["map"][0, 1]).all() and not np.isnan(r["map"][0, 2]).any()
    i = np.array([[30, -32768, 0]], np.int16)
    assert restate(i, Q)["counts"].tolist() == [1, 1, 1, 0]


# --------------------------------------------------------------------- C-ABI
def test_reproject_symbols_are_exported_and_declared(blib):
    header = open(os.path.join(_lib._HERE, "..", "include", "bicos_c.h")).read()
    for s in REPROJECT_SYMBOLS:
        assert hasattr(blib, s), s
        assert s in _lib.EXPORTS, s
        assert ("int %s(" % s) in header, s
    assert len(blib.bicos_reproject_device.argtypes) == 13
    assert len(blib.bicos_reproject_host.argtypes) == 12
    assert blib.bicos_reproject_device.argtypes[10] is ctypes.c_size_t
    assert blib.bicos_reproject_host.argtypes[10] is ctypes.c_size_t
    assert "#define BICOS_REPROJECT_ALLOW_NEGATIVE_Z 1" in header
    assert "#define BICOS_REPROJECT_F32_SENTINEL 2" in header
    assert (_lib.REPROJECT_ALLOW_NEGATIVE_Z, _lib.REPROJECT_F32_SENTINEL) == (1, 2)
    seg = blib.bicos_reproject_segment()
    assert seg > 0 and seg % 64 == 0  # whole waves


# (entry-independent arguments: disp_type, rows, cols, flags, xyz_map, points, counts) -> message
_BUF = (ctypes.c_uint32 * 64)()
_P = ctypes.addressof(_BUF)  # never dereferenced: every case fails before any HIP call
ARG_ERRORS = [
    ("bad_type", (0, 4, 8, 0, _P, None, None), "CV_16S"),
    ("f64_type", (6, 4, 8, 0, _P, None, None), "CV_16S"),
    ("negative_rows", (3, -1, 8, 0, _P, None, None), "negative"),
    ("negative_cols", (5, 4, -8, 0, _P, None, None), "negative"),
    ("too_many_pixels", (3, 65536, 32768, 0, _P, None, None), "int32"),
    ("no_output", (3, 4, 8, 0, None, None, None), "no output"),
    ("points_without_counts", (3, 4, 8, 0, None, _P, None), "counts"),
    ("unknown_flags", (5, 4, 8, 4, _P, None, None), "flag"),
]


@pytest.mark.parametrize("case", ARG_ERRORS, ids=lambda c: c[0])
def test_reproject_argument_errors(blib, case):
    _, (typ, rows, cols, flags, xyz, pts, counts), word = case
    q = _lib.reproject_q(Q)
    rc = blib.bicos_reproject_device(None, _P, typ, rows, cols, q, flags, xyz, pts, None, 8,
                                     counts, None)
    assert rc == _lib.BICOS_E_ARG
    assert word in blib.bicos_last_error().decode()
    rc = blib.bicos_reproject_host(None, _P, typ, rows, cols, q, flags, xyz, pts, None, 8, counts)
    assert rc == _lib.BICOS_E_ARG
    assert word in blib.bicos_last_error().decode()


def test_reproject_points_on_the_device_need_an_engine(blib):
    q = _lib.reproject_q(Q)
    rc = blib.bicos_reproject_device(None, _P, 3, 4, 8, q, 0, None, _P, None, 8, _P, None)
    assert rc == _lib.BICOS_E_ARG
    assert "engine" in blib.bicos_last_error().decode()


def test_reproject_index_needs_points_and_q(blib):
    q = _lib.reproject_q(Q)
    rc = blib.bicos_reproject_device(None, _P, 3, 4, 8, q, 0, _P, None, _P, 8, None, None)
    assert rc == _lib.BICOS_E_ARG and "index" in blib.bicos_last_error().decode()
    rc = blib.bicos_reproject_device(None, _P, 3, 4, 8, None, 0, _P, None, None, 0, None, None)
    assert rc == _lib.BICOS_E_ARG and "Q" in blib.bicos_last_error().decode()
    rc = blib.bicos_reproject_device(None, None, 3, 4, 8, q, 0, _P, None, None, 0, None, None)
    assert rc == _lib.BICOS_E_ARG and "null disparity" in blib.bicos_last_error().decode()


# -------------------------------------------------------------------- Python
def test_q_and_flag_marshalling(blib):
    q = _lib.reproject_q(Q)
    assert list(q) == [float(v) for v in Q.ravel()]
    assert list(_lib.reproject_q(Q.tolist())) == list(q)
    for bad in (np.eye(3), np.zeros(16), [[1, 2], [3, 4]], "Q"):
        with pytest.raises(ValueError):
            _lib.reproject_q(bad)
    assert _lib.reproject_flags(False, False) == 0
    assert _lib.reproject_flags(True, False) == 1
    assert _lib.reproject_flags(False, True) == 2
    assert _lib.reproject_flags(True, True) == 3


def test_engine_methods_and_their_defaults(blib):
    """Python hands users float maps with -32768.0 (Engine.match), so sentinel defaults on"""
    from libbicos_amd import device
    for name, extra in (("reproject_map", ()), ("reproject_points", ("with_index",))):
        sig = inspect.signature(getattr(device.Engine, name))
        p = sig.parameters
        assert list(p)[:3] == ["self", "disp", "Q"]
        for k in ("allow_negative_z", "sentinel", "out", "stream") + extra:
            assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
        assert p["allow_negative_z"].default is False and p["sentinel"].default is True
        assert p["out"].default is None and p["stream"].default is None
    assert inspect.signature(device.Engine.reproject_points).parameters["with_index"].default is False


def test_pybicos_reproject_validates_before_the_gpu(blib):
    from libbicos_amd import pybicos
    sig = inspect.signature(pybicos.reproject).parameters
    assert list(sig) == ["disparity", "Q", "allow_negative_z", "sentinel"]
    assert sig["allow_negative_z"].default is False and sig["sentinel"].default is True
    with pytest.raises(ValueError, match="dtype"):
        pybicos.reproject(np.zeros((4, 8), np.float64), Q)
    with pytest.raises(ValueError, match="dtype"):
        pybicos.reproject(np.zeros((4, 8), np.uint8), Q)
    with pytest.raises(ValueError, match="2-D"):
        pybicos.reproject(np.zeros((2, 4, 8), np.float32), Q)
    with pytest.raises(ValueError, match="4x4"):
        pybicos.reproject(np.zeros((4, 8), np.float32), np.eye(3))
