"""The speckle filter's interface without a GPU (include/bicos_c.h, "speckle filter"): the two
CPU restatements of tests/speckle_ref.py against each other and against answers derived by
hand, the C-ABI symbols and their argument checks (BICOS_E_ARG before any HIP call), and the
Python plumbing.
"""
import ctypes
import inspect
import os

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import speckle_ref as ref

SYMBOLS = ("bicos_speckle_device", "bicos_speckle_host", "bicos_speckle_tile")
INV = -32768
NAN = np.float32(np.nan)


# ---------------------------------------------------------------- the restatements
@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "float32"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 6), (5, 1), (7, 9), (12, 13)], ids=str)
def test_the_two_restatements_agree(shape, dtype):
    cases = ref.patterns(shape[0], shape[1], dtype)
    assert len(cases) > 20
    for name, d, max_size, max_diff, sentinel in cases:
        want = ref.restate(d, max_size, max_diff, sentinel)
        labels, sizes = ref.flood_fill(d, max_diff, sentinel)
        assert np.array_equal(labels, want["labels"]), name
        assert np.array_equal(sizes, want["sizes"]), name


@pytest.mark.parametrize("name,d", ref.golden_maps()[:6], ids=lambda v: v if isinstance(v, str) else "")
def test_the_two_restatements_agree_on_committed_maps(name, d):
    want = ref.restate(d, 4, 1.0, True)
    labels, sizes = ref.flood_fill(d, 1.0, True)
    assert np.array_equal(labels, want["labels"]) and np.array_equal(sizes, want["sizes"])


def test_size_boundary():
    """components of 3 and 4 pixels: max_size 3 removes the first alone"""
    d = np.array([[1, 1, INV, 9, 9],
                  [1, INV, INV, 9, 9]], np.int16)
    r = ref.restate(d, 3, 1.0)
    assert r["out"].tolist() == [[INV, INV, INV, 9, 9], [INV, INV, INV, 9, 9]]
    assert r["labels"].tolist() == [[0, 0, -1, 3, 3], [0, -1, -1, 3, 3]]
    assert r["counts"].tolist() == [4, 3, 3, 1]
    assert ref.restate(d, 2, 1.0)["counts"].tolist() == [7, 0, 3, 0]
    assert ref.restate(d, 4, 1.0)["counts"].tolist() == [0, 7, 3, 2]
    assert np.array_equal(ref.restate(d, 0, 1.0)["out"], d)


def test_difference_boundary():
    """|a - b| == max_diff links; one float step less of max_diff does not"""
    a, b = np.float32(1.25), np.float32(3.5)
    md = np.float32(2.25)
    d = np.array([[a, b]], np.float32)
    assert ref.restate(d, 1, md)["labels"].tolist() == [[0, 0]]
    assert ref.restate(d, 1, md)["counts"].tolist() == [2, 0, 0, 0]
    below = np.nextafter(md, np.float32(0))
    r = ref.restate(d, 1, below)
    assert r["labels"].tolist() == [[0, 1]] and r["counts"].tolist() == [0, 2, 0, 2]
    # and one float step more of the neighbour
    d2 = np.array([[a, np.nextafter(b, np.float32(np.inf))]], np.float32)
    assert ref.restate(d2, 1, md)["labels"].tolist() == [[0, 1]]
    i = np.array([[10, 12], [13, 15]], np.int16)
    assert ref.restate(i, 0, 2.0)["labels"].tolist() == [[0, 0], [2, 2]]
    assert ref.restate(i, 0, 3.0)["labels"].tolist() == [[0, 0], [0, 0]]


def test_chain_links_what_differs_by_more_than_max_diff():
    d = np.array([[1, 2, 3]], np.int16)  # 1 and 3 differ by 2 > 1, one component through 2
    r = ref.restate(d, 2, 1.0)
    assert r["labels"].tolist() == [[0, 0, 0]] and r["counts"].tolist() == [3, 0, 0, 0]
    assert ref.restate(d, 3, 1.0)["counts"].tolist() == [0, 3, 0, 1]


def test_nan_inf_and_sentinel():
    inf = np.float32(np.inf)
    d = np.array([[inf, inf, 5, NAN, -32768.0, -32768.0]], np.float32)
    # inf - inf is NaN: no link; inf - 5 = inf > 1: no link; without the flag -32768.0 is a number
    r = ref.restate(d, 1, 1.0, sentinel=False)
    assert r["labels"].tolist() == [[0, 1, 2, -1, 4, 4]]
    assert r["counts"].tolist() == [2, 3, 1, 3]
    assert np.isnan(r["out"][0, :4]).all() and r["out"][0, 4:].tolist() == [-32768.0, -32768.0]
    # with the flag it is invalid, and what removal writes
    r = ref.restate(d, 1, 1.0, sentinel=True)
    assert r["labels"].tolist() == [[0, 1, 2, -1, -1, -1]]
    assert r["counts"].tolist() == [0, 3, 3, 3]
    assert r["out"][0, :3].tolist() == [-32768.0] * 3 and np.isnan(r["out"][0, 3])
    # max_diff = +inf links infinities to finite numbers, still not to each other
    r = ref.restate(d, 0, np.inf, sentinel=True)
    assert r["labels"].tolist() == [[0, 1, 1, -1, -1, -1]]
    # an invalid pixel keeps its bits (NaN payload)
    p = np.array([[0x7FC00001, 0xFFC01234]], np.uint32).view(np.float32)
    assert ref.restate(p, 9, 1.0)["out"].view(np.uint32).tolist() == [[0x7FC00001, 0xFFC01234]]


# --------------------------------------------------------------------- C-ABI
def test_speckle_symbols_are_exported_and_declared(blib):
    header = open(os.path.join(_lib._HERE, "..", "include", "bicos_c.h")).read()
    for s in SYMBOLS:
        assert hasattr(blib, s), s
        assert s in _lib.EXPORTS, s
        assert ("int %s(" % s) in header, s
    assert len(blib.bicos_speckle_device.argtypes) == 12
    assert len(blib.bicos_speckle_host.argtypes) == 11
    assert blib.bicos_speckle_device.argtypes[6] is ctypes.c_float
    assert "#define BICOS_SPECKLE_F32_SENTINEL 1" in header
    assert _lib.SPECKLE_F32_SENTINEL == 1
    tr, tc = _lib.speckle_tile()
    assert tr > 0 and tc > 0 and (tr * tc) % 64 == 0  # whole waves


_BUF = (ctypes.c_uint32 * 256)()
_P = ctypes.addressof(_BUF)  # never dereferenced: every case fails before any HIP call
_E = 0x1000                  # a non-NULL "engine", never dereferenced either
# (disp_type, rows, cols, max_size, max_diff, flags, map, out) -> word of the message
ARG_ERRORS = [
    ("bad_type", (0, 4, 8, 1, 1.0, 0, _P, _P), "CV_16S"),
    ("f64_type", (6, 4, 8, 1, 1.0, 0, _P, _P), "CV_16S"),
    ("negative_rows", (3, -1, 8, 1, 1.0, 0, _P, _P), "negative image size"),
    ("negative_cols", (5, 4, -8, 1, 1.0, 0, _P, _P), "negative image size"),
    ("too_many_pixels", (3, 65536, 32768, 1, 1.0, 0, _P, _P), "int32"),
    ("unknown_flags", (5, 4, 8, 1, 1.0, 2, _P, _P), "flag"),
    ("negative_max_diff", (5, 4, 8, 1, -0.5, 0, _P, _P), "max_diff"),
    ("nan_max_diff", (5, 4, 8, 1, float("nan"), 0, _P, _P), "max_diff"),
    ("negative_max_size", (5, 4, 8, -1, 1.0, 0, _P, _P), "max_size"),
    ("null_map", (3, 4, 8, 1, 1.0, 0, None, _P), "null disparity"),
    ("null_out", (3, 4, 8, 1, 1.0, 0, _P, None), "null out"),
    ("overlap_after", (3, 4, 8, 1, 1.0, 0, _P, _P + 2), "overlap"),
    ("overlap_before", (5, 4, 8, 1, 1.0, 0, _P + 64, _P), "overlap"),
    ("overlap_last_byte", (3, 4, 8, 1, 1.0, 0, _P, _P + 62), "overlap"),
]


@pytest.mark.parametrize("case", ARG_ERRORS, ids=lambda c: c[0])
def test_speckle_argument_errors(blib, case):
    _, (typ, rows, cols, size, diff, flags, m, out), word = case
    rc = blib.bicos_speckle_device(_E, m, typ, rows, cols, size, diff, flags, out, None, None, None)
    assert rc == _lib.BICOS_E_ARG
    assert word in blib.bicos_last_error().decode()
    rc = blib.bicos_speckle_host(None, m, typ, rows, cols, size, diff, flags, out, None, None)
    assert rc == _lib.BICOS_E_ARG
    assert word in blib.bicos_last_error().decode()


def test_speckle_device_needs_an_engine(blib):
    rc = blib.bicos_speckle_device(None, _P, 3, 4, 8, 1, 1.0, 0, _P, None, None, None)
    assert rc == _lib.BICOS_E_ARG
    assert "engine" in blib.bicos_last_error().decode()


# -------------------------------------------------------------------- Python
def test_speckle_params_marshalling():
    assert _lib.speckle_params(5, 1) == (5, 1.0)
    assert _lib.speckle_params(np.int64(0), np.float32(0.5)) == (0, 0.5)
    assert _lib.speckle_params(3, float("inf")) == (3, float("inf"))
    for bad in ((-1, 1.0), (1.5, 1.0), (2 ** 31, 1.0), (1, -1.0), (1, float("nan"))):
        with pytest.raises(ValueError):
            _lib.speckle_params(*bad)


def test_engine_method_and_its_defaults(blib):
    """Python hands users float maps with -32768.0 (Engine.match), so sentinel defaults on"""
    from libbicos_amd import device
    p = inspect.signature(device.Engine.filter_speckles).parameters
    assert list(p)[:4] == ["self", "disp", "max_size", "max_diff"]
    assert p["max_diff"].default == 1.0
    for k in ("sentinel", "out", "labels", "counts", "stream"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert p["sentinel"].default is True and p["labels"].default is False
    assert p["out"].default is None and p["counts"].default is None and p["stream"].default is None
    assert "NEVER synchronises" in device.Engine.filter_speckles.__doc__


def test_pybicos_filter_speckles_validates_before_the_gpu(blib):
    from libbicos_amd import pybicos
    sig = inspect.signature(pybicos.filter_speckles).parameters
    assert list(sig) == ["disparity", "max_size", "max_diff", "sentinel"]
    assert sig["max_diff"].default == 1.0 and sig["sentinel"].default is True
    with pytest.raises(ValueError, match="2-D"):
        pybicos.filter_speckles(np.zeros((2, 4, 8), np.float32), 3)
    with pytest.raises(ValueError, match="dtype"):
        pybicos.filter_speckles(np.zeros((4, 8), np.float64), 3)
    with pytest.raises(ValueError, match="dtype"):
        pybicos.filter_speckles(np.zeros((4, 8), np.uint8), 3)
    with pytest.raises(ValueError, match="max_diff"):
        pybicos.filter_speckles(np.zeros((4, 8), np.int16), 3, -1.0)
    with pytest.raises(ValueError, match="max_size"):
        pybicos.filter_speckles(np.zeros((4, 8), np.int16), -3)
