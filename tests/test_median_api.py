"""The median filter's interface without a GPU (include/bicos_c.h, "median filter"): the two
CPU restatements of tests/median_ref.py against each other and against answers derived by
hand, the padding identity and the selection networks the kernel rests on, the C-ABI symbols
and their argument checks (BICOS_E_ARG before any HIP call), and the Python plumbing.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import median_ref as ref

SYMBOLS = ("bicos_median_device", "bicos_median_host", "bicos_median_tile")
INV = -32768
NAN = np.float32(np.nan)
bits = ref.bits


def same(a, b):
    return a["counts"].tolist() == b["counts"].tolist() and \
        np.array_equal(bits(a["out"]), bits(b["out"]))


# ---------------------------------------------------------------- the restatements
@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "float32"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 6), (5, 1), (2, 2), (7, 9), (12, 13)], ids=str)
def test_the_two_restatements_agree(shape, dtype):
    cases = ref.patterns(shape[0], shape[1], dtype)
    assert len(cases) >= 9
    for name, d, sentinel in cases:
        for ksize in (3, 5):
            win = ref.windows(d, ksize, sentinel)
            for fill_min in ref.fill_mins(ksize):
                a = ref.finish(d, win, fill_min)
                assert same(a, ref.restate_shifted(d, ksize, fill_min, sentinel)), (name, ksize, fill_min)
                assert int(a["counts"].sum()) == d.size


def test_the_patterns_hold_what_they_are_for():
    cases = {n: (d, s) for n, d, s in ref.patterns(12, 13, np.float32)}
    d, _ = cases["special-sentinel1"]
    assert len(np.unique(bits(d)[np.isnan(d)])) >= 4  # several NaN payloads survive
    assert np.isinf(d).any() and (bits(d) == 0x80000000).any() and (bits(d) == 0).any()
    assert (bits(d) == ref.SENTINEL_BITS).any()
    d, _ = cases["random30-ties-sentinel1"]
    assert 0.15 < 1 - ref.valid_mask(d, True).mean() < 0.45
    assert (bits(d) == ref.SENTINEL_BITS).any() and np.isnan(d).any()
    assert not ref.valid_mask(cases["all-invalid"][0], True).any()
    assert ref.valid_mask(cases["all-valid"][0], True).all()
    r = ref.restate(cases["holes"][0], 5, 13, True)
    assert r["counts"][2] > 0
    assert ref.restate(cases["outliers"][0], 3, 0)["counts"][1] > 0


def test_the_two_restatements_agree_on_committed_maps():
    maps = ref.golden_maps()
    assert len(maps) >= 6 and {d.dtype for _, d in maps} == {np.dtype(np.int16), np.dtype(np.float32)}
    for name, d in maps[:6]:
        a = ref.restate(d, 3, 5, True)
        assert same(a, ref.restate_shifted(d, 3, 5, True)), name


# --------------------------------------------------------- answers derived by hand
def test_one_outlier_in_a_3x3_map():
    d = np.array([[1, 2, 3], [4, 900, 6], [7, 8, 9]], np.int16)
    r = ref.restate(d, 3, 0)
    # corners see 4 values (lower median: rank 1), edges 6 (rank 2), the centre all 9 (rank 4)
    assert r["out"].tolist() == [[2, 3, 3], [4, 6, 6], [7, 7, 8]]
    assert r["counts"].tolist() == [4, 5, 0, 0]  # 3, 4, 6 and 7 are their windows' medians
    assert same(r, ref.restate_shifted(d, 3, 0))


def test_lower_median_of_an_even_count_at_a_corner():
    d = np.array([[10, 40, 0], [30, 20, 0], [0, 0, 0]], np.int16)
    for fn in (ref.restate, ref.restate_shifted):
        out = fn(d, 3, 0)["out"]
        assert out[0, 0] == 20  # sorted 10 20 30 40: m = 4, rank 1
    d5 = np.arange(1, 26, dtype=np.int16).reshape(5, 5)
    # ksize 5 at (0, 0): rows 0-2 x cols 0-2 = 1 2 3 6 7 8 11 12 13: m = 9, rank 4
    assert ref.restate(d5, 5, 0)["out"][0, 0] == 7 and ref.restate_shifted(d5, 5, 0)["out"][0, 0] == 7
    assert ref.restate(d5, 5, 0)["out"][2, 2] == 13


def test_negative_zero_sorts_before_positive_zero():
    nz, pz = np.float32(-0.0), np.float32(0.0)
    for fn in (ref.restate, ref.restate_shifted):
        out = fn(np.array([[pz, nz]], np.float32), 3, 0)["out"]
        assert bits(out).tolist() == [[0x80000000, 0x80000000]]  # m = 2, rank 0: -0.0
        out = fn(np.array([[pz, nz, pz]], np.float32), 3, 0)["out"]
        assert bits(out).tolist() == [[0x80000000, 0, 0x80000000]]
        out = fn(np.array([[-np.inf, NAN, np.inf, 1.0]], np.float32), 3, 0)["out"]
        assert bits(out)[0, 1] == bits(NAN.reshape(1))[0]
        assert out[0, 0] == -np.inf and out[0, 2] == 1.0 and out[0, 3] == 1.0


def test_fill_min_boundary():
    d = np.array([[5, INV, 7], [INV, INV, INV], [INV, 9, INV]], np.int16)  # centre: m = 3
    for fn in (ref.restate, ref.restate_shifted):
        r = fn(d, 3, 3)
        assert r["out"][1, 1] == 7  # filled at m == fill_min
        # (0,1): m = 2 (5, 7) stays; (1,0): 5, 9 m = 2 stays; (2,0): 9 m = 1; (2,2): 9
        assert r["out"].tolist() == [[5, INV, 7], [INV, 7, INV], [INV, 9, INV]]
        assert r["counts"].tolist() == [3, 0, 1, 5]
        r = fn(d, 3, 4)
        assert r["out"][1, 1] == INV and r["counts"].tolist() == [3, 0, 0, 6]
        r = fn(d, 3, 0)
        assert np.array_equal(r["out"], d)
        r = fn(d, 3, 1)
        assert r["counts"].tolist() == [3, 0, 6, 0] and (r["out"] != INV).all()


def test_sentinel_flag_and_nan_payloads():
    s = np.float32(-32768.0)
    d = np.array([[s, 1.0, s]], np.float32)
    for fn in (ref.restate, ref.restate_shifted):
        assert fn(d, 3, 0, False)["out"].tolist() == [[s, s, s]]  # a number like any other
        assert fn(d, 3, 0, False)["counts"].tolist() == [2, 1, 0, 0]
        assert fn(d, 3, 0, True)["out"].tolist() == [[s, 1.0, s]]
        assert fn(d, 3, 1, True)["out"].tolist() == [[1.0, 1.0, 1.0]]
        assert fn(d, 3, 1, True)["counts"].tolist() == [1, 0, 2, 0]
        p = np.array([[0x7FC00001, 0xFFC01234]], np.uint32).view(np.float32)
        assert bits(fn(p, 5, 1)["out"]).tolist() == [[0x7FC00001, 0xFFC01234]]
        assert fn(p, 5, 1)["counts"].tolist() == [0, 0, 0, 2]


@pytest.mark.parametrize("n", [9, 25])
def test_padding_identity_against_a_sort(n):
    """the j-th invalid slot becomes -inf for even j and +inf for odd j; rank (n - 1) / 2 of the
    padded n values is rank (m - 1) // 2 of the m valid ones (what the kernel's fixed network
    rests on), for every m, with ties, in every visiting order"""
    rng = np.random.default_rng(n)
    low, high = -10 ** 6, 10 ** 6
    for trial in range(3000):
        m = trial % (n + 1)
        vals = rng.integers(-4, 5, n)
        hole = np.zeros(n, bool)
        hole[rng.permutation(n)[:n - m]] = True
        padded, j = vals.copy(), 0
        for i in range(n):
            if hole[i]:
                padded[i] = low if j % 2 == 0 else high
                j += 1
        got = np.sort(padded)[(n - 1) // 2]
        if m == 0:
            assert got in (low, high)
        else:
            assert got == np.sort(vals[~hole])[(m - 1) // 2], (m, trial)


@pytest.mark.parametrize("n", [9, 25])
def test_selection_networks_by_the_zero_one_principle(n):
    """the exchange lists of libbicos_amd/csrc/median.hip leave the element of rank (n - 1) / 2
    in the wire the kernel returns: checked on all 2^n inputs of zeros and ones, which proves it
    for every input (min / max networks commute with monotone maps)"""
    src = open(os.path.join(_lib._HERE, "csrc", "median.hip")).read()
    body = src.split("// NETWORK %d\n" % n)[1].split("// END")[0]
    pairs = [(int(a), int(b)) for a, b in re.findall(r"CX\((\d+), (\d+)\)", body)]
    assert len(pairs) == {9: 19, 25: 99}[n]
    assert ("return v[%d];" % (n // 2)) in src.split("// NETWORK %d\n" % n)[1][:len(body) + 40]
    # input x = 64 * word + bit; wire i of input x carries bit i of x, 64 inputs to a uint64
    words = 1 << (n - 6)
    idx = np.arange(words, dtype=np.uint64)
    low = [0xAAAAAAAAAAAAAAAA, 0xCCCCCCCCCCCCCCCC, 0xF0F0F0F0F0F0F0F0, 0xFF00FF00FF00FF00,
           0xFFFF0000FFFF0000, 0xFFFFFFFF00000000]
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    wire = [np.full(words, low[i], np.uint64) if i < 6 else
            np.where((idx >> np.uint64(i - 6)) & np.uint64(1), full, np.uint64(0)) for i in range(n)]
    for a, b in pairs:
        wire[a], wire[b] = wire[a] & wire[b], wire[a] | wire[b]
    # the median of zeros and ones is one iff at least (n + 1) / 2 inputs are: the ones among
    # the word's index bits plus those among the bit's own six
    high_ones = sum(((idx >> np.uint64(i)) & np.uint64(1)).astype(np.int64) for i in range(n - 6))
    at_least = np.array([sum(1 << b for b in range(64) if bin(b).count("1") >= t)
                         for t in range(8)], np.uint64)  # at_least[7] == 0
    want = at_least[np.clip((n + 1) // 2 - high_ones, 0, 7)]
    assert np.array_equal(wire[n // 2], want)


@pytest.mark.parametrize("ksize", [3, 5])
@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "float32"])
def test_interior_of_an_all_valid_map_is_the_plain_median(ksize, dtype):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    d = rng.integers(-300, 300, (14, 17)).astype(dtype)
    h = ksize // 2
    want = ndimage.median_filter(d, size=ksize)[h:-h, h:-h]
    for fn in (ref.restate, ref.restate_shifted):
        assert np.array_equal(fn(d, ksize, 0)["out"][h:-h, h:-h], want)


# --------------------------------------------------------------------- C-ABI
def test_median_symbols_are_exported_and_declared(blib):
    header = open(os.path.join(_lib._HERE, "..", "include", "bicos_c.h")).read()
    for s in SYMBOLS:
        assert hasattr(blib, s), s
        assert s in _lib.EXPORTS, s
        assert ("int %s(" % s) in header, s
    assert len(blib.bicos_median_device.argtypes) == 11
    assert len(blib.bicos_median_host.argtypes) == 10
    assert "#define BICOS_MEDIAN_F32_SENTINEL 1" in header
    assert "median filter */" in header and "cv::medianBlur" in header
    assert _lib.MEDIAN_F32_SENTINEL == 1
    tr, tc = _lib.median_tile()
    assert tr > 0 and tc > 0 and (tr * tc) % 64 == 0  # whole waves


_BUF = (ctypes.c_uint32 * 256)()
_P = ctypes.addressof(_BUF)  # never dereferenced: every case fails before any HIP call
_Q = _P + 512                # a second map of 4 x 8 that does not overlap the first
_E = 0x1000                  # a non-NULL "engine", never dereferenced either
# (disp_type, rows, cols, ksize, fill_min, flags, map, out) -> word of the message
ARG_ERRORS = [
    ("bad_type", (0, 4, 8, 3, 0, 0, _P, _Q), "CV_16S"),
    ("f64_type", (6, 4, 8, 3, 0, 0, _P, _Q), "CV_16S"),
    ("ksize_1", (3, 4, 8, 1, 0, 0, _P, _Q), "ksize"),
    ("ksize_4", (3, 4, 8, 4, 0, 0, _P, _Q), "ksize"),
    ("ksize_7", (5, 4, 8, 7, 0, 0, _P, _Q), "ksize"),
    ("ksize_negative", (5, 4, 8, -3, 0, 0, _P, _Q), "ksize"),
    ("fill_min_negative", (3, 4, 8, 3, -1, 0, _P, _Q), "fill_min"),
    ("fill_min_10_of_9", (3, 4, 8, 3, 10, 0, _P, _Q), "fill_min"),
    ("fill_min_26_of_25", (5, 4, 8, 5, 26, 0, _P, _Q), "fill_min"),
    ("unknown_flags", (5, 4, 8, 3, 0, 2, _P, _Q), "flag"),
    ("negative_rows", (3, -1, 8, 3, 0, 0, _P, _Q), "negative image size"),
    ("negative_cols", (5, 4, -8, 3, 0, 0, _P, _Q), "negative image size"),
    ("too_many_pixels", (3, 65536, 32768, 3, 0, 0, _P, _Q), "int32"),
    ("null_map", (3, 4, 8, 3, 0, 0, None, _Q), "null disparity"),
    ("null_out", (3, 4, 8, 3, 0, 0, _P, None), "null out"),
]
DEVICE_ONLY = [
    ("in_place", (3, 4, 8, 3, 0, 0, _P, _P), "overlap"),
    ("overlap_after", (3, 4, 8, 3, 0, 0, _P, _P + 2), "overlap"),
    ("overlap_before", (5, 4, 8, 5, 25, 1, _P + 64, _P), "overlap"),
    ("overlap_last_byte", (3, 4, 8, 3, 9, 0, _P, _P + 62), "overlap"),
]


@pytest.mark.parametrize("case", ARG_ERRORS + DEVICE_ONLY, ids=lambda c: c[0])
def test_median_argument_errors(blib, case):
    name, (typ, rows, cols, ksize, fill_min, flags, m, out), word = case
    for e in (_E, None):
        rc = blib.bicos_median_device(e, m, typ, rows, cols, ksize, fill_min, flags, out, None, None)
        assert rc == _lib.BICOS_E_ARG
        assert word in blib.bicos_last_error().decode()
    if case in ARG_ERRORS:  # (the host entry stages both maps: its out may be the map)
        rc = blib.bicos_median_host(None, m, typ, rows, cols, ksize, fill_min, flags, out, None)
        assert rc == _lib.BICOS_E_ARG
        assert word in blib.bicos_last_error().decode()


# -------------------------------------------------------------------- Python
def test_median_params_marshalling():
    assert _lib.median_params(3, 0) == (3, 0)
    assert _lib.median_params(np.int64(5), np.int32(25)) == (5, 25)
    assert _lib.median_params(3, 9) == (3, 9)
    for bad in ((1, 0), (4, 0), (7, 0), (-3, 0), (3.5, 0), (3, -1), (3, 10), (5, 26), (3, 1.5),
                ("x", 0), (None, 0)):
        with pytest.raises(ValueError):
            _lib.median_params(*bad)


def test_engine_method_and_its_defaults(blib):
    """Python hands users float maps with -32768.0 (Engine.match), so sentinel defaults on"""
    from libbicos_amd import device
    p = inspect.signature(device.Engine.median_filter).parameters
    assert list(p) == ["self", "disp", "ksize", "fill_min", "sentinel", "out", "counts", "stream"]
    assert p["ksize"].default == 3 and p["fill_min"].default == 0
    for k in ("sentinel", "out", "counts", "stream"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert p["sentinel"].default is True
    assert p["out"].default is None and p["counts"].default is None and p["stream"].default is None
    assert "NEVER synchronises" in device.Engine.median_filter.__doc__


def test_pybicos_median_filter_validates_before_the_gpu(blib):
    import pybicos as alias
    from libbicos_amd import pybicos
    assert alias.median_filter is pybicos.median_filter
    sig = inspect.signature(pybicos.median_filter).parameters
    assert list(sig) == ["disparity", "ksize", "fill_min", "sentinel"]
    assert sig["ksize"].default == 3 and sig["fill_min"].default == 0
    assert sig["sentinel"].default is True
    with pytest.raises(ValueError, match="2-D"):
        pybicos.median_filter(np.zeros((2, 4, 8), np.float32))
    with pytest.raises(ValueError, match="dtype"):
        pybicos.median_filter(np.zeros((4, 8), np.float64))
    with pytest.raises(ValueError, match="dtype"):
        pybicos.median_filter(np.zeros((4, 8), np.uint8))
    with pytest.raises(ValueError, match="ksize"):
        pybicos.median_filter(np.zeros((4, 8), np.int16), 4)
    with pytest.raises(ValueError, match="fill_min"):
        pybicos.median_filter(np.zeros((4, 8), np.int16), 3, 10)
