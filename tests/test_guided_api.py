"""The disparity guide without a GPU (include/bicos_c.h, "disparity guide"): the numpy
restatements that tests/test_guided_gpu.py holds the kernels to -- the guided search and the
guide builder, the latter against answers written out by hand --, the five C-ABI symbols and
their argument checks (BICOS_E_ARG before any HIP call), and the Python validation.
"""
import ctypes

import numpy as np
import pytest

from libbicos_amd import _lib
from oracle import ref_numpy as N
from tests.test_range_api import _argmin_win, rolled_descriptors, search_range

GUIDED_SYMBOLS = ("bicos_search_device_guided", "bicos_match_device_guided",
                  "bicos_match_host_guided", "bicos_guide_device", "bicos_guide_host")
INV = -32768
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


# ------------------------------------------------------- the search restatement
def row_costs(d0, d1):
    """the rows' Hamming cost matrices [col0, col1], for search_guided's `costs` (a test that
    runs many guides over the same descriptors computes them once)"""
    return [N._row_costs(d0[r], d1[r]) for r in range(d0.shape[0])]


def search_guided(d0, d1, flags, guide, gmin, gmax, max_lr_diff=-1, costs=None):
    """search_range of tests/test_range_api.py with the forward candidates of (row, col0)
    restricted to max(gmin, lo) <= col0 - col1 <= min(gmax, hi), (lo, hi) = guide[row, col0];
    Consistency's reverse search runs over the global window [gmin, gmax] alone."""
    H, W, _ = d0.shape
    guide = np.asarray(guide)
    assert guide.shape == (H, W, 2) and guide.dtype == np.int16
    out = np.full((H, W), INV, np.int16)
    col0 = np.arange(W)
    dd = col0[:, None] - col0[None, :]
    gmask = (dd >= gmin) & (dd <= gmax)
    for r in range(H):
        lo = guide[r, :, 0].astype(np.int64)[:, None]
        hi = guide[r, :, 1].astype(np.int64)[:, None]
        cost = costs[r] if costs is not None else N._row_costs(d0[r], d1[r])
        fwd = _argmin_win(cost, gmask & (dd >= lo) & (dd <= hi), bool(flags & 1))
        ok = fwd >= 0
        if flags & 2:
            rev = _argmin_win(cost.T, gmask.T, bool(flags & 1))
            r0 = np.where(ok, rev[np.maximum(fwd, 0)], -1)
            ok &= (r0 >= 0) & (np.abs(col0 - r0) <= max_lr_diff)
            val = (col0 + r0) // 2 - fwd
        else:
            val = col0 - fwd
        out[r] = np.where(ok, val, INV).astype(np.int16)
    return out


def constant_guide(H, W, lo, hi):
    g = np.empty((H, W, 2), np.int16)
    g[..., 0] = lo
    g[..., 1] = hi
    return g


# ------------------------------------------------------ the builder restatement
def guide_ref(prior, shape, radius, spread=0, scale=1, fallback=(-32767, 32767), sentinel=True):
    """The guide builder of include/bicos_c.h in numpy -> (guide int16 [rows, cols, 2],
    [from_prior, fallback])."""
    prior = np.asarray(prior)
    prows, pcols = prior.shape
    rows, cols = shape
    if prior.dtype == np.int16:
        valid = prior != INV
    else:
        assert prior.dtype == np.float32
        valid = ~np.isnan(prior)
        if sentinel:
            valid &= prior != np.float32(-32768.0)
    v = prior.astype(np.float32)
    # per prior pixel: min / max / any over the clipped (2 spread + 1)^2 window
    pad = spread
    vp = np.pad(v, pad, constant_values=0)
    mp = np.pad(valid, pad, constant_values=False)
    vmin = np.full((prows, pcols), np.inf, np.float32)
    vmax = np.full((prows, pcols), -np.inf, np.float32)
    some = np.zeros((prows, pcols), bool)
    for dy in range(2 * spread + 1):
        for dx in range(2 * spread + 1):
            w = vp[dy:dy + prows, dx:dx + pcols]
            m = mp[dy:dy + prows, dx:dx + pcols]
            vmin = np.where(m, np.minimum(vmin, w), vmin)
            vmax = np.where(m, np.maximum(vmax, w), vmax)
            some |= m
    lim = np.float32(32767)
    fl = np.clip(np.floor(np.where(some, vmin, 0)), -lim, lim).astype(np.int64)
    ce = np.clip(np.ceil(np.where(some, vmax, 0)), -lim, lim).astype(np.int64)
    lo = np.clip(scale * fl - radius, -32767, 32767)
    hi = np.clip(scale * ce + (scale - 1) + radius, -32767, 32767)
    lo = np.where(some, lo, fallback[0])
    hi = np.where(some, hi, fallback[1])
    pr = np.minimum(np.arange(rows) // scale, prows - 1)
    pc = np.minimum(np.arange(cols) // scale, pcols - 1)
    g = np.empty((rows, cols, 2), np.int16)
    g[..., 0] = lo[pr][:, pc]
    g[..., 1] = hi[pr][:, pc]
    n_prior = int(some[pr][:, pc].sum())
    return g, [n_prior, rows * cols - n_prior]


# ------------------------------------------------- the search restatement, checked
@pytest.mark.parametrize("flags,lr", [(1, -1), (2, 1), (3, 2)])
@pytest.mark.parametrize("words,period,low", [(1, None, 10), (4, 97, None), (8, None, None)])
def test_constant_guide_is_the_range_search(flags, lr, words, period, low):
    H, W = 2, 150
    d0, d1 = rolled_descriptors(H, W, words, period, low)
    for lo, hi in ((-30, 5), (3, 40), (-(W - 1), W - 1)):
        want = search_range(d0, d1, flags, lo, hi, lr)
        assert np.array_equal(search_guided(d0, d1, flags, constant_guide(H, W, lo, hi), lo, hi, lr),
                              want)
        # ... and so is a covering guide under that global window, or that guide under none
        cover = constant_guide(H, W, -32768, 32767)
        assert np.array_equal(search_guided(d0, d1, flags, cover, lo, hi, lr), want)
    full = constant_guide(H, W, -(W - 1), W - 1)
    assert np.array_equal(search_guided(d0, d1, flags, full, INT_MIN, INT_MAX, lr),
                          N.search(d0, d1, flags, lr))


def test_guide_excluding_the_planted_shift_changes_the_result():
    """256-bit random descriptors rolled by 20: the ranged search over [-40, 0] finds disparity
    -20 wherever the match lies in the row; a guide of [-40, -21] on the even columns takes
    that candidate away from them and leaves the odd ones as they were"""
    H, W = 2, 150
    d0, d1 = rolled_descriptors(H, W, 8)
    ranged = search_range(d0, d1, 1, -40, 0)
    assert (ranged[:, : W - 20] == -20).all()
    g = constant_guide(H, W, -40, 0)
    g[:, 0::2, 1] = -21
    got = search_guided(d0, d1, 1, g, -40, 0)
    assert not np.array_equal(got, ranged)
    assert (got[:, 1: W - 20: 2] == -20).all()
    even = got[:, 0: W - 20: 2]
    assert (even != -20).all() and ((even == INV) | ((even >= -40) & (even <= -21))).all()


def test_empty_windows_are_invalid_pixels():
    H, W = 1, 64
    d0, d1 = rolled_descriptors(H, W, 4)
    g = constant_guide(H, W, -30, 0)
    g[0, 10] = (5, 4)          # lo > hi
    g[0, 11] = (200, 300)      # outside the image
    g[0, 12] = (-32768, 32767)  # everything: cut by the global window alone
    got = search_guided(d0, d1, 1, g, -30, 0)
    assert got[0, 10] == INV and got[0, 11] == INV
    assert got[0, 12] == search_range(d0, d1, 1, -30, 0)[0, 12]


# ------------------------------------------- the builder: answers written by hand
def test_builder_hole_with_spread_0_and_1():
    prior = np.array([[5, INV, 7]], np.int16)
    g, counts = guide_ref(prior, (1, 3), radius=1, spread=0, fallback=(3, 2))
    assert g.tolist() == [[[4, 6], [3, 2], [6, 8]]] and counts == [2, 1]
    g, counts = guide_ref(prior, (1, 3), radius=1, spread=1, fallback=(3, 2))
    assert g.tolist() == [[[4, 6], [4, 8], [6, 8]]] and counts == [3, 0]


def test_builder_scale_3_at_the_right_and_bottom_edges():
    """a 2 x 2 prior for a 7 x 8 guide: rows 6 and columns 6, 7 lie past 3 * 2 and take the
    last prior row / column; lo = 3 v, hi = 3 v + 2"""
    prior = np.array([[1, 2], [3, 4]], np.int16)
    g, counts = guide_ref(prior, (7, 8), radius=0, scale=3)
    assert counts == [56, 0]
    assert g[0, 0].tolist() == [3, 5] and g[2, 2].tolist() == [3, 5]
    assert g[2, 3].tolist() == [6, 8] and g[0, 7].tolist() == [6, 8]
    assert g[3, 0].tolist() == [9, 11] and g[6, 0].tolist() == [9, 11]
    assert g[6, 7].tolist() == [12, 14] and g[3, 3].tolist() == [12, 14]
    assert (g[:3, :3] == [3, 5]).all() and (g[3:, 3:] == [12, 14]).all()


def test_builder_float_prior_takes_floor_and_ceil():
    prior = np.array([[2.25]], np.float32)
    assert guide_ref(prior, (1, 1), radius=0)[0].tolist() == [[[2, 3]]]
    # scale 2, radius 1: lo = 2 * 2 - 1, hi = 2 * 3 + 1 + 1
    assert guide_ref(prior, (2, 2), radius=1, scale=2)[0][1, 1].tolist() == [3, 8]
    neg = np.array([[-2.25, np.nan]], np.float32)
    assert guide_ref(neg, (1, 2), radius=0, fallback=(1, 0))[0].tolist() == [[[-3, -2], [1, 0]]]
    # the sentinel is a value when the flag is off
    s = np.array([[-32768.0]], np.float32)
    assert guide_ref(s, (1, 1), 0, fallback=(1, 0), sentinel=True)[0].tolist() == [[[1, 0]]]
    assert guide_ref(s, (1, 1), 0, fallback=(1, 0), sentinel=False)[0].tolist() == \
        [[[-32767, -32767]]]


def test_builder_clamps_at_32767():
    prior = np.array([[32767, -32767]], np.int16)
    g, _ = guide_ref(prior, (1, 2), radius=5, scale=1)
    assert g.tolist() == [[[32762, 32767], [-32767, -32762]]]
    g, _ = guide_ref(prior, (8, 16), radius=5, scale=8)
    assert g[0, 0].tolist() == [32767, 32767] and g[7, 15].tolist() == [-32767, -32767]
    inf = np.array([[np.inf, -np.inf, 1e9]], np.float32)
    g, counts = guide_ref(inf, (1, 3), radius=5)
    assert g.tolist() == [[[32762, 32767], [-32767, -32762], [32762, 32767]]] and counts == [3, 0]
    g, _ = guide_ref(np.array([[7]], np.int16), (1, 1), radius=32767)
    assert g.tolist() == [[[-32760, 32767]]]


def test_builder_empty_fallback():
    prior = np.full((3, 4), INV, np.int16)
    g, counts = guide_ref(prior, (3, 4), radius=9, spread=3, fallback=(1, 0))
    assert (g == [1, 0]).all() and counts == [0, 12]
    nan = np.full((2, 2), np.nan, np.float32)
    g, counts = guide_ref(nan, (5, 5), radius=0, scale=2, fallback=(-32768, 32767))
    assert (g == [-32768, 32767]).all() and counts == [0, 25]


# --------------------------------------------------------------------- C-ABI
def test_guided_symbols_are_exported_and_declared(blib):
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "bicos_c.h")).read()
    for s in GUIDED_SYMBOLS:
        assert hasattr(blib, s), s
        assert s in _lib.EXPORTS, s
        assert ("int %s(" % s) in header, s
    assert "disparity guide" in header
    assert "tight global window" in header.lower() and "transposed" in header


def _guided_calls(blib, lo, hi, guide, pitch):
    """the three guided entries with NULL engine, NULL buffers and no GPU: rows 4, cols 64"""
    cfg = _lib.BicosConfig(0.5, -1.0, -1.0, 0, 0, 0, 1, 0)
    yield "search", blib.bicos_search_device_guided(None, None, None, 4, 64, 4, 1, -1, lo, hi,
                                                    guide, pitch, None, None)
    yield "search msg", blib.bicos_last_error().decode()
    yield "match_device", blib.bicos_match_device_guided(
        None, None, None, 8, 4, 64, 64, 256, 1, ctypes.byref(cfg), 1, lo, hi, guide, pitch,
        None, None, None)
    yield "match_device msg", blib.bicos_last_error().decode()
    yield "match_host", blib.bicos_match_host_guided(
        None, None, None, 8, 4, 64, 0, 1, ctypes.byref(cfg), 1, lo, hi, guide, pitch, None, None)
    yield "match_host msg", blib.bicos_last_error().decode()


@pytest.mark.parametrize("case,word", [("null", "null guide"), ("pitch", "guide_pitch"),
                                       ("misaligned", "aligned"), ("min_above_max", "disparity range")])
def test_guided_argument_errors_come_before_any_hip_call(blib, case, word):
    buf = np.zeros(4 * 64 * 2 + 8, np.int16)
    base = buf.ctypes.data
    assert base % 4 == 0
    guide, pitch, lo, hi = base, 64, -5, 5
    if case == "null":
        guide = None
    elif case == "pitch":
        pitch = 63
    elif case == "misaligned":
        guide = base + 2
    else:
        lo, hi = 5, 4
    got = list(_guided_calls(blib, lo, hi, guide, pitch))
    for (name, rc), (_, msg) in zip(got[0::2], got[1::2]):
        assert rc == _lib.BICOS_E_ARG, (name, rc, msg)
        assert word in msg, (name, msg)
    if case == "pitch":
        assert "63" in got[1][1] and "64" in got[1][1]
    if case == "min_above_max":
        assert "5" in got[1][1] and "4" in got[1][1]


def test_guided_no_global_bound_passes_the_argument_check(blib):
    """(INT_MIN, INT_MAX) is a legal window: the search entry then gets as far as asking for
    an engine (Consistency) -- still no HIP call"""
    buf = np.zeros(4 * 64 * 2, np.int16)
    rc = blib.bicos_search_device_guided(None, None, None, 4, 64, 4, 2, 1, INT_MIN, INT_MAX,
                                         buf.ctypes.data, 64, None, None)
    assert rc == _lib.BICOS_E_ARG
    assert "engine" in blib.bicos_last_error().decode()


def test_guide_builder_argument_errors(blib):
    prior = np.zeros((4, 8), np.int16)
    out = np.zeros((4, 8, 2), np.int16)
    P, G = prior.ctypes.data, out.ctypes.data

    def call(prior=P, typ=_lib.CV_16S, prows=4, pcols=8, rows=4, cols=8, scale=1, radius=0,
             spread=0, flo=0, fhi=0, flags=0, guide=G, pitch=0):
        a = (None, prior, typ, prows, pcols, rows, cols, scale, radius, spread, flo, fhi, flags,
             guide, pitch, None)
        rcs = (blib.bicos_guide_device(*a, None), blib.bicos_guide_host(*a))
        return rcs, blib.bicos_last_error().decode()

    for kw, word in ((dict(scale=0), "scale"), (dict(scale=9), "scale"),
                     (dict(radius=-1), "radius"), (dict(radius=32768), "radius"),
                     (dict(spread=8), "spread"), (dict(spread=-1), "spread"),
                     (dict(flo=-32769), "fallback"), (dict(fhi=32768), "fallback"),
                     (dict(typ=_lib.CV_8U), "CV_16S"), (dict(flags=2), "flag"),
                     (dict(prior=None), "null prior"), (dict(guide=None), "null guide"),
                     (dict(guide=G + 2), "aligned"), (dict(pitch=7), "guide_pitch"),
                     (dict(prows=0), "empty prior"), (dict(rows=-1), "negative")):
        rcs, msg = call(**kw)
        assert rcs == (_lib.BICOS_E_ARG, _lib.BICOS_E_ARG), (kw, rcs, msg)
        assert word in msg, (kw, msg)


# -------------------------------------------------------------------- Python
def test_python_validation_raises(blib):
    assert _lib.guide_params(3) == (3, 0, 1, -32767, 32767)
    assert _lib.guide_params(0, 7, 8, (5, 4)) == (0, 7, 8, 5, 4)
    assert _lib.guide_params(32767, fallback=(-32768, 32767))[3:] == (-32768, 32767)
    for bad in (dict(radius=-1), dict(radius=32768), dict(radius=1.5), dict(radius=True),
                dict(radius=0, spread=8), dict(radius=0, spread=-1), dict(radius=0, scale=0),
                dict(radius=0, scale=9), dict(radius=0, fallback=(1,)),
                dict(radius=0, fallback=(0, 40000)), dict(radius=0, fallback=7)):
        with pytest.raises(ValueError):
            _lib.guide_params(**bad)
    assert _lib.guide_window(None) == (INT_MIN, INT_MAX)
    assert _lib.guide_window((3, 9)) == (3, 9)
    with pytest.raises(ValueError):
        _lib.guide_window((9, 3))
    _lib.check_guide_shape((4, 16, 2), 4, 16)
    for shape in ((4, 16), (4, 16, 1), (16, 4, 2), (4, 32)):
        with pytest.raises(ValueError, match="guide"):
            _lib.check_guide_shape(shape, 4, 16)
    assert _lib.guide_shape(None, (5, 70), 3) == (15, 210)
    assert _lib.guide_shape((16, 215), (5, 70), 3) == (16, 215)
    for bad in ((1,), 7, (-1, 4), (2 ** 16, 2 ** 16)):
        with pytest.raises(ValueError):
            _lib.guide_shape(bad, (5, 70), 1)


def test_pybicos_refuses_a_bad_guide_and_several_gpus(blib):
    from libbicos_amd import pybicos
    imgs = [np.zeros((4, 16), np.uint8)] * 4
    good = np.zeros((4, 16, 2), np.int16)
    with pytest.raises(ValueError, match="several GPUs"):
        pybicos.match(imgs, imgs, pybicos.Config(), devices=[0, 1], guide=good)
    with pytest.raises(ValueError, match="int16"):
        pybicos.match(imgs, imgs, pybicos.Config(), guide=good.astype(np.int32))
    with pytest.raises(ValueError, match="guide must have shape"):
        pybicos.match(imgs, imgs, pybicos.Config(), guide=np.zeros((4, 16), np.int16))
    with pytest.raises(ValueError):
        pybicos.guide_from_disparity(np.zeros((4, 4), np.uint8), 1)
    with pytest.raises(ValueError):
        pybicos.guide_from_disparity(np.zeros((4, 4), np.int16), radius=-1)


def test_match_bands_refuses_a_guide(blib):
    from libbicos_amd import device
    with pytest.raises(ValueError, match="guide is not supported with several GPUs"):
        device.match_bands([], [], device.MatchConfig(), guide=object())
