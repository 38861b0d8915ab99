"""The disparity-range interface without a GPU: the three *_range C-ABI symbols and their
argument check (min > max is BICOS_E_ARG before any HIP call), the Python configuration
objects, and a self-check of the windowed-search restatement that tests/test_range_gpu.py
compares the kernels against (include/bicos_c.h, "disparity range").
"""
import ctypes

import numpy as np
import pytest

from libbicos_amd import _lib
from libbicos_amd.synthetic import random_descriptors
from oracle import ref_numpy as N

RANGE_SYMBOLS = ("bicos_match_device_range", "bicos_match_host_range",
                 "bicos_search_device_range")


# ---------------------------------------------------------------- the restatement
def _argmin_win(cost, mask, nodupes):
    BIG = 1 << 20
    c = np.where(mask, cost, BIG)
    best = np.argmin(c, axis=1)
    mins = c[np.arange(c.shape[0]), best]
    ok = mins < BIG
    if nodupes:
        ok &= (c == mins[:, None]).sum(axis=1) == 1
    return np.where(ok, best, -1)


def search_range(d0, d1, flags, dmin, dmax, max_lr_diff=-1):
    """bicos_search (reference bicos.hpp:50-113) with the candidates of col0 restricted to
    the col1 with dmin <= col0 - col1 <= dmax, both ways for Consistency."""
    H, W, _ = d0.shape
    out = np.full((H, W), -32768, np.int16)
    col0 = np.arange(W)
    dd = col0[:, None] - col0[None, :]
    mask = (dd >= dmin) & (dd <= dmax)
    for r in range(H):
        cost = N._row_costs(d0[r], d1[r])
        fwd = _argmin_win(cost, mask, bool(flags & 1))
        ok = fwd >= 0
        if flags & 2:
            rev = _argmin_win(cost.T, mask.T, bool(flags & 1))
            r0 = np.where(ok, rev[np.maximum(fwd, 0)], -1)
            ok &= (r0 >= 0) & (np.abs(col0 - r0) <= max_lr_diff)
            val = (col0 + r0) // 2 - fwd
        else:
            val = col0 - fwd
        out[r] = np.where(ok, val, -32768).astype(np.int16)
    return out


def rolled_descriptors(H, W, words, period=None, low_bits=None):
    """d0 random (synthetic.random_descriptors), d1 = d0 rolled by 20 columns; low_bits keeps
    only that many low bits of word 0 (ties)."""
    d0 = random_descriptors(H, W, words, period=period)
    if low_bits:
        d0 = d0 & np.uint32((1 << low_bits) - 1)
    if words == 8:  # transform output never sets bit 255 (include/bicos_c.h)
        d0[..., 7] &= np.uint32(0x7FFFFFFF)
    d1 = np.ascontiguousarray(np.roll(d0, 20, axis=1))
    return d0, d1


@pytest.mark.parametrize("flags,lr", [(1, -1), (2, 1), (3, 2)])
@pytest.mark.parametrize("words,period,low", [(1, None, 10), (4, 97, None), (8, None, None)])
def test_restatement_with_the_covering_range_is_the_full_search(flags, lr, words, period, low):
    H, W = 2, 150
    d0, d1 = rolled_descriptors(H, W, words, period, low)
    got = search_range(d0, d1, flags, -(W - 1), W - 1, lr)
    assert np.array_equal(got, N.search(d0, d1, flags, lr))


def test_restatement_window_changes_the_result():
    """a period-97 row loses every pixel to NoDuplicates unrestricted (each exact match at
    disparity -20 repeats 97 columns away); a window shorter than the period that holds -20
    keeps every pixel whose match lies in the row, at that disparity (but for the first 10
    columns: the 20 columns rolled in from the row's end have phases 87..96, 0..9, so those
    ten find their descriptor a second time at disparity -10)"""
    W = 301
    d0, d1 = rolled_descriptors(1, W, 4, period=97)
    full = N.search(d0, d1, 1)
    win = search_range(d0, d1, 1, -63, 0)
    assert (full != -32768).mean() == 0.0
    assert (win[0, 10: W - 20] == -20).all()


# --------------------------------------------------------------------- C-ABI
def test_range_symbols_are_exported_and_declared(blib):
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "bicos_c.h")).read()
    for s in RANGE_SYMBOLS:
        assert hasattr(blib, s), s
        assert s in _lib.EXPORTS, s
        assert ("int %s(" % s) in header, s


def test_search_range_min_above_max_is_an_argument_error(blib):
    """checked before any HIP call: a NULL engine, NULL buffers and no GPU are fine"""
    rc = blib.bicos_search_device_range(None, None, None, 4, 64, 4, 1, -1, 5, 4, None, None)
    assert rc == _lib.BICOS_E_ARG
    msg = blib.bicos_last_error().decode()
    assert "disparity" in msg and "5" in msg and "4" in msg


def test_match_range_min_above_max_is_an_argument_error(blib):
    cfg = _lib.BicosConfig(0.5, -1.0, -1.0, 0, 0, 0, 1, 0)
    rc = blib.bicos_match_device_range(None, None, None, 8, 4, 64, 64, 256, 1, ctypes.byref(cfg),
                                       1, 5, 4, None, None, None)
    assert rc == _lib.BICOS_E_ARG
    assert "disparity" in blib.bicos_last_error().decode()
    rc = blib.bicos_match_host_range(None, None, None, 8, 4, 64, 0, 1, ctypes.byref(cfg), 1,
                                     5, 4, None, None)
    assert rc == _lib.BICOS_E_ARG
    assert "disparity" in blib.bicos_last_error().decode()


def test_consistency_search_range_needs_an_engine(blib):
    rc = blib.bicos_search_device_range(None, None, None, 4, 64, 4, 2, 1, 0, 4, None, None)
    assert rc == _lib.BICOS_E_ARG
    assert "engine" in blib.bicos_last_error().decode()


# -------------------------------------------------------------------- Python
def test_match_config_validates_the_range(blib):
    from libbicos_amd.device import MatchConfig
    assert MatchConfig().disparity_range is None
    MatchConfig(disparity_range=(4, 5)).to_c()
    MatchConfig(disparity_range=(-7, -7)).to_c()
    c0, nx0 = MatchConfig().to_c()
    c1, nx1 = MatchConfig(disparity_range=(0, 63)).to_c()
    assert bytes(c0) == bytes(c1) and nx0 == nx1  # BicosConfig itself does not change
    for bad in ((5, 4), (0.5, 3), ("0", 3), (1,), (1, 2, 3), 7):
        with pytest.raises(ValueError):
            MatchConfig(disparity_range=bad).to_c()


def test_pybicos_config_range_property(blib):
    from libbicos_amd import pybicos
    cfg = pybicos.Config()
    assert cfg.disparity_range is None
    cfg.disparity_range = (8, 71)
    assert cfg.disparity_range == (8, 71)
    cfg.disparity_range = None
    assert cfg.disparity_range is None
    with pytest.raises(ValueError):
        cfg.disparity_range = (5, 4)
    with pytest.raises(ValueError):
        cfg.disparity_range = (1.5, 4)
    assert cfg.disparity_range is None


def test_range_is_refused_with_several_gpus(blib):
    from libbicos_amd import pybicos
    cfg = pybicos.Config()
    cfg.disparity_range = (0, 7)
    imgs = [np.zeros((4, 16), np.uint8)] * 4
    with pytest.raises(ValueError, match="several GPUs"):
        pybicos.match(imgs, imgs, cfg, devices=[0, 1])


def test_match_bands_refuses_a_range(blib):
    from libbicos_amd import device
    with pytest.raises(ValueError, match="disparity_range is not supported with several GPUs yet"):
        device.match_bands([], [], device.MatchConfig(disparity_range=(0, 7)))
