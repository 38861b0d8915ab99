"""Precision::DOUBLE on the GPU against the float64 oracle, byte for byte.

The oracle (oracle/bicos_oracle.c *_f64) states agree.cuh's operation order in IEEE double
and is itself held to exact rational arithmetic (tests/test_oracle_f64.py). Here every
double kernel instantiation family is launched and compared with it: no tolerance, no pixel
left out (same(): bit equality; only a NaN's payload may differ). Kernels are driven through
Engine.agree(..., precision=1) on raw disparity maps a search would never give, and through
Engine.match(MatchConfig(precision=1)) where the engine's plan matters.

Which case launches which family (u8 and u16 each):
  agree_lds_kernel<.., double, MAXN>          test_agree_buckets (W = 260), ..._tile_and_tiny_widths
  agree_lds_kernel<.., double, MAXN, CONS>    test_match_consistency_in_agree
  agree_reg_kernel<.., double, MAXN, exact>   test_agree_buckets (W = 257, n = 8/16/24/33/40/48/65)
  agree_reg_kernel<.., double, MAXN, padded>  test_agree_buckets (W = 257, the other n)
  agree_kernel<.., double>                    test_agree_buckets (n = 66, 100)
  launch_subpixel_m<.., double, 6|10|12, =>   test_subpixel_buckets (n = 6, 10, 12)
  launch_subpixel_m<.., double, 8|16|24|33|40, LO>  test_subpixel_buckets (both ends of each)
  launch_subpixel_m<.., double, 48|56|65, LO> (subpixel_wide.hip)  test_subpixel_buckets
"""
import numpy as np
import pytest

from libbicos_amd import _lib
from libbicos_amd.synthetic import random_stack, stereo_stack
from tests import double_cases as D
from tests.double_cases import same

pytestmark = pytest.mark.gpu

INVALID = -32768
U8, U16 = np.uint8, np.uint16


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def dev_pitched(a, P):
    """The stack as a view of a [n, H, P] buffer: row pitch P, plane pitch H P elements."""
    import torch
    t = dev(a)
    n, H, W = t.shape
    buf = torch.zeros((n, H, P), dtype=t.dtype, device="cuda")
    buf[:, :, :W] = t
    return buf[:, :, :W]


def host(t):
    return t.cpu().numpy()


def scaled(minvar, n):
    return None if minvar is None else float(np.float32(minvar) * np.float32(n))


def check_agree(gpu, oracle, raw, L, R, thr, mv, pitch=None):
    """The DOUBLE agree stage on (raw, L, R) == agree_f64, disparity and corrmap."""
    s0, s1 = (dev(L), dev(R)) if pitch is None else (dev_pitched(L, pitch), dev_pitched(R, pitch))
    out, corr = gpu.agree(dev(raw), s0, s1, thr, mv, precision=1)
    rd, rc = oracle.agree_f64(raw, L, R, thr, mv)
    got = host(corr)
    assert got.dtype == np.float64
    same(host(out), rd.astype(np.float32))
    same(got, rc)
    return rd, rc


def check_subpixel(gpu, oracle, raw, L, R, thr, step, mv):
    out, corr = gpu.agree(dev(raw), dev(L), dev(R), thr, mv, step=step, precision=1)
    ro, rc = oracle.agree_subpixel_f64(raw, L, R, thr, step, mv)
    got = host(corr)
    assert got.dtype == np.float64
    same(host(out), ro)
    same(got, rc)
    return ro, rc


def full_range(n, H, W, dt, seed):
    """Random samples over the whole type (u16 up to 65535), the extremes present."""
    s = random_stack(n, H, W, dt, seed=seed)
    s[0, 0, 0], s[n - 1, 0, 0] = 0, np.iinfo(dt).max
    return s


# ------------------------------------------------------------ agree without subpixel
# Both sides of every launch_agree_t bucket, and past the last (the generic kernel). W = 260:
# row and plane pitch multiples of 4 bytes for both types (agree_lds_kernel), two tiles. W =
# 257: odd, so neither pitch is (agree_reg_kernel; n == MAXN takes its exact form), two tiles.
# Thresholds next to the correlations of unrelated samples (around 0), so both verdicts occur.
@pytest.mark.parametrize("dt", [U8, U16])
@pytest.mark.parametrize("n", [2, 8, 9, 16, 17, 24, 25, 33, 34, 40, 41, 48, 49, 65, 66, 100])
def test_agree_buckets(gpu, oracle, n, dt):
    H = 3
    top = float(np.iinfo(dt).max)
    for W in (260, 257):
        L = full_range(n, H, W, dt, seed=10 * n + W)
        R = full_range(n, H, W, dt, seed=10 * n + W + 1)
        R[:, 0, 40] = 9                    # a constant right pixel ...
        raw = D.mixed_raw(H, W, seed=n + W)
        raw[0, 45] = 5                     # ... that (0, 45) is matched to: NaN, kept
        for thr, minvar in ((0.05, None), (-0.1, top * top / 12.5)):
            # (min-variance just below the variance of uniform samples, top^2 / 12: rejects
            # some pixels and keeps others)
            rd, rc = check_agree(gpu, oracle, raw, L, R, thr, scaled(minvar, n))
            kept = rd != INVALID
            assert kept.any() and (~kept & np.isfinite(rc)).any()
            if minvar is None:
                assert np.isnan(rc[0, 45]) and rd[0, 45] == 5
            else:
                assert (rc == -1.0).sum() > 1 and (rc > -1.0).any()


# One width per kernel across the 256-column tile, and images of 1 and 3 columns; the LDS
# kernel sees the odd widths through a pitch of 4 bytes' multiple. n = 8 / 16 are n == MAXN.
@pytest.mark.parametrize("dt", [U8, U16])
@pytest.mark.parametrize("n", [8, 16, 17])
def test_agree_tile_and_tiny_widths(gpu, oracle, n, dt):
    H = 4
    for W, pitch in ((259, None), (259, 260), (257, 264), (1, None), (3, None), (1, 4), (3, 4)):
        L = full_range(n, H, W, dt, seed=n + W)
        R = full_range(n, H, W, dt, seed=n + W + 50)
        raw = D.mixed_raw(H, W, seed=n + W, lo=-2, hi=3)
        check_agree(gpu, oracle, raw, L, R, 0.0, None, pitch)
        check_agree(gpu, oracle, raw, L, R, 0.0, scaled(float(np.iinfo(dt).max) ** 2 / 12.5, n),
                    pitch)


def _pattern_raw(H, W, rng):
    raw = np.empty((H, W), np.int16)
    raw[0] = INVALID                                         # all invalid
    raw[1] = 0                                               # all zero
    raw[2] = np.arange(W)                                    # col1 = 0 for every pixel
    raw[3] = np.arange(W) - (W - 1)                          # col1 = W - 1 for every pixel
    raw[4] = rng.integers(-40, W + 70, size=W)               # anything: left and right of the row
    raw[5] = np.where(np.arange(W) % 64 < 32, 5, 250)        # jumps: far gathers
    raw[6] = 12
    raw[6, ::7] = INVALID                                    # invalid pixels in flat runs
    raw[7] = np.arange(W) % 9 - 4                            # negative disparities (col1 > col0)
    raw[8] = W - 1                                           # only the last column stays in the row
    raw[9] = 20 + rng.integers(-2, 3, size=W)                # jitter
    return raw


# test_agree_disparity_patterns's rows (tests/test_gpu_parity.py) and the two uniform maps
@pytest.mark.parametrize("n,dt,W", [(7, U8, 1024), (33, U8, 1021), (24, U16, 514), (40, U16, 513)])
@pytest.mark.parametrize("minvar", [None, 2.0])
def test_agree_disparity_patterns(gpu, oracle, n, dt, W, minvar):
    H = 10
    L, R = stereo_stack(n, H, W, dt, dmin=3, drange=40, seed=n + 1000,
                        maxval=int(np.iinfo(dt).max))
    raw = _pattern_raw(H, W, np.random.default_rng(n))
    R[:, 1, 40:48] = 9                                       # flat right pixels: NaN
    rd, rc = check_agree(gpu, oracle, raw, L, R, 0.5, scaled(minvar, n))
    assert (rd[0] == INVALID).all() and np.isnan(rc[0]).all()
    assert np.isfinite(rc[2]).all() and np.isfinite(rc[3]).all()
    if minvar is None:
        assert np.isnan(rc[1, 40:48]).all() and (rd[1, 40:48] == 0).all()


# Variances exactly representable (n = 2, samples {a, a + 2k}: variance 2 k^2): '<' is strict,
# so min-variance == the variance keeps the pixel and one float step above rejects it (-1.0).
@pytest.mark.parametrize("dt", [U8, U16])
def test_agree_minvar_boundary(gpu, oracle, dt):
    L8, R8, raw8, vl, vr = D.minvar_boundary(dt)
    v = np.minimum(vl, vr)
    at = np.float32(v.min())
    assert float(at) == v.min()
    above = float(np.nextafter(at, np.float32(np.inf)))
    # 8 columns: agree_lds_kernel; the first 7 of them (odd width): agree_reg_kernel
    for W in (8, 7):
        L, R, raw = L8[:, :, :W].copy(), R8[:, :, :W].copy(), raw8[:, :W].copy()
        hit = (v == v.min())[:W]
        assert hit.any() and not hit.all()
        rd, rc = check_agree(gpu, oracle, raw, L, R, 0.5, float(at))
        assert (rd == 0).all() and (rc == 1.0).all()
        rd, rc = check_agree(gpu, oracle, raw, L, R, 0.5, above)
        assert (rc[0, hit] == -1.0).all() and (rd[0, hit] == INVALID).all()
        assert (rc[0, ~hit] == 1.0).all() and (rd[0, ~hit] == 0).all()
        # -1.0 is kept by a threshold of -1.0 ('<' again)
        rd, rc = check_agree(gpu, oracle, raw, L, R, -1.0, above)
        assert (rd == 0).all() and (rc[0, hit] == -1.0).all()


# The float threshold is widened, the correlation is not narrowed: thresholds one float step
# either side of pixels' float64 correlations (tests/test_oracle_f64.py proves that on the
# `up` pixels a comparison in float decides otherwise). Pitch None: agree_lds_kernel; a pitch
# of 257 bytes: agree_reg_kernel on the same scene.
@pytest.mark.parametrize("pitch", [None, 257])
def test_agree_float_thresholds(gpu, oracle, pitch):
    L, R, raw, corr, ts, up, down = D.threshold_cases()
    assert len(up) == 3 and len(down) == 3
    verdict = {}
    for T in ts:
        rd, rc = check_agree(gpu, oracle, raw, L, R, float(T), None, pitch)
        same(rc, corr)
        verdict[float(T)] = rd              # (== the GPU's map, by check_agree)
    for (r, c), T in up:
        assert corr[r, c] < float(T) and not np.float32(corr[r, c]) < T
        assert raw[r, c] != INVALID and verdict[float(T)][r, c] == INVALID   # rejected in double
    for (r, c), T in down:
        assert verdict[float(T)][r, c] == raw[r, c] != INVALID


# --------------------------------------------------------------- agree with subpixel
def _edge_stack(n, H, W, dt, seed):
    """Rows of full-range samples, of samples within 6 of 0, within 6 of the top, and of both
    mixed: next to the ends the parabola leaves the type's range and the narrowing wraps."""
    top = int(np.iinfo(dt).max)
    s = random_stack(n, H, W, dt, seed=seed)
    lo = random_stack(n, H, W, dt, seed=seed + 1, maxval=6)
    s[:, 1] = lo[:, 1]
    s[:, 2] = top - lo[:, 2]
    s[:, 3] = np.where(np.arange(W) % 3 == 0, top - lo[:, 3], lo[:, 3])
    return s


# Every LO and MAXN of subpixel.hip and subpixel_wide.hip, the three exact depths, and n ==
# MAXN. Rows mix edge pixels (col1 in {0, W - 1}), interior ones, invalid and off-row
# disparities (mixed_raw); W = 97 columns, 4 rows.
@pytest.mark.parametrize("dt", [U8, U16])
@pytest.mark.parametrize("n", [2, 3, 6, 7, 8, 9, 10, 12, 16, 17, 24, 25, 33, 34, 40, 41, 48, 49,
                               56, 57, 65])
def test_subpixel_buckets(gpu, oracle, n, dt):
    H, W = 4, 97
    top = float(np.iinfo(dt).max)
    L = _edge_stack(n, H, W, dt, seed=5 * n)
    R = _edge_stack(n, H, W, dt, seed=5 * n + 2)
    raw = D.mixed_raw(H, W, seed=n)
    off_centre = False
    for step, minvar in ((0.1, None), (0.25, None), (0.7, None), (2.0, None),
                         (0.25, top * top / 13.0)):
        ro, rc = check_subpixel(gpu, oracle, raw, L, R, 0.0, step, scaled(minvar, n))
        assert np.isfinite(ro).any() and np.isnan(ro).any()
        assert np.isfinite(rc[:, 3]).any() and np.isfinite(rc[:, W - 1]).any()
        frac = ro[np.isfinite(ro)] % 1
        off_centre |= bool((frac != 0).any())
    assert off_centre                       # some maxima lie off x = 0


# Narrow images with every col1, as test_subpixel_narrow_images_every_col1 for float
@pytest.mark.parametrize("W", [3, 4, 5])
@pytest.mark.parametrize("n,dt", [(8, U8), (17, U16), (33, U8), (49, U16)])
def test_subpixel_narrow_images_every_col1(gpu, oracle, W, n, dt):
    H = 6
    L = random_stack(n, H, W, dt, seed=W + n)
    R = random_stack(n, H, W, dt, seed=W + n + 1)
    raw = np.empty((H, W), np.int16)
    for y in range(H):
        for x in range(W):
            raw[y, x] = x - ((x + y) % W)   # col1 = (x + y) % W: all columns appear
    check_subpixel(gpu, oracle, raw, L, R, 0.1, 0.25, None)
    check_subpixel(gpu, oracle, raw, L, R, -1.0, 0.1, None)


# Argmax ties: y0 == y2 on every plane, so x and -x tie and the first maximum (x <= 0) wins
@pytest.mark.parametrize("n,dt", [(6, U8), (17, U16), (33, U8), (40, U8), (57, U16)])
@pytest.mark.parametrize("step", [0.25, 0.5])
def test_subpixel_symmetric_neighbours(gpu, oracle, n, dt, step):
    L, R, raw = D.symmetric_rows(n, dt)
    ro, rc = check_subpixel(gpu, oracle, raw, L, R, -1.0, step, None)
    best_x = raw.astype(np.float32) - ro
    assert np.isfinite(ro).all() and (best_x <= 0).all() and (best_x < 0).any()


# Min-variance rows: row 0 rejects the left side alone (a left pixel of variance ~ n / 4);
# row 1 rejects some x steps only (the matched right column is nearly flat, its neighbours are
# not: the interpolation has little variance near x = 0 and much near +-1); row 2 is ordinary;
# then a min-variance nothing reaches: every step is rejected, corr -1.0, best_x 0, and the
# pixel is kept only by a threshold <= -1.
@pytest.mark.parametrize("n,dt", [(8, U8), (12, U8), (34, U16), (49, U8), (65, U16)])
def test_subpixel_minvar_rows(gpu, oracle, n, dt):
    H, W = 3, 64
    top = float(np.iinfo(dt).max)
    t = np.arange(n).reshape(n, 1)
    L = random_stack(n, H, W, dt, seed=n + 3)
    R = random_stack(n, H, W, dt, seed=n + 4)
    L[:, 0, :] = 100 + t % 2
    R[:, 1, 1::2] = 50 + t % 2
    raw = np.zeros((H, W), np.int16)
    raw[1] = np.arange(W) - (1 + 2 * ((np.arange(W) * 5) % 31))   # col1 odd, in [1, 61]
    raw[:, 0] = INVALID
    mv = scaled(top * top / 100.0, n)
    ro, rc = check_subpixel(gpu, oracle, raw, L, R, 0.0, 0.25, mv)
    assert (rc[0, 1:W - 1] == -1.0).all() and np.isnan(ro[0, 1:W - 1]).all()
    moved = (ro[1] - raw[1].astype(np.float32))[np.isfinite(ro[1])]
    assert (rc[1, 1:] > -1.0).all() and len(moved) and (moved != 0).all()   # x = 0 was rejected
    ro, rc = check_subpixel(gpu, oracle, raw, L, R, -1.0, 0.25, mv)
    assert (ro[0, 1:] == 0.0).all()                      # corr -1, best_x 0, kept by -1
    huge = scaled(top * top, n)
    ro, rc = check_subpixel(gpu, oracle, raw, L, R, -1.0, 0.1, huge)
    ok = raw != INVALID
    assert (rc[ok] == -1.0).all() and (ro[ok] == raw[ok].astype(np.float32)).all()
    above = float(np.nextafter(np.float32(-1.0), np.float32(0.0)))
    ro, rc = check_subpixel(gpu, oracle, raw, L, R, above, 0.1, huge)
    assert np.isnan(ro).all() and (rc[ok] == -1.0).all()


# --------------------------------------------------------------------- whole matches
def check_match(gpu, oracle, L, R, kw, i16=False):
    import torch
    from libbicos_amd.device import MatchConfig
    H, W = L.shape[1:]
    out = torch.empty((H, W), dtype=torch.int16, device="cuda") if i16 else None
    d, c = gpu.match(dev(L), dev(R), MatchConfig(precision=1, **kw), out=out)
    rd, rc = oracle.match_f64(L, R, oracle.OracleConfig(**kw))
    got = host(c)
    assert got.dtype == np.float64
    if i16:
        assert d.dtype == torch.int16
        same(host(d), rd.astype(np.int16))
        assert np.array_equal(rd.astype(np.int16).astype(np.float32), rd)
    else:
        same(host(d), rd)
    same(got, rc)
    return rd, rc


def test_match_nodupes_takes_the_separate_agree(gpu, oracle):
    """n = 33 u8: the float plan fuses the agree into the search; DOUBLE must not, and gives
    the float64 oracle's bytes"""
    from libbicos_amd.device import MatchConfig
    L, R = stereo_stack(33, 32, 512)
    L[:, 1, 100:140] = 7  # flat patch: NaN correlations pass the threshold
    s0, s1 = dev(L), dev(R)
    assert gpu.plan(s0, s1, MatchConfig(nxcorr_threshold=0.9)) & _lib.PLAN_AGREE_IN_SEARCH
    assert not gpu.plan(s0, s1, MatchConfig(nxcorr_threshold=0.9, precision=1)) & \
        _lib.PLAN_AGREE_IN_SEARCH
    rd, rc = check_match(gpu, oracle, L, R, dict(nxcorr_threshold=0.9))
    assert (rd != INVALID).mean() > 0.5 and np.isnan(rc[1, 100:140]).any()
    check_match(gpu, oracle, L, R, dict(nxcorr_threshold=0.9, min_variance=2.0))


@pytest.mark.parametrize("n,H,W,dt,kw", [
    (40, 5, 1300, U8, dict(nxcorr_threshold=0.5, variant=1, max_lr_diff=0, no_dupes=True)),
    (17, 6, 900, U16, dict(nxcorr_threshold=0.8, variant=1, max_lr_diff=2, min_variance=1.0)),
])
def test_match_consistency_in_agree(gpu, oracle, monkeypatch, n, H, W, dt, kw):
    """The CONS form of agree_lds_kernel in double (tests/test_gpu_parity.py
    test_consistency_in_agree compares it with another launch only)"""
    from libbicos_amd.device import MatchConfig
    monkeypatch.setenv("BICOS_LR_ONE_PASS", "0")
    L, R = stereo_stack(n, H, W, dt, dmin=2, drange=50, seed=n * 7 + W)
    L[:, 1, 40:90] = 5  # flat patch: NaN correlations pass
    assert gpu.plan(dev(L), dev(R), MatchConfig(precision=1, **kw)) & \
        _lib.PLAN_CONSISTENCY_IN_AGREE
    rd, rc = check_match(gpu, oracle, L, R, kw)
    assert (rd != INVALID).any() and (rd == INVALID).any()


def test_match_subpixel_minvar_u16(gpu, oracle):
    L, R = stereo_stack(12, 6, 300, U16, dmin=3, drange=30, seed=29, maxval=65535)
    L[:, 2, 50:80] //= 4096           # a patch of little variance (samples 0..15)
    R[:, 2, 30:60] //= 4096
    rd, rc = check_match(gpu, oracle, L, R, dict(nxcorr_threshold=0.5, subpixel_step=0.25,
                                                 min_variance=1000.0, mode=1))
    assert np.isfinite(rd).any() and (rc == -1.0).any()


def test_match_with_a_range(gpu, oracle):
    from libbicos_amd.device import MatchConfig
    from tests.test_range_api import search_range
    n, step = 9, 0.1
    L, R = stereo_stack(n, 4, 301, U8, dmin=3, drange=30, seed=n + 17)
    raw = search_range(oracle.transform(L, 0), oracle.transform(R, 0), 1, 2, 40)
    mv = scaled(2.0, n)
    out, corr = gpu.match(dev(L), dev(R), MatchConfig(
        nxcorr_threshold=0.5, subpixel_step=step, min_variance=2.0, precision=1,
        disparity_range=(2, 40)))
    ro, rc = oracle.agree_subpixel_f64(raw, L, R, 0.5, step, mv)
    same(host(out), ro)
    same(host(corr), rc)
    assert np.isfinite(ro).mean() > 0.3


@pytest.mark.parametrize("n,H,W,dt,kw", [
    (8, 7, 640, U8, dict(nxcorr_threshold=0.9)),
    (17, 5, 1300, U16, dict(nxcorr_threshold=0.8, min_variance=1.5)),
    (40, 4, 900, U8, dict(nxcorr_threshold=0.9, variant=1, max_lr_diff=1)),
])
def test_match_int16_entry(gpu, oracle, monkeypatch, n, H, W, dt, kw):
    """out_f32 = 0: the int16 output form of the double agree kernels"""
    monkeypatch.setenv("BICOS_LR_ONE_PASS", "0")
    L, R = stereo_stack(n, H, W, dt, dmin=3, drange=30, seed=n + H)
    L[:, 1, 100:140] = 7
    check_match(gpu, oracle, L, R, kw, i16=True)
