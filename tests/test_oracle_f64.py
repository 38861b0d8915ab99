"""CPU tests of the float64 oracle (oracle/bicos_oracle.c, the *_f64 functions): the
statement of Precision::DOUBLE that the GPU's double kernels are held to byte for byte
(tests/test_double_gpu.py).

The reference has DOUBLE only in its CUDA build (include/impl/cuda/agree.cuh:35-65,
:110-259), so no reference binary can stand behind the oracle here. Instead:
(1) the C functions equal an exact-rational restatement (oracle/ref_exact.py: every fma,
    division and sqrt rounded once from exact arithmetic) bit for bit, in both oracle builds
    (libm fma without -march, hardware fma with -march=x86-64-v3);
(2) known answers that need neither: exactly representable variances at the strict
    min-variance boundary, the -1 threshold, NaN passing, argmax ties, a single x step;
(3) the float threshold compared in double: pixels are found on which narrowing the
    correlation to float changes the decision -- the GPU tests run the same thresholds.
"""
import math

import numpy as np
import pytest

from libbicos_amd.synthetic import random_stack
from oracle import ref_exact as X
from oracle import ref_numpy as N
from tests import double_cases as D
from tests.double_cases import same

BUILDS = ["", "v3"]
INVALID = -32768


def _bits(v):
    return np.float64(v).view(np.uint64)


def _eq1(got, want):
    """One double against one: the same bits, or both NaN."""
    return (math.isnan(got) and math.isnan(want)) or _bits(got) == _bits(want)


# ---------------------------------------------------------------- the exact helpers
def test_exact_sqrt_and_fma_known_values():
    # perfect squares, a square's neighbours (the sticky bit decides), and fma's one rounding
    for v in (0.0, 1.0, 4.0, 2.25, 2.0 ** 80, 3.0, 2.0, 1e22, 65535.0 ** 2 * 65):
        assert _bits(X.sqrt(v)) == _bits(math.sqrt(v)), v
    s = 1.0 + 2.0 ** -52
    sq = X.mul(s, s)  # (1 + u)^2 rounded
    assert X.sqrt(sq) == s
    assert X.sqrt(math.nextafter(1.0, 0.0)) == math.nextafter(1.0, 0.0)  # sqrt(1 - u/2) -> 1 - u/2
    # fma(a, a, -RN(a a)) is the product's rounding error: nonzero, which a * a - p is not
    a = 1.0 + 2.0 ** -30
    p = X.mul(a, a)
    assert X.fma(a, a, -p) == 2.0 ** -60
    assert X.div(1.0, 3.0) == 1.0 / 3.0 and math.isnan(X.div(0.0, 0.0))


# --------------------------------------------------------------------------- nxcorr
def _nxc_vectors(n, dt):
    top = 255 if dt == np.uint8 else 65535
    rng = np.random.default_rng(1000 * n + top)
    out = []
    for _ in range(12):  # full range
        out.append((rng.integers(0, top + 1, n), rng.integers(0, top + 1, n)))
    a = rng.integers(0, top + 1, n)
    a[0], a[-1] = 0, top
    b = a.copy()
    b[n // 2] ^= 1
    half = a // 2
    out += [(a, a.copy()),                      # identical: |corr| within an ulp of 1
            (a, top - a),                       # mirrored: within an ulp of -1
            (a, b),                             # one sample one step off
            (half, half + top // 2),            # shifted by a constant
            (half, 2 * half),                   # scaled
            (np.full(n, 7), np.full(n, top)),   # both constant: 0 / 0
            (np.full(n, top), rng.integers(0, top + 1, n)),   # one constant side
            (rng.integers(0, top + 1, n), np.zeros(n, np.int64))]
    return [(p.astype(dt), q.astype(dt)) for p, q in out]


@pytest.mark.parametrize("dt", [np.uint8, np.uint16])
@pytest.mark.parametrize("n", [2, 3, 7, 8, 9, 33, 64, 65])
def test_nxcorr_f64_equals_exact(oracle, n, dt):
    seen_nan = seen_near_one = False
    for p, q in _nxc_vectors(n, dt):
        # min-variance: off, tiny, and a value that rejects some of the random vectors
        v_mid = np.float32(n) * np.float32(0.25 * (255.0 if dt == np.uint8 else 65535.0)) ** 2
        for mv in (None, np.float32(0.5), v_mid):
            want = X.nxcorr(p, q, mv)
            for b in BUILDS:
                got = oracle.nxcorr_f64(p, q, None if mv is None else float(mv), variant=b)
                assert _eq1(got, want), (n, dt, p, q, mv, b, got, want)
            seen_nan |= math.isnan(want)
            seen_near_one |= abs(want) == 1.0 or 0 < 1.0 - abs(want) < 1e-15
    assert seen_nan and seen_near_one


# ---------------------------------------------------------------- agree / subpixel
def _sample(H, W, raw, k, seed):
    """Pixels to restate exactly: the columns with col1 in {0, W - 1}, the off-row and
    extreme disparities of mixed_raw, every invalid pixel of row 0, and k random ones."""
    rng = np.random.default_rng(seed)
    px = {(r, c) for r in range(H) for c in (0, 1, 2, 3, 5, W - 2, W - 1)}
    px |= {(0, c) for c in range(W) if raw[0, c] == INVALID}
    px |= {(int(r), int(c)) for r, c in zip(rng.integers(0, H, k), rng.integers(0, W, k))}
    rows, cols = zip(*sorted(px))
    return sorted(px), (np.array(rows), np.array(cols))


@pytest.mark.parametrize("n,dt,minvar", [(2, np.uint8, None), (9, np.uint16, None),
                                         (33, np.uint8, 5000.0), (65, np.uint16, 3.0e8)])
def test_agree_f64_equals_exact(oracle, n, dt, minvar):
    H, W = 3, 40
    L = random_stack(n, H, W, dt, seed=n)
    R = random_stack(n, H, W, dt, seed=n + 1)
    R[:, 1, 10] = 9                      # a constant right pixel: NaN
    raw = D.mixed_raw(H, W, seed=n)
    raw[1, 14] = 4                       # ... which (1, 14) is matched to
    mv = None if minvar is None else float(np.float32(minvar) * np.float32(n))
    px, idx = _sample(H, W, raw, 60, n)
    px.append((1, 14))
    idx = (np.append(idx[0], 1), np.append(idx[1], 14))
    for thr in (0.3, 0.0, -1.0):
        wd, wc = X.agree(raw, L, R, thr, mv, px)
        for b in BUILDS:
            gd, gc = oracle.agree_f64(raw, L, R, thr, mv, variant=b)
            same(gd[idx], wd[idx])
            same(gc[idx], wc[idx])
    if mv is None:
        assert np.isnan(wc[1, 14]) and wd[1, 14] == 4      # NaN passes, disparity kept
    else:
        assert wc[1, 14] == -1.0 and wd[1, 14] == 4        # variance 0 < min-variance first
        assert (wc[idx] == -1.0).sum() > 1 and (wc[idx] > -1.0).any()  # rejects some, not all
    assert (wd[idx] == INVALID).any() and (wd[idx] != INVALID).any()
    assert (raw[idx] == INVALID).any() and wd[0, 5] == INVALID and wd[0, W - 2] == INVALID


@pytest.mark.parametrize("n,dt,step,minvar", [
    (8, np.uint8, 0.1, None), (3, np.uint16, 0.1, 2.0e7), (17, np.uint16, 0.25, None),
    (6, np.uint8, 0.25, 300.0), (12, np.uint8, 0.7, None), (33, np.uint8, 1.0, None),
    (65, np.uint16, 2.0, 3.0e8), (41, np.uint8, 3.0, None), (2, np.uint8, 0.7, 50.0)])
def test_agree_subpixel_f64_equals_exact(oracle, n, dt, step, minvar):
    H, W = 3, 40
    L = random_stack(n, H, W, dt, seed=2 * n)
    R = random_stack(n, H, W, dt, seed=2 * n + 1)
    raw = D.mixed_raw(H, W, seed=n + 7)
    mv = None if minvar is None else float(np.float32(minvar) * np.float32(n))
    px, idx = _sample(H, W, raw, 40, n)
    wo, wc = X.agree_subpixel(raw, L, R, 0.1, step, mv, px)
    for b in BUILDS:
        go, gc = oracle.agree_subpixel_f64(raw, L, R, 0.1, step, mv, variant=b)
        same(go[idx], wo[idx])
        same(gc[idx], wc[idx])
    assert np.isnan(wo[idx]).any() and np.isfinite(wo[idx]).any()
    assert np.isfinite(wc[:, 3]).any() and np.isfinite(wc[:, W - 1]).any()   # both edges ran


def test_the_two_builds_agree_on_whole_maps(oracle):
    """Beyond the sampled pixels: every pixel of small maps, both builds, all four
    functions (libm fma against hardware fma)."""
    for n, dt in ((7, np.uint8), (34, np.uint16)):
        L = random_stack(n, 6, 90, dt, seed=n)
        R = random_stack(n, 6, 90, dt, seed=n + 1)
        raw = D.mixed_raw(6, 90, seed=n)
        mv = float(np.float32(100.0 if dt == np.uint8 else 1e7) * np.float32(n))
        a = [oracle.agree_f64(raw, L, R, 0.2, mv, variant=b) for b in BUILDS]
        s = [oracle.agree_subpixel_f64(raw, L, R, 0.2, 0.1, mv, variant=b) for b in BUILDS]
        for k in range(2):
            same(a[0][k], a[1][k])
            same(s[0][k], s[1][k])
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(12, 8, 200, np.uint16, dmin=3, drange=20, seed=3)
    for kw in (dict(nxcorr_threshold=0.7), dict(nxcorr_threshold=0.7, subpixel_step=0.25,
                                                min_variance=10.0, variant=1)):
        m = [oracle.match_f64(L, R, oracle.OracleConfig(**kw), variant=b) for b in BUILDS]
        same(m[0][0], m[1][0])
        same(m[0][1], m[1][1])


def test_match_f64_is_search_then_agree_f64(oracle):
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(9, 6, 160, np.uint8, dmin=3, drange=20, seed=9)
    raw, none = oracle.match_f64(L, R, oracle.OracleConfig(nxcorr_threshold=None))
    assert none is None
    same(raw, oracle.match(L, R, oracle.OracleConfig(nxcorr_threshold=None))[0])
    d, c = oracle.match_f64(L, R, oracle.OracleConfig(nxcorr_threshold=0.9, min_variance=5.0))
    mv = float(np.float32(5.0) * np.float32(9))
    wd, wc = oracle.agree_f64(raw, L, R, 0.9, mv)
    assert c.dtype == np.float64 and d.dtype == np.float32
    same(d, wd.astype(np.float32))
    same(c, wc)
    d, c = oracle.match_f64(L, R, oracle.OracleConfig(nxcorr_threshold=0.9, subpixel_step=0.25))
    wo, wc = oracle.agree_subpixel_f64(raw, L, R, 0.9, 0.25, None)
    same(d, wo)
    same(c, wc)
    # the float match is untouched by the new entry
    f, fc = oracle.match(L, R, oracle.OracleConfig(nxcorr_threshold=0.9))
    assert fc.dtype == np.float32
    assert np.nanmax(np.abs(fc.astype(np.float64) - oracle.agree_f64(raw, L, R, 0.9, None)[1])) < 1e-4


# ------------------------------------------------ known answers that need no oracle
@pytest.mark.parametrize("dt", [np.uint8, np.uint16])
def test_minvar_boundary_is_strict(oracle, dt):
    L, R, raw, vl, vr = D.minvar_boundary(dt)
    W = raw.shape[1]
    # n = 2, diffs -k, +k and -m, +m: covariance 2 k m, correlation exactly 1
    for c in range(W):
        assert oracle.nxcorr_f64(L[:, 0, c], R[:, 0, c]) == 1.0
    for c in range(W):
        v = min(vl[c], vr[c])             # the smaller variance decides
        at = np.float32(v)
        assert float(at) == v             # exactly representable
        above = np.nextafter(at, np.float32(np.inf))
        for b in BUILDS:
            assert oracle.nxcorr_f64(L[:, 0, c], R[:, 0, c], float(at), variant=b) == 1.0
            got = oracle.nxcorr_f64(L[:, 0, c], R[:, 0, c], float(above), variant=b)
            assert got == -1.0
        assert X.nxcorr(L[:, 0, c], R[:, 0, c], at) == 1.0
        assert X.nxcorr(L[:, 0, c], R[:, 0, c], above) == -1.0
    # through the agree: at the boundary of the row's smallest variance nothing is rejected;
    # one float step above it exactly the pixels holding that variance are
    v = np.minimum(vl, vr)
    at = np.float32(v.min())
    d, corr = oracle.agree_f64(raw, L, R, 0.5, float(at))
    assert (d == 0).all() and (corr == 1.0).all()
    d, corr = oracle.agree_f64(raw, L, R, 0.5, float(np.nextafter(at, np.float32(np.inf))))
    hit = v == v.min()
    assert hit.any() and not hit.all()
    assert (corr[0, hit] == -1.0).all() and (d[0, hit] == INVALID).all()
    assert (corr[0, ~hit] == 1.0).all() and (d[0, ~hit] == 0).all()


def test_threshold_minus_one_keeps_minus_one(oracle):
    a = np.array([10, 30, 20, 200], np.uint8)
    b = (np.uint8(255) - a).astype(np.uint8)          # mirrored: correlation -1
    c = oracle.nxcorr_f64(a, b)
    assert c == -1.0 == X.nxcorr(a, b)
    L = a.reshape(4, 1, 1).repeat(2, axis=2)
    R = b.reshape(4, 1, 1).repeat(2, axis=2)
    raw = np.zeros((1, 2), np.int16)
    d, corr = oracle.agree_f64(raw, L, R, -1.0, None)
    assert (d == 0).all() and (corr == -1.0).all()     # -1 < -1 is false: kept
    above = float(np.nextafter(np.float32(-1.0), np.float32(0.0)))
    d, corr = oracle.agree_f64(raw, L, R, above, None)
    assert (d == INVALID).all() and (corr == -1.0).all()
    # min-variance rejection is the same -1.0, kept only by a threshold <= -1
    d, corr = oracle.agree_f64(raw, L, R, -1.0, 1e9)
    assert (d == 0).all() and (corr == -1.0).all()
    o, corr = oracle.agree_subpixel_f64(raw, L, R, -1.0, 0.25, 1e9)
    assert (o == 0.0).all() and (corr == -1.0).all()


def test_constant_patch_is_nan_and_passes_every_threshold(oracle):
    L = random_stack(5, 1, 6, seed=1)
    R = random_stack(5, 1, 6, seed=2)
    R[:, 0, 2] = 77
    L[:, 0, 4] = 3
    raw = np.zeros((1, 6), np.int16)
    for thr in (-1.0, 0.0, 0.999, 1.0, 3.0e38):
        d, corr = oracle.agree_f64(raw, L, R, thr, None)
        assert np.isnan(corr[0, 2]) and np.isnan(corr[0, 4])
        assert d[0, 2] == 0 and d[0, 4] == 0
    assert (d[0, [0, 1, 3, 5]] == INVALID).all()       # nothing finite passes 3e38
    assert math.isnan(X.nxcorr(L[:, 0, 2], R[:, 0, 2]))


@pytest.mark.parametrize("n,dt", [(6, np.uint8), (17, np.uint16), (40, np.uint8)])
@pytest.mark.parametrize("step", [0.25, 0.5])
def test_symmetric_neighbours_first_maximum_wins(oracle, n, dt, step):
    """y0 == y2 on every plane: B = 0 and the parabola is even, so x and -x (both among the
    steps: -1 + k step is exact for these steps) interpolate the same samples and tie; the
    strict 'best < nxc' keeps the first, so best_x <= 0 everywhere."""
    L, R, raw = D.symmetric_rows(n, dt)
    xs = [float(x) for x in N.x_steps(step)]
    assert xs == [-x for x in reversed(xs)]
    out, corr = oracle.agree_subpixel_f64(raw, L, R, -1.0, step, None)
    best_x = raw.astype(np.float32) - out
    assert np.isfinite(out).all()
    assert (best_x <= 0).all()
    assert (best_x < 0).any()      # some maxima lie off the centre: the tie was real
    H, W = raw.shape
    px = [(r, c) for r in range(H) for c in range(0, W, 5)]
    wo, wc, wx = X.agree_subpixel(raw, L, R, -1.0, step, None, px, want_best_x=True)
    idx = tuple(np.array(px).T)
    same(out[idx], wo[idx])
    same(corr[idx], wc[idx])
    assert (wx[idx] <= 0).all()


def test_step_three_evaluates_minus_one_only(oracle):
    """step 3: x = -1 alone; A - B + C = y0 exactly, so the refine is the plain correlation
    with the left neighbour and the disparity moves by exactly +1 where that beats -1."""
    n, H, W = 9, 2, 30
    assert [float(x) for x in N.x_steps(3.0)] == [-1.0]
    L = random_stack(n, H, W, np.uint16, seed=31)
    R = random_stack(n, H, W, np.uint16, seed=32)
    raw = np.full((H, W), 2, np.int16)
    out, corr = oracle.agree_subpixel_f64(raw, L, R, -1.0, 3.0, None)
    for r in range(H):
        for c in range(4, W):           # col1 = c - 2 >= 2: interior
            want = oracle.nxcorr_f64(L[:, r, c], R[:, r, c - 3])
            assert _bits(corr[r, c]) == _bits(want)
            assert want > -1.0 and out[r, c] == 3.0


# ------------------------------------------------------ the float threshold in double
def test_float_threshold_is_compared_in_double(oracle):
    """Thresholds are float32 values next to pixels' float64 correlations. Where the
    correlation c lies strictly between T's float32 neighbours and rounds to T from below,
    'c < (double)T' rejects and '(float)c < T' keeps: a kernel that narrows is wrong there.
    The GPU test runs these very thresholds (tests/double_cases.py threshold_cases)."""
    L, R, raw, corr, ts, up, down = D.threshold_cases()
    assert len(up) == 3 and len(down) == 3 and len(ts) >= 6, (up, down, ts)
    assert all(t.dtype == np.float32 and 0 < t < 1 for t in ts)
    differing = 0
    for T in ts:
        lo = float(np.nextafter(T, np.float32(-np.inf)))
        hi = float(np.nextafter(T, np.float32(np.inf)))
        between = (corr > lo) & (corr < hi) & (corr != float(T))
        assert between.any(), T              # each threshold has a pixel within one float step
        d, c2 = oracle.agree_f64(raw, L, R, float(T), None)
        same(c2, corr)                       # the threshold does not touch the corrmap
        dbl = corr < float(T)
        assert np.array_equal(d == INVALID, (raw == INVALID) | _off_row(raw) | dbl)
        narrowed = corr.astype(np.float32) < T
        differing += int((between & (dbl != narrowed)).sum())
    for (r, c), T in up:
        v = corr[r, c]
        assert float(np.nextafter(T, np.float32(-np.inf))) < v < float(T)   # strictly between
        assert np.float32(v) == T
        assert (v < float(T)) and not (np.float32(v) < T)                   # the decisions differ
        d, _ = oracle.agree_f64(raw, L, R, float(T), None)
        assert d[r, c] == INVALID and raw[r, c] != INVALID
        # the exact restatement agrees on the correlation and on the verdict
        wd, wc = X.agree(raw, L, R, float(T), None, [(r, c)])
        assert _bits(wc[r, c]) == _bits(v) and wd[r, c] == INVALID
    for (r, c), T in down:
        v = corr[r, c]
        assert float(T) < v < float(np.nextafter(T, np.float32(np.inf)))
        d, _ = oracle.agree_f64(raw, L, R, float(T), None)
        assert d[r, c] == raw[r, c] != INVALID
    assert differing >= len(up)


def _off_row(raw):
    W = raw.shape[1]
    col1 = np.arange(W)[None, :] - raw.astype(np.int64)
    return (raw != INVALID) & ((col1 < 0) | (col1 >= W))
