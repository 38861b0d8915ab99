"""Inputs shared by the Precision::DOUBLE tests (tests/test_oracle_f64.py on the CPU,
tests/test_double_gpu.py on the GPU): built once, from the float64 oracle alone, so both
files judge the same pixels."""
import functools

import numpy as np

from libbicos_amd.synthetic import random_stack, stereo_stack

INVALID = -32768


def same(a, b):
    """Bit equality of two arrays; only a NaN against a NaN at the same pixel may differ in
    its bits (0 / 0 has another sign and payload from a C library than from the device), as
    in tests/test_gpu_parity.py's same(). No tolerance otherwise: -0.0 is not 0.0."""
    assert a.shape == b.shape, (a.shape, b.shape)
    assert a.dtype == b.dtype, (a.dtype, b.dtype)
    u = "u%d" % a.itemsize
    diff = a.view(u) != b.view(u)
    if a.dtype.kind == "f":
        diff &= ~(np.isnan(a) & np.isnan(b))
    if diff.any():
        bad = np.argwhere(diff)
        raise AssertionError("%d of %d differ, first at %s: %r vs %r" % (
            len(bad), a.size, bad[0], a[tuple(bad[0])], b[tuple(bad[0])]))


# ------------------------------------------------------------ the float threshold in double
@functools.lru_cache(maxsize=None)
def threshold_scene():
    """A small stereo pair and its raw search result (the scene whose correlations the
    thresholds are taken from). u8, n = 8, 4 x 256: two agree tiles per row."""
    from oracle import oracle as O
    L, R = stereo_stack(8, 4, 256, np.uint8, dmin=3, drange=20, seed=61)
    raw, _ = O.match(L, R, O.OracleConfig(nxcorr_threshold=None))
    return L, R, raw


def float_thresholds(corr, per_kind=3):
    """From a float64 corrmap: float32 thresholds next to pixels' correlations.

    Returns (thresholds, up, down). `up`: [((row, col), T)] pixels whose correlation c
    rounds UP to the float32 T = float32(c) > c -- there 'c < (double)T' rejects the pixel
    and '(float)c < T' keeps it: the pixels a kernel that narrows the correlation gets wrong.
    `down`: pixels with T = float32(c) < c, where both keep. `thresholds`: for every chosen
    pixel both float32 neighbours of c, sorted, positive (so a match config can carry them)."""
    up, down = [], []
    H, W = corr.shape
    for i in range(H * W):
        r, c = divmod((i * 389) % (H * W), W)  # spread over rows and tiles (389 is prime)
        v = corr[r, c]
        if not (np.isfinite(v) and 0.0 < v < 1.0):
            continue
        f = np.float32(v)
        if float(f) > v and len(up) < per_kind:
            up.append(((r, c), f))
        elif float(f) < v and len(down) < per_kind:
            down.append(((r, c), f))
    ts = set()
    for _, f in up:
        ts |= {float(f), float(np.nextafter(f, np.float32(-np.inf)))}
    for _, f in down:
        ts |= {float(f), float(np.nextafter(f, np.float32(np.inf)))}
    return [np.float32(t) for t in sorted(ts)], up, down


@functools.lru_cache(maxsize=None)
def threshold_cases():
    """(L, R, raw, thresholds, up, down) of threshold_scene(), from agree_f64 alone."""
    from oracle import oracle as O
    L, R, raw = threshold_scene()
    _, corr = O.agree_f64(raw, L, R, -2.0, None)  # -2: below every correlation, keeps all
    ts, up, down = float_thresholds(corr)
    return L, R, raw, corr, ts, up, down


# ------------------------------------------------------- exactly representable variances
def minvar_boundary(dt=np.uint8, W=8, n=2):
    """n = 2 stacks whose variances are exact: left samples {a, a + 2k} (mean a + k, diffs
    -k, +k, variance 2 k^2), right samples {b, b + 2m}. Returns (L, R, raw, var_l, var_r)
    with raw = 0 everywhere, var_* the per-column float64 variances (integers)."""
    top = 255 if np.dtype(dt) == np.uint8 else 65535
    x = np.arange(W)
    k = 1 + x % 5                  # 1..5
    m = 1 + (x // 2) % 4           # 1..4
    k = k * (1 if top == 255 else 1000)
    m = m * (1 if top == 255 else 1000)
    a = (7 * x) % 50
    b = top - 2 * m - (3 * x) % 40
    L = np.stack([a, a + 2 * k]).astype(dt).reshape(n, 1, W)
    R = np.stack([b, b + 2 * m]).astype(dt).reshape(n, 1, W)
    raw = np.zeros((1, W), np.int16)
    return L, R, raw, (2 * k * k).astype(np.float64), (2 * m * m).astype(np.float64)


# ------------------------------------------------------------------- symmetric neighbours
def symmetric_rows(n, dt=np.uint8, H=3, W=64, seed=5):
    """Right stack with R[:, :, c - 1] == R[:, :, c + 1] around every odd column c, and a raw
    map matching every pixel to an odd interior column: B = 0 there, so x and -x interpolate
    the same samples and the first (x <= 0) of two equal maxima must win."""
    L = random_stack(n, H, W, dt, seed=seed)
    R = random_stack(n, H, W, dt, seed=seed + 1)
    R[:, :, 2::2] = R[:, :, 0:1]           # every even column alike: neighbours of odd ones
    R[:, :, 0] = R[:, :, 2]
    cols = np.arange(W)
    col1 = 1 + 2 * ((cols * 7 + 3) % ((W - 2) // 2))   # odd, in [1, W - 3]
    raw = np.broadcast_to((cols - col1).astype(np.int16), (H, W)).copy()
    return L, R, raw


# -------------------------------------------------------------------------- mixed raw maps
def mixed_raw(H, W, seed, lo=-3, hi=12):
    """A raw disparity map no search would give: random disparities either side of zero,
    col1 = 0 and col1 = W - 1 columns, disparities pointing off both ends of the row, invalid
    pixels."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(lo, hi, size=(H, W)).astype(np.int16)
    if W > 3:
        raw[:, 3] = 3                      # col1 == 0
    raw[:, W - 1] = 0                      # col1 == W - 1
    raw[:, 0] = -(W - 1)                   # col1 == W - 1 from column 0
    if W > 6:
        raw[:, 5] = 9                      # col1 = -4: left of the row
        raw[:, W - 2] = -7                 # col1 = W + 5: right of the row
        raw[0, 1] = 32767
        raw[0, 2] = -32767
    raw[rng.random((H, W)) < 0.1] = INVALID
    return raw
