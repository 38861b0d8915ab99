"""Two independent numpy restatements of the median filter's definition (include/bicos_c.h,
"median filter") and the input patterns of its tests.

  restate()          the definition read literally: per pixel, the valid values of the clipped
                     window, sorted by the key, the element of rank (m - 1) // 2. The per-pixel
                     part (windows()) does not depend on fill_min, so the tests compute it once
                     per map and aperture and finish() it for every fill_min.
  restate_shifted()  vectorised over the ksize * ksize shifted copies of the map: invalid and
                     outside slots sort behind every valid key, and the rank is looked up per
                     pixel from its own m. It does not use the kernel's padding identity.

Neither knows anything of the GPU code. tests/test_median_api.py checks them against each
other and against answers derived by hand.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden.npz")
INV16 = -32768
SENTINEL_BITS = 0xC7000000  # -32768.0f


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


def valid_mask(d, sentinel=False):
    if d.dtype == np.int16:
        return d != INV16
    assert d.dtype == np.float32
    v = ~np.isnan(d)
    if sentinel:
        v &= bits(d) != SENTINEL_BITS
    return v


def order_key(d):
    """the integer the definition orders by (int64; only meaningful where the pixel is valid)"""
    if d.dtype == np.int16:
        return d.astype(np.int64)
    b = bits(d).astype(np.int64)
    return np.where(b >> 31 != 0, b ^ 0xFFFFFFFF, b ^ 0x80000000)


# ------------------------------------------------------------------ restatement (a)
def windows(d, ksize, sentinel=False):
    """per pixel: m = the number of valid values in its clipped window, med = their lower
    median (the map's dtype, bits copied; the pixel's own bits where m == 0)"""
    rows, cols = d.shape
    h = ksize // 2
    valid = valid_mask(d, sentinel)
    key = order_key(d)
    med = d.copy()
    m = np.zeros((rows, cols), np.int32)
    for r in range(rows):
        r0, r1 = max(r - h, 0), min(r + h + 1, rows)
        for c in range(cols):
            c0, c1 = max(c - h, 0), min(c + h + 1, cols)
            sel = valid[r0:r1, c0:c1]
            vals = d[r0:r1, c0:c1][sel]
            n = vals.size
            m[r, c] = n
            if n:
                order = np.argsort(key[r0:r1, c0:c1][sel], kind="stable")
                med[r, c] = vals[order[(n - 1) // 2]]
    return dict(med=med, m=m, valid=valid)


def finish(d, win, fill_min):
    """the output rule on windows(): dict(out, counts = [unchanged, changed, filled, invalid])"""
    valid, m, med = win["valid"], win["m"], win["med"]
    fill = ~valid & (m >= fill_min) if fill_min > 0 else np.zeros_like(valid)
    take = valid | fill
    out = np.where(take, med, d)
    # (np.where keeps the bits of both branches; checked here because everything rests on it)
    assert np.array_equal(bits(out)[~take], bits(d)[~take])
    same = bits(out) == bits(d)
    counts = np.array([(valid & same).sum(), (valid & ~same).sum(), fill.sum(),
                       (~valid & ~fill).sum()], np.uint32)
    assert counts.sum() == d.size
    return dict(out=out, counts=counts)


def restate(d, ksize, fill_min, sentinel=False):
    return finish(d, windows(d, ksize, sentinel), fill_min)


# ------------------------------------------------------------------ restatement (b)
def restate_shifted(d, ksize, fill_min, sentinel=False):
    rows, cols = d.shape
    h = ksize // 2
    valid = valid_mask(d, sentinel)
    big = np.int64(1) << 40  # behind every key
    key = np.where(valid, order_key(d), big)
    padded = np.full((rows + 2 * h, cols + 2 * h), big, np.int64)
    padded[h:h + rows, h:h + cols] = key
    stack = np.stack([padded[dy:dy + rows, dx:dx + cols]
                      for dy in range(ksize) for dx in range(ksize)])
    m = (stack != big).sum(axis=0)
    stack = np.sort(stack, axis=0)
    rank = np.maximum(m - 1, 0) // 2
    k = np.take_along_axis(stack, rank[None], axis=0)[0]
    if d.dtype == np.int16:
        med = np.where(m > 0, k, 0).astype(np.int16)
    else:
        k = np.where(m > 0, k, 0)
        b = np.where(k >> 31 != 0, k ^ 0x80000000, k ^ 0xFFFFFFFF)
        med = b.astype(np.uint32).view(np.float32)
    fill = ~valid & (m >= fill_min) & (fill_min > 0)
    out = d.copy()
    out[valid | fill] = med[valid | fill]
    same = bits(out) == bits(d)
    counts = np.array([(valid & same).sum(), (valid & ~same).sum(), fill.sum(),
                       (~valid & ~fill).sum()], np.uint32)
    return dict(out=out, counts=counts)


# ------------------------------------------------------------------------ patterns
def fill_mins(ksize):
    return (0, 1, ksize * ksize // 2 + 1, ksize * ksize)


def golden_maps():
    """the committed disparity maps of tests/golden/golden.npz (name, map)"""
    z = np.load(GOLDEN)
    return [(k.replace("/", "."), z[k]) for k in z.files if k.endswith("/disparity")]


NAN_PAYLOADS = np.array([0x7FC00000, 0x7FC00001, 0xFFC01234, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF],
                        np.uint32).view(np.float32)


def plane(rows, cols, dtype):
    r, c = np.mgrid[0:rows, 0:cols]
    p = 20 + 0.5 * r + 0.25 * c
    return p.astype(dtype) if dtype == np.float32 else np.floor(p * 16).astype(np.int16)


def patterns(rows, cols, dtype, seed=0):
    """-> list of (name, map, sentinel). dtype: np.int16 or np.float32."""
    rng = np.random.default_rng(1000 * rows + cols + seed)
    f32 = dtype == np.float32
    out = []

    def add(name, d, sentinel=False):
        assert d.dtype == dtype and d.shape == (rows, cols)
        out.append((name, d, sentinel))

    def invalidate(d, mask, sentinel):
        """float: NaNs of several payloads, and with `sentinel` -32768.0 among them"""
        if not f32:
            d[mask] = INV16
            return d
        n = int(mask.sum())
        inv = rng.choice(NAN_PAYLOADS, n)
        if sentinel:
            inv = np.where(rng.random(n) < 0.5, np.float32(-32768.0), inv)
        b = bits(d).copy()  # (through bits: assigning float NaNs could quieten a payload)
        b[mask] = bits(inv)
        return b.view(np.float32)

    def random_values(wide):
        if f32:
            v = rng.normal(0, 100 if wide else 2, (rows, cols)).astype(np.float32)
            return v if wide else np.round(v * 2) / np.float32(2)  # ties
        return rng.integers(-32767 if wide else -6, 32768 if wide else 7, (rows, cols)).astype(np.int16)

    for wide in (False, True):
        for sentinel in ((False, True) if f32 else (False,)):
            d = invalidate(random_values(wide), rng.random((rows, cols)) < 0.3, sentinel)
            add("random30-%s-sentinel%d" % ("wide" if wide else "ties", sentinel), d, sentinel)
    add("all-valid", random_values(True))
    add("all-invalid", invalidate(random_values(True), np.ones((rows, cols), bool), f32), f32)
    r, c = np.mgrid[0:rows, 0:cols]
    add("checkerboard", invalidate(random_values(False), (r + c) % 2 == 0, False))
    add("constant", np.full((rows, cols), 7, dtype))
    d = plane(rows, cols, dtype)
    spikes = rng.random((rows, cols)) < 0.04
    d[spikes] += dtype(1000)
    d[rng.random((rows, cols)) < 0.02] -= dtype(1000)
    add("outliers", d)
    holes = rng.random((rows, cols)) < 0.03
    seeds = rng.random((rows, cols)) < 0.01
    for dy in (0, 1):
        for dx in (0, 1):
            holes[dy:, dx:] |= seeds[:rows - dy, :cols - dx]
    add("holes", invalidate(plane(rows, cols, dtype), holes, f32), f32)
    if f32:
        special = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, -32768.0, 1.5, -1.5, 1e-45,
                                            -1e-45, 3.4e38, -32767.996, -32768.004], np.float32),
                                  NAN_PAYLOADS])
        d = rng.choice(special, (rows, cols))
        add("special-sentinel0", d, False)
        add("special-sentinel1", d, True)
        z = np.where(rng.random((rows, cols)) < 0.5, np.float32(0.0), np.float32(-0.0))
        add("signed-zeros", invalidate(z.astype(np.float32), rng.random((rows, cols)) < 0.2, False))
    else:
        d = rng.choice(np.array([-32767, 32767, 0, -1, 1, INV16], np.int16), (rows, cols))
        add("extremes", d)
    return out
