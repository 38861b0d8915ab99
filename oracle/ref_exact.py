"""TEST INFRASTRUCTURE ONLY -- exact-arithmetic statement of Precision::DOUBLE (reference
include/impl/cuda/agree.cuh:35-65 nxcorrd, :110-259 the two agree kernels with TPrecision =
double), used to hold the float64 functions of bicos_oracle.c to the bit
(tests/test_oracle_f64.py).

Every IEEE operation of the double path is computed here as an exact rational
(fractions.Fraction: the operands are doubles, hence rationals) and rounded ONCE by
float(Fraction), which is correctly rounded to nearest-even; the square root is rounded
through an integer square root with a sticky bit. No C library and no float64 arithmetic
decides a bit: floats are only converted, compared and negated. The float32 quadratic, the
x steps and the narrowing are ref_numpy's (they are the float path's, already pinned to the
reference's CPU code).

The magnitudes stay far from overflow, underflow and subnormals (samples <= 65535, n <= 256:
variances < 2^41, their product < 2^82, no nonzero diff below 2^-9), so "rounded once to 53
bits" is all of IEEE that matters; a zero result is +0 as in round-to-nearest (the chains
start at +0, so no -0 can appear).

Plain Python loops per pixel -- call it on a sample of pixels, not on images.
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

from . import ref_numpy as N

INVALID16 = -32768


def rn(q: Fraction) -> float:
    """The double nearest to the rational q (ties to even)."""
    return float(q)


def fma(a: float, b: float, c: float) -> float:
    return rn(Fraction(a) * Fraction(b) + Fraction(c))


def sub(a: float, b: float) -> float:
    return rn(Fraction(a) - Fraction(b))


def mul(a: float, b: float) -> float:
    return rn(Fraction(a) * Fraction(b))


def div(a: float, b: float) -> float:
    """a / b for finite a and b; x / 0 as IEEE has it (0 / 0 = NaN)."""
    if b == 0.0:
        if a == 0.0:
            return math.nan
        return math.inf if a > 0 else -math.inf
    return rn(Fraction(a) / Fraction(b))


def sqrt(x: float) -> float:
    """Correctly rounded sqrt of a finite x >= 0: with x = N / 4^e for an integer N >= 2^128
    (e chosen so), r = isqrt(N) has >= 64 bits and sqrt(x) lies in [r, r + 1) / 2^e, strictly
    above r exactly when r r != N. (2 r + sticky) / 2^(e + 1) is then on the same side of
    every 53-bit rounding boundary as sqrt(x), and one rounding of it is the answer."""
    if x == 0.0:
        return 0.0
    q = Fraction(x)
    k = q.denominator.bit_length() - 1  # the denominator of a double is 2^k
    e = (k + 1) // 2
    big = q.numerator << (2 * e - k)
    while big < (1 << 128):
        big <<= 2
        e += 1
    r = math.isqrt(big)
    sticky = int(r * r != big)
    return rn(Fraction(2 * r + sticky, 1 << (e + 1)))


def nxcorr(pix0: Sequence[int], pix1: Sequence[int], minvar: Optional[float] = None) -> float:
    """agree.cuh:35-65. minvar: the scaled float32 value (widened exactly), or None."""
    n = len(pix0)
    p0 = [int(v) for v in pix0]
    p1 = [int(v) for v in pix1]
    m0 = rn(Fraction(sum(p0), n))  # the sums are integers: exact in double
    m1 = rn(Fraction(sum(p1), n))
    cov = v0 = v1 = 0.0
    for a, b in zip(p0, p1):
        d0 = rn(Fraction(a) - Fraction(m0))
        d1 = rn(Fraction(b) - Fraction(m1))
        cov = fma(d0, d1, cov)
        v0 = fma(d0, d0, v0)
        v1 = fma(d1, d1, v1)
    if minvar is not None:
        mv = float(np.float32(minvar))  # a conversion: exact
        if v0 < mv or v1 < mv:
            return -1.0
    return div(cov, sqrt(mul(v0, v1)))


def _pixels(disp: np.ndarray, pixels: Optional[Iterable[Tuple[int, int]]]):
    if pixels is None:
        H, W = disp.shape
        return [(r, c) for r in range(H) for c in range(W)]
    return [(int(r), int(c)) for r, c in pixels]


def agree(disp: np.ndarray, s0: np.ndarray, s1: np.ndarray, thr: float,
          minvar: Optional[float], pixels=None):
    """agree.cuh:110-159 at `pixels` (an iterable of (row, col); None: every pixel). Returns
    (disparity int16, corrmap float64) of the whole shape; pixels not asked for keep their
    input disparity and a NaN correlation."""
    n, H, W = s0.shape
    d = np.array(disp, np.int16, copy=True)
    corr = np.full((H, W), np.nan, np.float64)
    t = float(np.float32(thr))
    for r, c in _pixels(disp, pixels):
        dv = int(d[r, c])
        if dv == INVALID16:
            continue
        c1 = c - dv
        if c1 < 0 or c1 >= W:
            d[r, c] = INVALID16
            continue
        v = nxcorr(s0[:, r, c], s1[:, r, c1], minvar)
        corr[r, c] = v
        if v < t:  # false for NaN
            d[r, c] = INVALID16
    return d, corr


def agree_subpixel(disp: np.ndarray, s0: np.ndarray, s1: np.ndarray, thr: float, step: float,
                   minvar: Optional[float], pixels=None, want_best_x: bool = False):
    """agree.cuh:161-259 at `pixels`. Returns (disparity float32, corrmap float64), NaN where
    invalid or not asked for; with want_best_x also the float32 best_x map (NaN where none)."""
    n, H, W = s0.shape
    out = np.full((H, W), np.nan, np.float32)
    corr = np.full((H, W), np.nan, np.float64)
    bx = np.full((H, W), np.nan, np.float32)
    t = float(np.float32(thr))
    xs = N.x_steps(step)
    for r, c in _pixels(disp, pixels):
        dv = int(disp[r, c])
        if dv == INVALID16:
            continue
        c1 = c - dv
        if c1 < 0 or c1 >= W:
            continue
        left = s0[:, r, c]
        if c1 == 0 or c1 == W - 1:
            v = nxcorr(left, s1[:, r, c1], minvar)
            corr[r, c] = v
            if not v < t:
                out[r, c] = np.float32(dv)
            continue
        A, B, C = N.quadratic(s1[:, r, c1 - 1], s1[:, r, c1], s1[:, r, c1 + 1])
        best_x = np.float32(0.0)
        best = -1.0
        for x in xs:
            v = nxcorr(left, N.interpolate(A, B, C, x, s0.dtype), minvar)
            if best < v:
                best_x, best = x, v
        corr[r, c] = best
        bx[r, c] = best_x
        if not best < t:
            out[r, c] = np.float32(np.float32(dv) - best_x)
    return (out, corr, bx) if want_best_x else (out, corr)
