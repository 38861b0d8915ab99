"""numpy restatement of include/bicos_c.h, "rectification": the maps of one camera from its
calibration (float64, the cofactor inverse written out) and the bilinear remap of a stack
(float32, one rounded operation at a time). The GPU tests compare bit for bit against these;
tests/test_rectify_api.py checks the restatement on its own terms."""
import numpy as np

F32 = np.float32


def inverse3(M):
    """inverse(M) by cofactors, each element its cofactor divided by the determinant, in plain
    Python floats (IEEE double, no contraction). Returns (iM as 9 floats row-major, det)."""
    (m00, m01, m02), (m10, m11, m12), (m20, m21, m22) = [[float(v) for v in r] for r in M]
    det = (m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20)) + \
        m02 * (m10 * m21 - m11 * m20)
    iM = [(m11 * m22 - m12 * m21) / det, (m02 * m21 - m01 * m22) / det, (m01 * m12 - m02 * m11) / det,
          (m12 * m20 - m10 * m22) / det, (m00 * m22 - m02 * m20) / det, (m02 * m10 - m00 * m12) / det,
          (m10 * m21 - m11 * m20) / det, (m01 * m20 - m00 * m21) / det, (m00 * m11 - m01 * m10) / det]
    return iM, det


def product3(P, R):
    """M = P[:, :3] * R, each element ((a0*b0 + a1*b1) + a2*b2)."""
    P = np.asarray(P, np.float64)
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    return [[(float(P[i, 0]) * float(R[0, j]) + float(P[i, 1]) * float(R[1, j])) +
             float(P[i, 2]) * float(R[2, j]) for j in range(3)] for i in range(3)]


def distort(iM, K, D, rows, cols):
    """The per-pixel part: float64 (map_x, map_y) before the final conversion to float32."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    d = np.zeros(8)
    dd = np.zeros(0) if D is None else np.asarray(D, np.float64).ravel()
    d[:dd.size] = dd
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in d)
    fx, cx, fy, cy = float(K[0, 0]), float(K[0, 2]), float(K[1, 1]), float(K[1, 2])
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64),
                       indexing="ij")
    with np.errstate(all="ignore"):
        X = (iM[0] * u + iM[1] * v) + iM[2]
        Y = (iM[3] * u + iM[4] * v) + iM[5]
        W = (iM[6] * u + iM[7] * v) + iM[8]
        x = X / W
        y = Y / W
        r2 = x * x + y * y
        kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = (x * kr + p1 * ((2.0 * x) * y)) + p2 * (r2 + (2.0 * x) * x)
        yd = (y * kr + p1 * (r2 + (2.0 * y) * y)) + p2 * ((2.0 * x) * y)
        return fx * xd + cx, fy * yd + cy


def maps(K, D, R, P, rows, cols):
    """(map_x, map_y) as float32 [rows, cols]."""
    iM, _ = inverse3(product3(P, R))
    mx, my = distort(iM, K, D, rows, cols)
    with np.errstate(all="ignore"):
        return mx.astype(F32), my.astype(F32)


def remap(stack, map_x, map_y, border=0):
    """stack [n, src_rows, src_cols] uint8 / uint16 -> (out [n, rows, cols], valid uint8)."""
    stack = np.asarray(stack)
    assert stack.ndim == 3 and stack.dtype in (np.uint8, np.uint16)
    _, sr, sc = stack.shape
    top_level = F32(255 if stack.dtype == np.uint8 else 65535)
    x = np.asarray(map_x, F32)
    y = np.asarray(map_y, F32)
    b = F32(border)
    with np.errstate(invalid="ignore"):
        inside = (x > F32(-1)) & (x < F32(sc)) & (y > F32(-1)) & (y < F32(sr))
    xs = np.where(inside, x, F32(0))
    ys = np.where(inside, y, F32(0))
    xf, yf = np.floor(xs), np.floor(ys)
    fx, fy = xs - xf, ys - yf
    assert fx.dtype == F32 and fy.dtype == F32
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    cx0, cx1 = (x0 >= 0) & (x0 < sc), x0 + 1 < sc
    ry0, ry1 = (y0 >= 0) & (y0 < sr), y0 + 1 < sr

    def tap(yi, xi, ok):
        v = stack[:, np.clip(yi, 0, sr - 1), np.clip(xi, 0, sc - 1)].astype(F32)
        return np.where(inside & ok, v, b)

    p00, p01 = tap(y0, x0, ry0 & cx0), tap(y0, x0 + 1, ry0 & cx1)
    p10, p11 = tap(y0 + 1, x0, ry1 & cx0), tap(y0 + 1, x0 + 1, ry1 & cx1)
    top = p00 + fx * (p01 - p00)
    bot = p10 + fx * (p11 - p10)
    v = top + fy * (bot - top)
    assert v.dtype == F32
    out = np.minimum(np.maximum(np.rint(v), F32(0)), top_level).astype(stack.dtype)
    valid = inside & cx0 & ry0 & ((fx == 0) | cx1) & ((fy == 0) | ry1)
    return out, valid.astype(np.uint8)


# ------------------------------------------------------------------ shared test material

def identity_maps(rows, cols):
    v, u = np.meshgrid(np.arange(rows, dtype=F32), np.arange(cols, dtype=F32), indexing="ij")
    return u, v


def camera(rows, cols, degrees=2.0, k1=-0.08):
    """A plausible calibration for a rows x cols sensor: (K, D, R, P) with a rotation of
    `degrees` about the optical axis tilted a little, and radial + tangential distortion."""
    f = 0.9 * cols
    K = np.array([[f, 0.3, cols / 2 - 0.7], [0, 1.01 * f, rows / 2 + 0.4], [0, 0, 1]])
    D = np.array([k1, 0.02, 1e-3, -7e-4, 0.004, 0.01, -0.003, 0.002])
    a, t = np.deg2rad(degrees), np.deg2rad(0.5)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])
    R = Rz @ Ry
    P = np.array([[f, 0, cols / 2, -40.0], [0, f, rows / 2, 0], [0, 0, 1, 0]])
    return K, D, R, P


def images(n, rows, cols, dtype, seed=0):
    """Full-range random planes; plane 0 holds the extremes in its corners."""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max
    s = rng.integers(0, top + 1, size=(n, rows, cols), dtype=np.int64).astype(dtype)
    s[0, 0, 0], s[0, -1, -1] = 0, top
    return s
