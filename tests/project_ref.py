"""The projection stage restated in numpy (include/bicos_c.h, "projection"): float64 for the
camera model, float32 where the definition says float32, one numpy operation per written
operation (numpy does not fuse). The GPU tests compare the kernels against `restate` bit for bit;
tests/test_project_api.py checks `restate` itself against a plain Python loop and hand-worked
cases.
"""
import numpy as np

from tests.normals_ref import NAN32, bits  # noqa: F401  (bits: re-exported for the tests)

VISIBLE, OCCLUDED, OUTSIDE, BEHIND, INVALID = range(5)
F64, F32 = np.float64, np.float32
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
OUTPUTS = ("uv", "depth", "cls", "tex", "depth_map", "index_map", "counts")


def camera(K, D=None, R=None, t=None):
    """-> dict of float64: R (9), t (3), fx fy cx cy, k1 .. k6, p1 p2 (missing coefficients 0)"""
    K = np.asarray(K, F64).reshape(3, 3)
    d = np.zeros(8, F64)
    if D is not None:
        D = np.asarray(D, F64).ravel()
        assert D.size in (0, 4, 5, 8)
        d[:D.size] = D
    return dict(R=(np.eye(3) if R is None else np.asarray(R, F64)).reshape(9),
                t=np.zeros(3) if t is None else np.asarray(t, F64).reshape(3),
                fx=K[0, 0], cx=K[0, 2], fy=K[1, 1], cy=K[1, 2],
                k1=d[0], k2=d[1], p1=d[2], p2=d[3], k3=d[4], k4=d[5], k5=d[6], k6=d[7])


def pinhole(c, points):
    """steps 1 to 4 -> dict(cls0 = VISIBLE (inside) | OUTSIDE | BEHIND | INVALID, uf, vf, zf, px,
    py); px, py only meaningful where inside"""
    p = np.asarray(points, F32).reshape(-1, 3)
    n = len(p)
    with np.errstate(all="ignore"):
        X, Y, Z = (p[:, k].astype(F64) for k in range(3))
        R, t = c["R"], c["t"]
        Xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0]
        Yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1]
        Zc = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2]
        x, y = Xc / Zc, Yc / Zc
        r2 = x * x + y * y
        kr = (1.0 + ((c["k3"] * r2 + c["k2"]) * r2 + c["k1"]) * r2) / \
             (1.0 + ((c["k6"] * r2 + c["k5"]) * r2 + c["k4"]) * r2)
        xd = (x * kr + c["p1"] * ((2.0 * x) * y)) + c["p2"] * (r2 + (2.0 * x) * x)
        yd = (y * kr + c["p1"] * (r2 + (2.0 * y) * y)) + c["p2"] * ((2.0 * x) * y)
        uf = (c["fx"] * xd + c["cx"]).astype(F32)
        vf = (c["fy"] * yd + c["cy"]).astype(F32)
        zf = Zc.astype(F32)
        pxf = np.floor(uf + F32(0.5))
        pyf = np.floor(vf + F32(0.5))
    assert pxf.dtype == F32 and uf.dtype == F32
    invalid = ~(np.isfinite(p).all(axis=1))
    behind = ~invalid & ~(Zc > 0)
    return dict(n=n, invalid=invalid, behind=behind, uf=uf, vf=vf, zf=zf, pxf=pxf, pyf=pyf)


def restate(points, cam, size, splat=0, tol=np.inf, image=None, fill=0):
    """-> dict of every output of the stage (tex only with an image [rows, cols] or
    [rows, cols, ch], uint8 or uint16)"""
    rows, cols = size
    pr = pinhole(cam, points)
    n, uf, vf, zf = pr["n"], pr["uf"], pr["vf"], pr["zf"]
    dead = pr["invalid"] | pr["behind"]
    with np.errstate(all="ignore"):
        inside = ~dead & np.isfinite(uf) & np.isfinite(vf) & (pr["pxf"] >= F32(0)) & \
            (pr["pxf"] < F32(cols)) & (pr["pyf"] >= F32(0)) & (pr["pyf"] < F32(rows))
    px = np.where(inside, pr["pxf"], 0).astype(np.int64)
    py = np.where(inside, pr["pyf"], 0).astype(np.int64)
    # the z-buffer: the smallest key per pixel
    key = (bits(zf).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    keys = np.full(rows * cols, EMPTY_KEY, np.uint64)
    idx = np.flatnonzero(inside)
    for dy in range(-splat, splat + 1):
        for dx in range(-splat, splat + 1):
            y, x = py[idx] + dy, px[idx] + dx
            ok = (y >= 0) & (y < rows) & (x >= 0) & (x < cols)
            np.minimum.at(keys, (y * cols + x)[ok], key[idx][ok])
    hi = (keys >> np.uint64(32)).astype(np.uint32)
    empty = keys == EMPTY_KEY
    depth_map = np.where(empty, NAN32, hi.view(F32)).astype(F32).reshape(rows, cols)
    index_map = np.where(empty, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)) \
        .astype(np.int32).reshape(rows, cols)
    zmin = np.zeros(n, F32)
    zmin[idx] = hi.view(F32)[py[idx] * cols + px[idx]]
    with np.errstate(all="ignore"):
        occluded = inside & ~(zf <= zmin + F32(tol))
    cls = np.full(n, OUTSIDE, np.uint8)
    cls[pr["invalid"]] = INVALID
    cls[pr["behind"]] = BEHIND
    cls[inside] = VISIBLE
    cls[occluded] = OCCLUDED
    uv = np.stack([np.where(dead, NAN32, uf), np.where(dead, NAN32, vf)], axis=1).astype(F32)
    out = dict(uv=uv, depth=np.where(dead, NAN32, zf).astype(F32), cls=cls, depth_map=depth_map,
               index_map=index_map,
               counts=np.bincount(cls, minlength=5).astype(np.uint32))
    if image is not None:
        out["tex"] = texture(image, uf, vf, cls == VISIBLE, fill)
    return out


def texture(image, uf, vf, visible, fill):
    """step 7 -> [n, channels] of the image's dtype"""
    img = np.asarray(image)
    img = img.reshape(img.shape[0], img.shape[1], -1)
    rows, cols, ch = img.shape
    top_level = F32(255.0 if img.dtype == np.uint8 else 65535.0)
    out = np.full((len(uf), ch), fill, img.dtype)
    v = np.flatnonzero(visible)
    if len(v) == 0:
        return out
    u, w = uf[v], vf[v]
    x0, y0 = np.floor(u), np.floor(w)
    fx, fy = u - x0, w - y0
    assert fx.dtype == F32
    xa = np.clip(x0.astype(np.int64), 0, cols - 1)
    xb = np.clip(x0.astype(np.int64) + 1, 0, cols - 1)
    ya = np.clip(y0.astype(np.int64), 0, rows - 1)
    yb = np.clip(y0.astype(np.int64) + 1, 0, rows - 1)
    for k in range(ch):
        p00, p01 = img[ya, xa, k].astype(F32), img[ya, xb, k].astype(F32)
        p10, p11 = img[yb, xa, k].astype(F32), img[yb, xb, k].astype(F32)
        top = p00 + fx * (p01 - p00)
        bot = p10 + fx * (p11 - p10)
        val = top + fy * (bot - top)
        assert val.dtype == F32
        out[v, k] = np.minimum(np.maximum(np.rint(val), F32(0)), top_level).astype(img.dtype)
    return out


# ------------------------------------------------------------------------ test data
def rotation(rx, ry, rz):
    """Rz * Ry * Rx from angles in radians, float64"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


DISTORTION = (-0.21, 0.07, 0.0011, -0.0007, -0.013, 0.004, -0.002, 0.0005)


def rig(rows, cols, nd=0, moved=True):
    """a camera for an image of rows x cols: focal length about the image width, optionally
    rotated a few degrees and shifted, with the first nd distortion coefficients -> (K, D, R, t)"""
    f = 1.1 * max(rows, cols, 8)
    K = np.array([[f, 0.3, (cols - 1) / 2.0 + 0.37], [0, f * 1.01, (rows - 1) / 2.0 - 0.21],
                  [0, 0, 1]], F64)
    D = np.array(DISTORTION[:nd], F64) if nd else None
    if not moved:
        return K, D, None, None
    return K, D, rotation(0.031, -0.052, 0.017), np.array([0.043, -0.021, 0.09], F64)


def cloud(count, rows, cols, K, seed=0, z=(1.0, 3.0), bad=0.08):
    """count float32 points scattered over a little more than the camera's view (so some fall
    outside), at two depth layers (so some are occluded), with some behind the camera, some not
    finite, and some exact duplicates of the depth of others"""
    rng = np.random.default_rng(seed + 1000 * count + rows)
    f = K[0, 0]
    u = rng.uniform(-0.15 * cols - 1, 1.15 * cols + 1, count)
    v = rng.uniform(-0.15 * rows - 1, 1.15 * rows + 1, count)
    Z = np.where(rng.random(count) < 0.5, z[0], z[1]) + rng.uniform(0, 0.2, count)
    Z = np.round(Z * 64) / 64  # few distinct depths: equal depths meet on a pixel
    p = np.stack([(u - K[0, 2]) / f * Z, (v - K[1, 2]) / K[1, 1] * Z, Z], axis=1).astype(F32)
    kind = rng.random(count)
    p[kind < bad * 0.4, 2] *= -1                      # behind
    p[(kind >= bad * 0.4) & (kind < bad * 0.5), 2] = 0  # Zc == 0 for an unmoved camera
    sel = np.flatnonzero((kind >= bad * 0.5) & (kind < bad))
    p[sel, rng.integers(0, 3, len(sel))] = rng.choice(
        np.array([np.nan, np.inf, -np.inf], F32), len(sel))
    return p


def picture(rows, cols, channels, dtype, seed=0):
    rng = np.random.default_rng(seed + 7 * rows + cols)
    top = 255 if dtype == np.uint8 else 65535
    img = rng.integers(0, top + 1, (rows, cols, channels)).astype(dtype)
    img.reshape(-1)[::11] = top  # saturated and empty levels among the taps
    img.reshape(-1)[5::13] = 0
    return img if channels > 1 else img[:, :, 0]
