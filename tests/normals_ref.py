"""Two numpy float64 restatements of the surface-normal definition (include/bicos_c.h, "surface
normals") and the input patterns of its tests.

  restate()        (a) vectorised over the pixels, with a Python loop over the window taps in
                   row-major order, so the order of every pixel's sums is exactly the text's. A
                   tap that is no member is SKIPPED (np.where keeps the old sum), as the text
                   says. The tap loop (windows()) depends on radius, max_diff and the sentinel
                   flag alone, so the tests run it once for those and finish() it for every Q,
                   flag and min_points.
  restate_loops()  (b) plain loops over the pixels and their windows on numpy scalars.

Neither knows anything of the GPU code. tests/test_normals_api.py checks them against each other
and against answers derived by hand.
"""
import numpy as np

ALLOW_NEGATIVE_Z, F32_SENTINEL = 1, 2
NORMAL, NO_POINT, SPARSE, DEGENERATE = 0, 1, 2, 3
INV16 = -32768
NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
F64, F32 = np.float64, np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def valid_mask(d, flags=0):
    if d.dtype == np.int16:
        return d != INV16
    assert d.dtype == np.float32
    v = ~np.isnan(d)
    if flags & F32_SENTINEL:
        v &= d != F32(-32768.0)
    return v


def reproj(q, x, y, d):
    """the text's reproj on float64 arrays or scalars -> three float64"""
    o = [((q[4 * i] * x + q[4 * i + 1] * y) + q[4 * i + 2] * d) + q[4 * i + 3] for i in range(4)]
    iw = 1.0 / o[3]
    return o[0] * iw, o[1] * iw, o[2] * iw


# ------------------------------------------------------------------ restatement (a)
def windows(d, radius, max_diff, flags=0):
    """steps 2 and 3 for every pixel (whatever its class): the integer and the double sums"""
    rows, cols = d.shape
    R = radius
    valid = valid_mask(d, flags)
    fp = np.where(valid, d.astype(F32), NAN32)
    dp = d.astype(F64)
    pad32 = np.full((rows + 2 * R, cols + 2 * R), NAN32, F32)
    pad32[R:R + rows, R:R + cols] = fp
    pad64 = np.zeros((rows + 2 * R, cols + 2 * R), F64)
    pad64[R:R + rows, R:R + cols] = dp
    zi = lambda: np.zeros((rows, cols), np.int64)  # noqa: E731
    m, Su, Sv, Suu, Suv, Svv = zi(), zi(), zi(), zi(), zi(), zi()
    Sd, Sud, Svd = (np.zeros((rows, cols), F64) for _ in range(3))
    md = F32(max_diff)
    with np.errstate(all="ignore"):
        for dv in range(-R, R + 1):
            for du in range(-R, R + 1):
                fq = pad32[R + dv:R + dv + rows, R + du:R + du + cols]
                dq = pad64[R + dv:R + dv + rows, R + du:R + du + cols]
                member = np.abs(fq - fp) <= md  # float32; False for NaN
                k = member.astype(np.int64)
                m += k
                Su += k * du
                Sv += k * dv
                Suu += k * du * du
                Suv += k * du * dv
                Svv += k * dv * dv
                e = dq - dp
                Sd = np.where(member, Sd + e, Sd)
                Sud = np.where(member, Sud + F64(du) * e, Sud)
                Svd = np.where(member, Svd + F64(dv) * e, Svd)
    return dict(valid=valid, m=m, Su=Su, Sv=Sv, Suu=Suu, Suv=Suv, Svv=Svv, Sd=Sd, Sud=Sud, Svd=Svd)


def finish(d, win, q, flags, min_points):
    """steps 1 and 4 to 9 on windows(): dict(map float32 [rows, cols, 3], cls, counts uint32[4])"""
    rows, cols = d.shape
    q = np.asarray(q, F64).reshape(16)
    y, x = np.meshgrid(np.arange(rows, dtype=F64), np.arange(cols, dtype=F64), indexing="ij")
    dp = d.astype(F64)
    m, Su, Sv, Suu, Suv, Svv = (win[k] for k in ("m", "Su", "Sv", "Suu", "Suv", "Svv"))
    Sd, Sud, Svd = win["Sd"], win["Sud"], win["Svd"]
    with np.errstate(all="ignore"):
        own = np.stack([c.astype(F32) for c in reproj(q, x, y, dp)], axis=-1)
        kept = win["valid"] & np.isfinite(own).all(axis=-1)
        if not flags & ALLOW_NEGATIVE_Z:
            kept &= ~(own[..., 2] < 0)
        C00 = Svv * m - Sv * Sv
        C01 = Su * Sv - Suv * m
        C02 = Suv * Sv - Svv * Su
        C11 = Suu * m - Su * Su
        C12 = Suv * Su - Suu * Sv
        C22 = Suu * Svv - Suv * Suv
        det = Suu * C00 + Suv * C01 + Su * C02
        for v in (C00, C01, C02, C11, C12, C22, det):
            assert np.abs(v).max(initial=0) < 2 ** 31
        c00, c01, c02, c11, c12, c22, dt = (v.astype(F64) for v in (C00, C01, C02, C11, C12, C22, det))
        a = ((c00 * Sud + c01 * Svd) + c02 * Sd) / dt
        b = ((c01 * Sud + c11 * Svd) + c12 * Sd) / dt
        c = ((c02 * Sud + c12 * Svd) + c22 * Sd) / dt
        d0 = dp + c
        P0 = reproj(q, x, y, d0)
        P1 = reproj(q, x + 1.0, y, d0 + a)
        P2 = reproj(q, x, y + 1.0, d0 + b)
        Ux, Uy, Uz = (P1[i] - P0[i] for i in range(3))
        Vx, Vy, Vz = (P2[i] - P0[i] for i in range(3))
        Nx, Ny, Nz = Uy * Vz - Uz * Vy, Uz * Vx - Ux * Vz, Ux * Vy - Uy * Vx
        away = (Nx * P0[0] + Ny * P0[1]) + Nz * P0[2] > 0
        Nx, Ny, Nz = (np.where(away, -v, v) for v in (Nx, Ny, Nz))
        L = np.sqrt((Nx * Nx + Ny * Ny) + Nz * Nz)
        unit = np.stack([(Nx / L).astype(F32), (Ny / L).astype(F32), (Nz / L).astype(F32)], axis=-1)
    cls = np.full((rows, cols), NORMAL, np.int32)
    cls[(L == 0) | ~np.isfinite(L)] = DEGENERATE
    cls[det == 0] = DEGENERATE
    cls[m < min_points] = SPARSE
    cls[~kept] = NO_POINT
    out = np.where((cls == NORMAL)[..., None], unit, NAN32).astype(F32)
    counts = np.array([(cls == k).sum() for k in range(4)], np.uint32)
    assert int(counts.astype(np.int64).sum()) == rows * cols
    return dict(map=out, cls=cls, counts=counts)


def restate(d, q, flags=0, radius=2, max_diff=1.0, min_points=3):
    return finish(d, windows(d, radius, max_diff, flags), q, flags, min_points)


def gather(want_map, index):
    """the list form of a map: its rows at `index`, three NaNs for an index outside it"""
    flat = want_map.reshape(-1, 3)
    index = np.asarray(index, np.int64)
    inside = (index >= 0) & (index < flat.shape[0])
    out = np.full((index.size, 3), NAN32, F32)
    out[inside] = flat[index[inside]]
    return out


# ------------------------------------------------------------------ restatement (b)
def restate_loops(d, q, flags=0, radius=2, max_diff=1.0, min_points=3):
    rows, cols = d.shape
    q = [F64(v) for v in np.asarray(q, F64).reshape(16)]
    out = np.full((rows, cols, 3), NAN32, F32)
    cls = np.zeros((rows, cols), np.int32)
    md = F32(max_diff)

    def invalid(v):
        if d.dtype == np.int16:
            return v == INV16
        return bool(np.isnan(v)) or bool(flags & F32_SENTINEL and v == F32(-32768.0))

    def pixel(y, x):
        dpv = d[y, x]
        if invalid(dpv):
            return NO_POINT, None
        dp = F64(dpv)
        X, Y, Z = (F32(v) for v in reproj(q, F64(x), F64(y), dp))
        if not (np.isfinite(X) and np.isfinite(Y) and np.isfinite(Z)):
            return NO_POINT, None
        if not flags & ALLOW_NEGATIVE_Z and Z < 0:
            return NO_POINT, None
        m = Su = Sv = Suu = Suv = Svv = 0
        Sd = Sud = Svd = F64(0.0)
        for r in range(max(y - radius, 0), min(y + radius, rows - 1) + 1):
            for c in range(max(x - radius, 0), min(x + radius, cols - 1) + 1):
                dqv = d[r, c]
                if invalid(dqv) or not np.abs(F32(dqv) - F32(dpv)) <= md:
                    continue
                du, dv = c - x, r - y
                e = F64(dqv) - dp
                m += 1
                Su += du
                Sv += dv
                Suu += du * du
                Suv += du * dv
                Svv += dv * dv
                Sd = Sd + e
                Sud = Sud + F64(du) * e
                Svd = Svd + F64(dv) * e
        if m < min_points:
            return SPARSE, None
        C00 = Svv * m - Sv * Sv
        C01 = Su * Sv - Suv * m
        C02 = Suv * Sv - Svv * Su
        C11 = Suu * m - Su * Su
        C12 = Suv * Su - Suu * Sv
        C22 = Suu * Svv - Suv * Suv
        det = Suu * C00 + Suv * C01 + Su * C02
        if det == 0:
            return DEGENERATE, None
        c00, c01, c02, c11, c12, c22, dt = (F64(v) for v in (C00, C01, C02, C11, C12, C22, det))
        a = ((c00 * Sud + c01 * Svd) + c02 * Sd) / dt
        b = ((c01 * Sud + c11 * Svd) + c12 * Sd) / dt
        c = ((c02 * Sud + c12 * Svd) + c22 * Sd) / dt
        d0 = dp + c
        P0 = reproj(q, F64(x), F64(y), d0)
        P1 = reproj(q, F64(x) + 1.0, F64(y), d0 + a)
        P2 = reproj(q, F64(x), F64(y) + 1.0, d0 + b)
        Ux, Uy, Uz = (P1[i] - P0[i] for i in range(3))
        Vx, Vy, Vz = (P2[i] - P0[i] for i in range(3))
        N = [Uy * Vz - Uz * Vy, Uz * Vx - Ux * Vz, Ux * Vy - Uy * Vx]
        if (N[0] * P0[0] + N[1] * P0[1]) + N[2] * P0[2] > 0:
            N = [-v for v in N]
        L = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
        if L == 0 or not np.isfinite(L):
            return DEGENERATE, None
        return NORMAL, [F32(v / L) for v in N]

    with np.errstate(all="ignore"):
        for y in range(rows):
            for x in range(cols):
                cls[y, x], n = pixel(y, x)
                if n is not None:
                    out[y, x] = n
    counts = np.array([(cls == k).sum() for k in range(4)], np.uint32)
    return dict(map=out, cls=cls, counts=counts)


# ------------------------------------------------------------------------ patterns
def rig_q(rows, cols, f=2000.0, baseline=0.1):
    """a cv::stereoRectify-shaped Q (cx1 == cx2): X = x - cx, Y = y - cy, Z = f, W = d / baseline"""
    return np.array([[1, 0, 0, -(cols - 1) / 2.0], [0, 1, 0, -(rows - 1) / 2.0],
                     [0, 0, 0, f], [0, 0, 1.0 / baseline, 0]], F64)


def odd_q(rows, cols):
    """W = 0.5 * d - 8: zero at d = 16 (not finite), negative below it (Z < 0)"""
    q = rig_q(rows, cols, 500.0)
    q[3] = [0, 0, 0.5, -8.0]
    return q


TILT = (40.3, 0.137, -0.071)  # d = 40.3 + 0.137 * col - 0.071 * row


def patterns(rows, cols, dtype, seed=0):
    """-> list of (name, map, Q). dtype: np.int16 or np.float32."""
    rng = np.random.default_rng(1000 * rows + cols + seed)
    f32 = dtype == np.float32
    r, c = np.mgrid[0:rows, 0:cols]
    q = rig_q(rows, cols)
    out = []

    def add(name, d, qq=q):
        d = np.ascontiguousarray(d)
        assert d.dtype == dtype and d.shape == (rows, cols)
        out.append((name, d, qq))

    def invalidate(d, mask):
        d = d.copy()
        if not f32:
            d[mask] = INV16
            return d
        n = int(mask.sum())
        inv = np.where(rng.random(n) < 0.5, F32(-32768.0), NAN32)
        d[mask] = inv
        return d

    # an exact plane with dyadic coefficients: every sum and the fit are exact
    if f32:
        add("exact", (16 + 0.25 * c - 0.5 * r).astype(F32))
    else:
        add("exact", (40 + 2 * c - 3 * r).astype(np.int16))
    tilted = TILT[0] + TILT[1] * c + TILT[2] * r
    if f32:
        add("tilted", tilted.astype(F32))
    add("rounded", np.rint(tilted).astype(dtype))
    rnd = rng.normal(30, 1.5, (rows, cols))
    rnd = rnd.astype(F32) if f32 else np.rint(rnd).astype(np.int16)
    add("random-holes", invalidate(rnd, rng.random((rows, cols)) < 0.3))
    if f32:
        special = np.array([np.nan, -32768.0, np.inf, -np.inf, 30.0, 30.5, 31.0, 29.75], F32)
        add("special", rng.choice(special, (rows, cols), p=[.08, .08, .05, .05, .2, .2, .17, .17]))
    else:
        add("special", rng.choice(np.array([INV16, -32767, 32767, 30, 31, 29], np.int16),
                                  (rows, cols), p=[.15, .05, .05, .3, .25, .2]))
    step = 20 + 0.125 * r + np.where(c >= cols // 2, 5.0, 0.0) + np.where(r >= rows // 2 + 1, 3.0, 0.0)
    add("step", step.astype(F32) if f32 else np.floor(step).astype(np.int16))
    add("all-invalid", invalidate(np.zeros((rows, cols), dtype), np.ones((rows, cols), bool)))
    near = 16 + rng.integers(-3, 4, (rows, cols)) * (0.5 if f32 else 1)
    add("odd-q", near.astype(dtype), odd_q(rows, cols))
    return out
