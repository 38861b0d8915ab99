"""The mesh definition of include/bicos_c.h ("mesh") restated in vectorised numpy, on top of the
reprojection's restatement (tests/test_reproject_api.restate) for the vertices, and the test map
the mesh tests share. tests/test_mesh_api.py checks this restatement against a plain double loop
over the quads and against hand-worked maps; the GPU tests compare the kernels with it exactly.
"""
import functools

import numpy as np

from tests.test_cli import Q
from tests.test_reproject_api import restate as restate_points

ALLOW_NEGATIVE_Z, F32_SENTINEL = 1, 2
KEYS = ("kept", "invalid", "nonfinite", "negative_z", "triangles", "quads_full", "quads_half",
        "quads_empty")


def restate(d, q, flags=0, max_diff=1.0):
    """-> dict(points [kept, 3], index [kept], counts uint32[4], kept mask: the reprojection's;
    vertex_map int32 [rows, cols]; triangles int32 [T, 3]; mesh_counts uint32[4];
    cases: how many quads fall under each row of the definition's table)"""
    d = np.asarray(d)
    v = restate_points(d, q, flags)
    rows, cols = d.shape
    kept = v["kept"]
    vmap = np.full((rows, cols), -1, np.int32)
    vmap[kept] = np.arange(int(kept.sum()), dtype=np.int32)
    out = dict(points=v["points"], index=v["index"], counts=v["counts"], kept=kept,
               vertex_map=vmap)
    if rows < 2 or cols < 2:
        out.update(triangles=np.zeros((0, 3), np.int32), mesh_counts=np.zeros(4, np.uint32),
                   cases=dict(ad=0, bc=0, missing=[0, 0, 0, 0]))
        return out
    f = d.astype(np.float32)
    md = np.float32(max_diff)
    corner = lambda a: (a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:])  # noqa: E731
    kA, kB, kC, kD = corner(kept)
    fA, fB, fC, fD = corner(f)
    rA, rB, rC, rD = corner(vmap)
    with np.errstate(all="ignore"):  # (values of pixels that are not kept are never used)
        step = lambda x, y: np.abs(x - y)  # noqa: E731  one float32 subtraction
        ad, bc = step(fA, fD), step(fB, fC)
        lAB = kA & kB & (step(fA, fB) <= md)
        lAC = kA & kC & (step(fA, fC) <= md)
        lBD = kB & kD & (step(fB, fD) <= md)
        lCD = kC & kD & (step(fC, fD) <= md)
        lAD = kA & kD & (ad <= md)
        lBC = kB & kC & (bc <= md)
        n = kA.astype(int) + kB + kC + kD
        four = n == 4
        diag_ad = four & (ad <= bc)
        diag_bc = four & ~(ad <= bc)
    three = n == 3
    # the four triangles a quad can hold, each with all of its three edges linked
    acd = (np.stack([rA, rC, rD], -1), lAC & lCD & lAD)
    adb = (np.stack([rA, rD, rB], -1), lAD & lBD & lAB)
    acb = (np.stack([rA, rC, rB], -1), lAC & lBC & lAB)
    bcd = (np.stack([rB, rC, rD], -1), lBC & lCD & lBD)
    # the table: (condition, T0, T1)
    table = [(diag_ad, acd, adb), (diag_bc, acb, bcd), (three & ~kD, acb, None),
             (three & ~kA, bcd, None), (three & ~kB, acd, None), (three & ~kC, adb, None)]
    shape = kA.shape
    t = np.zeros(shape + (2, 3), np.int32)
    e = np.zeros(shape + (2,), bool)
    for cond, t0, t1 in table:
        for slot, tri in ((0, t0), (1, t1)):
            if tri is None:
                continue
            on = cond & tri[1]
            t[on, slot] = tri[0][on]
            e[on, slot] = True
    per_quad = e.sum(-1)
    triangles = np.ascontiguousarray(t.reshape(-1, 3)[e.reshape(-1)])  # quads row-major, T0 then T1
    q2, q1, q0 = (int((per_quad == k).sum()) for k in (2, 1, 0))
    assert q2 + q1 + q0 == (rows - 1) * (cols - 1) and len(triangles) == 2 * q2 + q1
    out.update(triangles=triangles, mesh_counts=np.array([len(triangles), q2, q1, q0], np.uint32),
               cases=dict(ad=int(diag_ad.sum()), bc=int(diag_bc.sum()),
                          missing=[int((three & ~k).sum()) for k in (kA, kB, kC, kD)]))
    return out


def surface(rows, cols, dtype, seed, invalid=0.05):
    """The test map: a ramp on the left half, a plateau 12 above its end on the right (a step
    no max_diff of the tests links), a gentle slope down the rows, a column every 97 that drops
    by 30, and +-0.5 of noise in sixteenths, so that both diagonals, broken links and every
    missing-corner case occur. int16: floor, `invalid` of the pixels -32768; float32: sixteenths,
    `invalid` of the pixels NaN and a further 2 % -32768.0. The first pixel is 30."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    s = 20 + 0.25 * x * (x < cols // 2) + 0.125 * y + 12 * (x >= cols // 2) - 30 * (x % 97 == 96)
    s = s + rng.integers(-8, 9, size=(rows, cols)) / 16
    if np.dtype(dtype) == np.int16:
        d = np.floor(s).astype(np.int16)
        d[rng.random((rows, cols)) < invalid] = -32768
    else:
        d = (np.round(s * 16) / 16).astype(np.float32)
        d[rng.random((rows, cols)) < invalid] = np.nan
        d[rng.random((rows, cols)) < 0.02] = -32768.0
    d.flat[0] = 30
    return d


@functools.lru_cache(maxsize=None)
def case(rows, cols, dtype, flags, max_diff=1.0, seed=1):
    """(map, restatement) under tests/test_cli.py's Q, computed once and shared (read-only)"""
    d = surface(rows, cols, np.dtype(dtype).type, seed)
    d.setflags(write=False)
    return d, restate(d, Q, flags, max_diff)


def conditions(want, rows, cols):
    """what a test map must exercise before a comparison with it means anything (maps with at
    least 128 quads): more triangles than quads are not asked for, but at least as many; quads
    with 2, 1 and 0 triangles; both diagonals; each missing-corner case"""
    quads = (rows - 1) * (cols - 1)
    if quads < 128:
        return
    tri, q2, q1, q0 = (int(c) for c in want["mesh_counts"])
    assert tri >= quads, (tri, quads)
    assert q2 > 0 and q1 > 0 and q0 > 0, (q2, q1, q0)
    assert want["cases"]["ad"] > 0 and want["cases"]["bc"] > 0, want["cases"]
    assert all(m > 0 for m in want["cases"]["missing"]), want["cases"]
