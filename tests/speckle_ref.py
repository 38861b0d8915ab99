"""The speckle filter restated on the CPU (include/bicos_c.h, "speckle filter") -- a helper of
tests/test_speckle_api.py, test_speckle_gpu.py and test_speckle_cli.py, not a test.

restate()     numpy + scipy: the link graph exactly as defined (float32 subtraction, both ends
              valid), components from scipy.sparse.csgraph.connected_components, labels as the
              per-component minimum index, sizes by bincount
flood_fill()  an independent pure-Python flood fill over the same definition (labels, sizes)
patterns()    the maps the tests run, each with its parameters
"""
import os

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

F32_SENTINEL = 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden.npz")


def valid_mask(d, sentinel):
    if d.dtype == np.int16:
        return d != -32768
    v = ~np.isnan(d)
    if sentinel:
        v &= d != np.float32(-32768.0)
    return v


def removed_value(dtype, sentinel):
    if dtype == np.int16:
        return np.int16(-32768)
    return np.float32(-32768.0) if sentinel else np.float32(np.nan)


def restate(d, max_size, max_diff, sentinel=False):
    """-> dict(out, labels int32 [rows, cols], sizes int64 [rows, cols] (0 where invalid),
    counts uint32[4] = kept, removed, invalid, removed_components)"""
    d = np.asarray(d)
    assert d.dtype in (np.int16, np.float32) and d.ndim == 2
    assert max_size >= 0 and max_diff >= 0
    rows, cols = d.shape
    n = rows * cols
    valid = valid_mask(d, sentinel)
    f = d.astype(np.float32)
    md = np.float32(max_diff)
    idx = np.arange(n, dtype=np.int64).reshape(rows, cols)
    with np.errstate(invalid="ignore"):
        right = (np.abs(f[:, :-1] - f[:, 1:]) <= md) & valid[:, :-1] & valid[:, 1:]
        down = (np.abs(f[:-1, :] - f[1:, :]) <= md) & valid[:-1, :] & valid[1:, :]
    a = np.concatenate([idx[:, :-1][right], idx[:-1, :][down]])
    b = np.concatenate([idx[:, 1:][right], idx[1:, :][down]])
    g = coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(n, n))
    ncomp, comp = connected_components(g, directed=False) if n else (0, np.zeros(0, np.int64))
    first = np.full(ncomp, n, np.int64)
    np.minimum.at(first, comp, np.arange(n, dtype=np.int64))
    size = np.bincount(comp, minlength=ncomp)
    labels = np.where(valid.ravel(), first[comp], -1).astype(np.int32).reshape(rows, cols)
    sizes = np.where(valid.ravel(), size[comp], 0).reshape(rows, cols)
    removed = valid & (sizes <= max_size)
    out = d.copy()
    out[removed] = removed_value(d.dtype, sentinel)
    removed_components = int((removed & (labels == idx)).sum())
    counts = np.array([(valid & ~removed).sum(), removed.sum(), (~valid).sum(),
                       removed_components], np.uint32)
    assert int(counts[:3].astype(np.int64).sum()) == n
    return dict(out=out, labels=labels, sizes=sizes, counts=counts)


def flood_fill(d, max_diff, sentinel=False):
    """Pure Python, pixel by pixel in index order, so the first pixel of a component that the
    scan meets is its smallest index. -> (labels int32 [rows, cols], sizes int64 [rows, cols])"""
    d = np.asarray(d)
    rows, cols = d.shape
    md = np.float32(max_diff)
    sent = np.float32(-32768.0)

    def is_valid(v):
        if d.dtype == np.int16:
            return int(v) != -32768
        return not (v != v) and not (sentinel and v == sent)

    vals = [[np.float32(d[r, c]) for c in range(cols)] for r in range(rows)]
    ok = [[is_valid(d[r, c]) for c in range(cols)] for r in range(rows)]
    labels = np.full((rows, cols), -1, np.int32)
    sizes = np.zeros((rows, cols), np.int64)
    seen = [[False] * cols for _ in range(rows)]
    with np.errstate(invalid="ignore"):
        for r0 in range(rows):
            for c0 in range(cols):
                if seen[r0][c0] or not ok[r0][c0]:
                    continue
                seen[r0][c0] = True
                stack, members = [(r0, c0)], []
                while stack:
                    r, c = stack.pop()
                    members.append((r, c))
                    for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                        if 0 <= rr < rows and 0 <= cc < cols and ok[rr][cc] and not seen[rr][cc] \
                                and bool(abs(vals[r][c] - vals[rr][cc]) <= md):
                            seen[rr][cc] = True
                            stack.append((rr, cc))
                for r, c in members:
                    labels[r, c] = r0 * cols + c0
                    sizes[r, c] = len(members)
    return labels, sizes


# ------------------------------------------------------------------------ patterns
def _invalid(dtype):
    return np.int16(-32768) if dtype == np.int16 else np.float32(np.nan)


def _blank(rows, cols, dtype):
    return np.full((rows, cols), _invalid(dtype), dtype)


def serpentine(rows, cols, dtype):
    """a one-pixel-wide path through the whole map: even rows, joined at alternating ends"""
    d = _blank(rows, cols, dtype)
    d[0::2, :] = 5
    for k, r in enumerate(range(1, rows, 2)):
        d[r, cols - 1 if k % 2 == 0 else 0] = 5
    return d


def spiral(rows, cols, dtype):
    """a one-pixel-wide path spiralling inwards (5) between walls of a distant value (1000)"""
    path = np.zeros((rows, cols), bool)
    r, c, dr, dc = 0, 0, 0, 1
    path[0, 0] = True

    def free(rr, cc):  # (rr, cc) may become path: inside, and the cell beyond it is not path
        if not (0 <= rr < rows and 0 <= cc < cols) or path[rr, cc]:
            return False
        ar, ac = rr + dr, cc + dc
        return not (0 <= ar < rows and 0 <= ac < cols and path[ar, ac])

    turns = 0
    while turns < 2:
        if free(r + dr, c + dc):
            r, c = r + dr, c + dc
            path[r, c] = True
            turns = 0
        else:
            dr, dc = dc, -dr
            turns += 1
    d = np.full((rows, cols), 1000, dtype)
    d[path] = 5
    return d


def comb(rows, cols, dtype, along_last_row):
    """teeth joined only along the last row (or the last column): components that unite late"""
    d = _blank(rows, cols, dtype)
    if along_last_row:
        d[:, 0::2] = 5
        d[rows - 1, :] = 5
    else:
        d[0::2, :] = 5
        d[:, cols - 1] = 5
    return d


def hook(rows, cols, dtype):
    """one component whose smallest index, (0, cols-1), lies in the last tile column: down the
    last column, back along the last row, up the first column to row 1"""
    d = _blank(rows, cols, dtype)
    d[:, cols - 1] = 5
    d[rows - 1, :] = 5
    d[1:, 0] = 5
    return d


def blobs(rows, cols, dtype, rng):
    """plateaus 50 apart on a coarse random grid, some pixels invalid"""
    coarse = rng.integers(0, 4, size=(rows // 5 + 1, cols // 7 + 1))
    d = (np.kron(coarse, np.ones((5, 7), np.int64))[:rows, :cols] * 50).astype(dtype)
    d[rng.random((rows, cols)) < 0.08] = _invalid(dtype)
    return d


def surface_with_islands(rows, cols, dtype, rng):
    """a random-walk surface (neighbours within 1) with planted islands 40 above it"""
    walk = np.cumsum(rng.integers(-1, 2, size=cols)) + 100
    d = (walk[None, :] + np.cumsum(rng.integers(0, 2, size=(rows, 1)), axis=0)).astype(np.float64)
    for _ in range(max(1, rows * cols // 150)):
        r, c = int(rng.integers(0, rows)), int(rng.integers(0, cols))
        d[r:r + int(rng.integers(1, 4)), c:c + int(rng.integers(1, 5))] += 40
    d = d.astype(dtype)
    d[rng.random((rows, cols)) < 0.03] = _invalid(dtype)
    return d


def golden_maps():
    """the committed disparity maps of tests/golden/golden.npz (name, map)"""
    z = np.load(GOLDEN)
    return [(k.replace("/", "."), z[k]) for k in z.files if k.endswith("/disparity")]


def patterns(rows, cols, dtype, seed=0):
    """-> list of (name, map, max_size, max_diff, sentinel). dtype: np.int16 or np.float32.
    Sizes on both sides of actual component sizes come from restate() itself."""
    rng = np.random.default_rng(1000 * rows + cols + seed)
    n = rows * cols
    f32 = dtype == np.float32
    out = []

    def add(name, d, max_size, max_diff=1.0, sentinel=False):
        assert d.dtype == dtype and d.shape == (rows, cols)
        out.append((name, d, int(max_size), max_diff, sentinel))

    def both_sides(name, d, max_diff=1.0, sentinel=False, picks=2):
        """max_size just below and at the exact sizes of some of the map's components"""
        sizes = np.unique(restate(d, 0, max_diff, sentinel)["sizes"])
        sizes = sizes[sizes > 0]
        if sizes.size == 0:
            add(name + "-any", d, 3, max_diff, sentinel)
            return
        chosen = {int(sizes[0]), int(sizes[-1])} | {int(s) for s in rng.choice(sizes, picks)}
        for s in sorted(chosen):
            add("%s-below%d" % (name, s), d, s - 1, max_diff, sentinel)
            add("%s-at%d" % (name, s), d, s, max_diff, sentinel)

    const = np.full((rows, cols), 7, dtype)
    add("constant-kept", const, n - 1)
    add("constant-removed", const, n)
    add("constant-size0", const, 0)
    add("all-invalid", _blank(rows, cols, dtype), 5)
    checker = np.where((np.add.outer(np.arange(rows), np.arange(cols)) % 2) == 0, 10, 200).astype(dtype)
    add("checkerboard-removed", checker, 1)
    add("checkerboard-kept", checker, 0)
    add("checkerboard-linked", checker, n - 1, 190.0)
    for name, d in (("serpentine", serpentine(rows, cols, dtype)), ("spiral", spiral(rows, cols, dtype)),
                    ("comb-last-row", comb(rows, cols, dtype, True)),
                    ("comb-last-col", comb(rows, cols, dtype, False)), ("hook", hook(rows, cols, dtype))):
        both_sides(name, d, picks=1)
    both_sides("blobs", blobs(rows, cols, dtype, rng), picks=3)
    both_sides("surface", surface_with_islands(rows, cols, dtype, rng), picks=2)
    if f32:
        d = (rng.random((rows, cols)) * 4).astype(np.float32)
        pair = np.abs(d[0, 0] - d[0, 1]) if cols > 1 else (np.abs(d[0, 0] - d[1, 0]) if rows > 1
                                                            else np.float32(1))
        pair = np.float32(pair)
        for tag, md in (("exact", pair), ("step-below", np.nextafter(pair, np.float32(0))),
                        ("step-above", np.nextafter(pair, np.float32(np.inf)))):
            add("random-floats-" + tag, d, 4, md)
        # NaNs of several payloads, infinities, the sentinel value as a number and as invalid
        d = (rng.integers(0, 3, size=(rows, cols)) * 0.75).astype(np.float32)
        u = d.view(np.uint32)
        pick = rng.random((rows, cols))
        u[pick < 0.05] = 0x7FC00001
        u[(pick >= 0.05) & (pick < 0.08)] = 0xFFC01234
        d[(pick >= 0.08) & (pick < 0.16)] = np.inf
        d[(pick >= 0.16) & (pick < 0.20)] = -np.inf
        d[(pick >= 0.20) & (pick < 0.30)] = -32768.0
        for sentinel in (False, True):
            add("nan-inf-sentinel%d" % sentinel, d, 3, 1.0, sentinel)
            add("nan-inf-maxdiff-inf-sentinel%d" % sentinel, d, 6, np.inf, sentinel)
        add("constant-sentinel-flag", const, n, 1.0, True)
    else:
        d = rng.integers(-3, 4, size=(rows, cols)).astype(np.int16)
        pick = rng.random((rows, cols))
        d[pick < 0.08] = -32768
        d[(pick >= 0.08) & (pick < 0.14)] = 32767
        d[(pick >= 0.14) & (pick < 0.20)] = -32767
        add("int16-extremes", d, 3, 2.0)
        add("int16-extremes-wide", d, 6, 65534.0)
        add("int16-extremes-wide-below", d, 6, 65533.0)
    return out
