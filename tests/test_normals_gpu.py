"""Surface normals on the GPU (libbicos_amd/csrc/normals.hip; include/bicos_c.h, "surface
normals") against restatement (a) of tests/normals_ref.py, which tests/test_normals_api.py
checks against a second restatement and against hand-derived answers. Every comparison is bit
for bit: the normals through uint32 views (NaN payloads included), the counts as integers.
Every output lies between guard values that must survive the call, and the input is compared
after it.
"""
import ctypes
import functools

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import normals_ref as ref

pytestmark = pytest.mark.gpu

PAD = 64  # guard elements (outputs) or bytes times four (the map) on either side
OUT_GUARD = 0x5A5A5A5A
MAP_GUARD = 0xA5
DTYPES = {"int16": np.int16, "float32": np.float32}
INF = float("inf")
bits = ref.bits


def shapes():
    """maps smaller than a window, partial tiles on either side of a full one, 3 x 3 tiles with
    both seams, a map narrower than the halo under a tile seam, and an odd width"""
    tr, tc = _lib.normals_tile()
    return [(1, 1), (1, 7), (7, 1), (2, 2), (tr - 1, tc - 1), (tr, tc), (tr + 1, tc + 1),
            (2 * tr + 3, 2 * tc + 5), (tr + 2, 3), (5, tc + 3)]


@functools.lru_cache(maxsize=None)
def patterns(rows, cols, dtype):
    out = ref.patterns(rows, cols, DTYPES[dtype])
    for _, d, q in out:
        d.setflags(write=False)
        q.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def windows(rows, cols, dtype, name, radius, max_diff, sentinel):
    """the tap loop of the restatement, computed once and shared"""
    d = [p for p in patterns(rows, cols, dtype) if p[0] == name][0][1]
    return ref.windows(d, radius, max_diff, ref.F32_SENTINEL if sentinel else 0)


def want_for(rows, cols, dtype, name, q, flags, radius, max_diff, min_points):
    d = [p for p in patterns(rows, cols, dtype) if p[0] == name][0][1]
    win = windows(rows, cols, dtype, name, radius, max_diff, bool(flags & ref.F32_SENTINEL))
    return ref.finish(d, win, q, flags, min_points)


def an_index(rows, cols, seed=0):
    """shuffled, with repeats and entries outside the map on both sides"""
    rng = np.random.default_rng(seed + rows * 1000 + cols)
    n = rows * cols
    idx = np.concatenate([rng.permutation(n), rng.integers(0, n, 5),
                          np.array([-1, n, n + 7, -2 ** 31, 2 ** 31 - 1])])
    return rng.permutation(idx).astype(np.int32)


def run(handle, d, q, flags=0, radius=2, max_diff=1.0, min_points=3, want_map=True, index=None,
        want_counts=True, stream=None, offset=0, host=False):
    """bicos_normals_device (or _host) on a numpy map -> dict(map, normals, counts) of numpy
    results. Every device output lies between PAD guard elements, checked here, and the input,
    itself between guard bytes at `offset` bytes past a 256-byte boundary, is compared after
    the call."""
    import torch
    L = _lib.lib()
    rows, cols = d.shape
    n = rows * cols
    typ = _lib.CV_32F if d.dtype == np.float32 else _lib.CV_16S
    qa = _lib.reproject_q(q)
    r, diff, m = _lib.normals_params(radius, max_diff, min_points)
    count = 0 if index is None else len(index)
    if host:
        src = np.array(d)
        nmap = np.full((n * 3 + 1,), OUT_GUARD, np.uint32) if want_map else None
        lst = np.full((count * 3 + 1,), OUT_GUARD, np.uint32) if index is not None else None
        idx = np.append(np.asarray(index, np.int32), np.int32(0)) if index is not None else None
        cnt = (ctypes.c_uint32 * 4)(9, 9, 9, 9) if want_counts else None
        rc = L.bicos_normals_host(handle, src.ctypes.data, typ, rows, cols, qa, flags, r, diff, m,
                                  nmap.ctypes.data if want_map else None,
                                  idx.ctypes.data if index is not None else None, count,
                                  lst.ctypes.data if index is not None else None, cnt)
        _lib.check(rc, "bicos_normals_host")
        assert np.array_equal(src.view(np.uint8), np.array(d).view(np.uint8)), "the input was changed"
        got = {}
        if want_map:
            assert nmap[-1] == OUT_GUARD
            got["map"] = nmap[:-1].view(np.float32).reshape(rows, cols, 3)
        if index is not None:
            assert lst[-1] == OUT_GUARD
            got["normals"] = lst[:-1].view(np.float32).reshape(count, 3)
        if want_counts:
            got["counts"] = np.array(list(cnt), np.uint32)
        return got

    dev = torch.device("cuda", 0)
    raw = np.array(d).reshape(-1).view(np.uint8)
    lead = 4 * PAD + offset
    src = torch.full((lead + raw.size + 4 * PAD,), MAP_GUARD, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 256 == 0 and offset % d.dtype.itemsize == 0
    src[lead:lead + raw.size] = torch.from_numpy(raw.copy()).to(dev)

    def guarded(elems):
        return torch.full((elems + 2 * PAD,), OUT_GUARD, dtype=torch.int32, device=dev)

    nmap = guarded(n * 3) if want_map else None
    lst = guarded(count * 3) if index is not None else None
    cnt = guarded(4) if want_counts else None
    idx = torch.from_numpy(np.append(np.asarray(index, np.int32), np.int32(0))).to(dev) \
        if index is not None else None
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    at = lambda t: t.data_ptr() + PAD * 4 if t is not None else None  # noqa: E731
    rc = L.bicos_normals_device(handle, src.data_ptr() + lead, typ, rows, cols, qa, flags, r, diff, m,
                                at(nmap), idx.data_ptr() if idx is not None else None, count,
                                at(lst), at(cnt), s.cuda_stream)
    _lib.check(rc, "bicos_normals_device")
    s.synchronize()

    def inner(t):
        h = t.cpu().numpy().view(np.uint32)
        edge = np.concatenate([h[:PAD], h[h.size - PAD:]])
        assert (edge == OUT_GUARD).all(), "guard values overwritten"
        return h[PAD:h.size - PAD]

    back = src.cpu().numpy()
    assert (back[:lead] == MAP_GUARD).all() and (back[lead + raw.size:] == MAP_GUARD).all()
    assert np.array_equal(back[lead:lead + raw.size], raw), "the input was changed"
    got = {}
    if want_map:
        got["map"] = inner(nmap).view(np.float32).reshape(rows, cols, 3)
    if index is not None:
        got["normals"] = inner(lst).view(np.float32).reshape(count, 3)
    if want_counts:
        got["counts"] = inner(cnt)
    return got


def check(got, want, index=None, name=""):
    if "map" in got:
        assert np.array_equal(bits(got["map"]), bits(want["map"])), name
    if "normals" in got:
        assert np.array_equal(bits(got["normals"]), bits(ref.gather(want["map"], index))), name
    if "counts" in got:
        assert got["counts"].tolist() == want["counts"].tolist(), name


# ------------------------------------------------------------- shapes x patterns
@pytest.mark.parametrize("radius", [1, 2, 4])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("shape_at", range(10))
def test_every_pattern_at_every_shape(gpu, shape_at, dtype, radius):
    """every pattern x max_diff in {0, 1, +inf} x min_points in {3, the full window}, the flags
    taking turns: map and counts bit for bit, and with the full window the list in the same call"""
    assert len(shapes()) == 10
    rows, cols = shapes()[shape_at]
    full = (2 * radius + 1) ** 2
    index = an_index(rows, cols)
    total = np.zeros(4, np.uint64)
    turn = 0
    for name, d, q in patterns(rows, cols, dtype):
        for max_diff in (0.0, 1.0, INF):
            flags = turn % 4
            turn += 1
            for min_points in (3, full):
                want = want_for(rows, cols, dtype, name, q, flags, radius, max_diff, min_points)
                idx = index if min_points == full else None
                got = run(gpu._h, d, q, flags, radius, max_diff, min_points, index=idx)
                check(got, want, idx, (name, max_diff, min_points, flags))
                total += want["counts"]
    assert total[1] and total[2]
    if rows > 2 * radius and cols > 2 * radius:  # the cases exercise every class
        assert total[0] and total[3]


def test_the_shapes_are_what_they_are_for():
    tr, tc = _lib.normals_tile()
    s = shapes()
    assert (tr, tc) in s and (tr - 1, tc - 1) in s and (tr + 1, tc + 1) in s
    assert max(r for r, _ in s) <= 3 * tr and max(c for _, c in s) <= 3 * tc
    assert any(r > 2 * tr and c > 2 * tc for r, c in s)
    assert any(c < 4 and r > tr for r, c in s)  # narrower than the widest halo, under a seam
    assert any(c % 2 == 1 and r > 1 for r, c in s)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_both_flags(gpu, dtype):
    rows, cols = shapes()[7]
    seen = set()
    for name in ("special", "odd-q", "random-holes"):
        d, q = [p for p in patterns(rows, cols, dtype) if p[0] == name][0][1:]
        for flags in (0, 1, 2, 3):
            want = want_for(rows, cols, dtype, name, q, flags, 2, 1.0, 3)
            check(run(gpu._h, d, q, flags, 2, 1.0, 3), want, None, (name, flags))
            seen.add((name, flags, tuple(want["counts"].tolist())))
    # the flags matter: negative Z on odd-q; the sentinel on the float maps that hold it, once
    # negative Z is allowed (without the sentinel flag -32768.0 is a number, whose point lies
    # behind the camera: no point either way, but a lone sparse one where Z < 0 is kept)
    by = {(n, f): c for n, f, c in seen}
    assert by[("odd-q", 0)] != by[("odd-q", 1)]
    if dtype == "float32":
        assert by[("special", 1)] != by[("special", 3)]


@pytest.mark.parametrize("dtype,offset", [("int16", 2), ("int16", 4), ("int16", 8),
                                          ("float32", 4), ("float32", 8)])
def test_map_bases_off_a_16_byte_boundary(gpu, dtype, offset):
    rows, cols = shapes()[7]
    name = "random-holes"
    d, q = [p for p in patterns(rows, cols, dtype) if p[0] == name][0][1:]
    index = an_index(rows, cols, 3)
    for radius in (1, 4):
        want = want_for(rows, cols, dtype, name, q, 2, radius, 1.0, 3)
        check(run(gpu._h, d, q, 2, radius, 1.0, 3, index=index, offset=offset), want, index, radius)


def test_a_map_of_more_tiles_than_workgroups(gpu):
    """more than 1024 tiles: the workgroups stride over the tiles and sum their counts"""
    tr, tc = _lib.normals_tile()
    rows, cols = 1030 * tr + 5, 3
    r, c = np.mgrid[0:rows, 0:cols]
    d = (30 + 0.25 * c + ((r * 7) % 13) * 0.125).astype(np.float32)
    d[(r * 5 + c) % 11 == 0] = np.nan
    q = ref.rig_q(rows, cols)
    want = ref.restate(d, q, 0, 1, 1.0, 5)
    assert want["counts"][0] and want["counts"][1] and want["counts"][2]
    check(run(gpu._h, d, q, 0, 1, 1.0, 5), want)


# ------------------------------------------------------------------ call forms
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_list_forms(gpu, dtype):
    rows, cols = shapes()[6]
    name = "step"
    d, q = [p for p in patterns(rows, cols, dtype) if p[0] == name][0][1:]
    want = want_for(rows, cols, dtype, name, q, 0, 2, 1.0, 3)
    index = an_index(rows, cols, 1)
    assert (index < 0).any() and (index >= rows * cols).any()
    assert len(np.unique(index)) < len(index)
    # the list alone, with and without an engine
    for h in (gpu._h, None):
        got = run(h, d, q, 0, 2, 1.0, 3, want_map=False, index=index, want_counts=False)
        assert set(got) == {"normals"}
        check(got, want, index)
    # both outputs and the counts in one call
    got = run(gpu._h, d, q, 0, 2, 1.0, 3, index=index)
    assert set(got) == {"map", "normals", "counts"}
    check(got, want, index)
    # count = 0, beside a map and alone
    got = run(gpu._h, d, q, 0, 2, 1.0, 3, index=np.zeros(0, np.int32))
    assert got["normals"].shape == (0, 3)
    check(got, want, np.zeros(0, np.int32))
    got = run(gpu._h, d, q, 0, 2, 1.0, 3, want_map=False, index=np.zeros(0, np.int32), want_counts=False)
    assert got["normals"].shape == (0, 3)
    # the map alone, without counts and without an engine
    got = run(None, d, q, 0, 2, 1.0, 3, want_counts=False)
    assert set(got) == {"map"}
    check(got, want)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_the_host_entry_equals_the_device_entry(gpu, dtype):
    rows, cols = shapes()[7]
    index = an_index(rows, cols, 2)
    for name, radius, flags in (("random-holes", 2, 2), ("odd-q", 4, 1)):
        d, q = [p for p in patterns(rows, cols, dtype) if p[0] == name][0][1:]
        want = want_for(rows, cols, dtype, name, q, flags, radius, 1.0, 3)
        dev = run(gpu._h, d, q, flags, radius, 1.0, 3, index=index)
        for h in (gpu._h, None):
            host = run(h, d, q, flags, radius, 1.0, 3, index=index, host=True)
            for k in ("map", "normals", "counts"):
                assert host[k].tobytes() == dev[k].tobytes(), k
            check(host, want, index)
        only = run(None, d, q, flags, radius, 1.0, 3, want_map=False, index=index,
                   want_counts=False, host=True)
        assert set(only) == {"normals"}
        check(only, want, index)


def test_a_dependent_copy_on_a_non_default_stream_sees_the_result(gpu):
    import torch
    rows, cols = shapes()[7]
    name = "tilted"
    d, q = [p for p in patterns(rows, cols, "float32") if p[0] == name][0][1:]
    want = want_for(rows, cols, "float32", name, q, 0, 4, 1.0, 3)
    t = torch.from_numpy(np.array(d)).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    cnt = torch.zeros((4,), dtype=torch.int32, device=t.device)
    out = gpu.normals_map(t, q, radius=4, counts=cnt, stream=s)
    with torch.cuda.stream(s):
        copy = out.clone()
        cnt2 = cnt.clone()
    s.synchronize()
    assert np.array_equal(bits(copy.cpu().numpy()), bits(want["map"]))
    assert cnt2.cpu().numpy().view(np.uint32).tolist() == want["counts"].tolist()
    check(run(gpu._h, d, q, 0, 4, 1.0, 3, stream=torch.cuda.Stream()), want)


def test_same_call_twice_gives_the_same_bytes(gpu):
    rows, cols = shapes()[7]
    d, q = [p for p in patterns(rows, cols, "float32") if p[0] == "random-holes"][0][1:]
    a = run(gpu._h, d, q, 2, 4, INF, 3, index=an_index(rows, cols))
    b = run(gpu._h, d, q, 2, 4, INF, 3, index=an_index(rows, cols))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("rows,cols", [(0, 5), (5, 0), (0, 0)])
def test_empty_maps(gpu, rows, cols):
    import torch
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    q = _lib.reproject_q(ref.rig_q(4, 4))
    cnt = torch.full((4,), 9, dtype=torch.int32, device=dev)
    nmap = torch.full((4,), 7, dtype=torch.int32, device=dev)  # nothing of it is written
    idx = torch.tensor([0, 3, -1], dtype=torch.int32, device=dev)
    lst = torch.zeros((3, 3), dtype=torch.float32, device=dev)
    rc = L.bicos_normals_device(None, None, _lib.CV_16S, rows, cols, q, 0, 2, 1.0, 3,
                                nmap.data_ptr(), idx.data_ptr(), 3, lst.data_ptr(), cnt.data_ptr(),
                                None)
    assert rc == 0, L.bicos_last_error()
    torch.cuda.synchronize()
    assert cnt.tolist() == [0, 0, 0, 0] and nmap.tolist() == [7, 7, 7, 7]
    assert (bits(lst.cpu().numpy()) == 0x7FC00000).all()
    t = torch.zeros((rows, cols), dtype=torch.float32, device=dev)
    cnt.fill_(9)
    assert gpu.normals_map(t, ref.rig_q(4, 4), counts=cnt).shape == (rows, cols, 3)
    assert cnt.tolist() == [0, 0, 0, 0]
    got = gpu.normals_points(t, ref.rig_q(4, 4), idx)
    assert (bits(got.cpu().numpy()) == 0x7FC00000).all()


# ------------------------------------------------------------------- every API
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_engine_and_pybicos(gpu, dtype):
    import torch
    from libbicos_amd import pybicos
    rows, cols = shapes()[7]
    name = "random-holes"
    d, q = [p for p in patterns(rows, cols, dtype) if p[0] == name][0][1:]
    index = an_index(rows, cols, 4)
    t = torch.from_numpy(np.array(d)).cuda()
    it = torch.from_numpy(index).cuda()
    for sentinel in (False, True):
        flags = ref.F32_SENTINEL if sentinel else 0
        want = want_for(rows, cols, dtype, name, q, flags, 2, 1.0, 3)
        cnt = torch.zeros((4,), dtype=torch.int32, device=t.device)
        out = gpu.normals_map(t, q, sentinel=sentinel, counts=cnt)
        check(dict(map=out.cpu().numpy(), counts=cnt.cpu().numpy().view(np.uint32)), want)
        given = torch.empty((rows, cols, 3), dtype=torch.float32, device=t.device)
        assert gpu.normals_map(t, q, sentinel=sentinel, out=given) is given
        assert np.array_equal(bits(given.cpu().numpy()), bits(want["map"]))
        lst = gpu.normals_points(t, q, it, sentinel=sentinel)
        check(dict(normals=lst.cpu().numpy()), want, index)
        nmap = torch.empty_like(given)
        cnt.zero_()
        lst = gpu.normals_points(t, q, it, sentinel=sentinel, normal_map=nmap, counts=cnt)
        check(dict(map=nmap.cpu().numpy(), normals=lst.cpu().numpy(),
                   counts=cnt.cpu().numpy().view(np.uint32)), want, index)
        assert np.array_equal(bits(pybicos.normals(d, q, sentinel=sentinel)), bits(want["map"]))
        check(dict(normals=pybicos.normals(d, q, sentinel=sentinel, index=index)), want, index)
        assert np.array_equal(t.cpu().numpy().view(np.uint8), np.array(d).view(np.uint8))
    # other parameters reach the kernel
    want = want_for(rows, cols, dtype, name, q, 1, 4, INF, 81)
    out = gpu.normals_map(t, q, radius=4, max_diff=INF, min_points=81, allow_negative_z=True)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want["map"]))
    got = pybicos.normals(d, q, 4, INF, 81, True, False)
    assert np.array_equal(bits(got), bits(want["map"]))
    with pytest.raises(ValueError):
        gpu.normals_map(t, q, out=torch.zeros((rows, cols), device="cuda"))
    with pytest.raises(ValueError, match="radius"):
        gpu.normals_map(t, q, radius=5)
    with pytest.raises(ValueError, match="counts"):
        gpu.normals_points(t, q, it, counts=torch.zeros((4,), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        gpu.normals_points(t, q, it.to(torch.int64))


def test_match_reproject_normals_on_the_device(gpu):
    """Engine.match with a subpixel step -> reproject_points with index -> normals_points,
    without leaving the GPU, against the restatement applied to the downloaded map; and the
    same list through pybicos."""
    import torch
    from libbicos_amd import device, pybicos
    from libbicos_amd.synthetic import stereo_stack
    from tests.test_cli import Q
    L, R = stereo_stack(12, 40, 200)
    disp, _ = gpu.match(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(),
                        device.MatchConfig(nxcorr_threshold=0.75, subpixel_step=0.2))
    assert disp.dtype == torch.float32
    pts, idx, stats = gpu.reproject_points(disp, Q, with_index=True)
    assert stats["kept"] > 100
    lst = gpu.normals_points(disp, Q, idx, radius=2, max_diff=1.0, sentinel=True)
    d = disp.cpu().numpy()
    want = ref.restate(d, Q, ref.F32_SENTINEL, 2, 1.0, 3)
    index = idx.cpu().numpy()
    assert want["counts"][0] > 100
    # a listed pixel is one reproject keeps: never no_point
    assert (want["cls"].reshape(-1)[index] != ref.NO_POINT).all()
    check(dict(normals=lst.cpu().numpy()), want, index)
    assert lst.shape[0] == pts.shape[0]
    check(dict(normals=pybicos.normals(d, Q, index=index)), want, index)
    assert np.array_equal(bits(pybicos.normals(d, Q)), bits(want["map"]))
