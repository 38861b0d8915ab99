"""The ten staged host entries (libbicos_amd/csrc/host.cpp: median, mesh, pool, reproject,
rectify_maps, rectify, speckle, normals, guide and the pyramid match) called one after the other
on one engine, so that consecutive calls lay the engine's one staging buffer out differently,
in three rounds of shapes: less than a tile, then a tile and a remainder (the staging must
grow), then the first shapes again. Every output is compared byte for byte with the same
stage's *_device entry on the same input held in torch tensors, and the third round's bytes
with the first round's. The point lists of reproject and mesh are asked for with their full
capacity, half the kept count and 0 into buffers prefilled with a marker: exactly
min(count, capacity) entries may be written. Every entry with optional outputs runs once
without them. Once on a created engine, once on the NULL engine (the process-wide default one).
"""
import ctypes
import functools

import numpy as np
import pytest

from libbicos_amd import _lib
from libbicos_amd.synthetic import random_stack, stereo_stack
from tests import median_ref, normals_ref, rectify_ref

pytestmark = pytest.mark.gpu

ROUNDS = ("small", "large", "small")
FLAVOURS = ("i16", "f32")  # of the maps; the stacks are u8 / u16, the pyramid match raw / NXC
FMARK, IMARK, UMARK = np.float32(-777.25), np.int32(-7), np.uint32(0x5A5A5A5A)
WINDOW = (0, 63)
PYRAMID_SHAPE = {"small": (8, 24, 160), "large": (8, 30, 176)}  # (tests/test_pool_gpu.py: n8_u8)
GUIDE = dict(radius=2, spread=1, scale=2, fallback=(-5, 70))


def shape(tile, kind):
    """odd sizes below one tile, or one tile and a remainder, in both directions"""
    tr, tc = tile
    small = (min(9, tr - 1), min(13, tc - 1))
    assert small[0] % 2 == 1 and small[1] % 2 == 1 and small[0] < tr and small[1] < tc
    return small if kind == "small" else (tr + 3, tc + 5)


@functools.lru_cache(maxsize=None)
def disparity(rows, cols, flavour):
    """a seeded map with about 30 % invalid pixels (tests/median_ref.py), the valid ones moved
    in front of the camera so that reproject and mesh keep them"""
    dtype = np.int16 if flavour == "i16" else np.float32
    name, d, sentinel = median_ref.patterns(rows, cols, dtype)[0]
    assert name.startswith("random30") and not sentinel
    d = d.copy()
    valid = median_ref.valid_mask(d, False)
    assert 0.4 < valid.mean() < 0.95
    d[valid] = np.abs(d[valid]) + dtype(8)
    d.setflags(write=False)
    return d


def cv_type(d):
    return _lib.CV_32F if d.dtype == np.float32 else _lib.CV_16S


def to_dev(a):
    import torch
    a = np.array(a)  # (a writable copy: the inputs are shared and read-only)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def to_host(t):
    return t.cpu().numpy()


def ptr(a):
    return None if a is None else a.ctypes.data


def marked(shape_, dtype):
    mark = {np.dtype(np.float32): FMARK, np.dtype(np.int32): IMARK, np.dtype(np.uint32): UMARK}
    return np.full(shape_, mark.get(np.dtype(dtype), 0x5A), dtype)


def untouched(a):
    return a.tobytes() == marked(a.shape, a.dtype).tobytes()


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, (what, k)
        assert g.tobytes() == w.tobytes(), (what, k)


# ---------------------------------------------------------------------- median
def median_inputs(kind, flavour):
    return disparity(*shape(_lib.median_tile(), kind), flavour)


def median_device(gpu, d, optional=True):
    import torch
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda") if optional else None
    out = gpu.median_filter(to_dev(d), 5, 3, sentinel=False, counts=cnt)
    res = dict(out=to_host(out))
    if optional:
        res["counts"] = to_host(cnt)
    return res


def median_host(h, d, optional=True):
    out = marked(d.shape, d.dtype)
    cnt = marked(4, np.uint32) if optional else None
    rc = _lib.lib().bicos_median_host(h, ptr(d), cv_type(d), d.shape[0], d.shape[1], 5, 3, 0,
                                      ptr(out), ptr(cnt))
    _lib.check(rc, "bicos_median_host")
    res = dict(out=out)
    if optional:
        res["counts"] = cnt
    return res


# --------------------------------------------------------------------- speckle
def speckle_inputs(kind, flavour):
    return disparity(*shape(_lib.speckle_tile(), kind), flavour)


def speckle_device(gpu, d, optional=True):
    import torch
    if not optional:
        return dict(out=to_host(gpu.filter_speckles(to_dev(d), 4, 1.0, sentinel=False)))
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    out, lab = gpu.filter_speckles(to_dev(d), 4, 1.0, sentinel=False, labels=True, counts=cnt)
    return dict(out=to_host(out), labels=to_host(lab), counts=to_host(cnt))


def speckle_host(h, d, optional=True):
    out = marked(d.shape, d.dtype)
    lab = marked(d.shape, np.int32) if optional else None
    cnt = marked(4, np.uint32) if optional else None
    rc = _lib.lib().bicos_speckle_host(h, ptr(d), cv_type(d), d.shape[0], d.shape[1], 4, 1.0, 0,
                                       ptr(out), ptr(lab), ptr(cnt))
    _lib.check(rc, "bicos_speckle_host")
    return dict(out=out, labels=lab, counts=cnt) if optional else dict(out=out)


# ------------------------------------------------------------------- reproject
def reproject_inputs(kind, flavour):
    d = disparity(*shape(_lib.speckle_tile(), kind), flavour)
    if kind == "large":
        assert d.size > _lib.lib().bicos_reproject_segment()  # more than one segment
    return d


def reproject_device(gpu, d, capacity, optional=True):
    """capacity None: the dense map alone; else the list (with the map and the index if
    `optional`) -> the counts and the first min(kept, capacity) entries"""
    import torch
    rows, cols = d.shape
    q = _lib.reproject_q(normals_ref.rig_q(rows, cols))
    xyz = torch.empty((rows, cols, 3), dtype=torch.float32, device="cuda")
    src = to_dev(d)
    if capacity is None:
        rc = gpu._L.bicos_reproject_device(gpu._h, src.data_ptr(), cv_type(d), rows, cols, q,
                                           0, xyz.data_ptr(), None, None, 0, None,
                                           torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "bicos_reproject_device")
        return dict(xyz=to_host(xyz))
    pts = torch.empty((capacity + 1, 3), dtype=torch.float32, device="cuda")
    idx = torch.empty((capacity + 1,), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    rc = gpu._L.bicos_reproject_device(gpu._h, src.data_ptr(), cv_type(d), rows, cols, q, 0,
                                       xyz.data_ptr() if optional else None, pts.data_ptr(),
                                       idx.data_ptr() if optional else None, capacity,
                                       cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "bicos_reproject_device")
    counts = to_host(cnt)
    got = min(int(counts.view(np.uint32)[0]), capacity)
    res = dict(counts=counts, points=to_host(pts)[:got])
    if optional:
        res.update(xyz=to_host(xyz), index=to_host(idx)[:got])
    return res


def reproject_host(h, d, capacity, optional=True):
    rows, cols = d.shape
    q = _lib.reproject_q(normals_ref.rig_q(rows, cols))
    xyz = marked((rows, cols, 3), np.float32)
    if capacity is None:
        rc = _lib.lib().bicos_reproject_host(h, ptr(d), cv_type(d), rows, cols, q, 0, ptr(xyz),
                                             None, None, 0, None)
        _lib.check(rc, "bicos_reproject_host")
        return dict(xyz=xyz)
    pts = marked((d.size + 1, 3), np.float32)
    idx = marked(d.size + 1, np.int32)
    cnt = marked(4, np.uint32)
    rc = _lib.lib().bicos_reproject_host(h, ptr(d), cv_type(d), rows, cols, q, 0,
                                         ptr(xyz) if optional else None, ptr(pts),
                                         ptr(idx) if optional else None, capacity, ptr(cnt))
    _lib.check(rc, "bicos_reproject_host")
    got = min(int(cnt[0]), capacity)
    # exactly min(kept, capacity) entries were written
    assert untouched(pts[got:]), "points written past min(kept, capacity)"
    assert got == 0 or not untouched(pts[got - 1:got])
    res = dict(counts=cnt, points=pts[:got])
    if optional:
        assert untouched(idx[got:]), "index written past min(kept, capacity)"
        res.update(xyz=xyz, index=idx[:got])
    else:
        assert untouched(xyz) and untouched(idx)
    return res


# ------------------------------------------------------------------------ mesh
def mesh_inputs(kind, flavour):
    return disparity(*shape(_lib.normals_tile(), kind), flavour)


def mesh_device(gpu, d, vcap, tcap, optional=True):
    import torch
    rows, cols = d.shape
    q = _lib.reproject_q(normals_ref.rig_q(rows, cols))
    pts = torch.empty((vcap + 1, 3), dtype=torch.float32, device="cuda")
    idx = torch.empty((vcap + 1,), dtype=torch.int32, device="cuda")
    tri = torch.empty((tcap + 1, 3), dtype=torch.int32, device="cuda")
    vmap = torch.empty((rows, cols), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    src = to_dev(d)
    rc = gpu._L.bicos_mesh_device(gpu._h, src.data_ptr(), cv_type(d), rows, cols, q, 0, 1.0,
                                  pts.data_ptr(), idx.data_ptr() if optional else None, vcap,
                                  cnt.data_ptr(), tri.data_ptr(), tcap, cnt.data_ptr() + 16,
                                  vmap.data_ptr() if optional else None,
                                  torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "bicos_mesh_device")
    counts = to_host(cnt)
    verts = min(int(counts.view(np.uint32)[0]), vcap)
    tris = min(int(counts.view(np.uint32)[4]), tcap)
    res = dict(counts=counts, points=to_host(pts)[:verts], triangles=to_host(tri)[:tris])
    if optional:
        res.update(index=to_host(idx)[:verts], vertex_map=to_host(vmap))
    return res


def mesh_host(h, d, vcap, tcap, optional=True):
    rows, cols = d.shape
    q = _lib.reproject_q(normals_ref.rig_q(rows, cols))
    pts = marked((d.size + 1, 3), np.float32)
    idx = marked(d.size + 1, np.int32)
    tri = marked((2 * _lib.mesh_quads(rows, cols) + 1, 3), np.int32)
    vmap = marked((rows, cols), np.int32)
    cnt = marked(8, np.uint32)
    rc = _lib.lib().bicos_mesh_host(h, ptr(d), cv_type(d), rows, cols, q, 0, 1.0, ptr(pts),
                                    ptr(idx) if optional else None, vcap, ptr(cnt), ptr(tri),
                                    tcap, ptr(cnt) + 16, ptr(vmap) if optional else None)
    _lib.check(rc, "bicos_mesh_host")
    verts, tris = min(int(cnt[0]), vcap), min(int(cnt[4]), tcap)
    assert untouched(pts[verts:]), "points written past min(kept, vertex_capacity)"
    assert untouched(tri[tris:]), "triangles written past min(triangles, tri_capacity)"
    assert verts == 0 or not untouched(pts[verts - 1:verts])
    assert tris == 0 or not untouched(tri[tris - 1:tris])
    res = dict(counts=cnt, points=pts[:verts], triangles=tri[:tris])
    if optional:
        assert untouched(idx[verts:]), "index written past min(kept, vertex_capacity)"
        res.update(index=idx[:verts], vertex_map=vmap)
    else:
        assert untouched(idx) and untouched(vmap)
    return res


# --------------------------------------------------------------------- normals
def normals_inputs(kind, flavour):
    d = disparity(*shape(_lib.normals_tile(), kind), flavour)
    rng = np.random.default_rng(d.size)
    index = rng.integers(0, d.size, 19).astype(np.int32)
    index[3], index[11] = -1, d.size + 2  # outside the map: three NaNs
    return d, index


def normals_device(gpu, d, index, optional=True):
    """optional False: the list alone (no map, no counts)"""
    import torch
    q = normals_ref.rig_q(*d.shape)
    if not optional:
        return dict(normals=to_host(gpu.normals_points(to_dev(d), q, to_dev(index))))
    nm = torch.empty(d.shape + (3,), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    lst = gpu.normals_points(to_dev(d), q, to_dev(index), normal_map=nm, counts=cnt)
    return dict(normals=to_host(lst), normal_map=to_host(nm), counts=to_host(cnt))


def normals_host(h, d, index, optional=True):
    rows, cols = d.shape
    q = _lib.reproject_q(normals_ref.rig_q(rows, cols))
    nm = marked((rows, cols, 3), np.float32) if optional else None
    cnt = marked(4, np.uint32) if optional else None
    lst = marked((index.size, 3), np.float32)
    rc = _lib.lib().bicos_normals_host(h, ptr(d), cv_type(d), rows, cols, q, 0, 2, 1.0, 3, ptr(nm),
                                       ptr(index), index.size, ptr(lst), ptr(cnt))
    _lib.check(rc, "bicos_normals_host")
    return dict(normals=lst, normal_map=nm, counts=cnt) if optional else dict(normals=lst)


def normals_map_device(gpu, d):
    return dict(normal_map=to_host(gpu.normals_map(to_dev(d), normals_ref.rig_q(*d.shape))))


def normals_map_host(h, d):
    """the dense map alone: no list, no counts"""
    rows, cols = d.shape
    q = _lib.reproject_q(normals_ref.rig_q(rows, cols))
    nm = marked((rows, cols, 3), np.float32)
    rc = _lib.lib().bicos_normals_host(h, ptr(d), cv_type(d), rows, cols, q, 0, 2, 1.0, 3, ptr(nm),
                                       None, 0, None, None)
    _lib.check(rc, "bicos_normals_host")
    return dict(normal_map=nm)


# ----------------------------------------------------------------------- guide
def guide_inputs(kind, flavour):
    rows, cols = shape(_lib.median_tile(), kind)
    return disparity((rows + 1) // 2, (cols + 1) // 2, flavour), rows, cols


def guide_device(gpu, prior, rows, cols, optional=True):
    import torch
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda") if optional else None
    g = gpu.guide_from_disparity(to_dev(prior), GUIDE["radius"], GUIDE["spread"], GUIDE["scale"],
                                 GUIDE["fallback"], shape=(rows, cols), sentinel=False, counts=cnt)
    res = dict(guide=to_host(g))
    if optional:
        res["counts"] = to_host(cnt)
    return res


def guide_host(h, prior, rows, cols, optional=True):
    """into rows three pairs wider than the guide: what lies between them stays"""
    pitch = cols + 3
    g = np.full((rows, pitch, 2), 0x5A5A, np.int16)
    cnt = marked(2, np.uint32) if optional else None
    rc = _lib.lib().bicos_guide_host(h, ptr(prior), cv_type(prior), prior.shape[0], prior.shape[1],
                                     rows, cols, GUIDE["scale"], GUIDE["radius"], GUIDE["spread"],
                                     GUIDE["fallback"][0], GUIDE["fallback"][1], 0, ptr(g), pitch,
                                     ptr(cnt))
    _lib.check(rc, "bicos_guide_host")
    assert (g[:, cols:] == 0x5A5A).all(), "bicos_guide_host wrote between the guide's rows"
    res = dict(guide=np.ascontiguousarray(g[:, :cols]))
    if optional:
        res["counts"] = cnt
    return res


# ------------------------------------------------------------------------ pool
def stack_dtype(flavour):
    return np.uint8 if flavour == "i16" else np.uint16


def pool_inputs(kind, flavour):
    scale = 2 if kind == "small" else 3
    prows, pcols = shape(_lib.pool_tile(), kind)
    dt = stack_dtype(flavour)
    # one row and one column more than the launch reads
    s = random_stack(3, prows * scale + 1, pcols * scale + 1, dt, seed=5,
                     maxval=np.iinfo(dt).max)
    return s, scale


def pool_device(gpu, s, scale):
    return dict(out=to_host(gpu.pool(to_dev(s), scale)))


def padded_images(s, extra, fill):
    """the planes of `s` in rows `extra` elements wider -> (array, ctypes pointer list)"""
    wide = np.full(s.shape[:2] + (s.shape[2] + extra,), fill, s.dtype)
    wide[:, :, :s.shape[2]] = s
    return wide, (ctypes.c_void_p * s.shape[0])(*[wide[t].ctypes.data for t in range(s.shape[0])])


def pool_host(h, s, scale):
    n, rows, cols = s.shape
    prows, pcols = rows // scale, cols // scale
    wide, src = padded_images(s, 5, 7)
    out, dst = padded_images(np.zeros((n, prows, pcols), s.dtype), 3, 9)
    rc = _lib.lib().bicos_pool_host(h, src, n, rows, cols, wide.shape[2] * s.itemsize, s.itemsize,
                                    scale, dst, out.shape[2] * s.itemsize)
    _lib.check(rc, "bicos_pool_host")
    assert (out[:, :, pcols:] == 9).all(), "bicos_pool_host wrote between the output rows"
    return dict(out=np.ascontiguousarray(out[:, :, :pcols]))


# --------------------------------------------------------------------- rectify
def rectify_inputs(kind, flavour):
    rows, cols = shape(_lib.rectify_tile(), kind)
    dt = stack_dtype(flavour)
    return rectify_ref.images(3, rows + 2, cols + 4, dt, seed=rows), rows, cols


def camera_args(s, rows, cols):
    K, D, R, P = rectify_ref.camera(s.shape[1], s.shape[2])
    return K, D, R, P, (rows, cols)


def rectify_maps_device(gpu, s, rows, cols):
    mx, my = gpu.rectify_maps(*camera_args(s, rows, cols))
    return dict(map_x=to_host(mx), map_y=to_host(my))


def rectify_maps_host(s, rows, cols):
    """(the entry takes no engine: it runs on the default one)"""
    mx, my = marked((rows, cols), np.float32), marked((rows, cols), np.float32)
    k, d, nd, r, p, p_cols, rows, cols = _lib.rectify_camera(*camera_args(s, rows, cols))
    rc = _lib.lib().bicos_rectify_maps_host(k, d, nd, r, p, p_cols, rows, cols, ptr(mx), ptr(my))
    _lib.check(rc, "bicos_rectify_maps_host")
    return dict(map_x=mx, map_y=my)


def rectify_device(gpu, s, maps, optional=True):
    mx, my = to_dev(maps["map_x"]), to_dev(maps["map_y"])
    if not optional:
        return dict(out=to_host(gpu.rectify(to_dev(s), mx, my, border=3)))
    out, val = gpu.rectify(to_dev(s), mx, my, border=3, valid=True)
    return dict(out=to_host(out), valid=to_host(val))


def rectify_host(h, s, maps, optional=True):
    """images and maps in rows wider than they need: what lies between them stays"""
    n, rows, cols = (s.shape[0],) + maps["map_x"].shape
    wide, src = padded_images(s, 5, 7)
    out, dst = padded_images(np.zeros((n, rows, cols), s.dtype), 3, 9)
    mx = np.full((rows, cols + 2), FMARK, np.float32)
    my = np.full((rows, cols + 2), FMARK, np.float32)
    mx[:, :cols], my[:, :cols] = maps["map_x"], maps["map_y"]
    val = np.full((rows, cols), 0x5A, np.uint8) if optional else None
    rc = _lib.lib().bicos_rectify_host(h, src, n, s.shape[1], s.shape[2],
                                       wide.shape[2] * s.itemsize, s.itemsize, ptr(mx), ptr(my),
                                       (cols + 2) * 4, rows, cols, dst, out.shape[2] * s.itemsize,
                                       3, ptr(val))
    _lib.check(rc, "bicos_rectify_host")
    assert (out[:, :, cols:] == 9).all(), "bicos_rectify_host wrote between the output rows"
    res = dict(out=np.ascontiguousarray(out[:, :, :cols]))
    if optional:
        res["valid"] = val
    return res


# --------------------------------------------------------------- pyramid match
@functools.lru_cache(maxsize=None)
def pyramid_inputs(kind, flavour):
    L, R = stereo_stack(*PYRAMID_SHAPE[kind], np.uint8)
    return L, R, (None if flavour == "i16" else 0.9)


def pyramid_device(gpu, L, R, thr, optional=True):
    import torch
    from libbicos_amd.device import MatchConfig
    cfg = MatchConfig(disparity_range=WINDOW, nxcorr_threshold=thr)
    if not optional:
        d, _ = gpu.match_pyramid(to_dev(L), to_dev(R), cfg, scale=2, want_corrmap=False)
        return dict(disparity=to_host(d))
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    d, c, guide, coarse = gpu.match_pyramid(to_dev(L), to_dev(R), cfg, scale=2, return_guide=True,
                                            return_coarse=True, counts=cnt)
    res = dict(disparity=to_host(d), coarse=to_host(coarse), guide=to_host(guide),
               counts=to_host(cnt))
    if c is not None:
        res["corrmap"] = to_host(c)
    return res


def pyramid_host(h, L, R, thr, optional=True):
    from libbicos_amd.device import MatchConfig
    n, rows, cols = L.shape
    c, has_nxcorr = MatchConfig(disparity_range=WINDOW, nxcorr_threshold=thr).to_c()
    rng, sc, r, sp, flo, fhi = _lib.pyramid_params(WINDOW, 2)
    dt = np.float32 if has_nxcorr else np.int16
    d = marked((rows, cols), dt)
    corr = marked((rows, cols), np.float32) if optional and has_nxcorr else None
    coarse = marked((rows // sc, cols // sc), dt) if optional else None
    guide = marked((rows, cols, 2), np.int16) if optional else None
    cnt = marked(2, np.uint32) if optional else None
    p0 = (ctypes.c_void_p * n)(*[L[t].ctypes.data for t in range(n)])
    p1 = (ctypes.c_void_p * n)(*[R[t].ctypes.data for t in range(n)])
    rc = _lib.lib().bicos_match_host_pyramid(h, p0, p1, n, rows, cols, cols * L.itemsize,
                                             L.itemsize, ctypes.byref(c), has_nxcorr, rng[0],
                                             rng[1], sc, r, sp, flo, fhi, ptr(d), ptr(corr),
                                             ptr(coarse), ptr(guide), ptr(cnt))
    _lib.check(rc, "bicos_match_host_pyramid")
    if not optional:
        return dict(disparity=d)
    res = dict(disparity=d, coarse=coarse, guide=guide, counts=cnt)
    if corr is not None:
        res["corrmap"] = corr
    return res


# ------------------------------------------------------------------ the rounds
def capacities(full):
    """the capacity of the second of the three runs (full, half, none): half of what the full
    run kept"""
    kept = int(full["counts"].view(np.uint32)[0])
    assert kept > 1
    return kept // 2


@functools.lru_cache(maxsize=None)
def reference(gpu, kind, flavour):
    """every stage's *_device entry on this round's inputs, computed once and shared"""
    want = {}
    want["median"] = median_device(gpu, median_inputs(kind, flavour))
    want["median-bare"] = median_device(gpu, median_inputs(kind, flavour), optional=False)
    d = mesh_inputs(kind, flavour)
    tcap = 2 * _lib.mesh_quads(*d.shape)
    full = want["mesh-full"] = mesh_device(gpu, d, d.size, tcap)
    half = (int(full["counts"].view(np.uint32)[0]) // 2, int(full["counts"].view(np.uint32)[4]) // 2)
    assert half[0] > 0 and half[1] > 0, "the map must keep vertices and emit triangles"
    want["mesh-half"] = mesh_device(gpu, d, *half)
    want["mesh-none"] = mesh_device(gpu, d, 0, 0)
    want["mesh-bare"] = mesh_device(gpu, d, d.size, tcap, optional=False)
    want["pool"] = pool_device(gpu, *pool_inputs(kind, flavour))
    d = reproject_inputs(kind, flavour)
    full = want["reproject-full"] = reproject_device(gpu, d, d.size)
    want["reproject-half"] = reproject_device(gpu, d, capacities(full))
    want["reproject-none"] = reproject_device(gpu, d, 0)
    want["reproject-bare"] = reproject_device(gpu, d, d.size, optional=False)
    want["reproject-map"] = reproject_device(gpu, d, None)
    s, rows, cols = rectify_inputs(kind, flavour)
    want["rectify_maps"] = rectify_maps_device(gpu, s, rows, cols)
    want["rectify"] = rectify_device(gpu, s, want["rectify_maps"])
    want["rectify-bare"] = rectify_device(gpu, s, want["rectify_maps"], optional=False)
    want["speckle"] = speckle_device(gpu, speckle_inputs(kind, flavour))
    want["speckle-bare"] = speckle_device(gpu, speckle_inputs(kind, flavour), optional=False)
    d, index = normals_inputs(kind, flavour)
    want["normals"] = normals_device(gpu, d, index)
    want["normals-list"] = normals_device(gpu, d, index, optional=False)
    want["normals-map"] = normals_map_device(gpu, d)
    want["guide"] = guide_device(gpu, *guide_inputs(kind, flavour))
    want["guide-bare"] = guide_device(gpu, *guide_inputs(kind, flavour), optional=False)
    want["pyramid"] = pyramid_device(gpu, *pyramid_inputs(kind, flavour))
    want["pyramid-bare"] = pyramid_device(gpu, *pyramid_inputs(kind, flavour), optional=False)
    return want


def host_round(h, kind, flavour, want):
    """the ten host entries one after the other, each laying the staging out differently from
    the one before: median -> mesh -> pool -> reproject -> rectify_maps -> rectify -> speckle ->
    normals -> guide -> pyramid match, then the same order once more for the other variants"""
    got = {}
    mesh_d, repr_d = mesh_inputs(kind, flavour), reproject_inputs(kind, flavour)
    tcap = 2 * _lib.mesh_quads(*mesh_d.shape)
    mesh_counts = want["mesh-full"]["counts"].view(np.uint32)
    half = (int(mesh_counts[0]) // 2, int(mesh_counts[4]) // 2)
    s, rows, cols = rectify_inputs(kind, flavour)
    nd, nindex = normals_inputs(kind, flavour)

    got["median"] = median_host(h, median_inputs(kind, flavour))
    got["mesh-full"] = mesh_host(h, mesh_d, mesh_d.size, tcap)
    got["pool"] = pool_host(h, *pool_inputs(kind, flavour))
    got["reproject-full"] = reproject_host(h, repr_d, repr_d.size)
    got["rectify_maps"] = rectify_maps_host(s, rows, cols)
    got["rectify"] = rectify_host(h, s, want["rectify_maps"])
    got["speckle"] = speckle_host(h, speckle_inputs(kind, flavour))
    got["normals"] = normals_host(h, nd, nindex)
    got["guide"] = guide_host(h, *guide_inputs(kind, flavour))
    got["pyramid"] = pyramid_host(h, *pyramid_inputs(kind, flavour))
    # ... the optional outputs left out, and the smaller capacities
    got["median-bare"] = median_host(h, median_inputs(kind, flavour), optional=False)
    got["mesh-half"] = mesh_host(h, mesh_d, *half)
    got["reproject-half"] = reproject_host(h, repr_d, capacities(want["reproject-full"]))
    got["rectify-bare"] = rectify_host(h, s, want["rectify_maps"], optional=False)
    got["speckle-bare"] = speckle_host(h, speckle_inputs(kind, flavour), optional=False)
    got["normals-list"] = normals_host(h, nd, nindex, optional=False)
    got["guide-bare"] = guide_host(h, *guide_inputs(kind, flavour), optional=False)
    got["pyramid-bare"] = pyramid_host(h, *pyramid_inputs(kind, flavour), optional=False)
    got["mesh-none"] = mesh_host(h, mesh_d, 0, 0)
    got["reproject-none"] = reproject_host(h, repr_d, 0)
    got["normals-map"] = normals_map_host(h, nd)
    got["mesh-bare"] = mesh_host(h, mesh_d, mesh_d.size, tcap, optional=False)
    got["reproject-bare"] = reproject_host(h, repr_d, repr_d.size, optional=False)
    got["reproject-map"] = reproject_host(h, repr_d, None)
    return got


@pytest.mark.parametrize("engine", ["created", "default"])
def test_host_entries_interleaved_equal_the_device_entries(gpu, engine):
    h = gpu._h if engine == "created" else None
    rounds = []
    for kind in ROUNDS:
        for flavour in FLAVOURS:
            want = reference(gpu, kind, flavour)
            got = host_round(h, kind, flavour, want)
            assert set(got) == set(want)
            for stage in want:
                same(got[stage], want[stage], (engine, kind, flavour, stage))
            rounds.append(got)
    # the first shapes again after the staging grew: the first round's bytes
    per = len(FLAVOURS)
    for first, third in zip(rounds[:per], rounds[2 * per:]):
        for stage in first:
            same(third[stage], first[stage], (engine, "third round", stage))


def test_the_rounds_are_what_they_are_for(gpu):
    """the larger shapes span more than one tile in both directions, the smaller ones less than
    one; the capacity runs cut something off; the maps hold invalid pixels"""
    for tile in (_lib.median_tile(), _lib.speckle_tile(), _lib.normals_tile(), _lib.rectify_tile(),
                 _lib.pool_tile()):
        (sr, sc), (lr, lc) = shape(tile, "small"), shape(tile, "large")
        assert sr < tile[0] and sc < tile[1]
        assert tile[0] < lr <= 2 * tile[0] and tile[1] < lc <= 2 * tile[1]
    for kind in ("small", "large"):
        for flavour in FLAVOURS:
            want = reference(gpu, kind, flavour)
            kept = int(want["reproject-full"]["counts"].view(np.uint32)[0])
            invalid = int(want["reproject-full"]["counts"].view(np.uint32)[1])
            assert invalid > 0 and kept > 0
            assert len(want["reproject-half"]["points"]) == kept // 2 < kept
            assert len(want["reproject-none"]["points"]) == 0
            assert int(want["reproject-none"]["counts"].view(np.uint32)[0]) == kept
            tris = int(want["mesh-full"]["counts"].view(np.uint32)[4])
            assert len(want["mesh-half"]["triangles"]) == tris // 2 < tris
            assert len(want["mesh-none"]["triangles"]) == 0 == len(want["mesh-none"]["points"])
