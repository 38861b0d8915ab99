"""The mesh on the GPU (libbicos_amd/csrc/mesh.hip; include/bicos_c.h, "mesh") against the numpy
restatement of tests/mesh_ref.py, which tests/test_mesh_api.py checks against a plain loop and
hand-worked maps. Every comparison is exact: np.array_equal on the int32 outputs and uint32 views
of the points. Every output buffer is filled with a guard before the call, and nothing past the
written ranges may change.
"""
import ctypes

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import mesh_ref as ref
from tests.test_cli import Q

pytestmark = pytest.mark.gpu

GUARD = -12345.0  # float outputs
IGUARD = -7       # int32 outputs
F32S = ref.F32_SENTINEL
INF = float("inf")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def segment():
    return _lib.lib().bicos_reproject_segment()


def run(handle, d, flags, max_diff=1.0, with_index=True, with_vertex_map=True, vcap=None,
        tcap=None, stream=None):
    """bicos_mesh_device on a numpy map -> dict of numpy results. The buffers hold every pixel
    and every possible triangle, all guards before the call; vcap / tcap are what the call is
    told."""
    import torch
    L = _lib.lib()
    rows, cols = d.shape
    n = max(rows * cols, 1)
    m = max(2 * _lib.mesh_quads(rows, cols), 1)
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(np.array(d)).to(dev) if d.size else None  # (a writable copy)
    pts = torch.full((n, 3), GUARD, dtype=torch.float32, device=dev)
    idx = torch.full((n,), IGUARD, dtype=torch.int32, device=dev) if with_index else None
    tri = torch.full((m, 3), IGUARD, dtype=torch.int32, device=dev)
    vmap = torch.full((n,), IGUARD, dtype=torch.int32, device=dev) if with_vertex_map else None
    cnt = torch.full((4,), -1, dtype=torch.int32, device=dev)
    mcnt = torch.full((4,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    ptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
    rc = L.bicos_mesh_device(
        handle, ptr(t), _lib.CV_32F if d.dtype == np.float32 else _lib.CV_16S, rows, cols,
        _lib.reproject_q(Q), flags, max_diff, ptr(pts), ptr(idx),
        rows * cols if vcap is None else vcap, ptr(cnt), ptr(tri),
        2 * _lib.mesh_quads(rows, cols) if tcap is None else tcap, ptr(mcnt), ptr(vmap),
        s.cuda_stream)
    _lib.check(rc, "bicos_mesh_device")
    s.synchronize()
    out = dict(points=pts.cpu().numpy(), triangles=tri.cpu().numpy(),
               counts=cnt.cpu().numpy().view(np.uint32),
               mesh_counts=mcnt.cpu().numpy().view(np.uint32))
    if with_index:
        out["index"] = idx.cpu().numpy()
    if with_vertex_map:
        out["vertex_map"] = vmap.cpu().numpy()
    return out


def check(got, want, vcap=None, tcap=None):
    """every output present in `got` against the restatement `want`"""
    kept, tris = int(want["counts"][0]), int(want["mesh_counts"][0])
    nv = kept if vcap is None else min(kept, vcap)
    nt = tris if tcap is None else min(tris, tcap)
    assert got["counts"].tolist() == want["counts"].tolist()
    assert got["mesh_counts"].tolist() == want["mesh_counts"].tolist()
    assert np.array_equal(bits(got["points"][:nv]), bits(want["points"][:nv]))
    assert (got["points"][nv:] == GUARD).all()  # nothing past the list (or the capacity)
    assert np.array_equal(got["triangles"][:nt], want["triangles"][:nt])
    assert (got["triangles"][nt:] == IGUARD).all()
    if "index" in got:
        assert np.array_equal(got["index"][:nv], want["index"][:nv])
        assert (got["index"][nv:] == IGUARD).all()
    if "vertex_map" in got:
        n = want["vertex_map"].size
        assert np.array_equal(got["vertex_map"][:n], want["vertex_map"].ravel())
        assert (got["vertex_map"][n:] == IGUARD).all()


def shapes():
    seg = segment()
    return [(2, 2), (3, 65), (7, 257), (2, seg), (2, seg + 1), (3, seg - 1), (64, 2049),
            (1536, 2048)]


# ------------------------------------------------------------- shapes and types
@pytest.mark.parametrize("dtype,flags", [("int16", 0), ("float32", F32S)])
@pytest.mark.parametrize("shape_at", range(8))
def test_shapes(gpu, shape_at, dtype, flags):
    """the smallest map, odd maps, the quads whose lower row lies in another segment, a row that
    is a multiple of nothing, and a map with more segments than the scan has threads"""
    rows, cols = shapes()[shape_at]
    d, want = ref.case(rows, cols, dtype, flags)
    ref.conditions(want, rows, cols)
    if (rows, cols) == (1536, 2048):
        assert -(-d.size // segment()) > 1024
    check(run(gpu._h, d, flags), want)


# ------------------------------------------------------------------ parameters
@pytest.mark.parametrize("dtype,flags", [("int16", 0), ("float32", F32S)])
@pytest.mark.parametrize("max_diff", [0.0, 0.5, 1.0, INF])
def test_max_diff(gpu, max_diff, dtype, flags):
    d, want = ref.case(7, 257, dtype, flags, max_diff)
    if max_diff == 1.0:
        ref.conditions(want, 7, 257)
    assert want["mesh_counts"][0] > 0
    check(run(gpu._h, d, flags, max_diff), want)


def test_max_diff_orders_the_triangle_counts():
    """(what the four values of test_max_diff exercise: each links strictly more)"""
    n = [int(ref.case(7, 257, "float32", F32S, m)[1]["mesh_counts"][0]) for m in (0.0, 0.5, 1.0, INF)]
    assert 0 < n[0] < n[1] < n[2] < n[3]


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_float_maps_under_every_flag_combination(gpu, flags):
    d, want = ref.case(7, 257, "float32", flags)
    assert (d == np.float32(-32768.0)).sum() > 0 and np.isnan(d).sum() > 0
    assert want["mesh_counts"][0] > 0
    # without the sentinel flag -32768.0 is a number far behind the camera: kept only with
    # allow_negative_z
    assert (want["counts"][3] > 0) == (flags == 0)
    check(run(gpu._h, d, flags), want)


# ------------------------------------------------------------- degenerate maps
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_all_invalid(gpu, dtype):
    d = np.full((3, segment() + 5), -32768 if dtype == "int16" else np.nan, dtype)
    want = ref.restate(d, Q, 0, 1.0)
    quads = 2 * (segment() + 4)
    assert want["counts"].tolist() == [0, d.size, 0, 0]
    assert want["mesh_counts"].tolist() == [0, 0, 0, quads]
    check(run(gpu._h, d, 0), want)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_all_kept_and_flat(gpu, dtype):
    """every quad ties, takes AD and gives two triangles"""
    cols = segment() + 5
    d = np.full((3, cols), 30, dtype)
    want = ref.restate(d, Q, 0, 0.0)
    quads = 2 * (cols - 1)
    assert want["counts"].tolist() == [d.size, 0, 0, 0]
    assert want["mesh_counts"].tolist() == [2 * quads, quads, 0, 0]
    assert want["cases"]["ad"] == quads
    assert want["triangles"][:2].tolist() == [[0, cols, cols + 1], [0, cols + 1, 1]]
    check(run(gpu._h, d, 0, 0.0), want)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_single_kept_pixel(gpu, dtype):
    d = np.full((3, segment() + 5), -32768 if dtype == "int16" else np.nan, dtype)
    d[1, -2] = 30
    want = ref.restate(d, Q, 0, 1.0)
    assert want["counts"].tolist() == [1, d.size - 1, 0, 0]
    assert want["mesh_counts"][0] == 0 and (want["vertex_map"] >= 0).sum() == 1
    check(run(gpu._h, d, 0), want)


@pytest.mark.parametrize("shape", ["row", "column"])
def test_one_row_and_one_column(gpu, shape):
    """vertices and no triangles"""
    n = segment() + 3
    rows, cols = (1, n) if shape == "row" else (n, 1)
    d, want = ref.case(rows, cols, "float32", F32S)
    assert want["counts"][0] > 0.5 * n
    assert want["mesh_counts"].tolist() == [0, 0, 0, 0]
    check(run(gpu._h, d, F32S), want)


@pytest.mark.parametrize("rows,cols", [(0, 5), (5, 0), (0, 0)])
def test_empty_maps(gpu, rows, cols):
    got = run(gpu._h, np.zeros((rows, cols), np.int16), 0)
    assert got["counts"].tolist() == [0, 0, 0, 0] and got["mesh_counts"].tolist() == [0, 0, 0, 0]
    assert (got["points"] == GUARD).all() and (got["triangles"] == IGUARD).all()
    assert (got["index"] == IGUARD).all() and (got["vertex_map"] == IGUARD).all()
    counts, mcounts = (ctypes.c_uint32 * 4)(9, 9, 9, 9), (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    pts = np.full((1, 3), GUARD, np.float32)
    tri = np.full((1, 3), IGUARD, np.int32)
    rc = _lib.lib().bicos_mesh_host(None, None, _lib.CV_16S, rows, cols, _lib.reproject_q(Q), 0,
                                    1.0, pts.ctypes.data, None, 1, counts, tri.ctypes.data, 1,
                                    mcounts, None)
    assert rc == 0 and list(counts) == [0, 0, 0, 0] and list(mcounts) == [0, 0, 0, 0]
    assert (pts == GUARD).all() and (tri == IGUARD).all()


# ------------------------------------------------------------------ capacities
@pytest.mark.parametrize("tcap", [0, 1, 700])
def test_triangle_capacity_below_the_count(gpu, tcap):
    """the first tcap triangles, guards past them in the same allocation, the full count"""
    d, want = ref.case(7, 257, "float32", F32S)
    assert want["mesh_counts"][0] > tcap
    got = run(gpu._h, d, F32S, tcap=tcap)
    assert got["mesh_counts"][0] == want["mesh_counts"][0]
    check(got, want, tcap=tcap)


@pytest.mark.parametrize("vcap", [0, 1, 700])
def test_vertex_capacity_below_kept(gpu, vcap):
    """the first vcap points; the triangles and the vertex map are still those of the full
    numbering"""
    d, want = ref.case(7, 257, "float32", F32S)
    assert want["counts"][0] > vcap and want["triangles"].max() >= vcap
    got = run(gpu._h, d, F32S, vcap=vcap)
    assert got["counts"][0] == want["counts"][0]
    check(got, want, vcap=vcap)


# ------------------------------------------------------------------ vertex_map
@pytest.mark.parametrize("dtype,flags", [("int16", 0), ("float32", F32S)])
def test_vertex_map_given_and_not_given(gpu, dtype, flags):
    seg = segment()
    d, want = ref.case(3, seg - 1, dtype, flags)
    ref.conditions(want, 3, seg - 1)
    a = run(gpu._h, d, flags, with_vertex_map=True)
    b = run(gpu._h, d, flags, with_vertex_map=False, with_index=False)
    check(a, want)
    check(b, want)
    assert a["triangles"].tobytes() == b["triangles"].tobytes()
    # the inverse of the index
    kept = int(a["counts"][0])
    vm = a["vertex_map"][:d.size]
    assert np.array_equal(vm[a["index"][:kept]], np.arange(kept))
    assert (vm >= 0).sum() == kept and vm.min() == -1


def test_same_call_twice_gives_the_same_bytes(gpu):
    d, want = ref.case(64, 2049, "float32", F32S)
    ref.conditions(want, 64, 2049)
    a = run(gpu._h, d, F32S)
    b = run(gpu._h, d, F32S)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# --------------------------------------------------------------------- host entry
@pytest.mark.parametrize("dtype,flags", [("int16", 0), ("float32", F32S)])
def test_host_entry(gpu, dtype, flags):
    """host buffers with guards, capacities below the counts, with and without vertex_map"""
    L = _lib.lib()
    rows, cols = 3, segment() + 1
    d, want = ref.case(rows, cols, dtype, flags)
    ref.conditions(want, rows, cols)
    for vcap, tcap, with_map in ((d.size, 4 * (cols - 1), True), (500, 900, False)):
        pts = np.full((d.size, 3), GUARD, np.float32)
        idx = np.full(d.size, IGUARD, np.int32)
        tri = np.full((4 * (cols - 1), 3), IGUARD, np.int32)
        vmap = np.full(d.size + 8, IGUARD, np.int32)
        counts, mcounts = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 4)()
        rc = L.bicos_mesh_host(None, d.ctypes.data, _lib.CV_32F if dtype == "float32" else _lib.CV_16S,
                               rows, cols, _lib.reproject_q(Q), flags, 1.0, pts.ctypes.data,
                               idx.ctypes.data, vcap, counts, tri.ctypes.data, tcap, mcounts,
                               vmap.ctypes.data if with_map else None)
        _lib.check(rc, "bicos_mesh_host")
        got = dict(points=pts, index=idx, triangles=tri, counts=np.array(list(counts), np.uint32),
                   mesh_counts=np.array(list(mcounts), np.uint32))
        if with_map:
            got["vertex_map"] = vmap
        else:
            assert (vmap == IGUARD).all()
        assert want["counts"][0] > 500 and want["mesh_counts"][0] > 900
        check(got, want, vcap=vcap, tcap=tcap)


# ------------------------------------------------------------- engine reuse
def test_engine_reuse_across_streams_and_a_growing_workspace(oracle):
    """one engine: a mesh, then a match (whose workspace is far larger), then a mesh of a larger
    map, on two streams -- the Lease orders them on the shared workspace and the workspace grows
    between uses"""
    import torch
    from libbicos_amd import device
    from libbicos_amd.synthetic import stereo_stack
    eng = device.Engine(0)
    small, want_small = ref.case(7, 257, "int16", 0)
    large, want_large = ref.case(1536, 2048, "float32", F32S)
    L, R = stereo_stack(12, 40, 200)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    ts, tg = torch.from_numpy(small.copy()).cuda(), torch.from_numpy(large.copy()).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    r1 = eng.mesh(ts, Q, sentinel=False, with_index=True, stream=s1)
    disp, _ = eng.match(tl, tr, device.MatchConfig(nxcorr_threshold=0.75), stream=s2)
    r2 = eng.mesh(tg, Q, with_index=True, with_vertex_map=True, stream=s2)
    r3 = eng.mesh(ts, Q, sentinel=False, stream=s1)
    torch.cuda.synchronize()
    rd, _ = oracle.match(L, R, oracle.OracleConfig(nxcorr_threshold=0.75))
    assert np.array_equal(bits(disp.cpu().numpy()), bits(rd))
    for (p, t, i, vm, st), want in ((r1, want_small), (r2, want_large), (r3, want_small)):
        assert [st[k] for k in ref.KEYS] == want["counts"].tolist() + want["mesh_counts"].tolist()
        assert np.array_equal(bits(p.cpu().numpy()), bits(want["points"]))
        assert np.array_equal(t.cpu().numpy(), want["triangles"])
        if i is not None:
            assert np.array_equal(i.cpu().numpy(), want["index"])
        if vm is not None:
            assert np.array_equal(vm.cpu().numpy(), want["vertex_map"])
    assert r3[2] is None and r3[3] is None and r1[3] is None
    eng.close()


# ----------------------------------------------------- from a real match, every API
@pytest.mark.parametrize("cfg", [dict(nxcorr_threshold=0.75),
                                 dict(nxcorr_threshold=0.75, subpixel_step=0.2),
                                 dict(nxcorr_threshold=None)],
                         ids=["nxc_sentinel", "subpixel_nan", "int16"])
def test_end_to_end_from_a_match(gpu, cfg):
    import torch
    from libbicos_amd import device, pybicos
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(12, 40, 200)
    disp, _ = gpu.match(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(),
                        device.MatchConfig(**cfg))
    d = disp.cpu().numpy()
    want = ref.restate(d, Q, F32S, 1.0)  # Python's defaults
    quads = 39 * 199
    assert want["mesh_counts"][0] > quads
    pts, tri, idx, vmap, stats = gpu.mesh(disp, Q, with_index=True, with_vertex_map=True)
    assert [stats[k] for k in ref.KEYS] == want["counts"].tolist() + want["mesh_counts"].tolist()
    assert np.array_equal(bits(pts.cpu().numpy()), bits(want["points"]))
    assert tri.dtype == torch.int32 and np.array_equal(tri.cpu().numpy(), want["triangles"])
    assert np.array_equal(idx.cpu().numpy(), want["index"])
    assert np.array_equal(vmap.cpu().numpy(), want["vertex_map"])
    # the vertices are reproject_points' list
    p2, i2, st2 = gpu.reproject_points(disp, Q, with_index=True)
    assert torch.equal(p2.view(torch.int32), pts.view(torch.int32)) and torch.equal(i2, idx)
    assert all(st2[k] == stats[k] for k in st2)
    # one normal per vertex: the rows of the dense map at index
    sentinel = d.dtype == np.float32
    nrm = gpu.normals_points(disp, Q, idx, sentinel=sentinel)
    dense = gpu.normals_map(disp, Q, sentinel=sentinel)
    assert nrm.shape == (pts.shape[0], 3)
    assert torch.equal(nrm.view(torch.int32),
                       dense.reshape(-1, 3)[idx.long()].view(torch.int32))
    # out_* with a capacity: enough, then too small
    op = torch.empty((stats["kept"], 3), dtype=torch.float32, device=disp.device)
    ot = torch.empty((stats["triangles"], 3), dtype=torch.int32, device=disp.device)
    p3, t3, i3, v3, _ = gpu.mesh(disp, Q, out_points=op, out_triangles=ot)
    assert i3 is None and v3 is None
    assert p3.data_ptr() == op.data_ptr() and t3.data_ptr() == ot.data_ptr()
    assert np.array_equal(t3.cpu().numpy(), want["triangles"])
    with pytest.raises(RuntimeError, match="were kept"):
        gpu.mesh(disp, Q, out_points=op[:10])
    with pytest.raises(RuntimeError, match="were emitted"):
        gpu.mesh(disp, Q, out_triangles=ot[:10])
    with pytest.raises(ValueError):
        gpu.mesh(disp, Q, out_triangles=torch.empty((40, 3), device=disp.device))
    with pytest.raises(ValueError):
        gpu.mesh(disp, Q, max_diff=-1.0)
    with pytest.raises(ValueError):
        gpu.mesh(disp.double(), Q)
    # host buffers
    hp, ht = pybicos.mesh(d, Q)
    assert hp.dtype == np.float32 and np.array_equal(bits(hp), bits(want["points"]))
    assert ht.dtype == np.int32 and np.array_equal(ht, want["triangles"])
    loose = ref.restate(d, Q, ref.ALLOW_NEGATIVE_Z, 2.0)
    hp, ht = pybicos.mesh(d, Q, max_diff=2.0, allow_negative_z=True, sentinel=False)
    assert np.array_equal(bits(hp), bits(loose["points"])) and np.array_equal(ht, loose["triangles"])
