"""The mesh interface without a GPU (include/bicos_c.h, "mesh"): the C-ABI symbols and their
argument checks (BICOS_E_ARG before any HIP call), the Python plumbing, the .ply writer of the
command-line tool, and a self-check of the numpy restatement (tests/mesh_ref.py) that the GPU
tests compare the kernels against: it must equal a plain double loop over the quads, give the
hand-worked answers on small maps, and have the structure the definition promises.
"""
import ctypes
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import mesh_ref as ref
from tests.test_cli import Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLY_CHECK = os.path.join(ROOT, "tests", "cpp", "ply_check")
SYMBOLS = ("bicos_mesh_device", "bicos_mesh_host", "bicos_mesh_segment")
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------- the restatement, checked
def loop_mesh(d, q, flags, max_diff):
    """the definition, quad by quad, in plain Python -> (triangles, mesh_counts)"""
    v = ref.restate_points(d, q, flags)
    rows, cols = d.shape
    rank = np.full(d.size, -1, np.int64)
    rank[v["index"]] = np.arange(len(v["index"]))
    rank = rank.reshape(rows, cols)
    md = np.float32(max_diff)

    def link(p, s):
        return bool(np.abs(np.float32(d[p]) - np.float32(d[s])) <= md)

    tris, n2, n1, n0 = [], 0, 0, 0
    for r in range(rows - 1):
        for c in range(cols - 1):
            A, B, C, D = (r, c), (r, c + 1), (r + 1, c), (r + 1, c + 1)
            have = [p for p in (A, B, C, D) if rank[p] >= 0]
            cand = []
            if len(have) == 4:
                ad = np.abs(np.float32(d[A]) - np.float32(d[D]))
                bc = np.abs(np.float32(d[B]) - np.float32(d[C]))
                cand = [(A, C, D), (A, D, B)] if ad <= bc else [(A, C, B), (B, C, D)]
            elif len(have) == 3:
                if D not in have:
                    cand = [(A, C, B)]
                elif A not in have:
                    cand = [(B, C, D)]
                elif B not in have:
                    cand = [(A, C, D)]
                else:
                    cand = [(A, D, B)]
            out = [t for t in cand
                   if link(t[0], t[1]) and link(t[1], t[2]) and link(t[2], t[0])]
            tris += [[int(rank[p]) for p in t] for t in out]
            n2, n1, n0 = n2 + (len(out) == 2), n1 + (len(out) == 1), n0 + (len(out) == 0)
    return np.array(tris, np.int32).reshape(-1, 3), [len(tris), n2, n1, n0]


@pytest.mark.parametrize("max_diff", [0.0, 1.0, INF])
@pytest.mark.parametrize("dtype,flags", [("int16", 0), ("float32", ref.F32_SENTINEL)])
def test_restatement_is_the_double_loop(dtype, flags, max_diff):
    d, _ = ref.case(7, 257, dtype, flags)
    want = ref.restate(d, Q, flags, max_diff)
    tris, counts = loop_mesh(d, Q, flags, max_diff)
    assert counts[0] > 0
    assert want["mesh_counts"].tolist() == counts
    assert np.array_equal(want["triangles"], tris)


def test_the_issue_s_figures_for_the_test_map():
    _, w = ref.case(3, 65, "float32", ref.F32_SENTINEL)
    assert w["mesh_counts"].tolist() == [217, 92, 33, 3]
    assert w["cases"] == dict(ad=43, bc=53, missing=[4, 5, 12, 10])
    _, w = ref.case(7, 257, "float32", ref.F32_SENTINEL)
    assert w["mesh_counts"].tolist() == [2492, 1057, 378, 101]
    for shape in ((3, 65), (7, 257)):
        for dtype, flags in (("int16", 0), ("float32", ref.F32_SENTINEL)):
            ref.conditions(ref.case(shape[0], shape[1], dtype, flags)[1], *shape)


def _mesh(rows, max_diff=1.0, dtype=np.float32):
    w = ref.restate(np.array(rows, dtype), Q, 0, max_diff)
    return w["triangles"].tolist(), w["mesh_counts"].tolist()


def test_hand_worked_maps():
    n = NAN
    # 2x2, every corner there and flat: a tie takes AD. Vertices A=0, B=1, C=2, D=3
    assert _mesh([[30, 30], [30, 30]]) == ([[0, 2, 3], [0, 3, 1]], [2, 1, 0, 0])
    # |dA - dD| = 1 > |dB - dC| = 0: BC wins
    assert _mesh([[30, 30.5], [30.5, 31]]) == ([[0, 2, 1], [1, 2, 3]], [2, 1, 0, 0])
    # |dA - dD| = 0 < |dB - dC| = 1: AD
    assert _mesh([[30.5, 30], [31, 30.5]]) == ([[0, 2, 3], [0, 3, 1]], [2, 1, 0, 0])
    # each corner missing in turn; the others are renumbered in row-major order
    assert _mesh([[30, 30], [30, n]]) == ([[0, 2, 1]], [1, 0, 1, 0])   # D: (A, C, B)
    assert _mesh([[n, 30], [30, 30]]) == ([[0, 1, 2]], [1, 0, 1, 0])   # A: (B, C, D)
    assert _mesh([[30, n], [30, 30]]) == ([[0, 1, 2]], [1, 0, 1, 0])   # B: (A, C, D)
    assert _mesh([[30, 30], [n, 30]]) == ([[0, 2, 1]], [1, 0, 1, 0])   # C: (A, D, B)
    assert _mesh([[30, n], [n, 30]]) == ([], [0, 0, 0, 1])
    # int16, the same with -32768
    assert _mesh([[30, 30], [30, -32768]], dtype=np.int16) == ([[0, 2, 1]], [1, 0, 1, 0])
    # 2x3, vertices 0 1 2 / 3 4 5, the last column 2 above the others: the left quad is flat and
    # whole; in the right quad both diagonals step by 2 (a tie: AD), and both of its triangles
    # have an edge of 2, which max_diff = 1 does not link
    assert _mesh([[30, 30, 32], [30, 30, 32]]) == ([[0, 3, 4], [0, 4, 1]], [2, 1, 0, 1])
    # D is 1.5 above the rest: BC is the flatter diagonal, (A, C, B) is whole, (B, C, D) has the
    # broken edges B-D and C-D
    assert _mesh([[30, 30], [30, 31.5]], 1.0) == ([[0, 2, 1]], [1, 0, 1, 0])
    # max_diff = 0 links equal disparities only; inf links everything kept
    assert _mesh([[30, 30], [30, 30.5]], 0.0) == ([[0, 2, 1]], [1, 0, 1, 0])
    assert _mesh([[30, 90], [5, 60]], INF)[1] == [2, 1, 0, 0]
    # one row, one column: vertices and no triangles
    for shape in ((1, 5), (5, 1)):
        w = ref.restate(np.full(shape, 30, np.float32), Q, 0, 1.0)
        assert w["counts"].tolist() == [5, 0, 0, 0]
        assert w["triangles"].shape == (0, 3) and w["mesh_counts"].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("dtype,flags", [("int16", 0), ("float32", ref.F32_SENTINEL)])
@pytest.mark.parametrize("shape", [(3, 65), (7, 257), (64, 2049)])
def test_structure(shape, dtype, flags):
    rows, cols = shape
    d, w = ref.case(rows, cols, dtype, flags)
    ref.conditions(w, rows, cols)
    tri, kept = w["triangles"], int(w["counts"][0])
    assert tri.dtype == np.int32 and tri.min() >= 0 and tri.max() < kept
    # through index, every triangle is one of the four patterns inside one quad
    pix = w["index"][tri]
    r, c = pix // cols, pix % cols
    r0, c0 = r.min(axis=1), c.min(axis=1)
    rel = np.stack([r - r0[:, None], c - c0[:, None]], -1)  # [T, 3, (row, col)]
    A, B, C, D = (0, 0), (0, 1), (1, 0), (1, 1)
    patterns = [(A, C, D), (A, D, B), (A, C, B), (B, C, D)]
    hit = np.zeros(len(tri), bool)
    for p in patterns:
        hit |= (rel == np.array(p)).all(axis=(1, 2))
    assert hit.all()
    # (B, C, D) has no corner at A, so its bounding box starts at the quad's origin all the same
    assert (r0 < rows - 1).all() and (c0 < cols - 1).all()
    # no triangle twice, and with x right and y down every one turns the same way
    assert len(np.unique(tri, axis=0)) == len(tri)
    e1, e2 = rel[:, 1] - rel[:, 0], rel[:, 2] - rel[:, 0]
    assert ((e1[:, 1] * e2[:, 0] - e1[:, 0] * e2[:, 1]) < 0).all()  # (x1*y2 - y1*x2)
    # quads in row-major order
    quad = r0 * cols + c0
    assert (np.diff(quad) >= 0).all()
    t, q2, q1, q0 = (int(v) for v in w["mesh_counts"])
    assert t == len(tri) == 2 * q2 + q1 and q2 + q1 + q0 == (rows - 1) * (cols - 1)
    # the vertex map is the inverse of the index
    vm = w["vertex_map"].ravel()
    assert np.array_equal(vm[w["index"]], np.arange(kept)) and (vm >= 0).sum() == kept


# --------------------------------------------------------------------- C-ABI
def test_mesh_symbols_are_exported_and_declared(blib):
    header = open(os.path.join(_lib._HERE, "..", "include", "bicos_c.h")).read()
    for s in SYMBOLS:
        assert hasattr(blib, s), s
        assert s in _lib.EXPORTS, s
        assert ("int %s(" % s) in header, s
    assert len(blib.bicos_mesh_device.argtypes) == 17
    assert len(blib.bicos_mesh_host.argtypes) == 16
    for fn in (blib.bicos_mesh_device, blib.bicos_mesh_host):
        assert fn.argtypes[7] is ctypes.c_float
        assert fn.argtypes[10] is ctypes.c_size_t and fn.argtypes[13] is ctypes.c_size_t
    assert "#define BICOS_MESH_ALLOW_NEGATIVE_Z 1" in header
    assert "#define BICOS_MESH_F32_SENTINEL 2" in header
    assert (_lib.MESH_ALLOW_NEGATIVE_Z, _lib.MESH_F32_SENTINEL) == (1, 2)
    assert "mesh */" in header and "a tie takes AD" in header
    assert blib.bicos_mesh_segment() == blib.bicos_reproject_segment()


_BUF = (ctypes.c_uint32 * 2048)()
_P = ctypes.addressof(_BUF)  # never dereferenced: every case fails before any HIP call
_PTS = _P + 1024             # 4 x 8 points of 12 bytes
_IDX = _P + 2048             # 32 indices
_CNT = _P + 2560             # counts
_TRI = _P + 3072             # 2 * 3 * 7 triangles of 12 bytes
_MC = _P + 4096              # mesh_counts
_VM = _P + 4608              # 4 x 8 ranks
_E = 0x1000                  # a non-NULL "engine", never dereferenced either
_Q = (ctypes.c_double * 16)(*Q.ravel().tolist())
NAMES = ("typ", "rows", "cols", "Q", "flags", "max_diff", "map", "points", "index", "vcap",
         "counts", "triangles", "tcap", "mesh_counts", "vertex_map")
OK = (5, 4, 8, _Q, 0, 1.0, _P, _PTS, _IDX, 32, _CNT, _TRI, 42, _MC, _VM)


def _case(**kw):
    assert set(kw) <= set(NAMES)
    return tuple(kw.get(n, v) for n, v in zip(NAMES, OK))


ARG_ERRORS = [
    ("bad_type", _case(typ=0), "CV_16S"),
    ("f64_type", _case(typ=6), "CV_16S"),
    ("unknown_flags", _case(flags=4), "flag"),
    ("max_diff_negative", _case(max_diff=-0.5), "max_diff"),
    ("max_diff_nan", _case(max_diff=NAN), "max_diff"),
    ("negative_rows", _case(rows=-1), "negative image size"),
    ("negative_cols", _case(cols=-8), "negative image size"),
    ("too_many_pixels", _case(rows=65536, cols=32768), "int32"),
    ("null_map", _case(map=None), "null disparity"),
    ("null_q", _case(Q=None), "null Q"),
    ("null_points", _case(points=None), "null points"),
    ("null_triangles", _case(triangles=None), "null triangles"),
    ("null_counts", _case(counts=None), "null counts"),
    ("null_mesh_counts", _case(mesh_counts=None), "null mesh_counts"),
    ("points_overlap_map", _case(points=_P + 64), "points overlaps the map"),
    ("points_overlap_map_last_byte", _case(points=_P + 127), "points overlaps the map"),
    ("map_above_triangles", _case(map=_TRI + 500), "triangles overlaps the map"),
    ("index_overlaps_points", _case(index=_PTS + 380), "index overlaps points"),
    ("counts_overlap_map", _case(counts=_P + 124), "counts overlaps the map"),
    ("triangles_overlap_points", _case(triangles=_PTS), "triangles overlaps points"),
    ("mesh_counts_are_counts", _case(mesh_counts=_CNT), "mesh_counts overlaps counts"),
    ("mesh_counts_overlap_counts", _case(mesh_counts=_CNT + 12), "mesh_counts overlaps counts"),
    ("vertex_map_overlaps_map", _case(vertex_map=_P), "vertex_map overlaps the map"),
    ("vertex_map_overlaps_triangles", _case(vertex_map=_TRI + 100), "vertex_map overlaps triangles"),
]


@pytest.mark.parametrize("case", ARG_ERRORS, ids=lambda c: c[0])
def test_mesh_argument_errors(blib, case):
    _, (typ, rows, cols, q, flags, diff, m, pts, idx, vcap, cnt, tri, tcap, mc, vm), word = case
    rc = blib.bicos_mesh_device(_E, m, typ, rows, cols, q, flags, diff, pts, idx, vcap, cnt, tri,
                                tcap, mc, vm, None)
    assert rc == _lib.BICOS_E_ARG
    assert word in blib.bicos_last_error().decode()
    rc = blib.bicos_mesh_host(None, m, typ, rows, cols, q, flags, diff, pts, idx, vcap, cnt, tri,
                              tcap, mc, vm)
    assert rc == _lib.BICOS_E_ARG
    assert word in blib.bicos_last_error().decode()


def test_mesh_on_the_device_needs_an_engine(blib):
    for rows, cols in ((4, 8), (0, 8)):
        args = _case(rows=rows, cols=cols)
        typ, rows, cols, q, flags, diff, m, pts, idx, vcap, cnt, tri, tcap, mc, vm = args
        rc = blib.bicos_mesh_device(None, m, typ, rows, cols, q, flags, diff, pts, idx, vcap, cnt,
                                    tri, tcap, mc, vm, None)
        assert rc == _lib.BICOS_E_ARG and "engine" in blib.bicos_last_error().decode()


def test_legal_edges_pass_the_checks(blib):
    """an empty map with NULL everything is no argument error, and the host entry answers it
    without a GPU: nothing is launched. Buffers that touch without overlapping are legal too: a
    capacity below the buffer shortens what the call may write."""
    counts, mesh_counts = (ctypes.c_uint32 * 4)(9, 9, 9, 9), (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    for rows, cols in ((0, 5), (5, 0), (0, 0)):
        rc = blib.bicos_mesh_host(None, None, 3, rows, cols, None, 3, INF, None, None, 0, counts,
                                  None, 0, mesh_counts, None)
        assert rc == 0, blib.bicos_last_error()
        assert list(counts) == [0, 0, 0, 0] and list(mesh_counts) == [0, 0, 0, 0]
        assert blib.bicos_mesh_host(None, None, 3, rows, cols, None, 0, 0.0, None, None, 0, None,
                                    None, 0, None, None) == 0


# -------------------------------------------------------------------- Python
def test_mesh_parameter_marshalling():
    assert _lib.mesh_max_diff(1) == 1.0 and _lib.mesh_max_diff(np.float32(0)) == 0.0
    assert _lib.mesh_max_diff(INF) == INF
    for bad in (-1, -0.0001, NAN, None, "x"):
        with pytest.raises(ValueError):
            _lib.mesh_max_diff(bad)
    assert _lib.mesh_flags(False, False) == 0 and _lib.mesh_flags(True, True) == 3
    assert _lib.mesh_flags(True, False) == 1 and _lib.mesh_flags(False, True) == 2
    assert [_lib.mesh_quads(r, c) for r, c in ((0, 0), (1, 9), (9, 1), (2, 2), (3, 65))] == \
        [0, 0, 0, 1, 128]


def test_engine_method_and_its_defaults():
    from libbicos_amd import device
    p = inspect.signature(device.Engine.mesh).parameters
    assert list(p) == ["self", "disp", "Q", "max_diff", "allow_negative_z", "sentinel",
                       "with_index", "with_vertex_map", "out_points", "out_triangles", "stream"]
    for k in list(p)[3:]:
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert p["max_diff"].default == 1.0
    assert p["allow_negative_z"].default is False and p["sentinel"].default is True
    assert p["with_index"].default is False and p["with_vertex_map"].default is False
    assert p["out_points"].default is None and p["out_triangles"].default is None
    assert p["stream"].default is None


def test_pybicos_mesh_validates_before_the_gpu(blib):
    import pybicos as alias
    from libbicos_amd import pybicos
    assert alias.mesh is pybicos.mesh
    sig = inspect.signature(pybicos.mesh).parameters
    assert list(sig) == ["disparity", "Q", "max_diff", "allow_negative_z", "sentinel"]
    assert sig["max_diff"].default == 1.0
    assert sig["allow_negative_z"].default is False and sig["sentinel"].default is True
    d = np.zeros((4, 8), np.float32)
    with pytest.raises(ValueError, match="2-D"):
        pybicos.mesh(np.zeros((2, 4, 8), np.float32), Q)
    with pytest.raises(ValueError, match="dtype"):
        pybicos.mesh(np.zeros((4, 8), np.float64), Q)
    with pytest.raises(ValueError, match="4x4"):
        pybicos.mesh(d, np.eye(3))
    with pytest.raises(ValueError, match="max_diff"):
        pybicos.mesh(d, Q, max_diff=-1)
    with pytest.raises(ValueError, match="max_diff"):
        pybicos.mesh(d, Q, max_diff=NAN)
    # an empty map never reaches the GPU
    pts, tri = pybicos.mesh(np.zeros((0, 8), np.int16), Q)
    assert pts.shape == (0, 3) and pts.dtype == np.float32
    assert tri.shape == (0, 3) and tri.dtype == np.int32


# ------------------------------------------------------------- the .ply writer
def ply_bytes(points, triangles):
    """the file of the definition: the header's lines, then the records, with struct"""
    head = ["ply", "format binary_little_endian 1.0", "comment bicos-cli",
            "element vertex %d" % len(points), "property float x", "property float y",
            "property float z", "element face %d" % len(triangles),
            "property list uchar int vertex_indices", "end_header"]
    out = "".join(ln + "\n" for ln in head).encode("ascii")
    out += b"".join(struct.pack("<3f", *(float(v) for v in p)) for p in points)
    out += b"".join(struct.pack("<B3i", 3, *(int(v) for v in t)) for t in triangles)
    return out


def read_ply(path):
    """-> (points float32 [N, 3], triangles int32 [M, 3]) of a file that write_ply wrote"""
    b = open(path, "rb").read()
    end = b.index(b"end_header\n") + len(b"end_header\n")
    lines = b[:end].decode("ascii").split("\n")
    n = int([ln for ln in lines if ln.startswith("element vertex ")][0].split()[2])
    m = int([ln for ln in lines if ln.startswith("element face ")][0].split()[2])
    assert len(b) == end + 12 * n + 13 * m
    pts = np.frombuffer(b, "<f4", 3 * n, end).reshape(n, 3)
    rec = np.frombuffer(b, np.uint8, 13 * m, end + 12 * n).reshape(m, 13)
    assert (rec[:, 0] == 3).all()
    return pts, np.ascontiguousarray(rec[:, 1:]).view("<i4").reshape(m, 3)


def ply_built():
    if not os.path.exists(PLY_CHECK):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "ply.mk"],
                       check=True, capture_output=True)


@pytest.mark.parametrize("vertices,faces", [(5, 0), (0, 0), (300, 517), (3, 5000)],
                         ids=["no_faces", "nothing", "hundreds", "more_than_one_chunk"])
def test_ply_writer(blib, tmp_path, vertices, faces):
    ply_built()  # (links the library: blib has built it)
    rng = np.random.default_rng(vertices + faces)
    pts = (rng.standard_normal((vertices, 3)) * 100).astype(np.float32)
    if vertices:
        pts[0] = [0.0, -0.0, 1e-30]
    tri = rng.integers(0, max(vertices, 1), size=(faces, 3)).astype(np.int32)
    (tmp_path / "p.raw").write_bytes(pts.tobytes())
    (tmp_path / "t.raw").write_bytes(tri.tobytes())
    out = tmp_path / "m.ply"
    r = subprocess.run([PLY_CHECK, str(tmp_path / "p.raw"), str(vertices), str(tmp_path / "t.raw"),
                        str(faces), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == ply_bytes(pts, tri)
    got_p, got_t = read_ply(str(out))
    assert got_p.tobytes() == pts.tobytes() and np.array_equal(got_t, tri)
