"""The speckle filter on the GPU (libbicos_amd/csrc/speckle.hip; include/bicos_c.h, "speckle
filter") against the restatement of tests/speckle_ref.py, which tests/test_speckle_api.py
checks against a second restatement and against hand-derived answers. Every comparison is bit
for bit: the map through uint32 / uint16 views (NaN payloads included), labels and counts as
integers. Every call runs between guard values that must survive it.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import speckle_ref as ref
from tests.test_cli import Q, _built
from tests.test_reproject_api import F32_SENTINEL as REPROJECT_SENTINEL
from tests.test_reproject_api import restate as reproject_restate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECKLE_CPP = os.path.join(ROOT, "tests", "cpp", "speckle_cpp")
PAD = 64          # guard elements on either side of every output
LABEL_GUARD = -7
COUNT_GUARD = 0x5A5A5A5A
DTYPES = {"int16": np.int16, "float32": np.float32}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


def map_guard(dtype):
    return np.dtype(dtype).type(-12345)


def shapes():
    tr, tc = _lib.speckle_tile()
    return [(1, 1), (1, tc + 1), (tr + 1, 1)] + \
        [(r, c) for r in (tr - 1, tr, tr + 1) for c in (tc - 1, tc, tc + 1)] + \
        [(2 * tr + 3, 3 * tc + 5)]


@functools.lru_cache(maxsize=None)
def cases(rows, cols, dtype):
    """the patterns of one shape with their restatements, computed once and shared"""
    out = []
    for name, d, max_size, max_diff, sentinel in ref.patterns(rows, cols, DTYPES[dtype]):
        d.setflags(write=False)
        out.append((name, d, max_size, max_diff, sentinel, ref.restate(d, max_size, max_diff, sentinel)))
    return out


def run(handle, d, max_size, max_diff, sentinel, want_labels=True, want_counts=True,
        in_place=False, stream=None):
    """bicos_speckle_device on a numpy map -> dict(out, labels, counts) of numpy results.
    Every output lies between PAD guard elements, checked here."""
    import torch
    L = _lib.lib()
    rows, cols = d.shape
    n = rows * cols
    dev = torch.device("cuda", 0)
    tdt = torch.float32 if d.dtype == np.float32 else torch.int16
    g = float(map_guard(d.dtype))
    src = torch.full((n + 2 * PAD,), g, dtype=tdt, device=dev)
    src[PAD:PAD + n] = torch.from_numpy(np.array(d).reshape(-1)).to(dev)
    dst = src if in_place else torch.full((n + 2 * PAD,), g, dtype=tdt, device=dev)
    lab = torch.full((n + 2 * PAD,), LABEL_GUARD, dtype=torch.int32, device=dev) if want_labels else None
    cnt = torch.full((4 + 2 * PAD,), COUNT_GUARD, dtype=torch.int32, device=dev) if want_counts else None
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    at = lambda t: t.data_ptr() + PAD * t.element_size() if t is not None else None  # noqa: E731
    size, diff = _lib.speckle_params(max_size, max_diff)
    rc = L.bicos_speckle_device(handle, at(src), _lib.CV_32F if d.dtype == np.float32 else _lib.CV_16S,
                                rows, cols, size, diff, _lib.SPECKLE_F32_SENTINEL if sentinel else 0,
                                at(dst), at(lab), at(cnt), s.cuda_stream)
    _lib.check(rc, "bicos_speckle_device")
    s.synchronize()
    got = {}

    def inner(t, guard):
        h = t.cpu().numpy()
        edge = np.concatenate([h[:PAD], h[PAD + (h.size - 2 * PAD):]])
        assert (edge == guard).all(), "guard values overwritten"
        return h[PAD:h.size - PAD]

    got["out"] = inner(dst, map_guard(d.dtype)).reshape(rows, cols)
    if not in_place:  # the input is left alone
        assert np.array_equal(bits(inner(src, map_guard(d.dtype)).reshape(rows, cols)), bits(d))
    if want_labels:
        got["labels"] = inner(lab, LABEL_GUARD).reshape(rows, cols)
    if want_counts:
        got["counts"] = inner(cnt, COUNT_GUARD).view(np.uint32)
    return got


def check(got, want, name=""):
    assert np.array_equal(bits(got["out"]), bits(want["out"])), name
    if "labels" in got:
        assert np.array_equal(got["labels"], want["labels"]), name
    if "counts" in got:
        assert got["counts"].tolist() == want["counts"].tolist(), name


# ------------------------------------------------------------- shapes x patterns
@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("shape_at", range(13))
def test_every_pattern_at_every_shape(gpu, shape_at, dtype):
    """one-pixel maps and tiles, partial tiles on either side of a full one, and a map of
    3 x 4 tiles whose components cross two borders: map, labels and counts bit for bit"""
    rows, cols = shapes()[shape_at]
    assert len(shapes()) == 13
    all_cases = cases(rows, cols, dtype)
    names = {c[0].split("-")[0] for c in all_cases}
    assert {"constant", "all", "checkerboard", "serpentine", "spiral", "comb", "hook", "blobs",
            "surface"} <= names
    removed_some = kept_some = False
    for name, d, max_size, max_diff, sentinel, want in all_cases:
        check(run(gpu._h, d, max_size, max_diff, sentinel), want, name)
        removed_some |= bool(want["counts"][1])
        kept_some |= bool(want["counts"][0])
    assert removed_some and kept_some  # the cases exercise both verdicts


def test_the_large_shape_has_what_it_is_for(gpu):
    """the constant map is one component over every tile; the serpentine's path is one too"""
    tr, tc = _lib.speckle_tile()
    rows, cols = shapes()[-1]
    assert rows > 2 * tr and cols > 3 * tc
    by_name = {c[0]: c for c in cases(rows, cols, "int16")}
    want = by_name["constant-kept"][5]
    assert (want["labels"] == 0).all() and (want["sizes"] == rows * cols).all()
    serp = [c for n, c in by_name.items() if n.startswith("serpentine-at")][-1][5]
    assert serp["counts"][0] == 0
    assert serp["counts"][3] == 1 and serp["counts"][1] == (rows + 1) // 2 * cols + rows // 2
    hook = [c for n, c in by_name.items() if n.startswith("hook-below")][-1][5]
    assert hook["labels"].max() == cols - 1  # its smallest index lies in the last tile column


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_committed_disparity_maps(gpu, dtype):
    """real matched maps: the golden disparities, max_size on both sides of their speckles"""
    maps = [(n, d) for n, d in ref.golden_maps() if d.dtype == DTYPES[dtype]]
    assert len(maps) >= 6
    removed = 0
    for name, d in maps:
        for max_size, sentinel in ((4, True), (50, True), (50, False)):
            want = ref.restate(d, max_size, 1.0, sentinel)
            removed += int(want["counts"][1])
            check(run(gpu._h, d, max_size, 1.0, sentinel), want, name)
    assert removed > 0


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_more_tile_roots_in_one_workgroup_than_its_list_holds(gpu, dtype):
    """one-pixel-wide stripes down a map two tile rows high and more than 1024 columns wide:
    in the second tile row's first row every pixel is a tile-local root whose size has to
    reach a root in the row above, more of them side by side than the resolve launch's
    per-workgroup list holds (the rest take the direct path)"""
    tr, tc = _lib.speckle_tile()
    rows, cols = tr + 2, 1100
    d = np.empty((rows, cols), DTYPES[dtype])
    d[:, 0::2], d[:, 1::2] = 10, 200
    d[5, 7] = -32768 if dtype == "int16" else np.nan  # one stripe in two pieces
    for max_size in (rows - 1, rows):
        want = ref.restate(d, max_size, 1.0)
        assert (want["sizes"][0] == rows).sum() == cols - 1
        assert bool(want["counts"][0]) == (max_size < rows)
        check(run(gpu._h, d, max_size, 1.0, False), want)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_a_map_larger_than_one_pass_of_the_apply_launch(gpu, dtype):
    """more than 1024 * 1024 pixels: the apply launch's workgroups stride over the map"""
    rows, cols = 1030, 1040
    rng = np.random.default_rng(5)
    d = ref.surface_with_islands(rows, cols, DTYPES[dtype], rng)
    want = ref.restate(d, 6, 1.0)
    assert want["counts"][0] > 0.5 * d.size and want["counts"][1] > 1000
    check(run(gpu._h, d, 6, 1.0, False), want)


# ------------------------------------------------------------------ call forms
def _pick(rows, cols, dtype, prefix, both=True):
    """the first case of that name; with `both`, the first that keeps some pixels and removes
    some"""
    found = [c for c in cases(rows, cols, dtype) if c[0].startswith(prefix) and
             (not both or (c[5]["counts"][0] and c[5]["counts"][1]))]
    assert found, prefix
    return found[0]


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_in_place_equals_out_of_place(gpu, dtype):
    rows, cols = shapes()[-1]
    for prefix in ("blobs-at", "surface-at", "spiral-at"):
        name, d, max_size, max_diff, sentinel, want = _pick(rows, cols, dtype, prefix)
        a = run(gpu._h, d, max_size, max_diff, sentinel)
        b = run(gpu._h, d, max_size, max_diff, sentinel, in_place=True)
        check(b, want, name)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("labels,counts", [(False, False), (True, False), (False, True)])
def test_labels_and_counts_are_each_optional(gpu, dtype, labels, counts):
    rows, cols = shapes()[-1]
    name, d, max_size, max_diff, sentinel, want = _pick(rows, cols, dtype, "blobs-at")
    assert want["counts"][0] and want["counts"][1]
    got = run(gpu._h, d, max_size, max_diff, sentinel, want_labels=labels, want_counts=counts)
    assert set(got) == {"out"} | ({"labels"} if labels else set()) | ({"counts"} if counts else set())
    check(got, want, name)


def test_max_size_zero_returns_the_input_bits(gpu):
    rows, cols = shapes()[-1]
    name, d, _, max_diff, sentinel, _ = _pick(rows, cols, "float32", "nan-inf-sentinel1", both=False)
    assert len(np.unique(bits(d)[np.isnan(d)])) >= 2  # several NaN payloads
    got = run(gpu._h, d, 0, max_diff, sentinel)
    assert np.array_equal(bits(got["out"]), bits(d))
    assert got["counts"][1] == 0 and got["counts"][3] == 0
    check(got, ref.restate(d, 0, max_diff, sentinel), name)


def test_non_default_stream(gpu):
    import torch
    rows, cols = shapes()[-1]
    name, d, max_size, max_diff, sentinel, want = _pick(rows, cols, "float32", "surface-at")
    check(run(gpu._h, d, max_size, max_diff, sentinel, stream=torch.cuda.Stream()), want, name)


def test_same_call_twice_gives_the_same_bytes(gpu):
    rows, cols = shapes()[-1]
    name, d, max_size, max_diff, sentinel, want = _pick(rows, cols, "float32", "blobs-at")
    a = run(gpu._h, d, max_size, max_diff, sentinel)
    b = run(gpu._h, d, max_size, max_diff, sentinel)
    check(a, want, name)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_consecutive_calls_of_different_shapes_on_one_engine(gpu):
    """a fresh engine: its workspace is first sized by a small map, then grows, then is reused
    by a smaller map again"""
    from libbicos_amd import device
    eng = device.Engine(0)
    all_shapes = shapes()
    for rows, cols in (all_shapes[3], all_shapes[-1], all_shapes[1], all_shapes[-1]):
        for dtype in ("int16", "float32"):
            name, d, max_size, max_diff, sentinel, want = _pick(rows, cols, dtype, "blobs-at")
            check(run(eng._h, d, max_size, max_diff, sentinel, want_labels=(dtype == "int16")),
                  want, name)
    eng.close()


@pytest.mark.parametrize("rows,cols", [(0, 5), (5, 0), (0, 0)])
def test_empty_maps(gpu, rows, cols):
    got = run(gpu._h, np.zeros((rows, cols), np.int16), 3, 1.0, False)
    assert got["counts"].tolist() == [0, 0, 0, 0]
    counts = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    rc = _lib.lib().bicos_speckle_host(None, None, _lib.CV_16S, rows, cols, 3, 1.0, 0, None, None,
                                       counts)
    assert rc == 0 and list(counts) == [0, 0, 0, 0]


# ------------------------------------------------------------------- every API
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_python_and_host_entries(gpu, dtype):
    import torch
    from libbicos_amd import pybicos
    rows, cols = shapes()[-1]
    name, d, max_size, max_diff, _, _ = _pick(rows, cols, dtype, "surface-at")
    for sentinel in (True, False):
        want = ref.restate(d, max_size, max_diff, sentinel)
        assert want["counts"][0] and want["counts"][1]
        # Engine.filter_speckles: new tensors, labels and counts, nothing synchronised for us
        t = torch.from_numpy(np.array(d)).cuda()
        cnt = torch.zeros((4,), dtype=torch.int32, device=t.device)
        out, lab = gpu.filter_speckles(t, max_size, max_diff, sentinel=sentinel, labels=True, counts=cnt)
        assert out.data_ptr() != t.data_ptr() and out.dtype == t.dtype and lab.dtype == torch.int32
        check(dict(out=out.cpu().numpy(), labels=lab.cpu().numpy(),
                   counts=cnt.cpu().numpy().view(np.uint32)), want, name)
        assert np.array_equal(bits(t.cpu().numpy()), bits(d))
        # the map alone; in place through out=
        only = gpu.filter_speckles(t, max_size, max_diff, sentinel=sentinel)
        assert isinstance(only, torch.Tensor)
        same = gpu.filter_speckles(t, max_size, max_diff, sentinel=sentinel, out=t)
        assert same.data_ptr() == t.data_ptr()
        for got in (only, same):
            assert np.array_equal(bits(got.cpu().numpy()), bits(want["out"]))
        # pybicos: numpy in, (numpy, dict) out
        host, stats = pybicos.filter_speckles(d, max_size, max_diff, sentinel)
        assert host.dtype == d.dtype and np.array_equal(bits(host), bits(want["out"]))
        assert [stats[k] for k in ("kept", "removed", "invalid", "removed_components")] == \
            want["counts"].tolist()
        # bicos_speckle_host with labels, in place on a copy
        buf = np.array(d)
        labels = np.full((rows, cols), LABEL_GUARD, np.int32)
        counts = (ctypes.c_uint32 * 4)()
        rc = _lib.lib().bicos_speckle_host(
            None, buf.ctypes.data, _lib.CV_32F if dtype == "float32" else _lib.CV_16S, rows, cols,
            max_size, max_diff, 1 if sentinel else 0, buf.ctypes.data, labels.ctypes.data, counts)
        assert rc == 0, _lib.lib().bicos_last_error()
        check(dict(out=buf, labels=labels, counts=np.array(list(counts), np.uint32)), want, name)
    with pytest.raises(ValueError):
        gpu.filter_speckles(torch.zeros((4, 8), device="cuda"), 3, out=torch.zeros((4, 9), device="cuda"))
    with pytest.raises(ValueError):
        gpu.filter_speckles(torch.zeros((4, 8), dtype=torch.float64, device="cuda"), 3)


@pytest.mark.parametrize("dtype,flags", [("int16", 0), ("float32", 1), ("float32", 0)])
def test_cpp_api(gpu, dtype, flags, tmp_path):
    _built()
    if not os.path.exists(SPECKLE_CPP):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "speckle.mk"],
                       check=True, capture_output=True)
    rows, cols = shapes()[-1]
    name, d, max_size, max_diff, _, _ = _pick(rows, cols, dtype, "surface-at")
    want = ref.restate(d, max_size, max_diff, bool(flags))
    assert want["counts"][0] and want["counts"][1]
    raw = tmp_path / "d.raw"
    raw.write_bytes(d.tobytes())
    prefix = str(tmp_path / "o")
    r = subprocess.run([SPECKLE_CPP, str(raw), str(rows), str(cols),
                        str(_lib.CV_32F if dtype == "float32" else _lib.CV_16S), str(flags),
                        str(max_size), repr(float(max_diff)), prefix],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    line = " ".join(str(int(v)) for v in want["counts"])
    assert r.stdout.split("\n")[:4] == ["host " + line, "dev " + line, "buf " + line,
                                        "inplace " + line]
    for form in ("host", "dev", "buf", "inplace"):
        assert open(prefix + "." + form + ".map", "rb").read() == want["out"].tobytes(), form
    for form in ("host", "dev", "buf"):
        assert open(prefix + "." + form + ".lab", "rb").read() == want["labels"].tobytes(), form


@pytest.mark.parametrize("cfg", [dict(nxcorr_threshold=0.75),
                                 dict(nxcorr_threshold=0.75, subpixel_step=0.2),
                                 dict(nxcorr_threshold=None)],
                         ids=["nxc_sentinel", "subpixel_nan", "int16"])
def test_match_filter_reproject_on_the_device(gpu, cfg):
    """Engine.match -> filter_speckles -> reproject_points without leaving the GPU, against
    the two restatements applied one after the other to the matched map"""
    import torch
    from libbicos_amd import device
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(12, 40, 200)
    disp, _ = gpu.match(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(),
                        device.MatchConfig(**cfg))
    matched = disp.cpu().numpy()
    max_diff = 1.0
    cnt = torch.zeros((4,), dtype=torch.int32, device=disp.device)
    filtered = gpu.filter_speckles(disp, 20, max_diff, out=disp, counts=cnt)
    pts, idx, stats = gpu.reproject_points(filtered, Q, with_index=True)
    want = ref.restate(matched, 20, max_diff, True)
    assert want["counts"][1] > 0 and want["counts"][0] > 0
    assert cnt.cpu().numpy().view(np.uint32).tolist() == want["counts"].tolist()
    assert np.array_equal(bits(filtered.cpu().numpy()), bits(want["out"]))
    points = reproject_restate(want["out"], Q, REPROJECT_SENTINEL)
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), points["points"].view(np.uint32))
    assert np.array_equal(idx.cpu().numpy(), points["index"])
    assert [stats[k] for k in ("kept", "invalid", "nonfinite", "negative_z")] == \
        points["counts"].tolist()
