"""The median filter on the GPU (libbicos_amd/csrc/median.hip; include/bicos_c.h, "median
filter") against restatement (a) of tests/median_ref.py, which tests/test_median_api.py checks
against a second restatement and against hand-derived answers. Every comparison is bit for
bit: the map through uint32 / uint16 views (NaN payloads included), the counts as integers.
Every call runs between guard values that must survive it, and must leave its input alone.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import median_ref as ref
from tests import speckle_ref
from tests.test_cli import Q, _built
from tests.test_reproject_api import F32_SENTINEL as REPROJECT_SENTINEL
from tests.test_reproject_api import restate as reproject_restate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEDIAN_CPP = os.path.join(ROOT, "tests", "cpp", "median_cpp")
PAD = 64          # guard elements on either side of every output
MAP_GUARD = -12345  # as an integer of the map's width
COUNT_GUARD = 0x5A5A5A5A
DTYPES = {"int16": np.int16, "float32": np.float32}
bits = ref.bits


def shapes():
    """where the halo, the clipped window and the tile seam can go wrong: maps smaller than a
    window, partial tiles on either side of a full one, 3 x 3 tiles with both seams, a map
    narrower than the halo under a tile seam, and an odd width (int16 rows not dword-aligned)"""
    tr, tc = _lib.median_tile()
    return [(1, 1), (1, 7), (7, 1), (2, 2), (tr - 1, tc - 1), (tr, tc), (tr + 1, tc + 1),
            (2 * tr + 3, 2 * tc + 5), (tr + 2, 3), (5, tc + 3)]


@functools.lru_cache(maxsize=None)
def cases(rows, cols, dtype, ksize):
    """the patterns of one shape with the fill_min-independent part of their restatement,
    computed once and shared"""
    out = []
    for name, d, sentinel in ref.patterns(rows, cols, DTYPES[dtype]):
        d.setflags(write=False)
        out.append((name, d, sentinel, ref.windows(d, ksize, sentinel)))
    return out


def run(handle, d, ksize, fill_min, sentinel, want_counts=True, stream=None):
    """bicos_median_device on a numpy map -> dict(out, counts) of numpy results. Every output
    lies between PAD guard elements, checked here, and the input is compared after the call."""
    import torch
    L = _lib.lib()
    rows, cols = d.shape
    n = rows * cols
    dev = torch.device("cuda", 0)
    # the maps travel as integers of their width: bits in, bits out
    idt, ndt = (torch.int32, np.int32) if d.dtype == np.float32 else (torch.int16, np.int16)
    src = torch.full((n + 2 * PAD,), MAP_GUARD, dtype=idt, device=dev)
    src[PAD:PAD + n] = torch.from_numpy(np.array(d).reshape(-1).view(ndt)).to(dev)
    dst = torch.full((n + 2 * PAD,), MAP_GUARD, dtype=idt, device=dev)
    cnt = torch.full((4 + 2 * PAD,), COUNT_GUARD, dtype=torch.int32, device=dev) if want_counts else None
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    at = lambda t: t.data_ptr() + PAD * t.element_size() if t is not None else None  # noqa: E731
    k, fill = _lib.median_params(ksize, fill_min)
    rc = L.bicos_median_device(handle, at(src), _lib.CV_32F if d.dtype == np.float32 else _lib.CV_16S,
                               rows, cols, k, fill, _lib.MEDIAN_F32_SENTINEL if sentinel else 0,
                               at(dst), at(cnt), s.cuda_stream)
    _lib.check(rc, "bicos_median_device")
    s.synchronize()
    got = {}

    def inner(t, guard):
        h = t.cpu().numpy()
        edge = np.concatenate([h[:PAD], h[PAD + (h.size - 2 * PAD):]])
        assert (edge == guard).all(), "guard values overwritten"
        return h[PAD:h.size - PAD]

    got["out"] = inner(dst, MAP_GUARD).view(d.dtype).reshape(rows, cols)
    assert np.array_equal(bits(inner(src, MAP_GUARD).view(d.dtype).reshape(rows, cols)), bits(d)), \
        "the input was changed"
    if want_counts:
        got["counts"] = inner(cnt, COUNT_GUARD).view(np.uint32)
    return got


def check(got, want, name=""):
    assert np.array_equal(bits(got["out"]), bits(want["out"])), name
    if "counts" in got:
        assert got["counts"].tolist() == want["counts"].tolist(), name


# ------------------------------------------------------------- shapes x patterns
@pytest.mark.parametrize("ksize", [3, 5])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("shape_at", range(10))
def test_every_pattern_at_every_shape(gpu, shape_at, dtype, ksize):
    """every pattern x fill_min in {0, 1, ksize^2 / 2 + 1, ksize^2}: map and counts bit for bit"""
    assert len(shapes()) == 10
    rows, cols = shapes()[shape_at]
    all_cases = cases(rows, cols, dtype, ksize)
    names = {c[0].split("-")[0] for c in all_cases}
    assert {"random30", "all", "checkerboard", "constant", "outliers", "holes"} <= names
    assert ("special" in names and "signed" in names) == (dtype == "float32")
    total = np.zeros(4, np.uint64)
    for name, d, sentinel, win in all_cases:
        for fill_min in ref.fill_mins(ksize):
            want = ref.finish(d, win, fill_min)
            check(run(gpu._h, d, ksize, fill_min, sentinel), want, (name, fill_min))
            total += want["counts"]
    assert total[0] and total[3]
    if rows * cols > 4:  # the cases exercise every verdict
        assert total[1] and total[2]


def test_the_shapes_are_what_they_are_for():
    tr, tc = _lib.median_tile()
    s = shapes()
    assert (tr, tc) in s and (tr - 1, tc - 1) in s and (tr + 1, tc + 1) in s
    assert max(r for r, _ in s) <= 3 * tr and max(c for _, c in s) <= 3 * tc
    assert any(r > 2 * tr and c > 2 * tc for r, c in s)
    assert any(c % 2 == 1 and r > 1 for r, c in s)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_committed_disparity_maps(gpu, dtype):
    """real matched maps: the golden disparities"""
    maps = [(n, d) for n, d in ref.golden_maps() if d.dtype == DTYPES[dtype]]
    assert len(maps) >= 3
    touched = np.zeros(4, np.uint64)
    for name, d in maps[:6]:
        for ksize in (3, 5):
            for sentinel in (True, False):
                win = ref.windows(d, ksize, sentinel)
                for fill_min in (0, ksize * ksize // 2 + 1):
                    want = ref.finish(d, win, fill_min)
                    touched += want["counts"]
                    check(run(gpu._h, d, ksize, fill_min, sentinel), want, name)
    assert touched[1] > 0


# ------------------------------------------------------------------ call forms
def _pick(rows, cols, dtype, ksize, prefix):
    found = [c for c in cases(rows, cols, dtype, ksize) if c[0].startswith(prefix)]
    assert found, prefix
    return found[0]


def test_non_default_stream_no_counts_and_no_engine(gpu):
    import torch
    rows, cols = shapes()[7]
    for dtype, ksize in (("float32", 5), ("int16", 3)):
        name, d, sentinel, win = _pick(rows, cols, dtype, ksize, "holes")
        fill_min = ksize * ksize // 2 + 1
        want = ref.finish(d, win, fill_min)
        assert want["counts"][1] and want["counts"][2] and want["counts"][3]
        check(run(gpu._h, d, ksize, fill_min, sentinel, stream=torch.cuda.Stream()), want, name)
        got = run(gpu._h, d, ksize, fill_min, sentinel, want_counts=False)
        assert set(got) == {"out"}
        check(got, want, name)
        check(run(None, d, ksize, fill_min, sentinel), want, name)  # e == NULL: no workspace


def test_same_call_twice_gives_the_same_bytes(gpu):
    rows, cols = shapes()[7]
    name, d, sentinel, win = _pick(rows, cols, "float32", 5, "random30-ties-sentinel1")
    want = ref.finish(d, win, 1)
    a = run(gpu._h, d, 5, 1, sentinel)
    b = run(gpu._h, d, 5, 1, sentinel)
    check(a, want, name)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_a_map_of_more_tiles_than_workgroups(gpu):
    """more than 1024 tiles: the workgroups stride over the tiles and sum their counts. The map
    is a few distinct rows repeated, so the restatement of one period is the whole answer away
    from the top and bottom borders; those are compared with a restatement of their own."""
    tr, tc = _lib.median_tile()
    rows, cols = 36 * tr + 5, 30 * tc + 3
    assert ((rows + tr - 1) // tr) * ((cols + tc - 1) // tc) > 1024
    rng = np.random.default_rng(11)
    period = 8
    base = rng.integers(-40, 40, (period, cols)).astype(np.int16)
    base[rng.random(base.shape) < 0.25] = -32768
    d = np.tile(base, (rows // period + 1, 1))[:rows]
    # rows [4, 4 + period) of a map of 4 + period + 4 rows see the same windows as any interior row
    small = ref.restate(d[:period + 8], 5, 13)["out"]
    got = run(gpu._h, d, 5, 13, False)
    out = got["out"]
    assert np.array_equal(out[:period + 4], small[:period + 4])
    for r in range(4, rows - 4):
        assert np.array_equal(out[r], small[4 + (r - 4) % period]), r
    tail = ref.restate(d[rows - 12:], 5, 13)["out"]
    assert np.array_equal(out[rows - 4:], tail[-4:])
    c = got["counts"]
    assert int(c.sum()) == rows * cols and c[1] > 0 and c[2] > 0 and c[3] > 0
    valid = d != -32768
    assert c[0] == (valid & (out == d)).sum() and c[1] == (valid & (out != d)).sum()
    assert c[2] == (~valid & (out != -32768)).sum() and c[3] == (~valid & (out == -32768)).sum()


@pytest.mark.parametrize("rows,cols", [(0, 5), (5, 0), (0, 0)])
def test_empty_maps(gpu, rows, cols):
    got = run(gpu._h, np.zeros((rows, cols), np.int16), 3, 1, False)
    assert got["counts"].tolist() == [0, 0, 0, 0]
    counts = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    rc = _lib.lib().bicos_median_host(None, None, _lib.CV_16S, rows, cols, 3, 1, 0, None, counts)
    assert rc == 0 and list(counts) == [0, 0, 0, 0]


# ------------------------------------------------------------------- every API
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_python_and_host_entries(gpu, dtype):
    import torch
    from libbicos_amd import pybicos
    rows, cols = shapes()[7]
    ksize, fill_min = 5, 13
    name, d, _, _ = _pick(rows, cols, dtype, ksize, "holes")
    for sentinel in (True, False):
        want = ref.restate(d, ksize, fill_min, sentinel)
        assert want["counts"][1] and want["counts"][2]
        # Engine.median_filter: a new tensor and counts, nothing synchronised for us
        t = torch.from_numpy(np.array(d)).cuda()
        cnt = torch.zeros((4,), dtype=torch.int32, device=t.device)
        out = gpu.median_filter(t, ksize, fill_min, sentinel=sentinel, counts=cnt)
        assert out.data_ptr() != t.data_ptr() and out.dtype == t.dtype
        check(dict(out=out.cpu().numpy(), counts=cnt.cpu().numpy().view(np.uint32)), want, name)
        assert np.array_equal(bits(t.cpu().numpy()), bits(d))
        given = torch.empty_like(t)
        assert gpu.median_filter(t, ksize, fill_min, sentinel=sentinel, out=given) is given
        assert np.array_equal(bits(given.cpu().numpy()), bits(want["out"]))
        # pybicos: numpy in, (numpy, dict) out
        host, stats = pybicos.median_filter(d, ksize, fill_min, sentinel)
        assert host.dtype == d.dtype and np.array_equal(bits(host), bits(want["out"]))
        assert [stats[k] for k in ("unchanged", "changed", "filled", "invalid")] == \
            want["counts"].tolist()
        # bicos_median_host with out being the input buffer
        buf = np.array(d)
        counts = (ctypes.c_uint32 * 4)()
        rc = _lib.lib().bicos_median_host(
            None, buf.ctypes.data, _lib.CV_32F if dtype == "float32" else _lib.CV_16S, rows, cols,
            ksize, fill_min, 1 if sentinel else 0, buf.ctypes.data, counts)
        assert rc == 0, _lib.lib().bicos_last_error()
        check(dict(out=buf, counts=np.array(list(counts), np.uint32)), want, name)
    # the defaults: ksize 3, no filling, sentinel on
    t = torch.from_numpy(np.array(d)).cuda()
    assert np.array_equal(bits(gpu.median_filter(t).cpu().numpy()), bits(ref.restate(d, 3, 0, True)["out"]))
    with pytest.raises(ValueError, match="storage"):
        gpu.median_filter(t, out=t)
    with pytest.raises(ValueError, match="storage"):
        gpu.median_filter(t[:4], out=t[2:6])
    with pytest.raises(ValueError):
        gpu.median_filter(torch.zeros((4, 8), device="cuda"), out=torch.zeros((4, 9), device="cuda"))
    with pytest.raises(ValueError):
        gpu.median_filter(torch.zeros((4, 8), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="ksize"):
        gpu.median_filter(t, 7)


@pytest.mark.parametrize("dtype,flags", [("int16", 0), ("float32", 1), ("float32", 0)])
def test_cpp_api(gpu, dtype, flags, tmp_path):
    _built()
    if not os.path.exists(MEDIAN_CPP):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "median.mk"],
                       check=True, capture_output=True)
    rows, cols = shapes()[7]
    ksize, fill_min = 5, 13
    name, d, _, _ = _pick(rows, cols, dtype, ksize, "holes")
    want = ref.restate(d, ksize, fill_min, bool(flags))
    assert want["counts"][1] and want["counts"][2]
    raw = tmp_path / "d.raw"
    raw.write_bytes(d.tobytes())
    prefix = str(tmp_path / "o")
    r = subprocess.run([MEDIAN_CPP, str(raw), str(rows), str(cols),
                        str(_lib.CV_32F if dtype == "float32" else _lib.CV_16S), str(flags),
                        str(ksize), str(fill_min), prefix],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    line = " ".join(str(int(v)) for v in want["counts"])
    assert r.stdout.split("\n")[:4] == ["host " + line, "dev " + line, "hostinplace " + line,
                                        "buf " + line]
    for form in ("host", "dev", "hostinplace", "buf"):
        assert open(prefix + "." + form + ".map", "rb").read() == want["out"].tobytes(), form


@pytest.mark.parametrize("cfg", [dict(nxcorr_threshold=0.75),
                                 dict(nxcorr_threshold=0.75, subpixel_step=0.2),
                                 dict(nxcorr_threshold=None)],
                         ids=["nxc_sentinel", "subpixel_nan", "int16"])
def test_match_speckle_median_reproject_on_the_device(gpu, cfg):
    """Engine.match -> filter_speckles -> median_filter(5, fill_min=13) -> reproject_points
    without leaving the GPU, each stage against its restatement applied to the stage before.
    On this frame the restatements alone give changed = 540 and filled = 1 after the speckle
    filter removed its islands (computed from the CPU oracle's map of the same frame)."""
    import torch
    from libbicos_amd import device
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(12, 40, 200)
    disp, _ = gpu.match(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(),
                        device.MatchConfig(**cfg))
    matched = disp.cpu().numpy()
    cnt_s = torch.zeros((4,), dtype=torch.int32, device=disp.device)
    cnt_m = torch.zeros((4,), dtype=torch.int32, device=disp.device)
    despeckled = gpu.filter_speckles(disp, 20, 1.0, out=disp, counts=cnt_s)
    smoothed = gpu.median_filter(despeckled, 5, 13, counts=cnt_m)
    pts, idx, stats = gpu.reproject_points(smoothed, Q, with_index=True)
    want_s = speckle_ref.restate(matched, 20, 1.0, True)
    assert cnt_s.cpu().numpy().view(np.uint32).tolist() == want_s["counts"].tolist()
    assert np.array_equal(bits(despeckled.cpu().numpy()), bits(want_s["out"]))
    want_m = ref.restate(want_s["out"], 5, 13, True)
    assert want_m["counts"][1] > 0 and want_m["counts"][2] > 0  # changed, filled
    assert cnt_m.cpu().numpy().view(np.uint32).tolist() == want_m["counts"].tolist()
    assert np.array_equal(bits(smoothed.cpu().numpy()), bits(want_m["out"]))
    points = reproject_restate(want_m["out"], Q, REPROJECT_SENTINEL)
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), points["points"].view(np.uint32))
    assert np.array_equal(idx.cpu().numpy(), points["index"])
    assert [stats[k] for k in ("kept", "invalid", "nonfinite", "negative_z")] == \
        points["counts"].tolist()
