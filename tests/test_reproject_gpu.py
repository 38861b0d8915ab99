"""Reprojection on the GPU (libbicos_amd/csrc/reproject.hip; include/bicos_c.h, "reprojection")
against the numpy restatement of tests/test_reproject_api.py, which that file checks against
the project's CPU writer. Every comparison is bit for bit (uint32 views), except where the
definition says "three NaNs": those are compared by isnan.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from libbicos_amd import _lib
from tests.test_cli import CLI, Q, YAML, _built, _write_folder, read_tiff
from tests.test_reproject_api import (ALLOW_NEGATIVE_Z, F32_SENTINEL, make_map, restate,
                                      xyz_text)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPROJECT_CPP = os.path.join(ROOT, "tests", "cpp", "reproject_cpp")
GUARD = -12345.0  # fills the outputs before a call: whatever the call leaves alone keeps it


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(rows, cols, dtype, flags, seed=0):
    """(map, restatement), computed once and shared (read-only)"""
    d = make_map(rows, cols, np.dtype(dtype).type, seed + rows * 7 + cols)
    d.setflags(write=False)
    return d, restate(d, Q, flags)


def run(handle, d, flags, want_map=True, want_points=True, want_index=True, capacity=None,
        stream=None):
    """bicos_reproject_device on a numpy map -> dict of numpy results. The point and index
    buffers hold rows*cols entries, all GUARD before the call; `capacity` is what the call is
    told."""
    import torch
    L = _lib.lib()
    rows, cols = d.shape
    n = max(rows * cols, 1)
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(np.array(d)).to(dev) if d.size else None  # (a writable copy)
    xyz = torch.full((n, 3), GUARD, dtype=torch.float32, device=dev) if want_map else None
    pts = torch.full((n, 3), GUARD, dtype=torch.float32, device=dev) if want_points else None
    idx = torch.full((n,), -7, dtype=torch.int32, device=dev) if want_index else None
    cnt = torch.full((4,), -1, dtype=torch.int32, device=dev) if want_points else None
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    ptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
    rc = L.bicos_reproject_device(
        handle, ptr(t), _lib.CV_32F if d.dtype == np.float32 else _lib.CV_16S, rows, cols,
        _lib.reproject_q(Q), flags, ptr(xyz), ptr(pts), ptr(idx),
        rows * cols if capacity is None else capacity, ptr(cnt), s.cuda_stream)
    _lib.check(rc, "bicos_reproject_device")
    s.synchronize()
    out = {}
    if want_map:
        out["map"] = xyz.cpu().numpy()[:rows * cols].reshape(rows, cols, 3)
    if want_points:
        out["points"] = pts.cpu().numpy()
        out["counts"] = cnt.cpu().numpy().view(np.uint32)
    if want_index:
        out["index"] = idx.cpu().numpy()
    return out


def check(got, want, capacity=None):
    """every output present in `got` against the restatement `want`"""
    kept = int(want["counts"][0])
    n = kept if capacity is None else min(kept, capacity)
    if "map" in got:
        k = want["kept"]
        assert np.array_equal(bits(got["map"])[k], bits(want["map"])[k])
        assert np.isnan(got["map"][~k]).all()
    if "points" in got:
        assert got["counts"].tolist() == want["counts"].tolist()
        assert np.array_equal(bits(got["points"][:n]), bits(want["points"][:n]))
        assert (got["points"][n:] == GUARD).all()  # nothing past the list (or the capacity)
    if "index" in got:
        assert np.array_equal(got["index"][:n], want["index"][:n])
        assert (got["index"][n:] == -7).all()


def segment():
    return _lib.lib().bicos_reproject_segment()


def shapes():
    seg = segment()
    return [(1, 1), (1, 63), (3, 65), (7, 257), (1, seg), (1, seg - 1), (1, seg + 1),
            (2, seg // 2), (64, 2049), (1536, 2048)]


# ------------------------------------------------------------- shapes and types
@pytest.mark.parametrize("dtype,flags", [("int16", 0), ("float32", F32_SENTINEL)])
@pytest.mark.parametrize("shape_at", range(10))
def test_shapes(gpu, shape_at, dtype, flags):
    """tiny maps, maps around one segment, a row that is no multiple of anything, and a
    cfg2-sized map whose segments outnumber the scan's threads"""
    rows, cols = shapes()[shape_at]
    d, want = case(rows, cols, dtype, flags)
    assert want["counts"][0] > 0.3 * d.size
    if (rows, cols) == (1536, 2048):
        assert -(-d.size // segment()) > 1024  # more segments than the scan has threads
    got = run(gpu._h, d, flags)
    check(got, want)
    # the list is the dense map's non-NaN pixels in row-major order
    flat = got["map"].reshape(-1, 3)
    there = ~np.isnan(flat).any(axis=1)
    kept = int(got["counts"][0])
    assert np.array_equal(bits(flat[there]), bits(got["points"][:kept]))
    assert np.array_equal(np.flatnonzero(there), got["index"][:kept])


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [(7, 257), (3, 2731)])
def test_float_maps_under_every_flag_combination(gpu, shape, flags):
    d, want = case(shape[0], shape[1], "float32", flags, seed=5)
    assert want["counts"][0] > 0.3 * d.size
    assert (d == np.float32(-32768.0)).sum() > 0 and np.isnan(d).sum() > 0
    check(run(gpu._h, d, flags), want)


@pytest.mark.parametrize("flags", [0, 1])
def test_int16_maps_with_and_without_negative_z(gpu, flags):
    d, want = case(5, 1000, "int16", flags, seed=9)
    assert want["counts"][0] > 0.3 * d.size and want["counts"][1] > 0
    assert (want["counts"][3] > 0) == (flags == 0)
    check(run(gpu._h, d, flags), want)


# ------------------------------------------------------------- class extremes
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_all_invalid(gpu, dtype):
    seg = segment()
    d = np.full((3, seg + 5), -32768 if dtype == "int16" else np.nan, dtype)
    want = restate(d, Q, 0)
    assert want["counts"].tolist() == [0, d.size, 0, 0]
    check(run(gpu._h, d, 0), want)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_all_kept(gpu, dtype):
    d = np.full((3, segment() + 5), 30, dtype)
    want = restate(d, Q, 0)
    assert want["counts"].tolist() == [d.size, 0, 0, 0]
    check(run(gpu._h, d, 0), want)


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_single_kept_pixel_in_the_last_position(gpu, dtype):
    """(one point by construction, so the 0.3 floor of the other tests cannot hold here: the
    test demands that exactly this pixel comes out)"""
    d = np.full((3, segment() + 5), -32768 if dtype == "int16" else np.nan, dtype)
    d[-1, -1] = 30
    want = restate(d, Q, 0)
    assert want["counts"].tolist() == [1, d.size - 1, 0, 0]
    assert want["index"].tolist() == [d.size - 1]
    check(run(gpu._h, d, 0), want)


# -------------------------------------------------------- output combinations
@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("outs", [(True, False, False), (False, True, False), (False, True, True),
                                  (True, True, False), (True, True, True)],
                         ids=["map", "points", "points_index", "map_points", "all"])
def test_output_combinations(gpu, outs, dtype):
    d, want = case(7, 257, dtype, F32_SENTINEL)
    assert want["counts"][0] > 0.3 * d.size
    got = run(gpu._h, d, F32_SENTINEL, *outs)
    assert set(got) == {k for k, on in zip(("map", "points", "index"), outs) if on} | \
        ({"counts"} if outs[1] else set())
    check(got, want)


def test_dense_map_without_an_engine(gpu):
    for dtype in ("int16", "float32"):
        d, want = case(3, segment() + 1, dtype, 0, seed=2)
        assert want["counts"][0] > 0.3 * d.size
        check(run(None, d, 0, True, False, False), want)


@pytest.mark.parametrize("capacity", [0, 1, 700, 2049])
def test_capacity_below_kept(gpu, capacity):
    """the first `capacity` points and indices, nothing past them in the same allocations
    (still GUARD there), and the full count"""
    d, want = case(3, 2731, "float32", F32_SENTINEL, seed=5)
    assert want["counts"][0] > 0.3 * d.size and want["counts"][0] > capacity
    got = run(gpu._h, d, F32_SENTINEL, want_map=False, capacity=capacity)
    assert got["counts"][0] == want["counts"][0]
    check(got, want, capacity=capacity)


@pytest.mark.parametrize("rows,cols", [(0, 5), (5, 0), (0, 0)])
def test_empty_maps(gpu, rows, cols):
    got = run(gpu._h, np.zeros((rows, cols), np.int16), 0)
    assert got["counts"].tolist() == [0, 0, 0, 0]
    assert (got["points"] == GUARD).all() and (got["index"] == -7).all()
    counts = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    pts = np.full((1, 3), GUARD, np.float32)
    rc = _lib.lib().bicos_reproject_host(None, None, _lib.CV_16S, rows, cols, _lib.reproject_q(Q),
                                         0, None, pts.ctypes.data, None, 1, counts)
    assert rc == 0 and list(counts) == [0, 0, 0, 0] and (pts == GUARD).all()


def test_same_call_twice_gives_the_same_bytes(gpu):
    d, want = case(64, 2049, "float32", F32_SENTINEL)
    assert want["counts"][0] > 0.3 * d.size
    a = run(gpu._h, d, F32_SENTINEL)
    b = run(gpu._h, d, F32_SENTINEL)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------- engine reuse
def test_engine_reuse_across_streams_and_a_growing_workspace(oracle):
    """one engine: a reprojection, then a match (whose workspace is far larger), then a
    reprojection of a larger map, on two streams -- the Lease orders them on the shared
    workspace and the workspace grows between uses"""
    import torch
    from libbicos_amd import device
    from libbicos_amd.synthetic import stereo_stack
    eng = device.Engine(0)
    small, want_small = case(7, 257, "int16", 0)
    large, want_large = case(1536, 2048, "float32", F32_SENTINEL)
    assert want_small["counts"][0] > 0.3 * small.size
    assert want_large["counts"][0] > 0.3 * large.size
    L, R = stereo_stack(12, 40, 200)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    ts, tg = torch.from_numpy(small.copy()).cuda(), torch.from_numpy(large.copy()).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    p1, i1, st1 = eng.reproject_points(ts, Q, sentinel=False, with_index=True, stream=s1)
    disp, _ = eng.match(tl, tr, device.MatchConfig(nxcorr_threshold=0.75), stream=s2)
    m2 = eng.reproject_map(tg, Q, stream=s1)
    p2, i2, st2 = eng.reproject_points(tg, Q, with_index=True, stream=s2)
    torch.cuda.synchronize()
    rd, _ = oracle.match(L, R, oracle.OracleConfig(nxcorr_threshold=0.75))
    assert np.array_equal(bits(disp.cpu().numpy()), bits(rd))
    for p, i, st, want in ((p1, i1, st1, want_small), (p2, i2, st2, want_large)):
        assert [st[k] for k in ("kept", "invalid", "nonfinite", "negative_z")] == \
            want["counts"].tolist()
        assert np.array_equal(bits(p.cpu().numpy()), bits(want["points"]))
        assert np.array_equal(i.cpu().numpy(), want["index"])
    k = want_large["kept"]
    got = m2.cpu().numpy()
    assert np.array_equal(bits(got)[k], bits(want_large["map"])[k]) and np.isnan(got[~k]).all()
    eng.close()


# ----------------------------------------------------- from a real match, every API
@pytest.mark.parametrize("cfg", [dict(nxcorr_threshold=0.75),
                                 dict(nxcorr_threshold=0.75, subpixel_step=0.2),
                                 dict(nxcorr_threshold=None)],
                         ids=["nxc_sentinel", "subpixel_nan", "int16"])
def test_end_to_end_from_a_match(gpu, cfg, tmp_path):
    import torch
    from libbicos_amd import device, pybicos
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(12, 40, 200)
    disp, _ = gpu.match(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(),
                        device.MatchConfig(**cfg))
    pts, idx, stats = gpu.reproject_points(disp, Q, with_index=True)
    xyz = gpu.reproject_map(disp, Q)
    d = disp.cpu().numpy()
    want = restate(d, Q, F32_SENTINEL)  # Python's default: the sentinel is invalid
    assert want["counts"][0] > 0.3 * d.size
    assert [stats[k] for k in ("kept", "invalid", "nonfinite", "negative_z")] == \
        want["counts"].tolist()
    assert np.array_equal(bits(pts.cpu().numpy()), bits(want["points"]))
    assert np.array_equal(idx.cpu().numpy(), want["index"])
    k = want["kept"]
    got = xyz.cpu().numpy()
    assert np.array_equal(bits(got)[k], bits(want["map"])[k]) and np.isnan(got[~k]).all()
    # out= with a capacity: enough, then too small
    out = torch.empty((int(want["counts"][0]), 3), dtype=torch.float32, device=disp.device)
    p2, i2, _ = gpu.reproject_points(disp, Q, out=out)
    assert i2 is None and p2.data_ptr() == out.data_ptr()
    assert np.array_equal(bits(p2.cpu().numpy()), bits(want["points"]))
    with pytest.raises(RuntimeError, match="were kept"):
        gpu.reproject_points(disp, Q, out=out[:10])
    with pytest.raises(ValueError):
        gpu.reproject_map(disp, Q, out=torch.empty((40, 200), device=disp.device))
    with pytest.raises(ValueError):
        gpu.reproject_points(disp.double(), Q)
    # host buffers
    host = pybicos.reproject(d, Q)
    assert host.dtype == np.float32 and np.array_equal(bits(host), bits(want["points"]))
    loose = restate(d, Q, ALLOW_NEGATIVE_Z)
    assert np.array_equal(bits(pybicos.reproject(d, Q, allow_negative_z=True, sentinel=False)),
                          bits(loose["points"]))
    # the C++ API, maps in host and in device memory
    _built()
    if not os.path.exists(REPROJECT_CPP):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "reproject.mk"],
                       check=True, capture_output=True)
    raw = tmp_path / "d.raw"
    raw.write_bytes(d.tobytes())
    prefix = str(tmp_path / "o")
    r = subprocess.run([REPROJECT_CPP, str(raw), "40", "200",
                        str(_lib.CV_32F if d.dtype == np.float32 else _lib.CV_16S),
                        str(F32_SENTINEL), prefix] + [repr(float(v)) for v in Q.ravel()],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    line = " ".join(str(int(v)) for v in want["counts"])
    assert r.stdout.split("\n")[:3] == ["host " + line, "dev " + line, "buf " + line]
    for form in ("host", "dev", "buf"):
        assert open(prefix + "." + form + ".pts", "rb").read() == want["points"].tobytes()
        assert open(prefix + "." + form + ".idx", "rb").read() == want["index"].tobytes()
    for form in ("host", "dev"):
        m = np.fromfile(prefix + "." + form + ".map", np.float32).reshape(40, 200, 3)
        assert np.array_equal(bits(m)[k], bits(want["map"])[k]) and np.isnan(m[~k]).all()


# ------------------------------------------------------------------------ CLI
@pytest.mark.parametrize("extra,flags", [([], 0), (["--allow-negative-z"], ALLOW_NEGATIVE_Z),
                                         (["-t", "0"], 0), (["-s", "0.2"], 0)],
                         ids=["default", "allow_negative_z", "int16", "subpixel"])
def test_cli_point_cloud(extra, flags, tmp_path):
    """bicos-cli -q: the .xyz bytes are the '%g' text of the restatement of the TIFF map the
    CLI wrote (no sentinel flag, as before), the skipped counts on stderr its classes"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    _built()
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(12, 40, 200)
    src = str(tmp_path / "in")
    _write_folder(src, L, R, False)
    out = str(tmp_path / "out" / "disp.png")
    os.makedirs(os.path.dirname(out))
    qf = tmp_path / "q.yml"
    qf.write_text(YAML.format(", ".join(repr(float(v)) for v in Q.ravel())))
    r = subprocess.run([CLI, src] + extra + ["-o", out, "-q", str(qf)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    d = read_tiff(str(tmp_path / "out" / "disp.tiff"))
    want = restate(d, Q, flags)
    assert want["counts"][0] > 0.3 * d.size
    assert open(str(tmp_path / "out" / "disp.xyz"), "rb").read() == xyz_text(want["points"])
    skipped = [ln for ln in r.stderr.split("\n") if ln.startswith("Skipped")]
    expect = []
    if want["counts"][2]:
        expect.append("Skipped %d points with non-finite fp values" % want["counts"][2])
    if want["counts"][3]:
        expect.append("Skipped %d points with negative Z values" % want["counts"][3])
    assert skipped == expect
