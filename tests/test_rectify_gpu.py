"""Rectification on the GPU (include/bicos_c.h, "rectification"): rectify.hip bit for bit
against the numpy restatement tests/rectify_ref.py. Every output buffer is prefilled with a
guard value; the padding of pitched outputs and the bytes behind them must keep it.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import rectify_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECTIFY_CPP = os.path.join(ROOT, "tests", "cpp", "rectify_cpp")

GUARD = 0xA5
DTYPES = {"u8": np.uint8, "u16": np.uint16}
F32 = np.float32


# ------------------------------------------------------------------------ the maps
@functools.lru_cache(maxsize=None)
def make_maps(kind, rows, cols, sr, sc):
    """(map_x, map_y) float32 [rows, cols] into a source of sr x sc; never modified."""
    iu, iv = ref.identity_maps(rows, cols)
    rng = np.random.default_rng(rows * 1000 + cols)
    if kind == "identity":
        mx, my = iu, iv
    elif kind == "half":  # half-pixel shifts, leaving the frame on two sides
        mx, my = iu + F32(0.5), iv - F32(1.5)
    elif kind == "rot":  # a few degrees of rotation with radial distortion
        K, D, R, P = ref.camera(sr, sc, degrees=3.0)
        P = P.copy()
        P[0, 0] *= rows / sr * 1.05  # (the output grid spans about the source)
        P[1, 1] *= rows / sr * 1.05
        P[0, 2], P[1, 2] = cols / 2, rows / 2
        mx, my = ref.maps(K, D, R, P, rows, cols)
    elif kind == "uniform":  # no locality at all
        mx = rng.uniform(-3, sc + 3, (rows, cols)).astype(F32)
        my = rng.uniform(-3, sr + 3, (rows, cols)).astype(F32)
    elif kind == "special":
        vals = np.array([-1, -0.5, -1e-9, 0, sc - 1, sc - 0.5, sc, sr - 1, sr - 0.5, sr, np.nan,
                         np.inf, -np.inf, 1e30, -1e30, 0.25, 1.75], F32)
        # every special value in map_x against every one in map_y, then ordinary pixels
        gx, gy = np.meshgrid(vals, vals)
        mx = rng.uniform(0, sc - 1, rows * cols).astype(F32)
        my = rng.uniform(0, sr - 1, rows * cols).astype(F32)
        k = min(gx.size, rows * cols)
        mx[:k], my[:k] = gx.ravel()[:k], gy.ravel()[:k]
        mx, my = mx.reshape(rows, cols), my.reshape(rows, cols)
    else:
        raise KeyError(kind)
    mx, my = np.ascontiguousarray(mx, F32), np.ascontiguousarray(my, F32)
    mx.setflags(write=False)
    my.setflags(write=False)
    return mx, my


@functools.lru_cache(maxsize=None)
def make_case(kind, dt, n, rows, cols, sr, sc, border):
    """(stack, map_x, map_y, want, want_valid): the restatement's answer, computed once."""
    s = ref.images(n, sr, sc, DTYPES[dt], seed=n + sr)
    mx, my = make_maps(kind, rows, cols, sr, sc)
    want, valid = ref.remap(s, mx, my, border)
    for a in (s, want, valid):
        a.setflags(write=False)
    return s, mx, my, want, valid


# ------------------------------------------------------------- the C entry on raw buffers
def _strided(buf, off, shape, strides_elems):
    isz = buf.dtype.itemsize
    return np.lib.stride_tricks.as_strided(buf[off:], shape, [s * isz for s in strides_elems])


def device_rectify(s, mx, my, border=0, *, src_rp=None, src_pp=None, dst_rp=None, dst_pp=None,
                   map_rp=None, dst_off=0, want_valid=True, engine=None, stream=None):
    """bicos_rectify_device on buffers laid out as asked (pitches in elements, map_rp in floats,
    dst_off elements before the first output pixel). Returns (out, valid) after checking that
    every byte outside the output pixels still holds the guard."""
    import torch
    n, sr, sc = s.shape
    rows, cols = mx.shape
    dt = s.dtype
    src_rp = src_rp or sc
    src_pp = src_pp or src_rp * sr
    dst_rp = dst_rp or cols
    dst_pp = dst_pp or dst_rp * rows
    map_rp = map_rp or cols
    guard = np.array([GUARD] * dt.itemsize, np.uint8).view(dt)[0]
    hsrc = np.full(n * src_pp + 8, 77, dt)
    _strided(hsrc, 0, (n, sr, sc), (src_pp, src_rp, 1))[...] = s
    hmaps = []
    for m in (mx, my):
        h = np.full(rows * map_rp + 8, np.nan, F32)  # (padding that would read as "outside")
        _strided(h, 0, (rows, cols), (map_rp, 1))[...] = m
        hmaps.append(h)
    hdst = np.full(dst_off + n * dst_pp + 16, guard, dt)
    hval = np.full(rows * cols + 16, GUARD, np.uint8)

    def up(a):
        return torch.from_numpy(a.view(np.uint8).copy()).cuda()

    dsrc, dmx, dmy, ddst, dval = up(hsrc), up(hmaps[0]), up(hmaps[1]), up(hdst), up(hval)
    L = _lib.lib()
    st = stream if stream is not None else torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())  # the uploads
    rc = L.bicos_rectify_device(
        engine, dsrc.data_ptr(), n, sr, sc, src_rp, src_pp, dt.itemsize, dmx.data_ptr(),
        dmy.data_ptr(), 4 * map_rp if map_rp != cols else 0, rows, cols,
        ddst.data_ptr() + dst_off * dt.itemsize, dst_rp, dst_pp, border,
        dval.data_ptr() if want_valid else None, st.cuda_stream)
    _lib.check(rc, "bicos_rectify_device")
    st.synchronize()
    got_buf = ddst.cpu().numpy().view(dt).copy()
    view = _strided(got_buf, dst_off, (n, rows, cols), (dst_pp, dst_rp, 1))
    out = view.copy()
    view[...] = guard
    assert (got_buf == guard).all(), "bytes outside the output pixels were written"
    vbuf = dval.cpu().numpy()
    assert (vbuf[rows * cols:] == GUARD).all()
    if not want_valid:
        assert (vbuf == GUARD).all()
        return out, None
    return out, vbuf[:rows * cols].reshape(rows, cols)


def check(kind, dt, n, rows, cols, sr, sc, border=0, **layout):
    s, mx, my, want, want_valid = make_case(kind, dt, n, rows, cols, sr, sc, border)
    out, valid = device_rectify(s, mx, my, border, **layout)
    assert out.dtype == want.dtype and np.array_equal(out, want)
    if valid is not None:
        assert np.array_equal(valid, want_valid)
    return want, want_valid


def tile():
    return _lib.rectify_tile()


# ----------------------------------------------------------------- shapes and layouts
@pytest.mark.parametrize("kind", ["identity", "half", "rot", "uniform", "special"])
@pytest.mark.parametrize("dt", ["u8", "u16"])
@pytest.mark.parametrize("border", [0, 7])
def test_remap_37x70_from_50x91(gpu, kind, dt, border):
    want, valid = check(kind, dt, 3, 37, 70, 50, 91, border)
    if kind == "rot":  # the case is a real warp: most pixels inside, some not
        assert 0.5 < valid.mean() < 1.0
    if kind == "special":
        assert valid[0, :17].tolist() != [1] * 17


def test_identity_is_byte_exact(gpu):
    for dt in ("u8", "u16"):
        s, mx, my, want, valid = make_case("identity", dt, 2, 50, 91, 50, 91, 0)
        assert np.array_equal(want, s) and valid.all()  # the restatement's own property
        out, v = device_rectify(s, mx, my)
        assert np.array_equal(out, s) and v.all()
        assert s.min() == 0 and s.max() == np.iinfo(s.dtype).max


@pytest.mark.parametrize("dr", [-1, 0, 1])
@pytest.mark.parametrize("dc", [-1, 0, 1])
def test_sizes_around_one_tile(gpu, dr, dc):
    tr, tc = tile()
    check("uniform", "u8", 2, tr + dr, tc + dc, 19, 40, 7)
    check("rot", "u16", 2, tr + dr, tc + dc, 19, 40, 0)


def test_more_than_one_tile_each_way(gpu):
    tr, tc = tile()
    check("rot", "u8", 2, 2 * tr + 3, 2 * tc + 5, 21, 300, 7)


@pytest.mark.parametrize("cols", [1, 3, 5, 67])
@pytest.mark.parametrize("dt", ["u8", "u16"])
def test_narrow_outputs(gpu, cols, dt):
    check("uniform", dt, 2, 11, cols, 13, 9, 7)
    check("rot", dt, 1, 1, cols, 5, 1, 0)  # one row out, one column in


@pytest.mark.parametrize("n", [1, 2, 33, 65])
@pytest.mark.parametrize("dt", ["u8", "u16"])
def test_stack_sizes(gpu, n, dt):
    check("rot", dt, n, 19, 45, 23, 31, 7)


LAYOUTS = {
    "dense": dict(),
    "padded_rows": dict(src_rp=96, dst_rp=76),
    "padded_planes": dict(src_pp=91 * 50 + 13, dst_pp=70 * 37 + 6),
    "padded_maps": dict(map_rp=75),
    "all_padded": dict(src_rp=93, src_pp=93 * 50 + 5, dst_rp=72, dst_pp=72 * 38, map_rp=71),
    "odd_row_pitch": dict(dst_rp=71),           # no dword path for u8
    "odd_plane_pitch": dict(dst_pp=70 * 37 + 1),
    "unaligned_base": dict(dst_off=1),
    "unaligned_base_u16_dword": dict(dst_off=2, dst_rp=72),
}


@pytest.mark.parametrize("layout", list(LAYOUTS), ids=list(LAYOUTS))
@pytest.mark.parametrize("dt", ["u8", "u16"])
def test_pitches(gpu, layout, dt):
    check("rot", dt, 3, 37, 70, 50, 91, 7, **LAYOUTS[layout])
    check("uniform", dt, 3, 37, 70, 50, 91, 0, **LAYOUTS[layout])


def test_aligned_and_ragged_widths_take_both_store_paths(gpu):
    for cols in (64, 66, 68):  # valid's dword path needs cols % 4 == 0
        check("uniform", "u8", 2, 9, cols, 12, 33, 7)
        check("uniform", "u16", 2, 9, cols, 12, 33, 7, dst_rp=cols + 4)


def test_without_valid(gpu):
    check("rot", "u8", 3, 37, 70, 50, 91, 7, want_valid=False)
    check("rot", "u16", 3, 37, 70, 50, 91, 7, want_valid=False)


def test_engine_null_and_given(gpu):
    check("rot", "u8", 3, 37, 70, 50, 91, 7, engine=None)
    check("rot", "u8", 3, 37, 70, 50, 91, 7, engine=gpu._h)


def test_two_streams_on_one_engine(gpu):
    import torch
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(2):
        check("rot", "u8", 33, 37, 70, 50, 91, 7, engine=gpu._h, stream=a)
        check("uniform", "u16", 33, 37, 70, 50, 91, 0, engine=gpu._h, stream=b)


def test_extreme_planes(gpu):
    """constant planes of 0 and of the top level stay constant inside, whatever the fractions"""
    import torch
    for dt, top in ((np.uint8, 255), (np.uint16, 65535)):
        s = np.zeros((3, 50, 91), dt)
        s[1], s[2, ::2] = top, top
        mx, my = make_maps("rot", 37, 70, 50, 91)
        want, wv = ref.remap(s, mx, my, top)
        out, v = device_rectify(s, mx, my, top)
        assert np.array_equal(out, want) and np.array_equal(v, wv)
        assert (out[1] == top).all() and out[0].min() == 0


# -------------------------------------------------------------------- the maps kernel
def _maps_device(gpu, K, D, R, P, rows, cols):
    import torch
    k, d, nd, r, p, p_cols, rows, cols = _lib.rectify_camera(K, D, R, P, (rows, cols))
    buf = torch.full((2, rows * cols + 16), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, rows * cols:] = 123.0
    rc = _lib.lib().bicos_rectify_maps_device(k, d, nd, r, p, p_cols, rows, cols,
                                              buf[0].data_ptr(), buf[1].data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "bicos_rectify_maps_device")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:, rows * cols:] == 123.0).all()
    return h[0, :rows * cols].reshape(rows, cols), h[1, :rows * cols].reshape(rows, cols)


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("nd", [0, 4, 5, 8])
@pytest.mark.parametrize("rot", [False, True], ids=["R_null", "R_rotation"])
@pytest.mark.parametrize("p_cols", [3, 4])
def test_maps_kernel(gpu, nd, rot, p_cols):
    tr, tc = tile()
    for rows, cols in ((1, 1), (37, 70), (tr + 1, tc + 1)):
        K, D, R, P = ref.camera(rows, cols)
        D, R, P = D[:nd], (R if rot else None), P[:, :p_cols]
        wx, wy = ref.maps(K, D, R, P, rows, cols)
        gx, gy = _maps_device(gpu, K, D, R, P, rows, cols)
        assert _same_bits(gx, wx) and _same_bits(gy, wy)


def test_maps_that_are_not_finite_are_stored_as_they_come(gpu):
    """W = 0 on the line u + v = 4: infinities and NaNs, the restatement's own"""
    K = np.array([[10.0, 0, 4], [0, 10, 4], [0, 0, 1]])
    P = np.array([[1.0, 0, 0], [0, 1, 0], [0.25, 0.25, -0.25]])  # inverse row 2: (1, 1, -4), exact
    assert ref.inverse3(P)[0][6:] == [1, 1, -4]
    wx, wy = ref.maps(K, None, None, P, 9, 9)
    assert np.isnan(wx).any() and np.isfinite(wx).any()  # (0 * inf in the radial polynomial)
    gx, gy = _maps_device(gpu, K, None, None, P, 9, 9)
    assert _same_bits(gx, wx) and _same_bits(gy, wy)
    s = ref.images(2, 9, 9, np.uint8)
    want, wv = ref.remap(s, wx, wy, 7)
    out, v = device_rectify(s, gx, gy, 7)
    assert np.array_equal(out, want) and np.array_equal(v, wv)


# ----------------------------------------------------------------- through the layers
def test_engine_rectify_identity_then_match(gpu):
    import torch
    from libbicos_amd import device
    from libbicos_amd.synthetic import stereo_stack
    L, R = stereo_stack(8, 64, 96)
    tl, tr_ = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    iu, iv = ref.identity_maps(64, 96)
    mx, my = torch.from_numpy(iu).cuda(), torch.from_numpy(iv).cuda()
    rl, v = gpu.rectify(tl, mx, my, valid=True)
    rr = gpu.rectify(tr_, mx, my)
    cfg = device.MatchConfig(nxcorr_threshold=0.9)
    d0, c0 = gpu.match(tl, tr_, cfg)
    d1, c1 = gpu.match(rl, rr, cfg)  # the rectified stacks straight into the match
    torch.cuda.synchronize()
    assert np.array_equal(rl.cpu().numpy(), L) and np.array_equal(rr.cpu().numpy(), R)
    assert bool(v.all())
    assert np.array_equal(d0.cpu().numpy().view(np.uint8), d1.cpu().numpy().view(np.uint8))
    assert np.array_equal(c0.cpu().numpy().view(np.uint8), c1.cpu().numpy().view(np.uint8))


def test_engine_rectify_maps_equals_the_restatement(gpu):
    K, D, R, P = ref.camera(37, 70)
    mx, my = gpu.rectify_maps(K, D, R, P, (37, 70))
    wx, wy = ref.maps(K, D, R, P, 37, 70)
    assert _same_bits(mx.cpu().numpy(), wx) and _same_bits(my.cpu().numpy(), wy)


@pytest.mark.parametrize("dt", ["u8", "u16"])
def test_engine_rectify_strided_tensors_and_out(gpu, dt):
    import torch
    s, mx, my, want, wv = make_case("rot", dt, 3, 37, 70, 50, 91, 7)
    tdt = torch.uint8 if dt == "u8" else torch.int16
    big = torch.zeros((4, 52, 96), dtype=tdt, device="cuda")
    big[:3, 1:51, 2:93] = torch.from_numpy(np.array(s.view(np.int16) if dt == "u16" else s)).cuda()
    stack = big[:3, 1:51, 2:93]  # plane and row strides of the larger tensor
    maps = torch.full((2, 37, 80), float("nan"), device="cuda")
    maps[0, :, :70] = torch.from_numpy(np.array(mx)).cuda()
    maps[1, :, :70] = torch.from_numpy(np.array(my)).cuda()
    outbig = torch.full((3, 40, 75), 0x25, dtype=tdt, device="cuda")
    out = outbig[:, 2:39, 3:73]
    val = torch.full((37, 70), 9, dtype=torch.uint8, device="cuda")
    r, v = gpu.rectify(stack, maps[0, :, :70], maps[1, :, :70], border=7, out=out, valid=val)
    torch.cuda.synchronize()
    assert r is out and v is val
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint16) if dt == "u16" else got, want)
    assert np.array_equal(val.cpu().numpy(), wv)
    outbig[:, 2:39, 3:73] = 0x25
    assert bool((outbig == 0x25).all())
    with pytest.raises(ValueError):
        gpu.rectify(stack, maps[0, :, :70], maps[1, :36, :70])
    with pytest.raises(_lib.BicosError, match="border"):
        gpu.rectify(stack, maps[0, :, :70], maps[1, :, :70], border=70000)


def test_shift_and_back(gpu):
    """a stack shifted by an integer map and rectified back is the original where valid"""
    import torch
    s = ref.images(4, 30, 45, np.uint8, seed=9)
    t = torch.from_numpy(s).cuda()
    iu, iv = ref.identity_maps(30, 45)
    fwd = [torch.from_numpy(iu + F32(3)).cuda(), torch.from_numpy(iv - F32(2)).cuda()]
    back = [torch.from_numpy(iu - F32(3)).cuda(), torch.from_numpy(iv + F32(2)).cuda()]
    shifted, v1 = gpu.rectify(t, fwd[0], fwd[1], border=200, valid=True)
    again, v2 = gpu.rectify(shifted, back[0], back[1], border=100, valid=True)
    torch.cuda.synchronize()
    # valid of the way back says the tap lay in the shifted frame; the pixel there was itself
    # a real one iff its own source lay in the original frame
    # shifted(v, u) = s(v - 2, u + 3), real for v >= 2 and u < 42; again(v, u) =
    # shifted(v + 2, u - 3), a tap in the frame for v < 28 and u >= 3 -- and always a real one
    real = np.zeros((30, 45), bool)
    real[2:, :42] = True
    ok = np.zeros((30, 45), bool)
    ok[:28, 3:] = True
    assert np.array_equal(v1.cpu().numpy() == 1, real)
    assert np.array_equal(v2.cpu().numpy() == 1, ok)
    again, shifted = again.cpu().numpy(), shifted.cpu().numpy()
    assert np.array_equal(again[:, ok], s[:, ok])
    assert (again[:, ~ok] == 100).all() and (shifted[:, ~real] == 200).all()


@pytest.mark.parametrize("dt", ["u8", "u16"])
def test_host_entries_equal_the_device_result(gpu, dt):
    from libbicos_amd import pybicos
    s, mx, my, want, wv = make_case("rot", dt, 5, 37, 70, 50, 91, 7)
    out, v = pybicos.rectify(list(s), mx, my, border=7)
    assert out.dtype == s.dtype and np.array_equal(out, want) and np.array_equal(v, wv)
    out, v = pybicos.rectify(s, mx, my, border=7)
    assert np.array_equal(out, want) and np.array_equal(v, wv)
    # bicos_rectify_host with steps and a map pitch of its own, on a private engine
    n, d = 5, s.dtype.itemsize
    src = np.full((n, 50, 100), 3, s.dtype)
    src[:, :, :91] = s
    guard = np.array([GUARD] * d, np.uint8).view(s.dtype)[0]
    dst = np.full((n, 37, 80), guard, s.dtype)
    maps = np.full((2, 37, 75), np.nan, F32)
    maps[0, :, :70], maps[1, :, :70] = mx, my
    valid = np.full((37, 70), GUARD, np.uint8)
    ps = (ctypes.c_void_p * n)(*[src[t].ctypes.data for t in range(n)])
    pd = (ctypes.c_void_p * n)(*[dst[t].ctypes.data for t in range(n)])
    rc = _lib.lib().bicos_rectify_host(gpu._h, ps, n, 50, 91, 100 * d, d, maps[0].ctypes.data,
                                       maps[1].ctypes.data, 75 * 4, 37, 70, pd, 80 * d, 7,
                                       valid.ctypes.data)
    _lib.check(rc, "bicos_rectify_host")
    assert np.array_equal(dst[:, :, :70], want) and np.array_equal(valid, wv)
    assert (dst[:, :, 70:] == guard).all()


@pytest.mark.parametrize("dt", ["u8", "u16"])
def test_cpp_api(gpu, dt, tmp_path):
    """BICOS::rectify in host memory, on planar device views and on separate device images, and
    BICOS::rectify_maps in both memories (tests/cpp/rectify_cpp.cpp, built by build())"""
    assert os.path.exists(RECTIFY_CPP), "tests/cpp/rectify_cpp is built by __graft_entry__.build()"
    s, mx, my, want, wv = make_case("rot", dt, 5, 37, 70, 50, 91, 7)
    K, D, R, P = ref.camera(37, 70)
    s.tofile(tmp_path / "stack.raw")
    mx.tofile(tmp_path / "mx.raw")
    my.tofile(tmp_path / "my.raw")
    np.concatenate([K.ravel(), D, R.ravel(), P.ravel()]).astype(np.float64).tofile(tmp_path / "cam.raw")
    out = str(tmp_path / "out")
    r = subprocess.run([RECTIFY_CPP, str(tmp_path / "stack.raw"), "5", "50", "91",
                        "0" if dt == "u8" else "2", str(tmp_path / "mx.raw"),
                        str(tmp_path / "my.raw"), "37", "70", "7", str(tmp_path / "cam.raw"), out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for form in ("host", "planar", "separate"):
        got = np.fromfile(out + "." + form + ".stack", s.dtype).reshape(want.shape)
        assert np.array_equal(got, want), form
        assert np.array_equal(np.fromfile(out + "." + form + ".valid", np.uint8).reshape(wv.shape),
                              wv), form
    wx, wy = ref.maps(K, D, R, P, 37, 70)
    for form in ("host", "dev"):
        got = np.fromfile(out + ".maps." + form, np.float32).reshape(2, 37, 70)
        assert _same_bits(got[0], wx) and _same_bits(got[1], wy), form


def _yaml_matrix(name, m):
    m = np.atleast_2d(np.asarray(m, np.float64))
    return "%s: !!opencv-matrix\n   rows: %d\n   cols: %d\n   dt: d\n   data: [ %s ]\n" % (
        name, m.shape[0], m.shape[1], ", ".join(repr(float(v)) for v in m.ravel()))


@pytest.mark.parametrize("dt", ["u8", "u16"])
def test_cli_rectify(gpu, dt, tmp_path):
    """bicos-cli --rectify with D = 0, R = I, P = [M | 0] (an ideal camera; powers of two, so
    every step is exact and the maps are the identity grid): the same disparity TIFF and point
    cloud as without the option; a rotated camera changes the map"""
    from libbicos_amd.synthetic import stereo_stack
    from tests.test_cli import CLI, Q, _built, _write_folder
    _built()
    H, W = 48, 64
    L, R = stereo_stack(10, H, W, DTYPES[dt])
    two = dt == "u16"  # (16-bit images are kept only with two folders)
    src = str(tmp_path / "in")
    _write_folder(src, L, R, two)
    folders = [os.path.join(src, "left"), os.path.join(src, "right")] if two else [src]
    M = np.array([[64.0, 0, 32], [0, 64, 16], [0, 0, 1]])
    P = np.hstack([M, np.zeros((3, 1))])
    text = "%YAML:1.0\n---\n"
    for side in "12":
        text += _yaml_matrix("M" + side, M) + _yaml_matrix("D" + side, np.zeros((1, 5)))
        text += _yaml_matrix("R" + side, np.eye(3)) + _yaml_matrix("P" + side, P)
    plain = tmp_path / "rig.yml"
    plain.write_text(text)
    withq = tmp_path / "rigq.yml"
    withq.write_text(text + _yaml_matrix("Q", Q))
    qf = tmp_path / "q.yml"
    qf.write_text("%YAML:1.0\n---\n" + _yaml_matrix("Q", Q))

    def run(tag, extra):
        out = tmp_path / tag / "disp.png"
        os.makedirs(out.parent)
        r = subprocess.run([CLI] + folders + ["--limited", "-o", str(out)] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr + r.stdout
        xyz = out.with_suffix(".xyz")
        return out.with_suffix(".tiff").read_bytes(), xyz.read_bytes() if xyz.exists() else None, r

    base, base_xyz, _ = run("base", ["-q", str(qf)])
    got, got_xyz, r = run("rect", ["--rectify", str(plain), "-q", str(qf)])
    assert "Rectified" in r.stdout
    assert got == base and got_xyz == base_xyz and base_xyz
    got, got_xyz, _ = run("rectq", ["--rectify", str(withq)])  # the file's own Q
    assert got == base and got_xyz == base_xyz
    _, none_xyz, _ = run("noq", ["--rectify", str(plain)])
    assert none_xyz is None
    # a camera rotated about its axis is not the identity
    a = np.deg2rad(5.0)
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    turned = tmp_path / "turned.yml"
    turned.write_text(text.replace(_yaml_matrix("R1", np.eye(3)), _yaml_matrix("R1", rot)))
    other, _, _ = run("turned", ["--rectify", str(turned)])
    assert other != base
    # errors
    bad = tmp_path / "bad.yml"
    bad.write_text(text.replace("M2:", "N2:"))
    r = subprocess.run([CLI] + folders + ["--rectify", str(bad)], capture_output=True, text=True)
    assert r.returncode == 1 and "M2" in r.stderr
    r = subprocess.run([CLI] + folders + ["--rectify", str(tmp_path / "none.yml")],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "does not exist" in r.stderr


def test_pybicos_rectify_maps(gpu):
    from libbicos_amd import pybicos
    K, D, R, P = ref.camera(37, 70)
    mx, my = pybicos.rectify_maps(K, D[:5], R, P[:, :3], (37, 70))
    wx, wy = ref.maps(K, D[:5], R, P[:, :3], 37, 70)
    assert _same_bits(mx, wx) and _same_bits(my, wy)
