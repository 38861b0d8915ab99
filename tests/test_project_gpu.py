"""The projection on the GPU (libbicos_amd/csrc/project.hip; include/bicos_c.h, "projection")
against the numpy restatement of tests/project_ref.py, which tests/test_project_api.py checks
against a plain loop and hand-worked cases. Every comparison is exact: np.array_equal on the
integer outputs and on uint32 views of the floats. Every output lies inside a larger buffer that
is filled with a guard before the call, and nothing around the written range may change.
"""
import ctypes

import numpy as np
import pytest

from libbicos_amd import _lib
from tests import project_ref as ref
from tests.project_ref import bits

pytestmark = pytest.mark.gpu

INF = float("inf")
GUARD = {np.dtype(np.float32): -12345.0, np.dtype(np.int32): -7, np.dtype(np.uint8): 0xEE,
         np.dtype(np.uint16): 0xEEEE, np.dtype(np.uint32): 0xEEEEEEEE}
TAIL = 9  # guard elements on either side of every buffer


def spec(n, rows, cols, channels, img_dtype):
    return {"uv": (2 * n, np.float32), "depth": (n, np.float32), "cls": (n, np.uint8),
            "tex": (n * channels, img_dtype), "depth_map": (rows * cols, np.float32),
            "index_map": (rows * cols, np.int32), "counts": (5, np.uint32)}


def shaped(out, n, rows, cols, channels):
    """flat outputs -> the shapes of the restatement"""
    shape = {"uv": (n, 2), "tex": (n, channels), "depth_map": (rows, cols),
             "index_map": (rows, cols)}
    return {k: v.reshape(shape[k]) if k in shape else v for k, v in out.items()}


def run(handle, pts, cam, size, splat=0, tol=INF, image=None, fill=0, outputs=ref.OUTPUTS,
        pad=0, stream=None):
    """bicos_project_device on numpy inputs -> dict of numpy results. The points and every
    output are views TAIL elements into larger buffers (so 4-byte aligned and no more for the
    floats); the image's rows lie `pad` elements apart more than they are long."""
    import torch
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    rows, cols = size
    n = len(pts)
    outputs = [o for o in ref.OUTPUTS if o in outputs and (o != "tex" or image is not None)]
    big = torch.full((3 * n + 2 * TAIL,), 77.0, dtype=torch.float32, device=dev)
    big[TAIL:TAIL + 3 * n] = torch.from_numpy(np.ascontiguousarray(pts).reshape(-1)).to(dev)
    p_ptr = big.data_ptr() + 4 * TAIL
    img_ptr, depth, channels, pitch, img_dtype = None, 1, 1, 0, np.uint8
    if image is not None:
        img = np.asarray(image).reshape(rows, cols, -1)
        channels, img_dtype, depth = img.shape[2], img.dtype, img.itemsize
        pitch = cols * channels + pad
        host = np.full((rows, pitch), GUARD[np.dtype(img_dtype)] >> 1, img_dtype)
        host[:, :cols * channels] = img.reshape(rows, -1)
        t_img = torch.from_numpy(host).to(dev)
        img_ptr = t_img.data_ptr() if host.size else None
    sp = spec(n, rows, cols, channels, img_dtype)
    bufs = {}
    for o in outputs:
        size_o, dt = sp[o]
        host = np.full(size_o + 2 * TAIL, GUARD[np.dtype(dt)], dt)
        bufs[o] = torch.from_numpy(host.view(np.int32 if dt == np.uint32 else dt)).to(dev)

    def ptr(o):
        if o not in bufs:
            return None
        return bufs[o].data_ptr() + TAIL * bufs[o].element_size()
    r, tt, k, d, nd = _lib.project_camera(*cam)
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    rc = L.bicos_project_device(handle, p_ptr, n, r, tt, k, d, nd, rows, cols, splat, tol, img_ptr,
                                depth, channels, pitch, fill, *[ptr(o) for o in ref.OUTPUTS],
                                s.cuda_stream)
    _lib.check(rc, "bicos_project_device")
    s.synchronize()
    out = {}
    for o in outputs:
        size_o, dt = sp[o]
        h = bufs[o].cpu().numpy().view(dt)
        g = np.array([GUARD[np.dtype(dt)]], dt)[0]
        assert (h[:TAIL] == g).all() and (h[TAIL + size_o:] == g).all(), o + ": guard changed"
        out[o] = h[TAIL:TAIL + size_o]
    assert (big[:TAIL] == 77.0).all() and (big[TAIL + 3 * n:] == 77.0).all()
    return shaped(out, n, rows, cols, channels)


def check(got, want):
    """every output present in `got` against the restatement `want`, bit for bit"""
    assert got, "no output"
    for o, g in got.items():
        w = want[o]
        assert g.shape == w.shape, o
        if g.dtype == np.float32:
            assert np.array_equal(bits(g), bits(w)), o
        else:
            assert np.array_equal(g, w), o


def border_points(K, rows, cols, z=2.0):
    """points that an unmoved, undistorted camera K sees exactly on every corner and edge pixel
    and half a pixel around them (u = -0.5 is inside, u = cols - 0.5 is not)"""
    us = sorted({-0.75, -0.5, 0.0, 0.25, cols - 1.0, cols - 0.75, cols - 0.5, (cols - 1) / 2.0})
    vs = sorted({-0.75, -0.5, 0.0, 0.25, rows - 1.0, rows - 0.75, rows - 0.5, (rows - 1) / 2.0})
    p = [((u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z) for v in vs for u in us]
    return np.array(p, np.float32)


def case(count, rows, cols, nd=0, moved=True, channels=1, dtype=np.uint8, seed=0, borders=False):
    K, D, R, t = ref.rig(rows, cols, nd, moved)
    pts = ref.cloud(count, rows, cols, K, seed)
    if borders:
        pts = np.concatenate([pts, border_points(K, rows, cols), border_points(K, rows, cols, 1.5)])
    return pts, (K, D, R, t), ref.picture(rows, cols, channels, dtype, seed)


def want_for(pts, cam, size, **kw):
    return ref.restate(pts, ref.camera(*cam), size, **kw)


# ------------------------------------------------------------------ counts and images
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 255, 257, 2049])
def test_counts(gpu, count):
    """no point, less than a wave, a wave and one more, a workgroup's row of lanes and more than
    two workgroups"""
    assert _lib.project_group() == 1024
    pts, cam, img = case(count, 48, 64)
    kw = dict(splat=1, tol=0.5, image=img, fill=9)
    want = want_for(pts, cam, (48, 64), **kw)
    assert int(want["counts"].sum()) == count
    if count >= 255:
        assert (want["counts"] > 0).all()  # every class occurs
    check(run(gpu._h, pts, cam, (48, 64), **kw), want)


@pytest.mark.parametrize("splat", [0, 1, 3])
@pytest.mark.parametrize("size", [(1, 1), (5, 7), (48, 64), (97, 131)])
def test_images_and_splats(gpu, size, splat):
    """the smallest image (every splat clipped to one pixel), splats wider than the image, points
    on every border and corner"""
    rows, cols = size
    pts, cam, img = case(257, rows, cols, moved=False, borders=True)
    kw = dict(splat=splat, tol=0.0, image=img, fill=3)
    want = want_for(pts, cam, size, **kw)
    cls = want["cls"][257:]
    assert (cls == ref.OUTSIDE).any() and (cls <= ref.OCCLUDED).any()
    check(run(gpu._h, pts, cam, size, **kw), want)


@pytest.mark.parametrize("tol", [0.0, 0.5, INF])
def test_tolerance(gpu, tol):
    pts, cam, img = case(2049, 48, 64)
    want = want_for(pts, cam, (48, 64), splat=1, tol=tol, image=img)
    assert (want["counts"][ref.OCCLUDED] == 0) == (tol == INF)
    check(run(gpu._h, pts, cam, (48, 64), splat=1, tol=tol, image=img), want)


def test_tolerance_orders_the_occluded_counts():
    """(what the three values of test_tolerance exercise: each hides strictly fewer)"""
    pts, cam, _ = case(2049, 48, 64)
    n = [int(want_for(pts, cam, (48, 64), splat=1, tol=t)["counts"][ref.OCCLUDED])
         for t in (0.0, 0.5, INF)]
    assert n[0] > n[1] > n[2] == 0


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_image_types_and_pitches(gpu, dtype, channels, pad):
    pts, cam, img = case(257, 48, 64, channels=channels, dtype=dtype, borders=True)
    fill = 255 if dtype == np.uint8 else 65535
    kw = dict(splat=1, tol=0.5, image=img, fill=fill)
    want = want_for(pts, cam, (48, 64), **kw)
    vis = want["cls"] == ref.VISIBLE
    assert vis.sum() > 20 and len(np.unique(want["tex"][vis])) > 20
    check(run(gpu._h, pts, cam, (48, 64), pad=pad, **kw), want)


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("nd", [0, 4, 5, 8])
def test_distortion_models_and_poses(gpu, nd, moved):
    pts, cam, img = case(2049, 97, 131, nd=nd, moved=moved)
    kw = dict(splat=1, tol=0.5, image=img)
    want = want_for(pts, cam, (97, 131), **kw)
    assert (want["counts"] > 0).all()
    check(run(gpu._h, pts, cam, (97, 131), **kw), want)


def test_the_models_differ():
    """(what test_distortion_models_and_poses exercises: every coefficient group moves pixels)"""
    uv = []
    for nd in (0, 4, 5, 8):
        pts, cam, _ = case(2049, 97, 131, nd=nd)
        uv.append(bits(want_for(pts, cam, (97, 131))["uv"]))
    assert all((uv[i] != uv[i + 1]).any() for i in range(3))


@pytest.mark.parametrize("splat", [0, 1])
def test_4096_points_on_one_pixel(gpu, splat):
    """every point on the optical axis: one pixel takes every offer, a few depths many times
    over, so the smaller index has to win among equals"""
    rows, cols = 5, 7
    K = np.array([[50.0, 0, 3], [0, 50.0, 2], [0, 0, 1]])
    z = (1.0 + (np.arange(4096)[::-1] % 17) / 16.0).astype(np.float32)
    pts = np.stack([np.zeros_like(z), np.zeros_like(z), z], axis=1)
    cam = (K, None, None, None)
    want = want_for(pts, cam, (rows, cols), splat=splat, tol=0.0)
    first_nearest = int(np.flatnonzero(z == z.min())[0])
    assert want["index_map"][2, 3] == first_nearest and first_nearest > 0
    assert want["counts"].tolist() == [int((z == z.min()).sum()), int((z != z.min()).sum()), 0, 0, 0]
    assert (want["index_map"] >= 0).sum() == (2 * splat + 1) ** 2
    check(run(gpu._h, pts, cam, (rows, cols), splat=splat, tol=0.0), want)


# ---------------------------------------------------------------- the launch plans
@pytest.mark.parametrize("outputs", [
    ("uv", "depth", "cls", "tex", "counts"),  # no z-buffer: one launch
    ("counts",),
    ("tex",),
    ("depth_map", "index_map"),               # maps only: no resolve of the points
    ("index_map",),
    ("depth_map", "cls"),
], ids="-".join)
def test_output_subsets_without_an_occlusion_test(gpu, outputs):
    pts, cam, img = case(2049, 48, 64)
    kw = dict(splat=1, tol=INF, image=img)
    want = want_for(pts, cam, (48, 64), **kw)
    needs_z = "depth_map" in outputs or "index_map" in outputs
    # without a z-buffer the stage needs nothing of an engine
    got = run(gpu._h if needs_z else None, pts, cam, (48, 64), outputs=outputs, **kw)
    assert set(got) == set(outputs)
    check(got, want)


@pytest.mark.parametrize("outputs", [
    ("cls",), ("uv", "cls"), ("depth", "counts"), ("tex",), ("uv", "depth", "cls", "tex", "counts"),
], ids="-".join)
def test_output_subsets_with_an_occlusion_test(gpu, outputs):
    """uv and depth asked for or not: the class and the texture are the same"""
    pts, cam, img = case(2049, 48, 64)
    kw = dict(splat=1, tol=0.25, image=img, fill=200)
    got = run(gpu._h, pts, cam, (48, 64), outputs=outputs, **kw)
    assert set(got) == set(outputs)
    check(got, want_for(pts, cam, (48, 64), **kw))


def test_empty_image(gpu):
    """no pixel: every point in front of the camera is outside"""
    pts, cam, _ = case(257, 48, 64)
    for size in ((0, 64), (48, 0)):
        want = want_for(pts, cam, size, splat=1, tol=0.0)
        assert want["counts"][ref.VISIBLE] == 0 and want["counts"][ref.OUTSIDE] > 0
        check(run(gpu._h, pts, cam, size, splat=1, tol=0.0), want)


def test_no_points_still_fills_the_maps(gpu):
    pts = np.zeros((0, 3), np.float32)
    cam = ref.rig(5, 7)
    got = run(gpu._h, pts, cam, (5, 7), tol=0.0)
    assert got["counts"].tolist() == [0] * 5
    assert (bits(got["depth_map"]) == 0x7FC00000).all() and (got["index_map"] == -1).all()


def test_same_call_twice_gives_the_same_bytes(gpu):
    pts, cam, img = case(2049, 48, 64)
    kw = dict(splat=3, tol=0.5, image=img)
    a, b = (run(gpu._h, pts, cam, (48, 64), **kw) for _ in range(2))
    for o in a:
        assert a[o].tobytes() == b[o].tobytes(), o


def test_non_default_stream(gpu):
    import torch
    pts, cam, img = case(2049, 97, 131, nd=5)
    kw = dict(splat=1, tol=0.5, image=img)
    got = run(gpu._h, pts, cam, (97, 131), stream=torch.cuda.Stream(), **kw)
    check(got, want_for(pts, cam, (97, 131), **kw))


# ------------------------------------------------------------------- the layers
@pytest.mark.parametrize("channels,dtype,pad", [(1, np.uint8, 0), (3, np.uint16, 7)])
def test_host_entry(gpu, channels, dtype, pad):
    """host buffers with guards, a pitched host image"""
    L = _lib.lib()
    rows, cols, n = 48, 64, 257
    pts, cam, img = case(n, rows, cols, nd=8, channels=channels, dtype=dtype)
    want = want_for(pts, cam, (rows, cols), splat=1, tol=0.5, image=img, fill=7)
    pitch = cols * channels + pad
    himg = np.zeros((rows, pitch), dtype)
    himg[:, :cols * channels] = img.reshape(rows, -1)
    sp = spec(n, rows, cols, channels, dtype)
    bufs = {o: np.full(sp[o][0] + 2 * TAIL, GUARD[np.dtype(sp[o][1])], sp[o][1])
            for o in ref.OUTPUTS}
    r, tt, k, d, nd = _lib.project_camera(*cam)
    rc = L.bicos_project_host(None, pts.ctypes.data, n, r, tt, k, d, nd, rows, cols, 1, 0.5,
                              himg.ctypes.data, himg.itemsize, channels, pitch, 7,
                              *[bufs[o].ctypes.data + TAIL * bufs[o].itemsize for o in ref.OUTPUTS])
    _lib.check(rc, "bicos_project_host")
    got = {}
    for o in ref.OUTPUTS:
        h, size_o = bufs[o], sp[o][0]
        g = np.array([GUARD[h.dtype]], h.dtype)[0]
        assert (h[:TAIL] == g).all() and (h[TAIL + size_o:] == g).all(), o
        got[o] = h[TAIL:TAIL + size_o]
    check(shaped(got, n, rows, cols, channels), want)


def test_pybicos_project(gpu):
    import pybicos
    pts, cam, img = case(257, 48, 64, nd=4, channels=3)
    K, D, R, t = cam
    want = want_for(pts, cam, (48, 64), splat=2, tol=0.5, image=img, fill=1)
    got = pybicos.project(pts, K, D=D, R=R, t=t, splat=2, tol=0.5, image=img, fill=1,
                          outputs=ref.OUTPUTS)
    check(got, want)
    got = pybicos.project(pts, K, (48, 64), D=D, R=R, t=t)  # the defaults: no z-buffer
    assert set(got) == {"uv", "depth", "cls", "counts"}
    check(got, want_for(pts, cam, (48, 64)))


def test_engine_project(gpu):
    """torch tensors: a strided image view, caller-provided outputs, the default outputs"""
    import torch
    pts, cam, img = case(2049, 48, 64, nd=5, channels=3)
    K, D, R, t = cam
    kw = dict(splat=1, tol=0.5, fill=4)
    want = want_for(pts, cam, (48, 64), image=img, **kw)
    wide = torch.zeros((48, 80, 3), dtype=torch.uint8, device="cuda")
    wide[:, 9:73] = torch.from_numpy(img).cuda()
    view = wide[:, 9:73]
    assert not view.is_contiguous()
    tp = torch.from_numpy(pts).cuda()
    res = gpu.project(tp, K, D=D, R=R, t=t, image=view, outputs=ref.OUTPUTS, **kw)
    torch.cuda.synchronize()
    got = {o: v.cpu().numpy() for o, v in res.items()}
    got["counts"] = got["counts"].view(np.uint32)
    check(got, want)
    # caller-provided outputs are written in place and returned
    mine = dict(cls=torch.full((2049,), 99, dtype=torch.uint8, device="cuda"),
                index_map=torch.full((48, 64), -5, dtype=torch.int32, device="cuda"))
    res = gpu.project(tp, K, D=D, R=R, t=t, image=view, out=mine, **kw)
    assert set(res) == {"cls", "index_map"} and res["cls"] is mine["cls"]
    torch.cuda.synchronize()
    check({o: v.cpu().numpy() for o, v in mine.items()}, want)
    # grey [H, W], the defaults
    grey = torch.from_numpy(np.ascontiguousarray(img[:, :, 1])).cuda()
    res = gpu.project(tp, K, D=D, R=R, t=t, image=grey)
    assert set(res) == {"uv", "depth", "cls", "tex"}
    torch.cuda.synchronize()
    check({o: v.cpu().numpy() for o, v in res.items()},
          want_for(pts, cam, (48, 64), image=img[:, :, 1]))
    with pytest.raises(ValueError):
        gpu.project(tp, K, (48, 64), outputs=("tex",))
    with pytest.raises(ValueError):
        gpu.project(tp, K, (48, 64), out=dict(cls=torch.zeros(5, dtype=torch.uint8, device="cuda")))


def test_mesh_then_project_textures_each_vertex(gpu):
    """match -> mesh -> project into the rectified left camera itself (R = I, t = 0, K from Q):
    vertex i lands on its own pixel, so tex[i] is the image at index[i], and index_map is the
    inverse of index"""
    import torch
    from libbicos_amd import device
    from libbicos_amd.synthetic import stereo_stack
    from tests.normals_ref import rig_q
    L, R = stereo_stack(12, 40, 200)
    rows, cols = L.shape[1:]
    disp, _ = gpu.match(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(),
                        device.MatchConfig(nxcorr_threshold=0.5, subpixel_step=0.25))
    f = 2000.0
    q = rig_q(rows, cols, f)
    points, tris, index, _, stats = gpu.mesh(disp, q, with_index=True)
    assert stats["kept"] > 1000 and stats["triangles"] > 1000
    K = np.array([[f, 0, (cols - 1) / 2.0], [0, f, (rows - 1) / 2.0], [0, 0, 1]])
    img = ref.picture(rows, cols, 1, np.uint8)
    res = gpu.project(points, K, image=torch.from_numpy(img).cuda(), tol=0.0, outputs=ref.OUTPUTS)
    torch.cuda.synchronize()
    got = {o: v.cpu().numpy() for o, v in res.items()}
    got["counts"] = got["counts"].view(np.uint32)
    pts, idx = points.cpu().numpy(), index.cpu().numpy().astype(np.int64)
    check(got, want_for(pts, (K, None, None, None), (rows, cols), tol=0.0, image=img))
    assert got["counts"].tolist() == [len(pts), 0, 0, 0, 0]
    assert np.array_equal(got["tex"][:, 0], img.reshape(-1)[idx])
    inverse = np.full(rows * cols, -1, np.int32)
    inverse[idx] = np.arange(len(idx), dtype=np.int32)
    assert np.array_equal(got["index_map"].reshape(-1), inverse)
