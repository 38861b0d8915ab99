"""Stack pooling and the pyramid match on the GPU (include/bicos_c.h, "stack pooling" and
"pyramid match"): bicos_pool_device byte for byte against the numpy restatement of
tests/test_pool_api.py -- dense stacks across workgroup boundaries and both remainders, views of
larger buffers at every base and pitch residue with their guards, both kernels --, the host and
pybicos paths against the device path, and the pyramid match against the four public calls it is
defined as.
"""
import functools

import numpy as np
import pytest

from libbicos_amd import _lib
from libbicos_amd.synthetic import random_stack, stereo_stack
from tests import view_cases as V
from tests.test_pool_api import pool_ref, pyramid_window_ref
from tests.test_range_gpu import dev, host, same

pytestmark = pytest.mark.gpu

ALL_SCALES = (2, 3, 4, 5, 6, 7, 8)  # every instantiation of the kernels
WINDOW = (0, 63)


def as_unsigned(a, dt):
    """a downloaded stack as the dtype it stands for (torch holds uint16 bits in int16)"""
    return a.view(np.uint16) if np.dtype(dt) == np.uint16 else a


# ------------------------------------------------------------------- dense stacks
def inputs(n, rows, cols, dt, seed):
    """random data; an all-maximum stack; alternating 0 / maximum columns, where every block sum
    is an exact tie (even scales) or a multiple of the maximum"""
    top = np.iinfo(dt).max
    yield "random", random_stack(n, rows, cols, dt, seed=seed, maxval=top)
    yield "maximum", np.full((n, rows, cols), top, dt)
    alt = np.zeros((n, rows, cols), dt)
    alt[:, :, 1::2] = top
    yield "alternating", alt


def source_shapes(scale):
    """(5, 9) and (7, 67) as source sizes where a block fits and as output sizes with the
    largest remainders; an output of (2 t_r + 3, 4 t_c + 5) for the tile (t_r, t_c): more than
    one workgroup either way, a partial tile, a partial lane, both remainders"""
    tr, tc = _lib.pool_tile()
    shapes = [(r, c) for r, c in ((5, 9), (7, 67)) if r >= scale and c >= scale]
    shapes += [(scale * r + scale - 1, scale * c + scale - 1)
               for r, c in ((5, 9), (7, 67), (2 * tr + 3, 4 * tc + 5))]
    return shapes


@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("scale", ALL_SCALES)
def test_pool_device_equals_the_restatement(gpu, scale, dt):
    for i, (rows, cols) in enumerate(source_shapes(scale)):
        for n in (2, 3):
            for name, s in inputs(n, rows, cols, dt, seed=11 * scale + n + i):
                src = dev(s)
                got = gpu.pool(src, scale)
                want = pool_ref(s, scale)
                assert tuple(got.shape) == want.shape == (n, rows // scale, cols // scale)
                same(as_unsigned(host(got), dt), want, "%s %dx%d n=%d" % (name, rows, cols, n))
                same(as_unsigned(host(src), dt), s, "the source was written")
                if name == "maximum":
                    assert (want == np.iinfo(dt).max).all()


def padded(s, pitch):
    """the stack on the device as a view with a row pitch of `pitch` elements (>= cols): rows
    and planes a whole number of dwords apart when pitch is a multiple of 4, the base torch's"""
    import torch
    n, rows, cols = s.shape
    dtype = torch.uint8 if s.dtype == np.uint8 else torch.int16
    buf = torch.zeros((n, rows, pitch), dtype=dtype, device="cuda")
    view = buf[:, :, :cols]
    view.copy_(dev(s))
    return view


@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("scale", ALL_SCALES)
def test_pool_aligned_frames_run_the_dword_kernel(gpu, scale, dt):
    """what an aligned frame runs (every instantiated scale): the dword-load kernel, with the
    vector store (bits 3) and with element stores (bits 1), over two tiles and a part of a third
    in x, two in y, a partial lane at the right edge and both remainders"""
    import torch
    tr, tc = _lib.pool_tile()
    ran = set()
    prows = tr + 3
    for pcols, out_pitch in ((2 * tc + 8, None),       # dense, whole lanes: vector stores
                             (2 * tc + 6, 2 * tc + 8),  # a partial lane into an aligned view
                             (2 * tc + 7, None)):      # dense, odd: element stores
        rows, cols = scale * prows + scale - 1, scale * pcols + scale - 1
        for n in (2, 3):
            for name, s in inputs(n, rows, cols, dt, seed=5 * scale + n + pcols):
                src = padded(s, (cols + 3) // 4 * 4 + 4)
                out = None
                if out_pitch:
                    out = torch.zeros((n, prows, out_pitch), dtype=src.dtype,
                                      device="cuda")[:, :, :pcols]
                else:
                    out = torch.zeros((n, prows, pcols), dtype=src.dtype, device="cuda")
                bits = gpu.pool_kernel(src, out)
                assert bits == expect_kernel(src, out) and bits & 1, (pcols, out_pitch, bits)
                ran.add(bits)
                got = gpu.pool(src, scale, out=out)
                assert got is out
                same(as_unsigned(host(out.contiguous()), dt), pool_ref(s, scale),
                     "%s pcols=%d n=%d bits=%d" % (name, pcols, n, bits))
                if out_pitch:
                    assert not host(out._base[:, :, pcols:]).any(), "written past the row's end"
    assert ran == {1, 3}, "both stores of the dword-load kernel"


def test_pool_out_is_returned_as_given(gpu):
    import torch
    s = random_stack(3, 12, 40, np.uint8, seed=5)
    out = torch.zeros((3, 4, 13), dtype=torch.uint8, device="cuda")
    got = gpu.pool(dev(s), 3, out=out)
    assert got is out
    same(host(out), pool_ref(s, 3))
    with pytest.raises(ValueError, match="out must be"):
        gpu.pool(dev(s), 3, out=torch.zeros((3, 4, 12), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out must be"):
        gpu.pool(dev(s), 3, out=torch.zeros((3, 4, 13), dtype=torch.int16, device="cuda"))
    with pytest.raises(_lib.BicosError, match="overlaps"):
        flat = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        gpu.pool(flat[:1440].view(3, 12, 40), 3, out=flat[100:256].view(3, 4, 13))


# ------------------------------------------------------------------------- views
def view_pitches(H, W, residue):
    """(row pitch, plane pitch) in elements: the row pitch the smallest >= W + 3 with this
    residue mod 4, the plane pitch H rows plus `residue` elements"""
    rp = W + 3
    while rp % 4 != residue:
        rp += 1
    return rp, H * rp + residue


def expect_kernel(view, out):
    """the documented selection rule (bicos_pool_kernel): bit 0, the dword-load kernel, for a
    source whose base and two pitches are multiples of 4 bytes; bit 1, vector stores, likewise
    for the output"""
    isz = view.element_size()
    bits = 0
    for bit, t in ((1, view), (2, out)):
        if all(v % 4 == 0 for v in (t.data_ptr(), t.stride(0) * isz, t.stride(1) * isz)):
            bits |= bit
    return bits


def pool_into_views(gpu, s, scale, src_geo, dst_geo, guard):
    """gpu.pool of a view of `s` into a view of a guarded buffer -> (result, wide): the input
    buffer unchanged, the output buffer changed in its pixels alone"""
    n, H, W = s.shape
    ph, pw = H // scale, W // scale
    (sb, sr), (db, dr) = src_geo, dst_geo
    rp, pp = view_pitches(H, W, sr)
    sbuf, sview = V.stack_view(s, sb, rp, pp, guard, seed=3)
    snap = sbuf.clone()
    drp, dpp = view_pitches(ph, pw, dr)
    dbuf, dview = V.stack_view(np.zeros((n, ph, pw), s.dtype), db, drp, dpp, guard, seed=4)
    before = host(dbuf).copy()
    wide = gpu.pool_kernel(sview, dview)
    assert wide == expect_kernel(sview, dview), (src_geo, dst_geo)
    got = gpu.pool(sview, scale, out=dview)
    assert got is dview
    res = host(dview.contiguous())
    assert V.unchanged(sbuf, snap), "the source buffer (view or guards) was written"
    off = (dview.data_ptr() - dbuf.data_ptr()) // dview.element_size()
    pix = V.pixel_mask(dbuf.numel(), off, (n, ph, pw), (dpp, drp, 1))
    after = host(dbuf)
    assert np.array_equal(after[~pix], before[~pix]), \
        "a guard byte around or between the output's rows and planes was written"
    return res, wide


@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("scale", ALL_SCALES)
def test_pool_views_bases_pitches_and_guards(gpu, scale, dt):
    """source and destination at every base residue 0..3 and pitch residue 0..3 (elements), at
    every instantiated scale: identical to the dense call, guards intact, and both kernels
    taken, the dword-load kernel with either store"""
    n, H, W = 3, 17, 83
    s = random_stack(n, H, W, dt, seed=77 + scale, maxval=np.iinfo(dt).max)
    want = pool_ref(s, scale)
    same(as_unsigned(host(gpu.pool(dev(s), scale)), dt), want, "dense")
    geos = [(b, r) for b in range(4) for r in range(4)]
    ran = set()
    # the same residues on both sides, then each side against an aligned other side
    pairs = [(g, g) for g in geos] + [(g, (0, 0)) for g in geos[1:]] + \
        [((0, 0), g) for g in geos[1:]]
    for src_geo, dst_geo in pairs:
        results = []
        for guard in ("random", "ones"):
            res, wide = pool_into_views(gpu, s, scale, src_geo, dst_geo, guard)
            same(as_unsigned(res, dt), want, "views %r -> %r (%s)" % (src_geo, dst_geo, guard))
            results.append(res)
            ran.add(wide)
    assert ran == {0, 1, 2, 3}, \
        "the views must reach the per-element kernel and the dword-load kernel with either store"


# ------------------------------------------------------------- host and pybicos
@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_pool_host_and_pybicos_equal_the_device_path(gpu, dt):
    import ctypes
    import pybicos
    n, H, W = 3, 21, 150
    s = random_stack(n, H, W, dt, seed=9, maxval=np.iinfo(dt).max)
    for scale in (2, 3, 8):
        want = as_unsigned(host(gpu.pool(dev(s), scale)), dt)
        same(want, pool_ref(s, scale))
        same(pybicos.pool_stack(list(s), scale), want, "pybicos.pool_stack (list)")
        same(pybicos.pool_stack(s, scale), want, "pybicos.pool_stack (array)")
        # bicos_pool_host on images with steps of their own, guards around the output rows
        wide = np.full((n, H, W + 5), 7, dt)
        wide[:, :, :W] = s
        ph, pw = H // scale, W // scale
        out = np.full((n, ph, pw + 3), 9, dt)
        src = (ctypes.c_void_p * n)(*[wide[t].ctypes.data for t in range(n)])
        dst = (ctypes.c_void_p * n)(*[out[t].ctypes.data for t in range(n)])
        rc = gpu._L.bicos_pool_host(gpu._h, src, n, H, W, (W + 5) * s.itemsize, s.itemsize, scale,
                                    dst, (pw + 3) * s.itemsize)
        _lib.check(rc, "bicos_pool_host")
        same(np.ascontiguousarray(out[:, :, :pw]), want, "bicos_pool_host")
        assert (out[:, :, pw:] == 9).all(), "bicos_pool_host wrote between the output rows"


# ---------------------------------------------------------------- pyramid match
PYRAMID_CASES = {
    "n8_u8": dict(n=8, dt=np.uint8, cfg=dict(nxcorr_threshold=0.9)),
    "n33_u16_subpixel_minvar": dict(n=33, dt=np.uint16, cfg=dict(
        nxcorr_threshold=0.9, subpixel_step=0.25, min_variance=2.0)),
    "n40_consistency": dict(n=40, dt=np.uint8, cfg=dict(nxcorr_threshold=0.9, variant=1,
                                                        max_lr_diff=1)),
    "n33_u8_raw_int16_coarse": dict(n=33, dt=np.uint8, cfg=dict(nxcorr_threshold=None)),
}
ROWS, COLS = 24, 160


@functools.lru_cache(maxsize=None)
def stacks(n, dt):
    return stereo_stack(n, ROWS, COLS, dt)


def four_calls(gpu, L, R, kw, scale, radius, spread, fallback):
    """the definition: pool, ranged coarse match without a subpixel step, guide, guided match,
    one public call after the other -> (disparity, corrmap, coarse, guide, counts)"""
    import torch
    from libbicos_amd.device import MatchConfig
    rows, cols = L.shape[1], L.shape[2]
    p0, p1 = gpu.pool(L, scale), gpu.pool(R, scale)
    assert p0.is_contiguous() and tuple(p0.shape) == (L.shape[0], rows // scale, cols // scale)
    coarse_kw = dict(kw, subpixel_step=None)
    coarse, none = gpu.match(p0, p1, MatchConfig(
        disparity_range=pyramid_window_ref(WINDOW[0], WINDOW[1], scale), **coarse_kw),
        want_corrmap=False)
    assert none is None
    counts = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    fb = (max(WINDOW[0], -32767), min(WINDOW[1], 32767)) if fallback is None else fallback
    guide = gpu.guide_from_disparity(coarse, radius, spread, scale, fb, shape=(rows, cols),
                                     sentinel=True, counts=counts)
    d, c = gpu.match(L, R, MatchConfig(disparity_range=WINDOW, **kw), guide=guide)
    return d, c, coarse, guide, counts


def check_identity(gpu, L, R, kw, scale, radius=2, spread=1, fallback=None):
    import torch
    from libbicos_amd.device import MatchConfig
    d, c, coarse, guide, counts = four_calls(gpu, L, R, kw, scale, radius, spread, fallback)
    pc = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    res = gpu.match_pyramid(L, R, MatchConfig(disparity_range=WINDOW, **kw), scale=scale,
                            radius=radius, spread=spread, fallback=fallback, return_guide=True,
                            return_coarse=True, counts=pc)
    pd, pcorr, pguide, pcoarse = res
    same(host(pd), host(d), "disparity")
    if c is None:
        assert pcorr is None
    else:
        same(host(pcorr), host(c), "corrmap")
    same(host(pcoarse), host(coarse), "coarse map")
    same(host(pguide), host(guide), "guide")
    same(host(pc), host(counts), "counts")
    # ... and the same maps when the coarse map and the guide stay inside the engine
    qd, qcorr = gpu.match_pyramid(L, R, MatchConfig(disparity_range=WINDOW, **kw), scale=scale,
                                  radius=radius, spread=spread, fallback=fallback)
    same(host(qd), host(d), "disparity (nothing returned)")
    if c is not None:
        same(host(qcorr), host(c), "corrmap (nothing returned)")
    return host(pd), host(pguide), host(pc).view(np.uint32), host(pcoarse)


@pytest.mark.parametrize("scale", [2, 3])
@pytest.mark.parametrize("name", list(PYRAMID_CASES))
def test_match_pyramid_is_its_four_calls(gpu, name, scale):
    import torch
    case = PYRAMID_CASES[name]
    L, R = stacks(case["n"], case["dt"])
    d, guide, counts, coarse = check_identity(gpu, dev(L), dev(R), case["cfg"], scale)
    want_dtype = np.int16 if case["cfg"]["nxcorr_threshold"] is None else np.float32
    assert coarse.dtype == want_dtype and coarse.shape == (ROWS // scale, COLS // scale)
    # (this scene's disparity changes from row to row, so a pooled row mixes two of them and
    # the coarse map may keep little; test_match_pyramid_is_not_a_no_op has a scene it keeps)
    assert int(counts[0]) + int(counts[1]) == ROWS * COLS
    torch.cuda.synchronize()


def test_match_pyramid_on_strided_stacks(gpu):
    case = PYRAMID_CASES["n8_u8"]
    L, R = stacks(case["n"], case["dt"])
    rp, pp = view_pitches(ROWS, COLS, 1)
    _, lv = V.stack_view(L, 1, rp, pp, "random", seed=1)
    _, rv = V.stack_view(R, 1, rp, pp, "random", seed=2)
    assert not lv.is_contiguous() and lv.stride() == rv.stride()
    d, _, _, _ = check_identity(gpu, lv, rv, case["cfg"], 2)
    dense, _, _, _ = check_identity(gpu, dev(L), dev(R), case["cfg"], 2)
    same(d, dense, "strided against dense")


@pytest.mark.parametrize("name", ["n8_u8", "n33_u16_subpixel_minvar", "n40_consistency"])
def test_pybicos_match_pyramid_equals_the_device_path(gpu, name):
    import pybicos
    import torch
    from libbicos_amd.device import MatchConfig
    case = PYRAMID_CASES[name]
    kw = case["cfg"]
    L, R = stacks(case["n"], case["dt"])
    cfg = pybicos.Config()
    cfg.nxcorr_threshold = kw["nxcorr_threshold"]
    cfg.subpixel_step = kw.get("subpixel_step")
    cfg.min_variance = kw.get("min_variance")
    if kw.get("variant"):
        cfg.set_consistency(kw["max_lr_diff"], kw.get("no_dupes", False))
    cfg.disparity_range = WINDOW
    for scale, radius, spread, fallback in ((2, 2, 1, None), (3, 1, 0, (1, 0))):
        hd, hc, stats = pybicos.match_pyramid(list(L), list(R), cfg, scale=scale, radius=radius,
                                              spread=spread, fallback=fallback)
        counts = torch.zeros((2,), dtype=torch.int32, device="cuda")
        d, c = gpu.match_pyramid(dev(L), dev(R), MatchConfig(disparity_range=WINDOW, **kw),
                                 scale=scale, radius=radius, spread=spread, fallback=fallback,
                                 counts=counts)
        same(hd, host(d), "disparity")
        same(hc, host(c), "corrmap")
        got = host(counts).view(np.uint32)
        assert stats == dict(from_prior=int(got[0]), fallback=int(got[1]))


def test_match_pyramid_is_not_a_no_op(gpu):
    """one disparity, 16, in every row, so the stacks pooled by 2 match at 8 and the coarse map
    is valid -- but for a textureless band, which has no coarse disparity: with the fallback
    pair (1, 0), "do not search", the fine map is invalid wherever the guide fell back, and
    valid elsewhere in places"""
    L, R = (a.copy() for a in stereo_stack(8, ROWS, COLS, np.uint8, dmin=16, drange=0))
    L[:, :, 96:136] = 7
    R[:, :, 96:136] = 7
    kw = dict(nxcorr_threshold=0.9)
    d, guide, counts, coarse = check_identity(gpu, dev(L), dev(R), kw, 2, radius=2, spread=1,
                                              fallback=(1, 0))
    assert int(counts[0]) > 0 and int(counts[1]) > 0
    assert int(counts[0]) + int(counts[1]) == ROWS * COLS
    fell_back = (guide[..., 0] == 1) & (guide[..., 1] == 0)
    assert int(fell_back.sum()) == int(counts[1])
    assert (coarse == np.float32(-32768.0)).any(), "the coarse map has invalid pixels"
    invalid = d == np.float32(-32768.0)
    assert invalid[fell_back].all(), "a pixel without a window was searched"
    assert not invalid[~fell_back].all(), "nothing was found anywhere"
    # with the global window as the fallback those pixels are searched again
    d2, _, counts2, _ = check_identity(gpu, dev(L), dev(R), kw, 2, radius=2, spread=1)
    assert (counts2 == counts).all()
    assert (d2 == d)[~fell_back].all(), "the fallback pair reaches only the pixels that fell back"


def test_a_pyramid_call_disturbs_nothing_on_its_engine():
    """match_plan and the unguided, ranged and guided matches give the same bytes before and
    after pyramid calls on one engine of their own"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no ROCm GPU")
    from libbicos_amd import device
    from libbicos_amd.device import MatchConfig
    eng = device.Engine(0)
    guide = torch.empty((ROWS, COLS, 2), dtype=torch.int16, device="cuda")
    guide[..., 0] = 10
    guide[..., 1] = 50

    def snapshot():
        out = []
        for case in PYRAMID_CASES.values():
            L, R = (dev(a) for a in stacks(case["n"], case["dt"]))
            kw = case["cfg"]
            out.append(eng.plan(L, R, MatchConfig(**kw)))
            for cfg, g in ((MatchConfig(**kw), None),
                           (MatchConfig(disparity_range=WINDOW, **kw), None),
                           (MatchConfig(disparity_range=WINDOW, **kw), guide)):
                d, c = eng.match(L, R, cfg, guide=g)
                out.append(host(d).tobytes())
                out.append(None if c is None else host(c).tobytes())
        return out

    before = snapshot()
    for case in PYRAMID_CASES.values():
        L, R = (dev(a) for a in stacks(case["n"], case["dt"]))
        for scale in (2, 4):
            eng.match_pyramid(L, R, MatchConfig(disparity_range=WINDOW, **case["cfg"]), scale=scale)
    assert snapshot() == before
    eng.close()
