"""Stack pooling and the pyramid match without a GPU (include/bicos_c.h, "stack pooling" and
"pyramid match"): the numpy restatement of the pooling that tests/test_pool_gpu.py holds the
kernels to, against answers written out by hand; the new C-ABI symbols and their argument
checks (BICOS_E_ARG before any HIP call); the coarse window's arithmetic; the Python validation.
"""
import ctypes

import numpy as np
import pytest

from libbicos_amd import _lib

POOL_SYMBOLS = ("bicos_pool_device", "bicos_pool_host", "bicos_pool_tile",
                "bicos_match_device_pyramid", "bicos_match_host_pyramid")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
SCALES = (2, 3, 4, 5, 6, 7, 8)


# ---------------------------------------------------------------- the restatement
def pool_ref(stack, scale):
    """bicos_pool_* in numpy: [n, rows, cols] uint8 / uint16 -> [n, rows // s, cols // s], each
    pixel (sum of its s x s block + s*s // 2) // (s*s) in uint32; the remainder rows and columns
    are dropped unread."""
    a = np.asarray(stack)
    assert a.ndim == 3 and a.dtype in (np.uint8, np.uint16) and 2 <= scale <= 8
    n, rows, cols = a.shape
    s, pr, pc = scale, rows // scale, cols // scale
    assert pr >= 1 and pc >= 1
    blocks = a[:, :pr * s, :pc * s].astype(np.uint32).reshape(n, pr, s, pc, s)
    total = blocks.sum(axis=(2, 4), dtype=np.uint32)
    return ((total + np.uint32(s * s // 2)) // np.uint32(s * s)).astype(a.dtype)


def pyramid_window_ref(lo, hi, scale):
    """[floor(lo / scale), ceil(hi / scale)] in Python's unbounded integers"""
    return lo // scale, -((-hi) // scale)


# ------------------------------------------------- answers written out by hand
@pytest.mark.parametrize("block,want", [([0, 1, 1, 1], 1),   # (3 + 2) // 4
                                        ([0, 0, 1, 1], 1),   # a half rounds up
                                        ([0, 0, 0, 1], 0),
                                        ([255, 255, 255, 254], 255),
                                        ([1, 2, 3, 4], 3)])  # 2.5 -> 3
def test_two_by_two_blocks(block, want):
    for dt in (np.uint8, np.uint16):
        a = np.array(block, dt).reshape(1, 2, 2)
        assert pool_ref(a, 2).tolist() == [[[want]]]


@pytest.mark.parametrize("scale", SCALES)
def test_the_maximum_stays_the_maximum(scale):
    for dt in (np.uint8, np.uint16):
        top = np.iinfo(dt).max
        a = np.full((2, 2 * scale + 1, 3 * scale + 1), top, dt)
        got = pool_ref(a, scale)
        assert got.shape == (2, 2, 3) and got.dtype == dt and (got == top).all()
    # the largest sum there is: 64 * 65535 fits uint32 with the rounding term
    assert 64 * 65535 + 32 < 2 ** 32


def test_five_by_seven_at_scale_2_and_3_leaves_the_remainders_unread():
    a = np.arange(35, dtype=np.uint8).reshape(1, 5, 7)
    # s = 2: blocks {0,1,7,8} = 16 -> 18 // 4, {2,3,9,10} = 24 -> 26 // 4, ... ; row 4 and
    # column 6 belong to no block
    want2 = [[[4, 6, 8], [18, 20, 22]]]
    assert pool_ref(a, 2).tolist() == want2
    # s = 3: {0,1,2,7,8,9,14,15,16} = 72 -> 76 // 9 = 8, {3,4,5,10,11,12,17,18,19} = 99 ->
    # 103 // 9 = 11; rows 3, 4 and column 6 belong to no block
    want3 = [[[8, 11]]]
    assert pool_ref(a, 3).tolist() == want3
    b = a.copy()
    b[:, 4, :] = 255
    b[:, :, 6] = 255
    assert pool_ref(b, 2).tolist() == want2
    c = a.copy()
    c[:, 3:, :] = 255
    c[:, :, 6] = 255
    assert pool_ref(c, 3).tolist() == want3


def test_the_restatement_is_not_numpys_truncating_mean():
    a = np.array([[[0, 1], [1, 1]]], np.uint8)  # mean 0.75: truncates to 0, rounds to 1
    trunc = a.reshape(1, 1, 2, 1, 2).mean(axis=(2, 4)).astype(np.uint8)
    assert trunc.tolist() == [[[0]]] and pool_ref(a, 2).tolist() == [[[1]]]


# ------------------------------------------------------------- the coarse window
WINDOWS = [((0, 63), 2, (0, 32)), ((0, 63), 3, (0, 21)), ((-5, 5), 2, (-3, 3)),
           ((-63, 63), 4, (-16, 16)), ((-7, -1), 4, (-2, 0)), ((1, 7), 8, (0, 1)),
           ((-8, 8), 8, (-1, 1)), ((-9, 9), 8, (-2, 2)),
           ((INT_MIN, INT_MAX), 2, (-2 ** 30, 2 ** 30)),
           ((INT_MIN, INT_MAX), 3, (-715827883, 715827883)),
           ((INT_MIN, INT_MIN), 8, (-2 ** 28, -2 ** 28)),
           ((INT_MAX, INT_MAX), 8, (2 ** 28 - 1, 2 ** 28))]


@pytest.mark.parametrize("rng,scale,want", WINDOWS)
def test_coarse_window_arithmetic(blib, rng, scale, want):
    assert pyramid_window_ref(rng[0], rng[1], scale) == want
    assert _lib.pyramid_window(rng, scale) == want
    lo, hi = ctypes.c_int(7), ctypes.c_int(7)
    assert blib.bicos_pyramid_window(rng[0], rng[1], scale, ctypes.byref(lo), ctypes.byref(hi)) == 0
    assert (lo.value, hi.value) == want


def test_coarse_window_refuses_a_bad_scale(blib):
    lo, hi = ctypes.c_int(0), ctypes.c_int(0)
    for s in (1, 9, 0, -2):
        assert blib.bicos_pyramid_window(0, 9, s, ctypes.byref(lo), ctypes.byref(hi)) == \
            _lib.BICOS_E_ARG
        assert "scale" in blib.bicos_last_error().decode()


# --------------------------------------------------------------------- C-ABI
def test_pool_symbols_are_exported_and_declared(blib):
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "bicos_c.h")).read()
    for s in POOL_SYMBOLS + ("bicos_pool_kernel", "bicos_pyramid_window"):
        assert hasattr(blib, s), s
        assert s in _lib.EXPORTS, s
        assert ("int %s(" % s) in header, s
    assert "stack pooling" in header and "pyramid match" in header
    assert "round" in header and "half up" in header


def test_pool_tile_and_kernel_selection(blib):
    tr, tc = _lib.pool_tile()
    assert tr >= 1 and tc >= 4 and tc % 4 == 0
    # the documented rule: bit 0, the dword-load kernel, for a source whose base and two pitches
    # are multiples of 4 bytes; bit 1, vector stores, likewise for the output
    assert blib.bicos_pool_kernel(64, 16, 160, 1, 128, 8, 40) == 3
    assert blib.bicos_pool_kernel(64, 6, 60, 2, 128, 2, 10) == 3
    for args, want in (((65, 16, 160, 1, 128, 8, 40), 2), ((64, 17, 160, 1, 128, 8, 40), 2),
                       ((64, 16, 161, 1, 128, 8, 40), 2), ((64, 16, 160, 1, 130, 8, 40), 1),
                       ((64, 16, 160, 1, 128, 9, 40), 1), ((64, 16, 160, 1, 128, 8, 42), 1),
                       ((66, 6, 60, 2, 128, 2, 10), 2), ((64, 7, 60, 2, 128, 2, 10), 2),
                       ((64, 6, 60, 2, 128, 3, 10), 1), ((64, 6, 60, 2, 128, 2, 11), 1),
                       ((65, 17, 161, 1, 129, 9, 41), 0)):
        assert blib.bicos_pool_kernel(*args) == want, args


def test_pool_device_argument_errors_come_before_any_hip_call(blib):
    src = np.zeros(4 * 16 * 32 + 64, np.uint8)
    dst = np.zeros(4 * 8 * 16 + 64, np.uint8)
    S, D = src.ctypes.data, dst.ctypes.data

    def call(src=S, n=4, rows=16, cols=32, srp=32, spp=512, depth=1, scale=2, dst=D, drp=16,
             dpp=128):
        rc = blib.bicos_pool_device(None, src, n, rows, cols, srp, spp, depth, scale, dst, drp,
                                    dpp, None)
        return rc, blib.bicos_last_error().decode()

    for kw, word in ((dict(n=0), "at least one"), (dict(n=-3), "at least one"),
                     (dict(depth=0), "depth"), (dict(depth=4), "depth"),
                     (dict(scale=1), "scale"), (dict(scale=9), "scale"), (dict(scale=0), "scale"),
                     (dict(rows=1), "smaller than scale"), (dict(cols=1), "smaller than scale"),
                     (dict(rows=7, scale=8), "smaller than scale"), (dict(rows=-1), "smaller"),
                     (dict(srp=31), "source pitch"), (dict(spp=31), "source pitch"),
                     (dict(drp=15), "output pitch"), (dict(dpp=15), "output pitch"),
                     (dict(src=None), "null source"), (dict(dst=None), "null output"),
                     (dict(depth=2, src=S + 1), "2-byte aligned"),
                     (dict(depth=2, dst=D + 1), "2-byte aligned"),
                     (dict(dst=S), "overlaps"), (dict(dst=S + 100), "overlaps"),
                     (dict(src=D + 17), "overlaps"),
                     (dict(rows=2 ** 16 + 1, srp=2 ** 16), "2^32"),
                     (dict(rows=2 ** 17 + 2, srp=32, drp=2 ** 16), "2^32")):
        rc, msg = call(**kw)
        assert rc == _lib.BICOS_E_ARG, (kw, rc, msg)
        assert word in msg, (kw, msg)


def test_pool_host_argument_errors_come_before_any_hip_call(blib):
    imgs = [np.zeros((16, 32), np.uint16) for _ in range(3)]
    outs = [np.zeros((8, 16), np.uint16) for _ in range(3)]
    PP = ctypes.c_void_p * 3

    def call(src=None, dst=None, n=3, rows=16, cols=32, sstep=0, depth=2, scale=2, dstep=0,
             null_src=False, null_dst=False):
        s = PP(*[im.ctypes.data for im in imgs]) if src is None else src
        d = PP(*[im.ctypes.data for im in outs]) if dst is None else dst
        rc = blib.bicos_pool_host(None, None if null_src else s, n, rows, cols, sstep, depth,
                                  scale, None if null_dst else d, dstep)
        return rc, blib.bicos_last_error().decode()

    one_null = PP(imgs[0].ctypes.data, None, imgs[2].ctypes.data)
    for kw, word in ((dict(n=0), "at least one"), (dict(depth=3), "depth"),
                     (dict(scale=1), "scale"), (dict(scale=9), "scale"),
                     (dict(rows=1), "smaller than scale"), (dict(cols=1), "smaller than scale"),
                     (dict(sstep=63), "multiple"), (dict(dstep=33), "multiple"),
                     (dict(sstep=62), "source pitch"), (dict(dstep=30), "output pitch"),
                     (dict(null_src=True), "null"), (dict(null_dst=True), "null"),
                     (dict(src=one_null), "null source"), (dict(dst=one_null), "null output"),
                     (dict(rows=2 ** 17, sstep=2 ** 17), "2^32")):
        rc, msg = call(**kw)
        assert rc == _lib.BICOS_E_ARG, (kw, rc, msg)
        assert word in msg, (kw, msg)


def _pyramid_calls(blib, **kw):
    """both pyramid entries with no GPU: NULL engine, host buffers standing for every pointer
    (an error must come before anything is dereferenced)"""
    a = dict(n=8, rows=16, cols=64, rp=64, pp=1024, step=0, depth=1, has_nxcorr=1, lo=0, hi=31,
             scale=2, radius=2, spread=1, flo=0, fhi=31, null_cfg=False, null_stack=False,
             null_disp=False, guide_off=0, thr=0.5, sub=-1.0)
    a.update(kw)
    n = max(a["n"], 1)
    buf = np.zeros(16, np.int32)
    p = buf.ctypes.data
    cfg = _lib.BicosConfig(a["thr"], a["sub"], -1.0, 0, 0, 0, 1, 0)
    c = None if a["null_cfg"] else ctypes.byref(cfg)
    s = None if a["null_stack"] else p
    disp = None if a["null_disp"] else p
    guide = p + a["guide_off"] if a["guide_off"] else None
    yield "device", blib.bicos_match_device_pyramid(
        None, s, s, a["n"], a["rows"], a["cols"], a["rp"], a["pp"], a["depth"], c,
        a["has_nxcorr"], a["lo"], a["hi"], a["scale"], a["radius"], a["spread"], a["flo"],
        a["fhi"], disp, None, None, guide, None, None), blib.bicos_last_error().decode()
    lists = None if a["null_stack"] else (ctypes.c_void_p * n)(*([p] * n))
    yield "host", blib.bicos_match_host_pyramid(
        None, lists, lists, a["n"], a["rows"], a["cols"], a["step"], a["depth"], c,
        a["has_nxcorr"], a["lo"], a["hi"], a["scale"], a["radius"], a["spread"], a["flo"],
        a["fhi"], disp, None, None, guide, None), blib.bicos_last_error().decode()


PYRAMID_ERRORS = [
    (dict(null_cfg=True), "null config"), (dict(lo=5, hi=4), "disparity range"),
    (dict(scale=1), "scale"), (dict(scale=9), "scale"),
    (dict(rows=1), "smaller than scale"), (dict(cols=3, scale=4, rp=3, pp=48), "smaller than scale"),
    (dict(depth=3), "depth"), (dict(n=0), "at least one"), (dict(n=1), "at least two"),
    (dict(radius=-1), "radius"), (dict(radius=32768), "radius"), (dict(spread=8), "spread"),
    (dict(spread=-1), "spread"), (dict(flo=-32769), "fallback"), (dict(fhi=32768), "fallback"),
    (dict(null_stack=True), "null"), (dict(null_disp=True), "null buffer"),
    (dict(guide_off=2), "aligned"), (dict(sub=0.0), "subpixel_step"),
    (dict(cols=32768, rp=32768, pp=16 * 32768), "32767"),
]


@pytest.mark.parametrize("kw,word", PYRAMID_ERRORS)
def test_pyramid_argument_errors_come_before_any_hip_call(blib, kw, word):
    for name, rc, msg in _pyramid_calls(blib, **kw):
        assert rc == _lib.BICOS_E_ARG, (name, kw, rc, msg)
        assert word in msg, (name, kw, msg)


def test_pyramid_device_only_argument_errors(blib):
    for kw, word in ((dict(rp=63), "pitch"), (dict(pp=63), "pitch"), (dict(pp=1023), "pitch")):
        name, rc, msg = next(_pyramid_calls(blib, **kw))
        assert rc == _lib.BICOS_E_ARG and word in msg, (kw, rc, msg)
    # the host entry's step, in bytes
    for kw, word in ((dict(depth=2, step=129), "multiple"), (dict(step=63), "smaller than a row")):
        name, rc, msg = list(_pyramid_calls(blib, **kw))[1]
        assert rc == _lib.BICOS_E_ARG and word in msg, (kw, rc, msg)


def test_pyramid_too_many_images_is_a_bits_error(blib):
    for name, rc, msg in _pyramid_calls(blib, n=70):
        assert rc == _lib.BICOS_E_BITS and "too large" in msg, (name, rc, msg)


def test_pyramid_valid_arguments_get_as_far_as_the_engine(blib):
    """every bound of the window is legal, INT_MIN / INT_MAX included, and lo > hi in the
    fallback pair means "do not search": the device entry then asks for its engine"""
    for kw in (dict(), dict(lo=INT_MIN, hi=INT_MAX), dict(lo=-40, hi=-3), dict(flo=1, fhi=0),
               dict(scale=8, rows=8, cols=8, rp=8, pp=64), dict(has_nxcorr=0), dict(sub=0.25),
               dict(rows=17, cols=67, rp=80, pp=17 * 80, scale=3)):
        name, rc, msg = next(_pyramid_calls(blib, **kw))
        assert rc == _lib.BICOS_E_ARG and msg == "null engine", (kw, rc, msg)


# -------------------------------------------------------------------- Python
def test_python_validation_raises(blib):
    assert [_lib.pool_scale(s) for s in SCALES] == list(SCALES)
    for bad in (1, 9, 0, -2, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="scale"):
            _lib.pool_scale(bad)
    assert _lib.pool_shape(5, 7, 2) == (2, 3) and _lib.pool_shape(8, 8, 8) == (1, 1)
    for rows, cols in ((1, 9), (9, 1), (0, 0)):
        with pytest.raises(ValueError, match="smaller"):
            _lib.pool_shape(rows, cols, 2)
    assert _lib.pyramid_params((0, 63)) == ((0, 63), 2, 2, 1, 0, 63)
    assert _lib.pyramid_params((-40000, 40000), 4, 0, 0) == ((-40000, 40000), 4, 0, 0, -32767, 32767)
    assert _lib.pyramid_params((0, 63), 3, 5, 7, (1, 0)) == ((0, 63), 3, 5, 7, 1, 0)
    for bad in (dict(disparity_range=None), dict(disparity_range=(5, 4)),
                dict(disparity_range=(0, 9), scale=1), dict(disparity_range=(0, 9), scale=9),
                dict(disparity_range=(0, 9), radius=-1), dict(disparity_range=(0, 9), spread=8),
                dict(disparity_range=(0, 9), fallback=(0, 40000)),
                dict(disparity_range=(0, 9), fallback=3)):
        with pytest.raises(ValueError):
            _lib.pyramid_params(**bad)


def test_pybicos_validation_runs_before_any_device_call(blib):
    from libbicos_amd import pybicos
    imgs = [np.zeros((8, 16), np.uint8)] * 4
    for bad in (1, 9, 2.5):
        with pytest.raises(ValueError, match="scale"):
            pybicos.pool_stack(imgs, bad)
    with pytest.raises(ValueError, match="Empty"):
        pybicos.pool_stack([], 2)
    with pytest.raises(ValueError, match="uint8 or uint16"):
        pybicos.pool_stack([np.zeros((8, 16), np.float32)], 2)
    with pytest.raises(ValueError, match="share size"):
        pybicos.pool_stack([np.zeros((8, 16), np.uint8), np.zeros((8, 15), np.uint8)], 2)
    with pytest.raises(ValueError, match="smaller"):
        pybicos.pool_stack([np.zeros((3, 16), np.uint8)], 4)
    cfg = pybicos.Config()
    with pytest.raises(ValueError, match="disparity_range"):
        pybicos.match_pyramid(imgs, imgs, cfg)
    with pytest.raises(ValueError, match="disparity_range"):
        pybicos.match_pyramid(imgs, imgs, None)
    cfg.disparity_range = (0, 7)
    with pytest.raises(ValueError, match="scale"):
        pybicos.match_pyramid(imgs, imgs, cfg, scale=1)
    with pytest.raises(ValueError, match="radius"):
        pybicos.match_pyramid(imgs, imgs, cfg, radius=-1)
    with pytest.raises(ValueError, match="share"):
        pybicos.match_pyramid(imgs, imgs[:3], cfg)
    with pytest.raises(ValueError, match="smaller"):
        pybicos.match_pyramid([np.zeros((2, 16), np.uint8)] * 4,
                              [np.zeros((2, 16), np.uint8)] * 4, cfg, scale=4)
    import pybicos as alias
    assert alias.pool_stack is pybicos.pool_stack and alias.match_pyramid is pybicos.match_pyramid


def test_engine_validation_runs_before_any_device_call(blib):
    """Engine.pool and Engine.match_pyramid check their parameters before they look at a
    tensor or the engine: no GPU is needed to be refused"""
    import torch
    from libbicos_amd import device
    t = torch.zeros((4, 8, 16), dtype=torch.uint8)
    for bad in (1, 9, 2.5, None):
        with pytest.raises(ValueError, match="scale"):
            device.Engine.pool(None, t, bad)
    with pytest.raises(ValueError, match="CUDA/HIP"):
        device.Engine.pool(None, t, 2)
    with pytest.raises(ValueError, match="disparity_range"):
        device.Engine.match_pyramid(None, t, t, device.MatchConfig())
    cfg = device.MatchConfig(disparity_range=(0, 7))
    with pytest.raises(ValueError, match="scale"):
        device.Engine.match_pyramid(None, t, t, cfg, scale=9)
    with pytest.raises(ValueError, match="spread"):
        device.Engine.match_pyramid(None, t, t, cfg, spread=8)
    with pytest.raises(ValueError, match="fallback"):
        device.Engine.match_pyramid(None, t, t, cfg, fallback=(0, 70000))
    with pytest.raises(ValueError, match="CUDA/HIP"):
        device.Engine.match_pyramid(None, t, t, cfg)
